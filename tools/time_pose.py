"""Wall time and outcome of the pose-robust attack (spaa_sweep(pose=...)) against the plain one at the reference's geometry
(projector 256 x 256, camera 240 x 320, crop 240; ResNet-18 at its full input size; the 11 attacks of one (stealth loss, d_thr) point:
10 targeted + 1 untargeted samples, 50 iterations), on the same PCNet and scene, in one process:

  * the plain attack, the pose attack at draws = 2, 3 and 4, and the pose attack at draws = 3 with the default CaptureJitter behind
    the warp: the median of --runs wall times, the kinds alternating within each run, each bracketed by a device synchronise, after
    one warm-up of each kind;
  * the device time of the three new launches (spaa_pose_draw / _fwd / _bwd) per iteration, from HIP events around each launch over
    --profile-iters eager iterations of a PoseAttackState, per number of draws (with spaa_jitter_fwd_each in the jitter kind);
  * the mean pose_survival (32 warped captures per image) of the plain attack's inferred camera images and of each pose attack's,
    under the same PoseJitter ranges and one evaluation seed.

A J-draw iteration runs J classifier passes, as a J-member ensemble does: no ratio is promised.  PCNet and the classifier are
RANDOM-INIT (spaa_amd.synthetic), so the survival numbers say only that the loop does what it says, not how trained networks survive a
bumped camera; the record says so.  Appends one JSON line to --out and prints it.

    python tools/time_pose.py [--runs 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/pose_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spaa_amd import _lib, synthetic as syn  # noqa: E402
from spaa_amd.models import PCNet, WarpingNet  # noqa: E402
from spaa_amd.classifier import Classifier  # noqa: E402
from spaa_amd import projector_based_attack as A  # noqa: E402

DRAWS = (2, 3, 4)
LAUNCHES = ('spaa_pose_draw', 'spaa_pose_fwd', 'spaa_pose_bwd', 'spaa_jitter_fwd_each', 'spaa_jitter_bwd')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--profile-iters', type=int, default=10)
    ap.add_argument('--survival-draws', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose_time.jsonl'))
    args = ap.parse_args()
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
    sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    clf = Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0))
    setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
    scene = syn.scenes(1, 1, cam_sz)[0].to(dev)
    with torch.no_grad():
        true_idx = int(clf(scene, crop)[0][0].argmax())
    tgt = list(syn.IMAGENET10_TARGETS)
    configs = [(args.loss, args.d_thr, True, tgt), (args.loss, args.d_thr, False, [true_idx])]
    poses = {j: A.PoseJitter(draws=j, seed=args.seed) for j in DRAWS}
    jitter3 = A.CaptureJitter(draws=3, seed=args.seed)

    def attack(pose, jitter=None):
        (ct, _), (cu, _) = A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, iters=args.iters, pose=pose, jitter=jitter)
        return torch.cat((ct, cu))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    kinds = {'plain': lambda: attack(None)}
    kinds.update({f'pose{j}': (lambda j=j: attack(poses[j])) for j in DRAWS})
    kinds['pose3_jitter'] = lambda: attack(poses[3], jitter3)
    for name, fn in kinds.items():   # warm-up: engines, plans, the graphs' first captures
        fn()
        print(f'warm-up {name} done', file=sys.stderr, flush=True)
    graphs, runs, last = {}, [], {}
    for _ in range(args.runs):
        row = {}
        for name, fn in kinds.items():
            t, last[name] = timed(fn)
            graphs[name] = A.LAST_RUN['graph']
            row[name + '_s'] = round(t, 4)
        runs.append(row)
        print(row, file=sys.stderr, flush=True)
    med = lambda k: sorted(r[k] for r in runs)[len(runs) // 2]   # noqa: E731

    # device time of the new launches: HIP events around every launch of eager iterations (after one unrecorded iteration)
    launches = {}
    for name, pose, jitter in [(f'draws{j}', poses[j], None) for j in DRAWS] + [('draws3_jitter', poses[3], jitter3)]:
        st = A.PoseAttackState(pc, clf, tgt + [true_idx], scene, args.loss, setup, dev, pose, jitter=jitter)
        flags = [True] * len(tgt) + [False]
        st.iteration(flags, args.d_thr, 2, 1, 0.9)
        _lib.PROFILE = []
        for _ in range(args.profile_iters):
            st.iteration(flags, args.d_thr, 2, 1, 0.9)
        torch.cuda.synchronize()
        prof, _lib.PROFILE = _lib.PROFILE, None
        per = {n: 0.0 for n in LAUNCHES}
        total = 0.0
        for n, e0, e1 in prof:
            ms = e0.elapsed_time(e1)
            total += ms
            if n in per:
                per[n] += ms
        launches[name] = dict({n + '_us': round(per[n] * 1e3 / args.profile_iters, 2) for n in LAUNCHES if per[n]},
                              all_launches_us=round(total * 1e3 / args.profile_iters, 1))
        del st

    # how many of 32 warped captures of each inferred camera image still succeed, under the default ranges and one seed
    ev = A.PoseJitter()
    all_t, all_tg = tgt + [true_idx], [True] * len(tgt) + [False]
    survival = {}
    for name, cams in last.items():
        s = A.pose_survival(cams, clf, all_t, all_tg, crop, ev, draws=args.survival_draws, seed=12345)
        clean = A.attack_transfer(cams, [clf], all_t, all_tg, crop)[:, 0]
        survival[name] = dict(mean=round(float(s.mean()), 4), clean_success=int(clean.sum()), per_image=[round(float(v), 3) for v in s])

    rec = dict(tool='time_pose', weights='random-init (spaa_amd.synthetic): the survival numbers say only that the loop does what it '
                                         'says, not how trained networks survive a bumped camera',
               geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], classifier='resnet18', samples=len(tgt) + 1, iters=args.iters,
                             loss=args.loss, d_thr=args.d_thr),
               pose=dict(rotate=ev.rotate, zoom=ev.zoom, shift=ev.shift, tilt=ev.tilt, seed=args.seed),
               jitter=dict(gain=jitter3.gain, offset=jitter3.offset, shift=jitter3.shift, noise=jitter3.noise, quantize=jitter3.quantize),
               device=torch.cuda.get_device_name(0), graph=graphs, runs=runs,
               wall_s_median={name: med(name + '_s') for name in kinds},
               launch_device_time_per_iteration=dict(how=f'HIP events around each launch, mean of {args.profile_iters} eager iterations',
                                                     **launches),
               pose_survival=dict(draws=args.survival_draws, of_samples=len(tgt) + 1, **survival))
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
