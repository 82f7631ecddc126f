"""Wall time, added device time and outcome of the attention-weighted attack (spaa_sweep(attention=...)) against the plain one at the
reference's geometry (projector 256 x 256, camera 240 x 320, crop 240; ResNet-18 at its full input size; the 11 attacks of one
(stealth loss, d_thr) point: 10 targeted + 1 untargeted samples, 50 iterations), on the same PCNet and scene, in one process:

  * the plain attack and the attack with Attention(0.0) and Attention(0.25): the median of --runs wall times, each bracketed by a
    device synchronise, after one warm-up of each kind;
  * the device time of the new launches (spaa_cam_map, spaa_attention_apply; spaa_cam_alpha does not run for a global-average head)
    per iteration, from HIP events around each launch over --profile-iters eager iterations of an AttackState, and the sum over all
    launches of an iteration with and without attention;
  * per kind: the share of the camera perturbation energy |cam_infer_best - scene|^2 that lies where the classifier looks (M >= 0.5,
    M = Classifier.grad_cam of the result for the sample's class), the success counts and the mean caml2 (x 255) / camdE.

PCNet and the classifier are RANDOM-INIT (spaa_amd.synthetic): the outcome numbers say how the loop behaves, not what trained networks
give; the record says so.  Appends one JSON line to --out and prints it.

    python tools/time_attention.py [--runs 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/attention_time.jsonl]
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
from spaa_amd.differential_color_functions import stealth_loss_with_grad  # noqa: E402

FLOORS = (0.0, 0.25)
LAUNCHES = ('spaa_cam_alpha', 'spaa_cam_map', 'spaa_attention_apply')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--profile-iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attention_time.jsonl'))
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
    kinds_att = {'plain': None}
    kinds_att.update({f'attention{f:g}': A.Attention(f) for f in FLOORS})

    def attack(attention):
        (ct, _), (cu, _) = A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, iters=args.iters, attention=attention)
        return torch.cat((ct, cu))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    kinds = {name: (lambda a=a: attack(a)) for name, a in kinds_att.items()}
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

    # device time: HIP events around every launch of eager iterations (after one unrecorded iteration), with and without attention
    all_t, all_tg = tgt + [true_idx], [True] * len(tgt) + [False]
    launches = {}
    for name, att in kinds_att.items():
        st = A.AttackState(pc, clf, all_t, scene, args.loss, setup, dev, attention=att)
        st.iteration(all_tg, args.d_thr, 2, 1, 0.9)
        _lib.PROFILE = []
        for _ in range(args.profile_iters):
            st.iteration(all_tg, args.d_thr, 2, 1, 0.9)
        torch.cuda.synchronize()
        prof, _lib.PROFILE = _lib.PROFILE, None
        per = {n: 0.0 for n in LAUNCHES}
        total = 0.0
        for entry, e0, e1 in prof:
            ms = e0.elapsed_time(e1)
            total += ms
            if entry in per:
                per[entry] += ms
        launches[name] = dict({n + '_us': round(per[n] * 1e3 / args.profile_iters, 2) for n in LAUNCHES},
                              all_launches_us=round(total * 1e3 / args.profile_iters, 1), launches_per_iteration=len(prof) // args.profile_iters)
        del st
    B, (H, W) = len(all_t), cam_sz
    added = {name: round(launches[name]['all_launches_us'] - launches['plain']['all_launches_us'], 1) for name in launches if name != 'plain'}

    # where the perturbation went, and what it bought
    outcome = {}
    scene_b = scene[None].expand(B, -1, -1, -1).contiguous()
    for name, cams in last.items():
        M = clf.grad_cam(cams, all_t, crop)[:, 0]
        e = ((cams - scene_b) ** 2).sum(dim=1)
        share = (e * (M >= 0.5)).flatten(1).sum(dim=1) / e.flatten(1).sum(dim=1).clamp_min(1e-30)
        area = (M >= 0.5).float().flatten(1).mean(dim=1)
        ok = A.attack_transfer(cams, [clf], all_t, all_tg, crop)[:, 0]
        caml2, camdE, _ = stealth_loss_with_grad(cams, scene_b)
        outcome[name] = dict(energy_share_where_M_ge_half=round(float(share.mean()), 4), area_share_where_M_ge_half=round(float(area.mean()), 4),
                             success_targeted=int(ok[:len(tgt)].sum()), success_untargeted=int(ok[len(tgt):].sum()),
                             caml2_x255_mean=round(float(caml2.mean()) * 255, 4), camdE_mean=round(float(camdE.mean()), 4),
                             energy_share_per_image=[round(float(v), 3) for v in share])

    rec = dict(tool='time_attention', weights='random-init (spaa_amd.synthetic): the outcome numbers describe the loop, not trained networks',
               geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], classifier='resnet18', samples=B, iters=args.iters, loss=args.loss,
                             d_thr=args.d_thr),
               device=torch.cuda.get_device_name(0), graph=graphs, runs=runs, wall_s_median={name: med(name + '_s') for name in kinds},
               launch_device_time_per_iteration=dict(how=f'HIP events around each launch, mean of {args.profile_iters} eager iterations',
                                                     apply_bytes=B * H * W * 32, added_all_launches_us=added, **launches),
               outcome=outcome)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
