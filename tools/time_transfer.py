"""Wall time, added device time and outcome of the transferable attack (spaa_sweep(transfer=...)) against the plain one at the
reference's geometry (projector 256 x 256, camera 240 x 320, crop 240; the classifiers at their full input sizes; the 11 attacks of one
(stealth loss, d_thr) point: 10 targeted + 1 untargeted samples, 50 iterations), on the same PCNet and scene, in one process:

  * ResNet-18: the plain attack, Transfer(1, 0) (momentum alone), Transfer(0, 1.5) (smoothing alone) and Transfer(1, 1.5): the median of
    --runs wall times, each bracketed by a device synchronise, after one warm-up of each kind;
  * the two-member ensemble Inception-v3 + VGG-16, plain and Transfer(1, 1.5), timed in the same way; for these rows transfer_success of
    the results on the held-out ResNet-18 (which took no part in the attack), and the mean caml2 (x 255) / camdE;
  * the device time of the new launches (spaa_transfer_blur, spaa_transfer_momentum) per iteration, from HIP events around each launch
    over --profile-iters eager iterations of an AttackState, and the sum over all launches of an iteration with and without them.
  * the two kernels alone at the benchmark's shape (B = 64, 256 x 256, every sample on the adversarial step) for r = 0, 5 and 7.

--plain-only times the plain ResNet-18 row alone and passes no `transfer` keyword at all, so that it also runs on the commit before the
feature (--root: the checkout whose spaa_amd runs); its record carries --label.  The two plain figures should agree within the 3 % box
variance of profiles/r06_box_variance.txt: without a Transfer the loop launches what it launched before.

PCNet and the classifiers are RANDOM-INIT (spaa_amd.synthetic): the held-out success count says that the path runs, not whether momentum
and smoothing buy transfer or physical robustness -- that needs trained networks and a camera; the record says so.  Appends one JSON line
to --out and prints it.

    python tools/time_transfer.py [--runs 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/transfer_time.jsonl]
    python tools/time_transfer.py --plain-only --label parent --root <checkout of the parent commit>
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('spaa_transfer_blur', 'spaa_transfer_momentum')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--profile-iters', type=int, default=10)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--label', default='this commit')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'transfer_time.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from spaa_amd import _lib, synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier
    from spaa_amd import projector_based_attack as A
    from spaa_amd.differential_color_functions import stealth_loss_with_grad

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
    sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    r18 = Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0))
    setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
    scene = syn.scenes(1, 1, cam_sz)[0].to(dev)
    with torch.no_grad():
        true_idx = int(r18(scene, crop)[0][0].argmax())
    tgt = list(syn.IMAGENET10_TARGETS)
    configs = [(args.loss, args.d_thr, True, tgt), (args.loss, args.d_thr, False, [true_idx])]
    all_t, all_tg = tgt + [true_idx], [True] * len(tgt) + [False]

    def attack(clf, **kw):
        (ct, _), (cu, _) = A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, iters=args.iters, **kw)
        return torch.cat((ct, cu))

    kinds = {'resnet18_plain': (lambda: attack(r18))}
    transfers = {}
    if not args.plain_only:
        ens = [Classifier('inception_v3', dev, state_dict=syn.inception_v3_state_dict(4, logit_gain=20.0)),
               Classifier('vgg16', dev, state_dict=syn.vgg16_state_dict(3, logit_gain=5.0))]
        transfers = {'resnet18_transfer_mu1_sigma0': A.Transfer(1.0, 0.0), 'resnet18_transfer_mu0_sigma1.5': A.Transfer(0.0, 1.5),
                     'resnet18_transfer_mu1_sigma1.5': A.Transfer(1.0, 1.5)}
        for name, tr in transfers.items():
            kinds[name] = (lambda tr=tr: attack(r18, transfer=tr))
        kinds['ensemble_plain'] = (lambda: attack(ens))
        kinds['ensemble_transfer_mu1_sigma1.5'] = (lambda: attack(ens, transfer=A.Transfer(1.0, 1.5)))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

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
    B, (Hp, Wp) = len(all_t), prj_sz
    rec = dict(tool='time_transfer', label=args.label,
               weights='random-init (spaa_amd.synthetic): the outcome numbers say that the path runs; whether momentum and smoothing buy '
                       'transfer or physical robustness needs trained networks and a camera',
               geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], samples=B, iters=args.iters, loss=args.loss, d_thr=args.d_thr),
               device=torch.cuda.get_device_name(0), graph=graphs, runs=runs, wall_s_median={name: med(name + '_s') for name in kinds})

    if not args.plain_only:
        # device time: HIP events around every launch of eager iterations (after one unrecorded iteration), with and without a Transfer
        launches = {}
        for name, tr in dict(resnet18_plain=None, **transfers).items():
            st = A.AttackState(pc, r18, all_t, scene, args.loss, setup, dev, transfer=tr)
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
        added = {name: round(launches[name]['all_launches_us'] - launches['resnet18_plain']['all_launches_us'], 1)
                 for name in launches if name != 'resnet18_plain'}
        rec['launch_device_time_per_iteration'] = dict(
            how=f'HIP events around each launch, mean of {args.profile_iters} eager iterations; a launch skips the samples on the colour step',
            image_bytes=B * Hp * Wp * 16, added_all_launches_us=added, **launches)
        # the two kernels alone at the benchmark's shape (B = 64, 256 x 256, every sample on the adversarial step): HIP events around
        # --profile-iters launches after one unrecorded launch
        Bk, p = 64, _lib.ptr
        g = torch.randn(Bk, Hp, Wp, 4, device=dev) * 1e-3
        m, t = torch.zeros_like(g), torch.zeros_like(g)
        state = torch.zeros(Bk, 4, dtype=torch.int32, device=dev)
        tiles = _lib.load().spaa_transfer_tiles(Hp, Wp)
        l1, npart = torch.zeros(Bk, tiles, device=dev), Hp * Wp // 256
        ss = torch.zeros(Bk, npart, device=dev)
        alone = {}
        for sigma in (0.0, 1.5, 7 / 3):
            tr = A.Transfer(1.0, sigma)
            w = tr.weights().tolist()
            taps = (ctypes.c_float * len(w))(*w)
            per = {}
            for rep in range(args.profile_iters + 1):
                _lib.PROFILE = [] if rep else None
                _lib.call('spaa_transfer_blur', p(g), p(state), taps, tr.radius, p(t), p(l1), Bk, Hp, Wp)
                _lib.call('spaa_transfer_momentum', p(t), p(l1), tiles, 1.0, p(state), p(m), p(g), p(ss), npart, Bk, Hp * Wp)
                torch.cuda.synchronize()
                for entry, e0, e1 in _lib.PROFILE or []:
                    per[entry] = per.get(entry, 0.0) + e0.elapsed_time(e1)
            _lib.PROFILE = None
            alone[f'r{tr.radius}'] = {n + '_us': round(per[n] * 1e3 / args.profile_iters, 1) for n in LAUNCHES}
        rec['kernels_alone_at_benchmark_shape'] = dict(B=Bk, prj=prj_sz, image_bytes=Bk * Hp * Wp * 16,
                                                       how=f'HIP events around each launch, mean of {args.profile_iters}', **alone)
        del g, m, t, l1, ss
        # what it bought: the attacked classifiers' own success, the held-out one's, and the stealth metrics
        outcome = {}
        scene_b = scene[None].expand(B, -1, -1, -1).contiguous()
        for name, cams in last.items():
            own = ens if name.startswith('ensemble') else [r18]
            ok = A.attack_transfer(cams, own, all_t, all_tg, crop).all(axis=1)
            caml2, camdE, _ = stealth_loss_with_grad(cams, scene_b)
            outcome[name] = dict(success_targeted=int(ok[:len(tgt)].sum()), success_untargeted=int(ok[len(tgt):].sum()),
                                 caml2_x255_mean=round(float(caml2.mean()) * 255, 4), camdE_mean=round(float(camdE.mean()), 4))
            if name.startswith('ensemble'):
                held = A.transfer_success(cams, r18, all_t, all_tg, crop)
                outcome[name].update(held_out='resnet18', held_out_success_targeted=int(held[:len(tgt)].sum()),
                                     held_out_success_untargeted=int(held[len(tgt):].sum()))
        rec['outcome'] = outcome

    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
