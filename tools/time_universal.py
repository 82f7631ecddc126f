"""Time per iteration of the universal attack (UniversalAttackState) against the plain one (AttackState) on the same batch: B = 64
samples, each with its own scene, ResNet-18, at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240) and at the
benchmark's (256 x 256 both, crop 240), in one process:

  * the plain attack and Universal(N) for N in {2, 8, 64}: the median over --runs of the wall time of --iters eager iterations
    (bracketed by a device synchronise, after --warmup iterations of that kind), per iteration.  At these sizes spaa() itself runs the
    loop eagerly (B Hc Wc is above GRAPH_MAX_PIXELS);
  * the device time of the two new entry points per iteration, from HIP events around each launch over --profile-iters eager iterations,
    and the sum over all launches of an iteration;
  * the two entry points alone at B = 64, 256 x 256, ncls = 1000: every group on the adversarial step, and every group on the colour step.

--plain-only times the plain rows alone and touches nothing of the feature, so that it also runs on the commit before it (--root: the
checkout whose spaa_amd runs); its record carries --label.  The two plain figures should agree within the 3 % box variance of
profiles/r06_box_variance.txt: without a Universal the loop launches what it launched before.  The expectation for the universal rows
is the plain time plus the new launches (the per-sample passes are the plain attack's; the sums of squares move from the adjoint's
epilogue into spaa_grad_sumsq_ps, and the clamp gate is read from x).

PCNet and the classifier are RANDOM-INIT (spaa_amd.synthetic): the fooled counts say that the path runs, not what a universal projection
achieves -- that needs trained networks and real scenes; the record says so.  Appends one JSON line to --out and prints it.

    python tools/time_universal.py [--runs 3] [--iters 10] [--out profiles/universal_time.jsonl]
    python tools/time_universal.py --plain-only --label parent --root <checkout of the parent commit>
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('spaa_decide_universal', 'spaa_universal_combine')
SIZES = (2, 8, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--profile-iters', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--label', default='this commit')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'universal_time.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from spaa_amd import _lib, synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier
    from spaa_amd import projector_based_attack as A

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    B = args.batch
    r18 = Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0))
    targets = (list(syn.IMAGENET10_TARGETS) * ((B + 9) // 10))[:B]
    hp = dict(targeted=True, d_thr=5, adv_lr=2, col_lr=1, p_thresh=0.9)

    def timed(st):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            st.iteration(**hp)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    rec = dict(tool='time_universal', label=args.label, device=torch.cuda.get_device_name(0), batch=B, iters=args.iters, runs=args.runs,
               weights='random-init (spaa_amd.synthetic): the fooled counts say that the path runs; what a universal projection achieves '
                       'needs trained networks and real scenes',
               ms_per_iteration={}, fooled_members={}, launch_device_time_per_iteration={})
    for geometry, cam_sz in (('reference', (240, 320)), ('benchmark', (256, 256))):
        prj_sz, crop = (256, 256), (240, 240)
        sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
        pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
        pc.load_state_dict(sd)
        pc = pc.to(dev)
        setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
        scenes = syn.scenes(1, B, cam_sz)
        kinds = {'plain': lambda: A.AttackState(pc, r18, targets, scenes, args.loss, setup, dev)}
        if not args.plain_only:
            for n in SIZES:
                kinds[f'universal_{n}'] = (lambda n=n: A.UniversalAttackState(pc, r18, targets, scenes, args.loss, setup, dev, A.Universal(n)))
        ms, fooled, launches = {}, {}, {}
        for name, make in kinds.items():
            st = make()
            for _ in range(args.warmup):
                st.iteration(**hp)
            ms[name] = round(sorted(timed(st) for _ in range(args.runs))[args.runs // 2], 3)
            print(f'{geometry} {name}: {ms[name]} ms per iteration', file=sys.stderr, flush=True)
            # device time: HIP events around every launch of eager iterations
            _lib.PROFILE = []
            for _ in range(args.profile_iters):
                st.iteration(**hp)
            torch.cuda.synchronize()
            prof, _lib.PROFILE = _lib.PROFILE, None
            per, total = {n: 0.0 for n in LAUNCHES}, 0.0
            for entry, e0, e1 in prof:
                t = e0.elapsed_time(e1)
                total += t
                if entry in per:
                    per[entry] += t
            launches[name] = dict({n + '_us': round(per[n] * 1e3 / args.profile_iters, 1) for n in LAUNCHES if name != 'plain'},
                                  all_launches_us=round(total * 1e3 / args.profile_iters, 1),
                                  launches_per_iteration=len(prof) // args.profile_iters)
            if name != 'plain':   # (state[:, 3] of a group's first row: its fooled members after the iterations above)
                fooled[name] = st.state[::st.N, 3].tolist()
            del st
        rec['ms_per_iteration'][geometry] = ms
        rec['fooled_members'][geometry] = fooled
        rec['launch_device_time_per_iteration'][geometry] = launches
        del pc

    if not args.plain_only:
        # the two entry points alone at B = 64, 256 x 256: HIP events around --profile-iters calls after one unrecorded call
        Bk, HW, ncls, p = 64, 256 * 256, 1000, _lib.ptr
        nblk = HW // 256
        g = torch.randn(Bk, HW, 4, device=dev) * 1e-3
        out, partial, coef = torch.zeros_like(g), torch.zeros(Bk, nblk, device=dev), torch.zeros(Bk, device=dev)
        logits, seeds = torch.randn(Bk, ncls, device=dev), torch.zeros(Bk, ncls, device=dev)
        target, flags = torch.zeros(Bk, dtype=torch.int32, device=dev), torch.ones(Bk, dtype=torch.int32, device=dev)
        loss_partial = torch.rand(Bk, nblk, 3, device=dev)
        params = torch.tensor([[0.0, 1.0, 1.0, 5.0]] * Bk, device=dev)
        state, stats = torch.zeros(Bk, 4, dtype=torch.int32, device=dev), torch.zeros(Bk, 8, device=dev)
        us, uf, uw = torch.zeros(Bk, 2, dtype=torch.int32, device=dev), torch.zeros(Bk, 4, device=dev), torch.ones(Bk, device=dev)
        alone = {}
        for n in SIZES:
            for step in ('adversarial', 'colour'):
                per = {}
                for rep in range(args.profile_iters + 1):
                    _lib.PROFILE = [] if rep else None
                    _lib.call('spaa_decide_universal', p(logits), ncls, p(target), p(loss_partial), nblk, HW, None, p(params), p(flags), n, n,
                              0.9, 1.0 / Bk, 0, p(state), p(stats), p(us), p(uf), p(uw), p(seeds), Bk)
                    state[:, 1] = int(step == 'colour')
                    _lib.call('spaa_universal_combine', p(g), n, p(uw), p(state), p(partial), p(coef), p(out), Bk, HW)
                    torch.cuda.synchronize()
                    for entry, e0, e1 in _lib.PROFILE or []:
                        per[entry] = per.get(entry, 0.0) + e0.elapsed_time(e1)
                _lib.PROFILE = None
                alone[f'N{n}_{step}'] = {k + '_us': round(per[k] * 1e3 / args.profile_iters, 1) for k in LAUNCHES}
        rec['entry_points_alone'] = dict(B=Bk, prj=(256, 256), ncls=ncls, image_bytes=Bk * HW * 16,
                                         how=f'HIP events around each call, mean of {args.profile_iters}', **alone)

    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
