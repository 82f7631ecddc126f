"""Wall time and added device time of the ViT's attention-weighted attack (spaa_sweep(attention=Attention(0.25, rollout=True));
DESIGN.md 7m) against the plain one at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240; vit_b_16 at its
full size: 224 x 224, 197 tokens, 12 layers; the 11 attacks of one (stealth loss, d_thr) point: 10 targeted + 1 untargeted samples,
50 iterations), on the same PCNet and scene, in one process:

  * the plain attack and the attack with the rollout: the median of --runs wall times, each bracketed by a device synchronise, after
    one warm-up of each kind;
  * the device time of the new launches (spaa_attn_relevance: 12 per iteration, two kernels each; spaa_relevance_map;
    spaa_attention_apply) per iteration, from HIP events around each launch over --profile-iters eager iterations of an AttackState,
    next to spaa_attn_bwd's and the sum over all launches of an iteration with and without attention;
  * per kind the success counts and the mean caml2 (x 255) / camdE.

--plain-only times the plain attack alone and uses nothing this feature added, so that the same file runs against an older tree
(--root: where spaa_amd is imported from); its record goes to --out as well and is handed to the full run with --parent-json, which
stores it under `parent_plain`.

PCNet and the classifier are RANDOM-INIT (spaa_amd.synthetic): the outcome numbers say that the path runs, not what trained networks
give; the record says so.  Appends one JSON line to --out and prints it.

    python tools/time_vit_relevance.py [--runs 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/vit_relevance_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

LAUNCHES = ('spaa_attn_relevance', 'spaa_relevance_map', 'spaa_attention_apply', 'spaa_attn_bwd')


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--profile-iters', type=int, default=5)
    ap.add_argument('--floor', type=float, default=0.25)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--root', default=here)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=os.path.join(here, 'profiles', 'vit_relevance_time.jsonl'))
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
    clf = Classifier('vit_b_16', dev, state_dict=syn.vit_b_16_state_dict(logit_gain=4.0))
    setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
    scene = syn.scenes(1, 1, cam_sz)[0].to(dev)
    with torch.no_grad():
        true_idx = int(clf(scene, crop)[0][0].argmax())
    tgt = list(syn.IMAGENET10_TARGETS)
    configs = [(args.loss, args.d_thr, True, tgt), (args.loss, args.d_thr, False, [true_idx])]
    kinds_att = {'plain': None}
    if not args.plain_only:
        kinds_att['rollout'] = A.Attention(args.floor, rollout=True)

    def attack(attention):
        kw = {} if attention is None else dict(attention=attention)
        (ct, _), (cu, _) = A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, iters=args.iters, **kw)
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
    B = len(all_t)
    launches = {}
    for name, att in kinds_att.items():
        kw = {} if att is None else dict(attention=att)
        st = A.AttackState(pc, clf, all_t, scene, args.loss, setup, dev, **kw)
        st.iteration(all_tg, args.d_thr, 2, 1, 0.9)
        _lib.PROFILE = []
        for _ in range(args.profile_iters):
            st.iteration(all_tg, args.d_thr, 2, 1, 0.9)
        torch.cuda.synchronize()
        prof, _lib.PROFILE = _lib.PROFILE, None
        per, count = {n: 0.0 for n in LAUNCHES}, {n: 0 for n in LAUNCHES}
        total = 0.0
        for entry, e0, e1 in prof:
            ms = e0.elapsed_time(e1)
            total += ms
            if entry in per:
                per[entry] += ms
                count[entry] += 1
        launches[name] = dict({n + '_us': round(per[n] * 1e3 / args.profile_iters, 2) for n in LAUNCHES},
                              calls_per_iteration={n: count[n] // args.profile_iters for n in LAUNCHES},
                              all_launches_us=round(total * 1e3 / args.profile_iters, 1), launches_per_iteration=len(prof) // args.profile_iters)
        del st
    added = {name: round(launches[name]['all_launches_us'] - launches['plain']['all_launches_us'], 1) for name in launches if name != 'plain'}

    outcome = {}
    scene_b = scene[None].expand(B, -1, -1, -1).contiguous()
    for name, cams in last.items():
        ok = A.attack_transfer(cams, [clf], all_t, all_tg, crop)[:, 0]
        caml2, camdE, _ = stealth_loss_with_grad(cams, scene_b)
        outcome[name] = dict(success_targeted=int(ok[:len(tgt)].sum()), success_untargeted=int(ok[len(tgt):].sum()),
                             caml2_x255_mean=round(float(caml2.mean()) * 255, 4), camdE_mean=round(float(camdE.mean()), 4))

    rec = dict(tool='time_vit_relevance', tree='parent (plain only)' if args.plain_only else 'this commit',
               weights='random-init (spaa_amd.synthetic): the outcome numbers say that the path runs, not what trained networks give',
               geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], classifier='vit_b_16', tokens=197, layers=12, samples=B, iters=args.iters,
                             loss=args.loss, d_thr=args.d_thr, floor=args.floor),
               device=torch.cuda.get_device_name(0), graph=graphs, runs=runs, wall_s_median={name: med(name + '_s') for name in kinds},
               launch_device_time_per_iteration=dict(how=f'HIP events around each launch, mean of {args.profile_iters} eager iterations',
                                                     added_all_launches_us=added, **launches),
               outcome=outcome)
    if args.parent_json:
        with open(args.parent_json) as fh:
            parent = json.loads(fh.read().strip().splitlines()[-1])
        rec['parent_plain'] = dict(wall_s_median=parent['wall_s_median'], runs=parent['runs'],
                                   all_launches_us=parent['launch_device_time_per_iteration']['plain']['all_launches_us'])
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
