"""Wall time and outcome of one (stealth loss, d_thr) point at the reference's geometry (projector 256 x 256, camera 240 x 320,
crop 240; ResNet-18 at its full input size; 10 targeted + 1 untargeted samples, 50 iterations) for V = 2 and V = 3 camera views of
one projector -- V PCNets with distinct warps, each with its own scene -- two ways, in one process:

  * ONE multi-view attack of the V views (spaa_sweep with a list of PCNets and a list of scenes), with `focus` off and on;
  * the V single-view attacks of the same 11 samples (spaa_sweep with one PCNet and its scene), one after the other.

Each is bracketed by a device synchronise, after one warm-up of each kind.  Every projection -- the multi-view one and each single
view's -- is then pushed through ALL V PCNets and classified, and the record holds how many of the 11 projections fool every view
(top-1 == target for the targeted samples, top-1 != the attacked label for the untargeted one) and how many fool each view: for a
single-view projection the columns of the OTHER views say what it is worth a few degrees to the side.  PCNets and the classifier are
RANDOM-INIT (spaa_amd.synthetic), so the counts say how the loop behaves, not how trained networks behave; the record says so.
No ratio is promised: a multi-view step still runs V PCNet and classifier passes.  Appends one JSON line per V to --out and prints it.

    python tools/time_multiview.py [--runs 3] [--views 2 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/multiview_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.models import PCNet, WarpingNet  # noqa: E402
from spaa_amd.classifier import Classifier  # noqa: E402
from spaa_amd import projector_based_attack as A  # noqa: E402

# view -> (PCNet seed, affine of its warp, scene seed)
VIEWS = [(0, (0.9, 0.02, 0.05, -0.03, 0.9, 0.05), 1), (3, (0.92, -0.04, -0.03, 0.05, 0.87, -0.04), 2),
         (5, (0.86, 0.05, -0.06, -0.02, 0.93, 0.03), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--views', type=int, nargs='+', default=[2, 3])
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiview_time.jsonl'))
    args = ap.parse_args()
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
    pcs, scenes = [], []
    for seed, affine, scene_seed in VIEWS:
        sd = syn.pcnet_state_dict(seed, cam_sz=cam_sz, mask='ones', affine=affine)
        pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
        pc.load_state_dict(sd)
        pcs.append(pc.to(dev))
        scenes.append(syn.scenes(scene_seed, 1, cam_sz)[0].to(dev))
    clf = Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0))
    print('weights generated', file=sys.stderr, flush=True)
    setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
    with torch.no_grad():
        scene_top1 = [int(clf(s, crop)[0][0].argmax()) for s in scenes]
    tgt = list(syn.IMAGENET10_TARGETS)
    labels, targeted = tgt + [scene_top1[0]], [True] * len(tgt) + [False]      # (the untargeted label: view 0's, for every attack)
    configs = [(args.loss, args.d_thr, True, tgt), (args.loss, args.d_thr, False, [scene_top1[0]])]

    def attack(pcnet, scene, **kw):
        """The 11 projections [11,3,Hp,Wp] of one attack (multi-view for lists)."""
        (_, pt), (_, pu) = A.spaa_sweep(pcnet, clf, None, scene, setup, dev, configs, iters=args.iters, **kw)
        return torch.cat((pt, pu))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def fooled(prj, V):
        """Which of the V views each projection fools: the projection through view v's PCNet and scene, classified."""
        with torch.no_grad():
            cols = [A.attack_transfer(pcs[v](prj, scenes[v][None].expand(prj.shape[0], -1, -1, -1).contiguous()), [clf], labels, targeted,
                                      crop)[:, 0] for v in range(V)]
        got = np.stack(cols, axis=1)                                             # [11][V]
        return dict(fooled_all=int(got.all(axis=1).sum()), fooled_per_view=[int(n) for n in got.sum(axis=0)])

    lines = []
    for V in args.views:
        views, sc = pcs[:V], scenes[:V]
        kinds = {'multiview': lambda: attack(views, sc), 'multiview_focus': lambda: attack(views, sc, focus=True),
                 'singles': lambda: [attack(p, s) for p, s in zip(views, sc)]}
        for name, fn in kinds.items():   # warm-up: engines, plans, the graphs' first captures
            fn()
            print(f'V = {V}: warm-up {name} done', file=sys.stderr, flush=True)
        graphs, runs, last = {}, [], {}
        for _ in range(args.runs):
            row = {}
            for name, fn in kinds.items():
                t, last[name] = timed(fn)
                graphs[name] = A.LAST_RUN['graph']
                row[name + '_s'] = round(t, 4)
            row['multiview_over_singles'] = round(row['multiview_s'] / row['singles_s'], 3)
            runs.append(row)
            print(row, file=sys.stderr, flush=True)
        outcome = dict(multiview=fooled(last['multiview'], V), multiview_focus=fooled(last['multiview_focus'], V))
        for v, prj in enumerate(last['singles']):
            outcome[f'single_view{v}'] = fooled(prj, V)
        med = lambda k: sorted(r[k] for r in runs)[len(runs) // 2]   # noqa: E731
        rec = dict(tool='time_multiview', weights='random-init (spaa_amd.synthetic): the counts describe the loop, not trained networks',
                   geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], classifier='resnet18', views=V, samples=len(labels),
                                 iters=args.iters, loss=args.loss, d_thr=args.d_thr),
                   device=torch.cuda.get_device_name(0), scene_top1=scene_top1[:V], graph=graphs, runs=runs,
                   multiview_s_median=med('multiview_s'), multiview_focus_s_median=med('multiview_focus_s'),
                   singles_s_median=med('singles_s'), multiview_over_singles_median=med('multiview_over_singles'),
                   of_samples=len(labels), outcome=outcome)
        lines.append(json.dumps(rec))
        print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
