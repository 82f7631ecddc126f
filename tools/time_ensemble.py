"""Wall time and outcome of one (stealth loss, d_thr) point of the attack driver's grid at the reference's geometry (projector
256 x 256, camera 240 x 320, crop 240; ResNet-18, VGG-16 and Inception-v3 at their full input sizes; 10 targeted + 1 untargeted
samples, 50 iterations) two ways on the same PCNet and scene, in one process:

  * ONE ensemble attack of the three bodies (spaa_sweep with a list of classifiers), with `focus` off and on;
  * the three single-classifier attacks of the same 11 samples, one after the other.

Each is bracketed by a device synchronise, after one warm-up of each kind.  For the ensemble runs and for each single attack it also
records how many of the 11 inferred camera images fool ALL three members (attack_transfer: top-1 == target for the targeted samples,
top-1 != the attacked label for the untargeted one).  PCNet and the classifiers are RANDOM-INIT (spaa_amd.synthetic), so the counts
say how the loop behaves, not how real networks transfer; the record says so.  Appends one JSON line to --out and prints it.

    python tools/time_ensemble.py [--runs 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/ensemble_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.models import PCNet, WarpingNet  # noqa: E402
from spaa_amd.classifier import Classifier  # noqa: E402
from spaa_amd import projector_based_attack as A  # noqa: E402

MEMBERS = ('inception_v3', 'resnet18', 'vgg16')   # the driver's default order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensemble_time.jsonl'))
    args = ap.parse_args()
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
    sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    weights = dict(inception_v3=lambda: syn.inception_v3_state_dict(4, logit_gain=20.0),
                   resnet18=lambda: syn.resnet18_state_dict(2, logit_gain=20.0), vgg16=lambda: syn.vgg16_state_dict(3, logit_gain=5.0))
    clfs = [Classifier(n, dev, state_dict=weights[n]()) for n in MEMBERS]
    print('weights generated', file=sys.stderr, flush=True)
    setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
    scene = syn.scenes(1, 1, cam_sz)[0].to(dev)
    with torch.no_grad():
        scene_top1 = [int(c(scene, crop)[0][0].argmax()) for c in clfs]
    tgt = list(syn.IMAGENET10_TARGETS)

    def configs(true_idx):
        return [(args.loss, args.d_thr, True, tgt), (args.loss, args.d_thr, False, [true_idx])]

    def attack(classifier, true_idx, **kw):
        (ct, _), (cu, _) = A.spaa_sweep(pc, classifier, None, scene, setup, dev, configs(true_idx), iters=args.iters, **kw)
        return torch.cat((ct, cu))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def fooled_all(cams, true_idx):
        got = A.attack_transfer(cams, clfs, tgt + [true_idx], [True] * len(tgt) + [False], crop)
        return dict(fooled_all=int(got.all(axis=1).sum()), fooled_per_member=[int(v) for v in got.sum(axis=0)])

    kinds = {'ensemble': lambda: attack(clfs, scene_top1[0]), 'ensemble_focus': lambda: attack(clfs, scene_top1[0], focus=True),
             'singles': lambda: [attack(c, t) for c, t in zip(clfs, scene_top1)]}
    for name, fn in kinds.items():   # warm-up: engines, plans, the graphs' first captures
        fn()
        print(f'warm-up {name} done', file=sys.stderr, flush=True)
    graphs = {}
    runs, last = [], {}
    for _ in range(args.runs):
        row = {}
        for name, fn in kinds.items():
            row[name + '_s'], last[name] = timed(fn)
            graphs[name] = A.LAST_RUN['graph']
            row[name + '_s'] = round(row[name + '_s'], 4)
        row['ensemble_over_singles'] = round(row['ensemble_s'] / row['singles_s'], 3)
        runs.append(row)
        print(row, file=sys.stderr, flush=True)
    outcome = dict(ensemble=fooled_all(last['ensemble'], scene_top1[0]), ensemble_focus=fooled_all(last['ensemble_focus'], scene_top1[0]))
    for n, cams, t in zip(MEMBERS, last['singles'], scene_top1):
        outcome['single_' + n] = fooled_all(cams, t)
    med = lambda k: sorted(r[k] for r in runs)[len(runs) // 2]   # noqa: E731
    rec = dict(tool='time_ensemble', weights='random-init (spaa_amd.synthetic): the counts describe the loop, not real networks',
               geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], members=MEMBERS, samples=len(tgt) + 1, iters=args.iters,
                             loss=args.loss, d_thr=args.d_thr),
               device=torch.cuda.get_device_name(0), scene_top1=dict(zip(MEMBERS, scene_top1)), graph=graphs, runs=runs,
               ensemble_s_median=med('ensemble_s'), ensemble_focus_s_median=med('ensemble_focus_s'), singles_s_median=med('singles_s'),
               ensemble_over_singles_median=med('ensemble_over_singles'), of_samples=len(tgt) + 1, outcome=outcome)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
