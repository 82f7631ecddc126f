"""Wall time of one classifier's SPAA sweep at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240, ResNet-18
with synthetic weights; stealth_losses x d_threshes = 3 x 4 configs, 10 targeted + 1 untargeted samples each, 50 iterations), two ways
in the same process: as the reference's driver makes it (24 spaa() calls: B = 10 targeted and B = 1 untargeted per config) and as one
spaa_sweep.  Each whole sweep is bracketed by a device synchronise, after one warm-up sweep of each kind.  Prints one JSON line with
the timings of every run and, per config, the two ways' outcomes: which samples were attacked successfully (a recorded best image)
and the mean camera-side L2 / dE2000 of cam_infer_best against the scene.

    python tools/time_sweep.py [--runs 3] [--max-batch 64]
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
from spaa_amd.differential_color_functions import rgb2lab_diff, ciede2000_diff  # noqa: E402
from spaa_amd import projector_based_attack as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--max-batch', type=int, default=64)
    args = ap.parse_args()
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    cam_sz, prj_sz = (240, 320), (256, 256)
    sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    clf = Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0))
    setup = dict(classifier_crop_sz=(240, 240), prj_brightness=0.5, prj_im_sz=prj_sz)
    scene = syn.scenes(1, 1, cam_sz)[0].to(dev)
    with torch.no_grad():
        true_idx = int(clf(scene, (240, 240))[0][0].argmax())
    tgt = list(syn.IMAGENET10_TARGETS)
    configs = [c for loss in ('caml2', 'camdE', 'camdE_caml2') for d in (5, 7, 9, 11)
               for c in ((loss, d, True, tgt), (loss, d, False, [true_idx]))]

    def by_calls():
        return [A.spaa(pc, clf, None, t, tg, scene, d, loss, dev, setup) for loss, d, tg, t in configs]

    def by_sweep():
        return A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, max_batch=args.max_batch)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    by_calls()   # warm-up: engines, plans, graphs' first captures
    by_sweep()
    runs, res_calls, res_sweep = [], None, None
    for _ in range(args.runs):
        tc, res_calls = timed(by_calls)
        ts, res_sweep = timed(by_sweep)
        runs.append(dict(spaa_calls_s=round(tc, 4), sweep_s=round(ts, 4), speedup=round(tc / ts, 3)))

    def outcome(cam, prj):
        succ = [bool(v) for v in (prj != 0.5).flatten(1).any(1).cpu()]   # x_best is written only where an iteration succeeded
        sc = scene[None].expand(cam.shape[0], -1, -1, -1).contiguous()
        l2 = float(torch.norm(cam - sc, dim=1).mean())
        de = float(ciede2000_diff(rgb2lab_diff(cam.contiguous()), rgb2lab_diff(sc)).mean())
        return succ, l2, de

    per_cfg = []
    for (loss, d, tg, t), rc, rs in zip(configs, res_calls, res_sweep):
        sc_, l2c, dec = outcome(*rc)
        ss_, l2s, des = outcome(*rs)
        per_cfg.append(dict(loss=loss, d_thr=d, targeted=tg, n=len(t), succ_calls=sum(sc_), succ_sweep=sum(ss_),
                            succ_differ=sum(a != b for a, b in zip(sc_, ss_)), l2_calls=round(l2c, 6), l2_sweep=round(l2s, 6),
                            dE_calls=round(dec, 5), dE_sweep=round(des, 5)))
    sp = [r['speedup'] for r in runs]
    print(json.dumps(dict(tool='time_sweep', geometry=dict(prj=prj_sz, cam=cam_sz, crop=240, classifier='resnet18 (synthetic)',
                                                              configs=len(configs), samples=sum(len(c[3]) for c in configs), iters=50,
                                                              max_batch=args.max_batch),
                          device=torch.cuda.get_device_name(0), runs=runs, speedup_median=sorted(sp)[len(sp) // 2],
                          speedup_min=min(sp), speedup_max=max(sp),
                          succ_differ_total=sum(c['succ_differ'] for c in per_cfg), configs=per_cfg)))


if __name__ == '__main__':
    main()
