"""Wall time of the projector One-pixel DE attacker (spaa_amd.ProjectorOnePixelAttacker with a PCNet as the capture) for one
classifier's eleven attacks of run_projector_based_attack (projector_based_attack.py:110-131 in the reference): 256 x 256 projector
and camera, pixel_size 41, 4 generations, one untargeted attack with popsize 50 and ten targeted ones with popsize 10, on one RNG
stream.  The callback's verdict is ignored so that every generation runs.  ResNet-18 at 224 with synthetic weights.

    python tools/time_onepixel_projector.py [--repeat 3] [--out profiles/onepixel_projector_time.jsonl]

  fast      SimulatedCapture + Classifier(sort_results=False): spaa_onepixel_warp -> PCNetEngine.forward_from_xw ->
            spaa_capture_preproc -> body -> spaa_onepixel_score, batched
  foreign   the same capture as a plain callable with a sorting classifier: pcnet.forward and classifier(...) per candidate, as the
            reference drives a projector and a camera.  This is the baseline (the parent commit cannot run this attack at all).
  kernels   spaa_onepixel_warp (with and without cat8) and spaa_capture_preproc on their own at P = 50, against their bytes at the
            8 TB/s HBM rate DESIGN.md uses.

One warm-up run per route builds the engines; each timed run is one JSON line (appended to --out as well); a last line per route
gives median / min / max."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spaa_amd import _lib  # noqa: E402
from spaa_amd import one_pixel_attacker as opa  # noqa: E402
from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.classifier import Classifier, IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from spaa_amd.models import PCNet, WarpingNet, C_ptr  # noqa: E402

HBM = 8e12
SZ, CROP, TEN = (256, 256), (240, 240), [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]


def every_generation():
    """DE with the callback's return value dropped: a success does not end the attack."""
    real = opa.DifferentialEvolution

    def de(*a, callback=None, **k):
        def cb(x, convergence):
            callback(x, convergence)
        return real(*a, callback=cb, **k)
    opa.DifferentialEvolution = de


def eleven(att, clf, true_idx):
    np.random.seed(0)
    nfev = classified = 0
    for targeted, t, popsize in [(False, true_idx, 50)] + [(True, t, 10) for t in TEN]:
        att(att.im_prj_org, clf, targeted, target_idx=t, pixel_count=1, pixel_size=41, maxiter=4, popsize=popsize)
        nfev += int(att.last_result.nfev)
        classified += int(att.last_result.get('classified', att.last_result.nfev))
    return nfev, classified


def time_kernel(fn, launches=20, repeats=7):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / launches)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'onepixel_projector_time.jsonl'))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    every_generation()
    sd = syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect')
    pc = PCNet(sd['mask'], WarpingNet(out_size=SZ))
    pc.load_state_dict(sd)
    pc = pc.to('cuda')
    csd = syn.resnet18_state_dict(5, logit_gain=20.0)
    scene = syn.scenes(3, 1, SZ)[0]
    labels = {i: f'class{i}' for i in range(1000)}
    info = dict(prj_im_sz=SZ, prj_brightness=0.5, cam_im_sz=SZ, classifier_crop_sz=CROP)
    medians = {}
    for route, sort in (('fast', False), ('foreign', True)):
        clf = Classifier('resnet18', 'cuda', state_dict=csd, sort_results=sort)
        att = opa.ProjectorOnePixelAttacker(labels, info, capture=opa.SimulatedCapture(pc, scene))
        att.im_prj_org, att.im_cam_org = 0.5 * torch.ones(3, *SZ), scene
        true_idx = int(clf(scene, CROP)[0][0].argmax())
        secs = []
        for rep in range(args.repeat + 1):      # the first run builds the engines
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nfev, classified = eleven(att, clf, true_idx)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                secs.append(dt)
                emit(kind='attacks', route=route, run=rep, seconds=round(dt, 4), nfev=nfev, classified=classified,
                     ms_per_classified=round(1e3 * dt / classified, 3))
        medians[route] = statistics.median(secs)
        emit(kind='attacks_summary', route=route, runs=len(secs), median_s=round(medians[route], 4), min_s=round(min(secs), 4),
             max_s=round(max(secs), 4))
    emit(kind='ratio', foreign_over_fast=round(medians['foreign'] / medians['fast'], 2))

    # the two kernels on their own at P = 50
    P, (H, W) = 50, SZ
    eng = pc.engine(P, SZ)
    base = torch.zeros(1, H, W, 4, device='cuda')
    base[..., :3] = 127 / 255
    rng = np.random.default_rng(0)
    cand = np.stack([rng.integers(20, H - 20, P), rng.integers(20, W - 20, P), *(rng.integers(0, 256, P) for _ in range(3))], 1)
    cand = torch.from_numpy(cand.astype(np.int32)).to('cuda')
    s4 = torch.rand(H, W, 4, device='cuda')
    xw, cat8 = torch.zeros(P, H, W, 4, device='cuda'), torch.zeros(P, H, W, 8, device='cuda')
    y, pre = torch.rand(P, H, W, 4, device='cuda'), torch.zeros(P, 224, 224, 4, device='cuda')
    mean, std = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)

    def warp(c8):
        return lambda: _lib.call('spaa_onepixel_warp', _lib.ptr(base), _lib.ptr(cand), P, 1, 41, C_ptr(eng.tap_src), _lib.ptr(eng.tap_wm),
                                 _lib.ptr(s4), _lib.ptr(xw), _lib.ptr(cat8) if c8 else None, H, W, H, W)

    def preproc(q):
        return lambda: _lib.call('spaa_capture_preproc', _lib.ptr(y), _lib.ptr(pre), P, H, W, 8, 8, 240, 240, 224, 224, mean, std, q)

    table = H * W * 32 + H * W * 16
    for name, fn, nbytes in (('spaa_onepixel_warp', warp(False), P * H * W * 16 + table),
                             ('spaa_onepixel_warp+cat8', warp(True), P * H * W * 48 + table + H * W * 16),
                             ('spaa_capture_preproc', preproc(1), P * (240 * 240 + 224 * 224) * 16),
                             ('spaa_capture_preproc(quantize=0)', preproc(0), P * (240 * 240 + 224 * 224) * 16)):
        us = time_kernel(fn)
        med = statistics.median(us)
        emit(kind='kernel', name=name, P=P, bytes=nbytes, median_us=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
             us_at_hbm_rate=round(nbytes / HBM * 1e6, 2), tb_per_s=round(nbytes / med * 1e-6, 2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
