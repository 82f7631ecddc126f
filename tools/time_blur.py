"""Device time of the blur kernels, and wall time and outcome of the defocus-robust attack (spaa_sweep(blur=...)) against the plain one,
in one process:

  * at B = 64, 256 x 256, J = 3: spaa_blur_fwd and spaa_blur_bwd alone at sigmas that give the radius r = 2, 5 and 8 in every row, next
    to spaa_jitter_fwd and spaa_jitter_bwd at the same shape (they move the same images): HIP events around --reps back-to-back
    launches after a warm-up, the median of --windows such windows, the kinds alternating inside a round; with the bytes each launch
    has to move (computed from the shape) and the rate that makes;
  * at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240; ResNet-18; the 11 attacks of one (stealth loss,
    d_thr) point, 50 iterations): the plain attack and the blur attack at draws = 2, 3 and 4, the median of --runs wall times, each
    bracketed by a device synchronise, after one warm-up of each kind;
  * blur_survival of the plain attack's inferred camera images and of each blur attack's.

A J-draw iteration runs J classifier passes, as a J-member ensemble does: no ratio is promised, and no time here is a pass bar.  PCNet
and the classifier are RANDOM-INIT (spaa_amd.synthetic), so the survival numbers only show that the path runs; the record says so.
Appends one JSON line to --out and prints it.

    python tools/time_blur.py [--runs 3] [--loss camdE_caml2] [--d-thr 5] [--out profiles/blur_time.jsonl]
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
RADII = {2: (0.5, 0.66), 5: (1.4, 1.66), 8: (2.4, 2.5)}   # r -> a sigma range whose every value has ceil(3 sigma) = r


def kernel_times(B, H, W, J, reps, windows):
    """Median device time per launch [us] of the blur and jitter entry points at one shape, and the bytes each has to move."""
    dev = 'cuda:0'
    p, arr = _lib.ptr, _lib.ptr_array
    gen = torch.Generator(device=dev).manual_seed(0)
    y = torch.rand(B, H, W, 4, device=dev, generator=gen)
    ys = [y] * J
    outs = [torch.zeros_like(y) for _ in range(J)]
    grads = [torch.randn(B, H, W, 4, device=dev, generator=gen) for _ in range(J)]
    g_y = [torch.zeros_like(y) for _ in range(J)]
    gates = [torch.zeros(B, H * W, dtype=torch.uint8, device=dev) for _ in range(J)]
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    jit = torch.zeros(B, J, 8, device=dev)
    key = torch.zeros(B, J, dtype=torch.int32, device=dev)
    A.CaptureJitter(draws=J).draw(counter, jit, key, B, J, clean0=False)
    rows = {}
    for r, sigma in RADII.items():
        rows[r] = torch.zeros(B, J, 12, device=dev)
        A.CaptureBlur(sigma=sigma, draws=J).draw(counter, rows[r], B, J, clean0=False)   # (no identity row: every draw pays for the filter)
        assert (rows[r][..., 1] == r).all(), (r, rows[r][..., 1].unique())
    kinds = {'spaa_jitter_fwd': lambda: _lib.call('spaa_jitter_fwd', p(y), p(jit), p(key), J, 1, arr(outs), arr(gates), B, H, W),
             'spaa_jitter_bwd': lambda: _lib.call('spaa_jitter_bwd', arr(grads), p(jit), arr(gates), J, arr(g_y), B, H, W)}
    px = B * J * H * W
    # bytes per pixel and draw: an image read and an image written, 16 each; the jitter also a gate byte.  (The blur's halo re-reads and
    # the jitter's neighbour taps come from cache or cost extra: the rate below is of the bytes a launch HAS to move.)
    moved = {'spaa_jitter_fwd': 33 * px, 'spaa_jitter_bwd': 33 * px}
    for r in RADII:
        kinds[f'spaa_blur_fwd r={r}'] = (lambda r=r: _lib.call('spaa_blur_fwd', arr(ys), p(rows[r]), J, arr(outs), B, H, W))
        kinds[f'spaa_blur_bwd r={r}'] = (lambda r=r: _lib.call('spaa_blur_bwd', arr(grads), p(rows[r]), J, arr(g_y), B, H, W))
        moved[f'spaa_blur_fwd r={r}'] = moved[f'spaa_blur_bwd r={r}'] = 32 * px
    order = ['spaa_jitter_fwd', 'spaa_jitter_bwd'] + [k for k in kinds if k.startswith('spaa_blur_fwd')] + \
            [k for k in kinds if k.startswith('spaa_blur_bwd')]
    times = {k: [] for k in kinds}
    for w in range(windows + 1):                                          # (window 0 is the warm-up)
        for k in order:
            if k == 'spaa_jitter_bwd':
                kinds['spaa_jitter_fwd']()                                # (its gates)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                kinds[k]()
            e1.record()
            torch.cuda.synchronize()
            if w:
                times[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    out = {}
    for k in order:
        us = sorted(times[k])[len(times[k]) // 2]
        out[k] = dict(us=round(us, 1), spread_us=[round(min(times[k]), 1), round(max(times[k]), 1)], bytes=moved[k],
                      GBps=round(moved[k] / us / 1e3, 1))
    ratio = lambda a, b: round(out[a]['us'] / out[b]['us'], 2)   # noqa: E731
    out['ratio_to_jitter'] = {k: ratio(k, 'spaa_jitter_fwd' if '_fwd' in k else 'spaa_jitter_bwd') for k in order if 'blur' in k}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--loss', default='camdE_caml2')
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'blur_time.jsonl'))
    args = ap.parse_args()
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    shape = dict(B=64, H=256, W=256, J=3)
    kernels = kernel_times(**shape, reps=args.reps, windows=args.windows)
    print(kernels, file=sys.stderr, flush=True)

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
    blurs = {j: A.CaptureBlur(draws=j, seed=args.seed) for j in DRAWS}

    def attack(blur):
        (ct, _), (cu, _) = A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, iters=args.iters, blur=blur)
        return torch.cat((ct, cu))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    kinds = {'plain': lambda: attack(None)}
    kinds.update({f'blur{j}': (lambda j=j: attack(blurs[j])) for j in DRAWS})
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

    all_t, all_tg = tgt + [true_idx], [True] * len(tgt) + [False]
    sigmas = (0.5, 1.0, 1.5, 2.0, 2.5)
    survival = {}
    for name, cams in last.items():
        s = A.blur_survival(cams, clf, all_t, all_tg, crop, sigmas=sigmas)
        clean = A.attack_transfer(cams, [clf], all_t, all_tg, crop)[:, 0]
        survival[name] = dict(clean_success=int(clean.sum()), surviving_per_sigma=[int(v) for v in s.sum(axis=1)])

    ev = blurs[3]
    rec = dict(tool='time_blur', weights='random-init (spaa_amd.synthetic): the survival numbers only show that the path runs',
               device=torch.cuda.get_device_name(0),
               kernels=dict(shape=shape, radii={str(r): list(s) for r, s in RADII.items()},
                            how=f'HIP events around {args.reps} back-to-back launches, median of {args.windows} windows after a '
                                'warm-up window, kinds alternating; bytes from the shape', **kernels),
               geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], classifier='resnet18', samples=len(tgt) + 1, iters=args.iters,
                             loss=args.loss, d_thr=args.d_thr),
               blur=dict(sigma=list(ev.sigma), seed=args.seed),
               graph=graphs, runs=runs, wall_s_median={name: med(name + '_s') for name in kinds},
               blur_survival=dict(sigmas=list(sigmas), of_samples=len(tgt) + 1, **survival))
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
