"""Device time of the ConvNeXt-Tiny body (spaa_amd/convnext.py) and its depthwise 7 x 7 kernels (csrc/convnext_ops.hip), in one process:

  (a) spaa_dwconv7_fwd / spaa_dwconv7_bwd alone at B = 64 on the four stage shapes (56 x 56 x 96, 28 x 28 x 192, 14 x 14 x 384,
      7 x 7 x 768), under each of the kernel's two forms (spaa_dwconv7_form: 1 strips of 4 columns and runs of >= 7 rows, 2 strips of 2
      and runs of >= 4) and under the library's own choice (0), the forms alternating at each shape: HIP events around --inner launches in a row, the median of --reps such windows after one unrecorded window.  The
      launches of a window rotate over enough buffer sets that their working set exceeds CACHE_BYTES (the 256 MB last-level cache),
      so the bytes come from HBM and not from what the previous launch left in cache.  Each time is given as algorithmic bytes / time
      (input + output, + `add` for the backward pass; the 196 bytes of weights per channel are left out) against the 8 TB/s the
      project quotes for HBM, and as FLOPs / time (2 x 49 per element) against 157 TFLOP/s of fp32 vector arithmetic.  The layer has
      12.25 FLOP/B forward (8.2 backward with add) against a ridge of 19.6: its roof is the memory one.
  (b) one forward + backward pass of the body at B = 64, 224 x 224: the sum of the eager launch times (HIP events around every launch)
      per kernel family -- depthwise, LayerNorm, GELU, the tap-list convolution launches, everything else (patch gather, pools) --
      with each family's share and ResNet-18's total next to it;
  (c) the 11 attacks of one (stealth loss, d_thr) point at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240, 50
      iterations) with convnext_tiny and, alternating with it, with ResNet-18: the median of --runs wall times, each bracketed by a
      device synchronise, after a warm-up of each.

There is no pass mark: the body is new and has no parent to be compared with.  The networks are RANDOM-INIT (spaa_amd.synthetic): the
attack outcomes of (c) say only that the path runs.  Appends one JSON line to --out and prints it.

    python tools/time_convnext.py [--reps 7] [--inner 10] [--runs 3] [--out profiles/convnext_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12
FP32_VECTOR_FLOPS = 157e12
CACHE_BYTES = 256e6
STAGES = ((56, 56, 96), (28, 28, 192), (14, 14, 384), (7, 7, 768))
FAMILIES = {'spaa_dwconv7_fwd': 'depthwise', 'spaa_dwconv7_bwd': 'depthwise', 'spaa_layernorm_fwd': 'layernorm',
            'spaa_layernorm_bwd': 'layernorm', 'spaa_gelu_fwd': 'gelu', 'spaa_gelu_bwd': 'gelu', 'spaa_tapconv_f32': 'tapconv'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--skip-attack', action='store_true')
    ap.add_argument('--kernels-only', action='store_true', help='part (a) alone')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'convnext_time.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from spaa_amd import _lib, synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier, ClassifierEngine
    from spaa_amd import projector_based_attack as A

    if not torch.cuda.is_available():
        raise SystemExit('time_convnext: no GPU (a time measured anywhere else says nothing)')
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    p, B, lib = _lib.ptr, args.batch, _lib.load()
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731

    def window(launch, nset):
        """Median time of one launch: --inner launches (rotating over `nset` buffer sets) between two events."""
        turn = [0]

        def run():
            for _ in range(args.inner):
                launch(turn[0] % nset)
                turn[0] += 1
        run()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3 / args.inner)
        return med(out), min(out), max(out)

    # (a) the depthwise kernels alone
    alone = []
    for h, w, c in STAGES:
        n = B * h * w * c
        nset = max(2, int(CACHE_BYTES * 1.5 / (8 * n)) + 1)
        xs = [torch.randn(B, h, w, c, device=dev) for _ in range(nset)]
        outs = [torch.zeros(B, h, w, c, device=dev) for _ in range(nset)]
        adds = [torch.randn(B, h, w, c, device=dev) for _ in range(nset)]
        wt, bias = torch.randn(49, c, device=dev) / 7, torch.rand(c, device=dev)
        flops = 2 * 49 * n
        row = dict(shape=f'{B}x{h}x{w}x{c}', buffer_sets=nset, flops=flops)
        timed = []
        for form in (1, 2, 0):
            lib.spaa_dwconv7_form(form)
            tf = window(lambda i: _lib.call('spaa_dwconv7_fwd', p(xs[i]), p(wt), p(bias), p(outs[i]), B, h, w, c), nset)
            tb = window(lambda i: _lib.call('spaa_dwconv7_bwd', p(xs[i]), p(wt), p(adds[i]), p(outs[i]), B, h, w, c), nset)
            tn = window(lambda i: _lib.call('spaa_dwconv7_bwd', p(xs[i]), p(wt), None, p(outs[i]), B, h, w, c), nset)
            lib.spaa_dwconv7_form(0)
            timed += [(f'form{form}_fwd', tf, 8 * n), (f'form{form}_bwd_add', tb, 12 * n), (f'form{form}_bwd', tn, 8 * n)]
        for name, (t, lo, hi), nbytes in timed:
            least = max(nbytes / HBM_BYTES_PER_S, flops / FP32_VECTOR_FLOPS)
            row[name] = dict(us=round(t * 1e6, 1), us_min=round(lo * 1e6, 1), us_max=round(hi * 1e6, 1), bytes=nbytes,
                             TB_s=round(nbytes / t / 1e12, 2), share_of_8TB_s=round(nbytes / t / HBM_BYTES_PER_S, 3),
                             TFLOP_s=round(flops / t / 1e12, 1), share_of_157TFLOP_s=round(flops / t / FP32_VECTOR_FLOPS, 3),
                             least_us=round(least * 1e6, 1), bound='memory' if nbytes / HBM_BYTES_PER_S >= flops / FP32_VECTOR_FLOPS else 'fp32',
                             share_of_roof=round(least / t, 3))
        alone.append(row)
        print(row, file=sys.stderr, flush=True)
        del xs, outs, adds

    # (b) one forward + backward pass of the body, eager, per kernel family
    def body_pass(name, sd):
        eng = ClassifierEngine(name, sd, B, (240, 320), (240, 240), None, dev)
        y = torch.rand(B, 240, 320, 4, device=dev)
        g = torch.randn(B, eng.ncls, device=dev)
        eng.forward(y)
        eng.backward(g)
        torch.cuda.synchronize()
        _lib.PROFILE = []
        eng.forward(y)
        eng.backward(g)
        torch.cuda.synchronize()
        prof, _lib.PROFILE = _lib.PROFILE, None
        fam, cnt = {}, {}
        for entry, e0, e1 in prof:
            if entry.startswith('spaa_preproc'):
                continue
            k = FAMILIES.get(entry, 'other')
            fam[k] = fam.get(k, 0.0) + e0.elapsed_time(e1) * 1e3
            cnt[k] = cnt.get(k, 0) + 1
        total = sum(fam.values())
        flops = eng.body.flops_fwd()
        del eng
        return dict(launches=cnt, us={k: round(v, 1) for k, v in fam.items()}, share={k: round(v / total, 3) for k, v in fam.items()},
                    total_us=round(total, 1), fwd_gflop=round(flops / 1e9, 2))

    passes = dict(note='not measured (--kernels-only)')
    if not args.kernels_only:
        csd, rsd = syn.convnext_tiny_state_dict(8, logit_gain=4.0), syn.resnet18_state_dict(2, logit_gain=20.0)
        passes = dict(convnext_tiny=body_pass('convnext_tiny', csd), resnet18=body_pass('resnet18', rsd))
        print(passes, file=sys.stderr, flush=True)

    # (c) the 11 attacks of one (loss, d_thr) point at the reference geometry
    attack_rec = 'not measured (--skip-attack)'
    if not (args.skip_attack or args.kernels_only):
        cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
        sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
        pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
        pc.load_state_dict(sd)
        pc = pc.to(dev)
        clfs = dict(resnet18=Classifier('resnet18', dev, state_dict=rsd), convnext_tiny=Classifier('convnext_tiny', dev, state_dict=csd))
        setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
        scene = syn.scenes(1, 1, cam_sz)[0].to(dev)
        tgt = list(syn.IMAGENET10_TARGETS)

        def attack(clf):
            with torch.no_grad():
                true_idx = int(clf(scene, crop)[0][0].argmax())
            configs = [('camdE_caml2', 5, True, tgt), ('camdE_caml2', 5, False, [true_idx])]
            return A.spaa_sweep(pc, clf, None, scene, setup, dev, configs, iters=args.iters)

        runs, graphs = [], {}
        for name, clf in clfs.items():
            attack(clf)
        for _ in range(args.runs):
            row = {}
            for name, clf in clfs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                attack(clf)
                torch.cuda.synchronize()
                row[name + '_s'] = round(time.perf_counter() - t0, 4)
                graphs[name] = A.LAST_RUN['graph']
            runs.append(row)
            print(row, file=sys.stderr, flush=True)
        attack_rec = dict(geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], samples=len(tgt) + 1, iters=args.iters, loss='camdE_caml2', d_thr=5),
                          graph=graphs, runs=runs, wall_s_median={n: med([r[n + '_s'] for r in runs]) for n in clfs},
                          note='random-init weights: the outcomes say only that the path runs')

    rec = dict(tool='time_convnext', device=torch.cuda.get_device_name(0), weights='random-init (spaa_amd.synthetic)', batch=B,
               depthwise_alone=dict(how=f'HIP events around {args.inner} launches in a row rotating over buffer sets larger than '
                                        f'{CACHE_BYTES / 1e6:.0f} MB together, per launch, median (min, max) of {args.reps} windows '
                                        'after one unrecorded window',
                                    roofs=dict(hbm_bytes_per_s=HBM_BYTES_PER_S, fp32_vector_flops=FP32_VECTOR_FLOPS), layers=alone),
               forward_backward_pass=dict(how='HIP events around every launch of one eager forward + backward pass at 224 x 224 (the '
                                              'preprocessing launches left out), after one unrecorded pass', **passes),
               attack=attack_rec)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
