"""Device time of the ViT-B/16 body (spaa_amd/vit.py) and the kernels of csrc/vit_ops.hip, in one process, with the real widths
(D = 768, 12 layers, M = 3072, P = 16, T = 197) at B = 64, 224 x 224:

  1. each new kernel alone: HIP events around the launch, the median of --reps after one unrecorded launch.  LayerNorm and GELU as
     TB/s of algorithmic bytes (forward: input + output; LayerNorm adjoint: g + x + add + gx; GELU adjoint: g + pre + gx; the
     per-row statistics and the per-channel weights are left out) beside the 3.0 TB/s that spaa_transfer_momentum reaches (DESIGN.md
     7i: the project's yardstick for an elementwise pass); attention forward (4 T^2 D FLOPs per sample: q k^T and p v) and adjoint
     (10 T^2 D algorithmic: the scores, g . v, g_q, g_k and g_v once each; the two passes execute 14, each recomputing the scores and
     g . v) as TFLOP/s of fp32.
  2. one forward + backward pass of the body: the sum of the eager launch times (HIP events around every launch) per launch group --
     the convolution plans, attention, LayerNorm / GELU, the token bookkeeping --, the body's forward FLOPs and the share of the
     attention kernels.
  3. the 11 attacks of one (camdE_caml2, d_thr 5) point at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240,
     50 iterations) with vit_b_16 and, alternating with it, with ResNet-18: the median of --runs wall times, each bracketed by a
     device synchronise, after a warm-up of each.  The ResNet-18 figure is the one profiles/mobilenet_time.jsonl records (0.1676 s):
     that loop launches what it launched before, so it should stay inside the 3 % box variance of profiles/r06_box_variance.txt.

Nothing is tuned for these shapes: the plans run on the tiles that were measured for other layers (tapconv_tune.json is unchanged).
The networks are RANDOM-INIT (spaa_amd.synthetic).  Appends one JSON line to --out and prints it.

    python tools/time_vit.py [--reps 10] [--runs 3] [--out profiles/vit_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {'spaa_tapconv_f32': 'plans', 'spaa_linear_small': 'plans', 'spaa_attn_fwd': 'attention', 'spaa_attn_bwd': 'attention',
          'spaa_layernorm_fwd': 'layernorm_gelu', 'spaa_layernorm_bwd': 'layernorm_gelu', 'spaa_gelu_fwd': 'layernorm_gelu',
          'spaa_gelu_bwd': 'layernorm_gelu'}   # anything else: the token bookkeeping


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'vit_time.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from spaa_amd import _lib, synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier, ClassifierEngine
    from spaa_amd import projector_based_attack as A

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    p, B = _lib.ptr, args.batch
    D, M, T, H, DH = 768, 3072, 197, 12, 64
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731

    def events(fn, reps):
        fn()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return med(out)

    # 1. the kernels alone
    rows = B * T
    x, g, add, y = (torch.randn(rows, D, device=dev) for _ in range(4))
    w, b = torch.rand(D, device=dev) + 0.5, torch.rand(D, device=dev)
    mean, rstd = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
    t_lnf = events(lambda: _lib.call('spaa_layernorm_fwd', p(x), D, p(w), p(b), p(y), D, p(mean), p(rstd), rows, D, 1e-6), args.reps)
    t_lnb = events(lambda: _lib.call('spaa_layernorm_bwd', p(g), D, p(x), D, p(w), p(mean), p(rstd), p(add), D, p(y), D, rows, D), args.reps)
    pre, act, gp = (torch.randn(rows, M, device=dev) for _ in range(3))
    t_gf = events(lambda: _lib.call('spaa_gelu_fwd', p(pre), p(act), rows * M), args.reps)
    t_gb = events(lambda: _lib.call('spaa_gelu_bwd', p(gp), p(pre), p(act), rows * M), args.reps)
    qkv, g_qkv = torch.randn(B, T, 3 * D, device=dev), torch.zeros(B, T, 3 * D, device=dev)
    ctx, g_ctx = torch.zeros(B, T, D, device=dev), torch.randn(B, T, D, device=dev)
    lse, delta = torch.zeros(B, H, T, device=dev), torch.zeros(B, H, T, device=dev)
    t_af = events(lambda: _lib.call('spaa_attn_fwd', p(qkv), p(ctx), p(lse), B, T, H, DH), args.reps)
    t_ab = events(lambda: _lib.call('spaa_attn_bwd', p(qkv), p(ctx), p(lse), p(g_ctx), p(g_qkv), p(delta), B, T, H, DH), args.reps)

    def bw(nbytes, t):
        return dict(us=round(t * 1e6, 1), bytes=nbytes, TB_s=round(nbytes / t / 1e12, 2))

    def fl(flops, t):
        return dict(us=round(t * 1e6, 1), gflop=round(flops / 1e9, 2), TFLOP_s=round(flops / t / 1e12, 2))

    alone = dict(layernorm_fwd=bw(8 * rows * D, t_lnf), layernorm_bwd=bw(16 * rows * D, t_lnb), gelu_fwd=bw(8 * rows * M, t_gf),
                 gelu_bwd=bw(12 * rows * M, t_gb), attn_fwd=fl(4 * B * T * T * D, t_af), attn_bwd=fl(10 * B * T * T * D, t_ab))
    print(alone, file=sys.stderr, flush=True)
    del x, g, add, y, pre, act, gp, qkv, g_qkv, ctx, g_ctx

    # 2. one forward + backward pass of the body, eager, per launch group
    def body_pass(name, sd):
        eng = ClassifierEngine(name, sd, B, (240, 320), (240, 240), None, dev)
        yy = torch.rand(B, 240, 320, 4, device=dev)
        gg = torch.randn(B, eng.ncls, device=dev)
        eng.forward(yy)
        eng.backward(gg)
        torch.cuda.synchronize()
        _lib.PROFILE = []
        eng.forward(yy)
        eng.backward(gg)
        torch.cuda.synchronize()
        prof, _lib.PROFILE = _lib.PROFILE, None
        grp = {}
        for entry, e0, e1 in prof:
            if entry.startswith('spaa_preproc'):
                continue
            k = GROUPS.get(entry, 'bookkeeping_and_pools')
            grp[k] = grp.get(k, 0.0) + e0.elapsed_time(e1) * 1e3
        out = dict(launches=len(prof) - 2, us={k: round(v, 1) for k, v in grp.items()}, total_us=round(sum(grp.values()), 1),
                   fwd_gflop=round(eng.body.flops_fwd() / 1e9, 2))
        if hasattr(eng.body, 'flops_attention'):
            out['attention_fwd_gflop'] = round(eng.body.flops_attention() / 1e9, 2)
            out['attention_share_of_time'] = round(grp.get('attention', 0.0) / sum(grp.values()), 3)
            out['saved_for_backward_GB'] = round(4 * B * T * (6 * D + M) * eng.body.depth / 1e9, 2)
        del eng
        return out

    vsd, rsd = syn.vit_b_16_state_dict(7, logit_gain=4.0), syn.resnet18_state_dict(2, logit_gain=20.0)
    passes = dict(vit_b_16=body_pass('vit_b_16', vsd), resnet18=body_pass('resnet18', rsd))
    print(passes, file=sys.stderr, flush=True)

    # 3. the 11 attacks of one (loss, d_thr) point at the reference geometry
    cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
    sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    clfs = dict(resnet18=Classifier('resnet18', dev, state_dict=rsd), vit_b_16=Classifier('vit_b_16', dev, state_dict=vsd))
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

    rec = dict(tool='time_vit', device=torch.cuda.get_device_name(0), weights='random-init (spaa_amd.synthetic)', batch=B,
               kernels_alone=dict(how=f'HIP events around each launch, median of {args.reps} after one unrecorded launch; {rows} rows of {D} '
                                      f'(LayerNorm) / {M} (GELU) floats, attention at T = {T}, 12 heads of 64', **alone,
                                  yardstick='spaa_transfer_momentum: 3.0 TB/s (DESIGN.md 7i)'),
               forward_backward_pass=dict(how='HIP events around every launch of one eager forward + backward pass at 224 x 224 (the '
                                              'preprocessing launches left out), after one unrecorded pass', **passes),
               attack=dict(geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], samples=len(tgt) + 1, iters=args.iters, loss='camdE_caml2', d_thr=5),
                           graph=graphs, runs=runs, wall_s_median={n: med([r[n + '_s'] for r in runs]) for n in clfs},
                           parent_resnet18_s=0.1676),
               not_tuned='the plans run on tiles measured for other shapes; tapconv_tune.json is unchanged')
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
