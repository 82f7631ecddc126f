"""Device time of the MobileNetV2 body (spaa_amd/mobilenet.py) and its depthwise kernels (csrc/dwconv.hip), in one process:

  1. spaa_dwconv3_fwd / spaa_dwconv3_bwd alone at B = 64 on five layers of the network at 224 x 224: HIP events around each launch, the
     median of --reps after one unrecorded launch; algorithmic bytes (forward: input + output + gate bytes; backward: output gradient +
     pre-activation + input gradient; the 40 bytes of weights per channel are left out) over that time, and its share of the 8 TB/s
     the project quotes for HBM.  spaa_transfer_momentum reaches 3.0 TB/s: the project's own yardstick for an
     elementwise pass.
  2. one forward + backward pass of the body at B = 64, 224 x 224: the sum of the eager launch times (HIP events around every launch)
     per kernel family -- the tap-list convolution launches (stem, 1 x 1 plans), the depthwise launches, the head (ReLU6 of features.18,
     average pool and its adjoint, the linear layer) -- with ResNet-18's total next to it;
  3. the 11 attacks of one (stealth loss, d_thr) point at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240, 50
     iterations) with mobilenet_v2 and, alternating with it, with ResNet-18: the median of --runs wall times, each bracketed by a
     device synchronise, after a warm-up of each.  The ResNet-18 figure is the one profiles/transfer_time.jsonl records (0.169 s): the
     body is new code beside it, so it should stay inside the 3 % box variance of profiles/r06_box_variance.txt.

The networks are RANDOM-INIT (spaa_amd.synthetic).  Appends one JSON line to --out and prints it.

    python tools/time_mobilenet.py [--reps 10] [--runs 3] [--out profiles/mobilenet_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12
# (H, W, C, stride) of the depthwise layers timed alone: features.1, features.2, features.3, features.12 and features.16
LAYERS = ((112, 112, 32, 1), (112, 112, 96, 2), (56, 56, 144, 1), (14, 14, 576, 1), (7, 7, 960, 1))
FAMILIES = {'spaa_tapconv_f32': 'tapconv', 'spaa_dwconv3_fwd': 'depthwise', 'spaa_dwconv3_bwd': 'depthwise'}   # anything else: head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'mobilenet_time.jsonl'))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from spaa_amd import _lib, synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier, ClassifierEngine
    from spaa_amd import projector_based_attack as A

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    p, B = _lib.ptr, args.batch
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

    # 1. the depthwise kernels alone
    alone = []
    for h, w, c, s in LAYERS:
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        x = torch.randn(B, h, w, c, device=dev) * 4 + 2
        wt, bias = torch.randn(9, c, device=dev) * 0.3, torch.rand(c, device=dev) * 3
        out, mask = torch.zeros(B, ho, wo, c, device=dev), torch.zeros(B, ho, wo, c // 4, dtype=torch.uint8, device=dev)
        g_out, g_in = torch.randn(B, ho, wo, c, device=dev), torch.zeros(B, h, w, c, device=dev)
        tf = events(lambda: _lib.call('spaa_dwconv3_fwd', p(x), 1, p(wt), p(bias), p(out), p(mask), B, h, w, c, s), args.reps)
        tb = events(lambda: _lib.call('spaa_dwconv3_bwd', p(g_out), p(wt), p(x), p(g_in), B, h, w, c, s), args.reps)
        bf = 4 * x.numel() + 4 * out.numel() + mask.numel()
        bb = 4 * g_out.numel() + 4 * x.numel() + 4 * g_in.numel()
        alone.append(dict(layer=f'{h}x{w}x{c} s{s}', fwd_us=round(tf * 1e6, 1), fwd_bytes=bf, fwd_TB_s=round(bf / tf / 1e12, 2),
                          fwd_share_of_8TB_s=round(bf / tf / HBM_BYTES_PER_S, 3), bwd_us=round(tb * 1e6, 1), bwd_bytes=bb,
                          bwd_TB_s=round(bb / tb / 1e12, 2), bwd_share_of_8TB_s=round(bb / tb / HBM_BYTES_PER_S, 3)))
        print(alone[-1], file=sys.stderr, flush=True)
        del x, out, mask, g_out, g_in

    # 2. one forward + backward pass of the body, eager, per kernel family
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
        fam = {}
        for entry, e0, e1 in prof:
            if entry.startswith('spaa_preproc'):
                continue
            k = FAMILIES.get(entry, 'head_and_pools')
            fam[k] = fam.get(k, 0.0) + e0.elapsed_time(e1) * 1e3
        flops = eng.body.flops_fwd()
        del eng
        return dict(launches=len(prof) - 2, us={k: round(v, 1) for k, v in fam.items()}, total_us=round(sum(fam.values()), 1),
                    fwd_gflop=round(flops / 1e9, 2))

    msd, rsd = syn.mobilenet_v2_state_dict(6, logit_gain=4.0), syn.resnet18_state_dict(2, logit_gain=20.0)
    passes = dict(mobilenet_v2=body_pass('mobilenet_v2', msd), resnet18=body_pass('resnet18', rsd))
    print(passes, file=sys.stderr, flush=True)

    # 3. the 11 attacks of one (loss, d_thr) point at the reference geometry
    cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
    sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    clfs = dict(resnet18=Classifier('resnet18', dev, state_dict=rsd), mobilenet_v2=Classifier('mobilenet_v2', dev, state_dict=msd))
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

    rec = dict(tool='time_mobilenet', device=torch.cuda.get_device_name(0), weights='random-init (spaa_amd.synthetic)', batch=B,
               depthwise_alone=dict(how=f'HIP events around each launch, median of {args.reps} after one unrecorded launch', layers=alone,
                                    yardstick='spaa_transfer_momentum: 3.0 TB/s (DESIGN.md 7i)'),
               forward_backward_pass=dict(how='HIP events around every launch of one eager forward + backward pass at 224 x 224 (the '
                                              'preprocessing launches left out), after one unrecorded pass', **passes),
               attack=dict(geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], samples=len(tgt) + 1, iters=args.iters, loss='camdE_caml2', d_thr=5),
                           graph=graphs, runs=runs, wall_s_median={n: med([r[n + '_s'] for r in runs]) for n in clfs},
                           parent_resnet18_s=0.169))
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
