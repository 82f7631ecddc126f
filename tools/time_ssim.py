"""Device time of the SSIM stealth term's kernels and wall time of an attack with the term ('camssim'), in one process:

  (a) the new forward + adjoint (spaa_ssim_fwd + spaa_ssim_bwd, and spaa_ssim_value, the reduce) at B = 64, 256 x 256, next to
      spaa_train_loss_fwd_bwd(l1_w = 0, ssim_w = 1) at the same shape on the same images: the 121-tap pair the project had before,
      which computes the same map and the same gradient (of the batch mean).  HIP events around --reps back-to-back launches after
      --warmup unrecorded ones, repeated --runs times; the record keeps every run and the medians.  spaa_ssim_scene_stats (once per
      attack, not per iteration) is timed in the same way.
  (b) at the reference's geometry (projector 256 x 256, camera 240 x 320, crop 240, ResNet-18 at its full input size): the 11 attacks
      of one (loss, d_thr) point (10 targeted + 1 untargeted samples, 50 iterations) as one spaa_sweep with 'caml2_camssim' against
      'caml2': the median of --runs wall times, each bracketed by a device synchronise, after one warm-up of each kind; the mean
      calc_img_dists SSIM (and L2) of the results against the scene either way, and the device time of the term's launches per
      iteration from HIP events around every launch of --profile-iters eager iterations.

PCNet and the classifier are RANDOM-INIT (spaa_amd.synthetic): the outcome numbers say that the path runs, not what the term buys in
visibility -- that needs trained networks and a camera; the record says so.  One GPU, nothing else running on it, clocks as the box
sets them; a second process on the card moves the figures by the 3 % of profiles/r06_box_variance.txt.  Appends one JSON line to --out
and prints it.

    python tools/time_ssim.py [--runs 5] [--reps 20] [--out profiles/ssim_time.jsonl] [--kernels-only]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
TERM = ('spaa_ssim_fwd', 'spaa_ssim_bwd', 'spaa_ssim_value')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--d-thr', type=float, default=5)
    ap.add_argument('--profile-iters', type=int, default=10)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'ssim_time.jsonl'))
    args = ap.parse_args()
    from spaa_amd import _lib, metrics, synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier
    from spaa_amd import projector_based_attack as A

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    p, lib = _lib.ptr, _lib.load()
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731

    # ---- (a) the kernels alone
    B, H, W = 64, 256, 256
    torch.manual_seed(0)
    scene = torch.rand(B, H, W, 4, device=dev)
    y = (scene + 0.1 * (torch.rand(B, H, W, 4, device=dev) - 0.5)).clamp(0, 1)
    taps = (ctypes.c_float * 11)(*metrics.ssim_taps().tolist())
    window = metrics._window().to(dev)
    tiles = lib.spaa_ssim_tiles(H, W)
    w_ps = torch.ones(B, device=dev)
    mu2, e22, m_mu, m_11, m_12, g = (torch.zeros(B, H, W, 4, device=dev) for _ in range(6))
    partial, val = torch.zeros(B, tiles, device=dev), torch.zeros(B, device=dev)
    partial_old = torch.zeros(B * ((H + 15) // 16) * ((W + 15) // 16), 3, device=dev)
    gscale = 1.0 / (B * 3 * H * W)

    def new_pair():
        _lib.call('spaa_ssim_fwd', p(y), p(scene), p(mu2), p(e22), taps, p(w_ps), p(m_mu), p(m_11), p(m_12), p(partial), B, H, W)
        _lib.call('spaa_ssim_bwd', p(y), p(scene), p(m_mu), p(m_11), p(m_12), taps, p(w_ps), gscale, p(g), B, H, W)
        _lib.call('spaa_ssim_value', p(partial), p(w_ps), tiles, H, W, p(val), B)

    def old_pair():
        _lib.call('spaa_train_loss_fwd_bwd', p(y), p(scene), p(window), 0.0, 1.0, p(m_mu), p(m_11), p(m_12), p(partial_old), p(g), B, H, W)

    def scene_stats():
        _lib.call('spaa_ssim_scene_stats', p(scene), taps, p(mu2), p(e22), B, H, W)

    def device_us(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    scene_stats()
    # the two pairs agree: the old launch writes the gradient of the batch mean, the new one adds gscale times the per-sample one
    g.zero_()
    new_pair()
    g_new = g.clone()
    old_pair()
    torch.cuda.synchronize()
    agree = float((g_new - g)[..., :3].abs().max() / g[..., :3].abs().max())
    kernels = {name: [] for name in ('new_fwd_bwd_value_us', 'train_loss_fwd_bwd_us', 'scene_stats_us')}
    for _ in range(args.runs):   # interleaved, so that a drift of the clocks meets both alike
        kernels['new_fwd_bwd_value_us'].append(round(device_us(new_pair), 1))
        kernels['train_loss_fwd_bwd_us'].append(round(device_us(old_pair), 1))
        kernels['scene_stats_us'].append(round(device_us(scene_stats), 1))
    m_new, m_old = med(kernels['new_fwd_bwd_value_us']), med(kernels['train_loss_fwd_bwd_us'])
    rec = dict(tool='time_ssim', device=torch.cuda.get_device_name(0),
               kernels_alone=dict(B=B, H=H, W=W, image_bytes=B * H * W * 16,
                                  how=f'HIP events around {args.reps} back-to-back launches after {args.warmup} unrecorded, {args.runs} runs '
                                      'interleaved; medians',
                                  runs=kernels, median_us={k: med(v) for k, v in kernels.items()},
                                  old_over_new=round(m_old / m_new, 2), max_rel_gradient_difference=agree))
    print(json.dumps(rec['kernels_alone']), file=sys.stderr, flush=True)
    del scene, y, mu2, e22, m_mu, m_11, m_12, g, g_new, partial_old

    # ---- (b) the attack
    if not args.kernels_only:
        cam_sz, prj_sz, crop = (240, 320), (256, 256), (240, 240)
        sd = syn.pcnet_state_dict(0, cam_sz=cam_sz, mask='ones')
        pc = PCNet(sd['mask'], WarpingNet(out_size=cam_sz))
        pc.load_state_dict(sd)
        pc = pc.to(dev)
        r18 = Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0))
        setup = dict(classifier_crop_sz=crop, prj_brightness=0.5, prj_im_sz=prj_sz)
        sc = syn.scenes(1, 1, cam_sz)[0].to(dev)
        with torch.no_grad():
            true_idx = int(r18(sc, crop)[0][0].argmax())
        tgt = list(syn.IMAGENET10_TARGETS)
        all_t, all_tg = tgt + [true_idx], [True] * len(tgt) + [False]
        losses = ('caml2', 'caml2_camssim')

        def attack(loss):
            (ct, _), (cu, _) = A.spaa_sweep(pc, r18, None, sc, setup, dev, [(loss, args.d_thr, True, tgt), (loss, args.d_thr, False, [true_idx])],
                                            iters=args.iters)
            return torch.cat((ct, cu))

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        for loss in losses:   # warm-up: engines, plans, the graphs' first captures
            attack(loss)
        runs, last, graphs = [], {}, {}
        for _ in range(args.runs):
            row = {}
            for loss in losses:
                t, last[loss] = timed(lambda: attack(loss))
                graphs[loss] = A.LAST_RUN['graph']
                row[loss + '_s'] = round(t, 4)
            runs.append(row)
            print(row, file=sys.stderr, flush=True)
        nb = len(all_t)
        scene_b = sc[None].expand(nb, -1, -1, -1).contiguous()
        outcome = {}
        for loss, cams in last.items():
            d = metrics.calc_img_dists(cams, scene_b)
            outcome[loss] = dict(ssim_mean=round(float(d[2]), 5), l2_mean=round(float(d[3]), 4), linf_mean=round(float(d[4]), 4),
                                 dE_mean=round(float(d[5]), 4))
        launches = {}
        for loss in losses:
            st = A.AttackState(pc, r18, all_t, sc, loss, setup, dev)
            st.iteration(all_tg, args.d_thr, 2, 1, 0.9)
            _lib.PROFILE = []
            for _ in range(args.profile_iters):
                st.iteration(all_tg, args.d_thr, 2, 1, 0.9)
            torch.cuda.synchronize()
            prof, _lib.PROFILE = _lib.PROFILE, None
            per, total = {n: 0.0 for n in TERM}, 0.0
            for entry, e0, e1 in prof:
                ms = e0.elapsed_time(e1)
                total += ms
                if entry in per:
                    per[entry] += ms
            launches[loss] = dict({n + '_us': round(per[n] * 1e3 / args.profile_iters, 2) for n in TERM},
                                  all_launches_us=round(total * 1e3 / args.profile_iters, 1),
                                  launches_per_iteration=len(prof) // args.profile_iters)
            del st
        rec['attack'] = dict(
            weights='random-init (spaa_amd.synthetic): the outcome numbers say only that the path runs; what the term buys in visibility '
                    'needs trained networks and a camera',
            geometry=dict(prj=prj_sz, cam=cam_sz, crop=crop[0], samples=nb, iters=args.iters, d_thr=args.d_thr), graph=graphs, runs=runs,
            wall_s_median={loss: med([r[loss + '_s'] for r in runs]) for loss in losses}, outcome_calc_img_dists=outcome,
            launch_device_time_per_iteration=dict(how=f'HIP events around each launch, mean of {args.profile_iters} eager iterations',
                                                  **launches))

    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
