"""SPAA — Stealthy Projector-based Adversarial Attack, fused on device.

Drop-in for `spaa()` of /root/reference/src/python/projector_based_attack.py:212-339: same positional signature and
return value `(cam_infer_best, prj_adv_best)`; the reference's hard-coded locals (:243-258) are keyword arguments
with the reference values as defaults.  Differences in *mechanism*, not in result:

  * the sampling grid, skipConv1(s) and Lab(scene) are loop-invariant and computed once, not per iteration;
  * masks, top-1/confidence, loss reductions and best-so-far bookkeeping stay on the GPU (the reference syncs to
    the host three times per iteration: classifier.py:64, projector_based_attack.py:291,318);
  * ONE backward pass per iteration with a per-sample-selected cotangent instead of two (each sample consumes either
    the adversarial or the stealthiness gradient, :307 / :315, and samples are independent);
  * `cam_scene` may also be [B,3,H,W] (one scene per sample); the reference supports one scene x B targets (Q9),
    and its targeted mode needs B >= 8 because of a debug print (Q10) — not inherited.
"""
import warnings

import numpy as np
import torch

from . import _lib
from .models import PCNet, to_nhwc4, to_nchw
from .classifier import Classifier


import os

# B * Hc * Wc up to which spaa() replays the iteration as a captured HIP graph (0 disables); above it the GPU is busy for
# longer than the host needs to enqueue an iteration and eager launches lose nothing (measured: < 1 % at B = 64, 256 x 256)
CLAMP_BITS = os.environ.get('SPAA_CLAMP_BITS', '1') == '1'   # the step writes the next backward pass's clamp gate as bytes (A/B runs: 0)
GRAPH_MAX_PIXELS = int(os.environ.get('SPAA_GRAPH_MAX_PIXELS', str(16 * 256 * 256)))
LAST_RUN = {}   # of the last spaa() call: executed iterations (1 eager + iters - 1 replays = iters: a capture executes nothing), graph or not


LOSS_TERMS = ('prjl2', 'caml2', 'camdE')


def loss_weights(stealth_loss):
    """(prjl2_w, caml2_w, camdE_w) of a stealth-loss string (projector_based_attack.py:275-287: a term is on when its name occurs)."""
    return (0.1 if 'prjl2' in stealth_loss else 0.0, 1.0 if 'caml2' in stealth_loss else 0.0,
            1.0 if 'camdE' in stealth_loss else 0.0)


def _is_scalar(v):
    return isinstance(v, (bool, int, float)) or (isinstance(v, torch.Tensor) and v.ndim == 0) or getattr(v, 'ndim', None) == 0


def _unwrap(m):
    return m.module if hasattr(m, 'module') and not isinstance(m, (PCNet, Classifier)) else m


class AttackState:
    """Device-side state of one batched attack (everything the loop touches, allocated once)."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage='f32'):
        """`storage`: 'f32' (default; results identical to the reference to rounding) or 'f16' (fp16-storage mode of
        BASELINE.json configs[4]: network activations and their gradients are fp16 in HBM, images / losses / dE2000 /
        norms / accumulation fp32)."""
        dev = torch.device(device)
        self.storage = storage
        if dev.type != 'cuda':
            raise RuntimeError('spaa_amd.spaa runs on the GPU only (no CPU fallback); got device=%s' % device)
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        with _lib.on_device(dev):  # kernels launch on the current device: make it the one the state lives on
            self._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        B = len(target_idx)
        if B < 1:
            raise ValueError('target_idx is empty: nothing to attack')
        self.B, self.dev = B, dev
        prj_sz = tuple(setup_info['prj_im_sz'])
        self.cp_sz = tuple(setup_info['classifier_crop_sz'])
        self.gray = float(setup_info['prj_brightness'])
        cam_scene = cam_scene.detach().float()
        while cam_scene.ndim < 4:
            cam_scene = cam_scene[None]
        if cam_scene.shape[0] == 1:
            cam_scene = cam_scene.expand(B, -1, -1, -1)
        if cam_scene.shape[0] != B:
            raise ValueError('cam_scene must hold 1 or len(target_idx) scenes')
        self.eng = pcnet.engine(B, prj_sz, owner=self, storage=self.storage)
        Hc, Wc = self.eng.Hc, self.eng.Wc
        if tuple(cam_scene.shape[-2:]) != (Hc, Wc):
            raise ValueError(f'cam_scene is {tuple(cam_scene.shape[-2:])} but PCNet outputs {(Hc, Wc)}')
        self.clf = classifier.engine(B, (Hc, Wc), self.cp_sz, owner=self, storage=self.storage)
        # fp16 gradients need a loss scale (fp16's smallest normal is 6e-5; the per-pixel loss gradients are ~1/(B*H*W)).
        # Each sample's gradient is normalised before the step (:307, :315), so a positive per-branch scale changes
        # nothing but the fp16 rounding: stealth branch: 1/16 per pixel instead of 1/(B*H*W); adversarial branch: +-16
        # at the target logit instead of 1/B.
        self.gs_col, self.gs_adv = ((B * Hc * Wc) / 16.0, 16.0 * B) if self.storage == 'f16' else (1.0, 1.0)
        self.scene4 = to_nhwc4(cam_scene.contiguous().to(dev))
        self.eng.set_scene(self.scene4)
        self.scene_lab = torch.zeros_like(self.scene4)
        _lib.call('spaa_rgb2lab', _lib.ptr(self.scene4), _lib.ptr(self.scene_lab), B * Hc * Wc)
        Hp, Wp = prj_sz
        self.HWp, self.HWc = Hp * Wp, Hc * Wc
        self.x = torch.zeros(B, Hp, Wp, 4, device=dev)
        self.x[..., :3] = self.gray
        self.x_best = self.x.clone()
        self.cam_best = self.scene4.clone()
        self.state = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(B, 8, device=dev)
        self.stats[:, 5] = 1e6
        self.nblk_c = (self.HWc + 255) // 256
        self.nblk_p = (self.HWp + 255) // 256
        self.partial_loss = torch.zeros(B, self.nblk_c, 3, device=dev)
        # ||g_b||^2 partial sums: per 256-pixel block (spaa_grad_sumsq), or per 16 x 16 projector tile when the tiled grid_sample
        # adjoint computes them in its epilogue
        self.ss_tiles = self.eng.sumsq_tiles()
        self.partial_ss = torch.zeros(B, self.ss_tiles or self.nblk_p, device=dev)
        # The clamp gate of x.clamp(0, 1) (:265) for the backward pass as one byte per projector pixel, written by the step that writes x:
        # the grid_sample adjoint then reads 1 byte per pixel instead of x's 16.  The bytes describe self.x as long as nobody else has
        # written it: `_bits_version` remembers torch's version counter of self.x (in-place torch writes -- tests that inject an x --
        # bump it, this module's own kernels go through raw pointers and do not): a mismatch falls back to the comparisons on x.
        self.clamp_bits = torch.zeros(B, self.HWp, dtype=torch.uint8, device=dev) if self.ss_tiles and CLAMP_BITS else None
        self._bits_version = -1
        self.g_col = torch.zeros(B, Hc, Wc, 4, device=dev)
        self.gP = torch.zeros(B, Hc, Wc, 4, device=dev)
        self.g_logits = torch.zeros(B, self.clf.ncls, device=dev)
        self.prjl2 = torch.zeros(B, device=dev)
        self.target = torch.tensor([int(t) for t in target_idx], dtype=torch.int32, device=dev)
        # `stealth_loss`: one string for the batch, or one per sample (spaa_sweep).  self.prjl2_w / caml2_w / camdE_w are the batch's
        # weights when every sample has the same ones, else None: the per-sample table of the _ps launches carries them.
        losses = [stealth_loss] * B if isinstance(stealth_loss, str) else list(stealth_loss)
        if len(losses) != B:
            raise ValueError(f'stealth_loss: {len(losses)} strings for {B} samples')
        self.loss_w = [loss_weights(s) for s in losses]
        uniform = all(w == self.loss_w[0] for w in self.loss_w)
        self.prjl2_w, self.caml2_w, self.camdE_w = self.loss_w[0] if uniform else (None, None, None)
        self.any_prjl2 = any(w[0] for w in self.loss_w)
        self._ps_key = None      # (targeted, d_thr) per sample of the uploaded table, None: scalar launches
        self.ps_params = torch.zeros(B, 4, device=dev)
        self.ps_flags = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ps_prjl2_scale = torch.zeros(B, device=dev)

    def _per_sample(self, targeted, d_thr):
        """The batch's (targeted, d_thr) as scalars when every sample agrees and the loss weights are uniform (the launches of a single
        attack, unchanged); else uploads the per-sample table (once per distinct setting: a captured graph replays the table it
        read) and returns None."""
        B = self.B
        tg = [bool(targeted)] * B if _is_scalar(targeted) else [bool(t) for t in targeted]
        dt = [float(d_thr)] * B if _is_scalar(d_thr) else [float(d) for d in d_thr]
        if len(tg) != B or len(dt) != B:
            raise ValueError(f'targeted / d_thr: one value or {B} values')
        if self.caml2_w is not None and all(t == tg[0] for t in tg) and all(d == dt[0] for d in dt):
            return tg[0], dt[0]
        key = (tuple(tg), tuple(dt))
        if key != self._ps_key:
            params = torch.tensor([list(w) + [d] for w, d in zip(self.loss_w, dt)], dtype=torch.float32)
            self.ps_params.copy_(params)
            self.ps_flags.copy_(torch.tensor([int(t) for t in tg], dtype=torch.int32))
            self.ps_prjl2_scale.copy_(params[:, 0] / (B * self.HWp) * self.gs_col)
            self._ps_key = key
        return None

    def iteration(self, targeted, d_thr, adv_lr, col_lr, p_thresh, adv_w=1.0):
        """One pass of the loop body (projector_based_attack.py:264-328), ~90 kernel launches, no host sync.  `targeted` and `d_thr`:
        one value for the batch or one per sample."""
        with torch.cuda.device(self.dev):
            self._forward_decide(targeted, d_thr, p_thresh, adv_w)
            self._backward_step(adv_lr, col_lr)

    def forward_decide(self, targeted, d_thr, p_thresh, adv_w=1.0):
        """First half of `iteration` (:265-299): forward passes, losses and their gradient at the camera image, masks."""
        with torch.cuda.device(self.dev):
            self._forward_decide(targeted, d_thr, p_thresh, adv_w)

    def backward_step(self, adv_lr, col_lr):
        """Second half of `iteration` (:302-328): the backward pass, the normalised step and the best-so-far bookkeeping.
        (The halves are separate entry points so that the parity tests can compare / exchange the ReLU gates in between.)"""
        with torch.cuda.device(self.dev):
            self._backward_step(adv_lr, col_lr)

    def _forward_decide(self, targeted, d_thr, p_thresh, adv_w):
        B, p = self.B, _lib.ptr
        uni = self._per_sample(targeted, d_thr)
        y = self.eng.forward(self.x, clamp01=True)                                   # :265
        logits = self.clf.forward(y)                                                 # :266
        self._y, self._uniform = y, uni is not None
        if uni is None:   # several attack configurations in one batch: the same kernels, their parameters per sample
            if self.any_prjl2:
                _lib.call('spaa_prjl2_fwd', p(self.x), self.gray, p(self.prjl2), B, self.HWp)
            _lib.call('spaa_stealth_loss_fwd_bwd_ps', p(y), p(self.scene4), p(self.scene_lab), p(self.ps_params),
                      self.gs_col / (B * self.HWc), p(self.g_col), None, p(self.partial_loss), B, self.HWc)
            _lib.call('spaa_decide_ps', p(logits), self.clf.ncls, p(self.target), p(self.partial_loss), self.nblk_c, self.HWc,
                      p(self.prjl2) if self.any_prjl2 else None, p(self.ps_params), p(self.ps_flags), float(p_thresh),
                      adv_w / B * self.gs_adv, p(self.state), p(self.stats), p(self.g_logits), B)
            return
        targeted, d_thr = uni
        if self.prjl2_w:
            _lib.call('spaa_prjl2_fwd', p(self.x), self.gray, p(self.prjl2), B, self.HWp)    # :275
        _lib.call('spaa_stealth_loss_fwd_bwd', p(y), p(self.scene4), p(self.scene_lab), self.caml2_w, self.camdE_w,
                  self.gs_col / (B * self.HWc), p(self.g_col), None, p(self.partial_loss), B, self.HWc)   # :279-287 + bwd
        _lib.call('spaa_decide', p(logits), self.clf.ncls, p(self.target), int(bool(targeted)), p(self.partial_loss),
                  self.nblk_c, self.HWc, p(self.prjl2) if self.prjl2_w else None, self.prjl2_w, self.caml2_w,
                  self.camdE_w, float(d_thr), float(p_thresh), adv_w / B * self.gs_adv, p(self.state), p(self.stats),
                  p(self.g_logits), B)                                               # :269-272, :290-299, :318-320

    def _backward_step(self, adv_lr, col_lr):
        B, p, y = self.B, _lib.ptr, self._y
        g_adv = self.clf.backward(self.g_logits)                                     # :302 (classifier part)
        # (mixed configurations: the prjl2 scale is a [B] device tensor, and the sums of squares take the _ps launches)
        prjl2_scale = self.prjl2_w / (B * self.HWp) * self.gs_col if self._uniform else self.ps_prjl2_scale
        ss = (self.partial_ss, self.gray, prjl2_scale, self.state) if self.ss_tiles else None   # (||g||^2 from the adjoint's epilogue)
        bits = self.clamp_bits if (self.clamp_bits is not None and self._bits_version == self.x._version) else None
        if self.eng.can_select():   # (the per-sample choice and the clamp gate as the first phase of the fused head kernel)
            gx = self.eng.backward(None, select=(g_adv, self.g_col, self.state), sumsq=ss, clamp_bits=bits)   # :302 / :310 (PCNet part)
        else:
            _lib.call('spaa_select_grad', p(g_adv), p(self.g_col), p(self.state), p(self.eng.a['Ypre']), p(self.gP), B,
                      self.HWc)
            gx = self.eng.backward(self.gP, sumsq=ss, clamp_bits=bits)               # :302 / :310 (PCNet part)
        if not self.ss_tiles and self._uniform:
            _lib.call('spaa_grad_sumsq', p(gx), p(self.x), self.gray, prjl2_scale, p(self.state), p(self.partial_ss), B, self.HWp)
        elif not self.ss_tiles:
            _lib.call('spaa_grad_sumsq_ps', p(gx), p(self.x), self.gray, p(prjl2_scale), p(self.state), p(self.partial_ss), B,
                      self.HWp)
        _lib.call('spaa_step_and_track_n', p(self.x), p(gx), p(self.partial_ss), self.partial_ss.shape[1], p(self.state), float(adv_lr),
                  float(col_lr), p(self.x_best), p(y), p(self.cam_best), B, self.HWp, self.HWc,
                  p(self.clamp_bits) if self.clamp_bits is not None else None)       # :307,315,323-328
        self._bits_version = self.x._version

    def results(self):
        with torch.cuda.device(self.dev):
            return to_nchw(self.cam_best), to_nchw(self.x_best, clamp01=True)        # :337


def spaa(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr, stealth_loss, device, setup_info,
         *, iters=50, adv_lr=2, col_lr=1, p_thresh=0.9, trace=None, verbose=False, storage='f32'):
    """Stealthy Projector-based Adversarial Attack (SPAA Algorithm 1) — see module docstring.

    :param pcnet: spaa_amd.PCNet (optionally wrapped in DataParallel-like `.module`)
    :param classifier: spaa_amd.Classifier
    :param imagenet_labels: dict idx -> name (only used when verbose)
    :param target_idx: list of B class ids (true label if untargeted)
    :param targeted: bool
    :param cam_scene: [3,H,W] / [1,3,H,W] / [B,3,H,W] in [0,1]
    :param d_thr: SPAA Algorithm 1's threshold on the mean per-pixel L2 perturbation (x255)
    :param stealth_loss: string containing any of 'prjl2', 'caml2', 'camdE'
    :param setup_info: {'classifier_crop_sz', 'prj_brightness', 'prj_im_sz'}
    :param trace: optional list; receives per-iteration (state, stats) device tensors (no sync inside the loop)
    :return: (cam_infer_best [B,3,Hc,Wc], prj_adv_best [B,3,Hp,Wp] in [0,1])
    """
    pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
    if not isinstance(pcnet, PCNet):
        raise TypeError('spaa_amd.spaa needs a spaa_amd.PCNet (the HIP path has no generic PCNet fallback)')
    if not isinstance(classifier, Classifier):
        if not callable(classifier):
            raise TypeError('classifier must be a spaa_amd.Classifier or a callable (im, crop_sz) -> (raw_score, p, idx)')
        return _spaa_foreign_classifier(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr,
                                        stealth_loss, device, setup_info, iters, adv_lr, col_lr, p_thresh, trace)
    st = AttackState(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage)

    def report(i):
        if i % 30 == 0 or i == iters - 1:
            s, f = st.state.cpu(), st.stats.cpu()
            v = 7 if (targeted and st.B > 7) else 0
            name = imagenet_labels[int(s[v, 3])] if imagenet_labels else ''
            print(f'col_loss = {f[:, 3].mean():<9.4f} | prjl2 = {f[:, 4].mean() * 255:<9.4f} | caml2 = '
                  f'{f[:, 1].mean() * 255:<9.4f} | camdE = {f[:, 2].mean():<9.4f} | p = {f[v, 0]:.4f} | y = '
                  f'{int(s[v, 3]):3d} ({name})')

    _run(st, targeted, d_thr, iters, adv_lr, col_lr, p_thresh, trace, report if verbose else None)
    return st.results()


def _run(st, targeted, d_thr, iters, adv_lr, col_lr, p_thresh, trace=None, report=None):
    """The loop of spaa() (projector_based_attack.py:264-328) on an AttackState; `targeted` / `d_thr` one value or one per sample."""
    if trace is None and report is None and iters >= 4 and st.B * st.HWc <= GRAPH_MAX_PIXELS:
        # Few pixels (the reference's own calls: B = 1 and B = 10 at 240 x 320): an iteration's ~120 launches take the GPU
        # less time than the host needs to enqueue them.  The loop body has no host-side dependence on the iteration, so it is
        # captured ONCE as a HIP graph (after one eager iteration: kernel attributes, workspaces and the per-sample table exist)
        # and replayed.
        with torch.cuda.device(st.dev):
            st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)
            done = 1
            try:
                # (thread-local: GPU calls of OTHER threads -- a loader's pin-memory thread, another attack -- do not abort it)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)   # (recorded, not executed)
            except RuntimeError as e:
                # the capture was refused or a launch inside it failed: the remaining iterations run kernel by kernel (same
                # results; a real launch error shows again there, un-captured) -- said aloud, and recorded in LAST_RUN
                warnings.warn(f'spaa(): HIP-graph capture of the iteration failed, running eagerly: {type(e).__name__}: {e}',
                              RuntimeWarning, stacklevel=3)
                graph = None
            while done < iters:
                if graph is not None:
                    graph.replay()
                else:
                    st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)
                done += 1
        LAST_RUN.update(iterations=done, graph=graph is not None)
        return
    LAST_RUN.update(iterations=iters, graph=False)
    for i in range(iters):
        st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)
        if trace is not None:
            trace.append((st.state.clone(), st.stats.clone()))
        if report is not None:
            report(i)


def plan_sweep(configs, max_batch=64):
    """Host side of spaa_sweep: validates `configs` [(stealth_loss, d_thr, targeted, target_idx), ...] and flattens them, in order,
    into samples (config index, stealth_loss, d_thr, targeted, target), cut into chunks [(start, stop), ...] of at most `max_batch`
    samples (a chunk may hold several configs and may split one).  Errors name the config."""
    if int(max_batch) < 1:
        raise ValueError(f'max_batch must be >= 1, got {max_batch}')
    samples = []
    for i, cfg in enumerate(configs):
        try:
            loss, d_thr, targeted, target_idx = cfg
        except (TypeError, ValueError):
            raise ValueError(f'configs[{i}]: expected (stealth_loss, d_thr, targeted, target_idx), got {cfg!r}') from None
        if not isinstance(loss, str) or not loss or any(t not in LOSS_TERMS for t in loss.split('_')):
            raise ValueError(f'configs[{i}]: unknown stealth loss {loss!r} (terms joined by "_": {", ".join(LOSS_TERMS)})')
        target_idx = list(target_idx)
        if not target_idx:
            raise ValueError(f'configs[{i}]: target_idx is empty: nothing to attack')
        samples += [(i, loss, float(d_thr), bool(targeted), int(t)) for t in target_idx]
    if not samples:
        raise ValueError('configs is empty: nothing to attack')
    mb = int(max_batch)
    return samples, [(a, min(a + mb, len(samples))) for a in range(0, len(samples), mb)]


def split_sweep(samples, ncfg, chunk_results):
    """Inverse of plan_sweep's flattening: per-chunk (cam [n,...], prj [n,...]) in sample order -> one (cam, prj) per config."""
    cams = torch.cat([c for c, _ in chunk_results])
    prjs = torch.cat([p for _, p in chunk_results])
    assert cams.shape[0] == len(samples)
    out, a = [], 0
    for i in range(ncfg):
        b = a
        while b < len(samples) and samples[b][0] == i:
            b += 1
        out.append((cams[a:b], prjs[a:b]))
        a = b
    return out


def spaa_sweep(pcnet, classifier, imagenet_labels, cam_scene, setup_info, device, configs, *, iters=50, adv_lr=2, col_lr=1,
               p_thresh=0.9, max_batch=64, storage='f32', trace=None):
    """Several SPAA attacks on one PCNet, scene and classifier as few batched attacks (the reference's driver makes one spaa() call
    per configuration: projector_based_attack.py:24-148).  `configs`: [(stealth_loss, d_thr, targeted, target_idx), ...]; returns one
    (cam_infer_best, prj_adv_best) per config, in order -- what spaa(pcnet, classifier, imagenet_labels, target_idx, targeted,
    cam_scene, d_thr, stealth_loss, device, setup_info) returns for it: samples do not interact, so only the batch differs.  The
    samples of all configs are flattened in order and cut into chunks of at most `max_batch` (one AttackState each, the loop of
    spaa() with its loss weights, targeted flag and d_thr per sample); `trace` receives one list per chunk, of the per-iteration
    (state, stats) pairs spaa() records (the chunk's samples in flattened order)."""
    samples, chunks = plan_sweep(configs, max_batch)
    pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
    if not isinstance(pcnet, PCNet):
        raise TypeError('spaa_sweep needs a spaa_amd.PCNet (the HIP path has no generic PCNet fallback)')
    if not isinstance(classifier, Classifier):
        raise TypeError('spaa_sweep needs a spaa_amd.Classifier')
    if torch.device(device).type != 'cuda':
        raise RuntimeError('spaa_amd.spaa_sweep runs on the GPU only (no CPU fallback); got device=%s' % device)
    sc = cam_scene.detach()
    while sc.ndim < 4:
        sc = sc[None]
    cam_sz = tuple(pcnet.warping_net.out_size)
    if sc.ndim != 4 or sc.shape[0] != 1 or tuple(sc.shape[1:]) != (3,) + cam_sz:
        raise ValueError(f'cam_scene must be [3,H,W] or [1,3,H,W] with (H, W) = {cam_sz} (PCNet\'s output); got {tuple(cam_scene.shape)}')
    results = []
    for a, b in chunks:
        part = samples[a:b]
        st = AttackState(pcnet, classifier, [t for *_, t in part], sc, [s[1] for s in part], setup_info, device, storage=storage)
        tr = [] if trace is not None else None
        _run(st, [s[3] for s in part], [s[2] for s in part], iters, adv_lr, col_lr, p_thresh, tr)
        if trace is not None:
            trace.append(tr)
        results.append(st.results())
        del st
    return split_sweep(samples, len(configs), results)


class _StealthFn(torch.autograd.Function):
    """Per-sample camera-side stealth loss caml2_w * caml2 + camdE_w * camdE (projector_based_attack.py:279-284) through
    the fused HIP kernel; the kernel's analytic gradient is kept for backward."""

    @staticmethod
    def forward(ctx, cam_infer, scene4, scene_lab, caml2_w, camdE_w):
        from .models import to_nhwc4 as _to4
        y4 = _to4(cam_infer)
        b, h, w, _ = y4.shape
        nblk = (h * w + 255) // 256
        part = torch.zeros(b, nblk, 3, device=y4.device)
        g = torch.zeros_like(y4)
        _lib.call('spaa_stealth_loss_fwd_bwd', _lib.ptr(y4), _lib.ptr(scene4), _lib.ptr(scene_lab), float(caml2_w),
                  float(camdE_w), 1.0 / (h * w), _lib.ptr(g), None, _lib.ptr(part), b, h * w)
        sums = part.sum(dim=1) / (h * w)
        ctx.g = to_nchw(g)
        ctx.mark_non_differentiable(sums)
        return caml2_w * sums[:, 0] + camdE_w * sums[:, 1], sums

    @staticmethod
    def backward(ctx, g_loss, _g_sums):
        return ctx.g * g_loss.view(-1, 1, 1, 1), None, None, None, None


def _spaa_foreign_classifier(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr, stealth_loss,
                             device, setup_info, iters, adv_lr, col_lr, p_thresh, trace):
    """The reference accepts ANY callable `classifier(im, crop_sz) -> (raw_score, p_sorted, idx)`
    (projector_based_attack.py:266).  For a classifier that is not a spaa_amd.Classifier the fused loop cannot run its
    body, so this route keeps PCNet (forward + input gradient) and the stealth loss on the HIP kernels, lets torch.autograd
    carry the gradient through the foreign classifier, and follows the reference's loop :264-328 step by step — with one
    backward pass of the per-sample-selected loss instead of two (samples are independent, see AttackState)."""
    from .models import to_nhwc4 as _to4
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('spaa_amd.spaa runs on the GPU only (no CPU fallback); got device=%s' % device)
    B = len(target_idx)
    with _lib.on_device(dev):
        cp_sz = tuple(setup_info['classifier_crop_sz'])
        gray = float(setup_info['prj_brightness'])
        scene = cam_scene.detach().float().to(dev)
        while scene.ndim < 4:
            scene = scene[None]
        scene = (scene.expand(B, -1, -1, -1) if scene.shape[0] == 1 else scene).contiguous()
        scene4 = _to4(scene)
        scene_lab = torch.zeros_like(scene4)
        _lib.call('spaa_rgb2lab', _lib.ptr(scene4), _lib.ptr(scene_lab), scene4.numel() // 4)
        im_gray = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), gray, device=dev)
        prj_adv = im_gray.clone().requires_grad_(True)
        prjl2_w = 0.1 if 'prjl2' in stealth_loss else 0.0
        caml2_w = 1.0 if 'caml2' in stealth_loss else 0.0
        camdE_w = 1.0 if 'camdE' in stealth_loss else 0.0
        tgt = torch.as_tensor([int(t) for t in target_idx], device=dev)
        ar = torch.arange(B, device=dev)
        prj_best, cam_best = prj_adv.detach().clone(), scene.clone()
        col_best = torch.full((B,), 1e6, device=dev)
        for _ in range(iters):
            cam_infer = pcnet(torch.clamp(prj_adv, 0, 1), scene)                                   # :265
            raw_score, p, idx = classifier(cam_infer, cp_sz)                                       # :266
            sel = raw_score[ar, tgt.to(raw_score.device)].to(dev)
            adv_b = (-sel if targeted else sel) / B                                                # :269-272 (per sample)
            col_b, sums = _StealthFn.apply(cam_infer, scene4, scene_lab, caml2_w, camdE_w)         # :279-284
            if prjl2_w:
                col_b = col_b + prjl2_w * torch.norm(im_gray - prj_adv, dim=1).mean(1).mean(1)     # :275-276
            top1 = torch.as_tensor(idx[:, 0]).to(dev)
            p1 = torch.as_tensor(p[:, 0]).to(dev)
            high_pert = sums[:, 0] * 255 > d_thr                                                   # :291
            succ = (top1 == tgt) if targeted else (top1 != tgt)                                    # :294,298
            best_adv = succ & high_pert & ((p1 > p_thresh) if targeted else torch.ones_like(succ))  # :295,299
            loss = torch.where(best_adv, col_b / B, adv_b).sum()
            g, = torch.autograd.grad(loss, prj_adv)                                                # :302 / :310
            norm = g.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
            lr = torch.where(best_adv, float(col_lr), float(adv_lr)).view(-1, 1, 1, 1)
            with torch.no_grad():
                prj_adv -= lr * g / norm                                                           # :307, :315
                col = col_b.detach()
                best = (col < col_best) & best_adv                                                 # :318-320
                col_best = torch.where(best, col, col_best)
                upd = (succ | best).view(-1, 1, 1, 1)
                prj_best = torch.where(upd, prj_adv.detach(), prj_best)                            # :323-328 (post-step, Q4)
                cam_best = torch.where(upd, cam_infer.detach(), cam_best)
            if trace is not None:
                trace.append(dict(succ=succ.clone(), best_adv=best_adv.clone(), best=best.clone(), top1=top1.clone(),
                                  caml2=sums[:, 0].clone(), camdE=sums[:, 1].clone(), prj_adv=prj_adv.detach().clone()))
        return cam_best, torch.clamp(prj_best, 0, 1)                                               # :337


spaa_attack = spaa  # name used by BASELINE.json's north_star


# ---------------------------------------------------------------------------------------------------------------
# The reference's attack driver (projector_based_attack.py:24-148, :169-209)
ATTACKERS = ('SPAA', 'PerC-AL+CompenNet++', 'One-pixel_DE')
MODEL_TRAIN_CFG = dict(loss='l1+ssim', num_train=500, batch_size=24, max_iters=2000)   # get_model_train_cfg's defaults (train_network.py)


def get_attacker_cfg(attacker_name, data_root, setup_list, device_ids=[0], load_pretrained=False, plot_on=True):
    """projector_based_attack.py:169-192: the default attacker configuration, as a mapping with attribute access."""
    from .io import SetupInfo
    cfg = SetupInfo(attacker_name=attacker_name, classifier_names=['inception_v3', 'resnet18', 'vgg16'], data_root=data_root,
                    setup_list=setup_list, device='cuda', device_ids=device_ids, load_pretrained=load_pretrained, plot_on=plot_on)
    if attacker_name == 'SPAA':
        cfg.stealth_losses, cfg.d_threshes = ['caml2', 'camdE', 'camdE_caml2'], [5, 7, 9, 11]
    elif attacker_name == 'PerC-AL+CompenNet++':
        cfg.stealth_losses, cfg.d_threshes = ['camdE'], [11]
    elif attacker_name == 'One-pixel_DE':
        cfg.stealth_losses, cfg.d_threshes = ['-'], ['-']
    return cfg


def to_attacker_cfg_str(attacker_name):
    """projector_based_attack.py:195-209: (attacker_cfg_str, model_cfg_str), the result folders' names."""
    if attacker_name not in ATTACKERS:
        raise ValueError(f'{attacker_name} not supported!')
    m = MODEL_TRAIN_CFG
    tail = f'{m["loss"]}_{m["num_train"]}_{m["batch_size"]}_{m["max_iters"]}'
    if attacker_name == 'SPAA':
        return f'SPAA_PCNet_{tail}', f'PCNet_{tail}'
    if attacker_name == 'PerC-AL+CompenNet++':
        return f'{attacker_name}_{tail}', f'CompenNet++_{tail}'
    return attacker_name, None


def run_projector_based_attack(cfg, *, models=None, classifiers=None, iters=50, train=False, model_cfg=None, capture=None):
    """projector_based_attack.py:24-148 for the deep-learning attackers: per setup and classifier, 10 targeted attacks (the first 10
    imagenet10 classes) and 1 untargeted attack (the scene's top-1) for every stealth loss x d_thr; results under
    <setup>/prj/adv and <setup>/cam/infer/adv / <attacker_cfg_str>/<loss>/<d_thr>/<classifier>/img_0001..0011.png (1-10 targeted,
    11 untargeted).  For SPAA one classifier's whole sweep is ONE spaa_sweep call.
    `models`: setup name -> trained PCNet (SPAA) / CompenNetPlusplus (PerC-AL+CompenNet++); `classifiers`: classifier name ->
    spaa_amd.Classifier (the reference downloads the classifier weights here; that is not done).
    `train=True`: a setup without an entry in `models` is trained, or with cfg.load_pretrained loaded from its checkpoint, as the
    reference does (:50-60): train_network.train_eval_pcnet (SPAA) / train_eval_compennet_pp (PerC-AL+CompenNet++) on
    get_model_train_cfg's defaults, with the fields of `model_cfg` (a mapping, e.g. dict(max_iters=100)) laid over them; the last
    configuration is left in cfg.model_cfg.  The default, train=False, raises for such a setup.
    `capture` (One-pixel_DE only, :69-73,110-142): 'model' = models[setup] is a trained PCNet that stands in for the projector and the
    camera (SimulatedCapture; captures go under cam/infer/adv), or a function setup_info -> capture callable for a real ProCams pair
    (captures go under cam/raw/adv): see _run_one_pixel_de."""
    import itertools
    import random
    from os.path import join
    from . import io
    from .classifier import load_imagenet_labels
    name = cfg.attacker_name
    if name not in ATTACKERS:
        raise ValueError(f'{name} not supported!')
    if name == 'One-pixel_DE':
        if capture is None:
            raise NotImplementedError('One-pixel_DE attacks the real scene through a projector and a camera; use '
                                      'spaa_amd.DigitalOnePixelAttacker for the digital attack, or pass capture=\'model\' (a trained '
                                      'PCNet in `models` simulates the capture) or capture=<function setup_info -> capture callable>')
        return _run_one_pixel_de(cfg, models, classifiers, capture)
    device = torch.device(cfg.device)
    random.seed(0)   # (ut.reset_rng_seeds(0))
    torch.manual_seed(0)
    attacker_cfg_str = to_attacker_cfg_str(name)[0]
    for setup_name in cfg.setup_list:
        model = (models or {}).get(setup_name)
        if model is None and train:
            from . import train_network as tn
            mcfg = tn.get_model_train_cfg(model_list=['PCNet' if name == 'SPAA' else 'CompenNet++'], data_root=cfg.data_root,
                                          setup_list=[setup_name], device_ids=cfg.device_ids, load_pretrained=cfg.load_pretrained,
                                          plot_on=cfg.plot_on)
            mcfg.device = cfg.device
            mcfg.update(model_cfg or {})
            model, _, cfg.model_cfg = (tn.train_eval_pcnet if name == 'SPAA' else tn.train_eval_compennet_pp)(mcfg)
        if model is None:
            raise ValueError(f'run_projector_based_attack: pass models={{{setup_name!r}: trained '
                             f'{"PCNet" if name == "SPAA" else "CompenNetPlusplus"}}} (models are not trained here)')
        missing = [c for c in cfg.classifier_names if c not in (classifiers or {})]
        if missing:
            raise ValueError(f'run_projector_based_attack: pass classifiers={{name: spaa_amd.Classifier}} for {missing} '
                             '(weights cannot be downloaded here)')
        setup_path = join(cfg.data_root, 'setups', setup_name)
        setup_info = io.load_setup_info(setup_path)
        cp_sz = setup_info['classifier_crop_sz']
        th, tw = tuple(setup_info['cam_im_sz'])[::-1]
        im = io.torch_imread(join(setup_path, 'cam/raw/ref/img_0002.png'))
        i0, j0 = int(round((im.shape[-2] - th) / 2.)), int(round((im.shape[-1] - tw) / 2.))   # (img_proc.center_crop)
        cam_scene = im[..., i0:i0 + th, j0:j0 + tw].to(device)
        imagenet_labels = load_imagenet_labels(join(cfg.data_root, 'imagenet1000_clsidx_to_labels.txt'))
        target_labels = load_imagenet_labels(join(cfg.data_root, 'imagenet10_clsidx_to_labels.txt'))
        target_idx = list(dict(itertools.islice(target_labels.items(), 10)).keys())
        model.eval()
        for param in model.parameters():
            param.requires_grad = False
        for classifier_name in cfg.classifier_names:
            classifier = classifiers[classifier_name]
            with torch.no_grad():
                raw_score, _, _ = classifier(cam_scene, cp_sz)
            true_idx = int(raw_score[0].argmax())   # (pred_idx[0, 0] of the sorted result; also for a Classifier made with sort_results=False)
            grid = [(loss, d_thr) for loss in cfg.stealth_losses for d_thr in cfg.d_threshes]
            if name == 'SPAA':
                configs = [c for loss, d_thr in grid for c in ((loss, d_thr, True, target_idx), (loss, d_thr, False, [true_idx]))]
                res = spaa_sweep(model, classifier, imagenet_labels, cam_scene, setup_info, device, configs, iters=iters)
                res = {g: (res[2 * k], res[2 * k + 1]) for k, g in enumerate(grid)}
            else:
                from .perc_al import perc_al_compennet_pp
                res = {(loss, d_thr): tuple(perc_al_compennet_pp(model, classifier, imagenet_labels, t, tg, cam_scene, d_thr, device,
                                                                 setup_info) for t, tg in ((target_idx, True), ([true_idx], False)))
                       for loss, d_thr in grid}
            for (loss, d_thr), ((cam_tar, prj_tar), (cam_untar, prj_untar)) in res.items():
                folder = join(attacker_cfg_str, loss, str(d_thr), classifier_name)
                io.save_imgs(torch.cat((cam_tar, cam_untar), 0), join(setup_path, 'cam/infer/adv', folder))
                io.save_imgs(torch.cat((prj_tar, prj_untar), 0), join(setup_path, 'prj/adv', folder))
    return cfg


def _run_one_pixel_de(cfg, models, classifiers, capture):
    """projector_based_attack.py:69-73,110-142: Nichols & Jasper's projector-based One-pixel DE attacker on one setup.  Per classifier
    one untargeted attack on the scene's top-1 (popsize 50) and ten targeted ones (popsize 10), pixel_size 41, 4 generations, one after
    another on numpy's global RNG stream as in the reference (the untargeted attack first; it is saved last, as img_0011).  Projector
    images go under prj/adv/One-pixel_DE/-/-/<classifier>/; captures of a real `capture` under cam/raw/adv/..., those of
    capture='model' under cam/infer/adv/... (they are inferred: the real ones are still made by projecting prj/adv).
    An optional cfg.maxiter replaces the reference's hard-coded 4 generations."""
    import itertools
    import random
    from os.path import join
    from . import io
    from .classifier import load_imagenet_labels
    from .img_proc import center_crop, expand_4d
    from .models import PCNet
    from .one_pixel_attacker import ProjectorOnePixelAttacker, SimulatedCapture
    if len(cfg.setup_list) != 1:
        raise ValueError('One-pixel_DE: cfg.setup_list must hold exactly one setup (the projector and the camera see one scene), got '
                         f'{list(cfg.setup_list)}')
    if capture != 'model' and not callable(capture):
        raise ValueError("capture must be 'model' or a function setup_info -> capture callable")
    setup_name = cfg.setup_list[0]
    missing = [c for c in cfg.classifier_names if c not in (classifiers or {})]
    if missing:
        raise ValueError(f'run_projector_based_attack: pass classifiers={{name: spaa_amd.Classifier}} for {missing} '
                         '(weights cannot be downloaded here)')
    np.random.seed(0)   # (ut.reset_rng_seeds(0); DE draws from numpy's global state)
    random.seed(0)
    torch.manual_seed(0)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(0)
    setup_path = join(cfg.data_root, 'setups', setup_name)
    setup_info = io.load_setup_info(setup_path)
    cp_sz = setup_info['classifier_crop_sz']
    cam_scene = center_crop(io.torch_imread(join(setup_path, 'cam/raw/ref/img_0002.png')), tuple(setup_info['cam_im_sz'])[::-1])
    if isinstance(capture, str):
        model = (models or {}).get(setup_name)
        if not isinstance(model, PCNet):
            raise ValueError(f"run_projector_based_attack: capture='model' needs models={{{setup_name!r}: trained PCNet}}, got "
                             f'{type(model).__name__}')
        model.eval()
        for param in model.parameters():
            param.requires_grad = False
        cap, cam_kind = SimulatedCapture(model, cam_scene), 'cam/infer/adv'
    else:
        cap, cam_kind = capture(setup_info), 'cam/raw/adv'
    imagenet_labels = load_imagenet_labels(join(cfg.data_root, 'imagenet1000_clsidx_to_labels.txt'))
    target_labels = load_imagenet_labels(join(cfg.data_root, 'imagenet10_clsidx_to_labels.txt'))
    n = 10
    target_idx = list(dict(itertools.islice(target_labels.items(), n)).keys())
    one_pixel_de = ProjectorOnePixelAttacker(imagenet_labels, setup_info, capture=cap)
    im_prj_org = setup_info['prj_brightness'] * torch.ones(3, *setup_info['prj_im_sz'])
    one_pixel_de.im_prj_org, one_pixel_de.im_cam_org = im_prj_org, cam_scene
    attacker_cfg_str = to_attacker_cfg_str('One-pixel_DE')[0]
    for stealth_loss in cfg.stealth_losses:
        for d_thr in cfg.d_threshes:
            for classifier_name in cfg.classifier_names:
                folder = join(attacker_cfg_str, stealth_loss, str(d_thr), classifier_name)
                cam_path, prj_path = join(setup_path, cam_kind, folder), join(setup_path, 'prj/adv', folder)
                classifier = classifiers[classifier_name]
                with torch.no_grad():
                    raw_score, p, _ = classifier(cam_scene, cp_sz)
                true_idx = int(raw_score[0].argmax())   # (p.argmax() of the unsorted result; also for a sorting classifier)
                true_label = imagenet_labels[true_idx]
                print(f'\n-------------------- [One-pixel_DE] attacking [{classifier_name}], original prediction: ({true_label}, '
                      f'p={p.max():.2f}), Loss: [{stealth_loss}], d_thr: [{d_thr}] --------')
                print(f'[Untargeted] attacking [{classifier_name}]...')
                _, prj_untar, cam_untar = one_pixel_de(im_prj_org, classifier, False, target_idx=true_idx, pixel_count=1, pixel_size=41,
                                                       maxiter=cfg.get('maxiter', 4), popsize=50, verbose=True, true_label=true_label)
                for i in range(n):
                    print(f'\n[ Targeted ] attacking [{classifier_name}], target: ({imagenet_labels[target_idx[i]]})...')
                    _, prj_tar, cam_tar = one_pixel_de(im_prj_org, classifier, True, target_idx=target_idx[i], pixel_count=1,
                                                       pixel_size=41, maxiter=cfg.get('maxiter', 4), popsize=10, verbose=True,
                                                       true_label=true_label)
                    io.save_imgs(expand_4d(cam_tar), cam_path, idx=i)
                    io.save_imgs(expand_4d(prj_tar), prj_path, idx=i)
                io.save_imgs(expand_4d(cam_untar), cam_path, idx=n)
                io.save_imgs(expand_4d(prj_untar), prj_path, idx=n)
    if cam_kind == 'cam/raw/adv':
        print(f'\nThe next step is to inspect the camera-captured adversarial projections in {join(setup_path, cam_kind, attacker_cfg_str)}')
    else:
        print(f'\nThe next step is to project and capture [One-pixel_DE] generated adversarial projections in '
              f'{join(setup_path, "prj/adv", attacker_cfg_str)}')
    return cfg


def project_capture_real_attack(cfg, *, capture, models=None):
    """projector_based_attack.py:151-166 (steps 5.2 / 6.2 of the reference's main.py): project every adversarial image of
    <setup>/prj/adv/<attacker_cfg_str>/<loss>/<d_thr>/<classifier> and write its capture to the same folder under cam/raw/adv, as
    img_%04d.png counted in the sorted order of the projector images.  SPAA and PerC-AL+CompenNet++ only, and exactly one setup
    (ValueError otherwise; the reference asserts).  `capture` follows _run_one_pixel_de's convention: a function setup_info ->
    (im_prj uint8 [3,Hp,Wp] -> im_cam float [3,Hc,Wc]) for a real ProCams pair, or 'model': models[setup] (a trained PCNet) stands in
    for the projector and the camera through SimulatedCapture with the camera's 8-bit step.  A configured folder without projector
    images raises ValueError."""
    import os
    from os.path import join
    from . import io
    from .img_proc import center_crop, expand_4d
    name = cfg.attacker_name
    if name not in ('SPAA', 'PerC-AL+CompenNet++'):
        raise ValueError(f'{name} not supported, One-pixel_DE does not use this function!')
    if len(cfg.setup_list) != 1:
        raise ValueError(f'cfg.setup_list must hold exactly one setup (the projector and the camera see one scene), got '
                         f'{list(cfg.setup_list)}')
    if capture != 'model' and not callable(capture):
        raise ValueError("capture must be 'model' or a function setup_info -> capture callable")
    setup_name = cfg.setup_list[0]
    setup_path = join(cfg.data_root, 'setups', setup_name)
    setup_info = io.load_setup_info(setup_path)
    attacker_cfg_str = to_attacker_cfg_str(name)[0]
    folders = [join(attacker_cfg_str, loss, str(d_thr), c) for loss in cfg.stealth_losses for d_thr in cfg.d_threshes
               for c in cfg.classifier_names]
    for folder in folders:
        if not _nonempty(join(setup_path, 'prj/adv', folder)):
            raise ValueError(f'project_capture_real_attack: no projector images in {join(setup_path, "prj/adv", folder)}')
    if isinstance(capture, str):
        from .models import PCNet
        from .one_pixel_attacker import SimulatedCapture
        model = (models or {}).get(setup_name)
        if not isinstance(model, PCNet):
            raise ValueError(f"project_capture_real_attack: capture='model' needs models={{{setup_name!r}: trained PCNet}}, got "
                             f'{type(model).__name__}')
        model.eval()
        for param in model.parameters():
            param.requires_grad = False
        cam_scene = center_crop(io.torch_imread(join(setup_path, 'cam/raw/ref/img_0002.png')), tuple(setup_info['cam_im_sz'])[::-1])
        cap = SimulatedCapture(model, cam_scene, quantize=True)
    else:
        cap = capture(setup_info)
    for folder in folders:
        prj_path, cam_path = join(setup_path, 'prj/adv', folder), join(setup_path, 'cam/raw/adv', folder)
        for i, fn in enumerate(sorted(os.listdir(prj_path))):
            im_prj = torch.from_numpy(io._imread_rgb(join(prj_path, fn)).transpose(2, 0, 1).copy())
            io.save_imgs(expand_4d(cap(im_prj).detach().float()), cam_path, idx=i)
    print(f'\nThe camera-captured adversarial projections are in {join(setup_path, "cam/raw/adv", attacker_cfg_str)}')
    return cfg


def attack_results(ret, t, imgnet_labels, im_gray, prj_adv, cam_scene, cam_infer, cam_real, prj_im_sz, cp_sz):
    """projector_based_attack.py:362-414: the result montage of attack `t` as a float [3,Hm,Wm] image (spaa_amd.montage's bytes
    divided by 255).  ret['scene' / 'infer' / 'real'] = the classifier tuples (raw, p_sorted, idx_sorted); the L2 values come from
    metrics.l2_norm.  The tiles have prj_adv's own size (Hp, Wp): the reference passes prj_im_sz, which is (w, h), as (h, w), and so
    works for square projectors only; `prj_im_sz` is not used.  GPU only."""
    from . import metrics as M
    from .img_proc import center_crop
    from .montage import attack_montages, attack_texts
    for name, x in (('prj_adv', prj_adv), ('cam_scene', cam_scene), ('cam_infer', cam_infer), ('cam_real', cam_real)):
        if not x.is_cuda:
            raise RuntimeError(f'attack_results builds the montage on the GPU only (no CPU fallback): {name} is on {x.device}')
    scene = cam_scene.reshape(-1, *cam_scene.shape[-3:])[0]
    gray = im_gray.reshape(-1, *im_gray.shape[-3:])[0]
    scene_cp = center_crop(scene, cp_sz)
    l2 = (M.l2_norm(prj_adv[t], gray.to(prj_adv.device).expand_as(prj_adv[t])), M.l2_norm(center_crop(cam_infer[t], cp_sz), scene_cp),
          M.l2_norm(center_crop(cam_real[t], cp_sz), scene_cp))

    def top1(key, row):
        return imgnet_labels[int(ret[key][2][row, 0])], float(ret[key][1][row, 0])
    texts = attack_texts(t, top1('scene', 0), top1('infer', t), top1('real', t), l2)
    im = attack_montages(scene, prj_adv[t:t + 1], cam_infer[t:t + 1], cam_real[t:t + 1], cp_sz, [texts])[0]
    return im.float() / torch.full((), 255.0, device=im.device)     # (a true division: `/ 255` multiplies by 1 / 255 on the GPU)


# ---------------------------------------------------------------------------------------------------------------------------------
# The summary step (projector_based_attack.py:417-614): success rates and image metrics of every attack configuration of a setup.
SUMMARY_STEALTH_LOSSES = ['caml2', 'camdE', 'camdE_caml2', '-']
SUMMARY_D_THRESHES = [5, 7, 9, 11, '-']
SUMMARY_CLASSIFIERS = ['inception_v3', 'resnet18', 'vgg16']
SUMMARY_CHUNK = 64   # images per classifier launch in the summary (the last chunk is padded: one engine geometry per image size)
_PHASES = ['Valid', 'prj', 'infer', 'real']
_METRICS = ['PSNR', 'RMSE', 'SSIM', 'L2', 'Linf', 'dE']
SUMMARY_COLUMNS = (['Setup', 'Attacker', 'Stealth_loss', 'd_thr', 'Classifier', 'T.top-1_infer', 'T.top-5_infer', 'T.top-1_real',
                    'T.top-5_real', 'U.top-1_infer', 'U.top-1_real'] + [_PHASES[0] + '_' + m for m in _METRICS] +
                   [f'{g}.{x}_{m}' for g in ('T', 'U', 'All') for x in _PHASES[1:] for m in _METRICS])


def attack_success(idx_infer, idx_real, idx_scene, target_idx):
    """projector_based_attack.py:493-506: (T.top-1_infer, T.top-5_infer, T.top-1_real, T.top-5_real, U.top-1_infer, U.top-1_real)
    from class indices sorted by descending probability ([n + 1, >= 5]: rows 0..n-1 the targeted attacks on `target_idx`, row n
    the untargeted one) and the scene's (`idx_scene[0, 0]` is its top-1).  Targeted rates are fractions, untargeted flags 0/1."""
    n = len(target_idx)
    idx_infer, idx_real, idx_scene = np.asarray(idx_infer), np.asarray(idx_real), np.asarray(idx_scene)
    t1_infer = np.count_nonzero(idx_infer[:n, 0] == target_idx) / n
    t5_infer = np.count_nonzero([target_idx[i] in idx_infer[i, :5] for i in range(n)]) / n
    t1_real = np.count_nonzero(idx_real[:n, 0] == target_idx) / n
    t5_real = np.count_nonzero([target_idx[i] in idx_real[i, :5] for i in range(n)]) / n
    true_idx = idx_scene[0, 0]
    return (t1_infer, t5_infer, t1_real, t5_real, int(np.count_nonzero(idx_infer[n, 0] != true_idx)),
            int(np.count_nonzero(idx_real[n, 0] != true_idx)))


def write_stats(table, path):
    """The reference's table files: tab-separated, 4 decimals (stats.txt, stats_all.txt)."""
    table.to_csv(path, index=False, float_format='%.4f', sep='\t')


def _sorted_classes(classifier, ims, crop_sz, chunk=None, top1=None):
    """Class indices sorted by descending softmax probability (classifier.py:64-72) of every image of `ims` (a list of [b,3,H,W]
    tensors): images of one size go through the classifier in equal chunks of at most SUMMARY_CHUNK, the last one padded with
    zeros (one engine geometry per size).  `top1`: a list of len(ims) slots that receives each image's largest probability
    (float32 arrays, from the same softmax)."""
    chunk = chunk or SUMMARY_CHUNK
    out = [None] * len(ims)
    by_shape = {}
    for k, t in enumerate(ims):
        by_shape.setdefault(tuple(t.shape[1:]), []).append(k)
    for shape, ks in by_shape.items():
        stack = torch.cat([ims[k] for k in ks])
        b = -(-stack.shape[0] // -(-stack.shape[0] // chunk))   # (the fewest chunks of at most `chunk`, padding < their number)
        probs = []
        for s in range(0, stack.shape[0], b):
            part = stack[s:s + b]
            m = part.shape[0]
            if m < b:
                part = torch.cat((part, part.new_zeros(b - m, *shape)))
            with torch.no_grad():
                raw = classifier(part, crop_sz)[0]
                probs.append(torch.softmax(raw.detach(), dim=1)[:m].cpu())
        p_sorted, idx = torch.cat(probs).sort(descending=True)
        p_sorted, idx = p_sorted.numpy(), idx.numpy()
        a = 0
        for k in ks:
            out[k] = idx[a:a + ims[k].shape[0]]
            if top1 is not None:
                top1[k] = p_sorted[a:a + ims[k].shape[0], 0]
            a += ims[k].shape[0]
    return out


def _nonempty(d):
    import os
    return os.path.exists(d) and len(os.listdir(d)) > 0


MONTAGE_CHUNK = 264   # montages per attack_montages call in the summary (24 configurations; bounds the output buffer, ~300 MB at 256^2 tiles)


def summarize_single_attacker(attacker_name, data_root, setup_list, device='cuda', device_ids=[0], *, classifiers=None, montages=False,
                              gpu_decode=False):
    """projector_based_attack.py:417-574: per setup, one row per attack configuration (stealth loss x d_thr x classifier) of
    `attacker_name` found on disk -- targeted top-1 / top-5 and untargeted top-1 success of the inferred and the real
    camera-captured attacks, and PSNR / RMSE / SSIM / L2 / L_inf / dE2000 of the projector images (vs the grey illumination), the
    inferred and the captured images (centre-cropped, vs the centre-cropped scene) over the targeted (T), untargeted (U) and all
    (All) attacks; <setup>/ret/<attacker_cfg_str>/stats.txt as the reference writes it.  Returns the last setup's DataFrame.

    `classifiers`: classifier name -> spaa_amd.Classifier (the reference builds them from downloaded weights); a configuration
    present on disk whose classifier is not given raises ValueError.  Differences from the reference:
      * a missing or empty folder skips that configuration only (the reference leaves the classifier loop at the first one);
      * the Valid_* columns are NaN, with a note, when the validation inferences are not on disk (this project's trainers do not
        write */infer/test);
      * no stats.xlsx (no Excel engine is a dependency);
      * the result montages (attack_results, <setup>/ret/<attacker_cfg_str>/<loss>/<d_thr>/<classifier>/img_0001..0011.png) are
        written with `montages=True` only.  They come from spaa_amd.montage: all montages of a setup from ONE attack_montages call
        (split only every MONTAGE_CHUNK montages to bound memory), with the labels' top-1 probabilities from the softmax computed
        for the success rates and the L2 values from the img_stats sums.  Their text is a bitmap font at the tiles' edges and the
        colour map a restatement of Jet (spaa_amd/montage.py); the tiles have the projector images' own size.
      * `gpu_decode=True` decodes the attack results and the validation pair on `device` (io.torch_imread_mt(..., device=): one
        batch per folder, the same values) instead of through Pillow one file after the other.
    Mechanism: all images of a setup are loaded at once, each classifier sees them in chunks of SUMMARY_CHUNK, and every image
    metric of the setup comes from ONE metrics.img_stats launch, grouped on the host with metrics.dists_from_sums."""
    import itertools
    import os
    from os.path import join
    import pandas as pd
    from . import io
    from . import metrics as M
    from .classifier import load_imagenet_labels
    if attacker_name not in ATTACKERS:
        raise ValueError(f'{attacker_name} not supported!')
    device = torch.device(device)
    attacker_cfg_str, model_cfg_str = to_attacker_cfg_str(attacker_name)
    dl_based = attacker_name in ('SPAA', 'PerC-AL+CompenNet++')
    n = 10   # 10 targeted attacks and 1 untargeted attack
    target_labels = load_imagenet_labels(join(data_root, 'imagenet10_clsidx_to_labels.txt'))
    target_idx = list(dict(itertools.islice(target_labels.items(), n)).keys())
    table = pd.DataFrame(columns=SUMMARY_COLUMNS)
    for setup_name in setup_list:
        setup_path = join(data_root, 'setups', setup_name)
        print(f'\nCalculating stats of [{attacker_name}] on [{setup_path}]')
        setup_info = io.load_setup_info(setup_path)
        cp_sz = tuple(setup_info['classifier_crop_sz'])
        gray = float(setup_info['prj_brightness'])
        cam_scene = io.torch_imread(join(setup_path, 'cam/raw/ref/img_0002.png')).to(device)

        cfgs = []   # (stealth_loss, d_thr, classifier_name, prj_adv_path, cam_real_path, cam_infer_path)
        for stealth_loss, d_thr, classifier_name in itertools.product(SUMMARY_STEALTH_LOSSES, SUMMARY_D_THRESHES, SUMMARY_CLASSIFIERS):
            folder = join(attacker_cfg_str, stealth_loss, str(d_thr), classifier_name)
            dirs = [join(setup_path, 'prj/adv', folder), join(setup_path, 'cam/raw/adv', folder)]
            if dl_based:
                dirs.append(join(setup_path, 'cam/infer/adv', folder))
            missing = next((d for d in dirs if not _nonempty(d)), None)
            if missing is not None:
                print(f'No such folder/images: {missing}\n'
                      f'Maybe [{attacker_name}] has no [{join(stealth_loss, str(d_thr), classifier_name)}] attack cfg, or you forget '
                      'to project and capture.\n')
                continue
            cfgs.append((stealth_loss, d_thr, classifier_name, *dirs))
        no_clf = sorted({c[2] for c in cfgs if c[2] not in (classifiers or {})}, key=SUMMARY_CLASSIFIERS.index)
        if no_clf:
            raise ValueError(f'summarize_single_attacker: [{setup_name}] has attack results for {no_clf}: pass classifiers={{name: '
                             'spaa_amd.Classifier} for them (weights cannot be downloaded here)')

        rd = (lambda d: io.torch_imread_mt(d, device=device)) if gpu_decode else (lambda d: io.torch_imread_mt(d).to(device))
        prj = [rd(c[3]) for c in cfgs]
        real = [rd(c[4]) for c in cfgs]
        infer = [rd(c[5]) for c in cfgs] if dl_based else real
        for c, p, r, i in zip(cfgs, prj, real, infer):
            if not p.shape[0] == r.shape[0] == i.shape[0] > n:
                raise ValueError(f'{join(*map(str, c[:3]))}: expected the same number (> {n}) of prj / cam images, got '
                                 f'{p.shape[0]} / {r.shape[0]} / {i.shape[0]}')

        # classification: per classifier, the scene and every inferred / captured image of its configurations
        idx, top1 = {}, {}   # (config, 'scene' / 'infer' / 'real') -> sorted class indices, top-1 probabilities
        for cname in SUMMARY_CLASSIFIERS:
            ks = [k for k, c in enumerate(cfgs) if c[2] == cname]
            if not ks:
                continue
            clf = classifiers[cname]
            ims = [cam_scene[None]] + [infer[k] for k in ks] + ([real[k] for k in ks] if dl_based else [])
            top = [None] * len(ims)
            res = _sorted_classes(clf, ims, cp_sz, top1=top)
            for j, k in enumerate(ks):
                idx[k, 'scene'], top1[k, 'scene'] = res[0], top[0]
                idx[k, 'infer'], top1[k, 'infer'] = res[1 + j], top[1 + j]
                jr = 1 + len(ks) + j if dl_based else 1 + j
                idx[k, 'real'], top1[k, 'real'] = res[jr], top[jr]

        # image metrics: one launch over every pair of the setup
        xs, ys, pairs, spans = [], [cam_scene.reshape(-1)], [], {}
        xoff, yoff = 0, cam_scene.numel()

        def add(key, x, ps_fn):
            nonlocal xoff
            ps = ps_fn(xoff)
            xs.append(x.reshape(-1))
            xoff += x.numel()
            spans[key] = list(range(len(pairs), len(pairs) + len(ps)))
            pairs.extend(ps)

        for k in range(len(cfgs)):
            add((k, 'prj'), prj[k], lambda o, t=prj[k]: M.stack_pairs(t.shape[0], t.shape[-2:], x_off=o, rgb=(gray,) * 3))
            for kind, t in (('infer', infer[k]), ('real', real[k])) if dl_based else (('real', real[k]),):
                add((k, kind), t, lambda o, t=t: M.stack_pairs(t.shape[0], t.shape[-2:], cam_scene.shape[-2:], crop=cp_sz, x_off=o,
                                                                  y_off=0, y_step=0))
            if not dl_based:
                spans[k, 'infer'] = spans[k, 'real']
        valid = None
        if attacker_name == 'One-pixel_DE':
            valid = (0,) * 6
        else:
            if attacker_name == 'SPAA':
                vx, vy, vcrop = join(setup_path, 'cam/infer/test', model_cfg_str), join(setup_path, 'cam/raw/test'), cp_sz
            else:
                vx, vy, vcrop = join(setup_path, 'prj/infer/test', model_cfg_str), join(data_root, 'prj_share/test'), None
            if _nonempty(vx) and _nonempty(vy):
                a, b = rd(vx), rd(vy)
                if a.shape[0] != b.shape[0]:
                    raise ValueError(f'{vx} and {vy} hold {a.shape[0]} and {b.shape[0]} images')
                add('valid', a, lambda o: M.stack_pairs(a.shape[0], a.shape[-2:], b.shape[-2:], crop=vcrop, x_off=o, y_off=yoff))
                ys.append(b.reshape(-1))
            else:
                print(f'No validation inferences ({vx} and {vy}): the Valid_* columns are NaN')
                valid = (float('nan'),) * 6
        if pairs:
            with _lib.on_device(device):
                sums, npix = M.img_stats(torch.cat(xs), torch.cat(ys), pairs)
        if valid is None:
            valid = M.dists_from_sums(sums, npix, spans['valid'])

        rows = []
        for k, (stealth_loss, d_thr, cname, *_) in enumerate(cfgs):
            groups = [M.dists_from_sums(sums, npix, spans[k, kind][sel]) for sel in (slice(0, n), slice(n, n + 1), slice(None))
                      for kind in ('prj', 'infer', 'real')]
            rows.append([setup_name, attacker_cfg_str, stealth_loss, d_thr, cname,
                         *attack_success(idx[k, 'infer'], idx[k, 'real'], idx[k, 'scene'], target_idx), *valid,
                         *itertools.chain.from_iterable(groups)])
        table = pd.DataFrame(rows, columns=SUMMARY_COLUMNS) if rows else pd.DataFrame(columns=SUMMARY_COLUMNS)

        print(f'\n-------------------- [{attacker_name}] results on [{setup_name}] --------------------')
        print(table.to_string(index=False, float_format='%.4f'))
        print('-------------------------------------- End of result table ---------------------------\n')
        ret_path = join(setup_path, 'ret', attacker_cfg_str)
        os.makedirs(ret_path, exist_ok=True)
        write_stats(table, join(ret_path, 'stats.txt'))

        if montages and cfgs:
            from .montage import attack_montages, attack_texts
            if len({tuple(t.shape[1:]) for t in prj}) != 1 or len({tuple(t.shape[1:]) for t in infer}) != 1 or \
                    len({tuple(t.shape[1:]) for t in real}) != 1:
                raise ValueError(f'summarize_single_attacker: the montages of [{setup_name}] need images of one size per kind')
            imagenet_labels = load_imagenet_labels(join(data_root, 'imagenet1000_clsidx_to_labels.txt'))
            m = n + 1

            def label(k, kind, row):
                return imagenet_labels[int(idx[k, kind][row, 0])], float(top1[k, kind][row])

            def l2(k, kind, t):
                j = spans[k, kind][t]
                return sums[j, 2] / npix[j] * 255
            texts = [attack_texts(t, label(k, 'scene', 0), label(k, 'infer', t), label(k, 'real', t),
                                  (l2(k, 'prj', t), l2(k, 'infer', t), l2(k, 'real', t)))
                     for k in range(len(cfgs)) for t in range(m)]
            per = max(1, MONTAGE_CHUNK // m)           # whole configurations per call
            for a in range(0, len(cfgs), per):
                ks = range(a, min(a + per, len(cfgs)))
                with _lib.on_device(device):
                    ims = attack_montages(cam_scene, torch.cat([prj[k][:m] for k in ks]), torch.cat([infer[k][:m] for k in ks]),
                                          torch.cat([real[k][:m] for k in ks]), cp_sz, texts[a * m:(a + len(ks)) * m])
                for j, k in enumerate(ks):
                    io.save_imgs(ims[j * m:(j + 1) * m], join(setup_path, 'ret', attacker_cfg_str, cfgs[k][0], str(cfgs[k][1]), cfgs[k][2]))
    return table


def summarize_all_attackers(attacker_names, data_root, setup_list, recreate_stats_and_imgs=False, *, classifiers=None, montages=False):
    """projector_based_attack.py:577-614: concatenate <setup>/ret/<attacker_cfg_str>/stats.txt of every setup and attacker
    (recreated first by summarize_single_attacker when `recreate_stats_and_imgs`), and the pivot table of the SPAA paper's
    Table 1 (supplementary Table 2).  Writes <data_root>/setups/stats_all.txt and pivot_table_all.txt (tab-separated, 4
    decimals; the reference's .xlsx copies are not written: no Excel engine is a dependency).  `montages=True` is handed to
    summarize_single_attacker when the stats are recreated (the result montages).  Returns (table, pivot_table)."""
    import warnings
    from os.path import join
    import pandas as pd
    table = []
    for setup_name in setup_list:
        setup_path = join(data_root, 'setups', setup_name)
        for attacker_name in attacker_names:
            attacker_cfg_str = to_attacker_cfg_str(attacker_name)[0]
            ret_path = join(setup_path, 'ret', attacker_cfg_str)
            print(f'\nGathering stats of {ret_path}')
            if recreate_stats_and_imgs:
                summarize_single_attacker(attacker_name=attacker_name, data_root=data_root, setup_list=[setup_name],
                                          classifiers=classifiers, montages=montages)
            table.append(pd.read_csv(join(ret_path, 'stats.txt'), index_col=None, header=0, sep='\t'))
    table = pd.concat(table, axis=0, ignore_index=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', FutureWarning)   # (pandas' note on aggfunc=np.mean: the reference's call is kept as it is)
        pivot_table = pd.pivot_table(table, values=['T.top-1_real', 'T.top-5_real', 'U.top-1_real', 'T.real_L2', 'T.real_Linf',
                                                    'T.real_dE', 'T.real_SSIM', 'All.real_L2', 'All.real_Linf', 'All.real_dE',
                                                    'All.real_SSIM'],
                                     index=['Attacker', 'd_thr', 'Stealth_loss', 'Classifier'], aggfunc=np.mean, sort=False)
    pivot_table = pivot_table.sort_index(level=[0, 1], ascending=[False, True])   # to match SPAA Table order
    write_stats(table, join(data_root, 'setups/stats_all.txt'))
    pivot_table.to_csv(join(data_root, 'setups/pivot_table_all.txt'), float_format='%.4f', sep='\t', index=True)
    return table, pivot_table
