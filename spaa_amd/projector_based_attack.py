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
import ctypes
import dataclasses
import math
import os
import warnings

import torch

from . import _lib
from .models import PCNet, to_nhwc4, to_nchw
from .classifier import Attention, Classifier

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


def _require_gpu(device, who):
    """torch.device(device), which must be a GPU: `who` names the entry point in the error."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'spaa_amd.{who} runs on the GPU only (no CPU fallback); got device={device}')
    return dev


def _scene_batch(cam_scene, B):
    """`cam_scene` ([3,H,W], [1,3,H,W] or [B,3,H,W]) as float [B,3,H,W]; one scene is broadcast (a view).  Any other shape comes back
    as it is: the caller checks it and words its own error."""
    sc = cam_scene.detach().float()
    while sc.ndim < 4:
        sc = sc[None]
    return sc.expand(B, -1, -1, -1) if sc.ndim == 4 and sc.shape[0] == 1 else sc


class AttackState:
    """Device-side state of one batched attack (everything the loop touches, allocated once)."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage='f32', attention=None,
                 transfer=None):
        """`storage`: 'f32' (default; results identical to the reference to rounding) or 'f16' (fp16-storage mode of
        BASELINE.json configs[4]: network activations and their gradients are fp16 in HBM, images / losses / dE2000 /
        norms / accumulation fp32).  `attention`: an Attention (fp32 storage): every classifier engine of the state
        weights its gradient image by its own Grad-CAM map; attention_maps() returns the maps of the last iteration.  `transfer`: a
        Transfer (fp32 storage): the adversarial step follows the smoothed, momentum-accumulated gradient image
        `momentum` [B,Hp,Wp,4] instead of the raw one."""
        _attention_checked(attention, storage, type(self).__name__)
        _transfer_checked(transfer, storage, type(self).__name__)
        self.storage, self.attention, self.transfer = storage, attention, transfer
        dev = _require_gpu(device, 'spaa')
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
        cam_scene = _scene_batch(cam_scene, B)
        if cam_scene.shape[0] != B:
            raise ValueError('cam_scene must hold 1 or len(target_idx) scenes')
        self.eng = pcnet.engine(B, prj_sz, owner=self, storage=self.storage)
        Hc, Wc = self.eng.Hc, self.eng.Wc
        if tuple(cam_scene.shape[-2:]) != (Hc, Wc):
            raise ValueError(f'cam_scene is {tuple(cam_scene.shape[-2:])} but PCNet outputs {(Hc, Wc)}')
        self.clf = classifier.engine(B, (Hc, Wc), self.cp_sz, owner=self, storage=self.storage)
        if self.attention is not None:
            self.clf.attention_buffers(self.attention.rollout)
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
        if self.transfer is not None:
            # the momentum image m (zero: the first adversarial step is the smoothed gradient's), the smoothed gradient t and its |.|
            # sums per tile of the blur launch; the taps travel in the launch's arguments
            self.momentum = torch.zeros(B, Hp, Wp, 4, device=dev)
            self.transfer_t = torch.zeros(B, Hp, Wp, 4, device=dev)
            self.transfer_tiles = _lib.load().spaa_transfer_tiles(Hp, Wp)
            self.transfer_l1 = torch.zeros(B, self.transfer_tiles, device=dev)
            taps = self.transfer.weights().tolist()
            self._transfer_taps = (ctypes.c_float * len(taps))(*taps)

    def _shape_direction(self, gx, partial_ss, npartial):
        """The transferable step, directly before spaa_step_and_track_n: for every sample on the adversarial step the
        gradient image `gx` becomes the momentum image m <- mu m + t / |t|_1, t the Gaussian-smoothed gx, and its row of `partial_ss`
        the partial sums of ||m||^2; samples on the colour step keep gx, partial_ss and m bit for bit.  Two launches, no host read;
        without `transfer` none."""
        tr = self.transfer
        if tr is None:
            return
        p = _lib.ptr
        Hp, Wp = self.x.shape[1:3]
        _lib.call('spaa_transfer_blur', p(gx), p(self.state), self._transfer_taps, tr.radius, p(self.transfer_t), p(self.transfer_l1),
                  self.B, Hp, Wp)
        _lib.call('spaa_transfer_momentum', p(self.transfer_t), p(self.transfer_l1), self.transfer_tiles, float(tr.momentum),
                  p(self.state), p(self.momentum), p(gx), p(partial_ss), int(npartial), self.B, self.HWp)

    def _per_sample(self, targeted, d_thr, table=False):
        """The batch's (targeted, d_thr) as scalars when every sample agrees and the loss weights are uniform (the launches of a single
        attack, unchanged); else, or with `table` always, uploads the per-sample table (once per distinct setting: a captured graph
        replays the table it read) and returns None."""
        B = self.B
        tg = [bool(targeted)] * B if _is_scalar(targeted) else [bool(t) for t in targeted]
        dt = [float(d_thr)] * B if _is_scalar(d_thr) else [float(d) for d in d_thr]
        if len(tg) != B or len(dt) != B:
            raise ValueError(f'targeted / d_thr: one value or {B} values')
        if not table and self.caml2_w is not None and all(t == tg[0] for t in tg) and all(d == dt[0] for d in dt):
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

    def _adv_gradient(self):
        """The adversarial loss's gradient at the camera image [B,Hc,Wc,4]: the classifier's backward pass from the seed of the decision."""
        return self.clf.backward(self.g_logits, self.attention, self.target)         # :302 (classifier part)

    def _engine_maps(self, engines):
        if self.attention is None:
            raise RuntimeError('attention_maps(): this attack runs without attention (pass attention=Attention(...))')
        with torch.cuda.device(self.dev):
            return [e.attention_map() for e in engines]

    def attention_maps(self):
        """The Grad-CAM map M of the last iteration in the camera frame, [B, 1, Hc, Wc] in [0, 1] and 0 outside the classifier crop
        (EnsembleAttackState: a list of one per member, MultiViewAttackState: of one per view)."""
        return self._engine_maps([self.clf])[0]

    def trace_entry(self):
        """What spaa()'s `trace` records per iteration (copies; no sync)."""
        return self.state.clone(), self.stats.clone()

    def _backward_step(self, adv_lr, col_lr):
        B, p, y = self.B, _lib.ptr, self._y
        g_adv = self._adv_gradient()
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
        self._shape_direction(gx, self.partial_ss, self.partial_ss.shape[1])
        _lib.call('spaa_step_and_track_n', p(self.x), p(gx), p(self.partial_ss), self.partial_ss.shape[1], p(self.state), float(adv_lr),
                  float(col_lr), p(self.x_best), p(y), p(self.cam_best), B, self.HWp, self.HWc,
                  p(self.clamp_bits) if self.clamp_bits is not None else None)       # :307,315,323-328
        self._bits_version = self.x._version

    def results(self):
        with torch.cuda.device(self.dev):
            return to_nchw(self.cam_best), to_nchw(self.x_best, clamp01=True)        # :337


ENS_MAX = 4   # SPAA_ENS_MAX of include/spaa_hip.h


def _ensemble_members(classifier, storage, who):
    """The members of a list / tuple `classifier`, checked (before anything is allocated or launched): each a spaa_amd.Classifier (no
    foreign-callable route for ensembles), at most ENS_MAX of them, no object twice, one number of classes; fp32 storage."""
    members = [_unwrap(c) for c in classifier]
    if not members:
        raise ValueError(f'{who}: the classifier sequence is empty')
    for c in members:
        if not isinstance(c, Classifier):
            raise TypeError(f'{who}: every member of a classifier ensemble must be a spaa_amd.Classifier, got {type(c).__name__} '
                            '(a foreign callable can only be attacked alone)')
    if len(members) > ENS_MAX:
        raise ValueError(f'{who}: an ensemble holds at most {ENS_MAX} classifiers, got {len(members)}')
    if len({id(c) for c in members}) != len(members):
        raise ValueError(f'{who}: the same Classifier object is listed twice in the ensemble')
    ncls = [c.num_classes for c in members]
    if any(n != ncls[0] for n in ncls):
        raise ValueError(f'{who}: the members of an ensemble must have the same number of classes, got {ncls}')
    if len(members) >= 2 and storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented for an ensemble (the members' unit vectors need a loss "
                                  "scale of their own); use storage='f32'")
    return members


class EnsembleAttackState(AttackState):
    """One batched attack against K = 2..ENS_MAX classifiers that see the same camera image ("Ensemble attack"): AttackState
    with one leased engine per member, the decision over all members (spaa_decide_ens) and, as adversarial cotangent, the weighted sum
    of the members' unit gradient images (spaa_ens_sumsq + spaa_ens_combine).  PCNet's passes, the stealth loss, the colour step, the
    normalised step and the best tracking are AttackState's.  `state[:, 3]` counts the fooled members; each member's top-1 is in
    `ens_state`.  `focus`: a member that is already fooled rests (weight 0) until all are."""

    def __init__(self, pcnet, classifiers, target_idx, cam_scene, stealth_loss, setup_info, device, storage='f32', focus=False,
                 attention=None, transfer=None):
        self.members = _ensemble_members(classifiers, storage, 'EnsembleAttackState')
        if len(self.members) < 2:
            raise ValueError('EnsembleAttackState needs at least two classifiers (AttackState attacks one)')
        self.focus = bool(focus)
        super().__init__(pcnet, self.members[0], target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                         attention=attention, transfer=transfer)

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)   # (leases member 0's engine: self.clf)
        B, K = self.B, len(self.members)
        self.K = K
        self.clfs = [self.clf] + [c.engine(B, (self.eng.Hc, self.eng.Wc), self.cp_sz, owner=self, storage=self.storage)
                                  for c in self.members[1:]]
        if self.attention is not None:
            for e in self.clfs[1:]:
                e.attention_buffers(self.attention.rollout)
        self.ens_g_logits = [self.g_logits] + [torch.zeros_like(self.g_logits) for _ in range(K - 1)]
        self.ens_state = torch.zeros(B, K, 2, dtype=torch.int32, device=dev)
        self.ens_stats = torch.zeros(B, K, 2, device=dev)
        self.ens_w = torch.ones(B, K, device=dev)
        self.ens_partial = torch.zeros(B, K, self.nblk_c, device=dev)
        self.g_adv = torch.zeros(B, self.eng.Hc, self.eng.Wc, 4, device=dev)

    def _forward_decide(self, targeted, d_thr, p_thresh, adv_w):
        B, p = self.B, _lib.ptr
        self._per_sample(targeted, d_thr, table=True)   # (the ensemble decision has the per-sample table form only)
        y = self.eng.forward(self.x, clamp01=True)                                   # :265
        logits = self._member_logits(y)
        self._y, self._uniform = y, False
        if self.any_prjl2:
            _lib.call('spaa_prjl2_fwd', p(self.x), self.gray, p(self.prjl2), B, self.HWp)
        _lib.call('spaa_stealth_loss_fwd_bwd_ps', p(y), p(self.scene4), p(self.scene_lab), p(self.ps_params),
                  self.gs_col / (B * self.HWc), p(self.g_col), None, p(self.partial_loss), B, self.HWc)
        _lib.call('spaa_decide_ens', _lib.ptr_array(logits), self.K, self.clf.ncls, p(self.target), p(self.partial_loss), self.nblk_c,
                  self.HWc, p(self.prjl2) if self.any_prjl2 else None, p(self.ps_params), p(self.ps_flags), float(p_thresh),
                  int(self.focus), p(self.state), p(self.stats), p(self.ens_state), p(self.ens_stats), p(self.ens_w),
                  _lib.ptr_array(self.ens_g_logits), B)

    def _member_logits(self, y):
        """Every member's logits of the camera image y."""
        return [e.forward(y) for e in self.clfs]                                     # :266, once per member

    def _member_gradients(self):
        """Every member's gradient image at the camera image, from its seed of the decision."""
        return [e.backward(g, self.attention, self.target) for e, g in zip(self.clfs, self.ens_g_logits)]   # (each its own map)

    def attention_maps(self):
        return self._engine_maps(self.clfs)

    def _adv_gradient(self):
        gs = _lib.ptr_array(self._member_gradients())
        _lib.call('spaa_ens_sumsq', gs, self.K, _lib.ptr(self.ens_partial), self.B, self.HWc)
        _lib.call('spaa_ens_combine', gs, self.K, _lib.ptr(self.ens_partial), self.nblk_c, _lib.ptr(self.ens_w), _lib.ptr(self.g_adv),
                  self.B, self.HWc)
        return self.g_adv

    def trace_entry(self):
        return super().trace_entry() + (self.ens_state.clone(), self.ens_stats.clone())


VIEWS_MAX = 4   # SPAA_VIEWS_MAX of include/spaa_hip.h


def _view_pcnets(pcnet, cam_scene, who):
    """The views of a list / tuple `pcnet`, checked (before anything is allocated or launched): each a spaa_amd.PCNet, 2 to VIEWS_MAX of
    them, no object twice, and `cam_scene` a list / tuple of as many scenes.  Returns (list of PCNets, list of scenes); a sequence of
    one PCNet is that PCNet: (PCNet, its scene)."""
    views = [_unwrap(m) for m in pcnet]
    for m in views:
        if not isinstance(m, PCNet):
            raise TypeError(f'{who}: every view must be a spaa_amd.PCNet, got {type(m).__name__} (the HIP path has no generic PCNet '
                            'fallback)')
    if not views:
        raise ValueError(f'{who}: the pcnet sequence is empty')
    if len(views) == 1:
        if isinstance(cam_scene, (list, tuple)):
            if len(cam_scene) != 1:
                raise ValueError(f'{who}: {len(cam_scene)} scenes for one view')
            cam_scene = cam_scene[0]
        return views[0], cam_scene
    if len(views) > VIEWS_MAX:
        raise ValueError(f'{who}: a multi-view attack holds at most {VIEWS_MAX} views, got {len(views)}')
    if len({id(m) for m in views}) != len(views):
        raise ValueError(f'{who}: the same PCNet object is listed twice among the views')
    if not isinstance(cam_scene, (list, tuple)) or len(cam_scene) != len(views):
        n = len(cam_scene) if isinstance(cam_scene, (list, tuple)) else 'one tensor'
        raise ValueError(f'{who}: cam_scene must be a list of one scene per view ({len(views)}), got {n}')
    return views, list(cam_scene)


def _views_supported(views, classifier, storage, who):
    """What a multi-view attack does not serve, said before anything is allocated or launched.  `classifier`: as spaa() holds it after
    its own checks (a Classifier, a checked list of several, or anything else)."""
    if isinstance(classifier, list):
        raise NotImplementedError(f'{who}: an ensemble of classifiers against several views is not implemented; attack one '
                                  'classifier from several views, or several classifiers from one')
    if not isinstance(classifier, Classifier):
        raise TypeError(f'{who}: a multi-view attack needs a spaa_amd.Classifier, got {type(classifier).__name__} (a foreign '
                        'callable can only be attacked from one view)')
    if storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented for several views (the views' unit vectors need a "
                                  "loss scale of their own); use storage='f32'")
    sizes = [tuple(m.warping_net.out_size) for m in views]
    if any(sz != sizes[0] for sz in sizes):
        raise ValueError(f'{who}: the views must have the same camera size, got {sizes}')


class MultiViewAttackState(AttackState):
    """One batched attack against V = 2..VIEWS_MAX camera views of the same projector and scene ("Multi-view attack"): one
    projector image x through V PCNets, each with its own scene, and one classifier looking at each of the V camera images.
    AttackState (view 0's engines and buffers are its own) with one leased PCNet engine and one leased engine of the classifier per
    further view, the decision over all views (spaa_decide_views), the V backward passes down to the projector image and their
    combination there (spaa_ens_sumsq + spaa_views_combine): the mean of the views' stealth gradients on the colour step, the weighted
    sum of the views' unit gradient images on the adversarial step.  `state[:, 3]` counts the fooled views; each view's top-1 is in
    `view_state`, its p1, target logit, caml2 and camdE in `view_stats`.  `focus`: a view that is already fooled rests (weight 0) until
    all are."""

    def __init__(self, pcnets, classifier, target_idx, cam_scenes, stealth_loss, setup_info, device, storage='f32', focus=False,
                 attention=None, transfer=None):
        views, scenes = _view_pcnets(pcnets, cam_scenes, 'MultiViewAttackState')
        if not isinstance(views, list):
            raise ValueError('MultiViewAttackState needs at least two views (AttackState attacks one)')
        classifier = _unwrap(classifier)
        _views_supported(views, classifier, storage, 'MultiViewAttackState')
        self.pcnets, self._scenes, self.focus = views, scenes, bool(focus)
        super().__init__(views[0], classifier, target_idx, scenes[0], stealth_loss, setup_info, device, storage=storage,
                         attention=attention, transfer=transfer)

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)   # (view 0: self.eng, self.clf, ...)
        B, V = self.B, len(self.pcnets)
        self.V = V
        Hc, Wc = self.eng.Hc, self.eng.Wc
        # ||g||^2 of the COMBINED gradient comes from spaa_grad_sumsq_ps (a view's adjoint cannot sum it in its epilogue), and the
        # views' backward passes read the clamp gate from x
        self.ss_tiles, self.clamp_bits = 0, None
        self.partial_ss = torch.zeros(B, self.nblk_p, device=dev)
        self.engs, self.clfs = [self.eng], [self.clf]
        self.scene4s, self.scene_labs, self.g_cols, self.gPs = [self.scene4], [self.scene_lab], [self.g_col], [self.gP]
        self.partial_losses, self.view_g_logits, self.cam_bests = [self.partial_loss], [self.g_logits], [self.cam_best]
        for m, sc in zip(self.pcnets[1:], self._scenes[1:]):
            sc = _scene_batch(sc, B)
            if sc.shape[0] != B:
                raise ValueError('every view\'s cam_scene must hold 1 or len(target_idx) scenes')
            eng = m.engine(B, tuple(setup_info['prj_im_sz']), owner=self, storage=self.storage)
            if (eng.Hc, eng.Wc) != (Hc, Wc):
                raise ValueError(f'the views must have the same camera size, got {(Hc, Wc)} and {(eng.Hc, eng.Wc)}')
            if tuple(sc.shape[-2:]) != (Hc, Wc):
                raise ValueError(f'cam_scene is {tuple(sc.shape[-2:])} but PCNet outputs {(Hc, Wc)}')
            scene4 = to_nhwc4(sc.contiguous().to(dev))
            eng.set_scene(scene4)
            lab = torch.zeros_like(scene4)
            _lib.call('spaa_rgb2lab', _lib.ptr(scene4), _lib.ptr(lab), B * Hc * Wc)
            self.engs.append(eng)
            self.clfs.append(classifier.engine(B, (Hc, Wc), self.cp_sz, owner=self, storage=self.storage))
            if self.attention is not None:
                self.clfs[-1].attention_buffers(self.attention.rollout)
            self.scene4s.append(scene4)
            self.scene_labs.append(lab)
            self.g_cols.append(torch.zeros_like(self.g_col))
            self.gPs.append(torch.zeros_like(self.gP))
            self.partial_losses.append(torch.zeros_like(self.partial_loss))
            self.view_g_logits.append(torch.zeros_like(self.g_logits))
            self.cam_bests.append(scene4.clone())
        self.view_state = torch.zeros(B, V, 2, dtype=torch.int32, device=dev)
        self.view_stats = torch.zeros(B, V, 4, device=dev)
        self.view_w = torch.ones(B, V, device=dev)
        self.views_partial = torch.zeros(B, V, self.nblk_p, device=dev)
        self.g = torch.zeros(B, self.x.shape[1], self.x.shape[2], 4, device=dev)
        self._ys = None

    def _forward_decide(self, targeted, d_thr, p_thresh, adv_w):
        B, p = self.B, _lib.ptr
        self._per_sample(targeted, d_thr, table=True)   # (the decision over views has the per-sample table form only)
        ys, logits = [], []
        for v in range(self.V):
            y = self.engs[v].forward(self.x, clamp01=True)                           # :265, once per view
            logits.append(self.clfs[v].forward(y))                                   # :266
            _lib.call('spaa_stealth_loss_fwd_bwd_ps', p(y), p(self.scene4s[v]), p(self.scene_labs[v]), p(self.ps_params),
                      self.gs_col / (B * self.HWc), p(self.g_cols[v]), None, p(self.partial_losses[v]), B, self.HWc)
            ys.append(y)
        self._ys, self._y, self._uniform = ys, ys[0], False
        if self.any_prjl2:
            _lib.call('spaa_prjl2_fwd', p(self.x), self.gray, p(self.prjl2), B, self.HWp)
        _lib.call('spaa_decide_views', _lib.ptr_array(logits), self.V, self.clf.ncls, p(self.target),
                  _lib.ptr_array(self.partial_losses), self.nblk_c, self.HWc, p(self.prjl2) if self.any_prjl2 else None,
                  p(self.ps_params), p(self.ps_flags), float(p_thresh), adv_w / B * self.gs_adv, int(self.focus), p(self.state),
                  p(self.stats), p(self.view_state), p(self.view_stats), p(self.view_w), _lib.ptr_array(self.view_g_logits), B)

    def _backward_step(self, adv_lr, col_lr):
        B, p = self.B, _lib.ptr
        gxs = []
        for v, eng in enumerate(self.engs):
            g_adv = self.clfs[v].backward(self.view_g_logits[v], self.attention, self.target)   # :302 (classifier part), view v's seed and map
            if eng.can_select():
                gxs.append(eng.backward(None, select=(g_adv, self.g_cols[v], self.state), sumsq=None, clamp_bits=None))
            else:
                _lib.call('spaa_select_grad', p(g_adv), p(self.g_cols[v]), p(self.state), p(eng.a['Ypre']), p(self.gPs[v]), B,
                          self.HWc)
                gxs.append(eng.backward(self.gPs[v], sumsq=None, clamp_bits=None))   # :302 / :310 (PCNet part)
        gs = _lib.ptr_array(gxs)
        _lib.call('spaa_ens_sumsq', gs, self.V, p(self.views_partial), B, self.HWp)
        _lib.call('spaa_views_combine', gs, self.V, p(self.views_partial), self.nblk_p, p(self.view_w), p(self.state), p(self.g), B,
                  self.HWp)
        _lib.call('spaa_grad_sumsq_ps', p(self.g), p(self.x), self.gray, p(self.ps_prjl2_scale), p(self.state), p(self.partial_ss), B,
                  self.HWp)
        self._shape_direction(self.g, self.partial_ss, self.nblk_p)
        _lib.call('spaa_step_and_track_n', p(self.x), p(self.g), p(self.partial_ss), self.nblk_p, p(self.state), float(adv_lr),
                  float(col_lr), p(self.x_best), p(self._ys[0]), p(self.cam_best), B, self.HWp, self.HWc, None)   # :307,315,323-328
        _lib.call('spaa_views_track', _lib.ptr_array(self._ys), _lib.ptr_array(self.cam_bests), self.V, p(self.state), B, self.HWc)

    def attention_maps(self):
        return self._engine_maps(self.clfs)

    def trace_entry(self):
        return super().trace_entry() + (self.view_state.clone(), self.view_stats.clone())

    def results(self):
        with torch.cuda.device(self.dev):
            return [to_nchw(c) for c in self.cam_bests], to_nchw(self.x_best, clamp01=True)


JITTER_MAX = 4   # SPAA_JITTER_MAX of include/spaa_hip.h


@dataclasses.dataclass(frozen=True)
class CaptureJitter:
    """What separates a real capture from the inferred one, as ranges of a random perturbation of the camera image (DESIGN.md,
    "Capture-robust attack"): exposure / white balance `gain` (per channel, 1 +- gain) and `offset` (+- offset), a misregistration of
    +- `shift` camera pixels per axis, sensor noise of standard deviation `noise`, the camera's 8-bit step (`quantize`).  `draws`:
    captures attacked at once per iteration (2..4; the first one is the clean capture), `seed`: of the counter-based generator.
    `shift` <= 2 and `noise` <= 0.1 are what the adjoint kernel's border loop and the tests' noise tolerance assume."""
    gain: float = 0.1
    offset: float = 0.03
    shift: float = 0.75
    noise: float = 0.01
    quantize: bool = True
    draws: int = 3
    seed: int = 0

    def __post_init__(self):
        if not 2 <= int(self.draws) <= JITTER_MAX:
            raise ValueError(f'CaptureJitter: draws must be 2..{JITTER_MAX}, got {self.draws}')
        for name in ('gain', 'offset', 'shift', 'noise'):
            if not float(getattr(self, name)) >= 0:
                raise ValueError(f'CaptureJitter: {name} must be >= 0, got {getattr(self, name)}')
        if self.gain >= 1:
            raise ValueError(f'CaptureJitter: gain must be < 1 (a channel gain stays positive), got {self.gain}')
        if self.shift > 2:
            raise ValueError(f'CaptureJitter: shift must be <= 2 camera pixels, got {self.shift}')
        if self.noise > 0.1:
            raise ValueError(f'CaptureJitter: noise must be <= 0.1, got {self.noise}')

    def draw(self, counter, jit, key, B, J, clean0):
        """spaa_jitter_draw of these ranges: fills jit [B][J][8] / key [B][J] for iteration counter[0] and advances the counter."""
        _lib.call('spaa_jitter_draw', int(self.seed) & 0xffffffff, _lib.ptr(counter), float(self.gain), float(self.offset),
                  float(self.shift), float(self.noise), int(bool(clean0)), _lib.ptr(jit), _lib.ptr(key), B, J)


def _jitter_supported(jitter, pcnet, classifier, storage, focus, who):
    """What a jitter attack does not serve, said before anything is allocated or launched.  `pcnet` / `classifier`: as spaa() holds
    them after its own checks."""
    if not isinstance(jitter, CaptureJitter):
        raise TypeError(f'{who}: jitter must be a spaa_amd.CaptureJitter, got {type(jitter).__name__}')
    if isinstance(pcnet, list):
        raise NotImplementedError(f'{who}: capture jitter against several views is not implemented; attack one view with jitter')
    if isinstance(classifier, list):
        raise NotImplementedError(f'{who}: capture jitter against an ensemble of classifiers is not implemented; attack one '
                                  'classifier with jitter')
    if not isinstance(classifier, Classifier):
        raise TypeError(f'{who}: a jitter attack needs a spaa_amd.Classifier, got {type(classifier).__name__} (a foreign callable can '
                        'only be attacked without jitter)')
    if storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented with jitter (the draws' unit vectors need a loss "
                                  "scale of their own); use storage='f32'")
    if focus:
        raise ValueError(f'{who}: focus=True has no meaning with jitter (a sample must fool every draw of every iteration)')


def _attention_checked(attention, storage, who):
    """An attack state's own check of its `attention` (the entry points say more, earlier: _attention_supported)."""
    if attention is None:
        return
    if not isinstance(attention, Attention):
        raise TypeError(f'{who}: attention must be a spaa_amd.Attention or None, got {type(attention).__name__}')
    if storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented with attention (the feature map and its gradient are "
                                  "read as fp32); use storage='f32'")


def _attention_supported(attention, classifier, storage, jitter, who):
    """What an attention-weighted attack does not serve, said before anything is allocated or launched.  `classifier`: as spaa() holds
    it after its own checks (a Classifier, a checked list of several, or anything else).  A body without a feature map passes only
    with attention.rollout, where it has an attention rollout to offer instead."""
    if not isinstance(attention, Attention):
        raise TypeError(f'{who}: attention must be a spaa_amd.Attention or None, got {type(attention).__name__}')
    if jitter is not None:
        raise NotImplementedError(f'{who}: attention together with capture jitter is not implemented (every draw would need a map of '
                                  'its own, pulled back through the jitter); use attention or jitter')
    if not isinstance(classifier, (Classifier, list)):
        raise TypeError(f'{who}: an attention-weighted attack needs a spaa_amd.Classifier, got {type(classifier).__name__} (a foreign '
                        'callable has no feature map to read)')
    for c in classifier if isinstance(classifier, list) else [classifier]:
        if isinstance(c, Classifier) and not c.has_feature_map and not (attention.rollout and c.has_rollout):
            raise NotImplementedError(f'{who}: attention is not implemented for {c.name} (Grad-CAM needs a convolutional feature map, which '
                                      'this body does not have); attack it without attention=')
    _attention_checked(attention, storage, who)


TRANSFER_RMAX = 7   # SPAA_TRANSFER_RMAX of include/spaa_hip.h


@dataclasses.dataclass(frozen=True)
class Transfer:
    """The transferable adversarial step: what a sample on the adversarial step follows is not the raw gradient image
    at the projector but m <- `momentum` m + t / |t|_1 (MI-FGSM), t the gradient image convolved with a Gaussian of `sigma` projector
    pixels (TI-FGSM; radius ceil(3 sigma) <= TRANSFER_RMAX, zero beyond the border).  momentum = 0: no accumulation; sigma = 0: no
    smoothing; both 0 is the plain attack and refused."""
    momentum: float = 1.0
    sigma: float = 0.0

    def __post_init__(self):
        for name in ('momentum', 'sigma'):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f'Transfer: {name} must be a finite number, got {v!r}')
        if not 0 <= self.momentum <= 1:
            raise ValueError(f'Transfer: momentum must be in [0, 1], got {self.momentum}')
        if self.sigma < 0:
            raise ValueError(f'Transfer: sigma must be >= 0, got {self.sigma}')
        if self.radius > TRANSFER_RMAX:
            raise ValueError(f'Transfer: sigma = {self.sigma} needs the radius ceil(3 sigma) = {self.radius}, at most {TRANSFER_RMAX} '
                             f'(sigma <= {TRANSFER_RMAX}/3)')
        if self.momentum == 0 and self.sigma == 0:
            raise ValueError('Transfer(0, 0): no momentum and no smoothing is the plain attack (pass transfer=None)')

    @property
    def radius(self):
        """r = ceil(3 sigma): the filter has 2 r + 1 taps per axis."""
        return int(math.ceil(3 * self.sigma))

    def weights(self):
        """The 2 r + 1 taps exp(-i^2 / (2 sigma^2)), i = -r .. r, normalised to sum 1 in float64 and then rounded: a float32 tensor
        ([1.0] for sigma = 0)."""
        r = self.radius
        if r == 0:
            return torch.ones(1, dtype=torch.float32)
        i = torch.arange(-r, r + 1, dtype=torch.float64)
        w = torch.exp(-i * i / (2.0 * float(self.sigma) ** 2))
        return (w / w.sum()).to(torch.float32)


def _transfer_checked(transfer, storage, who):
    """An attack state's own check of its `transfer` (the entry points say more, earlier: _transfer_supported)."""
    if transfer is None:
        return
    if not isinstance(transfer, Transfer):
        raise TypeError(f'{who}: transfer must be a spaa_amd.Transfer or None, got {type(transfer).__name__}')
    if storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented with transfer (the momentum image and the smoothed "
                                  "gradient are fp32 and carry no loss scale); use storage='f32'")


def _transfer_supported(transfer, classifier, storage, who):
    """What a transferable attack does not serve, said before anything is allocated or launched.  `classifier`: as spaa() holds it
    after its own checks (a Classifier, a checked list of several, or anything else)."""
    if not isinstance(transfer, Transfer):
        raise TypeError(f'{who}: transfer must be a spaa_amd.Transfer or None, got {type(transfer).__name__}')
    if not isinstance(classifier, (Classifier, list)):
        raise TypeError(f'{who}: a transferable attack needs a spaa_amd.Classifier, got {type(classifier).__name__} (the route of a '
                        'foreign callable steps inside torch.autograd, where the fused direction kernels do not run)')
    _transfer_checked(transfer, storage, who)


class JitterAttackState(EnsembleAttackState):
    """One batched attack against J = jitter.draws randomly perturbed captures of the camera image per iteration (DESIGN.md,
    "Capture-robust attack"): EnsembleAttackState whose members are J leased engines of ONE classifier, member j looking at draw j
    of y = PCNet(x, s).  Draw 0 is the clean capture (the identity row), so a sample counts as successful only when the clean capture
    and every jittered draw of that iteration are fooled; the stealth loss and `cam_best` stay the clean inference.  The draws'
    parameters come from spaa_jitter_draw (a device-side counter: a replayed graph advances the sequence), the transform from
    spaa_jitter_fwd, and the members' gradient images are pulled back to y by spaa_jitter_bwd before they are combined.  `state`,
    `stats`, `ens_state`, `ens_stats` keep the ensemble's meaning with draws as members."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, jitter, storage='f32', transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        _jitter_supported(jitter, pcnet, classifier, storage, False, 'JitterAttackState')
        self.jitter, self.focus = jitter, False
        self.members = [classifier] * int(jitter.draws)   # (EnsembleAttackState._build leases one engine per entry)
        AttackState.__init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                             transfer=transfer)

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)
        B, J = self.B, self.K
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the iteration number the next draw reads
        self.jit = torch.zeros(B, J, 8, device=dev)
        self.key = torch.zeros(B, J, dtype=torch.int32, device=dev)         # (uint32 bit patterns)
        self.draw_ims = [torch.zeros_like(self.g_adv) for _ in range(J)]
        self.draw_gates = [torch.zeros(B, self.HWc, dtype=torch.uint8, device=dev) for _ in range(J)]
        self.draw_grads = [torch.zeros_like(self.g_adv) for _ in range(J)]

    def _member_logits(self, y):
        jt, p = self.jitter, _lib.ptr
        jt.draw(self.counter, self.jit, self.key, self.B, self.K, clean0=True)
        _lib.call('spaa_jitter_fwd', p(y), p(self.jit), p(self.key), self.K, int(bool(jt.quantize)), _lib.ptr_array(self.draw_ims),
                  _lib.ptr_array(self.draw_gates), self.B, self.eng.Hc, self.eng.Wc)
        return [e.forward(im) for e, im in zip(self.clfs, self.draw_ims)]            # :266, once per draw

    def _member_gradients(self):
        gs = super()._member_gradients()
        _lib.call('spaa_jitter_bwd', _lib.ptr_array(gs), _lib.ptr(self.jit), _lib.ptr_array(self.draw_gates), self.K,
                  _lib.ptr_array(self.draw_grads), self.B, self.eng.Hc, self.eng.Wc)
        return self.draw_grads


POSE_MAX_ROTATE, POSE_MAX_ZOOM, POSE_MAX_TILT, POSE_MAX_SHIFT = 10.0, 0.15, 0.1, 32.0


@dataclasses.dataclass(frozen=True)
class PoseJitter:
    """A small change of camera pose after the setup was captured (the camera bumped, re-mounted, zoomed a little), as ranges of a
    random homography of the camera image: an in-plane rotation of +- `rotate` degrees, a scale of 1 +- `zoom`, a
    translation of +- `shift` camera pixels per axis and a tilt of +- `tilt` per axis, the relative change of the projective
    denominator from the image centre to the edge of the longer side.  What leaves the frame is not seen and what enters it is black.
    `draws`: warped copies attacked at once per iteration (2..4; the first one is the unwarped capture), `seed`: of the counter-based
    generator.  The defaults are a guess at "the camera was bumped", not a measurement.  `rotate` <= 10, `zoom` <= 0.15 and `tilt`
    <= 0.1 are what bounds the window of the adjoint kernel (spaa_pose_bwd); `shift` <= 32."""
    rotate: float = 2.0
    zoom: float = 0.03
    shift: float = 3.0
    tilt: float = 0.02
    draws: int = 3
    seed: int = 0

    def __post_init__(self):
        if not 2 <= int(self.draws) <= JITTER_MAX:
            raise ValueError(f'PoseJitter: draws must be 2..{JITTER_MAX}, got {self.draws}')
        for name, most in (('rotate', POSE_MAX_ROTATE), ('zoom', POSE_MAX_ZOOM), ('shift', POSE_MAX_SHIFT), ('tilt', POSE_MAX_TILT)):
            v = float(getattr(self, name))
            if not v >= 0:
                raise ValueError(f'PoseJitter: {name} must be >= 0, got {getattr(self, name)}')
            if v > most:
                raise ValueError(f'PoseJitter: {name} must be <= {most:g}, got {getattr(self, name)}')

    def draw(self, counter, table, B, J, H, W, clean0):
        """spaa_pose_draw of these ranges: fills table [B][J][8] for iteration counter[0] of an H x W image and advances the counter."""
        _lib.call('spaa_pose_draw', int(self.seed) & 0xffffffff, _lib.ptr(counter), float(self.rotate), float(self.zoom),
                  float(self.shift), float(self.tilt), int(bool(clean0)), _lib.ptr(table), B, J, H, W)


def _pose_supported(pose, pcnet, classifier, storage, focus, attention, jitter, who):
    """What a pose attack does not serve, said before anything is allocated or launched.  `pcnet` / `classifier`: as spaa() holds
    them after its own checks; `jitter`: None or a checked CaptureJitter."""
    if not isinstance(pose, PoseJitter):
        raise TypeError(f'{who}: pose must be a spaa_amd.PoseJitter, got {type(pose).__name__}')
    if isinstance(pcnet, list):
        raise NotImplementedError(f'{who}: pose jitter against several views is not implemented; attack one view with pose')
    if isinstance(classifier, list):
        raise NotImplementedError(f'{who}: pose jitter against an ensemble of classifiers is not implemented; attack one classifier '
                                  'with pose')
    if not isinstance(classifier, Classifier):
        raise TypeError(f'{who}: a pose attack needs a spaa_amd.Classifier, got {type(classifier).__name__} (a foreign callable can '
                        'only be attacked without pose)')
    if attention is not None:
        raise NotImplementedError(f'{who}: attention together with pose jitter is not implemented (every draw would need a map of its '
                                  'own, pulled back through the warp); use attention or pose')
    if storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented with pose (the draws' unit vectors need a loss scale "
                                  "of their own); use storage='f32'")
    if focus:
        raise ValueError(f'{who}: focus=True has no meaning with pose (a sample must fool every draw of every iteration)')
    if jitter is not None and int(jitter.draws) != int(pose.draws):
        raise ValueError(f'{who}: pose and jitter are applied draw by draw and must name the same draws, got pose.draws = '
                         f'{pose.draws} and jitter.draws = {jitter.draws}')


class PoseAttackState(EnsembleAttackState):
    """One batched attack against J = pose.draws randomly warped copies of the camera image per iteration:
    EnsembleAttackState whose members are J leased engines of ONE classifier, member j looking at draw j of y = PCNet(x, s), as in
    JitterAttackState.  Draw 0 is the unwarped capture (the identity row), so a sample counts as successful only when the unwarped
    capture and every warped draw of that iteration are fooled; the stealth loss and `cam_best` stay the clean inference.  The
    homographies come from spaa_pose_draw (a device-side counter: a replayed graph advances the sequence), the warp from
    spaa_pose_fwd, and the members' gradient images are pulled back to y by spaa_pose_bwd before they are combined.  With `jitter`
    (a CaptureJitter of the same `draws`) draw j is Jitter_j(Pose_j(y)): spaa_jitter_fwd_each behind the warp, spaa_jitter_bwd before
    its adjoint.  `state`, `stats`, `ens_state`, `ens_stats` keep the ensemble's meaning with draws as members."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, pose, storage='f32', jitter=None,
                 transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        if jitter is not None:
            _jitter_supported(jitter, pcnet, classifier, storage, False, 'PoseAttackState')
        _pose_supported(pose, pcnet, classifier, storage, False, None, jitter, 'PoseAttackState')
        self.pose, self.jitter, self.focus = pose, jitter, False
        self.members = [classifier] * int(pose.draws)   # (EnsembleAttackState._build leases one engine per entry)
        AttackState.__init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                             transfer=transfer)

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)
        B, J = self.B, self.K
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the iteration number the next draw reads
        self.table = torch.zeros(B, J, 8, device=dev)
        self.pose_ims = [torch.zeros_like(self.g_adv) for _ in range(J)]
        self.pose_grads = [torch.zeros_like(self.g_adv) for _ in range(J)]
        if self.jitter is not None:
            self.jitter_counter = torch.zeros(1, dtype=torch.int32, device=dev)
            self.jit = torch.zeros(B, J, 8, device=dev)
            self.key = torch.zeros(B, J, dtype=torch.int32, device=dev)     # (uint32 bit patterns)
            self.draw_ims = [torch.zeros_like(self.g_adv) for _ in range(J)]
            self.draw_gates = [torch.zeros(B, self.HWc, dtype=torch.uint8, device=dev) for _ in range(J)]
            self.draw_grads = [torch.zeros_like(self.g_adv) for _ in range(J)]

    def _member_logits(self, y):
        jt, p, arr = self.jitter, _lib.ptr, _lib.ptr_array
        Hc, Wc = self.eng.Hc, self.eng.Wc
        self.pose.draw(self.counter, self.table, self.B, self.K, Hc, Wc, clean0=True)
        _lib.call('spaa_pose_fwd', p(y), p(self.table), self.K, arr(self.pose_ims), self.B, Hc, Wc)
        ims = self.pose_ims
        if jt is not None:
            jt.draw(self.jitter_counter, self.jit, self.key, self.B, self.K, clean0=True)
            _lib.call('spaa_jitter_fwd_each', arr(ims), p(self.jit), p(self.key), self.K, int(bool(jt.quantize)), arr(self.draw_ims),
                      arr(self.draw_gates), self.B, Hc, Wc)
            ims = self.draw_ims
        return [e.forward(im) for e, im in zip(self.clfs, ims)]                      # :266, once per draw

    def _member_gradients(self):
        p, arr = _lib.ptr, _lib.ptr_array
        gs = super()._member_gradients()
        if self.jitter is not None:
            _lib.call('spaa_jitter_bwd', arr(gs), p(self.jit), arr(self.draw_gates), self.K, arr(self.draw_grads), self.B, self.eng.Hc,
                      self.eng.Wc)
            gs = self.draw_grads
        _lib.call('spaa_pose_bwd', arr(gs), p(self.table), self.K, arr(self.pose_grads), self.B, self.eng.Hc, self.eng.Wc)
        return self.pose_grads


def _attack_state(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage, focus, jitter=None,
                  attention=None, transfer=None, pose=None):
    """AttackState for one Classifier, EnsembleAttackState for a checked list of several, MultiViewAttackState for a checked list of
    PCNets (with their list of scenes), JitterAttackState for one Classifier with a CaptureJitter (which takes no `attention`),
    PoseAttackState for one Classifier with a PoseJitter (with or without a CaptureJitter; no `attention`).  Each of them takes
    `transfer`."""
    if pose is not None:
        return PoseAttackState(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, pose, storage=storage,
                               jitter=jitter, transfer=transfer)
    if jitter is not None:
        return JitterAttackState(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, jitter, storage=storage,
                                 transfer=transfer)
    if isinstance(pcnet, list):
        return MultiViewAttackState(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                                    focus=focus, attention=attention, transfer=transfer)
    if isinstance(classifier, list):
        return EnsembleAttackState(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                                   focus=focus, attention=attention, transfer=transfer)
    return AttackState(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage, attention=attention,
                       transfer=transfer)


def spaa(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr, stealth_loss, device, setup_info,
         *, iters=50, adv_lr=2, col_lr=1, p_thresh=0.9, trace=None, verbose=False, storage='f32', focus=False, jitter=None,
         attention=None, transfer=None, pose=None):
    """Stealthy Projector-based Adversarial Attack (SPAA Algorithm 1) — see module docstring.

    :param pcnet: spaa_amd.PCNet (optionally wrapped in DataParallel-like `.module`), or a list / tuple of 2..4 of them: the same projector
        and scene seen from as many camera poses, ONE projection against all of these views (MultiViewAttackState; one Classifier,
        fp32 storage, one camera size).  `cam_scene` is then a list of one scene per view and the first return value a list of one
        camera image batch per view.  A sequence of one is that PCNet.
    :param classifier: spaa_amd.Classifier, or a list / tuple of 2..4 of them with the same classes: ONE projection against all of them
        (EnsembleAttackState; fp32 storage only).  A sequence of one is that classifier.
    :param focus: ensembles and views only: members / views that are already fooled rest until all are (default: every one pulls all
        the time)
    :param jitter: a CaptureJitter: ONE projection against `jitter.draws` randomly perturbed captures of the camera image per iteration,
        the first of them the clean one (JitterAttackState; one PCNet, one Classifier, fp32 storage, no `focus`).  The trace entries
        are the ensemble's, with draws as members.  None (default): the attack on the noiseless inferred capture
    :param attention: an Attention: the classifier's gradient image is weighted by floor + (1 - floor) M, M the Grad-CAM map of the
        sample's class on the classifier crop (fp32 storage, a spaa_amd.Classifier, no `jitter`).  In an ensemble every
        member uses its own map, with several views every view its own.  vit_b_16 has no such map and is refused, unless
        `attention.rollout` is set: then its M is the attention rollout of its class token, written in the backward
        pass itself, and convolutional members keep Grad-CAM.  None (default): the plain attack, launch for launch
    :param transfer: a Transfer: the adversarial step follows the Gaussian-smoothed, momentum-accumulated gradient image at the projector
        instead of the raw one (fp32 storage, a spaa_amd.Classifier).  Combines with ensembles, views, `focus`, `jitter`
        and `attention`: it acts on the projector-side gradient after them.  None (default): the plain attack, launch for launch
    :param pose: a PoseJitter: ONE projection against `pose.draws` randomly warped copies of the camera image per iteration (a small
        random change of camera pose: rotation, zoom, translation, tilt), the first of them the unwarped one (PoseAttackState, DESIGN.md
        7k; one PCNet, one Classifier, fp32 storage, no `focus`, no `attention`).  With `jitter` of the same `draws`, draw j is
        Jitter_j(Pose_j(y)).  The trace entries are the ensemble's, with draws as members.  None (default): launch for launch as before
    :param imagenet_labels: dict idx -> name (only used when verbose)
    :param target_idx: list of B class ids (true label if untargeted)
    :param targeted: bool
    :param cam_scene: [3,H,W] / [1,3,H,W] / [B,3,H,W] in [0,1]
    :param d_thr: SPAA Algorithm 1's threshold on the mean per-pixel L2 perturbation (x255)
    :param stealth_loss: string containing any of 'prjl2', 'caml2', 'camdE'
    :param setup_info: {'classifier_crop_sz', 'prj_brightness', 'prj_im_sz'}
    :param trace: optional list; receives per-iteration (state, stats) device tensors (no sync inside the loop); for an ensemble
        (state, stats, ens_state, ens_stats), where state[:, 3] counts the fooled members and ens_state holds each member's top-1;
        for several views (state, stats, view_state, view_stats) in the same way
    :return: (cam_infer_best [B,3,Hc,Wc], prj_adv_best [B,3,Hp,Wp] in [0,1]); for several views ([cam_infer_best per view], prj_adv_best)
    """
    pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
    if isinstance(pcnet, (list, tuple)):
        pcnet, cam_scene = _view_pcnets(pcnet, cam_scene, 'spaa')
    if not isinstance(pcnet, (PCNet, list)):
        raise TypeError('spaa_amd.spaa needs a spaa_amd.PCNet (the HIP path has no generic PCNet fallback)')
    if isinstance(classifier, (list, tuple)):
        classifier = _ensemble_members(classifier, storage, 'spaa')
        if len(classifier) == 1:
            classifier = classifier[0]
    if isinstance(pcnet, list):
        _views_supported(pcnet, classifier, storage, 'spaa')
    if jitter is not None:
        _jitter_supported(jitter, pcnet, classifier, storage, focus, 'spaa')
    if pose is not None:
        _pose_supported(pose, pcnet, classifier, storage, focus, attention, jitter, 'spaa')
    if attention is not None:
        _attention_supported(attention, classifier, storage, jitter, 'spaa')
    if transfer is not None:
        _transfer_supported(transfer, classifier, storage, 'spaa')
    if not isinstance(classifier, (Classifier, list)):
        if not callable(classifier):
            raise TypeError('classifier must be a spaa_amd.Classifier or a callable (im, crop_sz) -> (raw_score, p, idx)')
        return _spaa_foreign_classifier(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr,
                                        stealth_loss, device, setup_info, iters, adv_lr, col_lr, p_thresh, trace)
    st = _attack_state(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage, focus, jitter, attention,
                       transfer, pose)

    def report(i):
        if i % 30 == 0 or i == iters - 1:
            s, f = st.state.cpu(), st.stats.cpu()
            v = 7 if (targeted and st.B > 7) else 0
            if isinstance(st, MultiViewAttackState):   # (p = the least confident view's; y = how many views are fooled)
                name = f'of {st.V} views fooled'
            elif isinstance(st, EnsembleAttackState):   # (p = the least confident member's / draw's; y = how many are fooled)
                draws = isinstance(st, (JitterAttackState, PoseAttackState))
                name = f'of {st.K} draws fooled' if draws else f'of {st.K} members fooled'
            else:
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
            trace.append(st.trace_entry())
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
               p_thresh=0.9, max_batch=64, storage='f32', trace=None, focus=False, jitter=None, attention=None, transfer=None,
               pose=None):
    """Several SPAA attacks on one PCNet, scene and classifier as few batched attacks (the reference's driver makes one spaa() call
    per configuration: projector_based_attack.py:24-148).  `configs`: [(stealth_loss, d_thr, targeted, target_idx), ...]; returns one
    (cam_infer_best, prj_adv_best) per config, in order -- what spaa(pcnet, classifier, imagenet_labels, target_idx, targeted,
    cam_scene, d_thr, stealth_loss, device, setup_info) returns for it: samples do not interact, so only the batch differs.  The
    samples of all configs are flattened in order and cut into chunks of at most `max_batch` (one AttackState each, the loop of
    spaa() with its loss weights, targeted flag and d_thr per sample); `trace` receives one list per chunk, of the per-iteration
    (state, stats) pairs spaa() records (the chunk's samples in flattened order).  `classifier` may be a list / tuple of 2..4
    Classifiers, as in spaa(): every sample then attacks all of them at once (`focus` as there), and the trace entries are
    (state, stats, ens_state, ens_stats).  `pcnet` may be a list / tuple of 2..4 PCNets with `cam_scene` a list of their scenes, as
    in spaa(): every sample then attacks all views at once, each config's first return value is a list of one camera image batch
    per view, and the trace entries are (state, stats, view_state, view_stats).  `jitter`: a CaptureJitter, as in spaa(): every chunk
    is a jitter attack with that seed (the draws of a sample depend on its place in its chunk), the trace entries the ensemble's.
    `attention`: an Attention, as in spaa(): every chunk is an attention-weighted attack.  `transfer`: a Transfer, as in spaa(): every
    chunk's adversarial steps follow the smoothed, momentum-accumulated direction (each chunk's momentum starts at zero).  `pose`: a
    PoseJitter, as in spaa(): every chunk is a pose attack with that seed (the draws of a sample depend on its place in its chunk)."""
    samples, chunks = plan_sweep(configs, max_batch)
    pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
    if isinstance(pcnet, (list, tuple)):
        pcnet, cam_scene = _view_pcnets(pcnet, cam_scene, 'spaa_sweep')
    if not isinstance(pcnet, (PCNet, list)):
        raise TypeError('spaa_sweep needs a spaa_amd.PCNet (the HIP path has no generic PCNet fallback)')
    if isinstance(classifier, (list, tuple)):
        classifier = _ensemble_members(classifier, storage, 'spaa_sweep')
        if len(classifier) == 1:
            classifier = classifier[0]
    if isinstance(pcnet, list):
        _views_supported(pcnet, classifier, storage, 'spaa_sweep')
    if jitter is not None:
        _jitter_supported(jitter, pcnet, classifier, storage, focus, 'spaa_sweep')
    if pose is not None:
        _pose_supported(pose, pcnet, classifier, storage, focus, attention, jitter, 'spaa_sweep')
    if attention is not None:
        _attention_supported(attention, classifier, storage, jitter, 'spaa_sweep')
    if transfer is not None:
        _transfer_supported(transfer, classifier, storage, 'spaa_sweep')
    if not isinstance(classifier, (Classifier, list)):
        raise TypeError('spaa_sweep needs a spaa_amd.Classifier')
    _require_gpu(device, 'spaa_sweep')

    def one_scene(m, scene):
        sc = _scene_batch(scene, 1)
        cam_sz = tuple(m.warping_net.out_size)
        if sc.ndim != 4 or sc.shape[0] != 1 or tuple(sc.shape[1:]) != (3,) + cam_sz:
            raise ValueError(f'cam_scene must be [3,H,W] or [1,3,H,W] with (H, W) = {cam_sz} (PCNet\'s output); got {tuple(scene.shape)}')
        return sc

    sc = [one_scene(m, s) for m, s in zip(pcnet, cam_scene)] if isinstance(pcnet, list) else one_scene(pcnet, cam_scene)
    results = []
    for a, b in chunks:
        part = samples[a:b]
        st = _attack_state(pcnet, classifier, [t for *_, t in part], sc, [s[1] for s in part], setup_info, device, storage, focus,
                           jitter, attention, transfer, pose)
        tr = [] if trace is not None else None
        _run(st, [s[3] for s in part], [s[2] for s in part], iters, adv_lr, col_lr, p_thresh, tr)
        if trace is not None:
            trace.append(tr)
        results.append(st.results())
        del st
    if isinstance(pcnet, list):   # (a chunk's result holds one camera image per view: split view by view)
        per_view = [split_sweep(samples, len(configs), [(cams[v], prj) for cams, prj in results]) for v in range(len(pcnet))]
        return [([pv[i][0] for pv in per_view], per_view[0][i][1]) for i in range(len(configs))]
    return split_sweep(samples, len(configs), results)


class _StealthFn(torch.autograd.Function):
    """Per-sample camera-side stealth loss caml2_w * caml2 + camdE_w * camdE (projector_based_attack.py:279-284) through
    the fused HIP kernel; the kernel's analytic gradient is kept for backward."""

    @staticmethod
    def forward(ctx, cam_infer, scene4, scene_lab, caml2_w, camdE_w):
        y4 = to_nhwc4(cam_infer)
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
    dev = _require_gpu(device, 'spaa')
    B = len(target_idx)
    with _lib.on_device(dev):
        cp_sz = tuple(setup_info['classifier_crop_sz'])
        gray = float(setup_info['prj_brightness'])
        scene = _scene_batch(cam_scene, B).to(dev).contiguous()
        scene4 = to_nhwc4(scene)
        scene_lab = torch.zeros_like(scene4)
        _lib.call('spaa_rgb2lab', _lib.ptr(scene4), _lib.ptr(scene_lab), scene4.numel() // 4)
        im_gray = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), gray, device=dev)
        prj_adv = im_gray.clone().requires_grad_(True)
        prjl2_w, caml2_w, camdE_w = loss_weights(stealth_loss)
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


# The experiment driver and the summary step live in their own modules; their public names stay importable from here (the same
# objects).  Neither module imports this one at import time: they reach the attack through it when they are called.
from .attack_driver import (ATTACKERS, MODEL_TRAIN_CFG, AttackSetup, get_attacker_cfg, to_attacker_cfg_str,   # noqa: E402,F401
                            run_projector_based_attack, _run_one_pixel_de, project_capture_real_attack)
from .attack_summary import (SUMMARY_STEALTH_LOSSES, SUMMARY_D_THRESHES, SUMMARY_CLASSIFIERS, SUMMARY_CHUNK,   # noqa: E402,F401
                             SUMMARY_COLUMNS, MONTAGE_CHUNK, attack_success, write_stats, _sorted_classes, _nonempty,
                             attack_results, attack_transfer, capture_survival, pose_survival, transfer_success,
                             summarize_single_attacker, summarize_all_attackers)
