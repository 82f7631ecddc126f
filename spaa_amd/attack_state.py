"""The device-side states of the batched SPAA attack: AttackState (one PCNet, one classifier), EnsembleAttackState (several classifiers),
MultiViewAttackState (several PCNets), UniversalAttackState (groups of samples that share their projector image) and DrawAttackState (random draws of the camera image through a chain of stages:
JitterAttackState, PoseAttackState, JpegAttackState, BlurAttackState).  Lines quoted as :NNN are the reference's projector_based_attack.py."""
import ctypes

import torch

from . import _lib
from .models import to_nhwc4, to_nchw
from .attack_options import (JPEG_SUBSAMPLINGS, _unwrap, _ensemble_members, _view_pcnets, _views_supported, _jitter_supported,
                             _pose_supported, _jpeg_supported, _blur_supported, _attention_checked, _transfer_checked, _universal_supported)


def _is_scalar(v):
    return isinstance(v, (bool, int, float)) or (isinstance(v, torch.Tensor) and v.ndim == 0) or getattr(v, 'ndim', None) == 0


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
    label = None   # what spaa()'s report counts in state[:, 3]: 'members', 'draws', 'views'; None: the plain attack prints the class

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

    def _lease_view(self, pcnet, classifier, cam_scene, setup_info, whose=''):
        """One camera view: a leased PCNet engine holding the view's scene batch and a leased classifier engine looking at its output;
        returns (PCNet engine, classifier engine, scene [B,Hc,Wc,4], its Lab image).  Further views have the first one's camera size."""
        B = self.B
        sc = _scene_batch(cam_scene, B)
        if sc.shape[0] != B:
            raise ValueError(f'{whose}cam_scene must hold 1 or len(target_idx) scenes')
        eng = pcnet.engine(B, tuple(setup_info['prj_im_sz']), owner=self, storage=self.storage)
        Hc, Wc = eng.Hc, eng.Wc
        first = getattr(self, 'eng', eng)
        if (first.Hc, first.Wc) != (Hc, Wc):
            raise ValueError(f'the views must have the same camera size, got {(first.Hc, first.Wc)} and {(Hc, Wc)}')
        if tuple(sc.shape[-2:]) != (Hc, Wc):
            raise ValueError(f'cam_scene is {tuple(sc.shape[-2:])} but PCNet outputs {(Hc, Wc)}')
        clf = classifier.engine(B, (Hc, Wc), self.cp_sz, owner=self, storage=self.storage)
        if self.attention is not None:
            clf.attention_buffers(self.attention.rollout)
        scene4 = to_nhwc4(sc.contiguous().to(self.dev))
        eng.set_scene(scene4)
        scene_lab = torch.zeros_like(scene4)
        _lib.call('spaa_rgb2lab', _lib.ptr(scene4), _lib.ptr(scene_lab), B * Hc * Wc)
        if self.any_ssim:   # the window statistics of the scene alone: once per attack and view
            mu2, e22 = torch.zeros_like(scene4), torch.zeros_like(scene4)
            _lib.call('spaa_ssim_scene_stats', _lib.ptr(scene4), self._ssim_taps, _lib.ptr(mu2), _lib.ptr(e22), B, Hc, Wc)
            self.ssim_scene_stats.append((mu2, e22))
        return eng, clf, scene4, scene_lab

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        from .projector_based_attack import CLAMP_BITS, loss_weights, ssim_weight   # (the switches live with the entry points)
        B = len(target_idx)
        if B < 1:
            raise ValueError('target_idx is empty: nothing to attack')
        self.B, self.dev = B, dev
        prj_sz = tuple(setup_info['prj_im_sz'])
        self.cp_sz = tuple(setup_info['classifier_crop_sz'])
        self.gray = float(setup_info['prj_brightness'])
        # `stealth_loss`: one string for the batch, or one per sample (spaa_sweep)
        losses = [stealth_loss] * B if isinstance(stealth_loss, str) else list(stealth_loss)
        # the SSIM term has its own launches with a weight per sample; without it in any string nothing of it exists
        ssim_w = [ssim_weight(s) for s in losses]
        self.any_ssim, self.ssim, self.ssims = any(ssim_w), None, None
        if self.any_ssim:
            from .metrics import ssim_taps
            self._ssim_taps = (ctypes.c_float * 11)(*ssim_taps().tolist())
            self.ssim_scene_stats = []   # (mu2, e22) per view, in the order of the views
        self.eng, self.clf, self.scene4, self.scene_lab = self._lease_view(pcnet, classifier, cam_scene, setup_info)
        self.clfs = [self.clf]   # (one engine per member / view where there are several)
        Hc, Wc = self.eng.Hc, self.eng.Wc
        if self.any_ssim:
            # the three maps of dS/d(window statistics) are shared by the views (forward and adjoint run back to back), the tile sums
            # of S and the per-sample SSIM of the last iteration are per view: `ssims[v]`, `ssim` = `ssims[0]`
            self.ssim_w = torch.tensor(ssim_w, dtype=torch.float32, device=dev)
            self.ssim_maps = [torch.zeros(B, Hc, Wc, 4, device=dev) for _ in range(3)]
            self.ssim_tiles = _lib.load().spaa_ssim_tiles(Hc, Wc)
            self.ssim_partials = [torch.zeros(B, self.ssim_tiles, device=dev)]
            self.ssims = [torch.zeros(B, device=dev)]
            self.ssim = self.ssims[0]
        # fp16 gradients need a loss scale (fp16's smallest normal is 6e-5; the per-pixel loss gradients are ~1/(B*H*W)).
        # Each sample's gradient is normalised before the step (:307, :315), so a positive per-branch scale changes
        # nothing but the fp16 rounding: stealth branch: 1/16 per pixel instead of 1/(B*H*W); adversarial branch: +-16
        # at the target logit instead of 1/B.
        self.gs_col, self.gs_adv = ((B * Hc * Wc) / 16.0, 16.0 * B) if self.storage == 'f16' else (1.0, 1.0)
        Hp, Wp = prj_sz
        self.HWp, self.HWc = Hp * Wp, Hc * Wc
        self.x = torch.zeros(B, Hp, Wp, 4, device=dev)
        self.x[..., :3] = self.gray
        self.x_best, self.cam_best = self.x.clone(), self.scene4.clone()
        self.state = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(B, 8, device=dev)
        self.stats[:, 5] = 1e6
        self.nblk_c, self.nblk_p = (self.HWc + 255) // 256, (self.HWp + 255) // 256
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
        # self.prjl2_w / caml2_w / camdE_w are the batch's weights when every sample has the same ones, else None: the per-sample table
        # of the _ps launches carries them.
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

    def _prjl2_fwd(self):
        """prjl2 of the per-sample table route, where any sample weights it; returns the pointer the decision takes (or None)."""
        if self.any_prjl2:
            _lib.call('spaa_prjl2_fwd', _lib.ptr(self.x), self.gray, _lib.ptr(self.prjl2), self.B, self.HWp)
        return _lib.ptr(self.prjl2) if self.any_prjl2 else None

    def _stealth_loss_ps(self, y, v=None):
        """The stealth loss of camera image y (the state's own view, or view v) and its gradient, weighted by the per-sample table."""
        p = _lib.ptr
        scene4, lab, g_col, partial = ((self.scene4, self.scene_lab, self.g_col, self.partial_loss) if v is None else
                                       (self.scene4s[v], self.scene_labs[v], self.g_cols[v], self.partial_losses[v]))
        _lib.call('spaa_stealth_loss_fwd_bwd_ps', p(y), p(scene4), p(lab), p(self.ps_params), self.gs_col / (self.B * self.HWc),
                  p(g_col), None, p(partial), self.B, self.HWc)

    def _ssim_term(self, y, v=None):
        """The SSIM term of camera image y (the state's own view, or view v), directly behind the stealth-loss launch that has written
        g_col: for every sample with 'camssim' in its string, g_col += gscale d(1 - SSIM_b)/dy with gscale = gs_col / B (the loop's
        batch mean and loss scale; the SSIM mean over 3 Hc Wc is the launch's), and ssims[v] = SSIM_b.  The other samples' rows are
        not touched.  Three launches, no host read; without the term in any string none."""
        if not self.any_ssim:
            return
        p, v = _lib.ptr, v or 0
        scene4, g_col = (self.scene4, self.g_col) if not v else (self.scene4s[v], self.g_cols[v])
        (mu2, e22), (m_mu, m_11, m_12), partial = self.ssim_scene_stats[v], self.ssim_maps, self.ssim_partials[v]
        Hc, Wc = self.eng.Hc, self.eng.Wc
        _lib.call('spaa_ssim_fwd', p(y), p(scene4), p(mu2), p(e22), self._ssim_taps, p(self.ssim_w), p(m_mu), p(m_11), p(m_12),
                  p(partial), self.B, Hc, Wc)
        _lib.call('spaa_ssim_bwd', p(y), p(scene4), p(m_mu), p(m_11), p(m_12), self._ssim_taps, p(self.ssim_w),
                  self.gs_col / (self.B * 3 * self.HWc), p(g_col), self.B, Hc, Wc)
        _lib.call('spaa_ssim_value', p(partial), p(self.ssim_w), self.ssim_tiles, Hc, Wc, p(self.ssims[v]), self.B)

    def _forward_decide(self, targeted, d_thr, p_thresh, adv_w):
        B, p = self.B, _lib.ptr
        uni = self._per_sample(targeted, d_thr)
        y = self.eng.forward(self.x, clamp01=True)                                   # :265
        logits = self.clf.forward(y)                                                 # :266
        self._y, self._uniform = y, uni is not None
        if uni is None:   # several attack configurations in one batch: the same kernels, their parameters per sample
            prjl2 = self._prjl2_fwd()
            self._stealth_loss_ps(y)
            self._ssim_term(y)
            _lib.call('spaa_decide_ps', p(logits), self.clf.ncls, p(self.target), p(self.partial_loss), self.nblk_c, self.HWc,
                      prjl2, p(self.ps_params), p(self.ps_flags), float(p_thresh), adv_w / B * self.gs_adv,
                      p(self.state), p(self.stats), p(self.g_logits), B)
            return
        targeted, d_thr = uni
        if self.prjl2_w:
            _lib.call('spaa_prjl2_fwd', p(self.x), self.gray, p(self.prjl2), B, self.HWp)    # :275
        _lib.call('spaa_stealth_loss_fwd_bwd', p(y), p(self.scene4), p(self.scene_lab), self.caml2_w, self.camdE_w,
                  self.gs_col / (B * self.HWc), p(self.g_col), None, p(self.partial_loss), B, self.HWc)   # :279-287 + bwd
        self._ssim_term(y)
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
        maps = self._engine_maps(self.clfs)
        return maps if self.label else maps[0]

    def trace_entry(self):
        """What spaa()'s `trace` records per iteration (copies; no sync)."""
        return self.state.clone(), self.stats.clone()

    def _pcnet_backward(self, eng, g_adv, g_col, gP, sumsq=None, clamp_bits=None):
        """The PCNet part of the backward pass for one engine (:302 / :310), from each sample's choice between g_adv and g_col: the
        choice and the clamp gate as the first phase of the fused head kernel where the engine has it, else as a launch into gP."""
        if eng.can_select():
            return eng.backward(None, select=(g_adv, g_col, self.state), sumsq=sumsq, clamp_bits=clamp_bits)
        p = _lib.ptr
        _lib.call('spaa_select_grad', p(g_adv), p(g_col), p(self.state), p(eng.a['Ypre']), p(gP), self.B, self.HWc)
        return eng.backward(gP, sumsq=sumsq, clamp_bits=clamp_bits)

    def _step_and_track(self, gx, adv_lr, col_lr):
        """The normalised step along gx (||gx||^2 per sample in partial_ss) and the best-so-far bookkeeping (:307,315,323-328)."""
        p, n = _lib.ptr, self.partial_ss.shape[1]
        self._shape_direction(gx, self.partial_ss, n)
        _lib.call('spaa_step_and_track_n', p(self.x), p(gx), p(self.partial_ss), n, p(self.state), float(adv_lr), float(col_lr),
                  p(self.x_best), p(self._y), p(self.cam_best), self.B, self.HWp, self.HWc, p(self.clamp_bits))
        self._bits_version = self.x._version

    def _backward_step(self, adv_lr, col_lr):
        B, p = self.B, _lib.ptr
        g_adv = self._adv_gradient()
        # (mixed configurations: the prjl2 scale is a [B] device tensor, and the sums of squares take the _ps launches)
        prjl2_scale = self.prjl2_w / (B * self.HWp) * self.gs_col if self._uniform else self.ps_prjl2_scale
        ss = (self.partial_ss, self.gray, prjl2_scale, self.state) if self.ss_tiles else None   # (||g||^2 from the adjoint's epilogue)
        bits = self.clamp_bits if (self.clamp_bits is not None and self._bits_version == self.x._version) else None
        gx = self._pcnet_backward(self.eng, g_adv, self.g_col, self.gP, ss, bits)
        if not self.ss_tiles and self._uniform:
            _lib.call('spaa_grad_sumsq', p(gx), p(self.x), self.gray, prjl2_scale, p(self.state), p(self.partial_ss), B, self.HWp)
        elif not self.ss_tiles:
            _lib.call('spaa_grad_sumsq_ps', p(gx), p(self.x), self.gray, p(prjl2_scale), p(self.state), p(self.partial_ss), B,
                      self.HWp)
        self._step_and_track(gx, adv_lr, col_lr)

    def results(self):
        with torch.cuda.device(self.dev):
            return to_nchw(self.cam_best), to_nchw(self.x_best, clamp01=True)        # :337


class EnsembleAttackState(AttackState):
    """One batched attack against K = 2..ENS_MAX classifiers that see the same camera image ("Ensemble attack"): AttackState
    with one leased engine per member, the decision over all members (spaa_decide_ens) and, as adversarial cotangent, the weighted sum
    of the members' unit gradient images (spaa_ens_sumsq + spaa_ens_combine).  PCNet's passes, the stealth loss, the colour step, the
    normalised step and the best tracking are AttackState's.  `state[:, 3]` counts the fooled members; each member's top-1 is in
    `ens_state`.  `focus`: a member that is already fooled rests (weight 0) until all are."""
    label = 'members'

    def __init__(self, pcnet, classifiers, target_idx, cam_scene, stealth_loss, setup_info, device, storage='f32', focus=False,
                 attention=None, transfer=None):
        self.members, self.focus = self._members(classifiers, storage), bool(focus)   # (one engine is leased per member)
        super().__init__(pcnet, self.members[0], target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                         attention=attention, transfer=transfer)

    def _members(self, classifiers, storage):   # (the checked list of the members' classifiers)
        members = _ensemble_members(classifiers, storage, 'EnsembleAttackState')
        if len(members) < 2:
            raise ValueError('EnsembleAttackState needs at least two classifiers (AttackState attacks one)')
        return members

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)   # (leases member 0's engine: self.clf)
        B, K = self.B, len(self.members)
        self.K = K
        self.clfs = [self.clf] + [c.engine(B, (self.eng.Hc, self.eng.Wc), self.cp_sz, owner=self, storage=self.storage)
                                  for c in self.members[1:]]
        for e in self.clfs[1:] if self.attention is not None else []:
            e.attention_buffers(self.attention.rollout)
        self.ens_g_logits = [self.g_logits] + [torch.zeros_like(self.g_logits) for _ in range(K - 1)]
        self.ens_state = torch.zeros(B, K, 2, dtype=torch.int32, device=dev)
        self.ens_stats = torch.zeros(B, K, 2, device=dev)
        self.ens_w = torch.ones(B, K, device=dev)
        self.ens_partial = torch.zeros(B, K, self.nblk_c, device=dev)
        self.g_adv = torch.zeros(B, self.eng.Hc, self.eng.Wc, 4, device=dev)

    def _forward_decide(self, targeted, d_thr, p_thresh, adv_w):
        p = _lib.ptr
        self._per_sample(targeted, d_thr, table=True)   # (the ensemble decision has the per-sample table form only)
        y = self.eng.forward(self.x, clamp01=True)                                   # :265
        logits = self._member_logits(y)
        self._y, self._uniform = y, False
        prjl2 = self._prjl2_fwd()
        self._stealth_loss_ps(y)
        self._ssim_term(y)
        _lib.call('spaa_decide_ens', _lib.ptr_array(logits), self.K, self.clf.ncls, p(self.target), p(self.partial_loss), self.nblk_c,
                  self.HWc, prjl2, p(self.ps_params), p(self.ps_flags), float(p_thresh), int(self.focus), p(self.state), p(self.stats),
                  p(self.ens_state), p(self.ens_stats), p(self.ens_w),
                  _lib.ptr_array(self.ens_g_logits), self.B)

    def _member_logits(self, y):
        """Every member's logits of the camera image y."""
        return [e.forward(y) for e in self.clfs]                                     # :266, once per member

    def _member_gradients(self):
        """Every member's gradient image at the camera image, from its seed of the decision."""
        return [e.backward(g, self.attention, self.target) for e, g in zip(self.clfs, self.ens_g_logits)]   # (each its own map)

    def _adv_gradient(self):
        gs = _lib.ptr_array(self._member_gradients())
        _lib.call('spaa_ens_sumsq', gs, self.K, _lib.ptr(self.ens_partial), self.B, self.HWc)
        _lib.call('spaa_ens_combine', gs, self.K, _lib.ptr(self.ens_partial), self.nblk_c, _lib.ptr(self.ens_w), _lib.ptr(self.g_adv),
                  self.B, self.HWc)
        return self.g_adv

    def trace_entry(self):
        return super().trace_entry() + (self.ens_state.clone(), self.ens_stats.clone())


class MultiViewAttackState(AttackState):
    """One batched attack against V = 2..VIEWS_MAX camera views of the same projector and scene ("Multi-view attack"): one
    projector image x through V PCNets, each with its own scene, and one classifier looking at each of the V camera images.
    AttackState (view 0's engines and buffers are its own) with one leased PCNet engine and one leased engine of the classifier per
    further view, the decision over all views (spaa_decide_views), the V backward passes down to the projector image and their
    combination there (spaa_ens_sumsq + spaa_views_combine): the mean of the views' stealth gradients on the colour step, the weighted
    sum of the views' unit gradient images on the adversarial step.  `state[:, 3]` counts the fooled views; each view's top-1 is in
    `view_state`, its p1, target logit, caml2 and camdE in `view_stats`.  `focus`: a view that is already fooled rests (weight 0) until
    all are."""
    label = 'views'

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
        # ||g||^2 of the COMBINED gradient comes from spaa_grad_sumsq_ps (a view's adjoint cannot sum it in its epilogue), and the
        # views' backward passes read the clamp gate from x
        self.ss_tiles, self.clamp_bits = 0, None
        self.partial_ss = torch.zeros(B, self.nblk_p, device=dev)
        more = [self._lease_view(m, classifier, sc, setup_info, whose="every view's ") for m, sc in zip(self.pcnets[1:], self._scenes[1:])]
        self.engs, self.clfs, self.scene4s, self.scene_labs = ([own] + [view[i] for view in more] for i, own in
                                                               enumerate((self.eng, self.clf, self.scene4, self.scene_lab)))
        self.g_cols, self.gPs, self.partial_losses, self.view_g_logits = ([own] + [torch.zeros_like(own) for _ in more] for own in
                                                                          (self.g_col, self.gP, self.partial_loss, self.g_logits))
        self.cam_bests = [self.cam_best] + [scene4.clone() for scene4 in self.scene4s[1:]]
        if self.any_ssim:
            self.ssim_partials += [torch.zeros_like(self.ssim_partials[0]) for _ in more]
            self.ssims += [torch.zeros_like(self.ssim) for _ in more]
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
            self._stealth_loss_ps(y, v)
            self._ssim_term(y, v)
            ys.append(y)
        self._ys, self._y, self._uniform = ys, ys[0], False
        prjl2 = self._prjl2_fwd()
        _lib.call('spaa_decide_views', _lib.ptr_array(logits), self.V, self.clf.ncls, p(self.target),
                  _lib.ptr_array(self.partial_losses), self.nblk_c, self.HWc, prjl2, p(self.ps_params), p(self.ps_flags),
                  float(p_thresh), adv_w / B * self.gs_adv, int(self.focus), p(self.state),
                  p(self.stats), p(self.view_state), p(self.view_stats), p(self.view_w), _lib.ptr_array(self.view_g_logits), B)

    def _backward_step(self, adv_lr, col_lr):
        B, p = self.B, _lib.ptr
        gxs = []
        for v, eng in enumerate(self.engs):
            g_adv = self.clfs[v].backward(self.view_g_logits[v], self.attention, self.target)   # :302 (classifier part), view v's seed and map
            gxs.append(self._pcnet_backward(eng, g_adv, self.g_cols[v], self.gPs[v]))
        gs = _lib.ptr_array(gxs)
        _lib.call('spaa_ens_sumsq', gs, self.V, p(self.views_partial), B, self.HWp)
        _lib.call('spaa_views_combine', gs, self.V, p(self.views_partial), self.nblk_p, p(self.view_w), p(self.state), p(self.g), B,
                  self.HWp)
        _lib.call('spaa_grad_sumsq_ps', p(self.g), p(self.x), self.gray, p(self.ps_prjl2_scale), p(self.state), p(self.partial_ss), B,
                  self.HWp)
        self._step_and_track(self.g, adv_lr, col_lr)
        _lib.call('spaa_views_track', _lib.ptr_array(self._ys), _lib.ptr_array(self.cam_bests), self.V, p(self.state), B, self.HWc)

    def trace_entry(self):
        return super().trace_entry() + (self.view_state.clone(), self.view_stats.clone())

    def results(self):
        with torch.cuda.device(self.dev):
            return [to_nchw(c) for c in self.cam_bests], to_nchw(self.x_best, clamp01=True)


class UniversalAttackState(AttackState):
    """One batched attack in which every group of N = universal.size consecutive samples shares ONE projector image:
    AttackState -- one PCNet engine, one classifier engine, one scene per sample, the ordinary per-sample forward and backward passes --
    with the decision per group (spaa_decide_universal: the multi-view rule with members in the place of views, a group fooled when
    universal.need of its members are) and the B gradient images at the projector combined group by group (spaa_universal_combine: the
    mean on the colour step, the weighted sum of the members' unit images on the adversarial step) into `g`, whose N equal rows per
    group then take the ordinary step.  The N rows of a group hold the same `x`, `x_best`, `state` and `stats` words at every iteration,
    bitwise.  `state[:, 3]` counts the group's fooled members; each sample's own top-1 is in `uni_state`, its p1, target logit, caml2
    and camdE in `uni_stats`.  `focus`: a member that is already fooled rests (weight 0) until the group is fooled."""
    label = 'members'

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, universal, storage='f32', focus=False,
                 attention=None, transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        _universal_supported(universal, pcnet, classifier, storage, None, None, None, 'UniversalAttackState')
        B = len(target_idx)
        universal.groups(B, 'UniversalAttackState')
        if not isinstance(stealth_loss, str) and len(stealth_loss) == B:
            universal.check_uniform('stealth_loss', list(stealth_loss), 'UniversalAttackState')
        self.universal, self.N, self.need, self.focus = universal, int(universal.size), universal.need, bool(focus)
        super().__init__(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage,
                         attention=attention, transfer=transfer)

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)
        B = self.B
        # ||g||^2 of the COMBINED gradient comes from spaa_grad_sumsq_ps (the adjoint's epilogue sums a member's), and the backward
        # pass reads the clamp gate from x
        self.ss_tiles, self.clamp_bits = 0, None
        self.partial_ss = torch.zeros(B, self.nblk_p, device=dev)
        self.uni_state = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        self.uni_stats = torch.zeros(B, 4, device=dev)
        self.uni_w = torch.ones(B, device=dev)
        self.uni_partial = torch.zeros(B, self.nblk_p, device=dev)
        self.uni_coef = torch.zeros(B, device=dev)
        self.g = torch.zeros(B, self.x.shape[1], self.x.shape[2], 4, device=dev)

    def _per_sample(self, targeted, d_thr, table=False):
        """The per-sample table, always; a new (targeted, d_thr) setting must be uniform within every group."""
        before = self._ps_key
        super()._per_sample(targeted, d_thr, table=True)
        if self._ps_key != before:
            tg, dt = self._ps_key
            self._ps_key = None   # (a refused setting is checked again when it comes again)
            self.universal.check_uniform('targeted', list(tg), 'UniversalAttackState')
            self.universal.check_uniform('d_thr', list(dt), 'UniversalAttackState')
            self._ps_key = (tg, dt)

    def _forward_decide(self, targeted, d_thr, p_thresh, adv_w):
        B, p = self.B, _lib.ptr
        self._per_sample(targeted, d_thr)
        y = self.eng.forward(self.x, clamp01=True)                                   # :265, every sample its own scene
        logits = self.clf.forward(y)                                                 # :266
        self._y, self._uniform = y, False
        prjl2 = self._prjl2_fwd()
        self._stealth_loss_ps(y)
        self._ssim_term(y)
        _lib.call('spaa_decide_universal', p(logits), self.clf.ncls, p(self.target), p(self.partial_loss), self.nblk_c, self.HWc, prjl2,
                  p(self.ps_params), p(self.ps_flags), self.N, self.need, float(p_thresh), adv_w / B * self.gs_adv, int(self.focus),
                  p(self.state), p(self.stats), p(self.uni_state), p(self.uni_stats), p(self.uni_w), p(self.g_logits), B)

    def _backward_step(self, adv_lr, col_lr):
        B, p = self.B, _lib.ptr
        g_adv = self._adv_gradient()
        gx = self._pcnet_backward(self.eng, g_adv, self.g_col, self.gP)              # the B members' own gradient images
        _lib.call('spaa_universal_combine', p(gx), self.N, p(self.uni_w), p(self.state), p(self.uni_partial), p(self.uni_coef), p(self.g),
                  B, self.HWp)
        _lib.call('spaa_grad_sumsq_ps', p(self.g), p(self.x), self.gray, p(self.ps_prjl2_scale), p(self.state), p(self.partial_ss), B,
                  self.HWp)
        self._step_and_track(self.g, adv_lr, col_lr)

    def attention_maps(self):
        """[B, 1, Hc, Wc]: every sample's own map (the members are rows of the one classifier engine)."""
        return self._engine_maps(self.clfs)[0]

    def trace_entry(self):
        return super().trace_entry() + (self.uni_state.clone(), self.uni_stats.clone())


class JitterStage:
    """Capture jitter as a stage of a draw chain ("Capture-robust attack"): its device-side counter, the rows `jit` and noise
    keys `key` of spaa_jitter_draw, J images with their clamp gates, J gradient images; `build` returns them by their names on the state."""

    def __init__(self, jitter):
        self.options, self.draws = jitter, int(jitter.draws)

    def build(self, st, first):
        B, J, dev = st.B, st.K, st.dev
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the iteration number the next draw reads
        self.jit = torch.zeros(B, J, 8, device=dev)
        self.key = torch.zeros(B, J, dtype=torch.int32, device=dev)         # (uint32 bit patterns)
        self.ims = [torch.zeros_like(st.g_adv) for _ in range(J)]
        self.gates = [torch.zeros(B, st.HWc, dtype=torch.uint8, device=dev) for _ in range(J)]
        self.grads = [torch.zeros_like(st.g_adv) for _ in range(J)]
        return dict(jit=self.jit, key=self.key, draw_ims=self.ims, draw_gates=self.gates, draw_grads=self.grads,
                    **{'counter' if first else 'jitter_counter': self.counter})

    def forward(self, st, src):
        """Draws this iteration's rows, then draw j of `src`: the camera image y, or (behind another stage) that stage's image j."""
        jt, p, arr = self.options, _lib.ptr, _lib.ptr_array
        jt.draw(self.counter, self.jit, self.key, st.B, st.K, clean0=True)
        each = isinstance(src, list)
        _lib.call('spaa_jitter_fwd_each' if each else 'spaa_jitter_fwd', arr(src) if each else p(src), p(self.jit), p(self.key), st.K,
                  int(bool(jt.quantize)), arr(self.ims), arr(self.gates), st.B, st.eng.Hc, st.eng.Wc)
        return self.ims

    def backward(self, st, gs):
        _lib.call('spaa_jitter_bwd', _lib.ptr_array(gs), _lib.ptr(self.jit), _lib.ptr_array(self.gates), st.K, _lib.ptr_array(self.grads),
                  st.B, st.eng.Hc, st.eng.Wc)
        return self.grads


class PoseStage:
    """Camera-pose jitter as a stage of a draw chain: its device-side counter, the homography rows `table` of
    spaa_pose_draw, the J warped images, the J gradient images of its adjoint.  The first stage only: the warp launches from y."""

    def __init__(self, pose):
        self.options, self.draws = pose, int(pose.draws)

    def build(self, st, first):
        assert first, 'the pose warp has no launch form behind another stage'
        self.counter = torch.zeros(1, dtype=torch.int32, device=st.dev)     # the iteration number the next draw reads
        self.table = torch.zeros(st.B, st.K, 8, device=st.dev)
        self.ims = [torch.zeros_like(st.g_adv) for _ in range(st.K)]
        self.grads = [torch.zeros_like(st.g_adv) for _ in range(st.K)]
        return dict(counter=self.counter, table=self.table, pose_ims=self.ims, pose_grads=self.grads)

    def forward(self, st, y):
        self.options.draw(self.counter, self.table, st.B, st.K, st.eng.Hc, st.eng.Wc, clean0=True)
        _lib.call('spaa_pose_fwd', _lib.ptr(y), _lib.ptr(self.table), st.K, _lib.ptr_array(self.ims), st.B, st.eng.Hc, st.eng.Wc)
        return self.ims

    def backward(self, st, gs):
        _lib.call('spaa_pose_bwd', _lib.ptr_array(gs), _lib.ptr(self.table), st.K, _lib.ptr_array(self.grads), st.B, st.eng.Hc,
                  st.eng.Wc)
        return self.grads


class JpegStage:
    """The camera's JPEG codec as a stage of a draw chain, always the last one: its device-side counter, the quality rows
    `jpeg_rows` of spaa_jpeg_draw, J round-tripped images with their gate bytes, J gradient images, and for 4:2:0 the workspace
    between the two launches of spaa_jpeg_fwd.  It remembers its J input images: the 'soft' adjoint recomputes the coefficients."""

    def __init__(self, jpeg):
        self.options, self.draws = jpeg, int(jpeg.draws)
        self.code, self.soft = JPEG_SUBSAMPLINGS[jpeg.subsampling], int(jpeg.gradient == 'soft')

    def build(self, st, first):
        B, J, dev = st.B, st.K, st.dev
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the iteration number the next draw reads
        self.rows = torch.zeros(B, J, 4, device=dev)
        self.ims = [torch.zeros_like(st.g_adv) for _ in range(J)]
        self.gates = [torch.zeros(B, st.HWc, dtype=torch.uint8, device=dev) for _ in range(J)]
        self.grads = [torch.zeros_like(st.g_adv) for _ in range(J)]
        floats = _lib.load().spaa_jpeg_ws_floats(self.code, J, B, st.eng.Hc, st.eng.Wc)
        self.ws = torch.zeros(floats, device=dev) if floats else None
        self.src = None
        return dict(jpeg_rows=self.rows, jpeg_ims=self.ims, jpeg_gates=self.gates, jpeg_grads=self.grads,
                    **{'counter' if first else 'jpeg_counter': self.counter})

    def forward(self, st, src):
        """Draws this iteration's qualities, then draw j of `src`: the camera image y, or (behind another stage) that stage's image j."""
        self.options.draw(self.counter, self.rows, st.B, st.K, clean0=True)
        self.src = src if isinstance(src, list) else [src] * st.K
        _lib.call('spaa_jpeg_fwd', _lib.ptr_array(self.src), _lib.ptr(self.rows), st.K, self.code, _lib.ptr_array(self.ims),
                  _lib.ptr_array(self.gates), _lib.ptr(self.ws), st.B, st.eng.Hc, st.eng.Wc)
        return self.ims

    def backward(self, st, gs):
        _lib.call('spaa_jpeg_bwd', _lib.ptr_array(gs), _lib.ptr_array(self.src), _lib.ptr(self.rows), st.K, self.code, self.soft,
                  _lib.ptr_array(self.gates), _lib.ptr_array(self.grads), st.B, st.eng.Hc, st.eng.Wc)
        return self.grads


class BlurStage:
    """The camera's lens blur as a stage of a draw chain, behind the pose warp and in front of the sensor and the codec:
    its device-side counter, the tap rows `blur_rows` of spaa_blur_draw, J blurred images, J gradient images.  The filter is linear:
    its adjoint needs neither its input nor a gate."""

    def __init__(self, blur):
        self.options, self.draws = blur, int(blur.draws)

    def build(self, st, first):
        B, J, dev = st.B, st.K, st.dev
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)        # the iteration number the next draw reads
        self.rows = torch.zeros(B, J, 12, device=dev)
        self.ims = [torch.zeros_like(st.g_adv) for _ in range(J)]
        self.grads = [torch.zeros_like(st.g_adv) for _ in range(J)]
        return dict(blur_rows=self.rows, blur_ims=self.ims, blur_grads=self.grads,
                    **{'counter' if first else 'blur_counter': self.counter})

    def forward(self, st, src):
        """Draws this iteration's sigmas, then draw j of `src`: the camera image y, or (behind another stage) that stage's image j."""
        self.options.draw(self.counter, self.rows, st.B, st.K, clean0=True)
        src = src if isinstance(src, list) else [src] * st.K
        _lib.call('spaa_blur_fwd', _lib.ptr_array(src), _lib.ptr(self.rows), st.K, _lib.ptr_array(self.ims), st.B, st.eng.Hc, st.eng.Wc)
        return self.ims

    def backward(self, st, gs):
        _lib.call('spaa_blur_bwd', _lib.ptr_array(gs), _lib.ptr(self.rows), st.K, _lib.ptr_array(self.grads), st.B, st.eng.Hc, st.eng.Wc)
        return self.grads


class DrawAttackState(EnsembleAttackState):
    """One batched attack against J random draws of the camera image per iteration: EnsembleAttackState whose members are J leased
    engines of ONE classifier, member j looking at draw j of y = PCNet(x, s).  The draws come from a chain of `stages` applied to y,
    each drawing its parameters directly before its transform (a device-side counter per stage: a replayed graph advances the
    sequences); the members' gradient images go back to y through the stages' adjoints in reverse order before they are combined.
    Draw 0 is the identity row of every stage, so a sample counts as successful only when the clean capture and every other draw of
    that iteration are fooled; the stealth loss and `cam_best` stay the clean inference.  `state`, `stats`, `ens_state`, `ens_stats` keep
    the ensemble's meaning with draws as members; the stages' buffers are attributes of the state (`counter`: the first stage's)."""
    label = 'draws'

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, stages, storage='f32', transfer=None):
        self.stages = stages
        super().__init__(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage=storage, transfer=transfer)

    def _members(self, classifier, storage):
        return [classifier] * self.stages[0].draws

    def _build(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev):
        super()._build(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, dev)
        for i, stage in enumerate(self.stages):
            vars(self).update(stage.build(self, first=i == 0))

    def _member_logits(self, y):
        ims = y
        for stage in self.stages:
            ims = stage.forward(self, ims)
        return [e.forward(im) for e, im in zip(self.clfs, ims)]                      # :266, once per draw

    def _member_gradients(self):
        gs = super()._member_gradients()
        for stage in reversed(self.stages):
            gs = stage.backward(self, gs)
        return gs


class JitterAttackState(DrawAttackState):
    """The draw attack of one stage, capture jitter: J = jitter.draws perturbed captures per iteration (spaa_jitter_draw,
    spaa_jitter_fwd, spaa_jitter_bwd)."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, jitter, storage='f32', transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        _jitter_supported(jitter, pcnet, classifier, storage, False, 'JitterAttackState')
        self.jitter = jitter
        super().__init__(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, [JitterStage(jitter)], storage,
                         transfer)


class PoseAttackState(DrawAttackState):
    """The draw attack through random homographies: J = pose.draws warped copies per iteration (spaa_pose_draw, spaa_pose_fwd,
    spaa_pose_bwd).  With `jitter` (a CaptureJitter of the same `draws`) draw j is Jitter_j(Pose_j(y)): spaa_jitter_fwd_each behind the
    warp, spaa_jitter_bwd before its adjoint."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, pose, storage='f32', jitter=None,
                 transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        if jitter is not None:
            _jitter_supported(jitter, pcnet, classifier, storage, False, 'PoseAttackState')
        _pose_supported(pose, pcnet, classifier, storage, False, None, jitter, 'PoseAttackState')
        self.pose, self.jitter = pose, jitter
        stages = [PoseStage(pose)] + ([JitterStage(jitter)] if jitter is not None else [])
        super().__init__(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, stages, storage, transfer)


class JpegAttackState(DrawAttackState):
    """The draw attack through the camera's JPEG codec: J = jpeg.draws round trips per iteration at drawn qualities (spaa_jpeg_draw,
    spaa_jpeg_fwd, spaa_jpeg_bwd).  With `pose` and / or `jitter` (of the same `draws`) draw j is Jpeg_j(Jitter_j(Pose_j(y))), the order
    a camera applies them in."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, jpeg, storage='f32', pose=None,
                 jitter=None, transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        if jitter is not None:
            _jitter_supported(jitter, pcnet, classifier, storage, False, 'JpegAttackState')
        if pose is not None:
            _pose_supported(pose, pcnet, classifier, storage, False, None, jitter, 'JpegAttackState')
        _jpeg_supported(jpeg, pcnet, classifier, storage, False, None, jitter, pose, 'JpegAttackState')
        self.pose, self.jitter, self.jpeg = pose, jitter, jpeg
        stages = ([PoseStage(pose)] if pose is not None else []) + ([JitterStage(jitter)] if jitter is not None else [])
        super().__init__(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, stages + [JpegStage(jpeg)], storage,
                         transfer)


class BlurAttackState(DrawAttackState):
    """The draw attack through the camera's lens blur: J = blur.draws defocused copies per iteration at drawn sigmas (spaa_blur_draw,
    spaa_blur_fwd, spaa_blur_bwd).  With `pose`, `jitter` and / or `jpeg` (of the same `draws`) draw j is
    Jpeg_j(Jitter_j(Blur_j(Pose_j(y)))), the optical order: geometry, lens, sensor, codec."""

    def __init__(self, pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, blur, storage='f32', pose=None,
                 jitter=None, jpeg=None, transfer=None):
        pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
        if jitter is not None:
            _jitter_supported(jitter, pcnet, classifier, storage, False, 'BlurAttackState')
        if pose is not None:
            _pose_supported(pose, pcnet, classifier, storage, False, None, jitter, 'BlurAttackState')
        if jpeg is not None:
            _jpeg_supported(jpeg, pcnet, classifier, storage, False, None, jitter, pose, 'BlurAttackState')
        _blur_supported(blur, pcnet, classifier, storage, False, None, jitter, pose, jpeg, None, 'BlurAttackState')
        self.pose, self.jitter, self.jpeg, self.blur = pose, jitter, jpeg, blur
        stages = (([PoseStage(pose)] if pose is not None else []) + [BlurStage(blur)] +
                  ([JitterStage(jitter)] if jitter is not None else []) + ([JpegStage(jpeg)] if jpeg is not None else []))
        super().__init__(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, stages, storage, transfer)
