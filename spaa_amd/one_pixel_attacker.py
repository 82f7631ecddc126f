"""The One-pixel DE attacker of the SPAA comparison (reference: one_pixel_attacker/__init__.py, Su et al.'s attack as adapted by
Nichols & Jasper), behind the reference's signatures: the digital variant (:18-120) and the projector variant (:123-245, below).

`perturb_image(x, im, pixel_size)` and `DigitalOnePixelAttacker(class_names, classifier_crop_sz)` keep the reference's return
values and quirks: uint8 truncation `(im * 255).type(torch.uint8)`, `x.astype(int)`, squares painted in list order (a later
pixel overwrites an earlier one), the bounds and population multiplier of :80-86, `1 - p[target]` / `p[target]` as the energy,
the verbose lines, the final batch-2 classification of (im, im_adv) and the one-row DataFrame.  DE is spaa_amd.de, SciPy's
`differential_evolution` restated with batched, exact speculative evaluation.

Two routes:
  fast     a spaa_amd.Classifier with sort_results=False (what both reference callers construct).  The image is quantised
           once and uploaded; per batch, the candidates' integer vectors go up as int32 and spaa_onepixel_preproc paints them
           while it gathers the classifier input, the body runs, spaa_onepixel_score reduces the logits to energy / argmax /
           max p; three numbers per candidate come back.  Energies are memoised by integer vector for the attack, so float
           vectors that truncate alike get bit-identical energies (ties decide `<=` acceptance) and are evaluated once; the
           callback reads the best vector's memoised argmax instead of classifying again.
  foreign  any other classifier callable, or sort_results=True: every candidate goes to `classifier(im_adv, crop_sz)` as in
           the reference, through the same DE driver, with the image left where the caller put it (CPU-testable with the
           oracle classifier).

`ProjectorOnePixelAttacker(class_names, cfg, *, capture)` perturbs the PROJECTOR image; every candidate is projected, captured and
the capture classified.  No window or camera is opened: `capture` is the project-and-capture step.
  fast     capture = SimulatedCapture(pcnet, cam_scene) and a spaa_amd.Classifier with sort_results=False.  Per batch:
           spaa_onepixel_warp paints the candidates' squares while it samples the shared grey projector image through the PCNet
           engine's tap table (no candidate's projector image exists), PCNetEngine.forward_from_xw runs ShadingNet,
           spaa_capture_preproc applies the camera's 8-bit step while it gathers the classifier input, the body runs and
           spaa_onepixel_score reduces the logits.  Memo and callback as above (one shared evaluator base).
  foreign  any callable capture(im_prj uint8 [3,Hp,Wp]) -> im_cam float [3,Hc,Wc] (a real ProCams pair, the CPU oracle), or a
           SimulatedCapture with any other classifier: one capture and one classifier call per candidate, in the reference's order.
"""
import numpy as np
import pandas as pd
import torch

from . import _lib
from .de import DifferentialEvolution

SMALL_BATCH = 8   # fast route: batches of at most this many new candidates run on a second, small engine


def perturb_image(x, im, pixel_size):
    """one_pixel_attacker/__init__.py:18-44: uint8 copy of `im` with a pixel_size x pixel_size square (odd side
    2 * (pixel_size // 2) + 1) of colour (r, g, b) at (row, col) per 5-tuple of `x`, painted in order."""
    im_adv = im.clone() if im.dtype == torch.uint8 else (im * 255).type(torch.uint8)
    d = pixel_size // 2
    x = x.astype(int)
    for pixel in np.split(x, len(x) // 5):
        r, c, *rgb = pixel
        # the reference's two loops as one indexed assignment (same indices, negative ones wrap as in Python)
        rows = torch.arange(r - d, r + d + 1)[:, None]
        cols = torch.arange(c - d, c + d + 1)[None, :]
        im_adv[:, rows, cols] = torch.tensor(rgb, dtype=torch.uint8).to(im_adv.device)[:, None, None]
    return im_adv


class _MemoEvaluator:
    """A batched objective params [S, N] -> float32 energies [S], memoised by the truncated integer vector; `_run(rows, keys)`
    (subclasses) evaluates new integer vectors and hands (energy bits, argmax, max p bits) [3, S] int32 to `_record`."""

    def __init__(self, pixel_count, pixel_size, target_idx, targeted, max_batch, trace):
        self.npix, self.pixel_size = pixel_count, pixel_size
        self.target, self.targeted = int(target_idx), bool(targeted)
        self.trace, self.memo, self.classified = trace, {}, 0
        self.k = max_batch
        self.sizes = sorted({min(max_batch, SMALL_BATCH), max_batch})

    def _check_target(self, target_idx):
        if not 0 <= self.target < self.ncls:
            raise ValueError(f'target_idx {target_idx} out of range for {self.ncls} classes')

    def _padded(self, rows):
        """(engine batch B, int32 [B, 5 npix]): the rows, padded with repeats of a valid candidate."""
        S = len(rows)
        B = next(b for b in self.sizes if b >= S)
        cand = np.empty((B, 5 * self.npix), dtype=np.int32)
        cand[:S] = rows
        cand[S:] = rows[-1]
        return B, cand

    def _score(self, logits, B, S):
        _lib.call('spaa_onepixel_score', _lib.ptr(logits), self.ncls, self.target, int(self.targeted), _lib.ptr(self.res[0]),
                  _lib.ptr(self.res[1]), _lib.ptr(self.res[2]), B)
        return np.ascontiguousarray(self.res[:, :S].cpu().numpy())

    def _record(self, rows, keys, res):
        energy, pmax = res[0].view(np.float32), res[2].view(np.float32)
        for i, k in enumerate(keys):
            self.memo[k] = (energy[i], int(res[1, i]), pmax[i])
            if self.trace is not None:
                self.trace.append((rows[i].copy(), energy[i], int(res[1, i])))
        self.classified += len(rows)

    def __call__(self, params):
        ints = np.asarray(params).astype(int)
        keys = [r.tobytes() for r in ints]
        new, seen = [], set()
        for i, k in enumerate(keys):
            if k not in self.memo and k not in seen:
                new.append(i)
                seen.add(k)
        for s in range(0, len(new), self.k):
            sel = new[s:s + self.k]
            self._run(ints[sel], [keys[i] for i in sel])
        return np.array([self.memo[k][0] for k in keys], dtype=np.float32)

    def lookup(self, x):
        """(energy, argmax, max p) of a vector already evaluated (the best member, in the callback)."""
        return self.memo[np.asarray(x).astype(int).tobytes()]


def _quantised_base(im):
    """perturb_image's quantisation of the unperturbed image, once: [1, H, W, 4] fp32 (host), u8 / 255 by true division."""
    q = im.clone() if im.dtype == torch.uint8 else (im * 255).type(torch.uint8)
    base = torch.zeros(1, im.shape[1], im.shape[2], 4)
    base[0, :, :, :3] = (q.cpu().type(torch.float32) / 255).permute(1, 2, 0)
    return base


class _FastEvaluator(_MemoEvaluator):
    """The digital fast route: paint + classifier preprocessing in one launch, body, score."""

    def __init__(self, clf, im, crop_sz, pixel_count, pixel_size, target_idx, targeted, max_batch, trace):
        self.dev = clf.device
        if self.dev.type != 'cuda':
            raise RuntimeError('spaa_amd.Classifier runs on the GPU only (no CPU fallback); got device=%s' % self.dev)
        super().__init__(pixel_count, pixel_size, target_idx, targeted, max_batch, trace)
        _, self.H, self.W = im.shape
        base = _quantised_base(im)       # classify()'s u8 -> float (true division)
        with _lib.on_device(self.dev):
            self.base = base.to(self.dev)
            self.engines = {b: clf.engine(b, (self.H, self.W), tuple(crop_sz), owner=self) for b in self.sizes}
            self.cand = torch.zeros(max_batch, 5 * pixel_count, dtype=torch.int32, device=self.dev)
            self.res = torch.zeros(3, max_batch, dtype=torch.int32, device=self.dev)   # energy (f32 bits), argmax, max p (f32 bits)
        self.ncls = self.engines[self.sizes[0]].ncls
        self._check_target(target_idx)

    def _run(self, rows, keys):
        S = len(rows)
        B, cand = self._padded(rows)
        eng = self.engines[B]
        with _lib.on_device(self.dev):
            c = self.cand[:B]
            c.copy_(torch.from_numpy(cand))
            _lib.call('spaa_onepixel_preproc', _lib.ptr(self.base), _lib.ptr(c), B, self.npix, self.pixel_size, _lib.ptr(eng.pre),
                      self.H, self.W, eng.cy0, eng.cx0, eng.ch, eng.cw, eng.oh, eng.ow, eng._mean, eng._std)
            res = self._score(eng.forward_pre(), B, S)
        self._record(rows, keys, res)


class SimulatedCapture:
    """A trained PCNet as the project-and-capture step of ProjectorOnePixelAttacker: capture = pcnet(prj_u8 / 255, cam_scene), with
    `quantize` followed by the camera's 8-bit step trunc(y * 255) / 255 (the reference's capture() returns uint8 / 255, :159).
    Callable as any capture (the foreign route); with a spaa_amd.Classifier the attacker drives the PCNet engine directly."""

    def __init__(self, pcnet, cam_scene, *, quantize=True):
        from .models import PCNet
        if not isinstance(pcnet, PCNet):
            raise TypeError(f'SimulatedCapture needs a spaa_amd.PCNet, got {type(pcnet).__name__}')
        self.device = pcnet.shading_net.conv1.weight.device
        if self.device.type != 'cuda':
            raise RuntimeError('SimulatedCapture runs the PCNet on the GPU only (no CPU fallback); got device=%s' % self.device)
        self.pcnet, self.quantize = pcnet, bool(quantize)
        while cam_scene.ndim < 4:
            cam_scene = cam_scene[None]
        if cam_scene.shape[0] != 1 or tuple(cam_scene.shape[-2:]) != tuple(pcnet.warping_net.out_size):
            raise ValueError(f'cam_scene must be one image of the PCNet\'s camera size {tuple(pcnet.warping_net.out_size)}, got '
                             f'{tuple(cam_scene.shape)}')
        self.cam_scene = cam_scene.detach().float().to(self.device)

    @staticmethod
    def _over255(t):
        # (a true division on any device: `t / 255` with a Python scalar is a multiplication by 1 / 255 on the GPU)
        return t.type(torch.float32) / torch.full((), 255.0, device=t.device)

    def __call__(self, im_prj):
        x = self._over255(im_prj) if im_prj.dtype == torch.uint8 else im_prj
        with torch.no_grad():
            y = self.pcnet(x[None].to(self.device), self.cam_scene)[0]
        return self._over255((y * 255).type(torch.uint8)) if self.quantize else y


class _CaptureEvaluator(_MemoEvaluator):
    """The projector fast route: paint + warp in one launch, ShadingNet, 8-bit step + classifier preprocessing in one launch, body,
    score.  Only the integer vectors go up and three numbers per candidate come back."""

    def __init__(self, cap, clf, im, crop_sz, pixel_count, pixel_size, target_idx, targeted, max_batch, trace):
        from .models import to_nhwc4
        self.dev = clf.device
        if self.dev.type != 'cuda':
            raise RuntimeError('spaa_amd.Classifier runs on the GPU only (no CPU fallback); got device=%s' % self.dev)
        def index(d):     # ('cuda' is the current device)
            return d.index if d.index is not None else torch.cuda.current_device()
        if cap.device.type != self.dev.type or index(cap.device) != index(self.dev):
            raise RuntimeError(f'the PCNet ({cap.device}) and the classifier ({self.dev}) must be on one device')
        super().__init__(pixel_count, pixel_size, target_idx, targeted, max_batch, trace)
        _, self.Hp, self.Wp = im.shape
        self.quantize = cap.quantize
        base = _quantised_base(im)       # project()'s (im * 255) -> u8, then PCNet's input u8 / 255
        with _lib.on_device(self.dev):
            self.base = base.to(self.dev)
            scene4 = to_nhwc4(cap.cam_scene)
            self.pc, self.engines = {}, {}
            for b in self.sizes:
                pe = cap.pcnet.engine(b, (self.Hp, self.Wp), owner=self, storage='f32')
                pe.set_scene(scene4.expand(b, -1, -1, -1).contiguous())
                self.pc[b] = pe
                self.engines[b] = clf.engine(b, (pe.Hc, pe.Wc), tuple(crop_sz), owner=self)
            self.cand = torch.zeros(max_batch, 5 * pixel_count, dtype=torch.int32, device=self.dev)
            self.res = torch.zeros(3, max_batch, dtype=torch.int32, device=self.dev)
        self.ncls = self.engines[self.sizes[0]].ncls
        self._check_target(target_idx)

    def _run(self, rows, keys):
        from .models import C_ptr
        S = len(rows)
        B, cand = self._padded(rows)
        pe, eng = self.pc[B], self.engines[B]
        with _lib.on_device(self.dev):
            c = self.cand[:B]
            c.copy_(torch.from_numpy(cand))
            _lib.call('spaa_onepixel_warp', _lib.ptr(self.base), _lib.ptr(c), B, self.npix, self.pixel_size, C_ptr(pe.tap_src),
                      _lib.ptr(pe.tap_wm), _lib.ptr(pe.scene), _lib.ptr(pe.a['xw']), _lib.ptr(pe.a['cat8']) if pe.needs_cat8 else None,
                      self.Hp, self.Wp, pe.Hc, pe.Wc)
            y = pe.forward_from_xw()
            _lib.call('spaa_capture_preproc', _lib.ptr(y), _lib.ptr(eng.pre), B, pe.Hc, pe.Wc, eng.cy0, eng.cx0, eng.ch, eng.cw, eng.oh,
                      eng.ow, eng._mean, eng._std, int(self.quantize))
            res = self._score(eng.forward_pre(), B, S)
        self._record(rows, keys, res)


def _solve_de(att, ev, predict, im, classifier, target_idx, targeted_attack, pixel_count, pixel_size, maxiter, popsize, verbose,
              true_label, updating, seed, max_batch, trace):
    """The part of `attack` both attackers share (:78-100 / :198-221): bounds, population multiplier, objective, callback and DE.
    `ev`: None (foreign route: `predict(x) -> p` per candidate, `att.attack_success` as callback) or a function n_pop -> memoising
    evaluator (fast route: the callback reads the memo)."""
    d = pixel_size // 2
    _, n_rows, n_cols = im.shape
    bounds = [(d, n_rows - 1 - d), (d, n_cols - 1 - d), (0, 255), (0, 255), (0, 255)] * pixel_count
    if n_rows - 1 - d < d or n_cols - 1 - d < d:
        raise ValueError(f'pixel_size {pixel_size} leaves no valid square centre in a {n_rows}x{n_cols} image')
    popmul = max(1, popsize // len(bounds))
    fast = ev is not None

    if fast:
        n_pop = max(5, popmul * len(bounds))
        ev = ev(n_pop if max_batch is None else int(max_batch))
        objective = ev

        def callback_fn(x, convergence):
            e, pred, p_max = ev.lookup(x)
            if verbose:
                att._report(target_idx, np.float32(1) - e if targeted_attack else e, pred, p_max, targeted_attack, true_label)
            if (targeted_attack and pred == target_idx) or (not targeted_attack and pred != target_idx):
                return True
    else:
        def predict_one(x):
            p = predict(x, im, classifier, pixel_size)
            e = 1 - p[0, target_idx] if targeted_attack else p[0, target_idx]
            if trace is not None:
                trace.append((x.astype(int), e, int(p[0].argmax())))
            return e

        def objective(params):
            return np.array([predict_one(x) for x in params])

        def callback_fn(x, convergence):
            return att.attack_success(x, im, target_idx, classifier, pixel_size, targeted_attack, verbose, true_label)

    de_ret = DifferentialEvolution(objective, bounds, maxiter=maxiter, popsize=popmul, recombination=1, atol=-1,
                                   callback=callback_fn, polish=False, seed=seed, updating=updating,
                                   max_batch=(1 if max_batch is None and not fast else max_batch)).solve()
    if fast:
        de_ret['classified'] = ev.classified     # candidates that went through the classifier (memo misses)
    att.last_result = de_ret
    return de_ret


def _result_frame(classifier, p, pixel_count, target_idx, targeted_attack):
    """The one-row DataFrame of :106-117 / :230-242 from the batch-2 probabilities (original, adversarial)."""
    true_p, pred_p = p[0].max(), p[1].max()
    true_idx, pred_idx = p[0].argmax(), p[1].argmax()
    if targeted_attack:
        success = pred_idx == target_idx
    else:
        success = pred_idx != true_idx
    cdiff = p[0, target_idx] - p[1, target_idx]
    return pd.DataFrame([[classifier.name, pixel_count, true_idx, pred_idx, success, true_p, pred_p, cdiff]],
                        columns=['classifier', 'pixel_count', 'true_idx', 'pred_idx', 'success', 'true_p', 'pred_p', 'cdiff'])


class _OnePixelAttacker:
    """What the two attackers share: the verbose line, the DE callback and the call.  A subclass supplies `_predict(x, im, classifier,
    pixel_size) -> p` (one candidate through its route), `_gt(true_label)` (the line's GT field) and `attack`."""
    last_result = None     # the DE result of the last attack (x, fun, nfev, nit, success, message, evaluated, ...)

    def _report(self, target_idx, p_target, pred, p_max, targeted_attack, true_label):
        if targeted_attack:
            print(f'Target: {self.class_names[target_idx]:<20} ({p_target:.2f}) | '
                  f'Pred: {self.class_names[pred]:<20} ({p_max:.2f}) | '
                  f'GT: {self._gt(true_label)}')
        else:
            print(f'Untargeted | Pred: {self.class_names[pred]:<20} ({p_max:.2f}) | GT: {self._gt(true_label)}')

    def attack_success(self, x, im, target_idx, classifier, pixel_size, targeted_attack=False, verbose=False, true_label=None):
        p = self._predict(x, im, classifier, pixel_size)
        if verbose:
            self._report(target_idx, p[0, target_idx], p[0].argmax(), p[0].max(), targeted_attack, true_label)
        if (targeted_attack and p[0].argmax() == target_idx) or (not targeted_attack and p[0].argmax() != target_idx):
            return True

    def __call__(self, im, classifier, targeted_attack=False, target_idx=None, pixel_count=1, pixel_size=1, maxiter=75, popsize=400,
                 verbose=False, true_label=None, **kw):
        return self.attack(im, classifier, targeted_attack, target_idx, pixel_count, pixel_size, maxiter, popsize, verbose,
                           true_label, **kw)


class DigitalOnePixelAttacker(_OnePixelAttacker):
    """one_pixel_attacker/__init__.py:47-108."""

    def __init__(self, class_names, classifier_crop_sz):
        self.class_names = class_names
        self.classifier_crop_sz = classifier_crop_sz

    def perturb_and_predict(self, x, im, classifier, pixel_size):
        im_adv = perturb_image(x, im, pixel_size)
        _, p, _ = classifier(im_adv, self.classifier_crop_sz)
        return p

    def _predict(self, x, im, classifier, pixel_size):
        return self.perturb_and_predict(x, im, classifier, pixel_size)

    def _gt(self, true_label):       # (the digital attack is given the true class id)
        return f'{self.class_names[true_label]:<20}'

    def attack(self, im, classifier, targeted_attack=False, target_idx=None, pixel_count=1, pixel_size=1, maxiter=75, popsize=400,
               verbose=False, true_label=None, *, updating='immediate', seed=None, max_batch=None, trace=None):
        """The reference's attack (:73-105); returns (DataFrame, im_adv).  Keyword-only extras: `updating` ('immediate', the
        reference's, or 'deferred'); `seed` (None: numpy's global RandomState, as the reference; an int or a RandomState);
        `max_batch` (candidates per evaluation batch; default the population size on the fast route, 1 on the foreign one);
        `trace` (a list: receives (integer vector, energy, argmax) of every candidate evaluated, in evaluation order)."""
        from .classifier import Classifier

        ev = None
        if isinstance(classifier, Classifier) and not classifier.sort_results:
            def ev(k):
                return _FastEvaluator(classifier, im, self.classifier_crop_sz, pixel_count, pixel_size, target_idx, targeted_attack, k,
                                      trace)
        de_ret = _solve_de(self, ev, self.perturb_and_predict, im, classifier, target_idx, targeted_attack, pixel_count, pixel_size,
                           maxiter, popsize, verbose, true_label, updating, seed, max_batch, trace)

        im_adv = perturb_image(de_ret.x, im, pixel_size).type(torch.float32) / 255
        _, p, _ = classifier(torch.stack((im, im_adv), 0), self.classifier_crop_sz)  # p and idx are sorted, not the original orders.
        return _result_frame(classifier, p, pixel_count, target_idx, targeted_attack), im_adv


class ProjectorOnePixelAttacker(_OnePixelAttacker):
    """one_pixel_attacker/__init__.py:123-245 without the hardware: `cfg` is the setup info (`prj_im_sz`, `prj_brightness`,
    `cam_im_sz`, `classifier_crop_sz` are read; `prj_screen_sz`, `prj_offset`, `cam_raw_sz`, `cam_crop_sz`, `delay_*` are accepted and
    ignored), `capture` the project-and-capture step: a SimulatedCapture or any callable
    capture(im_prj uint8 [3,Hp,Wp]) -> im_cam float [3,Hc,Wc] in [0, 1]."""

    def __init__(self, class_names, cfg, *, capture):
        if not callable(capture):
            raise TypeError('capture must be a SimulatedCapture or a callable im_prj uint8 [3,Hp,Wp] -> im_cam float [3,Hc,Wc]')
        self.prj_im_sz, self.prj_brightness = tuple(cfg['prj_im_sz']), cfg['prj_brightness']
        self.cam_im_sz = tuple(cfg['cam_im_sz'])
        self.classifier_crop_sz = tuple(cfg['classifier_crop_sz'])
        self.capture = capture
        self.class_names = class_names
        self.im_prj_org = None
        self.im_cam_org = None

    def perturb_project_capture(self, x, im, pixel_size):
        im_prj_adv = perturb_image(x, im, pixel_size)
        im_cam_adv = self.capture(im_prj_adv)
        return im_prj_adv, im_cam_adv

    def step_and_predict(self, x, im, classifier, pixel_size):
        im_prj_adv, im_cam_adv = self.perturb_project_capture(x, im, pixel_size)
        with torch.no_grad():
            _, p, _ = classifier(im_cam_adv, self.classifier_crop_sz)
        return p

    def _predict(self, x, im, classifier, pixel_size):
        return self.step_and_predict(x, im, classifier, pixel_size)

    def _gt(self, true_label):       # (the driver passes the true class's name)
        return f'{true_label:<15}'

    def attack(self, im, classifier, targeted_attack=False, target_idx=None, pixel_count=1, pixel_size=1, maxiter=75, popsize=400,
               verbose=False, true_label=None, *, updating='immediate', seed=None, max_batch=None, trace=None):
        """The reference's attack (:193-242) on the initial projector image `im`; returns (DataFrame, im_prj_adv uint8, im_cam_adv
        float).  `self.im_cam_org` (the captured scene) must be set, as the reference's driver does.  Keyword-only extras as on
        DigitalOnePixelAttacker.attack."""
        from .classifier import Classifier
        from .img_proc import center_crop as cc

        if self.im_cam_org is None:
            raise RuntimeError('set im_cam_org (the camera-captured scene) before attacking')
        ev = None
        if isinstance(self.capture, SimulatedCapture) and isinstance(classifier, Classifier) and not classifier.sort_results:
            def ev(k):
                return _CaptureEvaluator(self.capture, classifier, im, self.classifier_crop_sz, pixel_count, pixel_size, target_idx,
                                         targeted_attack, k, trace)
        de_ret = _solve_de(self, ev, self.step_and_predict, im, classifier, target_idx, targeted_attack, pixel_count, pixel_size,
                           maxiter, popsize, verbose, true_label, updating, seed, max_batch, trace)

        im_prj_adv, im_cam_adv = self.perturb_project_capture(de_ret.x, im, pixel_size)
        with torch.no_grad():
            _, p, _ = classifier(torch.stack((cc(self.im_cam_org.to(im_cam_adv.device), self.classifier_crop_sz),
                                              cc(im_cam_adv, self.classifier_crop_sz)), 0), self.classifier_crop_sz)
        return _result_frame(classifier, p, pixel_count, target_idx, targeted_attack), im_prj_adv, im_cam_adv
