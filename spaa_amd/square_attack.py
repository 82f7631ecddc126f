"""The Square Attack on the projector image (Andriushchenko, Croce, Flammarion, Hein: "Square Attack: a query-efficient black-box
adversarial attack via random search", ECCV 2020): a query-based attacker that needs scores only -- no gradient, no model of the
projector-camera pair -- and so also runs against a real ProCams pair through `capture=<callable>`.  DESIGN.md 7r fixes the algorithm;
in short, per sample: the current projector image is uint8, every value clamp(c0 +/- eps8, 0, 255) around the grey level
c0 = trunc(prj_brightness * 255).  Iteration 0 captures the vertical stripes; iteration t paints K = `proposals` constant-colour squares
of side h(t) on the current image, captures and classifies each, takes the one of smallest loss (ties to the lowest k) and keeps it
iff its loss is below the best so far (strict; NaN never).  A sample whose accepted image succeeds by spaa()'s rule (untargeted: top-1
!= label; targeted: top-1 == target with probability > p_thresh) rests: no more queries are spent on it.

`ProjectorSquareAttacker(class_names, cfg, *, capture)` takes the cfg fields and the `capture` of ProjectorOnePixelAttacker.  Two routes:
  fast     capture = SimulatedCapture(pcnet, cam_scene) and a spaa_amd.Classifier with sort_results=False.  Engines of batch B K are leased
           once and everything stays on the device (csrc/square_ops.hip): spaa_square_propose draws the squares, spaa_square_warp paints
           them while it samples each sample's uint8 image through the PCNet engine's tap table, PCNetEngine.forward_from_xw,
           spaa_capture_preproc and the classifier body run as for the One-pixel attacker, spaa_square_score reduces the logits and
           decides, spaa_square_commit paints the accepted squares and keeps their captures.  The host reads the `done` column every
           `check_every` iterations.
  foreign  any callable capture(im_prj uint8 [3,Hp,Wp]) -> im_cam float [3,Hc,Wc] and any classifier callable (raw scores first, as
           spaa_amd.Classifier returns them): the same algorithm from the Python-integer draws below, the losses in float64, one capture
           and one classifier call per candidate in (b, k) order.  Needs no GPU of its own.
Both are state objects with `step()` (one iteration) that `attack` drives; tests drive them one iteration at a time.
"""
import math

import numpy as np
import torch

from . import _lib

M32 = 0xffffffff
FIRST_INIT, FIRST_PROPOSE = 0x27d4eb2f, 0x165667b1     # the first constants of the two tables (csrc/square_ops.hip)
MAX_PROPOSALS = 8
SCHEDULE = ((10, 1), (50, 2), (200, 4), (500, 8), (1000, 16), (2000, 32), (4000, 64), (6000, 128), (8000, 256))   # it <= bound: p_init / d


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw_word(first, seed, t, b, k, i):
    """draw_rng.hpp's draw_word in Python integers."""
    h = mix32((seed & M32) ^ first)
    for v in (t, b, k, i):
        h = mix32(h ^ (v & M32))
    return h


def centre(prj_brightness):
    """c0: the uint8 grey level of the unperturbed projector image, as (brightness * ones).mul(255).type(uint8) gives it."""
    return int(np.float32(prj_brightness) * np.float32(255))


def perturbed(c0, eps8, plus):
    return min(255, max(0, c0 + eps8 if plus else c0 - eps8))


def square_side(t, n_iters, p_init, Hp, Wp):
    """The side h of iteration t (1-based) of n_iters: the paper's piecewise-constant schedule on it = int(t / n_iters * 10000)."""
    it = int(t / n_iters * 10000)
    d = next((d for bound, d in SCHEDULE if it <= bound), 512)
    return min(max(int(round(math.sqrt(p_init / d * Hp * Wp))), 1), min(Hp, Wp) - 1)


def stripes(seed, b, c0, eps8, Hp, Wp):
    """uint8 [Hp, Wp, 3]: column w, channel ch = c0 +/- eps8 by bit 0 of the word (seed, 0, b, w, ch)."""
    row = np.array([[perturbed(c0, eps8, draw_word(FIRST_INIT, seed, 0, b, w, ch) & 1) for ch in range(3)] for w in range(Wp)], dtype=np.uint8)
    return np.broadcast_to(row, (Hp, Wp, 3)).copy()


def proposal(seed, t, b, k, h, c0, eps8, Hp, Wp):
    """(r, c, h, R, G, B, 0, 0) of proposal k of sample b at iteration t."""
    s = draw_word(FIRST_PROPOSE, seed, t, b, k, 2)
    return (draw_word(FIRST_PROPOSE, seed, t, b, k, 0) % (Hp - h + 1), draw_word(FIRST_PROPOSE, seed, t, b, k, 1) % (Wp - h + 1), h,
            perturbed(c0, eps8, s & 1), perturbed(c0, eps8, (s >> 1) & 1), perturbed(c0, eps8, (s >> 2) & 1), 0, 0)


def score_row(logits, y, targeted):
    """(loss, top-1, p1) of one row of logits in float64."""
    l = np.asarray(logits, dtype=np.float64).reshape(-1)
    mx = l.max()
    se = np.exp(l - mx).sum()
    loss = (mx + math.log(se)) - l[y] if targeted else l[y] - np.delete(l, y).max()
    return float(loss), int(np.argmax(l)), float(1.0 / se)


def choose(losses, best_loss):
    """(k*, accepted): the smallest loss, ties to the lowest k, NaN never; accepted iff it is below best_loss (strict)."""
    lo, ks = math.inf, -1
    for k, l in enumerate(losses):
        if l < lo:
            lo, ks = l, k
    return ks, ks >= 0 and lo < best_loss


def succeeds(top1, p1, y, targeted, p_thresh):
    return (top1 == y and p1 > p_thresh) if targeted else top1 != y


def unpack_u8(x):
    """packed int32 [B, Hp, Wp] (R | G << 8 | B << 16) -> uint8 [B, 3, Hp, Wp]."""
    return torch.stack([(x >> s) & 255 for s in (0, 8, 16)], 1).to(torch.uint8)


def _checked(n_cls, target_idx, targeted, eps8, n_iters, p_init, proposals, p_thresh, seed, check_every, b_off, prj_sz):
    """The request both routes share, checked: (labels, targeted flags)."""
    labels = [int(v) for v in np.asarray(target_idx).reshape(-1)]
    if not labels:
        raise ValueError('target_idx is empty')
    flags = [bool(targeted)] * len(labels) if np.ndim(targeted) == 0 else [bool(v) for v in targeted]
    if len(flags) != len(labels):
        raise ValueError(f'targeted has {len(flags)} entries for {len(labels)} samples')
    if any(not 0 <= v < n_cls for v in labels):
        raise ValueError(f'target_idx {labels} out of range for {n_cls} classes')
    if isinstance(eps8, bool) or not isinstance(eps8, (int, np.integer)) or not 1 <= eps8 <= 127:
        raise ValueError(f'eps8 must be an integer in 1..127 (8-bit levels around the grey image), got {eps8!r}')
    if not isinstance(n_iters, (int, np.integer)) or n_iters < 1:
        raise ValueError(f'n_iters must be a positive integer, got {n_iters!r}')
    if not 0 < p_init <= 1:
        raise ValueError(f'p_init must lie in (0, 1], got {p_init!r}')
    if not isinstance(proposals, (int, np.integer)) or not 1 <= proposals <= MAX_PROPOSALS:
        raise ValueError(f'proposals must be an integer in 1..{MAX_PROPOSALS}, got {proposals!r}')
    if not 0 <= p_thresh <= 1:
        raise ValueError(f'p_thresh must lie in [0, 1], got {p_thresh!r}')
    if not isinstance(seed, (int, np.integer)) or not 0 <= seed <= M32:
        raise ValueError(f'seed must be an integer in 0..2^32 - 1, got {seed!r}')
    if not isinstance(check_every, (int, np.integer)) or check_every < 1:
        raise ValueError(f'check_every must be a positive integer, got {check_every!r}')
    if not isinstance(b_off, (int, np.integer)) or b_off < 0 or b_off + len(labels) > 0x7fffffff:
        raise ValueError(f'b_off must be a non-negative integer, got {b_off!r}')
    if min(prj_sz) < 2:
        raise ValueError(f'the projector image {tuple(prj_sz)} leaves no square side in 1..min(Hp, Wp) - 1')
    return labels, flags


class _SquareState:
    """What the two routes share: the request, the iteration counter `t` (the next iteration; 0 = the stripes) and the side schedule."""

    def __init__(self, labels, flags, prj_sz, c0, eps8, n_iters, p_init, K, p_thresh, seed, b_off):
        self.labels, self.flags, self.B, self.K = labels, flags, len(labels), int(K)
        (self.Hp, self.Wp), self.c0, self.eps8 = prj_sz, c0, int(eps8)
        self.n_iters, self.p_init, self.p_thresh, self.seed, self.b_off = int(n_iters), float(p_init), float(p_thresh), int(seed), int(b_off)
        self.t, self.h = 0, 0

    def _side(self):
        return 0 if self.t == 0 else square_side(self.t, self.n_iters, self.p_init, self.Hp, self.Wp)


class ForeignSquareState(_SquareState):
    """The foreign route.  x_u8 uint8 [B, Hp, Wp, 3], prop int [B, K, 8], rows float64 [B, K, 4] (loss, top-1, p1, 0), best_loss float64
    [B], state int [B, 4] = (accepted, k*, done, queries), cam_best: the capture of every sample's current image."""

    def __init__(self, capture, classifier, crop_sz, *args):
        super().__init__(*args)
        self.capture, self.classifier, self.crop_sz = capture, classifier, tuple(crop_sz)
        B, K = self.B, self.K
        self.x_u8 = np.stack([stripes(self.seed, self.b_off + b, self.c0, self.eps8, self.Hp, self.Wp) for b in range(B)])
        self.prop = np.zeros((B, K, 8), dtype=np.int64)
        self.rows = np.zeros((B, K, 4))
        self.best_loss = np.full(B, np.inf)
        self.state = np.zeros((B, 4), dtype=np.int64)
        self.cam_best = [None] * B
        self.logits = {}                             # (b, k) -> the float64 logits of the last candidate evaluated there

    def _query(self, im_u8, y, targeted, at):
        with torch.no_grad():
            cam = self.capture(torch.from_numpy(np.ascontiguousarray(im_u8.transpose(2, 0, 1))))
            raw = self.classifier(cam, self.crop_sz)[0]
        logits = raw.detach().double().cpu().numpy().reshape(-1)
        if not 0 <= y < len(logits):
            raise ValueError(f'target_idx {y} out of range for {len(logits)} classes')
        self.logits[at] = logits
        return cam, score_row(logits, y, targeted)

    def step(self):
        h = self._side()
        for b in range(self.B):
            self.state[b, 0] = 0
            if self.state[b, 2]:                     # resting: nothing is captured
                self.prop[b] = 0
                continue
            y, targeted = self.labels[b], self.flags[b]
            cams = []
            for k in range(self.K if h else 1):      # (iteration 0: one capture of the stripes)
                im = self.x_u8[b]
                self.prop[b, k] = 0
                if h:
                    p = proposal(self.seed, self.t, self.b_off + b, k, h, self.c0, self.eps8, self.Hp, self.Wp)
                    self.prop[b, k] = p
                    im = im.copy()
                    im[p[0]:p[0] + h, p[1]:p[1] + h] = p[3:6]
                cam, self.rows[b, k, :3] = self._query(im, y, targeted, (b, k))
                cams.append(cam)
            if not h:
                self.rows[b, 1:] = self.rows[b, 0]
            ks, acc = choose(self.rows[b, :len(cams), 0], self.best_loss[b])
            if acc:
                p = self.prop[b, ks]
                if h:
                    self.x_u8[b, p[0]:p[0] + h, p[1]:p[1] + h] = p[3:6]
                self.best_loss[b] = self.rows[b, ks, 0]
                self.cam_best[b] = cams[ks]
                self.state[b, 2] = succeeds(int(self.rows[b, ks, 1]), self.rows[b, ks, 2], y, targeted, self.p_thresh)
            self.state[b, 0], self.state[b, 1] = acc, max(ks, 0)
            self.state[b, 3] += len(cams)
        self.h, self.t = h, self.t + 1

    def done(self):
        return self.state[:, 2].astype(bool)

    def results(self):
        if any(c is None for c in self.cam_best):
            raise RuntimeError('no candidate was accepted for some sample (iteration 0 gave a loss that is not finite)')
        info = dict(success=self.done(), queries=self.state[:, 3].copy(), best_loss=self.best_loss.copy(), iterations=self.t - 1)
        return torch.from_numpy(self.x_u8.transpose(0, 3, 1, 2).copy()), torch.stack([c.detach().float().cpu() for c in self.cam_best]), info


class FastSquareState(_SquareState):
    """The fast route; every tensor lives on the classifier's device.  x_u8 int32 [B, Hp, Wp] (packed), prop int32 [B, K, 8], rows
    float32 [B K, 4], best_loss float32 [B], state int32 [B, 4], cam_best float32 [B, Hc, Wc, 4] (PCNet's output, before the 8-bit step)."""

    def __init__(self, cap, clf, crop_sz, *args):
        from .models import to_nhwc4
        super().__init__(*args)
        self.dev = clf.device
        if self.dev.type != 'cuda':
            raise RuntimeError('spaa_amd.Classifier runs on the GPU only (no CPU fallback); got device=%s' % self.dev)

        def index(d):     # ('cuda' is the current device)
            return d.index if d.index is not None else torch.cuda.current_device()
        if cap.device.type != self.dev.type or index(cap.device) != index(self.dev):
            raise RuntimeError(f'the PCNet ({cap.device}) and the classifier ({self.dev}) must be on one device')
        B, K, P = self.B, self.K, self.B * self.K
        self.quantize = cap.quantize
        with _lib.on_device(self.dev):
            self.pe = cap.pcnet.engine(P, (self.Hp, self.Wp), owner=self, storage='f32')
            self.pe.set_scene(to_nhwc4(cap.cam_scene).expand(P, -1, -1, -1).contiguous())
            self.eng = clf.engine(P, (self.pe.Hc, self.pe.Wc), tuple(crop_sz), owner=self)
            if any(not 0 <= v < self.eng.ncls for v in self.labels):
                raise ValueError(f'target_idx {self.labels} out of range for {self.eng.ncls} classes')
            kw = dict(dtype=torch.int32, device=self.dev)
            self.x_u8 = torch.zeros(B, self.Hp, self.Wp, **kw)
            self.prop, self.state = torch.zeros(B, K, 8, **kw), torch.zeros(B, 4, **kw)
            self.label, self.targeted = torch.tensor(self.labels, **kw), torch.tensor([int(f) for f in self.flags], **kw)
            self.rows = torch.zeros(P, 4, device=self.dev)
            self.best_loss = torch.full((B,), float('inf'), device=self.dev)
            self.cam_best = torch.zeros(B, self.pe.Hc, self.pe.Wc, 4, device=self.dev)
            _lib.call('spaa_square_init', self.seed, self.b_off, self.c0, self.eps8, _lib.ptr(self.x_u8), B, self.Hp, self.Wp)

    def step(self):
        h = self._side()
        pe, eng, B, K = self.pe, self.eng, self.B, self.K
        with _lib.on_device(self.dev):
            _lib.call('spaa_square_propose', self.seed, self.t, self.b_off, h, self.c0, self.eps8, _lib.ptr(self.state), _lib.ptr(self.prop),
                      B, K, self.Hp, self.Wp)
            _lib.call('spaa_square_warp', _lib.ptr(self.x_u8), _lib.ptr(self.prop), B, K, _lib.ptr(pe.tap_src), _lib.ptr(pe.tap_wm),
                      _lib.ptr(pe.scene), _lib.ptr(pe.a['xw']), _lib.ptr(pe.a['cat8']) if pe.needs_cat8 else None, self.Hp, self.Wp, pe.Hc,
                      pe.Wc)
            y = pe.forward_from_xw()
            _lib.call('spaa_capture_preproc', _lib.ptr(y), _lib.ptr(eng.pre), B * K, pe.Hc, pe.Wc, eng.cy0, eng.cx0, eng.ch, eng.cw, eng.oh,
                      eng.ow, eng._mean, eng._std, int(self.quantize))
            self.logits = eng.forward_pre()
            _lib.call('spaa_square_score', _lib.ptr(self.logits), eng.ncls, _lib.ptr(self.label), _lib.ptr(self.targeted), self.p_thresh,
                      K if h else 1, _lib.ptr(self.rows), _lib.ptr(self.best_loss), _lib.ptr(self.state), B, K)
            _lib.call('spaa_square_commit', _lib.ptr(self.state), _lib.ptr(self.prop), _lib.ptr(y), _lib.ptr(self.x_u8),
                      _lib.ptr(self.cam_best), B, K, self.Hp, self.Wp, pe.Hc, pe.Wc)
        self.h, self.t = h, self.t + 1

    def done(self):
        return self.state[:, 2].cpu().numpy().astype(bool)

    def results(self):
        from .models import to_nchw
        from .one_pixel_attacker import SimulatedCapture
        state, best = self.state.cpu().numpy(), self.best_loss.cpu().numpy()
        if not np.isfinite(best).all():
            raise RuntimeError('no candidate was accepted for some sample (iteration 0 gave a loss that is not finite)')
        with _lib.on_device(self.dev):
            cam = to_nchw(self.cam_best)
            if self.quantize:      # the camera's 8-bit step, as SimulatedCapture applies it
                cam = SimulatedCapture._over255((cam * 255).type(torch.uint8))
            prj = unpack_u8(self.x_u8)
        info = dict(success=state[:, 2].astype(bool), queries=state[:, 3].astype(np.int64), best_loss=best.astype(np.float64),
                    iterations=self.t - 1)
        return prj, cam, info


class ProjectorSquareAttacker:
    """The Square Attack with a projector and a camera in the loop.  `cfg`: the setup info (`prj_im_sz`, `prj_brightness`, `cam_im_sz`,
    `classifier_crop_sz` are read; the hardware fields are accepted and ignored); `capture`: a SimulatedCapture or any callable
    capture(im_prj uint8 [3,Hp,Wp]) -> im_cam float [3,Hc,Wc] in [0, 1], as for ProjectorOnePixelAttacker."""

    def __init__(self, class_names, cfg, *, capture):
        if not callable(capture):
            raise TypeError('capture must be a SimulatedCapture or a callable im_prj uint8 [3,Hp,Wp] -> im_cam float [3,Hc,Wc]')
        self.prj_im_sz, self.prj_brightness = tuple(cfg['prj_im_sz']), cfg['prj_brightness']
        self.cam_im_sz = tuple(cfg['cam_im_sz'])
        self.classifier_crop_sz = tuple(cfg['classifier_crop_sz'])
        self.capture, self.class_names = capture, class_names

    def state(self, classifier, target_idx, targeted, *, eps8, n_iters, p_init=0.05, proposals=1, p_thresh=0.9, seed=0, check_every=10,
              b_off=0):
        """The attack's state before iteration 0 (`step()` runs one iteration): a FastSquareState or a ForeignSquareState."""
        from .classifier import Classifier
        from .one_pixel_attacker import SimulatedCapture
        if not callable(classifier):
            raise TypeError('classifier must be a spaa_amd.Classifier or a callable (im_cam, crop_sz) -> (raw scores, p, idx)')
        labels, flags = _checked(len(self.class_names), target_idx, targeted, eps8, n_iters, p_init, proposals, p_thresh, seed, check_every,
                                 b_off, self.prj_im_sz)
        args = (labels, flags, self.prj_im_sz, centre(self.prj_brightness), eps8, n_iters, p_init, proposals, p_thresh, seed, b_off)
        if isinstance(self.capture, SimulatedCapture) and isinstance(classifier, Classifier) and not classifier.sort_results:
            return FastSquareState(self.capture, classifier, self.classifier_crop_sz, *args)
        return ForeignSquareState(self.capture, classifier, self.classifier_crop_sz, *args)

    def attack(self, classifier, target_idx, targeted, *, eps8, n_iters, p_init=0.05, proposals=1, p_thresh=0.9, seed=0, check_every=10,
               b_off=0, trace=None):
        """Attacks len(target_idx) samples of the one scene at once, as spaa() does: `target_idx` the target classes (targeted) or the true
        class (untargeted), `targeted` one flag or one per sample.  Returns (prj_adv uint8 [B,3,Hp,Wp], cam_adv float [B,3,Hc,Wc], info)
        with per-sample `success`, `queries` (captures spent) and `best_loss` in `info`, and the iterations run.
        `eps8` (1..127): the L-infinity budget in 8-bit projector levels.  It has no default: nobody has measured which budget a real
        projector-camera pair needs for the attack to work or to go unnoticed, so the caller has to choose.
        `n_iters`: iterations after the stripes; `p_init`: the first squares' share of the image; `proposals`: squares tried per sample and
        iteration (1..8); `seed`, `b_off`: sample row r draws the words of sample b_off + r, so a batch split in two draws the same numbers;
        `check_every`: how often the loop looks whether every sample rests; `trace`: a list that receives
        (t, h, prop, rows, state, best_loss) as host arrays after every iteration."""
        st = self.state(classifier, target_idx, targeted, eps8=eps8, n_iters=n_iters, p_init=p_init, proposals=proposals, p_thresh=p_thresh,
                        seed=seed, check_every=check_every, b_off=b_off)
        for t in range(n_iters + 1):
            st.step()
            if trace is not None:
                trace.append(tuple([t, st.h] + [np.array(v.cpu() if isinstance(v, torch.Tensor) else v)
                                                for v in (st.prop, st.rows, st.state, st.best_loss)]))
            if t % check_every == 0 and t < n_iters and st.done().all():
                break
        self.last_state = st
        return st.results()

    __call__ = attack
