"""The One-pixel DE attacker of the SPAA comparison (reference: one_pixel_attacker/__init__.py:18-108, Su et al.'s attack as
adapted by Nichols & Jasper), digital variant, behind the reference's signatures.

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


class _FastEvaluator:
    """The fast route's batched objective: params [S, N] -> float32 energies [S], memoised by the truncated integer vector."""

    def __init__(self, clf, im, crop_sz, pixel_count, pixel_size, target_idx, targeted, max_batch, trace):
        self.dev = clf.device
        if self.dev.type != 'cuda':
            raise RuntimeError('spaa_amd.Classifier runs on the GPU only (no CPU fallback); got device=%s' % self.dev)
        _, self.H, self.W = im.shape
        self.npix, self.pixel_size = pixel_count, pixel_size
        self.target, self.targeted = int(target_idx), bool(targeted)
        self.trace, self.memo, self.classified = trace, {}, 0
        q = im.clone() if im.dtype == torch.uint8 else (im * 255).type(torch.uint8)   # perturb_image's quantisation, once
        base = torch.zeros(1, self.H, self.W, 4)
        base[0, :, :, :3] = (q.cpu().type(torch.float32) / 255).permute(1, 2, 0)      # classify()'s u8 -> float (true division)
        self.k = max_batch
        self.sizes = sorted({min(max_batch, SMALL_BATCH), max_batch})
        with _lib.on_device(self.dev):
            self.base = base.to(self.dev)
            self.engines = {b: clf.engine(b, (self.H, self.W), tuple(crop_sz), owner=self) for b in self.sizes}
            self.cand = torch.zeros(max_batch, 5 * pixel_count, dtype=torch.int32, device=self.dev)
            self.res = torch.zeros(3, max_batch, dtype=torch.int32, device=self.dev)   # energy (f32 bits), argmax, max p (f32 bits)
        self.ncls = self.engines[self.sizes[0]].ncls
        if not 0 <= self.target < self.ncls:
            raise ValueError(f'target_idx {target_idx} out of range for {self.ncls} classes')

    def _run(self, rows, keys):
        S = len(rows)
        B = next(b for b in self.sizes if b >= S)
        eng = self.engines[B]
        cand = np.empty((B, 5 * self.npix), dtype=np.int32)
        cand[:S] = rows
        cand[S:] = rows[-1]                 # padding: a repeat of a valid candidate
        with _lib.on_device(self.dev):
            c = self.cand[:B]
            c.copy_(torch.from_numpy(cand))
            _lib.call('spaa_onepixel_preproc', _lib.ptr(self.base), _lib.ptr(c), B, self.npix, self.pixel_size, _lib.ptr(eng.pre),
                      self.H, self.W, eng.cy0, eng.cx0, eng.ch, eng.cw, eng.oh, eng.ow, eng._mean, eng._std)
            logits = eng.forward_pre()
            _lib.call('spaa_onepixel_score', _lib.ptr(logits), self.ncls, self.target, int(self.targeted), _lib.ptr(self.res[0]),
                      _lib.ptr(self.res[1]), _lib.ptr(self.res[2]), B)
            res = np.ascontiguousarray(self.res[:, :S].cpu().numpy())
        energy, pmax = res[0].view(np.float32), res[2].view(np.float32)
        for i, k in enumerate(keys):
            self.memo[k] = (energy[i], int(res[1, i]), pmax[i])
            if self.trace is not None:
                self.trace.append((rows[i].copy(), energy[i], int(res[1, i])))
        self.classified += S

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


class DigitalOnePixelAttacker:
    """one_pixel_attacker/__init__.py:47-108."""

    def __init__(self, class_names, classifier_crop_sz):
        self.class_names = class_names
        self.classifier_crop_sz = classifier_crop_sz
        self.last_result = None     # the DE result of the last attack (x, fun, nfev, nit, success, message, evaluated, ...)

    def perturb_and_predict(self, x, im, classifier, pixel_size):
        im_adv = perturb_image(x, im, pixel_size)
        _, p, _ = classifier(im_adv, self.classifier_crop_sz)
        return p

    def _report(self, target_idx, p_target, pred, p_max, targeted_attack, true_label):
        if targeted_attack:
            print(f'Target: {self.class_names[target_idx]:<20} ({p_target:.2f}) | '
                  f'Pred: {self.class_names[pred]:<20} ({p_max:.2f}) | '
                  f'GT: {self.class_names[true_label]:<20}')
        else:
            print(f'Untargeted | Pred: {self.class_names[pred]:<20} ({p_max:.2f}) | GT: {self.class_names[true_label]:<20}')

    def attack_success(self, x, im, target_idx, classifier, pixel_size, targeted_attack=False, verbose=False, true_label=None):
        p = self.perturb_and_predict(x, im, classifier, pixel_size)
        if verbose:
            self._report(target_idx, p[0, target_idx], p[0].argmax(), p[0].max(), targeted_attack, true_label)
        if (targeted_attack and p[0].argmax() == target_idx) or (not targeted_attack and p[0].argmax() != target_idx):
            return True

    def attack(self, im, classifier, targeted_attack=False, target_idx=None, pixel_count=1, pixel_size=1, maxiter=75, popsize=400,
               verbose=False, true_label=None, *, updating='immediate', seed=None, max_batch=None, trace=None):
        """The reference's attack (:73-105); returns (DataFrame, im_adv).  Keyword-only extras: `updating` ('immediate', the
        reference's, or 'deferred'); `seed` (None: numpy's global RandomState, as the reference; an int or a RandomState);
        `max_batch` (candidates per evaluation batch; default the population size on the fast route, 1 on the foreign one);
        `trace` (a list: receives (integer vector, energy, argmax) of every candidate evaluated, in evaluation order)."""
        from .classifier import Classifier

        d = pixel_size // 2
        _, n_rows, n_cols = im.shape
        bounds = [(d, n_rows - 1 - d), (d, n_cols - 1 - d), (0, 255), (0, 255), (0, 255)] * pixel_count
        if n_rows - 1 - d < d or n_cols - 1 - d < d:
            raise ValueError(f'pixel_size {pixel_size} leaves no valid square centre in a {n_rows}x{n_cols} image')
        popmul = max(1, popsize // len(bounds))
        fast = isinstance(classifier, Classifier) and not classifier.sort_results

        if fast:
            n_pop = max(5, popmul * len(bounds))
            ev = _FastEvaluator(classifier, im, self.classifier_crop_sz, pixel_count, pixel_size, target_idx, targeted_attack,
                                n_pop if max_batch is None else int(max_batch), trace)
            objective = ev

            def callback_fn(x, convergence):
                e, pred, p_max = ev.lookup(x)
                if verbose:
                    self._report(target_idx, np.float32(1) - e if targeted_attack else e, pred, p_max, targeted_attack, true_label)
                if (targeted_attack and pred == target_idx) or (not targeted_attack and pred != target_idx):
                    return True
        else:
            def predict_one(x):
                p = self.perturb_and_predict(x, im, classifier, pixel_size)
                e = 1 - p[0, target_idx] if targeted_attack else p[0, target_idx]
                if trace is not None:
                    trace.append((x.astype(int), e, int(p[0].argmax())))
                return e

            def objective(params):
                return np.array([predict_one(x) for x in params])

            def callback_fn(x, convergence):
                return self.attack_success(x, im, target_idx, classifier, pixel_size, targeted_attack, verbose, true_label)

        de_ret = DifferentialEvolution(objective, bounds, maxiter=maxiter, popsize=popmul, recombination=1, atol=-1,
                                       callback=callback_fn, polish=False, seed=seed, updating=updating,
                                       max_batch=(1 if max_batch is None and not fast else max_batch)).solve()
        if fast:
            de_ret['classified'] = ev.classified     # candidates that went through the classifier (memo misses)
        self.last_result = de_ret

        im_adv = perturb_image(de_ret.x, im, pixel_size).type(torch.float32) / 255
        _, p, _ = classifier(torch.stack((im, im_adv), 0), self.classifier_crop_sz)  # p and idx are sorted, not the original orders.

        true_p, pred_p = p[0].max(), p[1].max()
        true_idx, pred_idx = p[0].argmax(), p[1].argmax()
        if targeted_attack:
            success = pred_idx == target_idx
        else:
            success = pred_idx != true_idx
        cdiff = p[0, target_idx] - p[1, target_idx]
        return pd.DataFrame([[classifier.name, pixel_count, true_idx, pred_idx, success, true_p, pred_p, cdiff]],
                            columns=['classifier', 'pixel_count', 'true_idx', 'pred_idx', 'success', 'true_p', 'pred_p',
                                     'cdiff']), im_adv

    def __call__(self, im, classifier, targeted_attack=False, target_idx=None, pixel_count=1, pixel_size=1, maxiter=75, popsize=400,
                 verbose=False, true_label=None, **kw):
        return self.attack(im, classifier, targeted_attack, target_idx, pixel_count, pixel_size, maxiter, popsize, verbose,
                           true_label, **kw)
