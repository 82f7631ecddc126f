"""CPU: the capture-jitter attack's host side -- the three new entry points are declared and exported, CaptureJitter's value checks,
the refusals of spaa() / spaa_sweep() (raised before anything touches a GPU), and the float64 / integer restatement
(tests/jitter_oracle.py) on its own: identity, adjointness, a central-difference check and the generator's statistics."""
import os
import re

import numpy as np
import pytest
import torch

import jitter_oracle as jo
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_jitter_draw', 'spaa_jitter_fwd', 'spaa_jitter_bwd')


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert re.search(r'#define\s+SPAA_JITTER_MAX\s+4\b', hdr) and A.JITTER_MAX == 4 == A.ENS_MAX
    assert 'jitter_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert spaa_amd.CaptureJitter is A.CaptureJitter and spaa_amd.JitterAttackState is A.JitterAttackState
    assert spaa_amd.capture_survival is A.capture_survival
    assert issubclass(A.JitterAttackState, A.EnsembleAttackState)


def test_capture_jitter_is_a_checked_immutable_value():
    j = A.CaptureJitter()
    assert (j.gain, j.offset, j.shift, j.noise, j.quantize, j.draws, j.seed) == (0.1, 0.03, 0.75, 0.01, True, 3, 0)
    assert j == A.CaptureJitter(0.1, 0.03, 0.75, 0.01, True, 3, 0) and hash(j) == hash(A.CaptureJitter())
    with pytest.raises(AttributeError):
        j.gain = 0.2
    for kw in (dict(draws=1), dict(draws=5), dict(gain=-0.1), dict(offset=-1e-3), dict(shift=-0.5), dict(noise=-0.01), dict(gain=1.0),
               dict(gain=1.5), dict(shift=2.01), dict(noise=0.11)):
        with pytest.raises(ValueError):
            A.CaptureJitter(**kw)
    for kw in (dict(draws=2), dict(draws=4), dict(gain=0.0, offset=0.0, shift=0.0, noise=0.0), dict(shift=2.0), dict(noise=0.1),
               dict(gain=0.99), dict(quantize=False, seed=7)):
        A.CaptureJitter(**kw)


@pytest.fixture(scope='module')
def parts():
    sd = syn.pcnet_state_dict(0, cam_sz=(64, 64))
    pcs = []
    for _ in range(2):
        pc = PCNet(sd['mask'], WarpingNet(out_size=(64, 64)))
        pc.load_state_dict(sd)
        pcs.append(pc)
    csd = syn.resnet18_state_dict(2)
    clfs = [Classifier('resnet18', 'cpu', state_dict=csd, input_sz=(56, 56)) for _ in range(2)]
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=(64, 64))
    return pcs, clfs, setup


def test_jitter_refusals(parts):
    """NotImplementedError for jitter with a list of classifiers, a list of PCNets or fp16 storage, TypeError for a foreign callable,
    ValueError for focus=True -- from spaa() and spaa_sweep() with device='cuda' and no GPU in reach: nothing was leased or launched."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    jt = A.CaptureJitter()

    def run(pcnet, classifier, sc=scene, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, sc, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(pcnet, classifier, sc=scene, **kw):
        return A.spaa_sweep(pcnet, classifier, None, sc, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='ensemble'):
            call(pcs[0], [clfs[0], clfs[1]], jitter=jt)
        with pytest.raises(NotImplementedError, match='views'):
            call([pcs[0], pcs[1]], clfs[0], [scene, scene], jitter=jt)
        with pytest.raises(NotImplementedError, match='f16'):
            call(pcs[0], clfs[0], jitter=jt, storage='f16')
        with pytest.raises(TypeError):
            call(pcs[0], lambda im, cp: None, jitter=jt)
        with pytest.raises(ValueError, match='focus'):
            call(pcs[0], clfs[0], jitter=jt, focus=True)
        with pytest.raises(TypeError, match='CaptureJitter'):
            call(pcs[0], clfs[0], jitter=dict(gain=0.1))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)   # no engine was built on the way
    with pytest.raises(NotImplementedError):
        A.JitterAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', jt, storage='f16')
    # jitter=None is the plain call, which on a CPU device raises what the plain call raises; so does a jitter attack
    for kw in (dict(jitter=None), dict(jitter=jt)):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2', 'cpu', setup, **kw)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.spaa_sweep(pcs[0], clfs[0], None, scene, setup, 'cpu', [('caml2', 5, True, [1, 2])], jitter=None)
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)


def _rows(rng, n, max_shift=2.0):
    """n planted table rows with shifts up to +-max_shift, among them the exact ends and integers."""
    rows = np.zeros((n, 8))
    rows[:, :3] = rng.uniform(0.8, 1.2, (n, 3))
    rows[:, 3] = rng.uniform(-0.05, 0.05, n)
    rows[:, 4:6] = rng.uniform(-max_shift, max_shift, (n, 2))
    special = [(2.0, -2.0), (-2.0, 2.0), (1.0, -1.0), (0.0, 0.0), (-0.5, 1.5)]
    for i, s in enumerate(special[:n]):
        rows[i, 4:6] = s
    return rows


def test_identity_row_leaves_the_image_unchanged():
    rng = np.random.default_rng(0)
    y = rng.uniform(0, 1, (2, 5, 7, 4))
    jit = np.tile(np.array(jo.IDENTITY_ROW), (2, 2, 1))
    out, gate, pre = jo.forward(y, jit, np.zeros((2, 2), dtype=np.uint32), False)
    assert np.array_equal(out[0, ..., :3], y[..., :3]) and np.array_equal(out[1], out[0]) and (out[..., 3] == 0).all()
    assert (gate == 7).all()
    # the same through the autograd form, whose gradient of sum(out) is then all ones
    yt = torch.from_numpy(np.ascontiguousarray(y[..., :3].transpose(0, 3, 1, 2))).requires_grad_(True)
    ot = jo.transform_torch(yt, jit[:, 0], np.zeros(2, dtype=np.uint32), True)
    assert torch.equal(ot.detach(), torch.floor(yt.detach() * 255.0) / 255.0)
    assert torch.equal(torch.autograd.grad(ot.sum(), yt)[0], torch.ones_like(yt))
    assert np.array_equal(jo.shift(y[0], 0.0, 0.0), y[0]) and np.array_equal(jo.shift_T(y[0], 0.0, 0.0), y[0])


@pytest.mark.parametrize('hw', [(5, 7), (17, 19)])
def test_adjoint_identity(hw):
    """<J u, v> = <u, J^T v> for the linear part J = gate . gain . S, to 1e-10 relative, shifts up to +-2."""
    H, W = hw
    rng = np.random.default_rng(1)
    B, J = 4, 4
    jit = _rows(rng, B * J).reshape(B, J, 8)
    u = rng.normal(size=(B, H, W, 3))
    v = rng.normal(size=(J, B, H, W, 3))
    gate = rng.integers(0, 8, (J, B, H, W)).astype(np.uint8)
    bits = np.stack([(gate >> c) & 1 for c in range(3)], axis=-1)
    worst = 0.0
    for b in range(B):
        for j in range(J):
            row = jit[b, j]
            Ju = bits[j, b] * row[:3] * jo.shift(u[b], row[jo.DX], row[jo.DY])
            lhs = (Ju * v[j, b]).sum()
            rhs = (u[b] * jo.backward(v, jit, gate)[j, b, ..., :3]).sum()
            scale = np.abs(Ju * v[j, b]).sum()
            worst = max(worst, abs(lhs - rhs) / scale)
    print(f'{hw}: worst |<Ju,v> - <u,JTv>| / sum|Ju v| = {worst:.3e}')
    assert worst <= 1e-10


def test_adjoint_against_central_differences():
    """backward() is the gradient of sum(v * forward(y)) where no value sits on the clamp: central differences at 6 x 5."""
    H, W = 6, 5
    rng = np.random.default_rng(2)
    B, J = 2, 3
    jit = _rows(rng, B * J).reshape(B, J, 8)
    jit[..., 3] = rng.uniform(-0.3, 0.3, (B, J))                 # offsets large enough that some values are clamped
    key = np.zeros((B, J), dtype=np.uint32)
    y = rng.uniform(0, 1, (B, H, W, 3))
    v = rng.normal(size=(J, B, H, W, 3))
    out, gate, pre = jo.forward(y, jit, key, False)
    assert (gate != 7).any() and np.minimum(np.abs(pre), np.abs(pre - 1)).min() > 1e-4
    g = jo.backward(v, jit, gate)[..., :3].sum(axis=0)           # d/dy of sum_j <v_j, out_j>
    # (piecewise linear: the difference quotient is exact but for the rounding of the two sums, ~1e-16 * 30 / eps = 3e-10 at eps 1e-5)
    eps, worst = 1e-5, 0.0
    for idx in np.ndindex(B, H, W, 3):
        yp, ym = y.copy(), y.copy()
        yp[idx] += eps
        ym[idx] -= eps
        fd = ((jo.forward(yp, jit, key, False)[0][..., :3] - jo.forward(ym, jit, key, False)[0][..., :3]) * v).sum() / (2 * eps)
        worst = max(worst, abs(fd - g[idx]))
    print(f'central differences: worst |fd - adjoint| = {worst:.3e} at max |g| = {np.abs(g).max():.3f}')
    assert worst <= 1e-8 * max(1.0, np.abs(g).max())


def test_noise_statistics():
    """3 * 2^16 normals of one key: mean, variance and the lag-1 correlations across neighbouring pixels and across channels; each bar
    is at least six standard errors at that count (1 / sqrt(N) = 2.3e-3, sqrt(2 / N) = 3.2e-3)."""
    n = jo.normals(jo.draw_word(0, 0, 0, 1, jo.KEY), 1 << 16)
    assert n.shape == (1 << 16, 3) and np.isfinite(n).all()
    mean, var = n.mean(), n.var()
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])   # noqa: E731
    c_pix = corr(n[:-1], n[1:])
    c_ch = max(abs(corr(n[:, 0], n[:, 1])), abs(corr(n[:, 1], n[:, 2])))
    print(f'normals: mean {mean:.4f}, var {var:.4f}, lag-1 pixel corr {c_pix:.4f}, channel corr {c_ch:.4f}, max |n| {np.abs(n).max():.3f}')
    assert abs(mean) < 0.015 and abs(var - 1) < 0.02 and abs(c_pix) < 0.015 and c_ch < 0.015
    other = jo.normals(jo.draw_word(0, 0, 0, 2, jo.KEY), 1 << 16)
    assert abs(corr(n, other)) < 0.015                            # another key: another field


def test_uniforms_of_distinct_indices_are_distinct():
    us = {jo.uniform(jo.draw_word(0, t, b, j, i)) for t in range(4) for b in range(8) for j in range(4) for i in range(8)}
    assert len(us) == 4 * 8 * 4 * 8 and all(0 <= u < 1 for u in us)
    assert jo.mix32(0) == 0 and jo.mix32(1) == int(jo.mix32(np.array([1], dtype=np.uint64))[0])   # (int and array forms agree)
    assert jo.draw_word(1, 0, 0, 0, 0) != jo.draw_word(0, 0, 0, 0, 0)


def test_draw_tables_follow_the_rule():
    jit, key = jo.draw_tables(3, 5, 6, 4, 0.1, 0.03, 0.75, 0.01, clean0=True)
    assert (jit[:, 0] == np.array(jo.IDENTITY_ROW)).all() and (jit[:, 1:, 6] == np.float32(0.01)).all() and (jit[..., 7] == 0).all()
    assert (np.abs(jit[:, 1:, :3] - 1) <= np.float32(0.1)).all() and (np.abs(jit[:, 1:, 3]) <= np.float32(0.03)).all()
    assert (np.abs(jit[:, 1:, 4:6]) <= 0.75).all() and len(set(key.ravel().tolist())) == key.size
    dirty, key2 = jo.draw_tables(3, 5, 6, 4, 0.1, 0.03, 0.75, 0.01, clean0=False)
    assert np.array_equal(dirty[:, 1:], jit[:, 1:]) and np.array_equal(key, key2) and (dirty[:, 0, :3] != 1).all()
    assert not np.array_equal(jo.draw_tables(3, 6, 6, 4, 0.1, 0.03, 0.75, 0.01, True)[0], jit)
