"""CPU: the transferable attack's host side -- the three new entry points are declared and exported, Transfer's value check and taps,
the refusals of spaa() / spaa_sweep() and of the attack states (raised before anything touches a GPU), and the float64 restatement
(tests/transfer_oracle.py) on its own: the filter is self-adjoint, an impulse in a corner gives the truncated outer product of the
taps, and a constant gradient gives the geometric series of the momentum."""
import math
import os
import re

import numpy as np
import pytest
import torch

import transfer_oracle as to
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_transfer_tiles', 'spaa_transfer_blur', 'spaa_transfer_momentum')


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS
    assert 'spaa_transfer_blur' in _lib._SIGNATURES and 'spaa_transfer_momentum' in _lib._SIGNATURES
    assert re.search(r'#define\s+SPAA_TRANSFER_RMAX\s+7\b', hdr) and A.TRANSFER_RMAX == 7
    assert 'transfer_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert spaa_amd.Transfer is A.Transfer
    assert spaa_amd.transfer_success is A.transfer_success
    # the host-side query needs no GPU: 16 x 32 pixel tiles, 0 for what the blur refuses
    assert [lib.spaa_transfer_tiles(h, w) for h, w in ((3, 3), (16, 32), (17, 33), (64, 64), (256, 256))] == [1, 1, 4, 8, 128]
    assert lib.spaa_transfer_tiles(0, 5) == 0 and lib.spaa_transfer_tiles(5, -1) == 0


def test_transfer_is_a_checked_immutable_value():
    t = A.Transfer()
    assert (t.momentum, t.sigma, t.radius) == (1.0, 0.0, 0) and t == A.Transfer(1, 0) and hash(t) == hash(A.Transfer(1.0, 0.0))
    with pytest.raises(AttributeError):
        t.sigma = 1.0
    for bad in (dict(momentum=-1e-6), dict(momentum=1.0001), dict(sigma=-0.1), dict(sigma=2.34), dict(sigma=float('inf')),
                dict(momentum=float('nan')), dict(sigma='1'), dict(momentum=None), dict(momentum=True), dict(momentum=0, sigma=0),
                dict(momentum=0.0)):
        with pytest.raises(ValueError):
            A.Transfer(**bad)
    assert torch.equal(t.weights(), torch.ones(1)) and t.weights().dtype == torch.float32
    for sigma in (0.1, 1 / 3, 0.34, 1.0, 1.5, 2.0, 7 / 3):
        tr = A.Transfer(0.5, sigma)
        r = tr.radius
        assert r == math.ceil(3 * sigma) and 1 <= r <= A.TRANSFER_RMAX
        w = tr.weights()
        assert w.dtype == torch.float32 and w.shape == (2 * r + 1,)
        assert torch.equal(w, w.flip(0)) and (w > 0).all() and w.argmax() == r           # symmetric, positive, peaked in the middle
        assert abs(float(w.double().sum()) - 1.0) <= (2 * r + 1) * 2.0 ** -25            # (each tap rounds by half an ulp at most)
        i = np.arange(-r, r + 1, dtype=np.float64)
        e = np.exp(-i * i / (2 * sigma * sigma))
        assert np.abs(w.double().numpy() - e / e.sum()).max() <= 2.0 ** -24 * (e / e.sum()).max()   # (float64 taps, rounded once)
    assert A.Transfer(0, 0.5).radius == 2 and A.Transfer(1, 7 / 3).radius == 7


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


def test_transfer_refusals(parts):
    """From spaa() and spaa_sweep() with device='cuda' and no GPU in reach: nothing was leased or launched."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    tr = A.Transfer(1.0, 1.0)

    def run(pcnet, classifier, sc=scene, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, sc, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(pcnet, classifier, sc=scene, **kw):
        return A.spaa_sweep(pcnet, classifier, None, sc, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='f16'):
            call(pcs[0], clfs[0], transfer=tr, storage='f16')
        with pytest.raises(TypeError):
            call(pcs[0], lambda im, cp: None, transfer=tr)
        for bad in (1.0, dict(momentum=1.0), 'on', True, (1.0, 1.5)):
            with pytest.raises(TypeError, match='Transfer'):
                call(pcs[0], clfs[0], transfer=bad)
        # the earlier checks keep their precedence
        with pytest.raises(NotImplementedError, match='ensemble'):
            call(pcs[0], [clfs[0], clfs[1]], transfer=tr, storage='f16')
        with pytest.raises(NotImplementedError, match='views'):
            call([pcs[0], pcs[1]], clfs[0], [scene, scene], transfer=tr, storage='f16')
        with pytest.raises(NotImplementedError, match='jitter'):
            call(pcs[0], clfs[0], transfer=tr, jitter=A.CaptureJitter(), storage='f16')
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)   # no engine was built on the way
    # the states themselves
    with pytest.raises(NotImplementedError, match='f16.*transfer'):
        A.AttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', storage='f16', transfer=tr)
    with pytest.raises(TypeError, match='Transfer'):
        A.AttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', transfer=0.5)
    with pytest.raises(TypeError, match='Transfer'):
        A.EnsembleAttackState(pcs[0], clfs, [1], scene, 'caml2', setup, 'cuda', transfer=0.5)
    with pytest.raises(TypeError, match='Transfer'):
        A.MultiViewAttackState(pcs, clfs[0], [1], [scene, scene], 'caml2', setup, 'cuda', transfer=0.5)
    with pytest.raises(TypeError, match='Transfer'):
        A.JitterAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', A.CaptureJitter(), transfer=0.5)
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)


def test_cpu_device_raises_the_no_fallback_error(parts):
    """transfer=None is the plain call, which on a CPU device raises what the plain call raises; so does a transferable attack (and not
    a TypeError about the keyword)."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    for kw in (dict(transfer=None), dict(transfer=A.Transfer()), dict(transfer=A.Transfer(0.5, 1.5))):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2', 'cpu', setup, **kw)
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa_sweep(pcs[0], clfs[0], None, scene, setup, 'cpu', [('caml2', 5, True, [1, 2])], **kw)
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs, None, [1], True, scene, 5, 'caml2', 'cpu', setup, **kw)
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs, clfs[0], None, [1], True, [scene, scene], 5, 'caml2', 'cpu', setup, **kw)
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2', 'cpu', setup, jitter=A.CaptureJitter(), **kw)
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)


# ---- the oracle on its own

@pytest.mark.parametrize('sigma', [0.0, 1 / 3, 1.0, 7 / 3])
def test_the_filter_is_self_adjoint(sigma):
    """<K u, v> = <u, K v>: symmetric taps and zero padding."""
    w = to.taps64(A.Transfer(1.0, sigma))
    gen = torch.Generator().manual_seed(int(sigma * 100))
    u = torch.randn(2, 9, 13, 4, generator=gen, dtype=torch.float64)
    v = torch.randn(2, 9, 13, 4, generator=gen, dtype=torch.float64)
    a = (to.blur(u, w)[..., :3] * v[..., :3]).sum()
    b = (u[..., :3] * to.blur(v, w)[..., :3]).sum()
    assert abs(a - b) <= 1e-12 * (u[..., :3].abs().sum() * v[..., :3].abs().max())
    assert (to.blur(u, w)[..., 3] == 0).all()                                            # the pad channel neither enters nor leaves


@pytest.mark.parametrize('hw', [(3, 3), (5, 7), (20, 24)])
@pytest.mark.parametrize('sigma', [0.0, 1.0, 7 / 3])
def test_corner_impulse_gives_the_truncated_outer_product(hw, sigma):
    w = to.taps64(A.Transfer(1.0, sigma))
    r = (w.numel() - 1) // 2
    H, W = hw
    g = torch.zeros(1, H, W, 4, dtype=torch.float64)
    g[0, 0, W - 1, :3] = torch.tensor([2.0, -1.0, 0.5])
    g[0, :, :, 3] = 7.0                                                                  # (garbage in the pad channel)
    t = to.blur(g, w)[0]
    wy = w[r:r + H]                                                                      # rows 0 .. H - 1 see taps r, r + 1, ...
    wx = w[:r + 1].flip(0)[:W].flip(0)                                                   # columns ... W - 1 see taps ..., r - 1, r
    want = torch.zeros(H, W, dtype=torch.float64)
    want[:wy.numel(), W - wx.numel():] = torch.outer(wy, wx)
    for c, a in enumerate((2.0, -1.0, 0.5)):
        assert (t[..., c] - a * want).abs().max() <= 1e-15
    assert (t[..., 3] == 0).all()


@pytest.mark.parametrize('mu', [0.0, 0.5, 1.0])
def test_constant_gradient_gives_the_geometric_series(mu):
    """The same g in every iteration: m_n = (1 + mu + ... + mu^(n - 1)) t / |t|_1, and the step direction is t / ||t||_2 throughout."""
    tr = A.Transfer(mu, 1.0)
    w = to.taps64(tr)
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(2, 6, 5, 4, generator=gen, dtype=torch.float64)
    col = torch.tensor([False, False])
    x0 = torch.full((2, 6, 5, 4), 0.5, dtype=torch.float64)
    t = to.blur(g, w)
    unit = t / t[..., :3].abs().sum(dim=(1, 2, 3))[:, None, None, None]
    n = 12
    for i, (m, x, E_m, E_x) in enumerate(to.recurrence([g] * n, [col] * n, x0, w, mu, 2.0, 1.0, 16), start=1):
        series = float(i) if mu == 1.0 else (1 - mu ** i) / (1 - mu)
        assert (m - series * unit).abs().max() <= 1e-13 * series * unit.abs().max()
        d = t / t[..., :3].pow(2).sum(dim=(1, 2, 3)).sqrt()[:, None, None, None]
        assert (x - (x0 - 2.0 * i * d)).abs().max() <= 1e-12
        assert (E_m >= 0).all() and (E_x[..., :3] > 0).all()
    # a sample on the colour step keeps its gradient and its momentum, and steps along its own gradient
    col = torch.tensor([False, True])
    m0 = torch.randn(2, 6, 5, 4, generator=gen, dtype=torch.float64)
    s = to.step(g, m0, col, w, mu)
    assert torch.equal(s['m'][1], m0[1]) and torch.equal(s['g'][1], g[1]) and (s['e_m'][1] == 0).all()
    assert torch.equal(s['g'][0], s['m'][0]) and (s['m'][0, ..., 3] == 0).all()
    # an all-zero gradient: n1 = 0 and the momentum only decays
    s = to.step(torch.zeros_like(g), m0, torch.tensor([False, False]), w, mu)
    assert (s['n1'] == 0).all() and torch.equal(s['m'][..., :3], mu * m0[..., :3])
