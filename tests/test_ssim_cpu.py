"""CPU: the SSIM stealth term's host side and its float64 restatement (tests/ssim_oracle.py) on its own -- the restatement against
torch.float64 autograd of a direct torch composition and against the reference's own fp32 results (tests/golden/ssim_stealth.npz,
written by tests/golden/make_golden_ssim.py), every mutation beyond its bar, ssim_weight, the refusal of the foreign-callable route,
and the new entry points in the header and the binding's table."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_oracle as so
from spaa_amd import _lib
from spaa_amd import projector_based_attack as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_ssim_tiles', 'spaa_ssim_scene_stats', 'spaa_ssim_fwd', 'spaa_ssim_bwd', 'spaa_ssim_value')
# every kind at a size below the radius, at one window and at a ragged rectangle
CASES = [(k, h, w) for k in so.KINDS for h, w in ((1, 1), (3, 5), (11, 11), (13, 18))]


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS
    assert all(n in _lib._SIGNATURES for n in ENTRY_POINTS[1:])
    assert re.search(r'#define\s+SPAA_SSIM_TILE_H\s+%d\b' % so.TILE_H, hdr) and re.search(r'#define\s+SPAA_SSIM_TILE_W\s+%d\b' % so.TILE_W, hdr)
    assert 'ssim_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    # the host-side query needs no GPU: 16 x 32 pixel tiles, 0 for what the launches refuse
    assert [lib.spaa_ssim_tiles(h, w) for h, w in ((1, 1), (16, 32), (17, 33), (21, 70), (64, 64), (256, 256))] == [1, 1, 4, 6, 8, 128]
    assert lib.spaa_ssim_tiles(0, 5) == 0 and lib.spaa_ssim_tiles(5, -1) == 0 and lib.spaa_ssim_tiles(1 << 16, 1 << 15) == 0


def test_ssim_weight_and_the_three_reference_terms():
    assert A.ssim_weight('caml2_camssim') == 1.0 and A.ssim_weight('camssim') == 1.0 and A.ssim_weight('camdE_caml2') == 0.0
    assert A.LOSS_TERMS == ('prjl2', 'caml2', 'camdE')
    assert A.loss_weights('camdE_caml2_camssim') == A.loss_weights('camdE_caml2') == (0.0, 1.0, 1.0)
    assert A.loss_weights('camssim') == (0.0, 0.0, 0.0)
    samples, _ = A.plan_sweep([('caml2', 2, True, [1]), ('caml2_camssim', 2, True, [1, 2])])
    assert [s[1] for s in samples] == ['caml2', 'caml2_camssim', 'caml2_camssim']
    with pytest.raises(ValueError, match='unknown stealth loss'):
        A.plan_sweep([('caml2_camsim', 2, True, [1])])


def test_foreign_callable_is_refused_before_anything_is_allocated():
    def clf(im, crop):   # (never called)
        raise AssertionError('the classifier was called')
    from spaa_amd import synthetic as syn
    from spaa_amd.models import PCNet, WarpingNet
    sd = syn.pcnet_state_dict(0, cam_sz=(16, 16), mask='rect')
    pc = PCNet(sd['mask'], WarpingNet(out_size=(16, 16)))
    # (device 'cpu': the route's first own check would be the GPU's; the term is refused before it)
    with pytest.raises(NotImplementedError, match='camssim'):
        A.spaa(pc, clf, None, [1], True, torch.zeros(3, 16, 16), 5, 'caml2_camssim', 'cpu', {})
    with pytest.raises(NotImplementedError, match='camssim'):
        A._spaa_foreign_classifier(pc, clf, None, [1], True, torch.zeros(3, 16, 16), 5, 'camssim', 'cpu', {}, 3, 2, 1, 0.9, None)


def test_taps_are_the_reference_gaussian():
    from spaa_amd.metrics import ssim_taps, _window
    w = so.taps()
    assert w.dtype == np.float32 and w.shape == (11,) and np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert np.array_equal(ssim_taps().numpy(), w)
    assert torch.equal(ssim_taps().unsqueeze(1).mm(ssim_taps().unsqueeze(0)).reshape(-1), _window())   # the 2-D window's factors


def _torch_ssim(y, s):
    """SSIM_b by a direct torch composition in float64: pad, the exact outer product of the taps as a grouped convolution."""
    w = torch.from_numpy(so.taps()).double()
    win = (w[:, None] * w[None, :])[None, None].expand(3, 1, 11, 11).contiguous()

    def f(x):
        return F.conv2d(F.pad(x, (5, 5, 5, 5), mode='replicate'), win, groups=3)

    mu1, mu2 = f(y), f(s)
    v1, v2, cov = f(y * y) - mu1 * mu1, f(s * s) - mu2 * mu2, f(y * s) - mu1 * mu2
    return (((2 * mu1 * mu2 + so.C1) * (2 * cov + so.C2)) / ((mu1 * mu1 + mu2 * mu2 + so.C1) * (v1 + v2 + so.C2))).mean()


@pytest.mark.parametrize('kind,H,W', CASES)
def test_restatement_against_float64_autograd(kind, H, W):
    y, s = so.inputs(kind, H, W)
    yt = torch.from_numpy(y[..., :3].astype(np.float64)).permute(2, 0, 1)[None].requires_grad_(True)
    st = torch.from_numpy(s[..., :3].astype(np.float64)).permute(2, 0, 1)[None]
    val = _torch_ssim(yt, st)
    g, = torch.autograd.grad(1 - val, yt)
    g = g[0].permute(1, 2, 0).numpy()
    # two float64 evaluations of the plain formulas through a 121-tap convolution and autograd: the walk of the reference's arithmetic
    # (so.REF) is linear in the unit roundoff to first order, so its fp32 bars times 2^-53 / 2^-24 bound each of the two evaluations
    # (the variance cancels in float64 as it does in fp32, only 2^29 times lower: a flat bright pair reaches 1e-12)
    bar, k = so.bars(y, s, so.REF), 2 * 2.0 ** -29
    assert abs(float(val.detach()) - so.ssim(y, s)) <= k * bar['value']
    assert (np.abs(g - so.grad(y, s)) <= k * bar['grad_sum'] / (3 * H * W)).all()
    assert np.allclose(so.grad_sum(y, s), so.grad(y, s) * 3 * H * W, rtol=1e-14, atol=0)


def test_restatement_against_the_reference_fixture(golden_dir):
    d = np.load(os.path.join(golden_dir, 'ssim_stealth.npz'))
    assert len(d['cases']) >= 4
    for i, case in enumerate(d['cases']):
        y, s = d[f'y{i}'], d[f's{i}']
        n = 3 * y.shape[0] * y.shape[1]
        bar = so.bars(y, s, so.REF)
        ev = abs(float(d[f'ssim{i}'].reshape(-1)[0]) - so.ssim(y, s))
        eg = np.abs(d[f'grad{i}'] - so.grad(y, s))
        # (the fixture's own storage as fp32: half an ulp)
        assert ev <= bar['value'] + so.U, f'{case}: SSIM differs from the reference by {ev:.3e}, bar {bar["value"]:.3e}'
        over = eg / (bar['grad_sum'] / n + so.U * np.abs(so.grad(y, s)))
        assert over.max() <= 1, f'{case}: the gradient differs from the reference by {over.max():.3f} of its bar'


@pytest.mark.parametrize('name', sorted(so.MUTATIONS))
def test_every_mutation_lands_beyond_its_bar(name):
    """On the textured pairs from one window up (below that the window variance is identically zero and the covariance mistakes have
    nothing to move): every result the mistake names moves by more than the kernels' bar, at some pixel for a gradient."""
    for H, W in [hw for hw in so.SIZES if min(hw) >= 7]:
        y, s = so.inputs('textured', H, W)
        bar = so.bars(y, s)
        for fn, mutant in so.MUTATIONS[name].items():
            ref, got = getattr(so, fn)(y, s), mutant(y, s)
            if fn == 'ssim':
                assert abs(got - ref) > 10 * bar['value'], f'{name} / {fn} at {H} x {W}: moved by {abs(got - ref):.3e}, bar {bar["value"]:.3e}'
            else:
                b = bar['grad_sum'] / (1 if fn == 'grad_sum' else 3 * H * W)
                assert (np.abs(got - ref) / b).max() > 10, f'{name} / {fn} at {H} x {W}: moved by {(np.abs(got - ref) / b).max():.2f} bars'


def test_bars_hold_for_an_fp32_numpy_evaluation():
    """The walk bounds ANY fp32 evaluation in the kernels' order of operations: a plain numpy float32 evaluation of the unshifted
    formulas with the separable filter stays inside the reference-arithmetic bars (which assume no shift) on every kind."""
    w = so.taps()
    for kind in so.KINDS:
        y, s = so.inputs(kind, 13, 18)
        y3, s3 = y[..., :3], s[..., :3]
        Fh, Fw = (so.filter_matrix(n, w).astype(np.float32) for n in (13, 18))

        def f(x):
            return np.einsum('pq,qrc->prc', Fh, np.einsum('qrc,sr->qsc', x, Fw))

        mu1, mu2, e11, e22, e12 = f(y3), f(s3), f(y3 * y3), f(s3 * s3), f(y3 * s3)
        c1, c2 = np.float32(so.C1), np.float32(so.C2)
        S = ((2 * mu1 * mu2 + c1) * (2 * (e12 - mu1 * mu2) + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * ((e11 - mu1 * mu1) + (e22 - mu2 * mu2) + c2))
        assert S.dtype == np.float32
        assert (np.abs(S - so.ssim_map(y, s)) <= so.bars(y, s, so.REF)['S']).all(), kind
