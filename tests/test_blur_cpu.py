"""CPU: the blur attack's host side and its float64 restatement (tests/blur_oracle.py) on its own.  The restated forward against torch
float64 F.pad(mode='replicate') + F.conv2d, the restated transpose (an explicit matrix) against autograd of that and against the fold
formula of include/spaa_hip.h, every mutation of blur_oracle.MUTATIONS moving a compared output beyond its bar, the drawn sigmas' rule,
CaptureBlur's value checks, the refusals of spaa() / spaa_sweep() (raised before anything touches a GPU), and the interface: declared,
exported, counted.  (The restatement itself needs nothing of the feature: the tests of the option value, the refusals, the stage
order and the interface are the ones that fail without it.)"""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blur_oracle as bo
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_blur_rows', 'spaa_blur_draw', 'spaa_blur_fwd', 'spaa_blur_bwd')
SIGMAS = (0.2, 0.33, 0.5, 1.0, 4.0 / 3.0, 1.7, 2.5, 2.6)
SHAPES = ((1, 1), (3, 5), (8, 9), (21, 13), (16, 40))


def torch_blur(y, r, w):
    """y [H][W][C] float64 tensor -> replicate padding by r and the two 1-D convolutions with the full kernel of the half kernel w."""
    k = torch.from_numpy(np.concatenate((w[r:0:-1], w[:r + 1])))
    x = y.permute(2, 0, 1)[:, None]                                            # [C,1,H,W]
    x = F.pad(x, (r, r, r, r), mode='replicate') if r else x
    x = F.conv2d(x, k.view(1, 1, 1, -1))
    x = F.conv2d(x, k.view(1, 1, -1, 1))
    return x[:, 0].permute(1, 2, 0)


@pytest.mark.parametrize('hw', SHAPES)
def test_forward_and_transpose_against_torch(hw):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    y, g = bo.float_image(rng, *hw), rng.normal(size=hw + (3,))
    worst_f = worst_t = worst_i = 0.0
    for sigma in SIGMAS:
        r, w = bo.taps(np.float32(sigma))
        assert r == min(8, int(np.ceil(np.float32(3.0) * np.float32(sigma)))) and abs(w[0] + 2 * w[1:].sum() - 1) < 1e-15 and (w[r + 1:] == 0).all()
        yt = torch.from_numpy(y).requires_grad_(True)
        out = torch_blur(yt, r, w)
        got = bo.forward(y, r, w)
        worst_f = max(worst_f, float(np.abs(got - out.detach().numpy()).max()))
        auto, = torch.autograd.grad((out * torch.from_numpy(g)).sum(), yt)
        back = bo.backward(g, r, w)
        worst_t = max(worst_t, float(np.abs(back - auto.numpy()).max()))
        worst_i = max(worst_i, abs(float((got * g).sum() - (y * back).sum())) / float(np.abs(got * g).sum()))
    print(f'accuracy: restatement {hw}: forward against F.pad + F.conv2d {worst_f:.2e}, transpose against autograd {worst_t:.2e}, '
          f'|<Ax,g> - <x,ATg>| / sum|Ax g| {worst_i:.2e} (bars 1e-13)')
    assert worst_f <= 1e-13 and worst_t <= 1e-13 and worst_i <= 1e-13


def test_fold_formula_is_the_transposed_matrix():
    """The header's formula (z_e, the two folds) against the explicit transposed matrix for n = 1 .. 40: n = 1 (everything in one pixel),
    n - 1 < r (both folds live at once), n = r, n = r + 1 and the interior."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for sigma in (0.2, 0.7, 1.0, 2.0, 2.6):
        r, w = bo.taps(np.float32(sigma))
        for n in range(1, 41):
            g = rng.normal(size=(n, 2))
            worst = max(worst, float(np.abs(bo.fold_formula(g, r, w) - bo.transpose_matrix(n, r, w) @ g).max()))
    print(f'accuracy: fold formula against the transposed matrix, n = 1..40: {worst:.2e} (bar 1e-14)')
    assert worst <= 1e-14


def test_rows_and_the_identity_row():
    assert np.array_equal(bo.row_of(0.0), [0, 0, 1] + [0] * 9) and bo.radius(0.0) == 0 and bo.tap_ulps(0.0) == 0
    y = bo.float_image(np.random.default_rng(2), 7, 9)
    r, w = bo.taps(0.0)
    assert np.array_equal(bo.forward(y, r, w), y) and np.array_equal(bo.backward(y, r, w), y)
    # ceil(3 sigma) in fp32: a sigma on either side of an integer 3 sigma, and the cap
    for sigma, r in ((np.float32(1 / 3), 1), (np.nextafter(np.float32(1 / 3), np.float32(1)), 2), (np.float32(2.0), 6),
                     (np.nextafter(np.float32(2.0), np.float32(3)), 7), (np.float32(2.5), 8), (np.float32(2.6), 8), (np.float32(1e-30), 1)):
        assert bo.radius(sigma) == r, (sigma, r)
        row = bo.row_of(sigma)
        assert row[1] == r and (row[3 + r:] == 0).all() and abs(row[2] + 2 * row[3:11].sum() - 1) < 1e-15 and np.isfinite(row).all()
    assert bo.rows_of(np.zeros((2, 3))).shape == (2, 3, 12)


def test_draw_sigmas_follow_the_rule():
    import jitter_oracle as jo
    s = bo.draw_sigmas(7, 2, 70, 4, 0.5, 2.0, clean0=True)
    assert s.shape == (70, 4) and (s[:, 0] == 0).all() and (s[:, 1:] >= 0.5).all() and (s[:, 1:] <= 2.0).all() and len(np.unique(s)) > 200
    assert np.array_equal(s, s.astype(np.float32).astype(np.float64))
    dirty = bo.draw_sigmas(7, 2, 70, 4, 0.5, 2.0, clean0=False)
    assert np.array_equal(dirty[:, 1:], s[:, 1:]) and (dirty[:, 0] >= 0.5).all()
    assert not np.array_equal(bo.draw_sigmas(7, 3, 70, 4, 0.5, 2.0, True), s)
    assert (bo.draw_sigmas(7, 2, 4, 2, 1.3, 1.3, False) == float(np.float32(1.3))).all()        # lo == hi gives exactly lo
    assert bo.draw_word(1, 2, 3, 1, 0) != jo.draw_word(1, 2, 3, 1, 0) and bo.draw_word(1, 2, 3, 1, 0, 'jitter_constant') == jo.draw_word(1, 2, 3, 1, 0)
    assert abs(dirty.mean() - 1.25) < 0.1


@pytest.mark.parametrize('bug', sorted(bo.MUTATIONS))
def test_mutations_are_caught(bug):
    """Each mutation moves the output it belongs to beyond ten times that output's bar."""
    assert set(bo.DRAW_MUTATIONS + bo.ROW_MUTATIONS + bo.FORWARD_MUTATIONS + bo.BACKWARD_MUTATIONS) == set(bo.MUTATIONS)
    rng = np.random.default_rng(4)
    if bug in bo.DRAW_MUTATIONS:
        good, bad = (bo.draw_sigmas(5, 1, 6, 3, 0.5, 2.0, True, _bug=b) for b in (None, bug))
        over = float((np.abs(bad - good) / bo.bar_sigma(0.5, 2.0)).max())
    elif bug in bo.ROW_MUTATIONS:
        over = 0.0
        for sigma in (np.float32(0.9), np.float32(1.7)):
            diff = np.abs(bo.row_of(sigma, bug) - bo.row_of(sigma))
            bar = bo.bar_row(sigma)
            over = max(over, float((diff[bar > 0] / bar[bar > 0]).max()), np.inf if (diff[bar == 0] > 0).any() else 0.0)
    else:
        hw = (21, 13)                                                          # (H > W: the column pass clamped with W reads other rows)
        y = bo.float_image(rng, *hw)
        sigma = np.float32(1.2)
        r, w = bo.taps(sigma)
        if bug in bo.FORWARD_MUTATIONS:
            diff, bar = np.abs(bo.forward(y, r, w, bug) - bo.forward(y, r, w)), bo.bar_forward(y, r, w, bo.tap_ulps(sigma))
        else:
            diff, bar = np.abs(bo.backward(y, r, w, bug) - bo.backward(y, r, w)), bo.bar_backward(y, r, w, bo.tap_ulps(sigma))
        over = float((diff / bar).max())
    print(f'mutation {bug} ({bo.MUTATIONS[bug]}): largest change / bar = {over:.3g}')
    assert over > 10, bug


def test_capture_blur_is_a_checked_immutable_value():
    b = A.CaptureBlur()
    assert (b.sigma, b.draws, b.seed) == ((0.5, 2.0), 3, 0) and b.sigma_range == (0.5, 2.0)
    assert b == A.CaptureBlur((0.5, 2.0), 3, 0) and hash(b) == hash(A.CaptureBlur())
    assert A.CaptureBlur(sigma=1).sigma_range == (1.0, 1.0) and A.CaptureBlur(sigma=[0, 1.5]).sigma == (0, 1.5)
    assert A.BLUR_RMAX == 8 and A.BLUR_SIGMA_MAX == 2.5 and 'not a measurement' in A.CaptureBlur.__doc__
    with pytest.raises(AttributeError):
        b.sigma = 1.0
    for kw in (dict(draws=1), dict(draws=5), dict(sigma=-0.1), dict(sigma=2.6), dict(sigma=(1.5, 0.5)), dict(sigma=(-0.5, 1)),
               dict(sigma=(0.5, 2.51)), dict(sigma=float('nan')), dict(sigma=(0.5, float('inf'))), dict(sigma=True), dict(sigma='1'),
               dict(sigma=(0.5, 1.0, 2.0)), dict(sigma=None)):
        with pytest.raises(ValueError):
            A.CaptureBlur(**kw)
    for kw in (dict(sigma=0), dict(sigma=0.0), dict(sigma=(0, 0))):
        with pytest.raises(ValueError, match='is no blur, the plain attack'):
            A.CaptureBlur(**kw)
    for kw in (dict(draws=2), dict(draws=4), dict(sigma=2.5), dict(sigma=(0, 2.5)), dict(sigma=0.01, seed=7)):
        A.CaptureBlur(**kw)


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


class _Passed:
    """What a stubbed `_attack_state` returns (as tools/attack_requests.py stubs it): it records the keywords it was built with."""
    seen = []

    def __init__(self, pcnet, classifier, target_idx, *rest, **kw):
        self.n = len(target_idx)
        _Passed.seen.append((rest, kw))

    def results(self):
        return torch.zeros(self.n, 1), torch.zeros(self.n, 1)


def test_blur_refusals(parts, monkeypatch):
    """Every refusal carries its message -- from spaa() and spaa_sweep() with device='cuda' and no GPU in reach: nothing was leased or
    launched; a request that passes reaches the (stubbed) state with its blur."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    bl = A.CaptureBlur()

    def run(pcnet, classifier, sc=scene, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, sc, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(pcnet, classifier, sc=scene, **kw):
        return A.spaa_sweep(pcnet, classifier, None, sc, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='lens blur against an ensemble of classifiers is not implemented'):
            call(pcs[0], [clfs[0], clfs[1]], blur=bl)
        with pytest.raises(NotImplementedError, match='lens blur against several views is not implemented'):
            call([pcs[0], pcs[1]], clfs[0], [scene, scene], blur=bl)
        with pytest.raises(NotImplementedError, match="storage='f16' is not implemented with blur"):
            call(pcs[0], clfs[0], blur=bl, storage='f16')
        with pytest.raises(TypeError, match='a blur attack needs a spaa_amd.Classifier'):
            call(pcs[0], lambda im, cp: None, blur=bl)
        with pytest.raises(ValueError, match='focus=True has no meaning with blur'):
            call(pcs[0], clfs[0], blur=bl, focus=True)
        with pytest.raises(NotImplementedError, match='attention together with lens blur is not implemented'):
            call(pcs[0], clfs[0], blur=bl, attention=A.Attention())
        with pytest.raises(TypeError, match='blur must be a spaa_amd.CaptureBlur'):
            call(pcs[0], clfs[0], blur=dict(sigma=1.0))
        for name, other in (('jitter', A.CaptureJitter(draws=2)), ('pose', A.PoseJitter(draws=4)), ('jpeg', A.JpegCapture(draws=2))):
            with pytest.raises(ValueError, match=rf'{name} and blur are applied draw by draw and must name the same draws, got {name}.draws = '
                                                 rf'{other.draws} and blur.draws = 3'):
                call(pcs[0], clfs[0], blur=bl, **{name: other})
    with pytest.raises(NotImplementedError, match='universal together with blur is not implemented'):
        run(pcs[0], clfs[0], blur=bl, universal=A.Universal(2))
    with pytest.raises(NotImplementedError, match='universal= is not implemented'):
        sweep(pcs[0], clfs[0], blur=bl, universal=A.Universal(2))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)   # no engine was built on the way
    with pytest.raises(NotImplementedError):
        A.BlurAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', bl, storage='f16')
    with pytest.raises(ValueError, match='same draws'):
        A.BlurAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', bl, jpeg=A.JpegCapture(draws=4))
    with pytest.raises(TypeError, match='blur must be a spaa_amd.CaptureBlur'):
        A.BlurAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', A.JpegCapture())
    # blur=None is the plain call, which on a CPU device raises what the plain call raises; so does a blur attack
    for kw in (dict(blur=None), dict(blur=bl), dict(blur=bl, jitter=A.CaptureJitter(), pose=A.PoseJitter(), jpeg=A.JpegCapture(),
                                                    transfer=A.Transfer())):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2_camssim', 'cpu', setup, **kw)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.gaussian_blur(torch.zeros(2, 3, 8, 8), 1.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.blur_survival(torch.zeros(2, 3, 64, 64), clfs[0], [1, 2], True, (60, 60))
    with pytest.raises(ValueError):
        A.gaussian_blur(torch.zeros(2, 8, 8), 1.0)
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)
    # what passes the checks reaches the state with its blur, and only then: the states stubbed, nothing built
    monkeypatch.setattr(A, '_attack_state', _Passed)
    _Passed.seen.clear()
    both = dict(jitter=A.CaptureJitter(), pose=A.PoseJitter(), jpeg=A.JpegCapture(), transfer=A.Transfer())
    for call in (run, sweep):
        call(pcs[0], clfs[0], iters=0)
        call(pcs[0], clfs[0], iters=0, blur=bl)
        call(pcs[0], clfs[0], iters=0, blur=bl, **both)
    assert [kw.get('blur') for _, kw in _Passed.seen] == [None, bl, bl] * 2


def test_the_stage_order_is_the_optical_one(parts, monkeypatch):
    """[Pose] + [Blur] + [Jitter] + [Jpeg], whatever is given; the state's own constructor stubbed out (it needs a GPU)."""
    pcs, clfs, setup = parts
    seen = []
    monkeypatch.setattr(A.DrawAttackState, '__init__', lambda self, *a, **k: seen.append([type(s).__name__ for s in a[7]]))
    bl, args = A.CaptureBlur(), (pcs[0], clfs[0], [1], None, 'caml2', setup, 'cuda')
    A.BlurAttackState(*args, bl)
    A.BlurAttackState(*args, bl, jitter=A.CaptureJitter())
    A.BlurAttackState(*args, bl, pose=A.PoseJitter(), jpeg=A.JpegCapture())
    A.BlurAttackState(*args, bl, pose=A.PoseJitter(), jitter=A.CaptureJitter(), jpeg=A.JpegCapture())
    assert seen == [['BlurStage'], ['BlurStage', 'JitterStage'], ['PoseStage', 'BlurStage', 'JpegStage'],
                    ['PoseStage', 'BlurStage', 'JitterStage', 'JpegStage']]
    st = A._attack_state(*args, 'f32', False, blur=bl, jpeg=A.JpegCapture())
    assert type(st) is A.BlurAttackState and seen[-1] == ['BlurStage', 'JpegStage']


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
        assert m, f'{name} is not declared in include/spaa_hip.h'
        assert len([a for a in m.group(1).split(',') if a.strip()]) == len(_lib._SIGNATURES[name]), name
    assert re.search(r'#define\s+SPAA_BLUR_RMAX\s+8\b', hdr) and A.BLUR_RMAX == bo.RMAX == 8 and A.BLUR_SIGMA_MAX == bo.SIGMA_MAX
    assert re.search(r'#define\s+SPAA_BLUR_TILE_W\s+32\b', hdr) and re.search(r'#define\s+SPAA_BLUR_TILE_H\s+16\b', hdr)
    assert '0x2545f491' in hdr and f'{bo.FIRST:#x}' == '0x2545f491'
    assert 'blur_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    for name in ('CaptureBlur', 'BlurAttackState', 'blur_survival', 'gaussian_blur'):
        assert getattr(spaa_amd, name) is getattr(A, name), name
    assert issubclass(A.BlurAttackState, A.DrawAttackState)


def test_request_and_launch_fixtures_still_hold():
    """blur= is a keyword that defaults to None and comes last everywhere, and the two fixtures know nothing of it."""
    for name in ('attack_request_outcomes.json', 'attack_launch_sequences.json'):
        assert 'blur' not in open(os.path.join(ROOT, 'tests', 'golden', name)).read().lower().replace('spaa_transfer_blur', ''), name
    for fn in (A.spaa, A.spaa_sweep, A._attack_state, A.checked_request):
        params = inspect.signature(fn).parameters
        assert params['blur'].default is None and list(params)[-1] == 'blur', fn.__name__
