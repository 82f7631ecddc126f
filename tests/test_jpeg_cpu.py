"""CPU: the JPEG attack's host side and its float64 restatement (tests/jpeg_oracle.py) on its own.  The quantisation tables against
Pillow's, the restated round trip against Pillow's encode + decode (the mean absolute difference in grey levels is printed as an
`accuracy:` line per case; profiles/jpeg_accuracy.txt holds the lines of one run), the adjoint against the linearisation and against
torch.autograd, the identity row, every mutation of jpeg_oracle.MUTATIONS caught, JpegCapture's value checks, the refusals of spaa() /
spaa_sweep() (raised before anything touches a GPU), and the interface: declared, exported, counted."""
import io
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_oracle as jp
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_jpeg_draw', 'spaa_jpeg_fwd', 'spaa_jpeg_bwd')
TABLE_QUALITIES = (1, 30, 49, 50, 75, 90, 100)
QUALITIES = (30, 50, 75, 90, 95)
SUBSAMPLINGS = (('4:4:4', 0), ('4:2:0', 2))
PILLOW_BAR = 2.0   # grey levels, mean absolute difference (libjpeg's integer DCT and fixed-point colour flip single roundings)


def pillow_tables(Q):
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), dtype=np.uint8)).save(buf, format='JPEG', quality=Q)
    q = Image.open(io.BytesIO(buf.getvalue())).quantization
    return np.array(q[0]).reshape(8, 8), np.array(q[1]).reshape(8, 8)


def pillow_roundtrip(im8, Q, sub):
    buf = io.BytesIO()
    Image.fromarray(im8).save(buf, format='JPEG', quality=Q, subsampling=sub)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB')).astype(np.float64)


@pytest.fixture(scope='module')
def images(golden_dir):
    fish = np.asarray(Image.open(os.path.join(golden_dir, 'anemone_fish.png')).convert('RGB'))
    assert fish.shape[0] >= 160 and fish.shape[1] >= 200, fish.shape
    smooth = np.rint(255 * jp.smooth_image(40, 56)).astype(np.uint8)
    return {'fish 120x152': np.ascontiguousarray(fish[20:140, 30:182]), 'fish 20x28': np.ascontiguousarray(fish[60:80, 90:118]),
            'smooth 40x56': smooth}


@pytest.fixture(scope='module')
def pillow(images):
    """Pillow's round trip of every case, once."""
    return {(name, Q, s): pillow_roundtrip(im, Q, code) for name, im in images.items() for Q in QUALITIES for s, code in SUBSAMPLINGS}


def test_tables_against_pillow():
    from spaa_amd.jpeg import quant_tables
    for Q in TABLE_QUALITIES:
        want = pillow_tables(Q)
        for got in (jp.quant_tables(Q), quant_tables(Q)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), Q
    for bug in jp.TABLE_MUTATIONS:
        wrong = [Q for Q in TABLE_QUALITIES if not all(np.array_equal(g, w) for g, w in zip(jp.quant_tables(Q, _bug=bug), pillow_tables(Q)))]
        print(f'mutation {bug}: tables differ from Pillow at Q in {wrong}')
        assert wrong, bug
    assert sorted(jp.zigzag_positions()[:6].tolist()) == [0, 1, 2, 8, 9, 16] and jp.zigzag_positions()[:4].tolist() == [0, 1, 8, 16]


def _mean_abs(images, pillow, bug=None):
    out = {}
    for (name, Q, s), want in pillow.items():
        got = 255.0 * jp.forward(images[name] / 255.0, Q, s, _bug=bug)['out']
        out[(name, Q, s)] = float(np.abs(got - want).mean())
    return out


def test_restatement_against_pillow_round_trip(images, pillow):
    diff = _mean_abs(images, pillow)
    for (name, Q, s), d in diff.items():
        print(f'accuracy: restatement against Pillow, {name} Q {Q} {s}: mean |difference| = {d:.3f} grey levels')
    worst = max(diff, key=diff.get)
    print(f'accuracy: restatement against Pillow, {len(diff)} cases: {min(diff.values()):.3f} .. {diff[worst]:.3f} grey levels (bar {PILLOW_BAR})')
    assert all(d <= PILLOW_BAR for d in diff.values()), (worst, diff[worst])


@pytest.mark.parametrize('bug', [b for b in jp.FORWARD_MUTATIONS if b not in jp.TABLE_MUTATIONS])
def test_forward_mutations_are_caught(images, pillow, bug):
    diff = _mean_abs(images, pillow, bug)
    over = {k: d for k, d in diff.items() if d > PILLOW_BAR}
    print(f'mutation {bug} ({jp.MUTATIONS[bug]}): {len(over)} of {len(diff)} cases over {PILLOW_BAR}, largest {max(diff.values()):.2f}')
    assert over, bug


ADJOINT_CASES = [((20, 28), 75, '4:2:0'), ((20, 28), 30, '4:4:4'), ((13, 9), 50, '4:2:0'), ((16, 16), 100, '4:4:4'), ((33, 17), 1, '4:2:0')]


def _adjoint_case(hw, seed):
    rng = np.random.default_rng(seed)
    return jp.float_image(rng, *hw), rng.normal(size=hw + (3,)), rng.normal(size=hw + (3,))


@pytest.mark.parametrize('gradient', ['soft', 'straight'])
@pytest.mark.parametrize('hw,Q,sub', ADJOINT_CASES)
def test_adjoint_identity_and_autograd(hw, Q, sub, gradient):
    """<L u, g> = <u, L^T g> against the restatement's linearisation to 1e-12 relative, and L^T g = torch.autograd's gradient of
    <forward_torch(y), g> in float64."""
    y, u, g = _adjoint_case(hw, 3)
    fw = jp.forward(y, Q, sub)
    assert not fw['in_gate'].all(), 'the case plants values outside [0, 1]'
    Lu, LTg = jp.linearised(u, y, Q, sub, gradient), jp.adjoint(g, y, Q, sub, gradient)
    lhs, rhs = (Lu * g).sum(), (u * LTg).sum()
    rel = abs(lhs - rhs) / np.abs(Lu * g).sum()
    yt = torch.from_numpy(y).requires_grad_(True)
    out = jp.forward_torch(yt, Q, sub, gradient)
    assert np.array_equal(out.detach().numpy(), fw['out'])                     # (the surrogate changes no forward value)
    auto, = torch.autograd.grad((out * torch.from_numpy(g)).sum(), yt)
    err = np.abs(auto.numpy() - LTg).max() / np.abs(LTg).max()
    print(f'{hw} Q {Q} {sub} {gradient}: |<Lu,g> - <u,LTg>| / sum|Lu g| = {rel:.2e}, adjoint against autograd {err:.2e}')
    assert rel <= 1e-12 and err <= 1e-12
    for bug in jp.ADJOINT_MUTATIONS:
        # (no padding, no padded cells; and 'straight' 4:4:4 is IDCT . DCT = the identity per block, which carries nothing to them)
        if (bug == 'nophi' and gradient != 'soft') or (bug == 'droppad' and ((hw[0] % 16 == 0 and hw[1] % 16 == 0) or
                                                                              (gradient == 'straight' and sub == '4:4:4'))):
            continue
        wrong = jp.adjoint(g, y, Q, sub, gradient, _bug=bug)
        bar = jp.bar_adjoint(g, y, Q, sub, gradient)
        over = (np.abs(wrong - LTg) / np.maximum(bar, 1e-300)).max()
        print(f'    mutation {bug}: largest error / fp32 bar = {over:.3g}')
        assert over > 10, bug


def test_identity_row_is_the_identity():
    y, u, g = _adjoint_case((11, 14), 5)
    for sub in ('4:4:4', '4:2:0'):
        fw = jp.forward(y, 0, sub)
        assert np.array_equal(fw['out'], y) and (fw['gate'] == 0x77).all()
        for gradient in ('soft', 'straight'):
            assert np.array_equal(jp.adjoint(g, y, 0, sub, gradient), g) and np.array_equal(jp.linearised(u, y, 0, sub, gradient), u)
        yt = torch.from_numpy(y).requires_grad_(True)
        assert torch.equal(torch.autograd.grad(jp.forward_torch(yt, 0, sub).sum(), yt)[0], torch.ones_like(yt))
    assert (jp.draw_rows(3, 0, 5, 4, 60, 95, True)[:, 0] == 0).all()


def test_draw_rows_follow_the_rule():
    rows = jp.draw_rows(7, 2, 70, 4, 60, 95, clean0=True)
    assert rows.shape == (70, 4, 4) and (rows[..., 1:] == 0).all() and (rows[:, 0, 0] == 0).all()
    q = rows[:, 1:, 0]
    assert (q >= 60).all() and (q <= 95).all() and (q == np.rint(q)).all() and len(np.unique(q)) > 20
    dirty = jp.draw_rows(7, 2, 70, 4, 60, 95, clean0=False)
    assert np.array_equal(dirty[:, 1:], rows[:, 1:]) and (dirty[:, 0, 0] >= 60).all()
    assert not np.array_equal(jp.draw_rows(7, 3, 70, 4, 60, 95, True), rows) and (jp.draw_rows(7, 2, 4, 2, 80, 80, False)[..., 0] == 80).all()
    # another first constant than the jitter's and the pose's: one seed, independent tables
    import jitter_oracle as jo
    assert jp.draw_word(1, 2, 3, 1, 0) != jo.draw_word(1, 2, 3, 1, 0)
    # the ends of the range are reached: n = 3 values over 400 rows
    ends = jp.draw_rows(0, 0, 100, 4, 1, 3, False)[..., 0]
    assert set(np.unique(ends).tolist()) == {1.0, 2.0, 3.0}


def test_safe_block_share_of_the_gpu_cases():
    """The condition of tests/test_jpeg_ops_gpu.py, checked where no GPU is needed: with its seeds at most 10 % of the 8 x 8 blocks of
    any case hold a c / T within 1e-3 of a half-integer, and at most 2 % of the pixels a pre-round value within 1e-3 of a boundary."""
    import jpeg_cases as jc
    worst_b = worst_p = 0.0
    for hw in jc.SHAPES:
        for sub in ('4:4:4', '4:2:0'):
            for J in jc.DRAWS:
                y, rows = jc.inputs(hw, J)
                for b in range(jc.B):
                    for j in range(J):
                        fw = jp.forward(y[b], int(rows[b, j, 0]), sub)
                        safe = jp.safe_pixels(fw, *hw, sub)
                        near = (jp.round_distance(fw['v']) < jp.ROUND_MARGIN).any(axis=-1) if fw['ratios'] is not None else np.zeros(hw, bool)
                        share_b, share_p = jp.unsafe_block_fraction(fw), float((near & safe).mean())
                        worst_b, worst_p = max(worst_b, share_b), max(worst_p, share_p)
                        assert share_b <= jc.MAX_UNSAFE_BLOCKS and share_p <= jc.MAX_NEAR_PIXELS, (hw, sub, J, b, j, share_b, share_p)
    print(f'accuracy: GPU cases, largest share of blocks left out {worst_b:.3%} (at most {jc.MAX_UNSAFE_BLOCKS:.0%}), of pixels near a '
          f'rounding boundary {worst_p:.3%} (at most {jc.MAX_NEAR_PIXELS:.0%})')


def test_jpeg_capture_is_a_checked_immutable_value():
    j = A.JpegCapture()
    assert (j.quality, j.subsampling, j.gradient, j.draws, j.seed) == ((60, 95), '4:2:0', 'soft', 3, 0)
    assert j == A.JpegCapture((60, 95), '4:2:0', 'soft', 3, 0) and hash(j) == hash(A.JpegCapture()) and j.quality_range == (60, 95)
    assert A.JpegCapture(quality=80).quality_range == (80, 80) and A.JpegCapture(quality=[70, 90]).quality == (70, 90)
    with pytest.raises(AttributeError):
        j.quality = 50
    for kw in (dict(draws=1), dict(draws=5), dict(quality=0), dict(quality=101), dict(quality=(95, 60)), dict(quality=(0, 50)),
               dict(quality=(50, 101)), dict(quality=75.0), dict(quality=(60.0, 95)), dict(quality=True), dict(quality=(60, 80, 95)),
               dict(subsampling='4:2:2'), dict(subsampling=2), dict(gradient='hard'), dict(gradient=None)):
        with pytest.raises(ValueError):
            A.JpegCapture(**kw)
    for kw in (dict(draws=2), dict(draws=4), dict(quality=1), dict(quality=100), dict(quality=(1, 100)), dict(subsampling='4:4:4'),
               dict(gradient='straight', seed=7)):
        A.JpegCapture(**kw)


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


def test_jpeg_refusals(parts):
    """Every refusal carries its message -- from spaa() and spaa_sweep() with device='cuda' and no GPU in reach: nothing was leased or
    launched."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    jg = A.JpegCapture()

    def run(pcnet, classifier, sc=scene, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, sc, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(pcnet, classifier, sc=scene, **kw):
        return A.spaa_sweep(pcnet, classifier, None, sc, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='camera JPEG against an ensemble of classifiers is not implemented'):
            call(pcs[0], [clfs[0], clfs[1]], jpeg=jg)
        with pytest.raises(NotImplementedError, match='camera JPEG against several views is not implemented'):
            call([pcs[0], pcs[1]], clfs[0], [scene, scene], jpeg=jg)
        with pytest.raises(NotImplementedError, match="storage='f16' is not implemented with jpeg"):
            call(pcs[0], clfs[0], jpeg=jg, storage='f16')
        with pytest.raises(TypeError, match='a JPEG attack needs a spaa_amd.Classifier'):
            call(pcs[0], lambda im, cp: None, jpeg=jg)
        with pytest.raises(ValueError, match='focus=True has no meaning with jpeg'):
            call(pcs[0], clfs[0], jpeg=jg, focus=True)
        with pytest.raises(NotImplementedError, match='attention together with camera JPEG is not implemented'):
            call(pcs[0], clfs[0], jpeg=jg, attention=A.Attention())
        with pytest.raises(TypeError, match='jpeg must be a spaa_amd.JpegCapture'):
            call(pcs[0], clfs[0], jpeg=dict(quality=75))
        with pytest.raises(ValueError, match=r'jitter and jpeg are applied draw by draw and must name the same draws, got jitter.draws = 2 and '
                                             r'jpeg.draws = 3'):
            call(pcs[0], clfs[0], jpeg=jg, jitter=A.CaptureJitter(draws=2))
        with pytest.raises(ValueError, match=r'pose and jpeg are applied draw by draw and must name the same draws, got pose.draws = 4 and '
                                             r'jpeg.draws = 3'):
            call(pcs[0], clfs[0], jpeg=jg, pose=A.PoseJitter(draws=4))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)   # no engine was built on the way
    with pytest.raises(NotImplementedError):
        A.JpegAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', jg, storage='f16')
    with pytest.raises(ValueError, match='same draws'):
        A.JpegAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', jg, jitter=A.CaptureJitter(draws=4))
    # jpeg=None is the plain call, which on a CPU device raises what the plain call raises; so does a JPEG attack
    for kw in (dict(jpeg=None), dict(jpeg=jg), dict(jpeg=jg, jitter=A.CaptureJitter(), pose=A.PoseJitter(), transfer=A.Transfer())):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2_camssim', 'cpu', setup, **kw)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.jpeg_roundtrip(torch.zeros(2, 3, 8, 8), 75)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.jpeg_survival(torch.zeros(2, 3, 64, 64), clfs[0], [1, 2], True, (60, 60))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)


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
    assert re.search(r'\bint64_t\s+spaa_jpeg_ws_floats\s*\(', hdr) and 'spaa_jpeg_ws_floats' in _lib.EXPORTS
    assert re.search(r'#define\s+SPAA_JPEG_444\s+0\b', hdr) and re.search(r'#define\s+SPAA_JPEG_420\s+2\b', hdr)
    from spaa_amd.attack_options import JPEG_SUBSAMPLINGS
    assert JPEG_SUBSAMPLINGS == {'4:4:4': 0, '4:2:0': 2}
    assert 'jpeg_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    # the workspace query is host arithmetic: none for 4:4:4, the padded planes for 4:2:0
    assert lib.spaa_jpeg_ws_floats(0, 3, 4, 20, 28) == 0 and lib.spaa_jpeg_ws_floats(2, 3, 4, 20, 28) == 3 * 4 * 32 * 32 * 3 // 2
    assert lib.spaa_jpeg_ws_floats(2, 2, 1, 16, 16) == 2 * 16 * 16 * 3 // 2 and lib.spaa_jpeg_ws_floats(1, 2, 1, 16, 16) == 0
    for name in ('JpegCapture', 'JpegAttackState', 'jpeg_survival', 'jpeg_roundtrip', 'quant_tables'):
        assert getattr(spaa_amd, name) is getattr(A, name), name
    assert issubclass(A.JpegAttackState, A.DrawAttackState)


def test_request_and_launch_fixtures_still_hold():
    """jpeg= is a keyword that defaults to None everywhere, and the two fixtures know nothing of it: the request outcomes
    (tests/test_attack_requests_cpu.py regenerates and compares them) and the launch sequences (tests/test_attack_launches_gpu.py) are
    those recorded before the feature."""
    import inspect
    for name in ('attack_request_outcomes.json', 'attack_launch_sequences.json'):
        assert 'jpeg' not in open(os.path.join(ROOT, 'tests', 'golden', name)).read().lower(), name
    for fn in (A.spaa, A.spaa_sweep, A._attack_state, A.checked_request):
        assert inspect.signature(fn).parameters['jpeg'].default is None, fn.__name__
