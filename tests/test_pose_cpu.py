"""CPU: the pose attack's host side -- the new entry points are declared and exported, PoseJitter's value checks, the refusals of
spaa() / spaa_sweep() (raised before anything touches a GPU), the float64 / integer restatement (tests/pose_oracle.py) on its own:
identity, adjointness, a central-difference check and the generator, and the window of the adjoint kernel: its 5 x 5 gather, restated
in numpy, against autograd's adjoint at the limits a PoseJitter allows."""
import os
import re

import numpy as np
import pytest
import torch

import jitter_oracle as jo
import pose_oracle as po
from spaa_amd import _lib, synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_pose_draw', 'spaa_pose_fwd', 'spaa_pose_bwd', 'spaa_jitter_fwd_each')


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert 'pose_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert spaa_amd.PoseJitter is A.PoseJitter and spaa_amd.PoseAttackState is A.PoseAttackState
    assert spaa_amd.pose_survival is A.pose_survival
    assert issubclass(A.PoseAttackState, A.EnsembleAttackState)
    assert (A.POSE_MAX_ROTATE, A.POSE_MAX_ZOOM, A.POSE_MAX_SHIFT, A.POSE_MAX_TILT) == po.LIMITS


def test_pose_jitter_is_a_checked_immutable_value():
    p = A.PoseJitter()
    assert (p.rotate, p.zoom, p.shift, p.tilt, p.draws, p.seed) == (2.0, 0.03, 3.0, 0.02, 3, 0)
    assert p == A.PoseJitter(2.0, 0.03, 3.0, 0.02, 3, 0) and hash(p) == hash(A.PoseJitter())
    with pytest.raises(AttributeError):
        p.rotate = 3.0
    for kw in (dict(draws=1), dict(draws=5), dict(rotate=-1.0), dict(zoom=-0.01), dict(shift=-0.5), dict(tilt=-0.01), dict(rotate=10.5),
               dict(zoom=0.16), dict(tilt=0.11), dict(shift=32.5), dict(rotate=float('nan'))):
        with pytest.raises(ValueError):
            A.PoseJitter(**kw)
    for kw in (dict(draws=2), dict(draws=4), dict(rotate=0.0, zoom=0.0, shift=0.0, tilt=0.0), dict(rotate=10.0), dict(zoom=0.15),
               dict(tilt=0.1), dict(shift=32.0), dict(seed=7)):
        A.PoseJitter(**kw)


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


def test_pose_refusals(parts):
    """NotImplementedError for pose with a list of classifiers, a list of PCNets, attention or fp16 storage, TypeError for a foreign
    callable or a pose that is no PoseJitter, ValueError for focus=True or a jitter of other draws -- from spaa() and spaa_sweep() with
    device='cuda' and no GPU in reach: nothing was leased or launched."""
    pcs, clfs, setup = parts
    scene = syn.scenes(1, 1, (64, 64))
    ps = A.PoseJitter()

    def run(pcnet, classifier, sc=scene, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, sc, 5, 'caml2', 'cuda', setup, **kw)

    def sweep(pcnet, classifier, sc=scene, **kw):
        return A.spaa_sweep(pcnet, classifier, None, sc, setup, 'cuda', [('caml2', 5, True, [1, 2])], **kw)

    for call in (run, sweep):
        with pytest.raises(NotImplementedError, match='ensemble'):
            call(pcs[0], [clfs[0], clfs[1]], pose=ps)
        with pytest.raises(NotImplementedError, match='views'):
            call([pcs[0], pcs[1]], clfs[0], [scene, scene], pose=ps)
        with pytest.raises(NotImplementedError, match='attention'):
            call(pcs[0], clfs[0], pose=ps, attention=A.Attention())
        with pytest.raises(NotImplementedError, match='f16'):
            call(pcs[0], clfs[0], pose=ps, storage='f16')
        with pytest.raises(TypeError):
            call(pcs[0], lambda im, cp: None, pose=ps)
        with pytest.raises(ValueError, match='focus'):
            call(pcs[0], clfs[0], pose=ps, focus=True)
        with pytest.raises(TypeError, match='PoseJitter'):
            call(pcs[0], clfs[0], pose=dict(rotate=2.0))
        with pytest.raises(TypeError, match='PoseJitter'):
            call(pcs[0], clfs[0], pose=A.CaptureJitter())
        with pytest.raises(ValueError, match='draws'):
            call(pcs[0], clfs[0], pose=A.PoseJitter(draws=3), jitter=A.CaptureJitter(draws=2))
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)   # no engine was built on the way
    with pytest.raises(NotImplementedError):
        A.PoseAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', ps, storage='f16')
    with pytest.raises(ValueError, match='draws'):
        A.PoseAttackState(pcs[0], clfs[0], [1], scene, 'caml2', setup, 'cuda', ps, jitter=A.CaptureJitter(draws=4))
    # pose=None is the plain call, which on a CPU device raises what the plain call raises; so does a pose attack
    for kw in (dict(pose=None), dict(pose=ps), dict(pose=ps, jitter=A.CaptureJitter())):
        with pytest.raises(RuntimeError, match='GPU only'):
            A.spaa(pcs[0], clfs[0], None, [1], True, scene, 5, 'caml2', 'cpu', setup, **kw)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.spaa_sweep(pcs[0], clfs[0], None, scene, setup, 'cpu', [('caml2', 5, True, [1, 2])], pose=None)
    with pytest.raises(TypeError, match='PoseJitter'):
        A.pose_survival(torch.zeros(1, 3, 64, 64), clfs[0], [1], True, (60, 60), A.CaptureJitter())
    with pytest.raises(RuntimeError, match='GPU only'):
        A.pose_survival(torch.zeros(1, 3, 64, 64), clfs[0], [1], True, (60, 60), ps)
    assert all(not c._engines for c in clfs) and all(not m._engines for m in pcs)


def test_identity_row_leaves_the_image_unchanged():
    rng = np.random.default_rng(0)
    y = rng.uniform(0, 1, (2, 5, 7, 4))
    table = np.tile(np.array(po.IDENTITY_ROW), (2, 2, 1))
    out = po.forward(y, table)
    # (grid_sample maps the exact positions to [-1, 1] and back: the last bits of float64; the explicit form copies)
    assert np.abs(out[0, ..., :3] - y[..., :3]).max() <= 2e-15 and np.array_equal(out[1], out[0]) and (out[..., 3] == 0).all()
    assert np.abs(po.backward(y[None], table[:, :1])[0, ..., :3] - y[..., :3]).max() <= 2e-15
    xs, ys = po.source(po.IDENTITY_ROW, 5, 7)
    assert np.array_equal(po.bilinear(y[0], xs, ys), y[0])
    assert np.array_equal(xs, np.tile(np.arange(7.0), (5, 1))) and np.array_equal(ys, np.tile(np.arange(5.0)[:, None], (1, 7)))
    assert np.array_equal(po.gather_adjoint(y[0, ..., :3], po.IDENTITY_ROW), y[0, ..., :3])
    assert np.array_equal(po.row_of(0, 0, 0, 0, 0, 0, 5, 7), np.array(po.IDENTITY_ROW))


def test_explicit_form_is_grid_sample():
    """out = bilinear(y, xs, ys) with zero fill is grid_sample(bilinear, zeros, align_corners=False) on the stated grid."""
    rng = np.random.default_rng(5)
    for H, W in ((5, 7), (24, 32)):
        rows = np.concatenate((po.corner_rows(H, W), po.random_rows(rng, 8, H, W)))
        y = rng.uniform(0, 1, (len(rows), H, W, 3))
        got = po.forward(y, rows[:, None])[0, ..., :3]
        want = np.stack([po.bilinear(y[b], *po.source(rows[b], H, W)) for b in range(len(rows))])
        assert np.abs(got - want).max() <= 1e-14


@pytest.mark.parametrize('hw', [(5, 7), (17, 19)])
def test_adjoint_identity(hw):
    """<W u, v> = <u, W^T v> to 1e-10 of sum |W u v|, at the limit corners and random poses."""
    H, W = hw
    rng = np.random.default_rng(1)
    rows = np.concatenate((po.corner_rows(H, W), po.random_rows(rng, 8, H, W, (10.0, 0.15, 3.0, 0.1))))   # (shifts that stay in the frame)
    B = len(rows)
    u = rng.normal(size=(B, H, W, 3))
    v = rng.normal(size=(1, B, H, W, 3))
    Wu = po.forward(u, rows[:, None])[0, ..., :3]
    WTv = po.backward(v, rows[:, None])[0, ..., :3]
    worst = 0.0
    for b in range(B):
        scale = np.abs(Wu[b] * v[0, b]).sum()
        worst = max(worst, abs((Wu[b] * v[0, b]).sum() - (u[b] * WTv[b]).sum()) / scale)
    print(f'{hw}: worst |<Wu,v> - <u,WTv>| / sum|Wu v| = {worst:.3e}')
    assert worst <= 1e-10


def test_adjoint_against_central_differences():
    """backward() is the gradient of sum(v * forward(y)): central differences at 6 x 5 (the warp is linear in y, so the quotient is
    exact but for the rounding of the two sums)."""
    H, W = 6, 5
    rng = np.random.default_rng(2)
    rows = np.concatenate((po.corner_rows(H, W)[[0, 5, 10, 15]], po.random_rows(rng, 2, H, W, (10.0, 0.15, 2.0, 0.1))))
    table = rows.reshape(2, 3, 8)
    B, J = 2, 3
    y = rng.uniform(0, 1, (B, H, W, 3))
    v = rng.normal(size=(J, B, H, W, 3))
    g = po.backward(v, table)[..., :3].sum(axis=0)               # d/dy of sum_j <v_j, out_j>
    eps, worst = 1e-5, 0.0
    for idx in np.ndindex(B, H, W, 3):
        yp, ym = y.copy(), y.copy()
        yp[idx] += eps
        ym[idx] -= eps
        fd = ((po.forward(yp, table)[..., :3] - po.forward(ym, table)[..., :3]) * v).sum() / (2 * eps)
        worst = max(worst, abs(fd - g[idx]))
    print(f'central differences: worst |fd - adjoint| = {worst:.3e} at max |g| = {np.abs(g).max():.3f}')
    assert worst <= 1e-8 * max(1.0, np.abs(g).max())


def test_draw_tables_follow_the_rule():
    H, W = 24, 32
    ranges = (2.0, 0.03, 3.0, 0.02)
    table = po.draw_tables(3, 5, 6, 4, *ranges, H, W, clean0=True)
    assert (table[:, 0] == np.array(po.IDENTITY_ROW)).all()
    rest = table[:, 1:]
    s = np.hypot(rest[..., 0], rest[..., 3])
    ang = np.degrees(np.arctan2(rest[..., 3], rest[..., 0]))
    assert np.array_equal(rest[..., 0], rest[..., 4]) and np.array_equal(rest[..., 1], -rest[..., 3])
    assert (np.abs(s - 1) <= 0.03 + 1e-12).all() and (np.abs(ang) <= 2.0 + 1e-12).all() and (np.abs(rest[..., [2, 5]]) <= 3.0).all()
    assert (np.abs(rest[..., 6:]) * 16 <= np.float32(0.02)).all() and (rest[..., 6:] != 0).all()
    # one entry by hand, in Python integers
    u = [(po.draw_word(3, 5, 2, 1, i) >> 8) / 2.0 ** 24 for i in range(6)]
    a, sc = 2.0 * (2 * u[0] - 1) * np.pi / 180, 1 + float(np.float32(0.03)) * (2 * u[1] - 1)
    want = (sc * np.cos(a), -sc * np.sin(a), 3.0 * (2 * u[2] - 1), sc * np.sin(a), sc * np.cos(a), 3.0 * (2 * u[3] - 1),
            float(np.float32(0.02)) * (2 * u[4] - 1) / 16, float(np.float32(0.02)) * (2 * u[5] - 1) / 16)
    assert np.allclose(table[2, 1], want, rtol=1e-15, atol=0)
    dirty = po.draw_tables(3, 5, 6, 4, *ranges, H, W, clean0=False)
    assert np.array_equal(dirty[:, 1:], rest) and (dirty[:, 0, 0] != 1).all()
    assert not np.array_equal(po.draw_tables(3, 6, 6, 4, *ranges, H, W, True), table)
    assert not np.array_equal(po.draw_tables(4, 5, 6, 4, *ranges, H, W, True), table)
    # R = max(H, W) / 2 whichever side is the longer one
    assert np.array_equal(po.draw_tables(3, 5, 6, 4, *ranges, W, H, True)[..., 6:], table[..., 6:])


def test_uniforms_are_distinct_and_not_the_jitter_generators():
    idx = [(t, b, j, i) for t in range(4) for b in range(8) for j in range(4) for i in range(6)]
    us = {jo.uniform(po.draw_word(0, *k)) for k in idx}
    assert len(us) == len(idx) and all(0 <= u < 1 for u in us)
    assert all(po.draw_word(0, *k) != jo.draw_word(0, *k) for k in idx)
    assert not us & {jo.uniform(jo.draw_word(0, *k)) for k in idx}
    assert po.draw_word(1, 0, 0, 0, 0) != po.draw_word(0, 0, 0, 0, 0)
    # the chain with the other first constant, spelled out
    h = jo.mix32(7 ^ 0x85ebca6b)
    for v in (1, 2, 3, 4):
        h = jo.mix32(h ^ v)
    assert po.draw_word(7, 1, 2, 3, 4) == h


def _gather_error(rows, H, W, rng):
    """max |5 x 5 gather - autograd's adjoint| over the rows, and the largest reach |m - H^-1 p| of a contribution."""
    g = rng.normal(size=(1, len(rows), H, W, 3))
    want = po.backward(g, rows[:, None])[0, ..., :3]
    err = max(np.abs(po.gather_adjoint(g[0, b], rows[b]) - want[b]).max() for b in range(len(rows)))
    return err, max(po.window_reach(row, H, W) for row in rows)


@pytest.mark.parametrize('hw', [(24, 32), (240, 320), (256, 256)])
def test_window_holds_every_contribution(hw):
    """The adjoint kernel's window: at the 16 limit corners (10 degrees, zoom 0.15, tilt 0.1 per axis) and for 100 random poses within
    the limits the 5 x 5 gather IS the adjoint (1e-12 against autograd's: a lost contribution would show as a weight of order 1),
    and no contribution lies 2.5 or more from H^-1 p, where rounding the centre could lose it."""
    H, W = hw
    rng = np.random.default_rng(H + W)
    err_c, reach_c = _gather_error(po.corner_rows(H, W), H, W, rng)
    err_r, reach_r = _gather_error(po.random_rows(rng, 100, H, W), H, W, rng)
    print(f'{hw}: corners |gather - autograd| {err_c:.3e}, reach {reach_c:.3f}; 100 random poses {err_r:.3e}, reach {reach_r:.3f}')
    assert err_c <= 1e-12 and err_r <= 1e-12
    assert max(reach_c, reach_r) < po.WINDOW + 0.5
    # a 3 x 3 window is not enough at these limits: the check above can fail
    small = max(np.abs(po.gather_adjoint(np.ones((H, W, 1)), row, window=1) - po.gather_adjoint(np.ones((H, W, 1)), row)).max()
                for row in po.corner_rows(H, W)[:4])
    assert small > 1e-3
