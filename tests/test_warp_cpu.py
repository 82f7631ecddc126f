"""CPU: the float64 restatement of the warp kernels (tests/warp_oracle.py) on its own and the tap plumbing of spaa_amd/models.py.
The restatement against oracle/spaa_oracle.py's tps_grid with F.affine_grid / F.grid_sample and against autograd, all in
torch.float64, to 1e-12; every entry of warp_oracle.MUTATIONS moves a result by more than the bar that tests/test_warp_ops_gpu.py
holds the kernels to, on that test's own inputs (so no bar is vacuous); models.tiled_taps on tap tables made by the restatement:
the number of tiles gathered from global memory (`direct`), every entry's index and weight."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spaa_oracle as so
import warp_oracle as wo
from spaa_amd import models as M

TOL = 1e-12
IDS = [wo.case_id(c) for c in wo.CASES]


def _f64(fn):
    """Runs fn with torch's default dtype float64 (tps_grid draws its linspace in the default dtype)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return fn()
    finally:
        torch.set_default_dtype(old)


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)[..., :3].transpose(0, 3, 1, 2)))


def _grid_t(grid, B):
    return torch.from_numpy(np.asarray(grid, dtype=np.float64)[None, ..., :2]).expand(B, -1, -1, -1)


@pytest.mark.parametrize('n', [1, 2, 3, 6, 17, 33, 52, 64])
def test_linspace_is_atens(n):
    a = wo.linspace(-1.0, 1.0, n)
    assert np.abs(a - torch.linspace(-1, 1, n, dtype=torch.float64).numpy()).max() <= 4 * np.finfo(np.float64).eps
    if n > 1:
        assert a[0] == -1.0 and a[-1] == 1.0
        assert np.array_equal(a, -a[::-1])                                    # the symmetric halves: exactly antisymmetric
    b = wo.linspace(0.0, 1.0, n)
    assert np.abs(b - torch.linspace(0, 1, n, dtype=torch.float64).numpy()).max() <= 4 * np.finfo(np.float64).eps


@pytest.mark.parametrize('sizes', wo.GRID_SIZES)
@pytest.mark.parametrize('T', wo.GRID_T)
@pytest.mark.parametrize('name', [p[0] for p in wo.GRID_PARAMS])
def test_grid_build_against_spaa_oracle(name, T, sizes):
    out_size, in_size = sizes
    aff, theta, ctrl, refine = wo.grid_inputs(name, T, out_size)
    coarse = wo.coarse_grid(aff, theta, ctrl, T, in_size, out_size)

    def ref():
        a = F.affine_grid(torch.from_numpy(aff.astype(np.float64)).view(1, 2, 3), torch.Size([1, 3, *in_size]), align_corners=True)
        t = so.tps_grid(torch.from_numpy(theta.astype(np.float64))[None], torch.from_numpy(ctrl.astype(np.float64)), (1, 3) + out_size)
        return F.grid_sample(a.permute(0, 3, 1, 2), t, align_corners=True)[0].permute(1, 2, 0)
    want = _f64(ref)
    assert np.abs(coarse - want.numpy()).max() <= TOL
    r = torch.from_numpy(refine[..., :2].astype(np.float64))
    assert np.abs(wo.finish_grid(coarse, refine) - torch.clamp(r + want, -1, 1).numpy()).max() <= TOL
    assert np.abs(wo.finish_grid(coarse) - torch.clamp(want, -1, 1).numpy()).max() <= TOL
    fine = wo.finish_grid(coarse, refine)
    assert (fine == 1.0).any() and (fine == -1.0).any() and (np.abs(fine) < 1).any()   # the planted refine crosses both limits


@pytest.mark.parametrize('case', wo.CASES, ids=IDS)
def test_sample_and_adjoint_against_autograd(case):
    (hc, wc), (hp, wp), kind, B = case
    d = wo.inputs(case)
    for mk in wo.MASK_KINDS:
        for clamp in (False, True):
            for with_s in (False, True):
                x = _nchw(d['x']).requires_grad_(True)
                m = 1.0 if d['mask'][mk] is None else torch.from_numpy(d['mask'][mk].astype(np.float64))
                xw = F.grid_sample(x.clamp(0, 1) if clamp else x, _grid_t(d['grid'], B), mode='bilinear', padding_mode='zeros',
                                   align_corners=True) * m
                loss = (xw * _nchw(d['g'])).sum()
                if with_s:
                    loss = loss + (xw * _nchw(d['s']) * _nchw(d['g_xs'])).sum()
                gx, = torch.autograd.grad(loss, x)
                got = wo.sample(d['x'], d['grid'], d['mask'][mk], clamp)
                assert (got[..., 3] == 0).all()
                assert np.abs(got[..., :3] - xw.detach().permute(0, 2, 3, 1).numpy()).max() <= TOL
                adj = wo.adjoint(d['g'], d['g_xs'] if with_s else None, d['s'] if with_s else None, d['x'], d['grid'],
                                 d['mask'][mk], clamp)
                assert (adj[..., 3] == 0).all()
                assert np.abs(adj[..., :3] - gx.permute(0, 2, 3, 1).numpy()).max() <= TOL * max(1.0, float(gx.abs().max()))


def test_prjl2_and_sumsq_against_autograd():
    B, hp, wp = 3, 4, 6
    x = wo.image(B, hp, wp, 3)
    x[:, 2, 3, :3] = 0.5                                                       # one pixel equal to gray: norm 0, gradient 0
    g = np.random.default_rng(0).standard_normal((B, hp, wp, 4))
    scale, state = np.array([0.3, 0.0, 0.7]), np.array([[0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]])
    xt = _nchw(x).requires_grad_(True)
    loss = (torch.norm(0.5 - xt, dim=1).sum(dim=(1, 2)) * torch.from_numpy(scale)).sum()
    gp, = torch.autograd.grad(loss, xt)
    got, ss = wo.prjl2_and_sumsq(g, x, 0.5, scale, state)
    want = g[..., :3] + gp.permute(0, 2, 3, 1).numpy()
    assert np.abs(got[..., :3] - want).max() <= TOL
    assert np.array_equal(got[1], g[1]) and np.array_equal(got[0, 2, 3], g[0, 2, 3]) and np.array_equal(got[..., 3], g[..., 3])
    assert np.abs(ss - (want ** 2).reshape(B, -1).sum(axis=1)).max() <= 1e-10
    off, _ = wo.prjl2_and_sumsq(g, x, 0.5, 0.3, np.array([[0, 0, 0, 0]] * 3))   # state[b][1] == 0: no term
    assert np.array_equal(off, g)
    one, _ = wo.prjl2_and_sumsq(g, x, 0.5, 0.3, state)                          # one scale for every image
    assert np.abs(one[0] - got[0]).max() <= TOL and not np.array_equal(one[1], g[1])


@pytest.mark.parametrize('case', wo.CASES, ids=IDS)
def test_taps_and_their_transposed_form(case):
    """The tap table reproduces `sample`, the CSR form reproduces `adjoint`; out-of-frame taps carry the sentinel and weight 0 and
    belong to no list."""
    (hc, wc), (hp, wp), kind, B = case
    d = wo.inputs(case)
    src, wgt = wo.taps(d['grid'], hp, wp)
    oof = src == wo.SENTINEL
    assert (wgt[oof] == 0).all() and ((src[~oof] >= 0) & (src[~oof] < hp * wp)).all()
    if kind == 'd':
        assert oof.all(axis=1).any()                                           # pixels wholly off the frame
    x = np.asarray(d['x'], dtype=np.float64)[..., :3].reshape(B, hp * wp, 3)
    val = (x[:, np.where(oof, 0, src)] * wgt[None, ..., None]).sum(axis=2).reshape(B, hc, wc, 3)
    assert np.abs(val - wo.sample(d['x'], d['grid'])[..., :3]).max() <= TOL
    m = d['mask']['frac']
    off, order, wm = wo.transposed(src, wgt, m, hp * wp)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == (~oof).sum()
    flat = src.reshape(-1)
    assert (flat[order[off[-1]:]] == wo.SENTINEL).all()
    sp = np.repeat(np.arange(hp * wp), np.diff(off))
    assert np.array_equal(flat[order[:off[-1]]], sp)
    assert (np.diff(order[:off[-1]])[np.diff(sp) == 0] > 0).all()              # ties in camera-pixel order
    g = np.asarray(d['g'], dtype=np.float64)[..., :3].reshape(B, hc * wc, 3)
    acc = np.zeros((B, hp * wp, 3))
    ent = order[:off[-1]]
    np.add.at(acc, (slice(None), sp), g[:, ent >> 2] * wm[ent].astype(np.float64)[None, :, None])
    assert np.abs(acc.reshape(B, hp, wp, 3) - wo.adjoint(d['g'], None, None, d['x'], d['grid'], m)[..., :3]).max() <= 1e-6


def _moved(mut, ref, bar):
    return bool((np.abs(mut - ref) > bar).any())


@pytest.mark.parametrize('case', wo.CASES, ids=IDS)
def test_mutations_of_sample_and_adjoint_exceed_the_bars(case):
    """On the inputs of the GPU tests' forward and adjoint checks, every mistake in MUTATIONS that can show on a variant (a mask
    mistake needs a mask, a gate mistake the clamp, a padding mistake taps off the frame
    where the mask is not 0: kind d without a mask) moves the float64 result by more than
    bar_fwd / bar_bwd."""
    (hc, wc), (hp, wp), kind, B = case
    d = wo.inputs(case)
    for mk in wo.MASK_KINDS:
        m = d['mask'][mk]
        for clamp in (False, True):
            ref_f, bf = wo.sample(d['x'], d['grid'], m, clamp), wo.bar_fwd(d['x'], d['grid'], clamp)
            ref_b = wo.adjoint(d['g'], d['g_xs'], d['s'], d['x'], d['grid'], m, clamp)
            bb = wo.bar_bwd(d['g'], d['g_xs'], d['s'], m, d['grid'], hp, wp)
            n = wo.reach(d['g'], d['g_xs'], d['s'], m, d['grid'], hp, wp)[1]
            assert bf < 1e-4 and 2 * wo.eps_c(d['grid'], hp, wp) + (n.max() + 8) * wo.U < 1e-4     # (the bars are tight ones)
            for name, fns in wo.MUTATIONS.items():
                if 'sample' not in fns and 'adjoint' not in fns:
                    continue
                shows = {'gate_strict': clamp, 'mask_wrong_pixel': m is not None, 'border_padding': kind == 'd' and m is None}.get(name, True)
                if not shows:
                    continue
                if 'sample' in fns:
                    assert _moved(fns['sample'](d['x'], d['grid'], m, clamp), ref_f, bf), (name, 'sample', mk, clamp)
                mut = fns['adjoint'](d['g'], d['g_xs'], d['s'], d['x'], d['grid'], m, clamp)
                assert _moved(mut[..., :3], ref_b[..., :3], bb), (name, 'adjoint', mk, clamp)


@pytest.mark.parametrize('sizes', wo.GRID_SIZES)
@pytest.mark.parametrize('T', wo.GRID_T)
@pytest.mark.parametrize('name', [p[0] for p in wo.GRID_PARAMS])
def test_mutations_of_the_grid_build_exceed_the_bars(name, T, sizes):
    out_size, in_size = sizes
    aff, theta, ctrl, refine = wo.grid_inputs(name, T, out_size)
    coarse = wo.coarse_grid(aff, theta, ctrl, T, in_size, out_size)
    bar = wo.bar_grid(aff, theta, ctrl, T, in_size, out_size)
    assert bar.max() < 2e-4
    mut = wo.MUTATIONS['linspace_not_symmetric']['coarse_grid'](aff, theta, ctrl, T, in_size, out_size)
    assert _moved(mut, coarse, bar)
    if T > 1 and name != 'identity':                                           # (T = 1 and theta = 0 have no w_0 to lose)
        mut = wo.MUTATIONS['tps_without_w0']['coarse_grid'](aff, theta, ctrl, T, in_size, out_size)
        assert _moved(mut, coarse, bar)
    fbar = bar + wo.U * (np.abs(coarse) + np.abs(refine[..., :2]))
    assert _moved(wo.MUTATIONS['grid_clamp_dropped']['finish_grid'](coarse, refine), wo.finish_grid(coarse, refine), fbar)
    if name == 'scale1.3':                                                     # the coarse grid itself leaves [-1, 1]
        assert _moved(wo.MUTATIONS['grid_clamp_dropped']['finish_grid'](coarse), wo.finish_grid(coarse), bar)


def test_every_mutation_is_covered():
    assert set(wo.MUTATIONS) == {'align_corners_false', 'ne_sw_swapped', 'gate_strict', 'mask_wrong_pixel', 'border_padding',
                                 'tps_without_w0', 'linspace_not_symmetric', 'grid_clamp_dropped'}
    assert {k for f in wo.MUTATIONS.values() for k in f} == {'sample', 'adjoint', 'coarse_grid', 'finish_grid'}


# (camera, projector, scale, TILED_BOX_CAP, tiles, direct tiles, the other observations)
TILE_ROWS = [((64, 64), (49, 33), 1.3, None, 12, 3, dict(box_cap=576, longest=105, out_of_frame=1949)),
             ((36, 52), (17, 33), 1.3, None, 6, 2, {}),
             ((48, 40), (33, 33), 0.9, None, 9, 0, dict(empty=134)),
             ((48, 40), (33, 33), 0.9, 200, 9, 4, {})]


@pytest.mark.parametrize('cam,prj,scale,cap,tiles,direct,more', TILE_ROWS)
def test_tiled_taps_tables(monkeypatch, cam, prj, scale, cap, tiles, direct, more):
    """models.tiled_taps on CPU tensors: a 0.05 rad rotation, offset (+0.03, -0.02), the grid clamped to [-1, 1].  The clamped 1.3
    grids pile a border strip of camera pixels onto the projector's border pixels: tiles whose box exceeds TILED_BOX_CAP are marked
    direct (rows = -1) and their entries carry the camera pixel itself."""
    (hc, wc), (hp, wp) = cam, prj
    assert M.TILED_BOX_CAP == 576
    if cap is not None:
        monkeypatch.setattr(M, 'TILED_BOX_CAP', cap)
    grid = wo.affine_grid(cam, scale, True)
    src, wgt = wo.taps(grid, hp, wp)
    mask = wo.masks(cam)[1]
    off, order, wm = wo.transposed(src, wgt, mask, hp * wp)
    res = M.tiled_taps(torch.from_numpy(off), torch.from_numpy(order), torch.from_numpy(wm), prj, cam)
    assert res is not None
    lidx, w_e, tbox, box_cap = res
    lidx, w_e, tbox = lidx.numpy(), w_e.numpy(), tbox.numpy()
    is_direct = tbox[:, 2] < 0
    assert len(tbox) == tiles and int(is_direct.sum()) == direct
    assert 2 * int(is_direct.sum()) <= tiles                                   # (more than half: tiled_taps returns None)
    assert box_cap >= 1 and box_cap * 4 * 16 <= 64 * 1024 and box_cap <= M.TILED_BOX_CAP
    counts = np.diff(off)
    if 'box_cap' in more:
        assert box_cap == more['box_cap'] and counts.max() == more['longest'] and int((src == wo.SENTINEL).sum()) == more['out_of_frame']
    if 'empty' in more:
        assert int((counts == 0).sum()) == more['empty']
    n_ent = int(off[-1])
    assert len(lidx) == n_ent and len(w_e) == n_ent
    assert np.array_equal(w_e, wm[order[:n_ent]])                              # the weights (x mask) in entry order
    sp = np.repeat(np.arange(hp * wp), counts)
    ntx = (wp + wo.TS - 1) // wo.TS
    tile = (sp // wp // wo.TS) * ntx + (sp % wp) // wo.TS
    cpix = order[:n_ent] >> 2
    y0, x0, ch, cw = (tbox[tile, k] for k in range(4))
    d = is_direct[tile]
    assert np.array_equal(lidx[d], cpix[d])                                    # a direct tile: the raw camera pixel
    assert (lidx >= 0).all() and (lidx[d] < hc * wc).all()
    assert (lidx[~d] < (ch * cw)[~d]).all() and ((ch * cw)[~d] <= box_cap).all()
    assert np.array_equal(((y0 + lidx // np.maximum(cw, 1)) * wc + x0 + lidx % np.maximum(cw, 1))[~d], cpix[~d])   # inside the box
    boxed = tbox[~is_direct]
    assert (boxed[:, 0] >= 0).all() and (boxed[:, 1] >= 0).all() and (boxed[:, 0] + boxed[:, 2] <= hc).all() and \
        (boxed[:, 1] + boxed[:, 3] <= wc).all()


def test_tiled_taps_gives_up_when_most_tiles_are_direct(monkeypatch):
    """More than half the tiles direct: None (the untiled gather stays in charge); no entries at all: None."""
    cam, prj = (48, 40), (33, 33)
    grid = wo.affine_grid(cam, 0.9, True)
    src, wgt = wo.taps(grid, *prj)
    off, order, wm = wo.transposed(src, wgt, None, prj[0] * prj[1])
    monkeypatch.setattr(M, 'TILED_BOX_CAP', 1)
    assert M.tiled_taps(torch.from_numpy(off), torch.from_numpy(order), torch.from_numpy(wm), prj, cam) is None
    src, wgt = wo.taps(wo.affine_grid(cam, 5.0, False, offset=(9.0, 9.0)), *prj)
    off, order, wm = wo.transposed(src, wgt, None, prj[0] * prj[1])
    assert int(off[-1]) == 0
    assert M.tiled_taps(torch.from_numpy(off), torch.from_numpy(order), torch.from_numpy(wm), prj, cam) is None
