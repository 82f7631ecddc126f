"""GPU: the kernels of csrc/warp.hip one by one, through direct calls of their C entry points, against the float64 restatement
(tests/warp_oracle.py): spaa_warp_taps, the two forward forms (spaa_warp_fwd with mask, clamp and cat8; spaa_warp_fwd_taps), the four
adjoint forms (spaa_warp_bwd after spaa_zero; spaa_warp_bwd_gather with a mask pointer, folded weights and g_xs / s;
spaa_warp_bwd_tiled, _sumsq and _sumsq_ps with and without gate bytes, boxed and direct tiles), the grid build
(spaa_warp_coarse_grid + spaa_warp_finish_grid), the layout conversions and the argument checks of all of them.

Shapes, batches and grids: warp_oracle.CASES.  Grid (a) is dyadic (every coordinate and weight exact in fp32: results bitwise), (b)
rotated and scaled by 0.9, (c) scaled by 1.3 and clamped (border strips pile onto border pixels: direct tiles), (d) unclamped out to
+-1.5 (pixels wholly off the frame).  Images hold 0.0, -0.0, 1.0 and their neighbours nextafter(0, -1) and nextafter(1, 2) for the
clamp and its gate; lanes no kernel reads hold nan and 1e30; every output is filled with a sentinel first and has one more image of
sentinels behind it, which must stay.

Every index table handed to a kernel comes from models.transposed_taps or models.tiled_taps and has its ranges asserted on the host
before the launch.

The bars are derived in warp_oracle's docstring (eps_c, bar_fwd, bar_bwd, eps_t, bar_grid), none is set from what a kernel produced;
tests/test_warp_cpu.py shows that each deliberate mistake of warp_oracle.MUTATIONS exceeds them.  Every test prints its largest
error / bar (profiles/warp_ops_accuracy.txt holds the lines of one run)."""
import numpy as np
import pytest
import torch

import warp_oracle as wo
from test_gpu_parity import hip  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = wo.U
FILL, IFILL = -7.0, -5
HIP_INVALID_VALUE = 1
GRAY = 0.5
IDS = [wo.case_id(c) for c in wo.CASES]
TILED_CASES = [c for c in wo.CASES if c[2] != 'a']          # (the planted dyadic grid is a wild warp: its boxes span the frame)
DIRECT_TILES = {((36, 52), (17, 33), 'c'): 2, ((64, 64), (49, 33), 'c'): 3}   # tests/test_warp_cpu.py::test_tiled_taps_tables


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _out(B, *shape, fill=FILL, dtype=torch.float32):
    """(full, out): `out` the first B images of a tensor of B + 1 images filled with the sentinel."""
    full = torch.full((B + 1,) + tuple(shape), fill, dtype=dtype, device=DEV)
    return full, full[:B]


def _guard(full, B, fill=FILL):
    """The image behind the output still holds the sentinel."""
    return bool((full[B:] == fill).all())


def _np(t):
    return t.cpu().numpy()


def _check_csr(off, order, wm, hwp, hwc):
    off, order = _np(off), _np(order)
    assert off.dtype == np.int32 and order.dtype == np.int32 and wm.dtype == torch.float32
    assert off.shape == (hwp + 1,) and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= 4 * hwc
    assert order.shape == (4 * hwc,) and (order >= 0).all() and (order < 4 * hwc).all() and wm.numel() == 4 * hwc
    assert len(np.unique(order)) == 4 * hwc


def _check_src(tap_src, hwp, hwc):
    s = _np(tap_src)
    assert s.dtype == np.int32 and s.shape == (4 * hwc,) and (((s >= 0) & (s < hwp)) | (s == wo.SENTINEL)).all()


def _check_tiled(off, tiled, prj, cam):
    """Every index of the tiled structure addresses its tile's LDS box, or the camera image for a direct tile."""
    (hp, wp), (hc, wc) = prj, cam
    lidx, w_e, tbox, box_cap = tiled
    off, lidx, tbox = _np(off), _np(lidx), _np(tbox)
    ntx, nty = (wp + wo.TS - 1) // wo.TS, (hp + wo.TS - 1) // wo.TS
    n_ent = int(off[-1])
    assert lidx.dtype == np.int32 and tbox.dtype == np.int32 and w_e.dtype == torch.float32
    assert lidx.shape == (n_ent,) and w_e.numel() == n_ent and tbox.shape == (ntx * nty, 4)
    assert 1 <= box_cap and box_cap * 4 * 16 <= 64 * 1024
    sp = np.repeat(np.arange(hp * wp), np.diff(off))
    tile = (sp // wp // wo.TS) * ntx + (sp % wp) // wo.TS
    direct = tbox[:, 2] < 0
    boxed = tbox[~direct]
    assert (boxed >= 0).all() and (boxed[:, 0] + boxed[:, 2] <= hc).all() and (boxed[:, 1] + boxed[:, 3] <= wc).all()
    assert (boxed[:, 2] * boxed[:, 3] <= box_cap).all()
    lim = np.where(direct, hc * wc, tbox[:, 2] * tbox[:, 3])[tile]
    assert (lidx >= 0).all() and (lidx < lim).all()
    return int(direct.sum())


def _tables(hip, grid_d, prj, cam, mask_d):
    """(off, order, wm, tap_src) of models.transposed_taps, range-checked."""
    off, order, wm, src = hip['models'].transposed_taps(grid_d, prj, cam, mask_d, want_table=True)
    _check_csr(off, order, wm, prj[0] * prj[1], cam[0] * cam[1])
    _check_src(src, prj[0] * prj[1], cam[0] * cam[1])
    return off, order, wm, src


# ---------------------------------------------------------------------------------------------------------------- spaa_warp_taps
def _taps(lib, grid, prj, cam):
    hwc = cam[0] * cam[1]
    src_full, src = _out(1, hwc, 4, fill=IFILL, dtype=torch.int32)
    wgt_full, wgt = _out(1, hwc, 4)
    grid_d = _d(grid)
    lib.call('spaa_warp_taps', lib.ptr(grid_d), prj[0], prj[1], cam[0], cam[1], lib.ptr(src), lib.ptr(wgt))
    assert _guard(src_full, 1, IFILL) and _guard(wgt_full, 1)
    return _np(src)[0], _np(wgt)[0]


@pytest.mark.parametrize('case', [c for c in wo.CASES if c[2] == 'a'], ids=lambda c: wo.case_id(c))
def test_taps_dyadic_grid_bitwise(hip, case):
    """Grid (a): indices and weights equal the restatement's bit for bit, the sentinel and weight 0 of the taps at x0 + 1 == W and
    y0 + 1 == H (gx = 1, gy = 1) included."""
    cam, prj, _, _ = case
    grid = wo.make_grid(case)
    src, wgt = _taps(hip['lib'], grid, prj, cam)
    ref_src, ref_wgt = wo.taps(grid, *prj)
    assert ((ref_src[:, 1] == wo.SENTINEL) & (ref_src[:, 0] != wo.SENTINEL)).any()      # x0 == W - 1: the east taps are outside
    assert ((ref_src[:, 2] == wo.SENTINEL) & (ref_src[:, 0] != wo.SENTINEL)).any()
    assert (ref_wgt == 1.0).any()                                                       # integer pixel centres
    assert np.array_equal(ref_wgt.astype(np.float32).astype(np.float64), ref_wgt)       # (exact in fp32)
    assert np.array_equal(src, ref_src)
    assert np.array_equal(wgt, ref_wgt.astype(np.float32))
    print(f'taps {wo.case_id(case)}: bitwise equal to float64')


@pytest.mark.parametrize('case', TILED_CASES, ids=lambda c: wo.case_id(c))
def test_taps_general_grids(hip, case):
    """Grids (b)-(d), stated so that a floor tie may fall either way: the in-frame indices of a pixel form one 2 x 2 block and the
    others lie outside the frame with the sentinel and weight exactly 0; where all four are inside, the weights sum to 1 within 4 u and
    sum w (x, y) is the float64 coordinate within eps_c; every weight is the float64 hat product within 2 eps_c + 4 u; a pixel with no
    tap inside has its float64 coordinate at least 1 - eps_c outside."""
    cam, (hp, wp), kind, _ = case
    grid = wo.make_grid(case)
    src, wgt = _taps(hip['lib'], grid, (hp, wp), cam)
    src, wgt = src.astype(np.int64), wgt.astype(np.float64)
    xs, ys = (a.reshape(-1) for a in wo.coords(grid, hp, wp))
    ec = wo.eps_c(grid, hp, wp)
    inside = src != wo.SENTINEL
    assert ((src[inside] >= 0) & (src[inside] < hp * wp)).all() and (wgt[~inside] == 0).all() and (wgt >= 0).all()
    dy, dx = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    y0 = np.where(inside, src // wp - dy, np.iinfo(np.int64).min).max(axis=1)
    x0 = np.where(inside, src % wp - dx, np.iinfo(np.int64).min).max(axis=1)
    some = inside.any(axis=1)
    yy, xx = y0[:, None] + dy, x0[:, None] + dx
    assert (np.where(inside, (src // wp == yy) & (src % wp == xx), True))[some].all()          # one block
    assert (inside == ((yy >= 0) & (yy < hp) & (xx >= 0) & (xx < wp)))[some].all()             # the others: outside the frame
    none = ~some
    assert (((xs <= -1 + ec) | (xs >= wp - ec) | (ys <= -1 + ec) | (ys >= hp - ec)))[none].all()
    if kind == 'd':
        assert none.any()
    full = inside.all(axis=1)
    assert full.any()
    r_sum = np.abs(wgt.sum(axis=1) - 1)[full].max() / (4 * U)
    r_c = max(np.abs((wgt * xx).sum(axis=1) - xs)[full].max(), np.abs((wgt * yy).sum(axis=1) - ys)[full].max()) / ec
    hat = np.maximum(0, 1 - np.abs(xs[:, None] - xx)) * np.maximum(0, 1 - np.abs(ys[:, None] - yy))
    r_w = np.abs(wgt - hat)[inside].max() / (2 * ec + 4 * U)
    print(f'taps {wo.case_id(case)}: |sum w - 1| / 4u = {r_sum:.3f}, |sum w (x, y) - float64| / eps_c = {r_c:.3f}, '
          f'|w - hat| / (2 eps_c + 4u) = {r_w:.3f}')
    assert r_sum <= 1 and r_c <= 1 and r_w <= 1


# ---------------------------------------------------------------------------------------------------------------- forward
def _cat8_of(xw, s):
    """(s, fl(xw * s), 0, 0) from the kernel's own xw: one fp32 product per channel."""
    out = np.zeros(xw.shape[:3] + (8,), dtype=np.float32)
    out[..., :3] = s[..., :3]
    out[..., 3:6] = xw[..., :3] * s[..., :3]
    return out


@pytest.mark.parametrize('case', wo.CASES, ids=IDS)
def test_forward_both_forms(hip, case):
    """spaa_warp_fwd (mask none / rectangle / fractional, clamp, cat8) and spaa_warp_fwd_taps against `sample` within bar_fwd, equal
    to it on grid (a); the pad lane is 0 whatever x's holds; cat8 is (s, fl(xw s), 0, 0) of the kernel's own xw; the two forms agree
    within 8 u V; every pixel of every image < B is written and the image behind stays.  The batches 1, 3, 5, 6 and 9 leave 1, 3,
    1, 2 and 1 images in the last group of four; spaa_warp_fwd_taps runs with 1, 2, 4, 10, 12, 16, 20, 30, 32 and 36 workgroups."""
    lib = hip['lib']
    cam, prj, kind, B = case
    (hc, wc), (hp, wp) = cam, prj
    d = wo.inputs(case)
    grid_d, x_d, s_d = _d(d['grid']), _d(d['x']), _d(d['s'])
    worst = worst_t = worst_2 = 0.0
    for mk in wo.MASK_KINDS:
        m = d['mask'][mk]
        m_d = None if m is None else _d(m)
        off, order, wm, src = _tables(hip, grid_d, prj, cam, m_d)
        for clamp in (0, 1):
            ref = wo.sample(d['x'], d['grid'], m, bool(clamp))
            bar = wo.bar_fwd(d['x'], d['grid'], bool(clamp))
            V = np.abs(np.clip(d['x'][..., :3], 0, 1) if clamp else d['x'][..., :3]).max()
            got = {}
            for cat in (False, True):
                xw_full, xw = _out(B, hc, wc, 4)
                c8_full, c8 = _out(B, hc, wc, 8)
                lib.call('spaa_warp_fwd', lib.ptr(x_d), lib.ptr(grid_d), lib.ptr(m_d), lib.ptr(s_d) if cat else None, lib.ptr(xw),
                         lib.ptr(c8) if cat else None, B, hp, wp, hc, wc, clamp)
                assert _guard(xw_full, B) and _guard(c8_full, B)
                got[cat] = _np(xw)
                assert np.isfinite(got[cat]).all() and (got[cat][..., 3] == 0).all()      # every pixel written, the pad lane 0
                if cat:
                    assert np.array_equal(_np(c8), _cat8_of(got[cat], d['s']))
                else:
                    assert (c8_full == FILL).all()
            assert np.array_equal(got[False], got[True])
            xt_full, xt = _out(B, hc, wc, 4)
            lib.call('spaa_warp_fwd_taps', lib.ptr(x_d), lib.ptr(src), lib.ptr(wm), lib.ptr(xt), B, hp, wp, hc, wc, clamp)
            assert _guard(xt_full, B)
            gt = _np(xt)
            assert np.isfinite(gt).all() and (gt[..., 3] == 0).all()
            if kind == 'a':
                assert np.array_equal(got[False], ref.astype(np.float32)) and np.array_equal(gt, ref.astype(np.float32))
            worst = max(worst, np.abs(got[False] - ref).max() / bar)
            worst_t = max(worst_t, np.abs(gt - ref).max() / bar)
            worst_2 = max(worst_2, np.abs(gt.astype(np.float64) - got[False]).max() / (8 * U * V))
    print(f'forward {wo.case_id(case)}: |fwd - float64| / bar_fwd = {worst:.3f}, |fwd_taps - float64| / bar_fwd = {worst_t:.3f}, '
          f'|fwd_taps - fwd| / (8 u V) = {worst_2:.3f}')
    assert worst <= 1 and worst_t <= 1
    assert worst_2 <= 1


# ---------------------------------------------------------------------------------------------------------------- adjoints
@pytest.mark.parametrize('case', wo.CASES, ids=IDS)
def test_adjoint_scatter_and_gather(hip, case):
    """spaa_warp_bwd (atomic scatter into a buffer cleared by spaa_zero) and spaa_warp_bwd_gather -- with a mask pointer and raw
    weights, with the mask folded into the weights, with and without g_xs / s -- against `adjoint` within bar_bwd(s).  The gather with
    a mask pointer equals the gather with folded weights bit for bit; projector pixels no camera pixel reaches are exactly 0; the
    gate passes x = 0, -0 and 1 and stops their outer neighbours; images >= B are never stored."""
    lib = hip['lib']
    cam, prj, kind, B = case
    (hc, wc), (hp, wp) = cam, prj
    d = wo.inputs(case)
    grid_d, x_d, s_d, g_d, gs_d = (_d(d[k]) for k in ('grid', 'x', 's', 'g', 'g_xs'))
    raw = _tables(hip, grid_d, prj, cam, None)
    worst = {'bwd': 0.0, 'gather': 0.0}
    for mk in wo.MASK_KINDS:
        m = d['mask'][mk]
        m_d = None if m is None else _d(m)
        folded = raw if m is None else _tables(hip, grid_d, prj, cam, m_d)
        for clamp in (0, 1):
            for with_s in (False, True):
                gs, s = (d['g_xs'], d['s']) if with_s else (None, None)
                ref = wo.adjoint(d['g'], gs, s, d['x'], d['grid'], m, bool(clamp))
                bar = wo.bar_bwd(d['g'], gs, s, m, d['grid'], hp, wp)
                gs_p, s_p = (lib.ptr(gs_d), lib.ptr(s_d)) if with_s else (None, None)

                def check(got, what):
                    assert np.isfinite(got).all() and (got[..., 3] == 0).all()
                    err = np.abs(got[..., :3] - ref[..., :3])
                    assert (got[..., :3][bar == 0] == 0).all()
                    worst[what] = max(worst[what], (err[bar > 0] / bar[bar > 0]).max())
                    assert (err <= bar).all(), (what, mk, clamp, with_s, (err[bar > 0] / bar[bar > 0]).max())

                full, gx = _out(B, hp, wp, 4)
                lib.call('spaa_zero', lib.ptr(gx), B * hp * wp * 16)
                assert (gx == 0).all() and _guard(full, B)
                lib.call('spaa_warp_bwd', lib.ptr(g_d), gs_p, lib.ptr(x_d), lib.ptr(grid_d), lib.ptr(m_d), s_p, lib.ptr(gx), B, hp, wp,
                         hc, wc, clamp)
                assert _guard(full, B)
                check(_np(gx), 'bwd')
                outs = []
                for (off, order, wm, _), mp in ((raw, lib.ptr(m_d)), (folded, None)):
                    full, gx = _out(B, hp, wp, 4)
                    lib.call('spaa_warp_bwd_gather', lib.ptr(g_d), gs_p, lib.ptr(x_d), mp, s_p, lib.ptr(off), lib.ptr(order),
                             lib.ptr(wm), lib.ptr(gx), B, hp, wp, hc, wc, clamp)
                    assert _guard(full, B)
                    outs.append(_np(gx))
                    check(outs[-1], 'gather')
                assert np.array_equal(outs[0], outs[1])
                empty = np.diff(_np(raw[0])).reshape(hp, wp) == 0
                assert (outs[1][:, empty] == 0).all()
                if clamp and not with_s and m is None:                      # the gate at the planted values
                    r, c0 = hp // 2, wp // 2 - 2
                    open_ = np.abs(wo.adjoint(d['g'], None, None, d['x'], d['grid'], None, False)[:, r, c0:c0 + 5, :3]) > bar[:, r, c0:c0 + 5]
                    assert open_.any()
                    for k, v in enumerate(wo.DYADIC_PLANT if kind == 'a' else wo.PLANTED):
                        passes = 0.0 <= np.float32(v) <= 1.0
                        assert ((outs[1][:, r, c0 + k, :3] != 0)[open_[:, k]] == passes).all(), v
                        assert passes or (outs[1][:, r, c0 + k, :3] == 0).all(), v
    print(f'adjoint {wo.case_id(case)}: |bwd - float64| / bar_bwd = {worst["bwd"]:.3f}, |gather - float64| / bar_bwd = '
          f'{worst["gather"]:.3f}')


def _gate_bytes(x):
    """One byte per pixel: bit c = (0 <= x_c <= 1), as the step kernel writes them."""
    ok = (x[..., :3] >= 0) & (x[..., :3] <= 1)
    return (ok[..., 0] * 1 + ok[..., 1] * 2 + ok[..., 2] * 4).astype(np.uint8)


def _tiled_call(lib, name, g_d, x_d, off, tiled, B, prj, cam, clamp, extra=(), partial_tiles=0):
    (hp, wp), (hc, wc) = prj, cam
    lidx, w_e, tbox, box_cap = tiled
    full, gx = _out(B, hp, wp, 4)
    args = [lib.ptr(g_d), lib.ptr(x_d), lib.ptr(off), lib.ptr(lidx), lib.ptr(w_e), lib.ptr(tbox), box_cap, lib.ptr(gx), B, hp, wp, hc,
            wc, clamp]
    ps_full = ps = None
    if partial_tiles:
        ps_full, ps = _out(B, partial_tiles)
        gray, scale, state, bits = extra
        args += [gray, scale, state, lib.ptr(ps), bits]
    lib.call(name, *args)
    assert _guard(full, B) and (ps_full is None or _guard(ps_full, B))
    return _np(gx), (None if ps is None else _np(ps))


def _tile_sums(gx, prj):
    """float64 [B][tiles]: sum of gx^2 over the three channels per 16 x 16 tile, and the number of addends per tile."""
    hp, wp = prj
    B = gx.shape[0]
    ntx, nty = (wp + wo.TS - 1) // wo.TS, (hp + wo.TS - 1) // wo.TS
    sq = (gx[..., :3].astype(np.float64) ** 2).sum(axis=-1)
    sums, n = np.zeros((B, ntx * nty)), np.zeros(ntx * nty)
    for ty in range(nty):
        for tx in range(ntx):
            blk = sq[:, ty * wo.TS:(ty + 1) * wo.TS, tx * wo.TS:(tx + 1) * wo.TS]
            sums[:, ty * ntx + tx] = blk.reshape(B, -1).sum(axis=1)
            n[ty * ntx + tx] = 3 * blk.shape[1] * blk.shape[2]
    return sums, n


@pytest.mark.parametrize('case', TILED_CASES, ids=lambda c: wo.case_id(c))
def test_adjoint_tiled_and_fused(hip, case):
    """spaa_warp_bwd_tiled equals spaa_warp_bwd_gather bit for bit and `adjoint` within bar_bwd; spaa_warp_bwd_tiled_sumsq and
    _sumsq_ps (the gate from x and from gate bytes, scale 0 and 0.3, per-image scales with zeros, a state with both values, one pixel
    equal to gray) against adjoint + prjl2_and_sumsq within bar_bwd + 8 u scale; scale 0 leaves the tiled result bit for bit; the
    partial sums against the float64 sum of the kernel's own g_x^2 per tile within (n + 2) u sum, n the addends, and equal over two
    runs.  The clamped 1.3 grids bring their direct tiles (asserted)."""
    lib, M = hip['lib'], hip['models']
    cam, prj, kind, B = case
    (hc, wc), (hp, wp) = cam, prj
    d = wo.inputs(case)
    x = d['x'].copy()
    x[:, hp // 2 + 1, wp // 2, :3] = GRAY                                      # norm 0: no prjl2 gradient there
    grid_d, x_d, g_d = _d(d['grid']), _d(x), _d(d['g'])
    bits_d = _d(_gate_bytes(x).reshape(B, hp * wp))
    state = np.zeros((B, 4), dtype=np.int32)
    state[::2, 1] = 1                                                          # images 0, 2, ..: on the colour step
    state[:, 0], state[:, 2] = 3, -1
    state_d = _d(state)
    scales = np.where(np.arange(B) % 3 == 1, 0.0, 0.3 + 0.1 * np.arange(B)).astype(np.float32)
    scales_d = _d(scales)
    ntiles = ((wp + wo.TS - 1) // wo.TS) * ((hp + wo.TS - 1) // wo.TS)
    worst = worst_f = worst_p = 0.0
    for mk in wo.MASK_KINDS:
        m = d['mask'][mk]
        off, order, wm, _ = _tables(hip, grid_d, prj, cam, None if m is None else _d(m))
        tiled = M.tiled_taps(off, order, wm, prj, cam)
        assert tiled is not None
        n_direct = _check_tiled(off, tiled, prj, cam)
        if (cam, prj, kind) in DIRECT_TILES and m is None:
            assert n_direct == DIRECT_TILES[(cam, prj, kind)]
        for clamp in (0, 1):
            ref = wo.adjoint(d['g'], None, None, x, d['grid'], m, bool(clamp))
            bar = wo.bar_bwd(d['g'], None, None, m, d['grid'], hp, wp)
            full, gg = _out(B, hp, wp, 4)
            lib.call('spaa_warp_bwd_gather', lib.ptr(g_d), None, lib.ptr(x_d), None, None, lib.ptr(off), lib.ptr(order), lib.ptr(wm),
                     lib.ptr(gg), B, hp, wp, hc, wc, clamp)
            gt, _ = _tiled_call(lib, 'spaa_warp_bwd_tiled', g_d, x_d, off, tiled, B, prj, cam, clamp)
            assert np.array_equal(gt, _np(gg))
            assert (gt[..., 3] == 0).all() and (gt[..., :3][bar == 0] == 0).all()
            err = np.abs(gt[..., :3] - ref[..., :3])
            worst = max(worst, (err[bar > 0] / bar[bar > 0]).max())
            assert (err <= bar).all()
            for bits in ((None, lib.ptr(bits_d)) if clamp else (None,)):
                for name, scale_arg, scale in (('spaa_warp_bwd_tiled_sumsq', 0.0, np.zeros(B)),
                                               ('spaa_warp_bwd_tiled_sumsq', 0.3, np.full(B, np.float32(0.3), dtype=np.float64)),
                                               ('spaa_warp_bwd_tiled_sumsq_ps', lib.ptr(scales_d), scales.astype(np.float64))):
                    extra = (GRAY, scale_arg, lib.ptr(state_d), bits)
                    gf, ps = _tiled_call(lib, name, g_d, x_d, off, tiled, B, prj, cam, clamp, extra, ntiles)
                    gf2, ps2 = _tiled_call(lib, name, g_d, x_d, off, tiled, B, prj, cam, clamp, extra, ntiles)
                    assert np.array_equal(gf, gf2) and np.array_equal(ps, ps2)             # two runs: bitwise
                    assert (gf[..., 3] == 0).all()
                    if not scale.any():
                        assert np.array_equal(gf, gt)
                    want, _ = wo.prjl2_and_sumsq(ref, x, GRAY, scale, state)
                    applies = (scale != 0) & (state[:, 1] != 0)
                    fbar = bar + (8 * U * scale * applies)[:, None, None, None]
                    errf = np.abs(gf[..., :3] - want[..., :3])
                    assert np.array_equal(gf[~applies], gt[~applies])                      # scale 0 or state 0: no term
                    assert np.array_equal(gf[:, hp // 2 + 1, wp // 2], gt[:, hp // 2 + 1, wp // 2])   # the pixel equal to gray
                    if applies.any():
                        assert not np.array_equal(gf[applies], gt[applies])
                    worst_f = max(worst_f, (errf[fbar > 0] / fbar[fbar > 0]).max())
                    assert (errf <= fbar).all(), (name, mk, clamp, scale_arg)
                    sums, n = _tile_sums(gf, prj)
                    errp = np.abs(ps.astype(np.float64) - sums)
                    pbar = (n + 2) * U * sums
                    assert (errp <= pbar).all(), (name, mk, clamp)
                    worst_p = max(worst_p, (errp[pbar > 0] / pbar[pbar > 0]).max())
    print(f'tiled {wo.case_id(case)}: |tiled - float64| / bar_bwd = {worst:.3f}, |fused - float64| / (bar_bwd + 8 u scale) = '
          f'{worst_f:.3f}, |partial - sum g_x^2| / ((n + 2) u sum) = {worst_p:.3f}')


def test_direct_tiles_equal_boxed_tiles(hip, monkeypatch):
    """(48, 40) -> (33, 33) at 0.9: no tile is direct; with TILED_BOX_CAP patched to 200 four of nine are.  The plain and the fused
    tiled adjoint give the same bits either way."""
    lib, M = hip['lib'], hip['models']
    case = ((48, 40), (33, 33), 'b', 9)
    cam, prj, _, B = case
    d = wo.inputs(case)
    grid_d, x_d, g_d = _d(d['grid']), _d(d['x']), _d(d['g'])
    state_d = _d(np.tile(np.array([[0, 1, 0, 0]], dtype=np.int32), (B, 1)))
    off, order, wm, _ = _tables(hip, grid_d, prj, cam, _d(d['mask']['frac']))
    boxed = M.tiled_taps(off, order, wm, prj, cam)
    monkeypatch.setattr(M, 'TILED_BOX_CAP', 200)
    direct = M.tiled_taps(off, order, wm, prj, cam)
    assert boxed is not None and direct is not None
    assert _check_tiled(off, boxed, prj, cam) == 0 and not bool((boxed[2][:, 2] < 0).any())
    assert _check_tiled(off, direct, prj, cam) == 4 and bool((direct[2][:, 2] < 0).any())
    ntiles = 9
    for clamp in (0, 1):
        a, _ = _tiled_call(lib, 'spaa_warp_bwd_tiled', g_d, x_d, off, boxed, B, prj, cam, clamp)
        b, _ = _tiled_call(lib, 'spaa_warp_bwd_tiled', g_d, x_d, off, direct, B, prj, cam, clamp)
        assert np.array_equal(a, b) and np.abs(a[..., :3]).max() > 0
        extra = (GRAY, 0.3, lib.ptr(state_d), None)
        a, pa = _tiled_call(lib, 'spaa_warp_bwd_tiled_sumsq', g_d, x_d, off, boxed, B, prj, cam, clamp, extra, ntiles)
        b, pb = _tiled_call(lib, 'spaa_warp_bwd_tiled_sumsq', g_d, x_d, off, direct, B, prj, cam, clamp, extra, ntiles)
        assert np.array_equal(a, b) and np.array_equal(pa, pb)


# ---------------------------------------------------------------------------------------------------------------- grid build
@pytest.mark.parametrize('sizes', wo.GRID_SIZES, ids=lambda s: f'{s[0][0]}x{s[0][1]}')
@pytest.mark.parametrize('T', wo.GRID_T)
@pytest.mark.parametrize('name', [p[0] for p in wo.GRID_PARAMS])
def test_grid_build(hip, name, T, sizes):
    """spaa_warp_coarse_grid against `coarse_grid` within bar_grid (T = 1, 2 and 36 control points; identity, rotated and 1.3-scaled
    affine, where the sampled field fades to zero outside the frame); spaa_warp_finish_grid with refine = NULL and with a planted
    refine that pushes values across +-1: against `finish_grid` within bar_grid + u (|coarse| + |refine|), and bit for bit
    clip(fl(refine + coarse)) of the kernel's own coarse grid.  Lanes 2 and 3 are written 0."""
    lib = hip['lib']
    out_size, in_size = sizes
    (ho, wo_), (hi, wi) = out_size, in_size
    aff, theta, ctrl, refine = wo.grid_inputs(name, T, out_size)
    c_full, coarse = _out(1, ho, wo_, 4)
    aff_d, theta_d, ctrl_d, refine_d = _d(aff), _d(theta), _d(ctrl), _d(refine)
    lib.call('spaa_warp_coarse_grid', lib.ptr(aff_d), lib.ptr(theta_d), lib.ptr(ctrl_d), T, hi, wi, ho, wo_, lib.ptr(coarse))
    assert _guard(c_full, 1)
    got = _np(coarse)[0]
    assert np.isfinite(got).all() and (got[..., 2:] == 0).all()
    ref = wo.coarse_grid(aff, theta, ctrl, T, in_size, out_size)
    bar = wo.bar_grid(aff, theta, ctrl, T, in_size, out_size)
    r_c = (np.abs(got[..., :2] - ref) / bar).max()
    worst_f = 0.0
    for r in (None, refine):
        f_full, fine = _out(1, ho, wo_, 4)
        lib.call('spaa_warp_finish_grid', lib.ptr(coarse), None if r is None else lib.ptr(refine_d), lib.ptr(fine), ho * wo_)
        assert _guard(f_full, 1)
        gf = _np(fine)[0]
        assert (gf[..., 2:] == 0).all()
        own = got[..., :2] if r is None else r[..., :2] + got[..., :2]                       # fp32: one rounding
        assert np.array_equal(gf[..., :2], np.clip(own, np.float32(-1), np.float32(1)))
        fbar = bar + (0 if r is None else U * (np.abs(ref) + np.abs(r[..., :2])))
        worst_f = max(worst_f, (np.abs(gf[..., :2] - wo.finish_grid(ref, r)) / fbar).max())
        if r is not None:
            assert (gf[..., :2] == 1).any() and (gf[..., :2] == -1).any() and (np.abs(gf[..., :2]) < 1).any()
    if name == 'scale1.3':
        assert (np.abs(ref) > 1).any()                                          # the coarse grid itself leaves [-1, 1]
    print(f'grid {name} T={T} {ho}x{wo_}<-{hi}x{wi}: |coarse - float64| / bar_grid = {r_c:.3f}, |fine - float64| / bar = {worst_f:.3f}')
    assert r_c <= 1 and worst_f <= 1


# ---------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize('B,H,W', [(1, 5, 7), (3, 16, 17), (5, 36, 52), (9, 4, 6)])
def test_layout_conversions_bitwise(hip, B, H, W):
    """spaa_nchw_to_nhwc4 and spaa_nhwc4_to_nchw against numpy, bit for bit (by value under the clamp, where the sign of a zero is
    free), clamp 0 and 1, with -0.0, 0, 1 and their neighbours planted; B H W of 35, 816, 9360 and 216: no multiple of 256; the pad lane
    is written 0; the round trip is the identity."""
    lib = hip['lib']
    assert (B * H * W) % 256 != 0
    x4 = wo.image(B, H, W, B + H)                                              # NHWC4 with garbage in lane 3
    nchw = np.ascontiguousarray(x4[..., :3].transpose(0, 3, 1, 2))
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)                    # noqa: E731
    nchw_d, x4_d = _d(nchw), _d(x4)
    assert (bits(nchw) == np.int32(-2 ** 31)).any()                            # a -0.0 is in
    for clamp in (0, 1):
        full, out4 = _out(B, H, W, 4)
        lib.call('spaa_nchw_to_nhwc4', lib.ptr(nchw_d), lib.ptr(out4), B, H, W, clamp)
        assert _guard(full, B)
        got4 = _np(out4)
        assert (bits(got4[..., 3]) == 0).all()
        full, out3 = _out(B, 3, H, W)
        lib.call('spaa_nhwc4_to_nchw', lib.ptr(x4_d), lib.ptr(out3), B, H, W, clamp)
        assert _guard(full, B)
        got3 = _np(out3)
        if clamp:
            assert np.array_equal(got4[..., :3], np.clip(x4[..., :3], 0, 1)) and np.array_equal(got3, np.clip(nchw, 0, 1))
            assert got4[..., :3].min() == 0 and got4[..., :3].max() == 1
        else:
            assert np.array_equal(bits(got4[..., :3]), bits(x4[..., :3])) and np.array_equal(bits(got3), bits(nchw))
            full, back = _out(B, 3, H, W)
            lib.call('spaa_nhwc4_to_nchw', lib.ptr(out4), lib.ptr(back), B, H, W, 0)
            assert _guard(full, B) and np.array_equal(bits(_np(back)), bits(nchw))


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_invalid_arguments(hip):
    """Every entry point of warp.hip: NULL for each required pointer, 0 for each size, cat8 or g_xs without s, box_cap < 1 and
    box_cap * 64 > 64 KiB, partial_ss / state / scales missing in the fused forms, a NULL or a negative length for spaa_zero: each
    call returns hipErrorInvalidValue and launches nothing (all outputs keep their sentinels).  The same argument lists, unchanged,
    return 0 first, so that it is the changed argument that is refused."""
    lib, M = hip['lib'], hip['models']
    raw = lib.load()
    p, stream = lib.ptr, lib._stream()
    case = ((5, 7), (4, 6), 'b', 1)
    cam, prj, _, _ = case
    (hc, wc), (hp, wp), B = cam, prj, 3
    d = wo.inputs((cam, prj, 'b', B))
    grid, x, s, g, gs = (_d(d[k]) for k in ('grid', 'x', 's', 'g', 'g_xs'))
    off, order, wm, src = _tables(hip, grid, prj, cam, None)
    tiled = M.tiled_taps(off, order, wm, prj, cam)
    assert tiled is not None and _check_tiled(off, tiled, prj, cam) == 0
    lidx, w_e, tbox, cap = tiled
    aff, theta, ctrl, _ = (_d(a) for a in wo.grid_inputs('rot0.9', 2, cam))
    state = _d(np.tile(np.array([[0, 1, 0, 0]], dtype=np.int32), (B, 1)))
    scales = _d(np.full(B, 0.3, dtype=np.float32))
    nchw = _d(np.zeros((B, 3, hp, wp), dtype=np.float32))
    of = [torch.full((B, max(hc * wc, hp * wp), 8), FILL, device=DEV) for _ in range(3)]      # float outputs, large enough for each
    oi = torch.full((hc * wc * 4,), IFILL, dtype=torch.int32, device=DEV)
    o0, o1, o2 = (p(t) for t in of)
    t_args = [p(g), p(x), p(off), p(lidx), p(w_e), p(tbox), cap, o0, B, hp, wp, hc, wc, 1]
    # name -> (arguments, indices of the required pointers, indices of the sizes, further refused argument lists as {index: value})
    table = {
        'spaa_warp_coarse_grid': ([p(aff), p(theta), p(ctrl), 2, hp, wp, hc, wc, o0], (0, 1, 2, 8), (3, 4, 5, 6, 7), []),
        'spaa_warp_finish_grid': ([p(grid), None, o0, hc * wc], (0, 2), (3,), []),
        'spaa_warp_fwd': ([p(x), p(grid), None, p(s), o0, o1, B, hp, wp, hc, wc, 1], (0, 1, 4), (6, 7, 8, 9, 10), [{3: None}]),
        'spaa_warp_bwd': ([p(g), p(gs), p(x), p(grid), None, p(s), o0, B, hp, wp, hc, wc, 1], (0, 2, 3, 6), (7, 8, 9, 10, 11),
                          [{5: None}]),
        'spaa_warp_taps': ([p(grid), hp, wp, hc, wc, p(oi), o0], (0, 5, 6), (1, 2, 3, 4), []),
        'spaa_warp_bwd_gather': ([p(g), p(gs), p(x), None, p(s), p(off), p(order), p(wm), o0, B, hp, wp, hc, wc, 1],
                                 (0, 2, 5, 6, 7, 8), (9, 10, 11, 12, 13), [{4: None}]),
        'spaa_warp_bwd_tiled': (t_args, (0, 1, 2, 3, 4, 5, 7), (6, 8, 9, 10, 11, 12), [{6: -1}, {6: 1025}]),
        'spaa_warp_bwd_tiled_sumsq': (t_args + [GRAY, 0.3, p(state), o1, None], (0, 1, 2, 3, 4, 5, 7, 17), (6, 8, 9, 10, 11, 12),
                                      [{6: -1}, {6: 1025}, {16: None}]),
        'spaa_warp_bwd_tiled_sumsq_ps': (t_args + [GRAY, p(scales), p(state), o1, None], (0, 1, 2, 3, 4, 5, 7, 15, 16, 17),
                                         (6, 8, 9, 10, 11, 12), [{6: -1}, {6: 1025}]),
        'spaa_warp_fwd_taps': ([p(x), p(src), p(wm), o0, B, hp, wp, hc, wc, 1], (0, 1, 2, 3), (4, 5, 6, 7, 8), []),
        'spaa_nchw_to_nhwc4': ([p(nchw), o0, B, hp, wp, 1], (0, 1), (2, 3, 4), []),
        'spaa_nhwc4_to_nchw': ([p(x), o0, B, hp, wp, 1], (0, 1), (2, 3, 4), []),
        'spaa_zero': ([o2, 64], (0,), (), [{1: -1}]),
    }
    assert 1025 * 4 * 16 > 64 * 1024 >= 1024 * 4 * 16
    assert len(table) == 13                                                    # warp.hip's entry points but spaa_version
    calls = 0
    for name, (args, ptrs, sizes, more) in table.items():
        fn = getattr(raw, name)
        assert fn(*args, stream) == 0, name
        torch.cuda.synchronize()
        for t in of:
            t.fill_(FILL)
        oi.fill_(IFILL)
        bad = [{i: None} for i in ptrs] + [{i: 0} for i in sizes] + more
        for change in bad:
            a = list(args)
            for i, v in change.items():
                a[i] = v
            assert fn(*a, stream) == HIP_INVALID_VALUE, (name, change)
            calls += 1
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in of) and bool((oi == IFILL).all())
    print(f'invalid arguments: {calls} refused calls over {len(table)} entry points')
