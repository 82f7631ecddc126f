"""GPU: the kernels of the SSIM stealth term (csrc/ssim_ops.hip) alone, through the C-ABI, against their float64 restatement
(tests/ssim_oracle.py): spaa_ssim_tiles, spaa_ssim_scene_stats, spaa_ssim_fwd, spaa_ssim_bwd (and spaa_ssim_value, the reduce of the
tile sums).

The tile is 16 rows x 32 columns (SPAA_SSIM_TILE_H x SPAA_SSIM_TILE_W).  Sizes (ssim_oracle.SIZES): 1 x 1 (every tap on one pixel),
3 x 5 (smaller than the radius: both edges feed one pixel), 11 x 11, 15 x 9 and 17 x 9 (just under / over a tile's height, the width
below a tile), 7 x 31 and 7 x 33 (the same across), 21 x 70 (2 x 3 tiles, ragged last tiles, halos across tile borders).  Contents
(ssim_oracle.KINDS): a flat bright image against a flat bright scene (the cancellation case), a textured pair, an image equal to its
scene (S = 1, zero gradient) and the textured pair with 0, -0.0 and 1 planted.  The pad channel of the images holds 7 and -3.

The bars are ssim_oracle.bars: running error bounds along the kernels' own sequence of operations, derived in that module's
docstring, none set from what a kernel produced; tests/test_ssim_cpu.py shows that each deliberate mistake of ssim_oracle.MUTATIONS
exceeds them.  Every test prints its largest error / bar (profiles/ssim_accuracy.txt holds the lines of one run)."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_oracle as so

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = so.U
HIP_INVALID_VALUE = 1
CASES = [(k, h, w) for k in so.KINDS for h, w in so.SIZES]
GSCALE = 1.0 / 96.0


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    w = so.taps()
    return dict(lib=_lib, p=_lib.ptr, tiles=_lib.load().spaa_ssim_tiles, taps=(ctypes.c_float * 11)(*w.tolist()))


def report(name, ratio):
    print(f'[ssim] {name}: max error / bar = {ratio:.4f}')


def run(hip, y, s, w_ps, g0=None, fill=None):
    """scene_stats, fwd, bwd and value on y, s [B][H][W][4] (CPU fp32) with weights w_ps; the outputs start as `fill` (a CPU tensor
    broadcast over every output) or 0 and g_y as g0.  Returns a dict of CPU tensors."""
    lib, p = hip['lib'], hip['p']
    B, H, W, _ = y.shape
    tiles = hip['tiles'](H, W)
    yd, sd, wd = y.to(DEV), s.to(DEV), torch.tensor(w_ps, dtype=torch.float32, device=DEV)

    def out(*shape):
        t = torch.zeros(*shape, device=DEV)
        if fill is not None:
            t.view(B, -1)[:] = fill.to(DEV).view(B, 1)
        return t

    mu2, e22 = torch.zeros(B, H, W, 4, device=DEV), torch.zeros(B, H, W, 4, device=DEV)
    m_mu, m_11, m_12, partial, val = out(B, H, W, 4), out(B, H, W, 4), out(B, H, W, 4), out(B, tiles), out(B)
    g = out(B, H, W, 4) if g0 is None else g0.to(DEV).clone()
    lib.call('spaa_ssim_scene_stats', p(sd), hip['taps'], p(mu2), p(e22), B, H, W)
    lib.call('spaa_ssim_fwd', p(yd), p(sd), p(mu2), p(e22), hip['taps'], p(wd), p(m_mu), p(m_11), p(m_12), p(partial), B, H, W)
    lib.call('spaa_ssim_bwd', p(yd), p(sd), p(m_mu), p(m_11), p(m_12), hip['taps'], p(wd), GSCALE, p(g), B, H, W)
    lib.call('spaa_ssim_value', p(partial), p(wd), tiles, H, W, p(val), B)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(mu2=mu2, e22=e22, m_mu=m_mu, m_11=m_11, m_12=m_12, partial=partial, ssim=val, g=g).items()}


def pair(kind, H, W, seed=0):
    y, s = so.inputs(kind, H, W, seed)
    return torch.from_numpy(y)[None], torch.from_numpy(s)[None]


@pytest.mark.parametrize('kind,H,W', CASES)
def test_kernels_against_the_restatement(hip, kind, H, W):
    y, s = pair(kind, H, W)
    g0 = torch.zeros(1, H, W, 4)
    g0[..., :3] = torch.linspace(-1e-3, 1e-3, H * W * 3).view(1, H, W, 3)      # g_y is accumulated into, not overwritten
    g0[..., 3] = 5.0
    r = run(hip, y, s, [1.0], g0=g0)
    yn, sn = y[0].numpy(), s[0].numpy()
    bar = so.bars(yn, sn)
    worst = 0.0
    # the scene's statistics
    m2, q22, b_m2, b_q22 = so.scene_stats(sn)
    for got, ref, b in ((r['mu2'], m2, b_m2), (r['e22'], q22, b_q22)):
        err = np.abs(got[0, ..., :3].double().numpy() - ref)
        assert (err <= b).all(), f'scene statistics: {(err / np.maximum(b, 1e-300)).max():.3f} of the bar'
        assert (got[0, ..., 3] == 0).all()
        worst = max(worst, (err[b > 0] / b[b > 0]).max() if (b > 0).any() else 0.0)
    # the three maps
    S, *ms = so.maps(yn, sn)
    for name, ref in zip(('m_mu', 'm_11', 'm_12'), ms):
        err = np.abs(r[name][0, ..., :3].double().numpy() - ref)
        assert (err <= bar[name]).all(), f'{name}: {(err / bar[name]).max():.3f} of the bar'
        assert (r[name][0, ..., 3] == 0).all()
        worst = max(worst, (err / bar[name]).max())
    # the tile sums of S and the value
    tiles_x = -(-W // so.TILE_W)
    for t in range(hip['tiles'](H, W)):
        ty, tx = divmod(t, tiles_x)
        sl = (slice(ty * so.TILE_H, (ty + 1) * so.TILE_H), slice(tx * so.TILE_W, (tx + 1) * so.TILE_W))
        b = bar['S'][sl].sum() + 15 * U * np.abs(S[sl]).sum()
        err = abs(float(r['partial'][0, t]) - S[sl].sum())
        assert err <= b, f'tile {t}: {err / b:.3f} of the bar'
        worst = max(worst, err / b)
    ev = abs(float(r['ssim'][0]) - so.ssim(yn, sn))
    assert ev <= bar['value'], f'SSIM: {ev / bar["value"]:.3f} of the bar'
    if kind == 'equal':
        assert abs(float(r['ssim'][0]) - 1.0) <= bar['value']
    # the gradient, added into g0: the bound of the unscaled gradient times the scale, the scale's and the product's rounding, and the
    # accumulation's
    gs = GSCALE * so.grad_sum(yn, sn)
    gfin = g0[0, ..., :3].double().numpy() + gs
    b = GSCALE * bar['grad_sum'] + 2 * U * np.abs(gs) + U * np.abs(gfin)
    err = np.abs(r['g'][0, ..., :3].double().numpy() - gfin)
    assert (err <= b).all(), f'gradient: {(err / b).max():.3f} of the bar'
    assert (r['g'][0, ..., 3] == 5.0).all()                                      # the pad channel is left alone
    report(f'{kind} {H}x{W}', max(worst, ev / bar['value'], (err / b).max()))


def test_weight_zero_sample_is_untouched_and_the_others_are_their_own_runs(hip):
    H, W = 21, 70
    ys, ss = zip(*(pair(k, H, W, seed) for seed, k in enumerate(('textured', 'planted', 'flat'))))
    y, s = torch.cat(ys), torch.cat(ss)
    fill = torch.tensor([0.0, float('nan'), 0.0])
    g0 = torch.zeros(3, H, W, 4)
    g0[1] = 1e30
    g0[1, ::2] = float('nan')
    fill[1] = float('nan')
    r = run(hip, y, s, [1.0, 0.0, 0.5], g0=g0, fill=fill)
    for name in ('m_mu', 'm_11', 'm_12', 'partial', 'ssim'):
        assert torch.isnan(r[name][1]).all(), f'{name}: the row of the weight-0 sample was written'
    assert torch.equal(r['g'][1].view(torch.int32), g0[1].view(torch.int32)), 'g_y of the weight-0 sample was written'
    r2 = run(hip, y, s, [1.0, 0.0, 0.5], g0=torch.full((3, H, W, 4), 1e30), fill=torch.full((3,), 1e30))
    for name in ('m_mu', 'm_11', 'm_12', 'partial', 'ssim'):
        assert (r2[name][1] == 1e30).all()
    for b, wgt in ((0, 1.0), (2, 0.5)):
        one = run(hip, y[b:b + 1], s[b:b + 1], [wgt])
        for name in ('mu2', 'e22', 'm_mu', 'm_11', 'm_12', 'partial', 'ssim', 'g'):
            assert torch.equal(one[name][0].view(torch.int32), r[name][b].view(torch.int32)), f'sample {b}: {name} differs from its own B = 1 run'
    # the weight scales the gradient and nothing else
    full = run(hip, y[2:3], s[2:3], [1.0])
    assert torch.equal(full['m_11'], run(hip, y[2:3], s[2:3], [0.5])['m_11'])
    assert torch.equal(full['g'] * 0.5, r['g'][2:3])                              # (a power of two: exact)
    report('weight 0 untouched, B = 3 against B = 1', 0.0)


def test_two_runs_are_bitwise_equal(hip):
    y, s = pair('planted', 21, 70)
    y, s = torch.cat([y, y.flip(1)]), torch.cat([s, s.flip(1)])
    a, b = run(hip, y, s, [1.0, 1.0]), run(hip, y, s, [1.0, 1.0])
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name
    report('two runs bitwise', 0.0)


def test_argument_checks_refuse_without_a_launch(hip):
    lib, p = hip['lib'].load(), hip['p']
    H, W, B = 5, 6, 2
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    img = [torch.full((B, H, W, 4), 3.0, device=DEV) for _ in range(9)]
    y, s, mu2, e22, m_mu, m_11, m_12, g, _ = img
    partial, w_ps, val = torch.full((B, 1), 3.0, device=DEV), torch.ones(B, device=DEV), torch.full((B,), 3.0, device=DEV)
    t = hip['taps']
    assert hip['tiles'](H, W) == 1 and hip['tiles'](0, W) == 0 and hip['tiles'](H, 0) == 0 and hip['tiles'](1 << 16, 1 << 15) == 0
    good = dict(stats=[p(s), t, p(mu2), p(e22), B, H, W], fwd=[p(y), p(s), p(mu2), p(e22), t, p(w_ps), p(m_mu), p(m_11), p(m_12), p(partial), B, H, W],
                bwd=[p(y), p(s), p(m_mu), p(m_11), p(m_12), t, p(w_ps), 1.0, p(g), B, H, W], value=[p(partial), p(w_ps), 1, H, W, p(val), B])
    fns = dict(stats=lib.spaa_ssim_scene_stats, fwd=lib.spaa_ssim_fwd, bwd=lib.spaa_ssim_bwd, value=lib.spaa_ssim_value)
    n = 0
    for name, args in good.items():
        bad = []
        for i, a in enumerate(args):
            if isinstance(a, ctypes.c_void_p) or a is t:            # every pointer in turn as NULL
                bad.append(args[:i] + [None] + args[i + 1:])
        sizes = [i for i, a in enumerate(args) if isinstance(a, int)]
        for i in sizes:                                             # every size in turn as 0 and as -1
            bad += [args[:i] + [v] + args[i + 1:] for v in (0, -1)]
        if name != 'value':
            bad.append(args[:-3] + [65536, H, W])                   # B beyond the grid's second dimension
            bad.append(args[:-3] + [B, 1 << 16, 1 << 15])           # H W beyond 2^30
        else:
            bad.append([p(partial), p(w_ps), 2, H, W, p(val), B])   # tiles that are not spaa_ssim_tiles(H, W)
        for a in bad:
            assert fns[name](*a, stream) == HIP_INVALID_VALUE, f'{name}{a}'
            n += 1
    torch.cuda.synchronize()
    for o in (mu2, e22, m_mu, m_11, m_12, g, partial, val):
        assert (o == 3.0).all(), 'a refused call has written'
    report(f'{n} refused calls', 0.0)
