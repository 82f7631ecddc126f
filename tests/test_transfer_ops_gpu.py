"""GPU: the kernels of the transferable step (csrc/transfer_ops.hip) alone, through the C-ABI, against their float64 restatement
(tests/transfer_oracle.py): spaa_transfer_blur and spaa_transfer_momentum on planted gradient images.

Shapes: (3, 3) is smaller than the halo, (5, 7) and (17, 19) are ragged in one tile and in four, (33, 40) has three rows of tiles and a
second, 8-pixel-wide column of them, (64, 64) is the tile-aligned one with 16 chunks of 256 pixels; each with the radii 0, 1, 3 and 7.
B = 3 with the state rows adversarial / colour / adversarial, and one case of B = 70.  Sample 0 is a random gradient with NaN and 1e30
in its pad channel; the last sample is, in turn, random, all zero (n1 = 0) or an impulse in the top right corner.

Tolerances are derived in tests/transfer_oracle.py, not measured (U = 2^-24):
  * t:   |t - t_64| <= 4 (2 r + 1) U (K (*) |g|) per element;
  * n1:  the sum of partial_l1 against the float64 sum of the kernel's OWN |t|, relative CHAIN_L1 U = 15 U: the longest chain of additions
         behind it is 5 (a thread's six values) + 6 (shuffle tree) + 3 (wave sums) + 1 (the tiles' double sum, rounded once);
  * ss:  the sum of partial_ss against the float64 ||m||^2 of the kernel's OWN m, relative chain_ss U with
         chain_ss = 1 + 3 ceil(chunks / npartial) + 9 (a thread's squares and additions per chunk, then the block sum): 13 when every
         chunk has its block, 58 for the 16 chunks of (64, 64) behind one block;
  * m:   |m - m_64| <= (bound of t) / n1 + 3 U |m_64| per element."""
import ctypes

import pytest
import torch

import transfer_oracle as to

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(3, 3), (5, 7), (17, 19), (33, 40), (64, 64)]
SIGMA = {0: 0.0, 1: 1 / 3, 3: 1.0, 7: 7 / 3}
CASES = [(hw, r, ('random', 'zero', 'impulse')[(i + j) % 3]) for i, hw in enumerate(SHAPES) for j, r in enumerate(SIGMA)]
SENTINEL = 123.0


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    from spaa_amd import projector_based_attack as A
    return dict(lib=_lib, A=A, tiles=_lib.load().spaa_transfer_tiles)


def gradient(kind, H, W, gen):
    g = torch.zeros(H, W, 4)
    if kind == 'random':
        g[..., :3] = torch.randn(H, W, 3, generator=gen) * 1e-3
    elif kind == 'impulse':
        g[0, W - 1, :3] = torch.tensor([2.0, -1.0, 0.5])
    return g


def planted(B, H, W, last, seed):
    """g [B,H,W,4] fp32 (CPU), state [B,4] int32: sample b is on the colour step when b % 3 == 1."""
    gen = torch.Generator().manual_seed(seed)
    kinds = ['random'] * B
    kinds[B - 1] = last
    if B > 3:
        kinds[3], kinds[6] = 'zero', 'impulse'
    g = torch.stack([gradient(k, H, W, gen) for k in kinds])
    g[0, ..., 3] = float('nan')                                     # the pad channel of g is never used
    g[0, 0, 0, 3] = 1e30
    state = torch.randint(0, 5, (B, 4), generator=gen, dtype=torch.int32)
    state[:, 1] = torch.tensor([3 if b % 3 == 1 else 0 for b in range(B)], dtype=torch.int32)
    m0 = torch.randn(B, H, W, 4, generator=gen) * 1e-4
    return g, state, m0, kinds


def taps_of(A, r, mu):
    tr = A.Transfer(mu, SIGMA[r])
    assert tr.radius == r
    w = tr.weights()
    return w, (ctypes.c_float * w.numel())(*w.tolist())


def run_blur(hip, g, state, ctaps, r):
    lib, p = hip['lib'], hip['lib'].ptr
    B, H, W, _ = g.shape
    tiles = hip['tiles'](H, W)
    t = torch.full((B, H, W, 4), SENTINEL, device=DEV)
    l1 = torch.full((B, tiles), SENTINEL, device=DEV)
    lib.call('spaa_transfer_blur', p(g), p(state), ctaps, r, p(t), p(l1), B, H, W)
    return t, l1


def run_momentum(hip, t, l1, mu, state, m0, g, ss0, npartial):
    lib, p = hip['lib'], hip['lib'].ptr
    B, H, W, _ = t.shape
    m, g, ss = m0.clone(), g.clone(), ss0.clone()
    lib.call('spaa_transfer_momentum', p(t), p(l1), l1.shape[1], float(mu), p(state), p(m), p(g), p(ss), npartial, B, H * W)
    return m, g, ss


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_case(hip, B, H, W, r, last, mu):
    w, ctaps = taps_of(hip['A'], r, mu)
    g_cpu, state_cpu, m0_cpu, kinds = planted(B, H, W, last, seed=H * 100 + W + r)
    g, state, m0 = g_cpu.to(DEV), state_cpu.to(DEV), m0_cpu.to(DEV)
    col = state_cpu[:, 1] != 0
    adv = ~col
    assert adv.any() and col.any()
    ref = to.step(g_cpu.double(), m0_cpu.double(), col, w.double(), mu)

    # ---- the blur
    t, l1 = run_blur(hip, g, state, ctaps, r)
    assert same_bits(g, g_cpu.to(DEV))                                               # not in place
    t_cpu, l1_cpu = t.cpu(), l1.cpu()
    assert (t_cpu[col] == SENTINEL).all() and (l1_cpu[col] == SENTINEL).all()      # a colour row is not written
    assert (t_cpu[adv][..., 3] == 0).all()
    err_t = (t_cpu.double() - ref['t'])[adv][..., :3].abs()
    tol_t = ref['e_t'][adv][..., :3]
    print(f'{(H, W)} r={r} B={B}: |t - t_64| / bound, worst element {float((err_t / tol_t.clamp_min(1e-300)).max()):.3f}')
    assert (err_t <= tol_t).all()
    if r == 0:
        assert same_bits(t[adv][..., :3], g[adv][..., :3])                           # one tap of 1.0: the identity
    own_n1 = t_cpu.double()[..., :3].abs().sum(dim=(1, 2, 3))
    n1 = l1_cpu.double().sum(dim=1)
    print(f'   n1 relative error / U {((n1 - own_n1).abs() / own_n1.clamp_min(1e-300))[adv].max() / to.U:.3f} (bound {to.CHAIN_L1})')
    assert ((n1 - own_n1).abs() <= to.CHAIN_L1 * to.U * own_n1)[adv].all()
    assert ((n1 - ref['n1']).abs() <= to.CHAIN_L1 * to.U * own_n1 + ref['e_t'][..., :3].sum(dim=(1, 2, 3)))[adv].all()
    zero_rows = [b for b in range(B) if kinds[b] == 'zero' and adv[b]]
    assert all(float(n1[b]) == 0.0 for b in zero_rows)

    # ---- the momentum, with as many partial sums as chunks (the loop's), fewer and more
    chunks = (H * W + 255) // 256
    results = {}
    for npartial in sorted({chunks, 1, max(1, chunks // 3), chunks + 2}):
        ss0 = torch.full((B, npartial), SENTINEL, device=DEV)
        m, g_out, ss = run_momentum(hip, t, l1, mu, state, m0, g, ss0, npartial)
        results[npartial] = (m, g_out, ss)
        assert same_bits(m[col], m0[col]) and same_bits(g_out[col], g[col]) and (ss[col] == SENTINEL).all()
        assert same_bits(g_out[adv], m[adv]) and (m[adv][..., 3] == 0).all()
        m_cpu = m.cpu().double()
        err_m = (m_cpu - ref['m'])[adv][..., :3].abs()
        tol_m = ref['e_m'][adv][..., :3]
        assert (err_m <= tol_m).all(), f'npartial={npartial}: worst {float((err_m / tol_m.clamp_min(1e-300)).max()):.3f} of the bound'
        own_ss = m_cpu[..., :3].pow(2).sum(dim=(1, 2, 3))
        got_ss = ss.cpu().double().sum(dim=1)
        chain = to.chain_ss(H * W, npartial)
        assert ((got_ss - own_ss).abs() <= chain * to.U * own_ss)[adv].all(), f'npartial={npartial}'
        if npartial > chunks:
            assert (ss.cpu()[adv][:, chunks:] == 0).all()                            # the row is written in full
        for b in zero_rows:                                                          # n1 = 0: the momentum only decays
            assert same_bits(m[b][..., :3], (m0[b][..., :3] * torch.tensor(mu, dtype=torch.float32)))
    first = results[chunks]
    assert all(same_bits(res[0], first[0]) for res in results.values())              # m does not depend on the split of the sums
    print(f'   |m - m_64| / bound, worst element {float(((first[0].cpu().double() - ref["m"])[adv][..., :3].abs() / ref["e_m"][adv][..., :3].clamp_min(1e-300)).max()):.3f}')

    # ---- two runs are bit-identical
    t2, l12 = run_blur(hip, g, state, ctaps, r)
    m2, g2, ss2 = run_momentum(hip, t2, l12, mu, state, m0, g, torch.full((B, chunks), SENTINEL, device=DEV), chunks)
    assert same_bits(t2, t) and same_bits(l12, l1) and same_bits(m2, first[0]) and same_bits(g2, first[1]) and same_bits(ss2, first[2])


@pytest.mark.parametrize('hw,r,last', CASES, ids=[f'{hw[0]}x{hw[1]}-r{r}-{last}' for hw, r, last in CASES])
def test_kernels_against_the_oracle(hip, hw, r, last):
    check_case(hip, 3, hw[0], hw[1], r, last, mu=0.5 if r != 3 else 1.0)


def test_seventy_samples(hip):
    check_case(hip, 70, 5, 7, 3, 'random', mu=0.75)


def test_impulse_is_the_truncated_outer_product(hip):
    """The corner impulse against the taps themselves: t[y][W - 1 - j] = a w[r + y] w[r + j], each a product of two fp32 numbers and one
    fp32 factor: three roundings."""
    H, W, r = 17, 19, 7
    w, ctaps = taps_of(hip['A'], r, 1.0)
    g = torch.zeros(1, H, W, 4)
    g[0, 0, W - 1, :3] = torch.tensor([2.0, -1.0, 0.5])
    state = torch.zeros(1, 4, dtype=torch.int32)
    t, l1 = run_blur(hip, g.to(DEV), state.to(DEV), ctaps, r)
    want = torch.zeros(H, W, dtype=torch.float64)
    want[:r + 1, W - r - 1:] = torch.outer(w.double()[r:], w.double()[:r + 1])
    for c, a in enumerate((2.0, -1.0, 0.5)):
        assert ((t[0, ..., c].cpu().double() - a * want).abs() <= 3 * to.U * want.abs() * abs(a)).all()
    assert (t.cpu()[0][want == 0] == 0).all()


def test_invalid_arguments_are_refused_with_nothing_written(hip):
    lib, p = hip['lib'], hip['lib'].ptr
    B, H, W, r = 2, 5, 7, 1
    w, ctaps = taps_of(hip['A'], r, 1.0)
    g = torch.randn(B, H, W, 4, device=DEV)
    state = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    t = torch.full((B, H, W, 4), SENTINEL, device=DEV)
    l1 = torch.full((B, 1), SENTINEL, device=DEV)
    m = torch.full((B, H, W, 4), SENTINEL, device=DEV)
    ss = torch.full((B, 1), SENTINEL, device=DEV)
    g0 = g.clone()
    ok = dict(g=p(g), state=p(state), taps=ctaps, r=r, t=p(t), l1=p(l1), B=B, Hp=H, Wp=W)
    for bad in (dict(r=-1), dict(r=8), dict(Hp=0), dict(Wp=0), dict(Wp=-3), dict(B=0), dict(B=65536), dict(g=None), dict(state=None),
                dict(taps=None), dict(t=None), dict(l1=None)):
        with pytest.raises(RuntimeError, match='spaa_transfer_blur failed'):
            lib.call('spaa_transfer_blur', *{**ok, **bad}.values())
    ok = dict(t=p(t), l1=p(l1), tiles=1, mu=0.5, state=p(state), m=p(m), g=p(g), ss=p(ss), npartial=1, B=B, HW=H * W)
    for bad in (dict(mu=1.5), dict(mu=-0.1), dict(mu=float('nan')), dict(tiles=0), dict(npartial=0), dict(B=0), dict(B=65536), dict(HW=0),
                dict(t=None), dict(l1=None), dict(state=None), dict(m=None), dict(g=None), dict(ss=None)):
        with pytest.raises(RuntimeError, match='spaa_transfer_momentum failed'):
            lib.call('spaa_transfer_momentum', *{**ok, **bad}.values())
    torch.cuda.synchronize()
    assert (t == SENTINEL).all() and (l1 == SENTINEL).all() and (m == SENTINEL).all() and (ss == SENTINEL).all() and torch.equal(g, g0)
    assert hip['tiles'](0, 7) == 0 and hip['tiles'](H, W) == 1
