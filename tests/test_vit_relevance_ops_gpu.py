"""GPU: spaa_attn_relevance and spaa_relevance_map of csrc/vit_ops.hip through the C-ABI against the float64 restatement of
tests/vit_relevance_oracle.py, on the shapes of vit_oracle.ATT_CASES (T = 1, the 64-row slot boundary, the real token count and the
cap) with that file's planted inputs (a positive, a negative and a zero seed, a target outside the classes, rho with exact zeros) and
within its derived bar (vit_relevance_oracle.bar_step; the library's expf as LIBM = 4 times the error of torch's fp32 exp on the CPU at
the same arguments).  Each test prints its largest error / bar as an `accuracy:` line (profiles/vit_relevance_accuracy.txt holds the
lines of one run).  tests/test_vit_relevance_cpu.py shows that each mutation of the oracle is beyond this bar on these inputs."""
import ctypes

import pytest
import torch

import vit_oracle as vo
import vit_relevance_oracle as ro
from spaa_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def d64(t):
    return t.detach().cpu().double()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def relevance(qkv, lse, g, rho, gl, tg, case):
    """One step into NaN-filled buffers: (rho_out [B, T], the head workspace)."""
    B, heads, T, dh = case
    ws, out = nan(B, heads, T), nan(B, T)
    p = _lib.ptr
    _lib.call('spaa_attn_relevance', p(qkv), p(lse), p(g), p(rho), p(gl), ro.NCLS, p(tg), p(ws), p(out), B, T, heads, dh)
    return out, ws


def class_map(rho, gl, tg, B, T):
    c, cmax = nan(B, T - 1), nan(B)
    p = _lib.ptr
    _lib.call('spaa_relevance_map', p(rho), p(gl), ro.NCLS, p(tg), p(c), p(cmax), B, T)
    return c, cmax


@pytest.mark.parametrize('case', vo.ATT_CASES, ids=lambda c: 'B%d_h%d_T%d_dh%d' % c)
def test_relevance_step_and_map(lib, case):
    B, heads, T, dh = case
    ratios = []
    for variant in ro.VARIANTS:
        host = ro.step_inputs(case, variant)
        qkv, lse, g, rho, gl, tg = (t.to(DEV) for t in host)
        q6, l6, g6, r6, gl6 = (t.double() for t in host[:5])
        seed = ro.seeds(gl6, host[5])
        assert (seed[0] == 0) == (variant in ('zero_seed', 'target_outside')) and (seed[1:] == -0.5).all() and (r6 == 0).any() == (T > 2)
        m_exp = ro.exp_error(q6, l6, heads)
        out, ws = relevance(qkv, lse, g, rho, gl, tg, case)
        out2, ws2 = relevance(qkv, lse, g, rho, gl, tg, case)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.isfinite(ws).all()          # (every element of both is written)
        assert same_bits(out, out2) and same_bits(ws, ws2)                      # no atomics, a fixed order
        ref, bar = ro.step(q6, l6, g6, r6, seed, heads), ro.bar_step(q6, l6, g6, r6, seed, heads, m_exp)
        ratio = float(((d64(out) - ref).abs() / bar.clamp_min(1e-300)).max())
        print(f'relevance step {case} {variant}: torch fp32 exp {m_exp:.2e} (relative, CPU; allowed {vo.LIBM} x); error / bar {ratio:.3f}')
        ratios.append(ratio)
        if seed[0] == 0:                                                        # no class to explain: that sample's rho is kept, bit for bit
            assert same_bits(out[0], rho[0]) and not ws[0].any()
        if B > 1:
            assert not same_bits(out[1], rho[1])
        # the top layer: rho_in = NULL stands for e_cls
        e_cls = torch.zeros(B, T, device=DEV)
        e_cls[:, 0] = 1.0
        top, _ = relevance(qkv, lse, g, None, gl, tg, case)
        top_e, _ = relevance(qkv, lse, g, e_cls, gl, tg, case)
        assert torch.isfinite(top).all() and same_bits(top, top_e)
        e6 = d64(e_cls)
        ratios.append(float(((d64(top) - ro.step(q6, l6, g6, e6, seed, heads)).abs() / ro.bar_step(q6, l6, g6, e6, seed, heads, m_exp).clamp_min(1e-300)).max()))
        # in place
        rho_io = rho.clone()
        ws3 = nan(B, heads, T)
        p = _lib.ptr
        _lib.call('spaa_attn_relevance', p(qkv), p(lse), p(g), p(rho_io), p(gl), ro.NCLS, p(tg), p(ws3), p(rho_io), B, T, heads, dh)
        assert same_bits(rho_io, out)
        if T > 1:
            signed = out.clone()
            signed[:, 1::2] *= -1.0                                             # (the map clamps: give it something to clamp)
            c, cmax = class_map(signed, gl, tg, B, T)
            c2, cmax2 = class_map(signed, gl, tg, B, T)
            c_ref, cmax_ref = ro.class_map(d64(signed), seed)
            assert same_bits(c, c2) and same_bits(cmax, cmax2)
            assert torch.equal(d64(c), c_ref) and torch.equal(d64(cmax), cmax_ref)          # a clamp and a maximum: exact
            assert (seed[0] != 0) or (not c[0].any() and float(cmax[0]) == 0.0)
    worst = max(ratios)
    print(f'accuracy: attn_relevance {case} (rho_out over {len(ro.VARIANTS)} seed variants, given rho and e_cls): largest error / bar = {worst:.3f}')
    assert worst <= 1.0, (case, ratios)


def test_invalid_arguments_are_refused_with_nothing_written(lib):
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    st = _lib._stream
    a, b, c, d, e, f, g = (torch.full((4096,), 7.0, device=DEV) for _ in range(7))
    tg = torch.zeros(8, dtype=torch.int32, device=DEV)
    ok = lambda **kw: dict(dict(qkv=P(a), lse=P(b), g=P(c), rho=P(d), gl=P(e), ncls=4, tg=P(tg), ws=P(f), out=P(g), B=1, T=4, heads=2, dh=8), **kw)   # noqa: E731

    def step(**kw):
        k = ok(**kw)
        return lib.spaa_attn_relevance(k['qkv'], k['lse'], k['g'], k['rho'], k['gl'], k['ncls'], k['tg'], k['ws'], k['out'], k['B'], k['T'],
                                       k['heads'], k['dh'], st())

    bad = [step(qkv=None), step(lse=None), step(g=None), step(gl=None), step(tg=None), step(ws=None), step(out=None),
           step(ncls=0), step(B=0), step(T=0), step(heads=0),
           step(dh=6),                                                           # dh % 4
           step(heads=1, dh=68),                                                 # dh > 64
           step(heads=1, T=257, dh=4),                                           # T > 256
           step(B=1 << 20, T=256, heads=1, dh=64),                               # 2^29 elements and more
           lib.spaa_relevance_map(None, P(e), 4, P(tg), P(f), P(g), 1, 4, st()),
           lib.spaa_relevance_map(P(a), None, 4, P(tg), P(f), P(g), 1, 4, st()),
           lib.spaa_relevance_map(P(a), P(e), 4, None, P(f), P(g), 1, 4, st()),
           lib.spaa_relevance_map(P(a), P(e), 4, P(tg), None, P(g), 1, 4, st()),
           lib.spaa_relevance_map(P(a), P(e), 4, P(tg), P(f), None, 1, 4, st()),
           lib.spaa_relevance_map(P(a), P(e), 0, P(tg), P(f), P(g), 1, 4, st()),
           lib.spaa_relevance_map(P(a), P(e), 4, P(tg), P(f), P(g), 0, 4, st()),
           lib.spaa_relevance_map(P(a), P(e), 4, P(tg), P(f), P(g), 1, 1, st()),            # no patch token
           lib.spaa_relevance_map(P(a), P(e), 4, P(tg), P(f), P(g), 1 << 15, 1 << 14, st())]   # 2^29 elements
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    for t in (a, b, c, d, e, f, g):
        assert (t == 7.0).all()
    with pytest.raises(RuntimeError, match='spaa_attn_relevance failed'):
        _lib.call('spaa_attn_relevance', P(a), P(b), P(c), P(d), P(e), 4, P(tg), P(f), P(g), 1, 257, 1, 4)
