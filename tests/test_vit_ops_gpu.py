"""GPU: every entry point of csrc/vit_ops.hip through the C-ABI against the float64 restatements of tests/vit_oracle.py, on that file's
inputs (planted rows included) and within its bars: first-order fp32 bounds in units of U = 2^-24 on the magnitudes that the kernel sums
(derivations at vit_oracle.bar_*), with what the device library's expf / logf / erfcf contribute taken as LIBM = 4 times the error of
torch's own fp32 evaluation of the same function on the CPU at the same arguments (both numbers are printed).  Each test prints its
largest error / bar as an `accuracy:` line (profiles/vit_ops_accuracy.txt holds the lines of one run).  tests/test_vit_cpu.py shows
that each mutation of the oracle is beyond these bars on these inputs."""
import ctypes

import pytest
import torch

import vit_oracle as vo
from spaa_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = vo.U


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def d64(t):
    return t.detach().cpu().double()


def worst(err, bar):
    return float((err / bar.clamp_min(1e-300)).max())


def report(name, ratio):
    print(f'accuracy: {name}: largest error / bar = {ratio:.3f}')
    assert ratio <= 1.0, (name, ratio)


def twice(fn):
    """Two runs of a launch into fresh buffers: bitwise equal (no atomics, a fixed accumulation order).  Returns the first run's outputs."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for s, t in zip(a, b):
        assert torch.equal(s.view(torch.int32), t.view(torch.int32))
    return a


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, w, b, stride=None):
    """x [rows, D] on the device, placed at the row stride `stride` (None: dense) in a NaN-filled buffer"""
    rows, D = x.shape
    st = stride or D
    xb = nan(rows, st)
    xb[:, :D] = x
    y, mean, rstd = nan(rows, st), nan(rows), nan(rows)
    p = _lib.ptr
    _lib.call('spaa_layernorm_fwd', p(xb), st, p(w), p(b), p(y), st, p(mean), p(rstd), rows, D, 1e-6)
    assert torch.isnan(y[:, D:]).all()                 # nothing is written between the rows
    return y[:, :D].contiguous(), mean, rstd


def ln_bwd(g, x, w, mean, rstd, add, stride=None):
    rows, D = x.shape
    st = stride or D
    xb, gx = nan(rows, st), nan(rows, st)
    xb[:, :D] = x
    p = _lib.ptr
    _lib.call('spaa_layernorm_bwd', p(g), D, p(xb), st, p(w), p(mean), p(rstd), p(add), D, p(gx), st, rows, D)
    assert torch.isnan(gx[:, D:]).all()
    return (gx[:, :D].contiguous(),)


@pytest.mark.parametrize('D,rows', vo.LN_CASES)
def test_layernorm_forward_and_adjoint(lib, D, rows):
    x, w, b, g, add = vo.ln_inputs(D, rows)
    xd, wd, bd, gd, ad = (t.to(DEV) for t in (x, w, b, g, add))
    x6, w6, b6, g6, a6 = (t.double() for t in (x, w, b, g, add))
    y_ref, mu_ref, rs_ref = vo.layernorm(x6, w6, b6)
    e_y, e_mu, e_rs = vo.bar_layernorm(x6, w6, b6)
    ratios = []
    for stride in (None, D + 8):                                    # dense, and rows further apart than D (the head's class-token rows)
        y, mean, rstd = twice(lambda: ln_fwd(xd, wd, bd, stride))
        ratios += [worst((d64(y) - y_ref).abs(), e_y), worst((d64(mean) - mu_ref).abs(), e_mu), worst((d64(rstd) - rs_ref).abs(), e_rs)]
    report(f'layernorm_fwd D={D} rows={rows} (y, mean, rstd; dense and strided)', max(ratios))
    # the adjoint on the kernel's own statistics (held to their bars above), with and without the summand
    m6, r6 = d64(mean), d64(rstd)
    ratios = []
    for addd, add6 in ((None, None), (ad, a6)):
        for stride in (None, D + 8):
            gx, = twice(lambda: ln_bwd(gd, xd, wd, mean, rstd, addd, stride))
            ratios.append(worst((d64(gx) - vo.layernorm_bwd(g6, x6, w6, m6, r6, add6)).abs(), vo.bar_layernorm_bwd(g6, x6, w6, m6, r6, add6)))
    report(f'layernorm_bwd D={D} rows={rows} (with and without add; dense and strided)', max(ratios))


def test_layernorm_long_rows_take_the_memory_form(lib):
    """D = 1040 > 1024: the row does not fit the register slots and is re-read from memory -- the same bars."""
    D, rows = 1040, 5
    x, w, b, g, add = vo.ln_inputs(D, rows)
    xd, wd, bd, gd, ad = (t.to(DEV) for t in (x, w, b, g, add))
    x6, w6, b6, g6, a6 = (t.double() for t in (x, w, b, g, add))
    y, mean, rstd = twice(lambda: ln_fwd(xd, wd, bd))
    y_ref, mu_ref, rs_ref = vo.layernorm(x6, w6, b6)
    e_y, e_mu, e_rs = vo.bar_layernorm(x6, w6, b6)
    gx, = twice(lambda: ln_bwd(gd, xd, wd, mean, rstd, ad))
    m6, r6 = d64(mean), d64(rstd)
    report('layernorm D=1040 (forward, adjoint)', max(
        worst((d64(y) - y_ref).abs(), e_y), worst((d64(mean) - mu_ref).abs(), e_mu), worst((d64(rstd) - rs_ref).abs(), e_rs),
        worst((d64(gx) - vo.layernorm_bwd(g6, x6, w6, m6, r6, a6)).abs(), vo.bar_layernorm_bwd(g6, x6, w6, m6, r6, a6))))


# ---- GELU ------------------------------------------------------------------------------------------------------------------------
def test_gelu_forward_and_adjoint(lib):
    x, g = vo.gelu_inputs()
    xd, gd = x.to(DEV), g.to(DEV)
    n, p = x.numel(), _lib.ptr

    def fwd():
        act = nan(n)
        _lib.call('spaa_gelu_fwd', p(xd), p(act), n)
        return (act,)

    def bwd():
        gx = nan(n)
        _lib.call('spaa_gelu_bwd', p(gd), p(xd), p(gx), n)
        return (gx,)

    act, = twice(fwd)
    gx, = twice(bwd)
    m_f = vo.measured_rel(vo.gelu, x)
    mag = vo.gelu_bwd_mag(g.double(), x.double())
    m_b = vo.measured_rel(lambda t: vo.gelu_bwd(g.to(t.dtype), t), x, mag)
    e_f = float(vo.gelu_rel(act.cpu(), vo.gelu(x.double())).max())
    e_b = float(vo.gelu_rel(gx.cpu(), vo.gelu_bwd(g.double(), x.double()), mag).max())
    print(f'gelu: relative error forward {e_f:.2e} (torch fp32 on the CPU {m_f:.2e}, bar {vo.LIBM * m_f:.2e}), adjoint {e_b:.2e} '
          f'(torch {m_b:.2e}, bar {vo.LIBM * m_b:.2e})')
    assert torch.isfinite(act).all() and torch.isfinite(gx).all()
    a, xs = act.cpu(), x
    assert a[xs == 40].item() == 40.0 and a[xs == -40].abs().max().item() == 0.0 and (a[xs == 0].abs() == 0).all()
    report('gelu_fwd', e_f / (vo.LIBM * m_f))
    report('gelu_bwd', e_b / (vo.LIBM * m_b))
    # in place, as the body's backward pass runs it
    gi = gd.clone()
    _lib.call('spaa_gelu_bwd', p(gi), p(xd), p(gi), n)
    assert torch.equal(gi, gx)


# ---- attention -------------------------------------------------------------------------------------------------------------------
def attn_fwd(qkv, B, heads, T, dh):
    ctx, lse = nan(B, T, heads * dh), nan(B, heads, T)
    p = _lib.ptr
    _lib.call('spaa_attn_fwd', p(qkv), p(ctx), p(lse), B, T, heads, dh)
    return ctx, lse


def attn_bwd(qkv, ctx, lse, g, B, heads, T, dh):
    g_qkv, delta = nan(B, T, 3 * heads * dh), nan(B, heads, T)
    p = _lib.ptr
    _lib.call('spaa_attn_bwd', p(qkv), p(ctx), p(lse), p(g), p(g_qkv), p(delta), B, T, heads, dh)
    return g_qkv, delta


def exp_log_errors(qkv6, heads):
    """torch's fp32 exp and log on the CPU against float64 at the arguments the forward kernel meets: s - max, and the row sums."""
    q, k, _ = vo.split_heads(qkv6, heads)
    s = q @ k.transpose(-1, -2) / (q.shape[-1] ** 0.5)
    arg = (s - s.max(dim=-1, keepdim=True).values).float()
    arg = arg[arg > -80]                                        # (below that the term vanishes against the row's 1)
    sums = torch.exp(s - s.max(dim=-1, keepdim=True).values).sum(dim=-1).float()
    return vo.measured_rel(torch.exp, arg), vo.measured_rel(torch.log, sums[sums > 1.0001]) if (sums > 1.0001).any() else U


@pytest.mark.parametrize('case', vo.ATT_CASES, ids=lambda c: 'B%d_h%d_T%d_dh%d' % c)
def test_attention_forward_and_adjoint(lib, case):
    B, heads, T, dh = case
    qkv, g = vo.attn_inputs(*case)
    qd, gd = qkv.to(DEV), g.to(DEV)
    q6, g6 = qkv.double(), g.double()
    m_exp, m_log = exp_log_errors(q6, heads)
    ctx, lse = twice(lambda: attn_fwd(qd, *case))
    ctx_ref, lse_ref = vo.attention(q6, heads)
    e_ctx, e_lse = vo.bar_attention(q6, heads, m_exp, m_log)
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    print(f'attention {case}: torch fp32 exp {m_exp:.2e}, log {m_log:.2e} (relative, CPU); allowed {vo.LIBM} x')
    report(f'attn_fwd {case} (ctx, lse)', max(worst((d64(ctx) - ctx_ref).abs(), e_ctx), worst((d64(lse) - lse_ref).abs(), e_lse)))
    # the adjoint on the oracle's ctx and lse rounded to fp32: the kernel's formula, element by element ...
    c32, l32 = ctx_ref.float(), lse_ref.float()
    g_qkv, delta = twice(lambda: attn_bwd(qd, c32.to(DEV), l32.to(DEV), gd, *case))
    assert torch.isfinite(g_qkv).all()
    ref = vo.attention_bwd(q6, c32.double(), l32.double(), g6, heads)
    bar = vo.bar_attention_bwd(q6, c32.double(), l32.double(), g6, heads, m_exp)
    report(f'attn_bwd {case} (g_qkv)', worst((d64(g_qkv) - ref).abs(), bar))
    # ... and as an adjoint: <attn'(g), u> = <g, d attn(u)> with the float64 Jacobian-vector product of the oracle's forward pass
    u = torch.randn(qkv.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    _, jvp = torch.autograd.functional.jvp(lambda t: vo.attention(t, heads)[0], q6, u)
    lhs, rhs = float((d64(g_qkv) * u).sum()), float((g6 * jvp).sum())
    tol = float((bar * u.abs()).sum())
    print(f'attention {case}: <g_qkv, u> = {lhs:.9e}, <g, J u> = {rhs:.9e}, difference {abs(lhs - rhs):.2e}, bound {tol:.2e}')
    report(f'attn adjoint identity {case}', abs(lhs - rhs) / tol)


# ---- patch / token bookkeeping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', (4, 16))
def test_patchify_and_assemble_are_exact(lib, P):
    B, gh, gw, D = 2, 2, 3, 8 if P == 4 else 48
    h, w, n = gh * P, gw * P, gh * gw
    gen = torch.Generator().manual_seed(P)
    img = torch.randn(B, h, w, 4, generator=gen)
    p = _lib.ptr
    # (device copies are made once and kept: a temporary's block may be handed out again before the launch that reads it)
    img_d = img.to(DEV)

    def fwd():
        out = nan(B * n, 4 * P * P)
        _lib.call('spaa_vit_patchify', p(img_d), p(out), B, h, w, P)
        return (out,)

    patches, = twice(fwd)
    assert torch.equal(patches.cpu(), vo.patchify(img, P))
    gp = torch.randn(B * n, 4 * P * P, generator=gen)
    gp_d = gp.to(DEV)

    def bwd():
        out = nan(B, h, w, 4)
        _lib.call('spaa_vit_unpatchify', p(gp_d), p(out), B, h, w, P)
        return (out,)

    g_img, = twice(bwd)
    assert torch.equal(g_img.cpu(), vo.unpatchify(gp, B, h, w, P))
    assert float((vo.patchify(img, P) * gp).sum()) == pytest.approx(float((img * vo.unpatchify(gp, B, h, w, P)).sum()), rel=1e-5)   # an adjoint pair
    emb, cls, pos = torch.randn(B, n, D, generator=gen), torch.randn(D, generator=gen), torch.randn(n + 1, D, generator=gen)
    emb_d, cls_d, pos_d = emb.to(DEV), cls.to(DEV), pos.to(DEV)

    def asm():
        out = nan(B, n + 1, D)
        _lib.call('spaa_vit_assemble', p(emb_d), p(cls_d), p(pos_d), p(out), B, n + 1, D)
        return (out,)

    x, = twice(asm)
    assert torch.equal(x.cpu(), vo.assemble(emb, cls, pos))            # (one fp32 addition per element: the same in torch)
    gx = torch.randn(B, n + 1, D, generator=gen)
    gx_d = gx.to(DEV)

    def asm_bwd():
        out = nan(B, n, D)
        _lib.call('spaa_vit_assemble_bwd', p(gx_d), p(out), B, n + 1, D)
        return (out,)

    g_emb, = twice(asm_bwd)
    assert torch.equal(g_emb.cpu(), gx[:, 1:])
    report(f'patchify / assemble P={P} (bit-exact)', 0.0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_with_nothing_written(lib):
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    st = _lib._stream
    big = 1 << 29
    a, b, c, d, e, f = (torch.full((4096,), 7.0, device=DEV) for _ in range(6))
    bad = [
        lib.spaa_layernorm_fwd(None, 8, P(b), P(c), P(d), 8, P(e), P(f), 2, 8, 1e-6, st()),             # null pointers
        lib.spaa_layernorm_fwd(P(a), 8, None, P(c), P(d), 8, P(e), P(f), 2, 8, 1e-6, st()),
        lib.spaa_layernorm_fwd(P(a), 8, P(b), P(c), None, 8, P(e), P(f), 2, 8, 1e-6, st()),
        lib.spaa_layernorm_fwd(P(a), 8, P(b), P(c), P(d), 8, None, P(f), 2, 8, 1e-6, st()),
        lib.spaa_layernorm_fwd(P(a), 6, P(b), P(c), P(d), 6, P(e), P(f), 2, 6, 1e-6, st()),             # D % 4
        lib.spaa_layernorm_fwd(P(a), 4, P(b), P(c), P(d), 8, P(e), P(f), 2, 8, 1e-6, st()),             # a stride below D
        lib.spaa_layernorm_fwd(P(a), 8, P(b), P(c), P(d), 8, P(e), P(f), 0, 8, 1e-6, st()),             # no rows
        lib.spaa_layernorm_fwd(P(a), 8, P(b), P(c), P(d), 8, P(e), P(f), big // 8, 8, 1e-6, st()),      # 2^29 elements
        lib.spaa_layernorm_bwd(None, 8, P(a), 8, P(b), P(e), P(f), None, 8, P(d), 8, 2, 8, st()),
        lib.spaa_layernorm_bwd(P(c), 8, P(a), 8, P(b), P(e), P(f), None, 8, None, 8, 2, 8, st()),
        lib.spaa_layernorm_bwd(P(c), 6, P(a), 6, P(b), P(e), P(f), None, 6, P(d), 6, 2, 6, st()),
        lib.spaa_gelu_fwd(None, P(d), 8, st()), lib.spaa_gelu_fwd(P(a), None, 8, st()), lib.spaa_gelu_fwd(P(a), P(d), 6, st()),
        lib.spaa_gelu_fwd(P(a), P(d), big, st()), lib.spaa_gelu_bwd(P(a), P(b), None, 8, st()), lib.spaa_gelu_bwd(P(a), P(b), P(d), 0, st()),
        lib.spaa_attn_fwd(None, P(d), P(e), 1, 4, 2, 8, st()), lib.spaa_attn_fwd(P(a), None, P(e), 1, 4, 2, 8, st()),
        lib.spaa_attn_fwd(P(a), P(d), None, 1, 4, 2, 8, st()),
        lib.spaa_attn_fwd(P(a), P(d), P(e), 1, 4, 2, 6, st()),                                           # dh % 4
        lib.spaa_attn_fwd(P(a), P(d), P(e), 1, 4, 1, 68, st()),                                          # dh > 64
        lib.spaa_attn_fwd(P(a), P(d), P(e), 1, 257, 1, 4, st()),                                         # T > 256
        lib.spaa_attn_fwd(P(a), P(d), P(e), 1 << 20, 256, 1, 64, st()),                                  # 2^29 elements and more
        lib.spaa_attn_bwd(P(a), P(b), P(e), P(c), None, P(f), 1, 4, 2, 8, st()),
        lib.spaa_attn_bwd(P(a), P(b), P(e), P(c), P(d), None, 1, 4, 2, 8, st()),
        lib.spaa_attn_bwd(P(a), P(b), P(e), P(c), P(d), P(f), 1, 257, 1, 4, st()),
        lib.spaa_attn_bwd(P(a), P(b), P(e), P(c), P(d), P(f), 1, 4, 1, 68, st()),
        lib.spaa_vit_patchify(None, P(d), 1, 8, 8, 4, st()), lib.spaa_vit_patchify(P(a), None, 1, 8, 8, 4, st()),
        lib.spaa_vit_patchify(P(a), P(d), 1, 8, 10, 4, st()),                                            # w % P
        lib.spaa_vit_patchify(P(a), P(d), 1 << 15, 64, 64, 4, st()),                                     # 2^29 elements
        lib.spaa_vit_unpatchify(P(a), None, 1, 8, 8, 4, st()), lib.spaa_vit_unpatchify(P(a), P(d), 1, 6, 8, 4, st()),
        lib.spaa_vit_assemble(P(a), P(b), P(c), None, 1, 5, 8, st()), lib.spaa_vit_assemble(P(a), None, P(c), P(d), 1, 5, 8, st()),
        lib.spaa_vit_assemble(P(a), P(b), P(c), P(d), 1, 5, 6, st()),                                    # D % 4
        lib.spaa_vit_assemble(P(a), P(b), P(c), P(d), 1, 1, 8, st()),                                    # no patch token
        lib.spaa_vit_assemble_bwd(P(a), None, 1, 5, 8, st()), lib.spaa_vit_assemble_bwd(P(a), P(d), 1, 5, 6, st()),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    for t in (a, b, c, d, e, f):
        assert (t == 7.0).all()
    with pytest.raises(RuntimeError, match='spaa_attn_fwd failed'):
        _lib.call('spaa_attn_fwd', P(a), P(d), P(e), 1, 257, 1, 4)
