"""GPU: the two entry points of csrc/convnext_ops.hip through the C-ABI against the float64 restatement of tests/convnext_oracle.py,
element by element within that file's derived bars ((taps inside the image + 1) x 2^-24 x (|bias| + sum |w| |v|) x SLACK; likewise
with |add| for the adjoint), on the shapes of `DW_CASES` -- the smallest that touch each risk: a map smaller than the 7 x 7 window in
both axes and in one, a width that no strip length divides, one channel quad, quad counts that are no multiple of a wave, more quads
than a wave, the largest stage map.  tests/test_convnext_cpu.py shows that every mutation of the oracle lands more than 100 bars away
on these inputs.  And the downsample route of the body: a 2 x 2 / stride-2 convolution on the tap-list plans on an odd map.

The kernel has two forms (strips of 4 columns and long runs of rows, strips of 2 and short runs; spaa_dwconv7_form): every case runs
under both, and under the library's own choice, which must be bitwise one of them.

Every test reports the largest error / bar it saw through convnext_oracle.note(): an `accuracy:` line on stdout and, where
SPAA_ACCURACY_FILE names a file, appended to it (profiles/convnext_accuracy.txt is written that way by one run of the two GPU files)."""
import ctypes

import pytest
import torch

import convnext_oracle as co
from spaa_amd import _lib
from test_gpu_parity import hip, rel_inf  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
FORMS = {1: 'strips of 4', 2: 'strips of 2'}


def set_form(form):
    return _lib.load().spaa_dwconv7_form(form)


def fwd(x, wt, bias):
    b, h, w, c = x.shape
    out = torch.full(x.shape, NAN, device=DEV)
    p = _lib.ptr
    _lib.call('spaa_dwconv7_fwd', p(x), p(wt), p(bias), p(out), b, h, w, c)
    return out


def bwd(g, wt, add):
    b, h, w, c = g.shape
    g_in = torch.full(g.shape, NAN, device=DEV)
    p = _lib.ptr
    _lib.call('spaa_dwconv7_bwd', p(g), p(wt), p(add), p(g_in), b, h, w, c)
    return g_in


@pytest.fixture(scope='module')
def results(hip):
    """Per case: the inputs (CPU fp32), the kernels' outputs (forward, backward with and without `add`, a second run of each) and the
    float64 references with their bars.  Computed once, shared by the tests below, never modified."""
    out = {}
    for case in co.DW_CASES:
        x, wt, bias, g, add = co.dw_inputs(*case)
        dx, dw, db, dg, da = (t.to(DEV) for t in (x, wt, bias, g, add))
        x64, w64, b64, g64, a64 = (t.double() for t in (x, wt, bias, g, add))
        ref = dict(fwd=co.dwconv7(x64, w64, b64), bwd=co.dwconv7_bwd(g64, w64), bwd_add=co.dwconv7_bwd(g64, w64, a64))
        bar = dict(fwd=co.bar_dwconv7(x64, w64, b64), bwd=co.bar_dwconv7_bwd(g64, w64), bwd_add=co.bar_dwconv7_bwd(g64, w64, a64))
        for form in (0, 1, 2):
            assert set_form(form) in (0, 1, 2)
            try:
                gpu = dict(fwd=fwd(dx, dw, db), fwd2=fwd(dx, dw, db), bwd=bwd(dg, dw, None), bwd_add=bwd(dg, dw, da), bwd_add2=bwd(dg, dw, da))
            finally:
                set_form(0)
            out[form, case] = dict(inp=(x64, w64, b64, g64, a64), gpu={k: v.cpu() for k, v in gpu.items()}, ref=ref, bar=bar)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', co.DW_CASES, ids=str)
def test_forward_and_backward_within_the_derived_bars(results, case, form):
    r = results[form, case]
    worst = {}
    for k in ('fwd', 'bwd', 'bwd_add'):
        got = r['gpu'][k].double()
        assert torch.isfinite(got).all() and got.shape == r['ref'][k].shape, k            # every element was written
        worst[k] = float(((got - r['ref'][k]).abs() / r['bar'][k]).max())
    co.note(f'spaa_dwconv7 {case}, {FORMS[form]}: largest |error| / bar forward {worst["fwd"]:.3f}, backward {worst["bwd"]:.3f}, backward with '
          f'add {worst["bwd_add"]:.3f}')
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', co.DW_CASES, ids=str)
def test_the_pair_is_an_adjoint(results, case, form):
    """<g, fwd(x) - bias> == <bwd(g), x>, in float64 on the kernels' outputs, to the sum of the two bars weighed by |g| and |x|."""
    r = results[form, case]
    x, _, bias, g, _ = r['inp']
    lhs = (g * (r['gpu']['fwd'].double() - bias)).sum()
    rhs = (r['gpu']['bwd'].double() * x).sum()
    tol = (r['bar']['fwd'] * g.abs()).sum() + (r['bar']['bwd'] * x.abs()).sum()
    co.note(f'spaa_dwconv7 adjoint identity {case}, {FORMS[form]}: |<g, A x> - <A^T g, x>| / bar = {abs(float(lhs - rhs)) / float(tol):.3f}')
    assert abs(float(lhs - rhs)) <= float(tol)


def test_two_runs_and_the_two_forms_are_bitwise_equal(results):
    """Two runs of a form agree bit for bit, and so do the two forms (they accumulate in the same order), hence the library's own choice."""
    bits = lambda t: t.view(torch.int32)     # noqa: E731
    for (form, case), r in results.items():
        assert torch.equal(bits(r['gpu']['fwd']), bits(r['gpu']['fwd2'])), (form, case)
        assert torch.equal(bits(r['gpu']['bwd_add']), bits(r['gpu']['bwd_add2'])), (form, case)
        for k in ('fwd', 'bwd', 'bwd_add'):
            assert torch.equal(bits(r['gpu'][k]), bits(results[1, case]['gpu'][k])), (form, case, k)
    assert set_form(7) == 0 and set_form(0) == 0                              # an unknown form changes nothing
    co.note(f'spaa_dwconv7 two runs and the forms 0, 1, 2 bitwise equal on {len(co.DW_CASES)} cases, forward and backward (bar: exact)')


def test_add_may_be_the_output_itself(hip):
    """The block's backward pass may accumulate in place: g_in == add."""
    case = (2, 9, 13, 96)
    _, wt, _, g, add = co.dw_inputs(*case)
    dg, dw, da = g.to(DEV), wt.to(DEV), add.to(DEV)
    want = bwd(dg, dw, da)
    p = _lib.ptr
    _lib.call('spaa_dwconv7_bwd', p(dg), p(dw), p(da), p(da), *case)
    assert torch.equal(da, want)


def test_invalid_arguments_are_refused_with_nothing_written(hip):
    lib = _lib.load()
    st = _lib._stream
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    x = torch.rand(2, 5, 7, 8, device=DEV)
    w, bias = torch.rand(49, 8, device=DEV), torch.rand(8, device=DEV)
    out = torch.full((2, 5, 7, 8), -7.0, device=DEV)
    g_in = torch.full((2, 5, 7, 8), -7.0, device=DEV)
    big = 1 << 13                                                               # 2 x 8192 x 8192 x 4 = 2^29 elements
    bad = [
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), P(out), 2, 5, 7, 6, st()),        # C % 4 != 0
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), P(out), 2, 5, 7, 0, st()),
        lib.spaa_dwconv7_fwd(None, P(w), P(bias), P(out), 2, 5, 7, 8, st()),        # null pointers
        lib.spaa_dwconv7_fwd(P(x), None, P(bias), P(out), 2, 5, 7, 8, st()),
        lib.spaa_dwconv7_fwd(P(x), P(w), None, P(out), 2, 5, 7, 8, st()),
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), None, 2, 5, 7, 8, st()),
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), P(out), 0, 5, 7, 8, st()),        # sizes < 1
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), P(out), 2, 0, 7, 8, st()),
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), P(out), 2, 5, -1, 8, st()),
        lib.spaa_dwconv7_fwd(P(x), P(w), P(bias), P(out), 2, big, big, 4, st()),    # 2^29 elements
        lib.spaa_dwconv7_bwd(P(x), P(w), P(x), P(g_in), 2, 5, 7, 6, st()),
        lib.spaa_dwconv7_bwd(None, P(w), P(x), P(g_in), 2, 5, 7, 8, st()),
        lib.spaa_dwconv7_bwd(P(x), None, P(x), P(g_in), 2, 5, 7, 8, st()),
        lib.spaa_dwconv7_bwd(P(x), P(w), P(x), None, 2, 5, 7, 8, st()),
        lib.spaa_dwconv7_bwd(P(x), P(w), P(x), P(g_in), 2, 5, 0, 8, st()),
        lib.spaa_dwconv7_bwd(P(x), P(w), None, P(g_in), 2, big, big, 4, st()),
    ]
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in bad), bad                                      # hipErrorInvalidValue
    assert (out == -7.0).all() and (g_in == -7.0).all()
    with pytest.raises(RuntimeError, match='spaa_dwconv7_fwd failed'):
        _lib.call('spaa_dwconv7_fwd', P(x), P(w), P(bias), P(out), 2, 5, 7, 6)


def test_downsample_route_on_an_odd_map(hip):
    """conv_fwd_plan(w, b, 2, 0) / conv_dgrad_plan(w, 2, 0) of a 2 x 2 kernel on 9 x 13 x 16 -> 4 x 6 x 32 against float64 at the 1e-5
    relative L-inf that tests/test_vit_gpu.py holds the 1 x 1 plans to; the row and the column that the forward floor drops get a
    gradient of exactly 0."""
    cp = hip['cp']
    gen = torch.Generator().manual_seed(77)
    b, h, w, cin, cout = 3, 9, 13, 16, 32
    wt = torch.randn(cout, cin, 2, 2, generator=gen) / (4 * cin) ** 0.5
    bias = torch.randn(cout, generator=gen)
    x = torch.randn(b, h, w, cin, generator=gen)
    out = torch.full((b, h // 2, w // 2, cout), NAN, device=DEV)
    cp.conv_fwd_plan(wt, bias, 2, 0, DEV, 'down').run(x.to(DEV), out)
    ref = co.patch_conv(x.double(), wt.double(), bias.double())
    e = rel_inf(out, ref)
    g = torch.randn(b, h // 2, w // 2, cout, generator=gen)
    g_in = torch.full((b, h, w, cin), NAN, device=DEV)
    cp.conv_dgrad_plan(wt, 2, 0, DEV, 'down_dgrad').run(g.to(DEV), g_in)
    x64 = x.double().requires_grad_(True)
    (co.patch_conv(x64, wt.double(), bias.double()) * g.double()).sum().backward()
    eg = rel_inf(g_in, x64.grad)
    co.note(f'downsample 2x2/2 on 9x13x16 -> 4x6x32: forward rel Linf {e:.2e}, input gradient {eg:.2e} (bar 1e-5)')
    assert ref.shape == out.shape and torch.isfinite(g_in).all()
    assert e < 1e-5 and eg < 1e-5
    assert (g_in[:, 8] == 0).all() and (g_in[:, :, 12] == 0).all() and (x64.grad[:, 8] == 0).all() and (x64.grad[:, :, 12] == 0).all()
