"""GPU: the blur kernels (csrc/blur_ops.hip) one by one, through the C ABI, against their float64 / integer restatement
(tests/blur_oracle.py).  B = 3 float images per shape, J = 2, 3, 4 draws, rows of planted sigmas that hold sigma = 0 (a bitwise copy),
r = 1, r = 8 and sigmas on both sides of an integer 3 sigma.  The shapes stand around the 32 x 16 tile of a workgroup
(SPAA_BLUR_TILE_W x SPAA_BLUR_TILE_H): a single pixel, both sides below r, a side of exactly r and of r + 1, one tile plus one pixel in
each axis, a few ragged tiles.  Every output lies between guard words in a sentinel-filled buffer.  r and the taps of every comparison
come from the fp32 sigma the kernel wrote.  The filter is linear and has no ties: no pixel is exempted from any comparison.  Every test
prints its largest error over the bar as an `accuracy:` line (profiles/blur_accuracy.txt holds the lines of one run)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import blur_oracle as bo
from test_gpu_parity import hip  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = 3
DRAWS = (2, 3, 4)
TILE_H, TILE_W = 16, 32
SHAPES = ((1, 1), (3, 5), (8, 9), (9, 8), (1, 2), (TILE_H + 1, TILE_W + 1), (40, 70))
HIP_INVALID_VALUE = 1
GUARD = 64             # floats on either side of an output
SENTINEL = -3.0
F32 = np.float32
# sigma = 0, r = 1, r = 8, 3 sigma = 1 exactly in fp32 (r = 1) and one ulp above (r = 2), one ulp above 3 sigma = 6 (r = 7); then r = 6, 3, 6
PLANTED = (F32(0.0), F32(0.3), F32(2.5), F32(1 / 3), np.nextafter(F32(1 / 3), F32(1)), np.nextafter(F32(2.0), F32(3)), F32(2.0), F32(1.0),
           F32(1.7))
PLANTED_R = (0, 1, 8, 1, 2, 7, 6, 3, 6)


def planted_sigmas(J):
    return np.array([PLANTED[(b * J + j) % len(PLANTED)] for b in range(B) for j in range(J)], dtype=F32).reshape(B, J)


@functools.lru_cache(maxsize=None)
def reference(hw, J):
    """The inputs of a case and the oracle's outputs, computed once and shared: y, g [B][H][W][3] float64 (fp32 values), and per (b, j)
    the forward, the transpose and their bars."""
    H, W = hw
    rng = np.random.default_rng(1000 * H + 10 * W + J)
    y = np.stack([bo.float_image(rng, H, W) for _ in range(B)])
    g = rng.normal(size=(J, B, H, W, 3)).astype(F32).astype(np.float64)
    sg = planted_sigmas(J)
    ref = {}
    for b in range(B):
        for j in range(J):
            r, w = bo.taps(sg[b, j])
            e = bo.tap_ulps(sg[b, j])
            ref[b, j] = (bo.forward(y[b], r, w), bo.bar_forward(y[b], r, w, e), bo.backward(g[j, b], r, w), bo.bar_backward(g[j, b], r, w, e))
    for v in (y, g):
        v.setflags(write=False)
    return y, g, sg, ref


def guarded(shape, fill=SENTINEL):
    """(the whole buffer, the view between its guard words) on the GPU."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def device_images(x):
    """[B][H][W][4] fp32 on the GPU with garbage in the pad channel (it is not read)."""
    x4 = torch.full(x.shape[:3] + (4,), float('nan'))
    x4[..., :3] = torch.from_numpy(np.array(x, dtype=F32))                   # (a copy: the shared reference is read-only)
    x4[0, 0, 0, 3] = 1e30
    return x4.to(DEV)


def make_rows(lib, sigmas):
    """spaa_blur_rows of fp32 sigmas [...] -> rows [..., 12] on the GPU, between guard words."""
    sg = torch.from_numpy(np.ascontiguousarray(sigmas, dtype=F32)).to(DEV)
    buf, rows = guarded(tuple(sg.shape) + (bo.ROW,))
    lib.call('spaa_blur_rows', lib.ptr(sg), lib.ptr(rows), sg.numel())
    torch.cuda.synchronize()
    assert guards_intact(buf)
    return rows


def check_rows(rows, sigmas):
    """Kernel rows against the oracle's rows of the kernel's own sigmas; returns the largest tap error over its bar."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, bo.ROW)
    worst = 0.0
    for row, s in zip(rows, np.asarray(sigmas, dtype=F32).ravel()):
        want, bar = bo.row_of(s), bo.bar_row(s)
        assert row[0] == want[0] and row[1] == want[1] and row[11] == 0 and (row[3 + int(row[1]):] == 0).all(), (row, want)
        if want[1] == 0:
            assert np.array_equal(row, want)
            continue
        taps = slice(2, 3 + int(want[1]))
        worst = max(worst, float((np.abs(row - want)[taps] / bar[taps]).max()))
    return worst


def run(lib, name, ins, rows, J, H, W):
    bufs, outs = zip(*[guarded((B, H, W, 4)) for _ in range(J)])
    lib.call(name, lib.ptr_array(list(ins)), lib.ptr(rows), J, lib.ptr_array(list(outs)), B, H, W)
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in bufs), f'{name} wrote outside its output'
    return outs


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('J', DRAWS)
@pytest.mark.parametrize('hw', SHAPES)
def test_forward_and_transpose_against_the_oracle(hip, hw, J):
    lib = hip['lib']
    H, W = hw
    y, g, sg, ref = reference(hw, J)
    rows = make_rows(lib, sg)
    rows_np = rows.cpu().numpy()
    worst_row = check_rows(rows_np, sg)
    assert [int(r) for r in rows_np[..., 1].ravel()] == [PLANTED_R[i % len(PLANTED)] for i in range(B * J)]
    y_d = device_images(y)
    g_d = [device_images(g[j]) for j in range(J)]
    outs = run(lib, 'spaa_blur_fwd', [y_d] * J, rows, J, H, W)
    g_y = run(lib, 'spaa_blur_bwd', g_d, rows, J, H, W)
    # two runs, and J equal pointers against J copies: bitwise
    for name, ins, first in (('spaa_blur_fwd', [y_d] * J, outs), ('spaa_blur_bwd', g_d, g_y)):
        again = run(lib, name, ins, rows, J, H, W)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, again)), name
    copies = run(lib, 'spaa_blur_fwd', [y_d.clone() for _ in range(J)], rows, J, H, W)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, copies))
    worst_f = worst_b = worst_i = 0.0
    for j in range(J):
        got_f, got_b = outs[j].cpu().numpy().astype(np.float64), g_y[j].cpu().numpy().astype(np.float64)
        assert (got_f[..., 3] == 0).all() and (got_b[..., 3] == 0).all() and np.isfinite(got_f).all() and np.isfinite(got_b).all()
        for b in range(B):
            want_f, bar_f, want_b, bar_b = ref[b, j]
            if sg[b, j] == 0:                                                  # the identity row: a copy, bit for bit
                assert torch.equal(bits(outs[j][b, ..., :3]), bits(y_d[b, ..., :3])) and torch.equal(bits(g_y[j][b, ..., :3]), bits(g_d[j][b, ..., :3]))
                continue
            worst_f = max(worst_f, float((np.abs(got_f[b, ..., :3] - want_f) / bar_f).max()))
            worst_b = max(worst_b, float((np.abs(got_b[b, ..., :3] - want_b) / bar_b).max()))
            # <A x, g> == <x, A^T g> from the device outputs, in float64: each side within what its bar allows
            lhs, rhs = (got_f[b, ..., :3] * g[j, b]).sum(), (y[b] * got_b[b, ..., :3]).sum()
            worst_i = max(worst_i, abs(lhs - rhs) / ((bar_f * np.abs(g[j, b])).sum() + (np.abs(y[b]) * bar_b).sum()))
    print(f'accuracy: spaa_blur_rows / spaa_blur_fwd / spaa_blur_bwd {hw} J={J}: largest |tap - float64| / bar = {worst_row:.3f}, |out - '
          f'float64| / bar = {worst_f:.3f}, |g_y - float64| / bar = {worst_b:.3f}, |<Ax,g> - <x,ATg>| / bar = {worst_i:.3f}')
    assert worst_row <= 1.0 and worst_f <= 1.0 and worst_b <= 1.0 and worst_i <= 1.0


@pytest.mark.parametrize('b,J', [(3, 2), (3, 3), (3, 4), (70, 4)])
@pytest.mark.parametrize('clean0', [0, 1])
def test_draw_three_iterations(hip, b, J, clean0):
    """Rows of t = 0, 1, 2 from three consecutive calls: the sigmas against the integer rule, the rows against the oracle's rows of the
    kernel's own sigmas, and spaa_blur_rows of those sigmas bit for bit; the counter reads 3; B = 70 x J = 4: more rows than the one
    workgroup has threads."""
    lib = hip['lib']
    seed = 0x9abc1234 if b == 3 else 5
    lo, hi = 0.5, 2.0
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    seen, worst_s, worst_t = [], 0.0, 0.0
    for t in range(3):
        buf, row = guarded((b, J, bo.ROW), -7.0)
        lib.call('spaa_blur_draw', seed, lib.ptr(counter), lo, hi, int(clean0), lib.ptr(row), b, J)
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == -7.0).all() and (buf[-GUARD:] == -7.0).all())
        got = row.cpu().numpy()
        want = bo.draw_sigmas(seed, t, b, J, lo, hi, clean0)
        worst_s = max(worst_s, float(np.abs(got[..., 0] - want).max() / bo.bar_sigma(lo, hi)))
        assert (got[:, 0, 0] == 0).all() if clean0 else (got[:, 0, 0] >= lo).all()
        assert (got[:, 1:, 0] >= lo).all() and (got[:, 1:, 0] <= hi).all()
        worst_t = max(worst_t, check_rows(got, got[..., 0]))
        assert torch.equal(bits(make_rows(lib, got[..., 0])), bits(row)), 'spaa_blur_rows and spaa_blur_draw make different rows'
        seen.append(got)
    assert int(counter.item()) == 3
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    print(f'accuracy: spaa_blur_draw B={b} J={J} clean0={clean0}: largest |sigma - rule| / bar = {worst_s:.3f}, |tap - float64| / bar = '
          f'{worst_t:.3f}; spaa_blur_rows of the drawn sigmas equal bit for bit (bar: exact)')
    assert worst_s <= 1.0 and worst_t <= 1.0


def test_draw_with_equal_ends_gives_exactly_that_sigma(hip):
    lib = hip['lib']
    counter = torch.full((1,), 41, dtype=torch.int32, device=DEV)
    for lo in (F32(1.3), F32(0.0), F32(2.5)):
        buf, row = guarded((5, 3, bo.ROW))
        lib.call('spaa_blur_draw', 9, lib.ptr(counter), float(lo), float(lo), 0, lib.ptr(row), 5, 3)
        assert (row[..., 0] == float(lo)).all() and guards_intact(buf)
        assert torch.equal(bits(row), bits(make_rows(lib, np.full((5, 3), lo, dtype=F32))))
    assert int(counter.item()) == 44
    print('accuracy: spaa_blur_draw lo == hi: every sigma is lo and every row spaa_blur_rows\'s, bit for bit (bar: exact)')


def test_invalid_arguments(hip):
    """J of 1 or 5, a null entry, a size below 1, n of 0, lo > hi, a negative or non-finite sigma and hi > 2.5 return
    hipErrorInvalidValue; nothing is launched (the outputs keep their fill, the counter its value)."""
    lib = hip['lib']
    raw = lib.load()
    H, W = 20, 28
    y_d = device_images(np.zeros((B, H, W, 3)))
    sg = torch.ones(B * 4, device=DEV)
    rows_buf, rows = guarded((B, 4, bo.ROW))
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = [torch.full((B, H, W, 4), SENTINEL, device=DEV) for _ in range(5)]
    p, arr, stream = lib.ptr, lib.ptr_array, lib._stream()
    ys = [y_d] * 5
    for J in (1, 5):
        assert raw.spaa_blur_draw(0, p(counter), 0.5, 2.0, 1, p(rows), B, J, stream) == HIP_INVALID_VALUE
        for name in ('spaa_blur_fwd', 'spaa_blur_bwd'):
            assert getattr(raw, name)(arr(ys[:J]), p(rows), J, arr(outs[:J]), B, H, W, stream) == HIP_INVALID_VALUE
    null2 = (C.c_void_p * 2)(outs[0].data_ptr(), None)
    y2, o2 = arr(ys[:2]), arr(outs[:2])
    for name in ('spaa_blur_fwd', 'spaa_blur_bwd'):
        fn = getattr(raw, name)
        for bad in ((None, p(rows), 2, o2), (null2, p(rows), 2, o2), (y2, None, 2, o2), (y2, p(rows), 2, None), (y2, p(rows), 2, null2)):
            assert fn(*bad, B, H, W, stream) == HIP_INVALID_VALUE
        for size in ((0, H, W), (B, 0, W), (B, H, 0), (-1, H, W), (65536, H, W), (B, 1 << 16, 1 << 15)):
            assert fn(y2, p(rows), 2, o2, *size, stream) == HIP_INVALID_VALUE
    for lo, hi in ((2.0, 0.5), (-0.5, 1.0), (0.5, 2.6), (float('nan'), 1.0), (0.5, float('nan')), (0.5, float('inf')), (float('-inf'), 1.0)):
        assert raw.spaa_blur_draw(0, p(counter), lo, hi, 1, p(rows), B, 2, stream) == HIP_INVALID_VALUE, (lo, hi)
    assert raw.spaa_blur_draw(0, None, 0.5, 2.0, 1, p(rows), B, 2, stream) == HIP_INVALID_VALUE
    assert raw.spaa_blur_draw(0, p(counter), 0.5, 2.0, 1, None, B, 2, stream) == HIP_INVALID_VALUE
    assert raw.spaa_blur_draw(0, p(counter), 0.5, 2.0, 1, p(rows), 0, 2, stream) == HIP_INVALID_VALUE
    for bad in ((None, p(rows), 4), (p(sg), None, 4), (p(sg), p(rows), 0), (p(sg), p(rows), -1)):
        assert raw.spaa_blur_rows(*bad, stream) == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and all((o == SENTINEL).all() for o in outs) and (rows_buf == SENTINEL).all()
