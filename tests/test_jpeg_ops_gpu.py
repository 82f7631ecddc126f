"""GPU: the JPEG kernels (csrc/jpeg_ops.hip) one by one, through the C ABI, against their float64 / integer restatement
(tests/jpeg_oracle.py) on the cases of tests/jpeg_cases.py: B = 3 float images per shape, J = 2, 3, 4 draws, planted quality rows that
mix the identity row with Q = 1, 50, 75 and 100, both subsamplings.

Forward: a block whose nearest c / T is within 1e-3 of a half-integer is left out with the pixels that read it (a condition on the
case, at most 10 % of the blocks: tests/test_jpeg_cpu.py checks it without a GPU); everywhere else the output is the oracle's exactly,
except that a pixel whose pre-round value is within 1e-3 of a rounding boundary (at most 2 % of them) may be one level off.  Adjoint:
both gradient modes within jpeg_oracle.bar_adjoint, with the kernel's own gate bytes.  Every test prints its largest error over the bar
as an `accuracy:` line (profiles/jpeg_accuracy.txt holds the lines of one run)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_oracle as jp
from test_gpu_parity import hip  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = jc.B
HIP_INVALID_VALUE = 1
CODES = {'4:4:4': 0, '4:2:0': 2}
SUBS = ('4:4:4', '4:2:0')


@functools.lru_cache(maxsize=None)
def reference(hw, J, sub):
    """The oracle's round trips of a case, computed once: (y, rows, [[forward dict of (b, j)]])."""
    y, rows = jc.inputs(hw, J)
    return y, rows, [[jp.forward(y[b], int(rows[b, j, 0]), sub) for j in range(J)] for b in range(B)]


def _device_images(y):
    """[B][H][W][4] fp32 on the GPU with garbage in the pad channel."""
    y4 = torch.full(y.shape[:3] + (4,), float('nan'))
    y4[..., :3] = torch.from_numpy(y).float()
    y4[0, 0, 0, 3] = 1e30
    return y4.to(DEV)


def _workspace(lib, code, J, H, W):
    n = lib.load().spaa_jpeg_ws_floats(code, J, B, H, W)
    return torch.full((n,), float('nan'), device=DEV) if n else None


def _fwd(lib, ys, rows_d, J, code, H, W):
    outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(J)]
    gates = [torch.full((B, H * W), 255, dtype=torch.uint8, device=DEV) for _ in range(J)]
    lib.call('spaa_jpeg_fwd', lib.ptr_array(ys), lib.ptr(rows_d), J, code, lib.ptr_array(outs), lib.ptr_array(gates),
             lib.ptr(_workspace(lib, code, J, H, W)), B, H, W)
    return outs, gates


def _bwd(lib, g_dev, ys, rows_d, J, code, soft, gates, H, W):
    g_y = [torch.full((B, H, W, 4), 9.0, device=DEV) for _ in range(J)]
    lib.call('spaa_jpeg_bwd', lib.ptr_array(g_dev), lib.ptr_array(ys), lib.ptr(rows_d), J, code, int(soft), lib.ptr_array(gates),
             lib.ptr_array(g_y), B, H, W)
    return g_y


@pytest.mark.parametrize('J', jc.DRAWS)
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('hw', jc.SHAPES)
def test_forward_against_the_oracle(hip, hw, sub, J):
    lib = hip['lib']
    H, W = hw
    y, rows, ref = reference(hw, J, sub)
    y_d = _device_images(y)
    rows_d = torch.from_numpy(rows).to(DEV)
    outs, gates = _fwd(lib, [y_d] * J, rows_d, J, CODES[sub], H, W)
    again, gates2 = _fwd(lib, [y_d] * J, rows_d, J, CODES[sub], H, W)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)) and all(torch.equal(a, b) for a, b in zip(gates, gates2))   # repeatable
    copies = [y_d.clone() for _ in range(J)]
    each, gates3 = _fwd(lib, copies, rows_d, J, CODES[sub], H, W)
    assert all(torch.equal(a, b) for a, b in zip(outs, each)) and all(torch.equal(a, b) for a, b in zip(gates, gates3))    # J equal pointers
    left_out = near_share = 0.0
    wrong = off_by_one = 0
    for j in range(J):
        got = outs[j].cpu().numpy()
        gate = gates[j].cpu().numpy().reshape(B, H, W)
        assert np.isfinite(got).all() and (got[..., 3] == 0).all()
        for b in range(B):
            fw = ref[b][j]
            if int(rows[b, j, 0]) == 0:
                assert np.array_equal(got[b, ..., :3], y[b].astype(np.float32)) and (gate[b] == 0x77).all()
                continue
            safe = jp.safe_pixels(fw, H, W, sub)
            share = jp.unsafe_block_fraction(fw)
            near = (jp.round_distance(fw['v']) < jp.ROUND_MARGIN).any(axis=-1)
            left_out, near_share = max(left_out, share), max(near_share, float((near & safe).mean()))
            assert share <= jc.MAX_UNSAFE_BLOCKS and (near & safe).mean() <= jc.MAX_NEAR_PIXELS, 'the case itself breaks its condition'
            want = np.rint(fw['out'] * 255.0)
            level = np.rint(got[b, ..., :3].astype(np.float64) * 255.0)
            assert np.array_equal(got[b, ..., :3], (level.astype(np.float32) / np.float32(255.0)))      # on the 8-bit grid
            diff = np.abs(level - want).max(axis=-1)
            wrong += int((diff[safe & ~near] != 0).sum())
            off_by_one = max(off_by_one, int(diff[safe & near].max(initial=0)))
            # the gate byte: in-gates exactly (y is fp32 on both sides), out-gates where v keeps 1e-3 from 0 and 255
            assert np.array_equal(gate[b] & 7, fw['gate'] & 7)
            clear = (np.minimum(np.abs(fw['v']), np.abs(fw['v'] - 255.0)) > jp.ROUND_MARGIN).all(axis=-1) & safe
            assert np.array_equal((gate[b] >> 4)[clear], (fw['gate'] >> 4)[clear]) and (gate[b] & 0x88 == 0).all()
    print(f'accuracy: spaa_jpeg_fwd {hw} {sub} J={J}: {wrong} pixels off outside the margins (bar 0), largest difference inside the '
          f'rounding margin {off_by_one} level (bar 1); blocks left out {left_out:.1%}, pixels in the margin {near_share:.2%}')
    assert wrong == 0 and off_by_one <= 1


@pytest.mark.parametrize('gradient', ['soft', 'straight'])
@pytest.mark.parametrize('J', jc.DRAWS)
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('hw', jc.SHAPES)
def test_adjoint_against_the_oracle(hip, hw, sub, J, gradient):
    lib = hip['lib']
    H, W = hw
    y, rows, ref = reference(hw, J, sub)
    y_d = _device_images(y)
    rows_d = torch.from_numpy(rows).to(DEV)
    outs, gates = _fwd(lib, [y_d] * J, rows_d, J, CODES[sub], H, W)
    gen = torch.Generator().manual_seed(H + W + J)
    g_out = [torch.randn(B, H, W, 4, generator=gen) for _ in range(J)]          # (garbage in the pad channel: it is not read)
    g_dev = [g.to(DEV) for g in g_out]
    soft = gradient == 'soft'
    g_y = _bwd(lib, g_dev, [y_d] * J, rows_d, J, CODES[sub], soft, gates, H, W)
    again = _bwd(lib, g_dev, [y_d] * J, rows_d, J, CODES[sub], soft, gates, H, W)
    assert all(torch.equal(a, b) for a, b in zip(g_y, again))                   # a gather: bitwise repeatable
    each = _bwd(lib, g_dev, [y_d.clone() for _ in range(J)], rows_d, J, CODES[sub], soft, gates, H, W)
    assert all(torch.equal(a, b) for a, b in zip(g_y, each))                    # J equal pointers
    worst = 0.0
    for j in range(J):
        got = g_y[j].cpu().numpy().astype(np.float64)
        gate = gates[j].cpu().numpy().reshape(B, H, W)                          # the kernel's own gate bytes
        assert (got[..., 3] == 0).all()
        for b in range(B):
            Q = int(rows[b, j, 0])
            g = g_out[j][b, ..., :3].numpy().astype(np.float64)
            if Q == 0:
                assert np.array_equal(got[b, ..., :3], g)
                continue
            bits = (np.stack([(gate[b] >> c) & 1 for c in range(3)], axis=-1).astype(bool),
                    np.stack([(gate[b] >> (4 + c)) & 1 for c in range(3)], axis=-1).astype(bool))
            want = jp.adjoint(g, y[b], Q, sub, gradient, gates=bits)
            bar = jp.bar_adjoint(g, y[b], Q, sub, gradient, gates=bits) + 1e-30
            safe = jp.safe_pixels(ref[b][j], H, W, sub)
            over = (np.abs(got[b, ..., :3] - want) / bar)[safe].max()
            worst = max(worst, float(over))
            assert np.abs(want[safe]).max() > 0
    print(f'accuracy: spaa_jpeg_bwd {hw} {sub} J={J} {gradient}: largest |g_y - float64| / bar = {worst:.3f}')
    assert worst <= 1.0


@pytest.mark.parametrize('b,J', [(3, 2), (3, 3), (3, 4), (70, 4)])
@pytest.mark.parametrize('clean0', [0, 1])
def test_draw_three_iterations(hip, b, J, clean0):
    """Rows of t = 0, 1, 2 from three consecutive calls against the integer rule, exactly; the counter reads 3; B = 70 x J = 4: more
    rows than the one workgroup has threads."""
    lib = hip['lib']
    seed = 0x9abc1234 if b == 3 else 5
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    seen = []
    for t in range(3):
        row = torch.full((b, J, 4), -7.0, device=DEV)
        lib.call('spaa_jpeg_draw', seed, lib.ptr(counter), 60, 95, int(clean0), lib.ptr(row), b, J)
        got = row.cpu().numpy()
        assert np.array_equal(got, jp.draw_rows(seed, t, b, J, 60, 95, clean0)), t
        assert (got[:, 0, 0] == 0).all() if clean0 else (got[:, 0, 0] >= 60).all()
        seen.append(got)
    assert int(counter.item()) == 3
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    print(f'accuracy: spaa_jpeg_draw B={b} J={J} clean0={clean0}: three iterations equal to the integer rule (bar: exact)')


def test_invalid_arguments(hip):
    """J of 1 or 5, a null entry, another subsampling code, 4:2:0 without its workspace and a quality range outside 1..100 return
    hipErrorInvalidValue; nothing is launched (the outputs keep their fill)."""
    lib = hip['lib']
    raw = lib.load()
    H, W = 20, 28
    y, rows = jc.inputs((H, W), 4)
    y_d = _device_images(y)
    rows_d = torch.from_numpy(rows).to(DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(5)]
    gates = [torch.full((B, H * W), 255, dtype=torch.uint8, device=DEV) for _ in range(5)]
    ws = torch.full((raw.spaa_jpeg_ws_floats(2, 4, B, H, W),), -3.0, device=DEV)
    p, arr, stream = lib.ptr, lib.ptr_array, lib._stream()
    ys = [y_d] * 5
    for J in (1, 5):
        assert raw.spaa_jpeg_draw(0, p(counter), 60, 95, 1, p(rows_d), B, J, stream) == HIP_INVALID_VALUE
        assert raw.spaa_jpeg_fwd(arr(ys[:J]), p(rows_d), J, 2, arr(outs[:J]), arr(gates[:J]), p(ws), B, H, W, stream) == HIP_INVALID_VALUE
        assert raw.spaa_jpeg_bwd(arr(outs[:J]), arr(ys[:J]), p(rows_d), J, 2, 1, arr(gates[:J]), arr(outs[:J]), B, H, W, stream) == HIP_INVALID_VALUE
    null2 = (C.c_void_p * 2)(outs[0].data_ptr(), None)
    nullg = (C.c_void_p * 2)(None, gates[1].data_ptr())
    o2, g2, y2 = arr(outs[:2]), arr(gates[:2]), arr(ys[:2])
    for bad in ((null2, p(rows_d), 2, 2, o2, g2, p(ws)), (y2, None, 2, 2, o2, g2, p(ws)), (y2, p(rows_d), 2, 2, null2, g2, p(ws)),
                (y2, p(rows_d), 2, 2, o2, nullg, p(ws)), (y2, p(rows_d), 2, 2, o2, g2, None), (y2, p(rows_d), 2, 1, o2, g2, p(ws)),
                (y2, p(rows_d), 2, 3, o2, g2, p(ws))):
        assert raw.spaa_jpeg_fwd(*bad, B, H, W, stream) == HIP_INVALID_VALUE
    for size in ((0, H, W), (B, 0, W), (B, H, 0)):
        assert raw.spaa_jpeg_fwd(y2, p(rows_d), 2, 2, o2, g2, p(ws), *size, stream) == HIP_INVALID_VALUE
        assert raw.spaa_jpeg_bwd(o2, y2, p(rows_d), 2, 2, 1, g2, arr(outs[2:4]), *size, stream) == HIP_INVALID_VALUE
    g_y = arr(outs[2:4])
    for bad in ((null2, y2, p(rows_d), 2, 2, 1, g2, g_y), (o2, null2, p(rows_d), 2, 2, 1, g2, g_y), (o2, y2, None, 2, 2, 1, g2, g_y),
                (o2, y2, p(rows_d), 2, 2, 1, nullg, g_y), (o2, y2, p(rows_d), 2, 2, 1, g2, null2), (o2, y2, p(rows_d), 2, 1, 1, g2, g_y)):
        assert raw.spaa_jpeg_bwd(*bad, B, H, W, stream) == HIP_INVALID_VALUE
    for lo, hi in ((0, 95), (60, 101), (95, 60)):
        assert raw.spaa_jpeg_draw(0, p(counter), lo, hi, 1, p(rows_d), B, 2, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jpeg_draw(0, None, 60, 95, 1, p(rows_d), B, 2, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jpeg_draw(0, p(counter), 60, 95, 1, None, B, 2, stream) == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and all((o == -3.0).all() for o in outs) and all((g == 255).all() for g in gates)
    assert (ws == -3.0).all() and np.array_equal(rows_d.cpu().numpy(), rows)
