"""GPU: the pose kernels (csrc/pose_ops.hip) one by one against their float64 / integer restatement (tests/pose_oracle.py):
spaa_pose_draw over three consecutive iterations, spaa_pose_fwd and spaa_pose_bwd on planted tables (identity, integer and fractional
translations, the 16 limit corners, a shift off the frame) against grid_sample in float64 on the kernel's own fp32 table and autograd's
adjoint, spaa_jitter_fwd_each against spaa_jitter_fwd, and the argument errors.

The bars are derived, not measured: eps_c = 8 * 2^-24 * max(H, W) bounds the error of a source coordinate (at most 8 fp32 roundings at
magnitude at most max(H, W) in the stated evaluation order).  Forward: a bilinear sample moves by at most eps_c D per axis, D the
largest difference of adjacent pixels (the test images hold a 0 beside a 1, so D = 1, which also bounds the step from a border pixel to
the zero fill), plus 8 roundings of the weights and the four-term sum at magnitude <= 1.  Backward: at most 16 contributions per input
pixel (11 was the most found), each weight off by at most 2 eps_c, plus the roundings of the sum."""
import ctypes as C

import numpy as np
import pytest
import torch

import jitter_oracle as jo
import pose_oracle as po
from test_gpu_parity import hip  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(5, 7), (16, 17), (24, 32)]      # every pixel on or beside a border / crosses a 256-pixel block / several blocks
B = 3
HIP_INVALID_VALUE = 1
RANGES = (2.0, 0.03, 3.0, 0.02)            # rotate, zoom, shift, tilt
U = 2.0 ** -24


def _draw(lib, seed, counter, ranges, clean0, b, j, H, W):
    table = torch.full((b, j, 8), -7.0, device=DEV)
    lib.call('spaa_pose_draw', seed, lib.ptr(counter), *[float(r) for r in ranges], int(clean0), lib.ptr(table), b, j, H, W)
    return table.cpu().numpy()


@pytest.mark.parametrize('b,J', [(3, 2), (3, 3), (3, 4), (70, 4)])
@pytest.mark.parametrize('clean0', [0, 1])
def test_draw_three_iterations(hip, b, J, clean0):
    """Tables of t = 0, 1, 2 from three consecutive calls against the restatement: relative 5e-7 (8 ulp: the angle, sinf / cosf, the
    product) with an absolute floor of 1e-12; the counter reads 3; B = 70 x J = 4: more rows than the one workgroup has threads."""
    lib = hip['lib']
    seed = 0x9abc1234 if b == 3 else 5
    H, W = (24, 32) if b == 3 else (48, 20)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst, seen = 0.0, []
    for t in range(3):
        table = _draw(lib, seed, counter, RANGES, clean0, b, J, H, W)
        ref = po.draw_tables(seed, t, b, J, *RANGES, H, W, clean0)
        err = np.abs(table.astype(np.float64) - ref)
        worst = max(worst, (err / np.maximum(np.abs(ref), 1e-30)).max())
        assert (err <= 5e-7 * np.abs(ref) + 1e-12).all(), t
        if clean0:
            assert (table[:, 0] == np.array(po.IDENTITY_ROW, dtype=np.float32)).all()
        else:
            assert (table[:, 0, 0] != 1).any()
        seen.append(table)
    print(f'draw B={b} J={J} clean0={clean0}: max |table - float64| / |float64| = {worst:.3e}')
    assert int(counter.item()) == 3
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def _image(H, W, seed):
    """y [B][H][W][4]: uniform in [0, 1] with a band of exact 0s across a band of exact 1s (D = 1), garbage in the pad channel."""
    y = torch.rand(B, H, W, 4, generator=torch.Generator().manual_seed(seed))
    y[:, H // 2, :, :3] = 0.0
    y[:, :, W // 2, :3] = 1.0
    y[..., 3] = torch.tensor(float('nan'))
    y[0, 0, 0, 3] = 1e30
    return y


IDENTITY, PLUS1, MINUS2, OFF = 0, 1, 2, 3   # places of the exact rows in _planted_rows


def _planted_rows(H, W, J):
    """float32 [n][B][J][8], n launches' tables: the identity, the integer translations (+1, -2) and (-2, +1), a shift larger than the
    image, fractional translations of both signs, the 16 limit corners, and random poses within the limits to fill the last table."""
    rows = [po.IDENTITY_ROW, po.row_of(0, 0, 1.0, -2.0, 0, 0, H, W), po.row_of(0, 0, -2.0, 1.0, 0, 0, H, W),
            po.row_of(0, 0, W + 3.0, -(H + 2.0), 0, 0, H, W), po.row_of(0, 0, 0.3, -0.6, 0, 0, H, W),
            po.row_of(0, 0, -1.25, 1.75, 0, 0, H, W), po.row_of(0, 0, 2.5, 0.999, 0, 0, H, W)]
    rows += list(po.corner_rows(H, W))
    n = -(-len(rows) // (B * J))
    rows += list(po.random_rows(np.random.default_rng(H * W + J), n * B * J - len(rows), H, W, (10.0, 0.15, 3.0, 0.1)))
    return np.stack(rows).astype(np.float32).reshape(n, B, J, 8)


def _place(i, J):
    """(launch, sample, draw) of planted row i."""
    return i // (B * J), (i % (B * J)) // J, i % J


def _fwd(lib, y, table, J):
    H, W = y.shape[1:3]
    outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(J)]
    lib.call('spaa_pose_fwd', lib.ptr(y), lib.ptr(table), J, lib.ptr_array(outs), B, H, W)
    return outs


def _bwd(lib, g, table, J):
    H, W = g[0].shape[1:3]
    g_y = [torch.full((B, H, W, 4), 9.0, device=DEV) for _ in range(J)]
    lib.call('spaa_pose_bwd', lib.ptr_array(g), lib.ptr(table), J, lib.ptr_array(g_y), B, H, W)
    return g_y


def _shifted(a, dx, dy):
    """out[i][k] = a[i + dy][k + dx] with zero fill."""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    out[max(0, -dy):min(H, H - dy), max(0, -dx):min(W, W - dx)] = a[max(0, dy):min(H, H + dy), max(0, dx):min(W, W + dx)]
    return out


@pytest.mark.parametrize('J', [2, 3, 4])
@pytest.mark.parametrize('hw', SHAPES)
def test_forward_planted_tables(hip, hw, J):
    lib = hip['lib']
    H, W = hw
    tables = _planted_rows(H, W, J)
    y = _image(H, W, H * W + J)
    y_np = y.numpy()
    D = max(np.abs(np.diff(y_np[..., :3], axis=1)).max(), np.abs(np.diff(y_np[..., :3], axis=2)).max())
    assert D == 1.0
    bar = 2 * po.eps_c(H, W) * D + 8 * U
    y_d = y.to(DEV)
    got, worst = [], 0.0
    for table in tables:
        t_d = torch.from_numpy(table).to(DEV)
        outs = _fwd(lib, y_d, t_d, J)
        again = _fwd(lib, y_d, t_d, J)
        assert all(torch.equal(a, b) for a, b in zip(outs, again))             # two runs: bitwise
        o = np.stack([t.cpu().numpy() for t in outs])                          # [J][B][H][W][4]
        assert np.isfinite(o).all() and (o[..., 3] == 0).all()                 # the pad channel is written 0 whatever y's holds
        ref = po.forward(y_np, table.astype(np.float64))
        worst = max(worst, np.abs(o.astype(np.float64) - ref).max())
        got.append(o)
    print(f'forward {hw} J={J}: max |out - float64| = {worst:.3e}, bar {bar:.3e}')
    assert worst <= bar

    def at(i):
        n, b, j = _place(i, J)
        return got[n][j, b, ..., :3], y_np[b, ..., :3]
    o, src = at(IDENTITY)
    assert np.array_equal(o, src)                                               # the identity row: y bitwise
    o, src = at(PLUS1)
    assert np.array_equal(o, _shifted(src, 1, -2))                              # integer translations: the shifted copy, zero filled
    o, src = at(MINUS2)
    assert np.array_equal(o, _shifted(src, -2, 1))
    assert (at(OFF)[0] == 0).all()                                              # a shift larger than the image: all zero


@pytest.mark.parametrize('J', [2, 3, 4])
@pytest.mark.parametrize('hw', SHAPES)
def test_backward_against_the_float64_adjoint(hip, hw, J):
    lib = hip['lib']
    H, W = hw
    tables = _planted_rows(H, W, J)
    gen = torch.Generator().manual_seed(H + W + J)
    g_out = [torch.randn(B, H, W, 4, generator=gen) for _ in range(J)]          # (garbage in the pad channel: it is not read)
    u = _image(H, W, 7 * H + J)
    g_np = np.stack([g.numpy() for g in g_out])
    g_dev, u_d = [g.to(DEV) for g in g_out], u.to(DEV)
    gmax = np.abs(g_np[..., :3]).reshape(J, B, -1).max(axis=2)
    bar = 2 * po.eps_c(H, W) * 16 + 16 * U
    worst = worst_id = 0.0
    got_all = []
    for table in tables:
        t_d = torch.from_numpy(table).to(DEV)
        got = torch.stack(_bwd(lib, g_dev, t_d, J)).cpu()
        assert torch.equal(got, torch.stack(_bwd(lib, g_dev, t_d, J)).cpu())    # a gather: bitwise repeatable
        got = got.numpy()
        assert np.isfinite(got).all() and (got[..., 3] == 0).all()
        ref = po.backward(g_np, table.astype(np.float64))
        err = np.abs(got.astype(np.float64) - ref).reshape(J, B, -1).max(axis=2) / gmax
        worst = max(worst, err.max())
        # <W u, v> = <u, W^T v> from the two kernels' own outputs, summed in float64
        outs = np.stack([o.cpu().numpy() for o in _fwd(lib, u_d, t_d, J)]).astype(np.float64)[..., :3]
        for j in range(J):
            for b in range(B):
                prod = outs[j, b] * g_np[j, b, ..., :3].astype(np.float64)
                rhs = (u.numpy()[b, ..., :3].astype(np.float64) * got[j, b, ..., :3].astype(np.float64)).sum()
                if np.abs(prod).sum() > 0:
                    worst_id = max(worst_id, abs(prod.sum() - rhs) / np.abs(prod).sum())
                else:
                    assert rhs == 0
        got_all.append(got)
    print(f'backward {hw} J={J}: max |g_y - float64| / max |g_out| per (draw, sample) = {worst:.3e}, bar {bar:.3e}; '
          f'|<Wu,v> - <u,WTv>| / sum |Wu v| = {worst_id:.3e}')
    assert worst <= bar
    assert worst_id <= 1e-5

    def at(i):
        n, b, j = _place(i, J)
        return got_all[n][j, b, ..., :3], g_np[j, b, ..., :3]
    o, src = at(IDENTITY)
    assert np.array_equal(o, src)
    o, src = at(PLUS1)                                          # out[i][k] = y[i - 2][k + 1]: g_y[r][q] = g_out[r + 2][q - 1]
    assert np.array_equal(o, _shifted(src, -1, 2))
    assert (at(OFF)[0] == 0).all()                                              # an all-outside row gives zero


@pytest.mark.parametrize('hw', SHAPES)
def test_jitter_fwd_each_is_jitter_fwd(hip, hw):
    """With J equal input pointers spaa_jitter_fwd_each is spaa_jitter_fwd bit for bit (images and gate bytes, with and without the
    8-bit step); with J inputs of its own, draw j is what spaa_jitter_fwd makes of input j as its draw j."""
    lib = hip['lib']
    H, W = hw
    for J in (2, 3, 4):
        rng = np.random.default_rng(J)
        rows = np.zeros((B, J, 8), dtype=np.float32)
        rows[..., :3] = rng.uniform(0.85, 1.15, (B, J, 3))
        rows[..., 3] = rng.uniform(-0.04, 0.04, (B, J))
        rows[..., 4:6] = rng.uniform(-2, 2, (B, J, 2))
        rows[..., 6] = 0.02
        rows[0, 0] = jo.IDENTITY_ROW
        jit = torch.from_numpy(rows).to(DEV)
        key = torch.from_numpy(rng.integers(0, 2 ** 31, (B, J)).astype(np.int32)).to(DEV)
        ys = [_image(H, W, 10 * J + j).to(DEV) for j in range(J)]

        def run(name, y, quantize):
            outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(J)]
            gates = [torch.full((B, H * W), 255, dtype=torch.uint8, device=DEV) for _ in range(J)]
            lib.call(name, y, lib.ptr(jit), lib.ptr(key), J, quantize, lib.ptr_array(outs), lib.ptr_array(gates), B, H, W)
            return outs, gates
        for q in (0, 1):
            one = run('spaa_jitter_fwd', lib.ptr(ys[0]), q)
            each = run('spaa_jitter_fwd_each', lib.ptr_array([ys[0]] * J), q)
            assert all(torch.equal(a, b) for a, b in zip(one[0] + one[1], each[0] + each[1]))
            own = run('spaa_jitter_fwd_each', lib.ptr_array(ys), q)
            for j in range(J):
                ref = run('spaa_jitter_fwd', lib.ptr(ys[j]), q)
                assert torch.equal(own[0][j], ref[0][j]) and torch.equal(own[1][j], ref[1][j])


def test_invalid_arguments(hip):
    """J of 1 or 5, a null entry and a size < 1 return hipErrorInvalidValue; nothing is launched (the outputs keep their fill)."""
    lib = hip['lib']
    raw = lib.load()
    H, W = 5, 7
    y = _image(H, W, 1).to(DEV)
    table = torch.from_numpy(_planted_rows(H, W, 4)[0]).to(DEV)
    keep = table.clone()
    jit = torch.zeros(B, 4, 8, device=DEV)
    key = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(5)]
    gates = [torch.full((B, H * W), 255, dtype=torch.uint8, device=DEV) for _ in range(5)]
    p, arr, stream = lib.ptr, lib.ptr_array, lib._stream()
    for J in (1, 5):
        assert raw.spaa_pose_draw(0, p(counter), 2.0, 0.03, 3.0, 0.02, 1, p(table), B, J, H, W, stream) == HIP_INVALID_VALUE
        assert raw.spaa_pose_fwd(p(y), p(table), J, arr(outs[:J]), B, H, W, stream) == HIP_INVALID_VALUE
        assert raw.spaa_pose_bwd(arr(outs[:J]), p(table), J, arr(outs[:J]), B, H, W, stream) == HIP_INVALID_VALUE
        assert raw.spaa_jitter_fwd_each(arr(outs[:J]), p(jit), p(key), J, 0, arr(outs[:J]), arr(gates[:J]), B, H, W,
                                        stream) == HIP_INVALID_VALUE
    null2 = (C.c_void_p * 2)(outs[0].data_ptr(), None)
    nullg = (C.c_void_p * 2)(None, gates[1].data_ptr())
    assert raw.spaa_pose_fwd(p(y), p(table), 2, null2, B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_fwd(None, p(table), 2, arr(outs[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_fwd(p(y), None, 2, arr(outs[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_fwd(p(y), p(table), 2, None, B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_bwd(null2, p(table), 2, arr(outs[2:4]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_bwd(arr(outs[:2]), None, 2, arr(outs[2:4]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_bwd(arr(outs[:2]), p(table), 2, null2, B, H, W, stream) == HIP_INVALID_VALUE
    for b, h, w in ((0, H, W), (B, 0, W), (B, H, 0)):
        assert raw.spaa_pose_fwd(p(y), p(table), 2, arr(outs[:2]), b, h, w, stream) == HIP_INVALID_VALUE
        assert raw.spaa_pose_bwd(arr(outs[:2]), p(table), 2, arr(outs[2:4]), b, h, w, stream) == HIP_INVALID_VALUE
        assert raw.spaa_pose_draw(0, p(counter), 2.0, 0.03, 3.0, 0.02, 1, p(table), b, 2, h, w, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_draw(0, None, 2.0, 0.03, 3.0, 0.02, 1, p(table), B, 2, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_pose_draw(0, p(counter), 2.0, 0.03, 3.0, 0.02, 1, None, B, 2, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_fwd_each(null2, p(jit), p(key), 2, 0, arr(outs[2:4]), arr(gates[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_fwd_each(arr(outs[:2]), p(jit), p(key), 2, 0, null2, arr(gates[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_fwd_each(arr(outs[:2]), p(jit), p(key), 2, 0, arr(outs[2:4]), nullg, B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_fwd_each(None, p(jit), p(key), 2, 0, arr(outs[2:4]), arr(gates[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and torch.equal(table, keep)
    assert all((o == -3.0).all() for o in outs) and all((g == 255).all() for g in gates)
