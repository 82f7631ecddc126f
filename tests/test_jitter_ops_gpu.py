"""GPU: the capture-jitter kernels (csrc/jitter_ops.hip) one by one against their float64 / integer restatement
(tests/jitter_oracle.py): spaa_jitter_draw over three consecutive iterations, spaa_jitter_fwd and spaa_jitter_bwd on planted tables
that hold integer, fractional and extreme shifts of both signs, and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import jitter_oracle as jo
from test_gpu_parity import hip  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(5, 7), (16, 17), (24, 32)]      # every pixel on or beside a border / crosses a 256-pixel block / several blocks
B = 3
HIP_INVALID_VALUE = 1
RANGES = (0.1, 0.03, 0.75, 0.01)           # gain, offset, shift, noise


def _draw(lib, seed, counter, ranges, clean0, b, j):
    jit = torch.full((b, j, 8), -7.0, device=DEV)
    key = torch.zeros(b, j, dtype=torch.int32, device=DEV)
    lib.call('spaa_jitter_draw', seed, lib.ptr(counter), *[float(r) for r in ranges], int(clean0), lib.ptr(jit), lib.ptr(key), b, j)
    return jit.cpu().numpy(), key.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('b,J', [(3, 2), (3, 3), (3, 4), (70, 4)])
@pytest.mark.parametrize('clean0', [0, 1])
def test_draw_three_iterations(hip, b, J, clean0):
    """Tables of t = 0, 1, 2 from three consecutive calls: keys exact, floats within 3e-7 (two roundings at magnitude 1), the counter
    reads 3; B = 70 x J = 4: more rows than the one workgroup has threads."""
    lib = hip['lib']
    seed = 0x9abc1234 if b == 3 else 5
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    seen = []
    for t in range(3):
        jit, key = _draw(lib, seed, counter, RANGES, clean0, b, J)
        ref_jit, ref_key = jo.draw_tables(seed, t, b, J, *RANGES, clean0)
        assert np.array_equal(key, ref_key), t
        worst = max(worst, np.abs(jit.astype(np.float64) - ref_jit).max())
        if clean0:
            assert (jit[:, 0] == np.array(jo.IDENTITY_ROW, dtype=np.float32)).all()
        else:
            assert (jit[:, 0, :3] != 1).any()
        assert (jit[..., 7] == 0).all()
        seen.append(jit)
    print(f'draw B={b} J={J} clean0={clean0}: max |table - float64| = {worst:.3e}')
    assert worst <= 3e-7
    assert int(counter.item()) == 3
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def _planted_rows(J, sigma):
    """[B][J][8]: per (sample, draw) a shift from the list (0, +1, -2, fractional of both signs, +-2 ends), gains != 1, offsets."""
    shifts = [(0.0, 0.0), (1.0, -2.0), (-2.0, 1.0), (0.3, -0.6), (-1.25, 1.75), (2.0, 2.0), (-2.0, -2.0), (1.5, -0.5), (-0.75, 0.0),
              (0.0, 2.0), (-1.0, -1.0), (0.999, -1.999)]
    rng = np.random.default_rng(J)
    rows = np.zeros((B, J, 8), dtype=np.float32)
    for b in range(B):
        for j in range(J):
            dx, dy = shifts[(b * J + j) % len(shifts)]
            rows[b, j] = (*rng.uniform(0.85, 1.15, 3), rng.uniform(-0.04, 0.04), dx, dy, sigma if (b + j) % 2 else sigma * 0.5, 0)
    rows[0, 0] = jo.IDENTITY_ROW
    return rows


def _image(H, W, seed):
    """y [B][H][W][4]: uniform in [0, 1] with a band of exact 0s and 1s, garbage in the pad channel."""
    y = torch.rand(B, H, W, 4, generator=torch.Generator().manual_seed(seed))
    y[:, H // 2, :, :3] = 0.0
    y[:, :, W // 2, :3] = 1.0
    y[..., 3] = torch.tensor(float('nan'))
    y[0, 0, 0, 3] = 1e30
    return y


def _fwd(lib, y, jit, key, J, quantize):
    H, W = y.shape[1:3]
    outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(J)]
    gates = [torch.full((B, H * W), 255, dtype=torch.uint8, device=DEV) for _ in range(J)]
    lib.call('spaa_jitter_fwd', lib.ptr(y), lib.ptr(jit), lib.ptr(key), J, int(quantize), lib.ptr_array(outs), lib.ptr_array(gates),
             B, H, W)
    return outs, gates


@pytest.mark.parametrize('J', [2, 3, 4])
@pytest.mark.parametrize('hw', SHAPES)
def test_forward_planted_tables(hip, hw, J):
    lib = hip['lib']
    H, W = hw
    worst = 0.0
    for sigma in (0.0, 0.02):
        rows = _planted_rows(J, sigma)
        key_np = np.array([[jo.draw_word(1, 0, b, j, jo.KEY) for j in range(J)] for b in range(B)], dtype=np.uint32)
        y = _image(H, W, H * W + J)
        y_d, jit_d = y.to(DEV), torch.from_numpy(rows).to(DEV)
        key_d = torch.from_numpy(key_np.view(np.int32)).to(DEV)
        outs, gates = _fwd(lib, y_d, jit_d, key_d, J, 0)
        ref, ref_gate, pre = jo.forward(y.numpy(), rows, key_np, False)
        got = np.stack([o.cpu().numpy() for o in outs])
        assert np.isfinite(got).all() and (got[..., 3] == 0).all()            # the pad channel is written 0 whatever y's holds
        err = np.abs(got.astype(np.float64) - ref).max()
        worst = max(worst, err)
        assert err <= 2e-6, (sigma, err)
        # the identity row (sample 0, draw 0; its sigma is 0 in both passes): y bitwise in the colour channels
        assert np.array_equal(got[0, 0, ..., :3], y.numpy()[0, ..., :3])
        # quantize = 1: floor(o 255) / 255 in fp32 of the quantize = 0 output, exactly
        outs_q, gates_q = _fwd(lib, y_d, jit_d, key_d, J, 1)
        for o, oq, g, gq in zip(outs, outs_q, gates, gates_q):
            want = torch.floor(o * 255.0) / torch.full((), 255.0, device=DEV)
            assert torch.equal(oq, want) and torch.equal(g, gq)
        got_gate = np.stack([g.cpu().numpy().reshape(B, H, W) for g in gates])
        assert (got_gate[0, 0] == 7).all() and (got_gate <= 7).all()          # (the identity draw: pre = y, inside everywhere)
        if sigma >= 0.005:
            # gate bytes of the noisy draws (pre is continuous there): the oracle's everywhere except where the float64 pre is within
            # 1e-5 of 0 or 1 (at most 0.1 % of the case)
            noisy = np.broadcast_to((rows[..., 6] >= 0.005).T[:, :, None, None], got_gate.shape)
            near = (np.minimum(np.abs(pre), np.abs(pre - 1)) < 1e-5).any(axis=-1)
            assert near[noisy].mean() <= 1e-3, near[noisy].mean()
            assert np.array_equal(got_gate[noisy & ~near], ref_gate[noisy & ~near])
            assert (ref_gate[noisy] != 7).any()
    print(f'forward {hw} J={J}: max |out - float64| = {worst:.3e}')


def test_forward_gate_case_is_continuous(hip):
    """The gate case of the issue on its own: sigma >= 0.005 in every row, so that pre is continuous and the excluded share small."""
    lib = hip['lib']
    H, W, J = 24, 32, 4
    rows = _planted_rows(J, 0.02)
    rows[0, 0] = (1.1, 0.9, 1.05, 0.02, 0.4, -0.3, 0.005, 0)
    assert (rows[..., 6] >= 0.005).all()
    key_np = np.arange(B * J, dtype=np.uint32).reshape(B, J) * np.uint32(2654435761)
    y = _image(H, W, 99)
    outs, gates = _fwd(lib, y.to(DEV), torch.from_numpy(rows).to(DEV), torch.from_numpy(key_np.view(np.int32)).to(DEV), J, 0)
    ref, ref_gate, pre = jo.forward(y.numpy(), rows, key_np, False)
    near = (np.minimum(np.abs(pre), np.abs(pre - 1)) < 1e-5).any(axis=-1)
    print(f'gate case: the oracle excludes {near.mean():.5f} of the pixels; gates != 7 at {(ref_gate != 7).mean():.3f}')
    assert near.mean() <= 1e-3
    got_gate = np.stack([g.cpu().numpy().reshape(B, H, W) for g in gates])
    assert np.array_equal(got_gate[~near], ref_gate[~near]) and (ref_gate != 7).mean() > 0.01


@pytest.mark.parametrize('J', [2, 3, 4])
@pytest.mark.parametrize('hw', SHAPES)
def test_backward_against_the_float64_adjoint(hip, hw, J):
    lib = hip['lib']
    H, W = hw
    rows = _planted_rows(J, 0.02)
    rows[B - 1, J - 1] = (1, 1, 1, 0.0, 1.0, -2.0, 0.0, 0)                    # an integer shift with unit gain: an exact shifted copy
    key_np = np.array([[jo.draw_word(2, 0, b, j, jo.KEY) for j in range(J)] for b in range(B)], dtype=np.uint32)
    y = _image(H, W, 7 * H + J)
    y[B - 1, ..., :3] = y[B - 1, ..., :3] * 0.5 + 0.25                          # (the copy draw: nothing clamped)
    jit_d = torch.from_numpy(rows).to(DEV)
    outs, gates = _fwd(lib, y.to(DEV), jit_d, torch.from_numpy(key_np.view(np.int32)).to(DEV), J, 1)
    gen = torch.Generator().manual_seed(H + W + J)
    g_out = [torch.randn(B, H, W, 4, generator=gen) for _ in range(J)]          # (garbage in the pad channel: it is not read)
    g_dev = [g.to(DEV) for g in g_out]

    def run():
        g_y = [torch.full((B, H, W, 4), 9.0, device=DEV) for _ in range(J)]
        lib.call('spaa_jitter_bwd', lib.ptr_array(g_dev), lib.ptr(jit_d), lib.ptr_array(gates), J, lib.ptr_array(g_y), B, H, W)
        return torch.stack(g_y).cpu()
    got = run()
    again = run()
    assert torch.equal(got, again)                                              # a gather: bitwise repeatable
    gate_np = np.stack([g.cpu().numpy().reshape(B, H, W) for g in gates])       # the kernel's own gate bytes
    ref = jo.backward(np.stack([g.numpy() for g in g_out]), rows, gate_np)
    got = got.numpy()
    assert (got[..., 3] == 0).all()
    err = np.abs(got.astype(np.float64) - ref).reshape(J, B, -1).max(axis=2) / np.abs(ref).reshape(J, B, -1).max(axis=2)
    print(f'backward {hw} J={J}: max |g_y - float64| / max |ref| per (draw, sample) = {err.max():.3e}')
    assert (err <= 2e-6).all()
    # the copy draw: out[i][k] = y[i - 2][k + 1], so g_y[r][q] = g_out[r + 2][q - 1] away from the border
    assert (gate_np[J - 1, B - 1] == 7).all()
    copy, src = got[J - 1, B - 1, ..., :3], g_out[J - 1][B - 1, ..., :3].numpy()
    assert np.array_equal(copy[1:H - 3, 2:W - 1], src[3:H - 1, 1:W - 2])


def test_invalid_arguments(hip):
    """J of 1 or 5, and a null entry, return hipErrorInvalidValue; nothing is launched (the outputs keep their fill)."""
    lib = hip['lib']
    raw = lib.load()
    H, W = 5, 7
    y = _image(H, W, 1).to(DEV)
    jit = torch.from_numpy(_planted_rows(4, 0.0)).to(DEV)
    key = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = [torch.full((B, H, W, 4), -3.0, device=DEV) for _ in range(5)]
    gates = [torch.full((B, H * W), 255, dtype=torch.uint8, device=DEV) for _ in range(5)]
    p, arr, stream = lib.ptr, lib.ptr_array, lib._stream()
    for J in (1, 5):
        assert raw.spaa_jitter_draw(0, p(counter), 0.1, 0.1, 0.1, 0.1, 1, p(jit), p(key), B, J, stream) == HIP_INVALID_VALUE
        assert raw.spaa_jitter_fwd(p(y), p(jit), p(key), J, 0, arr(outs[:J]), arr(gates[:J]), B, H, W, stream) == HIP_INVALID_VALUE
        assert raw.spaa_jitter_bwd(arr(outs[:J]), p(jit), arr(gates[:J]), J, arr(outs[:J]), B, H, W, stream) == HIP_INVALID_VALUE
    null2 = (C.c_void_p * 2)(outs[0].data_ptr(), None)
    nullg = (C.c_void_p * 2)(None, gates[1].data_ptr())
    assert raw.spaa_jitter_fwd(p(y), p(jit), p(key), 2, 0, null2, arr(gates[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_fwd(p(y), p(jit), p(key), 2, 0, arr(outs[:2]), nullg, B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_fwd(None, p(jit), p(key), 2, 0, arr(outs[:2]), arr(gates[:2]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_bwd(null2, p(jit), arr(gates[:2]), 2, arr(outs[2:4]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_bwd(arr(outs[:2]), p(jit), nullg, 2, arr(outs[2:4]), B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_bwd(arr(outs[:2]), p(jit), arr(gates[:2]), 2, null2, B, H, W, stream) == HIP_INVALID_VALUE
    assert raw.spaa_jitter_draw(0, None, 0.1, 0.1, 0.1, 0.1, 1, p(jit), p(key), B, 2, stream) == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert int(counter.item()) == 0 and all((o == -3.0).all() for o in outs) and all((g == 255).all() for g in gates)
