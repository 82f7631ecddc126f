"""CPU: the float64 restatement of the fused shading tail and head (tests/shading_tail_oracle.py) on its own -- against torch.float64
autograd through conv_transpose2d / conv2d / relu / clamp, every mutation beyond the bars on the cases the GPU test runs
(tests/test_shading_tail_ops_gpu.py), the share of gate bits the bars leave out under its cap on every one of them, and the production
packing of the four weight images (spaa_amd.models.pack_tail) unpacked by their documented layouts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import shading_tail_oracle as so
from spaa_amd import models as M

CASES = so.cases()
F64 = torch.float64


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _close(a, b):
    return np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize('B,H2,W2', [(1, 1, 1), (3, 3, 5), (2, 9, 17)])
def test_restatement_equals_float64_autograd(B, H2, W2):
    """Forward: every intermediate.  Backward: the masks and the clamp gate are the forward's own, the cotangent is the select choice,
    and P6 is the gradient at the pre-activation of X6 (x6 = relu(pre6): `mask6` is its gate)."""
    rng = np.random.default_rng(17 * H2 + W2)
    w2, b2, w6, b6 = so.weights(1)
    ops = so.operands(w2, b2, w6, b6, 'f32')
    pre6 = rng.standard_normal((B, H2, W2, so.C6)).astype(np.float32)
    res1 = rng.uniform(-0.2, 1.2, (B, 2 * H2, 2 * W2, 4)).astype(np.float32)
    g_adv, g_col = (rng.standard_normal((B, 2 * H2, 2 * W2, 4)).astype(np.float32) for _ in range(2))
    state = rng.integers(1, 9, (B, 4)).astype(np.int32)
    state[:, 1] = np.arange(B) % 2
    # torch
    p6t = _nchw(pre6).requires_grad_(True)
    x7 = F.relu(F.conv_transpose2d(F.relu(p6t), torch.from_numpy(w2).to(F64), torch.from_numpy(b2).to(F64), stride=2))
    ypre = F.relu(F.conv2d(x7, torch.from_numpy(w6).to(F64), torch.from_numpy(b6).to(F64), padding=1) + _nchw(res1)[:, :3])
    y = torch.clamp(ypre, max=1.0)
    # the restatement
    r = so.tail(np.maximum(pre6, 0), res1, ops, 'f32')
    assert _close(r['x7'], _nhwc(x7)) and _close(r['ypre'], _nhwc(ypre)) and _close(r['y'], _nhwc(y))
    assert np.array_equal(so.unpack_bits(r['mask7'], so.C7), _nhwc(x7) > 0)
    yp = _nhwc(ypre)
    assert np.array_equal(r['gate_y'], so.pack_gate3((yp > 0) & (yp <= 1)))
    mask6 = so.pack_bits(pre6 > 0)
    ypre4 = np.concatenate([r['ypre'], np.full((B, 2 * H2, 2 * W2, 1), 7.0)], -1)
    for form, cot, kw in (('plain', g_adv, {}), ('select', np.where((state[:, 1] != 0)[:, None, None, None], g_col, g_adv), dict(state=state, g_col=g_col))):
        p6t.grad = None
        if form == 'plain':   # the cotangent of conv6's output as given: no clamp in the way
            pre = F.conv2d(x7, torch.from_numpy(w6).to(F64), padding=1)
            pre.backward(_nchw(cot)[:, :3], retain_graph=True)
            got = so.head(g_adv, r['mask7'], mask6, ops, 'f32')
            assert _close(got, _nhwc(p6t.grad))
        else:
            y.backward(_nchw(cot)[:, :3], retain_graph=True)
            for gate in (ypre4, r['gate_y']):
                assert _close(so.head(g_adv, r['mask7'], mask6, ops, 'f32', gate=gate, **kw), _nhwc(p6t.grad))


def test_clamp_gate_at_its_edges_is_autograd_s():
    """relu then clamp(max = 1) in torch passes a gradient exactly where 0 < pre <= 1: what `gate_y` and the select head restate."""
    pre = torch.tensor(so.PLANTED, dtype=torch.float32, requires_grad=True)
    torch.clamp(F.relu(pre), max=1.0).sum().backward()
    four = np.zeros((1, 1, len(so.PLANTED), 4))
    four[0, 0, :, 0] = np.maximum(np.array(so.PLANTED, dtype=np.float32), 0)
    assert np.array_equal(so.cotangent(np.ones_like(four), np.array([[5, 0, 5, 5]]), np.ones_like(four), four)[0, 0, :, 0], pre.grad.numpy().astype(np.float64))
    assert pre.grad.tolist() == [0, 0, 1, 0, 1, 0, 0]


def _bits_moved(a, b, sure, n):
    return bool(((so.unpack_bits(a, n) != so.unpack_bits(b, n)) & sure).any())


def tail_differs(r, fb, m):
    """Would the GPU test's forward assertions fail on `m` in place of the kernel's results?"""
    if any((np.abs(m[k] - r[k]) > fb['pre']).any() for k in ('y', 'ypre')):
        return True
    g = lambda d: (d['gate_y'][..., None] >> np.arange(3, dtype=np.uint8)) & 1
    return _bits_moved(m['mask7'], r['mask7'], fb['one7'] | fb['zero7'], so.C7) or bool(((g(m) != g(r)) & fb['gate_sure']).any())


@pytest.mark.parametrize('content,storage,B,H2,W2', CASES)
def test_left_out_share_and_every_mutation(content, storage, B, H2, W2):
    inp, ops = so.case_inputs(content, storage, B, H2, W2)
    r, fb = so.reference_fwd(content, storage, B, H2, W2)
    for k, share in fb['left_out'].items():
        assert share < so.LEFT_OUT_CAP, f'{k}: {share:.2e} of the bits lie within their bar of a gate edge'
    if inp['zero_image'] is not None:      # the planted image: no bar, every edge asserted
        z = inp['zero_image']
        assert (fb['pre'][z] == 0).all() and fb['gate_sure'][z].all() and fb['zero7'][z].all()
        assert np.array_equal(r['pre'][z], inp['res1'][z, ..., :3].astype(np.float64))
        assert all((inp['res1'][z, ..., :3] == np.float32(v)).any() for v in so.PLANTED)
    bwd = so.reference_bwd(content, storage, B, H2, W2)
    forms = so.head_forms(inp)
    nothing_to_convolve = not inp['x6'].any()          # (B = 1 'edges': the only image is the all-zero one)
    for name, (fns, storages, contents) in so.MUTATIONS.items():
        if storage not in storages or content not in contents:
            continue
        if 'tail' in fns and not (nothing_to_convolve and name not in ('relu_ge', 'clamp_lt')):
            assert tail_differs(r, fb, so.tail(inp['x6'], inp['res1'], ops, storage, _bug=name)), f'{name}: the tail stays within the bars'
        if 'head' in fns:
            moved = [form for form, kw in forms.items()
                     if (np.abs(so.head(inp['g_adv'], inp['mask7_in'], inp['mask6_in'], ops, storage, _bug=name, **kw) - bwd[form][0]) > bwd[form][1]).any()]
            want = {'relu_ge': ['select'], 'clamp_lt': ['select'], 'state_column_0': ['select', 'select_g'], 'g_adv_g_col_swapped': ['select', 'select_g']}
            assert moved == want.get(name, list(forms)), f'{name}: the head moves {moved}'


def test_bars_relate_to_the_measured_x6_figure():
    """The derived bf16x6 bar of transConv2's chain holds the measured 1.1e-6 of sum |W| |x| well inside, and is not built from it."""
    assert 1.1e-6 < so.U * (so.DROP + (6 * 64 + 1) * so.SPLIT) < 30 * 1.1e-6


@pytest.mark.parametrize('storage', so.STORAGES)
def test_production_packing_unpacks_to_the_raw_weights(storage):
    torch.manual_seed(5)
    sn = M.ShadingNetSPAA(False)
    wt, w6 = sn.transConv2.weight.detach(), sn.conv6.weight.detach()
    f16 = storage == 'f16'
    t = M.pack_tail(wt, w6, f16)
    routed = M.pcnet_routes(sn, False, 1, (16, 16), storage, device='cpu').tail
    assert set(routed) == set(t) | {'b2', 'b6'} and all(torch.equal(routed[k], t[k]) for k in t)      # the engine's images are these
    assert torch.equal(routed['b2'], sn.transConv2.bias.detach()) and torch.equal(routed['b6'], sn.conv6.bias.detach())

    def matrix(img, rows, cols):
        if f16:
            assert img.dtype == torch.float16 and tuple(img.shape) == (rows, cols)
            return img.double()
        assert img.dtype == torch.int16 and tuple(img.shape) == (3, rows, cols)      # cp.split_planes: bf16 h, m, l
        return img.view(torch.bfloat16).double().sum(0)

    want = (lambda w: w.half().double()) if f16 else (lambda w: w.double())
    w2 = matrix(t['w2'], 128, 64).reshape(2, 2, 32, 64).permute(3, 2, 0, 1)         # [32 (2 py + px) + c][k]
    w2t = matrix(t['w2t'], 64, 128).reshape(64, 2, 2, 32).permute(0, 3, 1, 2)       # [n][32 (2 py + px) + c]
    assert torch.equal(w2, want(wt)) and torch.equal(w2t, want(wt))
    assert t['w6'].dtype == (torch.float16 if f16 else torch.float32) and tuple(t['w6'].shape) == (3, 9, 32)
    assert torch.equal(t['w6'].double().reshape(3, 3, 3, 32).permute(0, 3, 1, 2), want(w6))      # [o][3 ky + kx][c]
    assert t['w6t'].dtype == torch.float32 and tuple(t['w6t'].shape) == (27, 32)                 # [3 t + o][c], taps mirrored: fp32 in both storages
    assert torch.equal(t['w6t'].reshape(3, 3, 3, 32).permute(2, 3, 0, 1).flip(2, 3), w6)
    # ... and the operand values the oracle works from are these images' values
    ops = so.operands(wt.numpy(), sn.transConv2.bias.detach().numpy(), w6.numpy(), sn.conv6.bias.detach().numpy(), storage)
    assert np.array_equal(ops['w2'], w2.numpy()) and np.array_equal(ops['w6'], want(w6).numpy()) and np.array_equal(ops['w6a'], w6.double().numpy())
