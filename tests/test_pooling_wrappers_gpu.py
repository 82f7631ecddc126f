"""GPU (-m gpu): every wrapper of spaa_amd/pooling.py against the entry point it stands for, called directly with hand-written
arguments: bitwise-equal outputs, and the entry point the wrapper chose.  (What the entry points compute is checked against float64 in
tests/test_pool_ops_gpu.py.)  B = 2, 9 x 11, C = 8 -- ragged windows at the right and bottom edges, two channel quads -- and, for the
windowed forms, channels [8, 16) of a 16-wide buffer.  Output buffers start as NaN, so an element one side does not write shows."""
import pytest
import torch

from spaa_amd import pooling

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F16, F32, U8 = torch.float16, torch.float32, torch.uint8
B, H, W, C, CS, COFF = 2, 9, 11, 8, 16, 8
DTYPES = [pytest.param(F32, id='f32'), pytest.param(F16, id='f16')]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture
def calls(lib, monkeypatch):
    """Names of the entry points launched, in order."""
    names, call = [], lib.call
    monkeypatch.setattr(lib, 'call', lambda name, *a: (names.append(name), call(name, *a))[1])
    return names


def rnd(*shape, dt, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(device=DEV, dtype=dt)


def nan(*shape, dt):
    return torch.full(shape, float('nan'), device=DEV, dtype=dt)


def same(a, b):
    """Bitwise-equal tensors (NaN patterns included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(U8), b.contiguous().view(U8))


def sfx(dt):
    return '_f16' if dt == F16 else ''


def osz(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def max_pair(lib, dt, hw, k, s, p, cs, coff, entry):
    """Forward through wrapper and entry point; returns (x, pooled, arg) of the direct call after comparing."""
    h, w = hw
    ho, wo = osz(h, k, s, p), osz(w, k, s, p)
    x = rnd(B, h, w, C, dt=dt)
    o1, o2 = nan(B, ho, wo, cs, dt=dt), nan(B, ho, wo, cs, dt=dt)
    a1, a2 = torch.full((B, ho, wo, C), 255, device=DEV, dtype=U8), torch.full((B, ho, wo, C), 255, device=DEV, dtype=U8)
    pooling.maxpool_fwd(x, o1, a1, k, s, p, coff)
    if entry.startswith('spaa_maxpool3s2'):
        lib.call(entry, lib.hptr(x), lib.hptr(o2), lib.ptr(a2), B, h, w, C, ho, wo)
    else:
        lib.call(entry, lib.hptr(x), lib.hptr(o2), lib.ptr(a2), B, h, w, C, ho, wo, k, s, p, cs, coff)
    torch.cuda.synchronize()
    assert same(o1, o2) and same(a1, a2) and not o2[..., coff:coff + C].isnan().any() and int(a2.max()) < 255
    return x, o2, a2


MAX_CASES = [pytest.param(F32, (H, W), 3, 2, 1, C, 0, 'spaa_maxpool3s2', id='3s2p1-f32-whole'),
             pytest.param(F32, (H, W), 3, 2, 0, CS, COFF, 'spaa_maxpool', id='3s2p0-f32-window'),
             pytest.param(F16, (H, W), 3, 2, 0, CS, COFF, 'spaa_maxpool', id='3s2p0-f16-window'),
             pytest.param(F16, (H, W), 3, 2, 1, C, 0, 'spaa_maxpool', id='3s2p1-f16-whole'),      # (fp16 has no 3s2 pair: the generic kernel)
             pytest.param(F32, (H, W), 3, 2, 1, CS, COFF, 'spaa_maxpool', id='3s2p1-f32-window'),  # (nor has a window)
             pytest.param(F32, (8, 12), 2, 2, 0, C, 0, 'spaa_maxpool', id='2s2-f32'),
             pytest.param(F16, (8, 12), 2, 2, 0, C, 0, 'spaa_maxpool', id='2s2-f16')]


@pytest.mark.parametrize('dt,hw,k,s,p,cs,coff,family', MAX_CASES)
def test_maxpool(lib, calls, dt, hw, k, s, p, cs, coff, family):
    fwd, bwd = (family + '_fwd', family + '_bwd') if family.endswith('3s2') else (family + '_fwd' + sfx(dt), family + '_bwd' + sfx(dt))
    x, pooled, arg = max_pair(lib, dt, hw, k, s, p, cs, coff, fwd)
    assert calls == [fwd, fwd]
    if (hw, k, s, p) == ((H, W), 3, 2, 1):
        assert pooled.shape[1:3] == (5, 6)
    if (hw, k, s, p) == ((H, W), 3, 2, 0):
        assert pooled.shape[1:3] == (4, 5)
    g_out = rnd(*pooled.shape, dt=dt, seed=1)
    for gate in (False, True):
        g1, g2 = nan(*x.shape, dt=dt), nan(*x.shape, dt=dt)
        del calls[:]
        pooling.maxpool_bwd(g_out, arg, g1, k, s, p, gate, coff)
        args = (lib.hptr(g_out), lib.ptr(arg), int(gate), lib.hptr(g2), B, *hw, C, *pooled.shape[1:3])
        lib.call(bwd, *args) if family.endswith('3s2') else lib.call(bwd, *args, k, s, p, cs, coff)
        torch.cuda.synchronize()
        assert calls == [bwd, bwd] and same(g1, g2) and not g2.isnan().any() and float(g2.float().abs().max()) > 0
    # ConvPlan's unpool fallback names its channel count
    if (k, s, p) == (2, 2, 0):
        g1 = nan(*x.shape, dt=dt)
        pooling.maxpool_bwd(g_out, arg, g1, k, s, p, True, c=C)
        torch.cuda.synchronize()
        assert same(g1, g2)


@pytest.mark.parametrize('dt', DTYPES)
def test_avgpool2d(lib, calls, dt):
    x, g_out = rnd(B, H, W, C, dt=dt), rnd(B, H, W, CS, dt=dt, seed=1)
    o1, o2, g1, g2 = nan(B, H, W, CS, dt=dt), nan(B, H, W, CS, dt=dt), nan(B, H, W, C, dt=dt), nan(B, H, W, C, dt=dt)
    pooling.avgpool2d_fwd(x, o1, 3, 1, 1, COFF)
    lib.call('spaa_avgpool2d_fwd' + sfx(dt), lib.hptr(x), lib.hptr(o2), B, H, W, C, H, W, 3, 1, 1, CS, COFF)
    pooling.avgpool2d_bwd(g_out, g1, 3, 1, 1, COFF)
    lib.call('spaa_avgpool2d_bwd' + sfx(dt), lib.hptr(g_out), lib.hptr(g2), B, H, W, C, H, W, 3, 1, 1, CS, COFF)
    torch.cuda.synchronize()
    assert calls == ['spaa_avgpool2d_fwd' + sfx(dt)] * 2 + ['spaa_avgpool2d_bwd' + sfx(dt)] * 2
    assert same(o1, o2) and same(g1, g2) and not o2[..., COFF:].isnan().any() and o2[..., :COFF].isnan().all() and not g2.isnan().any()


@pytest.mark.parametrize('dt', DTYPES)
def test_global_avgpool(lib, calls, dt):
    x, g_feat = rnd(B, H, W, C, dt=dt), rnd(B, 1, 1, C, dt=F32, seed=1)
    f1, f2 = nan(B, 1, 1, C, dt=F32), nan(B, 1, 1, C, dt=F32)
    pooling.global_avgpool_fwd(x, f1)
    lib.call('spaa_avgpool_fwd' + sfx(dt), lib.hptr(x), lib.ptr(f2), B, H * W, C)
    torch.cuda.synchronize()
    assert H * W == 99 and same(f1, f2) and not f2.isnan().any()
    for act in (x, None):
        g1, g2 = nan(B, H, W, C, dt=dt), nan(B, H, W, C, dt=dt)
        pooling.global_avgpool_bwd(g_feat, act, g1)
        lib.call('spaa_avgpool_bwd' + sfx(dt), lib.ptr(g_feat), lib.hptr(act), lib.hptr(g2), B, H * W, C)
        torch.cuda.synchronize()
        assert same(g1, g2) and not g2.isnan().any() and bool((g2 == 0).any()) == (act is not None)
    assert calls == ['spaa_avgpool_fwd' + sfx(dt)] * 2 + ['spaa_avgpool_bwd' + sfx(dt)] * 4


def test_adaptive_avgpool(lib, calls):
    x, g_out = rnd(B, H, W, C, dt=F32), rnd(B, 7, 7, C, dt=F32, seed=1)
    o1, o2 = nan(B, 7, 7, C, dt=F32), nan(B, 7, 7, C, dt=F32)
    pooling.adaptive_avgpool_fwd(x, o1)
    lib.call('spaa_adaptive_avgpool_fwd', lib.ptr(x), lib.ptr(o2), B, H, W, C, 7, 7)
    torch.cuda.synchronize()
    assert same(o1, o2) and not o2.isnan().any()
    for gate in (None, x):
        g1, g2 = nan(B, H, W, C, dt=F32), nan(B, H, W, C, dt=F32)
        pooling.adaptive_avgpool_bwd(g_out, gate, g1)
        lib.call('spaa_adaptive_avgpool_bwd', lib.ptr(g_out), lib.ptr(gate), lib.ptr(g2), B, H, W, C, 7, 7)
        torch.cuda.synchronize()
        assert same(g1, g2) and not g2.isnan().any()
    assert calls == ['spaa_adaptive_avgpool_fwd'] * 2 + ['spaa_adaptive_avgpool_bwd'] * 4


@pytest.mark.parametrize('dt', DTYPES)
def test_gate_mask(lib, calls, dt):
    act = rnd(B, H, W, CS, dt=dt)
    m1, m2 = torch.full((B, H, W, CS // 4), 255, device=DEV, dtype=U8), torch.full((B, H, W, CS // 4), 255, device=DEV, dtype=U8)
    pooling.gate_mask(act, m1, C, COFF)
    lib.call('spaa_gate_mask', lib.hptr(act), int(dt == F16), lib.ptr(m2), B * H * W, C, CS, COFF)
    torch.cuda.synchronize()
    assert calls == ['spaa_gate_mask'] * 2 and same(m1, m2)
    assert torch.equal(m2[..., COFF // 4:], lib.pack_gate_mask(act[..., COFF:].float())) and bool((m2[..., :COFF // 4] == 255).all())
