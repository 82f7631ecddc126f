"""GPU: the entry points of the fused shading tail and head (csrc/shading_tail.hip) alone, through the C-ABI, against their float64
restatement (tests/shading_tail_oracle.py): spaa_shading_tail_fwd, _g, _f16, _f16_g, spaa_shading_head_bwd, _f16, _select, _select_g,
_select_f16, _select_f16_g.  No PCNetEngine: the weight images come from spaa_amd.models.pack_tail, the masks from
_lib.pack_gate_mask.

Shapes (B, H2, W2), each in both storages (shading_tail_oracle.SHAPES): (1, 1, 1) every pixel a border, one tile; (2, 6, 14) one forward
tile, one column short of full; (2, 7, 15) H + 1 = 15 and W + 1 = 31: a second forward tile of one row and one column; (1, 8, 16) one
full head tile; (2, 9, 17) one X6 row and column over a head tile, ragged forward tiles; (3, 5, 23) odd sizes; and (B*, 9, 17) with
B* from the device's compute units so that both kernels have more tiles than their grid has workgroups (131 images on 256 units: 524
tiles against 256 and 512): some workgroups walk a second tile -- the next tile's prefetch, the barrier that does not wait for global
memory, the reuse of the LDS tile.  Contents: 'random' and 'edges' (one image with X6 = 0 and b2 = b6 = 0, res1 planted with 0, -0.0, 1,
its two neighbours, -1e-30 and 2: on it the outputs are compared bitwise).

The bars are the oracle's (derived in its docstring, none set from what a kernel produced); tests/test_shading_tail_cpu.py shows that
each deliberate mistake of shading_tail_oracle.MUTATIONS exceeds them on these cases.  Outputs start as NaN / 0xA5 inside allocations
with guard bands of at least an image row: no prefill may remain, the guards and the inputs stay as they were, and a second launch
gives the same bits.  Every test prints its largest error / bar (profiles/shading_tail_accuracy.txt holds the lines of one run)."""
import ctypes

import numpy as np
import pytest
import torch

import shading_tail_oracle as so

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HIP_INVALID_VALUE = 1
PARAMS = [(c, s, B, h2, w2) for B, h2, w2 in so.SHAPES for s in so.STORAGES for c in so.CONTENTS]
IDS = [f'{c}-{s}-{"walk" if B is None else B}x{h2}x{w2}' for c, s, B, h2, w2 in PARAMS]
TAIL = {'f32': ('spaa_shading_tail_fwd', 'spaa_shading_tail_fwd_g'), 'f16': ('spaa_shading_tail_fwd_f16', 'spaa_shading_tail_fwd_f16_g')}
HEAD = {'f32': ('spaa_shading_head_bwd', 'spaa_shading_head_bwd_select', 'spaa_shading_head_bwd_select_g'),
        'f16': ('spaa_shading_head_bwd_f16', 'spaa_shading_head_bwd_select_f16', 'spaa_shading_head_bwd_select_f16_g')}


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib, models
    return dict(lib=_lib, models=models, cus=torch.cuda.get_device_properties(0).multi_processor_count)


def report(name, ratio):
    print(f'[tail] {name}: max error / bar = {ratio:.4f}')


class Guarded:
    """An output tensor inside a larger allocation: `guard` elements (at least one image row, a multiple of 16 bytes: the inside keeps the
    allocation's alignment) before and after, everything prefilled with NaN (floats) or 0xA5 (bytes)."""

    def __init__(self, shape, dtype, row):
        item = torch.empty((), dtype=dtype).element_size()
        self.guard = -(-row * item // 16) * 16 // item
        n = int(np.prod(shape))
        self.raw = torch.empty(n + 2 * self.guard, dtype=dtype, device=DEV)
        self.raw.fill_(0xA5 if dtype == torch.uint8 else float('nan'))
        self.before = self.raw.cpu()
        self.t = self.raw[self.guard:self.guard + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0

    def check(self, name):
        """No prefill inside, the guards as they were; returns the inside on the CPU."""
        now, g = self.raw.cpu(), self.guard
        same = (lambda a, b: torch.equal(a.view(torch.uint8), b.view(torch.uint8)))
        assert same(now[:g], self.before[:g]) and same(now[-g:], self.before[-g:]), f'{name}: written outside the tensor'
        inside = now[g:-g].view(*self.t.shape)
        left = (inside == 0xA5) if inside.dtype == torch.uint8 else torch.isnan(inside)
        assert not left.any(), f'{name}: {int(left.sum())} elements were never written'
        return inside

    def untouched(self):
        return torch.equal(self.raw.cpu().view(torch.uint8), self.before.view(torch.uint8))


def setup(hip, content, storage, B, H2, W2):
    """The case's inputs on the GPU (and their CPU originals, for the unchanged-inputs check), the packed weights, the shapes."""
    if B is None:
        B = so.walk_batch(hip['cus'])
        assert 4 * B > 2 * hip['cus'] + 8
        assert so.fwd_tiles(B, H2, W2) == so.bwd_tiles(B, H2, W2) == 4 * B > 2 * hip['cus']      # more tiles than either grid has slots
    inp, _ = so.case_inputs(content, storage, B, H2, W2)
    lib, f16 = hip['lib'], storage == 'f16'
    pk = hip['models'].pack_tail(torch.from_numpy(inp['w2']), torch.from_numpy(inp['w6']), f16)
    host = {k: torch.from_numpy(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    host.update(pk)
    # the masks as _lib.pack_gate_mask makes them from an activation with these signs
    dev = {k: v.to(DEV) for k, v in host.items()}
    for k, n in (('mask7_in', so.C7), ('mask6_in', so.C6)):
        act = torch.from_numpy(so.unpack_bits(inp[k], n)).float().to(DEV) * 2 - 1
        dev[k] = lib.pack_gate_mask(act)
        assert torch.equal(dev[k].cpu(), host[k])
    w = lib.hptr if f16 else lib.ptr
    return dict(B=B, H2=H2, W2=W2, H=2 * H2, W=2 * W2, f16=f16, inp=inp, host=host, dev=dev, p=lib.ptr, w=w, lib=lib,
                case=(content, storage, B, H2, W2))


def inputs_unchanged(s):
    for k, v in s['host'].items():
        assert torch.equal(s['dev'][k].cpu().view(torch.uint8), v.view(torch.uint8)), f'input {k} was written'


def tail_launch(s, gate, with_ypre=True):
    """One forward launch into fresh guarded outputs; returns dict(y, ypre, mask7, gate_y) of CPU tensors (None where not asked for)."""
    B, H, W, d, p = s['B'], s['H'], s['W'], s['dev'], s['p']
    out = dict(y=Guarded((B, H, W, 4), torch.float32, 4 * W), ypre=Guarded((B, H, W, 4), torch.float32, 4 * W) if with_ypre else None,
               mask7=Guarded((B, H, W, so.C7 // 4), torch.uint8, W * so.C7 // 4), gate_y=Guarded((B, H, W), torch.uint8, W) if gate else None)
    args = [s['lib'].hptr(d['x6']), s['w'](d['w2']), p(d['b2']), s['w'](d['w6']), p(d['b6']), p(d['res1']), p(out['y'].t),
            p(out['ypre'].t) if with_ypre else None, p(out['mask7'].t)]
    name = TAIL['f16' if s['f16'] else 'f32'][1 if gate else 0]
    s['lib'].call(name, *args, *([p(out['gate_y'].t)] if gate else []), B, s['H2'], s['W2'])
    torch.cuda.synchronize()
    return name, {k: (g.check(f'{name} {k}') if g is not None else None) for k, g in out.items()}


def same(x, y):
    """Bitwise equal (-0.0 is not 0.0)."""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def bits3(ypre):
    ok = (ypre[..., :3] > 0) & (ypre[..., :3] <= 1)
    return ok[..., 0].to(torch.uint8) | (ok[..., 1].to(torch.uint8) << 1) | (ok[..., 2].to(torch.uint8) << 2)


def ratio_under(name, got, ref, bar):
    err = np.abs(got.double().numpy() - ref)
    ok = err <= bar
    assert ok.all(), f'{name}: {int((~ok).sum())} of {ok.size} beyond the bar, the worst {np.nanmax(err / np.maximum(bar, 1e-300)):.3f} of it (NaN: {int(np.isnan(err).sum())})'
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


@pytest.mark.parametrize('content,storage,B,H2,W2', PARAMS, ids=IDS)
def test_tail_forward(hip, content, storage, B, H2, W2):
    s = setup(hip, content, storage, B, H2, W2)
    r, fb = so.reference_fwd(*s['case'])
    (plain, a), (gname, b), (_, c) = tail_launch(s, False), tail_launch(s, True), tail_launch(s, True, with_ypre=False)
    inputs_unchanged(s)
    # across the forms, bitwise
    assert same(a['y'], b['y']) and same(a['y'], c['y']) and same(a['ypre'], b['ypre'])
    assert same(a['mask7'], b['mask7']) and same(a['mask7'], c['mask7'])
    assert same(b['gate_y'], bits3(b['ypre'])) and same(c['gate_y'], b['gate_y'])
    assert same(a['y'][..., :3], torch.clamp(a['ypre'][..., :3], max=1.0)) and (a['y'][..., 3] == 0).all() and (a['ypre'][..., 3] == 0).all()
    # a second launch of each, bitwise
    for again, first in ((tail_launch(s, False)[1], a), (tail_launch(s, True)[1], b), (tail_launch(s, True, with_ypre=False)[1], c)):
        assert all(first[k] is None or same(first[k], again[k]) for k in first)
    # against the restatement
    worst = max(ratio_under(f'{plain} y', a['y'][..., :3], r['y'], fb['pre']), ratio_under(f'{plain} ypre', a['ypre'][..., :3], r['ypre'], fb['pre']))
    m7 = so.unpack_bits(a['mask7'].numpy(), so.C7)
    assert m7[fb['one7']].all() and not m7[fb['zero7']].any(), f'{plain}: mask7 bits differ where |pre7| exceeds its bar'
    gate = lambda g: ((np.asarray(g)[..., None] >> np.arange(3, dtype=np.uint8)) & 1).astype(bool)
    assert np.array_equal(gate(b['gate_y'].numpy())[fb['gate_sure']], gate(r['gate_y'])[fb['gate_sure']]), f'{gname}: gate_y bits differ away from the edges'
    clamped = r['pre'] > 1
    assert (a['y'][..., :3].numpy()[clamped & fb['gate_sure']] == 1).all()
    assert max(fb['left_out'].values()) < so.LEFT_OUT_CAP
    z = s['inp']['zero_image']
    if z is not None:      # X7 = 0 and b6 = 0: pre IS res1 -- bitwise, the edges of the clamp gate included
        res = s['host']['res1'][z, ..., :3]
        want = torch.clamp_min(res + 0.0, 0.0)
        assert same(a['ypre'][z, ..., :3], want) and same(a['y'][z, ..., :3], torch.clamp(want, max=1.0))
        assert same(b['gate_y'][z], bits3(want)) and same(b['gate_y'][z], torch.from_numpy(r['gate_y'][z]))
        assert (a['mask7'][z] == 0).all()
    report(f'{plain} / {gname} {content} {s["B"]}x{H2}x{W2}', worst)


def head_launch(s, form, g_adv=None, state=None, gate=None):
    """One backward launch into a fresh guarded P6; form 0 plain, 1 select (gate: a ypre tensor), 2 select_g (gate: the byte)."""
    B, H2, W2, d, p = s['B'], s['H2'], s['W2'], s['dev'], s['p']
    out = Guarded((B, H2, W2, so.C6), torch.float16 if s['f16'] else torch.float32, W2 * so.C6)
    name = HEAD['f16' if s['f16'] else 'f32'][form]
    rest = (p(d['w6t']), s['w'](d['w2t']), p(d['mask7_in']), p(d['mask6_in']), s['lib'].hptr(out.t), B, H2, W2)
    g_adv = d['g_adv'] if g_adv is None else g_adv
    if form == 0:
        s['lib'].call(name, p(g_adv), *rest)
    else:
        s['lib'].call(name, p(g_adv), p(d['g_col']), p(d['state'] if state is None else state), p(gate), *rest)
    torch.cuda.synchronize()
    return name, out.check(name)


@pytest.mark.parametrize('content,storage,B,H2,W2', PARAMS, ids=IDS)
def test_head_backward(hip, content, storage, B, H2, W2):
    s = setup(hip, content, storage, B, H2, W2)
    ref, d = so.reference_bwd(*s['case']), s['dev']
    byte = bits3(d['ypre_in'])
    assert torch.equal(byte.cpu(), torch.from_numpy(so.head_forms(s['inp'])['select_g']['gate']))
    runs = dict(plain=lambda: head_launch(s, 0), select=lambda: head_launch(s, 1, gate=d['ypre_in']), select_g=lambda: head_launch(s, 2, gate=byte))
    got = {form: run() for form, run in runs.items()}
    inputs_unchanged(s)
    for form, run in runs.items():      # a second launch, bitwise
        assert same(run()[1], got[form][1]), f'{got[form][0]}: two launches differ'
    assert same(got['select'][1], got['select_g'][1]), 'the byte form differs from the ypre form on the same ypre'
    # state[:, 1] = 0 and a gate that lets everything pass: the plain launch on g_adv
    state0 = d['state'].clone()
    state0[:, 1] = 0
    clean = d['g_adv'].clone()
    clean[..., 3] = 0
    for form, gate in ((1, torch.full_like(d['ypre_in'], 0.5)), (2, torch.full_like(byte, 7))):
        assert same(head_launch(s, form, state=state0, gate=gate)[1], got['plain'][1])
    assert same(head_launch(s, 0, g_adv=clean)[1], got['plain'][1]), 'channel 3 of the cotangent reached P6'
    worst = {got[form][0]: ratio_under(got[form][0], got[form][1], *ref[form]) for form in runs}
    for name, ratio in worst.items():
        report(f'{name} {content} {s["B"]}x{H2}x{W2}', ratio)


def test_refusals_leave_the_outputs_alone(hip):
    s = setup(hip, 'random', 'f32', 2, 6, 14)
    s16 = setup(hip, 'random', 'f16', 2, 6, 14)
    lib, p, B, H2, W2, H, W = hip['lib'].load(), s['p'], 2, 6, 14, 12, 28
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = dict(y=Guarded((B, H, W, 4), torch.float32, 4 * W), ypre=Guarded((B, H, W, 4), torch.float32, 4 * W),
                mask7=Guarded((B, H, W, 8), torch.uint8, 8 * W), gate_y=Guarded((B, H, W), torch.uint8, W),
                p6=Guarded((B, H2, W2, 64), torch.float32, 64 * W2), p6h=Guarded((B, H2, W2, 64), torch.float16, 64 * W2))
    y, ypre, m7, gy = (p(outs[k].t) for k in ('y', 'ypre', 'mask7', 'gate_y'))
    n = 0
    for st, p6 in ((s, p(outs['p6'].t)), (s16, p(outs['p6h'].t))):
        d, w = st['dev'], st['w']
        tail, tail_g = (getattr(lib, nm) for nm in TAIL['f16' if st['f16'] else 'f32'])
        head, sel, sel_g = (getattr(lib, nm) for nm in HEAD['f16' if st['f16'] else 'f32'])
        fwd = [hip['lib'].hptr(d['x6']), w(d['w2']), p(d['b2']), w(d['w6']), p(d['b6']), p(d['res1']), y]
        bwd = [p(d['w6t']), w(d['w2t']), p(d['mask7_in']), p(d['mask6_in']), p6]
        byte_t = bits3(d['ypre_in'])
        ga, gc, stt, yin, byte = p(d['g_adv']), p(d['g_col']), p(d['state']), p(d['ypre_in']), p(byte_t)
        refused = [tail_g(*fwd, ypre, m7, None, B, H2, W2, stream),               # _g without gate_y
                   tail(*fwd, None, m7, B, H2, W2, stream),                       # neither ypre nor gate_y
                   sel(ga, gc, None, yin, *bwd, B, H2, W2, stream), sel_g(ga, gc, None, byte, *bwd, B, H2, W2, stream),      # select without state
                   sel(ga, None, stt, yin, *bwd, B, H2, W2, stream), sel_g(ga, None, stt, byte, *bwd, B, H2, W2, stream),    # state but no g_col
                   sel(ga, gc, stt, None, *bwd, B, H2, W2, stream), sel_g(ga, gc, stt, None, *bwd, B, H2, W2, stream),       # no gate at all
                   tail(*fwd, ypre, m7, 0, H2, W2, stream), tail_g(*fwd, ypre, m7, gy, 0, H2, W2, stream),                   # B = 0
                   head(ga, *bwd, 0, H2, W2, stream), sel(ga, gc, stt, yin, *bwd, 0, H2, W2, stream), sel_g(ga, gc, stt, byte, *bwd, 0, H2, W2, stream)]
        assert refused == [HIP_INVALID_VALUE] * len(refused), refused
        n += len(refused)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values()), 'a refused call has written'
    report(f'{n} refused calls', 0.0)
