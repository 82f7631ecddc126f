"""GPU (-m gpu): every tuned convolution / linear launch of the benchmarked configurations against an fp64 reference of the SAME launch.

bench.py times its configurations at batch 64 on whatever spaa_amd/tapconv_tune.json picked for each layer shape: split-K forms of the
DMA-staged bf16x6 tiles, stream-K, Winograd K ranges and canvases, the fp16 split-K of the fully connected layers -- forms that exist
only at those shapes.  Here one eager iteration of each configuration (built by bench.build_attack itself) runs with
ConvPlan.run / SmallLinearPlan.run wrapped: every outer launch keeps copies of the operands it reads, and after it its output window
is compared element by element with the same launch restated in fp64 on the GPU (tests/tapconv_emu.emulate over the packed
weights, the launch's epilogue applied in fp64):

    |y - r| <= tau_family * (s + |bias| + |add|)   (+ half an fp16 ulp of r where the output is fp16),   s = sum |W| |x|

with the operands rounded as the kernel family rounds them (exact fp32: bf16x6, fp32-MFMA, Winograd, the linear kernel; fp16 weights
and fp16 inputs: the fp16-storage tiles; fp16 image and weights: tile 76 in fp16 storage).  Against the launch's own inputs no
ReLU gate can flip, so no gate-aware logic is needed; the byte masks a launch writes are checked wherever the fp64 value is farther
from 0 than the bound.
"""
import inspect
import time

import pytest
import torch

import bench
from spaa_amd import _lib
from spaa_amd import convplan as cp
from tapconv_emu import emulate, packed_taps

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64

# tau per kernel family = MARGIN x the largest err / (s + |bias| + |add|) measured over the six configurations below on MI355X (for
# fp16 outputs: beyond half an fp16 ulp).  Worst launches: x6 classifier.6_dgrad 1000_4096 (tile 22, VGG-16 f32), wino
# Conv2d_4a_3x3_dgrad (tile 70, Inception-v3 f32), fp16 the ResNet-18 stem's input gradient (tile 72, f16), linear the ResNet-18 fc.
# A family without a measurement (the fp32-MFMA / VALU tiles: no benchmarked layer runs on them) fails the test until measured.
MARGIN = 3.0
MEASURED_ON_MI355X = {'x6': 1.093e-6, 'wino': 6.268e-7, 'fp16': 3.092e-7, 'linear': 3.353e-8}
TAU = {k: MARGIN * v for k, v in MEASURED_ON_MI355X.items()}
MEASURED = {k: 0.0 for k in TAU}      # the largest of this session (printed like tests/gates.py's MEASURED)

# fused forms with tests of their own (tests/test_gpu_parity.py): their input is not the tensor `inp`
EXEMPT = ('pool_adjoint', 'unpool')

CONFIGS = [('resnet18', 'f32', 'spaa'), ('resnet18', 'f16', 'spaa'), ('inception_v3', 'f32', 'spaa'), ('inception_v3', 'f16', 'spaa'),
           ('vgg16', 'f16', 'perc_al'), ('vgg16', 'f32', 'perc_al')]
# VGG-16's full head (25088 -> 4096 -> 4096 -> 1000) at batch 64: the tune keys of its fully connected layers
VGG_HEAD_KEYS = ('25088_4096_1_1_1_64', '4096_4096_1_1_1_64', '4096_25088_1_1_1_64')
WINO_TILES, X6_TILES = cp.WINO_TILES, cp.X6_TILES      # (derived from the tile table: spaa_amd/tiles.py)


def family(tile, in_f16, out_f16):
    """(family, operands): the tau family of a launch and how its operands are rounded -- 'fp32' exact, 'f16' fp16 weights (the
    half_plane values) and fp16 inputs, 'f16img' the fp32 image rounded to fp16 as well (tile 76 in fp16 storage)."""
    if tile == 75:
        return 'linear', 'fp32'
    if in_f16:
        return 'fp16', 'f16'
    if tile == 76 and out_f16 and 'c3h' not in cp.DEFAULT_DISABLE:
        return 'fp16', 'f16img'
    if tile in WINO_TILES:
        return 'wino', 'fp32'
    return ('x6' if tile in X6_TILES else 'f32'), 'fp32'


def tune_key(plan, b, hout, wout):
    hm, wm = (hout, wout) if plan.s_out == 1 else ((hout + plan.s_out - 1) // plan.s_out, (wout + plan.s_out - 1) // plan.s_out)
    return f'{plan.cin_p}_{plan.cout}_{plan.alg_taps}_{plan.s_in}_{plan.s_out}_{b * hm * wm}' + ('_fold' if plan.nfold > 1 else '')


def bits(mask, coff, n):
    """uint8 [.., C/4] byte masks (include/spaa_hip.h: bit e of byte c / 4 = channel c) -> bool [.., n] of channels coff..coff+n-1."""
    m = (mask.unsqueeze(-1) >> torch.arange(4, device=mask.device, dtype=torch.uint8)) & 1
    return m.flatten(-2)[..., coff:coff + n].bool()


def half_ulp(r):
    """Half an fp16 ulp of |r| (2^-25 in the subnormal range)."""
    e = torch.frexp(r.abs().clamp(min=2.0 ** -14))[1]
    return torch.ldexp(torch.ones_like(r), e - 12)


def _clone(t):
    return None if t is None else t.clone()


def _ratio(err, scale, slack):
    ok = scale > 0
    return float(((err - slack).clamp(min=0)[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0


def check(rec, y, r, scale, fam, out_f16, what):
    """|y - r| <= tau * scale (+ half an fp16 ulp): records err / scale of the launch, returns the element bound used for masks."""
    slack = half_ulp(r.abs() + TAU[fam] * scale) if out_f16 else torch.zeros_like(r)
    err = (y.double() - r).abs()
    ratio = _ratio(err, scale, slack)
    rec['ratio'] = max(rec.get('ratio', 0.0), ratio)
    MEASURED[fam] = max(MEASURED[fam], ratio)
    bound = TAU[fam] * scale + slack
    bad = err > bound
    assert not bool(bad.any()), (rec['name'], rec['key'], rec['tile'], rec['ksplit'], what, f'{int(bad.sum())} elements outside the bound',
                                 f'err / scale {ratio:.3e} > tau {TAU[fam]:.3e}')
    return bound


def audit_conv(plan, a, pre_out, out, rec):
    """The fp64 reference of one ConvPlan launch (arguments `a`, operands cloned before it ran; `out` as written)."""
    inp = a['inp']
    b, hout, wout, _ = out.shape
    in_f16, out_f16 = inp.dtype == torch.float16, out.dtype == torch.float16
    fam, ops = rec['family'], rec['operands']
    cin2k = getattr(plan, 'cin2_k', 0)
    x = inp[..., a['in_coff']:a['in_coff'] + plan.cin_p - cin2k]
    if cin2k:
        x = torch.cat([x, a['inp2'][..., a['in2_coff']:a['in2_coff'] + cin2k]], -1)
    if ops == 'f16img':
        x = x.half()
    r, s = emulate(plan, x, hout, wout, F64, inp.device, packed_taps(plan, half=ops != 'fp32'), bias=False, magnitude=True)
    bias = plan.bias
    if a['inp2'] is not None and not cin2k:   # a fused 1 x 1 second source at output resolution (attach_second_source[_h16])
        x2 = a['inp2'][..., a['in2_coff']:a['in2_coff'] + plan.cin2].double()
        if in_f16:
            w2 = plan.w2_half.double()
        else:
            w2 = plan.w2_split.view(3, -1, plan.cin2).view(torch.bfloat16).double().sum(0)[:plan.cout]
        r, s = r + x2 @ w2.t(), s + x2.abs() @ w2.abs().t()
        bias = plan.bias2
    scale = s
    pre = r
    if bias is not None:
        pre = pre + bias.double()
        scale = scale + bias.double().abs()
    if a['add'] is not None:
        ad = a['add'][..., a['add_coff']:a['add_coff'] + plan.cout].double()
        pre, scale = pre + ad, scale + ad.abs()
    act = a['act']
    v = pre
    if act == _lib.ACT_RELU:
        v = v.clamp(min=0)
    elif act == _lib.ACT_RELU_CLAMP1:
        v = v.clamp(min=0)
        relu_v = v
        v = v.clamp(max=1)
    elif act == _lib.ACT_LEAKY01:
        v = torch.where(v > 0, v, 0.1 * v)
    off = torch.zeros_like(pre, dtype=torch.bool)     # gated off: exactly zero whatever the sum
    if a['gate'] is not None:
        g = a['gate'][..., a['gate_coff']:a['gate_coff'] + plan.cout].double()
        if a['gate_mode'] == _lib.GATE_MUL:
            v, scale = v * g, scale * g.abs()
        else:
            off = ~((g > 0) & (g <= 1)) if a['gate_mode'] == _lib.GATE_POS_LE1 else ~(g > 0)
    elif a['gate_bits'] is not None:
        off = ~bits(a['gate_bits'], a['gate_coff'], plan.cout)
    v = v.masked_fill(off, 0.0)
    oc = a['out_coff']
    if a['pool'] is not None:
        pooled, _parg, _want = a['pool']
        rp = torch.nn.functional.max_pool2d(v.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        sp = torch.nn.functional.max_pool2d(scale.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        check(rec, pooled[..., :plan.cout], rp, sp, fam, out_f16, 'pooled')
        if plan.last_pool_fused:      # (the full-size output is not written)
            return
    y = out[..., oc:oc + plan.cout]
    bound = check(rec, y, v, scale, fam, out_f16, 'out')
    if a['mask_out'] is not None:
        sure = (pre.abs() > bound) | off
        mb = bits(a['mask_out'], oc, plan.cout)
        wrong = (mb != (v > 0)) & sure
        assert not bool(wrong.any()), (rec['name'], rec['key'], rec['tile'], f'{int(wrong.sum())} mask bits differ from the fp64 sign')
    if a['aux_out'] is not None:
        aux = a['aux_out'][..., oc:oc + plan.cout]
        if act == _lib.ACT_RELU_CLAMP1:
            check(rec, aux, relu_v, scale, fam, out_f16, 'aux_out (pre-clamp)')
        elif a['gate2'] is not None or a['gate2_bits'] is not None:
            g2 = (a['gate2'][..., :plan.cout] > 0) if a['gate2'] is not None else bits(a['gate2_bits'], 0, plan.cout)
            check(rec, aux, v.masked_fill(~g2, 0.0), scale, fam, out_f16, 'aux_out (second gate)')


class Auditor:
    """Wraps ConvPlan.run / SmallLinearPlan.run (pytest monkeypatch) for one configuration."""

    def __init__(self, monkeypatch):
        self.records, self.stack, self.replays = [], [], []
        self.orig = cp.ConvPlan.run
        self.orig_small = cp.SmallLinearPlan.run
        self.sig = inspect.signature(self.orig)
        # (plain functions, not bound methods: looked up through a plan they bind to it like the originals)
        monkeypatch.setattr(cp.ConvPlan, 'run', lambda plan, *a, **kw: self._conv(plan, *a, **kw))
        monkeypatch.setattr(cp.SmallLinearPlan, 'run', lambda plan, inp, out, **kw: self._small(plan, inp, out, **kw))

    def _conv(self, plan, *args, **kw):
        ba = self.sig.bind(plan, *args, **kw)
        ba.apply_defaults()
        a = dict(ba.arguments)
        if a['_wino'] is not None:      # the Winograd form of a layer: reported into the outer launch, audited as that layer
            res = self.orig(plan, *args, **kw)
            if self.stack:
                self.stack[-1]['inner'] = (plan.last_tile, plan.last_ksplit, plan.last_wino_plan)
            return res
        inp, out = a['inp'], a['out']
        rec = dict(name=plan.name, key=tune_key(plan, out.shape[0], out.shape[1], out.shape[2]), kind='conv')
        exempt = [k for k in EXEMPT if a[k] is not None]
        # every operand the launch reads, as it was before (`add` may alias `out`; untouched channels of `out` stay)
        cl = {k: _clone(a[k]) for k in ('inp', 'add', 'gate', 'gate_bits', 'gate2', 'gate2_bits', 'inp2')}
        pre_out = out.clone()
        self.stack.append(rec)
        try:
            res = self.orig(plan, *args, **kw)
        finally:
            self.stack.pop()
        torch.cuda.synchronize()
        inner = rec.pop('inner', None)
        rec['tile'], rec['ksplit'] = (inner[0], inner[1]) if inner else (plan.last_tile, plan.last_ksplit)
        rec['family'], rec['operands'] = family(rec['tile'], inp.dtype == torch.float16, out.dtype == torch.float16)
        assert rec['family'] in TAU, (rec, 'a kernel family without a measured tau')
        rec['wino_plan'] = inner[2] if inner else None
        rec['h16p_plan'] = getattr(plan, 'last_h16p_plan', None) if rec['tile'] == 68 and rec['ksplit'] > 1 else None
        self.records.append(rec)
        if exempt:
            rec['exempt'] = '+'.join(exempt)
            return res
        a2 = dict(a, **cl)
        audit_conv(plan, a2, pre_out, out, rec)
        rec['audited'] = True
        if rec['ksplit'] > 1 and (rec['tile'] in WINO_TILES or rec['tile'] == 68):
            # K ranges of the Winograd / patch-staged fp16 kernel: replayed with the in-kernel fix-up at the end (bitwise the two-pass form)
            after = {k: _clone(a[k]) for k in ('mask_out', 'aux_out')}
            after['out'] = out.clone()
            after['pooled'] = _clone(a['pool'][0]) if a['pool'] is not None else None
            alias = a['add'] is not None and a['add'].data_ptr() == out.data_ptr()
            self.replays.append((plan, a2, pre_out, after, alias, rec))
        return res

    def _small(self, plan, inp, out, **kw):
        if not plan.applies(inp, out, kw):     # (the wrapped 1 x 1 convolution plan: audited as a ConvPlan launch)
            return self.orig_small(plan, inp, out, **kw)
        x = inp.clone()
        res = self.orig_small(plan, inp, out, **kw)
        torch.cuda.synchronize()
        m = x.shape[0] * x.shape[1] * x.shape[2]
        rec = dict(name=plan.name, key=tune_key(plan.conv, out.shape[0], out.shape[1], out.shape[2]), kind='linear', tile=plan.last_tile,
                   ksplit=plan.last_ksplit, family='linear', operands='fp32', wino_plan=None, h16p_plan=None)
        self.records.append(rec)
        xd, wd = x.view(m, plan.k).double(), plan.w.double()
        r, s = xd @ wd.t(), xd.abs() @ wd.abs().t()
        if plan.bias is not None:
            r, s = r + plan.bias.double(), s + plan.bias.double().abs()
        check(rec, out.view(m, plan.n), r, s, 'linear', False, 'out')
        rec['audited'] = True
        return res

    def replay_fixup(self, monkeypatch):
        """Every audited Winograd / tile-68 launch with K ranges once more with the K ranges combined inside the kernel."""
        monkeypatch.setattr(cp, 'WINO_SPLITK_FIXUP', True)
        n = 0
        for plan, a, pre_out, after, alias, rec in self.replays:
            out = pre_out.clone()
            args = {k: a[k] for k in self.sig.parameters if k not in ('self', 'inp', 'out', '_wino')}
            if alias:
                args['add'] = out
            mine = {k: (after[k].clone() if after[k] is not None else None) for k in ('mask_out', 'aux_out')}
            args.update(mine)
            if a['pool'] is not None:
                args['pool'] = (a['pool'][0].clone(), a['pool'][1].clone(), a['pool'][2])
            for t in mine.values():
                if t is not None:
                    t.fill_(0 if t.dtype == torch.uint8 else float('nan'))
            self.orig(plan, a['inp'], out, **args)
            torch.cuda.synchronize()
            wp = plan.wino.last_wino_plan if rec['tile'] in WINO_TILES else plan.last_h16p_plan
            assert wp[1] == rec['ksplit'], (rec['name'], wp, rec['ksplit'])
            oc, co = a['out_coff'], plan.cout
            same = torch.equal(out, after['out'])
            if after['pooled'] is not None:
                same = same and torch.equal(args['pool'][0], after['pooled'])
            if mine['aux_out'] is not None:
                same = same and torch.equal(mine['aux_out'][..., oc:oc + co], after['aux_out'][..., oc:oc + co])
            if mine['mask_out'] is not None:
                same = same and torch.equal(mine['mask_out'][..., oc // 4:(oc + co) // 4], after['mask_out'][..., oc // 4:(oc + co) // 4])
            assert same, (rec['name'], rec['key'], rec['tile'], 'in-kernel K-range fix-up differs from the two-pass form')
            ws = plan.wino._ws_fix if rec['tile'] in WINO_TILES else plan._ws_fix
            assert ws is not None and int(ws[:cp.SPLITK_HDR].view(torch.int32).abs().max()) == 0, (rec['name'], 'arrival counters left set')
            n += 1
        monkeypatch.setattr(cp, 'WINO_SPLITK_FIXUP', False)
        return n


def report(tag, recs, nrep):
    fams = sorted({r['family'] for r in recs})
    print(f'\n=== {tag}: {len(recs)} launches, {sum(1 for r in recs if r.get("audited"))} audited, '
          f'{sum(1 for r in recs if "exempt" in r)} exempt ({", ".join(sorted({r["exempt"] for r in recs if "exempt" in r})) or "-"}), '
          f'{nrep} K-range launches replayed with the in-kernel fix-up')
    for f in fams:
        rs = [r for r in recs if r['family'] == f and r.get('audited')]
        worst = max(rs, key=lambda r: r['ratio']) if rs else None
        if worst:
            print(f'  family {f:6s}: {len(rs):4d} audited, worst err/scale {worst["ratio"]:.3e} = {worst["ratio"] / TAU[f]:.3f} tau '
                  f'({worst["name"]} {worst["key"]} tile {worst["tile"]} ksplit {worst["ksplit"]})')
    seen = {}
    for r in recs:
        k = (r['key'], r['tile'], r['ksplit'])
        seen.setdefault(k, []).append(r)
    print(f'  {len(seen)} distinct (key, tile, ksplit):')
    for (key, tile, ks), rs in sorted(seen.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        worst = max((r.get('ratio', 0.0) for r in rs), default=0.0)
        st = 'exempt' if all('exempt' in r for r in rs) else f'{worst:.2e}'
        print(f'    {key:28s} tile {tile:3d} ksplit {ks:3d} x{len(rs):3d}  {rs[0]["family"]:6s} {st}')


@pytest.mark.parametrize('classifier,storage,attack', CONFIGS, ids=[f'{c}-{s}-{a}' for c, s, a in CONFIGS])
def test_tuned_launches_against_fp64(classifier, storage, attack, monkeypatch):
    """One eager iteration of a benchmarked configuration (bench.build_attack, batch 64, 256 x 256 scenes): every convolution and
    linear launch within tau_family of its fp64 reference; every K-split launch audited; the Winograd / tile-68 K-range launches
    bitwise equal with the in-kernel fix-up."""
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    with torch.cuda.device(0):
        st, *_ = bench.build_attack(0, 64, 256, 8, DEV, classifier, storage, attack)
        torch.cuda.synchronize()
        aud = Auditor(monkeypatch)
        st.step()
        torch.cuda.synchronize()
        nrep = aud.replay_fixup(monkeypatch)
    recs = aud.records
    report(f'{classifier} {storage} {attack}', recs, nrep)
    print(f'  wall {time.perf_counter() - t0:.1f} s; largest err/scale this session: ' + ', '.join(f'{k} {v:.3e}' for k, v in MEASURED.items()))
    assert recs, 'no launch went through ConvPlan.run / SmallLinearPlan.run'
    missing = [r for r in recs if not r.get('audited') and 'exempt' not in r]
    assert not missing, missing[:3]
    for r in recs:
        if 'exempt' in r:
            assert set(r['exempt'].split('+')) <= set(EXEMPT), r
            assert r['ksplit'] == 1, ('a K-split launch must be audited', r)
    assert nrep == len(aud.replays)
    if classifier == 'vgg16':
        head = {r['key']: r for r in recs if r['key'] in VGG_HEAD_KEYS}
        assert set(head) == set(VGG_HEAD_KEYS), sorted(head)
        assert all(r.get('audited') for r in recs if r['key'] in VGG_HEAD_KEYS)
        if storage == 'f32':
            print('  VGG-16 head (f32): ' + ', '.join(f'{k} -> tile {head[k]["tile"]} ksplit {head[k]["ksplit"]}' for k in VGG_HEAD_KEYS))
        else:
            fc6 = [r for r in recs if r['key'] == VGG_HEAD_KEYS[0]]
            assert any(r['family'] == 'fp16' and r['ksplit'] > 1 for r in fc6), [(r['tile'], r['ksplit'], r['family']) for r in fc6]
