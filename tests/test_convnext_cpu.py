"""CPU: what tests/test_convnext_ops_gpu.py and tests/test_convnext_gpu.py rest on.  The restatement of the depthwise 7 x 7 layer and
its adjoint (tests/convnext_oracle.py) agrees with torch's grouped convolution and autograd in float64; the whole float64 network
agrees with a torch.nn module assembled here from the same state dict, logits and input gradient; every mutation of the oracle lands
beyond the bar its GPU test holds the kernels to, on the inputs that test uses; folding the layer scale into block.5 is exact; and
Classifier('convnext_tiny') is a known name that constructs without a GPU and refuses what the body does not serve."""
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import convnext_oracle as co
import spaa_oracle as so
from spaa_amd import _lib, convnext, synthetic as syn
from spaa_amd.classifier import BODIES, INPUT_SZ, LAST_LINEAR, NO_FEATURE_MAP, Classifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_inf(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def test_entry_points_and_registration():
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ('spaa_dwconv7_fwd', 'spaa_dwconv7_bwd'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert 'convnext_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert 'convnext_tiny' in BODIES and INPUT_SZ['convnext_tiny'] == (224, 224) and LAST_LINEAR['convnext_tiny'] == 'classifier.2'
    assert 'convnext_tiny' not in NO_FEATURE_MAP


def expected_keys(ncls, dims=(96, 192, 384, 768), depths=(3, 3, 9, 3)):
    keys = {'features.0.0.weight': (dims[0], 3, 4, 4), 'features.0.0.bias': (dims[0],), 'features.0.1.weight': (dims[0],),
            'features.0.1.bias': (dims[0],), 'classifier.0.weight': (dims[-1],), 'classifier.0.bias': (dims[-1],),
            'classifier.2.weight': (ncls, dims[-1]), 'classifier.2.bias': (ncls,)}
    for si, (c, d) in enumerate(zip(dims, depths)):
        s = 2 * si + 1
        if si:
            cp_ = dims[si - 1]
            keys.update({f'features.{s - 1}.0.weight': (cp_,), f'features.{s - 1}.0.bias': (cp_,), f'features.{s - 1}.1.weight': (c, cp_, 2, 2),
                         f'features.{s - 1}.1.bias': (c,)})
        for i in range(d):
            p = f'features.{s}.{i}.'
            keys.update({p + 'block.0.weight': (c, 1, 7, 7), p + 'block.0.bias': (c,), p + 'block.2.weight': (c,), p + 'block.2.bias': (c,),
                         p + 'block.3.weight': (4 * c, c), p + 'block.3.bias': (4 * c,), p + 'block.5.weight': (c, 4 * c),
                         p + 'block.5.bias': (c,), p + 'layer_scale': (c, 1, 1)})
    return keys


def test_state_dict_has_torchvisions_keys_and_shapes():
    import inspect
    dflt = {k: v.default for k, v in inspect.signature(syn.convnext_tiny_state_dict).parameters.items()}
    assert dflt == dict(seed=8, num_classes=1000, logit_gain=1.0, dims=(96, 192, 384, 768), depths=(3, 3, 9, 3))
    sd = syn.convnext_tiny_state_dict(num_classes=10)
    want = expected_keys(10)
    assert set(sd) == set(want) and len(want) == 8 + 3 * 4 + 18 * 9
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape and sd[k].dtype == torch.float32, k
    a = co.state_dict()
    assert set(a) == set(expected_keys(co.NUM_CLASSES, co.DIMS, co.DEPTHS))
    b = syn.convnext_tiny_state_dict(seed=8, num_classes=co.NUM_CLASSES, logit_gain=co.LOGIT_GAIN, dims=co.DIMS, depths=co.DEPTHS)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # the layer scale is of order 1: a block is not the identity
    assert all(float(v.min()) >= 0.5 for k, v in a.items() if k.endswith('layer_scale'))
    assert convnext.config(a) == (4, co.DIMS, co.DEPTHS) and co.config(a) == (co.DIMS, co.DEPTHS)
    with pytest.raises(ValueError, match='multiples of 4'):
        syn.convnext_tiny_state_dict(dims=(6, 12), depths=(1, 1))


@pytest.mark.parametrize('case', co.DW_CASES[:6], ids=str)
def test_dwconv7_restatement_against_torch(case):
    """dwconv7 against F.conv2d(groups=C) and its adjoint against autograd, float64."""
    x, wt, bias, g, add = (t.double() for t in co.dw_inputs(*case))
    c = case[3]
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = F.conv2d(xn, wt.t().reshape(c, 1, 7, 7), bias, padding=3, groups=c)
    out = co.dwconv7(x, wt, bias)
    assert out.shape == x.shape and torch.allclose(out, ref.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    ref.backward(g.permute(0, 3, 1, 2))
    gin = co.dwconv7_bwd(g, wt, add)
    assert torch.allclose(gin, xn.grad.permute(0, 2, 3, 1) + add, rtol=1e-12, atol=1e-12)
    assert torch.allclose(co.dwconv7_bwd(g, wt), xn.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    # the pair is an adjoint
    lhs, rhs = float((g * (out - bias)).sum()), float((co.dwconv7_bwd(g, wt) * x).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))
    n = co.tap_count(case[1], case[2])
    assert float(n.max()) <= 49 and float(n.min()) >= min(case[1], 4) * min(case[2], 4)


class _LN2d(nn.Module):
    """LayerNorm over the channels of an NCHW map (torchvision's LayerNorm2d)."""

    def __init__(self, c):
        super().__init__()
        self.ln = nn.LayerNorm(c, eps=1e-6)

    def forward(self, x):
        return self.ln(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class _Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dw, self.ln = nn.Conv2d(c, c, 7, padding=3, groups=c), nn.LayerNorm(c, eps=1e-6)
        self.fc1, self.act, self.fc2 = nn.Linear(c, 4 * c), nn.GELU(), nn.Linear(4 * c, c)
        self.ls = nn.Parameter(torch.ones(c, 1, 1))

    def forward(self, x):
        y = self.fc2(self.act(self.fc1(self.ln(self.dw(x).permute(0, 2, 3, 1))))).permute(0, 3, 1, 2)
        return x + self.ls * y


def torch_module(sd):
    """convnext_tiny as torch.nn modules, filled from `sd` (float64)."""
    dims, depths = co.config(sd)

    def fill(m, key):
        m.weight.data, m.bias.data = sd[key + '.weight'].clone(), sd[key + '.bias'].clone()
        return m

    stem_ln = _LN2d(dims[0])
    fill(stem_ln.ln, 'features.0.1')
    layers = [fill(nn.Conv2d(3, dims[0], 4, stride=4), 'features.0.0'), stem_ln]
    for si, (c, d) in enumerate(zip(dims, depths)):
        s = 2 * si + 1
        if si:
            ln = _LN2d(dims[si - 1])
            fill(ln.ln, f'features.{s - 1}.0')
            layers += [ln, fill(nn.Conv2d(dims[si - 1], c, 2, stride=2), f'features.{s - 1}.1')]
        for i in range(d):
            p, blk = f'features.{s}.{i}.', _Block(c)
            fill(blk.dw, p + 'block.0'), fill(blk.ln, p + 'block.2'), fill(blk.fc1, p + 'block.3'), fill(blk.fc2, p + 'block.5')
            blk.ls.data = sd[p + 'layer_scale'].clone()
            layers.append(blk)
    head = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(1), fill(nn.LayerNorm(dims[-1], eps=1e-6), 'classifier.0'),
                         fill(nn.Linear(dims[-1], sd['classifier.2.weight'].shape[0]), 'classifier.2'))
    return nn.Sequential(*layers, head).double().eval()


@pytest.mark.parametrize('geom', list(co.GEOMS))
def test_oracle_against_torchs_own_modules(geom):
    _, crop, insz = co.GEOMS[geom]
    sd = co.to64(co.state_dict())
    r = torch.randn(co.B, co.NUM_CLASSES, generator=torch.Generator().manual_seed(1)).double()
    x1 = so.classifier_preprocess(co.images(geom), crop, insz).double().requires_grad_(True)
    rec = {}
    raw = co.forward(sd, x1, record=rec)
    (raw * r).sum().backward()
    x2 = x1.detach().clone().requires_grad_(True)
    ref = torch_module(sd)(x2)
    (ref * r).sum().backward()
    assert rel_inf(raw, ref) < 1e-12 and rel_inf(x1.grad, x2.grad) < 1e-10
    sizes = convnext.map_sizes(insz, 4, 4)
    assert len(rec['blocks']) == sum(co.DEPTHS) and tuple(rec['feat'].shape) == (co.B, *sizes[-1], co.DIMS[-1])
    assert sizes == ([(16, 16), (8, 8), (4, 4), (2, 2)] if geom == 'square' else [(9, 13), (4, 6), (2, 3), (1, 1)])
    # the logits are not degenerate: the classes differ and so do the samples
    assert float(raw.detach().std(dim=1).min()) > 0.05 and float(raw.detach().std(dim=0).min()) > 1e-3


KERNEL_BUGS = [k for k, fns in co.MUTATIONS.items() if co.forward not in fns]


@pytest.mark.parametrize('bug', KERNEL_BUGS)
def test_kernel_level_mutations_land_beyond_the_bars(bug):
    """On every case of the GPU test (but a 1 x 1 map for a mirror or a transposition, which leave its one tap in place) the mistaken
    function differs from the right one by more than the bar somewhere: a kernel that made the mistake would fail that case."""
    seen = 0
    for case in co.DW_CASES:
        x, wt, bias, g, add = (t.double() for t in co.dw_inputs(*case))
        for fn in co.MUTATIONS[bug]:
            if fn is co.dwconv7:
                good, bad, bar = fn(x, wt, bias), fn(x, wt, bias, _bug=bug), co.bar_dwconv7(x, wt, bias)
            else:
                good, bad, bar = fn(g, wt, add), fn(g, wt, add, _bug=bug), co.bar_dwconv7_bwd(g, wt, add)
            worst = float(((bad - good).abs() / bar).max())
            if (bug, case) in co.BLIND:
                assert worst == 0.0
                continue
            assert worst > 100, (bug, case, fn.__name__, worst)
            seen += 1
    assert seen >= len(co.DW_CASES) - 1


def test_layer_scale_on_the_residual_lands_beyond_the_bars():
    for geom in co.GEOMS:
        _, crop, insz = co.GEOMS[geom]
        sd = co.to64(co.state_dict())
        x = so.classifier_preprocess(co.images(geom), crop, insz).double()
        assert rel_inf(co.forward(sd, x, _bug='layer_scale_on_residual'), co.forward(sd, x)) > 1e-3       # the bar is 1e-5


def test_bars_hold_for_torchs_own_fp32_pass():
    """The bars are not vacuous the other way either: torch's fp32 grouped convolution stays inside them."""
    for case in co.DW_CASES[:6]:
        x, wt, bias, g, add = co.dw_inputs(*case)
        c = case[3]
        out32 = F.conv2d(x.permute(0, 3, 1, 2), wt.t().reshape(c, 1, 7, 7), bias, padding=3, groups=c).permute(0, 2, 3, 1)
        ref, bar = co.dwconv7(x.double(), wt.double(), bias.double()), co.bar_dwconv7(x.double(), wt.double(), bias.double())
        assert float(((out32.double() - ref).abs() / bar).max()) < 1.0


def test_folding_the_layer_scale_is_exact():
    sd = co.to64(co.state_dict())
    p = 'features.5.1.'
    w, b, ls = sd[p + 'block.5.weight'], sd[p + 'block.5.bias'], sd[p + 'layer_scale']
    wf, bf = convnext.fold_layer_scale(w, b, ls)
    a = torch.randn(5, w.shape[1], generator=torch.Generator().manual_seed(3)).double()
    x = torch.randn(5, w.shape[0], generator=torch.Generator().manual_seed(4)).double()
    folded, plain = x + (a @ wf.t() + bf), x + ls.reshape(-1) * (a @ w.t() + b)
    assert wf.shape == w.shape and bf.shape == b.shape and rel_inf(folded, plain) < 1e-14
    # ... and the depthwise weight goes tap-major
    wd = sd[p + 'block.0.weight']
    assert torch.equal(convnext.dw_weight(wd)[7 * 2 + 5], wd[:, 0, 2, 5]) and torch.equal(convnext.dw_weight(wd), co.dw_weight(wd))


def test_the_four_constructor_refusals():
    sd = co.state_dict()
    with pytest.raises(ValueError, match='multiple of 4 in both directions'):
        Classifier('convnext_tiny', 'cpu', state_dict=sd, input_sz=(64, 66))
    bad = syn.convnext_tiny_state_dict(num_classes=4, dims=(16, 32), depths=(1, 1))
    bad = {k: (v[:14] if k.startswith(('features.0.', 'features.1.')) and v.shape[0] == 16 else v) for k, v in bad.items()}
    with pytest.raises(ValueError, match='every width must be a multiple of 4'):
        Classifier('convnext_tiny', 'cpu', state_dict=bad, input_sz=(64, 64))
    with pytest.raises(ValueError, match='final map of 0 x 1'):
        Classifier('convnext_tiny', 'cpu', state_dict=sd, input_sz=(28, 32))
    with pytest.raises(NotImplementedError, match="ConvNeXtBody: storage='f16' is not implemented"):
        convnext.ConvNeXtBody(sd, co.B, (64, 64), 'cpu', storage='f16')
    # ... and a state dict of another architecture is told so, not answered with a KeyError
    with pytest.raises(ValueError, match="not a ConvNeXt's"):
        Classifier('convnext_tiny', 'cpu', state_dict=syn.resnet18_state_dict(num_classes=10), input_sz=(64, 64))


def test_classifier_is_a_known_name_and_constructs_on_the_cpu():
    sd = co.state_dict()
    clf = Classifier('convnext_tiny', 'cpu', state_dict={'module.' + k: v for k, v in sd.items()}, input_sz=co.GEOMS['odd'][2])
    assert clf.num_classes == co.NUM_CLASSES and clf.has_feature_map and not clf.has_rollout and clf.input_sz == (36, 52)
    assert set(clf.state_dict) == set(sd)                                       # keys under a `module.` prefix load as they are
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        clf.classify(torch.rand(1, 3, 40, 56), (36, 52))
    with pytest.raises(RuntimeError, match='state_dict='):
        Classifier('convnext_tiny', 'cpu')
