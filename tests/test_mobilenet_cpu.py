"""CPU: the host side of the MobileNetV2 body -- the four depthwise / ReLU6 entry points are declared and exported, the synthetic
weights have torchvision's key set and shapes, the float64 restatement (tests/mobilenet_oracle.py) differentiates correctly, the
fixtures of the GPU tests saturate every ReLU6 on BOTH sides (so that a ReLU6 implemented as a ReLU cannot pass them), and
Classifier('mobilenet_v2') constructs without a GPU and refuses to run there."""
import os
import re

import pytest
import torch

import mobilenet_cases as mc
import mobilenet_oracle as mo
import spaa_oracle as so
from spaa_amd import _lib, synthetic as syn
from spaa_amd.classifier import BODIES, INPUT_SZ, Classifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_dwconv3_fwd', 'spaa_dwconv3_bwd', 'spaa_relu6_gate', 'spaa_global_avgpool_bwd_bits')


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert 'dwconv.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert 'mobilenet_v2' in BODIES and INPUT_SZ['mobilenet_v2'] == (224, 224)


def expected_keys(num_classes):
    """torchvision.models.mobilenet_v2().state_dict() without the num_batches_tracked counters: name -> shape."""
    keys = {}

    def conv_bn(conv, bn, cout, cin_per_group, k):
        keys[conv + '.weight'] = (cout, cin_per_group, k, k)
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            keys[f'{bn}.{s}'] = (cout,)

    conv_bn('features.0.0', 'features.0.1', 32, 3, 3)
    for name, t, cin, cout, _ in mo.blocks():
        hid, j = cin * t, 0
        if t != 1:
            conv_bn(f'{name}.conv.0.0', f'{name}.conv.0.1', hid, cin, 1)
            j = 1
        conv_bn(f'{name}.conv.{j}.0', f'{name}.conv.{j}.1', hid, 1, 3)
        conv_bn(f'{name}.conv.{j + 1}', f'{name}.conv.{j + 2}', cout, hid, 1)
    conv_bn('features.18.0', 'features.18.1', 1280, 320, 1)
    keys['classifier.1.weight'], keys['classifier.1.bias'] = (num_classes, 1280), (num_classes,)
    return keys


def test_state_dict_has_torchvisions_keys_and_shapes():
    for ncls in (1000, 16):
        sd = syn.mobilenet_v2_state_dict(num_classes=ncls)
        want = expected_keys(ncls)
        assert set(sd) == set(want)
        assert len(want) == 52 * 5 + 2                                     # 52 convolutions with their BatchNorms, one linear layer
        for k, shape in want.items():
            assert tuple(sd[k].shape) == shape and sd[k].dtype == torch.float32, k
    a, b = syn.mobilenet_v2_state_dict(), syn.mobilenet_v2_state_dict(seed=6)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a['features.0.0.weight'], syn.mobilenet_v2_state_dict(seed=7)['features.0.0.weight'])
    g = syn.mobilenet_v2_state_dict(logit_gain=3.0)
    assert torch.allclose(g['classifier.1.weight'], 3.0 * a['classifier.1.weight']) and torch.equal(g['features.18.0.weight'], a['features.18.0.weight'])


def test_block_table():
    bl = mo.blocks()
    assert len(bl) == 17 and bl[0] == ('features.1', 1, 32, 16, 1) and bl[-1] == ('features.17', 6, 160, 320, 1)
    assert [b[0] for b in bl if b[4] == 2] == ['features.2', 'features.4', 'features.7', 'features.14']
    assert sum(1 for _, t, cin, cout, s in bl if s == 1 and cin == cout) == 10                       # residual blocks
    assert len(mo.SITES) == 35
    from spaa_amd import mobilenet
    assert mobilenet.block_specs() == bl


def test_oracle_gradient_agrees_with_central_differences():
    sd = mo.to64(mc.state_dict())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 8, 8, generator=g, dtype=torch.float64, requires_grad=True)
    r = torch.randn(2, mc.NUM_CLASSES, generator=g, dtype=torch.float64)
    f = lambda t: (mo.forward(sd, t) * r).sum()     # noqa: E731
    f(x).backward()
    assert float(x.grad.abs().max()) > 0
    # The network is piecewise linear, so a central difference is exact up to rounding unless a unit crosses a kink inside the step.
    # The synthetic weights keep the layer-to-layer gain near 1 (spaa_amd/synthetic.py), so a step of 1e-7 moves the hidden units by
    # ~1e-7 -- kink crossings are rare among the ~2e4 units of an 8 x 8 input -- and costs 2^-52 |f| / eps ~ 1e-8 of rounding against
    # directional derivatives of ~1e-2 .. 1.  Bar: 1e-5 of |grad| |d|.
    eps = 1e-7
    for _ in range(4):
        d = torch.randn(x.shape, generator=g, dtype=torch.float64)
        with torch.no_grad():
            num = (f(x + eps * d) - f(x - eps * d)) / (2 * eps)
        ana = (x.grad * d).sum()
        err, scale = abs(float(num - ana)), float(x.grad.norm() * d.norm())
        print(f'central differences: {float(num):.9e} against {float(ana):.9e}, error / (|grad| |d|) = {err / scale:.2e}')
        assert err <= 1e-5 * scale
    # the gate override of the oracle: with its own gates it reproduces autograd's gradient exactly
    rec = []
    mo.forward(sd, x.detach(), record=rec)
    gates = [(v > 0) & (v < 6) for v in rec]
    x2 = x.detach().clone().requires_grad_(True)
    (mo.forward(sd, x2, gates=gates) * r).sum().backward()
    assert torch.equal(x2.grad, x.grad)


@pytest.mark.parametrize('geom', list(mc.GEOMS))
def test_fixtures_saturate_every_relu6_on_both_sides(geom):
    """At both GPU-test geometries every one of the 35 ReLU6 sites has at least 5 % of its units <= 0 and at least 5 % >= 6 under the
    float64 oracle: a condition on the INPUTS of tests/test_mobilenet_gpu.py, which keeps them from passing with a ReLU in place of
    the ReLU6."""
    _, crop, insz = mc.GEOMS[geom]
    pre = so.classifier_preprocess(mc.images(geom), crop, insz).double()
    rec = []
    with torch.no_grad():
        logits = mo.forward(mo.to64(mc.state_dict()), pre, record=rec)
    assert len(rec) == 35
    lo = [float((v <= 0).double().mean()) for v in rec]
    hi = [float((v >= 6).double().mean()) for v in rec]
    print(f'{geom}: smallest share <= 0 {min(lo):.3f} ({mo.SITES[lo.index(min(lo))]}), smallest share >= 6 {min(hi):.3f} '
          f'({mo.SITES[hi.index(min(hi))]})')
    for name, a, b in zip(mo.SITES, lo, hi):
        assert a >= 0.05 and b >= 0.05, (name, a, b)
    p1 = torch.softmax(logits, dim=1).max(dim=1).values
    print(f'{geom}: top-1 probabilities {p1.tolist()}')
    assert (p1 > 1.5 / mc.NUM_CLASSES).all(), 'softmax is flat: raise LOGIT_GAIN'


def test_classifier_constructs_on_the_cpu_and_refuses_to_run_there():
    sd = mc.state_dict()
    clf = Classifier('mobilenet_v2', 'cpu', state_dict=sd)
    assert clf.num_classes == mc.NUM_CLASSES and clf.input_sz == (224, 224)
    assert Classifier('mobilenet_v2', 'cpu', state_dict=syn.mobilenet_v2_state_dict(), input_sz=(64, 64)).num_classes == 1000
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        clf.classify(torch.rand(1, 3, 64, 64), (60, 60))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        clf.grad_cam(torch.rand(1, 3, 64, 64), [0], (60, 60))
    # the other names keep reading their own last layer
    assert Classifier('resnet18', 'cpu', state_dict=syn.resnet18_state_dict(num_classes=10)).num_classes == 10
    with pytest.raises(ValueError, match='unknown classifier'):
        Classifier('mobilenet_v3', 'cpu', state_dict=sd)
