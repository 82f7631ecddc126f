"""What the classifier bodies (ResNet-18, VGG-16, Inception-v3) launch, recorded WITHOUT a GPU: the bodies are built and walked on
device='cpu' with `_lib.call`, `ConvPlan.run` and `SmallLinearPlan.run` replaced by recorders and the device checks by stubs (the
technique of tests/test_convplan_launch_cpu.py).  Nothing is computed.  A launch is kept as a list: the entry point, or
'plan:<name>' followed by the plan's `fixed_tile`; then every argument in order -- integers as they are, tensors and pointers as
't<n>:<shape>:<dtype>' with n counted by first appearance within the stage (pointers by the tensor `_lib.ptr` / `_lib.hptr` was last
asked for at that address) -- and, for a plan, a dict of its keywords that are not None.

    python tools/classifier_sequences.py [--root DIR] OUT.json

writes the fixture tests/golden/classifier_launch_sequences.json, one line per configuration (recorded ONCE, from the commit before a
change that must keep the launches; tests/test_classifier_launches_cpu.py compares).  Only constructor arguments, attributes and module
switches of that commit are used, so the recorder runs on both sides of such a change.  --root: the checkout whose spaa_amd runs."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def cfg(body, storage, batch, hw, live=None, **switches):
    """`switches`: module attributes of spaa_amd.classifier / spaa_amd.inception during construction and the passes; `live`: attributes
    set on the built body."""
    return dict(body=body, storage=storage, batch=batch, hw=hw, live=live or {}, switches=switches)


CONFIGS = [
    cfg('resnet18', 'f32', 2, 64), cfg('resnet18', 'f16', 2, 64),
    cfg('resnet18', 'f32', 32, 224),      # the only shape on the tile-74 route of layer2.0.conv1_dgrad: 32 * 56 * 56 >= 100000
    cfg('resnet18', 'f32', 2, 64, FUSE_POOL_ADJOINT=True),
    cfg('resnet18', 'f16', 2, 64, FOLD_S2_F16=1), cfg('resnet18', 'f16', 2, 64, FOLD_S2_F16=2),
    cfg('resnet18', 'f32', 2, 64, USE_GATE_MASKS=False),
    cfg('vgg16', 'f32', 2, 64),           # (2 x 2 features: the adaptive pool)
    cfg('vgg16', 'f32', 1, 224), cfg('vgg16', 'f16', 1, 224),
    cfg('vgg16', 'f16', 1, 224, live=dict(fuse_pool=False)),
    cfg('vgg16', 'f32', 2, 64, BODY_GATE_MASKS=False),
    cfg('inception_v3', 'f32', 2, 75), cfg('inception_v3', 'f16', 2, 75),
    cfg('inception_v3', 'f32', 2, 75, FUSE_ENTRY=False),
    cfg('inception_v3', 'f32', 2, 75, BODY_GATE_MASKS=False),
]
STAGES = ('forward', 'backward', 'forward_nomask')     # forward_nomask: the forward pass once more with write_masks = False
_DTYPES = {torch.float32: 'f32', torch.float16: 'f16', torch.uint8: 'u8'}


def config_name(c):
    extra = [f'{k}={v}' for k, v in sorted({**c['switches'], **c['live']}.items())]
    return '-'.join([c['body'], c['storage'], f"b{c['batch']}", str(c['hw'])] + extra)


def state_dict(body, num_classes=10):
    from spaa_amd import synthetic as syn
    if body == 'vgg16':
        return syn.vgg16_state_dict(num_classes=num_classes, fc_width=64)
    return dict(resnet18=syn.resnet18_state_dict, inception_v3=syn.inception_v3_state_dict)[body](num_classes=num_classes)


class Recorder:
    def __init__(self):
        self.seq, self.labels, self.seen = [], {}, {}

    def cut(self):
        seq, self.seq, self.labels = self.seq, [], {}
        return seq

    def see(self, t):
        if t is not None:
            self.seen[t.data_ptr()] = (tuple(t.shape), t.dtype)

    def label(self, address):
        shape, dtype = self.seen[address]
        n = self.labels.setdefault(address, len(self.labels))
        return f"t{n}:{'x'.join(map(str, shape))}:{_DTYPES[dtype]}"

    def value(self, v):
        if isinstance(v, torch.Tensor):
            self.see(v)
            return self.label(v.data_ptr())
        if isinstance(v, C.c_void_p):
            return self.label(v.value)
        if isinstance(v, (tuple, list)):
            return [self.value(x) for x in v]
        assert v is None or isinstance(v, (bool, int)), v
        return v


@contextlib.contextmanager
def recording(rec):
    from spaa_amd import _lib, convplan as cp
    saved = [(_lib, k, getattr(_lib, k)) for k in ('call', 'check_dev', 'check_mask', '_same_device', 'ptr', 'hptr')]
    saved += [(cp.ConvPlan, 'run', cp.ConvPlan.run), (cp.SmallLinearPlan, 'run', cp.SmallLinearPlan.run)]
    ptr, hptr = _lib.ptr, _lib.hptr

    def seeing(fn):
        def wrapped(t):
            rec.see(t)
            return fn(t)
        return wrapped

    def run(self, inp, out, **kw):
        rec.seq.append(['plan:' + self.name, self.fixed_tile, rec.value(inp), rec.value(out),
                        {k: rec.value(v) for k, v in kw.items() if v is not None}])
        return out

    _lib.call = lambda name, *args: rec.seq.append([name] + [rec.value(a) for a in args])
    _lib.check_dev = _lib.check_mask = lambda *a, **k: None
    _lib._same_device = lambda t: None
    _lib.ptr, _lib.hptr = seeing(ptr), seeing(hptr)
    cp.ConvPlan.run = cp.SmallLinearPlan.run = run
    try:
        yield
    finally:
        for obj, k, v in saved:
            setattr(obj, k, v)


@contextlib.contextmanager
def switched(switches):
    from spaa_amd import classifier, inception
    saved = [(m, k, getattr(m, k)) for m in (classifier, inception) for k in switches if hasattr(m, k)]
    assert {k for _, k, _ in saved} == set(switches), 'unknown switch'
    for m, k, _ in saved:
        setattr(m, k, switches[k])
    try:
        yield
    finally:
        for m, k, v in saved:
            setattr(m, k, v)


def record(c, sd=None):
    """{'forward': [...], 'backward': [...], 'forward_nomask': [...]} of a configuration."""
    from spaa_amd import classifier
    out = {}
    with switched(c['switches']), recording(rec := Recorder()):
        body = classifier.BODIES[c['body']](sd or state_dict(c['body']), c['batch'], (c['hw'], c['hw']), 'cpu', c['storage'])
        for k, v in c['live'].items():
            assert hasattr(body, k), k
            setattr(body, k, v)
        x4, g = torch.zeros(c['batch'], c['hw'], c['hw'], 4), torch.zeros(c['batch'], 10)
        body.forward(x4)
        out['forward'] = rec.cut()
        body.backward(g)
        out['backward'] = rec.cut()
        body.write_masks = False
        body.forward(x4)
        out['forward_nomask'] = rec.cut()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(HERE))
    ap.add_argument('out')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import spaa_amd
    print(f'# spaa_amd from {os.path.dirname(os.path.abspath(spaa_amd.__file__))}')
    sds, lines = {}, []
    for c in CONFIGS:
        sd = sds.setdefault(c['body'], state_dict(c['body']))
        lines.append(f' {json.dumps(config_name(c))}: {json.dumps(record(c, sd), separators=(",", ":"))}')
        print(config_name(c))
    with open(args.out, 'w') as fh:
        fh.write('{"sequences": {\n' + ',\n'.join(lines) + '\n}}\n')


if __name__ == '__main__':
    main()
