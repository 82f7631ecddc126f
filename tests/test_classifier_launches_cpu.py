"""CPU: the classifier bodies launch what they launched before their pooling calls moved behind spaa_amd/pooling.py and their shared
parts into ClassifierBody: every entry point and plan of a forward pass, a backward pass and a forward pass without gate masks, with
every integer argument, every keyword of a plan run and every tensor (labelled by first appearance, with shape and dtype), against
tests/golden/classifier_launch_sequences.json -- recorded by tools/classifier_sequences.py from the commit before that change.
Nothing runs on a GPU: the recorder builds the bodies on device='cpu' and replaces the launches by stubs.

The second half checks that the pooling wrappers refuse, on the host and before any launch, the operands the kernels cannot check."""
import importlib.util
import inspect
import json
import os
import re

import pytest
import torch

from spaa_amd import _lib, classifier, inception, pooling

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'classifier_launch_sequences.json')
_spec = importlib.util.spec_from_file_location('classifier_sequences', os.path.join(os.path.dirname(HERE), 'tools', 'classifier_sequences.py'))
seq = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(seq)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)['sequences']


@pytest.fixture(scope='module')
def recorded():
    """config name -> its three stages, recorded once per configuration (1-4 s each); state dicts once per body."""
    sds, done = {}, {}

    def get(c):
        name = seq.config_name(c)
        if name not in done:
            sd = sds.setdefault(c['body'], seq.state_dict(c['body']))
            done[name] = json.loads(json.dumps(seq.record(c, sd)))
        return done[name]
    return get


def test_fixture_holds_the_configurations(golden):
    assert sorted(golden) == sorted(seq.config_name(c) for c in seq.CONFIGS)
    assert all(sorted(v) == sorted(seq.STAGES) and all(v[s] for s in seq.STAGES) for v in golden.values())
    # the routes the configurations are there for
    entries = lambda name, stage: [r[0] for r in golden[name][stage]]  # noqa: E731
    tile = {name: [r[1] for r in v['backward'] if r[0] == 'plan:layer2.0.conv1_dgrad'] for name, v in golden.items() if name.startswith('resnet18')}
    assert tile.pop('resnet18-f32-b32-224') == [74] and all(t == [0] for t in tile.values())
    assert 'spaa_maxpool3s2_fwd' in entries('resnet18-f32-b2-64', 'forward') and 'spaa_maxpool3s2_bwd' in entries('resnet18-f32-b2-64', 'backward')
    assert 'spaa_maxpool_fwd_f16' in entries('resnet18-f16-b2-64', 'forward') and 'spaa_maxpool_bwd_f16' in entries('resnet18-f16-b2-64', 'backward')
    assert not any(e.startswith('spaa_maxpool') for e in entries('resnet18-f32-b2-64-FUSE_POOL_ADJOINT=True', 'backward'))
    assert 'spaa_adaptive_avgpool_fwd' in entries('vgg16-f32-b2-64', 'forward') and 'spaa_adaptive_avgpool_bwd' in entries('vgg16-f32-b2-64', 'backward')
    assert not any(e.startswith('spaa_') for e in entries('vgg16-f16-b1-224', 'forward') + entries('vgg16-f16-b1-224', 'backward'))
    assert entries('vgg16-f16-b1-224-fuse_pool=False', 'forward').count('spaa_maxpool_fwd_f16') == 5
    assert {'spaa_maxpool_fwd', 'spaa_gate_mask', 'spaa_avgpool2d_fwd', 'spaa_avgpool_fwd'} <= set(entries('inception_v3-f32-b2-75', 'forward'))
    assert 'spaa_gate_mask' not in entries('inception_v3-f32-b2-75', 'forward_nomask')
    assert {'spaa_maxpool_bwd_f16', 'spaa_avgpool2d_bwd_f16', 'spaa_avgpool_bwd_f16'} <= set(entries('inception_v3-f16-b2-75', 'backward'))


@pytest.mark.parametrize('stage', seq.STAGES)
@pytest.mark.parametrize('cfg', seq.CONFIGS, ids=seq.config_name)
def test_launches_are_the_recorded_ones(cfg, stage, golden, recorded):
    got, want = recorded(cfg)[stage], golden[seq.config_name(cfg)][stage]
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{seq.config_name(cfg)} {stage}, launch {n}'
    assert len(got) == len(want)


def test_bodies_launch_through_wrappers_only():
    """No raw entry-point call and no `_f16` choice in a body's passes; the pooling entry points are named in pooling.py and _lib.py only."""
    for body in (classifier.ResNet18Body, classifier.VGG16Body, inception.InceptionV3Body):
        for fn in (body.forward, body.backward):
            src = inspect.getsource(fn)
            assert '_lib.call' not in src and '_f16' not in src, fn.__qualname__
    pkg = os.path.dirname(os.path.abspath(classifier.__file__))
    names = re.compile(r'spaa_(maxpool|avgpool|adaptive_avgpool|gate_mask)')
    for fname in sorted(os.listdir(pkg)):
        if fname.endswith('.py') and fname not in ('pooling.py', '_lib.py'):
            with open(os.path.join(pkg, fname)) as fh:
                assert not names.search(fh.read()), fname
    assert not hasattr(inception, 'BODY_GATE_MASKS') and not hasattr(inception, 'USE_GATE_MASKS')      # (each switch is read in one place)


def test_engine_without_probes():
    src = inspect.getsource(classifier.ClassifierEngine)
    assert 'hasattr' not in src and 'getattr' not in src
    for body in (classifier.ResNet18Body, classifier.VGG16Body, inception.InceptionV3Body):
        assert issubclass(body, classifier.ClassifierBody)
    assert classifier.X6P_DGRAD_MIN_PIXELS == 100000


# ---- the wrappers' host-side checks ---------------------------------------------------------------------------------

def t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


F16, U8 = torch.float16, torch.uint8
BAD = {
    'dtypes_differ': (lambda: pooling.maxpool_fwd(t(2, 9, 11, 8), t(2, 4, 5, 8, dtype=F16), t(2, 4, 5, 8, dtype=U8), 3, 2, 0), '`out`.*storage type'),
    'dtypes_differ_bwd': (lambda: pooling.avgpool2d_bwd(t(2, 9, 11, 8, dtype=F16), t(2, 9, 11, 8), 3, 1, 1), '`g_in`.*storage type'),
    'batch_differs': (lambda: pooling.avgpool2d_fwd(t(2, 9, 11, 8), t(3, 9, 11, 8), 3, 1, 1), '`out`.*batch'),
    'not_4d': (lambda: pooling.global_avgpool_fwd(t(2, 99, 8), t(2, 1, 1, 8)), '`x` must be a 4-D'),
    'int_activation': (lambda: pooling.gate_mask(t(2, 4, 5, 8, dtype=torch.int32), t(2, 4, 5, 2, dtype=U8), 8), '`act` must be a 4-D'),
    'output_size': (lambda: pooling.maxpool_fwd(t(2, 9, 11, 8), t(2, 5, 5, 8), t(2, 5, 5, 8, dtype=U8), 3, 2, 0), '`out` is 5 x 5.*gives 4 x 5'),
    'output_size_avg': (lambda: pooling.avgpool2d_fwd(t(2, 9, 11, 8), t(2, 9, 10, 8), 3, 1, 1), '`out` is 9 x 10.*gives 9 x 11'),
    'output_size_bwd': (lambda: pooling.maxpool_bwd(t(2, 5, 5, 8), t(2, 5, 5, 8, dtype=U8), t(2, 9, 11, 8), 3, 2, 1, True), '`g_out` is 5 x 5.*gives 5 x 6'),
    'window_past_buffer': (lambda: pooling.maxpool_fwd(t(2, 9, 11, 8), t(2, 4, 5, 16), t(2, 4, 5, 8, dtype=U8), 3, 2, 0, out_coff=12), r'\[12, 12 \+ 8\) of `out` \(16 wide\)'),
    'window_past_buffer_bwd': (lambda: pooling.avgpool2d_bwd(t(2, 9, 11, 16), t(2, 9, 11, 12), 3, 1, 1, gout_coff=8), r'\[8, 8 \+ 12\) of `g_out` \(16 wide\)'),
    'offset_not_4': (lambda: pooling.maxpool_fwd(t(2, 9, 11, 8), t(2, 4, 5, 16), t(2, 4, 5, 8, dtype=U8), 3, 2, 0, out_coff=6), 'multiples of 4'),
    'channels_not_4': (lambda: pooling.maxpool_fwd(t(2, 9, 11, 6), t(2, 4, 5, 6), t(2, 4, 5, 6, dtype=U8), 3, 2, 0), 'multiples of 4'),
    'channels_not_4_gate': (lambda: pooling.gate_mask(t(2, 4, 5, 16), t(2, 4, 5, 4, dtype=U8), 6, 8), 'multiples of 4'),
    'argmax_not_bytes': (lambda: pooling.maxpool_fwd(t(2, 9, 11, 8), t(2, 4, 5, 8), t(2, 4, 5, 8), 3, 2, 0), '`arg` must be torch.uint8'),
    'argmax_shape': (lambda: pooling.maxpool_bwd(t(2, 4, 5, 16), t(2, 4, 5, 16, dtype=U8), t(2, 9, 11, 8), 3, 2, 0, False, 8), r'`arg` must be torch.uint8 \(2, 4, 5, 8\)'),
    'mask_shape': (lambda: pooling.gate_mask(t(2, 4, 5, 16), t(2, 4, 5, 2, dtype=U8), 8, 8), r'`mask` must be torch.uint8 \(2, 4, 5, 4\)'),
    'max_k12': (lambda: pooling.maxpool_fwd(t(2, 13, 13, 8), t(2, 2, 2, 8), t(2, 2, 2, 8, dtype=U8), 12, 1, 0), 'k=12.*k <= 11'),
    'max_k12_bwd': (lambda: pooling.maxpool_bwd(t(2, 2, 2, 8), t(2, 2, 2, 8, dtype=U8), t(2, 13, 13, 8), 12, 1, 0, True), 'k=12.*k <= 11'),
    'avg_k16': (lambda: pooling.avgpool2d_fwd(t(2, 17, 17, 8), t(2, 2, 2, 8), 16, 1, 0), 'k=16.*k <= 15'),
    'padding_over_half': (lambda: pooling.avgpool2d_fwd(t(2, 9, 11, 8), t(2, 11, 13, 8), 3, 1, 2), '2p <= k'),
    'unpool_width': (lambda: pooling.maxpool_bwd(t(2, 4, 5, 16), t(2, 4, 5, 8, dtype=U8), t(2, 8, 10, 16), 2, 2, 0, True, c=8), '`g_in` is 16 channels wide, the caller pools 8'),
    'features_f16': (lambda: pooling.global_avgpool_fwd(t(2, 9, 11, 8, dtype=F16), t(2, 1, 1, 8, dtype=F16)), '`feat` must be fp32'),
    'features_size': (lambda: pooling.global_avgpool_bwd(t(2, 1, 1, 16), None, t(2, 9, 11, 8)), r'`g_feat` must be fp32 \[2, ..., 8\]'),
    'global_gate_shape': (lambda: pooling.global_avgpool_bwd(t(2, 1, 1, 8), t(2, 9, 10, 8), t(2, 9, 11, 8)), '`act` must be'),
    'adaptive_f16': (lambda: pooling.adaptive_avgpool_fwd(t(2, 9, 11, 8, dtype=F16), t(2, 7, 7, 8, dtype=F16)), 'fp32 only'),
    'adaptive_channels': (lambda: pooling.adaptive_avgpool_bwd(t(2, 7, 7, 8), None, t(2, 9, 11, 12)), 'same channel count'),
}


@pytest.mark.parametrize('name', sorted(BAD))
def test_wrapper_refuses(name, monkeypatch):
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda *a: launched.append(a))
    monkeypatch.setattr(_lib, 'check_dev', lambda *a, **k: None)       # (CPU tensors: the refusal must come from the wrapper's own check)
    monkeypatch.setattr(_lib, 'check_mask', lambda *a, **k: None)
    fn, match = BAD[name]
    with pytest.raises(ValueError, match=match):
        fn()
    assert not launched


def test_wrappers_refuse_cpu_tensors():
    """With nothing stubbed, a tensor that is not on the GPU never reaches a launch."""
    with pytest.raises(ValueError, match='on the GPU'):
        pooling.avgpool2d_fwd(t(2, 9, 11, 8), t(2, 9, 11, 8), 3, 1, 1)
    with pytest.raises(ValueError, match='on the GPU'):
        pooling.global_avgpool_fwd(t(2, 9, 11, 8), t(2, 1, 1, 8))
