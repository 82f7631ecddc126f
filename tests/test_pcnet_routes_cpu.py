"""pcnet_routes() (spaa_amd/models.py): which kernel serves which ShadingNet layer, decided without a GPU.  The expected routes are
what the engine chose before the decisions moved out of PCNetEngine.__init__ (its attributes at that commit, read on the GPU)."""
import pytest
import torch

from spaa_amd import models as M

FUSED = dict(skip3='fused', conv1_pair='fused', tail='fused', clamp_gate='byte')
SEPARATE = dict(skip2='separate', skip3='separate', conv1_pair='separate', conv1_pair_bwd='separate')


@pytest.fixture(scope='module')
def nets():
    torch.manual_seed(0)
    return {True: M.ShadingNetSPAA(True), False: M.ShadingNetSPAA(False), 'cache': {}}


def routes(nets, storage, rough=True, batch=64, cam=(256, 256), **kw):
    """(record, route strings); a record is built once per distinct set of arguments and module flags (plans and images take a while to pack)."""
    flags = tuple(getattr(M, k) for k in ('FS2_H16', 'S2F_X6', 'FUSE_SKIP2', 'FUSE_SKIP2_MIN_PIXELS', 'FUSE_TAIL'))
    key = (storage, rough, batch, cam, tuple(sorted(kw.items())), flags)
    if key not in nets['cache']:
        nets['cache'][key] = M.pcnet_routes(nets[rough], rough, batch, cam, storage, device='cpu', **kw)
    return nets['cache'][key], M.describe_routes(nets['cache'][key])


def has(names, **want):
    return {k: names[k] for k in want} == want


def test_default_f32(nets):
    r, n = routes(nets, 'f32')
    assert has(n, skip2='x6p', s2f='x6', conv1_pair_bwd='separate', **FUSED)
    assert r.fuse_skip2 and r.fuse_skip3 and r.fuse_tail and r.want_gate_y and r.d['conv2_s'].fixed_tile == 74
    assert {'transConv1x', 'conv5x'} <= set(r.f) and {'conv2x', 'conv3x'} <= set(r.d)
    assert r.fs2 is None and sorted(r.s2fx) == ['f2', 'f2s'] and r.pair1 is not None and r.pair1_bwd is None
    assert sorted(r._packed_from) == ['conv1', 'conv1_s', 'conv2', 'conv2_s', 'conv6', 'transConv2']


def test_default_f16(nets):
    r, n = routes(nets, 'f16')
    assert has(n, skip2='fs2', s2f='h16', conv1_pair_bwd='fused', **FUSED)
    assert sorted(r.fs2) == ['c2', 'c2s', 'f2', 'f2s', 'tc', 'tcd'] and r.s2fx is None and r.pair1_bwd is not None
    assert {'transConv1x', 'conv5x'} <= set(r.f) and {'conv2x', 'conv3x'} <= set(r.d)
    assert sorted(r._packed_from) == ['conv1', 'conv1_s', 'conv2', 'conv2_s', 'conv6', 'skipConv2', 'transConv1', 'transConv2']


@pytest.mark.parametrize('storage', ['f32', 'f16'])
def test_fuse_skip2_false_is_every_layer_on_its_plan(nets, storage):
    r, n = routes(nets, storage, fuse_skip2=False)
    assert has(n, s2f='plan', tail='fused', clamp_gate='byte', **SEPARATE)
    assert not r.fuse_skip2 and not r.fuse_skip3 and r.fs2 is r.s2fx is r.pair1 is r.pair1_bwd is None
    assert not {'transConv1x', 'conv5x'} & set(r.f) and not {'conv2x', 'conv3x'} & set(r.d)
    # ... and with the tail off (the training step) no packed image is left, and no clamp-gate bytes are wanted
    r, n = routes(nets, storage, fuse_skip2=False, fuse_tail=False)
    assert has(n, s2f='plan', tail='separate', clamp_gate='ypre', **SEPARATE)
    assert not r.fuse_tail and not r.want_gate_y and r._packed_from == {}


def test_few_pixels_keep_the_routes_that_do_not_need_skip2(nets):
    r, n = routes(nets, 'f32', batch=1, cam=(64, 64))      # 256 < FUSE_SKIP2_MIN_PIXELS = 16384
    assert has(n, skip2='separate', s2f='x6', skip3='separate', conv1_pair='fused', conv1_pair_bwd='separate',
               tail='fused', clamp_gate='byte')


def test_no_rough_f16(nets):
    r, n = routes(nets, 'f16', rough=False)
    assert has(n, skip2='h16p', conv1_pair='separate', conv1_pair_bwd='separate', tail='fused', clamp_gate='byte')
    assert r.fs2 is None and 'transConv1x' in r.f and 'conv2x' in r.d and 'conv2_s' not in r.d


def test_switches(nets, monkeypatch):
    monkeypatch.setattr(M, 'FS2_H16', False)
    assert has(routes(nets, 'f16')[1], skip2='h16p', s2f='plan', **FUSED)
    monkeypatch.setattr(M, 'S2F_X6', False)
    assert has(routes(nets, 'f32')[1], skip2='x6p', s2f='plan', **FUSED)
    monkeypatch.setattr(M, 'FUSE_SKIP2', 31 & ~8)
    assert has(routes(nets, 'f32')[1], skip2='x6p', skip3='separate', conv1_pair='fused')
    monkeypatch.setattr(M, 'FUSE_SKIP2', 31 & ~16)
    assert has(routes(nets, 'f32')[1], skip2='x6p', skip3='fused', conv1_pair='separate', conv1_pair_bwd='separate')
    monkeypatch.setattr(M, 'FUSE_SKIP2', 31)
    monkeypatch.setattr(M, 'FUSE_SKIP2_MIN_PIXELS', 0)
    assert has(routes(nets, 'f32', batch=1, cam=(64, 64))[1], skip2='x6p', skip3='fused')
    monkeypatch.setattr(M, 'FUSE_TAIL', False)
    r, n = routes(nets, 'f32')
    assert has(n, tail='separate', clamp_gate='ypre') and not r.want_gate_y


def test_arguments_are_checked(nets):
    with pytest.raises(ValueError, match='storage'):
        routes(nets, 'bf16')
    with pytest.raises(ValueError, match='divisible by 4'):
        routes(nets, 'f32', cam=(250, 256))
    with pytest.raises(ValueError, match='conv1_s'):
        M.pcnet_routes(nets[False], True, 2, (64, 64))
