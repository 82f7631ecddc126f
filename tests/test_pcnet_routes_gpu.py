"""PCNetEngine launches what it launched before its routes moved into pcnet_routes() and its hand-fused kernels behind one wrapper
each: the order of entry points (every _lib.call) and plans (every ConvPlan.run) of set_scene, one forward and one backward pass
against tests/golden/pcnet_launch_sequences.json, recorded with this module's recorder (tools/engine_digest.py --sequences) from
the commit before that change.  Camera (48, 80), projector (64, 64), batch 2, FUSE_SKIP2_MIN_PIXELS = 0: the smallest shape of the
fused-route tests with a non-square, ragged-tile camera and every route alive.  The helpers use only the constructor arguments and
attributes that commit had, so that the recorder and tools/engine_digest.py run on both sides of the change."""
import contextlib
import json
import os

import pytest
import torch

from spaa_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CAM, PRJ, B = (48, 80), (64, 64), 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pcnet_launch_sequences.json')
# storage x (default routes | fuse_skip2=False with the tail off, as the training step) x use_rough, and the attack loop's
# backward(None, select=..., sumsq=...) on the two default rough engines (a scalar prjl2 scale in fp32, one per sample in fp16)
CONFIGS = [dict(storage=s, fused=fu, rough=r, select=False) for s in ('f32', 'f16') for fu in (True, False) for r in (True, False)] \
    + [dict(storage=s, fused=True, rough=True, select=True) for s in ('f32', 'f16')]


def config_name(c):
    return '-'.join([c['storage'], 'default' if c['fused'] else 'separate', 'rough' if c['rough'] else 'norough'] + ['select'] * c['select'])


def build_engine(M, cfg, tail_argument=False):
    """(PCNet, PCNetEngine) of a configuration.  The tail goes off through the attribute (`tail_argument`: through the constructor)."""
    sd = syn.pcnet_state_dict(5, cam_sz=CAM, mask='rect')
    if not cfg['rough']:   # ShadingNetSPAA(use_rough=False) has a 3-channel conv1_s
        sd['shading_net.conv1_s.weight'] = sd['shading_net.conv1_s.weight'][:, :3].contiguous()
    pc = M.PCNet(sd['mask'], M.WarpingNet(out_size=CAM), use_rough=cfg['rough'])
    pc.load_state_dict(sd)
    pc = pc.to(DEV)
    kw = {} if cfg['fused'] else dict(fuse_skip2=False, **(dict(fuse_tail=False) if tail_argument else {}))
    old, M.FUSE_SKIP2_MIN_PIXELS = M.FUSE_SKIP2_MIN_PIXELS, 0
    try:
        eng = M.PCNetEngine(pc, B, PRJ, cfg['storage'], **kw)
    finally:
        M.FUSE_SKIP2_MIN_PIXELS = old
    if not cfg['fused'] and not tail_argument:
        eng.fuse_tail = False
    return pc, eng


def run_passes(M, eng, cfg, between=lambda stage: None):
    """set_scene, forward and backward on seeded inputs; `between(stage)` is called before each.  Returns the sumsq partials or None."""
    gen = torch.Generator().manual_seed(7)
    x = M.to_nhwc4(torch.rand(B, 3, *PRJ, generator=gen).to(DEV))
    scene = M.to_nhwc4(syn.scenes(3, B, CAM).to(DEV))
    g = [torch.randn(B, *CAM, 4, generator=gen).to(DEV) for _ in range(2)]
    for t in g:
        t[..., 3] = 0
    between('set_scene')
    eng.set_scene(scene)
    between('forward')
    eng.forward(x)
    between('backward')
    if not cfg['select']:
        eng.backward(g[0])
        return None
    state = torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.int32, device=DEV)   # (sample 1 takes the second cotangent)
    part = torch.zeros(B, eng.sumsq_tiles(), device=DEV)
    scale = 1e-3 if cfg['storage'] == 'f32' else torch.tensor([1e-3, 2e-3], device=DEV)
    eng.backward(None, select=(g[0], g[1], state), sumsq=(part, 0.5, scale, state))
    return part


@contextlib.contextmanager
def recording(lib, cp, seq):
    """Appends the name of every _lib.call and 'plan:<name>' of every ConvPlan.run to `seq`."""
    call, run = lib.call, cp.ConvPlan.run

    def rec_call(name, *args):
        seq.append(name)
        return call(name, *args)

    def rec_run(self, *args, **kw):
        seq.append('plan:' + self.name)
        return run(self, *args, **kw)

    lib.call, cp.ConvPlan.run = rec_call, rec_run
    try:
        yield
    finally:
        lib.call, cp.ConvPlan.run = call, run


def record_sequences(M, lib, cp, cfg, tail_argument=False):
    """{'set_scene': [...], 'forward': [...], 'backward': [...]} of a configuration."""
    _, eng = build_engine(M, cfg, tail_argument)
    assert not cfg['select'] or (eng.can_select() and eng.sumsq_tiles() > 0)
    stages = {}
    with recording(lib, cp, seq := []):
        run_passes(M, eng, cfg, lambda stage: stages.setdefault(stage, len(seq)))
    torch.cuda.synchronize()
    cuts = list(stages.values()) + [len(seq)]
    return {stage: seq[cuts[i]:cuts[i + 1]] for i, stage in enumerate(stages)}


@pytest.fixture(scope='module')
def hip():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib, convplan, models
    _lib.load()
    return dict(lib=_lib, cp=convplan, models=models)


@pytest.mark.parametrize('cfg', CONFIGS, ids=config_name)
def test_launch_sequence_is_the_recorded_one(hip, cfg):
    with open(GOLDEN) as fh:
        want = json.load(fh)['sequences'][config_name(cfg)]
    got = record_sequences(hip['models'], hip['lib'], hip['cp'], cfg, tail_argument=True)
    for stage in ('set_scene', 'forward', 'backward'):
        assert got[stage] == want[stage], f'{config_name(cfg)} {stage}'


def test_describe_and_workspaces_follow_the_constructor(hip):
    """The engine reports its routes, and one built with the tail off allocates no clamp-gate bytes."""
    M = hip['models']
    _, e1 = build_engine(M, dict(storage='f16', fused=True, rough=True))
    _, e0 = build_engine(M, dict(storage='f16', fused=False, rough=True), tail_argument=True)
    assert e1.describe() == dict(skip2='fs2', s2f='h16', skip3='fused', conv1_pair='fused', conv1_pair_bwd='fused', tail='fused',
                                 clamp_gate='byte', select='head', warp_bwd='tiled', sumsq='fused')
    assert e0.describe() == dict(skip2='separate', s2f='plan', skip3='separate', conv1_pair='separate',
                                 conv1_pair_bwd='separate', tail='separate', clamp_gate='ypre', select='separate', warp_bwd='tiled', sumsq='fused')
    assert e1.gate_y is not None and e0.gate_y is None and not e0.fuse_tail
    e1.pair1 = e1.pair1_bwd = None      # (switched on the live engine, as the parity tests do)
    assert e1.describe()['conv1_pair'] == e1.describe()['conv1_pair_bwd'] == 'separate'


def test_stale_packed_weights_and_missing_scene_raise(hip):
    """Host-side errors, before any launch: a parameter behind a packed weight image changed after the engine was built, and
    a['Ypre'] asked for before set_scene()."""
    M = hip['models']
    pc, eng = build_engine(M, dict(storage='f32', fused=True, rough=True))
    with pytest.raises(RuntimeError, match=r'call set_scene\(\) first'):
        eng.a['Ypre']
    scene = torch.zeros(B, *CAM, 4, device=DEV)
    with torch.no_grad():
        pc.shading_net.skipConv3.weight.mul_(1.0)      # (no packed image: the plans are the trainer's to refresh)
    with recording(hip['lib'], hip['cp'], seq := []):
        eng.set_scene(scene)
        with torch.no_grad():
            pc.shading_net.conv2.weight.mul_(1.0)
        n = len(seq)
        with pytest.raises(RuntimeError, match='shading_net.conv2 has changed'):
            eng.set_scene(scene)
    assert n > 0 and len(seq) == n
    # the training step's engine uses none of the images: its parameters change every step
    pc0, e0 = build_engine(M, dict(storage='f32', fused=False, rough=True), tail_argument=True)
    with torch.no_grad():
        for p in pc0.shading_net.parameters():
            p.mul_(1.0)
    e0.set_scene(scene)
