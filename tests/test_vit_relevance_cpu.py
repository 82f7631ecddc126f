"""CPU: the host side of the ViT's relevance rollout -- the two entry points are declared and exported, the float64
restatement (tests/vit_relevance_oracle.py) is consistent with itself (the recurrence the kernels run against the matrix form, the
recomputed P and dP against autograd's), every mutation of it lands beyond its bar on the inputs the GPU tests use, and
Attention(rollout=...) is validated and lets a ViT through exactly where it is set."""
import os
import re

import pytest
import torch

import spaa_oracle as so
import vit_oracle as vo
import vit_relevance_oracle as ro
from spaa_amd import _lib, synthetic as syn
from spaa_amd.classifier import Attention, Classifier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_attn_relevance', 'spaa_relevance_map')
TARGETS = [3, 7, 12]
MAP_BAR = 1e-4            # tests/test_vit_relevance_gpu.py: |M - M_ref| on M in [0, 1]


def pre64(geom):
    _, crop, insz = vo.GEOMS[geom][:3]
    return so.classifier_preprocess(vo.images(geom), crop, insz).double()


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES


@pytest.mark.parametrize('geom', list(vo.GEOMS))
def test_recurrence_is_the_matrix_form(geom):
    """Row 0 of (I + A_L) ... (I + A_1) by the matrix product and by the row vector pushed down from the top layer: <= 1e-12; and the
    condition of the GPU tests: every sample's maximum is positive."""
    sd = vo.to64(vo.state_dict(geom))
    As = [ro._abar(z) for z in ro.layer_products(sd, pre64(geom), TARGETS)]
    assert len(As) == vo.GEOMS[geom][5] and As[0].shape == (vo.B, vo.config(sd)[3], vo.config(sd)[3])
    a, b = ro.rollout_matrix(As), ro.rollout_rows(As)
    err = float((a - b).abs().max())
    m, cmax = ro.network_map(sd, pre64(geom), TARGETS)
    print(f'{geom}: recurrence against matrix form {err:.2e}; cmax {cmax.tolist()}')
    assert err <= 1e-12
    assert (cmax > 0).all() and float(m.max()) == 1.0 and float(m.min()) >= 0.0
    assert all(float(A.min()) >= 0 for A in As)
    # ... and by step(), layer by layer on the network's own qkv, lse and g_ctx with the loop's seeds divided out: what the kernels
    # are given.  (dP must be the gradient through everything above the layer, the later layers' attention included: with the
    # probabilities cut out of the graph the two differ at depth 2 and 3.)
    rho = ro.network_rows(sd, pre64(geom), TARGETS, torch.tensor([-1.0 / 3.0, 0.25, 1.0], dtype=torch.float64))
    assert float((rho - a).abs().max()) <= 1e-12 and float((ro.normalised(ro.class_map(rho)[0]) - m).abs().max()) <= 1e-12


def test_step_recomputes_what_autograd_gives():
    """step() forms P from lse and dP = g_ctx v^T itself; against a softmax whose probabilities are leaves of autograd's graph, with the
    loop's cotangent a multiple `seed` of the class logit's gradient (here: of g_ctx)."""
    heads, D, T = 12, 48, 7
    gen = torch.Generator().manual_seed(2)
    qkv = torch.randn(2, T, 3 * D, dtype=torch.float64, generator=gen)
    g = torch.randn(2, T, D, dtype=torch.float64, generator=gen)
    rho = torch.rand(2, T, dtype=torch.float64, generator=gen)
    seed = torch.tensor([-0.5, 0.25], dtype=torch.float64)
    q, k, v = vo.split_heads(qkv, heads)
    pr = torch.softmax(q @ k.transpose(-1, -2) / (D // heads) ** 0.5, dim=-1).detach().requires_grad_(True)
    ctx = (pr @ v).permute(0, 2, 1, 3).reshape(2, T, D)
    (ctx * g).sum().backward()                                   # g: the class logit's gradient at ctx
    A = (pr * pr.grad).clamp(min=0).mean(dim=1)
    want = rho + (rho.unsqueeze(1) @ A).squeeze(1)
    lse = vo.attention(qkv, heads)[1]
    got = ro.step(qkv, lse, g * seed.reshape(2, 1, 1), rho, seed, heads)          # the loop's g_ctx = seed x that gradient
    assert float((got - want).detach().abs().max()) <= 1e-12
    # a sample without a seed keeps its rho, whatever g_ctx holds
    none = ro.step(qkv, lse, g, rho, torch.tensor([0.0, 0.25], dtype=torch.float64), heads)
    assert torch.equal(none[0], rho[0]) and not torch.equal(none[1], rho[1])
    gl = torch.tensor([[0.0, -0.5, 0.0], [0.25, 0.0, 0.0]], dtype=torch.float64)
    assert ro.seeds(gl, torch.tensor([1, 0], dtype=torch.int32)).tolist() == [-0.5, 0.25]
    assert ro.seeds(gl, torch.tensor([-1, 3], dtype=torch.int32)).tolist() == [0.0, 0.0]
    c, cmax = ro.class_map(torch.tensor([[1.0, -2.0, 0.5], [1.0, 0.25, 3.0]], dtype=torch.float64), torch.tensor([1.0, 0.0]))
    assert c.tolist() == [[0.0, 0.5], [0.0, 0.0]] and cmax.tolist() == [0.5, 0.0]
    assert ro.normalised(c).tolist() == [[0.0, 1.0], [1.0, 1.0]]


STEP_LEVEL = [m for m, fns in ro.MUTATIONS.items() if ro.step in fns]
NETWORK_LEVEL = [m for m, fns in ro.MUTATIONS.items() if ro.network_map in fns]


def test_step_level_mutations_land_beyond_the_bar():
    """On the inputs of tests/test_vit_relevance_ops_gpu.py (vit_oracle.ATT_CASES x the seed variants) a step that makes the mistake is
    beyond the step's bar -- at some case: (1, 1, 1, 4) has one head and one token, where most of them cannot show."""
    worst = {m: 0.0 for m in STEP_LEVEL}
    for case in vo.ATT_CASES:
        for variant in ro.VARIANTS:
            qkv, lse, g, rho, gl, tg = (t.double() if t.is_floating_point() else t for t in ro.step_inputs(case, variant))
            seed = ro.seeds(gl, tg)
            bar = ro.bar_step(qkv, lse, g, rho, seed, case[1], 2 * vo.U)       # (a generous library term: the mutations are far beyond it)
            ref = ro.step(qkv, lse, g, rho, seed, case[1])
            assert torch.isfinite(ref).all() and torch.isfinite(bar).all()
            for m in STEP_LEVEL:
                worst[m] = max(worst[m], float(((ro.step(qkv, lse, g, rho, seed, case[1], m) - ref).abs() / bar.clamp_min(1e-300)).max()))
    print('step-level mutations, largest error / bar:', {k: f'{v:.3g}' for k, v in worst.items()})
    assert set(worst) == set(ro.MUTATIONS) - {'layers_in_forward_order', 'class_token_column_kept'}
    assert all(v > 10 for v in worst.values()), worst


@pytest.mark.parametrize('bug', NETWORK_LEVEL)
def test_network_level_mutations_land_beyond_the_bar(bug):
    """On the fixtures of tests/test_vit_relevance_gpu.py a rollout that makes the mistake misses the map's bar (1e-4 on M in [0, 1]).
    Four mistakes are asserted on 'wide' and 'tall' (depth 2 and 3) only.  'real' has one layer: it cannot see the order of the
    layers at all; and with rho = e_cls its patch columns are row 0 of A itself, so that the head sum for the mean (a factor of 12)
    and the missing identity (which changes the class token's column only) leave M = c / max c exactly as it is -- those two are
    step-level mistakes, which the step's own bar catches at every depth (test_step_level_mutations_land_beyond_the_bar).  The
    side A is multiplied from is asserted with them.  Every other mistake must show on all three."""
    deep = ('wide', 'tall')
    errs = {}
    for geom in vo.GEOMS:
        sd = vo.to64(vo.state_dict(geom))
        ref = ro.network_map(sd, pre64(geom), TARGETS)[0]
        errs[geom] = float((ro.network_map(sd, pre64(geom), TARGETS, bug)[0] - ref).abs().max())
    print(f'{bug}: largest |M - M_ref| per fixture {errs} (bar {MAP_BAR})')
    if bug in ('layers_in_forward_order', 'A_rho_for_rho_A', 'head_sum', 'no_identity'):
        assert all(errs[g] > 10 * MAP_BAR for g in deep)
    else:
        assert all(e > 10 * MAP_BAR for e in errs.values())


@pytest.mark.parametrize('geom', list(vo.GEOMS))
def test_fp32_evaluation_is_well_inside_the_bar(geom):
    """torch's own fp32 evaluation of the restatement against float64: a hundredth of the bar, so the bar can hold."""
    sd32 = vo.state_dict(geom)
    ref = ro.network_map(vo.to64(sd32), pre64(geom), TARGETS)[0]
    err = float((ro.network_map(sd32, pre64(geom).float(), TARGETS)[0].double() - ref).abs().max())
    print(f'{geom}: torch fp32 against float64, |M - M_ref| {err:.2e}')
    assert err < MAP_BAR / 10


def test_attention_rollout_is_a_checked_field():
    a = Attention(0.25, rollout=True)
    assert a.rollout is True and a.floor == 0.25 and Attention(0.25).rollout is False and Attention() == Attention(0.0, False)
    assert a != Attention(0.25) and hash(a) == hash(Attention(0.25, True))
    for bad in (1, 0, None, 'yes', 1.0):
        with pytest.raises(ValueError, match='rollout must be a bool'):
            Attention(0.25, rollout=bad)
    with pytest.raises(ValueError, match='floor'):
        Attention(1.5, rollout=True)


def test_attention_supported_lets_a_vit_through_with_rollout_only():
    from spaa_amd import projector_based_attack as A
    geom = 'wide'
    vit = Classifier('vit_b_16', 'cpu', state_dict=vo.state_dict(geom), input_sz=vo.GEOMS[geom][2])
    r18 = Classifier('resnet18', 'cpu', state_dict=syn.resnet18_state_dict(num_classes=vo.NUM_CLASSES))
    assert vit.has_rollout and not vit.has_feature_map and r18.has_feature_map and not r18.has_rollout
    for c in (vit, [r18, vit], [vit, r18]):
        with pytest.raises(NotImplementedError, match='vit_b_16'):
            A._attention_supported(Attention(0.25), c, 'f32', None, 'spaa')
        A._attention_supported(Attention(0.25, rollout=True), c, 'f32', None, 'spaa')
    A._attention_supported(Attention(0.25, rollout=True), [r18, r18], 'f32', None, 'spaa')     # (convolutional bodies: Grad-CAM either way)
    with pytest.raises(NotImplementedError, match='capture jitter'):
        A._attention_supported(Attention(0.25, rollout=True), vit, 'f32', A.CaptureJitter(draws=2, seed=1), 'spaa')
    with pytest.raises(NotImplementedError, match="storage='f16'"):
        A._attention_supported(Attention(0.25, rollout=True), vit, 'f16', None, 'spaa')
    with pytest.raises(NotImplementedError, match="storage='f16'"):
        A._attention_checked(Attention(0.25, rollout=True), 'f16', 'AttackState')
    with pytest.raises(NotImplementedError, match='no convolutional feature map'):
        vit.grad_cam(torch.rand(1, 3, 40, 56), [0], (36, 52))
    with pytest.raises(RuntimeError, match='GPU only'):
        vit.relevance(torch.rand(1, 3, 40, 56), [0], (36, 52))
