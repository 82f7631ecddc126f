"""CPU: the universal attack's host side -- the two entry points are declared and exported, the Universal option checks itself, every
refusal of spaa() and spaa_sweep() is raised before anything touches a GPU and after every refusal there was before, the float64
restatement (tests/universal_oracle.py) with rate = 1 is the multi-view restatement with members in the place of views, and on the
engineered cases of tests/universal_cases.py -- which hold the mix of groups they are meant to hold -- every deliberate mistake of the
restatement is seen."""
import os
import re

import numpy as np
import pytest
import torch

import multiview_oracle as mo
import universal_cases as uc
import universal_oracle as uo
from spaa_amd import _lib, synthetic as syn
from spaa_amd import attack_options as O
from spaa_amd import projector_based_attack as A
from spaa_amd.attack_options import UNIVERSAL_MAX, Universal   # (the feature itself: without it nothing here has a subject)
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('spaa_decide_universal', 'spaa_universal_combine')


def test_entry_points_are_declared_and_exported():
    import spaa_amd
    hdr = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), f'{name} is not declared in include/spaa_hip.h'
        assert hasattr(lib, name), f'{name} is not exported by libspaa_hip.so'
        assert name in _lib.EXPORTS and name in _lib._SIGNATURES
    assert re.search(r'#define\s+SPAA_UNIVERSAL_MAX\s+64\b', hdr) and A.UNIVERSAL_MAX == O.UNIVERSAL_MAX == UNIVERSAL_MAX == 64
    assert 'universal_ops.hip' in open(os.path.join(ROOT, 'spaa_amd', 'csrc', 'Makefile')).read()
    assert spaa_amd.UniversalAttackState is A.UniversalAttackState and issubclass(A.UniversalAttackState, A.AttackState)
    assert spaa_amd.Universal is A.Universal is O.Universal is Universal and spaa_amd.universal_success is A.universal_success
    assert A.UniversalAttackState.label == 'members'


def test_universal_validation():
    u = A.Universal(3)
    assert (u.size, u.rate, u.need) == (3, 1.0, 3) and A.Universal(64).need == 64
    with pytest.raises(Exception):           # frozen
        u.size = 4
    assert [A.Universal(n, r).need for n, r in ((2, 0.5), (3, 0.5), (10, 0.3), (64, 0.01), (5, 0.8), (5, 0.81), (7, 1))] == [1, 2, 3, 1, 4, 5, 7]
    assert all(A.Universal(n, r).need == uo.need_of(n, r) for n in (2, 3, 10, 64) for r in (0.1, 0.25, 0.5, 0.7, 1.0))
    for size in (1, 0, -2, 65, 2.0, '2', True, None):
        with pytest.raises(ValueError, match='size'):
            A.Universal(size)
    for rate in (0, 0.0, -0.5, 1.01, float('nan'), float('inf'), '1', None, True):
        with pytest.raises(ValueError, match='rate'):
            A.Universal(2, rate)
    assert u.groups(6) == 2 and A.Universal(64).groups(64) == 1
    for B in (2, 4, 7):
        with pytest.raises(ValueError, match='groups of universal.size = 3'):
            u.groups(B)
    u.check_uniform('d_thr', [5, 5, 5, 9, 9, 9])
    with pytest.raises(ValueError, match=r'd_thr must be uniform within a universal group; group 1 \(samples 3\.\.5\)'):
        u.check_uniform('d_thr', [5, 5, 5, 9, 5, 9])


def _pcnet(sz):
    sd = syn.pcnet_state_dict(0, cam_sz=sz)
    pc = PCNet(sd['mask'], WarpingNet(out_size=sz))
    pc.load_state_dict(sd)
    return pc


@pytest.fixture(scope='module')
def parts():
    pcs = [_pcnet((64, 64)) for _ in range(2)]
    csd = syn.resnet18_state_dict(2)
    clfs = [Classifier('resnet18', 'cpu', state_dict=csd, input_sz=(56, 56)) for _ in range(2)]
    setup = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=(64, 64))
    return pcs, clfs, setup


def test_universal_refusals(parts):
    """Every refusal that needs no device, from spaa() with device='cuda' and no GPU in reach: nothing was allocated or launched."""
    pcs, clfs, setup = parts
    sc = syn.scenes(1, 4, (64, 64))
    uni = A.Universal(2)

    def run(pcnet=pcs[0], classifier=clfs[0], cam_scene=sc, targets=(1, 2, 3, 4), targeted=True, d_thr=5, loss='caml2', device='cuda',
            universal=uni, **kw):
        return A.spaa(pcnet, classifier, None, list(targets), targeted, cam_scene, d_thr, loss, device, setup, universal=universal, **kw)

    with pytest.raises(NotImplementedError, match='spaa: a universal projection against several views'):
        run(pcnet=[pcs[0], pcs[1]], cam_scene=[sc, sc])
    with pytest.raises(NotImplementedError, match='spaa: a universal projection against an ensemble'):
        run(classifier=[clfs[0], clfs[1]])
    for name, value in (('jitter', A.CaptureJitter(draws=2)), ('pose', A.PoseJitter(draws=2)), ('jpeg', A.JpegCapture(draws=2))):
        with pytest.raises(NotImplementedError, match=f'spaa: universal together with {name} is not implemented'):
            run(**{name: value})
    with pytest.raises(TypeError, match='spaa: a universal attack needs a spaa_amd.Classifier, got function'):
        run(classifier=lambda im, cp: None)
    with pytest.raises(NotImplementedError, match="spaa: storage='f16' is not implemented for a universal projection"):
        run(storage='f16')
    with pytest.raises(TypeError, match='spaa: universal must be a spaa_amd.Universal or None, got int'):
        run(universal=2)
    # the groups: the batch, and what must be uniform within a group (the error names the group)
    with pytest.raises(ValueError, match='3 samples does not divide into groups of universal.size = 2'):
        run(targets=(1, 2, 3), cam_scene=sc[:3])
    with pytest.raises(ValueError, match=r'targeted must be uniform within a universal group; group 1 \(samples 2\.\.3\)'):
        run(targeted=[True, True, False, True])
    with pytest.raises(ValueError, match=r'd_thr must be uniform within a universal group; group 0 \(samples 0\.\.1\)'):
        run(d_thr=[5, 9, 5, 5])
    with pytest.raises(ValueError, match=r'stealth_loss must be uniform within a universal group; group 1 \(samples 2\.\.3\)'):
        run(loss=['caml2', 'caml2', 'caml2', 'camdE_caml2'])
    # what combines with it passes every check and stops at the device (one scene is broadcast, groups may differ from each other)
    for kw in (dict(), dict(focus=True), dict(attention=A.Attention(0.25)), dict(transfer=A.Transfer(1, 1.5)), dict(loss='camdE_caml2_camssim'),
               dict(cam_scene=sc[0]), dict(targeted=[True, True, False, False], d_thr=[5, 5, 9, 9]),
               dict(loss=['caml2', 'caml2', 'prjl2_caml2', 'prjl2_caml2']), dict(universal=A.Universal(4, 0.5))):
        with pytest.raises(RuntimeError, match='GPU only'):
            run(device='cpu', **kw)
    # without universal, focus=True on one classifier stays what it was: accepted and without effect
    with pytest.raises(RuntimeError, match='GPU only'):
        run(device='cpu', universal=None, focus=True)
    assert all(not p._engines for p in pcs) and all(not c._engines for c in clfs)   # no engine was built on the way
    # the sweep batches the configurations of one scene: it says so, before it looks at anything else
    with pytest.raises(NotImplementedError, match='spaa_sweep: universal= is not implemented'):
        A.spaa_sweep(pcs[0], clfs[0], None, sc[0], setup, 'cuda', [('caml2', 5, True, [1, 2])], universal=uni)
    with pytest.raises(NotImplementedError):
        A.UniversalAttackState([pcs[0], pcs[1]], clfs[0], [1, 2], sc[:2], 'caml2', setup, 'cuda', uni)


def test_universal_none_leaves_the_request_check_unchanged(parts):
    """A handful of existing requests: with universal=None the answer is the one without the keyword, and with a Universal every
    refusal there was before still comes first."""
    pcs, clfs, setup = parts
    sc = torch.zeros(3, 64, 64)

    def answer(*args, **kw):
        try:
            pc, cl, scene = O.checked_request('spaa', *args, **kw)
            return ('ok', type(pc).__name__, type(cl).__name__, type(scene).__name__)
        except Exception as e:   # noqa: BLE001  (the outcome IS the exception)
            return (type(e).__name__, str(e))

    requests = [(pcs[0], clfs[0], sc, 'f32', False, None, None, None, None),
                ([pcs[0]], [clfs[0]], [sc], 'f32', True, None, None, A.Attention(0.25), A.Transfer()),
                ([pcs[0], pcs[1]], clfs[0], [sc, sc], 'f32', True, None, None, None, None),
                ([pcs[0], pcs[1]], [clfs[0], clfs[1]], [sc, sc], 'f32', False, None, None, None, None),
                ([pcs[0], pcs[0]], clfs[0], [sc, sc], 'f32', False, None, None, None, None),
                (pcs[0], [clfs[0], clfs[1]], sc, 'f16', False, None, None, None, None),
                (pcs[0], clfs[0], sc, 'f32', True, A.CaptureJitter(draws=2), None, None, None),
                (pcs[0], clfs[0], sc, 'f32', False, A.CaptureJitter(draws=2), A.PoseJitter(draws=3), None, None),
                (pcs[0], lambda im, cp: None, sc, 'f32', False, None, None, None, A.Transfer()),
                (pcs[0], clfs[0], sc, 'f16', False, None, None, A.Attention(0.25), None),
                (object(), clfs[0], sc, 'f32', False, None, None, None, None)]
    kinds = set()
    for req in requests:
        before = answer(*req)
        assert answer(*req, jpeg=None, universal=None) == before
        with_uni = answer(*req, universal=A.Universal(2))
        if before[0] != 'ok':
            assert with_uni == before, 'an earlier refusal must still come first'
        kinds.add(before[0])
    assert kinds == {'ok', 'TypeError', 'ValueError', 'NotImplementedError'}


def _random_case(N, U, ncls, seed):
    rng = np.random.default_rng(seed)
    B = U * N
    logits = rng.standard_normal((B, ncls)) * 3.0
    target = np.repeat(rng.integers(0, ncls, U), N)      # (the views of a sample share its target: so do the members of a group)
    # group u: its first u % (N + 1) members see the target class, the others do not; odd groups are targeted
    sees = np.concatenate([np.arange(N) < u % (N + 1) for u in range(U)])
    logits[np.arange(B), target] = np.where(sees, 15.0, -15.0)
    targeted = np.repeat(np.arange(U) % 2 == 1, N)
    weights = np.repeat(np.array(uc.LOSS_WEIGHTS)[rng.integers(0, 4, U)], N, axis=0)
    return dict(B=B, logits=logits, target=target, targeted=targeted, caml2=rng.uniform(0.02, 0.04, B), camdE=rng.uniform(1, 5, B),
                weights=weights, d_thr=np.repeat(np.where(np.arange(U) % 3 == 1, 9.0, 5.0), N), prjl2=rng.uniform(0.01, 0.05, B),
                col_best=np.repeat(rng.choice([1e6, 1e-3], U), N))


@pytest.mark.parametrize('N', [2, 3, 4])
@pytest.mark.parametrize('focus', [False, True])
def test_rate_one_is_the_multi_view_restatement(N, focus):
    """decide_universal / combine_universal with need = N against multiview_oracle.decide_views / combine_views on the transposed
    inputs (view v of sample u = member v of group u), exactly."""
    U, ncls, HW = 7, 12, 5
    c = _random_case(N, U, ncls, seed=10 * N + focus)
    p_thresh = 0.5
    tgt_u = c['target'][::N]
    got = uo.decide_universal(c['logits'], c['target'], c['targeted'], c['caml2'], c['camdE'], c['weights'], c['d_thr'], p_thresh, focus, N,
                              N, prjl2=c['prjl2'], col_best=c['col_best'])
    member = lambda a, v: np.asarray(a)[v::N]   # noqa: E731
    want = mo.decide_views([member(c['logits'], v) for v in range(N)], tgt_u, c['targeted'][::N],
                           np.stack([member(c['caml2'], v) for v in range(N)], axis=1),
                           np.stack([member(c['camdE'], v) for v in range(N)], axis=1), c['weights'][::N], c['d_thr'][::N], p_thresh, focus,
                           prjl2=c['prjl2'][::N], col_best=c['col_best'][::N])
    for key, table in (('uni_state', 'view_state'), ('uni_stats', 'view_stats'), ('uni_w', 'view_w')):
        assert np.array_equal(got[key].reshape((U, N) + got[key].shape[1:]), want[table]), key
    for key in ('state_succ', 'best_adv', 'best', 'nfooled', 'p_min', 'tl_mean', 'caml2', 'camdE', 'col', 'prjl2', 'col_best_after'):
        assert np.array_equal(got[key][::N], want[key]), key
        assert np.array_equal(got[key], np.repeat(want[key], N)), key                # (the group's value in each of its rows)
    assert 0 < got['best_adv'].sum() < U * N and ((got['nfooled'] > 0) & (got['nfooled'] < N)).any()
    rng = np.random.default_rng(N)
    g = rng.standard_normal((U * N, HW, 4))
    g[1, :, :3] = 0.0
    w = rng.uniform(0.5, 1.5, U * N)
    col_step = got['best_adv']
    out, mag = uo.combine_universal(g, w, col_step, N)
    ref = mo.combine_views([g[v::N] for v in range(N)], w.reshape(U, N), col_step[::N])
    assert np.array_equal(out[::N], ref) and all(np.array_equal(out[v::N], ref) for v in range(N)) and (out[..., 3] == 0).all()
    assert (mag >= np.abs(out[..., :3]) - 1e-15).all()


def test_the_cases_hold_the_mix_and_are_clear():
    """Over tests/universal_cases.py's decide cases: groups with nobody fooled, some but not enough, enough but not all, and all;
    best_adv both ways; a new best and none; group_succ without group_fooled; resting members; a tie -- and in every case at most one
    sample near a tie or near p_thresh, no group near its d_thr."""
    seen = set()
    for BN, ncls, HW, rate in uc.DECIDE_CASES:
        c = uc.decide_case(BN, ncls, HW, rate)
        N, need = c['N'], c['need']
        assert c['nblk'] == {1: 1, 3120: 13, 65537: 257}[HW] and need == (N if rate == 1.0 else (N + 1) // 2)
        for focus in (False, True):
            ref = uc.decide_reference(c, focus)
            clear = (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)
            assert (~clear).sum() <= 1 and (ref['d_margin'] > 1e-3).all(), 'the case itself is near a tie: choose other inputs'
            assert (c['tie'] is None) == clear.all()
            if c['tie'] is not None:
                b, first = c['tie']
                assert ref['gap'][b] == 0 and ref['top1'][b] == first            # the first maximum wins
            nf = ref['nfooled'][::N]
            seen |= {'none'} if (nf == 0).any() else set()
            seen |= {'not enough'} if ((nf > 0) & (nf < need)).any() else set()
            seen |= {'enough, not all'} if ((nf >= need) & (nf < N)).any() else set()
            seen |= {'all'} if (nf == N).any() else set()
            seen |= {f'best_adv {bool(v)}' for v in ref['best_adv']} | {f'best {bool(v)}' for v in ref['best'][ref['best_adv']]}
            seen |= {'succ, not fooled'} if (ref['state_succ'] & ~ref['group_fooled']).any() else set()
            seen |= {'low pert'} if (ref['group_fooled'] & ~ref['high_pert']).any() else set()
            seen |= {'resting'} if (ref['uni_w'] == 0).any() else set()
            enough = ref['group_fooled'] & (ref['nfooled'] < N)
            seen |= {'fooled group, nobody rests'} if focus and enough.any() and (ref['uni_w'][enough] == 1).all() else set()
            seen |= {'mixed targeted'} if len(set(c['targeted'][::N].tolist())) == 2 else set()
    assert seen == {'none', 'not enough', 'enough, not all', 'all', 'best_adv True', 'best_adv False', 'best True', 'best False',
                    'succ, not fooled', 'low pert', 'resting', 'fooled group, nobody rests', 'mixed targeted'}, seen


DECIDE_MUTATIONS = ('need_is_n', 'mean_over_need', 'prjl2_summed', 'focus_rests_fooled', 'boundary_off_by_one')
COMBINE_MUTATIONS = ('unit_on_colour', 'mean_on_adv', 'boundary_off_by_one', 'order_reversed')


def test_every_mutation_is_named_once():
    assert set(DECIDE_MUTATIONS) | set(COMBINE_MUTATIONS) == set(uo.MUTATIONS) and len(uo.MUTATIONS) == 8


@pytest.mark.parametrize('mutation', DECIDE_MUTATIONS)
def test_decide_mutations_are_seen(mutation):
    """Each mistake changes a flag, a count, a weight or a value beyond the comparison's tolerance in some decide case; the decision
    itself differs from itself nowhere."""
    caught = 0
    for BN, ncls, HW, rate in uc.DECIDE_CASES:
        c = uc.decide_case(BN, ncls, HW, rate)
        for focus in (False, True):
            ref = uc.decide_reference(c, focus)
            assert not uc.decide_differs(ref, uc.decide_reference(c, focus))
            caught += uc.decide_differs(ref, uc.decide_reference(c, focus, mutation))
    assert caught >= 4, f'{mutation}: seen in {caught} cases only'


@pytest.mark.parametrize('mutation', COMBINE_MUTATIONS)
def test_combine_mutations_exceed_the_bar(mutation):
    """Each mistake moves the combination by more than the derived bar, in every combine case."""
    for N in uc.COMBINE_N:
        for HW in uc.COMBINE_HW:
            g, w, state = uc.combine_case(N, HW, seed=10 * HW + N)
            want, mag = uo.combine_universal(g, w, state[:, 1] != 0, N)
            got, _ = uo.combine_universal(g, w, state[:, 1] != 0, N, mutation=mutation)
            bar = uo.combine_bar(N, HW)
            assert 0 < bar < 1e-5
            assert (np.abs(got - want)[..., :3] > bar * mag).any(), (mutation, N, HW)


def test_combine_restatement_by_hand():
    """Two groups of two on four pixels: the unit images with weights, a zero member, the plain mean, the pad channel."""
    g = np.zeros((4, 4, 4))
    g[0, 0, :3] = (3.0, 0.0, 4.0)
    g[1, 1, 1] = 2.0
    g[2, 0, :3] = (3.0, 0.0, 4.0)
    g[3, 1, 1] = -8.0
    g[..., 3] = 7.0                        # (the pad channel is not part of the norm, and not passed on)
    out, mag = uo.combine_universal(g, [1.0, 0.5, 1.0, 1.0], [False, False, True, True], 2)
    assert np.allclose(out[0, 0], (0.6, 0.0, 0.8, 0.0)) and np.allclose(out[0, 1], (0.0, 0.5, 0.0, 0.0)) and np.array_equal(out[0], out[1])
    assert np.allclose(out[2, 0], (1.5, 0.0, 2.0, 0.0)) and np.allclose(out[2, 1], (0.0, -4.0, 0.0, 0.0)) and np.array_equal(out[2], out[3])
    assert np.allclose(mag[0, 0], (0.6, 0.0, 0.8)) and np.allclose(mag[3, 1], (0.0, 4.0, 0.0))
    g[1] = 0.0
    out, _ = uo.combine_universal(g, [1.0, 1.0, 1.0, 1.0], [False, False, False, False], 2)
    assert np.allclose(out[0, 0], (0.6, 0.0, 0.8, 0.0)) and (out[:2, 1:] == 0).all()
    assert uo.combine_bar(2, 256) < uo.combine_bar(64, 256) < uo.combine_bar(64, 256 * 257)
