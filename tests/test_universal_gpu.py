"""GPU: the universal attack loop (UniversalAttackState through spaa) on a 64 x 64 synthetic PCNet with one scene per sample: one
teacher-forced first iteration against the float64 oracle (tests/universal_oracle.py), a group of two against the multi-view attack
on two equal PCNets, groups of equal members against the plain AttackState, twelve iterations whose group rows must stay bitwise equal
and whose group words must be the stated functions of the member tables, the graph route, one call each with transfer and attention,
and universal_success on scenes held out from the attack."""
import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import spaa_oracle as so
import universal_oracle as uo
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
SETUP = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ)
LOSS = 'camdE_caml2'
INPUT_SZ = (56, 56)
AFFINE = (0.9, 0.02, 0.05, -0.03, 0.9, 0.05)
SCENE_SEEDS = [1, 2, 3, 4, 5, 6]      # the six scenes of the attack; 7 and 8 are held out
# every scene shows the classifier the same class, at the grey image with confidences 0.982, 0.996, 0.9998, ...: a threshold of 0.99
# lies between the members of the first group (margins 0.008 and 0.006), so they disagree from the start
P_THRESH = 0.99
P_HIGH = 0.9975                       # between the second and the third member: one of three fooled, not enough for a rate of 0.5
UNTARGETED_OTHER = 7                  # an untargeted group on a class that no scene shows: every member fooled from the start
TARGETED = [True] * 3 + [False] * 3
D_THR = [5.0] * 6

_CACHE = {}


def _csd():
    if 'csd' not in _CACHE:
        _CACHE['csd'] = syn.resnet18_state_dict(2, logit_gain=20.0)
    return _CACHE['csd']


def _sd():
    return syn.pcnet_state_dict(0, cam_sz=SZ, mask='rect', affine=AFFINE)


def scenes_of(seeds):
    return torch.cat([syn.scenes(s, 1, SZ) for s in seeds])


def oracle_case():
    """CPU side: the oracle's classifier, the six scenes and the B = 6 targets: group 0 targeted on the class the scenes show (a
    success for every member, confident above P_THRESH for some only), group 1 untargeted on UNTARGETED_OTHER (every member fooled)."""
    oc = so.OracleClassifier('resnet18', _csd(), input_sz=INPUT_SZ)
    scenes = scenes_of(SCENE_SEEDS)
    true_idx = int(oc(scenes[:1], SETUP['classifier_crop_sz'])[0][0].argmax())
    return oc, scenes, [true_idx] * 3 + [UNTARGETED_OTHER] * 3


def oracle_first_iteration():
    """The float64 first iteration of the case (focus does not enter it but through the weights), computed once and shared (read only)."""
    if 'ref' not in _CACHE:
        oc, scenes, targets = oracle_case()
        _CACHE['ref'] = uo.first_iteration(_sd(), oc, targets, TARGETED, scenes, D_THR, LOSS, SETUP, 3, 3, p_thresh=P_THRESH)
    return _CACHE['ref']


@pytest.fixture(scope='module')
def clf(hip):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=_csd(), input_sz=INPUT_SZ)


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, _sd(), SZ)


def _flat(t, B):
    return t.reshape(B, -1, 4).cpu().numpy().astype(np.float64)


def _rows_equal(t, N):
    g = t.reshape(t.shape[0] // N, N, -1)
    return torch.equal(g, g[:, :1].expand_as(g))


def test_first_iteration_against_the_oracle(hip, pcnet, clf):
    A = hip['attack']
    B, N = 6, 3
    _, scenes, targets = oracle_case()
    ref = oracle_first_iteration()
    clear = (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)              # [B], the rule of test_ensemble_gpu.clear_pairs
    clear_d = ref['d_margin'] > 1e-3
    print(f'oracle: top-2 gaps {ref["gap"].tolist()}, |p1 - p_thresh| {ref["p_margin"].tolist()}, |caml2 255 - d_thr| '
          f'{ref["d_margin"].tolist()}, fooled {ref["fooled"].astype(int).tolist()}, best_adv {ref["best_adv"].tolist()}')
    assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other seeds'
    assert ((ref['nfooled'] > 0) & (ref['nfooled'] < N)).any()          # the members disagree somewhere: the tables are not trivial
    assert ref['best_adv'].any() and not ref['best_adv'].all()          # both steps are taken
    row = np.repeat(clear.reshape(B // N, N).all(axis=1), N) & clear_d

    for focus in (False, True):
        st = A.UniversalAttackState(pcnet, clf, targets, scenes, [LOSS] * B, SETUP, DEV, A.Universal(N), focus=focus)
        assert (st.N, st.need, st.B) == (N, N, B) and len(st.clfs) == 1 and st.ss_tiles == 0
        st.forward_decide(TARGETED, D_THR, P_THRESH)
        st.backward_step(2, 1)
        us, uf, uw = st.uni_state.cpu().numpy(), st.uni_stats.cpu().numpy().astype(np.float64), st.uni_w.cpu().numpy()
        state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy().astype(np.float64)
        # member rows and group flags: the oracle's wherever its margins are clear
        assert (us[clear] == ref['uni_state'][clear]).all(), (us, ref['uni_state'])
        assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
        assert (state[row, 1] == ref['best_adv'][row]).all() and (state[row, 2] == ref['best'][row]).all()
        w_ref = np.where(focus & ref['fooled'] & ~ref['group_fooled'], 0.0, 1.0)
        assert (uw[row] == w_ref[row]).all() and (focus and (uw == 0).any() or not focus and (uw == 1).all())
        assert np.allclose(uf[:, 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(uf[:, 1], ref['tl'], rtol=1e-3, atol=1e-3)
        assert np.allclose(uf[:, 2], ref['uni_stats'][:, 2], rtol=1e-4) and np.allclose(uf[:, 3], ref['uni_stats'][:, 3], rtol=1e-4)
        assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], ref['camdE'], rtol=1e-4)
        assert np.allclose(stats[:, 3], ref['col'], rtol=1e-4)
        assert _rows_equal(st.state, N) and _rows_equal(st.stats[:, :7], N) and _rows_equal(st.x, N) and _rows_equal(st.g, N)
        # wiring: the state's g is the combination of the engine's OWN per-sample input gradients with the weights and flags it wrote
        col_step = state[:, 1] != 0
        g_own = _flat(st.eng.g['x'], B)
        g = _flat(st.g, B)
        own, mag = uo.combine_universal(g_own, uw, col_step, N)
        err = np.abs(g - own)[..., :3]
        worst = (err / np.where(mag > 0, mag, 1.0)).reshape(B, -1).max(axis=1)
        print(f'focus {focus}: g against the float64 combination of the engine\'s own gradients, relative to the terms, per sample '
              f'{worst.tolist()}, bar {uo.combine_bar(N, st.HWp):.2e}')
        assert (err <= uo.combine_bar(N, st.HWp) * mag).all() and (g[..., 3] == 0).all()
        # against the oracle's direction: nothing beyond the members' own errors and the new kernel's rounding.  Adversarial groups:
        # the members' unit-vector errors, weighted; colour groups (an unnormalised mean): the members' errors over N, relative to
        # the oracle's norm
        ref_out, _ = uo.combine_universal(ref['g'], uw, col_step, N)
        norm = np.sqrt((ref_out ** 2).sum(axis=(1, 2)))
        l2 = np.sqrt(((g - ref_out) ** 2).sum(axis=(1, 2)))
        e_unit = np.sqrt(((eo.unit_images(g_own)[0] - eo.unit_images(ref['g'])[0]) ** 2).sum(axis=(1, 2)))      # [B]
        e_abs = np.sqrt(((g_own[..., :3] - ref['g']) ** 2).sum(axis=(1, 2)))
        group_sum = lambda a: np.repeat(a.reshape(B // N, N).sum(axis=1), N)   # noqa: E731
        rel = np.where(col_step, l2 / norm, l2)
        bound = np.where(col_step, group_sum(e_abs) / N / norm, group_sum(uw * e_unit)) + 2e-6 * N
        print(f'focus {focus}: member errors (unit) {e_unit.tolist()}, combined error {rel.tolist()}, bound {bound.tolist()}')
        assert (rel[row] <= bound[row]).all() and row.sum() >= 3
        del st


@pytest.mark.parametrize('targeted', [True, False])
def test_a_group_of_two_is_the_two_view_attack(hip, clf, targeted):
    """Universal(2) at B = 2 with the scenes (s0, s1) on one PCNet against MultiViewAttackState at B = 1 on two PCNet objects of equal
    weights with the scenes [s0, s1], one iteration from the grey image: equal flags and member tables (the integers exactly; the
    floats to 1e-4, the engines run at different batch sizes), x within 1e-5 at adv_lr = 2 (twice the 2e-6 combination bound times
    the step, as test_two_equal_views_are_the_single_view_attack derives).  Targeted: the members disagree, the adversarial step;
    untargeted on a class nobody shows: the colour step."""
    A = hip['attack']
    oc, scenes, targets = oracle_case()
    target = targets[0] if targeted else UNTARGETED_OTHER
    pc_u, pc_a, pc_b = (make_pcnet(hip, _sd(), SZ) for _ in range(3))
    uni = A.UniversalAttackState(pc_u, clf, [target, target], scenes[:2], LOSS, SETUP, DEV, A.Universal(2))
    two = A.MultiViewAttackState([pc_a, pc_b], clf, [target], [scenes[0:1], scenes[1:2]], LOSS, SETUP, DEV)
    for st in (uni, two):
        st.forward_decide(targeted, 5.0, P_THRESH)
        st.backward_step(2, 1)
    assert torch.equal(uni.state[0], two.state[0]) and torch.equal(uni.state[1], two.state[0])
    assert torch.equal(uni.uni_state, two.view_state[0]) and torch.equal(uni.uni_w, two.view_w[0])
    d_tab = ((uni.uni_stats - two.view_stats[0]).abs() / two.view_stats[0].abs().clamp_min(1e-3)).max().item()
    d_stats = ((uni.stats[0, :7] - two.stats[0, :7]).abs() / two.stats[0, :7].abs().clamp_min(1e-3)).max().item()
    dx = (uni.x - two.x).abs().amax(dim=(1, 2, 3))
    print(f'targeted {targeted}: state {uni.state[0].tolist()}, member table rel diff {d_tab:.2e}, stats rel diff {d_stats:.2e}, '
          f'max |x - x_views| per row {dx.tolist()}')
    assert d_tab <= 1e-4 and d_stats <= 1e-4
    assert int(uni.state[0, 1]) == (0 if targeted else 1) and (not targeted or int(uni.state[0, 3]) == 1)
    assert (dx <= 1e-5).all() and (uni.x[..., :3] != 0.5).any() and torch.equal(uni.x[0], uni.x[1])


def test_equal_members_are_the_plain_attack(hip, pcnet, clf):
    """Groups of two equal scenes and targets against the plain AttackState on the same batch, one iteration from the grey image: the
    same flags, x within 1e-5 at adv_lr = 2, and on the colour step ((g + g) / 2 is g) bitwise."""
    A = hip['attack']
    B = 4
    _, scenes, targets = oracle_case()
    sc = scenes[[0, 0, 3, 3]]
    tg, targeted, d_thr = [targets[0], targets[0], UNTARGETED_OTHER, UNTARGETED_OTHER], [True, True, False, False], [5.0] * B
    one = A.AttackState(pcnet, clf, tg, sc, [LOSS] * B, SETUP, DEV)
    uni = A.UniversalAttackState(pcnet, clf, tg, sc, [LOSS] * B, SETUP, DEV, A.Universal(2))
    assert uni.eng is not one.eng and uni.clf is not one.clf
    for st in (one, uni):
        st.forward_decide(targeted, d_thr, P_THRESH)
        st.backward_step(2, 1)
    assert torch.equal(uni.state[:, 0:3], one.state[:, 0:3])
    assert torch.equal(uni.state[:, 3], 2 * (uni.uni_state[:, 0] >> 1))              # (fooled members: both or none)
    assert torch.equal(uni.stats[:, 1:6], one.stats[:, 1:6]) and torch.equal(uni.uni_state[:, 1], one.state[:, 3])
    assert torch.equal(uni.uni_stats[:, 0], one.stats[:, 0]) and torch.equal(uni.uni_stats[:, 2], one.stats[:, 1])
    col = one.state[:, 1] != 0
    assert col.tolist() == [False, False, True, True]
    dx = (uni.x - one.x).abs().amax(dim=(1, 2, 3))
    print(f'equal members against the plain attack: max |x - x_plain| per sample {dx.tolist()}')
    assert (dx <= 1e-5).all() and (one.x[..., :3] != 0.5).any()
    assert torch.equal(uni.g[col], one.eng.g['x'][col])
    assert torch.equal(uni.x[col], one.x[col])                            # (the same g, the same norm, the same step)
    cam_u, prj_u = uni.results()
    cam_1, prj_1 = one.results()
    assert cam_u.shape == cam_1.shape == (B, 3, *SZ) and prj_u.shape == (B, 3, *SZ)
    assert torch.equal(cam_u, cam_1) and (prj_u - prj_1).abs().max() <= 1e-5


@pytest.mark.parametrize('focus', [False, True])
def test_twelve_iterations_keep_the_rows_of_a_group_equal(hip, pcnet, clf, focus):
    """At every iteration the rows of a group hold the same x, x_best and state, bit for bit, the group words are the stated
    functions of the member table, and the trace entry has four tensors.  Without focus every member must be fooled; with focus a
    group is fooled by two of its three (rate 0.5), and the threshold P_HIGH lets one be fooled at the start."""
    A = hip['attack']
    B, N = 6, 3
    _, scenes, targets = oracle_case()
    universal, p_thresh = (A.Universal(N, 0.5), P_HIGH) if focus else (A.Universal(N), P_THRESH)
    need = universal.need
    assert need == (2 if focus else 3)
    st = A.UniversalAttackState(pcnet, clf, targets, scenes, LOSS, SETUP, DEV, universal, focus=focus)
    targeted = torch.tensor(TARGETED)
    tgt = torch.tensor(targets)
    best_before = torch.full((B,), 1e6)
    group = lambda t: t.reshape(B // N, N)   # noqa: E731
    rows = lambda t: t.repeat_interleave(N)   # noqa: E731
    seen_col_step = seen_adv_step = False
    for i in range(12):
        st.iteration(TARGETED, D_THR, 2, 1, p_thresh)
        assert _rows_equal(st.x, N) and _rows_equal(st.x_best, N) and _rows_equal(st.state, N) and _rows_equal(st.stats[:, :7], N), i
        entry = st.trace_entry()
        assert len(entry) == 4
        state, stats, us, uf = (t.cpu() for t in entry)
        assert state.shape == (B, 4) and stats.shape == (B, 8) and us.shape == (B, 2) and uf.shape == (B, 4)
        succ, fooled = (us[:, 0] & 1).bool(), (us[:, 0] & 2).bool()
        assert ((us[:, 0] & ~3) == 0).all() and (us[:, 1] >= 0).all() and (us[:, 1] < 1000).all()
        assert torch.equal(succ, torch.where(targeted, us[:, 1] == tgt, us[:, 1] != tgt)), i
        assert torch.equal(fooled, torch.where(targeted, succ & (uf[:, 0] > p_thresh), succ)), i
        # the group's caml2 / camdE: the members' means summed in index order and divided by N, in fp32 as the kernel (exactly)
        c, d = group(uf[:, 2]), group(uf[:, 3])
        caml2, camdE = rows(((c[:, 0] + c[:, 1]) + c[:, 2]) / N), rows(((d[:, 0] + d[:, 1]) + d[:, 2]) / N)
        assert torch.equal(stats[:, 1], caml2) and torch.equal(stats[:, 2], camdE), i
        assert torch.equal(stats[:, 3], caml2 + camdE) and (stats[:, 4] == 0).all(), i     # (both weights 1, no prjl2)
        nsucc, nfooled = rows(group(succ).sum(dim=1)), rows(group(fooled).sum(dim=1))
        best_adv = (nfooled >= need) & (stats[:, 1] * 255.0 > torch.tensor(D_THR))
        assert torch.equal(state[:, 0].bool(), nsucc >= need) and torch.equal(state[:, 1].bool(), best_adv), i
        assert torch.equal(state[:, 3], nfooled.int()) and torch.equal(stats[:, 0], rows(group(uf[:, 0]).min(dim=1).values)), i
        best = best_adv & (stats[:, 3] < best_before)
        assert torch.equal(state[:, 2].bool(), best), i
        assert torch.equal(stats[:, 5], torch.where(best, stats[:, 3], best_before)), i
        best_before = stats[:, 5].clone()
        want_w = torch.where(fooled & ~(nfooled >= need), 0.0, 1.0) if focus else torch.ones(B)
        assert torch.equal(st.uni_w.cpu(), want_w), i
        seen_col_step |= bool(best_adv.any())
        seen_adv_step |= bool((~best_adv).any())
    assert seen_col_step and seen_adv_step                              # both steps were taken in this run
    cam, prj = st.results()
    assert cam.shape == prj.shape == (B, 3, *SZ) and torch.isfinite(cam).all() and torch.isfinite(prj).all()
    assert prj.min() >= 0 and prj.max() <= 1 and _rows_equal(prj, N) and not _rows_equal(cam, N)


def test_the_graph_route_is_the_eager_loop(hip, pcnet, clf, monkeypatch):
    """spaa(..., universal=) replays a captured graph at this size; eager, graph and repeated runs are bitwise equal, and a traced run
    records four tensors per iteration."""
    A = hip['attack']
    N = 3
    _, scenes, targets = oracle_case()
    kw = dict(iters=8, focus=True, p_thresh=P_HIGH, universal=A.Universal(N, 0.5))
    args = (pcnet, clf, None, targets, TARGETED, scenes, 5, LOSS, DEV, SETUP)
    cam_g, prj_g = A.spaa(*args, **kw)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    assert cam_g.shape == prj_g.shape == (6, 3, *SZ) and _rows_equal(prj_g, N)
    cam_2, prj_2 = A.spaa(*args, **kw)
    assert A.LAST_RUN == dict(iterations=8, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    cam_e, prj_e = A.spaa(*args, **kw)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    monkeypatch.undo()
    assert not torch.equal(prj_g, torch.full_like(prj_g, 0.5))          # (a group succeeded: the images are not the grey start)
    tr = []
    cam_t, prj_t = A.spaa(*args, trace=tr, **kw)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and len(tr) == 8 and all(len(e) == 4 for e in tr)
    assert torch.equal(cam_t, cam_g) and torch.equal(prj_t, prj_g)


def test_transfer_and_attention_keep_the_rows_equal(hip, pcnet, clf):
    """One run each with transfer=Transfer(1, 1.5) and attention=Attention(0.25): the rows of a group stay equal, the momentum rows
    too, and every sample has its own attention map."""
    A = hip['attack']
    B, N = 6, 3
    _, scenes, targets = oracle_case()
    st = A.UniversalAttackState(pcnet, clf, targets, scenes, LOSS, SETUP, DEV, A.Universal(N), transfer=A.Transfer(1, 1.5))
    for _ in range(4):
        st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    assert _rows_equal(st.x, N) and _rows_equal(st.x_best, N) and _rows_equal(st.momentum, N) and _rows_equal(st.state, N)
    assert (st.momentum[:N] != 0).any() and torch.isfinite(st.x).all()    # (group 0 took adversarial steps)
    del st
    st = A.UniversalAttackState(pcnet, clf, targets, scenes, LOSS, SETUP, DEV, A.Universal(N), attention=A.Attention(0.25))
    for _ in range(4):
        st.iteration(TARGETED, D_THR, 2, 1, P_THRESH)
    assert _rows_equal(st.x, N) and _rows_equal(st.x_best, N) and _rows_equal(st.state, N) and torch.isfinite(st.x).all()
    maps = st.attention_maps()
    assert isinstance(maps, torch.Tensor) and maps.shape == (B, 1, *SZ) and not _rows_equal(maps, N)
    del st
    cam, prj = A.spaa(pcnet, clf, None, targets, TARGETED, scenes, 5, LOSS + '_camssim', DEV, SETUP, iters=4, p_thresh=P_THRESH,
                      universal=A.Universal(N), transfer=A.Transfer(1, 1.5), attention=A.Attention(0.25))
    assert _rows_equal(prj, N) and torch.isfinite(cam).all() and torch.isfinite(prj).all()


def test_universal_success_on_held_out_scenes(hip, pcnet, clf):
    """The evaluation hook: one projector image, or one per scene, projected onto two scenes held out from the attack.  (The weights
    are random: the fooling rate itself says only that the path runs.)"""
    A = hip['attack']
    _, scenes, targets = oracle_case()
    _, prj = A.spaa(pcnet, clf, None, targets[3:], False, scenes[3:], 5, LOSS, DEV, SETUP, iters=6, universal=A.Universal(3))
    held_out = scenes_of([7, 8])
    tg = [UNTARGETED_OTHER, targets[0]]
    ok, cam = A.universal_success(pcnet, clf, prj[0], held_out, tg, False, SETUP['classifier_crop_sz'])
    assert ok.shape == (2,) and ok.dtype == bool and cam.shape == (2, 3, *SZ) and cam.is_cuda and torch.isfinite(cam).all()
    assert np.array_equal(ok, A.transfer_success(cam, clf, tg, False, SETUP['classifier_crop_sz']))
    assert ok[0]                                                        # (untargeted on a class nobody shows)
    with torch.no_grad():
        assert torch.equal(cam, pcnet(prj[:1].expand(2, -1, -1, -1).contiguous(), held_out.to(DEV)))
    ok_t, cam_t = A.universal_success(pcnet, clf, prj[:2], held_out, tg, [False, True], SETUP['classifier_crop_sz'], p_thresh=0.5)
    assert torch.equal(cam_t, cam) and np.array_equal(ok_t, A.transfer_success(cam, clf, tg, [False, True], SETUP['classifier_crop_sz'], 0.5))
    with pytest.raises(ValueError, match='3 projector images for 2 scenes'):
        A.universal_success(pcnet, clf, prj, held_out, tg, False, SETUP['classifier_crop_sz'])
