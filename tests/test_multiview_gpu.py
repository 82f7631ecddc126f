"""GPU: the multi-view attack loop (MultiViewAttackState through spaa / spaa_sweep) on 64 x 64 synthetic PCNets with distinct warps
and scenes: one teacher-forced first iteration against the float64 oracle (tests/multiview_oracle.py), two equal views against the
single-view AttackState, twelve traced iterations whose sample tables must be the stated functions of the view tables, the eager /
graph / repeat identities, the sweep's list forms and the argument errors."""
import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import multiview_oracle as mo
import spaa_oracle as so
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
SETUP = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ)
LOSS = 'camdE_caml2'
P_THRESH = 0.97                    # between the views' confidences at the grey image (0.98, 0.96, 0.99): the views disagree from the start
# view -> (PCNet seed, affine of its warp, scene seed): the same projector seen from four poses
VIEWS = [(0, (0.9, 0.02, 0.05, -0.03, 0.9, 0.05), 1), (3, (0.92, -0.04, -0.03, 0.05, 0.87, -0.04), 2),
         (5, (0.86, 0.05, -0.06, -0.02, 0.93, 0.03), 3), (8, (0.95, -0.02, 0.04, 0.03, 0.84, 0.02), 4)]
INPUT_SZ = (56, 56)
TARGETED = [True, True, False, False]
D_THR = [5.0, 5.0, 9.0, 5.0]
UNTARGETED_OTHER = 7               # an untargeted sample on a class that no view shows: every view fooled from the start

_CACHE = {}


def _csd():
    if 'csd' not in _CACHE:
        _CACHE['csd'] = syn.resnet18_state_dict(2, logit_gain=20.0)
    return _CACHE['csd']


def view_sd(v):
    seed, affine, _ = VIEWS[v]
    return syn.pcnet_state_dict(seed, cam_sz=SZ, mask='rect', affine=affine)


def view_scene(v):
    return syn.scenes(VIEWS[v][2], 1, SZ)


def oracle_case(V):
    """CPU side of a case: the views' PCNet weights and scenes, the oracle's classifier, the B = 4 targets: targeted on class 204 (no view
    shows it) and on the class every view gives its scene (a success in every view, confident above P_THRESH in some views only), then
    untargeted on that class (no view fooled) and on UNTARGETED_OTHER (every view fooled)."""
    oc = so.OracleClassifier('resnet18', _csd(), input_sz=INPUT_SZ)
    scenes = [view_scene(v) for v in range(V)]
    true_idx = int(oc(scenes[0], SETUP['classifier_crop_sz'])[0][0].argmax())
    return [view_sd(v) for v in range(V)], scenes, oc, [204, true_idx, true_idx, UNTARGETED_OTHER]


def oracle_first_iteration(V):
    """The float64 first iteration of the V-view case, computed once and shared (read only)."""
    if ('ref', V) not in _CACHE:
        sds, scenes, oc, targets = oracle_case(V)
        _CACHE['ref', V] = mo.first_iteration(sds, oc, targets, TARGETED, scenes, D_THR, LOSS, SETUP, p_thresh=P_THRESH)
    return _CACHE['ref', V]


@pytest.fixture(scope='module')
def clf(hip):
    return hip['clf'].Classifier('resnet18', DEV, state_dict=_csd(), input_sz=INPUT_SZ)


@pytest.fixture(scope='module')
def pcnets(hip):
    return [make_pcnet(hip, view_sd(v), SZ) for v in range(len(VIEWS))]


def _flat(t, B):
    return t.reshape(B, -1, 4).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('V', [2, 3])
def test_first_iteration_against_the_oracle(hip, pcnets, clf, V):
    A = hip['attack']
    B = 4
    _, scenes, _, targets = oracle_case(V)
    ref = oracle_first_iteration(V)
    clear = (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)              # [B][V], the rule of test_ensemble_gpu.clear_pairs
    clear_d = ref['d_margin'] > 1e-3
    print(f'oracle V = {V}: top-2 gaps {ref["gap"].tolist()}, |p1 - p_thresh| {ref["p_margin"].tolist()}, |caml2 255 - d_thr| '
          f'{ref["d_margin"].tolist()}, fooled {ref["fooled"].astype(int).tolist()}, best_adv {ref["best_adv"].tolist()}')
    assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other seeds'
    assert ((ref['nfooled'] > 0) & (ref['nfooled'] < V)).any()          # the views disagree somewhere: the tables are not trivial
    assert ref['best_adv'].any() and not ref['best_adv'].all()          # both steps are taken
    row = clear.all(axis=1) & clear_d

    for focus in (False, True):
        st = A.MultiViewAttackState(pcnets[:V], clf, targets, scenes, [LOSS] * B, SETUP, DEV, focus=focus)
        assert st.V == V and len({id(e) for e in st.clfs}) == V and len({id(e) for e in st.engs}) == V
        st.forward_decide(TARGETED, D_THR, P_THRESH)
        st.backward_step(2, 1)
        vs, vf, vw = st.view_state.cpu().numpy(), st.view_stats.cpu().numpy().astype(np.float64), st.view_w.cpu().numpy()
        state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy().astype(np.float64)
        # view rows and sample flags: the oracle's wherever its margins are clear
        assert (vs[clear] == ref['view_state'][clear]).all(), (vs, ref['view_state'])
        assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
        assert (state[row, 1] == ref['best_adv'][row]).all() and (state[row, 2] == ref['best'][row]).all()
        w_ref = eo.focus_weights(ref['fooled'], focus)
        assert (vw[row] == w_ref[row]).all()
        assert np.allclose(vf[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(vf[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
        assert np.allclose(vf[..., 2], ref['view_stats'][..., 2], rtol=1e-4) and np.allclose(vf[..., 3], ref['view_stats'][..., 3], rtol=1e-4)
        assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4) and np.allclose(stats[:, 2], ref['camdE'], rtol=1e-4)
        assert np.allclose(stats[:, 3], ref['col'], rtol=1e-4)
        # wiring: the state's g is the combination of the view engines' OWN input gradients with the weights and flags it wrote
        col_step = state[:, 1] != 0
        g_own = [_flat(e.g['x'], B) for e in st.engs]
        g = _flat(st.g, B)
        own = mo.combine_views(g_own, vw, col_step)
        err = np.abs(g - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2))
        print(f'V = {V} focus {focus}: g against the float64 combination of the engines\' own gradients, per sample {err.tolist()}')
        assert (err <= 2e-6).all() and (g[..., 3] == 0).all()
        # against the oracle's direction: nothing beyond the views' own errors and the new kernel's rounding.  Adversarial samples:
        # the views' unit-vector errors, weighted; colour samples (an unnormalised mean): the views' errors over V, relative to
        # the oracle's norm
        ref_out = mo.combine_views(ref['g'], vw, col_step)
        norm = np.sqrt((ref_out ** 2).sum(axis=(1, 2)))
        l2 = np.sqrt(((g - ref_out) ** 2).sum(axis=(1, 2)))
        e_unit = np.stack([np.sqrt(((eo.unit_images(g_own[v])[0] - eo.unit_images(ref['g'][v])[0]) ** 2).sum(axis=(1, 2)))
                           for v in range(V)], axis=1)                                     # [B][V]
        e_abs = np.stack([np.sqrt(((g_own[v][..., :3] - ref['g'][v]) ** 2).sum(axis=(1, 2))) for v in range(V)], axis=1)
        rel = np.where(col_step, l2 / norm, l2)
        bound = np.where(col_step, e_abs.sum(axis=1) / V / norm, (vw * e_unit).sum(axis=1)) + 2e-6 * V
        print(f'V = {V} focus {focus}: view errors (unit) {e_unit.tolist()}, combined error {rel.tolist()}, bound {bound.tolist()}')
        assert (rel[row] <= bound[row]).all() and row.sum() >= 3
        del st


def test_two_equal_views_are_the_single_view_attack(hip, clf):
    """Two distinct PCNet objects with equal weights and scenes against AttackState on one of them, one iteration from the grey
    image: the same flags, x within 1e-5 at adv_lr = 2 (twice the 2e-6 combination bound times the step), and on the colour step
    (g + g) / 2 is g bitwise."""
    A = hip['attack']
    B = 4
    _, scenes, _, targets = oracle_case(1)
    pc_a, pc_b = make_pcnet(hip, view_sd(0), SZ), make_pcnet(hip, view_sd(0), SZ)
    one = A.AttackState(pc_a, clf, targets, scenes[0], [LOSS] * B, SETUP, DEV)
    two = A.MultiViewAttackState([pc_a, pc_b], clf, targets, [scenes[0], scenes[0]], [LOSS] * B, SETUP, DEV)
    assert two.engs[0] is not one.eng and two.engs[0] is not two.engs[1] and two.clfs[0] is not two.clfs[1]
    for st in (one, two):
        st.forward_decide(TARGETED, D_THR, P_THRESH)
        st.backward_step(2, 1)
    assert torch.equal(two.state[:, 0:3], one.state[:, 0:3])
    assert torch.equal(two.state[:, 3], 2 * (two.view_state[:, 0, 0] >> 1))              # (fooled views: both or none)
    assert torch.equal(two.stats[:, 1:6], one.stats[:, 1:6]) and torch.equal(two.view_state[:, 0], two.view_state[:, 1])
    assert torch.equal(two.view_state[:, 0, 1], one.state[:, 3])
    col = one.state[:, 1] != 0
    assert col.any() and not col.all()
    dx = (two.x - one.x).abs().amax(dim=(1, 2, 3))
    print(f'two equal views against one: max |x - x_single| per sample {dx.tolist()}')
    assert (dx <= 1e-5).all() and (one.x[..., :3] != 0.5).any()
    assert torch.equal(two.g[col], one.eng.g['x'][col])
    assert torch.equal(two.x[col], one.x[col])                            # (the same g, the same norm, the same step)
    (cam_a, cam_b), prj = two.results()
    cam_1, prj_1 = one.results()
    assert torch.equal(cam_a, cam_1) and torch.equal(cam_b, cam_1) and (prj - prj_1).abs().max() <= 1e-5


def _sweep_configs(targets):
    return [(LOSS, D_THR[0], True, targets[:2]), (LOSS, D_THR[2], False, targets[2:3]), (LOSS, D_THR[3], False, targets[3:])]


@pytest.mark.parametrize('focus', [False, True])
def test_twelve_traced_iterations(hip, pcnets, clf, focus):
    """In every iteration state and stats are the stated functions of the view tables; col_loss_best never rises; the images stay
    finite and in range."""
    A = hip['attack']
    V = 3
    _, scenes, _, targets = oracle_case(V)
    tr = []
    res = A.spaa_sweep(pcnets[:V], clf, None, scenes, SETUP, DEV, _sweep_configs(targets), iters=12, trace=tr, focus=focus,
                       p_thresh=P_THRESH)
    assert A.LAST_RUN == dict(iterations=12, graph=False)
    assert len(tr) == 1 and len(tr[0]) == 12 and all(len(e) == 4 for e in tr[0])
    targeted = torch.tensor(TARGETED)
    d_thr = torch.tensor(D_THR)
    tgt = torch.tensor(targets)[:, None]
    best_before = torch.full((4,), 1e6)
    seen_col_step = seen_adv_step = False
    for i, entry in enumerate(tr[0]):
        state, stats, vs, vf = (t.cpu() for t in entry)
        assert state.shape == (4, 4) and stats.shape == (4, 8) and vs.shape == (4, V, 2) and vf.shape == (4, V, 4)
        succ, fooled = (vs[..., 0] & 1).bool(), (vs[..., 0] & 2).bool()
        assert ((vs[..., 0] & ~3) == 0).all() and (vs[..., 1] >= 0).all() and (vs[..., 1] < 1000).all()
        assert torch.equal(succ, torch.where(targeted[:, None], vs[..., 1] == tgt, vs[..., 1] != tgt)), i
        assert torch.equal(fooled, torch.where(targeted[:, None], succ & (vf[..., 0] > P_THRESH), succ)), i
        # the sample's caml2 / camdE: the views' means summed in index order and divided by V, in fp32 as the kernel (exactly)
        caml2, camdE = vf[:, 0, 2].clone(), vf[:, 0, 3].clone()
        for v in range(1, V):
            caml2, camdE = caml2 + vf[:, v, 2], camdE + vf[:, v, 3]
        caml2, camdE = caml2 / V, camdE / V
        assert torch.equal(stats[:, 1], caml2) and torch.equal(stats[:, 2], camdE), i
        # col_loss = caml2 + camdE here (both weights 1, no prjl2): one fp32 addition, with or without a fused multiply
        assert torch.equal(stats[:, 3], caml2 + camdE) and (stats[:, 4] == 0).all(), i
        high_pert = stats[:, 1] * 255.0 > d_thr                        # (fp32, as the kernel)
        best_adv = fooled.all(dim=1) & high_pert
        assert torch.equal(state[:, 0].bool(), succ.all(dim=1)) and torch.equal(state[:, 1].bool(), best_adv), i
        assert torch.equal(state[:, 3], fooled.sum(dim=1).int()), i
        assert torch.equal(stats[:, 0], vf[..., 0].min(dim=1).values), i
        tl = vf[..., 1].double()
        assert ((stats[:, 6].double() - tl.mean(dim=1)).abs() <= V * 2.0 ** -24 * tl.abs().sum(dim=1)).all(), i
        best = best_adv & (stats[:, 3] < best_before)
        assert torch.equal(state[:, 2].bool(), best), i
        assert torch.equal(stats[:, 5], torch.where(best, stats[:, 3], best_before)) and (stats[:, 5] <= best_before).all(), i
        best_before = stats[:, 5].clone()
        seen_col_step |= bool(best_adv.any())
        seen_adv_step |= bool((~best_adv).any())
    assert seen_col_step and seen_adv_step                              # both steps were taken in this run
    for (cams, prj), cfg in zip(res, _sweep_configs(targets)):
        assert isinstance(cams, list) and len(cams) == V
        assert all(c.shape == (len(cfg[3]), 3, *SZ) and torch.isfinite(c).all() for c in cams)
        assert prj.shape == (len(cfg[3]), 3, *SZ) and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])


def test_identities(hip, pcnets, clf, monkeypatch):
    """Eager and graph-replayed runs, and two runs, are bitwise equal; a sequence of one PCNet is that PCNet's plain attack; a sweep
    returns per configuration what spaa() returns for it."""
    A = hip['attack']
    V = 2
    _, scenes, _, targets = oracle_case(V)
    views = pcnets[:V]
    args = (clf, None, targets[:3], True, scenes, 5, LOSS, DEV, SETUP)
    got_g = A.spaa(views, *args, iters=8, focus=True)
    assert A.LAST_RUN == dict(iterations=8, graph=True)                 # the small case replays a captured graph
    assert isinstance(got_g[0], list) and len(got_g[0]) == V and got_g[1].shape == (3, 3, *SZ)
    got_2 = A.spaa(tuple(views), clf, None, targets[:3], True, tuple(scenes), 5, LOSS, DEV, SETUP, iters=8, focus=True)
    assert A.LAST_RUN == dict(iterations=8, graph=True) and _same(got_2, got_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    got_e = A.spaa(views, *args, iters=8, focus=True)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and _same(got_e, got_g)
    monkeypatch.undo()
    assert not torch.equal(got_g[1], torch.full_like(got_g[1], 0.5))    # (somebody succeeded: the images are not the grey start)
    # the sweep's list forms, graph and eager
    cfgs = _sweep_configs(targets)
    res_g = A.spaa_sweep(views, clf, None, scenes, SETUP, DEV, cfgs, iters=6)
    assert A.LAST_RUN == dict(iterations=6, graph=True)
    tr = []
    res_e = A.spaa_sweep(views, clf, None, scenes, SETUP, DEV, cfgs, iters=6, trace=tr)
    assert A.LAST_RUN == dict(iterations=6, graph=False) and len(res_g) == len(res_e) == len(cfgs)
    assert all(_same(g, e) for g, e in zip(res_g, res_e))
    # one configuration: the sweep's batch is spaa()'s batch, so the result is spaa()'s bitwise
    for loss, d_thr, targeted, tg in cfgs[:2]:
        (swept,) = A.spaa_sweep(views, clf, None, scenes, SETUP, DEV, [(loss, d_thr, targeted, tg)], iters=6)
        assert _same(swept, A.spaa(views, clf, None, tg, targeted, scenes, d_thr, loss, DEV, SETUP, iters=6))
    # several configurations in one batch (other tile choices, other rounding): after one iteration, spaa()'s images to 1e-5
    res_1 = A.spaa_sweep(views, clf, None, scenes, SETUP, DEV, cfgs, iters=1)
    for (cams, prj), (loss, d_thr, targeted, tg) in zip(res_1, cfgs):
        want = A.spaa(views, clf, None, tg, targeted, scenes, d_thr, loss, DEV, SETUP, iters=1)
        assert len(cams) == V and all((c - w).abs().max() <= 1e-5 for c, w in zip(cams, want[0])) and (prj - want[1]).abs().max() <= 1e-5
    # pcnet=[p] is pcnet=p
    one = A.spaa(views[0], clf, None, targets[:3], True, scenes[0], 5, LOSS, DEV, SETUP, iters=6)
    for seq, sc in (([views[0]], scenes[0]), ((views[0],), [scenes[0]])):
        got = A.spaa(seq, clf, None, targets[:3], True, sc, 5, LOSS, DEV, SETUP, iters=6, focus=True)
        assert isinstance(got[0], torch.Tensor) and torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])


def test_argument_errors(hip, pcnets, clf):
    """With a device in reach: the errors of the list forms are raised before any engine is leased or kernel launched; a scene of the
    wrong size for its view is refused; four views are served."""
    A = hip['attack']
    scenes = [view_scene(v) for v in range(4)]
    twins = [make_pcnet(hip, view_sd(0), SZ) for _ in range(5)]
    other = make_pcnet(hip, syn.pcnet_state_dict(0, cam_sz=(48, 64), mask='rect'), (48, 64))
    clf2 = hip['clf'].Classifier('resnet18', DEV, state_dict=_csd(), input_sz=INPUT_SZ)

    def run(pcnet, cam_scene, classifier=clf2, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, cam_scene, 5, LOSS, DEV, SETUP, iters=2, **kw)

    def sweep(pcnet, cam_scene, classifier=clf2, **kw):
        return A.spaa_sweep(pcnet, classifier, None, cam_scene, SETUP, DEV, [(LOSS, 5, True, [1, 2])], iters=2, **kw)

    for call in (run, sweep):
        with pytest.raises(TypeError, match='spaa_amd.PCNet'):
            call([twins[0], torch.nn.Identity()], scenes[:2])
        with pytest.raises(ValueError, match='at most 4'):
            call(twins, scenes + scenes[:1])
        with pytest.raises(ValueError, match='twice'):
            call([twins[0], twins[0]], scenes[:2])
        with pytest.raises(ValueError, match='one scene per view'):
            call(twins[:2], scenes[:3])
        with pytest.raises(NotImplementedError, match='ensemble'):
            call(twins[:2], scenes[:2], classifier=[clf2, clf])
        with pytest.raises(TypeError, match='spaa_amd.Classifier'):
            call(twins[:2], scenes[:2], classifier=lambda im, cp: None)
        with pytest.raises(NotImplementedError, match='f16'):
            call(twins[:2], scenes[:2], storage='f16')
        with pytest.raises(ValueError, match='same camera size'):
            call([twins[0], other], [scenes[0], syn.scenes(1, 1, (48, 64))])
    with pytest.raises(ValueError, match='cam_scene must be'):
        sweep(twins[:2], [scenes[0], syn.scenes(1, 1, (48, 64))])
    assert all(not p._engines for p in twins + [other]) and not clf2._engines
    cams, prj = run(twins[:4], scenes)                                  # four views are served, each with engines of its own
    assert len(cams) == 4 and all(c.shape == (2, 3, *SZ) for c in cams) and torch.isfinite(prj).all()
    assert all(sum(len(v) for v in p._engines.values()) == 1 for p in twins[:4]) and not twins[4]._engines
    assert sum(len(v) for v in clf2._engines.values()) == 4             # V engines of the one classifier
    with pytest.raises(ValueError, match='but PCNet outputs'):           # (spaa() learns a scene's size when it builds the state)
        run(twins[:2], [scenes[0], syn.scenes(1, 1, (48, 64))])
    with pytest.raises(ValueError, match='1 or len'):
        run(twins[:2], [scenes[0], syn.scenes(1, 3, SZ)])
