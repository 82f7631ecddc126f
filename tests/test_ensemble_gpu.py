"""GPU: the ensemble attack loop (EnsembleAttackState through spaa / spaa_sweep / the driver) on a 64 x 64 synthetic PCNet: one
teacher-forced first iteration against the float64 oracle (tests/ensemble_oracle.py), twelve traced iterations whose sample tables
must be the stated functions of the member tables, the eager / graph / repeat / one-member identities, the argument errors and the
driver's '+' names."""
import os

import numpy as np
import pytest
import torch

import ensemble_oracle as eo
import spaa_oracle as so
from spaa_amd import synthetic as syn
from test_gpu_parity import hip, make_pcnet  # noqa: F401  (hip: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SZ = (64, 64)
SETUP = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ)
LOSS = 'camdE_caml2'
P_THRESH = 0.9
PCNET_SEED, SCENE_SEED = 0, 1
# name -> (state dict, input size): test-sized bodies
BODIES = {'resnet18': (lambda: syn.resnet18_state_dict(2, logit_gain=20.0), (56, 56)),
          'vgg16': (lambda: syn.vgg16_state_dict(3, logit_gain=5.0, fc_width=256), (48, 48)),
          'inception_v3': (lambda: syn.inception_v3_state_dict(4, logit_gain=20.0), (107, 107))}
TARGETED = [True, True, False, False]
D_THR = [5.0, 5.0, 9.0, 5.0]
UNTARGETED_OTHER = 7               # an untargeted sample on a class that no member gives the scene: every member fooled from the start


_CSD = {}


def _csd(name):
    if name not in _CSD:
        _CSD[name] = BODIES[name][0]()
    return _CSD[name]


def oracle_case(names):
    """CPU side of a case: PCNet weights, scene, the oracle's members, the B = 4 targets (two targeted, then untargeted on the first
    member's class of the scene and on UNTARGETED_OTHER)."""
    sd = syn.pcnet_state_dict(PCNET_SEED, cam_sz=SZ, mask='rect')
    scene = syn.scenes(SCENE_SEED, 1, SZ)
    ocs = [so.OracleClassifier(n, _csd(n), input_sz=BODIES[n][1]) for n in names]
    true_idx = int(ocs[0](scene, SETUP['classifier_crop_sz'])[0][0].argmax())
    return sd, scene, ocs, [204, 291, true_idx, UNTARGETED_OTHER]


def clear_pairs(ref):
    """[B][K]: the oracle's own margins say that an fp32 implementation must decide this (sample, member) pair as it does."""
    return (ref['gap'] > 1e-3) & (ref['p_margin'] > 1e-3)


@pytest.fixture(scope='module')
def members(hip):
    return {n: hip['clf'].Classifier(n, DEV, state_dict=_csd(n), input_sz=BODIES[n][1]) for n in BODIES}


@pytest.fixture(scope='module')
def pcnet(hip):
    return make_pcnet(hip, syn.pcnet_state_dict(PCNET_SEED, cam_sz=SZ, mask='rect'), SZ)


@pytest.mark.parametrize('names', [('resnet18', 'vgg16'), ('resnet18', 'vgg16', 'inception_v3')])
def test_first_iteration_against_the_oracle(hip, pcnet, members, names):
    A = hip['attack']
    K, B = len(names), 4
    sd, scene, ocs, targets = oracle_case(names)
    ref = eo.first_iteration(sd, ocs, targets, TARGETED, scene, D_THR, SETUP, p_thresh=P_THRESH)
    clear = clear_pairs(ref)
    clear_d = ref['d_margin'] > 1e-3
    print(f'oracle {names}: top-2 gaps {ref["gap"].tolist()}, |p1 - p_thresh| {ref["p_margin"].tolist()}, |caml2 255 - d_thr| '
          f'{ref["d_margin"].tolist()}, fooled {ref["fooled"].astype(int).tolist()}, best_adv {ref["best_adv"].tolist()}')
    assert (~clear).sum() <= 1 and clear_d.all(), 'the case itself is near a tie: choose other seeds'
    assert (ref['nfooled'] > 0).any() and (ref['nfooled'] < K).any()       # members disagree somewhere: the tables are not trivial

    for focus in (False, True):
        st = A.EnsembleAttackState(pcnet, [members[n] for n in names], targets, scene, [LOSS] * B, SETUP, DEV, focus=focus)
        assert st.K == K and len({id(e) for e in st.clfs}) == K
        st.forward_decide(TARGETED, D_THR, P_THRESH)
        st.backward_step(2, 1)
        es, ef, ew = st.ens_state.cpu().numpy(), st.ens_stats.cpu().numpy().astype(np.float64), st.ens_w.cpu().numpy()
        state, stats = st.state.cpu().numpy(), st.stats.cpu().numpy().astype(np.float64)
        # member rows and sample flags: the oracle's wherever its margins are clear
        assert (es[clear] == ref['ens_state'][clear]).all(), (es, ref['ens_state'])
        row = clear.all(axis=1)
        assert (state[row, 0] == ref['state_succ'][row]).all() and (state[row, 3] == ref['nfooled'][row]).all()
        assert (state[row & clear_d, 1] == ref['best_adv'][row & clear_d]).all()
        w_ref = eo.focus_weights(ref['fooled'], focus)
        assert (ew[row] == w_ref[row]).all()
        assert np.allclose(ef[..., 0][clear], ref['p1'][clear], rtol=1e-3) and np.allclose(ef[..., 1], ref['tl'], rtol=1e-3, atol=1e-3)
        assert np.allclose(stats[:, 1], ref['caml2'], rtol=1e-4)
        # wiring: the state's g_adv is the combination of the member engines' OWN gradient images with the weights it wrote
        g_own = [e.g_y.reshape(B, -1, 4).cpu().numpy().astype(np.float64) for e in st.clfs]
        g_adv = st.g_adv.reshape(B, -1, 4).cpu().numpy().astype(np.float64)
        own = eo.combine(g_own, ew)
        err = np.abs(g_adv - own).max(axis=(1, 2)) / np.abs(own).max(axis=(1, 2))
        print(f'{names} focus {focus}: g_adv against the float64 combination of the engines\' own gradients, per sample {err.tolist()}')
        assert (err <= 2e-6).all() and (g_adv[..., 3] == 0).all()
        # against the oracle's direction: nothing beyond the members' own unit-vector errors and the new kernels' rounding
        e_bk = np.stack([np.sqrt(((eo.unit_images(g_own[k])[0] - eo.unit_images(ref['g'][k])[0]) ** 2).sum(axis=(1, 2)))
                         for k in range(K)], axis=1)                                       # [B][K]
        ref_adv = eo.combine(ref['g'], ew)                                                 # (the oracle's members, the weights used)
        l2 = np.sqrt(((g_adv - ref_adv) ** 2).sum(axis=(1, 2)))
        bound = (ew * e_bk).sum(axis=1) + 2e-6 * K
        print(f'{names} focus {focus}: unit-vector errors of the members {e_bk.tolist()}, combined direction L2 error {l2.tolist()}, '
              f'bound {bound.tolist()}')
        assert (l2 <= bound).all()
        del st


def _sweep_configs(targets):
    return [(LOSS, D_THR[0], True, targets[:2]), (LOSS, D_THR[2], False, targets[2:3]), (LOSS, D_THR[3], False, targets[3:])]


@pytest.mark.parametrize('focus', [False, True])
def test_twelve_traced_iterations(hip, pcnet, members, focus):
    """In every iteration state and stats are the stated functions of the member tables; col_loss_best never rises; the images stay
    finite and in range."""
    A = hip['attack']
    names = ('resnet18', 'vgg16')
    K = len(names)
    _, scene, _, targets = oracle_case(names)
    tr = []
    res = A.spaa_sweep(pcnet, [members[n] for n in names], None, scene, SETUP, DEV, _sweep_configs(targets), iters=12, trace=tr,
                       focus=focus, p_thresh=P_THRESH)
    assert A.LAST_RUN == dict(iterations=12, graph=False)
    assert len(tr) == 1 and len(tr[0]) == 12 and all(len(e) == 4 for e in tr[0])
    targeted = torch.tensor(TARGETED)
    d_thr = torch.tensor(D_THR)
    best_before = torch.full((4,), 1e6)
    seen_col_step = seen_adv_step = False
    for i, entry in enumerate(tr[0]):
        state, stats, es, ef = (t.cpu() for t in entry)
        assert state.shape == (4, 4) and stats.shape == (4, 8) and es.shape == (4, K, 2) and ef.shape == (4, K, 2)
        succ, fooled = (es[..., 0] & 1).bool(), (es[..., 0] & 2).bool()
        assert ((es[..., 0] & ~3) == 0).all() and (es[..., 1] >= 0).all() and (es[..., 1] < 1000).all()
        want_succ = torch.where(targeted[:, None], es[..., 1] == torch.tensor(targets)[:, None], es[..., 1] != torch.tensor(targets)[:, None])
        assert torch.equal(succ, want_succ), i
        assert torch.equal(fooled, torch.where(targeted[:, None], succ & (ef[..., 0] > P_THRESH), succ)), i
        high_pert = stats[:, 1] * 255.0 > d_thr                        # (fp32, as the kernel)
        best_adv = fooled.all(dim=1) & high_pert
        assert torch.equal(state[:, 0].bool(), succ.all(dim=1)) and torch.equal(state[:, 1].bool(), best_adv), i
        assert torch.equal(state[:, 3], fooled.sum(dim=1).int()), i
        assert torch.equal(stats[:, 0], ef[..., 0].min(dim=1).values), i
        tl = ef[..., 1].double()
        assert ((stats[:, 6].double() - tl.mean(dim=1)).abs() <= K * 2.0 ** -24 * tl.abs().sum(dim=1)).all(), i
        best = best_adv & (stats[:, 3] < best_before)
        assert torch.equal(state[:, 2].bool(), best), i
        assert torch.equal(stats[:, 5], torch.where(best, stats[:, 3], best_before)) and (stats[:, 5] <= best_before).all(), i
        best_before = stats[:, 5].clone()
        seen_col_step |= bool(best_adv.any())
        seen_adv_step |= bool((~best_adv).any())
    assert seen_col_step and seen_adv_step                              # both steps were taken in this run
    for (cam, prj), cfg in zip(res, _sweep_configs(targets)):
        assert cam.shape == (len(cfg[3]), 3, *SZ) and prj.shape == (len(cfg[3]), 3, *SZ)
        assert torch.isfinite(cam).all() and torch.isfinite(prj).all() and prj.min() >= 0 and prj.max() <= 1


def test_identities(hip, pcnet, members, monkeypatch):
    """Eager and graph-replayed runs, and two runs, are bitwise equal; a sequence of one member is that member's plain attack."""
    A = hip['attack']
    names = ('resnet18', 'vgg16')
    clfs = [members[n] for n in names]
    _, scene, _, targets = oracle_case(names)
    args = (None, targets[:3], True, scene, 5, LOSS, DEV, SETUP)
    cam_g, prj_g = A.spaa(pcnet, clfs, *args, iters=8, focus=True)
    assert A.LAST_RUN == dict(iterations=8, graph=True)
    cam_2, prj_2 = A.spaa(pcnet, tuple(clfs), *args, iters=8, focus=True)
    assert A.LAST_RUN == dict(iterations=8, graph=True) and torch.equal(cam_2, cam_g) and torch.equal(prj_2, prj_g)
    monkeypatch.setattr(A, 'GRAPH_MAX_PIXELS', 0)
    cam_e, prj_e = A.spaa(pcnet, clfs, *args, iters=8, focus=True)
    assert A.LAST_RUN == dict(iterations=8, graph=False) and torch.equal(cam_e, cam_g) and torch.equal(prj_e, prj_g)
    monkeypatch.undo()
    # the sweep's per-sample form, graph and eager
    cfgs = _sweep_configs(targets)
    res_g = A.spaa_sweep(pcnet, clfs, None, scene, SETUP, DEV, cfgs, iters=6)
    assert A.LAST_RUN == dict(iterations=6, graph=True)
    tr = []
    res_e = A.spaa_sweep(pcnet, clfs, None, scene, SETUP, DEV, cfgs, iters=6, trace=tr)
    assert A.LAST_RUN == dict(iterations=6, graph=False)
    for (cg, pg), (ce, pe) in zip(res_g, res_e):
        assert torch.equal(cg, ce) and torch.equal(pg, pe)
    # classifier=[c] is classifier=c
    one = A.spaa(pcnet, clfs[0], *args, iters=6)
    for seq in ([clfs[0]], (clfs[0],)):
        got = A.spaa(pcnet, seq, *args, iters=6, focus=True)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
    tr1, tr2 = [], []
    A.spaa(pcnet, clfs[0], *args, iters=2, trace=tr1)
    A.spaa(pcnet, [clfs[0]], *args, iters=2, trace=tr2)
    assert all(len(e) == 2 for e in tr2) and all(torch.equal(a, b) for x, y in zip(tr1, tr2) for a, b in zip(x, y))


def test_argument_errors(hip, pcnet, members):
    """The errors are raised before any engine is leased or kernel launched."""
    A = hip['attack']
    r18 = members['resnet18']
    scene = syn.scenes(SCENE_SEED, 1, SZ)
    twins = [hip['clf'].Classifier('resnet18', DEV, state_dict=_csd('resnet18'), input_sz=(56, 56)) for _ in range(5)]
    small = hip['clf'].Classifier('resnet18', DEV, state_dict=syn.resnet18_state_dict(2, num_classes=10), input_sz=(56, 56))

    def run(classifier, **kw):
        return A.spaa(pcnet, classifier, None, [1, 2], True, scene, 5, LOSS, DEV, SETUP, iters=2, **kw)

    def sweep(classifier, **kw):
        return A.spaa_sweep(pcnet, classifier, None, scene, SETUP, DEV, [(LOSS, 5, True, [1, 2])], iters=2, **kw)

    for call in (run, sweep):
        with pytest.raises(TypeError):
            call([twins[0], lambda im, cp: None])
        with pytest.raises(ValueError, match='at most 4'):
            call(twins)
        with pytest.raises(ValueError, match='twice'):
            call([twins[0], twins[0]])
        with pytest.raises(ValueError, match='number of classes'):
            call([twins[0], small])
        with pytest.raises(NotImplementedError):
            call([twins[0], twins[1]], storage='f16')
    assert all(not c._engines for c in twins + [small])
    cam, prj = run(twins[:4])                                       # four members are served
    assert cam.shape == (2, 3, *SZ) and torch.isfinite(prj).all()
    assert all(len(c._engines) == 1 for c in twins[:4]) and not twins[4]._engines and r18 is not twins[0]


def _write_labels(fn, labels):
    with open(fn, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def test_driver_writes_the_ensemble_folder(hip, pcnet, members, tmp_path):
    """run_projector_based_attack with a '+' name on a temporary setup folder: 11 + 11 files in the folder of that name, and
    attack_transfer on them."""
    A = hip['attack']
    from spaa_amd import io
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ, cam_im_sz=SZ))
    io.save_imgs(syn.scenes(1, 2, SZ), str(setup_path / 'cam/raw/ref'))
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    ten = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in ten})
    name = 'vgg16+resnet18'
    clfs = dict(resnet18=members['resnet18'], vgg16=members['vgg16'])
    cfg = A.get_attacker_cfg('SPAA', str(root), ['synth'], device_ids=[0])
    cfg.classifier_names, cfg.stealth_losses, cfg.d_threshes = [name], ['camdE_caml2'], [5]
    A.run_projector_based_attack(cfg, models={'synth': pcnet}, classifiers=clfs, iters=12)
    leaf = os.path.join('SPAA_PCNet_l1+ssim_500_24_2000', 'camdE_caml2', '5', name)
    files = [f'img_{i:04d}.png' for i in range(1, 12)]
    for kind in ('prj/adv', 'cam/infer/adv'):
        base = setup_path / kind
        assert {os.path.relpath(dp, base) for dp, dn, fn in os.walk(base) if fn} == {leaf}
        assert sorted(os.listdir(base / leaf)) == files
    # the same attack through spaa_sweep: the driver handed over the members in the written order and the first member's label
    scene = io.torch_imread(str(setup_path / 'cam/raw/ref/img_0002.png')).to(DEV)
    true_idx = int(members['vgg16'](scene, (60, 60))[0][0].argmax())
    (ct, pt), (cu, pu) = A.spaa_sweep(pcnet, [clfs['vgg16'], clfs['resnet18']], None, scene, io.load_setup_info(str(setup_path)), DEV,
                                      [('camdE_caml2', 5, True, ten), ('camdE_caml2', 5, False, [true_idx])], iters=12)
    io.save_imgs(torch.cat((pt, pu)), str(tmp_path / 'want'))
    ims = torch.stack([io.torch_imread(str(setup_path / 'prj/adv' / leaf / f)) for f in files])
    want = torch.stack([io.torch_imread(str(tmp_path / 'want' / f)) for f in files])
    assert torch.equal(ims, want)
    cams = torch.stack([io.torch_imread(str(setup_path / 'cam/infer/adv' / leaf / f)) for f in files])
    got = A.attack_transfer(cams, [clfs['vgg16'], clfs['resnet18']], ten + [true_idx], [True] * 10 + [False], (60, 60))
    assert got.shape == (11, 2) and got.dtype == bool
    for k, c in enumerate((clfs['vgg16'], clfs['resnet18'])):
        top1 = c(cams.to(DEV), (60, 60))[0].argmax(dim=1).cpu().numpy()
        assert np.array_equal(got[:, k], np.where([True] * 10 + [False], top1 == np.array(ten + [true_idx]), top1 != np.array(ten + [true_idx])))
    with pytest.raises(ValueError, match='classifiers='):
        A.run_projector_based_attack(cfg, models={'synth': pcnet}, classifiers=dict(resnet18=members['resnet18']))
