"""GPU (-m gpu): the One-pixel DE attacker's fast route (spaa_amd/one_pixel_attacker.py, csrc/onepixel.hip).  The two kernels
against their host definitions (spaa_onepixel_preproc bitwise against spaa_preproc_fwd of the host-perturbed image;
spaa_onepixel_score against torch.softmax / numpy.argmax), batch-position independence, the energies of every vector of the
reference fixture tests/golden/onepixel_*.npz, whole attacks against the fixture, a SciPy replay of a GPU attack, and the
error cases."""
import glob
import os

import numpy as np
import pytest
import torch
from scipy.optimize import differential_evolution as scipy_de

from spaa_amd import synthetic as syn
from spaa_amd.classifier import Classifier, IMAGENET_MEAN, IMAGENET_STD, center_crop_origin
from spaa_amd.de import DifferentialEvolution
from spaa_amd.one_pixel_attacker import DigitalOnePixelAttacker, _FastEvaluator, perturb_image

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[len('onepixel_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'onepixel_*.npz')))
LABELS = {i: f'class{i}' for i in range(1000)}
MEASURED = {}     # case -> largest |GPU energy - fixture energy|


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


def nhwc4(x):
    b, c, h, w = x.shape
    out = torch.zeros(b, h, w, 4, dtype=x.dtype)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.contiguous()


def random_candidates(rng, P, npix, ps, H, W):
    d = ps // 2
    v = np.empty((P, npix, 5), dtype=np.int32)
    v[..., 0] = rng.integers(d, H - d, size=(P, npix))
    v[..., 1] = rng.integers(d, W - d, size=(P, npix))
    v[..., 2:] = rng.integers(0, 256, size=(P, npix, 3))
    v[: P // 4, :, 0] = d            # squares against the image edge: cut by the center crop
    v[P // 4: P // 2, :, 1] = W - 1 - d
    return v.reshape(P, 5 * npix)


@pytest.mark.parametrize('P,npix,ps,hw,crop,out', [
    (400, 1, 5, (256, 256), (240, 240), (224, 224)),
    (37, 3, 41, (256, 256), (240, 240), (299, 299)),
    (64, 2, 1, (250, 300), (240, 256), (224, 224)),
    (9, 3, 5, (240, 320), (224, 224), (299, 299)),
])
def test_preproc_bitwise(lib, P, npix, ps, hw, crop, out):
    import ctypes as C
    rng = np.random.default_rng(P)
    H, W = hw
    im = torch.from_numpy(rng.random((3, H, W)).astype(np.float32))
    cand = random_candidates(rng, P, npix, ps, H, W)
    q = (im * 255).type(torch.uint8)
    base = nhwc4((q.type(torch.float32) / 255)[None]).to(DEV)
    # the host-perturbed images, through the existing preprocessing kernel
    imgs = torch.stack([perturb_image(c.astype(float), im, ps) for c in cand]).type(torch.float32) / 255
    y = nhwc4(imgs).to(DEV)
    cy0, cx0 = center_crop_origin(H, W, crop)
    mean, std = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
    ref = torch.zeros(P, *out, 4, device=DEV)
    got = torch.full((P, *out, 4), float('nan'), device=DEV)
    lib.call('spaa_preproc_fwd', lib.ptr(y), lib.ptr(ref), P, H, W, cy0, cx0, crop[0], crop[1], out[0], out[1], mean, std)
    c_dev = torch.from_numpy(cand).to(DEV)
    lib.call('spaa_onepixel_preproc', lib.ptr(base), lib.ptr(c_dev), P, npix, ps, lib.ptr(got), H, W, cy0, cx0, crop[0], crop[1],
             out[0], out[1], mean, std)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_score_against_softmax(lib):
    rng = np.random.default_rng(3)
    P, ncls = 300, 1000
    lg = torch.from_numpy((rng.standard_normal((P, ncls)) * 4).astype(np.float32))
    lg[0, 5] = lg[0, 700] = lg[0].max() + 1.0       # a tie at the top: the first index wins
    lg[1] = 0.25                                    # all equal: index 0
    lg[2, 999] = lg[2, 998] = lg[2].max() + 2.0
    lg[3, 0] = lg[3].max() + 1e-3
    lg_d = lg.to(DEV)
    p_ref = torch.softmax(lg_d, dim=1).cpu().numpy()
    for target, targeted in ((5, 0), (700, 1), (999, 1)):
        energy = torch.zeros(P, device=DEV)
        am = torch.zeros(P, dtype=torch.int32, device=DEV)
        pmax = torch.zeros(P, device=DEV)
        lib.call('spaa_onepixel_score', lib.ptr(lg_d), ncls, target, targeted, lib.ptr(energy), lib.ptr(am), lib.ptr(pmax), P)
        e = energy.cpu().numpy()
        pt = 1 - e if targeted else e
        assert np.abs(pt - p_ref[:, target]).max() <= 1e-6
        assert np.array_equal(am.cpu().numpy(), p_ref.argmax(axis=1))
        assert np.abs(pmax.cpu().numpy() - p_ref.max(axis=1)).max() <= 1e-6
        assert am[0].item() == 5 and am[1].item() == 0 and am[2].item() == 998 and am[3].item() == 0


def fixture_classifier(z):
    sd = syn.resnet18_state_dict(int(z['sd_seed']), logit_gain=float(z['logit_gain']))
    return Classifier('resnet18', DEV, state_dict=sd, sort_results=False, input_sz=tuple(z['input_sz']))


def evaluator(z, clf, max_batch):
    im = torch.from_numpy(z['im'])
    return _FastEvaluator(clf, im, tuple(z['crop']), int(z['pixel_count']), int(z['pixel_size']), int(z['target_idx']),
                          bool(z['targeted']), max_batch, None)


def test_sample_independence(lib):
    z = np.load(os.path.join(GOLDEN, 'onepixel_demo.npz'))
    clf = fixture_classifier(z)
    B = 24
    ev = evaluator(z, clf, B)
    rng = np.random.default_rng(0)
    xs = z['calls_x']
    c = xs[0]
    seen = []
    for pos in range(B):
        rows = xs[rng.choice(len(xs), B, replace=False)].copy()
        rows[pos] = c
        ev._run(rows, [f'{pos}:{i}'.encode() for i in range(B)])
        seen.append(ev.memo[f'{pos}:{pos}'.encode()])
    assert len({float(e).hex() for e, _, _ in seen}) == 1 and len({a for _, a, _ in seen}) == 1


@pytest.mark.parametrize('case', CASES)
def test_fixture_energies(lib, case):
    z = np.load(os.path.join(GOLDEN, f'onepixel_{case}.npz'))
    clf = fixture_classifier(z)
    ev = evaluator(z, clf, 64)
    keep = ~z['calls_cb']
    xs, es, ams = z['calls_x'][keep], z['calls_e'][keep], z['calls_argmax'][keep]
    got = ev(xs.astype(float))
    err = float(np.abs(got.astype(np.float64) - es).max())
    MEASURED[case] = err
    print(f'[onepixel] {case}: largest |energy - fixture| {err:.3e} over {len(xs)} vectors (margin {float(z["margin"]):.3e})')
    assert err <= 1e-5
    assert all(ev.lookup(x)[1] == a for x, a in zip(xs, ams))


def run_attack(z, clf, **kw):
    att = DigitalOnePixelAttacker(LABELS, tuple(z['crop']))
    np.random.seed(int(z['seed']))
    df, im_adv = att(torch.from_numpy(z['im']), clf, targeted_attack=bool(z['targeted']), target_idx=int(z['target_idx']),
                     pixel_count=int(z['pixel_count']), pixel_size=int(z['pixel_size']), maxiter=int(z['maxiter']),
                     popsize=int(z['popsize']), verbose=False, true_label=int(z['target_idx']), **kw)
    return att.last_result, df, im_adv


def replay(z, trace, updating):
    """SciPy's DE with energies looked up in a GPU trace (a miss raises): the calls it makes and its result."""
    table = {x.astype(int).tobytes(): (e, a) for x, e, a in trace}
    calls = []

    def f(x):
        e = table[x.astype(int).tobytes()][0]
        calls.append(x.astype(int))
        return e

    t, targeted = int(z['target_idx']), bool(z['targeted'])

    def cb(x, conv):
        a = table[x.astype(int).tobytes()][1]
        return True if ((targeted and a == t) or (not targeted and a != t)) else None

    d = int(z['pixel_size']) // 2
    _, h, w = z['im'].shape
    bounds = [(d, h - 1 - d), (d, w - 1 - d), (0, 255), (0, 255), (0, 255)] * int(z['pixel_count'])
    np.random.seed(int(z['seed']))
    r = scipy_de(f, bounds, maxiter=int(z['maxiter']), popsize=max(1, int(z['popsize']) // len(bounds)), recombination=1,
                 atol=-1, callback=cb, polish=False, updating=updating)
    return r, calls


@pytest.mark.parametrize('case', CASES)
def test_attack_matches_fixture(lib, case):
    z = np.load(os.path.join(GOLDEN, f'onepixel_{case}.npz'))
    clf = fixture_classifier(z)
    if case not in MEASURED:
        test_fixture_energies(lib, case)
    keep = ~z['calls_cb']
    fx = {x.tobytes(): e for x, e in zip(z['calls_x'][keep], z['calls_e'][keep])}
    if float(z['margin']) > 10 * MEASURED[case]:
        trace = []
        r, df, im_adv = run_attack(z, clf, trace=trace)
        rr, calls = replay(z, trace, 'immediate')
        assert len(calls) == int(keep.sum()) and all(np.array_equal(a, b) for a, b in zip(calls, z['calls_x'][keep]))
        assert np.array_equal(r.x, z['x']) and (r.nfev, r.nit, r.success) == (int(z['nfev']), int(z['nit']), bool(z['success_de']))
        assert df.iloc[0].pred_idx == z['df_pred_idx'] and df.iloc[0].success == z['df_success']
        assert torch.equal(im_adv, torch.from_numpy(z['im_adv']))
        print(f'[onepixel] {case}: end to end, nfev {r.nfev}, classified {r.classified}')
    else:
        # teacher-forced: the GPU evaluates every candidate (checked against the fixture), DE consumes the fixture's energies
        ev = evaluator(z, clf, max(5, int(z['popsize'])))

        def forced(params):
            e = ev(params)
            for i, x in enumerate(np.asarray(params).astype(int)):
                if x.tobytes() in fx:
                    assert abs(float(e[i]) - float(fx[x.tobytes()])) <= 1e-5
                    e[i] = fx[x.tobytes()]
            return e

        t, targeted = int(z['target_idx']), bool(z['targeted'])

        def cb(x, conv):
            a = ev.lookup(x)[1]
            return True if ((targeted and a == t) or (not targeted and a != t)) else None

        d = int(z['pixel_size']) // 2
        _, h, w = z['im'].shape
        bounds = [(d, h - 1 - d), (d, w - 1 - d), (0, 255), (0, 255), (0, 255)] * int(z['pixel_count'])
        np.random.seed(int(z['seed']))
        r = DifferentialEvolution(forced, bounds, maxiter=int(z['maxiter']), popsize=max(1, int(z['popsize']) // len(bounds)),
                                  recombination=1, atol=-1, callback=cb, polish=False).solve()
        assert np.array_equal(r.x, z['x']) and (r.nfev, r.nit) == (int(z['nfev']), int(z['nit']))
        print(f'[onepixel] {case}: teacher-forced (margin {float(z["margin"]):.2e} <= 10 x {MEASURED[case]:.2e})')


@pytest.mark.parametrize('updating', ['immediate', 'deferred'])
@pytest.mark.parametrize('max_batch', [None, 7])
def test_replay_with_scipy(lib, updating, max_batch):
    z = np.load(os.path.join(GOLDEN, 'onepixel_demo.npz'))
    clf = fixture_classifier(z)
    trace = []
    r, _, _ = run_attack(z, clf, trace=trace, updating=updating, max_batch=max_batch)
    assert len({x.tobytes() for x, _, _ in trace}) == len(trace) == r.classified
    rr, _ = replay(z, trace, updating)
    assert np.array_equal(r.x, rr.x) and (r.nfev, r.nit, r.success) == (rr.nfev, rr.nit, rr.success)
    print(f'[onepixel] replay {updating} max_batch {max_batch}: nfev {r.nfev}, evaluated {r.evaluated}, '
          f'classified {r.classified}')


def test_errors(lib):
    z = np.load(os.path.join(GOLDEN, 'onepixel_demo.npz'))
    sd = syn.resnet18_state_dict(int(z['sd_seed']), logit_gain=float(z['logit_gain']))
    im = torch.from_numpy(z['im'])
    att = DigitalOnePixelAttacker(LABELS, (240, 240))
    cpu_clf = Classifier('resnet18', 'cpu', state_dict=sd, sort_results=False, input_sz=(64, 64))
    with pytest.raises(RuntimeError, match='GPU only'):
        att(im, cpu_clf, target_idx=3, pixel_size=5, maxiter=1, popsize=10)
    clf = Classifier('resnet18', DEV, state_dict=sd, sort_results=False, input_sz=(64, 64))
    with pytest.raises(ValueError, match='no valid square centre'):
        att(im, clf, target_idx=3, pixel_size=im.shape[1] + 2, maxiter=1, popsize=10)
    assert not clf._engines        # raised before any engine was built or any launch made
