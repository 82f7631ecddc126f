"""GPU (-m gpu): the projector One-pixel DE attacker's fast route (spaa_amd/one_pixel_attacker.py, csrc/onepixel.hip).
spaa_onepixel_warp bitwise against host painting + spaa_warp_fwd_taps, its cat8 output bitwise against s * xw;
spaa_capture_preproc bitwise against torch's truncation + spaa_preproc_fwd; batch-position independence; the energies of every
vector of the reference fixture tests/golden/prj_onepixel_*.npz within the tolerance the fixture stores (see
tests/golden/make_golden_onepixel_prj.py for its rule) and every argmax equal; whole attacks against the fixture; fast against
foreign route; the driver with capture='model'; the error cases."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from spaa_amd import synthetic as syn
from spaa_amd.classifier import Classifier, IMAGENET_MEAN, IMAGENET_STD, center_crop_origin
from spaa_amd.de import DifferentialEvolution
from spaa_amd.models import PCNet, WarpingNet, C_ptr
from spaa_amd.one_pixel_attacker import ProjectorOnePixelAttacker, SimulatedCapture, _CaptureEvaluator, perturb_image

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[len('prj_onepixel_'):-4] for p in glob.glob(os.path.join(GOLDEN, 'prj_onepixel_*.npz')))
LABELS = {i: f'class{i}' for i in range(1000)}
MEASURED = {}     # case -> largest |GPU energy - fixture energy|
# projector size, camera size, affine: the 64 x 64 fixture geometry, pcnet_nonsq.npz's, and a magnified warp whose clamped border
# gives taps outside the projector image
GEOM = {'sq': ((64, 64), (64, 64), None), 'nonsq': ((64, 64), (48, 80), None),
        'outside': ((40, 56), (64, 64), (1.2, 0.02, 0.05, -0.03, 1.2, 0.05))}


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
    v[: P // 4, :, 0] = d            # squares against every image edge
    v[P // 4: P // 2, :, 1] = W - 1 - d
    v[P // 2: (5 * P) // 8, :, 0] = H - 1 - d
    v[(5 * P) // 8: (3 * P) // 4, :, 1] = d
    return v.reshape(P, 5 * npix)


def make_pcnet(cam, seed=0, affine=None):
    kw = dict(affine=affine) if affine is not None else {}
    sd = syn.pcnet_state_dict(seed, cam_sz=cam, mask='rect', **kw)
    pc = PCNet(sd['mask'], WarpingNet(out_size=cam))
    pc.load_state_dict(sd)
    return pc.to(DEV)


_ENGINES = {}


def tap_table(geom):
    """(tap_src, tap weight x mask) of the geometry's engine, built once."""
    if geom not in _ENGINES:
        prj, cam, affine = GEOM[geom]
        eng = make_pcnet(cam, affine=affine).engine(1, prj)
        _ENGINES[geom] = (eng.tap_src, eng.tap_wm)
    return _ENGINES[geom]


@pytest.mark.parametrize('P,npix,ps,geom', [
    (1, 1, 1, 'sq'), (5, 2, 9, 'sq'), (37, 3, 41, 'sq'), (64, 1, 41, 'sq'),
    (5, 1, 41, 'nonsq'), (37, 2, 9, 'nonsq'), (64, 3, 1, 'nonsq'),
    (1, 3, 9, 'outside'), (37, 1, 1, 'outside'), (64, 2, 9, 'outside'),
])
def test_warp_bitwise(lib, P, npix, ps, geom):
    (Hp, Wp), (Hc, Wc), _ = GEOM[geom]
    tap_src, tap_wm = tap_table(geom)
    outside = tap_src == 0x7fffffff
    masked = tap_wm.view(-1, 4).abs().sum(1) == 0
    assert masked.any() and not masked.all()                   # the rectangular mask: pixels with weight 0 and pixels without
    assert bool(outside.any()) == (geom == 'outside')
    rng = np.random.default_rng(1000 * P + 10 * npix + ps)
    im = torch.from_numpy(rng.random((3, Hp, Wp)).astype(np.float32))
    cand = random_candidates(rng, P, npix, ps, Hp, Wp)
    q = (im * 255).type(torch.uint8)
    base = nhwc4((q.type(torch.float32) / 255)[None]).to(DEV)
    imgs = torch.stack([perturb_image(c.astype(float), im, ps) for c in cand]).type(torch.float32) / 255
    x = nhwc4(imgs).to(DEV)
    scene = torch.zeros(Hc, Wc, 4, device=DEV)
    scene[..., :3] = torch.from_numpy(rng.random((Hc, Wc, 3)).astype(np.float32)).to(DEV)
    c_dev = torch.from_numpy(cand).to(DEV)
    for clamp in (0, 1):
        ref = torch.full((P, Hc, Wc, 4), float('nan'), device=DEV)
        lib.call('spaa_warp_fwd_taps', lib.ptr(x), C_ptr(tap_src), lib.ptr(tap_wm), lib.ptr(ref), P, Hp, Wp, Hc, Wc, clamp)
        for with_cat8 in (False, True):
            got = torch.full((P, Hc, Wc, 4), float('nan'), device=DEV)
            cat8 = torch.full((P, Hc, Wc, 8), float('nan'), device=DEV)
            lib.call('spaa_onepixel_warp', lib.ptr(base), lib.ptr(c_dev), P, npix, ps, C_ptr(tap_src), lib.ptr(tap_wm),
                     lib.ptr(scene), lib.ptr(got), lib.ptr(cat8) if with_cat8 else None, Hp, Wp, Hc, Wc)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
            if with_cat8:
                want = torch.zeros(P, Hc, Wc, 8, device=DEV)
                want[..., :3] = scene[..., :3]
                want[..., 3:6] = got[..., :3] * scene[..., :3]
                assert torch.equal(cat8.view(torch.int32), want.view(torch.int32))
            else:
                assert torch.isnan(cat8).all()
    assert (ref[:, masked.view(Hc, Wc)] == 0).all() and (ref[:, ~masked.view(Hc, Wc)][..., :3] != 0).any()


@pytest.mark.parametrize('P,hw,crop,out', [(3, (256, 256), (240, 240), (224, 224)), (2, (250, 300), (240, 256), (299, 299)),
                                           (5, (64, 64), (60, 60), (56, 56)), (3, (48, 80), (44, 72), (48, 48))])
@pytest.mark.parametrize('quantize', [1, 0])
def test_capture_preproc_bitwise(lib, P, hw, crop, out, quantize):
    rng = np.random.default_rng(P + quantize)
    H, W = hw
    y = torch.from_numpy(rng.random((P, H, W, 4)).astype(np.float32))
    k = torch.from_numpy(rng.integers(0, 256, size=(P, H, W, 4)).astype(np.float32)) / 255
    exact = torch.from_numpy(rng.random((P, H, W, 1)) < 0.3)
    y = torch.where(exact, k, y)                  # values exactly on k / 255 ...
    y[:, ::7, ::5] = 0.0                          # ... and the two ends of the range
    y[:, 3::7, 2::5] = 1.0
    y[..., 3] = 0
    y = y.to(DEV)
    # (the truncation on the host: the reference's capture() divides by 255 there, a true division)
    yq = ((y.cpu() * 255).to(torch.uint8).float() / 255).to(DEV) if quantize else y
    assert not quantize or not torch.equal(yq, y)
    cy0, cx0 = center_crop_origin(H, W, crop)
    mean, std = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
    ref = torch.zeros(P, *out, 4, device=DEV)
    got = torch.full((P, *out, 4), float('nan'), device=DEV)
    lib.call('spaa_preproc_fwd', lib.ptr(yq.contiguous()), lib.ptr(ref), P, H, W, cy0, cx0, crop[0], crop[1], out[0], out[1], mean, std)
    lib.call('spaa_capture_preproc', lib.ptr(y), lib.ptr(got), P, H, W, cy0, cx0, crop[0], crop[1], out[0], out[1], mean, std, quantize)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


_SHARED = {}


def fixture_setup(z):
    """(classifier, SimulatedCapture, scene) of a fixture; PCNets and classifiers are shared between the tests of this module."""
    ck = ('clf', int(z['sd_seed']), float(z['logit_gain']), tuple(z['input_sz']))
    if ck not in _SHARED:
        sd = syn.resnet18_state_dict(ck[1], logit_gain=ck[2])
        _SHARED[ck] = Classifier('resnet18', DEV, state_dict=sd, sort_results=False, input_sz=ck[3])
    pk = ('pc', int(z['pc_seed']), tuple(z['cam_sz']))
    if pk not in _SHARED:
        _SHARED[pk] = make_pcnet(pk[2], seed=pk[1])
    scene = syn.scenes(int(z['scene_seed']), 1, tuple(z['cam_sz']))[0]
    return _SHARED[ck], SimulatedCapture(_SHARED[pk], scene, quantize=bool(z['quantize'])), scene


def evaluator(z, max_batch):
    clf, cap, _ = fixture_setup(z)
    im = float(z['brightness']) * torch.ones(3, *z['prj_sz'])
    return _CaptureEvaluator(cap, clf, im, tuple(z['crop']), int(z['pixel_count']), int(z['pixel_size']), int(z['target_idx']),
                             bool(z['targeted']), max_batch, None)


def test_sample_independence(lib):
    z = np.load(os.path.join(GOLDEN, 'prj_onepixel_targeted41.npz'))
    B = 12
    ev = evaluator(z, B)
    rng = np.random.default_rng(0)
    xs = np.unique(z['calls_x'], axis=0)
    c = xs[0]
    seen = []
    for pos in range(B):
        rows = xs[rng.choice(len(xs), B, replace=False)].copy()
        rows[pos] = c
        ev._run(rows, [f'{pos}:{i}'.encode() for i in range(B)])
        seen.append(ev.memo[f'{pos}:{pos}'.encode()])
    assert len({float(e).hex() for e, _, _ in seen}) == 1 and len({a for _, a, _ in seen}) == 1


def reference_energies(z, keep):
    """What the GPU is held to: float64 where the fixture has it (quantize=False), else the reference's fp32 energies."""
    return z['calls_e64'][keep] if 'calls_e64' in z.files else z['calls_e'][keep].astype(np.float64)


@pytest.mark.parametrize('case', CASES)
def test_fixture_energies(lib, case):
    z = np.load(os.path.join(GOLDEN, f'prj_onepixel_{case}.npz'))
    ev = evaluator(z, 64)
    keep = np.ones(len(z['calls_x']), dtype=bool)       # no vector is left out: the callback's and the final capture's too
    xs, ams = z['calls_x'], z['calls_argmax']
    got = ev(xs.astype(float))
    err = float(np.abs(got.astype(np.float64) - reference_energies(z, keep)).max())
    MEASURED[case] = err
    print(f'[onepixel-prj] {case}: largest |energy - fixture| {err:.3e} over {len(xs)} vectors (tolerance {float(z["energy_tol"]):.3e}, '
          f'margin {float(z["margin"]):.3e})')
    assert err <= float(z['energy_tol'])
    assert all(ev.lookup(x)[1] == a for x, a in zip(xs, ams))


def attacker(z, cap, scene):
    info = dict(prj_im_sz=tuple(int(v) for v in z['prj_sz']), prj_brightness=float(z['brightness']),
                cam_im_sz=tuple(int(v) for v in z['cam_sz'][::-1]), classifier_crop_sz=tuple(int(v) for v in z['crop']))
    att = ProjectorOnePixelAttacker(LABELS, info, capture=cap)
    att.im_prj_org = float(z['brightness']) * torch.ones(3, *z['prj_sz'])
    att.im_cam_org = scene
    return att


@pytest.mark.parametrize('case', CASES)
def test_attack_matches_fixture(lib, case):
    z = np.load(os.path.join(GOLDEN, f'prj_onepixel_{case}.npz'))
    clf, cap, scene = fixture_setup(z)
    if case not in MEASURED:
        test_fixture_energies(lib, case)
    keep = ~z['calls_cb']
    fx = {x.tobytes(): e for x, e in zip(z['calls_x'][keep], z['calls_e'][keep])}
    fr = {x.tobytes(): e for x, e in zip(z['calls_x'][keep], reference_energies(z, keep))}
    tol = float(z['energy_tol'])
    kw = dict(targeted_attack=bool(z['targeted']), target_idx=int(z['target_idx']), pixel_count=int(z['pixel_count']),
              pixel_size=int(z['pixel_size']), maxiter=int(z['maxiter']), popsize=int(z['popsize']))
    if float(z['margin']) > 10 * MEASURED[case]:
        att = attacker(z, cap, scene)
        trace = []
        np.random.seed(int(z['seed']))
        df, im_prj_adv, im_cam_adv = att(att.im_prj_org, clf, verbose=False, true_label=str(z['true_label']), trace=trace, **kw)
        r = att.last_result
        assert np.array_equal(r.x, z['x']) and (r.nfev, r.nit, r.success) == (int(z['nfev']), int(z['nit']), bool(z['success_de']))
        assert df.iloc[0].pred_idx == z['df_pred_idx'] and df.iloc[0].success == z['df_success']
        assert im_prj_adv.dtype == torch.uint8 and torch.equal(im_prj_adv.cpu(), torch.from_numpy(z['im_prj_adv']))
        # the capture: within the PCNet forward tolerance, or one 8-bit step where a value sits on a boundary
        step = 1 / 255 if bool(z['quantize']) else 0.0
        assert (im_cam_adv.cpu() - torch.from_numpy(z['im_cam_adv'])).abs().max().item() <= step + float(z['delta'])
        print(f'[onepixel-prj] {case}: end to end, nfev {r.nfev}, classified {r.classified}')
    else:
        # teacher-forced: the GPU evaluates every candidate (checked against the fixture), DE consumes the fixture's energies
        ev = evaluator(z, max(5, int(z['popsize'])))

        def forced(params):
            e = ev(params)
            for i, x in enumerate(np.asarray(params).astype(int)):
                if x.tobytes() in fx:
                    assert abs(float(e[i]) - float(fr[x.tobytes()])) <= tol
                    e[i] = fx[x.tobytes()]
            return e

        t, targeted = int(z['target_idx']), bool(z['targeted'])

        def cb(x, conv):
            a = ev.lookup(x)[1]
            return True if ((targeted and a == t) or (not targeted and a != t)) else None

        d = int(z['pixel_size']) // 2
        h, w = z['prj_sz']
        bounds = [(d, h - 1 - d), (d, w - 1 - d), (0, 255), (0, 255), (0, 255)] * int(z['pixel_count'])
        np.random.seed(int(z['seed']))
        r = DifferentialEvolution(forced, bounds, maxiter=int(z['maxiter']), popsize=max(1, int(z['popsize']) // len(bounds)),
                                  recombination=1, atol=-1, callback=cb, polish=False).solve()
        assert np.array_equal(r.x, z['x']) and (r.nfev, r.nit) == (int(z['nfev']), int(z['nit']))
        print(f'[onepixel-prj] {case}: teacher-forced (margin {float(z["margin"]):.2e} <= 10 x {MEASURED[case]:.2e})')


def test_fast_and_foreign_routes_agree(lib):
    """quantize=False: both routes are held to float64 within energy_tol, so to each other within twice that; the foreign route is
    SimulatedCapture as a plain callable (pcnet.forward per candidate) with a sorting classifier."""
    z = np.load(os.path.join(GOLDEN, 'prj_onepixel_noquant.npz'))
    clf, cap, scene = fixture_setup(z)
    xs = np.unique(z['calls_x'], axis=0)
    fast = evaluator(z, 16)(xs.astype(float))
    sd = syn.resnet18_state_dict(int(z['sd_seed']), logit_gain=float(z['logit_gain']))
    sorting = Classifier('resnet18', DEV, state_dict=sd, sort_results=True, input_sz=tuple(z['input_sz']))
    att = attacker(z, cap, scene)
    t, e64 = int(z['target_idx']), {x.tobytes(): e for x, e in zip(z['calls_x'], z['calls_e64'])}
    for x, ef in zip(xs, fast):
        raw, _, _ = sorting(att.perturb_project_capture(x.astype(float), att.im_prj_org, int(z['pixel_size']))[1], tuple(z['crop']))
        p = torch.softmax(raw.detach(), dim=1)[0, t].item()
        es = 1 - p if bool(z['targeted']) else p
        assert abs(es - e64[x.tobytes()]) <= float(z['energy_tol']) and abs(es - float(ef)) <= 2 * float(z['energy_tol'])
    # and a whole attack through the foreign route takes one capture per candidate
    trace = []
    np.random.seed(int(z['seed']))
    att(att.im_prj_org, sorting, targeted_attack=True, target_idx=t, pixel_count=1, pixel_size=int(z['pixel_size']), maxiter=1,
        popsize=int(z['popsize']), trace=trace)
    assert 'classified' not in att.last_result and len(trace) == att.last_result.nfev


def _write_labels(path, labels):
    with open(path, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def test_driver_with_model_capture(lib, tmp_path):
    from PIL import Image
    from spaa_amd import io
    from spaa_amd import projector_based_attack as A
    z = np.load(os.path.join(GOLDEN, 'prj_onepixel_targeted41.npz'))
    clf, _, _ = fixture_setup(z)
    pc = _SHARED[('pc', int(z['pc_seed']), tuple(z['cam_sz']))]
    sz = (64, 64)
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(1, 2, sz), str(setup_path / 'cam/raw/ref'))           # img_0001, img_0002
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    ten = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in ten})
    cfg = A.get_attacker_cfg('One-pixel_DE', str(root), ['synth'], device_ids=[0])
    cfg.classifier_names, cfg.maxiter = ['resnet18'], 1
    A.run_projector_based_attack(cfg, models={'synth': pc}, classifiers={'resnet18': clf}, capture='model')
    names = [f'img_{i:04d}.png' for i in range(1, 12)]
    leaf = os.path.join('One-pixel_DE', '-', '-', 'resnet18')
    for kind in ('prj/adv', 'cam/infer/adv'):
        assert sorted(os.listdir(setup_path / kind / leaf)) == names
    assert sorted(os.listdir(setup_path / 'cam/raw')) == ['ref']                   # simulated captures do not pose as real ones
    # the same attacks by hand on the same RNG stream: untargeted first (saved as img_0011), then the targeted ones
    scene = io.torch_imread(str(setup_path / 'cam/raw/ref/img_0002.png'))
    att = ProjectorOnePixelAttacker(LABELS, io.load_setup_info(str(setup_path)), capture=SimulatedCapture(pc, scene))
    att.im_cam_org = scene
    true_idx = int(clf(scene, (60, 60))[0][0].argmax())
    np.random.seed(0)
    runs = [(11, False, true_idx, 50), (1, True, ten[0], 10), (2, True, ten[1], 10)]
    for no, targeted, t, popsize in runs:
        _, prj, cam = att(0.5 * torch.ones(3, *sz), clf, targeted, target_idx=t, pixel_count=1, pixel_size=41, maxiter=1, popsize=popsize)
        assert np.array_equal(np.asarray(Image.open(setup_path / 'prj/adv' / leaf / f'img_{no:04d}.png')), prj.permute(1, 2, 0).cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(setup_path / 'cam/infer/adv' / leaf / f'img_{no:04d}.png')),
                              np.uint8(cam.permute(1, 2, 0).cpu().numpy() * 255))
    with pytest.raises(ValueError, match='trained PCNet'):
        A.run_projector_based_attack(cfg, models={'synth': torch.nn.Identity()}, classifiers={'resnet18': clf}, capture='model')
    two = A.get_attacker_cfg('One-pixel_DE', str(root), ['synth', 'other'])
    with pytest.raises(ValueError, match='exactly one setup'):
        A.run_projector_based_attack(two, models={'synth': pc}, classifiers={'resnet18': clf}, capture='model')
    with pytest.raises(NotImplementedError, match='projector'):
        A.run_projector_based_attack(cfg, models={'synth': pc}, classifiers={'resnet18': clf})


def test_errors(lib):
    z = np.load(os.path.join(GOLDEN, 'prj_onepixel_targeted41.npz'))
    clf, cap, scene = fixture_setup(z)
    pc = _SHARED[('pc', int(z['pc_seed']), tuple(z['cam_sz']))]
    with pytest.raises(ValueError, match='camera size'):
        SimulatedCapture(pc, torch.rand(3, 32, 32))
    att = attacker(z, cap, scene)
    with pytest.raises(ValueError, match='out of range'):
        att(att.im_prj_org, clf, target_idx=1000, pixel_size=5, maxiter=1, popsize=10)
    with pytest.raises(ValueError, match='no valid square centre'):
        att(att.im_prj_org, clf, target_idx=3, pixel_size=65, maxiter=1, popsize=10)
    sd = syn.resnet18_state_dict(int(z['sd_seed']), logit_gain=float(z['logit_gain']))
    cpu_clf = Classifier('resnet18', 'cpu', state_dict=sd, sort_results=False, input_sz=(56, 56))
    with pytest.raises(RuntimeError, match='GPU only'):
        att(att.im_prj_org, cpu_clf, target_idx=3, pixel_size=5, maxiter=1, popsize=10)
    # the engine's new entry refuses to run without a scene, and a missing pointer is an error, not a launch
    eng = pc.engine(2, (64, 64), owner=att)
    eng.scene = None
    with pytest.raises(RuntimeError, match='set_scene'):
        eng.forward_from_xw()
    with pytest.raises(RuntimeError, match='spaa_onepixel_warp'):
        lib.call('spaa_onepixel_warp', None, None, 1, 1, 1, None, None, None, None, None, 64, 64, 64, 64)
