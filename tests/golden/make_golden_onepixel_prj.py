"""Generates tests/golden/prj_onepixel_*.npz: the REFERENCE's ProjectorOnePixelAttacker (one_pixel_attacker/__init__.py:123-245,
imported unmodified; scipy.optimize.differential_evolution underneath) with the reference's PCNet as the projector and the camera,
and the oracle classifier (oracle/spaa_oracle.py, OracleClassifier(sort_results=False)) on synthetic ResNet-18 weights.  Runs only
in the build container.

    python tests/golden/make_golden_onepixel_prj.py

The attacker is made with object.__new__ (its __init__ opens a camera and a projector window) and its attributes are set by hand;
`project` keeps the uint8 projector image and `capture` returns PCNet(prj / 255, scene), followed by the camera's 8-bit step
trunc(y * 255) / 255 (the reference's capture() returns uint8 / 255) unless the case says quantize=False.  The PCNet's weights are
synthetic.pcnet_state_dict (a centred rectangular mask, affine scale 0.9).  Every step_and_predict call is recorded (integer vector,
energy, argmax, whether the callback made it) and replayed through spaa_amd.de for `margin`, as make_golden_onepixel.py does.

Tolerances, stored in the fixture as `energy_tol`:
  quantize=False   every recorded vector is also evaluated with the oracle in float64 (`calls_e64`); energy_tol = max(3 x the fp32
                   oracle's largest error against float64, 1e-5): the project's rule for a GPU result against float64.
  quantised        a rounding-level difference in PCNet's output can move a value across a k/255 boundary.  Every vector is evaluated
                   three more times with every capture value within DELTA of a boundary forced up, forced down, or flipped at random;
                   energy_tol = 2 x the largest energy change seen + 1e-5.  DELTA = 1e-4, the PCNet forward tolerance of
                   tests/test_gpu_parity.py at 64 x 64 (relative L-inf of an output whose largest value is 1).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository root and oracle/ on sys.path)
import spaa_oracle as so  # noqa: E402
from make_golden_onepixel import Audit  # noqa: E402
from spaa_amd import synthetic as syn  # noqa: E402

SD_SEED, GAIN, FLOOR, DELTA, BRIGHTNESS = 5, 20.0, 1e-5, 1e-4, 0.5

CASES = [
    # run_projector_based_attack's targeted call (projector_based_attack.py:129-131), scaled to a 64 x 64 projector
    dict(name='targeted41', prj=(64, 64), cam=(64, 64), crop=(60, 60), input_sz=(56, 56), pc_seed=0, scene_seed=1, seed=1,
         quantize=True, target='second', kw=dict(targeted_attack=True, pixel_count=1, pixel_size=41, maxiter=4, popsize=10)),
    # the geometry of pcnet_nonsq.npz, two squares that overlap now and then
    dict(name='nonsq_2px', prj=(64, 64), cam=(48, 80), crop=(44, 72), input_sz=(48, 48), pc_seed=3, scene_seed=4, seed=2,
         quantize=True, target='top', kw=dict(targeted_attack=False, pixel_count=2, pixel_size=9, maxiter=2, popsize=20)),
    # the callback stops after the first generation: untargeted on a class that is not the prediction
    dict(name='early_stop', prj=(64, 64), cam=(64, 64), crop=(60, 60), input_sz=(56, 56), pc_seed=0, scene_seed=1, seed=3,
         quantize=True, target='second', kw=dict(targeted_attack=False, pixel_count=1, pixel_size=1, maxiter=10, popsize=10)),
    # the first case without the camera's 8-bit step
    dict(name='noquant', prj=(64, 64), cam=(64, 64), crop=(60, 60), input_sz=(56, 56), pc_seed=0, scene_seed=1, seed=1,
         quantize=False, target='second', kw=dict(targeted_attack=True, pixel_count=1, pixel_size=41, maxiter=4, popsize=10)),
]


def trunc8(y):
    return (y * 255).type(torch.uint8).type(torch.float32) / 255


def forced(y, mode, rng):
    """trunc8(y) with every value within DELTA of a boundary k/255 put above it ('up'), below it ('down') or either ('random')."""
    k = torch.round(y * 255)
    near = (y - k / 255).abs() < DELTA
    if mode == 'up':
        side = torch.ones_like(near)
    elif mode == 'down':
        side = torch.zeros_like(near)
    else:
        side = torch.from_numpy(rng.integers(0, 2, size=tuple(y.shape)).astype(bool))
    q = torch.where(side, k, k - 1).clamp(0, 255)
    return torch.where(near, q / 255, trunc8(y))


def energy_of(p, t, targeted):
    return np.float32(1 - p[0, t] if targeted else p[0, t])


def main():
    ref = mg.ref_shims.load_reference()
    sys.modules.pop('one_pixel_attacker', None)
    import one_pixel_attacker as ref_opa
    assert not hasattr(ref_opa, 'mock_calls'), 'the one_pixel_attacker stub is still in place'
    csd = syn.resnet18_state_dict(SD_SEED, logit_gain=GAIN)
    csd64 = {k: v.double() for k, v in csd.items()}
    labels = {i: f'class{i}' for i in range(1000)}
    for c in CASES:
        kw = dict(c['kw'])
        clf = so.OracleClassifier('resnet18', csd, sort_results=False, input_sz=c['input_sz'])
        sd = syn.pcnet_state_dict(c['pc_seed'], cam_sz=c['cam'], mask='rect')
        pc = mg.ref_shims.make_reference_pcnet(ref, sd, c['prj'], c['cam'])
        scene = syn.scenes(c['scene_seed'], 1, c['cam'])[0]
        # (classes ranked on the capture of the unperturbed projector image: what the attack starts from)
        with torch.no_grad():
            start = pc(((BRIGHTNESS * torch.ones(3, *c['prj']) * 255).type(torch.uint8).type(torch.float32) / 255)[None], scene[None])[0]
        ranked = [int(i) for i in np.argsort(-clf(trunc8(start) if c['quantize'] else start, c['crop'])[1][0], kind='stable')[:2]]
        kw['target_idx'] = t = ranked[0] if c['target'] == 'top' else ranked[1]
        targeted = kw['targeted_attack']
        true_label = labels[int(clf(scene, c['crop'])[1][0].argmax())]

        att = object.__new__(ref_opa.ProjectorOnePixelAttacker)
        att.class_names, att.classifier_crop_sz = labels, c['crop']
        att.prj_im_sz, att.prj_brightness, att.cam_im_sz = c['prj'], BRIGHTNESS, c['cam'][::-1]
        att.delay_time, att.delay_frames = 0.0, 0
        att.im_prj_org = BRIGHTNESS * torch.ones(3, *c['prj'])
        att.im_cam_org = scene
        shown = {}

        def project(im, delay_time=0.3):
            assert im.dtype == torch.uint8
            shown['prj'] = im.clone()

        def raw_capture():
            with torch.no_grad():
                return pc((shown['prj'].type(torch.float32) / 255)[None], scene[None])[0]

        def capture(delay_frames=13):
            y = raw_capture()
            return trunc8(y) if c['quantize'] else y

        att.project, att.capture = project, capture
        calls, in_cb = [], [False]
        orig_sp, orig_succ = att.step_and_predict, att.attack_success

        def sp(x, im, classifier, pixel_size):
            p = orig_sp(x, im, classifier, pixel_size)
            calls.append((x.astype(int), energy_of(p, t, targeted), int(p[0].argmax()), in_cb[0]))
            return p

        def succ(*a, **k):
            in_cb[0] = True
            try:
                return orig_succ(*a, **k)
            finally:
                in_cb[0] = False

        att.step_and_predict, att.attack_success = sp, succ
        got = {}
        real_de = ref_opa.differential_evolution

        def spy(*a, **k):
            got['ret'] = real_de(*a, **k)
            return got['ret']

        ref_opa.differential_evolution = spy
        np.random.seed(c['seed'])
        df, im_prj_adv, im_cam_adv = att(att.im_prj_org, clf, verbose=True, true_label=true_label, **kw)
        ref_opa.differential_evolution = real_de
        r = got['ret']
        xs = np.array([k[0] for k in calls])
        es = np.array([k[1] for k in calls], dtype=np.float32)
        ams = np.array([k[2] for k in calls])
        cbs = np.array([k[3] for k in calls])

        # replay the consumed energies through spaa_amd.de: same decisions, and the smallest acceptance margin
        table = {x.tobytes(): e for x, e, cb in zip(xs, es, cbs) if not cb}
        d = kw['pixel_size'] // 2
        h, w = c['prj']
        bounds = [(d, h - 1 - d), (d, w - 1 - d), (0, 255), (0, 255), (0, 255)] * kw['pixel_count']
        popmul = max(1, kw['popsize'] // len(bounds))
        cb_iter = iter([k for k in calls if k[3]])

        def cb(x, conv):
            k = next(cb_iter)
            assert np.array_equal(k[0], x.astype(int))
            return True if ((targeted and k[2] == t) or (not targeted and k[2] != t)) else None

        np.random.seed(c['seed'])
        audit = Audit(lambda P: np.array([table[x.astype(int).tobytes()] for x in P]), bounds, maxiter=kw['maxiter'],
                      popsize=popmul, recombination=1, atol=-1, callback=cb, polish=False, max_batch=1)
        rr = audit.solve()
        assert np.array_equal(rr.x, r.x) and rr.nfev == r.nfev and rr.nit == r.nit, (rr, r)

        # the tolerance of this case, over EVERY recorded vector
        extra = {}
        rng = np.random.default_rng(c['seed'] + 100)
        if c['quantize']:
            change, nnear = 0.0, 0
            for x, e in zip(xs, es):
                project(ref_opa.perturb_image(x.astype(float), att.im_prj_org, kw['pixel_size']))
                y = raw_capture()
                assert energy_of(clf(trunc8(y), c['crop'])[1], t, targeted) == e
                nnear = max(nnear, int(((y - torch.round(y * 255) / 255).abs() < DELTA).sum()))
                for mode in ('up', 'down', 'random'):
                    ef = energy_of(clf(forced(y, mode, rng), c['crop'])[1], t, targeted)
                    change = max(change, abs(float(ef) - float(e)))
            tol = 2 * change + FLOOR
            extra.update(energy_change=change, near_boundary=nnear)
        else:
            sd64 = {k: v.double() for k, v in sd.items()}
            clf64 = so.OracleClassifier('resnet18', csd64, sort_results=False, input_sz=c['input_sz'])
            e64 = []
            for x in xs:
                u8 = ref_opa.perturb_image(x.astype(float), att.im_prj_org, kw['pixel_size'])
                y = so.pcnet_forward(sd64, (u8.double() / 255)[None], scene.double()[None])[0]
                p = clf64(y, c['crop'])[1]
                e64.append(float(1 - p[0, t] if targeted else p[0, t]))
            e64 = np.array(e64)
            own = float(np.abs(es.astype(np.float64) - e64).max())
            tol = max(3 * own, FLOOR)
            extra.update(calls_e64=e64, oracle_err64=own)
        row = df.iloc[0]
        mg.save('prj_onepixel_' + c['name'], seed=c['seed'], prj_sz=np.array(c['prj']), cam_sz=np.array(c['cam']), crop=np.array(c['crop']),
                input_sz=np.array(c['input_sz']), pc_seed=c['pc_seed'], scene_seed=c['scene_seed'], brightness=BRIGHTNESS,
                quantize=c['quantize'], targeted=targeted, target_idx=t, true_label=true_label, pixel_count=kw['pixel_count'],
                pixel_size=kw['pixel_size'], maxiter=kw['maxiter'], popsize=kw['popsize'], sd_seed=SD_SEED, logit_gain=GAIN,
                x=r.x, fun=r.fun, nfev=r.nfev, nit=r.nit, success_de=r.success,
                df_true_idx=row.true_idx, df_pred_idx=row.pred_idx, df_success=row.success, df_true_p=row.true_p,
                df_pred_p=row.pred_p, df_cdiff=row.cdiff, df_pixel_count=row.pixel_count, df_classifier=row.classifier,
                im_prj_adv=im_prj_adv.numpy(), im_cam_adv=im_cam_adv.numpy(), calls_x=xs, calls_e=es, calls_argmax=ams, calls_cb=cbs,
                margin=audit.margin, delta=DELTA, energy_tol=tol, **extra)
        print(f"  {c['name']}: nfev {r.nfev} nit {r.nit} calls {len(calls)} margin {audit.margin:.3e} energy_tol {tol:.3e} "
              f"{ {k: (v if np.ndim(v) == 0 else '...') for k, v in extra.items()} } success {row.success} pred {row.pred_idx} "
              f"({row.pred_p:.3f})")


if __name__ == '__main__':
    main()
