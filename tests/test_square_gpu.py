"""GPU (-m gpu): the Square Attack's fast route (spaa_amd/square_attack.py, csrc/square_ops.hip).  One step() against the composition
of the entry points that were there before -- host painting, spaa_warp_fwd_taps, PCNetEngine.forward_from_xw, spaa_capture_preproc,
ClassifierEngine.forward_pre -- bitwise through the logits, with the camera's 8-bit step on and off; about 12 teacher-forced
iterations against the foreign route on the same SimulatedCapture and classifier (proposals exactly, decisions wherever the float64
margins exceed square_oracle.loss_bar, at most 10 % of them excluded that way); resting samples frozen and the query counter; the
early stop; the driver's 'Square' branch with capture='model'."""
import os

import numpy as np
import pytest
import torch

import square_cases as sc
import square_oracle as sq
from spaa_amd import synthetic as syn
from spaa_amd import square_attack as sa
from spaa_amd.classifier import Classifier
from spaa_amd.models import PCNet, WarpingNet, C_ptr, to_nhwc4
from spaa_amd.one_pixel_attacker import SimulatedCapture

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LABELS = {i: f'class{i}' for i in range(1000)}
N = sc.NET
INFO = dict(prj_im_sz=N['prj_sz'], prj_brightness=N['brightness'], cam_im_sz=N['cam_sz'][::-1], classifier_crop_sz=N['crop'])
_SHARED = {}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


def nets():
    """(PCNet, classifier, scene), built once"""
    if not _SHARED:
        sd = syn.pcnet_state_dict(N['pc_seed'], cam_sz=N['cam_sz'], mask='rect')
        pc = PCNet(sd['mask'], WarpingNet(out_size=N['cam_sz']))
        pc.load_state_dict(sd)
        csd = syn.resnet18_state_dict(N['sd_seed'], logit_gain=N['logit_gain'])
        _SHARED.update(pc=pc.to(DEV), clf=Classifier('resnet18', DEV, state_dict=csd, sort_results=False, input_sz=N['input_sz']),
                       scene=syn.scenes(N['scene_seed'], 1, N['cam_sz'])[0])
    return _SHARED['pc'], _SHARED['clf'], _SHARED['scene']


def host_images(x_packed, prop):
    """float32 [B K][Hp][Wp][4] on the device: every sample's image with each of its proposals painted, u8 / 255 on the host"""
    x = sa.unpack_u8(x_packed).permute(0, 2, 3, 1).cpu().numpy()
    prop = prop.cpu().numpy()
    B, K, _ = prop.shape
    imgs = np.stack([sq.paint(x[b], list(prop[b, k])) for b in range(B) for k in range(K)])
    out = torch.zeros(*imgs.shape[:3], 4)
    out[..., :3] = torch.from_numpy(imgs).type(torch.float32) / 255
    return out.to(DEV)


class Holder:
    """owns the second pair of engines"""


@pytest.mark.parametrize('quantize', [True, False])
def test_step_equals_composition(lib, quantize):
    pc, clf, scene = nets()
    cap = SimulatedCapture(pc, scene, quantize=quantize)
    att = sa.ProjectorSquareAttacker(LABELS, INFO, capture=cap)
    true_idx = int(clf(scene.to(DEV), N['crop'])[0][0].argmax())
    st = att.state(clf, [sc.TARGETS[0], true_idx, sc.TARGETS[2]], [True, False, True], eps8=48, n_iters=1000, p_init=0.1, proposals=3, seed=5)
    assert isinstance(st, sa.FastSquareState)
    B, K, P = 3, 3, 9
    before = np.zeros((B, 4), dtype=np.int32)
    holder = Holder()
    pe = pc.engine(P, N['prj_sz'], owner=holder, storage='f32')
    assert pe is not st.pe
    pe.set_scene(to_nhwc4(cap.cam_scene).expand(P, -1, -1, -1).contiguous())
    eng = clf.engine(P, (pe.Hc, pe.Wc), N['crop'], owner=holder)
    assert eng is not st.eng
    for t in range(3):
        x_before = st.x_u8.clone()
        st.step()
        logits = st.logits.clone()
        assert st.h == (0 if t == 0 else sa.square_side(t, 1000, 0.1, *N['prj_sz']))
        imgs = host_images(x_before, st.prop)
        lib.call('spaa_warp_fwd_taps', lib.ptr(imgs), C_ptr(pe.tap_src), lib.ptr(pe.tap_wm), lib.ptr(pe.a['xw']), P, *N['prj_sz'], pe.Hc, pe.Wc, 1)
        assert torch.equal(pe.a['xw'].view(torch.int32), st.pe.a['xw'].view(torch.int32))
        if pe.needs_cat8:
            cat = torch.zeros(P, pe.Hc, pe.Wc, 8, device=DEV)
            cat[..., :3] = pe.scene[..., :3]
            cat[..., 3:6] = pe.a['xw'][..., :3] * pe.scene[..., :3]
            pe.a['cat8'].copy_(cat)
        y = pe.forward_from_xw()
        lib.call('spaa_capture_preproc', lib.ptr(y), lib.ptr(eng.pre), P, pe.Hc, pe.Wc, eng.cy0, eng.cx0, eng.ch, eng.cw, eng.oh, eng.ow,
                 eng._mean, eng._std, int(quantize))
        want = eng.forward_pre()
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and torch.equal(want.view(torch.int32), logits.view(torch.int32)), t
        # and the tables follow from those logits: the chosen capture is kept, the chosen square painted
        state, rows = st.state.cpu().numpy(), st.rows.view(B, K, 4).cpu().numpy()
        x_now = sa.unpack_u8(st.x_u8).permute(0, 2, 3, 1).cpu().numpy()
        x_old = sa.unpack_u8(x_before).permute(0, 2, 3, 1).cpu().numpy()
        for b in range(B):
            if before[b, 2]:                            # a sample that rests keeps its tables
                assert state[b, 0] == 0 and np.array_equal(state[b, 1:], before[b, 1:]) and np.array_equal(x_now[b], x_old[b])
                continue
            ks = int(np.argmin(rows[b, :K if t else 1, 0]))    # (the stripes: one candidate)
            assert state[b, 1] == ks and state[b, 3] == before[b, 3] + (1 if t == 0 else K)
            if state[b, 0]:
                assert torch.equal(st.cam_best[b], y[b * K + ks])
                assert np.array_equal(x_now[b], sq.paint(x_old[b], list(st.prop[b, ks].cpu().numpy())))
            else:
                assert np.array_equal(x_now[b], x_old[b])
        assert t > 0 or state[:, 0].all()               # the stripes are accepted unconditionally
        before = state
    assert not before[:, 2].all()                       # some sample searched to the end


@pytest.mark.parametrize('case', sorted(sc.ROUTE_CASES))
def test_teacher_forced_against_foreign_route(lib, case):
    pc, clf, scene = nets()
    cap = SimulatedCapture(pc, scene, quantize=False)
    c = sc.ROUTE_CASES[case]
    true_idx = int(clf(scene.to(DEV), N['crop'])[0][0].argmax())
    labels = list(sc.TARGETS) if c['targeted'] else [true_idx] * 3
    kw = dict(eps8=c['eps8'], n_iters=c['n_iters'], p_init=c['p_init'], proposals=c['K'], seed=c['seed'])
    fast = sa.ProjectorSquareAttacker(LABELS, INFO, capture=cap).state(clf, labels, c['targeted'], **kw)
    slow = sa.ProjectorSquareAttacker(LABELS, INFO, capture=lambda im: cap(im)).state(clf, labels, c['targeted'], **kw)
    assert isinstance(fast, sa.FastSquareState) and isinstance(slow, sa.ForeignSquareState)
    B, K = 3, c['K']
    total = excluded = 0
    worst = 0.0
    for t in range(c['iters'] + 1):
        # teacher forcing: the foreign side starts every iteration from the GPU's own tables
        slow.x_u8 = sa.unpack_u8(fast.x_u8).permute(0, 2, 3, 1).cpu().numpy()
        slow.best_loss = fast.best_loss.double().cpu().numpy()
        slow.state = fast.state.cpu().numpy().astype(np.int64)
        best_before, done_before = slow.best_loss.copy(), slow.state[:, 2].copy()
        fast.step()
        slow.step()
        assert fast.h == slow.h and np.array_equal(fast.prop.cpu().numpy(), slow.prop)           # proposals: exactly
        state, rows = fast.state.cpu().numpy(), fast.rows.view(B, K, 4).cpu().numpy()
        assert np.array_equal(state[:, 3], slow.state[:, 3])                                    # queries: exactly
        nk = K if t else 1
        for b in range(B):
            if done_before[b]:
                continue
            loss = slow.rows[b, :nk, 0]
            ks = int(slow.state[b, 1])
            bar = max(sq.loss_bar(slow.logits[(b, k)]) for k in range(nk))
            worst = max(worst, float(np.abs(rows[b, :nk, 0] - loss).max()) / bar)
            margin = min([abs(loss[ks] - best_before[b])] + [abs(loss[k] - loss[ks]) for k in range(nk) if k != ks])
            total += 1
            if margin <= bar:
                excluded += 1
                continue
            assert tuple(state[b, :3]) == tuple(slow.state[b, :3]), (t, b, margin, bar)
    sq.note(f'teacher-forced {case}: {excluded} of {total} decisions within the loss bar; largest |fp32 route loss - foreign route loss| / bar '
            f'= {worst:.3f} (the two routes run the networks at different batch sizes)')
    assert total >= 30 and excluded <= sc.MAX_EXCLUDED * total


def test_resting_samples_and_queries(lib):
    pc, clf, scene = nets()
    cap = SimulatedCapture(pc, scene, quantize=True)
    att = sa.ProjectorSquareAttacker(LABELS, INFO, capture=cap)
    kw = dict(eps8=40, n_iters=1000, p_init=0.1, proposals=2, seed=9, p_thresh=0.0)
    probe = att.state(clf, [0, 0, 0, 0], False, **kw)
    probe.step()
    top1 = probe.rows.view(4, 2, 4)[:, 0, 1].cpu().numpy().astype(int)
    del probe
    # samples 0 and 2 must search (untargeted on their own top-1); sample 1 (untargeted on another class) and sample 3 (targeted on its
    # own top-1, p_thresh 0) succeed with the stripes and rest from iteration 1 on
    labels, flags = [top1[0], (top1[1] + 1) % 1000, top1[2], top1[3]], [False, False, False, True]
    st = att.state(clf, labels, flags, **kw)
    st.step()
    state0 = st.state.cpu().numpy()
    assert state0[:, 0].all() and list(state0[:, 2]) == [0, 1, 0, 1] and list(state0[:, 3]) == [1, 1, 1, 1]
    frozen = [t.clone() for t in (st.x_u8, st.best_loss, st.state, st.cam_best)]
    for t in range(1, 5):
        st.step()
        state = st.state.cpu().numpy()
        assert list(state[:, 3]) == [1 + 2 * t, 1, 1 + 2 * t, 1] and list(state[:, 2]) == [0, 1, 0, 1]
        prop = st.prop.cpu().numpy()
        assert not prop[[1, 3]].any() and (prop[[0, 2], :, 2] == st.h).all() and st.h > 0
        for now, then in zip((st.x_u8, st.best_loss, st.cam_best), (frozen[0], frozen[1], frozen[3])):
            assert torch.equal(now[[1, 3]].view(torch.int32), then[[1, 3]].view(torch.int32))
        assert (state[[1, 3], 0] == 0).all() and np.array_equal(state[[1, 3], 1:], state0[[1, 3], 1:])
    assert (st.best_loss <= frozen[1]).all()
    prj, cam, info = st.results()
    assert prj.dtype == torch.uint8 and tuple(prj.shape) == (4, 3, *N['prj_sz']) and tuple(cam.shape) == (4, 3, *N['cam_sz'])
    assert torch.equal(prj, sa.unpack_u8(st.x_u8)) and (torch.abs(prj.int() - 127) == 40).all()
    assert list(info['success']) == [False, True, False, True] and list(info['queries']) == [9, 1, 9, 1] and info['iterations'] == 4
    assert torch.equal(SimulatedCapture._over255((cam * 255).round().type(torch.uint8)), cam)      # the camera's 8-bit step: k / 255
    # every sample rests after the stripes: the loop stops at its first look
    prj, cam, info = att.attack(clf, [(t + 1) % 1000 for t in top1], False, check_every=10, **kw)
    assert info['iterations'] == 0 and info['success'].all() and list(info['queries']) == [1, 1, 1, 1]
    with pytest.raises(ValueError, match='out of range'):
        att.attack(clf, [1000], True, eps8=8, n_iters=2)


def _write_labels(path, labels):
    with open(path, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def test_driver_with_model_capture(lib, tmp_path):
    from PIL import Image
    from spaa_amd import io
    from spaa_amd import projector_based_attack as A
    pc, clf, _ = nets()
    sz = N['prj_sz']
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=N['crop'], prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(1, 2, sz), str(setup_path / 'cam/raw/ref'))           # img_0001, img_0002
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    ten = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in ten})
    cfg = A.get_attacker_cfg('Square', str(root), ['synth'], device_ids=[0])
    cfg.classifier_names, cfg.square_eps8, cfg.square_iters, cfg.square_proposals = ['resnet18'], 32, 3, 2
    A.run_projector_based_attack(cfg, models={'synth': pc}, classifiers={'resnet18': clf}, capture='model')
    names = [f'img_{i:04d}.png' for i in range(1, 12)]
    leaf = os.path.join('Square', '-', '-', 'resnet18')
    for kind in ('prj/adv', 'cam/infer/adv'):
        assert sorted(os.listdir(setup_path / kind / leaf)) == names
    assert sorted(os.listdir(setup_path / 'cam/raw')) == ['ref']                   # simulated captures do not pose as real ones
    # the same batch by hand
    scene = io.torch_imread(str(setup_path / 'cam/raw/ref/img_0002.png'))
    att = sa.ProjectorSquareAttacker(LABELS, io.load_setup_info(str(setup_path)), capture=SimulatedCapture(pc, scene))
    true_idx = int(clf(scene.to(DEV), N['crop'])[0][0].argmax())
    prj, cam, info = att.attack(clf, ten + [true_idx], [True] * 10 + [False], eps8=32, n_iters=3, proposals=2)
    for i in (0, 5, 10):
        assert np.array_equal(np.asarray(Image.open(setup_path / 'prj/adv' / leaf / names[i])), prj[i].permute(1, 2, 0).cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(setup_path / 'cam/infer/adv' / leaf / names[i])),
                              np.uint8(cam[i].permute(1, 2, 0).cpu().numpy() * 255))
    with pytest.raises(ValueError, match='trained PCNet'):
        A.run_projector_based_attack(cfg, models={'synth': torch.nn.Identity()}, classifiers={'resnet18': clf}, capture='model')
