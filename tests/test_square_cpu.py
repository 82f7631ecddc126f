"""CPU: the Square Attack's host side (spaa_amd/square_attack.py).  The side schedule on both sides of every boundary; the Python-integer
draws; the foreign route of ProjectorSquareAttacker, driven with the oracle PCNet as the `capture` callable and the oracle classifier,
against the independent restatement tests/square_oracle.py -- integers exactly, losses to float64 roundoff; every named mutation of
the oracle changes some output these tests compare; resting, the query counter and the early stop; the argument refusals; the new
entry points in the header and the library; the driver's 'Square' branch with a capture function."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import spaa_oracle as so
import square_cases as sc
import square_oracle as sq
from spaa_amd import synthetic as syn
from spaa_amd import projector_based_attack as A
from spaa_amd import square_attack as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = {i: f'class{i}' for i in range(1000)}
CHECKED = ('h', 'prop', 'rows', 'state', 'best_loss', 'x_u8')      # what the route comparisons compare, per iteration


def test_schedule_boundaries():
    """n_iters = 10000 makes `it` the iteration number itself: the divisor changes right after 10, 50, 200, 500, 1000, 2000, 4000, 6000
    and 8000.  At 256 x 256 and p_init = 0.8 the ten sides round(sqrt(0.8 * 65536 / d)) are all different."""
    sides = {1: 229, 2: 162, 4: 114, 8: 81, 16: 57, 32: 40, 64: 29, 128: 20, 256: 14, 512: 10}
    assert all(int(round(math.sqrt(0.8 * 65536 / d))) == h for d, h in sides.items())
    bounds = [10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000]
    ds = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    for side in (sa.square_side, sq.side):
        assert side(1, 10000, 0.8, 256, 256) == 229 and side(10000, 10000, 0.8, 256, 256) == 10
        for i, bound in enumerate(bounds):
            assert side(bound, 10000, 0.8, 256, 256) == sides[ds[i]], (side, bound)
            assert side(bound + 1, 10000, 0.8, 256, 256) == sides[ds[i + 1]], (side, bound)
        # `it` is truncated: iteration 3 of 2000 is it = 15, iteration 2 is it = 10
        assert side(2, 2000, 0.8, 256, 256) == 229 and side(3, 2000, 0.8, 256, 256) == 162
        # the clamps: at least 1, at most min(Hp, Wp) - 1
        assert side(10000, 10000, 0.001, 40, 56) == 1
        assert side(1, 10000, 1.0, 40, 56) == 39 and side(1, 10000, 1.0, 56, 40) == 39
        assert side(1, 10000, 0.05, 64, 64) == 14


def test_draws_agree_with_the_oracle():
    assert sa.FIRST_INIT == sq.INIT and sa.FIRST_PROPOSE == sq.PROPOSE and len({sq.INIT, sq.PROPOSE, 0x9e3779b9, 0x85ebca6b, 0xc2b2ae35}) == 5
    for seed, b in ((0, 0), (7, 3), (0xffffffff, 70000)):
        for c0, eps8 in ((127, 16), (3, 127), (250, 20)):
            im = sa.stripes(seed, b, c0, eps8, 5, 37)
            assert im.dtype == np.uint8 and np.array_equal(im, sq.stripes(seed, b, c0, eps8, 5, 37))
            assert (im == im[:1]).all() and set(np.unique(im)) <= {max(0, c0 - eps8), min(255, c0 + eps8)}
            for t, k, h in ((1, 0, 1), (5, 7, 7), (900, 3, 39)):
                p = sa.proposal(seed, t, b, k, h, c0, eps8, 40, 56)
                assert list(p) == sq.proposal(seed, t, b, k, h, c0, eps8, 40, 56)
                assert 0 <= p[0] <= 40 - h and 0 <= p[1] <= 56 - h
    assert len({tuple(sa.stripes(1, b, 127, 16, 1, 64).reshape(-1)) for b in range(4)}) == 4      # samples draw their own stripes
    assert sa.centre(0.5) == 127 and sa.centre(1.0) == 255 and sa.centre(0.0) == 0


class OracleNet:
    """The oracle PCNet as the capture callable and the oracle classifier, both memoised, with the order of the captures recorded."""

    def __init__(self, quantize=False):
        n = sc.NET
        self.sd = syn.pcnet_state_dict(n['pc_seed'], cam_sz=n['cam_sz'], mask='rect')
        self.scene = syn.scenes(n['scene_seed'], 1, n['cam_sz'])[0]
        self.clf = so.OracleClassifier('resnet18', syn.resnet18_state_dict(n['sd_seed'], logit_gain=n['logit_gain']), sort_results=False,
                                       input_sz=n['input_sz'])
        self.quantize, self.cams, self.scores, self.order = quantize, {}, {}, []
        self.info = dict(prj_im_sz=n['prj_sz'], prj_brightness=n['brightness'], cam_im_sz=n['cam_sz'][::-1], classifier_crop_sz=n['crop'])

    def capture(self, im_prj):
        assert im_prj.dtype == torch.uint8 and tuple(im_prj.shape) == (3, *sc.NET['prj_sz'])
        key = im_prj.numpy().tobytes()
        self.order.append(key)
        if key not in self.cams:
            y = so.pcnet_forward(self.sd, (im_prj.type(torch.float32) / 255)[None], self.scene[None])[0]
            self.cams[key] = (y * 255).type(torch.uint8).type(torch.float32) / 255 if self.quantize else y
        return self.cams[key]

    def classifier(self, cam, crop_sz):
        key = cam.numpy().tobytes()
        if key not in self.scores:
            self.scores[key] = self.clf(cam, crop_sz)
        return self.scores[key]

    def evaluate(self, im):
        """image uint8 [Hp, Wp, 3] -> logits float64, as square_oracle.run wants it"""
        cam = self.capture(torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))))
        return self.classifier(cam, sc.NET['crop'])[0][0].double().numpy()

    def true_idx(self):
        return int(self.clf(self.scene, sc.NET['crop'])[0][0].argmax())


_NET = {}


def oracle_net():
    if 'net' not in _NET:
        _NET['net'] = OracleNet()
    return _NET['net']


def route_request(case, true_idx):
    c = sc.ROUTE_CASES[case]
    labels = list(sc.TARGETS) if c['targeted'] else [true_idx] * 3
    return labels, [c['targeted']] * 3, c


def excluded_fraction(records, evaluate_logits):
    """The share of the live decisions after iteration 0 whose float64 margins -- chosen loss against best_loss, and chosen loss against
    the runner-up proposal -- lie within the fp32 loss bar: the decisions a float32 route may take differently."""
    n = close = 0
    for prev, r in zip(records, records[1:]):
        for b in range(len(r['state'])):
            if prev['state'][b, 2]:
                continue
            losses = r['rows'][b, :, 0]
            ks = int(r['state'][b, 1])
            gaps = [abs(losses[ks] - prev['best_loss'][b])] + [abs(losses[k] - losses[ks]) for k in range(len(losses)) if k != ks]
            n += 1
            close += min(gaps) <= evaluate_logits(r, b)
    return close / n


@pytest.mark.parametrize('case', sorted(sc.ROUTE_CASES))
def test_foreign_route_matches_oracle(case):
    net = oracle_net()
    labels, flags, c = route_request(case, net.true_idx())
    c0 = int(np.float32(sc.NET['brightness']) * np.float32(255))
    net.order = []
    ref = sq.run(net.evaluate, labels, flags, c['K'], *sc.NET['prj_sz'], c0, c['eps8'], c['n_iters'], c['p_init'], 0.9, c['seed'],
                 iters=c['iters'])
    ref_order, net.order = net.order, []
    att = sa.ProjectorSquareAttacker(LABELS, net.info, capture=net.capture)
    st = att.state(net.classifier, labels, flags, eps8=c['eps8'], n_iters=c['n_iters'], p_init=c['p_init'], proposals=c['K'], seed=c['seed'])
    assert isinstance(st, sa.ForeignSquareState)
    for r in ref:
        st.step()
        assert st.h == r['h'] and st.t == r['t'] + 1
        assert np.array_equal(st.prop, r['prop']) and np.array_equal(st.state, r['state']) and np.array_equal(st.x_u8, r['x_u8'])
        assert np.array_equal(st.rows[..., 1], r['rows'][..., 1])
        for got, want in ((st.rows[..., 0], r['rows'][..., 0]), (st.rows[..., 2], r['rows'][..., 2]), (st.best_loss, r['best_loss'])):
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert net.order == ref_order                          # one capture per candidate, in (b, k) order
    assert len(ref_order) == int(ref[-1]['state'][:, 3].sum())
    prj, cam, info = st.results()
    assert prj.dtype == torch.uint8 and tuple(prj.shape) == (3, 3, *sc.NET['prj_sz']) and tuple(cam.shape) == (3, 3, *sc.NET['cam_sz'])
    assert np.array_equal(prj.permute(0, 2, 3, 1).numpy(), ref[-1]['x_u8']) and np.array_equal(info['queries'], ref[-1]['state'][:, 3])
    assert (np.abs(prj.numpy().astype(int) - c0) == c['eps8']).all()         # every value sits on the L-infinity sphere
    for b in range(3):                                     # cam_adv is the capture of prj_adv
        assert torch.equal(cam[b], net.capture(prj[b]))
    # the condition of the GPU comparison (tests/test_square_gpu.py), on float64 alone: few decisions are close calls
    before = {r['t'] + 1: r['x_u8'] for r in ref}           # iteration t paints on the images iteration t - 1 left

    def bar(r, b):
        return max(sq.loss_bar(net.evaluate(sq.paint(before[r['t']][b], p))) for p in r['prop'][b])
    frac = excluded_fraction(ref, bar)
    print(f'[square] {case}: {frac:.1%} of the float64 decisions lie within the fp32 loss bar')
    assert frac <= sc.MAX_EXCLUDED


def test_every_mutation_changes_a_checked_output():
    seen = {m: set() for m in sq.MUTATIONS}
    for ev, kw in sc.synth_requests():
        base = sq.run(ev, **kw)
        for m in sq.MUTATIONS:
            other = sq.run(ev, mut=m, **kw)
            seen[m] |= {k for k in CHECKED if any(not np.array_equal(a[k], b[k]) for a, b in zip(base, other))}
    assert all(seen.values()), {m: sorted(v) for m, v in seen.items()}
    # and each slip shows where it is made
    assert 'h' in seen['h_clamp_min'] and 'prop' in seen['mod_short'] and 'prop' in seen['sign_order'] and 'rows' in seen['margin_with_y']
    assert seen['rest_counted'] == {'state'} and 'state' in seen['tie_high'] and 'x_u8' in seen['accept_le'] and 'state' in seen['no_p_thresh']


def synth_attacker(ev):
    """The foreign route on BlockEvaluate: the `capture` hands the projector image on, the `classifier` evaluates it."""
    info = dict(prj_im_sz=(32, 48), prj_brightness=127.5 / 255, cam_im_sz=(48, 32), classifier_crop_sz=(32, 32))

    def classifier(cam, crop_sz):
        return torch.from_numpy(ev(cam.permute(1, 2, 0).numpy()))[None], None, None
    return sa.ProjectorSquareAttacker({i: str(i) for i in range(sc.SYNTH_NCLS)}, info, capture=lambda im: im), classifier


def test_foreign_route_on_ties_and_resting():
    """The integer-valued evaluate: exact ties between proposals, candidates equal to best_loss, samples that succeed early and rest."""
    rested = 0
    for ev, kw in sc.synth_requests():
        ref = sq.run(ev, **kw)
        att, classifier = synth_attacker(ev)
        st = att.state(classifier, kw['labels'], kw['flags'], eps8=kw['eps8'], n_iters=kw['n_iters'], p_init=kw['p_init'], proposals=kw['K'],
                       seed=kw['seed'])
        calls = ev.calls
        for prev, r in zip([None] + ref, ref):
            st.step()
            assert st.h == r['h'] and np.array_equal(st.prop, r['prop']) and np.array_equal(st.state, r['state'])
            assert np.array_equal(st.x_u8, r['x_u8']) and np.array_equal(st.best_loss, r['best_loss'])
            for b in range(len(kw['labels'])):
                if prev is not None and prev['state'][b, 2]:      # resting: a row of zeros, nothing spent, nothing changed
                    assert not st.prop[b].any() and st.state[b, 0] == 0 and np.array_equal(st.state[b, 1:], prev['state'][b, 1:])
                    assert np.array_equal(st.x_u8[b], prev['x_u8'][b]) and st.best_loss[b] == prev['best_loss'][b]
                    rested += 1
                else:
                    assert np.array_equal(st.rows[b], np.pad(r['rows'][b], ((0, 0), (0, 1))))
        assert ev.calls - calls == int(ref[-1]['state'][:, 3].sum())          # queries = captures spent
        live = [r['state'][:, 3] for r in ref]
        assert (np.diff(np.array(live), axis=0) >= 0).all()
    assert rested > 50


def test_early_stop():
    ev, kw = sc.synth_requests()[1]
    labels, flags = kw['labels'][3:], kw['flags'][3:]               # the untargeted samples of a request in which all of them succeed
    ref = sq.run(ev, **dict(kw, labels=labels, flags=flags, b_off=3))
    last = max(int(np.argmax([r['state'][b, 2] for r in ref])) for b in range(3))
    assert all(ref[-1]['state'][:, 2]) and 0 < last < kw['n_iters'] - 12
    att, classifier = synth_attacker(ev)
    kwargs = dict(eps8=kw['eps8'], n_iters=kw['n_iters'], p_init=kw['p_init'], proposals=kw['K'], seed=kw['seed'], b_off=3)
    for every in (1, 5):
        trace, calls = [], ev.calls
        prj, cam, info = att.attack(classifier, labels, flags, check_every=every, trace=trace, **kwargs)
        stop = -(-last // every) * every                             # the first look at or after the last success
        assert info['iterations'] == stop == len(trace) - 1 and info['success'].all()
        assert np.array_equal(info['queries'], ref[-1]['state'][:, 3]) and ev.calls - calls == info['queries'].sum()
        assert np.array_equal(prj.permute(0, 2, 3, 1).numpy(), ref[-1]['x_u8']) and np.array_equal(info['best_loss'], ref[-1]['best_loss'])
        assert torch.equal(cam, prj.float())                         # (this capture hands the projector image on)
        for (t, h, prop, rows, state, best), r in zip(trace, ref):
            assert (t, h) == (r['t'], r['h']) and np.array_equal(prop, r['prop']) and np.array_equal(state, r['state'])
    # the same samples as rows 3..5 of the whole batch: b_off shifts the draws
    whole = sq.run(ev, **kw)
    assert np.array_equal(whole[-1]['x_u8'][3:], ref[-1]['x_u8']) and np.array_equal(whole[-1]['state'][3:], ref[-1]['state'])


def test_argument_refusals():
    ev, kw = sc.synth_requests()[0]
    att, classifier = synth_attacker(ev)
    good, calls = dict(eps8=8, n_iters=5), ev.calls
    with pytest.raises(TypeError, match='eps8'):
        att.attack(classifier, [1], True, n_iters=5)                 # no default budget
    with pytest.raises(TypeError, match='capture'):
        sa.ProjectorSquareAttacker({}, dict(prj_im_sz=(8, 8), prj_brightness=0.5, cam_im_sz=(8, 8), classifier_crop_sz=(8, 8)), capture=None)
    with pytest.raises(TypeError, match='classifier'):
        att.attack(None, [1], True, **good)
    for bad in (dict(eps8=0), dict(eps8=128), dict(eps8=8.0), dict(eps8=True), dict(n_iters=0), dict(p_init=0.0), dict(p_init=1.5),
                dict(proposals=0), dict(proposals=9), dict(p_thresh=1.5), dict(seed=-1), dict(seed=1 << 32), dict(check_every=0),
                dict(b_off=-1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            att.attack(classifier, [1], True, **dict(good, **bad))
    with pytest.raises(ValueError, match='empty'):
        att.attack(classifier, [], True, **good)
    with pytest.raises(ValueError, match='out of range'):
        att.attack(classifier, [sc.SYNTH_NCLS], True, **good)
    with pytest.raises(ValueError, match='entries'):
        att.attack(classifier, [1, 2], [True], **good)
    tiny = sa.ProjectorSquareAttacker({0: 'a', 1: 'b'}, dict(prj_im_sz=(1, 9), prj_brightness=0.5, cam_im_sz=(9, 1), classifier_crop_sz=(1, 1)),
                                      capture=lambda im: im)
    with pytest.raises(ValueError, match='no square side'):
        tiny.attack(classifier, [1], True, **good)
    assert ev.calls == calls                                          # nothing was captured on the way to a refusal


@pytest.mark.parametrize('name', ['spaa_square_init', 'spaa_square_propose', 'spaa_square_warp', 'spaa_square_score', 'spaa_square_commit'])
def test_header_and_library_export(name):
    from spaa_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'spaa_hip.h')).read()
    assert re.search(r'\bint\s+' + name + r'\s*\(', header)
    assert name in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_package_export():
    import spaa_amd
    assert spaa_amd.ProjectorSquareAttacker is sa.ProjectorSquareAttacker


def _write_labels(path, labels):
    with open(path, 'w') as fh:
        fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')


def test_driver_with_a_cpu_capture(tmp_path, capsys):
    """capture = function setup_info -> capture callable: the foreign route needs no GPU.  One batch of 11 samples (ten targeted, then
    the untargeted one), two iterations; eleven projector images and eleven captures, the captures under cam/raw/adv."""
    from PIL import Image
    from spaa_amd import io
    net = oracle_net()
    sz = sc.NET['prj_sz']
    root = tmp_path / 'data'
    setup_path = root / 'setups' / 'synth'
    io.save_setup_info(str(setup_path), dict(classifier_crop_sz=sc.NET['crop'], prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(sc.NET['scene_seed'], 2, sz), str(setup_path / 'cam/raw/ref'))           # img_0001, img_0002
    _write_labels(root / 'imagenet1000_clsidx_to_labels.txt', {k: f'class{k}, extra' for k in range(1000)})
    ten = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]
    _write_labels(root / 'imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in ten})
    scene = io.torch_imread(str(setup_path / 'cam/raw/ref/img_0002.png'))
    seen = []

    def make_capture(info):
        assert tuple(info['prj_im_sz']) == sz

        def capture(im_prj):
            seen.append(im_prj.clone())
            y = so.pcnet_forward(net.sd, (im_prj.type(torch.float32) / 255)[None], scene[None])[0]
            return (y * 255).type(torch.uint8).type(torch.float32) / 255
        return capture

    cfg = A.get_attacker_cfg('Square', str(root), ['synth'])
    assert cfg.stealth_losses == ['-'] and cfg.d_threshes == ['-'] and cfg.square_eps8 is None
    assert A.to_attacker_cfg_str('Square') == ('Square', None)
    cfg.classifier_names, cfg.square_iters, cfg.square_proposals = ['resnet18'], 2, 2
    with pytest.raises(NotImplementedError, match='capture='):
        A.run_projector_based_attack(cfg, classifiers={'resnet18': net.clf})
    with pytest.raises(ValueError, match='square_eps8'):
        A.run_projector_based_attack(cfg, classifiers={'resnet18': net.clf}, capture=make_capture)
    two = A.get_attacker_cfg('Square', str(root), ['synth', 'other'])
    with pytest.raises(ValueError, match='exactly one setup'):
        A.run_projector_based_attack(two, classifiers={'resnet18': net.clf}, capture=make_capture)
    assert not (setup_path / 'prj').exists() and not seen
    cfg.square_eps8 = 32
    A.run_projector_based_attack(cfg, classifiers={'resnet18': net.clf}, capture=make_capture)
    names = [f'img_{i:04d}.png' for i in range(1, 12)]
    leaf = os.path.join('Square', '-', '-', 'resnet18')
    assert sorted(os.listdir(setup_path / 'prj/adv' / leaf)) == names
    assert sorted(os.listdir(setup_path / 'cam/raw/adv' / leaf)) == names
    assert not (setup_path / 'cam/infer').exists()
    # the same batch by hand: sample i of the batch is image i + 1
    true_idx = int(net.clf(scene, sc.NET['crop'])[0][0].argmax())
    att = sa.ProjectorSquareAttacker(LABELS, io.load_setup_info(str(setup_path)), capture=make_capture(dict(prj_im_sz=sz)))
    n_seen = len(seen)
    prj, cam, info = att.attack(net.clf, ten + [true_idx], [True] * 10 + [False], eps8=32, n_iters=2, proposals=2)
    assert len(seen) - n_seen == n_seen == int(info['queries'].sum()) and (info['queries'] <= 5).all()
    for i in (0, 9, 10):
        assert np.array_equal(np.asarray(Image.open(setup_path / 'prj/adv' / leaf / names[i])), prj[i].permute(1, 2, 0).numpy())
        assert np.array_equal(np.asarray(Image.open(setup_path / 'cam/raw/adv' / leaf / names[i])),
                              np.uint8(cam[i].permute(1, 2, 0).numpy() * 255))
    # the summary step reads the reference's three attackers only
    with pytest.raises(ValueError, match='not supported'):
        A.summarize_single_attacker('Square', str(root), ['synth'])
