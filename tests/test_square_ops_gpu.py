"""GPU (-m gpu): the Square Attack's entry points (csrc/square_ops.hip) through the C ABI, one at a time, into sentinel-filled outputs
with guard words behind them.  spaa_square_init and spaa_square_propose against the Python-integer draws of tests/square_oracle.py;
spaa_square_warp bitwise against host painting + spaa_warp_fwd_taps on the three small geometries, its cat8 output bitwise against
s * xw, and independent of a row's position in the batch; spaa_square_score on engineered logits (ties, a candidate equal to
best_loss, NaN rows, target hits on either side of p_thresh, a resting sample) with the loss held to float64 within
square_oracle.loss_bar; spaa_square_commit bitwise against a host restatement; every bad argument is refused and writes nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import square_cases as sc
import square_oracle as sq
from spaa_amd import synthetic as syn
from spaa_amd.models import PCNet, WarpingNet, C_ptr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -1            # int32 sentinel (0xffffffff: no packed pixel, whose top byte is 0, and no valid state word)
GUARD = 64


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from spaa_amd import _lib
    _lib.load()
    return _lib


def guarded(n, dtype=torch.int32, fill=SENT):
    """n elements and GUARD more behind them, all `fill`: (the whole buffer, its first n elements)"""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def tail_intact(buf, n, fill=SENT):
    t = buf[n:]
    return bool(torch.isnan(t).all()) if isinstance(fill, float) and math.isnan(fill) else bool((t == fill).all())


def pack(u8):
    u = u8.astype(np.int32)
    return u[..., 0] | u[..., 1] << 8 | u[..., 2] << 16


def nhwc4(imgs_u8):
    """uint8 [N, H, W, 3] -> float32 [N, H, W, 4] on the device, u8 / 255 by true division (on the host)"""
    out = torch.zeros(*imgs_u8.shape[:3], 4)
    out[..., :3] = torch.from_numpy(imgs_u8).type(torch.float32) / 255
    return out.to(DEV)


_TAPS = {}


def tap_table(geom):
    if geom not in _TAPS:
        prj, cam, affine = sc.GEOM[geom]
        kw = dict(affine=affine) if affine is not None else {}
        sd = syn.pcnet_state_dict(0, cam_sz=cam, mask='rect', **kw)
        pc = PCNet(sd['mask'], WarpingNet(out_size=cam))
        pc.load_state_dict(sd)
        eng = pc.to(DEV).engine(1, prj)
        _TAPS[geom] = (eng.tap_src, eng.tap_wm)
    return _TAPS[geom]


@pytest.mark.parametrize('B', [1, 5])
def test_init(lib, B):
    Hp, Wp = 40, 56
    for seed, b_off, c0, eps8 in ((0, 0, 127, 16), (0xfffffffe, 9, 3, 127), (5, 70000, 250, 20)):
        buf, x = guarded(B * Hp * Wp)
        lib.call('spaa_square_init', seed, b_off, c0, eps8, lib.ptr(buf), B, Hp, Wp)
        torch.cuda.synchronize()
        want = pack(np.stack([sq.stripes(seed, b_off + b, c0, eps8, Hp, Wp) for b in range(B)]))
        assert np.array_equal(x.view(B, Hp, Wp).cpu().numpy(), want) and tail_intact(buf, B * Hp * Wp)


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('B', [1, 5])
def test_propose(lib, B, K):
    Hp, Wp, c0, eps8 = 40, 56, 120, 30
    state = torch.zeros(B, 4, dtype=torch.int32)
    state[:, 3] = 11
    if B > 1:
        state[1, 2] = state[3, 2] = 1                  # two resting samples
    resting = state[:, 2].numpy().astype(bool)
    state = state.to(DEV)
    for seed, t, b_off in ((3, 1, 0), (0xffffffff, 977, 9)):
        for h in (1, 7, min(Hp, Wp) - 1, 0):
            buf, prop = guarded(B * K * 8)
            lib.call('spaa_square_propose', seed, t, b_off, h, c0, eps8, lib.ptr(state), lib.ptr(buf), B, K, Hp, Wp)
            torch.cuda.synchronize()
            want = np.zeros((B, K, 8), dtype=np.int32)
            for b in range(B):
                for k in range(K):
                    if h and not resting[b]:
                        want[b, k] = sq.proposal(seed, t, b_off + b, k, h, c0, eps8, Hp, Wp)
            assert np.array_equal(prop.view(B, K, 8).cpu().numpy(), want) and tail_intact(buf, B * K * 8)
            if h:
                live = want[~resting]
                assert (live[..., 2] == h).all() and (live[..., 0] <= Hp - h).all() and (live[..., 1] <= Wp - h).all()
                assert np.isin(live[..., 3:6], (c0 - eps8, c0 + eps8)).all()


def corner_proposals(rng, B, K, Hp, Wp):
    """prop int32 [B][K][8]: squares in all four corners, rows that paint nothing, a square of the largest side, random ones."""
    prop = np.zeros((B, K, 8), dtype=np.int32)
    top = min(Hp, Wp) - 1
    for i in range(B * K):
        h = int(rng.integers(1, top + 1)) if i % 7 != 6 else top
        r, c = int(rng.integers(0, Hp - h + 1)), int(rng.integers(0, Wp - h + 1))
        r, c = [(0, 0), (0, Wp - h), (Hp - h, 0), (Hp - h, Wp - h), (r, c), (r, c), (r, c)][i % 7]
        prop[i // K, i % K] = (r, c, h, *rng.integers(0, 256, size=3), 0, 0)
        if i % 7 == 4:
            prop[i // K, i % K, :3] = 0            # h == 0
    return prop


def painted(x, prop):
    """uint8 [B K][Hp][Wp][3]: x[b] with proposal (b, k) painted"""
    B, K, _ = prop.shape
    return np.stack([sq.paint(x[b], list(prop[b, k])) for b in range(B) for k in range(K)])


def run_warp(lib, x, prop, geom, scene, with_cat8):
    (Hp, Wp), (Hc, Wc), _ = sc.GEOM[geom]
    tap_src, tap_wm = tap_table(geom)
    B, K, _ = prop.shape
    n = B * K * Hc * Wc
    xbuf, xw = guarded(4 * n, torch.float32, float('nan'))
    cbuf, cat8 = guarded(8 * n, torch.float32, float('nan'))
    lib.call('spaa_square_warp', lib.ptr(torch.from_numpy(pack(x)).to(DEV)), lib.ptr(torch.from_numpy(prop).to(DEV)), B, K, C_ptr(tap_src),
             lib.ptr(tap_wm), lib.ptr(scene), lib.ptr(xbuf), lib.ptr(cbuf) if with_cat8 else None, Hp, Wp, Hc, Wc)
    torch.cuda.synchronize()
    assert tail_intact(xbuf, 4 * n, float('nan')) and tail_intact(cbuf, 8 * n, float('nan'))
    return xw.view(B * K, Hc, Wc, 4), cat8.view(B * K, Hc, Wc, 8)


@pytest.mark.parametrize('B,K', [(1, 1), (3, 3), (2, 8), (5, 1)])
@pytest.mark.parametrize('geom', ['sq', 'nonsq', 'outside'])
def test_warp_bitwise(lib, geom, B, K):
    (Hp, Wp), (Hc, Wc), _ = sc.GEOM[geom]
    tap_src, tap_wm = tap_table(geom)
    assert bool((tap_src == 0x7fffffff).any()) == (geom == 'outside')
    rng = np.random.default_rng(100 * B + K)
    x = rng.integers(0, 256, size=(B, Hp, Wp, 3), dtype=np.uint8)
    prop = corner_proposals(rng, B, K, Hp, Wp)
    imgs = nhwc4(painted(x, prop))
    scene = torch.zeros(Hc, Wc, 4, device=DEV)
    scene[..., :3] = torch.from_numpy(rng.random((Hc, Wc, 3)).astype(np.float32)).to(DEV)
    P = B * K
    for clamp in (0, 1):
        ref = torch.full((P, Hc, Wc, 4), float('nan'), device=DEV)
        lib.call('spaa_warp_fwd_taps', lib.ptr(imgs), C_ptr(tap_src), lib.ptr(tap_wm), lib.ptr(ref), P, Hp, Wp, Hc, Wc, clamp)
        for with_cat8 in (False, True):
            got, cat8 = run_warp(lib, x, prop, geom, scene, with_cat8)
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
            if with_cat8:
                want = torch.zeros(P, Hc, Wc, 8, device=DEV)
                want[..., :3] = scene[..., :3]
                want[..., 3:6] = got[..., :3] * scene[..., :3]
                assert torch.equal(cat8.view(torch.int32), want.view(torch.int32))
            else:
                assert torch.isnan(cat8).all()
    assert (ref[..., :3] != 0).any()
    if P > 1:                                      # the squares are seen: rows of one sample differ
        assert not torch.equal(ref[0], ref[P - 1])


def test_warp_batch_position_independence(lib):
    geom = 'outside'
    (Hp, Wp), (Hc, Wc), _ = sc.GEOM[geom]
    rng = np.random.default_rng(7)
    scene = torch.zeros(Hc, Wc, 4, device=DEV)
    im = rng.integers(0, 256, size=(1, Hp, Wp, 3), dtype=np.uint8)
    p = np.array([[[5, 9, 17, 200, 3, 90, 0, 0]]], dtype=np.int32)
    alone, _ = run_warp(lib, im, p, geom, scene, False)
    seen = []
    for b, k in ((0, 0), (2, 2), (1, 7), (4, 3)):
        x = rng.integers(0, 256, size=(5, Hp, Wp, 3), dtype=np.uint8)
        prop = corner_proposals(rng, 5, 8, Hp, Wp)
        x[b], prop[b, k] = im[0], p[0, 0]
        got, _ = run_warp(lib, x, prop, geom, scene, False)
        seen.append(got[b * 8 + k])
    assert all(torch.equal(s.view(torch.int32), alone[0].view(torch.int32)) for s in seen)


def engineered_logits(ncls, K, rng):
    """(logits float32 [8 K][ncls], label [8], targeted [8], state before [8][4], best_loss before [8]); K == 3"""
    lg = (3 * rng.standard_normal((8, K, ncls))).astype(np.float32)
    label = np.array([2, 4, 1, 0, 3, 3, 5, ncls], dtype=np.int32)
    targeted = np.array([0, 1, 0, 1, 1, 1, 0, 0], dtype=np.int32)
    lg[0, 2] = lg[0, 0]                            # sample 0: proposals 0 and 2 tie exactly, below proposal 1
    lg[0, 1] = lg[0, 0]
    lg[0, 1, 2] += 5
    lg[2, 0] = lg[2, 1]                            # sample 2: a row with one NaN away from the label, which would win if the NaN were
    lg[2, 0, 1] -= 10                              # dropped from the maximum; a row whose label logit is NaN; one good row
    lg[2, 0, 5] = np.nan
    lg[2, 2, 1] = np.nan
    lg[3] = np.nan                                 # sample 3: nothing but NaN
    a = math.log(9 * (ncls - 1))                   # the target's logit at which its probability is 0.9 over zeros
    lg[4:6] = 0
    lg[4, :, 3] = (a - 0.01, a - 1, a - 2)         # sample 4: the best candidate hits the target with p just below 0.9
    lg[5, :, 3] = (a - 1, a + 0.01, a - 0.01)      # sample 5: and just above
    state = np.zeros((8, 4), dtype=np.int32)
    best = np.full(8, np.inf, dtype=np.float32)
    state[6], best[6] = (1, 2, 1, 7), 0.5          # sample 6 rests
    return lg.reshape(8 * K, ncls), label, targeted, state, best


@pytest.mark.parametrize('ncls', [10, 1000])
def test_score(lib, ncls):
    K, B = 3, 8
    rng = np.random.default_rng(ncls)
    lg, label, targeted, state0, best0 = engineered_logits(ncls, K, rng)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    logits, lab, tg = dev(lg), dev(label), dev(targeted)
    rbuf, rows = guarded(B * K * 4, torch.float32, float('nan'))
    sbuf, state = guarded(B * 4)
    bbuf, best = guarded(B, torch.float32, float('nan'))
    state.copy_(dev(state0.reshape(-1)))
    best.copy_(dev(best0))
    lib.call('spaa_square_score', lib.ptr(logits), ncls, lib.ptr(lab), lib.ptr(tg), 0.9, K, lib.ptr(rbuf), lib.ptr(bbuf), lib.ptr(sbuf), B, K)
    torch.cuda.synchronize()
    assert tail_intact(rbuf, B * K * 4, float('nan')) and tail_intact(sbuf, B * 4) and tail_intact(bbuf, B, float('nan'))
    got_rows, got_state, got_best = rows.view(B, K, 4).cpu().numpy(), state.view(B, 4).cpu().numpy(), best.cpu().numpy()
    assert (got_rows[..., 3] == 0).all()
    # every row against float64
    worst = 0.0
    with np.errstate(invalid='ignore'):
        for b in range(B):
            for k in range(K):
                l64 = lg[b * K + k].astype(np.float64)
                if b == 7:                                       # a label outside the classes: NaN
                    assert np.isnan(got_rows[b, k, 0])
                    continue
                loss, top1, p1 = sq.score(l64, int(label[b]), bool(targeted[b]))
                if np.isnan(loss):
                    assert np.isnan(got_rows[b, k, 0])
                    continue
                worst = max(worst, abs(float(got_rows[b, k, 0]) - loss) / sq.loss_bar(l64))
                assert got_rows[b, k, 1] == top1 and abs(float(got_rows[b, k, 2]) - p1) <= 2.0 ** -24 * (ncls + 8) * p1
    sq.note(f'spaa_square_score ncls={ncls}: largest |loss - float64| / bar = {worst:.3f}')
    assert worst <= 1.0
    # the decisions, from the kernel's own losses: (accepted, k*, done, queries)
    want = {0: (1, 0, None, K), 1: (1, None, None, K), 2: (1, 1, None, K), 3: (0, 0, 0, K), 4: (1, 0, 0, K), 5: (1, 1, 1, K), 6: (0, 2, 1, 7),
            7: (0, 0, 0, K)}
    for b, (acc, ks, done, q) in want.items():
        loss = got_rows[b, :, 0]
        if ks is None:
            ks = int(np.nanargmin(loss))
        if done is None:                                         # untargeted: top-1 != label; targeted: == label with p1 > 0.9
            t1, p1 = got_rows[b, ks, 1], got_rows[b, ks, 2]
            done = int(t1 == label[b] and p1 > np.float32(0.9)) if targeted[b] else int(t1 != label[b])
        assert tuple(got_state[b]) == (acc, ks, done, q), b
        assert got_best[b].tobytes() == (loss[ks] if acc else best0[b]).tobytes(), b
    assert got_rows[0, 0, 0] == got_rows[0, 2, 0] < got_rows[0, 1, 0]                      # the tie went to the lowest k
    assert got_rows[4, 0, 1] == 3 and 0.899 < got_rows[4, 0, 2] < 0.9 < got_rows[5, 1, 2] < 0.901
    # the same candidates again: every loss now EQUALS best_loss, so nothing is accepted; live samples pay K more queries
    lib.call('spaa_square_score', lib.ptr(logits), ncls, lib.ptr(lab), lib.ptr(tg), 0.9, K, lib.ptr(rbuf), lib.ptr(bbuf), lib.ptr(sbuf), B, K)
    torch.cuda.synchronize()
    again, best2 = state.view(B, 4).cpu().numpy(), best.cpu().numpy()
    assert np.array_equal(rows.view(B, K, 4).cpu().numpy(), got_rows, equal_nan=True) and best2.tobytes() == got_best.tobytes()
    for b in range(B):
        rests = got_state[b, 2] != 0
        assert tuple(again[b]) == (0, got_state[b, 1], got_state[b, 2], got_state[b, 3] + (0 if rests else K)), b
    assert again[5, 3] == K and again[6, 3] == 7
    # count = 1 (the stripes: the K rows show one image): only row 0 competes, one query is paid
    state.copy_(dev(state0.reshape(-1)))
    best.copy_(dev(best0))
    lib.call('spaa_square_score', lib.ptr(logits), ncls, lib.ptr(lab), lib.ptr(tg), 0.9, 1, lib.ptr(rbuf), lib.ptr(bbuf), lib.ptr(sbuf), B, K)
    torch.cuda.synchronize()
    first, best1 = state.view(B, 4).cpu().numpy(), best.cpu().numpy()
    for b in range(B):
        if b == 6:
            assert tuple(first[b]) == (0, 2, 1, 7) and best1[b] == np.float32(0.5)
            continue
        ok = not np.isnan(got_rows[b, 0, 0])
        assert tuple(first[b, :2]) == (int(ok), 0) and first[b, 3] == 1, b
        assert best1[b].tobytes() == (got_rows[b, 0, 0] if ok else best0[b]).tobytes(), b


@pytest.mark.parametrize('geom', ['nonsq', 'outside'])
def test_commit_bitwise(lib, geom):
    (Hp, Wp), (Hc, Wc), _ = sc.GEOM[geom]
    B, K = 7, 3
    rng = np.random.default_rng(Hp + Wc)
    prop = corner_proposals(rng, B, K, Hp, Wp)
    #                  acc k*
    state = np.array([[1, 2, 0, 5], [0, 1, 0, 5], [1, 0, 1, 9], [1, 1, 0, 2], [0, 0, 1, 3], [1, 5, 0, 1], [1, 0, 0, 4]], dtype=np.int32)
    prop[3, 1, :3] = 0                              # accepted with h == 0: the capture is kept, nothing is painted
    prop[6, 0, :3] = (Hp - 3, 2, 5)                 # accepted, but the square leaves the image: not painted
    x = pack(rng.integers(0, 256, size=(B, Hp, Wp, 3), dtype=np.uint8))
    y = rng.random((B * K, Hc, Wc, 4)).astype(np.float32)
    cam0 = rng.random((B, Hc, Wc, 4)).astype(np.float32)
    xbuf, xd = guarded(B * Hp * Wp)
    cbuf, cam = guarded(B * Hc * Wc * 4, torch.float32, float('nan'))
    xd.copy_(torch.from_numpy(x.reshape(-1)).to(DEV))
    cam.copy_(torch.from_numpy(cam0.reshape(-1)).to(DEV))
    lib.call('spaa_square_commit', lib.ptr(torch.from_numpy(state).to(DEV)), lib.ptr(torch.from_numpy(prop).to(DEV)),
             lib.ptr(torch.from_numpy(y).to(DEV)), lib.ptr(xbuf), lib.ptr(cbuf), B, K, Hp, Wp, Hc, Wc)
    torch.cuda.synchronize()
    assert tail_intact(xbuf, B * Hp * Wp) and tail_intact(cbuf, B * Hc * Wc * 4, float('nan'))
    want_x, want_cam = x.copy(), cam0.copy()
    for b in (0, 2, 3, 6):                          # (sample 5 names a proposal that does not exist: left alone)
        ks = state[b, 1]
        want_cam[b] = y[b * K + ks]
        r, c, h = prop[b, ks, :3]
        if b != 6:
            want_x[b, r:r + h, c:c + h] = pack(prop[b, ks, 3:6])
    assert np.array_equal(xd.view(B, Hp, Wp).cpu().numpy(), want_x)
    assert cam.view(B, Hc, Wc, 4).cpu().numpy().tobytes() == want_cam.tobytes()
    assert not np.array_equal(want_x[0], x[0]) and np.array_equal(want_x[1], x[1])


def test_bad_arguments_are_refused_and_write_nothing(lib):
    (Hp, Wp), (Hc, Wc), _ = sc.GEOM['nonsq']
    tap_src, tap_wm = tap_table('nonsq')
    B, K, ncls = 2, 3, 10
    P = B * K
    xbuf, _ = guarded(B * Hp * Wp)
    pbuf, _ = guarded(P * 8)
    sbuf, _ = guarded(B * 4)
    wbuf, _ = guarded(P * Hc * Wc * 4, torch.float32, float('nan'))
    cbuf, _ = guarded(P * Hc * Wc * 8, torch.float32, float('nan'))
    rbuf, _ = guarded(P * 4, torch.float32, float('nan'))
    bbuf, _ = guarded(B, torch.float32, float('nan'))
    mbuf, _ = guarded(B * Hc * Wc * 4, torch.float32, float('nan'))
    scene, logits = torch.zeros(Hc, Wc, 4, device=DEV), torch.zeros(P, ncls, device=DEV)
    lab, y = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(P, Hc, Wc, 4, device=DEV)
    p = lib.ptr
    good = {
        'spaa_square_init': [1, 0, 127, 16, p(xbuf), B, Hp, Wp],
        'spaa_square_propose': [1, 1, 0, 5, 127, 16, p(sbuf), p(pbuf), B, K, Hp, Wp],
        'spaa_square_warp': [p(xbuf), p(pbuf), B, K, C_ptr(tap_src), p(tap_wm), p(scene), p(wbuf), p(cbuf), Hp, Wp, Hc, Wc],
        'spaa_square_score': [p(logits), ncls, p(lab), p(lab), 0.9, K, p(rbuf), p(bbuf), p(sbuf), B, K],
        'spaa_square_commit': [p(sbuf), p(pbuf), p(y), p(xbuf), p(mbuf), B, K, Hp, Wp, Hc, Wc],
    }
    bad = {
        'spaa_square_init': [(4, None), (5, 0), (5, 65536), (6, 1), (7, 1), (2, 256), (2, -1), (3, 0), (3, 128), (1, -1)],
        'spaa_square_propose': [(6, None), (7, None), (8, 0), (9, 0), (9, 9), (3, -1), (3, min(Hp, Wp)), (1, -1), (2, -1), (4, 256), (5, 0),
                                (5, 128), (10, 1)],
        'spaa_square_warp': [(0, None), (1, None), (4, None), (5, None), (7, None), (6, None), (2, 0), (3, 0), (3, 9), (9, 1), (11, 0), (12, 0)],
        'spaa_square_score': [(0, None), (2, None), (3, None), (6, None), (7, None), (8, None), (1, 1), (9, 0), (10, 0), (10, 9), (5, -1),
                              (5, 0), (5, K + 1), (4, 1.5), (4, -0.1), (4, float('nan'))],
        'spaa_square_commit': [(0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, 0), (6, 9), (7, 1), (9, 0), (10, 0)],
    }
    n = 0
    for name, cases in bad.items():
        for pos, value in cases:
            args = list(good[name])
            args[pos] = value
            with pytest.raises(RuntimeError, match=name):
                lib.call(name, *args)
            n += 1
    torch.cuda.synchronize()
    assert n == 62
    for buf, fill in ((xbuf, SENT), (pbuf, SENT), (sbuf, SENT), (wbuf, float('nan')), (cbuf, float('nan')), (rbuf, float('nan')),
                      (bbuf, float('nan')), (mbuf, float('nan'))):
        assert tail_intact(buf, 0, fill)
