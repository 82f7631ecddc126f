"""GPU: the ensemble and the multi-view entry points of csrc/group_ops.hip are one decide kernel and one combine kernel.  Fed the same
inputs, spaa_decide_ens / spaa_decide_views and spaa_ens_combine / spaa_views_combine give the same bits."""
import numpy as np
import pytest
import torch

from test_multiview_ops_gpu import P_THRESH, _dev, _tables, decide_case, lib  # noqa: F401  (lib: module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _decide(lib, name, c, G, focus, row):
    """spaa_decide_views (row 4: the case's first loss table for every view, adv_scale 1) or spaa_decide_ens (row 2: that table once)
    on the case's G logits; outputs prefilled with sentinels."""
    B, ncls = c['B'], c['ncls']
    lg = [_dev(a) for a in c['logits']]
    table = _dev(c['partial'][0])
    out = dict(state=torch.full((B, 4), -7, dtype=torch.int32, device=DEV), stats=torch.full((B, 8), -7.0, device=DEV),
               grp_state=torch.full((B, G, 2), -7, dtype=torch.int32, device=DEV), grp_stats=torch.full((B, G, row), -7.0, device=DEV),
               w=torch.full((B, G), -7.0, device=DEV), seeds=[torch.full((B, ncls), -7.0, device=DEV) for _ in range(G)])
    out['stats'][:, 5] = _dev(c['col_best'])
    p = lib.ptr
    target, prjl2, params, flags = _tables(c)
    tail = (p(out['state']), p(out['stats']), p(out['grp_state']), p(out['grp_stats']), p(out['w']), lib.ptr_array(out['seeds']), B)
    if name == 'spaa_decide_views':
        lib.call(name, lib.ptr_array(lg), G, ncls, p(target), lib.ptr_array([table] * G), c['nblk'], c['HW'], p(prjl2), p(params), p(flags),
                 P_THRESH, 1.0, int(focus), *tail)
    else:
        lib.call(name, lib.ptr_array(lg), G, ncls, p(target), p(table), c['nblk'], c['HW'], p(prjl2), p(params), p(flags), P_THRESH,
                 int(focus), *tail)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('focus', [False, True])
@pytest.mark.parametrize('ncls', [10, 1000])        # (10: 246 lanes without a candidate; 1000: no multiple of 256)
@pytest.mark.parametrize('G', [2, 4])               # (not 3: (3 m) / 3 need not round back to m)
def test_decide_views_on_one_image_is_decide_ens_bitwise(lib, G, ncls, focus):
    c = decide_case(G, ncls, 3120, seed=31 * G + ncls)
    v = _decide(lib, 'spaa_decide_views', c, G, focus, 4)
    e = _decide(lib, 'spaa_decide_ens', c, G, focus, 2)
    assert torch.equal(v['state'], e['state']) and torch.equal(v['stats'][:, 0:7], e['stats'][:, 0:7])
    assert torch.equal(v['w'], e['w']) and all(torch.equal(a, b) for a, b in zip(v['seeds'], e['seeds']))
    assert torch.equal(v['grp_state'], e['grp_state']) and torch.equal(v['grp_stats'][..., :2], e['grp_stats'])
    # every view's means are the one image's, and so is their mean over G
    assert torch.equal(v['grp_stats'][..., 2:4], v['stats'][:, None, 1:3].expand(c['B'], G, 2))
    # the case is not a trivial one: members disagree, and with focus some rest
    assert v['state'][:, 3].tolist() == [1, G, G - 1, G] and (v['w'] == 0).any().item() == bool(focus)


@pytest.mark.parametrize('HW', [1, 255, 257])
@pytest.mark.parametrize('G', [2, 4])
def test_views_combine_off_the_colour_step_is_ens_combine_bitwise(lib, G, HW):
    rng = np.random.default_rng(100 * G + HW)
    B, nblk = 3, (HW + 255) // 256
    gs = [rng.standard_normal((B, HW, 4)).astype(np.float32) for _ in range(G)]
    gs[1][0, :, :3] = 0.0                                # (sample 0's member 1: zero norm)
    w = rng.uniform(0.5, 1.5, (B, G)).astype(np.float32)
    w[2, 0] = 0.0
    state = np.array([[1, 0, 1, 3], [0, 0, 0, 0], [1, 0, 0, 2]], dtype=np.int32)     # (column 1 all 0: no sample on the colour step)
    g_dev, w_dev, state_dev = [_dev(g) for g in gs], _dev(w), _dev(state, torch.int32)
    arr = lib.ptr_array(g_dev)
    partial = torch.zeros(B, G, nblk, device=DEV)
    out_v, out_e = torch.full((B, HW, 4), -7.0, device=DEV), torch.full((B, HW, 4), 7.0, device=DEV)
    lib.call('spaa_ens_sumsq', arr, G, lib.ptr(partial), B, HW)
    lib.call('spaa_views_combine', arr, G, lib.ptr(partial), nblk, lib.ptr(w_dev), lib.ptr(state_dev), lib.ptr(out_v), B, HW)
    lib.call('spaa_ens_combine', arr, G, lib.ptr(partial), nblk, lib.ptr(w_dev), lib.ptr(out_e), B, HW)
    torch.cuda.synchronize()
    assert torch.equal(out_v, out_e) and (out_v[..., 3] == 0).all() and (out_v[..., :3] != 0).any(dim=2).all()
