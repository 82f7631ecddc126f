"""CPU: which kernel every ConvPlan launch gets, pinned against tests/golden/convplan_launches.json.

`ConvPlan.run`, `ConvPlan.wgrad` and `SmallLinearPlan.run` are driven on CPU tensors with `_lib.call`, `_lib.check_dev` and
`_lib.check_mask` replaced by stubs: nothing is computed, the stub keeps what WOULD have been launched -- the entry points in order,
every field of the `TapConv` descriptor (pointers as the name of the tensor they point at), the workspaces, the `last_*` attributes,
the profile record, the exception.  The fixture keeps a record without its zero / null entries (`compact`).  It was written by
tests/golden/make_golden_convplan_launches.py from the convplan.py named in its `commit` entry; it carries its own tune table, so
an edit of tapconv_tune.json does not move it.  The two host-side launcher-plan queries (spaa_tapconv_wino_plan,
spaa_tapconv_h16p_plan) are the library's own, as in tests/test_cabi_cpu.py.
"""
import ctypes as C
import json
import os

import pytest
import torch

from spaa_amd import _lib
from spaa_amd import convplan as cp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'convplan_launches.json')
SWITCHES = dict(FORCE_TILE=0, DEFAULT_DISABLE={''}, WINO_SPLITK_FIXUP=False, H16P_CV=(0, 0, 0), FORCE_KSPLIT=0, X6P_STD=True, WINOGRAD=True,
                WINO_SPLITK=True, H16P_LEAN_WIDE=2, DEBUG_TAPMAJOR=0, DEBUG_PERSIST_CAP=0, DEBUG_WINO=0, DEBUG_WINO_NOCANVAS=0, DEBUG_THINMF=0,
                DEBUG_SMALLCIN_NOSLAB=0, DEBUG_H16_2STAGE=0, SMALL_LINEAR=True, PROFILE=None, PROFILE_ONLY=None)
ATTRS = ('last_tile', 'last_ksplit', 'last_wino_plan', 'last_h16p_plan', 'last_pool_fused', 'last_unpool_fused')
F16, F32 = 'f16', 'f32'


def case(name, plan, b, hw, src=F32, dst=None, ops=(), sw=None, tune=None, out_hw=None, attach=None, op='run', profile=False, **kw):
    return dict(name=name, plan=plan, b=b, hw=hw, src=src, dst=dst or src, ops=ops, sw=sw or {}, tune=tune or {}, out_hw=out_hw,
                attach=attach, op=op, profile=profile, kw=kw)


# plan = (builder, Cin, Cout, kernel, stride, pad[, fold]); b, hw = batch and size of `inp`; ops = the optional operands present;
# sw = module switches of the call; tune = the tune table of the call (key `Cin_Cout_taps_sin_sout_M[_fold]` -> tile + 100 k)
CASES = [
    # register-staged and DMA-staged tiles
    case('default_16', ('conv', 20, 24, 3, 1, 1), 2, (8, 8)),
    case('default_18', ('conv', 20, 40, 3, 1, 1), 2, (8, 8)),
    case('tuned_22_stem', ('conv', 3, 64, 7, 2, 3), 8, (16, 32), tune={'4_64_49_2_1_1024': 22}),
    case('default_29', ('dgrad', 3, 32, 3, 1, 1), 2, (8, 8), sw=dict(DEFAULT_DISABLE={'thinmf'})),
    case('f16in_thin_29', ('dgrad', 3, 32, 3, 1, 1), 2, (8, 8), src=F16, dst=F32, sw=dict(DEFAULT_DISABLE={'thinmf'})),
    case('default_38', ('conv', 3, 32, 3, 1, 1), 2, (8, 8)),
    case('f32in_f16out_38', ('conv', 6, 32, 3, 1, 1), 2, (8, 8), dst=F16, tune={'8_32_9_1_1_128': 34}),
    case('f32in_f16out_16', ('conv', 32, 24, 3, 1, 1), 2, (8, 8), dst=F16),
    case('f32in_f16out_18', ('conv', 32, 40, 3, 1, 1), 2, (8, 8), dst=F16),
    case('default_34', ('conv', 32, 128, 1, 1, 0), 512, (8, 8)),
    case('default_36', ('conv', 32, 64, 1, 1, 0), 512, (8, 8)),
    case('default_37', ('conv', 32, 32, 1, 1, 0), 512, (8, 8)),
    case('default_34_splitk2', ('conv', 64, 128, 3, 1, 1), 200, (8, 16)),
    case('default_34_splitk4', ('conv', 128, 128, 3, 1, 1), 4, (8, 16)),
    case('tuned_splitk3', ('conv', 64, 96, 3, 1, 1), 4, (8, 16), tune={'64_96_9_1_1_512': 336}),
    case('tuned_splitk_refused', ('conv', 32, 96, 1, 1, 0), 4, (8, 16), tune={'32_96_1_1_1_512': 234}),
    case('streamk_51', ('conv', 256, 256, 3, 1, 1), 2, (7, 7), tune={'256_256_9_1_1_98': 951}, sw=dict(WINOGRAD=False)),
    case('streamk_refused', ('conv', 64, 96, 3, 1, 1), 4, (8, 16), tune={'64_96_9_1_1_512': 936}),
    case('fold_to_34', ('deconv', 32, 8, 2, 2, 0), 2, (8, 8), tune={'32_8_1_1_2_128_fold': 22}),
    case('fold_default', ('deconv', 32, 8, 2, 2, 0), 2, (8, 8)),
    case('fold_on_68', ('deconv', 64, 32, 3, 2, 1, True), 256, (16, 32), src=F16),
    # fp16 implicit-GEMM tiles
    case('h16_60', ('conv', 64, 128, 1, 1, 0), 512, (8, 16), src=F16),
    case('h16_60_to_61_few_tiles', ('conv', 64, 128, 1, 1, 0), 2, (8, 16), src=F16, sw=dict(DEFAULT_DISABLE={'h16splitk'})),
    case('h16_60_to_61_waste', ('conv', 64, 192, 1, 1, 0), 300, (8, 16), src=F16),
    case('h16_60_kept_n64_off', ('conv', 64, 128, 1, 1, 0), 2, (8, 16), src=F16, sw=dict(DEFAULT_DISABLE={'h16n64', 'h16splitk'})),
    case('h16_61', ('conv', 64, 64, 1, 1, 0), 2, (8, 16), src=F16),
    case('h16_62', ('conv', 64, 32, 1, 1, 0), 2, (8, 16), src=F16),
    case('h16_63', ('conv', 64, 16, 1, 1, 0), 2, (8, 16), src=F16),
    case('h16_splitk_rule', ('conv', 256, 32, 3, 1, 1), 2, (8, 8), src=F16),
    case('h16_splitk_forced', ('conv', 256, 128, 1, 1, 0), 2, (8, 16), src=F16, sw=dict(FORCE_TILE=60, FORCE_KSPLIT=2)),
    # tile 68
    case('h16p_s1', ('conv', 64, 64, 3, 1, 1), 256, (16, 32), src=F16),
    case('h16p_s2_fwd', ('conv', 64, 128, 3, 2, 1), 192, (16, 64), src=F16),     # (8 x 32 outputs: one full tile of the stride-2 form)
    case('h16p_s2_fwd_forced', ('conv', 64, 128, 3, 2, 1), 2, (16, 32), src=F16, sw=dict(FORCE_TILE=68)),
    case('h16p_canvas', ('conv', 256, 256, 3, 1, 1), 64, (14, 14), src=F16),
    case('h16p_canvas_fixup', ('conv', 256, 256, 3, 1, 1), 64, (14, 14), src=F16, sw=dict(WINO_SPLITK_FIXUP=True)),
    case('h16p_canvas_cv', ('conv', 128, 128, 3, 1, 1), 8, (14, 14), src=F16, sw=dict(H16P_CV=(64, 2, 1))),
    case('h16p_lean_wide', ('conv', 128, 128, 3, 1, 1), 256, (16, 32), src=F16),
    case('h16p_lean_wide_off', ('conv', 288, 128, 3, 1, 1), 256, (16, 32), src=F16),
    case('h16p_lean_bit16', ('conv', 64, 64, 3, 1, 1), 256, (16, 32), src=F16, sw=dict(DEFAULT_DISABLE={'h16plean'})),
    case('h16p_pool_fused', ('conv', 64, 64, 3, 1, 1), 256, (16, 32), src=F16, ops=('pool',), act=_lib.ACT_RELU),
    case('h16p_pool_unfused', ('conv', 64, 64, 3, 1, 1), 256, (16, 32), src=F16, ops=('pool',), act=_lib.ACT_RELU, sw=dict(DEFAULT_DISABLE={'h16ppool'})),
    case('f32_pool_unfused', ('conv', 32, 64, 3, 1, 1), 2, (8, 8), ops=('pool',), act=_lib.ACT_RELU),
    case('h16p_unpool_fused', ('dgrad', 64, 64, 3, 1, 1), 256, (8, 16), src=F16, ops=('unpool',)),
    case('h16p_unpool_unfused', ('dgrad', 64, 64, 3, 1, 1), 256, (8, 16), src=F16, ops=('unpool',), sw=dict(DEFAULT_DISABLE={'h16punp'})),
    case('h16p_second_source', ('deconv', 64, 32, 3, 2, 1, True), 2, (8, 8), src=F16, ops=('inp2',), attach=('h16', 32)),
    case('h16_second_source_missing', ('deconv', 64, 32, 3, 2, 1, True), 2, (8, 8), src=F16, ops=('inp2',)),
    # Winograd tiles
    case('wino_73_pad1', ('conv', 64, 64, 3, 1, 1), 64, (14, 14), tune={'64_64_9_1_1_12544': 73}),
    case('wino_70_pad0', ('conv', 64, 64, 3, 1, 0), 8, (16, 32), out_hw=(14, 30), tune={'64_64_9_1_1_3360': 70}),
    case('wino_71_pad2', ('dgrad', 64, 64, 3, 1, 0), 8, (14, 30), out_hw=(16, 32), tune={'64_64_9_1_1_4096': 71}),
    case('wino_70_kranges', ('conv', 256, 256, 3, 1, 1), 64, (7, 7), tune={'256_256_9_1_1_3136': 70}),
    case('wino_70_kranges_fixup', ('conv', 256, 256, 3, 1, 1), 64, (7, 7), tune={'256_256_9_1_1_3136': 70}, sw=dict(WINO_SPLITK_FIXUP=True)),
    case('wino_tuned_k4', ('conv', 256, 256, 3, 1, 1), 64, (7, 7), tune={'256_256_9_1_1_3136': 470}),
    case('wino_no_splitk', ('conv', 256, 256, 3, 1, 1), 64, (7, 7), tune={'256_256_9_1_1_3136': 70}, sw=dict(WINO_SPLITK=False)),
    case('wino_2src_f32', ('conv2src', 64, 64, 64), 2, (8, 8), ops=('inp2',)),
    case('wino_2src_f16', ('conv2src', 64, 64, 64), 2, (8, 8), src=F16, ops=('inp2',)),
    case('wino_2src_no_inp2', ('conv2src', 64, 64, 64), 2, (8, 8)),
    case('wino_2src_size_mismatch', ('conv2src', 64, 64, 64), 2, (8, 8), ops=('inp2',), out_hw=(6, 6)),
    case('wino_size_mismatch', ('conv', 64, 64, 3, 1, 1), 8, (16, 32), out_hw=(14, 30), tune={'64_64_9_1_1_3360': 70}),
    case('wino_off', ('conv', 64, 64, 3, 1, 1), 8, (16, 32), tune={'64_64_9_1_1_4096': 70}, sw=dict(WINOGRAD=False)),
    case('wino_default_big', ('conv', 64, 256, 3, 1, 1), 98, (16, 32)),
    case('wino_epilogue', ('conv', 64, 64, 3, 1, 1), 8, (16, 32), ops=('add', 'gate', 'aux_out', 'gate2', 'mask_out'), tune={'64_64_9_1_1_4096': 73},
         act=_lib.ACT_RELU, gate_mode=_lib.GATE_POS_LE1),
    # tile 72
    case('thinmf_f32_s2', ('dgrad', 3, 64, 7, 2, 3), 2, (8, 16), out_hw=(16, 32)),
    case('thinmf_f16', ('dgrad', 3, 64, 3, 1, 1), 2, (8, 16), src=F16, dst=F32),
    case('thinmf_f32_s1_not_taken', ('dgrad', 3, 64, 3, 1, 1), 2, (8, 16)),
    case('thinmf_forced_s1', ('dgrad', 3, 64, 3, 1, 1), 2, (8, 16), sw=dict(FORCE_TILE=72)),
    case('thinmf_pool_adjoint', ('dgrad', 3, 64, 7, 2, 3), 2, (4, 8), ops=('pool_adjoint',), pa_hw=(8, 16), out_hw=(16, 32)),
    case('pool_adjoint_other_tile', ('dgrad', 3, 64, 7, 2, 3), 2, (4, 8), ops=('pool_adjoint',), pa_hw=(8, 16), out_hw=(16, 32),
         sw=dict(DEFAULT_DISABLE={'thinmf'})),
    case('pool_adjoint_bad_operands', ('dgrad', 3, 64, 7, 2, 3), 2, (4, 8), ops=('pool_adjoint',), pa_hw=(9, 16), out_hw=(16, 32)),
    # tile 74
    case('x6p_canonical', ('deconv', 64, 32, 3, 2, 1), 2, (8, 16), tune={'64_32_9_1_2_256': 74}),
    case('x6p_noncanonical', ('deconv', 64, 32, 4, 2, 0), 2, (7, 15), out_hw=(16, 32), tune={'64_32_16_1_2_256': 74}),
    case('x6p_std_off', ('deconv', 64, 32, 3, 2, 1), 2, (8, 16), tune={'64_32_9_1_2_256': 74}, sw=dict(X6P_STD=False)),
    case('x6p_second_source', ('deconv', 64, 32, 3, 2, 1), 2, (8, 16), ops=('inp2',), attach=('x6p', 32)),
    case('x6p_second_source_missing', ('deconv', 64, 32, 3, 2, 1), 2, (8, 16), ops=('inp2',)),
    case('x6p_not_ok', ('deconv', 64, 32, 2, 2, 0, False), 2, (8, 16), tune={'64_32_4_1_2_256': 74}),
    case('x6p_not_ok_forced', ('deconv', 64, 32, 2, 2, 0, False), 2, (8, 16), sw=dict(FORCE_TILE=74)),
    # tile 76
    case('c3_f32', ('conv', 3, 64, 3, 1, 1), 2, (8, 8), tune={'4_64_9_1_1_128': 76}),
    case('c3_f16out', ('conv', 3, 64, 3, 1, 1), 2, (8, 8), dst=F16),
    case('c3_off', ('conv', 3, 64, 3, 1, 1), 2, (8, 8), dst=F16, tune={'4_64_9_1_1_128': 76}, sw=dict(DEFAULT_DISABLE={'c3'})),
    case('c3h_off', ('conv', 3, 64, 3, 1, 1), 2, (8, 8), dst=F16, tune={'4_64_9_1_1_128': 76}, sw=dict(DEFAULT_DISABLE={'c3h'})),
    case('c3_tuned_on_non_image', ('conv', 4, 64, 3, 1, 1), 2, (8, 8), tune={'4_64_9_1_1_128': 76}),
    case('c3_fixed_on_non_image', ('conv', 4, 64, 3, 1, 1), 2, (8, 8), fixed_tile=76),
    # forced tiles: eligible, then falling back to 0
    case('force_9', ('conv', 32, 4, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=9, DEFAULT_DISABLE={'thinmf'})),
    case('force_9_off', ('conv', 32, 8, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=9)),
    case('force_10', ('conv', 32, 32, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=10)),
    case('force_10_off', ('conv', 64, 32, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=10)),
    case('force_11', ('conv', 32, 4, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=11)),
    case('force_11_off', ('conv', 48, 4, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=11)),
    case('force_38', ('conv', 3, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=38)),
    case('force_38_off', ('conv', 32, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=38)),
    case('force_76', ('conv', 3, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=76)),
    case('force_76_off', ('conv', 32, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=76)),
    case('force_28', ('conv', 32, 4, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=28)),
    case('force_28_off', ('conv', 16, 4, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=28)),
    case('force_47', ('conv', 16, 4, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=47)),
    case('force_29_off', ('conv', 16, 8, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=29)),
    case('force_x6d', ('conv', 32, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=48)),
    case('force_x6d_off', ('conv', 20, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=48)),
    case('force_h16', ('conv', 64, 64, 3, 1, 1), 2, (8, 8), src=F16, sw=dict(FORCE_TILE=64)),
    case('force_h16_off', ('conv', 64, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=64)),
    case('force_68', ('conv', 64, 64, 3, 1, 1), 2, (8, 8), src=F16, sw=dict(FORCE_TILE=68)),
    case('force_68_off', ('conv', 64, 64, 3, 1, 1), 2, (8, 8), sw=dict(FORCE_TILE=68)),
    case('force_68_not_patch', ('conv', 64, 64, 1, 1, 0), 2, (8, 8), src=F16, sw=dict(FORCE_TILE=68)),
    case('force_70_mismatch', ('conv', 64, 64, 3, 1, 1), 2, (8, 8), out_hw=(6, 6), sw=dict(FORCE_TILE=70)),
    # epilogue reroutes
    case('gate_mul_reroute', ('conv', 32, 40, 3, 1, 1), 2, (8, 8), ops=('gate',), gate_mode=_lib.GATE_MUL, tune={'32_40_9_1_1_128': 22}),
    case('gate_mul_error', ('conv', 20, 40, 3, 1, 1), 2, (8, 8), ops=('gate',), gate_mode=_lib.GATE_MUL),
    case('mask_reroute', ('conv', 32, 40, 3, 1, 1), 2, (8, 8), ops=('mask_out',), tune={'32_40_9_1_1_128': 4}),
    case('mask_reroute_splitk', ('conv', 64, 128, 3, 1, 1), 4, (8, 16), ops=('gate_bits', 'aux_out', 'gate2_bits'), tune={'64_128_9_1_1_512': 204}),
    case('mask_error', ('dgrad', 3, 32, 3, 1, 1), 2, (8, 8), ops=('mask_out',)),
    case('dtype_mismatch', ('conv', 32, 40, 3, 1, 1), 2, (8, 8), dst=F16, ops=('add',), add_dtype=F32),
    case('f16in_needs_cin32', ('conv', 20, 40, 3, 1, 1), 2, (8, 8), src=F16),
    case('coff_windows', ('conv', 32, 40, 3, 1, 1), 2, (8, 8), ops=('add', 'gate'), cs_in=48, cs_out=64, in_coff=8, out_coff=12, add_coff=4,
         gate_coff=8, act=_lib.ACT_LEAKY01),
    # linear layers
    case('linear_small_75', ('linear', 16, 12), 3, (1, 1)),
    case('linear_wrapped', ('linear', 16, 12), 3, (1, 1), act=_lib.ACT_RELU),
    case('linear_dgrad_rows', ('linear_dgrad', 16, 12), 80, (1, 1)),
    # bench.py's instrumented pass
    case('profile_wino', ('conv', 256, 256, 3, 1, 1), 64, (7, 7), tune={'256_256_9_1_1_3136': 70}, profile=True),
    case('profile_h16p_cv', ('conv', 256, 256, 3, 1, 1), 64, (14, 14), src=F16, profile=True, ops=('add', 'mask_out')),
    case('profile_streamk', ('conv', 256, 256, 3, 1, 1), 2, (7, 7), tune={'256_256_9_1_1_98': 951}, sw=dict(WINOGRAD=False), profile=True),
    case('profile_pool_fused', ('conv', 64, 64, 3, 1, 1), 256, (16, 32), src=F16, ops=('pool',), act=_lib.ACT_RELU, profile=True),
    case('profile_unpool_fused', ('dgrad', 64, 64, 3, 1, 1), 256, (8, 16), src=F16, ops=('unpool',), profile=True),
    case('profile_second_source', ('deconv', 64, 32, 3, 2, 1), 2, (8, 16), ops=('inp2',), attach=('x6p', 32), profile=True),
    case('profile_2src', ('conv2src', 64, 64, 64), 2, (8, 8), ops=('inp2',), profile=True),
    case('profile_only_skips', ('conv', 32, 64, 1, 1, 0), 512, (8, 8), profile=True, sw=dict(PROFILE_ONLY={70})),
    # weight gradient
    case('wgrad_conv', ('conv', 32, 40, 3, 1, 1), 2, (8, 8), op='wgrad'),
    case('wgrad_four_classes', ('deconv', 64, 32, 3, 2, 1, False), 2, (8, 16), op='wgrad'),
]
CASE_BY_NAME = {c['name']: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# the coverage the fixture must show: (tile, sign of ksplit, reserved1) of a launch; messages raised
_CV64 = _lib.H16P_CV | 1 << _lib.H16P_CV_BN_SHIFT    # tile 68's canvas / K-range form on the 64-wide N tile
WANT_OUTCOMES = {(16, 0, 0), (18, 0, 0), (22, 0, 0), (29, 0, 0), (38, 0, 0), (34, 0, 0), (36, 0, 0), (37, 0, 0), (34, 1, 0), (36, 1, 0), (51, -1, 0),
                 (60, 0, 0), (61, 0, 0), (62, 0, 0), (63, 0, 0), (60, 1, 0), (68, 0, 0), (68, 1, _CV64), (68, 1, _CV64 | _lib.SPLITK_FIXUP),
                 (68, 0, _lib.H16P_LEAN_WIDE), (68, 0, _lib.H16P_ONE_WG), (68, 0, _lib.H16P_POOL), (68, 0, _lib.H16P_UNPOOL), (70, 1, 0),
                 (70, 1, _lib.SPLITK_FIXUP), (71, 0, 0), (73, 0, 0), (72, 0, 0), (74, 0, 0), (76, 0, 0), (76, 0, _lib.C3_F16_OPERANDS), (0, 0, 0)}
WANT_RAISES = {'must have the storage type of `out`', 'pool_adjoint needs fp32 tensors', 'a two-source plan needs `inp2`',
               'fp16-storage input needs Cin % 32 == 0', 'GATE_MUL needs a layer shape served by the DMA-staged kernels',
               'gate masks need a layer shape served by the bf16x6 / smallcin kernels', 'tile 76 serves 3-channel-image convolutions only',
               'a two-source plan runs on the Winograd kernel', 'an fp16 second source needs attach_second_source_h16()',
               'a second source needs attach_second_source()', 'pool_adjoint is served by the thin-output matrix-core kernel only'}


def build_plan(spec, attach=None):
    kind, a = spec[0], spec[1:]
    if kind in ('linear', 'linear_dgrad'):
        ci, co = a
        w = torch.zeros(co, ci)
        plan = cp.linear_fwd_plan(w, torch.zeros(co), device='cpu', name=kind) if kind == 'linear' else cp.linear_dgrad_plan(w, device='cpu', name=kind)
    elif kind == 'conv2src':
        ca, cb, co = a
        plan = cp.conv_fwd_plan_2src(torch.zeros(co, ca, 3, 3), torch.zeros(co, cb, 3, 3), torch.zeros(co), device='cpu', name=kind)
    else:
        ci, co, k, s, p = a[:5]
        fold = a[5] if len(a) > 5 else None
        if kind == 'conv':
            plan = cp.conv_fwd_plan(torch.zeros(co, ci, k, k), torch.zeros(co), s, p, device='cpu', name=kind)
        elif kind == 'dgrad':      # input gradient of conv ci -> co: reads co channels, writes ci
            plan = cp.conv_dgrad_plan(torch.zeros(co, ci, k, k), s, p, device='cpu', name=kind, fold=fold)
        else:
            assert kind == 'deconv'
            plan = cp.deconv_fwd_plan(torch.zeros(ci, co, k, k), torch.zeros(co), s, p, device='cpu', name=kind, fold=fold)
    if attach is not None:
        how, cin2 = attach
        w2, b2 = torch.zeros(plan.cout, cin2), torch.zeros(plan.cout)
        plan.attach_second_source(w2, b2) if how == 'x6p' else plan.attach_second_source_h16(w2, b2)
    return plan


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


def plan_tensors(plan, prefix=''):
    p = getattr(plan, 'conv', plan)
    names = {k: getattr(p, k, None) for k in ('weights', 'w_split', 'w_half', 'taps', 'bias', 'bias2', 'w2_split', 'w2_half')}
    names.update(c3=getattr(p, '_c3', None), c3h=getattr(p, '_c3h', None), thin_s=p._thin.get('s'), thin_h=p._thin.get('h'), ws=p._ws, ws_fix=p._ws_fix)
    out = {prefix + k: v for k, v in names.items() if v is not None}
    if prefix == '':
        out.update({'streamk': v for v in cp._STREAMK_WS.values()})
        if p.wino is not None:
            out.update(plan_tensors(p.wino, 'wino.'))
    return out


def describe(d, tensors):
    """Every field of a TapConv descriptor: scalars as they are, pointers as the name of the tensor they point at."""
    by_ptr = {}
    for k, v in tensors.items():
        by_ptr.setdefault(v.data_ptr(), k)
    rec = {}
    for f, t in _lib.TapConv._fields_:
        v = getattr(d, f)
        if t is C.c_void_p:
            assert v is None or v in by_ptr, f'descriptor field {f}: pointer to no known tensor'
            rec[f] = 'null' if v is None else by_ptr[v]
        elif f == 'tap_range':
            rec[f] = list(v)
        elif f == 'cls':
            rec[f] = [{n: getattr(c, n) for n, _ in _lib.TapClass._fields_} for c in v]
        else:
            rec[f] = v
    return rec


def operands(c, plan):
    p = getattr(plan, 'conv', plan)
    kw, b, (h, w) = dict(c['kw']), c['b'], c['hw']
    dt = {F16: torch.float16, F32: torch.float32}
    cs_in, cs_out = kw.pop('cs_in', p.cin_p - getattr(p, 'cin2_k', 0)), kw.pop('cs_out', (p.cout + 3) // 4 * 4)
    t = dict(inp=torch.zeros(b, h, w, cs_in, dtype=dt[c['src']]))
    gh, gw = kw.pop('pa_hw', (2 * h, 2 * w) if 'unpool' in c['ops'] else (h, w))     # the layer's input grid
    ho, wo = c['out_hw'] or ((gh * p.s_out, gw * p.s_out) if p.s_in == 1 else ((gh + 1) // 2, (gw + 1) // 2))
    t['out'] = torch.zeros(b, ho, wo, cs_out, dtype=dt[c['dst']])
    add_dtype = dt[kw.pop('add_dtype', c['dst'])]
    for o in c['ops']:
        if o in ('add', 'gate', 'aux_out', 'gate2'):
            t[o] = torch.zeros(b, ho, wo, cs_out, dtype=add_dtype)
        elif o in ('mask_out', 'gate_bits', 'gate2_bits'):
            t[o] = torch.zeros(b, ho, wo, cs_out // 4, dtype=torch.uint8)
        elif o == 'inp2':
            t[o] = (torch.zeros(b, h, w, p.cin2_k, dtype=dt[c['src']]) if getattr(p, 'cin2_k', 0)
                    else torch.zeros(b, ho, wo, getattr(p, 'cin2', 32), dtype=dt[c['src']]))
        elif o == 'pool':
            t['pooled'], t['parg'] = torch.zeros(b, ho // 2, wo // 2, cs_out, dtype=dt[c['dst']]), torch.zeros(b, ho // 2, wo // 2, p.cout, dtype=torch.uint8)
        elif o == 'unpool':
            t['parg'], t['gfull'] = torch.zeros(b, h, w, cs_in, dtype=torch.uint8), torch.zeros(b, 2 * h, 2 * w, cs_in, dtype=dt[c['src']])
        elif o == 'pool_adjoint':
            t['parg'] = torch.zeros(b, h, w, cs_in, dtype=torch.uint8)
    args = {k: t[k] for k in ('add', 'gate', 'aux_out', 'gate2', 'mask_out', 'gate_bits', 'gate2_bits', 'inp2') if k in t}
    if 'pool' in c['ops']:
        args['pool'] = (t['pooled'], t['parg'], True)
    if 'unpool' in c['ops']:
        args['unpool'] = (t['parg'], t['gfull'])
    if 'pool_adjoint' in c['ops']:
        args['pool_adjoint'] = (t['parg'], (gh, gw), True)
    fixed = kw.pop('fixed_tile', 0)
    if fixed:
        p.fixed_tile = fixed
    args.update(kw)
    return t, args


def run_case(c, tune, patch):
    """One case of the table with the launches stubbed: the record the fixture keeps."""
    for k, v in {**SWITCHES, **c['sw']}.items():
        patch(cp, k, set(v) if isinstance(v, (set, list)) else v)
    patch(cp, 'TUNE', dict(tune))
    patch(cp, '_NEAREST', {})
    patch(_lib, 'check_dev', lambda *a, **k: None)
    patch(_lib, 'check_mask', lambda *a, **k: None)
    rec = dict(calls=[])
    plan = build_plan(c['plan'], c['attach'])
    tensors, args = operands(c, plan)

    def call(name, *a):
        if name in ('spaa_tapconv_f32', 'spaa_tapconv_wgrad'):
            r = dict(entry=name, desc=describe(a[0]._obj, {**plan_tensors(plan), **tensors}))
            if name == 'spaa_tapconv_wgrad':
                r['nchunk'] = a[-1]
        else:
            r = dict(entry=name, ints=[x for x in a if isinstance(x, int)])
        rec['calls'].append(r)

    patch(_lib, 'call', call)
    if c['profile']:
        patch(cp, 'PROFILE', [])
        patch(torch.cuda, 'Event', _Event)
    try:
        if c['op'] == 'wgrad':
            dw, db = plan.wgrad(tensors['inp'], tensors['out'])
            rec['dw'], rec['db'] = dw.numel(), db.numel()
        else:
            assert plan.run(tensors['inp'], tensors['out'], **args) is tensors['out']
    except (ValueError, RuntimeError) as e:
        rec['raises'] = [type(e).__name__, str(e)]
    rec['ws'] = {k: v.numel() for k, v in plan_tensors(plan).items() if k.split('.')[-1] in ('ws', 'ws_fix')}
    rec['attrs'] = {pre + a: (list(v) if isinstance(v, tuple) else v) for pre, p in (('', plan), ('wino.', getattr(getattr(plan, 'conv', plan), 'wino', None)))
                    if p is not None for a in ATTRS for v in [p.__dict__.get(a, 'absent')]}
    if c['profile']:
        rec['profile'] = [[r[0], r[1], r[2], r[5], r[6]] for r in cp.PROFILE]
    return rec


REFRESH = {'wino': ((64, 32, 3, 3), 1, 'fwd'), 'c3': ((64, 3, 3, 3), 1, 'fwd'), 'thin': ((32, 3, 3, 3), 2, 'dgrad')}


def packed_layouts(plan):
    """Every lazily packed layout this plan can have, packed now (name -> tensor)."""
    out = dict(w_half=plan.half_plane()) if plan.cin_p % 32 == 0 else {}
    if plan.c3_ok():
        out.update(c3=plan.c3_pack(), c3h=plan.c3_pack(True))
    if plan.thin_ok():
        out.update(thin_s=plan.thin_fold(False), thin_h=plan.thin_fold(True))
    return out


def refresh_case(kind, patch):
    """`refresh` on a plan whose lazily packed layouts are really packed (`wino` + `w_half`; `_c3` / `_c3h` of a first layer; `_thin`
    of a thin input gradient), and the plan built freshly from the new parameter."""
    patch(cp, 'TUNE', {})
    shape, stride, how = REFRESH[kind]
    g = torch.Generator().manual_seed(5)
    w0, w1 = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    b0, b1 = (torch.randn(shape[0], generator=g), torch.randn(shape[0], generator=g)) if how == 'fwd' else (None, None)

    def builder(w, b=b0):
        return cp.conv_fwd_plan(w, b, stride, 1, device='cpu') if how == 'fwd' else cp.conv_dgrad_plan(w, stride, 1, device='cpu')

    plan = cp.attach_maps(builder(w0), builder, w0)
    stale = packed_layouts(plan)
    plan.refresh(w1, b1)
    return plan, builder(w1, b1), stale


def compact(rec):
    """The record of `run_case` as the fixture keeps it: without the descriptor fields that are zero / null, the all-zero classes
    past the last used one and the attributes that are absent.  Nothing is lost: what a record leaves out HAS that value, and the
    comparison runs over the fields of both records."""
    out = dict(rec, attrs={k: v for k, v in rec['attrs'].items() if v != 'absent'}, calls=[])
    for r in rec['calls']:
        r = dict(r)
        if 'desc' in r:
            d = {k: v for k, v in r['desc'].items() if v not in (0, 'null', [0, 0, 0, 0])}
            d['cls'] = [{k: v for k, v in c.items() if v} for c in d['cls']]
            while d['cls'] and not d['cls'][-1]:
                d['cls'].pop()
            r['desc'] = d
        out['calls'].append(r)
    return out


FIXTURE = {}
if os.path.exists(GOLDEN):    # (absent only while make_golden_convplan_launches.py writes it)
    with open(GOLDEN) as _fh:
        FIXTURE = json.load(_fh)


def _diff(path, got, want, out):
    if isinstance(want, dict) and isinstance(got, dict):
        for k in sorted(set(want) | set(got)):
            _diff(f'{path}.{k}', got.get(k, '<missing>'), want.get(k, '<missing>'), out)
    elif isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        for i, (g, w) in enumerate(zip(got, want)):
            _diff(f'{path}[{i}]', g, w, out)
    elif got != want:
        out.append(f'{path}: got {got!r}, fixture {want!r}')


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_launch_matches_fixture(name, monkeypatch):
    want = FIXTURE['cases'][name]
    got = json.loads(json.dumps(compact(run_case(CASE_BY_NAME[name], want['tune'], monkeypatch.setattr))))
    bad = []
    _diff(name, got, {k: v for k, v in want.items() if k != 'tune'}, bad)
    assert not bad, '\n'.join(bad)


def test_fixture_covers_every_route():
    """The fixture holds every case of the table and nothing else, every listed kernel outcome and every `raise` of `run`."""
    assert sorted(FIXTURE['cases']) == sorted(CASE_BY_NAME)
    assert all(FIXTURE['cases'][c['name']]['tune'] == c['tune'] for c in CASES)
    launches = [r['desc'] for c in FIXTURE['cases'].values() for r in c['calls'] if r['entry'] == 'spaa_tapconv_f32']
    launches = [{**dict.fromkeys(('tile', 'ksplit', 'reserved0', 'reserved1', 'reserved2'), 0), **d} for d in launches]
    outcomes = {(d['tile'], (d['ksplit'] > 1) - (d['ksplit'] < 0), d['reserved1']) for d in launches}
    assert WANT_OUTCOMES <= outcomes, sorted(WANT_OUTCOMES - outcomes)
    raised = [c['raises'][1] for c in FIXTURE['cases'].values() if 'raises' in c]
    missing = [m for m in WANT_RAISES if not any(m in r for r in raised)]
    assert not missing, missing
    pad_codes = {(d['reserved0'] & _lib.WINO_PAD) >> _lib.WINO_PAD_SHIFT for d in launches if d['tile'] in (70, 71, 73)}
    assert pad_codes == {cp.wino_pad_code(p) for p in (1, 0, 2)} == {0, 1, 2}      # Winograd paddings 1 / 0 / 2
    assert {d['reserved2'] for d in launches if d['tile'] == 74} == {0, _lib.X6P_STD}
    entries = {r['entry'] for c in FIXTURE['cases'].values() for r in c['calls']}
    assert {'spaa_maxpool_bwd_f16', 'spaa_maxpool_fwd', 'spaa_maxpool_fwd_f16', 'spaa_linear_small', 'spaa_tapconv_wgrad'} <= entries


@pytest.mark.parametrize('kind', sorted(REFRESH))
def test_refresh_equals_fresh_plan(kind, monkeypatch):
    plan, fresh, stale = refresh_case(kind, monkeypatch.setattr)
    assert set(stale) == {'wino': {'w_half'}, 'c3': {'c3', 'c3h'}, 'thin': {'w_half', 'thin_s', 'thin_h'}}[kind]
    assert plan.w_half is None and plan._thin == {} and plan._c3 is None and plan._c3h is None      # every packed layout dropped
    assert (plan.wino is not None) == (kind == 'wino')
    for a, b in ((plan, fresh), (plan.wino, fresh.wino)) if kind == 'wino' else ((plan, fresh),):
        assert torch.equal(a.weights, b.weights) and torch.equal(a.w_split, b.w_split)
    if fresh.bias is not None:
        assert torch.equal(plan.bias, fresh.bias) and (plan.wino is None or plan.wino.bias is plan.bias)
    now, want = packed_layouts(plan), packed_layouts(fresh)
    for k in stale:
        assert torch.equal(now[k], want[k]) and not torch.equal(now[k], stale[k]), k


@pytest.mark.parametrize('how', ['x6p', 'h16', '2src'])
def test_refresh_refuses_second_source(how):
    if how == '2src':
        plan = build_plan(('conv2src', 64, 64, 64))
    else:
        plan = build_plan(('deconv', 64, 32, 3, 2, 1, how == 'h16'), attach=(how, 32))
    with pytest.raises(RuntimeError) as e:
        plan.refresh(torch.zeros(1))
    assert str(e.value) == FIXTURE['refresh_second_source_error'][how]
