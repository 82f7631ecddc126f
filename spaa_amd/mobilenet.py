"""MobileNetV2 (torchvision.models.mobilenet_v2, eval, width 1.0) forward and input-gradient: the 1 x 1 layers on the tap-list
convolution plans (spaa_amd/convplan.py, as Inception-v3's 1 x 1 layers), the depthwise 3 x 3 layers and every ReLU6 on the kernels of
csrc/dwconv.hip.

The architecture is third-party; it is restated here from its published definition (Sandler et al., "MobileNetV2: Inverted Residuals
and Linear Bottlenecks", 2018) with torchvision's key names: `features.0` the 3 x 3 / stride-2 stem, `features.1` the t = 1 block
(depthwise `conv.0`, projection `conv.1` / `conv.2`), `features.2` .. `features.17` the t = 6 blocks (expansion `conv.0`, depthwise
`conv.1`, projection `conv.2` / `conv.3`), `features.18` the 1 x 1 layer to 1280 channels, `classifier.1` the linear layer.  Every
BatchNorm (eps 1e-5) is folded into its convolution.  There are 35 ReLU6 sites: the stem, 17 depthwise layers, 16 expansions,
`features.18`.

Where a ReLU6 is applied.  A 1 x 1 expansion (and the stem) writes its PRE-activation; the depthwise layer that follows clamps it as
it loads and writes its own clamped output with gate bytes.  The projections are linear, so block inputs carry no gate.  `features.18`
is clamped in place by spaa_relu6_gate: its output is the feature map that the head pools and Grad-CAM reads.
Backward, per block: the projection's input gradient under the depthwise layer's gate bytes (`gate_bits`), spaa_dwconv3_bwd under the
gate of the expansion's pre-activation, the expansion's input gradient, plus the gradient of the block's output where the block is
residual.

fp16 storage is not implemented for this body.
"""
import torch

from . import _lib
from . import convplan as cp
from .classifier import ClassifierBody

# (expansion t, output channels c, repeats n, stride s of the first block of the group)
BLOCK_TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))
STEM_C, LAST_C = 32, 1280
# (the 1 x 1 plans serve K and N of 16 and 24 as they are -- tests/test_mobilenet_gpu.py checks them against float64 -- so no width is padded)


def block_specs():
    """(name, expansion, cin, cout, stride) of features.1 .. features.17."""
    out, cin, idx = [], STEM_C, 1
    for t, c, n, s in BLOCK_TABLE:
        for i in range(n):
            out.append((f'features.{idx}', t, cin, c, s if i == 0 else 1))
            cin, idx = c, idx + 1
    return out


def pack_gate6(act):
    """The gate bytes of a ReLU6 for the activation or pre-activation `act` [..., C]: bit e of byte q = (0 < act[..., 4 q + e] < 6)."""
    c = act.shape[-1]
    assert c % 4 == 0
    bits = ((act > 0) & (act < 6)).view(*act.shape[:-1], c // 4, 4).to(torch.uint8)
    wgt = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=act.device)
    return (bits * wgt).sum(dim=-1).to(torch.uint8).contiguous()


class MobileNetV2Body(ClassifierBody):
    body_masks_switch = False

    def __init__(self, sd, batch, in_hw, dev, storage='f32'):
        if storage != 'f32':
            raise NotImplementedError(f"MobileNetV2Body: storage={storage!r} is not implemented (the depthwise kernels are fp32); use storage='f32'")
        super().__init__(sd, batch, in_hw, dev, storage)
        self.masks = True       # a ReLU6 has no float-gate form here: the gate bytes are always written and read
        z, zb, osz, B = self.z, self.zb, self.out_size, batch
        h, w = in_hw
        wgt, b = self.folded('features.0.0', 'features.0.1')
        self.stem_f = cp.conv_fwd_plan(wgt, b, 2, 1, dev, 'features.0')
        self.stem_d = cp.conv_dgrad_plan(wgt, 2, 1, dev, 'features.0_dgrad')
        hh, ww = osz(h, 3, 2, 1), osz(w, 3, 2, 1)
        self.s_pre, self.g_s = z(B, hh, ww, STEM_C), z(B, hh, ww, STEM_C)
        self.blocks = []
        x_buf = self.s_pre     # (block 1's depthwise layer reads the stem's pre-activation)
        for name, t, cin, cout, stride in block_specs():
            blk = dict(name=name, stride=stride, x=x_buf, hin=hh, win=ww, residual=stride == 1 and cin == cout and t != 1)
            hid = cin * t
            if t != 1:
                we, be = self.folded(name + '.conv.0.0', name + '.conv.0.1')
                blk['fe'] = cp.conv_fwd_plan(we, be, 1, 0, dev, name + '.expand')
                blk['de'] = cp.conv_dgrad_plan(we, 1, 0, dev, name + '.expand_dgrad')
                blk['e_pre'], blk['g_e'] = z(B, hh, ww, hid), z(B, hh, ww, hid)
                blk['g_x'] = z(B, hh, ww, cin)
                dwk, pj = name + '.conv.1', name + '.conv.2'
                wd, bd = self.folded(dwk + '.0', dwk + '.1')
                wp, bp = self.folded(pj, name + '.conv.3')
            else:
                blk['e_pre'], blk['g_e'] = self.s_pre, self.g_s
                wd, bd = self.folded(name + '.conv.0.0', name + '.conv.0.1')
                wp, bp = self.folded(name + '.conv.1', name + '.conv.2')
            # depthwise weight [C, 1, 3, 3] -> [9][C] tap-major
            blk['dw_w'] = wd.view(hid, 9).t().contiguous().to(dev)
            blk['dw_b'] = bd.contiguous().to(dev)
            ho, wo = osz(hh, 3, stride, 1), osz(ww, 3, stride, 1)
            blk['d'], blk['g_d'], blk['m_d'] = z(B, ho, wo, hid), z(B, ho, wo, hid), zb(B, ho, wo, hid // 4)
            blk['fp'] = cp.conv_fwd_plan(wp, bp, 1, 0, dev, name + '.project')
            blk['dp'] = cp.conv_dgrad_plan(wp, 1, 0, dev, name + '.project_dgrad')
            blk['out'] = z(B, ho, wo, cout)
            blk['hid'], blk['hout'], blk['wout'] = hid, ho, wo
            self.blocks.append(blk)
            x_buf, hh, ww = blk['out'], ho, wo
        wl, bl = self.folded('features.18.0', 'features.18.1')
        self.last_f = cp.conv_fwd_plan(wl, bl, 1, 0, dev, 'features.18')
        self.last_d = cp.conv_dgrad_plan(wl, 1, 0, dev, 'features.18_dgrad')
        self.feat, self.g_feat, self.m_feat = z(B, hh, ww, LAST_C), z(B, hh, ww, LAST_C), zb(B, hh, ww, LAST_C // 4)
        self.g_x_last = z(B, hh, ww, self.blocks[-1]['out'].shape[3])
        self.build_head(LAST_C, 'classifier.1')
        self.g_in = self.zf(B, h, w, 4)

    # ---- the depthwise launches ------------------------------------------------------------------------------------
    def dw_fwd(self, blk, write_mask):
        p = _lib.ptr
        _lib.call('spaa_dwconv3_fwd', p(blk['e_pre']), 1, p(blk['dw_w']), p(blk['dw_b']), p(blk['d']), p(blk['m_d']) if write_mask else None,
                  self.B, blk['hin'], blk['win'], blk['hid'], blk['stride'])

    def dw_bwd(self, blk):
        p = _lib.ptr
        _lib.call('spaa_dwconv3_bwd', p(blk['g_d']), p(blk['dw_w']), p(blk['e_pre']), p(blk['g_e']), self.B, blk['hin'], blk['win'], blk['hid'],
                  blk['stride'])

    # ---- execution -------------------------------------------------------------------------------------------------
    def forward(self, x4):
        wm = self.write_masks
        self.stem_f.run(x4, self.s_pre)
        for blk in self.blocks:
            if 'fe' in blk:
                blk['fe'].run(blk['x'], blk['e_pre'])
            self.dw_fwd(blk, wm)
            blk['fp'].run(blk['d'], blk['out'], add=blk['x'] if blk['residual'] else None)
        self.last_f.run(self.blocks[-1]['out'], self.feat)
        b, h, w, c = self.feat.shape
        _lib.call('spaa_relu6_gate', _lib.ptr(self.feat), _lib.ptr(self.m_feat) if wm else None, b * h * w, c)
        return self.head_fwd(self.feat)

    def head_bwd(self, g_logits, last, g_last):
        """g_logits [B, ncls] -> `g_last`, the gradient w.r.t. the pre-activation of features.18 (under its ReLU6 gate bytes)."""
        b, h, w, c = last.shape
        _lib.call('spaa_global_avgpool_bwd_bits', _lib.ptr(self.head_grad(g_logits)), _lib.ptr(self.m_feat), _lib.ptr(g_last), b, h * w, c)

    def backward(self, g_logits):
        """g_logits [B, ncls] -> gradient w.r.t. the normalised input [B, h, w, 4]."""
        self.head_bwd(g_logits, self.feat, self.g_feat)
        self.last_d.run(self.g_feat, self.g_x_last)
        gP = self.g_x_last
        for blk in reversed(self.blocks):
            blk['dp'].run(gP, blk['g_d'], gate_bits=blk['m_d'])
            self.dw_bwd(blk)
            if 'de' in blk:
                blk['de'].run(blk['g_e'], blk['g_x'], add=gP if blk['residual'] else None)
                gP = blk['g_x']
        self.stem_d.run(self.g_s, self.g_in)
        return self.g_in

    def attention_source(self):
        return self.feat, self.g_pooled, True

    def refresh_masks(self):
        """Recompute the gate bytes from the activation buffers (after a test has overwritten the activations)."""
        for blk in self.blocks:
            blk['m_d'].copy_(pack_gate6(blk['d'].float()))
        self.m_feat.copy_(pack_gate6(self.feat.float()))

    def fwd_plans(self):
        yield self.stem_f, self.s_pre.shape[1:3]
        for blk in self.blocks:
            if 'fe' in blk:
                yield blk['fe'], (blk['hin'], blk['win'])
            yield blk['fp'], (blk['hout'], blk['wout'])
        yield self.last_f, self.feat.shape[1:3]
        yield self.fc_f, (1, 1)

    def flops_dw(self):
        """Algorithmic FLOPs (2 x MAC) of the 17 depthwise layers, forward."""
        return sum(2 * 9 * self.B * blk['hout'] * blk['wout'] * blk['hid'] for blk in self.blocks)

    def flops_fwd(self):
        return super().flops_fwd() + self.flops_dw()
