"""ConvNeXt-Tiny (torchvision.models.convnext_tiny, eval) forward and input-gradient: the stem, the two linear layers of every block,
the downsample convolutions and the head on the tap-list convolution plans (spaa_amd/convplan.py), the depthwise 7 x 7 layers on the
kernels of csrc/convnext_ops.hip, LayerNorm, exact GELU and the patch gather on those of csrc/vit_ops.hip.

The architecture is third-party; it is restated here from its published definition (Liu et al., "A ConvNet for the 2020s", 2022) with
torchvision's key names: `features.0.0` the 4 x 4 / stride-4 stem convolution and `features.0.1` its LayerNorm over the channels of
every pixel; `features.{1,3,5,7}.{i}` the blocks (`block.0` depthwise 7 x 7 with padding 3, `block.2` LayerNorm, `block.3` linear
C -> 4 C, GELU, `block.5` linear 4 C -> C, `layer_scale` [C, 1, 1]): x + layer_scale * branch(x); `features.{2,4,6}` the downsamples
(`.0` LayerNorm over channels, `.1` a 2 x 2 / stride-2 convolution without padding: an odd side loses its last row or column);
`classifier.0` LayerNorm after adaptive_avg_pool2d(1), `classifier.2` the linear head.  Every LayerNorm has eps 1e-6, GELU is the
exact erf form, stochastic depth is the identity.  Widths and depths are read from the tensors (ConvNeXt-Tiny: 96, 192, 384, 768 with
3, 3, 9, 3 blocks).

The stem runs as the ViT's patch embedding does: spaa_vit_patchify with P = 4 and `features.0.0` as a 1 x 1 plan over K = 4 P P = 64.
Layer scale is folded into `block.5` on the host (W' = diag(ls) W, b' = ls b), as BatchNorm is folded for the other bodies: the
launch's epilogue is then bias + residual, which the plans have.  A block is five launches forward (dwconv7, LayerNorm, block.3,
GELU, block.5 + residual) and five backward (block.5's input gradient, the GELU adjoint, block.3's input gradient, the LayerNorm
adjoint, spaa_dwconv7_bwd with add = the gradient of the block's output).

Saved per block for the backward pass: the depthwise output (the LayerNorm's input), mean and rstd, and block.3's pre-activation:
5 C floats per pixel.  The body ends in a convolutional feature map (the last block's output), so Grad-CAM reads it as it reads the
other CNNs'; there are no ReLU gates.  fp16 storage is not implemented.
"""
import torch

from . import _lib
from . import convplan as cp
from . import pooling
from .classifier import ClassifierBody, _strip
from .vit import patch_weight

LN_EPS = 1e-6
STEM, STEM_LN = 'features.0.0', 'features.0.1'
HEAD_LN, HEAD = 'classifier.0', 'classifier.2'


def config(sd):
    """(P, dims, depths) as the state dict `sd` (no `module.` prefixes) has them: the stem's kernel size, the width and the number
    of blocks of every stage `features.{1, 3, 5, ...}`.  ValueError where `sd` is not a ConvNeXt's (no stem convolution, no block)."""
    w = sd.get(STEM + '.weight')
    if w is None or w.ndim != 4 or 'features.1.0.block.0.weight' not in sd:
        raise ValueError(f"convnext_tiny: the state dict is not a ConvNeXt's (it needs {STEM}.weight [C, 3, P, P] and features.1.0.block.0.weight)")
    dims, depths, s = [], [], 1
    while f'features.{s}.0.block.0.weight' in sd:
        n = 0
        while f'features.{s}.{n}.block.0.weight' in sd:
            n += 1
        dims.append(int(sd[f'features.{s}.0.block.0.weight'].shape[0]))
        depths.append(n)
        s += 2
    return int(w.shape[2]), tuple(dims), tuple(depths)


def map_sizes(input_sz, P, nstage):
    """The (h, w) of every stage's map: the stem divides by P, every downsample halves and drops an odd side's last row or column."""
    h, w = input_sz[0] // P, input_sz[1] // P
    out = [(h, w)]
    for _ in range(nstage - 1):
        h, w = h // 2, w // 2
        out.append((h, w))
    return out


def check_geometry(sd, input_sz):
    """ValueError where this implementation does not serve the network `sd` at the input size `input_sz` (nothing is allocated)."""
    P, dims, depths = config(sd)
    h, w = input_sz
    if h % P or w % P or h < P or w < P:
        raise ValueError(f'convnext_tiny: input_sz {tuple(input_sz)} must be a multiple of {P} in both directions (the stem is a '
                         f'{P} x {P} / stride-{P} convolution and runs through the patch gather)')
    widths = (int(sd[STEM + '.weight'].shape[0]),) + dims
    if any(c % 4 for c in widths):
        raise ValueError(f'convnext_tiny: every width must be a multiple of 4 (the kernels own channel quads), got {widths}')
    hl, wl = map_sizes(input_sz, P, len(dims))[-1]
    if hl < 1 or wl < 1:
        raise ValueError(f'convnext_tiny: input_sz {tuple(input_sz)} leaves a final map of {hl} x {wl} after the stem and '
                         f'{len(dims) - 1} downsamples; it must be at least 1 x 1')


def fold_layer_scale(w, b, ls):
    """block.5 with the block's layer scale folded in: (diag(ls) W, ls b) for W [C, 4 C], b [C], ls [C, 1, 1]."""
    ls = ls.reshape(-1)
    return ls[:, None] * w, ls * b


def dw_weight(w):
    """block.0.weight [C, 1, 7, 7] -> [49][C] tap-major (tap = 7 ky + kx)."""
    return w.reshape(w.shape[0], 49).t().contiguous()


class ConvNeXtBody(ClassifierBody):
    body_masks_switch = False

    def __init__(self, sd, batch, in_hw, dev, storage='f32'):
        if storage != 'f32':
            raise NotImplementedError(f"ConvNeXtBody: storage={storage!r} is not implemented (the depthwise, LayerNorm and GELU kernels are "
                                      "fp32); use storage='f32'")
        sd = _strip(sd)
        check_geometry(sd, in_hw)
        super().__init__(sd, batch, in_hw, dev, storage)
        sd, zf, B = self.sd, self.zf, batch
        h, w = in_hw
        self.P, self.dims, self.depths = P, dims, depths = config(sd)
        sizes = map_sizes(in_hw, P, len(dims))

        def vec(key):
            return sd[key].detach().float().reshape(-1).contiguous().to(dev)

        def ln(key):
            return vec(key + '.weight'), vec(key + '.bias')

        def lin(wt, bs, name):
            wt = wt.reshape(wt.shape[0], wt.shape[1], 1, 1)
            return cp.conv_fwd_plan(wt, bs, 1, 0, dev, name), cp.conv_dgrad_plan(wt, 1, 0, dev, name + '_dgrad')

        c0 = int(sd[STEM + '.weight'].shape[0])
        if c0 != dims[0]:
            raise ValueError(f'convnext_tiny: the stem writes {c0} channels, the first stage has {dims[0]}')
        h0, w0 = sizes[0]
        wp = patch_weight(sd[STEM + '.weight'].detach().float().cpu())
        self.stem_f = cp.conv_fwd_plan(wp, sd[STEM + '.bias'], 1, 0, dev, STEM)
        self.stem_d = cp.conv_dgrad_plan(wp, 1, 0, dev, STEM + '_dgrad')
        self.stem_ln = ln(STEM_LN)
        self.patches, self.g_patches = zf(B, h0, w0, 4 * P * P), zf(B, h0, w0, 4 * P * P)
        self.emb, self.g_emb = zf(B, h0, w0, c0), zf(B, h0, w0, c0)
        self.st_stem = (zf(B * h0 * w0), zf(B * h0 * w0))
        self.x0 = zf(B, h0, w0, c0)
        self.stages, self.blocks = [], []
        x = self.x0
        for si, (C, depth, (hh, ww)) in enumerate(zip(dims, depths, sizes)):
            s = 2 * si + 1
            # shared between the blocks of a stage: the LayerNorm and GELU outputs and every gradient
            stg = dict(C=C, hw=(hh, ww), nrm=zf(B, hh, ww, C), act=zf(B, hh, ww, 4 * C), g_act=zf(B, hh, ww, 4 * C), g_n=zf(B, hh, ww, C),
                       g_d=zf(B, hh, ww, C), g_x=(zf(B, hh, ww, C), zf(B, hh, ww, C)), blocks=[])
            if si > 0:
                cprev, (hp, wp_) = dims[si - 1], sizes[si - 1]
                key = f'features.{s - 1}'
                wd, bd = sd[key + '.1.weight'], sd[key + '.1.bias']
                stg['down'] = dict(ln=ln(key + '.0'), f=cp.conv_fwd_plan(wd, bd, 2, 0, dev, key + '.1'),
                                   d=cp.conv_dgrad_plan(wd, 2, 0, dev, key + '.1_dgrad'), x=x, st=(zf(B * hp * wp_), zf(B * hp * wp_)),
                                   nrm=zf(B, hp, wp_, cprev), g_nrm=zf(B, hp, wp_, cprev), out=zf(B, hh, ww, C), g_x=zf(B, hp, wp_, cprev))
                x = stg['down']['out']
            for i in range(depth):
                p = f'features.{s}.{i}'
                blk = dict(name=p, x=x, stage=stg, dw_w=dw_weight(sd[p + '.block.0.weight'].detach().float()).to(dev), dw_b=vec(p + '.block.0.bias'),
                           ln=ln(p + '.block.2'))
                blk['f3'], blk['d3'] = lin(sd[p + '.block.3.weight'], sd[p + '.block.3.bias'], p + '.block.3')
                w5, b5 = fold_layer_scale(sd[p + '.block.5.weight'].detach().float(), sd[p + '.block.5.bias'].detach().float(),
                                          sd[p + '.layer_scale'].detach().float())
                blk['f5'], blk['d5'] = lin(w5, b5, p + '.block.5')
                # what the backward pass reads
                blk['d'], blk['st'], blk['pre'] = zf(B, hh, ww, C), (zf(B * hh * ww), zf(B * hh * ww)), zf(B, hh, ww, 4 * C)
                blk['out'] = zf(B, hh, ww, C)
                stg['blocks'].append(blk)
                self.blocks.append(blk)
                x = blk['out']
            self.stages.append(stg)
        self.feat = x
        self.head_ln = ln(HEAD_LN)
        self.build_head(dims[-1], HEAD)
        self.hn, self.g_hn, self.st_head = zf(B, 1, 1, dims[-1]), zf(B, 1, 1, dims[-1]), (zf(B), zf(B))
        self.g_in = zf(B, h, w, 4)

    # ---- the launches of csrc/vit_ops.hip and csrc/convnext_ops.hip ----------------------------------------------------------------
    @staticmethod
    def ln_fwd(x, wb, y, st):
        D = x.shape[-1]
        _lib.call('spaa_layernorm_fwd', _lib.ptr(x), D, _lib.ptr(wb[0]), _lib.ptr(wb[1]), _lib.ptr(y), D, _lib.ptr(st[0]), _lib.ptr(st[1]),
                  x.numel() // D, D, LN_EPS)

    @staticmethod
    def ln_bwd(g, x, wb, st, gx):
        D = x.shape[-1]
        _lib.call('spaa_layernorm_bwd', _lib.ptr(g), D, _lib.ptr(x), D, _lib.ptr(wb[0]), _lib.ptr(st[0]), _lib.ptr(st[1]), None, D, _lib.ptr(gx), D,
                  x.numel() // D, D)

    def dw_fwd(self, blk):
        b, h, w, c = blk['x'].shape
        _lib.call('spaa_dwconv7_fwd', _lib.ptr(blk['x']), _lib.ptr(blk['dw_w']), _lib.ptr(blk['dw_b']), _lib.ptr(blk['d']), b, h, w, c)

    @staticmethod
    def dw_bwd(blk, g_d, add, g_x):
        b, h, w, c = g_d.shape
        _lib.call('spaa_dwconv7_bwd', _lib.ptr(g_d), _lib.ptr(blk['dw_w']), _lib.ptr(add), _lib.ptr(g_x), b, h, w, c)

    # ---- execution -----------------------------------------------------------------------------------------------------------------
    def forward(self, x4):
        p, B = _lib.ptr, self.B
        h, w = self.in_hw
        _lib.call('spaa_vit_patchify', p(x4), p(self.patches), B, h, w, self.P)
        self.stem_f.run(self.patches, self.emb)
        self.ln_fwd(self.emb, self.stem_ln, self.x0, self.st_stem)
        for stg in self.stages:
            if 'down' in stg:
                dn = stg['down']
                self.ln_fwd(dn['x'], dn['ln'], dn['nrm'], dn['st'])
                dn['f'].run(dn['nrm'], dn['out'])
            for blk in stg['blocks']:
                self.dw_fwd(blk)
                self.ln_fwd(blk['d'], blk['ln'], stg['nrm'], blk['st'])
                blk['f3'].run(stg['nrm'], blk['pre'])
                _lib.call('spaa_gelu_fwd', p(blk['pre']), p(stg['act']), blk['pre'].numel())
                blk['f5'].run(stg['act'], blk['out'], add=blk['x'])
        pooling.global_avgpool_fwd(self.feat, self.pooled)
        self.ln_fwd(self.pooled, self.head_ln, self.hn, self.st_head)
        self.fc_f.run(self.hn, self.logits)
        return self.logits.view(B, self.ncls)

    def head_grad(self, g_logits):
        """g_logits [B, ncls] -> the gradient at the pooled features [B, 1, 1, C], behind the adjoint of classifier.0's LayerNorm."""
        self.fc_d.run(g_logits.view(self.B, 1, 1, self.ncls), self.g_hn)
        self.ln_bwd(self.g_hn, self.pooled, self.head_ln, self.st_head, self.g_pooled)
        return self.g_pooled

    def backward(self, g_logits):
        """g_logits [B, ncls] -> gradient w.r.t. the normalised input [B, h, w, 4]."""
        p, B = _lib.ptr, self.B
        h, w = self.in_hw
        last = self.stages[-1]
        g = last['g_x'][0]
        pooling.global_avgpool_bwd(self.head_grad(g_logits), None, g)
        for stg in reversed(self.stages):
            for i in range(len(stg['blocks']) - 1, -1, -1):
                blk = stg['blocks'][i]
                blk['d5'].run(g, stg['g_act'])
                _lib.call('spaa_gelu_bwd', p(stg['g_act']), p(blk['pre']), p(stg['g_act']), blk['pre'].numel())
                blk['d3'].run(stg['g_act'], stg['g_n'])
                self.ln_bwd(stg['g_n'], blk['d'], blk['ln'], blk['st'], stg['g_d'])
                g_x = stg['g_x'][1] if g is stg['g_x'][0] else stg['g_x'][0]
                self.dw_bwd(blk, stg['g_d'], g, g_x)
                g = g_x
            if 'down' in stg:
                dn = stg['down']
                dn['d'].run(g, dn['g_nrm'])
                self.ln_bwd(dn['g_nrm'], dn['x'], dn['ln'], dn['st'], dn['g_x'])
                g = dn['g_x']
        self.ln_bwd(g, self.emb, self.stem_ln, self.st_stem, self.g_emb)
        self.stem_d.run(self.g_emb, self.g_patches)
        _lib.call('spaa_vit_unpatchify', p(self.g_patches), p(self.g_in), B, h, w, self.P)
        return self.g_in

    def attention_source(self):
        return self.feat, self.g_pooled, True

    def refresh_masks(self):
        """Nothing to do: the body has no gates (GELU is smooth; its adjoint reads the pre-activation itself)."""

    def fwd_plans(self):
        yield self.stem_f, self.x0.shape[1:3]
        for stg in self.stages:
            if 'down' in stg:
                yield stg['down']['f'], stg['hw']
            for blk in stg['blocks']:
                yield blk['f3'], stg['hw']
                yield blk['f5'], stg['hw']
        yield self.fc_f, (1, 1)

    def flops_dw(self):
        """Algorithmic FLOPs (2 x 49 MACs per element) of the depthwise layers, forward."""
        return sum(2 * 49 * blk['d'].numel() for blk in self.blocks)

    def flops_fwd(self):
        return super().flops_fwd() + self.flops_dw()
