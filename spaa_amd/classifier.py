"""Frozen ImageNet classifier on HIP kernels behind the reference's `Classifier` contract.

Mirrors /root/reference/src/python/classifier.py:12-75: `Classifier(model_name, device, device_ids, fix_params,
sort_results)` and `classifier(im, crop_sz) -> (raw_score Tensor[B,1000], p_sorted ndarray, idx ndarray)`.
The network bodies are torchvision's (third-party, not in the reference tree; pinned torchvision==0.15.1): the
architecture is restated here as a layer table over the tap-list convolution kernel, with eval-mode BatchNorm
folded into the convolutions.  Pretrained weights cannot be downloaded in this environment (the reference fetches
them by URL, classifier.py:24-36): pass `state_dict=` (torchvision key names) or `weights_path=`.

`ClassifierEngine` is what the fused attack loop drives: forward = crop + area-resize + normalise -> net -> logits;
backward = input gradient only (all parameters frozen, classifier.py:41-44).
"""
import dataclasses
import os
import weakref

import numpy as np
import torch

from . import _lib
from . import convplan as cp
from . import pooling
from .models import to_nhwc4, to_nchw, USE_GATE_MASKS

FUSE_POOL = os.environ.get('SPAA_FUSE_POOL', '1') != '0'   # VGG-16, fp16 storage: the 2 x 2 max-pools in the epilogue of the convolution before them
FOLD_S2_F16 = int(os.environ.get('SPAA_FOLD_S2_F16', '0'))   # fp16 storage: ResNet's stride-2 input gradients with the four parity classes folded into N: 0 never (default: neutral in the loop, 238.7-239.3 it/s either way), 1 layer2.0 (49.5 -> 38 us per launch), 2 all three
# 1: ResNet-18's max-pool adjoint as the prologue of the stem's input gradient.  Measured SLOWER (profiles/r05_frontend.txt: stem_dgrad
# 190 -> 304 us for the 55 us launch it removes -- the patch formed by loads + VALU work in four dependent round trips per channel block
# where the LDS-DMA of the separate form costs no issue slots): off by default, kept with its bitwise test.
FUSE_POOL_ADJOINT = os.environ.get('SPAA_FUSE_POOL_ADJOINT', '0') == '1'
BODY_GATE_MASKS = os.environ.get('SPAA_BODY_MASKS', '1') != '0'   # 0: VGG-16 / Inception-v3 gate with the activation itself (A/B measurements)

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
INPUT_SZ = {'resnet18': (224, 224), 'vgg16': (224, 224), 'inception_v3': (299, 299), 'mobilenet_v2': (224, 224), 'vit_b_16': (224, 224),
            'convnext_tiny': (224, 224)}


@dataclasses.dataclass(frozen=True)
class Attention:
    """Attention-weighted attack: the classifier's gradient image at the camera is multiplied by floor + (1 - floor) M,
    M in [0, 1] the Grad-CAM map of the sample's class resampled onto the classifier crop.  `floor`: the weight where the classifier
    does not look (0: the adversarial step puts nothing there; 1: the plain attack).  `rollout`: a body without a
    convolutional feature map (vit_b_16) takes the gradient-weighted attention rollout of its class token as M instead of being
    refused; the convolutional bodies keep Grad-CAM either way."""
    floor: float = 0.0
    rollout: bool = False

    def __post_init__(self):
        if isinstance(self.floor, bool) or not isinstance(self.floor, (int, float)) or not 0 <= float(self.floor) <= 1:
            raise ValueError(f'Attention: floor must be a number in [0, 1], got {self.floor!r}')
        if not isinstance(self.rollout, bool):
            raise ValueError(f'Attention: rollout must be a bool, got {self.rollout!r}')


def center_crop_origin(h, w, size):
    """img_proc.py:126-132."""
    th, tw = size
    return int(round((h - th) / 2.)), int(round((w - tw) / 2.))


def _strip(sd):
    out = {}
    for k, v in sd.items():
        while k.startswith('module.'):
            k = k[len('module.'):]
        out[k] = v
    return out


class ClassifierBody:
    """What the bodies share: the storage mode and its allocators, the layer-size and BatchNorm-folding helpers, the ReLU-gate
    switches, the global-average-pool + linear head of ResNet-18, Inception-v3 and MobileNetV2, and flops_fwd() over `fwd_plans()`.
    A body provides forward(x4) -> logits [B, ncls], backward(g_logits) -> gradient w.r.t. x4, refresh_masks(), fwd_plans() and
    attention_source()."""
    body_masks_switch = True   # SPAA_BODY_MASKS=0 applies (VGG-16, Inception-v3: the A/B switch never covered ResNet-18)

    def __init__(self, sd, batch, in_hw, dev, storage):
        self.sd = _strip(sd)
        self.B, self.dev, self.storage, self.in_hw = batch, dev, storage, tuple(in_hw)
        self.h16 = storage == 'f16'
        self.act_dtype = torch.float16 if self.h16 else torch.float32   # activations / gradients; input image, features, logits fp32
        # ReLU gates as byte masks (1 byte per 4 channels) written by the forward epilogues: an input-gradient launch reads 2 bits per
        # element instead of the activation and stays on the branch-free epilogue (epilogue.hpp fast_epi_*;
        # profiles/r05_configs4_f16s_tapconv_layers.json: VGG-16 features.2_dgrad 689 us against 477 forward with the activation as gate)
        self.masks = (USE_GATE_MASKS or self.h16) and (BODY_GATE_MASKS or not self.body_masks_switch)
        self.write_masks = True       # (ClassifierEngine clears it for a forward pass nobody differentiates: the masks are skipped)

    def z(self, *shape):
        return torch.zeros(*shape, device=self.dev, dtype=self.act_dtype)

    def zf(self, *shape):
        return torch.zeros(*shape, device=self.dev)

    def zb(self, *shape):
        return torch.zeros(*shape, device=self.dev, dtype=torch.uint8)

    @staticmethod
    def out_size(n, k, s, p):
        return (n + 2 * p - k) // s + 1

    def folded(self, conv, bn, eps=1e-5):
        """Weight and bias of the convolution `conv` with its eval-mode BatchNorm `bn` folded in."""
        sd = self.sd
        return cp.fold_bn(sd[conv + '.weight'], sd[bn + '.weight'], sd[bn + '.bias'], sd[bn + '.running_mean'], sd[bn + '.running_var'], eps=eps)

    def build_head(self, c, key='fc'):
        """adaptive_avg_pool2d(1) over `c` channels + the linear layer `key` (ResNet-18, Inception-v3: 'fc'; MobileNetV2: 'classifier.1')."""
        sd, B = self.sd, self.B
        self.ncls = sd[key + '.weight'].shape[0]
        self.pooled, self.g_pooled = self.zf(B, 1, 1, c), self.zf(B, 1, 1, c)
        self.fc_f = cp.linear_fwd_plan(sd[key + '.weight'], sd[key + '.bias'], self.dev, 'fc')
        self.fc_d = cp.linear_dgrad_plan(sd[key + '.weight'], self.dev, 'fc_dgrad')
        self.logits = self.zf(B, 1, 1, self.ncls)

    def head_fwd(self, last):
        pooling.global_avgpool_fwd(last, self.pooled)
        self.fc_f.run(self.pooled, self.logits)
        return self.logits.view(self.B, self.ncls)

    def head_grad(self, g_logits):
        """The head's part of the backward pass alone: g_logits [B, ncls] -> the gradient at the features the head pools (here
        `g_pooled`; what attention_source() names as the gradient)."""
        self.fc_d.run(g_logits.view(self.B, 1, 1, self.ncls), self.g_pooled)
        return self.g_pooled

    def head_bwd(self, g_logits, last, g_last):
        """g_logits [B, ncls] -> `g_last`, the gradient w.r.t. the pre-activation of `last` (a ReLU output: gated)."""
        pooling.global_avgpool_bwd(self.head_grad(g_logits), last, g_last)

    def attention_source(self):
        """What Grad-CAM reads after a backward pass (or after head_grad alone): (A, G, pooled).  A [B, h, w, C]: the fp32 feature map
        that enters the head's average pool.  G: the ungated gradient there -- with `pooled`, as the head's g_pooled [B, 1, 1, C] (the
        gradient at every position is g_pooled / (h w)), else as the map [B, h, w, C] itself."""
        raise NotImplementedError

    def relevance_grid(self):
        """The (rows, columns) of the map that backward(g_logits, relevance=...) writes where the body has an attention rollout
        (vit_b_16's patch grid); None for a body that hands Grad-CAM a feature map instead."""
        return None

    def flops_fwd(self):
        return sum(plan.flops(self.B, h, w) for plan, (h, w) in self.fwd_plans())


# layer2.0.conv1's input gradient (128 -> 64 channels, 28^2 -> 56^2) at benchmark batches: the patch-staged stride-2 kernel with its
# four parity classes in one launch (tools/lab/x6p_resnet.py: 79 -> 71 us), from this many input pixels (batch x 56 x 56) on
X6P_DGRAD_MIN_PIXELS = 100000


class ResNet18Body(ClassifierBody):
    """torchvision.models.resnet18 (eval) forward + input-gradient on tapconv/maxpool/avgpool kernels."""
    body_masks_switch = False

    def __init__(self, sd, batch, in_hw, dev, storage='f32'):
        super().__init__(sd, batch, in_hw, dev, storage)
        sd, z, osz = self.sd, self.z, self.out_size
        h, w = in_hw
        wgt, b = self.folded('conv1', 'bn1')
        self.stem_f = cp.conv_fwd_plan(wgt, b, 2, 3, dev, 'stem')
        self.stem_d = cp.conv_dgrad_plan(wgt, 2, 3, dev, 'stem_dgrad')
        h1, w1 = osz(h, 7, 2, 3), osz(w, 7, 2, 3)
        self.c1 = z(batch, h1, w1, 64)
        h2, w2 = osz(h1, 3, 2, 1), osz(w1, 3, 2, 1)
        self.mp = z(batch, h2, w2, 64)
        self.mp_arg = self.zb(batch, h2, w2, 64)
        self.blocks = []
        cin, hh, ww = 64, h2, w2
        x_buf = self.mp
        for li, cout in enumerate((64, 128, 256, 512), start=1):
            for bi in range(2):
                p = f'layer{li}.{bi}'
                stride = 2 if (li > 1 and bi == 0) else 1
                ho, wo = osz(hh, 3, stride, 1), osz(ww, 3, stride, 1)
                blk = dict(name=p, stride=stride, x=x_buf)
                w1_, b1_ = self.folded(p + '.conv1', p + '.bn1')
                w2_, b2_ = self.folded(p + '.conv2', p + '.bn2')
                blk['f1'] = cp.conv_fwd_plan(w1_, b1_, stride, 1, dev, p + '.conv1')
                blk['d1'] = self.conv1_dgrad_plan(w1_, stride, cin, batch * hh * ww, p + '.conv1_dgrad')
                blk['f2'] = cp.conv_fwd_plan(w2_, b2_, 1, 1, dev, p + '.conv2')
                blk['d2'] = cp.conv_dgrad_plan(w2_, 1, 1, dev, p + '.conv2_dgrad')
                if p + '.downsample.0.weight' in sd:
                    wd, bd = self.folded(p + '.downsample.0', p + '.downsample.1')
                    blk['fd'] = cp.conv_fwd_plan(wd, bd, stride, 0, dev, p + '.downsample')
                    blk['dd'] = cp.conv_dgrad_plan(wd, stride, 0, dev, p + '.downsample_dgrad')
                    blk['idt'] = z(batch, ho, wo, cout)
                    blk['g_t'] = z(batch, hh, ww, cin)
                blk['o1'] = z(batch, ho, wo, cout)
                blk['out'] = z(batch, ho, wo, cout)
                blk['m_o1'] = self.zb(batch, ho, wo, cout // 4)
                blk['m_out'] = self.zb(batch, ho, wo, cout // 4)
                blk['g_o1'] = z(batch, ho, wo, cout)
                blk['g_x'] = z(batch, hh, ww, cin)
                self.blocks.append(blk)
                x_buf, cin, hh, ww = blk['out'], cout, ho, wo
        self.build_head(512)
        self.g_last = z(batch, hh, ww, 512)
        self.g_c1 = z(batch, h1, w1, 64)
        self.g_in = self.zf(batch, h, w, 4)

    def conv1_dgrad_plan(self, w1, stride, cin, in_pixels, name):
        """The input-gradient plan `d1` of a block's conv1 (`cin` channels on `in_pixels` = batch x H x W pixels): the two routes that
        are not the plan's own choice are decided here."""
        # fp16 storage: the stride-2 input gradients with the four parity classes folded into N (FOLD_S2_F16: 1 layer2.0, 2 all three)
        fold = True if (FOLD_S2_F16 and self.storage == 'f16' and stride == 2 and (cin <= 64 or FOLD_S2_F16 > 1)) else None
        d1 = cp.conv_dgrad_plan(w1, stride, 1, self.dev, name, fold=fold)
        if stride == 2 and cin in (32, 64) and self.storage == 'f32' and in_pixels >= X6P_DGRAD_MIN_PIXELS:
            d74 = cp.conv_dgrad_plan(w1, stride, 1, self.dev, name, fold=False)
            if d74.x6p_ok():
                d74.fixed_tile = 74
                return d74
        return d1

    def forward(self, x4):
        R = _lib.ACT_RELU
        self.stem_f.run(x4, self.c1, act=R)
        pooling.maxpool_fwd(self.c1, self.mp, self.mp_arg, 3, 2, 1)
        masks = self.masks and self.write_masks
        for blk in self.blocks:
            blk['f1'].run(blk['x'], blk['o1'], act=R, mask_out=blk['m_o1'] if masks else None)
            if 'fd' in blk:
                blk['fd'].run(blk['x'], blk['idt'])
                idt = blk['idt']
            else:
                idt = blk['x']
            blk['f2'].run(blk['o1'], blk['out'], add=idt, act=R, mask_out=blk['m_out'] if masks else None)
        return self.head_fwd(self.blocks[-1]['out'])

    def backward(self, g_logits):
        """g_logits [B,ncls] -> gradient w.r.t. the normalised input [B,h,w,4]."""
        self.head_bwd(g_logits, self.blocks[-1]['out'], self.g_last)
        gP = self.g_last
        for i in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[i]
            # the block's input is the previous block's output; block 0's is the max-pool output (gated in maxpool_bwd)
            if self.masks:
                kw2, kw1 = dict(gate_bits=blk['m_o1']), dict(gate_bits=self.blocks[i - 1]['m_out'] if i > 0 else None)
            else:
                kw2, kw1 = dict(gate=blk['o1']), dict(gate=blk['x'] if i > 0 else None)
            blk['d2'].run(gP, blk['g_o1'], **kw2)
            if 'dd' in blk:
                blk['dd'].run(gP, blk['g_t'])
                blk['d1'].run(blk['g_o1'], blk['g_x'], add=blk['g_t'], **kw1)
            else:
                blk['d1'].run(blk['g_o1'], blk['g_x'], add=gP, **kw1)
            gP = blk['g_x']
        if FUSE_POOL_ADJOINT and not self.h16 and gP.is_contiguous() and gP.shape[3] == 64:
            # the pool's adjoint as the prologue of the stem's input gradient (csrc/tapconv_thinmf.hip, POOL): g_c1 -- 205 MB at batch
            # 64 -- is neither written nor read (measured slower, see FUSE_POOL_ADJOINT)
            self.stem_d.run(gP, self.g_in, pool_adjoint=(self.mp_arg, tuple(self.c1.shape[1:3]), True))
            return self.g_in
        pooling.maxpool_bwd(gP, self.mp_arg, self.g_c1, 3, 2, 1, True)
        self.stem_d.run(self.g_c1, self.g_in)
        return self.g_in

    def attention_source(self):
        return self.blocks[-1]['out'], self.g_pooled, True

    def refresh_masks(self):
        """Recompute the gate masks from the activation buffers (after a test has overwritten the activations)."""
        for blk in self.blocks:
            blk['m_o1'].copy_(_lib.pack_gate_mask(blk['o1'].float()))
            blk['m_out'].copy_(_lib.pack_gate_mask(blk['out'].float()))

    def fwd_plans(self):
        yield self.stem_f, self.c1.shape[1:3]
        for blk in self.blocks:
            for k in ('f1', 'f2', 'fd'):
                if k in blk:
                    yield blk[k], blk['out'].shape[1:3]
        yield self.fc_f, (1, 1)


VGG16_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512, 'M']


class VGG16Body(ClassifierBody):
    """torchvision.models.vgg16 (eval: dropout is the identity) forward + input-gradient."""

    def __init__(self, sd, batch, in_hw, dev, storage='f32'):
        super().__init__(sd, batch, in_hw, dev, storage)
        sd, z, zf = self.sd, self.z, self.zf
        h, w = in_hw
        # `ops` in layer order.  Neighbours are facts of construction: a convolution knows the pool that follows it (`pool`) and the
        # convolution directly below it (`below`: its input is that layer's ReLU output and carries its gate); a pool knows the
        # convolution it pools (`conv`).  Everything else is None.
        self.ops = []
        cin, idx, last = 3, 0, None
        for v in VGG16_CFG:
            if v == 'M':
                ho, wo = h // 2, w // 2
                op = dict(kind='pool', hin=h, win=w, c=cin, out=z(batch, ho, wo, cin), arg=self.zb(batch, ho, wo, cin), g=z(batch, h, w, cin), conv=last)
                last['pool'] = op
                h, w = ho, wo
                idx += 1
            else:
                wt, bs = sd[f'features.{idx}.weight'], sd[f'features.{idx}.bias']
                op = dict(kind='conv', f=cp.conv_fwd_plan(wt, bs, 1, 1, dev, f'features.{idx}'),
                          d=cp.conv_dgrad_plan(wt, 1, 1, dev, f'features.{idx}_dgrad'),
                          out=z(batch, h, w, v), g=zf(batch, h, w, 4) if cin == 3 else z(batch, h, w, cin),
                          pool=None, below=last if (last is not None and last['kind'] == 'conv') else None)
                # the ReLU gate of a conv -> conv transition as a byte mask (ClassifierBody.masks), written by the lower layer's epilogue
                if op['below'] is not None and self.masks:
                    op['below']['m'] = self.zb(batch, h, w, cin // 4)
                cin = v
                idx += 2
            self.ops.append(op)
            last = op
        self.feat_hw = (h, w)
        # fp16 storage: conv -> ReLU -> 2 x 2 max-pool in ONE launch (csrc/tapconv_h16p.hip POOL); tests that read the convolution's own
        # activation switch it off on the live body
        self.fuse_pool = FUSE_POOL and storage == 'f16'
        self.pool7 = z(batch, 7, 7, 512)
        self.g_pool7 = z(batch, 7, 7, 512)
        self.g_feat = z(batch, h, w, 512)
        w1 = sd['classifier.0.weight']
        w1p = w1.view(w1.shape[0], 512, 49).permute(0, 2, 1).reshape(w1.shape[0], 49 * 512)  # NCHW flatten -> NHWC
        self.fc = [(cp.linear_fwd_plan(w1p, sd['classifier.0.bias'], dev, 'classifier.0'),
                    cp.linear_dgrad_plan(w1p, dev, 'classifier.0_dgrad')),
                   (cp.linear_fwd_plan(sd['classifier.3.weight'], sd['classifier.3.bias'], dev, 'classifier.3'),
                    cp.linear_dgrad_plan(sd['classifier.3.weight'], dev, 'classifier.3_dgrad')),
                   (cp.linear_fwd_plan(sd['classifier.6.weight'], sd['classifier.6.bias'], dev, 'classifier.6'),
                    cp.linear_dgrad_plan(sd['classifier.6.weight'], dev, 'classifier.6_dgrad'))]
        self.ncls = sd['classifier.6.weight'].shape[0]
        fcw = sd['classifier.0.weight'].shape[0]
        self.h1, self.h2 = z(batch, 1, 1, fcw), z(batch, 1, 1, fcw)
        self.logits = zf(batch, 1, 1, self.ncls)
        self.g_h1, self.g_h2 = z(batch, 1, 1, fcw), z(batch, 1, 1, fcw)

    def pool_fused(self, conv):
        """Does the convolution's own launch pool (forward) / unpool (backward)?  `fuse_pool` is read at run time: tests switch it on a
        live body.  (ConvPlan.run falls back to the separate pooling launch wherever its fused kernel form does not serve the layer.)"""
        return self.fuse_pool and conv['pool'] is not None

    def forward(self, x4):
        B, R = self.B, _lib.ACT_RELU
        t = x4
        for op in self.ops:
            if op['kind'] == 'pool':
                if not self.pool_fused(op['conv']):
                    pooling.maxpool_fwd(t, op['out'], op['arg'], 2, 2, 0)
            elif self.pool_fused(op):
                # conv -> ReLU -> MaxPool2d(2, 2) as one launch where the patch-staged fp16 kernel serves the layer (its epilogue pools:
                # the full-size activation is not written)
                op['f'].run(t, op['out'], act=R, pool=(op['pool']['out'], op['pool']['arg'], self.write_masks))
            else:
                op['f'].run(t, op['out'], act=R, mask_out=op.get('m') if self.write_masks else None)
            op['inp'] = t
            t = op['out']
        if self.feat_hw != (7, 7):
            if self.h16:
                raise NotImplementedError('fp16-storage VGG-16 needs a 224x224 input (7x7 features: no adaptive pooling)')
            pooling.adaptive_avgpool_fwd(t, self.pool7)
            t = self.pool7
        flat = t.view(B, 1, 1, 49 * 512)
        self.fc[0][0].run(flat, self.h1, act=R)
        self.fc[1][0].run(self.h1, self.h2, act=R)
        self.fc[2][0].run(self.h2, self.logits)
        return self.logits.view(B, self.ncls)

    def head_grad(self, g_logits):
        """The head's part of the backward pass alone: g_logits [B, ncls] -> the (ungated) gradient w.r.t. the last pool's output."""
        B = self.B
        self.fc[2][1].run(g_logits.view(B, 1, 1, self.ncls), self.g_h2, gate=self.h2)
        self.fc[1][1].run(self.g_h2, self.g_h1, gate=self.h1)
        self.fc[0][1].run(self.g_h1, self.g_pool7.view(B, 1, 1, 49 * 512))
        g = self.g_pool7
        if self.feat_hw != (7, 7):
            pooling.adaptive_avgpool_bwd(g, None, self.g_feat)
            g = self.g_feat
        return g

    def attention_source(self):
        return self.ops[-1]['out'], self.g_pool7 if self.feat_hw == (7, 7) else self.g_feat, False

    def backward(self, g_logits):
        g = self.head_grad(g_logits)
        # g is the gradient w.r.t. the last pool's output
        for op in reversed(self.ops):
            if op['kind'] == 'pool':
                if self.pool_fused(op['conv']):
                    continue       # (g stays the gradient w.r.t. the pool's output: the convolution below unpools it in its prologue)
                # input of a pool is a conv+ReLU output: gather + ReLU gate -> gradient w.r.t. that conv's pre-activation
                pooling.maxpool_bwd(g, op['arg'], op['g'], 2, 2, 0, True)
            else:
                kw = dict(unpool=(op['pool']['arg'], op['pool']['g'])) if self.pool_fused(op) else {}
                below = op['below']
                if below is not None and 'm' in below:
                    op['d'].run(g, op['g'], gate_bits=below['m'], **kw)
                else:
                    op['d'].run(g, op['g'], gate=below['out'] if below is not None else None, **kw)
            g = op['g']
        return g

    def refresh_masks(self):
        """Recompute the gate masks from the activation buffers (after a test has overwritten the activations)."""
        for op in self.ops:
            if 'm' in op:
                op['m'].copy_(_lib.pack_gate_mask(op['out'].float()))

    def fwd_plans(self):
        for op in self.ops:
            if op['kind'] == 'conv':
                yield op['f'], op['out'].shape[1:3]
        for f, _ in self.fc:
            yield f, (1, 1)


def _inception_body(sd, batch, in_hw, dev, storage='f32'):
    from .inception import InceptionV3Body
    return InceptionV3Body(sd, batch, in_hw, dev, storage)


def _mobilenet_body(sd, batch, in_hw, dev, storage='f32'):
    from .mobilenet import MobileNetV2Body
    return MobileNetV2Body(sd, batch, in_hw, dev, storage)


def _vit_body(sd, batch, in_hw, dev, storage='f32'):
    from .vit import ViTB16Body
    return ViTB16Body(sd, batch, in_hw, dev, storage)


def _convnext_body(sd, batch, in_hw, dev, storage='f32'):
    from .convnext import ConvNeXtBody
    return ConvNeXtBody(sd, batch, in_hw, dev, storage)


BODIES = {'resnet18': ResNet18Body, 'vgg16': VGG16Body, 'inception_v3': _inception_body, 'mobilenet_v2': _mobilenet_body,
          'vit_b_16': _vit_body, 'convnext_tiny': _convnext_body}
LAST_LINEAR = {'vgg16': 'classifier.6', 'mobilenet_v2': 'classifier.1', 'vit_b_16': 'heads.head', 'convnext_tiny': 'classifier.2'}   # the last linear layer's key where it is not 'fc'


NO_FEATURE_MAP = ('vit_b_16',)   # bodies without a convolutional feature map: Grad-CAM and attention= are refused for them
ROLLOUT = ('vit_b_16',)          # ... of which these serve Attention(rollout=True) and Classifier.relevance with an attention rollout


class ClassifierEngine:
    """crop -> area resize -> normalise -> net, forward and input-gradient, for a fixed batch/geometry."""

    def __init__(self, name, state_dict, batch, im_hw, crop_sz, input_sz=None, device='cuda', storage='f32'):
        self.storage = storage
        if name not in BODIES:
            raise NotImplementedError(f'classifier body {name!r} is not implemented on HIP yet (have: {list(BODIES)})')
        self.name, self.B, self.dev = name, batch, torch.device(device)
        self.H, self.W = im_hw
        self.ch, self.cw = crop_sz
        self.cy0, self.cx0 = center_crop_origin(self.H, self.W, crop_sz)
        self.oh, self.ow = tuple(input_sz) if input_sz is not None else INPUT_SZ[name]
        self.body = BODIES[name](state_dict, batch, (self.oh, self.ow), self.dev, storage)
        self.pre = torch.zeros(batch, self.oh, self.ow, 4, device=self.dev)
        self.g_y = torch.zeros(batch, self.H, self.W, 4, device=self.dev)
        import ctypes as C
        self._mean = (C.c_float * 3)(*IMAGENET_MEAN)
        self._std = (C.c_float * 3)(*IMAGENET_STD)
        self.ncls = self.body.ncls
        self.owner = None   # weakref to the attack state this engine is leased to (Classifier.engine)
        self.version = 0    # bumped whenever the activation workspaces are overwritten
        self._grad_ready = False   # the last forward pass wrote what backward() reads (gate masks, arg-max bytes)
        self._cam = None    # the Grad-CAM buffers (attention_buffers())

    def forward(self, y4, need_grad=True):
        """`need_grad=False`: nobody will call backward() on this pass (PerC-AL's second, decision-only forward pass on the quantised
        image, perc_al/__init__.py:220-238): the bodies that write ReLU-gate masks skip them."""
        _lib.check_dev(y4)
        assert y4.shape == (self.B, self.H, self.W, 4)
        self.version += 1
        self._grad_ready = self.body.write_masks = bool(need_grad)
        _lib.call('spaa_preproc_fwd', _lib.ptr(y4), _lib.ptr(self.pre), self.B, self.H, self.W, self.cy0, self.cx0,
                  self.ch, self.cw, self.oh, self.ow, self._mean, self._std)
        return self.body.forward(self.pre)

    def forward_pre(self):
        """The body's forward pass on `pre` as the caller filled it (the One-pixel attacker's spaa_onepixel_preproc writes its
        candidates there): logits [B, ncls].  A decision-only pass, as forward(need_grad=False)."""
        self.version += 1
        self._grad_ready = self.body.write_masks = False
        return self.body.forward(self.pre)

    def attention_buffers(self, rollout=False):
        """Allocates what the Grad-CAM launches write (once; an attack state does it before its loop, so that a captured iteration
        allocates nothing): c [B, h w], its maximum [B], the channel means [B, C] where the body hands over a gradient map, and the
        map M [B, H, W] in the camera frame that attention_map() renders.  `rollout` (Attention.rollout): a body with an attention
        rollout (relevance_grid()) gets c over its patch grid and the body's own workspaces instead; without it such a
        body is refused as before (its attention_source() raises)."""
        if self.storage != 'f32':
            raise NotImplementedError(f"ClassifierEngine: attention with storage={self.storage!r} is not implemented (the feature map and "
                                      "its gradient are read as fp32); use storage='f32'")
        grid = self.body.relevance_grid()
        if grid is not None and not rollout:
            self.body.attention_source()
        if self._cam is None:
            if grid is not None:
                b, (h, w), pooled = self.B, grid, True
                self.body.relevance_buffers()
            else:
                A, G, pooled = self.body.attention_source()
                b, h, w, c = A.shape
            self._cam = dict(c=torch.zeros(b, h * w, device=self.dev), max=torch.zeros(b, device=self.dev),
                             alpha=None if pooled else torch.zeros(b, c, device=self.dev),
                             M=torch.zeros(b, self.H, self.W, device=self.dev), hw=(h, w), valid=False)
        return self._cam

    def grad_cam(self, g_logits, target):
        """c and its per-sample maximum from the feature map and the gradient of the last backward pass -- or of
        body.head_grad(g_logits) alone -- with the seed g_logits[b, target[b]].  `target`: int32 [B] on the device."""
        cam = self.attention_buffers()
        A, G, pooled = self.body.attention_source()
        _lib.check_dev(A, G, g_logits)
        b, h, w, c = A.shape
        if target.dtype != torch.int32 or tuple(target.shape) != (b,) or tuple(g_logits.shape) != (b, self.ncls) or c % 4:
            raise ValueError(f'ClassifierEngine.grad_cam: target must be int32 [{b}] and g_logits [{b}, {self.ncls}] (got {target.dtype} '
                             f'{tuple(target.shape)}, {tuple(g_logits.shape)}); the feature map needs whole channel quads (C = {c})')
        p = _lib.ptr
        if pooled:
            if G.numel() != b * c:
                raise ValueError(f'ClassifierEngine.grad_cam: the pooled gradient must hold {b} x {c} values, got {tuple(G.shape)}')
            alpha, scale = G, 1.0 / (h * w)
        else:
            if G.shape != A.shape:
                raise ValueError(f'ClassifierEngine.grad_cam: gradient map {tuple(G.shape)} against feature map {tuple(A.shape)}')
            _lib.call('spaa_cam_alpha', p(G), p(cam['alpha']), b, h * w, c, c)
            alpha, scale = cam['alpha'], 1.0
        _lib.call('spaa_cam_map', p(A), p(alpha), scale, p(g_logits), self.ncls, p(target), p(cam['c']), p(cam['max']), b, h * w, c)
        cam['valid'] = True
        return cam

    def attention_apply(self, floor, g_y=None, M_out=None):
        """spaa_attention_apply of the last grad_cam(): weights `g_y` in place and / or writes M into `M_out` [B, H, W]."""
        cam = self._cam
        if cam is None or not cam['valid']:
            raise RuntimeError('ClassifierEngine: no class-activation map yet (backward(..., attention=...) or grad_cam() computes one)')
        fh, fw = cam['hw']
        _lib.call('spaa_attention_apply', _lib.ptr(cam['c']), _lib.ptr(cam['max']), float(floor), _lib.ptr(g_y), _lib.ptr(M_out), self.B,
                  self.H, self.W, self.cy0, self.cx0, self.ch, self.cw, fh, fw)

    def attention_map(self):
        """M of the last grad_cam() (or rollout) in the camera frame, [B, 1, H, W] (0 outside the classifier crop): a copy."""
        cam = self._cam if self._cam is not None else self.attention_buffers()
        self.attention_apply(0.0, None, cam['M'])
        return cam['M'].view(self.B, 1, self.H, self.W).clone()

    def _relevance_args(self, g_logits, target):
        """What body.backward(..., relevance=) takes: (target, c, cmax) of the rollout buffers, after the checks grad_cam() makes."""
        cam = self.attention_buffers(rollout=True)
        _lib.check_dev(g_logits)
        if target.dtype != torch.int32 or tuple(target.shape) != (self.B,) or tuple(g_logits.shape) != (self.B, self.ncls):
            raise ValueError(f'ClassifierEngine.backward: target must be int32 [{self.B}] and g_logits [{self.B}, {self.ncls}] (got '
                             f'{target.dtype} {tuple(target.shape)}, {tuple(g_logits.shape)})')
        _lib._same_device(target)
        return target, cam['c'], cam['max']

    def backward(self, g_logits, attention=None, target=None):
        """The gradient image at the camera frame.  `attention` (an Attention; with `target`, the samples' classes as int32 [B]): the
        image is weighted by floor + (1 - floor) M, M the Grad-CAM map of this pass (attention_map() returns it) -- for a body with an
        attention rollout and `attention.rollout`, the rollout map that the body's backward pass writes on its way."""
        if attention is not None and not isinstance(attention, Attention):
            raise TypeError(f'ClassifierEngine.backward: attention must be a spaa_amd.Attention or None, got {type(attention).__name__}')
        if attention is not None and target is None:
            raise ValueError('ClassifierEngine.backward: attention needs `target` (the class of every sample)')
        if not self._grad_ready:
            # (a need_grad=False pass overwrote the activations but left the ReLU-gate masks / pool arg-max bytes of the pass before it)
            raise RuntimeError('ClassifierEngine.backward(): the last forward() ran with need_grad=False (its gate masks were not '
                               'written); run forward(..., need_grad=True) first')
        rollout = attention is not None and attention.rollout and self.body.relevance_grid() is not None
        if rollout:
            g_pre = self.body.backward(g_logits, relevance=self._relevance_args(g_logits, target))
            self._cam['valid'] = True
        else:
            g_pre = self.body.backward(g_logits)
        _lib.call('spaa_preproc_bwd', _lib.ptr(g_pre), _lib.ptr(self.g_y), self.B, self.H, self.W, self.cy0, self.cx0,
                  self.ch, self.cw, self.oh, self.ow, self._std)
        if attention is not None:
            if not rollout:
                self.grad_cam(g_logits, target)
            self.attention_apply(attention.floor, g_y=self.g_y)
        return self.g_y


def _classify_impl(clf, im, crop_sz):
    """spaa::classify.  Returns (logits [B,ncls], saved)."""
    b, _, h, w = im.shape
    with _lib.on_device(im.device):
        eng = clf.engine(b, (h, w), tuple(crop_sz))
        im4 = to_nhwc4(im)
        logits = eng.forward(im4).clone()
        saved = dict(eng=eng, version=eng.version, im4=im4, clf=weakref.ref(clf), key=(b, (h, w), tuple(crop_sz)))
        clf._last_saved = saved
        return logits, saved


def _classify_backward_impl(saved, g):
    eng = saved['eng']
    with _lib.on_device(g.device):
        if eng.version != saved['version']:  # workspaces reused by a later forward: recompute this call's activations
            if eng.owner is not None and eng.owner() is not None and saved['clf']() is not None:
                # ... and the engine has since been leased to an attack state: leave ITS workspaces alone, take a free engine
                eng = saved['eng'] = saved['clf']().engine(*saved['key'])
            eng.forward(saved['im4'])
            saved['version'] = eng.version
        return to_nchw(eng.backward(g.detach().float().contiguous()))


class Classifier(object):
    """classifier.py:12-75 on HIP.  Extra keyword arguments: `state_dict`/`weights_path` (no download here) and
    `input_sz` (tests use reduced sizes)."""

    def __init__(self, model_name, device, device_ids=(0,), fix_params=True, sort_results=True, state_dict=None,
                 weights_path=None, input_sz=None):
        self.name = model_name
        self.fix_params = fix_params
        self.device = torch.device(device)
        self.sort_results = sort_results
        if model_name not in INPUT_SZ:
            raise ValueError(f'unknown classifier {model_name!r}')
        self.input_sz = tuple(input_sz) if input_sz is not None else INPUT_SZ[model_name]
        if state_dict is None and weights_path is not None:
            state_dict = torch.load(weights_path, map_location='cpu')
        if state_dict is None:
            raise RuntimeError('no network access: pass state_dict= (torchvision key names) or weights_path= instead of '
                               'the pretrained-weights URL the reference downloads (classifier.py:24-36)')
        if not fix_params:
            raise NotImplementedError('spaa_amd classifiers are frozen (input gradients only)')
        self.state_dict = {k: v.detach().float().cpu() for k, v in _strip(state_dict).items()}
        if model_name == 'vit_b_16':
            # what the ViT body does not serve (input size against patch size and position embedding, width against the 12 heads): said
            # here, on the CPU, before any engine is built
            from . import vit
            self.state_dict = vit.canonical(self.state_dict)
            vit.check_geometry(self.state_dict, self.input_sz)
        if model_name == 'convnext_tiny':
            # likewise: input size against the stem and the downsamples, widths against the channel quads of the kernels
            from . import convnext
            convnext.check_geometry(self.state_dict, self.input_sz)
        self._engines = {}

    @property
    def num_classes(self):
        """Rows of the last linear layer (what an engine reports as `ncls`), read from the weights: no engine is built."""
        return int(self.state_dict[LAST_LINEAR.get(self.name, 'fc') + '.weight'].shape[0])

    @property
    def has_feature_map(self):
        """Does the body end in a convolutional feature map that Grad-CAM can read?  (Every body but the vision transformer.)"""
        return self.name not in NO_FEATURE_MAP

    @property
    def has_rollout(self):
        """Does the body write an attention-rollout map in its backward pass?  (The vision transformer.)"""
        return self.name in ROLLOUT

    def engine(self, batch, im_hw, crop_sz, owner=None, storage='f32'):
        """Cached engine for a batch size / geometry; an engine leased to an `owner` (attack state) is not handed to
        anyone else while the owner lives (see PCNet.engine).  `storage`: 'f32' or 'f16' (fp16 activations in HBM)."""
        key = (batch, tuple(im_hw), tuple(crop_sz), storage)
        pool = self._engines.setdefault(key, [])
        for e in pool:
            if e.owner is None or e.owner() is None:
                break
        else:
            with _lib.on_device(self.device):
                e = ClassifierEngine(self.name, self.state_dict, batch, im_hw, crop_sz, self.input_sz, self.device, storage)
            pool.append(e)
        e.owner = weakref.ref(owner) if owner is not None else None
        return e

    def classify(self, im, crop_sz=(240, 240)):
        if im.dtype == torch.uint8:
            im = im.type(torch.float32) / 255
        while im.ndim < 4:
            im = im[None]
        if self.device.type != 'cuda':
            raise RuntimeError('spaa_amd.Classifier runs on the GPU only (no CPU fallback); got device=%s' % self.device)
        from . import ops
        raw_score = torch.ops.spaa.classify(im.to(self.device), ops.handle_of(self), int(crop_sz[0]), int(crop_sz[1]))
        # Compatibility outputs (classifier.py:64-72).  The fused attack loop does NOT use these: it takes top-1 and
        # its probability on device (spaa_decide); the full 1000-way sort is only done for API parity here.
        p = torch.softmax(raw_score.detach(), dim=1).cpu()
        if self.sort_results:
            p_sorted, idx = p.sort(descending=True)
        else:
            p_sorted, idx = p, torch.arange(p.shape[1]).repeat(p.shape[0], 1)
        return raw_score, p_sorted.numpy(), idx.numpy()

    def __call__(self, im, crop_sz):
        return self.classify(im, crop_sz)

    def grad_cam(self, im, class_idx, crop_sz=(240, 240)):
        """Where the classifier looks for `class_idx` (a list of B classes) in `im` [B, 3, H, W] on the GPU: the Grad-CAM map M of
        DESIGN.md 7h as float32 [B, 1, H, W] on the device, in [0, 1], 0 outside the classifier crop.  One forward pass and the
        head's part of the backward pass (the body's backward pass does not run)."""
        if not self.has_feature_map:
            raise NotImplementedError(f'grad_cam: Grad-CAM is not implemented for {self.name} (the body has no convolutional feature map)')
        im, classes = self._map_inputs('grad_cam', im, class_idx)
        b, _, h, w = im.shape
        with _lib.on_device(im.device):
            eng = self.engine(b, (h, w), tuple(crop_sz))
            eng.attention_buffers()
            eng.forward(to_nhwc4(im.float().contiguous()), need_grad=False)
            seed, target = self._one_hot(classes, eng.ncls, im.device)
            eng.body.head_grad(seed)
            eng.grad_cam(seed, target)
            return eng.attention_map()

    def _map_inputs(self, who, im, class_idx):
        """The checks grad_cam() and relevance() share: (im as float [B, 3, H, W] on the device, the classes as ints)."""
        if self.device.type != 'cuda':
            raise RuntimeError('spaa_amd.Classifier runs on the GPU only (no CPU fallback); got device=%s' % self.device)
        if im.dtype == torch.uint8:
            im = im.type(torch.float32) / 255
        if im.ndim != 4 or im.shape[1] != 3:
            raise ValueError(f'{who}: im must be [B, 3, H, W], got {tuple(im.shape)}')
        classes = [int(c) for c in class_idx]
        b = im.shape[0]
        if len(classes) != b or any(not 0 <= c < self.num_classes for c in classes):
            raise ValueError(f'{who}: class_idx must hold {b} classes in [0, {self.num_classes}), got {classes}')
        return im.to(self.device), classes

    @staticmethod
    def _one_hot(classes, ncls, dev):
        """(seed [B, ncls] with 1 at each sample's class, target int32 [B]) on `dev`."""
        target = torch.tensor(classes, dtype=torch.int32, device=dev)
        seed = torch.zeros(len(classes), ncls, device=dev)
        seed[torch.arange(len(classes), device=dev), target.long()] = 1.0
        return seed, target

    def relevance(self, im, class_idx, crop_sz=(240, 240)):
        """Where the classifier looks for `class_idx`, whatever its body: float32 [B, 1, H, W] on the device, in [0, 1], 0 outside the
        classifier crop.  For vit_b_16 the gradient-weighted attention rollout of the class token over the patch
        grid, resampled onto the crop as Grad-CAM's map is: one forward and one backward pass of the body.  For a convolutional
        body grad_cam()'s map."""
        if not self.has_rollout:
            return self.grad_cam(im, class_idx, crop_sz)
        im, classes = self._map_inputs('relevance', im, class_idx)
        b, _, h, w = im.shape
        with _lib.on_device(im.device):
            eng = self.engine(b, (h, w), tuple(crop_sz))
            eng.attention_buffers(rollout=True)
            eng.forward(to_nhwc4(im.float().contiguous()))
            seed, target = self._one_hot(classes, eng.ncls, im.device)
            eng.body.backward(seed, relevance=eng._relevance_args(seed, target))
            eng._cam['valid'] = True
            return eng.attention_map()


def load_imagenet_labels(filename):
    """classifier.py:109-116 (the label file is a Python dict literal)."""
    import ast
    with open(filename) as f:
        labels = ast.literal_eval(f.read())
    return {k: v.split(',')[0] for k, v in labels.items()}
