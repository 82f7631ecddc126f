"""ViT-B/16 (torchvision.models.vit_b_16, eval) forward and input-gradient: every linear layer (patch embedding, QKV, output
projection, MLP, head) on the tap-list convolution plans (spaa_amd/convplan.py) over the token map [B, T, 1, C], and LayerNorm, exact
GELU, softmax attention and the patch / token bookkeeping on the kernels of csrc/vit_ops.hip.

The architecture is third-party; it is restated here from its published definition (Dosovitskiy et al., "An Image is Worth 16x16
Words: Transformers for Image Recognition at Scale", 2020) with torchvision's key names: `conv_proj` the P x P / stride-P patch
embedding, `class_token`, `encoder.pos_embedding`, `encoder.layers.encoder_layer_{i}` with `ln_1`, `self_attention.in_proj_{weight,
bias}` (rows q, then k, then v), `self_attention.out_proj`, `ln_2`, `mlp.0` / `mlp.3` (older checkpoints: `mlp.linear_1` /
`mlp.linear_2`), `encoder.ln` and `heads.head`.  Every LayerNorm has eps 1e-6, GELU is the exact erf form, dropout is the identity.

  x = [class_token; conv_proj(image) flattened row-major] + pos_embedding                      [B, T, D]
  per layer:  x = x + out_proj(MHA(ln_1(x)));  x = x + mlp.3(gelu(mlp.0(ln_2(x))))
  logits = heads.head(encoder.ln(x[:, 0]))

D, the depth, the MLP width, P and T are read from the state dict.  The number of heads is not in it and is fixed at 12.  This
implementation needs D % 48 == 0 (head width dh = D / 12 a multiple of 4), dh <= 64 and T <= 256, the input height and width multiples
of P, and (h / P)(w / P) + 1 == T (the position embedding is not interpolated).

The patch embedding: spaa_vit_patchify gathers each patch into a row of 4 P^2 floats and `conv_proj` runs as a 1 x 1 plan over
K = 4 P^2 (the tap lists hold at most 64 taps, a 16 x 16 kernel has 256), its weight rearranged on the host with zeros for the fourth
input channel.

Saved per layer for the backward pass: the block input x, x_mid (after the attention residual), the two (mean, rstd) pairs, qkv, ctx,
lse and the MLP's pre-activation: (6 D + M) floats per token, 0.39 GB per layer and 4.6 GB in all at B = 64 with the real widths.
The probabilities are not kept (119 MB per layer at B = 64): the attention adjoint recomputes them from lse.

Grad-CAM has no meaning here (there is no convolutional feature map): attention_source() raises.  What the body offers instead is the
gradient-weighted attention rollout of its class token (Chefer, Gur and Wolf 2021), written by backward(g_logits,
relevance=...) on its way down the layers from what the attention adjoint reads anyway.  fp16 storage is not implemented.
"""
import torch

from . import _lib
from . import convplan as cp
from .classifier import ClassifierBody, _strip

HEADS = 12
LN_EPS = 1e-6
MAX_T, MAX_DH = 256, 64
LAYER = 'encoder.layers.encoder_layer_{}.'
ALIASES = {'mlp.linear_1.': 'mlp.0.', 'mlp.linear_2.': 'mlp.3.'}


def canonical(sd):
    """The state dict with `module.` prefixes stripped and the older `mlp.linear_1` / `mlp.linear_2` names as `mlp.0` / `mlp.3`."""
    out = {}
    for k, v in _strip(sd).items():
        for old, new in ALIASES.items():
            k = k.replace(old, new)
        out[k] = v
    return out


def config(sd):
    """(D, depth, mlp_dim, P, T) as the state dict `sd` (canonical names) has them."""
    w = sd['conv_proj.weight']
    depth = 0
    while LAYER.format(depth) + 'ln_1.weight' in sd:
        depth += 1
    return int(w.shape[0]), depth, int(sd[LAYER.format(0) + 'mlp.0.weight'].shape[0]), int(w.shape[2]), int(sd['encoder.pos_embedding'].shape[1])


def check_geometry(sd, input_sz):
    """ValueError where this implementation does not serve the network `sd` at the input size `input_sz` (nothing is allocated)."""
    D, depth, _, P, T = config(sd)
    h, w = input_sz
    if depth < 1:
        raise ValueError('vit_b_16: the state dict has no encoder layer (encoder.layers.encoder_layer_0.*)')
    if h % P or w % P or h < P or w < P:
        raise ValueError(f'vit_b_16: input_sz {tuple(input_sz)} must be a multiple of the patch size {P} in both directions')
    if (h // P) * (w // P) + 1 != T:
        raise ValueError(f'vit_b_16: input_sz {tuple(input_sz)} gives {(h // P) * (w // P)} patches + the class token, but pos_embedding '
                         f'has {T} rows (the position embedding is not interpolated)')
    if D % (4 * HEADS):
        raise ValueError(f'vit_b_16: the width D = {D} must be a multiple of {4 * HEADS} ({HEADS} heads of a width that is a multiple of 4)')
    if D // HEADS > MAX_DH or T > MAX_T:
        raise ValueError(f'vit_b_16: head width {D // HEADS} (at most {MAX_DH}) / {T} tokens (at most {MAX_T}) are beyond the attention kernels')


def patch_weight(w):
    """conv_proj.weight [D, 3, P, P] -> [D, 4 P P, 1, 1] in the column order of spaa_vit_patchify ((ky P + kx) 4 + c, zeros for c = 3)."""
    d, c, p, _ = w.shape
    w4 = torch.zeros(d, p, p, 4, dtype=w.dtype)
    w4[..., :c] = w.permute(0, 2, 3, 1)
    return w4.reshape(d, 4 * p * p, 1, 1).contiguous()


class ViTB16Body(ClassifierBody):
    body_masks_switch = False

    def __init__(self, sd, batch, in_hw, dev, storage='f32'):
        if storage != 'f32':
            raise NotImplementedError(f"ViTB16Body: storage={storage!r} is not implemented (LayerNorm, GELU and attention are fp32); use storage='f32'")
        sd = canonical(sd)
        check_geometry(sd, in_hw)
        super().__init__(sd, batch, in_hw, dev, storage)
        sd, zf, B = self.sd, self.zf, batch
        h, w = in_hw
        self.D, self.depth, self.M, self.P, self.T = D, depth, M, P, T = config(sd)
        self.n, self.dh = T - 1, D // HEADS
        n = self.n

        def lin(key, name):
            wt = sd[key + '.weight'] if key + '.weight' in sd else sd[key + '_weight']
            bs = sd[key + '.bias'] if key + '.bias' in sd else sd[key + '_bias']
            wt = wt.reshape(wt.shape[0], wt.shape[1], 1, 1)
            return cp.conv_fwd_plan(wt, bs, 1, 0, dev, name), cp.conv_dgrad_plan(wt, 1, 0, dev, name + '_dgrad')

        def vec(key):
            return sd[key].detach().float().reshape(-1).contiguous().to(dev)

        wp = patch_weight(sd['conv_proj.weight'].detach().float().cpu())
        self.proj_f = cp.conv_fwd_plan(wp, sd['conv_proj.bias'], 1, 0, dev, 'conv_proj')
        self.proj_d = cp.conv_dgrad_plan(wp, 1, 0, dev, 'conv_proj_dgrad')
        self.cls, self.pos = vec('class_token'), vec('encoder.pos_embedding')
        self.patches, self.g_patches = zf(B, n, 1, 4 * P * P), zf(B, n, 1, 4 * P * P)
        self.emb, self.g_emb = zf(B, n, 1, D), zf(B, n, 1, D)
        self.x0 = zf(B, T, 1, D)
        self.layers = []
        x = self.x0
        for i in range(depth):
            p = LAYER.format(i)
            ly = dict(name=p[:-1], x=x)
            ly['ln1'], ly['ln2'] = (vec(p + 'ln_1.weight'), vec(p + 'ln_1.bias')), (vec(p + 'ln_2.weight'), vec(p + 'ln_2.bias'))
            ly['in_f'], ly['in_d'] = lin(p + 'self_attention.in_proj', ly['name'] + '.in_proj')
            ly['out_f'], ly['out_d'] = lin(p + 'self_attention.out_proj', ly['name'] + '.out_proj')
            ly['m0_f'], ly['m0_d'] = lin(p + 'mlp.0', ly['name'] + '.mlp.0')
            ly['m3_f'], ly['m3_d'] = lin(p + 'mlp.3', ly['name'] + '.mlp.3')
            # what the backward pass reads
            ly['st1'], ly['st2'] = (zf(B * T), zf(B * T)), (zf(B * T), zf(B * T))
            ly['qkv'], ly['ctx'], ly['lse'] = zf(B, T, 1, 3 * D), zf(B, T, 1, D), zf(B, HEADS, T)
            ly['x_mid'], ly['pre'], ly['out'] = zf(B, T, 1, D), zf(B, T, 1, M), zf(B, T, 1, D)
            self.layers.append(ly)
            x = ly['out']
        # shared between the layers: the LayerNorm outputs, the GELU output and every gradient but the one the head writes
        self.nrm, self.act = zf(B, T, 1, D), zf(B, T, 1, M)
        self.g_act, self.g_n, self.g_ctx, self.g_qkv = zf(B, T, 1, M), zf(B, T, 1, D), zf(B, T, 1, D), zf(B, T, 1, 3 * D)
        self.g_mid, self.g_x, self.delta = zf(B, T, 1, D), (zf(B, T, 1, D), zf(B, T, 1, D)), zf(B, HEADS, T)
        # The head's gradient reaches token 0 only: spaa_layernorm_bwd writes those B rows (row stride T D) and nothing ever writes the
        # others, which stay the zeros they were allocated as.
        self.g_top = zf(B, T, 1, D)
        self.ln = (vec('encoder.ln.weight'), vec('encoder.ln.bias'))
        self.st_head = (zf(B), zf(B))
        self.ncls = sd['heads.head.weight'].shape[0]
        self.hn, self.g_hn = zf(B, 1, 1, D), zf(B, 1, 1, D)
        self.fc_f = cp.linear_fwd_plan(sd['heads.head.weight'], sd['heads.head.bias'], dev, 'heads.head')
        self.fc_d = cp.linear_dgrad_plan(sd['heads.head.weight'], dev, 'heads.head_dgrad')
        self.logits = zf(B, 1, 1, self.ncls)
        self.g_in = zf(B, h, w, 4)
        self.rho = self.rho_heads = None   # the rollout's workspaces (relevance_buffers())

    # ---- the launches of csrc/vit_ops.hip ------------------------------------------------------------------------------------------
    def ln_fwd(self, x, wb, y, st, rows=None, x_stride=None):
        D = self.D
        _lib.call('spaa_layernorm_fwd', _lib.ptr(x), x_stride or D, _lib.ptr(wb[0]), _lib.ptr(wb[1]), _lib.ptr(y), D, _lib.ptr(st[0]), _lib.ptr(st[1]),
                  rows or self.B * self.T, D, LN_EPS)

    def ln_bwd(self, g, x, wb, st, add, gx, rows=None, wide=None):
        """`wide`: the row stride of x and gx where they are the class-token rows of a [B, T, D] tensor (g is dense)."""
        D = self.D
        _lib.call('spaa_layernorm_bwd', _lib.ptr(g), D, _lib.ptr(x), wide or D, _lib.ptr(wb[0]), _lib.ptr(st[0]), _lib.ptr(st[1]), _lib.ptr(add), D,
                  _lib.ptr(gx), wide or D, rows or self.B * self.T, D)

    # ---- execution -----------------------------------------------------------------------------------------------------------------
    def forward(self, x4):
        p, B, T, D = _lib.ptr, self.B, self.T, self.D
        h, w = self.in_hw
        _lib.call('spaa_vit_patchify', p(x4), p(self.patches), B, h, w, self.P)
        self.proj_f.run(self.patches, self.emb)
        _lib.call('spaa_vit_assemble', p(self.emb), p(self.cls), p(self.pos), p(self.x0), B, T, D)
        for ly in self.layers:
            self.ln_fwd(ly['x'], ly['ln1'], self.nrm, ly['st1'])
            ly['in_f'].run(self.nrm, ly['qkv'])
            _lib.call('spaa_attn_fwd', p(ly['qkv']), p(ly['ctx']), p(ly['lse']), B, T, HEADS, self.dh)
            ly['out_f'].run(ly['ctx'], ly['x_mid'], add=ly['x'])
            self.ln_fwd(ly['x_mid'], ly['ln2'], self.nrm, ly['st2'])
            ly['m0_f'].run(self.nrm, ly['pre'])
            _lib.call('spaa_gelu_fwd', p(ly['pre']), p(self.act), B * T * self.M)
            ly['m3_f'].run(self.act, ly['out'], add=ly['x_mid'])
        self.ln_fwd(self.layers[-1]['out'], self.ln, self.hn, self.st_head, rows=B, x_stride=T * D)
        self.fc_f.run(self.hn, self.logits)
        return self.logits.view(B, self.ncls)

    def head_grad(self, g_logits):
        """g_logits [B, ncls] -> the gradient at the normalised class token [B, 1, 1, D]."""
        self.fc_d.run(g_logits.view(self.B, 1, 1, self.ncls), self.g_hn)
        return self.g_hn

    def relevance_grid(self):
        return self.in_hw[0] // self.P, self.in_hw[1] // self.P

    def relevance_buffers(self):
        """The rollout's workspaces (allocated once, by the engine's attention_buffers() before an attack's loop): the two rho [B, T]
        that the layers alternate between and the per-head sums [B, heads, T]."""
        if self.rho is None:
            self.rho, self.rho_heads = (self.zf(self.B, self.T), self.zf(self.B, self.T)), self.zf(self.B, HEADS, self.T)
        return self.rho

    def backward(self, g_logits, relevance=None):
        """g_logits [B, ncls] -> gradient w.r.t. the normalised input [B, h, w, 4].  `relevance` = (target int32 [B], c [B, T - 1],
        cmax [B]): the pass also writes the class token's attention-rollout map of each sample's class `target` into c
        and its maximum into cmax -- one spaa_attn_relevance after each layer's attention adjoint, whose inputs it shares, and
        spaa_relevance_map at the end.  g_logits must be zero but at the targets (the seed is divided out)."""
        p, B, T, D = _lib.ptr, self.B, self.T, self.D
        h, w = self.in_hw
        if relevance is not None:
            target, c, cmax = relevance
            rho, rho_in = self.relevance_buffers(), None
        self.ln_bwd(self.head_grad(g_logits), self.layers[-1]['out'], self.ln, self.st_head, None, self.g_top, rows=B, wide=T * D)
        g = self.g_top
        for i in range(self.depth - 1, -1, -1):
            ly = self.layers[i]
            ly['m3_d'].run(g, self.g_act)
            _lib.call('spaa_gelu_bwd', p(self.g_act), p(ly['pre']), p(self.g_act), B * T * self.M)
            ly['m0_d'].run(self.g_act, self.g_n)
            self.ln_bwd(self.g_n, ly['x_mid'], ly['ln2'], ly['st2'], g, self.g_mid)
            ly['out_d'].run(self.g_mid, self.g_ctx)
            _lib.call('spaa_attn_bwd', p(ly['qkv']), p(ly['ctx']), p(ly['lse']), p(self.g_ctx), p(self.g_qkv), p(self.delta), B, T, HEADS, self.dh)
            if relevance is not None:
                _lib.call('spaa_attn_relevance', p(ly['qkv']), p(ly['lse']), p(self.g_ctx), p(rho_in), p(g_logits), self.ncls, p(target),
                          p(self.rho_heads), p(rho[i & 1]), B, T, HEADS, self.dh)
                rho_in = rho[i & 1]
            ly['in_d'].run(self.g_qkv, self.g_n)
            self.ln_bwd(self.g_n, ly['x'], ly['ln1'], ly['st1'], self.g_mid, self.g_x[i & 1])
            g = self.g_x[i & 1]
        if relevance is not None:
            _lib.call('spaa_relevance_map', p(rho_in), p(g_logits), self.ncls, p(target), p(c), p(cmax), B, T)
        _lib.call('spaa_vit_assemble_bwd', p(g), p(self.g_emb), B, T, D)
        self.proj_d.run(self.g_emb, self.g_patches)
        _lib.call('spaa_vit_unpatchify', p(self.g_patches), p(self.g_in), B, h, w, self.P)
        return self.g_in

    def attention_source(self):
        raise NotImplementedError('ViTB16Body: Grad-CAM is not implemented for vit_b_16 (the body has no convolutional feature map)')

    def refresh_masks(self):
        """Nothing to do: the body has no gates (GELU is smooth; its adjoint reads the pre-activation itself)."""

    def fwd_plans(self):
        yield self.proj_f, (self.n, 1)
        for ly in self.layers:
            for k in ('in_f', 'out_f', 'm0_f', 'm3_f'):
                yield ly[k], (self.T, 1)
        yield self.fc_f, (1, 1)

    def flops_attention(self):
        """Algorithmic FLOPs (2 x MAC) of q k^T and p v over all layers, forward."""
        return self.depth * 4 * self.B * self.T * self.T * self.D

    def flops_fwd(self):
        return super().flops_fwd() + self.flops_attention()
