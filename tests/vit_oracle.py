"""TEST INFRASTRUCTURE: the float64 restatement of torchvision's vit_b_16 (eval) in plain torch, the per-kernel restatements that
tests/test_vit_ops_gpu.py holds csrc/vit_ops.hip to, the fixtures of tests/test_vit_gpu.py, the bars with their derivations, and
`MUTATIONS`: the same functions with one deliberate mistake each (tests/test_vit_cpu.py shows that every one lands beyond its bar on
the inputs the GPU tests use, so a kernel that made the mistake could not pass them).

Definition (Dosovitskiy et al. 2020; torchvision's key names).  D = conv_proj's output channels, P its kernel size, T the rows of
encoder.pos_embedding, 12 heads of dh = D / 12, eps 1e-6 in every LayerNorm:
  tokens = conv_proj(x) (P x P, stride P, no padding) flattened row-major; x = [class_token; tokens] + pos_embedding
  per layer: x = x + out_proj(MHA(ln_1(x))), x = x + mlp.3(gelu(mlp.0(ln_2(x)))); in_proj rows are q, then k, then v; scores
  q k^T / sqrt(dh), softmax over keys, heads concatenated in order; GELU is x Phi(x)
  logits = heads.head(encoder.ln(x[:, 0]))

Bars.  U = 2^-24 is the unit roundoff of fp32.  A sum of n fp32 terms in ANY order is within (n - 1) U sum|terms| of the exact sum to
first order, a product or a fused multiply-add adds U of its result; the bars below are these first-order bounds, evaluated in float64
on the magnitudes that the kernel sums, times SLACK = 2 for the second-order terms.  expf, logf and erfcf come from the device
library; their error is not derived but measured: torch's own fp32 evaluation of the same function of the same fp32 arguments on the
CPU against float64 (`measured_rel`), and the bars allow LIBM = 4 times that for a different library's rounding."""
import math

import torch
import torch.nn.functional as F

import spaa_oracle as so
from spaa_amd import synthetic as syn

U = 2.0 ** -24
SLACK = 2.0
LIBM = 4.0
HEADS = 12
EPS = 1e-6
FLT_MIN = 2.0 ** -126


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------------- the kernels, restated
def patchify(x4, P, _bug=None):
    """[B, h, w, 4] -> [B n, 4 P P]: tokens row-major over the patch grid, column (ky P + kx) 4 + c."""
    b, h, w, c = x4.shape
    t = x4.reshape(b, h // P, P, w // P, P, c)
    t = t.permute(0, 3, 1, 2, 4, 5) if _bug == 'column_major_tokens' else t.permute(0, 1, 3, 2, 4, 5)
    return t.reshape(b * (h // P) * (w // P), P * P * c)


def unpatchify(gp, B, h, w, P):
    """The adjoint of patchify: [B n, 4 P P] -> [B, h, w, 4]."""
    return gp.reshape(B, h // P, w // P, P, P, 4).permute(0, 1, 3, 2, 4, 5).reshape(B, h, w, 4)


def assemble(emb, cls, pos, _bug=None):
    """emb [B, n, D], cls [D], pos [T, D] -> [B, T, D]."""
    b = emb.shape[0]
    x = torch.cat([cls.reshape(1, 1, -1).expand(b, -1, -1), emb], dim=1) + pos.reshape(1, *pos.shape[-2:])
    if _bug == 'class_token_without_pos':
        x = torch.cat([x[:, :1] - pos.reshape(-1, pos.shape[-1])[0], x[:, 1:]], dim=1)
    return x


def layernorm(x, w, b, eps=EPS, _bug=None):
    """Rows of x [..., D] -> (y, mean, rstd): biased variance."""
    if _bug == 'eps_1e-5':
        eps = 1e-5
    mu = x.mean(dim=-1, keepdim=True)
    c = x - mu
    var = (c * c).sum(dim=-1, keepdim=True) / (x.shape[-1] - 1 if _bug == 'unbiased_variance' else x.shape[-1])
    rs = 1.0 / torch.sqrt(var + eps)
    return c * rs * w + b, mu.squeeze(-1), rs.squeeze(-1)


def layernorm_bwd(g, x, w, mean, rstd, add=None, _bug=None):
    """gx = rstd (gh - mean(gh) - xh mean(gh xh)) (+ add), gh = g w, xh = (x - mean) rstd, with the mean and rstd GIVEN."""
    gh, xh = g * w, (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    m1, m2 = gh.mean(dim=-1, keepdim=True), (gh * xh).mean(dim=-1, keepdim=True)
    if _bug == 'ln_bwd_without_xhat_term':
        m2 = torch.zeros_like(m2)
    gx = rstd.unsqueeze(-1) * (gh - m1 - xh * m2)
    return gx if add is None else gx + add


def Phi(x):
    return 0.5 * torch.special.erfc(-x * 0.7071067811865476)


def phi(x):
    return 0.3989422804014327 * torch.exp(-0.5 * x * x)


def gelu(x, _bug=None):
    if _bug == 'tanh_gelu':
        return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return x * Phi(x)


def gelu_bwd(g, x, _bug=None):
    if _bug == 'tanh_gelu':
        t = torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3))
        return g * (0.5 * (1 + t) + 0.5 * x * (1 - t * t) * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x))
    return g * (Phi(x) + x * phi(x))


def split_heads(qkv, heads, _bug=None):
    """qkv [B, T, 3 D] -> q, k, v [B, heads, T, dh]."""
    b, t, d3 = qkv.shape
    d = d3 // 3
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    if _bug == 'k_v_swapped':
        k, v = v, k
    sh = lambda m: m.reshape(b, t, heads, d // heads).permute(0, 2, 1, 3)     # noqa: E731
    return sh(q), sh(k), sh(v)


def attention(qkv, heads=HEADS, _bug=None):
    """qkv [B, T, 3 D] -> (ctx [B, T, D], lse [B, heads, T])."""
    b, t, d3 = qkv.shape
    d = d3 // 3
    q, k, v = split_heads(qkv, heads, _bug)
    s = q @ k.transpose(-1, -2) / math.sqrt(d if _bug == 'scale_by_D' else d // heads)
    if _bug == 'softmax_without_max':
        # in fp32, as the kernel would: exp overflows where a score passes 88.7
        e = torch.exp(s.float()).to(s.dtype)
        p, lse = e / e.sum(dim=-1, keepdim=True), torch.log(e.sum(dim=-1))
    else:
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse.unsqueeze(-1))
    o = p @ v                                                             # [B, heads, T, dh]
    if _bug == 'heads_reversed':
        o = o.flip(1)
    return o.permute(0, 2, 1, 3).reshape(b, t, d), lse


def attention_bwd(qkv, ctx, lse, g_ctx, heads=HEADS):
    """g_qkv from the GIVEN ctx and lse, as the kernel forms it: p = exp(s - lse), delta = g_ctx . ctx per head."""
    b, t, d3 = qkv.shape
    d = d3 // 3
    dh = d // heads
    q, k, v = split_heads(qkv, heads)
    sh = lambda m: m.reshape(b, t, heads, dh).permute(0, 2, 1, 3)     # noqa: E731
    go, cx = sh(g_ctx), sh(ctx)
    scale = 1 / math.sqrt(dh)
    p = torch.exp(q @ k.transpose(-1, -2) * scale - lse.unsqueeze(-1))
    ds = p * (go @ v.transpose(-1, -2) - (go * cx).sum(dim=-1, keepdim=True))
    un = lambda m: m.permute(0, 2, 1, 3).reshape(b, t, d)     # noqa: E731
    return torch.cat([un(ds @ k * scale), un(ds.transpose(-1, -2) @ q * scale), un(p.transpose(-1, -2) @ go)], dim=-1)


# ------------------------------------------------------------------------------------------------------------------------ the network
def config(sd):
    w = sd['conv_proj.weight']
    depth = 0
    while f'encoder.layers.encoder_layer_{depth}.ln_1.weight' in sd:
        depth += 1
    return int(w.shape[0]), depth, int(w.shape[2]), int(sd['encoder.pos_embedding'].shape[1])


def forward(sd, x, _bug=None):
    """x: the normalised input [B, 3, h, w] -> logits [B, ncls]."""
    D, depth, P, T = config(sd)
    b, _, h, w = x.shape
    x4 = torch.cat([x, torch.zeros_like(x[:, :1])], dim=1).permute(0, 2, 3, 1)
    w4 = torch.cat([sd['conv_proj.weight'], torch.zeros_like(sd['conv_proj.weight'][:, :1])], dim=1).permute(0, 2, 3, 1).reshape(D, -1)
    emb = patchify(x4, P, _bug) @ w4.t() + sd['conv_proj.bias']
    t = assemble(emb.reshape(b, T - 1, D), sd['class_token'].reshape(-1), sd['encoder.pos_embedding'].reshape(T, D), _bug)
    for i in range(depth):
        p = f'encoder.layers.encoder_layer_{i}.'
        n1 = layernorm(t, sd[p + 'ln_1.weight'], sd[p + 'ln_1.bias'], _bug=_bug)[0]
        qkv = n1 @ sd[p + 'self_attention.in_proj_weight'].t() + sd[p + 'self_attention.in_proj_bias']
        ctx = attention(qkv, HEADS, _bug)[0]
        t = t + ctx @ sd[p + 'self_attention.out_proj.weight'].t() + sd[p + 'self_attention.out_proj.bias']
        n2 = layernorm(t, sd[p + 'ln_2.weight'], sd[p + 'ln_2.bias'], _bug=_bug)[0]
        a = gelu(n2 @ sd[p + 'mlp.0.weight'].t() + sd[p + 'mlp.0.bias'], _bug)
        t = t + a @ sd[p + 'mlp.3.weight'].t() + sd[p + 'mlp.3.bias']
    top = t.mean(dim=1) if _bug == 'head_on_token_mean' else t[:, 0]
    return layernorm(top, sd['encoder.ln.weight'], sd['encoder.ln.bias'], _bug=_bug)[0] @ sd['heads.head.weight'].t() + sd['heads.head.bias']


def classifier(sd, input_sz, sort_results=True):
    """The oracle-side stand-in for Classifier('vit_b_16', ...): (im, crop_sz) -> (raw_score, p_sorted ndarray, idx ndarray)."""

    def call(im, crop_sz=(240, 240)):
        if im.dtype == torch.uint8:
            im = im.type(torch.float32) / 255
        raw = forward(sd, so.classifier_preprocess(im, crop_sz, input_sz).to(next(iter(sd.values())).dtype))
        p = F.softmax(raw, dim=1).detach().cpu()
        if sort_results:
            p_sorted, idx = p.sort(descending=True)
        else:
            p_sorted, idx = p, torch.arange(p.shape[1]).repeat(p.shape[0], 1)
        return raw, p_sorted.numpy(), idx.numpy()

    return call


# -------------------------------------------------------------------------------------------------- fixtures of tests/test_vit_gpu.py
NUM_CLASSES, LOGIT_GAIN, B = 16, 4.0, 3
# name -> (image H x W, classifier crop, network input, P, D, depth, mlp width); T = (h / P)(w / P) + 1 = 25, 16, 5
GEOMS = {'wide': ((40, 56), (36, 52), (32, 48), 8, 96, 2, 384),
         'tall': ((24, 16), (24, 16), (20, 12), 4, 96, 3, 384),
         'real': ((40, 40), (36, 36), (32, 32), 16, 768, 1, 3072)}
_SD = {}


def state_dict(geom):
    if geom not in _SD:
        _, _, insz, P, D, depth, M = GEOMS[geom]
        _SD[geom] = syn.vit_b_16_state_dict(7, num_classes=NUM_CLASSES, logit_gain=LOGIT_GAIN, dim=D, depth=depth, mlp_dim=M, patch=P,
                                            input_sz=insz)
    return _SD[geom]


def images(geom):
    (h, w) = GEOMS[geom][0]
    return torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(21 + sorted(GEOMS).index(geom)))


# ------------------------------------------------------------------------------------------ inputs of tests/test_vit_ops_gpu.py
LN_CASES = [(d, rows) for d in (4, 48, 96, 768) for rows in (1, 3, 50)]
ATT_CASES = [(1, 1, 1, 4), (2, 3, 5, 8), (1, 2, 64, 64), (1, 2, 65, 64), (2, 1, 197, 64), (1, 1, 256, 16)]


def ln_inputs(D, rows):
    """x [rows, D] with planted rows (as far as `rows` allows: row 0 of variance 1e-6 .. 1e-4 around a zero mean -- at unit variance an
    eps of 1e-5 instead of 1e-6 changes y by 5e-6 only, here by tens of percent --, then a constant row, a row with a 1e4 outlier),
    weight, bias, the gradient g and the summand add."""
    gen = torch.Generator().manual_seed(100 * D + rows)
    x = torch.randn(rows, D, generator=gen) * 1.5 + 0.3
    x[0] = torch.randn(D, generator=gen) * (10.0 ** -(2 + (rows % 3) * 0.5))          # variance 1e-4, 1e-5 or 1e-6 (D = 4: about that)
    if rows > 1:
        x[1] = 0.7
    if rows > 2:
        x[2, D // 2] = 1e4
    w = torch.rand(D, generator=gen) + 0.5
    b = torch.rand(D, generator=gen) * 0.4 - 0.2
    g = torch.randn(rows, D, generator=gen)
    add = torch.randn(rows, D, generator=gen)
    return x, w, b, g, add


def gelu_inputs():
    gen = torch.Generator().manual_seed(5)
    x = torch.cat([torch.linspace(-12, 12, 4001), torch.randn(4083, generator=gen) * 3,
                   torch.tensor([0.0, -0.0, 1e-30, -1e-30, 40.0, -40.0, 12.0, -12.0, 1.0, -1.0, 0.5, -0.5])])
    assert x.numel() % 4 == 0
    return x, torch.randn(x.numel(), generator=gen)


def attn_inputs(B_, heads, T, dh):
    """qkv [B, T, 3 D] with unit-variance scores (the scale of ln_1's output through in_proj with the q, k rows at 1.5), and in head 0 of
    sample 0 planted query rows as far as T allows: row 0 with scores near +-80 and row 3 with scores near +-95 (exp(80) is still finite
    in fp32, which overflows from 88.7 on: it is row 3 that a softmax without the maximum subtracted cannot survive), row 1 with all
    scores equal (q = 0), row 2 with one key far above the rest.  Also g_ctx."""
    gen = torch.Generator().manual_seed(1000 * T + dh)
    D = heads * dh
    qkv = torch.randn(B_, T, 3 * D, generator=gen)
    qkv[..., :2 * D] *= dh ** 0.25 * 1.2                    # q . k / sqrt(dh) has standard deviation ~1.4
    k = qkv[0, :, D:D + dh]                                 # (a view: the keys of head 0, sample 0)

    def aim(row, key, score):
        """q_row such that q_row . k_key / sqrt(dh) = score"""
        qkv[0, row, :dh] = k[key] * (score * math.sqrt(dh) / float(k[key] @ k[key]))

    if T > 1:
        k[1] = -k[0]                                        # scores -80 / -95 where key 0 scores +80 / +95
        qkv[0, 1, :dh] = 0.0
    aim(0, 0, 80.0)
    if T > 2:
        aim(2, 2, 12.0)
    if T > 3:
        aim(3, 0, 95.0)
    return qkv, torch.randn(B_, T, D, generator=gen)


# --------------------------------------------------------------------------------------------------------------------------- the bars
def measured_rel(fn32, x32, mag=None):
    """Largest error of torch's fp32 evaluation of `fn32` on the CPU at the fp32 arguments `x32` against float64, relative to `mag`
    (float64; default: |the float64 value|), with the floor FLT_MIN under the denominator."""
    ref = fn32(x32.double())
    return float(((fn32(x32).double() - ref).abs() / (ref.abs() if mag is None else mag).clamp_min(FLT_MIN)).max())


def bar_layernorm(x, w, b, eps=EPS):
    """Per-element bounds (e_y [rows, D], e_mean [rows], e_rstd [rows]) for fp32 LayerNorm of the float64 `x` (fp32 values).
    mean: D terms summed, one division: (D + 1) U mean|x|.  c = x - mean: e_c = e_mean + U |c|.  var = mean(c^2): 2 |c| e_c per term,
    D + 2 roundings.  rstd = 1 / sqrt(var + eps): half the relative error of var + eps, plus the add, the root and the division (3 U).
    y = fma(c rstd, w, b): |w| (e_c rstd + |c| e_rstd + 2 U |c| rstd) + U |y|."""
    D = x.shape[-1]
    y, mu, rs = layernorm(x, w, b, eps)
    mu, rs = mu.unsqueeze(-1), rs.unsqueeze(-1)
    c = (x - mu).abs()
    e_mu = (D + 1) * U * x.abs().mean(dim=-1, keepdim=True)
    e_c = e_mu + U * c
    var = (c * c).mean(dim=-1, keepdim=True)
    e_var = (2 * c * e_c).mean(dim=-1, keepdim=True) + (D + 2) * U * var
    e_rs = rs * (0.5 * e_var / (var + eps) + 3 * U)
    e_y = w.abs() * (e_c * rs + c * e_rs + 2 * U * c * rs) + U * y.abs()
    return SLACK * e_y, SLACK * e_mu.squeeze(-1), SLACK * e_rs.squeeze(-1)


def bar_layernorm_bwd(g, x, w, mean, rstd, add=None):
    """gh = g w (U); xh = (x - mean) rstd (2 U); m1 = mean(gh): (D + 2) U mean|gh|; m2 = mean(gh xh): (D + 5) U mean|gh xh|; the inner
    sum of three terms and its products: |xh| e_m2 + |m2| 2 U |xh| + 4 U (|gh| + |m1| + |xh m2|); times rstd (U), plus add (U)."""
    D = x.shape[-1]
    rs = rstd.unsqueeze(-1)
    gh, xh = (g * w).abs(), ((x - mean.unsqueeze(-1)) * rs).abs()
    m1s, m2s = (g * w).mean(dim=-1, keepdim=True).abs(), (g * w * (x - mean.unsqueeze(-1)) * rs).mean(dim=-1, keepdim=True).abs()
    e_m1 = (D + 2) * U * gh.mean(dim=-1, keepdim=True)
    e_m2 = (D + 5) * U * (gh * xh).mean(dim=-1, keepdim=True)
    e_in = e_m1 + xh * e_m2 + 2 * U * xh * m2s + 4 * U * (gh + m1s + xh * m2s)
    gx = layernorm_bwd(g, x, w, mean, rstd)
    e = rs * e_in + U * gx.abs()
    if add is not None:
        e = e + U * (gx + add).abs()
    return SLACK * e


def _abs_heads(qkv, heads):
    return split_heads(qkv.abs(), heads)


def bar_attention(qkv, heads, m_exp, m_log):
    """(e_ctx [B, T, D], e_lse [B, heads, T]).  s = scale q . k: e_s = (dh + 1) U scale sum|q k|.  exp(s - max): relative error
    d_e = e_s + e_s(max) + U |s - max| (the argument) + LIBM m_exp (the library).  The row sum of T such terms: max d_e + T U; p: d_p =
    d_e + max d_e + (T + 1) U.  ctx = sum_j p_j v_j over T terms: sum_j |p_j v_j| (d_p_j + (T + 1) U).  lse = max + log(sum): e_s(max) +
    the sum's relative error + LIBM m_log |log sum| + U |lse|."""
    b, t, d3 = qkv.shape
    d = d3 // 3
    dh = d // heads
    scale = 1 / math.sqrt(dh)
    q, k, v = split_heads(qkv, heads)
    s = q @ k.transpose(-1, -2) * scale
    e_s = (dh + 1) * U * scale * (q.abs() @ k.abs().transpose(-1, -2))
    m, arg = s.max(dim=-1, keepdim=True)
    e_m = e_s.gather(-1, arg)
    d_e = e_s + e_m + U * (s - m).abs() + LIBM * m_exp
    d_sum = d_e.max(dim=-1, keepdim=True).values + t * U
    ctx, lse = attention(qkv, heads)
    p = torch.exp(s - lse.unsqueeze(-1))
    d_p = d_e + d_sum + U
    e_ctx = (p * (d_p + (t + 1) * U)) @ v.abs()
    logsum = (lse.unsqueeze(-1) - m).abs()
    e_lse = e_m + d_sum + LIBM * m_log * logsum + U * lse.unsqueeze(-1).abs() + U * m.abs()
    return SLACK * e_ctx.permute(0, 2, 1, 3).reshape(b, t, d), SLACK * e_lse.squeeze(-1)


def bar_attention_bwd(qkv, ctx, lse, g_ctx, heads, m_exp):
    """e_g_qkv [B, T, 3 D] for the kernel's formula on the given ctx and lse (fp32 values, each within U of what it stands for).
    p = exp(s - lse): relative d_p = e_s + U (|s| + 2 |lse|) + LIBM m_exp.  dp = g . v: e_dp = (dh + 1) U sum|g v|; delta = g . ctx:
    e_delta = (dh + 7) U sum|g ctx| (its dh terms, the wave sum, the rounding of ctx itself).  ds = p (dp - delta): e_ds = p (e_dp +
    e_delta + U (|dp| + |delta|)) + (d_p + U) |ds|.  g_q = scale sum_j ds k: scale (sum_j e_ds |k| + (T + 2) U sum_j |ds k|), g_k
    likewise over i; g_v = sum_i p g: sum_i |p g| (d_p + (T + 1) U)."""
    b, t, d3 = qkv.shape
    d = d3 // 3
    dh = d // heads
    scale = 1 / math.sqrt(dh)
    q, k, v = split_heads(qkv, heads)
    sh = lambda m: m.reshape(b, t, heads, dh).permute(0, 2, 1, 3)     # noqa: E731
    go, cx = sh(g_ctx), sh(ctx)
    s = q @ k.transpose(-1, -2) * scale
    l_ = lse.unsqueeze(-1)
    e_s = (dh + 1) * U * scale * (q.abs() @ k.abs().transpose(-1, -2))
    d_p = e_s + U * (s.abs() + 2 * l_.abs()) + LIBM * m_exp
    p = torch.exp(s - l_)
    dp, delta = go @ v.transpose(-1, -2), (go * cx).sum(dim=-1, keepdim=True)
    e_dp = (dh + 1) * U * (go.abs() @ v.abs().transpose(-1, -2))
    e_delta = (dh + 7) * U * (go.abs() * cx.abs()).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta)
    e_ds = p * (e_dp + e_delta + U * (dp.abs() + delta.abs())) + (d_p + U) * ds.abs()
    e_q = scale * (e_ds @ k.abs() + (t + 2) * U * (ds.abs() @ k.abs()))
    e_k = scale * (e_ds.transpose(-1, -2) @ q.abs() + (t + 2) * U * (ds.abs().transpose(-1, -2) @ q.abs()))
    e_v = (p * (d_p + (t + 1) * U)).transpose(-1, -2) @ go.abs()
    un = lambda m: m.permute(0, 2, 1, 3).reshape(b, t, d)     # noqa: E731
    return SLACK * torch.cat([un(e_q), un(e_k), un(e_v)], dim=-1)


def gelu_rel(y, ref, mag=None):
    """The error measure of the GELU tests, element by element: |y - ref| / max(mag, FLT_MIN), mag = |ref| forward (a product: nothing
    cancels) and gelu_bwd_mag for the adjoint."""
    return (y.double() - ref).abs() / (ref.abs() if mag is None else mag).clamp_min(FLT_MIN)


def gelu_bwd_mag(g, x):
    """The magnitudes the GELU adjoint sums: |g| (Phi(x) + |x| phi(x)).  (Phi + x phi itself passes through zero near x = -0.75, where
    an error relative to the result would say nothing about the kernel.)"""
    return g.abs() * (Phi(x) + x.abs() * phi(x))


# -------------------------------------------------------------------------------------------------------------------------- mutations
# name -> the functions that make the mistake (called with _bug=name).  `forward` makes every one of them but the LayerNorm adjoint's
# (its gradient is autograd's).
MUTATIONS = {
    'scale_by_D': (attention,),
    'k_v_swapped': (attention,),
    'heads_reversed': (attention,),
    'eps_1e-5': (layernorm,),
    'unbiased_variance': (layernorm,),
    'ln_bwd_without_xhat_term': (layernorm_bwd,),
    'tanh_gelu': (gelu, gelu_bwd),
    'softmax_without_max': (attention,),
    'column_major_tokens': (patchify,),
    'class_token_without_pos': (assemble,),
    'head_on_token_mean': (forward,),
}
