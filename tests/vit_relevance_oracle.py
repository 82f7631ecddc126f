"""TEST INFRASTRUCTURE: the float64 restatement of the ViT's relevance rollout (Chefer, Gur and Wolf, "Transformer
Interpretability Beyond Attention Visualization", 2021, restated from the paper), the bar of one layer's step with its derivation, and
`MUTATIONS`: the same functions with one deliberate mistake each (tests/test_vit_relevance_cpu.py shows that every one lands beyond
its bar on the inputs the GPU tests use).

Definition.  Per encoder layer l, with P_h [T, T] the attention probabilities of head h and dP_h the gradient of the sample's class
logit with respect to them:
  A_l = mean over the heads of max(0, P_h * dP_h)        (elementwise product; T x T)
  R   = (I + A_L) ... (I + A_1)
and the map is row 0 of R (the class token) at the T - 1 patch columns, row-major on the patch grid, clamped at 0 and divided by its
maximum (1 everywhere where the maximum is 0).

Two formulations, on purpose.  `network_map` is the reference of the GPU tests: autograd's gradient with respect to each layer's
probabilities, and the matrix product R.  `step` / `rollout_rows` are what the kernels do: the class token's row alone, pushed down from the top layer,
rho_L = e_cls, rho_(l-1) = rho_l + rho_l A_l, with P = exp(scale q k^T - lse) and dP = g_ctx v^T recomputed from what the attention
adjoint reads, and the loop's cotangent divided by its seed s = g_logits[b, target[b]] (the rollout is not scale invariant: A is added
to I).  A sample whose seed is 0, or whose target is no class, has A = 0."""
import math

import torch

import vit_oracle as vo
from vit_oracle import HEADS, LIBM, SLACK, U

NCLS = 5


# ----------------------------------------------------------------------------------------------------------------- one layer's step
def _abar(z, _bug=None):
    """z [B, heads, T, T] = P * dP / seed -> A [B, T, T]."""
    if _bug == 'no_relu':
        return z.mean(dim=1)
    if _bug == 'abs_for_relu':
        return z.abs().mean(dim=1)
    if _bug == 'relu_after_head_mean':
        return z.mean(dim=1).clamp(min=0)
    if _bug == 'head_sum':
        return z.clamp(min=0).sum(dim=1)
    return z.clamp(min=0).mean(dim=1)


def _push(rho, A, _bug=None):
    """rho [B, T], A [B, T, T] -> rho + rho A."""
    if _bug == 'A_rho_for_rho_A':
        return rho + (A @ rho.unsqueeze(-1)).squeeze(-1)
    if _bug == 'no_identity':
        return (rho.unsqueeze(1) @ A).squeeze(1)
    return rho + (rho.unsqueeze(1) @ A).squeeze(1)


def seeds(g_logits, target):
    """[B]: g_logits[b, target[b]], 0 where target[b] is no class."""
    ncls = g_logits.shape[1]
    ok = (target >= 0) & (target < ncls)
    s = g_logits.gather(1, target.clamp(0, ncls - 1).long().unsqueeze(1)).squeeze(1)
    return torch.where(ok, s, torch.zeros_like(s))


def step_parts(qkv, lse, g_ctx, seed, heads=HEADS, _bug=None):
    """(p, dp, z) [B, heads, T, T] of the GIVEN qkv [B, T, 3 D], lse [B, heads, T], g_ctx [B, T, D] and seed [B]: z = p dp / seed, 0 for
    a sample whose seed is 0."""
    b, t, d3 = qkv.shape
    d = d3 // 3
    dh = d // heads
    q, k, v = vo.split_heads(qkv, heads)
    go = g_ctx.reshape(b, t, heads, dh).permute(0, 2, 1, 3)
    p = torch.exp(q @ k.transpose(-1, -2) / math.sqrt(dh) - lse.unsqueeze(-1))
    dp = go @ v.transpose(-1, -2)
    live = seed != 0
    div = torch.where(live, seed, torch.ones_like(seed))
    if _bug == 'seed_sign_ignored':
        div = div.abs()
    z = p * dp / div.reshape(b, 1, 1, 1) * live.to(p.dtype).reshape(b, 1, 1, 1)
    return p, dp, z


def step(qkv, lse, g_ctx, rho, seed, heads=HEADS, _bug=None):
    """rho_out [B, T] = rho + rho A of one layer."""
    return _push(rho, _abar(step_parts(qkv, lse, g_ctx, seed, heads, _bug)[2], _bug), _bug)


def class_map(rho, seed=None, _bug=None):
    """(c [B, T - 1], cmax [B]) from the bottom layer's rho [B, T]."""
    c = (rho[:, :-1] if _bug == 'class_token_column_kept' else rho[:, 1:]).clamp(min=0)
    if seed is not None:
        c = c * (seed != 0).to(c.dtype).unsqueeze(1)
    return c, c.max(dim=1).values


def normalised(c):
    """m [B, T - 1] = c / max c, 1 everywhere where the maximum is 0 (what spaa_attention_apply reads c and cmax as)."""
    cmax = c.max(dim=1, keepdim=True).values
    return torch.where(cmax > 0, c / cmax.clamp_min(1e-300), torch.ones_like(c))


# ------------------------------------------------------------------------------------------------------------------------ the network
def _network(sd, x, target):
    """The forward pass of vit_oracle.forward with the attention written out, and autograd's gradients of sum_b logits[b, target[b]]:
    per layer, in forward order, (qkv [B, T, 3 D], P [B, heads, T, T], dP, g_ctx [B, T, D]).  P stays part of the graph: dP is the
    derivative with respect to that layer's probabilities through everything above them, the later layers' attention included -- what
    the backward pass itself carries (g_ctx v^T), and what the paper's gradient hooks on the attention maps give."""
    D, depth, P, T = vo.config(sd)
    b = x.shape[0]
    x4 = torch.cat([x, torch.zeros_like(x[:, :1])], dim=1).permute(0, 2, 3, 1)
    w4 = torch.cat([sd['conv_proj.weight'], torch.zeros_like(sd['conv_proj.weight'][:, :1])], dim=1).permute(0, 2, 3, 1).reshape(D, -1)
    emb = vo.patchify(x4, P) @ w4.t() + sd['conv_proj.bias']
    t = vo.assemble(emb.reshape(b, T - 1, D), sd['class_token'].reshape(-1), sd['encoder.pos_embedding'].reshape(T, D))
    t = t.detach().requires_grad_(True)
    qkvs, probs, ctxs = [], [], []
    for i in range(depth):
        p = f'encoder.layers.encoder_layer_{i}.'
        n1 = vo.layernorm(t, sd[p + 'ln_1.weight'], sd[p + 'ln_1.bias'])[0]
        qkv = n1 @ sd[p + 'self_attention.in_proj_weight'].t() + sd[p + 'self_attention.in_proj_bias']
        q, k, v = vo.split_heads(qkv, HEADS)
        pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // HEADS), dim=-1)
        ctx = (pr @ v).permute(0, 2, 1, 3).reshape(b, T, D)
        qkvs.append(qkv)
        probs.append(pr)
        ctxs.append(ctx)
        t = t + ctx @ sd[p + 'self_attention.out_proj.weight'].t() + sd[p + 'self_attention.out_proj.bias']
        n2 = vo.layernorm(t, sd[p + 'ln_2.weight'], sd[p + 'ln_2.bias'])[0]
        t = t + vo.gelu(n2 @ sd[p + 'mlp.0.weight'].t() + sd[p + 'mlp.0.bias']) @ sd[p + 'mlp.3.weight'].t() + sd[p + 'mlp.3.bias']
    logits = vo.layernorm(t[:, 0], sd['encoder.ln.weight'], sd['encoder.ln.bias'])[0] @ sd['heads.head.weight'].t() + sd['heads.head.bias']
    grads = torch.autograd.grad(logits[torch.arange(b), torch.as_tensor(target).long()].sum(), probs + ctxs)
    return [(qkv.detach(), pr.detach(), gp, gc) for qkv, pr, gp, gc in zip(qkvs, probs, grads[:depth], grads[depth:])]


def layer_products(sd, x, target):
    """x: the normalised input [B, 3, h, w]; target: the classes [B].  Per layer, in forward order, z_l = P * dP [B, heads, T, T], dP
    autograd's gradient of logits[b, target[b]] with respect to the layer's probabilities."""
    return [pr * gp for _, pr, gp, _ in _network(sd, x, target)]


def network_rows(sd, x, target, seed):
    """rho [B, T] at the bottom layer as the kernels form it: `step` layer by layer from the top on the network's own qkv, lse and
    g_ctx, the latter scaled by `seed` [B] as the loop's cotangent is."""
    rho = None
    for qkv, pr, _, gc in reversed(_network(sd, x, target)):
        if rho is None:
            rho = torch.zeros(qkv.shape[0], qkv.shape[1], dtype=qkv.dtype)
            rho[:, 0] = 1
        rho = step(qkv, vo.attention(qkv, HEADS)[1], gc * seed.reshape(-1, 1, 1), rho, seed)
    return rho


def rollout_matrix(As):
    """Row 0 of R = (I + A_L) ... (I + A_1) for As = [A_1 .. A_L], each [B, T, T]: the matrix form."""
    b, T, _ = As[0].shape
    R = torch.eye(T, dtype=As[0].dtype).expand(b, T, T).clone()
    for A in As:
        R = R + A @ R
    return R[:, 0]


def rollout_rows(As, _bug=None):
    """The same row by the recurrence the kernels run: rho_L = e_cls, rho_(l-1) = rho_l + rho_l A_l."""
    b, T, _ = As[0].shape
    rho = torch.zeros(b, T, dtype=As[0].dtype)
    rho[:, 0] = 1
    for A in (As if _bug == 'layers_in_forward_order' else reversed(As)):
        rho = _push(rho, A, _bug)
    return rho


def network_map(sd, x, target, _bug=None):
    """(m [B, T - 1] in [0, 1], cmax [B]): the reference (matrix form) without `_bug`, the recurrence with the mistake `_bug` else."""
    As = [_abar(z, _bug) for z in layer_products(sd, x, target)]
    rho = rollout_matrix(As) if _bug is None else rollout_rows(As, _bug)
    c, cmax = class_map(rho, None, _bug)
    return normalised(c), cmax


# ------------------------------------------------------------------------------------ inputs of tests/test_vit_relevance_ops_gpu.py
VARIANTS = ('positive_seed', 'negative_seed', 'zero_seed', 'target_outside')


def step_inputs(case, variant):
    """For a case (B, heads, T, dh) of vit_oracle.ATT_CASES: qkv and g_ctx of vit_oracle.attn_inputs (planted rows included), the fp32
    lse of the float64 attention, rho [B, T] >= 0 with exact zeros planted at every third token (and a 1 at the class token), g_logits
    [B, NCLS] with a single entry per sample, and target int32 [B].  `variant`: the seed of sample 0 -- 0.25, -1 / 3, 0 at a valid
    target, or 0.25 with the target outside [0, NCLS) (-1 for an odd T, NCLS else); the other samples' seeds are -0.5."""
    B_, heads, T, dh = case
    qkv, g_ctx = vo.attn_inputs(*case)
    lse = vo.attention(qkv.double(), heads)[1].float()
    gen = torch.Generator().manual_seed(77 * T + dh)
    rho = torch.rand(B_, T, generator=gen) * 0.5
    rho[:, 2::3] = 0.0
    rho[:, 0] = 1.0
    target = torch.tensor([(2 + 3 * b) % NCLS for b in range(B_)], dtype=torch.int32)
    g_logits = torch.zeros(B_, NCLS)
    g_logits[torch.arange(B_), target.long()] = -0.5
    g_logits[0, int(target[0])] = {'positive_seed': 0.25, 'negative_seed': -1.0 / 3.0, 'zero_seed': 0.0, 'target_outside': 0.25}[variant]
    if variant == 'target_outside':
        target[0] = -1 if T % 2 else NCLS
    return qkv, lse, g_ctx, rho, g_logits, target


def exp_error(qkv, lse, heads):
    """torch's fp32 exp on the CPU against float64 at the arguments the step's kernel meets (scale q . k - lse, above -80: below that p
    vanishes against the row's 1), relative."""
    q, k, _ = vo.split_heads(qkv.double(), heads)
    arg = (q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]) - lse.double().unsqueeze(-1)).float()
    arg = arg[arg > -80]
    return vo.measured_rel(torch.exp, arg) if arg.numel() else U


# --------------------------------------------------------------------------------------------------------------------------- the bar
def bar_step(qkv, lse, g_ctx, rho, seed, heads, m_exp):
    """e_rho_out [B, T] for the kernel's formula on the given (fp32-valued, float64-typed) inputs, to first order in U = 2^-24.
    p = exp(scale q . k - lse): relative d_p = e_s + U (|s| + 2 |lse|) + LIBM m_exp, e_s = (dh + 1) U scale sum|q k| (as
    vit_oracle.bar_attention_bwd).  dp = g_ctx . v: e_dp = (dh + 1) U sum|g v|.  x = p dp (1 / seed): the product, the reciprocal and
    the multiplication by it, 3 U: e_x = (p e_dp + (d_p + 3 U) |p dp|) / |seed|.  z = max(0, x) is 1-Lipschitz: e_z = e_x.  Per head
    w_j = sum_i rho_i z_ij over T queries (fused multiply-adds per lane, then the wave's tree): (T + 2) U sum_i |rho_i z_ij| + sum_i
    |rho_i| e_z.  The head mean: heads - 1 additions and one division, heads + 1 roundings on sum_h |w|, over heads.  The final
    addition: U |rho_out|.  Times SLACK for the second order.
    Underflow (absolute, not times SLACK): an fp32 result below FLT_MIN = 2^-126 may be lost whole (a denormal keeps fewer bits, or
    is flushed), which no relative term covers -- the planted rows have p = exp(-95 ..) and, at the top layer, patch columns that are
    such a z alone.  A lost p costs FLT_MIN |dp| / |seed| of z, a lost product p dp FLT_MIN / |seed|, a lost x FLT_MIN; each of the T
    products rho z and the head sum FLT_MIN again."""
    b, t, d3 = qkv.shape
    dh = d3 // 3 // heads
    scale = 1 / math.sqrt(dh)
    q, k, v = vo.split_heads(qkv, heads)
    go = g_ctx.reshape(b, t, heads, dh).permute(0, 2, 1, 3)
    s = q @ k.transpose(-1, -2) * scale
    l_ = lse.unsqueeze(-1)
    e_s = (dh + 1) * U * scale * (q.abs() @ k.abs().transpose(-1, -2))
    d_p = e_s + U * (s.abs() + 2 * l_.abs()) + LIBM * m_exp
    p, dp, z = step_parts(qkv, lse, g_ctx, seed, heads)
    e_dp = (dh + 1) * U * (go.abs() @ v.abs().transpose(-1, -2))
    live = (seed != 0).to(p.dtype).reshape(b, 1, 1, 1)
    inv = live / torch.where(seed != 0, seed, torch.ones_like(seed)).abs().reshape(b, 1, 1, 1)
    e_z = (p * e_dp + (d_p + 3 * U) * (p * dp).abs()) * inv
    u_z = (vo.FLT_MIN * (dp.abs() + 1) * inv + vo.FLT_MIN) * live
    r = rho.abs().reshape(b, 1, t, 1)
    zc = z.clamp(min=0)
    e_w = (t + 2) * U * (r * zc).sum(dim=2) + (r * e_z).sum(dim=2)                        # [B, heads, T]
    w = (rho.reshape(b, 1, t, 1) * zc).sum(dim=2)
    e_mean = (e_w.sum(dim=1) + (heads + 1) * U * w.abs().sum(dim=1)) / heads
    u_mean = ((r * u_z).sum(dim=2) + t * vo.FLT_MIN).sum(dim=1) / heads + vo.FLT_MIN
    return SLACK * (e_mean + U * step(qkv, lse, g_ctx, rho, seed, heads).abs()) + u_mean


# -------------------------------------------------------------------------------------------------------------------------- mutations
# name -> the functions that make the mistake (called with _bug=name)
MUTATIONS = {
    'no_relu': (step, network_map),
    'abs_for_relu': (step, network_map),
    'relu_after_head_mean': (step, network_map),
    'head_sum': (step, network_map),
    'A_rho_for_rho_A': (step, network_map),
    'no_identity': (step, network_map),
    'seed_sign_ignored': (step,),
    'layers_in_forward_order': (network_map,),
    'class_token_column_kept': (network_map,),
}
