"""Float64 restatement of the transferable adversarial step (spaa_transfer_blur + spaa_transfer_momentum), written for the
tests: nothing in the reference does this.  Images are [B,H,W,4] (the layout of the kernels), float64 torch tensors on the CPU.

Per sample b on the adversarial step (col[b] false):
    t   = K (*) g_b      K = outer(w, w), w the float32 taps of Transfer.weights(); F.conv2d with padding = r, per colour channel
    n1  = sum |t| over pixels and the three colour channels
    m_b = mu m_b + t / n1     (n1 == 0: mu m_b)
    g_b = m_b,  ss_b = ||m_b||^2
A sample on the colour step keeps g_b and m_b.

The error bounds of the tests are derived here from the formats and the summation orders of the kernels (U = 2^-24, the unit roundoff
of fp32), never from what the kernels return."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
# The longest chains of fp32 additions behind one sum of the implementation (each addition rounds once, so a sum of non-negative terms
# is within chain * U of its exact value, relatively):
#   one entry of partial_l1: a thread adds the 6 values |t.rgb| of its two pixels (5 additions), the wave's shuffle tree adds 6 levels,
#   the four wave sums take 3 more additions: 14.  The tiles' sums meet in a double that is rounded once: + 1.
CHAIN_L1 = 5 + 6 + 3 + 1


def chain_ss(HW, npartial):
    """One entry of partial_ss: a thread squares and adds 3 values for each of its ceil(chunks / npartial) chunks (the square rounds once,
    the additions 3 per chunk), then the block sum's 6 + 3 additions."""
    chunks = (HW + 255) // 256
    per_block = -(-chunks // npartial)
    return 1 + 3 * per_block + 9


def taps64(transfer):
    """The float32 taps of a Transfer as float64 (what the kernel multiplies with, exactly)."""
    return transfer.weights().double()


def blur(g, w):
    """K (*) g: [B,H,W,4] float64 -> [B,H,W,4], the pad channel 0 whatever g's pad channel holds."""
    w = torch.as_tensor(w, dtype=torch.float64)
    r = (w.numel() - 1) // 2
    k = torch.outer(w, w)[None, None].expand(3, 1, -1, -1).contiguous()
    x = torch.as_tensor(g, dtype=torch.float64)[..., :3].permute(0, 3, 1, 2)
    t = F.conv2d(x, k, padding=r, groups=3).permute(0, 2, 3, 1)
    return torch.cat((t, torch.zeros_like(t[..., :1])), dim=3)


def blur_bound(g, w):
    """|t_fp32 - t_64| <= 4 (2 r + 1) U (K (*) |g|) per element: each pass is a dot product of 2 r + 1 terms accumulated with fused
    multiply-adds ((2 r + 1) U to first order, relative to the dot product of the absolute values), the second pass carries the first
    one's error and adds its own, and the factor 4 instead of 2 covers the higher-order terms."""
    n = torch.as_tensor(w).numel()
    return 4.0 * n * U * blur(torch.as_tensor(g, dtype=torch.float64).abs(), w)


def step(g, m, col, w, mu):
    """One application of steps 1-5.  g, m: [B,H,W,4] float64; col: bool [B] (True: the sample is on the colour step).  Returns a dict:
    t, n1 [B], m (new), g (new), ss [B] = ||m||^2 over the colour channels, and the element bounds e_t (blur_bound) and e_m: the bound on
    |m_fp32 - m_64| for ONE step from the same m: e_t / n1 + 3 U |m_64| (the rounding of the division, of the fused multiply-add, and n1's
    own relative error)."""
    g = torch.as_tensor(g, dtype=torch.float64)
    m = torch.as_tensor(m, dtype=torch.float64)
    col = torch.as_tensor(col, dtype=torch.bool)
    adv = (~col)[:, None, None, None]
    t = blur(g, w)
    e_t = blur_bound(g, w)
    n1 = t[..., :3].abs().sum(dim=(1, 2, 3))
    safe = torch.where(n1 > 0, n1, torch.ones_like(n1))[:, None, None, None]
    q = torch.where((n1 > 0)[:, None, None, None], t / safe, torch.zeros_like(t))
    m_new = torch.where(adv, mu * m + q, m)
    m_new[..., 3] = torch.where(adv[..., 0], torch.zeros_like(m_new[..., 3]), m[..., 3])
    e_m = torch.where(adv, e_t / safe + 3.0 * U * m_new.abs(), torch.zeros_like(m_new))
    g_new = torch.where(adv, m_new, g)
    return dict(t=torch.where(adv, t, torch.zeros_like(t)), n1=torch.where(col, torch.zeros_like(n1), n1), m=m_new, g=g_new,
                ss=m_new[..., :3].pow(2).sum(dim=(1, 2, 3)), e_t=e_t, e_m=e_m)


def recurrence(grads, cols, x0, w, mu, adv_lr, col_lr, chain_norm):
    """The loop's direction and step over len(grads) iterations from recorded gradient images: grads[i] [B,H,W,4] is the gradient image
    that entered _shape_direction in iteration i, cols[i] bool [B] its colour-step flags, x0 the projector image before iteration 0.
    m starts at zero; x <- x - lr d / ||d||_2 with d = m (adversarial step, lr = adv_lr) or d = g (colour step, lr = col_lr).
    Yields per iteration (m, x, E_m, E_x): the float64 values and the accumulated element bounds
        E_m <- mu E_m + e_m                                           (the recurrence is linear in its own error)
        E_x <- E_x + lr (E_d / ||d|| + |d| / ||d|| (||E_d||_2 / ||d|| + chain_norm U)) + 4 U (|x| + lr)
    with E_d = E_m on the adversarial step and 0 on the colour step (the recorded g is the kernel's own input there), chain_norm the
    addition chain behind ||d||^2 (relative error chain_norm U of the square, at most that of the root), and 4 U (|x| + lr) the roundings
    of the division, the product and the subtraction of the step itself."""
    x = torch.as_tensor(x0, dtype=torch.float64).clone()
    m = torch.zeros_like(x)
    E_m, E_x = torch.zeros_like(x), torch.zeros_like(x)
    for g, col in zip(grads, cols):
        col = torch.as_tensor(col, dtype=torch.bool)
        s = step(g, m, col, w, mu)
        adv = (~col)[:, None, None, None]
        m = s['m']
        E_m = torch.where(adv, mu * E_m + s['e_m'], E_m)
        d = s['g'].clone()
        d[..., 3] = 0
        E_d = torch.where(adv, E_m, torch.zeros_like(E_m))
        E_d[..., 3] = 0
        nrm = d.pow(2).sum(dim=(1, 2, 3)).sqrt()[:, None, None, None]
        lr = torch.where(adv, torch.full_like(nrm, float(adv_lr)), torch.full_like(nrm, float(col_lr)))
        E_nrm = E_d.pow(2).sum(dim=(1, 2, 3)).sqrt()[:, None, None, None]
        E_x = E_x + lr * (E_d / nrm + d.abs() / nrm * (E_nrm / nrm + chain_norm * U)) + 4.0 * U * (x.abs() + lr)
        x = x - lr * d / nrm
        yield m, x, E_m, E_x
