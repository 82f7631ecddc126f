"""Float64 / integer restatements of the capture jitter ("Capture-robust attack"), for the jitter tests: the counter-based
generator in Python integers (`mix32`, `draw_word`, `draw_tables`, `normals`), the transform and its adjoint in numpy float64
(`shift`, `shift_T`, `forward`, `backward`), the transform in torch double for autograd (`transform_torch`) and one whole first
iteration of the jitter attack built from the oracle's PCNet, its classifier and the ensemble oracle's decision (`first_iteration`).
A helper, not a test module."""
import numpy as np
import torch

M32 = 0xffffffff
GAIN, OFFSET, DX, DY, SIGMA, KEY = 0, 3, 4, 5, 6, 7   # parameter indices = columns of a table row (KEY: the noise key's index)
IDENTITY_ROW = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def mix32(x):
    """The 32-bit mixing function, on a Python int or a numpy uint64 array of 32-bit values."""
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint64) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        return x
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw_word(seed, t, b, j, i):
    """The 32-bit word of (seed, iteration t, sample b, draw j, parameter index i)."""
    h = mix32((seed & M32) ^ 0x9e3779b9)
    for v in (t, b, j, i):
        h = mix32(h ^ (v & M32))
    return h


def uniform(h):
    """u = (h >> 8) 2^-24 in [0, 1)."""
    return (h >> 8) / 16777216.0


def draw_tables(seed, t, B, J, gain, offset, shift, noise, clean0):
    """(jit float64 [B][J][8], key uint32 [B][J]) of iteration t.  The four ranges are taken as the float32 values the C entry point
    receives; the arithmetic is float64 (the kernel's differs by its fp32 roundings)."""
    gain, offset, shift, noise = (float(np.float32(v)) for v in (gain, offset, shift, noise))
    jit = np.zeros((B, J, 8))
    key = np.zeros((B, J), dtype=np.uint32)
    for b in range(B):
        for j in range(J):
            key[b, j] = draw_word(seed, t, b, j, KEY)
            if clean0 and j == 0:
                jit[b, j] = IDENTITY_ROW
                continue
            s = [2.0 * uniform(draw_word(seed, t, b, j, i)) - 1.0 for i in range(6)]
            jit[b, j] = (1 + gain * s[0], 1 + gain * s[1], 1 + gain * s[2], offset * s[OFFSET], shift * s[DX], shift * s[DY], noise, 0)
    return jit, key


def normals(key, npix):
    """Standard normals [npix][3] of one noise key: Box-Muller from two uniforms of (key, pixel, channel)."""
    pix = np.arange(npix, dtype=np.uint64)
    a = mix32(np.uint64(int(key)) ^ ((pix * np.uint64(0x9e3779b1)) & np.uint64(M32)))
    out = np.zeros((npix, 3))
    for c in range(3):
        h1 = mix32((a + np.uint64(2 * c)) & np.uint64(M32))
        h2 = mix32((a + np.uint64(2 * c + 1)) & np.uint64(M32))
        u1 = ((h1 >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (h2 >> np.uint64(8)).astype(np.float64) / 16777216.0
        out[:, c] = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return out


def axis_taps(d, n):
    """One axis of S for a shift d over n samples: (idx0, idx1, f) with out[m] = (1 - f) in[idx0[m]] + f in[idx1[m]]."""
    k = int(np.floor(d))
    m = np.arange(n)
    return np.clip(m + k, 0, n - 1), np.clip(m + k + 1, 0, n - 1), float(d) - k


def shift(im, dx, dy):
    """S: the bilinear translation of im [H][W][C] by (dx, dy) with replicate border, columns (dx) then rows (dy)."""
    c0, c1, fx = axis_taps(dx, im.shape[1])
    r0, r1, fy = axis_taps(dy, im.shape[0])
    cols = (1 - fx) * im[:, c0] + fx * im[:, c1]
    return (1 - fy) * cols[r0] + fy * cols[r1]


def shift_T(g, dx, dy):
    """S^T as a scatter: every output pixel adds its weighted value to the input pixels its taps read."""
    c0, c1, fx = axis_taps(dx, g.shape[1])
    r0, r1, fy = axis_taps(dy, g.shape[0])
    cols = np.zeros_like(g)
    np.add.at(cols, r0, (1 - fy) * g)
    np.add.at(cols, r1, fy * g)
    out = np.zeros_like(g)
    np.add.at(out, (slice(None), c0), (1 - fx) * cols)
    np.add.at(out, (slice(None), c1), fx * cols)
    return out


def forward(y, jit, key, quantize):
    """y [B][H][W][>= 3], jit [B][J][8], key [B][J] -> (out [J][B][H][W][4], gate uint8 [J][B][H][W], pre [J][B][H][W][3]), float64."""
    y = np.asarray(y, dtype=np.float64)[..., :3]
    B, H, W, _ = y.shape
    J = jit.shape[1]
    pre = np.zeros((J, B, H, W, 3))
    for b in range(B):
        for j in range(J):
            row = np.asarray(jit[b, j], dtype=np.float64)
            p = row[GAIN:GAIN + 3] * shift(y[b], row[DX], row[DY]) + row[OFFSET]
            if row[SIGMA] != 0:
                p = p + row[SIGMA] * normals(key[b, j], H * W).reshape(H, W, 3)
            pre[j, b] = p
    out = np.zeros((J, B, H, W, 4))
    out[..., :3] = np.clip(pre, 0, 1)
    if quantize:
        out = np.floor(out * 255.0) / 255.0
    inside = (pre >= 0) & (pre <= 1)
    gate = (inside[..., 0] * 1 + inside[..., 1] * 2 + inside[..., 2] * 4).astype(np.uint8)
    return out, gate, pre


def backward(g_out, jit, gate):
    """g_out [J][B][H][W][>= 3], gate uint8 [J][B][H][W] -> g_y [J][B][H][W][4] = S^T(gain_c gate_c g_out), the pad channel 0."""
    g_out = np.asarray(g_out, dtype=np.float64)[..., :3]
    J, B, H, W, _ = g_out.shape
    bits = np.stack([(np.asarray(gate) >> c) & 1 for c in range(3)], axis=-1).astype(np.float64)
    out = np.zeros((J, B, H, W, 4))
    for b in range(B):
        for j in range(J):
            row = np.asarray(jit[b, j], dtype=np.float64)
            out[j, b, ..., :3] = shift_T(row[GAIN:GAIN + 3] * bits[j, b] * g_out[j, b], row[DX], row[DY])
    return out


def transform_torch(y, rows, keys, quantize):
    """The transform of one draw in torch (y's dtype) for autograd: y [B,3,H,W], rows [B][8], keys [B] -> out [B,3,H,W].  The
    quantisation is straight-through and the noise a constant, as in the adjoint kernel."""
    B, _, H, W = y.shape
    outs = []
    for b in range(B):
        row = [float(v) for v in rows[b]]
        c0, c1, fx = axis_taps(row[DX], W)
        r0, r1, fy = axis_taps(row[DY], H)
        cols = (1 - fx) * y[b][:, :, torch.as_tensor(c0)] + fx * y[b][:, :, torch.as_tensor(c1)]
        s = (1 - fy) * cols[:, torch.as_tensor(r0)] + fy * cols[:, torch.as_tensor(r1)]
        pre = torch.tensor(row[GAIN:GAIN + 3], dtype=y.dtype).view(3, 1, 1) * s + row[OFFSET]
        if row[SIGMA] != 0:
            n = normals(keys[b], H * W).reshape(H, W, 3).transpose(2, 0, 1)
            pre = pre + row[SIGMA] * torch.from_numpy(np.ascontiguousarray(n)).to(y.dtype)
        o = pre.clamp(0, 1)
        if quantize:
            o = o + (torch.floor(o * 255.0) / 255.0 - o).detach()
        outs.append(o)
    return torch.stack(outs)


def first_iteration(pcnet_sd, oracle_classifier, target, targeted, cam_scene, d_thr, setup_info, jit, key, quantize, p_thresh=0.9,
                    dtype=torch.float64):
    """The first iteration of the jitter attack from the grey projector image, in `dtype` on the CPU, with the tables `jit` [B][J][8] /
    `key` [B][J] given (teacher-forced): y = PCNet(clamp(x), s); member j = the classifier behind draw j's transform, its logits and
    g_bj = d(-/+ logit_j[b, target_b]) / dy through the transform; then the ensemble oracle's decision (no focus) and combination.
    Returns what ensemble_oracle.first_iteration returns."""
    import ensemble_oracle as eo
    import spaa_oracle as so
    B, J = len(target), jit.shape[1]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        cast = lambda sd: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}   # noqa: E731
        c = oracle_classifier
        clf = so.OracleClassifier(c.name, cast(c.sd), sort_results=c.sort_results, input_sz=c.input_sz)
        scene = so.expand_4d(cam_scene.to(dtype)).expand(B, -1, -1, -1)
        x = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), float(setup_info['prj_brightness']))
        with torch.no_grad():
            y = so.pcnet_forward(pcnet_sd if dtype == torch.float32 else cast(pcnet_sd), x.clamp(0, 1), scene)
        y = y.detach().requires_grad_(True)
        sign = torch.tensor([-1.0 if t else 1.0 for t in targeted])
        idx = torch.arange(B)
        logits, gs = [], []
        for j in range(J):
            raw = clf(transform_torch(y, jit[:, j], key[:, j], quantize), setup_info['classifier_crop_sz'])[0]
            g, = torch.autograd.grad((sign * raw[idx, torch.as_tensor(list(target))]).sum(), y)
            logits.append(raw.detach().numpy().astype(np.float64))
            gs.append(g.permute(0, 2, 3, 1).reshape(B, -1, 3).numpy().astype(np.float64))
        caml2 = torch.norm(scene - y.detach(), dim=1).mean(1).mean(1).numpy().astype(np.float64)
    finally:
        torch.set_default_dtype(old)
    out = eo.decide_ens(logits, target, targeted, caml2, d_thr, p_thresh, False)
    top2 = [np.sort(lg, axis=1)[:, -2:] for lg in logits]
    out.update(cam=y.detach(), caml2=caml2, g=gs, g_adv=eo.combine(gs, out['ens_w']), logits=logits,
               gap=np.stack([t[:, 1] - t[:, 0] for t in top2], axis=1),
               p_margin=np.where(np.asarray(targeted, dtype=bool)[:, None], np.abs(out['p1'] - p_thresh), np.inf),
               d_margin=np.abs(caml2 * 255.0 - np.asarray(d_thr, dtype=np.float64)))
    return out


def survives(logits, target, targeted):
    """[N] bool: top-1 == target for a targeted image, top-1 != target otherwise (the rule of attack_transfer)."""
    top1 = np.asarray(logits).argmax(axis=1)
    return np.where(np.asarray(targeted, dtype=bool), top1 == np.asarray(target), top1 != np.asarray(target))
