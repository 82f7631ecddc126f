"""TEST INFRASTRUCTURE: the float64 restatement of torchvision's convnext_tiny (eval) in plain torch, the restatement of the depthwise
7 x 7 layer and its adjoint that tests/test_convnext_ops_gpu.py holds csrc/convnext_ops.hip to, the fixtures of
tests/test_convnext_gpu.py, the bars with their derivation, and `MUTATIONS`: the same functions with one deliberate mistake each
(tests/test_convnext_cpu.py shows that every one lands beyond its bar on the inputs the GPU tests use, so a kernel that made the
mistake could not pass them).  LayerNorm and GELU are those of tests/vit_oracle.py.

Definition (Liu et al. 2022; torchvision's key names), NHWC inside:
  x = LayerNorm(features.0.1)(conv 4 x 4 / 4 (features.0.0))
  per block features.{s}.{i}: x = x + layer_scale * block.5(gelu(block.3(LayerNorm(block.2)(dwconv7(block.0)(x)))))
  between the stages features.{s}: x = conv 2 x 2 / 2 (.1)(LayerNorm(.0)(x)), an odd side losing its last row or column
  logits = classifier.2(LayerNorm(classifier.0)(mean over the pixels of x))
Every LayerNorm is over the channels of a pixel with eps 1e-6.

Bars.  U = 2^-24 is the unit roundoff of fp32.  A chain of n fused multiply-adds acc = fmaf(w, v, acc) from acc = bias carries, to
first order, at most one rounding of magnitude U |partial sum| per step, and every partial sum is at most T = |bias| + sum |w| |v|:
the running-error bound n U T.  One more rounding for the `add` of the backward pass, whose magnitude joins T; forward the + 1 is
kept as well (the bound is not tight, the bar need not be).  n is the number of taps that lie inside the image for that output.
Times SLACK = 2 (tests/vit_oracle.py) for the second-order terms.  No constant is picked by hand."""
import os

import torch
import torch.nn.functional as F

import spaa_oracle as so
import vit_oracle as vo
from spaa_amd import synthetic as syn

U = vo.U
SLACK = vo.SLACK
K, PAD = 7, 3


def note(line):
    """A figure a test measured: printed as an `accuracy:` line and, where the environment variable SPAA_ACCURACY_FILE names a file,
    appended to it (`SPAA_ACCURACY_FILE=profiles/convnext_accuracy.txt pytest -m gpu tests/test_convnext_ops_gpu.py
    tests/test_convnext_gpu.py` on a fresh file is how that file is made)."""
    print('accuracy: ' + line)
    path = os.environ.get('SPAA_ACCURACY_FILE')
    if path:
        with open(path, 'a') as fh:
            fh.write('accuracy: ' + line + '\n')


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------------- the kernel pair, restated
def _taps(w, _bug=None):
    """w [49][C] tap-major -> [7, 7, C]."""
    c = w.shape[1]
    if _bug == 'weight_channel_major':          # the same memory read as [C][49]
        w = w.reshape(c, K * K).t()
    return w.reshape(K, K, c)


def _correlate(x, wk, pad):
    """out[y, x] = sum wk[ky, kx] in[y - pad + ky, x - pad + kx], zeros outside, output of the input's size; NHWC."""
    b, h, w, c = x.shape
    m = PAD + 1                                   # margin wide enough for the padding mutations
    xp = F.pad(x, (0, 0, m, m, m, m))
    out = torch.zeros_like(x)
    for ky in range(K):
        for kx in range(K):
            y0, x0 = m - pad + ky, m - pad + kx
            out = out + wk[ky, kx] * xp[:, y0:y0 + h, x0:x0 + w]
    return out


def dwconv7(x, w, bias=None, _bug=None):
    """Depthwise 7 x 7, stride 1, zero padding 3: x [B, H, W, C], w [49][C] (tap 7 ky + kx), bias [C]."""
    wk = _taps(w, _bug)
    if _bug == 'window_mirrored':
        wk = wk.flip(0, 1)
    if _bug == 'ky_kx_swapped':
        wk = wk.transpose(0, 1)
    out = _correlate(x, wk, {'padding_2': 2, 'padding_4': 4}.get(_bug, PAD))
    return out if bias is None or _bug == 'bias_dropped' else out + bias


def dwconv7_bwd(g, w, add=None, _bug=None):
    """The adjoint: g_in[y, x] = add[y, x] + sum w[ky, kx] g[y + 3 - ky, x + 3 - kx]."""
    wk = _taps(w, _bug)
    if _bug != 'adjoint_not_mirrored':
        wk = wk.flip(0, 1)
    if _bug == 'ky_kx_swapped':
        wk = wk.transpose(0, 1)
    out = _correlate(g, wk, PAD)
    return out if add is None or _bug == 'add_dropped' else out + add


def tap_count(h, w):
    """[1, h, w, 1]: how many of the 49 taps lie inside the image for each output (the same map for the adjoint)."""
    return dwconv7(torch.ones(1, h, w, 1, dtype=torch.float64), torch.ones(K * K, 1, dtype=torch.float64))


def bar_dwconv7(x, w, bias):
    """Per-element bound for spaa_dwconv7_fwd on the float64 tensors (fp32 values): SLACK (n + 1) U (|bias| + sum |w| |v|)."""
    n = tap_count(x.shape[1], x.shape[2])
    return SLACK * (n + 1) * U * dwconv7(x.abs(), w.abs(), bias.abs())


def bar_dwconv7_bwd(g, w, add=None):
    """... and for spaa_dwconv7_bwd: SLACK (n + 1) U (sum |w| |g| + |add|)."""
    n = tap_count(g.shape[1], g.shape[2])
    return SLACK * (n + 1) * U * dwconv7_bwd(g.abs(), w.abs(), None if add is None else add.abs())


# (B, H, W, C) of tests/test_convnext_ops_gpu.py: a map smaller than the window in both axes and in one, a width that no strip length
# divides, one channel quad, quad counts that are no multiple of a wave (C = 8, 12), more quads than a wave, the largest stage map
DW_CASES = [(1, 1, 1, 4), (2, 2, 3, 8), (1, 7, 7, 768), (2, 9, 13, 96), (1, 14, 14, 384), (3, 20, 37, 12), (1, 56, 56, 96)]


def dw_inputs(b, h, w, c):
    """x, weight [49][C], bias, the output gradient g and the summand add: fp32 values on the CPU."""
    gen = torch.Generator().manual_seed(((b * 131 + h) * 131 + w) * 131 + c)
    x = torch.randn(b, h, w, c, generator=gen) * 1.5 + 0.3
    wt = torch.randn(K * K, c, generator=gen) / K
    bias = torch.rand(c, generator=gen) * 2 - 1
    g = torch.randn(b, h, w, c, generator=gen)
    add = torch.randn(b, h, w, c, generator=gen)
    return x, wt, bias, g, add


# ------------------------------------------------------------------------------------------------------------------------ the network
def config(sd):
    dims, depths, s = [], [], 1
    while f'features.{s}.0.block.0.weight' in sd:
        n = 0
        while f'features.{s}.{n}.block.0.weight' in sd:
            n += 1
        dims.append(int(sd[f'features.{s}.0.block.0.weight'].shape[0]))
        depths.append(n)
        s += 2
    return tuple(dims), tuple(depths)


def dw_weight(w):
    """[C, 1, 7, 7] -> [49][C]."""
    return w.reshape(w.shape[0], K * K).t()


def patch_conv(x, w, b):
    """A P x P / stride-P convolution without padding on NHWC x (a side that P does not divide loses its remainder): w [N, Cin, P, P]."""
    n, cin, P, _ = w.shape
    bsz, h, wd, _ = x.shape
    ho, wo = h // P, wd // P
    t = x[:, :ho * P, :wo * P].reshape(bsz, ho, P, wo, P, cin).permute(0, 1, 3, 2, 4, 5).reshape(bsz, ho, wo, P * P * cin)
    return t @ w.permute(0, 2, 3, 1).reshape(n, P * P * cin).t() + b


def block(sd, p, x, _bug=None):
    d = dwconv7(x, dw_weight(sd[p + 'block.0.weight']), sd[p + 'block.0.bias'])
    n = vo.layernorm(d, sd[p + 'block.2.weight'], sd[p + 'block.2.bias'])[0]
    a = vo.gelu(n @ sd[p + 'block.3.weight'].t() + sd[p + 'block.3.bias'])
    branch = a @ sd[p + 'block.5.weight'].t() + sd[p + 'block.5.bias']
    ls = sd[p + 'layer_scale'].reshape(-1)
    return ls * (x + branch) if _bug == 'layer_scale_on_residual' else x + ls * branch


def forward(sd, x, record=None, _bug=None):
    """x: the normalised input [B, 3, h, w] -> logits [B, ncls].  `record` (a dict) receives 'stem', 'blocks' (every block's output in
    order), 'feat' (the last of them: the map the head pools), 'pooled' and 'normed', all NHWC."""
    dims, depths = config(sd)
    t = patch_conv(x.permute(0, 2, 3, 1), sd['features.0.0.weight'], sd['features.0.0.bias'])
    t = vo.layernorm(t, sd['features.0.1.weight'], sd['features.0.1.bias'])[0]
    rec = dict(stem=t, blocks=[])
    for si, depth in enumerate(depths):
        s = 2 * si + 1
        if si > 0:
            t = vo.layernorm(t, sd[f'features.{s - 1}.0.weight'], sd[f'features.{s - 1}.0.bias'])[0]
            t = patch_conv(t, sd[f'features.{s - 1}.1.weight'], sd[f'features.{s - 1}.1.bias'])
        for i in range(depth):
            t = block(sd, f'features.{s}.{i}.', t, _bug)
            rec['blocks'].append(t)
    rec['feat'] = t
    rec['pooled'] = t.mean(dim=(1, 2))
    rec['normed'] = vo.layernorm(rec['pooled'], sd['classifier.0.weight'], sd['classifier.0.bias'])[0]
    if record is not None:
        record.update(rec)
    return rec['normed'] @ sd['classifier.2.weight'].t() + sd['classifier.2.bias']


def classifier(sd, input_sz, sort_results=True):
    """The oracle-side stand-in for Classifier('convnext_tiny', ...): (im, crop_sz) -> (raw_score, p_sorted ndarray, idx ndarray)."""

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


# --------------------------------------------------------------------------------------------- fixtures of tests/test_convnext_gpu.py
NUM_CLASSES, LOGIT_GAIN, B = 16, 4.0, 3
DIMS, DEPTHS = (16, 32, 48, 64), (1, 1, 2, 1)
# name -> (image H x W, classifier crop, network input): maps 16, 8, 4, 2 / 9 x 13 -> 4 x 6 -> 2 x 3 -> 1 x 1 (odd at the first two
# downsamples, smaller than the 7 x 7 window from the second stage on)
GEOMS = {'square': ((64, 64), (60, 60), (64, 64)), 'odd': ((40, 56), (36, 52), (36, 52))}
_SD = {}


def state_dict(full=False):
    """The test network (narrow and shallow, the same key layout), or with `full` torchvision's real widths and depths."""
    if full not in _SD:
        kw = {} if full else dict(dims=DIMS, depths=DEPTHS)
        _SD[full] = syn.convnext_tiny_state_dict(8, num_classes=NUM_CLASSES, logit_gain=LOGIT_GAIN, **kw)
    return _SD[full]


def images(geom):
    (h, w) = GEOMS[geom][0]
    return torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(31 + sorted(GEOMS).index(geom)))


# -------------------------------------------------------------------------------------------------------------------------- mutations
# name -> the functions that make the mistake (called with _bug=name)
MUTATIONS = {
    'window_mirrored': (dwconv7,),
    'adjoint_not_mirrored': (dwconv7_bwd,),
    'padding_2': (dwconv7,),
    'padding_4': (dwconv7,),
    'ky_kx_swapped': (dwconv7, dwconv7_bwd),
    'bias_dropped': (dwconv7,),
    'add_dropped': (dwconv7_bwd,),
    'weight_channel_major': (dwconv7, dwconv7_bwd),
    'layer_scale_on_residual': (forward,),
}
# where a mistake cannot show: on a 1 x 1 map only the centre tap lies inside the image, which a mirror or a transposition leaves in place
BLIND = {('window_mirrored', (1, 1, 1, 4)), ('adjoint_not_mirrored', (1, 1, 1, 4)), ('ky_kx_swapped', (1, 1, 1, 4))}
