"""TEST INFRASTRUCTURE: torchvision's mobilenet_v2 (eval, width 1.0) restated in plain torch from the published architecture
(Sandler et al. 2018) and torchvision's key names, in whatever dtype the weights and the input have (the tests use float64).

`forward(sd, x, record=None, gates=None)` -> logits.
  record: a list that receives, per ReLU6 site in the order of SITES, the PRE-activation (NCHW, detached).
  gates : a list of 35 boolean NCHW tensors: the value of every ReLU6 is still clamp(v, 0, 6), but its DERIVATIVE is the given gate
          instead of (0 < v < 6) -- how the parity tests run the float64 backward pass with the HIP pass's own gates (tests/gates.py
          explains why).
`feature(sd, x)` additionally returns the clamped features.18 map (what Grad-CAM reads).
`classifier(sd, input_sz)` wraps it as the (im, crop_sz) -> (raw_score, p_sorted, idx) callable the oracle's spaa() takes.
"""
import torch
import torch.nn.functional as F

import spaa_oracle as so

BLOCK_TABLE = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def blocks():
    """(name, t, cin, cout, stride) of features.1 .. features.17."""
    out, cin, idx = [], 32, 1
    for t, c, n, s in BLOCK_TABLE:
        for i in range(n):
            out.append((f'features.{idx}', t, cin, c, s if i == 0 else 1))
            cin, idx = c, idx + 1
    return out


def sites():
    """Names of the 35 ReLU6 sites in forward order."""
    out = ['features.0']
    for name, t, _, _, _ in blocks():
        if t != 1:
            out.append(name + '.expand')
        out.append(name + '.dw')
    return out + ['features.18']


SITES = sites()
assert len(SITES) == 35


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, 1e-5)


class _Relu6:
    def __init__(self, record, gates):
        self.record, self.gates, self.n = record, gates, 0

    def __call__(self, v):
        if self.record is not None:
            self.record.append(v.detach())
        i, self.n = self.n, self.n + 1
        if self.gates is None:
            return F.hardtanh(v, 0.0, 6.0)
        lin = v * self.gates[i].to(v.dtype)
        return (F.hardtanh(v, 0.0, 6.0) - lin).detach() + lin


def feature(sd, x, record=None, gates=None):
    r6 = _Relu6(record, gates)
    x = r6(_bn(sd, 'features.0.1', F.conv2d(x, sd['features.0.0.weight'], None, 2, 1)))
    for name, t, cin, cout, stride in blocks():
        p, idt, j = name + '.conv', x, 0
        hid = cin * t
        if t != 1:
            x = r6(_bn(sd, f'{p}.0.1', F.conv2d(x, sd[f'{p}.0.0.weight'])))
            j = 1
        x = r6(_bn(sd, f'{p}.{j}.1', F.conv2d(x, sd[f'{p}.{j}.0.weight'], None, stride, 1, 1, hid)))
        x = _bn(sd, f'{p}.{j + 2}', F.conv2d(x, sd[f'{p}.{j + 1}.weight']))
        if stride == 1 and cin == cout:
            x = x + idt
    x = r6(_bn(sd, 'features.18.1', F.conv2d(x, sd['features.18.0.weight'])))
    assert r6.n == 35
    logits = F.linear(F.adaptive_avg_pool2d(x, 1).flatten(1), sd['classifier.1.weight'], sd['classifier.1.bias'])   # (dropout: identity in eval)
    return logits, x


def forward(sd, x, record=None, gates=None):
    return feature(sd, x, record, gates)[0]


def classifier(sd, input_sz, sort_results=True):
    """The oracle-side stand-in for Classifier('mobilenet_v2', ...): (im, crop_sz) -> (raw_score, p_sorted ndarray, idx ndarray)."""

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
