"""TEST INFRASTRUCTURE: the MobileNetV2 fixtures that tests/test_mobilenet_cpu.py (the saturation condition, checked on the CPU) and
tests/test_mobilenet_gpu.py (the parity tests) share: the synthetic weights, the two geometries and their input images."""
import torch

from spaa_amd import synthetic as syn

NUM_CLASSES = 16
LOGIT_GAIN = 4.0     # softmax over the 16 logits is not flat: test_mobilenet_cpu.py asserts the top-1 probabilities it gives
B = 3
# (image H x W, classifier crop, network input): a square one whose final map is 2 x 2, and a non-square one that is odd at every
# stride-2 layer (33 x 47 -> 17 x 24 -> 9 x 12 -> 5 x 6 -> 3 x 3 -> 2 x 2)
GEOMS = {'square': ((64, 64), (60, 60), (64, 64)), 'odd': ((40, 52), (36, 48), (33, 47))}
_SD = {}


def state_dict():
    if 'sd' not in _SD:
        _SD['sd'] = syn.mobilenet_v2_state_dict(6, num_classes=NUM_CLASSES, logit_gain=LOGIT_GAIN)
    return _SD['sd']


def images(geom):
    """The B camera-frame images [B, 3, H, W] in [0, 1) of a geometry."""
    (h, w), _, _ = GEOMS[geom]
    g = torch.Generator().manual_seed(11 + sorted(GEOMS).index(geom))
    return torch.rand(B, 3, h, w, generator=g)
