"""The reference's montage composition (projector_based_attack.py:362-414) restated on the CPU with the calls the reference itself
makes: centre crop, F.interpolate(mode='area'), torch abs / min / max and the normalisation, numpy `.mean(0)` and `np.uint8(. * 255)`,
a table lookup for cv.applyColorMap, a restated torchvision make_grid(nrow=5, padding=5, pad_value=1), the 26-pixel top border, and
the final np.uint8(x * 255) of utils.save_imgs.  The text is stamped from the product's own font table and `layout_labels` (the
reference renders a TrueType font through PIL; that difference is documented, not tested).  A constant difference image, where the
reference divides by zero, takes colour index 0.  Not the reference's code; no GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from spaa_amd import montage as mt


def cc(x, size):
    """img_proc.py:126-132 (center_crop)."""
    h, w = x.shape[-2:]
    th, tw = size
    i, j = int(round((h - th) / 2.)), int(round((w - tw) / 2.))
    return x[..., i:i + th, j:j + tw]


def rz(x, cp_sz, size):
    """resize(cc(x, cp_sz), size) of one [3,H,W] CPU image (img_proc.py:174-197 for a 3-D tensor)."""
    return F.interpolate(cc(x, cp_sz)[None].contiguous(), tuple(size), mode='area')[0]


def diff(scene, real, cp_sz, size):
    """(|rz(real) - rz(scene)| float32 [3,Hp,Wp], its min, its max)."""
    d = torch.abs(rz(real, cp_sz, size) - rz(scene, cp_sz, size))
    return d, d.min(), d.max()


def diff_index(scene, real, cp_sz, size):
    """uint8 [Hp,Wp]: the colour index of the difference tile (:377-381)."""
    d, mn, mx = diff(scene, real, cp_sz, size)
    if mx == mn:
        return np.zeros(tuple(size), dtype=np.uint8)
    d = (d - mn) / (mx - mn)
    return np.uint8(d.numpy().mean(0) * 255)


def stamp(im_u8, texts, Wp):
    """Text of one montage uint8 [3,Hm,Wm] in place: every set font bit inside the image becomes (0, 0, 0)."""
    _, hm, wm = im_u8.shape
    for x, y, g in mt.layout_labels(texts, Wp):
        for gy in range(mt.FONT_H):
            for gx in range(mt.FONT_W):
                if (mt.FONT[g, gy] >> gx) & 1 and 0 <= y + gy < hm and 0 <= x + gx < wm:
                    im_u8[:, y + gy, x + gx] = 0
    return im_u8


def montage(scene, prj, infer, real, cp_sz, texts, lut=mt.JET):
    """uint8 [3,Hm,Wm] of one attack: scene [3,Hs,Ws], prj [3,Hp,Wp], infer, real [3,H,W] float32 CPU tensors in [0,1]."""
    hp, wp = prj.shape[-2:]
    colour = torch.from_numpy(np.asarray(lut)[diff_index(scene, real, cp_sz, (hp, wp))].transpose(2, 0, 1).astype(np.float32)) / 255
    tiles = (rz(scene, cp_sz, (hp, wp)), prj, rz(infer, cp_sz, (hp, wp)), rz(real, cp_sz, (hp, wp)), colour)
    grid = torch.ones(3, hp + 10, 5 * (wp + 5) + 5)                         # make_grid(nrow=5, padding=5, pad_value=1)
    for k, t in enumerate(tiles):
        grid[:, 5:5 + hp, 5 + k * (wp + 5):5 + k * (wp + 5) + wp] = t
    im = torch.cat((torch.ones(3, 26, grid.shape[-1]), grid), 1)           # expand_boarder(im, (0, 26, 0, 0))
    return stamp(np.uint8(im.numpy() * 255), texts, wp)
