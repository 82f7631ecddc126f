"""On-disk formats either side of the attack path, with the reference's conventions (host side; PNG encoding of device tensors aside,
PNG decoding to device tensors aside, no GPU work).

Mirrors /root/reference/src/python:
  utils.py:84-167     SimpleDataset / torch_imread / torch_imread_mt / save_imgs  (PNG via OpenCV there: BGR on disk order
                      is an OpenCV-internal detail, files hold ordinary RGB PNGs; float images are written with
                      np.uint8(x * 255), i.e. TRUNCATION, file names img_%04d.png counted from 1 + idx)
  train_network.py:85-95, utils.py:674-675   load_setup_info / save of setup_info.yml (OmegaConf/yaml mapping)
  utils.py:679-680, :717-721                 opt_to_string / save_checkpoint (state_dict in `<dir>/<title>.pth`)
so that a setup directory captured and trained by the reference can be consumed, and results land where its
`summarize_*` functions expect them.  Pillow replaces OpenCV as the codec (OpenCV is not a dependency of this package); images that
are already on the GPU are encoded there (spaa_amd/png.py).
"""
import os
import warnings
from os.path import abspath, join

import numpy as np
import torch
import torch.nn.functional as F
import yaml
from PIL import Image

from . import png


def _imread_rgb(filename):
    with Image.open(filename) as im:
        return np.asarray(im.convert('RGB'))  # cv.imread(...)[..., ::-1]: 8-bit, 3 channels, alpha dropped


def _read_bytes(path):
    with open(path, 'rb') as fh:
        return fh.read()


def _imread_device(paths, device):
    """The files as uint8 tensors [3,H,W] on `device`: those `png.parse_png` accepts are decoded there in one `png.decode_records`
    batch, the rest (palette, 16-bit, interlaced, not PNG at all) are read through Pillow and copied over.  A PNG file that is
    broken raises ValueError with its path; it is never handed to Pillow instead."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError(f'spaa_amd.io decodes on the GPU or, with device=None, through Pillow; got device={device}')
    out, records, where = [None] * len(paths), [], []
    for i, path in enumerate(paths):
        data = _read_bytes(path)
        rec = None
        if data[:8] == png.PNG_SIGNATURE:
            try:
                rec = png.parse_png(data)
            except ValueError as e:
                raise ValueError(f'{path}: {e}') from None
        if rec is None:
            out[i] = torch.from_numpy(_imread_rgb(path).transpose(2, 0, 1).copy()).to(device)
        else:
            records.append(rec)
            where.append(i)
    images, status = png.decode_records(records, device)
    bad = [f'{paths[where[k]]}: {png.STATUS_TEXT.get(int(st), "status " + str(int(st)))}' for k, st in enumerate(status) if st]
    if bad:
        raise ValueError('PNG decode failed: ' + '; '.join(bad))
    for k, im in zip(where, images):
        out[k] = im
    return out


def _div255(x):
    """x / 255 with the host's rounding.  On a GPU, torch divides by a Python number by multiplying with its reciprocal, which is
    one rounding more than the host's division; dividing by a tensor on the device is a true division there."""
    return x / torch.full((), 255.0, device=x.device) if x.is_cuda else x.div(255)


def torch_imread(filename, *, device=None):
    """utils.py:116-117: float tensor [3,H,W] in [0,1].  `device`: a CUDA device decodes the file there (spaa_amd.png) and returns a
    tensor on it, bit-equal to the host result."""
    if device is not None:
        return _div255(_imread_device([filename], device)[0].float())
    return torch.from_numpy(_imread_rgb(filename).transpose(2, 0, 1).copy()).float() / 255


def torch_imread_mt(img_dir, size=None, index=None, gray_scale=False, normalize=False, *, device=None):
    """utils.py:120-143: every image of a directory in sorted order -> [N,3,H,W] (or [N,1,H,W]) in [0,1] ([-1,1]).
    `size` is (h, w); resizing is bilinear with half-pixel centres like cv.resize's default (the reference resizes the
    uint8 image in fixed point: results can differ by one grey level).
    `device=None`: Pillow, one file after the other, a host tensor.  A CUDA device: the files are read as bytes and decoded on that
    device in one batch (spaa_amd.png.decode_records; files its parser declines go through Pillow one by one), and the same
    expressions run there: the result is a tensor on the device, bit-equal to the host result moved over, except after a resize,
    where the two bilinear kernels may round differently before the `round()` (one grey level)."""
    names = sorted(os.listdir(img_dir))
    if index is not None:
        names = [names[i] for i in index]
    paths = [join(img_dir, n) for n in names]
    for path in paths:
        assert os.path.isfile(path), path + ' does not exist'
    ims = []
    for im in (_imread_device(paths, device) if device is not None else
               (torch.from_numpy(_imread_rgb(path).transpose(2, 0, 1).copy()) for path in paths)):
        im = im.float()
        if size is not None and tuple(im.shape[-2:]) != tuple(size):
            im = F.interpolate(im[None], tuple(size), mode='bilinear', align_corners=False)[0].round().clamp(0, 255)
        ims.append(im)
    imgs = _div255(torch.stack(ims))
    if gray_scale:
        imgs = (0.2989 * imgs[:, 0] + 0.5870 * imgs[:, 1] + 0.1140 * imgs[:, 2])[:, None]
    if normalize:
        imgs = (imgs - 0.5) / 0.5
    return imgs


def save_imgs(im_4d, path, idx=0):
    """utils.py:146-167: [N,3,H,W] tensor or [N,H,W,3] array -> path/img_%04d.png numbered from idx + 1; float images are
    scaled by 255 and truncated to uint8 exactly as `np.uint8(x * 255)` does.
    A float32 or uint8 CUDA tensor [N,3,H,W] is encoded on its device (spaa_amd.png.encode_png: same names, same decoded pixels;
    float values outside [0,1] keep the low 8 bits of the truncated product); anything else -- host arrays, CPU tensors, other
    dtypes -- is written through Pillow."""
    os.makedirs(path, exist_ok=True)
    if isinstance(im_4d, torch.Tensor) and im_4d.is_cuda and im_4d.ndim == 4 and im_4d.shape[1] == 3 and im_4d.numel() > 0 and \
            im_4d.dtype in (torch.float32, torch.uint8) and 3 * im_4d.shape[3] <= png.MAX_ROW_BYTES:
        for i, data in enumerate(png.encode_png(im_4d)):
            with open(join(path, 'img_{:04d}.png'.format(i + 1 + idx)), 'wb') as fh:
                fh.write(data)
        return
    if isinstance(im_4d, torch.Tensor):
        imgs = im_4d.detach().cpu().numpy().transpose(0, 2, 3, 1)
    else:
        imgs = np.asarray(im_4d)
    if imgs.dtype == np.float32:
        imgs = np.uint8(imgs * 255)
    for i in range(imgs.shape[0]):
        Image.fromarray(np.ascontiguousarray(imgs[i])).save(join(path, 'img_{:04d}.png'.format(i + 1 + idx)))


class SetupInfo(dict):
    """Mapping with attribute access (the reference passes an OmegaConf DictConfig: both `cfg.key` and `cfg['key']`)."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def load_setup_info(setup_path):
    """train_network.py:85-95: `<setup>/setup_info.yml`, else `<setup>/../setup_info_default.yml` with a warning."""
    fn = join(setup_path, 'setup_info.yml')
    if not os.path.exists(fn):
        default = join(setup_path, '../setup_info_default.yml')
        warnings.warn(f'{fn} not found, loading {default} instead')
        fn = default
    with open(fn) as fh:
        cfg = yaml.safe_load(fh)
    return SetupInfo({k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()})


def save_setup_info(setup_path, cfg):
    """utils.py:672-675."""
    os.makedirs(setup_path, exist_ok=True)
    with open(join(setup_path, 'setup_info.yml'), 'w') as fh:
        yaml.safe_dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in dict(cfg).items()}, fh)


def opt_to_string(opt):
    """utils.py:679-680: the checkpoint / log title of a training configuration."""
    return (f'{opt["setup_name"]}_{opt["model_name"]}_{opt["loss"]}_{opt["num_train"]}_{opt["batch_size"]}_{opt["max_iters"]}_'
            f'{opt["lr"]}_{opt["lr_drop_ratio"]}_{opt["lr_drop_rate"]}_{opt["l2_reg"]}')


def save_checkpoint(checkpoint_dir, model, title):
    """utils.py:717-721."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    fn = abspath(join(checkpoint_dir, title + '.pth'))
    torch.save(model.state_dict(), fn)
    return fn


def load_checkpoint(model, filename, map_location='cpu'):
    """Loads a reference-trained `.pth` (state_dict, possibly with nested DataParallel 'module.' prefixes) into a
    spaa_amd module (PCNet / CompenNetPlusplus strip the prefixes themselves)."""
    model.load_state_dict(torch.load(filename, map_location=map_location))
    return model
