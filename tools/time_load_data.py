"""Time of train_network.load_data on a synthetic setup directory, split into the host's PNG decode and the three launches of the
direct-light mask (csrc/direct_mask.hip).  A record, not a gate: one JSON line appended to profiles/load_data_time.jsonl.

    python tools/time_load_data.py [--out profiles/load_data_time.jsonl] [--cam 240 320] [--prj 256 256] [--train 50] [--cb 10]
"""
import argparse
import json
import os
import sys
import tempfile
import time
from os.path import join

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spaa_amd import img_proc, io, synthetic as syn  # noqa: E402
from spaa_amd import train_network as tn  # noqa: E402


def write_setup(root, cam, prj, n_train, n_valid, n_cb):
    """Random smooth images in the reference's folders; the checkerboard captures light a centred rectangle."""
    setup = join(root, 'setups', 'synth')
    io.save_setup_info(setup, dict(classifier_crop_sz=(min(cam),) * 2, prj_brightness=0.5, prj_im_sz=prj, cam_im_sz=cam[::-1]))
    io.save_imgs(syn.scenes(1, 2, cam), join(setup, 'cam/raw/ref'))
    io.save_imgs(syn.scenes(2, n_train, cam), join(setup, 'cam/raw/train'))
    io.save_imgs(syn.scenes(3, n_valid, cam), join(setup, 'cam/raw/test'))
    io.save_imgs(syn.scenes(4, n_train, prj), join(root, 'prj_share/train'))
    io.save_imgs(syn.scenes(5, n_valid, prj), join(root, 'prj_share/test'))
    h, w = cam
    yy, xx = np.mgrid[0:h, 0:w]
    lit = (abs(yy - h / 2) < h / 3) & (abs(xx - w / 2) < w / 3)
    albedo = syn.scenes(6, 1, cam, lo=0.4, hi=1.0)[0]
    cb = torch.stack([albedo * torch.from_numpy(lit * 0.5 * (0.9 + 0.1 * (((yy + 3 * k) // 16 + (xx + 5 * k) // 16) % 2)) + 0.03).float()
                      for k in range(n_cb)])
    io.save_imgs(cb.clamp(0, 1), join(setup, 'cam/raw/cb'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=join(ROOT, 'profiles', 'load_data_time.jsonl'))
    ap.add_argument('--cam', type=int, nargs=2, default=(240, 320), help='camera image size (h, w)')
    ap.add_argument('--prj', type=int, nargs=2, default=(256, 256))
    ap.add_argument('--train', type=int, default=50)
    ap.add_argument('--valid', type=int, default=20)
    ap.add_argument('--cb', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--gpu-decode', action='store_true', help='decode the PNG files on the device (load_data(gpu_decode=True))')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_load_data needs a GPU'
    decode_s, launches = [0.0], []
    imread, dmask = io.torch_imread_mt, img_proc.direct_mask

    def timed_imread(*args, **kw):
        t0 = time.perf_counter()
        r = imread(*args, **kw)
        decode_s[0] += time.perf_counter() - t0
        return r

    io.torch_imread_mt = timed_imread
    img_proc.direct_mask = lambda *args, **kw: dmask(*args, timings=launches, **kw)
    with tempfile.TemporaryDirectory() as root:
        write_setup(root, tuple(a.cam), tuple(a.prj), a.train, a.valid, a.cb)
        best = None
        for _ in range(a.repeat + 1):               # the first pass also loads the library and creates the context
            decode_s[0], launches[:] = 0.0, []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tn.load_data(root, 'synth', device='cuda', gpu_decode=a.gpu_decode)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            rec = dict(total_s=total, png_decode_s=decode_s[0], **{name + '_us': 1e3 * e0.elapsed_time(e1) for name, e0, e1 in launches})
            best = rec if best is None or _ == 1 or rec['total_s'] < best['total_s'] else best
    rec = dict(tool='time_load_data', gpu_decode=a.gpu_decode, cam_sz=list(a.cam), prj_sz=list(a.prj), n_train=a.train, n_valid=a.valid, n_cb=a.cb,
               mask_pixels=int(out[5].sum()), **{k: round(v, 6 if k.endswith('_s') else 1) for k, v in best.items()},
               device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as fh:
        fh.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
