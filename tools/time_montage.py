"""Time of the result montages of one setup (spaa_amd.montage.attack_montages, csrc/montage.hip) against the per-image composition
of the reference's structure written with torch ops on the same GPU.  A record, not a gate: one JSON line appended to
profiles/montage_time.jsonl.

    python tools/time_montage.py [--out profiles/montage_time.jsonl] [--cfgs 12] [--cam 240 320] [--crop 240 240] [--prj 256 256]

Workload: `cfgs` configurations x 11 attacks.  Measured: the device time of the two entry points (HIP events), the end-to-end time
of attack_montages + the copy to the host + the PNG writes (io.save_imgs), and, for comparison, one montage at a time from
F.interpolate(mode='area'), min / max, the host round trip for the colour map and the grid assembly -- what the reference's
attack_results costs without its seven PIL round trips for the text (the comparison draws no text).
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
import torch.nn.functional as F  # noqa: E402

from spaa_amd import io, montage as mt  # noqa: E402
from spaa_amd.img_proc import center_crop  # noqa: E402


def torch_montage(scene, prj, infer, real, cp_sz, lut):
    """One montage, float [3,Hm,Wm] on the device, as projector_based_attack.py:365-394 builds it (no text)."""
    size = tuple(prj.shape[-2:])
    s, i, r = (F.interpolate(center_crop(x, cp_sz)[None], size, mode='area')[0] for x in (scene, infer, real))
    d = torch.abs(r - s)
    d = (d - d.min()) / (d.max() - d.min())
    colour = torch.from_numpy(lut[np.uint8(d.cpu().numpy().mean(0) * 255)].transpose(2, 0, 1).astype(np.float32) / 255).to(scene.device)
    hp, wp = size
    grid = torch.ones(3, hp + 10, 5 * (wp + 5) + 5, device=scene.device)
    for k, t in enumerate((s, prj, i, r, colour)):
        grid[:, 5:5 + hp, 5 + k * (wp + 5):5 + k * (wp + 5) + wp] = t
    return torch.cat((torch.ones(3, 26, grid.shape[-1], device=scene.device), grid), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=join(ROOT, 'profiles', 'montage_time.jsonl'))
    ap.add_argument('--cfgs', type=int, default=12)
    ap.add_argument('--cam', type=int, nargs=2, default=(240, 320), help='camera image size (h, w)')
    ap.add_argument('--crop', type=int, nargs=2, default=(240, 240), help='classifier crop size (h, w)')
    ap.add_argument('--prj', type=int, nargs=2, default=(256, 256))
    ap.add_argument('--repeat', type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_montage needs a GPU'
    dev = torch.device('cuda', 0)
    n = 11 * a.cfgs
    g = torch.Generator().manual_seed(0)
    scene = (torch.randint(0, 256, (3, *a.cam), generator=g).float() / 255).to(dev)
    prj = (torch.randint(0, 256, (n, 3, *a.prj), generator=g).float() / 255).to(dev)
    infer = (torch.randint(0, 256, (n, 3, *a.cam), generator=g).float() / 255).to(dev)
    real = (torch.randint(0, 256, (n, 3, *a.cam), generator=g).float() / 255).to(dev)
    texts = [mt.attack_texts(t % 11, ('tabby, tabby cat', 0.87), ('hamster', 0.64), ('hamster', 0.51), (4.56, 7.89, 8.12)) for t in range(n)]
    cp = tuple(a.crop)
    best = None
    with tempfile.TemporaryDirectory() as root:
        for rep in range(a.repeat + 1):             # the first pass also loads the library and creates the context
            launches = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mt.attack_montages(scene, prj, infer, real, cp, texts, timings=launches)
            host = out.permute(0, 2, 3, 1).cpu().numpy()
            t1 = time.perf_counter()
            for k in range(a.cfgs):
                io.save_imgs(host[11 * k:11 * (k + 1)], join(root, 'hip', str(k)))
            t2 = time.perf_counter()
            rec = dict(compose_and_copy_s=t1 - t0, png_write_s=t2 - t1, end_to_end_s=t2 - t0,
                       **{name + '_us': 1e3 * e0.elapsed_time(e1) for name, e0, e1 in launches})
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ims = torch.stack([torch_montage(scene, prj[i], infer[i], real[i], cp, mt.JET) for i in range(n)])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for k in range(a.cfgs):
                io.save_imgs(ims[11 * k:11 * (k + 1)], join(root, 'torch', str(k)))
            t2 = time.perf_counter()
            rec.update(torch_per_image_compose_s=t1 - t0, torch_per_image_end_to_end_s=t2 - t0)
            if rep and (best is None or rec['end_to_end_s'] < best['end_to_end_s']):
                best = rec
    rec = dict(tool='time_montage', montages=n, cam_sz=list(a.cam), crop_sz=list(a.crop), prj_sz=list(a.prj),
               montage_sz=list(mt.montage_size(*a.prj)), output_mb=round(out.numel() / 1e6, 1),
               **{k: round(v, 6 if k.endswith('_s') else 1) for k, v in best.items()}, device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as fh:
        fh.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
