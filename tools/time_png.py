"""Time of writing PNG files from device-resident images: io.save_imgs' GPU route (spaa_amd.png.encode_png, csrc/png.hip) against
the route it replaces, the same tensors copied to the host and written one by one through Pillow.  A record, not a gate: one JSON
line appended to profiles/png_time.jsonl.

    python tools/time_png.py [--out profiles/png_time.jsonl] [--passes 3]

Two workloads, each written as folders of 11 images, one save_imgs call per folder (what the drivers do):
  floats    528 float32 images, 264 of 256 x 256 and 264 of 240 x 320: synthetic.scenes plus uniform noise of +-8 grey levels
            (one classifier's SPAA sweep: 24 folders x 11 images x 2 kinds)
  montages  132 uint8 montages of 292 x 1310 from montage.attack_montages (12 configurations x 11 attacks)
Per workload: the end-to-end wall time of each route over `passes` passes, the routes alternating (median, min, max); one more pass
of the new route with a device synchronise after every step, which splits it into the filter launch, the copy of the histograms, the
host's Huffman tables, the pack launch, the copy of the deflate streams, and CRC + file writes; and, for information only, Pillow
at compress_level=1 in a pool of 16 threads.  Every file of the new route is read back once and compared with the tensor.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from os.path import join

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from spaa_amd import io, montage as mt, png, synthetic as syn  # noqa: E402

PER_FOLDER = 11


def float_batches(dev):
    g = torch.Generator().manual_seed(0)
    out = []
    for k, sz in enumerate(((256, 256), (240, 320))):
        x = syn.scenes(10 + k, 264, sz)
        x = (x + (torch.randint(-8, 9, x.shape, generator=g).float() / 255)).clamp(0, 1).to(dev)
        out += list(x.split(PER_FOLDER))
    return out


def montage_batches(dev):
    n = 132
    g = torch.Generator().manual_seed(1)
    scene = syn.scenes(20, 1, (240, 320))[0].to(dev)
    prj = syn.scenes(21, n, (256, 256)).to(dev)
    infer = (syn.scenes(22, n, (240, 320)) + torch.randint(-8, 9, (n, 3, 240, 320), generator=g).float() / 255).clamp(0, 1).to(dev)
    real = (syn.scenes(23, n, (240, 320)) + torch.randint(-8, 9, (n, 3, 240, 320), generator=g).float() / 255).clamp(0, 1).to(dev)
    texts = [mt.attack_texts(t % 11, ('tabby, tabby cat', 0.87), ('hamster', 0.64), ('hamster', 0.51), (4.56, 7.89, 8.12)) for t in range(n)]
    return list(mt.attack_montages(scene, prj, infer, real, (240, 240), texts).split(PER_FOLDER))


def to_host_u8(x):
    a = x.detach().cpu().numpy()
    return (np.uint8(a * 255) if a.dtype == np.float32 else a).transpose(0, 2, 3, 1)


def new_route(batches, root):
    for k, x in enumerate(batches):
        io.save_imgs(x, join(root, str(k)))


def parent_route(batches, root):
    for k, x in enumerate(batches):
        io.save_imgs(x.cpu(), join(root, str(k)))               # a CPU tensor: the Pillow path


def pillow_pool_route(batches, root, pool):
    def write(arg):
        im, path = arg
        Image.fromarray(np.ascontiguousarray(im)).save(path, compress_level=1)
    for k, x in enumerate(batches):
        os.makedirs(join(root, str(k)), exist_ok=True)
        host = to_host_u8(x)
        list(pool.map(write, [(host[i], join(root, str(k), 'img_{:04d}.png'.format(i + 1))) for i in range(len(host))]))


def new_route_split(batches, root):
    """The steps of png.encode_png + the file writes, a synchronise after each: seconds per step, summed over the batches."""
    t = dict(filter_launch_s=0.0, copy_hist_s=0.0, host_tables_s=0.0, pack_launch_s=0.0, copy_streams_s=0.0, crc_write_s=0.0)

    def lap(key, t0):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t[key] += t1 - t0
        return t1
    for k, x in enumerate(batches):
        os.makedirs(join(root, str(k)), exist_ok=True)
        m, _, h, w = x.shape
        row = 1 + 3 * w
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        streams, stats = png.filter_hist(x)
        t0 = lap('filter_launch_s', t0)
        stats = stats.cpu().numpy()
        t0 = lap('copy_hist_s', t0)
        hist = stats[:m * 257].reshape(m, 257)
        adler = png.adler32_from_rows(stats[m * 257:].reshape(m, h, 2), row)
        tabs = [png.deflate_tables(hist[i]) for i in range(m)]
        offsets = np.concatenate(([0], np.cumsum([(png.deflate_bits(hist[i], tb[1], tb[3]) + 7) // 8 for i, tb in enumerate(tabs)])))
        t0 = lap('host_tables_s', t0)
        out = png.pack(streams, np.stack([tb[0] for tb in tabs]), np.stack([tb[1] for tb in tabs]), [tb[2] for tb in tabs],
                       [tb[3] for tb in tabs], offsets[:-1], offsets[-1])
        t0 = lap('pack_launch_s', t0)                            # (includes the copy of the tables to the device)
        buf = out.cpu().numpy().tobytes()
        t0 = lap('copy_streams_s', t0)
        for i in range(m):
            with open(join(root, str(k), 'img_{:04d}.png'.format(i + 1)), 'wb') as fh:
                fh.write(png.wrap_png(w, h, buf[offsets[i]:offsets[i + 1]], adler[i]))
        t0 = lap('crc_write_s', t0)
    return t


def check_files(batches, root):
    nbytes = 0
    for k, x in enumerate(batches):
        want = to_host_u8(x)
        for i in range(len(want)):
            path = join(root, str(k), 'img_{:04d}.png'.format(i + 1))
            nbytes += os.path.getsize(path)
            with Image.open(path) as im:
                assert np.array_equal(np.asarray(im), want[i]), path
    return nbytes


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return dict(median_s=round(statistics.median(ts), 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4))


def measure(batches, passes, pool):
    rec = dict(images=sum(len(b) for b in batches), shapes=sorted({tuple(b.shape[1:]) for b in batches}), dtype=str(batches[0].dtype),
               raw_mb=round(sum(b.numel() for b in batches) / 1e6, 1))
    times = dict(new=[], parent=[], pillow_level1_pool16=[])
    with tempfile.TemporaryDirectory() as root:
        new_route(batches[:1], join(root, 'warm'))               # loads the library, the kernels and Pillow
        parent_route(batches[:1], join(root, 'warm'))
        for p in range(passes):
            times['new'].append(timed(new_route, batches, join(root, f'new{p}')))
            times['parent'].append(timed(parent_route, batches, join(root, f'parent{p}')))
            times['pillow_level1_pool16'].append(timed(pillow_pool_route, batches, join(root, f'pool{p}'), pool))
        rec['new_file_mb'] = round(check_files(batches, join(root, 'new0')) / 1e6, 2)
        rec['parent_file_mb'] = round(check_files(batches, join(root, 'parent0')) / 1e6, 2)
        rec['new_split'] = {k: round(v, 4) for k, v in new_route_split(batches, join(root, 'split')).items()}
    for k, ts in times.items():
        rec[k] = stats(ts)
    rec['parent_over_new'] = round(rec['parent']['median_s'] / rec['new']['median_s'], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=join(ROOT, 'profiles', 'png_time.jsonl'))
    ap.add_argument('--passes', type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_png needs a GPU'
    dev = torch.device('cuda', 0)
    with ThreadPoolExecutor(16) as pool:
        rec = dict(tool='time_png', passes=a.passes, per_call=PER_FOLDER,
                   floats=measure(float_batches(dev), a.passes, pool), montages=measure(montage_batches(dev), a.passes, pool),
                   device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as fh:
        fh.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
