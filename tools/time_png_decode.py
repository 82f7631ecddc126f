"""Time of reading PNG files into device tensors: io.torch_imread_mt(..., device=) (spaa_amd.png.decode_records, csrc/png_decode.hip)
against the host path it stands beside -- Pillow one file after the other, and the same Pillow reads in a pool of 16 threads, which
is the fair host baseline.  A record, not a gate: one JSON line appended to profiles/png_decode_time.jsonl.

    python tools/time_png_decode.py [--out profiles/png_decode_time.jsonl] [--passes 3] [--camera 1400]

Workloads, each one folder read by one call:
  camera    `--camera` files of 240 x 320 RGB written by Pillow at its default level (synthetic.scenes plus +-8 grey levels of noise)
  sweep     528 files as this project's encoder writes them, 264 of 256 x 256 and 264 of 240 x 320 (read as two folders)
  montages  132 montages of 292 x 1310 from montage.attack_montages, written by this project's encoder
Per workload: the wall time of each route over `passes` passes after one warm-up pass, the routes alternating (median, min, max);
the device route split into file read, host parse, pinned packing + host-to-device copy, the inflate kernel, the unfilter kernel and
the copy of status words and Adler sums (the four device steps from events on the stream); and the inflate kernel on ONE image alone,
the rate of a single wave.  Every image of the device route is compared once with the host route.
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

import torch  # noqa: E402

from spaa_amd import io, montage as mt, png, synthetic as syn  # noqa: E402


def noisy(seed, n, sz):
    g = torch.Generator().manual_seed(seed)
    x = syn.scenes(seed, n, sz)
    return (x + torch.randint(-8, 9, x.shape, generator=g).float() / 255).clamp(0, 1)


def write_workloads(root, n_camera, dev):
    """-> {name: [folders]}"""
    io.save_imgs(noisy(10, n_camera, (240, 320)), join(root, 'camera'))                    # host tensors: Pillow writes them
    io.save_imgs(noisy(11, 264, (256, 256)).to(dev), join(root, 'sweep_prj'))              # device tensors: this project's encoder
    io.save_imgs(noisy(12, 264, (240, 320)).to(dev), join(root, 'sweep_cam'))
    n = 132
    scene = syn.scenes(20, 1, (240, 320))[0].to(dev)
    texts = [mt.attack_texts(t % 11, ('tabby, tabby cat', 0.87), ('hamster', 0.64), ('hamster', 0.51), (4.56, 7.89, 8.12)) for t in range(n)]
    m = mt.attack_montages(scene, syn.scenes(21, n, (256, 256)).to(dev), noisy(22, n, (240, 320)).to(dev),
                           noisy(23, n, (240, 320)).to(dev), (240, 240), texts)
    io.save_imgs(m, join(root, 'montages'))
    return dict(camera=[join(root, 'camera')], sweep=[join(root, 'sweep_prj'), join(root, 'sweep_cam')], montages=[join(root, 'montages')])


def host_route(folders):
    return [io.torch_imread_mt(d) for d in folders]


def pool_route(folders, pool):
    """io.torch_imread_mt's host expressions with the Pillow reads spread over the pool."""
    out = []
    for d in folders:
        paths = [join(d, n) for n in sorted(os.listdir(d))]
        ims = list(pool.map(lambda p: torch.from_numpy(io._imread_rgb(p).transpose(2, 0, 1).copy()), paths))
        out.append(torch.stack([im.float() for im in ims]).div(255))
    return out


def device_route(folders, dev):
    return [io.torch_imread_mt(d, device=dev) for d in folders]


def device_split(folders, dev):
    """Seconds per step of the device route, summed over the folders."""
    t = dict(file_read_s=0.0, host_parse_s=0.0, pack_and_h2d_s=0.0, inflate_kernel_s=0.0, unfilter_kernel_s=0.0, status_copy_s=0.0,
             float_stack_s=0.0)
    for d in folders:
        paths = [join(d, n) for n in sorted(os.listdir(d))]
        t0 = time.perf_counter()
        blobs = [io._read_bytes(p) for p in paths]
        t1 = time.perf_counter()
        records = [png.parse_png(b) for b in blobs]
        t2 = time.perf_counter()
        ev = {}
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        images, status = png.decode_records(records, dev, timings=ev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        assert not status.any()
        io._div255(torch.stack([im.float() for im in images]))
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        dev_s = (ev['h2d'] + ev['inflate'] + ev['unfilter'] + ev['d2h']) / 1e3
        t['file_read_s'] += t1 - t0
        t['host_parse_s'] += t2 - t1
        t['pack_and_h2d_s'] += (t4 - t3) - dev_s + ev['h2d'] / 1e3          # host packing into the pinned block + the copy
        t['inflate_kernel_s'] += ev['inflate'] / 1e3
        t['unfilter_kernel_s'] += ev['unfilter'] / 1e3
        t['status_copy_s'] += ev['d2h'] / 1e3
        t['float_stack_s'] += t5 - t4
    return t


def single_image(folder, dev, repeat=5):
    """The two kernels on the folder's first image alone: the rate of ONE wave (median of `repeat` after a warm-up)."""
    path = join(folder, sorted(os.listdir(folder))[0])
    rec = png.parse_png(io._read_bytes(path))
    runs = []
    for _ in range(repeat + 1):
        ev = {}
        png.decode_records([rec], dev, timings=ev)
        runs.append(ev)
    runs = runs[1:]
    stream = rec.height * (1 + rec.width * rec.channels)
    inflate_ms = statistics.median(r['inflate'] for r in runs)
    return dict(shape=[rec.height, rec.width, rec.channels], deflate_bytes=len(rec.deflate), scanline_bytes=stream,
                inflate_ms=round(inflate_ms, 4), unfilter_ms=round(statistics.median(r['unfilter'] for r in runs), 4),
                inflate_mb_per_s_out=round(stream / 1e3 / inflate_ms, 2))


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts):
    return dict(median_s=round(statistics.median(ts), 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4))


def measure(folders, passes, pool, dev):
    files = [join(d, n) for d in folders for n in os.listdir(d)]
    rec = dict(images=len(files), file_mb=round(sum(os.path.getsize(f) for f in files) / 1e6, 2))
    _, want = timed(host_route, folders)
    _, got = timed(device_route, folders, dev)                     # warm-up of both, and the comparison
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)), 'the device route differs from the host route'
    del got
    times = dict(device=[], pillow_sequential=[], pillow_pool16=[])
    for _ in range(passes):
        times['device'].append(timed(device_route, folders, dev)[0])
        times['pillow_sequential'].append(timed(host_route, folders)[0])
        times['pillow_pool16'].append(timed(pool_route, folders, pool)[0])
    for k, ts in times.items():
        rec[k] = stats(ts)
    rec['device_split'] = {k: round(v, 5) for k, v in device_split(folders, dev).items()}
    rec['one_image_alone'] = single_image(folders[-1], dev)
    rec['sequential_over_device'] = round(rec['pillow_sequential']['median_s'] / rec['device']['median_s'], 2)
    rec['pool16_over_device'] = round(rec['pillow_pool16']['median_s'] / rec['device']['median_s'], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=join(ROOT, 'profiles', 'png_decode_time.jsonl'))
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--camera', type=int, default=1400)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_png_decode needs a GPU'
    dev = torch.device('cuda', 0)
    rec = dict(tool='time_png_decode', passes=a.passes)
    with tempfile.TemporaryDirectory() as root, ThreadPoolExecutor(16) as pool:
        for name, folders in write_workloads(root, a.camera, dev).items():
            rec[name] = measure(folders, a.passes, pool, dev)
            print(name, json.dumps(rec[name]), flush=True)
    rec['device'] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as fh:
        fh.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
