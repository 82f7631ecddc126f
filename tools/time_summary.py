"""Wall time of summarize_single_attacker (spaa_amd/attack_summary.py) on a synthetic SPAA setup at the reference's geometry,
against the same summary computed the way the reference's loop does it (projector_based_attack.py:448-541: per configuration, the
classifier on the scene, the inferred and the captured images, and one metrics.calc_img_dists per group).

    python tools/time_summary.py [--out profiles/summary_time.jsonl] [--repeat 2]

Setup: prj 256 x 256, camera 256 x 256, classifier crop 240 x 240, 3 stealth losses x 4 d_thr x 3 classifiers = 36 configurations of
11 images (10 targeted + 1 untargeted), captured images = inferred images + noise.  Classifiers: synthetic weights at the full input
sizes (Inception-v3 299, ResNet-18 224, VGG-16 224 with its 4096-wide head).  Both routes run once untimed first (engines, plans);
then each is timed `--repeat` times, the best kept.  Both include reading the PNGs.  Appends one JSON line to --out and prints it.
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time
from os.path import join

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spaa_amd import io, metrics as M, synthetic as syn  # noqa: E402
from spaa_amd import projector_based_attack as A  # noqa: E402
from spaa_amd.classifier import Classifier  # noqa: E402

LOSSES, D_THR, CLFS = ['caml2', 'camdE', 'camdE_caml2'], [5, 7, 9, 11], ['inception_v3', 'resnet18', 'vgg16']
TEN = [1, 7, 21, 207, 340, 745, 779, 846, 947, 950]


def _cc(x, size):
    i, j = M.center_crop_origin(x.shape[-2], x.shape[-1], size)
    return x[..., i:i + size[0], j:j + size[1]]


def make_setup(root, sz=(256, 256)):
    setup_path = join(root, 'setups', 'synth')
    io.save_setup_info(setup_path, dict(classifier_crop_sz=(240, 240), prj_brightness=0.5, prj_im_sz=sz, cam_im_sz=sz))
    io.save_imgs(syn.scenes(1, 2, sz), join(setup_path, 'cam/raw/ref'))
    for fn, labels in (('imagenet1000_clsidx_to_labels.txt', {k: f'class{k}' for k in range(1000)}),
                       ('imagenet10_clsidx_to_labels.txt', {k: f'name{k}' for k in TEN})):
        with open(join(root, fn), 'w') as fh:
            fh.write('{' + ',\n'.join(f"{k}: '{v}'" for k, v in labels.items()) + '}')
    cfg_str, model_cfg_str = A.to_attacker_cfg_str('SPAA')
    g = torch.Generator().manual_seed(0)
    for k, (loss, d_thr, cname) in enumerate(itertools.product(LOSSES, D_THR, CLFS)):
        folder = join(cfg_str, loss, str(d_thr), cname)
        scene = syn.scenes(1, 2, sz)[1:]
        prj = (0.5 + 0.2 * torch.randn(11, 3, *sz, generator=g)).clamp(0, 1)
        infer = (scene + 0.05 * torch.randn(11, 3, *sz, generator=g)).clamp(0, 1)
        real = (infer + 0.03 * torch.randn(11, 3, *sz, generator=g)).clamp(0, 1)
        for kind, ims in (('prj/adv', prj), ('cam/infer/adv', infer), ('cam/raw/adv', real)):
            io.save_imgs(ims, join(setup_path, kind, folder))
    io.save_imgs(torch.rand(5, 3, *sz, generator=g), join(setup_path, 'cam/raw/test'))
    io.save_imgs(torch.rand(5, 3, *sz, generator=g), join(setup_path, 'cam/infer/test', model_cfg_str))
    return setup_path


def per_configuration(setup_path, classifiers, dev='cuda', n=10):
    """The reference's loop (projector_based_attack.py:448-541) without its montages: returns the rows' numeric part."""
    info = io.load_setup_info(setup_path)
    cp_sz = tuple(info['classifier_crop_sz'])
    cfg_str, model_cfg_str = A.to_attacker_cfg_str('SPAA')
    im_gray = info['prj_brightness'] * torch.ones(1, 3, *info['prj_im_sz']).to(dev)
    cam_scene = io.torch_imread(join(setup_path, 'cam/raw/ref/img_0002.png')).to(dev)
    valid = M.calc_img_dists(_cc(io.torch_imread_mt(join(setup_path, 'cam/infer/test', model_cfg_str)), cp_sz).to(dev),
                             _cc(io.torch_imread_mt(join(setup_path, 'cam/raw/test')), cp_sz).to(dev))
    rows = []
    for loss, d_thr, cname in itertools.product(A.SUMMARY_STEALTH_LOSSES, A.SUMMARY_D_THRESHES, A.SUMMARY_CLASSIFIERS):
        folder = join(cfg_str, loss, str(d_thr), cname)
        paths = [join(setup_path, k, folder) for k in ('prj/adv', 'cam/raw/adv', 'cam/infer/adv')]
        if not all(os.path.exists(p) and os.listdir(p) for p in paths):
            continue
        prj, real, infer = (io.torch_imread_mt(p).to(dev) for p in paths)
        clf = classifiers[cname]
        ret = {k: clf(v, cp_sz) for k, v in (('scene', cam_scene), ('infer', infer), ('real', real))}
        succ = A.attack_success(ret['infer'][2], ret['real'][2], ret['scene'][2], TEN)
        cs = _cc(cam_scene, cp_sz)
        groups = []
        for sel in (slice(0, n), slice(n, n + 1), slice(None)):
            groups += [M.calc_img_dists(prj[sel], im_gray.expand_as(prj[sel])),
                       M.calc_img_dists(_cc(infer[sel], cp_sz), cs.expand_as(_cc(infer[sel], cp_sz))),
                       M.calc_img_dists(_cc(real[sel], cp_sz), cs.expand_as(_cc(real[sel], cp_sz)))]
        rows.append([*succ, *valid, *itertools.chain.from_iterable(groups)])
    return np.array(rows, dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=join(ROOT, 'profiles', 'summary_time.jsonl'))
    ap.add_argument('--repeat', type=int, default=2)
    args = ap.parse_args()
    dev = 'cuda'
    classifiers = {'inception_v3': Classifier('inception_v3', dev, state_dict=syn.inception_v3_state_dict(4, logit_gain=5.0)),
                   'resnet18': Classifier('resnet18', dev, state_dict=syn.resnet18_state_dict(2, logit_gain=20.0)),
                   'vgg16': Classifier('vgg16', dev, state_dict=syn.vgg16_state_dict(3, logit_gain=5.0))}
    with tempfile.TemporaryDirectory() as root:
        setup_path = make_setup(root)
        routes = {'summary': lambda: A.summarize_single_attacker('SPAA', root, ['synth'], classifiers=classifiers, gpu_decode=False),
                  'summary_gpu_decode': lambda: A.summarize_single_attacker('SPAA', root, ['synth'], classifiers=classifiers,
                                                                           gpu_decode=True),
                  'per_configuration': lambda: per_configuration(setup_path, classifiers)}
        best, out = {}, {}
        for name, fn in routes.items():
            for rep in range(args.repeat + 1):   # the first run builds the engines
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    best[name] = min(best.get(name, dt), dt)
            out[name] = r
    table = out['summary']
    got = table[A.SUMMARY_COLUMNS[5:]].to_numpy(dtype=np.float64)
    want = out['per_configuration']
    line = dict(tool='time_summary', configurations=int(len(table)), images_per_configuration=11, prj_sz=[256, 256], crop=[240, 240],
                summary_s=round(best['summary'], 3), summary_gpu_decode_s=round(best['summary_gpu_decode'], 3),
                gpu_decode_equal=bool(out['summary_gpu_decode'].equals(table)), per_configuration_s=round(best['per_configuration'], 3),
                ratio=round(best['per_configuration'] / best['summary'], 2),
                success_equal=bool(np.array_equal(got[:, :6], want[:, :6])),
                metrics_max_rel=float(np.max(np.abs(got[:, 6:] / want[:, 6:] - 1))),
                device=torch.cuda.get_device_name(0))
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
