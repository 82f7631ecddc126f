"""The summary step of the reference's experiments (projector_based_attack.py:362-614): the result montage of one attack, and the
success rates and image metrics of every attack configuration of a setup.  spaa_amd.projector_based_attack re-exports the public
names; SUMMARY_CHUNK and MONTAGE_CHUNK are read here.  pandas is imported by the functions that build tables, not by the module."""
import itertools
import os
from os.path import join

import numpy as np
import torch

from . import _lib, io, montage
from . import metrics as M
from .img_proc import center_crop
from .attack_driver import ATTACKERS, AttackSetup, target_classes, to_attacker_cfg_str

SUMMARY_STEALTH_LOSSES = ['caml2', 'camdE', 'camdE_caml2', '-']
SUMMARY_D_THRESHES = [5, 7, 9, 11, '-']
SUMMARY_CLASSIFIERS = ['inception_v3', 'resnet18', 'vgg16']
SUMMARY_CHUNK = 64   # images per classifier launch in the summary (the last chunk is padded: one engine geometry per image size)
MONTAGE_CHUNK = 264   # montages per attack_montages call in the summary (24 configurations; bounds the output buffer, ~300 MB at 256^2 tiles)
_PHASES = ['Valid', 'prj', 'infer', 'real']
_METRICS = ['PSNR', 'RMSE', 'SSIM', 'L2', 'Linf', 'dE']
SUMMARY_COLUMNS = (['Setup', 'Attacker', 'Stealth_loss', 'd_thr', 'Classifier', 'T.top-1_infer', 'T.top-5_infer', 'T.top-1_real',
                    'T.top-5_real', 'U.top-1_infer', 'U.top-1_real'] + [_PHASES[0] + '_' + m for m in _METRICS] +
                   [f'{g}.{x}_{m}' for g in ('T', 'U', 'All') for x in _PHASES[1:] for m in _METRICS])
N_TARGETED = 10   # a configuration is 10 targeted attacks and 1 untargeted attack


def attack_results(ret, t, imgnet_labels, im_gray, prj_adv, cam_scene, cam_infer, cam_real, prj_im_sz, cp_sz):
    """projector_based_attack.py:362-414: the result montage of attack `t` as a float [3,Hm,Wm] image (spaa_amd.montage's bytes
    divided by 255).  ret['scene' / 'infer' / 'real'] = the classifier tuples (raw, p_sorted, idx_sorted); the L2 values come from
    metrics.l2_norm.  The tiles have prj_adv's own size (Hp, Wp): the reference passes prj_im_sz, which is (w, h), as (h, w), and so
    works for square projectors only; `prj_im_sz` is not used.  GPU only."""
    for name, x in (('prj_adv', prj_adv), ('cam_scene', cam_scene), ('cam_infer', cam_infer), ('cam_real', cam_real)):
        if not x.is_cuda:
            raise RuntimeError(f'attack_results builds the montage on the GPU only (no CPU fallback): {name} is on {x.device}')
    scene = cam_scene.reshape(-1, *cam_scene.shape[-3:])[0]
    gray = im_gray.reshape(-1, *im_gray.shape[-3:])[0]
    scene_cp = center_crop(scene, cp_sz)
    l2 = (M.l2_norm(prj_adv[t], gray.to(prj_adv.device).expand_as(prj_adv[t])), M.l2_norm(center_crop(cam_infer[t], cp_sz), scene_cp),
          M.l2_norm(center_crop(cam_real[t], cp_sz), scene_cp))

    def top1(key, row):
        return imgnet_labels[int(ret[key][2][row, 0])], float(ret[key][1][row, 0])
    texts = montage.attack_texts(t, top1('scene', 0), top1('infer', t), top1('real', t), l2)
    im = montage.attack_montages(scene, prj_adv[t:t + 1], cam_infer[t:t + 1], cam_real[t:t + 1], cp_sz, [texts])[0]
    return im.float() / torch.full((), 255.0, device=im.device)     # (a true division: `/ 255` multiplies by 1 / 255 on the GPU)


def attack_success(idx_infer, idx_real, idx_scene, target_idx):
    """projector_based_attack.py:493-506: (T.top-1_infer, T.top-5_infer, T.top-1_real, T.top-5_real, U.top-1_infer, U.top-1_real)
    from class indices sorted by descending probability ([n + 1, >= 5]: rows 0..n-1 the targeted attacks on `target_idx`, row n
    the untargeted one) and the scene's (`idx_scene[0, 0]` is its top-1).  Targeted rates are fractions, untargeted flags 0/1."""
    n = len(target_idx)
    idx_infer, idx_real, idx_scene = np.asarray(idx_infer), np.asarray(idx_real), np.asarray(idx_scene)
    t1_infer = np.count_nonzero(idx_infer[:n, 0] == target_idx) / n
    t5_infer = np.count_nonzero([target_idx[i] in idx_infer[i, :5] for i in range(n)]) / n
    t1_real = np.count_nonzero(idx_real[:n, 0] == target_idx) / n
    t5_real = np.count_nonzero([target_idx[i] in idx_real[i, :5] for i in range(n)]) / n
    true_idx = idx_scene[0, 0]
    return (t1_infer, t5_infer, t1_real, t5_real, int(np.count_nonzero(idx_infer[n, 0] != true_idx)),
            int(np.count_nonzero(idx_real[n, 0] != true_idx)))


def attack_transfer(ims, classifiers, target_idx, targeted, crop_sz):
    """Which classifier each adversarial image fools: bool [N][K] for the images `ims` [N,3,H,W], the K `classifiers` and one class id
    per image in `target_idx`; `targeted` (one flag, or one per image): top-1 == target, else top-1 != target (the image's true class).
    The evaluation hook of an ensemble attack: column k is member k.  Top-1 through _sorted_classes, as the summary's rates."""
    n = ims.shape[0]
    tgt = np.asarray([int(t) for t in target_idx])
    tg = np.full(n, bool(targeted)) if np.ndim(targeted) == 0 else np.asarray([bool(t) for t in targeted])
    if tgt.shape != (n,) or tg.shape != (n,):
        raise ValueError(f'attack_transfer: {n} images, {tgt.size} targets, {tg.size} targeted flags')
    out = np.zeros((n, len(classifiers)), dtype=bool)
    for k, clf in enumerate(classifiers):
        top1 = _sorted_classes(clf, [ims], crop_sz)[0][:, 0]
        out[:, k] = np.where(tg, top1 == tgt, top1 != tgt)
    return out


SURVIVAL_CHUNK = 64   # images per launch of capture_survival
SURVIVAL_ROUND = 4    # jittered captures per launch of capture_survival (SPAA_JITTER_MAX)


def capture_survival(ims, classifier, target_idx, targeted, crop_sz, jitter, *, draws=32, seed=0):
    """The fraction of `draws` randomly jittered captures of each camera image that still succeed: float [N] for the images `ims`
    [N,3,H,W], one class id per image in `target_idx` and `targeted` (one flag, or one per image; success as in attack_transfer).
    The evaluation hook of a jitter attack.  The captures are those of `jitter` (a CaptureJitter: its ranges and `quantize`; its
    `draws` and `seed` belong to the attack) with the generator seeded by `seed`, none of them the clean one: spaa_jitter_draw +
    spaa_jitter_fwd in rounds of four captures (round r is the generator's iteration r), on chunks of at most 64 images (an image's
    captures depend on its place in its chunk)."""
    from .models import to_nhwc4
    from .projector_based_attack import CaptureJitter
    if not isinstance(jitter, CaptureJitter):
        raise TypeError(f'capture_survival: jitter must be a spaa_amd.CaptureJitter, got {type(jitter).__name__}')
    n = ims.shape[0]
    tgt = torch.as_tensor([int(t) for t in target_idx])
    tg = torch.full((n,), bool(targeted)) if np.ndim(targeted) == 0 else torch.as_tensor([bool(t) for t in targeted])
    if tuple(tgt.shape) != (n,) or tuple(tg.shape) != (n,) or int(draws) < 1:
        raise ValueError(f'capture_survival: {n} images, {tgt.numel()} targets, {tg.numel()} targeted flags, {draws} draws')
    dev = classifier.device
    if dev.type != 'cuda':
        raise RuntimeError(f'capture_survival runs on the GPU only (no CPU fallback); the classifier is on {dev}')
    jt = CaptureJitter(jitter.gain, jitter.offset, jitter.shift, jitter.noise, jitter.quantize, SURVIVAL_ROUND, seed)
    J, (H, W) = SURVIVAL_ROUND, ims.shape[-2:]
    b = min(n, SURVIVAL_CHUNK)
    hits = torch.zeros(n)
    with _lib.on_device(dev):
        eng = classifier.engine(b, (H, W), tuple(crop_sz))
        jit = torch.zeros(b, J, 8, device=dev)
        key = torch.zeros(b, J, dtype=torch.int32, device=dev)
        outs = [torch.zeros(b, H, W, 4, device=dev) for _ in range(J)]
        gates = [torch.zeros(b, H * W, dtype=torch.uint8, device=dev) for _ in range(J)]
        for s in range(0, n, b):
            part = ims[s:s + b].to(dev).float()
            m = part.shape[0]
            if m < b:   # (one engine geometry: the last chunk is padded)
                part = torch.cat((part, part.new_zeros(b - m, *part.shape[1:])))
            y4 = to_nhwc4(part.contiguous())
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            t_dev, tg_dev = tgt[s:s + m].to(dev), tg[s:s + m].to(dev)
            count = torch.zeros(m, device=dev)
            for done in range(0, int(draws), J):
                jt.draw(counter, jit, key, b, J, clean0=False)
                _lib.call('spaa_jitter_fwd', _lib.ptr(y4), _lib.ptr(jit), _lib.ptr(key), J, int(bool(jt.quantize)),
                          _lib.ptr_array(outs), _lib.ptr_array(gates), b, H, W)
                for j in range(min(J, int(draws) - done)):
                    top1 = eng.forward(outs[j], need_grad=False)[:m].argmax(dim=1)
                    count += torch.where(tg_dev, top1 == t_dev, top1 != t_dev).float()
            hits[s:s + m] = count.cpu()
    return (hits / int(draws)).numpy()


def pose_survival(ims, classifier, target_idx, targeted, crop_sz, pose, *, draws=32, seed=0, jitter=None):
    """The fraction of `draws` randomly warped captures of each camera image that still succeed: float [N], the arguments and the
    success rule as in capture_survival.  The evaluation hook of a pose attack.  The captures are those of `pose` (a PoseJitter: its
    ranges; its `draws` and `seed` belong to the attack) with the generator seeded by `seed`, none of them the unwarped one:
    spaa_pose_draw + spaa_pose_fwd in rounds of four captures (round r is the generator's iteration r), on chunks of at most 64
    images (an image's captures depend on its place in its chunk).  With `jitter` (a CaptureJitter: its ranges and `quantize`) every
    warped capture is then jittered, none of them cleanly, by the jitter generator of the same `seed`."""
    from .models import to_nhwc4
    from .projector_based_attack import CaptureJitter, PoseJitter
    if not isinstance(pose, PoseJitter):
        raise TypeError(f'pose_survival: pose must be a spaa_amd.PoseJitter, got {type(pose).__name__}')
    if jitter is not None and not isinstance(jitter, CaptureJitter):
        raise TypeError(f'pose_survival: jitter must be a spaa_amd.CaptureJitter or None, got {type(jitter).__name__}')
    n = ims.shape[0]
    tgt = torch.as_tensor([int(t) for t in target_idx])
    tg = torch.full((n,), bool(targeted)) if np.ndim(targeted) == 0 else torch.as_tensor([bool(t) for t in targeted])
    if tuple(tgt.shape) != (n,) or tuple(tg.shape) != (n,) or int(draws) < 1:
        raise ValueError(f'pose_survival: {n} images, {tgt.numel()} targets, {tg.numel()} targeted flags, {draws} draws')
    dev = classifier.device
    if dev.type != 'cuda':
        raise RuntimeError(f'pose_survival runs on the GPU only (no CPU fallback); the classifier is on {dev}')
    ps = PoseJitter(pose.rotate, pose.zoom, pose.shift, pose.tilt, SURVIVAL_ROUND, seed)
    jt = None if jitter is None else CaptureJitter(jitter.gain, jitter.offset, jitter.shift, jitter.noise, jitter.quantize,
                                                   SURVIVAL_ROUND, seed)
    J, (H, W) = SURVIVAL_ROUND, ims.shape[-2:]
    b = min(n, SURVIVAL_CHUNK)
    hits = torch.zeros(n)
    with _lib.on_device(dev):
        eng = classifier.engine(b, (H, W), tuple(crop_sz))
        table = torch.zeros(b, J, 8, device=dev)
        outs = [torch.zeros(b, H, W, 4, device=dev) for _ in range(J)]
        if jt is not None:
            jit = torch.zeros(b, J, 8, device=dev)
            key = torch.zeros(b, J, dtype=torch.int32, device=dev)
            jouts = [torch.zeros(b, H, W, 4, device=dev) for _ in range(J)]
            gates = [torch.zeros(b, H * W, dtype=torch.uint8, device=dev) for _ in range(J)]
        for s in range(0, n, b):
            part = ims[s:s + b].to(dev).float()
            m = part.shape[0]
            if m < b:   # (one engine geometry: the last chunk is padded)
                part = torch.cat((part, part.new_zeros(b - m, *part.shape[1:])))
            y4 = to_nhwc4(part.contiguous())
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            jcounter = torch.zeros(1, dtype=torch.int32, device=dev)
            t_dev, tg_dev = tgt[s:s + m].to(dev), tg[s:s + m].to(dev)
            count = torch.zeros(m, device=dev)
            for done in range(0, int(draws), J):
                ps.draw(counter, table, b, J, H, W, clean0=False)
                _lib.call('spaa_pose_fwd', _lib.ptr(y4), _lib.ptr(table), J, _lib.ptr_array(outs), b, H, W)
                seen = outs
                if jt is not None:
                    jt.draw(jcounter, jit, key, b, J, clean0=False)
                    _lib.call('spaa_jitter_fwd_each', _lib.ptr_array(outs), _lib.ptr(jit), _lib.ptr(key), J, int(bool(jt.quantize)),
                              _lib.ptr_array(jouts), _lib.ptr_array(gates), b, H, W)
                    seen = jouts
                for j in range(min(J, int(draws) - done)):
                    top1 = eng.forward(seen[j], need_grad=False)[:m].argmax(dim=1)
                    count += torch.where(tg_dev, top1 == t_dev, top1 != t_dev).float()
            hits[s:s + m] = count.cpu()
    return (hits / int(draws)).numpy()


def jpeg_survival(ims, classifier, target_idx, targeted, crop_sz, *, qualities=(95, 90, 75, 50, 30), subsampling='4:2:0'):
    """Which camera images still succeed behind a JPEG re-encode: bool [len(qualities), N] for the images `ims` [N,3,H,W], one class id
    per image in `target_idx` and `targeted` (one flag, or one per image), by the success rule of capture_survival.  The evaluation
    hook of a JPEG attack, and the answer to a classifier that sits behind the input-transformation defence.  Row q is the round trip
    of every image at qualities[q] (spaa_jpeg_fwd through jpeg_roundtrip).  Deterministic: nothing is drawn."""
    from .jpeg import jpeg_roundtrip
    n = ims.shape[0]
    tgt = np.asarray([int(t) for t in target_idx])
    tg = np.full(n, bool(targeted)) if np.ndim(targeted) == 0 else np.asarray([bool(t) for t in targeted])
    if tgt.shape != (n,) or tg.shape != (n,) or len(qualities) < 1:
        raise ValueError(f'jpeg_survival: {n} images, {tgt.size} targets, {tg.size} targeted flags, {len(qualities)} qualities')
    dev = classifier.device
    if dev.type != 'cuda':
        raise RuntimeError(f'jpeg_survival runs on the GPU only (no CPU fallback); the classifier is on {dev}')
    out = np.zeros((len(qualities), n), dtype=bool)
    with _lib.on_device(dev):
        y = ims.to(dev).float()
        for q, quality in enumerate(qualities):
            top1 = _sorted_classes(classifier, [jpeg_roundtrip(y, int(quality), subsampling)], crop_sz)[0][:, 0]
            out[q] = np.where(tg, top1 == tgt, top1 != tgt)
    return out


def blur_survival(ims, classifier, target_idx, targeted, crop_sz, *, sigmas=(0.5, 1.0, 1.5, 2.0, 2.5)):
    """Which camera images still succeed through a defocused lens: bool [len(sigmas), N] for the images `ims` [N,3,H,W], one class id
    per image in `target_idx` and `targeted` (one flag, or one per image), by the success rule of capture_survival.  The evaluation
    hook of a blur attack, and the answer to a classifier that sits behind Gaussian smoothing of its input.  Row s is every image
    through the Gaussian of sigmas[s] camera pixels (spaa_blur_fwd through gaussian_blur).  Deterministic: nothing is
    drawn."""
    from .blur import gaussian_blur
    n = ims.shape[0]
    tgt = np.asarray([int(t) for t in target_idx])
    tg = np.full(n, bool(targeted)) if np.ndim(targeted) == 0 else np.asarray([bool(t) for t in targeted])
    if tgt.shape != (n,) or tg.shape != (n,) or len(sigmas) < 1:
        raise ValueError(f'blur_survival: {n} images, {tgt.size} targets, {tg.size} targeted flags, {len(sigmas)} sigmas')
    dev = classifier.device
    if dev.type != 'cuda':
        raise RuntimeError(f'blur_survival runs on the GPU only (no CPU fallback); the classifier is on {dev}')
    out = np.zeros((len(sigmas), n), dtype=bool)
    with _lib.on_device(dev):
        y = ims.to(dev).float()
        for s, sigma in enumerate(sigmas):
            top1 = _sorted_classes(classifier, [gaussian_blur(y, float(sigma))], crop_sz)[0][:, 0]
            out[s] = np.where(tg, top1 == tgt, top1 != tgt)
    return out


def transfer_success(cam, classifier, target_idx, targeted, crop_sz, p_thresh=0.9):
    """Which camera images `cam` [B,3,H,W] fool `classifier`, by the success rule of the attack's own decision (spaa_decide): bool [B];
    one class id per image in `target_idx` and `targeted` (one flag, or one per image): top-1 == target with p1 > `p_thresh`, else
    top-1 != target (the image's true class).  The evaluation hook of a transferable attack (Transfer): `classifier` is one that took
    no part in it.  Top-1 and p1 through _sorted_classes, as the summary's rates."""
    n = cam.shape[0]
    tgt = np.asarray([int(t) for t in target_idx])
    tg = np.full(n, bool(targeted)) if np.ndim(targeted) == 0 else np.asarray([bool(t) for t in targeted])
    if tgt.shape != (n,) or tg.shape != (n,):
        raise ValueError(f'transfer_success: {n} images, {tgt.size} targets, {tg.size} targeted flags')
    p1 = [None]
    top1 = _sorted_classes(classifier, [cam], crop_sz, top1=p1)[0][:, 0]
    return np.where(tg, (top1 == tgt) & (p1[0] > np.float32(p_thresh)), top1 != tgt)


def universal_success(pcnet, classifier, prj_adv, cam_scenes, target_idx, targeted, crop_sz, p_thresh=0.9):
    """A universal projection on scenes it may never have seen: `prj_adv` ([3,Hp,Wp] / [1,3,Hp,Wp]: one projector image for all, or
    [M,3,Hp,Wp]: one per scene) is projected onto the scenes `cam_scenes` [M,3,H,W] through `pcnet`, and `classifier` looks at the M
    inferred captures.  Returns (success bool [M] by transfer_success's rule, cam_infer [M,3,H,W]); one class id per scene in
    `target_idx` (its true class if untargeted) and `targeted` (one flag, or one per scene).  The evaluation hook of a universal attack
    (Universal): the mean of the first return value over scenes held out from the attack is its fooling rate.  GPU only."""
    scenes = cam_scenes.detach().float()
    if scenes.ndim != 4 or scenes.shape[1] != 3:
        raise ValueError(f'universal_success: cam_scenes must be [M,3,H,W], got {tuple(cam_scenes.shape)}')
    m = scenes.shape[0]
    prj = prj_adv.detach().float()
    while prj.ndim < 4:
        prj = prj[None]
    if prj.shape[0] == 1:
        prj = prj.expand(m, -1, -1, -1)
    if prj.shape[0] != m:
        raise ValueError(f'universal_success: {prj.shape[0]} projector images for {m} scenes (one for all, or one per scene)')
    dev = next(pcnet.parameters()).device
    with torch.no_grad(), _lib.on_device(dev):
        cam = pcnet(torch.clamp(prj.to(dev), 0, 1).contiguous(), scenes.to(dev).contiguous()).detach()
        return transfer_success(cam, classifier, target_idx, targeted, crop_sz, p_thresh), cam


def write_stats(table, path):
    """The reference's table files: tab-separated, 4 decimals (stats.txt, stats_all.txt)."""
    table.to_csv(path, index=False, float_format='%.4f', sep='\t')


def _sorted_classes(classifier, ims, crop_sz, chunk=None, top1=None):
    """Class indices sorted by descending softmax probability (classifier.py:64-72) of every image of `ims` (a list of [b,3,H,W]
    tensors): images of one size go through the classifier in equal chunks of at most SUMMARY_CHUNK, the last one padded with
    zeros (one engine geometry per size).  `top1`: a list of len(ims) slots that receives each image's largest probability
    (float32 arrays, from the same softmax)."""
    chunk = chunk or SUMMARY_CHUNK
    out = [None] * len(ims)
    by_shape = {}
    for k, t in enumerate(ims):
        by_shape.setdefault(tuple(t.shape[1:]), []).append(k)
    for shape, ks in by_shape.items():
        stack = torch.cat([ims[k] for k in ks])
        b = -(-stack.shape[0] // -(-stack.shape[0] // chunk))   # (the fewest chunks of at most `chunk`, padding < their number)
        probs = []
        for s in range(0, stack.shape[0], b):
            part = stack[s:s + b]
            m = part.shape[0]
            if m < b:
                part = torch.cat((part, part.new_zeros(b - m, *shape)))
            with torch.no_grad():
                raw = classifier(part, crop_sz)[0]
                probs.append(torch.softmax(raw.detach(), dim=1)[:m].cpu())
        p_sorted, idx = torch.cat(probs).sort(descending=True)
        p_sorted, idx = p_sorted.numpy(), idx.numpy()
        a = 0
        for k in ks:
            out[k] = idx[a:a + ims[k].shape[0]]
            if top1 is not None:
                top1[k] = p_sorted[a:a + ims[k].shape[0], 0]
            a += ims[k].shape[0]
    return out


def _nonempty(d):
    return os.path.exists(d) and len(os.listdir(d)) > 0


class _PairList:
    """The image pairs of one metrics.img_stats launch: `xs` / `ys` the flattened image stacks of the two sides (ys[0] is the
    scene), `pairs` the metrics.Pair records, `spans[key]` the indices in `pairs` of the stack added as `key`."""

    def __init__(self, scene):
        self.xs, self.ys, self.pairs, self.spans = [], [scene.reshape(-1)], [], {}
        self.xoff, self.yoff = 0, scene.numel()

    def add(self, key, x, *, y=None, **kw):
        """One pair per image of the stack `x` by metrics.stack_pairs(**kw), or against the y stack `y` (one image each)."""
        if y is not None:
            kw.update(y_hw=y.shape[-2:], y_off=self.yoff)
            self.ys.append(y.reshape(-1))
            self.yoff += y.numel()
        ps = M.stack_pairs(x.shape[0], x.shape[-2:], x_off=self.xoff, **kw)
        self.xs.append(x.reshape(-1))
        self.xoff += x.numel()
        self.spans[key] = list(range(len(self.pairs), len(self.pairs) + len(ps)))
        self.pairs.extend(ps)


class _SetupSummary:
    """The summary of one attacker on one setup, as six steps (`run`).  `read`: folder -> its images as one [m,3,H,W] stack on
    `device`.  The scene is kept uncropped: the pairs and the montages crop it."""

    def __init__(self, attacker_name, setup, target_idx, device, classifiers, read):
        self.attacker_name, self.setup, self.target_idx = attacker_name, setup, target_idx
        self.device, self.classifiers, self.read = device, classifiers, read
        self.attacker_cfg_str, self.model_cfg_str = to_attacker_cfg_str(attacker_name)
        self.dl_based = attacker_name in ('SPAA', 'PerC-AL+CompenNet++')
        self.cp_sz = tuple(setup.crop_sz)
        self.gray = float(setup.info['prj_brightness'])
        self.cam_scene = setup.raw_scene().to(device)

    def find_configs(self):
        """Step 1: the configurations with images on disk: (stealth_loss, d_thr, classifier_name, prj, cam_real[, cam_infer] paths)."""
        cfgs = []
        for stealth_loss, d_thr, classifier_name in itertools.product(SUMMARY_STEALTH_LOSSES, SUMMARY_D_THRESHES, SUMMARY_CLASSIFIERS):
            folder = (self.attacker_cfg_str, stealth_loss, d_thr, classifier_name)
            dirs = [self.setup.prj_adv(*folder), self.setup.cam_raw_adv(*folder)]
            if self.dl_based:
                dirs.append(self.setup.cam_infer_adv(*folder))
            missing = next((d for d in dirs if not _nonempty(d)), None)
            if missing is not None:
                print(f'No such folder/images: {missing}\n'
                      f'Maybe [{self.attacker_name}] has no [{join(stealth_loss, str(d_thr), classifier_name)}] attack cfg, or you '
                      'forget to project and capture.\n')
                continue
            cfgs.append((stealth_loss, d_thr, classifier_name, *dirs))
        no_clf = sorted({c[2] for c in cfgs if c[2] not in (self.classifiers or {})}, key=SUMMARY_CLASSIFIERS.index)
        if no_clf:
            raise ValueError(f'summarize_single_attacker: [{self.setup.name}] has attack results for {no_clf}: pass '
                             'classifiers={name: spaa_amd.Classifier} for them (weights cannot be downloaded here)')
        return cfgs

    def load_images(self, cfgs):
        """Step 2: (prj, infer, real), each one [m,3,H,W] stack per configuration; One-pixel DE infers nothing: infer = real."""
        n = N_TARGETED
        prj = [self.read(c[3]) for c in cfgs]
        real = [self.read(c[4]) for c in cfgs]
        infer = [self.read(c[5]) for c in cfgs] if self.dl_based else real
        for c, p, r, i in zip(cfgs, prj, real, infer):
            if not p.shape[0] == r.shape[0] == i.shape[0] > n:
                raise ValueError(f'{join(*map(str, c[:3]))}: expected the same number (> {n}) of prj / cam images, got '
                                 f'{p.shape[0]} / {r.shape[0]} / {i.shape[0]}')
        return prj, infer, real

    def classify(self, cfgs, infer, real):
        """Step 3: (config, 'scene' / 'infer' / 'real') -> (sorted class indices, top-1 probabilities), one call per classifier."""
        cls = {}
        for cname in SUMMARY_CLASSIFIERS:
            ks = [k for k, c in enumerate(cfgs) if c[2] == cname]
            if not ks:
                continue
            ims = [self.cam_scene[None]] + [infer[k] for k in ks] + ([real[k] for k in ks] if self.dl_based else [])
            top = [None] * len(ims)
            res = _sorted_classes(self.classifiers[cname], ims, self.cp_sz, top1=top)
            for j, k in enumerate(ks):
                jr = 1 + len(ks) + j if self.dl_based else 1 + j
                cls[k, 'scene'], cls[k, 'infer'], cls[k, 'real'] = (res[0], top[0]), (res[1 + j], top[1 + j]), (res[jr], top[jr])
        return cls

    def image_stats(self, prj, infer, real):
        """Step 4: every image pair of the setup, the validation pair included, through ONE img_stats launch; returns (pairs, sums,
        npix, the six Valid_* values)."""
        pairs = _PairList(self.cam_scene)
        for k in range(len(prj)):
            pairs.add((k, 'prj'), prj[k], rgb=(self.gray,) * 3)
            for kind, t in (('infer', infer[k]), ('real', real[k])) if self.dl_based else (('real', real[k]),):
                pairs.add((k, kind), t, y_hw=self.cam_scene.shape[-2:], crop=self.cp_sz, y_off=0, y_step=0)
            if not self.dl_based:
                pairs.spans[k, 'infer'] = pairs.spans[k, 'real']
        valid, setup = None, self.setup
        if self.attacker_name == 'One-pixel_DE':
            valid = (0,) * 6
        else:
            if self.attacker_name == 'SPAA':
                vx, vy, vcrop = join(setup.path, 'cam/infer/test', self.model_cfg_str), join(setup.path, 'cam/raw/test'), self.cp_sz
            else:
                vx, vy, vcrop = join(setup.path, 'prj/infer/test', self.model_cfg_str), join(setup.data_root, 'prj_share/test'), None
            if _nonempty(vx) and _nonempty(vy):
                a, b = self.read(vx), self.read(vy)
                if a.shape[0] != b.shape[0]:
                    raise ValueError(f'{vx} and {vy} hold {a.shape[0]} and {b.shape[0]} images')
                pairs.add('valid', a, y=b, crop=vcrop)
            else:
                print(f'No validation inferences ({vx} and {vy}): the Valid_* columns are NaN')
                valid = (float('nan'),) * 6
        sums = npix = None
        if pairs.pairs:
            with _lib.on_device(self.device):
                sums, npix = M.img_stats(torch.cat(pairs.xs), torch.cat(pairs.ys), pairs.pairs)
        if valid is None:
            valid = M.dists_from_sums(sums, npix, pairs.spans['valid'])
        return pairs, sums, npix, valid

    def form_rows(self, cfgs, cls, pairs, sums, npix, valid):
        """Step 5: one row of SUMMARY_COLUMNS per configuration."""
        n = N_TARGETED
        rows = []
        for k, (stealth_loss, d_thr, cname, *_) in enumerate(cfgs):
            groups = [M.dists_from_sums(sums, npix, pairs.spans[k, kind][sel]) for sel in (slice(0, n), slice(n, n + 1), slice(None))
                      for kind in ('prj', 'infer', 'real')]
            rows.append([self.setup.name, self.attacker_cfg_str, stealth_loss, d_thr, cname,
                         *attack_success(cls[k, 'infer'][0], cls[k, 'real'][0], cls[k, 'scene'][0], self.target_idx), *valid,
                         *itertools.chain.from_iterable(groups)])
        return rows

    def write_montages(self, cfgs, prj, infer, real, cls, pairs, sums, npix):
        """Step 6: the result montages under <setup>/ret: labels from step 3's softmax, L2 values from step 4's sums."""
        if len({tuple(t.shape[1:]) for t in prj}) != 1 or len({tuple(t.shape[1:]) for t in infer}) != 1 or \
                len({tuple(t.shape[1:]) for t in real}) != 1:
            raise ValueError(f'summarize_single_attacker: the montages of [{self.setup.name}] need images of one size per kind')
        imagenet_labels = self.setup.imagenet_labels()
        m = N_TARGETED + 1

        def label(k, kind, row):
            idx, top1 = cls[k, kind]
            return imagenet_labels[int(idx[row, 0])], float(top1[row])

        def l2(k, kind, t):
            j = pairs.spans[k, kind][t]
            return sums[j, 2] / npix[j] * 255
        texts = [montage.attack_texts(t, label(k, 'scene', 0), label(k, 'infer', t), label(k, 'real', t),
                                      (l2(k, 'prj', t), l2(k, 'infer', t), l2(k, 'real', t)))
                 for k in range(len(cfgs)) for t in range(m)]
        per = max(1, MONTAGE_CHUNK // m)           # whole configurations per call
        for a in range(0, len(cfgs), per):
            ks = range(a, min(a + per, len(cfgs)))
            with _lib.on_device(self.device):
                ims = montage.attack_montages(self.cam_scene, *(torch.cat([t[k][:m] for k in ks]) for t in (prj, infer, real)),
                                              self.cp_sz, texts[a * m:(a + len(ks)) * m])
            for j, k in enumerate(ks):
                io.save_imgs(ims[j * m:(j + 1) * m], self.setup.ret(self.attacker_cfg_str, *cfgs[k][:3]))

    def run(self, montages):
        """The six steps in order; returns the setup's table (also printed, and written to <setup>/ret/<attacker_cfg_str>/stats.txt)."""
        import pandas as pd
        cfgs = self.find_configs()
        prj, infer, real = self.load_images(cfgs)
        cls = self.classify(cfgs, infer, real)
        pairs, sums, npix, valid = self.image_stats(prj, infer, real)
        rows = self.form_rows(cfgs, cls, pairs, sums, npix, valid)
        table = pd.DataFrame(rows, columns=SUMMARY_COLUMNS) if rows else pd.DataFrame(columns=SUMMARY_COLUMNS)
        print(f'\n-------------------- [{self.attacker_name}] results on [{self.setup.name}] --------------------')
        print(table.to_string(index=False, float_format='%.4f'))
        print('-------------------------------------- End of result table ---------------------------\n')
        os.makedirs(self.setup.ret(self.attacker_cfg_str), exist_ok=True)
        write_stats(table, self.setup.ret(self.attacker_cfg_str, 'stats.txt'))
        if montages and cfgs:
            self.write_montages(cfgs, prj, infer, real, cls, pairs, sums, npix)
        return table


def summarize_single_attacker(attacker_name, data_root, setup_list, device='cuda', device_ids=[0], *, classifiers=None, montages=False,
                              gpu_decode=False):
    """projector_based_attack.py:417-574: per setup, one row per attack configuration (stealth loss x d_thr x classifier) of
    `attacker_name` found on disk -- targeted top-1 / top-5 and untargeted top-1 success of the inferred and the real
    camera-captured attacks, and PSNR / RMSE / SSIM / L2 / L_inf / dE2000 of the projector images (vs the grey illumination), the
    inferred and the captured images (centre-cropped, vs the centre-cropped scene) over the targeted (T), untargeted (U) and all
    (All) attacks; <setup>/ret/<attacker_cfg_str>/stats.txt as the reference writes it.  Returns the last setup's DataFrame.

    `classifiers`: classifier name -> spaa_amd.Classifier (the reference builds them from downloaded weights); a configuration
    present on disk whose classifier is not given raises ValueError.  Differences from the reference:
      * a missing or empty folder skips that configuration only (the reference leaves the classifier loop at the first one);
      * the Valid_* columns are NaN, with a note, when the validation inferences are not on disk (this project's trainers do not
        write */infer/test);
      * no stats.xlsx (no Excel engine is a dependency);
      * the result montages (attack_results, <setup>/ret/<attacker_cfg_str>/<loss>/<d_thr>/<classifier>/img_0001..0011.png) are
        written with `montages=True` only.  They come from spaa_amd.montage: all montages of a setup from ONE attack_montages call
        (split only every MONTAGE_CHUNK montages to bound memory), with the labels' top-1 probabilities from the softmax computed
        for the success rates and the L2 values from the img_stats sums.  Their text is a bitmap font at the tiles' edges and the
        colour map a restatement of Jet (spaa_amd/montage.py); the tiles have the projector images' own size.
      * `gpu_decode=True` decodes the attack results and the validation pair on `device` (io.torch_imread_mt(..., device=): one
        batch per folder, the same values) instead of through Pillow one file after the other.
    Mechanism: all images of a setup are loaded at once, each classifier sees them in chunks of SUMMARY_CHUNK, and every image
    metric of the setup comes from ONE metrics.img_stats launch, grouped on the host with metrics.dists_from_sums."""
    import pandas as pd
    if attacker_name not in ATTACKERS:
        raise ValueError(f'{attacker_name} not supported!')
    device = torch.device(device)
    target_idx = target_classes(data_root, N_TARGETED)
    read = (lambda d: io.torch_imread_mt(d, device=device)) if gpu_decode else (lambda d: io.torch_imread_mt(d).to(device))
    table = pd.DataFrame(columns=SUMMARY_COLUMNS)
    for setup_name in setup_list:
        print(f'\nCalculating stats of [{attacker_name}] on [{join(data_root, "setups", setup_name)}]')
        setup = AttackSetup(data_root, setup_name)
        table = _SetupSummary(attacker_name, setup, target_idx, device, classifiers, read).run(montages)
    return table


def summarize_all_attackers(attacker_names, data_root, setup_list, recreate_stats_and_imgs=False, *, classifiers=None, montages=False):
    """projector_based_attack.py:577-614: concatenate <setup>/ret/<attacker_cfg_str>/stats.txt of every setup and attacker
    (recreated first by summarize_single_attacker when `recreate_stats_and_imgs`), and the pivot table of the SPAA paper's
    Table 1 (supplementary Table 2).  Writes <data_root>/setups/stats_all.txt and pivot_table_all.txt (tab-separated, 4
    decimals; the reference's .xlsx copies are not written: no Excel engine is a dependency).  `montages=True` is handed to
    summarize_single_attacker when the stats are recreated (the result montages).  Returns (table, pivot_table)."""
    import warnings
    import pandas as pd
    table = []
    for setup_name in setup_list:
        for attacker_name in attacker_names:
            ret_path = join(data_root, 'setups', setup_name, 'ret', to_attacker_cfg_str(attacker_name)[0])
            print(f'\nGathering stats of {ret_path}')
            if recreate_stats_and_imgs:
                summarize_single_attacker(attacker_name=attacker_name, data_root=data_root, setup_list=[setup_name],
                                          classifiers=classifiers, montages=montages)
            table.append(pd.read_csv(join(ret_path, 'stats.txt'), index_col=None, header=0, sep='\t'))
    table = pd.concat(table, axis=0, ignore_index=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', FutureWarning)   # (pandas' note on aggfunc=np.mean: the reference's call is kept as it is)
        pivot_table = pd.pivot_table(table, values=['T.top-1_real', 'T.top-5_real', 'U.top-1_real', 'T.real_L2', 'T.real_Linf',
                                                    'T.real_dE', 'T.real_SSIM', 'All.real_L2', 'All.real_Linf', 'All.real_dE',
                                                    'All.real_SSIM'],
                                     index=['Attacker', 'd_thr', 'Stealth_loss', 'Classifier'], aggfunc=np.mean, sort=False)
    pivot_table = pivot_table.sort_index(level=[0, 1], ascending=[False, True])   # to match SPAA Table order
    write_stats(table, join(data_root, 'setups/stats_all.txt'))
    pivot_table.to_csv(join(data_root, 'setups/pivot_table_all.txt'), float_format='%.4f', sep='\t', index=True)
    return table, pivot_table
