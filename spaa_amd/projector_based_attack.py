"""SPAA — Stealthy Projector-based Adversarial Attack, fused on device.

Drop-in for `spaa()` of /root/reference/src/python/projector_based_attack.py:212-339: same positional signature and
return value `(cam_infer_best, prj_adv_best)`; the reference's hard-coded locals (:243-258) are keyword arguments
with the reference values as defaults.  Differences in *mechanism*, not in result:

  * the sampling grid, skipConv1(s) and Lab(scene) are loop-invariant and computed once, not per iteration;
  * masks, top-1/confidence, loss reductions and best-so-far bookkeeping stay on the GPU (the reference syncs to
    the host three times per iteration: classifier.py:64, projector_based_attack.py:291,318);
  * ONE backward pass per iteration with a per-sample-selected cotangent instead of two (each sample consumes either
    the adversarial or the stealthiness gradient, :307 / :315, and samples are independent);
  * `cam_scene` may also be [B,3,H,W] (one scene per sample); the reference supports one scene x B targets (Q9),
    and its targeted mode needs B >= 8 because of a debug print (Q10) — not inherited.
"""
import os
import warnings

import torch

from . import _lib
from .models import PCNet, to_nhwc4, to_nchw   # noqa: F401
from .classifier import Attention, Classifier   # noqa: F401  (Attention: re-exported)
from .attack_options import (ENS_MAX, VIEWS_MAX, JITTER_MAX, TRANSFER_RMAX, UNIVERSAL_MAX, POSE_MAX_ROTATE, POSE_MAX_ZOOM,   # noqa: F401
                             POSE_MAX_TILT, POSE_MAX_SHIFT, CaptureJitter, PoseJitter, JpegCapture, CaptureBlur, Transfer, Universal,
                             BLUR_RMAX, BLUR_SIGMA_MAX,
                             checked_request, _unwrap, _ensemble_members, _universal_supported,
                             _view_pcnets, _views_supported, _jitter_supported, _pose_supported, _jpeg_supported, _blur_supported,
                             _attention_checked,
                             _attention_supported, _transfer_checked, _transfer_supported)
from .attack_state import (AttackState, EnsembleAttackState, MultiViewAttackState, UniversalAttackState, DrawAttackState,   # noqa: F401
                           JitterAttackState, PoseAttackState, JpegAttackState, BlurAttackState, JitterStage, PoseStage, JpegStage, BlurStage,
                           _is_scalar, _require_gpu,
                           _scene_batch)

# B * Hc * Wc up to which spaa() replays the iteration as a captured HIP graph (0 disables); above it the GPU is busy for
# longer than the host needs to enqueue an iteration and eager launches lose nothing (measured: < 1 % at B = 64, 256 x 256)
CLAMP_BITS = os.environ.get('SPAA_CLAMP_BITS', '1') == '1'   # the step writes the next backward pass's clamp gate as bytes (A/B runs: 0)
GRAPH_MAX_PIXELS = int(os.environ.get('SPAA_GRAPH_MAX_PIXELS', str(16 * 256 * 256)))
LAST_RUN = {}   # of the last spaa() call: executed iterations (1 eager + iters - 1 replays = iters: a capture executes nothing), graph or not
LOSS_TERMS = ('prjl2', 'caml2', 'camdE')


def loss_weights(stealth_loss):
    """(prjl2_w, caml2_w, camdE_w) of a stealth-loss string (projector_based_attack.py:275-287: a term is on when its name occurs)."""
    return (0.1 if 'prjl2' in stealth_loss else 0.0, 1.0 if 'caml2' in stealth_loss else 0.0,
            1.0 if 'camdE' in stealth_loss else 0.0)


def ssim_weight(stealth_loss):
    """The weight of the SSIM term 1 - SSIM(cam_infer, cam_scene) of a stealth-loss string: 1.0 when 'camssim' occurs in it, else 0.0
    (not a term of the reference, so not one of loss_weights()'s three)."""
    return 1.0 if 'camssim' in stealth_loss else 0.0


def _attack_state(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage, focus, jitter=None,
                  attention=None, transfer=None, pose=None, jpeg=None, universal=None, blur=None):
    """AttackState for one Classifier, EnsembleAttackState for a checked list of several, MultiViewAttackState for a checked list of
    PCNets (with their list of scenes), JitterAttackState for one Classifier with a CaptureJitter, PoseAttackState for one Classifier
    with a PoseJitter (with or without a CaptureJitter), JpegAttackState for one Classifier with a JpegCapture (with or without either of
    the other two), BlurAttackState for one Classifier with a CaptureBlur (with or without any of the other three); the last four take no
    `attention`; UniversalAttackState for one PCNet and one Classifier with a Universal.  Each of
    them takes `transfer`."""
    args = (pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device)
    if blur is not None:
        return BlurAttackState(*args, blur, storage=storage, pose=pose, jitter=jitter, jpeg=jpeg, transfer=transfer)
    if universal is not None:
        return UniversalAttackState(*args, universal, storage=storage, focus=focus, attention=attention, transfer=transfer)
    if jpeg is not None:
        return JpegAttackState(*args, jpeg, storage=storage, pose=pose, jitter=jitter, transfer=transfer)
    if pose is not None:
        return PoseAttackState(*args, pose, storage=storage, jitter=jitter, transfer=transfer)
    if jitter is not None:
        return JitterAttackState(*args, jitter, storage=storage, transfer=transfer)
    if isinstance(pcnet, list):
        return MultiViewAttackState(*args, storage=storage, focus=focus, attention=attention, transfer=transfer)
    if isinstance(classifier, list):
        return EnsembleAttackState(*args, storage=storage, focus=focus, attention=attention, transfer=transfer)
    return AttackState(*args, storage=storage, attention=attention, transfer=transfer)


def spaa(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr, stealth_loss, device, setup_info,
         *, iters=50, adv_lr=2, col_lr=1, p_thresh=0.9, trace=None, verbose=False, storage='f32', focus=False, jitter=None,
         attention=None, transfer=None, pose=None, jpeg=None, universal=None, blur=None):
    """Stealthy Projector-based Adversarial Attack (SPAA Algorithm 1) — see module docstring.

    :param pcnet: spaa_amd.PCNet (optionally wrapped in DataParallel-like `.module`), or a list / tuple of 2..4 of them: the same projector
        and scene seen from as many camera poses, ONE projection against all of these views (MultiViewAttackState; one Classifier,
        fp32 storage, one camera size).  `cam_scene` is then a list of one scene per view and the first return value a list of one
        camera image batch per view.  A sequence of one is that PCNet.
    :param classifier: spaa_amd.Classifier, or a list / tuple of 2..4 of them with the same classes: ONE projection against all of them
        (EnsembleAttackState; fp32 storage only).  A sequence of one is that classifier.
    :param focus: ensembles, views and universal groups only: members / views that are already fooled rest until all are (a universal
        group: until enough are) (default: every one pulls all the time)
    :param jitter: a CaptureJitter: ONE projection against `jitter.draws` randomly perturbed captures of the camera image per iteration,
        the first of them the clean one (JitterAttackState; one PCNet, one Classifier, fp32 storage, no `focus`).  The trace entries
        are the ensemble's, with draws as members.  None (default): the attack on the noiseless inferred capture
    :param attention: an Attention: the classifier's gradient image is weighted by floor + (1 - floor) M, M the Grad-CAM map of the
        sample's class on the classifier crop (fp32 storage, a spaa_amd.Classifier, no `jitter`).  In an ensemble every
        member uses its own map, with several views every view its own.  vit_b_16 has no such map and is refused, unless
        `attention.rollout` is set: then its M is the attention rollout of its class token, written in the backward
        pass itself, and convolutional members keep Grad-CAM.  None (default): the plain attack, launch for launch
    :param transfer: a Transfer: the adversarial step follows the Gaussian-smoothed, momentum-accumulated gradient image at the projector
        instead of the raw one (fp32 storage, a spaa_amd.Classifier).  Combines with ensembles, views, `focus`, `jitter`
        and `attention`: it acts on the projector-side gradient after them.  None (default): the plain attack, launch for launch
    :param pose: a PoseJitter: ONE projection against `pose.draws` randomly warped copies of the camera image per iteration (a small
        random change of camera pose: rotation, zoom, translation, tilt), the first of them the unwarped one (PoseAttackState, DESIGN.md
        7k; one PCNet, one Classifier, fp32 storage, no `focus`, no `attention`).  With `jitter` of the same `draws`, draw j is
        Jitter_j(Pose_j(y)).  The trace entries are the ensemble's, with draws as members.  None (default): launch for launch as before
    :param jpeg: a JpegCapture: ONE projection against `jpeg.draws` JPEG round trips of the camera image per iteration, each at a
        quality drawn from `jpeg.quality`, the first of them the uncompressed capture (JpegAttackState; one PCNet, one
        Classifier, fp32 storage, no `focus`, no `attention`).  With `pose` and / or `jitter` of the same `draws` the codec comes last:
        draw j is Jpeg_j(Jitter_j(Pose_j(y))).  The decision's stealth loss and `cam_best` stay the clean inference's.  None
        (default): launch for launch as before
    :param universal: a Universal: the batch is cut into groups of `universal.size` consecutive samples, each sample with its own scene
        (`cam_scene` [B,3,H,W]) and its own class in `target_idx`, and every group shares ONE projector image: the light pattern that
        fools the classifier whatever scene of the group stands in front of the projector (UniversalAttackState; one
        PCNet, one Classifier, fp32 storage, no `jitter`, `pose` or `jpeg`; B a multiple of the size; `targeted`, `d_thr` and the
        stealth loss uniform within a group).  A group is fooled when ceil(universal.rate * size) of its members are; the members'
        gradient images meet at the projector as the views' of a multi-view attack do.  Combines with `attention`, `transfer` and
        `focus` (a fooled member rests until its group is fooled).  The return shapes stay: the rows of a group in `prj_adv_best`
        are equal, `cam_infer_best` is per sample; the trace entries are (state, stats, uni_state, uni_stats), where state[:, 3]
        counts the group's fooled members.  attack_summary.universal_success projects the result onto scenes held out from the
        attack.  None (default): launch for launch as before
    :param blur: a CaptureBlur: ONE projection against `blur.draws` defocused copies of the camera image per iteration, each through a
        Gaussian lens blur of a sigma drawn from `blur.sigma` (camera pixels, border replicated), the first of them the sharp capture
        (BlurAttackState; one PCNet, one Classifier, fp32 storage, no `focus`, no `attention`, no `universal`).  With
        `pose`, `jitter` and / or `jpeg` of the same `draws` the stages run in the optical order, geometry, lens, sensor, codec: draw j
        is Jpeg_j(Jitter_j(Blur_j(Pose_j(y)))).  Combines with `transfer` and every stealth-loss string; the decision's stealth loss
        and `cam_best` stay the clean inference's.  attack_summary.blur_survival replays a result through fixed sigmas.  None
        (default): launch for launch as before
    :param imagenet_labels: dict idx -> name (only used when verbose)
    :param target_idx: list of B class ids (true label if untargeted)
    :param targeted: bool
    :param cam_scene: [3,H,W] / [1,3,H,W] / [B,3,H,W] in [0,1]
    :param d_thr: SPAA Algorithm 1's threshold on the mean per-pixel L2 perturbation (x255)
    :param stealth_loss: string containing any of 'prjl2', 'caml2', 'camdE', 'camssim' (the last: 1 - SSIM of the inferred capture
        against the scene joins the colour loss; a spaa_amd.Classifier only)
    :param setup_info: {'classifier_crop_sz', 'prj_brightness', 'prj_im_sz'}
    :param trace: optional list; receives per-iteration (state, stats) device tensors (no sync inside the loop); for an ensemble
        (state, stats, ens_state, ens_stats), where state[:, 3] counts the fooled members and ens_state holds each member's top-1;
        for several views (state, stats, view_state, view_stats) in the same way
    :return: (cam_infer_best [B,3,Hc,Wc], prj_adv_best [B,3,Hp,Wp] in [0,1]); for several views ([cam_infer_best per view], prj_adv_best)
    """
    pcnet, classifier, cam_scene = checked_request('spaa', pcnet, classifier, cam_scene, storage, focus, jitter, pose, attention, transfer,
                                                   jpeg, universal, blur)
    if universal is not None:   # (`targeted` / `d_thr` may be one per sample here: groups may differ from each other, not within)
        for name, value in (('targeted', targeted), ('d_thr', d_thr)):
            if not _is_scalar(value):
                universal.check_uniform(name, list(value), 'spaa')
    if not isinstance(classifier, (Classifier, list)):
        if not callable(classifier):
            raise TypeError('classifier must be a spaa_amd.Classifier or a callable (im, crop_sz) -> (raw_score, p, idx)')
        return _spaa_foreign_classifier(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr,
                                        stealth_loss, device, setup_info, iters, adv_lr, col_lr, p_thresh, trace)
    st = _attack_state(pcnet, classifier, target_idx, cam_scene, stealth_loss, setup_info, device, storage, focus, jitter, attention,
                       transfer, pose, jpeg, universal, blur=blur)

    def report(i):
        if i % 30 == 0 or i == iters - 1:
            s, f = st.state.cpu(), st.stats.cpu()
            v = 7 if (targeted and st.B > 7) else 0
            name = f'of {getattr(st, "N", len(st.clfs))} {st.label} fooled' if st.label else (imagenet_labels[int(s[v, 3])] if imagenet_labels else '')
            print(f'col_loss = {f[:, 3].mean():<9.4f} | prjl2 = {f[:, 4].mean() * 255:<9.4f} | caml2 = '
                  f'{f[:, 1].mean() * 255:<9.4f} | camdE = {f[:, 2].mean():<9.4f} | p = {f[v, 0]:.4f} | y = '
                  f'{int(s[v, 3]):3d} ({name})')

    _run(st, targeted, d_thr, iters, adv_lr, col_lr, p_thresh, trace, report if verbose else None)
    return st.results()


def _run(st, targeted, d_thr, iters, adv_lr, col_lr, p_thresh, trace=None, report=None):
    """The loop of spaa() (projector_based_attack.py:264-328) on an AttackState; `targeted` / `d_thr` one value or one per sample."""
    if trace is None and report is None and iters >= 4 and st.B * st.HWc <= GRAPH_MAX_PIXELS:
        # Few pixels (the reference's own calls: B = 1 and B = 10 at 240 x 320): an iteration's ~120 launches take the GPU
        # less time than the host needs to enqueue them.  The loop body has no host-side dependence on the iteration, so it is
        # captured ONCE as a HIP graph (after one eager iteration: kernel attributes, workspaces and the per-sample table exist)
        # and replayed.
        with torch.cuda.device(st.dev):
            st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)
            done = 1
            try:
                # (thread-local: GPU calls of OTHER threads -- a loader's pin-memory thread, another attack -- do not abort it)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)   # (recorded, not executed)
            except RuntimeError as e:
                # the capture was refused or a launch inside it failed: the remaining iterations run kernel by kernel (same
                # results; a real launch error shows again there, un-captured) -- said aloud, and recorded in LAST_RUN
                warnings.warn(f'spaa(): HIP-graph capture of the iteration failed, running eagerly: {type(e).__name__}: {e}',
                              RuntimeWarning, stacklevel=3)
                graph = None
            while done < iters:
                if graph is not None:
                    graph.replay()
                else:
                    st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)
                done += 1
        LAST_RUN.update(iterations=done, graph=graph is not None)
        return
    LAST_RUN.update(iterations=iters, graph=False)
    for i in range(iters):
        st.iteration(targeted, d_thr, adv_lr, col_lr, p_thresh)
        if trace is not None:
            trace.append(st.trace_entry())
        if report is not None:
            report(i)


def plan_sweep(configs, max_batch=64):
    """Host side of spaa_sweep: validates `configs` [(stealth_loss, d_thr, targeted, target_idx), ...] and flattens them, in order,
    into samples (config index, stealth_loss, d_thr, targeted, target), cut into chunks [(start, stop), ...] of at most `max_batch`
    samples (a chunk may hold several configs and may split one).  Errors name the config."""
    if int(max_batch) < 1:
        raise ValueError(f'max_batch must be >= 1, got {max_batch}')
    samples = []
    for i, cfg in enumerate(configs):
        try:
            loss, d_thr, targeted, target_idx = cfg
        except (TypeError, ValueError):
            raise ValueError(f'configs[{i}]: expected (stealth_loss, d_thr, targeted, target_idx), got {cfg!r}') from None
        if not isinstance(loss, str) or not loss or any(t not in LOSS_TERMS + ('camssim',) for t in loss.split('_')):
            raise ValueError(f'configs[{i}]: unknown stealth loss {loss!r} (terms joined by "_": {", ".join(LOSS_TERMS)}, camssim)')
        target_idx = list(target_idx)
        if not target_idx:
            raise ValueError(f'configs[{i}]: target_idx is empty: nothing to attack')
        samples += [(i, loss, float(d_thr), bool(targeted), int(t)) for t in target_idx]
    if not samples:
        raise ValueError('configs is empty: nothing to attack')
    mb = int(max_batch)
    return samples, [(a, min(a + mb, len(samples))) for a in range(0, len(samples), mb)]


def split_sweep(samples, ncfg, chunk_results):
    """Inverse of plan_sweep's flattening: per-chunk (cam [n,...], prj [n,...]) in sample order -> one (cam, prj) per config."""
    cams = torch.cat([c for c, _ in chunk_results])
    prjs = torch.cat([p for _, p in chunk_results])
    assert cams.shape[0] == len(samples)
    out, a = [], 0
    for i in range(ncfg):
        b = a
        while b < len(samples) and samples[b][0] == i:
            b += 1
        out.append((cams[a:b], prjs[a:b]))
        a = b
    return out


def spaa_sweep(pcnet, classifier, imagenet_labels, cam_scene, setup_info, device, configs, *, iters=50, adv_lr=2, col_lr=1,
               p_thresh=0.9, max_batch=64, storage='f32', trace=None, focus=False, jitter=None, attention=None, transfer=None,
               pose=None, jpeg=None, universal=None, blur=None):
    """Several SPAA attacks on one PCNet, scene and classifier as few batched attacks (the reference's driver makes one spaa() call
    per configuration: projector_based_attack.py:24-148).  `configs`: [(stealth_loss, d_thr, targeted, target_idx), ...]; returns one
    (cam_infer_best, prj_adv_best) per config, in order -- what spaa(pcnet, classifier, imagenet_labels, target_idx, targeted,
    cam_scene, d_thr, stealth_loss, device, setup_info) returns for it: samples do not interact, so only the batch differs.  The
    samples of all configs are flattened in order and cut into chunks of at most `max_batch` (one AttackState each, the loop of
    spaa() with its loss weights, targeted flag and d_thr per sample); `trace` receives one list per chunk, of the per-iteration
    (state, stats) pairs spaa() records (the chunk's samples in flattened order).  `classifier` may be a list / tuple of 2..4
    Classifiers, as in spaa(): every sample then attacks all of them at once (`focus` as there), and the trace entries are
    (state, stats, ens_state, ens_stats).  `pcnet` may be a list / tuple of 2..4 PCNets with `cam_scene` a list of their scenes, as
    in spaa(): every sample then attacks all views at once, each config's first return value is a list of one camera image batch
    per view, and the trace entries are (state, stats, view_state, view_stats).  `jitter`: a CaptureJitter, as in spaa(): every chunk
    is a jitter attack with that seed (the draws of a sample depend on its place in its chunk), the trace entries the ensemble's.
    `attention`: an Attention, as in spaa(): every chunk is an attention-weighted attack.  `transfer`: a Transfer, as in spaa(): every
    chunk's adversarial steps follow the smoothed, momentum-accumulated direction (each chunk's momentum starts at zero).  `pose`: a
    PoseJitter, as in spaa(): every chunk is a pose attack with that seed (the draws of a sample depend on its place in its chunk).
    `jpeg`: a JpegCapture, as in spaa(): every chunk is a JPEG attack with that seed, in the same way.  `blur`: a CaptureBlur, as in spaa(): every chunk is a blur attack with that seed, in the same way.  `universal` is refused: the
    sweep batches configurations of ONE scene, a universal projection is over several."""
    if universal is not None:
        raise NotImplementedError('spaa_sweep: universal= is not implemented (the sweep batches the configurations of one scene; a '
                                  'universal projection shares one image among several scenes): call spaa(..., universal=...)')
    samples, chunks = plan_sweep(configs, max_batch)
    pcnet, classifier, cam_scene = checked_request('spaa_sweep', pcnet, classifier, cam_scene, storage, focus, jitter, pose, attention,
                                                   transfer, jpeg, None, blur)
    if not isinstance(classifier, (Classifier, list)):
        raise TypeError('spaa_sweep needs a spaa_amd.Classifier')
    _require_gpu(device, 'spaa_sweep')

    def one_scene(m, scene):
        sc = _scene_batch(scene, 1)
        cam_sz = tuple(m.warping_net.out_size)
        if sc.ndim != 4 or sc.shape[0] != 1 or tuple(sc.shape[1:]) != (3,) + cam_sz:
            raise ValueError(f'cam_scene must be [3,H,W] or [1,3,H,W] with (H, W) = {cam_sz} (PCNet\'s output); got {tuple(scene.shape)}')
        return sc

    sc = [one_scene(m, s) for m, s in zip(pcnet, cam_scene)] if isinstance(pcnet, list) else one_scene(pcnet, cam_scene)
    results = []
    for a, b in chunks:
        part = samples[a:b]
        st = _attack_state(pcnet, classifier, [t for *_, t in part], sc, [s[1] for s in part], setup_info, device, storage, focus,
                           jitter, attention, transfer, pose, jpeg, blur=blur)
        tr = [] if trace is not None else None
        _run(st, [s[3] for s in part], [s[2] for s in part], iters, adv_lr, col_lr, p_thresh, tr)
        if trace is not None:
            trace.append(tr)
        results.append(st.results())
        del st
    if isinstance(pcnet, list):   # (a chunk's result holds one camera image per view: split view by view)
        per_view = [split_sweep(samples, len(configs), [(cams[v], prj) for cams, prj in results]) for v in range(len(pcnet))]
        return [([pv[i][0] for pv in per_view], per_view[0][i][1]) for i in range(len(configs))]
    return split_sweep(samples, len(configs), results)


class _StealthFn(torch.autograd.Function):
    """Per-sample camera-side stealth loss caml2_w * caml2 + camdE_w * camdE (projector_based_attack.py:279-284) through
    the fused HIP kernel; the kernel's analytic gradient is kept for backward."""

    @staticmethod
    def forward(ctx, cam_infer, scene4, scene_lab, caml2_w, camdE_w):
        y4 = to_nhwc4(cam_infer)
        b, h, w, _ = y4.shape
        nblk = (h * w + 255) // 256
        part = torch.zeros(b, nblk, 3, device=y4.device)
        g = torch.zeros_like(y4)
        _lib.call('spaa_stealth_loss_fwd_bwd', _lib.ptr(y4), _lib.ptr(scene4), _lib.ptr(scene_lab), float(caml2_w),
                  float(camdE_w), 1.0 / (h * w), _lib.ptr(g), None, _lib.ptr(part), b, h * w)
        sums = part.sum(dim=1) / (h * w)
        ctx.g = to_nchw(g)
        ctx.mark_non_differentiable(sums)
        return caml2_w * sums[:, 0] + camdE_w * sums[:, 1], sums

    @staticmethod
    def backward(ctx, g_loss, _g_sums):
        return ctx.g * g_loss.view(-1, 1, 1, 1), None, None, None, None


def _spaa_foreign_classifier(pcnet, classifier, imagenet_labels, target_idx, targeted, cam_scene, d_thr, stealth_loss,
                             device, setup_info, iters, adv_lr, col_lr, p_thresh, trace):
    """The reference accepts ANY callable `classifier(im, crop_sz) -> (raw_score, p_sorted, idx)`
    (projector_based_attack.py:266).  For a classifier that is not a spaa_amd.Classifier the fused loop cannot run its
    body, so this route keeps PCNet (forward + input gradient) and the stealth loss on the HIP kernels, lets torch.autograd
    carry the gradient through the foreign classifier, and follows the reference's loop :264-328 step by step — with one
    backward pass of the per-sample-selected loss instead of two (samples are independent, see AttackState)."""
    if ssim_weight(stealth_loss):
        raise NotImplementedError("spaa(): the 'camssim' term runs in the fused loop only: pass a spaa_amd.Classifier, not a callable")
    dev = _require_gpu(device, 'spaa')
    B = len(target_idx)
    with _lib.on_device(dev):
        cp_sz = tuple(setup_info['classifier_crop_sz'])
        gray = float(setup_info['prj_brightness'])
        scene = _scene_batch(cam_scene, B).to(dev).contiguous()
        scene4 = to_nhwc4(scene)
        scene_lab = torch.zeros_like(scene4)
        _lib.call('spaa_rgb2lab', _lib.ptr(scene4), _lib.ptr(scene_lab), scene4.numel() // 4)
        im_gray = torch.full((B, 3) + tuple(setup_info['prj_im_sz']), gray, device=dev)
        prj_adv = im_gray.clone().requires_grad_(True)
        prjl2_w, caml2_w, camdE_w = loss_weights(stealth_loss)
        tgt = torch.as_tensor([int(t) for t in target_idx], device=dev)
        ar = torch.arange(B, device=dev)
        prj_best, cam_best = prj_adv.detach().clone(), scene.clone()
        col_best = torch.full((B,), 1e6, device=dev)
        for _ in range(iters):
            cam_infer = pcnet(torch.clamp(prj_adv, 0, 1), scene)                                   # :265
            raw_score, p, idx = classifier(cam_infer, cp_sz)                                       # :266
            sel = raw_score[ar, tgt.to(raw_score.device)].to(dev)
            adv_b = (-sel if targeted else sel) / B                                                # :269-272 (per sample)
            col_b, sums = _StealthFn.apply(cam_infer, scene4, scene_lab, caml2_w, camdE_w)         # :279-284
            if prjl2_w:
                col_b = col_b + prjl2_w * torch.norm(im_gray - prj_adv, dim=1).mean(1).mean(1)     # :275-276
            top1 = torch.as_tensor(idx[:, 0]).to(dev)
            p1 = torch.as_tensor(p[:, 0]).to(dev)
            high_pert = sums[:, 0] * 255 > d_thr                                                   # :291
            succ = (top1 == tgt) if targeted else (top1 != tgt)                                    # :294,298
            best_adv = succ & high_pert & ((p1 > p_thresh) if targeted else torch.ones_like(succ))  # :295,299
            loss = torch.where(best_adv, col_b / B, adv_b).sum()
            g, = torch.autograd.grad(loss, prj_adv)                                                # :302 / :310
            norm = g.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
            lr = torch.where(best_adv, float(col_lr), float(adv_lr)).view(-1, 1, 1, 1)
            with torch.no_grad():
                prj_adv -= lr * g / norm                                                           # :307, :315
                col = col_b.detach()
                best = (col < col_best) & best_adv                                                 # :318-320
                col_best = torch.where(best, col, col_best)
                upd = (succ | best).view(-1, 1, 1, 1)
                prj_best = torch.where(upd, prj_adv.detach(), prj_best)                            # :323-328 (post-step, Q4)
                cam_best = torch.where(upd, cam_infer.detach(), cam_best)
            if trace is not None:
                trace.append(dict(succ=succ.clone(), best_adv=best_adv.clone(), best=best.clone(), top1=top1.clone(),
                                  caml2=sums[:, 0].clone(), camdE=sums[:, 1].clone(), prj_adv=prj_adv.detach().clone()))
        return cam_best, torch.clamp(prj_best, 0, 1)                                               # :337


spaa_attack = spaa  # name used by BASELINE.json's north_star


# The experiment driver and the summary step live in their own modules; their public names stay importable from here (the same
# objects).  Neither module imports this one at import time: they reach the attack through it when they are called.
from .attack_driver import (ATTACKERS, MODEL_TRAIN_CFG, AttackSetup, get_attacker_cfg, to_attacker_cfg_str,   # noqa: E402,F401
                            run_projector_based_attack, _run_one_pixel_de, project_capture_real_attack)
from .jpeg import jpeg_roundtrip, quant_tables   # noqa: E402,F401
from .blur import gaussian_blur   # noqa: E402,F401
from .attack_summary import (SUMMARY_STEALTH_LOSSES, SUMMARY_D_THRESHES, SUMMARY_CLASSIFIERS, SUMMARY_CHUNK,   # noqa: E402,F401
                             SUMMARY_COLUMNS, MONTAGE_CHUNK, attack_success, write_stats, _sorted_classes, _nonempty,
                             attack_results, attack_transfer, capture_survival, pose_survival, jpeg_survival, blur_survival, transfer_success,
                             universal_success,
                             summarize_single_attacker, summarize_all_attackers)