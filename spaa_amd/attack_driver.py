"""The reference's experiment driver (projector_based_attack.py:24-209): the attacker configurations, one setup folder as the steps
read it (AttackSetup), and the steps that write adversarial images.  spaa_amd.projector_based_attack re-exports the public names;
this module imports it, perc_al and the One-pixel attacker only when a step is called, and calls them through their modules."""
import itertools
import os
import random
from os.path import join

import numpy as np
import torch

from . import io
from .classifier import load_imagenet_labels
from .img_proc import center_crop, expand_4d

ATTACKERS = ('SPAA', 'PerC-AL+CompenNet++', 'One-pixel_DE')
QUERY_ATTACKERS = ('Square',)    # attackers of this project that the reference lacks: the driver runs them, the summary step does not read them
MODEL_TRAIN_CFG = dict(loss='l1+ssim', num_train=500, batch_size=24, max_iters=2000)   # get_model_train_cfg's defaults (train_network.py)


def get_attacker_cfg(attacker_name, data_root, setup_list, device_ids=[0], load_pretrained=False, plot_on=True):
    """projector_based_attack.py:169-192: the default attacker configuration, as a mapping with attribute access."""
    cfg = io.SetupInfo(attacker_name=attacker_name, classifier_names=['inception_v3', 'resnet18', 'vgg16'], data_root=data_root,
                    setup_list=setup_list, device='cuda', device_ids=device_ids, load_pretrained=load_pretrained, plot_on=plot_on)
    if attacker_name == 'SPAA':
        cfg.stealth_losses, cfg.d_threshes = ['caml2', 'camdE', 'camdE_caml2'], [5, 7, 9, 11]
    elif attacker_name == 'PerC-AL+CompenNet++':
        cfg.stealth_losses, cfg.d_threshes = ['camdE'], [11]
    elif attacker_name == 'One-pixel_DE':
        cfg.stealth_losses, cfg.d_threshes = ['-'], ['-']
    elif attacker_name == 'Square':
        # square_eps8 (the budget in 8-bit projector levels) has no default: see ProjectorSquareAttacker.attack
        cfg.stealth_losses, cfg.d_threshes, cfg.square_eps8, cfg.square_iters, cfg.square_proposals = ['-'], ['-'], None, 1000, 1
    return cfg


def to_attacker_cfg_str(attacker_name):
    """projector_based_attack.py:195-209: (attacker_cfg_str, model_cfg_str), the result folders' names."""
    if attacker_name not in ATTACKERS + QUERY_ATTACKERS:
        raise ValueError(f'{attacker_name} not supported!')
    m = MODEL_TRAIN_CFG
    tail = f'{m["loss"]}_{m["num_train"]}_{m["batch_size"]}_{m["max_iters"]}'
    if attacker_name == 'SPAA':
        return f'SPAA_PCNet_{tail}', f'PCNet_{tail}'
    if attacker_name == 'PerC-AL+CompenNet++':
        return f'{attacker_name}_{tail}', f'CompenNet++_{tail}'
    return attacker_name, None


def target_classes(data_root, n=10):
    """The class ids of the targeted attacks: the first `n` of <data_root>/imagenet10_clsidx_to_labels.txt, in the file's order."""
    target_labels = load_imagenet_labels(join(data_root, 'imagenet10_clsidx_to_labels.txt'))
    return list(dict(itertools.islice(target_labels.items(), n)).keys())


def _under(kind):
    return lambda self, *folder: join(self.path, kind, *map(str, folder))


class AttackSetup:
    """One setup, <data_root>/setups/<setup_name>, as the attack steps and the summary read it: its setup info, the camera-captured
    scene, the two label files of `data_root`, and the result folders <kind>/<attacker_cfg_str>/<loss>/<d_thr>/<classifier>."""

    def __init__(self, data_root, setup_name):
        self.data_root, self.name = data_root, setup_name
        self.path = join(data_root, 'setups', setup_name)
        self.info = io.load_setup_info(self.path)
        self.crop_sz = self.info['classifier_crop_sz']

    def raw_scene(self):
        """The scene under the grey illumination as the camera wrote it, float [3,H,W] (the summary's pairs crop it themselves)."""
        return io.torch_imread(join(self.path, 'cam/raw/ref/img_0002.png'))

    def cam_scene(self):
        """The scene at the camera size PCNet works on: the centre crop of the reference's drivers."""
        return center_crop(self.raw_scene(), tuple(self.info['cam_im_sz'])[::-1])

    def imagenet_labels(self):
        return load_imagenet_labels(join(self.data_root, 'imagenet1000_clsidx_to_labels.txt'))

    def target_idx(self, n=10):
        return target_classes(self.data_root, n)

    @staticmethod
    def folder(attacker_cfg_str, loss, d_thr, classifier):
        return join(attacker_cfg_str, loss, str(d_thr), classifier)

    # where a configuration's images live: each takes folder()'s arguments (with fewer of them, a folder above it)
    prj_adv, cam_infer_adv, cam_raw_adv, ret = map(_under, ('prj/adv', 'cam/infer/adv', 'cam/raw/adv', 'ret'))


def _freeze(model):
    """The attacks treat the model as a constant (projector_based_attack.py:62-67)."""
    model.eval()
    for param in model.parameters():
        param.requires_grad = False


def _one_setup(cfg, who=''):
    """The only setup of `cfg` (steps with a projector and a camera in the loop)."""
    if len(cfg.setup_list) != 1:
        raise ValueError(f'{who}cfg.setup_list must hold exactly one setup (the projector and the camera see one scene), got '
                         f'{list(cfg.setup_list)}')
    return cfg.setup_list[0]


def ensemble_members(classifier_name):
    """The member names of an entry of cfg.classifier_names: 'a+b+c' is the ensemble of a, b and c, in the written order; a name
    without '+' is its own only member."""
    members = classifier_name.split('+')
    if not all(members):
        raise ValueError(f'classifier name {classifier_name!r}: an empty member name')
    return members


def _require_classifiers(cfg, classifiers):
    names = [m for c in cfg.classifier_names for m in ensemble_members(c)]
    missing = [c for c in dict.fromkeys(names) if c not in (classifiers or {})]
    if missing:
        raise ValueError(f'run_projector_based_attack: pass classifiers={{name: spaa_amd.Classifier}} for {missing} '
                         '(weights cannot be downloaded here)')


def _check_capture(capture):
    if capture != 'model' and not callable(capture):
        raise ValueError("capture must be 'model' or a function setup_info -> capture callable")


def _resolve_capture(capture, who, models, setup, cam_scene=None):
    """(capture callable, simulated) of a checked `capture` argument: 'model' = models[setup] (a trained PCNet, frozen here) stands in
    for the projector and the camera through SimulatedCapture with the camera's 8-bit step on `cam_scene` (read from the setup when
    not given); a function = capture(setup_info), a real ProCams pair.  `who` names the calling step in the error."""
    if not isinstance(capture, str):
        return capture(setup.info), False
    from .models import PCNet
    from .one_pixel_attacker import SimulatedCapture
    model = (models or {}).get(setup.name)
    if not isinstance(model, PCNet):
        raise ValueError(f"{who}: capture='model' needs models={{{setup.name!r}: trained PCNet}}, got {type(model).__name__}")
    _freeze(model)
    return SimulatedCapture(model, setup.cam_scene() if cam_scene is None else cam_scene, quantize=True), True


def _scene_top1(classifier, cam_scene, crop_sz):
    """(the class the classifier gives the unattacked scene, its probabilities): argmax of the raw scores, which holds for sorted and
    unsorted results alike (pred_idx[0, 0] / p.argmax() in the reference)."""
    with torch.no_grad():
        raw_score, p, _ = classifier(cam_scene, crop_sz)
    return int(raw_score[0].argmax()), p


def _train_model(cfg, setup_name, model_cfg):
    """projector_based_attack.py:50-60, run_projector_based_attack's `train=True`; leaves the configuration in cfg.model_cfg."""
    from . import train_network as tn
    spaa = cfg.attacker_name == 'SPAA'
    mcfg = tn.get_model_train_cfg(model_list=['PCNet' if spaa else 'CompenNet++'], data_root=cfg.data_root, setup_list=[setup_name],
                                  device_ids=cfg.device_ids, load_pretrained=cfg.load_pretrained, plot_on=cfg.plot_on)
    mcfg.device = cfg.device
    mcfg.update(model_cfg or {})
    model, _, cfg.model_cfg = (tn.train_eval_pcnet if spaa else tn.train_eval_compennet_pp)(mcfg)
    return model


def run_projector_based_attack(cfg, *, models=None, classifiers=None, iters=50, train=False, model_cfg=None, capture=None):
    """projector_based_attack.py:24-148 for the deep-learning attackers: per setup and classifier, 10 targeted attacks (the first 10
    imagenet10 classes) and 1 untargeted attack (the scene's top-1) for every stealth loss x d_thr; results under
    <setup>/prj/adv and <setup>/cam/infer/adv / <attacker_cfg_str>/<loss>/<d_thr>/<classifier>/img_0001..0011.png (1-10 targeted,
    11 untargeted).  For SPAA one classifier's whole sweep is ONE spaa_sweep call.
    A name with '+' in cfg.classifier_names, such as 'inception_v3+resnet18+vgg16', is the ensemble of the named members of
    `classifiers` (SPAA only): one projection per sample against all of them, written to a folder of that name like any classifier's.
    Its untargeted label is the scene's top-1 under the FIRST member; a warning is printed when the members disagree on the scene.
    `models`: setup name -> trained PCNet (SPAA) / CompenNetPlusplus (PerC-AL+CompenNet++); `classifiers`: classifier name ->
    spaa_amd.Classifier (the reference downloads the classifier weights here; that is not done).
    `train=True`: a setup without an entry in `models` is trained, or with cfg.load_pretrained loaded from its checkpoint, as the
    reference does (:50-60): train_network.train_eval_pcnet (SPAA) / train_eval_compennet_pp (PerC-AL+CompenNet++) on
    get_model_train_cfg's defaults, with the fields of `model_cfg` (a mapping, e.g. dict(max_iters=100)) laid over them; the last
    configuration is left in cfg.model_cfg.  The default, train=False, raises for such a setup.
    `capture` (One-pixel_DE only, :69-73,110-142): 'model' = models[setup] is a trained PCNet that stands in for the projector and the
    camera (SimulatedCapture; captures go under cam/infer/adv), or a function setup_info -> capture callable for a real ProCams pair
    (captures go under cam/raw/adv): see _run_one_pixel_de."""
    from . import perc_al, projector_based_attack as core
    name = cfg.attacker_name
    if name not in ATTACKERS + QUERY_ATTACKERS:
        raise ValueError(f'{name} not supported!')
    if name == 'Square':
        if capture is None:
            raise NotImplementedError('Square attacks the real scene through a projector and a camera; pass capture=\'model\' (a trained '
                                      'PCNet in `models` simulates the capture) or capture=<function setup_info -> capture callable>')
        return _run_square(cfg, models, classifiers, capture)
    if name == 'One-pixel_DE':
        if capture is None:
            raise NotImplementedError('One-pixel_DE attacks the real scene through a projector and a camera; use '
                                      'spaa_amd.DigitalOnePixelAttacker for the digital attack, or pass capture=\'model\' (a trained '
                                      'PCNet in `models` simulates the capture) or capture=<function setup_info -> capture callable>')
        return _run_one_pixel_de(cfg, models, classifiers, capture)
    device = torch.device(cfg.device)
    random.seed(0)   # (ut.reset_rng_seeds(0))
    torch.manual_seed(0)
    attacker_cfg_str = to_attacker_cfg_str(name)[0]
    grid = [(loss, d_thr) for loss in cfg.stealth_losses for d_thr in cfg.d_threshes]
    for setup_name in cfg.setup_list:
        model = (models or {}).get(setup_name)
        if model is None and train:
            model = _train_model(cfg, setup_name, model_cfg)
        if model is None:
            raise ValueError(f'run_projector_based_attack: pass models={{{setup_name!r}: trained '
                             f'{"PCNet" if name == "SPAA" else "CompenNetPlusplus"}}} (models are not trained here)')
        _require_classifiers(cfg, classifiers)
        setup = AttackSetup(cfg.data_root, setup_name)
        cam_scene = setup.cam_scene().to(device)
        imagenet_labels, target_idx = setup.imagenet_labels(), setup.target_idx()
        _freeze(model)
        for classifier_name in cfg.classifier_names:
            members = ensemble_members(classifier_name)
            if len(members) > 1:
                if name != 'SPAA':
                    raise NotImplementedError(f'{name}: classifier ensembles ({classifier_name!r}) are attacked by SPAA only')
                classifier = [classifiers[m] for m in members]
                tops = [_scene_top1(c, cam_scene, setup.crop_sz)[0] for c in classifier]
                true_idx = tops[0]
                if any(t != true_idx for t in tops):
                    print(f'warning: the members of [{classifier_name}] disagree on the unattacked scene (top-1 {dict(zip(members, tops))}); '
                          f'the untargeted attack uses {members[0]}\'s label {true_idx}')
            else:
                classifier = classifiers[classifier_name]
                true_idx, _ = _scene_top1(classifier, cam_scene, setup.crop_sz)
            if name == 'SPAA':
                configs = [c for loss, d_thr in grid for c in ((loss, d_thr, True, target_idx), (loss, d_thr, False, [true_idx]))]
                res = core.spaa_sweep(model, classifier, imagenet_labels, cam_scene, setup.info, device, configs, iters=iters)
                res = {g: (res[2 * k], res[2 * k + 1]) for k, g in enumerate(grid)}
            else:
                res = {(loss, d_thr): tuple(perc_al.perc_al_compennet_pp(model, classifier, imagenet_labels, t, tg, cam_scene, d_thr,
                                                                         device, setup.info)
                                            for t, tg in ((target_idx, True), ([true_idx], False)))
                       for loss, d_thr in grid}
            for (loss, d_thr), ((cam_tar, prj_tar), (cam_untar, prj_untar)) in res.items():
                folder = (attacker_cfg_str, loss, d_thr, classifier_name)
                io.save_imgs(torch.cat((cam_tar, cam_untar), 0), setup.cam_infer_adv(*folder))
                io.save_imgs(torch.cat((prj_tar, prj_untar), 0), setup.prj_adv(*folder))
    return cfg


def _run_one_pixel_de(cfg, models, classifiers, capture):
    """projector_based_attack.py:69-73,110-142: Nichols & Jasper's projector-based One-pixel DE attacker on one setup.  Per classifier
    one untargeted attack on the scene's top-1 (popsize 50) and ten targeted ones (popsize 10), pixel_size 41, 4 generations, one after
    another on numpy's global RNG stream as in the reference (the untargeted attack first; it is saved last, as img_0011).  Projector
    images go under prj/adv/One-pixel_DE/-/-/<classifier>/; captures of a real `capture` under cam/raw/adv/..., those of
    capture='model' under cam/infer/adv/... (they are inferred: the real ones are still made by projecting prj/adv).
    An optional cfg.maxiter replaces the reference's hard-coded 4 generations."""
    from .one_pixel_attacker import ProjectorOnePixelAttacker
    setup_name = _one_setup(cfg, 'One-pixel_DE: ')
    _check_capture(capture)
    _require_classifiers(cfg, classifiers)
    np.random.seed(0)   # (ut.reset_rng_seeds(0); DE draws from numpy's global state)
    random.seed(0)
    torch.manual_seed(0)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(0)
    setup = AttackSetup(cfg.data_root, setup_name)
    cam_scene = setup.cam_scene()
    cap, simulated = _resolve_capture(capture, 'run_projector_based_attack', models, setup, cam_scene)
    cam_adv = setup.cam_infer_adv if simulated else setup.cam_raw_adv
    imagenet_labels = setup.imagenet_labels()
    n = 10
    target_idx = setup.target_idx(n)
    one_pixel_de = ProjectorOnePixelAttacker(imagenet_labels, setup.info, capture=cap)
    im_prj_org = setup.info['prj_brightness'] * torch.ones(3, *setup.info['prj_im_sz'])
    one_pixel_de.im_prj_org, one_pixel_de.im_cam_org = im_prj_org, cam_scene
    attacker_cfg_str = to_attacker_cfg_str('One-pixel_DE')[0]
    attack = dict(pixel_count=1, pixel_size=41, maxiter=cfg.get('maxiter', 4), verbose=True)
    for stealth_loss, d_thr, classifier_name in itertools.product(cfg.stealth_losses, cfg.d_threshes, cfg.classifier_names):
        folder = (attacker_cfg_str, stealth_loss, d_thr, classifier_name)
        cam_path, prj_path = cam_adv(*folder), setup.prj_adv(*folder)
        classifier = classifiers[classifier_name]
        true_idx, p = _scene_top1(classifier, cam_scene, setup.crop_sz)
        true_label = imagenet_labels[true_idx]
        print(f'\n-------------------- [One-pixel_DE] attacking [{classifier_name}], original prediction: ({true_label}, '
              f'p={p.max():.2f}), Loss: [{stealth_loss}], d_thr: [{d_thr}] --------')
        print(f'[Untargeted] attacking [{classifier_name}]...')
        _, prj_untar, cam_untar = one_pixel_de(im_prj_org, classifier, False, target_idx=true_idx, popsize=50, true_label=true_label,
                                               **attack)
        for i in range(n):
            print(f'\n[ Targeted ] attacking [{classifier_name}], target: ({imagenet_labels[target_idx[i]]})...')
            _, prj_tar, cam_tar = one_pixel_de(im_prj_org, classifier, True, target_idx=target_idx[i], popsize=10, true_label=true_label,
                                               **attack)
            io.save_imgs(expand_4d(cam_tar), cam_path, idx=i)
            io.save_imgs(expand_4d(prj_tar), prj_path, idx=i)
        io.save_imgs(expand_4d(cam_untar), cam_path, idx=n)
        io.save_imgs(expand_4d(prj_untar), prj_path, idx=n)
    if simulated:
        print(f'\nThe next step is to project and capture [One-pixel_DE] generated adversarial projections in '
              f'{setup.prj_adv(attacker_cfg_str)}')
    else:
        print(f'\nThe next step is to inspect the camera-captured adversarial projections in {cam_adv(attacker_cfg_str)}')
    return cfg


def _run_square(cfg, models, classifiers, capture):
    """The Square Attack (spaa_amd.square_attack) on one setup, with One-pixel_DE's capture rules.  Per classifier the ten targeted
    attacks and the untargeted one on the scene's top-1 run as ONE batch of 11 samples (sample i draws the words of sample i).
    Projector images go under prj/adv/Square/-/-/<classifier>/ (1-10 targeted, 11 untargeted); captures of a real `capture` under
    cam/raw/adv/..., those of capture='model' under cam/infer/adv/...  cfg.square_eps8 is required (no default: see
    ProjectorSquareAttacker.attack); cfg.square_iters, cfg.square_proposals and an optional cfg.seed are handed on."""
    from .square_attack import ProjectorSquareAttacker
    setup_name = _one_setup(cfg, 'Square: ')
    _check_capture(capture)
    _require_classifiers(cfg, classifiers)
    if cfg.get('square_eps8') is None:
        raise ValueError('Square: set cfg.square_eps8, the L-infinity budget in 8-bit projector levels (1..127); it has no default')
    setup = AttackSetup(cfg.data_root, setup_name)
    cam_scene = setup.cam_scene()
    cap, simulated = _resolve_capture(capture, 'run_projector_based_attack', models, setup, cam_scene)
    cam_adv = setup.cam_infer_adv if simulated else setup.cam_raw_adv
    imagenet_labels = setup.imagenet_labels()
    n = 10
    target_idx = setup.target_idx(n)
    square = ProjectorSquareAttacker(imagenet_labels, setup.info, capture=cap)
    attacker_cfg_str = to_attacker_cfg_str('Square')[0]
    for stealth_loss, d_thr, classifier_name in itertools.product(cfg.stealth_losses, cfg.d_threshes, cfg.classifier_names):
        folder = (attacker_cfg_str, stealth_loss, d_thr, classifier_name)
        classifier = classifiers[classifier_name]
        true_idx, p = _scene_top1(classifier, cam_scene, setup.crop_sz)
        print(f'\n-------------------- [Square] attacking [{classifier_name}], original prediction: ({imagenet_labels[true_idx]}, '
              f'p={p.max():.2f}), eps8: [{cfg.square_eps8}] --------')
        prj, cam, info = square.attack(classifier, list(target_idx) + [true_idx], [True] * n + [False], eps8=cfg.square_eps8,
                                       n_iters=cfg.get('square_iters', 1000), proposals=cfg.get('square_proposals', 1),
                                       seed=cfg.get('seed', 0))
        print(f'success {info["success"].astype(int).tolist()}, queries {info["queries"].tolist()}')
        io.save_imgs(cam, cam_adv(*folder))
        io.save_imgs(prj, setup.prj_adv(*folder))
    if simulated:
        print(f'\nThe next step is to project and capture [Square] generated adversarial projections in {setup.prj_adv(attacker_cfg_str)}')
    else:
        print(f'\nThe next step is to inspect the camera-captured adversarial projections in {cam_adv(attacker_cfg_str)}')
    return cfg


def project_capture_real_attack(cfg, *, capture, models=None):
    """projector_based_attack.py:151-166 (steps 5.2 / 6.2 of the reference's main.py): project every adversarial image of
    <setup>/prj/adv/<attacker_cfg_str>/<loss>/<d_thr>/<classifier> and write its capture to the same folder under cam/raw/adv, as
    img_%04d.png counted in the sorted order of the projector images.  SPAA and PerC-AL+CompenNet++ only, and exactly one setup
    (ValueError otherwise; the reference asserts).  `capture` follows _run_one_pixel_de's convention: a function setup_info ->
    (im_prj uint8 [3,Hp,Wp] -> im_cam float [3,Hc,Wc]) for a real ProCams pair, or 'model': models[setup] (a trained PCNet) stands in
    for the projector and the camera through SimulatedCapture with the camera's 8-bit step.  A configured folder without projector
    images raises ValueError."""
    from .attack_summary import _nonempty
    name = cfg.attacker_name
    if name not in ('SPAA', 'PerC-AL+CompenNet++'):
        raise ValueError(f'{name} not supported, One-pixel_DE does not use this function!')
    setup_name = _one_setup(cfg)
    _check_capture(capture)
    setup = AttackSetup(cfg.data_root, setup_name)
    attacker_cfg_str = to_attacker_cfg_str(name)[0]
    folders = [(attacker_cfg_str, loss, d_thr, c) for loss in cfg.stealth_losses for d_thr in cfg.d_threshes
               for c in cfg.classifier_names]
    for folder in folders:
        if not _nonempty(setup.prj_adv(*folder)):
            raise ValueError(f'project_capture_real_attack: no projector images in {setup.prj_adv(*folder)}')
    cap, _ = _resolve_capture(capture, 'project_capture_real_attack', models, setup)
    for folder in folders:
        prj_path, cam_path = setup.prj_adv(*folder), setup.cam_raw_adv(*folder)
        for i, fn in enumerate(sorted(os.listdir(prj_path))):
            im_prj = torch.from_numpy(io._imread_rgb(join(prj_path, fn)).transpose(2, 0, 1).copy())
            io.save_imgs(expand_4d(cap(im_prj).detach().float()), cam_path, idx=i)
    print(f'\nThe camera-captured adversarial projections are in {setup.cam_raw_adv(attacker_cfg_str)}')
    return cfg
