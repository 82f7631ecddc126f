"""spaa_amd — the SPAA attack loop (PCNet + frozen classifier + CIEDE2000/L2 stealth loss + alternating
normalised-gradient step) on hand-written HIP kernels for MI355X (gfx950).

Scope: the one hot path of BingyaoHuang/SPAA named in BASELINE.json (`spaa()` and what it calls), behind the
reference's own Python call signatures.  See DESIGN.md and INTEGRATION.md.
"""
from . import synthetic  # noqa: F401  (host-side data generation only)


def __getattr__(name):
    # Lazy: importing the package must not require the GPU library (CPU-side tests import `synthetic`/`convplan`).
    if name in ('PCNet', 'WarpingNet', 'ShadingNetSPAA', 'PCNetEngine'):
        from . import models
        return getattr(models, name)
    if name in ('Classifier', 'ClassifierEngine', 'load_imagenet_labels'):
        from . import classifier
        return getattr(classifier, name)
    if name in ('spaa', 'spaa_attack', 'AttackState', 'spaa_sweep', 'run_projector_based_attack', 'get_attacker_cfg',
                'to_attacker_cfg_str', 'summarize_single_attacker', 'summarize_all_attackers', 'project_capture_real_attack',
                'attack_results', 'EnsembleAttackState', 'MultiViewAttackState', 'attack_transfer', 'CaptureJitter', 'JitterAttackState',
                'capture_survival', 'Attention', 'Transfer', 'transfer_success', 'PoseJitter', 'PoseAttackState', 'pose_survival',
                'JpegCapture', 'JpegAttackState', 'jpeg_survival', 'jpeg_roundtrip', 'quant_tables', 'Universal',
                'CaptureBlur', 'BlurAttackState', 'blur_survival', 'gaussian_blur',
                'UniversalAttackState', 'universal_success'):
        from . import projector_based_attack
        return getattr(projector_based_attack, name)
    if name in ('rgb2lab_diff', 'ciede2000_diff', 'deltaE', 'stealth_loss_with_grad'):
        from . import differential_color_functions
        return getattr(differential_color_functions, name)
    if name in ('CompenNet', 'CompenNetPlusplus'):
        from . import models
        return getattr(models, name)
    if name in ('PerC_AL', 'perc_al_compennet_pp'):
        from . import perc_al
        return getattr(perc_al, name)
    if name in ('PCNetTrainer', 'train_pcnet', 'CompenNetTrainer', 'train_compennet_pp', 'init_compennet', 'evaluate_model', 'load_data',
                'get_model_train_cfg', 'train_eval_pcnet', 'train_eval_compennet_pp'):
        from . import train_network
        return getattr(train_network, name)
    if name in ('DigitalOnePixelAttacker', 'ProjectorOnePixelAttacker', 'SimulatedCapture', 'perturb_image'):
        from . import one_pixel_attacker
        return getattr(one_pixel_attacker, name)
    if name in ('ProjectorSquareAttacker',):
        from . import square_attack
        return getattr(square_attack, name)
    if name in ('calc_img_dists', 'img_stats', 'dists_from_sums'):
        from . import metrics
        return getattr(metrics, name)
    if name in ('threshold_im', 'get_affine_transform', 'center_crop', 'expand_4d', 'resize'):
        from . import img_proc
        return getattr(img_proc, name)
    if name in ('attack_montages', 'layout_labels', 'attack_texts', 'JET'):
        from . import montage
        return getattr(montage, name)
    if name in ('torch_imread', 'torch_imread_mt', 'save_imgs', 'load_setup_info', 'save_checkpoint'):
        from . import io
        return getattr(io, name)
    raise AttributeError(name)
