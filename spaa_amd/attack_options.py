"""What an attack can be asked for besides the plain SPAA loop -- the option values CaptureJitter, PoseJitter, JpegCapture, CaptureBlur, Transfer and Universal (Attention is
spaa_amd.classifier's), the limits of include/spaa_hip.h -- and the check of a request, made before anything is allocated or launched:
`checked_request` for spaa() and spaa_sweep(), the `_supported` functions for the attack states that are built directly."""
import dataclasses
import math

import torch

from . import _lib
from .models import PCNet
from .classifier import Attention, Classifier

ENS_MAX = VIEWS_MAX = JITTER_MAX = 4   # SPAA_ENS_MAX, SPAA_VIEWS_MAX, SPAA_JITTER_MAX of include/spaa_hip.h
TRANSFER_RMAX = 7   # SPAA_TRANSFER_RMAX of include/spaa_hip.h
POSE_MAX_ROTATE, POSE_MAX_ZOOM, POSE_MAX_TILT, POSE_MAX_SHIFT = 10.0, 0.15, 0.1, 32.0


@dataclasses.dataclass(frozen=True)
class CaptureJitter:
    """What separates a real capture from the inferred one, as ranges of a random perturbation of the camera image (DESIGN.md,
    "Capture-robust attack"): exposure / white balance `gain` (per channel, 1 +- gain) and `offset` (+- offset), a misregistration of
    +- `shift` camera pixels per axis, sensor noise of standard deviation `noise`, the camera's 8-bit step (`quantize`).  `draws`:
    captures attacked at once per iteration (2..4; the first one is the clean capture), `seed`: of the counter-based generator.
    `shift` <= 2 and `noise` <= 0.1 are what the adjoint kernel's border loop and the tests' noise tolerance assume."""
    gain: float = 0.1
    offset: float = 0.03
    shift: float = 0.75
    noise: float = 0.01
    quantize: bool = True
    draws: int = 3
    seed: int = 0

    def __post_init__(self):
        if not 2 <= int(self.draws) <= JITTER_MAX:
            raise ValueError(f'CaptureJitter: draws must be 2..{JITTER_MAX}, got {self.draws}')
        for name in ('gain', 'offset', 'shift', 'noise'):
            if not float(getattr(self, name)) >= 0:
                raise ValueError(f'CaptureJitter: {name} must be >= 0, got {getattr(self, name)}')
        if self.gain >= 1:
            raise ValueError(f'CaptureJitter: gain must be < 1 (a channel gain stays positive), got {self.gain}')
        if self.shift > 2:
            raise ValueError(f'CaptureJitter: shift must be <= 2 camera pixels, got {self.shift}')
        if self.noise > 0.1:
            raise ValueError(f'CaptureJitter: noise must be <= 0.1, got {self.noise}')

    def draw(self, counter, jit, key, B, J, clean0):
        """spaa_jitter_draw of these ranges: fills jit [B][J][8] / key [B][J] for iteration counter[0] and advances the counter."""
        _lib.call('spaa_jitter_draw', int(self.seed) & 0xffffffff, _lib.ptr(counter), float(self.gain), float(self.offset),
                  float(self.shift), float(self.noise), int(bool(clean0)), _lib.ptr(jit), _lib.ptr(key), B, J)


@dataclasses.dataclass(frozen=True)
class PoseJitter:
    """A small change of camera pose after the setup was captured (the camera bumped, re-mounted, zoomed a little), as ranges of a
    random homography of the camera image: an in-plane rotation of +- `rotate` degrees, a scale of 1 +- `zoom`, a
    translation of +- `shift` camera pixels per axis and a tilt of +- `tilt` per axis, the relative change of the projective
    denominator from the image centre to the edge of the longer side.  What leaves the frame is not seen and what enters it is black.
    `draws`: warped copies attacked at once per iteration (2..4; the first one is the unwarped capture), `seed`: of the counter-based
    generator.  The defaults are a guess at "the camera was bumped", not a measurement.  `rotate` <= 10, `zoom` <= 0.15 and `tilt`
    <= 0.1 are what bounds the window of the adjoint kernel (spaa_pose_bwd); `shift` <= 32."""
    rotate: float = 2.0
    zoom: float = 0.03
    shift: float = 3.0
    tilt: float = 0.02
    draws: int = 3
    seed: int = 0

    def __post_init__(self):
        if not 2 <= int(self.draws) <= JITTER_MAX:
            raise ValueError(f'PoseJitter: draws must be 2..{JITTER_MAX}, got {self.draws}')
        for name, most in (('rotate', POSE_MAX_ROTATE), ('zoom', POSE_MAX_ZOOM), ('shift', POSE_MAX_SHIFT), ('tilt', POSE_MAX_TILT)):
            v = float(getattr(self, name))
            if not v >= 0:
                raise ValueError(f'PoseJitter: {name} must be >= 0, got {getattr(self, name)}')
            if v > most:
                raise ValueError(f'PoseJitter: {name} must be <= {most:g}, got {getattr(self, name)}')

    def draw(self, counter, table, B, J, H, W, clean0):
        """spaa_pose_draw of these ranges: fills table [B][J][8] for iteration counter[0] of an H x W image and advances the counter."""
        _lib.call('spaa_pose_draw', int(self.seed) & 0xffffffff, _lib.ptr(counter), float(self.rotate), float(self.zoom),
                  float(self.shift), float(self.tilt), int(bool(clean0)), _lib.ptr(table), B, J, H, W)


JPEG_SUBSAMPLINGS = {'4:4:4': 0, '4:2:0': 2}   # SPAA_JPEG_444, SPAA_JPEG_420 of include/spaa_hip.h
JPEG_GRADIENTS = ('soft', 'straight')


def jpeg_quality_range(quality, who='JpegCapture'):
    """(lo, hi) of a quality that is one integer or an ordered pair of integers, each in 1..100."""
    pair = tuple(quality) if isinstance(quality, (tuple, list)) else (quality, quality)
    if len(pair) != 2 or any(isinstance(q, bool) or not isinstance(q, int) for q in pair):
        raise ValueError(f'{who}: quality must be an integer or a pair of integers, got {quality!r}')
    if not 1 <= pair[0] <= pair[1] <= 100:
        raise ValueError(f'{who}: quality must be in 1..100 and an ordered pair (low, high), got {quality!r}')
    return pair


@dataclasses.dataclass(frozen=True)
class JpegCapture:
    """The camera's codec as the last thing that happens to a capture: a JPEG round trip at a `quality` drawn
    uniformly from the integers of the range (one integer: that quality), with `subsampling` '4:2:0' (phones, DSLRs) or '4:4:4'.
    `gradient`: what stands for the derivative of the coefficient rounding in the backward pass: 'soft' (3 r^2, r the rounding
    residue: it mutes the frequencies the codec deletes) or 'straight' (1).  `draws`: round trips attacked at once per iteration
    (2..4; the first one is the uncompressed capture), `seed`: of the counter-based generator."""
    quality: object = (60, 95)
    subsampling: str = '4:2:0'
    gradient: str = 'soft'
    draws: int = 3
    seed: int = 0

    def __post_init__(self):
        if not 2 <= int(self.draws) <= JITTER_MAX:
            raise ValueError(f'JpegCapture: draws must be 2..{JITTER_MAX}, got {self.draws}')
        jpeg_quality_range(self.quality)
        if isinstance(self.quality, list):
            object.__setattr__(self, 'quality', tuple(self.quality))   # (hashable)
        if self.subsampling not in JPEG_SUBSAMPLINGS:
            raise ValueError(f"JpegCapture: subsampling must be one of {', '.join(map(repr, JPEG_SUBSAMPLINGS))}, got {self.subsampling!r}")
        if self.gradient not in JPEG_GRADIENTS:
            raise ValueError(f"JpegCapture: gradient must be one of {', '.join(map(repr, JPEG_GRADIENTS))}, got {self.gradient!r}")

    @property
    def quality_range(self):
        return jpeg_quality_range(self.quality)

    def draw(self, counter, row, B, J, clean0):
        """spaa_jpeg_draw of this range: fills row [B][J][4] for iteration counter[0] and advances the counter."""
        lo, hi = self.quality_range
        _lib.call('spaa_jpeg_draw', int(self.seed) & 0xffffffff, _lib.ptr(counter), lo, hi, int(bool(clean0)), _lib.ptr(row), B, J)


BLUR_RMAX = 8          # SPAA_BLUR_RMAX of include/spaa_hip.h
BLUR_SIGMA_MAX = 2.5   # the largest sigma whose radius ceil(3 sigma) fits BLUR_RMAX


def blur_sigma_range(sigma, who='CaptureBlur'):
    """(lo, hi) of a sigma that is one number or an ordered pair of numbers, 0 <= lo <= hi <= BLUR_SIGMA_MAX."""
    pair = tuple(sigma) if isinstance(sigma, (tuple, list)) else (sigma, sigma)
    if len(pair) != 2 or any(isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) for s in pair):
        raise ValueError(f'{who}: sigma must be a finite number or a pair of finite numbers, got {sigma!r}')
    if not 0 <= pair[0] <= pair[1] <= BLUR_SIGMA_MAX:
        raise ValueError(f'{who}: sigma must be in 0..{BLUR_SIGMA_MAX:g} camera pixels (the radius ceil(3 sigma) is at most {BLUR_RMAX}) '
                         f'and an ordered pair (low, high), got {sigma!r}')
    return float(pair[0]), float(pair[1])


@dataclasses.dataclass(frozen=True)
class CaptureBlur:
    """The camera's lens out of focus: the capture convolved with a Gaussian of `sigma` camera pixels along both axes,
    the border replicated, sigma drawn uniformly from the range (one number: that sigma; radius ceil(3 sigma) <= BLUR_RMAX, so sigma
    <= BLUR_SIGMA_MAX).  `draws`: blurred copies attacked at once per iteration (2..4; the first one is the sharp capture), `seed`: of
    the counter-based generator.  The default range is a guess at "slightly out of focus", not a measurement.  A range that ends at 0
    is the plain attack and refused."""
    sigma: object = (0.5, 2.0)
    draws: int = 3
    seed: int = 0

    def __post_init__(self):
        if not 2 <= int(self.draws) <= JITTER_MAX:
            raise ValueError(f'CaptureBlur: draws must be 2..{JITTER_MAX}, got {self.draws}')
        _, hi = blur_sigma_range(self.sigma)
        if isinstance(self.sigma, list):
            object.__setattr__(self, 'sigma', tuple(self.sigma))   # (hashable)
        if hi == 0:
            raise ValueError('CaptureBlur(0): a sigma of 0 is no blur, the plain attack (pass blur=None)')

    @property
    def sigma_range(self):
        return blur_sigma_range(self.sigma)

    def draw(self, counter, rows, B, J, clean0):
        """spaa_blur_draw of this range: fills rows [B][J][12] for iteration counter[0] and advances the counter."""
        lo, hi = self.sigma_range
        _lib.call('spaa_blur_draw', int(self.seed) & 0xffffffff, _lib.ptr(counter), lo, hi, int(bool(clean0)), _lib.ptr(rows), B, J)


@dataclasses.dataclass(frozen=True)
class Transfer:
    """The transferable adversarial step: what a sample on the adversarial step follows is not the raw gradient image
    at the projector but m <- `momentum` m + t / |t|_1 (MI-FGSM), t the gradient image convolved with a Gaussian of `sigma` projector
    pixels (TI-FGSM; radius ceil(3 sigma) <= TRANSFER_RMAX, zero beyond the border).  momentum = 0: no accumulation; sigma = 0: no
    smoothing; both 0 is the plain attack and refused."""
    momentum: float = 1.0
    sigma: float = 0.0

    def __post_init__(self):
        for name in ('momentum', 'sigma'):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f'Transfer: {name} must be a finite number, got {v!r}')
        if not 0 <= self.momentum <= 1:
            raise ValueError(f'Transfer: momentum must be in [0, 1], got {self.momentum}')
        if self.sigma < 0:
            raise ValueError(f'Transfer: sigma must be >= 0, got {self.sigma}')
        if self.radius > TRANSFER_RMAX:
            raise ValueError(f'Transfer: sigma = {self.sigma} needs the radius ceil(3 sigma) = {self.radius}, at most {TRANSFER_RMAX} '
                             f'(sigma <= {TRANSFER_RMAX}/3)')
        if self.momentum == 0 and self.sigma == 0:
            raise ValueError('Transfer(0, 0): no momentum and no smoothing is the plain attack (pass transfer=None)')

    @property
    def radius(self):
        """r = ceil(3 sigma): the filter has 2 r + 1 taps per axis."""
        return int(math.ceil(3 * self.sigma))

    def weights(self):
        """The 2 r + 1 taps exp(-i^2 / (2 sigma^2)), i = -r .. r, normalised to sum 1 in float64 and then rounded: a float32 tensor
        ([1.0] for sigma = 0)."""
        r = self.radius
        if r == 0:
            return torch.ones(1, dtype=torch.float32)
        i = torch.arange(-r, r + 1, dtype=torch.float64)
        w = torch.exp(-i * i / (2.0 * float(self.sigma) ** 2))
        return (w / w.sum()).to(torch.float32)


UNIVERSAL_MAX = 64   # SPAA_UNIVERSAL_MAX of include/spaa_hip.h


@dataclasses.dataclass(frozen=True)
class Universal:
    """A universal projection: the batch is cut into groups of `size` consecutive samples, each with its own scene, and
    every group shares ONE projector image (2 <= size <= UNIVERSAL_MAX, the batch a multiple of it).  A group counts as fooled when
    ceil(`rate` * size) of its members are (`rate` in (0, 1]; 1: all of them, the multi-view rule with members in the place of views)."""
    size: int
    rate: float = 1.0

    def __post_init__(self):
        if isinstance(self.size, bool) or not isinstance(self.size, int):
            raise ValueError(f'Universal: size must be an integer, got {self.size!r}')
        if not 2 <= self.size <= UNIVERSAL_MAX:
            raise ValueError(f'Universal: size must be 2..{UNIVERSAL_MAX}, got {self.size}')
        r = self.rate
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(r) or not 0 < r <= 1:
            raise ValueError(f'Universal: rate must be in (0, 1], got {r!r}')

    @property
    def need(self):
        """The number of fooled members that makes a group fooled: ceil(rate * size) (a product that is an integer but for its
        rounding, as 0.3 * 10, is that integer)."""
        return min(self.size, max(1, int(math.ceil(float(self.rate) * self.size - 1e-9))))

    def groups(self, B, who='Universal'):
        """U = B / size, the number of groups of a batch of B samples."""
        if B < self.size or B % self.size:
            raise ValueError(f'{who}: a batch of {B} samples does not divide into groups of universal.size = {self.size}')
        return B // self.size

    def check_uniform(self, name, values, who='Universal'):
        """`values` (one per sample) must be equal within every group; the error names the first group that mixes them."""
        n = self.size
        for u in range(len(values) // n):
            row = values[u * n:(u + 1) * n]
            if any(v != row[0] for v in row):
                raise ValueError(f'{who}: {name} must be uniform within a universal group; group {u} (samples {u * n}..'
                                 f'{(u + 1) * n - 1}) holds {sorted(set(row), key=str)}')


def _unwrap(m):
    return m.module if hasattr(m, 'module') and not isinstance(m, (PCNet, Classifier)) else m


def _ensemble_members(classifier, storage, who):
    """The members of a list / tuple `classifier`, checked: each a spaa_amd.Classifier (no foreign-callable route for ensembles), at most
    ENS_MAX of them, no object twice, one number of classes; fp32 storage."""
    members = [_unwrap(c) for c in classifier]
    if not members:
        raise ValueError(f'{who}: the classifier sequence is empty')
    for c in members:
        if not isinstance(c, Classifier):
            raise TypeError(f'{who}: every member of a classifier ensemble must be a spaa_amd.Classifier, got {type(c).__name__} '
                            '(a foreign callable can only be attacked alone)')
    if len(members) > ENS_MAX:
        raise ValueError(f'{who}: an ensemble holds at most {ENS_MAX} classifiers, got {len(members)}')
    if len({id(c) for c in members}) != len(members):
        raise ValueError(f'{who}: the same Classifier object is listed twice in the ensemble')
    ncls = [c.num_classes for c in members]
    if any(n != ncls[0] for n in ncls):
        raise ValueError(f'{who}: the members of an ensemble must have the same number of classes, got {ncls}')
    if len(members) >= 2:
        _need_f32('for an ensemble', _OWN_SCALE.format('members'), storage, who)
    return members


def _view_pcnets(pcnet, cam_scene, who):
    """The views of a list / tuple `pcnet`, checked: each a spaa_amd.PCNet, 2 to VIEWS_MAX of them, no object twice, and `cam_scene` a
    list / tuple of as many scenes.  Returns (list of PCNets, list of scenes); a sequence of one PCNet is that PCNet: (PCNet, its
    scene)."""
    views = [_unwrap(m) for m in pcnet]
    for m in views:
        if not isinstance(m, PCNet):
            raise TypeError(f'{who}: every view must be a spaa_amd.PCNet, got {type(m).__name__} (the HIP path has no generic PCNet '
                            'fallback)')
    if not views:
        raise ValueError(f'{who}: the pcnet sequence is empty')
    if len(views) == 1:
        if isinstance(cam_scene, (list, tuple)):
            if len(cam_scene) != 1:
                raise ValueError(f'{who}: {len(cam_scene)} scenes for one view')
            cam_scene = cam_scene[0]
        return views[0], cam_scene
    if len(views) > VIEWS_MAX:
        raise ValueError(f'{who}: a multi-view attack holds at most {VIEWS_MAX} views, got {len(views)}')
    if len({id(m) for m in views}) != len(views):
        raise ValueError(f'{who}: the same PCNet object is listed twice among the views')
    if not isinstance(cam_scene, (list, tuple)) or len(cam_scene) != len(views):
        n = len(cam_scene) if isinstance(cam_scene, (list, tuple)) else 'one tensor'
        raise ValueError(f'{who}: cam_scene must be a list of one scene per view ({len(views)}), got {n}')
    return views, list(cam_scene)


# The refusals that the features share, each stated once; a feature's function below passes its own words.
_OWN_SCALE = "the {}' unit vectors need a loss scale of their own"


def _need_f32(where, why, storage, who):
    if storage != 'f32':
        raise NotImplementedError(f"{who}: storage={storage!r} is not implemented {where} ({why}); use storage='f32'")


def _need_classifier(attack, why, classifier, who, kinds=Classifier):   # (`classifier`: a Classifier, a checked list, or anything else)
    if not isinstance(classifier, kinds):
        raise TypeError(f'{who}: {attack} needs a spaa_amd.Classifier, got {type(classifier).__name__} ({why})')


def _need_one_of_each(what, short, pcnet, classifier, who):   # (draws: of one camera image, through one classifier)
    if isinstance(pcnet, list):
        raise NotImplementedError(f'{who}: {what} against several views is not implemented; attack one view with {short}')
    if isinstance(classifier, list):
        raise NotImplementedError(f'{who}: {what} against an ensemble of classifiers is not implemented; attack one classifier with '
                                  f'{short}')


def _no_focus(short, focus, who):
    if focus:
        raise ValueError(f'{who}: focus=True has no meaning with {short} (a sample must fool every draw of every iteration)')


def _is_a(value, name, kind, who, or_none=''):
    if not isinstance(value, kind):
        raise TypeError(f'{who}: {name} must be a spaa_amd.{kind.__name__}{or_none}, got {type(value).__name__}')


def _views_supported(views, classifier, storage, who):
    """What a multi-view attack does not serve.  `classifier`: as spaa() holds it after its own checks."""
    if isinstance(classifier, list):
        raise NotImplementedError(f'{who}: an ensemble of classifiers against several views is not implemented; attack one '
                                  'classifier from several views, or several classifiers from one')
    _need_classifier('a multi-view attack', 'a foreign callable can only be attacked from one view', classifier, who)
    _need_f32('for several views', _OWN_SCALE.format('views'), storage, who)
    sizes = [tuple(m.warping_net.out_size) for m in views]
    if any(sz != sizes[0] for sz in sizes):
        raise ValueError(f'{who}: the views must have the same camera size, got {sizes}')


def _jitter_supported(jitter, pcnet, classifier, storage, focus, who):
    """What a jitter attack does not serve.  `pcnet` / `classifier`: as spaa() holds them after its own checks."""
    _is_a(jitter, 'jitter', CaptureJitter, who)
    _need_one_of_each('capture jitter', 'jitter', pcnet, classifier, who)
    _need_classifier('a jitter attack', 'a foreign callable can only be attacked without jitter', classifier, who)
    _need_f32('with jitter', _OWN_SCALE.format('draws'), storage, who)
    _no_focus('jitter', focus, who)


def _pose_supported(pose, pcnet, classifier, storage, focus, attention, jitter, who):
    """What a pose attack does not serve.  `pcnet` / `classifier`: as spaa() holds them after its own checks; `jitter`: None or a checked
    CaptureJitter."""
    _is_a(pose, 'pose', PoseJitter, who)
    _need_one_of_each('pose jitter', 'pose', pcnet, classifier, who)
    _need_classifier('a pose attack', 'a foreign callable can only be attacked without pose', classifier, who)
    if attention is not None:
        raise NotImplementedError(f'{who}: attention together with pose jitter is not implemented (every draw would need a map of its '
                                  'own, pulled back through the warp); use attention or pose')
    _need_f32('with pose', _OWN_SCALE.format('draws'), storage, who)
    _no_focus('pose', focus, who)
    if jitter is not None and int(jitter.draws) != int(pose.draws):
        raise ValueError(f'{who}: pose and jitter are applied draw by draw and must name the same draws, got pose.draws = '
                         f'{pose.draws} and jitter.draws = {jitter.draws}')


def _jpeg_supported(jpeg, pcnet, classifier, storage, focus, attention, jitter, pose, who):
    """What a JPEG attack does not serve.  `pcnet` / `classifier`: as spaa() holds them after its own checks; `jitter` / `pose`: None or
    checked values."""
    _is_a(jpeg, 'jpeg', JpegCapture, who)
    _need_one_of_each('camera JPEG', 'jpeg', pcnet, classifier, who)
    _need_classifier('a JPEG attack', 'a foreign callable can only be attacked without jpeg', classifier, who)
    if attention is not None:
        raise NotImplementedError(f'{who}: attention together with camera JPEG is not implemented (every draw would need a map of its '
                                  'own, pulled back through the codec); use attention or jpeg')
    _need_f32('with jpeg', _OWN_SCALE.format('draws'), storage, who)
    _no_focus('jpeg', focus, who)
    for name, other in (('pose', pose), ('jitter', jitter)):
        if other is not None and int(other.draws) != int(jpeg.draws):
            raise ValueError(f'{who}: {name} and jpeg are applied draw by draw and must name the same draws, got {name}.draws = '
                             f'{other.draws} and jpeg.draws = {jpeg.draws}')


def _blur_supported(blur, pcnet, classifier, storage, focus, attention, jitter, pose, jpeg, universal, who):
    """What a blur attack does not serve.  `pcnet` / `classifier`: as spaa() holds them after its own checks; `jitter` / `pose` / `jpeg`:
    None or checked values; `universal`: None or what the caller passed."""
    _is_a(blur, 'blur', CaptureBlur, who)
    _need_one_of_each('lens blur', 'blur', pcnet, classifier, who)
    _need_classifier('a blur attack', 'a foreign callable can only be attacked without blur', classifier, who)
    if attention is not None:
        raise NotImplementedError(f'{who}: attention together with lens blur is not implemented (every draw would need a map of its '
                                  'own, pulled back through the blur); use attention or blur')
    _need_f32('with blur', _OWN_SCALE.format('draws'), storage, who)
    _no_focus('blur', focus, who)
    for name, other in (('pose', pose), ('jitter', jitter), ('jpeg', jpeg)):
        if other is not None and int(other.draws) != int(blur.draws):
            raise ValueError(f'{who}: {name} and blur are applied draw by draw and must name the same draws, got {name}.draws = '
                             f'{other.draws} and blur.draws = {blur.draws}')
    if universal is not None:
        raise NotImplementedError(f'{who}: universal together with blur is not implemented (the draws of a sample and the members '
                                  'of a group would need a rule of their own); use universal or blur')


def _attention_checked(attention, storage, who):
    """An attack state's own check of its `attention` (the entry points say more, earlier: _attention_supported)."""
    if attention is not None:
        _is_a(attention, 'attention', Attention, who, ' or None')
        _need_f32('with attention', 'the feature map and its gradient are read as fp32', storage, who)


def _attention_supported(attention, classifier, storage, jitter, who):
    """What an attention-weighted attack does not serve.  `classifier`: as spaa() holds it after its own checks.  A body without a
    feature map passes only with attention.rollout, where it has an attention rollout to offer instead."""
    _is_a(attention, 'attention', Attention, who, ' or None')
    if jitter is not None:
        raise NotImplementedError(f'{who}: attention together with capture jitter is not implemented (every draw would need a map of '
                                  'its own, pulled back through the jitter); use attention or jitter')
    _need_classifier('an attention-weighted attack', 'a foreign callable has no feature map to read', classifier, who, (Classifier, list))
    for c in classifier if isinstance(classifier, list) else [classifier]:
        if isinstance(c, Classifier) and not c.has_feature_map and not (attention.rollout and c.has_rollout):
            raise NotImplementedError(f'{who}: attention is not implemented for {c.name} (Grad-CAM needs a convolutional feature map, which '
                                      'this body does not have); attack it without attention=')
    _attention_checked(attention, storage, who)


def _transfer_checked(transfer, storage, who):
    """An attack state's own check of its `transfer` (the entry points say more, earlier: _transfer_supported)."""
    if transfer is not None:
        _is_a(transfer, 'transfer', Transfer, who, ' or None')
        _need_f32('with transfer', 'the momentum image and the smoothed gradient are fp32 and carry no loss scale', storage, who)


def _transfer_supported(transfer, classifier, storage, who):
    """What a transferable attack does not serve.  `classifier`: as spaa() holds it after its own checks."""
    _is_a(transfer, 'transfer', Transfer, who, ' or None')
    _need_classifier('a transferable attack', 'the route of a foreign callable steps inside torch.autograd, where the fused direction '
                     'kernels do not run', classifier, who, (Classifier, list))
    _transfer_checked(transfer, storage, who)


def _universal_supported(universal, pcnet, classifier, storage, jitter, pose, jpeg, who):
    """What a universal attack does not serve.  `pcnet` / `classifier`: as spaa() holds them after its own checks; `jitter` / `pose` /
    `jpeg`: None or checked values.  (`attention`, `transfer`, `focus` and every stealth-loss string combine with it.)"""
    _is_a(universal, 'universal', Universal, who, ' or None')
    _need_one_of_each('a universal projection', 'universal', pcnet, classifier, who)
    for name, other in (('jitter', jitter), ('pose', pose), ('jpeg', jpeg)):
        if other is not None:
            raise NotImplementedError(f'{who}: universal together with {name} is not implemented (the draws of a sample and the members '
                                      f'of a group would need a rule of their own); use universal or {name}')
    _need_classifier('a universal attack', 'a foreign callable can only be attacked scene by scene', classifier, who)
    _need_f32('for a universal projection', _OWN_SCALE.format('members'), storage, who)


def checked_request(who, pcnet, classifier, cam_scene, storage, focus, jitter, pose, attention, transfer, jpeg=None, universal=None,
                    blur=None):
    """The request of spaa() / spaa_sweep() (`who`), checked in the one order that decides which error a caller sees; returns the
    normalised (pcnet, classifier, cam_scene): unwrapped, a sequence of one collapsed, a list where there are several."""
    pcnet, classifier = _unwrap(pcnet), _unwrap(classifier)
    if isinstance(pcnet, (list, tuple)):
        pcnet, cam_scene = _view_pcnets(pcnet, cam_scene, who)
    if not isinstance(pcnet, (PCNet, list)):
        raise TypeError(f"{'spaa_amd.spaa' if who == 'spaa' else who} needs a spaa_amd.PCNet (the HIP path has no generic PCNet fallback)")
    if isinstance(classifier, (list, tuple)):
        classifier = _ensemble_members(classifier, storage, who)
        if len(classifier) == 1:
            classifier = classifier[0]
    if isinstance(pcnet, list):
        _views_supported(pcnet, classifier, storage, who)
    if jitter is not None:
        _jitter_supported(jitter, pcnet, classifier, storage, focus, who)
    if pose is not None:
        _pose_supported(pose, pcnet, classifier, storage, focus, attention, jitter, who)
    if jpeg is not None:
        _jpeg_supported(jpeg, pcnet, classifier, storage, focus, attention, jitter, pose, who)
    if blur is not None:
        _blur_supported(blur, pcnet, classifier, storage, focus, attention, jitter, pose, jpeg, universal, who)
    if attention is not None:
        _attention_supported(attention, classifier, storage, jitter, who)
    if transfer is not None:
        _transfer_supported(transfer, classifier, storage, who)
    if universal is not None:
        _universal_supported(universal, pcnet, classifier, storage, jitter, pose, jpeg, who)
    return pcnet, classifier, cam_scene
