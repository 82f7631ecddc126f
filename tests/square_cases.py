"""The cases the square tests share: the small geometries of tests/test_onepixel_projector_gpu.py, the network setup, the attack requests
of the route comparisons, and a cheap integer-valued `evaluate` on which exact ties, early successes and confident / unconfident
target hits all occur within a few iterations.  A helper, not a test module."""
import numpy as np

# projector size, camera size, affine (tests/test_onepixel_projector_gpu.py's GEOM)
GEOM = {'sq': ((64, 64), (64, 64), None), 'nonsq': ((64, 64), (48, 80), None),
        'outside': ((40, 56), (64, 64), (1.2, 0.02, 0.05, -0.03, 1.2, 0.05))}

# the networks of the route comparisons: synthetic PCNet and ResNet-18 (random weights: outcomes say only that the path runs)
NET = dict(pc_seed=0, sd_seed=2, logit_gain=20.0, scene_seed=1, prj_sz=(64, 64), cam_sz=(64, 64), crop=(60, 60), input_sz=(56, 56),
           brightness=0.5)
TARGETS = [204, 291, 340]      # targeted samples' classes; the untargeted samples take the scene's top-1

# Route comparisons: B = 3, about 12 iterations.  n_iters is far above the iterations run so that the squares stay large (h = 20 of 64
# at p_init 0.1, so that few squares miss the lit part of the scene and change nothing) and eps8 is large, which keeps the loss differences between candidates well above fp32 roundoff: the condition that at
# most 10 % of the decisions fall inside the loss bar is asserted on the float64 oracle alone in tests/test_square_cpu.py.
ROUTE_CASES = {
    'targeted_k1': dict(targeted=True, K=1, seed=20, eps8=64, n_iters=12000, p_init=0.1, iters=12),
    'targeted_k3': dict(targeted=True, K=3, seed=21, eps8=64, n_iters=12000, p_init=0.1, iters=12),
    'untargeted_k1': dict(targeted=False, K=1, seed=22, eps8=64, n_iters=12000, p_init=0.1, iters=12),
    'untargeted_k3': dict(targeted=False, K=3, seed=20, eps8=64, n_iters=12000, p_init=0.1, iters=12),
}
MAX_EXCLUDED = 0.10


class BlockEvaluate:
    """logits [ncls] = floor(A . (sums of the image over g x g blocks) / scale) as float64: integers, so that two candidates often tie
    exactly, and few enough classes that samples succeed early.  Calls are counted."""

    def __init__(self, seed, ncls, Hp, Wp, g=8, scale=40000):
        rng = np.random.default_rng(seed)
        self.g, self.scale, self.calls = g, scale, 0
        self.A = rng.integers(-4, 5, size=(ncls, (Hp // g) * (Wp // g) * 3))

    def __call__(self, im):
        self.calls += 1
        g = self.g
        H, W, _ = im.shape
        f = im[:H // g * g, :W // g * g].astype(np.int64).reshape(H // g, g, W // g, g, 3).sum(axis=(1, 3)).reshape(-1)
        return np.floor_divide(self.A @ f, self.scale).astype(np.float64)


SYNTH_NCLS = 6


def synth_requests():
    """(evaluate, keyword arguments of square_oracle.run) on BlockEvaluate, for the mutation and resting tests: three targeted samples
    and three untargeted ones whose label is the top-1 of their own stripes, so that they have to search; three seeds, and one request
    with p_init = 1, where the side reaches its upper clamp."""
    import square_oracle as so
    out = []
    for seed, p_init, n_iters, iters in ((1, 0.3, 40, 40), (2, 0.3, 40, 40), (3, 0.3, 40, 40), (4, 1.0, 10000, 3)):
        ev = BlockEvaluate(seed, SYNTH_NCLS, 32, 48)
        kw = dict(K=3, Hp=32, Wp=48, c0=127, eps8=100, n_iters=n_iters, p_init=p_init, p_thresh=0.9, seed=seed, iters=iters)
        own = [so.score(ev(so.stripes(seed, b, 127, 100, 32, 48)), 0, False)[1] for b in (3, 4, 5)]
        out.append((ev, dict(kw, labels=[0, 1, 2] + own, flags=[True] * 3 + [False] * 3)))
    return out
