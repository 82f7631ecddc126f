"""The inputs of tests/test_jpeg_ops_gpu.py, shared with the CPU test that checks their condition (tests/test_jpeg_cpu.py): B = 3 float
images per shape and number of draws, and planted quality rows that mix the identity row with Q = 1, 50, 75 and 100.  The seeds are
chosen so that the oracle alone leaves out at most MAX_UNSAFE_BLOCKS of the blocks of any round trip (tests/test_jpeg_cpu.py checks
it without a GPU).  A helper, not a test module."""
import numpy as np

import jpeg_oracle as jp

B = 3
DRAWS = (2, 3, 4)
# one block, one 4:2:0 MCU, padding on both axes, more than one 32 x 32 workgroup tile on one axis, and 2 x 3 tiles with padding
SHAPES = ((8, 8), (16, 16), (20, 28), (48, 80), (40, 72))
QUALITIES = (0, 1, 50, 75, 100)
MAX_UNSAFE_BLOCKS = 0.10
MAX_NEAR_PIXELS = 0.02
SEEDS = {((8, 8), 2): 4, ((8, 8), 3): 2, ((8, 8), 4): 35, ((16, 16), 3): 24, ((16, 16), 4): 44, ((20, 28), 2): 1, ((20, 28), 3): 4,
         ((20, 28), 4): 5}   # (every other case: 0)


def rows_for(J):
    """row float32 [B][J][4]: the five planted qualities in turn, draw 0 of sample 0 the identity row."""
    rows = np.zeros((B, J, 4), dtype=np.float32)
    rows[..., 0] = np.array([QUALITIES[(b * J + j) % 5] for b in range(B) for j in range(J)]).reshape(B, J)
    return rows


def inputs(hw, J):
    """(y float64 [B][H][W][3] of values that fp32 holds exactly: what the kernel is given, rows float32 [B][J][4])."""
    rng = np.random.default_rng(SEEDS.get((hw, J), 0))
    y = np.stack([jp.float_image(rng, *hw) for _ in range(B)])
    return y.astype(np.float32).astype(np.float64), rows_for(J)
