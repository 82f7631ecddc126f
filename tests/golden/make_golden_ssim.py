"""Generates tests/golden/ssim_stealth.npz by running the UNMODIFIED reference's pytorch_ssim._ssim(size_average=False) and its autograd
gradient on a few small image pairs (tests/ssim_oracle.py: inputs).  Runs only where the reference is at hand (imported via
oracle/ref_shims.py); the fixture it writes is data (inputs and expected outputs), not reference source.

    python tests/golden/make_golden_ssim.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_shims  # noqa: E402  (knows where the reference is)
import ssim_oracle as oracle  # noqa: E402

# (kind, H, W): below the radius, one window, a ragged rectangle, the cancellation case
CASES = (('textured', 3, 5), ('textured', 11, 11), ('planted', 13, 18), ('flat', 12, 12), ('equal', 9, 7))


def main():
    if not ref_shims.reference_available():
        raise RuntimeError('reference sources are not present')
    sys.path.insert(0, ref_shims.REF_ROOT)
    import pytorch_ssim   # (the package needs torch only: no stand-ins)
    window = pytorch_ssim.create_window(11, 3)
    out = {}
    for i, (kind, H, W) in enumerate(CASES):
        y, s = oracle.inputs(kind, H, W)
        yt = torch.from_numpy(y[..., :3].copy()).permute(2, 0, 1)[None].requires_grad_(True)
        st = torch.from_numpy(s[..., :3].copy()).permute(2, 0, 1)[None]
        val = pytorch_ssim._ssim(yt, st, window, 11, 3, size_average=False)
        g, = torch.autograd.grad((1 - val).sum(), yt)
        out[f'y{i}'], out[f's{i}'] = y, s
        out[f'ssim{i}'] = val.detach().numpy().astype(np.float32)
        out[f'grad{i}'] = g[0].permute(1, 2, 0).numpy().astype(np.float32)   # d (1 - SSIM) / d y, [H][W][3]
        print(f'{kind} {H}x{W}: ssim {float(val):.6f}, oracle {oracle.ssim(y, s):.6f}, '
              f'max |grad - oracle| {np.abs(out[f"grad{i}"] - oracle.grad(y, s)).max():.2e}')
    out['cases'] = np.array([f'{k}:{h}:{w}' for k, h, w in CASES])
    path = os.path.join(HERE, 'ssim_stealth.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    main()
