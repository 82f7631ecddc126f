"""Wall time of the One-pixel DE attacker's fast route (spaa_amd/one_pixel_attacker.py) for the reference's two configurations,
with max_batch=1 (SciPy's one-candidate loop) and with the default (speculative batches of the population size).

    python tools/time_onepixel.py [--input-sz 224] [--repeat 2]

  demo       test_digital_one_pixel_attack.py: 256 x 256 image, crop 256, untargeted, pixel_size 5, popsize 50, maxiter 50
  projector  run_projector_based_attack (projector_based_attack.py:117-119): crop 240, targeted, pixel_size 41, popsize 10,
             maxiter 4

ResNet-18 with synthetic weights (no pretrained weights here).  Prints one JSON line per run: seconds, nfev, nit,
evaluations consumed per second, evaluated / nfev (speculation) and classified / nfev (what reached the GPU after the memo).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.classifier import Classifier  # noqa: E402
from spaa_amd.io import torch_imread  # noqa: E402
from spaa_amd.one_pixel_attacker import DigitalOnePixelAttacker  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--input-sz', type=int, default=224)
    ap.add_argument('--repeat', type=int, default=2)
    args = ap.parse_args()
    labels = {i: f'class{i}' for i in range(1000)}
    clf = Classifier('resnet18', 'cuda', state_dict=syn.resnet18_state_dict(5, logit_gain=20.0), sort_results=False,
                     input_sz=(args.input_sz, args.input_sz))
    fish = torch_imread(os.path.join(ROOT, 'tests', 'golden', 'anemone_fish.png'))
    scene = syn.scenes(3, 1, (256, 256))[0]
    top = int(clf(fish, (256, 256))[1][0].argmax())
    second = int(np.argsort(-clf(scene, (240, 240))[1][0])[1])
    configs = {
        'demo': (fish, (256, 256), dict(targeted_attack=False, target_idx=top, pixel_count=1, pixel_size=5, maxiter=50, popsize=50)),
        'projector': (scene, (240, 240), dict(targeted_attack=True, target_idx=second, pixel_count=1, pixel_size=41, maxiter=4,
                                              popsize=10)),
    }
    for name, (im, crop, kw) in configs.items():
        for mb in (1, None):
            att = DigitalOnePixelAttacker(labels, crop)
            for rep in range(args.repeat + 1):      # the first run builds the engines
                np.random.seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                att(im, clf, max_batch=mb, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                r = att.last_result
                if rep == 0:
                    continue
                print(json.dumps(dict(config=name, max_batch=mb if mb is not None else 'population', input_sz=args.input_sz,
                                      seconds=round(dt, 4), nfev=int(r.nfev), nit=int(r.nit),
                                      evals_per_s=round(r.nfev / dt, 1), evaluated_over_nfev=round(r.evaluated / r.nfev, 3),
                                      classified_over_nfev=round(r.classified / r.nfev, 3))), flush=True)


if __name__ == '__main__':
    main()
