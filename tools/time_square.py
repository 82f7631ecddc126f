"""Time of one iteration of the Square Attack's fast route (spaa_amd.square_attack.FastSquareState.step) at the reference geometry:
projector 256 x 256, camera 240 x 320, classifier crop 240, ResNet-18 at 224 with synthetic weights, B = 11 samples (the driver's
batch: ten targeted, one untargeted), K = 1 and K = 4 proposals.

    python tools/time_square.py [--iters 40] [--repeat 5] [--out profiles/square_time.jsonl]

  iteration     ms per step(): the host clock around `iters` steps that end in one synchronise (streamed), and with a synchronise
                after every step (synced: what a loop pays that reads the tables every iteration)
  evaluator     the yardstick: the One-pixel attacker's _CaptureEvaluator._run on the same number of rows (B K) -- the same warp +
                ShadingNet + preprocessing + classifier body, with its candidate upload and result download; this code is the same on
                the parent commit, so the two figures of one run compare an iteration with what the parent pays for as many captures
  entry_point   the five new entry points alone, from HIP events around each call (the _lib.PROFILE hook), per iteration

PCNet and classifier are random-init, so whether the attack succeeds says only that the path runs.  One JSON line per figure, appended
to --out as well."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from spaa_amd import _lib  # noqa: E402
from spaa_amd import one_pixel_attacker as opa  # noqa: E402
from spaa_amd import square_attack as sa  # noqa: E402
from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.classifier import Classifier  # noqa: E402
from spaa_amd.models import PCNet, WarpingNet  # noqa: E402

PRJ, CAM, CROP, TEN, B = (256, 256), (240, 320), (240, 240), [1, 7, 21, 207, 340, 745, 779, 846, 947, 950], 11


def clock(fn, n, sync_each):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'square_time.jsonl'))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    sd = syn.pcnet_state_dict(0, cam_sz=CAM, mask='rect')
    pc = PCNet(sd['mask'], WarpingNet(out_size=CAM))
    pc.load_state_dict(sd)
    pc = pc.to('cuda')
    clf = Classifier('resnet18', 'cuda', state_dict=syn.resnet18_state_dict(5, logit_gain=20.0), sort_results=False)
    scene = syn.scenes(3, 1, CAM)[0]
    cap = opa.SimulatedCapture(pc, scene)
    info = dict(prj_im_sz=PRJ, prj_brightness=0.5, cam_im_sz=CAM[::-1], classifier_crop_sz=CROP)
    att = sa.ProjectorSquareAttacker({i: f'class{i}' for i in range(1000)}, info, capture=cap)
    true_idx = int(clf(scene, CROP)[0][0].argmax())
    rng = np.random.default_rng(0)
    for K in (1, 4):
        rows = B * K
        # n_iters = 1000 x the most steps this tool can run on one state (it stays <= 10): the squares keep the first side,
        # h = round(sqrt(0.05 * 65536)) = 57, through the streamed, the synced and the profiled steps
        n_iters = 1000 * (3 + (2 * args.repeat + 1) * args.iters)
        st = att.state(clf, TEN + [true_idx], [True] * 10 + [False], eps8=16, n_iters=n_iters, proposals=K, seed=1)
        for _ in range(3):                       # the stripes and two iterations: engines built, code objects loaded
            st.step()
        ev = opa._CaptureEvaluator(cap, clf, 0.5 * torch.ones(3, *PRJ), CROP, 1, 41, TEN[0], True, rows, None)
        cand = np.stack([rng.integers(20, PRJ[0] - 20, rows), rng.integers(20, PRJ[1] - 20, rows), *(rng.integers(0, 256, rows) for _ in range(3))],
                        1).astype(np.int64)
        serial = iter(range(1 << 30))

        def evaluate():
            ev._run(cand, [b'%d:%d' % (next(serial), i) for i in range(rows)])
        for _ in range(3):
            evaluate()
        figures = {'streamed': [], 'synced': [], 'evaluator': []}
        for _ in range(args.repeat):             # the three alternate, so that a drift of the machine hits them alike
            figures['streamed'].append(clock(st.step, args.iters, False))
            figures['evaluator'].append(clock(evaluate, args.iters, False))
            figures['synced'].append(clock(st.step, args.iters, True))
        med = {k: statistics.median(v) for k, v in figures.items()}
        for k, v in figures.items():
            emit(kind='evaluator' if k == 'evaluator' else 'iteration', mode=k, B=B, K=K, rows=rows, h=st.h, median_ms=round(med[k], 4),
                 min_ms=round(min(v), 4), max_ms=round(max(v), 4), runs=len(v), steps_per_run=args.iters)
        emit(kind='gap', K=K, rows=rows, synced_over_evaluator=round(med['synced'] / med['evaluator'], 4),
             streamed_over_evaluator=round(med['streamed'] / med['evaluator'], 4))
        _lib.PROFILE = []
        for _ in range(args.iters):
            st.step()
        torch.cuda.synchronize()
        calls, _lib.PROFILE = _lib.PROFILE, None
        per = {}
        for name, e0, e1 in calls:
            per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
        new = {n: statistics.median(v) for n, v in per.items() if n.startswith('spaa_square_')}
        for n, us in new.items():
            emit(kind='entry_point', name=n, K=K, rows=rows, median_us=round(us, 2), calls=len(per[n]))
        emit(kind='entry_points_sum', K=K, rows=rows, new_us=round(sum(new.values()), 2),
             all_us=round(sum(statistics.median(v) * len(v) for v in per.values()) / args.iters, 2),
             done=int(st.state[:, 2].sum()), queries=st.state[:, 3].cpu().tolist())
        del st, ev
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
