"""SHA-256 digests of what the attack states compute in the configurations of tools/attack_sequences.py: after three eager iterations
x, x_best, every view's cam_best, state, stats, the extra trace tensors, the momentum image and the draw tables; the two return values
of one spaa() call with iters=6 and no trace (the captured-graph path; the line also says what LAST_RUN says); the return values of one
spaa_sweep() of two configs cut into two chunks (max_batch=2).  For a change that must keep the attack's results bit for bit: run it
on both commits on the same machine, every pair of lines must be identical.

    python tools/attack_digest.py [--root DIR]

--root: the checkout whose spaa_amd runs (default: this one)."""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from engine_digest import digest  # noqa: E402
import attack_sequences as S  # noqa: E402

TABLES = ('momentum', 'jit', 'key', 'table', 'counter', 'jitter_counter')


def flat(v):
    """The tensors of a return value (a tensor, or a list of one per view), in order."""
    return list(v) if isinstance(v, (list, tuple)) else [v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(HERE))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from spaa_amd import _lib, projector_based_attack as A
    print(f'# spaa_amd from {os.path.dirname(os.path.abspath(A.__file__))}, library {_lib.load().spaa_version().decode()}')
    world = S.World()

    def line(name, what, tensors):
        print(f'{name:20s} {what:16s} {" ".join(digest(t) for t in tensors)}', flush=True)

    for name, c in S.CONFIGS.items():
        st, targeted, d_thr = world.state(c)
        for _ in range(3):
            st.iteration(targeted, d_thr, S.ADV_LR, S.COL_LR, S.P_THRESH)
        torch.cuda.synchronize()
        line(name, 'x', [st.x])
        line(name, 'x_best', [st.x_best])
        line(name, 'cam_best', getattr(st, 'cam_bests', [st.cam_best]))
        line(name, 'trace_entry', st.trace_entry())
        for k in TABLES:
            if getattr(st, k, None) is not None:
                line(name, k, [getattr(st, k)])
        del st
        pc, clf, sc, loss, targeted, d_thr, kw = world.request(c)
        # (spaa() takes one stealth loss, one flag and one d_thr; the sweep below mixes them)
        cam, prj = A.spaa(pc, clf, None, S.TARGETS, True, sc, 5.0, S.LOSS, S.DEV, S.SETUP, iters=6, **kw)
        line(name, f'spaa {A.LAST_RUN["iterations"]} graph={A.LAST_RUN["graph"]}'.replace(' ', '_'), flat(cam) + [prj])
        cfgs = [(S.LOSS, 5.0, True, S.TARGETS[:2]), ('caml2', 9.0, False, S.TARGETS[2:])]
        res = A.spaa_sweep(pc, clf, None, sc, S.SETUP, S.DEV, cfgs, iters=6, max_batch=2, **kw)
        line(name, f'sweep2 graph={A.LAST_RUN["graph"]}', [t for cam, prj in res for t in flat(cam) + [prj]])


if __name__ == '__main__':
    main()
