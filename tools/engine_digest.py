"""SHA-256 digests of what PCNetEngine computes in the configurations of tests/test_pcnet_routes_gpu.py (seeded inputs): the output Y,
the gradients g['x'], g['P1'], g['P6'], every gate mask, the clamp-gate bytes and the sumsq partials.  For a change that must keep
the engine's launches: run it on both commits on the same machine, every pair of lines must be identical (same library, same
launches, same arguments).

    python tools/engine_digest.py [--root DIR] [--sequences OUT.json]

--root: the checkout whose spaa_amd runs (default: this one).  --sequences: also write the launch sequences of every configuration,
the fixture tests/golden/pcnet_launch_sequences.json (recorded ONCE, from the commit before such a change)."""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def digest(t):
    return 'none' if t is None else hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(HERE))
    ap.add_argument('--sequences', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
    sys.path.insert(0, os.path.abspath(args.root))
    import test_pcnet_routes_gpu as t
    from spaa_amd import _lib, convplan as cp, models as M
    _lib.load()
    print(f'# spaa_amd from {os.path.dirname(os.path.abspath(M.__file__))}, library {_lib.load().spaa_version().decode()}')
    sequences = {}
    for cfg in t.CONFIGS:
        name = t.config_name(cfg)
        _, eng = t.build_engine(M, cfg)
        part = t.run_passes(M, eng, cfg)
        torch.cuda.synchronize()
        out = dict(Y=dict.__getitem__(eng.a, 'Y'), gx=eng.g['x'], gP1=eng.g['P1'], gP6=eng.g['P6'], gate_y=eng.gate_y, sumsq=part)
        out.update({'m' + k: v for k, v in sorted(eng.m.items())})
        for k, v in out.items():
            print(f'{name:28s} {k:7s} {digest(v)}')
        if args.sequences:
            sequences[name] = t.record_sequences(M, _lib, cp, cfg)
    if args.sequences:
        with open(args.sequences, 'w') as fh:
            fh.write('{"sequences": {\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in sequences.items()) + '\n}}\n')


if __name__ == '__main__':
    main()
