"""Generates tests/golden/convplan_launches.json: what every case of tests/test_convplan_launch_cpu.py launches, as computed by the
spaa_amd/convplan.py of the checked-out commit (recorded in the fixture's `commit` entry), plus the bf16 planes of one small seeded
weight for tests/test_convplan_cpu.py.  Needs the built library (the two host-side launcher-plan queries) and no GPU.

    python tests/golden/make_golden_convplan_launches.py

Run ONCE, before a change of convplan.py that must keep its behaviour; the test then pins the changed file to this record.
"""
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_convplan_launch_cpu as t  # noqa: E402
from spaa_amd import convplan as cp  # noqa: E402


class Patcher:
    """setattr with an undo list (what pytest's monkeypatch does inside the test)."""

    def __init__(self):
        self.undo = []

    def __call__(self, obj, name, value):
        self.undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def restore(self):
        for obj, name, value in reversed(self.undo):
            setattr(obj, name, value)
        self.undo = []


def plane_weight():
    return torch.randn(4, 32, generator=torch.Generator().manual_seed(11))


def save(fixture):
    """One case per line, keys sorted."""
    head = {k: v for k, v in fixture.items() if k != 'cases'}
    lines = [f' {json.dumps(k)}: {json.dumps(v, sort_keys=True)}' for k, v in sorted(fixture['cases'].items())]
    with open(t.GOLDEN, 'w') as fh:
        fh.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": {\n' + ',\n'.join(lines) + '\n}}\n')


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    commit = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=root, check=True, capture_output=True, text=True).stdout.strip()
    dirty = subprocess.run(['git', 'status', '--porcelain', 'spaa_amd/convplan.py'], cwd=root, check=True, capture_output=True, text=True).stdout.strip()
    assert not dirty, 'spaa_amd/convplan.py differs from the commit: the fixture records the committed file'
    patch, cases = Patcher(), {}
    for c in t.CASES:
        rec = t.compact(t.run_case(c, c['tune'], patch))
        patch.restore()
        rec['tune'] = c['tune']
        cases[c['name']] = rec
        d = [r['desc'] for r in rec['calls'] if 'desc' in r]
        print(f"{c['name']:32s}", [(x.get('tile', 0), x.get('ksplit', 0), x.get('reserved1', 0)) for x in d] or [r['entry'] for r in rec['calls']], rec.get('raises', ''))
    errors = {}
    for how in ('x6p', 'h16', '2src'):
        plan = t.build_plan(('conv2src', 64, 64, 64)) if how == '2src' else t.build_plan(('deconv', 64, 32, 3, 2, 1, how == 'h16'), attach=(how, 32))
        try:
            plan.refresh(torch.zeros(1))
        except RuntimeError as e:
            errors[how] = str(e)
    fixture = dict(commit=commit, cases=cases, refresh_second_source_error=errors,
                   planes=dict(seed=11, shape=[4, 32], int16=cp.split_planes(plane_weight()).tolist()))
    save(fixture)
    print('wrote', t.GOLDEN, os.path.getsize(t.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
