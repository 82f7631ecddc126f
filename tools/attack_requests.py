"""What spaa() and spaa_sweep() answer to every combination of their request arguments, without a GPU: `_attack_state` and
`_spaa_foreign_classifier` are replaced by stubs, so a request either passes every check ('ok') or raises; the exception's type name
and message are the outcome.  The order of the checks decides which error a caller sees: the full product pins it.

    python tools/attack_requests.py [--root DIR] --write OUT.json

writes the fixture tests/golden/attack_request_outcomes.json: the distinct outcomes once, and per caller one index per combination in
the order of `combinations()` (recorded ONCE, from the commit before a change that must keep the refusals;
tests/test_attack_requests_cpu.py compares).  --root: the checkout whose spaa_amd runs."""
import argparse
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SZ = (64, 64)
SETUP = dict(classifier_crop_sz=(60, 60), prj_brightness=0.5, prj_im_sz=SZ)
NUM_CLASSES = 16


def _foreign(im, cp):
    raise AssertionError('the foreign callable is never called')


def axes():
    """[(axis name, [(value name, value), ...]), ...] of the request arguments, built on the CPU."""
    from spaa_amd import synthetic as syn
    from spaa_amd import projector_based_attack as A
    from spaa_amd.models import PCNet, WarpingNet
    from spaa_amd.classifier import Classifier

    def pcnet():
        sd = syn.pcnet_state_dict(0, cam_sz=SZ)
        pc = PCNet(sd['mask'], WarpingNet(out_size=SZ))
        pc.load_state_dict(sd)
        return pc

    pc, pc2 = pcnet(), pcnet()
    csd = syn.resnet18_state_dict(2, num_classes=NUM_CLASSES)
    r18, r18b = (Classifier('resnet18', 'cpu', state_dict=csd, input_sz=(56, 56)) for _ in range(2))
    vit = Classifier('vit_b_16', 'cpu', input_sz=(32, 48), state_dict=syn.vit_b_16_state_dict(
        7, num_classes=NUM_CLASSES, dim=96, depth=2, mlp_dim=384, patch=8, input_sz=(32, 48)))
    return [('pcnet', [('one', pc), ('[one]', [pc]), ('[two]', [pc, pc2]), ('[same, same]', [pc, pc])]),
            ('classifier', [('one', r18), ('[two]', [r18, r18b]), ('foreign', _foreign), ('vit', vit), ('[same, same]', [r18, r18])]),
            ('storage', [('f32', 'f32'), ('f16', 'f16')]),
            ('focus', [('off', False), ('on', True)]),
            ('jitter', [('none', None), ('draws2', A.CaptureJitter(draws=2)), ('string', 'jitter')]),
            ('pose', [('none', None), ('draws2', A.PoseJitter(draws=2)), ('draws3', A.PoseJitter(draws=3))]),
            ('attention', [('none', None), ('0.25', A.Attention(0.25)), ('rollout', A.Attention(0.25, rollout=True))]),
            ('transfer', [('none', None), ('default', A.Transfer())])]


def combinations(ax):
    """(names, values) of every combination, the last axis fastest."""
    for combo in itertools.product(*[values for _, values in ax]):
        yield tuple(n for n, _ in combo), tuple(v for _, v in combo)


class _Passed:
    """What the stubbed `_attack_state` returns: a state whose results are empty images of the right count."""

    def __init__(self, pcnet, classifier, target_idx, *rest, **kw):
        self.n, self.views = len(target_idx), len(pcnet) if isinstance(pcnet, list) else 0

    def results(self):
        cam, prj = torch.zeros(self.n, 1), torch.zeros(self.n, 1)
        return ([cam] * self.views if self.views else cam), prj


def outcomes(A, ax=None):
    """{'spaa': [...], 'spaa_sweep': [...]}: per combination 'ok' or [exception type name, message]."""
    saved = A._attack_state, A._spaa_foreign_classifier
    A._attack_state, A._spaa_foreign_classifier = _Passed, lambda *a, **k: 'ok'
    sc = torch.zeros(3, *SZ)
    out = {'spaa': [], 'spaa_sweep': []}
    try:
        for _, (pcnet, classifier, storage, focus, jitter, pose, attention, transfer) in combinations(ax or axes()):
            scene = [sc] * len(pcnet) if isinstance(pcnet, list) and len(pcnet) > 1 else sc
            kw = dict(iters=0, storage=storage, focus=focus, jitter=jitter, pose=pose, attention=attention, transfer=transfer)
            for who, call in (('spaa', lambda: A.spaa(pcnet, classifier, None, [1, 2], True, scene, 5, 'caml2', 'cuda', SETUP, **kw)),
                              ('spaa_sweep', lambda: A.spaa_sweep(pcnet, classifier, None, scene, SETUP, 'cuda',
                                                                  [('caml2', 5, True, [1, 2])], **kw))):
                try:
                    call()
                    out[who].append('ok')
                except Exception as e:   # noqa: BLE001  (the outcome IS the exception)
                    out[who].append([type(e).__name__, str(e)])
    finally:
        A._attack_state, A._spaa_foreign_classifier = saved
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(HERE))
    ap.add_argument('--write', required=True, metavar='OUT.json')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from spaa_amd import projector_based_attack as A
    print(f'# spaa_amd from {os.path.dirname(os.path.abspath(A.__file__))}')
    ax = axes()
    got = outcomes(A, ax)
    distinct = {}
    index = {who: [distinct.setdefault(json.dumps(o), len(distinct)) for o in lst] for who, lst in got.items()}
    with open(args.write, 'w') as fh:
        fh.write('{"axes": ' + json.dumps([[name, [n for n, _ in values]] for name, values in ax]) + ',\n"outcomes": [\n'
                 + ',\n'.join(' ' + o for o in distinct) + '\n],\n'
                 + ',\n'.join(f'{json.dumps(who)}: {json.dumps(ix, separators=(",", ":"))}' for who, ix in index.items()) + '}\n')
    print(f'{len(index["spaa"])} combinations, {len(distinct)} distinct outcomes')


if __name__ == '__main__':
    main()
