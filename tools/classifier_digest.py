"""SHA-256 digests of what the classifier bodies compute in the configurations of tools/classifier_sequences.py, on seeded inputs: the
logits of a forward pass, the input gradient of the backward pass after it, and the logits of a forward pass with write_masks = False.
For a change that must keep the bodies' launches: run it on both commits on the same machine, every pair of lines must be identical
(same library, same launches, same arguments).

    python tools/classifier_digest.py [--root DIR]

--root: the checkout whose spaa_amd runs (default: this one).  Only what the recorder uses of a body is used here, so the tool runs on
both sides of such a change."""
import argparse
import hashlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import classifier_sequences as seq  # noqa: E402


NCLS = 12   # (the backward pass reads the logit gradient as a [B, 1, 1, classes] activation: channel quads)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(HERE))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from spaa_amd import _lib, classifier
    print(f'# spaa_amd from {os.path.dirname(os.path.abspath(classifier.__file__))}, library {_lib.load().spaa_version().decode()}')
    sds = {}
    for c in seq.CONFIGS:
        name, b, hw = seq.config_name(c), c['batch'], c['hw']
        sd = sds.setdefault(c['body'], seq.state_dict(c['body'], NCLS))
        gen = torch.Generator().manual_seed(11)
        x4 = torch.randn(b, hw, hw, 4, generator=gen)
        x4[..., 3] = 0
        x4, g = x4.cuda(), torch.randn(b, NCLS, generator=gen).cuda()
        with seq.switched(c['switches']):
            body = classifier.BODIES[c['body']](sd, b, (hw, hw), torch.device('cuda'), c['storage'])
            for k, v in c['live'].items():
                setattr(body, k, v)
            out = dict(logits=body.forward(x4).clone())
            out['g_in'] = body.backward(g).clone()
            body.write_masks = False
            out['logits_nomask'] = body.forward(x4).clone()
        torch.cuda.synchronize()
        assert all(torch.isfinite(v).all() for v in out.values()), name
        for k, v in out.items():
            print(f'{name:50s} {k:14s} {digest(v)}  max |.| {float(v.abs().max()):.3e}')
        del body
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
