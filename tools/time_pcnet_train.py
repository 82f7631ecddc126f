"""Milliseconds per PCNet training step (PCNetTrainer.step: forward, l1+ssim loss, backward, Adam) at the reference's batch of 24,
projector and camera 256 x 256, synthetic weights and images, for the models the paper's ablation compares
(reproduce_paper_results.py:64): `PCNet`, `PCNet_no_mask_no_rough`, and `PCNet_no_rough` with the batch-1 scene-only layers
(PCNetTrainer collapse=True) and without them (collapse=False).  Device events around `--steps` steps after `--warmup` steps;
each step ends with the loss read-back the reference's loop also has (`.item()`).  One JSON line per configuration.

    python tools/time_pcnet_train.py [--only PCNet_no_rough ...]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.models import PCNet, WarpingNet  # noqa: E402
from spaa_amd.train_network import PCNetTrainer  # noqa: E402

# name -> (use_mask, use_rough, collapse)
CONFIGS = {
    'PCNet': (True, True, None),
    'PCNet_no_mask_no_rough': (False, False, None),
    'PCNet_no_rough': (True, False, True),
    'PCNet_no_rough_batchB': (True, False, False),
}

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=24)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--only', nargs='*', default=None, choices=list(CONFIGS))
args = ap.parse_args()
dev = 'cuda:0'
sz, B = (256, 256), args.batch
prj = syn.scenes(2, B, sz).to(dev)
cam = (syn.scenes(3, B, sz) * 0.8 + 0.05).to(dev)
for name in args.only or CONFIGS:
    use_mask, use_rough, collapse = CONFIGS[name]
    sd = syn.pcnet_state_dict(5, cam_sz=sz, mask='rect')
    if not use_rough:
        sd['shading_net.conv1_s.weight'] = sd['shading_net.conv1_s.weight'][:, :3].contiguous()
    if not use_mask:
        del sd['mask']
    pc = PCNet(sd.get('mask'), WarpingNet(out_size=sz), use_mask=use_mask, use_rough=use_rough)
    pc.load_state_dict(sd)
    pc = pc.to(dev)
    tr = PCNetTrainer(pc, syn.scenes(1, 1, sz), B, device=dev, collapse=collapse)
    for _ in range(args.warmup):
        tr.step(prj, cam, 'l1+ssim')
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        loss, _ = tr.step(prj, cam, 'l1+ssim')
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    print(json.dumps(dict(what='pcnet_train_step', model=pc.name, config=name, collapse=tr.collapse, batch=B, size=list(sz),
                          steps=args.steps, ms_per_step=round(ms, 3), last_loss=round(loss, 6))), flush=True)
    del tr, pc
    torch.cuda.empty_cache()
