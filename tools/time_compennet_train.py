"""Milliseconds per CompenNet++ training step (CompenNetTrainer.step: forward, l1+ssim loss, backward, Adam) at the reference's
batch of 24, camera 240 x 320 -> projector 256 x 256, synthetic weights and images; device events around `--steps` steps after
`--warmup` steps.  Each step ends with the loss read-back the reference's loop also has (`.item()`)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spaa_amd import synthetic as syn  # noqa: E402
from spaa_amd.models import CompenNet, CompenNetPlusplus, WarpingNet  # noqa: E402
from spaa_amd.train_network import CompenNetTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=24)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=3)
args = ap.parse_args()
dev = 'cuda:0'
cam_sz, prj_sz, B = (240, 320), (256, 256), args.batch
model = CompenNetPlusplus(WarpingNet(out_size=prj_sz), CompenNet())
model.load_state_dict(syn.compennet_pp_state_dict(5, out_size=prj_sz))
model = model.to(dev)
tr = CompenNetTrainer(model, syn.scenes(1, 1, cam_sz), B, device=dev)
cam = syn.scenes(2, B, cam_sz).to(dev)
prj = syn.scenes(3, B, prj_sz).to(dev)
for _ in range(args.warmup):
    tr.step(cam, prj)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(args.steps):
    loss, _ = tr.step(cam, prj)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / args.steps
print(json.dumps(dict(what='compennet_pp_train_step', batch=B, cam=list(cam_sz), prj=list(prj_sz), steps=args.steps, ms_per_step=round(ms, 3),
                      last_loss=round(loss, 6))))
