"""Test-side oracle of the CompenNet++ training iteration (train_network.py:130-232): the oracle's forward passes
(oracle/spaa_oracle.py compennet_pp_forward / compennet_forward) and compute_loss under torch.autograd, one torch.optim.Adam
over all parameters and StepLR, on the CPU."""
import torch

import spaa_oracle as so
from spaa_amd import synthetic as syn

# the tensors whose full gradients and updated values the reference fixture keeps (tests/golden/make_golden_compennet_train.py)
PP_KEYS = ('warping_net.affine_mat', 'warping_net.theta', 'warping_net.grid_refine_net.0.weight', 'warping_net.grid_refine_net.6.bias',
           'compen_net.conv1_s.weight', 'compen_net.conv4_s.bias', 'compen_net.skipConv1.0.weight', 'compen_net.transConv2.weight',
           'compen_net.conv6.weight')
CN_KEYS = ('conv1.weight', 'conv1_s.weight', 'conv4_s.bias', 'skipConv1.0.weight', 'skipConv1.4.bias', 'transConv2.weight',
           'conv6.bias')


def pp_inputs(seed, it, bsz, cam_sz, prj_sz):
    """(camera batch, projector batch) of CompenNet++ iteration `it` of the fixture; its scene is syn.scenes(seed + 1, 1, cam_sz)."""
    return syn.scenes(seed + 20 + it, bsz, cam_sz), syn.scenes(seed + 30 + it, bsz, prj_sz) * 0.8 + 0.05


def cn_inputs(seed, bsz, prj_sz):
    """(scene, input batch, target batch) of the fixture's bare CompenNet iteration: input |prj - 0.3 s| as init_compennet builds it."""
    prj = syn.scenes(seed + 42, bsz, prj_sz) * 0.8 + 0.05
    s = syn.scenes(seed + 41, 1, prj_sz)
    return s, torch.abs(prj - 0.3 * s), prj


def compen_only(sd):
    """The bare CompenNet's state dict inside a CompenNet++ one."""
    return {k[len('compen_net.'):]: v.clone() for k, v in sd.items() if k.startswith('compen_net.')}


class CompenNetTrainOracle:
    """`sd` of a CompenNet++ (warping_net.* + compen_net.*, `out_size` = projector size) or of a bare CompenNet
    (`out_size` None).  `step(cam, prj, loss)` = model(cam, scene expanded to the batch) -> compute_loss -> backward ->
    Adam step -> StepLR step."""

    def __init__(self, sd, cam_scene, batch_size, out_size=None, lr=1e-3, l2_reg=1e-4, lr_drop_rate=800, lr_drop_ratio=0.2):
        self.out_size = tuple(out_size) if out_size is not None else None
        self.buffers = {k: v.clone() for k, v in sd.items() if k.endswith('ctrl_pts')}
        self.p = {k: v.clone().float().requires_grad_(True) for k, v in sd.items() if k not in self.buffers}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=lr, weight_decay=l2_reg)
        self.sched = torch.optim.lr_scheduler.StepLR(self.opt, step_size=lr_drop_rate, gamma=lr_drop_ratio)
        self.scene = so.expand_4d(cam_scene).expand(batch_size, -1, -1, -1)
        self.iters = 0

    def sd(self):
        d = dict(self.p)
        d.update(self.buffers)
        return d

    def forward(self, cam):
        if self.out_size is None:
            return so.compennet_forward(self.sd(), cam, self.scene, prefix='')
        return so.compennet_pp_forward(self.sd(), cam, self.scene, self.out_size)

    def lr(self):
        return self.opt.param_groups[0]['lr']

    def step(self, cam, prj, loss='l1+ssim'):
        infer = self.forward(cam)
        train_loss, l2 = so.compute_loss(infer, prj, loss)
        self.opt.zero_grad()
        train_loss.backward()
        self.grads = {k: v.grad.detach().clone() for k, v in self.p.items()}
        self.opt.step()
        self.sched.step()
        self.iters += 1
        return float(train_loss.detach()), float(l2.detach())
