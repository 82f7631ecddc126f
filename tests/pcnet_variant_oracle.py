"""Test-side restatement of the reference's PCNet training iteration for the ablation variants `train_eval_pcnet` builds by
name (/root/reference/src/python/train_network.py:476-595): no mask, no rough input (ShadingNetSPAA(use_rough=False), a
3-channel conv1_s), WarpingNet without the grid-refine net, and a frozen ShadingNet (fix_shading_net=True).  torch autograd and
torch.optim on the CPU on top of the oracle's forward (oracle/spaa_oracle.py): a ones mask stands for use_mask=False (x * 1 is
exact), the no-refine grid is the oracle's batch-1 grid without the refine net (models.py:175-178).  Shared by
tests/test_pcnet_variants_cpu.py, tests/test_pcnet_variants_gpu.py and tests/golden/make_golden_pcnet_variants.py."""
import torch

import spaa_oracle as so
from spaa_amd import synthetic as syn

# fixture name -> (use_mask, use_rough, with_refine, fix_shading_net, seed)
VARIANTS = {
    'no_mask_no_rough': (False, False, True, False, 11),
    'no_rough': (True, False, True, False, 12),
    'no_mask': (False, True, True, False, 13),
    'wo_refine': (True, True, False, False, 14),
    'fix_shading_net': (True, True, True, True, 15),
}
CAM_SZ, PRJ_SZ, BSZ = (48, 64), (64, 64), 3
LOSSES = ('l1+ssim', 'l1')
# gradients (and updated parameters) stored in full in the fixtures, where the variant has them; every gradient's norm is stored too
KEYS = ('warping_net.affine_mat', 'warping_net.theta', 'warping_net.grid_refine_net.6.bias', 'shading_net.conv6.weight',
        'shading_net.conv1_s.weight', 'shading_net.conv1_s.bias', 'shading_net.conv4_s.bias', 'shading_net.skipConv1.0.weight',
        'shading_net.transConv2.bias')


def fixture_name(variant):
    return 'pcnet_train_' + variant


def variant_sd(seed, use_mask, use_rough, with_refine, cam_sz=CAM_SZ):
    """syn.pcnet_state_dict shaped for the variant: conv1_s sliced to 3 input channels without the rough input (as the
    pcnet_norough_64 fixture does), no refine-net entries without the refine net, no `mask` buffer without the mask."""
    sd = syn.pcnet_state_dict(seed, cam_sz=cam_sz, mask='rect')
    if not use_rough:
        sd['shading_net.conv1_s.weight'] = sd['shading_net.conv1_s.weight'][:, :3].contiguous()
    if not with_refine:
        sd = {k: v for k, v in sd.items() if 'grid_refine_net' not in k}
    if not use_mask:
        del sd['mask']
    return sd


def inputs(seed, it, bsz=BSZ, cam_sz=CAM_SZ, prj_sz=PRJ_SZ):
    """(projector batch, camera batch) of iteration `it`; the scene is syn.scenes(seed + 1, 1, cam_sz)."""
    return syn.scenes(seed + 20 + it, bsz, prj_sz), syn.scenes(seed + 30 + it, bsz, cam_sz) * 0.8 + 0.05


class PCNetVariantOracle:
    """train_network.py:247-265 optimisers / schedulers and the :300-320 loop body for one variant.  Parameters of a frozen
    ShadingNet get no gradient, so torch.optim.Adam skips them; without the refine net its group is empty, as in the reference."""

    def __init__(self, sd, cam_scene, batch_size, use_mask=True, use_rough=True, with_refine=True, fix_shading_net=False,
                 l2_reg=1e-4, lr_drop_ratio=0.2, cam_sz=CAM_SZ):
        self.use_mask, self.use_rough, self.with_refine, self.fix = use_mask, use_rough, with_refine, fix_shading_net
        self.buffers = {k: v.clone() for k, v in sd.items() if k in ('mask', 'warping_net.ctrl_pts')}
        if not use_mask:
            self.buffers['mask'] = torch.ones(1, 1, *cam_sz)
        self.p = {k: v.clone().requires_grad_(not (fix_shading_net and 'warping_net' not in k))
                  for k, v in sd.items() if k not in self.buffers}
        aff = [self.p['warping_net.affine_mat'], self.p['warping_net.theta']]
        ref = [v for k, v in self.p.items() if 'warping_net.grid_refine_net' in k]
        shd = [v for k, v in self.p.items() if 'warping_net' not in k]
        self.opts = [torch.optim.Adam([{'params': aff}], lr=1e-2, weight_decay=0),
                     torch.optim.Adam([{'params': ref}], lr=5e-3, weight_decay=0),
                     torch.optim.Adam([{'params': shd}], lr=1e-3, weight_decay=l2_reg)]
        self.scheds = [torch.optim.lr_scheduler.MultiStepLR(o, milestones=[m], gamma=lr_drop_ratio)
                       for o, m in zip(self.opts, (100, 1200, 1800))]
        self.scene = so.expand_4d(cam_scene).expand(batch_size, -1, -1, -1)
        self.iters = 0

    def sd(self):
        d = dict(self.p)
        d.update(self.buffers)
        return d

    def forward(self, prj):
        # with the refine net: the literal per-batch grid; without it the oracle's batch-1 grid (its warping_fine_grid skips the
        # refine net when the state dict has none), expanded
        return so.pcnet_forward(self.sd(), prj, self.scene, per_batch_grid=self.with_refine, use_rough=self.use_rough)

    def step(self, prj, cam, loss=None):
        if loss is None:
            loss = 'l1' if self.iters <= 400 else 'l1+ssim'
        infer = self.forward(prj)
        train_loss, l2 = so.compute_loss(infer, cam, loss)
        for o in self.opts:
            o.zero_grad()
        train_loss.backward()
        self.grads = {k: v.grad.detach().clone() for k, v in self.p.items() if v.requires_grad}
        for o in self.opts:
            o.step()
        for s in self.scheds:
            s.step()
        self.iters += 1
        return float(train_loss.detach()), float(l2.detach())
