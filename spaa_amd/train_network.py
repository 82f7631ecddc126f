"""PCNet and CompenNet++ training on HIP.  First what the two trainers share (`_TrainedPlans`, `_GridTrainer`,
`_LossHead`, `_adam`), then PCNet (`PCNetTrainer`, `compute_loss`, `train_pcnet`: train_network.py:235-392), CompenNet++
(`CompenNetTrainer`, `evaluate_model`, `train_compennet_pp`, `init_compennet`: :98-232, :395-441) and the drivers in front of the
attack (`load_data`, `get_model_train_cfg`, `train_eval_pcnet`, `train_eval_compennet_pp`: :39-82, :444-733).

`PCNetTrainer` mirrors `train_pcnet` of the reference's train_network.py:235-363 and `compute_loss` :367-392: one iteration =
forward of PCNet (WarpingNet with its CURRENT parameters: the sampling grid is rebuilt every step, models.py:163-185) ->
l1 [+ (1 - SSIM)] loss -> gradients of all 44 parameter tensors -> three Adam optimisers (affine/TPS lr 1e-2, grid-refine
net lr 5e-3, ShadingNet lr 1e-3 with L2 weight decay `l2_reg`) with MultiStepLR(milestones 100 / 1200 / 1800, gamma
`lr_drop_ratio`) -> `l1` only for the first 400 iterations, then `l1+ssim` (:300-303).  `CompenNetTrainer`: see its docstring.

Everything arithmetic runs in libspaa_hip.so:
  PCNet forward / input gradients  PCNetEngine (tapconv kernels; the packed weights are refreshed on the device each step)
  CompenNet forward / backward     tapconv plans (_CompenNetEngine), spaa_batch_sum_gate, spaa_relu_gate; the warps: spaa_warp_fwd
  weight / bias gradients          spaa_tapconv_wgrad          (csrc/tapconv_wgrad.hip)
  loss + its gradient              spaa_train_loss_fwd_bwd     (csrc/color.hip), spaa_select_grad (clamp gate)
  grid (current parameters)        spaa_warp_coarse_grid, refine-net tapconv plans, spaa_warp_finish_grid
  grid / affine / TPS gradients    spaa_warp_bwd_grid (PCNet) or spaa_warp_bwd_grid2 (CompenNet++), spaa_warp_finish_grid_bwd,
                                   spaa_warp_coarse_grid_bwd   (csrc/train_ops.hip)
  optimiser                        spaa_adam_step
PyTorch supplies device memory and index plumbing (re-packing a changed parameter into the kernels' layout through
precomputed index maps).  No CPU fallback.
"""
import math
import os
import random

import torch

from . import _lib
from . import convplan as cp
from .models import PCNet, PCNetEngine, to_nhwc4, to_nchw, C_ptr, transposed_taps

# ShadingNet's convolutions, module name -> (stride, padding), as PCNetEngine builds them (models.py); transConv1 / 2 and skipConv1 apart
_SHADING = {
    'conv1': (2, 1), 'conv2': (2, 1), 'conv3': (1, 1), 'conv4': (1, 1), 'conv5': (1, 1), 'conv1_s': (2, 1),
    'conv2_s': (2, 1), 'conv3_s': (1, 1), 'conv4_s': (1, 1), 'conv6': (1, 1), 'skipConv3': (1, 1), 'skipConv2': (1, 0)}


def _zeros(dev):
    return lambda *shape: torch.zeros(*shape, device=dev)


def _window(window_size=11, sigma=1.5):
    g = torch.Tensor([math.exp(-(i - window_size // 2) ** 2 / float(2 * sigma ** 2)) for i in range(window_size)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().reshape(-1).contiguous()


# ================================================================================================================
# What the two trainers share: trained plans, the WarpingNet's grid, the loss head, Adam
# ================================================================================================================
class _TrainedPlans:
    """The plans whose packed weights follow the parameters: `refresh()` re-packs each on the device from its parameter."""

    def __init__(self, dev):
        self.dev, self.maps = dev, []   # maps: (plan, weight parameter, bias parameter or None)

    def reg(self, plan, builder, mod, with_bias):
        cp.attach_maps(plan, builder, mod.weight.detach().cpu())
        self.maps.append((plan, mod.weight, mod.bias if with_bias else None))
        return plan

    def wg_plan(self, mod, builder):
        """A plan used for its geometry only (taps, classes, packing layout): tap list on the device, unpack map attached."""
        w = mod.weight.detach().cpu()
        pl = builder(w)
        pl.weights, pl.taps, pl.w_split = pl.weights.to(self.dev), pl.taps.to(self.dev), None
        cp.attach_maps(pl, builder, w)
        return pl

    def dgrad(self, mod, deconv, st, pad, name):
        """The registered input-gradient plan of one trained convolution (`deconv`: a transposed one)."""
        bwd = cp.deconv_dgrad_plan if deconv else cp.conv_dgrad_plan
        return self.reg(bwd(mod.weight, st, pad, self.dev, name), lambda w: bwd(w, st, pad, 'cpu'), mod, False)

    def layer(self, mod, deconv, st, pad, names, dgrad=True):
        """(forward, input-gradient, weight-gradient) plans of one trained convolution, the first two registered and named `names`.
        A transposed convolution's weight-gradient plan is unfolded (one weight matrix per output-parity class); without `dgrad`
        there is no input-gradient plan (None)."""
        fwd, unfold = (cp.deconv_fwd_plan, dict(fold=False)) if deconv else (cp.conv_fwd_plan, {})
        f = self.reg(fwd(mod.weight, mod.bias, st, pad, self.dev, names[0]), lambda w: fwd(w, None, st, pad, 'cpu'), mod, True)
        wg = self.wg_plan(mod, lambda w: fwd(w, None, st, pad, 'cpu', **unfold))
        return f, self.dgrad(mod, deconv, st, pad, names[1]) if dgrad else None, wg

    def refresh(self):
        for plan, w, b in self.maps:
            plan.refresh(w, b)


class _GridTrainer:
    """The WarpingNet's sampling grid under training: `forward()` builds it from the CURRENT parameters (models.py:168-178) and keeps
    every intermediate; `backward(grads)` turns the gradient w.r.t. the fine grid (`ws['g_fine']`, filled by the caller's own warp
    kernel) into the gradients of the grid-refine net, `affine_mat` and `theta`.  `src_size`: the size of the images the grid samples
    (PCNet: the projector's; CompenNet++: the camera's).  Without the grid-refine net (`with_refine=False`) there are no refine plans."""

    def __init__(self, wn, src_size, plans, dev):
        self.wn, self.src_size = wn, tuple(src_size)
        H, W = self.out_size = wn.out_size
        z = _zeros(dev)
        ncol = 6 + 2 * (wn.nctrl + 2)
        self.ws = dict(coarse=z(1, H, W, 4), fine=z(H, W, 4), g_fine=z(H, W, 4), g_sum=z(1, H, W, 4),
                       partial=z(((H * W + 255) // 256) * ncol), g_params=z(ncol))
        self.rf, self.rd, self.rwg = {}, {}, {}
        if not wn.with_refine:
            return
        # grid-refine net (models.py:123-134): two convolutions, two transposed convolutions
        for i, deconv, pad in ((0, False, 1), (2, False, 1), (4, True, 0), (6, True, 0)):
            self.rf[i], self.rd[i], self.rwg[i] = plans.layer(wn.grid_refine_net[i], deconv, 2, pad, (f'refine{i}', f'refine{i}_dgrad'))
        self.ws.update(r0=z(1, H // 2, W // 2, 32), r2=z(1, H // 4, W // 4, 64), r4=z(1, H // 2, W // 2, 32), refine=z(1, H, W, 4),
                       g_r6=z(1, H, W, 4), g_r4=z(1, H // 2, W // 2, 32), g_r2=z(1, H // 4, W // 4, 64),
                       g_r0=z(1, H // 2, W // 2, 32), g_c0=z(1, H, W, 4))

    def forward(self):
        """The fine grid [H,W,4] (models.py:168-178 with the current parameters)."""
        p, wn, ws = _lib.ptr, self.wn, self.ws
        (hi, wi), (H, W) = self.src_size, self.out_size
        self._aff = wn.affine_mat.detach().float().contiguous().view(-1)
        self._theta = wn.theta.detach().float().contiguous().view(-1)
        self._ctrl = wn.ctrl_pts.detach().float().contiguous().view(-1)
        _lib.call('spaa_warp_coarse_grid', p(self._aff), p(self._theta), p(self._ctrl), wn.nctrl, hi, wi, H, W, p(ws['coarse']))
        if self.rf:
            R, L = _lib.ACT_RELU, _lib.ACT_LEAKY01
            self.rf[0].run(ws['coarse'], ws['r0'], act=R)
            self.rf[2].run(ws['r0'], ws['r2'], act=R)
            self.rf[4].run(ws['r2'], ws['r4'], act=R)
            self.rf[6].run(ws['r4'], ws['refine'], act=L)
        _lib.call('spaa_warp_finish_grid', p(ws['coarse']), p(ws.get('refine')), p(ws['fine']), H * W)
        return ws['fine']

    def backward(self, grads):
        p, wn, ws = _lib.ptr, self.wn, self.ws
        (hi, wi), (H, W) = self.src_size, self.out_size
        _lib.call('spaa_warp_finish_grid_bwd', p(ws['g_fine']), p(ws['coarse']), p(ws.get('refine')), p(ws['g_sum']),
                  p(ws.get('g_r6')), H * W)
        g_coarse = ws['g_sum']   # (without the refine net the coarse grid is the fine grid before the clamp)
        if self.rf:
            wp = 'warping_net.grid_refine_net.'

            def rwgrad(i, inp, gout):
                dw, db = self.rwg[i].wgrad(inp, gout)
                grads[wp + f'{i}.weight'] = self.rwg[i].unpack_grad(dw)
                grads[wp + f'{i}.bias'] = db

            rwgrad(6, ws['r4'], ws['g_r6'])
            self.rd[6].run(ws['g_r6'], ws['g_r4'], gate=ws['r4'])
            rwgrad(4, ws['r2'], ws['g_r4'])
            self.rd[4].run(ws['g_r4'], ws['g_r2'], gate=ws['r2'])
            rwgrad(2, ws['r0'], ws['g_r2'])
            self.rd[2].run(ws['g_r2'], ws['g_r0'], gate=ws['r0'])
            rwgrad(0, ws['coarse'], ws['g_r0'])
            self.rd[0].run(ws['g_r0'], ws['g_c0'], add=ws['g_sum'])               # + the skip connection (models.py:176)
            g_coarse = ws['g_c0']
        _lib.call('spaa_warp_coarse_grid_bwd', p(g_coarse), p(self._aff), p(self._theta), p(self._ctrl), wn.nctrl, hi, wi, H, W,
                  p(ws['partial']), p(ws['g_params']))
        grads['warping_net.affine_mat'] = ws['g_params'][:6].view(1, 2, 3)
        grads['warping_net.theta'] = ws['g_params'][6:].view(1, wn.nctrl + 2, 2)


class _LossHead:
    """compute_loss (train_network.py:367-392) and its gradient as one launch of spaa_train_loss_fwd_bwd, workspaces kept across steps.
    `gate`: also the workspace of the output layer's clamp / ReLU gate (the trainers; `compute_loss` takes the values alone)."""

    def __init__(self, B, H, W, dev, gate=True):
        z = _zeros(dev)
        self.B, self.H, self.W = B, H, W
        self.window = _window().to(dev)
        nblk = ((H + 15) // 16) * ((W + 15) // 16)
        self.ws = dict(mmu=z(B, H, W, 4), m11=z(B, H, W, 4), m12=z(B, H, W, 4), partial=z(B * nblk, 3), gY=z(B, H, W, 4))
        if gate:
            self.ws['gP'] = z(B, H, W, 4)
            self.ones_state = torch.ones(B, 4, dtype=torch.int32, device=dev)

    def launch(self, y4, t4, l1_w, ssim_w):
        p, ws = _lib.ptr, self.ws
        _lib.call('spaa_train_loss_fwd_bwd', p(y4), p(t4), p(self.window), l1_w, ssim_w, p(ws['mmu']), p(ws['m11']), p(ws['m12']),
                  p(ws['partial']), p(ws['gY']), self.B, self.H, self.W)

    def grad(self, y4, t4, ypre, loss):
        """The loss `loss` of the inferred image y4 against t4; returns its gradient w.r.t. the output layer's pre-activation
        (`ypre`: relu of it, the clamp / ReLU gate)."""
        p, ws = _lib.ptr, self.ws
        self.launch(y4, t4, 1.0 if 'l1' in loss else 0.0, 1.0 if 'ssim' in loss else 0.0)
        _lib.call('spaa_select_grad', p(ws['gY']), p(ws['gY']), p(self.ones_state), p(ypre), p(ws['gP']), self.B, self.H * self.W)
        return ws['gP']

    def value(self, loss):
        """(loss value, l2 (MSE) value) of the last `grad` as Python floats: the one host sync of a step."""
        part = self.ws['partial'].sum(dim=0).cpu()
        n_el = 3.0 * self.B * self.H * self.W
        l1_w, ssim_w = (1.0 if 'l1' in loss else 0.0), (1.0 if 'ssim' in loss else 0.0)
        l1, l2 = float(part[1]) / n_el, float(part[2]) / n_el
        return l1_w * l1 + ssim_w * (1.0 - float(part[0]) / n_el), l2


def _adam(params, grads, m, v, names, lr, wd, t):
    """Step `t` of torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, L2 weight decay `wd`) on the parameters `names`."""
    p = _lib.ptr
    for n in names:
        prm = params[n]
        gt = grads[n].contiguous()
        assert gt.numel() == prm.numel(), n
        _lib.call('spaa_adam_step', p(prm.data.view(-1)), p(gt.view(-1)), p(m[n].view(-1)), p(v[n].view(-1)), prm.numel(), lr, 0.9,
                  0.999, 1e-8, wd, t)


# ================================================================================================================
# PCNet training (train_network.py:235-363)
# ================================================================================================================
class PCNetTrainer:
    """State of one PCNet training run: engine, per-parameter Adam moments, schedules.  `step(prj_batch, cam_batch)` is one
    iteration of the reference's loop body (train_network.py:293-357).

    Every model `train_eval_pcnet` builds by name (:476-595) trains: `use_mask` (no mask: the warped image is not masked),
    `use_rough` (False: ShadingNetSPAA(use_rough=False), the surface branch sees the scene alone), WarpingNet `with_refine`
    (False: no grid-refine net, its Adam group is empty) and `fix_shading_net` (the ShadingNet's parameters have
    requires_grad=False: no weight gradients, no Adam step, their values stay as they are).

    `collapse`: the layers that see only the scene (skipConv1 and, with use_rough=False, conv1_s .. conv4_s) run once, at batch 1
    -- the scene is one image expanded to the batch (:245) -- their outputs are broadcast into the batch-B residual inputs, and
    their gradients start from the batch sum of the cotangents they feed (spaa_batch_sum_gate_bits).  The default (None) is on for
    every variant and off for the SPAA configuration (mask, rough input, refine net, trainable ShadingNet), whose step stays the
    batch-B one."""

    def __init__(self, pcnet, cam_scene, batch_size, l2_reg=1e-4, lr_drop_ratio=0.2, device='cuda', collapse=None):
        if not isinstance(pcnet, PCNet):
            raise TypeError('PCNetTrainer needs a spaa_amd.PCNet')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('spaa_amd training runs on the GPU only (no CPU fallback)')
        self.dev, self.pc, self.B = dev, pcnet, batch_size
        self.l2_reg, self.gamma = float(l2_reg), float(lr_drop_ratio)
        wn, sn = pcnet.warping_net, pcnet.shading_net
        if wn.theta.shape[1] != wn.nctrl + 2:
            raise NotImplementedError('training covers the reduced TPS form (T + 2 parameters) the reference uses')
        self.refine, self.rough, self.use_mask = bool(wn.with_refine), bool(pcnet.use_rough), bool(pcnet.use_mask)
        self.fix_shading = not any(prm.requires_grad for prm in sn.parameters())     # PCNet(fix_shading_net=True)
        spaa_cfg = self.refine and self.rough and self.use_mask and not self.fix_shading
        self.collapse = (not spaa_cfg) if collapse is None else bool(collapse)
        with _lib.on_device(dev):
            s = cam_scene.detach().float().to(dev)
            while s.ndim < 4:
                s = s[None]
            self.scene1 = to_nhwc4(s[:1].contiguous())
            self.scene4 = to_nhwc4(s.expand(batch_size, -1, -1, -1).contiguous())
            self.Hc, self.Wc = wn.out_size
            self.loss = _LossHead(batch_size, self.Hc, self.Wc, dev)
            # parameter groups of train_network.py:247-256 (a frozen ShadingNet: torch.optim.Adam skips parameters without a gradient)
            self.params = dict(pcnet.named_parameters())
            self.groups = {
                'w1': dict(names=['warping_net.affine_mat', 'warping_net.theta'], lr=1e-2, wd=0.0, milestone=100),
                'w2': dict(names=[n for n in self.params if 'warping_net.grid_refine_net' in n], lr=5e-3, wd=0.0, milestone=1200),
                's': dict(names=[] if self.fix_shading else [n for n in self.params if 'warping_net' not in n], lr=1e-3,
                          wd=self.l2_reg, milestone=1800)}
            trained = [n for g in self.groups.values() for n in g['names']]
            self.m = {n: torch.zeros_like(self.params[n], device=dev) for n in trained}
            self.v = {n: torch.zeros_like(self.params[n], device=dev) for n in trained}
        self.grads = {}
        self.eng = None   # created at the first step (needs the projector size)
        self.iters = 0

    # ------------------------------------------------------------------------------------------------------------
    def _make_engine(self, prj_size):
        """PCNetEngine + index maps to refresh its packed weights, wgrad plans (unfolded geometry), the WarpingNet's grid."""
        sn, dev = self.pc.shading_net, self.dev
        eng = PCNetEngine(self.pc, self.B, prj_size, fuse_skip2=False, fuse_tail=False)   # (the weight gradients of conv6 / transConv2 read X7 and its gradient)
        plans = self.plans = _TrainedPlans(dev)

        def layers():
            """(plan name, module, forward builder, input-gradient builder of eng.d's plan or None, weight-gradient builder: its plan matters
            for its geometry only, a transposed convolution's is unfolded) of every ShadingNet layer as PCNetEngine builds it (models.py)."""
            for nm, (st, pad) in _SHADING.items():
                fb = (lambda w, st=st, pad=pad: cp.conv_fwd_plan(w, None, st, pad, 'cpu'))
                in_ch = (3, 6) if nm == 'conv1_s' else None
                db = (lambda w, st=st, pad=pad, in_ch=in_ch: cp.conv_dgrad_plan(w, st, pad, 'cpu', in_ch=in_ch))
                yield nm, getattr(sn, nm), fb, db if nm in eng.d else None, fb
            for nm, pad in (('transConv1', 1), ('transConv2', 0)):
                yield (nm, getattr(sn, nm), lambda w, pad=pad: cp.deconv_fwd_plan(w, None, 2, pad, 'cpu'),
                       lambda w, pad=pad: cp.deconv_dgrad_plan(w, 2, pad, 'cpu'),
                       lambda w, pad=pad: cp.deconv_fwd_plan(w, None, 2, pad, 'cpu', fold=False))
            for nm, i, pad in (('skip1a', 0, 0), ('skip1b', 2, 1), ('skip1c', 4, 1)):
                fb = (lambda w, pad=pad: cp.conv_fwd_plan(w, None, 1, pad, 'cpu'))
                yield nm, sn.skipConv1[i], fb, None, fb

        self.wg, self.skip_d, self.sd = {}, {}, {}
        if not self.fix_shading:   # (a frozen ShadingNet keeps the packed weights the engine was built with)
            for nm, mod, fb, db, wb in layers():
                plans.reg(eng.f[nm], fb, mod, True)
                if db is not None:
                    plans.reg(eng.d[nm], db, mod, False)
                self.wg[nm] = plans.wg_plan(mod, wb)
            # input-gradient plans of the two inner skipConv1 layers (the attack never needs them: skipConv1 sees the scene only)
            for key, i in (('skip1b', 2), ('skip1c', 4)):
                self.skip_d[key] = plans.dgrad(sn.skipConv1[i], False, 1, 1, key + '_dgrad')
            # use_rough=False: the surface branch's input gradients (the engine has none: for the attack the branch is a constant)
            for nm in ('conv2_s', 'conv3_s', 'conv4_s') if not self.rough else ():
                self.sd[nm] = plans.dgrad(getattr(sn, nm), False, *_SHADING[nm], 'train.' + nm + '_dgrad')
        self.warp = _GridTrainer(self.pc.warping_net, prj_size, plans, dev)   # (the grid samples the projector image)
        B, H, W = self.B, self.Hc, self.Wc
        z = _zeros(dev)
        nb = 1 if self.collapse else B                               # skipConv1 runs at batch 1 when collapsed
        self.t0, self.t1 = z(nb, H, W, 4), z(nb, H, W, 4)            # skipConv1 intermediates (kept for its gradients)
        self.g_r1, self.g_t1, self.g_t0 = z(nb, H, W, 4), z(nb, H, W, 4), z(nb, H, W, 4)
        if self.collapse:
            self.r1, self.sum_r1 = z(1, H, W, 4), z(1, H, W, 4)
        if self.collapse and not self.rough:
            # the surface branch at batch 1: activations, their ReLU-gate bytes, gradients (w.r.t. the pre-activations) and the
            # input gradients that join the batch sums
            H2, W2, H4, W4 = H // 2, W // 2, H // 4, W // 4
            shp = {'S1': (H2, W2, 32), 'S2': (H4, W4, 64), 'S3': (H4, W4, 128), 'S4': (H4, W4, 256)}
            self.s1a = {k: z(1, *v) for k, v in shp.items()}
            self.s1m = {k: torch.zeros(1, v[0], v[1], v[2] // 4, dtype=torch.uint8, device=dev) for k, v in shp.items()}
            self.s1g = {k: z(1, *v) for k, v in shp.items()}
            self.s1t = {k: z(1, *shp[k]) for k in ('S1', 'S2', 'S3')}
        self.eng = eng

    def _build_grid(self):
        """The engine's grid and taps from the WarpingNet's current parameters."""
        eng = self.eng
        eng.grid = self.warp.forward()
        eng.tap_off, eng.tap_order, eng.tap_wm, eng.tap_src = transposed_taps(eng.grid, (eng.Hp, eng.Wp), (self.Hc, self.Wc), eng.mask,
                                                                              want_table=True)
        eng.tiled = None   # (the grid changes every step: the per-tile boxes of the LDS-staged gather are not rebuilt)

    def _set_scene(self):
        """PCNetEngine.set_scene, keeping the skipConv1 intermediates; with `collapse` the scene-only layers at batch 1, broadcast."""
        eng = self.eng
        eng.version += 1
        eng.scene = self.scene4
        R = _lib.ACT_RELU
        scene, r1 = (self.scene1, self.r1) if self.collapse else (self.scene4, eng.a['R1'])
        eng.f['skip1a'].run(scene, self.t0, act=R)
        eng.f['skip1b'].run(self.t0, self.t1, act=R)
        eng.f['skip1c'].run(self.t1, r1, act=R)
        if not self.collapse:
            if not self.rough:
                eng._surface_branch(self.scene4)
            return
        eng.a['R1'].copy_(self.r1.expand_as(eng.a['R1']))
        if not self.rough:
            a, m, f = self.s1a, self.s1m, eng.f
            f['conv1_s'].run(self.scene1, a['S1'], act=R, mask_out=m['S1'])
            f['conv2_s'].run(a['S1'], a['S2'], act=R, mask_out=m['S2'])
            f['conv3_s'].run(a['S2'], a['S3'], act=R, mask_out=m['S3'])
            f['conv4_s'].run(a['S3'], a['S4'], act=R, mask_out=m['S4'])
            for k in ('S1', 'S2', 'S3', 'S4'):
                dict.__getitem__(eng.a, k).copy_(a[k].expand_as(eng.a[k]))

    def _batch_sum(self, g, add, gate_bits, out, B):
        """out = gate(sum_b g[b] + add) (spaa_batch_sum_gate_bits) over NHWC [B,H,W,C] -> [1,H,W,C]."""
        _, h, w, c = out.shape
        _lib.call('spaa_batch_sum_gate_bits', _lib.ptr(g), _lib.ptr(add), C_ptr(gate_bits) if gate_bits is not None else None,
                  _lib.ptr(out), B, h, w, c, c)

    # ------------------------------------------------------------------------------------------------------------
    def step(self, prj_batch, cam_batch, loss=None):
        """One training iteration (train_network.py:293-357).  Returns (loss value, l2 (MSE) value) as Python floats — the one
        host sync of the step, which the reference also has (`.item()` :307,346)."""
        if loss is None:
            loss = 'l1' if self.iters <= 400 else 'l1+ssim'                     # :300-303
        if loss == '':
            raise TypeError('Loss type not specified')                            # compute_loss :368-369
        if 'l2' in loss or 'huber' in loss:
            raise NotImplementedError("spaa_amd training implements the reference's PCNet losses 'l1' and 'l1+ssim'")
        with _lib.on_device(self.dev):
            return self._step(prj_batch, cam_batch, loss)

    def _step(self, prj_batch, cam_batch, loss):
        p = _lib.ptr
        B, H, W = self.B, self.Hc, self.Wc
        x4 = to_nhwc4(prj_batch.to(self.dev))
        t4 = to_nhwc4(cam_batch.to(self.dev))
        if self.eng is None:
            self._make_engine(tuple(prj_batch.shape[-2:]))
        eng = self.eng
        # ---- forward with the current parameters
        self.plans.refresh()
        self._build_grid()
        self._set_scene()
        y4 = eng.forward(x4, clamp01=False)                                      # model(prj, scene) :306
        # ---- loss and its gradient w.r.t. conv6's pre-activation (compute_loss :367-392, then the output layer's clamp / ReLU gate)
        gP = self.loss.grad(y4, t4, eng.a['Ypre'], loss)
        # ---- backward: input gradients (fills every layer's pre-activation gradient), then weight gradients
        eng.backward(gP, input_grad=False)   # (no gradient w.r.t. the projector image: it is data here)
        if not self.fix_shading:
            self._shading_wgrads(gP)
        # ---- WarpingNet: grid gradient (summed over the batch), then refine net, TPS / affine parameters
        _lib.call('spaa_warp_bwd_grid', p(eng.g['xw']), p(x4), p(eng.grid), p(eng.mask), p(self.warp.ws['g_fine']), B, eng.Hp, eng.Wp,
                  H, W)
        self.warp.backward(self.grads)
        # ---- optimiser steps (:318-320) and schedulers (:354-356)
        self.iters += 1
        for grp in self.groups.values():
            lr = grp['lr'] * (self.gamma if (self.iters - 1) >= grp['milestone'] else 1.0)
            _adam(self.params, self.grads, self.m, self.v, grp['names'], lr, grp['wd'], self.iters)
        self.pc.invalidate()
        return self.loss.value(loss)

    def _shading_wgrads(self, gP):
        """Weight and bias gradients of every ShadingNet layer from `gP` (w.r.t. conv6's pre-activation) and the pre-activation
        gradients eng.backward left."""
        p = _lib.ptr
        eng = self.eng
        a, g = eng.a, eng.g
        gr = self.grads
        wplan = self.wg

        def wgrad(name, pname, inp, gout, in_coff=0):
            dw, db = wplan[name].wgrad(inp, gout, in_coff=in_coff)
            gr[pname + '.weight'] = wplan[name].unpack_grad(dw)
            gr[pname + '.bias'] = db

        sp = 'shading_net.'
        wgrad('conv6', sp + 'conv6', a['X7'], gP)
        wgrad('transConv2', sp + 'transConv2', a['X6'], g['P7'])
        wgrad('transConv1', sp + 'transConv1', a['X5'], g['P6'])
        wgrad('conv5', sp + 'conv5', a['X4'], g['P5'])
        wgrad('conv4', sp + 'conv4', a['X3'], g['P4'])
        wgrad('conv3', sp + 'conv3', a['X2'], g['P3'])
        wgrad('conv2', sp + 'conv2', a['X1'], g['P2'])
        wgrad('conv1', sp + 'conv1', a['xw'], g['P1'])
        wgrad('skipConv3', sp + 'skipConv3', a['X2'], g['P5'])
        wgrad('skipConv2', sp + 'skipConv2', a['X1'], g['P6'])
        if self.rough:
            wgrad('conv4_s', sp + 'conv4_s', a['S3'], g['S4'])
            wgrad('conv3_s', sp + 'conv3_s', a['S2'], g['S3'])
            wgrad('conv2_s', sp + 'conv2_s', a['S1'], g['S2'])
            wgrad('conv1_s', sp + 'conv1_s', a['cat8'], g['S1'])
        elif self.collapse:
            # the surface branch ran once (batch 1): res_k_s = relu(conv_k_s(.)) enters relu(conv_k(x) + res_k_s) of every sample,
            # so d/d res_k_s = sum_b P_k[b]; gS_k = gate(S_k) . (conv_{k+1}_s^T(gS_{k+1}) + sum_b P_k[b])
            sa, sm, sg, st = self.s1a, self.s1m, self.s1g, self.s1t
            self._batch_sum(g['P4'], None, sm['S4'], sg['S4'], self.B)
            wgrad('conv4_s', sp + 'conv4_s', sa['S3'], sg['S4'])
            self.sd['conv4_s'].run(sg['S4'], st['S3'])
            self._batch_sum(g['P3'], st['S3'], sm['S3'], sg['S3'], self.B)
            wgrad('conv3_s', sp + 'conv3_s', sa['S2'], sg['S3'])
            self.sd['conv3_s'].run(sg['S3'], st['S2'])
            self._batch_sum(g['P2'], st['S2'], sm['S2'], sg['S2'], self.B)
            wgrad('conv2_s', sp + 'conv2_s', sa['S1'], sg['S2'])
            self.sd['conv2_s'].run(sg['S2'], st['S1'])
            self._batch_sum(g['P1'], st['S1'], sm['S1'], sg['S1'], self.B)
            wgrad('conv1_s', sp + 'conv1_s', self.scene1, sg['S1'])
        else:
            # the same chain at batch B (the B samples' branches are identical; the weight gradients sum over them).  The first gate
            # is the batch-1 kernel over the B images laid end to end as one [1, B H/4, W/4, 256] tensor
            m = eng.m
            s4 = g['S4']
            self._batch_sum(g['P4'], None, m['S4'], s4.view(1, -1, *s4.shape[2:]), 1)
            wgrad('conv4_s', sp + 'conv4_s', a['S3'], g['S4'])
            self.sd['conv4_s'].run(g['S4'], g['S3'], add=g['P3'], gate_bits=m['S3'])
            wgrad('conv3_s', sp + 'conv3_s', a['S2'], g['S3'])
            self.sd['conv3_s'].run(g['S3'], g['S2'], add=g['P2'], gate_bits=m['S2'])
            wgrad('conv2_s', sp + 'conv2_s', a['S1'], g['S2'])
            self.sd['conv2_s'].run(g['S2'], g['S1'], add=g['P1'], gate_bits=m['S1'])
            wgrad('conv1_s', sp + 'conv1_s', self.scene4, g['S1'])
        # skipConv1 (on the scene; its output is added to conv6's pre-activation, models.py:291,301)
        if self.collapse:   # (batch 1: the ReLU gate of R1 is the same for every sample, so the batch sum comes first)
            self._batch_sum(gP, None, None, self.sum_r1, self.B)
            _lib.call('spaa_relu_gate', p(self.sum_r1), p(self.r1), p(self.g_r1), self.g_r1.numel())
            skip_in = self.scene1
        else:
            _lib.call('spaa_relu_gate', p(gP), p(a['R1']), p(self.g_r1), gP.numel())                 # ReLU after skipConv1.4
            skip_in = self.scene4
        wgrad('skip1c', sp + 'skipConv1.4', self.t1, self.g_r1)
        self.skip_d['skip1c'].run(self.g_r1, self.g_t1, gate=self.t1)
        wgrad('skip1b', sp + 'skipConv1.2', self.t0, self.g_t1)
        self.skip_d['skip1b'].run(self.g_t1, self.g_t0, gate=self.t0)
        wgrad('skip1a', sp + 'skipConv1.0', skip_in, self.g_t0)


def compute_loss(prj_infer, prj_train, loss_option):
    """train_network.py:367-392 on HIP for the options PCNet training uses ('l1', 'l1+ssim'): returns (train_loss, l2_loss)
    as 0-dim tensors (no gradient: `PCNetTrainer.step` carries the gradient path)."""
    if loss_option == '':
        raise TypeError('Loss type not specified')
    dev = prj_infer.device
    with _lib.on_device(dev):
        y4, t4 = to_nhwc4(prj_infer), to_nhwc4(prj_train.to(dev))
        b, h, w, _ = y4.shape
        head = _LossHead(b, h, w, dev, gate=False)
        head.launch(y4, t4, 1.0, 1.0)   # (both terms always; the option picks from them below)
        s = head.ws['partial'].sum(dim=0) / (3.0 * b * h * w)
        loss = torch.zeros((), device=dev)
        if 'l1' in loss_option:
            loss = loss + s[1]
        if 'l2' in loss_option:
            loss = loss + s[2]
        if 'ssim' in loss_option:
            loss = loss + (1 - s[0])
        return loss, s[2]


def train_pcnet(model, train_data, valid_data, cfg):
    """train_network.py:235-363 (without the visdom plots): `train_data` = dict(cam_scene [1,3,H,W], cam_train, prj_train),
    `cfg` with max_iters, batch_size, num_train, l2_reg, lr_drop_ratio, device.  Returns (model, valid_psnr, valid_rmse,
    valid_ssim) like the reference."""
    get = _cfg_getter(cfg)
    dev = torch.device(get('device', 'cuda'))
    tr = PCNetTrainer(model, train_data['cam_scene'], get('batch_size'), get('l2_reg', 1e-4), get('lr_drop_ratio', 0.2), dev)
    cam_train, prj_train = train_data['cam_train'], train_data['prj_train']
    valid_psnr = valid_rmse = valid_ssim = 0.0
    for it in range(get('max_iters')):
        idx = random.sample(range(get('num_train')), get('batch_size'))            # :295
        loss, l2 = tr.step(prj_train[idx], cam_train[idx])
        if get('verbose', False) and (it % 50 == 0 or it == get('max_iters') - 1):
            print(f'Iter:{it:5d} | Train Loss: {loss:.4f} | Train RMSE: {math.sqrt(l2 * 3):.4f}')
    if valid_data is not None:
        from . import metrics
        with torch.no_grad():
            infer = model(valid_data['prj_valid'].to(dev), train_data['cam_scene'].to(dev).expand(valid_data['prj_valid'].shape[0], -1, -1, -1))
        valid_psnr, valid_rmse, valid_ssim = (metrics.psnr(infer, valid_data['cam_valid']), metrics.rmse(infer, valid_data['cam_valid']),
                                              metrics.ssim(infer, valid_data['cam_valid']))
    return model, valid_psnr, valid_rmse, valid_ssim


# ================================================================================================================
# CompenNet++ training (train_network.py:98-232)
# ================================================================================================================
# CompenNet's convolutions (models.py:17-45): module name -> (stride, padding); the transposed ones are k2 / s2 / p0
_COMPEN_CONV = {
    'conv1': (2, 1), 'conv2': (2, 1), 'conv3': (1, 1), 'conv4': (1, 1), 'conv5': (1, 1), 'conv1_s': (2, 1), 'conv2_s': (2, 1),
    'conv3_s': (1, 1), 'conv4_s': (1, 1), 'conv6': (1, 1), 'skipConv2': (1, 0), 'skipConv3': (1, 0), 'skipConv1.0': (1, 1),
    'skipConv1.2': (1, 1), 'skipConv1.4': (1, 1)}
_COMPEN_DECONV = ('transConv1', 'transConv2')


class _CompenNetEngine:
    """CompenNet's forward and backward pass for training, workspaces kept across steps.

    The backbone runs at batch B.  The surface branch (conv1_s .. conv4_s) runs once, at batch 1: the scene is one image
    expanded to the batch (train_network.py:139), so every sample's branch is the same.  Its outputs are broadcast into the
    backbone's residual inputs; its gradient is the batch sum of the backbone pre-activation gradients it feeds
    (spaa_batch_sum_gate), the same gradient as the reference's up to summation order.  Every plan is registered with `plans`
    (_TrainedPlans), which refreshes the packed weights on the device each step.  `input_grad`: also produce the gradients
    w.r.t. both inputs (the warped camera image and the warped scene: CompenNet++ needs them for the grid)."""

    def __init__(self, cn, B, H, W, dev, plans, input_grad):
        self.cn, self.B, self.H, self.W, self.dev, self.input_grad = cn, B, H, W, dev, input_grad
        self.f, self.d, self.wg = {}, {}, {}
        no_d = () if input_grad else ('conv1', 'conv1_s', 'skipConv1.0')   # (the layers that read the inputs: self.d[.] is None)
        layers = [(nm, False, sp) for nm, sp in _COMPEN_CONV.items()] + [(nm, True, (2, 0)) for nm in _COMPEN_DECONV]
        for nm, deconv, (st, pad) in layers:
            self.f[nm], self.d[nm], self.wg[nm] = plans.layer(cn.get_submodule(nm), deconv, st, pad,
                                                              ('train.' + nm, 'train.' + nm + '_dgrad'), nm not in no_d)
        H2, W2, H4, W4 = H // 2, W // 2, H // 4, W // 4
        z = _zeros(dev)
        shp = {'S1': (H2, W2, 32), 'S2': (H4, W4, 64), 'S3': (H4, W4, 128), 'S4': (H4, W4, 256)}
        self.a = {k: z(1, *v) for k, v in shp.items()}                                   # surface branch, batch 1
        self.a.update({'b' + k: z(B, *v) for k, v in shp.items()})                       # ... broadcast to the batch
        self.a.update(t0=z(B, H, W, 4), t1=z(B, H, W, 4), R1=z(B, H, W, 4), X1=z(B, H2, W2, 32), R2=z(B, H2, W2, 64),
                      X2=z(B, H4, W4, 64), R3=z(B, H4, W4, 128), X3=z(B, H4, W4, 128), X4=z(B, H4, W4, 256), X5=z(B, H4, W4, 128),
                      X6=z(B, H2, W2, 64), X7=z(B, H, W, 32), Y=z(B, H, W, 4), Ypre=z(B, H, W, 4))
        self.g = dict(P7=z(B, H, W, 32), P6=z(B, H2, W2, 64), P5=z(B, H4, W4, 128), P4=z(B, H4, W4, 256), P3=z(B, H4, W4, 128),
                      t2=z(B, H4, W4, 64), P2=z(B, H4, W4, 64), t1s=z(B, H2, W2, 32), P1=z(B, H2, W2, 32), r1=z(B, H, W, 4),
                      t1=z(B, H, W, 4), t0=z(B, H, W, 4), xs=z(B, H, W, 4), xw=z(B, H, W, 4),
                      S4=z(1, H4, W4, 256), sum3=z(1, H4, W4, 128), S3=z(1, H4, W4, 128), sum2=z(1, H4, W4, 64), S2=z(1, H4, W4, 64),
                      sum1=z(1, H2, W2, 32), S1=z(1, H2, W2, 32), sw=z(1, H, W, 4))

    def forward(self, xw, sw):
        """models.py:74-94: xw [B,H,W,4] the (warped) image, sw [1,H,W,4] the (warped) scene.  Returns (Y, Ypre) [B,H,W,4]:
        the output and relu(pre-activation) of conv6 (its clamp gate)."""
        a, f = self.a, self.f
        R, N = _lib.ACT_RELU, _lib.ACT_NONE
        f['conv1_s'].run(sw, a['S1'], act=R)
        f['conv2_s'].run(a['S1'], a['S2'], act=R)
        f['conv3_s'].run(a['S2'], a['S3'], act=R)
        f['conv4_s'].run(a['S3'], a['S4'], act=R)
        for k in ('S1', 'S2', 'S3', 'S4'):
            a['b' + k].copy_(a[k].expand_as(a['b' + k]))
        f['skipConv1.0'].run(xw, a['t0'], act=R)
        f['skipConv1.2'].run(a['t0'], a['t1'], act=R)
        f['skipConv1.4'].run(a['t1'], a['R1'], act=R)
        f['conv1'].run(xw, a['X1'], add=a['bS1'], act=R)
        f['skipConv2'].run(a['X1'], a['R2'], act=N)
        f['conv2'].run(a['X1'], a['X2'], add=a['bS2'], act=R)
        f['skipConv3'].run(a['X2'], a['R3'], act=N)
        f['conv3'].run(a['X2'], a['X3'], add=a['bS3'], act=R)
        f['conv4'].run(a['X3'], a['X4'], add=a['bS4'], act=R)
        f['conv5'].run(a['X4'], a['X5'], add=a['R3'], act=R)
        f['transConv1'].run(a['X5'], a['X6'], add=a['R2'], act=R)
        f['transConv2'].run(a['X6'], a['X7'], act=R)
        f['conv6'].run(a['X7'], a['Y'], add=a['R1'], act=_lib.ACT_RELU_CLAMP1, aux_out=a['Ypre'])
        return a['Y'], a['Ypre']

    def backward(self, gP, xw, sw, grads, prefix):
        """gP: gradient w.r.t. conv6's pre-activation (clamp gate applied) [B,H,W,4].  Fills `grads` with every parameter's
        gradient (names `prefix` + parameter name); with `input_grad`, returns (g_xw [B,H,W,4], g_sw [1,H,W,4])."""
        a, g, d = self.a, self.g, self.d
        p = _lib.ptr

        def wgrad(nm, inp, gout):
            dw, db = self.wg[nm].wgrad(inp, gout)
            grads[prefix + nm + '.weight'] = self.wg[nm].unpack_grad(dw)
            grads[prefix + nm + '.bias'] = db

        def bsum(gb, act, out):
            _lib.call('spaa_batch_sum_gate', p(gb), p(act), p(out), self.B, gb.shape[1], gb.shape[2], gb.shape[3], gb.shape[3])

        # backbone (batch B)
        wgrad('conv6', a['X7'], gP)
        _lib.call('spaa_relu_gate', p(gP), p(a['R1']), p(g['r1']), gP.numel())          # res1 = relu(skipConv1.4(.))
        d['conv6'].run(gP, g['P7'], gate=a['X7'])
        wgrad('transConv2', a['X6'], g['P7'])
        d['transConv2'].run(g['P7'], g['P6'], gate=a['X6'])
        wgrad('transConv1', a['X5'], g['P6'])
        wgrad('skipConv2', a['X1'], g['P6'])                                           # res2 enters transConv1's sum
        d['transConv1'].run(g['P6'], g['P5'], gate=a['X5'])
        wgrad('conv5', a['X4'], g['P5'])
        wgrad('skipConv3', a['X2'], g['P5'])                                           # res3 enters conv5's sum
        d['conv5'].run(g['P5'], g['P4'], gate=a['X4'])
        wgrad('conv4', a['X3'], g['P4'])
        d['conv4'].run(g['P4'], g['P3'], gate=a['X3'])
        wgrad('conv3', a['X2'], g['P3'])
        d['skipConv3'].run(g['P5'], g['t2'])
        d['conv3'].run(g['P3'], g['P2'], add=g['t2'], gate=a['X2'])
        wgrad('conv2', a['X1'], g['P2'])
        d['skipConv2'].run(g['P6'], g['t1s'])
        d['conv2'].run(g['P2'], g['P1'], add=g['t1s'], gate=a['X1'])
        wgrad('conv1', xw, g['P1'])
        # skipConv1 chain (on the image)
        wgrad('skipConv1.4', a['t1'], g['r1'])
        d['skipConv1.4'].run(g['r1'], g['t1'], gate=a['t1'])
        wgrad('skipConv1.2', a['t0'], g['t1'])
        d['skipConv1.2'].run(g['t1'], g['t0'], gate=a['t0'])
        wgrad('skipConv1.0', xw, g['t0'])
        # surface branch (batch 1): res_k_s = relu(conv_k_s(.)) enters relu(conv_k(x) + res_k_s) of every sample
        bsum(g['P4'], a['S4'], g['S4'])
        wgrad('conv4_s', a['S3'], g['S4'])
        bsum(g['P3'], a['S3'], g['sum3'])
        d['conv4_s'].run(g['S4'], g['S3'], add=g['sum3'], gate=a['S3'])
        wgrad('conv3_s', a['S2'], g['S3'])
        bsum(g['P2'], a['S2'], g['sum2'])
        d['conv3_s'].run(g['S3'], g['S2'], add=g['sum2'], gate=a['S2'])
        wgrad('conv2_s', a['S1'], g['S2'])
        bsum(g['P1'], a['S1'], g['sum1'])
        d['conv2_s'].run(g['S2'], g['S1'], add=g['sum1'], gate=a['S1'])
        wgrad('conv1_s', sw, g['S1'])
        if not self.input_grad:
            return None
        d['skipConv1.0'].run(g['t0'], g['xs'])
        d['conv1'].run(g['P1'], g['xw'], add=g['xs'])
        d['conv1_s'].run(g['S1'], g['sw'])
        return g['xw'], g['sw']


class CompenNetTrainer:
    """State of one CompenNet++ (or bare CompenNet) training run: engine, Adam moments, learning rate.  `step(cam_batch,
    prj_batch)` is one iteration of the reference's loop body (train_network.py:180-192) plus its scheduler step (:226):
    one torch.optim.Adam over ALL parameters (WarpingNet included) with L2 weight decay `l2_reg`, StepLR(lr_drop_rate,
    lr_drop_ratio).  The kernels: the module docstring."""

    def __init__(self, model, cam_scene, batch_size, lr=1e-3, l2_reg=1e-4, lr_drop_rate=800, lr_drop_ratio=0.2, device='cuda'):
        from .models import CompenNet, CompenNetPlusplus
        if isinstance(model, CompenNetPlusplus):
            self.pp, cn, wn = True, model.compen_net, model.warping_net
        elif isinstance(model, CompenNet):
            self.pp, cn, wn = False, model, None
        else:
            raise TypeError('CompenNetTrainer needs a spaa_amd.CompenNetPlusplus or spaa_amd.CompenNet')
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise RuntimeError('spaa_amd training runs on the GPU only (no CPU fallback)')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        for n, prm in model.named_parameters():
            if prm.device != dev or prm.dtype != torch.float32:
                raise ValueError(f'CompenNetTrainer: parameter {n} is {prm.dtype} on {prm.device}; move the model to {dev} first')
        if wn is not None and not wn.with_refine:
            raise NotImplementedError('CompenNet++ training covers WarpingNet with the grid-refine net (with_refine=True)')
        s = cam_scene.detach().float()
        while s.ndim < 4:
            s = s[None]
        if s.shape[0] != 1 or s.shape[1] != 3:
            raise ValueError(f'cam_scene must be one [3,H,W] / [1,3,H,W] image, got {tuple(cam_scene.shape)}')
        self.Hs, self.Ws = s.shape[-2:]                         # source size of the warp (camera), = output size without it
        self.H, self.W = wn.out_size if self.pp else (self.Hs, self.Ws)
        if self.H % 4 or self.W % 4:
            raise ValueError(f'CompenNet training needs an output (projector) size divisible by 4, got {self.H}x{self.W}')
        self.model, self.cn, self.wn, self.dev, self.B = model, cn, wn, dev, int(batch_size)
        self.lr, self.l2_reg = float(lr), float(l2_reg)
        self.lr_drop_rate, self.gamma = int(lr_drop_rate), float(lr_drop_ratio)
        self.prefix = 'compen_net.' if self.pp else ''
        self.params = dict(model.named_parameters())
        with _lib.on_device(dev):
            self.scene4 = to_nhwc4(s.to(dev))
            self.m = {n: torch.zeros_like(p) for n, p in self.params.items()}
            self.v = {n: torch.zeros_like(p) for n, p in self.params.items()}
            self.plans = _TrainedPlans(dev)
            self.eng = _CompenNetEngine(cn, self.B, self.H, self.W, dev, self.plans, input_grad=self.pp)
            if self.pp:
                self.warp = _GridTrainer(wn, (self.Hs, self.Ws), self.plans, dev)   # (the grid samples the camera images)
                self.xw, self.sw = (torch.zeros(n, self.H, self.W, 4, device=dev) for n in (self.B, 1))   # the warped images, scene
            self.loss = _LossHead(self.B, self.H, self.W, dev)
        self.grads = {}
        self.iters = 0

    # ------------------------------------------------------------------------------------------------------------
    def step(self, cam_batch, prj_batch, loss='l1+ssim'):
        """One training iteration (train_network.py:180-192, :226): `cam_batch` [B,3,Hc,Wc] the model input, `prj_batch`
        [B,3,Hp,Wp] the target.  Returns (loss value, l2 (MSE) value) as Python floats."""
        if loss == '':
            raise TypeError('Loss type not specified')                            # compute_loss :368-369
        if 'l2' in loss or 'huber' in loss:
            raise NotImplementedError("spaa_amd CompenNet++ training implements the losses 'l1', 'ssim' and 'l1+ssim'")
        if 'l1' not in loss and 'ssim' not in loss:
            raise ValueError(f'unknown loss option {loss!r}')
        B = self.B
        if tuple(cam_batch.shape) != (B, 3, self.Hs, self.Ws) or tuple(prj_batch.shape) != (B, 3, self.H, self.W):
            raise ValueError(f'expected cam_batch [{B},3,{self.Hs},{self.Ws}] and prj_batch [{B},3,{self.H},{self.W}], got '
                             f'{tuple(cam_batch.shape)} and {tuple(prj_batch.shape)}')
        with _lib.on_device(self.dev):
            return self._step(cam_batch, prj_batch, loss)

    def _step(self, cam_batch, prj_batch, loss):
        p = _lib.ptr
        B, H, W, eng = self.B, self.H, self.W, self.eng
        cam4 = to_nhwc4(cam_batch.to(self.dev))
        t4 = to_nhwc4(prj_batch.to(self.dev))
        # ---- forward with the current parameters (model(cam, scene) :185)
        self.plans.refresh()
        if self.pp:
            fine = self.warp.forward()
            _lib.call('spaa_warp_fwd', p(cam4), p(fine), None, None, p(self.xw), None, B, self.Hs, self.Ws, H, W, 0)
            _lib.call('spaa_warp_fwd', p(self.scene4), p(fine), None, None, p(self.sw), None, 1, self.Hs, self.Ws, H, W, 0)
            xw, sw = self.xw, self.sw
        else:
            xw, sw = cam4, self.scene4
        y4, ypre = eng.forward(xw, sw)
        # ---- loss and its gradient w.r.t. conv6's pre-activation (compute_loss :367-392, then the clamp / ReLU gate of conv6)
        gP = self.loss.grad(y4, t4, ypre, loss)
        # ---- backward; the WarpingNet's from the gradients w.r.t. BOTH warped images (models.py:208-209)
        gin = eng.backward(gP, xw, sw, self.grads, self.prefix)
        if self.pp:
            _lib.call('spaa_warp_bwd_grid2', p(gin[0]), p(cam4), B, p(gin[1]), p(self.scene4), 1, p(fine), p(self.warp.ws['g_fine']),
                      self.Hs, self.Ws, H, W)
            self.warp.backward(self.grads)
        # ---- Adam over all parameters (:190-192), then StepLR (:226)
        self.iters += 1
        _adam(self.params, self.grads, self.m, self.v, self.params, self.lr, self.l2_reg, self.iters)
        if self.iters % self.lr_drop_rate == 0:
            self.lr *= self.gamma
        self.model.invalidate()
        return self.loss.value(loss)


def _cfg_getter(cfg):
    return (lambda k, d=None: cfg[k] if k in cfg else d) if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))


def _model_name(model):
    return model.name if hasattr(model, 'name') else model.module.name


def evaluate_model(model, valid_data, chunk_sz=10):
    """train_network.py:395-441: (psnr, rmse, ssim, inference on the host) over `valid_data` (cam_scene, cam_valid,
    prj_valid), the metrics of each of `chunk_sz` chunks (metrics.calc_img_dists) weighted by its size.  PCNet maps the
    projector image to the camera image; CompenNet++ (and a bare CompenNet) the camera image to the projector image."""
    from . import metrics
    cam_scene, cam_valid, prj_valid = valid_data['cam_scene'], valid_data['cam_valid'], valid_data['prj_valid']
    name = _model_name(model)
    if 'PCNet' in name:
        model_in, gt = prj_valid, cam_valid
    elif 'CompenNet' in name:
        model_in, gt = cam_valid, prj_valid
    else:
        raise ValueError(f'evaluate_model: unknown model {name!r}')
    dev = next(model.parameters()).device
    num_valid = cam_valid.shape[0]
    if cam_scene.ndim == 3:
        cam_scene = cam_scene[None]
    if cam_scene.shape[0] == 1:
        cam_scene = cam_scene.expand(num_valid, -1, -1, -1)
    valid_psnr, valid_rmse, valid_ssim = 0., 0., 0.
    with torch.no_grad():
        model.eval()
        infer = torch.zeros(gt.shape)
        for idx in torch.chunk(torch.arange(num_valid), chunk_sz):
            out = model(model_in[idx].to(dev), cam_scene[idx].to(dev))
            if isinstance(out, tuple):
                out = out[0]
            infer[idx] = out.detach().cpu()
            m = metrics.calc_img_dists(out, gt[idx].to(dev))
            valid_psnr += m[0] * len(idx) / num_valid
            valid_rmse += m[1] * len(idx) / num_valid
            valid_ssim += m[2] * len(idx) / num_valid
    return valid_psnr, valid_rmse, valid_ssim, infer


def train_compennet_pp(model, train_data, valid_data, cfg):
    """train_network.py:130-232 (without the visdom plots): `train_data` = dict(cam_scene [1,3,H,W], cam_train, prj_train),
    `cfg` (dict or attribute object) with device, max_iters, batch_size, num_train, lr, l2_reg, lr_drop_rate, lr_drop_ratio,
    loss; with data_root, the trained state dict is saved as `<data_root>/../checkpoint/<io.opt_to_string(cfg)>.pth` like the
    reference's.  Batch indices are random.sample(range(num_train), batch_size) as in the reference.  Validation (when
    `valid_data` is given) runs after the last iteration.  Returns (model, valid_psnr, valid_rmse, valid_ssim)."""
    get = _cfg_getter(cfg)
    dev = torch.device(get('device', 'cuda'))
    loss_opt = get('loss', 'l1+ssim')
    bsz, num_train, max_iters = get('batch_size'), get('num_train'), get('max_iters')
    tr = CompenNetTrainer(model, train_data['cam_scene'], bsz, get('lr', 1e-3), get('l2_reg', 1e-4), get('lr_drop_rate', 800),
                          get('lr_drop_ratio', 0.2), dev)
    cam_train, prj_train = train_data['cam_train'], train_data['prj_train']
    for it in range(max_iters):
        idx = random.sample(range(num_train), bsz)                                # :178
        loss, l2 = tr.step(cam_train[idx], prj_train[idx], loss_opt)
        if get('verbose', False) and (it % 50 == 0 or it == max_iters - 1):
            print(f'Iter:{it:5d} | Train Loss: {loss:.4f} | Train RMSE: {math.sqrt(l2 * 3):.4f} | Learn Rate: {tr.lr:.5f}')
    valid_psnr = valid_rmse = valid_ssim = 0.0
    if valid_data is not None:
        valid_psnr, valid_rmse, valid_ssim, _ = evaluate_model(model, valid_data)
    if get('data_root') is not None:                                                # :229-230
        from . import io
        opt = {k: get(k) for k in ('setup_name', 'model_name', 'loss', 'num_train', 'batch_size', 'max_iters', 'lr', 'lr_drop_ratio',
                                   'lr_drop_rate', 'l2_reg')}
        if opt['model_name'] is None:
            opt['model_name'] = _model_name(model)
        io.save_checkpoint(os.path.join(get('data_root'), '../checkpoint'), model, io.opt_to_string(opt))
    return model, valid_psnr, valid_rmse, valid_ssim


def _init_cfg(data_root, device, model_name, max_iters=500, batch_size=48, num_train=500):
    """init_cfg of train_network.py:118-120 (+ the model name train_compennet_pp adds, :160)."""
    return dict(data_root=data_root, setup_name='init', num_dataset=1, device=device, max_epochs=2000, max_iters=max_iters,
                batch_size=batch_size, lr=1e-3, lr_drop_ratio=0.2, lr_drop_rate=800, loss='l1+ssim', l2_reg=1e-4, plot_on=True,
                train_plot_rate=50, valid_rate=200, num_train=num_train, model_name=model_name)


def init_compennet(compennet, data_root, cfg, *, max_iters=500, batch_size=48, num_train=500):
    """train_network.py:98-127: initialise a bare CompenNet to |x - s| without actual projections.  Loads
    `<data_root>/../checkpoint/init_CompenNet_...pth` if it exists; otherwise trains on `prj_share/init` (scene) and
    `prj_share/train` (target prj, input |prj - 0.3 scene|) with the reference's init_cfg and saves that checkpoint.  The
    keyword-only extras shrink the run (tests); their defaults are the reference's."""
    from . import io
    init_cfg = _init_cfg(data_root, _cfg_getter(cfg)('device', 'cuda'), _model_name(compennet), max_iters, batch_size, num_train)
    ckpt_file = os.path.join(data_root, '../checkpoint', io.opt_to_string(init_cfg) + '.pth')   # the name :100 spells out
    if os.path.exists(ckpt_file):
        dev = next(compennet.parameters()).device
        compennet.load_state_dict(torch.load(ckpt_file, map_location=dev))
        compennet.invalidate()
        print('CompenNet state dict found! Loading...')
        return compennet
    print('CompenNet state dict not found! Initializing...')
    cam_scene = io.torch_imread_mt(os.path.join(data_root, 'prj_share/init'))
    prj_train = io.torch_imread_mt(os.path.join(data_root, 'prj_share/train'))
    init_data = dict(cam_scene=cam_scene, cam_train=torch.abs(prj_train - 0.3 * cam_scene.expand_as(prj_train)), prj_train=prj_train)
    compennet, _, _, _ = train_compennet_pp(compennet, init_data, None, init_cfg)
    return compennet


# ================================================================================================================
# The reference's drivers in front of the attack: load_data, get_model_train_cfg, train_eval_pcnet, train_eval_compennet_pp
# (train_network.py:39-82, :444-733).  No DataParallel, no visdom (`plot_on` is accepted and ignored), no .xlsx log.
# ================================================================================================================
LOG_COLUMNS = ['Setup', 'Model', 'Loss', 'Num train', 'Batch', 'Iters', 'PSNR', 'RMSE', 'SSIM', 'L2', 'L-inf', 'dE']   # utils.py:683
PCNET_MODELS = ('PCNet', 'PCNet_no_mask', 'PCNet_no_rough', 'PCNet_no_mask_no_rough', 'PCNet_w/o_refine')


def load_data(data_root, setup_name, input_size=None, compensation=False, *, device='cuda', gpu_decode=False):
    """train_network.py:39-82: reads `<data_root>/setups/<setup_name>/cam/raw/{ref,train,test,cb}` and `<data_root>/prj_share/
    {train,test}` and returns (cam_scene [1,3,H,W] = ref/img_0002, cam_train, cam_valid, prj_train, prj_valid (as many as cam_valid),
    im_mask bool [H,W], mask_corners, setup_info), all on the host like the reference's.  The direct-light mask of the checkerboard
    captures (Nayar's separation with backlight 0.9, then img_proc.threshold_im's chain) is three launches of csrc/direct_mask.hip on
    `device`; there is no CPU fallback.  `compensation=True` (unused by the reference) is not implemented.
    `gpu_decode=True` decodes the PNG files on `device` as well (io.torch_imread_mt(..., device=)) and copies the batches back: the same
    values on the same devices."""
    from os.path import join
    from . import io, img_proc
    if compensation:
        raise NotImplementedError('load_data: only compensation=False (the branch the reference uses) is implemented')
    dev = img_proc._require_gpu(device)
    setup_path = join(data_root, 'setups', setup_name)
    print(f"Loading data from '{setup_path}'")
    setup_info = io.load_setup_info(setup_path)
    rd = (lambda *a, **kw: io.torch_imread_mt(*a, device=dev, **kw)) if gpu_decode else io.torch_imread_mt
    host = (lambda t: t.cpu()) if gpu_decode else (lambda t: t)
    cam_ref = host(rd(join(setup_path, 'cam/raw/ref'), size=input_size))
    gray_idx = 1                                   # ref/img_0002: the surface lit by prj_brightness
    cam_scene = cam_ref[gray_idx].unsqueeze(0)
    cam_train = host(rd(join(setup_path, 'cam/raw/train'), size=input_size))
    prj_train = host(rd(join(data_root, 'prj_share/train')))
    cam_valid = host(rd(join(setup_path, 'cam/raw/test'), size=input_size))
    prj_valid = host(rd(join(data_root, 'prj_share/test'), index=list(range(cam_valid.shape[0]))))
    im_cb = rd(join(setup_path, 'cam/raw/cb'), size=input_size)      # (stays where it was decoded: the mask kernels take either)
    if im_cb.shape[0] < 2:
        raise ValueError(f'load_data: the direct-light separation needs at least two checkerboard captures, found {im_cb.shape[0]}')
    im_mask, _, mask_corners = img_proc._finish(img_proc.direct_mask(im_cb, img_proc.BACKLIGHT, device=dev))
    return cam_scene, cam_train, cam_valid, prj_train, prj_valid, torch.from_numpy(im_mask), mask_corners, setup_info


def get_model_train_cfg(model_list, data_root=None, setup_list=None, device_ids=[0], center_crop=False, load_pretrained=False,
                        plot_on=True, single=False):
    """train_network.py:444-473: the default training configuration (a mapping with attribute access)."""
    from .io import SetupInfo
    cfg = SetupInfo(data_root=data_root, setup_list=setup_list, device='cuda', device_ids=device_ids, load_pretrained=load_pretrained,
                    max_iters=2000, batch_size=24, lr=1e-3, lr_drop_ratio=0.2, lr_drop_rate=800, l2_reg=1e-4, train_plot_rate=50,
                    valid_rate=200, plot_on=plot_on, center_crop=center_crop)
    if single:
        cfg.update(model_name=model_list[0], num_train=500, loss='l1+ssim')
    else:
        cfg.update(model_list=model_list, num_train_list=[500], loss_list=['l1+ssim'])
    return cfg


def _reset_rng_seeds(seed):
    """utils.py:70-76."""
    import numpy as np
    np.random.seed(seed)
    random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def _init_log(log_dir):
    """utils.py:678-684 without the .xlsx twin: (rows, `<log_dir>/<datetime>.txt`)."""
    import time
    os.makedirs(log_dir, exist_ok=True)
    return [], os.path.join(log_dir, time.strftime('%Y-%m-%d_%H_%M_%S', time.localtime()) + '.txt')


def _write_log(rows, filename):
    """utils.py:687-694: the table as CSV with 4 decimals (rewritten after every row, so an interrupted run keeps its rows)."""
    import pandas as pd
    ret = pd.DataFrame(rows, columns=LOG_COLUMNS)
    ret.to_csv(filename, mode='w', index=False, float_format='%.4f')
    print(f'Log file saved to {filename}')
    return ret


def _mean_rows(rows, model_list, n_setups):
    """train_network.py:583-586: per model, the mean of the numeric columns over its rows."""
    import numpy as np
    out = []
    for model_name in model_list:
        sel = [r for r in rows if r[1] == model_name]
        out.append([f'[mean]_{n_setups}_setups', model_name, float('nan')] + [float(np.mean([r[k] for r in sel])) for k in range(3, 12)])
    return out


def _affine_from_corners(mask_corners):
    """The WarpingNet's initial affine (train_network.py:542-546): grid_sample warps inversely, so the matrix maps the output
    square's corners to the mask's box."""
    from .img_proc import get_affine_transform
    src_pts = [[-1, -1], [1, -1], [1, 1]]
    return torch.from_numpy(get_affine_transform(mask_corners[0:3], src_pts)).float().flatten()


def _build_pcnet(model_name, cam_mask, mask_corners, out_size, device):
    """A fresh PCNet by name (train_network.py:532-552): seed 123, ShadingNetSPAA / WarpingNet variants from the name, the affine
    from the mask corners."""
    from .models import ShadingNetSPAA, WarpingNet
    _reset_rng_seeds(123)
    use_rough, use_mask = 'no_rough' not in model_name, 'no_mask' not in model_name
    shading_net = ShadingNetSPAA(use_rough=use_rough)
    warping_net = WarpingNet(out_size=tuple(out_size), with_refine='w/o_refine' not in model_name)   # warps prj to the camera view
    warping_net.set_affine(_affine_from_corners(mask_corners))
    return PCNet(cam_mask.float(), warping_net, shading_net, fix_shading_net=False, use_mask=use_mask, use_rough=use_rough).to(device)


def _build_compennet_pp(model_name, compen_net, mask_corners, prj_size, device):
    """A fresh CompenNet++ (train_network.py:653-668): seed 0, a WarpingNet with the affine from the mask corners, a copy of the
    initialised CompenNet."""
    from .models import CompenNetPlusplus, WarpingNet
    _reset_rng_seeds(0)
    warping_net = WarpingNet(out_size=tuple(prj_size), with_refine='w/o_refine' not in model_name)   # warps the camera view to prj
    warping_net.set_affine(_affine_from_corners(mask_corners))
    return CompenNetPlusplus(warping_net, compen_net).to(device)


def _setup_data(cfg_default, setup_name, device, crop):
    """Loads one setup (train_network.py:488-509, :615-630): host training tensors, validation data on the device."""
    from .img_proc import center_crop as cc
    cam_scene, cam_train, cam_valid, prj_train, prj_valid, cam_mask, mask_corners, setup_info = load_data(
        cfg_default.data_root, setup_name, device=device)
    cfg_default.setup_info = setup_info
    if crop:
        cp_sz = tuple(setup_info['classifier_crop_sz'])
        cam_scene, cam_train, cam_valid, cam_mask = (cc(t, cp_sz) for t in (cam_scene, cam_train, cam_valid, cam_mask))
    cam_scene = cam_scene.to(device)
    cam_valid, prj_valid = cam_valid.to(device), prj_valid.to(device)
    valid_data = dict(cam_scene=cam_scene.expand(cam_valid.shape[0], -1, -1, -1), cam_valid=cam_valid, prj_valid=prj_valid)
    return cam_scene, cam_train, prj_train, cam_mask, mask_corners, valid_data


def _configurations(cfg_default, setup_name):
    """The num_train x model x loss loops (train_network.py:511-530): yields (cfg, model_name, loss, num_train, model_version)."""
    from .io import SetupInfo
    for num_train in cfg_default.num_train_list:
        cfg = SetupInfo({k: v for k, v in cfg_default.items() if k not in ('num_train_list', 'model_list', 'loss_list', 'setup_list')})
        cfg.num_train = num_train
        for model_name in cfg_default.model_list:
            cfg.model_name = model_name.replace('/', '_')
            for loss in cfg_default.loss_list:
                cfg.setup_name = setup_name.replace('/', '_')
                cfg.loss = loss
                yield cfg, model_name, loss, num_train, f'{cfg.model_name}_{loss}_{num_train}_{cfg.batch_size}_{cfg.max_iters}'


def _print_options(cfg):
    print('-------------------------------------- Training Options -----------------------------------')
    print('\n'.join(f'{k}: {v}' for k, v in cfg.items()))


def _save_compensations(model, cam_scene, setup_path, model_version):
    """train_network.py:696-719: the compensations of `<setup>/cam/desire/test` to `<setup>/prj/cmp/test/<model_version>`."""
    import warnings
    from os.path import join
    from . import io
    desire_path = join(setup_path, 'cam/desire/test')
    if os.path.isdir(desire_path):
        desire = io.torch_imread_mt(desire_path)
        with torch.no_grad():
            cmp = torch.cat([model(d.to(cam_scene.device), cam_scene.expand(d.shape[0], -1, -1, -1)).cpu() for d in desire.split(16)])
        io.save_imgs(cmp, join(setup_path, 'prj/cmp/test', model_version))
        print('Compensation images saved to ' + join(setup_path, 'prj/cmp/test', model_version))
    else:
        warnings.warn(f'images and folder {desire_path:s} does not exist, no compensation images saved!')


def _train_eval(cfg_default, log, crop, build, train, save_ckpt, gt_key, infer_dir, infer_what, after=None):
    """The loop of both drivers (train_network.py:476-594, :597-733).  Per model family: `build(model_name, cam_mask, mask_corners,
    cam_train, prj_train, device)` makes a fresh model; `train` is its train_* function, `save_ckpt` says that the checkpoint is saved
    here and not by `train`; the model infers `valid_data[gt_key]`, written to `<setup>/<infer_dir>/<model_version>`; `after(model,
    cam_scene, setup_path, model_version)` is an extra step per configuration.  `log`: `_init_log`'s pair."""
    from os.path import join
    from . import io, metrics
    data_root = cfg_default.data_root
    device = torch.device(cfg_default.device)
    rows, log_file = log
    model = cfg = None
    for setup_name in cfg_default.setup_list:
        setup_path = join(data_root, 'setups', setup_name)
        cam_scene, cam_train, prj_train, cam_mask, mask_corners, valid_data = _setup_data(cfg_default, setup_name, device, crop)
        for cfg, model_name, loss, num_train, model_version in _configurations(cfg_default, setup_name):
            model = build(model_name, cam_mask, mask_corners, cam_train, prj_train, device)
            train_data = dict(cam_scene=cam_scene, cam_train=cam_train[:num_train], prj_train=prj_train[:num_train], mask=cam_mask)
            _print_options(cfg)
            if not cfg.load_pretrained:
                print(f'------------------------------------ Start training {model_name:s} ---------------------------')
                model = train(model, train_data, valid_data, cfg)[0]
                if save_ckpt:
                    print('Checkpoint saved to ' + io.save_checkpoint(join(data_root, '../checkpoint'), model, io.opt_to_string(cfg)))
            else:
                print(f'------------------------------------ Loading pretrained {model_name:s} ---------------------------')
                model.load_state_dict(torch.load(join(data_root, '../checkpoint', io.opt_to_string(cfg) + '.pth'), map_location=device))
            infer = evaluate_model(model, valid_data)[-1]
            rows.append([setup_name, model_name, loss, num_train, cfg.batch_size, cfg.max_iters,
                         *metrics.calc_img_dists(infer, valid_data[gt_key])])
            _write_log(rows, log_file)
            infer_path = join(setup_path, infer_dir, model_version)
            io.save_imgs(infer, infer_path)
            print(f'Inferred {infer_what} images saved to ' + infer_path)
            if after is not None:
                after(model, cam_scene, setup_path, model_version)
    rows += _mean_rows(rows, cfg_default.model_list, len(cfg_default.setup_list))
    ret = _write_log(rows, log_file)
    print(ret.to_string(justify='center', float_format='%.4f'))
    return model, ret, cfg


def train_eval_pcnet(cfg_default):
    """train_network.py:476-594: for every setup x num_train x model x loss of `cfg_default` (get_model_train_cfg), train a PCNet
    (`train_pcnet`) or, with load_pretrained, load `<data_root>/../checkpoint/<io.opt_to_string(cfg)>.pth`; evaluate it on the
    validation pairs; write the inferred camera images to `<setup>/cam/infer/test/<model_version>`; log one row per configuration
    and the per-model `[mean]_N_setups` rows to `<data_root>/../log/<datetime>.txt`.  The checkpoint is saved here after training
    (the reference's train_pcnet does it, :361).  Models by name: PCNet, PCNet_no_mask, PCNet_no_rough, PCNet_no_mask_no_rough,
    PCNet_w/o_refine.  Returns (the last model, the log as a DataFrame, the last configuration)."""
    def build(model_name, cam_mask, mask_corners, cam_train, prj_train, device):
        if not model_name.startswith('PCNet'):
            raise ValueError(f'train_eval_pcnet: unknown model {model_name!r} (one of {PCNET_MODELS})')
        return _build_pcnet(model_name, cam_mask, mask_corners, tuple(cam_train.shape[-2:]), device)

    return _train_eval(cfg_default, _init_log(os.path.join(cfg_default.data_root, '../log')), cfg_default.center_crop, build, train_pcnet,
                       True, 'cam_valid', 'cam/infer/test', 'camera-captured (relit)')


def train_eval_compennet_pp(cfg_default):
    """train_network.py:597-733, like `train_eval_pcnet` for CompenNet++: a CompenNet initialised once by `init_compennet` (its
    checkpoint is loaded when present), then per configuration a WarpingNet with the affine from the mask corners + a copy of that
    CompenNet, trained by `train_compennet_pp` (seed 0; it saves the checkpoint itself) or loaded; the inferred projector images go to
    `<setup>/prj/infer/test/<model_version>`, and when `<setup>/cam/desire/test` exists its compensations to `<setup>/prj/cmp/test/
    <model_version>`.  An optional `cfg_default['init_compennet']` = dict(max_iters=, batch_size=, num_train=) shrinks the
    initialisation run (its defaults are the reference's)."""
    from .models import CompenNet
    log = _init_log(os.path.join(cfg_default.data_root, '../log'))
    compen_net = init_compennet(CompenNet().to(torch.device(cfg_default.device)), cfg_default.data_root, cfg_default,
                                **(cfg_default.get('init_compennet') or {}))

    def build(model_name, cam_mask, mask_corners, cam_train, prj_train, device):
        return _build_compennet_pp(model_name, compen_net, mask_corners, tuple(prj_train.shape[2:4]), device)

    return _train_eval(cfg_default, log, False, build, train_compennet_pp, False, 'prj_valid', 'prj/infer/test',
                       'projector input validation', _save_compensations)
