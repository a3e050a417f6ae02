"""The host side of plnerf_train_step (include/plnerf_hip_step.h): one library call per optimisation step.

A `StepPlan` owns what the call needs beyond the networks and their optimizers -- the workspace the library carves up,
the flat gradient buffer whose slices become the parameters' `.grad`, the two linspace tables -- and the three structs
of the ABI.  `plnerf_step_config` and `plnerf_step_io` are filled once; a step rewrites `plnerf_step_args` and the one
output pointer.  Device memory that can move under a plan (a network's packed buffer on `.to()` or a precision change,
optim.FlatAdam's flat buffers, the moments after a `load_state_dict`) is looked at before every step with a handful of
pointer compares, the way FlatAdam.step confirms its own layout: `current()` says whether the plan still describes the
live objects, and train.TrainStep builds a new one when it does not.  A plan never steps memory it has not just seen.
"""
import ctypes

import torch

from . import _lib as L
from . import functional as Fn
from .optim import FlatAdam


def plan_key(kw, kind, max_rays, H, W, K, near, far, bank, seed):
    """Everything a plan's config is built from: a step whose key differs gets a plan of its own."""
    return (kind, int(max_rays), int(H), int(W), float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]), float(near),
            float(far), id(bank) if bank is not None else None, int(seed), int(kw["N_samples"]), int(kw["N_importance"]),
            kw["color_mode"], bool(kw.get("lindisp", False)), kw.get("perturb", 0.) > 0., bool(kw.get("white_bkgd", False)),
            bool(kw.get("farcolorfix", False)), float(kw.get("raw_noise_std", 0.)), float(kw.get("zero_tol", 1e-4)),
            float(kw.get("epsilon", 1e-3)), bool(kw.get("ndc", True)), L.FWD_KERNEL)


class _NetSlot:
    """One network, its optimizer and the device addresses the plan recorded for them."""

    def __init__(self, net, opt, grad_flat, io_net, others):
        self.net, self.opt, self.io = net, opt, io_net
        self.group = opt.param_groups[0]
        self.ps = self.group['params']
        self.fl = opt._flat[0]
        self.precision = net.precision
        sizes = self.fl['sizes']
        self.n = sum(sizes)
        self.last_off = self.n - sizes[-1]
        self.base = self.fl['param'].data_ptr()
        self.m_ptr, self.v_ptr = self.fl['m'].data_ptr(), self.fl['v'].data_ptr()
        net.status_word()                  # (allocates the packed buffer and zeroes its status word, if that is still to do)
        self.packed_ptr = net._packed.data_ptr()
        self.grad_flat = grad_flat         # [n + GRAD_TAIL]
        self.grads = [t.view(p.shape) for t, p in zip(grad_flat[:self.n].split(sizes), self.ps)]
        self.guards = list(opt.guards)
        status_off = L.lib().plnerf_mlp_status_offset(L.PRECISION[net.precision])
        words = []
        for g in self.guards:              # a guard is one of the step's two networks (its word moves with the packed buffer,
            owner = next((o for o in others if o is g), None)      # which current() watches) or a plain device word
            if owner is not None:
                owner.status_word()
                words.append(owner._packed.data_ptr() + status_off)
            elif isinstance(g, torch.Tensor):
                words.append(g.data_ptr())
            else:
                raise ValueError("a guard that is neither of the step's networks nor a device word")
        opt._guarded_now = bool(self.guards)
        wptr = opt._withheld_ptr(self.fl['param'].device)
        self.withheld = opt._withheld
        self.steps = None
        io = self.io
        for k, p in enumerate(self.ps):
            io.params[k] = p.data.data_ptr()
        io.param_flat, io.grad_flat, io.exp_avg, io.exp_avg_sq = self.base, grad_flat.data_ptr(), self.m_ptr, self.v_ptr
        io.n_params = self.n
        io.packed = self.packed_ptr
        io.skip_if_set, io.skip_if_set2 = (words + [None, None])[:2]
        io.withheld = None if wptr is None else wptr.value

    def current(self):
        ps, fl, net, opt = self.ps, self.fl, self.net, self.opt
        pk = net._packed
        return (opt._flat[0] is fl and opt.param_groups[0] is self.group and self.group['params'] is ps and
                fl['param'].data_ptr() == self.base and ps[0].data.data_ptr() == self.base and
                ps[-1].data.data_ptr() == self.base + 4 * self.last_off and fl['m'].data_ptr() == self.m_ptr and
                fl['v'].data_ptr() == self.v_ptr and pk is not None and pk.data_ptr() == self.packed_ptr and
                net.precision == self.precision and opt._withheld is self.withheld and len(opt.guards) == len(self.guards) and
                all(a is b for a, b in zip(opt.guards, self.guards)))

    def next_adam_step(self):
        """The optimizer's step count after this update if all 24 parameters agree on it (one launch, one bias correction),
        else None.  Does not advance anything."""
        state, ps = self.opt.state, self.ps
        steps = self.steps
        if steps is None or state[ps[0]]['step'] is not steps[0] or state[ps[-1]]['step'] is not steps[-1]:
            steps = self.steps = [state[p]['step'] for p in ps]      # (a load_state_dict replaced the tensors)
        s0 = float(steps[0])
        if self.fl.get('uniform_step') != s0 and not all(float(s) == s0 for s in steps):
            return None
        return int(s0) + 1

    def advance(self):
        """What FlatAdam.step leaves on the host after its one launch."""
        torch._foreach_add_(self.steps, 1.0)
        self.fl['uniform_step'] = float(self.steps[0])
        self.opt._guarded_now = bool(self.guards)
        self.opt._launches_per_step = 1
        ps, grads = self.ps, self.grads
        if ps[0].grad is not grads[0] or ps[-1].grad is not grads[-1]:      # (the other route, or a zero_grad, replaced them)
            for p, g in zip(ps, grads):
                p.grad = g


class StepPlan:
    """kind "view": rays of one view per step (TrainStep.step_view); "bank": of `bank`, a train.RayBank (step_batch).
    nets = (coarse, fine), opts = (coarse optimizer, fine optimizer): native networks of one 16-bit precision, each
    stepped by a FlatAdam with one flat group over exactly its 24 parameters (supported() says whether they are)."""

    @staticmethod
    def supported(nets, opts):
        for net, opt in zip(nets, opts):
            if not (isinstance(opt, FlatAdam) and len(opt.param_groups) == 1 and len(opt._flat) == 1 and opt._flat[0] is not None):
                return False
            group = opt.param_groups[0]
            ps, plist = group['params'], net.param_list()
            if len(ps) != len(plist) or any(a is not b for a, b in zip(ps, plist)):
                return False
            if group.get('weight_decay', 0) or group.get('amsgrad') or group.get('maximize'):
                return False
            if any(not (isinstance(g, torch.Tensor) or any(g is n for n in nets)) for g in opt.guards):
                return False
        return opts[0].param_groups[0]['betas'] == opts[1].param_groups[0]['betas'] and \
            opts[0].param_groups[0]['eps'] == opts[1].param_groups[0]['eps']

    def __init__(self, kw, nets, opts, kind, max_rays, H, W, K, near, far, seed, bank=None):
        coarse, fine = nets
        dev = coarse.param_list()[0].device
        self.device = dev
        self.kind = kind
        self.bank = bank
        cfg = self.config = L.StepConfig()
        cfg.max_rays, cfg.n_samples, cfg.n_importance = int(max_rays), int(kw["N_samples"]), int(kw["N_importance"])
        cfg.mode, cfg.color_mode = L.MODE["linear"], L.COLOR[kw["color_mode"]]
        cfg.lindisp, cfg.perturb = int(bool(kw.get("lindisp", False))), int(kw.get("perturb", 0.) > 0.)
        cfg.white_bkgd, cfg.farcolorfix = int(bool(kw.get("white_bkgd", False))), int(bool(kw.get("farcolorfix", False)))
        cfg.raw_noise_std = float(kw.get("raw_noise_std", 0.))
        cfg.zero_tol, cfg.epsilon = float(kw.get("zero_tol", 1e-4)), float(kw.get("epsilon", 1e-3))
        cfg.ndc, cfg.ndc_focal = int(bool(kw.get("ndc", True))), float(K[0][0])
        cfg.H, cfg.W = int(H), int(W)
        cfg.fx, cfg.fy, cfg.cx, cfg.cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
        cfg.near, cfg.far = float(near), float(far)
        cfg.precision, cfg.fwd_kernel = L.PRECISION[coarse.precision], L.FWD_KERNEL
        cfg.input_ch, cfg.input_ch_views = int(coarse.input_ch), int(coarse.hip_view_ch)
        cfg.ray_source = L.STEP_RAYS_BANK if kind == "bank" else L.STEP_RAYS_VIEW
        cfg.n_views = len(bank.i_train) if bank is not None else 0
        group = opts[0].param_groups[0]
        cfg.beta1, cfg.beta2, cfg.adam_eps = float(group['betas'][0]), float(group['betas'][1]), float(group['eps'])
        cfg.seed = int(seed)
        cfg.bank_seed = int(bank.seed) if bank is not None else 0
        nbytes = L.lib().plnerf_train_step_workspace_bytes(ctypes.byref(cfg))
        if nbytes == 0:
            raise ValueError("plnerf_train_step refuses this configuration")
        # zeroed once: the loss kernel's partial sums (every step leaves them zeroed)
        raw = torch.zeros((nbytes + L.STEP_WORKSPACE_ALIGN) // 4 + 1, device=dev, dtype=torch.float32)
        pad = (-raw.data_ptr()) % L.STEP_WORKSPACE_ALIGN
        self.workspace = raw[pad // 4:]
        self.workspace_bytes = nbytes
        self.t_vals = Fn.cpu_linspace(cfg.n_samples, dev)
        self.u_vals = Fn.cpu_linspace(cfg.n_importance, dev)
        # both networks' gradients back to back in one allocation, a GRAD_TAIL behind each (functional._mlp_backward_launch's
        # layout); the backward writes every gradient entry and [0] of the tail, the rest of the tail is never read
        sizes = [sum(o._flat[0]['sizes']) + Fn.GRAD_TAIL for o in opts]
        self.grad_block = torch.zeros(sum(sizes), device=dev, dtype=torch.float32)
        io = self.io = L.StepIo()
        self.slots = (_NetSlot(coarse, opts[0], self.grad_block[:sizes[0]], io.coarse, nets),
                      _NetSlot(fine, opts[1], self.grad_block[sizes[0]:], io.fine, nets))
        io.t_vals, io.u_vals = self.t_vals.data_ptr(), self.u_vals.data_ptr()
        if bank is not None:
            io.views, io.poses, io.images = bank.views.data_ptr(), bank.poses.data_ptr(), bank.images.data_ptr()
            self.bank_ptrs = (io.views, io.poses, io.images)
        self.args = L.StepArgs()
        self.args.loss_scale = 1.0
        self._refs = (ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(self.args), ctypes.c_void_p(self.workspace.data_ptr()))

    def current(self):
        """Does every address the structs hold still belong to the live objects?"""
        if not (self.slots[0].current() and self.slots[1].current()):
            return False
        b = self.bank
        return b is None or (b.views.data_ptr(), b.poses.data_ptr(), b.images.data_ptr()) == self.bank_ptrs

    def adam_steps(self):
        """(coarse, fine) step counts after this update, or None when an optimizer's parameters disagree on theirs."""
        c, f = self.slots[0].next_adam_step(), self.slots[1].next_adam_step()
        return None if (c is None or f is None) else (c, f)

    def run(self, rays, step, ray_id0, lr_coarse, lr_fine, adam_steps, loss_scale=1.0, c2w=None, image=None, crop=None,
            epoch=0, pos0=0):
        """Enqueue one step on the current stream; returns its loss4 = [total, fine, coarse, psnr] (a fresh tensor: an
        earlier step's stays what it was).  c2w: 12 host floats; image: the view's [H, W, 3] fp32 device tensor; crop:
        (r0, c0, rows, cols)."""
        a = self.args
        a.rays, a.step, a.ray_id0 = rays, step, ray_id0
        if self.kind == "view":
            a.c2w[:] = c2w
            a.image = L.dptr(image, "image").value
            a.crop_r0, a.crop_c0, a.crop_rows, a.crop_cols = crop
        else:
            a.epoch, a.pos0 = epoch, pos0
        a.lr_coarse, a.lr_fine = lr_coarse, lr_fine
        a.adam_step_coarse, a.adam_step_fine = adam_steps
        a.loss_scale = loss_scale
        loss4 = torch.empty(4, device=self.device)
        self.io.loss4 = loss4.data_ptr()
        cfg, io, args, ws = self._refs
        L.check(L.lib().plnerf_train_step(cfg, io, args, ws, self.workspace_bytes, L.stream()), "plnerf_train_step")
        self.slots[0].advance()
        self.slots[1].advance()
        return loss4
