"""The host side of plnerf_train_step (include/plnerf_hip_step.h) and of its piecewise-constant sibling
plnerf_train_step_const (include/plnerf_hip_conststep.h): one library call per optimisation step.

A `StepPlan` owns what the call needs beyond the networks and their optimizers -- the workspace the library carves up,
the flat gradient buffer whose slices become the parameters' `.grad`, the two linspace tables -- and the three structs
of the ABI.  `plnerf_step_config` and `plnerf_step_io` are filled once; a step rewrites `plnerf_step_args` and the one
output pointer.  Device memory that can move under a plan (a network's packed buffer on `.to()` or a precision change,
optim.FlatAdam's flat buffers, the moments after a `load_state_dict`) is looked at before every step with a handful of
pointer compares, the way FlatAdam.step confirms its own layout: `current()` says whether the plan still describes the
live objects, and train.TrainStep builds a new one when it does not.  A plan never steps memory it has not just seen.

`DepthStepPlan` is the same for plnerf_depth_train_step (include/plnerf_hip_depthstep.h).  What the two plans share is
written once: the config fields in onecall's fillers (which the frame renderers use too, and from whose tuples the plan
keys are built), and in `_Plan` below the workspace that serves both modes' entries, the gradient block, the two _NetSlots
and the tail of a step; `_flat_adam_over` is the test both supported() start from.

A rank of a data-parallel run takes the step as its two halves (include/experimental/plnerf_hip_dpstep.h): `run_grads(...)`
enqueues everything up to the complete gradients, the caller sums `grad_block` over the ranks (ONE all-reduce: both networks'
gradients and their status tails lie back to back there), and `apply(1 / world)` enqueues the optimizers.  A plan built with
`data_parallel=True` guards those optimizers by the reduced tails instead of the networks' own status words.
"""
import ctypes

import torch

from . import _lib as L
from . import functional as Fn
from .onecall import aligned_workspace, fill_adam, fill_depth, fill_pinhole, fill_sampling, pinhole, sampling, tables
from .optim import FlatAdam


def plan_key(kw, kind, max_rays, H, W, K, near, far, bank, seed):
    """Everything a plan's config is built from: a step whose key differs gets a plan of its own.  The sampling and camera
    fields are the tuples the config is filled from."""
    return (kind, int(max_rays), id(bank) if bank is not None else None, int(seed), sampling(kw),
            pinhole(kw.get("ndc", True), K, H, W, near, far), L.FWD_KERNEL)


class _NetSlot:
    """One network, its optimizer and the device addresses the plan recorded for them.  The network's 24 parameters are
    parameters `first` .. `first + 23` of the optimizer's one flat group: all of it (an optimizer per network, StepPlan)
    or one half (the depth loop's one optimizer over both networks, DepthStepPlan)."""

    def __init__(self, net, opt, grad_flat, io_net, others, first=0, launches=1, tails=None):
        """tails: a data-parallel step's guard words instead of the optimizer's own -- 1-element views of the reduced range
        status tails in the plan's gradient block (_Plan._build), what FlatAdam.step takes as `guards=` on the Python
        route."""
        self.net, self.opt, self.io = net, opt, io_net
        self.group = opt.param_groups[0]
        self.all_ps = self.group['params']
        self.fl = opt._flat[0]
        self.precision = net.precision
        sizes = self.fl['sizes'][first:first + L.N_PARAM_TENSORS]
        self.ps = self.all_ps[first:first + L.N_PARAM_TENSORS]
        self.n = sum(sizes)
        self.last_off = self.n - sizes[-1]
        self.launches = launches           # plnerf_adam_step launches of one step of `opt` (FlatAdam._launches_per_step)
        lo = 4 * sum(self.fl['sizes'][:first])
        self.flat_ptr = self.fl['param'].data_ptr()
        self.base = self.flat_ptr + lo
        self.m_ptr, self.v_ptr = self.fl['m'].data_ptr() + lo, self.fl['v'].data_ptr() + lo
        self.lo = lo
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
        if tails is not None:
            words = [t.data_ptr() for t in tails]
        self.guarded = bool(words)         # what FlatAdam.step leaves in _guarded_now: was this step's launch guarded at all
        opt._guarded_now = self.guarded
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
        return (opt._flat[0] is fl and opt.param_groups[0] is self.group and self.group['params'] is self.all_ps and
                fl['param'].data_ptr() == self.flat_ptr and ps[0].data.data_ptr() == self.base and
                ps[-1].data.data_ptr() == self.base + 4 * self.last_off and fl['m'].data_ptr() + self.lo == self.m_ptr and
                fl['v'].data_ptr() + self.lo == self.v_ptr and pk is not None and pk.data_ptr() == self.packed_ptr and
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
        self.opt._guarded_now = self.guarded
        self.opt._launches_per_step = self.launches
        ps, grads = self.ps, self.grads
        if ps[0].grad is not grads[0] or ps[-1].grad is not grads[-1]:      # (the other route, or a zero_grad, replaced them)
            for p, g in zip(ps, grads):
                p.grad = g


def _flat_adam_over(opt, params, nets):
    """Is `opt` a FlatAdam with one flat group over exactly `params`, plain Adam (no decay, amsgrad or maximize), guarded
    by nothing but device words and the step's own networks?  What a _NetSlot takes for granted."""
    if not (isinstance(opt, FlatAdam) and len(opt.param_groups) == 1 and len(opt._flat) == 1 and opt._flat[0] is not None):
        return False
    group = opt.param_groups[0]
    ps = group['params']
    if len(ps) != len(params) or any(a is not b for a, b in zip(ps, params)):
        return False
    if group.get('weight_decay', 0) or group.get('amsgrad') or group.get('maximize'):
        return False
    return all(isinstance(g, torch.Tensor) or any(g is n for n in nets) for g in opt.guards)


class _Plan:
    """What both plans are made of behind their filled config."""
    ENTRY = ENTRY_CONST = None      # the entry point and its piecewise-constant sibling: same structs, same workspace
    # (include/experimental/plnerf_hip_dpstep.h: ENTRY + "_grads" / ENTRY_CONST + "_grads", then ENTRY + "_apply" for both)

    def _build(self, cfg, io, args, nets, opts, firsts, launches, guarded_by=None):
        """opts[k], firsts[k]: network k's optimizer and the index of its first parameter in that optimizer's flat group;
        launches: _NetSlot's.  guarded_by: a data-parallel plan -- guarded_by[k] are the networks (0 coarse, 1 fine) whose
        reduced status tails guard network k's optimizer launch, instead of the optimizer's own guards: the tail of network
        j is the float behind its gradients in grad_block, which the caller's SUM all-reduce of grad_block leaves non-zero
        as a 32-bit word exactly when some rank's forward of that network left the half range."""
        dev = self.device = nets[0].param_list()[0].device
        self.config, self.io, self.args = cfg, io, args
        # ONE workspace for both entries (they carve it alike): a constant_init warm-up switches entries between steps on
        # the same memory and the same gradient buffers.  A query answers 0 for the mode its entry does not serve, and for a
        # shape its kernels refuse (N_samples = 2).
        by_mode = {}
        for mode, entry in (("linear", self.ENTRY), ("constant", self.ENTRY_CONST)):
            if hasattr(cfg, "mode"):
                cfg.mode = L.MODE[mode]
            by_mode[mode] = getattr(L.lib(), entry + "_workspace_bytes")(ctypes.byref(cfg))
        self.modes = tuple(m for m, n in by_mode.items() if n)
        nbytes = self.workspace_bytes = max(by_mode.values())
        if nbytes == 0:
            raise ValueError(f"{self.ENTRY} and {self.ENTRY_CONST} refuse this configuration")
        # zeroed once: the loss kernel's partial sums (every step leaves them zeroed)
        self.workspace = aligned_workspace(nbytes, dev, zero=True)
        self.t_vals, self.u_vals = tables(cfg, io, dev)
        # both networks' gradients back to back in one allocation, a GRAD_TAIL behind each (functional._mlp_backward_launch's
        # layout, which FlatAdam.step walks as one run per network); the backward writes every gradient entry and [0] of the
        # tail, the rest of the tail is never read
        n24 = L.N_PARAM_TENSORS
        sizes = [sum(o._flat[0]['sizes'][first:first + n24]) + Fn.GRAD_TAIL for o, first in zip(opts, firsts)]
        self.grad_block = torch.zeros(sum(sizes), device=dev, dtype=torch.float32)
        blocks = (self.grad_block[:sizes[0]], self.grad_block[sizes[0]:])
        self.tails = tuple(b[-Fn.GRAD_TAIL:-Fn.GRAD_TAIL + 1] for b in blocks)      # (coarse, fine): [n_params] of each block
        self.data_parallel = guarded_by is not None
        by = guarded_by if guarded_by is not None else (None, None)
        self.slots = tuple(_NetSlot(nets[k], opts[k], blocks[k], (io.coarse, io.fine)[k], nets, firsts[k], launches,
                                    None if by[k] is None else [self.tails[j] for j in by[k]]) for k in (0, 1))
        self._refs = (ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(self.workspace.data_ptr()))

    def _enqueue(self, mode, suffix=""):
        entry = (self.ENTRY_CONST if mode == "constant" else self.ENTRY) + suffix
        cfg, io, args, ws = self._refs
        L.check(getattr(L.lib(), entry)(cfg, io, args, ws, self.workspace_bytes, L.stream()), entry)

    def _step(self, mode):
        """Enqueue the step the structs describe through `mode`'s entry; leave on the host what FlatAdam.step would."""
        self._enqueue(mode)
        self.slots[0].advance()
        self.slots[1].advance()

    def apply(self, grad_scale=1.0):
        """The second half of a step begun by run_grads (the structs still describe it): the optimizer launches, every
        gradient entry multiplied by grad_scale (1 / world once grad_block holds the SUM over the ranks); leaves on the
        host what FlatAdam.step would."""
        entry = self.ENTRY + "_apply"
        cfg, io, args, _ = self._refs
        L.check(getattr(L.lib(), entry)(cfg, io, args, float(grad_scale), L.stream()), entry)
        self.slots[0].advance()
        self.slots[1].advance()


class StepPlan(_Plan):
    """kind "view": rays of one view per step (TrainStep.step_view); "bank": of `bank`, a train.RayBank (step_batch).
    nets = (coarse, fine), opts = (coarse optimizer, fine optimizer): native networks of one 16-bit precision, each
    stepped by a FlatAdam with one flat group over exactly its 24 parameters (supported() says whether they are)."""
    ENTRY, ENTRY_CONST = "plnerf_train_step", "plnerf_train_step_const"

    @staticmethod
    def supported(nets, opts):
        return all(_flat_adam_over(opt, net.param_list(), nets) for net, opt in zip(nets, opts)) and \
            opts[0].param_groups[0]['betas'] == opts[1].param_groups[0]['betas'] and \
            opts[0].param_groups[0]['eps'] == opts[1].param_groups[0]['eps']

    def __init__(self, kw, nets, opts, kind, max_rays, H, W, K, near, far, seed, bank=None, data_parallel=False):
        """data_parallel: the plan of a rank's share of a step (run_grads, the caller's SUM all-reduce of grad_block,
        apply(1 / world)): the fine optimizer is guarded by both networks' reduced status tails, the coarse one by the
        coarse network's, as train.TrainStep._exchange_and_step guards them."""
        self.kind = kind
        self.bank = bank
        cfg = L.StepConfig()
        fill_sampling(cfg, kw, max_rays, nets[0], seed)      # (mode: _build's queries and every run() write it)
        fill_pinhole(cfg, kw.get("ndc", True), K, H, W, near, far)
        fill_adam(cfg, opts[0].param_groups[0])
        cfg.ray_source = L.STEP_RAYS_BANK if kind == "bank" else L.STEP_RAYS_VIEW
        cfg.n_views = len(bank.i_train) if bank is not None else 0
        cfg.bank_seed = int(bank.seed) if bank is not None else 0
        io, args = L.StepIo(), L.StepArgs()
        self._build(cfg, io, args, nets, opts, (0, 0), 1, ((0,), (0, 1)) if data_parallel else None)
        if bank is not None:
            io.views, io.poses, io.images = bank.views.data_ptr(), bank.poses.data_ptr(), bank.images.data_ptr()
            self.bank_ptrs = (io.views, io.poses, io.images)
        args.loss_scale = 1.0

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

    def run(self, *args, mode="linear", **kw):
        """Enqueue one step on the current stream; returns its loss4 = [total, fine, coarse, psnr] (a fresh tensor: an
        earlier step's stays what it was).  Arguments: _describe's.  mode "constant": the step in piecewise-constant mode
        (plnerf_train_step_const), one of self.modes."""
        loss4 = self._describe(*args, mode=mode, **kw)
        self._step(mode)
        return loss4

    def run_grads(self, *args, mode="linear", **kw):
        """run's first half (plnerf_train_step_grads / plnerf_train_step_const_grads): everything up to the complete
        gradients in grad_block, no optimizer launch and nothing advanced on the host; apply() is the second half.
        Same arguments, same return value."""
        loss4 = self._describe(*args, mode=mode, **kw)
        self._enqueue(mode, "_grads")
        return loss4

    def _describe(self, rays, step, ray_id0, lr_coarse, lr_fine, adam_steps, loss_scale=1.0, c2w=None, image=None, crop=None,
                  epoch=0, pos0=0, mode="linear"):
        """Write one step into the structs.  c2w: 12 host floats; image: the view's [H, W, 3] fp32 device tensor; crop:
        (r0, c0, rows, cols).  Returns the tensor the step's loss4 goes to."""
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
        self.config.mode = L.MODE[mode]
        return loss4


def depth_plan_key(args, kw, max_rays, views, seed):
    """Everything a DepthStepPlan's config is built from (the DepthViews by identity; current() watches their tensors); the
    sampling fields are the tuple the config is filled from."""
    g = lambda name, default: getattr(args, name, default)
    return (int(max_rays), id(views), int(seed), sampling(kw), bool(g("is_joint", False)),
            float(g("space_carving_weight", 0.)), float(g("space_carving_threshold", 0.0)), L.FWD_KERNEL)


class DepthStepPlan(_Plan):
    """The host side of plnerf_depth_train_step (include/plnerf_hip_depthstep.h), StepPlan's sibling for the depth loop:
    nets = (coarse, fine) stepped by ONE FlatAdam `opt` whose one flat group holds exactly their 48 parameters, coarse
    first (depth.create_nerf); `views` a depth.DepthViews; scale, shift: DEPTH_SCALES / DEPTH_SHIFTS [V, 1]; ss_grad,
    ss_m, ss_v [2, V]: their dense gradient and Adam moments.  The workspace is zeroed once (the loss kernel's partials);
    a step's rendered outputs are views of it (outputs()), valid until this plan's next step."""
    ENTRY, ENTRY_CONST = "plnerf_depth_train_step", "plnerf_depth_train_step_const"
    CLIP_VALUE = 0.1      # clip_grad_value_ of run_nerf_sample_based_depth.py:1156

    @staticmethod
    def supported(nets, opt):
        return _flat_adam_over(opt, list(nets[0].param_list()) + list(nets[1].param_list()), nets)

    def __init__(self, args, kw, nets, opt, views, max_rays, seed, input_scale, scale, shift, ss_grad, ss_m, ss_v,
                 ss_betas=(0.9, 0.999), ss_eps=1e-8, data_parallel=False):
        """data_parallel: as StepPlan's; both halves of the one optimizer are guarded by both networks' reduced tails."""
        g = lambda name, default: getattr(args, name, default)
        self.views = views
        cfg = L.DepthStepConfig()
        fill_sampling(cfg, kw, max_rays, nets[0], seed)
        fill_depth(cfg, input_scale, nets[0])
        fill_adam(cfg, opt.param_groups[0])
        cfg.n_views, cfg.H, cfg.W, cfg.n_hyp = views.n_views, views.H, views.W, views.n_hyp
        cfg.pose_rows = int(views.poses.shape[1])
        cfg.near, cfg.far = float(views.near), float(views.far)
        cfg.is_joint = int(bool(g("is_joint", False)))
        cfg.space_carving_weight = float(g("space_carving_weight", 0.))
        cfg.space_carving_threshold = float(g("space_carving_threshold", 0.0))
        cfg.clip_value = self.CLIP_VALUE
        cfg.ss_beta1, cfg.ss_beta2, cfg.ss_adam_eps = float(ss_betas[0]), float(ss_betas[1]), float(ss_eps)
        io = L.DepthStepIo()
        # the flat group's two halves, which FlatAdam.step walks as two runs (one plnerf_adam_step launch each)
        self._build(cfg, io, L.DepthStepArgs(), nets, (opt, opt), (0, L.N_PARAM_TENSORS), 2,
                    ((0, 1), (0, 1)) if data_parallel else None)
        # (both entries carve the workspace alike, so one layout serves either)
        entry = self.ENTRY if "linear" in self.modes else self.ENTRY_CONST
        self.layout = L.DepthStepViews()
        L.check(getattr(L.lib(), entry + "_layout")(ctypes.byref(cfg), ctypes.byref(self.layout)), entry + "_layout")
        self.tensors = (views.images, views.hypotheses, views.valid, views.poses, views.intrinsics, scale, shift, ss_grad,
                        ss_m, ss_v)
        self.ptrs = self._tensor_ptrs()
        (io.images, io.hyp, io.valid, io.poses, io.intrinsics, io.scale, io.shift, io.ss_grad, io.ss_exp_avg,
         io.ss_exp_avg_sq) = self.ptrs

    def _tensor_ptrs(self):
        v = self.views
        live = (v.images, v.hypotheses, v.valid, v.poses, v.intrinsics) + self.tensors[5:]
        return tuple(None if t is None else t.data_ptr() for t in live)

    def current(self):
        """Does every address the structs hold still belong to the live objects (networks, optimizer, the DepthViews'
        tensors, the scale / shift buffers)?"""
        return self.slots[0].current() and self.slots[1].current() and self._tensor_ptrs() == self.ptrs

    def adam_step(self):
        """The optimizer's step count after this update, or None when its 48 parameters disagree on theirs."""
        c, f = self.slots[0].next_adam_step(), self.slots[1].next_adam_step()
        return c if (c is not None and c == f) else None

    def run(self, *args, mode="linear", **kw):
        """Enqueue one step on the current stream; returns its loss5 = [total, image, image (coarse), space carving, psnr]
        (a fresh tensor: an earlier step's stays what it was).  Arguments: _describe's.  mode "constant":
        plnerf_depth_train_step_const (one of self.modes)."""
        loss5 = self._describe(*args, **kw)
        self._step(mode)
        return loss5

    def run_grads(self, *args, mode="linear", **kw):
        """run's first half (plnerf_depth_train_step_grads / _const_grads): up to the complete gradients in grad_block and,
        with ss_step, ss_grad; no optimizer launch, nothing advanced on the host; apply() is the second half."""
        loss5 = self._describe(*args, **kw)
        self._enqueue(mode, "_grads")
        return loss5

    def _describe(self, view, rays, step, ray_id0, lr, adam_step, carve, ss_step=False, ss_lr=0.0, ss_adam_step=0):
        """Write one step into the structs; returns the tensor its loss5 goes to."""
        a = self.args
        a.view, a.rays, a.step, a.ray_id0 = view, rays, step, ray_id0
        a.lr, a.adam_step = lr, adam_step
        a.carve, a.ss_step, a.ss_lr, a.ss_adam_step = int(carve), int(ss_step), ss_lr, ss_adam_step
        loss5 = torch.empty(5, device=self.device)
        self.io.loss5 = loss5.data_ptr()
        return loss5

    def view_of(self, name, shape, dtype=torch.float32):
        """One of the layout's outputs as a tensor over the workspace (no copy)."""
        off = getattr(self.layout, name) // 4
        n = 1
        for s in shape:
            n *= s
        t = self.workspace[off:off + n]
        return (t if dtype == torch.float32 else t.view(dtype)).view(*shape)

    def outputs(self, R):
        """The step's rendered tensors under the reference's keys, as views of the workspace: valid until this plan's next
        step."""
        S, N = self.config.n_samples, self.config.n_importance
        v = self.view_of
        return {'rgb_map': v("rgb", (R, 3)), 'rgb0': v("rgb0", (R, 3)), 'depth_map': v("depth", (R,)), 'depth0': v("depth0", (R,)),
                'acc_map': v("acc", (R,)), 'acc0': v("acc0", (R,)), 'disp_map': v("disp", (R,)), 'disp0': v("disp0", (R,)),
                'pred_hyp': v("pred_hyp", (R, N)), 'z_std': v("z_std", (R,)), 'z_vals': v("z_vals", (R, S + N)),
                'z_vals0': v("z_vals0", (R, S))}
