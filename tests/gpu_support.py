"""What the GPU tests (tests/test_gpu_*.py) share, each written once: the device and comparison basics and the `P` fixture;
the closed-form networks of both scripts, as create_nerf builds them; the synthetic scenes and depth views; the state
comparisons of the one-call steps; and context managers for the three things those tests switch on and off again.

This is a plain module, so pytest does not rewrite its asserts: every assert here carries its own message."""
import contextlib
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import plnerf_oracle as orc
from run_args import depth_args, depth_args_of, nvs_args

T = torch.from_numpy
ATOL = RTOL = 1e-5


# ----------------------------------------------------------------------------- basics
def dev():
    return torch.device("cuda:0")


def g(x):
    return x.to(dev())


def maxdiff(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max()) if a.numel() else 0.0


def assert_close(a, b, atol=ATOL, rtol=RTOL, what=""):
    a, b = a.detach().cpu(), (b.detach().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)))
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a.double() - b.double()).abs()
    bound = atol + rtol * b.double().abs()
    bad = err > bound
    # NaN positions must agree
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    assert torch.equal(nan_a, nan_b), f"{what}: NaN pattern differs"
    bad = bad & ~nan_a
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} elements off, max abs err {float(err[~nan_a].max()):.3e}"


def same_bits(a, b):
    """torch.equal on the bit patterns: as strict for numbers, and a NaN (the disparity of a ray that met no density is
    1 / max(1e-10, 0 / 0)) equals itself."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def P():
    import plnerf_amd
    return plnerf_amd


# ----------------------------------------------------------------------------- networks and cases
def make_net(P, sd, precision="fp32"):
    net = P.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True,
                 precision=precision)
    net.load_state_dict(sd)
    return net.to(dev())


def ambiguous_rows(sd, pts, vd, eps):
    """Samples with some ReLU pre-activation within eps of zero (fp64 evaluation of the oracle net)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    R, S = pts.shape[:2]
    emb = torch.cat([orc.positional_encoding(pts.reshape(-1, 3).double(), 10),
                     orc.positional_encoding(vd.double()[:, None].expand(R, S, 3).reshape(-1, 3), 4)], -1)
    enc_xyz, enc_dir = emb[:, :63], emb[:, 63:]
    h, bad = enc_xyz, torch.zeros(R * S, dtype=torch.bool)
    for i in range(8):
        pre = torch.nn.functional.linear(h, sd64[f"pts_linears.{i}.weight"], sd64[f"pts_linears.{i}.bias"])
        bad |= (pre.abs() < eps).any(-1)
        h = torch.relu(pre)
        if i == 4:
            h = torch.cat([enc_xyz, h], -1)
    feat = torch.nn.functional.linear(h, sd64["feature_linear.weight"], sd64["feature_linear.bias"])
    pre = torch.nn.functional.linear(torch.cat([feat, enc_dir], -1), sd64["views_linears.0.weight"],
                                     sd64["views_linears.0.bias"])
    bad |= (pre.abs() < eps).any(-1)
    return bad


def quad_case(R, S, seed):
    gen = torch.Generator().manual_seed(seed)
    raw = torch.randn(R, S, 4, generator=gen)
    raw[..., 3] = raw[..., 3] * 4.0 + 1.0
    raw[: R // 2, S // 4: S // 2, 3] += 30.0
    z, _ = torch.sort(2.0 + 4.0 * torch.rand(R, S, generator=gen), -1)
    near, far = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    d = torch.randn(R, 3, generator=gen)
    noise = torch.randn(R, S, generator=gen)
    return raw, z, near, far, d, noise


def g5_batch(gd, p):
    o, d = T(gd[p + "rays_o"]), T(gd[p + "rays_d"])
    return o, d, float(gd[p + "near"]), float(gd[p + "far"])


def nvs_nets(P, precision="f16x3", **over):
    """create_nerf on run_args.nvs_args (N_rand 256, a fresh checkpoint directory) with the closed-form weights:
    (args, render kwargs, fine optimizer, coarse optimizer)."""
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "exp"))
    args = nvs_args(d, precision, **dict(dict(N_rand=256), **over))
    kw, _, start, _, opt, opt_c = P.create_nerf(args, device=dev())
    kw["network_fn"].load_state_dict(orc.closed_form_state_dict(0, False))
    kw["network_fine"].load_state_dict(orc.closed_form_state_dict(1, False))
    return args, kw, opt, opt_c


def depth_nets(args, load=True):
    """depth.create_nerf(args) with (load) the two closed-form depth state dicts in place of its initial weights: create_nerf's
    own tuple (train kwargs, test kwargs, start, grad_vars, optimizer)."""
    from plnerf_amd import depth
    made = depth.create_nerf(args, device=dev())
    if load:
        made[0]["network_fn"].load_state_dict(orc.closed_form_state_dict_depth(0, True))
        made[0]["network_fine"].load_state_dict(orc.closed_form_state_dict_depth(1, True))
    return made


def depth_setup(gd, precision="fp32"):
    """The depth script's networks at a golden file's sampling: (the depth module, kwargs, grad_vars, optimizer)."""
    from plnerf_amd import depth
    kw, _, _, grad_vars, opt = depth_nets(depth_args_of(gd, precision))
    chans = (kw["network_fn"].input_ch, kw["network_fn"].input_ch_views)
    assert chans == (57, 3), ("input channels of the depth network", chans)
    return depth, kw, grad_vars, opt


def depth_step(flags, start=None, seed=5, load=True, **over):
    """A DepthTrainStep on run_args.depth_args (N_rand 256) and depth_nets; `flags` are further keywords of the step
    (one_call, one_call_const, range_check_every); `start` None is the one create_nerf found in the checkpoint directory."""
    from plnerf_amd import depth
    args = depth_args(**dict(dict(N_rand=256), **over))
    kw, _, found, grad_vars, opt = depth_nets(args, load)
    return depth.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, seed=seed, start=found if start is None else start,
                                **flags)


# ----------------------------------------------------------------------------- scenes
def scene(P, n_views, H, W, forward_facing=False, seed=0):
    """(poses, random images, K) of n_views views on a circle, or facing forward with slightly perturbed rotations."""
    gen = torch.Generator().manual_seed(seed)
    if forward_facing:
        poses = torch.eye(4).repeat(n_views, 1, 1)
        for i in range(n_views):
            poses[i, :3, 3] = torch.tensor([0.05 * i - 0.1, 0.02 * i, 0.1])
            poses[i, :3, :3] += 0.01 * torch.randn(3, 3, generator=gen)
    else:
        poses = torch.stack([P.rays.pose_spherical(-180.0 + 360.0 * i / n_views + 7.0, -30.0 + 3.0 * i, 4.0)
                             for i in range(n_views)])
    images = torch.rand(n_views, H, W, 3, generator=gen)
    K = [[1.3 * W + 0.37, 0, W / 2 - 0.25], [0, 1.3 * W - 0.61, H / 2 + 0.5], [0, 0, 1]]
    return poses, images, K


def _circle_poses_and_intrinsics(P, V, H, W):
    poses = torch.stack([P.rays.pose_spherical(-180.0 + 360.0 * i / V + 7.0, -30.0 + 3.0 * i, 4.0) for i in range(V)])
    intr = torch.stack([torch.tensor([1.1 * W + 0.37 * i, 1.2 * W - 0.61 * i, W / 2 - 0.25 + 0.1 * i, H / 2 + 0.5 - 0.2 * i])
                        for i in range(V)])
    return poses, intr


def depth_views(P, n_hyp, seed=0, valid_p=0.5, V=3, H=24, W=32):
    """V views of H x W: random colours, hypotheses in [2, 6), about half the pixels invalid (valid_p None: no mask).  The
    generator draws images, hypotheses, mask, in that order."""
    gen = torch.Generator().manual_seed(seed)
    poses, intr = _circle_poses_and_intrinsics(P, V, H, W)
    images = torch.rand(V, H, W, 3, generator=gen)
    hyp = 2.0 + 4.0 * torch.rand(V, n_hyp, H, W, 1, generator=gen)
    valid = None if valid_p is None else g(torch.rand(V, 1, H, W, 1, generator=gen) < valid_p)
    return P.DepthViews(g(images), g(poses), g(intr), g(hyp), valid, 2.0, 6.0)


def perturbed_depth_views(P, V, H, W, n_hyp, seed=0, pose_rows=4):
    """Not depth_views with other arguments: the generator perturbs the rotations FIRST, then draws images, hypotheses and a
    mask that keeps about 70 % of the pixels; the host tensors come back too."""
    gen = torch.Generator().manual_seed(seed)
    poses, intr = _circle_poses_and_intrinsics(P, V, H, W)
    poses[:, :3, :3] += 0.01 * torch.randn(V, 3, 3, generator=gen)
    poses = poses[:, :pose_rows].contiguous()
    images = torch.rand(V, H, W, 3, generator=gen)
    hyp = 2.0 + 4.0 * torch.rand(V, n_hyp, H, W, 1, generator=gen)
    valid = torch.rand(V, 1, H, W, 1, generator=gen) > 0.3
    views = P.DepthViews(g(images), g(poses), g(intr), g(hyp), g(valid), 2.0, 6.0)
    return views, images, poses, intr, hyp[..., 0], valid.reshape(V, H, W)


# ----------------------------------------------------------------------------- the one-call steps against their yardsticks
def settings(dataset):
    """blender-like: white background, no NDC, near 2 / far 6; llff-like: NDC rays, near 0 / far 1, density noise."""
    llff = dataset == "llff"
    over = dict(dataset=dataset, white_bkgd=not llff, raw_noise_std=1.0 if llff else 0.0)
    return llff, over, ((0.0, 1.0) if llff else (2.0, 6.0))


def size(R):
    """(H, W, precrop) with at least R pixels inside the precrop window."""
    return {256: (20, 26, (8, 9)), 1024: (40, 50, (16, 17)), 4096: (90, 110, (33, 35))}[R]


def nvs_state(ts):
    """Everything a TrainStep leaves behind on the device and in its two optimizers."""
    out = []
    for net, opt in ((ts.nets[0], ts.optimizer_coarse), (ts.nets[1], ts.optimizer)):
        for p in net.parameters():
            st = opt.state[p]
            out.append((p.detach(), st['exp_avg'], st['exp_avg_sq'], p.grad, float(st['step'])))
    return out


def depth_state(ts):
    """Everything a DepthTrainStep leaves behind on the device and in its one optimizer."""
    out = []
    for net in ts.nets:
        for p in net.parameters():
            st = ts.optimizer.state[p]
            out.append((p.detach(), st['exp_avg'], st['exp_avg_sq'], p.grad, float(st['step'])))
    return out


def _assert_same_entries(a_all, b_all, what):
    for k, (a, b) in enumerate(zip(a_all, b_all)):
        for name, x, y in zip(("param", "exp_avg", "exp_avg_sq", "grad"), a[:4], b[:4]):
            assert x is not None and y is not None, (what, k, name, "is None")
            assert torch.equal(x, y), (what, k, name, float((x - y).abs().max()))
        assert a[4] == b[4], (what, k, "step count", a[4], b[4])


def _lrs(opt):
    return [gr['lr'] for gr in opt.param_groups]


def assert_same_nvs_state(ts, ref, what=""):
    assert ts.global_step == ref.global_step, (what, "global_step", ts.global_step, ref.global_step)
    _assert_same_entries(nvs_state(ts), nvs_state(ref), what)
    for name in ("optimizer", "optimizer_coarse"):
        a, b = _lrs(getattr(ts, name)), _lrs(getattr(ref, name))
        assert a == b, (what, name, "learning rates", a, b)


def assert_same_depth_state(ts, ref, what=""):
    assert ts.global_step == ref.global_step, (what, "global_step", ts.global_step, ref.global_step)
    a_all, b_all = depth_state(ts), depth_state(ref)
    assert len(a_all) == len(b_all) == 48, (what, "parameter tensors", len(a_all), len(b_all))
    _assert_same_entries(a_all, b_all, what)
    assert _lrs(ts.optimizer) == _lrs(ref.optimizer), (what, "learning rates", _lrs(ts.optimizer), _lrs(ref.optimizer))
    for name in ("depth_scales", "depth_shifts"):
        x, y = getattr(ts, name).detach(), getattr(ref, name).detach()
        assert torch.equal(x, y), (what, name, float((x - y).abs().max()))


def assert_same_losses(logs):
    for k, ((la, pa), (lb, pb)) in enumerate(zip(*logs)):
        assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(pa, pb), (k, float(la), float(lb), float(pa), float(pb))


def assert_same_depth_step(one, ref, a, b, what=""):
    """What one step_view returned and left, after every step."""
    for name, x, y in zip(("loss", "img_loss", "space_carving"), a[:3], b[:3]):
        assert torch.isfinite(x) and torch.equal(x, y), (what, name, float(x), float(y))
    assert torch.equal(one.last_pixels, ref.last_pixels), (what, "last_pixels")
    for key in ("pred_hyp", "rgb_map", "rgb0", "depth_map", "depth0", "acc_map", "acc0", "disp_map", "disp0", "z_std", "z_vals",
                "z_vals0"):
        assert same_bits(a[3][key], b[3][key]), (what, key)
    assert_same_depth_state(one, ref, what)


# ----------------------------------------------------------------------------- switched on for a block, then put back
class Counting:
    """Stands in for the loaded library: counts every call of a bound entry point."""

    def __init__(self, handle):
        self._handle, self.calls = handle, []

    def __getattr__(self, name):
        fn = getattr(self._handle, name)

        def counted(*args):
            self.calls.append(name)
            return fn(*args)
        return counted


@contextlib.contextmanager
def counting_calls():
    """The package's library handle replaced by a Counting proxy (yielded) for the block."""
    from plnerf_amd import _lib
    real = _lib._lib
    proxy = _lib._lib = Counting(real)
    try:
        yield proxy
    finally:
        _lib._lib = real


@contextlib.contextmanager
def kernel_timer():
    """A functional.KernelTimer watching for the block (the one-call routes stand back while one does)."""
    from plnerf_amd import functional as Fn
    found, Fn.KERNEL_TIMER = Fn.KERNEL_TIMER, Fn.KernelTimer()
    try:
        yield Fn.KERNEL_TIMER
    finally:
        Fn.KERNEL_TIMER = found


@contextlib.contextmanager
def stage_tap(module, tap=None):
    """`module`.STAGE_TAP (plnerf_amd.render's or plnerf_amd.depth's) set to `tap`, a new dict by default, for the block."""
    found, module.STAGE_TAP = module.STAGE_TAP, ({} if tap is None else tap)
    try:
        yield module.STAGE_TAP
    finally:
        module.STAGE_TAP = found
