"""TrainStep(one_call_const=True) and DepthTrainStep(one_call_const=True) on a real MI355X: a step that renders in
piecewise-constant mode -- kw["mode"] == "constant", or a constant_init warm-up step -- is ONE library call
(plnerf_train_step_const / plnerf_depth_train_step_const, include/plnerf_hip_conststep.h) and leaves, bit for bit, what the
Python route leaves: losses, parameters, both Adam moments, the `.grad`s, step counts, learning rates, the depth loop's
pixels, rendered outputs, scales and shifts.  The warm-up switches entries on one plan and one workspace; the fallbacks keep
the Python route; tests/c_abi_const_step_gpu.cpp runs the warm-up without Python and meets the same parameters.

The bound is exact, not measured: both routes launch the same kernels with the same arguments on one stream
(tests/test_gpu_one_call.py's argument), and the one kernel that is new, plnerf_fine_epilogue_const_bwd, equals the launches
it replaces bit for bit (tests/test_gpu_const_bwd.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import c_hosts
from gpu_support import (P, assert_same_depth_state, assert_same_depth_step, assert_same_losses, assert_same_nvs_state,
                         counting_calls, depth_step, depth_views, g, kernel_timer, nvs_nets, scene, settings)
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu
V = 3      # (gpu_support.depth_views' default)
STEPS = 4
# (rays, N_samples, N_importance): the sampler's smallest row (one interior weight) on a batch that is no multiple of the
# 4-ray workgroup; one wave per row; several workgroups of every kernel and a second 64-lane pass of the final quadrature
SHAPES = [(37, 3, 5), (64, 16, 24), (256, 64, 32)]
H, W, PRECROP = 20, 26, (8, 9)      # 16 x 18 = 288 pixels inside the precrop window: every batch above fits


def _make(P, precision, flags, start=0, seed=5, **over):
    args, kw, opt, opt_c = nvs_nets(P, precision, **over)
    return P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=seed, range_check_every=0, **flags)


def _pair(P, precision, flags=None, **over):
    """(the one-call object, the Python-route object) on the same networks and optimizers."""
    return _make(P, precision, dict(one_call_const=True) if flags is None else flags, **over), _make(P, precision, {}, **over)


def _run_views(P, pair, R, llff=False, near=2.0, far=6.0, steps=STEPS, crop_steps=2, each_step=None):
    poses, images, K = scene(P, 4, H, W, forward_facing=llff, seed=3)
    images = g(images)
    logs = ([], [])
    for k in range(steps):
        crop = PRECROP if k < crop_steps else None      # (precrop_iters: the first steps draw from the central window)
        for ts, log in zip(pair, logs):
            log.append(ts.step_view(H, W, K, poses[k % 4][:3, :4], images[k % 4], near=near, far=far, n_rand=R, precrop=crop))
        if each_step is not None:
            each_step(k)
    return logs


# ------------------------------------------------------------------------------ NVS: mode = "constant"
@pytest.mark.parametrize("R,Ns,Ni", SHAPES)
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_step_view_in_constant_mode_is_the_python_route_bit_for_bit(P, precision, R, Ns, Ni):
    one, ref = _pair(P, precision, mode="constant", N_samples=Ns, N_importance=Ni)
    logs = _run_views(P, (one, ref), R)
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "step_view")
    assert one.one_call_const_steps == STEPS and one.one_call_steps == 0 and one.merged_steps == 0
    assert ref.one_call_const_steps == 0 and ref.merged_steps == STEPS


@pytest.mark.parametrize("R,Ns,Ni", SHAPES)
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_step_batch_in_constant_mode_is_the_python_route_bit_for_bit(P, precision, R, Ns, Ni):
    """... through the short last batch of an epoch (3 views x 20 x 26 pixels are no multiple of any R above)."""
    poses, images, K = scene(P, 5, H, W, seed=4)
    bank = P.RayBank(images, poses, K, [0, 2, 3], 2.0, 6.0, seed=9)
    per_epoch = -(-bank.M // R)
    assert bank.M % R != 0
    one, ref = (_make(P, precision, flags, start=per_epoch - 2, mode="constant", N_samples=Ns, N_importance=Ni)
                for flags in (dict(one_call_const=True), {}))
    logs, sizes = ([], []), []
    for _ in range(STEPS):
        for ts, log in zip((one, ref), logs):
            log.append(ts.step_batch(bank, R))
        assert one.last_batch == ref.last_batch
        sizes.append(one.last_batch[2])
    assert sizes == [R, bank.M % R, R, R]
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "step_batch")
    assert one.one_call_const_steps == STEPS and one.one_call_steps == 0


# ------------------------------------------------------------------------------ NVS: the constant_init warm-up
def test_warm_up_switches_entries_on_one_plan_and_one_workspace(P):
    """constant_init = 3: iterations 1 and 2 render in constant mode, 3 to 5 in linear mode.  With both switches on all five
    are one call each, the state equals the all-Python run after EVERY step, and the two entries share one plan: one
    workspace, one flat gradient block."""
    one, ref = _pair(P, "f16x3", dict(one_call=True, one_call_const=True), constant_init=3, N_samples=16, N_importance=24)
    seen = []

    def each_step(k):
        assert_same_nvs_state(one, ref, f"warm-up step {k}")
        plan = one._plan
        seen.append((id(plan), plan.workspace.data_ptr(), plan.grad_block.data_ptr()))
    logs = _run_views(P, (one, ref), 64, steps=5, each_step=each_step)
    assert_same_losses(logs)
    assert one.one_call_const_steps == 2 and one.one_call_steps == 3 and ref.merged_steps == 5
    assert len(set(seen)) == 1, seen
    assert set(one._plan.modes) == {"linear", "constant"}


# ------------------------------------------------------------------------------ NVS: settings that ride along
@pytest.mark.parametrize("variant", ["noise", "det", "ndc", "black"])
def test_settings_ride_along_at_the_smallest_shape(P, variant):
    """Density noise, perturb = 0 (the linspace tables), NDC rays and a black background; the precrop window rides in every
    run of this file (the first two steps draw from it)."""
    llff, over, (near, far) = settings("llff" if variant == "ndc" else "blender")
    over.update(dict(noise=dict(raw_noise_std=1.0), det=dict(perturb=0.0), ndc={}, black=dict(white_bkgd=False))[variant])
    one, ref = _pair(P, "f16x3", mode="constant", N_samples=3, N_importance=5, **over)
    assert bool(one.kw.get("ndc", True)) == llff
    logs = _run_views(P, (one, ref), 37, llff, near, far, steps=3)
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, variant)
    assert one.one_call_const_steps == 3


# ------------------------------------------------------------------------------ NVS: fallbacks
def test_fallbacks_count_no_const_step_and_stay_the_python_route(P):
    render_module = sys.modules["plnerf_amd.render"]      # (the package attribute `render` is the function)

    def run(what, precision="f16x3", flags=None, tap=False, unfused=False, **over):
        one, ref = _pair(P, precision, flags, mode="constant", **dict(dict(N_samples=16, N_importance=24), **over))
        if tap:
            render_module.STAGE_TAP = {}
        if unfused:
            render_module.FUSE_CONST_EPILOGUE = False
        try:
            logs = _run_views(P, (one, ref), 64, steps=2)
        finally:
            render_module.STAGE_TAP = None
            render_module.FUSE_CONST_EPILOGUE = True
        assert_same_losses(logs)
        assert_same_nvs_state(one, ref, what)
        assert one.one_call_const_steps == 0 and one.one_call_steps == 0 and one.global_step == 2, what
    run("fp32", precision="fp32")
    run("stage tap", tap=True)
    run("FUSE_CONST_EPILOGUE off", unfused=True)
    run("one_call_const=False", flags=dict(one_call_const=False))
    run("one_call alone", flags=dict(one_call=True))


def _outcome(step):
    """The step's loss, or the message of the error it raised."""
    try:
        return step()[0]
    except RuntimeError as e:
        return str(e)


def _same_outcome(a, b):
    return torch.equal(a, b) if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) else (isinstance(a, str) and a == b)


def test_two_coarse_samples_do_not_qualify(P):
    """N_samples = 2 leaves the constant-mode sampler no interior weight: the const entry refuses the shape, so the step keeps
    the Python route -- and meets whatever that route does with such a step, a loss or its error, without counting."""
    one, ref = _pair(P, "f16x3", mode="constant", N_samples=2, N_importance=5)
    poses, images, K = scene(P, 2, H, W, seed=3)
    images = g(images)
    assert one._one_call_mode(37) is None
    a, b = (_outcome(lambda: ts.step_view(H, W, K, poses[0][:3, :4], images[0], near=2.0, far=6.0, n_rand=37)) for ts in (one, ref))
    assert _same_outcome(a, b), (a, b)
    assert one.one_call_const_steps == 0 and one.one_call_steps == 0 and one._plan is None
    views = depth_views(P, 3, seed=31)
    d_one, d_ref = (_dstep(P, flags, N_samples=2, N_importance=5) for flags in (dict(one_call_const=True), {}))
    a, b = (_outcome(lambda: ts.step_view(views, 0, 37)) for ts in (d_one, d_ref))
    assert _same_outcome(a, b), (a, b)
    assert d_one.one_call_const_steps == 0 and d_one.one_call_steps == 0 and d_one._plan is None


# ------------------------------------------------------------------------------ NVS: one library call
def test_a_constant_mode_step_is_one_library_call(P):
    one = _make(P, "f16x3", dict(one_call_const=True), mode="constant", N_samples=16, N_importance=24)
    poses, images, K = scene(P, 3, H, W, seed=1)
    images = g(images)
    bank = P.RayBank(images, poses, K, [0, 1, 2], 2.0, 6.0, seed=3)
    step = {"view": lambda k: one.step_view(H, W, K, poses[k % 3][:3, :4], images[k % 3], near=2.0, far=6.0, n_rand=64),
            "bank": lambda k: one.step_batch(bank, 64)}
    for kind in ("view", "bank"):
        step[kind](0)                               # (builds the plan: its size queries are calls too)
        with counting_calls() as proxy:
            for k in range(5):
                step[kind](k)
        assert proxy.calls == ["plnerf_train_step_const"] * 5, proxy.calls
    assert one.one_call_const_steps == 12 and one.one_call_steps == 0


# ------------------------------------------------------------------------------ depth: mode = "constant"
def _dstep(P, flags, seed=5, load=True, **over):
    return depth_step(dict(flags, range_check_every=0), seed=seed, load=load, mode="constant", **over)


@pytest.mark.parametrize("R,Ns,Ni", [(37, 6, 5), (64, 16, 24)])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("n_hyp", [1, 3])
def test_depth_step_view_in_constant_mode_is_the_python_route_bit_for_bit(P, n_hyp, joint, R, Ns, Ni):
    """warm_start_nerf = 2: iterations 1 and 2 run without the space-carving term (the final stage's backward is the
    quadrature's alone), 3 and 4 with it (plnerf_fine_epilogue_const_bwd).  Compared after every step: the three losses, the
    pixels, the twelve rendered outputs, the 48 parameter states, the scales and shifts."""
    views = depth_views(P, n_hyp, seed=R + n_hyp)
    over = dict(N_samples=Ns, N_importance=Ni, warm_start_nerf=2, is_joint=joint)
    one, ref = _dstep(P, dict(one_call_const=True), **over), _dstep(P, {}, **over)
    for k in range(STEPS):
        a, b = one.step_view(views, (2 * k + 1) % V, R), ref.step_view(views, (2 * k + 1) % V, R)
        assert_same_depth_step(one, ref, a, b, f"step {k}")
    assert one.one_call_const_steps == STEPS and one.one_call_steps == 0 and one.merged_steps == 0
    assert ref.one_call_const_steps == 0 and ref.merged_steps == STEPS


def test_depth_scale_shift_stepping_in_constant_mode(P):
    """The scales and shifts step too (freeze_ss = 100).  The yardstick is the same class forced onto the Python route at every
    step (a kernel timer is watching), as in tests/test_gpu_depth_one_call.py: with either switch on the scales' Adam is
    plnerf_depth_ss_adam on both routes, so everything is equal, scales and shifts included."""
    views = depth_views(P, 3, seed=21)
    over = dict(freeze_ss=100, scaleshift_lr=1e-3, scale_init=1.02, shift_init=-0.03, N_samples=6, N_importance=5,
                warm_start_nerf=1, raw_noise_std=0.5)
    one, forced = _dstep(P, dict(one_call_const=True), **over), _dstep(P, dict(one_call_const=True), **over)
    for k in range(STEPS):
        a = one.step_view(views, k % V, 37)
        with kernel_timer():
            b = forced.step_view(views, k % V, 37)
        assert_same_depth_step(one, forced, a, b, f"step {k}")
    assert one.one_call_const_steps == STEPS and forced.one_call_const_steps == 0
    assert one._ss_steps == forced._ss_steps == STEPS - 1      # (iteration 1 is the warm start)
    assert bool((one.depth_scales.detach() != 1.02).any())
    assert torch.equal(one._ss_m, forced._ss_m) and torch.equal(one._ss_v, forced._ss_v)


def test_depth_fallbacks_count_no_const_step(P):
    views = depth_views(P, 3, seed=31)
    for what, flags, over in (("fp32", dict(one_call_const=True), dict(precision="fp32")),
                              ("one_call alone", dict(one_call=True), {}),
                              ("off", dict(one_call_const=False), {})):
        over = dict(dict(N_samples=6, N_importance=5), **over)
        one, ref = _dstep(P, flags, **over), _dstep(P, {}, **over)
        for k in range(2):
            a, b = one.step_view(views, k, 37), ref.step_view(views, k, 37)
            for x, y in zip(a[:3], b[:3]):
                assert torch.equal(x, y), what
        assert_same_depth_state(one, ref, what)
        assert one.one_call_const_steps == 0 and one.one_call_steps == 0 and one.global_step == 2, what


def test_depth_checkpoint_after_const_steps_resumes_on_either_route(P, tmp_path):
    from plnerf_amd import depth
    views = depth_views(P, 3, seed=71)
    R = 37

    def run(first, then, tag):
        d = tmp_path / tag
        os.makedirs(d / "exp")
        over = dict(N_samples=6, N_importance=5, ckpt_dir=str(d), expname="exp")
        ts = _dstep(P, dict(one_call_const=first), **over)
        losses = [ts.step_view(views, k % V, R)[0].clone() for k in range(2)]
        assert ts.one_call_const_steps == (2 if first else 0)
        depth.save_checkpoint(os.path.join(str(d), "exp", "{:06d}.tar".format(ts.global_step)), ts.global_step, ts.nets[0],
                              ts.nets[1], ts.optimizer, ts.depth_scales, ts.depth_shifts)
        ts2 = _dstep(P, dict(one_call_const=then), load=False, no_reload=False, **over)
        assert ts2.global_step == 2
        losses += [ts2.step_view(views, k % V, R)[0].clone() for k in range(2, 4)]
        assert ts2.one_call_const_steps == (2 if then else 0)
        return ts2, losses
    ref, ref_losses = run(False, False, "ref")
    for first, then in ((True, False), (True, True), (False, True)):
        ts, losses = run(first, then, f"r{int(first)}{int(then)}")
        assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses)), (first, then)
        assert_same_depth_state(ts, ref, f"resume {first} {then}")


def test_a_constant_mode_depth_step_is_one_library_call(P):
    views = depth_views(P, 3, seed=41)
    one = _dstep(P, dict(one_call_const=True), N_samples=8, N_importance=8, warm_start_nerf=3, freeze_ss=100, scaleshift_lr=1e-3)
    one.step_view(views, 0, 64)                     # (builds the plan: its size queries are calls too)
    with counting_calls() as proxy:
        for k in range(5):                          # (without the term, with it, with the scales' step)
            one.step_view(views, k % V, 64)
    assert proxy.calls == ["plnerf_depth_train_step_const"] * 5, proxy.calls
    assert one.one_call_const_steps == 6


# ------------------------------------------------------------------------------ the torch-free host
def test_c_host_runs_the_warm_up_without_python(P, tmp_path):
    """tests/c_abi_const_step_gpu.cpp -- the HIP runtime and include/plnerf_hip_conststep.h, nothing else -- runs 2
    plnerf_train_step_const steps and then 2 plnerf_train_step steps on one workspace of max(const, linear) bytes; TrainStep with
    constant_init = 3 on the Python route, from the same hashed weights, image and pose, ends on the same parameters."""
    from plnerf_amd import _lib as L_
    exe = c_hosts.build("c_abi_const_step_gpu", tmp_path)
    R, Ns, Ni, IMG_H, IMG_W, precision = 64, 16, 24, 40, 48, "f16x3"
    out_path = tmp_path / "params.bin"
    run = c_hosts.run(exe, L_.PRECISION[precision], R, Ns, Ni, 2, 2, L_.FWD_KERNEL,
                      c_hosts.write_tables(tmp_path / "tables.bin", Ns, Ni), out_path)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert len(c_hosts.parse_steps(run.stdout)) == 4
    host = torch.from_numpy(np.fromfile(str(out_path), dtype=np.float32))

    args, kw, opt, opt_c = nvs_nets(P, precision, N_samples=Ns, N_importance=Ni, constant_init=3)
    shapes = orc.param_shapes()
    for which, net in enumerate((kw["network_fn"], kw["network_fine"])):
        net.load_state_dict(c_hosts.hashed_state_dict(which, shapes))
    K, c2w, image = c_hosts.step_scene(IMG_H, IMG_W)
    image = g(image)
    ts = P.TrainStep(args, kw, opt, opt_c, start=0, distributed=False, seed=11, range_check_every=0)
    for _ in range(4):
        loss, _ = ts.step_view(IMG_H, IMG_W, K, c2w, image, near=2.0, far=6.0, n_rand=R)
        assert torch.isfinite(loss)
    assert ts.one_call_steps == 0 and ts.one_call_const_steps == 0 and ts.merged_steps == 4
    off = 0
    for which, net in enumerate(ts.nets):
        sd = net.state_dict()
        for name, shape in shapes:
            n = int(np.prod(shape))
            ours = sd[name].detach().cpu().reshape(-1)
            assert torch.equal(host[off:off + n], ours), (which, name, float((host[off:off + n] - ours).abs().max()))
            off += n
    assert off == host.numel()
