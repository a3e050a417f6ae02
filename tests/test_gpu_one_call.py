"""TrainStep(one_call=True) on a real MI355X: every qualifying step is ONE library call (plnerf_train_step) and leaves, bit
for bit, what the existing route leaves -- losses, parameters, both optimizers' moments, the `.grad`s, step counts and
learning rates -- for both ray sources, every 16-bit precision, blender-like and llff-like settings, 256 to 4096 rays,
128 + 64 and 64 + 128 samples, an epoch's short last batch, across the constant_init switch and across a checkpoint;
the range guard withholds a clamped step the same way; and tests/c_abi_step_gpu.cpp trains through the entry without
Python and meets the same losses.

The bound is exact, not measured: both routes launch the same kernels with the same arguments on one stream, and
test_training_step_is_bitwise_reproducible and test_weight_gradients_do_not_depend_on_what_the_workspace_held establish
that those kernels are deterministic and indifferent to what their workspace held."""
import os

import pytest
import torch

import c_hosts
from gpu_support import (P, assert_same_losses, assert_same_nvs_state, counting_calls, g, kernel_timer, nvs_nets, scene, settings,
                         size, stage_tap)
from oracle import plnerf_oracle as orc
from run_args import nvs_args

pytestmark = pytest.mark.gpu
STEPS = 5


def _pair(P, precision, start=0, seed=5, **over):
    """The same networks and optimizers twice: (one-call TrainStep, existing-route TrainStep)."""
    out = []
    for one_call in (True, False):
        args, kw, opt, opt_c = nvs_nets(P, precision, **over)
        out.append(P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=seed, one_call=one_call,
                               range_check_every=0))
    return out


def _run_views(P, pair, R, llff, near, far, steps=STEPS, crop_steps=2, scene_seed=3):
    H, W, precrop = size(R)
    poses, images, K = scene(P, 4, H, W, forward_facing=llff, seed=scene_seed)
    images = g(images)
    logs = ([], [])
    for k in range(steps):
        view = k % 4
        crop = precrop if k < crop_steps else None      # (precrop_iters: the first steps draw from the central window)
        for ts, log in zip(pair, logs):
            log.append(ts.step_view(H, W, K, poses[view][:3, :4], images[view], near=near, far=far, n_rand=R, precrop=crop))
    return logs


CASES = [
    # precision, dataset, rays, N_samples, N_importance
    ("f16x3", "blender", 1024, 128, 64),       # blender_linear.txt
    ("f16x3", "llff", 1024, 128, 64),          # llff_linear.txt
    ("f16x3", "blender", 256, 64, 128),
    ("f16x3", "llff", 256, 64, 128),
    ("f16x3", "blender", 4096, 128, 64),
    ("f16x3", "llff", 4096, 64, 128),
    ("bf16x3", "blender", 1024, 64, 128),
    ("bf16x3", "llff", 256, 128, 64),
    ("f16", "blender", 256, 128, 64),
    ("f16", "llff", 1024, 64, 128),
]


@pytest.mark.parametrize("precision,dataset,R,Ns,Ni", CASES)
def test_step_view_is_the_existing_route_bit_for_bit(P, precision, dataset, R, Ns, Ni):
    llff, over, (near, far) = settings(dataset)
    one, ref = _pair(P, precision, N_samples=Ns, N_importance=Ni, **over)
    assert bool(one.kw.get("ndc", True)) == llff
    logs = _run_views(P, (one, ref), R, llff, near, far)
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "step_view")
    assert one.one_call_steps == STEPS and ref.one_call_steps == 0 and ref.merged_steps == STEPS and one.merged_steps == 0
    # `.grad` are slices of the plan's one flat buffer, in parameter order
    for net in one.nets:
        ps = list(net.parameters())
        assert all(b.grad.data_ptr() == a.grad.data_ptr() + 4 * a.numel() for a, b in zip(ps, ps[1:]))


@pytest.mark.parametrize("precision,dataset,R,Ns,Ni", CASES)
def test_step_batch_is_the_existing_route_bit_for_bit(P, precision, dataset, R, Ns, Ni):
    """... through the short last batch of an epoch: with M bank pixels an epoch has ceil(M / R) steps; the run starts
    two steps before its last one."""
    llff, over, (near, far) = settings(dataset)
    H, W, _ = size(R)
    poses, images, K = scene(P, 5, H, W, forward_facing=llff, seed=4)
    bank = P.RayBank(images, poses, K, [0, 2, 3], near, far, seed=9)
    per_epoch = -(-bank.M // R)
    assert bank.M % R != 0
    start = per_epoch - 3
    one, ref = _pair(P, precision, start=start, N_samples=Ns, N_importance=Ni, **over)
    logs, sizes = ([], []), []
    for _ in range(STEPS):
        for ts, log in zip((one, ref), logs):
            log.append(ts.step_batch(bank, R))
        assert one.last_batch == ref.last_batch
        sizes.append(one.last_batch[2])
    assert sizes == [R, R, bank.M % R, R, R]
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "step_batch")
    assert one.one_call_steps == STEPS and ref.one_call_steps == 0 and ref.merged_steps == STEPS


def test_exact_fp32_keeps_the_existing_route(P):
    """merged_backward_ok holds for the 16-bit precisions only: an fp32 run with one_call=True takes today's route at every
    step, and is today's run."""
    one, ref = _pair(P, "fp32")
    logs = _run_views(P, (one, ref), 256, False, 2.0, 6.0, steps=3)
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "fp32")
    assert one.one_call_steps == 0 and one.merged_steps == 0 and one.global_step == 3


def test_constant_init_steps_fall_back_and_the_switch_is_seamless(P):
    """The reference's warm-up (iterations i < constant_init render in constant mode) is not the entry's business: those
    steps take the existing route, the rest the library's, and the run equals the existing route's across the switch."""
    one, ref = _pair(P, "f16x3", constant_init=3)
    logs = _run_views(P, (one, ref), 256, False, 2.0, 6.0)
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "constant_init")
    qualifying = sum(1 for step in range(STEPS) if not step + 1 < 3)
    assert qualifying == 3 and one.one_call_steps == qualifying and ref.one_call_steps == 0


def test_other_fallbacks_leave_the_count_alone(P):
    """A stage tap, a kernel timer, mode = constant: today's route, silently, per step."""
    import sys
    render_module = sys.modules["plnerf_amd.render"]      # (the package attribute `render` is the function)
    one, ref = _pair(P, "f16x3")
    H, W, _ = size(256)
    poses, images, K = scene(P, 2, H, W, seed=2)
    images = g(images)
    view = lambda ts: ts.step_view(H, W, K, poses[0][:3, :4], images[0], near=2.0, far=6.0, n_rand=256)
    with kernel_timer():
        a, b = view(one), view(ref)
    assert one.one_call_steps == 0 and torch.equal(a[0], b[0])
    a, b = view(one), view(ref)
    assert one.one_call_steps == 1 and torch.equal(a[0], b[0])
    with stage_tap(render_module):
        a, b = view(one), view(ref)
    assert one.one_call_steps == 1 and torch.equal(a[0], b[0])
    one.kw["mode"] = ref.kw["mode"] = "constant"
    a, b = view(one), view(ref)
    assert one.one_call_steps == 1 and torch.equal(a[0], b[0])
    one.kw["mode"] = ref.kw["mode"] = "linear"
    a, b = view(one), view(ref)
    assert one.one_call_steps == 2 and torch.equal(a[0], b[0])
    assert_same_nvs_state(one, ref, "fallbacks")


def test_checkpoint_after_one_call_steps_resumes_on_either_route(P, tmp_path):
    """The reference's checkpoint (both networks, the fine optimizer) written after 3 steps and resumed for 2 more: the run
    is the same whichever route took the first three and whichever takes the last two."""
    H, W, _ = size(256)
    poses, images, K = scene(P, 4, H, W, seed=6)
    images = g(images)

    def run(first_one_call, then_one_call, tag):
        d = tmp_path / tag
        os.makedirs(d / "exp")
        args = nvs_args(str(d), "f16x3", N_rand=256)
        kw, _, start, _, opt, opt_c = P.create_nerf(args, device=torch.device("cuda:0"))
        kw["network_fn"].load_state_dict(orc.closed_form_state_dict(0, False))
        kw["network_fine"].load_state_dict(orc.closed_form_state_dict(1, False))
        ts = P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=5, one_call=first_one_call, range_check_every=0)
        losses = [ts.step_view(H, W, K, poses[k % 4][:3, :4], images[k % 4], near=2.0, far=6.0, n_rand=256)[0] for k in range(3)]
        assert ts.one_call_steps == (3 if first_one_call else 0)
        P.save_checkpoint(P.checkpoint_path(str(d), "exp", ts.global_step), ts.global_step, kw["network_fn"], kw["network_fine"], opt)
        args2 = nvs_args(str(d), "f16x3", N_rand=256, no_reload=False)
        kw2, _, start2, _, opt2, opt_c2 = P.create_nerf(args2, device=torch.device("cuda:0"))
        assert start2 == 3
        ts2 = P.TrainStep(args2, kw2, opt2, opt_c2, start=start2, distributed=False, seed=5, one_call=then_one_call,
                          range_check_every=0)
        losses += [ts2.step_view(H, W, K, poses[k % 4][:3, :4], images[k % 4], near=2.0, far=6.0, n_rand=256)[0] for k in range(3, 5)]
        assert ts2.one_call_steps == (2 if then_one_call else 0)
        return ts2, losses
    ref, ref_losses = run(False, False, "ref")
    for first, then in ((True, False), (True, True), (False, True)):
        ts, losses = run(first, then, f"r{int(first)}{int(then)}")
        assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses)), (first, then)
        assert_same_nvs_state(ts, ref, f"resume {first} {then}")


def test_range_guard_withholds_a_clamped_step_like_the_existing_route(P):
    """A coarse network whose first layer leaves the IEEE-half range (finite weights; the forward clamps and says so): the
    status word is set, both guarded Adam launches change nothing, check_range() raises and winds the step counts back."""
    from plnerf_amd import _lib
    sd = orc.closed_form_state_dict(0, False)
    sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * 6.0e4        # (test_half_modes_flag_range_overflow_...'s network)
    sd["pts_linears.1.weight"] = sd["pts_linears.1.weight"] * 1.0e-5
    assert float(sd["pts_linears.0.weight"].abs().max()) < 65504.0
    one, ref = _pair(P, "f16x3")
    H, W, _ = size(256)
    poses, images, K = scene(P, 2, H, W, seed=8)
    images = g(images)
    for ts in (one, ref):
        ts.nets[0].load_state_dict(sd)
        before = [p.detach().clone() for n in ts.nets for p in n.parameters()]
        ts.step_view(H, W, K, poses[0][:3, :4], images[0], near=2.0, far=6.0, n_rand=256)
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, (p for n in ts.nets for p in n.parameters()))), \
            "a guarded step reached the weights"
        assert int(ts.nets[0].status_word().item()) & _lib.RANGE_ACTIVATION
        assert float(ts.optimizer.state[next(ts.nets[1].parameters())]['step']) == 1.0      # (advanced on the host ...)
        with pytest.raises(FloatingPointError, match="exceeded the IEEE-half range"):
            ts.check_range()
        for net, opt in ((ts.nets[0], ts.optimizer_coarse), (ts.nets[1], ts.optimizer)):
            assert all(float(opt.state[p]['step']) == 0.0 for p in net.parameters())          # (... and wound back)
        assert int(ts.nets[0].status_word().item()) == 0
    assert one.one_call_steps == 1 and ref.one_call_steps == 0
    # with the word cleared and a sane network back in place both routes go on, and agree
    for ts in (one, ref):
        ts.nets[0].load_state_dict(orc.closed_form_state_dict(0, False))
    logs = ([], [])
    for ts, log in zip((one, ref), logs):
        log.append(ts.step_view(H, W, K, poses[1][:3, :4], images[1], near=2.0, far=6.0, n_rand=256))
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "after the guard")
    assert one.one_call_steps == 2


def test_range_poll_runs_on_the_one_call_route(P):
    one, _ = _pair(P, "f16x3")
    one.range_check_every = 2
    polls = []
    check = one.check_range
    one.check_range = lambda: (polls.append(one.global_step), check())
    H, W, _ = size(256)
    poses, images, K = scene(P, 2, H, W, seed=8)
    images = g(images)
    for _ in range(4):
        one.step_view(H, W, K, poses[0][:3, :4], images[0], near=2.0, far=6.0, n_rand=256)
    assert polls == [2, 4] and one.one_call_steps == 4


def test_a_qualifying_step_is_one_library_call(P):
    one, _ = _pair(P, "f16x3")
    H, W, _ = size(1024)
    poses, images, K = scene(P, 3, H, W, seed=1)
    images = g(images)
    bank = P.RayBank(images, poses, K, [0, 1, 2], 2.0, 6.0, seed=3)
    step = {"view": lambda k: one.step_view(H, W, K, poses[k % 3][:3, :4], images[k % 3], near=2.0, far=6.0, n_rand=1024),
            "bank": lambda k: one.step_batch(bank, 1024)}
    for kind in ("view", "bank"):
        step[kind](0)                               # (builds the plan: its size queries are calls too)
        with counting_calls() as proxy:
            for k in range(10):
                step[kind](k)
        assert proxy.calls == ["plnerf_train_step"] * 10, proxy.calls
    assert one.one_call_steps == 22


def test_plan_follows_buffers_that_move(P):
    """A precision change re-allocates the packed buffers; a load_state_dict replaces the optimizer's step tensors: the plan
    is rebuilt or refreshed, never stepped against dead memory, and the run stays the existing route's."""
    one, ref = _pair(P, "f16x3")
    H, W, _ = size(256)
    poses, images, K = scene(P, 2, H, W, seed=12)
    images = g(images)
    logs = ([], [])

    def both(k):
        for ts, log in zip((one, ref), logs):
            log.append(ts.step_view(H, W, K, poses[k % 2][:3, :4], images[k % 2], near=2.0, far=6.0, n_rand=256))
    both(0)
    first_plan = one._plan
    for ts in (one, ref):
        for net in ts.nets:
            net.precision = "bf16x3"
    both(1)
    assert one._plan is not first_plan
    for ts in (one, ref):
        ts.optimizer.load_state_dict(ts.optimizer.state_dict())
    both(2)
    assert_same_losses(logs)
    assert_same_nvs_state(one, ref, "moved buffers")
    assert one.one_call_steps == 3


@pytest.mark.parametrize("precision", ["f16x3"])
def test_c_host_trains_without_python(P, precision, tmp_path):
    """tests/c_abi_step_gpu.cpp -- the HIP runtime and include/plnerf_hip_step.h, nothing else -- runs 5 steps through
    plnerf_train_step; the Python one-call route from the same hashed weights, image and pose meets the same losses and
    parameters, bit for bit (the same entry on the same inputs)."""
    from plnerf_amd import _lib as L_
    exe = c_hosts.build("c_abi_step_gpu", tmp_path)
    R, Ns, Ni, IMG_H, IMG_W = 256, 64, 128, 40, 48
    run = c_hosts.run(exe, L_.PRECISION[precision], R, Ns, Ni, STEPS, L_.FWD_KERNEL,
                      c_hosts.write_tables(tmp_path / "tables.bin", Ns, Ni))
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    host_losses, host_sums = c_hosts.parse_steps(run.stdout), c_hosts.parse_sums(run.stdout, "params")
    assert len(host_losses) == STEPS

    args, kw, opt, opt_c = nvs_nets(P, precision, N_samples=Ns, N_importance=Ni)
    for which, net in enumerate((kw["network_fn"], kw["network_fine"])):
        net.load_state_dict(c_hosts.hashed_state_dict(which, orc.param_shapes()))
    K, c2w, image = c_hosts.step_scene(IMG_H, IMG_W)
    image = g(image)
    ts = P.TrainStep(args, kw, opt, opt_c, start=0, distributed=False, seed=11, one_call=True, range_check_every=0)
    ours = [ts.step_view(IMG_H, IMG_W, K, c2w, image, near=2.0, far=6.0, n_rand=R) for _ in range(STEPS)]
    assert ts.one_call_steps == STEPS
    bits = c_hosts.bits
    for k, ((loss, psnr), (h_loss, h_psnr)) in enumerate(zip(ours, host_losses)):
        assert torch.isfinite(loss) and (bits(loss), bits(psnr)) == (h_loss, h_psnr), (k, float(loss), hex(h_loss))
    sums = [c_hosts.checksum(torch.cat([p.detach().reshape(-1) for p in net.parameters()])) for net in ts.nets]
    assert sums == host_sums
