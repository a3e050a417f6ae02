"""The one-call training steps under data parallelism (include/experimental/plnerf_hip_dpstep.h; stepplan's run_grads / apply;
train.ONE_CALL_DP) on a real MI355X.

What is held, and why the bound is exact everywhere: a one-call step is `grads` then `apply(1.0f)` -- the same launches
with the same arguments in the same order -- so (1) the split on one plan leaves, bit for bit, what run() leaves; (2)
apply(grad_scale) is the launch optim.FlatAdam.step(grad_scale=, guards=) makes, clip and guard words included; (3) a rank of
a data-parallel run on the new route (two library calls around ONE all-reduce of the plan's gradient block) leaves, bit for
bit, what the Python-driven route leaves: both reduce the same per-rank gradients, and a SUM over two ranks is one fp32
addition per entry whichever rank's term comes first.  The yardstick of (3) is the same object with the switch off.  (4) No
entry of the header writes outside the bytes it is given (tests/dpstep_cases.py)."""
import os
import subprocess
import sys

import pytest
import torch

import containment as C
import dpstep_cases as cases
from gpu_support import (P, assert_same_depth_state, assert_same_nvs_state, depth_nets, depth_views, dev, g, nvs_nets, scene, size)
from run_args import depth_args

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 256
SS = dict(freeze_ss=100, scaleshift_lr=1e-3, scale_init=1.02, shift_init=-0.03)


# ----------------------------------------------------------------------------- the steps, driven plan by plan
def _nvs(P, data_parallel=False, **over):
    """A TrainStep (one process) and the view plan of 256 rays of a 20 x 26 view; data_parallel: the plan a rank would have,
    guarded by its gradient block's tails."""
    from plnerf_amd import stepplan
    args, kw, opt, opt_c = nvs_nets(P, **over)
    ts = P.TrainStep(args, kw, opt, opt_c, distributed=False, seed=5, one_call=True, one_call_const=True, range_check_every=0)
    H, W, _ = size(R)
    poses, images, K = scene(P, 4, H, W, seed=3)
    if data_parallel:
        plan = stepplan.StepPlan(ts.kw, ts.nets, (opt_c, opt), "view", R, H, W, K, 2.0, 6.0, ts.seed, None, data_parallel=True)
    else:
        plan = ts._plan_for("view", R, H, W, K, 2.0, 6.0, None)
    assert plan is not None and plan.data_parallel == data_parallel
    return ts, plan, (H, W, poses, g(images))


def _nvs_describe(ts, plan, view, k, mode):
    H, W, poses, images = view
    c2w = [float(v) for v in poses[k % 4][:3, :4].reshape(-1)]
    return ((R, ts.global_step, 0, ts.optimizer_coarse.param_groups[0]['lr'], ts.optimizer.param_groups[0]['lr'], plan.adam_steps()),
            dict(c2w=c2w, image=images[k % 4].contiguous(), crop=(0, 0, H, W), mode=mode))


@pytest.mark.parametrize("mode", ["linear", "constant"])
def test_the_split_is_the_step_nvs(P, mode):
    """run_grads then apply(1.0) against run, on one StepPlan each, three steps."""
    (whole, plan_w, view), (split, plan_s, _) = _nvs(P, mode=mode), _nvs(P, mode=mode)
    assert mode in plan_w.modes
    for k in range(3):
        a, kw = _nvs_describe(whole, plan_w, view, k, mode)
        loss_w = plan_w.run(*a, **kw)
        a, kw = _nvs_describe(split, plan_s, view, k, mode)
        loss_s = plan_s.run_grads(*a, **kw)
        before = [float(s) for s in plan_s.slots[0].steps]
        plan_s.apply(1.0)
        assert [float(s) for s in plan_s.slots[0].steps] == [b + 1.0 for b in before]      # (apply advances, run_grads does not)
        whole._one_call_done(loss_w, mode)
        split._one_call_done(loss_s, mode)
        assert bool(torch.isfinite(loss_w).all()) and torch.equal(loss_w, loss_s), (k, loss_w, loss_s)
        assert_same_nvs_state(split, whole, f"{mode} step {k}")
    assert torch.equal(plan_w.grad_block, plan_s.grad_block)


def _depth(P, data_parallel=False, **over):
    """A DepthTrainStep (one process) and its plan of 256 rays of 24 x 32 views, 64 + 32 samples."""
    from plnerf_amd import depth, stepplan
    args = depth_args(**dict(dict(N_rand=R), **dict(SS, **over)))
    kw, _, found, grad_vars, opt = depth_nets(args)
    ts = depth.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, seed=5, start=found, range_check_every=0, one_call=True,
                              one_call_const=True)
    views = depth_views(P, 3, seed=21)
    ts.init_depth_scale_shift(views.n_views, views.device)
    input_scale = ts._one_call_ok(views, R)
    assert input_scale is not None
    if data_parallel:
        plan = stepplan.DepthStepPlan(ts.args, ts.kw, ts.nets, opt, views, R, ts.seed, input_scale, ts.depth_scales.detach(),
                                      ts.depth_shifts.detach(), ts._ss_grad, ts._ss_m, ts._ss_v, data_parallel=True)
    else:
        plan = ts._plan_for(views, R, input_scale)
    assert plan is not None and plan.data_parallel == data_parallel
    return ts, plan


def _depth_describe(ts, plan, k, ss_step):
    ts._ss_steps += int(ss_step)
    return ((2 * k + 1) % 3, R, ts.global_step, 0, ts.optimizer.param_groups[0]['lr'], plan.adam_step(), True), \
        dict(ss_step=ss_step, ss_lr=1e-3, ss_adam_step=ts._ss_steps)


def _same_depth(a, b, what):
    assert_same_depth_state(a, b, what)
    for name in ("_ss_m", "_ss_v", "_ss_grad"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert a._ss_steps == b._ss_steps, (what, a._ss_steps, b._ss_steps)


@pytest.mark.parametrize("mode", ["linear", "constant"])
def test_the_split_is_the_step_depth(P, mode):
    """... for DepthStepPlan: three steps, the second and third also stepping the scales and shifts."""
    (whole, plan_w), (split, plan_s) = _depth(P, mode=mode), _depth(P, mode=mode)
    assert mode in plan_w.modes
    for k in range(3):
        a, kw = _depth_describe(whole, plan_w, k, k > 0)
        loss_w = plan_w.run(*a, mode=mode, **kw)
        a, kw = _depth_describe(split, plan_s, k, k > 0)
        loss_s = plan_s.run_grads(*a, mode=mode, **kw)
        plan_s.apply(1.0)
        whole.global_step += 1
        split.global_step += 1
        assert bool(torch.isfinite(loss_w).all()) and torch.equal(loss_w, loss_s), (k, loss_w, loss_s)
        _same_depth(split, whole, f"{mode} step {k}")
    assert bool((split.depth_scales.detach() != 1.02).any())
    assert torch.equal(plan_w.grad_block, plan_s.grad_block)


# ----------------------------------------------------------------------------- apply(grad_scale) is FlatAdam's
def _assign_grads(plan):
    for slot in plan.slots:
        for p, grad in zip(slot.ps, slot.grads):
            p.grad = grad


@pytest.mark.parametrize("flagged", [False, True])
def test_apply_is_flat_adams_step_nvs(P, flagged):
    """After one run_grads on a rank's plan: apply(0.25) on one replica, FlatAdam.step(grad_scale=0.25, guards=the tails) on
    the other.  flagged: the fine network's tail set by hand, as the exchange leaves it when some rank's forward clamped --
    the fine optimizer (guarded by both tails) is withheld on both routes and counted once, the coarse one steps."""
    (one, plan_a, view), (ref, plan_b, _) = _nvs(P, data_parallel=True), _nvs(P, data_parallel=True)
    for ts, plan in ((one, plan_a), (ref, plan_b)):
        a, kw = _nvs_describe(ts, plan, view, 0, "linear")
        plan.run_grads(*a, **kw)
        if flagged:
            plan.tails[1].fill_(1.0)
    fine_before = [p.detach().clone() for p in one.nets[1].parameters()]
    coarse_before = [p.detach().clone() for p in one.nets[0].parameters()]
    plan_a.apply(0.25)
    _assign_grads(plan_b)
    ref.optimizer.step(grad_scale=0.25, guards=[plan_b.tails[0], plan_b.tails[1]])
    ref.optimizer_coarse.step(grad_scale=0.25, guards=[plan_b.tails[0]])
    assert_same_nvs_state(one, ref, f"flagged {flagged}")
    for ts in (one, ref):
        assert int(ts.optimizer._withheld.item()) == int(flagged) and int(ts.optimizer_coarse._withheld.item()) == 0
        assert all(torch.equal(a, p.detach()) for a, p in zip(fine_before, ts.nets[1].parameters())) == flagged
        assert not any(torch.equal(a, p.detach()) for a, p in zip(coarse_before, ts.nets[0].parameters()))
        assert ts.optimizer.withheld_steps() == int(flagged) and ts.optimizer_coarse.withheld_steps() == 0
    assert_same_nvs_state(one, ref, f"flagged {flagged}, wound back")


@pytest.mark.parametrize("flagged,grad_scale", [(False, 0.25), (True, 0.25), (False, 64.0)])
def test_apply_is_flat_adams_step_depth(P, flagged, grad_scale):
    """... with clip_value = 0.1 inside the launches, and the scales' and shifts' Adam at the same grad_scale.  flagged: the
    one optimizer over both networks is guarded by both tails -- neither half steps, the two launches count as one step.
    grad_scale 64: the closed-form networks' gradients are small (largest entry about 0.008), so only a large factor puts
    scaled entries outside [-0.1, 0.1], where the clip inside the kernel decides the step."""
    from plnerf_amd import _lib as L
    (one, plan_a), (ref, plan_b) = _depth(P, data_parallel=True), _depth(P, data_parallel=True)
    for ts, plan in ((one, plan_a), (ref, plan_b)):
        a, kw = _depth_describe(ts, plan, 0, True)
        plan.run_grads(*a, **kw)
        if flagged:
            plan.tails[0].fill_(1.0)
    before = [p.detach().clone() for n in one.nets for p in n.parameters()]
    plan_a.apply(grad_scale)
    _assign_grads(plan_b)
    assert plan_b.config.clip_value == pytest.approx(0.1)
    ref.optimizer.step(clip_value=0.1, grad_scale=grad_scale, guards=list(plan_b.tails))
    L.check(L.lib().plnerf_depth_ss_adam(L.dptr(ref.depth_scales.detach()), L.dptr(ref.depth_shifts.detach()), L.dptr(ref._ss_grad),
                                         L.dptr(ref._ss_m), L.dptr(ref._ss_v), 3, 1e-3, 0.9, 0.999, 1e-8, 1, grad_scale, L.stream()),
            "plnerf_depth_ss_adam")
    _same_depth(one, ref, f"flagged {flagged}, grad_scale {grad_scale}")
    for ts in (one, ref):
        assert int(ts.optimizer._withheld.item()) == 2 * int(flagged)
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, (p for n in ts.nets for p in n.parameters()))) == flagged
        assert ts.optimizer.withheld_steps() == int(flagged)
    _same_depth(one, ref, f"flagged {flagged}, wound back")
    largest = max(float((s.grad_flat[:s.n] * grad_scale).abs().max()) for s in plan_a.slots)      # (without the tails)
    print(f"largest scaled gradient entry at grad_scale {grad_scale} (clip_value 0.1): {largest}")
    assert grad_scale < 1.0 or largest > 0.1, "no scaled entry is outside the clip: this case does not test it"


# ----------------------------------------------------------------------------- two gloo ranks on cuda:0
_COMMON = r"""
import os, sys, tempfile, torch, torch.distributed as dist
ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plnerf_amd as P
from plnerf_amd import dp, train
rank, world, _ = dp.init_from_env(backend="gloo")          # every rank on cuda:0; gloo moves CUDA tensors through the host
assert world == 2
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
import gpu_support as G


def both(new, old, fn):
    # the same step on the two replicas, the new route first: every rank issues its collectives in this order
    out = []
    for ts, switch in ((new, True), (old, False)):
        train.ONE_CALL_DP = switch
        out.append(fn(ts))
    train.ONE_CALL_DP = True
    return out


def ranks_agree(ts, what):
    digest = [float(p.detach().double().sum()) for n in ts.nets for p in n.parameters()]
    gathered = [None] * world
    dist.all_gather_object(gathered, digest)
    assert all(d == gathered[0] for d in gathered), what + ": replicas on the two ranks diverged"
"""

_NVS_WORKER = _COMMON + r"""
N_RAND = 128


def make():
    args, kw, opt, opt_c = G.nvs_nets(P, N_rand=N_RAND)
    return P.TrainStep(args, kw, opt, opt_c, distributed=True, seed=3, one_call=True, one_call_const=True, range_check_every=0)


new, old = make(), make()
assert new.bucket is not None and new.world == 2
H, W, _ = G.size(256)
poses, images, K = G.scene(P, 4, H, W, seed=3)
images = images.to(dev)
steps = 0


def view_step(k):
    global steps
    (la, pa), (lb, pb) = both(new, old, lambda ts: ts.step_view(H, W, K, poses[k % 4][:3, :4], images[k % 4], near=2.0, far=6.0,
                                                                n_rand=N_RAND))
    steps += 1
    assert bool(torch.isfinite(la)) and torch.equal(la, lb) and torch.equal(pa, pb), (k, float(la), float(lb))
    G.assert_same_nvs_state(new, old, f"step_view {k}")
    assert new.one_call_steps + new.one_call_const_steps == steps, (new.one_call_steps, new.one_call_const_steps, steps)
    assert old.one_call_steps == old.one_call_const_steps == 0 and old.merged_steps == steps
    assert new.bucket.collectives == 1 and old.bucket.collectives == 1, (new.bucket.collectives, old.bucket.collectives)
    assert new.bucket.pending() == 0


# ---- step_view: 3 linear steps, then 2 steps across a constant_init warm-up boundary (constant, then linear again)
for k in range(3):
    view_step(k)
assert new.one_call_steps == 3
new.args.constant_init = old.args.constant_init = new.global_step + 2
for k in range(3, 5):
    view_step(k)
assert (new.one_call_steps, new.one_call_const_steps) == (4, 1)
new.args.constant_init = old.args.constant_init = 0
ranks_agree(new, "step_view")

# ---- step_batch: three 9 x 19 views, M = 513 = 256 + 256 + 1: global step 5 is the 1-ray batch that ends epoch 1 (rank 0
#      steps it, rank 1 the stand-in ray at weight 0), step 6 opens epoch 2
bposes, bimages, bK = G.scene(P, 3, 9, 19, seed=4)
bank = P.RayBank(bimages, bposes, bK, [0, 1, 2], 2.0, 6.0, seed=9)
assert bank.M == 513 and new.global_step == 5
sizes = []
for k in range(3):
    a, b = both(new, old, lambda ts: ts.step_batch(bank, N_RAND))
    steps += 1
    assert new.last_batch == old.last_batch, (new.last_batch, old.last_batch)
    sizes.append((new.last_batch[2], new.last_batch[4]))
    for x, y in zip(a, b):
        assert G.same_bits(x.reshape(1), y.reshape(1)), (k, float(x), float(y))
    assert bool(torch.isnan(a[0])) == (new.last_batch[2] == 0)
    G.assert_same_nvs_state(new, old, f"step_batch {k}")
    assert new.one_call_steps + new.one_call_const_steps == steps and new.bucket.collectives == 1
assert sizes == [(1 - rank, 1), (128, 256), (128, 256)], sizes
ranks_agree(new, "step_batch")

# ---- the guard: rank 1's fine forward "leaves the half range" (its status word set as the clamping kernel would set it)
before = [[p.detach().clone() for n in ts.nets for p in n.parameters()] for ts in (new, old)]
n_coarse = len(list(new.nets[0].parameters()))
counts = [float(ts.optimizer.state[next(ts.nets[1].parameters())]['step']) for ts in (new, old)]
if rank == 1:
    for ts in (new, old):
        ts.nets[1].status_word().fill_(1)
both(new, old, lambda ts: ts.step_view(H, W, K, poses[0][:3, :4], images[0], near=2.0, far=6.0, n_rand=N_RAND))
steps += 1
assert new.one_call_steps + new.one_call_const_steps == steps
for ts, was, count in zip((new, old), before, counts):
    now = [p.detach() for n in ts.nets for p in n.parameters()]
    assert all(torch.equal(a, p) for a, p in zip(was[n_coarse:], now[n_coarse:])), "a guarded step reached the fine weights"
    assert not any(torch.equal(a, p) for a, p in zip(was[:n_coarse], now[:n_coarse])), "the coarse step was withheld too"
    assert int(ts.nets[1].status_word().item()) == rank, "status words are per rank (the tails carry them)"
    raised = None
    try:
        ts.check_range()
    except FloatingPointError as e:
        raised = str(e)
    assert raised is not None, f"rank {rank} did not raise"
    assert ("another rank" in raised) == (rank == 0), raised
    assert float(ts.optimizer.state[next(ts.nets[1].parameters())]['step']) == count       # wound back
assert float(new._plan.tails[0]) == 0.0 and float(new._plan.tails[1]) == 1.0
G.assert_same_nvs_state(new, old, "guarded step")
ranks_agree(new, "guarded step")
print(f"rank {rank} ok")
dist.destroy_process_group()
"""

_DEPTH_WORKER = _COMMON + r"""
from plnerf_amd import depth
from run_args import depth_args
N_RAND = 128
SS = dict(freeze_ss=100, scaleshift_lr=1e-3, scale_init=1.02, shift_init=-0.03, warm_start_nerf=0, space_carving_weight=0.007)
views = G.depth_views(P, 3, seed=21)


def make(**over):
    args = depth_args(**dict(dict(N_rand=N_RAND), **dict(SS, **over)))
    kw, _, found, grad_vars, opt = G.depth_nets(args)
    return depth.DepthTrainStep(args, kw, opt, grad_vars, distributed=True, seed=5, start=found, range_check_every=0,
                                one_call=True, one_call_const=True)


for over, counted in ((dict(mode="linear"), "one_call_steps"), (dict(mode="constant"), "one_call_const_steps"),
                      (dict(mode="linear", is_joint=True), None)):
    new, old = make(**over), make(**over)
    assert new.bucket is not None
    for k in range(3):
        a, b = both(new, old, lambda ts: ts.step_view(views, (2 * k + 1) % 3, N_RAND))
        G.assert_same_depth_step(new, old, a, b, f"{over} step {k}")
        for name in ("_ss_m", "_ss_v", "_ss_grad"):
            assert torch.equal(getattr(new, name), getattr(old, name)), (over, k, name)
        assert new._ss_steps == old._ss_steps == k + 1
        assert new.bucket.collectives == 1 and old.bucket.collectives == 1
    assert bool((new.depth_scales.detach() != 1.02).any()), "the scales never stepped"
    assert old.one_call_steps == old.one_call_const_steps == 0 and old.merged_steps == 3
    if counted is None:      # is_joint: a collective in the middle of the forward -- the Python-driven route, not counted
        assert new.one_call_steps == new.one_call_const_steps == 0 and new.merged_steps == 3
    else:
        assert getattr(new, counted) == 3 and new.one_call_steps + new.one_call_const_steps == 3 and new.merged_steps == 0
    ranks_agree(new, str(over))
    gathered = [None] * world
    dist.all_gather_object(gathered, new.depth_scales.detach().cpu().tolist())
    assert gathered[0] == gathered[1], "the ranks' depth scales diverged"
    del new, old
    torch.cuda.empty_cache()
print(f"rank {rank} ok")
dist.destroy_process_group()
"""


def _run_two_ranks(tmp_path, name, program, port_base, limit=280):
    """Two ranks of one worker program, spawned as tests/test_gpu_step.py spawns its ranks, each under a time limit of its
    own."""
    script = tmp_path / name
    script.write_text(program)
    port = port_base + (os.getpid() % 200)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, str(script), ROOT], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=limit + 30)[0] for p in procs]
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank} failed ({p.returncode}):\n{out[-3000:]}"
        assert f"rank {rank} ok" in out


def test_two_ranks_take_the_one_call_route_nvs(P, tmp_path):
    """TrainStep(distributed=True, one_call=True, one_call_const=True) on two gloo ranks, the switch on against the switch off:
    step_view through a constant_init boundary, step_batch through a 1-ray global batch (a rank left without rays) into the
    next epoch, and the range guard travelling in the gradient block's tails."""
    _run_two_ranks(tmp_path, "dp_one_call_nvs_worker.py", _NVS_WORKER, 27300)


def test_two_ranks_take_the_one_call_route_depth(P, tmp_path):
    """DepthTrainStep on two gloo ranks, linear and constant mode, every step also stepping the scales and shifts (their
    gradient goes through its own small all-reduce); is_joint keeps the Python-driven route and is not counted."""
    _run_two_ranks(tmp_path, "dp_one_call_depth_worker.py", _DEPTH_WORKER, 27700)


# ----------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("case_id,build", cases.all_cases(), ids=[c for c, _ in cases.all_cases()])
def test_no_entry_writes_outside_its_buffers(P, case_id, build):
    C.run_case(P._lib, build(P._lib), dev())
