"""The depth-supervised loop's data feed on a real MI355X (depth.DepthViews, plnerf_select_depth_rays,
plnerf_depth_scale_shift_grad, DepthTrainStep.step_view): the rays against the depth script's full-image get_rays bit for
bit, the pixel sample's distinctness across ranks, the scale / shift gradient against torch autograd of the reference's
compute_space_carving_loss, step_view against DepthTrainStep.__call__, the scale / shift Adam against torch's, the
learning-rate schedule, resuming, and two data-parallel ranks."""
import os
import subprocess
import sys

import pytest
import torch

from abi_support import ROOT
from gpu_support import P, depth_step, perturbed_depth_views

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("H,W,n_hyp,R,pose_rows", [(800, 800, 1, 4096, 4), (800, 800, 3, 1, 4), (37, 53, 3, 37 * 53, 3),
                                                  (37, 53, 1, 37 * 53, 4), (37, 53, 3, 1, 4)])
def test_feed_is_the_depth_scripts_full_image_route(P, H, W, n_hyp, R, pose_rows):
    """Rays, view directions, targets, mask and scaled hypotheses at the chosen pixels: bit-equal to what
    get_ray_batch_from_one_image_hypothesis_idx (:960-1001) and :1120 compute from the full H x W ray grid on the GPU."""
    from plnerf_amd import depth
    V = 3
    views, images, poses, intr, hyp, valid = perturbed_depth_views(P, V, H, W, n_hyp, seed=H + n_hyp, pose_rows=pose_rows)
    scale = (0.8 + 0.4 * torch.rand(V, 1, generator=torch.Generator().manual_seed(1))).to(DEV)
    shift = (0.3 * torch.randn(V, 1, generator=torch.Generator().manual_seed(2))).to(DEV)
    for v in range(V):
        for s_, t_ in ((scale, shift), (None, None)):
            cols, target, th, mask, raw, pix = views.select(v, 5 + v, R, 0, s_, t_, seed=11, want_extras=True)
            assert th.shape == (n_hyp, R, 1) and mask.shape == (R,) and target.shape == (R, 3)
            rows, cs = pix[:, 0].long(), pix[:, 1].long()
            c2w, k = poses[v].to(DEV), intr[v].to(DEV)
            o_ref, d_ref = depth.get_rays(H, W, k, c2w)                      # the full-image route, on the GPU
            vd_ref = d_ref / torch.norm(d_ref, dim=-1, keepdim=True)
            assert torch.equal(cols.rays_d, d_ref[rows, cs]) and torch.equal(cols.rays_o, o_ref[rows, cs]), v
            assert torch.equal(cols.viewdirs, vd_ref[rows, cs]), v
            assert torch.equal(target, images[v].to(DEV)[rows, cs])
            h_ref = hyp[v].to(DEV)[:, rows, cs].unsqueeze(-1)
            assert torch.equal(raw, h_ref)
            want = h_ref if s_ is None else h_ref * s_[v] + t_[v]
            assert torch.equal(th, want), v
            assert torch.equal(mask, valid[v].to(DEV)[rows, cs].float())
            assert (cols.near == 2.0).all() and (cols.far == 6.0).all()
            if R == H * W:      # a full permutation of the view
                assert sorted((rows * W + cs).tolist()) == list(range(H * W))
    # no valid map: every pixel counts
    nv = P.DepthViews(views.images, views.poses, views.intrinsics, views.hypotheses, None, 2.0, 6.0)
    assert (nv.select(0, 0, min(R, 64))[3] == 1.0).all()


def test_pixels_are_distinct_and_ranks_disjoint(P):
    H, W = 37, 53
    views = perturbed_depth_views(P, 2, H, W, 1)[0]
    n = H * W
    for R in (1, 100, n // 2):
        _, _, _, _, _, a = views.select(1, 3, R, 0, want_extras=True)
        _, _, _, _, _, b = views.select(1, 3, n - R, R, want_extras=True)
        ia, ib = (a[:, 0] * W + a[:, 1]).tolist(), (b[:, 0] * W + b[:, 1]).tolist()
        assert len(set(ia)) == R and len(set(ib)) == n - R and not set(ia) & set(ib)
        assert sorted(ia + ib) == list(range(n))
    # the same sample as plnerf_select_rays for (seed, step): the feed's pixels of one step do not depend on the split
    whole = views.select(1, 3, 300, 0, want_extras=True)[5]
    assert torch.equal(torch.cat([views.select(1, 3, 120, 0, want_extras=True)[5],
                                  views.select(1, 3, 180, 120, want_extras=True)[5]]), whole)
    K = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]]
    nvs = P.select_view_rays(H, W, K, torch.eye(4)[:3], None, 300, 2.0, 6.0, seed=0, step=3, want_pixels=True)[2]
    assert torch.equal(nvs, whole)
    assert not torch.equal(views.select(1, 4, 300, 0, want_extras=True)[5], whole)
    with pytest.raises(RuntimeError, match="code -3"):
        views.select(1, 3, 2, n - 1)
    with pytest.raises(RuntimeError, match="code -3"):
        views.select(0, 0, n + 1, 0)


# ------------------------------------------------------------------------------------------ scale / shift gradient
def _reference_space_carving(pred_depth, target_hypothesis, is_joint=False, mask=None, norm_p=2, threshold=0.0):
    """model/run_nerf_helpers.py:52-86, restated."""
    n_rays, n_points = pred_depth.shape
    if target_hypothesis.shape[-1] == 1:
        target_hypothesis_repeated = target_hypothesis.repeat(1, 1, n_points)
    else:
        target_hypothesis_repeated = target_hypothesis
    distances = torch.norm(pred_depth.unsqueeze(-1) - target_hypothesis_repeated.unsqueeze(-1), p=norm_p, dim=-1)
    if mask is not None:
        mask = mask.unsqueeze(0).repeat(distances.shape[0], 1).unsqueeze(-1)
        distances = distances * mask
    if threshold > 0:
        distances = torch.where(distances < threshold, torch.tensor([0.0]).to(distances.device), distances)
    if is_joint:
        quantile_mean = torch.mean(distances, axis=1)
        samples_min = torch.min(quantile_mean, axis=0)[0]
        loss = torch.mean(samples_min, axis=-1)
    else:
        best_hyp = torch.min(distances, dim=0)[0]
        ray_mean = torch.mean(best_hyp, dim=-1)
        loss = torch.mean(ray_mean)
    return loss


def _autograd_ss(pred, raw, scale, shift, view, weight, joint, mask, threshold):
    S = scale.detach().clone().requires_grad_(True)
    T = shift.detach().clone().requires_grad_(True)
    th = raw * S[view] + T[view]
    loss = weight * _reference_space_carving(pred, th, is_joint=joint, mask=mask, threshold=threshold)
    loss.backward()
    return S.grad.reshape(-1), T.grad.reshape(-1)


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("n_hyp", [1, 3])
@pytest.mark.parametrize("threshold,masked,ties", [(0.0, False, False), (0.05, True, False), (0.0, True, True)])
def test_scale_shift_gradient_against_autograd(P, joint, n_hyp, threshold, masked, ties):
    from plnerf_amd import functional as Fn
    gen = torch.Generator().manual_seed(3 + n_hyp + 10 * joint)
    R, NP, V, view = 512, 64, 4, 2
    raw = (2.0 + 4.0 * torch.rand(n_hyp, R, 1, generator=gen)).to(DEV)
    if ties and n_hyp > 1:
        raw[1] = raw[0]        # two hypotheses at equal distance from every sample: the first one is taken
    scale = torch.tensor([[0.9], [1.0], [1.1], [1.05]], device=DEV)
    shift = torch.tensor([[0.1], [0.0], [-0.2], [0.05]], device=DEV)
    th = raw * scale[view] + shift[view]
    pred = (2.0 + 4.0 * torch.rand(R, NP, generator=gen)).to(DEV)
    if ties:
        pred[:, :4] = th[0, :, :1]      # zero distance: torch.norm's gradient is 0 there
    mask = (torch.rand(R, generator=gen) > 0.25).float().to(DEV) if masked else None
    w = 0.007
    g = Fn.depth_scale_shift_grad(pred, th, raw, w, view, V, threshold=threshold, mask=mask, is_joint=joint)
    gs_ref, gt_ref = _autograd_ss(pred, raw, scale, shift, view, w, joint, mask, threshold)
    for got, ref in ((g[0], gs_ref), (g[1], gt_ref)):
        top = float(ref.abs().max())
        assert top > 0
        assert float((got - ref).abs().max()) <= 1e-6 * top, (got, ref)
        assert bool((got[torch.arange(V, device=DEV) != view] == 0).all())
    # the hypothesis choice is the loss kernel's: d loss / d pred_hyp of plnerf_depth_loss, negated and summed, is g_shift
    dummy = torch.zeros(R, 3, device=DEV)
    _, _, _, g_hyp = Fn.depth_loss_and_grads(dummy, None, dummy + 1, pred, th, w, threshold=threshold, mask=mask,
                                             is_joint=joint)
    assert abs(float(g[1, view]) + float(g_hyp.double().sum())) <= 1e-6 * max(float(gt_ref.abs().max()), 1e-30)
    again = Fn.depth_scale_shift_grad(pred, th, raw, w, view, V, threshold=threshold, mask=mask, is_joint=joint)
    assert torch.equal(again, g)                      # bit-reproducible
    if joint:                                          # a given choice (the sharded path's) is the one differentiated
        choice = Fn.joint_choice(pred, th, mask, threshold, None)
        assert torch.equal(Fn.depth_scale_shift_grad(pred, th, raw, w, view, V, threshold=threshold, mask=mask,
                                                     is_joint=True, joint_choice=choice), g)


# --------------------------------------------------------------------------------------------------------- the step
def _step(P, start=0, **over):
    """The step as the loop builds it (its default range poll), at `start` whatever a checkpoint directory holds."""
    return depth_step({}, start=start, **over)


def _params(ts):
    return [p.detach().clone() for n in ts.nets for p in n.parameters()]


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_step_view_equals_call_on_the_selected_batch(P, precision):
    views = perturbed_depth_views(P, 4, 48, 64, 3)[0]
    a, b = _step(P, precision=precision), _step(P, precision=precision)
    for k, img_i in enumerate((2, 0, 3)):
        la = a.step_view(views, img_i)
        cols, target, th, mask = views.select(img_i, k, 256, 0, seed=5)
        lb = b(cols, target, th, mask)
        for x, y in zip(la[:3], lb[:3]):
            assert torch.equal(x, y), (k, x, y)
    assert all(torch.equal(x, y) for x, y in zip(_params(a), _params(b)))
    # freeze_ss = 0 (the default): the scales / shifts never move
    assert torch.equal(a.depth_scales.detach(), torch.ones(4, 1, device=DEV))
    assert torch.equal(a.depth_shifts.detach(), torch.zeros(4, 1, device=DEV))


def test_scale_shift_adam_against_torch(P):
    """freeze_ss > 0: the scale / shift Adam after 5 steps against torch.optim.Adam driven by autograd gradients of the
    reference expression (on the pred_hyp each step produced, the rays it drew, the scales before the step)."""
    V = 4
    views, images, poses, intr, hyp, valid = perturbed_depth_views(P, V, 48, 64, 3, seed=9)
    ts = _step(P, freeze_ss=100, scaleshift_lr=1e-3, scale_init=1.02, shift_init=-0.03, space_carving_threshold=0.01)
    S = (torch.ones(V, 1, device=DEV) * 1.02).requires_grad_(True)
    T = (torch.ones(V, 1, device=DEV) * -0.03).requires_grad_(True)
    opt = torch.optim.Adam(params=(S, T), lr=1e-3)
    ts.init_depth_scale_shift(V, DEV)
    for k, img_i in enumerate((1, 1, 3, 0, 1)):
        scale_before = ts.depth_scales.detach().clone()
        out = ts.step_view(views, img_i)[3]
        pix = ts.last_pixels.long()
        raw = hyp[img_i].to(DEV)[:, pix[:, 0], pix[:, 1]].unsqueeze(-1)
        m = valid[img_i].to(DEV)[pix[:, 0], pix[:, 1]].float()
        opt.zero_grad()
        th = raw * S[img_i] + T[img_i]
        loss = 0.007 * _reference_space_carving(out["pred_hyp"].detach(), th, mask=m, threshold=0.01)
        loss.backward()
        opt.step()
        assert float((scale_before - ts.depth_scales.detach()).abs().max()) > 0 or k == 0
    assert float((ts.depth_scales.detach() - S.detach()).abs().max()) <= 1e-6
    assert float((ts.depth_shifts.detach() - T.detach()).abs().max()) <= 1e-6
    moved = (ts.depth_scales.detach() != 1.02).reshape(-1).tolist()
    assert moved[1] and moved[3] and moved[0] and not moved[2]      # the Adam momentum moves rows after their step only


def test_learning_rate_follows_the_schedule(P):
    views = perturbed_depth_views(P, 2, 32, 32, 1)[0]
    ts = _step(P, start_decay_lrate=2, end_decay_lrate=5, N_rand=64)
    seen = []
    for _ in range(8):
        ts.step_view(views, 1)
        seen.append(ts.optimizer.param_groups[0]["lr"])
    from plnerf_amd import depth
    want, lr = [], 5e-4
    for i in range(1, 9):
        new = depth.learning_rate(i, 5e-4, 2, 5)
        lr = lr if new is None else new
        want.append(lr)
    assert seen == want and seen[0] == 5e-4 and seen[-1] == 5e-4 * 0.1 ** 1.0


def test_resume_draws_the_pixels_of_the_next_iteration(P):
    views = perturbed_depth_views(P, 3, 32, 40, 1)[0]
    k = 3
    a = _step(P, N_rand=64)
    for _ in range(k + 1):
        a.step_view(views, 2)
    b = _step(P, start=k, N_rand=64)
    assert b.global_step == k
    b.step_view(views, 2)
    assert torch.equal(a.last_pixels, b.last_pixels)
    c = _step(P, start=k + 1, N_rand=64)
    c.step_view(views, 2)
    assert not torch.equal(a.last_pixels, c.last_pixels)


# ---------------------------------------------------------------------------------------------------- data parallel
_DP_WORKER = r"""
import hashlib, os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import plnerf_amd as P
from plnerf_amd import dp
from gpu_support import depth_step, perturbed_depth_views
JOINT, N_RAND, STEPS = bool(int(sys.argv[2])), 128, 3
rank, world, _ = dp.init_from_env(backend="gloo")          # every rank on cuda:0; gloo moves CUDA tensors through the host
torch.cuda.set_device(0)
views = perturbed_depth_views(P, 4, 40, 48, 3, seed=4)[0]
over = dict(freeze_ss=100, scaleshift_lr=1e-3, is_joint=JOINT, N_samples=128, N_importance=64)


def make(distributed):
    ts = depth_step({}, start=0, N_rand=N_RAND, **over)
    if distributed:      # (depth_step builds a one-process step: rebuild the same nets as a replica of the group)
        from plnerf_amd import depth
        ts = depth.DepthTrainStep(ts.args, ts.kw, ts.optimizer, ts.grad_vars, distributed=True, seed=5)
    return ts


ts = make(True)
assert ts.bucket is not None and ts.world == world
for k in range(STEPS):
    ts.step_view(views, (1, 3, 1)[k])
    assert ts.bucket.pending() == 0
state = [ts.depth_scales.detach().cpu(), ts.depth_shifts.detach().cpu()]
digest = hashlib.sha256(torch.cat([p.detach().reshape(-1) for n in ts.nets for p in n.parameters()] +
                                  [s.reshape(-1).to(ts.depth_scales.device) for s in state]).cpu().numpy().tobytes()).hexdigest()
gathered = [None] * world
dist.all_gather_object(gathered, digest)
assert all(d == gathered[0] for d in gathered), "replicas diverged"
if rank == 0:
    ts1 = make(False)
    for k in range(STEPS):
        ts1.step_view(views, (1, 3, 1)[k], n_rand=world * N_RAND)
    ds = float((ts1.depth_scales.detach().cpu() - state[0]).abs().max())
    dt = float((ts1.depth_shifts.detach().cpu() - state[1]).abs().max())
    moved = float((state[0] - 1.0).abs().max())
    diff = torch.cat([(p.detach() - q.detach()).abs().reshape(-1) for n, m in zip(ts.nets, ts1.nets)
                      for p, q in zip(n.parameters(), m.parameters())])
    worst, beyond = float(diff.max()), float((diff > 2e-4).double().mean())
    print(f"depth feed dp: scale {ds:.3e} shift {dt:.3e} (moved {moved:.3e}), weights {worst:.3e}, "
          f"fraction beyond 2e-4 {beyond:.2e}")
    assert moved > 0
    assert ds <= 1e-6 and dt <= 1e-6, (ds, dt)
    # Adam moves every weight by ~lr per step whatever the size of its gradient: a weight whose gradient is ~0 may step the
    # other way under the other summation order and separate by up to 2 lr per step (test_gpu_step.py's depth bound,
    # 1.1e-3, is this for about one flip; measured here 2.3e-4 and 1.15e-3).  So: the NVS steps' 2e-4 for all but a few
    # weights, 2 lr per step for those.
    assert worst <= 2 * 5e-4 * STEPS, worst
    assert beyond <= 1e-4, beyond
print(f"rank {rank} ok")
dist.destroy_process_group()
"""


@pytest.mark.parametrize("joint", [False, True])
def test_data_parallel_step_view_two_ranks(P, tmp_path, joint):
    """Two gloo ranks on one GPU, each with its shard (ray ids rank * R ...) of one view per step: the scale / shift
    gradient summed over the ranks with 1 / world, bit-identical replicas (scales and shifts included), and one process
    stepping the global batch within 1e-6 (scales / shifts) and 2e-4 (weights, but for the few whose Adam step
    flips sign: 2 lr per step).  joint: the hypotheses chosen over the
    global batch (functional.joint_choice) are those the scale / shift gradient differentiates."""
    script = tmp_path / "dp_depthfeed_worker.py"
    script.write_text(_DP_WORKER)
    port = 31100 + (os.getpid() % 200) + 200 * joint
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), ROOT, str(int(joint))], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank} failed:\n{out[-3000:]}"
        assert f"rank {rank} ok" in out
    print([l for l in outs[0].splitlines() if l.startswith("depth feed dp")])
