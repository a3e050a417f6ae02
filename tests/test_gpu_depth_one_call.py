"""DepthTrainStep(one_call=True) on a real MI355X: every qualifying step_view is ONE library call
(plnerf_depth_train_step) and leaves, bit for bit, what the existing route leaves -- losses, all 48 parameters, both
moments, the `.grad`s, step counts, the step's pixels and depth hypotheses -- for every 16-bit precision, one and three depth
hypotheses per pixel, batches below one tile, of several workgroups and of the whole view, across the switch-on of the
space-carving term and the stepping of the depth scales and shifts; plnerf_depth_ss_adam meets torch.optim.Adam; the
fallbacks, the range guard, moved buffers and a checkpoint behave as on the existing route; and
tests/c_abi_depth_step_gpu.cpp trains through the entry without Python and meets the same parameters.

The bound between the two routes is exact, not measured: both launch the same kernels with the same arguments on one
stream (tests/test_gpu_one_call.py's argument).  Against torch.optim.Adam the bound is the one
tests/test_gpu_parity.py::test_fused_adam_matches_torch holds for plnerf_adam_step (atol = rtol = 1e-6): the same fp32
expressions, torch's own kernel fusing some of them differently."""
import os

import numpy as np
import pytest
import torch

import c_hosts
from gpu_support import (P, assert_same_depth_state, assert_same_depth_step, counting_calls, depth_state, depth_step,
                         depth_views, kernel_timer, stage_tap)
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, H, W = 3, 24, 32      # (gpu_support.depth_views' defaults)
STEPS = 4
# (rays, N_samples, N_importance): 222 and 407 MLP rows -- no multiple of the 32-row tile, below the saved planes' 256-row
# padding; several workgroups of every kernel; the sample covers the whole view
SHAPES = [(37, 6, 5), (256, 64, 32), (H * W, 8, 8)]


def _step(P, one_call, seed=5, load=True, **over):
    return depth_step(dict(range_check_every=0, one_call=one_call), seed=seed, load=load, **over)


def _pair(P, **over):
    return _step(P, True, **over), _step(P, False, **over)


def _run(one, ref, views, R, steps=STEPS):
    for k in range(steps):
        a = one.step_view(views, (2 * k + 1) % V, R)
        b = ref.step_view(views, (2 * k + 1) % V, R)
        assert_same_depth_step(one, ref, a, b, f"step {k}")


# ------------------------------------------------------------------------------ 1. bit equality, scales frozen
@pytest.mark.parametrize("R,Ns,Ni", SHAPES)
@pytest.mark.parametrize("n_hyp", [1, 3])
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3", "f16"])
def test_step_view_is_the_existing_route_bit_for_bit(P, precision, n_hyp, R, Ns, Ni):
    """freeze_ss = 0; warm_start_nerf = 2: iterations 1 and 2 run without the space-carving term, 3 and 4 with it."""
    views = depth_views(P, n_hyp, seed=R + n_hyp)
    one, ref = _pair(P, precision=precision, N_samples=Ns, N_importance=Ni, warm_start_nerf=2)
    _run(one, ref, views, R)
    assert one.one_call_steps == STEPS and ref.one_call_steps == 0 and ref.merged_steps == STEPS and one.merged_steps == 0
    assert torch.equal(one.depth_scales.detach(), torch.ones(V, 1, device=DEV))
    # `.grad` are slices of the plan's one flat buffer, in parameter order
    for net in one.nets:
        ps = list(net.parameters())
        assert all(b.grad.data_ptr() == a.grad.data_ptr() + 4 * a.numel() for a, b in zip(ps, ps[1:]))


VARIANTS = {
    "joint": dict(is_joint=True),
    "joint_threshold": dict(is_joint=True, space_carving_threshold=0.05, warm_start_nerf=2),
    "noise_1": dict(raw_noise_std=1.0),
    "noise_half": dict(raw_noise_std=0.5, is_joint=True),
    "det": dict(perturb=0.0),
    "det_joint": dict(perturb=0.0, is_joint=True, raw_noise_std=0.5),
    "black_left": dict(white_bkgd=False, color_mode="left"),
    "lindisp_threshold": dict(lindisp=True, space_carving_threshold=0.05),
    "no_mask": dict(valid_p=None),
}


@pytest.mark.parametrize("R,Ns,Ni,precision,n_hyp", [(37, 6, 5, "f16x3", 3), (256, 64, 32, "bf16x3", 1)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_settings_of_the_depth_script_bit_for_bit(P, variant, R, Ns, Ni, precision, n_hyp):
    over = dict(VARIANTS[variant])
    views = depth_views(P, n_hyp, seed=11, valid_p=over.pop("valid_p", 0.5))
    one, ref = _pair(P, precision=precision, N_samples=Ns, N_importance=Ni, **over)
    _run(one, ref, views, R, steps=3)
    assert one.one_call_steps == 3


# ------------------------------------------------------------------------------ 2. scale / shift stepping
SS = dict(freeze_ss=100, scaleshift_lr=1e-3, scale_init=1.02, shift_init=-0.03)


@pytest.mark.parametrize("R,Ns,Ni,n_hyp,joint", [(37, 6, 5, 3, False), (256, 64, 32, 1, True), (H * W, 8, 8, 3, True)])
def test_scale_shift_stepping_one_call_against_its_own_fallback(P, R, Ns, Ni, n_hyp, joint):
    """The same object class forced onto the existing route at every step (a kernel timer is watching): one arithmetic for
    the scales' Adam, so everything is equal, scales and shifts included."""
    views = depth_views(P, n_hyp, seed=21)
    over = dict(SS, N_samples=Ns, N_importance=Ni, is_joint=joint, warm_start_nerf=1)
    one, forced = _step(P, True, **over), _step(P, True, **over)
    for k in range(STEPS):
        a = one.step_view(views, k % V, R)
        with kernel_timer():
            b = forced.step_view(views, k % V, R)
        assert_same_depth_step(one, forced, a, b, f"step {k}")
    assert one.one_call_steps == STEPS and forced.one_call_steps == 0
    assert one._ss_steps == forced._ss_steps == STEPS - 1      # (iteration 1 is the warm start)
    moved = (one.depth_scales.detach() != 1.02).reshape(-1)
    assert bool(moved.any()) and torch.equal(one._ss_m, forced._ss_m) and torch.equal(one._ss_v, forced._ss_v)


@pytest.mark.parametrize("R,Ns,Ni,n_hyp", [(37, 6, 5, 3), (256, 64, 32, 1)])
def test_scale_shift_stepping_against_torch_adam(P, R, Ns, Ni, n_hyp):
    """After the FIRST stepping iteration networks and losses are equal to the one_call=False run (the scales only reach the
    next step's target_h) and the scales and shifts are within 1e-6 of torch.optim.Adam's."""
    views = depth_views(P, n_hyp, seed=22)
    one, ref = _pair(P, N_samples=Ns, N_importance=Ni, **SS)
    a, b = one.step_view(views, 1, R), ref.step_view(views, 1, R)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for (pa, ma, va, ga, sa), (pb, mb, vb, gb, sb) in zip(depth_state(one), depth_state(ref)):
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and sa == sb
    assert one.one_call_steps == 1 and ref.optimizer_ss is not None and one.optimizer_ss is None
    for x, y in ((one.depth_scales, ref.depth_scales), (one.depth_shifts, ref.depth_shifts)):
        print("scale / shift |ours - torch| max:", float((x.detach() - y.detach()).abs().max()))
        assert torch.allclose(x.detach(), y.detach(), atol=1e-6, rtol=1e-6)
    assert float((one.depth_scales.detach()[1] - 1.02).abs()) > 0 and float((ref.depth_scales.detach()[1] - 1.02).abs()) > 0


# ------------------------------------------------------------------------------ 3. the new kernel alone
@pytest.mark.parametrize("n_views", [5, 300])      # (300: more entries than the one workgroup has threads)
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_depth_ss_adam_against_torch(P, n_views, grad_scale):
    from plnerf_amd import _lib as L
    gen = torch.Generator().manual_seed(3)
    scale = (1.0 + 0.1 * torch.rand(n_views, 1, generator=gen)).to(DEV)
    shift = (0.1 * torch.randn(n_views, 1, generator=gen)).to(DEV)
    S, T = scale.clone().requires_grad_(True), shift.clone().requires_grad_(True)
    opt = torch.optim.Adam(params=(S, T), lr=1e-3)
    m, v = torch.zeros(2, n_views, device=DEV), torch.zeros(2, n_views, device=DEV)
    for step in range(1, 4):
        # a gradient that is zero for all but one view: the others still move by their moments, as in torch
        g = torch.zeros(2, n_views, device=DEV)
        g[:, step % n_views] = torch.tensor([0.37 * step, -1.3 / step], device=DEV) * 8.0
        L.check(L.lib().plnerf_depth_ss_adam(L.dptr(scale), L.dptr(shift), L.dptr(g), L.dptr(m), L.dptr(v), n_views, 1e-3, 0.9,
                                             0.999, 1e-8, step, grad_scale, L.stream()), "plnerf_depth_ss_adam")
        S.grad, T.grad = (g[0] * grad_scale).reshape(-1, 1), (g[1] * grad_scale).reshape(-1, 1)
        opt.step()
    for ours, ref, init in ((scale, S, 1.0), (shift, T, 0.0)):
        err = float((ours - ref.detach()).abs().max())
        print("plnerf_depth_ss_adam |ours - torch| max:", err)
        assert torch.allclose(ours, ref.detach(), atol=1e-6, rtol=1e-6), err
    touched = [1, 2, 3] if n_views > 3 else []
    assert all(float((scale[k] - S.detach()[k]).abs()) <= 1e-6 for k in touched)
    assert torch.equal(scale[4], (S.detach()[4])) and float(m[0, 4]) == 0.0      # a view that never had a gradient stays put
    assert float((m[0, 1]).abs()) > 0 and float(v[1, 3]) > 0


# ------------------------------------------------------------------------------ 4. fallbacks
def test_fp32_and_a_bounding_box_keep_the_existing_route(P):
    views = depth_views(P, 3, seed=31)
    for over in (dict(precision="fp32"), dict(bb_scale=1.5)):
        one, ref = _pair(P, N_samples=6, N_importance=5, **over)
        for k in range(2):
            a, b = one.step_view(views, k, 37), ref.step_view(views, k, 37)
            for x, y in zip(a[:3], b[:3]):
                assert torch.equal(x, y), over
        assert_same_depth_state(one, ref, str(over))
        assert one.one_call_steps == 0 and one.global_step == 2


def test_fallbacks_leave_the_count_alone_and_switch_seamlessly(P):
    """A stage tap and a caller-made batch through __call__ take the existing route; the next qualifying step is one call
    again, and the run equals the all-fallback run."""
    from plnerf_amd import depth
    views = depth_views(P, 3, seed=32)
    one, ref = _pair(P, N_samples=6, N_importance=5, warm_start_nerf=1)
    R = 37
    a, b = one.step_view(views, 0, R), ref.step_view(views, 0, R)
    assert one.one_call_steps == 1 and torch.equal(a[0], b[0])
    with stage_tap(depth):
        a, b = one.step_view(views, 1, R), ref.step_view(views, 1, R)
    assert one.one_call_steps == 1 and torch.equal(a[0], b[0])
    assert_same_depth_state(one, ref, "tap")
    a, b = one.step_view(views, 2, R), ref.step_view(views, 2, R)
    assert one.one_call_steps == 2
    assert_same_depth_step(one, ref, a, b, "after the tap")
    outs = []
    for ts in (one, ref):
        cols, target, th, mask = views.select(1, ts.global_step, R, 0, scale=ts.depth_scales, shift=ts.depth_shifts, seed=5)
        outs.append(ts(cols, target, th, mask))
    assert one.one_call_steps == 2 and torch.equal(outs[0][0], outs[1][0]) and "raw" in outs[0][3]
    a, b = one.step_view(views, 0, R), ref.step_view(views, 0, R)
    assert one.one_call_steps == 3 and one.global_step == 5
    assert_same_depth_step(one, ref, a, b, "after __call__")


# ------------------------------------------------------------------------------ 5. one library call
def test_a_qualifying_step_is_one_library_call(P):
    views = depth_views(P, 3, seed=41)
    one = _step(P, True, N_samples=8, N_importance=8, warm_start_nerf=3, **SS)
    one.step_view(views, 0, 256)                    # (builds the plan: its size queries are calls too)
    with counting_calls() as proxy:
        for k in range(8):                          # (without the term, with it, with the scales' step)
            one.step_view(views, k % V, 256)
    assert proxy.calls == ["plnerf_depth_train_step"] * 8, proxy.calls
    assert one.one_call_steps == 9 and one._ss_steps == 6


# ------------------------------------------------------------------------------ 6. range guard
def test_range_guard_withholds_a_clamped_step_like_the_existing_route(P):
    """A coarse network whose first layer leaves the IEEE-half range: the status word is set, both guarded Adam launches
    change nothing and count themselves, check_range() raises at the poll and winds the step counts back."""
    from plnerf_amd import _lib
    sd = orc.closed_form_state_dict_depth(0, True)
    sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * 6.0e4
    sd["pts_linears.1.weight"] = sd["pts_linears.1.weight"] * 1.0e-5
    assert float(sd["pts_linears.0.weight"].abs().max()) < 65504.0
    views = depth_views(P, 3, seed=51)
    one, ref = _pair(P, N_samples=6, N_importance=5)
    withheld = []
    for ts in (one, ref):
        ts.nets[0].load_state_dict(sd)
        before = [p.detach().clone() for n in ts.nets for p in n.parameters()]
        ts.step_view(views, 0, 37)
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, (p for n in ts.nets for p in n.parameters()))), \
            "a guarded step reached the weights"
        assert int(ts.nets[0].status_word().item()) & _lib.RANGE_ACTIVATION
        assert float(ts.optimizer.state[next(ts.nets[1].parameters())]['step']) == 1.0      # (advanced on the host ...)
        withheld.append((int(ts.optimizer._withheld.item()), ts.optimizer._launches_per_step))
        ts.range_check_every = 2
        with pytest.raises(FloatingPointError, match="exceeded the IEEE-half range"):
            ts.step_view(views, 1, 37)              # (global step 2: the poll)
        assert ts.global_step == 2
        assert all(float(ts.optimizer.state[p]['step']) == 0.0 for n in ts.nets for p in n.parameters())   # (... and wound back)
        assert int(ts.nets[0].status_word().item()) == 0
    assert withheld[0] == withheld[1] == (2, 2)
    assert one.one_call_steps == 2 and ref.one_call_steps == 0


# ------------------------------------------------------------------------------ 7. buffers that move
def test_plan_follows_buffers_that_move(P):
    views = depth_views(P, 3, seed=61)
    one, ref = _pair(P, N_samples=6, N_importance=5)
    R = 37

    def both(k, vs):
        a, b = one.step_view(vs, k % V, R), ref.step_view(vs, k % V, R)
        assert_same_depth_step(one, ref, a, b, f"step {k}")
    both(0, views)
    first = one._plan
    for ts in (one, ref):
        for net in ts.nets:
            net.to(DEV)
    both(1, views)
    assert one._plan is first                       # (nothing moved)
    for ts in (one, ref):
        for net in ts.nets:
            net.precision = "bf16x3"
    both(2, views)
    assert one._plan is not first
    second = one._plan
    for ts in (one, ref):
        ts.optimizer.load_state_dict(ts.optimizer.state_dict())
    both(3, views)
    replaced = depth_views(P, 3, seed=61)
    both(4, replaced)
    assert one._plan is not second
    third = one._plan
    replaced.images = replaced.images.clone()       # the same object, one tensor re-allocated
    both(5, replaced)
    assert one._plan is not third and one.one_call_steps == 6


# ------------------------------------------------------------------------------ 8. checkpoint
def test_checkpoint_after_one_call_steps_resumes_on_either_route(P, tmp_path):
    from plnerf_amd import depth
    views = depth_views(P, 3, seed=71)
    R = 37

    def run(first_one_call, then_one_call, tag):
        d = tmp_path / tag
        os.makedirs(d / "exp")
        over = dict(N_samples=6, N_importance=5, ckpt_dir=str(d), expname="exp")
        ts = _step(P, first_one_call, **over)
        losses = [ts.step_view(views, k % V, R)[0].clone() for k in range(2)]
        assert ts.one_call_steps == (2 if first_one_call else 0)
        depth.save_checkpoint(os.path.join(str(d), "exp", "{:06d}.tar".format(ts.global_step)), ts.global_step, ts.nets[0],
                              ts.nets[1], ts.optimizer, ts.depth_scales, ts.depth_shifts)
        ts2 = _step(P, then_one_call, load=False, no_reload=False, **over)
        assert ts2.global_step == 2
        losses += [ts2.step_view(views, k % V, R)[0].clone() for k in range(2, 4)]
        assert ts2.one_call_steps == (2 if then_one_call else 0)
        return ts2, losses
    ref, ref_losses = run(False, False, "ref")
    for first, then in ((True, False), (True, True), (False, True)):
        ts, losses = run(first, then, f"r{int(first)}{int(then)}")
        assert all(torch.equal(a, b) for a, b in zip(losses, ref_losses)), (first, then)
        assert_same_depth_state(ts, ref, f"resume {first} {then}")


# ------------------------------------------------------------------------------ 9. the torch-free host
@pytest.mark.parametrize("precision,n_hyp", [("f16x3", 3)])
def test_c_host_trains_without_python(P, precision, n_hyp, tmp_path):
    """tests/c_abi_depth_step_gpu.cpp -- the HIP runtime and include/plnerf_hip_depthstep.h, nothing else -- runs 3 steps
    through plnerf_depth_train_step; step_view(one_call=True) from the same hashed weights, views and hypotheses meets the
    same losses, parameters, scales and shifts, bit for bit."""
    from plnerf_amd import _lib as L_
    exe = c_hosts.build("c_abi_depth_step_gpu", tmp_path)
    R, Ns, Ni, steps = 256, 64, 32, 3
    run = c_hosts.run(exe, L_.PRECISION[precision], R, Ns, Ni, steps, L_.FWD_KERNEL, n_hyp,
                      c_hosts.write_tables(tmp_path / "tables.bin", Ns, Ni))
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    host_losses = c_hosts.parse_steps(run.stdout)
    host_sums, host_ss = c_hosts.parse_sums(run.stdout, "params"), c_hosts.parse_sums(run.stdout, "ss")
    assert len(host_losses) == steps

    one = _step(P, True, seed=11, load=False, precision=precision, N_samples=Ns, N_importance=Ni, **SS)
    for which, net in enumerate(one.nets):
        shapes = [(name, tuple(t.shape)) for name, t in net.state_dict().items()]
        assert len(shapes) == 24
        net.load_state_dict(c_hosts.hashed_state_dict(which, shapes))
    px, _hashed = V * H * W, c_hosts.hashed
    images = torch.from_numpy(_hashed(999, px * 3)).reshape(V, H, W, 3)
    hyp = torch.from_numpy(np.float32(2.0) + np.float32(4.0) * _hashed(998, px * n_hyp)).reshape(V, n_hyp, H, W)
    valid = torch.from_numpy(_hashed(997, px) > np.float32(0.3)).reshape(V, H, W)
    poses = torch.eye(4).repeat(V, 1, 1)
    intr = torch.zeros(V, 4)
    for v in range(V):
        poses[v, 0, 3], poses[v, 2, 3] = float(np.float32(0.1) * np.float32(v)), 4.0
        intr[v] = torch.tensor([40.0 + v, 42.0 - v, 16.0, 12.0])
    views = P.DepthViews(images.to(DEV), poses.to(DEV), intr.to(DEV), hyp.to(DEV), valid.to(DEV), 2.0, 6.0)
    ours = [one.step_view(views, k % V, R) for k in range(steps)]
    assert one.one_call_steps == steps and one._ss_steps == steps
    bits, checksum = c_hosts.bits, c_hosts.checksum
    for k, (step, (h_loss, h_carve)) in enumerate(zip(ours, host_losses)):
        assert torch.isfinite(step[0]) and (bits(step[0]), bits(step[2])) == (h_loss, h_carve), (k, float(step[0]), hex(h_loss))
    assert [checksum(torch.cat([p.detach().reshape(-1) for p in net.parameters()])) for net in one.nets] == host_sums
    assert [checksum(one.depth_scales), checksum(one.depth_shifts)] == host_ss
