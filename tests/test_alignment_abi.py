"""The 16-byte alignment the headers demand of the float4 arrays -- raw, g_raw, raw_out [n,4] and feature_linear's weight
and bias -- is checked on the host before any launch: every entry that takes such a pointer answers PLNERF_EINVAL when it is
4 bytes off, on a machine without a device (where a launch would be PLNERF_ELAUNCH).  The one-call entries refuse a
misaligned feature_linear with their other argument checks, before the step's first launch.  tests/test_gpu_containment.py
repeats the kernel-level refusals on real buffers and shows that nothing was written."""
import ctypes

import pytest
import torch

import abi_support as abi
import containment as C

EINVAL = -1
# The aligned control of each refusal -- the same call with the pointer on a 16-byte boundary is NOT PLNERF_EINVAL -- is made
# only on a machine without a device, where a call that passes its checks fails at its first launch (PLNERF_ELAUNCH).  With a
# device it would launch on made-up addresses; there tests/test_gpu_containment.py makes the aligned calls on real memory.
NO_DEVICE = not torch.cuda.is_available()


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_every_float4_pointer_is_refused_when_misaligned(L):
    cases = C.misaligned_cases(L)
    entries = {call.entry for _, calls in cases for call in calls}
    assert entries == {"plnerf_quad_fwd", "plnerf_quad_bwd", "plnerf_quad_bwd_rays", "plnerf_coarse_epilogue", "plnerf_fine_epilogue",
                       "plnerf_coarse_epilogue_const", "plnerf_fine_epilogue_const", "plnerf_fine_epilogue_const_bwd",
                       "plnerf_mlp_pack_weights", "plnerf_mlp_fwd", "plnerf_mlp_bwd", "plnerf_mlp_bwd_multi"}
    for case_id, calls in cases:
        try:
            C.refused_on_fake_pointers(L, calls)
        except AssertionError as e:
            raise AssertionError(f"{case_id}: {e}") from None
    if NO_DEVICE:      # the control: aligned, the same calls pass every argument check
        for case_id, calls in C.misaligned_cases(L, shift=0):
            try:
                C.accepted_on_fake_pointers(L, calls)
            except AssertionError as e:
                raise AssertionError(f"{case_id} (aligned control): {e}") from None


def _flat_net(net, base, move):
    """A plnerf_step_net / plnerf_view_net whose 24 tensors lie in state_dict order from the made-up address `base`
    (16-byte aligned); tensor `move` starts 4 bytes late."""
    counts = [s[0] * (s[1] if len(s) == 2 else 1) for s in C.param_shapes(63, 27)]
    for k in range(24):
        net.params[k] = base + 4 * sum(counts[:k]) + (4 if k == move else 0)
    return sum(counts)


@pytest.mark.parametrize("move", [18, 19], ids=["feature_linear.weight", "feature_linear.bias"])
@pytest.mark.parametrize("entry", ["plnerf_train_step", "plnerf_train_step_const"])
def test_train_steps_refuse_a_misaligned_feature_linear(L, entry, move):
    cfg = C._step_config(L, C.MODE_LINEAR if entry == "plnerf_train_step" else C.MODE_CONSTANT, "f16x3")
    nbytes = getattr(L.lib(), entry + "_workspace_bytes")(ctypes.byref(cfg))
    assert nbytes > 0
    io, args = L.StepIo(), L.StepArgs()
    for k, (net, bad) in enumerate(((io.coarse, None), (io.fine, move))):
        base = (k + 1) << 28
        net.n_params = _flat_net(net, base, bad)
        net.param_flat, net.grad_flat, net.exp_avg, net.exp_avg_sq, net.packed = base, base + (1 << 24), base + (2 << 24), base + (3 << 24), base + (4 << 24)
    io.t_vals, io.u_vals, io.loss4 = 1 << 20, 2 << 20, 3 << 20
    args.rays, args.image, args.crop_rows, args.crop_cols = 8, 4 << 20, C.ONE_CALL_H, C.ONE_CALL_W
    args.adam_step_fine = args.adam_step_coarse = 1
    call = lambda: getattr(L.lib(), entry)(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(1 << 30), nbytes, None)
    assert call() == EINVAL
    if NO_DEVICE:
        _flat_net(io.fine, 2 << 28, None)
        assert call() not in (0, EINVAL)


@pytest.mark.parametrize("move", [18, 19], ids=["feature_linear.weight", "feature_linear.bias"])
def test_render_view_refuses_a_misaligned_feature_linear(L, move):
    cfg = C._step_config(L, C.MODE_LINEAR, "f16x3", max_rays=32, perturb=0, noise=0.0)
    nbytes = L.lib().plnerf_render_view_workspace_bytes(ctypes.byref(cfg))
    assert nbytes > 0
    io, args = L.ViewIo(), L.ViewArgs()
    for k, (net, bad) in enumerate(((io.coarse, move), (io.fine, None))):
        _flat_net(net, (k + 1) << 28, bad)
        net.packed = ((k + 1) << 28) + (4 << 24)
    io.t_vals, io.u_vals, io.rgb = 1 << 20, 2 << 20, 3 << 20
    args.n_pix, args.pack_weights = 8, 1
    call = lambda: L.lib().plnerf_render_view(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(1 << 30), nbytes, None)
    assert call() == EINVAL
    if NO_DEVICE:
        _flat_net(io.coarse, 1 << 28, None)
        assert call() not in (0, EINVAL)


@pytest.mark.parametrize("move", [18, 19], ids=["feature_linear.weight", "feature_linear.bias"])
@pytest.mark.parametrize("entry", ["plnerf_depth_train_step", "plnerf_depth_train_step_const"])
def test_depth_steps_refuse_a_misaligned_feature_linear(L, entry, move):
    cfg = C.depth_step_config(L, "f16x3")
    nbytes = getattr(L.lib(), entry + "_workspace_bytes")(ctypes.byref(cfg))
    assert nbytes > 0
    io, args = L.DepthStepIo(), L.DepthStepArgs()
    for k, (net, bad) in enumerate(((io.coarse, move), (io.fine, None))):
        base = (k + 1) << 28
        net.n_params = _flat_net(net, base, bad)
        net.param_flat, net.grad_flat, net.exp_avg, net.exp_avg_sq, net.packed = base, base + (1 << 24), base + (2 << 24), base + (3 << 24), base + (4 << 24)
    io.t_vals, io.u_vals, io.loss5 = 1 << 20, 2 << 20, 3 << 20
    io.images, io.hyp, io.poses, io.intrinsics = 4 << 20, 5 << 20, 6 << 20, 7 << 20
    args.view, args.rays, args.adam_step = 0, 8, 1
    call = lambda: getattr(L.lib(), entry)(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(1 << 30), nbytes, None)
    assert call() == EINVAL
    if NO_DEVICE:
        _flat_net(io.coarse, 1 << 28, None)
        assert call() not in (0, EINVAL)
