"""The depth-supervised loop's data feed without a GPU: the C ABI of include/plnerf_hip_depthfeed.h (plain C99, linked
against the library, argument validation before any device work; the signatures themselves are compared in
tests/test_abi_headers.py), the learning-rate schedule and the scale / shift stepping rule of
run_nerf_sample_based_depth.py:1104-1161, and the depth checkpoint's wire format."""
import os
import re
import subprocess

import pytest
import torch

import abi_support as abi
from run_args import depth_args

HEADER = os.path.join(abi.INCLUDE, "plnerf_hip_depthfeed.h")


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_depthfeed_names_and_constants_match_the_header(L):
    """The header's entry points are this table's, and the workspace size the binding restates are the header's.
    (Argument by argument: tests/test_abi_headers.py.)"""
    assert set(abi.prototypes(HEADER)) == set(L.DEPTHFEED_SIGNATURES) == {"plnerf_select_depth_rays",
                                                                          "plnerf_depth_scale_shift_grad"}
    ws = int(re.search(r"#define\s+PLNERF_DEPTH_SS_WORKSPACE_BYTES\s+(\d+)", open(HEADER).read()).group(1))
    assert L.DEPTH_SS_WORKSPACE_BYTES == ws


_C = r"""
#include <stdio.h>
#include "plnerf_hip_depthfeed.h"

int main(void) {
    int (*sel)(int, int, int, int, int, const float*, const float*, const uint8_t*, const float*, int, const float*,
               const float*, const float*, float, float, uint64_t, uint32_t, int, int, float*, float*, float*, float*,
               float*, float*, float*, float*, float*, int*, plnerf_stream_t) = plnerf_select_depth_rays;
    int (*ssg)(const float*, const float*, const float*, const float*, int, int, int, int, int, const int*, float, float,
               int, int, float*, float*, void*, plnerf_stream_t) = plnerf_depth_scale_shift_grad;
    float d[64] = {0};
    double ws[8] = {0};
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION < 601) return 2;
    /* validation before any device work: these calls never touch the (absent) GPU */
#define SEL(nv, v, H, W, nh, img, rows, id0, R, o) \
    sel(nv, v, H, W, nh, img, d, NULL, d, rows, d, NULL, NULL, 2.f, 6.f, 0, 0, id0, R, o, o, NULL, o, o, o, o, o, NULL, NULL, NULL)
    if (SEL(0, 0, 4, 4, 1, d, 4, 0, 1, d) != PLNERF_EINVAL) return 3;          /* no views */
    if (SEL(2, 2, 4, 4, 1, d, 4, 0, 1, d) != PLNERF_EINVAL) return 4;          /* view outside [0, n_views) */
    if (SEL(2, -1, 4, 4, 1, d, 4, 0, 1, d) != PLNERF_EINVAL) return 5;
    if (SEL(2, 1, 4, 4, 1, d, 5, 0, 1, d) != PLNERF_EINVAL) return 6;          /* pose rows neither 3 nor 4 */
    if (SEL(2, 1, 4, 4, 0, d, 4, 0, 1, d) != PLNERF_EINVAL) return 7;          /* no hypotheses */
    if (SEL(2, 1, 4, 4, 1, NULL, 4, 0, 1, d) != PLNERF_EINVAL) return 8;       /* no images */
    if (SEL(2, 1, 37, 53, 1, d, 4, 1900, 62, d) != PLNERF_ERANGE) return 9;    /* ray ids [1900, 1962) past H*W = 1961 */
    if (SEL(2, 1, 32768, 32769, 1, d, 4, 0, 1, d) != PLNERF_ERANGE) return 10; /* H*W > 2^30 */
    if (SEL(2, 1, 37, 53, 1, d, 3, 1961, 0, NULL) != PLNERF_OK) return 11;     /* nothing to do */
    if (SEL(2, 1, 37, 53, 1, d, 3, 0, 4, NULL) != PLNERF_EINVAL) return 12;    /* rays without outputs */
    if (ssg(d, d, d, NULL, 0, 4, 1, 1, 0, NULL, 1.f, 0.f, 3, 1, d, d, ws, NULL) != PLNERF_EINVAL) return 13;   /* R = 0 */
    if (ssg(d, d, d, NULL, 8, 4, 1, 1, 0, NULL, 1.f, 0.f, 3, 3, d, d, ws, NULL) != PLNERF_EINVAL) return 14;   /* view */
    if (ssg(d, d, d, NULL, 8, 4, 1, 2, 0, NULL, 1.f, 0.f, 3, 1, d, d, ws, NULL) != PLNERF_EINVAL) return 15;   /* points */
    if (ssg(d, d, NULL, NULL, 8, 4, 1, 1, 0, NULL, 1.f, 0.f, 3, 1, d, d, ws, NULL) != PLNERF_EINVAL) return 16; /* raw */
    if (ssg(d, d, d, NULL, 8, 4, 1, 1, 0, NULL, 1.f, 0.f, 3, 1, d, d, NULL, NULL) != PLNERF_EINVAL) return 17; /* ws */
    if (ssg(d, d, d, NULL, 65536, 16385, 1, 1, 0, NULL, 1.f, 0.f, 3, 1, d, d, ws, NULL) != PLNERF_ERANGE) return 18;
    printf("depthfeed abi ok\n");
    return 0;
}
"""


def test_depthfeed_header_is_plain_c_and_links(L, tmp_path):
    out = subprocess.run([abi.compile_c(_C, tmp_path, "depthfeed_abi")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "depthfeed abi ok" in out.stdout


# ------------------------------------------------------------------------------------------------ host-side rules
def _reference_lr(optimizer_lr, i, lrate, start_decay_lrate, end_decay_lrate):
    """run_nerf_sample_based_depth.py:1104-1108 with update_learning_rate (train_utils/hyperparameter_update.py:3-5)."""
    if i > start_decay_lrate and i <= end_decay_lrate:
        portion = (i - start_decay_lrate) / (end_decay_lrate - start_decay_lrate)
        decay_rate = 0.1
        return lrate * (decay_rate ** portion)
    return optimizer_lr


def _depth_args(tmp, **over):
    at = dict(N_importance=64, N_samples=128, precision="fp32", ckpt_dir=str(tmp), expname="exp", ft_path=None, N_rand=64)
    return depth_args(**dict(at, **over))


@pytest.mark.parametrize("s,e", [(400000, 500000), (10, 30), (7, 8)])
def test_learning_rate_schedule_is_the_reference_expression(L, s, e):
    from plnerf_amd import depth
    lrate = 5e-4
    mid = (s + e) // 2
    for i in (s, s + 1, mid, e, e + 1, e + 1000, 1, 0):
        got = depth.learning_rate(i, lrate, s, e)
        want = _reference_lr(None, i, lrate, s, e)
        assert got == want, (i, got, want)        # the same Python float arithmetic: equal, not close
    assert depth.learning_rate(s, lrate, s, e) is None and depth.learning_rate(e + 1, lrate, s, e) is None
    assert depth.learning_rate(e, lrate, s, e) == lrate * 0.1 ** 1.0


@pytest.mark.parametrize("start", [0, 9, 19])
def test_step_learning_rate_counts_from_start(L, tmp_path, start):
    """DepthTrainStep.learning_rate() is the schedule at the reference's i = start + 1 (the next iteration), and the
    rate a loop that writes it every iteration holds is the reference's."""
    from plnerf_amd import depth
    args = _depth_args(tmp_path, start_decay_lrate=10, end_decay_lrate=30)
    kw, _, _, grad_vars, opt = depth.create_nerf(args, device=torch.device("cpu"))
    ts = depth.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, start=start)
    assert ts.global_step == start
    held = ref = args.lrate
    for i in range(start + 1, start + 40):
        assert ts.learning_rate() == depth.learning_rate(i, args.lrate, 10, 30)
        assert ts.learning_rate(i) == ts.learning_rate()
        lr = ts.learning_rate()
        held = held if lr is None else lr
        ref = _reference_lr(ref, i, args.lrate, 10, 30)
        assert held == ref, (i, held, ref)
        ts.global_step += 1
    assert held == args.lrate * 0.1 ** 1.0


def _reference_ss_steps(n_iters, warm_start_nerf, freeze_ss, space_carving_weight):
    """Which iterations move DEPTH_SCALES / DEPTH_SHIFTS in the reference loop (:1130-1161): their grads are None until
    the first iteration whose loss contains the space-carving term (zero_grad under torch 1.12 keeps a tensor a tensor),
    and torch.optim.Adam skips a parameter whose grad is None."""
    has_grad, out = False, []
    for i in range(1, n_iters + 1):
        if space_carving_weight > 0. and i > warm_start_nerf:
            has_grad = True
        out.append(i < freeze_ss and has_grad)
    return out


@pytest.mark.parametrize("warm,freeze,weight", [(0, 0, 0.007), (0, 5, 0.007), (3, 8, 0.007), (8, 3, 0.007), (0, 9, 0.0),
                                                (2, 100, 0.1), (5, 6, 1.0), (5, 5, 1.0)])
def test_scale_shift_stepping_rule(L, warm, freeze, weight):
    from plnerf_amd import depth
    got = [depth.scaleshift_steps(i, warm, freeze, weight) for i in range(1, 21)]
    assert got == _reference_ss_steps(20, warm, freeze, weight)


def test_depth_checkpoint_wire_format_and_reload(L, tmp_path):
    """depth.save_checkpoint writes the dict of run_nerf_sample_based_depth.py:1168-1183 (depth_scales / depth_shifts
    [V, 1] fp32); depth.create_nerf on it restores start, both networks and the optimizer state (not the scales)."""
    from plnerf_amd import depth
    (tmp_path / "exp").mkdir()
    args = _depth_args(tmp_path)
    cpu = torch.device("cpu")
    kw, _, start, grad_vars, opt = depth.create_nerf(args, device=cpu)
    assert start == 0
    # one optimizer step, so that the state dict holds moments and a step count
    for p in grad_vars:
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    V = 5
    scales = torch.linspace(0.9, 1.1, V).reshape(V, 1).requires_grad_(True)
    shifts = torch.linspace(-0.1, 0.1, V).reshape(V, 1).requires_grad_(True)
    path = os.path.join(str(tmp_path), "exp", "{:06d}.tar".format(77))
    depth.save_checkpoint(path, 77, kw["network_fn"], kw["network_fine"], opt, depth_scales=scales, depth_shifts=shifts)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"global_step", "network_fn_state_dict", "network_fine_state_dict", "optimizer_state_dict",
                       "depth_shifts", "depth_scales"}
    assert ck["global_step"] == 77
    for k, ref in (("depth_scales", scales), ("depth_shifts", shifts)):
        assert ck[k].shape == (V, 1) and ck[k].dtype == torch.float32 and torch.equal(ck[k], ref.detach())
    args2 = _depth_args(tmp_path, no_reload=False)
    kw2, _, start2, _, opt2 = depth.create_nerf(args2, device=cpu)
    assert start2 == 77
    for n in ("network_fn", "network_fine"):
        for a, b in zip(kw[n].parameters(), kw2[n].parameters()):
            assert torch.equal(a, b)
    s1, s2 = opt.state_dict(), opt2.state_dict()
    assert s1["param_groups"] == s2["param_groups"] and set(s1["state"]) == set(s2["state"])
    for k in s1["state"]:
        for name, v in s1["state"][k].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(s2["state"][k][name])), (k, name)
    # no fine network: the reference leaves the key out
    path2 = os.path.join(str(tmp_path), "coarse_only.tar")
    depth.save_checkpoint(path2, 3, kw["network_fn"], None, opt)
    assert set(torch.load(path2, map_location="cpu")) == {"global_step", "network_fn_state_dict", "optimizer_state_dict"}
