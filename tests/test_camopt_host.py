"""The camera-code optimisation without a GPU: fixture g10_camera_code_opt.npz (the reference's own optimize_camera_embedding,
recorded iteration by iteration by tests/golden/make_golden_camopt.py) against the fp64 restatement of tests/camopt_fp64.py --
the objective and its gradient at every recorded code, the update rule fed the recorded gradients and losses -- and the two
host-side pieces of plnerf_amd.camcode: coef from weights, and the batch sizes."""
import numpy as np
import pytest
import torch

import camopt_fp64 as R

from camopt_fp64 import CODE_TOL, GRAD_BOUND, GRAD_FP32_VS_FP64, LOSS_BOUND, LOSS_FP32_VS_FP64


@pytest.fixture(scope="module")
def g():
    return R.fixture()


@pytest.fixture(scope="module")
def cache64(g):
    return R.cache(g, torch.float64)


def scales(g):
    return float(g["loss_sum"].max()), float(np.abs(g["grad"]).max())


def test_fixture_is_the_scene_the_issue_names(g):
    assert (int(g["H"]), int(g["W"]), int(g["N_samples"]), int(g["N_importance"]), int(g["N_rand"]), int(g["n_cam"])) == \
        (4, 6, 8, 8, 6, 4)
    assert int(g["n_batches"]) == 2 and g["cam"].shape == (100, 4) and g["grad"].shape == (100, 4)
    assert g["loss_sum"].shape == (100,) and g["lr"].shape == (100,) and not g["cam"][0].any()
    assert np.abs(g["cam_target"]).min() > 0      # the target is the scene at a non-zero code
    assert float(g["lr"][0]) == 0.5 and float(g["lr"][-1]) < 0.5 / 4      # the scheduler halves at least twice


def test_restatement_matches_the_reference_at_every_recorded_code(g, cache64):
    l_scale, g_scale = scales(g)
    worst_l = worst_g = 0.0
    for i in range(g["cam"].shape[0]):
        loss, grad = R.loss_and_grad(cache64, g["cam"][i])
        worst_l = max(worst_l, abs(float(loss) - float(g["loss_sum"][i])) / l_scale)
        worst_g = max(worst_g, float((grad - torch.from_numpy(g["grad"][i]).double()).abs().max()) / g_scale)
    print(f"fp64 restatement against the fixture: loss {worst_l:.3e} (bound {LOSS_BOUND:.3e}), gradient {worst_g:.3e} "
          f"(bound {GRAD_BOUND:.3e})")
    assert worst_l <= LOSS_BOUND and worst_g <= GRAD_BOUND


def test_measured_fp32_distance_is_what_the_bounds_were_fixed_from(g, cache64):
    """The constants above, re-measured (first 10 and last 10 codes: the whole sweep is the test above's cost again)."""
    cache32 = R.cache(g, torch.float32)
    l_scale, g_scale = scales(g)
    worst_l = worst_g = 0.0
    for i in list(range(10)) + list(range(90, 100)):
        l64, g64 = R.loss_and_grad(cache64, g["cam"][i])
        l32, g32 = R.loss_and_grad(cache32, g["cam"][i])
        worst_l = max(worst_l, abs(float(l32) - float(l64)) / l_scale)
        worst_g = max(worst_g, float((g32.double() - g64).abs().max()) / g_scale)
    print(f"fp32 against fp64 restatement: loss {worst_l:.3e}, gradient {worst_g:.3e}")
    assert worst_l <= LOSS_FP32_VS_FP64 * 1.05 and worst_g <= GRAD_FP32_VS_FP64 * 1.05


def test_restated_update_reproduces_the_recorded_run(g):
    u = R.Update(int(g["n_cam"]), int(g["n_batches"]))
    worst = 0.0
    for i in range(g["cam"].shape[0]):
        worst = max(worst, float((u.cam - torch.from_numpy(g["cam"][i])).abs().max()))
        assert u.lr == float(g["lr"][i]), (i, u.lr, float(g["lr"][i]))      # exactly
        psnr = u.step(g["grad"][i], g["loss_sum"][i])
        assert psnr == float(g["psnr"][i]), (i, psnr)
    print(f"restated Adam against the recorded codes: {worst:.2e}")
    assert worst <= CODE_TOL
    assert u.best_iter == int(g["best_iter"])      # exactly
    assert float((u.best_cam - torch.from_numpy(g["best_cam"])).abs().max()) <= CODE_TOL
    assert u.max_psnr == float(g["best_psnr"])
    # the reference's quirk: the stored code is the one AFTER the best iteration's step, i.e. the next recorded code
    assert np.array_equal(g["best_cam"], g["cam"][int(g["best_iter"]) + 1])


@pytest.mark.parametrize("mode,color_mode", [("linear", "midpoint"), ("linear", "left"), ("constant", "midpoint")])
def test_coef_from_weights_is_raw2outputs_colour_rule(mode, color_mode):
    from plnerf_amd import camcode
    gen = torch.Generator().manual_seed(5)
    for S in (1, 2, 7, 16):
        w = torch.rand(9, S + 1 if mode == "linear" else S, generator=gen, dtype=torch.float64)
        w[3] = 0.0
        got = camcode.coef_from_weights(w.clone(), mode, color_mode)
        want = R.coef_reference(w, mode, color_mode)
        assert got.shape == want.shape == (9, S)
        assert float((got - want).abs().max()) <= 1e-15
        # ... and on colours: sum_s c_s rgb_s is the reference's rgb_map
        rgb = torch.rand(9, S, 3, generator=gen, dtype=torch.float64)
        if mode == "constant":
            ref = torch.sum(w[..., None] * rgb, -2)
        elif color_mode == "midpoint":
            cc = torch.cat([rgb[:, :1], rgb, rgb[:, -1:]], 1)
            ref = torch.sum(w[..., None] * (.5 * (cc[:, 1:] + cc[:, :-1])), -2)
        else:
            ref = torch.sum(w[..., None] * torch.cat([rgb[:, :1], rgb], 1), -2)
        assert float((torch.sum(got[..., None] * rgb, -2) - ref).abs().max()) <= 1e-14


def test_batch_sizes_are_compute_samples_per_subset(g):
    from plnerf_amd import camcode
    cases = g["subset_cases"]
    assert len(cases) >= 12
    unequal = 0
    for n_pix, n_rand, per, normal, extra in cases.tolist():
        assert camcode.compute_samples_per_subset(n_pix, 2 * n_rand) == (per, normal, extra)
        sizes = camcode.batch_sizes(n_pix, n_rand)
        assert sizes == [per] * normal + [per + 1] * extra and sum(sizes) == n_pix
        unequal += extra > 0 and normal > 0
        lam = camcode.ray_weights(sizes)
        assert lam.shape == (n_pix,) and abs(float(lam.double().sum()) - len(sizes) / 3.0) < 1e-4
    assert unequal >= 3
    with pytest.raises(NotImplementedError, match="no code to optimise"):
        from argparse import Namespace
        camcode.optimize_camera_embedding(None, None, 4, 6, None, Namespace(input_ch_cam=0, N_rand=6), {})
