"""End-to-end parity of the BENCHMARKED arithmetic (precision="f16x3", and its sibling "bf16x3") on a real MI355X.

bench.py times the training step with the 3-term split forward and the half-plane backward; test_gpu_parity.py pins
every stage in fp32 and the MLP stage in all modes.  These tests pin what the benchmark actually runs, end to end,
against the reference-generated fixtures (G5 render_rays, G6 training step) and against the fp32 CPU oracle over a
100-step optimisation (the "PSNR vs ref" proxy of BASELINE.json's metric).

Stated tolerances (each asserted below):
  * G5, coarse pass (continuous in the network output):      1e-5 abs+rel, the contract
  * G5, final maps (pass through the discontinuous sampler):  1e-5 on rgb / acc / depth in f16x3; bf16x3 2e-5;
    z_std 2e-5 (measured values are printed)
  * G6 loss:                                                  1e-5
  * G6 gradients, per tensor, f16x3 / bf16x3:                 max error over the fixture's sampled entries <= 6e-3
    (coarse net) / 3e-3 (fine net) of the largest sampled |g| of that tensor, and the tensor's gradient norm within
    2e-3 (measured: 3.6e-3 / 1.4e-3.  The backward of the 16-bit modes runs on IEEE-half planes -- 11-bit operands,
    DESIGN.md section 3 -- so an entry carries a few 2^-12 of its random-walk scale; fp32 mode is asserted at
    2e-4 / 2e-3 by test_gpu_parity.py::test_train_step_golden_and_oracle and measures 1.5e-4 of |g|)
  * 100 steps, f16x3 vs the fp32 oracle on identical draws:   see test_hundred_steps_track_fp32_oracle
"""
import os
import tempfile

import numpy as np
import pytest
import torch

from abi_support import ROOT
from gpu_support import P, T, assert_close, depth_setup, dev, g, g5_batch, make_net, maxdiff
from oracle import plnerf_oracle as orc
from run_args import depth_args_of, nvs_args

pytestmark = pytest.mark.gpu
SPLIT_MODES = ["f16x3", "bf16x3"]


def _ckdir():
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "exp"))
    return d


# final-map bounds per mode: (rgb/acc/depth/disp, z_std)
G5_FINAL_TOL = {"f16x3": (1e-5, 2e-5), "bf16x3": (2e-5, 2e-5)}


@pytest.mark.parametrize("precision", SPLIT_MODES)
def test_g5_render_rays_all_cases_in_split_modes(P, golden, precision):
    """All four reference-generated render_rays cases (64+128, 128+64, NDC, noise) through render() in the mode
    bench.py times."""
    gd = golden("g5_render_rays")
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    tol, tol_std = G5_FINAL_TOL[precision]
    for c in range(int(gd["n_cases"])):
        p = f"c{c}_"
        o, d, near, far = g5_batch(gd, p)
        net_c = make_net(P, orc.closed_form_state_dict(0, True), precision)
        net_f = make_net(P, orc.closed_form_state_dict(1, True), precision)
        qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
        kw = dict(network_query_fn=qfn, perturb=1.0, N_importance=int(gd[p + "N_importance"]), network_fine=net_f,
                  N_samples=int(gd[p + "N_samples"]), network_fn=net_c, white_bkgd=bool(gd[p + "white_bkgd"]),
                  raw_noise_std=float(gd[p + "raw_noise_std"]), mode=str(gd[p + "mode"]), color_mode="midpoint")
        f = float(gd[p + "focal"])
        H, W = int(gd[p + "H"]), int(gd[p + "W"])
        K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
        with torch.no_grad():
            rgb, disp, acc, extras = P.render(H, W, K, chunk=32768, rays=(g(o), g(d)), ndc=bool(gd[p + "ndc"]),
                                              near=near, far=far, use_viewdirs=True, retraw=True, pytest=True, **kw)
        got = dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc)
        for k in ("rgb0", "acc0", "depth0", "disp0"):
            assert_close(got[k], gd[p + k], what=f"{precision} g5 case {c} {k}")
        errs = {k: maxdiff(got[k], T(gd[p + k])) for k in ("rgb_map", "acc_map", "depth_map", "z_std", "raw")}
        print(f"{precision} g5 case {c}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k in ("rgb_map", "acc_map", "depth_map"):
            assert_close(got[k], gd[p + k], atol=tol, rtol=tol, what=f"{precision} g5 case {c} {k}")
        assert_close(got["z_std"], gd[p + "z_std"], atol=tol_std, rtol=tol_std, what=f"{precision} g5 case {c} z_std")


G6_GRAD_TOL = {"coarse": 6e-3, "fine": 3e-3}


@pytest.mark.parametrize("precision", SPLIT_MODES)
def test_g6_train_step_in_split_modes(P, golden, precision):
    """One optimisation step of the reference (G6: loss, sampled gradients, parameters after Adam) in the benchmarked
    arithmetic."""
    gd = golden("g6_train_step")
    stride = int(gd["sample_stride"])
    for c in range(int(gd["n_cases"])):
        p = f"c{c}_"
        args = nvs_args(_ckdir(), precision, N_samples=int(gd[p + "N_samples"]), N_importance=int(gd[p + "N_importance"]))
        kw, _, _, _, opt, opt_c = P.create_nerf(args, device=dev())
        kw["network_fn"].load_state_dict(orc.closed_form_state_dict(0, False))
        kw["network_fine"].load_state_dict(orc.closed_form_state_dict(1, False))
        batch, target = T(gd[p + "ray_batch"]), T(gd[p + "target"])
        rays = (g(batch[:, 0:3]), g(batch[:, 3:6]))
        K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
        rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=rays, near=2.0, far=6.0, retraw=True,
                                          pytest=True, **kw)
        opt.zero_grad()
        opt_c.zero_grad()
        loss = P.img2mse(rgb, g(target)) + P.img2mse(extras["rgb0"], g(target))
        loss.backward()
        assert abs(float(loss.detach()) - float(gd[p + "loss"])) <= 1e-5, (float(loss.detach()), float(gd[p + "loss"]))
        worst = {"coarse": 0.0, "fine": 0.0}
        for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
            for name, prm in net.named_parameters():
                ref = T(gd[p + f"grad_{tag}_{name}_sample"])
                got = prm.grad.reshape(-1)[::stride].cpu()
                ref_norm = float(gd[p + f"grad_{tag}_{name}_norm"])
                err = float((got - ref).abs().max())
                scale = max(float(ref.abs().max()), 1e-6)
                worst[tag] = max(worst[tag], err / scale)
                assert err <= G6_GRAD_TOL[tag] * scale + 1e-8, f"{precision} {tag} {name}: grad err {err:.3e} of {scale:.3e}"
                assert abs(float(prm.grad.norm()) - ref_norm) <= 2e-3 * ref_norm + 1e-9, f"{precision} {tag} {name}: norm"
        print(f"{precision} g6 case {c}: loss {float(loss.detach()):.7f} (ref {float(gd[p + 'loss']):.7f}), worst grad err / "
              f"max|g|: coarse {worst['coarse']:.2e}, fine {worst['fine']:.2e}")
        opt.step()
        opt_c.step()
        for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
            for name, prm in net.named_parameters():
                ref = T(gd[p + f"param_{tag}_{name}_sample"])
                assert float((prm.detach().reshape(-1)[::stride].cpu() - ref).abs().max()) <= 1.25e-3


def test_hundred_steps_track_fp32_oracle(P):
    """The "PSNR vs ref" proxy: 100 optimisation steps of TrainStep in f16x3 against the fp32 CPU oracle's loop
    (orc.train_step) from identical weights, on identical rays, targets and draws (pytest=True).  The loop is
    chaotic in the long run (a ReLU or sampler-bin flip anywhere decorrelates the trajectories), so the statement is
    made where it is meaningful: step-wise agreement early, PSNR agreement late.

      * steps 0..19:   |loss - oracle loss| <= 2e-4 * oracle loss at every step
      * steps 80..99:  mean PSNR within 0.1 dB of the oracle's mean PSNR (the fine-image PSNR the reference prints)
      * the loss falls by more than a factor 2 on both sides (the run does optimise something)
    """
    n_steps, R = 100, 64
    args = nvs_args(_ckdir(), "f16x3")
    kw, _, start, _, opt, opt_c = P.create_nerf(args, device=dev())
    sd_c, sd_f = orc.closed_form_state_dict(0, False), orc.closed_form_state_dict(1, False)
    kw["network_fn"].load_state_dict(sd_c)
    kw["network_fine"].load_state_dict(sd_f)
    batch, _ = orc.synthetic_blender_rays(R, seed=11)
    # a learnable target: a smooth function of the ray direction (random targets have no signal to fit)
    dirs = torch.nn.functional.normalize(batch[:, 3:6], dim=-1)
    target = (0.5 + 0.5 * torch.sin(3.0 * dirs + torch.tensor([0.0, 1.0, 2.0]))).float()
    rays = (g(batch[:, 0:3]), g(batch[:, 3:6]))
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    ts = P.TrainStep(args, dict(kw, pytest=True), opt, opt_c, start=start, distributed=False)
    okw = dict(N_samples=64, N_importance=128, mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True,
               raw_noise_std=0.0, pytest=True)
    state, lr = {}, 5e-4
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref_losses, got_losses, ref_psnr, got_psnr = [], [], [], []
    for step in range(n_steps):
        out = orc.train_step(sd_c, sd_f, batch, target, okw, lr=lr, adam_state=state, return_psnr=True)
        ref_losses.append(float(out[0]))
        ref_psnr.append(float(out[3]))
        loss, psnr = ts(800, 800, K, rays, g(target), near=2.0, far=6.0)
        got_losses.append(float(loss))
        got_psnr.append(float(psnr))
        lr = 5e-4 * 0.1 ** (step / 250000.0)      # the rate TrainStep installs after this step (lrate_decay = 250)
    rl, gl = np.array(ref_losses), np.array(got_losses)
    rel = np.abs(gl - rl) / rl
    dpsnr = abs(np.mean(got_psnr[80:]) - np.mean(ref_psnr[80:]))
    print(f"100 steps f16x3 vs fp32 oracle: loss {rl[0]:.5f} -> {rl[-1]:.5f} (oracle), {gl[0]:.5f} -> {gl[-1]:.5f} (HIP); "
          f"max rel gap steps 0-19 {rel[:20].max():.2e}, 20-49 {rel[20:50].max():.2e}, 50-99 {rel[50:].max():.2e}; "
          f"mean PSNR last 20: oracle {np.mean(ref_psnr[80:]):.3f} dB, HIP {np.mean(got_psnr[80:]):.3f} dB")
    assert rel[:20].max() <= 2e-4, rel[:20].max()
    assert dpsnr <= 0.1, dpsnr
    assert rl[-1] < 0.5 * rl[0] and gl[-1] < 0.5 * gl[0]


def test_two_hundred_steps_psnr_vs_exact_fp32_on_the_analytic_scene(P):
    """BASELINE.json's metric is "training rays/sec ...; PSNR vs ref": the bench line's `psnr_vs_ref` leg -- 200 steps at
    4096 rays on the analytic scene (tools/scene.py) in the benchmarked arithmetic and in the exact-fp32 kernels (whose
    gradients are reference-equal to 1e-5, test_gpu_fullsize.py), from identical weights, pixels and draws.  At 200
    steps the two trajectories have not decorrelated yet, so the gap measures the arithmetic: asserted at 0.1 dB on the
    training PSNR (measured -0.013) and on a loss that has fallen by 5x.  (2000 steps, three seeds and the fp32-vs-fp32
    noise floor: profiles/r04_psnr_summary.txt.)"""
    from tools.scene import psnr_vs_ref
    out = psnr_vs_ref(P, dev(), 200, rays=4096, precision="f16x3", views=8)
    run, ref = out["run"], out["ref"]
    print(f"200 steps x 4096 rays: train PSNR (last 20) f16x3 {run['psnr_train_tail_mean']:.3f} dB, fp32 "
          f"{ref['psnr_train_tail_mean']:.3f} dB (gap {out['gap_db_train']:+.3f}); held-out view {run['psnr_heldout_view']:.3f} / "
          f"{ref['psnr_heldout_view']:.3f} dB; {run['ms_per_step']:.2f} / {ref['ms_per_step']:.2f} ms per step")
    assert abs(out["gap_db_train"]) <= 0.1, out["gap_db_train"]
    assert abs(out["gap_db_heldout"]) <= 0.5, out["gap_db_heldout"]
    assert run["loss_at"]["200"] < 0.2 * run["loss_at"]["1"] and ref["loss_at"]["200"] < 0.2 * ref["loss_at"]["1"]
    assert abs(run["loss_at"]["10"] - ref["loss_at"]["10"]) <= 1e-4 * ref["loss_at"]["10"]      # early steps: same trajectory


# ----------------------------------------------------------------------------- BASELINE configs[4]: depth variant, 128+64
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_depth_variant_config5_sampling_golden(P, golden, precision):
    """The depth-supervised step (run_nerf_sample_based_depth.py:792-958, 1126-1157) at configs[4]'s sampling,
    N_samples = 128 / N_importance = 64, against the reference's own outputs (G8b): the render dict and one clipped
    training step.  pred_hyp and the fine maps pass through the sampler's ill-conditioned closed form (DESIGN.md
    section 6): asserted at 2e-4; everything upstream of it at 1e-5."""
    gd = golden("g8b_depth_variant_128_64")
    stride = int(gd["sample_stride"])
    Dp, kw, grad_vars, opt = depth_setup(gd, precision)
    batch, target, target_h = g(T(gd["ray_batch"])), g(T(gd["target"])), g(T(gd["target_h"]))
    with torch.no_grad():
        ret = Dp.render_rays(batch, retraw=True, pytest=True, **kw)
    assert torch.equal(ret["u"].cpu(), T(gd["render_u"]))
    for k in ("rgb0", "acc0", "depth0", "disp0", "z_vals0", "weights0"):
        assert_close(ret[k], gd["render_" + k], what=f"{precision} g8b {k}")
    errs = {}
    for k in ("rgb_map", "acc_map", "depth_map", "z_vals", "pred_hyp", "z_std"):
        errs[k] = maxdiff(ret[k], T(gd["render_" + k]))
        assert_close(ret[k], gd["render_" + k], atol=2e-4, rtol=2e-4, what=f"{precision} g8b {k}")
    print(f"{precision} g8b: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    step = Dp.DepthTrainStep(depth_args_of(gd, precision), kw, opt, grad_vars, distributed=False)
    loss, img_loss, sc, _ = step(batch, target, target_h, pytest=True)
    assert abs(float(loss) - float(gd["loss"])) <= 1e-5, (float(loss), float(gd["loss"]))
    assert abs(float(sc) - float(gd["space_carving_loss"])) <= 2e-4, (float(sc), float(gd["space_carving_loss"]))
    for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
        for name, prm in net.named_parameters():
            ref = T(gd[f"param_{tag}_{name}_sample"])
            assert float((prm.detach().reshape(-1)[::stride].cpu() - ref).abs().max()) <= 1.25e-3, (tag, name)


def test_depth_variant_full_size_properties(P, golden):
    """configs[4]'s per-GPU workload (4096 rays x (128 + 64) samples, space-carving loss through pred_hyp) in the
    benchmarked arithmetic: size-independent invariants of one full training step."""
    gd = golden("g8b_depth_variant_128_64")
    Dp, kw, grad_vars, opt = depth_setup(gd, "f16x3")
    R = 4096
    batch, target = orc.synthetic_blender_rays(R, seed=5)
    rng = np.random.default_rng(5)
    target_h = torch.from_numpy(rng.uniform(2.0, 6.0, size=(3, R, 1)).astype(np.float32))
    batch, target, target_h = g(batch), g(target), g(target_h)
    with torch.no_grad():
        ret = Dp.render_rays(batch, retraw=True, **kw)
        first = Dp.render_rays(batch[:1000], retraw=True, cached_u=ret["u"][:1000], **dict(kw, perturb=0.0))
        again = Dp.render_rays(batch[:1000], retraw=True, cached_u=ret["u"][:1000], **dict(kw, perturb=0.0))
    z, w, hyp = ret["z_vals"], ret["weights"], ret["pred_hyp"]
    assert z.shape == (R, 192) and w.shape == (R, 192) and hyp.shape == (R, 64)   # weights[..., 1:], as the reference returns
    assert (z[:, 1:] >= z[:, :-1]).all() and (z >= 2.0).all() and (z <= 6.0).all()          # merged samples sorted, in range
    assert (hyp >= 2.0).all() and (hyp <= 6.0).all() and torch.isfinite(hyp).all()
    assert (w >= 0).all() and (w.sum(-1) <= ret["acc_map"] + 1e-5).all() and (ret["acc_map"] <= 1.0 + 1e-5).all()
    assert ((ret["rgb_map"] >= -1e-6) & (ret["rgb_map"] <= 1.0 + 1e-5)).all()
    for k in ("rgb_map", "depth_map", "pred_hyp", "z_vals"):                                   # deterministic given u
        assert torch.equal(first[k], again[k]), k
    step = Dp.DepthTrainStep(depth_args_of(gd, "f16x3"), kw, opt, grad_vars, distributed=False)
    before = [p.detach().clone() for p in grad_vars]
    loss, img_loss, sc, _ = step(batch, target, target_h)
    assert torch.isfinite(loss) and float(sc) >= 0.0
    moved = max(float((a - b.detach()).abs().max()) for a, b in zip(before, grad_vars))
    assert all(torch.isfinite(p).all() for p in grad_vars) and 0.0 < moved <= 5.5e-4            # Adam's first step: <= lr (+ rounding)


# ----------------------------------------------------------------------------- checkpoint wire format (section 8f-3)
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_reference_written_checkpoint_loads_and_continues(P, golden, precision, tmp_path):
    """tests/golden/g9_reference_checkpoint.tar was written by the reference (run_plnerf.py:1324-1332) after G6's
    step.  create_nerf(no_reload=False) picks it up (run_plnerf.py:454-471); the render on fresh rays equals the
    reference's render after ITS reload, and one more optimisation step -- fine Adam resuming from the file's
    moments, coarse Adam restarting, as in the reference -- lands on the reference's loss, gradients and weights."""
    import shutil
    gd = golden("g9_checkpoint")
    (tmp_path / "exp").mkdir()
    shutil.copyfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_reference_checkpoint.tar"),
                    str(tmp_path / "exp" / "000001.tar"))
    args = nvs_args(str(tmp_path), precision, no_reload=False)
    kw, _, start, grad_vars, opt, opt_c = P.create_nerf(args, device=dev())
    assert start == int(gd["global_step"]) == 1
    assert all(float(opt.state[p]["step"]) == 1.0 for p in grad_vars)
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    rb = T(gd["render_batch"])
    with torch.no_grad():
        rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=(g(rb[:, 0:3]), g(rb[:, 3:6])), near=2.0,
                                          far=6.0, retraw=True, pytest=True, **kw)
    got = dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc)
    for k in ("rgb0", "acc0", "depth0", "rgb_map", "acc_map", "depth_map"):
        assert_close(got[k], gd["render_" + k], what=f"{precision} g9 render {k}")
    assert_close(got["z_std"], gd["render_z_std"], atol=2e-5, rtol=2e-5, what=f"{precision} g9 render z_std")
    batch, target = T(gd["ray_batch"]), g(T(gd["target"]))
    rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=(g(batch[:, 0:3]), g(batch[:, 3:6])), near=2.0,
                                      far=6.0, retraw=True, pytest=True, **kw)
    opt.zero_grad()
    opt_c.zero_grad()
    loss = P.img2mse(rgb, target) + P.img2mse(extras["rgb0"], target)
    loss.backward()
    assert abs(float(loss.detach()) - float(gd["loss"])) <= 1e-5, (float(loss.detach()), float(gd["loss"]))
    stride = int(gd["sample_stride"])
    gtol = {"fp32": {"coarse": 2e-4, "fine": 2e-3}, "f16x3": G6_GRAD_TOL}[precision]
    for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
        for name, prm in net.named_parameters():
            ref = T(gd[f"grad_{tag}_{name}_sample"])
            err = float((prm.grad.reshape(-1)[::stride].cpu() - ref).abs().max())
            assert err <= gtol[tag] * max(float(ref.abs().max()), 1e-6) + 1e-8, (precision, tag, name, err)
    opt.step()
    opt_c.step()
    assert all(float(opt.state[p]["step"]) == 2.0 for p in grad_vars)
    worst = {"coarse": 0.0, "fine": 0.0}
    for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
        for name, prm in net.named_parameters():
            ref = T(gd[f"param_{tag}_{name}_sample"])
            worst[tag] = max(worst[tag], float((prm.detach().reshape(-1)[::stride].cpu() - ref).abs().max()))
    print(f"{precision} g9: loss {float(loss.detach()):.7f}; max |param - reference| after the resumed step: coarse "
          f"{worst['coarse']:.2e} (restarted Adam), fine {worst['fine']:.2e} (resumed Adam)")
    # coarse Adam restarts: a first step (every weight moves ~lr, sign flips cost 2 lr).  The fine Adam's second step
    # divides by sqrt(v) built from two gradients: same bound.
    assert worst["coarse"] <= 1.25e-3 and worst["fine"] <= 1.25e-3


# ----------------------------------------------------------------------------- the two forward kernels of the half modes
_KERNEL_PROBE = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
import plnerf_amd as P
from oracle import plnerf_oracle as orc
dev = torch.device("cuda:0")
out = {}
for prec in ("f16x3", "f16", "bf16x3", "bf16"):
    net = P.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True, precision=prec)
    net.load_state_dict(orc.closed_form_state_dict(3, True))
    net = net.to(dev)
    gen = torch.Generator().manual_seed(5)
    pts = ((torch.rand(37, 101, 3, generator=gen) * 2 - 1) * 2.5).to(dev)          # 3737 rows: ragged last tile
    vd = torch.nn.functional.normalize(torch.randn(37, 3, generator=gen), dim=-1).to(dev)
    cot = torch.randn(37, 101, 4, generator=gen).to(dev)
    with torch.no_grad():
        out[prec + "_infer"] = net.query(pts, vd).cpu()
    raw = net.query(pts, vd)
    (raw * cot).sum().backward()
    out[prec + "_train"] = raw.detach().cpu()
    out[prec + "_grads"] = torch.cat([p.grad.reshape(-1) for p in net.parameters()]).cpu()
torch.save(out, sys.argv[2])
'''


def test_register_resident_and_ping_pong_forward_kernels_agree(P, tmp_path):
    """The 16-bit modes have two forward kernels (mlp_rr.hip; mlp_h16_fwd_pp.inc: which one serves what is the
    dispatch of mlp_api.hip -- the bf16-element modes use the register-resident one for inference only).  Forced to one or the other for BOTH roles (PLNERF_FWD_KERNEL, read once per process), they must
    produce the same outputs to rounding (they sum in different orders) and -- through the saved half planes and relu
    bits each writes -- the same parameter gradients; both against the fp32 oracle within the modes' bounds."""
    import subprocess
    import sys
    script = tmp_path / "probe.py"
    script.write_text(_KERNEL_PROBE)
    res = {}
    for k in ("rr", "pp"):
        path = str(tmp_path / f"{k}.pt")
        env = dict(os.environ, PLNERF_FWD_KERNEL=k)
        r = subprocess.run([sys.executable, str(script), ROOT, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        res[k] = torch.load(path)
    sd = orc.closed_form_state_dict(3, True)
    gen = torch.Generator().manual_seed(5)
    pts = (torch.rand(37, 101, 3, generator=gen) * 2 - 1) * 2.5
    vd = torch.nn.functional.normalize(torch.randn(37, 3, generator=gen), dim=-1)
    ref = orc.query_network(sd, pts, vd)
    # (bf16x3 carries 16 mantissa bits per operand: on this network -- sharpened weights, |x| up to 2.5 -- it measures
    #  1.2e-5 on the ping-pong kernel and 1.4e-5 on the register-resident one; its 1e-5 statement is G1 / G5's)
    for prec, tol in (("f16x3", 1e-5), ("f16", 2e-3), ("bf16x3", 3e-5), ("bf16", 1e-2)):
        for role in ("infer", "train"):
            a, b = res["rr"][f"{prec}_{role}"], res["pp"][f"{prec}_{role}"]
            print(f"{prec} {role}: rr vs pp {maxdiff(a, b):.2e}; rr vs oracle {maxdiff(a, ref):.2e}; pp vs oracle {maxdiff(b, ref):.2e}")
            assert maxdiff(a, ref) <= tol and maxdiff(b, ref) <= tol
        ga, gb = res["rr"][f"{prec}_grads"], res["pp"][f"{prec}_grads"]
        cos = float(torch.nn.functional.cosine_similarity(ga.double().reshape(1, -1), gb.double().reshape(1, -1)))
        rel = float((ga - gb).abs().max() / gb.abs().max())
        print(f"{prec} gradients: rr vs pp max diff / max|g| {rel:.2e}, cosine {cos:.8f}")
        if prec in ("f16x3", "bf16x3"):       # same relu branches on both sides (the forward errors are ~1e-6): sharp agreement
            assert rel <= 2e-3 and cos >= 0.999999
        else:
            assert cos >= 0.99


# ----------------------------------------------------------------------------- caller-embedded inputs, split kernel
@pytest.mark.parametrize("precision", SPLIT_MODES)
@pytest.mark.parametrize("widths", [(63, 27), (57, 3), (64, 32), (5, 1)])
def test_embedded_inputs_on_the_split_kernel(P, widths, precision):
    """NeRF.forward's own signature -- a caller-supplied encoding [N, input_ch + input_ch_views] -- in the split modes:
    served by the register-resident kernel (slot values loaded per tile, mlp_rr.hip) for every width the C ABI admits, the
    depth-supervised variant's 57 | 3 among them.  A ragged row count (three 128-row tiles, the last one cut inside a
    wave), forward against the fp32 oracle at the 1e-5 contract, all 24 gradient tensors at the split modes' bound."""
    in_ch, view_ch = widths
    torch.manual_seed(23)
    ref_net = P.NeRF(D=8, W=256, input_ch=in_ch, input_ch_views=view_ch, output_ch=5, skips=[4], use_viewdirs=True)
    sd = {k: v.detach().clone() for k, v in ref_net.state_dict().items()}
    gen = torch.Generator().manual_seed(29)
    N = 300
    emb = torch.randn(N, in_ch + view_ch, generator=gen)
    cot = torch.randn(N, 4, generator=gen)

    def oracle(sd_, pre=None):          # the trunk of oracle.nerf_mlp with the input widths read off the weights
        F = torch.nn.functional
        x, v = emb[:, :in_ch], emb[:, in_ch:]
        h = x
        for i in range(8):
            z = F.linear(h, sd_[f"pts_linears.{i}.weight"], sd_[f"pts_linears.{i}.bias"])
            if pre is not None:
                pre.append(z.detach())
            h = F.relu(z)
            if i == 4:
                h = torch.cat([x, h], -1)
        sigma = F.linear(h, sd_["alpha_linear.weight"], sd_["alpha_linear.bias"])
        feat = F.linear(h, sd_["feature_linear.weight"], sd_["feature_linear.bias"])
        zv = F.linear(torch.cat([feat, v], -1), sd_["views_linears.0.weight"], sd_["views_linears.0.bias"])
        if pre is not None:
            pre.append(zv.detach())
        return torch.cat([F.linear(F.relu(zv), sd_["rgb_linear.weight"], sd_["rgb_linear.bias"]), sigma], -1)

    sd_o = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    emb, cot = emb.double(), cot.double()
    # ReLU makes the parameter gradients discontinuous: a pre-activation within the forward's rounding error of zero may
    # take the other branch and move gradient entries by O(1e-2).  Rows with such a value get a
    # zero cotangent; the comparison is sharp on the rest.
    pre = []
    oracle({k: v.double() for k, v in sd.items()}, pre)
    near = torch.stack([(z.abs() < 1e-5).any(-1) for z in pre]).any(0)
    cot = cot * (~near).double()[:, None]
    ref = oracle(sd_o)
    (ref * cot).sum().backward()
    net = P.NeRF(D=8, W=256, input_ch=in_ch, input_ch_views=view_ch, output_ch=5, skips=[4], use_viewdirs=True,
                 precision=precision)
    net.load_state_dict(sd)
    net = net.to(dev())
    out = net(g(emb.float()))
    err = maxdiff(out, ref.detach().float())
    print(f"embedded {in_ch}|{view_ch}, {precision}: forward max err {err:.2e}")
    assert err <= 1e-5 * max(1.0, float(ref.detach().abs().max()))
    (out * g(cot.float())).sum().backward()
    worst = 0.0
    for name, prm in net.named_parameters():
        r = sd_o[name].grad.float()
        scale = max(float(r.abs().max()), 1e-6)
        worst = max(worst, maxdiff(prm.grad, r) / scale)
    print(f"embedded {in_ch}|{view_ch}, {precision}: worst gradient error / max|g| over the 24 tensors {worst:.2e} "
          f"({int(near.sum())} of {N} rows muted)")
    assert worst <= 6e-3


# ----------------------------------------------------------------------------- networks without view directions
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_network_without_view_directions(P, precision, tmp_path):
    """use_viewdirs=False (run_nerf_helpers.py:102-103, 125-126: `output_linear` on the trunk's last layer): the four
    outputs are expressed exactly in the view-dependent head the kernels implement (NeRF.param_list) and autograd
    carries the gradients back to output_linear.  Both entries -- forward(embedded) and the fused query(pts, None) --
    against the same network in fp64 torch; then the reference's own route: create_nerf(args) with
    use_viewdirs=False, render, loss.backward(), both Adams."""
    F = torch.nn.functional
    torch.manual_seed(31)
    net = P.NeRF(D=8, W=256, input_ch=63, input_ch_views=0, output_ch=5, skips=[4], use_viewdirs=False,
                 precision=precision).to(dev())
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(37)
    pts = (torch.rand(7, 43, 3, generator=gen) * 2 - 1) * 1.5          # 301 rows: a ragged tile
    cot = torch.randn(7, 43, 4, generator=gen)

    def ref(sd_, x, pre=None):
        h = x
        for i in range(8):
            z = F.linear(h, sd_[f"pts_linears.{i}.weight"], sd_[f"pts_linears.{i}.bias"])
            if pre is not None:
                pre.append(z.detach())
            h = F.relu(z)
            if i == 4:
                h = torch.cat([x, h], -1)
        return F.linear(h, sd_["output_linear.weight"], sd_["output_linear.bias"])

    emb_fn, _ = P.get_embedder(10, 0)
    x = emb_fn(pts.reshape(-1, 3)).double()
    # (rows with a trunk pre-activation within the forward's rounding error of zero get no cotangent: DESIGN.md section 6)
    pre = []
    ref(sd, x, pre)
    near = torch.stack([(z.abs() < 1e-5).any(-1) for z in pre]).any(0)
    cot = cot * (~near).float().reshape(7, 43, 1)
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out_ref = ref(sd_o, x)
    (out_ref[:, :4] * cot.reshape(-1, 4).double()).sum().backward()
    tol = 1e-5
    out_q = net.query(g(pts), None)
    assert out_q.shape == (7, 43, 5) and float(out_q[..., 4].detach().abs().max()) == 0.0
    err_q = maxdiff(out_q[..., :4].reshape(-1, 4), out_ref[:, :4].detach().float())
    out_f = net(g(x.float()))
    err_f = maxdiff(out_f[..., :4], out_ref[:, :4].detach().float())
    print(f"no view directions, {precision}: forward max err query {err_q:.2e}, forward(embedded) {err_f:.2e}")
    assert err_q <= tol and err_f <= tol
    (out_q[..., :4] * g(cot)).sum().backward()
    gtol = 2e-4 if precision == "fp32" else 6e-3
    worst = 0.0
    for name, prm in net.named_parameters():
        r = sd_o[name].grad
        if r is None:                       # views_linears: unused by this network, in the reference as well
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0
            continue
        r = r.float()
        if name.startswith("output_linear"):
            r, got = r[:4], prm.grad[:4].cpu()      # (the fifth output never reaches the loss)
        else:
            got = prm.grad.cpu()
        worst = max(worst, float((got - r).abs().max()) / max(float(r.abs().max()), 1e-6))
    print(f"no view directions, {precision}: worst gradient error / max|g| {worst:.2e}")
    assert worst <= gtol
    # the reference's route
    (tmp_path / "exp").mkdir()
    args = nvs_args(str(tmp_path), precision, use_viewdirs=False)
    kw, _, _, grad_vars, opt, opt_c = P.create_nerf(args, device=dev())
    batch, target = orc.synthetic_blender_rays(64, seed=2)
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    before = [p.detach().clone() for p in kw["network_fine"].parameters()]
    rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=(g(batch[:, 0:3]), g(batch[:, 3:6])), near=2.0,
                                      far=6.0, retraw=True, **kw)
    loss = P.img2mse(rgb, g(target)) + P.img2mse(extras["rgb0"], g(target))
    opt.zero_grad(); opt_c.zero_grad()
    loss.backward()
    opt.step(); opt_c.step()
    moved = max(float((a - b.detach()).abs().max()) for a, b in zip(before, kw["network_fine"].parameters()))
    assert torch.isfinite(rgb).all() and 0.0 < moved <= 5.5e-4


@pytest.mark.parametrize("shape", [(8, 128, True), (6, 256, True), (7, 64, False), (6, 32, True), (4, 128, True),
                                   (2, 256, False), (6, 256, True, 2), (5, 96, True, 1), (4, 128, False, 0)])
def test_narrower_and_shallower_networks(P, shape):
    """netwidth < 256, netdepth 6 / 7 and a skip after another layer (with one to three layers behind it) are zero-padded
    / identity-extended into the compiled 8 x 256 network (NeRF.param_list) -- exactly: fp32 mode against the same
    network in fp64 torch, forward and every real parameter's gradient, fused entry and embedded entry."""
    D, Wd, use_viewdirs = shape[:3]
    skip = shape[3] if len(shape) > 3 else 4
    F = torch.nn.functional
    torch.manual_seed(41)
    net = P.NeRF(D=D, W=Wd, input_ch=63, input_ch_views=27 if use_viewdirs else 0, output_ch=5, skips=[skip],
                 use_viewdirs=use_viewdirs, precision="fp32").to(dev())
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(43)
    pts = (torch.rand(5, 37, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(5, 3, generator=gen), dim=-1)
    cot = torch.randn(5, 37, 4, generator=gen)
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    x = emb_fn(pts.reshape(-1, 3)).double()
    v = embd_fn(vd[:, None].expand(5, 37, 3).reshape(-1, 3)).double()
    h = x
    for i in range(D):
        h = F.relu(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]))
        if i == skip:      # (netdepth <= 4: the default skips=[4] never takes effect, run_nerf_helpers.py:109-112)
            h = torch.cat([x, h], -1)
    if use_viewdirs:
        sigma = F.linear(h, sd["alpha_linear.weight"], sd["alpha_linear.bias"])
        feat = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
        hv = F.relu(F.linear(torch.cat([feat, v], -1), sd["views_linears.0.weight"], sd["views_linears.0.bias"]))
        ref = torch.cat([F.linear(hv, sd["rgb_linear.weight"], sd["rgb_linear.bias"]), sigma], -1)
    else:
        ref = F.linear(h, sd["output_linear.weight"], sd["output_linear.bias"])[:, :4]
    (ref * cot.reshape(-1, 4).double()).sum().backward()
    out = net.query(g(pts), g(vd) if use_viewdirs else None)[..., :4]
    err = maxdiff(out.reshape(-1, 4), ref.detach().float())
    emb_in = torch.cat([x, v], -1) if use_viewdirs else x
    err_e = maxdiff(net(g(emb_in.float()))[..., :4], ref.detach().float())
    (out * g(cot)).sum().backward()
    worst = 0.0
    for name, prm in net.named_parameters():
        r = sd[name].grad
        if r is None:
            continue
        r = r.float()
        got = prm.grad.cpu()
        if name.startswith("output_linear"):
            r, got = r[:4], got[:4]
        worst = max(worst, float((got - r).abs().max()) / max(float(r.abs().max()), 1e-6))
    print(f"D={D} W={Wd} viewdirs={use_viewdirs}: forward {err:.2e} (embedded entry {err_e:.2e}), worst gradient error / max|g| {worst:.2e}")
    assert err <= 1e-5 and err_e <= 1e-5 and worst <= 2e-4
    if len(shape) > 3:      # (create_nerf always builds skips=[4], run_plnerf.py:425-437: the route below has no other skip)
        return
    # the reference's route with these arguments: create_nerf, render, backward, both Adams (f16x3, the default mode)
    args = nvs_args(_ckdir(), "f16x3", netdepth=D, netwidth=Wd, netdepth_fine=D, netwidth_fine=Wd, use_viewdirs=use_viewdirs)
    kw, _, _, grad_vars, opt, opt_c = P.create_nerf(args, device=dev())
    batch, target = orc.synthetic_blender_rays(64, seed=4)
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    before = [p.detach().clone() for p in kw["network_fine"].parameters()]
    rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=(g(batch[:, 0:3]), g(batch[:, 3:6])), near=2.0,
                                      far=6.0, retraw=True, **kw)
    loss = P.img2mse(rgb, g(target)) + P.img2mse(extras["rgb0"], g(target))
    opt.zero_grad(); opt_c.zero_grad()
    loss.backward()
    opt.step(); opt_c.step()
    moved = max(float((a - b.detach()).abs().max()) for a, b in zip(before, kw["network_fine"].parameters()))
    assert torch.isfinite(rgb).all() and 0.0 < moved <= 5.5e-4


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16x3"])
def test_input_gradients_match_the_oracle(P, precision):
    """What autograd gives the reference module when its inputs require a gradient (no reference training path asks: the
    samples are detached, run_plnerf.py:728): d / d pts and d / d viewdirs through the fused entry (in-kernel encoding), and
    d / d (embedded rows) through NeRF.forward -- plnerf_mlp_input_grad from the dgrad kernel's planes, then the
    encoding's derivative -- against the oracle's autograd on the host; the parameter gradients of the same backward
    are unchanged by the request."""
    sd = orc.closed_form_state_dict(1, True)
    gen = torch.Generator().manual_seed(77)
    R, S = 70, 23                                  # (1610 rows: the last 32-row tile is ragged)
    pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    cot = torch.randn(R, S, 4, generator=gen)
    # the reference in fp64: the encoding's derivative multiplies the rows' gradient by up to 2^9 and sums terms that
    # cancel, so the oracle's own fp32 autograd is 1.2e-3 of max |g| from it on these inputs -- the kernel path is not
    sd64 = {k: v.double() for k, v in sd.items()}
    p_o, v_o = pts.double().requires_grad_(True), vd.double().requires_grad_(True)
    (orc.query_network(sd64, p_o, v_o) * cot.double()).sum().backward()
    tol = 2e-5 if precision == "fp32" else 4e-3      # (16-bit modes: half planes in the backward)

    def smallest_preactivation(emb64):
        """Per row: the smallest |pre-activation| of any ReLU unit, in fp64 (the trunk's eight layers and the view layer)."""
        enc_xyz, enc_dir = emb64[..., :orc.XYZ_CH], emb64[..., orc.XYZ_CH:]
        h, small = enc_xyz, torch.full((emb64.shape[0],), float("inf"), dtype=torch.float64)
        F = torch.nn.functional
        for i in range(orc.DEPTH):
            z = F.linear(h, sd64[f"pts_linears.{i}.weight"], sd64[f"pts_linears.{i}.bias"])
            small = torch.minimum(small, z.abs().min(-1).values)
            h = F.relu(z)
            if i == orc.SKIP_AFTER:
                h = torch.cat([enc_xyz, h], -1)
        feat = F.linear(h, sd64["feature_linear.weight"], sd64["feature_linear.bias"])
        zv = F.linear(torch.cat([feat, enc_dir], -1), sd64["views_linears.0.weight"], sd64["views_linears.0.bias"])
        return torch.minimum(small, zv.abs().min(-1).values)
    # A row may sit beyond `tol` for ONE reason: a unit whose pre-activation is within the forward's rounding error of zero
    # takes the other side of its ReLU than the fp64 reference does, and the row's gradient differs by that unit's whole
    # contribution.  Asserted: every such row has a unit with |z| (fp64) below the mode's forward error
    # -- and at most three rows do.
    flip_below = {"fp32": 2e-6, "f16x3": 1e-5, "bf16x3": 5e-5}[precision]      # (the mode's forward error on a hidden unit)
    net = make_net(P, sd, precision)
    p_g, v_g = g(pts).requires_grad_(True), g(vd).requires_grad_(True)
    (net.query(p_g, v_g) * g(cot)).sum().backward()
    emb_q = torch.cat([orc.positional_encoding(pts.reshape(-1, 3), orc.XYZ_FREQS),
                       orc.positional_encoding(vd[:, None, :].expand(R, S, 3).reshape(-1, 3), orc.DIR_FREQS)], -1).double()
    small = smallest_preactivation(emb_q)                     # [R * S]
    small_ray = small.reshape(R, S).min(-1).values            # (a direction's gradient sums its ray's rows)
    for got, ref, what, sm in ((p_g.grad, p_o.grad, "pts", small), (v_g.grad, v_o.grad, "viewdirs", small_ray)):
        row_err = (got.cpu().double() - ref).abs().reshape(-1, 3).max(-1).values / float(ref.abs().max())
        bad = row_err > tol
        print(f"{precision} d/d {what}: median row {float(row_err.median()):.2e}, worst {float(row_err.max()):.2e} of max |g|, "
              f"{int(bad.sum())} rows beyond {tol:g}" + (f", their smallest |z| {[f'{float(x):.1e}' for x in sm[bad]]}" if bad.any() else ""))
        assert got.shape == ref.shape and int(bad.sum()) <= 3 and float(row_err.max()) <= 5e-2, (what, float(row_err.max()))
        assert bool((sm[bad] < flip_below).all()), f"{what}: a row beyond {tol:g} without a pre-activation near zero"
    w_with = [p.grad.clone() for p in net.parameters()]
    net.zero_grad()
    (net.query(g(pts), g(vd)) * g(cot)).sum().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(w_with, net.parameters()))
    # only one of the two inputs asks
    p_only = g(pts).requires_grad_(True)
    (net.query(p_only, g(vd)) * g(cot)).sum().backward()
    assert torch.equal(p_only.grad, p_g.grad)
    # the embedded entry: rows of 63 + 27 channels
    emb = torch.cat([orc.positional_encoding(pts.reshape(-1, 3), orc.XYZ_FREQS),
                     orc.positional_encoding(vd[:, None, :].expand(R, S, 3).reshape(-1, 3), orc.DIR_FREQS)], -1)
    e_o = emb.double().requires_grad_(True)
    (orc.nerf_mlp(sd64, e_o) * cot.reshape(-1, 4).double()).sum().backward()
    e_g = g(emb).requires_grad_(True)
    (net(e_g) * g(cot.reshape(-1, 4))).sum().backward()
    # (a pre-activation within fp32 rounding of zero takes the other side of its ReLU in fp64: such a row's gradient
    # differs by that unit's whole contribution -- DESIGN.md section 6 -- so rows are counted, as in test_gpu_fullsize.py)
    row_err = (e_g.grad.cpu().double() - e_o.grad).abs().max(-1).values / float(e_o.grad.abs().max())
    bad = row_err > tol
    small_e = smallest_preactivation(emb.double())
    print(f"{precision} d/d embedded: median row {float(row_err.median()):.2e}, worst {float(row_err.max()):.2e} of max |g|, "
          f"{int(bad.sum())} of {row_err.numel()} rows beyond {tol:g}" + (f", their smallest |z| {[f'{float(x):.1e}' for x in small_e[bad]]}" if bad.any() else ""))
    assert e_g.grad.shape == emb.shape and int(bad.sum()) <= 3 and float(row_err.max()) <= 5e-2
    assert bool((small_e[bad] < flip_below).all()), "a row beyond the bound without a pre-activation near zero"


# ----------------------------------------------------------------------------- range of the half modes
def test_half_modes_flag_range_overflow_and_withhold_the_step(P):
    """`f16x3` / `f16` clamp at the IEEE-half maximum (65,504).  A forward that gets there must not pass silently: the
    kernels set the packed buffer's status word, NeRF.check_range() raises, and the guarded Adam leaves the weights
    alone for as long as the word is set.  The same network in `fp32` is exact and sets nothing; in `bf16x3` (fp32
    exponent range in the forward) the forward is exact too, inference sets nothing, but the TRAINING forward writes
    IEEE-half saved planes for the backward: clamping there sets PLNERF_RANGE_SAVED (forward right, gradients wrong),
    check_range() raises and the guarded step is withheld as well."""
    from plnerf_amd import _lib
    sd = orc.closed_form_state_dict(2, False)
    sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * 6.0e4        # weights within the half range, h0 ~ 1e5..1e6 beyond it
    sd["pts_linears.1.weight"] = sd["pts_linears.1.weight"] * 1.0e-5       # (back to O(1) for the rest of the trunk)
    assert float(sd["pts_linears.0.weight"].abs().max()) < 65504.0
    gen = torch.Generator().manual_seed(3)
    pts = (torch.rand(6, 40, 3, generator=gen) * 2 - 1) * 2.0
    vd = torch.nn.functional.normalize(torch.randn(6, 3, generator=gen), dim=-1)
    ref = orc.query_network(sd, pts, vd)
    for prec, flagged in (("fp32", False), ("bf16x3", False), ("f16x3", True), ("f16", True)):
        net = make_net(P, sd, prec)
        for grad in (False, True):          # inference kernel, then the training forward
            with torch.set_grad_enabled(grad):
                raw = net.query(g(pts), g(vd))
            err = maxdiff(raw, ref)
            bits = net.range_status()
            print(f"{prec} grad={grad}: err {err:.2e}, status {bits}")
            assert bool(bits & _lib.RANGE_ACTIVATION) == flagged, (prec, grad, bits)
            assert bool(bits & _lib.RANGE_SAVED) == (prec == "bf16x3" and grad), (prec, grad, bits)
            if not flagged:
                assert err <= 2e-5 * (1.0 + float(ref.abs().max())), (prec, err)
        if flagged or prec == "bf16x3":
            with pytest.raises(FloatingPointError, match="exceeded the IEEE-half range"):
                net.check_range()
            assert net.range_status() == 0                                   # cleared by the check
        else:
            net.check_range()
    # weights beyond the range are caught at packing time.  What is packed for the view layer is W_c = W_vf W_f (the
    # composed layer of the 16-bit modes, mlp_layout.h): feature_linear's own entries never become halves, so a large one
    # is flagged exactly when it takes an entry of W_c out of the range -- and computed exactly when it does not.
    def weight_flag(key, value):
        sd_w = orc.closed_form_state_dict(2, False)
        sd_w[key][3, 5] = value
        net = make_net(P, sd_w, "f16x3")
        with torch.no_grad():
            raw = net.query(g(pts), g(vd))
        return net.range_status() & _lib.RANGE_WEIGHT, raw, sd_w
    assert weight_flag("pts_linears.3.weight", 1.0e5)[0]
    assert weight_flag("feature_linear.weight", 1.0e9)[0]
    sd_c = orc.closed_form_state_dict(2, False)
    wc_big = float((sd_c["views_linears.0.weight"][:, 3].abs().max() * 1.0e5))
    assert wc_big < 6.0e4, wc_big                                             # (this entry of feature_linear stays inside W_c's range)
    flag, raw, sd_w = weight_flag("feature_linear.weight", 1.0e5)
    assert not flag
    ref_w = orc.query_network(sd_w, pts, vd)
    assert maxdiff(raw, ref_w) <= 2e-5 * (1.0 + float(ref_w.abs().max()))
    # the guarded optimizer: a step computed from a clamped forward does not reach the weights
    for prec, bit in (("f16x3", _lib.RANGE_ACTIVATION), ("bf16x3", _lib.RANGE_SAVED)):
        net = make_net(P, sd, prec)
        opt = P.FlatAdam(net.parameters(), lr=1e-3, guards=[net])            # (the network: its word is resolved per step)
        before = [p.detach().clone() for p in net.parameters()]
        for _ in range(2):
            opt.zero_grad()
            (net.query(g(pts), g(vd)) ** 2).sum().backward()
            opt.step()
        assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters())), prec
        # the host advanced its step counts before each launch; the kernels counted what they withheld
        assert float(opt.state[next(net.parameters())]['step']) == 2.0
        assert opt.withheld_steps() == 2
        assert float(opt.state[next(net.parameters())]['step']) == 0.0 and opt.withheld_steps() == 0
        assert net.range_status(reset=True) & bit, prec
        net.load_state_dict(orc.closed_form_state_dict(2, False))                # a sane network again: steps apply
        opt.zero_grad()
        (net.query(g(pts), g(vd)) ** 2).sum().backward()
        opt.step()
        assert net.range_status() == 0 and opt.withheld_steps() == 0
        assert float(opt.state[next(net.parameters())]['step']) == 1.0
        sane = list(orc.closed_form_state_dict(2, False).values())
        assert any(not torch.equal(q, p.detach().cpu()) for q, p in zip(sane, net.parameters())), prec


# ----------------------------------------------------------------------------- shapes outside the compiled trunk: generic.py
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (37, 5, 3), (64, 64, 16), (65, 63, 17), (300, 257, 129), (1000, 1, 512), (3, 700, 90)])
def test_generic_gemm_vs_fp64(P, M, N, K):
    """plnerf_gemm_f32 (exact-fp32 MFMA, 64 x 64 tiles, ragged edges) in every form generic.LinearFn uses it: a layer
    (x W^T + b, relu), its input gradient (the relu's derivative gated into A), its weight gradient with the bias gradient as
    the ones column (A transposed by strides), and accumulation -- against fp64 torch."""
    from plnerf_amd import _lib as L
    gen = torch.Generator().manual_seed(M * 1000 + N * 10 + K)
    x, w, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)

    def gemm(a, a_rs, a_cs, bm, b_rs, b_cs, m, n, k, bias=None, gate=None, relu=0, acc=0, ones=0, out=None, splits=1):
        c = torch.full((m, n), float("nan"), device=dev()) if out is None else out
        part = torch.full((splits * m * n,), float("nan"), device=dev()) if splits > 1 else None
        L.check(L.lib().plnerf_gemm_f32(L.dptr(a), a_rs, a_cs, L.dptr(bm), b_rs, b_cs, L.dptr(bias), L.dptr(gate), m, n, k, relu, acc,
                                        ones, L.dptr(c), c.stride(0), splits, L.dptr(part), L.stream()), "plnerf_gemm_f32")
        return c
    tol = lambda ref: 2e-6 * (1.0 + float(ref.abs().max())) * max(1.0, K ** 0.5 / 4)
    y_ref = torch.relu(x.double() @ w.double().T + b.double())
    y = gemm(g(x), K, 1, g(w), 1, K, M, N, K, bias=g(b), relu=1)
    assert maxdiff(y, y_ref.float()) <= tol(y_ref)
    gy = torch.randn(M, N, generator=gen)
    gated = gy.double() * (y_ref > 0)
    gx = gemm(g(gy), N, 1, g(w), K, 1, M, K, N, gate=y)
    gx_ref = gated @ w.double()
    assert maxdiff(gx, gx_ref.float()) <= 2e-6 * (1.0 + float(gx_ref.abs().max())) * max(1.0, N ** 0.5 / 4)
    gwb = gemm(g(gy), 1, N, g(x), K, 1, N, K + 1, M, gate=y, ones=1)
    gwb_ref = torch.cat([gated.T @ x.double(), gated.sum(0)[:, None]], 1)
    assert maxdiff(gwb, gwb_ref.float()) <= 2e-6 * (1.0 + float(gwb_ref.abs().max())) * max(1.0, M ** 0.5 / 4)
    # the same with the k range (here: the rows) dealt out over several workgroups per tile and summed in order: more ranges
    # than 16-deep stages must not leave an unwritten partial in the sum (NaN-filled above)
    for splits in (2, 7, 64):
        gwb_s = gemm(g(gy), 1, N, g(x), K, 1, N, K + 1, M, gate=y, ones=1, splits=splits)
        assert torch.isfinite(gwb_s).all(), splits
        assert maxdiff(gwb_s, gwb_ref.float()) <= 2e-6 * (1.0 + float(gwb_ref.abs().max())) * max(1.0, M ** 0.5 / 4), splits
    y_s = gemm(g(x), K, 1, g(w), 1, K, M, N, K, bias=g(b), relu=1, splits=3)
    assert maxdiff(y_s, y_ref.float()) <= tol(y_ref)
    # accumulate into an existing C, no bias, no relu
    c0 = torch.randn(M, N, generator=gen)
    c = gemm(g(x), K, 1, g(w), 1, K, M, N, K, acc=1, out=g(c0).clone())
    assert maxdiff(c, (c0.double() + x.double() @ w.double().T).float()) <= tol(y_ref)


@pytest.mark.parametrize("shape", [dict(D=10, W=512, skips=[4, 7], L=10, Lv=4), dict(D=9, W=320, skips=[4], L=10, Lv=4),
                                   dict(D=8, W=256, skips=[4], L=12, Lv=6), dict(D=8, W=256, skips=[2], L=10, Lv=4),
                                   dict(D=12, W=96, skips=[3, 6, 9], L=5, Lv=2), dict(D=9, W=384, skips=[4], L=10, Lv=0)])
def test_network_shapes_outside_the_trunk_run_layer_by_layer(P, shape):
    """netdepth > 8, netwidth > 256, several live skips, multires > 10 / multires_views > 4 (run_nerf_helpers.py:76-128
    builds any of them; run_plnerf.py:784-799): not expressible in the compiled trunk, served by generic.py -- one exact-fp32
    MFMA product per nn.Linear, plnerf_embed_rows for the encoding.  Through run_network (the reference's call) against the
    same module in fp64 torch: forward 1e-5, every parameter's gradient 2e-4 of its max |g|."""
    F = torch.nn.functional
    D, Wd, skips, Lx, Lv = shape["D"], shape["W"], shape["skips"], shape["L"], shape["Lv"]
    use_viewdirs = Lv > 0
    torch.manual_seed(47)
    emb_fn, in_ch = P.get_embedder(Lx, 0)
    embd_fn, in_ch_v = P.get_embedder(Lv, 0) if use_viewdirs else (None, 0)
    net = P.NeRF(D=D, W=Wd, input_ch=in_ch, input_ch_views=in_ch_v, output_ch=5, skips=skips, use_viewdirs=use_viewdirs,
                 precision="f16x3").to(dev())
    assert not net.is_supported()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(53)
    R, S = 7, 41
    pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    cot = torch.randn(R, S, 4, generator=gen)
    x = emb_fn(pts.reshape(-1, 3).double())
    h = x
    for i in range(D):
        h = F.relu(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]))
        if i in skips:
            h = torch.cat([x, h], -1)
    if use_viewdirs:
        v = embd_fn(vd[:, None].expand(R, S, 3).reshape(-1, 3).double())
        sigma = F.linear(h, sd["alpha_linear.weight"], sd["alpha_linear.bias"])
        feat = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
        hv = F.relu(F.linear(torch.cat([feat, v], -1), sd["views_linears.0.weight"], sd["views_linears.0.bias"]))
        ref = torch.cat([F.linear(hv, sd["rgb_linear.weight"], sd["rgb_linear.bias"]), sigma], -1)
    else:
        ref = F.linear(h, sd["output_linear.weight"], sd["output_linear.bias"])
    (ref[:, :4] * cot.reshape(-1, 4).double()).sum().backward()
    out = P.run_network(g(pts), g(vd) if use_viewdirs else None, net, emb_fn, embd_fn)
    assert out.shape == (R, S, ref.shape[-1])
    err = maxdiff(out.reshape(-1, ref.shape[-1]), ref.detach().float())
    (out[..., :4] * g(cot)).sum().backward()
    worst = 0.0
    for name, prm in net.named_parameters():
        r = sd[name].grad
        if r is None:      # (views_linears without view directions: not on the path, as in the reference)
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0
            continue
        worst = max(worst, float((prm.grad.cpu().double() - r).abs().max()) / max(float(r.abs().max()), 1e-9))
    print(f"generic route D={D} W={Wd} skips={skips} multires={Lx}|{Lv}: forward {err:.2e}, worst gradient error / max|g| {worst:.2e}")
    assert err <= 1e-5 * (1.0 + float(ref.abs().max())) and worst <= 2e-4


def test_create_nerf_trains_a_shape_outside_the_trunk(P):
    """The reference's route end to end with netwidth 512 / netdepth 10 (create_nerf warns once per network and serves them
    on the generic route): render, loss, backward, both Adams -- finite, the weights move by an Adam step."""
    import warnings
    args = nvs_args(_ckdir(), "f16x3", netdepth=10, netwidth=512, netdepth_fine=9, netwidth_fine=320)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        kw, _, _, grad_vars, opt, opt_c = P.create_nerf(args, device=dev())
    assert sum("layer by layer" in str(w.message) for w in caught) == 2
    batch, target = orc.synthetic_blender_rays(48, seed=4)
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    before = [p.detach().clone() for p in kw["network_fine"].parameters()]
    rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=(g(batch[:, 0:3]), g(batch[:, 3:6])), near=2.0,
                                      far=6.0, retraw=True, **kw)
    loss = P.img2mse(rgb, g(target)) + P.img2mse(extras["rgb0"], g(target))
    opt.zero_grad(); opt_c.zero_grad()
    loss.backward()
    opt.step(); opt_c.step()
    moved = max(float((a - b.detach()).abs().max()) for a, b in zip(before, kw["network_fine"].parameters()))
    assert torch.isfinite(rgb).all() and torch.isfinite(loss) and 0.0 < moved <= 5.5e-4
