"""HIP path vs the CPU oracle and the reference-generated golden vectors, on a real MI355X.

Every test calls through the C ABI of libplnerf_hip.so (via plnerf_amd's ctypes binding).
Tolerances: bit-exact for searchsorted indices; 1e-5 (abs+rel) for rendered quantities, per
stage on identical inputs (the end-to-end pipeline is discontinuous in the
sampler, so per-stage parity is the meaningful statement).
"""
import os

import numpy as np
import pytest
import torch

from gpu_support import P, T, ambiguous_rows, assert_close, depth_setup, dev, g, g5_batch, make_net, maxdiff, quad_case
from oracle import plnerf_oracle as orc
from run_args import depth_args_of

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- quadrature
def test_quad_fwd_golden(P, golden):
    gd = golden("g2_raw2outputs")
    for c in range(int(gd["n_cases"])):
        p = f"c{c}_"
        ffix = bool(gd[p + "farcolorfix"]) if (p + "farcolorfix") in gd.files else False
        std = float(gd[p + "noise_std"])
        res = P.raw2outputs(g(T(gd[p + "raw"])), g(T(gd[p + "z"])), g(T(gd[p + "near"])), g(T(gd[p + "far"])),
                            g(T(gd[p + "rays_d"])), str(gd[p + "mode"]), str(gd[p + "color_mode"]),
                            raw_noise_std=std, pytest=std > 0, white_bkgd=bool(gd[p + "white_bkgd"]),
                            farcolorfix=ffix)
        for nme, v in zip(["rgb_map", "disp_map", "acc_map", "weights", "depth_map", "tau", "T"], res):
            if v is None:
                assert (p + nme) not in gd.files
            else:
                # tau holds 1e10 sentinels; disp can be huge when depth ~ 0: relative bound carries those
                assert_close(v, gd[p + nme], what=f"g2 case {c} {nme}")


@pytest.mark.parametrize("mode,cmode", [("linear", "midpoint"), ("linear", "left"), ("constant", "midpoint")])
@pytest.mark.parametrize("S", [64, 192, 37, 65])      # (65: one element past the scan's 64-lane chunk in both modes)
def test_quad_fwd_bwd_vs_oracle(P, mode, cmode, S):
    from plnerf_amd.functional import QuadratureFn
    R = 67
    raw, z, near, far, d, noise = quad_case(R, S, 7 + S)
    gen = torch.Generator().manual_seed(99)
    n = S + 1 if mode == "linear" else S
    cot = [torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen),
           torch.randn(R, n, generator=gen) * 0.1, torch.randn(R, generator=gen)]
    for wb in (False, True):
        # oracle
        raw_o = raw.clone().requires_grad_(True)
        ro = orc.raw2outputs(raw_o, z, near, far, d, mode, cmode, white_bkgd=wb, noise=noise)
        loss_o = sum((a * b).sum() for a, b in zip(ro[:5], cot))
        loss_o.backward()
        # HIP
        raw_h = g(raw).requires_grad_(True)
        rh = QuadratureFn.apply(raw_h, g(z), g(near), g(far), g(d), g(noise), mode, cmode, wb, False)
        for nme, a, b in zip(["rgb", "disp", "acc", "weights", "depth"], rh[:5], ro[:5]):
            assert_close(a, b, what=f"{mode}/{cmode}/S{S}/wb{wb} {nme}")
        if mode == "linear":
            assert_close(rh[5], ro[5], what="tau")
            assert_close(rh[6], ro[6], what="T")
        loss_h = sum((a * g(b)).sum() for a, b in zip(rh[:5], cot))
        loss_h.backward()
        ref = raw_o.grad
        scale = float(ref.abs().max())
        assert_close(raw_h.grad, ref, atol=1e-5 * max(scale, 1.0), rtol=2e-4,
                     what=f"{mode}/{cmode}/S{S}/wb{wb} d/draw")


def test_quad_edge_cases(P):
    # S == 2 (minimum), one ray, z ending exactly at far, all-negative density (acc == 0 -> disp NaN like the reference)
    raw = torch.randn(1, 2, 4)
    z = torch.tensor([[2.5, 6.0]])
    near, far, d = torch.full((1, 1), 2.0), torch.full((1, 1), 6.0), torch.tensor([[0.0, 0.0, -1.0]])
    for mode in ("linear", "constant"):
        ro = orc.raw2outputs(raw, z, near, far, d, mode, "midpoint")
        rh = P.raw2outputs(g(raw), g(z), g(near), g(far), g(d), mode, "midpoint")
        for a, b in zip(rh[:5], ro[:5]):
            assert_close(a, b, what=f"edge S=2 {mode}")
    raw2 = torch.randn(5, 16, 4)
    raw2[..., 3] = -1.0
    z2, _ = torch.sort(2 + 4 * torch.rand(5, 16), -1)
    near, far, d = torch.full((5, 1), 2.0), torch.full((5, 1), 6.0), torch.randn(5, 3)
    ro = orc.raw2outputs(raw2, z2, near, far, d, "constant", "midpoint")
    rh = P.raw2outputs(g(raw2), g(z2), g(near), g(far), g(d), "constant", "midpoint")
    for a, b in zip(rh[:5], ro[:5]):
        assert_close(a, b, what="edge empty-ray constant")
    # zero rays
    rh = P.raw2outputs(g(torch.zeros(0, 8, 4)), g(torch.zeros(0, 8)), g(torch.zeros(0, 1)), g(torch.zeros(0, 1)),
                       g(torch.zeros(0, 3)), "linear", "midpoint")
    assert rh[0].shape == (0, 3) and rh[3].shape == (0, 9)


# ----------------------------------------------------------------------------- samplers
def test_sample_pdf_golden_bit_exact(P, golden):
    from plnerf_amd import functional as Fn
    gd = golden("g3_sample_pdf")
    for c in range(int(gd["n_cases"])):
        bins, w, N = g(T(gd[f"c{c}_bins"])), g(T(gd[f"c{c}_weights"])), int(gd[f"c{c}_N"])
        s, inds = Fn.sample_const(bins, w, Fn.cpu_linspace(N, dev()), want_inds=True)
        assert torch.equal(inds.cpu(), T(gd[f"c{c}_det_inds"])), f"case {c}: det searchsorted indices differ"
        assert_close(s, gd[f"c{c}_det_samples"], what=f"g3 case {c} det samples")
        nbit = int((s.cpu() == T(gd[f"c{c}_det_samples"])).sum())
        print(f"g3 case {c}: {nbit}/{s.numel()} det samples bit-identical")
        u = Fn.numpy_uniform([bins.shape[0], N], dev())
        s, inds = Fn.sample_const(bins, w, u, want_inds=True)
        assert torch.equal(inds.cpu(), T(gd[f"c{c}_rnd_inds"])), f"case {c}: random-u indices differ"
        assert_close(s, gd[f"c{c}_rnd_samples"], what=f"g3 case {c} rnd samples")
        # public wrapper
        assert_close(P.sample_pdf(bins, w, N, det=True), gd[f"c{c}_det_samples"], what="sample_pdf wrapper")


def test_sample_pdf_bit_exact_large(P):
    """det=True indices bit-exact against torch's CPU kernels on 4096 rays at the BASELINE sizes."""
    from plnerf_amd import functional as Fn
    for B, N, seed in ((63, 128, 1), (127, 64, 2), (191, 64, 3), (9, 16, 4)):
        gen = torch.Generator().manual_seed(seed)
        R = 4096
        bins, _ = torch.sort(2.0 + 4.0 * torch.rand(R, B, generator=gen), -1)
        w = torch.rand(R, B - 1, generator=gen) ** 6
        w[::7] *= 1e-5
        s_ref, i_ref = orc.sample_pdf(bins, w, N, det=True, return_inds=True)
        s, inds = Fn.sample_const(g(bins), g(w), Fn.cpu_linspace(N, dev()), want_inds=True)
        assert torch.equal(inds.cpu(), i_ref), f"B={B}: {(inds.cpu() != i_ref).sum()} index mismatches"
        assert_close(s, s_ref, what=f"sample_pdf large B={B}")


def test_sample_pdf_every_bin_count(P):
    """The search indices depend on the LAST BIT of the cdf, i.e. on the association order of torch.sum / cumsum on the
    host (the pdf's normalisation): every weight count 1..70 and a few beyond, with weights that put draws exactly ON cdf
    entries (equal weights, u = k / (N - 1)) -- where one ulp decides the bin -- and with random ones.  (4 <= n <= 7 takes
    its own order in torch's vectorised sum: found in round 5 by tools/fuzz_samplers.py.)"""
    from plnerf_amd import functional as Fn
    R = 257
    for n in list(range(1, 71)) + [100, 127, 128, 129, 255, 256, 509, 510]:
        gen = torch.Generator().manual_seed(n)
        bins, _ = torch.sort(2.0 + 4.0 * torch.rand(R, n + 1, generator=gen), -1)
        w = torch.rand(R, n, generator=gen)
        w[: R // 3] = torch.round(w[: R // 3] * 4.0) * 0.25          # few distinct values: draws land ON cdf entries
        w[R // 3: R // 2] = 0.5                                       # all equal
        for N, det in ((33, True), (64, True), (50, False)):
            u = torch.rand(R, N, generator=gen) if not det else None
            s_ref, i_ref = orc.sample_pdf(bins, w, N, det=det, u=u, return_inds=True)
            s, inds = Fn.sample_const(g(bins), g(w), Fn.cpu_linspace(N, dev()) if det else g(u), want_inds=True)
            assert torch.equal(inds.cpu(), i_ref), f"n={n} N={N} det={det}: {int((inds.cpu() != i_ref).sum())} index mismatches"
            assert float((s.cpu() - s_ref).abs().max()) <= 1e-4, (n, N, det)


def test_sample_pl_golden(P, golden):
    from plnerf_amd import functional as Fn
    gd = golden("g4_sample_pl")
    for c in range(int(gd["n_cases"])):
        p = f"c{c}_"
        args = [g(T(gd[p + k])) for k in ("z", "weights", "tau", "T", "near", "far")]
        s, Tb, taub, binb, inds = Fn.sample_pl(*args, g(T(gd[p + "u"])), 1e-4, 1e-3, want_extras=True, want_inds=True)
        assert torch.equal(inds.cpu(), T(gd[p + "inds"])), f"g4 case {c}: indices differ"
        assert torch.equal(Tb.cpu(), T(gd[p + "T_below"]))
        assert torch.equal(taub.cpu(), T(gd[p + "tau_below"]))
        assert torch.equal(binb.cpu(), T(gd[p + "bin_below"]))
        assert_close(s, gd[p + "samples"], what=f"g4 case {c} samples")
        # public wrapper with the reference's pytest draw
        out = P.sample_pdf_reformulation(*args, int(gd[p + "N"]), det=False, pytest=True)
        assert_close(out[0], gd[p + "samples"], what="sample_pdf_reformulation wrapper")


def test_sample_pl_vs_oracle_large_and_det(P):
    from plnerf_amd import functional as Fn
    R, S, N = 2048, 64, 128
    raw, z, near, far, d, _ = quad_case(R, S, 21)
    _, _, _, w, _, tau, Tr = orc.raw2outputs(raw, z, near, far, d, "linear", "midpoint")
    u = torch.rand(R, N, generator=torch.Generator().manual_seed(5))
    ref = orc.sample_pdf_reformulation(z, w, tau, Tr, near, far, N, u=u, return_inds=True)
    out = Fn.sample_pl(g(z), g(w), g(tau), g(Tr), g(near), g(far), g(u), 1e-4, 1e-3, want_extras=True,
                       want_inds=True)
    assert torch.equal(out[4].cpu(), ref[4])
    # The reference's closed form is ill-conditioned in fp32 where the discriminant cancels
    # (tau0^2 ~ 2 dtau ln/span at large tau): a 1-ulp difference between the device logf/sqrtf and
    # the CPU's is amplified to ~1e-4 on a handful of draws.  Bound: 1e-5 for >= 99.99 % of the
    # samples, 1e-3 for the rest.
    err = (out[0].cpu() - ref[0]).abs()
    frac_bad = float((err > 1e-5 + 1e-5 * ref[0].abs()).float().mean())
    print(f"sample_pl large: max err {float(err.max()):.3e}, fraction beyond 1e-5: {frac_bad:.2e}")
    assert frac_bad <= 1e-4 and float(err.max()) <= 1e-3
    # det=True (u reaches 1.0): defined by clamping, equals the oracle's clamp
    ref = orc.sample_pdf_reformulation(z, w, tau, Tr, near, far, N, det=True)[0]
    out = P.sample_pdf_reformulation(g(z), g(w), g(tau), g(Tr), g(near), g(far), N, det=True)[0]
    assert_close(out, ref, what="sample_pl det")


def test_sampler_backward_vs_oracle_autograd(P):
    """The depth-supervised variant back-propagates through sample_pdf_reformulation
    (depth_supervised_exps/run_nerf_sample_based_depth.py:923-934): d samples / d (tau, T) from
    plnerf_sample_pl_bwd, and d (tau, T) / d raw joined into plnerf_quad_bwd, against torch autograd
    on the oracle's restatement of the same functions.

    The closed form is ill-conditioned in fp32 (the discriminant cancels; see the forward test): the
    oracle's own fp32 autograd differs from its fp64 autograd by ~1e-3 of max|g| on g_tau.  The
    yardstick is therefore the fp64 oracle, and the bound is the fp32 oracle's own distance from it
    (x2, + 1e-5)."""
    from plnerf_amd import functional as Fn

    def rel(a, b):
        return float((a.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-300)

    for (R, S, N, seed) in [(64, 64, 64, 3), (33, 192, 128, 4), (16, 21, 77, 5)]:
        raw, z, near, far, d, _ = quad_case(R, S, seed)
        gen = torch.Generator().manual_seed(seed)
        u = torch.rand(R, N, generator=gen) * 0.999
        cot = torch.randn(R, N, generator=gen)
        cot_rgb = torch.randn(R, 3, generator=gen)
        with torch.no_grad():
            _, _, _, w, _, tau, Tr = orc.raw2outputs(raw, z, near, far, d, "linear", "midpoint")

        # stage 1: sampler alone, gradients with respect to tau and T
        def sampler_grads(dt):
            tau_r, T_r = tau.to(dt).clone().requires_grad_(True), Tr.to(dt).clone().requires_grad_(True)
            s_ref = orc.sample_pdf_reformulation(z.to(dt), w.to(dt), tau_r, T_r, near.to(dt), far.to(dt), N,
                                                 u=u.to(dt))[0]
            (s_ref * cot.to(dt)).sum().backward()
            return tau_r.grad, T_r.grad
        ref64, ref32 = sampler_grads(torch.float64), sampler_grads(torch.float32)
        tau_h, T_h = g(tau).requires_grad_(True), g(Tr).requires_grad_(True)
        s_hip = Fn.sample_pl(g(z), g(w), tau_h, T_h, g(near), g(far), g(u), 1e-4, 1e-3)
        (s_hip * g(cot)).sum().backward()
        for name, a, b64, b32 in (("g_tau", tau_h.grad, ref64[0], ref32[0]), ("g_T", T_h.grad, ref64[1], ref32[1])):
            e_hip, e_orc = rel(a, b64), rel(b32, b64)
            print(f"sampler bwd R={R} S={S} N={N}: {name} err vs fp64 oracle: HIP {e_hip:.3e}, fp32 oracle {e_orc:.3e}")
            assert e_hip <= 2 * e_orc + 1e-5, (name, e_hip, e_orc)
            # (round 6: the kernel evaluates the cancelling derivative in fp64 from the fp32 inputs -- it is the exact gradient of
            # the forward's values to fp32 rounding, whatever the fp32 oracle's own distance is; csrc/sampler.hip)
            assert e_hip <= 2e-6, (name, e_hip, e_orc)      # (measured 7e-9 ... 3e-7; the fp32 oracle 1.5e-6 ... 1.5e-3)

        # stage 2: raw -> (rgb, tau, T) -> samples, one loss through both the image and the sampler
        def raw_grad(dt):
            raw_r = raw.to(dt).clone().requires_grad_(True)
            out = orc.raw2outputs(raw_r, z.to(dt), near.to(dt), far.to(dt), d.to(dt), "linear", "midpoint",
                                  white_bkgd=True)
            # interval indices from the fp32 weights, so every precision inverts the same intervals
            s_ref = orc.sample_pdf_reformulation(z.to(dt), w.to(dt), out[5], out[6], near.to(dt), far.to(dt), N,
                                                 u=u.to(dt))[0]
            ((s_ref * cot.to(dt)).sum() + (out[0] * cot_rgb.to(dt)).sum()).backward()
            return raw_r.grad
        r64, r32 = raw_grad(torch.float64), raw_grad(torch.float32)
        raw_h = g(raw).requires_grad_(True)
        outh = P.raw2outputs(raw_h, g(z), g(near), g(far), g(d), "linear", "midpoint", white_bkgd=True)
        s_hip = Fn.sample_pl(g(z), g(w), outh[5], outh[6], g(near), g(far), g(u), 1e-4, 1e-3)
        ((s_hip * g(cot)).sum() + (outh[0] * g(cot_rgb)).sum()).backward()
        e_hip, e_orc = rel(raw_h.grad, r64), rel(r32, r64)
        print(f"raw grad through sampler + image R={R} S={S}: err vs fp64 oracle: HIP {e_hip:.3e}, fp32 oracle {e_orc:.3e}")
        assert e_hip <= 2 * e_orc + 1e-5, (e_hip, e_orc)


def test_sample_const_backward_vs_oracle_autograd(P):
    """plnerf_sample_const_bwd: d samples / d weights of sample_pdf (through the normalised cdf), which the
    depth-supervised variant needs in piecewise-constant mode (depth_supervised_exps/model/run_nerf_helpers.py:
    343-394), against torch autograd on the oracle's restatement -- fp64 as yardstick, like the PL sampler."""
    from plnerf_amd import functional as Fn

    def rel(a, b):
        return float((a.detach().cpu().double() - b).abs().max()) / (float(b.abs().max()) + 1e-300)

    for (R, B, N, seed) in [(64, 63, 128, 1), (33, 191, 64, 2), (16, 9, 40, 3)]:
        gen = torch.Generator().manual_seed(seed)
        bins = torch.sort(torch.rand(R, B, generator=gen) * 4 + 2, -1)[0]
        w = torch.rand(R, B - 1, generator=gen) ** 3
        w[:, ::7] = 0.0                                   # empty bins: the denom < 1e-5 branch
        u = torch.rand(R, N, generator=gen)
        cot = torch.randn(R, N, generator=gen)

        def oracle(dt):
            wr = w.to(dt).clone().requires_grad_(True)
            s = orc.sample_pdf(bins.to(dt), wr, N, u=u.to(dt))
            (s * cot.to(dt)).sum().backward()
            return wr.grad
        g64, g32 = oracle(torch.float64), oracle(torch.float32)
        wh = g(w).requires_grad_(True)
        s = Fn.sample_const(g(bins), wh, g(u))
        (s * g(cot)).sum().backward()
        e_hip, e_orc = rel(wh.grad, g64), rel(g32, g64)
        print(f"sample_const bwd R={R} B={B} N={N}: err vs fp64 oracle: HIP {e_hip:.3e}, fp32 oracle {e_orc:.3e}")
        assert e_hip <= 2 * e_orc + 1e-5, (e_hip, e_orc)
        # (round 6: the kernel forms pdf and cdf in fp64 from the fp32 weights for the derivative's value -- 1e-7 from fp64 autograd,
        # where the fp32 chain's c1 - c0 leaves up to 1.7e-3 on a narrow bin; csrc/sampler.hip)
        assert e_hip <= 2e-6, (e_hip, e_orc)


@pytest.mark.parametrize("S", [64, 128, 37, 1])
def test_ray_sampling_prologue_bit_exact(P, S):
    """plnerf_stratified_z / plnerf_ray_points against the reference's torch expressions (run_plnerf.py:683-708):
    the same operations in the same order, each rounded once, so the results are bit-identical -- with and without
    the stratified jitter, in depth and in disparity (`lindisp`)."""
    from plnerf_amd import functional as Fn
    R = 777
    gen = torch.Generator().manual_seed(S)
    near = g(0.5 + 2.0 * torch.rand(R, 1, generator=gen))
    far = near + g(0.5 + 5.0 * torch.rand(R, 1, generator=gen))
    rays_o, rays_d = g(torch.randn(R, 3, generator=gen)), g(torch.randn(R, 3, generator=gen))
    t_vals = Fn.cpu_linspace(S, dev())
    t_rand = g(torch.rand(R, S, generator=gen))
    for lindisp in (False, True):
        if not lindisp:
            z_ref = near * (1. - t_vals) + far * t_vals
        else:
            z_ref = 1. / (1. / near * (1. - t_vals) + 1. / far * t_vals)
        z_ref = z_ref.expand([R, S])
        assert torch.equal(Fn.stratified_z(near, far, t_vals, None, lindisp), z_ref)
        mids = .5 * (z_ref[..., 1:] + z_ref[..., :-1])
        upper = torch.cat([mids, z_ref[..., -1:]], -1)
        lower = torch.cat([z_ref[..., :1], mids], -1)
        z_jit = lower + (upper - lower) * t_rand
        z = Fn.stratified_z(near, far, t_vals, t_rand, lindisp)
        assert torch.equal(z, z_jit)
        pts_ref = rays_o[..., None, :] + rays_d[..., None, :] * z_jit[..., :, None]
        assert torch.equal(Fn.ray_points(rays_o, rays_d, z), pts_ref)


def test_merge_sort(P):
    from plnerf_amd import functional as Fn
    for R, S, N in ((513, 64, 128), (64, 128, 64), (3, 1, 1), (7, 500, 524)):
        gen = torch.Generator().manual_seed(S)
        z, _ = torch.sort(2 + 4 * torch.rand(R, S, generator=gen), -1)
        zn = 1.0 + 6 * torch.rand(R, N, generator=gen)           # some outside [near, far] -> clamped
        zn[0, : min(N, 3)] = z[0, 0]                              # ties
        near, far = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
        ref, _ = torch.sort(torch.cat([z, torch.clamp(zn, near, far)], -1), -1)
        out = Fn.merge_sort(g(z), g(zn), g(near), g(far))
        assert torch.equal(out.cpu(), ref), f"merge_sort R={R} S={S} N={N}"
        # near/far as strided views of a ray batch (how render_rays passes them)
        rb = g(torch.cat([torch.zeros(R, 6), near, far, torch.zeros(R, 3)], -1))
        out = Fn.merge_sort(g(z), g(zn), rb[:, 6:7], rb[:, 7:8])
        assert torch.equal(out.cpu(), ref), f"merge_sort (strided bounds) R={R} S={S} N={N}"
    # a general sort, not a merge: unsorted first list, negative values, a NaN (last, as torch.sort puts it), and row
    # lengths that land in every padded size of the register sort (64 / 128 / 256 / 512 / 1024 keys)
    for R, S, N in ((5, 30, 35), (9, 3, 60), (4, 200, 100), (6, 100, 28), (3, 700, 100)):
        gen = torch.Generator().manual_seed(S + N)
        z = 8 * torch.rand(R, S, generator=gen) - 4
        zn = 8 * torch.rand(R, N, generator=gen) - 4
        z[0, 0] = float("nan")
        near, far = torch.full((R, 1), -3.0), torch.full((R, 1), 3.0)
        ref, _ = torch.sort(torch.cat([z, torch.clamp(zn, near, far)], -1), -1)
        out = Fn.merge_sort(g(z), g(zn), g(near), g(far)).cpu()
        assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.equal(torch.nan_to_num(out, nan=9.0),
                                                                           torch.nan_to_num(ref, nan=9.0)), (R, S, N)


# ----------------------------------------------------------------------------- MLP
def test_mlp_fwd_golden(P, golden):
    gd = golden("g1_mlp")
    pts, vd = g(T(gd["pts"])), g(T(gd["viewdirs"]))
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    for tag, sharp in (("plain", False), ("sharp", True)):
        net = make_net(P, orc.closed_form_state_dict(0, sharp))
        with torch.no_grad():
            raw = P.run_network(pts, vd, net, emb_fn, embd_fn)
            raw_emb = net(g(T(gd["embedded"])))
        scale = float(np.abs(gd[f"raw_{tag}"]).max())
        print(f"g1 {tag}: max|raw|={scale:.3f} max err fused={maxdiff(raw, T(gd[f'raw_{tag}'])):.3e} "
              f"embedded={maxdiff(raw_emb, T(gd[f'raw_from_embedded_{tag}'])):.3e}")
        assert_close(raw, gd[f"raw_{tag}"], what=f"g1 fused {tag}")
        assert_close(raw_emb, gd[f"raw_from_embedded_{tag}"], what=f"g1 embedded {tag}")
    # the generic (torch-op) encoder equals the reference's encoding bit for bit on CPU, closely on GPU
    assert_close(torch.cat([emb_fn(pts.reshape(-1, 3)),
                            embd_fn(vd[:, None].expand(pts.shape).reshape(-1, 3))], -1), gd["embedded"],
                 atol=2e-6, rtol=2e-6, what="Embedder")


@pytest.mark.parametrize("R,S", [(5, 64), (3, 37), (16, 192)])
def test_mlp_fwd_bwd_vs_oracle(P, R, S):
    """Forward and all 24 parameter gradients against autograd on the oracle, including a
    row count that is not a multiple of the 64-row tile."""
    gen = torch.Generator().manual_seed(R * 1000 + S)
    pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 2.5
    vd = torch.randn(R, 3, generator=gen)
    vd = vd / vd.norm(dim=-1, keepdim=True)
    cot = torch.randn(R, S, 4, generator=gen)
    sd = orc.closed_form_state_dict(3, False)
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    raw_o = orc.query_network(sd_o, pts, vd)
    (raw_o * cot).sum().backward()
    net = make_net(P, sd)
    raw_h = net.query(g(pts), g(vd))
    assert_close(raw_h, raw_o, what="mlp fwd")
    (raw_h * g(cot)).sum().backward()
    for name, prm in net.named_parameters():
        ref = sd_o[name].grad
        scale = float(ref.abs().max())
        err = maxdiff(prm.grad, ref)
        assert err <= 2e-5 * max(scale, 1e-3) + 1e-7, f"grad {name}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_c_host_without_torch(P, precision, tmp_path):
    """The drop-in boundary is the C ABI, not the Python mirror: tests/c_abi_gpu.cpp -- a host that knows only
    include/plnerf_hip.h and the HIP runtime (g++, no torch, no Python) -- packs the weights, runs the network, the
    piecewise-linear quadrature, both backwards and one Adam step on device memory it allocated itself; its outputs are
    compared with the oracle (forward 1e-5; gradients at the bounds of test_mlp_fwd_bwd_vs_oracle / test_mlp_bf16_modes) and
    with the Python mirror's on the same inputs (the same kernels: bit for bit)."""
    import c_hosts
    exe = c_hosts.build("c_abi_gpu", tmp_path)
    R, S = 37, 50                                  # (1850 rows: ragged against every tile size)
    gen = torch.Generator().manual_seed(4242)
    pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 2.5
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    z, _ = torch.sort(2.0 + 4.0 * torch.rand(R, S, generator=gen), -1)
    near, far = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    d = torch.randn(R, 3, generator=gen)
    g_rgb, g_depth, g_acc = torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen)
    sd = orc.closed_form_state_dict(3, True)
    names = [n for n, _ in orc.param_shapes()]
    with open(tmp_path / "in.bin", "wb") as f:
        for t in [sd[n] for n in names] + [pts, vd, z, near, far, d, g_rgb, g_depth, g_acc]:
            f.write(t.contiguous().float().numpy().tobytes())
    prec = {"fp32": 0, "f16x3": 3}[precision]      # PLNERF_PREC_*
    from plnerf_amd import _lib as L_
    run = c_hosts.run(exe, prec, R, S, tmp_path / "in.bin", tmp_path / "out.bin", L_.FWD_KERNEL)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = np.fromfile(tmp_path / "out.bin", dtype=np.float32)
    pos = [0]

    def take(*shape):
        n = int(np.prod(shape))
        a = torch.from_numpy(out[pos[0]:pos[0] + n].copy()).reshape(*shape)
        pos[0] += n
        return a
    raw, rgb, disp, acc, depth, w, g_raw = (take(R, S, 4), take(R, 3), take(R), take(R), take(R), take(R, S + 1),
                                            take(R, S, 4))
    grads = {n: take(*shp) for n, shp in orc.param_shapes()}
    w0_after = take(*dict(orc.param_shapes())[names[0]])
    assert pos[0] == out.size
    # the oracle on the same inputs
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    raw_o = orc.query_network(sd_o, pts, vd)
    ro = orc.raw2outputs(raw_o, z, near, far, d, "linear", "midpoint", white_bkgd=True)
    ((ro[0] * g_rgb).sum() + (ro[4] * g_depth).sum() + (ro[2] * g_acc).sum()).backward()
    assert_close(raw, raw_o, what="C host: raw")
    for name, a, b in (("rgb", rgb, ro[0]), ("disp", disp, ro[1]), ("acc", acc, ro[2]), ("weights", w, ro[3]), ("depth", depth, ro[4])):
        assert_close(a, b, what=f"C host: {name}")
    gtol = 2e-5 if precision == "fp32" else 1.5e-3
    for n in names:
        ref = sd_o[n].grad
        err, scale = maxdiff(grads[n], ref), float(ref.abs().max())
        assert err <= gtol * max(scale, 1e-3) + 1e-7, f"C host: grad {n}: {err:.3e} vs scale {scale:.3e}"
    # Adam, step 1 from zero moments: the parameter moves by lr * g / (|g| + eps (1 - beta2)^0.5 ...) -- torch's own step
    p0 = sd[names[0]].clone().requires_grad_(True)
    p0.grad = grads[names[0]].clone()
    torch.optim.Adam([p0], lr=5e-4, betas=(0.9, 0.999), eps=1e-8).step()
    assert float((w0_after - p0.detach()).abs().max()) <= 1e-7
    # the Python mirror drives the same kernels: bit for bit
    from plnerf_amd.functional import QuadratureFn
    net = make_net(P, sd, precision)
    raw_h = net.query(g(pts), g(vd))
    rh = QuadratureFn.apply(raw_h, g(z), g(near), g(far), g(d), None, "linear", "midpoint", True, False)
    ((rh[0] * g(g_rgb)).sum() + (rh[4] * g(g_depth)).sum() + (rh[2] * g(g_acc)).sum()).backward()
    assert torch.equal(raw_h.detach().cpu(), raw) and torch.equal(rh[0].detach().cpu(), rgb)
    for n, prm in net.named_parameters():
        assert torch.equal(prm.grad.cpu(), grads[n]), n


@pytest.mark.parametrize("precision,fwd_tol,grad_tol", [("bf16x3", 1e-5, 1.5e-3), ("f16x3", 2e-6, 1.5e-3), ("bf16", 5e-3, 5e-2),
                                                        ("f16", 1e-3, 5e-2)])
def test_mlp_bf16_modes(P, golden, precision, fwd_tol, grad_tol):
    """The bf16-MFMA modes: bf16x3 (3-term split) must hold the 1e-5 forward bound on the golden
    vectors (G1) like fp32 does; plain bf16 is the throughput mode and is only held to 5e-3."""
    gd = golden("g1_mlp")
    pts, vd = g(T(gd["pts"])), g(T(gd["viewdirs"]))
    for tag, sharp in (("plain", False), ("sharp", True)):
        net = make_net(P, orc.closed_form_state_dict(0, sharp), precision)
        with torch.no_grad():
            raw = net.query(pts, vd)
            raw_emb = net(g(T(gd["embedded"])))
        e1, e2 = maxdiff(raw, T(gd[f"raw_{tag}"])), maxdiff(raw_emb, T(gd[f"raw_from_embedded_{tag}"]))
        print(f"{precision} g1 {tag}: max err fused={e1:.3e} embedded={e2:.3e}")
        assert e1 <= fwd_tol and e2 <= fwd_tol
    # forward + all 24 gradients, two tile shapes (incl. a ragged tail).  ReLU makes the gradient
    # discontinuous: a pre-activation within the forward's rounding error of zero can flip its mask
    # and move a gradient entry by O(1e-2).  So the cotangent is zeroed on samples that have any
    # pre-activation within `amb` of zero in an fp64 evaluation -- on the remaining samples every mode
    # takes the same ReLU branches as the oracle and the comparison is sharp.
    #
    # The 16-bit modes keep the saved activations and the (scaled) pre-activation gradients as IEEE half
    # planes (11-bit mantissa) for the weight-gradient contraction: an unbiased 2^-12 rounding per element.
    # With the random-sign cotangent used here every gradient entry is itself a random walk over the samples,
    # so signal and rounding noise both grow as sqrt(n) and the relative error stays at a few 2^-12 whatever
    # the batch (observed 5e-4 ... 8.4e-4 from 320 to 18,432 samples); on a coherent training gradient it
    # averages down (G6: unchanged at 1.2e-4 ... 3.2e-4).  Bound for the split modes: 1.5e-3 of max|g|.
    amb = {"bf16x3": 5e-5, "f16x3": 5e-6}.get(precision, 0.0)     # plain 16-bit operands: no sharp comparison possible
    for R, S in ((5, 64), (7, 101), (96, 192)):
        gen = torch.Generator().manual_seed(R * 100 + S)
        ptsr = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 2.5
        vdr = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
        cot = torch.randn(R, S, 4, generator=gen)
        sd = orc.closed_form_state_dict(3, False)
        keep = ~ambiguous_rows(sd, ptsr, vdr, amb)
        cot = cot * keep.reshape(R, S, 1)
        sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        raw_o = orc.query_network(sd_o, ptsr, vdr)
        (raw_o * cot).sum().backward()
        net = make_net(P, sd, precision)
        raw_h = net.query(g(ptsr), g(vdr))
        assert maxdiff(raw_h, raw_o) <= fwd_tol, f"{precision} fwd R={R} S={S}: {maxdiff(raw_h, raw_o):.3e}"
        (raw_h * g(cot)).sum().backward()
        worst, worst_cos = 0.0, 1.0
        for name, prm in net.named_parameters():
            ref = sd_o[name].grad
            worst = max(worst, maxdiff(prm.grad, ref) / max(float(ref.abs().max()), 1e-3))
            worst_cos = min(worst_cos, float(torch.nn.functional.cosine_similarity(
                prm.grad.detach().cpu().reshape(1, -1).double(), ref.reshape(1, -1).double())))
        print(f"{precision} R={R} S={S}: {int(keep.sum())}/{keep.numel()} unambiguous samples, "
              f"fwd err {maxdiff(raw_h, raw_o):.3e}, worst grad err/max|g| {worst:.3e}, worst cosine {worst_cos:.8f}")
        if precision in ("bf16x3", "f16x3"):
            assert worst <= grad_tol and worst_cos >= 0.999999, (worst, worst_cos)
        else:   # bf16 flips ReLU branches near zero: hold direction, not entries
            assert worst_cos >= 0.99


def test_render_rays_golden_bf16x3(P, golden):
    """End-to-end render on the golden rays in bf16x3 mode (reported; rgb asserted at 1e-4)."""
    gd = golden("g5_render_rays")
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    for c in (0, 1):
        p = f"c{c}_"
        o, d, near, far = g5_batch(gd, p)
        net_c = make_net(P, orc.closed_form_state_dict(0, True), "bf16x3")
        net_f = make_net(P, orc.closed_form_state_dict(1, True), "bf16x3")
        qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
        kw = dict(network_query_fn=qfn, perturb=1.0, N_importance=int(gd[p + "N_importance"]), network_fine=net_f,
                  N_samples=int(gd[p + "N_samples"]), network_fn=net_c, white_bkgd=True, raw_noise_std=0.0,
                  mode="linear", color_mode="midpoint")
        K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
        with torch.no_grad():
            rgb, disp, acc, extras = P.render(800, 800, K, chunk=32768, rays=(g(o), g(d)), ndc=False, near=near,
                                              far=far, use_viewdirs=True, retraw=True, pytest=True, **kw)
        print(f"bf16x3 g5 case {c}: rgb0 err {maxdiff(extras['rgb0'], T(gd[p + 'rgb0'])):.3e}, "
              f"rgb err {maxdiff(rgb, T(gd[p + 'rgb_map'])):.3e}, depth err {maxdiff(extras['depth_map'], T(gd[p + 'depth_map'])):.3e}")
        assert_close(extras["rgb0"], gd[p + "rgb0"], atol=2e-5, rtol=2e-5, what="bf16x3 rgb0")
        assert_close(rgb, gd[p + "rgb_map"], atol=1e-4, rtol=1e-4, what="bf16x3 rgb_map")


def test_mlp_embedded_path_grads(P):
    gen = torch.Generator().manual_seed(17)
    N = 100
    emb = torch.randn(N, 90, generator=gen)
    cot = torch.randn(N, 4, generator=gen)
    sd = orc.closed_form_state_dict(5, False)
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    (orc.nerf_mlp(sd_o, emb) * cot).sum().backward()
    net = make_net(P, sd)
    out = net(g(emb))
    assert_close(out, orc.nerf_mlp(sd, emb), what="embedded fwd")
    (out * g(cot)).sum().backward()
    for name, prm in net.named_parameters():
        ref = sd_o[name].grad
        scale = float(ref.abs().max())
        assert maxdiff(prm.grad, ref) <= 2e-5 * max(scale, 1e-3) + 1e-7, f"grad {name}"


def test_unsupported_and_cpu_fail_loudly(P):
    """The FUSED entries refuse a shape outside the compiled trunk (query: the in-kernel encoding; packed_weights) -- since
    round 6 NeRF.forward serves it layer by layer instead (generic.py; tests/test_gpu_modes.py) -- a shape the reference's own
    forward cannot run raises, and nothing falls back to the CPU."""
    for kw in (dict(D=8, W=128, skips=[2]), dict(D=8, W=512)):      # five layers behind a skip; wider than the trunk
        net = P.NeRF(input_ch=63, input_ch_views=27, use_viewdirs=True, **kw).to(dev())
        with pytest.raises(NotImplementedError):
            net.query(g(torch.zeros(2, 3, 3)), g(torch.zeros(2, 3)))
        with pytest.raises(NotImplementedError):
            net.packed_weights()
        assert net(g(torch.zeros(2, 90))).shape == (2, 4)            # (the layer-by-layer route)
    with pytest.raises(RuntimeError, match="input features"):      # a skip after the LAST trunk layer, as F.linear would
        P.NeRF(D=5, W=64, input_ch=63, input_ch_views=27, skips=[4], use_viewdirs=True).to(dev())(g(torch.zeros(2, 90)))
    net = P.NeRF(input_ch=63, input_ch_views=27, use_viewdirs=True)     # left on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(2, 90))


# ----------------------------------------------------------------------------- render_rays
def test_render_rays_golden(P, golden):
    """render() end to end on the reference's deterministic (pytest=True) draws.  The sampler is
    discontinuous, so end-to-end agreement is asserted at 1e-4 on the maps, and the
    count of rays beyond 1e-5 is reported; per-stage 1e-5 parity is asserted by the tests above."""
    gd = golden("g5_render_rays")
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    for c in range(int(gd["n_cases"])):
        p = f"c{c}_"
        o, d, near, far = g5_batch(gd, p)
        net_c = make_net(P, orc.closed_form_state_dict(0, True))
        net_f = make_net(P, orc.closed_form_state_dict(1, True))
        qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
        kw = dict(network_query_fn=qfn, perturb=1.0, N_importance=int(gd[p + "N_importance"]), network_fine=net_f,
                  N_samples=int(gd[p + "N_samples"]), network_fn=net_c, white_bkgd=bool(gd[p + "white_bkgd"]),
                  raw_noise_std=float(gd[p + "raw_noise_std"]), mode=str(gd[p + "mode"]), color_mode="midpoint")
        ndc = bool(gd[p + "ndc"])
        f = float(gd[p + "focal"])
        H, W = int(gd[p + "H"]), int(gd[p + "W"])
        K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
        with torch.no_grad():
            rgb, disp, acc, extras = P.render(H, W, K, chunk=32768, rays=(g(o), g(d)), ndc=ndc, near=near, far=far,
                                              use_viewdirs=True, retraw=True, pytest=True, **kw)
        got = dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc)
        assert set(got) == {"rgb_map", "disp_map", "acc_map", "depth_map", "raw", "rgb0", "disp0", "depth0", "acc0",
                            "z_std"}
        for k in ("rgb0", "acc0", "depth0", "disp0"):       # coarse pass: continuous, strict
            assert_close(got[k], gd[p + k], what=f"g5 case {c} {k}")
        for k in ("rgb_map", "acc_map", "depth_map", "z_std"):
            err = maxdiff(got[k], T(gd[p + k]))
            print(f"g5 case {c} {k}: max err {err:.3e}")
            assert_close(got[k], gd[p + k], what=f"g5 case {c} {k}")      # 1e-5: the contract, end to end


def test_render_rays_vs_oracle_shared_randomness(P):
    """Same rays, same t_rand/u on both sides, 64+128 linear: all outputs."""
    R, Ns, Ni = 96, 64, 128
    batch, _ = orc.synthetic_blender_rays(R, seed=3)
    t_rand = torch.rand(R, Ns, generator=torch.Generator().manual_seed(1))
    sd_c, sd_f = orc.closed_form_state_dict(0, True), orc.closed_form_state_dict(1, True)
    # oracle draws with numpy seed 0 under pytest=True: reproduce the same on both sides
    ref = orc.render_rays(batch, sd_c, sd_f, Ns, "linear", "midpoint", retraw=True, perturb=1.0, N_importance=Ni,
                          white_bkgd=True, pytest=True)
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    with torch.no_grad():
        got = P.render_rays(g(batch), make_net(P, sd_c), qfn, Ns, "linear", "midpoint", retraw=True, perturb=1.0,
                            N_importance=Ni, network_fine=make_net(P, sd_f), white_bkgd=True, pytest=True)
    for k in ("rgb0", "acc0", "depth0"):
        assert_close(got[k], ref[k], what=k)
    bad = ((got["rgb_map"].cpu() - ref["rgb_map"]).abs() > 1e-5).any(-1).sum()
    print(f"render_rays: rgb_map max err {maxdiff(got['rgb_map'], ref['rgb_map']):.3e}, rays beyond 1e-5: {int(bad)}/{R}")
    assert int(bad) == 0
    assert_close(got["rgb_map"], ref["rgb_map"], what="rgb_map")


# ----------------------------------------------------------------------------- training step
def test_train_step_golden_and_oracle(P, golden):
    """One optimisation step (run_plnerf.py:1283-1316) through create_nerf/render/backward/Adam:
    loss, sampled gradients and parameters against the reference's own step (G6)."""
    import tempfile, os
    from argparse import Namespace
    gd = golden("g6_train_step")
    stride = int(gd["sample_stride"])
    for c in range(int(gd["n_cases"])):
        p = f"c{c}_"
        d = tempfile.mkdtemp()
        os.makedirs(os.path.join(d, "exp"))
        args = Namespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4,
                         N_importance=int(gd[p + "N_importance"]), N_samples=int(gd[p + "N_samples"]), netdepth=8,
                         netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4,
                         coarse_lrate=5e-4, ft_path=None, ckpt_dir=d, expname="exp", no_reload=True, perturb=1.0,
                         white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint",
                         dataset="blender", no_ndc=False, lindisp=False)
        kw, _, _, grad_vars, opt, opt_c = P.create_nerf(args, device=dev())
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
        worst = 0.0
        for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
            for name, prm in net.named_parameters():
                ref = T(gd[p + f"grad_{tag}_{name}_sample"])
                got = prm.grad.reshape(-1)[::stride].cpu()
                ref_norm = float(gd[p + f"grad_{tag}_{name}_norm"])
                err = float((got - ref).abs().max())
                worst = max(worst, err / max(ref_norm, 1e-12))
                # coarse-net gradients are continuous in the inputs; fine-net ones see the re-sorted samples
                tol = (2e-4 if tag == "coarse" else 2e-3) * max(float(ref.abs().max()), 1e-6) + 1e-8
                assert err <= tol, f"{tag} {name}: grad err {err:.3e} (tol {tol:.3e})"
                assert abs(float(prm.grad.norm()) - ref_norm) <= 2e-3 * ref_norm + 1e-9
        print(f"g6 case {c}: loss {float(loss.detach()):.6f}, worst grad err / |grad| = {worst:.3e}")
        opt.step()
        opt_c.step()
        for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
            for name, prm in net.named_parameters():
                ref = T(gd[p + f"param_{tag}_{name}_sample"])
                # Adam's first step moves every weight by ~lr regardless of gradient scale; a sign flip
                # of a near-zero gradient shows up as 2*lr, so bound by 2.5*lr
                assert float((prm.detach().reshape(-1)[::stride].cpu() - ref).abs().max()) <= 1.25e-3


# ----------------------------------------------------------------------------- depth-supervised variant (8f-1)
def test_depth_variant_network_golden(P, golden):
    """57 | 3 input channels, pi-scaled encoder, softplus density (depth_supervised_exps/model/
    run_nerf_helpers.py:100-205) through the same fused MLP, against the reference's own outputs (G8);
    also the non-default widths' weight gradients against the oracle."""
    gd = golden("g8_depth_variant")
    Dp, kw, _, _ = depth_setup(gd)
    pts, vd = g(T(gd["mlp_pts"])), g(T(gd["mlp_viewdirs"]))
    with torch.no_grad():
        raw = kw["network_query_fn"](pts, vd, kw["embedded_cam"], kw["network_fn"])
    assert_close(raw, gd["mlp_raw"], what="g8 network output")
    for prec, tol in (("f16x3", 1e-5), ("bf16x3", 2e-5)):
        Dp2, kw2, _, _ = depth_setup(gd, prec)
        with torch.no_grad():
            raw2 = kw2["network_query_fn"](pts, vd, kw2["embedded_cam"], kw2["network_fn"])
        err = maxdiff(raw2, T(gd["mlp_raw"]))
        print(f"g8 network {prec}: max err {err:.3e}")
        assert err <= tol * (1 + float(T(gd["mlp_raw"]).abs().max()))
    # gradients of the 57- and 3-wide weight blocks (fp32 path) vs oracle autograd
    net = kw["network_fn"]
    emb = g(T(gd["mlp_embedded"]))
    cot = torch.randn(emb.shape[0], 4, generator=torch.Generator().manual_seed(1))
    out = net(emb)
    (out * g(cot)).sum().backward()
    sd = {k: v.clone().requires_grad_(True) for k, v in orc.closed_form_state_dict_depth(0, True).items()}
    (orc.nerf_mlp_depth(sd, T(gd["mlp_embedded"])) * cot).sum().backward()
    for name, prm in net.named_parameters():
        ref = sd[name].grad
        err = float((prm.grad.cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
        assert err <= 1e-4, (name, err)
    # the same through the half backward of the 16-bit modes (57 | 3 wide weight-gradient blocks included)
    Dp3, kw3, _, _ = depth_setup(gd, "f16x3")
    net3 = kw3["network_fn"]
    (net3(emb) * g(cot)).sum().backward()
    worst = 0.0
    for name, prm in net3.named_parameters():
        ref = sd[name].grad
        assert prm.grad.shape == ref.shape
        worst = max(worst, float((prm.grad.cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30))
    print(f"g8 network f16x3 gradients: worst err / max|g| = {worst:.3e}")
    assert worst <= 3e-3, worst


def test_depth_variant_render_and_train_step_golden(P, golden):
    """render_rays of the depth-supervised variant (pred_hyp attached) and one training step
    (run_nerf_sample_based_depth.py:792-958, 1126-1157) against the reference (G8)."""
    gd = golden("g8_depth_variant")
    stride = int(gd["sample_stride"])
    Dp, kw, grad_vars, opt = depth_setup(gd)
    batch, target, target_h = g(T(gd["ray_batch"])), g(T(gd["target"])), g(T(gd["target_h"]))
    args = depth_args_of(gd)
    step = Dp.DepthTrainStep(args, kw, opt, grad_vars, distributed=False)
    # forward only first: every output of the dict
    with torch.no_grad():
        ret = Dp.render_rays(batch, retraw=True, pytest=True, **{k: v for k, v in kw.items()})
    assert set(ret) == {"rgb_map", "disp_map", "acc_map", "depth_map", "z_vals", "weights", "pred_hyp", "u", "raw",
                        "rgb0", "disp0", "acc0", "depth0", "z_vals0", "weights0", "z_std"}
    assert torch.equal(ret["u"].cpu(), T(gd["render_u"]))
    for k in ("rgb0", "acc0", "depth0", "disp0", "z_vals0", "weights0"):      # coarse pass: continuous, strict
        assert_close(ret[k], gd["render_" + k], what=f"g8 {k}")
    for k in ("rgb_map", "acc_map", "depth_map", "z_vals", "pred_hyp", "z_std"):
        err = maxdiff(ret[k], T(gd["render_" + k]))
        print(f"g8 {k}: max err {err:.3e}")
        assert_close(ret[k], gd["render_" + k], atol=1e-4, rtol=1e-4, what=f"g8 {k}")
    loss, img_loss, sc, _ = step(batch, target, target_h, pytest=True)
    assert abs(float(loss) - float(gd["loss"])) <= 1e-5, (float(loss), float(gd["loss"]))
    assert abs(float(sc) - float(gd["space_carving_loss"])) <= 1e-4, (float(sc), float(gd["space_carving_loss"]))
    # parameters after the clipped Adam step (first step: every weight moves by ~lr, sign flips of tiny
    # gradients show as 2*lr)
    for net, tag in ((kw["network_fn"], "coarse"), (kw["network_fine"], "fine")):
        for name, prm in net.named_parameters():
            ref = T(gd[f"param_{tag}_{name}_sample"])
            assert float((prm.detach().reshape(-1)[::stride].cpu() - ref).abs().max()) <= 1.25e-3, (tag, name)


def test_depth_variant_gradients_vs_oracle(P):
    """Gradients of the full depth-supervised loss (image + space carving through pred_hyp + coarse image) with
    respect to both networks, HIP vs oracle on shared draws, before clipping.

    The loss runs through the ill-conditioned closed form of the sampler (see
    test_sampler_backward_vs_oracle_autograd): the fp32 oracle's own gradients sit ~1e-2 of max|g| away from
    its fp64 gradients on the fine network.  Yardstick = fp64 oracle; bound = twice the fp32 oracle's own
    distance from it (+5e-4), per network, plus a cosine check on the whole gradient."""
    import sys
    from plnerf_amd import depth as Dp
    R, Ns, Ni = 48, 32, 48
    gdummy = {"N_importance": Ni, "N_samples": Ns, "space_carving_weight": 0.05}
    Dp, kw, grad_vars, opt = depth_setup(gdummy)
    batch, target = orc.synthetic_blender_rays(R, seed=11)
    gen = torch.Generator().manual_seed(11)
    t_rand, u_fine, u_hyp = torch.rand(R, Ns, generator=gen), torch.rand(R, Ni, generator=gen) * 0.999, \
        torch.rand(R, Ni, generator=gen) * 0.999
    target_h = 2.0 + 4.0 * torch.rand(3, R, 1, generator=gen)

    def oracle(dt):
        sd_c = {k: v.to(dt) for k, v in orc.closed_form_state_dict_depth(0, True).items()}
        sd_f = {k: v.to(dt) for k, v in orc.closed_form_state_dict_depth(1, True).items()}
        okw = dict(N_samples=Ns, N_importance=Ni, mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True,
                   t_rand=t_rand.to(dt), u_fine=u_fine.to(dt), cached_u=u_hyp.to(dt))
        return orc.depth_train_step(sd_c, sd_f, batch.to(dt), target.to(dt), target_h.to(dt), okw,
                                    space_carving_weight=0.05)
    loss_o, sc_o, g_c32, g_f32 = oracle(torch.float32)
    _, _, g_c64, g_f64 = oracle(torch.float64)
    # HIP: same draws injected by patching the two draw helpers for this call
    dmod = sys.modules[Dp.__name__]
    rmod = sys.modules[Dp.__name__.rsplit(".", 1)[0] + ".render"]   # (the package attribute `render` is the function)
    orig_jitter, orig_draw = dmod._draw_t_rand, rmod._draw_u
    try:
        dmod._draw_t_rand = lambda *a, **k: g(t_rand)      # (the stratified jitter, whichever prologue consumes it)
        rmod._draw_u = lambda *a, **k: g(u_fine)
        ret = Dp.render_rays(g(batch), retraw=True, cached_u=g(u_hyp), **kw)
    finally:
        dmod._draw_t_rand, rmod._draw_u = orig_jitter, orig_draw
    sc = Dp.compute_space_carving_loss(ret["pred_hyp"], g(target_h))
    loss = P.img2mse(ret["rgb_map"], g(target)) + 0.05 * sc + P.img2mse(ret["rgb0"], g(target))
    loss.backward()
    print(f"depth loss HIP {float(loss.detach()):.6f} oracle {float(loss_o):.6f}; space carving "
          f"{float(sc.detach()):.5f} / {float(sc_o):.5f}")
    assert abs(float(loss.detach()) - float(loss_o)) <= 2e-5 and abs(float(sc.detach()) - float(sc_o)) <= 2e-4

    def rel(a, b):
        return float((a.double() - b).abs().max()) / (float(b.abs().max()) + 1e-300)
    for net, g32, g64, tag in ((kw["network_fn"], g_c32, g_c64, "coarse"), (kw["network_fine"], g_f32, g_f64, "fine")):
        e_hip = max(rel(prm.grad.cpu(), g64[name]) for name, prm in net.named_parameters())
        e_orc = max(rel(g32[name], g64[name]) for name in g64)
        flat_h = torch.cat([prm.grad.cpu().double().reshape(-1) for _, prm in net.named_parameters()])
        flat_o = torch.cat([g64[name].reshape(-1) for name, _ in net.named_parameters()])
        cos = float(torch.dot(flat_h, flat_o) / (flat_h.norm() * flat_o.norm()))
        print(f"depth variant {tag} gradients vs fp64 oracle: HIP {e_hip:.3e}, fp32 oracle {e_orc:.3e}, cosine {cos:.7f}")
        assert e_hip <= 2 * e_orc + 5e-4, (tag, e_hip, e_orc)
        assert cos >= 0.9999, (tag, cos)


def test_depth_variant_constant_mode_vs_oracle(P):
    """The depth-supervised step in piecewise-constant mode (the depth script's argparse default): pred_hyp from
    sample_pdf_return_u with gradients through plnerf_sample_const_bwd and the constant-mode quadrature, against
    the oracle on shared draws (fp64 yardstick as in the linear-mode test).  Default-initialised (not
    "sharpened") networks: with saturated rays most bins are empty, sample_pdf divides by cdf steps of ~1e-5, and
    the fp32 gradient -- the reference's own included -- is cancellation noise (cosine 0.89 against fp64 for both
    the oracle and this path)."""
    import sys
    from plnerf_amd import depth as Dp
    R, Ns, Ni = 40, 32, 48
    gdummy = {"N_importance": Ni, "N_samples": Ns, "space_carving_weight": 0.05}
    Dp, kw, grad_vars, opt = depth_setup(gdummy)
    kw = dict(kw, mode="constant")
    kw["network_fn"].load_state_dict(orc.closed_form_state_dict_depth(0, False))
    kw["network_fine"].load_state_dict(orc.closed_form_state_dict_depth(1, False))
    batch, target = orc.synthetic_blender_rays(R, seed=12)
    gen = torch.Generator().manual_seed(12)
    t_rand, u_fine, u_hyp = torch.rand(R, Ns, generator=gen), torch.rand(R, Ni, generator=gen), \
        torch.rand(R, Ni, generator=gen)
    target_h = 2.0 + 4.0 * torch.rand(3, R, 1, generator=gen)

    def oracle(dt):
        sd_c = {k: v.to(dt) for k, v in orc.closed_form_state_dict_depth(0, False).items()}
        sd_f = {k: v.to(dt) for k, v in orc.closed_form_state_dict_depth(1, False).items()}
        okw = dict(N_samples=Ns, N_importance=Ni, mode="constant", color_mode="midpoint", perturb=1.0, white_bkgd=True,
                   t_rand=t_rand.to(dt), u_fine=u_fine.to(dt), cached_u=u_hyp.to(dt))
        return orc.depth_train_step(sd_c, sd_f, batch.to(dt), target.to(dt), target_h.to(dt), okw,
                                    space_carving_weight=0.05)
    loss_o, sc_o, g_c32, g_f32 = oracle(torch.float32)
    _, _, g_c64, g_f64 = oracle(torch.float64)
    dmod = sys.modules[Dp.__name__]
    rmod = sys.modules[Dp.__name__.rsplit(".", 1)[0] + ".render"]
    orig_jitter, orig_draw = dmod._draw_t_rand, rmod._draw_u
    try:
        dmod._draw_t_rand = lambda *a, **k: g(t_rand)      # (the stratified jitter, whichever prologue consumes it)
        rmod._draw_u = lambda *a, **k: g(u_fine)
        ret = Dp.render_rays(g(batch), retraw=True, cached_u=g(u_hyp), **kw)
    finally:
        dmod._draw_t_rand, rmod._draw_u = orig_jitter, orig_draw
    assert ret["pred_hyp"].requires_grad and ret["weights"].shape == (R, Ns + Ni)
    sc = Dp.compute_space_carving_loss(ret["pred_hyp"], g(target_h))
    loss = P.img2mse(ret["rgb_map"], g(target)) + 0.05 * sc + P.img2mse(ret["rgb0"], g(target))
    loss.backward()
    print(f"constant-mode depth loss HIP {float(loss.detach()):.6f} oracle {float(loss_o):.6f}; space carving "
          f"{float(sc.detach()):.5f} / {float(sc_o):.5f}")
    assert abs(float(loss.detach()) - float(loss_o)) <= 2e-5 and abs(float(sc.detach()) - float(sc_o)) <= 2e-4

    def rel(a, b):
        return float((a.double() - b).abs().max()) / (float(b.abs().max()) + 1e-300)
    for net, g32, g64, tag in ((kw["network_fn"], g_c32, g_c64, "coarse"), (kw["network_fine"], g_f32, g_f64, "fine")):
        e_hip = max(rel(prm.grad.cpu(), g64[name]) for name, prm in net.named_parameters())
        e_orc = max(rel(g32[name], g64[name]) for name in g64)
        flat_h = torch.cat([prm.grad.cpu().double().reshape(-1) for _, prm in net.named_parameters()])
        flat_o = torch.cat([g64[name].reshape(-1) for name, _ in net.named_parameters()])
        cos = float(torch.dot(flat_h, flat_o) / (flat_h.norm() * flat_o.norm()))
        print(f"constant-mode {tag} gradients vs fp64 oracle: HIP {e_hip:.3e}, fp32 oracle {e_orc:.3e}, cosine {cos:.7f}")
        assert e_hip <= 2 * e_orc + 5e-4, (tag, e_hip, e_orc)
        assert cos >= 0.9999, (tag, cos)


def test_depth_variant_render_wrappers(P, golden):
    """depth.render / render_hyp (run_nerf_sample_based_depth.py:85-248): ray packing from c2w or from a ray batch,
    chunking, the 5.33:9 crop, reshape of every dict entry -- equal to render_rays on the packed batch."""
    gd = golden("g8_depth_variant")
    Dp, kw, _, _ = depth_setup(gd)
    kw = dict(kw, perturb=0.0)                    # deterministic draws: chunking must not change anything
    H, W = 6, 16
    intr = torch.tensor([14.0, 14.0, W / 2, H / 2], device=dev())
    c2w = P.rays.pose_spherical(20.0, -30.0, 4.0)[:3, :4].to(dev())
    with torch.no_grad():
        rgb, disp, acc, extras = Dp.render(H, W, intr, chunk=40, c2w=c2w, near=2.0, far=6.0, **kw)
        assert rgb.shape == (H, W, 3) and extras["pred_hyp"].shape == (H, W, int(gd["N_importance"]))
        ro, rd = Dp.get_rays(H, W, intr, c2w)
        vd = rd / rd.norm(dim=-1, keepdim=True)
        packed = torch.cat([ro, rd, torch.full_like(rd[..., :1], 2.0), torch.full_like(rd[..., :1], 6.0), vd], -1)
        ref = Dp.render_rays(packed.reshape(-1, 11), **kw)
        assert torch.equal(rgb.reshape(-1, 3), ref["rgb_map"]) and torch.equal(extras["pred_hyp"].reshape(H * W, -1), ref["pred_hyp"])
        rgb2 = Dp.render_hyp(H, W, intr, chunk=1 << 20, rays=torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)]), near=2.0,
                             far=6.0, **kw)[0]
        assert torch.equal(rgb2, ref["rgb_map"])
        crop = Dp.render(H, W, intr, c2w=c2w, near=2.0, far=6.0, with_5_9=True, **kw)[0]
        Wc = int(H / 9. * 16. / 3.); Wc -= Wc % 2
        s0 = (W - Wc) // 2
        assert crop.shape == (H, Wc, 3) and torch.equal(crop, rgb[:, s0:s0 + Wc])


def test_single_pass_variants_vs_oracle(P):
    """N_importance = 0: render_rays returns the coarse pass only (run_plnerf.py:714, 744); the depth-supervised
    variant then draws pred_hyp from the coarse weights with N_samples draws (run_nerf_sample_based_depth.py:
    872-886).  Both against the oracle on the reference's deterministic pytest draws."""
    from plnerf_amd import depth as Dp
    R, Ns = 24, 48
    batch, _ = orc.synthetic_blender_rays(R, seed=21)
    # NVS path
    sd = orc.closed_form_state_dict(0, True)
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    with torch.no_grad():
        ret = P.render_rays(g(batch), make_net(P, sd), qfn, Ns, "linear", "midpoint", retraw=True, perturb=1.0,
                            N_importance=0, white_bkgd=True, pytest=True)
    ref = orc.render_rays(batch, sd, None, Ns, "linear", "midpoint", retraw=True, perturb=1.0, N_importance=0,
                          white_bkgd=True, pytest=True)
    assert set(ret) == {"rgb_map", "disp_map", "acc_map", "depth_map", "raw"}
    for k in ("rgb_map", "acc_map", "depth_map", "disp_map"):
        assert_close(ret[k], ref[k], what=f"single pass {k}")
    # depth-supervised variant
    gdummy = {"N_importance": 0, "N_samples": Ns, "space_carving_weight": 0.05}
    Dp, kw, _, _ = _depth_setup_single(P, gdummy)
    out = Dp.render_rays(g(batch), retraw=True, pytest=True, **kw)
    sd_d = orc.closed_form_state_dict_depth(0, True)
    refd = orc.render_rays_depth(batch, sd_d, None, Ns, "linear", "midpoint", perturb=1.0, N_importance=0,
                                 white_bkgd=True, pytest=True)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "depth_map", "z_vals", "weights", "pred_hyp", "u", "raw"}
    assert out["pred_hyp"].shape == (R, Ns) and out["pred_hyp"].requires_grad
    assert torch.equal(out["u"].cpu(), refd["u"])
    for k in ("rgb_map", "acc_map", "depth_map", "z_vals", "weights"):
        assert_close(out[k], refd[k], what=f"depth single pass {k}")
    assert_close(out["pred_hyp"], refd["pred_hyp"], atol=1e-4, rtol=1e-4, what="depth single pass pred_hyp")


def _depth_setup_single(P, gd):
    """_depth_setup for N_importance = 0: one network."""
    from plnerf_amd import depth as Dp
    kw, kw_test, start, grad_vars, opt = Dp.create_nerf(depth_args_of(gd), device=dev())
    assert kw["network_fine"] is None and len(grad_vars) == 24
    kw["network_fn"].load_state_dict(orc.closed_form_state_dict_depth(0, True))
    return Dp, kw, grad_vars, opt


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_empty_and_ragged_batches(P, precision):
    """Ragged ends of a chunked image (batchify_rays run_plnerf.py:95-106 hands render_rays whatever is left):
    an empty ray batch flows through forward and backward with zero gradients, and a single ray with odd sample
    counts (9 + 5: nothing a multiple of a tile) matches the oracle."""
    sd = orc.closed_form_state_dict(0, True)
    nc, nf = make_net(P, sd, precision), make_net(P, sd, precision)
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    kw = dict(network_fine=nf, white_bkgd=True, perturb=1.0)
    ret = P.render_rays(torch.zeros(0, 11, device=dev()), nc, qfn, 16, "linear", "midpoint", retraw=True,
                        N_importance=8, **kw)
    assert ret["rgb_map"].shape == (0, 3) and ret["raw"].shape == (0, 24, 4) and ret["z_std"].shape == (0,)
    (ret["rgb_map"].sum() + ret["rgb0"].sum()).backward()
    for net in (nc, nf):
        assert all(p.grad is not None and float(p.grad.abs().sum()) == 0.0 for p in net.parameters())
    batch, _ = orc.synthetic_blender_rays(1, seed=3)
    with torch.no_grad():
        ret = P.render_rays(g(batch), nc, qfn, 9, "linear", "midpoint", N_importance=5, pytest=True, **kw)
    ref = orc.render_rays(batch, sd, sd, 9, "linear", "midpoint", perturb=1.0, N_importance=5, white_bkgd=True,
                          pytest=True)
    tol = 1e-5 if precision == "fp32" else 1e-4
    for k in ("rgb_map", "rgb0", "acc_map", "depth_map"):
        assert_close(ret[k], ref[k], atol=tol, rtol=tol, what=f"1 ray 9+5 {precision} {k}")


def test_render_rays_random_configurations(P):
    """Differential sweep of render_rays' argument space against the oracle on the reference's deterministic
    (pytest=True) draws: sample counts, mode / colour mode, background, noise, disparity sampling, constant_init,
    farcolorfix.  Coarse-pass outputs to 1e-5 on every ray; the final maps to 3e-5 on all but a few rays and to 5e-3
    on those (they sit behind the sampler's discontinuities)."""
    rng = np.random.default_rng(1234)
    # the "sharpened" weights (acc ~ 1): with near-zero densities 1 - exp(-sigma dist) cancels to ~4 digits in ANY
    # fp32 evaluation (the reference's included), and the sampler turns that into 1e-3 shifts of the fine samples
    sd = orc.closed_form_state_dict(0, True)
    nc, nf = make_net(P, sd), make_net(P, sd)
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    for case in range(14):
        mode = ["linear", "constant"][int(rng.integers(2))]
        cfg = dict(
            N_samples=int(rng.choice([8, 17, 32, 64])), N_importance=int(rng.choice([4, 9, 32, 128])),
            mode=mode, color_mode=["midpoint", "left"][int(rng.integers(2))], white_bkgd=bool(rng.integers(2)),
            raw_noise_std=float(rng.choice([0.0, 1.0])), lindisp=bool(rng.integers(2)),
            # jittered draws only: det=True puts u = 1.0 on the searchsorted knife edge, where a 1-ulp
            # difference in a coarse weight moves the last draw of EVERY ray by a bin -- the det path is pinned
            # bit-exactly on identical inputs by the sampler tests instead
            perturb=1.0,
            constant_init=bool(rng.integers(4) == 0), farcolorfix=bool(rng.integers(2)))
        R = int(rng.choice([1, 7, 33]))
        batch, _ = orc.synthetic_blender_rays(R, seed=100 + case)
        kw = dict(cfg)
        Ns, mo, cm = kw.pop("N_samples"), kw.pop("mode"), kw.pop("color_mode")
        with torch.no_grad():
            ret = P.render_rays(g(batch), nc, qfn, Ns, mo, cm, retraw=True, network_fine=nf, pytest=True, **kw)
        ref = orc.render_rays(batch, sd, sd, Ns, mo, cm, retraw=True, pytest=True, **kw)
        assert set(ret) == set(ref), (cfg, set(ret) ^ set(ref))
        for k in ("rgb0", "acc0", "depth0"):
            assert_close(ret[k], ref[k], what=f"case {case} {cfg} {k}")
        # behind the sampler a 1e-7 difference in a coarse weight can move a draw into the neighbouring bin (flat
        # stretches of the cdf where relu(sigma + noise) = 0): a few fine samples then differ between ANY two fp32
        # implementations.  A wrong flag or a wrong operand would move every ray.
        assert ret["raw"].shape == ref["raw"].shape and ret["z_std"].shape == ref["z_std"].shape
        for k in ("rgb_map", "acc_map", "depth_map"):
            a, b = ret[k].detach().cpu().double(), ref[k].double()
            err = ((a - b).abs() / (1.0 + b.abs())).reshape(a.shape[0], -1).amax(dim=1)
            assert float(err.max()) <= 5e-3, f"case {case} {cfg} {k}: max error {float(err.max()):.2e}"
            assert int((err > 3e-5).sum()) <= max(1, a.shape[0] // 4), f"case {case} {cfg} {k}: {int((err > 3e-5).sum())} rays off"


def test_fused_adam_matches_torch(P):
    """plnerf_adam_step against torch.optim.Adam; with clip_value against clip_grad_value_ + Adam (the depth-supervised
    loop, run_nerf_sample_based_depth.py:1156-1157); a set guard word withholds the launch and counts it."""
    from plnerf_amd import _lib as L
    gen = torch.Generator().manual_seed(0)
    n = 100003
    p0, gr = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-3
    for clip in (0.0, 7e-4):
        ref = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=5e-4, betas=(0.9, 0.999))
        p, m, v = g(p0.clone()), g(torch.zeros(n)), g(torch.zeros(n))
        for step in range(1, 4):
            ref.grad = gr * step
            if clip > 0:
                torch.nn.utils.clip_grad_value_([ref], clip)
            opt.step()
            L.check(L.lib().plnerf_adam_step(L.dptr(p), L.dptr(g(gr * step)), L.dptr(m), L.dptr(v), n, 5e-4, 0.9, 0.999,
                                             1e-8, step, 1.0, clip, None, None, None, L.stream()), "adam")
        assert_close(p, ref.detach(), atol=1e-6, rtol=1e-6, what=f"adam params (clip {clip})")
    # data parallel: the buffer holds the SUM over `world` ranks, the launch takes 1 / world -- and clip_value bounds the
    # AVERAGED gradient (clip_grad_value_ after the mean, as one rank stepping the global batch does), not the sum
    world, clip = 8, 7e-4
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=5e-4, betas=(0.9, 0.999))
    p, m, v = g(p0.clone()), g(torch.zeros(n)), g(torch.zeros(n))
    for step in range(1, 4):
        total = gr * step * world * 0.5          # averaged: entries on both sides of the clip value
        ref.grad = total / world
        assert 0.05 < float((ref.grad.abs() > clip).float().mean()) < 0.95
        torch.nn.utils.clip_grad_value_([ref], clip)
        opt.step()
        L.check(L.lib().plnerf_adam_step(L.dptr(p), L.dptr(g(total)), L.dptr(m), L.dptr(v), n, 5e-4, 0.9, 0.999, 1e-8, step,
                                         1.0 / world, clip, None, None, None, L.stream()), "adam")
    assert_close(p, ref.detach(), atol=1e-6, rtol=1e-6, what="adam params (1 / world, then clip)")
    assert_close(m, opt.state[ref]["exp_avg"], atol=1e-9, rtol=1e-5, what="adam first moment (1 / world, then clip)")
    # guards: either word set -> nothing changes, the launch is counted
    words = g(torch.zeros(2)).to(torch.int32)
    count = g(torch.zeros(1)).to(torch.int32)
    before = (p.clone(), m.clone(), v.clone())
    for which in (0, 1):
        words.zero_()
        words[which] = 4
        L.check(L.lib().plnerf_adam_step(L.dptr(p), L.dptr(g(gr)), L.dptr(m), L.dptr(v), n, 5e-4, 0.9, 0.999, 1e-8, 4, 1.0,
                                         0.0, L.dptr(words[0:1], "w", torch.int32), L.dptr(words[1:2], "w", torch.int32),
                                         L.dptr(count, "c", torch.int32), L.stream()), "adam")
    assert all(torch.equal(a, b) for a, b in zip(before, (p, m, v))) and int(count.item()) == 2
    words.zero_()
    L.check(L.lib().plnerf_adam_step(L.dptr(p), L.dptr(g(gr)), L.dptr(m), L.dptr(v), n, 5e-4, 0.9, 0.999, 1e-8, 4, 1.0, 0.0,
                                     L.dptr(words[0:1], "w", torch.int32), L.dptr(words[1:2], "w", torch.int32),
                                     L.dptr(count, "c", torch.int32), L.stream()), "adam")
    assert not torch.equal(before[0], p) and int(count.item()) == 2


# ----------------------------------------------------------------------------- full-size properties
def test_flat_adam_is_torch_adam(P, tmp_path):
    """optim.FlatAdam (what create_nerf hands out on the GPU) against torch.optim.Adam on the same gradients:
    per-step parameters over a changing learning rate (run_plnerf.py:1311-1315), parameters without a gradient
    skipped, gradients in one buffer / two buffers / scattered tensors, and the checkpoint's optimizer_state_dict
    (run_plnerf.py:1324-1332) crossing over in both directions."""
    from plnerf_amd.optim import FlatAdam
    torch.manual_seed(0)
    shapes = [(256, 63), (256,), (256, 256), (256,), (3, 128), (3,)]
    mk = lambda: [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i)).to(dev()))
                  for i, s in enumerate(shapes)]
    pa, pb = mk(), mk()
    oa = FlatAdam(pa, lr=5e-4, betas=(0.9, 0.999))
    ob = torch.optim.Adam(pb, lr=5e-4, betas=(0.9, 0.999))
    assert isinstance(oa, torch.optim.Adam)
    sizes = [p.numel() for p in pa]
    gen = torch.Generator(device=dev()).manual_seed(1)
    for it in range(6):
        flat = torch.randn(sum(sizes), device=dev(), generator=gen) * (10.0 ** (it - 3))
        if it % 3 == 0:      # one buffer (what MlpFn.backward produces)
            ga = [t.view(s) for t, s in zip(flat.split(sizes), shapes)]
        elif it % 3 == 1:    # two buffers (two networks under one optimizer, depth-supervised variant)
            a, b = flat[:sum(sizes[:3])].clone(), flat[sum(sizes[:3]):].clone()
            ga = [t.view(s) for t, s in zip(list(a.split(sizes[:3])) + list(b.split(sizes[3:])), shapes)]
        else:                # unrelated tensors
            ga = [t.clone().view(s) for t, s in zip(flat.split(sizes), shapes)]
        skip = 4 if it == 4 else -1          # a parameter without a gradient is left alone
        for k, (x, y) in enumerate(zip(pa, pb)):
            x.grad = None if k == skip else ga[k]
            y.grad = None if k == skip else ga[k].clone()
        lr = 5e-4 * 0.1 ** (it / 3.0)
        for o in (oa, ob):
            for grp in o.param_groups:
                grp["lr"] = lr
            o.step()
        for k, (x, y) in enumerate(zip(pa, pb)):
            assert_close(x, y, atol=1e-7, rtol=2e-6, what=f"FlatAdam step {it} param {k}")
    assert float(oa.state[pa[4]]["step"]) == 5.0 and float(oa.state[pa[0]]["step"]) == 6.0
    # wire format: each loads the other's state and they keep agreeing
    path = str(tmp_path / "opt.tar")
    torch.save({"a": oa.state_dict(), "b": ob.state_dict()}, path)
    ck = torch.load(path, map_location=dev())
    pc, pd = mk(), mk()
    for src, dst in ((pa, pc), (pb, pd)):
        for x, y in zip(src, dst):
            y.data.copy_(x.data)
    oc = FlatAdam(pc, lr=5e-4, betas=(0.9, 0.999)); oc.load_state_dict(ck["b"])     # torch -> flat
    od = torch.optim.Adam(pd, lr=5e-4, betas=(0.9, 0.999)); od.load_state_dict(ck["a"])   # flat -> torch
    flat = torch.randn(sum(sizes), device=dev(), generator=gen)
    for ps, o in ((pc, oc), (pd, od)):
        for x, t, s_ in zip(ps, flat.split(sizes), shapes):
            x.grad = t.clone().view(s_)
        o.step()
    for k, (x, y) in enumerate(zip(pc, pd)):
        assert_close(x, y, atol=1e-7, rtol=2e-6, what=f"after state_dict crossing, param {k}")
    assert float(oc.state[pc[0]]["step"]) == 7.0 and float(oc.state[pc[4]]["step"]) == 6.0


def test_full_size_properties(P):
    """BASELINE config 2 sizes (4096 rays, 64+128): size-independent invariants."""
    from plnerf_amd import functional as Fn
    R, S, N = 4096, 64, 128
    raw, z, near, far, d, _ = quad_case(R, S, 77)
    rgb, disp, acc, w, depth, tau, Tr = P.raw2outputs(g(raw), g(z), g(near), g(far), g(d), "linear", "midpoint",
                                                      white_bkgd=False)
    # weights are a partition of 1 - T_end; T is non-increasing; acc == sum(weights)
    assert (w >= 0).all() and (Tr[:, 1:] <= Tr[:, :-1] + 1e-7).all()
    assert_close(acc, w.sum(-1), what="acc == sum w")
    assert_close(w.sum(-1) + Tr[:, -1], torch.ones(R), atol=2e-5, what="sum w + T_end == 1")
    assert ((depth >= 2.0 * acc - 1e-4) & (depth <= 6.0 * acc + 1e-4)).all()
    u = torch.rand(R, N, device=dev())
    zs = Fn.sample_pl(g(z), w, tau, Tr, g(near), g(far), u, 1e-4, 1e-3)
    assert (zs >= 2.0).all() and (zs <= 6.0).all()
    merged = Fn.merge_sort(g(z), zs, g(near), g(far))
    assert (merged[:, 1:] >= merged[:, :-1]).all()                       # sortedness
    assert_close(merged.sum(-1), g(z).sum(-1) + zs.sum(-1), atol=1e-3, rtol=1e-5, what="multiset preserved")
    # sorting is idempotent
    assert torch.equal(Fn.merge_sort(merged[:, :S], merged[:, S:], g(near), g(far)), merged)
    # quadrature is linear in the colours: doubling sigmoid(rgb) logits is not linear, but white_bkgd is affine
    rgb_w = P.raw2outputs(g(raw), g(z), g(near), g(far), g(d), "linear", "midpoint", white_bkgd=True)[0]
    assert_close(rgb_w, rgb + (1 - acc)[:, None], atol=2e-6, what="white background is rgb + 1 - acc")
    # MLP at full netchunk size: rows are independent -> any split of the batch gives identical rows
    net = make_net(P, orc.closed_form_state_dict(0, False))
    pts = g((torch.rand(1024, 64, 3) * 2 - 1) * 3)
    vd = torch.nn.functional.normalize(g(torch.randn(1024, 3)), dim=-1)
    with torch.no_grad():
        full = net.query(pts, vd)
        half = torch.cat([net.query(pts[:300], vd[:300]), net.query(pts[300:], vd[300:])], 0)
    assert torch.equal(full, half)


# ----------------------------------------------------------------------------- caller side (section 8f)
def test_train_loop_matches_oracle_over_steps(P):
    """TrainStep (run_plnerf.py:1283-1316: two Adams, LR decay, quirks) for 3 steps against the oracle's
    loop on the same rays and the reference's deterministic draws: loss curve and final weights."""
    import tempfile, os
    from argparse import Namespace
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "exp"))
    args = Namespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128, N_samples=64,
                     netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4,
                     coarse_lrate=5e-4, ft_path=None, ckpt_dir=d, expname="exp", no_reload=True, perturb=1.0,
                     white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", dataset="blender",
                     no_ndc=False, lindisp=False, lrate_decay=1, constant_init=0, chunk=32768, precision="fp32")
    kw, _, start, _, opt, opt_c = P.create_nerf(args, device=dev())
    sd_c, sd_f = orc.closed_form_state_dict(0, False), orc.closed_form_state_dict(1, False)
    kw["network_fn"].load_state_dict(sd_c)
    kw["network_fine"].load_state_dict(sd_f)
    batch, target = orc.synthetic_blender_rays(48, seed=9)
    rays = (g(batch[:, 0:3]), g(batch[:, 3:6]))
    K = [[1111.111, 0, 400], [0, 1111.111, 400], [0, 0, 1]]
    ts = P.TrainStep(args, dict(kw, pytest=True), opt, opt_c, start=start, distributed=False)
    okw = dict(N_samples=64, N_importance=128, mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True,
               raw_noise_std=0.0, pytest=True)
    state, lr = {}, 5e-4
    for step in range(3):
        ref_loss, _, _ = orc.train_step(sd_c, sd_f, batch, target, okw, lr=lr, adam_state=state)
        loss, psnr = ts(800, 800, K, rays, g(target), near=2.0, far=6.0)
        assert abs(float(loss) - float(ref_loss)) <= 2e-5 * max(1.0, float(ref_loss)), (step, float(loss), float(ref_loss))
        lr = 5e-4 * 0.1 ** (step / 1000.0)            # the rate the reference installs after this step
        assert abs(opt.param_groups[0]["lr"] - lr) < 1e-12 and abs(opt_c.param_groups[0]["lr"] - lr) < 1e-12
    worst = 0.0
    for net, sd in ((kw["network_fn"], sd_c), (kw["network_fine"], sd_f)):
        for name, prm in net.named_parameters():
            worst = max(worst, maxdiff(prm, sd[name]))
    print(f"3 training steps: final loss {float(loss):.6f}, max |param - oracle| {worst:.3e}")
    assert worst <= 2.5e-3       # Adam moves each weight ~lr per step; sign flips of ~0 gradients cost <= 2 lr / step


def test_full_image_render_c2w(P):
    """render(c2w=...) (run_plnerf.py:136-138, 95-107): every pixel of a small view, chunked, against the
    oracle on the same rays with det sampling disabled (random draws injected through pytest=True)."""
    H, W, f = 12, 16, 18.0
    K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
    c2w = P.rays.pose_spherical(25.0, -30.0, 4.0)[:3, :4]
    sd_c, sd_f = orc.closed_form_state_dict(0, True), orc.closed_form_state_dict(1, True)
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    kw = dict(network_query_fn=qfn, perturb=1.0, N_importance=64, network_fine=make_net(P, sd_f), N_samples=32,
              network_fn=make_net(P, sd_c), white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint")
    with torch.no_grad():
        rgb, disp, acc, extras = P.render(H, W, K, chunk=H * W, c2w=g(c2w), ndc=False, near=2.0, far=6.0,
                                          use_viewdirs=True, pytest=True, **kw)
        rgb_chunked = P.render(H, W, K, chunk=50, c2w=g(c2w), ndc=False, near=2.0, far=6.0, use_viewdirs=True,
                               pytest=False, **dict(kw, perturb=0.0, mode="constant"))[0]
    assert rgb.shape == (H, W, 3) and acc.shape == (H, W) and extras["depth_map"].shape == (H, W)
    assert rgb_chunked.shape == (H, W, 3) and torch.isfinite(rgb_chunked).all()
    o, dd = orc.get_rays(H, W, K, c2w)
    batch = orc.pack_ray_batch(o, dd, 2.0, 6.0)
    ref = orc.render_rays(batch, sd_c, sd_f, 32, "linear", "midpoint", perturb=1.0, N_importance=64,
                          white_bkgd=True, pytest=True)
    print(f"full image: rgb max err {maxdiff(rgb.reshape(-1, 3), ref['rgb_map']):.3e}")
    assert_close(rgb.reshape(-1, 3), ref["rgb_map"], what="full-image rgb")
    assert_close(extras["rgb0"].reshape(-1, 3), ref["rgb0"], what="full-image rgb0")


def test_render_path(P, tmp_path):
    """render_path (run_plnerf.py:178-216): one render() per pose, numpy stacks, render_factor downsampling;
    image writing is outside the path and refuses loudly."""
    H, W, f = 8, 12, 14.0
    K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
    poses = torch.stack([P.rays.pose_spherical(a, -30.0, 4.0) for a in (0.0, 40.0, 80.0)]).to(dev())
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    sd = orc.closed_form_state_dict(0, True)
    kw = dict(network_query_fn=qfn, perturb=0.0, N_importance=16, network_fine=make_net(P, sd), N_samples=16,
              network_fn=make_net(P, sd), white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint",
              ndc=False, near=2.0, far=6.0, use_viewdirs=True)
    rgbs, disps = P.render_path(poses, (H, W, f), K, 64, kw)
    assert rgbs.shape == (3, H, W, 3) and disps.shape == (3, H, W) and np.isfinite(rgbs).all()
    with torch.no_grad():
        one = P.render(H, W, K, chunk=64, c2w=poses[1, :3, :4], **kw)[0]
    assert np.array_equal(rgbs[1], one.cpu().numpy())
    half = P.render_path(poses[:1], (H, W, f), K, 64, kw, render_factor=2)[0]
    assert half.shape == (1, H // 2, W // 2, 3)
    with pytest.raises(NotImplementedError):
        P.render_path(poses[:1], (H, W, f), K, 64, kw, savedir=str(tmp_path))
