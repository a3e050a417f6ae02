"""Piecewise-constant mode's one-launch stages (plnerf_coarse_epilogue_const / plnerf_fine_epilogue_const,
csrc/epilogue.hip) on a real MI355X: against the separate launches they replace -- plnerf_quad_fwd in constant mode, torch's
z_mid, plnerf_sample_const, plnerf_merge_sort, plnerf_ray_points -- bit for bit, forward and backward, at every bin count at
which torch.sum's order changes, at the tiers of the sort network, on rows that take the sampler's special cases; then through
render.render_rays, depth.render_rays and the two training steps, with the switches on and off.

Every comparison is torch.equal (NaNs, which torch.equal never calls equal, are held to the same bits: _same): the kernel runs the separate kernels' own device functions on the same fp32 values
(csrc/ray_dev.h).  The one exception is z_std, which torch.std forms in fp32 and the kernel in fp64 from the same samples:
atol = rtol = 2e-6, the bound of the linear sibling's test (tests/test_gpu_step.py)."""
import sys

import pytest
import torch

from gpu_support import (P, assert_close, assert_same_losses, assert_same_nvs_state, depth_nets, dev, g, make_net, maxdiff,
                         nvs_nets, quad_case, scene)
from oracle import plnerf_oracle as orc
from run_args import depth_args_of

pytestmark = pytest.mark.gpu
R_DEFAULT = 133      # (four rays per workgroup: the last one is ragged)
ZSTD = dict(atol=2e-6, rtol=2e-6)


@pytest.fixture(scope="module")
def Fn(P):
    from plnerf_amd import functional
    return functional


def _same(a, b):
    """torch.equal, with NaNs held to the same bits: the disparity of a ray without any density is 0 / 0 on either route, and
    torch.equal calls two NaNs different."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if torch.equal(a, b):
        return True
    return a.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case(R, S, N, seed, with_noise=False):
    raw, z, near, far, d, _ = quad_case(R, S, seed)
    gen = torch.Generator().manual_seed(S * 7 + N)
    o = torch.randn(R, 3, generator=gen)
    u = torch.rand(R, N, generator=gen)
    noise = torch.rand(R, S, generator=gen) if with_noise else None
    cot = torch.randn(R, 3, generator=gen)
    return dict(raw=raw, z=z, near=near, far=far, o=o, d=d, u=u, noise=noise, cot=cot)


def _separate_coarse(Fn, c, N, white):
    """QuadratureFn("constant") -> torch z_mid -> Fn.sample_const -> Fn.merge_sort -> Fn.ray_points, with raw.grad under
    the rgb cotangent."""
    raw = g(c["raw"]).requires_grad_(True)
    z, near, far = g(c["z"]), g(c["near"]), g(c["far"])
    noise = None if c["noise"] is None else g(c["noise"])
    rgb, disp, acc, w, depth, _, _ = Fn.QuadratureFn.apply(raw, z, near, far, g(c["d"]), noise, "constant", "midpoint",
                                                           white, False)
    z_mid = .5 * (z[..., 1:] + z[..., :-1])
    zs = Fn.sample_const(z_mid, w[..., 1:-1], g(c["u"])).detach()
    z_fine = Fn.merge_sort(z, zs, near, far)
    pts = Fn.ray_points(g(c["o"]), g(c["d"]), z_fine)
    z_std = torch.std(torch.clamp(zs, near, far), dim=-1, unbiased=False)
    (rgb * g(c["cot"])).sum().backward()
    return dict(rgb0=rgb, disp0=disp, acc0=acc, depth0=depth, weights=w, z_fine=z_fine, pts=pts), z_std, raw.grad


def _fused_coarse(Fn, c, N, white, u="given", draws=None):
    raw = g(c["raw"]).requires_grad_(True)
    noise = None if c["noise"] is None else g(c["noise"])
    u = g(c["u"]) if isinstance(u, str) else u
    out = Fn.CoarseEpilogueFn.apply(raw, g(c["z"]), g(c["near"]), g(c["far"]), g(c["o"]), g(c["d"]), noise, u, N, "left",
                                    white, True, 1e-4, 1e-3, draws, True, "constant")
    (out[0] * g(c["cot"])).sum().backward()
    names = ("rgb0", "disp0", "acc0", "depth0", "z_fine", "pts")
    return dict(zip(names, out[:6]), weights=out[7]), out[6], raw.grad


def _assert_coarse_equal(Fn, c, N, white, what):
    sep, std_s, grad_s = _separate_coarse(Fn, c, N, white)
    fus, std_f, grad_f = _fused_coarse(Fn, c, N, white)
    for k in sep:
        assert _same(sep[k], fus[k]), (what, k, maxdiff(sep[k], fus[k]))
    assert_close(std_f, std_s, what=f"{what} z_std", **ZSTD)
    assert torch.equal(grad_s, grad_f), (what, "raw.grad", maxdiff(grad_s, grad_f))
    return sep


# n = S - 2 is the length of the row torch.sum adds up: 1, 2, the 4..7 special case, 7, the first 8-lane vector; then the
# workloads' sizes and the edges of the sort network's tiers (S + N <= 64 / 128 / 256 / 512 / 1024 with the N sub-tiers)
SHAPES = [(3, 1), (4, 5), (6, 7), (9, 64), (10, 65), (37, 23), (64, 128), (128, 64), (66, 190), (130, 127), (300, 200),
          (512, 512), (63, 1), (65, 65)]      # (the last two: the scan's and the cdf's 64-lane chunk edges)


@pytest.mark.parametrize("S,N", SHAPES)
def test_coarse_entry_equals_the_separate_launches(Fn, S, N):
    white = SHAPES.index((S, N)) % 2 == 0
    c = _case(R_DEFAULT, S, N, 1000 + S, with_noise=(S == 37))
    _assert_coarse_equal(Fn, c, N, white, f"S={S} N={N}")


def test_coarse_entry_on_a_single_ray(Fn):
    _assert_coarse_equal(Fn, _case(1, 64, 128, 5), 128, True, "R=1")


def test_coarse_entry_hard_rows(Fn):
    """Rows that take the sampler's and the sort's special cases, at (16, 24)."""
    S, N, R = 16, 24, R_DEFAULT
    c = _case(R, S, N, 77)
    c["raw"][0, :, 3] = -5.0                 # no density at all: a flat pdf from the 1e-5 term (relu'd to zero)
    c["raw"][1, :, 3] = -5.0
    c["raw"][1, 6, 3] = 1e6                  # one opaque sample: the cdf is a plateau on both sides of one step
    c["raw"][2, :, 3] = 0.0                  # exact zeros: every cdf step is the same
    for row, (p, q) in ((70, (4, 5)), (71, (0, 1)), (72, (S - 2, S - 1))):      # coarse depths not ascending: the general
        c["z"][row, [p, q]] = c["z"][row, [q, p]]                                 # sort network (neighbours: intervals stay short)
    c["near"][5:9] = 3.6                     # near / far inside the depth range: the clamp acts
    c["far"][5:9] = 3.9
    c["u"][0, :4] = torch.tensor([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24])      # the ends of the cdf
    c["u"][1, :4] = torch.tensor([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24])
    sep = _assert_coarse_equal(Fn, c, N, True, "hard rows")
    zf = sep["z_fine"]
    assert bool((zf[:, 1:] >= zf[:, :-1]).all())
    # the clamp really acted on the rows it was built for, and the flat rows really are flat
    z, near, far = g(c["z"]), g(c["near"]), g(c["far"])
    w = sep["weights"]
    zs = Fn.sample_const(.5 * (z[..., 1:] + z[..., :-1]), w[..., 1:-1], g(c["u"]))
    assert bool(((zs[5:9] < near[5:9]) | (zs[5:9] > far[5:9])).any())
    assert float(w[0].detach().abs().max()) == 0.0 and float(w[1, 6].detach()) == 1.0


def test_draws_in_the_kernel_equal_the_same_draws_handed_in(Fn):
    """DrawSource(seed=11, ray_id0=40, step=5): the coarse entry draws on stream U, the final entry on HYP_STREAM."""
    S, N, R = 37, 23, R_DEFAULT
    c = _case(R, S, N, 3)
    src = Fn.DrawSource(seed=11, ray_id0=40, step=5)
    a = _fused_coarse(Fn, c, N, False, u=src.uniform(R, N, Fn.DrawSource.U, dev()))
    b = _fused_coarse(Fn, c, N, False, u=None, draws=src)
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    u_hyp = src.uniform(R, N, Fn.FineEpilogueFn.HYP_STREAM, dev())
    fa = _fused_final(Fn, c, N, True, u=u_hyp)
    fb = _fused_final(Fn, c, N, True, u=None, draws=src)
    assert torch.equal(fb[0]["u_out"], u_hyp)
    for k in fa[0]:
        assert torch.equal(fa[0][k], fb[0][k]), k
    assert torch.equal(fa[1], fb[1])
    assert not torch.equal(fa[0]["samples"], _fused_final(Fn, c, N, True, u=src.uniform(R, N, Fn.DrawSource.U, dev()))[0]["samples"])


def test_shared_row_of_draws(Fn):
    """One row [N] for every ray (stride 0) == the separate route on the expanded row."""
    S, N, R = 37, 23, R_DEFAULT
    c = _case(R, S, N, 4)
    row = torch.linspace(0., 1., N)
    c["u"] = row.expand(R, N).contiguous()
    sep, std_s, grad_s = _separate_coarse(Fn, c, N, True)
    fus, std_f, grad_f = _fused_coarse(Fn, c, N, True, u=g(row))
    for k in sep:
        assert torch.equal(sep[k], fus[k]), k
    assert_close(std_f, std_s, what="z_std", **ZSTD)
    assert torch.equal(grad_s, grad_f)
    a, b = _separate_final(Fn, c, N, True), _fused_final(Fn, c, N, True, u=g(row))
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[2], b[2])


# ----------------------------------------------------------------------------- the final stage
def _hyp_cot(c, N):
    gen = torch.Generator().manual_seed(N + 1)
    return torch.randn(c["raw"].shape[0], N, generator=gen)


def _separate_final(Fn, c, N, white):
    raw = g(c["raw"]).requires_grad_(True)
    z, near, far, u = g(c["z"]), g(c["near"]), g(c["far"]), g(c["u"])
    noise = None if c["noise"] is None else g(c["noise"])
    rgb, disp, acc, w, depth, _, _ = Fn.QuadratureFn.apply(raw, z, near, far, g(c["d"]), noise, "constant", "midpoint",
                                                           white, False)
    z_mid = .5 * (z[..., 1:] + z[..., :-1])
    s, inds = Fn.sample_const(z_mid, w[..., 1:-1], u, want_inds=True)
    ((rgb * g(c["cot"])).sum() + (s * g(_hyp_cot(c, N))).sum()).backward()
    out = dict(rgb=rgb, disp=disp, acc=acc, depth=depth, weights=w, samples=s, inds=inds, u_out=u, bins_out=z_mid)
    return out, torch.std(s, dim=-1, unbiased=False), raw.grad


def _fused_final(Fn, c, N, white, u="given", draws=None):
    raw = g(c["raw"]).requires_grad_(True)
    noise = None if c["noise"] is None else g(c["noise"])
    u = g(c["u"]) if isinstance(u, str) else u
    rgb, disp, acc, depth, w, tau, T, s, u_out, inds, z_std = Fn.FineEpilogueFn.apply(
        raw, g(c["z"]), g(c["near"]), g(c["far"]), g(c["d"]), noise, u, N, "left", white, True, 1e-4, 1e-3, draws, "constant")
    assert tau.numel() == 0 and T.numel() == 0
    bins = s.grad_fn.saved_tensors[8]      # bins_out: what the backward hands plnerf_sample_const_bwd
    ((rgb * g(c["cot"])).sum() + (s * g(_hyp_cot(c, N))).sum()).backward()
    out = dict(rgb=rgb, disp=disp, acc=acc, depth=depth, weights=w, samples=s, inds=inds, u_out=u_out, bins_out=bins)
    return out, z_std, raw.grad


@pytest.mark.parametrize("S,N", [(3, 1), (9, 7), (64, 128), (192, 128)])
def test_final_entry_equals_the_separate_chain(Fn, S, N):
    c = _case(R_DEFAULT, S, N, 2000 + S, with_noise=(S == 9))
    white = S != 64
    sep, std_s, grad_s = _separate_final(Fn, c, N, white)
    fus, std_f, grad_f = _fused_final(Fn, c, N, white)
    for k in sep:
        assert _same(sep[k], fus[k]), (k, maxdiff(sep[k], fus[k]))
    assert fus["inds"].dtype == torch.int64
    assert_close(std_f, std_s, what="z_std", **ZSTD)
    assert torch.equal(grad_s, grad_f), maxdiff(grad_s, grad_f)
    # a cotangent on the returned weights joins the sampler's: still the separate route's gradient
    ra, rb = g(c["raw"]).requires_grad_(True), g(c["raw"]).requires_grad_(True)
    z, near, far, u = g(c["z"]), g(c["near"]), g(c["far"]), g(c["u"])
    noise = None if c["noise"] is None else g(c["noise"])
    wc = g(torch.randn(R_DEFAULT, S, generator=torch.Generator().manual_seed(S)))
    q = Fn.QuadratureFn.apply(ra, z, near, far, g(c["d"]), noise, "constant", "midpoint", white, False)
    s = Fn.sample_const(.5 * (z[..., 1:] + z[..., :-1]), q[3][..., 1:-1], u)
    ((q[3] * wc).sum() + (s * g(_hyp_cot(c, N))).sum()).backward()
    f = Fn.FineEpilogueFn.apply(rb, z, near, far, g(c["d"]), noise, u, N, "midpoint", white, False, 1e-4, 1e-3, None,
                                "constant")
    ((f[4] * wc).sum() + (f[7] * g(_hyp_cot(c, N))).sum()).backward()
    assert torch.equal(ra.grad, rb.grad), maxdiff(ra.grad, rb.grad)


# ----------------------------------------------------------------------------- render.render_rays
def _render_module():
    import plnerf_amd  # noqa: F401
    return sys.modules["plnerf_amd.render"]      # (the package attribute `render` is the function)


@pytest.mark.parametrize("kw_mode", [dict(mode="constant"), dict(mode="linear", constant_init=True)], ids=["constant", "constant_init"])
def test_render_rays_takes_the_one_launch_route_and_equals_the_separate_one(P, Fn, kw_mode, monkeypatch):
    Rd = _render_module()
    nc = make_net(P, orc.closed_form_state_dict(0, False), "f16x3")
    nf = make_net(P, orc.closed_form_state_dict(1, False), "f16x3")
    emb, _ = P.get_embedder(10, 0)
    embd, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb, embd)
    batch, _ = orc.synthetic_blender_rays(50, seed=4)
    kw = dict(N_samples=16, N_importance=24, color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=1.0,
              retraw=True, network_fine=nf, **kw_mode)

    def run(fuse):
        prev = Fn.set_draw_source(Fn.DrawSource(seed=8, ray_id0=16, step=4))
        Rd.FUSE_CONST_EPILOGUE = fuse
        try:
            with torch.no_grad():
                return P.render_rays(g(batch), nc, qfn, **kw)
        finally:
            Rd.FUSE_CONST_EPILOGUE = True
            Fn.set_draw_source(prev)
    off = run(False)
    on = run(True)
    assert set(on) == set(off) and {"rgb_map", "rgb0", "disp0", "acc0", "depth0", "z_std", "raw"} <= set(on)
    for k in on:
        if k == "z_std":
            assert_close(on[k], off[k], what="z_std", **ZSTD)
        else:
            assert _same(on[k], off[k]), (k, maxdiff(on[k], off[k]))
    # the one-launch route is really taken: the separate stages are out of reach
    def refuse(*a, **k):
        raise AssertionError("a separate stage ran")
    for name in ("sample_const", "merge_sort", "ray_points"):
        monkeypatch.setattr(Fn, name, refuse)
    again = run(True)
    assert torch.equal(again["rgb_map"], on["rgb_map"]) and torch.equal(again["rgb0"], on["rgb0"])
    with pytest.raises(AssertionError, match="a separate stage ran"):
        run(False)


# ----------------------------------------------------------------------------- depth.render_rays
def _depth_kw(golden, precision):
    """The depth variant's two networks (closed-form weights) at 16 + 24 samples in constant mode."""
    from plnerf_amd import depth as Dp
    args = depth_args_of(golden("g8b_depth_variant_128_64"), precision, N_samples=16, N_importance=24, mode="constant")
    kw, _, _, grad_vars, opt = depth_nets(args)
    return Dp, args, kw, grad_vars, opt


def _depth_render(Dp, Fn, kw, batch, fuse, grad=False, **over):
    prev = Fn.set_draw_source(Fn.DrawSource(seed=8, ray_id0=16, step=4))
    Dp.FUSE_STAGES = fuse
    try:
        with torch.set_grad_enabled(grad):
            return Dp.render_rays(batch, retraw=True, **dict(kw, **over))
    finally:
        Dp.FUSE_STAGES = True
        Fn.set_draw_source(prev)


def _assert_same_dict(on, off):
    assert set(on) == set(off)
    for k in on:
        if k == "z_std":
            assert_close(on[k], off[k], what="z_std", **ZSTD)
        else:
            assert _same(on[k], off[k]), (k, maxdiff(on[k], off[k]))


@pytest.mark.parametrize("case", ["two_pass", "single_pass", "joint"])
def test_depth_render_rays_constant_mode_equals_the_separate_launches(P, Fn, golden, case, monkeypatch):
    n_imp = 0 if case == "single_pass" else 24
    Dp, _, kw, _, _ = _depth_kw(golden, "fp32")
    if n_imp == 0:      # the hypotheses come from the one network's own pass
        kw = dict(kw, N_importance=0, network_fine=None)
    assert kw["mode"] == "constant"
    batch = g(orc.synthetic_blender_rays(60, seed=21)[0])
    over = dict(is_joint=True) if case == "joint" else {}
    off = _depth_render(Dp, Fn, kw, batch, False, **over)
    on = _depth_render(Dp, Fn, kw, batch, True, **over)
    _assert_same_dict(on, off)
    assert tuple(on["weights"].shape) == (60, 16 + n_imp) and tuple(on["pred_hyp"].shape) == (60, n_imp or 16)
    if n_imp:
        assert {"weights0", "z_vals0", "rgb0", "z_std"} <= set(on) and tuple(on["weights0"].shape) == (60, 16)
    if case == "joint":
        assert bool((on["u"] == on["u"][:1]).all())
    # without a DrawSource the draws are handed in (perturb = 0: the linspace row)
    Dp.FUSE_STAGES = False
    try:
        with torch.no_grad():
            off_det = Dp.render_rays(batch, retraw=True, **dict(kw, perturb=0., **over))
    finally:
        Dp.FUSE_STAGES = True
    with torch.no_grad():
        on_det = Dp.render_rays(batch, retraw=True, **dict(kw, perturb=0., **over))
    _assert_same_dict(on_det, off_det)
    # the one-launch stages are really taken
    def refuse(*a, **k):
        raise AssertionError("a separate stage ran")
    for name in ("sample_const", "merge_sort"):
        monkeypatch.setattr(Fn, name, refuse)
    _depth_render(Dp, Fn, kw, batch, True, **over)


def test_depth_render_rays_constant_mode_gradients(P, Fn, golden):
    """A loss on pred_hyp and the images, backpropagated to both networks: plnerf_sample_const_bwd + plnerf_quad_bwd behind the
    one-launch stage, like the separate route."""
    batch = g(orc.synthetic_blender_rays(60, seed=22)[0])
    grads, outs = [], []
    for fuse in (True, False):
        Dp, _, kw, grad_vars, _ = _depth_kw(golden, "fp32")
        ret = _depth_render(Dp, Fn, kw, batch, fuse, grad=True)
        loss = ret["rgb_map"].sum() + 0.3 * ret["rgb0"].mean() + 0.01 * ret["pred_hyp"].square().mean() + \
            ret["depth_map"].mean() + 0.1 * ret["weights"].square().sum()
        loss.backward()
        outs.append({k: v.detach() for k, v in ret.items()})
        grads.append([p.grad.detach().clone() for p in grad_vars])
    _assert_same_dict(*outs)
    assert len(grads[0]) == len(grads[1]) and any(float(a.abs().max()) > 0 for a in grads[0])
    for a, b in zip(*grads):
        assert torch.equal(a, b), maxdiff(a, b)


# ----------------------------------------------------------------------------- training
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_train_step_through_the_constant_init_warm_up(P, Fn, precision):
    """constant_init = 3: the first steps render in constant mode (i < constant_init), the rest in linear mode.  Five steps
    of 64 rays at 16 + 24 samples with the switch on and off: the same run (f16x3: the merged backward; fp32: autograd's)."""
    Rd = _render_module()
    H, W = 20, 26
    poses, images, K = scene(P, 4, H, W, seed=3)
    images = g(images)
    pair = []
    for _ in range(2):
        args, kw, opt, opt_c = nvs_nets(P, precision, N_samples=16, N_importance=24, constant_init=3)
        pair.append(P.TrainStep(args, kw, opt, opt_c, distributed=False, seed=5, one_call=False, range_check_every=0))
    logs = ([], [])
    for k in range(5):
        for ts, log, fuse in zip(pair, logs, (True, False)):
            Rd.FUSE_CONST_EPILOGUE = fuse
            try:
                log.append(ts.step_view(H, W, K, poses[k % 4][:3, :4], images[k % 4], near=2.0, far=6.0, n_rand=64))
            finally:
                Rd.FUSE_CONST_EPILOGUE = True
    assert_same_losses(logs)
    assert_same_nvs_state(pair[0], pair[1], f"constant_init {precision}")
    assert pair[0].one_call_steps == 0 and pair[0].merged_steps == (5 if precision == "f16x3" else 0)


def test_depth_train_step_in_constant_mode(P, Fn, golden):
    R = 64
    batch, target = orc.synthetic_blender_rays(R, seed=9)
    target_h = 2.0 + 4.0 * torch.rand(3, R, 1, generator=torch.Generator().manual_seed(9))
    batch, target, target_h = g(batch), g(target), g(target_h)
    runs = []
    for fuse in (True, False):
        Dp, args, kw, grad_vars, opt = _depth_kw(golden, "f16x3")
        step = Dp.DepthTrainStep(args, kw, opt, grad_vars, distributed=False, seed=2)
        losses = []
        Dp.FUSE_STAGES = fuse
        try:
            for _ in range(3):
                loss, img_loss, sc, _ = step(batch, target, target_h)
                losses.append((loss.detach().clone(), img_loss.detach().clone(), torch.as_tensor(sc).detach().clone()))
        finally:
            Dp.FUSE_STAGES = True
        state = []
        for p in grad_vars:
            st = opt.state[p]
            state.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
        runs.append((losses, state))
    for k, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert all(torch.isfinite(x).all() and torch.equal(x, y) for x, y in zip(a, b)), (k, a, b)
    for k, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
            assert torch.equal(x, y), (k, name, maxdiff(x, y))
