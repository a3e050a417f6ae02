"""generic.HONOUR_PRECISION: networks outside the compiled trunk with their forward in the network's own 16-bit mode
(plnerf_gemm_h16) and their backward in fp32 -- against the same module in fp64 torch, against the switch-off route, through
a guarded training step and through render()."""
import os
import tempfile
import warnings

import pytest
import torch

from gpu_support import assert_close, dev, g, maxdiff, same_bits, stage_tap
from run_args import nvs_args

pytestmark = pytest.mark.gpu

# tests/test_gpu_modes.py's bounds per mode on the compiled trunk: forward error / (1 + max |reference|)
FORWARD_TOL = {"f16x3": 1e-5, "bf16x3": 3e-5, "f16": 2e-3, "bf16": 1e-2}
FLIP_BELOW = {"f16x3": 1e-5, "bf16x3": 5e-5}      # (the mode's forward error on a hidden unit)
GRAD_TOL = 2e-4                                      # of max |g|, the existing generic test's
G5_FINAL_TOL = (1e-5, 2e-5)                          # f16x3: rgb / acc / depth / disp, z_std
SHAPES = [dict(D=9, W=320, skips=[4], L=10, Lv=4), dict(D=12, W=96, skips=[3, 6, 9], L=5, Lv=2),
          dict(D=8, W=256, skips=[4], L=12, Lv=6), dict(D=9, W=272, skips=[4], L=10, Lv=0)]
R, S = 21, 37                                        # 777 rows


@pytest.fixture(scope="module")
def P():
    import plnerf_amd
    return plnerf_amd


@pytest.fixture
def honour():
    """The switch on for the test, put back afterwards."""
    from plnerf_amd import generic
    found = generic.HONOUR_PRECISION
    generic.HONOUR_PRECISION = True
    try:
        yield generic
    finally:
        generic.HONOUR_PRECISION = found


def build(P, shape, precision, seed=47):
    D, Wd, skips, Lx, Lv = shape["D"], shape["W"], shape["skips"], shape["L"], shape["Lv"]
    torch.manual_seed(seed)
    emb_fn, in_ch = P.get_embedder(Lx, 0)
    embd_fn, in_ch_v = P.get_embedder(Lv, 0) if Lv > 0 else (None, 0)
    net = P.NeRF(D=D, W=Wd, input_ch=in_ch, input_ch_views=in_ch_v, output_ch=5, skips=skips, use_viewdirs=Lv > 0,
                 precision=precision).to(dev())
    assert not net.is_supported()
    return net, emb_fn, embd_fn


def inputs():
    gen = torch.Generator().manual_seed(53)
    pts = (torch.rand(R, S, 3, generator=gen) * 2 - 1) * 1.5
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    cot = torch.randn(R, S, 4, generator=gen)
    return pts, vd, cot


_REFERENCES = {}


class ReluTaking(torch.autograd.Function):
    """relu(z) whose backward takes the branch `branch` says (a bool per element) instead of z > 0."""

    @staticmethod
    def forward(ctx, z, branch):
        ctx.save_for_backward(branch)
        return torch.relu(z)

    @staticmethod
    def backward(ctx, grad):
        return grad * ctx.saved_tensors[0].to(grad.dtype), None


def reference(P, k):
    """Shape k in fp64 torch, once: (state dict, forward(params, branches) -> (output, the ReLU layers' pre-activations in
    the route's order: the trunk's, then the view layer's), output)."""
    if k in _REFERENCES:
        return _REFERENCES[k]
    F = torch.nn.functional
    shape = SHAPES[k]
    net, emb_fn, embd_fn = build(P, shape, "f16x3")
    sd = {n: v.detach().cpu().double() for n, v in net.state_dict().items()}
    pts, vd, _ = inputs()
    x = emb_fn(pts.reshape(-1, 3).double())
    v = embd_fn(vd[:, None].expand(R, S, 3).reshape(-1, 3).double()) if shape["Lv"] > 0 else None

    def forward(params, branches=None):
        pre, h = [], x

        def relu(z):
            pre.append(z)
            return F.relu(z) if branches is None else ReluTaking.apply(z, branches[len(pre) - 1])
        for i in range(shape["D"]):
            h = relu(F.linear(h, params[f"pts_linears.{i}.weight"], params[f"pts_linears.{i}.bias"]))
            if i in shape["skips"]:
                h = torch.cat([x, h], -1)
        if v is None:
            return F.linear(h, params["output_linear.weight"], params["output_linear.bias"]), pre
        sigma = F.linear(h, params["alpha_linear.weight"], params["alpha_linear.bias"])
        feat = F.linear(h, params["feature_linear.weight"], params["feature_linear.bias"])
        hv = relu(F.linear(torch.cat([feat, v], -1), params["views_linears.0.weight"], params["views_linears.0.bias"]))
        return torch.cat([F.linear(hv, params["rgb_linear.weight"], params["rgb_linear.bias"]), sigma], -1), pre
    with torch.no_grad():
        out, pre = forward(sd)
    _REFERENCES[k] = (sd, forward, out, [z.detach() for z in pre])
    return _REFERENCES[k]


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3", "f16", "bf16"])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=lambda k: "D{D}W{W}L{L}v{Lv}".format(**SHAPES[k]))
def test_networks_in_their_own_precision_against_fp64(P, honour, k, precision):
    """Through run_network (the reference's call), 777 rows: the forward within the mode's bound on the compiled trunk; in
    the split modes every parameter's gradient within 2e-4 of max |g|.  The backward runs in fp32 on the activations the
    16-bit forward wrote, so it takes a ReLU unit's branch from THAT forward: a unit (of one row) whose fp64 pre-activation
    lies inside the mode's forward error (flip_below) is legitimately undecided and is left out of the comparison -- the
    fp64 reference's backward takes, at exactly those units, the branch the GPU's forward took (read off the activations
    the route's ReLU layers returned); every other unit and every row stays in.  The share of such units is capped at 1 %
    of every layer's units x rows -- asserted on the fp64 pre-activations -- and printed."""
    from plnerf_amd import generic
    shape = SHAPES[k]
    sd, forward, ref, pre = reference(P, k)
    net, emb_fn, embd_fn = build(P, shape, precision)
    pts, vd, cot = inputs()
    use_viewdirs = shape["Lv"] > 0
    split = precision in FLIP_BELOW
    taken, found = [], generic.linear

    def recording(x, layer, relu, *rest):
        y = found(x, layer, relu, *rest)
        if relu:
            taken.append(y.detach() > 0)
        return y
    generic.linear = recording
    try:
        out = P.run_network(g(pts), g(vd) if use_viewdirs else None, net, emb_fn, embd_fn)
    finally:
        generic.linear = found
    assert out.shape == (R, S, ref.shape[-1])
    err = maxdiff(out.reshape(-1, ref.shape[-1]), ref.float())
    rel = err / (1.0 + float(ref.abs().max()))
    print(f"{precision} {shape}: forward error / (1 + max |ref|) {rel:.2e} (bound {FORWARD_TOL[precision]:g})")
    assert net.range_status() == 0
    assert rel <= FORWARD_TOL[precision], (precision, shape, rel)
    if not split:
        return
    assert len(taken) == len(pre) and all(t.shape == z.shape for t, z in zip(taken, pre))
    undecided = [z.abs() < FLIP_BELOW[precision] for z in pre]
    shares = [float(u.double().mean()) for u in undecided]
    flipped = sum(int((u & (t.cpu() != (z > 0))).sum()) for u, t, z in zip(undecided, taken, pre))
    decided_apart = sum(int((~u & (t.cpu() != (z > 0))).sum()) for u, t, z in zip(undecided, taken, pre))
    print(f"{precision} {shape}: undecided units per layer (share of units x rows) max {max(shares):.2e}; "
          f"{sum(int(u.sum()) for u in undecided)} units left out, {flipped} of them on the other branch; "
          f"{decided_apart} decided units on the other branch")
    assert max(shares) <= 0.01, shares
    branches = [torch.where(u, t.cpu(), z > 0) for u, t, z in zip(undecided, taken, pre)]
    leaves = {n: t.clone().requires_grad_(True) for n, t in sd.items()}
    (forward(leaves, branches)[0][:, :4] * cot.reshape(-1, 4).double()).sum().backward()
    (out[..., :4] * g(cot)).sum().backward()
    worst = 0.0
    for name, prm in net.named_parameters():
        r = leaves[name].grad
        if r is None:      # (views_linears without view directions: not on the path, as in the reference)
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0
            continue
        worst = max(worst, float((prm.grad.cpu().double() - r).abs().max()) / max(float(r.abs().max()), 1e-9))
    print(f"{precision} {shape}: worst gradient error / max |g| {worst:.2e}")
    assert worst <= GRAD_TOL, (precision, shape, worst)


def test_switch_off_is_the_fp32_route_bit_for_bit(P):
    """An f16x3 network of D = 9, W = 320: with the switch off its forward and gradients equal, bit for bit, those of the
    same weights in a precision="fp32" network; with it on the forward differs somewhere and agrees to f16x3's bound."""
    from plnerf_amd import generic
    assert generic.HONOUR_PRECISION is False
    shape = SHAPES[0]
    pts, vd, cot = inputs()
    net16, emb_fn, embd_fn = build(P, shape, "f16x3")
    net32, _, _ = build(P, shape, "fp32")
    net32.load_state_dict(net16.state_dict())

    def run(net):
        net.zero_grad()
        out = P.run_network(g(pts), g(vd), net, emb_fn, embd_fn)
        (out[..., :4] * g(cot)).sum().backward()
        return out.detach(), [p.grad.clone() for p in net.parameters()]
    out32, grads32 = run(net32)
    out16, grads16 = run(net16)
    assert same_bits(out16, out32) and all(torch.equal(a, b) for a, b in zip(grads16, grads32))
    with pytest.raises(NotImplementedError):
        net16.status_word()      # (no word without the switch, as before)
    generic.HONOUR_PRECISION = True
    try:
        on, _ = run(net16)
        again, _ = run(net32)      # (an fp32 network ignores the switch)
    finally:
        generic.HONOUR_PRECISION = False
    assert same_bits(again, out32)
    assert not torch.equal(on, out32)
    assert maxdiff(on, out32) <= FORWARD_TOL["f16x3"] * (1.0 + float(out32.abs().max()))


def _train_step(P, precision):
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "exp"))
    args = nvs_args(d, precision, N_rand=64, netwidth=320, netwidth_fine=320, N_samples=16, N_importance=16)
    torch.manual_seed(5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        kw, _, start, _, opt, opt_c = P.create_nerf(args, device=dev())
    told = [str(w.message) for w in caught if "layer by layer" in str(w.message)]
    assert len(told) == 2 and all(f"precision={precision!r}" in m and "backward in fp32" in m for m in told), told
    ts = P.TrainStep(args, kw, opt, opt_c, start=start, distributed=False, seed=3, range_check_every=0)
    return ts, kw, opt, opt_c


def _one_step(P, ts):
    H, W = 20, 26
    gen = torch.Generator().manual_seed(11)
    image = g(torch.rand(H, W, 3, generator=gen))
    K = [[1.3 * W, 0, W / 2], [0, 1.3 * W, H / 2], [0, 0, 1]]
    c2w = P.rays.pose_spherical(30.0, -30.0, 4.0)
    return ts.step_view(H, W, K, c2w, image, near=2.0, far=6.0, n_rand=64)


def test_a_clamped_forward_withholds_the_step(P, honour):
    """create_nerf with netwidth 320 and the switch on: one first-layer weight scaled (inside the half range) so that an
    activation passes 65,504.  f16x3: the step is withheld by both optimizers, the weights stay, check_range() names an
    activation.  bf16x3 (fp32's exponent range, no half saved planes on this route): the step applies."""
    for precision, clamps in (("f16x3", True), ("bf16x3", False)):
        ts, kw, opt, opt_c = _train_step(P, precision)
        coarse, fine = kw["network_fn"], kw["network_fine"]
        assert not coarse.is_supported() and not fine.is_supported()
        with torch.no_grad():
            coarse.pts_linears[0].weight[0, :3] = torch.tensor([6.0e4, 6.0e4, 6.0e4], device=dev())
            coarse.pts_linears[1].weight[:, 0] *= 1.0e-5      # (back to O(1) behind it)
        before = [p.detach().clone() for n in (coarse, fine) for p in n.parameters()]
        loss, _ = _one_step(P, ts)
        torch.cuda.synchronize()
        after = [p.detach() for n in (coarse, fine) for p in n.parameters()]
        if clamps:
            assert opt.withheld_steps() == 1 and opt_c.withheld_steps() == 1
            assert all(torch.equal(a, b) for a, b in zip(before, after))
            assert coarse.range_status() == P._lib.RANGE_ACTIVATION and fine.range_status() == 0
            with pytest.raises(FloatingPointError, match="an activation exceeded the IEEE-half range"):
                ts.check_range()
            assert coarse.range_status() == 0
        else:
            assert bool(torch.isfinite(loss))
            assert coarse.range_status() == 0 and fine.range_status() == 0
            ts.check_range()
            assert opt.withheld_steps() == 0 and opt_c.withheld_steps() == 0
            assert any(not torch.equal(a, b) for a, b in zip(before, after))


VIEW_H, VIEW_W = 16, 24
VIEW_SAMPLING = dict(N_samples=16, N_importance=16, mode="linear", color_mode="midpoint", perturb=0.0, white_bkgd=True,
                     raw_noise_std=0.0)


def _carve_half_space(net, normal=(0.4, 0.2, 1.0), offset=1.93, gain=40.0, floor=-3.0):
    """Give a torch-initialised D = 8, W = 320 network a scene with empty space in it: unit 0 of every trunk layer carries
    relu(normal . x - offset) forward unchanged, and the density is gain * that + floor + (the other units' small share):
    negative -- exactly zero after the renderer's relu -- outside the half space, in every arithmetic."""
    with torch.no_grad():
        for i, fc in enumerate(net.pts_linears):
            fc.weight[0, :] = 0.0
            fc.bias[0] = 0.0
            if i == 0:
                fc.weight[0, :3] = torch.tensor(normal, device=fc.weight.device)
                fc.bias[0] = -offset
            else:      # (behind a skip the encoding's channels come first)
                fc.weight[0, net.input_ch if (i - 1) in net.skips else 0] = 1.0
        net.alpha_linear.weight[0, 0] = gain
        net.alpha_linear.bias[0] = floor


def _view(P):
    K = [[1.3 * VIEW_W, 0, VIEW_W / 2], [0, 1.3 * VIEW_W, VIEW_H / 2], [0, 0, 1]]
    return K, P.rays.pose_spherical(40.0, -25.0, 4.0)[:3, :4]


def _view_networks(P):
    shape = dict(D=8, W=320, skips=[4], L=10, Lv=4)
    net_c, emb_fn, embd_fn = build(P, shape, "f16x3", seed=61)
    net_f, _, _ = build(P, shape, "f16x3", seed=62)
    _carve_half_space(net_c)
    _carve_half_space(net_f)
    return net_c, net_f, emb_fn, embd_fn


def _differing(z_a, z_b):
    """Per ray: do the importance samples differ in any bit (as fp32)."""
    z_a, z_b = z_a.detach().cpu().float().contiguous(), z_b.detach().cpu().float().contiguous()
    return ~(z_a.view(torch.int32) == z_b.view(torch.int32)).all(-1)


def test_render_of_a_small_view(P, honour):
    """24 x 16 pixels at 16 + 16 samples through a W = 320 pair in f16x3, switch on against switch off (the fp32 route): the
    final maps within G5's final tolerance on every ray whose importance samples agree bit for bit; the share of the other
    rays is printed and capped at 5 %.

    An importance sample is the inverse of a cdf that is continuous in the network's output: two arithmetics whose outputs
    differ in the last bits give samples that differ in the last bits on every ray that meets density (torch-initialised
    networks, whose density is non-zero almost everywhere, measured 296 of 384 rays).  Only a ray whose coarse weights are
    exactly zero in both has bit-equal samples, so the scene is built to have empty space (_carve_half_space): density only
    beyond a plane that 15 of the 384 rays (3.9 %) reach.  The scene is fixed by this check, made first and on the CPU: the
    fp32 route's own restatement in oracle/ (the oracle's MLP takes any width at D = 8 with the skip after layer 4) in
    fp32 against the same in fp64 differs on 10 of the 384 rays, under the cap, and sees density on at least one ray.

    Beyond what the issue asks: the coarse maps within the contract on every ray, and the final maps within the same
    tolerance on the rays where the sampler chose the same intervals (its search indices agree) -- the rays that do meet
    density, which the bitwise criterion leaves out."""
    import sys
    from oracle import plnerf_oracle as orc
    Rn = sys.modules[P.render.__module__]      # (the module: the package attribute `render` is the function)
    H, W = VIEW_H, VIEW_W
    net_c, net_f, emb_fn, embd_fn = _view_networks(P)
    K, c2w = _view(P)
    # -- the CPU check of the scene: oracle fp32 against oracle fp64
    sd_c, sd_f = ({k: v.detach().cpu() for k, v in n.state_dict().items()} for n in (net_c, net_f))
    o, d = orc.get_rays(H, W, torch.tensor(K), torch.as_tensor(c2w).float())
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    batch = torch.cat([o, d, torch.full((H * W, 1), 2.0), torch.full((H * W, 1), 6.0), d / d.norm(dim=-1, keepdim=True)], -1)
    with torch.no_grad():
        r32, i32 = orc.render_rays(batch, sd_c, sd_f, return_internals=True, **VIEW_SAMPLING)
        r64, i64 = orc.render_rays(batch.double(), {k: v.double() for k, v in sd_c.items()},
                                   {k: v.double() for k, v in sd_f.items()}, return_internals=True, **VIEW_SAMPLING)
    assert i64["z_samples"].dtype == torch.float64
    cpu_share = float(_differing(i32["z_samples"], i64["z_samples"]).double().mean())
    dense = int((r64["acc0"] > 0).sum())
    print(f"oracle fp32 against fp64: importance samples differ on {cpu_share:.2%} of the rays; {dense} rays meet density")
    assert cpu_share <= 0.05 and dense > 0, (cpu_share, dense)
    # -- the GPU: switch on against switch off
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)
    kw = dict(VIEW_SAMPLING, network_query_fn=qfn, network_fn=net_c, network_fine=net_f, use_viewdirs=True, ndc=False)

    def run():
        with torch.no_grad(), stage_tap(Rn) as tap:
            rgb, disp, acc, extras = P.render(H, W, K, chunk=32768, c2w=g(c2w), near=2.0, far=6.0, **kw)
        maps = dict(extras, rgb_map=rgb.reshape(-1, 3), disp_map=disp.reshape(-1), acc_map=acc.reshape(-1))
        return ({k: v.reshape(H * W, -1) for k, v in maps.items() if torch.is_tensor(v)}, tap["z_samples"].reshape(H * W, -1),
                tap["inds"].reshape(H * W, -1))
    on, z_on, i_on = run()
    honour.HONOUR_PRECISION = False
    off, z_off, i_off = run()
    honour.HONOUR_PRECISION = True
    assert net_c.range_status() == 0 and net_f.range_status() == 0
    differing = _differing(z_on, z_off)
    share = float(differing.double().mean())
    met = int((off["acc0"] > 0).any(-1).sum())
    print(f"render W=320 f16x3 on/off: importance samples differ in some bit on {int(differing.sum())} of {H * W} rays "
          f"({share:.2%}); {met} rays meet density")
    assert share <= 0.05, share
    assert met > 0 and not torch.equal(on["rgb0"], off["rgb0"])      # (the scene is not empty, and the 16-bit route did run)
    tol, tol_std = G5_FINAL_TOL
    for rays, what in ((~differing, "bit-equal samples"), ((i_on == i_off).all(-1).cpu(), "equal intervals")):
        for k in ("rgb_map", "acc_map", "depth_map"):
            assert_close(on[k][rays], off[k][rays], atol=tol, rtol=tol, what=f"final {k}, {what}")
        assert_close(on["z_std"][rays], off["z_std"][rays], atol=tol_std, rtol=tol_std, what=f"z_std, {what}")
    for k in ("rgb0", "acc0", "depth0"):
        assert_close(on[k], off[k], what=f"coarse {k}")


