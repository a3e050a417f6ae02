"""plnerf_generic_fwd_f32 and plnerf_render_view_any (include/experimental/plnerf_hip_anyview.h) on a real MI355X, and their
host side (plnerf_amd.anyview, render_path_frames, evaluate.render_images_with_metrics(one_call=True)).

Every bound here is exact.  The fp32 layer loop against generic.forward with its switches off; AnyViewRenderer's nine planes
against render() under DrawSource(seed, 0, step) for a device pose, over the four kinds of pair (a slot on the fused trunk, a
16-bit chain, fp32 layers) and both modes, both colour modes, jitter, density noise and NDC; the frame's independence of the
block, of max_net_rows and of how the pixel range is split; two fused slots against plnerf_render_view; a sentinel arena around
every buffer; the range status of a 16-bit chain; the frame files; the metric rows; and tests/c_abi_anyview_gpu.cpp, which
renders a mixed pair without Python.

The networks outside the trunk are the cheapest that really are: netdepth 9 at netwidth 72 (skip behind layer 4) and netdepth 4
at netwidth 40 with live skips behind layers 0 and 2.  Frames are 5 x 9 in blocks of 16 pixels (16, 16, 13) with 8 + 8 samples
and max_net_rows = 100, so the network calls cut inside a ray."""
import contextlib
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import arena as A
import c_hosts
from gpu_support import P, counting_calls, dev, g, make_net, same_bits, scene
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu
PLANES = ("rgb", "disp", "acc", "depth", "rgb0", "disp0", "acc0", "depth0", "z_std")
SHAPES = {"deep": dict(D=9, W=72, skips=[4]), "skips": dict(D=4, W=40, skips=[0, 2])}
H_VIEW, W_VIEW, CHUNK, NS, NI, NET_ROWS = 5, 9, 16, 8, 8, 100
LAYERS32 = 2      # PLNERF_ANYVIEW_LAYERS32 (_lib.ANYVIEW_LAYERS32)
K_VIEW = [[11.3, 0, 4.1], [0, 9.7, 2.6], [0, 0, 1]]


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


@contextlib.contextmanager
def honouring(on=True):
    """generic.HONOUR_PRECISION set for the block (a network outside the trunk then runs in its own 16-bit precision)."""
    from plnerf_amd import generic
    found, generic.HONOUR_PRECISION = generic.HONOUR_PRECISION, on
    try:
        yield
    finally:
        generic.HONOUR_PRECISION = found


def _generic_net(P, shape, precision="fp32", seed=47, use_viewdirs=True, L=10, M=4):
    """A network outside the compiled trunk with nn.Linear's initial weights under `seed` (and a density that is not all
    clamped away: the importance samples then have something to follow)."""
    torch.manual_seed(seed)
    net = P.NeRF(D=shape["D"], W=shape["W"], input_ch=3 + 6 * L, input_ch_views=3 + 6 * M, output_ch=5, skips=shape["skips"],
                 use_viewdirs=use_viewdirs, precision=precision).to(dev())
    assert not net.is_supported()
    if use_viewdirs:
        with torch.no_grad():
            net.alpha_linear.bias.fill_(0.75)
    return net


def _fused_net(P, which, precision):
    return make_net(P, orc.closed_form_state_dict(which, False), precision)


def _kwargs(P, coarse, fine, **over):
    """What create_nerf hands render() for this pair: the query function names its encoders."""
    emb, embd = P.get_embedder(10, 0)[0], P.get_embedder(4, 0)[0]

    def query(inputs, viewdirs, fn):
        return P.run_network(inputs, viewdirs, fn, emb, embd, netchunk=1 << 16)
    query.embedders = (emb, embd)
    kw = dict(network_fn=coarse, network_fine=fine, network_query_fn=query, N_samples=NS, N_importance=NI, use_viewdirs=True,
              mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=0.0, lindisp=False)
    kw.update(over)
    return kw


def _pose(forward_facing=False):
    """A generic rotation with a translation, or a camera that looks down -z with a small tilt ([3,4] fp32, host)."""
    import plnerf_amd as P_
    if not forward_facing:
        c2w = P_.rays.pose_spherical(40.0, -30.0, 4.0)[:3, :4].clone()
        c2w[:, 3] += torch.tensor([0.3, -0.2, 0.1])
        return c2w
    a, b = 0.07, -0.05      # a small tilt about x and y: the camera still looks down -z
    rx = torch.tensor([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], dtype=torch.float64)
    ry = torch.tensor([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]], dtype=torch.float64)
    return torch.cat([ry @ rx, torch.tensor([[0.1], [-0.05], [0.2]], dtype=torch.float64)], 1).float()


def _reference_frame(P, kw, H, W, K, c2w, chunk, near, far, seed, step, ndc=False):
    from plnerf_amd import functional as Fn
    prev = Fn.set_draw_source(Fn.DrawSource(seed, 0, step))
    try:
        with torch.no_grad():
            rgb, disp, acc, extras = P.render(H, W, K, chunk=chunk, c2w=g(c2w), near=near, far=far, ndc=ndc, **kw)
    finally:
        Fn.set_draw_source(prev)
    return {"rgb": rgb, "disp": disp, "acc": acc, "depth": extras["depth_map"], "rgb0": extras["rgb0"], "disp0": extras["disp0"],
            "acc0": extras["acc0"], "depth0": extras["depth0"], "z_std": extras["z_std"]}


def _frame(vr, c2w, step, export=False):
    rgb, disp, acc, extras = vr.render(c2w, step=step, export=export)
    out = {"rgb": rgb, "disp": disp, "acc": acc, "depth": extras["depth_map"], "rgb0": extras["rgb0"], "disp0": extras["disp0"],
           "acc0": extras["acc0"], "depth0": extras["depth0"], "z_std": extras["z_std"]}
    return out, extras


# ----------------------------------------------------------------------------- 1. the fp32 layer loop
def _fwd_f32(net, wide, cols, ld_out_pad=3, sentinel=777.0):
    """plnerf_generic_fwd_f32 on rows given through a stride wider than the row, into a sentinel-filled output with columns
    behind the result, on a workspace of the query's exact size filled with NaN bytes.  Returns (out, the whole buffer)."""
    from plnerf_amd import _lib as L, generic
    n = wide.shape[0]
    shape = generic._describe(net, wide[:, :cols])[0]
    tensors, table = generic._param_table([t for fc in generic._layers(net) for t in (fc.weight, fc.bias)])
    width = 4 if net.use_viewdirs else shape.output_ch
    out = torch.full((n, width + ld_out_pad), sentinel, device=dev())
    nbytes = L.lib().plnerf_generic_fwd_f32_workspace_bytes(ctypes.byref(shape), n)
    assert nbytes > 0
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=dev())
    L.check(L.lib().plnerf_generic_fwd_f32(ctypes.byref(shape), table, ctypes.c_void_p(wide.data_ptr()), wide.stride(0), n,
                                           ctypes.c_void_p(ws.data_ptr()), nbytes, L.dptr(out), out.stride(0), L.stream()),
            "plnerf_generic_fwd_f32")
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0xFF).all()      # nothing behind the bytes the query asked for
    del tensors
    return out[:, :width], out


@functools.lru_cache(maxsize=None)
def _layer_loop_net(kind):
    import plnerf_amd as P_
    if kind == "plain":
        return _generic_net(P_, SHAPES["deep"], use_viewdirs=False, seed=5)
    if kind == "wide":
        return _generic_net(P_, dict(D=2, W=1024, skips=[]), seed=6)
    return _generic_net(P_, SHAPES[kind], seed=7)


@pytest.mark.parametrize("kind,n", [(k, n) for k in ("deep", "skips", "plain") for n in (1, 63, 65, 200)] + [("wide", 70)])
def test_fp32_layer_loop_is_generic_forward(P, kind, n):
    """Both shapes off the trunk, a network without view directions (output_ch 5) and D = 2, W = 1024 at 70 rows, where
    generic._splits deals the second layer's k range over two workgroups: bit for bit generic.forward with its switches off."""
    from plnerf_amd import generic
    net = _layer_loop_net(kind)
    cols = net.input_ch + net.view_ch
    gen = torch.Generator().manual_seed(100 + n)
    wide = g(torch.rand(n, cols + 5, generator=gen) * 2 - 1)
    if kind == "wide":
        assert generic._splits(n, 1024, 1024) == 2
    assert not generic.HONOUR_PRECISION and not generic.CHAIN_INFERENCE
    with torch.no_grad():
        ref = generic.forward(net, wide[:, :cols])
    got, whole = _fwd_f32(net, wide, cols)
    assert got.shape == ref.shape == (n, 4 if net.use_viewdirs else 5)
    assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert (whole[:, ref.shape[1]:] == 777.0).all()      # the columns behind ld_out's result are untouched


# ----------------------------------------------------------------------------- 2. frames against render()
def _pair(P, name):
    """(coarse, fine, whether generic.HONOUR_PRECISION is on, the routes expected)."""
    from plnerf_amd import _lib as L
    F, C16, L32 = L.ANYVIEW_FUSED, L.ANYVIEW_CHAIN16, L.ANYVIEW_LAYERS32
    if name == "fused_chain16":
        return _fused_net(P, 0, "f16x3"), _generic_net(P, SHAPES["deep"], "f16x3", seed=11), True, (F, C16)
    if name == "chain16_fused":
        return _generic_net(P, SHAPES["skips"], "bf16x3", seed=12), _fused_net(P, 1, "f16x3"), True, (C16, F)
    if name == "layers32_layers32":
        return _generic_net(P, SHAPES["deep"], "fp32", seed=13), _generic_net(P, SHAPES["skips"], "fp32", seed=14), False, (L32, L32)
    assert name == "fused_layers32"      # the default-switch case of a mixed pair: the fine network's f16x3 is not honoured
    return _fused_net(P, 0, "f16x3"), _generic_net(P, SHAPES["deep"], "f16x3", seed=15), False, (F, L32)


CASES = {
    "linear_midpoint_jitter_noise": (dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=0.5), False, 2.0, 6.0),
    "linear_left_u_vals": (dict(mode="linear", color_mode="left", perturb=0.0, white_bkgd=False), False, 2.0, 6.0),
    "constant_jitter_noise": (dict(mode="constant", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=1.0), False, 2.0, 6.0),
    "ndc": (dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=False), True, 0.0, 1.0),
}


@pytest.mark.parametrize("pair,case", [("fused_chain16", "linear_midpoint_jitter_noise"), ("fused_chain16", "constant_jitter_noise"),
                                       ("chain16_fused", "linear_left_u_vals"), ("chain16_fused", "linear_midpoint_jitter_noise"),
                                       ("layers32_layers32", "constant_jitter_noise"), ("layers32_layers32", "linear_left_u_vals"),
                                       ("fused_layers32", "ndc"), ("fused_layers32", "linear_midpoint_jitter_noise")])
def test_any_view_equals_render(P, pair, case):
    coarse, fine, honour, routes = _pair(P, pair)
    over, forward_facing, near, far = CASES[case]
    kw = _kwargs(P, coarse, fine, **over)
    c2w, seed, step = _pose(forward_facing), 9, 4
    with honouring(honour):
        ref = _reference_frame(P, kw, H_VIEW, W_VIEW, K_VIEW, c2w, CHUNK, near, far, seed, step, ndc=forward_facing)
        assert not P.ViewRenderer.supported(kw) and P.AnyViewRenderer.supported(kw)
        vr = P.AnyViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, CHUNK, near, far, ndc=forward_facing, seed=seed, max_net_rows=NET_ROWS)
        assert vr.routes == routes
        got, extras = _frame(vr, c2w, step)
        assert set(extras) == {"rgb0", "disp0", "acc0", "depth0", "depth_map", "z_std"}
        for name in PLANES:
            assert got[name].shape == ref[name].shape and (name.startswith("disp") or torch.isfinite(ref[name]).all()), name
            assert same_bits(got[name], ref[name]), (pair, case, name, float((got[name] - ref[name]).abs().max()))
        assert float(ref["acc"].max()) > 0 and float(ref["rgb"].std()) > 0      # (not an empty frame)
        words = vr.status_words()
        assert [w is None for w in words] == [r == LAYERS32 for r in routes]      # exact fp32 has no range to leave
        assert all(int(w.item()) == 0 for w in words if w is not None)
        assert vr.current()
    if honour:      # the switch is part of the route: switched off, the renderer no longer describes what render() would do
        assert not vr.current()
        with pytest.raises(RuntimeError, match="AnyViewRenderer: the networks' parameters moved"):
            vr.enqueue(c2w, step=step)


# ----------------------------------------------------------------------------- 3. independence
def _snapshot(vr):
    return {k: v.clone() for k, v in vr.planes.items()}, vr.rgb8.clone(), vr.depth16.clone()


def _same_frames(a, b):
    return all(same_bits(a[0][k], b[0][k]) for k in PLANES) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_frame_does_not_depend_on_blocks_rows_or_calls(P):
    coarse, fine, honour, _ = _pair(P, "fused_chain16")
    kw = _kwargs(P, coarse, fine, **CASES["linear_midpoint_jitter_noise"][0])
    c2w, step, n = _pose(), 2, H_VIEW * W_VIEW
    with honouring(honour):
        frames = []
        for chunk, rows in ((16, 100), (45, 100), (16, 1 << 21), (45, 1 << 21), (16, 7)):
            vr = P.AnyViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, chunk, 2.0, 6.0, seed=3, max_net_rows=rows)
            vr.render(c2w, step=step, export=True)
            frames.append(_snapshot(vr))
        assert all(_same_frames(f, frames[0]) for f in frames[1:])
        vr.render(c2w, step=step, export=True)                       # rendered twice
        assert _same_frames(_snapshot(vr), frames[0])
        vr.render(c2w, step=step + 1, export=True)                   # (another step is another frame)
        assert not torch.equal(vr.planes["rgb"], frames[0][0]["rgb"])

        # two calls over [0, 20) and [20, 45) are one call; a call touches no pixel outside its range
        vr = P.AnyViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, 16, 2.0, 6.0, seed=3, max_net_rows=100)
        for v in vr.planes.values():
            v.fill_(777.0)
        vr.rgb8.fill_(0xA5)
        vr.depth16.fill_(0x5A5A)
        vr.enqueue(c2w, step=step, export=True, pix0=20, n_pix=25)
        planes, rgb8, depth16 = _snapshot(vr)
        inside = torch.zeros(n, dtype=torch.bool, device=dev())
        inside[20:] = True
        for k in PLANES:
            assert same_bits(planes[k][inside], frames[0][0][k][inside]) and (planes[k][~inside] == 777.0).all(), k
        assert (rgb8[~inside] == 0xA5).all() and (depth16[~inside] == 0x5A5A).all()
        vr.enqueue(c2w, step=step, export=True, pix0=0, n_pix=20)
        assert _same_frames(_snapshot(vr), frames[0])


# ----------------------------------------------------------------------------- 4. the tie to plnerf_render_view
def test_two_fused_slots_are_render_view(P):
    coarse, fine = _fused_net(P, 0, "f16x3"), _fused_net(P, 1, "f16x3")
    kw = _kwargs(P, coarse, fine, **CASES["linear_midpoint_jitter_noise"][0])
    c2w = _pose()
    assert P.ViewRenderer.supported(kw) and P.AnyViewRenderer.supported(kw)
    one = P.ViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, CHUNK, 2.0, 6.0, seed=9)
    any_ = P.AnyViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, CHUNK, 2.0, 6.0, seed=9, max_net_rows=NET_ROWS)
    assert any_.workspace_bytes == one.workspace_bytes
    with counting_calls() as lib:
        one.render(c2w, step=4, export=True)
        any_.render(c2w, step=4, export=True)
    assert [c for c in lib.calls if "render_view" in c] == ["plnerf_render_view", "plnerf_render_view_any"]
    a, b = _snapshot(one), _snapshot(any_)
    for k in PLANES:
        assert torch.equal(a[0][k].view(torch.uint8), b[0][k].view(torch.uint8)), k
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(torch.unique(a[1])) > 1 and len(torch.unique(a[2])) > 1


# ----------------------------------------------------------------------------- 5. containment
def test_every_buffer_is_written_inside_its_bytes(P):
    """Planes, export planes and workspace of exact size, carved from a sentinel arena; two planes left NULL; the workspace
    once at 0x00 and once at 0xFF; then a refused call, which touches nothing."""
    from plnerf_amd import _lib as L
    coarse, fine, honour, _ = _pair(P, "fused_chain16")
    kw = _kwargs(P, coarse, fine, **CASES["linear_midpoint_jitter_noise"][0])
    c2w, n = _pose(), H_VIEW * W_VIEW
    left_out = ("disp0", "z_std")
    with honouring(honour):
        vr = P.AnyViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, CHUNK, 2.0, 6.0, seed=9, max_net_rows=NET_ROWS)
        vr.render(c2w, step=4, export=True)
        want = _snapshot(vr)
        sizes = {name: n * (3 if name in ("rgb", "rgb0") else 1) * 4 for name in PLANES if name not in left_out}
        results = []
        for ws_byte in (0x00, 0xFF):
            arena = A.Arena(dev(), sum(A.Arena.room(b) for b in list(sizes.values()) + [3 * n, 2 * n, vr.workspace_bytes]) + A.MIN_GUARD)
            bufs = {name: arena.carve(name, nbytes, align=4) for name, nbytes in sizes.items()}
            rgb8, depth16 = arena.carve("rgb8", 3 * n, align=1), arena.carve("depth16", 2 * n, align=2)
            ws = arena.carve("workspace", vr.workspace_bytes, align=256, role="scratch")
            ws.set_bytes(ws_byte)
            io = vr.io
            for name in PLANES:
                setattr(io, name, bufs[name].dptr if name in bufs else None)
            vr._aim(c2w, 4, True, 0, None)
            io.rgb8, io.depth16 = rgb8.dptr, depth16.dptr
            refs = (ctypes.byref(vr.config), ctypes.byref(io), ctypes.byref(vr.args), ctypes.c_void_p(ws.dptr), vr.workspace_bytes, L.stream())
            L.check(L.lib().plnerf_render_view_any(*refs), "plnerf_render_view_any")
            torch.cuda.synchronize()
            arena.check()
            for name, buf in bufs.items():
                assert torch.equal(buf.u8(), want[0][name].reshape(-1).view(torch.uint8)), (name, ws_byte)
            assert torch.equal(rgb8.u8(), want[1].reshape(-1)) and torch.equal(depth16.u8(), want[2].view(torch.uint8).reshape(-1))
            results.append(arena)
        # a refused call (the pixel range leaves the view) enqueues nothing: every buffer keeps what it held
        arena = results[-1]
        before = arena.mem.clone()
        vr.args.pix0, vr.args.n_pix = 40, 6
        assert L.lib().plnerf_render_view_any(*refs) == -3
        vr.args.pix0, vr.args.n_pix = 0, n
        assert L.lib().plnerf_render_view_any(refs[0], refs[1], refs[2], refs[3], vr.workspace_bytes - 1, refs[5]) == -1
        torch.cuda.synchronize()
        assert torch.equal(arena.mem, before)


# ----------------------------------------------------------------------------- 6. the range status of a 16-bit chain
def test_a_chain16_network_reports_its_range(P):
    """One weight beyond 65,504 in an f16x3 network outside the trunk: plnerf_generic_fwd packs it clamped and raises the
    weight bit in the network's own status word; the renderer's check names that network.  (A clamped value; no fault.)"""
    from plnerf_amd import _lib as L
    coarse = _fused_net(P, 0, "f16x3")
    fine = _generic_net(P, SHAPES["deep"], "f16x3", seed=21)
    with torch.no_grad():
        fine.pts_linears[3].weight[5, 7] = 70000.0
    kw = _kwargs(P, coarse, fine, **CASES["linear_left_u_vals"][0])
    c2w = _pose()
    with honouring(True):
        fine.status_word().zero_()
        vr = P.AnyViewRenderer(kw, H_VIEW, W_VIEW, K_VIEW, CHUNK, 2.0, 6.0, seed=9, max_net_rows=NET_ROWS)
        vr.enqueue(c2w, step=1)
        torch.cuda.synchronize()
        assert int(fine.status_word().item()) & L.RANGE_WEIGHT
        assert vr.status_words()[1].data_ptr() == fine.status_word().data_ptr() and int(vr.status_words()[0].item()) == 0
        with pytest.raises(FloatingPointError, match=r"the fine network \(chain16\).*precision='f16x3'"):
            vr.check_range()
        assert int(fine.status_word().item()) == 0      # (read and cleared)
        with pytest.raises(FloatingPointError, match=r"the fine network \(chain16\)"):
            vr.render(c2w, step=1)
        # render() raises the same way: the layered route ORs the same bit into the same word
        _reference_frame(P, kw, H_VIEW, W_VIEW, K_VIEW, c2w, CHUNK, 2.0, 6.0, 9, 1)
        assert int(fine.status_word().item()) & L.RANGE_WEIGHT
        with pytest.raises(FloatingPointError, match="a weight"):
            fine.check_range()


# ----------------------------------------------------------------------------- 7. frame files
def test_render_path_frames_serves_a_generic_fine_network(P, tmp_path):
    """On the parent commit this is ViewRenderer's ValueError."""
    H, W, focal = 6, 8, 10.0
    K = [[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]]
    coarse, fine, _, _ = _pair(P, "fused_layers32")
    kw = _kwargs(P, coarse, fine, near=2.0, far=6.0, ndc=False, **CASES["linear_midpoint_jitter_noise"][0])
    poses = torch.stack([P.rays.pose_spherical(th, -30.0, 4.0) for th in (20.0, 75.0)], 0)
    savedir = tmp_path / "frames"
    with counting_calls() as lib:
        rgbs, disps = P.render_path_frames(poses, (H, W, focal), K, CHUNK, kw, savedir=str(savedir), seed=6, max_net_rows=NET_ROWS)
    assert lib.calls.count("plnerf_render_view_any") == 2 and "plnerf_render_view" not in lib.calls
    assert rgbs.shape == (2, H, W, 3) and disps.shape == (2, H, W) and rgbs.dtype == np.float32
    assert sorted(os.listdir(str(savedir))) == ["000.png", "001.png"]
    render_kw = {k: v for k, v in kw.items() if k not in ("near", "far", "ndc")}
    for i in range(2):
        ref = _reference_frame(P, render_kw, H, W, K, poses[i, :3, :4], CHUNK, 2.0, 6.0, 6, i)
        assert np.array_equal(rgbs[i], ref["rgb"].cpu().numpy()) and np.array_equal(disps[i], ref["disp"].cpu().numpy(), equal_nan=True)
        decoded = P.read_png(str(savedir / f"{i:03d}.png"))
        assert decoded.dtype == np.uint8 and np.array_equal(decoded, to8b(ref["rgb"].cpu().numpy()))
    assert not np.array_equal(rgbs[0], rgbs[1])


# ----------------------------------------------------------------------------- 8. metrics
@pytest.mark.parametrize("pair", ["fused_fused", "fused_layers32"])
def test_metrics_one_call_gives_the_same_rows(P, pair):
    from plnerf_amd import evaluate
    if pair == "fused_fused":
        coarse, fine, entry = _fused_net(P, 0, "f16x3"), _fused_net(P, 1, "f16x3"), "plnerf_render_view"
    else:
        coarse, fine, _, _ = _pair(P, pair)
        entry = "plnerf_render_view_any"
    H, W = 7, 8      # (the SSIM window is 7 x 7)
    poses, images, K_ulp = scene(P, 2, H, W)
    # The entries hold the focal lengths as fp32 and multiply by 1.0f / f; torch's device kernels, which render() builds its
    # rays with, multiply by float(1.0 / f) of the Python float.  The rows can be render()'s only where the two are one number:
    # 11.3 and 9.7 (K_VIEW) are such focal lengths, the scene's own 1.3 W + 0.37 = 10.77 is not -- that K keeps render() (below).
    K = K_VIEW
    assert evaluate.entry_rays_are_renders(K) and not evaluate.entry_rays_are_renders(K_ulp)
    assert np.float32(1.0 / K_ulp[0][0]) != np.float32(1.0) / np.float32(K_ulp[0][0])
    kw =_kwargs(P, coarse, fine, near=2.0, far=6.0, ndc=False, mode="linear", color_mode="midpoint", perturb=0.0, white_bkgd=True)
    args = types.SimpleNamespace(dataset="blender", chunk=CHUNK)
    call = functools.partial(evaluate.render_images_with_metrics, None, [0, 1], g(images), None, None, g(poses), H, W, K, None, args, kw)
    with counting_calls() as lib:
        default, res = call()
    assert entry not in lib.calls and "plnerf_render_view_any" not in lib.calls
    with counting_calls() as lib:
        one, res_one = call(one_call=True)
    assert lib.calls.count(entry) == 2
    a, b = default.as_dict(), one.as_dict()
    assert set(a) == set(b) >= {"img_loss", "psnr", "ssim", "img_loss0", "psnr0"}
    assert all(a[k] == b[k] for k in a), (a, b)
    for k in res:
        assert torch.equal(res[k], res_one[k]), k
    # kwargs that ask for draws keep render(), silently
    with counting_calls() as lib:
        evaluate.render_images_with_metrics(1, [0, 1], g(images), None, None, g(poses), H, W, K, None, args, dict(kw, perturb=1.0),
                                            keep_images=False, one_call=True)
    assert entry not in lib.calls and "plnerf_render_view_any" not in lib.calls
    # so do intrinsics at which the entries' rays are an ulp from render()'s: the rows stay render()'s there too
    call = functools.partial(evaluate.render_images_with_metrics, None, [0, 1], g(images), None, None, g(poses), H, W, K_ulp, None,
                             args, kw, keep_images=False)
    with counting_calls() as lib:
        one, _ = call(one_call=True)
    assert entry not in lib.calls and "plnerf_render_view_any" not in lib.calls
    a, b = call()[0].as_dict(), one.as_dict()
    assert set(a) == set(b) and all(a[k] == b[k] for k in a), (a, b)


# ----------------------------------------------------------------------------- 9. a host without Python
def test_c_host_renders_a_mixed_pair_without_python(P, tmp_path):
    """tests/c_abi_anyview_gpu.cpp -- the HIP runtime and include/experimental/plnerf_hip_anyview.h, nothing else -- renders a
    6 x 10 view three ways and checks them byte-identical itself; AnyViewRenderer on the same hashed weights and pose produces
    the same bytes."""
    from plnerf_amd import _lib as L_
    from plnerf_amd.view import depth16_numpy
    exe = c_hosts.build("c_abi_anyview_gpu", tmp_path)
    IMG_H, IMG_W = 6, 10
    run = c_hosts.run(exe, L_.PRECISION["f16x3"], L_.FWD_KERNEL, c_hosts.write_tables(tmp_path / "tables.bin", NS, NI))
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    host = c_hosts.parse_planes(run.stdout)
    assert set(host) == {"rgb8", "rgb", "depth16"}

    coarse = _fused_net(P, 0, "f16x3")
    coarse.load_state_dict(c_hosts.hashed_state_dict(0, orc.param_shapes()))
    fine = _generic_net(P, SHAPES["deep"], "fp32", seed=1)
    fine.load_state_dict(c_hosts.hashed_state_dict(1, [(name, tuple(v.shape)) for name, v in fine.state_dict().items()]))
    kw = _kwargs(P, coarse, fine, mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=0.0)
    K = [[20.0, 0, 0.5 * IMG_W], [0, 21.0, 0.5 * IMG_H], [0, 0, 1]]
    c2w = torch.tensor([[1.0, 0, 0, 0.1], [0, 1.0, 0, -0.2], [0, 0, 1.0, 4.0]])
    vr = P.AnyViewRenderer(kw, IMG_H, IMG_W, K, 16, 2.0, 6.0, ndc=False, seed=11, max_net_rows=NET_ROWS)
    assert vr.routes == (L_.ANYVIEW_FUSED, L_.ANYVIEW_LAYERS32)
    rgb, _, _, extras = vr.render(c2w, step=3, export=True)
    assert torch.isfinite(rgb).all()
    assert c_hosts.fnv1a(extras["rgb8"].cpu().numpy().tobytes()) == host["rgb8"]
    assert c_hosts.fnv1a(rgb.cpu().numpy().tobytes()) == host["rgb"]
    assert c_hosts.fnv1a(depth16_numpy(extras["depth16"]).tobytes()) == host["depth16"]
