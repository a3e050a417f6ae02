"""plnerf_render_view and its two kernels (include/plnerf_hip_view.h) on a real MI355X.

Every bound here is exact.  plnerf_view_rays against the torch expressions render() evaluates on the device for a full view
(rays.get_rays, raybatch.unit_directions, the near / far columns); plnerf_frame_export against numpy's to8b / to16b on the
same fp32 inputs, tails and alignments included; plnerf_render_view against render() under DrawSource(seed, 0, step) -- the
same kernels with the same arguments on one stream -- for both modes, both colour modes, jitter on and off, density noise,
NDC, fp32 and f16x3; the frame's independence of max_rays and of how the pixel range is split over calls; the export
through the call; render_path_frames' files; and tests/c_abi_view_gpu.cpp, which renders a frame without Python."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import c_hosts
from gpu_support import P, dev, g, nvs_nets, same_bits
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu
PLANES = ("rgb", "disp", "acc", "depth", "rgb0", "disp0", "acc0", "depth0", "z_std")


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def to16b(x):
    return (65535 * np.clip(x, 0, 1)).astype(np.uint16)


def _pose(forward_facing=False):
    """A generic rotation with a translation ([3,4] fp32, host)."""
    import plnerf_amd as P_
    if not forward_facing:
        c2w = P_.rays.pose_spherical(40.0, -30.0, 4.0)[:3, :4].clone()
        c2w[:, 3] += torch.tensor([0.3, -0.2, 0.1])
        return c2w
    a, b = 0.07, -0.05      # a small tilt about x and y: the camera still looks down -z
    rx = torch.tensor([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], dtype=torch.float64)
    ry = torch.tensor([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]], dtype=torch.float64)
    return torch.cat([ry @ rx, torch.tensor([[0.1], [-0.05], [0.2]], dtype=torch.float64)], 1).float()


# ----------------------------------------------------------------------------- plnerf_view_rays
def _view_rays(H, W, K, c2w, pix0, R, near, far, want_viewdirs=True):
    from plnerf_amd import _lib as L
    o, d, v = (torch.full((R, 3), 777.0, device=dev()) for _ in range(3))
    n, f = (torch.full((R,), 777.0, device=dev()) for _ in range(2))
    c2w_host = (ctypes.c_float * 12)(*[float(x) for x in c2w.cpu().reshape(-1)])
    L.check(L.lib().plnerf_view_rays(H, W, K[0][0], K[1][1], K[0][2], K[1][2], c2w_host, pix0, R, near, far, L.dptr(o), L.dptr(d),
                                     L.dptr(v) if want_viewdirs else None, L.dptr(n), L.dptr(f), L.stream()), "plnerf_view_rays")
    return o, d, v, n, f


@pytest.mark.parametrize("pix0,R", [(11, 50), (11, 1), (116, 1), (0, 117), (0, 0)])
def test_view_rays_are_get_rays_of_those_pixels(P, pix0, R):
    """H x W = 9 x 13, off-centre principal point, fx != fy, intrinsics that are not fp32 numbers; [11, 61) crosses four row
    ends.  The reference is what render() evaluates for a full view whose pose lives on the device."""
    from plnerf_amd import raybatch as RB
    H, W, near, far = 9, 13, 2.0, 6.0
    K = [[11.3, 0, 6.1], [0, 9.7, 4.3], [0, 0, 1]]
    c2w = _pose()
    o_ref, d_ref = P.get_rays(H, W, K, g(c2w))
    rows, _ = RB.pack_rays(o_ref, d_ref, near, far, [RB.unit_directions(d_ref)])
    assert rows.is_cuda and rows.shape == (H * W, 11)
    rows = rows[pix0:pix0 + R]
    o, d, v, n, f = _view_rays(H, W, K, c2w, pix0, R, near, far)
    assert torch.equal(o, rows[:, 0:3]) and torch.equal(d, rows[:, 3:6]) and torch.equal(v, rows[:, 8:11])
    assert torch.equal(n, rows[:, 6]) and torch.equal(f, rows[:, 7])
    # viewdirs is nullable: the other outputs are what they were, and nothing is written through the missing pointer
    o2, d2, v2, n2, f2 = _view_rays(H, W, K, c2w, pix0, R, near, far, want_viewdirs=False)
    assert torch.equal(o2, o) and torch.equal(d2, d) and torch.equal(n2, n) and torch.equal(f2, f) and (v2 == 777.0).all()


# ----------------------------------------------------------------------------- plnerf_frame_export
def _ulp_neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf), dtype=np.float32), x, np.nextafter(x, np.float32(np.inf), dtype=np.float32)]


def _crafted(levels):
    """k / levels one ulp below, on and one ulp above for several k; exact 0 and 1; negatives; values above 1; a denormal;
    +-inf.  The first three are chosen so that n = 1 still meets a code boundary, a clamp and an infinity."""
    vals = [np.nextafter(np.float32(128.0 / levels), np.float32(0)), np.float32(np.inf), np.float32(-0.5)]
    for k in (1, 2, 3, 127, 128, 254, levels - 1, levels // 3, levels // 2 + 1):
        vals += _ulp_neighbours(np.float32(k) / np.float32(levels))
    vals += [0.0, -0.0, 1.0, 1.0 + 2.0 ** -23, 1.5, 300.0, -1e-3, -7.0, 1e-40, -1e-40, 2.0 ** -126, -np.inf, 0.999999, 0.5,
             0.499, 0.503, 0.9985, 0.005, 1.6e-5, 0.99999]      # (codes 127, 128, 254, 1 | 1, 65534 whatever the rounding at a boundary)
    return np.array(vals, dtype=np.float32)


def _export(rgb, gray, scale, n, off8=0, off16=0):
    """plnerf_frame_export into sentinel-filled, over-allocated outputs; returns (rgb8, gray16, bytes around each)."""
    from plnerf_amd import _lib as L
    pad = 16
    out8 = torch.full((pad + 3 * n + pad,), 0xA5, dtype=torch.uint8, device=dev())
    out16 = torch.full((pad + 2 * n + pad,), 0xA5, dtype=torch.uint8, device=dev())
    p8 = ctypes.c_void_p(out8.data_ptr() + pad + off8) if rgb is not None else None
    p16 = ctypes.c_void_p(out16.data_ptr() + pad + off16) if gray is not None else None
    L.check(L.lib().plnerf_frame_export(L.dptr(rgb), p8, L.dptr(gray), float(scale), p16, n, L.stream()), "plnerf_frame_export")
    h8, h16 = out8.cpu().numpy(), out16.cpu().numpy()
    body8 = h8[pad + off8:pad + off8 + 3 * n]
    body16 = h16[pad + off16:pad + off16 + 2 * n].copy().view(np.uint16)
    around8 = np.concatenate([h8[:pad + off8], h8[pad + off8 + 3 * n:]])
    around16 = np.concatenate([h16[:pad + off16], h16[pad + off16 + 2 * n:]])
    return body8, body16, around8, around16


@pytest.mark.parametrize("off8,off16", [(0, 0), (1, 2), (2, 0), (3, 2)])
@pytest.mark.parametrize("n", [1, 2, 3, 1003])
def test_frame_export_is_to8b_and_to16b(P, n, off8, off16):
    scale = np.float32(1.0) / np.float32(6.0)
    rgb_h = np.resize(_crafted(255), 3 * n).astype(np.float32)
    # the grey plane is scaled before it is quantised: feed values whose PRODUCT with the scale sits at the code boundaries
    gray_h = (np.resize(_crafted(65535), n) * np.float32(6.0)).astype(np.float32)
    rgb8, gray16, around8, around16 = _export(g(torch.from_numpy(rgb_h)).view(n, 3), g(torch.from_numpy(gray_h)), scale, n, off8, off16)
    with np.errstate(invalid="ignore", over="ignore"):
        want8, want16 = to8b(rgb_h), to16b(gray_h * scale)
    assert np.array_equal(rgb8, want8), np.flatnonzero(rgb8 != want8)[:8]
    assert np.array_equal(gray16, want16), np.flatnonzero(gray16 != want16)[:8]
    assert (around8 == 0xA5).all() and (around16 == 0xA5).all()       # not a byte before, none past 3 n / 2 n
    if n == 1003:                                                     # the crafted values do reach every kind of code
        assert {0, 1, 127, 128, 254, 255} <= set(want8.tolist()) and {0, 1, 65534, 65535} <= set(want16.tolist())


@pytest.mark.parametrize("n", [1, 3, 1003])
def test_frame_export_one_plane_at_a_time_and_nan(P, n):
    """Either plane may be absent; NaN maps to code 0 (asserted: numpy's cast of NaN is undefined)."""
    rng = np.random.default_rng(n)
    rgb_h = rng.uniform(-0.2, 1.2, 3 * n).astype(np.float32)
    gray_h = rng.uniform(-1.0, 7.0, n).astype(np.float32)
    nan8, nan16 = rng.random(3 * n) < 0.3, rng.random(n) < 0.3
    nan8[0], nan16[0] = True, True
    rgb_h[nan8], gray_h[nan16] = np.nan, np.nan
    scale = np.float32(1.0) / np.float32(6.0)
    with np.errstate(invalid="ignore"):
        want8, want16 = to8b(np.nan_to_num(rgb_h, nan=0.0)), to16b(np.nan_to_num(gray_h, nan=0.0) * scale)
    rgb_t, gray_t = g(torch.from_numpy(rgb_h)).view(n, 3), g(torch.from_numpy(gray_h))
    both = _export(rgb_t, gray_t, scale, n)
    assert (both[0][nan8] == 0).all() and (both[1][nan16] == 0).all()
    assert np.array_equal(both[0], want8) and np.array_equal(both[1], want16)
    only8 = _export(rgb_t, None, scale, n)
    assert np.array_equal(only8[0], want8) and (only8[3] == 0xA5).all() and (only8[1].view(np.uint8) == 0xA5).all()
    only16 = _export(None, gray_t, scale, n)
    assert np.array_equal(only16[1], want16) and (only16[2] == 0xA5).all() and (only16[0] == 0xA5).all()
    # NaN times a zero scale, and an infinity times it: both NaN, both code 0
    odd = _export(None, g(torch.tensor([np.inf, np.nan, 1.0] * n)[:n].float()), 0.0, n)
    assert (odd[1] == 0).all()


def test_frame_export_scale_is_a_multiplier(P):
    """gray * gray_scale is torch's fp32 product of the two; against the reference's division by far a code can move by one
    (a reciprocal multiply and a division differ by under 2 ulp = 0.02 of a code: only truncation at a boundary moves one)."""
    n, far = 1003, 6.0
    gen = torch.Generator().manual_seed(5)
    gray_t = g(torch.rand(n, generator=gen) * 7.0)
    scale_t = torch.tensor(1.0, device=dev()) / torch.tensor(far, device=dev())
    got = _export(None, gray_t, float(scale_t), n)[1]
    assert np.array_equal(got, to16b((gray_t * scale_t).cpu().numpy()))
    by_division = to16b((gray_t / far).cpu().numpy())
    step = np.abs(got.astype(np.int64) - by_division.astype(np.int64))
    assert step.max() <= 1, int(step.max())


# ----------------------------------------------------------------------------- plnerf_render_view against render()
H_VIEW, W_VIEW = 13, 9
K_VIEW = [[11.3, 0, 4.1], [0, 9.7, 6.6], [0, 0, 1]]


@functools.lru_cache(maxsize=None)
def _networks(precision):
    """create_nerf's render kwargs with the closed-form weights of the other GPU tests, (64, 128) samples."""
    import plnerf_amd as P_
    _, kw, _, _ = nvs_nets(P_, precision, N_samples=64, N_importance=128)
    return kw


def _kwargs(precision, **over):
    kw = dict(_networks(precision))
    kw.update(over)
    kw.setdefault("ndc", False)
    return kw


def _reference_frame(P, kw, H, W, K, c2w, chunk, near, far, seed, step):
    from plnerf_amd import functional as Fn
    prev = Fn.set_draw_source(Fn.DrawSource(seed, 0, step))
    try:
        with torch.no_grad():
            rgb, disp, acc, extras = P.render(H, W, K, chunk=chunk, c2w=g(c2w), near=near, far=far, **kw)
    finally:
        Fn.set_draw_source(prev)
    return {"rgb": rgb, "disp": disp, "acc": acc, "depth": extras["depth_map"], "rgb0": extras["rgb0"], "disp0": extras["disp0"],
            "acc0": extras["acc0"], "depth0": extras["depth0"], "z_std": extras["z_std"]}


def _renderer(P, kw, H, W, K, chunk, near, far, seed):
    kw = dict(kw)
    ndc = kw.pop("ndc")
    return P.ViewRenderer(kw, H, W, K, chunk, near, far, ndc=ndc, seed=seed)


def _frame(vr, c2w, step, export=False):
    rgb, disp, acc, extras = vr.render(c2w, step=step, export=export)
    out = {"rgb": rgb, "disp": disp, "acc": acc, "depth": extras["depth_map"], "rgb0": extras["rgb0"], "disp0": extras["disp0"],
           "acc0": extras["acc0"], "depth0": extras["depth0"], "z_std": extras["z_std"]}
    return out, extras


CASES = {
    "linear_midpoint_jitter_white": (dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True), False, 2.0, 6.0),
    "linear_left_u_vals": (dict(mode="linear", color_mode="left", perturb=0.0, white_bkgd=False), False, 2.0, 6.0),
    "noise_1": (dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=False, raw_noise_std=1.0), False, 2.0, 6.0),
    "noise_half": (dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=0.5), False, 2.0, 6.0),
    "ndc": (dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=False, ndc=True), True, 0.0, 1.0),
    "constant": (dict(mode="constant", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=1.0), False, 2.0, 6.0),
}


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_render_view_equals_render(P, case, precision):
    over, forward_facing, near, far = CASES[case]
    kw = _kwargs(precision, **over)
    c2w = _pose(forward_facing)
    seed, step = 9, 4
    ref = _reference_frame(P, kw, H_VIEW, W_VIEW, K_VIEW, c2w, 50, near, far, seed, step)
    vr = _renderer(P, kw, H_VIEW, W_VIEW, K_VIEW, 50, near, far, seed)
    got, extras = _frame(vr, c2w, step)
    assert set(extras) == {"rgb0", "disp0", "acc0", "depth0", "depth_map", "z_std"}
    for name in PLANES:
        assert got[name].shape == ref[name].shape and (name.startswith("disp") or torch.isfinite(ref[name]).all()), name
        assert same_bits(got[name], ref[name]), (case, precision, name, float((got[name] - ref[name]).abs().max()))
    assert [int(w.item()) for w in vr.status_words()] == [0, 0]


def test_another_step_or_seed_is_another_frame(P):
    kw = _kwargs("f16x3", **CASES["noise_half"][0])
    c2w = _pose()
    vr = _renderer(P, kw, H_VIEW, W_VIEW, K_VIEW, 50, 2.0, 6.0, 9)
    a = _frame(vr, c2w, 4)[0]["rgb"].clone()
    b = _frame(vr, c2w, 5)[0]["rgb"].clone()
    c = _frame(_renderer(P, kw, H_VIEW, W_VIEW, K_VIEW, 50, 2.0, 6.0, 10), c2w, 4)[0]["rgb"]
    again = _frame(vr, c2w, 4)[0]["rgb"]
    assert torch.equal(a, again) and not torch.equal(a, b) and not torch.equal(a, c)


def test_unsupported_configurations_raise(P):
    kw = _kwargs("f16x3", **CASES["linear_midpoint_jitter_white"][0])
    kw.pop("ndc")
    assert P.ViewRenderer.supported(kw)
    for change, word in ((dict(N_importance=0), "N_importance"), (dict(network_fine=None), "two networks"),
                         (dict(use_viewdirs=False), "use_viewdirs"), (dict(network_query_fn=lambda *a: None), "encoders"),
                         (dict(pytest=True), "pytest")):
        bad = dict(kw, **change)
        assert not P.ViewRenderer.supported(bad)
        with pytest.raises(ValueError, match=word):
            P.ViewRenderer(bad, H_VIEW, W_VIEW, K_VIEW, 50, 2.0, 6.0)


def test_moved_parameters_are_refused_on_the_host(P):
    """A renderer holds the parameters' addresses: when one has moved, enqueue() raises before anything is enqueued, and a
    new renderer on the same networks renders the same frame."""
    kw = _kwargs("f16x3", N_samples=8, N_importance=8, **CASES["linear_left_u_vals"][0])
    c2w = _pose()
    vr = _renderer(P, kw, 4, 6, K_VIEW, 16, 2.0, 6.0, 9)
    first = {k: v.clone() for k, v in _frame(vr, c2w, 4)[0].items()}
    p = kw["network_fine"].param_list()[3]
    old = p.data
    try:
        p.data = p.data.clone()
        assert not vr.current()
        with pytest.raises(RuntimeError, match="ViewRenderer: the networks' parameters moved"):
            vr.enqueue(c2w, step=4)
        fresh = _renderer(P, kw, 4, 6, K_VIEW, 16, 2.0, 6.0, 9)
        assert fresh.current()
        again = _frame(fresh, c2w, 4)[0]
        for name in PLANES:
            assert same_bits(again[name], first[name]), name      # (torch.equal, but for a disparity that is NaN in both)
    finally:
        p.data = old      # (the networks are shared with the other tests)
    assert vr.current()


# ----------------------------------------------------------------------------- independence of the chunking
def _snapshot(vr):
    return {k: v.clone() for k, v in vr.planes.items()}, vr.rgb8.clone(), vr.depth16.clone()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_frame_does_not_depend_on_the_chunking(P, precision):
    kw = _kwargs(precision, **CASES["noise_half"][0])
    c2w, step, n = _pose(), 2, H_VIEW * W_VIEW
    frames = []
    for chunk in (32, 50, 117):
        vr = _renderer(P, kw, H_VIEW, W_VIEW, K_VIEW, chunk, 2.0, 6.0, 3)
        vr.render(c2w, step=step, export=True)
        frames.append(_snapshot(vr))
    whole = frames[0]
    for planes, rgb8, depth16 in frames[1:]:
        assert all(same_bits(planes[k], whole[0][k]) for k in PLANES)
        assert torch.equal(rgb8, whole[1]) and torch.equal(depth16, whole[2])

    # two calls over [0, 60) and [60, 117) are one call
    vr = _renderer(P, kw, H_VIEW, W_VIEW, K_VIEW, 50, 2.0, 6.0, 3)
    for v in vr.planes.values():
        v.fill_(777.0)
    vr.enqueue(c2w, step=step, export=True, pix0=0, n_pix=60)
    vr.enqueue(c2w, step=step, export=True, pix0=60, n_pix=57)
    planes, rgb8, depth16 = _snapshot(vr)
    assert all(same_bits(planes[k], whole[0][k]) for k in PLANES)
    assert torch.equal(rgb8, whole[1]) and torch.equal(depth16, whole[2])

    # a call over [20, 70) touches no pixel outside that range, in the fp32 planes and in the 8 / 16-bit ones
    for v in vr.planes.values():
        v.fill_(777.0)
    vr.rgb8.fill_(0xA5)
    vr.depth16.fill_(0x5A5A)
    vr.enqueue(c2w, step=step, export=True, pix0=20, n_pix=50)
    planes, rgb8, depth16 = _snapshot(vr)
    inside = torch.zeros(n, dtype=torch.bool, device=dev())
    inside[20:70] = True
    for k in PLANES:
        assert same_bits(planes[k][inside], whole[0][k][inside]), k
        assert (planes[k][~inside] == 777.0).all(), k
    assert torch.equal(rgb8[inside], whole[1][inside]) and (rgb8[~inside] == 0xA5).all()
    assert torch.equal(depth16[inside], whole[2][inside]) and (depth16[~inside] == 0x5A5A).all()


# ----------------------------------------------------------------------------- export through the call
@pytest.mark.parametrize("case", ["linear_midpoint_jitter_white", "ndc"])
def test_export_through_the_call(P, case):
    from plnerf_amd.view import depth16_numpy
    over, forward_facing, near, far = CASES[case]
    kw = _kwargs("f16x3", **over)
    vr = _renderer(P, kw, H_VIEW, W_VIEW, K_VIEW, 50, near, far, 1)
    got, extras = _frame(vr, _pose(forward_facing), 0, export=True)
    assert extras["rgb8"].shape == (H_VIEW, W_VIEW, 3) and extras["rgb8"].dtype == torch.uint8
    assert extras["depth16"].shape == (H_VIEW, W_VIEW)
    scale = np.float32(1.0) / np.float32(far)
    assert vr.args.depth16_scale == scale
    assert np.array_equal(extras["rgb8"].cpu().numpy(), to8b(got["rgb"].cpu().numpy()))
    want16 = to16b((got["depth"] * torch.tensor(scale, device=dev())).cpu().numpy())
    assert np.array_equal(depth16_numpy(extras["depth16"]), want16)
    assert len(np.unique(want16)) > 1 and len(np.unique(extras["rgb8"].cpu().numpy())) > 1      # not a flat frame


# ----------------------------------------------------------------------------- render_path_frames
def test_render_path_frames_writes_the_frames(P, tmp_path):
    H, W, focal = 12, 8, 10.0
    K = [[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]]
    kw = _kwargs("f16x3", near=2.0, far=6.0, **CASES["linear_midpoint_jitter_white"][0])
    poses = torch.stack([P.rays.pose_spherical(th, -30.0, 4.0) for th in (20.0, 75.0)], 0)
    savedir = tmp_path / "frames"
    rgbs, disps = P.render_path_frames(poses, (H, W, focal), K, 40, kw, savedir=str(savedir), seed=6)
    assert rgbs.shape == (2, H, W, 3) and disps.shape == (2, H, W) and rgbs.dtype == np.float32
    assert sorted(os.listdir(str(savedir))) == ["000.png", "001.png"]
    render_kw = {k: v for k, v in kw.items() if k not in ("near", "far")}
    for i in range(2):
        ref = _reference_frame(P, render_kw, H, W, K, poses[i, :3, :4], 40, 2.0, 6.0, 6, i)
        assert np.array_equal(rgbs[i], ref["rgb"].cpu().numpy()) and np.array_equal(disps[i], ref["disp"].cpu().numpy(), equal_nan=True)
        decoded = P.read_png(str(savedir / f"{i:03d}.png"))
        assert decoded.dtype == np.uint8 and np.array_equal(decoded, to8b(rgbs[i]))
    assert not np.array_equal(rgbs[0], rgbs[1])
    # render_factor: the frames shrink, as render_path's do; nothing is written without a savedir
    half, _ = P.render_path_frames(poses[:1], (H, W, focal), K, 40, kw, render_factor=2, seed=6)
    assert half.shape == (1, H // 2, W // 2, 3)
    with torch.no_grad():
        same, _ = P.render_path(g(poses[:1]), (H, W, focal), K, 40, kw, render_factor=2)
    assert same.shape == half.shape
    # render_path itself keeps refusing to write
    with pytest.raises(NotImplementedError):
        P.render_path(poses, (H, W, focal), K, 40, kw, savedir=str(tmp_path / "other"))
    assert not (tmp_path / "other").exists()


# ----------------------------------------------------------------------------- a host without Python
@pytest.mark.parametrize("precision", ["f16x3"])
def test_c_host_renders_without_python(P, precision, tmp_path):
    """tests/c_abi_view_gpu.cpp -- the HIP runtime and include/plnerf_hip_view.h, nothing else -- renders a 16 x 12 view in
    blocks of 64 and of 192 pixels and checks them byte-identical and finite itself; ViewRenderer on the same hashed
    weights and pose produces the same bytes (the same entry on the same inputs)."""
    from plnerf_amd import _lib as L_
    from plnerf_amd.view import depth16_numpy
    exe = c_hosts.build("c_abi_view_gpu", tmp_path)
    Ns, Ni, IMG_H, IMG_W = 64, 128, 16, 12
    run = c_hosts.run(exe, L_.PRECISION[precision], L_.FWD_KERNEL, c_hosts.write_tables(tmp_path / "tables.bin", Ns, Ni))
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    host, _fnv1a = c_hosts.parse_planes(run.stdout), c_hosts.fnv1a
    assert set(host) == {"rgb8", "rgb", "depth16"}

    _, kw, _, _ = nvs_nets(P, precision, N_samples=Ns, N_importance=Ni)
    for which, net in enumerate((kw["network_fn"], kw["network_fine"])):
        net.load_state_dict(c_hosts.hashed_state_dict(which, orc.param_shapes()))
    kw = dict(kw, mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True, raw_noise_std=0.0)
    kw.pop("ndc", None)
    K = [[20.0, 0, 0.5 * IMG_W], [0, 21.0, 0.5 * IMG_H], [0, 0, 1]]
    c2w = torch.tensor([[1.0, 0, 0, 0.1], [0, 1.0, 0, -0.2], [0, 0, 1.0, 4.0]])
    vr = P.ViewRenderer(kw, IMG_H, IMG_W, K, 64, 2.0, 6.0, ndc=False, seed=11)
    rgb, _, _, extras = vr.render(c2w, step=3, export=True)
    assert torch.isfinite(rgb).all()
    assert _fnv1a(extras["rgb8"].cpu().numpy().tobytes()) == host["rgb8"]
    assert _fnv1a(rgb.cpu().numpy().tobytes()) == host["rgb"]
    assert _fnv1a(depth16_numpy(extras["depth16"]).tobytes()) == host["depth16"]
