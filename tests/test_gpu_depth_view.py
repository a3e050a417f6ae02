"""plnerf_depth_render_view and its two kernels (include/experimental/plnerf_hip_depthview.h) on a real MI355X.

Every bound here is exact but one.  plnerf_depth_view_rays against the torch expressions depth.render() evaluates on the
device for a full view (depth.get_rays with the intrinsics and the pose as device tensors, raybatch.unit_directions, the
near / far columns); plnerf_frame_export_u16 against numpy on the plane itself; plnerf_depth_render_view against
depth.render_rays on the same rays under DrawSource(seed, first pixel, step) -- the same kernels with the same arguments on
one stream -- and, at test time, against depth.render(); the frame's independence of max_rays and of how the pixel range is
split over calls; error_row against the rows depth.test_images_samples' present route accumulates (bit for bit with its
blocks; within 1e-12 relative of tests/sampleerr_fp64.py with other blocks: the bound tests/test_gpu_sample_error.py uses for
another order of the same fp64 additions); the one_call keyword of the two evaluation loops; the range check; the guard
bands of tests/depthview_cases.py through tests/containment.py's runner; and tests/c_abi_depth_view_gpu.cpp, which renders a
frame without Python.

The view is 9 x 13 with fx != fy and an off-centre principal point, none of them an fp32 number; 6 + 5 samples, so the rows
per ray are no multiple of any tile; networks as depth.create_nerf builds them (pi-encoding 57 | 3, softplus beta 10) with
alpha_linear sharpened."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

import c_hosts
import containment as C
import depthview_cases as cases
import sampleerr_fp64 as ref64
from gpu_support import P, depth_nets, dev, g, same_bits
from oracle import plnerf_oracle as orc
from run_args import depth_args

pytestmark = pytest.mark.gpu
PLANES = ("rgb", "disp", "acc", "depth", "rgb0", "disp0", "acc0", "depth0", "z_std")
H, W, NS, NI = 9, 13, 6, 5
INTRINSIC = (11.3, 9.7, 6.1, 4.3)      # fx, fy, cx, cy
NEAR, FAR = 2.0, 6.0
KERNEL_REL = 1e-12


def _pose():
    """A generic rotation with a translation ([3,4] fp32, host)."""
    import plnerf_amd as P_
    c2w = P_.rays.pose_spherical(40.0, -30.0, 4.0)[:3, :4].clone()
    c2w[:, 3] += torch.tensor([0.3, -0.2, 0.1])
    return c2w


def _intrinsic():
    return torch.tensor(INTRINSIC, dtype=torch.float32, device=dev())


# ----------------------------------------------------------------------------- plnerf_depth_view_rays
def _view_rays(Hv, Wv, c2w, pix0, R, want_viewdirs=True):
    from plnerf_amd import _lib as L
    o, d, v = (torch.full((max(R, 1), 3), 777.0, device=dev()) for _ in range(3))
    n, f = (torch.full((max(R, 1),), 777.0, device=dev()) for _ in range(2))
    c2w_host = (ctypes.c_float * 12)(*[float(x) for x in c2w.cpu().reshape(-1)])
    L.check(L.lib().plnerf_depth_view_rays(Hv, Wv, *INTRINSIC, c2w_host, pix0, R, NEAR, FAR, L.dptr(o), L.dptr(d),
                                           L.dptr(v) if want_viewdirs else None, L.dptr(n), L.dptr(f), L.stream()),
            "plnerf_depth_view_rays")
    return o[:R], d[:R], v[:R], n[:R], f[:R]


@functools.lru_cache(maxsize=None)
def _reference_rows(Hv, Wv):
    """What depth.render() evaluates for a full view whose pose and intrinsics live on the device: [H W, 11] rows."""
    from plnerf_amd import depth as Dp
    from plnerf_amd import raybatch as RB
    o_ref, d_ref = Dp.get_rays(Hv, Wv, _intrinsic(), g(_pose()))
    rows, _ = RB.pack_rays(o_ref, d_ref, NEAR, FAR, [RB.unit_directions(d_ref)])
    assert rows.is_cuda and rows.shape == (Hv * Wv, 11)
    return rows


@pytest.mark.parametrize("Hv,Wv,pix0,R", [(9, 13, 11, 50), (9, 13, 0, 1), (9, 13, 116, 1), (9, 13, 12, 1), (9, 13, 0, 117),
                                          (37, 53, 0, 37 * 53)])
def test_view_rays_are_get_rays_of_those_pixels(P, Hv, Wv, pix0, R):
    """[11, 61) crosses four row ends; single pixels: the first, the last, a row end; the whole view; 37 x 53 (1,961 pixels:
    eight workgroups, the last one short)."""
    rows = _reference_rows(Hv, Wv)[pix0:pix0 + R]
    c2w = _pose()
    o, d, v, n, f = _view_rays(Hv, Wv, c2w, pix0, R)
    assert torch.equal(o, rows[:, 0:3]) and torch.equal(d, rows[:, 3:6]) and torch.equal(v, rows[:, 8:11])
    assert torch.equal(n, rows[:, 6]) and torch.equal(f, rows[:, 7])
    o2, d2, v2, n2, f2 = _view_rays(Hv, Wv, c2w, pix0, R, want_viewdirs=False)
    assert torch.equal(o2, o) and torch.equal(d2, d) and torch.equal(n2, n) and torch.equal(f2, f) and (v2 == 777.0).all()


# ----------------------------------------------------------------------------- plnerf_frame_export_u16
def _crafted_mm():
    """Depths whose product with 1000 sits at k / 1000 one ulp below, on and one ulp above a code; 0, negatives, 65.535 and
    above; +-inf (NaN is a test of its own: numpy's cast of it is undefined).  The first two are chosen so that n = 1 and
    n = 2 still meet a code boundary and a clamp."""
    vals = [np.nextafter(np.float32(3.0), np.float32(0)), np.float32(70.0)]
    for k in (1, 2, 999, 1000, 2500, 32767, 32768, 65534):
        x = np.float32(k) / np.float32(1000.0)
        vals += [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]
    vals += [0.0, -0.0, -1e-3, -7.0, 1e-40, 65.535, np.nextafter(np.float32(65.535), np.float32(0)), 65.5355, 65.536, 66.0, 1e9,
             np.inf, -np.inf, 5.9999, 2.0, 0.0004, 0.0015]
    return np.array(vals, dtype=np.float32)


def _want_u16(gray, mult):
    """The header's definition: trunc(min(max(fl(gray * mult), 0), 65535)), NaN -> 0; on every product in [0, 65536) this IS
    numpy's (gray * mult).astype(np.uint16), which is asserted too."""
    with np.errstate(invalid="ignore", over="ignore"):
        prod = gray * np.float32(mult)
        want = np.clip(np.nan_to_num(prod, nan=0.0, posinf=np.inf, neginf=-np.inf), 0, 65535).astype(np.uint16)
        defined = (prod >= 0) & (prod < 65536)
        assert np.array_equal(want[defined], prod[defined].astype(np.uint16))
    return want


def _export_u16(gray, mult, n, off16=0):
    """plnerf_frame_export_u16 into a sentinel-filled, over-allocated output; returns (codes, the bytes around them)."""
    from plnerf_amd import _lib as L
    pad = 16
    out16 = torch.full((pad + 2 * n + pad,), 0xA5, dtype=torch.uint8, device=dev())
    p16 = ctypes.c_void_p(out16.data_ptr() + pad + off16)
    L.check(L.lib().plnerf_frame_export_u16(L.dptr(gray), float(mult), p16, n, L.stream()), "plnerf_frame_export_u16")
    h16 = out16.cpu().numpy()
    body16 = h16[pad + off16:pad + off16 + 2 * n].copy().view(np.uint16)
    around16 = np.concatenate([h16[:pad + off16], h16[pad + off16 + 2 * n:]])
    return body16, around16


@pytest.mark.parametrize("off16", [0, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 1003])
def test_frame_export_u16_is_numpys_cast(P, n, off16):
    gray_h = np.resize(_crafted_mm(), n).astype(np.float32)
    got, around16 = _export_u16(g(torch.from_numpy(gray_h)), 1000.0, n, off16)
    want = _want_u16(gray_h, 1000.0)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert (around16 == 0xA5).all()                                   # not a byte before, none past 2 n
    if n == 1003:                                                     # the crafted values do reach every kind of code
        assert {0, 1, 2, 999, 1000, 32767, 32768, 65534, 65535} <= set(want.tolist())


@pytest.mark.parametrize("off16", [0, 2])
@pytest.mark.parametrize("n", [1, 3, 1003])
def test_frame_export_u16_nan_and_infinities(P, n, off16):
    """NaN -> 0, -inf -> 0, +inf -> 65535 (asserted: numpy leaves these casts undefined), also under a zero multiplier; on
    the word path (off16 = 0) and on the value-by-value path of an output that is only 2-byte aligned (off16 = 2)."""
    rng = np.random.default_rng(n)
    gray_h = rng.uniform(-1.0, 70.0, n).astype(np.float32)
    nan = rng.random(n) < 0.3
    nan[0] = True
    gray_h[nan] = np.nan
    got, around16 = _export_u16(g(torch.from_numpy(gray_h)), 1000.0, n, off16)
    assert (got[nan] == 0).all() and np.array_equal(got, _want_u16(gray_h, 1000.0)) and (around16 == 0xA5).all()
    odd = torch.tensor([np.inf, -np.inf, np.nan] * n)[:n].float()
    got, around16 = _export_u16(g(odd), 1000.0, n, off16)
    assert np.array_equal(got, np.array([65535, 0, 0] * n, dtype=np.uint16)[:n]) and (around16 == 0xA5).all()
    got, _ = _export_u16(g(odd), 0.0, n, off16)                              # inf * 0 and NaN * 0 are NaN
    assert (got == 0).all()


# ----------------------------------------------------------------------------- networks
def _args(precision, **over):
    """The evaluation loops' arguments: no loss fields, 6 + 5 samples, a black background, chunks of 50 rays."""
    at = dict(precision=precision, N_importance=NI, N_samples=NS, white_bkgd=False, chunk=50, dataset="scannet")
    return depth_args(train=False, **dict(at, **over))


@functools.lru_cache(maxsize=None)
def _networks(precision):
    """depth.create_nerf's (train kwargs, test kwargs) with the closed-form weights of the other depth tests, alpha_linear
    sharpened; 6 + 5 samples."""
    kw, kw_test = depth_nets(_args(precision))[:2]
    assert kw["network_fn"].input_ch == 57 and kw["network_fn"].input_ch_views == 3 and kw["network_fn"].density_beta == 10.0
    return kw, kw_test


def _kwargs(precision, test_time=False, **over):
    kw = dict(_networks(precision)[1 if test_time else 0])
    kw.update(over)
    return kw


def _renderer(P, kw, chunk, seed=0, Hv=H, Wv=W):
    return P.DepthViewRenderer(kw, Hv, Wv, chunk, NEAR, FAR, seed=seed)


def _frame(vr, step=0, **more):
    rgb, disp, acc, extras = vr.render(_pose(), _intrinsic(), step=step, want_hyp=True, **more)
    out = {"rgb": rgb, "disp": disp, "acc": acc, "depth": extras["depth_map"], "rgb0": extras["rgb0"], "disp0": extras["disp0"],
           "acc0": extras["acc0"], "depth0": extras["depth0"], "z_std": extras["z_std"], "pred_hyp": extras["pred_hyp"]}
    return out, extras


def _named(ret, lead):
    names = {"rgb": "rgb_map", "disp": "disp_map", "acc": "acc_map", "depth": "depth_map", "rgb0": "rgb0", "disp0": "disp0",
             "acc0": "acc0", "depth0": "depth0", "z_std": "z_std", "pred_hyp": "pred_hyp"}
    return {k: ret[v].reshape(*lead, *ret[v].shape[1:]) for k, v in names.items()}


def _render_rays_frame(kw, seed, step):
    """depth.render_rays on the view's rays (all of them in one batch: a ray's global id is its pixel index) under
    DrawSource(seed, first pixel = 0, step)."""
    from plnerf_amd import depth as Dp
    from plnerf_amd import functional as Fn
    prev = Fn.set_draw_source(Fn.DrawSource(seed, 0, step))
    try:
        with torch.no_grad():
            ret = Dp.render_rays(_reference_rows(H, W), **kw)
    finally:
        Fn.set_draw_source(prev)
    return _named(ret, (H, W))


CASES = {
    "linear_midpoint_jitter": dict(mode="linear", color_mode="midpoint", perturb=1.0),
    "linear_left_u_vals": dict(mode="linear", color_mode="left", perturb=0.0),
    "noise_1": dict(mode="linear", color_mode="midpoint", perturb=1.0, raw_noise_std=1.0),
    "noise_half": dict(mode="linear", color_mode="midpoint", perturb=1.0, raw_noise_std=0.5),
    "lindisp": dict(mode="linear", color_mode="midpoint", perturb=1.0, lindisp=True),
    "constant": dict(mode="constant", color_mode="midpoint", perturb=1.0, raw_noise_std=1.0),
    "white_bkgd": dict(mode="linear", color_mode="midpoint", perturb=1.0, white_bkgd=True),
}


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_equals_render_rays(P, case, precision):
    kw = _kwargs(precision, **CASES[case])
    seed, step = 9, 4
    want = _render_rays_frame(kw, seed, step)
    vr = _renderer(P, kw, 50, seed)
    got, extras = _frame(vr, step)
    assert set(extras) == {"rgb0", "disp0", "acc0", "depth0", "depth_map", "z_std", "pred_hyp"}
    for name in PLANES + ("pred_hyp",):
        assert got[name].shape == want[name].shape and (name.startswith("disp") or torch.isfinite(want[name]).all()), name
        assert same_bits(got[name], want[name]), (case, precision, name, float((got[name] - want[name]).abs().max()))
    assert float(got["depth"].max() - got["depth"].min()) > 0 and float(got["pred_hyp"].std()) > 0      # not a flat frame
    assert [int(w.item()) for w in vr.status_words()] == [0, 0]


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("chunk", [32, 50, 117])
def test_frame_at_test_time_equals_render(P, precision, chunk):
    """perturb = 0, no noise (render_kwargs_test): depth.render() with the pose and the intrinsics as device tensors."""
    from plnerf_amd import depth as Dp
    kw = _kwargs(precision, test_time=True)
    assert kw["perturb"] == 0 and kw["raw_noise_std"] == 0
    with torch.no_grad():
        rgb, disp, acc, ex = Dp.render(H, W, _intrinsic(), chunk=chunk, c2w=g(_pose()), near=NEAR, far=FAR, **kw)
    want = {"rgb": rgb, "disp": disp, "acc": acc, "depth": ex["depth_map"], "rgb0": ex["rgb0"], "disp0": ex["disp0"],
            "acc0": ex["acc0"], "depth0": ex["depth0"], "z_std": ex["z_std"], "pred_hyp": ex["pred_hyp"]}
    got, _ = _frame(_renderer(P, kw, chunk))
    for name in PLANES + ("pred_hyp",):
        assert same_bits(got[name], want[name]), (precision, chunk, name)


def test_another_step_or_seed_is_another_frame(P):
    kw = _kwargs("f16x3", **CASES["noise_half"])
    vr = _renderer(P, kw, 50, 9)
    a = _frame(vr, 4)[0]["pred_hyp"].clone()
    b = _frame(vr, 5)[0]["pred_hyp"].clone()
    c = _frame(_renderer(P, kw, 50, 10), 4)[0]["pred_hyp"]
    again = _frame(vr, 4)[0]["pred_hyp"]
    assert torch.equal(a, again) and not torch.equal(a, b) and not torch.equal(a, c)


def test_unsupported_configurations_raise(P):
    kw = _kwargs("f16x3")
    assert P.DepthViewRenderer.supported(kw)
    cam = torch.zeros(4, device=dev())
    for change, word in ((dict(N_importance=0), "N_importance"), (dict(network_fine=None), "two networks"),
                         (dict(use_viewdirs=False), "use_viewdirs"), (dict(network_query_fn=lambda *a: None), "encoders"),
                         (dict(pytest=True), "pytest"), (dict(is_joint=True), "is_joint"), (dict(embedded_cam=cam), "camera code"),
                         (dict(mode="constant", N_samples=2), "sample counts"), (dict(retraw=True), "retraw")):
        bad = dict(kw, **change)
        assert not P.DepthViewRenderer.supported(bad)
        with pytest.raises(ValueError, match=word):
            P.DepthViewRenderer(bad, H, W, 50, NEAR, FAR)


def test_moved_parameters_are_refused_on_the_host(P):
    """A renderer holds the parameters' addresses: when one has moved, enqueue() raises before anything is enqueued, and a
    new renderer on the same networks renders the same frame."""
    kw = _kwargs("f16x3", N_samples=8, N_importance=8)
    vr = _renderer(P, kw, 16, 9, Hv=4, Wv=6)
    first = {k: v.clone() for k, v in _frame(vr, 4)[0].items()}
    p = kw["network_fine"].param_list()[3]
    old = p.data
    try:
        p.data = p.data.clone()
        assert not vr.current()
        with pytest.raises(RuntimeError, match="DepthViewRenderer: the networks' parameters moved"):
            vr.enqueue(_pose(), _intrinsic(), step=4)
        fresh = _renderer(P, kw, 16, 9, Hv=4, Wv=6)
        assert fresh.current()
        again = _frame(fresh, 4)[0]
        for name in PLANES + ("pred_hyp",):
            assert same_bits(again[name], first[name]), name      # (torch.equal, but for a disparity that is NaN in both)
    finally:
        p.data = old      # (the networks are shared with the other tests)
    assert vr.current()


# ----------------------------------------------------------------------------- independence of the chunking
def _snapshot(vr):
    planes = {k: v.clone() for k, v in vr.planes.items()}
    planes["pred_hyp"] = vr.pred_hyp.clone()
    return planes, vr.rgb8.clone(), vr.depth16.clone(), vr.depth_mm16.clone()


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_frame_does_not_depend_on_the_chunking(P, precision):
    kw = _kwargs(precision, **CASES["noise_half"])
    step, n = 2, H * W
    c2w, intr = _pose(), _intrinsic()
    frames = []
    for chunk in (32, 50, 117):
        vr = _renderer(P, kw, chunk, 3)
        vr.render(c2w, intr, step=step, export=True, want_hyp=True)
        frames.append(_snapshot(vr))
    whole = frames[0]
    names = PLANES + ("pred_hyp",)
    for planes, rgb8, depth16, mm16 in frames[1:]:
        assert all(same_bits(planes[k], whole[0][k]) for k in names)
        assert torch.equal(rgb8, whole[1]) and torch.equal(depth16, whole[2]) and torch.equal(mm16, whole[3])
    # the exports are the planes': to8b, to16b(depth * fp32(1 / far)) and the millimetres
    assert np.array_equal(whole[1].cpu().numpy(), (255 * np.clip(whole[0]["rgb"].cpu().numpy(), 0, 1)).astype(np.uint8))
    scale = torch.tensor(np.float32(1.0) / np.float32(FAR), device=dev())
    assert np.array_equal(whole[2].cpu().numpy().view(np.uint16),
                          (65535 * np.clip((whole[0]["depth"] * scale).cpu().numpy(), 0, 1)).astype(np.uint16))
    assert np.array_equal(whole[3].cpu().numpy().view(np.uint16), _want_u16(whole[0]["depth"].cpu().numpy(), 1000.0))
    assert len(np.unique(whole[3].cpu().numpy())) > 1

    # two calls over [0, 40) and [40, 117) are one call
    vr = _renderer(P, kw, 50, 3)
    for v in list(vr.planes.values()) + [vr.pred_hyp]:
        v.fill_(777.0)
    vr.enqueue(c2w, intr, step=step, export=True, pix0=0, n_pix=40, want_hyp=True)
    vr.enqueue(c2w, intr, step=step, export=True, pix0=40, n_pix=77, want_hyp=True)
    planes, rgb8, depth16, mm16 = _snapshot(vr)
    assert all(same_bits(planes[k], whole[0][k]) for k in names)
    assert torch.equal(rgb8, whole[1]) and torch.equal(depth16, whole[2]) and torch.equal(mm16, whole[3])

    # a call over [20, 70) touches no pixel outside that range, in the fp32 planes and in the 8 / 16-bit ones
    for v in list(vr.planes.values()) + [vr.pred_hyp]:
        v.fill_(777.0)
    vr.rgb8.fill_(0xA5)
    vr.depth16.fill_(0x5A5A)
    vr.depth_mm16.fill_(0x5A5A)
    vr.enqueue(c2w, intr, step=step, export=True, pix0=20, n_pix=50, want_hyp=True)
    planes, rgb8, depth16, mm16 = _snapshot(vr)
    inside = torch.zeros(n, dtype=torch.bool, device=dev())
    inside[20:70] = True
    for k in names:
        assert same_bits(planes[k][inside], whole[0][k][inside]), k
        assert (planes[k][~inside] == 777.0).all(), k
    assert torch.equal(rgb8[inside], whole[1][inside]) and (rgb8[~inside] == 0xA5).all()
    assert torch.equal(depth16[inside], whole[2][inside]) and (depth16[~inside] == 0x5A5A).all()
    assert torch.equal(mm16[inside], whole[3][inside]) and (mm16[~inside] == 0x5A5A).all()


# ----------------------------------------------------------------------------- the sampling error
def _masks():
    gen = torch.Generator().manual_seed(21)
    random = torch.rand(H * W, generator=gen) < 0.4
    second_block_empty = random.clone()
    second_block_empty[50:100] = False      # blocks of 50: [50, 100) is the second
    return {"random": random, "all": torch.ones(H * W, dtype=torch.bool), "second_block_empty": second_block_empty}


def _present_route_rows(Dp, args, kw, valid, monkeypatch=None):
    """One view through depth.test_images_samples' present route; returns its fp64 row (sum, count) by watching the rows it
    accumulates."""
    from plnerf_amd import evaluate
    seen = []
    real = Dp.sample_error_rows

    def spy(pred_hyp, depth, valid_, **kw_):
        out = real(pred_hyp, depth, valid_, **kw_)
        seen.append(kw_["out"])
        return out
    Dp.sample_error_rows = spy
    try:
        Dp.test_images_samples(None, [0], None, None, valid[None], g(_pose())[None], H, W, _intrinsic()[None], None, args,
                               dict(kw, near=NEAR, far=FAR))
    finally:
        Dp.sample_error_rows = real
    assert seen and all(s.data_ptr() == seen[0].data_ptr() for s in seen) and evaluate.sample_error_rows is real
    return seen[0].clone()


@pytest.mark.parametrize("mask", ["random", "all", "second_block_empty"])
def test_error_row_is_the_present_routes(P, mask):
    from plnerf_amd import depth as Dp
    valid = g(_masks()[mask])
    kw = _kwargs("f16x3", test_time=True)
    args = _args("f16x3", chunk=50)
    want = _present_route_rows(Dp, args, kw, valid)
    assert int(want[1].item()) == int(valid.sum().item()) and float(want[0]) > 0
    # blocks equal to the chunk: the same blocks, added in the same fp64 order -- with and without a hypothesis plane
    vr = _renderer(P, kw, 50)
    for want_hyp in (False, True):
        _, _, _, extras = vr.render(_pose(), _intrinsic(), valid=valid, want_hyp=want_hyp)
        assert torch.equal(extras["sample_error_row"], want), (mask, want_hyp, extras["sample_error_row"].tolist(), want.tolist())
        assert ("pred_hyp" in extras) == want_hyp
    # other blocks: another order of the same additions
    hyp, depth = extras["pred_hyp"].clone(), extras["depth_map"].clone()
    s64, c64 = ref64.sample_error(hyp, depth, valid.view(H, W))
    for chunk in (32, 117):
        row = _renderer(P, kw, chunk).render(_pose(), _intrinsic(), valid=valid)[3]["sample_error_row"].tolist()
        print(f"error_row {mask} chunk {chunk}: {row} fp64 {s64, c64} rel {abs(row[0] - s64) / abs(s64):.3e}")
        assert row[1] == c64 and abs(row[0] - s64) <= KERNEL_REL * abs(s64), (mask, chunk, row, s64, c64)
    # two calls over the frame accumulate into the row the caller zeroed once
    vr.error_row.zero_()
    vr.enqueue(_pose(), _intrinsic(), pix0=0, n_pix=50, valid=valid)
    vr.enqueue(_pose(), _intrinsic(), pix0=50, n_pix=67, valid=valid)
    assert torch.equal(vr.error_row, want)


def _scene(V=3):
    import plnerf_amd as P_
    intrinsics = torch.tensor([[11.3, 9.7, 6.1, 4.3], [12.1, 10.4, 6.6, 4.9], [10.7, 11.2, 5.8, 3.9]], device=dev())[:V]
    poses = torch.stack([P_.rays.pose_spherical(a, -30.0, 4.0) for a in (10.0, 70.0, 250.0)]).to(dev())[:V]
    rng = np.random.default_rng(12)
    images = torch.from_numpy(rng.random((V, H, W, 3), dtype=np.float32)).to(dev())
    depths = torch.from_numpy((rng.random((V, H, W, 1), dtype=np.float32) * 3 + 2.5)).to(dev())
    valid = torch.from_numpy(rng.random((V, H, W)) < 0.4).to(dev())
    valid[1] = False                               # a view without a valid pixel: NaN in the reference, skipped
    return images, depths, valid, poses, intrinsics


def test_keyword_route_of_test_images_samples(P):
    from plnerf_amd import depth as Dp
    images, depths, valid, poses, intrinsics = _scene()
    kw = dict(_kwargs("f16x3", test_time=True), near=NEAR, far=FAR)
    args = _args("f16x3", chunk=50)
    a = Dp.test_images_samples(None, [0, 1, 2], images, depths, valid, poses, H, W, intrinsics, None, args, kw, one_call=True)
    b = Dp.test_images_samples(None, [0, 1, 2], images, depths, valid, poses, H, W, intrinsics, None, args, kw, one_call=False)
    c = Dp.test_images_samples(None, [0, 1, 2], images, depths, valid, poses, H, W, intrinsics, None, args, kw)
    assert a.total_weight == b.total_weight == c.total_weight == 2
    assert a.as_dict() == b.as_dict() == c.as_dict() and list(a.as_dict()) == ["importance_sampling_error"]
    assert math.isfinite(a.get("importance_sampling_error")) and a.get("importance_sampling_error") > 0
    # a configuration the call does not serve takes the present route silently
    cam_args = _args("f16x3", chunk=50, input_ch_cam=0)
    joint = dict(kw, is_joint=True)
    d = Dp.test_images_samples(None, [0, 2], images, depths, valid, poses, H, W, intrinsics, None, cam_args, joint, one_call=True)
    e = Dp.test_images_samples(None, [0, 2], images, depths, valid, poses, H, W, intrinsics, None, cam_args, joint)
    assert d.as_dict() == e.as_dict()
    # ... and so do kwargs that ask for draws: the renderer's would be its own, not the present route's
    assert Dp._view_renderer(kw, H, W, args) is not None and Dp._view_renderer(joint, H, W, args) is None
    assert Dp._view_renderer(dict(kw, perturb=1.0), H, W, args) is None
    assert Dp._view_renderer(dict(kw, raw_noise_std=0.5), H, W, args) is None
    torch.manual_seed(3)
    f = Dp.test_images_samples(None, [0, 2], images, depths, valid, poses, H, W, intrinsics, None, args, dict(kw, perturb=1.0),
                               one_call=True)
    torch.manual_seed(3)
    h = Dp.test_images_samples(None, [0, 2], images, depths, valid, poses, H, W, intrinsics, None, args, dict(kw, perturb=1.0))
    assert f.as_dict() == h.as_dict() and f.as_dict() != a.as_dict()


def test_keyword_route_of_render_images_with_metrics(P):
    from plnerf_amd import depth as Dp
    images, depths, valid, poses, intrinsics = _scene()
    valid[1] = valid[0]
    kw = dict(_kwargs("f16x3", test_time=True), near=NEAR, far=FAR)
    args = _args("f16x3", chunk=50)
    run = lambda **more: Dp.render_images_with_metrics(None, [0, 1, 2], images, depths, valid, poses, H, W, intrinsics, None, args,
                                                       kw, **more)
    (ma, ra), (mb, rb) = run(one_call=True), run()
    assert ma.as_dict() == mb.as_dict() and {"psnr", "ssim", "depth_rmse", "psnr0"} <= set(ma.as_dict())
    assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra)


# ----------------------------------------------------------------------------- render_video_frames
def test_render_video_frames_writes_render_videos_files(P, tmp_path):
    """Four poses on the 9 x 13 view (each of the two staging sets is used twice), per-view intrinsics, jitter and density
    noise on: the files are exactly '{idx}.png' in either directory, and each decodes to to8b(rgb) / the millimetre codes of
    the frame DepthViewRenderer.render(pose, intrinsic, step=idx) gives -- the colour in rgb_dir, the depth in depth_dir."""
    kw = dict(_kwargs("f16x3", **CASES["noise_half"]), near=NEAR, far=FAR)
    n = 4
    poses = torch.stack([P.rays.pose_spherical(a, -30.0, 4.0) for a in (10.0, 70.0, 130.0, 250.0)])
    intrinsics = torch.tensor([[11.3, 9.7, 6.1, 4.3], [12.1, 10.4, 6.6, 4.9], [10.7, 11.2, 5.8, 3.9], [11.9, 9.1, 6.3, 4.6]])
    rgb_dir, depth_dir = tmp_path / "video", tmp_path / "video_depth"
    assert P.render_video_frames(g(poses), H, W, g(intrinsics), str(rgb_dir), str(depth_dir), kw, 50, seed=6) == n
    names = sorted(f"{i}.png" for i in range(n))
    assert sorted(os.listdir(str(rgb_dir))) == names and sorted(os.listdir(str(depth_dir))) == names
    vr = _renderer(P, {k: v for k, v in kw.items() if k not in ("near", "far")}, 50, seed=6)
    frames = []
    for i in range(n):
        rgb, _, _, extras = vr.render(poses[i, :3, :4], intrinsics[i], step=i, export=True)
        want8 = (255 * np.clip(rgb.cpu().numpy(), 0, 1)).astype(np.uint8)
        want16 = _want_u16(extras["depth_map"].cpu().numpy(), 1000.0)
        assert np.array_equal(extras["rgb8"].cpu().numpy(), want8)
        assert np.array_equal(extras["depth_mm16"].cpu().numpy().view(np.uint16), want16)
        got8, got16 = P.read_png(str(rgb_dir / f"{i}.png")), P.read_png(str(depth_dir / f"{i}.png"))
        assert got8.dtype == np.uint8 and got8.shape == (H, W, 3) and np.array_equal(got8, want8), i
        assert got16.dtype == np.uint16 and got16.shape == (H, W) and np.array_equal(got16, want16), i
        assert len(np.unique(want16)) > 1 and not np.array_equal(got16, extras["depth16"].cpu().numpy().view(np.uint16))      # millimetres, not depth / far
        frames.append(want16)
    assert not np.array_equal(frames[0], frames[1])
    # one intrinsic for every pose; no pose: nothing rendered, nothing written, 0 returned
    one = tmp_path / "one"
    assert P.render_video_frames(poses[:2], H, W, INTRINSIC, str(one / "rgb"), str(one / "depth"), kw, 117, seed=6) == 2
    assert np.array_equal(P.read_png(str(one / "depth" / "0.png")), frames[0])      # (INTRINSIC is view 0's; blocks of 117, not 50)
    assert sorted(os.listdir(str(one / "rgb"))) == ["0.png", "1.png"]
    none = tmp_path / "none"
    assert P.render_video_frames(poses[:0], H, W, intrinsics[:0], str(none / "rgb"), str(none / "depth"), kw, 50) == 0
    assert not none.exists()
    # a network outside the half range does not pass silently: the status words ride along with the frame
    from plnerf_amd import depth as Dp
    bad, _, _, _, _ = Dp.create_nerf(_args("f16x3"), device=dev())
    sd = orc.closed_form_state_dict_depth(0, True)
    sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * 6.0e4
    sd["pts_linears.1.weight"] = sd["pts_linears.1.weight"] * 1.0e-5
    bad["network_fn"].load_state_dict(sd)
    bad["network_fine"].load_state_dict(orc.closed_form_state_dict_depth(1, True))
    with pytest.raises(FloatingPointError, match="coarse network"):
        P.render_video_frames(poses[:3], H, W, intrinsics[:3], str(tmp_path / "b" / "rgb"), str(tmp_path / "b" / "depth"),
                              dict(bad, near=NEAR, far=FAR), 50)


# ----------------------------------------------------------------------------- the range guard
def test_a_network_outside_the_half_range_raises_and_the_word_clears(P):
    from plnerf_amd import depth as Dp
    kw, _, _, _, _ = Dp.create_nerf(_args("f16x3"), device=dev())
    sd = orc.closed_form_state_dict_depth(0, True)      # (tests/test_gpu_depth_one_call.py's network: the first layer's
    sd["pts_linears.0.weight"] = sd["pts_linears.0.weight"] * 6.0e4      # activations pass 65504, the weights do not)
    sd["pts_linears.1.weight"] = sd["pts_linears.1.weight"] * 1.0e-5
    assert float(sd["pts_linears.0.weight"].abs().max()) < 65504.0
    kw["network_fn"].load_state_dict(sd)
    kw["network_fine"].load_state_dict(orc.closed_form_state_dict_depth(1, True))
    vr = _renderer(P, kw, 50)
    with pytest.raises(FloatingPointError, match="coarse network"):
        vr.render(_pose(), _intrinsic())
    assert [int(w.item()) for w in vr.status_words()] == [0, 0]
    vr.enqueue(_pose(), _intrinsic())
    assert int(vr.status_words()[0].item()) != 0 and int(vr.status_words()[1].item()) == 0
    with pytest.raises(FloatingPointError):
        vr.check_range()
    vr.check_range()      # the word cleared


# ----------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("build", [b for _, b in cases.all_cases()], ids=[i for i, _ in cases.all_cases()])
def test_guard_bands(build):
    """tests/test_gpu_containment.py's conditions (a)-(f) for the three device-writing entries of the experimental header."""
    from plnerf_amd import _lib as L
    L.lib()
    results = C.run_case(L, build(L), dev())
    if "mm16_odd" in results:      # the value in front of the call's output is what it was
        odd = results["mm16_odd"].view(torch.int16)
        assert int(odd[0]) == cases.KEPT and torch.equal(odd[1:], results["mm16"].view(torch.int16))
    if "error_row0" in results:
        full, part = results["error_row0"].view(torch.float64), results["error_row1"].view(torch.float64)
        assert 0 < float(part[1]) < float(full[1]) <= cases.H * cases.W and float(part[0]) > 0


# ----------------------------------------------------------------------------- a host without Python
@pytest.mark.parametrize("precision", ["f16x3"])
def test_c_host_renders_without_python(P, precision, tmp_path):
    """tests/c_abi_depth_view_gpu.cpp -- the HIP runtime and the experimental header, nothing else -- renders the 9 x 13 view
    in blocks of 32 from the tables written here; DepthViewRenderer on the same inputs produces the same bytes."""
    from plnerf_amd import _lib as L_
    from plnerf_amd import functional as Fn
    exe = c_hosts.build("c_abi_depth_view_gpu", tmp_path)
    kw = _kwargs(precision, **CASES["white_bkgd"])
    valid = _masks()["random"]
    blobs = []
    for net in (kw["network_fn"], kw["network_fine"]):
        params = [p.detach().cpu().contiguous() for p in net.param_list()]
        assert [tuple(p.shape) for p in params] == [tuple(shape) for _, shape in orc.param_shapes_depth()]      # state_dict order
        blobs += [p.numpy().tobytes() for p in params]
    blobs += [Fn.cpu_linspace(NS, "cpu").numpy().tobytes(), Fn.cpu_linspace(NI, "cpu").numpy().tobytes(),
              valid.to(torch.uint8).numpy().tobytes()]
    (tmp_path / "inputs.bin").write_bytes(b"".join(blobs))
    run = c_hosts.run(exe, L_.PRECISION[precision], L_.FWD_KERNEL, tmp_path / "inputs.bin")
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])      # (no retry)
    host = c_hosts.parse_planes(run.stdout)

    c2w = torch.tensor([[0.8, -0.6, 0.0, 0.1], [0.6, 0.8, 0.0, -0.2], [0.0, 0.0, 1.0, 4.0]])
    vr = _renderer(P, kw, 32, seed=11)
    rgb, _, _, extras = vr.render(c2w, _intrinsic(), step=3, export=True, valid=g(valid), want_hyp=True)
    assert torch.isfinite(rgb).all()
    mine = {name: vr.planes[name] for name in PLANES}
    mine.update(pred_hyp=vr.pred_hyp, rgb8=vr.rgb8, depth16=vr.depth16, depth_mm16=vr.depth_mm16, error_row=vr.error_row)
    assert set(host) == set(mine)
    for name, t in mine.items():
        assert c_hosts.fnv1a(t.cpu().numpy().tobytes()) == host[name], name
