"""Held-out view metrics on the GPU: plnerf_eval_metrics against the fp64 restatement (tests/eval_fp64.py) over frame
sizes, clamping, constant and identical images, rgb0 and depth masks; bit-reproducibility across calls and batch
sizes; render_images_with_metrics end to end (NVS and depth-supervised variants) on closed-form networks."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import eval_fp64 as ref
from gpu_support import P, dev
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu

SSIM_ABS, SSE_REL = 1e-6, 1e-6


def _frame(kind, H, W, seed):
    """(pred, target, pred0) [H,W,3] fp32 numpy."""
    rng = np.random.default_rng(seed)
    t = rng.random((H, W, 3), dtype=np.float32)
    p = (rng.random((H, W, 3), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)     # outside [0, 1] on both sides
    p0 = (rng.random((H, W, 3), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    if kind == "constant":
        t = np.full((H, W, 3), 0.75, np.float32)
        p = np.full((H, W, 3), 0.25, np.float32)
    elif kind == "identical":
        p = t.copy()
    elif kind == "smooth":           # a target near its prediction: SSIM close to 1, where cancellation would show
        p = np.clip(t + rng.normal(0, 0.02, t.shape).astype(np.float32), -0.05, 1.05).astype(np.float32)
    return p, t, p0


def _mask(kind, H, W, seed):
    rng = np.random.default_rng(seed + 100)
    return {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool),
            "random": rng.random((H, W)) < 0.3}[kind]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


CASES = [(H, W, kind, mask, with0) for (H, W) in ((7, 7), (8, 12), (37, 53), (800, 800))
         for kind, mask, with0 in (("random", "random", True), ("random", "empty", False), ("constant", "full", True),
                                   ("identical", "random", False), ("smooth", "full", True))]


@pytest.mark.parametrize("H,W,kind,mask,with0", CASES)
def test_kernel_against_fp64_restatement(P, H, W, kind, mask, with0):
    L = P._lib
    seed = H * 1000 + W
    p, t, p0 = _frame(kind, H, W, seed)
    rng = np.random.default_rng(seed + 7)
    d = (rng.random((H, W), dtype=np.float32) * 4 + 2).astype(np.float32)
    td = (d + rng.normal(0, 0.1, (H, W))).astype(np.float32)
    v = _mask(mask, H, W, seed)
    g = lambda a: torch.from_numpy(a).to(dev())
    row = P.metric_rows(g(p), g(t), g(p0) if with0 else None, g(d), g(td), g(v)).cpu().numpy()[0]

    e_ssim = abs(row[L.EVAL_SSIM] - ref.ssim(p, t))
    e_sse = _rel(row[L.EVAL_SSE_RGB], ref.sse(p, t))
    assert e_ssim <= SSIM_ABS and e_sse <= SSE_REL, (e_ssim, e_sse)
    e_sse0 = 0.0
    if with0:
        e_sse0 = _rel(row[L.EVAL_SSE_RGB0], ref.sse(p0, t))
        assert e_sse0 <= SSE_REL
    else:
        assert np.isnan(row[L.EVAL_SSE_RGB0])
    dsse, count = ref.depth_sums(d, td, v)
    assert row[L.EVAL_DEPTH_COUNT] == count
    e_depth = _rel(row[L.EVAL_DEPTH_SSE], dsse) if count else abs(row[L.EVAL_DEPTH_SSE])
    assert e_depth <= SSE_REL
    if kind == "identical":
        assert row[L.EVAL_SSE_RGB] == 0.0 and abs(row[L.EVAL_SSIM] - 1.0) <= 1e-12
    if kind == "constant":
        a, b = 0.25, 0.75
        assert abs(row[L.EVAL_SSIM] - (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)) <= 1e-12
    # (the measured errors, for DESIGN.md: `pytest -s` prints them)
    print(f"\nEVALERR {H}x{W} {kind} {mask} rgb0={with0}: ssim_abs {e_ssim:.3e} sse_rel {e_sse:.3e} "
          f"sse0_rel {e_sse0:.3e} depth_rel {e_depth:.3e}")

    m = P.image_metrics(g(p), g(t), g(p0) if with0 else None, g(d), g(td), g(v))
    assert list(m)[:3] == ["img_loss", "psnr", "ssim"]
    assert ("img_loss0" in m) == with0 and ("depth_rmse" in m) == (count > 0)
    assert m["img_loss"] == row[L.EVAL_SSE_RGB] / (3 * H * W)


def test_no_depth_gives_no_depth_rmse(P):
    p, t, _ = _frame("random", 9, 10, 3)
    g = lambda a: torch.from_numpy(a).to(dev())
    m = P.image_metrics(g(p), g(t))
    assert list(m) == ["img_loss", "psnr", "ssim"]
    with pytest.raises(RuntimeError):
        P.image_metrics(g(p[:6]), g(t[:6]))        # smaller than one 7x7 window: PLNERF_EINVAL
    with pytest.raises(ValueError):
        P.image_metrics(g(p), g(t), depth=g(p[..., 0]))


def test_bit_reproducible_and_batch_independent(P):
    H, W, n = 123, 201, 3
    rng = np.random.default_rng(11)
    p = torch.from_numpy((rng.random((n, H, W, 3), dtype=np.float32) * 1.4 - 0.2)).to(dev())
    t = torch.from_numpy(rng.random((n, H, W, 3), dtype=np.float32)).to(dev())
    p0 = torch.from_numpy(rng.random((n, H, W, 3), dtype=np.float32)).to(dev())
    d = torch.from_numpy(rng.random((n, H, W), dtype=np.float32)).to(dev())
    td = torch.from_numpy(rng.random((n, H, W), dtype=np.float32)).to(dev())
    v = torch.from_numpy(rng.random((n, H, W)) < 0.5).to(dev())
    a = P.metric_rows(p, t, p0, d, td, v)
    b = P.metric_rows(p, t, p0, d, td, v)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    singles = torch.cat([P.metric_rows(p[i], t[i], p0[i], d[i], td[i], v[i]) for i in range(n)])
    assert torch.equal(a.view(torch.int64), singles.view(torch.int64))
    for i in range(n):      # and each row is its frame's
        assert abs(float(a[i, P._lib.EVAL_SSIM]) - ref.ssim(p[i].cpu().numpy(), t[i].cpu().numpy())) <= SSIM_ABS


# ---- render_images_with_metrics
def _nvs_setup(P, H, W):
    emb_fn, _ = P.get_embedder(10, 0)
    embd_fn, _ = P.get_embedder(4, 0)
    qfn = lambda inputs, viewdirs, fn: P.run_network(inputs, viewdirs, fn, emb_fn, embd_fn)

    def net(i):
        n = P.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        n.load_state_dict(orc.closed_form_state_dict(i, True))
        return n.to(dev())
    kw = dict(network_query_fn=qfn, perturb=0.0, N_importance=16, network_fine=net(1), N_samples=16, network_fn=net(0),
              white_bkgd=True, raw_noise_std=0.0, mode="linear", color_mode="midpoint", ndc=False, near=2.0, far=6.0,
              use_viewdirs=True)
    f = 14.0
    K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
    poses = torch.stack([P.rays.pose_spherical(a, -30.0, 4.0) for a in (0.0, 40.0, 80.0, 120.0)]).to(dev())
    rng = np.random.default_rng(4)
    images = rng.random((4, H, W, 3), dtype=np.float32)
    return kw, K, poses, images


def _running_mean(values):
    m, w = 0, 0
    for v in values:
        m, w = (m * w + v) / (w + 1.0), w + 1.0
    return m


def test_render_images_with_metrics_nvs(P):
    H, W = 12, 16
    kw, K, poses, images = _nvs_setup(P, H, W)
    args = Namespace(dataset="blender", chunk=64)
    indices = np.array([0, 1, 2, 3])
    calls = []

    def lpips_stub(a, b, normalize=False):
        calls.append((tuple(a.shape), tuple(b.shape), normalize, float(a.min()), float(a.max())))
        return ((a - b).abs().mean() * 0.5 + 0.125).reshape(1, 1, 1, 1)

    np.random.seed(5)
    metrics, res = P.render_images_with_metrics(2, indices, images, None, None, poses, H, W, K, lpips_stub, args, kw)
    np.random.seed(5)
    chosen = np.random.choice(indices, size=2, replace=False)
    m = metrics.as_dict()
    assert list(m) == ["img_loss", "psnr", "ssim", "lpips", "img_loss0", "psnr0"]
    assert list(res) == ["rgbs", "target_rgbs", "depths", "target_depths", "target_valid_depths", "rgbs0", "depths0"]
    assert res["rgbs"].shape == (2, 3, H, W) and res["depths"].shape == (2, 1, H, W) and res["rgbs"].device.type == "cpu"
    assert torch.equal(res["target_rgbs"], torch.from_numpy(images[chosen]).permute(0, 3, 1, 2))
    assert not res["target_valid_depths"].any() and not res["target_depths"].any()

    # white_bkgd keeps rgb and rgb0 in [0, 1]: clamping changes nothing, so res's frames are the scored ones
    rgbs, rgbs0, depths = [], [], []
    with torch.no_grad():
        for i in chosen:
            rgb, _, _, ex = P.render(H, W, K, chunk=64, c2w=poses[i, :3, :4], **kw)
            for x in (rgb, ex["rgb0"]):
                assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
            rgbs.append(rgb.cpu().numpy()); rgbs0.append(ex["rgb0"].cpu().numpy()); depths.append((ex["depth_map"] / 6.0).cpu())
    for n in range(2):
        assert np.array_equal(res["rgbs"][n].permute(1, 2, 0).numpy(), rgbs[n])
        assert np.array_equal(res["rgbs0"][n].permute(1, 2, 0).numpy(), rgbs0[n])
        assert torch.equal(res["depths"][n, 0], depths[n])
    frames = [res["rgbs"][n].permute(1, 2, 0).numpy() for n in range(2)]
    frames0 = [res["rgbs0"][n].permute(1, 2, 0).numpy() for n in range(2)]
    targets = [images[i] for i in chosen]
    mse = [ref.sse(f, t) / (3 * H * W) for f, t in zip(frames, targets)]
    mse0 = [ref.sse(f, t) / (3 * H * W) for f, t in zip(frames0, targets)]
    assert _rel(m["img_loss"], _running_mean(mse)) <= SSE_REL
    assert _rel(m["img_loss0"], _running_mean(mse0)) <= SSE_REL
    assert abs(m["psnr"] - _running_mean([-10 * np.log10(x) for x in mse])) <= 1e-5
    assert abs(m["psnr0"] - _running_mean([-10 * np.log10(x) for x in mse0])) <= 1e-5
    assert abs(m["ssim"] - _running_mean([ref.ssim(f, t) for f, t in zip(frames, targets)])) <= SSIM_ABS

    # the stub saw the clamped frame and the target, [1,3,H,W], normalize=True; its [0,0,0] was recorded
    assert len(calls) == 2 and all(c[:3] == ((1, 3, H, W), (1, 3, H, W), True) and c[3] >= 0 and c[4] <= 1 for c in calls)
    stub = [float(np.abs(f - t).mean()) * 0.5 + 0.125 for f, t in zip(frames, targets)]
    assert abs(m["lpips"] - _running_mean(stub)) <= 1e-6

    # no LPIPS network: the key is left out; keep_images=False: the same metrics, no res; count=None: every view in order
    np.random.seed(5)
    m2, res2 = P.render_images_with_metrics(2, indices, images, None, None, poses, H, W, K, None, args, kw,
                                            keep_images=False)
    assert res2 is None
    assert m2.as_dict() == {k: v for k, v in m.items() if k != "lpips"}
    m3, res3 = P.render_images_with_metrics(None, indices, torch.from_numpy(images).to(dev()), None, None, poses, H, W,
                                            K, None, args, kw)
    assert torch.equal(res3["target_rgbs"], torch.from_numpy(images).permute(0, 3, 1, 2))
    assert "depth_rmse" not in m3.as_dict()


def test_render_images_with_metrics_depth_variant(P, golden):
    from plnerf_amd import depth as Dp
    gd = golden("g8_depth_variant")
    args = Namespace(multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0,
                     N_importance=int(gd["N_importance"]), N_samples=int(gd["N_samples"]), netdepth=8, netwidth=256,
                     netdepth_fine=8, netwidth_fine=256, netchunk=65536, lrate=5e-4, perturb=1.0, white_bkgd=True,
                     raw_noise_std=0.0, mode="linear", color_mode="midpoint", lindisp=False, no_reload=True,
                     precision="fp32", bb_center=0.0, bb_scale=1.0, chunk=96, dataset="scannet")
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev())
    kw["network_fn"].load_state_dict(orc.closed_form_state_dict_depth(0, True))
    kw["network_fine"].load_state_dict(orc.closed_form_state_dict_depth(1, True))
    kw.update(near=2.0, far=6.0)
    H, W, N = 10, 14, 3
    intrinsics = torch.tensor([[14.0, 14.0, W / 2, H / 2], [12.0, 13.0, W / 2 + 0.5, H / 2 - 0.5],
                               [16.0, 15.0, W / 2 - 1.0, H / 2]], device=dev())
    poses = torch.stack([P.rays.pose_spherical(a, -30.0, 4.0) for a in (10.0, 70.0, 130.0)]).to(dev())
    rng = np.random.default_rng(8)
    images = torch.from_numpy(rng.random((N, H, W, 3), dtype=np.float32)).to(dev())
    depths = torch.from_numpy((rng.random((N, H, W, 1), dtype=np.float32) * 3 + 2.5)).to(dev())
    valid = torch.from_numpy(rng.random((N, H, W)) < 0.4).to(dev())
    valid[1] = False                               # a view without a valid depth: no term for it, as in the reference

    metrics, res = Dp.render_images_with_metrics(None, [0, 1, 2], images, depths, valid, poses, H, W, intrinsics, None,
                                                 args, kw)
    m = metrics.as_dict()
    assert list(m) == ["img_loss", "psnr", "ssim", "img_loss0", "psnr0", "depth_rmse"]
    rmse, ssims = [], []
    with torch.no_grad():
        for i in range(N):
            rgb, _, _, ex = Dp.render(H, W, intrinsics[i], chunk=96, c2w=poses[i, :3, :4], **kw)
            assert torch.equal(res["depths"][i, 0], (ex["depth_map"] / 6.0).cpu())
            assert torch.equal(res["target_valid_depths"][i, 0], valid[i].cpu())
            dsse, count = ref.depth_sums(ex["depth_map"].cpu().numpy(), depths[i, :, :, 0].cpu().numpy(), valid[i].cpu().numpy())
            if count:
                rmse.append(np.sqrt(dsse / count))
            ssims.append(ref.ssim(rgb.cpu().numpy(), images[i].cpu().numpy()))
    assert len(rmse) == 2
    assert _rel(m["depth_rmse"], _running_mean(rmse)) <= SSE_REL
    assert abs(m["ssim"] - _running_mean(ssims)) <= SSIM_ABS
    with pytest.raises(NotImplementedError):
        Dp.render_images_with_metrics(None, [0], images, depths, valid, poses, H, W, intrinsics, None, args, kw,
                                      with_test_time_optimization=True)
