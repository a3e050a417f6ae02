"""Importance-sampling error on the GPU: plnerf_sample_error against the fp64 restatement (tests/sampleerr_fp64.py) over
ray counts, hypothesis counts and valid masks; bit-reproducibility; a frame scored chunk by chunk with `accumulate`
against one call; R = 0; the error codes; and depth.test_images_samples end to end against a restatement of the
reference's loop (whole-frame render, then :396-411 in torch) on closed-form networks, linear and constant modes."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

import sampleerr_fp64 as ref
from gpu_support import P, dev
from oracle import plnerf_oracle as orc

pytestmark = pytest.mark.gpu

KERNEL_REL = 1e-12      # the kernel's fp64 sum against the fp64 restatement (another order of the same additions)


def _rays(R, N, seed, offset=0):
    """(pred_hyp [R,N], depth [R]) fp32 on the device: depths in [2, 6), hypotheses spread around them (both signs of
    h - d).  offset > 0 places pred_hyp `offset` floats into its buffer (not 16-B aligned: the kernel's scalar path)."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    depth = torch.rand(R, device=dev(), generator=g) * 4 + 2
    buf = torch.empty(offset + R * N, device=dev())
    hyp = buf[offset:].view(R, N)
    hyp.copy_(depth[:, None] + torch.randn(R, N, device=dev(), generator=g) * 0.5)
    return hyp, depth


def _masks(R, seed):
    g = torch.Generator(device=dev()).manual_seed(seed + 1)
    return {"empty": torch.zeros(R, dtype=torch.bool, device=dev()), "full": torch.ones(R, dtype=torch.bool, device=dev()),
            "random": torch.rand(R, device=dev(), generator=g) < 0.3, "none": None}


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("R", [1, 37, 32768, 640000])
@pytest.mark.parametrize("N", [1, 63, 64, 128, 192])
def test_kernel_against_fp64_restatement(P, R, N):
    L = P._lib
    hyp, depth = _rays(R, N, R * 7 + N)
    for name, valid in _masks(R, R + N).items():
        row = P.sample_error_rows(hyp, depth, valid).cpu().tolist()
        s, c = ref.sample_error(hyp, depth, valid)
        assert row[L.SAMPLEERR_COUNT] == c, name
        if c == 0:
            assert row[L.SAMPLEERR_SUM] == 0.0, name
        else:
            assert _rel(row[L.SAMPLEERR_SUM], s) <= KERNEL_REL, (name, row, s)
        print(f"\nSAMPLEERR R={R} N={N} {name}: sum_rel {_rel(row[0], s) if c else 0.0:.3e} count {c}")


@pytest.mark.parametrize("N", [64, 128])
def test_unaligned_hypotheses_take_the_scalar_path(P, N):
    """The same values from a pred_hyp 4 bytes into its buffer (no 16-B vector loads) as from an aligned copy."""
    R = 4099
    hyp, depth = _rays(R, N, 5, offset=1)
    valid = _masks(R, 5)["random"]
    a = P.sample_error_rows(hyp, depth, valid)
    b = P.sample_error_rows(hyp.clone(), depth, valid)
    s, c = ref.sample_error(hyp, depth, valid)
    assert a[1] == b[1] == c
    assert _rel(float(a[0]), s) <= KERNEL_REL and _rel(float(b[0]), s) <= KERNEL_REL


def test_nan_in_an_uncounted_ray_is_not_read(P):
    hyp, depth = _rays(300, 64, 9)
    valid = torch.ones(300, dtype=torch.bool, device=dev())
    hyp[17, 5] = float("nan")
    depth[200] = float("nan")
    valid[17] = valid[200] = False
    row = P.sample_error_rows(hyp, depth, valid).cpu().tolist()
    s, c = ref.sample_error(hyp, depth, valid)
    assert row[1] == c == 298 and _rel(row[0], s) <= KERNEL_REL
    valid[17] = True
    assert math.isnan(float(P.sample_error_rows(hyp, depth, valid)[0]))


def test_bit_reproducible(P):
    hyp, depth = _rays(640000, 128, 21)
    valid = _masks(640000, 21)["random"]
    ws = torch.empty(P._lib.sample_error_workspace_bytes(640000), dtype=torch.uint8, device=dev())
    first = P.sample_error_rows(hyp, depth, valid, workspace=ws).clone()
    for _ in range(5):
        again = P.sample_error_rows(hyp, depth, valid, workspace=ws)
        assert torch.equal(again.view(torch.int64), first.view(torch.int64))


@pytest.mark.parametrize("chunk", [32768, 10007])
def test_chunked_accumulate_equals_one_call(P, chunk):
    R, N = 640000, 128
    hyp, depth = _rays(R, N, 33)
    valid = _masks(R, 33)["random"]
    whole = P.sample_error_rows(hyp, depth, valid).cpu().tolist()
    row = torch.zeros(P._lib.SAMPLEERR_ROW, dtype=torch.float64, device=dev())
    ws = torch.empty(P._lib.sample_error_workspace_bytes(chunk), dtype=torch.uint8, device=dev())
    for first in range(0, R, chunk):
        P.sample_error_rows(hyp[first:first + chunk], depth[first:first + chunk], valid[first:first + chunk], out=row,
                            workspace=ws, accumulate=True)
    chunked = row.cpu().tolist()
    assert chunked[1] == whole[1]
    assert _rel(chunked[0], whole[0]) <= 1e-13, (chunked, whole)


def test_empty_input(P):
    L = P._lib
    empty_h, empty_d = torch.empty(0, 128, device=dev()), torch.empty(0, device=dev())
    row = torch.tensor([1.25, 7.0], dtype=torch.float64, device=dev())
    before = row.clone()
    P.sample_error_rows(empty_h, empty_d, torch.empty(0, dtype=torch.bool, device=dev()), out=row, accumulate=True)
    P.sample_error_rows(empty_h, empty_d, out=row, accumulate=True)
    assert torch.equal(row.view(torch.int64), before.view(torch.int64))
    P.sample_error_rows(empty_h, empty_d, out=row)                 # overwrite: zeros
    assert row.cpu().tolist() == [0.0, 0.0]
    rc = L.lib().plnerf_sample_error(0, 64, None, None, None, 1, None, L.dptr(row, "row", torch.float64), L.stream())
    assert rc == 0


def test_error_codes(P):
    L = P._lib
    EINVAL, ERANGE = -1, -3
    hyp, depth = _rays(100, 64, 3)
    row = torch.zeros(2, dtype=torch.float64, device=dev())
    ws = torch.empty(L.sample_error_workspace_bytes(100), dtype=torch.uint8, device=dev())
    h, d, w, r = (L.dptr(hyp), L.dptr(depth), L.dptr(ws, "ws", torch.uint8), L.dptr(row, "row", torch.float64))
    f = L.lib().plnerf_sample_error
    s = L.stream()
    assert f(100, 64, h, d, None, 0, w, r, s) == 0
    assert f(100, 64, h, d, None, 0, w, None, s) == EINVAL          # row
    assert f(100, 64, None, d, None, 0, w, r, s) == EINVAL          # pred_hyp
    assert f(100, 64, h, None, None, 0, w, r, s) == EINVAL          # depth
    assert f(100, 64, h, d, None, 0, None, r, s) == EINVAL          # workspace
    assert f(-1, 64, h, d, None, 0, w, r, s) == ERANGE              # R < 0
    assert f(100, 0, h, d, None, 0, w, r, s) == ERANGE              # N < 1
    assert f(100, 1025, h, d, None, 0, w, r, s) == ERANGE           # N > PLNERF_SAMPLEERR_MAX_N
    with pytest.raises(RuntimeError, match="plnerf_sample_error"):
        P.sample_error_rows(torch.zeros(4, 1025, device=dev()), torch.zeros(4, device=dev()))
    torch.cuda.synchronize()


# ---- depth.test_images_samples
def _setup(P, mode, n_samples, n_importance, chunk):
    from plnerf_amd import depth as Dp
    args = Namespace(multires=9, i_embed=0, use_viewdirs=True, multires_views=0, input_ch_cam=0,
                     N_importance=n_importance, N_samples=n_samples, netdepth=8, netwidth=256, netdepth_fine=8,
                     netwidth_fine=256, netchunk=65536, lrate=5e-4, perturb=1.0, white_bkgd=True, raw_noise_std=0.0,
                     mode=mode, color_mode="midpoint", lindisp=False, no_reload=True, precision="fp32", bb_center=0.0,
                     bb_scale=1.0, chunk=chunk, dataset="scannet")
    _, kw, _, _, _ = Dp.create_nerf(args, device=dev())
    kw["network_fn"].load_state_dict(orc.closed_form_state_dict_depth(0, True))
    kw["network_fine"].load_state_dict(orc.closed_form_state_dict_depth(1, True))
    kw.update(near=2.0, far=6.0)
    return Dp, args, kw


def _running_mean(values):
    m, w = 0, 0
    for v in values:
        m, w = (m * w + v) / (w + 1.0), w + 1.0
    return m


@pytest.mark.parametrize("mode,n_samples,n_importance", [("linear", 32, 48), ("constant", 16, 40)])
def test_test_images_samples_end_to_end(P, mode, n_samples, n_importance, monkeypatch):
    H, W, V, chunk = 10, 14, 4, 48      # 140 rays per view: three chunks, the last one short
    Dp, args, kw = _setup(P, mode, n_samples, n_importance, chunk)
    intrinsics = torch.tensor([[14.0, 14.0, W / 2, H / 2], [12.0, 13.0, W / 2 + 0.5, H / 2 - 0.5],
                               [16.0, 15.0, W / 2 - 1.0, H / 2], [13.0, 13.0, W / 2, H / 2 + 1.0]], device=dev())
    poses = torch.stack([P.rays.pose_spherical(a, -30.0, 4.0) for a in (10.0, 70.0, 130.0, 250.0)]).to(dev())
    rng = np.random.default_rng(12)
    images = torch.from_numpy(rng.random((V, H, W, 3), dtype=np.float32)).to(dev())
    depths = torch.from_numpy((rng.random((V, H, W, 1), dtype=np.float32) * 3 + 2.5)).to(dev())
    valid = torch.from_numpy(rng.random((V, H, W)) < 0.4).to(dev())
    valid[2] = False                               # a view without a valid pixel: NaN in the reference, skipped

    scored = []
    real = Dp.sample_error_rows

    def spy(pred_hyp, depth, valid_, **kw_):
        scored.append((pred_hyp.clone(), depth.clone(), valid_.clone()))
        return real(pred_hyp, depth, valid_, **kw_)
    monkeypatch.setattr(Dp, "sample_error_rows", spy)
    metrics = Dp.test_images_samples(None, [0, 1, 2, 3], images, depths, valid, poses, H, W, intrinsics, None, args, kw)
    monkeypatch.setattr(Dp, "sample_error_rows", real)
    m = metrics.as_dict()
    assert list(m) == ["importance_sampling_error"] and metrics.total_weight == 3

    # the reference's loop: the whole frame rendered, then :396-411 in torch (fp32)
    ref_values, fp64_values = [], []
    with torch.no_grad():
        for i in range(V):
            _, _, _, ex = Dp.render(H, W, intrinsics[i], chunk=chunk, c2w=poses[i, :3, :4], **kw)
            N = ex["pred_hyp"].shape[-1]
            assert N == n_importance
            # the chunks test_images_samples scored are this render's hypotheses and depths, bit for bit
            mine = scored[3 * i:3 * i + 3]
            assert [t[0].shape[0] for t in mine] == [48, 48, 44]
            assert torch.equal(torch.cat([t[0] for t in mine]), ex["pred_hyp"].reshape(-1, N))
            assert torch.equal(torch.cat([t[1] for t in mine]), ex["depth_map"].reshape(-1))
            assert torch.equal(torch.cat([t[2] for t in mine]), valid[i].reshape(-1))
            v = ref.reference_view_mean(ex["pred_hyp"], ex["depth_map"], valid[i])
            if not torch.isnan(v):
                ref_values.append(v.item())
                s, c = ref.sample_error(ex["pred_hyp"], ex["depth_map"], valid[i])
                fp64_values.append(s / c)
    assert len(scored) == 3 * V and len(ref_values) == 3
    assert _rel(m["importance_sampling_error"], _running_mean(ref_values)) <= 1e-6
    assert _rel(m["importance_sampling_error"], _running_mean(fp64_values)) <= KERNEL_REL

    # count: np.random.choice under the caller's seed, as render_images_with_metrics
    np.random.seed(4)
    m2 = Dp.test_images_samples(2, [0, 1, 2, 3], images, depths, valid, poses, H, W, intrinsics, None, args, kw)
    np.random.seed(4)
    chosen = [int(i) for i in np.random.choice([0, 1, 2, 3], size=2, replace=False)]
    picked = [fp64_values[[0, 1, 3].index(i)] for i in chosen if i != 2]
    assert m2.total_weight == len(picked)
    if picked:
        assert _rel(m2.get("importance_sampling_error"), _running_mean(picked)) <= KERNEL_REL
    with pytest.raises(NotImplementedError):
        Dp.test_images_samples(None, [0], images, depths, valid, poses, H, W, intrinsics, None, args, kw,
                               with_test_time_optimization=True)
