"""Held-out view metrics without a GPU: the C ABI of include/plnerf_hip_eval.h (plain C99, links against the library,
argument validation before any device work, the constants _lib restates; the signatures themselves are compared in
tests/test_abi_headers.py), MeanTracker's running means, and the fp64 restatement the GPU tests compare the kernel with,
pinned to closed forms."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi_support as abi
import eval_fp64 as ref

HEADER = os.path.join(abi.INCLUDE, "plnerf_hip_eval.h")


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_eval_names_and_constants_match_the_header(L):
    """The header's entry points are this table's, and the row layout and tile constants the binding restates are the header's.
    (Argument by argument: tests/test_abi_headers.py.)"""
    assert set(abi.prototypes(HEADER)) == set(L.EVAL_SIGNATURES) == {"plnerf_eval_metrics"}
    # the row layout and tile constants the binding restates
    code = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+PLNERF_EVAL_(\w+)\s+(\d+)\b", code)}
    assert consts["ROW"] == L.EVAL_ROW and consts["TILE_H"] == L.EVAL_TILE_H and consts["TILE_W"] == L.EVAL_TILE_W
    assert [consts[k] for k in ("SSE_RGB", "SSE_RGB0", "SSIM", "DEPTH_SSE", "DEPTH_COUNT")] == [
        L.EVAL_SSE_RGB, L.EVAL_SSE_RGB0, L.EVAL_SSIM, L.EVAL_DEPTH_SSE, L.EVAL_DEPTH_COUNT]


_C = r"""
#include <stdio.h>
#include "plnerf_hip_eval.h"

int main(void) {
    int (*p)(int, int, int, const float*, const float*, const float*, const float*, const float*, const uint8_t*, void*,
             double*, plnerf_stream_t) = plnerf_eval_metrics;
    float f[4] = {0};
    uint8_t v[4] = {0};
    double rows[PLNERF_EVAL_ROW];
    char ws[64];
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION < 601) return 2;
    /* validation before any device work: these calls never touch the (absent) GPU */
    if (p(1, 6, 8, f, f, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_EINVAL) return 3;      /* H < 7 */
    if (p(1, 8, 6, f, f, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_EINVAL) return 4;      /* W < 7 */
    if (p(0, 8, 8, f, f, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_EINVAL) return 5;      /* n < 1 */
    if (p(1, 8, 8, NULL, f, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_EINVAL) return 6;
    if (p(1, 8, 8, f, NULL, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_EINVAL) return 7;
    if (p(1, 8, 8, f, f, NULL, NULL, NULL, NULL, NULL, rows, NULL) != PLNERF_EINVAL) return 8;
    if (p(1, 8, 8, f, f, NULL, NULL, NULL, NULL, ws, NULL, NULL) != PLNERF_EINVAL) return 9;
    if (p(1, 8, 8, f, f, NULL, f, f, NULL, ws, rows, NULL) != PLNERF_EINVAL) return 10;           /* partial depth */
    if (p(1, 8, 8, f, f, NULL, NULL, NULL, v, ws, rows, NULL) != PLNERF_EINVAL) return 11;
    if (p(65536, 8, 8, f, f, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_ERANGE) return 12;
    if (p(1, 32768, 16385, f, f, NULL, NULL, NULL, NULL, ws, rows, NULL) != PLNERF_ERANGE) return 13;
    printf("eval abi ok %zu %zu %zu\n", PLNERF_EVAL_WORKSPACE_BYTES(1, 7, 7), PLNERF_EVAL_WORKSPACE_BYTES(3, 800, 800),
           PLNERF_EVAL_WORKSPACE_BYTES(2, 33, 65));
    return 0;
}
"""


def test_eval_header_is_plain_c_and_links(L, tmp_path):
    out = subprocess.run([abi.compile_c(_C, tmp_path, "eval_abi")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    sizes = [int(x) for x in out.stdout.split("eval abi ok")[1].split()]
    assert sizes == [L.eval_workspace_bytes(1, 7, 7), L.eval_workspace_bytes(3, 800, 800),
                     L.eval_workspace_bytes(2, 33, 65)] == [40, 3 * 25 * 13 * 40, 2 * 2 * 2 * 40]


def test_mean_tracker_matches_the_reference_update():
    from plnerf_amd import MeanTracker
    seq = [({"psnr": 20.0, "ssim": 0.5}, 1.0), ({"psnr": 22.5, "ssim": 0.75}, 1.0), ({"psnr": 19.25}, 2.0),
           ({"psnr": 30.0, "ssim": 0.125, "lpips": 0.3}, 0.5)]
    t = MeanTracker()
    means, w = {}, 0
    for values, weight in seq:
        t.add(values, weight)
        for k, v in values.items():      # run_nerf_helpers.py:545-549, restated
            means[k] = (means.get(k, 0) * w + v) / (w + weight)
        w += weight
    assert list(t.as_dict()) == ["psnr", "ssim", "lpips"]
    for k in means:
        assert t.has(k) and t.get(k) == means[k]        # bit-equal: the same operations in the same order
    assert t.total_weight == w == 4.5
    t.reset()
    assert t.as_dict() == {} and t.total_weight == 0


def test_compute_rmse_and_psnr_helpers():
    import torch
    from plnerf_amd import compute_rmse
    from plnerf_amd.evaluate import _psnr
    a, b = torch.tensor([1.0, 2.0, 4.0]), torch.tensor([1.0, 1.0, 2.0])
    assert abs(float(compute_rmse(a, b)) - np.sqrt(5.0 / 3.0)) < 1e-6
    assert torch.isnan(compute_rmse(a[:0], b[:0]))
    assert _psnr(0.01) == pytest.approx(20.0, abs=1e-12) and _psnr(0.0) == float("inf")


# ---- the fp64 restatement, pinned to closed forms
def test_restatement_identical_images_give_one():
    rng = np.random.default_rng(0)
    x = rng.random((19, 23, 3)).astype(np.float32)
    assert ref.ssim(x, x) == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("a,b", [(0.25, 0.75), (0.0, 1.0), (0.5, 0.5), (0.9, 0.1)])
def test_restatement_constant_images(a, b):
    x, y = np.full((11, 13, 3), a, np.float32), np.full((11, 13, 3), b, np.float32)
    a64, b64 = float(np.float32(a)), float(np.float32(b))
    expect = (2 * a64 * b64 + ref.C1) / (a64 * a64 + b64 * b64 + ref.C1)
    assert ref.ssim(x, y) == pytest.approx(expect, abs=1e-12)


def test_restatement_7x7_is_one_window():
    rng = np.random.default_rng(1)
    x, y = rng.random((7, 7, 3)), rng.random((7, 7, 3))
    expect = []
    for c in range(3):
        xc, yc = x[..., c], y[..., c]
        ux, uy = xc.mean(), yc.mean()
        vx, vy = xc.var(ddof=1), yc.var(ddof=1)
        vxy = ((xc - ux) * (yc - uy)).sum() / 48.0
        expect.append((2 * ux * uy + ref.C1) * (2 * vxy + ref.C2) / ((ux ** 2 + uy ** 2 + ref.C1) * (vx + vy + ref.C2)))
    assert ref.ssim(x, y) == pytest.approx(float(np.mean(expect)), abs=1e-13)
    with pytest.raises(ValueError):
        ref.ssim(x[:6], y[:6])


def test_restatement_clamps_pred_only():
    rng = np.random.default_rng(2)
    y = rng.random((9, 9, 3))
    x = rng.random((9, 9, 3)) * 1.6 - 0.3
    assert ref.ssim(x, y) == ref.ssim(np.clip(x, 0, 1), y)
    assert ref.sse(x, y) != ref.sse(np.clip(x, 0, 1), y)
