"""Importance-sampling error without a GPU: the C ABI of include/plnerf_hip_sampleerr.h (plain C99, links against the
library, argument validation before any device work, the constants _lib restates, the workspace size; the signatures
themselves are compared in tests/test_abi_headers.py), and the fp64 restatement the GPU tests compare the kernel with,
pinned to closed forms and to the reference's fp32 expression."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_support as abi
import sampleerr_fp64 as ref

HEADER = os.path.join(abi.INCLUDE, "plnerf_hip_sampleerr.h")


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_sampleerr_names_and_constants_match_the_header(L):
    """The header's entry points are this table's, and the row layout and limits the binding restates are the header's.
    (Argument by argument: tests/test_abi_headers.py.)"""
    assert set(abi.prototypes(HEADER)) == set(L.SAMPLEERR_SIGNATURES) == {"plnerf_sample_error",
                                                                          "plnerf_sample_error_workspace_bytes"}
    code = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+PLNERF_SAMPLEERR_(\w+)\s+(\d+)\b", code)}
    assert consts == {"ROW": L.SAMPLEERR_ROW, "SUM": L.SAMPLEERR_SUM, "COUNT": L.SAMPLEERR_COUNT,
                      "RAYS_PER_GROUP": L.SAMPLEERR_RAYS_PER_GROUP, "MAX_N": L.SAMPLEERR_MAX_N}


@pytest.mark.parametrize("R", [-5, 0, 1, 63, 64, 65, 32768, 640000])
def test_workspace_bytes(L, R):
    assert L.lib().plnerf_sample_error_workspace_bytes(R) == L.sample_error_workspace_bytes(R) == \
        (-(-R // 64) * 16 if R > 0 else 0)


_C = r"""
#include <stdio.h>
#include "plnerf_hip_sampleerr.h"

int main(void) {
    int (*p)(int, int, const float*, const float*, const uint8_t*, int, void*, double*, plnerf_stream_t) =
        plnerf_sample_error;
    size_t (*ws)(int) = plnerf_sample_error_workspace_bytes;
    float f[4] = {0};
    uint8_t v[4] = {0};
    double row[PLNERF_SAMPLEERR_ROW] = {1.5, 2.0};
    char w[64];
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION < 601) return 2;
    /* validation before any device work: these calls never touch the (absent) GPU */
    if (p(4, 1, f, f, v, 0, w, NULL, NULL) != PLNERF_EINVAL) return 3;                    /* row NULL */
    if (p(4, 1, NULL, f, v, 0, w, row, NULL) != PLNERF_EINVAL) return 4;
    if (p(4, 1, f, NULL, v, 0, w, row, NULL) != PLNERF_EINVAL) return 5;
    if (p(4, 1, f, f, v, 0, NULL, row, NULL) != PLNERF_EINVAL) return 6;
    if (p(-1, 1, f, f, v, 0, w, row, NULL) != PLNERF_ERANGE) return 7;                    /* R < 0 */
    if (p(4, 0, f, f, v, 0, w, row, NULL) != PLNERF_ERANGE) return 8;                     /* N < 1 */
    if (p(4, PLNERF_SAMPLEERR_MAX_N + 1, f, f, v, 0, w, row, NULL) != PLNERF_ERANGE) return 9;
    /* R = 0 with accumulate: nothing to add, no launch, NULL inputs allowed */
    if (p(0, 128, NULL, NULL, NULL, 1, NULL, row, NULL) != PLNERF_OK) return 10;
    if (row[0] != 1.5 || row[1] != 2.0) return 11;
    printf("sampleerr abi ok %zu %zu %zu %zu\n", ws(0), ws(1), ws(65), ws(640000));
    return 0;
}
"""


def test_sampleerr_header_is_plain_c_and_links(L, tmp_path):
    out = subprocess.run([abi.compile_c(_C, tmp_path, "sampleerr_abi")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    sizes = [int(x) for x in out.stdout.split("sampleerr abi ok")[1].split()]
    assert sizes == [L.sample_error_workspace_bytes(R) for R in (0, 1, 65, 640000)] == [0, 16, 32, 160000]


def test_python_wrapper_checks_shapes():
    from plnerf_amd import sample_error_rows
    h, d = torch.zeros(5, 8), torch.zeros(5)
    with pytest.raises(ValueError):
        sample_error_rows(h, torch.zeros(4))                       # depth is not pred_hyp's rays
    with pytest.raises(ValueError):
        sample_error_rows(h, d, valid=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        sample_error_rows(h, d, accumulate=True)                   # nothing to add to


# ---- the fp64 restatement, pinned to closed forms
@pytest.mark.parametrize("N", [1, 3, 64, 128])
def test_restatement_constant_offset(N):
    rng = np.random.default_rng(N)
    d = torch.from_numpy(rng.random(37) * 4 + 2)
    h = d[:, None] + 0.25 * torch.ones(37, N, dtype=torch.float64)
    s, c = ref.sample_error(h, d)
    assert c == 37 and s == pytest.approx(37 * 0.25, rel=1e-14)


@pytest.mark.parametrize("N", [2, 63, 192])
def test_restatement_ramp_and_mask(N):
    d = torch.full((11,), 3.0, dtype=torch.float64)
    h = d[:, None] + torch.arange(N, dtype=torch.float64)           # |h_k - d| = k: mean (N - 1) / 2
    valid = torch.tensor([i % 3 == 0 for i in range(11)])
    s, c = ref.sample_error(h, d, valid)
    assert c == 4 and s == pytest.approx(4 * (N - 1) / 2, rel=1e-14)
    h2 = d[:, None] + torch.where(torch.arange(N) % 2 == 0, 0.5, -0.5).double()      # symmetric about d: 0.5
    assert ref.sample_error(h2, d, valid) == (pytest.approx(4 * 0.5, rel=1e-14), 4)


def test_restatement_empty_and_nan():
    d, h = torch.ones(6, dtype=torch.float64), torch.zeros(6, 4, dtype=torch.float64)
    assert ref.sample_error(h, d, torch.zeros(6, dtype=torch.bool)) == (0.0, 0)
    h[2, 1] = float("nan")
    mask = torch.ones(6, dtype=torch.bool)
    mask[2] = False
    assert ref.sample_error(h, d, mask) == (5.0, 5)                  # an uncounted NaN is not read into the sum
    assert np.isnan(ref.sample_error(h, d)[0])


def test_restatement_matches_the_reference_fp32_expression():
    g = torch.Generator().manual_seed(3)
    H, W, N = 9, 13, 64
    depth = torch.rand(H, W, generator=g) * 4 + 2
    hyp = depth[..., None] + torch.randn(H, W, N, generator=g) * 0.3
    valid = torch.rand(H, W, generator=g) < 0.5
    s, c = ref.sample_error(hyp, depth, valid)
    assert abs(float(ref.reference_view_mean(hyp, depth, valid)) - s / c) <= 1e-6 * (s / c)
    assert torch.isnan(ref.reference_view_mean(hyp, depth, torch.zeros(H, W, dtype=torch.bool)))
