"""Importance-sampling error without a GPU: the C ABI of include/plnerf_hip_sampleerr.h (plain C99, links against the
library, argument validation before any device work, ctypes binding _lib.SAMPLEERR_SIGNATURES argument by argument,
the workspace size), and the fp64 restatement the GPU tests compare the kernel with, pinned to closed forms and to the
reference's fp32 expression."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import sampleerr_fp64 as ref      # noqa: E402

HEADER = os.path.join(ROOT, "include", "plnerf_hip_sampleerr.h")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "pl-nerf_amd", "libplnerf_hip.so")):
        ge.build()
    from plnerf_amd import _lib
    return _lib


def _prototypes(path):
    code = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"^(int|size_t|const char\*)\s+(plnerf_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.M | re.S):
        params = [re.match(r"^(.*?)\b\w+$", a).group(1).strip()
                  for a in (x.strip() for x in " ".join(args.split()).split(",")) if a != "void"]
        protos[name] = (ret, params)
    return protos


def _c_class(t):
    t = t.replace("const ", "").strip()
    if t.endswith("*") or t == "plnerf_stream_t":
        return "ptr"
    return {"int": "i32", "float": "f32", "uint64_t": "u64", "uint32_t": "u32", "int64_t": "i64", "size_t": "u64",
            "double": "f64"}[t]


def _ct_class(t):
    if t is ctypes.c_char_p or t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return {ctypes.c_int: "i32", ctypes.c_float: "f32", ctypes.c_uint64: "u64", ctypes.c_uint32: "u32",
            ctypes.c_int64: "i64", ctypes.c_double: "f64"}[t]


def test_ctypes_signatures_match_the_sampleerr_header(L):
    protos = _prototypes(HEADER)
    assert set(protos) == set(L.SAMPLEERR_SIGNATURES) == {"plnerf_sample_error", "plnerf_sample_error_workspace_bytes"}
    assert not set(protos) & (set(L.SIGNATURES) | set(L.BATCHING_SIGNATURES) | set(L.EVAL_SIGNATURES) |
                              set(L.DEPTHFEED_SIGNATURES))
    for name, (ret, params) in protos.items():
        res, args = L.SAMPLEERR_SIGNATURES[name]
        assert _ct_class(res) == _c_class(ret)
        assert [_ct_class(t) for t in args] == [_c_class(c) for c in params], name
    assert L.ABI_VERSION == 601 and L.lib().plnerf_version() == 601
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
    src = tmp_path / "sampleerr_abi.c"
    src.write_text(_C)
    exe = str(tmp_path / "sampleerr_abi")
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe, "-L", libdir, "-lplnerf_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
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
