"""The C ABI of the use_batching ray source (include/plnerf_hip_batching.h), without a GPU: the header is plain C99 and
links against the library with the declared prototype, its argument validation runs before any device work, and the
ctypes binding (_lib.BATCHING_SIGNATURES) matches the header argument by argument -- the checks tests/abi_check.c and
test_host_cpu.py apply to plnerf_hip.h."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "plnerf_hip_batching.h")


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


def test_ctypes_signatures_match_the_batching_header(L):
    protos = _prototypes(HEADER)
    assert set(protos) == set(L.BATCHING_SIGNATURES) == {"plnerf_select_bank_rays"}
    assert not set(protos) & set(L.SIGNATURES)
    for name, (ret, params) in protos.items():
        res, args = L.BATCHING_SIGNATURES[name]
        assert _ct_class(res) == _c_class(ret)
        assert [_ct_class(t) for t in args] == [_c_class(c) for c in params], name
    assert L.ABI_VERSION == 601 and L.lib().plnerf_version() == 601


_C = r"""
#include <stdio.h>
#include "plnerf_hip_batching.h"

int main(void) {
    int (*p)(int, const int*, int, int, float, float, float, float, const float*, const float*, uint64_t, uint32_t, int,
             int, float, float, float*, float*, float*, float*, float*, float*, int*, plnerf_stream_t) =
        plnerf_select_bank_rays;
    int views[1] = {0};
    float dummy[12] = {0};
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION < 601) return 2;
    /* validation before any device work: these calls never touch the (absent) GPU */
    if (p(0, views, 4, 4, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 1, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy, NULL,
          NULL, NULL) != PLNERF_EINVAL) return 3;
    if (p(1, NULL, 4, 4, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 1, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy, NULL,
          NULL, NULL) != PLNERF_EINVAL) return 4;
    /* M = 3 * 12 * 17 = 612: positions [600, 613) run past the epoch */
    if (p(3, views, 12, 17, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 600, 13, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy,
          NULL, NULL, NULL) != PLNERF_ERANGE) return 5;
    /* M = 2 * 32768 * 32768 = 2^31 > 2^30 */
    if (p(2, views, 32768, 32768, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 1, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy,
          NULL, NULL, NULL) != PLNERF_ERANGE) return 6;
    /* nothing to do */
    if (p(3, views, 12, 17, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 612, 0, 0.f, 1.f, NULL, NULL, NULL, NULL, NULL, NULL,
          NULL, NULL) != PLNERF_OK) return 7;
    if (p(3, views, 12, 17, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 4, 0.f, 1.f, NULL, NULL, NULL, NULL, NULL, NULL,
          NULL, NULL) != PLNERF_EINVAL) return 8;
    printf("batching abi ok\n");
    return 0;
}
"""


def test_batching_header_is_plain_c_and_links(L, tmp_path):
    src = tmp_path / "batching_abi.c"
    src.write_text(_C)
    exe = str(tmp_path / "batching_abi")
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", exe, "-L", libdir, "-lplnerf_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "batching abi ok" in out.stdout
