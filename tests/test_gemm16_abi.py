"""The experimental header include/experimental/plnerf_hip_gemm16.h, without a GPU, as tests/test_dpstep_abi.py holds its
header: the one row of the fifth table _lib.GEMM16_HEADERS against the header's prototype and the library's exports, the
signature argument by argument, what lib() bound, every refusal that comes before a launch (through the binding and from a
C99 host) -- and that the four existing tables and the ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi

HEADER = "experimental/plnerf_hip_gemm16.h"
ENTRIES = {"plnerf_gemm_h16"}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
EXPERIMENTAL = ("experimental/plnerf_hip_depthview.h",)
CAMCODE = ("experimental/plnerf_hip_camcode.h",)
DPSTEP = ("experimental/plnerf_hip_dpstep.h",)
OK, EINVAL, ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.GEMM16_HEADERS) == 1
    header, signatures, mirrors = L.GEMM16_HEADERS[0]
    assert header == HEADER and mirrors == {}
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def test_names_agree(L, row):
    path, signatures, _ = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES == set(L.GEMM16_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert not abi.structs(path)


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type: a scalar is that ctypes type, every pointer and the
    stream are c_void_p (the entry takes no struct)."""
    path, signatures, _ = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == 14, (name, len(args), len(params))
        assert params[-1] == "plnerf_stream_t" and ret == "int"
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[abi.bare(c_type)], (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The fifth table shares no name with the other four and adds nothing to them."""
    others = set(L.ALL_SIGNATURES) | set(L.EXPERIMENTAL_SIGNATURES) | set(L.CAMCODE_TABLE_SIGNATURES) | set(L.DPSTEP_TABLE_SIGNATURES)
    assert not set(L.GEMM16_TABLE_SIGNATURES) & others
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert tuple(header for header, _, _ in L.EXPERIMENTAL_HEADERS) == EXPERIMENTAL
    assert tuple(header for header, _, _ in L.CAMCODE_HEADERS) == CAMCODE
    assert tuple(header for header, _, _ in L.DPSTEP_HEADERS) == DPSTEP
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES):
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)


def test_refusals_come_before_any_launch(L):
    """Through the binding, without a device, on fake pointers that are never followed (a launch here would be
    PLNERF_ELAUNCH): every argument error, the fp32 code, the grid limit -- and the empty products, which are PLNERF_OK."""
    fn = L.lib().plnerf_gemm_h16
    p = ctypes.c_void_p(4096)
    f16x3 = L.PRECISION["f16x3"]

    def call(a=p, lda=8, w=p, ldw=8, bias=p, M=4, N=4, K=8, relu=1, precision=f16x3, c=p, ldc=4, status=None):
        return fn(a, lda, w, ldw, bias, M, N, K, relu, precision, c, ldc, status, None)
    for bad in (dict(M=-1), dict(N=-1), dict(K=-1), dict(lda=7), dict(ldw=7), dict(ldc=3), dict(c=None), dict(a=None),
                dict(w=None), dict(precision=L.PRECISION["fp32"]), dict(precision=5), dict(precision=-1)):
        assert call(**bad) == EINVAL, bad
    assert call(M=0) == OK and call(N=0) == OK and call(M=0, a=None, w=None) == OK
    # more than 2^31 - 1 tiles of 128 x 128: refused, not wrapped
    assert call(M=2 ** 31 - 1, N=2 ** 31 - 1, ldc=2 ** 31 - 1) == ERANGE
    for name in ("bf16x3", "bf16", "f16x3", "f16"):      # (every 16-bit mode is accepted as far as the checks go)
        assert call(precision=L.PRECISION[name], M=0) == OK


_C = r"""
#include <stdio.h>
#include "experimental/plnerf_hip_gemm16.h"

/* never dereferenced: every call below is refused by the argument checks, or is an empty product */
static float host[64];

int main(void) {
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    if (plnerf_gemm_h16(host, 8, host, 8, host, 4, 4, 8, 1, PLNERF_PREC_FP32, host, 4, NULL, NULL) != PLNERF_EINVAL) return 3;
    if (plnerf_gemm_h16(host, 7, host, 8, host, 4, 4, 8, 1, PLNERF_PREC_F16X3, host, 4, NULL, NULL) != PLNERF_EINVAL) return 4;
    if (plnerf_gemm_h16(host, 8, host, 8, host, 4, 4, 8, 1, PLNERF_PREC_BF16X3, NULL, 4, NULL, NULL) != PLNERF_EINVAL) return 5;
    if (plnerf_gemm_h16(NULL, 8, host, 8, NULL, 4, 4, 8, 0, PLNERF_PREC_F16, host, 4, NULL, NULL) != PLNERF_EINVAL) return 6;
    if (plnerf_gemm_h16(host, 8, host, 8, NULL, 0, 4, 8, 0, PLNERF_PREC_BF16, host, 4, NULL, NULL) != PLNERF_OK) return 7;
    if (plnerf_gemm_h16(host, 8, host, 8, NULL, 4, 0, 8, 0, PLNERF_PREC_BF16, host, 0, NULL, NULL) != PLNERF_OK) return 8;
    printf("gemm16 abi ok\n");
    return 0;
}
"""


def test_header_is_plain_c_and_the_checks_come_first(L, tmp_path_factory):
    exe = abi.compile_c(_C, tmp_path_factory.mktemp("gemm16_abi"), "gemm16_abi")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "gemm16 abi ok" in out.stdout


def test_the_switch_exists_and_is_off(L):
    from plnerf_amd import generic
    assert generic.HONOUR_PRECISION is False
