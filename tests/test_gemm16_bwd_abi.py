"""The experimental header include/experimental/plnerf_hip_gemm16_bwd.h, without a GPU, as tests/test_gemm16_abi.py holds the
forward's: the one row of the sixth table _lib.GEMM16_BWD_HEADERS against the header's prototypes and the library's exports,
the signatures argument by argument (15 for dgrad, 17 for wgrad), what lib() bound, every refusal that comes before a launch
(through the binding and from a C99 host) -- and that the five existing tables and the ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi

HEADER = "experimental/plnerf_hip_gemm16_bwd.h"
ENTRIES = {"plnerf_gemm_h16_dgrad": 15, "plnerf_gemm_h16_wgrad": 17}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
EXPERIMENTAL = ("experimental/plnerf_hip_depthview.h",)
CAMCODE = ("experimental/plnerf_hip_camcode.h",)
DPSTEP = ("experimental/plnerf_hip_dpstep.h",)
GEMM16 = ("experimental/plnerf_hip_gemm16.h",)
OK, EINVAL, ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.GEMM16_BWD_HEADERS) == 1
    header, signatures, mirrors = L.GEMM16_BWD_HEADERS[0]
    assert header == HEADER and mirrors == {}
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def test_names_agree(L, row):
    path, signatures, _ = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == set(ENTRIES) == set(L.GEMM16_BWD_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert not abi.structs(path)


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type: a scalar is that ctypes type, every pointer and the
    stream are c_void_p (the entries take no struct)."""
    path, signatures, _ = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == ENTRIES[name], (name, len(args), len(params))
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
    """The sixth table shares no name with the other five and adds nothing to them."""
    tables = (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES,
              L.GEMM16_TABLE_SIGNATURES)
    assert not set(L.GEMM16_BWD_TABLE_SIGNATURES) & set().union(*map(set, tables))
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert tuple(header for header, _, _ in L.EXPERIMENTAL_HEADERS) == EXPERIMENTAL
    assert tuple(header for header, _, _ in L.CAMCODE_HEADERS) == CAMCODE
    assert tuple(header for header, _, _ in L.DPSTEP_HEADERS) == DPSTEP
    assert tuple(header for header, _, _ in L.GEMM16_HEADERS) == GEMM16
    assert set(L.GEMM16_TABLE_SIGNATURES) == {"plnerf_gemm_h16"} and len(L.GEMM16_TABLE_SIGNATURES["plnerf_gemm_h16"][1]) == 14
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in tables:
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint(L.GEMM16_BWD_TABLE_SIGNATURES, {**table, "plnerf_gemm_h16_wgrad": None})


def test_dgrad_refusals_come_before_any_launch(L):
    """Through the binding, without a device, on fake pointers that are never followed (a launch here would be
    PLNERF_ELAUNCH): every argument error, the fp32 code, the grid limit -- and the empty products, which are PLNERF_OK."""
    fn = L.lib().plnerf_gemm_h16_dgrad
    p = ctypes.c_void_p(4096)
    f16x3 = L.PRECISION["f16x3"]

    def call(g=p, ldg=4, y=p, ldy=4, w=p, ldw=8, M=4, N=4, K=8, precision=f16x3, absmax=p, dx=p, lddx=8, status=None):
        return fn(g, ldg, y, ldy, w, ldw, M, N, K, precision, absmax, dx, lddx, status, None)
    for bad in (dict(M=-1), dict(N=-1), dict(K=-1), dict(ldg=3), dict(ldy=3), dict(ldw=7), dict(lddx=7), dict(dx=None),
                dict(g=None), dict(w=None), dict(precision=L.PRECISION["fp32"]), dict(precision=5), dict(precision=-1)):
        assert call(**bad) == EINVAL, bad
    # ldy is checked only when y is given; an empty output is PLNERF_OK whatever the operands
    assert call(M=0, y=None, ldy=0) == OK and call(M=0) == OK and call(K=0, ldw=0, lddx=0) == OK
    assert call(M=0, g=None, w=None) == OK
    # more than 2^31 - 1 tiles of 128 x 128: refused, not wrapped
    assert call(M=2 ** 31 - 1, K=2 ** 31 - 1, ldw=2 ** 31 - 1, lddx=2 ** 31 - 1) == ERANGE
    for name in ("bf16x3", "bf16", "f16x3", "f16"):      # (every 16-bit mode is accepted as far as the checks go)
        assert call(precision=L.PRECISION[name], M=0) == OK


def test_wgrad_refusals_come_before_any_launch(L):
    fn = L.lib().plnerf_gemm_h16_wgrad
    p = ctypes.c_void_p(4096)
    f16x3 = L.PRECISION["f16x3"]

    def call(g=p, ldg=4, y=p, ldy=4, x=p, ldx=8, M=4, N=4, K=8, precision=f16x3, absmax=p, dwb=p, lddwb=9, k_splits=1,
             partials=None, status=None):
        return fn(g, ldg, y, ldy, x, ldx, M, N, K, precision, absmax, dwb, lddwb, k_splits, partials, status, None)
    for bad in (dict(M=-1), dict(N=-1), dict(K=-1), dict(ldg=3), dict(ldy=3), dict(ldx=7), dict(lddwb=8), dict(dwb=None),
                dict(g=None), dict(x=None), dict(k_splits=2), dict(precision=L.PRECISION["fp32"]), dict(precision=5),
                dict(precision=-1)):
        assert call(**bad) == EINVAL, bad
    assert call(N=0, ldg=0, y=None, ldy=0) == OK and call(N=0, ldg=0, ldy=0, g=None, x=None) == OK
    assert call(N=0, ldg=0, ldy=0, k_splits=3, partials=p) == OK
    # more than 2^31 - 1 workgroups: tiles alone, and tiles times k_splits
    big = 2 ** 31 - 2
    assert call(N=big, ldg=big, ldy=big, K=big, ldx=big, lddwb=big + 1) == ERANGE
    assert call(N=4096, ldg=4096, ldy=4096, K=4095, ldx=4095, lddwb=4096, k_splits=2 ** 22, partials=p) == ERANGE      # 1024 tiles
    for name in ("bf16x3", "bf16", "f16x3", "f16"):
        assert call(precision=L.PRECISION[name], N=0, ldg=0, ldy=0) == OK


_C = r"""
#include <stdio.h>
#include "experimental/plnerf_hip_gemm16_bwd.h"

/* never dereferenced: every call below is refused by the argument checks, or is an empty product */
static float host[64];

int main(void) {
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    if (plnerf_gemm_h16_dgrad(host, 4, host, 4, host, 8, 4, 4, 8, PLNERF_PREC_FP32, host, host, 8, NULL, NULL) != PLNERF_EINVAL) return 3;
    if (plnerf_gemm_h16_dgrad(host, 3, NULL, 0, host, 8, 4, 4, 8, PLNERF_PREC_F16X3, host, host, 8, NULL, NULL) != PLNERF_EINVAL) return 4;
    if (plnerf_gemm_h16_dgrad(host, 4, host, 3, host, 8, 4, 4, 8, PLNERF_PREC_F16X3, NULL, host, 8, NULL, NULL) != PLNERF_EINVAL) return 5;
    if (plnerf_gemm_h16_dgrad(host, 4, NULL, 0, host, 8, 4, 4, 8, PLNERF_PREC_BF16X3, NULL, NULL, 8, NULL, NULL) != PLNERF_EINVAL) return 6;
    if (plnerf_gemm_h16_dgrad(NULL, 4, NULL, 0, host, 8, 4, 4, 8, PLNERF_PREC_F16, NULL, host, 8, NULL, NULL) != PLNERF_EINVAL) return 7;
    if (plnerf_gemm_h16_dgrad(host, 4, NULL, 0, host, 8, 0, 4, 8, PLNERF_PREC_BF16, NULL, host, 8, NULL, NULL) != PLNERF_OK) return 8;
    if (plnerf_gemm_h16_dgrad(host, 4, NULL, 0, host, 0, 4, 4, 0, PLNERF_PREC_BF16, NULL, host, 0, NULL, NULL) != PLNERF_OK) return 9;
    if (plnerf_gemm_h16_wgrad(host, 4, host, 4, host, 8, 4, 4, 8, PLNERF_PREC_FP32, host, host, 9, 1, NULL, NULL, NULL) != PLNERF_EINVAL) return 10;
    if (plnerf_gemm_h16_wgrad(host, 4, NULL, 0, host, 8, 4, 4, 8, PLNERF_PREC_F16X3, host, host, 8, 1, NULL, NULL, NULL) != PLNERF_EINVAL) return 11;
    if (plnerf_gemm_h16_wgrad(host, 4, NULL, 0, host, 8, 4, 4, 8, PLNERF_PREC_F16X3, host, host, 9, 2, NULL, NULL, NULL) != PLNERF_EINVAL) return 12;
    if (plnerf_gemm_h16_wgrad(host, 4, NULL, 0, NULL, 8, 4, 4, 8, PLNERF_PREC_BF16X3, NULL, host, 9, 1, NULL, NULL, NULL) != PLNERF_EINVAL) return 13;
    if (plnerf_gemm_h16_wgrad(host, 4, NULL, 0, host, 8, 4, 4, 8, PLNERF_PREC_BF16, NULL, NULL, 9, 1, NULL, NULL, NULL) != PLNERF_EINVAL) return 14;
    if (plnerf_gemm_h16_wgrad(host, 0, NULL, 0, host, 8, 4, 0, 8, PLNERF_PREC_BF16, NULL, host, 9, 1, NULL, NULL, NULL) != PLNERF_OK) return 15;
    printf("gemm16 bwd abi ok\n");
    return 0;
}
"""


def test_header_is_plain_c_and_the_checks_come_first(L, tmp_path_factory):
    exe = abi.compile_c(_C, tmp_path_factory.mktemp("gemm16_bwd_abi"), "gemm16_bwd_abi")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "gemm16 bwd abi ok" in out.stdout


def test_the_switch_exists_and_is_off(L):
    from plnerf_amd import generic
    assert generic.HONOUR_PRECISION_BACKWARD is False and generic.HONOUR_PRECISION is False
