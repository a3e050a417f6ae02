"""The experimental header include/experimental/plnerf_hip_unique.h, without a GPU, as tests/test_generic_fwd_abi.py holds its
header: the one row of the tenth table _lib.UNIQUE_HEADERS against the header's prototypes, its struct and the library's
exports, the signatures argument by argument, what lib() bound, every refusal that comes before a launch (through the binding
and from a C99 host) -- and that the nine existing tables and the ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi

HEADER = "experimental/plnerf_hip_unique.h"
ENTRIES = {"plnerf_mlp_unique_workspace_bytes", "plnerf_mlp_unique_layout", "plnerf_mlp_fwd_unique_served", "plnerf_mlp_fwd_unique",
           "plnerf_mlp_unique_fold"}
ARGUMENTS = {"plnerf_mlp_unique_workspace_bytes": 1, "plnerf_mlp_unique_layout": 2, "plnerf_mlp_fwd_unique_served": 6,
             "plnerf_mlp_fwd_unique": 15, "plnerf_mlp_unique_fold": 4}
ENQUEUES = {"plnerf_mlp_fwd_unique", "plnerf_mlp_unique_fold"}      # the entries that take a stream
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
OTHER_EXPERIMENTAL = {"EXPERIMENTAL_HEADERS": ("experimental/plnerf_hip_depthview.h",),
                      "CAMCODE_HEADERS": ("experimental/plnerf_hip_camcode.h",),
                      "DPSTEP_HEADERS": ("experimental/plnerf_hip_dpstep.h",),
                      "GEMM16_HEADERS": ("experimental/plnerf_hip_gemm16.h",),
                      "GEMM16_BWD_HEADERS": ("experimental/plnerf_hip_gemm16_bwd.h",),
                      "GENERIC_FWD_HEADERS": ("experimental/plnerf_hip_generic.h",),
                      "GENERIC_TRAIN_HEADERS": ("experimental/plnerf_hip_generic_train.h",),
                      "ANYVIEW_HEADERS": ("experimental/plnerf_hip_anyview.h",)}
OK, EINVAL, ENOSYS = 0, -1, -4


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.UNIQUE_HEADERS) == 1
    header, signatures, mirrors = L.UNIQUE_HEADERS[0]
    assert header == HEADER and set(mirrors) == {"plnerf_unique_layout"}
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def _others(L):
    return (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES,
            L.GEMM16_TABLE_SIGNATURES, L.GEMM16_BWD_TABLE_SIGNATURES, L.GENERIC_FWD_TABLE_SIGNATURES,
            L.GENERIC_TRAIN_TABLE_SIGNATURES, L.ANYVIEW_TABLE_SIGNATURES)


def test_names_agree(L, row):
    path, signatures, mirrors = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES == set(L.UNIQUE_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert set(abi.structs(path)) == set(mirrors)


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type: a scalar is that ctypes type, a pointer to the header's
    struct is a POINTER to its mirror, every other pointer and the stream c_void_p."""
    path, signatures, mirrors = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == ARGUMENTS[name], (name, len(args), len(params))
        assert ret == ("size_t" if name.endswith("_bytes") else "int")
        assert (params[-1] == "plnerf_stream_t") == (name in ENQUEUES), name
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            bare = abi.bare(c_type)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[bare], (where, c_type, ct)
            elif bare.rstrip("*").strip() in mirrors:
                assert ct is ctypes.POINTER(mirrors[bare.rstrip("*").strip()]), (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)


def test_the_struct_mirror_agrees(L, row):
    path, _, mirrors = row
    for name, fields in abi.structs(path).items():
        mirror = mirrors[name]
        assert [f for f, _ in mirror._fields_] == [f for _, f, _ in fields], name
        for (c_type, field, length), (_, ct) in zip(fields, mirror._fields_):
            assert length is None and ct is abi.SCALARS[abi.bare(c_type)], (name, field, c_type, ct)
    assert ctypes.sizeof(L.UniqueLayout) == 10 * ctypes.sizeof(ctypes.c_size_t)


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The tenth table shares no name with the other nine and adds nothing to them."""
    others = set().union(*[set(t) for t in _others(L)])
    assert not set(L.UNIQUE_TABLE_SIGNATURES) & others
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    for table, headers in OTHER_EXPERIMENTAL.items():
        assert tuple(header for header, _, _ in getattr(L, table)) == headers, table
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in _others(L):
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)


def test_refusals_come_before_any_launch(L):
    """Through the binding, without a device, on fake pointers that are never followed (a launch here would be
    PLNERF_ELAUNCH): every argument error of the two enqueuing entries -- and the empty call, which is PLNERF_OK."""
    fwd, fold = L.lib().plnerf_mlp_fwd_unique, L.lib().plnerf_mlp_unique_fold
    p = ctypes.c_void_p(4096)
    f16x3 = L.PRECISION["f16x3"]

    def call(packed=p, precision=f16x3, pts=p, vd=p, in_ch=63, view_ch=27, n=387, spr=3, scale=1.0, beta=0.0, raw=p, saved=p,
             kernel=0, ws=p):
        return fwd(packed, precision, pts, vd, in_ch, view_ch, n, spr, scale, beta, raw, saved, kernel, ws, None)
    for bad in (dict(packed=None), dict(pts=None), dict(vd=None), dict(raw=None), dict(raw=ctypes.c_void_p(4096 + 4)), dict(ws=None),
                dict(ws=ctypes.c_void_p(4096 + 16)), dict(n=-1), dict(spr=0), dict(spr=2), dict(n=388), dict(kernel=7),
                dict(kernel=L.FWD_KERNELS["pp"]), dict(in_ch=62), dict(in_ch=0), dict(view_ch=26), dict(view_ch=33), dict(scale=0.0),
                dict(beta=-1.0), dict(precision=L.PRECISION["fp32"]), dict(precision=L.PRECISION["f16"]),
                dict(precision=L.PRECISION["bf16"])):
        assert call(**bad) == EINVAL, bad
    assert call(precision=9) == ENOSYS
    assert call(n=0) == OK and call(n=0, packed=None, pts=None, vd=None, raw=None, ws=None) == OK
    found = os.environ.get("PLNERF_FWD_UNIQUE")
    os.environ["PLNERF_FWD_UNIQUE"] = "0"      # switched off: the entry refuses, the caller takes plnerf_mlp_fwd
    try:
        assert call() == EINVAL
    finally:
        os.environ.pop("PLNERF_FWD_UNIQUE")
        if found is not None:
            os.environ["PLNERF_FWD_UNIQUE"] = found
    for bad in (dict(g=None), dict(g=ctypes.c_void_p(4096 + 8)), dict(n=0), dict(n=-3), dict(ws=None), dict(ws=ctypes.c_void_p(4096 + 128))):
        kw = dict(dict(g=p, n=387, ws=p), **bad)
        assert fold(kw["g"], kw["n"], kw["ws"], None) == EINVAL, bad


_C = r"""
#include <stdio.h>
#include "experimental/plnerf_hip_unique.h"

/* never dereferenced by the device: every call below is refused by the argument checks, or is empty */
static float host[64];

int main(void) {
    plnerf_unique_layout lo;
    char* ws = (char*)4096;
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    if (plnerf_mlp_unique_layout(387, &lo) != PLNERF_OK || lo.total != plnerf_mlp_unique_workspace_bytes(387)) return 3;
    if (lo.words != 0 || lo.rows_u % 256 || lo.g_raw_u % 256 || lo.absmax >= lo.total || lo.n_absmax != 1) return 4;
    if (plnerf_mlp_unique_layout(0, &lo) != PLNERF_EINVAL || plnerf_mlp_unique_workspace_bytes(0) != 0) return 5;
    if (plnerf_mlp_fwd_unique_served(PLNERF_PREC_FP32, 0, PLNERF_FWD_KERNEL_AUTO, 192, 786432, 1) != 0) return 6;
    if (plnerf_mlp_fwd_unique_served(PLNERF_PREC_F16X3, 1, PLNERF_FWD_KERNEL_AUTO, 192, 786432, 1) != 0) return 7;
    if (plnerf_mlp_fwd_unique_served(PLNERF_PREC_F16X3, 0, PLNERF_FWD_KERNEL_PP, 192, 786432, 1) != 0) return 8;
    if (plnerf_mlp_fwd_unique(host, PLNERF_PREC_FP32, host, host, 63, 27, 387, 3, 1.0f, 0.0f, host, NULL, PLNERF_FWD_KERNEL_AUTO, ws,
                              NULL) != PLNERF_EINVAL) return 9;
    if (plnerf_mlp_fwd_unique(host, PLNERF_PREC_F16X3, host, host, 63, 27, 387, 3, 1.0f, 0.0f, host, NULL, PLNERF_FWD_KERNEL_AUTO, ws + 8,
                              NULL) != PLNERF_EINVAL) return 10;
    if (plnerf_mlp_fwd_unique(host, PLNERF_PREC_BF16X3, host, host, 63, 27, 0, 3, 1.0f, 0.0f, host, NULL, PLNERF_FWD_KERNEL_AUTO, ws,
                              NULL) != PLNERF_OK) return 11;
    if (plnerf_mlp_unique_fold(NULL, 387, ws, NULL) != PLNERF_EINVAL) return 12;
    printf("unique abi ok\n");
    return 0;
}
"""


def test_header_is_plain_c_and_the_checks_come_first(L, tmp_path_factory):
    exe = abi.compile_c(_C, tmp_path_factory.mktemp("unique_abi"), "unique_abi")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "unique abi ok" in out.stdout


def test_the_switch_is_mirrored_in_the_module(L):
    from plnerf_amd import functional
    assert functional.FWD_UNIQUE is (os.environ.get("PLNERF_FWD_UNIQUE") != "0") and functional.FINE_QUERY is False
