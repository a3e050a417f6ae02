"""The experimental header include/experimental/plnerf_hip_generic.h, without a GPU, as tests/test_gemm16_abi.py holds its
header: the one row of the seventh table _lib.GENERIC_FWD_HEADERS against the header's prototypes, its struct and the
library's exports, the signatures argument by argument, what lib() bound, every refusal that comes before a launch (through
the binding and from a C99 host), the size query -- and that the six existing tables and the ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi

HEADER = "experimental/plnerf_hip_generic.h"
ENTRIES = {"plnerf_pack_h16", "plnerf_generic_fwd_workspace_bytes", "plnerf_generic_fwd"}
ARGUMENTS = {"plnerf_pack_h16": 9, "plnerf_generic_fwd_workspace_bytes": 3, "plnerf_generic_fwd": 12}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
EXPERIMENTAL = ("experimental/plnerf_hip_depthview.h",)
CAMCODE = ("experimental/plnerf_hip_camcode.h",)
DPSTEP = ("experimental/plnerf_hip_dpstep.h",)
GEMM16 = ("experimental/plnerf_hip_gemm16.h",)
GEMM16_BWD = ("experimental/plnerf_hip_gemm16_bwd.h",)
OK, EINVAL, ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.GENERIC_FWD_HEADERS) == 1
    header, signatures, mirrors = L.GENERIC_FWD_HEADERS[0]
    assert header == HEADER and set(mirrors) == {"plnerf_generic_shape"}
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def _others(L):
    return (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES,
            L.GEMM16_TABLE_SIGNATURES, L.GEMM16_BWD_TABLE_SIGNATURES)


def test_names_agree(L, row):
    path, signatures, mirrors = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES == set(L.GENERIC_FWD_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert set(abi.structs(path)) == set(mirrors)


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type: a scalar is that ctypes type, a pointer to the
    header's struct is a POINTER to its mirror, the host array of parameter pointers a POINTER(c_void_p), every other
    pointer and the stream c_void_p."""
    path, signatures, mirrors = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == ARGUMENTS[name], (name, len(args), len(params))
        assert ret == ("size_t" if name.endswith("_bytes") else "int")
        if ret == "int":
            assert params[-1] == "plnerf_stream_t"
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            bare = abi.bare(c_type)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[bare], (where, c_type, ct)
            elif bare.rstrip("*").strip() in mirrors:
                assert ct is ctypes.POINTER(mirrors[bare.rstrip("*").strip()]), (where, c_type, ct)
            elif bare.count("*") == 2:      # (const float* const* params: host memory the library follows)
                assert ct is ctypes.POINTER(ctypes.c_void_p), (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)


def test_the_struct_mirror_agrees(L, row):
    path, _, mirrors = row
    lengths = {"PLNERF_GENERIC_MAX_SKIPS": L.GENERIC_MAX_SKIPS}
    for name, fields in abi.structs(path).items():
        mirror = mirrors[name]
        assert [f for f, _ in mirror._fields_] == [f for _, f, _ in fields], name
        for (c_type, field, length), (_, ct) in zip(fields, mirror._fields_):
            want = abi.SCALARS[abi.bare(c_type)]
            assert ct is (want if length is None else want * lengths[length]), (name, field, c_type, length, ct)
    code = open(path).read()
    assert f"#define PLNERF_GENERIC_MAX_SKIPS {L.GENERIC_MAX_SKIPS}\n" in code
    assert f"#define PLNERF_GENERIC_WORKSPACE_ALIGN {L.GENERIC_WORKSPACE_ALIGN}\n" in code
    assert [L.pack_ld(k) for k in (1, 8, 9, 63, 100, 320)] == [8, 8, 16, 64, 104, 320]


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The seventh table shares no name with the other six and adds nothing to them."""
    others = set().union(*[set(t) for t in _others(L)])
    assert not set(L.GENERIC_FWD_TABLE_SIGNATURES) & others
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert tuple(header for header, _, _ in L.EXPERIMENTAL_HEADERS) == EXPERIMENTAL
    assert tuple(header for header, _, _ in L.CAMCODE_HEADERS) == CAMCODE
    assert tuple(header for header, _, _ in L.DPSTEP_HEADERS) == DPSTEP
    assert tuple(header for header, _, _ in L.GEMM16_HEADERS) == GEMM16 and set(L.GEMM16_TABLE_SIGNATURES) == {"plnerf_gemm_h16"}
    assert tuple(header for header, _, _ in L.GEMM16_BWD_HEADERS) == GEMM16_BWD
    assert set(L.GEMM16_BWD_TABLE_SIGNATURES) == {"plnerf_gemm_h16_dgrad", "plnerf_gemm_h16_wgrad"}
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in _others(L):
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)


def _shape(L, **over):
    kw = dict(D=9, W=100, input_ch=63, view_ch=27, use_viewdirs=1, output_ch=0, n_view_layers=1, skips=(4,))
    kw.update(over)
    skips = kw.pop("skips")
    s = L.GenericShape(n_skips=kw.pop("n_skips", len(skips)), **kw)
    for q, k in enumerate(skips):
        s.skips[q] = k
    return s


def _param_table(count, null_at=None):
    table = (ctypes.c_void_p * count)(*[4096] * count)
    if null_at is not None:
        table[null_at] = None
    return table


def test_the_size_query(L):
    """Restated from the header: packed weights of every layer that runs, two packed [n, W] buffers, the fp32 concatenation
    rows (one buffer; two when two skips are adjacent), every piece rounded up to 256 bytes."""
    query = L.lib().plnerf_generic_fwd_workspace_bytes

    def up(v):
        return -(-v // 256) * 256

    def packed(rows, K, planes):
        return up(planes * rows * L.pack_ld(K) * 2)

    def expect(D, W, in_ch, view_ch, viewdirs, out_ch, n_views, skips, n, planes):
        dims = [(W, in_ch if i == 0 else (in_ch + W if i - 1 in skips else W)) for i in range(D)]
        if viewdirs:
            dims += [(W // 2, W + view_ch if v == 0 else W // 2) for v in range(n_views)] + [(W, W), (1, W), (3, W // 2)]
        else:
            dims += [(out_ch, W)]
        total = sum(packed(N, K, planes) for N, K in dims) + 2 * packed(n, W, planes)
        ld = max(in_ch + W if skips else 0, W + view_ch if viewdirs else 0)
        ld = -(-ld // 4) * 4
        buffers = (1 if ld else 0) + (1 if any(k + 1 in skips for k in skips) else 0)
        return total + buffers * up(n * ld * 4)
    for name, planes in (("f16x3", 2), ("bf16x3", 2), ("f16", 1), ("bf16", 1)):
        code = L.PRECISION[name]
        assert query(ctypes.byref(_shape(L)), 129, code) == expect(9, 100, 63, 27, True, 0, 1, (4,), 129, planes)
        assert query(ctypes.byref(_shape(L, skips=(3, 4, 6))), 777, code) == expect(9, 100, 63, 27, True, 0, 1, (3, 4, 6), 777, planes)
        s = _shape(L, use_viewdirs=0, output_ch=5, view_ch=0, skips=())
        assert query(ctypes.byref(s), 300, code) == expect(9, 100, 63, 0, False, 5, 1, (), 300, planes)
        assert query(ctypes.byref(_shape(L)), 0, code) > 0
    f16x3 = L.PRECISION["f16x3"]
    assert query(ctypes.byref(_shape(L)), 129, L.PRECISION["fp32"]) == 0
    assert query(ctypes.byref(_shape(L)), -1, f16x3) == 0
    assert query(ctypes.byref(_shape(L, D=0)), 129, f16x3) == 0
    assert query(None, 129, f16x3) == 0


def test_refusals_come_before_any_launch(L):
    """Through the binding, without a device, on fake pointers that are never followed (a launch here would be
    PLNERF_ELAUNCH): every argument error of the three entries -- and the empty calls, which are PLNERF_OK."""
    fwd, query, pack = L.lib().plnerf_generic_fwd, L.lib().plnerf_generic_fwd_workspace_bytes, L.lib().plnerf_pack_h16
    p = ctypes.c_void_p(4096)
    f16x3 = L.PRECISION["f16x3"]
    n_params = 2 * (9 + 1 + 3)

    def call(shape=None, params=-1, rows=p, ld_rows=90, n=129, precision=f16x3, ws=4096, ws_bytes=None, out=p, ld_out=4, status=None):
        shape = _shape(L) if shape is None else shape
        params = _param_table(n_params) if params == -1 else params
        ref = ctypes.byref(shape) if shape is not False else None
        if ws_bytes is None:
            ws_bytes = query(ref, max(n, 0), precision) or 1 << 40
        return fwd(ref, params, rows, ld_rows, n, precision,
                   ctypes.c_void_p(ws) if ws else None, ws_bytes, out, ld_out, status, None)
    need = query(ctypes.byref(_shape(L)), 129, f16x3)
    assert need > 0
    for bad in (dict(precision=L.PRECISION["fp32"]), dict(precision=5), dict(precision=-1),
                dict(ws_bytes=need - 1), dict(ws=4096 + 4), dict(ws=4096 + 8), dict(ws=None),
                dict(shape=_shape(L, D=0)), dict(shape=_shape(L, D=-1)), dict(shape=_shape(L, W=0)), dict(shape=_shape(L, W=1)),
                dict(shape=_shape(L, input_ch=0)), dict(shape=_shape(L, view_ch=-1)), dict(shape=_shape(L, n_view_layers=0)),
                dict(shape=_shape(L, use_viewdirs=0, output_ch=0)),
                dict(shape=_shape(L, skips=(9,))), dict(shape=_shape(L, skips=(4, 10))), dict(shape=_shape(L, skips=(8,))),
                dict(shape=_shape(L, skips=(-1,))), dict(shape=_shape(L, skips=(), n_skips=17)), dict(shape=_shape(L, skips=(), n_skips=-1)),
                dict(shape=False), dict(params=None), dict(params=_param_table(n_params, null_at=0)),
                dict(params=_param_table(n_params, null_at=n_params - 1)), dict(params=_param_table(n_params, null_at=19)),
                dict(rows=None), dict(out=None), dict(n=-1), dict(ld_rows=89), dict(ld_out=3)):
        assert call(**bad) == EINVAL, bad
    assert call(ws_bytes=need, n=0) == OK and call(n=0, rows=None, out=None, ws=None, ws_bytes=0) == OK
    # without use_viewdirs the view layers' slots are not read
    plain = _shape(L, use_viewdirs=0, output_ch=5)
    assert call(shape=plain, params=_param_table(2 * (9 + 1 + 1), null_at=18), n=0, ld_out=5) == OK
    assert call(shape=plain, params=_param_table(2 * (9 + 1 + 1), null_at=20), n=0, ld_out=5) == EINVAL
    assert call(shape=plain, n=129, ld_out=4) == EINVAL
    # a dimension beyond the compiled limit, more than 2^31 - 1 tiles: refused, not wrapped
    assert call(shape=_shape(L, W=65538), n=0) == ERANGE
    assert call(shape=_shape(L, W=65536, skips=()), n=2 ** 31 - 1) == ERANGE
    for name in ("bf16x3", "bf16", "f16x3", "f16"):      # (every 16-bit mode is accepted as far as the checks go)
        assert call(precision=L.PRECISION[name], n=0) == OK

    def packs(src=p, ld=8, rows=4, K=8, precision=f16x3, dst=p, status=None, bit=L.RANGE_WEIGHT):
        return pack(src, ld, rows, K, precision, dst, status, bit, None)
    for bad in (dict(rows=-1), dict(K=-1), dict(ld=7), dict(src=None), dict(dst=None), dict(dst=ctypes.c_void_p(4096 + 4)),
                dict(precision=L.PRECISION["fp32"]), dict(precision=7), dict(bit=0), dict(bit=3), dict(bit=L.RANGE_SAVED)):
        assert packs(**bad) == EINVAL, bad
    assert packs(rows=0) == OK and packs(K=0, ld=0) == OK and packs(rows=0, bit=L.RANGE_ACTIVATION, src=None, dst=None) == OK
    assert packs(rows=2 ** 31 - 1, K=2 ** 31 - 1, ld=2 ** 31 - 1) == ERANGE


_C = r"""
#include <stdio.h>
#include <string.h>
#include "experimental/plnerf_hip_generic.h"

/* never dereferenced by the device: every call below is refused by the argument checks, or is empty */
static float host[64];

int main(void) {
    plnerf_generic_shape s;
    const float* table[26];
    const float* const* params = (const float* const*)table;
    size_t need;
    int i;
    char* ws = (char*)4096;
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    if (PLNERF_PACK_LD(63) != 64 || PLNERF_PACK_LD(64) != 64 || PLNERF_PACK_BYTES(5, 100, 2) != 2080u) return 3;
    memset(&s, 0, sizeof s);
    s.D = 9; s.W = 100; s.input_ch = 63; s.view_ch = 27; s.use_viewdirs = 1; s.n_view_layers = 1; s.n_skips = 1; s.skips[0] = 4;
    for (i = 0; i < 26; ++i) table[i] = host;
    need = plnerf_generic_fwd_workspace_bytes(&s, 129, PLNERF_PREC_F16X3);
    if (need == 0 || plnerf_generic_fwd_workspace_bytes(&s, 129, PLNERF_PREC_FP32) != 0) return 4;
    if (plnerf_generic_fwd_workspace_bytes(&s, 129, PLNERF_PREC_F16) >= need) return 5;
    if (plnerf_generic_fwd(&s, params, host, 90, 129, PLNERF_PREC_FP32, ws, need, host, 4, NULL, NULL) != PLNERF_EINVAL) return 6;
    if (plnerf_generic_fwd(&s, params, host, 90, 129, PLNERF_PREC_F16X3, ws, need - 1, host, 4, NULL, NULL) != PLNERF_EINVAL) return 7;
    if (plnerf_generic_fwd(&s, params, host, 90, 129, PLNERF_PREC_F16X3, ws + 4, need, host, 4, NULL, NULL) != PLNERF_EINVAL) return 8;
    if (plnerf_generic_fwd(&s, params, host, 90, 0, PLNERF_PREC_BF16X3, ws, need, host, 4, NULL, NULL) != PLNERF_OK) return 9;
    s.skips[0] = 9;
    if (plnerf_generic_fwd(&s, params, host, 90, 129, PLNERF_PREC_F16X3, ws, need, host, 4, NULL, NULL) != PLNERF_EINVAL) return 10;
    s.skips[0] = 4;
    s.D = 0;
    if (plnerf_generic_fwd(&s, params, host, 90, 129, PLNERF_PREC_F16X3, ws, need, host, 4, NULL, NULL) != PLNERF_EINVAL) return 11;
    if (plnerf_pack_h16(host, 7, 4, 8, PLNERF_PREC_F16X3, ws, NULL, PLNERF_RANGE_WEIGHT, NULL) != PLNERF_EINVAL) return 12;
    if (plnerf_pack_h16(host, 8, 4, 8, PLNERF_PREC_F16X3, ws, NULL, 0, NULL) != PLNERF_EINVAL) return 13;
    if (plnerf_pack_h16(host, 8, 0, 8, PLNERF_PREC_BF16, ws, NULL, PLNERF_RANGE_ACTIVATION, NULL) != PLNERF_OK) return 14;
    printf("generic fwd abi ok\n");
    return 0;
}
"""


def test_header_is_plain_c_and_the_checks_come_first(L, tmp_path_factory):
    exe = abi.compile_c(_C, tmp_path_factory.mktemp("generic_fwd_abi"), "generic_fwd_abi")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "generic fwd abi ok" in out.stdout


def test_the_switch_exists_and_is_off(L):
    from plnerf_amd import generic
    assert generic.CHAIN_INFERENCE is False
    assert generic.HONOUR_PRECISION is False and generic.HONOUR_PRECISION_BACKWARD is False
