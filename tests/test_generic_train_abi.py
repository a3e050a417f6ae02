"""The experimental header include/experimental/plnerf_hip_generic_train.h, without a GPU, as tests/test_generic_fwd_abi.py
holds its header: the one row of the eighth table _lib.GENERIC_TRAIN_HEADERS against the header's prototypes and the library's
exports, the signatures argument by argument, what lib() bound, every refusal that comes before a launch (through the binding
and from a C99 host), the size queries, the split rule against generic._splits -- and that the seven existing tables and the
ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi

HEADER = "experimental/plnerf_hip_generic_train.h"
ARGUMENTS = {"plnerf_generic_train_saved_bytes": 3, "plnerf_generic_train_workspace_bytes": 3,
             "plnerf_generic_train_wgrad_splits": 3, "plnerf_generic_train_fwd": 12, "plnerf_generic_train_bwd": 14}
ENTRIES = set(ARGUMENTS)
NO_STREAM = {"plnerf_generic_train_wgrad_splits"}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
OK, EINVAL, ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.GENERIC_TRAIN_HEADERS) == 1
    header, signatures, mirrors = L.GENERIC_TRAIN_HEADERS[0]
    assert header == HEADER and mirrors == {}      # (the struct is the seventh table's)
    return os.path.join(abi.INCLUDE, header), signatures


def _others(L):
    return (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES,
            L.GEMM16_TABLE_SIGNATURES, L.GEMM16_BWD_TABLE_SIGNATURES, L.GENERIC_FWD_TABLE_SIGNATURES)


def test_names_agree(L, row):
    path, signatures = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES == set(L.GENERIC_TRAIN_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert abi.structs(path) == {}
    assert '#include "plnerf_hip_generic.h"' in open(path).read()


def test_signatures_agree(L, row):
    """tests/test_generic_fwd_abi.py's rule per return and argument type: a scalar is that ctypes type, a pointer to the shape
    is a POINTER to its mirror, a host array of device pointers a POINTER(c_void_p), every other pointer and the stream
    c_void_p."""
    path, signatures = row
    mirrors = L.GENERIC_FWD_STRUCTS
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == ARGUMENTS[name], (name, len(args), len(params))
        assert ret == ("size_t" if name.endswith("_bytes") else "int")
        assert (params[-1] == "plnerf_stream_t") is (ret == "int" and name not in NO_STREAM), name
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            bare = abi.bare(c_type)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[bare], (where, c_type, ct)
            elif bare.rstrip("*").strip() in mirrors:
                assert ct is ctypes.POINTER(mirrors[bare.rstrip("*").strip()]), (where, c_type, ct)
            elif bare.count("*") == 2:      # (params, grads: host memory the library follows)
                assert ct is ctypes.POINTER(ctypes.c_void_p), (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The eighth table shares no name with the other seven and adds nothing to them."""
    others = set().union(*[set(t) for t in _others(L)])
    assert not set(L.GENERIC_TRAIN_TABLE_SIGNATURES) & others
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert tuple(header for header, _, _ in L.EXPERIMENTAL_HEADERS) == ("experimental/plnerf_hip_depthview.h",)
    assert tuple(header for header, _, _ in L.CAMCODE_HEADERS) == ("experimental/plnerf_hip_camcode.h",)
    assert tuple(header for header, _, _ in L.DPSTEP_HEADERS) == ("experimental/plnerf_hip_dpstep.h",)
    assert tuple(header for header, _, _ in L.GEMM16_HEADERS) == ("experimental/plnerf_hip_gemm16.h",)
    assert set(L.GEMM16_TABLE_SIGNATURES) == {"plnerf_gemm_h16"}
    assert tuple(header for header, _, _ in L.GEMM16_BWD_HEADERS) == ("experimental/plnerf_hip_gemm16_bwd.h",)
    assert set(L.GEMM16_BWD_TABLE_SIGNATURES) == {"plnerf_gemm_h16_dgrad", "plnerf_gemm_h16_wgrad"}
    assert tuple(header for header, _, _ in L.GENERIC_FWD_HEADERS) == ("experimental/plnerf_hip_generic.h",)
    assert set(L.GENERIC_FWD_TABLE_SIGNATURES) == {"plnerf_pack_h16", "plnerf_generic_fwd_workspace_bytes", "plnerf_generic_fwd"}
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


def _table(count, null_at=None):
    table = (ctypes.c_void_p * count)(*[4096] * count)
    if null_at is not None:
        table[null_at] = None
    return table


def _splits(N, K1, M):
    from plnerf_amd import generic
    return generic._splits(N, K1, M)


def test_the_split_rule_is_the_layered_route_s(L):
    sizes = (1, 4, 33, 101, 257, 513, 1025)
    rule = L.lib().plnerf_generic_train_wgrad_splits
    seen = set()
    for N in sizes:
        for K1 in sizes:
            for M in (0, 511, 512, 1600, 262144):
                assert rule(N, K1, M) == _splits(N, K1, M), (N, K1, M)
                seen.add(rule(N, K1, M))
    assert {1, 3, 512} <= seen and max(seen) == 512      # (262,144 rows over one tile; 1,600 rows: three splits)
    assert rule(100, 164, 1600) == 3 and rule(320, 384, 1600) == 3


def test_the_size_queries(L):
    """Restated from the header.  saved: the packed weights, then per layer that runs its gate plane (ReLU layers) and its
    output (packed, or the fp32 concatenation rows).  workspace: the words, two [n, W] fp32 buffers, the largest partials."""
    saved, work = L.lib().plnerf_generic_train_saved_bytes, L.lib().plnerf_generic_train_workspace_bytes

    def up(v, to=256):
        return -(-v // to) * to

    def expect(D, W, in_ch, view_ch, viewdirs, out_ch, n_views, skips, n, planes):
        dims = [(W, in_ch if i == 0 else (in_ch + W if i - 1 in skips else W)) for i in range(D)]
        relu = [True] * D
        cat = [up(in_ch + W, 4) if i in skips else 0 for i in range(D)]
        if viewdirs:
            dims += [(W // 2, W + view_ch if v == 0 else W // 2) for v in range(n_views)] + [(W, W), (1, W), (3, W // 2)]
            relu += [True] * n_views + [False] * 3
            cat += [0] * n_views + [up(W + view_ch, 4), 0, 0]
        else:
            dims += [(out_ch, W)]
            relu += [False]
            cat += [0]
        total = sum(up(planes * N * L.pack_ld(K) * 2) for N, K in dims)
        for (N, K), gated, ld in zip(dims, relu, cat):
            if gated:
                total += up(n * -(-N // 32) * 4)
            if ld:
                total += up(n * ld * 4)
            elif gated:
                total += up(planes * n * L.pack_ld(N) * 2)
        layers = D + n_views + (3 if viewdirs else 1)
        partials = max(_splits(N, K + 1, n) * N * (K + 1) * 4 if _splits(N, K + 1, n) > 1 else 0 for N, K in dims)
        return total, up(layers * 4) + 2 * up(n * up(W, 4) * 4) + up(partials)
    for name, planes in (("f16x3", 2), ("bf16x3", 2), ("f16", 1), ("bf16", 1)):
        code = L.PRECISION[name]
        for kw, args in ((dict(), (9, 100, 63, 27, True, 0, 1, (4,))), (dict(skips=(3, 4, 6)), (9, 100, 63, 27, True, 0, 1, (3, 4, 6))),
                         (dict(use_viewdirs=0, output_ch=5, view_ch=0, skips=()), (9, 100, 63, 0, False, 5, 1, ()))):
            for n in (129, 1600):
                want = expect(*args, n, planes)
                s = _shape(L, **kw)
                assert (saved(ctypes.byref(s), n, code), work(ctypes.byref(s), n, code)) == want, (name, kw, n)
        assert saved(ctypes.byref(_shape(L)), 0, code) > 0 and work(ctypes.byref(_shape(L)), 0, code) > 0
    # per hidden element: 4 bytes (split) or 2 (plain) + a bit, against 4 bytes of fp32 -- at 8 x 512, 196,608 rows
    big = _shape(L, D=8, W=512, n_view_layers=1)
    n = 196608
    hidden = n * (7 * 512 + 256)      # (the layer in front of the skip keeps fp32 rows: counted apart)
    cats = n * ((63 + 512 + 3) // 4 * 4 + (512 + 27 + 3) // 4 * 4) * 4 + n * (512 // 32) * 4
    for name, per in (("f16x3", 4), ("f16", 2)):
        got = saved(ctypes.byref(big), n, L.PRECISION[name]) - saved(ctypes.byref(big), 0, L.PRECISION[name])      # (less the weights)
        assert abs(got - cats - hidden * (per + 1 / 8)) < 64 * 256, (name, got)
    f16x3 = L.PRECISION["f16x3"]
    for query in (saved, work):
        assert query(ctypes.byref(_shape(L)), 129, L.PRECISION["fp32"]) == 0
        assert query(ctypes.byref(_shape(L)), -1, f16x3) == 0
        assert query(ctypes.byref(_shape(L, D=0)), 129, f16x3) == 0
        assert query(ctypes.byref(_shape(L, skips=(8,))), 129, f16x3) == 0
        assert query(ctypes.byref(_shape(L, W=65538)), 129, f16x3) == 0
        assert query(None, 129, f16x3) == 0


def test_refusals_come_before_any_launch(L):
    """Through the binding, without a device, on fake pointers that are never followed (a launch here would be
    PLNERF_ELAUNCH): every argument error of the forward and the backward -- and the empty forward, which is PLNERF_OK."""
    fwd, bwd = L.lib().plnerf_generic_train_fwd, L.lib().plnerf_generic_train_bwd
    q_saved, q_work = L.lib().plnerf_generic_train_saved_bytes, L.lib().plnerf_generic_train_workspace_bytes
    p = ctypes.c_void_p(4096)
    f16x3 = L.PRECISION["f16x3"]
    n_layers = 9 + 1 + 3

    def forward(shape=None, params=-1, rows=p, ld_rows=90, n=129, precision=f16x3, sv=4096, sv_bytes=None, out=p, ld_out=4):
        shape = _shape(L) if shape is None else shape
        params = _table(2 * n_layers) if params == -1 else params
        ref = ctypes.byref(shape) if shape is not False else None
        if sv_bytes is None:
            sv_bytes = q_saved(ref, max(n, 0), precision) or 1 << 40
        return fwd(ref, params, rows, ld_rows, n, precision, ctypes.c_void_p(sv) if sv else None, sv_bytes, out, ld_out, None, None)

    def backward(shape=None, rows=p, ld_rows=90, n=129, precision=f16x3, sv=4096, sv_bytes=None, g=p, ld_g=4, grads=-1, ws=8192,
                 ws_bytes=None):
        shape = _shape(L) if shape is None else shape
        grads = _table(n_layers) if grads == -1 else grads
        ref = ctypes.byref(shape) if shape is not False else None
        if sv_bytes is None:
            sv_bytes = q_saved(ref, max(n, 0), precision) or 1 << 40
        if ws_bytes is None:
            ws_bytes = q_work(ref, max(n, 0), precision) or 1 << 40
        return bwd(ref, rows, ld_rows, n, precision, ctypes.c_void_p(sv) if sv else None, sv_bytes, g, ld_g, grads,
                   ctypes.c_void_p(ws) if ws else None, ws_bytes, None, None)
    need_s, need_w = q_saved(ctypes.byref(_shape(L)), 129, f16x3), q_work(ctypes.byref(_shape(L)), 129, f16x3)
    assert need_s > 0 and need_w > 0
    shapes = (dict(shape=_shape(L, D=0)), dict(shape=_shape(L, D=-1)), dict(shape=_shape(L, W=0)), dict(shape=_shape(L, W=1)),
              dict(shape=_shape(L, input_ch=0)), dict(shape=_shape(L, view_ch=-1)), dict(shape=_shape(L, n_view_layers=0)),
              dict(shape=_shape(L, use_viewdirs=0, output_ch=0)),
              dict(shape=_shape(L, skips=(9,))), dict(shape=_shape(L, skips=(4, 10))), dict(shape=_shape(L, skips=(8,))),
              dict(shape=_shape(L, skips=(-1,))), dict(shape=_shape(L, skips=(), n_skips=17)), dict(shape=_shape(L, skips=(), n_skips=-1)),
              dict(shape=False), dict(precision=L.PRECISION["fp32"]), dict(precision=5), dict(precision=-1), dict(n=-1),
              dict(ld_rows=89), dict(rows=None), dict(sv_bytes=need_s - 1), dict(sv=4096 + 4), dict(sv=4096 + 8), dict(sv=None))
    for bad in shapes + (dict(params=None), dict(params=_table(2 * n_layers, null_at=0)),
                         dict(params=_table(2 * n_layers, null_at=2 * n_layers - 1)), dict(params=_table(2 * n_layers, null_at=19)),
                         dict(out=None), dict(ld_out=3)):
        assert forward(**bad) == EINVAL, bad
    for bad in shapes + (dict(grads=None), dict(grads=_table(n_layers, null_at=0)), dict(grads=_table(n_layers, null_at=9)),
                         dict(grads=_table(n_layers, null_at=n_layers - 1)), dict(g=None), dict(ld_g=3),
                         dict(ws_bytes=need_w - 1), dict(ws=8192 + 4), dict(ws=8192 + 8), dict(ws=None)):
        assert backward(**bad) == EINVAL, bad
    assert backward(n=0, grads=None) == EINVAL and backward(n=0, grads=_table(n_layers, null_at=3)) == EINVAL
    assert forward(sv_bytes=need_s, n=0) == OK and forward(n=0, rows=None, out=None, sv=None, sv_bytes=0) == OK
    # without use_viewdirs the view layers' slots are not read
    plain = _shape(L, use_viewdirs=0, output_ch=5)
    assert forward(shape=plain, params=_table(2 * (9 + 1 + 1), null_at=18), n=0, ld_out=5) == OK
    assert forward(shape=plain, params=_table(2 * (9 + 1 + 1), null_at=20), n=0, ld_out=5) == EINVAL
    assert forward(shape=plain, n=129, ld_out=4) == EINVAL and backward(shape=plain, n=129, ld_g=4) == EINVAL
    assert backward(shape=plain, grads=_table(9 + 1 + 1, null_at=10), ld_g=5) == EINVAL
    # a dimension beyond the compiled limit, more than 2^31 - 1 tiles: refused, not wrapped
    assert forward(shape=_shape(L, W=65538), n=0) == ERANGE and backward(shape=_shape(L, W=65538), n=0) == ERANGE
    assert forward(shape=_shape(L, W=65536, skips=()), n=2 ** 31 - 1) == ERANGE
    assert backward(shape=_shape(L, W=65536, skips=()), n=2 ** 31 - 1) == ERANGE
    for name in ("bf16x3", "bf16", "f16x3", "f16"):      # (every 16-bit mode is accepted as far as the checks go)
        assert forward(precision=L.PRECISION[name], n=0) == OK


_C = r"""
#include <stdio.h>
#include <string.h>
#include "experimental/plnerf_hip_generic_train.h"

/* never dereferenced by the device: every call below is refused by the argument checks, or is empty */
static float host[64];

int main(void) {
    plnerf_generic_shape s;
    const float* table[26];
    float* blocks[13];
    const float* const* params = (const float* const*)table;
    float* const* grads = (float* const*)blocks;
    size_t saved, work;
    int i;
    char* sv = (char*)4096;
    char* ws = (char*)8192;
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    memset(&s, 0, sizeof s);
    s.D = 9; s.W = 100; s.input_ch = 63; s.view_ch = 27; s.use_viewdirs = 1; s.n_view_layers = 1; s.n_skips = 1; s.skips[0] = 4;
    for (i = 0; i < 26; ++i) table[i] = host;
    for (i = 0; i < 13; ++i) blocks[i] = host;
    saved = plnerf_generic_train_saved_bytes(&s, 129, PLNERF_PREC_F16X3);
    work = plnerf_generic_train_workspace_bytes(&s, 129, PLNERF_PREC_F16X3);
    if (saved == 0 || work == 0 || plnerf_generic_train_saved_bytes(&s, 129, PLNERF_PREC_FP32) != 0) return 3;
    if (plnerf_generic_train_saved_bytes(&s, 129, PLNERF_PREC_F16) >= saved) return 4;
    if (plnerf_generic_train_wgrad_splits(100, 164, 1600) != 3 || plnerf_generic_train_wgrad_splits(1025, 1025, 262144) != 1) return 5;
    if (plnerf_generic_train_fwd(&s, params, host, 90, 129, PLNERF_PREC_FP32, sv, saved, host, 4, NULL, NULL) != PLNERF_EINVAL) return 6;
    if (plnerf_generic_train_fwd(&s, params, host, 90, 129, PLNERF_PREC_F16X3, sv, saved - 1, host, 4, NULL, NULL) != PLNERF_EINVAL) return 7;
    if (plnerf_generic_train_fwd(&s, params, host, 90, 129, PLNERF_PREC_F16X3, sv + 4, saved, host, 4, NULL, NULL) != PLNERF_EINVAL) return 8;
    if (plnerf_generic_train_fwd(&s, params, host, 90, 0, PLNERF_PREC_BF16X3, sv, saved, host, 4, NULL, NULL) != PLNERF_OK) return 9;
    if (plnerf_generic_train_bwd(&s, host, 90, 129, PLNERF_PREC_F16X3, sv, saved, host, 4, grads, ws, work - 1, NULL, NULL) != PLNERF_EINVAL) return 10;
    if (plnerf_generic_train_bwd(&s, host, 90, 129, PLNERF_PREC_F16X3, sv, saved, NULL, 4, grads, ws, work, NULL, NULL) != PLNERF_EINVAL) return 11;
    if (plnerf_generic_train_bwd(&s, host, 90, 129, PLNERF_PREC_F16X3, sv, saved, host, 3, grads, ws, work, NULL, NULL) != PLNERF_EINVAL) return 12;
    blocks[4] = NULL;
    if (plnerf_generic_train_bwd(&s, host, 90, 129, PLNERF_PREC_F16X3, sv, saved, host, 4, grads, ws, work, NULL, NULL) != PLNERF_EINVAL) return 13;
    s.D = 0;
    if (plnerf_generic_train_bwd(&s, host, 90, 129, PLNERF_PREC_F16X3, sv, saved, host, 4, grads, ws, work, NULL, NULL) != PLNERF_EINVAL) return 14;
    printf("generic train abi ok\n");
    return 0;
}
"""


def test_header_is_plain_c_and_the_checks_come_first(L, tmp_path_factory):
    exe = abi.compile_c(_C, tmp_path_factory.mktemp("generic_train_abi"), "generic_train_abi")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "generic train abi ok" in out.stdout


def test_the_switch_exists_and_is_off(L):
    from plnerf_amd import generic
    assert generic.CHAIN_TRAINING is False
    assert generic.CHAIN_INFERENCE is False
    assert generic.HONOUR_PRECISION is False and generic.HONOUR_PRECISION_BACKWARD is False
