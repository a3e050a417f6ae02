"""The experimental header include/experimental/plnerf_hip_mesh.h, without a GPU, as tests/test_anyview_abi.py holds its
header: the one row of the eleventh table _lib.MESH_HEADERS against the header's prototypes and the library's exports, the
signatures argument by argument, what lib() bound, that the header is plain C99, the size queries restated, every refusal that
comes before a launch (on fake pointers that are never followed), that the cases of the GPU tests build on a CPU and match
the prototypes -- and that the other ten tables and the ABI version are what they were."""
import ctypes
import os

import pytest

import abi_support as abi
import containment as C
import mesh_cases

HEADER = "experimental/plnerf_hip_mesh.h"
ENTRIES = {"plnerf_density_grid_workspace_bytes": 6, "plnerf_density_grid": 15, "plnerf_mc_workspace_bytes": 3,
           "plnerf_mc_count": 9, "plnerf_mc_emit": 12}
OK, EINVAL, ELAUNCH, ERANGE, ENOSYS = 0, -1, -2, -3, -4


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.MESH_HEADERS) == 1
    header, signatures, mirrors = L.MESH_HEADERS[0]
    assert header == HEADER and mirrors == {}
    return os.path.join(abi.INCLUDE, header), signatures


def _others(L):
    return (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES,
            L.GEMM16_TABLE_SIGNATURES, L.GEMM16_BWD_TABLE_SIGNATURES, L.GENERIC_FWD_TABLE_SIGNATURES,
            L.GENERIC_TRAIN_TABLE_SIGNATURES, L.ANYVIEW_TABLE_SIGNATURES, L.UNIQUE_TABLE_SIGNATURES)


# ----------------------------------------------------------------------------- the row against the header and the library
def test_names_agree(L, row):
    path, signatures = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == set(ENTRIES) == set(L.MESH_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert abi.structs(path) == {}      # (the slot is the ninth table's plnerf_anyview_net)
    assert HEADER not in [h for h, _, _ in L.HEADERS]      # (experimental: outside the registry)


def test_signatures_agree(L, row):
    path, signatures = row
    structs = {**abi.abi_structs(), **L.GENERIC_FWD_STRUCTS, **L.ANYVIEW_STRUCTS}
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == ENTRIES[name], (name, len(args), len(params))
        assert ret == ("size_t" if name.endswith("_bytes") else "int")
        if ret == "int":
            assert params[-1] == "plnerf_stream_t"
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            bare = abi.bare(c_type)
            if bare.endswith("*") or bare == "plnerf_stream_t":
                assert abi.ct_class(ct) == "ptr", (where, c_type, ct)
                if bare.rstrip("*").strip() in structs:
                    assert ct is ctypes.POINTER(structs[bare.rstrip("*").strip()]), (where, c_type, ct)
                else:
                    assert ct is ctypes.c_void_p, (where, c_type, ct)
            else:
                assert ct is abi.SCALARS[bare], (where, c_type, ct)
    code = open(path).read()
    for macro, value in (("STATS", L.GRID_STATS), ("MIN", L.GRID_MIN), ("MAX", L.GRID_MAX), ("SUM", L.GRID_SUM), ("SUMSQ", L.GRID_SUMSQ)):
        assert f"#define PLNERF_GRID_{macro} {value}\n" in code, macro


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    others = set().union(*[set(t) for t in _others(L)])
    assert not set(L.MESH_TABLE_SIGNATURES) & others
    assert len(others) == sum(len(t) for t in _others(L))
    assert set(L.ANYVIEW_TABLE_SIGNATURES) == {"plnerf_generic_fwd_f32_workspace_bytes", "plnerf_generic_fwd_f32",
                                               "plnerf_render_view_any_workspace_bytes", "plnerf_render_view_any"}
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    with pytest.raises(ValueError, match="one entry point, one header"):
        L._disjoint({"plnerf_mc_emit": None}, L.MESH_TABLE_SIGNATURES)


def test_the_header_is_plain_c99(L, tmp_path):
    """A C99 host that includes the header alone and takes every entry's address compiles with -Wall -Werror -pedantic and
    links against the library."""
    source = '#include "experimental/plnerf_hip_mesh.h"\n#include <stdio.h>\nint main(void) {\n    void* entries[] = {' + \
             ", ".join(f"(void*)(size_t)&{name}" for name in ENTRIES) + \
             '};\n    printf("%d %d\\n", (int)(sizeof entries / sizeof entries[0]), PLNERF_GRID_STATS);\n    return 0;\n}\n'
    source = source.replace("(void*)(size_t)&", "(void*)(size_t)")      # (a function designator converts by itself)
    exe = abi.compile_c(source, tmp_path, "mesh_header")
    import subprocess
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == [str(len(ENTRIES)), "4"], (out.returncode, out.stdout, out.stderr)


# ----------------------------------------------------------------------------- size queries
def _up(v):
    return -(-v // 256) * 256


def _fused(L, null=None):
    net = L.AnyViewNet()
    net.route = L.ANYVIEW_FUSED
    for k in range(L.N_PARAM_TENSORS):
        net.fused.params[k] = 4096 + 64 * k
    net.fused.packed = 4096
    if null == "packed":
        net.fused.packed = None
    elif null is not None:
        net.fused.params[null] = None
    return net


def _generic(L, keep, route, precision="f16x3", params=-1, **over):
    kw = dict(D=9, W=72, input_ch=63, view_ch=27, use_viewdirs=1, output_ch=0, n_view_layers=1, skips=(4,))
    kw.update(over)
    skips = kw.pop("skips")
    shape = L.GenericShape(n_skips=len(skips), **kw)
    for q, k in enumerate(skips):
        shape.skips[q] = k
    net = L.AnyViewNet()
    net.route = route
    ctypes.memmove(ctypes.byref(net.shape), ctypes.byref(shape), ctypes.sizeof(shape))
    count = 2 * (shape.D + shape.n_view_layers + 3)
    table = (ctypes.c_void_p * count)(*[4096] * count) if params == -1 else params
    keep.append(table)
    net.params = ctypes.cast(table, ctypes.c_void_p).value if table is not None else None
    net.precision = L.PRECISION[precision]
    return net, shape


def test_the_size_queries(L):
    lib = L.lib()
    grid, mc = lib.plnerf_density_grid_workspace_bytes, lib.plnerf_mc_workspace_bytes
    P = L.PRECISION["f16x3"]

    def partials(n, rows):
        return n // rows * -(-rows // 1024) + -(-(n % rows) // 1024)
    # a fused slot: positions, one direction, raw outputs, one stats partial (4 fp64) per 1,024 rows of a block
    for res, max_rows in ((21, 100), (21, 1000), (21, 10000), (2, 3), (64, 5000), (64, 1 << 21)):
        n = res ** 3
        rows = min(n, max_rows)
        want = _up(12 * rows) + _up(12) + _up(16 * rows) + _up(32 * partials(n, rows))
        assert grid(ctypes.byref(_fused(L)), P, 63, 27, res, max_rows) == want, (res, max_rows)
    # a generic slot adds the embedded rows and its route's own workspace
    keep = []
    for route, query in ((L.ANYVIEW_LAYERS32, lambda s, r: lib.plnerf_generic_fwd_f32_workspace_bytes(ctypes.byref(s), r)),
                         (L.ANYVIEW_CHAIN16, lambda s, r: lib.plnerf_generic_fwd_workspace_bytes(ctypes.byref(s), r, P))):
        net, shape = _generic(L, keep, route)
        rows = 100
        want = _up(12 * rows) + _up(12) + _up(16 * rows) + _up(32 * partials(729, rows)) + _up(4 * 90 * rows) + _up(query(shape, rows))
        assert grid(ctypes.byref(net), 17, 5, 1, 9, rows) == want, route      # (precision and widths of the call are ignored)
    # marching cubes: one word per point, two per 1,024-point block, two per 1,024 blocks
    for shape in ((2, 2, 2), (2, 3, 5), (9, 9, 9), (17, 17, 17), (512, 512, 512), (1024, 1024, 1024), (1025, 1023, 3)):
        n = shape[0] * shape[1] * shape[2]
        nb = -(-n // 1024)
        ns = -(-nb // 1024)
        assert mc(*shape) == _up(4 * n) + 2 * _up(4 * nb) + 2 * _up(4 * ns), shape
    assert mc(512, 512, 512) / 512 ** 3 < 4.008      # bytes per lattice point, as the header says
    for bad in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 2, 2), (-3, 2, 2), (1025, 1024, 1024), (1 << 16, 1 << 16, 2)):
        assert mc(*bad) == 0, bad


# ----------------------------------------------------------------------------- refusals, on fake pointers
def test_density_grid_refusals_come_before_any_launch(L):
    lib = L.lib()
    query, entry = lib.plnerf_density_grid_workspace_bytes, lib.plnerf_density_grid
    P = L.PRECISION["f16x3"]
    p = 4096
    keep = []

    def call(net=-1, precision=P, input_ch=63, input_ch_views=27, resolution=21, xs=p, ys=p, zs=p, max_rows=100, field=p, stats=p,
             ws=p, ws_bytes=None):
        net = _fused(L) if net == -1 else net
        ref = ctypes.byref(net) if net is not None else None
        need = query(ref, precision, input_ch, input_ch_views, resolution, max_rows)
        code = entry(ref, precision, input_ch, input_ch_views, resolution, xs, ys, zs, max_rows, 1, field, stats, ws,
                     (need or 1 << 40) if ws_bytes is None else ws_bytes, None)
        return need, code
    need = query(ctypes.byref(_fused(L)), P, 63, 27, 21, 100)
    assert need > 0 and need % 256 == 0
    bad_route = _fused(L)
    bad_route.route = 3
    refused_by_both = [
        (dict(net=None), EINVAL), (dict(resolution=1), EINVAL), (dict(resolution=0), EINVAL), (dict(resolution=-4), EINVAL),
        (dict(max_rows=0), EINVAL), (dict(max_rows=-1), EINVAL), (dict(net=bad_route), EINVAL),
        (dict(resolution=1025), ERANGE), (dict(resolution=1 << 30), ERANGE),
        (dict(input_ch=64), EINVAL), (dict(input_ch=69), EINVAL), (dict(input_ch_views=33), EINVAL), (dict(input_ch_views=4), EINVAL),
        (dict(precision=17), ENOSYS),
        (dict(resolution=1024, max_rows=1 << 30), ERANGE),      # a fused block of more rows than the forward takes
        (dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32, skips=(8,))[0]), EINVAL),
        (dict(net=_generic(L, keep, L.ANYVIEW_CHAIN16, skips=(8,))[0]), EINVAL),
        (dict(net=_generic(L, keep, L.ANYVIEW_CHAIN16, precision="fp32")[0]), EINVAL),
        (dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32, use_viewdirs=0, output_ch=5)[0]), EINVAL),
        (dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32, input_ch=64)[0]), EINVAL),
        (dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32, input_ch=105)[0]), EINVAL),      # 17 bands
        (dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32, W=65538)[0]), ERANGE),
        (dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32)[0], resolution=256, max_rows=1 << 23), ERANGE),      # plnerf_gemm_f32's rows
    ]
    for kw, code in refused_by_both:
        assert call(**kw) == (0, code), (kw, call(**kw))
    assert call(resolution=1024, max_rows=1 << 21)[0] > 0      # 2^30 points are served
    refused_by_the_entry = [
        dict(xs=None), dict(ys=None), dict(zs=None), dict(field=None), dict(ws=None), dict(ws=p + 4), dict(ws=p + 128),
        dict(ws_bytes=need - 1), dict(net=_fused(L, null="packed")), dict(net=_fused(L, null=0)), dict(net=_fused(L, null=23)),
        dict(net=_generic(L, keep, L.ANYVIEW_LAYERS32, params=None)[0]),
    ]
    for kw in refused_by_the_entry:
        got = call(**kw)
        assert got[0] > 0 and got[1] == EINVAL, (kw, got)
    off = _fused(L)
    off.fused.params[18] = 4096 + 4      # feature_linear.weight off 16 bytes
    assert call(net=off)[1] == EINVAL
    table = (ctypes.c_void_p * 26)(*[4096] * 26)
    table[25] = None
    assert call(net=_generic(L, keep, L.ANYVIEW_CHAIN16, params=table)[0])[1] == EINVAL
    # stats may be left out: every check passes and the launch itself fails on a machine without a device
    import torch
    if not torch.cuda.is_available():
        got = call(stats=None)
        assert got[0] > 0 and got[1] == ELAUNCH, got


def test_marching_cubes_refusals_come_before_any_launch(L):
    lib = L.lib()
    count, emit, query = lib.plnerf_mc_count, lib.plnerf_mc_emit, lib.plnerf_mc_workspace_bytes
    p = 4096
    need = query(9, 9, 9)

    def counted(field=p, shape=(9, 9, 9), iso=0.0, ws=p, ws_bytes=need, counts=p):
        return count(field, *shape, iso, ws, ws_bytes, counts, None)

    def emitted(field=p, shape=(9, 9, 9), iso=0.0, ws=p, ws_bytes=need, v=p, cap_v=10, t=p, cap_t=10):
        return emit(field, *shape, iso, ws, ws_bytes, v, cap_v, t, cap_t, None)
    for fn in (counted, emitted):
        for bad in (dict(field=None), dict(ws=None), dict(ws=p + 4), dict(ws=p + 128), dict(ws_bytes=need - 1), dict(shape=(1, 9, 9)),
                    dict(shape=(9, 0, 9)), dict(shape=(9, 9, -2)), dict(iso=float("nan"))):
            assert fn(**bad) == EINVAL, (fn.__name__, bad)
        assert fn(shape=(1025, 1024, 1024), ws_bytes=1 << 40) == ERANGE
    assert counted(counts=None) == EINVAL
    for bad in (dict(cap_v=-1), dict(cap_t=-1), dict(v=None), dict(t=None)):
        assert emitted(**bad) == EINVAL, bad
    assert emitted(cap_v=1 << 31) == ERANGE and emitted(cap_t=1 << 31) == ERANGE
    # the empty surface: no launch (a launch here, without a device, would be PLNERF_ELAUNCH)
    assert emitted(v=None, cap_v=0, t=None, cap_t=0) == OK


# ----------------------------------------------------------------------------- the GPU tests' cases build on a CPU
def test_the_gpu_cases_build_and_match_the_prototypes(L, row):
    protos = abi.prototypes(row[0])
    main = abi.prototypes(os.path.join(abi.INCLUDE, "plnerf_hip.h"))
    cases = [mesh_cases.grid_case(L, precision)[0] for precision in ("f16x3", "bf16x3", "fp32")]
    cases.append(mesh_cases.grid_case(L, "f16x3", resolution=2, max_rows=(3, 8))[0])
    fields = mesh_cases.mc_fields()
    assert {"2x3x5", "cell", "outside", "inside", "at_iso", "sphere"} <= set(fields)
    cases += [mesh_cases.mc_case(L, name, f, iso)[0] for name, (f, iso) in fields.items()]
    cases.append(mesh_cases.mc_case(L, "sphere", *fields["sphere"], short=True)[0])
    seen = set()
    for calls in cases:
        C.case_buffers(calls)      # (no two buffers of a case share a name)
        for call in calls:
            ret, params = (protos if call.entry in protos else main)[call.entry]
            C.check_against_prototype(call, params, getattr(L.lib(), call.entry).argtypes)
            seen.add(call.entry)
    assert {"plnerf_density_grid", "plnerf_mc_count", "plnerf_mc_emit"} <= seen
