"""The experimental header include/experimental/plnerf_hip_anyview.h, without a GPU, as tests/test_generic_fwd_abi.py holds
its header: the one row of the ninth table _lib.ANYVIEW_HEADERS against the header's prototypes, its structs and the
library's exports, the signatures argument by argument, the struct mirrors field by field, what lib() bound, every refusal
that comes before a launch (size queries answering 0, the entries PLNERF_EINVAL / PLNERF_ERANGE, on fake pointers that are never
followed), that the torch-free host compiles -- and that the other eight tables and the ABI version are what they were."""
import ctypes
import os

import pytest

import abi_support as abi
import c_hosts

HEADER = "experimental/plnerf_hip_anyview.h"
STRUCTS = ("plnerf_anyview_net", "plnerf_anyview_io")
ENTRIES = {"plnerf_generic_fwd_f32_workspace_bytes": 2, "plnerf_generic_fwd_f32": 10,
           "plnerf_render_view_any_workspace_bytes": 2, "plnerf_render_view_any": 6}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
OK, EINVAL, ERANGE = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.ANYVIEW_HEADERS) == 1
    header, signatures, mirrors = L.ANYVIEW_HEADERS[0]
    assert header == HEADER and set(mirrors) == set(STRUCTS)
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def _others(L):
    return (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES, L.DPSTEP_TABLE_SIGNATURES,
            L.GEMM16_TABLE_SIGNATURES, L.GEMM16_BWD_TABLE_SIGNATURES, L.GENERIC_FWD_TABLE_SIGNATURES,
            L.GENERIC_TRAIN_TABLE_SIGNATURES)


def _structs(L):
    """Every struct a prototype or a field of this header may name: the registered ABI's, plnerf_generic_shape, its own."""
    return {**abi.abi_structs(), **L.GENERIC_FWD_STRUCTS, **L.ANYVIEW_STRUCTS}


# ----------------------------------------------------------------------------- the row against the header and the library
def test_names_agree(L, row):
    path, signatures, mirrors = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == set(ENTRIES) == set(L.ANYVIEW_TABLE_SIGNATURES)
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert set(abi.structs(path)) == set(mirrors)
    assert HEADER not in [h for h, _, _ in L.HEADERS]      # (experimental: outside the registry)


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type: a scalar is that ctypes type, a pointer to a struct is
    a POINTER to its mirror, the host array of parameter pointers a POINTER(c_void_p), every other pointer and the stream
    c_void_p."""
    path, signatures, _ = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params) == ENTRIES[name], (name, len(args), len(params))
        assert ret == ("size_t" if name.endswith("_bytes") else "int")
        if ret == "int":
            assert params[-1] == "plnerf_stream_t"
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            bare = abi.bare(c_type)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[bare], (where, c_type, ct)
            elif bare.rstrip("*").strip() in _structs(L):
                assert ct is ctypes.POINTER(_structs(L)[bare.rstrip("*").strip()]), (where, c_type, ct)
            elif bare.count("*") == 2:      # (const float* const* params: host memory the library follows)
                assert ct is ctypes.POINTER(ctypes.c_void_p), (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)


def test_struct_mirrors_agree(L, row):
    path, _, mirrors = row
    for name, fields in abi.structs(path).items():
        mirror = mirrors[name]._fields_
        assert [f[0] for f in mirror] == [f[1] for f in fields], name
        for (fname, ftype), (c_type, _, length) in zip(mirror, fields):
            t = abi.bare(c_type)
            assert length is None, (name, fname)
            want = _structs(L)[t] if t in _structs(L) else (ctypes.c_void_p if abi.c_class(t) == "ptr" else abi.SCALARS[t])
            assert ftype is want, (name, fname, ftype, want)
    code = open(path).read()
    for macro, value in (("FUSED", L.ANYVIEW_FUSED), ("CHAIN16", L.ANYVIEW_CHAIN16), ("LAYERS32", L.ANYVIEW_LAYERS32)):
        assert f"#define PLNERF_ANYVIEW_{macro} {value} " in code, macro
    # the frame planes are plnerf_view_io's, under its names and in its order
    names = [f for f, _ in L.AnyViewIo._fields_]
    assert names[names.index("t_vals"):] == [f for f, _ in L.ViewIo._fields_][2:]


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The ninth table shares no name with the other eight and adds nothing to them; the registered headers are the ten."""
    others = set().union(*[set(t) for t in _others(L)])
    assert not set(L.ANYVIEW_TABLE_SIGNATURES) & others
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert tuple(h for h, _, _ in L.GENERIC_FWD_HEADERS) == ("experimental/plnerf_hip_generic.h",)
    assert set(L.GENERIC_FWD_TABLE_SIGNATURES) == {"plnerf_pack_h16", "plnerf_generic_fwd_workspace_bytes", "plnerf_generic_fwd"}
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in _others(L):
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)


# ----------------------------------------------------------------------------- plnerf_generic_fwd_f32: refusals and the size query
def _shape(L, **over):
    kw = dict(D=9, W=72, input_ch=63, view_ch=27, use_viewdirs=1, output_ch=0, n_view_layers=1, skips=(4,))
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


def _splits(M, N, K):      # generic._splits
    tiles = -(-M // 64) * -(-N // 64)
    return max(1, min(1024 // tiles, K // 512)) if tiles < 256 else 1


def test_the_f32_size_query(L):
    """Restated from the header: two fp32 [n, W] buffers, the concatenation rows (one buffer; two when two skips are adjacent),
    the widest layer's partial products, every piece rounded up to 256 bytes."""
    from plnerf_amd import generic
    query = L.lib().plnerf_generic_fwd_f32_workspace_bytes

    def up(v):
        return -(-v // 256) * 256

    def expect(D, W, in_ch, view_ch, viewdirs, out_ch, n_views, skips, n):
        dims = [(W, in_ch if i == 0 else (in_ch + W if i - 1 in skips else W)) for i in range(D)]
        if viewdirs:
            dims += [(W // 2, W + view_ch if v == 0 else W // 2) for v in range(n_views)] + [(W, W), (1, W), (3, W // 2)]
        else:
            dims += [(out_ch, W)]
        ld = max(in_ch + W if skips else 0, W + view_ch if viewdirs else 0)
        buffers = (1 if ld else 0) + (1 if any(k + 1 in skips for k in skips) else 0)
        partials = max((_splits(n, N, K) * n * N * 4 if _splits(n, N, K) > 1 else 0) for N, K in dims)
        return 2 * up(n * -(-W // 4) * 16) + buffers * up(n * -(-ld // 4) * 16) + up(partials)
    assert query(ctypes.byref(_shape(L)), 129) == expect(9, 72, 63, 27, True, 0, 1, (4,), 129)
    assert query(ctypes.byref(_shape(L, D=4, W=40, skips=(0, 2))), 777) == expect(4, 40, 63, 27, True, 0, 1, (0, 2), 777)
    assert query(ctypes.byref(_shape(L, skips=(3, 4, 6))), 200) == expect(9, 72, 63, 27, True, 0, 1, (3, 4, 6), 200)
    plain = _shape(L, use_viewdirs=0, output_ch=5, view_ch=0, skips=())
    assert query(ctypes.byref(plain), 300) == expect(9, 72, 63, 0, False, 5, 1, (), 300)
    wide = _shape(L, D=2, W=1024, skips=())      # 70 rows: the second layer's k range is dealt out over two workgroups
    assert _splits(70, 1024, 1024) == 2 == generic._splits(70, 1024, 1024)
    assert query(ctypes.byref(wide), 70) == expect(2, 1024, 63, 27, True, 0, 1, (), 70) > 2 * 70 * 1024 * 4 * 2
    assert L.lib().plnerf_generic_fwd_f32(ctypes.byref(_shape(L)), _param_table(26), None, 90, 0, None, 0, None, 4, None) == OK
    for refused in ((_shape(L), -1), (_shape(L, D=0), 129), (_shape(L, skips=(8,)), 129), (None, 129), (_shape(L), 4194241),
                    (_shape(L, W=65537), 10)):
        assert query(ctypes.byref(refused[0]) if refused[0] is not None else None, refused[1]) == 0, refused[1]
    assert query(ctypes.byref(_shape(L)), 4194240) > 0
    # the restated k_splits rule is generic._splits over the shapes where it matters
    for M, N, K in ((1, 1, 1), (70, 1024, 1024), (64, 64, 5000), (1000, 1024, 2048), (4097, 256, 4096), (63, 3, 512), (200, 40, 103)):
        assert _splits(M, N, K) == generic._splits(M, N, K)


def test_generic_fwd_f32_refusals_come_before_any_launch(L):
    """Through the binding, without a device (a launch here would be PLNERF_ELAUNCH): plnerf_generic_fwd's refusals but the
    precision's, and n beyond plnerf_gemm_f32's rows."""
    fwd, query = L.lib().plnerf_generic_fwd_f32, L.lib().plnerf_generic_fwd_f32_workspace_bytes
    p = ctypes.c_void_p(4096)
    n_params = 2 * (9 + 1 + 3)

    def call(shape=None, params=-1, rows=p, ld_rows=90, n=129, ws=4096, ws_bytes=None, out=p, ld_out=4):
        shape = _shape(L) if shape is None else shape
        params = _param_table(n_params) if params == -1 else params
        ref = ctypes.byref(shape) if shape is not False else None
        if ws_bytes is None:
            ws_bytes = query(ref, max(n, 0)) or 1 << 40
        return fwd(ref, params, rows, ld_rows, n, ctypes.c_void_p(ws) if ws else None, ws_bytes, out, ld_out, None)
    need = query(ctypes.byref(_shape(L)), 129)
    assert need > 0
    for bad in (dict(ws_bytes=need - 1), dict(ws=4096 + 4), dict(ws=4096 + 8), dict(ws=None),
                dict(shape=_shape(L, D=0)), dict(shape=_shape(L, W=0)), dict(shape=_shape(L, W=1)), dict(shape=_shape(L, input_ch=0)),
                dict(shape=_shape(L, view_ch=-1)), dict(shape=_shape(L, n_view_layers=0)), dict(shape=_shape(L, use_viewdirs=0, output_ch=0)),
                dict(shape=_shape(L, skips=(8,))), dict(shape=_shape(L, skips=(9,))), dict(shape=_shape(L, skips=(-1,))),
                dict(shape=_shape(L, skips=(), n_skips=17)), dict(shape=False), dict(params=None),
                dict(params=_param_table(n_params, null_at=0)), dict(params=_param_table(n_params, null_at=n_params - 1)),
                dict(rows=None), dict(out=None), dict(n=-1), dict(ld_rows=89), dict(ld_out=3)):
        assert call(**bad) == EINVAL, bad
    assert call(n=0) == OK and call(n=0, rows=None, out=None, ws=None, ws_bytes=0) == OK
    assert call(shape=_shape(L, W=65538), n=0) == ERANGE
    assert call(n=4194241) == ERANGE
    # plnerf_generic_fwd itself keeps refusing fp32
    assert L.lib().plnerf_generic_fwd(ctypes.byref(_shape(L)), _param_table(n_params), p, 90, 129, L.PRECISION["fp32"], p, 1 << 40, p, 4,
                                      None, None) == EINVAL
    assert L.lib().plnerf_generic_fwd_workspace_bytes(ctypes.byref(_shape(L)), 129, L.PRECISION["fp32"]) == 0


# ----------------------------------------------------------------------------- plnerf_render_view_any: refusals and the size query
def _config(L, **over):
    cfg = L.StepConfig(max_rays=16, n_samples=8, n_importance=8, mode=L.MODE["linear"], color_mode=L.COLOR["midpoint"], perturb=1,
                       white_bkgd=1, zero_tol=1e-4, epsilon=1e-3, H=5, W=9, fx=11.3, fy=9.7, cx=4.1, cy=2.6, near=2.0, far=6.0,
                       precision=L.PRECISION["f16x3"], fwd_kernel=0, input_ch=63, input_ch_views=27, seed=7)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _slot(L, slot, route, keep, shape=None, precision="f16x3", params=-1):
    slot.route = route
    if route == L.ANYVIEW_FUSED:
        for k in range(L.N_PARAM_TENSORS):
            slot.fused.params[k] = 4096 + 64 * k
        slot.fused.packed = 4096
        return
    shape = _shape(L) if shape is None else shape
    ctypes.memmove(ctypes.byref(slot.shape), ctypes.byref(shape), ctypes.sizeof(shape))
    table = _param_table(2 * (shape.D + shape.n_view_layers + 3)) if params == -1 else params
    keep.append(table)
    slot.params = ctypes.cast(table, ctypes.c_void_p).value if table is not None else None
    slot.precision = L.PRECISION[precision]


def _io(L, keep, coarse=None, fine=None, max_net_rows=100):
    """A fused coarse slot and a LAYERS32 fine slot unless told otherwise (dicts of _slot's keywords); keep: what the slots point at."""
    io = L.AnyViewIo(max_net_rows=max_net_rows, t_vals=4096, u_vals=4096, rgb=4096)
    _slot(L, io.coarse, keep=keep, **(coarse or dict(route=L.ANYVIEW_FUSED)))
    _slot(L, io.fine, keep=keep, **(fine or dict(route=L.ANYVIEW_LAYERS32)))
    return io


def test_render_view_any_refusals_and_the_size_query(L):
    """Every refusal the header lists, on fake pointers: the size query answers 0 where the configuration or a slot is refused,
    the entry the code; what the query cannot see (the pointers, the workspace, the pixel range) the entry refuses alone."""
    lib = L.lib()
    query, entry = lib.plnerf_render_view_any_workspace_bytes, lib.plnerf_render_view_any
    keep = []

    def call(cfg=None, io=None, args=None, ws=4096, ws_bytes=None):
        cfg = _config(L) if cfg is None else cfg
        io = _io(L, keep) if io is None else io
        args = L.ViewArgs(n_pix=45, pack_weights=1) if args is None else args
        need = query(ctypes.byref(cfg), ctypes.byref(io))
        code = entry(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(ws) if ws else None,
                     (need or 1 << 40) if ws_bytes is None else ws_bytes, None)
        return need, code

    def slot(route, **kw):
        return dict(route=route, **kw)
    FUSED, CHAIN16, LAYERS32 = L.ANYVIEW_FUSED, L.ANYVIEW_CHAIN16, L.ANYVIEW_LAYERS32
    need = query(ctypes.byref(_config(L)), ctypes.byref(_io(L, keep)))
    fused_need = lib.plnerf_render_view_workspace_bytes(ctypes.byref(_config(L)))
    assert need > fused_need > 0 and need % L.STEP_WORKSPACE_ALIGN == 0
    # two fused slots need exactly plnerf_render_view's bytes; a generic slot adds the embedded rows and its network workspace
    both_fused = _io(L, keep, fine=slot(FUSED))
    assert query(ctypes.byref(_config(L)), ctypes.byref(both_fused)) == fused_need
    rows = min(16 * 16, 100)
    generic_bytes = lib.plnerf_generic_fwd_f32_workspace_bytes(ctypes.byref(_shape(L)), rows)
    assert need == fused_need + -(-rows * 90 * 4 // 256) * 256 + -(-generic_bytes // 256) * 256
    chain = _io(L, keep, fine=slot(CHAIN16))
    chain_bytes = lib.plnerf_generic_fwd_workspace_bytes(ctypes.byref(_shape(L)), rows, L.PRECISION["f16x3"])
    assert query(ctypes.byref(_config(L)), ctypes.byref(chain)) == fused_need + -(-rows * 90 * 4 // 256) * 256 + -(-chain_bytes // 256) * 256
    # max_net_rows bounds it: beyond a block's rows it changes nothing
    sizes = [query(ctypes.byref(_config(L)), ctypes.byref(_io(L, keep, max_net_rows=m))) for m in (1, 100, 256, 1 << 21)]
    assert sizes[0] < sizes[1] < sizes[2] == sizes[3]
    # no fused slot: the configuration's precision and widths are not looked at (multires 12 | 6: 75 | 39 columns)
    wide = dict(shape=_shape(L, input_ch=75, view_ch=39))
    unfused = _io(L, keep, coarse=slot(LAYERS32, **wide), fine=slot(CHAIN16, precision="bf16", **wide))
    assert call(cfg=_config(L, precision=17, input_ch=5, input_ch_views=1), io=unfused, ws_bytes=0)[0] > 0

    refused_by_both = [
        (dict(io=_io(L, keep, fine=slot(3))), EINVAL),                                               # a bad route
        (dict(io=_io(L, keep, coarse=slot(-1))), EINVAL),
        (dict(io=_io(L, keep, fine=slot(LAYERS32, shape=_shape(L, input_ch=57)))), EINVAL),           # mismatched encoding widths
        (dict(io=_io(L, keep, fine=slot(CHAIN16, shape=_shape(L, view_ch=21)))), EINVAL),
        (dict(io=_io(L, keep, coarse=slot(LAYERS32), fine=slot(LAYERS32, shape=_shape(L, input_ch=57)))), EINVAL),
        (dict(cfg=_config(L, input_ch=57)), EINVAL),                                                 # a fused slot against other config widths
        (dict(cfg=_config(L, input_ch_views=21)), EINVAL),
        (dict(io=_io(L, keep, max_net_rows=0)), EINVAL),                                             # max_net_rows < 1
        (dict(io=_io(L, keep, max_net_rows=-5)), EINVAL),
        (dict(io=_io(L, keep, fine=slot(LAYERS32, shape=_shape(L, skips=(8,))))), EINVAL),           # a skip at D - 1
        (dict(io=_io(L, keep, fine=slot(CHAIN16, shape=_shape(L, skips=(8,))))), EINVAL),
        (dict(io=_io(L, keep, fine=slot(CHAIN16, precision="fp32"))), EINVAL),                       # CHAIN16 in fp32
        (dict(io=_io(L, keep, fine=slot(LAYERS32, shape=_shape(L, use_viewdirs=0, output_ch=5)))), EINVAL),
        (dict(io=_io(L, keep, fine=slot(LAYERS32, shape=_shape(L, input_ch=64)))), EINVAL),          # not 3 + 6 L
        (dict(io=_io(L, keep, coarse=slot(LAYERS32, shape=_shape(L, input_ch=105)), fine=slot(LAYERS32, shape=_shape(L, input_ch=105)))),
         EINVAL),                                                                                    # 17 bands
        (dict(io=_io(L, keep, fine=slot(LAYERS32, shape=_shape(L, W=65538)))), ERANGE),
        (dict(cfg=_config(L, n_importance=0)), EINVAL), (dict(cfg=_config(L, mode=5)), EINVAL), (dict(cfg=_config(L, H=0)), EINVAL),
        (dict(cfg=_config(L, n_samples=600, n_importance=600)), ERANGE), (dict(cfg=_config(L, H=40000, W=40000)), ERANGE),
    ]
    for kw, code in refused_by_both:
        assert call(**kw) == (0, code), (kw, call(**kw))
    # LAYERS32 over more rows than plnerf_gemm_f32 takes: bounded by max_net_rows, refused without the bound
    big = _config(L, max_rays=1 << 18)
    assert call(cfg=big, io=_io(L, keep, max_net_rows=1 << 23)) == (0, ERANGE)
    assert call(cfg=big, io=_io(L, keep, max_net_rows=1 << 21), args=L.ViewArgs(n_pix=46))[1] == ERANGE      # (only the pixels are wrong)

    refused_by_the_entry = [
        (dict(ws_bytes=need - 1), EINVAL), (dict(ws=4096 + 4), EINVAL), (dict(ws=4096 + 128), EINVAL), (dict(ws=None), EINVAL),
        (dict(args=L.ViewArgs(pix0=1, n_pix=45)), ERANGE), (dict(args=L.ViewArgs(pix0=40, n_pix=6)), ERANGE),      # 5 x 9 = 45 pixels
        (dict(args=L.ViewArgs(pix0=-1, n_pix=5)), EINVAL), (dict(args=L.ViewArgs(n_pix=0)), EINVAL),
        (dict(io=_io(L, keep, fine=slot(LAYERS32, params=None))), EINVAL),
        (dict(io=_io(L, keep, fine=slot(CHAIN16, params=_param_table(26, null_at=25)))), EINVAL),
    ]
    for kw, code in refused_by_the_entry:
        got = call(**kw)
        assert got[0] > 0 and got[1] == code, (kw, got)
    for missing in ("t_vals", "rgb"):
        io = _io(L, keep)
        setattr(io, missing, None)
        assert call(io=io)[1] == EINVAL, missing
    io = _io(L, keep)
    io.coarse.fused.packed = None
    assert call(io=io)[1] == EINVAL
    io = _io(L, keep)
    io.coarse.fused.params[18] = 4096 + 4      # feature_linear.weight off 16 bytes
    assert call(io=io)[1] == EINVAL
    io = _io(L, keep)
    io.depth16 = 4096
    assert call(io=io)[1] == EINVAL            # depth16 without a depth plane
    io = _io(L, keep)
    io.u_vals = None                           # det draws without u_vals
    assert call(cfg=_config(L, perturb=0), io=io)[1] == EINVAL
    assert entry(None, None, None, None, 0, None) == EINVAL and query(None, None) == 0
    assert query(ctypes.byref(_config(L)), None) == 0


# ----------------------------------------------------------------------------- the host side
def test_the_host_program_compiles_without_a_device(L, tmp_path):
    """... and, run with no arguments, prints its usage line and leaves with status 2 before any call into the runtime."""
    run = c_hosts.run(c_hosts.build("c_abi_anyview_gpu", tmp_path))
    assert run.returncode == 2 and run.stdout == "", (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert run.stderr.startswith("usage: ") and run.stderr.count("\n") == 1, run.stderr[-2000:]


def test_unsupported_configurations_have_a_reason(L):
    """Without a GPU nothing is served; the reasons come before any device work, and the exports are in place."""
    import plnerf_amd
    from plnerf_amd import anyview, evaluate, view
    import inspect
    assert plnerf_amd.AnyViewRenderer is anyview.AnyViewRenderer and "AnyViewRenderer" in plnerf_amd.__all__
    assert anyview.AnyViewRenderer.unsupported_reason({}) is not None
    assert not anyview.AnyViewRenderer.supported({"network_fn": None, "network_fine": None})
    with pytest.raises(ValueError, match="two networks"):
        anyview.AnyViewRenderer({}, 4, 4, [[1, 0, 2], [0, 1, 2], [0, 0, 1]], 16, 2.0, 6.0)
    with pytest.raises(ValueError, match="two networks"):      # neither renderer serves it: ViewRenderer's refusal, as before
        view.render_path_frames([], (4, 4, 1.0), [[1, 0, 2], [0, 1, 2], [0, 0, 1]], 16, {})
    from plnerf_amd.render import MAX_ROWS_PER_LAUNCH
    assert inspect.signature(view.render_path_frames).parameters["max_net_rows"].default == MAX_ROWS_PER_LAUNCH
    assert inspect.signature(evaluate.render_images_with_metrics).parameters["one_call"].default is False
