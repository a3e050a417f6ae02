"""The experimental header include/experimental/plnerf_hip_depthview.h, without a GPU.  It lies outside the registry
(_lib.HEADERS, whose glob include/plnerf_hip*.h is not recursive), so what tests/test_abi_headers.py and
tests/test_containment_table.py give a registered header is restated here for the one row of _lib.EXPERIMENTAL_HEADERS: the
names against the table and the library, the signatures argument by argument, the struct mirrors field by field, what lib()
bound, a guard-band case for every entry that takes a stream (tests/depthview_cases.py, run on the GPU by
tests/test_gpu_depth_view.py); and what is specific to this header: a C99 host with the struct sizes, every refusal on fake
pointers and the workspace query, and the host side of render_video_frames (file names, the 16-bit PNG)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import abi_support as abi
import containment as C
import depthview_cases as cases

HEADER = "experimental/plnerf_hip_depthview.h"
STRUCTS = ("plnerf_depth_view_config", "plnerf_depth_view_io", "plnerf_depth_view_args")
ENTRIES = {"plnerf_depth_view_rays", "plnerf_frame_export_u16", "plnerf_depth_render_view_workspace_bytes",
           "plnerf_depth_render_view"}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
EINVAL, ERANGE, ENOSYS = -1, -3, -4


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.EXPERIMENTAL_HEADERS) == 1
    header, signatures, mirrors = L.EXPERIMENTAL_HEADERS[0]
    assert header == HEADER
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


# ----------------------------------------------------------------------------- the registry's checks, for this row
def test_names_agree(L, row):
    path, signatures, mirrors = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert set(mirrors) == set(STRUCTS) == set(abi.structs(path))


def _structs(L):
    """The registered ABI's struct mirrors (plnerf_view_net is reused from plnerf_hip_view.h) and this header's."""
    return {**abi.abi_structs(), **L.EXPERIMENTAL_HEADERS[0][2]}


def _check_type(L, where, c_type, ct):
    """tests/test_abi_headers.py's rule for one return or argument type."""
    assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
    t = abi.bare(c_type)
    if abi.c_class(c_type) != "ptr":
        assert ct is abi.SCALARS[t], (where, c_type, ct)
        return
    pointee = t[:-1].strip() if t.endswith("*") else None
    if pointee in _structs(L):
        assert ct is ctypes.POINTER(_structs(L)[pointee]), (where, c_type, ct)
    elif ct is not ctypes.c_void_p:
        assert pointee, (where, c_type, ct, "the stream is c_void_p")
        assert ct is ctypes.POINTER(abi.SCALARS[pointee]), (where, c_type, ct)


def test_signatures_agree(L, row):
    path, signatures, _ = row
    protos = abi.prototypes(path)
    for name, (ret, params) in protos.items():
        res, args = signatures[name]
        _check_type(L, (name, "return"), ret, res)
        assert len(args) == len(params), (name, len(args), len(params))
        for k, (c_type, ct) in enumerate(zip(params, args)):
            _check_type(L, (name, k), c_type, ct)


def test_struct_mirrors_agree(L, row):
    path, _, mirrors = row
    for name, fields in abi.structs(path).items():
        mirror = mirrors[name]._fields_
        assert [f[0] for f in mirror] == [f[1] for f in fields], name
        for (fname, ftype), (c_type, _, length) in zip(mirror, fields):
            t = abi.bare(c_type)
            want = _structs(L)[t] if t in _structs(L) else abi.expected_ctype(c_type)
            if length is None:
                assert ftype is want, (name, fname, ftype, want)
            else:
                assert ftype._type_ is want and ftype._length_ == int(length), (name, fname)


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_registered_abi_is_what_it_was(L):
    """The experimental row shares no name with the registry and adds nothing to it.  (The registry holds ten headers; the
    names are spelled out so that a row slipped into it fails here.)"""
    assert not set(L.EXPERIMENTAL_SIGNATURES) & set(L.ALL_SIGNATURES)
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601
    with pytest.raises(ValueError, match="one entry point, one header"):
        L._disjoint({"plnerf_version": None}, L.ALL_SIGNATURES)


# ----------------------------------------------------------------------------- guard-band cases exist and restate the prototypes
def test_every_entry_with_a_stream_has_a_guard_band_case(L, row):
    path, signatures, _ = row
    protos = abi.prototypes(path)
    built = [(case_id, build(L)) for case_id, build in cases.all_cases()]
    assert len({case_id for case_id, _ in built}) == len(built)
    covered = {call.entry for _, calls in built for call in calls}
    with_stream = {name for name, (_, params) in protos.items() if "plnerf_stream_t" in params}
    assert covered == with_stream, covered ^ with_stream
    assert set(protos) - with_stream == cases.NO_DEVICE_WRITES
    for _, calls in built:
        C.case_buffers(calls)      # (one Buf per name)
        for call in calls:
            ret, params = protos[call.entry]
            assert ret == "int" and params[-1] == "plnerf_stream_t", call.entry
            C.check_against_prototype(call, params, signatures[call.entry][1])


# ----------------------------------------------------------------------------- a C99 host
_C = r"""
#include <stdio.h>
#include <string.h>
#include "experimental/plnerf_hip_depthview.h"
#include "plnerf_hip_depthstep.h" /* (the training step's size, to compare with) */
#include "plnerf_hip_conststep.h"

static plnerf_depth_view_config good_config(void) {
    plnerf_depth_view_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = 1024; c.n_samples = 128; c.n_importance = 64; c.mode = PLNERF_MODE_LINEAR; c.color_mode = PLNERF_COLOR_MIDPOINT;
    c.perturb = 1; c.white_bkgd = 1; c.zero_tol = 1e-4f; c.epsilon = 1e-3f; c.H = 400; c.W = 400; c.near = 2.f; c.far = 6.f;
    c.precision = PLNERF_PREC_F16X3; c.fwd_kernel = PLNERF_FWD_KERNEL_AUTO; c.input_ch = 57; c.input_ch_views = 3;
    c.input_scale = 3.14159265f; c.density_beta = 10.f; c.seed = 7;
    return c;
}

/* the training step's configuration of the same shapes */
static plnerf_depth_step_config step_config(const plnerf_depth_view_config* v) {
    plnerf_depth_step_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = v->max_rays; c.n_samples = v->n_samples; c.n_importance = v->n_importance; c.color_mode = v->color_mode;
    c.perturb = v->perturb; c.white_bkgd = v->white_bkgd; c.raw_noise_std = v->raw_noise_std; c.zero_tol = v->zero_tol;
    c.epsilon = v->epsilon; c.n_views = 1; c.H = v->H; c.W = v->W; c.n_hyp = 1; c.pose_rows = 3; c.near = v->near; c.far = v->far;
    c.precision = v->precision; c.fwd_kernel = v->fwd_kernel; c.input_ch = v->input_ch; c.input_ch_views = v->input_ch_views;
    c.input_scale = v->input_scale; c.density_beta = v->density_beta; c.seed = v->seed;
    return c;
}

int main(int argc, char** argv) {
    size_t (*q)(const plnerf_depth_view_config*) = plnerf_depth_render_view_workspace_bytes;
    int (*p)(const plnerf_depth_view_config*, const plnerf_depth_view_io*, const plnerf_depth_view_args*, void*, size_t,
             plnerf_stream_t) = plnerf_depth_render_view;
    plnerf_depth_view_config c = good_config(), bad;
    plnerf_depth_step_config sc;
    plnerf_depth_view_io io;
    plnerf_depth_view_args a;
    /* never dereferenced: every call below is refused by the argument checks, before any device work */
    static float host[1024];
    static double row[2];
    static uint8_t bytes[16];
    static uint16_t shorts[16];
    const float c2w[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4};
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    size_t need, last;
    int i;
    if (argc > 1) {
        printf("%zu %zu %zu\n", sizeof(plnerf_depth_view_config), sizeof(plnerf_depth_view_io), sizeof(plnerf_depth_view_args));
        return 0;
    }
    if (plnerf_version() != PLNERF_VERSION) return 2;

    /* ---- the workspace query ---- */
    need = q(&c);
    if (need == 0 || need % 256 != 0 || q(NULL) != 0) return 3;
    sc = step_config(&c);
    if (plnerf_depth_train_step_workspace_bytes(&sc) == 0 || need >= plnerf_depth_train_step_workspace_bytes(&sc)) return 30;
    last = 0;
    for (i = 1; i <= 40000; i = i * 3 + 1) {                                         /* monotone in max_rays */
        bad = c; bad.max_rays = i;
        if (q(&bad) == 0 || q(&bad) < last) return 31;
        last = q(&bad);
        sc = step_config(&bad);
        if (q(&bad) >= plnerf_depth_train_step_workspace_bytes(&sc)) return 36;
    }
    bad = c; bad.mode = PLNERF_MODE_CONSTANT;                                        /* both modes, one entry */
    sc = step_config(&bad);
    if (q(&bad) == 0 || q(&bad) >= plnerf_depth_train_step_const_workspace_bytes(&sc)) return 32;
    bad.n_samples = 2;
    if (q(&bad) != 0) return 33;                                                     /* constant mode needs 3 samples */
    bad = c; bad.raw_noise_std = 1.f;
    sc = step_config(&bad);
    if (q(&bad) <= need || q(&bad) >= plnerf_depth_train_step_workspace_bytes(&sc)) return 34;

    /* ---- plnerf_depth_render_view ---- */
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + 4 * i; io.fine.params[i] = host + 4 * i; }
    io.coarse.packed = io.fine.packed = host;
    io.t_vals = host; io.rgb = host;
    memcpy(a.c2w, c2w, sizeof c2w);
    a.fx = 555.f; a.fy = 556.f; a.cx = 200.f; a.cy = 200.f;
    a.n_pix = 400 * 400; a.pack_weights = 1; a.depth16_scale = 1.f / 6.f; a.depth_mm_mult = 1000.f;
    if (((uintptr_t)host % 16) != 0) return 29;                                      /* (static storage: the aligned case below) */
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 4;                 /* null config */
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return 5;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return 6;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return 7;
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return 8;               /* workspace too small */
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return 9;        /* ... or misaligned */
    bad = c; bad.n_importance = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 10;
    bad = c; bad.mode = 5;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 11;
    bad = c; bad.color_mode = 2;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 26;
    bad = c; bad.fwd_kernel = 9;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 27;
    bad = c; bad.input_ch = 58;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 28;
    bad = c; bad.input_scale = 0.f;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 37;
    bad = c; bad.density_beta = -1.f;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 38;
    bad = c; bad.raw_noise_std = -1.f;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 39;
    bad = c; bad.H = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 60;
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS || q(&bad) != 0) return 12; /* a precision that is not built */
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 13; /* S + N over PLNERF_MAX_SAMPLES */
    bad = c; bad.max_rays = 1 << 24;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 14; /* the row-count overflow */
    bad = c; bad.H = 40000; bad.W = 40000;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 61; /* H W over 2^30 */
    bad = c; bad.max_rays = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 15;
    a.pix0 = 1;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 16;                  /* pixels past H W */
    a.pix0 = 400 * 400 - 5; a.n_pix = 6;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 17;
    a.pix0 = -1; a.n_pix = 5;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 18;
    a.pix0 = 0; a.n_pix = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 19;
    a.n_pix = 400 * 400;
    a.fx = 0.f;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 62;                  /* a focal length of 0 */
    a.fx = 555.f; a.fy = 0.f;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 63;
    a.fy = 556.f;
    io.rgb = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 20;                  /* the one required plane */
    io.rgb = host; io.t_vals = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 21;
    io.t_vals = host; io.fine.params[5] = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 22;
    io.fine.params[5] = host; io.coarse.packed = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 23;
    io.coarse.packed = host;
    bad = c; bad.perturb = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 24;                /* det draws without u_vals */
    io.valid = bytes;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 64;                  /* valid without error_row */
    io.valid = NULL; io.error_row = row;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 65;                  /* ... and the reverse */
    io.error_row = NULL;
    io.depth16 = shorts;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 25;                  /* depth16 without a depth plane */
    io.depth16 = NULL; io.depth_mm16 = shorts;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 66;                  /* depth_mm16 without a depth plane */
    io.depth_mm16 = NULL;
    io.depth = host; io.depth16 = (uint16_t*)((char*)shorts + 1);
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 69;                  /* depth16 off 2 bytes */
    io.depth16 = NULL; io.depth_mm16 = (uint16_t*)((char*)shorts + 1);
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 70;                  /* depth_mm16 off 2 bytes */
    io.depth_mm16 = NULL; io.depth = NULL;
    io.valid = bytes; io.error_row = (double*)((char*)row + 4);
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 71;                  /* error_row off 8 bytes */
    io.valid = NULL; io.error_row = NULL;
    bad = c; bad.n_importance = 2147483647;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 72; /* no signed overflow in S + N */
    bad = c; bad.n_samples = 2147483647;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 73;
    io.coarse.params[18] = host + 1;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 67;                  /* feature_linear.weight off 16 bytes */
    io.coarse.params[18] = host; io.fine.params[19] = host + 3;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 68;                  /* ... and the fine network's bias */
    io.fine.params[19] = host;

    /* ---- plnerf_depth_view_rays: plnerf_view_rays' refusals ---- */
    if (plnerf_depth_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, NULL, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 40;
    if (plnerf_depth_view_rays(0, 13, 10.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 41;
    if (plnerf_depth_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, -1, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 42;
    if (plnerf_depth_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 0, -1, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 43;
    if (plnerf_depth_view_rays(9, 13, 0.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 44;
    if (plnerf_depth_view_rays(9, 13, 10.f, 0.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 49;
    if (plnerf_depth_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 114, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_ERANGE) return 45;
    if (plnerf_depth_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, NULL, host, host, host, NULL) != PLNERF_EINVAL) return 46;
    if (plnerf_depth_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 117, 0, 2.f, 6.f, NULL, NULL, NULL, NULL, NULL, NULL) != PLNERF_OK) return 47;
    if (plnerf_depth_view_rays(40000, 40000, 10.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_ERANGE) return 48;

    /* ---- plnerf_frame_export_u16 ---- */
    if (plnerf_frame_export_u16(host, 1000.f, shorts, -1, NULL) != PLNERF_EINVAL) return 50;
    if (plnerf_frame_export_u16(NULL, 1000.f, shorts, 4, NULL) != PLNERF_EINVAL) return 51;
    if (plnerf_frame_export_u16(host, 1000.f, NULL, 4, NULL) != PLNERF_EINVAL) return 52;
    if (plnerf_frame_export_u16(host, 1000.f, (uint16_t*)((char*)shorts + 1), 4, NULL) != PLNERF_EINVAL) return 53;
    if (plnerf_frame_export_u16(NULL, 1000.f, NULL, 0, NULL) != PLNERF_OK) return 54;          /* nothing to do */
    if (plnerf_frame_export_u16(host, 1000.f, shorts, (1 << 30) + 1, NULL) != PLNERF_ERANGE) return 55;
    printf("depth view abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("depthview_abi"), "depthview_abi")


def test_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "depth view abi ok" in out.stdout


def test_structure_sizes_are_the_compilers(L, c_host):
    out = subprocess.run([c_host, "sizes"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert [int(x) for x in out.stdout.split()] == [ctypes.sizeof(L.DEPTHVIEW_STRUCTS[n]) for n in STRUCTS]


def test_ctypes_calls_are_refused_without_a_device(L):
    """The same checks through the binding."""
    lib = L.lib()
    assert lib.plnerf_depth_render_view(None, None, None, None, 0, None) == EINVAL
    assert lib.plnerf_depth_render_view_workspace_bytes(None) == 0
    cfg = cases.view_config(L, L.MODE["linear"])
    nbytes = lib.plnerf_depth_render_view_workspace_bytes(ctypes.byref(cfg))
    assert nbytes > 0 and nbytes % L.STEP_WORKSPACE_ALIGN == 0
    # at least one block's samples, positions and raw outputs of both passes: 8 floats per sample
    assert nbytes >= cfg.max_rays * (2 * cfg.n_samples + cfg.n_importance) * 8 * 4
    io, args = L.DepthViewIo(), L.DepthViewArgs(n_pix=64, fx=9.0, fy=9.0)
    ref = (ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(256), nbytes, None)
    assert lib.plnerf_depth_render_view(*ref) == EINVAL                      # no networks, no planes
    args.pix0, args.n_pix = 95, 5
    assert lib.plnerf_depth_render_view(*ref) == ERANGE                      # 9 x 11 = 99 pixels
    cfg.precision = 17
    assert lib.plnerf_depth_render_view(*ref) == ENOSYS
    c2w = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4)
    p = ctypes.c_void_p(256)
    assert lib.plnerf_depth_view_rays(8, 8, 9.0, 9.0, 4.0, 4.0, c2w, 60, 5, 2.0, 6.0, p, p, None, p, p, None) == ERANGE
    assert lib.plnerf_depth_view_rays(8, 8, 9.0, 9.0, 4.0, 4.0, c2w, 0, 5, 2.0, 6.0, p, p, None, None, p, None) == EINVAL
    assert lib.plnerf_frame_export_u16(p, 1000.0, None, 5, None) == EINVAL
    assert lib.plnerf_frame_export_u16(None, 1000.0, None, 0, None) == 0


# ----------------------------------------------------------------------------- the host side of render_video_frames
def test_frame_names_are_render_videos(L):
    from plnerf_amd import depthview
    assert [depthview.frame_name(i) for i in (0, 7, 12, 123)] == ["0.png", "7.png", "12.png", "123.png"]      # str(idx) + '.png'
    import plnerf_amd
    assert plnerf_amd.render_video_frames is depthview.render_video_frames
    assert plnerf_amd.DepthViewRenderer is depthview.DepthViewRenderer


def test_millimetre_plane_round_trips_through_the_png(L, tmp_path):
    """The staging buffer holds the uint16 codes as int16 bit patterns; what render_video_frames writes from it is read back
    as the same uint16 values, codes above 32767 included."""
    from plnerf_amd import depthview, png
    codes = np.array([[0, 1, 999, 32767], [32768, 40000, 65534, 65535], [2500, 6000, 258, 513]], dtype=np.uint16)
    staged = codes.view(np.int16)
    path = str(tmp_path / depthview.frame_name(3))
    png.write_png(path, staged.view(np.uint16))
    back = png.read_png(path)
    assert back.dtype == np.uint16 and back.shape == codes.shape and np.array_equal(back, codes)
    with pytest.raises(ValueError):
        png.write_png(path, staged)      # int16 itself is not a PNG sample type: the view is what is written


def test_unsupported_configurations_have_a_reason(L):
    """Without a GPU nothing is served; the reasons come before any device work."""
    from plnerf_amd import depthview
    assert depthview.DepthViewRenderer.unsupported_reason({}) is not None
    assert not depthview.DepthViewRenderer.supported({"network_fn": None, "network_fine": None})
    with pytest.raises(ValueError, match="two networks"):
        depthview.DepthViewRenderer({}, 4, 4, 16, 2.0, 6.0)
