"""The C ABI of the one-call view render (include/plnerf_hip_view.h), without a GPU: the header is plain C99 and links
against the library, the ctypes Structures have the compiler's sizes, the workspace query answers 0 for a refused
configuration, grows with max_rays and stays below the training step's, and every refusal of plnerf_view_rays,
plnerf_frame_export and plnerf_render_view comes back before any device work.  (_lib.VIEW_SIGNATURES and the Structures
against the header, field by field: tests/test_abi_headers.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

import abi_support as abi

STRUCTS = ("plnerf_view_net", "plnerf_view_io", "plnerf_view_args")
EINVAL, ERANGE, ENOSYS = -1, -3, -4


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_error_codes_are_the_headers(L):
    code = open(os.path.join(abi.INCLUDE, "plnerf_hip.h")).read()
    for name, value in (("EINVAL", EINVAL), ("ERANGE", ERANGE), ("ENOSYS", ENOSYS)):
        assert int(re.search(r"#define\s+PLNERF_%s\s+\(?(-?\d+)\)?" % name, code).group(1)) == value


def test_library_exports_the_view_entries(L):
    """Fails on a library built without csrc/view.hip and csrc/render_view.hip."""
    entries = {"plnerf_view_rays", "plnerf_frame_export", "plnerf_render_view_workspace_bytes", "plnerf_render_view"}
    assert set(L.VIEW_SIGNATURES) == entries <= abi.exported_symbols(L.LIB_PATH)
    assert set(L.VIEW_STRUCTS) == set(STRUCTS)


_C = r"""
#include <stdio.h>
#include <string.h>
#include "plnerf_hip_view.h"
#include "plnerf_hip_conststep.h" /* (the constant-mode step's size, to compare with) */

static plnerf_step_config good_config(void) {
    plnerf_step_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = 1024; c.n_samples = 128; c.n_importance = 64; c.mode = PLNERF_MODE_LINEAR; c.color_mode = PLNERF_COLOR_MIDPOINT;
    c.perturb = 1; c.white_bkgd = 1; c.zero_tol = 1e-4f; c.epsilon = 1e-3f; c.H = 400; c.W = 400; c.fx = 555.f; c.fy = 555.f;
    c.cx = 200.f; c.cy = 200.f; c.near = 2.f; c.far = 6.f; c.precision = PLNERF_PREC_F16X3; c.fwd_kernel = PLNERF_FWD_KERNEL_AUTO;
    c.input_ch = 63; c.input_ch_views = 27; c.seed = 7;
    return c;
}

int main(int argc, char** argv) {
    size_t (*q)(const plnerf_step_config*) = plnerf_render_view_workspace_bytes;
    int (*p)(const plnerf_step_config*, const plnerf_view_io*, const plnerf_view_args*, void*, size_t, plnerf_stream_t) =
        plnerf_render_view;
    plnerf_step_config c = good_config(), bad;
    plnerf_view_io io;
    plnerf_view_args a;
    /* never dereferenced: every call below is refused by the argument checks, before any device work */
    static float host[1024];
    static uint8_t bytes[16];
    static uint16_t shorts[16];
    const float c2w[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4};
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    size_t need, last;
    int i;
    if (argc > 1) {
        printf("%zu %zu %zu\n", sizeof(plnerf_view_net), sizeof(plnerf_view_io), sizeof(plnerf_view_args));
        return 0;
    }
    if (plnerf_version() != PLNERF_VERSION) return 2;

    /* ---- the workspace query ---- */
    need = q(&c);
    if (need == 0 || need % 256 != 0 || q(NULL) != 0) return 3;
    if (need >= plnerf_train_step_workspace_bytes(&c)) return 30;                   /* nothing saved, no backward scratch */
    last = 0;
    for (i = 1; i <= 40000; i = i * 3 + 1) {                                         /* non-decreasing in max_rays */
        bad = c; bad.max_rays = i;
        if (q(&bad) == 0 || q(&bad) < last) return 31;
        last = q(&bad);
    }
    bad = c; bad.mode = PLNERF_MODE_CONSTANT;                                        /* both modes, one entry */
    if (q(&bad) == 0 || q(&bad) >= plnerf_train_step_const_workspace_bytes(&bad)) return 32;
    bad.n_samples = 2;
    if (q(&bad) != 0) return 33;                                                     /* constant mode needs 3 samples */
    bad = c; bad.raw_noise_std = 1.f; bad.ndc = 1; bad.ndc_focal = 555.0;
    if (q(&bad) <= need || q(&bad) >= plnerf_train_step_workspace_bytes(&bad)) return 34;
    bad = c; bad.ray_source = 99; bad.n_views = -1; bad.beta1 = -1.f;                /* ignored fields */
    if (q(&bad) != need) return 35;

    /* ---- plnerf_render_view ---- */
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + i; io.fine.params[i] = host + i; }
    io.coarse.packed = io.fine.packed = host;
    io.t_vals = host; io.rgb = host;
    memcpy(a.c2w, c2w, sizeof c2w);
    a.n_pix = 400 * 400; a.pack_weights = 1; a.depth16_scale = 1.f / 6.f;
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
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS || q(&bad) != 0) return 12; /* a precision that is not built */
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 13; /* S + N > 1024 */
    bad = c; bad.n_importance = 2147483647;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 70; /* no signed overflow in S + N */
    bad = c; bad.max_rays = 1 << 24;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 14; /* the row-count overflow */
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
    io.depth16 = shorts;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 25;                  /* depth16 without a depth plane */
    io.depth16 = NULL;

    /* ---- plnerf_view_rays ---- */
    if (plnerf_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, NULL, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 40;
    if (plnerf_view_rays(0, 13, 10.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 41;
    if (plnerf_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, -1, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 42;
    if (plnerf_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 0, -1, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 43;
    if (plnerf_view_rays(9, 13, 0.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_EINVAL) return 44;
    if (plnerf_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 114, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_ERANGE) return 45;
    if (plnerf_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, NULL, host, host, host, NULL) != PLNERF_EINVAL) return 46;
    if (plnerf_view_rays(9, 13, 10.f, 11.f, 6.f, 4.f, c2w, 117, 0, 2.f, 6.f, NULL, NULL, NULL, NULL, NULL, NULL) != PLNERF_OK) return 47;
    if (plnerf_view_rays(40000, 40000, 10.f, 11.f, 6.f, 4.f, c2w, 0, 4, 2.f, 6.f, host, host, host, host, host, NULL) != PLNERF_ERANGE) return 48;

    /* ---- plnerf_frame_export ---- */
    if (plnerf_frame_export(host, bytes, NULL, 1.f, NULL, -1, NULL) != PLNERF_EINVAL) return 50;
    if (plnerf_frame_export(host, NULL, NULL, 1.f, NULL, 4, NULL) != PLNERF_EINVAL) return 51;   /* a plane without its output */
    if (plnerf_frame_export(NULL, bytes, NULL, 1.f, NULL, 4, NULL) != PLNERF_EINVAL) return 52;
    if (plnerf_frame_export(NULL, NULL, host, 1.f, NULL, 4, NULL) != PLNERF_EINVAL) return 53;
    if (plnerf_frame_export(NULL, NULL, NULL, 1.f, shorts, 4, NULL) != PLNERF_EINVAL) return 54;
    if (plnerf_frame_export(host, bytes, host, 1.f, shorts, 0, NULL) != PLNERF_OK) return 55;    /* nothing to do */
    if (plnerf_frame_export(NULL, NULL, NULL, 1.f, NULL, 4, NULL) != PLNERF_OK) return 56;
    if (plnerf_frame_export(host, bytes, NULL, 1.f, NULL, (1 << 30) + 1, NULL) != PLNERF_ERANGE) return 57;
    printf("view abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("view_abi"), "view_abi")


def test_view_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "view abi ok" in out.stdout


def test_structure_sizes_are_the_compilers(L, c_host):
    out = subprocess.run([c_host, "sizes"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    sizes = [int(x) for x in out.stdout.split()]
    assert sizes == [ctypes.sizeof(L.VIEW_STRUCTS[n]) for n in STRUCTS]


def _config(L, **over):
    cfg = L.StepConfig(max_rays=256, n_samples=64, n_importance=128, mode=L.MODE["linear"], precision=L.PRECISION["f16x3"],
                       H=8, W=8, fx=9.0, fy=9.0, cx=4.0, cy=4.0, near=2.0, far=6.0, input_ch=63, input_ch_views=27, perturb=1)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_workspace_is_smaller_than_the_training_steps_and_grows_with_the_block(L):
    lib = L.lib()
    sizes = []
    for max_rays in (1, 2, 50, 256, 257, 4096, 32768):
        cfg = _config(L, max_rays=max_rays)
        view, train = (fn(ctypes.byref(cfg)) for fn in (lib.plnerf_render_view_workspace_bytes, lib.plnerf_train_step_workspace_bytes))
        assert 0 < view < train and view % L.STEP_WORKSPACE_ALIGN == 0, (max_rays, view, train)
        # at least one block's samples, positions and raw outputs of both passes: 8 floats per sample
        assert view >= max_rays * (64 + 192) * 8 * 4
        sizes.append(view)
    assert sizes == sorted(sizes)
    for refused in (dict(n_importance=0), dict(max_rays=0), dict(mode=7), dict(precision=17), dict(n_samples=1), dict(H=0),
                    dict(fx=0.0), dict(input_ch=64), dict(n_samples=2, mode=L.MODE["constant"])):
        assert lib.plnerf_render_view_workspace_bytes(ctypes.byref(_config(L, **refused))) == 0, refused
    assert lib.plnerf_render_view_workspace_bytes(None) == 0


def test_ctypes_calls_are_refused_without_a_device(L):
    """The same checks through the binding."""
    lib = L.lib()
    assert lib.plnerf_render_view(None, None, None, None, 0, None) == EINVAL
    cfg = _config(L)
    nbytes = lib.plnerf_render_view_workspace_bytes(ctypes.byref(cfg))
    io, args = L.ViewIo(), L.ViewArgs(n_pix=64)
    assert lib.plnerf_render_view(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(256), nbytes, None) == EINVAL
    args = L.ViewArgs(pix0=60, n_pix=5)
    assert lib.plnerf_render_view(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ctypes.c_void_p(256), nbytes, None) == ERANGE
    c2w = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4)
    p = ctypes.c_void_p(256)
    assert lib.plnerf_view_rays(8, 8, 9.0, 9.0, 4.0, 4.0, c2w, 60, 5, 2.0, 6.0, p, p, None, p, p, None) == ERANGE
    assert lib.plnerf_view_rays(8, 8, 9.0, 9.0, 4.0, 4.0, c2w, 0, 5, 2.0, 6.0, p, p, None, None, p, None) == EINVAL
    assert lib.plnerf_frame_export(p, None, None, 1.0, None, 5, None) == EINVAL
    assert lib.plnerf_frame_export(None, None, None, 1.0, None, 5, None) == 0
