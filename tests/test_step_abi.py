"""The C ABI of the one-call training step (include/plnerf_hip_step.h), without a GPU: the header is plain C99 and links
against the library, the library exports the two entry points, the four ctypes Structures have the compiler's sizes, and
plnerf_train_step's argument checks run before any device work.  (_lib.STEP_SIGNATURES and the Structures against the
header, field by field: tests/test_abi_headers.py.)"""
import ctypes
import subprocess

import pytest

import abi_support as abi

STRUCTS = ("plnerf_step_config", "plnerf_step_net", "plnerf_step_io", "plnerf_step_args")


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_library_exports_the_step_entries(L):
    """Fails on a library built without csrc/train_step.hip."""
    entries = {"plnerf_train_step", "plnerf_train_step_workspace_bytes"}
    assert set(L.STEP_SIGNATURES) == entries <= abi.exported_symbols(L.LIB_PATH)
    assert set(L.STEP_STRUCTS) == set(STRUCTS)


_C = r"""
#include <stdio.h>
#include <string.h>
#include "plnerf_hip_step.h"

static plnerf_step_config good_config(void) {
    plnerf_step_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = 1024; c.n_samples = 128; c.n_importance = 64; c.mode = PLNERF_MODE_LINEAR; c.color_mode = PLNERF_COLOR_MIDPOINT;
    c.perturb = 1; c.white_bkgd = 1; c.zero_tol = 1e-4f; c.epsilon = 1e-3f; c.H = 400; c.W = 400; c.fx = 555.f; c.fy = 555.f;
    c.cx = 200.f; c.cy = 200.f; c.near = 2.f; c.far = 6.f; c.precision = PLNERF_PREC_F16X3; c.fwd_kernel = PLNERF_FWD_KERNEL_AUTO;
    c.input_ch = 63; c.input_ch_views = 27; c.ray_source = PLNERF_STEP_RAYS_VIEW; c.beta1 = 0.9f; c.beta2 = 0.999f;
    c.adam_eps = 1e-8f; c.seed = 7;
    return c;
}

int main(int argc, char** argv) {
    size_t (*q)(const plnerf_step_config*) = plnerf_train_step_workspace_bytes;
    int (*p)(const plnerf_step_config*, const plnerf_step_io*, const plnerf_step_args*, void*, size_t, plnerf_stream_t) =
        plnerf_train_step;
    plnerf_step_config c = good_config(), bad;
    plnerf_step_io io;
    plnerf_step_args a;
    /* never dereferenced: every call below is refused by the argument checks, before any device work */
    static float host[PLNERF_N_PARAMS + 64];
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    size_t need;
    int i;
    if (argc > 1) {
        printf("%zu %zu %zu %zu\n", sizeof(plnerf_step_config), sizeof(plnerf_step_net), sizeof(plnerf_step_io), sizeof(plnerf_step_args));
        return 0;
    }
    if (plnerf_version() != PLNERF_VERSION) return 2;
    need = q(&c);
    if (need == 0 || need % 256 != 0 || q(NULL) != 0) return 3;
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + i; io.fine.params[i] = host + i; }
    io.coarse.param_flat = io.coarse.grad_flat = io.coarse.exp_avg = io.coarse.exp_avg_sq = host;
    io.fine = io.coarse;
    io.coarse.n_params = io.fine.n_params = PLNERF_N_PARAMS;
    io.coarse.packed = io.fine.packed = host;
    io.t_vals = host; io.loss4 = host;
    a.rays = 1024; a.image = host; a.crop_rows = 400; a.crop_cols = 400; a.adam_step_fine = 1; a.adam_step_coarse = 1;
    a.loss_scale = 1.f; a.lr_fine = a.lr_coarse = 5e-4f;
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 4;                 /* null config */
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return 5;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return 6;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return 7;
    a.rays = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 8;                   /* R = 0 */
    a.rays = 1025;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 9;                   /* R > max_rays */
    a.rays = 1024;
    bad = c; bad.mode = PLNERF_MODE_CONSTANT;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 10; /* unsupported mode */
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS) return 11;                /* unknown precision */
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 12;                /* S + N > 1024 */
    bad = c; bad.n_importance = 2147483647;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 22; /* no signed overflow in S + N */
    bad = c; bad.max_rays = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 13;
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return 14;              /* workspace too small */
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return 15;       /* ... or misaligned */
    a.ray_id0 = 400 * 400 - 1000;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 16;                  /* rays past the pixel window */
    a.ray_id0 = 0;
    io.fine.params[5] = host + PLNERF_N_PARAMS;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 17;                  /* a parameter outside its flat buffer */
    io.fine.params[5] = host + 5;
    io.loss4 = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 18;
    io.loss4 = host;
    bad = c; bad.perturb = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 19;                /* det draws without u_vals */
    bad = c; bad.ray_source = PLNERF_STEP_RAYS_BANK; bad.n_views = 3;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 20;                /* bank source without its arrays */
    a.adam_step_fine = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 21;
    printf("step abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("step_abi"), "step_abi")


def test_step_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "step abi ok" in out.stdout


def test_structure_sizes_are_the_compilers(L, c_host):
    out = subprocess.run([c_host, "sizes"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    sizes = [int(x) for x in out.stdout.split()]
    assert sizes == [ctypes.sizeof(L.STEP_STRUCTS[n]) for n in STRUCTS]


def test_ctypes_calls_are_refused_without_a_device(L):
    """The same checks through the binding: a null config, R = 0, an unsupported mode."""
    lib = L.lib()
    assert lib.plnerf_train_step(None, None, None, None, 0, None) == -1
    cfg = L.StepConfig(max_rays=256, n_samples=64, n_importance=128, mode=L.MODE["constant"], precision=L.PRECISION["f16x3"],
                       H=8, W=8, input_ch=63, input_ch_views=27)
    assert lib.plnerf_train_step_workspace_bytes(ctypes.byref(cfg)) == 0
    assert lib.plnerf_train_step(ctypes.byref(cfg), ctypes.byref(L.StepIo()), ctypes.byref(L.StepArgs()), None, 0, None) == -1
    cfg.mode = L.MODE["linear"]
    nbytes = lib.plnerf_train_step_workspace_bytes(ctypes.byref(cfg))
    assert nbytes > 256 * 192 * 4 * 4 and nbytes % L.STEP_WORKSPACE_ALIGN == 0
    args = L.StepArgs(rays=0)
    assert lib.plnerf_train_step(ctypes.byref(cfg), ctypes.byref(L.StepIo()), ctypes.byref(args), ctypes.c_void_p(256), nbytes,
                                 None) == -1
