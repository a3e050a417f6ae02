"""The C ABI of the piecewise-constant one-call steps (include/plnerf_hip_conststep.h), without a GPU: the header is plain
C99 and links against the library, the library exports the six entry points, and every refusal comes before any device
work.  (_lib.CONSTSTEP_SIGNATURES against the header: tests/test_abi_headers.py.)"""
import ctypes
import subprocess

import pytest

import abi_support as abi

ENTRIES = {"plnerf_fine_epilogue_const_bwd", "plnerf_train_step_const_workspace_bytes", "plnerf_train_step_const",
           "plnerf_depth_train_step_const_workspace_bytes", "plnerf_depth_train_step_const_layout",
           "plnerf_depth_train_step_const"}


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_library_exports_the_const_entries(L):
    """Fails on a library built without csrc/epilogue_bwd.hip or the const entries of the step sources."""
    assert set(L.CONSTSTEP_SIGNATURES) == ENTRIES <= abi.exported_symbols(L.LIB_PATH)


_C = r"""
#include <stdio.h>
#include <string.h>
#include "plnerf_hip_conststep.h"

static plnerf_step_config nvs_config(void) {
    plnerf_step_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = 1024; c.n_samples = 128; c.n_importance = 64; c.mode = PLNERF_MODE_CONSTANT; c.color_mode = PLNERF_COLOR_MIDPOINT;
    c.perturb = 1; c.white_bkgd = 1; c.zero_tol = 1e-4f; c.epsilon = 1e-3f; c.H = 400; c.W = 400; c.fx = 555.f; c.fy = 555.f;
    c.cx = 200.f; c.cy = 200.f; c.near = 2.f; c.far = 6.f; c.precision = PLNERF_PREC_F16X3; c.fwd_kernel = PLNERF_FWD_KERNEL_AUTO;
    c.input_ch = 63; c.input_ch_views = 27; c.ray_source = PLNERF_STEP_RAYS_VIEW; c.beta1 = 0.9f; c.beta2 = 0.999f;
    c.adam_eps = 1e-8f; c.seed = 7;
    return c;
}

static plnerf_depth_step_config depth_config(void) {
    plnerf_depth_step_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = 1024; c.n_samples = 64; c.n_importance = 128; c.color_mode = PLNERF_COLOR_MIDPOINT; c.perturb = 1;
    c.white_bkgd = 1; c.zero_tol = 1e-4f; c.epsilon = 1e-3f; c.n_views = 3; c.H = 480; c.W = 640; c.n_hyp = 3; c.pose_rows = 4;
    c.near = 0.5f; c.far = 8.f; c.precision = PLNERF_PREC_F16X3; c.fwd_kernel = PLNERF_FWD_KERNEL_AUTO; c.input_ch = 57;
    c.input_ch_views = 3; c.input_scale = 3.14159265f; c.density_beta = 10.f; c.space_carving_weight = 0.007f;
    c.clip_value = 0.1f; c.beta1 = 0.9f; c.beta2 = 0.999f; c.adam_eps = 1e-8f; c.ss_beta1 = 0.9f; c.ss_beta2 = 0.999f;
    c.ss_adam_eps = 1e-8f; c.seed = 7;
    return c;
}

/* never dereferenced: every call below is refused by the argument checks (or has R == 0), before any device work */
static float host[PLNERF_N_PARAMS + 64];

static int nvs(void) {
    size_t (*q)(const plnerf_step_config*) = plnerf_train_step_const_workspace_bytes;
    int (*p)(const plnerf_step_config*, const plnerf_step_io*, const plnerf_step_args*, void*, size_t, plnerf_stream_t) =
        plnerf_train_step_const;
    plnerf_step_config c = nvs_config(), bad;
    plnerf_step_io io;
    plnerf_step_args a;
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    size_t need, linear;
    int i;
    need = q(&c);
    bad = c; bad.mode = PLNERF_MODE_LINEAR;
    linear = plnerf_train_step_workspace_bytes(&bad);
    if (need == 0 || need % 256 != 0 || linear == 0 || linear % 256 != 0 || q(NULL) != 0) return 3;
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
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 4;                 /* null structs */
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return 5;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return 6;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return 7;                 /* null workspace */
    a.rays = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 8;                   /* rays = 0 */
    a.rays = 1025;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 9;                   /* rays = max_rays + 1 */
    a.rays = 1024;
    bad = c; bad.mode = PLNERF_MODE_LINEAR;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 10; /* the linear entry's mode */
    bad = c; bad.n_samples = 2;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0) return 11; /* the sampler needs 3 depths */
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS) return 12;                /* unknown precision */
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 13;                /* S + N > 1024 */
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return 14;              /* workspace too small */
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return 15;       /* ... or misaligned */
    io.fine.params[5] = host + PLNERF_N_PARAMS;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 16;                  /* a parameter outside its flat buffer */
    return 0;
}

static int depth(void) {
    size_t (*q)(const plnerf_depth_step_config*) = plnerf_depth_train_step_const_workspace_bytes;
    int (*lay)(const plnerf_depth_step_config*, plnerf_depth_step_views*) = plnerf_depth_train_step_const_layout;
    int (*p)(const plnerf_depth_step_config*, const plnerf_depth_step_io*, const plnerf_depth_step_args*, void*, size_t,
             plnerf_stream_t) = plnerf_depth_train_step_const;
    plnerf_depth_step_config c = depth_config(), bad;
    plnerf_depth_step_io io;
    plnerf_depth_step_args a;
    plnerf_depth_step_views v, vl;
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    size_t need, linear;
    int i;
    need = q(&c);
    linear = plnerf_depth_train_step_workspace_bytes(&c);
    if (need == 0 || need % 256 != 0 || linear == 0 || linear % 256 != 0 || q(NULL) != 0) return 30;
    if (lay(&c, &v) != PLNERF_OK || lay(&c, NULL) != PLNERF_EINVAL || lay(NULL, &v) != PLNERF_EINVAL) return 31;
    if (plnerf_depth_train_step_layout(&c, &vl) != PLNERF_OK) return 32;
    /* the loss partials lie at offset 0 of both carves: everything behind them agrees, output by output */
    if (memcmp(&v, &vl, sizeof v) != 0 || v.rgb % 256 || v.rgb >= need || v.pred_hyp >= need) return 33;
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + i; }
    io.coarse.param_flat = io.coarse.grad_flat = io.coarse.exp_avg = io.coarse.exp_avg_sq = host;
    io.coarse.n_params = PLNERF_N_PARAMS;
    io.coarse.packed = host;
    io.fine = io.coarse;
    io.t_vals = host; io.loss5 = host; io.images = host; io.hyp = host; io.poses = host; io.intrinsics = host;
    a.rays = 1024; a.view = 2; a.adam_step = 1; a.lr = 5e-4f; a.carve = 1;
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 34;                /* null structs */
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return 35;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return 36;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return 37;
    a.rays = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 38;
    a.rays = 1025;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 39;
    a.rays = 1024;
    bad = c; bad.n_samples = 2;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0 || lay(&bad, &v) != PLNERF_EINVAL) return 40;
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS || q(&bad) != 0) return 41;
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 42; /* S + N over the limit */
    /* inside the linear step's limits, over the const backward's LDS row: 4 waves x (1000 + 6 * 999 + 4 * 900) floats */
    bad = c; bad.max_rays = 8; bad.n_samples = 100; bad.n_importance = 900;
    if (plnerf_depth_train_step_workspace_bytes(&bad) == 0 || q(&bad) != 0 || lay(&bad, &v) != PLNERF_ERANGE) return 43;
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return 44;              /* workspace too small */
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return 45;       /* ... or misaligned */
    io.fine.params[5] = host + PLNERF_N_PARAMS;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 46;                  /* a parameter outside its flat buffer */
    io.fine.params[5] = host + 5;
    a.ss_step = 1; a.ss_adam_step = 1;
    io.scale = io.shift = io.ss_grad = io.ss_exp_avg = io.ss_exp_avg_sq = host;
    a.carve = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 47;                  /* ss_step without carve */
    return 0;
}

static int kernel(void) {
    int (*k)(const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*,
             const float*, int, const int64_t*, int, int, int, int, const float*, const float*, const float*, const float*,
             const float*, float*, uint32_t*, plnerf_stream_t) = plnerf_fine_epilogue_const_bwd;
    const float* h = host;
    const int64_t* inds = (const int64_t*)host;
    if (k(h, h, h, h, h, NULL, h, h, h, 8, inds, 4, 2, 8, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 60; /* S = 2 */
    if (k(h, h, h, h, h, NULL, h, h, h, 0, inds, 4, 16, 0, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 61; /* N = 0 */
    if (k(h, h, h, h, h, NULL, h, h, h, 7, inds, 4, 16, 8, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 62; /* stride */
    if (k(h, h, h, h, h, NULL, h, h, h, 8, NULL, 4, 16, 8, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 63; /* g_hyp, no inds */
    if (k(h, h, h, h, h, NULL, h, NULL, h, 8, inds, 4, 16, 8, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 64; /* no bins */
    if (k(h, h, h, h, h, NULL, h, h, h, 8, inds, -1, 16, 8, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 65; /* R < 0 */
    if (k(h, h, h, h, h, NULL, h, h, h, 8, inds, 4, 16, 8, 0, NULL, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_EINVAL) return 66; /* no g_rgb */
    if (k(h, h, h, h, h, NULL, h, h, h, 8, inds, 4, 16, 8, 0, h, NULL, NULL, NULL, h, NULL, NULL, NULL) != PLNERF_EINVAL) return 67; /* no g_raw */
    if (k(h, h, h, h, h, NULL, h, h, h, 8, inds, 4, PLNERF_MAX_SAMPLES + 1, 8, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_ERANGE) return 68;
    if (k(h, h, h, h, h, NULL, h, h, h, 1025, inds, 4, 16, 1025, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_ERANGE) return 69;
    if (k(h, h, h, h, h, NULL, h, h, h, 1024, inds, 4, 1022, 1024, 0, h, NULL, NULL, NULL, h, host, NULL, NULL) != PLNERF_ERANGE) return 70; /* LDS row */
    if (k(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, 16, 8, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != PLNERF_OK) return 71; /* R = 0 */
    return 0;
}

int main(void) {
    int rc;
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    if ((rc = nvs()) || (rc = depth()) || (rc = kernel())) return rc;
    printf("conststep abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("conststep_abi"), "conststep_abi")


def test_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "conststep abi ok" in out.stdout


def test_const_and_linear_workspaces_share_one_layout(L):
    """Through the binding: both size queries are multiples of 256, and the layout query's offsets -- the loss partials at
    the head of the carve, every output behind them -- equal the linear layout's."""
    lib = L.lib()
    cfg = L.StepConfig(max_rays=256, n_samples=64, n_importance=128, mode=L.MODE["constant"], precision=L.PRECISION["f16x3"],
                       H=8, W=8, input_ch=63, input_ch_views=27)
    const = lib.plnerf_train_step_const_workspace_bytes(ctypes.byref(cfg))
    assert lib.plnerf_train_step_workspace_bytes(ctypes.byref(cfg)) == 0
    cfg.mode = L.MODE["linear"]
    linear = lib.plnerf_train_step_workspace_bytes(ctypes.byref(cfg))
    assert lib.plnerf_train_step_const_workspace_bytes(ctypes.byref(cfg)) == 0
    assert const > 0 and linear > 0 and const % L.STEP_WORKSPACE_ALIGN == 0 and linear % L.STEP_WORKSPACE_ALIGN == 0
    assert lib.plnerf_train_step_const(None, None, None, None, 0, None) == -1
    d = L.DepthStepConfig(max_rays=256, n_samples=64, n_importance=128, precision=L.PRECISION["f16x3"], n_views=2, H=8, W=8,
                          n_hyp=3, pose_rows=4, input_ch=57, input_ch_views=3, input_scale=1.0)
    dc = lib.plnerf_depth_train_step_const_workspace_bytes(ctypes.byref(d))
    dl = lib.plnerf_depth_train_step_workspace_bytes(ctypes.byref(d))
    assert dc > 0 and dl > 0 and dc % L.STEP_WORKSPACE_ALIGN == 0 and dl % L.STEP_WORKSPACE_ALIGN == 0
    vc, vl = L.DepthStepViews(), L.DepthStepViews()
    assert lib.plnerf_depth_train_step_const_layout(ctypes.byref(d), ctypes.byref(vc)) == 0
    assert lib.plnerf_depth_train_step_layout(ctypes.byref(d), ctypes.byref(vl)) == 0
    assert [getattr(vc, n) for n in L.DEPTH_STEP_VIEWS] == [getattr(vl, n) for n in L.DEPTH_STEP_VIEWS]
    assert lib.plnerf_depth_train_step_const(None, None, None, None, 0, None) == -1
