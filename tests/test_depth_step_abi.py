"""The C ABI of the depth-supervised one-call step (include/plnerf_hip_depthstep.h), without a GPU: the header is plain C99
and links against the library, the library exports the four entry points, the four ctypes Structures have the compiler's
sizes, and plnerf_depth_train_step's argument checks run before any device work.  (_lib.DEPTHSTEP_SIGNATURES and the
Structures against the header, field by field: tests/test_abi_headers.py.)"""
import ctypes
import os
import re
import subprocess

import pytest

import abi_support as abi

HEADER = os.path.join(abi.INCLUDE, "plnerf_hip_depthstep.h")
STRUCTS = ("plnerf_depth_step_config", "plnerf_depth_step_io", "plnerf_depth_step_args", "plnerf_depth_step_views")
ENTRIES = {"plnerf_depth_train_step_workspace_bytes", "plnerf_depth_train_step_layout", "plnerf_depth_train_step",
           "plnerf_depth_ss_adam"}
EINVAL, ERANGE, ENOSYS = -1, -3, -4      # PLNERF_E* of include/plnerf_hip.h


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_error_codes_are_the_headers():
    main = open(os.path.join(abi.INCLUDE, "plnerf_hip.h")).read()
    for name, want in (("PLNERF_EINVAL", EINVAL), ("PLNERF_ERANGE", ERANGE), ("PLNERF_ENOSYS", ENOSYS)):
        assert int(re.search(r"#define\s+" + name + r"\s+\(?(-?\d+)\)?", main).group(1)) == want


def test_struct_names_and_view_fields_are_the_headers(L):
    structs = abi.structs(HEADER)
    assert set(structs) == set(STRUCTS) == set(L.DEPTHSTEP_STRUCTS)
    # the layout query reports at least what a caller inspects after a step
    assert {"rgb", "rgb0", "depth", "depth0", "acc", "acc0", "disp", "disp0", "z_std", "pred_hyp", "z_vals", "z_vals0", "pixels",
            "target_h", "mask"} <= {f[1] for f in structs["plnerf_depth_step_views"]}


def test_library_exports_the_depth_step_entries(L):
    """Fails on a library built without csrc/depth_train_step.hip."""
    assert set(L.DEPTHSTEP_SIGNATURES) == ENTRIES <= abi.exported_symbols(L.LIB_PATH)


_C = r"""
#include <stdio.h>
#include <string.h>
#include "plnerf_hip_depthstep.h"

static plnerf_depth_step_config good_config(void) {
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

int main(int argc, char** argv) {
    size_t (*q)(const plnerf_depth_step_config*) = plnerf_depth_train_step_workspace_bytes;
    int (*lay)(const plnerf_depth_step_config*, plnerf_depth_step_views*) = plnerf_depth_train_step_layout;
    int (*p)(const plnerf_depth_step_config*, const plnerf_depth_step_io*, const plnerf_depth_step_args*, void*, size_t,
             plnerf_stream_t) = plnerf_depth_train_step;
    int (*ss)(float*, float*, const float*, float*, float*, int, float, float, float, float, int, float, plnerf_stream_t) =
        plnerf_depth_ss_adam;
    plnerf_depth_step_config c = good_config(), bad;
    plnerf_depth_step_io io;
    plnerf_depth_step_args a;
    plnerf_depth_step_views v;
    /* never dereferenced: every call below is refused by the argument checks, before any device work */
    static float host[PLNERF_N_PARAMS + 64];
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    size_t need;
    int i;
    if (argc > 1) {
        printf("%zu %zu %zu %zu\n", sizeof(plnerf_depth_step_config), sizeof(plnerf_depth_step_io),
               sizeof(plnerf_depth_step_args), sizeof(plnerf_depth_step_views));
        return 0;
    }
    if (plnerf_version() != PLNERF_VERSION) return 2;
    need = q(&c);
    if (need == 0 || need % 256 != 0 || q(NULL) != 0) return 3;
    if (lay(&c, &v) != PLNERF_OK || lay(&c, NULL) != PLNERF_EINVAL || lay(NULL, &v) != PLNERF_EINVAL) return 30;
    if (v.rgb % 256 || v.pixels % 256 || v.rgb >= need || v.pred_hyp >= need || v.z_vals0 >= v.z_vals || v.rgb == v.rgb0) return 31;
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + i; io.fine.params[i] = host + i; }
    io.coarse.param_flat = io.coarse.grad_flat = io.coarse.exp_avg = io.coarse.exp_avg_sq = host;
    io.coarse.n_params = PLNERF_N_PARAMS;
    io.coarse.packed = host;
    io.fine = io.coarse;
    io.t_vals = host; io.loss5 = host; io.images = host; io.hyp = host; io.poses = host; io.intrinsics = host;
    a.rays = 1024; a.view = 2; a.adam_step = 1; a.lr = 5e-4f; a.carve = 1;
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 4;                 /* null structs */
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return 5;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return 6;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return 7;
    a.rays = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 8;                   /* rays = 0 */
    a.rays = 1025;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 9;                   /* rays > max_rays */
    a.rays = 1024;
    a.view = 3;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 10;                  /* view = n_views */
    a.view = -1;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 11;
    a.view = 2;
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return 12;       /* a misaligned workspace */
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return 13;              /* ... or one byte short */
    bad = c; bad.n_importance = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL || q(&bad) != 0 || lay(&bad, &v) != PLNERF_EINVAL) return 14;
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS || q(&bad) != 0 || lay(&bad, &v) != PLNERF_ENOSYS) return 15;
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 16;                /* compiled limits */
    bad = c; bad.n_importance = 2147483647;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE || q(&bad) != 0) return 28; /* no signed overflow in S + N */
    a.ray_id0 = 480 * 640 - 1000;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return 17;                  /* ray_id0 + rays > H * W */
    a.ray_id0 = 0;
    io.fine.params[5] = host + PLNERF_N_PARAMS;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 18;                  /* a parameter outside its flat buffer */
    io.fine.params[5] = host + 5;
    io.loss5 = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 19;
    io.loss5 = host;
    io.hyp = NULL;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 20;
    io.hyp = host;
    bad = c; bad.perturb = 0;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 21;                /* det draws without u_vals */
    a.ss_step = 1; a.ss_adam_step = 1;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 22;                  /* stepping scales that are not there */
    io.scale = io.shift = io.ss_grad = io.ss_exp_avg = io.ss_exp_avg_sq = host;
    a.carve = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 23;                  /* ... or without the carving term */
    a.carve = 1; a.ss_step = 0;
    a.adam_step = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return 24;
    if (ss(NULL, host, host, host, host, 4, 1e-3f, 0.9f, 0.999f, 1e-8f, 1, 1.f, NULL) != PLNERF_EINVAL) return 25;
    if (ss(host, host, host, host, host, 0, 1e-3f, 0.9f, 0.999f, 1e-8f, 1, 1.f, NULL) != PLNERF_EINVAL) return 26;
    if (ss(host, host, host, host, host, 4, 1e-3f, 0.9f, 0.999f, 1e-8f, 0, 1.f, NULL) != PLNERF_EINVAL) return 27;
    printf("depth step abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("depth_step_abi"), "depth_step_abi")


def test_depth_step_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "depth step abi ok" in out.stdout


def test_structure_sizes_are_the_compilers(L, c_host):
    out = subprocess.run([c_host, "sizes"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    sizes = [int(x) for x in out.stdout.split()]
    assert sizes == [ctypes.sizeof(L.DEPTHSTEP_STRUCTS[n]) for n in STRUCTS]


def _good(L):
    return L.DepthStepConfig(max_rays=256, n_samples=64, n_importance=32, color_mode=L.COLOR["midpoint"], perturb=1, n_views=3,
                             H=24, W=32, n_hyp=3, pose_rows=4, near=2.0, far=6.0, precision=L.PRECISION["f16x3"], input_ch=57,
                             input_ch_views=3, input_scale=3.14159265, density_beta=10.0, space_carving_weight=0.007,
                             clip_value=0.1, beta1=0.9, beta2=0.999, adam_eps=1e-8, ss_beta1=0.9, ss_beta2=0.999,
                             ss_adam_eps=1e-8)


def test_ctypes_calls_are_refused_without_a_device(L):
    """The same checks through the binding: null structs, rays = 0 and > max_rays, view = n_views, a misaligned and a short
    workspace, n_importance = 0, a precision that is not built."""
    lib = L.lib()
    assert lib.plnerf_depth_train_step(None, None, None, None, 0, None) == EINVAL
    cfg = _good(L)
    nbytes = lib.plnerf_depth_train_step_workspace_bytes(ctypes.byref(cfg))
    assert nbytes > 256 * 96 * 4 * 4 and nbytes % L.STEP_WORKSPACE_ALIGN == 0
    layout = L.DepthStepViews()
    assert lib.plnerf_depth_train_step_layout(ctypes.byref(cfg), ctypes.byref(layout)) == 0
    offs = [getattr(layout, n) for n in L.DEPTH_STEP_VIEWS]
    assert len(set(offs)) == len(offs) and all(o % L.STEP_WORKSPACE_ALIGN == 0 and 0 < o < nbytes for o in offs)
    # (a host block standing in for device memory: every call below is refused before anything could read it)
    block = (ctypes.c_float * 1024)()
    host = ctypes.addressof(block)
    io = L.DepthStepIo()
    for net in (io.coarse, io.fine):
        for k in range(L.N_PARAM_TENSORS):
            net.params[k] = host + 4 * k
        net.param_flat = net.grad_flat = net.exp_avg = net.exp_avg_sq = net.packed = host
        net.n_params = 512
    io.t_vals = io.loss5 = io.images = io.hyp = io.poses = io.intrinsics = host
    ws = ctypes.c_void_p(1 << 20)

    def call(cfg, args, ws=ws, nbytes=nbytes):
        return lib.plnerf_depth_train_step(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(args), ws, nbytes, None)
    good = dict(view=1, rays=256, adam_step=1, lr=5e-4)
    assert call(cfg, L.DepthStepArgs(**dict(good, rays=0))) == EINVAL
    assert call(cfg, L.DepthStepArgs(**dict(good, rays=257))) == EINVAL
    assert call(cfg, L.DepthStepArgs(**dict(good, view=3))) == EINVAL
    assert call(cfg, L.DepthStepArgs(**good), ws=ctypes.c_void_p((1 << 20) + 4)) == EINVAL
    assert call(cfg, L.DepthStepArgs(**good), nbytes=nbytes - 1) == EINVAL
    assert call(cfg, L.DepthStepArgs(**dict(good, ray_id0=24 * 32 - 255))) == ERANGE
    bad = _good(L)
    bad.n_importance = 0
    assert call(bad, L.DepthStepArgs(**good)) == EINVAL and lib.plnerf_depth_train_step_workspace_bytes(ctypes.byref(bad)) == 0
    bad = _good(L)
    bad.precision = 17
    assert call(bad, L.DepthStepArgs(**good)) == ENOSYS and lib.plnerf_depth_train_step_workspace_bytes(ctypes.byref(bad)) == 0
    assert lib.plnerf_depth_ss_adam(None, None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None) == EINVAL
