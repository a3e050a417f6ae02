"""The experimental header include/experimental/plnerf_hip_dpstep.h, without a GPU, as tests/test_camcode_abi.py holds its
header: the one row of the fourth table _lib.DPSTEP_HEADERS against the header's prototypes and the library's exports, the
signatures argument by argument, what lib() bound, a guard-band case for every entry that takes a stream
(tests/dpstep_cases.py, run on the GPU by tests/test_gpu_one_call_dp.py), a C99 host with every refusal on fake pointers --
and that the three existing tables and the ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi
import containment as C
import dpstep_cases as cases

HEADER = "experimental/plnerf_hip_dpstep.h"
ENTRIES = {"plnerf_train_step_grads", "plnerf_train_step_const_grads", "plnerf_train_step_apply",
           "plnerf_depth_train_step_grads", "plnerf_depth_train_step_const_grads", "plnerf_depth_train_step_apply"}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
EXPERIMENTAL = ("experimental/plnerf_hip_depthview.h",)
CAMCODE = ("experimental/plnerf_hip_camcode.h",)
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.DPSTEP_HEADERS) == 1
    header, signatures, mirrors = L.DPSTEP_HEADERS[0]
    assert header == HEADER and mirrors == {}      # (the structs are the registered steps')
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def test_names_agree(L, row):
    path, signatures, _ = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert not abi.structs(path)


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type: a scalar is that ctypes type, a pointer to one of the
    registered ABI's structs is POINTER(its mirror), any other pointer and the stream are c_void_p."""
    path, signatures, _ = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params), (name, len(args), len(params))
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            t = abi.bare(c_type)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[t], (where, c_type, ct)
                continue
            pointee = t[:-1].strip() if t.endswith("*") else None
            if pointee in abi.abi_structs():
                assert ct is ctypes.POINTER(abi.abi_structs()[pointee]), (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The fourth table shares no name with the other three and adds nothing to them."""
    others = set(L.ALL_SIGNATURES) | set(L.EXPERIMENTAL_SIGNATURES) | set(L.CAMCODE_TABLE_SIGNATURES)
    assert not set(L.DPSTEP_TABLE_SIGNATURES) & others
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert tuple(header for header, _, _ in L.EXPERIMENTAL_HEADERS) == EXPERIMENTAL
    assert tuple(header for header, _, _ in L.CAMCODE_HEADERS) == CAMCODE
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES, L.CAMCODE_TABLE_SIGNATURES):
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)


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


_C = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "experimental/plnerf_hip_dpstep.h"

static plnerf_step_config nvs_config(int mode) {
    plnerf_step_config c;
    memset(&c, 0, sizeof c);
    c.max_rays = 1024; c.n_samples = 64; c.n_importance = 128; c.mode = mode; c.color_mode = PLNERF_COLOR_MIDPOINT;
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

/* never dereferenced: every call below is refused by the argument checks, before any device work */
static float host[PLNERF_N_PARAMS + 64];

typedef int (*nvs_grads_fn)(const plnerf_step_config*, const plnerf_step_io*, const plnerf_step_args*, void*, size_t,
                            plnerf_stream_t);

static int nvs_grads(nvs_grads_fn p, int mode, size_t need, int base) {
    plnerf_step_config c = nvs_config(mode), bad;
    plnerf_step_io io;
    plnerf_step_args a;
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    int i;
    if (need == 0) return base;
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + i; }
    io.coarse.param_flat = io.coarse.grad_flat = io.coarse.exp_avg = io.coarse.exp_avg_sq = host;
    io.coarse.n_params = PLNERF_N_PARAMS;
    io.coarse.packed = host;
    io.fine = io.coarse;
    io.t_vals = host; io.loss4 = host;
    a.rays = 1024; a.image = host; a.crop_rows = 400; a.crop_cols = 400; a.loss_scale = 1.f;      /* (no Adam step counts) */
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 1;               /* null structs */
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 2;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return base + 3;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return base + 4;               /* null workspace */
    a.rays = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 5;
    a.rays = 1025;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 6;
    a.rays = 1024;
    bad = c; bad.mode = mode == PLNERF_MODE_LINEAR ? PLNERF_MODE_CONSTANT : PLNERF_MODE_LINEAR;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 7;               /* the sibling's mode */
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS) return base + 8;
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return base + 9;
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return base + 10;            /* workspace too small */
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return base + 11;     /* ... or misaligned */
    a.ray_id0 = 400 * 400 - 1023;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return base + 12;                /* a shard past the view's pixels */
    a.ray_id0 = 0;
    io.fine.params[5] = host + PLNERF_N_PARAMS;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 13;                /* a parameter outside its flat buffer */
    return 0;
}

static int nvs_apply(void) {
    plnerf_step_config c = nvs_config(PLNERF_MODE_LINEAR), bad;
    plnerf_step_io io;
    plnerf_step_args a;
    int i;
    memset(&io, 0, sizeof io);
    memset(&a, 0, sizeof a);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io.coarse.params[i] = host + i; }
    io.coarse.param_flat = io.coarse.grad_flat = io.coarse.exp_avg = io.coarse.exp_avg_sq = host;
    io.coarse.n_params = PLNERF_N_PARAMS;
    io.coarse.packed = host;
    io.fine = io.coarse;
    a.adam_step_fine = 1; a.adam_step_coarse = 1; a.lr_fine = a.lr_coarse = 5e-4f;
    if (plnerf_train_step_apply(NULL, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 61;    /* null structs */
    if (plnerf_train_step_apply(&c, NULL, &a, 0.5f, NULL) != PLNERF_EINVAL) return 62;
    if (plnerf_train_step_apply(&c, &io, NULL, 0.5f, NULL) != PLNERF_EINVAL) return 63;
    if (plnerf_train_step_apply(&c, &io, &a, 0.f, NULL) != PLNERF_EINVAL) return 64;       /* grad_scale */
    if (plnerf_train_step_apply(&c, &io, &a, -0.5f, NULL) != PLNERF_EINVAL) return 65;
    if (plnerf_train_step_apply(&c, &io, &a, INFINITY, NULL) != PLNERF_EINVAL) return 66;
    if (plnerf_train_step_apply(&c, &io, &a, NAN, NULL) != PLNERF_EINVAL) return 67;
    a.adam_step_fine = 0;
    if (plnerf_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 68;      /* Adam step counts */
    a.adam_step_fine = 1; a.adam_step_coarse = 0;
    if (plnerf_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 69;
    a.adam_step_coarse = 1;
    bad = nvs_config(PLNERF_MODE_CONSTANT);                                              /* (serves both modes) */
    io.coarse.exp_avg = NULL;
    if (plnerf_train_step_apply(&bad, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 70;    /* a net check_net refuses */
    io.coarse.exp_avg = host;
    io.fine.n_params = 0;
    if (plnerf_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 71;
    return 0;
}

typedef int (*depth_grads_fn)(const plnerf_depth_step_config*, const plnerf_depth_step_io*, const plnerf_depth_step_args*,
                              void*, size_t, plnerf_stream_t);

static void depth_io(plnerf_depth_step_io* io) {
    int i;
    memset(io, 0, sizeof *io);
    for (i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) { io->coarse.params[i] = host + i; }
    io->coarse.param_flat = io->coarse.grad_flat = io->coarse.exp_avg = io->coarse.exp_avg_sq = host;
    io->coarse.n_params = PLNERF_N_PARAMS;
    io->coarse.packed = host;
    io->fine = io->coarse;
    io->t_vals = host; io->loss5 = host; io->images = host; io->hyp = host; io->poses = host; io->intrinsics = host;
}

static int depth_grads(depth_grads_fn p, size_t need, int base) {
    plnerf_depth_step_config c = depth_config(), bad;
    plnerf_depth_step_io io;
    plnerf_depth_step_args a;
    void* ws = (void*)(((uintptr_t)host + 255) / 256 * 256);
    if (need == 0) return base;
    depth_io(&io);
    memset(&a, 0, sizeof a);
    a.rays = 1024; a.view = 2; a.lr = 5e-4f; a.carve = 1;                                  /* (no Adam step count) */
    if (p(NULL, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 1;
    if (p(&c, NULL, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 2;
    if (p(&c, &io, NULL, ws, need, NULL) != PLNERF_EINVAL) return base + 3;
    if (p(&c, &io, &a, NULL, need, NULL) != PLNERF_EINVAL) return base + 4;
    a.rays = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 5;
    a.rays = 1024; a.view = 3;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 6;
    a.view = 2;
    bad = c; bad.precision = 17;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ENOSYS) return base + 7;
    bad = c; bad.n_samples = 600; bad.n_importance = 600;
    if (p(&bad, &io, &a, ws, need, NULL) != PLNERF_ERANGE) return base + 8;
    if (p(&c, &io, &a, ws, need - 1, NULL) != PLNERF_EINVAL) return base + 9;
    if (p(&c, &io, &a, (char*)ws + 4, need, NULL) != PLNERF_EINVAL) return base + 10;
    a.ss_step = 1;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 11;                /* ss_step without ss_grad */
    io.scale = io.shift = io.ss_grad = host;
    a.carve = 0;
    if (p(&c, &io, &a, ws, need, NULL) != PLNERF_EINVAL) return base + 12;                /* ss_step without carve */
    return 0;
}

static int depth_apply(void) {
    plnerf_depth_step_config c = depth_config();
    plnerf_depth_step_io io;
    plnerf_depth_step_args a;
    depth_io(&io);
    memset(&a, 0, sizeof a);
    a.adam_step = 1; a.lr = 5e-4f;
    if (plnerf_depth_train_step_apply(NULL, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 81;
    if (plnerf_depth_train_step_apply(&c, NULL, &a, 0.5f, NULL) != PLNERF_EINVAL) return 82;
    if (plnerf_depth_train_step_apply(&c, &io, NULL, 0.5f, NULL) != PLNERF_EINVAL) return 83;
    if (plnerf_depth_train_step_apply(&c, &io, &a, 0.f, NULL) != PLNERF_EINVAL) return 84;
    if (plnerf_depth_train_step_apply(&c, &io, &a, -1.f, NULL) != PLNERF_EINVAL) return 85;
    if (plnerf_depth_train_step_apply(&c, &io, &a, INFINITY, NULL) != PLNERF_EINVAL) return 86;
    if (plnerf_depth_train_step_apply(&c, &io, &a, NAN, NULL) != PLNERF_EINVAL) return 87;
    a.adam_step = 0;
    if (plnerf_depth_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 88;
    a.adam_step = 1;
    a.ss_step = 1; a.ss_adam_step = 0;
    io.scale = io.shift = io.ss_grad = io.ss_exp_avg = io.ss_exp_avg_sq = host;
    if (plnerf_depth_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 89; /* the scales' step count */
    a.ss_adam_step = 1; io.ss_exp_avg = NULL;
    if (plnerf_depth_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 90;
    io.ss_exp_avg = host; a.ss_step = 0;
    io.fine.packed = NULL;
    if (plnerf_depth_train_step_apply(&c, &io, &a, 0.5f, NULL) != PLNERF_EINVAL) return 91; /* a net check_net refuses */
    return 0;
}

int main(void) {
    plnerf_step_config lin = nvs_config(PLNERF_MODE_LINEAR), con = nvs_config(PLNERF_MODE_CONSTANT);
    plnerf_depth_step_config d = depth_config();
    int rc;
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    /* the workspace is the one-call step's: its size queries answer for the halves */
    if ((rc = nvs_grads(plnerf_train_step_grads, PLNERF_MODE_LINEAR, plnerf_train_step_workspace_bytes(&lin), 10))) return rc;
    if ((rc = nvs_grads(plnerf_train_step_const_grads, PLNERF_MODE_CONSTANT, plnerf_train_step_const_workspace_bytes(&con), 30)))
        return rc;
    if ((rc = nvs_apply())) return rc;
    if ((rc = depth_grads(plnerf_depth_train_step_grads, plnerf_depth_train_step_workspace_bytes(&d), 100))) return rc;
    if ((rc = depth_grads(plnerf_depth_train_step_const_grads, plnerf_depth_train_step_const_workspace_bytes(&d), 120))) return rc;
    if ((rc = depth_apply())) return rc;
    printf("dpstep abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("dpstep_abi"), "dpstep_abi")


def test_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "dpstep abi ok" in out.stdout


def _nets(io):
    host = (ctypes.c_float * 64)()
    base = ctypes.addressof(host)
    for net in (io.coarse, io.fine):
        for k in range(len(net.params)):
            net.params[k] = base + 4 * k
        net.param_flat = net.grad_flat = net.exp_avg = net.exp_avg_sq = net.packed = base
        net.n_params = 64
    return host


@pytest.mark.parametrize("grad_scale", [0.0, -0.25, float("inf"), float("-inf"), float("nan")])
def test_apply_refuses_a_grad_scale_that_is_not_finite_and_positive(L, grad_scale):
    """Through the binding, without a device: the refusal comes before any launch (a launch here would be PLNERF_ELAUNCH)."""
    lib = L.lib()
    cfg = L.StepConfig(max_rays=256, n_samples=64, n_importance=128, mode=L.MODE["linear"], precision=L.PRECISION["f16x3"],
                       H=8, W=8, input_ch=63, input_ch_views=27)
    io, a = L.StepIo(), L.StepArgs(adam_step_fine=1, adam_step_coarse=1)
    keep = _nets(io)
    assert lib.plnerf_train_step_apply(ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(a), grad_scale, None) == EINVAL
    d = L.DepthStepConfig(max_rays=256, n_samples=64, n_importance=128, precision=L.PRECISION["f16x3"], n_views=2, H=8, W=8,
                          n_hyp=3, pose_rows=4, input_ch=57, input_ch_views=3, input_scale=1.0)
    dio, da = L.DepthStepIo(), L.DepthStepArgs(adam_step=1)
    keep2 = _nets(dio)
    assert lib.plnerf_depth_train_step_apply(ctypes.byref(d), ctypes.byref(dio), ctypes.byref(da), grad_scale, None) == EINVAL
    del keep, keep2


def test_ctypes_calls_are_refused_without_a_device(L):
    """Null structs and Adam step counts of 0, through the binding."""
    lib = L.lib()
    cfg = L.StepConfig(max_rays=256, n_samples=64, n_importance=128, mode=L.MODE["linear"], precision=L.PRECISION["f16x3"],
                       H=8, W=8, input_ch=63, input_ch_views=27)
    io, a = L.StepIo(), L.StepArgs(adam_step_fine=1, adam_step_coarse=1)
    keep = _nets(io)
    c, i, s = ctypes.byref(cfg), ctypes.byref(io), ctypes.byref(a)
    for args in ((None, i, s), (c, None, s), (c, i, None)):
        assert lib.plnerf_train_step_apply(*args, 0.5, None) == EINVAL
        assert lib.plnerf_train_step_grads(*args, ctypes.c_void_p(256), 1 << 30, None) == EINVAL
        assert lib.plnerf_train_step_const_grads(*args, ctypes.c_void_p(256), 1 << 30, None) == EINVAL
    for fine, coarse in ((0, 1), (1, 0), (-3, 1)):
        a.adam_step_fine, a.adam_step_coarse = fine, coarse
        assert lib.plnerf_train_step_apply(c, i, s, 0.5, None) == EINVAL
    d = L.DepthStepConfig(max_rays=256, n_samples=64, n_importance=128, precision=L.PRECISION["f16x3"], n_views=2, H=8, W=8,
                          n_hyp=3, pose_rows=4, input_ch=57, input_ch_views=3, input_scale=1.0)
    dio, da = L.DepthStepIo(), L.DepthStepArgs(adam_step=1)
    keep2 = _nets(dio)
    c, i, s = ctypes.byref(d), ctypes.byref(dio), ctypes.byref(da)
    for args in ((None, i, s), (c, None, s), (c, i, None)):
        assert lib.plnerf_depth_train_step_apply(*args, 0.5, None) == EINVAL
        assert lib.plnerf_depth_train_step_grads(*args, ctypes.c_void_p(256), 1 << 30, None) == EINVAL
        assert lib.plnerf_depth_train_step_const_grads(*args, ctypes.c_void_p(256), 1 << 30, None) == EINVAL
    da.adam_step = 0
    assert lib.plnerf_depth_train_step_apply(c, i, s, 0.5, None) == EINVAL
    da.adam_step, da.ss_step, da.ss_adam_step = 1, 1, 0
    assert lib.plnerf_depth_train_step_apply(c, i, s, 0.5, None) == EINVAL
    del keep, keep2


def test_the_switch_and_the_plan_halves_exist(L):
    """The host side: the module switch defaults to on; both plans have the two halves beside run()."""
    from plnerf_amd import dp, stepplan, train
    assert train.ONE_CALL_DP is True
    for plan in (stepplan.StepPlan, stepplan.DepthStepPlan):
        assert callable(plan.run) and callable(plan.run_grads) and callable(plan.apply)
        assert plan.ENTRY + "_grads" in L.DPSTEP_TABLE_SIGNATURES and plan.ENTRY_CONST + "_grads" in L.DPSTEP_TABLE_SIGNATURES
        assert plan.ENTRY + "_apply" in L.DPSTEP_TABLE_SIGNATURES
    assert callable(dp.GradientBucket.reduce_block)
