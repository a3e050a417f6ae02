"""The experimental header include/experimental/plnerf_hip_camcode.h, without a GPU, as tests/test_depthview_abi.py holds its
header: the one row of the third table _lib.CAMCODE_HEADERS against the header's prototypes and the library's exports, the
signatures argument by argument, the state struct's mirror field by field, what lib() bound, a guard-band case for every
entry that takes a stream (tests/camcode_cases.py, run on the GPU by tests/test_gpu_camcode.py), a C99 host with the struct's
size and every refusal on fake pointers -- and that the two existing tables and the ABI version are what they were."""
import ctypes
import os
import subprocess

import pytest

import abi_support as abi
import camcode_cases as cases
import containment as C

HEADER = "experimental/plnerf_hip_camcode.h"
STRUCTS = ("plnerf_camcode_state",)
ENTRIES = {"plnerf_camcode_sweep_workspace_bytes", "plnerf_camcode_sweep", "plnerf_camcode_update"}
REGISTERED = ("plnerf_hip.h", "plnerf_hip_batching.h", "plnerf_hip_eval.h", "plnerf_hip_depthfeed.h", "plnerf_hip_sampleerr.h",
              "plnerf_hip_constepi.h", "plnerf_hip_step.h", "plnerf_hip_depthstep.h", "plnerf_hip_conststep.h", "plnerf_hip_view.h")
EXPERIMENTAL = ("experimental/plnerf_hip_depthview.h",)
EINVAL, ERANGE = -1, -3


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


@pytest.fixture(scope="module")
def row(L):
    assert len(L.CAMCODE_HEADERS) == 1
    header, signatures, mirrors = L.CAMCODE_HEADERS[0]
    assert header == HEADER
    return os.path.join(abi.INCLUDE, header), signatures, mirrors


def test_names_agree(L, row):
    path, signatures, mirrors = row
    declared = set(abi.prototypes(path))
    assert declared == set(signatures) == ENTRIES
    assert declared <= abi.exported_symbols(L.LIB_PATH), declared - abi.exported_symbols(L.LIB_PATH)
    assert set(mirrors) == set(STRUCTS) == set(abi.structs(path))


def test_signatures_agree(L, row):
    """tests/test_abi_headers.py's rule per return and argument type.  The state struct lives in DEVICE memory, so a pointer
    to it is a device pointer like any other (c_void_p), not a ctypes pointer to the mirror."""
    path, signatures, mirrors = row
    for name, (ret, params) in abi.prototypes(path).items():
        res, args = signatures[name]
        assert len(args) == len(params), (name, len(args), len(params))
        for where, c_type, ct in [((name, "return"), ret, res)] + [((name, k), p, a) for k, (p, a) in enumerate(zip(params, args))]:
            assert abi.ct_class(ct) == abi.c_class(c_type), (where, c_type, ct)
            t = abi.bare(c_type)
            if abi.c_class(c_type) != "ptr":
                assert ct is abi.SCALARS[t], (where, c_type, ct)
            else:
                assert ct is ctypes.c_void_p, (where, c_type, ct)      # device pointers and the stream


def test_struct_mirror_agrees(L, row):
    path, _, mirrors = row
    for name, fields in abi.structs(path).items():
        mirror = mirrors[name]._fields_
        assert [f[0] for f in mirror] == [f[1] for f in fields], name
        for (fname, ftype), (c_type, _, length) in zip(mirror, fields):
            want = abi.expected_ctype(c_type)
            if length is None:
                assert ftype is want, (name, fname, ftype, want)
            else:
                assert ftype._type_ is want and ftype._length_ == int(length), (name, fname)
    assert L.CamcodeState.cam.offset == 0      # plnerf_camcode_sweep's `cam` may point at the state


def test_binding_agrees(L, row):
    for name, (res, args) in row[1].items():
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


def test_the_other_tables_are_what_they_were(L):
    """The third table shares no name with the other two and adds nothing to them."""
    assert not set(L.CAMCODE_TABLE_SIGNATURES) & (set(L.ALL_SIGNATURES) | set(L.EXPERIMENTAL_SIGNATURES))
    assert tuple(header for header, _, _ in L.HEADERS) == REGISTERED
    assert tuple(header for header, _, _ in L.EXPERIMENTAL_HEADERS) == EXPERIMENTAL
    assert set(L.ALL_SIGNATURES) == set().union(*[signatures for _, signatures, _ in L.HEADERS])
    assert L.ABI_VERSION == 601 == L.lib().plnerf_version()
    for table in (L.ALL_SIGNATURES, L.EXPERIMENTAL_SIGNATURES):
        with pytest.raises(ValueError, match="one entry point, one header"):
            L._disjoint({next(iter(table)): None}, table)
    header = open(os.path.join(abi.INCLUDE, HEADER)).read()
    for name, value in (("MAX_WIDTH", L.CAMCODE_MAX_WIDTH), ("MAX_CAM", L.CAMCODE_MAX_CAM), ("MAX_ROWS", L.CAMCODE_MAX_ROWS),
                        ("MAX_GROUPS", L.CAMCODE_MAX_GROUPS)):
        assert f"#define PLNERF_CAMCODE_{name} {value} " in header, name


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
#include <stdio.h>
#include <string.h>
#include "experimental/plnerf_hip_camcode.h"

int main(int argc, char** argv) {
    /* never dereferenced: every call below is refused by the argument checks, before any device work */
    static double host8[1024];
    float* f = (float*)host8;
    double* d = host8;
    void* ws = (void*)(((uintptr_t)host8 + 255) / 256 * 256);
    plnerf_camcode_state* st = (plnerf_camcode_state*)host8;
    size_t need = plnerf_camcode_sweep_workspace_bytes(37);
    if (argc > 1) {
        printf("%zu\n", sizeof(plnerf_camcode_state));
        return 0;
    }
    if (plnerf_version() != PLNERF_VERSION) return 2;
    if (need == 0 || need % 256 != 0 || plnerf_camcode_sweep_workspace_bytes(0) != 0 ||
        plnerf_camcode_sweep_workspace_bytes(-3) != 0) return 3;
    if (plnerf_camcode_sweep_workspace_bytes(1) == 0 || plnerf_camcode_sweep_workspace_bytes(1 << 30) < need) return 4;
#define SWEEP(A, coef, n_rows, rpr, width, cam, n_cam, w_cam, stride, w_rgb, b_rgb, target, bkgd, lam, ws, bytes, loss, g) \
    plnerf_camcode_sweep(A, coef, n_rows, rpr, width, cam, n_cam, w_cam, stride, w_rgb, b_rgb, target, bkgd, lam, ws, bytes, loss, g, NULL)
    if (SWEEP(NULL, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 10;
    if (SWEEP(f, NULL, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 11;
    if (SWEEP(f, f, 74, 2, 64, NULL, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 12;
    if (SWEEP(f, f, 74, 2, 64, f, 4, NULL, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 13;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, NULL, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 14;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, NULL, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 15;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, NULL, f, f, ws, need, d, f) != PLNERF_EINVAL) return 16;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, NULL, ws, need, d, f) != PLNERF_EINVAL) return 17;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, NULL, need, d, f) != PLNERF_EINVAL) return 18;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, NULL, f) != PLNERF_EINVAL) return 19;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, NULL) != PLNERF_EINVAL) return 20;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need - 1, d, f) != PLNERF_EINVAL) return 21;   /* too small */
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, (char*)ws + 4, need, d, f) != PLNERF_EINVAL) return 22;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, (double*)((char*)d + 4), f) != PLNERF_EINVAL) return 23;
    if (SWEEP(f, f, 74, 2, 0, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 24;        /* width */
    if (SWEEP(f, f, 74, 2, 129, f, 4, f, 140, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 25;
    if (SWEEP(f, f, 74, 2, 64, f, 0, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 26;       /* n_cam */
    if (SWEEP(f, f, 74, 2, 64, f, 33, f, 120, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 27;
    if (SWEEP(f, f, 74, 0, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 28;       /* rows_per_ray */
    if (SWEEP(f, f, 2050, 1025, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 29;
    if (SWEEP(f, f, 75, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 30;       /* not a multiple */
    if (SWEEP(f, f, -2, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 31;
    if (SWEEP(f, f, 74, 2, 64, f, 4, f, 3, f, f, f, f, f, ws, need, d, f) != PLNERF_EINVAL) return 32;        /* stride < n_cam */
    if (SWEEP(f, f, (1 << 30) + 2, 2, 64, f, 4, f, 71, f, f, f, f, f, ws, need, d, f) != PLNERF_ERANGE) return 33;
    if (SWEEP(NULL, NULL, 0, 2, 64, NULL, 4, NULL, 71, NULL, NULL, NULL, NULL, NULL, NULL, 0, d, f) != PLNERF_OK) return 34;

#define UPDATE(st, n_cam, loss, g, nb, b1, b2, eps, factor, patience, ph, lh, nh) \
    plnerf_camcode_update(st, n_cam, loss, g, nb, b1, b2, eps, factor, patience, ph, lh, nh, NULL)
    if (UPDATE(NULL, 4, d, f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 40;
    if (UPDATE(st, 4, NULL, f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 41;
    if (UPDATE(st, 4, d, NULL, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 42;
    if (UPDATE(st, 0, d, f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 43;
    if (UPDATE(st, 33, d, f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 44;
    if (UPDATE(st, 4, d, f, 0, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 45;
    if (UPDATE(st, 4, d, f, 2, 1.f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 46;
    if (UPDATE(st, 4, d, f, 2, .9f, -.1f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 47;
    if (UPDATE(st, 4, d, f, 2, .9f, .999f, -1.f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 48;
    if (UPDATE(st, 4, d, f, 2, .9f, .999f, 1e-8f, 1.f, 3, f, f, 100) != PLNERF_EINVAL) return 49;
    if (UPDATE(st, 4, d, f, 2, .9f, .999f, 1e-8f, 0.f, 3, f, f, 100) != PLNERF_EINVAL) return 50;
    if (UPDATE(st, 4, d, f, 2, .9f, .999f, 1e-8f, .5f, -1, f, f, 100) != PLNERF_EINVAL) return 51;
    if (UPDATE(st, 4, d, f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, -1) != PLNERF_EINVAL) return 52;
    if (UPDATE((plnerf_camcode_state*)((char*)st + 2), 4, d, f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 53;
    if (UPDATE(st, 4, (double*)((char*)d + 4), f, 2, .9f, .999f, 1e-8f, .5f, 3, f, f, 100) != PLNERF_EINVAL) return 54;
    printf("camcode abi ok\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_host(L, tmp_path_factory):
    return abi.compile_c(_C, tmp_path_factory.mktemp("camcode_abi"), "camcode_abi")


def test_header_is_plain_c_and_the_checks_come_first(c_host):
    out = subprocess.run([c_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "camcode abi ok" in out.stdout


def test_structure_size_is_the_compilers(L, c_host):
    out = subprocess.run([c_host, "sizes"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert [int(x) for x in out.stdout.split()] == [ctypes.sizeof(L.CAMCODE_STRUCTS[n]) for n in STRUCTS]


def test_ctypes_calls_are_refused_without_a_device(L):
    """The same checks through the binding."""
    lib = L.lib()
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(1024)
    need = lib.plnerf_camcode_sweep_workspace_bytes(5)
    assert need > 0 and need % L.STEP_WORKSPACE_ALIGN == 0 and lib.plnerf_camcode_sweep_workspace_bytes(0) == 0
    good = [p, p, 10, 2, 64, p, 4, p, 71, p, p, p, None, p, q, need, p, p, None]
    for k, bad in ((0, None), (2, 11), (3, 1025), (4, 129), (6, 33), (8, 3), (14, ctypes.c_void_p(260)), (15, need - 1),
                   (16, ctypes.c_void_p(260)), (17, None)):
        args = list(good)
        args[k] = bad
        assert lib.plnerf_camcode_sweep(*args) == EINVAL, k
    args = list(good)
    args[2] = (1 << 30) + 2
    assert lib.plnerf_camcode_sweep(*args) == ERANGE
    args[2] = 0
    assert lib.plnerf_camcode_sweep(*args) == 0      # zero rays: OK, nothing launched
    assert lib.plnerf_camcode_update(None, 4, p, p, 2, 0.9, 0.999, 1e-8, 0.5, 3, None, None, 0, None) == EINVAL
    assert lib.plnerf_camcode_update(p, 4, p, p, 2, 0.9, 0.999, 1e-8, 1.5, 3, None, None, 0, None) == EINVAL


def test_unsupported_configurations_have_a_reason(L):
    """Without a GPU nothing is served by the cached route; the reasons come before any device work."""
    from plnerf_amd import camcode
    import plnerf_amd
    assert plnerf_amd.optimize_camera_embedding is camcode.optimize_camera_embedding
    assert plnerf_amd.CameraCodeOptimizer is camcode.CameraCodeOptimizer
    assert camcode.CameraCodeOptimizer.unsupported_reason({}) is not None
    net = plnerf_amd.NeRF(D=8, W=256, input_ch=57, input_ch_views=3, input_ch_cam=4, use_viewdirs=True)
    kw = dict(network_fn=net, network_fine=net, use_viewdirs=True, perturb=0., raw_noise_std=0., mode="linear",
              color_mode="midpoint", N_samples=8, N_importance=8)
    assert "GPU" in camcode.CameraCodeOptimizer.unsupported_reason(kw)
    with pytest.raises(NotImplementedError, match="does not serve"):
        camcode.CameraCodeOptimizer(kw, 4, 6, None)
    with pytest.raises(ValueError, match="route"):
        camcode.optimize_camera_embedding(None, None, 4, 6, None, None, kw, route="quick")
