"""Piecewise-constant mode's one-launch stages without a GPU: the C ABI of include/plnerf_hip_constepi.h (plain C99, links
against the library, both symbols exported; the signatures themselves are compared in tests/test_abi_headers.py) and every
refusal of its table, which is decided before anything touches a device: the calls below carry NULL device pointers and run
on a machine without one."""
import ctypes
import os
import subprocess
import sys

import pytest

import abi_support as abi

HEADER = os.path.join(abi.INCLUDE, "plnerf_hip_constepi.h")
NAMES = {"plnerf_coarse_epilogue_const", "plnerf_fine_epilogue_const"}
OK, EINVAL, ERANGE = 0, -1, -3
MAX_SAMPLES = 1022      # PLNERF_MAX_SAMPLES


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


def test_constepi_names_and_argument_counts_match_the_header(L):
    protos = abi.prototypes(HEADER)
    assert set(protos) == set(L.CONSTEPI_SIGNATURES) == NAMES
    assert len(protos["plnerf_coarse_epilogue_const"][1]) == 25 and len(protos["plnerf_fine_epilogue_const"][1]) == 26
    # the main header and its restatement are what they were: the new entries live in the companion header only
    main = open(os.path.join(abi.INCLUDE, "plnerf_hip.h")).read()
    assert "_epilogue_const" not in main and "_epilogue_const" not in open(os.path.join(abi.ROOT, "tests", "abi_check.c")).read()


def test_both_symbols_are_exported_and_bound(L):
    assert NAMES <= abi.exported_symbols(L.LIB_PATH)
    for name in NAMES:
        fn = getattr(L.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L.CONSTEPI_SIGNATURES[name][1]


_P = ctypes.c_void_p(64)      # a non-NULL "device pointer": no refused call reads it


def _coarse(L, R=4, S=8, N=4, u=None, stride=0, **null):
    names = ("raw", "z", "near", "far", "rays_o", "rays_d")
    outs = ("rgb_map", "disp_map", "acc_map", "depth_map", "weights", "z_fine", "pts", "z_std")
    ptr = lambda k: None if null.get(k) else _P
    return L.lib().plnerf_coarse_epilogue_const(*[ptr(k) for k in names], None, u, stride, 0, 0, 0, R, S, N, 0,
                                                *[ptr(k) for k in outs], None)


def _fine(L, R=4, S=8, N=4, u=None, stride=0, **null):
    names = ("raw", "z", "near", "far", "rays_d")
    outs = ("rgb_map", "disp_map", "acc_map", "depth_map", "weights", "bins_out", "samples", "inds", "u_out", "z_std")
    ptr = lambda k: None if null.get(k) else _P
    return L.lib().plnerf_fine_epilogue_const(*[ptr(k) for k in names], None, u, stride, 0, 0, 0, R, S, N, 0,
                                              *[ptr(k) for k in outs], None)


@pytest.mark.parametrize("call", [_coarse, _fine], ids=["coarse", "final"])
def test_sizes_are_refused_before_any_device_work(L, call):
    # PLNERF_EINVAL: R < 0, S < 3, N < 1 (with every pointer NULL: the sizes are looked at first)
    every = dict.fromkeys(("raw", "z", "near", "far", "rays_o", "rays_d", "rgb_map", "disp_map", "acc_map", "depth_map",
                           "weights", "bins_out", "z_fine", "pts", "samples", "inds", "u_out", "z_std"), True)
    assert call(L, R=-1, **every) == EINVAL
    for S in (-1, 0, 1, 2):
        assert call(L, S=S, **every) == EINVAL, S
    assert call(L, N=0, **every) == EINVAL and call(L, N=-3, **every) == EINVAL
    # u given with a stride other than 0 or N
    assert call(L, N=4, u=_P, stride=3, **every) == EINVAL and call(L, N=4, u=_P, stride=-4, **every) == EINVAL
    # PLNERF_ERANGE: the compiled limits, again before the pointers
    assert call(L, S=MAX_SAMPLES + 1, N=1, **every) == ERANGE
    # R == 0: PLNERF_OK with nothing launched (no device here: a launch would fail), whatever the pointers
    assert call(L, R=0, **every) == OK
    assert call(L, R=0, S=3, N=1, u=_P, stride=1) == OK
    # the smallest sizes are sizes: with R == 0 they pass every check
    assert call(L, R=0, S=3, N=1, **every) == OK and call(L, R=0, S=MAX_SAMPLES, N=2, **every) == OK


def test_row_limits_differ_between_the_two_entries(L):
    # coarse: the merged row S + N <= 1024; final: the samples N <= 1024 on their own
    assert _coarse(L, R=0, S=512, N=512) == OK and _coarse(L, R=0, S=512, N=513) == ERANGE
    assert _coarse(L, R=0, S=3, N=1021) == OK and _coarse(L, R=0, S=3, N=1022) == ERANGE
    assert _fine(L, R=0, S=512, N=1024) == OK and _fine(L, R=0, S=512, N=1025) == ERANGE
    assert _fine(L, R=0, S=MAX_SAMPLES, N=1024) == OK      # (the largest row: 4 x 8186 floats, inside the 160 KB of LDS)


@pytest.mark.parametrize("missing", ["raw", "z", "near", "far", "rays_o", "rays_d", "rgb_map", "disp_map", "acc_map",
                                     "depth_map", "z_fine", "pts", "z_std"])
def test_coarse_required_pointers(L, missing):
    assert _coarse(L, **{missing: True}) == EINVAL


@pytest.mark.parametrize("missing", ["raw", "z", "near", "far", "rays_d", "rgb_map", "disp_map", "acc_map", "depth_map",
                                     "weights", "samples", "inds", "z_std"])
def test_final_required_pointers(L, missing):
    assert _fine(L, **{missing: True}) == EINVAL


_C = r"""
#include <stdio.h>
#include "plnerf_hip_constepi.h"

int main(void) {
    int (*c)(const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*,
             int, uint64_t, uint32_t, int, int, int, int, int, float*, float*, float*, float*, float*, float*, float*, float*,
             plnerf_stream_t) = plnerf_coarse_epilogue_const;
    int (*f)(const float*, const float*, const float*, const float*, const float*, const float*, const float*, int, uint64_t,
             uint32_t, int, int, int, int, int, float*, float*, float*, float*, float*, float*, float*, int64_t*, float*,
             float*, plnerf_stream_t) = plnerf_fine_epilogue_const;
    float x[4] = {0};
    int64_t i[4] = {0};
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION != 601) return 2;
    /* validation before any device work: these calls never touch the (absent) GPU */
    if (c(x, x, x, x, x, x, NULL, NULL, 0, 0, 0, 0, 4, 2, 4, 0, x, x, x, x, NULL, x, x, x, NULL) != PLNERF_EINVAL) return 3;
    if (f(x, x, x, x, x, NULL, NULL, 0, 0, 0, 0, 4, 2, 4, 0, x, x, x, x, x, NULL, x, i, NULL, x, NULL) != PLNERF_EINVAL) return 4;
    if (c(x, x, x, x, x, x, NULL, x, 3, 0, 0, 0, 4, 8, 4, 0, x, x, x, x, NULL, x, x, x, NULL) != PLNERF_EINVAL) return 5;
    if (f(x, x, x, x, x, NULL, x, 3, 0, 0, 0, 4, 8, 4, 0, x, x, x, x, x, NULL, x, i, NULL, x, NULL) != PLNERF_EINVAL) return 6;
    if (c(x, x, x, x, x, x, NULL, NULL, 0, 0, 0, 0, 4, 8, 1017, 0, x, x, x, x, NULL, x, x, x, NULL) != PLNERF_ERANGE) return 7;
    if (f(x, x, x, x, x, NULL, NULL, 0, 0, 0, 0, 4, 8, 1025, 0, x, x, x, x, x, NULL, x, i, NULL, x, NULL) != PLNERF_ERANGE) return 8;
    if (c(x, x, x, x, x, x, NULL, NULL, 0, 0, 0, 0, 4, PLNERF_MAX_SAMPLES + 1, 1, 0, x, x, x, x, NULL, x, x, x, NULL) !=
        PLNERF_ERANGE) return 9;
    if (f(x, x, x, x, x, NULL, NULL, 0, 0, 0, 0, 4, 8, 4, 0, x, x, x, x, NULL, NULL, x, i, NULL, x, NULL) != PLNERF_EINVAL)
        return 10;                                                      /* weights are required by the final stage */
    if (c(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, 0, 64, 128, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
          NULL, NULL) != PLNERF_OK) return 11;                          /* R = 0: nothing to launch */
    if (f(NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, 0, 64, 128, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
          NULL, NULL, NULL) != PLNERF_OK) return 12;
    printf("constepi abi ok\n");
    return 0;
}
"""


def test_constepi_header_is_plain_c_and_links(L, tmp_path):
    out = subprocess.run([abi.compile_c(_C, tmp_path, "constepi_abi")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "constepi abi ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_function_wrappers_keep_their_positional_calls():
    """CoarseEpilogueFn / FineEpilogueFn took 15 (16) and 14 positional arguments before the constant mode: the mode is a
    trailing argument that defaults to "linear", and render's switch exists and is on."""
    import inspect
    import plnerf_amd
    from plnerf_amd import functional as Fn
    Rd = sys.modules["plnerf_amd.render"]      # (the package attribute `render` is the function)
    coarse = inspect.signature(Fn.CoarseEpilogueFn.forward).parameters
    fine = inspect.signature(Fn.FineEpilogueFn.forward).parameters
    assert list(coarse)[-2:] == ["want_weights", "mode"] and coarse["mode"].default == "linear" and len(coarse) == 18
    assert list(fine)[-2:] == ["draws", "mode"] and fine["mode"].default == "linear" and len(fine) == 16
    assert Rd.FUSE_CONST_EPILOGUE is True
