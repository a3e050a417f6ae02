"""The C ABI of the use_batching ray source (include/plnerf_hip_batching.h), without a GPU: the header is plain C99 and
links against the library with the declared prototype, and its argument validation runs before any device work.  (The
ctypes binding _lib.BATCHING_SIGNATURES against the header: tests/test_abi_headers.py.)"""
import subprocess

import pytest

import abi_support as abi


@pytest.fixture(scope="module")
def L():
    return abi.built_lib()


_C = r"""
#include <stdio.h>
#include "plnerf_hip_batching.h"

int main(void) {
    int (*p)(int, const int*, int, int, float, float, float, float, const float*, const float*, uint64_t, uint32_t, int,
             int, float, float, float*, float*, float*, float*, float*, float*, int*, plnerf_stream_t) =
        plnerf_select_bank_rays;
    int views[1] = {0};
    float dummy[12] = {0};
    if (plnerf_version() != PLNERF_VERSION || PLNERF_VERSION < 601) return 2;
    /* validation before any device work: these calls never touch the (absent) GPU */
    if (p(0, views, 4, 4, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 1, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy, NULL,
          NULL, NULL) != PLNERF_EINVAL) return 3;
    if (p(1, NULL, 4, 4, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 1, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy, NULL,
          NULL, NULL) != PLNERF_EINVAL) return 4;
    /* M = 3 * 12 * 17 = 612: positions [600, 613) run past the epoch */
    if (p(3, views, 12, 17, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 600, 13, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy,
          NULL, NULL, NULL) != PLNERF_ERANGE) return 5;
    /* M = 2 * 32768 * 32768 = 2^31 > 2^30 */
    if (p(2, views, 32768, 32768, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 1, 0.f, 1.f, dummy, dummy, NULL, dummy, dummy,
          NULL, NULL, NULL) != PLNERF_ERANGE) return 6;
    /* nothing to do */
    if (p(3, views, 12, 17, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 612, 0, 0.f, 1.f, NULL, NULL, NULL, NULL, NULL, NULL,
          NULL, NULL) != PLNERF_OK) return 7;
    if (p(3, views, 12, 17, 1.f, 1.f, 2.f, 2.f, dummy, NULL, 0, 0, 0, 4, 0.f, 1.f, NULL, NULL, NULL, NULL, NULL, NULL,
          NULL, NULL) != PLNERF_EINVAL) return 8;
    printf("batching abi ok\n");
    return 0;
}
"""


def test_batching_header_is_plain_c_and_links(L, tmp_path):
    assert set(L.BATCHING_SIGNATURES) == {"plnerf_select_bank_rays"}
    out = subprocess.run([abi.compile_c(_C, tmp_path, "batching_abi")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "batching abi ok" in out.stdout
