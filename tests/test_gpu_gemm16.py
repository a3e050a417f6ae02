"""plnerf_gemm_h16 (include/experimental/plnerf_hip_gemm16.h) on the GPU: the product against fp64 under a derived bound, the
row partition bit for bit, the range status word, and guard bands around every buffer."""
import ctypes

import pytest
import torch

import arena as A
from gpu_support import dev, g

pytestmark = pytest.mark.gpu

MODES = ("bf16x3", "bf16", "f16x3", "f16")
SHAPES = [(1, 1, 1), (37, 5, 3), (127, 63, 17), (128, 64, 16), (129, 65, 63), (300, 257, 129), (64, 320, 319), (3, 700, 575)]
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from plnerf_amd import _lib
    return _lib


def ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset) if t is not None else None


def gemm(L, a, lda, w, ldw, bias, M, N, K, relu, mode, c, ldc, status=None):
    """The raw entry on device tensors (a, w, c: flat or 2-D, the leading dimensions as given)."""
    rc = L.lib().plnerf_gemm_h16(ptr(a), lda, ptr(w), ldw, ptr(bias), M, N, K, int(relu), L.PRECISION[mode], ptr(c), ldc,
                                 ptr(status), L.stream())
    assert rc == 0, (rc, mode, M, N, K)


def padded(x, ld):
    """x [rows, cols] inside NaN-filled rows of `ld` floats (device)."""
    out = torch.full((x.shape[0], ld), NAN, dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return g(out)


def bound(mode, a, w, bias=None):
    """The bound on |C_ij - (a w^T + bias)_ij| -- see test_product_against_fp64."""
    a, w = a.double().abs(), w.double().abs()
    K = a.shape[1]
    S = a @ w.T
    acc = (K + 4) * 2.0 ** -24
    if mode == "bf16x3":
        b = (3 * 2.0 ** -7 * 2.0 ** -8 + acc) * S
    elif mode == "f16x3":
        b = (3 * 2.0 ** -11 * 2.0 ** -11 + acc) * S + 2.0 ** -25 * (a.sum(1)[:, None] + w.sum(1)[None, :])
    else:
        u = 2.0 ** -11 if mode == "f16" else 2.0 ** -8
        b = (u + u + u * u + acc) * S
    if bias is not None:
        b = b + 2.0 ** -24 * bias.double().abs()[None, :]
    return b


def case(M, N, K):
    gen = torch.Generator().manual_seed(M * 1000 + N * 10 + K)
    return torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(N, generator=gen)


@pytest.fixture(scope="module")
def references():
    """(a, w, bias, a w^T in fp64) per shape, computed once."""
    out = {}
    for shape in SHAPES:
        a, w, b = case(*shape)
        out[shape] = (a, w, b, a.double() @ w.double().T)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_product_against_fp64(L, references, shape, mode):
    """C = relu?(A W^T + bias) against fp64, with and without bias and relu, and once with lda / ldw / ldc beyond K / K / N,
    NaN in every padding column and a NaN-prefilled C: the padding of C is NaN afterwards, every written element finite.

    The bound is derived from the conversions the kernel uses.  Every conversion rounds to nearest even: IEEE half has 11
    significant bits (unit roundoff 2^-11), bf16 has 8 (2^-8).
      x3 modes.  x = hi + lo + d with |lo| <= u_hi |x| and |d| <= u_hi u_lo |x| (lo is the exact fp32 residual x - hi, rounded
      once).  The three products leave out lo.lo and the two d terms: |a w - (ah wh + al wh + ah wl)| <= (u_hi u_lo + u_hi u_lo
      + u_hi^2) |a||w| to first order, which is 3 u_hi u_lo when u_hi <= u_lo.  IEEE half: u_hi = u_lo = 2^-11.  bf16: the
      bound is asserted with the figures the issue states, u_hi = 2^-7 (a truncated hi) and u_lo = 2^-8; this kernel rounds hi
      to nearest (u_hi = 2^-8 = u_lo), so its own 3 u_hi u_lo is half of that and the asserted bound holds with room (with a
      truncated hi the omitted lo.lo term, u_hi^2 = 2 u_hi u_lo, would not be covered by it).  The fp32 accumulation of the
      k-steps' products in the MFMA and the rounding of the sum the bias is added to: (K + 4) 2^-24.  With
      S_ij = sum_k |a_ik||w_jk| in fp64:
          bf16x3:  (3 * 2^-7 * 2^-8 + (K + 4) 2^-24) S_ij
          f16x3:   (3 * 2^-11 * 2^-11 + (K + 4) 2^-24) S_ij + 2^-25 sum_k (|a_ik| + |w_jk|)
      the last term: lo (or a small hi) landing among the f16 subnormals, spacing 2^-24.
      plain modes.  One conversion per operand, u_a = u_w = u (2^-11 for f16, 2^-8 for bf16):
          (u_a + u_w + u_a u_w + (K + 4) 2^-24) S_ij
      With a bias the result is fl(sum + bias_j): one more fp32 rounding, of a value up to |sum| + |bias_j|; the |sum| share
      is inside the (K + 4), the other is 2^-24 |bias_j|, added to the bound of the runs that pass a bias (only those)."""
    M, N, K = shape
    a, w, b, prod = references[shape]
    worst = 0.0
    for with_bias, relu in ((True, True), (False, False), (True, False), (False, True)):
        c = torch.full((M, N), NAN, device=dev())
        gemm(L, g(a), K, g(w), K, g(b) if with_bias else None, M, N, K, relu, mode, c, N)
        ref = prod + b.double()[None, :] if with_bias else prod
        err = (c.cpu().double() - (torch.relu(ref) if relu else ref)).abs()      # (relu is 1-Lipschitz: the same bound)
        lim = bound(mode, a, w, b if with_bias else None)
        worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
        assert bool(torch.isfinite(c).all()), (mode, shape, with_bias, relu)
        assert bool((err <= lim).all()), (mode, shape, with_bias, relu, float((err / lim).max()))
    # leading dimensions beyond the sizes: lda a multiple of four beyond K (16-byte rows whose last chunk is ragged), ldw odd
    lda, ldw, ldc = (K + 7) // 4 * 4, K + 3, N + 5
    c = torch.full((M, ldc), NAN, device=dev())
    gemm(L, padded(a, lda), lda, padded(w, ldw), ldw, g(b), M, N, K, False, mode, c, ldc)
    err = (c[:, :N].cpu().double() - (prod + b.double()[None, :])).abs()
    lim = bound(mode, a, w, b)
    worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
    print(f"gemm_h16 {mode} {shape}: worst error / bound {worst:.3f}")
    assert bool(torch.isfinite(c[:, :N]).all()) and bool(torch.isnan(c[:, N:]).all())
    assert bool((err <= lim).all()), (mode, shape, "padded", float((err / lim).max()))


@pytest.mark.parametrize("mode", MODES)
def test_row_partition_is_invisible(L, mode):
    """300 rows in one call, in two calls split at row 131, and at another offset inside a larger A: bitwise equal; two
    identical calls are bitwise equal."""
    M, N, K = 300, 257, 129
    a, w, b = case(M, N, K)
    ad, wd, bd = g(a), g(w), g(b)

    def run(src, first, rows):
        c = torch.full((rows, N), NAN, device=dev())
        gemm(L, src[first:], K, wd, K, bd, rows, N, K, True, mode, c, N)
        return c
    whole = run(ad, 0, M)
    assert torch.equal(whole, run(ad, 0, M))
    assert torch.equal(whole, torch.cat([run(ad, 0, 131), run(ad, 131, M - 131)], 0))
    gen = torch.Generator().manual_seed(9)
    larger = g(torch.cat([torch.randn(77, K, generator=gen), a, torch.randn(200, K, generator=gen)], 0))
    assert torch.equal(whole, run(larger, 0, 77 + M + 200)[77:77 + M])
    assert torch.equal(whole[40:], run(larger, 77 + 40, M - 40))


@pytest.mark.parametrize("mode", MODES)
def test_range_status(L, mode):
    """M = 40, N = 8, K = 24.  One element of A at 1e5: the IEEE-half modes set PLNERF_RANGE_ACTIVATION and only that, the bf16
    modes nothing (and stay within the product bound).  One element of W at 1e5, then infinite: the half modes set
    PLNERF_RANGE_WEIGHT.  A NULL status with the same inputs is PLNERF_OK."""
    M, N, K = 40, 8, 24
    a, w, b = case(M, N, K)
    half = mode in ("f16x3", "f16")

    def run(a_, w_, with_status=True):
        status = torch.zeros(1, dtype=torch.int32, device=dev()) if with_status else None
        c = torch.full((M, N), NAN, device=dev())
        gemm(L, g(a_), K, g(w_), K, g(b), M, N, K, False, mode, c, N, status)
        torch.cuda.synchronize()
        return c, (int(status.item()) if with_status else None)
    assert run(a, w)[1] == 0
    big_a = a.clone()
    big_a[17, 5] = 1e5
    c, bits = run(big_a, w)
    assert bits == (L.RANGE_ACTIVATION if half else 0), bits
    if half:
        assert bool(torch.isfinite(c).all())
    else:
        err = (c.cpu().double() - (big_a.double() @ w.double().T + b.double()[None, :])).abs()
        assert bool((err <= bound(mode, big_a, w, b)).all())
    run(big_a, w, with_status=False)
    for value in (1e5, float("inf")):
        big_w = w.clone()
        big_w[3, 20] = value
        c, bits = run(a, big_w)
        assert bits == (L.RANGE_WEIGHT if half else 0), (value, bits)
        if half:
            assert bool(torch.isfinite(c).all())
        run(a, big_w, with_status=False)


@pytest.mark.parametrize("mode", MODES)
def test_nothing_outside_the_given_bytes_changes(L, mode):
    """Every buffer in an arena between guard bands (tests/arena.py: the fill is NaN as fp32), at the ragged shape
    (129, 65, 63) with ldc > N: A, W, bias, C and the status word.  A is carved at a 4-byte alignment that is no multiple of
    8 (a base offset by one float): accepted, and the result within the bound."""
    M, N, K = 129, 65, 63
    lda, ldw, ldc = K, K, N + 3
    a, w, b = case(M, N, K)
    sizes = dict(a=((M - 1) * lda + K) * 4, w=((N - 1) * ldw + K) * 4, bias=N * 4, c=((M - 1) * ldc + N) * 4, status=4)
    ar = A.Arena(dev(), sum(A.Arena.room(n) for n in sizes.values()) + A.MIN_GUARD)
    ba = ar.carve("a", sizes["a"], align=4, role="in")
    bw = ar.carve("w", sizes["w"], align=4, role="in")
    bb = ar.carve("bias", sizes["bias"], align=4, role="in")
    bc = ar.carve("c", sizes["c"], align=4, role="out")
    bs = ar.carve("status", 4, align=4, role="zeroed")
    assert ba.dptr % 8 == 4
    ba.put(a)
    bw.put(w)
    bb.put(b)
    for buf in (ba, bw, bb):
        buf.freeze()
    rc = L.lib().plnerf_gemm_h16(ctypes.c_void_p(ba.dptr), lda, ctypes.c_void_p(bw.dptr), ldw, ctypes.c_void_p(bb.dptr), M, N, K,
                                 0, L.PRECISION[mode], ctypes.c_void_p(bc.dptr), ldc, ctypes.c_void_p(bs.dptr), L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    ar.check()
    flat = torch.full((M * ldc,), NAN, device=dev())
    flat[:sizes["c"] // 4] = bc.f32()
    c = flat.reshape(M, ldc)
    assert bool(torch.isnan(c[:, N:]).all()) and bool(torch.isfinite(c[:, :N]).all())
    err = (c[:, :N].cpu().double() - (a.double() @ w.double().T + b.double()[None, :])).abs()
    assert bool((err <= bound(mode, a, w, b)).all()), float((err / bound(mode, a, w, b)).max())
