"""plnerf_gemm_h16_dgrad / _wgrad (include/experimental/plnerf_hip_gemm16_bwd.h) on the GPU: both products against fp64 under
a derived bound over the gradient's range, determinism and the row partition, the launch scale, the range status word, and
guard bands around every buffer."""
import ctypes
import struct

import pytest
import torch

import arena as A
from gpu_support import dev, g

pytestmark = pytest.mark.gpu

MODES = ("bf16x3", "bf16", "f16x3", "f16")
HALF = ("f16x3", "f16")
# (33, 128, 127): wgrad's ones column is the last column of a 128-wide tile; (33, 128, 128): a tile of its own
SHAPES = [(1, 1, 1), (37, 5, 3), (127, 63, 17), (128, 64, 16), (129, 65, 63), (300, 257, 129), (64, 320, 319), (777, 4, 320),
          (33, 128, 127), (33, 128, 128)]
# (magnitude of g, row-wise log-normal spread, only with the max |g| word given)
MAGNITUDES = [(1.0, 0.0, False), (1e-6, 3.0, False), (1e-30, 0.0, False), (1e20, 0.0, False), (1e-41, 0.0, True)]
SPLITS = (1, 2, 7)
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from plnerf_amd import _lib
    return _lib


def ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset) if t is not None else None


def dgrad(L, gd, ldg, yd, ldy, wd, ldw, M, N, K, mode, word, dx, lddx, status=None):
    rc = L.lib().plnerf_gemm_h16_dgrad(ptr(gd), ldg, ptr(yd), ldy, ptr(wd), ldw, M, N, K, L.PRECISION[mode], ptr(word), ptr(dx),
                                       lddx, ptr(status), L.stream())
    assert rc == 0, (rc, mode, M, N, K)


def wgrad(L, gd, ldg, yd, ldy, xd, ldx, M, N, K, mode, word, dwb, lddwb, splits=1, status=None, fill=None):
    """`partials` is allocated here: k_splits * N * (K + 1) floats, uninitialised -- or filled with `fill`."""
    partials = None
    if splits > 1:
        partials = torch.empty(splits * N * (K + 1), device=dev())
        if fill is not None:
            partials.fill_(fill)
    rc = L.lib().plnerf_gemm_h16_wgrad(ptr(gd), ldg, ptr(yd), ldy, ptr(xd), ldx, M, N, K, L.PRECISION[mode], ptr(word), ptr(dwb),
                                       lddwb, splits, ptr(partials), ptr(status), L.stream())
    assert rc == 0, (rc, mode, M, N, K, splits)


def padded(x, ld):
    """x [rows, cols] inside NaN-filled rows of `ld` floats (device)."""
    out = torch.full((x.shape[0], ld), NAN, dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return g(out)


def shift(word):
    """The launch scale's shift s for a max |g| word (a float or None), restated from csrc/mlp_layout.h's dzh_shift (target
    exponent 4: the maximum lands in [2^3, 2^4); at most 127; 0 for zero, infinity, NaN and for no word)."""
    if word is None:
        return 0
    bits = struct.unpack("<I", struct.pack("<f", word))[0] & 0x7fffffff
    e = bits >> 23
    if bits == 0 or e == 255:
        return 0
    return min(4 + 126 - e, 127)


def bound(mode, a, b, s):
    """The bound on |out_ij - sum_c a_ic b_jc|: a [I, C] the gated gradient, b [J, C] the other operand (the ones column
    included), s the launch scale's shift -- see test_products_against_fp64."""
    a, b = a.double().abs(), b.double().abs()
    C = a.shape[1]
    S = a @ b.T
    acc = (C + 4) * 2.0 ** -24
    u = 2.0 ** -11 if mode in HALF else 2.0 ** -8
    lim = (3 * u * u + acc) * S if mode.endswith("x3") else (2 * u + u * u + acc) * S
    if mode in HALF:
        lim = lim + 2.0 ** -25 * (2.0 ** -s * b.sum(1)[None, :] + a.sum(1)[:, None])
    return lim + 2.0 ** -150


def operands(M, N, K, magnitude=1.0, spread=0.0, gated=True):
    """(g, y or None, w, x): y has a few NaNs (gated off) with an infinite g under them; g is finite wherever it counts."""
    gen = torch.Generator().manual_seed(M * 1000 + N * 10 + K)
    grad = torch.randn(M, N, generator=gen) * magnitude * torch.exp(spread * torch.randn(M, 1, generator=gen))
    y = torch.randn(M, N, generator=gen)
    w, x = torch.randn(N, K, generator=gen), torch.randn(M, K, generator=gen)
    if not gated:
        return grad, None, w, x
    y[torch.rand(M, N, generator=gen) < 0.02] = NAN
    grad[torch.isnan(y)] = float("inf")
    return grad, y, w, x


_CASES = {}


def case(shape, magnitude=1.0, spread=0.0, gated=True):
    """The operands of a shape with their fp64 products, computed once: (g, y, w, x, gated g, max |gated g|, dX, [dW | db])."""
    key = (shape, magnitude, spread, gated)
    if key not in _CASES:
        grad, y, w, x = operands(*shape, magnitude, spread, gated)
        gt = torch.where(y > 0, grad, torch.zeros(())) if gated else grad
        x1 = torch.cat([x, torch.ones(shape[0], 1)], 1)
        _CASES[key] = (grad, y, w, x, gt, float(gt.abs().max()), gt.double() @ w.double(), gt.double().T @ x1.double(), x1)
    return _CASES[key]


def worst_ratio(out, ref, lim):
    assert bool(torch.isfinite(out).all())
    return float(((out.cpu().double() - ref).abs() / lim).max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_products_against_fp64(L, shape, mode):
    """dX = gate(G) W and [dW | db] = gate(G)^T [X | 1] against fp64, with and without the gate, over the gradient's range
    (|g| about 1, 1e-6 with a row-wise log-normal spread of 3, 1e-30, 1e20: the word given in the IEEE-half modes, NULL and
    the word in the bf16 modes; 1e-41, fp32 subnormals, only with the word), wgrad at k_splits 1, 2 and 7 (at M = 37 there
    are two stages: with 7 splits five ranges are empty).  Then once with every leading dimension beyond its width, NaN in
    all padding and NaN-prefilled outputs: the outputs' padding is NaN afterwards, every written element finite.

    The bound is tests/test_gpu_gemm16.py's, with the gated gradient g~ in A's part, b the other operand (the ones column
    included), C the contraction length and S = sum_c |g~||b|.  Every conversion rounds to nearest even, u = 2^-11 (IEEE
    half) or 2^-8 (bf16: hi is rounded, not truncated):
      x3 modes     (3 u^2 + (C + 4) 2^-24) S        the omitted lo.lo and the two second-order residuals; fp32 accumulation
      plain modes  (2 u + u^2 + (C + 4) 2^-24) S
      IEEE half    + 2^-25 (2^-s sum_c |b| + sum_c |g~|): an element of the SCALED gradient (or of b) landing among the half
                   subnormals, spacing 2^-24, carries an absolute error of 2^-25 -- 2^-25 2^-s in the gradient's own units.
    The power-of-two scale is exact and drops out.  One term is added here to what the issue lists: 2^-150, half the spacing
    of fp32's subnormals, for the rounding of the result itself when it is one (the 1e-41 runs: at C = 1 the listed terms
    come to 3e-48, below what fp32 can hold).  With wgrad's splits the partial sums are added in fp32: their C - 1 additions
    are inside the (C + 4)."""
    M, N, K = shape
    worst = 0.0
    for magnitude, spread, word_only in MAGNITUDES:
        for gated in (True, False):
            grad, y, w, x, gt, top, ref_d, ref_w, x1 = case(shape, magnitude, spread, gated)
            gd, yd, wd, xd = g(grad), (g(y) if gated else None), g(w), g(x)
            words = [top] if mode in HALF or word_only else [None, top]
            for word in words:
                s = shift(word)
                wordd = g(torch.tensor([word], dtype=torch.float32)) if word is not None else None
                lim_d, lim_w = bound(mode, gt, w.T, s), bound(mode, gt.T, x1.T, s)
                dx = torch.full((M, K), NAN, device=dev())
                dgrad(L, gd, N, yd, N, wd, K, M, N, K, mode, wordd, dx, K)
                ratios = {"dgrad": worst_ratio(dx, ref_d, lim_d)}
                for splits in SPLITS:
                    dwb = torch.full((N, K + 1), NAN, device=dev())
                    wgrad(L, gd, N, yd, N, xd, K, M, N, K, mode, wordd, dwb, K + 1, splits)
                    ratios[f"wgrad/{splits}"] = worst_ratio(dwb, ref_w, lim_w)
                print(f"gemm_h16 bwd {mode} {shape} |g| {magnitude:g} gate {gated} word {word is not None}: worst error / bound "
                      + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
                worst = max(worst, *ratios.values())
                assert all(v <= 1.0 for v in ratios.values()), (mode, shape, magnitude, gated, word, ratios)
    # leading dimensions beyond the widths: ldg a multiple of four beyond N (16-byte rows whose last chunk is ragged), the others odd
    grad, y, w, x, gt, top, ref_d, ref_w, x1 = case(shape)
    ldg, ldy, ldw, ldx, lddx, lddwb = (N + 7) // 4 * 4, N + 1, K + 3, K + 5, K + 2, K + 4
    word = top if mode in HALF else None
    wordd = g(torch.tensor([top], dtype=torch.float32)) if word is not None else None
    dx = torch.full((M, lddx), NAN, device=dev())
    dgrad(L, padded(grad, ldg), ldg, padded(y, ldy), ldy, padded(w, ldw), ldw, M, N, K, mode, wordd, dx, lddx)
    assert bool(torch.isnan(dx[:, K:]).all())
    assert worst_ratio(dx[:, :K], ref_d, bound(mode, gt, w.T, shift(word))) <= 1.0
    for splits in SPLITS:
        dwb = torch.full((N, lddwb), NAN, device=dev())
        wgrad(L, padded(grad, ldg), ldg, padded(y, ldy), ldy, padded(x, ldx), ldx, M, N, K, mode, wordd, dwb, lddwb, splits, fill=NAN)
        assert bool(torch.isnan(dwb[:, K + 1:]).all())
        assert worst_ratio(dwb[:, :K + 1], ref_w, bound(mode, gt.T, x1.T, shift(word))) <= 1.0
    print(f"gemm_h16 bwd {mode} {shape}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("mode", MODES)
def test_empty_products(L, mode):
    """dgrad with N == 0 writes dX as zeros; wgrad with M == 0 writes [dW | db] as zeros, whatever k_splits."""
    dx = torch.full((5, 7), NAN, device=dev())
    dgrad(L, None, 0, None, 0, None, 7, 5, 0, 7, mode, None, dx, 7)
    assert bool((dx == 0).all())
    for splits in (1, 3):
        dwb = torch.full((5, 8), NAN, device=dev())
        wgrad(L, None, 5, None, 0, None, 7, 0, 5, 7, mode, None, dwb, 8, splits)
        assert bool((dwb == 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_determinism_and_partition(L, mode):
    """Two identical calls are bitwise equal (both entries, every k_splits).  dgrad: 300 rows in one call, in two calls
    split at row 131 and at an offset inside a larger operand: bitwise equal.  wgrad at k_splits 2 and 7 against k_splits 1:
    the conversions are the same elements' in every split, only the fp32 order differs, so the results differ by the two
    accumulation shares of the bound at most, 2 (C + 4) 2^-24 S (+ 2^-149); not bitwise, by design."""
    shape = (300, 257, 129)
    M, N, K = shape
    grad, y, w, x, gt, top, ref_d, ref_w, x1 = case(shape)
    wordd = g(torch.tensor([top], dtype=torch.float32)) if mode in HALF else None
    gd, yd, wd, xd = g(grad), g(y), g(w), g(x)

    def run_d(gsrc, ysrc, first, rows):
        dx = torch.full((rows, K), NAN, device=dev())
        dgrad(L, gsrc[first:], N, ysrc[first:], N, wd, K, rows, N, K, mode, wordd, dx, K)
        return dx

    def run_w(splits):
        dwb = torch.full((N, K + 1), NAN, device=dev())
        wgrad(L, gd, N, yd, N, xd, K, M, N, K, mode, wordd, dwb, K + 1, splits)
        return dwb
    whole = run_d(gd, yd, 0, M)
    assert torch.equal(whole, run_d(gd, yd, 0, M))
    assert torch.equal(whole, torch.cat([run_d(gd, yd, 0, 131), run_d(gd, yd, 131, M - 131)], 0))
    gen = torch.Generator().manual_seed(9)
    before, after = torch.randn(77, N, generator=gen), torch.randn(200, N, generator=gen)
    larger_g, larger_y = g(torch.cat([before, grad, after], 0)), g(torch.cat([after[:77], y, before.repeat(3, 1)[:200]], 0))
    assert torch.equal(whole[40:], run_d(larger_g, larger_y, 77 + 40, M - 40))
    one = run_w(1)
    slack = 2 * (M + 4) * 2.0 ** -24 * (gt.double().abs().T @ x1.double().abs()) + 2.0 ** -149
    for splits in SPLITS:
        again = run_w(splits)
        assert torch.equal(again, run_w(splits)), splits
        assert bool(((again.cpu().double() - one.cpu().double()).abs() <= slack).all()), splits


@pytest.mark.parametrize("mode", MODES)
def test_the_scale_is_doing_the_work(L, mode):
    """g about 1e-9, (129, 65, 63).  f16x3: with the word both products are within the bound; with NULL (s = 0: the gradient
    sinks below the half subnormals) the error exceeds THAT bound -- the test can see a missing scale.  Every mode: a word that
    understates max |g| by 2^20 puts the scaled gradient beyond 65,504 -- the IEEE-half modes set PLNERF_RANGE_ACTIVATION (and
    only that) and every output is finite, the bf16 modes set nothing; an infinite element of g (and so an infinite word,
    s = 0) does the same."""
    shape = (129, 65, 63)
    M, N, K = shape
    grad, y, w, x, gt, top, ref_d, ref_w, x1 = case(shape, 1e-9)
    gd, yd, wd, xd = g(grad), g(y), g(w), g(x)

    def run(gsrc, word, with_status=False):
        wordd = g(torch.tensor([word], dtype=torch.float32)) if word is not None else None
        status = torch.zeros(2, dtype=torch.int32, device=dev()) if with_status else None
        dx, dwb = torch.full((M, K), NAN, device=dev()), torch.full((N, K + 1), NAN, device=dev())
        dgrad(L, gsrc, N, yd, N, wd, K, M, N, K, mode, wordd, dx, K, status)
        wgrad(L, gsrc, N, yd, N, xd, K, M, N, K, mode, wordd, dwb, K + 1, 2, status[1:] if with_status else None)
        torch.cuda.synchronize()
        return dx, dwb, ([int(v) for v in status.tolist()] if with_status else None)
    if mode == "f16x3":
        lim_d, lim_w = bound(mode, gt, w.T, shift(top)), bound(mode, gt.T, x1.T, shift(top))
        dx, dwb, _ = run(gd, top)
        with_word = worst_ratio(dx, ref_d, lim_d), worst_ratio(dwb, ref_w, lim_w)
        dx, dwb, _ = run(gd, None)
        without = worst_ratio(dx, ref_d, lim_d), worst_ratio(dwb, ref_w, lim_w)
        print(f"f16x3, |g| 1e-9: worst error / bound with the word {with_word}, without {without}")
        assert max(with_word) <= 1.0 and min(without) > 1.0
    expect = L.RANGE_ACTIVATION if mode in HALF else 0
    dx, dwb, bits = run(gd, top * 2.0 ** -20, with_status=True)
    assert bits == [expect, expect], bits
    if mode in HALF:
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dwb).all())
    run(gd, top * 2.0 ** -20)      # (a NULL status: the clamp is silent)
    infinite = gt.clone()      # (the gated gradient: the infinity counts under either gate value, so no gate here)
    infinite[17, 5] = float("inf")
    yd = None
    dx, dwb, bits = run(g(infinite), float("inf"), with_status=True)
    assert bits == [expect, expect], bits
    if mode in HALF:
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dwb).all())


@pytest.mark.parametrize("mode", MODES)
def test_range_status(L, mode):
    """M = 40, N = 8, K = 24.  One element of w at 1e5, then infinite: dgrad sets PLNERF_RANGE_WEIGHT in the IEEE-half modes
    and only that; one element of x at 1e5: wgrad sets PLNERF_RANGE_ACTIVATION.  The bf16 modes set nothing and stay within
    the bound.  Clean operands set nothing.  A NULL status with the same inputs is PLNERF_OK."""
    shape = (40, 8, 24)
    M, N, K = shape
    grad, y, w, x, gt, top, _, _, _ = case(shape)
    half = mode in HALF
    wordd = g(torch.tensor([top], dtype=torch.float32)) if half else None
    s = shift(top if half else None)
    gd, yd = g(grad), g(y)

    def run_d(w_, with_status=True):
        status = torch.zeros(1, dtype=torch.int32, device=dev()) if with_status else None
        dx = torch.full((M, K), NAN, device=dev())
        dgrad(L, gd, N, yd, N, g(w_), K, M, N, K, mode, wordd, dx, K, status)
        torch.cuda.synchronize()
        return dx, (int(status.item()) if with_status else None)

    def run_w(x_, with_status=True, splits=1):
        status = torch.zeros(1, dtype=torch.int32, device=dev()) if with_status else None
        dwb = torch.full((N, K + 1), NAN, device=dev())
        wgrad(L, gd, N, yd, N, g(x_), K, M, N, K, mode, wordd, dwb, K + 1, splits, status)
        torch.cuda.synchronize()
        return dwb, (int(status.item()) if with_status else None)
    assert run_d(w)[1] == 0 and run_w(x)[1] == 0 and run_w(x, splits=2)[1] == 0
    for value in (1e5, float("inf")):
        big_w = w.clone()
        big_w[3, 20] = value
        dx, bits = run_d(big_w)
        assert bits == (L.RANGE_WEIGHT if half else 0), (value, bits)
        if half:
            assert bool(torch.isfinite(dx).all())
        elif value == 1e5:
            assert worst_ratio(dx, gt.double() @ big_w.double(), bound(mode, gt, big_w.T, s)) <= 1.0
        run_d(big_w, with_status=False)
    big_x = x.clone()
    big_x[17, 5] = 1e5
    for splits in (1, 2):
        dwb, bits = run_w(big_x, splits=splits)
        assert bits == (L.RANGE_ACTIVATION if half else 0), bits
        big_x1 = torch.cat([big_x, torch.ones(M, 1)], 1)
        if half:
            assert bool(torch.isfinite(dwb).all())
        else:
            assert worst_ratio(dwb, gt.double().T @ big_x1.double(), bound(mode, gt.T, big_x1.T, s)) <= 1.0
    run_w(big_x, with_status=False)


@pytest.mark.parametrize("scratch_fill", (0x00, 0xFF))
@pytest.mark.parametrize("mode", MODES)
def test_nothing_outside_the_given_bytes_changes(L, mode, scratch_fill):
    """Every buffer of both entries in an arena between guard bands (tests/arena.py), at the ragged shape (129, 65, 63) with
    padded leading dimensions: g, y, w, x, the max |g| word (`in`), dX and [dW | db] (`out`), the partials of three splits
    (`scratch`: once at 0x00, once at 0xFF), the status word (`zeroed`).  g is carved at a base offset by one float."""
    shape = (129, 65, 63)
    M, N, K = shape
    splits = 3
    ldg, ldy, ldw, ldx, lddx, lddwb = N + 2, N + 1, K + 1, K + 3, K + 2, K + 4
    grad, y, w, x, gt, top, ref_d, ref_w, x1 = case(shape)

    def span(rows, ld, cols):
        return ((rows - 1) * ld + cols) * 4
    sizes = dict(g=span(M, ldg, N), y=span(M, ldy, N), w=span(N, ldw, K), x=span(M, ldx, K), word=4, dx=span(M, lddx, K),
                 dwb=span(N, lddwb, K + 1), partials=splits * N * (K + 1) * 4, status=4)
    ar = A.Arena(dev(), sum(A.Arena.room(n) for n in sizes.values()) + A.MIN_GUARD)
    roles = dict(g="in", y="in", w="in", x="in", word="in", dx="out", dwb="out", partials="scratch", status="zeroed")
    b = {name: ar.carve(name, sizes[name], align=4, role=roles[name]) for name in sizes}
    assert b["g"].dptr % 8 == 4

    def put(buf, t, ld):
        flat = torch.full((t.shape[0] * ld,), NAN)
        flat.reshape(t.shape[0], ld)[:, :t.shape[1]] = t
        buf.put(flat[:buf.nbytes // 4])
    put(b["g"], grad, ldg)
    put(b["y"], y, ldy)
    put(b["w"], w, ldw)
    put(b["x"], x, ldx)
    b["word"].put(torch.tensor([top], dtype=torch.float32))
    b["partials"].set_bytes(scratch_fill)
    for name in ("g", "y", "w", "x", "word"):
        b[name].freeze()
    p = {name: ctypes.c_void_p(buf.dptr) for name, buf in b.items()}
    code = L.PRECISION[mode]
    assert L.lib().plnerf_gemm_h16_dgrad(p["g"], ldg, p["y"], ldy, p["w"], ldw, M, N, K, code, p["word"], p["dx"], lddx,
                                         p["status"], L.stream()) == 0
    assert L.lib().plnerf_gemm_h16_wgrad(p["g"], ldg, p["y"], ldy, p["x"], ldx, M, N, K, code, p["word"], p["dwb"], lddwb, splits,
                                         p["partials"], p["status"], L.stream()) == 0
    torch.cuda.synchronize()
    ar.check()

    def rows_of(buf, rows, ld):
        flat = torch.full((rows * ld,), NAN, device=dev())
        flat[:buf.nbytes // 4] = buf.f32()
        return flat.reshape(rows, ld)
    dx, dwb = rows_of(b["dx"], M, lddx), rows_of(b["dwb"], N, lddwb)
    assert bool(torch.isnan(dx[:, K:]).all()) and bool(torch.isnan(dwb[:, K + 1:]).all())
    s = shift(top)
    assert worst_ratio(dx[:, :K], ref_d, bound(mode, gt, w.T, s)) <= 1.0
    assert worst_ratio(dwb[:, :K + 1], ref_w, bound(mode, gt.T, x1.T, s)) <= 1.0
