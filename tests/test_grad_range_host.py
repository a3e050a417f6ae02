"""tests/grad_range_cases.py without a GPU: what tests/test_gpu_grad_range.py takes for granted about its own inputs."""
import numpy as np

import grad_range_cases as C


def test_the_oracle_flags_few_rows():
    """The rows are drawn so that the fp64 oracle flags none of them at the widest amb; the cap the GPU tests assert holds for
    every mode, and every ray kept SPR of its candidates (draw_rows asserts it)."""
    pts, vd = C.rows()
    assert pts.shape == (C.N_RAYS, C.SPR, 3) and vd.shape == (C.N_RAYS, 3) and float(pts.abs().max()) <= 2.5
    for mode in ("fp32", "bf16x3", "f16x3", "bf16", "f16"):
        share = float(C.flagged(C.amb_of(mode)).mean())
        assert share <= C.AMB_CAP, (mode, share)


def test_cotangents_shift_exactly():
    """ldexp of the base cotangent over the whole window of part (b) is exact (undoing it gives the same bits), the wide
    cotangent spans 2^-25 .. 1, and part (c)'s maxima are exactly the powers of two it names."""
    c = C.base(0.0)
    mag = np.abs(c[c != 0])
    assert c.dtype == np.float32 and c.shape == (C.N_ROWS, 4) and 2.0 ** -7 <= mag.min() and mag.max() < 1.0
    assert len(np.unique(np.floor(np.log2(np.abs(c).max(-1))))) == 7      # every factor 2^0 .. 2^-6 occurs
    for k in (-60, -24, -1, 1, 24, 60, 100):
        shifted = np.ldexp(c, k)
        assert shifted.dtype == np.float32 and np.isfinite(shifted).all()
        assert np.array_equal(np.ldexp(shifted, -k).view(np.int32), c.view(np.int32)), k
    wide = np.abs(C.base(0.0, 24))
    assert 2.0 ** -25 <= wide[wide != 0].min() < 2.0 ** -22 and 0.5 <= wide.max() < 1.0
    for p in (123, 125, 126, 135):
        g_raw, up = C.low_end(0.0, p)
        assert g_raw.dtype == np.float32 and np.abs(g_raw).max() == np.float32(2.0) ** -p and np.abs(up).max() == 1.0
    cand = C.absmax_candidates(c)
    assert cand.dtype == np.int32 and cand.shape == (C.N_ROWS * 4 // 32,) and cand.max() == np.abs(c).max().view(np.int32)


def test_the_yardstick_is_linear_in_the_cotangent():
    """The float64 oracle gradient of 2^-60 c is 2^-60 times that of c, to float64 rounding: what part (b) rests on."""
    ref = C.reference(0.0, "base")
    small = C.oracle_grads(np.ldexp(C.base(0.0).astype(np.float64), -60))
    assert len(ref) == 24
    for name, r in ref.items():
        assert np.abs(r).max() > 0 and np.array_equal(np.ldexp(small[name], 60), r), name
