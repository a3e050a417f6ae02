/*
 * plnerf_hip_gemm16_bwd.h -- EXPERIMENTAL: the two BACKWARD products of one nn.Linear of a network outside the compiled trunk
 * (the layer-by-layer route), in the arithmetic of the 16-bit precision modes.  The forward product is plnerf_gemm_h16
 * (plnerf_hip_gemm16.h); the arithmetic here is exactly that entry's.
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * Conventions: those of plnerf_hip_gemm16.h (device pointers, row strides in floats, the call enqueues on `stream` and
 * returns, every argument is checked before the launch, nothing outside the stated bytes is read or written).  No alignment
 * is demanded: an odd stride or an offset base is read dword by dword.
 *
 * The gated gradient.  Both entries take the upstream gradient g [M, N] (row m at g + m ldg, ldg >= N) and, optionally, the
 * layer's saved output y (indexed like g with ldy; NULL: no gate).  An element of g counts only where y > 0 (a NaN in y
 * gates the element off).  The gate is applied in the loader: no M x N temporary exists.
 *
 * Arithmetic.  precision is one of PLNERF_PREC_BF16X3, _BF16, _F16X3, _F16.  Both operands are split on the fly into
 * x = hi + lo of IEEE half or bf16 (both conversions round to nearest even); in the x3 modes each 16-deep step of the
 * contraction is hi.hi, lo.hi, hi.lo, in this order, the gated gradient in A's part (lo.hi = the gradient's lo with the
 * other operand's hi), on v_mfma_f32_32x32x16_f16 / _bf16 with fp32 accumulation; the plain modes issue the one hi.hi
 * product.  The contraction index ascends from 0 in steps of 16 (wgrad: from the start of each split).
 *
 * The gradient's scale.  g_absmax: NULL, or a device pointer to one fp32 word holding an upper bound of max |g| over the
 * operand.  The kernel derives a shift s from that word (the launch scale of the fused 16-bit backward: the maximum lands in
 * [2^3, 2^4); s = 127 at most; s = 0 for a word that is zero or not finite), multiplies the gated gradient by 2^s before the
 * split (exact) and the sums by 2^-s in the epilogue.  NULL: s = 0.  The scale applies in every mode when the word is given;
 * the IEEE-half modes need it for gradients below the half range (a mean-squared-error loss over 4096 rays: 1e-7 and less).
 *
 * Range (IEEE-half modes; PLNERF_RANGE_* of plnerf_hip.h).  An element of w beyond +-65,504 or not finite is clamped there
 * and sets PLNERF_RANGE_WEIGHT; such an element of x, or of the SCALED gated gradient (the word was no upper bound, or the
 * gradient is not finite), is clamped and sets PLNERF_RANGE_ACTIVATION.  At most one atomic OR per workgroup, none when
 * `status` is NULL.  The bf16 modes carry fp32's exponent range and set nothing.
 *
 * PLNERF_EINVAL: a negative size, a stride below its width (ldy only when y is given), a NULL output, a NULL operand with a
 * non-empty contraction, a precision that is none of the four 16-bit modes.  PLNERF_ERANGE: more than 2^31 - 1 workgroups in
 * a launch (output tiles of 128 x 128; 128 x 32 or 32 x 128 when an output dimension is <= 32; times k_splits), or -- wgrad --
 * K + 1 beyond INT_MAX.
 */
#ifndef PLNERF_HIP_GEMM16_BWD_H
#define PLNERF_HIP_GEMM16_BWD_H

#include "../plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dX[M, K] = (G (.) [Y > 0])[M, N] . W[N, K]: the contraction runs over n.  W is read in place, as nn.Linear holds it: the
 * element (n, k) at w + n ldw + k (ldw >= K).  dX: row m at dx + m lddx (lddx >= K).  A row's result does not depend on the
 * rows beside it, the tile or the launch it sits in.
 * M == 0 or K == 0: PLNERF_OK, no launch.  N == 0: dX is written as zeros. */
int plnerf_gemm_h16_dgrad(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* w, int64_t ldw,
                          int M, int N, int K, int precision, const float* g_absmax,
                          float* dx, int64_t lddx, int* status, plnerf_stream_t stream);

/* [dW | db][N, K + 1] = (G (.) [Y > 0])^T[N, M] . [X | 1][M, K + 1]: the contraction runs over the rows m; column K of the
 * result is the bias gradient.  X: row m at x + m ldx (ldx >= K).  The ones column is synthesised in the loader (the exact
 * value 1 for rows below M) and never read from memory.  dwb: row n at dwb + n lddwb (lddwb >= K + 1).
 * k_splits > 1 deals the rows out over that many workgroups per output tile.  With S = ceil(M / 32) stages of 32 rows and
 * P = ceil(S / k_splits), split z (0 <= z < k_splits) contracts the rows [32 z P, min(M, 32 (z + 1) P)): a function of
 * (M, k_splits) alone; a split whose range is empty contributes exact zeros.  The splits' products go to `partials`
 * (k_splits * N * (K + 1) floats, caller-owned, no initialisation needed) and a second launch adds them in split order and
 * applies 2^-s.  Neither launch uses a floating-point atomic: two identical calls are bitwise equal.  k_splits <= 1: one
 * launch, `partials` may be NULL.
 * N == 0: PLNERF_OK, no launch.  M == 0: dwb is written as zeros.  PLNERF_EINVAL also for k_splits > 1 with a NULL
 * `partials`. */
int plnerf_gemm_h16_wgrad(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* x, int64_t ldx,
                          int M, int N, int K, int precision, const float* g_absmax,
                          float* dwb, int64_t lddwb, int k_splits, float* partials, int* status, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_GEMM16_BWD_H */
