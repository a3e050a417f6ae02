/*
 * plnerf_hip_gemm16.h -- EXPERIMENTAL: one nn.Linear of a network OUTSIDE the compiled trunk (netwidth > 256, netdepth > 8,
 * several live skips, multires > 10: the layer-by-layer route) in the arithmetic of the 16-bit precision modes.
 *
 * Experimental like the other headers of this directory: the library exports this entry and the binding binds it, but it is
 * outside the registered ABI -- no PLNERF_VERSION step, and it may still change.
 *
 * plnerf_gemm_f32 (plnerf_hip.h) serves that route on the exact-fp32 MFMA whatever the network's precision says.  This entry
 * is the FORWARD product of a layer in the modes PLNERF_PREC_BF16X3, _BF16, _F16X3 and _F16: operands and result are fp32 in
 * memory; both operands are split on the fly into x = hi + lo of IEEE half or bf16 (both conversions round to nearest even)
 * and each 16-deep k-step is hi.hi + lo.hi + hi.lo (A's lo with W's hi, then A's hi with W's lo), in this order, on
 * v_mfma_f32_32x32x16_f16 / _bf16 with fp32 accumulation; the plain modes issue the one product of the rounded operands.
 * k ascends from 0 whatever the tile and the launch: a row's result does not depend on the rows beside it.  The backward
 * products of such a layer stay on plnerf_gemm_f32, over the fp32 activations this entry writes.
 *
 * Conventions: those of plnerf_hip.h (device pointers, the call enqueues on `stream` and returns, every argument is checked
 * before the launch).  No alignment is demanded: rows that are not 16-byte aligned (an odd lda, an offset base) are read
 * dword by dword.
 */
#ifndef PLNERF_HIP_GEMM16_H
#define PLNERF_HIP_GEMM16_H

#include "../plnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C[M, N] = relu?(A[M, K] . W[N, K]^T + bias[N]).  A: row i at a + i lda (lda >= K); W as nn.Linear holds it: row j at
 * w + j ldw (ldw >= K); bias: [N] or NULL; C: row i at c + i ldc (ldc >= N).  Nothing between K and lda / ldw, or N and ldc, is
 * read or written.  K == 0: C = relu?(bias).  M == 0 or N == 0: PLNERF_OK, no launch.
 * precision: a PLNERF_PREC_* code; PLNERF_PREC_FP32 (and any value that is none of the four 16-bit modes) is PLNERF_EINVAL.
 * status: the range status word to OR into (semantics of PLNERF_RANGE_*), or NULL.  IEEE-half modes: an element of A beyond
 * +-65,504 or not finite enters the product clamped to +-65,504 and sets PLNERF_RANGE_ACTIVATION, such an element of W
 * PLNERF_RANGE_WEIGHT (at most one atomic OR per workgroup; with NULL the clamp is silent).  bf16-element modes carry fp32's
 * exponent range and set nothing.
 * PLNERF_EINVAL: a negative size, lda or ldw < K, ldc < N, c NULL, a or w NULL with K > 0, the precision.  PLNERF_ERANGE:
 * more than 2^31 - 1 output tiles (128 rows x 128 columns; 128 x 32 when N <= 32). */
int plnerf_gemm_h16(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias, int M, int N, int K, int relu,
                    int precision, float* c, int64_t ldc, int* status, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_GEMM16_H */
