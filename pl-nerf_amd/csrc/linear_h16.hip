// One nn.Linear of the generic route on the 16-bit MFMAs: C[M, N] = relu?(A[M, K] . W[N, K]^T + bias[N]), operands and
// result fp32 in memory (include/experimental/plnerf_hip_gemm16.h).
//
// Reference: run_nerf_helpers.py:76-128 builds ANY netdepth / netwidth / skip list / encoding width; what the fused kernels
// are not compiled for runs layer by layer (pl-nerf_amd/generic.py).  linear.hip serves that route on the exact-fp32 MFMA
// whatever `precision` says; this file is the forward of the four 16-bit modes, in the arithmetic the fused kernels use
// (DESIGN section 5): both operands are split ON THE FLY, in the loader, into x = hi + lo of IEEE half or bf16 (hi = the
// value rounded to nearest even, lo = the fp32 residual x - hi, exact, rounded to nearest even), and every 16-deep k-step of
// a 32 x 32 block is, in this order, hi.hi, lo.hi (A's lo with W's hi), hi.lo on v_mfma_f32_32x32x16_f16 / _bf16 with fp32
// accumulation; the plain modes issue the one hi.hi product.
//
// Structure (linear_h16_dev.h: Tile, and run_stages for the pipeline's description -- this kernel carries the loop in its own
// text, see there): 256 threads = four waves on a 128 x 128 tile, 128 x 32 for N <= 32; a stage is 32 k deep.  Both operands are k-contiguous in memory: a thread loads four consecutive k of a row (one
// 16-byte load when the base and the row stride allow it, dwords otherwise: the first layer reads K = lda = 63), splits them
// and writes the halves k-fastest into the stage's planes (row stride 80 bytes = 5 sixteen-byte slots: odd, so the sixteen
// rows of a ds_read_b128 lane group lie on sixteen different slots of the 256-byte bank row), where a lane's eight
// k-elements of an MFMA operand are one 16-byte read.
//
// Edges: rows past M, columns past N and k past K contribute exact zeros and are never loaded; neither is anything between K
// and the row stride.  Range (PLNERF_RANGE_* of plnerf_hip.h), IEEE-half modes only: an element of A beyond +-65,504 or not
// finite is clamped there and raises PLNERF_RANGE_ACTIVATION, such an element of W PLNERF_RANGE_WEIGHT -- one atomic OR per
// workgroup at most, none when `status` is NULL.  bf16 elements carry fp32's exponent range and set nothing.
#include "linear_h16_dev.h"
#include "../../include/experimental/plnerf_hip_gemm16.h"

namespace {

struct Gemm16Args {
    const float* a; long long lda;
    const float* w; long long ldw;
    const float* bias;      // [N] or nullptr
    int M, N, K;
    int relu;
    float* c; long long ldc;
    unsigned* status;       // or nullptr
    int tiles_n;            // column tiles: workgroup b owns tile (b / tiles_n, b % tiles_n) -- the tiles that share rows of A
                            // run side by side
    int a_vec, w_vec;       // the operand's rows may be read 16 bytes at a time
};

template <bool BF, class T>
__global__ __launch_bounds__(THREADS) void gemm_h16_kernel(const Gemm16Args p) {
    constexpr int NS = T::NS, WM = T::WM, BM = T::BM, BN = T::BN;
    typedef typename Elem<BF>::v8 v8;
    constexpr int TM = T::TM, TN = T::TN, A_PLANE = T::A_PLANE, W_PLANE = T::B_PLANE, W_OFF = T::B_OFF, STAGE = T::STAGE;
    constexpr int CA = TM * (KS / 4) / THREADS, CW = TN * (KS / 4) / THREADS;      // four-k chunks per thread and stage
    static_assert(TM * (KS / 4) % THREADS == 0 && TN * (KS / 4) % THREADS == 0, "whole chunks per thread");
    // two stages, and nothing else: the split variants' 81,920 bytes fit a CU's 163,840 exactly twice, so the range flags
    // are gathered in the first dword of the stages once the k loop is done with them, not in a word of their own
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_m = (int)(blockIdx.x / (unsigned)p.tiles_n), tile_n = (int)(blockIdx.x % (unsigned)p.tiles_n);
    const int i0 = tile_m * TM, j0 = tile_n * TN;
    const int wi = (wave % WM) * BM * 32, wj = (wave / WM) * BN * 32;

    f32x16 acc[BM][BN];
    plnerf::zero_acc(acc);
    f32x4 ra[CA], rw[CW];
    unsigned top_a = 0u, top_w = 0u;      // IEEE-half elements: the largest magnitudes split so far (bit patterns)
    const int n_stages = (p.K + KS - 1) / KS;

    // (chunk q of a thread: row (tid + 256 q) >> 3 of the tile, k-elements 4 ((tid + 256 q) & 7) .. + 3 of the stage)
    auto fetch = [&](const int s) {      // stage s of both operands, global memory -> registers
        const int k0 = s * KS;
#pragma unroll
        for (int q = 0; q < CA; ++q) {
            const int ch = tid + THREADS * q;
            ra[q] = load4(p.a, p.lda, i0 + (ch >> 3), p.M, k0 + 4 * (ch & 7), p.K, p.a_vec);
        }
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            const int ch = tid + THREADS * q;
            rw[q] = load4(p.w, p.ldw, j0 + (ch >> 3), p.N, k0 + 4 * (ch & 7), p.K, p.w_vec);
        }
    };
    auto stash = [&](unsigned char* stage) {      // registers -> the stage's planes, split
#pragma unroll
        for (int q = 0; q < CA; ++q) {
            const int ch = tid + THREADS * q;
            if constexpr (!BF) clamp4(ra[q], top_a);
            store4<BF, NS>(stage, A_PLANE, ch >> 3, ch & 7, ra[q]);
        }
#pragma unroll
        for (int q = 0; q < CW; ++q) {
            const int ch = tid + THREADS * q;
            if constexpr (!BF) clamp4(rw[q], top_w);
            store4<BF, NS>(stage + W_OFF, W_PLANE, ch >> 3, ch & 7, rw[q]);
        }
    };

    // (run_stages' loop in this kernel's own text: linear_h16_dev.h describes it and says why it is not called here)
    if (n_stages > 0) {
        fetch(0);
        stash(smem);
    }
    __syncthreads();
    // this lane's operand rows: row (lane & 31) of a block, k-elements 8 (lane >> 5) .. + 7 of a k-step
    const int frag = (lane & 31) * RS + (lane >> 5) * 16;
    for (int s = 0; s < n_stages; ++s) {
        const unsigned char* cur = smem + (s & 1) * STAGE;
        if (s + 1 < n_stages) fetch(s + 1);
#pragma unroll
        for (int ks = 0; ks < KS / 16; ++ks) {
            v8 fa[BM][NS], fw[BN][NS];
#pragma unroll
            for (int b = 0; b < BM; ++b)
#pragma unroll
                for (int h = 0; h < NS; ++h)
                    fa[b][h] = *reinterpret_cast<const v8*>(cur + h * A_PLANE + (wi + 32 * b) * RS + frag + ks * 32);
#pragma unroll
            for (int b = 0; b < BN; ++b)
#pragma unroll
                for (int h = 0; h < NS; ++h)
                    fw[b][h] = *reinterpret_cast<const v8*>(cur + W_OFF + h * W_PLANE + (wj + 32 * b) * RS + frag + ks * 32);
#pragma unroll
            for (int bi = 0; bi < BM; ++bi)
#pragma unroll
                for (int bj = 0; bj < BN; ++bj) {
                    acc[bi][bj] = Elem<BF>::mfma(fa[bi][0], fw[bj][0], acc[bi][bj]);                          // hi . hi
                    if constexpr (NS == 2) {
                        acc[bi][bj] = Elem<BF>::mfma(fa[bi][1], fw[bj][0], acc[bi][bj]);                      // lo . hi
                        acc[bi][bj] = Elem<BF>::mfma(fa[bi][0], fw[bj][1], acc[bi][bj]);                      // hi . lo
                    }
                }
        }
        // (the other buffer's last readers were the previous stage's MFMAs, behind the barrier that ended it)
        if (s + 1 < n_stages) stash(smem + ((s + 1) & 1) * STAGE);
        __syncthreads();
    }

#pragma unroll
    for (int bj = 0; bj < BN; ++bj) {
        const int j = j0 + wj + 32 * bj + (lane & 31);
        if (j >= p.N) continue;
        const float bias = p.bias ? p.bias[j] : 0.0f;
#pragma unroll
        for (int bi = 0; bi < BM; ++bi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + wi + 32 * bi + plnerf::frag_row(r, lane);
                if (i >= p.M) continue;
                float v = acc[bi][bj][r] + bias;
                if (p.relu) v = v > 0.0f ? v : 0.0f;
                p.c[(long long)i * p.ldc + j] = v;
            }
    }

    if constexpr (!BF)
        raise_range(reinterpret_cast<unsigned*>(smem), p.status,
                    beyond_half(top_a, PLNERF_RANGE_ACTIVATION) | beyond_half(top_w, PLNERF_RANGE_WEIGHT), tid);
}

}  // namespace

extern "C" int plnerf_gemm_h16(const float* a, int64_t lda, const float* w, int64_t ldw, const float* bias, int M, int N, int K,
                               int relu, int precision, float* c, int64_t ldc, int* status, plnerf_stream_t stream) {
    if (M < 0 || N < 0 || K < 0 || ldc < N || lda < K || ldw < K || !c) return PLNERF_EINVAL;
    if (!is_h16(precision)) return PLNERF_EINVAL;
    if (M == 0 || N == 0) return PLNERF_OK;
    if (K > 0 && (!a || !w)) return PLNERF_EINVAL;
    Gemm16Args p{a, lda, w, ldw, bias, M, N, K, relu ? 1 : 0, c, ldc, reinterpret_cast<unsigned*>(status), 1,
                 vec_rows(a, lda), vec_rows(w, ldw)};
    return with_mode(precision, [&](auto bf, auto ns) {
        return with_tile<decltype(ns)::value, false>(M, N, [&](auto tile) -> int {
            typedef decltype(tile) T;
            const long long tiles_m = ((long long)M + T::TM - 1) / T::TM, tiles_n = ((long long)N + T::TN - 1) / T::TN;
            if (tiles_m * tiles_n > 0x7fffffffLL) return PLNERF_ERANGE;
            p.tiles_n = (int)tiles_n;
            return launch_tile<gemm_h16_kernel<decltype(bf)::value, T>, T>(tiles_m * tiles_n, p, (hipStream_t)stream);
        });
    });
}
