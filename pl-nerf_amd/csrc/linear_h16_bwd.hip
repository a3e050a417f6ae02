// The two backward products of one nn.Linear of the generic route on the 16-bit MFMAs
// (include/experimental/plnerf_hip_gemm16_bwd.h), in linear_h16.hip's arithmetic and structure:
//   dgrad  dX[M, K]          = gate(G)[M, N] . W[N, K]                 (contraction over n)
//   wgrad  [dW | db][N, K+1] = gate(G)^T[N, M] . [X | 1][M, K + 1]     (contraction over the rows m)
// gate(G) = G where the layer's saved output Y > 0, else 0 (no gate without Y), times 2^s: the launch scale of the fused
// 16-bit backward (mlp_layout.h: dzh_shift of the caller's max |g| word), undone on the sums in the epilogue.
//
// One kernel serves both: an output tile of rows i and columns j, a contraction index c.  Operand A (rows i) is the gated
// gradient, operand B (rows j) is W or [X | 1]; both are split on the fly into hi + lo and stored c-fastest into the stage's
// planes exactly as the forward stores its k, so tile, pipeline and MFMA order are the forward's (linear_h16_dev.h: Tile,
// run_stages).  What differs is where an operand's contraction lies in memory:
//   contiguous (dgrad's gradient: c = n along a row of G): the forward's loader, load4 -- four consecutive c of one row;
//   strided    (dgrad's W, both of wgrad's): the element (row r of the tile, c) lies at base + c ld + r.  A thread takes ONE
//              tile row r and four consecutive c: four dword loads, each coalesced across the wave along r (64 lanes = 256
//              contiguous bytes), which are the four c-consecutive values store4 wants -- the transpose happens on the way
//              into LDS, as one 8-byte store per plane and thread, and costs no LDS pass of its own.
// (The alternative -- halves stored row-major and MFMA fragments built with the transposing LDS reads of mlp_wgrad.hip -- was
// not built; LABNOTES says what was measured.)
//
// Tiles (with_tile): 128 x 128, 128 x 32 when the tile's columns are <= 32 (dgrad with K <= 32; wgrad with K + 1 <= 32) and
// 32 x 128 when wgrad's rows are (the head layers: N = 1, 3, 4).
//
// wgrad's long contraction: k_splits workgroups per tile, split z over the stages [z P, min(S, (z + 1) P)), S = ceil(M / 32),
// P = ceil(S / k_splits); the partial tiles go to `partials` unscaled and reduce_splits adds them in split order.  No
// floating-point atomics anywhere.
//
// Edges: tile rows and columns outside the output and c outside the contraction contribute exact zeros and are never loaded;
// the ones column is the value 1 for c < M, never read.  Range, IEEE-half modes: clamp4 on the scaled gated gradient and on x
// (PLNERF_RANGE_ACTIVATION) and on w (PLNERF_RANGE_WEIGHT), one atomic OR per workgroup at most.
#include "linear_h16_dev.h"
#include "mlp_layout.h"
#include "../../include/experimental/plnerf_hip_gemm16_bwd.h"

namespace {

struct BwdArgs {
    const float* g; long long ldg;
    const float* y; long long ldy;      // y: the gate, or nullptr
    const float* b; long long ldb;      // dgrad: w; wgrad: x
    int I, J, C;                        // output rows, output columns (wgrad: K + 1), contraction length
    const unsigned* gmax;               // max |g| word (fp32 bits), or nullptr
    float* out; long long ldo;          // k_splits > 1: partials, split z at out + z I J
    unsigned* status;                   // or nullptr
    int tiles_j;                        // entry e of the (split, tile) list: split e / tiles, tile t = e % tiles = (t / tiles_j, t % tiles_j)
    int tiles;
    int k_splits, per_split;            // stages per split
    int g_vec, y_vec;                   // dgrad: the rows of g / y may be read 16 bytes at a time
};

// four consecutive c of tile row r of a contraction-strided operand: base[(c + e) ld + r], zeros outside [0, rows) x [0, C).
// ONES: row `rows` (one past the last) is the ones column of [X | 1]: the exact value 1 where c + e < C, no load.
template <bool ONES>
__device__ __forceinline__ f32x4 load4t(const float* base, const long long ld, const int r, const int rows, const int c,
                                        const int C) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r < rows) {
        if (c < C) {
            const float* src = base + (long long)c * ld + r;
            v[0] = src[0];
            if (c + 1 < C) v[1] = src[ld];
            if (c + 2 < C) v[2] = src[2 * ld];
            if (c + 3 < C) v[3] = src[3 * ld];
        }
    } else if (ONES && r == rows) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < C ? 1.0f : 0.0f;
    }
    return v;
}

// One stage of a contraction-strided operand whose tile has T rows: chunk q of thread `tid` is tile row tid % T (the same in
// every chunk: THREADS is a multiple of T) and the four contraction indices from c0 + 4 (tid / T + (THREADS / T) q).  A stage
// that lies inside the contraction whole (uniform) is loaded without a bounds test per element, from one address per thread
// and offsets that are the same for every thread: the per-element tests and 64-bit products of load4t, sixteen times per
// operand, thread and stage, made the loader the bottleneck (wgrad 5.0 ms against 3.7 ms for fp32 -- LABNOTES).
template <int T, int NQ, bool ONES>
__device__ __forceinline__ void fetch_strided(f32x4 (&v)[NQ], const float* base, const long long ld, const int r0, const int rows,
                                              const int c0, const int C, const int tid) {
    static_assert(THREADS % T == 0 && NQ * THREADS == T * (KS / 4), "a thread keeps its tile row");
    const int r = r0 + tid % T, kc = tid / T;
    if (c0 + KS <= C) {
        if (r < rows) {
            const float* src = base + ((long long)c0 + 4 * kc) * ld + r;
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[q][e] = src[(long long)(4 * (THREADS / T) * q + e) * ld];
        } else {
            const float fill = ONES && r == rows ? 1.0f : 0.0f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) v[q] = f32x4{fill, fill, fill, fill};
        }
    } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] = load4t<ONES>(base, ld, r, rows, c0 + 4 * (kc + (THREADS / T) * q), C);
    }
}

// (a NaN in y compares false: gated off)
__device__ __forceinline__ f32x4 gate4(const f32x4 g, const f32x4 y, const float scale) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (y[e] > 0.0f ? g[e] : 0.0f) * scale;
    return v;
}

// WGRAD: A strided, B = [X | 1] strided; else A contiguous, B = W strided.
template <bool BF, class T, bool WGRAD>
__global__ __launch_bounds__(THREADS) void gemm_h16_bwd_kernel(const BwdArgs p) {
    constexpr int NS = T::NS, BM = T::BM, BN = T::BN;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Workgroup ids are dealt round-robin over the eight XCDs, each with an L2 of its own, and the tiles of one split (of one
    // row of tiles in dgrad) read the same rows of the M-sized operands: give each of the eight residue classes of the id a
    // contiguous eighth of the (split, tile) list, so that those tiles meet in one L2.  A bijection of [0, gridDim.x) for any
    // grid size (the first r classes take q + 1 entries, the others q); placement is a matter of speed only.
    const unsigned q = gridDim.x / 8u, r = gridDim.x % 8u, cls = blockIdx.x % 8u;
    const unsigned wg = (cls < r ? cls * (q + 1u) : r * (q + 1u) + (cls - r) * q) + blockIdx.x / 8u;
    const int split = (int)(wg / (unsigned)p.tiles), tile = (int)(wg % (unsigned)p.tiles);
    const int i0 = (tile / p.tiles_j) * T::TM, j0 = (tile % p.tiles_j) * T::TN;
    const int wi = (wave % T::WM) * BM * 32, wj = (wave / T::WM) * BN * 32;

    // (mlp_layout.h: the one derivation of the launch scale; the word is a maximum of absolute values)
    const unsigned gbits = p.gmax ? *p.gmax & 0x7fffffffu : 0u;
    const float scale = __uint_as_float(plnerf::lay::dzh_scale_bits(gbits));

    f32x16 acc[BM][BN];
    plnerf::zero_acc(acc);
    constexpr int TM = T::TM, TN = T::TN;
    constexpr int CA = TM * (KS / 4) / THREADS, CB = TN * (KS / 4) / THREADS;      // four-c chunks per thread and stage
    static_assert(TM * (KS / 4) % THREADS == 0 && TN * (KS / 4) % THREADS == 0, "whole chunks per thread");
    f32x4 ra[CA], ry[CA], rb[CB];
    unsigned top_a = 0u, top_b = 0u;      // IEEE-half elements: the largest magnitudes split so far (bit patterns)
    const int all_stages = p.C / KS + (p.C % KS != 0);
    const int s_begin = min(split * p.per_split, all_stages), s_end = min(s_begin + p.per_split, all_stages);
    const bool gated = p.y != nullptr;

    // chunk q of a thread, ch = tid + 256 q.  Contiguous operand: row ch >> 3 of the tile, c-elements 4 (ch & 7) .. + 3 of the
    // stage (the forward's).  Strided operand of T rows: row ch % T, c-elements 4 (ch / T) .. + 3.
    auto fetch = [&](const int s) {      // stage s of both operands, global memory -> registers
        const int c0 = s * KS;
        if constexpr (WGRAD) {
            fetch_strided<TM, CA, false>(ra, p.g, p.ldg, i0, p.I, c0, p.C, tid);
            if (gated) fetch_strided<TM, CA, false>(ry, p.y, p.ldy, i0, p.I, c0, p.C, tid);
        } else {
#pragma unroll
            for (int q = 0; q < CA; ++q) {
                const int ch = tid + THREADS * q;
                ra[q] = load4(p.g, p.ldg, i0 + (ch >> 3), p.I, c0 + 4 * (ch & 7), p.C, p.g_vec);
                if (gated) ry[q] = load4(p.y, p.ldy, i0 + (ch >> 3), p.I, c0 + 4 * (ch & 7), p.C, p.y_vec);
            }
        }
        // (wgrad: J = K + 1 and the operand has K columns -- the column one past them is the ones column)
        fetch_strided<TN, CB, WGRAD>(rb, p.b, p.ldb, j0, WGRAD ? p.J - 1 : p.J, c0, p.C, tid);
    };
    auto stash = [&](unsigned char* stage) {      // registers -> the stage's planes: gated, scaled, split
#pragma unroll
        for (int q = 0; q < CA; ++q) {
            const int ch = tid + THREADS * q;
            f32x4 v = gated ? gate4(ra[q], ry[q], scale) : ra[q] * scale;
            if constexpr (!BF) clamp4(v, top_a);
            if constexpr (WGRAD) store4<BF, NS>(stage, T::A_PLANE, ch % TM, ch / TM, v);
            else store4<BF, NS>(stage, T::A_PLANE, ch >> 3, ch & 7, v);
        }
#pragma unroll
        for (int q = 0; q < CB; ++q) {
            const int ch = tid + THREADS * q;
            if constexpr (!BF) clamp4(rb[q], top_b);
            store4<BF, NS>(stage + T::B_OFF, T::B_PLANE, ch % TN, ch / TN, rb[q]);
        }
    };
    run_stages<BF, T>(acc, smem, s_begin, s_end, wi, wj, lane, fetch, stash);

    // one launch: the sums times 2^-s; split: this split's tile as it is (reduce_splits applies 2^-s to the total)
    const float unscale = p.k_splits > 1 ? 1.0f : __uint_as_float(plnerf::lay::dzh_unscale_bits(gbits));
    float* out = p.out + (long long)split * p.I * p.J;
#pragma unroll
    for (int bj = 0; bj < BN; ++bj) {
        const int j = j0 + wj + 32 * bj + (lane & 31);
        if (j >= p.J) continue;
#pragma unroll
        for (int bi = 0; bi < BM; ++bi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + wi + 32 * bi + plnerf::frag_row(r, lane);
                if (i >= p.I) continue;
                out[(long long)i * p.ldo + j] = acc[bi][bj][r] * unscale;
            }
    }

    if constexpr (!BF)
        raise_range(reinterpret_cast<unsigned*>(smem), p.status,
                    beyond_half(top_a, PLNERF_RANGE_ACTIVATION) |
                        beyond_half(top_b, WGRAD ? PLNERF_RANGE_ACTIVATION : PLNERF_RANGE_WEIGHT), tid);
}

// dwb[i, j] = 2^-s sum_z partials[z][i, j], z ascending
__global__ __launch_bounds__(THREADS) void reduce_splits(const float* partials, const int k_splits, const int I, const int J,
                                                         const unsigned* gmax, float* out, const long long ldo) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x, n = (long long)I * J;
    if (e >= n) return;
    float sum = partials[e];
    for (int z = 1; z < k_splits; ++z) sum += partials[z * n + e];
    const unsigned gbits = gmax ? *gmax & 0x7fffffffu : 0u;
    out[e / J * ldo + e % J] = sum * __uint_as_float(plnerf::lay::dzh_unscale_bits(gbits));
}

// the (split, tile) list of one product, and its launch
template <bool WGRAD>
int launch(BwdArgs p, const int precision, hipStream_t st) {
    return with_mode(precision, [&](auto bf, auto ns) {
        return with_tile<decltype(ns)::value, WGRAD>(p.I, p.J, [&](auto tile) -> int {
            typedef decltype(tile) T;
            const long long tiles_i = ((long long)p.I + T::TM - 1) / T::TM, tiles_j = ((long long)p.J + T::TN - 1) / T::TN;
            if (tiles_i * tiles_j > 0x7fffffffLL || tiles_i * tiles_j * p.k_splits > 0x7fffffffLL) return PLNERF_ERANGE;
            p.tiles_j = (int)tiles_j;
            p.tiles = (int)(tiles_i * tiles_j);
            const int all_stages = p.C / KS + (p.C % KS != 0);
            p.per_split = (all_stages + p.k_splits - 1) / p.k_splits;
            return launch_tile<gemm_h16_bwd_kernel<decltype(bf)::value, T, WGRAD>, T>(p.tiles * (long long)p.k_splits, p, st);
        });
    });
}

}  // namespace

extern "C" int plnerf_gemm_h16_dgrad(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* w, int64_t ldw,
                                     int M, int N, int K, int precision, const float* g_absmax, float* dx, int64_t lddx,
                                     int* status, plnerf_stream_t stream) {
    if (M < 0 || N < 0 || K < 0 || ldg < N || (y && ldy < N) || ldw < K || lddx < K || !dx) return PLNERF_EINVAL;
    if (!is_h16(precision)) return PLNERF_EINVAL;
    if (M == 0 || K == 0) return PLNERF_OK;
    if (N > 0 && (!g || !w)) return PLNERF_EINVAL;
    const BwdArgs p{g, ldg, y, ldy, w, ldw, M, K, N, reinterpret_cast<const unsigned*>(g_absmax), dx, lddx,
                    reinterpret_cast<unsigned*>(status), 1, 1, 1, 0, vec_rows(g, ldg), y ? vec_rows(y, ldy) : 0};
    return launch<false>(p, precision, (hipStream_t)stream);
}

extern "C" int plnerf_gemm_h16_wgrad(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* x, int64_t ldx,
                                     int M, int N, int K, int precision, const float* g_absmax, float* dwb, int64_t lddwb,
                                     int k_splits, float* partials, int* status, plnerf_stream_t stream) {
    if (M < 0 || N < 0 || K < 0 || ldg < N || (y && ldy < N) || ldx < K || lddwb < (int64_t)K + 1 || !dwb) return PLNERF_EINVAL;
    if (!is_h16(precision)) return PLNERF_EINVAL;
    if (k_splits > 1 && !partials) return PLNERF_EINVAL;
    if (K == 0x7fffffff) return PLNERF_ERANGE;      // (K + 1 columns)
    if (N == 0) return PLNERF_OK;
    if (M > 0 && (!g || (K > 0 && !x))) return PLNERF_EINVAL;
    const int splits = k_splits > 1 && M > 0 ? k_splits : 1;      // (no rows: one launch writes the zeros)
    const hipStream_t st = (hipStream_t)stream;
    const long long cells = (long long)N * ((long long)K + 1), reduce_blocks = (cells + THREADS - 1) / THREADS;
    if (splits > 1 && reduce_blocks > 0x7fffffffLL) return PLNERF_ERANGE;
    const BwdArgs p{g, ldg, y, ldy, x, ldx, N, K + 1, M, reinterpret_cast<const unsigned*>(g_absmax),
                    splits > 1 ? partials : dwb, splits > 1 ? (long long)K + 1 : (long long)lddwb,
                    reinterpret_cast<unsigned*>(status), 1, 1, splits, 0, 0, 0};
    const int rc = launch<true>(p, precision, st);
    if (rc != PLNERF_OK || splits == 1) return rc;
    hipLaunchKernelGGL(reduce_splits, dim3((unsigned)reduce_blocks), dim3(THREADS), 0, st, partials, splits, N, K + 1,
                       reinterpret_cast<const unsigned*>(g_absmax), dwb, (long long)lddwb);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
