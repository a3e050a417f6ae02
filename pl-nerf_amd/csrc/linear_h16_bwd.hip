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
//
// The one-call training backward (plnerf_generic_train_bwd, include/experimental/plnerf_hip_generic_train.h) runs the same
// kernel with other operand SOURCES (SRC_SAVED, SRC_SAVED_PACKED): the gate from the forward's bit plane instead of the fp32
// y; B -- dgrad's W, wgrad's X where X is a layer's packed output -- from packed planes, a copy where the layered entries
// split (the planes hold what that split makes); and two epilogue options for dgrad: add to what is there (the second of the
// two gradients of the trunk's last activation), and the integer maximum of |dx|'s bit patterns into the word the next
// layer's launch scale is read from.  The MFMA operands, their order and the sums are the layered entries' bit for bit.
#include "generic_net.h"
#include "mlp_layout.h"
#include "../../include/experimental/plnerf_hip_gemm16_bwd.h"
#include "../../include/experimental/plnerf_hip_generic_train.h"

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
    // SRC_SAVED, SRC_SAVED_PACKED (y is not read):
    const unsigned* gate; long long ldgate;      // the gate plane (generic_net.h: gate_ld words per row), or nullptr
    long long b_plane;                  // SRC_SAVED_PACKED: b is the hi plane of packed rows (ldb in elements), lo b_plane bytes on
    int b_pairs;                        // SRC_SAVED_PACKED: b may be read as dwords (4-byte aligned, ldb even)
    int accumulate;                     // dgrad: out += the product
    unsigned* omax;                     // dgrad: atomic max of the bit patterns of |out| as written, or nullptr
};

enum { SRC_ROWS = 0, SRC_SAVED = 1, SRC_SAVED_PACKED = 2 };

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

// One stage of a contraction-strided PACKED operand, fetch_strided's chunks: the four 16-bit elements of a chunk as the two
// dwords store4 would write per plane.  ONES: row `rows` is the ones column, hi = 1 (`one`: its bits), lo = 0 -- what
// split2 makes of 1.0f.  Zeros outside [0, rows) x [0, C).  One address per thread and plane; the chunks' and elements'
// offsets are multiples of ld that are the same for every thread.
template <int T, int NQ, int NS, bool ONES, int NV>
__device__ __forceinline__ void fetch_strided_packed(u32x2 (&v)[NS][NV], const unsigned short* hi, const long long plane_bytes,
                                                     const long long ld, const int r0, const int rows, const int c0, const int C,
                                                     const int tid, const unsigned one) {
    static_assert(THREADS % T == 0 && NQ * THREADS == T * (KS / 4) && NQ <= NV, "a thread keeps its tile row");
    const int r = r0 + tid % T, kc = tid / T, ldi = (int)ld;
    const long long at = ((long long)c0 + 4 * kc) * ld + r;
#pragma unroll
    for (int h = 0; h < NS; ++h) {
        const unsigned short* src = reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(hi) + h * plane_bytes) + at;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = c0 + 4 * (kc + (THREADS / T) * q);
            unsigned e[4] = {0u, 0u, 0u, 0u};
            if (r < rows) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) e[k] = src[(4 * (THREADS / T) * q + k) * ldi];
            } else if (ONES && r == rows && h == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < C) e[k] = one;
            }
            v[h][q] = u32x2{e[0] | e[1] << 16, e[2] | e[3] << 16};
        }
    }
}

// The same stage read as DWORDS, two adjacent tile rows each (`hi` 4-byte aligned, ld even): half the loads.  A thread takes
// the rows 2 (tid % (T / 2)) and + 1 and the chunks tid / (T / 2) + G q: v[h][2 q] is the lower row's chunk, v[h][2 q + 1] the
// upper row's (pairs_at: where they go in the stage).  At the ragged edge (the upper row is the first one outside) the lower
// row is read alone: nothing beyond column `rows` of a packed row is read.
template <int T> struct Pairs {
    static constexpr int HALF = T / 2, G = THREADS / HALF, NQ2 = (HALF * (KS / 4) + THREADS - 1) / THREADS, NQ = 2 * NQ2;
    static_assert(THREADS % HALF == 0 && (G >= KS / 4 ? NQ2 == 1 : G * NQ2 == KS / 4), "the chunks of a row pair");
};
template <int T, int NS, bool ONES, int NV>
__device__ __forceinline__ void fetch_packed_pairs(u32x2 (&v)[NS][NV], const unsigned short* hi, const long long plane_bytes,
                                                   const long long ld, const int r0, const int rows, const int c0, const int C,
                                                   const int tid, const unsigned one) {
    typedef Pairs<T> P;
    static_assert(P::NQ <= NV, "room for both rows' chunks");
    const int r = r0 + 2 * (tid % P::HALF), kc = tid / P::HALF, ldi = (int)ld;
    const bool active = kc < KS / 4;      // (a 32-row tile has more threads than chunks of row pairs)
    const long long at = ((long long)c0 + 4 * kc) * ld + r;
#pragma unroll
    for (int h = 0; h < NS; ++h) {
        const unsigned short* src = reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(hi) + h * plane_bytes) + at;
#pragma unroll
        for (int q = 0; q < P::NQ2; ++q) {
            const int c = c0 + 4 * (kc + P::G * q);
            unsigned d[4] = {0u, 0u, 0u, 0u};      // element c + k of the lower row in the low half, of the upper row in the high half
            if (active) {
                if (r + 1 < rows) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < C) d[k] = *reinterpret_cast<const unsigned*>(src + (4 * P::G * q + k) * ldi);
                } else if (r < rows) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < C) d[k] = src[(4 * P::G * q + k) * ldi] | (ONES && h == 0 ? one << 16 : 0u);
                } else if (ONES && r == rows && h == 0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < C) d[k] = one;
                }
            }
            v[h][2 * q] = u32x2{(d[0] & 0xffffu) | d[1] << 16, (d[2] & 0xffffu) | d[3] << 16};
            v[h][2 * q + 1] = u32x2{d[0] >> 16 | (d[1] & 0xffff0000u), d[2] >> 16 | (d[3] & 0xffff0000u)};
        }
    }
}
// byte offset in a plane of the stage of fetch_packed_pairs' v[.][i], or -1: nothing to store
template <int T>
__device__ __forceinline__ int pairs_at(const int tid, const int i) {
    typedef Pairs<T> P;
    const int kc = tid / P::HALF;
    return kc < KS / 4 ? (2 * (tid % P::HALF) + (i & 1)) * RS + (kc + P::G * (i >> 1)) * 8 : -1;
}

// the four gate bits of a chunk (bit e: element e passes): strided (wgrad: unit r, rows c .. c + 3, one word each; `src` is
// the word of (c, r), `bit` = r & 31) and contiguous (dgrad: row `row`, units c .. c + 3 with c a multiple of four: one
// word).  Zeros outside.
__device__ __forceinline__ unsigned gate_bits_t(const unsigned* src, const int ld, const int bit, const bool inside, const int c,
                                                const int C) {
    unsigned m = 0u;
    if (inside) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < C) m |= ((src[e * ld] >> bit) & 1u) << e;
    }
    return m;
}
__device__ __forceinline__ unsigned gate_bits(const unsigned* gate, const long long ld, const int row, const int rows, const int c,
                                              const int C) {
    return row < rows && c < C ? (gate[(long long)row * ld + (c >> 5)] >> (c & 31)) & 15u : 0u;
}
__device__ __forceinline__ f32x4 gate4_bits(const f32x4 g, const unsigned m, const float scale) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((m >> e) & 1u ? g[e] : 0.0f) * scale;
    return v;
}

// (a NaN in y compares false: gated off)
__device__ __forceinline__ f32x4 gate4(const f32x4 g, const f32x4 y, const float scale) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (y[e] > 0.0f ? g[e] : 0.0f) * scale;
    return v;
}

// WGRAD: A strided, B = [X | 1] strided; else A contiguous, B = W strided.  SRC: the header comment.
template <bool BF, class T, bool WGRAD, int SRC = SRC_ROWS>
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
    f32x4 ra[CA], ry[SRC == SRC_ROWS ? CA : 1], rb[SRC == SRC_SAVED_PACKED ? 1 : CB];
    unsigned rg[SRC == SRC_ROWS ? 1 : CA];                        // the saved gate's bits per chunk
    constexpr int QB = CB > Pairs<TN>::NQ ? CB : Pairs<TN>::NQ;      // (either loader's chunks)
    u32x2 qb[NS][SRC == SRC_SAVED_PACKED ? QB : 1];              // the packed B's dwords per plane and chunk
    unsigned top_a = 0u, top_b = 0u;      // IEEE-half elements: the largest magnitudes split so far (bit patterns)
    const int all_stages = p.C / KS + (p.C % KS != 0);
    const int s_begin = min(split * p.per_split, all_stages), s_end = min(s_begin + p.per_split, all_stages);
    const bool gated = SRC == SRC_ROWS ? p.y != nullptr : p.gate != nullptr;

    // chunk q of a thread, ch = tid + 256 q.  Contiguous operand: row ch >> 3 of the tile, c-elements 4 (ch & 7) .. + 3 of the
    // stage (the forward's).  Strided operand of T rows: row ch % T, c-elements 4 (ch / T) .. + 3.
    auto fetch = [&](const int s) {      // stage s of both operands, global memory -> registers
        const int c0 = s * KS;
        if constexpr (WGRAD) {
            fetch_strided<TM, CA, false>(ra, p.g, p.ldg, i0, p.I, c0, p.C, tid);
            if constexpr (SRC == SRC_ROWS) {
                if (gated) fetch_strided<TM, CA, false>(ry, p.y, p.ldy, i0, p.I, c0, p.C, tid);
            } else if (gated) {
                const int r = i0 + tid % TM, c = c0 + 4 * (tid / TM), ldg = (int)p.ldgate;
                const unsigned* src = p.gate + (long long)c * p.ldgate + (r >> 5);
#pragma unroll
                for (int q = 0; q < CA; ++q)
                    rg[q] = gate_bits_t(src + 4 * (THREADS / TM) * q * ldg, ldg, r & 31, r < p.I, c + 4 * (THREADS / TM) * q, p.C);
            }
        } else {
#pragma unroll
            for (int q = 0; q < CA; ++q) {
                const int ch = tid + THREADS * q;
                ra[q] = load4(p.g, p.ldg, i0 + (ch >> 3), p.I, c0 + 4 * (ch & 7), p.C, p.g_vec);
                if constexpr (SRC == SRC_ROWS) {
                    if (gated) ry[q] = load4(p.y, p.ldy, i0 + (ch >> 3), p.I, c0 + 4 * (ch & 7), p.C, p.y_vec);
                } else if (gated) {
                    rg[q] = gate_bits(p.gate, p.ldgate, i0 + (ch >> 3), p.I, c0 + 4 * (ch & 7), p.C);
                }
            }
        }
        // (wgrad: J = K + 1 and the operand has K columns -- the column one past them is the ones column)
        if constexpr (SRC == SRC_SAVED_PACKED) {
            const unsigned short* b = reinterpret_cast<const unsigned short*>(p.b);
            const unsigned one = BF ? 0x3f80u : 0x3c00u;
            if (p.b_pairs)      // (uniform)
                fetch_packed_pairs<TN, NS, WGRAD>(qb, b, p.b_plane, p.ldb, j0, WGRAD ? p.J - 1 : p.J, c0, p.C, tid, one);
            else
                fetch_strided_packed<TN, CB, NS, WGRAD>(qb, b, p.b_plane, p.ldb, j0, WGRAD ? p.J - 1 : p.J, c0, p.C, tid, one);
        } else
            fetch_strided<TN, CB, WGRAD>(rb, p.b, p.ldb, j0, WGRAD ? p.J - 1 : p.J, c0, p.C, tid);
    };
    auto stash = [&](unsigned char* stage) {      // registers -> the stage's planes: gated, scaled, split
#pragma unroll
        for (int q = 0; q < CA; ++q) {
            const int ch = tid + THREADS * q;
            f32x4 v;
            if constexpr (SRC == SRC_ROWS) v = gated ? gate4(ra[q], ry[q], scale) : ra[q] * scale;
            else v = gated ? gate4_bits(ra[q], rg[q], scale) : ra[q] * scale;
            if constexpr (!BF) clamp4(v, top_a);
            if constexpr (WGRAD) store4<BF, NS>(stage, T::A_PLANE, ch % TM, ch / TM, v);
            else store4<BF, NS>(stage, T::A_PLANE, ch >> 3, ch & 7, v);
        }
        if constexpr (SRC == SRC_SAVED_PACKED) {      // (clamped and split by the pack or the epilogue that wrote the planes)
#pragma unroll
            for (int q = 0; q < (CB > Pairs<TN>::NQ ? CB : Pairs<TN>::NQ); ++q) {
                const int ch = tid + THREADS * q;
                const int at = p.b_pairs ? (q < Pairs<TN>::NQ ? pairs_at<TN>(tid, q) : -1) : q < CB ? (ch % TN) * RS + (ch / TN) * 8 : -1;
                if (at < 0) continue;
#pragma unroll
                for (int h = 0; h < NS; ++h) *reinterpret_cast<u32x2*>(stage + T::B_OFF + h * T::B_PLANE + at) = qb[h][q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < CB; ++q) {
                const int ch = tid + THREADS * q;
                if constexpr (!BF) clamp4(rb[q], top_b);
                store4<BF, NS>(stage + T::B_OFF, T::B_PLANE, ch % TN, ch / TN, rb[q]);
            }
        }
    };
    run_stages<BF, T>(acc, smem, s_begin, s_end, wi, wj, lane, fetch, stash);

    // one launch: the sums times 2^-s; split: this split's tile as it is (reduce_splits applies 2^-s to the total)
    const float unscale = p.k_splits > 1 ? 1.0f : __uint_as_float(plnerf::lay::dzh_unscale_bits(gbits));
    float* out = p.out + (long long)split * p.I * p.J;
    unsigned top_o = 0u;
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
                if constexpr (SRC == SRC_ROWS) {
                    out[(long long)i * p.ldo + j] = acc[bi][bj][r] * unscale;
                } else {
                    // (autograd adds the two gradients of one tensor; an fp32 sum of two terms does not depend on their order)
                    float v = acc[bi][bj][r] * unscale;
                    if (p.accumulate) v += out[(long long)i * p.ldo + j];
                    out[(long long)i * p.ldo + j] = v;
                    const unsigned mag = __float_as_uint(v) & 0x7fffffffu;
                    top_o = mag > top_o ? mag : top_o;
                }
            }
    }
    if constexpr (SRC != SRC_ROWS) {
        // max |out| of this tile, gathered in the dead stages' second dword (run_stages ends behind a barrier; raise_range
        // below uses the first): one global atomic per workgroup at most.  An integer maximum: the same word in any order.
        if (p.omax) {      // (uniform)
            unsigned* wg_max = reinterpret_cast<unsigned*>(smem) + 1;
            if (tid == 0) *wg_max = 0u;
            __syncthreads();
            if (top_o) atomicMax(wg_max, top_o);
            __syncthreads();
            if (tid == 0 && *wg_max) atomicMax(p.omax, *wg_max);
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
template <bool WGRAD, int SRC = SRC_ROWS>
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
            return launch_tile<gemm_h16_bwd_kernel<decltype(bf)::value, T, WGRAD, SRC>, T>(p.tiles * (long long)p.k_splits, p, st);
        });
    });
}

// max |g| over columns [col0, col0 + cols) of g[rows, ld] into *word, as bit patterns (the word zeroed before): what the
// dgrad epilogue gathers for a hidden layer, here for the upstream gradient's columns
__global__ __launch_bounds__(THREADS) void absmax_cols_kernel(const float* __restrict__ g, const long long ld, const int rows,
                                                              const int col0, const int cols, unsigned* word) {
    __shared__ unsigned wg_max;
    if (threadIdx.x == 0) wg_max = 0u;
    __syncthreads();
    unsigned top = 0u;
    const long long total = (long long)rows * cols;
    for (long long at = (long long)blockIdx.x * THREADS + threadIdx.x; at < total; at += (long long)gridDim.x * THREADS) {
        const unsigned mag = __float_as_uint(g[at / cols * ld + col0 + at % cols]) & 0x7fffffffu;
        top = mag > top ? mag : top;
    }
    if (top) atomicMax(&wg_max, top);
    __syncthreads();
    if (threadIdx.x == 0 && wg_max) atomicMax(word, wg_max);
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

extern "C" int plnerf_generic_train_bwd(const plnerf_generic_shape* shape, const float* rows, int64_t ld_rows, int n, int precision,
                                        const void* saved, size_t saved_bytes, const float* g_out, int64_t ld_g, float* const* grads,
                                        void* workspace, size_t workspace_bytes, int* status, plnerf_stream_t stream) {
    Net net;
    int rc = describe(shape, precision, net);
    if (rc != PLNERF_OK) return rc;
    const plnerf_generic_shape* s = shape;
    if (n < 0 || !grads || ld_rows < (int64_t)s->input_ch + s->view_ch || ld_g < net.width_out) return PLNERF_EINVAL;
    for (int l = 0; l < net.n_layers; ++l)
        if (net.runs(l) && !grads[l]) return PLNERF_EINVAL;
    const int planes = planes_of(precision);
    const TrainLayout lay = lay_out_train(net, n, planes);
    if (n > 0) {
        if (!rows || !g_out || !saved || !workspace || ((uintptr_t)saved % PLNERF_GENERIC_WORKSPACE_ALIGN) != 0 ||
            ((uintptr_t)workspace % PLNERF_GENERIC_WORKSPACE_ALIGN) != 0 || saved_bytes < lay.saved_bytes ||
            workspace_bytes < lay.workspace_bytes)
            return PLNERF_EINVAL;
        rc = check_grids(net, n, false);
        if (rc != PLNERF_OK) return rc;
    }
    const hipStream_t st = (hipStream_t)stream;
    const unsigned char* sv = static_cast<const unsigned char*>(saved);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    unsigned* range = reinterpret_cast<unsigned*>(status);
    const int D = s->D, W = s->W, F = net.feature();
    // IEEE-half elements: layer l's launch scale comes from word l, max |g| of the gradient of its output (the bf16 modes: s = 0)
    const bool half = n > 0 && (precision == PLNERF_PREC_F16X3 || precision == PLNERF_PREC_F16);
    unsigned* words = reinterpret_cast<unsigned*>(ws + lay.words);
    auto word = [&](const int l) { return half ? words + l : nullptr; };
    float* const G[2] = {reinterpret_cast<float*>(ws + lay.g[0]), reinterpret_cast<float*>(ws + lay.g[1])};
    float* partials = reinterpret_cast<float*>(ws + lay.partials);
    auto gate = [&](const int l) {
        return n > 0 && lay.gate[l] != TrainLayout::NONE ? reinterpret_cast<const unsigned*>(sv + lay.gate[l]) : nullptr;
    };

    // [dW | db] of layer l from the gradient g of its output and its input x: fp32 rows, or packed planes of n rows
    auto wgrad = [&](const int l, const float* g, const long long ldg, const void* x, const long long ldx, const bool x_packed) {
        int N, K;
        net.dims(l, N, K);
        const int splits = n > 0 ? wgrad_splits(N, K + 1, n) : 1;
        const BwdArgs p{g, ldg, nullptr, 0, static_cast<const float*>(x), ldx, N, K + 1, n, word(l),
                        splits > 1 ? partials : grads[l], (long long)K + 1, range, 1, 1, splits, 0, 0, 0,
                        gate(l), gate_ld(N), (long long)n * ldx * 2, x_packed && ((uintptr_t)x & 3) == 0 && ldx % 2 == 0, 0, nullptr};
        const int e = x_packed ? launch<true, SRC_SAVED_PACKED>(p, precision, st) : launch<true, SRC_SAVED>(p, precision, st);
        if (e != PLNERF_OK || splits == 1) return e;
        const long long reduce_blocks = ((long long)N * ((long long)K + 1) + THREADS - 1) / THREADS;
        hipLaunchKernelGGL(reduce_splits, dim3((unsigned)reduce_blocks), dim3(THREADS), 0, st, partials, splits, N, K + 1, word(l),
                           grads[l], (long long)K + 1);
        PLNERF_CHECK_LAUNCH();
        return (int)PLNERF_OK;
    };
    // columns [koff, koff + cols) of the gradient of layer l's input, into dx (row stride lay.ld_g): stored, or added to what is
    // there; omax: the word of the layer whose output those columns are
    auto dgrad = [&](const int l, const float* g, const long long ldg, const int koff, const int cols, float* dx,
                     const bool accumulate, unsigned* omax) {
        int N, K;
        net.dims(l, N, K);
        const long long ldw = PLNERF_PACK_LD(K);
        const unsigned short* w = reinterpret_cast<const unsigned short*>(sv + lay.weight[l]) + koff;
        const BwdArgs p{g, ldg, nullptr, 0, reinterpret_cast<const float*>(w), ldw, n, cols, N, word(l), dx, lay.ld_g, range, 1, 1, 1, 0,
                        vec_rows(g, ldg), 0, gate(l), gate_ld(N), (long long)N * ldw * 2, ((uintptr_t)w & 3) == 0 && ldw % 2 == 0,
                        accumulate ? 1 : 0, omax};
        return launch<false, SRC_SAVED_PACKED>(p, precision, st);
    };
    auto packed = [&](const int l) { return static_cast<const void*>(sv + lay.act[l]); };
    auto absmax = [&](const int col0, const int cols, unsigned* to) {
        if (!to) return (int)PLNERF_OK;
        const long long blocks = ((long long)n * cols + THREADS - 1) / THREADS;
        hipLaunchKernelGGL(absmax_cols_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(THREADS), 0, st, g_out,
                           (long long)ld_g, n, col0, cols, to);
        PLNERF_CHECK_LAUNCH();
        return (int)PLNERF_OK;
    };
#define TRAIN_TRY(call)              \
    do {                             \
        const int e__ = (call);      \
        if (e__ != PLNERF_OK) return e__; \
    } while (0)

    if (n == 0) {      // no rows: every weight gradient is zeros, and nothing is read
        for (int l = 0; l < net.n_layers; ++l)
            if (net.runs(l)) TRAIN_TRY(wgrad(l, nullptr, 1, nullptr, 1, false));
        return PLNERF_OK;
    }
    if (half && hipMemsetAsync(words, 0, (size_t)net.n_layers * sizeof(unsigned), st) != hipSuccess) return PLNERF_ELAUNCH;

    int cur = 0;      // G[cur]: the gradient of the output of the layer whose turn it is; its dgrad writes G[cur ^ 1]
    if (!s->use_viewdirs) {
        TRAIN_TRY(absmax(0, s->output_ch, word(F)));
        TRAIN_TRY(wgrad(F, g_out, ld_g, packed(D - 1), PLNERF_PACK_LD(W), true));
        TRAIN_TRY(dgrad(F, g_out, ld_g, 0, W, G[cur], false, word(D - 1)));
    } else {
        const int last_view = D + net.views - 1;
        const float* cat_view = reinterpret_cast<const float*>(sv + lay.cat[F]);
        TRAIN_TRY(absmax(0, 3, word(F + 2)));
        TRAIN_TRY(absmax(3, 1, word(F + 1)));
        TRAIN_TRY(wgrad(F + 2, g_out, ld_g, packed(last_view), PLNERF_PACK_LD(W / 2), true));      // rgb_linear
        TRAIN_TRY(dgrad(F + 2, g_out, ld_g, 0, W / 2, G[cur], false, word(last_view)));
        for (int l = last_view; l >= D; --l, cur ^= 1) {
            if (l > D) {
                TRAIN_TRY(wgrad(l, G[cur], lay.ld_g, packed(l - 1), PLNERF_PACK_LD(W / 2), true));
                TRAIN_TRY(dgrad(l, G[cur], lay.ld_g, 0, W / 2, G[cur ^ 1], false, word(l - 1)));
            } else {      // the first view layer reads [feature | view columns]: only the feature columns flow on
                TRAIN_TRY(wgrad(l, G[cur], lay.ld_g, cat_view, lay.ld_cat_view, false));
                TRAIN_TRY(dgrad(l, G[cur], lay.ld_g, 0, W, G[cur ^ 1], false, word(F)));
            }
        }
        // the trunk's last activation feeds feature_linear and alpha_linear: the first gradient is stored, the second added
        TRAIN_TRY(wgrad(F, G[cur], lay.ld_g, packed(D - 1), PLNERF_PACK_LD(W), true));
        TRAIN_TRY(dgrad(F, G[cur], lay.ld_g, 0, W, G[cur ^ 1], false, nullptr));
        cur ^= 1;
        TRAIN_TRY(wgrad(F + 1, g_out + 3, ld_g, packed(D - 1), PLNERF_PACK_LD(W), true));
        TRAIN_TRY(dgrad(F + 1, g_out + 3, ld_g, 0, W, G[cur], true, word(D - 1)));
    }
    for (int l = D - 1; l >= 0; --l, cur ^= 1) {
        if (l == 0) return wgrad(0, G[cur], lay.ld_g, rows, ld_rows, false);      // (nobody reads the gradient of `rows`)
        if (net.skip(l - 1)) {      // the layer reads [encoding | activation]: only the activation columns flow on
            TRAIN_TRY(wgrad(l, G[cur], lay.ld_g, sv + lay.cat[l - 1], lay.ld_cat_trunk, false));
            TRAIN_TRY(dgrad(l, G[cur], lay.ld_g, s->input_ch, W, G[cur ^ 1], false, word(l - 1)));
        } else {
            TRAIN_TRY(wgrad(l, G[cur], lay.ld_g, packed(l - 1), PLNERF_PACK_LD(W), true));
            TRAIN_TRY(dgrad(l, G[cur], lay.ld_g, 0, W, G[cur ^ 1], false, word(l - 1)));
        }
    }
#undef TRAIN_TRY
    return PLNERF_OK;
}
