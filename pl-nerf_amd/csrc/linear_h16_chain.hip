// The layer-by-layer route's forward as ONE call, without autograd, on 16-bit activation planes
// (include/experimental/plnerf_hip_generic.h): plnerf_pack_h16, the layer kernel on packed operands, plnerf_generic_fwd.
//
// Reference: run_nerf_helpers.py:76-128 builds ANY netdepth / netwidth / skip list / encoding width; linear_h16.hip is one
// such layer in a 16-bit mode's arithmetic with fp32 rows in memory on both sides: every column tile converts its rows of A
// again, every row tile the weights.  Here the split x = hi + lo (clamp4 / split2 of linear_h16_dev.h, the same functions)
// happens ONCE per value: the weights in plnerf_pack_h16 before the first layer, an activation in the epilogue of the layer
// that produces it.  A consumer's loader is then a copy, its MFMA operands are the bits linear_h16.hip's loader would have
// made, k ascends in the same 16-deep steps from 0 -- so the results are plnerf_gemm_h16's bit for bit, and the range bit a
// consumer's loader raised is raised by the producer's epilogue.
//
// The layer kernel is linear_h16.hip's (linear_h16_dev.h: the same Tile, the same two-stage loop) with three choices per
// operand: A from fp32 rows (split in the loader, as there) or from packed planes; W from packed
// planes; C as fp32 rows through ldc (as there) or as packed planes.  A packed operand's loader moves 16 bytes = 8 k-elements
// per load (a 32-deep stage of a row is four such chunks per plane) where the chunk lies inside K, elements on a ragged tail:
// nothing between K and the row stride is read.  The packed epilogue: in the accumulator layout a lane owns one output
// column, so a direct store is 2 bytes per lane; the stages are dead behind the k loop's last barrier and hold a whole hi + lo tile, so the
// halves are staged there (row stride 2 TN + 16 bytes) and leave as 16-byte row chunks, elements on a ragged edge (measured
// against the direct stores: faster in every mode, LABNOTES).
#include "generic_net.h"
#include "../../include/experimental/plnerf_hip_generic_train.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int PACK_CHUNK = 8;      // k-elements per 16-byte chunk of a packed row

// eight consecutive k of one packed row (zeros outside [0, rows) x [0, K)): one 16-byte load where the chunk lies inside K
// (a packed row starts 16-byte aligned and k is a multiple of eight), element loads otherwise
__device__ __forceinline__ u32x4 load8(const unsigned short* plane, const long long ldp, const int row, const int rows,
                                       const int k, const int K) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < rows && k < K) {
        const unsigned short* src = plane + (long long)row * ldp + k;
        if (k + PACK_CHUNK <= K) {
            v = *reinterpret_cast<const u32x4*>(src);
        } else {
#pragma unroll
            for (int e = 0; e < PACK_CHUNK; ++e)
                if (k + e < K) v[e >> 1] |= (unsigned)src[e] << (16 * (e & 1));
        }
    }
    return v;
}

struct ChainArgs {
    const void* a;          // fp32 rows (lda in floats) or the hi plane of packed rows (lda in elements; lo a_plane bytes on)
    long long lda, a_plane;
    const unsigned short* w;      // packed [N, K]: hi plane, row stride ldw elements; lo w_plane bytes on
    long long ldw, w_plane;
    const float* bias;      // [N] or nullptr
    int M, N, K;
    int relu;
    void* c;                // fp32 rows (ldc in floats) or the hi plane of packed rows (ldc in elements; lo c_plane bytes on)
    long long ldc, c_plane;
    unsigned* status;       // or nullptr
    int tiles_n;
    int a_vec;              // fp32 A: its rows may be read 16 bytes at a time
    unsigned* gate;         // GP: the gate plane, row i at gate + i ldgate words (bit j & 31 of word j >> 5: acc + bias > 0)
    long long ldgate;
};

// AP: A is packed; CP: C is packed; GP: the epilogue also writes the gate plane (the training forward's ReLU layers)
template <bool BF, class T, bool AP, bool CP, bool GP = false>
__global__ __launch_bounds__(THREADS) void chain_h16_kernel(const ChainArgs p) {
    constexpr int NS = T::NS, WM = T::WM, BM = T::BM, BN = T::BN;
    typedef typename Elem<BF>::v8 v8;
    constexpr int TM = T::TM, TN = T::TN, A_PLANE = T::A_PLANE, W_PLANE = T::B_PLANE, W_OFF = T::B_OFF, STAGE = T::STAGE;
    constexpr int CA = TM * (KS / 4) / THREADS;                                    // fp32 A: four-k chunks per thread and stage
    constexpr int A_CHUNKS = TM * (KS / PACK_CHUNK), W_CHUNKS = TN * (KS / PACK_CHUNK);      // packed: eight-k chunks per plane
    constexpr int PA = (A_CHUNKS + THREADS - 1) / THREADS, PW = (W_CHUNKS + THREADS - 1) / THREADS;
    static_assert(TM * (KS / 4) % THREADS == 0, "whole chunks per thread");
    constexpr int T_ROW = TN * 2 + 16;      // packed C: bytes per row of the output tile staged in LDS (one plane: TM rows)
    static_assert(NS * TM * T_ROW <= T::LDS && T_ROW % 16 == 0 && TM * (TN / PACK_CHUNK) % THREADS == 0, "the tile fits the stages");
    // two stages and nothing else, as in linear_h16.hip: the range flags are gathered in the stages' first dword
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_m = (int)(blockIdx.x / (unsigned)p.tiles_n), tile_n = (int)(blockIdx.x % (unsigned)p.tiles_n);
    const int i0 = tile_m * TM, j0 = tile_n * TN;
    const int wi = (wave % WM) * BM * 32, wj = (wave / WM) * BN * 32;

    f32x16 acc[BM][BN];
    plnerf::zero_acc(acc);
    f32x4 ra[AP ? 1 : CA];
    u32x4 qa[AP ? NS : 1][PA], qw[NS][PW];
    unsigned top = 0u;      // IEEE-half elements: the largest activation magnitude split here (loader and epilogue), as bits
    const int n_stages = (p.K + KS - 1) / KS;

    // (packed chunk ch of a plane: row ch >> 2 of the tile, k-elements 8 (ch & 3) .. + 7 of the stage)
    auto fetch = [&](const int s) {      // stage s of both operands, global memory -> registers
        const int k0 = s * KS;
        if constexpr (AP) {
#pragma unroll
            for (int h = 0; h < NS; ++h) {
                const unsigned short* plane =
                    reinterpret_cast<const unsigned short*>(static_cast<const unsigned char*>(p.a) + h * p.a_plane);
#pragma unroll
                for (int q = 0; q < PA; ++q) {
                    const int ch = tid + THREADS * q;
                    qa[h][q] = load8(plane, p.lda, i0 + (ch >> 2), ch < A_CHUNKS ? p.M : 0, k0 + PACK_CHUNK * (ch & 3), p.K);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < CA; ++q) {
                const int ch = tid + THREADS * q;
                ra[q] = load4(static_cast<const float*>(p.a), p.lda, i0 + (ch >> 3), p.M, k0 + 4 * (ch & 7), p.K, p.a_vec);
            }
        }
#pragma unroll
        for (int h = 0; h < NS; ++h) {
            const unsigned short* plane =
                reinterpret_cast<const unsigned short*>(reinterpret_cast<const unsigned char*>(p.w) + h * p.w_plane);
#pragma unroll
            for (int q = 0; q < PW; ++q) {
                const int ch = tid + THREADS * q;
                qw[h][q] = load8(plane, p.ldw, j0 + (ch >> 2), ch < W_CHUNKS ? p.N : 0, k0 + PACK_CHUNK * (ch & 3), p.K);
            }
        }
    };
    auto stash = [&](unsigned char* stage) {      // registers -> the stage's planes
        if constexpr (AP) {
#pragma unroll
            for (int h = 0; h < NS; ++h)
#pragma unroll
                for (int q = 0; q < PA; ++q) {
                    const int ch = tid + THREADS * q;
                    if (ch < A_CHUNKS) *reinterpret_cast<u32x4*>(stage + h * A_PLANE + (ch >> 2) * RS + (ch & 3) * 16) = qa[h][q];
                }
        } else {
#pragma unroll
            for (int q = 0; q < CA; ++q) {
                const int ch = tid + THREADS * q;
                if constexpr (!BF) clamp4(ra[q], top);
                store4<BF, NS>(stage, A_PLANE, ch >> 3, ch & 7, ra[q]);
            }
        }
#pragma unroll
        for (int h = 0; h < NS; ++h)
#pragma unroll
            for (int q = 0; q < PW; ++q) {
                const int ch = tid + THREADS * q;
                if (ch < W_CHUNKS) *reinterpret_cast<u32x4*>(stage + W_OFF + h * W_PLANE + (ch >> 2) * RS + (ch & 3) * 16) = qw[h][q];
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
            for (int r = 0; r < 16; r += 2) {      // (rows r and r + 1 of the fragment are adjacent rows of C)
                const int i = i0 + wi + 32 * bi + plnerf::frag_row(r, lane);
                float v0 = acc[bi][bj][r] + bias, v1 = acc[bi][bj][r + 1] + bias;
                if constexpr (GP) {
                    // The backward's gate is the fp32 sign, which the halves do not keep (a positive value below the
                    // element's range packs to zeros).  The 32 lanes of a half-wave hold the 32 columns of one row of the
                    // block (the lanes behind `continue` vote 0; a NaN compares false): one word each, stored by the
                    // lane of the block's first column, which lies inside N whenever any of its columns does.
                    const unsigned long long b0 = __builtin_amdgcn_ballot_w64(v0 > 0.0f), b1 = __builtin_amdgcn_ballot_w64(v1 > 0.0f);
                    if ((lane & 31) == 0) {
                        unsigned* word = p.gate + (long long)i * p.ldgate + (j >> 5);
                        if (i < p.M) word[0] = (unsigned)(b0 >> (lane & 32));
                        if (i + 1 < p.M) word[p.ldgate] = (unsigned)(b1 >> (lane & 32));
                    }
                }
                if (p.relu) {
                    v0 = v0 > 0.0f ? v0 : 0.0f;
                    v1 = v1 > 0.0f ? v1 : 0.0f;
                }
                if constexpr (CP) {
                    // what the consumer's loader did to this value in linear_h16.hip: clamp (noting the magnitude), split
                    // (a row past M holds relu?(bias): not an element of C, and not counted)
                    if constexpr (!BF) {
                        f32x4 t = {v0, v1, 0.0f, 0.0f};
                        if (i >= p.M) t[0] = 0.0f;
                        if (i + 1 >= p.M) t[1] = 0.0f;
                        clamp4(t, top);
                        v0 = t[0];
                        v1 = t[1];
                    }
                    unsigned hi, lo = 0u;
                    split2<BF, NS>(v0, v1, hi, lo);
                    // into the tile staged in the dead stages (rows past M and their garbage stay there)
                    unsigned char* t = smem + (wi + 32 * bi + plnerf::frag_row(r, lane)) * T_ROW + (wj + 32 * bj + (lane & 31)) * 2;
                    *reinterpret_cast<unsigned short*>(t) = (unsigned short)(hi & 0xffffu);
                    *reinterpret_cast<unsigned short*>(t + T_ROW) = (unsigned short)(hi >> 16);
                    if constexpr (NS == 2) {
                        *reinterpret_cast<unsigned short*>(t + TM * T_ROW) = (unsigned short)(lo & 0xffffu);
                        *reinterpret_cast<unsigned short*>(t + TM * T_ROW + T_ROW) = (unsigned short)(lo >> 16);
                    }
                } else {
                    float* c = static_cast<float*>(p.c);
                    if (i < p.M) c[(long long)i * p.ldc + j] = v0;
                    if (i + 1 < p.M) c[(long long)(i + 1) * p.ldc + j] = v1;
                }
            }
    }

    if constexpr (CP) {      // the staged tile -> global memory, 16 bytes = 8 columns of a row per store (uniform)
        __syncthreads();
        constexpr int ROW_CHUNKS = TN / PACK_CHUNK;
#pragma unroll
        for (int h = 0; h < NS; ++h)
#pragma unroll
            for (int q = 0; q < TM * ROW_CHUNKS / THREADS; ++q) {
                const int ch = tid + THREADS * q, row = ch / ROW_CHUNKS, col = (ch % ROW_CHUNKS) * PACK_CHUNK;
                const int i = i0 + row, j = j0 + col;
                if (i >= p.M || j >= p.N) continue;
                const u32x4 v = *reinterpret_cast<const u32x4*>(smem + h * TM * T_ROW + row * T_ROW + col * 2);
                unsigned short* dst = reinterpret_cast<unsigned short*>(static_cast<unsigned char*>(p.c) + h * p.c_plane) +
                                      (long long)i * p.ldc + j;
                if (j + PACK_CHUNK <= p.N) {
                    *reinterpret_cast<u32x4*>(dst) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < PACK_CHUNK; ++e)
                        if (j + e < p.N) dst[e] = (unsigned short)(v[e >> 1] >> (16 * (e & 1)));
                }
            }
        __syncthreads();      // (the range flags below reuse the first dword)
    }
    if constexpr (!BF && (!AP || CP))
        raise_range(reinterpret_cast<unsigned*>(smem), p.status, beyond_half(top, PLNERF_RANGE_ACTIVATION), tid);
}

template <bool BF, int NS, bool AP, bool CP, bool GP = false>
int launch_shape(ChainArgs p, hipStream_t st) {
    return with_tile<NS, false>(p.M, p.N, [&](auto tile) -> int {
        typedef decltype(tile) T;
        const long long tiles_m = ((long long)p.M + T::TM - 1) / T::TM, tiles_n = ((long long)p.N + T::TN - 1) / T::TN;
        if (tiles_m * tiles_n > 0x7fffffffLL) return PLNERF_ERANGE;
        p.tiles_n = (int)tiles_n;
        return launch_tile<chain_h16_kernel<BF, T, AP, CP, GP>, T>(tiles_m * tiles_n, p, st);
    });
}

int launch_layer(const ChainArgs& p, const int precision, const bool a_packed, const bool c_packed, hipStream_t st) {
    return with_mode(precision, [&](auto bf, auto ns) {
        constexpr bool BF = decltype(bf)::value;
        constexpr int NS = decltype(ns)::value;
        if (p.gate) {
            if (a_packed) return c_packed ? launch_shape<BF, NS, true, true, true>(p, st) : launch_shape<BF, NS, true, false, true>(p, st);
            return c_packed ? launch_shape<BF, NS, false, true, true>(p, st) : launch_shape<BF, NS, false, false, true>(p, st);
        }
        if (a_packed) return c_packed ? launch_shape<BF, NS, true, true>(p, st) : launch_shape<BF, NS, true, false>(p, st);
        return c_packed ? launch_shape<BF, NS, false, true>(p, st) : launch_shape<BF, NS, false, false>(p, st);
    });
}

// ---- plnerf_pack_h16: one thread per eight-column chunk of a row
template <bool BF, int NS>
__global__ __launch_bounds__(THREADS) void pack_h16_kernel(const float* __restrict__ src, const long long ld, const int rows,
                                                           const int K, const int vec, unsigned short* __restrict__ dst,
                                                           unsigned* status, const unsigned range_bit) {
    __shared__ unsigned wg_range;
    const int chunks = (K - 1) / PACK_CHUNK + 1;      // per row (K > 0); ldp = 8 chunks
    const long long at = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int row = (int)(at / chunks), k = (int)(at % chunks) * PACK_CHUNK;
    unsigned top = 0u;
    if (row < rows) {
        f32x4 v0 = load4(src, ld, row, rows, k, K, vec), v1 = load4(src, ld, row, rows, k + 4, K, vec);
        if constexpr (!BF) {
            clamp4(v0, top);
            clamp4(v1, top);
        }
        unsigned h[4], l[4] = {0u, 0u, 0u, 0u};
        split2<BF, NS>(v0[0], v0[1], h[0], l[0]);
        split2<BF, NS>(v0[2], v0[3], h[1], l[1]);
        split2<BF, NS>(v1[0], v1[1], h[2], l[2]);
        split2<BF, NS>(v1[2], v1[3], h[3], l[3]);
        const u32x4 hi = {h[0], h[1], h[2], h[3]}, lo = {l[0], l[1], l[2], l[3]};
        const long long ldp = (long long)chunks * PACK_CHUNK;
        unsigned short* d_hi = dst + (long long)row * ldp + k;
        unsigned short* d_lo = d_hi + (long long)rows * ldp;
        if (k + PACK_CHUNK <= K) {
            *reinterpret_cast<u32x4*>(d_hi) = hi;
            if constexpr (NS == 2) *reinterpret_cast<u32x4*>(d_lo) = lo;
        } else {      // (the ragged tail: nothing at or beyond column K is written)
#pragma unroll
            for (int e = 0; e < PACK_CHUNK; ++e)
                if (k + e < K) {
                    d_hi[e] = (unsigned short)(hi[e >> 1] >> (16 * (e & 1)));
                    if constexpr (NS == 2) d_lo[e] = (unsigned short)(lo[e >> 1] >> (16 * (e & 1)));
                }
        }
    }
    if constexpr (!BF) raise_range(&wg_range, status, beyond_half(top, range_bit), threadIdx.x);
}

// ---- the encoding columns into a concatenation's fp32 rows: dst[i, 0 .. cols) = src[i, 0 .. cols)
__global__ __launch_bounds__(THREADS) void copy_cols_kernel(const float* __restrict__ src, const long long lds_, const int rows,
                                                            const int cols, float* __restrict__ dst, const long long ldd) {
    const long long at = (long long)blockIdx.x * THREADS + threadIdx.x;
    const long long row = at / cols;
    const int col = (int)(at % cols);
    if (row < rows) dst[row * ldd + col] = src[row * lds_ + col];
}

int pack_launch(const float* src, const int64_t ld, const int rows, const int K, const int precision, void* dst, unsigned* status,
                const unsigned range_bit, hipStream_t st) {
    const long long groups = ((long long)rows * ((K - 1) / PACK_CHUNK + 1) + THREADS - 1) / THREADS;
    if (groups > 0x7fffffffLL || K > 0x7ffffff0) return PLNERF_ERANGE;      // (K + 7 stays an int)
    const dim3 grid((unsigned)groups), block(THREADS);
    unsigned short* d = static_cast<unsigned short*>(dst);
    const int vec = vec_rows(src, ld);
    with_mode(precision, [&](auto bf, auto ns) {
        hipLaunchKernelGGL((pack_h16_kernel<decltype(bf)::value, decltype(ns)::value>), grid, block, 0, st, src, ld, rows, K,
                           vec, d, status, range_bit);
        return 0;
    });
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

// ---- the network (generic_net.h: Net, describe, weight_offset) and where everything lies in the workspace
struct Layout {
    size_t act[2], cat[2], bytes;      // two packed activation buffers, up to two fp32 concatenation buffers
    long long ld_cat;                  // floats per concatenation row (a multiple of four), 0: none
    int n_cat;
};

Layout lay_out(const Net& net, const int n, const int planes) {
    const plnerf_generic_shape* s = net.s;
    Layout w{};
    size_t off = weight_offset(net, net.n_layers, planes);
    const size_t act = round_up(PLNERF_PACK_BYTES(n, s->W, planes), WS_ALIGN);
    w.act[0] = off;
    w.act[1] = off + act;
    off += 2 * act;
    bool any = false, adjacent = false;
    for (int q = 0; q < s->n_skips; ++q) {
        any = true;
        if (net.skip(s->skips[q] + 1)) adjacent = true;      // (two concatenations in a row: one is read while the other is written)
    }
    long long ld = 0;
    if (any) ld = (long long)s->input_ch + s->W;
    if (s->use_viewdirs && (long long)s->W + s->view_ch > ld) ld = (long long)s->W + s->view_ch;
    w.ld_cat = (ld + 3) / 4 * 4;
    w.n_cat = ld ? (adjacent ? 2 : 1) : 0;
    const size_t cat = round_up((size_t)n * (size_t)w.ld_cat * sizeof(float), WS_ALIGN);
    for (int q = 0; q < w.n_cat; ++q) {
        w.cat[q] = off;
        off += cat;
    }
    w.bytes = off;
    return w;
}

int copy_cols(const float* src, const int64_t ld_src, const int rows, const int cols, float* dst, const long long ldd, hipStream_t st) {
    if (rows == 0 || cols == 0) return PLNERF_OK;
    const long long groups = ((long long)rows * cols + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)groups), dim3(THREADS), 0, st, src, (long long)ld_src, rows, cols, dst, ldd);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

}  // namespace

extern "C" int plnerf_pack_h16(const float* src, int64_t ld, int rows, int K, int precision, void* dst, int* status, int range_bit,
                               plnerf_stream_t stream) {
    if (rows < 0 || K < 0 || ld < K || !is_h16(precision)) return PLNERF_EINVAL;
    if (range_bit != (int)PLNERF_RANGE_ACTIVATION && range_bit != (int)PLNERF_RANGE_WEIGHT) return PLNERF_EINVAL;
    if (rows == 0 || K == 0) return PLNERF_OK;
    if (!src || !dst || !plnerf::aligned16(dst)) return PLNERF_EINVAL;
    return pack_launch(src, ld, rows, K, precision, dst, reinterpret_cast<unsigned*>(status), (unsigned)range_bit, (hipStream_t)stream);
}

extern "C" size_t plnerf_generic_fwd_workspace_bytes(const plnerf_generic_shape* shape, int n, int precision) {
    Net net;
    if (describe(shape, precision, net) != PLNERF_OK || n < 0) return 0;
    return lay_out(net, n, planes_of(precision)).bytes;
}

namespace {

// where a layer's output goes: packed planes [n, N] (ld 0), or the fp32 rows of the concatenation that follows it (ld: their
// stride in floats); the gate plane of a ReLU layer, or nullptr
struct Place {
    void* c;
    long long ld;
    unsigned* gate;
};

// The checks both forwards share, before any launch: PLNERF_OK, or the refusal.
int check_forward(const Net& net, const float* const* params, const int64_t ld_rows, const int n, const int64_t ld_out) {
    const plnerf_generic_shape* s = net.s;
    if (n < 0 || !params || ld_rows < (int64_t)s->input_ch + s->view_ch || ld_out < net.width_out) return PLNERF_EINVAL;
    for (int l = 0; l < net.n_layers; ++l)
        if (net.runs(l) && (!params[2 * l] || !params[2 * l + 1])) return PLNERF_EINVAL;
    return PLNERF_OK;
}

// The weight packs into `weights` (layer l at weight_offset), then every layer: the trunk in order, alpha_linear,
// feature_linear, the view layers, rgb_linear.  place(l) says where layer l's output goes, asked once per hidden layer and
// feature_linear in that order: the no-grad forward alternates two buffers, the training forward keeps every one.
template <class PlaceFn>
int run_layers(const Net& net, const float* const* params, const float* rows, const int64_t ld_rows, const int n, const int precision,
               unsigned char* weights, PlaceFn&& place, float* out, const int64_t ld_out, unsigned* word, hipStream_t st) {
    const plnerf_generic_shape* s = net.s;
    const int planes = planes_of(precision), D = s->D, W = s->W;

    // the weights, once per call
    for (int l = 0; l < net.n_layers; ++l) {
        if (!net.runs(l)) continue;
        int N, K;
        net.dims(l, N, K);
        if (K == 0) continue;
        const int e = pack_launch(params[2 * l], K, N, K, precision, weights + weight_offset(net, l, planes), word, PLNERF_RANGE_WEIGHT, st);
        if (e != PLNERF_OK) return e;
    }

    // one layer: A from fp32 rows (a_packed false) or packed planes of n rows, C likewise
    auto layer = [&](const int l, const void* a, const long long lda, const bool a_packed, const int relu, void* c,
                     const long long ldc, const bool c_packed, unsigned* gate) {
        int N, K;
        net.dims(l, N, K);
        if (N == 0) return (int)PLNERF_OK;
        const long long ldw = PLNERF_PACK_LD(K);
        const ChainArgs p{a, lda, (long long)n * lda * 2, reinterpret_cast<const unsigned short*>(weights + weight_offset(net, l, planes)),
                          ldw, (long long)N * ldw * 2, params[2 * l + 1], n, N, K, relu, c, ldc, (long long)n * ldc * 2, word, 1,
                          a_packed ? 0 : vec_rows(static_cast<const float*>(a), lda), gate, gate_ld(N)};
        return launch_layer(p, precision, a_packed, c_packed, st);
    };

    const void* a = rows;                    // the next layer's input ...
    long long lda = ld_rows;
    bool a_packed = false;                   // ... which the first layer reads in place
    for (int l = 0; l < D; ++l) {
        const Place to = place(l);
        int e;
        if (net.skip(l)) {      // [encoding | this layer] for the next one: fp32, through ldc, beside a copy of the encoding
            float* rows_cat = static_cast<float*>(to.c);
            e = copy_cols(rows, ld_rows, n, s->input_ch, rows_cat, to.ld, st);
            if (e != PLNERF_OK) return e;
            e = layer(l, a, lda, a_packed, 1, rows_cat + s->input_ch, to.ld, false, to.gate);
            a = rows_cat, lda = to.ld, a_packed = false;
        } else {
            e = layer(l, a, lda, a_packed, 1, to.c, PLNERF_PACK_LD(W), true, to.gate);
            a = to.c, lda = PLNERF_PACK_LD(W), a_packed = true;
        }
        if (e != PLNERF_OK) return e;
    }
    // (D - 1 is no skip: the trunk's activation is packed)
    if (!s->use_viewdirs) return layer(net.feature(), a, lda, true, 0, out, ld_out, false, nullptr);
    int e = layer(net.feature() + 1, a, lda, true, 0, out + 3, ld_out, false, nullptr);      // alpha_linear -> column 3
    if (e != PLNERF_OK) return e;
    const Place cat = place(net.feature());
    float* rows_cat = static_cast<float*>(cat.c);
    e = layer(net.feature(), a, lda, true, 0, rows_cat, cat.ld, false, nullptr);      // [feature | view columns]
    if (e != PLNERF_OK) return e;
    e = copy_cols(rows + s->input_ch, ld_rows, n, s->view_ch, rows_cat + W, cat.ld, st);
    if (e != PLNERF_OK) return e;
    a = rows_cat, lda = cat.ld, a_packed = false;
    for (int v = 0; v < net.views; ++v) {
        const Place to = place(D + v);
        e = layer(D + v, a, lda, a_packed, 1, to.c, PLNERF_PACK_LD(W / 2), true, to.gate);
        if (e != PLNERF_OK) return e;
        a = to.c, lda = PLNERF_PACK_LD(W / 2), a_packed = true;
    }
    return layer(net.feature() + 2, a, lda, true, 0, out, ld_out, false, nullptr);      // rgb_linear -> columns 0 .. 2
}

}  // namespace

extern "C" int plnerf_generic_fwd(const plnerf_generic_shape* shape, const float* const* params, const float* rows, int64_t ld_rows,
                                  int n, int precision, void* workspace, size_t workspace_bytes, float* out, int64_t ld_out,
                                  int* status, plnerf_stream_t stream) {
    Net net;
    int rc = describe(shape, precision, net);
    if (rc == PLNERF_OK) rc = check_forward(net, params, ld_rows, n, ld_out);
    if (rc != PLNERF_OK) return rc;
    if (n == 0) return PLNERF_OK;
    const Layout lay = lay_out(net, n, planes_of(precision));
    if (!rows || !out || !workspace || ((uintptr_t)workspace % PLNERF_GENERIC_WORKSPACE_ALIGN) != 0 || workspace_bytes < lay.bytes)
        return PLNERF_EINVAL;
    rc = check_grids(net, n, lay.n_cat != 0);
    if (rc != PLNERF_OK) return rc;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    // two packed buffers and up to two concatenation buffers in turn: a layer never writes the buffer it reads (the view
    // layers reuse the trunk's: feature_linear and alpha_linear are enqueued by then)
    int held = 0, cat = 0;
    auto place = [&](const int l) {
        const int D = net.s->D;
        if (l == net.feature()) return Place{ws + lay.cat[0], lay.ld_cat, nullptr};      // (no trunk layer reads a concatenation any more)
        const bool reads_cat = l > 0 && l < D && net.skip(l - 1);
        if (l < D && net.skip(l)) {
            if (reads_cat) cat ^= (lay.n_cat - 1);      // (this layer READS a concatenation: write the other buffer)
            return Place{ws + lay.cat[cat], lay.ld_cat, nullptr};
        }
        if (l >= D || (l > 0 && !reads_cat)) held ^= 1;      // (this layer READS the packed buffer in use: write the other)
        return Place{ws + lay.act[held], 0, nullptr};
    };
    return run_layers(net, params, rows, ld_rows, n, precision, ws, place, out, ld_out, reinterpret_cast<unsigned*>(status),
                      (hipStream_t)stream);
}

extern "C" size_t plnerf_generic_train_saved_bytes(const plnerf_generic_shape* shape, int n, int precision) {
    Net net;
    if (describe(shape, precision, net) != PLNERF_OK || n < 0) return 0;
    return lay_out_train(net, n, planes_of(precision)).saved_bytes;
}

extern "C" size_t plnerf_generic_train_workspace_bytes(const plnerf_generic_shape* shape, int n, int precision) {
    Net net;
    if (describe(shape, precision, net) != PLNERF_OK || n < 0) return 0;
    return lay_out_train(net, n, planes_of(precision)).workspace_bytes;
}

extern "C" int plnerf_generic_train_wgrad_splits(int N, int K1, int M) { return wgrad_splits(N, K1, M); }

extern "C" int plnerf_generic_train_fwd(const plnerf_generic_shape* shape, const float* const* params, const float* rows,
                                        int64_t ld_rows, int n, int precision, void* saved, size_t saved_bytes, float* out,
                                        int64_t ld_out, int* status, plnerf_stream_t stream) {
    Net net;
    int rc = describe(shape, precision, net);
    if (rc == PLNERF_OK) rc = check_forward(net, params, ld_rows, n, ld_out);
    if (rc != PLNERF_OK) return rc;
    if (n == 0) return PLNERF_OK;
    const TrainLayout lay = lay_out_train(net, n, planes_of(precision));
    if (!rows || !out || !saved || ((uintptr_t)saved % PLNERF_GENERIC_WORKSPACE_ALIGN) != 0 || saved_bytes < lay.saved_bytes)
        return PLNERF_EINVAL;
    rc = check_grids(net, n, net.s->n_skips > 0 || net.s->use_viewdirs);
    if (rc != PLNERF_OK) return rc;
    unsigned char* sv = static_cast<unsigned char*>(saved);
    auto place = [&](const int l) {      // every layer's output in a place of its own: the backward reads them all
        unsigned* gate = lay.gate[l] == TrainLayout::NONE ? nullptr : reinterpret_cast<unsigned*>(sv + lay.gate[l]);
        if (lay.cat[l] != TrainLayout::NONE)
            return Place{sv + lay.cat[l], l == net.feature() ? lay.ld_cat_view : lay.ld_cat_trunk, gate};
        return Place{sv + lay.act[l], 0, gate};
    };
    return run_layers(net, params, rows, ld_rows, n, precision, sv, place, out, ld_out, reinterpret_cast<unsigned*>(status),
                      (hipStream_t)stream);
}
