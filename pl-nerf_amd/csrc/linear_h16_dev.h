// What the split-operand layer GEMMs of the generic route share: the forward (linear_h16.hip), the two backward products
// (linear_h16_bwd.hip) and the one-call forward on packed planes (linear_h16_chain.hip).
//   device: the element types with their MFMA, the on-the-fly split x = hi + lo, the IEEE-half clamp; Tile, the geometry of a
//           workgroup's tile and of its two stages in LDS; run_stages, the two-stage software pipeline with its MFMA loop and
//           the one description of it; raise_range, the workgroup's range flags into the status word.
//   host:   the 16-bit-mode predicate, the precision and tile-shape dispatches, launch_tile.
// The backward's kernel says how a stage is fetched and stashed and calls run_stages.  The forward's and the chain's carry
// the same loop in their own text: through run_stages (and with their loaders as shared functions or types) their results
// were the same bits, but the compiler laid the code out differently and the IEEE-half forward and chain legs measured about
// 1 % slower in two visits (profiles/generic_tile_ab.txt, LABNOTES); as they stand their assembly is the one they had but for
// the order of the range gather's last instructions.  Internal: every including file gets its own copies.
#pragma once

#include <atomic>
#include <type_traits>

#include "common.h"
#include "mlp_frag.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr float H16_MAX = 65504.0f;
constexpr int KS = 32;                  // k per stage
constexpr int RS = KS * 2 + 16;         // row stride of a plane, bytes
constexpr int THREADS = 256;

template <bool BF> struct Elem;
template <> struct Elem<false> {
    typedef f16x8 v8;
    typedef f16x2 v2;
    static __device__ __forceinline__ f32x16 mfma(const v8 a, const v8 b, const f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x2 widen(const unsigned h) {
        return __builtin_convertvector(__builtin_bit_cast(v2, h), f32x2);
    }
};
template <> struct Elem<true> {
    typedef bf16x8 v8;
    typedef bf16x2 v2;
    static __device__ __forceinline__ f32x16 mfma(const v8 a, const v8 b, const f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x2 widen(const unsigned h) {
        const f32x2 r = {__uint_as_float(h << 16), __uint_as_float(h & 0xffff0000u)};
        return r;
    }
};

// two fp32 values -> one dword of the hi plane (both rounded to nearest even) and one of the lo plane (the residuals, exact in
// fp32, rounded once)
template <bool BF, int NS>
__device__ __forceinline__ void split2(const float v0, const float v1, unsigned& hi, unsigned& lo) {
    typedef typename Elem<BF>::v2 v2;
    const f32x2 v = {v0, v1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, v2));
    if constexpr (NS == 2) {
        // (x - hi is exact in fp32; written as fma(hi, -1, x), the same value, which for IEEE half is one mixed-precision
        // instruction per element: widen, subtract, round)
        const f32x2 h = Elem<BF>::widen(hi);
        const f32x2 r = {__builtin_fmaf(h[0], -1.0f, v0), __builtin_fmaf(h[1], -1.0f, v1)};
        lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, v2));
    }
}

// four consecutive k of one row (zeros outside [0, rows) x [0, K)): one 16-byte load where the whole chunk lies inside K and
// `vec` says the address is aligned, dwords otherwise.  (A loader that keeps each chunk's address through the k loop and
// takes the stages inside K without a branch was measured against this one in the same run, 512 x 512 x 262,144: slower in
// every mode, f16x3 0.96 against 0.76 ms -- LABNOTES.)
__device__ __forceinline__ f32x4 load4(const float* base, const long long ld, const int row, const int rows, const int k,
                                       const int K, const int vec) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row < rows && k < K) {
        const float* src = base + (long long)row * ld + k;
        if (vec && k + 4 <= K) {
            v = *reinterpret_cast<const f32x4*>(src);
        } else {
            v[0] = src[0];
            if (k + 1 < K) v[1] = src[1];
            if (k + 2 < K) v[2] = src[2];
            if (k + 3 < K) v[3] = src[3];
        }
    }
    return v;
}

// IEEE-half elements: a value beyond the half range (or not finite) is clamped to it (a NaN leaves as a finite value); `top`
// keeps the largest magnitude met, as its bit pattern -- an infinity's or a NaN's compares above every finite one's
__device__ __forceinline__ void clamp4(f32x4& v, unsigned& top) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned mag = __float_as_uint(v[e]) & 0x7fffffffu;
        top = mag > top ? mag : top;
        v[e] = fminf(fmaxf(v[e], -H16_MAX), H16_MAX);
    }
}

template <bool BF, int NS>
__device__ __forceinline__ void store4(unsigned char* plane_hi, const int plane_bytes, const int row, const int kc, const f32x4 v) {
    unsigned h0, h1, l0 = 0u, l1 = 0u;
    split2<BF, NS>(v[0], v[1], h0, l0);
    split2<BF, NS>(v[2], v[3], h1, l1);
    unsigned char* dst = plane_hi + row * RS + kc * 8;
    const u32x2 hi = {h0, h1}, lo = {l0, l1};
    *reinterpret_cast<u32x2*>(dst) = hi;
    if constexpr (NS == 2) *reinterpret_cast<u32x2*>(dst + plane_bytes) = lo;
}

// ---- the tile: WM x WN waves, each BM x BN blocks of 32 x 32, and its two stages in dynamic LDS.  A stage is
// A hi | A lo | B hi | B lo (NS == 1: no lo planes), a plane its operand's tile rows at the 80-byte stride.  Nothing static lies
// beside the stages: the split 128 x 128 tile's 81,920 bytes fit a CU's 163,840 exactly twice.
template <int WM_, int WN_, int BM_, int BN_, int NS_>
struct Tile {
    static_assert(WM_ * WN_ == 4, "four waves");
    static constexpr int WM = WM_, WN = WN_, BM = BM_, BN = BN_, NS = NS_;
    static constexpr int TM = WM * BM * 32, TN = WN * BN * 32;
    static constexpr int A_PLANE = TM * RS, B_PLANE = TN * RS;
    static constexpr int B_OFF = NS * A_PLANE, STAGE = NS * (A_PLANE + B_PLANE), LDS = 2 * STAGE;
    static_assert(LDS <= 81920, "two workgroups share a CU");
};

// ---- the pipeline: stages [s_begin, s_end) of the contraction through the two buffers in `smem`, accumulated into this
// wave's blocks (rows from wi, columns from wj of the tile).
//   fetch(s)      loads stage s of both operands into the caller's registers;
//   stash(stage)  writes them to a stage's planes.
// The next stage's global loads are issued before the current stage's MFMAs and land in the other buffer behind them, one
// barrier per stage.  The contraction index ascends in 16-deep steps from the range's start, each step hi.hi, lo.hi, hi.lo
// (the plain modes: hi.hi), whatever the tile: a row's result does not depend on the tile or the launch it sits in.  The
// buffers alternate from the range's start, not from stage 0: a split of the backward may begin at an odd stage.
// Ends behind a barrier, the empty range too: the stages are dead, and what follows may reuse them (raise_range; the chain
// kernel's packed epilogue stages its output tile there).  The forward's and the chain's kernels carry this loop in their own
// text with s_begin = 0 (the header says why): a change here is a change there.
template <bool BF, class T, class Fetch, class Stash>
__device__ __forceinline__ void run_stages(f32x16 (&acc)[T::BM][T::BN], unsigned char* smem, const int s_begin, const int s_end,
                                           const int wi, const int wj, const int lane, Fetch&& fetch, Stash&& stash) {
    typedef typename Elem<BF>::v8 v8;
    constexpr int BM = T::BM, BN = T::BN, NS = T::NS;
    if (s_begin < s_end) {
        fetch(s_begin);
        stash(smem);
    }
    __syncthreads();
    // this lane's operand rows: row (lane & 31) of a block, k-elements 8 (lane >> 5) .. + 7 of a 16-deep step
    const int frag = (lane & 31) * RS + (lane >> 5) * 16;
    for (int s = s_begin; s < s_end; ++s) {
        const unsigned char* cur = smem + ((s - s_begin) & 1) * T::STAGE;
        if (s + 1 < s_end) fetch(s + 1);
#pragma unroll
        for (int ks = 0; ks < KS / 16; ++ks) {
            v8 fa[BM][NS], fb[BN][NS];
#pragma unroll
            for (int b = 0; b < BM; ++b)
#pragma unroll
                for (int h = 0; h < NS; ++h)
                    fa[b][h] = *reinterpret_cast<const v8*>(cur + h * T::A_PLANE + (wi + 32 * b) * RS + frag + ks * 32);
#pragma unroll
            for (int b = 0; b < BN; ++b)
#pragma unroll
                for (int h = 0; h < NS; ++h)
                    fb[b][h] = *reinterpret_cast<const v8*>(cur + T::B_OFF + h * T::B_PLANE + (wj + 32 * b) * RS + frag + ks * 32);
#pragma unroll
            for (int bi = 0; bi < BM; ++bi)
#pragma unroll
                for (int bj = 0; bj < BN; ++bj) {
                    acc[bi][bj] = Elem<BF>::mfma(fa[bi][0], fb[bj][0], acc[bi][bj]);                          // hi . hi
                    if constexpr (NS == 2) {
                        acc[bi][bj] = Elem<BF>::mfma(fa[bi][1], fb[bj][0], acc[bi][bj]);                      // lo . hi
                        acc[bi][bj] = Elem<BF>::mfma(fa[bi][0], fb[bj][1], acc[bi][bj]);                      // hi . lo
                    }
                }
        }
        // (the other buffer's last readers were the previous stage's MFMAs, behind the barrier that ended it)
        if (s + 1 < s_end) stash(smem + ((s + 1 - s_begin) & 1) * T::STAGE);
        __syncthreads();
    }
}

// `bit` where clamp4's largest magnitude lies beyond the IEEE-half range
__device__ __forceinline__ unsigned beyond_half(const unsigned top, const unsigned bit) {
    return top > __float_as_uint(H16_MAX) ? bit : 0u;
}

// This thread's PLNERF_RANGE_* bits -> the status word: gathered in one LDS word, one global atomic OR per workgroup at most,
// none when `status` is NULL.  Uniform: every thread of the workgroup arrives.  The tile kernels keep nothing in LDS beside
// the stages and gather in the stages' first dword: only behind the stage loop's last barrier, or one of their own.
__device__ __forceinline__ void raise_range(unsigned* wg_range, unsigned* status, const unsigned range, const int tid) {
    if (!status) return;
    if (tid == 0) *wg_range = 0u;
    __syncthreads();
    if (range) atomicOr(wg_range, range);
    __syncthreads();
    if (tid == 0 && *wg_range) atomicOr(status, *wg_range);
}

// ---- host side
inline bool is_h16(const int precision) {
    return precision == PLNERF_PREC_BF16X3 || precision == PLNERF_PREC_BF16 || precision == PLNERF_PREC_F16X3 ||
           precision == PLNERF_PREC_F16;
}
inline int planes_of(const int precision) { return precision == PLNERF_PREC_BF16X3 || precision == PLNERF_PREC_F16X3 ? 2 : 1; }
// (an operand whose rows a thread may read 16 bytes at a time: the chunks start at multiples of four k)
inline int vec_rows(const float* base, const int64_t ld) { return plnerf::aligned16(base) && ld % 4 == 0 ? 1 : 0; }

// f(BF, NS) as two std::integral_constants for a 16-bit mode (is_h16 holds: the caller has refused every other value)
template <class F>
int with_mode(const int precision, F&& f) {
    typedef std::integral_constant<int, 1> one;
    typedef std::integral_constant<int, 2> two;
    switch (precision) {
        case PLNERF_PREC_BF16X3: return f(std::true_type{}, two{});
        case PLNERF_PREC_BF16: return f(std::true_type{}, one{});
        case PLNERF_PREC_F16X3: return f(std::false_type{}, two{});
        default: return f(std::false_type{}, one{});
    }
}

// f(Tile) for an output of rows x cols: 128 x 128 as 2 x 2 waves of 2 x 2 blocks; 128 x 32, four waves of one block each,
// where there are at most 32 columns (the one- and three-column head layers would otherwise spend 127 / 128 of a tile on
// padding); SHORT (wgrad alone, whose rows are a head layer's outputs): 32 x 128 where there are at most 32 rows.
template <int NS, bool SHORT, class F>
int with_tile(const int rows, const int cols, F&& f) {
    if constexpr (SHORT)
        if (rows <= 32) return f(Tile<1, 4, 1, 1, NS>{});
    return cols <= 32 ? f(Tile<4, 1, 1, 1, NS>{}) : f(Tile<2, 2, 2, 2, NS>{});
}

// Kernel<<<grid, 256, T::LDS>>>(p).  Beyond 64 KiB of dynamic LDS a kernel has to be told: once per instantiation (the static
// is this function's, and Kernel is among its template arguments) and device, not per layer and chunk.
template <auto Kernel, class T, class Args>
int launch_tile(const long long grid, const Args& p, hipStream_t st) {
    if (T::LDS > 64 * 1024) {
        static std::atomic<unsigned long long> raised{0ull};
        int device = 0;
        if (hipGetDevice(&device) != hipSuccess) return PLNERF_ELAUNCH;
        const unsigned long long bit = 1ull << (device & 63);
        if (!(raised.load(std::memory_order_relaxed) & bit)) {
            if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, T::LDS) != hipSuccess)
                return PLNERF_ELAUNCH;
            raised.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(THREADS), T::LDS, st, p);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

}  // namespace
