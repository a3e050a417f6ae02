// What the split-operand layer GEMMs of the generic route share: the forward (linear_h16.hip) and the two backward products
// (linear_h16_bwd.hip).  The element types with their MFMA, the on-the-fly split x = hi + lo, the four-element loader of a
// contraction-contiguous operand, the IEEE-half clamp and the store into a stage's planes.  Internal: every including file
// gets its own copies.
#pragma once

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

}  // namespace
