// Register-resident forward kernel of the 16-bit-operand MFMA MLP (IEEE-half elements: precision modes F16X3 / F16).
//
// Reference: run_network (run_plnerf.py:78-92) = Embedder (run_nerf_helpers.py:24-54) + NeRF.forward (:105-128).
//
// Why a second forward kernel.  The ping-pong kernel (mlp_h16_fwd_pp.inc) keeps the ACTIVATIONS of a 64-row tile in
// LDS and each wave's 32-feature slab of the WEIGHTS in registers: every 64 rows re-fetch all of the network's weight
// fragments from L2 (37 KB per row in split mode, 12 TB/s of L2 reads chip-wide), every layer costs an LDS round
// trip of the activations and two workgroup barriers per half tile, and 160 KB of LDS cap the tile at 64 rows.
// Here the roles are swapped:
//
//   * a wave owns 32 rows for the whole network and keeps their activations in REGISTERS.  With
//     OUT^T[feature][row] = W . X^T the accumulator layout of v_mfma_f32_32x32x16_f16 (lane = row, four consecutive
//     features per register group) IS the next layer's B-operand layout once the k order inside a 16-deep k-step
//     is permuted (bits 2 and 3 of k swapped) -- and the weights' k order is free, so the permutation is folded
//     into the packed weights.  Bias + ReLU + hi/lo split turn 16 accumulator registers into the 16 operand
//     registers of two k-steps, in place: no LDS traffic, no barrier, no other wave involved.
//   * the four waves of a workgroup (one per SIMD, up to 512 registers each) share ONE stream of weight fragments
//     that an LDS-DMA ring (global_load_lds_dwordx4, 4 slots x 32 KB) pulls from L2: 128 rows per fetch instead of
//     64, one barrier per 48 MFMAs whose only job is to hand a landed slot over.
//   * the sigma and rgb heads are folded into the epilogues that hold their inputs in fp32 registers; the saved
//     half planes of the training forward leave straight from the registers, in 32-row tiles of the accumulator
//     layout (SV_LAYOUT_TILED, mlp_layout.h: one contiguous KiB per store instruction); the weight-gradient
//     kernels read that layout as it is.
//
// Per unit (one 32-feature slab x 16 k-steps in split mode) a wave issues 48 MFMAs, 32 ds_read_b128 of weight
// fragments shared by all four waves, and the previous slab's ~45 VALU epilogue; HBM sees pts in, raw (and the saved
// planes) out.
//
// With one wave per SIMD nothing hides an instruction except the MFMA in flight ahead of it, so the stream is kept
// lean on purpose (DESIGN.md section 4.1, each item a measured step): lo halves by v_fma_mix, SGPR-based DMA
// addresses, three opaque LDS base registers so that every DS access is base + immediate, no LDS read whose result
// the next MFMA waits for (accumulator set-up and head weights are requested ahead), no branch and no uncounted store
// in the stream (saved rows are padded to whole workgroup tiles; stores share vmcnt with the weight DMA and are
// counted in the hand-over waits), non-temporal plane stores, accumulators in architectural VGPRs (Makefile).
// (This file is the kernel's body, included by mlp_rr.hip -- packing, dispatch -- and by mlp_rr_inst.hip, one instantiation
// per object: instantiations of 20-30 thousand instructions compile in parallel instead of one after the other.)
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "mlp_internal.h"
#include "mlp_layout.h"
#include "mlp_pack_src.h"
#include "pe_sincos.h"

// RR_BF16 (-DRR_BF16: the bf16 objects of csrc/Makefile): the same kernel on bf16 elements -- fp32's exponent
// range, so no clamp in the forward; the lo halves by shift / subtract / convert (v_fma_mix knows IEEE half only).
// Inference of both modes; the split mode also trains on it: the saved state of every 16-bit mode is IEEE half, so the
// training variant converts every pair a second time, saturating, and remembers the largest magnitude it converted --
// a value beyond the half range raises PLNERF_RANGE_SAVED (the forward result is right, the backward's planes are
// clamped: the guarded Adam step is withheld, plnerf_hip.h).
#ifdef RR_BF16
#define RR_NS plnerf_rr_bf16
#else
#define RR_NS plnerf_rr
#endif
namespace RR_NS {
using namespace plnerf;
using namespace plnerf::lay;

#ifdef RR_BF16
typedef __bf16 H16T;
#else
typedef _Float16 H16T;
#endif
typedef H16T h16x8 __attribute__((ext_vector_type(8)));
typedef H16T h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#ifdef RR_BF16
#define RR_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
#else
#define RR_MFMA __builtin_amdgcn_mfma_f32_32x32x16_f16
#endif
// LDS-space views.  The ring (128 KB) and the head block behind it lie beyond the 64 KB a DS instruction's immediate
// offset reaches; three base registers (ring slots 0-1, slots 2-3, head block), opaque to the optimiser, keep every
// access at "base + immediate" -- left alone, the compiler rebuilds an address with a v_add_u32 per read.
typedef __attribute__((address_space(3))) const unsigned char lds_cbyte;
typedef __attribute__((address_space(3))) const h16x8 lds_h16x8;
typedef __attribute__((address_space(3))) const float lds_cfloat;
typedef __attribute__((address_space(3))) const f32x2 lds_f32x2;
typedef __attribute__((address_space(3))) const f32x4 lds_f32x4;

#ifdef RR_TRACE
#ifndef RR_SINGLE_TU
#error "trace builds are single-translation-unit builds (tools/build_variant.sh)"
#endif
__device__ unsigned long long g_rr_trace[128];     // [0..3] walk begin / end (shader clock, wall clock); [8 + u] start of unit u
#endif

typedef plnerf::impl::RrFwdArgs FwdArgs;      // (mlp_internal.h: shared by the translation units)

namespace {

#ifndef RR_PFD
#define RR_PFD 2
#endif
#ifndef RR_SCHED
#define RR_SCHED 1      // 1: pin the order of every k-step product; 2: only of the products that carry an epilogue chunk; 0: free
#endif
constexpr int HEAD_FLOATS = HB_END - HB;
constexpr size_t HEAD_BYTES = (size_t)HEAD_FLOATS * 4;
constexpr int H_BIAS = HB_BIAS - HB, H_BF = HB_BF - HB, H_BV = HB_BV - HB, H_WA = HB_WA - HB, H_BA = HB_BA - HB,
              H_WR = HB_WR - HB, H_BR = HB_BR - HB;
// largest magnitude the hi + lo pair of halves represents (65504 + 65504 2^-11 ...): activations are clamped to it
constexpr float H16_MAX_SPLIT = 65504.0f;
constexpr int RR_THREADS = 256;     // four waves, one per SIMD
constexpr int RR_ROWS = 128;        // rows per workgroup and row tile (32 per wave)
static_assert(SV_ROW_PAD % (2 * RR_ROWS) == 0, "saved planes are padded to whole workgroup tiles (up to two row tiles per wave)");
constexpr int SLOT_BYTES = 32768;   // one ring slot = one unit's weight fragments
constexpr int NSLOTS = 4;
constexpr int N_LAYERS = 9;         // L0..L7, view layer (= FwdGemmC order: feature_linear is composed into the view layer, mlp_layout.h)
constexpr int LV = GC_VIEWS;        // the view layer's index

// ---- the k order of the register-resident operand ------------------------------------------------------------
// A 16-deep k-step holds, in lane half g, element e: hidden feature 16 s + 8 (e >> 2) + 4 g + (e & 3)  -- where the
// accumulators of slab s / 2 leave it.  Encoding channels are assigned so that each lane half evaluates whole
// frequency bands: xyz (63 channels + 1 pad): lane half g, slot t = 8 s + e in 0..31: t < 30: band 5 g + t / 6,
// function/axis t % 6 (sin x, sin y, sin z, cos x, cos y, cos z, the reference's order); t = 30, 31: x, y | z, pad.
// Direction (27 + 5 pad): slot t in 0..15: t < 12: band 2 g + t / 6; then x, y, z, channel 27 | channels 28..31 (the five
// channels the reference's encoding does not have: zero weights there; a caller-embedded input may use all 32).
// (rr_pe_channel / rr_dpe_channel: mlp_layout.h -- the weight-gradient stage reads the encoding planes in this order too)
// padded input index (the `k` of mlp_pack_src.h's fwd_src) held by k-step s, lane half g, element e of GEMM gm
__host__ __device__ constexpr int rr_k_index(int gm, int s, int g, int e) {
    const int hidden = 8 * (e >> 2) + 4 * g + (e & 3);
    if (gm == GC_L0) return rr_pe_channel(g, 8 * s + e);
    if (gm == GC_L5) return s < 4 ? rr_pe_channel(g, 8 * s + e) : PE_K + 16 * (s - 4) + hidden;
    if (gm == GC_VIEWS) return s < 16 ? 16 * s + hidden : W + rr_dpe_channel(g, 8 * (s - 16) + e);
    return 16 * s + hidden;
}

// ---- packing: same block order as the ping-pong kernel's forward section -- [32-feature slab][k-step][plane]
// [64 lanes x 8 halves] -- with the k order above.  One slab's k-steps are contiguous: a unit is one DMA run.
template <int NS>
__global__ void rr_pack_kernel(ParamPtrs P, unsigned char* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= FWDC_FLOATS / 8) return;
    int g = 0, off = 0;
    while (g < N_FWDC - 1 && idx >= off + fwdc_K[g] * fwdc_N[g] / 8) { off += fwdc_K[g] * fwdc_N[g] / 8; ++g; }
    const int r = idx - off, KS = fwdc_K[g] / 16;
    const int blk = r >> 6, lane = r & 63;
    const int ft = blk / KS, ks = blk - ft * KS;
    const int row = ft * 32 + (lane & 31), gl = lane >> 5;
    h16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = fwdc_src(P, g, rr_k_index(g, ks, gl, e), row);
        hi[e] = (H16T)v;
        lo[e] = (H16T)(v - (float)hi[e]);
    }
    h16x8* dst = reinterpret_cast<h16x8*>(out) + (size_t)off * NS + ((size_t)blk * NS) * 64 + lane;
    dst[0] = hi;
    if (NS == 2) dst[64] = lo;
}

// ---- compile-time schedule: the network as a sequence of units -------------------------------------------------
// A unit = slabs [j0, j0 + nj) x k-steps [k0, k0 + nk) of one GEMM: one contiguous run of the packed weights
// (<= one ring slot), nj * nk k-step products.  Split mode (2 KB per k-step): L0 four slabs per unit, K = 16 layers
// one slab, the two long K ranges (skip layer 20, view layer 18 k-steps) two units per slab.  Plain mode (1 KB):
// L0 four slabs, K = 16 layers two slabs, long K ranges one slab.
struct Unit {
    int layer, j0, nj, k0, nk;
    bool first, last;       // first / last unit of its slabs' K range
};
constexpr int layer_ks(int l) { return fwdc_K[l] / 16; }
constexpr int layer_slabs(int l) { return fwdc_N[l] / 32; }
constexpr int units_per_layer(int ns, int l) {
    const int ks = layer_ks(l), sl = layer_slabs(l);
    if (ks == 4) return 2;
    if (ks == 16) return ns == 2 ? sl : sl / 2;
    return ns == 2 ? 2 * sl : sl;
}
constexpr int n_units(int ns) {
    int n = 0;
    for (int l = 0; l < N_LAYERS; ++l) n += units_per_layer(ns, l);
    return n;
}
constexpr Unit unit_desc(int ns, int u) {
    int l = 0;
    while (u >= units_per_layer(ns, l)) { u -= units_per_layer(ns, l); ++l; }
    const int ks = layer_ks(l);
    if (ks == 4) return Unit{l, u * 4, 4, 0, 4, true, true};
    if (ks == 16) { const int nj = ns == 2 ? 1 : 2; return Unit{l, u * nj, nj, 0, 16, true, true}; }
    if (ns == 1) return Unit{l, u, 1, 0, ks, true, true};
    const int h = ks / 2;
    return Unit{l, u >> 1, 1, (u & 1) * h, (u & 1) ? ks - h : h, (u & 1) == 0, (u & 1) == 1};
}
constexpr int unit_pieces(int ns, const Unit& d) { return d.nj * d.nk * ns; }              // 1 KB DMA pieces
constexpr int unit_elem_off(int ns, const Unit& d) {                                         // halves from the section start
    return (fwdc_off(d.layer) + (d.j0 * layer_ks(d.layer) + d.k0) * 512) * ns;
}
// Pending epilogues: the slabs completed by unit u - 1 get their epilogues in chunks (eight per slab) dealt out over
// the first `window` products of unit u after product 0: chunk c right BEFORE the MFMAs of product
// 1 + c * window / nch.  A chunk writes into k-step 2 j + (i >> 1) of the NEXT layer's operand (behind the 4 encoding
// k-steps in the skip layer); unit u must not read that k-step earlier.  The window is the widest that respects this.
// (rt row tiles per wave: the chunks of a slab's rt tiles follow each other, c = (slab q * rt + tile) * 8 + chunk)
constexpr bool epi_window_ok(int ns, int rt, int u, int window) {
    const Unit d = unit_desc(ns, u), p = unit_desc(ns, u - 1);
    const int nch = 8 * p.nj * rt;
    if (d.layer != p.layer + 1) return true;
    for (int c = 0; c < nch; ++c) {
        const int tc = 1 + c * window / nch, q = c / (8 * rt), i = (c & 7) >> 1;
        const int kr = 2 * (p.j0 + q) + (i >> 1) + (d.layer == 5 ? 4 : 0);
        if (kr >= d.k0 && kr < d.k0 + d.nk && (kr - d.k0) * d.nj < tc) return false;
    }
    return true;
}
constexpr int epi_window(int ns, int rt, int u) {
    const Unit d = unit_desc(ns, u);
    for (int wdw = d.nj * d.nk - 1; wdw >= 1; --wdw)
        if (epi_window_ok(ns, rt, u, wdw)) return wdw;
    return 0;
}
// Vector-memory STORES a wave issues while it runs unit u (training): the pending epilogues of unit u - 1's slabs put
// out two plane fragments per slab and row tile, and the layer's relu-bit row once its last slab is done.  They share the vmcnt counter with the weight DMA, in issue order, so the hand-over wait of
// unit u + 1 has to allow for them on top of the DMA pieces that may still fly.
constexpr int stores_in_unit(int ns, int rt, int u) {
    if (u < 1 || u >= n_units(ns)) return 0;
    const Unit p = unit_desc(ns, u - 1);
    if (!p.last) return 0;
    const bool layer_done = p.j0 + p.nj == layer_slabs(p.layer);
    return 2 * p.nj * rt + (layer_done ? rt : 0);
}
// row tiles (32 rows each) a wave carries through the network: the split mode's two operand planes leave room for one;
// the plain mode takes two, so that every weight fragment fetched from LDS feeds two MFMAs
constexpr int row_tiles(int ns) { return ns == 2 ? 1 : 2; }
constexpr bool schedule_ok(int ns) {
    for (int u = 0; u < n_units(ns); ++u) {
        const Unit d = unit_desc(ns, u);
        if (unit_pieces(ns, d) * 1024 > SLOT_BYTES || d.nj * d.nk < 8) return false;
        if (u > 0 && unit_desc(ns, u - 1).last && epi_window(ns, row_tiles(ns), u) < 1) return false;
    }
    return true;
}
static_assert(schedule_ok(1) && schedule_ok(2), "unit schedule: a unit fits a slot; pending epilogues precede their readers");
constexpr int INIT_AHEAD = 4;
// The accumulators of unit u + 1 are loaded with their biases INIT_AHEAD products before unit u ends (run_step).  Where unit
// u + 1 reuses an accumulator that unit u - 1's pending epilogue still reads during unit u (L0's four-slab units
// followed by L1's slab 0), the epilogue's last chunk on it must come earlier.
constexpr bool init_hoist_ok(int ns) {
    const int rt = row_tiles(ns);
    for (int u = 1; u + 1 < n_units(ns); ++u) {
        const Unit d = unit_desc(ns, u), p = unit_desc(ns, u - 1), n = unit_desc(ns, u + 1);
        if (!p.last || !n.first) continue;
        const int nch = 8 * p.nj * rt, win = epi_window(ns, rt, u), t_init = d.nj * d.nk - INIT_AHEAD;
        for (int sl = n.j0; sl < n.j0 + n.nj; ++sl) {
            if (sl < p.j0 || sl >= p.j0 + p.nj) continue;
            const int c_last = (sl - p.j0 + 1) * 8 * rt - 1;
            if (1 + c_last * win / nch >= t_init) return false;
        }
        for (int sl = n.j0; sl < n.j0 + n.nj; ++sl)          // (and never the running unit's own accumulators)
            if (sl >= d.j0 && sl < d.j0 + d.nj) return false;
    }
    return true;
}
static_assert(init_hoist_ok(1) && init_hoist_ok(2), "hoisted accumulator set-up overwrites a slab that is still in use");


// ---- LDS-DMA: 64 lanes x 16 B from global memory to LDS at a wave-uniform address, not visible to hipcc's wait
// counting (cdna_hip_programming.md section 5.7): completion = the issuing wave's vmcnt, then a barrier.
// (M0 carries the LDS destination; it is compiler-reserved, never allocated to a value, and nothing else in this
// kernel uses it, so it is written in the statement that needs it and not restored.)
// Address = wave-uniform base (an SGPR pair, advanced by scalar adds) + the lane's 16-byte slot (one VGPR for the whole
// kernel): no vector ALU work per piece.
__device__ __forceinline__ void dma_1k(const void* gsrc_uniform, const unsigned lane_off, const unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(gsrc_uniform), "s"(lds_dst)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory"); }

template <int NS, int U>
__device__ __forceinline__ void issue_unit(const FwdArgs& a, const unsigned lds_base, const int wave, const int lane) {
    if constexpr (U < n_units(NS)) {
        constexpr Unit d = unit_desc(NS, U);
        constexpr int NP = unit_pieces(NS, d);
        const unsigned char* src = reinterpret_cast<const unsigned char*>(a.wrr) + (size_t)unit_elem_off(NS, d) * 2;
        const unsigned slot = lds_base + (U % NSLOTS) * SLOT_BYTES;
#pragma unroll
        for (int p = 0; p < (NP + 3) / 4; ++p) {
            const int piece = 4 * p + wave;
            if (4 * p + 3 < NP || piece < NP)        // (the view layer's 18 pieces in plain mode: waves 0, 1 take five)
                dma_1k(src + (size_t)piece * 1024, lane * 16, slot + piece * 1024);
        }
    }
}
// pieces every wave has issued for unit u (a wave may have issued one more: waiting with the smaller count over-waits,
// which is safe)
// piece q (of this wave) of unit U
template <int NS, int U>
__device__ __forceinline__ void issue_piece(const FwdArgs& a, const unsigned lds_base, const int wave, const int lane, const int q) {
    if constexpr (U < n_units(NS)) {
        constexpr Unit d = unit_desc(NS, U);
        constexpr int NP = unit_pieces(NS, d);
        const unsigned char* src = reinterpret_cast<const unsigned char*>(a.wrr) + (size_t)unit_elem_off(NS, d) * 2;
        const unsigned slot = lds_base + (U % NSLOTS) * SLOT_BYTES;
        const int piece = 4 * q + wave;
        if (4 * q + 3 < NP || piece < NP) dma_1k(src + (size_t)piece * 1024, lane * 16, slot + piece * 1024);
    }
}
template <int NS>
constexpr int max_pieces_per_wave(int u) { return u < n_units(NS) ? (unit_pieces(NS, unit_desc(NS, u)) + 3) / 4 : 0; }

template <int NS>
constexpr int pieces_per_wave(int u) { return u < n_units(NS) ? unit_pieces(NS, unit_desc(NS, u)) / 4 : 0; }

// ---- the wave's state ----
template <int NS>
struct Wave {
    h16x8 X[16][NS], Y[16][NS];     // activation operands of two consecutive layers (hi | lo planes)
    h16x8 P[4][NS];                 // the encoding in use: xyz (4 k-steps) or direction (the first 2)
    float px, py, pz, dx, dy, dz;   // the row's position and view direction
    f32x16 acc[8];
    float sig, o0, o1, o2;          // head partials
    f32x2 hw[3];                    // head weights (w_alpha | the three w_rgb rows) of the NEXT epilogue chunk, requested one chunk ahead
    float amax;                     // largest activation magnitude split into halves so far (range check)
    unsigned mw[8];                 // relu bit words of the layer in flight (training)
    h16x8 hvf[1];                   // the view layer's half fragment being assembled (training)
    u32x4 svf[2];                   // bf16 elements, training: the slab's two IEEE-half fragments for the saved planes
    float ud[16];                   // caller-embedded input, and training: this lane's direction slots, kept for the view layer
};

// two fp32 values -> one dword (two halves) of the hi plane (+ one of the lo plane) of an operand fragment
template <int NS>
__device__ __forceinline__ void put_split(h16x8 (&dst)[NS], const int e0, const float v0, const float v1) {
    const f32x2 v = {v0, v1};
    const h16x2 h = __builtin_convertvector(v, h16x2);
    u32x4 d0 = __builtin_bit_cast(u32x4, dst[0]);
    d0[e0 >> 1] = __builtin_bit_cast(unsigned, h);
    dst[0] = __builtin_bit_cast(h16x8, d0);
    if constexpr (NS == 2) {
#ifdef RR_BF16
        const unsigned hb = __builtin_bit_cast(unsigned, h);
        const f32x2 r = {v0 - __uint_as_float(hb << 16), v1 - __uint_as_float(hb & 0xffff0000u)};
        const unsigned l = __builtin_bit_cast(unsigned, __builtin_convertvector(r, h16x2));
#else
        // lo = f16(v - f32(hi)), one v_fma_mix per value: f32(hi) * -1 + v evaluated in fp32 (exact), rounded once to half
        // -- bit-identical to convert / subtract / convert (tools/probes/fma_mix_split_probe.hip), 2 instructions for 5
        unsigned l;
        const unsigned hb = __builtin_bit_cast(unsigned, h);
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(hb), "v"(v0));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(hb), "v"(v1));
#endif
        u32x4 d1 = __builtin_bit_cast(u32x4, dst[1]);
        d1[e0 >> 1] = l;
        dst[1] = __builtin_bit_cast(h16x8, d1);
    }
}

struct PeSinCos { float s, c; };
__device__ __attribute__((noinline)) PeSinCos pe_sincos_far(const float theta) {
    PeSinCos r;
    sincosf(theta, &r.s, &r.c);
    return r;
}

// NB bands starting at band f0 of (x, y, z) -> 6 NB values in the reference's order (sin xyz, cos xyz per band)
template <int NB>
__device__ __forceinline__ void encode_bands(const float x, const float y, const float z, const int f0, float (&v)[6 * NB]) {
    const float co[3] = {x, y, z};
    const float top = ldexpf(1.0f, f0 + NB - 1);
    if (__builtin_expect(fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z)) * top < PE_FAST_LIMIT, 1)) {
        const PeTurns t[3] = {pe_turns(x), pe_turns(y), pe_turns(z)};
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const float sc = ldexpf(1.0f, f0 + k);
#pragma unroll
            for (int d = 0; d < 3; ++d) pe_sincos(t[d], sc, &v[6 * k + d], &v[6 * k + 3 + d]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const float sc = ldexpf(1.0f, f0 + k);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const PeSinCos r = pe_sincos_far(co[d] * sc);
                v[6 * k + d] = r.s; v[6 * k + 3 + d] = r.c;
            }
        }
    }
}

// the 32 xyz-encoding values / 16 direction-encoding values of lane half g, in slot order (rr_pe_channel / rr_dpe_channel)
// (sc: the encoder's input scale -- band arguments are (x * sc) * 2^k, the reference's association, the identity slots x)
__device__ __forceinline__ void xyz_values(const float x, const float y, const float z, const int g, float (&v)[32],
                                           const float sc) {
    float b[30];
    encode_bands<5>(x * sc, y * sc, z * sc, 5 * g, b);
#pragma unroll
    for (int t = 0; t < 30; ++t) v[t] = b[t];
    v[30] = g ? z : x;
    v[31] = g ? 0.0f : y;
}
__device__ __forceinline__ void dir_values(const float x, const float y, const float z, const int g, float (&u)[16],
                                           const float sc) {
    float b[12];
    encode_bands<2>(x * sc, y * sc, z * sc, 2 * g, b);
#pragma unroll
    for (int t = 0; t < 12; ++t) u[t] = b[t];
    u[12] = g ? 0.0f : x; u[13] = g ? 0.0f : y; u[14] = g ? 0.0f : z; u[15] = 0.0f;
}

struct Lane {
    int lane, g, wave, trow, grow;      // trow: row within the tile; grow: global row (clamped)
    int prow;                           // global row, not clamped: < sv_rows(n_rows), the padded row count of the saved planes
    bool rowv;                          // the row exists
    int wrow0, n_rows;                  // first global row of the wave; rows in the launch
    float pe_scale;                     // the in-kernel encoding's input scale (uniform)
    const unsigned char* lds;           // the workgroup's LDS
    const float* hd;                    // head block in LDS
    lds_cbyte* ring01;                  // LDS: ring slots 0, 1 + 16 lane   (opaque bases, see lds_cbyte)
    lds_cbyte* ring23;                  //      ring slots 2, 3 + 16 lane
    lds_cfloat* hdg;                    //      head block + 4 g floats
    size_t N;
};

template <int NS>
__device__ __forceinline__ void encode_xyz(Wave<NS>& w, const Lane& ln) {
    float v[32];
    xyz_values(w.px, w.py, w.pz, ln.g, v, ln.pe_scale);
#pragma unroll
    for (int t = 0; t < 32; t += 2) put_split<NS>(w.P[t >> 3], t & 7, v[t], v[t + 1]);
}
template <int NS>
__device__ __forceinline__ void encode_dir(Wave<NS>& w, const Lane& ln) {
    float u[16];
    dir_values(w.dx, w.dy, w.dz, ln.g, u, ln.pe_scale);
#pragma unroll
    for (int t = 0; t < 16; t += 2) put_split<NS>(w.P[t >> 3], t & 7, u[t], u[t + 1]);
}

// caller-embedded input: the 32 + 16 slot values of this lane (rr_pe_channel / rr_dpe_channel order) are loaded once per
// tile (kernel prologue) -- v[] goes into the operand registers P for L0 AND the skip layer (they stay live in between,
// there is nothing to re-evaluate them from), the direction channels wait in w.ud until the view layer.
template <int NS>
__device__ __forceinline__ void split_xyz(Wave<NS>& w, const float (&v)[32]) {
#pragma unroll
    for (int t = 0; t < 32; t += 2) put_split<NS>(w.P[t >> 3], t & 7, v[t], v[t + 1]);
}
template <int NS>
__device__ __forceinline__ void split_dir(Wave<NS>& w, const float (&u)[16]) {
#pragma unroll
    for (int t = 0; t < 16; t += 2) put_split<NS>(w.P[t >> 3], t & 7, u[t], u[t + 1]);
}

// a half plane of the saved state / its relu-bit plane (mlp_layout.h)
__device__ __forceinline__ _Float16* plane_ptr(const FwdArgs& a, const int p, const size_t N) {
    return reinterpret_cast<_Float16*>(a.saved) + (size_t)p * W * N;
}
__device__ __forceinline__ unsigned char* mask_ptr(const FwdArgs& a, const int p, const size_t N) {
    return reinterpret_cast<unsigned char*>(a.saved) + (size_t)SVC_FLOATS * 2 * N + (size_t)p * (W / 8) * N;
}

// ---- saved half planes (training): SV_LAYOUT_TILED (mlp_layout.h) -- a fragment leaves as the wave's registers hold
// it, one contiguous KiB per store instruction: no transposition, no LDS, two stores per 32-feature slab ----
__device__ __forceinline__ void store_frag_tiled(const u32x4 f, _Float16* tile, const int width, const int j, const int frag,
                                                 const Lane& ln) {
    // Unconditional: the planes' rows are padded to whole workgroup tiles (SV_ROW_PAD, mlp_layout.h), so every wave of
    // every workgroup has a tile -- rows past n_rows land in padding nobody reads.  A store that may or may not be
    // issued could not be counted in the hand-over waits (stores_in_unit), and its branch sat in the MFMA stream.
    // (non-temporal: the backward reads the planes after the whole launch has written 4.2 GB past them; -1 % on the
    // training forward against plain stores, same box)
    __builtin_nontemporal_store(f, reinterpret_cast<u32x4*>(tile + ((size_t)((j * 2 + frag) * 64 + ln.lane)) * 8));
    (void)width;
}

__device__ __forceinline__ unsigned or_halves(const unsigned w) {      // w | (the other lane half's w)
    const u32x2 s = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    return s[0] | s[1];
}
// relu bits of a finished slab, from the slab's two hi-plane operand fragments (every half is f16(relu(x)) >= +0, so
// "x > 0" is "half != 0", the ping-pong kernel's test as well).  Dword q of fragment f holds features
// 16 f + 8 (q >> 1) + 2 (q & 1) + {0, 1} (+ 4 g); min(half, 1) is the bit, pair by pair:
//     sum_q  min_u16x2(d_q, {1, 1}) << (8 (q >> 1) + 2 (q & 1))     low halves at their positions, high halves 16 above
// folded (high part one position up) into 16 bits per fragment, instead of a compare, a select and an OR per value.
__device__ __forceinline__ unsigned relu_half_word(const u32x4 d) {
    const unsigned one = 0x00010001u;
    unsigned acc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        // (the instruction itself: written as __builtin_elementwise_min on a two-short vector, this compiler's lowering
        // -- compares, a byte permute, a multiply -- returned wrong bits; tools/probes/relu_bits_probe.hip checks both)
        unsigned b;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(b) : "v"(d[q]), "v"(one));
        acc |= b << (8 * (q >> 1) + 2 * (q & 1));
    }
    return (acc | ((acc >> 16) << 1)) & 0xFFFFu;
}
// two fp32 values -> one dword of an IEEE-half fragment of the saved planes, saturating (bf16 elements: the operand
// fragments are not IEEE half, and the values have fp32's range)
__device__ __forceinline__ void put_saved_f16(u32x4& frag, const int e0, const float v0, const float v1) {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f32x2 c = {__builtin_amdgcn_fmed3f(v0, -H16_MAX, H16_MAX), __builtin_amdgcn_fmed3f(v1, -H16_MAX, H16_MAX)};
    frag[e0 >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(c, f16x2));
}
__device__ __forceinline__ unsigned relu_word(const u32x4 f0, const u32x4 f1, const Lane& ln) {
    const unsigned bits = relu_half_word(f0) | (relu_half_word(f1) << 16);
    return or_halves(bits << (4 * ln.g));
}

// ---- epilogue of slab j of layer L in eight chunks (chunk c = accumulator registers 2 c, 2 c + 1 = features
// 32 j + 8 i + 4 g + r0, + 1 with i = c >> 1, r0 = 2 (c & 1); bias included): ReLU, operand split into one dword per
// plane of the next layer's k-step 2 j + (i >> 1), head partials, saved plane + relu bits.  A chunk is ~10 VALU:
// with one wave per SIMD about five other instructions hide behind each MFMA (MI355X_MICROARCH.md), so the side work
// of a unit is dealt out in pieces this small, evenly over its k-step products. ----
template <int NS, bool SAVE, int L>
__device__ __forceinline__ void epi_chunk(Wave<NS>& w, const int j, const int c, const FwdArgs& a, const Lane& ln) {
    const f32x16& acc = w.acc[j];
    const int i = c >> 1, r0 = 2 * (c & 1);
    float v[2];
#pragma unroll
    for (int r = 0; r < 2; ++r)      // ReLU and the half range in one v_med3_f32 (a value beyond it would become inf)
#ifdef RR_BF16
        v[r] = fmaxf(acc[4 * i + r0 + r], 0.0f);
#else
        v[r] = __builtin_amdgcn_fmed3f(acc[4 * i + r0 + r], 0.0f, H16_MAX_SPLIT);
#endif
    // (the clamp above keeps the halves finite; how far the activations really went is remembered for the status word)
#ifndef RR_BF16
    w.amax = fmaxf(w.amax, fmaxf(fabsf(acc[4 * i + r0]), fabsf(acc[4 * i + r0 + 1])));
    asm volatile("" : "+v"(w.amax));
#else
    if constexpr (SAVE) {      // (bf16 elements: only what goes into the IEEE-half saved planes can leave a range)
        w.amax = fmaxf(w.amax, fmaxf(fabsf(v[0]), fabsf(v[1])));
        asm volatile("" : "+v"(w.amax));
    }
#endif
    const int f0 = 32 * j + 8 * i + 4 * ln.g + r0;
    // head weights: this chunk's arrive in w.hw (asked for by the previous chunk of this row tile -- an LDS read whose
    // result is needed at once would stall the wave, and with it the MFMA issue, for the LDS latency); ask for the next
    const int jn = c < 7 ? j : j + 1, cn = (c + 1) & 7;
    const int f0n = 32 * jn + 8 * (cn >> 1) + 2 * (cn & 1);      // (without the lane half's 4 g: that is in hdg)
    if constexpr (L == 7) {          // sigma = w_alpha . relu(h7)
        if (j == 0 && c == 0) w.hw[0] = *reinterpret_cast<lds_f32x2*>(ln.hdg + H_WA + (f0 - 4 * ln.g));
        const f32x2 wa = w.hw[0];
        if (jn < W / 32) w.hw[0] = *reinterpret_cast<lds_f32x2*>(ln.hdg + H_WA + f0n);
        w.sig = fmaf(v[0], wa[0], w.sig);
        w.sig = fmaf(v[1], wa[1], w.sig);
        asm volatile("" : "+v"(w.sig));      // (keeps the partial sums here: LLVM otherwise sinks the whole chain to the
                                             // kernel's end and holds every operand live until then)
    }
    if constexpr (L == LV) {         // rgb = W_rgb . relu(hv); training: the hv plane and its relu bits
        if (j == 0 && c == 0) {
#pragma unroll
            for (int o = 0; o < 3; ++o) w.hw[o] = *reinterpret_cast<lds_f32x2*>(ln.hdg + H_WR + o * HV + (f0 - 4 * ln.g));
        }
        const f32x2 w0 = w.hw[0], w1 = w.hw[1], w2 = w.hw[2];
        if (jn < HV / 32) {
#pragma unroll
            for (int o = 0; o < 3; ++o) w.hw[o] = *reinterpret_cast<lds_f32x2*>(ln.hdg + H_WR + o * HV + f0n);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            w.o0 = fmaf(v[r], w0[r], w.o0);
            w.o1 = fmaf(v[r], w1[r], w.o1);
            w.o2 = fmaf(v[r], w2[r], w.o2);
        }
        asm volatile("" : "+v"(w.o0), "+v"(w.o1), "+v"(w.o2));
        if constexpr (SAVE) {
            // relu bits at the lane-half-0 positions; the whole word moves by 4 g once, in the last chunk
            unsigned bits = c == 0 ? 0u : w.mw[j];
            bits |= (v[0] > 0.0f ? 1u << (8 * i + r0) : 0u) | (v[1] > 0.0f ? 1u << (8 * i + r0 + 1) : 0u);
#ifdef RR_BF16
            put_saved_f16(w.svf[0], 4 * (i & 1) + r0, v[0], v[1]);
            const u32x4 hvbits = w.svf[0];
#else
            put_split<1>(w.hvf, 4 * (i & 1) + r0, v[0], v[1]);
            const u32x4 hvbits = __builtin_bit_cast(u32x4, w.hvf[0]);
#endif
            if (c % 4 == 3)
                store_frag_tiled(hvbits, plane_ptr(a, 0, ln.N) + (size_t)SVC_HV_OFF * ln.N + (size_t)ln.wrow0 * HV, HV, j,
                                 i >> 1, ln);
            w.mw[j] = c == 7 ? or_halves(bits << (4 * ln.g)) : bits;
        }
    }
    if constexpr (L < LV) {
        h16x8 (&dst)[NS] = ((L % 2 == 0) ? w.X : w.Y)[2 * j + (i >> 1)];
        put_split<NS>(dst, 4 * (i & 1) + r0, v[0], v[1]);
        if constexpr (SAVE) {
            // the hi plane IS the saved half plane (f16(x)).  relu bits: x > 0 (a compare and a select per value; the
            // word is assembled at the lane-half-0 positions and moves by 4 g once, in the last chunk)
#ifdef RR_BF16
            // (bf16 elements: the saved planes are IEEE half all the same -- a second, saturating conversion per pair)
            put_saved_f16(w.svf[i >> 1], 4 * (i & 1) + r0, v[0], v[1]);
            const u32x4 sv0 = w.svf[0], sv1 = w.svf[1], svc = w.svf[i >> 1];
#else
            const u32x4 sv0 = __builtin_bit_cast(u32x4, ((L % 2 == 0) ? w.X : w.Y)[2 * j][0]);
            const u32x4 sv1 = __builtin_bit_cast(u32x4, ((L % 2 == 0) ? w.X : w.Y)[2 * j + 1][0]);
            const u32x4 svc = __builtin_bit_cast(u32x4, dst[0]);
#endif
            if (c == 7) w.mw[j] = relu_word(sv0, sv1, ln);
            if (c % 4 == 3) store_frag_tiled(svc, plane_ptr(a, L, ln.N) + (size_t)ln.wrow0 * W, W, j, i >> 1, ln);
        }
    }
}

// the layer's relu-bit words -> the row's 32 (view layer: 16) bytes of the mask plane
template <int NS, int L>
__device__ __forceinline__ void store_mask_row(const Wave<NS>& w, const FwdArgs& a, const Lane& ln) {
    if constexpr (L <= 7) {
        unsigned char* row = mask_ptr(a, L, ln.N) + (size_t)ln.prow * (W / 8);      // (padded row: always inside the plane)
        // (element-wise selects: a vector-valued ?: is lowered through a scratch array indexed by g)
        u32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = ln.g ? w.mw[4 + e] : w.mw[e];
        *reinterpret_cast<u32x4*>(row + 16 * ln.g) = q;
    } else if constexpr (L == LV) {
        unsigned char* row = mask_ptr(a, 8, ln.N) + (size_t)ln.prow * (HV / 8);
        u32x2 q;
#pragma unroll
        for (int e = 0; e < 2; ++e) q[e] = ln.g ? w.mw[2 + e] : w.mw[e];
        *reinterpret_cast<u32x2*>(row + 8 * ln.g) = q;
    }
}

template <int NS, int L>
__device__ __forceinline__ void init_acc(Wave<NS>& w, const int j, const Lane& ln) {
    constexpr int boff = L < LV ? H_BIAS + L * W : H_BV;      // (the view layer's slot holds b_c = W_vf b_f + b_v)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x4 b = *reinterpret_cast<lds_f32x4*>(ln.hdg + boff + 32 * j + 8 * i);
#pragma unroll
        for (int r = 0; r < 4; ++r) w.acc[j][4 * i + r] = b[r];
    }
}

// operand fragment of k-step k of layer L
template <int NS, int L>
__device__ __forceinline__ const h16x8 (&b_frag(const Wave<NS>& w, const int k))[NS] {
    if constexpr (L == 0) return w.P[k];
    else if constexpr (L == 5) { if (k < 4) return w.P[k]; return w.X[k - 4]; }
    else if constexpr (L == LV) { if (k < 16) return w.Y[k]; return w.P[k - 16]; }      // (h7, where L7's epilogues left it)
    else if constexpr (L % 2 == 1) return w.X[k];
    else return w.Y[k];
}

// weight fragment (slab sl, k-step kk of the unit in slot `slot`) for this lane
template <int NS>
__device__ __forceinline__ void load_a(h16x8 (&af)[NS], const Lane& ln, const int slot, const int nk,
                                       const int sl, const int kk) {
    lds_cbyte* base = slot < 2 ? ln.ring01 : ln.ring23;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        af[s] = *reinterpret_cast<lds_h16x8*>(base + (slot & 1) * SLOT_BYTES + ((sl * nk + kk) * NS + s) * 1024);
}

constexpr int PFD = RR_PFD;      // weight fragments requested this many k-step products ahead

// Product T of unit U (every index a compile-time constant: nested loops whose bounds depend on an outer loop's
// counter are not reliably unrolled, and a rolled one would index the register arrays dynamically).
template <int NS, int RT, bool SAVE, int U, int T>
__device__ __forceinline__ void run_step(Wave<NS> (&w)[RT], h16x8 (&af)[PFD + 1][NS], const FwdArgs& a, const Lane (&ln)[RT],
                                         const unsigned lds_base) {
    constexpr Unit d = unit_desc(NS, U);
    constexpr int L = d.layer, NSTEP = d.nj * d.nk, SP = 1;
    constexpr bool HAS_NEXT = U + 1 < n_units(NS);
    constexpr bool PEND = U > 0 && unit_desc(NS, U > 0 ? U - 1 : 0).last;
    constexpr Unit pd = unit_desc(NS, U > 0 ? U - 1 : 0);
    constexpr int NCH = PEND ? 8 * pd.nj * RT : 0;
    constexpr int NPC = max_pieces_per_wave<NS>(U + 3);
    constexpr int kk = T / d.nj, sl = T - kk * d.nj;          // (k-step, slab) order: independent accumulators alternate
    if constexpr (T == SP) {
        // my pieces of unit U + 1 have landed; what was issued after them may fly: unit U + 2's pieces and (training) the
        // plane stores of unit U - 1's run, interleaved with them
        wait_vm<pieces_per_wave<NS>(U + 2) + (SAVE ? stores_in_unit(NS, RT, U - 1) : 0)>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    {   // request the fragment of product T + PFD (this unit's, or the next unit's first ones)
        constexpr int tn = T + PFD;
        if constexpr (tn < NSTEP) {
            constexpr int kn = tn / d.nj, sn = tn - kn * d.nj;
            load_a<NS>(af[tn % (PFD + 1)], ln[0], U % NSLOTS, d.nk, sn, kn);
        } else if constexpr (HAS_NEXT) {
            constexpr Unit nd = unit_desc(NS, HAS_NEXT ? U + 1 : U);
            constexpr int t2 = tn - NSTEP, kn = t2 / nd.nj, sn = t2 - kn * nd.nj;
            load_a<NS>(af[tn % (PFD + 1)], ln[0], (U + 1) % NSLOTS, nd.nk, sn, kn);
        }
    }
    if constexpr (PEND && T >= 1) {
        // the chunks of the pending epilogues that belong to this product: 1 + c * WIN / NCH == T
        //   <=>  ceil((T - 1) NCH / WIN) <= c < ceil(T NCH / WIN);   chunk c = (slab * RT + row tile) * 8 + piece
        constexpr int WIN = epi_window(NS, RT, U);
        constexpr int c0r = ((T - 1) * NCH + WIN - 1) / WIN, c1r = (T * NCH + WIN - 1) / WIN;
        constexpr int c0 = c0r < NCH ? c0r : NCH, c1 = c1r < NCH ? c1r : NCH;
#pragma unroll
        for (int c = c0; c < c1; ++c) {
            const int rt = (c >> 3) % RT, q = c / (8 * RT);
            epi_chunk<NS, SAVE, pd.layer>(w[rt], pd.j0 + q, c & 7, a, ln[rt]);
            if constexpr (SAVE) {
                if ((c & 7) == 7 && pd.j0 + q + 1 == layer_slabs(pd.layer)) store_mask_row<NS, pd.layer>(w[rt], a, ln[rt]);
            }
        }
    }
    if constexpr (T > SP) {
        constexpr int q0 = (T - SP - 1) * NPC / (NSTEP - SP - 1), q1 = (T - SP) * NPC / (NSTEP - SP - 1);
#pragma unroll
        for (int q = q0; q < q1; ++q) issue_piece<NS, U + 3>(a, lds_base, ln[0].wave, ln[0].lane, q);
    }
    if constexpr (HAS_NEXT && T == NSTEP - INIT_AHEAD) {
        // the next unit's accumulators start from the biases: the LDS reads go out a few products early, so that its first
        // MFMA does not wait for them (the registers are free: slab j + 1's last use was a whole layer ago)
        constexpr Unit nd = unit_desc(NS, HAS_NEXT ? U + 1 : U);
        if constexpr (nd.first) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int q = 0; q < nd.nj; ++q) init_acc<NS, nd.layer>(w[rt], nd.j0 + q, ln[rt]);
        }
    }
    const h16x8 (&aw)[NS] = af[T % (PFD + 1)];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {          // one weight fragment, RT row tiles
        const h16x8 (&bf)[NS] = b_frag<NS, L>(w[rt], d.k0 + kk);
        f32x16& acc = w[rt].acc[d.j0 + sl];
        acc = RR_MFMA(aw[0], bf[0], acc, 0, 0, 0);
        if constexpr (NS == 2) {
            acc = RR_MFMA(aw[NS - 1], bf[0], acc, 0, 0, 0);
            acc = RR_MFMA(aw[0], bf[NS - 1], acc, 0, 0, 0);
        }
    }
    // keep this order: the scheduler otherwise hoists every LDS read of the region to its top and spills
    if constexpr (RR_SCHED == 1) __builtin_amdgcn_sched_barrier(0);
}

template <int NS, int RT, bool SAVE, int U, int... Ts>
__device__ __forceinline__ void run_steps(Wave<NS> (&w)[RT], h16x8 (&af)[PFD + 1][NS], const FwdArgs& a, const Lane (&ln)[RT],
                                          const unsigned lds_base,
                                          std::integer_sequence<int, Ts...>) {
    (run_step<NS, RT, SAVE, U, Ts>(w, af, a, ln, lds_base), ...);
}

// Unit U: its k-step products in (k-step, slab) order, each on the wave's RT row tiles.  The weight fragments of the
// first PFD products arrive in `carry` (requested by the previous unit); the last PFD products request the next unit's.
// The sync point after the first product hands the NEXT unit's slot over: every wave waits for its own DMA pieces of
// unit U + 1, the barrier makes all pieces visible (and proves that every wave has left unit U - 1, whose slot unit
// U + 3 may now overwrite).  Side work dealt out over the products: the pending epilogues (the slabs completed by the
// previous unit, eight chunks per slab and row tile), the DMA pieces of unit U + 3.
template <int NS, int RT, bool SAVE, bool EMB, int U>
__device__ __forceinline__ void run_unit(Wave<NS> (&w)[RT], h16x8 (&carry)[PFD][NS], const FwdArgs& a, const Lane (&ln)[RT],
                                         const unsigned lds_base) {
    constexpr Unit d = unit_desc(NS, U);
    constexpr int L = d.layer, NSTEP = d.nj * d.nk;
#ifdef RR_TRACE
    if (blockIdx.x == (RR_TRACE) && threadIdx.x == 0) g_rr_trace[8 + U] = clock64();
#endif
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        // (the skip layer's xyz operand: P still holds L0's -- until round 4 the in-kernel encoding was evaluated again
        // here to spare the four operand registers in between: 30 sines / cosines, ~2.4 k cycles of a 143 k-cycle walk;
        // same-box A/B, fine training forward 2209 -> 2152 us, step -1.1 %, results bit-identical)
        if constexpr (d.first && d.j0 == 0 && L == LV) {
            if constexpr (EMB || SAVE) split_dir<NS>(w[rt], w[rt].ud);      // (training: the prologue evaluated them for the saved plane)
            else encode_dir<NS>(w[rt], ln[rt]);
        }
        if constexpr (d.first && U == 0) {      // (every later unit's accumulators are set up inside the unit before it)
#pragma unroll
            for (int sl = 0; sl < d.nj; ++sl) init_acc<NS, L>(w[rt], d.j0 + sl, ln[rt]);
        }
    }
    h16x8 af[PFD + 1][NS];
#pragma unroll
    for (int p = 0; p < PFD; ++p)
#pragma unroll
        for (int s = 0; s < NS; ++s) af[p][s] = carry[p][s];
    __builtin_amdgcn_sched_barrier(0);
    run_steps<NS, RT, SAVE, U>(w, af, a, ln, lds_base, std::make_integer_sequence<int, NSTEP>{});
#pragma unroll
    for (int p = 0; p < PFD; ++p)
#pragma unroll
        for (int s = 0; s < NS; ++s) carry[p][s] = af[(NSTEP + p) % (PFD + 1)][s];
}

template <int NS, int RT, bool SAVE, bool EMB, int U>
__device__ __forceinline__ void run_units(Wave<NS> (&w)[RT], h16x8 (&carry)[PFD][NS], const FwdArgs& a, const Lane (&ln)[RT],
                                          const unsigned lds_base) {
    if constexpr (U < n_units(NS)) {
        run_unit<NS, RT, SAVE, EMB, U>(w, carry, a, ln, lds_base);
        run_units<NS, RT, SAVE, EMB, U + 1>(w, carry, a, ln, lds_base);
    }
}

// the head block comes in by DMA like the weights: 16 pieces of 1 KB (four per wave; the block itself is 12,320 bytes,
// what follows it in the packed buffer rides along unused)
constexpr int HEAD_PIECES = 16;
static_assert(HEAD_PIECES * 1024 >= (int)HEAD_BYTES && HEAD_PIECES % 4 == 0, "head block DMA");
constexpr size_t rr_lds_bytes() { return (size_t)NSLOTS * SLOT_BYTES + (size_t)HEAD_PIECES * 1024; }

// CNT: the counted kernel (the unique-row forward's compact rows, mlp_unique.hip) -- a.n_dev points at the device-side row
// count; everything else, the grid included, is sized by a.n_rows as in the plain kernel.
template <int NS, bool SAVE, bool EMB, bool CNT = false>
__global__ __launch_bounds__(RR_THREADS) void mlp_fwd_rr_kernel(FwdArgs a) {
    constexpr int RT = row_tiles(NS);
    static_assert(!(CNT && EMB), "the counted kernel encodes pts / viewdirs itself");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_byte*)smem;
    float* hd = reinterpret_cast<float*>(smem + (size_t)NSLOTS * SLOT_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * (RR_ROWS * RT);
    lds_cbyte* ring01 = (lds_cbyte*)smem + lane * 16;
    lds_cbyte* ring23 = ring01 + 2 * SLOT_BYTES;
    lds_cfloat* hdg = (lds_cfloat*)hd + 4 * (lane >> 5);
    asm volatile("" : "+v"(ring01));
    asm volatile("" : "+v"(ring23));
    asm volatile("" : "+v"(hdg));
    Lane ln[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        ln[rt].lane = lane; ln[rt].g = lane >> 5; ln[rt].wave = wave;
        ln[rt].trow = (wave * RT + rt) * 32 + (lane & 31);
        ln[rt].rowv = row0 + ln[rt].trow < a.n_rows;
        ln[rt].grow = min(row0 + ln[rt].trow, a.n_rows - 1);
        ln[rt].prow = row0 + ln[rt].trow;
        ln[rt].lds = smem; ln[rt].hd = hd; ln[rt].N = sv_rows((size_t)a.n_rows);
        ln[rt].ring01 = ring01; ln[rt].ring23 = ring23; ln[rt].hdg = hdg;
        ln[rt].wrow0 = row0 + (wave * RT + rt) * 32; ln[rt].n_rows = a.n_rows; ln[rt].pe_scale = a.pe_scale;
    }
#ifdef RR_TRACE
    if (blockIdx.x == (RR_TRACE) && tid == 0) { g_rr_trace[0] = clock64(); g_rr_trace[1] = wall_clock64(); }
#endif
    // The rows' six input floats first, as loads the compiler does not track (it would wait for them with vmcnt(0) and
    // drain the DMA queue behind them); then the head block and the first three units' weights, all by DMA.  One
    // counted wait below covers the inputs: they are older than every DMA piece.
    // (counted kernel: the row count is asked for first, as a scalar load the compiler does not track either, and waited
    // for only after the input loads are out -- their addresses are valid over the whole buffer whatever the count says.
    // Like the input loads' registers, the count's SGPR must not be copied or spilled between the load and the wait below:
    // nothing uses n_dev in between, and the disassembly of the four counted objects (this compiler, gfx950, the
    // Makefile's flags) shows the loaded register untouched up to the s_waitcnt and compared right behind it -- look
    // again after a compiler change, as for the in6 loads.)
    unsigned n_dev = 0u;
    if constexpr (CNT) asm volatile("s_load_dword %0, %1, 0x0" : "=s"(n_dev) : "s"(a.n_dev) : "memory");
    float in6[RT][6];
    float ev[EMB ? RT : 1][32], eu[EMB ? RT : 1][16];      // caller-embedded input: this lane's slot values
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        if constexpr (EMB) {
            // slot (g, t) <- channel rr_pe_channel(g, t) / rr_dpe_channel(g, t) of the row; channels the network does not
            // have (in_ch < 64, view_ch < 32) are read from the row's first element and zeroed after the wait
            const float* row = a.embedded + (size_t)ln[rt].grow * (size_t)(a.in_ch + a.view_ch);
            const int g = ln[rt].g;
#pragma unroll
            for (int t = 0; t < 32; ++t) {
                const int ch = t < 30 ? 3 + 30 * g + t : (t == 30 ? (g ? 2 : 0) : (g ? PE_K - 1 : 1));      // = rr_pe_channel(g, t)
                asm volatile("global_load_dword %0, %1, off" : "=v"(ev[rt][t]) : "v"(row + (ch < a.in_ch ? ch : 0)) : "memory");
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int ch = t < 12 ? 3 + 12 * g + t : (g ? 28 + (t - 12) : (t < 15 ? t - 12 : 27));        // = rr_dpe_channel(g, t)
                asm volatile("global_load_dword %0, %1, off" : "=v"(eu[rt][t]) : "v"(row + (ch < a.view_ch ? a.in_ch + ch : 0)) : "memory");
            }
        } else {
            const float* pp = a.pts + 3 * (size_t)ln[rt].grow;
            const float* pv = a.viewdirs + 3 * (size_t)(ln[rt].grow / a.spr);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                asm volatile("global_load_dword %0, %1, off" : "=v"(in6[rt][c]) : "v"(pp + c) : "memory");
                asm volatile("global_load_dword %0, %1, off" : "=v"(in6[rt][3 + c]) : "v"(pv + c) : "memory");
            }
        }
    }
    if constexpr (CNT) {
        // a workgroup whose first row is at or past the count has no row: gone before any DMA, LDS use or barrier
        // (uniform; the end of the program waits for the input loads in flight)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(n_dev) : : "memory");
        if (row0 >= (int)n_dev) return;
    }
#pragma unroll
    for (int p = 0; p < HEAD_PIECES / 4; ++p)
        dma_1k(reinterpret_cast<const unsigned char*>(a.packed) + (size_t)(4 * p + wave) * 1024, lane * 16,
               lds_base + NSLOTS * SLOT_BYTES + (4 * p + wave) * 1024);
    issue_unit<NS, 0>(a, lds_base, wave, lane);
    issue_unit<NS, 1>(a, lds_base, wave, lane);
    issue_unit<NS, 2>(a, lds_base, wave, lane);
    wait_vm<HEAD_PIECES / 4 + pieces_per_wave<NS>(0) + pieces_per_wave<NS>(1) + pieces_per_wave<NS>(2)>();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {      // (nothing reads them above the wait)
        if constexpr (EMB) {
            const int g = ln[rt].g;
#pragma unroll
            for (int t = 0; t < 32; ++t) {
                asm volatile("" : "+v"(ev[rt][t]));
                const int ch = t < 30 ? 3 + 30 * g + t : (t == 30 ? (g ? 2 : 0) : (g ? PE_K - 1 : 1));
                ev[rt][t] = ch < a.in_ch ? ev[rt][t] : 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                asm volatile("" : "+v"(eu[rt][t]));
                const int ch = t < 12 ? 3 + 12 * g + t : (g ? 28 + (t - 12) : (t < 15 ? t - 12 : 27));
                eu[rt][t] = ch < a.view_ch ? eu[rt][t] : 0.0f;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) asm volatile("" : "+v"(in6[rt][c]));
        }
    }
#ifdef RR_TRACE
    if (blockIdx.x == (RR_TRACE) && tid == 0) g_rr_trace[4] = clock64();
#endif
    Wave<NS> w[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        Wave<NS>& wt = w[rt];
        const Lane& lt = ln[rt];
        wt.sig = wt.o0 = wt.o1 = wt.o2 = wt.amax = 0.0f;
        // ---- this lane's row: position and view direction stay in six registers; the xyz encoding (32 of the 64 channels
        // per lane) is evaluated once, before L0, and its operand registers P live on to the skip layer; the direction
        // encoding (16 of 32 channels per lane) is evaluated before the view layer -- in training once, here, where the
        // saved plane needs it, and kept as 16 values (ud) ----
        if constexpr (EMB) {
            split_xyz<NS>(wt, ev[rt]);
#pragma unroll
            for (int t = 0; t < 16; ++t) wt.ud[t] = eu[rt][t];
        } else {
            wt.px = in6[rt][0]; wt.py = in6[rt][1]; wt.pz = in6[rt][2];
            wt.dx = in6[rt][3]; wt.dy = in6[rt][4]; wt.dz = in6[rt][5];
            if constexpr (!SAVE) encode_xyz<NS>(wt, lt);      // (training: below, from the values the saved plane takes too)
        }
        if constexpr (SAVE) {
            // saved encoding planes (below): the slot values v / u, rounded to half like the operands' hi planes
            float v[32], u[16];
            if constexpr (EMB) {
#pragma unroll
                for (int t = 0; t < 32; ++t) v[t] = ev[rt][t];
#pragma unroll
                for (int t = 0; t < 16; ++t) u[t] = eu[rt][t];
            } else {
                // ONE evaluation of the row's 30 sines / cosines feeds L0's operand registers and the saved plane (left
                // as two calls, the opaque copies of the inputs above kept the compiler from merging them: the training
                // prologue spent 8.2 k cycles here where the inference one spends 2.4 k; clock stamps)
                xyz_values(wt.px, wt.py, wt.pz, lt.g, v, lt.pe_scale);
#pragma unroll
                for (int t = 0; t < 32; t += 2) put_split<NS>(wt.P[t >> 3], t & 7, v[t], v[t + 1]);
                dir_values(wt.dx, wt.dy, wt.dz, lt.g, u, lt.pe_scale);
#pragma unroll
                for (int t = 0; t < 16; ++t) wt.ud[t] = u[t];      // (the view layer's operand is split from these: run_unit)
            }
            // The saved encoding planes leave AS THE OPERAND REGISTERS LIE (round 5): k-step s of a lane = 8 halves = one 16-byte
            // store, a wave's 64 lanes one contiguous KiB -- the TILED layout of mlp_layout.h for a 64- (32-) wide plane whose
            // "column" 16 s + 8 (e >> 2) + 4 g + (e & 3) holds channel rr_pe_channel(g, 8 s + e): the weight-gradient stage
            // reads it with the same transposing LDS reads as every tiled plane and un-permutes the 64 (32) columns of its
            // result.  (Until round 4 the planes were row-major in the reference's channel order: 48 two-byte LDS writes per
            // lane, a fence, and six LDS -> HBM copies per row tile, 2.5 k of the tile walk's 169 k cycles.)
            _Float16* pe_tile = plane_ptr(a, 0, lt.N) + (size_t)SVC_PE_OFF * lt.N + (size_t)lt.wrow0 * PE_K;
            _Float16* dpe_tile = plane_ptr(a, 0, lt.N) + (size_t)SVC_DPE_OFF * lt.N + (size_t)lt.wrow0 * DPE_K;
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                u32x4 f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x2 pr = {v[8 * ks + 2 * q], v[8 * ks + 2 * q + 1]};
                    f[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(pr, f16x2));
                }
                __builtin_nontemporal_store(f, reinterpret_cast<u32x4*>(pe_tile + (size_t)(ks * 64 + lane) * 8));
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x2 pr = {u[8 * ks + 2 * q], u[8 * ks + 2 * q + 1]};
                    f[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(pr, f16x2));
                }
                __builtin_nontemporal_store(f, reinterpret_cast<u32x4*>(dpe_tile + (size_t)(ks * 64 + lane) * 8));
            }
        }
    }
#ifdef RR_TRACE
    if (blockIdx.x == (RR_TRACE) && tid == 0) g_rr_trace[5] = clock64();
#endif
    // unit 0's weights and the head block are in place for everyone
    // (training: the prologue's six encoding-plane stores per row tile were issued after all three units' pieces)
    wait_vm<pieces_per_wave<NS>(1) + pieces_per_wave<NS>(2) + (SAVE ? 6 * RT : 0)>();
    __syncthreads();
#ifdef RR_TRACE
    if (blockIdx.x == (RR_TRACE) && tid == 0) g_rr_trace[6] = clock64();
#endif
    h16x8 carry[PFD][NS];
    {
        constexpr Unit d0 = unit_desc(NS, 0);
#pragma unroll
        for (int p = 0; p < PFD; ++p) load_a<NS>(carry[p], ln[0], 0, d0.nk, p % d0.nj, p / d0.nj);
    }
    run_units<NS, RT, SAVE, EMB, 0>(w, carry, a, ln, lds_base);
    // the last unit's slab epilogues (view layer) and the heads
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        constexpr Unit ld = unit_desc(NS, n_units(NS) - 1);
#pragma unroll
        for (int c = 0; c < 8 * ld.nj; ++c) epi_chunk<NS, SAVE, ld.layer>(w[rt], ld.j0 + (c >> 3), c & 7, a, ln[rt]);
        if constexpr (SAVE) store_mask_row<NS, LV>(w[rt], a, ln[rt]);
    }
#ifdef RR_TRACE
    if (blockIdx.x == (RR_TRACE) && tid == 0) { g_rr_trace[2] = clock64(); g_rr_trace[3] = wall_clock64(); }
#endif
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const Wave<NS>& wt = w[rt];
        const Lane& lt = ln[rt];
        const u32x2 s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(wt.sig), __float_as_uint(wt.sig), false, false);
        const u32x2 s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(wt.o0), __float_as_uint(wt.o0), false, false);
        const u32x2 s2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(wt.o1), __float_as_uint(wt.o1), false, false);
        const u32x2 s3 = __builtin_amdgcn_permlane32_swap(__float_as_uint(wt.o2), __float_as_uint(wt.o2), false, false);
#ifndef RR_BF16
        if (a.status && !(wt.amax <= H16_MAX)) atomicOr(a.status, PLNERF_RANGE_ACTIVATION);   // (rare; sticky until cleared)
#else
        if constexpr (SAVE) {
            if (a.status && !(wt.amax <= H16_MAX)) atomicOr(a.status, PLNERF_RANGE_SAVED);
        }
#endif
        if (lt.g == 0 && lt.rowv) {
            const float sg = (__uint_as_float(s0[0]) + __uint_as_float(s0[1])) + hd[H_BA];
            const float r = (__uint_as_float(s1[0]) + __uint_as_float(s1[1])) + hd[H_BR + 0];
            const float g = (__uint_as_float(s2[0]) + __uint_as_float(s2[1])) + hd[H_BR + 1];
            const float b = (__uint_as_float(s3[0]) + __uint_as_float(s3[1])) + hd[H_BR + 2];
            reinterpret_cast<float4*>(a.raw_out)[row0 + lt.trow] = make_float4(r, g, b, density_activation(sg, a.act_beta));
        }
    }
}

template <int NS, bool SAVE, bool EMB, bool CNT = false>
int launch(const FwdArgs& a, hipStream_t st) {
    const size_t lds = rr_lds_bytes();
    constexpr int ROWS = RR_ROWS * row_tiles(NS);
    if (CNT != (a.n_dev != nullptr)) return PLNERF_EINVAL;
    (void)hipFuncSetAttribute((const void*)mlp_fwd_rr_kernel<NS, SAVE, EMB, CNT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL((mlp_fwd_rr_kernel<NS, SAVE, EMB, CNT>), dim3((a.n_rows + ROWS - 1) / ROWS), dim3(RR_THREADS), lds, st, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

}  // namespace
}  // namespace RR_NS (plnerf_rr | plnerf_rr_bf16)
