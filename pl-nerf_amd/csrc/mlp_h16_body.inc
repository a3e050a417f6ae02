// Body of the 16-bit-operand MFMA MLP kernels, compiled once per element type (see mlp_h16.hip):
//   H16T     element type (__bf16 or _Float16)      H16_MFMA  the matching 32x32x16 MFMA builtin
typedef H16T bf16x8 __attribute__((ext_vector_type(8)));
typedef H16T bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int HEAD_FLOATS = HB_END - HB;            // biases + sigma/rgb rows, fp32, first in the pack
constexpr size_t HEAD_BYTES = (size_t)HEAD_FLOATS * 4;
constexpr int BLDA = 264;   // bf16 elements per activation row (256 + 8): 528 B
constexpr int BLDP = 72;    // xyz-encoding row (64 + 8)
constexpr int BLDD = 40;    // direction-encoding row (32 + 8)
constexpr int NTHREADS = 512;

// PLNERF_TRACE=<block>: wave 0 of that workgroup stamps the shader clock at phase boundaries of the
// forward kernel into g_trace (read back with plnerf_debug_trace; tools/trace_fwd.py)
#ifdef PLNERF_TRACE
__device__ unsigned long long g_trace[64];
#define TR(i) do { if (blockIdx.x == (PLNERF_TRACE) && threadIdx.x == 0) { g_trace[i] = clock64(); if ((i) == 0) g_trace[48] = wall_clock64(); if ((i) == 42) g_trace[49] = wall_clock64(); } } while (0)
#else
#define TR(i) do { } while (0)
#endif

__host__ __device__ constexpr int tile_rows(int ns) { return ns == 1 ? 128 : 64; }

// head-block accessors (same order as the fp32 pack's head block)
__device__ __forceinline__ const float* head(const void* packed) { return (const float*)packed; }
constexpr int H_BIAS = HB_BIAS - HB, H_BF = HB_BF - HB, H_BV = HB_BV - HB, H_WA = HB_WA - HB, H_BA = HB_BA - HB,
              H_WR = HB_WR - HB, H_BR = HB_BR - HB;

// ------------------------------------------------------------------------------------
// packing: [head fp32][fwd GEMMs: NS planes of the mode's element type][dgrad GEMMs: one IEEE-half plane][compose block
// fp32: written first, by impl::compose_pack -- the view layer's operands are packed FROM it];
// the GEMMs are those of the composed network (mlp_layout.h: FwdGemmC / BwdGemmC);
// a GEMM's weight operand is stored as blocks
// (32-feature tile ft, 16-deep k step ks), block order [ft][ks], NS planes per block, each plane
// 64 lanes x 8 bf16 (1 KiB): lane l = (g<<5 | ff) holds W[32 ft + ff][16 ks + 8 g + 0..7].
// ------------------------------------------------------------------------------------
template <int NS>
__global__ void pack_bf16_kernel(ParamPtrs P, unsigned char* __restrict__ out, int regions, int fwd_ns,
                                 unsigned* __restrict__ status) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int FWD_GROUPS = FWDC_FLOATS / 8;
    constexpr int BWD_GROUPS = BWDC_FLOATS / 8;
    if (idx < HEAD_FLOATS && (regions & 1)) {
        // head block: the fp32 pack's order; the view layer's bias slot holds b_c = W_vf b_f + b_v (compose block)
        const int h = idx + HB;
        float v;
        if (h < HB_BF) { const int r = h - HB_BIAS; v = P.p[2 * (r >> 8) + 1][r & 255]; }
        else if (h < HB_BV) v = P.p[P_BF][h - HB_BF];
        else if (h < HB_WA) v = P.cb[CB_BC + (h - HB_BV)];
        else if (h < HB_BA) v = P.p[P_WA][h - HB_WA];
        else if (h < HB_WR) v = (h == HB_BA) ? P.p[P_BA][0] : 0.0f;
        else if (h < HB_BR) v = P.p[P_WR][h - HB_WR];
        else v = (h - HB_BR) < 3 ? P.p[P_BR][h - HB_BR] : 0.0f;
        reinterpret_cast<float*>(out)[idx] = v;
    }
    if (idx >= FWD_GROUPS + BWD_GROUPS) return;
    const bool is_fwd = idx < FWD_GROUPS;
    if (!(regions & (is_fwd ? 1 : 2))) return;   // regions: bit 0 = head + forward GEMMs, bit 1 = backward GEMMs
    int rem = is_fwd ? idx : idx - FWD_GROUPS;      // group index within the fwd / bwd region
    int g = 0, off = 0;                              // off in groups
    if (is_fwd) {
        while (g < N_FWDC - 1 && rem >= off + fwdc_K[g] * fwdc_N[g] / 8) { off += fwdc_K[g] * fwdc_N[g] / 8; ++g; }
    } else {
        while (g < N_BWDC - 1 && rem >= off + bwdc_K[g] * bwdc_N[g] / 8) { off += bwdc_K[g] * bwdc_N[g] / 8; ++g; }
    }
    const int r = rem - off;                         // group within the GEMM: (ft*KS + ks)*64 + lane
    const int KS = (is_fwd ? fwdc_K[g] : bwdc_K[g]) / 16;
    const int blk = r >> 6, lane = r & 63;
    const int ft = blk / KS, ks = blk - ft * KS;
    const int row = ft * 32 + (lane & 31), k0 = ks * 16 + 8 * (lane >> 5);
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = is_fwd ? fwdc_src(P, g, k0 + e, row) : bwdc_src(P, g, k0 + e, row);
        hi[e] = (H16T)v;
        lo[e] = (H16T)(v - (float)hi[e]);
        if (std::is_same<H16T, _Float16>::value && !(fabsf(v) <= H16_MAX) && status)
            atomicOr(status, PLNERF_RANGE_WEIGHT);      // a weight beyond the half range (or not finite)
    }
    // element offset of the GEMM's region: planes are interleaved per block; the dgrad section starts after
    // the forward section (fwd_ns planes) and always holds ONE plane.  A call with both region bits packs both
    // sections in this launch (NS = the forward section's plane count).
    const int ns_here = (is_fwd || regions != 3) ? NS : 1;
    const size_t region = (size_t)(is_fwd ? 0 : FWDC_FLOATS) * fwd_ns + (size_t)off * 8 * ns_here;
    bf16x8* dst = reinterpret_cast<bf16x8*>(out + HEAD_BYTES) + region / 8 + ((size_t)blk * ns_here) * 64 + lane;
    dst[0] = hi;
    if (ns_here == 2) dst[64] = lo;
}

// WAVE-UNIFORM pointer (bf16x8 units) to block (ft, ks = ks0) of a GEMM; lanes add their own index, so
// every weight load is "scalar base + one shared lane offset" and needs no per-load address registers
template <int NS>
__device__ __forceinline__ const bf16x8* wblock(const void* packed, bool fwd, int elem_off, int KS, int ft, int ks0,
                                                int fwd_ns = NS) {
    const bf16x8* base = reinterpret_cast<const bf16x8*>((const unsigned char*)packed + HEAD_BYTES);
    const size_t region = ((size_t)(fwd ? 0 : FWDC_FLOATS) * fwd_ns + (size_t)elem_off * NS) / 8;
    return base + region + ((size_t)(ft * KS + ks0) * NS) * 64;
}

// ------------------------------------------------------------------------------------
// tile GEMM: acc[t] (32 features x 32 samples) += W[ft rows][k range] . X^T[k range][sample tile t]
//   a      : weight blocks of this wave's feature tile, starting at the first k step (lane included)
//   b_lane : &X_plane0[(lane & 31) * ld + 8 * (lane >> 5)] at the first k of the range
// Software pipeline, KC k-steps fully unrolled (all indices static):
//   weight fragments (global, L2-resident) are fetched PF steps ahead into a PF+1 slot ring,
//   activation fragments (LDS) one step ahead into a 2-slot ring,
// The source order is "issue next loads, then this step's MFMAs"; hipcc schedules around it and
// inserts the counted vmcnt/lgkmcnt waits.  (Pinning the two phases with sched_barrier(0) measured
// 24 % SLOWER in bf16 and neutral in bf16x3, so it is off.)
// ------------------------------------------------------------------------------------
#ifndef PLNERF_WPF
#define PLNERF_WPF 4
#endif
constexpr int WPF = PLNERF_WPF;   // weight prefetch distance (k-steps)

template <int NS, int PFQ = WPF>
struct WQueue {
    bf16x8 q[PFQ + 1][NS];   // one ring, reused by every GEMM of the tile walk
};

// request the first min(KC, WPF) weight blocks of a GEMM.
// `rot` rotates the order in which the k-steps of a GEMM are visited (step i handles k-step
// (i + rot) mod KC).  Every workgroup walks the same layers at the same pace, so without it all
// CUs of an XCD ask the L2 for the same few KB of weights at the same moment and only the one or
// two L2 channels that own those lines are busy; rotating by workgroup spreads the simultaneous
// requests over the whole layer (all channels).  Only the fp32 summation order changes.
template <int NS, int KC, int PFQ = WPF>
__device__ __forceinline__ void wq_prime(WQueue<NS, PFQ>& w, const bf16x8* __restrict__ a, const int rot, const int lane) {
    constexpr int PF = KC < PFQ ? KC : PFQ;
#pragma unroll
    for (int p = 0; p < PF; ++p) {
        const int ks = (p + rot) & (KC - 1);
#pragma unroll
        for (int s = 0; s < NS; ++s) w.q[p][s] = a[(ks * NS + s) * 64 + lane];
    }
}

template <int NS, int NT, int KC, int PFQ = WPF>
__device__ __forceinline__ void mma_bf16(f32x16 (&acc)[NT], WQueue<NS, PFQ>& w, const bf16x8* __restrict__ a,
                                         const H16T* b_lane, const int ld, const int plane_stride,
                                         const int rot, const int lane) {
    static_assert((KC & (KC - 1)) == 0, "KC must be a power of two");
    constexpr int PF = KC < PFQ ? KC : PFQ;
    bf16x8 bq[2][NT][NS];
    {
        const H16T* b0 = b_lane + (rot & (KC - 1)) * 16;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int s = 0; s < NS; ++s)
                bq[0][t][s] = *reinterpret_cast<const bf16x8*>(b0 + s * plane_stride + (size_t)t * 32 * ld);
    }
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        // keep the rotated addresses from being hoisted out of the (outer) layer loop as 2*KC
        // loop-invariant address registers: recompute them per step from an opaque copy of rot
        int rot_i = rot;
        asm volatile("" : "+s"(rot_i));
        if (i + PF < KC) {
            const int ks = (i + PF + rot_i) & (KC - 1);
#pragma unroll
            for (int s = 0; s < NS; ++s) w.q[(i + PF) % (PF + 1)][s] = a[(ks * NS + s) * 64 + lane];
        }
        if (i + 1 < KC) {
            const H16T* b1 = b_lane + ((i + 1 + rot_i) & (KC - 1)) * 16;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    bq[(i + 1) & 1][t][s] =
                        *reinterpret_cast<const bf16x8*>(b1 + s * plane_stride + (size_t)t * 32 * ld);
        }
        const bf16x8 ah = w.q[i % (PF + 1)][0];
        const bf16x8 al = w.q[i % (PF + 1)][NS - 1];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = H16_MFMA(ah, bq[i & 1][t][0], acc[t], 0, 0, 0);
            if (NS == 2) {
                acc[t] = H16_MFMA(al, bq[i & 1][t][0], acc[t], 0, 0, 0);
                acc[t] = H16_MFMA(ah, bq[i & 1][t][NS - 1], acc[t], 0, 0, 0);
            }
        }
    }
}

template <int NT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}

// four consecutive fp32 values -> 16-bit hi (+ lo) planes; conversions in pairs (v_cvt_pk_{f16,bf16}_f32)
template <int NS>
__device__ __forceinline__ void split4(const float (&v)[4], H16T* p0, const int plane_stride) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef H16T h2 __attribute__((ext_vector_type(2)));
    const f2 a = {v[0], v[1]}, b = {v[2], v[3]};
    const h2 ha = __builtin_convertvector(a, h2), hb = __builtin_convertvector(b, h2);
    bf16x4 hi = {ha[0], ha[1], hb[0], hb[1]};
    *reinterpret_cast<bf16x4*>(p0) = hi;
    if (NS == 2) {
        const f2 ra = a - __builtin_convertvector(ha, f2), rb = b - __builtin_convertvector(hb, f2);
        const h2 la = __builtin_convertvector(ra, h2), lb = __builtin_convertvector(rb, h2);
        bf16x4 lo = {la[0], la[1], lb[0], lb[1]};
        *reinterpret_cast<bf16x4*>(p0 + plane_stride) = lo;
    }
}

// saturating fp32 -> half (an overflow to inf would turn into NaN gradients)
__device__ __forceinline__ _Float16 to_half_sat(float x) { return (_Float16)fminf(fmaxf(x, -H16_MAX), H16_MAX); }

// ------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------
struct FwdArgs {
    const void* packed;
    const float* pts;
    const float* viewdirs;
    const float* embedded;
    int xyz_ch, dir_ch;   // columns of `embedded`: input_ch | input_ch_views
    int n_rows, spr;
    float* raw_out;
    void* saved;          // training: half planes + relu masks (mlp_layout.h); nullptr = inference
    unsigned* status;     // range status word of the packed buffer (half elements only; nullptr otherwise)
    float pe_scale;       // the in-kernel encoding's input scale: sin / cos(x * pe_scale * 2^k) (1, or pi: depth variant)
    float act_beta;       // > 0: sigma leaves as softplus(beta)(sigma) (common.h: density_activation)
};

#include "mlp_h16_fwd_pp.inc"

#ifdef H16_HAS_BWD
// ------------------------------------------------------------------------------------
// backward: dgrad chain of every 16-bit mode, on plain IEEE-half operands (this file's f16 instantiation).
// The upstream gradient is multiplied by ONE power-of-two scale per launch (max |g_raw| -> [8, 16), mlp_layout.h)
// as it is loaded, so the whole chain -- linear in g_raw -- lives in half range; each layer's masked
// pre-activation gradient tile in LDS is already the (scaled) half plane the weight-gradient stage reads, and
// is copied out as it is.  One MFMA per product: with the saved state in half anyway (section 3 of DESIGN.md)
// a 3-term chain bought 5.7e-4 -> 8.3e-4 of max |g| at three times the MFMA work.
// ------------------------------------------------------------------------------------
struct BwdArgs {
    const void* packed;
    const float* g_raw;
    int n_rows;
    const void* saved;      // half planes + relu masks written by the training forward (masks are read here)
    void* dz;               // half planes of the scaled pre-activation gradients, for the wgrad stage
    unsigned* gmax;         // max |g_raw| of this launch as fp32 bits (the workspace's word): read, or -- n_cand > 0 -- written
    int fwd_ns;             // plane count of the packed forward section (locates the dgrad section)
    const unsigned* cand;   // n_cand > 0: candidates whose maximum IS that word (plnerf_quad_bwd's per-workgroup maxima);
    int n_cand;             //   every workgroup takes the maximum itself, the network's first one stores it for the later kernels
    const unsigned* live;   // the live-row list's home (mlp_bwd_plan.h: "live rows"), or nullptr: tile t then handles COMPACT rows
                            //   [TM t, TM t + TM) -- upstream gradient and masks come from the listed rows, dz goes to the compact ones
};
// Up to two networks' chains in ONE grid (plnerf_mlp_bwd_multi; round 5): tiles [0, tiles0) belong to n[0], the rest to
// n[1].  A training step's coarse and fine backward launched separately end on partial rounds (262,144 rows = 1,366
// tiles = 5.34 rounds of 256) and pay two launch ramps; measured bound of one grid: profiles/r05_merged_bwd_bound.txt.
struct BwdArgs2 {
    BwdArgs n[2];
    int tiles0;
};
// Rows per workgroup tile.  192 since round 4 (64 until round 3): a wave's 32-feature slab of weight fragments is fetched
// once per 192 rows instead of once per 64 -- the fetches (128 KB per workgroup and layer through the CU's texture path,
// which the dz stores share) were what the 64-row kernel waited for (DESIGN.md section 10).  255 VGPR without spills and
// 159,872 B of LDS: ONE workgroup of eight waves per CU instead of two.  Same-box, kernel level (rocprofv3, fine launch):
// 64 rows 1103 us, 128 rows 1086 us, 192 rows 1017 us; step -1.2 %; results bit-identical (a row's arithmetic does not
// depend on its tile): profiles/r04_dgrad_tile_ab.txt.
constexpr int BWD_TM = PLNERF_BWD_TM;

// relu mask of a saved activation plane -> one bit per (sample, feature) in LDS.  The tile's rows are contiguous
// in the mask plane (32 B per row): one dword per thread and layer.  LDS rows are padded to 9 words: the epilogue
// reads one byte per lane with lanes on consecutive rows, and a 32-byte stride would put 32 lanes on 4 banks.
#ifndef PLNERF_BWD_WPF
#define PLNERF_BWD_WPF 4
#endif
constexpr int BWD_WPF = PLNERF_BWD_WPF;      // the dgrad kernel's weight prefetch distance (k-steps)
constexpr int MASK_ROW_WORDS = 9;
constexpr int MASK_TILE_BYTES = BWD_TM * 4 * MASK_ROW_WORDS;   // one layer's mask rows of a tile in LDS
constexpr int MASK_WORDS = (BWD_TM * 8 + NTHREADS - 1) / NTHREADS;   // mask words per thread and layer (the last may be partial)
static_assert(BWD_TM % 32 == 0 && MASK_WORDS >= 1, "whole 32-row tiles");
__device__ __forceinline__ unsigned mask_word(const unsigned char* __restrict__ mask_plane, const int row, const int w) {
    return reinterpret_cast<const unsigned*>(mask_plane + (size_t)row * 32)[w];      // word w of the row's 32 mask bytes
}
__device__ __forceinline__ void mask_commit(unsigned char* maskb, const unsigned word, const int tid, const int k = 0) {
    const int q = tid + NTHREADS * k;
    if (q < BWD_TM * 8) reinterpret_cast<unsigned*>(maskb)[(q >> 3) * MASK_ROW_WORDS + (q & 7)] = word;
}

// ReLU nibble -> AND mask over four packed halves (16 entries x 8 B in LDS, built once per workgroup): applying
// relu' to four values costs a nibble extraction, one 8-byte LDS read and two v_and instead of 12 VALU
__device__ __forceinline__ void build_nibble_table(unsigned* tbl, const int tid) {
    if (tid < 16) {
        tbl[2 * tid + 0] = ((tid & 1) ? 0x0000ffffu : 0u) | ((tid & 2) ? 0xffff0000u : 0u);
        tbl[2 * tid + 1] = ((tid & 4) ? 0x0000ffffu : 0u) | ((tid & 8) ? 0xffff0000u : 0u);
    }
}

// (`tiles`: the workgroup's first 32-row tile of the layer's dz plane, TILED order of mlp_layout.h -- the wave's fragments
// go out from the registers as they are, one contiguous KiB per store; rows past n_rows land in the planes' row padding)
// (WA_LANE: `wa` is the lane's own 16 alpha-row weights, [4 rg + j] = w_alpha[f_base + 8 rg + 4 (lane >> 5) + j], fetched by
// the caller ahead of the K loop; otherwise the alpha row itself)
template <int NT, bool MASK, bool ALPHA, bool WA_LANE = false>
__device__ __forceinline__ void store_dz(f32x16 (&acc)[NT], H16T* g, const float* gr, const float* __restrict__ wa,
                                         const unsigned char* maskb, const unsigned* tbl, const int f_base,
                                         const int lane, H16T* __restrict__ tiles) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef H16T h2 __attribute__((ext_vector_type(2)));
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    // The relu masks first, for the whole slab: NT x 4 mask bytes, then NT x 4 table entries, each batch back to back.
    // (Left inside the loop below, every byte read and every table read was followed by a wait for the LDS -- the
    // compiler cannot prove that the tile writes in between do not alias them -- sixteen exposed LDS latencies per
    // layer: 1.6 k of a layer's ~7 k cycles.)
    u2 am[NT][4];
    if (MASK) {
        unsigned mb[NT][4];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
                mb[t][rg] = maskb[(t * 32 + (lane & 31)) * (4 * MASK_ROW_WORDS) + ((f_base + 8 * rg) >> 3)];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg)
                am[t][rg] = *reinterpret_cast<const u2*>(tbl + 2 * ((mb[t][rg] >> (4 * (lane >> 5))) & 0xFu));
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int s = t * 32 + (lane & 31);
        const float ga = ALPHA ? gr[s * 4 + 3] : 0.0f;
        u2 wprev = {0u, 0u};
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int f0 = f_base + 8 * rg + 4 * (lane >> 5);
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = acc[t][4 * rg + j];
                if (ALPHA) v[j] = fmaf(ga, WA_LANE ? wa[4 * rg + j] : wa[f0 + j], v[j]);
                v[j] = __builtin_amdgcn_fmed3f(v[j], -H16_MAX, H16_MAX);   // saturate: an inf would become NaN gradients (without: dgrad -3 %, step -0.3 %; kept)
            }
            const f2 a = {v[0], v[1]}, b = {v[2], v[3]};
            u2 w = {__builtin_bit_cast(unsigned, __builtin_convertvector(a, h2)),
                    __builtin_bit_cast(unsigned, __builtin_convertvector(b, h2))};
            if (MASK) w = w & am[t][rg];
            if (rg & 1) {      // fragment rg >> 1 of slab f_base / 32: register groups 2 f and 2 f + 1
                const u4 frag = {wprev[0], wprev[1], w[0], w[1]};
                // (non-temporal: nothing reads a dz plane before the whole launch has written 3.8 GB past it; measured
                // -1.2 % step time against plain stores, same box)
                __builtin_nontemporal_store(frag, reinterpret_cast<u4*>(tiles + (size_t)t * 32 * W + ((size_t)(((f_base >> 5) * 2 + (rg >> 1)) * 64 + lane)) * 8));
                // The next layer's LDS tile, one 16-byte write per lane and register-group PAIR.  A lane holds 4 features
                // (8 bytes) of group rg and 4 of group rg + 1, its partner in the other lane half the 4 in between: written
                // as they lie, two ds_write_b64 per pair put rows s and s + 8 of a 16-lane group on the same banks at this
                // row stride (528 B; 16.6 % of the kernel's LDS-active cycles were bank conflicts, r02 PMC) -- and a stride
                // that frees 8-byte writes conflicts the K loop's 16-byte reads.  One v_permlane32_swap per dword trades
                // the halves' pieces instead (lane half 0 <- the partner's piece of the even group, lane half 1 <- the
                // partner's piece of the odd one): each lane then owns 8 consecutive features, and a 16-byte write at this
                // stride is conflict-free like the reads.
                const u2 x0 = __builtin_amdgcn_permlane32_swap(wprev[0], w[0], false, false);
                const u2 x1 = __builtin_amdgcn_permlane32_swap(wprev[1], w[1], false, false);
                const u4 own8 = {x0[0], x1[0], x0[1], x1[1]};
                *reinterpret_cast<u4*>(g + (size_t)s * BLDA + (f_base + 8 * (rg - 1) + 8 * (lane >> 5))) = own8;
            }
            wprev = w;
        }
    }
}

__global__ __launch_bounds__(NTHREADS, BWD_TM <= 96 ? 4 : 2) void mlp_bwd_h16_kernel(BwdArgs2 p) {
    const bool second = (int)blockIdx.x >= p.tiles0;      // (uniform: scalar selects)
    const BwdArgs a = second ? p.n[1] : p.n[0];
    const int bid = second ? (int)blockIdx.x - p.tiles0 : (int)blockIdx.x;
    static_assert(sizeof(H16T) == 2, "half planes");
    constexpr int NS = 1, TM = BWD_TM, NT = TM / 32;
    constexpr int G_PLANE = TM * BLDA;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    H16T* g = reinterpret_cast<H16T*>(smem_raw);
    float* gr = reinterpret_cast<float*>(g + G_PLANE);
    unsigned char* maskb = reinterpret_cast<unsigned char*>(gr + TM * 4);
    unsigned* tbl = reinterpret_cast<unsigned*>(maskb + 8 * MASK_TILE_BYTES);
    int* rowl = reinterpret_cast<int*>(tbl + 32);      // live rows: the tile's TM list entries
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform
    const int row0 = bid * TM;
    const size_t N = (size_t)a.n_rows;
    const float* hd = head(a.packed);
    const int rot = bid >> 3;   // consecutive blocks of one XCD (b, b+8, ...) get consecutive rotations (the network's own tile index: a row's arithmetic does not depend on what else shares the grid)
    TR(0);
    build_nibble_table(tbl, tid);
    const size_t NSV = sv_rows(N);      // row stride of the saved state (padded, mlp_layout.h)
    const size_t ND = dz_rows(N);       // row stride of the dz planes (padded to this kernel's tiles)
#define DPLANE(p) (reinterpret_cast<H16T*>(a.dz) + (size_t)(p) * W * ND)
#define DTILES(p) (DPLANE(p) + (size_t)row0 * W)      // the workgroup's two 32-row tiles of plane p (row0 % 64 == 0)
#define MASKP(p) (reinterpret_cast<const unsigned char*>(a.saved) + (size_t)SVC_FLOATS * 2 * NSV + (size_t)(p) * (W / 8) * NSV)
#define WBK(g_, KS) wblock<NS>(a.packed, false, bwdc_off(g_), KS, wave, 0, a.fwd_ns)
    float dz_scale;
    {
        unsigned gbits;
        if (a.n_cand > 0) {      // (uniform) the producer left per-workgroup maxima instead of one word: no absmax pass, no memset
            __shared__ unsigned cand_max[NTHREADS / 64];
            unsigned m = 0u;      // (non-negative floats and NaNs order as unsigned integers)
            for (int i = tid; i < a.n_cand; i += NTHREADS) m = max(m, a.cand[i]);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
            if (lane == 0) cand_max[wave] = m;
            __syncthreads();
            gbits = cand_max[0];
#pragma unroll
            for (int w = 1; w < NTHREADS / 64; ++w) gbits = max(gbits, cand_max[w]);
            if (bid == 0 && tid == 0) *a.gmax = gbits;      // (the weight-gradient reduction and plnerf_mlp_input_grad read it, after this launch)
        } else {
            gbits = *a.gmax;
        }
        dz_scale = __uint_as_float(dzh_scale_bits(gbits));      // (mlp_layout.h: the one derivation of the launch scale)
    }
    static_assert(TM <= NTHREADS, "one upstream-gradient row per thread");
    // Live rows (mlp_bwd_plan.h): the tile's rows are COMPACT rows [row0, row0 + TM) -- row k of the tile reads its upstream
    // gradient and its masks from source row list[row0 + k] and writes dz at compact row row0 + k, where the weight-gradient
    // stage looks for it.  A tile past n_live has nothing to do (the grid is sized from n_rows on the host, which never reads
    // n_live); rows of the last live tile past n_live get dz = 0, as rows past n_rows do without a list.  (After the scale block:
    // the network's first workgroup has stored the launch scale's word, live rows or none.)
    const bool listed = a.live != nullptr;      // (uniform)
    const int n_eff = listed ? (int)a.live[plnerf::bwdplan::live_scan_word(plnerf::bwdplan::LIVE_N)] : a.n_rows;
    if (row0 >= n_eff) return;
    const int rows_valid = min(TM, n_eff - row0);
    if (listed) {      // (entries past n_live: the last live row's -- nothing is fetched from a row that is not live; their dz is zero)
        if (tid < TM) rowl[tid] = (int)a.live[plnerf::bwdplan::live_entry_word((size_t)min(row0 + tid, n_eff - 1))];
        __syncthreads();
    }
#define SRC_ROW(r) (listed ? rowl[r] : row0 + (r))      // source row of the tile's row r
    float4 g_up = make_float4(0.f, 0.f, 0.f, 0.f);      // (the prologue's first request: see the masks below)
    if (tid < rows_valid) g_up = reinterpret_cast<const float4*>(a.g_raw)[SRC_ROW(tid)];
    // dz_view's own inputs, requested with the upstream gradient and the masks so that they share that one latency: a thread's items
    // idx = tid + NTHREADS k all have the same feature octet c = tid & 15 (its 24 rgb-head weights: registers) and
    // consecutive bytes of the view layer's mask plane.  (Loaded inside the loop below -- a predicated byte load and 24
    // weight loads per iteration, each iteration waiting for its own -- this phase lasted 11.3 k cycles, more than a trunk
    // layer; clock stamps.)
    constexpr int VIEW_ITEMS = (TM * (HV / 8) + NTHREADS - 1) / NTHREADS;
    static_assert(NTHREADS % 16 == 0 && H_WR % 4 == 0 && H_WA % 4 == 0 && HV % 8 == 0, "a thread keeps its feature octet across its items; 16-byte weight loads");
    const int vc = tid & 15;
    unsigned hvm[VIEW_ITEMS];
    {
        const unsigned char* hv_mask = MASKP(8);
#pragma unroll
        for (int k = 0; k < VIEW_ITEMS; ++k) {
            const int idx = tid + NTHREADS * k;
            hvm[k] = (idx < TM * (HV / 8) && (idx >> 4) < rows_valid) ? hv_mask[(size_t)SRC_ROW(idx >> 4) * (HV / 8) + (idx & 15)] : 0u;
        }
    }
    float wr8[3][8];
    {
        const float* wr = hd + H_WR;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4 lo = *reinterpret_cast<const float4*>(wr + q * HV + vc * 8);
            const float4 hi = *reinterpret_cast<const float4*>(wr + q * HV + vc * 8 + 4);
            wr8[q][0] = lo.x; wr8[q][1] = lo.y; wr8[q][2] = lo.z; wr8[q][3] = lo.w;
            wr8[q][4] = hi.x; wr8[q][5] = hi.y; wr8[q][6] = hi.z; wr8[q][7] = hi.w;
        }
    }
    // All eight trunk ReLU masks of the tile (8 x 2 KB) are requested here, once: vmcnt retires in order, so a
    // mask load in flight inside the layer loop (HBM latency, ~5000 cycles) holds up the first weight fragment
    // of the K loop behind it -- every layer.  They are the LAST requests of the prologue: loads return in the order
    // they were issued, so the upstream gradient (first) releases the first barrier, dz_view's inputs (next) its
    // arithmetic, and the masks land while that runs -- they are not needed before mask_commit.
    unsigned mw[8][MASK_WORDS];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int k = 0; k < MASK_WORDS; ++k) {
            const int q = tid + NTHREADS * k;      // word q of the tile: row q / 8, word q % 8 of its 32 bytes
            mw[p][k] = (q < TM * 8 && (q >> 3) < rows_valid) ? mask_word(MASKP(p), SRC_ROW(q >> 3), q & 7) : 0u;
        }
    if (tid < TM) {
        float4 v = g_up;
        v.x *= dz_scale; v.y *= dz_scale; v.z *= dz_scale; v.w *= dz_scale;
        reinterpret_cast<float4*>(gr)[tid] = v;
    }
    __syncthreads();
    TR(43);
    // dz_view = (g_rgb W_rgb) * relu'(hv): 8 features per thread-iteration, coalesced planes
    {
        H16T* dzv_plane = DPLANE(0) + (size_t)DZC_V_OFF * ND;
#pragma unroll
        for (int k = 0; k < VIEW_ITEMS; ++k) {
            const int idx = tid + NTHREADS * k;
            if (idx < TM * (HV / 8)) {
                const int s = idx >> 4;
                const float4 gs = reinterpret_cast<const float4*>(gr)[s];
                bf16x8 h;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float t = gs.x * wr8[0][e];
                    t = fmaf(gs.y, wr8[1][e], t);
                    t = fmaf(gs.z, wr8[2][e], t);
                    t = ((hvm[k] >> e) & 1u) ? t : 0.0f;
                    h[e] = (H16T)fminf(fmaxf(t, -H16_MAX), H16_MAX);
                }
                *reinterpret_cast<bf16x8*>(g + (size_t)s * BLDA + vc * 8) = h;
                if (s < rows_valid) *reinterpret_cast<bf16x8*>(dzv_plane + (size_t)(row0 + s) * HV + vc * 8) = h;
            }
        }
    }
    __syncthreads();
    TR(44);
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
        for (int k = 0; k < MASK_WORDS; ++k) mask_commit(maskb + (size_t)p * MASK_TILE_BYTES, mw[p][k], tid, k);
    const H16T* g_lane = g + (lane & 31) * BLDA + 8 * (lane >> 5);
    f32x16 acc[NT];
    // d h7 = dz_view . W_c + g_sigma w_alpha, masked by h7  (K = 128; W_c = W_vf W_f, the composed view layer of mlp_layout.h:
    // until round 5 this was two GEMMs, dz_view . W_vf -> the dz_feature plane -> . W_f)
    WQueue<NS, BWD_WPF> wq;
    const bf16x8* wp = WBK(DC_VIEWS, 8);
    wq_prime<NS, 8, BWD_WPF>(wq, wp, rot, lane);
    float wa_lane[16];      // (requested ahead of the K loop: inside the epilogue the four loads' L2 latency was exposed)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
        const float4 w4 = *reinterpret_cast<const float4*>(hd + H_WA + wave * 32 + 8 * rg + 4 * (lane >> 5));
        wa_lane[4 * rg + 0] = w4.x; wa_lane[4 * rg + 1] = w4.y; wa_lane[4 * rg + 2] = w4.z; wa_lane[4 * rg + 3] = w4.w;
    }
    zero_acc(acc);
    mma_bf16<NS, NT, 8, BWD_WPF>(acc, wq, wp, g_lane, BLDA, G_PLANE, rot, lane);
    wp = WBK(DC_L7, 16);
    wq_prime<NS, 16, BWD_WPF>(wq, wp, rot, lane);
    TR(47);
    __syncthreads();
    store_dz<NT, true, true, true>(acc, g, gr, wa_lane, maskb + 7 * MASK_TILE_BYTES, tbl, wave * 32, lane, DTILES(7));
    __syncthreads();
    TR(1);
#pragma unroll 1
    for (int l = 7; l >= 1; --l) {
        TR(2 + 5 * (7 - l));
        zero_acc(acc);
        mma_bf16<NS, NT, 16, BWD_WPF>(acc, wq, wp, g_lane, BLDA, G_PLANE, rot, lane);
        if (l > 1) {
            wp = wblock<NS>(a.packed, false, bwdc_off(DC_L7) + (8 - l) * W * W, 16, wave, 0, a.fwd_ns);
            wq_prime<NS, 16, BWD_WPF>(wq, wp, rot, lane);
        }
        TR(3 + 5 * (7 - l));
        __syncthreads();
        TR(4 + 5 * (7 - l));
        store_dz<NT, true, false>(acc, g, gr, nullptr, maskb + (size_t)(l - 1) * MASK_TILE_BYTES, tbl, wave * 32, lane,
                                  DTILES(l - 1));
        TR(5 + 5 * (7 - l));
        __syncthreads();
        TR(6 + 5 * (7 - l));
    }
    TR(42);
#undef SRC_ROW
#undef DPLANE
#undef DTILES
#undef MASKP
#undef WBK
}
#endif  // H16_HAS_BWD

template <int NS>
int fwd_launch(const FwdArgs& a, hipStream_t st) {
    constexpr int TM = tile_rows(NS);
    dim3 grid((a.n_rows + TM - 1) / TM);
    if (a.saved) {
        // training: ping-pong kernel, the tile's saved half plane is written out as side work
        const size_t lds = pp_lds_bytes<NS>();
        (void)hipFuncSetAttribute((const void*)mlp_fwd_pp_kernel<NS, true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((mlp_fwd_pp_kernel<NS, true>), grid, dim3(NTHREADS), lds, st, a);
    } else {
        // inference: ping-pong kernel
        const size_t lds = pp_lds_bytes<NS>();
        (void)hipFuncSetAttribute((const void*)mlp_fwd_pp_kernel<NS, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        hipLaunchKernelGGL((mlp_fwd_pp_kernel<NS, false>), grid, dim3(NTHREADS), lds, st, a);
    }
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

#ifdef H16_HAS_BWD
inline int bwd_launch(const BwdArgs* jobs, int n, hipStream_t st) {
    const size_t lds = (size_t)BWD_TM * BLDA * 2 + (size_t)BWD_TM * 16 + (size_t)8 * MASK_TILE_BYTES + 128 + (size_t)BWD_TM * 4;      // (+ 32 B static)
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)mlp_bwd_h16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    for (int j = 0; j < n; j += 2) {      // two networks per grid
        BwdArgs2 p{};
        p.n[0] = jobs[j];
        p.n[1] = jobs[j + 1 < n ? j + 1 : j];
        p.tiles0 = plnerf::bwdplan::dgrad_tiles(jobs[j].n_rows);
        const int tiles = p.tiles0 + (j + 1 < n ? plnerf::bwdplan::dgrad_tiles(jobs[j + 1].n_rows) : 0);
        hipLaunchKernelGGL(mlp_bwd_h16_kernel, dim3(tiles), dim3(NTHREADS), lds, st, p);
        PLNERF_CHECK_LAUNCH();
    }
    return PLNERF_OK;
}
#endif

}  // namespace

// ---- entry points of this element type (called from the dispatchers in mlp_h16.hip) ----
inline size_t h16_compose_offset(int ns) {   // head + forward section (ns planes) + dgrad section (one half plane)
    return HEAD_BYTES + (size_t)FWDC_FLOATS * ns * 2 + (size_t)BWDC_FLOATS * 2;
}
inline size_t h16_packed_bytes(int ns) { return h16_compose_offset(ns) + (size_t)CB_FLOATS * 4; }   // + the compose block (fp32)

// regions: bit 0 = head + forward GEMMs (ns planes of this element type), bit 1 = dgrad GEMMs (ns planes of this
// element type, placed after a forward section of fwd_ns planes)
inline int h16_pack(const float* const* params, int xyz_ch, int dir_ch, int ns, int regions, int fwd_ns, void* packed,
                    unsigned* status, hipStream_t st) {
    ParamPtrs P;
    P.xyz_ch = xyz_ch; P.dir_ch = dir_ch;
    P.cb = reinterpret_cast<const float*>((const unsigned char*)packed + h16_compose_offset(fwd_ns));      // (written by impl::compose_pack, earlier on this stream)
    for (int i = 0; i < PLNERF_N_PARAM_TENSORS; ++i) P.p[i] = params[i];
    const int groups = (FWDC_FLOATS + BWDC_FLOATS) / 8;
    const int threads = 256, blocks = (groups + threads - 1) / threads;
    if (ns == 1) hipLaunchKernelGGL(pack_bf16_kernel<1>, dim3(blocks), dim3(threads), 0, st, P, (unsigned char*)packed, regions, fwd_ns, status);
    else hipLaunchKernelGGL(pack_bf16_kernel<2>, dim3(blocks), dim3(threads), 0, st, P, (unsigned char*)packed, regions, fwd_ns, status);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

inline int h16_fwd(const void* packed, int ns, const float* pts, const float* viewdirs, const float* embedded,
                   int xyz_ch, int dir_ch, int n_rows, int samples_per_ray, plnerf::impl::FwdOpt opt, float* raw_out, void* saved,
                   unsigned* status, hipStream_t st) {
    FwdArgs a{packed, pts, viewdirs, embedded, xyz_ch, dir_ch, n_rows, samples_per_ray < 1 ? 1 : samples_per_ray,
              raw_out, saved, status, opt.pe_scale, opt.act_beta};
    return ns == 1 ? fwd_launch<1>(a, st) : fwd_launch<2>(a, st);
}

#ifdef H16_HAS_BWD
inline int h16_dgrad(int n, const plnerf::impl::DgradJob* jobs, hipStream_t st) {
    BwdArgs a[plnerf::impl::MAX_BWD_JOBS];
    for (int j = 0; j < n; ++j)
        a[j] = BwdArgs{jobs[j].packed, jobs[j].g_raw, jobs[j].n_rows, jobs[j].saved, jobs[j].dz, jobs[j].gmax, jobs[j].fwd_ns,
                       jobs[j].cand, jobs[j].n_cand, jobs[j].live};
    return bwd_launch(a, n, st);
}
#endif
