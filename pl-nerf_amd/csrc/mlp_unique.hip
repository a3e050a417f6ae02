// The fine pass's unique-row forward (mlp_unique_plan.h: the rule, who is served, the workspace): the launches around the
// register-resident forward kernel, built like mlp_live.hip.
//
//   uniq_count_kernel     workgroup b counts the EVALUATED (not interior) rows among rows [1024 b, 1024 b + 1024)
//   uniq_scan_kernel      ONE workgroup turns the counts into exclusive offsets (in place) and leaves n_eval
//   uniq_scatter_kernel   workgroup b takes its rows' flags again and writes, from its offset on, its evaluated rows' index,
//                         position and direction (one direction per compact row), and src[row] for each of its rows; the
//                         last workgroup fills the compact inputs up to the next forward tile with copies of the last row
//   (the forward: mlp_fwd_rr_kernel with a device-side row count, mlp_rr_body.inc)
//   uniq_expand_kernel    raw[row] = raw_u[src[row]]
//   uniq_fold_kernel      before the backward: g_raw_u[c] = sum of g_raw over compact row c's run, zero from n_eval on, and
//                         each workgroup's max |g_raw_u|
// Every position is a pure function of pts: no atomics, the same list on every run; no workgroup waits for another inside a
// launch.  The host never reads n_eval.
#include "common.h"
#include "mlp_internal.h"
#include "mlp_unique_plan.h"

using namespace plnerf;

namespace {

constexpr int UB_THREADS = 256;
constexpr int UB_PER_THREAD = uniq::BLOCK_ROWS / UB_THREADS;      // consecutive rows per thread: thread order = row order
static_assert(uniq::BLOCK_ROWS % UB_THREADS == 0, "");
constexpr int SCAN_THREADS = 1024;
constexpr int FOLD_THREADS = uniq::BLOCK_ROWS;

struct UniqArgs {
    const uint32_t* pts;     // [n_rows][3] as words
    const uint32_t* dirs;    // [n_rows / spr][3] as words
    int n_rows, spr;
    unsigned* words;
    unsigned* rows_u;
    unsigned* src;
    uint32_t* pts_u;
    uint32_t* dirs_u;
};

// flags of the thread's UB_PER_THREAD consecutive rows (bit k = row base + k is evaluated), rows past n_rows: none
__device__ __forceinline__ unsigned thread_flags(const UniqArgs& a, const int base) {
    unsigned f = 0u;
#pragma unroll
    for (int k = 0; k < UB_PER_THREAD; ++k) {
        const int row = base + k;
        if (row < a.n_rows && !uniq::interior(a.pts, (size_t)row, (size_t)a.n_rows, a.spr)) f |= 1u << k;
    }
    return f;
}

__global__ __launch_bounds__(UB_THREADS) void uniq_count_kernel(UniqArgs a) {
    __shared__ int wsum[UB_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    int c = __popc(thread_flags(a, b * uniq::BLOCK_ROWS + tid * UB_PER_THREAD));
    c = wave_sum(c);
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < UB_THREADS / 64; ++w) s += wsum[w];
        a.words[uniq::SCAN_WORDS + b] = (unsigned)s;
    }
}

// exclusive scan of the block counts, in place; thread t owns a run of consecutive counts
__global__ __launch_bounds__(SCAN_THREADS) void uniq_scan_kernel(UniqArgs a) {
    const int nb = uniq::blocks((size_t)a.n_rows);
    const int per = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
    __shared__ unsigned wtot[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* cnt = a.words + uniq::SCAN_WORDS;
    const int i0 = min(nb, tid * per), i1 = min(nb, i0 + per);
    unsigned mine = 0u;
    for (int i = i0; i < i1; ++i) mine += cnt[i];
    unsigned incl = mine;      // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
        before += w < wave ? wtot[w] : 0u;
        total += wtot[w];
    }
    unsigned run = before + incl - mine;
    for (int i = i0; i < i1; ++i) {
        const unsigned c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    if (tid == 0) a.words[0] = total;
}

__global__ __launch_bounds__(UB_THREADS) void uniq_scatter_kernel(UniqArgs a) {
    __shared__ unsigned wtot[UB_THREADS / 64];
    __shared__ unsigned n_eval_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int base = b * uniq::BLOCK_ROWS + tid * UB_PER_THREAD;
    const unsigned f = thread_flags(a, base);
    const unsigned mine = (unsigned)__popc(f);
    unsigned incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned pos = a.words[uniq::SCAN_WORDS + b] + incl - mine;
#pragma unroll
    for (int w = 0; w < UB_THREADS / 64; ++w) pos += w < wave ? wtot[w] : 0u;
#pragma unroll
    for (int k = 0; k < UB_PER_THREAD; ++k) {
        const int row = base + k;
        if (row >= a.n_rows) break;
        if (f & (1u << k)) {      // (pos < n_eval <= n_rows: inside every compact buffer)
            a.rows_u[pos] = (unsigned)row;
            const uint32_t* p = a.pts + 3 * (size_t)row;
            const uint32_t* d = a.dirs + 3 * (size_t)(row / a.spr);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a.pts_u[3 * (size_t)pos + c] = p[c];
                a.dirs_u[3 * (size_t)pos + c] = d[c];
            }
            ++pos;
        }
        a.src[row] = pos - 1u;      // (row 0 is the first row of a ray: evaluated, so pos >= 1 here)
    }
    // The last workgroup holds the launch's last row -- the last row of a ray, always evaluated -- and so knows n_eval: it
    // fills the compact inputs from n_eval to the next multiple of uniq::FILL (<= padded(n_rows), the buffers' rows) with
    // copies of that row.  The forward's last live tile computes on them instead of on whatever the workspace held.
    if (b != (int)gridDim.x - 1) return;      // (uniform)
    const int last = a.n_rows - 1;
    if (last >= base && last < base + UB_PER_THREAD) n_eval_s = pos;
    __syncthreads();
    const size_t n_eval = n_eval_s;
    const size_t end = (n_eval + uniq::FILL - 1) / uniq::FILL * uniq::FILL;
    const uint32_t* p = a.pts + 3 * (size_t)last;
    const uint32_t* d = a.dirs + 3 * (size_t)(last / a.spr);
    for (size_t c = n_eval + tid; c < end; c += UB_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.pts_u[3 * c + k] = p[k];
            a.dirs_u[3 * c + k] = d[k];
        }
    }
}

__global__ __launch_bounds__(256) void uniq_expand_kernel(const float4* __restrict__ raw_u, const unsigned* __restrict__ src,
                                                          float4* __restrict__ raw, int n_rows) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row < n_rows) raw[row] = raw_u[src[row]];
}

// a + t where a term that is exactly zero is skipped: the sum's value, with the sign of a zero kept (-0 + +0 would be +0)
__device__ __forceinline__ float add_nonzero(const float a, const float t) { return t != 0.0f ? a + t : a; }
__device__ __forceinline__ unsigned abs_bits(const float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

__global__ __launch_bounds__(FOLD_THREADS) void uniq_fold_kernel(const float4* __restrict__ g, const unsigned* __restrict__ words,
                                                                 const unsigned* __restrict__ rows_u, float4* __restrict__ g_u,
                                                                 unsigned* __restrict__ absmax, int n_rows) {
    __shared__ unsigned wmax[FOLD_THREADS / 64];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * FOLD_THREADS + tid;
    const int n_eval = (int)words[0];
    unsigned m = 0u;
    if (c < n_rows) {
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (c < n_eval) {
            const int r0 = (int)rows_u[c], r1 = c + 1 < n_eval ? (int)rows_u[c + 1] : n_rows;
            acc = g[r0];
            for (int r = r0 + 1; r < r1; ++r) {      // (the run's interior rows, in row order)
                const float4 t = g[r];
                acc.x = add_nonzero(acc.x, t.x); acc.y = add_nonzero(acc.y, t.y);
                acc.z = add_nonzero(acc.z, t.z); acc.w = add_nonzero(acc.w, t.w);
            }
        }
        g_u[c] = acc;
        m = max(max(abs_bits(acc.x), abs_bits(acc.y)), max(abs_bits(acc.z), abs_bits(acc.w)));      // (non-negative floats and NaNs order as unsigned integers)
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < FOLD_THREADS / 64; ++w) m = max(m, wmax[w]);
        absmax[blockIdx.x] = m;      // (one plain store per workgroup; the gradient chain takes the maximum of the array)
    }
}

}  // namespace

namespace plnerf {
namespace impl {

int unique_list(const float* pts, const float* viewdirs, int n_rows, int spr, void* workspace, hipStream_t st) {
    if (n_rows < 1 || spr < 1) return PLNERF_EINVAL;
    const uniq::Workspace lo = uniq::workspace((size_t)n_rows);
    unsigned char* ws = (unsigned char*)workspace;
    const UniqArgs a{reinterpret_cast<const uint32_t*>(pts), reinterpret_cast<const uint32_t*>(viewdirs), n_rows, spr,
                     (unsigned*)(ws + lo.words), (unsigned*)(ws + lo.rows_u), (unsigned*)(ws + lo.src),
                     (uint32_t*)(ws + lo.pts_u), (uint32_t*)(ws + lo.dirs_u)};
    const int nb = uniq::blocks((size_t)n_rows);
    hipLaunchKernelGGL(uniq_count_kernel, dim3(nb), dim3(UB_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(uniq_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(uniq_scatter_kernel, dim3(nb), dim3(UB_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

int unique_expand(int n_rows, const void* workspace, float* raw_out, hipStream_t st) {
    const uniq::Workspace lo = uniq::workspace((size_t)n_rows);
    const unsigned char* ws = (const unsigned char*)workspace;
    hipLaunchKernelGGL(uniq_expand_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, st, (const float4*)(ws + lo.raw_u),
                       (const unsigned*)(ws + lo.src), (float4*)raw_out, n_rows);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

int unique_fold(const float* g_raw, int n_rows, void* workspace, hipStream_t st) {
    const uniq::Workspace lo = uniq::workspace((size_t)n_rows);
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL(uniq_fold_kernel, dim3(uniq::blocks((size_t)n_rows)), dim3(FOLD_THREADS), 0, st, (const float4*)g_raw,
                       (const unsigned*)(ws + lo.words), (const unsigned*)(ws + lo.rows_u), (float4*)(ws + lo.g_raw_u),
                       (unsigned*)(ws + lo.absmax), n_rows);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

}  // namespace impl
}  // namespace plnerf
