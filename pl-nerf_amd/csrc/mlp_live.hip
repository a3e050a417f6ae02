// The live-row list of the 16-bit modes' MLP backward (mlp_bwd_plan.h: "live rows"): the ascending indices of the rows
// whose upstream gradient is not exactly (0, 0, 0, 0), and their number, left in the network's workspace ahead of dgrad.
//
// A two-level scan in three launches on the backward's stream, up to two networks per launch (blockIdx.y):
//   live_count_kernel     workgroup b counts the live rows among rows [1024 b, 1024 b + 1024)
//   live_scan_kernel      ONE workgroup per network turns the counts into exclusive offsets (in place) and leaves n_live
//   live_scatter_kernel   workgroup b takes its rows' flags again and writes its live rows' indices from its offset on
// Every position of the list is a pure function of the gradient: no atomics, the same list on every run; no workgroup
// waits for another inside a launch.  The host never reads n_live.
#include "common.h"
#include "mlp_bwd_plan.h"
#include "mlp_internal.h"

using namespace plnerf;

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_PER_THREAD = bwdplan::LIVE_BLOCK_ROWS / LB_THREADS;      // consecutive rows per thread: thread order = row order
static_assert(bwdplan::LIVE_BLOCK_ROWS % LB_THREADS == 0, "");
constexpr int SCAN_THREADS = 1024;

struct LiveNet {
    const float4* g;        // [n_rows] upstream gradient rows
    int n_rows;
    unsigned* words;        // the workspace's partials section as 4-byte words
};
struct LiveArgs {
    LiveNet n[impl::MAX_BWD_JOBS];
};

__device__ __forceinline__ bool row_live(const float4 v) {      // (a NaN compares unequal: live)
    return !(v.x == 0.0f && v.y == 0.0f && v.z == 0.0f && v.w == 0.0f);
}

// flags of the thread's LB_PER_THREAD consecutive rows (bit k = row base + k), rows past n_rows: not live
__device__ __forceinline__ unsigned thread_flags(const LiveNet& a, const int base) {
    unsigned f = 0u;
#pragma unroll
    for (int k = 0; k < LB_PER_THREAD; ++k) {
        const int row = base + k;
        if (row < a.n_rows && row_live(a.g[row])) f |= 1u << k;
    }
    return f;
}

__global__ __launch_bounds__(LB_THREADS) void live_count_kernel(LiveArgs p) {
    const LiveNet& a = p.n[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= bwdplan::live_blocks((size_t)a.n_rows)) return;      // (uniform: the grid is the larger network's)
    __shared__ int wsum[LB_THREADS / 64];
    const int tid = threadIdx.x;
    int c = __popc(thread_flags(a, b * bwdplan::LIVE_BLOCK_ROWS + tid * LB_PER_THREAD));
    c = wave_sum(c);
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < LB_THREADS / 64; ++w) s += wsum[w];
        a.words[bwdplan::live_scan_word(bwdplan::LIVE_COUNTS + b)] = (unsigned)s;
    }
}

// exclusive scan of one network's block counts, in place; thread t owns a run of consecutive counts
__global__ __launch_bounds__(SCAN_THREADS) void live_scan_kernel(LiveArgs p) {
    const LiveNet& a = p.n[blockIdx.x];
    const int nb = bwdplan::live_blocks((size_t)a.n_rows);
    const int per = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
    __shared__ unsigned wtot[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* cnt = a.words + bwdplan::live_scan_word(bwdplan::LIVE_COUNTS);
    const int i0 = tid * per, i1 = min(nb, i0 + per);
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
    if (tid == 0) a.words[bwdplan::live_scan_word(bwdplan::LIVE_N)] = total;
}

__global__ __launch_bounds__(LB_THREADS) void live_scatter_kernel(LiveArgs p) {
    const LiveNet& a = p.n[blockIdx.y];
    const int b = blockIdx.x;
    if (b >= bwdplan::live_blocks((size_t)a.n_rows)) return;      // (uniform)
    __shared__ unsigned wtot[LB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = b * bwdplan::LIVE_BLOCK_ROWS + tid * LB_PER_THREAD;
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
    unsigned pos = a.words[bwdplan::live_scan_word(bwdplan::LIVE_COUNTS + b)] + incl - mine;
#pragma unroll
    for (int w = 0; w < LB_THREADS / 64; ++w) pos += w < wave ? wtot[w] : 0u;
#pragma unroll
    for (int k = 0; k < LB_PER_THREAD; ++k)
        if (f & (1u << k)) a.words[bwdplan::live_entry_word(pos++)] = (unsigned)(base + k);
}

}  // namespace

namespace plnerf {
namespace impl {

int live_list(int n, const LiveJob* jobs, hipStream_t st) {
    if (n < 1 || n > MAX_BWD_JOBS) return PLNERF_EINVAL;
    LiveArgs a{};
    int blocks = 1;
    for (int j = 0; j < n; ++j) {
        if (!bwdplan::live_list_fits((size_t)jobs[j].n_rows)) return PLNERF_EINVAL;
        a.n[j] = LiveNet{reinterpret_cast<const float4*>(jobs[j].g_raw), jobs[j].n_rows, reinterpret_cast<unsigned*>(jobs[j].partials)};
        const int nb = bwdplan::live_blocks((size_t)jobs[j].n_rows);
        blocks = nb > blocks ? nb : blocks;
    }
    hipLaunchKernelGGL(live_count_kernel, dim3(blocks, n), dim3(LB_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(live_scan_kernel, dim3(n), dim3(SCAN_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(live_scatter_kernel, dim3(blocks, n), dim3(LB_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

}  // namespace impl
}  // namespace plnerf
