// Mesh extraction (include/experimental/plnerf_hip_mesh.h).
//
// plnerf_density_grid: extract_fields (nerf_extract_mesh.py:531-562) as one call.  Per block of at most max_rows consecutive
// lattice indices
//   grid_points_kernel   the block's positions (xs[x], ys[y], zs[z]) and ONE zero view direction into the workspace
//   (the slot's forward: plnerf_mlp_fwd, or plnerf_embed_rows + plnerf_generic_fwd / _f32 -- no MLP kernel is written here)
//   grid_store_kernel    field = max(raw[3], 0), and each workgroup's (min, max, sum, sum of squares) of its 1,024 rows
// and behind the last block grid_stats_kernel, one workgroup, adds the partials in index order.
//
// plnerf_mc_count / plnerf_mc_emit: indexed marching cubes on the generated table mc_table.h, built like mlp_live.hip /
// mlp_unique.hip: count -> scan -> scan as separate launches, no workgroup waits for another inside a launch, no atomics, every
// offset a pure function of the field.
//   mc_count_kernel   workgroup b takes lattice points [1024 b, 1024 b + 1024): per point its crossing flags along x, y, z
//                     (64-lane ballots give the offsets inside a wave) and the triangles of the cell it is the corner of;
//                     word[p] = the point's vertex offset inside the block | flags << 12, and the block's two totals
//   mc_scan_kernel    workgroup g turns the totals of blocks [1024 g, 1024 g + 1024) into exclusive offsets, in place, and
//                     leaves its own totals; launched a second time, as ONE workgroup, over those: the counts
//   mc_emit_kernel    workgroup b again: its points' vertices from word[p], and its cells' triangles from the cell's offset
//                     inside the block (recomputed as mc_count_kernel computed it) -- a triangle's corner on the edge owned
//                     by lattice point q along axis a is word[q]'s offset + the flags of q below a + q's block's offsets
#include "anyview_slot.h"
#include "../../include/experimental/plnerf_hip_mesh.h"
#define PLNERF_MC_TABLE_QUALIFIER __device__
#include "mc_table.h"

using namespace plnerf;

namespace {

using namespace plnerf_step;

// ================================================================================================ the density lattice
constexpr int STORE_THREADS = 256;
constexpr int STORE_ROWS = 1024;      // rows per workgroup of grid_store_kernel = rows per stats partial
constexpr uint64_t MAX_POINTS = 1ull << 30;

struct GridPlan {
    float *pts, *dir, *raw;
    double* partials;
    float* embedded;
    void* net_ws;
    size_t net_ws_bytes;
    int rows;              // of a full block
    size_t n_partials;
    size_t bytes;
};

size_t partials_of(uint64_t n, int rows) {
    const uint64_t per = ((uint64_t)rows + STORE_ROWS - 1) / STORE_ROWS, rest = n % (uint64_t)rows;
    return (size_t)(n / (uint64_t)rows * per + (rest + STORE_ROWS - 1) / STORE_ROWS);
}

GridPlan carve(const plnerf_anyview_net& net, int cols, uint64_t n, int rows, void* workspace) {
    Carver w{(unsigned char*)workspace, 0};
    GridPlan p{};
    p.rows = rows;
    p.pts = w.floats(3 * (size_t)rows);
    p.dir = w.floats(3);
    p.raw = w.floats(4 * (size_t)rows);
    p.n_partials = partials_of(n, rows);
    p.partials = w.take<double>(p.n_partials * PLNERF_GRID_STATS * sizeof(double));
    if (generic(net)) {
        p.embedded = w.floats((size_t)rows * (size_t)cols);
        p.net_ws_bytes = net_workspace_bytes(net, rows);
        p.net_ws = w.take<void>(p.net_ws_bytes);
    }
    p.bytes = w.off;
    return p;
}

// everything that can be judged without following a pointer of `net`: PLNERF_OK, the slot's encoding, the lattice's points and
// a full block's rows
int check_grid(const plnerf_anyview_net* net, int precision, int input_ch, int input_ch_views, int resolution, int max_rows,
               Encoding& enc, uint64_t& n, int& rows) {
    if (!net || resolution < 2 || max_rows < 1) return PLNERF_EINVAL;
    if (net->route != PLNERF_ANYVIEW_FUSED && !generic(*net)) return PLNERF_EINVAL;
    if ((uint64_t)resolution > 1024) return PLNERF_ERANGE;      // (1024^3 = 2^30)
    n = (uint64_t)resolution * (uint64_t)resolution * (uint64_t)resolution;
    if (n > MAX_POINTS) return PLNERF_ERANGE;
    rows = n < (uint64_t)max_rows ? (int)n : max_rows;
    if (net->route == PLNERF_ANYVIEW_FUSED) {
        // the in-kernel encoding's widths and the row count's limit, as check_pass() holds the one-call entries to them
        if (input_ch < 3 || input_ch > 63 || (input_ch - 3) % 6 != 0 || input_ch_views < 3 || input_ch_views > 27 ||
            (input_ch_views - 3) % 6 != 0)
            return PLNERF_EINVAL;
        if (plnerf_mlp_packed_bytes(precision) == 0) return PLNERF_ENOSYS;
        if (rows > INT32_MAX / 4) return PLNERF_ERANGE;
        enc = Encoding{(input_ch - 3) / 6, (input_ch_views - 3) / 6, input_ch + input_ch_views};
        return PLNERF_OK;
    }
    return check_shape(*net, rows, enc);
}

__global__ __launch_bounds__(256) void grid_points_kernel(const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ zs, const unsigned res, const unsigned i0,
                                                          const int rows, float* __restrict__ pts, float* __restrict__ dir) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 3 && blockIdx.x == 0) dir[i] = 0.0f;
    if (i >= rows) return;
    const unsigned idx = i0 + (unsigned)i;      // (< 2^30)
    const unsigned z = idx % res, xy = idx / res, y = xy % res, x = xy / res;
    pts[3 * (size_t)i + 0] = xs[x];
    pts[3 * (size_t)i + 1] = ys[y];
    pts[3 * (size_t)i + 2] = zs[z];
}

struct Stats { double mn, mx, sum, sq; };

__device__ __forceinline__ void stats_add(Stats& s, const Stats& o) {
    s.mn = o.mn < s.mn ? o.mn : s.mn;
    s.mx = o.mx > s.mx ? o.mx : s.mx;
    s.sum += o.sum;
    s.sq += o.sq;
}

// the workgroup's stats in thread 0, added in a fixed order: lanes by xor butterflies, then the waves in wave order
template <int THREADS>
__device__ __forceinline__ Stats stats_reduce(Stats s) {
    __shared__ Stats per_wave[THREADS / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Stats o{__shfl_xor(s.mn, d), __shfl_xor(s.mx, d), __shfl_xor(s.sum, d), __shfl_xor(s.sq, d)};
        stats_add(s, o);
    }
    if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < THREADS / 64; ++w) stats_add(s, per_wave[w]);
    return s;
}

__device__ __forceinline__ Stats stats_none() { return Stats{__builtin_inf(), -__builtin_inf(), 0.0, 0.0}; }

__global__ __launch_bounds__(STORE_THREADS) void grid_store_kernel(const float* __restrict__ raw, const int rows,
                                                                   float* __restrict__ field, double* __restrict__ partials) {
    Stats s = stats_none();
#pragma unroll
    for (int k = 0; k < STORE_ROWS / STORE_THREADS; ++k) {
        const int r = blockIdx.x * STORE_ROWS + k * STORE_THREADS + threadIdx.x;
        if (r >= rows) break;
        const float v = raw[4 * (size_t)r + 3];
        const float d = v > 0.0f ? v : (v != v ? v : 0.0f);      // relu: a NaN stays one
        field[r] = d;
        const double x = (double)d;
        stats_add(s, Stats{x == x ? x : __builtin_inf(), x == x ? x : -__builtin_inf(), x, x * x});
    }
    if (!partials) return;      // (uniform)
    s = stats_reduce<STORE_THREADS>(s);
    if (threadIdx.x == 0) {
        double* out = partials + (size_t)blockIdx.x * PLNERF_GRID_STATS;
        out[PLNERF_GRID_MIN] = s.mn; out[PLNERF_GRID_MAX] = s.mx; out[PLNERF_GRID_SUM] = s.sum; out[PLNERF_GRID_SUMSQ] = s.sq;
    }
}

__global__ __launch_bounds__(STORE_THREADS) void grid_stats_kernel(const double* __restrict__ partials, const size_t n_partials,
                                                                   double* __restrict__ stats) {
    Stats s = stats_none();
    for (size_t j = threadIdx.x; j < n_partials; j += STORE_THREADS) {
        const double* p = partials + j * PLNERF_GRID_STATS;
        stats_add(s, Stats{p[PLNERF_GRID_MIN], p[PLNERF_GRID_MAX], p[PLNERF_GRID_SUM], p[PLNERF_GRID_SUMSQ]});
    }
    s = stats_reduce<STORE_THREADS>(s);
    if (threadIdx.x == 0) {
        stats[PLNERF_GRID_MIN] = s.mn; stats[PLNERF_GRID_MAX] = s.mx; stats[PLNERF_GRID_SUM] = s.sum; stats[PLNERF_GRID_SUMSQ] = s.sq;
    }
}

// ================================================================================================ marching cubes
constexpr int MC_THREADS = 256;
constexpr int MC_BLOCK = 1024;                          // lattice points per workgroup
constexpr int MC_CHUNKS = MC_BLOCK / MC_THREADS;        // a thread's points: chunk i holds points base + 256 i + tid
constexpr int MC_PARTS = MC_CHUNKS * (MC_THREADS / 64); // (chunk, wave) pairs of a block, in point order
constexpr int SCAN_THREADS = 1024;                      // = blocks per workgroup of mc_scan_kernel
constexpr unsigned OFFSET_BITS = 12, OFFSET_MASK = (1u << OFFSET_BITS) - 1u;      // a block holds at most 3,072 vertices
static_assert(3 * MC_BLOCK <= (1 << OFFSET_BITS), "");

struct McArgs {
    const float* f;
    unsigned nx, ny, nz, n;      // n = nx ny nz <= 2^30
    double iso;
    uint32_t* word;              // [n]
    uint32_t *bv, *bt;           // [nb]: the blocks' vertex / triangle totals, then offsets inside their group of 1,024 blocks
    uint32_t *sv, *st;           // [ns]: the groups' totals, then offsets
    unsigned nb, ns;
};

struct McLayout { size_t word, bv, bt, sv, st, total; unsigned nb, ns; };

McLayout mc_layout(uint64_t n) {
    McLayout lo{};
    lo.nb = (unsigned)((n + MC_BLOCK - 1) / MC_BLOCK);
    lo.ns = (lo.nb + SCAN_THREADS - 1) / SCAN_THREADS;      // (<= 1,024: one workgroup scans the groups)
    const auto up = [](size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; };
    size_t off = 0;
    lo.word = off; off += up((size_t)n * 4);
    lo.bv = off; off += up((size_t)lo.nb * 4);
    lo.bt = off; off += up((size_t)lo.nb * 4);
    lo.sv = off; off += up((size_t)lo.ns * 4);
    lo.st = off; off += up((size_t)lo.ns * 4);
    lo.total = off;
    return lo;
}

__device__ __forceinline__ bool mc_inside(const McArgs& a, const size_t idx) { return (double)a.f[idx] >= a.iso; }

// lattice point p: its crossing flags (bit k: the edge from p along axis k crosses) and, where p is the low corner of a cell,
// that cell's state; returns whether it is
__device__ __forceinline__ bool mc_point(const McArgs& a, const unsigned p, unsigned& flags, unsigned& state) {
    const unsigned z = p % a.nz, xy = p / a.nz, y = xy % a.ny, x = xy / a.ny;
    const size_t sx = (size_t)a.ny * a.nz, sy = a.nz;
    const bool hx = x + 1 < a.nx, hy = y + 1 < a.ny, hz = z + 1 < a.nz;
    const bool in0 = mc_inside(a, p);
    flags = 0u;
    state = 0u;
    if (hx && hy && hz) {
#pragma unroll
        for (int i = 0; i < 8; ++i)      // corner i at (i & 1, (i >> 1) & 1, (i >> 2) & 1) along (x, y, z)
            state |= (unsigned)mc_inside(a, (size_t)p + (i & 1 ? sx : 0) + (i & 2 ? sy : 0) + (i & 4 ? 1 : 0)) << i;
        flags = (((state >> 1) ^ state) & 1u) | ((((state >> 2) ^ state) & 1u) << 1) | ((((state >> 4) ^ state) & 1u) << 2);
        return true;
    }
    if (hx && mc_inside(a, (size_t)p + sx) != in0) flags |= 1u;
    if (hy && mc_inside(a, (size_t)p + sy) != in0) flags |= 2u;
    if (hz && mc_inside(a, (size_t)p + 1) != in0) flags |= 4u;
    return false;
}

__device__ __forceinline__ unsigned wave_incl_sum_u32(unsigned v) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d);
        if (l >= d) v += o;
    }
    return v;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(McArgs a) {
    __shared__ unsigned cv[MC_PARTS], ct[MC_PARTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned base = blockIdx.x * (unsigned)MC_BLOCK;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned flags[MC_CHUNKS], before[MC_CHUNKS];
#pragma unroll
    for (int i = 0; i < MC_CHUNKS; ++i) {
        const unsigned p = base + i * MC_THREADS + tid;
        unsigned state = 0u, nt = 0u;
        flags[i] = 0u;
        if (p < a.n && mc_point(a, p, flags[i], state)) nt = plnerf_mc_ntri[state];
        // vertices are numbered by point, then axis: a lane's offset inside its wave is every flag of the lanes below it
        const unsigned long long b0 = __ballot(flags[i] & 1u), b1 = __ballot(flags[i] & 2u), b2 = __ballot(flags[i] & 4u);
        before[i] = __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
        const unsigned t_all = wave_sum(nt);
        if (lane == 0) {
            cv[i * (MC_THREADS / 64) + wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
            ct[i * (MC_THREADS / 64) + wave] = t_all;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MC_CHUNKS; ++i) {
        const unsigned p = base + i * MC_THREADS + tid;
        unsigned off = before[i];
        for (int j = 0; j < i * (MC_THREADS / 64) + wave; ++j) off += cv[j];
        if (p < a.n) a.word[p] = off | (flags[i] << OFFSET_BITS);
    }
    if (tid == 0) {
        unsigned v = 0u, t = 0u;
        for (int j = 0; j < MC_PARTS; ++j) { v += cv[j]; t += ct[j]; }
        a.bv[blockIdx.x] = v;
        a.bt[blockIdx.x] = t;
    }
}

// Exclusive scan, in place, of cnt_v / cnt_t [count] in groups of SCAN_THREADS (one per workgroup); the groups' totals go to
// tot_v / tot_t [gridDim.x] -- as 32-bit words, saturated at 0xFFFFFFFF, when `final` (the one-workgroup second level, whose
// sums may pass 2^32: its offsets then wrap, and the caller is told by the saturated count).
__global__ __launch_bounds__(SCAN_THREADS) void mc_scan_kernel(uint32_t* __restrict__ cnt_v, uint32_t* __restrict__ cnt_t,
                                                               const unsigned count, uint32_t* __restrict__ tot_v,
                                                               uint32_t* __restrict__ tot_t, const int final) {
    __shared__ unsigned long long wv[SCAN_THREADS / 64], wt[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned i = blockIdx.x * (unsigned)SCAN_THREADS + tid;
    const unsigned v = i < count ? cnt_v[i] : 0u, t = i < count ? cnt_t[i] : 0u;
    // (a group's sums fit 32 bits below the final level: 1,024 blocks of at most 3,072 vertices / 5,120 triangles)
    unsigned long long iv = v, it = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long ov = __shfl_up(iv, d), ot = __shfl_up(it, d);
        if (lane >= d) { iv += ov; it += ot; }
    }
    if (lane == 63) { wv[wave] = iv; wt[wave] = it; }
    __syncthreads();
    unsigned long long bv = 0ull, bt = 0ull, all_v = 0ull, all_t = 0ull;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
        bv += w < wave ? wv[w] : 0ull;
        bt += w < wave ? wt[w] : 0ull;
        all_v += wv[w];
        all_t += wt[w];
    }
    if (i < count) {
        cnt_v[i] = (uint32_t)(bv + iv - v);
        cnt_t[i] = (uint32_t)(bt + it - t);
    }
    if (tid == 0) {
        const unsigned long long cap = 0xFFFFFFFFull;
        tot_v[blockIdx.x] = (uint32_t)(final && all_v > cap ? cap : all_v);
        tot_t[blockIdx.x] = (uint32_t)(final && all_t > cap ? cap : all_t);
    }
}

// the index of the vertex on the edge lattice point q owns along `axis`
__device__ __forceinline__ unsigned mc_vertex_index(const McArgs& a, const unsigned q, const unsigned axis) {
    const unsigned w = a.word[q], b = q / MC_BLOCK;
    return (w & OFFSET_MASK) + __popc((w >> OFFSET_BITS) & ((1u << axis) - 1u)) + a.bv[b] + a.sv[b / SCAN_THREADS];
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_kernel(McArgs a, double* __restrict__ vertices, const unsigned cap_v,
                                                             int32_t* __restrict__ triangles, const unsigned cap_t) {
    __shared__ unsigned ct[MC_PARTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned base = blockIdx.x * (unsigned)MC_BLOCK;
    const unsigned strides[3] = {a.ny * a.nz, a.nz, 1u};
    unsigned state[MC_CHUNKS], nt[MC_CHUNKS], before[MC_CHUNKS];
#pragma unroll
    for (int i = 0; i < MC_CHUNKS; ++i) {
        const unsigned p = base + i * MC_THREADS + tid;
        unsigned flags = 0u;
        state[i] = 0u;
        nt[i] = 0u;
        if (p < a.n && mc_point(a, p, flags, state[i])) nt[i] = plnerf_mc_ntri[state[i]];
        const unsigned incl = wave_incl_sum_u32(nt[i]);
        before[i] = incl - nt[i];
        if (lane == 63) ct[i * (MC_THREADS / 64) + wave] = incl;
        if (p >= a.n || !flags) continue;
        // ---- this point's vertices, axis by axis
        unsigned at = mc_vertex_index(a, p, 0u);
        const unsigned z = p % a.nz, xy = p / a.nz, y = xy % a.ny, x = xy / a.ny;
        const double f1 = (double)a.f[p];
#pragma unroll
        for (unsigned axis = 0; axis < 3; ++axis) {
            if (!(flags & (1u << axis))) continue;
            if (at < cap_v) {
                const double f2 = (double)a.f[(size_t)p + strides[axis]];
                const double t = (a.iso - f1) / (f2 - f1);
                double c[3] = {(double)x, (double)y, (double)z};
                c[axis] = c[axis] + t;
                double* out = vertices + 3 * (size_t)at;
                out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
            }
            ++at;
        }
    }
    __syncthreads();
    const unsigned block_at = a.bt[blockIdx.x] + a.st[blockIdx.x / SCAN_THREADS];
#pragma unroll
    for (int i = 0; i < MC_CHUNKS; ++i) {
        if (!nt[i]) continue;
        const unsigned p = base + i * MC_THREADS + tid;
        unsigned at = block_at + before[i];
        for (int j = 0; j < i * (MC_THREADS / 64) + wave; ++j) at += ct[j];
        for (unsigned k = 0; k < nt[i]; ++k, ++at) {
            if (at >= cap_t) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // edge e = 4 axis + u + 2 v: along `axis` from the corner with offsets (u, v) along the other two axes
                const unsigned e = (unsigned)plnerf_mc_tri[state[i]][3 * k + c];
                const unsigned axis = e >> 2, u = e & 1u, v = (e >> 1) & 1u;
                const unsigned q = p + u * strides[axis == 0 ? 1 : 0] + v * strides[axis == 2 ? 1 : 2];
                triangles[3 * (size_t)at + c] = (int32_t)mc_vertex_index(a, q, axis);
            }
        }
    }
}

int mc_check(const float* field, int nx, int ny, int nz, double iso, const void* workspace, size_t workspace_bytes, McLayout& lo) {
    if (!field || !workspace || ((uintptr_t)workspace % ALIGN) != 0 || nx < 2 || ny < 2 || nz < 2 || iso != iso) return PLNERF_EINVAL;
    const uint64_t n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    if (n > MAX_POINTS) return PLNERF_ERANGE;
    lo = mc_layout(n);
    return workspace_bytes < lo.total ? PLNERF_EINVAL : PLNERF_OK;
}

McArgs mc_args(const float* field, int nx, int ny, int nz, double iso, const void* workspace, const McLayout& lo) {
    unsigned char* ws = (unsigned char*)const_cast<void*>(workspace);
    return McArgs{field, (unsigned)nx, (unsigned)ny, (unsigned)nz, (unsigned)((uint64_t)nx * ny * nz), iso,
                  (uint32_t*)(ws + lo.word), (uint32_t*)(ws + lo.bv), (uint32_t*)(ws + lo.bt), (uint32_t*)(ws + lo.sv),
                  (uint32_t*)(ws + lo.st), lo.nb, lo.ns};
}

}  // namespace

extern "C" size_t plnerf_density_grid_workspace_bytes(const plnerf_anyview_net* net, int precision, int input_ch, int input_ch_views,
                                                      int resolution, int max_rows) {
    Encoding enc{};
    uint64_t n = 0;
    int rows = 0;
    if (check_grid(net, precision, input_ch, input_ch_views, resolution, max_rows, enc, n, rows) != PLNERF_OK) return 0;
    return carve(*net, enc.cols, n, rows, nullptr).bytes;
}

extern "C" int plnerf_density_grid(const plnerf_anyview_net* net, int precision, int input_ch, int input_ch_views, int resolution,
                                   const float* xs, const float* ys, const float* zs, int max_rows, int pack_weights, float* field,
                                   double* stats, void* workspace, size_t workspace_bytes, plnerf_stream_t stream) {
    // ---- every check first: a refused call enqueues nothing ----
    Encoding enc{};
    uint64_t n = 0;
    int rows = 0;
    int rc = check_grid(net, precision, input_ch, input_ch_views, resolution, max_rows, enc, n, rows);
    if (rc) return rc;
    if (!xs || !ys || !zs || !field || !workspace || ((uintptr_t)workspace % ALIGN) != 0) return PLNERF_EINVAL;
    if ((rc = check_slot(*net, enc.cols))) return rc;
    const GridPlan p = carve(*net, enc.cols, n, rows, workspace);
    if (workspace_bytes < p.bytes) return PLNERF_EINVAL;
    const bool fused = net->route == PLNERF_ANYVIEW_FUSED;
    if (fused && (rc = check_params_aligned(net->fused.params))) return rc;

    hipStream_t st = (hipStream_t)stream;
    if (fused && pack_weights)
        STEP_OK(plnerf_mlp_pack_weights(net->fused.params, precision, input_ch, input_ch_views, net->fused.packed, stream));
    size_t partial = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += (uint64_t)rows) {
        const int m = n - i0 < (uint64_t)rows ? (int)(n - i0) : rows;
        hipLaunchKernelGGL(grid_points_kernel, dim3((m + 255) / 256), dim3(256), 0, st, xs, ys, zs, (unsigned)resolution, (unsigned)i0, m,
                           p.pts, p.dir);
        PLNERF_CHECK_LAUNCH();
        // the block is one ray of m samples: every row reads the one zero direction
        if (fused) {
            STEP_OK(plnerf_mlp_fwd(net->fused.packed, precision, p.pts, p.dir, nullptr, input_ch, input_ch_views, m, m, 1.0f, 0.0f, p.raw,
                                   nullptr, PLNERF_FWD_KERNEL_AUTO, stream));
        } else {
            STEP_OK(plnerf_embed_rows(p.pts, p.dir, nullptr, m, m, enc.L, enc.M, 0, 1.0f, nullptr, 1.0f, p.embedded, stream));
            if (net->route == PLNERF_ANYVIEW_CHAIN16)
                STEP_OK(plnerf_generic_fwd(&net->shape, net->params, p.embedded, enc.cols, m, net->precision, p.net_ws, p.net_ws_bytes,
                                           p.raw, 4, net->status, stream));
            else
                STEP_OK(plnerf_generic_fwd_f32(&net->shape, net->params, p.embedded, enc.cols, m, p.net_ws, p.net_ws_bytes, p.raw, 4,
                                               stream));
        }
        const int groups = (m + STORE_ROWS - 1) / STORE_ROWS;
        hipLaunchKernelGGL(grid_store_kernel, dim3(groups), dim3(STORE_THREADS), 0, st, p.raw, m, field + i0,
                           stats ? p.partials + partial * PLNERF_GRID_STATS : nullptr);
        PLNERF_CHECK_LAUNCH();
        partial += (size_t)groups;
    }
    if (stats) {
        hipLaunchKernelGGL(grid_stats_kernel, dim3(1), dim3(STORE_THREADS), 0, st, p.partials, partial, stats);
        PLNERF_CHECK_LAUNCH();
    }
    return PLNERF_OK;
}

extern "C" size_t plnerf_mc_workspace_bytes(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const uint64_t n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    return n > MAX_POINTS ? 0 : mc_layout(n).total;
}

extern "C" int plnerf_mc_count(const float* field, int nx, int ny, int nz, double iso, void* workspace, size_t workspace_bytes,
                               uint32_t* counts, plnerf_stream_t stream) {
    McLayout lo{};
    const int rc = mc_check(field, nx, ny, nz, iso, workspace, workspace_bytes, lo);
    if (rc) return rc;
    if (!counts) return PLNERF_EINVAL;
    const McArgs a = mc_args(field, nx, ny, nz, iso, workspace, lo);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_count_kernel, dim3(lo.nb), dim3(MC_THREADS), 0, st, a);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_scan_kernel, dim3(lo.ns), dim3(SCAN_THREADS), 0, st, a.bv, a.bt, lo.nb, a.sv, a.st, 0);
    PLNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, a.sv, a.st, lo.ns, counts, counts + 1, 1);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}

extern "C" int plnerf_mc_emit(const float* field, int nx, int ny, int nz, double iso, const void* workspace, size_t workspace_bytes,
                              double* vertices, int64_t cap_vertices, int32_t* triangles, int64_t cap_triangles,
                              plnerf_stream_t stream) {
    McLayout lo{};
    const int rc = mc_check(field, nx, ny, nz, iso, workspace, workspace_bytes, lo);
    if (rc) return rc;
    if (cap_vertices < 0 || cap_triangles < 0 || (cap_vertices > 0 && !vertices) || (cap_triangles > 0 && !triangles)) return PLNERF_EINVAL;
    if (cap_vertices > INT32_MAX || cap_triangles > INT32_MAX) return PLNERF_ERANGE;
    if (cap_vertices == 0 && cap_triangles == 0) return PLNERF_OK;
    const McArgs a = mc_args(field, nx, ny, nz, iso, workspace, lo);
    hipLaunchKernelGGL(mc_emit_kernel, dim3(lo.nb), dim3(MC_THREADS), 0, (hipStream_t)stream, a, vertices, (unsigned)cap_vertices,
                       triangles, (unsigned)cap_triangles);
    PLNERF_CHECK_LAUNCH();
    return PLNERF_OK;
}
