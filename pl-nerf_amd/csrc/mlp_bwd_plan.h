// What the host side of the MLP backward decides: the byte layout of the workspace a caller hands to plnerf_mlp_bwd and
// the launch plan of the weight-gradient stage and the dgrad grid -- row ranges per network, the deal of one round of
// workgroups over two networks, the head launch, the dgrad tiles.  Plain C++ -- no HIP include -- so that a host
// compiler can build it: tests/test_mlp_bwd_plan.py sweeps every decision made here.  mlp_api.hip carves the
// workspace through workspace(); mlp_wgrad.hip and mlp_h16_body.inc turn the plan into kernel arguments and grids.
#pragma once
#include <stddef.h>

#include "mlp_layout.h"

// Row ranges (split-K) of the 256-wide weight-gradient jobs.  Half planes: 8 tiles (L1..L7 and the composed view layer,
// mlp_layout.h; 9 tiles x 28 = 252 until round 5, when feature_linear had a job of its own) x 32 = 256 workgroups, ONE
// round on the 256 CUs (each keeps its 256 x 256 partial in registers for twice as many rows as with 56, and the partial
// sums written and re-read by the reduction halve: 134 -> 67 MB per network; step -1.5 %).  The fp32 kernel (17 tiles
// of 256 threads, several workgroups per CU) wants the 56 it was tuned with (28: +8 % step).
#ifndef PLNERF_WG_SPLITS
#define PLNERF_WG_SPLITS 32
#endif
#ifndef PLNERF_WG_SPLITS_F32
#define PLNERF_WG_SPLITS_F32 56
#endif

namespace plnerf {
namespace bwdplan {

// ---- workspace -------------------------------------------------------------------------------------------------
// [dz planes][scalars][split-K partials][head partials][G/s reduction][g_eff], byte offsets from the workspace's start:
//   dz         fp32 mode: DZ_PER_ROW floats per row; 16-bit modes: the half planes, rows padded to the dgrad tile
//   gmax       16-bit modes: max |g_raw| as fp32 bits (+ pad, WSH_SCALARS_BYTES); fp32 mode: an empty section
//   partials   MAX_SPLITS row ranges of PART_PER_SPLIT floats
//   head_part  MAX_HEAD_WGS workgroups of HEAD_PART floats
//   gred       the reduced G and s of the composed view layer (16-bit modes; the fp32 mode leaves it unused)
//   g_eff      [n_rows][4] floats: the upstream gradient after the density activation's derivative
struct Workspace {
    size_t dz, gmax, partials, head_part, gred, g_eff, total;
};
constexpr Workspace workspace(size_t n_rows, bool half) {
    Workspace w{};
    w.dz = 0;
    w.gmax = half ? (size_t)lay::DZH_BYTES_PER_ROW * lay::dz_rows(n_rows) : (size_t)lay::DZ_PER_ROW * n_rows * sizeof(float);
    w.partials = w.gmax + (half ? (size_t)lay::WSH_SCALARS_BYTES : 0);
    w.head_part = w.partials + (size_t)lay::MAX_SPLITS * lay::PART_PER_SPLIT * sizeof(float);
    w.gred = w.head_part + (size_t)lay::MAX_HEAD_WGS * lay::HEAD_PART * sizeof(float);
    w.g_eff = w.gred + (size_t)lay::GRED_FLOATS * sizeof(float);
    w.total = w.g_eff + n_rows * 16;
    return w;
}
static_assert(lay::DZH_BYTES_PER_ROW % 16 == 0 && (lay::DZ_PER_ROW * sizeof(float)) % 16 == 0 && lay::WSH_SCALARS_BYTES % 16 == 0 &&
              (lay::PART_PER_SPLIT * sizeof(float)) % 16 == 0 && (lay::MAX_HEAD_WGS * lay::HEAD_PART * sizeof(float)) % 16 == 0 &&
              (lay::GRED_FLOATS * sizeof(float)) % 16 == 0, "every section of the workspace starts on a 16-byte boundary");

// ---- rounds of row ranges ----------------------------------------------------------------------------------------
// A launch's row ranges are the y extent of its grid; a round is what one or two networks share of it.  The thin
// launch has three tiles only (tiled saved planes: two -- the direction columns ride on the main launch's view job), so
// more row ranges than the main launch to cover the 256 CUs: 3 x 85 = 255, 2 x 127 = 254 workgroups.
constexpr int MAIN_ROUND = PLNERF_WG_SPLITS;
constexpr int F32_SPLITS = PLNERF_WG_SPLITS_F32;      // exact-fp32 mode: one network per launch, main and thin alike
constexpr int THIN_TILES_ROWS = 3, THIN_ROUND_ROWS = 85;
constexpr int THIN_TILES_TILED = 2, THIN_ROUND_TILED = 127;
constexpr int thin_tiles(bool all_tiled) { return all_tiled ? THIN_TILES_TILED : THIN_TILES_ROWS; }
constexpr int thin_round(bool all_tiled) { return all_tiled ? THIN_ROUND_TILED : THIN_ROUND_ROWS; }
// the partials section holds MAX_SPLITS ranges: a larger round would write past it
static_assert(MAIN_ROUND >= 1 && MAIN_ROUND <= lay::MAX_SPLITS, "PLNERF_WG_SPLITS overruns the workspace's partials");
static_assert(F32_SPLITS >= 1 && F32_SPLITS <= lay::MAX_SPLITS, "PLNERF_WG_SPLITS_F32 overruns the workspace's partials");
static_assert(THIN_ROUND_ROWS <= lay::MAX_SPLITS && THIN_ROUND_TILED <= lay::MAX_SPLITS, "");

// The ranges one network launches when it may use `cap` of a round: about 1,024 rows each until the cap is reached,
// the length rounded to whole 64-row stages (half kernels: two tiles of the tiled layout) or 16 rows (fp32).
// Rounding the length up can leave the LAST ranges without a row (131,072 rows over 85 ranges of 1,600: ranges 82..84
// start past the end).  A workgroup without rows writes no partial, and the reduction would add whatever the workspace
// held there (round 4: found by comparing two schedules of the same step bit for bit) -- so the ranges are counted
// again after the rounding: only ranges that hold a row are launched and summed.
struct Ranges {
    int splits, rows_per_split;
};
constexpr Ranges row_ranges(int n_rows, bool half, int cap) {
    int splits = (n_rows + 1023) / 1024;
    splits = splits < 1 ? 1 : (splits > cap ? cap : splits);
    int rps = (n_rows + splits - 1) / splits;
    rps = half ? (rps + 63) & ~63 : (rps + 15) & ~15;
    return Ranges{(n_rows + rps - 1) / rps, rps};
}

// One round dealt over two networks in proportion to their rows, each at least one range.  (n_rows1 = 0: a single
// network, all of the round.)
struct Deal {
    int cap[2];
};
constexpr Deal deal(int round, int n_rows0, int n_rows1) {
    if (n_rows1 <= 0) return Deal{{round, 0}};
    const double f = (double)n_rows0 / ((double)n_rows0 + (double)n_rows1);
    int s0 = (int)(round * f + 0.5);
    s0 = s0 < 1 ? 1 : (s0 > round - 1 ? round - 1 : s0);
    return Deal{{s0, round - s0}};
}

// ---- head launch: sigma / rgb head rows, about 256 rows per workgroup ---------------------------------------------
// Half planes: whole 32-row tiles per workgroup.  That rounding can leave the last workgroups without a row (131,073
// rows: 512 workgroups of 288 rows, the last 56 empty); unlike a row range of the split-K launches an empty head
// workgroup writes its partial -- zeros -- so all n_head partials are summed.
constexpr int HEAD_CAP = lay::MAX_HEAD_WGS;
static_assert(HEAD_CAP == lay::MAX_HEAD_WGS, "the workspace's head section holds one partial per head workgroup");
struct Head {
    int n_head, rows_per_head_wg;
};
constexpr Head head_launch(int n_rows, bool half) {
    int n = (n_rows + 255) / 256;
    n = n < 1 ? 1 : (n > HEAD_CAP ? HEAD_CAP : n);
    const int rows = (n_rows + n - 1) / n;
    return Head{n, half ? (rows + 31) & ~31 : rows};
}

// ---- dgrad grid of the 16-bit modes: workgroup tiles of one network (two networks share a grid) -------------------
constexpr int dgrad_tiles(int n_rows) { return (n_rows + lay::DZ_ROW_PAD - 1) / lay::DZ_ROW_PAD; }

}  // namespace bwdplan
}  // namespace plnerf
