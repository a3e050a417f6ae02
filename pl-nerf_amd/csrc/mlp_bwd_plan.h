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

// ---- live rows (16-bit modes) --------------------------------------------------------------------------------------
// A row whose upstream gradient is (0, 0, 0, 0) has dz = 0 in every layer and adds nothing to any gradient: the backward
// runs over the LIVE rows only.  Ahead of dgrad a two-level scan (per-block counts, one workgroup's scan of them, an
// ordered scatter: mlp_live.hip) leaves the ascending indices of the rows whose four gradient floats are not all == 0.0f
// (a NaN row is live) and their number n_live in the workspace; dgrad writes dz of live row k at COMPACT row k of the
// unchanged planes, and every later reader takes its source rows (saved planes, upstream gradient) from the list.  The
// host never reads n_live: grids stay sized from n_rows, the row ranges below are taken again on the device from n_live.
//
// Where the list lives -- no section of its own, the workspace's size and sections are as they were: the partials
// section holds MAX_SPLITS slots, of which a 16-bit main launch writes only [0, MAIN_ROUND) (a network's share of the
// round is at most the round), and the thin launch, which may use every slot, writes nothing below PART_PE0 of a slot
// (its encoding and direction partials and L0's bias partial).  So floats [PART_MAIN, PART_PE0) of the slots
// [MAIN_ROUND, MAX_SPLITS) are written by no launch and read by none (the reduction reads a main-launch element of at
// most MAIN_ROUND slots): the list is chunked over their PART_MAIN areas, LIVE_CHUNK entries per slot, and the scan's
// words (n_live, the per-block counts) sit in the PART_VMAIN area of the first such slot.  Each network has a
// workspace of its own, so the two networks of a merged call cannot meet.  Where there is no room -- a build whose
// main round takes every slot, or more rows than the chunks hold -- live_list_fits() says so and the backward is dense.
constexpr int LIVE_SLOT0 = MAIN_ROUND;                              // first slot no main launch writes
constexpr int LIVE_SLOTS = lay::MAX_SPLITS - LIVE_SLOT0;
constexpr int LIVE_CHUNK_LOG2 = 19;
constexpr size_t LIVE_CHUNK = (size_t)1 << LIVE_CHUNK_LOG2;         // list entries (uint32) per slot: its PART_MAIN area
constexpr int LIVE_BLOCK_ROWS = 1024;                               // rows per workgroup of the count and scatter launches
constexpr int LIVE_N = 0;                                           // scan words: [LIVE_N] = n_live, [LIVE_COUNTS + b] = block b's count, then its offset
constexpr int LIVE_COUNTS = 16;
constexpr int LIVE_MAX_BLOCKS = lay::PART_PE0 - lay::PART_VMAIN - LIVE_COUNTS;
static_assert(LIVE_CHUNK <= (size_t)(lay::PART_VMAIN - lay::PART_MAIN) && LIVE_SLOT0 >= MAIN_ROUND && LIVE_SLOT0 + LIVE_SLOTS <= lay::MAX_SPLITS &&
              lay::PART_MAIN < lay::PART_VMAIN && lay::PART_VMAIN + LIVE_COUNTS + LIVE_MAX_BLOCKS <= lay::PART_PE0,
              "the live-row list and its scan words stay inside [PART_MAIN, PART_PE0) of slots no main launch writes");
static_assert(THIN_ROUND_ROWS <= lay::MAX_SPLITS && THIN_ROUND_TILED <= lay::MAX_SPLITS && lay::PART_PE0 < lay::PART_PE5 &&
              lay::PART_PE5 < lay::PART_VDIR && lay::PART_VDIR < lay::PART_BIAS,
              "everything a thin launch writes lies at or above PART_PE0 of its slot");
constexpr int live_blocks(size_t n_rows) { return (int)((n_rows + LIVE_BLOCK_ROWS - 1) / LIVE_BLOCK_ROWS); }
// the most rows the chunks and the count words hold (0: no slot is free)
constexpr size_t LIVE_MAX_ROWS = LIVE_SLOTS < 1 ? 0
                                 : ((size_t)LIVE_SLOTS * LIVE_CHUNK < (size_t)LIVE_MAX_BLOCKS * LIVE_BLOCK_ROWS ? (size_t)LIVE_SLOTS * LIVE_CHUNK
                                                                                                                 : (size_t)LIVE_MAX_BLOCKS * LIVE_BLOCK_ROWS);
constexpr bool live_list_fits(size_t n_rows) { return n_rows <= LIVE_MAX_ROWS && LIVE_MAX_ROWS > 0; }
// word offsets (4-byte units) from the start of the partials section
constexpr size_t live_entry_word(size_t i) {
    return (size_t)(LIVE_SLOT0 + (int)(i >> LIVE_CHUNK_LOG2)) * lay::PART_PER_SPLIT + lay::PART_MAIN + (i & (LIVE_CHUNK - 1));
}
constexpr size_t live_scan_word(int k) { return (size_t)LIVE_SLOT0 * lay::PART_PER_SPLIT + lay::PART_VMAIN + (size_t)k; }
// The row ranges and the head launch over the live rows: the same rules as above on n_live, evaluated by every workgroup
// and by the reduction alike (one text, compiled for both sides).  `launched`: the ranges the host launched for the
// network, row_ranges(n_rows, true, cap).splits -- NOT the dealt cap: rounding the length up can leave the host fewer
// ranges than its cap (262,144 rows at a cap of 73: 72 ranges), and fewer rows could then ask for more ranges than the
// grid has workgroups (73,729 live rows at a cap of 73: 73).  Without a live row there is no range: no workgroup
// writes a partial and the reduction adds none.  An empty head workgroup writes zeros, as above, and head_launch grows
// with its rows, so all of the host's n_head partials (sized from n_rows >= n_live) are written.
constexpr Ranges live_ranges(int n_live, int launched) { return n_live < 1 ? Ranges{0, 64} : row_ranges(n_live, true, launched); }
constexpr Head live_head(int n_live) { return head_launch(n_live < 0 ? 0 : n_live, true); }

}  // namespace bwdplan
}  // namespace plnerf
