// What the host side of the fine pass's unique-row forward decides (mlp_unique.hip): which rows are evaluated, who is
// served, and the byte layout of the workspace a caller hands to plnerf_mlp_fwd_unique.  Plain C++ -- no HIP include -- so
// that a host compiler can build it (tests/test_fwd_unique_host.py).
//
// The rule.  Row i of a launch of n_rows rows, spr consecutive rows per ray, is INTERIOR when rows i - 1 and i + 1 belong to
// its ray (the same row / spr) and pts[i - 1], pts[i], pts[i + 1] are equal BITWISE in all three components (+0.0 and -0.0
// are different inputs).  Equal position on one ray is equal direction: an identical network input.  Interior rows are
// not evaluated: their output is a copy of the run's first row.  Both ends of a run, and the first and last row of every
// ray, are evaluated -- an interior row borders zero-length intervals only, so the rows that carry a gradient, and their
// order, are those of the plain forward, and with them the backward's live list, tiles and ranges.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlp_bwd_plan.h"
#include "mlp_fwd_route.h"
#include "mlp_layout.h"

namespace plnerf {
namespace uniq {

constexpr int BLOCK_ROWS = 1024;      // rows per workgroup of the count / scatter launches, compact rows per workgroup of the fold
constexpr int SCAN_WORDS = 16;        // words[0] = n_eval; words[SCAN_WORDS + b] = block b's count, then its offset
constexpr int blocks(size_t n_rows) { return (int)((n_rows + BLOCK_ROWS - 1) / BLOCK_ROWS); }
// the compact buffers are filled to whole forward tiles: the largest workgroup tile of the register-resident kernel
constexpr size_t FILL = lay::SV_ROW_PAD;
constexpr size_t padded(size_t n_rows) { return lay::sv_rows(n_rows); }

// byte offsets from the workspace's start; every section starts on a 256-byte boundary
struct Workspace {
    size_t words;        // uint32 [SCAN_WORDS + blocks]: n_eval and the scan
    size_t rows_u;       // uint32 [padded]: original row of compact row c (c < n_eval)
    size_t src;          // uint32 [padded]: compact row whose output row takes = (evaluated rows in [0, row]) - 1
    size_t pts_u;        // float [padded][3]: pts of the compact rows, filled to the next multiple of FILL with the last one
    size_t dirs_u;       // float [padded][3]: their directions, one per row
    size_t raw_u;        // float [padded][4]: the forward's output in compact order
    size_t g_raw_u;      // float [padded][4]: the folded upstream gradient (rows past n_eval: zero)
    size_t absmax;       // uint32 [blocks]: max |g_raw_u| per fold workgroup as fp32 bits (plnerf_mlp_bwd_multi's g_absmax)
    size_t total;
};
constexpr size_t up256(size_t v) { return (v + 255) / 256 * 256; }
constexpr Workspace workspace(size_t n_rows) {
    Workspace w{};
    const size_t np = padded(n_rows);
    w.words = 0;
    w.rows_u = up256((size_t)(SCAN_WORDS + blocks(n_rows)) * 4);
    w.src = w.rows_u + up256(np * 4);
    w.pts_u = w.src + up256(np * 4);
    w.dirs_u = w.pts_u + up256(np * 12);
    w.raw_u = w.dirs_u + up256(np * 12);
    w.g_raw_u = w.raw_u + up256(np * 16);
    w.absmax = w.g_raw_u + up256(np * 16);
    w.total = w.absmax + up256((size_t)blocks(n_rows) * 4);
    return w;
}

// Is the route served?  Decided on the host before anything is launched: the register-resident kernel of the 16-bit split
// modes (elem / ns / forced: mlp_fwd_route.h), the in-kernel encoding, at least three rows per ray (fewer: no row can be
// interior) and the backward over live rows (`bwd_compact`: with the dense backward every row of the planes is read, and
// the planes past n_eval are not written).  `enabled`: the PLNERF_FWD_UNIQUE switch.
constexpr bool served(int elem, int ns, bool training, bool embedded, int forced, int spr, size_t n_rows, bool bwd_compact,
                      bool enabled) {
    return enabled && ns == 2 && !embedded && spr >= 3 && n_rows >= 1 && n_rows % (size_t)spr == 0 && n_rows <= (size_t)INT32_MAX / 16 &&
           route::fwd_uses_rr(elem, ns, training, embedded, forced) && (!training || (bwd_compact && bwdplan::live_list_fits(n_rows)));
}

// The rule, one text for both sides (constexpr: the device kernels of mlp_unique.hip call it too).  p: [n_rows][3] words.
constexpr bool same3(const uint32_t* a, const uint32_t* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }
constexpr bool interior(const uint32_t* p, size_t row, size_t n_rows, int spr) {
    const size_t k = row % (size_t)spr;
    if (k == 0 || k == (size_t)spr - 1 || row + 1 >= n_rows) return false;
    return same3(p + 3 * (row - 1), p + 3 * row) && same3(p + 3 * row, p + 3 * (row + 1));
}
// the list as the three launches leave it: returns n_eval; rows_u [n_eval], src [n_rows]
inline size_t host_list(const uint32_t* p, size_t n_rows, int spr, uint32_t* rows_u, uint32_t* src) {
    size_t n = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        if (!interior(p, r, n_rows, spr)) rows_u[n++] = (uint32_t)r;
        src[r] = (uint32_t)(n - 1);
    }
    return n;
}

}  // namespace uniq
}  // namespace plnerf
