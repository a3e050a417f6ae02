// Prints what pl-nerf_amd/csrc/mlp_bwd_plan.h decides, for tests/test_mlp_bwd_plan.py.  Without an argument it answers
// the queries on its standard input, one per line:
//   const                      the rounds, the thin tile counts and the two workspace capacities
//   ranges N HALF CAP          splits, rows per split
//   deal ROUND N0 N1           the two networks' caps
//   head N HALF                head workgroups, rows per head workgroup
//   tiles N                    dgrad workgroup tiles
//   ws N HALF                  byte offsets dz gmax partials head_part gred g_eff total
//   shift BITS                 mlp_layout.h's launch scale of the half dz planes for max |g_raw| = the fp32 with these bits
//                              (decimal): the shift s, then 2^s and 2^-s as fp32 bits
// With the argument `sweep` it checks the plan's invariants over every row count up to 3,000,000 and prints, per
// property, how many cases it checked and how many broke it (with the first few of those).
#include <cstdio>
#include <cstring>

#include "mlp_bwd_plan.h"

using namespace plnerf;
using namespace plnerf::bwdplan;

static_assert(row_ranges(131072, true, 85).splits == 82 && workspace(0, true).dz == 0, "constexpr");

namespace {
struct Tally {
    const char* what;
    long checked = 0, bad = 0;
    void operator()(bool ok, long a, long b, long c) {
        ++checked;
        if (!ok && ++bad <= 5) std::printf("broken: %s at %ld %ld %ld\n", what, a, b, c);
    }
    void print() const { std::printf("%s checked=%ld bad=%ld\n", what, checked, bad); }
};

Tally t_ranges{"ranges"}, t_deal{"deal"}, t_head{"head"};

// 1 <= splits <= cap; every launched range holds a row and the ranges cover all rows; whole 64- (16-) row stages
void check_ranges(int n, bool half, int cap) {
    const Ranges r = row_ranges(n, half, cap);
    const long s = r.splits, rps = r.rows_per_split;
    t_ranges(s >= 1 && s <= cap && (s - 1) * rps < n && n <= s * rps && rps % (half ? 64 : 16) == 0, n, half, cap);
}
// The head workgroups cover all rows and fit the workspace's head section; half planes: whole 32-row tiles.  (Empty head
// workgroups are allowed: the kernel writes zeros for them.)
void check_head(int n, bool half) {
    const Head h = head_launch(n, half);
    t_head(h.n_head >= 1 && h.n_head <= lay::MAX_HEAD_WGS && (long)h.n_head * h.rows_per_head_wg >= n &&
               (!half || h.rows_per_head_wg % 32 == 0), n, half, 0);
}
// the thinner grid of row counts: every count up to 5,000, then steps of 977, and the neighbours of the powers of two
template <typename F>
void thin_grid(F f) {
    for (int n = 1; n <= 5000; ++n) f(n);
    for (int n = 5000; n <= 3000000; n += 977) f(n);
    for (int p = 8192; p <= 2097152; p *= 2)
        for (int d = -1; d <= 1; ++d) f(p + d);
}

int sweep() {
    const int N = 3000000;
    for (int n = 1; n <= N; ++n) {
        check_ranges(n, true, MAIN_ROUND);
        check_ranges(n, true, THIN_ROUND_ROWS);
        check_ranges(n, true, THIN_ROUND_TILED);
        check_ranges(n, false, F32_SPLITS);
        check_head(n, true);
        check_head(n, false);
    }
    for (int cap = 1; cap <= 127; ++cap) thin_grid([&](int n) { check_ranges(n, true, cap); });
    // two networks: each gets a range of every round, and the round is used up
    const int rounds[3] = {MAIN_ROUND, THIN_ROUND_ROWS, THIN_ROUND_TILED};
    const int steps[] = {1, 2, 3, 7, 64, 296, 1000, 2400, 8000, 65536, 131072, 262144, 720000, 786432, 1000003, 3000000};
    for (int round : rounds)
        for (int a : steps)
            thin_grid([&](int b) {
                for (int swap = 0; swap < 2; ++swap) {
                    const Deal d = swap ? deal(round, b, a) : deal(round, a, b);
                    t_deal(d.cap[0] >= 1 && d.cap[1] >= 1 && d.cap[0] + d.cap[1] == round, round, swap ? b : a, swap ? a : b);
                }
            });
    t_ranges.print();
    t_deal.print();
    t_head.print();
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sweep")) return sweep();
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        long a = 0, b = 0, c = 0;
        if (!std::strncmp(line, "const", 5)) {
            std::printf("main_round=%d f32_splits=%d thin_rows=%dx%d thin_tiled=%dx%d max_splits=%d max_head_wgs=%d\n", MAIN_ROUND,
                        F32_SPLITS, thin_tiles(false), thin_round(false), thin_tiles(true), thin_round(true), lay::MAX_SPLITS,
                        lay::MAX_HEAD_WGS);
        } else if (std::sscanf(line, "ranges %ld %ld %ld", &a, &b, &c) == 3) {
            const Ranges r = row_ranges((int)a, b != 0, (int)c);
            std::printf("%d %d\n", r.splits, r.rows_per_split);
        } else if (std::sscanf(line, "deal %ld %ld %ld", &a, &b, &c) == 3) {
            const Deal d = deal((int)a, (int)b, (int)c);
            std::printf("%d %d\n", d.cap[0], d.cap[1]);
        } else if (std::sscanf(line, "head %ld %ld", &a, &b) == 2) {
            const Head h = head_launch((int)a, b != 0);
            std::printf("%d %d\n", h.n_head, h.rows_per_head_wg);
        } else if (std::sscanf(line, "tiles %ld", &a) == 1) {
            std::printf("%d\n", dgrad_tiles((int)a));
        } else if (std::sscanf(line, "ws %ld %ld", &a, &b) == 2) {
            const Workspace w = workspace((size_t)a, b != 0);
            std::printf("%zu %zu %zu %zu %zu %zu %zu\n", w.dz, w.gmax, w.partials, w.head_part, w.gred, w.g_eff, w.total);
        } else if (std::sscanf(line, "shift %ld", &a) == 1) {
            std::printf("%d %u %u\n", lay::dzh_shift((unsigned)a), lay::dzh_scale_bits((unsigned)a), lay::dzh_unscale_bits((unsigned)a));
        } else {
            std::printf("? %s", line);
            return 1;
        }
    }
    return 0;
}
