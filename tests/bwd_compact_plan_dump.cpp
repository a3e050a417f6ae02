// Stand-alone host program over the live-row helpers of pl-nerf_amd/csrc/mlp_bwd_plan.h (tests/test_bwd_compact_plan.py
// builds and runs it; the header is plain C++).  `sweep` checks the invariants and prints one line per family; the
// other queries print the helpers' answers for the test's literal tables.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "mlp_bwd_plan.h"

using namespace plnerf;
using namespace plnerf::bwdplan;

// the row counts of tests/test_mlp_bwd_plan.py's ROWS, then the benchmark's two networks and the largest count the list holds
static const long long ROWS[] = {0, 1, 191, 192, 193, 961, 1152, 1153, 1000, 262144, 786432, (long long)LIVE_MAX_ROWS};

static std::vector<long long> live_counts(long long n_rows) {
    std::set<long long> s;
    if (n_rows <= 4096) {
        for (long long k = 0; k <= n_rows; ++k) s.insert(k);
    } else {      // 0, everything around the multiples of the stage (64), the dgrad tile (192) and the count block up to 4096,
                  // a grid of such edges over the rest, n_rows
        for (long long k = 0; k <= 4096; ++k) s.insert(k);
        for (long long e : {64LL, 192LL, 1024LL})
            for (long long m = e; m <= n_rows; m += e * (1 + n_rows / (e * 997)))
                for (long long d = -1; d <= 1; ++d)
                    if (m + d >= 0 && m + d <= n_rows) s.insert(m + d);
        for (long long d = 0; d <= 193; ++d) s.insert(n_rows - d);
    }
    return std::vector<long long>(s.begin(), s.end());
}

static int sweep() {
    long long checked = 0, bad = 0;
    // ---- the device-side row ranges over [0, n_live)
    for (long long n_rows : ROWS) {
        if (n_rows < 1 || n_rows > 2147483647LL) continue;
        for (int round : {MAIN_ROUND, THIN_ROUND_ROWS, THIN_ROUND_TILED}) {
            for (int cap = 1; cap <= round; cap += (n_rows > 4096 && cap > 2 && cap + 7 < round) ? 7 : 1) {
                const Ranges host = row_ranges((int)n_rows, true, cap);      // what the host launches: the grid's ranges for this network
                for (long long n_live : live_counts(n_rows)) {
                    const Ranges r = live_ranges((int)n_live, host.splits);
                    ++checked;
                    bool ok = r.rows_per_split > 0 && r.rows_per_split % 64 == 0;      // whole 64-row stages
                    ok = ok && r.splits >= 0 && r.splits <= cap && r.splits <= round;   // never more ranges than the round holds
                    ok = ok && r.splits <= host.splits;                                 // ... nor than the grid the host sized from n_rows
                    // cover [0, n_live) exactly once: range i = [i rps, min(n_live, (i + 1) rps)), every one non-empty,
                    // the last one reaching n_live; a workgroup past them starts at or past n_live
                    ok = ok && (long long)r.splits * r.rows_per_split >= n_live;
                    ok = ok && (r.splits == 0 ? n_live == 0 : (long long)(r.splits - 1) * r.rows_per_split < n_live);
                    if (!ok) {
                        if (++bad <= 10) std::printf("BAD ranges n_rows=%lld cap=%d n_live=%lld -> %d x %d\n", n_rows, cap, n_live, r.splits, r.rows_per_split);
                    }
                }
            }
        }
    }
    std::printf("ranges checked=%lld bad=%lld\n", checked, bad);
    // ---- the head launch over the live rows: its workgroups cover them, and are no more than the host launched
    checked = bad = 0;
    for (long long n_rows : ROWS) {
        if (n_rows < 1 || n_rows > 2147483647LL) continue;
        const Head host = head_launch((int)n_rows, true);
        for (long long n_live : live_counts(n_rows)) {
            const Head h = live_head((int)n_live);
            ++checked;
            const bool ok = h.n_head >= 1 && h.n_head <= host.n_head && h.rows_per_head_wg % 32 == 0 &&
                            (long long)h.n_head * h.rows_per_head_wg >= n_live;
            if (!ok && ++bad <= 10) std::printf("BAD head n_rows=%lld n_live=%lld -> %d x %d\n", n_rows, n_live, h.n_head, h.rows_per_head_wg);
        }
    }
    std::printf("head checked=%lld bad=%lld\n", checked, bad);
    // ---- where the list lives: inside the workspace's partials section, in slots no main launch writes, below what a
    // thin launch writes; entries and scan words distinct
    checked = bad = 0;
    for (long long n_rows : ROWS) {
        if (!live_list_fits((size_t)n_rows)) continue;      // (a build without room -- PLNERF_WG_SPLITS = MAX_SPLITS -- runs dense: nothing to place)
        ++checked;
        bool ok = true;
        {
            const Workspace w = workspace((size_t)n_rows, true);
            const size_t section_words = (w.head_part - w.partials) / 4;
            auto check_word = [&](size_t word, bool scan) {
                const size_t slot = word / lay::PART_PER_SPLIT, in_slot = word % lay::PART_PER_SPLIT;
                bool good = word < section_words;                                   // inside the section (so inside the workspace)
                good = good && slot >= (size_t)MAIN_ROUND && slot < (size_t)lay::MAX_SPLITS;      // no main launch writes this slot
                good = good && in_slot < (size_t)lay::PART_PE0;                     // a thin launch writes PART_PE0 and up
                good = good && (scan ? in_slot >= (size_t)lay::PART_VMAIN : in_slot < (size_t)lay::PART_VMAIN);   // entries and scan words apart
                return good;
            };
            // every entry at the chunk edges, a stride through the rest (the index is affine inside a chunk), the last one
            std::set<size_t> idx;
            for (size_t c = 0; c * LIVE_CHUNK < (size_t)n_rows; ++c) {
                for (size_t i : {(size_t)0, (size_t)1, LIVE_CHUNK - 2, LIVE_CHUNK - 1}) idx.insert(c * LIVE_CHUNK + i);
                for (size_t i = 0; i < LIVE_CHUNK; i += 4093) idx.insert(c * LIVE_CHUNK + i);
            }
            if (n_rows > 0) idx.insert((size_t)n_rows - 1);
            size_t prev = 0;
            bool have_prev = false;
            for (size_t i : idx) {
                if (i >= (size_t)n_rows) break;
                const size_t word = live_entry_word(i);
                ok = ok && check_word(word, false) && (!have_prev || word > prev);      // strictly increasing: no two entries share a word
                prev = word; have_prev = true;
            }
            ok = ok && check_word(live_scan_word(LIVE_N), true);
            const int nb = live_blocks((size_t)n_rows);
            ok = ok && nb <= LIVE_MAX_BLOCKS;
            for (int b = 0; b < nb; ++b) ok = ok && check_word(live_scan_word(LIVE_COUNTS + b), true) && live_scan_word(LIVE_COUNTS + b) > live_scan_word(LIVE_N);
        }
        if (!ok && ++bad <= 10) std::printf("BAD layout n_rows=%lld\n", n_rows);
    }
    std::printf("layout checked=%lld bad=%lld\n", checked, bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "sweep")) return sweep();
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        long long a = 0, b = 0;
        if (std::sscanf(line, "live_ranges %lld %lld", &a, &b) == 2) {
            const Ranges r = live_ranges((int)a, (int)b);
            std::printf("%d %d\n", r.splits, r.rows_per_split);
        } else if (std::sscanf(line, "live_head %lld", &a) == 1) {
            const Head h = live_head((int)a);
            std::printf("%d %d\n", h.n_head, h.rows_per_head_wg);
        } else if (std::sscanf(line, "entry %lld", &a) == 1) {
            std::printf("%zu\n", live_entry_word((size_t)a));
        } else if (std::sscanf(line, "scan %lld", &a) == 1) {
            std::printf("%zu\n", live_scan_word((int)a));
        } else if (std::sscanf(line, "fits %lld", &a) == 1) {
            std::printf("%d\n", live_list_fits((size_t)a) ? 1 : 0);
        } else if (!std::strncmp(line, "const", 5)) {
            std::printf("slot0=%d slots=%d chunk=%zu block_rows=%d max_blocks=%d\n", LIVE_SLOT0, LIVE_SLOTS, (size_t)LIVE_CHUNK, LIVE_BLOCK_ROWS,
                        LIVE_MAX_BLOCKS);
        } else {
            std::printf("?\n");
        }
    }
    return 0;
}
