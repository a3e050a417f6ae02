// Host check of pl-nerf_amd/csrc/pe_sincos.h on the encoding sweep's fast-path arguments (tests/pe_fp64.py:
// fast_path_records), against double-precision sin / cos of the same fp32 argument.  The file holds records of
// (float xs = fl(x s), int32 band); the argument is xs 2^band, exact.
//   g++ -O2 -ffp-contract=off -I pl-nerf_amd/csrc tests/pe_sweep_check.cpp -o pe_sweep_check && ./pe_sweep_check records.bin
// Exits 1 above 1.2e-7 absolute (the header's figure), 2 on a malformed file.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "pe_sincos.h"

struct Record { float xs; int32_t band; };

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s records.bin\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<Record> rec;
    Record r;
    while (std::fread(&r, sizeof r, 1, f) == 1) rec.push_back(r);
    std::fclose(f);
    if (rec.empty()) { std::fprintf(stderr, "no records\n"); return 2; }
    double worst = 0.0; Record at = rec[0]; size_t near_limit = 0;
    for (const Record& q : rec) {
        if (q.band < 0 || q.band > 15) return 2;
        const float sc = (float)(1 << q.band), theta = q.xs * sc;
        if (!(fabsf(theta) < PE_FAST_LIMIT)) { std::fprintf(stderr, "record past the fast path: %a band %d\n", q.xs, q.band); return 2; }
        if (fabsf(theta) >= 0.5f * PE_FAST_LIMIT) ++near_limit;
        float s, c;
        pe_sincos(pe_turns(q.xs), sc, &s, &c);
        const double e = fmax(fabs((double)s - sin((double)theta)), fabs((double)c - cos((double)theta)));
        if (e > worst) { worst = e; at = q; }
    }
    std::printf("PEERR host pe_sincos.h: %zu arguments (%zu in the last octave below 2^22), max abs err %.3e at xs = %a band %d\n",
                rec.size(), near_limit, worst, at.xs, at.band);
    return worst <= 1.2e-7 ? 0 : 1;
}
