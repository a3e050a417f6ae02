// Prints what pl-nerf_amd/csrc/mlp_unique_plan.h decides, for tests/test_fwd_unique_host.py (a host compiler builds it: the
// header is plain C++).
//   table            the predicate over element x NS x training x embedded x fwd_kernel x rows per ray x backward x switch
//   layout N...      the workspace's offsets for each row count
//   list             stdin: "n_rows spr" and 3 n_rows words (hex) -> n_eval, rows_u, src as the launches leave them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mlp_unique_plan.h"

using namespace plnerf;

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "table")) {
        for (int elem = 0; elem < 2; ++elem)
            for (int ns = 1; ns <= 2; ++ns)
                for (int training = 0; training < 2; ++training)
                    for (int emb = 0; emb < 2; ++emb)
                        for (int forced = 0; forced < 3; ++forced)
                            for (int spr : {1, 2, 3, 192})
                                for (int compact = 0; compact < 2; ++compact)
                                    for (int enabled = 0; enabled < 2; ++enabled)
                                        printf("%s %d %d %d %d %d %d %d served=%d\n", elem ? "bf16" : "f16", ns, training, emb, forced, spr,
                                               compact, enabled,
                                               (int)uniq::served(elem, ns, training != 0, emb != 0, forced, spr, (size_t)spr * 64,
                                                                 compact != 0, enabled != 0));
        // rows that are no whole rays, and more rows than the backward's list holds
        printf("ragged served=%d\n", (int)uniq::served(0, 2, true, false, 0, 7, 449, true, true));
        printf("beyond-the-live-list training=%d inference=%d\n",
               (int)uniq::served(0, 2, true, false, 0, 4, (bwdplan::LIVE_MAX_ROWS / 4 + 1) * 4, true, true),
               (int)uniq::served(0, 2, false, false, 0, 4, (bwdplan::LIVE_MAX_ROWS / 4 + 1) * 4, true, true));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "layout")) {
        for (int k = 2; k < argc; ++k) {
            const size_t n = (size_t)atoll(argv[k]);
            const uniq::Workspace w = uniq::workspace(n);
            printf("%zu: padded=%zu blocks=%d words=%zu rows_u=%zu src=%zu pts_u=%zu dirs_u=%zu raw_u=%zu g_raw_u=%zu absmax=%zu total=%zu\n", n,
                   uniq::padded(n), uniq::blocks(n), w.words, w.rows_u, w.src, w.pts_u, w.dirs_u, w.raw_u, w.g_raw_u, w.absmax, w.total);
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "list")) {
        size_t n = 0;
        int spr = 0;
        if (scanf("%zu %d", &n, &spr) != 2 || n < 1 || spr < 1) return 2;
        std::vector<uint32_t> p(3 * n), rows_u(n), src(n);
        for (size_t i = 0; i < 3 * n; ++i)
            if (scanf("%x", &p[i]) != 1) return 3;
        const size_t n_eval = uniq::host_list(p.data(), n, spr, rows_u.data(), src.data());
        printf("%zu\n", n_eval);
        for (size_t c = 0; c < n_eval; ++c) printf("%u ", rows_u[c]);
        printf("\n");
        for (size_t r = 0; r < n; ++r) printf("%u ", src[r]);
        printf("\n");
        return 0;
    }
    return 1;
}
