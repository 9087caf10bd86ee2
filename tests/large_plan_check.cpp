// Stand-alone host program: prints the constants of the large path's host-side plan (lexls_amd/csrc/lqr_large_plan.h) as `name value`
// lines, then `--`, then for every shape line on stdin
//     id batch n cap rows_max nObj level_max[0] .. level_max[nObj - 1]
// the work-space layout, the cleared range, the total, the geometry of every instantiated form of the one-launch kernel and what is
// launched around each level.  tests/test_large_plan.py and tests/test_large_cases.py read the output.  No HIP, no GPU.
#include "lqr_large_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace lexls::large;

int main()
{
#define SHOW(name) std::printf(#name " %llu\n", (unsigned long long)(name))
    SHOW(TC), SHOW(TJ), SHOW(NTP), SHOW(FNW), SHOW(FNT), SHOW(FCPW), SHOW(FTC), SHOW(FRC), SHOW(kStepCandWindow), SHOW(TRB), SHOW(TCH), SHOW(kTrsmColsMax);
    SHOW(GBM), SHOW(GBN), SHOW(GBK), SHOW(kLevelEndRows), SHOW(PTC_MIN), SHOW(kPersistMaxG), SHOW(kRecNoPos), SHOW(kRecTagMax);
    SHOW(sizeof(LargeState)), SHOW(sizeof(PersistCtl)), SHOW(sizeof(PersistCand)), SHOW(lexls::kMaxLdsBytes);
#undef SHOW
    std::printf("--\n");
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        long id;
        uint32_t batch, n, cap, rows_max, nObj;
        in >> id >> batch >> n >> cap >> rows_max >> nObj;
        std::vector<uint32_t> level_max(in ? nObj : 0);
        for (uint32_t &v : level_max) in >> v;
        if (!in)
        {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        const uint32_t maxdim  = max_level_dim(level_max.data(), nObj);
        const FastWorkspace w = fast_workspace_layout(batch, n, cap, maxdim);
        std::printf("shape %ld maxdim %u\n", id, maxdim);
        std::printf("layout W1 %zu norms0 %zu norms1 %zu D %zu E %zu st0 %zu st1 %zu pos0 %zu pos1 %zu ctl %zu mailbox %zu colbuf %zu\n", w.W1, w.norms[0], w.norms[1], w.D, w.E,
                    w.st[0], w.st[1], w.pos[0], w.pos[1], w.ctl, w.mailbox, w.colbuf);
        std::printf("clear %zu %zu Gmax %u colld %u total %zu\n", w.ctl, w.clear_end(w.Gmax), w.Gmax, w.colld, w.total);
        const LargeLds l = large_lds_bytes(n, maxdim);
        std::printf("lds piv %zu app %zu trsm %zu step %zu fields_fit %d\n", l.piv, l.app, l.trsm, step_lds_bytes(maxdim), (int)persist_fields_fit(n, maxdim));
#define FORM(NW_, CPW_)                                                                                                                                     \
    {                                                                                                                                                       \
        const uint32_t ptc = NW_ * CPW_, G = persist_grid(n, ptc);                                                                                          \
        const size_t lds   = persist_lds_bytes((int)ptc, n, maxdim);                                                                                        \
        std::printf("form %d %d G %u lds %zu stride %zu mailbox %zu colbuf %zu clear_end %zu within %d\n", NW_, CPW_, G, lds, persist_mailbox_stride(G),       \
                    persist_mailbox_bytes(G), persist_colbuf_bytes(G, maxdim), w.clear_end(G), (int)persist_within_limits(G, lds));                        \
    }
        LEXLS_PERSIST_FORMS(FORM)
#undef FORM
        for (uint32_t k = 0; k < nObj; k++)
        {
            const LevelPlan p = plan_level(level_max[k], rows_max, n, k + 1 == nObj);
            std::printf("level %u gauss %d trsm_cols %d trsm_grid %u trsm_block %u gemm_grid %u %u level_end_grid %u\n", k, (int)p.gauss, (int)p.trsm_cols, p.trsm_grid,
                        p.trsm_block, p.gemm_grid[0], p.gemm_grid[1], p.level_end_grid);
        }
    }
    return 0;
}
