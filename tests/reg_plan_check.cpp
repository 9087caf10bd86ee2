// Stand-alone host program: one regularized factorization per line (tests/reg_cases.py, plan_line) through the planner of
// lexls_amd/csrc/lexls_dispatch.h and, where a regularized wave kernel serves it, through the placement rule of lexls_lds.h exactly as that
// kernel's launcher calls it (launch_wave_t2, lqr_small_impl.h).  Prints the kernel's name, the order of the LDS window of the routines' work
// matrix and whether the null-space basis is kept in LDS (reg_cfg), and the dynamic LDS of the launch.  tests/test_reg_cases.py holds the table
// of tests/reg_cases.py equal to this output.  No HIP, no GPU: plain host arithmetic.
#include "lexls_dispatch.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace lexls;

template <int NC, int MD>
static size_t reg_launch_lds(const DispatchQuery &q, uint32_t &reg_cfg)
{
    return wave_reg_lds_bytes<MD>(q.nVar, q.reg_type, q.reg_lds_share, wave_lds_bytes<NC, MD>(q.nObj, wave_img_doubles<MD>(q.nVar, q.nObj)), reg_cfg);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::string id;
        unsigned fixed, policy, share;
        DispatchQuery q;
        in >> id >> q.batch >> q.nVar >> q.nObj >> q.cap >> q.uniform_dim >> q.max_rows >> q.max_level_dim >> fixed >> q.reg_type >> policy >> share;
        if (!in)
        {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        q.has_fixed     = fixed != 0;
        q.policy        = static_cast<KernelPolicy>(policy);
        q.reg_lds_share = share; // bytes of LDS one wavefront's optional pieces may fill (wave_reg_lds_share(): 20 KB by default)
        const KernelPlan p = plan_lqr(q);
        uint32_t reg_cfg = 0;
        size_t lds       = 0;
        if (p.id == KernelId::wave_41x12_fR) lds = reg_launch_lds<41, 12>(q, reg_cfg);
        if (p.id == KernelId::wave_64x16_fR) lds = reg_launch_lds<64, 16>(q, reg_cfg);
        std::printf("%s|%s|%u|%u|%zu\n", id.c_str(), p.name, reg_cfg & 0xffu, (reg_cfg >> 8) & 1u, lds);
    }
    return 0;
}
