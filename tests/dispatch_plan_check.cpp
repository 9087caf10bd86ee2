// Stand-alone host program: reads one grid entry per line (scripts/record_dispatch_table.py, query_line), feeds it
// through the planners of lexls_amd/csrc/lexls_dispatch.h and prints what they decide.  tests/test_dispatch_plan.py compares the output
// with tests/dispatch_table.json.  No HIP, no GPU: the planner is plain host arithmetic.
#include "lexls_dispatch.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace lexls;

int main()
{
    std::string line;
    while (std::getline(std::cin, line))
    {
        std::istringstream in(line);
        std::string kind;
        long id;
        unsigned align, keep, do_solve, policy, guard, qtol0, fixed, sweep;
        DispatchQuery q;
        in >> kind >> id >> q.batch >> q.nVar >> q.nObj >> q.cap >> q.uniform_dim >> q.max_rows >> q.max_level_dim >> fixed >> q.reg_type >> align >> keep >> do_solve >> policy >>
            guard >> qtol0 >> q.wave_capacity >> sweep;
        if (!in)
        {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        q.has_fixed           = fixed != 0;
        q.align               = align;
        q.write_factor        = keep != 0;
        q.do_solve            = do_solve != 0;
        q.opportunistic_solve = !q.do_solve;
        q.policy              = static_cast<KernelPolicy>(policy);
        q.guard               = guard != 0;
        q.qtol_off            = qtol0 != 0;
        q.sweep_serves        = sweep != 0;
        if (kind == "lse")
        {
            const KernelPlan p = plan_lqr(q);
            std::printf("%ld|%s|E%d R%d X%d S%d H%d C%d|%s\n", id, p.name, p.estimating, p.register_resident, p.solves_x, p.needs_solve_launch,
                        p.factor_in_hbm, p.reciprocal_solve, q.guard && guard == 2 && p.estimating ? kernel_name(plan_guard_resolve(q)) : "");
        }
        else // a resident LexLSI round: by reference or not, the persistent launch, the stage path's kernel
        {
            const bool by_ref   = plan_round_gathers_by_reference(q);
            const KernelId fuse = plan_lsi_fused(q);
            q.gather_by_reference = by_ref;
            std::printf("%ld|%s|G%d|%s\n", id, kernel_name(fuse), by_ref, plan_lqr(q).name);
        }
    }
    return 0;
}
