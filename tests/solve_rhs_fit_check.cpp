// Stand-alone host program (no HIP): the placement rules of lexls_lse_solve_rhs (lexls_amd/csrc/lexls_lds.h: tangent_map_placement for plain
// factors, solve_rhs_reg_form for damped ones) on their own.  Reads "nVar cap nObj" lines and prints "plain variant|damped variant|bytes with
// state and matrices in LDS|bytes of the state alone|bytes of the work form|work doubles of the damped variant" per line.
// tests/test_solve_rhs_cases.py builds and runs it.
#include "lexls_lds.h"

#include <cstdio>

int main()
{
    using namespace lexls;
    unsigned n = 0, cap = 0, nobj = 0;
    while (std::scanf("%u %u %u", &n, &cap, &nobj) == 3)
    {
        const SolveRhsRegForm f = solve_rhs_reg_form(n, cap, nobj);
        std::printf("%s|%s|%zu|%zu|%zu|%zu\n", solve_rhs_placement_name(tangent_map_placement(n, cap, nobj)), solve_rhs_reg_form_name(f),
                    solve_rhs_reg_lds_bytes(n, cap, nobj, SolveRhsRegForm::lds), solve_rhs_reg_lds_bytes(n, cap, nobj, SolveRhsRegForm::hbm),
                    solve_rhs_reg_lds_bytes(n, cap, nobj, SolveRhsRegForm::work), solve_rhs_reg_work_doubles(n, cap, f));
    }
    return 0;
}
