// Stand-alone host program (no HIP): the placement rule of lexls_lse_solve_tangent (lexls_amd/csrc/lexls_lds.h: tangent_map_placement) on its own.
// Reads "nVar cap nObj" lines and prints "placement name|bytes staged|bytes lds|bytes work|work doubles per tile|bytes of tangent_rhs" per line.
// tests/test_tangent_cases.py builds and runs it.
#include "lexls_lds.h"

#include <cstdio>

int main()
{
    using lexls::TangentPlacement;
    unsigned n = 0, cap = 0, nObj = 0;
    while (std::scanf("%u %u %u", &n, &cap, &nObj) == 3)
        std::printf("%s|%zu|%zu|%zu|%zu|%zu\n", lexls::tangent_placement_name(lexls::tangent_map_placement(n, cap, nObj)),
                    lexls::tangent_map_lds_bytes(n, cap, nObj, TangentPlacement::staged), lexls::tangent_map_lds_bytes(n, cap, nObj, TangentPlacement::lds),
                    lexls::tangent_map_lds_bytes(n, cap, nObj, TangentPlacement::work), lexls::tangent_map_work_doubles(n, cap), lexls::tangent_rhs_lds_bytes(n, cap));
    return 0;
}
