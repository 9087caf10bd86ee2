// Stand-alone host program (no HIP): the placement rule of lexls_lsi_batch_solve_bounds (lexls_amd/csrc/lexls_lds.h: bounds_check_placement) on its own.
// Reads "nVar" lines and prints "variant name|bytes lds|bytes hbm|budget" per line.  tests/test_lsi_solve_bounds_api.py builds and runs it.
#include "lexls_lds.h"

#include <cstdio>

int main()
{
    using lexls::BoundsCheckPlacement;
    unsigned n = 0;
    while (std::scanf("%u", &n) == 1)
        std::printf("%s|%zu|%zu|%zu\n", lexls::bounds_check_placement_name(lexls::bounds_check_placement(n)), lexls::bounds_check_lds_bytes(n, BoundsCheckPlacement::lds),
                    lexls::bounds_check_lds_bytes(n, BoundsCheckPlacement::hbm), lexls::kBoundsCheckLdsBudget);
    return 0;
}
