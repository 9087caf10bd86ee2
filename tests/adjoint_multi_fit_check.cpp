// Stand-alone host program (no HIP): the fit rule of lexls_lse_solve_adjoint_multi (lexls_amd/csrc/lexls_lds.h: adjoint_multi_form) on its own.
// Reads "nVar cap" lines and prints "form name|bytes staged|bytes hbm" per line.  tests/test_adjoint_multi_cases.py builds and runs it.
#include "lexls_lds.h"

#include <cstdio>

int main()
{
    unsigned n = 0, cap = 0;
    while (std::scanf("%u %u", &n, &cap) == 2)
        std::printf("%s|%zu|%zu\n", lexls::adjoint_multi_form_name(lexls::adjoint_multi_form(n, cap)), lexls::adjoint_multi_lds_bytes(n, cap, true),
                    lexls::adjoint_multi_lds_bytes(n, cap, false));
    return 0;
}
