// Stand-alone host program (no HIP): the placement rule of the regularized lexls_lse_solve_adjoint_multi (lexls_amd/csrc/lexls_lds.h:
// adjoint_reg_multi_form) on its own.  Reads "nVar cap nObj" lines and prints "variant name|bytes with the matrices in LDS|bytes of the state
// alone" per line.  tests/test_adjoint_reg_multi_cases.py builds and runs it.
#include "lexls_lds.h"

#include <cstdio>

int main()
{
    unsigned n = 0, cap = 0, nobj = 0;
    while (std::scanf("%u %u %u", &n, &cap, &nobj) == 3)
        std::printf("%s|%zu|%zu\n", lexls::adjoint_reg_multi_form_name(lexls::adjoint_reg_multi_form(n, cap, nobj), lexls::adjoint_reg_in_lds(n, cap, nobj)),
                    lexls::adjoint_reg_multi_lds_bytes(n, cap, nobj, true), lexls::adjoint_reg_multi_lds_bytes(n, cap, nobj, false));
    return 0;
}
