// Stand-alone host program (no HIP): the lds/hbm rule of the regularized lexls_lse_solve_adjoint (lexls_amd/csrc/lexls_lds.h: adjoint_reg_in_lds)
// on its own.  Reads "nVar cap nObj" lines and prints "variant name|bytes with the matrices in LDS|bytes without|doubles of the matrices|served
// types" per line.  tests/test_adjoint_reg_cases.py builds and runs it.
#include "lexls_lds.h"

#include <cstdio>

int main()
{
    unsigned n = 0, cap = 0, nobj = 0;
    while (std::scanf("%u %u %u", &n, &cap, &nobj) == 3)
    {
        std::printf("%s|%zu|%zu|%zu|", lexls::adjoint_reg_form_name(lexls::adjoint_reg_in_lds(n, cap, nobj)), lexls::adjoint_reg_lds_bytes(n, cap, nobj, true),
                    lexls::adjoint_reg_lds_bytes(n, cap, nobj, false), lexls::adjoint_reg_matrix_doubles(n, nobj));
        for (unsigned t = 0; t < 12; t++)
            if (lexls::adjoint_reg_serves(t)) std::printf("%u ", t);
        std::printf("\n");
    }
    return 0;
}
