// Stand-alone host program (no HIP): the rule for how far a kernel may trust a level's stored rank (lexls_amd/csrc/lse_kept_factor.h:
// trusted_rank) on its own.  Takes rows "n nf T dim rk Fc" as command-line arguments, six numbers each, and prints the rule's answer per row.
// tests/test_kept_factor_rule.py builds and runs it.
#include "lse_kept_factor.h"

#include <cstdio>
#include <cstdlib>

constexpr uint32_t kStored = 3; // (the rule takes the stored rank by address and reads it only where it counts)
static_assert(lexls::trusted_rank(7, 0, 7, 3, &kStored, 2) == 3 && lexls::trusted_rank(7, 7, 7, 3, nullptr, 2) == 0, "the rule is a constant expression");

int main(int argc, char **argv)
{
    if ((argc - 1) % 6 != 0) return 2;
    for (int i = 1; i + 5 < argc; i += 6)
    {
        uint32_t v[6];
        for (int j = 0; j < 6; j++) v[j] = (uint32_t)std::strtoul(argv[i + j], nullptr, 10);
        std::printf("%u\n", lexls::trusted_rank(v[0], v[1], v[2], v[3], &v[4], v[5]));
    }
    return 0;
}
