// The subset product of the Sobol subset pass (lcgp_amd/csrc/sobol_subset.h), the very text the kernel compiles, built for the host
// by tests/test_sobol_subset_host.py:   g++ -std=c++17 -O2 -ffp-contract=off -I lcgp_amd/csrc tests/native/sobol_subset_host.cpp
//   usage: sobol_subset_host <DD: 8 or 16> <in> <out>
// in:  records of { uint64 mask; double J[DD]; double A[DD]; }.   out: per record { double m0, product, difference; }.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sobol_subset.h"

template <int DD>
int run(FILE* in, FILE* out) {
    struct Rec { uint64_t mask; double J[DD]; double A[DD]; };
    Rec r;
    while (fread(&r, sizeof(Rec), 1, in) == 1) {
        const double m0 = sobol_subset_product<DD>(0u, r.J, r.A);
        const double res[3] = {m0, sobol_subset_product<DD>((unsigned)r.mask, r.J, r.A),
                               sobol_subset_diff<DD>((unsigned)r.mask, r.J, r.A, m0)};
        if (fwrite(res, sizeof(double), 3, out) != 3) return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 1;
    const int dd = atoi(argv[1]);
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 1;
    static_assert(sobol_subset_chunk(8) >= 1 && sobol_subset_chunk(16) >= 1 && SOBOL_SUBSET_DMAX == 16, "chunk rule");
    int rc = dd == 8 ? run<8>(in, out) : dd == 16 ? run<16>(in, out) : 1;
    fclose(in);
    fclose(out);
    return rc;
}
