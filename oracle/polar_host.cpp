// oracle/polar_host.cpp -- TEST INFRASTRUCTURE ONLY: the library's own 3x3 polar rotation (umeregrobust_amd/csrc/polar.h, the text
// rtume_kernel and icp_step_kernel compile) built for the host, so the routine can be judged without a GPU.
// -ffp-contract=off: each operation rounds once; the judgement must not depend on which products the host compiler fuses.
#define UMEREG_POLAR_HOST 1
#include "../umeregrobust_amd/csrc/polar.h"

// A, R: fp64 [n,3,3] row major.
extern "C" __attribute__((visibility("default"))) int orc_polar_rotation_f64(const double* A, int n, double* R)
{
    if (!A || !R || n < 0) return 1;
    for (int i = 0; i < n; ++i) {
        double a[3][3], r[3][3];
        for (int p = 0; p < 3; ++p)
            for (int q = 0; q < 3; ++q) a[p][q] = A[(long)i * 9 + p * 3 + q];
        umereg::polar_rotation(a, r);
        for (int p = 0; p < 3; ++p)
            for (int q = 0; q < 3; ++q) R[(long)i * 9 + p * 3 + q] = r[p][q];
    }
    return 0;
}
