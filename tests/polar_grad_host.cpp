// csrc/polar_grad.h compiled for the host, for tests/test_rtume_grad_cases_cpu.py: for every record `A[9] gR[9] min_gap` read from
// stdin (row major, hexadecimal floats) one line `has_frames s[3] gA[9] R[9] U[9] V[9]`: polar_frames and polar_rotation_grad as
// rtume_bwd_kernel calls them, and polar_rotation's R for the same A.  Without frames s, gA, U and V are printed as zeros.  Host only:
// it launches nothing and needs no device.  Built with -ffp-contract=off: each operation rounds once.
#define UMEREG_POLAR_HOST 1
#include <cstdio>

#include "polar_grad.h"

static bool read3x3(double (&m)[3][3])
{
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q)
            if (std::scanf("%la", &m[p][q]) != 1) return false;
    return true;
}

static void print3x3(const double (&m)[3][3])
{
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) std::printf(" %a", m[p][q]);
}

int main()
{
    double A[3][3], gR[3][3], min_gap = 0.0;
    while (read3x3(A) && read3x3(gR) && std::scanf("%la", &min_gap) == 1) {
        double U[3][3] = {}, V[3][3] = {}, s[3] = {}, gA[3][3] = {}, R[3][3];
        const bool has_frames = umereg::polar_frames(A, U, V, s);
        if (has_frames) umereg::polar_rotation_grad(U, V, s, gR, min_gap, gA);
        umereg::polar_rotation(A, R);
        std::printf("%d %a %a %a", has_frames ? 1 : 0, s[0], s[1], s[2]);
        print3x3(gA);
        print3x3(R);
        print3x3(U);
        print3x3(V);
        std::printf("\n");
    }
    return 0;
}
