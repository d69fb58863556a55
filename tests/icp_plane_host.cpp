// csrc/icp_plane_math.h compiled for the host, for tests/test_icp_plane_cpu.py.  Records on stdin (hexadecimal floats), one line out each:
//   N c[6]            covariance upper triangle {xx, xy, xz, yy, yz, zz}  ->  n[3]           covariance_normal
//   S a[21] b[6]      upper triangle of sum J J^T (row by row), sum J r   ->  x[6]           plane_solve
//   U x[6]                                                               ->  R[9] t[3]      euler_update
// Host only: it launches nothing and needs no device.  Built with -ffp-contract=off: each operation rounds once.
#define UMEREG_ICP_PLANE_HOST 1
#include <cstdio>

#include "icp_plane_math.h"

template <int N>
static bool read(double (&v)[N])
{
    for (int k = 0; k < N; ++k)
        if (std::scanf("%la", &v[k]) != 1) return false;
    return true;
}

int main()
{
    char kind = 0;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'N') {
            double c[6], n[3];
            if (!read(c)) return 1;
            umereg::covariance_normal(c, n);
            std::printf("%a %a %a\n", n[0], n[1], n[2]);
        } else if (kind == 'S') {
            double a[21], b[6], x[6];
            if (!read(a) || !read(b)) return 1;
            umereg::plane_solve(a, b, x);
            std::printf("%a %a %a %a %a %a\n", x[0], x[1], x[2], x[3], x[4], x[5]);
        } else if (kind == 'U') {
            double x[6], R[3][3], t[3];
            if (!read(x)) return 1;
            umereg::euler_update(x, R, t);
            for (int p = 0; p < 3; ++p)
                for (int q = 0; q < 3; ++q) std::printf("%a ", R[p][q]);
            std::printf("%a %a %a\n", t[0], t[1], t[2]);
        } else {
            return 2;
        }
    }
    return 0;
}
