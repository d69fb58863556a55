// csrc/icp_gicp_math.h compiled for the host, for tests/test_icp_gicp_cpu.py.  Records on stdin (hexadecimal floats), one line out each:
//   W a[3] b[3] eps                          ->  W[6]    gicp_weight: upper triangle {xx, xy, xz, yy, yz, zz} of inv(M)
//   A n, then n times p[3] d[3] a[3] b[3] eps ->  s[27]   gicp_accumulate over the n correspondences, in order, from zero:
//                                                         the 21 upper entries of sum J0^T W J0 (row by row), then sum J0^T W d
//   T n, then n times p[3] d[3] W[6]          ->  s[27]   gicp_accumulate alone, with the weights as given
// Host only: it launches nothing and needs no device.  Built with -ffp-contract=off: each operation rounds once.
#define UMEREG_ICP_GICP_HOST 1
#include <cstdio>

#include "icp_gicp_math.h"

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
        if (kind == 'W') {
            double a[3], b[3], eps[1], W[6];
            if (!read(a) || !read(b) || !read(eps)) return 1;
            umereg::gicp_weight(a, b, eps[0], W);
            std::printf("%a %a %a %a %a %a\n", W[0], W[1], W[2], W[3], W[4], W[5]);
        } else if (kind == 'A') {
            double n[1], s[27] = {0.0};
            if (!read(n)) return 1;
            for (long i = 0; i < (long)n[0]; ++i) {
                double p[3], d[3], a[3], b[3], eps[1], W[6];
                if (!read(p) || !read(d) || !read(a) || !read(b) || !read(eps)) return 1;
                umereg::gicp_weight(a, b, eps[0], W);
                umereg::gicp_accumulate(p, d, W, s);
            }
            for (int k = 0; k < 27; ++k) std::printf(k == 26 ? "%a\n" : "%a ", s[k]);
        } else if (kind == 'T') {
            double n[1], s[27] = {0.0};
            if (!read(n)) return 1;
            for (long i = 0; i < (long)n[0]; ++i) {
                double p[3], d[3], W[6];
                if (!read(p) || !read(d) || !read(W)) return 1;
                umereg::gicp_accumulate(p, d, W, s);
            }
            for (int k = 0; k < 27; ++k) std::printf(k == 26 ? "%a\n" : "%a ", s[k]);
        } else {
            return 2;
        }
    }
    return 0;
}
