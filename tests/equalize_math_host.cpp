// csrc/equalize_math.h compiled for the host, for tests/test_equalizer_cpu.py and tests/test_equalizer_gpu.py.  Records on stdin, one line
// out each (floats cross as hexadecimal floats, bit for bit; f32 values are read and printed through double, which holds them exactly):
//   X seed j c                                   ->  xi                     eq_xi (decimal integers)
//   A j Qt M xi0                                 ->  u                      eq_alloc (decimal integers)
//   Q r2 s                                       ->  q                      eq_area_weight
//   P p[3] n[3] r2 c xi1 xi2                     ->  t1[3] t2[3] x[3]       eq_basis, eq_place
//   W d2 rho2                                    ->  w                      eq_weight
//   D dx dy dz                                   ->  d2                     eq_d2
// Host only: it launches nothing and needs no device.  Built with -ffp-contract=off: each operation rounds once.
#define UMEREG_EQUALIZE_HOST 1
#include <cstdio>

#include "equalize_math.h"

static bool readf(float* v, int n)
{
    for (int k = 0; k < n; ++k) {
        double d;
        if (std::scanf("%la", &d) != 1) return false;
        v[k] = (float)d;
    }
    return true;
}

int main()
{
    char kind = 0;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'X') {
            unsigned long long seed, j, c;
            if (std::scanf("%llu %llu %llu", &seed, &j, &c) != 3) return 1;
            std::printf("%u\n", umereg::eq_xi((uint32_t)seed, (uint32_t)j, (uint32_t)c));
        } else if (kind == 'A') {
            unsigned long long j, Qt, M, xi0;
            if (std::scanf("%llu %llu %llu %llu", &j, &Qt, &M, &xi0) != 4) return 1;
            std::printf("%llu\n", (unsigned long long)umereg::eq_alloc(j, Qt, M, (uint32_t)xi0));
        } else if (kind == 'Q') {
            float v[2];
            if (!readf(v, 2)) return 1;
            std::printf("%u\n", umereg::eq_area_weight(v[0], v[1]));
        } else if (kind == 'P') {
            float p[3], n[3], rc[2], t1[3], t2[3], x[3];
            unsigned long long xi1, xi2;
            if (!readf(p, 3) || !readf(n, 3) || !readf(rc, 2) || std::scanf("%llu %llu", &xi1, &xi2) != 2) return 1;
            umereg::eq_basis(n, t1, t2);
            umereg::eq_place(p, n, rc[0], rc[1], (uint32_t)xi1, (uint32_t)xi2, x);
            std::printf("%a %a %a %a %a %a %a %a %a\n", (double)t1[0], (double)t1[1], (double)t1[2], (double)t2[0], (double)t2[1],
                        (double)t2[2], (double)x[0], (double)x[1], (double)x[2]);
        } else if (kind == 'W') {
            float v[2];
            if (!readf(v, 2)) return 1;
            std::printf("%a\n", umereg::eq_weight(v[0], v[1]));
        } else if (kind == 'D') {
            float v[3];
            if (!readf(v, 3)) return 1;
            std::printf("%a\n", (double)umereg::eq_d2(v[0], v[1], v[2]));
        } else {
            return 2;
        }
    }
    return 0;
}
