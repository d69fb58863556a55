// Prints what csrc/voxel_centroid_math.h decides, for tests/test_voxel_centroid_cpu.py.  Two kinds of input line (floats in any form
// strtod reads, hexadecimal included):
//   `q p voxel`                  -> `cell quantum`: floorf(p / voxel) as an integer and the point's integer share of its voxel's sum
//   `c cell sum count voxel`     -> the centroid's f32 bit pattern as an unsigned integer
// Host only: it launches nothing and needs no device.
#include <cstdio>
#include <cstring>

#include "voxel_centroid_math.h"

int main()
{
    char tag[4];
    while (std::scanf("%3s", tag) == 1) {
        if (tag[0] == 'q') {
            double p, v;
            if (std::scanf("%lf %lf", &p, &v) != 2) return 1;
            const float cell = umereg::voxel_cell((float)p, (float)v);
            std::printf("%lld %lld\n", (long long)cell, umereg::voxel_quantum((float)p, (float)v, cell));
        } else if (tag[0] == 'c') {
            long long cell, sum;
            int count;
            double v;
            if (std::scanf("%lld %lld %d %lf", &cell, &sum, &count, &v) != 4) return 1;
            const float c = umereg::voxel_centroid((float)cell, sum, count, (float)v);
            unsigned int bits;
            std::memcpy(&bits, &c, 4);
            std::printf("%u\n", bits);
        } else {
            return 1;
        }
    }
    return 0;
}
