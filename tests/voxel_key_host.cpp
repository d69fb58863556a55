// Prints what csrc/voxel_key.h decides, for tests/test_voxel_key_cpu.py: for every input line `x y z voxel n` (floats in any form
// strtod reads, hexadecimal included) one line `ok key cap home_slot` -- whether the point has a key, the key, the table capacity
// for a cloud of n points and the key's home slot in that table (key and slot 0 where there is no key).  Host only: it launches
// nothing and needs no device.
#include <cstdio>

#include "voxel_key.h"

int main()
{
    double x, y, z, v;
    int n;
    while (std::scanf("%lf %lf %lf %lf %d", &x, &y, &z, &v, &n) == 5) {
        const float p[3] = {(float)x, (float)y, (float)z};
        unsigned long long key = 0ull;
        const bool ok = umereg::voxel_key(p, (float)v, key);
        const unsigned int cap = umereg::vox_ws(n).cap;
        std::printf("%d %llu %u %u\n", ok ? 1 : 0, ok ? key : 0ull, cap, ok ? umereg::voxel_home_slot(key, cap) : 0u);
    }
    return 0;
}
