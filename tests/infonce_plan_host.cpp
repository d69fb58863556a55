// Prints what csrc/infonce_plan.h decides, for tests/test_infonce_cpu.py: a first line with the constants, then
// `ok row_blocks col_steps part da dp nm total` for every `B N M S` read from stdin (`0` alone where the sizes are refused).
// Host only: it launches nothing and needs no device.
#include <cstdio>

#include "infonce_plan.h"

int main()
{
    using namespace umereg;
    std::printf("kInfoNceD %d kInfoNceWaves %d kInfoNceThreads %d kInfoNceRows %d kInfoNceCols %d kInfoNceLdsStride %d kInfoNceMaxS %d "
                "kInfoNceScatterRows %d kInfoNceLdsBytes %zu kInfoNceScatterLdsBytes %zu kInfoNceLdsPerCu %zu\n",
                kInfoNceD, kInfoNceWaves, kInfoNceThreads, kInfoNceRows, kInfoNceCols, kInfoNceLdsStride, kInfoNceMaxS, kInfoNceScatterRows,
                kInfoNceLdsBytes, kInfoNceScatterLdsBytes, kInfoNceLdsPerCu);
    long long B = 0, N = 0, M = 0, S = 0;
    while (std::scanf("%lld %lld %lld %lld", &B, &N, &M, &S) == 4) {
        if (!infonce_sizes_ok(B, N, M, S)) {
            std::printf("0\n");
            continue;
        }
        const InfoNceLayout L = infonce_layout((int)B, (int)S);
        std::printf("1 %d %d %zu %zu %zu %zu %zu\n", infonce_row_blocks((int)S), infonce_col_steps((int)S), L.part, L.da, L.dp, L.nm, L.total);
    }
    return 0;
}
