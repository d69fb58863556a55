// Prints what csrc/bn_act_plan.h decides, for tests/test_bn_act_cpu.py: a first line with the constants, then
// `unit slab slabs width scratch_bytes` for every `n C` pair read from stdin (C must be one the header accepts), and
// `partials` for every line `-1 count`.  Host only: it launches nothing and needs no device.
#include <cstdio>

#include "bn_act_plan.h"

int main()
{
    std::printf("kBnThreads %d kBnMaxC %d kBnMinPasses %d kBnMaxSlabs %d kGsChunk %d kGsWidth %d\n", umereg::kBnThreads, umereg::kBnMaxC,
                umereg::kBnMinPasses, umereg::kBnMaxSlabs, umereg::kGsChunk, umereg::kGsWidth);
    long long a = 0, b = 0;
    while (std::scanf("%lld %lld", &a, &b) == 2) {
        if (a < 0) {
            std::printf("%zu\n", umereg::gs_partials((size_t)b));
            continue;
        }
        if (!umereg::bn_channels_ok((int)b)) {
            std::printf("refused\n");
            continue;
        }
        const umereg::BnPlan p = umereg::bn_plan((int)a, (int)b);
        std::printf("%d %d %d %d %zu\n", p.unit, p.slab, p.slabs, p.width, umereg::bn_scratch_bytes((int)a, (int)b));
    }
    return 0;
}
