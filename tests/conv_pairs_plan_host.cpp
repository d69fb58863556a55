// Prints what csrc/conv_pairs_plan.h decides, for tests/test_conv_pairs_cpu.py: a first line with the constants, then
// `cout tile_cols` for every channel count the operators accept, then `p blocks` for p = 0 .. kCpTM.  Host only: it launches
// nothing and needs no device.
#include <cstdio>

#include "conv_pairs_plan.h"

int main()
{
    std::printf("kCpTM %d kCpSlots %d kCpThreads %d\n", umereg::kCpTM, umereg::kCpSlots, umereg::kCpThreads);
    for (int cout = 32; cout <= 256; cout += 32) std::printf("c %d %d\n", cout, umereg::cp_tile_cols(cout));
    for (int p = 0; p <= umereg::kCpTM; ++p) std::printf("p %d %d\n", p, umereg::cp_blocks(p));
    return 0;
}
