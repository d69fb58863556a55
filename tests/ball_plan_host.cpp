// Prints what csrc/ball_search.h's lds_plan decides, for tests/test_ball_plan_cpu.py: a first line with the constants, then
// `K cap waves` for K = 1 .. kMaxBallK.  Host only: it launches nothing and needs no device.
#include <cstdio>

#include "ball_search.h"

int main()
{
    std::printf("kSelRegs %d kScanUnroll %d kMaxBallK %d kWave %d\n", umereg::kSelRegs, umereg::kScanUnroll, umereg::kMaxBallK, umereg::kWave);
    for (int K = 1; K <= umereg::kMaxBallK; ++K) {
        int cap = 0, waves = 0;
        umereg::lds_plan(K, &cap, &waves);
        std::printf("%d %d %d\n", K, cap, waves);
    }
    return 0;
}
