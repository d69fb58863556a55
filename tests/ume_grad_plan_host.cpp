// Prints what csrc/ume_grad_plan.h's bwd_plan decides, for tests/test_ume_grad_plan_cpu.py: a first line with the constants, then
// `n_rt n_jt tiles_per_split splits n_work` for every `rows cols` pair read from stdin.  Host only: it launches nothing and needs no
// device.
#include <cstdio>

#include "ume_grad_plan.h"

int main()
{
    std::printf("kRowTiles %d kRowKp %d\n", umereg::kRowTiles, umereg::kRowKp);
    int rows = 0, cols = 0;
    while (std::scanf("%d %d", &rows, &cols) == 2) {
        const umereg::BwdPlan p = umereg::bwd_plan(rows, cols);
        std::printf("%d %d %d %d %d\n", p.n_rt, p.n_jt, p.tiles_per_split, p.splits, p.n_work);
    }
    return 0;
}
