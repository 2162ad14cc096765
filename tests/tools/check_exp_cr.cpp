// check_exp_cr.cpp -- csrc/dn_exp_cr.h on the host, alone: prints x and dn_exp_cr(x) as hexadecimal floats for float32 arguments (what
// dn_ppo_loss passes: -log_std) and float64 ones over [-6, 6], for arguments next to 0, at the ends of the range and outside it.
// tests/test_ppo_loss_cpu.py builds it with the host compiler (-ffp-contract=off, as the library is built), plainly and under the address
// and undefined-behaviour sanitizers, and holds every line to 40-digit arithmetic.
#include <cmath>
#include <cstdio>

#include "dn_exp_cr.h"

static int emit(const double x)
{
    double y = -1.0;
    const bool ok = dn_exp_cr(x, y);
    std::printf("%a %a %d\n", x, ok ? y : -1.0, ok ? 1 : 0);
    return ok ? 1 : 0;
}

int main()
{
    int done = 0;
    for (int i = 0; i <= 6000; ++i) done += emit((double)(float)(-6.0 + 0.002 * i + 1e-4 * std::sin((double)i)));     // float32 arguments
    for (int i = 0; i <= 6000; ++i) done += emit(-6.0 + 0.002 * i + 1e-4 * std::cos((double)i));                        // float64 arguments
    for (int e = -52; e <= -1; ++e) {               // 2^-53 is not asked: exp(2^-53) lies 2^-107 above the middle of two doubles
        done += emit(std::ldexp(1.0, e));
        done += emit(-std::ldexp(1.5, e));
    }
    const double edges[] = {0.0, -0.0, 700.0, -700.0, 699.999, -699.999, 0.5 * 0.6931471805599453, -0.5 * 0.6931471805599453, 1.0, -1.0, 88.5, -745.0,
                            700.0000001, -700.0000001, 1e308, -1e308, HUGE_VAL, -HUGE_VAL, std::nan("")};
    for (const double x : edges) done += emit(x);
    std::printf("{\"answered\": %d}\n", done);
    return 0;
}
