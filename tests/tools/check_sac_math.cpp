// check_sac_math.cpp -- csrc/dn_sac_math.h on the host, alone.  tests/test_sac_loss_cpu.py builds it with the host compiler
// (-ffp-contract=off, as the library is built), plainly and under the address and undefined-behaviour sanitizers, and reads three kinds of
// lines, every number a hexadecimal float:
//   S pre a J                                   dn_sac_squash on a grid of pre over [-30, 30] and at the named points, held to 40-digit arithmetic
//   E mean raw eps g_a g_lp a term d_mean d_raw dn_sac_elem and dn_sac_elem_backward on drawn elements (a fixed generator), both clamp branches and
//                                               saturated elements among them, held to the NumPy statement of the same forms
//   M q0 q1 q2 q3 min pick                      dn_sac_min_step over four values with ties and NaN
// and a last JSON line with the counts.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "dn_sac_math.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uniform()                             // splitmix64, top 53 bits
{
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}

static void squash(const double pre)
{
    double a, J;
    dn_sac_squash(pre, a, J);
    std::printf("S %a %a %a\n", pre, a, J);
}

int main()
{
    int ns = 0, ne = 0, nm = 0;
    for (int i = 0; i <= 4000; ++i, ++ns) squash(-30.0 + 0.015 * i + 1e-3 * std::sin((double)i));
    const double named[] = {0.0, -0.0, 1e-8, -1e-8, 1e-3, -1e-3, 20.0, -20.0, 40.0};
    for (const double x : named) { squash(x); ++ns; }

    const double lo = -20.0, hi = 2.0;
    for (int i = 0; i < 4000; ++i, ++ne) {
        const int kind = i % 10;
        // float32 values, as the kernel's inputs are
        const double raw = (double)(float)(kind == 0 ? -20.5 - 4.0 * uniform() : kind == 1 ? 2.25 + 1.5 * uniform() : -5.0 + 6.5 * uniform());
        const double mean = (double)(float)(kind == 2 ? 12.0 + 4.0 * uniform() : kind == 3 ? -12.0 - 4.0 * uniform() : 4.0 * uniform() - 2.0);
        const double eps = (double)(float)(kind == 4 ? 0.0 : 6.0 * uniform() - 3.0);
        const double g_a = (double)(float)(2.0 * uniform() - 1.0), g_lp = (double)(float)(2.0 * uniform() - 1.0);
        const DnSacElem e = dn_sac_elem(mean, i == 7 ? lo : i == 8 ? hi : raw, eps, lo, hi);
        double d_mean, d_raw;
        dn_sac_elem_backward(e, i == 7 ? lo : i == 8 ? hi : raw, eps, lo, hi, g_a, g_lp, d_mean, d_raw);
        std::printf("E %a %a %a %a %a %a %a %a %a\n", mean, i == 7 ? lo : i == 8 ? hi : raw, eps, g_a, g_lp, e.a, e.term, d_mean, d_raw);
    }

    const double nan = std::nan("");
    const double sets[][4] = {{1.0, 2.0, 3.0, 4.0}, {4.0, 3.0, 2.0, 1.0}, {2.0, 1.0, 1.0, 3.0}, {1.0, 1.0, 1.0, 1.0}, {5.0, nan, 1.0, 2.0},
                              {nan, 1.0, 2.0, 3.0}, {3.0, nan, nan, 0.0}, {-0.0, 0.0, 1.0, 2.0}, {2.0, 2.0, -1.0, -1.0}};
    for (const auto &q : sets) {
        double m = q[0];
        int pick = 0;
        for (int c = 1; c < 4; ++c) dn_sac_min_step(m, pick, q[c], c);
        std::printf("M %a %a %a %a %a %d\n", q[0], q[1], q[2], q[3], m, pick);
        ++nm;
    }
    std::printf("{\"squash\": %d, \"elements\": %d, \"mins\": %d, \"alpha\": \"%a\", \"target\": \"%a\"}\n", ns, ne, nm, dn_sac_alpha(-1.2039728164672852),
                dn_sac_target(0.5, 0.0, 0.99, 2.0, 0.25, -3.0));
    return 0;
}
