// dn_exp_cr.h -- exp(x) in float64, correctly rounded: plain C++ for host and device (dn_ppo_loss.hip forms exp(-log_std) with it, once per
// column and workgroup; tests/tools/check_exp_cr.cpp runs the same code on the host).
//
// Why the loss head needs it.  In the first PPO epoch new and old log-probabilities differ by the float32 rounding of the stored one, about
// 1e-7, and a row's approx_kl term (ratio - 1) - lr is about lr^2 / 2 ~ 1e-14 beside a ratio rounded to 2^-53: the term depends on the very
// bits of lr.  The float64 library exp is within an ulp of exp(-log_std) but not always the nearest double (one column in some dozens,
// measured); that ulp moves the last bit of logp in a quarter of the rows and the rounding of their ratios with it.  exp(-log_std) is A
// values per workgroup, so the cost of forming it in double-double arithmetic is nothing, and its bits stop depending on the library.
//
// Method: x = k ln 2 + r with ln 2 in three parts (the first two with trailing zero bits, so k times them is exact), m = r / 512,
// p = exp(m) - 1 by its series to m^6 (|m| < 7e-4: the rest is below 2e-26), the first two terms in double-double; nine times
// p <- 2 p + p^2 in double-double (exp(2 m) - 1); the result is 2^k (1 + p), rounded once.  The relative error before that rounding is below
// 2^-90, so the result is the nearest double unless exp(x) lies within 2^-90 of the middle between two doubles.  Outside |x| <= 700, and for
// NaN, the caller's library exp is the answer (overflow, underflow and NaN are its business): dn_exp_cr returns false.
#pragma once

#ifdef __HIP__
#define DN_EXP_CR_FN __host__ __device__ inline
#else
#define DN_EXP_CR_FN inline
#endif

// hi + lo = a + b exactly (Knuth)
DN_EXP_CR_FN void dn_two_sum(const double a, const double b, double &hi, double &lo)
{
    hi = a + b;
    const double bb = hi - a;
    lo = (a - (hi - bb)) + (b - bb);
}

// hi + lo = a b exactly
DN_EXP_CR_FN void dn_two_prod(const double a, const double b, double &hi, double &lo)
{
    hi = a * b;
    lo = __builtin_fma(a, b, -hi);
}

// (ah + al) + (bh + bl), renormalised
DN_EXP_CR_FN void dn_dd_add(const double ah, const double al, const double bh, const double bl, double &hi, double &lo)
{
    double s, e;
    dn_two_sum(ah, bh, s, e);
    e += al + bl;
    dn_two_sum(s, e, hi, lo);
}

// (ah + al)^2, renormalised
DN_EXP_CR_FN void dn_dd_sqr(const double ah, const double al, double &hi, double &lo)
{
    double p, e;
    dn_two_prod(ah, ah, p, e);
    e += 2.0 * ah * al;
    dn_two_sum(p, e, hi, lo);
}

DN_EXP_CR_FN bool dn_exp_cr(const double x, double &out)
{
    if (!(x >= -700.0 && x <= 700.0)) return false;
    // ln 2 = L1 + L2 + L3: L1 and L2 carry 32 and 30 significant bits, so k L1 and k L2 are exact for |k| <= 1024
    const double L1 = 0x1.62e42feep-1, L2 = 0x1.a39ef358p-33, L3 = -0x1.b0e2633fe0685p-67, INV_LN2 = 0x1.71547652b82fep0;
    const double k = __builtin_rint(x * INV_LN2);
    double rh, rl;
    dn_two_sum(x - k * L1, -k * L2, rh, rl);           // x - k L1 is exact: both are multiples of 2^-32 ulp-wise and the difference is small
    double th, tl;
    dn_two_prod(-k, L3, th, tl);
    dn_dd_add(rh, rl, th, tl, rh, rl);
    const double mh = rh * 0x1p-9, ml = rl * 0x1p-9;   // exact scalings
    // p = m + m^2 / 2 in double-double, + m^3 / 6 + m^4 / 24 + m^5 / 120 + m^6 / 720 in double (below 6e-11: a double's 2^-53 of it is enough)
    double qh, ql, ph, pl;
    dn_dd_sqr(mh, ml, qh, ql);
    dn_dd_add(mh, ml, 0.5 * qh, 0.5 * ql, ph, pl);
    const double m = mh, tail = m * m * m * (1.0 / 6.0 + m * (1.0 / 24.0 + m * (1.0 / 120.0 + m * (1.0 / 720.0))));
    dn_dd_add(ph, pl, tail, 0.0, ph, pl);
    for (int i = 0; i < 9; ++i) {                      // exp(2 m) - 1 = 2 p + p^2
        dn_dd_sqr(ph, pl, qh, ql);
        dn_dd_add(2.0 * ph, 2.0 * pl, qh, ql, ph, pl);
    }
    double sh, sl;
    dn_two_sum(1.0, ph, sh, sl);
    out = __builtin_ldexp(sh + (sl + pl), (int)k);     // |x| <= 700: no subnormal result, the scaling is exact
    return true;
}
