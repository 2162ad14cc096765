// dn_sac_math.h -- the per-element arithmetic of the SAC loss heads (dn_sac_policy, dn_sac_policy_backward, dn_sac_critic_loss,
// dn_sac_actor_loss; include/dronenav.h states it line by line): plain C++ for host and device.  dn_sac_loss.hip runs it a row per lane;
// tests/tools/check_sac_math.cpp runs the same code on the host.  The last function is the Polyak update's (dn_polyak_update,
// dn_sac_train.hip; tests/tools/check_sac_train_layout.cpp).  Everything is IEEE float64 under -ffp-contract=off; exp, tanh and log are
// the float64 library functions (no cancellation follows them), exp(log_ent_coef) is the correctly rounded one of dn_exp_cr.h.  NaN and
// infinity are not special-cased.
//
// Two forms are deliberate, and differ from the literal float32 expression of SB3's squashed Gaussian [from recall]:
//   sech^2(pre) is J = 4 t / ((1 + t)(1 + t)) with t = exp(-2 |pre|), never 1 - a * a, which has lost everything once |pre| > 9;
//   the Gaussian's exponent is -0.5 eps^2 from eps itself, never from (pre - mean) / std, which loses eps when std is small against |mean|.
// tanh is the library's: (1 - t) / (1 + t) cancels near pre = 0.
#pragma once

#include <math.h>

#include "dn_exp_cr.h"

#define DN_SAC_FN DN_EXP_CR_FN

constexpr double DN_SAC_HALF_LOG_2PI = 0.9189385332046727;  // 0.5 log(2 pi)
constexpr double DN_SAC_LOG_EPS = 1e-6;                     // SB3's epsilon inside log(1 - tanh^2 + epsilon)

// torch.clamp: a NaN stays a NaN
DN_SAC_FN double dn_sac_clamp(const double x, const double lo, const double hi) { return x < lo ? lo : x > hi ? hi : x; }

// a = tanh(pre) and J = sech^2(pre) = 4 t / ((1 + t)(1 + t)), t = exp(-2 |pre|)
DN_SAC_FN void dn_sac_squash(const double pre, double &a, double &J)
{
    a = tanh(pre);
    const double t = exp(-2.0 * fabs(pre));
    const double u = 1.0 + t;
    J = 4.0 * t / (u * u);
}

// One element of the squashed policy head: what forward and backward both form from (mean, raw log_std, eps).
struct DnSacElem {
    double ls, std, pre, a, J, term;                   // term = -0.5 eps^2 - ls - 0.5 log(2 pi) - log(J + 1e-6)
};

DN_SAC_FN DnSacElem dn_sac_elem(const double mean, const double raw, const double eps, const double lo, const double hi)
{
    DnSacElem e;
    e.ls = dn_sac_clamp(raw, lo, hi);
    e.std = exp(e.ls);
    e.pre = mean + e.std * eps;
    dn_sac_squash(e.pre, e.a, e.J);
    e.term = -0.5 * eps * eps - e.ls - DN_SAC_HALF_LOG_2PI - log(e.J + DN_SAC_LOG_EPS);
    return e;
}

// The gradients of one element given g_a = d L / d a and g_lp = d L / d log_prob: d a / d pre = J, d term / d pre = 2 a J / (J + 1e-6),
// d pre / d ls = std eps, d term / d ls = -1 directly; torch.clamp passes the gradient at its bounds and stops it outside.
DN_SAC_FN void dn_sac_elem_backward(const DnSacElem &e, const double raw, const double eps, const double lo, const double hi, const double g_a,
                                    const double g_lp, double &d_mean, double &d_raw)
{
    const double K = 2.0 * e.a * e.J / (e.J + DN_SAC_LOG_EPS);
    const double d_pre = g_a * e.J + g_lp * K;
    const double d_ls = d_pre * e.std * eps - g_lp;
    d_mean = d_pre;
    d_raw = (raw >= lo && raw <= hi) ? d_ls : 0.0;
}

// torch.min over the critics, c ascending: the running minimum m and its index.  A NaN wins, the first one stays; a tie keeps the lowest c.
DN_SAC_FN void dn_sac_min_step(double &m, int &pick, const double q, const int c)
{
    if (q < m || (q != q && m == m)) {
        m = q;
        pick = c;
    }
}

// alpha = exp(log_ent_coef), rounded correctly where dn_exp_cr answers
DN_SAC_FN double dn_sac_alpha(const double log_ent_coef)
{
    double alpha;
    if (!dn_exp_cr(log_ent_coef, alpha)) alpha = exp(log_ent_coef);
    return alpha;
}

// The TD target of one row: y = r + (1 - done) gamma (nq - alpha next_log_prob)
DN_SAC_FN double dn_sac_target(const double reward, const double done, const double gamma, const double nq, const double alpha, const double next_lp)
{
    return reward + (1.0 - done) * gamma * (nq - alpha * next_lp);
}

// The Polyak update of one target element (dn_polyak_update): omt = 1.0 - tau is formed once on the host in float64; both float32 values
// are widened, two float64 products and one float64 add (no contraction), rounded once to float32.
DN_SAC_FN float dn_polyak(const float target, const float source, const double tau, const double omt)
{
    const double keep = omt * (double)target;
    const double take = tau * (double)source;
    return (float)(keep + take);
}
