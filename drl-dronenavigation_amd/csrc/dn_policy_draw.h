// dn_policy_draw.h -- one drone's action draw from the policy's head and the standard normals z, stated once: the stand-alone sampling
// kernels (dn_glue.hip) and the step kernels that draw where the action is consumed (dn_kernels.hip sample_action_from) call the same
// functions, so the two produce the same bits.  Device code only.
#ifndef DN_POLICY_DRAW_H
#define DN_POLICY_DRAW_H

#include "dn_internal.h"

namespace {

template <typename T> DN_DEV T clipv(T x, T lo, T hi)
{   // np.clip = minimum(maximum(x, lo), hi); NaN propagates (both compares false)
    return x < lo ? lo : (x > hi ? hi : x);
}

// SB3 DiagGaussianDistribution.sample / log_prob [3P-recall] (dn_policy_sample, dn_step_sampled): a = mu + exp(log_std) z, and
// lp = log N(a; mu, sigma) summed over the four action dims, with (a - mu)/sigma = z.  The np.clip of collect_rollouts is the caller's.
DN_DEV void gaussian_draw(const float mu[4], const float ls[4], const float z[4], float a[4], float &lp)
{
    lp = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = mu[j] + expf(ls[j]) * z[j];
        lp += -0.5f * z[j] * z[j] - ls[j] - 0.91893853320467274178f;
    }
}

// tanh(x) = 1 - 2 / (1 + e^{2x}): v_exp_f32 + v_rcp_f32 (absolute error ~1e-7; +-1 exactly once e^{2x} over- or underflows)
DN_DEV float tanh_squash(const float x)
{
    const float e = __builtin_amdgcn_exp2f(x * 2.88539008177792681472f);        // 2 log2(e)
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}
// One drone's squashed-Gaussian draw (SB3 SAC Actor [3P-recall]): shared by dn_squashed_sample_kernel and the step kernels
// (dn_step_squashed), so that the two produce the same bits.  The log-probability costs four logf: only on request.
DN_DEV void squashed_draw(const float4 m, const float4 l, const float z[4], const bool want_lp, float a[4], float &lp)
{
    const float mu[4] = {m.x, m.y, m.z, m.w};
    const float ls[4] = {clipv(l.x, -20.0f, 2.0f), clipv(l.y, -20.0f, 2.0f), clipv(l.z, -20.0f, 2.0f), clipv(l.w, -20.0f, 2.0f)};
    lp = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = tanh_squash(mu[j] + expf(ls[j]) * z[j]);
    if (want_lp) {
#pragma unroll
        for (int j = 0; j < 4; ++j) lp += (-0.5f * z[j] * z[j] - ls[j] - 0.91893853320467274178f) - logf(1.0f - a[j] * a[j] + 1e-6f);
    }
}

}  // namespace

#endif
