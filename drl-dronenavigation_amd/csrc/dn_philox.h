// dn_philox.h -- the keyed noise streams: Philox4x32-10 and the two Box-Muller forms on its words.  Shared by the step kernels
// (dn_kernels.hip) and the sampling kernels of the rollout glue (dn_glue.hip).  Device code only.
#ifndef DN_PHILOX_H
#define DN_PHILOX_H

#include "dn_internal.h"

namespace {

// ---- noise (BASELINE config 5; sigma = 0 is the reference): Philox4x32-10 + float64 Box-Muller ------
DN_DEV void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        unsigned n1 = (unsigned)p1;
        unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        unsigned n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// The EXACT form (draws that feed the dynamics: action noise, the policies' sampling, random spawn): Box-Muller on one pair of Philox words, float64 throughout, every operation spelled out (no libm call: the device
// library's log / sin / cos carry argument-reduction paths for inputs that cannot occur here and cost ~300 instructions
// a pair; this is ~80).  u = (r + 0.5) / 2^32 lies strictly inside (0, 1).
//   ln u1:  u1 = m 2^e, m in [sqrt(1/2), sqrt(2)),  ln m = 2 atanh(s) = 2 s (1 + s^2/3 + ... + s^14/15),  s = (m-1)/(m+1),
//           |s| <= 0.1716: truncation 3e-14 relative, and no cancellation as u1 -> 1 (e = 0, m - 1 exact);
//   angle:  2 pi u2 = k pi/2 + theta, k = rint(4 u2), theta = 2 pi (u2 - k/4) in [-pi/4, pi/4] (the subtraction is
//           exact), sin / cos Taylor to theta^13 / theta^14 (2e-14), quadrant fix-up by k.
// Equal to the libm form (log, sqrt, cos, sin of the C library) to ~1e-13 before the float32 cast.
DN_DEV void box_muller_pair64(unsigned ra, unsigned rb, float &z0, float &z1)
{
    const double u1 = ((double)ra + 0.5) * (1.0 / 4294967296.0);
    const double u2 = ((double)rb + 0.5) * (1.0 / 4294967296.0);
    double m = __builtin_amdgcn_frexp_mant(u1);            // [0.5, 1)
    int e = __builtin_amdgcn_frexp_exp(u1);
    if (m < 0.70710678118654752440) { m = m + m; e = e - 1; }
    const double num = m - 1.0, den = m + 1.0;
    double r = __builtin_amdgcn_rcp(den);
    double q = __builtin_fma(-den, r, 1.0);
    r = __builtin_fma(r, q, r);
    q = __builtin_fma(-den, r, 1.0);
    r = __builtin_fma(r, q, r);
    const double sv = num * r, s2 = sv * sv;
    double pl = 1.0 / 15.0;
    pl = __builtin_fma(pl, s2, 1.0 / 13.0);
    pl = __builtin_fma(pl, s2, 1.0 / 11.0);
    pl = __builtin_fma(pl, s2, 1.0 / 9.0);
    pl = __builtin_fma(pl, s2, 1.0 / 7.0);
    pl = __builtin_fma(pl, s2, 1.0 / 5.0);
    pl = __builtin_fma(pl, s2, 1.0 / 3.0);
    pl = __builtin_fma(pl, s2, 1.0);
    const double ln_u1 = __builtin_fma((double)e, 0.69314718055994530942, (sv + sv) * pl);
    const double t = -2.0 * ln_u1;                         // > 0
    double y = __builtin_amdgcn_rsq(t);
    y = y * __builtin_fma(-0.5 * t * y, y, 1.5);
    y = y * __builtin_fma(-0.5 * t * y, y, 1.5);
    const double rad = t * y;
    const double k4 = __builtin_rint(u2 * 4.0);
    const double th = (2.0 * 3.14159265358979323846) * __builtin_fma(k4, -0.25, u2);
    const double t2 = th * th;
    double ps = 1.0 / 6227020800.0;                        //  1/13!
    ps = __builtin_fma(ps, t2, -1.0 / 39916800.0);         // -1/11!
    ps = __builtin_fma(ps, t2, 1.0 / 362880.0);
    ps = __builtin_fma(ps, t2, -1.0 / 5040.0);
    ps = __builtin_fma(ps, t2, 1.0 / 120.0);
    ps = __builtin_fma(ps, t2, -1.0 / 6.0);
    const double sn = __builtin_fma(th * t2, ps, th);
    double pc = -1.0 / 87178291200.0;                      // -1/14!
    pc = __builtin_fma(pc, t2, 1.0 / 479001600.0);         //  1/12!
    pc = __builtin_fma(pc, t2, -1.0 / 3628800.0);
    pc = __builtin_fma(pc, t2, 1.0 / 40320.0);
    pc = __builtin_fma(pc, t2, -1.0 / 720.0);
    pc = __builtin_fma(pc, t2, 1.0 / 24.0);
    pc = __builtin_fma(pc, t2, -0.5);
    const double cs = __builtin_fma(pc, t2, 1.0);
    const int k = (int)k4 & 3;
    const double c = (k & 1) ? sn : cs, d = (k & 1) ? cs : sn;          // odd quadrants swap the two ...
    const double cosv = (k == 1 || k == 2) ? -c : c;                    // ... and the signs follow cos(a + pi/2) = -sin a
    const double sinv = (k >= 2) ? -d : d;
    z0 = (float)(rad * cosv);
    z1 = (float)(rad * sinv);
}
// The FLOAT32 form (observation noise: 13 of the 17 draws of a config-5 step, 26 when an episode ends): the same Box-Muller on the
// hardware transcendentals, ~25 instructions a pair instead of ~80.  Observation noise is added to a float32 output and feeds nothing
// back inside the environment, so an error of 1e-6 in z is 1e-8 in the observation; the draws that DO feed the dynamics keep the exact
// form above, because the action chain rounds in float32 and the near-cancelling rotor torques of a hovering drone turn a last-bit
// difference in one thrust into 1e-4 in the unit angular-velocity columns (seen when the action noise was tried in this form).
// Care is taken where float32 would lose the draw:
//   ln u1:  for u1 < 1/2 the float32 value of u1 carries it to 2^-24 relative; for u1 >= 1/2 it does not (u1 -> 1 rounds to 1 and the
//           radius to 0), so the COMPLEMENT w = 1 - u1 = (~word + 0.5) / 2^32 is formed from the integer (exact to 2^-24 relative)
//           and -ln(1 - w) taken as w (1 + w/2 + w^2/3) below w = 2^-9 (next term: 2e-9 relative) and as -ln2 log2(1 - w) above;
//   angle:  v_sin_f32 / v_cos_f32 take their argument in revolutions, i.e. u2 itself: no 2 pi product to round.
// Against the float64 libm evaluation of the same formula the draws differ by at most 1.2e-6 absolute (mean 7e-8; measured over 3.3e7 draws:
// tests/test_gpu_parity.py::test_observation_noise_draws_match_their_definition); sigma z enters the state at sigma <= 1e-2.
DN_DEV void box_muller_pair32(unsigned ra, unsigned rb, float &z0, float &z1)
{
    const bool upper = ra >= 0x80000000u;
    const float u1 = __builtin_fmaf((float)ra, 2.3283064365386963e-10f, 1.1641532182693481e-10f);          // (ra + 0.5) 2^-32
    const float w = __builtin_fmaf((float)(~ra), 2.3283064365386963e-10f, 1.1641532182693481e-10f);        // 1 - u1, exact to 2^-24 relative
    const float arg = upper ? 1.0f - w : u1;
    float L = -0.69314718055994530942f * __builtin_amdgcn_logf(arg);                                          // -ln(arg); v_log_f32 = log2
    const float series = w * __builtin_fmaf(w, __builtin_fmaf(w, 0.33333333333333333f, 0.5f), 1.0f);
    L = (upper && w < 0.001953125f) ? series : L;
    const float rad = __builtin_amdgcn_sqrtf(L + L);
    const float u2 = __builtin_fmaf((float)rb, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
    z0 = rad * __builtin_amdgcn_cosf(u2);                                                                    // cos(2 pi u2)
    z1 = rad * __builtin_amdgcn_sinf(u2);
}
// Philox counter = (drone id lo, drone id hi, vector step lo, stream | vector step hi << 8): the 64-bit vector-step counter
// enters whole, so the streams do not repeat when its low word wraps (2^32 vector steps = hours of fused stepping);
// stream ids are below 256.
template <bool EXACT = true>
DN_DEV void noise4(unsigned long long seed, unsigned long long gid, unsigned long long step, unsigned stream, float z[4])
{
    unsigned r[4];
    philox4x32((unsigned)gid, (unsigned)(gid >> 32), (unsigned)step, stream | ((unsigned)(step >> 32) << 8), (unsigned)seed, (unsigned)(seed >> 32), r);
    if (EXACT) { box_muller_pair64(r[0], r[1], z[0], z[1]); box_muller_pair64(r[2], r[3], z[2], z[3]); }
    else { box_muller_pair32(r[0], r[1], z[0], z[1]); box_muller_pair32(r[2], r[3], z[2], z[3]); }
}

}  // namespace

#endif
