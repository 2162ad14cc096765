// dn_action_chain.h -- A1-A3, the float32 action chain (rescale -> thrust -> PWM -> RPM -> forces), exactly as the reference's numpy
// float32 arrays: shared by the step kernels (dn_kernels.hip) and dn_action_chain_kernel (dn_glue.hip).  Device code only; the units
// that include it are compiled with -ffp-contract=off (build.py), so every operation below rounds on its own.
#ifndef DN_ACTION_CHAIN_H
#define DN_ACTION_CHAIN_H

#include "dn_internal.h"
#include "dn_action_sat.h"

namespace {

// ---- constants: Sol/resources/safegym/cf2x.urdf:5,11-12 via BaseAviary._parse_urdf_parameters (BaseAviary.py:1123-1163)
constexpr float KF32 = (float)3.16e-10, KM32 = (float)7.94e-12;
constexpr float PWM2RPM_SCALE32 = (float)0.2685, PWM2RPM_CONST32 = (float)4070.3;
constexpr float MIN_PWM32 = 20000.0f, MAX_PWM32 = 65535.0f;
// a_low / a_high = float32(KF * (SCALE * PWM + CONST)**2), PBDroneEnv.py:113-116
constexpr float A_LOW32 = (float)(3.16e-10 * ((0.2685 * 20000.0 + 4070.3) * (0.2685 * 20000.0 + 4070.3)));
constexpr float A_HIGH32 = (float)(3.16e-10 * ((0.2685 * 65535.0 + 4070.3) * (0.2685 * 65535.0 + 4070.3)));

// ---- A1-A3: float32 action chain ------------------------------------------------------------------
// Bit-exact against numpy float32 (golden actions.npz).  IEEE divide and sqrt expand to 10 and 23 instructions on
// gfx950 (scaling, fix-up); every divisor here is a constant and every operand range is known, so the chain uses
//   a / c  =  q0 + fma(-q0, c, a) * RN(1/c),  q0 = a * RN(1/c)        (Markstein's correction, 3 instructions)
//   sqrt   =  v_sqrt_f32 (1 ulp) + a one-ulp-down / one-ulp-up test with fma residuals
// which tests/tools/check_action_chain_exact.c proves identical to the correctly rounded results for EVERY float32
// input that can reach them (2.1e9 actions, 2e7 thrusts, 1e7 roots; exhaustive).  Clips are v_med3_f32; np.clip's
// NaN propagation is restored by the final select.
constexpr float DEN32 = A_HIGH32 - A_LOW32;
constexpr float INV_DEN32 = 1.0f / DEN32, INV_KF32 = 1.0f / KF32, INV_SCALE32 = 1.0f / PWM2RPM_SCALE32;
DN_DEV float div_const32(float a, float c, float inv_c)
{
    const float q0 = a * inv_c;
    const float r = __builtin_fmaf(-q0, c, a);
    return __builtin_fmaf(r, inv_c, q0);
}
DN_DEV float sqrt_rn32(float x)
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, x), rp = __builtin_fmaf(-sp, s, x);
    float out = rm <= 0.0f ? sm : s;
    out = rp > 0.0f ? sp : out;
    return out;
}
DN_DEV float rescale_unclipped32(float a)
{   // PBDroneEnv.rescale_action, PBDroneEnv.py:949-971, before its final clip to [-1, 1]
    const float ac = __builtin_amdgcn_fmed3f(a, -2.0f, 2.0f);   // beyond +-2 the result is saturated anyway
    const float num = ac - A_LOW32;
    const float q = div_const32(num, DEN32, INV_DEN32);
    const float m = 2.0f * q;                // (high - low) = 1 - (-1)
    return -1.0f + m;
}
DN_DEV float rescale_action32(float a) { return __builtin_amdgcn_fmed3f(rescale_unclipped32(a), -1.0f, 1.0f); }
// cmd: the (rescaled) action.  rescale_action's own clip to [-1, 1] may be left out by the caller: the thrust clip below
// is to [a_low, a_high], a sub-interval, and clip(clip(x, -1, 1), lo, hi) = clip(x, lo, hi).  a: the raw action (NaN test).
DN_DEV float rotor_force_from_cmd(float cmd, float a, float &torque, float *rpm_out = nullptr, bool nan_check = true)
{
    // PBDroneEnv._preprocessAction, PBDroneEnv.py:889.  The clip makes thrust >= a_low > 0, so cmd2pwm's
    // maximum(thrust, 0) (env_utils.py:29) is the identity.
    const float thrust = __builtin_amdgcn_fmed3f(cmd, A_LOW32, A_HIGH32);
    const float t = div_const32(thrust, KF32, INV_KF32);             // env_utils.py:30 (n_motor = 1)
    const float s = sqrt_rn32(t);
    float pwm = div_const32(s - PWM2RPM_CONST32, PWM2RPM_SCALE32, INV_SCALE32);
    pwm = __builtin_amdgcn_fmed3f(pwm, MIN_PWM32, MAX_PWM32);        // env_utils.py:39
    const float r0 = PWM2RPM_SCALE32 * pwm;
    const float rpm = r0 + PWM2RPM_CONST32;          // pwm2rpm, env_utils.py:58
    const float sq = rpm * rpm;                      // BaseAviary._physics, BaseAviary.py:776-777
    const bool nan = nan_check && a != a;            // np.clip / sqrt propagate NaN
    if (rpm_out) *rpm_out = nan ? a : rpm;
    torque = nan ? a : sq * KM32;
    return nan ? a : sq * KF32;
}
DN_DEV float rotor_force_from_action(float a, bool normalize_actions, float &torque, float *rpm_out = nullptr, bool nan_check = true)
{
    return rotor_force_from_cmd(normalize_actions ? rescale_unclipped32(a) : a, a, torque, rpm_out, nan_check);
}
// The saturation fast path (round 6).  The thrust clip of rotor_force_from_cmd is the chain's ONLY read of the command, so every
// command <= a_low yields the force / torque of a_low and every command >= a_high those of a_high; rescale_action is monotone in
// the action, so in raw-action space that is two float32 thresholds (csrc/dn_action_sat.h; tests/tools/check_action_chain_exact.c
// proves thresholds and constants against the literal numpy-order chain for all 2^32 - 2^24 non-NaN actions).  99.6 % of U(-1,1)
// actions -- and of a sigma = 1 Gaussian policy's -- lie outside the 0.0072-wide band in between: per rotor the WAVE takes the chain
// only if one of its lanes is inside the band (or NaN: both compares false), 21 % of rotor evaluations at U(-1,1); then every
// lane takes it, and a saturated lane's chain returns the same two constants: bit-exact by construction either way.
constexpr float ACT_SAT_LO32 = __builtin_bit_cast(float, DN_ACT_SAT_LO_BITS), ACT_SAT_HI32 = __builtin_bit_cast(float, DN_ACT_SAT_HI_BITS);
constexpr float F_LO32 = __builtin_bit_cast(float, DN_F_LO_BITS), F_HI32 = __builtin_bit_cast(float, DN_F_HI_BITS);
constexpr float TQ_LO32 = __builtin_bit_cast(float, DN_TQ_LO_BITS), TQ_HI32 = __builtin_bit_cast(float, DN_TQ_HI_BITS);
static_assert(__builtin_bit_cast(unsigned, A_LOW32) == DN_A_LOW_BITS && __builtin_bit_cast(unsigned, A_HIGH32) == DN_A_HIGH_BITS,
              "dn_action_sat.h was derived for other action bounds");
DN_DEV float rotor_force_sat(const float a, const bool normalize_actions, float &torque)
{
    const float t_lo = normalize_actions ? ACT_SAT_LO32 : A_LOW32, t_hi = normalize_actions ? ACT_SAT_HI32 : A_HIGH32;   // wave-uniform
    const bool hi = a >= t_hi, lo = a <= t_lo;
    float f = hi ? F_HI32 : F_LO32;
    torque = hi ? TQ_HI32 : TQ_LO32;
    if (__ballot(!(hi || lo)) != 0ull)            // wave-uniform: a lane inside the band, or a NaN (np.clip / sqrt propagate it: the chain's own select)
        f = rotor_force_from_cmd(normalize_actions ? rescale_unclipped32(a) : a, a, torque, nullptr, true);
    return f;
}

DN_DEV float z_torque32(const float tq[4])
{   // z_torque = -t0 + t1 - t2 + t3, left to right in float32 (BaseAviary.py:780)
    float z = -tq[0];
    z = z + tq[1];
    z = z - tq[2];
    z = z + tq[3];
    return z;
}

}  // namespace

#endif
