// dn_shapes.h -- which step kernel a fleet gets: the pick dn_create makes, as a pure host function.
//
// Includes include/dronenav.h and the standard library only: a plain host compiler builds it without the HIP headers, and
// tests/tools/check_kernel_shapes.cpp walks it over its whole domain on the CPU (tests/test_kernel_shapes_cpu.py).
//
// Read it from the bottom: dn_pick_shapes = the measured pick (dn_pick_fused, dn_pick_single: one rule per shape, tried in a fixed order),
// then the DN_WAVES / DN_WAVES_SINGLE overrides, then the two cases that force the one-wave kernels.
#ifndef DN_SHAPES_H
#define DN_SHAPES_H

#include "../../include/dronenav.h"

// Shape crossovers, measured on the 256-CU MI355X and kept as TILES PER CU (a 64-drone tile is one workgroup): what decides a
// shape is how many waves meet on a SIMD, so a partitioned (CPX) or smaller device scales the fleet sizes with its own
// hipDeviceProp_t.multiProcessorCount (dn_create) instead of inheriting the 256-CU figures.
constexpr long long DN_CALIBRATION_CUS = 256;
constexpr long long DN_TWO_WAVE_TILES_PER_CU = 4;   // 1024 tiles = 65536 drones on 256 CUs: one tile per SIMD
constexpr long long DN_PQX_TILES_PER_CU = 4;        // three-wave single step: while the tiles alone leave SIMDs idle
constexpr long long DN_FIVE_WAVE_TILES_PER_CU = 2;  // the same with the normaliser on a fifth wave: up to two tiles per CU (round 6: beyond, the four-wave kernel's X wave carries the normaliser -- 149 registers since its statistics are addressed from a walked pair -- and wins: dn_rule_four_waves)
constexpr long long DN_ROLE_PIPE_TILES_PER_CU = 6;  // role-pipelined fused step (eight roles per tile): up to one tile per CU and from three to six, see dn_eight_roles_take
constexpr long long DN_FOUR_WAVE_TILES_PER_CU = 3;  // four-wave fused step: up to three tiles per CU (768 tiles on 256 CUs)

struct DnShapes { int fused, single; };     // kernel shape of dn_step_many (k > 1) and of dn_step (k == 1), see dn_launch_step_many

// The configuration the multi-wave kernels past three waves, the sampling steps and the policy-fused step are built for: no reward
// wrappers, Physics.PYB, ActionType.THRUST, fixed spawn, damping as it is.
inline bool dn_config_is_plain(const dn_config &c)
{
    return !c.clip_rew && !c.norm_rew && c.physics == 0 && c.action_type == 0 && !c.random_spawn && !c.zero_damping;
}

inline bool dn_config_is_noisy(const dn_config &c) { return c.act_noise_sigma > 0.0f || c.obs_noise_sigma > 0.0f; }

// The kernels cut by dependency (dn_step_pqx_kernel, dn_step_many_4w_kernel and its five-wave form) are built for the plain configuration
// without the ground-contact term.
inline bool dn_config_cut_by_dependency(const dn_config &c) { return dn_config_is_plain(c) && !c.ground_contact; }

// The role-pipelined kernel (dn_step_many_rp8_kernel): plain configuration with the normaliser, no noise.
inline bool dn_config_role_pipelined(const dn_config &c) { return dn_config_cut_by_dependency(c) && !dn_config_is_noisy(c) && c.normalize_obs; }

// One rule per shape: the configurations its kernel is built for, and the largest fleet, in tiles, at which it was measured to win.
struct DnShapeRule {
    bool usable;
    long long max_tiles;
    bool takes(long long blocks) const { return usable && blocks <= max_tiles; }
};

// Measured on MI355X (profiles/r01_r_sweep_shapes.txt): the fused K-step kernel is bound by the dependent
// instruction stream of a wave, and two or three waves per tile win while the tiles alone leave SIMDs idle
// (<= 1024 tiles = 65536 drones on 1024 SIMDs); the single-step launch is latency bound (launch + load round
// trip) and one wave is never slower.  DN_WAVES=1|2|3 forces a shape (A/B measurements, the bit-identity test).
inline DnShapeRule dn_rule_two_waves(const dn_config &c, int num_cus)
{
    const long long tiles = DN_TWO_WAVE_TILES_PER_CU * num_cus;
    return {true, c.normalize_obs ? tiles / 2 : tiles};
}

// The three-wave shape (flight / report / aux) exists for fused launches.  Measured (profiles/r01_r_sweep_shapes.txt,
// profiles/r01_r_sweep_options.txt, with the report wave yielding to the other two by s_setprio): without the
// normaliser it wins wherever more than one wave per tile wins, i.e. up to 1024 tiles (65536 drones: 2.3 us per step
// against 2.5 with two waves and 2.9 with one); with the normaliser (27 more float64 per drone in a wave) up to 512
// tiles (32768 drones: 1.8 us against 2.1 with two waves), one wave beyond (49152 drones: 3.3 us against 3.5).
// The option kernels are wider in registers (the three-wave kernels are compiled for three waves per SIMD, two with
// the normaliser: __launch_bounds__), so their crossovers sit lower (profiles/r01_r_sweep_options.txt, us per step).
// No bound here lies above the two-wave one.
inline DnShapeRule dn_rule_three_waves(const dn_config &c, int num_cus)
{
    const long long tiles = DN_TWO_WAVE_TILES_PER_CU * num_cus;
    //   XOPT options (reward wrappers, force terms, rpm actions), all on: 32768 drones 2.15 (3w) / 2.97 (2w) / 3.70 (1w);
    //     49152: 2.43 / 2.99 / 3.66; 65536: 4.48 / 3.14 / 3.72  -> three waves up to 768 tiles, two up to 1024;
    //     with the normaliser 32768: 2.43 / 2.80 / 4.50; 65536: 4.74 / 5.42 / 4.56 -> three up to 512 tiles, one beyond;
    if (!dn_config_is_plain(c) && !c.normalize_obs) return {true, tiles * 3 / 4};
    //   noise (Philox + Box-Muller per observation column): 16384 drones 3.51 / 4.63 / 5.86; 32768: 4.86 / 4.78 / 6.02;
    //     49152: 5.36 / 4.88 / 6.04 -> three waves up to 256 tiles, two beyond (same with the normaliser, up to 512);
    //     noise + XOPT without the normaliser follows the XOPT row (49152: 5.75 / 6.23 / 6.99).
    if (dn_config_is_noisy(c)) return {true, tiles / 4};
    return dn_rule_two_waves(c, num_cus);
}

// Four waves (dn_step_many_4w_kernel: the recurrence itself on two waves; plain configuration without the ground-contact term,
// us per step against the three- / two- / one-wave pick of the table above):
//   normaliser off   8 192 / 16 384 / 24 576 / 32 768 / 49 152 drones   1.01 / 1.02 / 1.23 / 1.23 / 1.66   against 1.28 / 1.29 / 1.29 / 1.28 / 1.71
//                    65 536: 2.58 against 1.92 -> up to 768 tiles
//   normaliser on    8 192 / 16 384 / 24 576 / 32 768 / 49 152           1.37 / 1.39 / 1.73 / 1.76 / 3.27   against 1.48 / 1.50 / 1.87 / 1.89 / 3.36 -> up to 768 tiles
//   with noise       16 384 / 32 768 / 49 152                            2.99 / 4.47 / 4.84   against 3.75 / 4.85 / 4.84 (normaliser on: 3.43 / 3.75 / 7.44 against
//                    3.62 / 5.73 / 6.98) -> up to 512 tiles
// ... and from two to three tiles per CU the four-wave kernel WITH the normaliser on its X wave, once its statistics are addressed from a walked
// scalar pair (195 -> 149 registers: three tiles = twelve waves per CU resident; four waves | five | eight roles, profiles/r06_sweep_4wnorm.txt):
// 34 816 drones 1.80 | 2.06 | 1.93, 40 960 1.83 | 2.13 | 1.96, 49 152 1.95 | 2.23 | 2.06, 53 248 2.66 | 3.14 | 2.44 -> four waves in (2, 3] tiles per CU.
inline DnShapeRule dn_rule_four_waves(const dn_config &c, int num_cus)
{
    const long long tiles = DN_FOUR_WAVE_TILES_PER_CU * num_cus;
    return {dn_config_cut_by_dependency(c), dn_config_is_noisy(c) ? tiles * 2 / 3 : tiles};
}

// Five waves (normaliser on; round 3): the four-wave kernel with the normaliser on a wave of its own (NW = 5), where the report wave set
// the pace.  DN_WAVES=4 keeps the four-wave shape for A/B runs; see profiles/r03_notes.md.
// Two tiles per CU lie within the four-wave bound with and without noise (3 x 2 / 3 = 2).
inline DnShapeRule dn_rule_five_waves(const dn_config &c, int num_cus)
{
    return {dn_config_cut_by_dependency(c) && c.normalize_obs != 0, DN_FIVE_WAVE_TILES_PER_CU * num_cus};
}

// Role-pipelined kernel (round 4, dn_step_many_rp8_kernel: eight roles per tile; plain configuration with the normaliser, no noise).
// Fleet sweep, 64-step launches, us per step (five waves | eight roles; profiles/r04_sweep_rp.txt): 4 096 drones 1.08 | 0.93, 8 192
// 1.11 | 0.99, 16 384 1.18 | 1.05, 20 480 1.52 | 1.53, 24 576 1.53 | 1.57, 32 768 1.63 | 1.66, 40 960 2.79 | 2.37, 49 152 2.98 | 2.47
// -> eight roles up to one tile per CU and from two to three tiles per CU (where two of its workgroups fit a CU and the third tile
// follows), five waves in between, where sixteen waves saturate the vector ALUs either way.  Without the normaliser the six-role form
// lost to the four-wave kernel at every size (32 768 drones: 1.68 against 1.40) and was removed in round 5.
// Round 6, beyond three tiles per CU (one wave | eight roles, 64-step launches, the one-wave kernel 27 % faster than it was:
// profiles/r06_sweep_large.txt): 57 344 drones 3.41 | 2.53, 65 536 3.53 | 2.70, 81 920 4.56 | 3.37, 98 304 4.67 | 3.93, 114 688
// 4.76 | 4.58 (K = 20: 5.07 | 5.22), 131 072 4.86 | 5.16 -> eight roles up to six tiles per CU, one wave beyond.
// The one shape with a band instead of a bound: from two to three tiles per CU the four-wave kernel has won since (dn_rule_four_waves).
inline bool dn_eight_roles_take(const dn_config &c, int num_cus, long long blocks)
{
    const long long cus = num_cus;
    return dn_config_role_pipelined(c) && (blocks <= cus || (blocks > 3 * cus && blocks <= DN_ROLE_PIPE_TILES_PER_CU * cus));
}

// The measured pick of dn_step_many (k > 1): the first rule that takes the fleet.
inline int dn_pick_fused(const dn_config &c, int num_cus, long long blocks)
{
    if (dn_eight_roles_take(c, num_cus, blocks)) return 8;
    if (dn_rule_five_waves(c, num_cus).takes(blocks)) return 5;
    if (dn_rule_four_waves(c, num_cus).takes(blocks)) return 4;
    if (dn_rule_three_waves(c, num_cus).takes(blocks)) return 3;
    if (dn_rule_two_waves(c, num_cus).takes(blocks)) return 2;
    return 1;
}

// dn_step (one control step per launch) is latency bound: 1.65 us of kernel boundary that an empty kernel already pays
// (profiles/r03_dispatch_floor.txt; the 2.9 us of round 2 was the host's eager launch cadence), a ~1.2 us memory round trip
// with nothing to overlap it, plus the dependent instruction stream of the step.  Cutting the step
// by dependency over three waves (dn_step_pqx_kernel) shortens that stream while the chip has idle SIMDs; built for the
// plain configuration without the ground-contact term.  DN_WAVES_SINGLE=1|3 overrides the pick (sweeps).
// Measured (profiles/r02_sweep_single.txt, us per step, one wave / three waves): 32768 drones 6.4 / 4.7, 65536: 7.7 / 6.8,
// 98304: 9.5 / 9.8; with the normaliser 32768: 8.7 / 6.8, 49152: 9.5 / 10.9 -> three waves up to 1024 tiles, 512 with the
// normaliser's statistics (27 float64 per drone through one wave's loads and stores).
inline DnShapeRule dn_rule_three_wave_single(const dn_config &c, int num_cus)
{
    const long long tiles = DN_PQX_TILES_PER_CU * num_cus;
    return {dn_config_cut_by_dependency(c), c.normalize_obs ? tiles / 2 : tiles};
}

// The measured pick of dn_step (k == 1).
inline int dn_pick_single(const dn_config &c, int num_cus, long long blocks) { return dn_rule_three_wave_single(c, num_cus).takes(blocks) ? 3 : 1; }

// DN_WAVES: its FIRST character names a fused shape whatever the fleet size, and the single step follows it; any other first character
// (an empty value included) leaves `picked` as it is.  A shape the configuration's kernels do not have falls back to the nearest one below.
inline DnShapes dn_override_waves(DnShapes picked, const dn_config &c, const char *dn_waves)
{
    const bool cut = dn_config_cut_by_dependency(c);
    const int single = cut ? 3 : 1;
    const int widest_cut = cut ? (c.normalize_obs ? 5 : 4) : 3;
    switch (dn_waves ? dn_waves[0] : '\0') {
    case '1': return {1, 1};
    case '2': return {2, 2};
    case '3': return {3, single};
    case '4': return {cut ? 4 : 3, single};                            // the recurrence itself on two waves (dn_step_many_4w_kernel): plain configuration only
    case '5': return {widest_cut, single};                             // + the normaliser on a fifth wave (normaliser on only)
    case '8': return {dn_config_role_pipelined(c) ? 8 : widest_cut, single};   // the role-pipelined kernel (eight roles; normaliser on, no noise)
    default: return picked;
    }
}

// DN_WAVES_SINGLE: the first character again, 1 or 3 (3 only where the three-wave single step is built); the fused shape stays.
inline DnShapes dn_override_waves_single(DnShapes picked, const dn_config &c, const char *dn_waves_single)
{
    const char w = dn_waves_single ? dn_waves_single[0] : '\0';
    if (w == '1') picked.single = 1;
    else if (w == '3' && dn_config_cut_by_dependency(c)) picked.single = 3;
    return picked;
}

// The pick of dn_create.  `resolved`: the configuration after DN_GROUND_CONTACT_AUTO has become 0 or 1.  dn_waves / dn_waves_single: what
// getenv returned for DN_WAVES / DN_WAVES_SINGLE, or nullptr.
inline DnShapes dn_pick_shapes(const dn_config &resolved, int num_cus, const char *dn_waves, const char *dn_waves_single)
{
    const dn_config &c = resolved;
    const long long blocks = (c.num_envs + 63) / 64;
    DnShapes s = {dn_pick_fused(c, num_cus, blocks), dn_pick_single(c, num_cus, blocks)};
    s = dn_override_waves(s, c, dn_waves);
    s = dn_override_waves_single(s, c, dn_waves_single);
    const bool pid = c.action_type == 2 || c.action_type == 3 || c.action_type == 5;
    if (pid) return {1, 1};                 // the controller reads the step's entry state: one-wave kernels (dn_kernels.hip, PidCtx)
    if (c.random_spawn) return {1, 1};      // the spawn draw lives in the one-wave option kernels only
    return s;
}

#endif
