/*
 * dronenav.h -- C ABI of libdronenav.so: the MI355X-native vectorised drone-navigation
 * environment (hand-written HIP for gfx950).
 *
 * This is the drop-in boundary for the reference's hot path.  In the reference
 * (eRGiBi/DRL-DroneNavigation, pure Python, paths relative to /root/reference) that path is
 *     SB3 SubprocVecEnv(...)                          Sol/Model/PBDroneSimulator.py:653-666
 *       -> Monitor(NormalizeObservation(PBDroneEnv))  Sol/Model/PBDroneSimulator.py:154-196
 *         -> PBDroneEnv.step / reset                  Sol/Model/Environments/PBDroneEnv.py:171,609
 *           -> BaseAviary.step / reset                Sol/PyBullet/BaseAviary.py:324,276
 *             -> pybullet.stepSimulation              Sol/PyBullet/BaseAviary.py:439-440
 * i.e. N worker processes with one PyBullet world and one drone each.  Here one dn_env holds all
 * N drones of one GPU; dn_step() advances every drone by one control step (240 Hz) in a single
 * kernel launch and applies the VecEnv auto-reset in the same launch.
 *
 * Conventions
 *   - plain C, no torch types; all *device* pointers are raw HIP device addresses (e.g.
 *     tensor.data_ptr()), `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - the caller owns every I/O buffer; the library owns the persistent per-drone state allocated
 *     by dn_create() and freed by dn_destroy(); no caller buffer is retained across calls.
 *   - every function returns DN_OK (0) or a negative dn_status; dn_last_error() returns a
 *     thread-local message.  HIP errors are surfaced, never abort()ed.
 *   - a dn_env is used from one host thread at a time; work is enqueued on the caller's stream and
 *     the calls do not synchronise unless stated.
 *   - there is NO CPU fallback: without a HIP device dn_create() fails with DN_ERR_NO_DEVICE.
 */
#ifndef DRONENAV_H
#define DRONENAV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_ABI_VERSION 10
#define DN_MAX_WAYPOINTS 64
#define DN_OBS_DIM 13      /* 12 kinematic + distance, PBDroneEnv._computeObs, PBDroneEnv.py:296-336 */
#define DN_ACT_DIM 4       /* four rotor thrust commands, PBDroneEnv._actionSpace, PBDroneEnv.py:225-243 */
#define DN_MAX_LATENCY 8   /* deepest command pipeline of dn_enable_actuator, control steps (33 ms) */
#define DN_GROUND_CONTACT_AUTO 2   /* dn_config.ground_contact: resolved by dn_create (see the field) */

typedef enum dn_status {
    DN_OK = 0,
    DN_ERR_INVALID_ARGUMENT = -1,
    DN_ERR_HIP = -2,
    DN_ERR_OUT_OF_MEMORY = -3,
    DN_ERR_NO_DEVICE = -4,
    DN_ERR_BAD_STATE = -5
} dn_status;

/* Replaces the constructor arguments of PBDroneEnv (PBDroneEnv.py:41-65) as filled in by
 * PBDroneSimulator.make_env (PBDroneSimulator.py:154-171), plus the wrapper switches of
 * make_env (:181-196) and the SubprocVecEnv size (:653-666). */
typedef struct dn_config {
    int64_t num_envs;                           /* drones on this GPU (SubprocVecEnv's n_envs) */
    int32_t device_id;                          /* HIP device ordinal */
    int32_t num_waypoints;                      /* len(target_points), 1..DN_MAX_WAYPOINTS */
    double waypoints[DN_MAX_WAYPOINTS * 3];     /* target_points, row-major xyz */
    double spawn[3];                            /* initial_xyzs[0] */
    double aviary_dim[6];                       /* x_low y_low z_low x_high y_high z_high */
    double threshold;                           /* gate radius, 0.3 in PBDroneSimulator.py:116 */
    int32_t max_steps;                          /* --max_env_steps */
    int32_t circle;                             /* Track.is_circle: torus corridor around the unit circle at z=1 */
    int32_t cylinder;                           /* corridor check on (make_env passes True) */
    int32_t include_distance;                   /* obs[12] = distance/max_target_dist (True in the driver) */
    int32_t normalize_actions;                  /* PBDroneEnv.rescale_action (True in the driver) */
    int32_t normalize_obs;                      /* per-drone normalize.NormalizeObservation (always on in make_env) */
    int32_t ground_contact;                     /* len(p.getContactPoints())>0 vs plane.urdf (PBDroneEnv.py:699), which the reference always tests,
                                                   APPROXIMATED as: lowest point of the collision cylinder within Bullet's contact margin of z = 0
                                                   (the one term of the step that is neither pinned nor exact).  0 off | 1 on |
                                                   DN_GROUND_CONTACT_AUTO (2, the default): on unless the term is provably unreachable -- corridor
                                                   test on and every point low enough to touch the floor already outside the corridor of every track
                                                   segment, so that `terminated` cannot depend on it (true for the circle tracks at z = 1 and the
                                                   8-gate race track; false for the registry tracks that spawn at z = 0.1).  dn_create resolves it;
                                                   dn_get_config returns the resolved value */
    int32_t compute_f32;                        /* 0: float64 arithmetic in registers over the float32 state
                                                      (parity grade, default); 1: float32 arithmetic */
    float act_noise_sigma;                      /* sim-to-real: Gaussian action noise (0 = reference) */
    float obs_noise_sigma;                      /* sim-to-real: Gaussian observation noise (0 = reference) */
    uint64_t seed;                              /* Philox key for the noise streams */
    int64_t env_id_offset;                      /* global id of drone 0 (rank * num_envs when sharded) */
    int32_t clip_rew;                           /* --clip_rew: TransformReward(clip(r, -10, 10)), PBDroneSimulator.py:191-192 */
    int32_t norm_rew;                           /* --norm_rew: NormalizeReward(gamma .99, eps 1e-8), PBDroneSimulator.py:193-194
                                                   (normalize.py:100-147); both sit inside Monitor, clip first */
    int32_t physics;                            /* enums.Physics (enums.py:12-21) as dispatched by BaseAviary.step (BaseAviary.py:412-437):
                                                   0 PYB (what the reference always runs: :411 pins it) | 1 PYB_GND (_groundEffect, :800-832)
                                                   | 2 PYB_DRAG (_drag, :836-862) | 3 PYB_DW (_downwash: other drones of the same world,
                                                   none here -> as PYB) | 4 PYB_GND_DRAG_DW */
    int32_t action_type;                        /* 0 ActionType.THRUST (PBDroneEnv._preprocessAction, PBDroneEnv.py:872-895)
                                                   | 1 ActionType.RPM (BaseSingleAgentAviary.py:176-179: rpm = HOVER_RPM (1 + 0.05 a))
                                                   | 2 PID (a[0:3] = destination) | 3 VEL (a[0:3] direction, |a[3]| speed) | 4 ONE_D_RPM (a[0])
                                                   | 5 ONE_D_PID (a[0]): BaseSingleAgentAviary._preprocessAction (:180-222) with the
                                                   DSLPIDControl loop (Sol/PyBullet/DSLPIDControl.py) per drone; the action buffer stays [N, 4] */
    int32_t random_spawn;                       /* PBDroneEnv(random_spawn=True): every episode starts at a random point around a random track line
                                                   (PositionGenerator.generate_random_point_around_line, position_generator.py:121-152, max_distance
                                                   0.1, fed by the dormant block PBDroneEnv.py:622-627); draws are Philox words keyed by `seed`, the
                                                   global drone id and the vector step, so sharding does not move them.  0 = the reference as it runs */
    int32_t zero_damping;                       /* p.changeDynamics(linearDamping=0, angularDamping=0): the line the reference keeps commented out
                                                   (BaseAviary.py:571-573).  0 = Bullet's default damping 0.04 (1 + |v|), what the reference simulates */
} dn_config;

/* One drone's persistent state, host-side AoS view used by dn_get_state/dn_set_state (tests,
 * checkpointing).  Field names follow the reference's attributes.  It does not carry the body scales of
 * dn_enable_dynamics: a checkpoint of a randomised fleet is dn_get_state + dn_get_dynamics (restore: dn_set_state + dn_set_dynamics),
 * nor the wind of dn_enable_wind (+ dn_get_wind / dn_set_wind), nor the actuator state of dn_enable_actuator (+ dn_get_actuator /
 * dn_set_actuator), nor the sensor state of dn_enable_sensor (+ dn_get_sensor / dn_set_sensor), nor the track of dn_enable_tracks
 * (+ dn_get_tracks; restore: dn_set_tracks BEFORE dn_set_state, which holds idx to the drone's own track).
 * A record written by dn_get_state and handed back to dn_set_state restores every device word bit for bit, the observation normaliser's
 * included (rms_m2, ABI 10): a restored, resharded or set_attr-edited fleet continues with the bits of the uninterrupted one.  With
 * normalize_obs dn_set_state refuses an rms_count that is not positive and finite. */
typedef struct dn_env_state {
    float pos[3], quat[4], vel[3], ang_v[3];    /* Bullet base state, BaseAviary.py:596-598 (quat = x,y,z,w) */
    float prev_vel[3], prev_ang_v[3];           /* PBDroneEnv.prev_vel / prev_ang_v */
    float cur_pos[3];                           /* PBDroneEnv._current_position (stale copy, quirk Q3) */
    float d, d_prev;                            /* _distance_to_target, _prev_distance_to_target */
    int32_t idx;                                /* _current_target_index */
    int32_t steps;                              /* _steps */
    int32_t just_found;                         /* just_found */
    float ep_ret;                               /* Monitor: running episode return (high word, see ep_ret_lo) */
    int32_t ep_len;                             /* Monitor: running episode length */
    double rms_mean[DN_OBS_DIM];                /* normalize.RunningMeanStd.mean  (normalize_obs only) */
    double rms_var[DN_OBS_DIM];                 /*                         .var  (the device carries the second moment var x count: rms_m2 below) */
    double rms_count;                           /*                         .count                     */
    double rr_returns;                          /* NormalizeReward.returns (discounted return, norm_rew only)  */
    double rr_mean, rr_var, rr_count;           /* NormalizeReward.return_rms                                  */
    float last_rpm[4];                          /* BaseAviary.last_clipped_action (physics with drag only; zeros otherwise) */
    double pid[9];                              /* DSLPIDControl.integral_pos_e, .last_rpy, .integral_rpy_e (action types PID / VEL / ONE_D_PID) */
    float ep_ret_lo;                            /* Monitor: low part of the running return -- the return is ep_ret + ep_ret_lo, ep_ret_lo a multiple k/256
                                                   (k a signed byte) of ep_ret's ulp, so that the float64 sum SB3's Monitor keeps is not re-rounded to
                                                   24 bits every step; dn_set_state rounds what it is given to that grid */
    double rms_m2[DN_OBS_DIM];                  /* the device's own words M2 = .var x .count (normalize_obs only; ABI 10, appended: no earlier offset moved).
                                                   dn_get_state fills them verbatim beside rms_var = M2 / count.  dn_set_state takes rms_m2[k] as it is while
                                                   rms_count > 0, rms_m2[k] is finite and rms_m2[k] / rms_count == rms_var[k] -- a blob then restores the
                                                   statistics bit for bit, which rms_var alone cannot (neighbouring M2 divide to the same var) -- and
                                                   otherwise rebuilds M2 from rms_var and rms_count: an edited var or count is honoured with rms_m2 left
                                                   stale, and a producer that does not know the field leaves it zero */
} dn_env_state;

/* Wave-reduced episode statistics accumulated on the device since dn_create / dn_reset_stats. */
typedef struct dn_stats {
    int64_t env_steps;                          /* drone steps simulated */
    int64_t episodes;                           /* episodes finished (done flags raised) */
    int64_t truncated;                          /* of which TimeLimit.truncated */
    int64_t completed;                          /* of which all waypoints reached (+200 branch) */
    int64_t sum_ep_len;                         /* sum of Monitor 'l' */
    int64_t sum_found_targets;                  /* sum of info['found_targets'] at episode end */
    double sum_ep_return;                       /* sum of Monitor 'r' (fixed-point 1e-6 accumulation) */
} dn_stats;

typedef struct dn_env dn_env;

int32_t dn_abi_version(void);
const char *dn_last_error(void);
int32_t dn_device_count(void);

/* Fills *cfg with the driver's literals (threshold 0.3, max_steps 4096, cylinder, include_distance,
 * normalize_actions on; ground_contact = DN_GROUND_CONTACT_AUTO; circle/normalize_obs/noise off) and an empty track. */
void dn_config_default(dn_config *cfg);

/* Replaces N x PBDroneEnv.__init__ + the env.reset(seed=seed+rank) of make_env
 * (PBDroneSimulator.py:154-173).  Allocates the device state. */
int32_t dn_create(const dn_config *cfg, dn_env **out);
int32_t dn_destroy(dn_env *env);
int64_t dn_num_envs(const dn_env *env);
/* The configuration the environment runs with: *out = the dn_config given to dn_create with ground_contact resolved
 * to 0 / 1 (ABI 6).  What `PBDroneEnv.__dict__` answers in the reference. */
int32_t dn_get_config(const dn_env *env, dn_config *out);
/* What dn_create makes of cfg->ground_contact (host arithmetic on the track geometry only, no device needed): 0 / 1, or a
 * negative dn_status for an invalid configuration (ABI 6). */
int32_t dn_resolve_ground_contact(const dn_config *cfg);
/* Compute units of the environment's device (hipDeviceProp_t.multiProcessorCount): the kernel-shape crossovers below are
 * tiles (64 drones) per CU, calibrated on the 256-CU MI355X (ABI 6). */
int32_t dn_get_num_cus(const dn_env *env);

/* Replaces VecEnv.reset() -> N x Monitor.reset/NormalizeObservation.reset/PBDroneEnv.reset
 * (PBDroneEnv.py:609-665, BaseAviary.py:276-320).  obs: device float[N*13]. */
int32_t dn_reset(dn_env *env, float *obs, void *stream);

/* Replaces VecEnv.step_async+step_wait -> N x worker step (PBDroneEnv.step, PBDroneEnv.py:171-199)
 * with SubprocVecEnv auto-reset and Monitor statistics.  All pointers are device pointers:
 *   actions       const float[N*4]   policy output in [-1,1] (action_space, PBDroneEnv.py:230-236)
 *   obs           float[N*13]        next observation (already the reset observation where done)
 *   reward        float[N]
 *   done          uint8[N]           terminated || truncated
 *   truncated     uint8[N]           info["TimeLimit.truncated"] = truncated && !terminated
 *   found_targets int32[N]           info["found_targets"] (PBDroneEnv.py:442)
 *   terminal_obs  float[N*13]|NULL   info["terminal_observation"]; rows written only where done
 *   ep_return     float[N]|NULL      Monitor info["episode"]["r"]; written only where done
 *   ep_length     int32[N]|NULL      Monitor info["episode"]["l"]; written only where done
 *   done_mask     uint64[ceil(N/64)]|NULL  one wave-ballot word per 64 drones (bit l = drone 64*w+l done) */
int32_t dn_step(dn_env *env, const float *actions, float *obs, float *reward, uint8_t *done,
                uint8_t *truncated, int32_t *found_targets, float *terminal_obs, float *ep_return,
                int32_t *ep_length, uint64_t *done_mask, void *stream);

/* k consecutive control steps enqueued back-to-back (open-loop action sequences: replays, random-action
 * collection, benchmarks).  Every buffer is step-major [k, N, ...] -- the (n_steps, n_envs, ...) layout of an
 * SB3 RolloutBuffer -- with the same meaning and optionality as in dn_step; done_mask is [k, ceil(N/64)].
 * N must be a multiple of 4 so that every step's obs slice stays 16-byte aligned. */
int32_t dn_step_many(dn_env *env, int64_t k, const float *actions, float *obs, float *reward, uint8_t *done,
                     uint8_t *truncated, int32_t *found_targets, float *terminal_obs, float *ep_return,
                     int32_t *ep_length, uint64_t *done_mask, void *stream);

/* Rows A5-A9 of a control step on their own (plus the A10/A11 wrappers): the rigid-body transition of the step -- what
 * p.stepSimulation (BaseAviary.py:439-440) leaves in Bullet -- is GIVEN, and everything the reference does with it runs
 * through the same device code as dn_step: _updateAndStoreKinematicInformation / getEulerFromQuaternion
 * (BaseAviary.py:588-598), _computeObs (PBDroneEnv.py:296-398), _computeReward (:475-607), _computeTerminated /
 * _computeTruncated (:444-473, :678-786), _update_state_post_step (:196-223), and on done the SubprocVecEnv auto-reset
 * (:609-665) with Monitor's record.  The persistent state advances exactly as in dn_step (the given pose and velocities
 * become the body state).  Exists so that fixtures which script a kinematic sequence reach the HIP path directly.
 *   kinematics    const double[N*13]  per drone pos(3) quat(4: x,y,z,w, unit) vel(3) ang_v(3), world frame, float64 as
 *                                     the reference holds them (the velocities are rounded to float32, the state's type)
 *   other buffers as in dn_step.  Reference configuration only (no noise / reward wrappers / extra physics). */
int32_t dn_eval_kinematics(dn_env *env, const double *kinematics, float *obs, float *reward, uint8_t *done,
                           uint8_t *truncated, int32_t *found_targets, float *terminal_obs, float *ep_return,
                           int32_t *ep_length, void *stream);

/* Episode-done compaction: expands the per-wave ballot words written by dn_step into the ordered
 * list of finished drones (what the host needs to build the per-env `infos` of SubprocVecEnv
 * without scanning N flags).  indices: device int32[N]; count: device int32[1]. */
int32_t dn_compact_done(const uint64_t *done_mask, int64_t num_envs, int32_t *indices, int32_t *count,
                        int32_t device_id, void *stream);

/* dn_compact_done plus, for every finished drone in index order, its episode-end record as one row of 16 float32 words:
 * terminal_observation[13] (SubprocVecEnv's info["terminal_observation"]), Monitor's episode return, its length (int32 bits) and
 * TimeLimit.truncated | found_targets << 8 (int32 bits) -- what SubprocVecEnv's worker puts into `info` when an episode ends
 * (PBDroneSimulator.py:653-666 with Monitor, :196).  The host copies count x 64 bytes instead of four whole per-drone arrays.
 * Inputs: the buffers the last dn_step wrote.  indices: device int32[N]; count: device int32[1]; packed: device float[N x 16]. */
int32_t dn_pack_done(const uint64_t *done_mask, int64_t num_envs, const float *terminal_obs, const float *ep_return, const int32_t *ep_length,
                     const uint8_t *truncated, const int32_t *found_targets, int32_t *indices, int32_t *count, float *packed,
                     int32_t device_id, void *stream);

/* Measurement helper ("a measured stream-copy ceiling on the box"): a hand-written float4 copy of `bytes` bytes
 * (a multiple of 16, both pointers 16-byte aligned, device memory) -- one 16-byte load and one 16-byte store per lane, one lane per
 * 16 bytes (the form that measured fastest: profiles/r04_copy_sweep.txt) -- enqueued on `stream`.  What bench.py quotes as `hbm_copy_ceiling` beside the
 * nominal 8 TB/s; it replaces no reference code. */
int32_t dn_stream_copy(void *dst, const void *src, int64_t bytes, int32_t device_id, void *stream);

/* Host <-> device copies of the whole persistent state (synchronous).  states: host array [N]. */
int32_t dn_get_state(dn_env *env, dn_env_state *states, int64_t count);
int32_t dn_set_state(dn_env *env, const dn_env_state *states, int64_t count);

/* Episode statistics (synchronises `stream`). */
int32_t dn_get_stats(dn_env *env, dn_stats *out, void *stream);
int32_t dn_reset_stats(dn_env *env, void *stream);

/* Kernel shape chosen for this environment's launches (fused != 0: dn_step_many with k > 1; fused == 0: dn_step), as waves
 * per 64-drone tile.  Fused: 8 = the role-pipelined kernel (thrust | linear + flags | angular | attitude | distance bookkeeping +
 * reward terms | scalars | the normaliser's two column halves; plain configuration with normalize_obs, no noise: up to 1 tile per CU
 * and from 2 to 3 tiles per CU), 5 = the four-wave shape
 * with the observation normaliser on a wave of its own (normalize_obs in the plain configuration, 1 to 2 tiles per CU -- 32 768 drones
 * on 256 CUs -- and with noise up to 3), 4 = the recurrence itself on two waves (linear + rules | angular + attitude) plus an observation
 * and a report wave (plain configuration up to 3 tiles per CU), 3 = flight + report + aux wave, 2 = a flight wave + a report wave
 * (mid-size fleets with the optional terms, where more waves cost occupancy), 1 = one wave.
 * Single step: 3 = three waves cut by dependency (dn_step_pqx_kernel, plain configuration up to 4 tiles per CU), 1 = one wave.
 * The multi-wave shapes win while the tiles alone leave SIMDs idle; crossovers are tiles per CU (dn_get_num_cus).  All shapes
 * produce identical bits -- on one device: the observation-noise draws (obs_noise_sigma > 0; 13 of a noisy step's 17 normals) use the
 * hardware's float32 log2 / sqrt / sin / cos (within 1.2e-6 of the float64 definition, tests/test_gpu_parity.py::
 * test_observation_noise_draws_match_their_definition), so noisy runs are bit-reproducible across kernel shapes, launches and shards
 * of one GPU generation, not across generations or against a CPU evaluation; everything that feeds the dynamics (action noise, policy
 * sampling, random spawn) and the whole noise-free configuration is exact arithmetic.  DN_EXACT_OBS_NOISE=1 (read by dn_create) draws the
 * observation noise in the exact form as well (bit-equal to the float64 definition for > 99.99 % of draws, one float32 ulp otherwise).
 * Environment variables DN_WAVES=1|2|3|4|5|8 and DN_WAVES_SINGLE=1|3 (read by dn_create) force a shape. */
int32_t dn_get_kernel_waves(const dn_env *env, int32_t fused);

/* The arithmetic switches dn_create resolved from the process environment (ABI 9), as a bit mask: a checkpoint or a shard restored in a
 * process with another setting would otherwise replay other observation noise / other last bits silently -- compare this value.
 *   DN_EXACT_FLAG_OBS_NOISE  DN_EXACT_OBS_NOISE=1: observation noise in the exact float64 Box-Muller form (see above).
 *   DN_EXACT_FLAG_NORM       DN_EXACT_NORM=1: the observation normaliser's OUTPUT stage in float64.  The running statistics are float64
 *                            and updated by the same expressions either way (normalize.py:34-47); the normalised value
 *                            (obs - mean) / sqrt(var + 1e-8) (normalize.py:94-97) leaves as a float32, and by default it is formed in
 *                            float32 on the hardware reciprocal square root: within 3 float32 ulp (3.6e-7 relative) of the float64
 *                            evaluation, 30x inside the 1e-5 parity bar, for a third less vector-ALU time in the normaliser.  With the
 *                            switch the output is the float32 nearest to the float64 evaluation (1/2 ulp).
 * Accepted values: 1 | true | on | yes and 0 | false | off | no (any case; unset or empty = off); anything else fails dn_create with
 * DN_ERR_INVALID_ARGUMENT. */
#define DN_EXACT_FLAG_OBS_NOISE 1
#define DN_EXACT_FLAG_NORM 2
int32_t dn_get_exact_flags(const dn_env *env);

/* Vector-step counter: the Philox counter word of the noise streams and the source of dn_stats.env_steps.  It
 * lives on the device and is advanced by the step kernels themselves, so dn_step / dn_step_many launches captured
 * into a hipGraph keep counting when the graph is replayed.  Both calls synchronise the device. */
int32_t dn_get_step_count(const dn_env *env, uint64_t *out);
int32_t dn_set_step_count(dn_env *env, uint64_t value);

/* The float32 action chain on its own: replaces N x PBDroneEnv._preprocessAction (PBDroneEnv.py:872-895, with
 * rescale_action :949-971 and env_utils.cmd2pwm / pwm2rpm, env_utils.py:8-59) plus the rotor force / torque lines of
 * BaseAviary._physics (BaseAviary.py:776-780).  dn_step runs exactly this code in-kernel; the entry point exists so
 * the chain can be checked bit for bit.  actions: device float[N*4]; rpm, forces: device float[N*4] or NULL;
 * z_torque: device float[N] or NULL (at least one output). */
int32_t dn_preprocess_action(const float *actions, int64_t num_envs, int32_t normalize_actions, float *rpm,
                             float *forces, float *z_torque, int32_t device_id, void *stream);

/* Generalised advantage estimation on device buffers laid out [n_steps, n_envs]
 * (the reference's only in-tree statement of the recursion: Sol/Model/Algorithms/cleanRLPPO.py:234-248).
 * dones[t] is the episode-start flag of step t (cleanRL: dones[t] = next_done before step t),
 * last_values/last_dones are V(s_T) and the done flag after the final step. */
int32_t dn_gae(const float *rewards, const float *values, const uint8_t *dones,
               const float *last_values, const uint8_t *last_dones, int64_t n_steps, int64_t n_envs,
               double gamma, double gae_lambda, float *advantages, float *returns,
               int32_t device_id, void *stream);

/* One network of the reference's agents, by `arch`:
 *   DN_MLP_ARCH_PPO (0)  actor or critic of SB3's ActorCriticPolicy with net_arch pi = vf = [512, 512, 256], Tanh
 *                        (Sol/Model/PBDroneSimulator.py:251-286): obs -> 512 -> 512 -> 256 -> out_dim;
 *   DN_MLP_ARCH_SAC (1)  latent_pi + heads of SB3's SAC Actor with net_arch pi = [256, 256], ReLU
 *                        (Sol/Model/PBDroneSimulator.py:297-303): obs -> 256 -> 256 -> out_dim, the mu and log_std heads stacked
 *                        into one [8, 256] matrix (rows 0..3 mu, 4..7 log_std); w3 / b3 are unused and may be NULL.
 * Weights are bfloat16 in the fragment order of the kernel (drl-dronenavigation_amd/policy_mfma.py::pack_mlp / pack_sac_actor
 * produce it from the [out, in] float32 matrices), biases float32 padded to a multiple of 32 (the head's to 32).  All pointers
 * are device pointers.
 * w1 for input rows of more than 16 columns (DN_MLP_ARCH_PPO only): layer 1 runs KS1 = 2 (obs_dim <= 32) or 4 (obs_dim <= 64) K-steps of
 * 16 inputs -- input k sits in K-step k >> 4, lane group (k >> 3) & 1, slot k & 7, columns at and beyond obs_dim are zero -- and w1 holds,
 * per M-tile of 32 output rows, the KS1 fragments (64 lanes x 8 values) in K-step order; in the float32 grade the KS1 hi fragments and then
 * the KS1 lo fragments, the rule of the other layers.  obs_dim <= 16 is KS1 = 1: the layout it always had. */
#define DN_MLP_ARCH_PPO 0
#define DN_MLP_ARCH_SAC 1
typedef struct dn_mlp_net {
    const void *w1, *w2, *w3, *wh;              /* packed bf16 weights of the hidden layers and the head */
    const float *b1, *b2, *b3, *bh;             /* biases */
    float *out;                                 /* float[num_envs * out_dim] */
    int32_t out_dim;                            /* 1..32 (4 action means / 1 value / 8 = mu | log_std) */
    int32_t grade;                              /* 0: bf16 weights and activations, float32 accumulate (the speed option, ~1e-3 on the action mean)
                                                   1: float32 grade -- both operands split into two bf16 words, three MFMAs per product
                                                      (pack_mlp / pack_sac_actor(..., grade="fp32") pack the hi / lo fragment streams); matches the
                                                      reference's float32 networks to <= 1e-4.
                                                   2: float16 weights and activations, float32 accumulate: the speed of grade 0 with an
                                                      eighth of its rounding error (11 mantissa bits: ~1e-3 on the action mean).
                                                   All networks of one call share grade and arch. */
    int32_t arch;                               /* DN_MLP_ARCH_* (appended in ABI 5) */
    int32_t reserved_;                          /* 0 */
} dn_mlp_net;

/* Forward pass of one or two such networks over the same observations in one launch (replaces the mlp_extractor +
 * action_net / value_net part of SB3's ActorCriticPolicy.forward / predict_values): a fused MFMA kernel, one wavefront
 * per 32 drones, activations resident in registers.  obs: device float[num_envs * obs_dim], ONE tensor per call (a caller with two sources
 * concatenates them), read as it is (no rescaling); obs_dim in 1..64 for DN_MLP_ARCH_PPO, in 1..16 for DN_MLP_ARCH_SAC, anything else is
 * DN_ERR_INVALID_ARGUMENT.  Every w1 of the call must be packed for that obs_dim's KS1.  Rows of 17..64 columns run wide forms of the
 * default four-wave kernel (grades 0 and 2) and of the float32-grade kernel, whatever DN_MLP_SHAPE says.
 * row_mask: device uint8[num_envs] or NULL; with a mask, a 32-drone tile without a flagged drone writes zeros and
 * skips the network (V(terminal_observation) is needed only where an episode hit the time limit). */
int32_t dn_mlp_forward(const dn_mlp_net *nets, int32_t num_nets, const float *obs, const uint8_t *row_mask,
                       int64_t num_envs, int32_t obs_dim, int32_t device_id, void *stream);

/* The small element-wise steps of SB3's OnPolicyAlgorithm.collect_rollouts around the policy network, as kernels
 * [3P-recall of SB3]:
 *   dn_policy_sample  DiagGaussianDistribution.sample + log_prob and the np.clip(actions, -1, 1) handed to env.step:
 *                     actions = mean + exp(log_std) z with z ~ N(0,1) from the environment's Philox streams (seed, global
 *                     drone id, the vector-step counter; reproducible under hipGraph replay), `clipped` = the copy that goes
 *                     to dn_step, log_prob = sum over the 4 action dims.  mean/actions/clipped: device float[N*4];
 *                     log_std: HOST float[4]; log_prob: device float[N].
 *   dn_add_bootstrap  reward[i] += gamma * terminal_value[i] where truncated[i] (TimeLimit bootstrap). */
int32_t dn_policy_sample(dn_env *env, const float *mean, const float *log_std, uint64_t seed, int32_t deterministic,
                         float *actions, float *clipped, float *log_prob, void *stream);
/* The SAC actor's sampling step on top of dn_mlp_forward(arch = DN_MLP_ARCH_SAC) (replaces SB3's Actor.forward /
 * action_log_prob after latent_pi, Sol/Model/PBDroneSimulator.py:297-338) [3P-recall of SB3]: log_std clamped to [-20, 2],
 * actions = tanh(mu + exp(log_std) z), z ~ N(0,1) from the environment's Philox streams exactly as dn_policy_sample draws it
 * (seed, global drone id, vector-step counter; reproducible under hipGraph replay and independent of the sharding); the result
 * lies inside dn_step's action box.  mu_log_std: device float[N*8], rows (mu[4], log_std[4]); actions: device float[N*4];
 * log_prob: device float[N] or NULL (sum over the four dims of log N(pre; mu, sigma) - log(1 - a^2 + 1e-6)). */
int32_t dn_squashed_sample(dn_env *env, const float *mu_log_std, uint64_t seed, int32_t deterministic, float *actions,
                           float *log_prob, void *stream);
/* dn_squashed_sample + dn_step in one launch (the SAC collection loop's per-step pair): the action is drawn inside the step
 * kernel from the (mu | log_std) rows exactly as dn_squashed_sample draws it (same Philox stream, same bits); actions_out
 * receives it (the replay buffer's action), log_prob_out (may be NULL) its log-probability.  Other arguments as dn_step; same
 * configuration limits as dn_step_sampled. */
int32_t dn_step_squashed(dn_env *env, const float *mu_log_std, uint64_t seed, int32_t deterministic, float *actions_out,
                         float *log_prob_out, float *obs, float *reward, uint8_t *done, uint8_t *truncated,
                         int32_t *found_targets, float *terminal_obs, float *ep_return, int32_t *ep_length,
                         uint64_t *done_mask, void *stream);
int32_t dn_add_bootstrap(float *reward, const float *terminal_value, const uint8_t *truncated, double gamma,
                         int64_t num_envs, int32_t device_id, void *stream);
/* dn_policy_sample + dn_step in one launch (the rollout loop's per-step pair): the action is drawn inside the step kernel
 * from `mean` exactly as dn_policy_sample draws it (same Philox stream, same bits); actions_out receives the UNclipped
 * action (what SB3's collect_rollouts stores), log_prob_out its log-probability, the clipped action goes into the step.
 * Other arguments as dn_step.  Built for the configuration without reward wrappers / extra physics terms / RPM actions /
 * random spawn / zero damping (DN_ERR_INVALID_ARGUMENT otherwise: use dn_policy_sample + dn_step there). */
int32_t dn_step_sampled(dn_env *env, const float *mean, const float *log_std, uint64_t seed, int32_t deterministic,
                        float *actions_out, float *log_prob_out, float *obs, float *reward, uint8_t *done, uint8_t *truncated,
                        int32_t *found_targets, float *terminal_obs, float *ep_return, int32_t *ep_length,
                        uint64_t *done_mask, void *stream);

/* dn_mlp_forward + dn_step_sampled in ONE launch (ABI 6): the policy kernel's workgroup that evaluated the actor (nets[0], out_dim 4)
 * for 128 drones (64 in the float32 grade) draws their actions and runs their control step before it leaves -- no kernel boundary
 * and no round trip of the action means between the policy and the environment (SB3 collect_rollouts' forward -> sample -> clip ->
 * env.step, Sol/Model/PBDroneSimulator.py:261-286).  nets[1] (optional) is the critic, evaluated by the other workgroups of the same
 * launch; both write their `out` as dn_mlp_forward does.  policy_obs: device float[N * obs_dim], the observation the networks read
 * (must not alias `obs`, the step's output).  Same results, bit for bit, as the two calls it replaces when dn_mlp_forward runs its pair
 * shape (DN_MLP_SHAPE=8: the kernel this launch extends; the default four-wave shape sums K in another order).  Limits: PPO arch, the float64
 * reference configuration without noise / reward wrappers / extra physics / ground contact, fleets on which dn_create picked the
 * three-wave single step (dn_get_kernel_waves(env, 0) == 3), num_envs a multiple of 128 (64 in the float32 grade);
 * DN_ERR_INVALID_ARGUMENT otherwise (use the two calls). */
int32_t dn_mlp_step_sampled(dn_env *env, const dn_mlp_net *nets, int32_t num_nets, const float *policy_obs, int32_t obs_dim,
                            const float *log_std, uint64_t seed, int32_t deterministic, float *actions_out, float *log_prob_out,
                            float *obs, float *reward, uint8_t *done, uint8_t *truncated, int32_t *found_targets, float *terminal_obs,
                            float *ep_return, int32_t *ep_length, uint64_t *done_mask, void *stream);

/* Measurement hook (ABI 8; lifetime rules ABI 9).  The step kernel of the NEXT dn_step / dn_step_many / dn_step_sampled / dn_step_squashed call on `env` is dispatched with these two hipEvents
 * (hipEvent_t passed as void *, created with timing enabled; either may be NULL) attached to its own dispatch packet
 * (hipExtLaunchKernelGGL): hipEventElapsedTime(start, stop) is then the duration of that kernel alone -- what a profiler's kernel trace
 * reports -- where a pair of hipEventRecord around the call also times the host's launch path and puts two marker packets on the
 * stream.  One shot: consumed by the next step-family call on `env` whatever its outcome -- a call that fails validation, dn_eval_kinematics
 * and dn_mlp_step_sampled (no hook) DROP the events instead of leaving them armed for a later launch.  An armed launch cannot be
 * captured into a hipGraph (DN_ERR_INVALID_ARGUMENT if the stream is capturing).  It stands where the reference wraps its training loop in cProfile
 * (Sol/Utilities/Profiler.py:5-16), at the granularity this path has: one launch.  Used by bench.py's roofline figure. */
int32_t dn_set_launch_events(dn_env *env, void *start_event, void *stop_event);

/* Bytes of HBM the persistent state of `num_envs` drones occupies (capacity planning).  The body scales of dn_enable_dynamics are a
 * separate allocation of 16 bytes per drone and are not included, nor is the wind of dn_enable_wind (32 bytes per drone), nor the
 * actuator state of dn_enable_actuator (152 bytes per drone), nor the sensor state of dn_enable_sensor (1092 bytes per drone). */
int64_t dn_state_bytes(int64_t num_envs, int32_t normalize_obs);

/* Per-drone dynamics randomisation (sim-to-real).  Each drone carries four float32 scale factors relative to the nominal cf2x body:
 *   s_m   mass: linear acceleration = R F / (M s_m) - g (gravity stays g); the drag force of Physics.PYB_DRAG also accelerates M s_m
 *   s_I   inertia: diag(Ixx, Iyy, Izz) s_I in I w, the gyroscopic term and I^-1 (Bullet's damping form unchanged)
 *   s_kf  thrust coefficient: every rotor force after the action chain, ground effect included (it is KF rpm^2 coeff)
 *   s_km  torque coefficient: the yaw torque after the chain
 * The action chain (rescale_action -> cmd2pwm -> pwm2rpm), HOVER_RPM of ActionType.RPM and the DSLPIDControl loop stay NOMINAL: they model
 * the drone a flight stack knows, only the simulated body differs.  Scales of 1 reproduce the nominal arithmetic bit for bit.
 * resample = 1: every episode start (dn_reset and every in-kernel auto-reset) draws new scales, each lo + (hi - lo) u in float64 stored as
 * float32, u = (r + 0.5) / 2^32, the four words r from ONE Philox4x32-10 call keyed (seed; global drone id, the vector-step counter of
 * the step the episode starts on, stream 13) -- sharding does not move the draws, and a hipGraph replay keeps drawing fresh ones.  New
 * scales act from the first physics step of the new episode; the reset observation does not depend on them.  resample = 0: the scales
 * are what dn_set_dynamics last wrote (1 after the first dn_enable_dynamics).
 * The scales live in the one-wave option kernels: enabling forces dn_get_kernel_waves(env, 0 / 1) == 1.  dn_step_sampled,
 * dn_step_squashed, dn_mlp_step_sampled and dn_eval_kinematics refuse an env with dynamics enabled (DN_ERR_INVALID_ARGUMENT): use
 * dn_policy_sample / dn_squashed_sample + dn_step. */
typedef struct dn_dynamics_config {
    float mass[2], inertia[2], kf[2], km[2];   /* scale ranges [lo, hi]: 0 < lo <= hi, finite */
    int32_t resample;                          /* 1: draw at every episode start; 0: keep dn_set_dynamics' values */
    int32_t reserved;                          /* must be 0 */
} dn_dynamics_config;
/* Validates the ranges and enables the feature.  The first call allocates 16 bytes per drone (outside dn_state_bytes) and sets every
 * scale to 1; a later call changes the ranges and `resample` and keeps the current scales.  Synchronises the device. */
int32_t dn_enable_dynamics(dn_env *env, const dn_dynamics_config *cfg);
/* Device [N][4] float32 rows (s_m, s_I, s_kf, s_km), copied on `stream`; DN_ERR_BAD_STATE if dynamics are not enabled.  dn_set_dynamics
 * does not validate the values (the caller's device buffer is not read on the host): every scale must be positive and finite. */
int32_t dn_set_dynamics(dn_env *env, const float *scales, void *stream);
int32_t dn_get_dynamics(dn_env *env, float *scales, void *stream);
/* 1: dynamics enabled, *out = the configuration last given to dn_enable_dynamics; 0: not enabled (*out untouched); < 0: error. */
int32_t dn_get_dynamics_config(const dn_env *env, dn_dynamics_config *out);

/* Per-drone wind (sim-to-real external disturbance).  Each drone carries a steady wind wbar and a gust g (float32 x 3, world frame, m/s)
 * that push it with F_w = (k_xy w_x, k_xy w_y, k_z w_z) N, w = wbar + g, at the centre of mass (no torque): F_w / (M s_m) joins the
 * linear acceleration in every physics mode (s_m = the mass scale of dn_enable_dynamics, 1 without).  Bullet's damping and the
 * PYB_DRAG / ground-effect terms keep using the ground velocity.  The defaults of coeff are the cf2x rotor-drag coefficients at hover,
 * k = DRAG_COEFF 4 HOVER_RPM 2 pi / 60 = (5.5626e-3, 6.2490e-3) N s / m: a 5 m/s wind is about 1.03 m/s^2 on the nominal body.
 *   steady:  resample = 1: every episode start (dn_reset and every in-kernel auto-reset) draws, from ONE Philox4x32-10 call keyed
 *            (seed; global drone id, the vector step the episode starts on, stream 14) with u_j = (r_j + 0.5) / 2^32, in float64:
 *            s = speed lo + (hi - lo) u0, theta = azimuth lo + (hi - lo) u1 (the direction the air moves toward), v = vertical lo +
 *            (hi - lo) u2, and stores wbar = (s cos theta, s sin theta, v) as float32.  resample = 0: wbar is what dn_set_wind last wrote.
 *   gust:    an Ornstein-Uhlenbeck process with correlation time tau and stationary standard deviation sigma = (sigma_xy, sigma_xy,
 *            sigma_z).  a = exp(-dt / tau), dt = 1/240, b = sigma sqrt(1 - a^2) (float64 on the host).  After the physics of vector
 *            step sc: g <- float32(a g + b xi), xi = the first three normal draws of (seed; drone id, sc, stream 15) (Box-Muller in
 *            float64, as the action noise).  An episode start at sc, whatever resample is, sets g = float32(sigma xi'), xi' from stream 16:
 *            a draw from the stationary law, taken instead of the update.  sigma = (0, 0) switches the process off: no draws, g keeps
 *            its value and becomes 0 at the drone's next episode start.
 * New values act from the first physics step of the new episode; the reset observation does not depend on them.  wbar and g are float32
 * state: a fused launch of K steps equals K single steps bit for bit.  A checkpoint is dn_get_state + dn_get_wind + dn_get_step_count.
 * The wind lives in the one-wave option kernels: enabling forces dn_get_kernel_waves(env, 0 / 1) == 1.  dn_step_sampled,
 * dn_step_squashed, dn_mlp_step_sampled and dn_eval_kinematics refuse an env with wind enabled (DN_ERR_INVALID_ARGUMENT). */
typedef struct dn_wind_config {
    float speed[2];       /* horizontal steady speed [lo, hi], m/s: 0 <= lo <= hi, finite */
    float azimuth[2];     /* direction the air moves toward, radians [lo, hi]: finite, lo <= hi */
    float vertical[2];    /* vertical steady component [lo, hi], m/s: finite, lo <= hi */
    float gust_sigma[2];  /* stationary gust standard deviation (xy, z), m/s: finite, >= 0 */
    float gust_tau;       /* gust correlation time, s: finite, > 0 */
    float coeff[2];       /* (k_xy, k_z), N s / m: finite, >= 0 */
    int32_t resample;     /* 1: draw wbar at every episode start; 0: keep dn_set_wind's */
    int32_t reserved;     /* must be 0 */
} dn_wind_config;
/* Validates the configuration and enables the feature.  The first call allocates 32 bytes per drone (outside dn_state_bytes) and sets
 * wbar = g = 0 (still air until each drone's next episode start, unless dn_set_wind writes them); a later call changes the
 * configuration and keeps the current values.  Synchronises the device. */
int32_t dn_enable_wind(dn_env *env, const dn_wind_config *cfg);
/* Device [N][4] float32 rows (x, y, z, 0) of wbar (`mean`) and g (`gust`), copied on `stream`; NULL = leave (set) / skip (get).
 * DN_ERR_BAD_STATE if wind is not enabled.  dn_set_wind does not validate the values (the caller's device buffers are not read on the
 * host): every value must be finite. */
int32_t dn_set_wind(dn_env *env, const float *mean, const float *gust, void *stream);
int32_t dn_get_wind(dn_env *env, float *mean, float *gust, void *stream);
/* 1: wind enabled, *out = the configuration last given to dn_enable_wind; 0: not enabled (*out untouched); < 0: error. */
int32_t dn_get_wind_config(const dn_env *env, dn_wind_config *out);

/* Per-drone actuator model (sim-to-real): command latency and motor lag between the action handed to dn_step and the rotors.
 *   latency: every drone has an integer latency d in [0, DN_MAX_LATENCY] control steps.  At a control step which the drone enters with
 *            episode step counter s (dn_env_state.steps), the action chain consumes the action commanded d vector steps ago if s >= d, and
 *            `fill` otherwise: the pipeline of a fresh episode holds no command of that episode yet, and commands of the previous episode
 *            never leak into the next one.  The rule is stateless apart from a per-drone history of the last 8 commanded actions (128
 *            bytes), so dn_set_state needs no special case.  Action noise (act_noise_sigma) is drawn and added when a command is CONSUMED,
 *            keyed by the vector step of consumption: an env with latency equals, bit for bit, the same env without latency fed the
 *            shifted actions.  Works with every action_type.  The buffers of dn_step keep holding the COMMANDED action.
 *   lag:     each drone carries four effective rotor speeds r (float32) and a coefficient a = exp(-dt / tau) (float32, dt = 1/240; tau = 0
 *            gives a = 0).  After the nominal action chain has produced the commanded speeds c (float32, pwm2rpm),
 *            r <- float32(a r + (1 - a) c), evaluated in the compute type (compute_f32) in exactly this nesting, unfused; the rotor forces
 *            KF r^2 and the yaw torque from KM r^2 are formed from r in float32 as BaseAviary._physics forms them from c, and everything
 *            downstream (ground effect, PYB_DRAG's last_rpm, s_kf, s_km) sees r.  a = 0 reproduces c exactly.  An episode start sets
 *            r = rpm_fill, the chain's speeds for `fill`, evaluated once by dn_enable_actuator on the device (the dn_preprocess_action
 *            path).  motor_tau = [0, 0] switches the filter off: the nominal bits, `coeff` is not read and `rpm` only changes at episode
 *            starts.  Any other range needs ActionType.THRUST (DN_ERR_INVALID_ARGUMENT otherwise; latency stays available).
 *   draws:   resample = 1: every episode start (dn_reset and every in-kernel auto-reset) draws from ONE Philox4x32-10 call keyed (seed;
 *            global drone id, the vector step the episode starts on, stream 17) with u_j = (r_j + 0.5) / 2^32 in float64:
 *            d = latency lo + floor((hi - lo + 1) u_0) clamped to hi; tau = tau lo + (tau hi - tau lo) u_1, a = float32(exp(-dt / tau))
 *            (the device library's exp, at episode starts only), a = 0 where tau = 0.  Sharding does not move the draws, and a hipGraph
 *            replay keeps drawing fresh ones.  resample = 0: d and a are what dn_set_actuator last wrote (0 and 0 after the first enable).
 * New values act from the first step of the new episode; the terminal step and the reset observation do not depend on them.  r, a, d and
 * the history are held in registers / gathered per lane across a fused launch and stored at its end: K steps in one launch equal K
 * single steps bit for bit.  A checkpoint is dn_get_state + dn_get_actuator + dn_get_step_count.
 * The actuator lives in the one-wave option kernels: enabling forces dn_get_kernel_waves(env, 0 / 1) == 1.  dn_step_sampled,
 * dn_step_squashed, dn_mlp_step_sampled and dn_eval_kinematics refuse an env with the actuator enabled (DN_ERR_INVALID_ARGUMENT). */
typedef struct dn_actuator_config {
    int32_t latency[2];   /* latency range [lo, hi], control steps: 0 <= lo <= hi <= DN_MAX_LATENCY */
    float motor_tau[2];   /* motor time constant range [lo, hi], s: finite, 0 <= lo <= hi; [0, 0] = no lag */
    float fill[4];        /* the action a fresh episode's pipeline holds: finite */
    int32_t resample;     /* 1: draw d and a at every episode start; 0: keep dn_set_actuator's */
    int32_t reserved;     /* must be 0 */
} dn_actuator_config;
/* Validates the configuration and enables the feature.  The first call allocates 152 bytes per drone (outside dn_state_bytes) and sets
 * d = 0, a = 0, r = rpm_fill and every history entry to `fill`; a later call changes the configuration (rpm_fill included) and keeps the
 * current values.  Synchronises the device. */
int32_t dn_enable_actuator(dn_env *env, const dn_actuator_config *cfg);
/* Device buffers, copied on `stream`; NULL = leave (set) / skip (get): latency int32[N] (d), coeff float[N] (a), rpm float[N][4] (r),
 * history float[N][8][4] with history[i][j] = the action drone i was commanded j + 1 vector steps ago.  DN_ERR_BAD_STATE if the actuator
 * is not enabled.  dn_set_actuator does not validate the values (the caller's device buffers are not read on the host): d must lie in
 * [0, DN_MAX_LATENCY] (the kernels clamp it), a in [0, 1), every other value finite. */
int32_t dn_set_actuator(dn_env *env, const int32_t *latency, const float *coeff, const float *rpm, const float *history, void *stream);
int32_t dn_get_actuator(dn_env *env, int32_t *latency, float *coeff, float *rpm, float *history, void *stream);
/* 1: actuator enabled, *out = the configuration last given to dn_enable_actuator; 0: not enabled (*out untouched); < 0: error. */
int32_t dn_get_actuator_config(const dn_env *env, dn_actuator_config *out);

/* Per-drone sensor model (sim-to-real): observation latency and a per-episode constant bias (a state-estimator offset) between the state
 * and the observation row the policy sees.  Let o_k be the observation row as produced BEFORE the normaliser -- the observation columns plus
 * the white noise of obs_noise_sigma -- after the episode's k-th control step (k = dn_env_state.steps once the step is over; o_0 is the reset
 * observation, noise stream 5; o_k for k >= 1 the step observation, noise stream 1; the noise stays keyed by the vector step at which the row
 * was MEASURED).  Every drone has an integer latency d in [0, DN_MAX_LATENCY] control steps and a bias row b[13] (float32, observation-column
 * units).  The row handed to the normaliser (normalize_obs), or written to the output without it, after the episode's k-th step is
 *       y_k = float32(o_{k - min(d, k)} + b)          one float32 add per column, unfused
 *   - a fresh episode's pipeline holds that episode's own reset observation: rows of the previous episode never leak into the next one;
 *   - terminal_observation of a step that ends an episode is y_k of that step;
 *   - the reset observation written for a finished drone, and by dn_reset, is float32(o_0 + b_new): the NEW episode's bias, no delay;
 *   - with normalize_obs the running statistics are updated with the delivered rows, once each, exactly where they are updated today;
 *   - nothing feeds back: state, reward, done, truncated, found_targets and the Monitor outputs are bit for bit those of the same env
 *     without the sensor model.
 *   draws:   resample = 1: every episode start (dn_reset and every in-kernel auto-reset) draws from FOUR Philox4x32-10 calls keyed (seed;
 *            global drone id, the vector step the episode starts on, streams 18, 19, 20, 21; streams 0-9 and 11-17 belong to the other
 *            features).  Value c of the call on stream 18 + q is u_m = (r_c + 0.5) / 2^32 in float64 with m = 4 q + c:
 *            b_j = float32(bias_amp[j] (2 u_j - 1)) in float64 for the 13 columns, d = latency lo + floor((hi - lo + 1) u_13) clamped to
 *            hi (u_14, u_15 unused).  Sharding does not move the draws.  resample = 0: d and b are what dn_set_sensor last wrote (0 and 0
 *            after the first enable).
 *   off:     with resample = 1, latency = [0, 0] switches the delay off (no history traffic) and all-zero bias_amp switches the add off
 *            (-0.0f + 0.0f would flip a sign bit); with both off the kernels take the path of an env without the sensor model.  With
 *            resample = 0 the values are the caller's and both are always applied.  The history is maintained only while the delay is on.
 *   units:   bias_amp is in observation-column units: metres / aviary extent for columns 0-2, radians / pi for 3-5, (m/s) / 3 for 6-8,
 *            the unit angular-velocity columns 9-11 as they are, metres / max_target_dist for 12.
 *   memory:  1092 bytes per drone in one allocation of its own: a ring of 16 slots x 64 bytes (the pre-bias row of each of the last 16
 *            vector steps, stored [slot][4 quads of 16 bytes][N], slot = (vector step + offset) mod 16), the bias row (64 bytes, [4][N])
 *            and d.  dn_set_step_count adjusts the offset so that rows already stored keep their meaning; a launch captured in a hipGraph
 *            bakes the offset in, so re-capture after dn_set_step_count.
 * K steps in one launch equal K single steps bit for bit, history included.  A checkpoint is dn_get_state + dn_get_sensor +
 * dn_get_step_count (plus the other features' getters); restore the step counter before dn_set_sensor's history.
 * The sensor model lives in the one-wave option kernels: enabling forces dn_get_kernel_waves(env, 0 / 1) == 1.  dn_step_sampled,
 * dn_step_squashed, dn_mlp_step_sampled and dn_eval_kinematics refuse an env with the sensor enabled (DN_ERR_INVALID_ARGUMENT).
 * Layout: 4-byte members only, no padding: latency at 0, bias_amp at 8, resample at 60, reserved at 64; 68 bytes. */
typedef struct dn_sensor_config {
    int32_t latency[2];   /* latency range [lo, hi], control steps: 0 <= lo <= hi <= DN_MAX_LATENCY */
    float bias_amp[13];   /* bias amplitude per observation column, column units: finite, >= 0; b_j is uniform in [-amp_j, amp_j] */
    int32_t resample;     /* 1: draw d and b at every episode start; 0: keep dn_set_sensor's */
    int32_t reserved;     /* must be 0 */
} dn_sensor_config;
/* Validates the configuration and enables the feature.  The first call allocates 1092 bytes per drone (outside dn_state_bytes) and sets
 * d = 0, b = 0 and an all-zero history; a later call changes the configuration and keeps the current values.  Synchronises the device. */
int32_t dn_enable_sensor(dn_env *env, const dn_sensor_config *cfg);
/* Device buffers, read / written on `stream`; NULL = leave (set) / skip (get): latency int32[N] (d), bias float[N][13] (b),
 * history float[N][9][13] with history[i][j] = the pre-bias row o_{k - j} of drone i, k = its dn_env_state.steps, in this LOGICAL order
 * whatever the device layout (the calls convert, reading the step counter on the device).  Entries with k - j < 0 are ignored on set
 * and unspecified on get.  DN_ERR_BAD_STATE if the sensor is not enabled.  dn_set_sensor does not validate the values (the caller's device
 * buffers are not read on the host): d must lie in [0, DN_MAX_LATENCY] (the kernels clamp it), every other value finite. */
int32_t dn_set_sensor(dn_env *env, const int32_t *latency, const float *bias, const float *history, void *stream);
int32_t dn_get_sensor(dn_env *env, int32_t *latency, float *bias, float *history, void *stream);
/* 1: sensor enabled, *out = the configuration last given to dn_enable_sensor; 0: not enabled (*out untouched); < 0: error. */
int32_t dn_get_sensor_config(const dn_env *env, dn_sensor_config *out);

/* Privileged observations (asymmetric actor-critic, teacher-student): the ground truth the four models above hide from the policy, written
 * per drone and step by the step kernels themselves -- inside a fused launch too, where episodes restart and parameters are redrawn.  One
 * row is DN_PRIV_DIM = 52 float32 (208 bytes), thirteen 16-byte quads; a group of columns is written when its bit is in `groups`:
 *   columns  0..12  DN_PRIV_OBS   the TRUE observation: the observation columns of the state this step leaves, before obs_noise_sigma's
 *                                 noise, before the sensor model and before the normaliser; 13..15 are 0
 *           16..19  DN_PRIV_DYN   s_m, s_I, s_kf, s_km                                      (dn_get_dynamics)
 *           20..22  DN_PRIV_WIND  wbar, 23 is 0;  24..26: g, 27 is 0                        (dn_get_wind)
 *           28..31  DN_PRIV_ACT   the effective rotor speeds r                              (dn_get_actuator rpm)
 *           32, 33  DN_PRIV_ACT   the actuator's latency d and coefficient a; d as a float32 number
 *               34  DN_PRIV_SENS  the sensor's latency d, as a float32 number
 *               35  DN_PRIV_OBS   the episode step counter (dn_env_state.steps), as a float32 number
 *           36..48  DN_PRIV_SENS  the sensor bias b[13]; 49..51 are 0
 *   step row (`rows`): where the episode goes on, the true observation of the new state; where it ended, the new episode's noise-free
 *     reset observation -- as `obs` is the reset row there.  Every parameter column holds what the model's dn_get_* would return right
 *     after this step: for a drone whose episode restarted, the NEW episode's draws, r = rpm_fill and step counter 0.  The latency
 *     columns carry the values the kernels use, i.e. clamped to [0, DN_MAX_LATENCY].
 *   terminal row (`terminal_rows`, optional): written only where done, like terminal_obs.  Columns 0..12 are the true observation of the
 *     terminal state; every parameter column holds the value at the ENTRY of the terminal step (what dn_get_* returned before it: the
 *     finished episode's body, wind, actuator and sensor); column 35 is the finished episode's length.
 *   a model that is not enabled is written as its neutral value: scales 1, wind 0, d 0, a 0, r 0, bias 0.
 *   a group that is not in `groups` is not written at all: the caller's bytes stay as they are (a launch-uniform branch per group: a
 *     caller that wants the 64-byte true observation alone does not pay for 208 bytes).
 *   nothing feeds back: every other output and every byte of state is that of the same env without the feature.
 * The rows are a persistent binding (dn_bind_privileged), not an argument of dn_step: the entry points keep their signatures and a
 * captured hipGraph keeps writing into the bound buffers.  Every launch rewrites all selected columns of every step row it covers; K steps
 * in one launch equal K single steps bit for bit.  dn_reset writes the step row of the fresh episodes into step slot 0.
 * The rows are written by one more family of the one-wave option kernels, which carries the four models (on or off): enabling forces
 * dn_get_kernel_waves(env, 0 / 1) == 1.  dn_step_sampled, dn_step_squashed, dn_mlp_step_sampled and dn_eval_kinematics refuse an env with
 * the feature enabled (DN_ERR_INVALID_ARGUMENT).
 * Layout: groups at 0, reserved at 4; 8 bytes. */
#define DN_PRIV_DIM 52
#define DN_PRIV_OBS 1
#define DN_PRIV_DYN 2
#define DN_PRIV_WIND 4
#define DN_PRIV_ACT 8
#define DN_PRIV_SENS 16
#define DN_PRIV_ALL 31
typedef struct dn_privileged_config {
    int32_t groups;       /* mask of DN_PRIV_*: non-zero, known bits only */
    int32_t reserved;     /* must be 0 */
} dn_privileged_config;
/* Validates the mask and enables the feature; a later call changes the mask and keeps the binding.  Allocates nothing. */
int32_t dn_enable_privileged(dn_env *env, const dn_privileged_config *cfg);
/* 1: enabled, *out = the configuration last given to dn_enable_privileged; 0: not enabled (*out untouched); < 0: error. */
int32_t dn_get_privileged_config(const dn_env *env, dn_privileged_config *out);
/* Binds the caller's device buffers, 16-byte aligned: rows float[capacity_steps][N][DN_PRIV_DIM], step-major like every dn_step_many
 * buffer, and terminal_rows of the same shape or NULL.  dn_step and dn_reset write step slot 0; dn_step_many with k > capacity_steps
 * fails with DN_ERR_INVALID_ARGUMENT.  rows = NULL unbinds (terminal_rows must be NULL too, capacity_steps is ignored): an env that is
 * enabled but unbound writes nothing.  DN_ERR_BAD_STATE if the feature is not enabled.  The buffers must outlive the binding; a launch
 * captured in a hipGraph bakes the pointers in. */
int32_t dn_bind_privileged(dn_env *env, float *rows, float *terminal_rows, int64_t capacity_steps);

/* Goal observations: where the drone is supposed to fly, as the policy may see it.  The 13 observation columns carry no direction to the
 * target; with this feature the step kernels write, per drone and step -- inside a fused launch too --, one row of DN_GOAL_DIM = 8 float32
 * (two 16-byte quads).  The row is a pure function of
 *   y   the observation row as delivered to the normaliser: after obs_noise_sigma's noise and after the sensor model's latency and bias,
 *       before the normaliser (the row `obs` holds when normalize_obs is off),
 *   i   the target index the row is written with, and
 *   the waypoints wp[0..W-1], dim_high = (x_high, y_high, z_high) of the aviary box and 1 / max_target_dist (the scale of column 12):
 *     p_hat = y[0:3] * dim_high                                 the position the policy is shown: noise, latency and bias are in it
 *     e     = (wp[i] - p_hat) / max_target_dist                 to the current target
 *     n     = (wp[i+1] - wp[i]) / max_target_dist               the segment after it; (0, 0, 0) where i + 1 == W
 *     DN_GOAL_FRAME_WORLD:  row = [ e_x e_y e_z float(i) | n_x n_y n_z (i + 1 < W ? 1 : 0) ]
 *     DN_GOAL_FRAME_BODY:   e and n multiplied by R^T, R = Rz(yaw) Ry(pitch) Rx(roll), (roll, pitch, yaw) = pi * y[3:6]: the
 *                           convention of the observation's own Euler columns, applied to the DELIVERED columns (float32 sinf / cosf)
 *   The row is built from the delivered position on purpose: from the true position, wp - e would hand the policy what the sensor model
 *   hides.  The index is the true one (a lap counter knows which gate is next).
 *   step row (`rows`): where the episode goes on, i = the waypoint index the step leaves (dn_env_state.idx after it) and y = the
 *     step's row; where it ended, i = 0 and y = the new episode's reset row -- as `obs` is the reset row there.
 *   terminal row (`terminal_rows`, optional): written only where done, like terminal_obs; y = the terminal row (terminal_obs before the
 *     normaliser), i = min(index the episode ended with, W - 1) -- a completed track ends with index W.
 *   The rows are neither normalised nor clipped, and nothing feeds back: every other output and every byte of state is that of the same
 *   env without the feature.
 * The rows are a persistent binding (dn_bind_goal) like the privileged rows: the entry points keep their signatures and a captured
 * hipGraph keeps writing.  K steps in one launch equal K single steps bit for bit.  dn_reset writes the fresh episodes' rows (i = 0) into
 * step slot 0.  The rows are written by one more family of the one-wave option kernels, which carries the four models and the privileged
 * rows (on or off): enabling forces dn_get_kernel_waves(env, 0 / 1) == 1.  dn_step_sampled, dn_step_squashed, dn_mlp_step_sampled and
 * dn_eval_kinematics refuse an env with the feature enabled (DN_ERR_INVALID_ARGUMENT).
 * Layout: frame at 0, reserved at 4; 8 bytes. */
#define DN_GOAL_DIM 8
#define DN_GOAL_FRAME_WORLD 0
#define DN_GOAL_FRAME_BODY 1
typedef struct dn_goal_config {
    int32_t frame;        /* DN_GOAL_FRAME_WORLD or DN_GOAL_FRAME_BODY */
    int32_t reserved;     /* must be 0 */
} dn_goal_config;
/* Validates the frame and enables the feature; a later call changes the frame and keeps the binding.  Allocates nothing. */
int32_t dn_enable_goal(dn_env *env, const dn_goal_config *cfg);
/* 1: enabled, *out = the configuration last given to dn_enable_goal; 0: not enabled (*out untouched); < 0: error. */
int32_t dn_get_goal_config(const dn_env *env, dn_goal_config *out);
/* Binds the caller's device buffers, 16-byte aligned: rows float[capacity_steps][N][DN_GOAL_DIM], step-major like every dn_step_many
 * buffer, and terminal_rows of the same shape or NULL.  dn_step and dn_reset write step slot 0; dn_step_many with k > capacity_steps
 * fails with DN_ERR_INVALID_ARGUMENT.  rows = NULL unbinds (terminal_rows must be NULL too, capacity_steps is ignored): an env that is
 * enabled but unbound writes nothing and launches the kernels it would launch without the feature.  DN_ERR_BAD_STATE if the feature is
 * not enabled.  The buffers must outlive the binding; a launch captured in a hipGraph bakes the pointers in. */
int32_t dn_bind_goal(dn_env *env, float *rows, float *terminal_rows, int64_t capacity_steps);

/* Track bank: each drone of a fleet flies one of several tracks.  A bank is T tracks, 1 <= T <= DN_MAX_TRACKS; track t has W_t >= 1
 * waypoints, given one track after the other in `waypoints`; the sum of W_t is at most DN_MAX_WAYPOINTS (the 64-entry corridor table the
 * kernels stage into LDS holds the whole bank, so LDS use and occupancy of no kernel change).  All tracks share the env's spawn,
 * aviary_dim, threshold and max_steps.  Track 0 must equal the track of dn_config -- the same count and bit-equal waypoints -- so that
 * enabling the bank on a flying fleet changes nothing for any drone.
 *   Definition: the table rows of track t are the rows a dn_config with that one track gets (including row 0 of each track, whose base
 *   point is the spawn); the library builds both with the same function.  For a drone on track t everything the step does with waypoints
 *   uses t's rows and W_t: the gate row, the corridor of the next segment, the last gate (completion and its +200), observation column
 *   12, the orientation reward, the fresh episode's distance to waypoint 0, the goal rows (wp[i], wp[i+1], i + 1 < W_t) and the terminal
 *   goal index min(idx, W_t - 1).  The step of the drone's own track is unchanged in every bit: a bank drone on track t equals the same
 *   drone (same num_envs, seed, env_id_offset, actions) of an env created with track t alone.  idx in dn_env_state and found_targets stay
 *   the index within the drone's track.
 *   Per drone: track (the track of its current episode) and finished (the track of its most recently ended episode, -1 before the
 *   first), int32, in one allocation of the model's own outside dn_state_bytes.
 *   Draw (resample = 1): every episode start -- dn_reset and every in-kernel auto-reset -- draws the track with ONE Philox4x32-10 call
 *   keyed like the other models: (seed; global drone id, the vector step the episode starts on, stream 22).
 *     u = (r_0 + 0.5) / 2^32 in float64;  cdf_k = S_k / S_{T-1}, S = the float64 partial sums of the float32 weights in index order
 *     (formed on the host);  t = the number of k in 0..T-2 with u >= cdf_k.  A zero weight is never drawn.
 *   The new track is the one the reset row, the reset goal row and the fresh d / d_prev are measured on; the terminal observation, the
 *   terminal goal row, the reward, found_targets and `finished` belong to the track the step was entered with.
 *   (As in every auto-reset, the fresh distance is measured from the position the reference keeps in _current_position, not from the
 *   spawn, and the reset row's column 12 shows the ended episode's distance; likewise the first dn_reset after dn_set_tracks shows the
 *   distance the state held.)
 *   Checkpoint of a bank fleet: dn_get_state + dn_get_tracks (+ the models' getters); restore as dn_set_tracks, THEN dn_set_state, which
 *   holds every idx to the waypoint count of the track the drone is on at that moment (DN_ERR_INVALID_ARGUMENT beyond it).  `finished`
 *   and the counters are reporting state and are not restored.
 *   resample = 0: a drone keeps its track across episode starts (dn_set_tracks writes it).
 *   Per-track counters, int64 [T][5], added at episode ends under the entry track, inside fused launches too:
 *   episodes, completed, truncated, sum of found_targets at episode end, sum of episode lengths.
 * The bank rides in the goal family of the one-wave option kernels (with the goal rows unbound that family writes none): enabling forces
 * dn_get_kernel_waves(env, 0 / 1) == 1, and dn_step_sampled, dn_step_squashed, dn_mlp_step_sampled and dn_eval_kinematics refuse the env.
 * Layout: num_tracks at 0, num_waypoints at 4, waypoints at 264 (8-byte aligned), weight at 1800, resample at 2056, reserved at 2060;
 * 2064 bytes. */
#define DN_MAX_TRACKS 64
typedef struct dn_track_bank_config {
    int32_t num_tracks;                         /* T, 1..DN_MAX_TRACKS */
    int32_t num_waypoints[DN_MAX_TRACKS];       /* W_t, each >= 1, sum <= DN_MAX_WAYPOINTS */
    double  waypoints[DN_MAX_WAYPOINTS * 3];    /* the tracks' waypoints one track after the other, row-major xyz */
    float   weight[DN_MAX_TRACKS];              /* draw weights, finite and >= 0, not all zero (resample = 1) */
    int32_t resample, reserved;                 /* resample: 0 or 1; reserved: must be 0 */
} dn_track_bank_config;
/* The first call allocates and sets track = 0, finished = -1 and zero counters; a later call with the same geometry (counts and
 * waypoints) changes weights and resample and keeps the assignment; a later call with another geometry is refused.
 * DN_ERR_INVALID_ARGUMENT: a circle env; random_spawn (the spawn draw reads track lines); counts out of range or a sum over
 * DN_MAX_WAYPOINTS; non-finite waypoints; negative or non-finite weights, or all weights zero; track 0 different from the config's;
 * reserved != 0.  An env created with DN_GROUND_CONTACT_AUTO resolves the term again over every track of the bank (on if any track
 * needs it); dn_get_config returns the result. */
int32_t dn_enable_tracks(dn_env *env, const dn_track_bank_config *cfg);
/* track: int32[N] on the device.  Writes the assignment and does not touch the state: reset afterwards.  Values are not validated (the
 * kernels hold an index to the bank).  DN_ERR_BAD_STATE before dn_enable_tracks. */
int32_t dn_set_tracks(dn_env *env, const int32_t *track, void *stream);
/* track, finished: int32[N] on the device; either may be NULL.  DN_ERR_BAD_STATE before dn_enable_tracks. */
int32_t dn_get_tracks(dn_env *env, int32_t *track, int32_t *finished, void *stream);
/* out: int64[T][5] on the host (synchronises the device); reset != 0 zeroes the counters afterwards.  DN_ERR_BAD_STATE before
 * dn_enable_tracks. */
int32_t dn_get_track_stats(dn_env *env, int64_t *out, int32_t reset);
/* *out = the configuration last given to dn_enable_tracks.  DN_ERR_BAD_STATE before dn_enable_tracks (*out untouched). */
int32_t dn_get_track_bank_config(const dn_env *env, dn_track_bank_config *out);

/* Observation and action history rows, stacked on the device (what SB3's VecFrameStack does for the reference's VecEnv, plus the policy's
 * own previous actions): under command latency, motor lag and observation latency the 13 columns of one instant are no Markov state.  One
 * row of W float32 per drone and step, W = 4 ceil((13 F + 4 A + E) / 4) <= 64 (the widest row dn_mlp_forward takes):
 *   columns [0, 13 F)              F observation frames, oldest first, newest last (SB3's order)
 *   columns [13 F, 13 F + 4 A)     A action frames, oldest first; the newest is the action of the step that produced the newest observation
 *   the next E columns             the `extra` columns of the step, copied through (the 8 goal columns, for instance)
 *   the rest                       zero
 * Step rule, per drone, with P the row before the step, o the step's `obs` row (already the reset row where done), a its action, d its done
 * flag, tau its `terminal_obs` row, x / xtau its extras, and shift(P) = P without its oldest observation frame and its oldest action frame:
 *   d = 0:  row = shift(P) with o and a as the newest frames, then x
 *   d = 1:  terminal row = shift(P) with tau and a as the newest frames, then xtau -- written only where done, like terminal_obs, and only
 *           when terminal_rows is given;  row = zero frames with o as the newest observation frame, zero action frames, then x
 *           (VecFrameStack at an episode boundary).
 * Every word is a copy of a float32 word the caller holds (NaN payloads and -0.0 included) or zero; nothing is normalised or rescaled, so
 * with normalize_obs a frame carries the statistics of its own step.
 * A kernel of its own, run after the step, on buffers every step kernel already writes: no dn_env, no state in the library, no model level,
 * dn_get_kernel_waves unchanged.  All buffers are step-major like dn_step_many's:
 *   prev           const float[N][W]     the row before step 0; NULL = every episode starts (all zero).  May alias any step slot of `rows`
 *                                        (the caller's current rows, updated in place): a drone's previous row is read before any of its
 *                                        rows is written
 *   obs            const float[k][N][13]
 *   actions        const float[k][N][4]  NULL = zero action frames (the reset call); required when `done` is given
 *   done           const uint8[k][N]     NULL = no episode ended
 *   terminal_obs   const float[k][N][13] read where done; required when terminal_rows is given
 *   extra, terminal_extra  const float[k][N][E] or NULL (then zero)
 *   rows           float[k][N][W];  terminal_rows  float[k][N][W] or NULL
 * prev, rows and terminal_rows 16-byte aligned; for k > 1, N a multiple of 4 as for dn_step_many.  A reset is k = 1 with
 * prev = actions = done = NULL.  Validates before the first device call; enqueues one launch on `stream` (capturable).
 * Layout of dn_history_config: frames at 0, actions at 4, extra_dim at 8, reserved at 12; 16 bytes. */
typedef struct dn_history_config {
    int32_t frames;       /* F, 1..4 */
    int32_t actions;      /* A, 0..4 */
    int32_t extra_dim;    /* E >= 0 */
    int32_t reserved;     /* must be 0 */
} dn_history_config;
/* W, or a negative dn_status (DN_ERR_INVALID_ARGUMENT: NULL, a range out of bounds, W > 64, reserved != 0). */
int32_t dn_history_width(const dn_history_config *cfg);
int32_t dn_stack_history(const dn_history_config *cfg, int64_t k, int64_t n, const float *prev, const float *obs, const float *actions,
                         const uint8_t *done, const float *terminal_obs, const float *extra, const float *terminal_extra, float *rows,
                         float *terminal_rows, int32_t device_id, void *stream);

/* A fleet-wide running normaliser for policy and critic input rows (what SB3's VecNormalize is to the reference's VecEnv [from recall]):
 * the privileged rows, cat(obs, goal) and the history rows reach the networks raw otherwise -- rotor speeds of order 1e4 beside columns
 * of order 1.  One RunningMeanStd per row kind over the WHOLE fleet, the arithmetic of Sol/Model/Environments/normalize.py:10-47
 * (RunningMeanStd, update_mean_var_count_from_moments) with the N rows of a step as the batch (the per-drone NormalizeObservation calls
 * it with a batch of one).  State, float64 on the device, dn_rownorm_state_doubles(width) = 1 + 2 width doubles:
 *   stats[0] = count (starts at 1e-4), stats[1 .. width] = mean (0), stats[1 + width .. 2 width] = var (1) -- the variance itself, not
 *   a second moment: a copy of the state is the state.
 * Update with a batch of n rows, per column, bm / bv the batch mean and population variance:
 *   delta = bm - mean; tot = count + n; mean += delta n / tot; var = (var count + bv n + delta^2 count n / tot) / tot; count = tot
 * Output: out = clip((x - mean) / sqrt(var + epsilon), -clip, +clip) as float32; a NaN stays a NaN in its own cell (np.clip), clip = +inf
 * is no clip.  x - mean is formed in float64 and rounded to float32, then multiplied by the float32 reciprocal square root of
 * float32(var + epsilon): within 3 float32 ulp of the float64 evaluation, the output stage of the step kernels' normaliser.
 * Order within a step, SB3's VecNormalize.step_wait [from recall]: update with the step's N rows (reset rows included), then normalise
 * those rows with the updated statistics; terminal rows are normalised with update = 0 and do not move the statistics.
 *   update = 1   k times in sequence: step t's rows are normalised with the statistics after steps 0 .. t.  out may be NULL (update only).
 *   update = 0   all k n rows are normalised with `stats` as they are; `stats` is not written.  out is required.
 *   rows         const float[k][n][width], dense and step-major like dn_step_many's buffers, 4-byte aligned
 *   out          float[k][n][width]: rows itself (in place) or apart from it; 16-byte loads and stores when width % 4 == 0 and both
 *                pointers are 16-byte aligned, 4-byte ones otherwise
 *   scratch      the caller's device memory, 8-byte aligned, at least dn_rownorm_scratch_bytes(k, n, width): the per-block moments and
 *                the per-step snapshots.  The library allocates nothing and keeps nothing between calls.
 * Bit-reproducible: the batch moments are formed in float64 per block of 1024 consecutive rows (a constant) in a shifted form and merged
 * in ascending block order; no atomics, no workgroup waits for another: three ordinary launches on `stream` (one with update = 0),
 * capturable.  K steps in one call equal K calls of one step bit for bit.  Validates before the first device call.
 * Each rank keeps its own statistics (no collective).  Layout of dn_rownorm_config: width at 0, clip at 4, epsilon at 8; 16 bytes. */
typedef struct dn_rownorm_config {
    int32_t width;        /* W, 1..64 */
    float clip;           /* > 0; +inf = no clip.  VecNormalize's clip_obs is 10 */
    double epsilon;       /* >= 0; the reference's is 1e-8 */
} dn_rownorm_config;
/* normalize.py:10-47.  1 + 2 width; a negative dn_status for a width outside 1..64. */
int64_t dn_rownorm_state_doubles(int32_t width);
/* normalize.py:10-47.  Bytes of scratch for k steps of n rows; a negative dn_status for a width outside 1..64 or k, n < 1. */
int64_t dn_rownorm_scratch_bytes(int64_t k, int64_t n, int32_t width);
/* normalize.py:10-47 (RunningMeanStd.__init__, lines 13-17).  stats <- 1e-4, 0, 1, on `stream`. */
int32_t dn_rownorm_init(const dn_rownorm_config *cfg, double *stats, int32_t device_id, void *stream);
/* normalize.py:10-47 (update and update_mean_var_count_from_moments, lines 19-47) and the normalised rows. */
int32_t dn_rownorm(const dn_rownorm_config *cfg, double *stats, int64_t k, int64_t n, const float *rows, float *out, int32_t update,
                   void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

/* A fleet-wide running return normaliser for rewards: the reward half of SB3's VecNormalize (norm_reward=True) [from recall].  One
 * discounted return per drone and ONE RunningMeanStd of those returns over the WHOLE fleet -- the arithmetic of
 * Sol/Model/Environments/normalize.py:10-47 (RunningMeanStd, update_mean_var_count_from_moments) with the N returns of a step as the
 * batch -- and the reward divided by the returns' standard deviation.  (The reference's NormalizeReward, dn_config.norm_rew, keeps one
 * statistic per drone, a batch of one, inside the one-wave option kernel.)  State, the caller's, float64 on the device:
 *   stats[3]     count (starts at 1e-4), mean (0), var (1) -- the variance itself, not a second moment: a copy of the state is the state
 *   returns[n]   the discounted return of every drone's running episode, 0 at the start
 * Per vector step, r[n] the float32 rewards and d[n] the done flags (truncations included), in this order:
 *   1. returns = returns * gamma + r      the reward widened to float64, product and sum unfused as numpy evaluates them: bit-exact
 *   2. the update of normalize.py:32-47 with the n returns as the batch, bm / bv their np.mean / np.var:
 *        delta = bm - mean; tot = count + n; mean += delta n / tot; var = (var count + bv n + delta^2 count n / tot) / tot; count = tot
 *   3. out = clip(r / sqrt(var + epsilon), -clip, +clip) as float32, with the updated variance.  No mean is subtracted.  Formed as
 *      r times the float32 reciprocal square root of float32(var + epsilon), the output stage of dn_rownorm: within 3 float32 ulp of the
 *      float64 evaluation.  A NaN stays a NaN in its own cell (np.clip); clip = +inf is no clip.
 *   4. returns = 0 where d
 * A NaN reward poisons its drone's return and the statistics, as it does in the reference.
 *   update = 1   k times in sequence: step t is scaled with the statistics after steps 0 .. t.  done, returns and scratch are required;
 *                out may be NULL (update only).
 *   update = 0   step 3 alone on `stats` as they are (normalize_reward for evaluation): reads no done and no returns, writes neither stats
 *                nor returns; out is required; done, returns and scratch are ignored.
 *   rewards      const float[k][n], step-major like dn_step_many's buffers, 4-byte aligned
 *   done         const uint8_t[k][n]
 *   out          float[k][n]: rewards itself (in place) or apart from it; 16-byte loads and stores when both pointers are 16-byte aligned
 *                and n is a multiple of 4, 4-byte ones otherwise, with the same bits
 *   scratch      the caller's device memory, 8-byte aligned, at least dn_retnorm_scratch_bytes(k, n): the per-block moments and the
 *                per-step snapshots.  The library allocates nothing and keeps nothing between calls.
 * Bit-reproducible: the batch moments are formed in float64 per block of 1024 consecutive drones (a constant) in a shifted form and merged
 * in ascending block order; no atomics, no workgroup waits for another: three ordinary launches on `stream` (one with update = 0),
 * capturable.  K steps in one call equal K calls of one step bit for bit, in out, stats and returns.  Validates before the first device
 * call.  Each rank keeps its own statistics (no collective).
 * Layout of dn_retnorm_config: gamma at 0, epsilon at 8, clip at 16, reserved at 20; 24 bytes. */
typedef struct dn_retnorm_config {
    double gamma;         /* in [0, 1]; VecNormalize's is 0.99 */
    double epsilon;       /* >= 0; 1e-8 */
    float clip;           /* > 0; +inf = no clip.  VecNormalize's clip_reward is 10 */
    int32_t reserved;     /* 0 */
} dn_retnorm_config;
/* normalize.py:10-47.  Bytes of scratch for k steps of n drones; a negative dn_status for k or n < 1. */
int64_t dn_retnorm_scratch_bytes(int64_t k, int64_t n);
/* normalize.py:10-47 (RunningMeanStd.__init__, lines 13-17).  stats <- 1e-4, 0, 1 and returns[n] <- 0, on `stream`.  Either may be NULL
 * and is then left alone: stats = NULL resets the returns only, which is what VecNormalize.reset() does [from recall]. */
int32_t dn_retnorm_init(double *stats, double *returns, int64_t n, int32_t device_id, void *stream);
/* normalize.py:10-47 (update and update_mean_var_count_from_moments, lines 19-47) on the discounted returns, and the scaled rewards. */
int32_t dn_retnorm(const dn_retnorm_config *cfg, double *stats, double *returns, int64_t k, int64_t n, const float *rewards,
                   const uint8_t *done, float *out, int32_t update, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

/* PPO minibatches on the device: the reading half of SB3's RolloutBuffer, get(batch_size) [from recall] -- swap-and-flatten, one random
 * permutation per epoch, the gathered minibatches, and the per-minibatch advantage normalisation of PPO.train [from recall] -- on the
 * step-major [n_steps][n_envs] buffers that dn_step_many, dn_gae and the collectors leave, without a flattened copy and with pinned
 * bits.  Env-free; the learner itself stays the caller's.
 * Sample numbering: M = n_steps n_envs <= 2^31 - 1; sample s is drone s / n_steps at step s % n_steps, SB3's swap_and_flatten order
 *   [from recall] (a caller who passes SB3's own np.random.permutation as `indices` gets SB3's minibatches); its source row is
 *   (s % n_steps) n_envs + s / n_steps.
 * Sample selection: output row j of the call, 0 <= j < batch, is sample indices[j] when `indices` (device int64[batch]) is not NULL; a
 *   value outside [0, M) is clamped into it, so no read ever leaves the source.  With NULL indices row j is sample pi(start + j), pi the
 *   keyed bijection of [0, M) under (seed, epoch + (epoch_offset ? *epoch_offset : 0)), the sum mod 2^64.
 *   pi: b = max(1, bit_length(M - 1)), h = max(1, (b + 1) / 2), mask = 2^h - 1; six round keys k_r = the high 32 bits of six successive
 *   splitmix64 outputs from the state seed ^ (epoch * 0xD1342543DE82EF95); one pass over v: L = (v >> h) & mask, R = v & mask, six times
 *   F = fmix32(R + k_r) >> (32 - h), (L, R) = (R, (L ^ F) & mask) (fmix32: murmur3's finaliser), v' = L << h | R; pi(i) repeats the pass
 *   from v = i until v' < M.  Evaluated per element: no permutation array, no sort (csrc/dn_permute.h, host and device).
 *   epoch_offset   device int64[1] or NULL: lets a captured graph reshuffle on every replay, the way the environment's device-side step
 *                  counter keeps the noise moving
 *   indices_out    device int64[batch] or NULL: receives the samples taken
 *   start          0 <= start and start + batch <= M; with `indices`, start must be 0
 * Copies: every field's rows are copied bit for bit (32-bit words, float32 or int32), dst row j from the source row of sample j.
 * Advantage normalisation: the `normalize` field is then out = (a - mean) / (std + epsilon), mean over the batch gathered values and std
 *   their unbiased standard deviation (torch.std: divide by batch - 1); skipped when batch == 1, as SB3 skips it.  Moments, the
 *   subtraction and a true division are float64, rounded once to float32.  A NaN advantage makes the minibatch's output NaN, as in torch.
 * Bit-reproducible: the moments are float64 per block of 1024 consecutive output rows (the normalisers' constant) in dn_retnorm's shifted
 *   form (shift = the block's first gathered value; lanes by a fixed tree, waves ascending), the blocks merged in ascending order by the
 *   normalisers' merge.  The order of every float64 operation is a function of `batch` alone.
 *   scratch        the caller's device memory, 8-byte aligned, at least dn_minibatch_scratch_bytes(batch): the per-block pairs, the mean
 *                  and the denominator.  The library allocates nothing and keeps nothing between calls.
 * At most three ordinary launches on `stream`: gather + block moments, a one-wave merge, the division; one launch when no field is
 * normalised or batch == 1.  No workgroup waits for another, no atomics, capturable.  Validates before the first device call:
 * DN_ERR_INVALID_ARGUMENT with a dn_last_error text.
 * Layout of dn_minibatch_field: src at 0, dst at 8, width at 16, normalize at 20; 24 bytes.
 * Layout of dn_minibatch_config: seed at 0, epoch at 8, epsilon at 16, num_fields at 24, reserved at 28; 32 bytes. */
#define DN_MINIBATCH_MAX_FIELDS 8
typedef struct dn_minibatch_field {
    const void *src;      /* device, 32-bit words [n_steps][n_envs][width], dense, step-major (float32 or int32: copied bit for bit) */
    void *dst;            /* device, [batch][width], dense; never src */
    int32_t width;        /* 1..64 */
    int32_t normalize;    /* 1 on at most one field, which must be width 1 and float32: the advantages */
} dn_minibatch_field;
typedef struct dn_minibatch_config {
    uint64_t seed;
    uint64_t epoch;
    double epsilon;       /* >= 0; SB3's 1e-8 */
    int32_t num_fields;   /* 1..8 */
    int32_t reserved;     /* 0 */
} dn_minibatch_config;
/* Bytes of scratch for a minibatch of `batch` rows; a negative dn_status for batch < 1. */
int64_t dn_minibatch_scratch_bytes(int64_t batch);
/* Host only: needs no device and makes no HIP call.  out[0 .. count) <- pi(start) .. pi(start + count - 1) of [0, m) under (seed, epoch),
 * in HOST memory, by the code the kernel runs.  1 <= m <= 2^31 - 1, 0 <= start, 0 <= count, start + count <= m. */
int32_t dn_minibatch_permutation(uint64_t seed, uint64_t epoch, int64_t m, int64_t start, int64_t count, int64_t *out);
/* SB3 RolloutBuffer.get [from recall] for one minibatch, and PPO.train's advantage normalisation [from recall]. */
int32_t dn_minibatch(const dn_minibatch_config *cfg, const dn_minibatch_field *fields, int64_t n_steps, int64_t n_envs, int64_t start,
                     int64_t batch, const int64_t *indices, const int64_t *epoch_offset, int64_t *indices_out, void *scratch,
                     int64_t scratch_bytes, int32_t device_id, void *stream);

/* The PPO loss head on the device: SB3's PPO.train body [from recall] between the three head outputs of a diagonal-Gaussian actor-critic
 * (action_net, log_std, value_net of MlpActorCritic) and the scalar loss -- the clipped surrogate, the value loss, the entropy term, SB3's
 * logged statistics, and the gradients of the loss with respect to the three head outputs.  Env-free; the networks' own forward and
 * backward, the optimiser and the learner loop stay the caller's.
 * Inputs (device float32, dense), row b < batch, column j < A = act_dim: mean[batch][A], log_std[A], value[batch]; of the minibatch
 *   actions[batch][A], old_log_prob[batch], advantages[batch], returns[batch], and old_values[batch], which is read when the value clip
 *   is on and must be NULL when it is off.
 * Scalars: clip_range c > 0, finite; clip_range_vf cv: > 0 and finite = clip the value step, any finite value <= 0 = no value clip (NaN and
 *   the infinities are refused); ent_coef and vf_coef >= 0, finite.  They are host arguments: a captured graph keeps the values it was captured with.
 * Arithmetic: every input is widened to float64 once; everything below is float64.  ratio = exp(lr) is the float64 library function;
 *   inv_j = exp(-log_std_j) is rounded correctly (csrc/dn_exp_cr.h): every bit of logp hangs on it, and in the first epoch, lr ~ 1e-7,
 *   approx_kl's term (ratio - 1) - lr ~ lr^2 / 2 hangs on the last bit of lr.
 *   inv_j = exp(-log_std_j)                       z_bj = (actions_bj - mean_bj) inv_j
 *   logp_b = sum_j (-0.5 z_bj^2 - log_std_j - 0.5 log(2 pi)), j ascending
 *   lr_b = logp_b - old_log_prob_b                ratio_b = exp(lr_b)
 *   p1 = adv ratio, p2 = adv clamp(ratio, 1 - c, 1 + c)
 *   policy_loss = -mean_b min(p1, p2)             clip_fraction = mean_b [|ratio - 1| > c]        approx_kl = mean_b ((ratio - 1) - lr)
 *   vpred_b = value_b, or with the value clip old_b + clamp(value_b - old_b, -cv, cv)             value_loss = mean_b (returns_b - vpred_b)^2
 *   entropy_loss = -sum_j (0.5 + 0.5 log(2 pi) + log_std_j)
 *   loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
 * Gradients of loss (what torch's autograd gives for the composition above):
 *   w_b = 1 if p1 < p2, 0 if p1 > p2; on p1 == p2: 1 if 1 - c <= ratio <= 1 + c, else 0.5 (torch.min splits a tie, torch.clamp passes its
 *   bounds);  g_b = -adv_b w_b ratio_b / batch;  d_mean_bj = g_b z_bj inv_j;  d_log_std_j = sum_b g_b (z_bj^2 - 1) - ent_coef;
 *   d_value_b = vf_coef (-2) (returns_b - vpred_b) [no value clip, or -cv <= value_b - old_b <= cv] / batch.
 *   NaN and infinity are not special-cased: a NaN advantage gives NaN in loss and policy_loss, a NaN d_log_std, and NaN in d_mean of
 *   its own row only.
 * Outputs, each rounded once: float32 d_mean[batch][A], d_log_std[A], d_value[batch], log_prob_out[batch] (logp; may be NULL), loss[1];
 *   float64 stats[8] = loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, 0, 0.  No output may overlap an input.
 * Bit-reproducible: the means are float64 sums per block of 1024 consecutive rows (the normalisers' constant; lanes by a fixed tree,
 *   waves ascending), the blocks added in ascending order.  The order of every float64 operation is a function of (batch, act_dim) alone.
 *   scratch        the caller's device memory, 8-byte aligned, at least dn_ppo_loss_scratch_bytes(batch, act_dim): the block sums.  The
 *                  library allocates nothing and keeps nothing between calls.
 * Two ordinary launches on `stream`: rows + block sums, a one-wave merge.  No workgroup waits for another, no atomics, capturable.
 * Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a dn_last_error text that names the argument.
 * Layout of dn_ppo_loss_config: clip_range at 0, clip_range_vf at 8, ent_coef at 16, vf_coef at 24, act_dim at 32, reserved at 36;
 * 40 bytes. */
#define DN_PPO_MAX_ACT 8
typedef struct dn_ppo_loss_config {
    double clip_range;      /* > 0, finite; SB3's 0.2 */
    double clip_range_vf;   /* > 0: clip the value step; <= 0: no value clip (SB3's None) */
    double ent_coef;        /* >= 0, finite */
    double vf_coef;         /* >= 0, finite */
    int32_t act_dim;        /* 1..8 */
    int32_t reserved;       /* 0 */
} dn_ppo_loss_config;
/* Bytes of scratch for `batch` rows of `act_dim` columns; a negative dn_status for batch < 1 or beyond 2^31 - 1, or act_dim outside 1..8. */
int64_t dn_ppo_loss_scratch_bytes(int64_t batch, int32_t act_dim);
/* SB3 PPO.train [from recall]: the loss of one minibatch, its statistics and its gradients with respect to the head outputs. */
int32_t dn_ppo_loss(const dn_ppo_loss_config *cfg, int64_t batch, const float *mean, const float *log_std, const float *value,
                    const float *actions, const float *old_log_prob, const float *advantages, const float *returns,
                    const float *old_values, float *d_mean, float *d_log_std, float *d_value, float *log_prob_out, float *loss,
                    double *stats, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

/* The PPO optimiser step on the device: what SB3's PPO.train [from recall] puts between loss.backward() and the next minibatch --
 * torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) and torch.optim.Adam(eps=1e-5).step() -- over n_tensors <= 32 tensors in one
 * call.  Env-free; the networks' backward and the learner loop stay the caller's.
 * Inputs: `tensors`, a HOST array of n_tensors entries, each four device pointers to `count` dense float32 -- the parameter, its
 *   gradient and the two moments exp_avg (m) and exp_avg_sq (v); `lr`, one device float64, read by the kernel, so a schedule or a replayed
 *   graph changes the rate by writing it; `state`, device float64 [4] = {step, c1, c2, 0}, initially {0, 1, 1, 0}: c1 = beta1^step and
 *   c2 = beta2^step as running products, so no pow is taken.  beta1, beta2 in [0, 1), eps >= 0 and max_grad_norm, finite, are host
 *   arguments: a captured graph keeps the values it was captured with.
 * Arithmetic: every input is widened to float64 once; everything below is an IEEE float64 basic operation (true division and square
 *   root, no reciprocal shortcuts, no contraction); every output is rounded once.
 *   total = sqrt(sum over all elements of all tensors of g g)           the order of the sum is fixed, see below
 *   c = max_grad_norm / (total + 1e-6);  coef = c > 1 ? 1 : c            clip_grad_norm_; a NaN stays a NaN
 *                                                                        max_grad_norm <= 0 is SB3's None: coef = 1
 *   step' = step + 1;  c1' = c1 beta1;  c2' = c2 beta2;  bc1 = 1 - c1';  bc2 = 1 - c2'
 *   gs = g coef
 *   m' = m + (gs - m) (1 - beta1)                                        torch's lerp_
 *   v' = v beta2 + (1 - beta2) gs gs
 *   p' = p - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps))              from the unrounded m', v'
 *   NaN and infinity are not special-cased: one NaN gradient makes total, coef and with them every parameter NaN, as in torch.  No
 *   weight decay, amsgrad or maximize, one parameter group, and a non-finite step is not skipped.
 * Outputs: float32 p', m', v' in place; float64 state <- {step', c1', c2', 0}; float64 stats[4] <- {total, coef, lr, step'}.  The scaled
 *   gradients are not written back.  With flags bit 0 every gradient is zeroed after it is read (zero_grad(set_to_none=False)); the other
 *   bits must be 0.  Overlap between tensors, or of a tensor with lr, state, stats or scratch, is the caller's business: it is not checked.
 * Bit-reproducible: each tensor is cut into chunks of DN_ADAM_CHUNK consecutive elements (the last chunk of a tensor is short; no chunk
 *   straddles two tensors), numbered tensor by tensor.  A chunk's sum of g g: each of 256 lanes adds its four consecutive elements in
 *   ascending order, the 64 lanes of a wave by a fixed tree, the four waves ascending.  The chunk sums: lane l of one wave adds sums l,
 *   l + 64, ... ascending, then the same tree.  The order of every float64 operation is a function of the tensor counts alone; a tensor
 *   whose four pointers are 16-byte aligned moves as 16-byte words, any other as 4-byte words, with the same bits.
 *   scratch        the caller's device memory, 8-byte aligned, at least dn_adam_scratch_bytes(counts, n_tensors): the chunk sums.  The
 *                  library allocates nothing and keeps nothing between calls.
 * Two ordinary launches on `stream`: chunk sums + the state's advance, the update.  No workgroup waits for another, no atomics,
 *   capturable: the pointers of the table are captured with it, so the gradients must be the same tensors at replay.
 * Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a dn_last_error text that names the argument.
 * Layouts: dn_adam_tensor param at 0, grad at 8, exp_avg at 16, exp_avg_sq at 24, count at 32; 40 bytes.  dn_adam_config beta1 at 0,
 *   beta2 at 8, eps at 16, max_grad_norm at 24, n_tensors at 32, flags at 36; 40 bytes. */
#define DN_ADAM_MAX_TENSORS 32
#define DN_ADAM_CHUNK 1024
#define DN_ADAM_ZERO_GRADS 1
typedef struct dn_adam_tensor {
    float *param;           /* device, count float32, 4-byte aligned; updated in place */
    float *grad;            /* read; zeroed with DN_ADAM_ZERO_GRADS */
    float *exp_avg;         /* m, updated in place */
    float *exp_avg_sq;      /* v, updated in place */
    int64_t count;          /* >= 1 */
} dn_adam_tensor;
typedef struct dn_adam_config {
    double beta1, beta2;    /* in [0, 1); SB3's 0.9, 0.999 */
    double eps;             /* >= 0, finite; SB3's 1e-5 */
    double max_grad_norm;   /* finite; > 0: clip the global norm; <= 0: no clip (SB3's None) */
    int32_t n_tensors;      /* 1..32 */
    int32_t flags;          /* bit 0 = DN_ADAM_ZERO_GRADS */
} dn_adam_config;
/* Bytes of scratch for tensors of these element counts (a host array): 8 * sum ceil(count / DN_ADAM_CHUNK); a negative dn_status for a
 * NULL list, n_tensors outside 1..32, a count below 1, or more than 2^31 - 1 chunks. */
int64_t dn_adam_scratch_bytes(const int64_t *counts, int32_t n_tensors);
/* clip_grad_norm_ + Adam.step [from recall] over the tensors of the table, on the device. */
int32_t dn_adam_step(const dn_adam_config *cfg, const dn_adam_tensor *tensors, const double *lr, double *state, double *stats,
                     void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

/* SAC replay minibatches on the device: SB3's ReplayBuffer.sample(batch_size) [from recall] -- a slot and a drone drawn uniformly with
 * replacement per row, the gathered transition, the terminal observation where the episode ended, and dones * (1 - timeouts) -- in one
 * ordinary launch, from either of the two buffer layouts, with a keyed draw whose bits are pinned.  Env-free; the SAC losses, the target
 * update and the learner loop stay the caller's.
 * The window: T = buffer_size slots of N = n_envs drones; S = valid of them hold a whole transition.  skip = -1: they are slots 0 .. S - 1.
 *   skip in 0 .. S: slot `skip` is the one being replaced (a full ring mid-cycle has lost its observation row) and the valid slots are
 *   0 .. S without it.  1 <= S, S + (skip >= 0) <= T <= 2^31 - 1, 1 <= N <= 2^31 - 1, T N <= 2^62.
 * The draw: row j (0-based) under (seed, draw + (draw_offset ? *draw_offset : 0)), the sum mod 2^64 (csrc/dn_replay_draw.h, host and
 *   device):
 *     x = seed ^ (draw * 0xD1342543DE82EF95); z = the (j + 1)-th splitmix64 output from the state x
 *     raw = ((z >> 32) * S) >> 32;  env = ((z & 0xFFFFFFFF) * N) >> 32;  slot = raw + (skip >= 0 && raw >= skip)
 *   With replacement; not rejection sampled: each value's probability is within 2^-32 of uniform.  Row j does not depend on `batch`: a
 *   call for G B rows is G independent batches of B (SAC's gradient_steps).  The flat index of a transition is slot * N + env.
 *   indices        device int64[batch] or NULL.  Not NULL: row j is the transition indices[j] instead -- slot = indices[j] / N and
 *                  env = indices[j] % N by C's division, the slot then clamped into [0, T) and the drone into [0, N), so no read ever
 *                  leaves the buffers; the draw plays no part and draw_offset must be NULL.
 *   draw_offset    device int64[1] or NULL: lets a captured graph draw afresh on every replay, as epoch_offset does for dn_minibatch
 *   indices_out    device int64[batch] or NULL: receives the flat indices of the transitions taken (after the clamp)
 * Sources (dn_replay_source; all device, dense):
 *   DN_REPLAY_PLAIN  float32 obs[T][N][D], next_obs[T][N][D], actions[T][N][A], rewards[T][N], dones[T][N], timeouts[T][N];
 *                    skip must be -1.  out dones_j = dones * (1.0f - timeouts), float32.
 *   DN_REPLAY_RING   float32 obs = the ring [T + 1][N][D] (row t + 1 is both what the step of slot t produced and the input of slot
 *                    t + 1; row T is the spare row), next_obs = terminal_obs[T][N][D], actions, rewards; uint8 dones = done_flags[T][N],
 *                    timeouts = timeout_flags[T][N] (non-zero = set).  out obs_j = ring[slot][env];
 *                    next_obs_j = done ? terminal_obs[slot][env] : ring[slot + 1][env]; dones_j = done && !timeout ? 1.0f : 0.0f.
 * Outputs (device, dense): float32 obs[batch][D], next_obs[batch][D], actions[batch][A], rewards[batch], dones[batch].  Observation,
 *   action and reward words are copied bit for bit (32-bit words: NaN payloads survive).  D = obs_dim in 1..64, A = act_dim in 1..8.  No
 *   output may be a source pointer.
 * One ordinary launch on `stream`: every output word is written once, by a vector store; no atomics, no workgroup waits for another,
 *   nothing is allocated or kept between calls; capturable.  Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a
 *   dn_last_error text.
 * Layout of dn_replay_config: seed at 0, draw at 8, buffer_size at 16, n_envs at 24, valid at 32, skip at 40, obs_dim at 48, act_dim at
 *   52, layout at 56, reserved at 60; 64 bytes.
 * Layout of dn_replay_source: obs at 0, next_obs at 8, actions at 16, rewards at 24, dones at 32, timeouts at 40; 48 bytes. */
#define DN_REPLAY_PLAIN 0
#define DN_REPLAY_RING 1
#define DN_REPLAY_MAX_OBS 64
#define DN_REPLAY_MAX_ACT 8
typedef struct dn_replay_config {
    uint64_t seed;
    uint64_t draw;
    int64_t buffer_size;  /* T */
    int64_t n_envs;       /* N */
    int64_t valid;        /* S */
    int64_t skip;         /* -1, or the slot being replaced, in 0..S */
    int32_t obs_dim;      /* D, 1..64 */
    int32_t act_dim;      /* A, 1..8 */
    int32_t layout;       /* DN_REPLAY_PLAIN or DN_REPLAY_RING */
    int32_t reserved;     /* 0 */
} dn_replay_config;
typedef struct dn_replay_source {
    const void *obs;       /* PLAIN: obs; RING: the ring of T + 1 rows */
    const void *next_obs;  /* PLAIN: next_obs; RING: terminal_obs */
    const void *actions;
    const void *rewards;
    const void *dones;     /* PLAIN: float32 dones; RING: uint8 done_flags */
    const void *timeouts;  /* PLAIN: float32 timeouts; RING: uint8 timeout_flags */
} dn_replay_source;
/* Host only: needs no device and makes no HIP call.  out[0 .. count) <- the flat indices slot * N + env of rows start .. start + count - 1
 * under (seed, draw), in HOST memory, by the code the kernel runs.  1 <= valid, n_envs <= 2^31 - 1, skip -1 or in 0..valid, 0 <= start,
 * 0 <= count, start + count <= 2^31 - 1. */
int32_t dn_replay_indices(uint64_t seed, uint64_t draw, int64_t valid, int64_t n_envs, int64_t skip, int64_t start, int64_t count,
                          int64_t *out);
/* SB3 ReplayBuffer.sample [from recall] for `batch` rows, 1 <= batch <= 2^31 - 1. */
int32_t dn_replay_sample(const dn_replay_config *cfg, const dn_replay_source *src, int64_t batch, const int64_t *indices,
                         const int64_t *draw_offset, float *obs, float *next_obs, float *actions, float *rewards, float *dones,
                         int64_t *indices_out, int32_t device_id, void *stream);

/* The SAC loss heads on the device: SB3's SAC.train body [from recall] between the networks' head outputs and the scalar losses -- the
 * squashed Gaussian's reparametrised sample with its log-probability, the TD target and the critic loss, the actor loss, the
 * entropy-coefficient loss, and the gradients with respect to every head output.  Env-free; the networks' own forward and backward, the
 * optimisers (dn_adam_step with eps 1e-8 and no clip), the Polyak update and the learner loop stay the caller's.  One gradient step of
 * SB3, for a replay batch (obs, next_obs, actions, rewards, dones), an actor with heads mu and log_std, C critics and log_ent_coef:
 *   a_pi, lp      = squash(mu(obs), log_std(obs), eps)                      dn_sac_policy; backward dn_sac_policy_backward
 *   a_n, lp_n     = squash(mu(next_obs), log_std(next_obs), eps_n)          dn_sac_policy, no gradient
 *   critic_loss   from Q_c(obs, actions), Qtarget_c(next_obs, a_n), lp_n    dn_sac_critic_loss
 *   actor_loss, ent_coef_loss from lp, Q_c(obs, a_pi)                       dn_sac_actor_loss
 * Arithmetic (csrc/dn_sac_math.h, which host and device both run): every float32 input is widened to float64 once; every operation below
 *   is an IEEE float64 operation, no contraction; exp, tanh and log are the float64 library functions; every output is rounded once.  NaN
 *   and infinity are not special-cased.
 * The squashed policy head, row b < batch, column j < A = act_dim, raw = the log_std head's output, eps = the caller's N(0, 1) draw:
 *   ls = clamp(raw, log_std_min, log_std_max)     torch.clamp: a NaN stays, the gradient passes at the bounds
 *   std = exp(ls)            pre = mean + std eps            a = tanh(pre)
 *   t = exp(-2 |pre|)        J = 4 t / ((1 + t)(1 + t))      sech^2(pre); never formed as 1 - a a, which is lost once |pre| > 9
 *   term_j = -0.5 eps^2 - ls - 0.5 log(2 pi) - log(J + 1e-6)      eps itself, not (pre - mean) / std, which loses eps at a small std
 *   log_prob_b = term_0 + term_1 + ..., j ascending;  actions_bj = a
 *   Where the literal float32 expression of SB3 is well conditioned the two agree (|pre| <= 6, log_std >= -5: to 2^-40 of the terms plus
 *   the literal form's own cancellation 2^-51 / (J + 1e-6)).
 * Its backward, given g_a[batch][A] = d L / d actions and g_lp[batch] = d L / d log_prob (NULL = zero), recomputed from mean, raw, eps:
 *   K = 2 a J / (J + 1e-6);  d_pre = g_a J + g_lp K;  d_mean = d_pre;  d_ls = d_pre std eps - g_lp;
 *   d_log_std = d_ls where log_std_min <= raw <= log_std_max, else 0.
 * The critic loss, row b, critic c < C = n_critics:
 *   alpha = exp(log_ent_coef[0]), read from device memory when the kernel runs and rounded correctly (csrc/dn_exp_cr.h); with
 *           log_ent_coef NULL the host value ent_coef (SB3's fixed coefficient)
 *   nq = min_c next_q_c                           c ascending; a NaN on either side wins, as in torch.min
 *   y = rewards + (1 - dones) gamma (nq - alpha next_log_prob)
 *   e_c = q_c - y;  critic_loss = 0.5 (S_0 / batch + S_1 / batch + ...), S_c = sum_b e_c^2, c ascending;  d_q_c = e_c / batch
 *   target_q = (float) y: for the caller's logging; the loss uses the unrounded y.
 *   stats[8] = critic_loss, alpha, mean_b y, mean_b q_0 .. mean_b q_3 (0 from n_critics on), 0.
 * The actor and entropy-coefficient loss, row b:
 *   qmin = min_c q_pi_c                           c ascending; a tie picks the lowest c, the first NaN wins
 *   actor_loss = sum_b (alpha log_prob - qmin) / batch;  d_log_prob = alpha / batch;  d_q_pi_c = -[c is the pick] / batch
 *   with log_ent_coef: ent_coef_loss = -(log_ent_coef m), d_log_ent_coef = -m, m = sum_b (log_prob + target_entropy) / batch
 *   with a fixed coefficient ent_coef_loss = 0, d_log_ent_coef must be NULL and is not written.
 *   stats[8] = actor_loss, ent_coef_loss, alpha, mean_b log_prob, mean_b qmin, d_log_ent_coef (0 when fixed), 0, 0.
 *   Both losses read log_ent_coef when they run: a caller who steps the coefficient's optimiser after the actor loss reproduces SB3's order.
 * Per-critic inputs and outputs (q, next_q, d_q, q_pi, d_q_pi) are HOST arrays of n_critics device pointers, each to `batch` dense
 *   float32.  gamma, target_entropy, ent_coef, log_std_min, log_std_max are host values: a captured graph keeps the ones it was
 *   captured with.  Each entry point reads the fields of dn_sac_config that its arithmetic names, and `reserved`.
 * Bit-reproducible: the policy head is a row per lane with nothing reduced; [batch][A] tensors move as 16-byte words when A % 4 == 0 and
 *   all of them are 16-byte aligned, else as 4-byte words, with the same bits.  The sums over b are float64 sums per block of 1024
 *   consecutive rows (lanes by a fixed tree, waves ascending), the blocks added in ascending order: the order of every float64 operation
 *   is a function of (batch, act_dim, n_critics) alone.
 *   scratch        the caller's device memory, 8-byte aligned, at least dn_sac_loss_scratch_bytes(batch, n_critics): the block sums.  One
 *                  size serves both losses.  The library allocates nothing and keeps nothing between calls.
 * Launches on `stream`: one for dn_sac_policy, one for dn_sac_policy_backward, two for each loss (rows + block sums, a one-wave merge).  No
 *   workgroup waits for another, no atomics, capturable.  No output may overlap an input or another output.
 * Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a dn_last_error text that names the argument and the value.
 * Layout of dn_sac_config: gamma at 0, target_entropy at 8, ent_coef at 16, log_std_min at 24, log_std_max at 32, act_dim at 40,
 *   n_critics at 44, reserved at 48; 56 bytes. */
#define DN_SAC_MAX_ACT 8
#define DN_SAC_MAX_CRITICS 4
typedef struct dn_sac_config {
    double gamma;           /* in [0, 1]; SB3's 0.99 (critic loss) */
    double target_entropy;  /* finite; SB3's "auto" is -act_dim (actor loss) */
    double ent_coef;        /* >= 0, finite: alpha when log_ent_coef is NULL (both losses) */
    double log_std_min;     /* finite, < log_std_max; SB3's -20 (policy head) */
    double log_std_max;     /* finite; SB3's 2 (policy head) */
    int32_t act_dim;        /* 1..8 (policy head) */
    int32_t n_critics;      /* 1..4 (both losses) */
    int64_t reserved;       /* 0 */
} dn_sac_config;
/* Bytes of scratch for either loss over `batch` rows and `n_critics` critics: 8 (2 n_critics + 2) per block of 1024 rows; a negative
 * dn_status for batch < 1 or beyond 2^31 - 1, or n_critics outside 1..4. */
int64_t dn_sac_loss_scratch_bytes(int64_t batch, int32_t n_critics);
/* SB3 SquashedDiagGaussianDistribution [from recall]: actions[batch][A] and log_prob[batch] from mean, log_std (raw), noise [batch][A]. */
int32_t dn_sac_policy(const dn_sac_config *cfg, int64_t batch, const float *mean, const float *log_std, const float *noise, float *actions,
                      float *log_prob, int32_t device_id, void *stream);
/* Its backward: d_mean[batch][A], d_log_std[batch][A] from g_actions[batch][A] and g_log_prob[batch], either of which may be NULL (zero). */
int32_t dn_sac_policy_backward(const dn_sac_config *cfg, int64_t batch, const float *mean, const float *log_std, const float *noise,
                               const float *g_actions, const float *g_log_prob, float *d_mean, float *d_log_std, int32_t device_id,
                               void *stream);
/* SB3 SAC.train [from recall]: the TD target, the critic loss, its statistics and d_q_c. */
int32_t dn_sac_critic_loss(const dn_sac_config *cfg, int64_t batch, const float *const *q, const float *const *next_q,
                           const float *next_log_prob, const float *rewards, const float *dones, const float *log_ent_coef,
                           float *const *d_q, float *target_q, float *loss, double *stats, void *scratch, int64_t scratch_bytes,
                           int32_t device_id, void *stream);
/* SB3 SAC.train [from recall]: the actor loss and the entropy-coefficient loss, their statistics and gradients. */
int32_t dn_sac_actor_loss(const dn_sac_config *cfg, int64_t batch, const float *log_prob, const float *const *q_pi,
                          const float *log_ent_coef, float *d_log_prob, float *const *d_q_pi, float *d_log_ent_coef, float *actor_loss,
                          float *ent_coef_loss, double *stats, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

/* The training pass of the reference's Tanh networks on the device: a forward that saves what the backward needs, and a backward from
 * the gradient with respect to the head output (what dn_ppo_loss hands out) to every weight and bias gradient and, where asked, to the
 * input.  Env-free; the loss head, the optimiser and the learner loop are dn_ppo_loss, dn_adam_step and the caller's.
 * The network: `layers`, a HOST array of n_layers = 2..4 linear layers, the head last; layer 0 has in_dim 1..64 (any value), every
 *   hidden width (the out_dim of every layer but the last) is a multiple of 32 in 32..512, the head's out_dim is 1..32, and
 *   layers[l].in_dim == layers[l - 1].out_dim.  weight and bias are torch's nn.Linear tensors, float32 [out_dim][in_dim] and [out_dim],
 *   dense, read in place: nothing is packed on the host and no second copy of the weights exists.  batch is 1..2^24 rows, any value.
 *     h_0 = x;  h_l = tanh(h_{l-1} W_l^T + b_l) for the hidden layers;  out = h_{L-1} W_L^T + b_L
 *   dn_mlp_train_forward writes out [batch][head out_dim] and saves the hidden activations as float32 in scratch.
 *   dn_mlp_train_backward must follow a forward with the same config, layers, batch, x and scratch (the caller's business: nothing can
 *   check it).  With dZ_L = d_out [batch][head out_dim] and dZ_l = dH_l (1 - h_l^2) it forms
 *     d_bias_l = sum over the rows of dZ_l;  d_weight_l = dZ_l^T h_{l-1};  dH_{l-1} = dZ_l W_l;  d_x = dH_0 where d_x is not NULL.
 *   flags bit 0 (DN_MLP_TRAIN_ACCUMULATE): each finished float32 gradient is added to the tensor (one float32 add) instead of
 *   overwriting it.  Bit 1 (DN_MLP_TRAIN_NO_PARAM_GRADS): the backward forms d_x only; d_weight and d_bias are neither read nor
 *   written and may be NULL.  d_x is always overwritten.  The other bits and `reserved` must be 0; `activation` must be
 *   DN_MLP_ACT_TANH: these three entry points take Tanh only.  ReLU, an input from two tensors, a head of two parts and several
 *   networks a call are dn_sac_train_forward / dn_sac_train_backward below, on the same product kernel.
 * Arithmetic, float32 grade: every matrix product runs on v_mfma_f32_32x32x16_bf16 with BOTH operands split on the device, as they
 *   are staged, into two bfloat16 words hi = bf16(v), lo = bf16(v - hi), round to nearest even (csrc/dn_bf16_split.h); a product is
 *   the three MFMAs lo hi, hi lo, hi hi, in this order, into one float32 accumulator, K-steps of 16 in ascending order.  Bias add,
 *   tanh(z) = 1 - 2 / (1 + 2^(2 log2(e) z)) (v_exp_f32, v_rcp_f32) and 1 - h h are float32; activations and dZ travel between the
 *   launches as float32.
 * Bit-reproducible: no atomics, no workgroup waits for another, and the order of every addition is a function of (batch, the layer
 *   dimensions) alone.  Row b of out, of the saved activations, of every dZ and of d_x depends on no other row and not on batch.  The
 *   sums over the batch: the rows are cut into chunks of DN_MLP_TRAIN_CHUNK consecutive rows (the last is short).  One workgroup forms
 *   each (chunk, output tile) partial of d_weight_l -- the MFMA chain above over the chunk's rows in ascending K-steps of 16 rows, rows
 *   at and beyond batch staged as exact zeros -- as float32 into scratch.  The chunk's partial of d_bias_l[o] is a float64 sum: lane
 *   group g = 0..7 adds the rows 4 g .. 4 g + 3 of every 32 rows of the chunk in ascending order, then the eight groups are added in
 *   ascending order.  One merge launch adds the chunks' partials in ascending chunk order in float64 and rounds once to float32.
 *   scratch        the caller's device memory, 16-byte aligned, at least dn_mlp_train_scratch_bytes(cfg, layers, batch).  With
 *                  r(b) = b rounded up to a multiple of 256 and C = ceil(batch / DN_MLP_TRAIN_CHUNK) its regions are, in this order:
 *                  h_l, r(4 batch out_l) bytes per hidden layer; dZ_l, the same again per hidden layer; the d_weight partials,
 *                  r(4 C out_l in_l) per layer; the d_bias partials, r(8 C out_l) per layer.  The library allocates nothing and keeps
 *                  nothing between calls.
 * Ordinary launches on `stream`, capturable: the forward one per layer; the backward one weight-gradient and one data-gradient launch
 *   per layer (none for layer 0's data gradient without d_x, no weight-gradient launches with bit 1) and the merge.  Every output word
 *   is written exactly once by a vector store (read once and written once with bit 0).  No output (out, d_x, d_weight, d_bias,
 *   scratch) may overlap an input (x, d_out, weight, bias) or, among the gradient tensors, d_x and out, one another.
 * Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a dn_last_error text that names the argument.
 * Layouts: dn_mlp_train_layer weight at 0, bias at 8, d_weight at 16, d_bias at 24, in_dim at 32, out_dim at 36; 40 bytes.
 *   dn_mlp_train_config n_layers at 0, activation at 4, flags at 8, reserved at 12; 16 bytes. */
#define DN_MLP_TRAIN_MAX_LAYERS 4
#define DN_MLP_ACT_TANH 0
#define DN_MLP_ACT_RELU 1
#define DN_MLP_TRAIN_ACCUMULATE 1
#define DN_MLP_TRAIN_NO_PARAM_GRADS 2
#define DN_MLP_TRAIN_CHUNK 1024
typedef struct dn_mlp_train_layer {
    const float *weight;    /* device float32 [out_dim][in_dim], dense, torch's nn.Linear layout, read in place */
    const float *bias;      /* device float32 [out_dim] */
    float *d_weight;        /* device float32 [out_dim][in_dim]; may be NULL for dn_mlp_train_forward and with bit 1 */
    float *d_bias;          /* device float32 [out_dim]; as d_weight */
    int32_t in_dim;         /* layer 0: 1..64; else the out_dim of the layer before */
    int32_t out_dim;        /* hidden: a multiple of 32 in 32..512; head: 1..32 */
} dn_mlp_train_layer;
typedef struct dn_mlp_train_config {
    int32_t n_layers;       /* 2..4 linear layers, the head included */
    int32_t activation;     /* DN_MLP_ACT_TANH */
    int32_t flags;          /* bit 0 = DN_MLP_TRAIN_ACCUMULATE, bit 1 = DN_MLP_TRAIN_NO_PARAM_GRADS */
    int32_t reserved;       /* 0 */
} dn_mlp_train_config;
/* Bytes of scratch for this network over `batch` rows (the formula above; only the dimensions of `layers` are read): host only, no HIP
 * call.  A negative dn_status for a NULL argument, a dimension or chain the calls refuse, or batch outside 1..2^24. */
int64_t dn_mlp_train_scratch_bytes(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch);
/* out [batch][head out_dim] from x [batch][layers[0].in_dim]; the hidden activations stay in scratch for the backward. */
int32_t dn_mlp_train_forward(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, const float *x, int64_t batch, float *out,
                             void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);
/* Every d_weight and d_bias, and d_x [batch][layers[0].in_dim] where it is not NULL, from d_out [batch][head out_dim]. */
int32_t dn_mlp_train_backward(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, const float *x, const float *d_out,
                              int64_t batch, float *d_x, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

/* The training pass of the SAC networks on the device, and the Polyak update of the target critics: what SB3's SAC.train [from recall]
 * does between the replay minibatch, the loss heads above and the optimiser -- the actor (latent_pi with the heads mu | log_std), the
 * critics over cat(obs, actions) and their targets.  The second, wider family on the product kernel of dn_mlp_train_*: everything that
 * comment says of the arithmetic (v_mfma_f32_32x32x16_bf16, both operands split into bf16 hi + lo as they are staged, lo hi, hi lo,
 * hi hi into one float32 accumulator, K-steps of 16 ascending), of the chunks of DN_MLP_TRAIN_CHUNK rows, of the float64 bias sums and of
 * the merge holds here word for word, and a network that both families can express (Tanh, one network, one input tensor, a head of one
 * part) gets the same bits from both.  What this family adds is addressing, and ReLU:
 *   activation     DN_MLP_ACT_TANH or DN_MLP_ACT_RELU.  ReLU forward: h = z > 0 ? z : +0.  Backward: dZ = h > 0 ? dH : +0.0, read from
 *                  the saved activation as torch's threshold_backward does.  A NaN pre-activation is outside the contract (it becomes +0).
 *   x = (x0 | x1)  layer 0 reads x0 [batch][in0] and x1 [batch][in1] side by side, gathered as they are staged and never materialised:
 *                  in0 1..64, in1 0..63, in0 + in1 <= 64 = layers[c][0].in_dim; x1 is NULL exactly when in1 = 0.  The input gradient
 *                  leaves as d_x0 [batch][in0] and d_x1 [batch][in1]; either may be NULL (not wanted: its columns are not stored).
 *   head parts     the head is head_parts = 1..2 linear layers over the last hidden layer (the actor's mu and log_std), read in place as
 *                  the row blocks of one head: out_dim 1..32 each, at most 32 together.  Outputs and head gradients are one dense
 *                  [batch][out_dim of the part] tensor a part.  The forward, the head's weight-gradient partials and dH of the last hidden
 *                  layer run over the concatenated k / n in the order an undivided head has.
 *   n_nets         1..4 networks of identical dimensions that share x (the twin critics), advanced by the same launches: a grid
 *                  dimension is the network (network x chunk for the weight gradient), and the number of launches does not depend on
 *                  n_nets.  Network c's outputs and gradients have the bits it gets alone.  d_x = sum over the networks of dZ0_c W0_c is
 *                  ONE product [dZ0_0 | dZ0_1 | ...] against the stacked W0_c, K running over the networks in ascending order: K-steps
 *                  of 16 over network 0's hidden units, then network 1's, into one accumulator.
 * `layers` is a HOST array dn_mlp_train_layer[n_nets][n_layers - 1 + head_parts], network-major; a network's last head_parts entries
 *   are the head's parts, each with in_dim = the last hidden width.  Hidden widths are multiples of 32 in 32..512, batch is 1..2^24.
 *   `out` and `d_out` are HOST arrays of n_nets * head_parts device pointers, network-major.  flags: DN_MLP_TRAIN_ACCUMULATE and
 *   DN_MLP_TRAIN_NO_PARAM_GRADS with the meaning above; with the latter at least one of d_x0, d_x1 is required.
 * Bit-reproducible as above: no atomics, no workgroup waits for another, every output word written exactly once, row b of every
 *   per-row output independent of the other rows and of batch, and the order of every addition a function of (n_nets, the dimensions,
 *   batch) alone: within a product k ascends over the concatenated operand; the batch sums are per chunk and merged in ascending chunk
 *   order in float64.
 *   scratch        the caller's device memory, 16-byte aligned, at least dn_sac_train_scratch_bytes(cfg, layers, batch): n_nets
 *                  consecutive blocks, network 0 first.  With r and C as above, in = in0 + in1 for layer 0 and the head taken as one layer
 *                  of out_L = the sum of its parts, a block's regions are, in this order: h_l, r(4 batch out_l) per hidden layer; dZ_l,
 *                  the same again per hidden layer; the d_weight partials, r(4 C out_l in_l) per layer; the d_bias partials,
 *                  r(8 C out_l) per layer.
 * Launches on `stream`, capturable: the forward one per layer; the backward one weight-gradient and one data-gradient launch per layer
 *   (none for layer 0's data gradient without d_x0 and d_x1, no weight-gradient launches with DN_MLP_TRAIN_NO_PARAM_GRADS) and the merge.
 *   No output may overlap an input or another output.
 * dn_polyak_update: target_i <- (1 - tau) target_i + tau source_i over n_tensors = 1..DN_ADAM_MAX_TENSORS tensors of counts[i] >= 1
 *   float32 elements, one launch.  source, target and counts are HOST arrays.  omt = 1.0 - tau is formed on the host in float64; an
 *   element is (float)(omt * (double)t + tau * (double)s): two float64 products and one float64 add, no contraction, rounded once
 *   (csrc/dn_sac_math.h dn_polyak, which host and device both compile).  That is the float64 statement, not the exact one: beside a
 *   float32 tie (tau = 0.005 and t / 200 half an ulp of the result) it may be one float32 ulp from (1 - tau) t + tau s evaluated in a
 *   wider format and rounded once.  tau is a host double in [0, 1]: a captured graph keeps it.
 *   No target may overlap a source or another target.
 * Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a dn_last_error text that names the argument, layers[c][l].field
 *   included.
 * Layout of dn_sac_train_config: n_nets at 0, n_layers at 4, head_parts at 8, activation at 12, in0 at 16, in1 at 20, flags at 24,
 *   reserved at 28; 32 bytes. */
#define DN_SAC_TRAIN_MAX_NETS 4
#define DN_SAC_TRAIN_MAX_PARTS 2
typedef struct dn_sac_train_config {
    int32_t n_nets;         /* 1..4 networks of identical dimensions sharing x */
    int32_t n_layers;       /* 2..4 linear layers a network, the head counted once */
    int32_t head_parts;     /* 1..2 */
    int32_t activation;     /* DN_MLP_ACT_TANH or DN_MLP_ACT_RELU */
    int32_t in0;            /* 1..64 */
    int32_t in1;            /* 0..63, in0 + in1 <= 64 */
    int32_t flags;          /* bit 0 = DN_MLP_TRAIN_ACCUMULATE, bit 1 = DN_MLP_TRAIN_NO_PARAM_GRADS */
    int32_t reserved;       /* 0 */
} dn_sac_train_config;
/* Bytes of scratch (the formula above; only the dimensions of `layers` are read): host only, no HIP call.  A negative dn_status for a
 * NULL argument, a configuration, dimension or chain the calls refuse, or batch outside 1..2^24. */
int64_t dn_sac_train_scratch_bytes(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch);
/* out[c * head_parts + p] [batch][out_dim of part p] from (x0 | x1); the hidden activations stay in scratch for the backward. */
int32_t dn_sac_train_forward(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, const float *x0, const float *x1,
                             int64_t batch, float *const *out, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);
/* Every d_weight and d_bias, and d_x0, d_x1 where they are not NULL, from d_out[c * head_parts + p]; after a forward with the same
 * config, layers, batch, x0, x1 and scratch. */
int32_t dn_sac_train_backward(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, const float *x0, const float *x1,
                              const float *const *d_out, int64_t batch, float *d_x0, float *d_x1, void *scratch, int64_t scratch_bytes,
                              int32_t device_id, void *stream);
int32_t dn_polyak_update(int32_t n_tensors, const float *const *source, float *const *target, const int64_t *counts, double tau,
                         int32_t device_id, void *stream);

/* One LSTM layer on the device with torch.nn.LSTM semantics -- num_layers = 1, unidirectional, bias = True, proj_size = 0, time-major:
 * the recurrent policy of the reference's fourth learner (sb3_contrib RecurrentPPO, MlpLstmPolicy [from recall]).  dn_lstm_forward over a
 * sequence saves what dn_lstm_backward needs; with T = 1 and h_T = h0, c_T = c0 it is the rollout step that updates a resident state in
 * place.  Env-free; the third family on the product kernel of dn_mlp_train_*: what that comment says of the arithmetic
 * (v_mfma_f32_32x32x16_bf16, both operands split into bf16 hi + lo as they are staged, lo hi, hi lo, hi hi into one float32 accumulator,
 * K-steps of 16 ascending), of the chunks of DN_MLP_TRAIN_CHUNK rows, of the float64 bias sums and of the merge holds here word for word.
 * The layer: in_dim I = 1..64 (any value), hidden H a multiple of 32 in 32..512.  The parameters are torch's tensors, float32, dense, read
 *   in place: weight_ih_l0 [4H][I], weight_hh_l0 [4H][H], bias_ih_l0 [4H], bias_hh_l0 [4H], the gate rows in torch's order i, f, g, o.
 *   T = 1..1024 steps, B = 1..2^24 rows a step, T B <= 2^24.  x is [T][B][I]; episode_starts is uint8 [T][B] or NULL (no starts).
 * Forward, step t = 0..T-1, row b: sb3_contrib's _process_sequence [from recall] multiplies both states by 1 - episode_start.
 *     keep = episode_starts is NULL or episode_starts[t][b] == 0
 *     hp = keep ? h_{t-1}[b] : +0.0, cp = keep ? c_{t-1}[b] : +0.0, with h_{-1} = h0, c_{-1} = c0 [B][H]
 *     z[n] = sum over k of (x_t[b] | hp)[k] (W_ih | W_hh)[n][k] + (b_ih[n] + b_hh[n])     k ascends over the I columns of x, then the H of hp;
 *                                                  the bias pair is one float32 add, adding it to the accumulator one more
 *     i = sig(z[j]), f = sig(z[H + j]), g = tanh(z[2H + j]), o = sig(z[3H + j])
 *                                                  sig(z) = 1 / (1 + 2^(-log2(e) z)), tanh as dn_mlp_train_*: v_exp_f32, v_rcp_f32
 *     c_t = f cp + i g;  h_t = o tanh(c_t)          float32, no contraction
 *   Outputs: h_seq, c_seq [T][B][H] (the backward reads both) and h_T, c_T [B][H], the last step's.  h_T may be the tensor h0 and c_T
 *   the tensor c0 (the same address): step 0 alone reads h0 and c0, step t > 0 reads h_seq[t - 1] and c_seq[t - 1], and h_T, c_T are
 *   written by the last step after both were read.  The activated gates stay in scratch as float32 [T][B][4H].
 * Backward, t = T-1..0, from d_hseq [T][B][H]; the two carries start at zero.  It must follow a forward with the same config, params, T,
 *   B, x, episode_starts, h0, c0, h_seq, c_seq and scratch (the caller's business), and it consumes the saved gates: dZ is written over
 *   them, so a second backward without a forward in between is the caller's error.  It reads h0 and c0 again (row 0 .. B-1 of hprev
 *   and of cp), so they must still hold what the forward read: a forward whose h_T was h0 or whose c_T was c0 has overwritten
 *   them and cannot be followed by a backward.  The in-place pair is for the forward-only rollout step.
 *     dh = d_hseq[t][b] + carry_h;  tc = tanh(c_seq[t][b]);  dc = carry_c + dh o (1 - tc tc)
 *     dz_i = dc g i (1 - i), dz_f = dc cp f (1 - f), dz_g = dc i (1 - g g), dz_o = dh tc o (1 - o)     products left to right
 *     carry_c = keep ? dc f : +0.0;  carry_h = keep ? (dZ_t W_hh)[b] : +0.0     one product a step with K = 4H, the mask in its epilogue
 *   and after the loop: d_x [T][B][I] = dZ W_ih as one product over all T B rows, where d_x is not NULL; d_w_ih = dZ^T x and
 *   d_w_hh = dZ^T hprev as one weight-gradient product over the T B rows against the column blocks (x | hprev), row t B + b of hprev
 *   being keep ? (t ? h_seq[t - 1][b] : h0[b]) : +0.0, addressed as it is staged and never materialised.  The chunks are
 *   DN_MLP_TRAIN_CHUNK consecutive rows of the T B and may straddle steps.  d_b_ih and d_b_hh both receive the column sums of dZ.
 *   Gradients with respect to h0, c0, h_T and c_T are not formed.
 *   flags: DN_MLP_TRAIN_ACCUMULATE and DN_MLP_TRAIN_NO_PARAM_GRADS with the meaning above (with the latter d_x is required and the four
 *   gradient tensors are neither read nor written and may be NULL); the other bits and `reserved` must be 0.
 * Bit-reproducible as above: no atomics, no workgroup waits for another, row b of every per-row output independent of the other rows
 *   and of B, and a sequence of T steps gives the bits of T calls with T = 1 that chain the state.
 *   scratch        the caller's device memory, 16-byte aligned.  With r(b) = b rounded up to a multiple of 256 and
 *                  C = ceil(T B / DN_MLP_TRAIN_CHUNK) its regions are, in this order: the gates, r(16 T B H) bytes; carry_h and carry_c,
 *                  r(4 B H) each; the weight-gradient partials [C][4H][I + H], r(16 C H (I + H)); the float64 bias partials [C][4H],
 *                  r(32 C H).  dn_lstm_backward asks for all of it, dn_lstm_scratch_bytes(cfg, T, B); dn_lstm_forward for the gates
 *                  alone, r(16 T B H), so a rollout step holds no gradient scratch.
 * Launches on `stream`, capturable: the forward two a step (the product, then the cell); the backward two a step (the cell, then the
 *   product; none for step 0's), one for d_x where it is wanted, and the weight gradient with its merge without bit 1.  Every output
 *   word is written exactly once by a vector store (read once and written once with bit 0).  No output (h_seq, c_seq, h_T, c_T; d_x and
 *   the gradient tensors; scratch) may overlap an input or another output, except that h_T may be h0 itself and c_T c0 itself.
 * Validates before the first device call: DN_ERR_INVALID_ARGUMENT with a dn_last_error text that names the argument.
 * Layouts: dn_lstm_config in_dim at 0, hidden at 4, flags at 8, reserved at 12; 16 bytes.
 *   dn_lstm_params w_ih at 0, w_hh at 8, b_ih at 16, b_hh at 24, d_w_ih at 32, d_w_hh at 40, d_b_ih at 48, d_b_hh at 56; 64 bytes. */
typedef struct dn_lstm_config {
    int32_t in_dim;         /* I: 1..64 */
    int32_t hidden;         /* H: a multiple of 32 in 32..512 */
    int32_t flags;          /* bit 0 = DN_MLP_TRAIN_ACCUMULATE, bit 1 = DN_MLP_TRAIN_NO_PARAM_GRADS */
    int32_t reserved;       /* 0 */
} dn_lstm_config;
typedef struct dn_lstm_params {
    const float *w_ih;      /* device float32 [4H][I], torch's weight_ih_l0, read in place */
    const float *w_hh;      /* device float32 [4H][H], weight_hh_l0 */
    const float *b_ih;      /* device float32 [4H], bias_ih_l0; not read by dn_lstm_backward */
    const float *b_hh;      /* device float32 [4H], bias_hh_l0; as b_ih */
    float *d_w_ih;          /* device float32 [4H][I]; may be NULL for dn_lstm_forward and with bit 1 */
    float *d_w_hh;          /* device float32 [4H][H]; as d_w_ih */
    float *d_b_ih;          /* device float32 [4H]; as d_w_ih */
    float *d_b_hh;          /* device float32 [4H]; as d_w_ih; receives the value d_b_ih does */
} dn_lstm_params;
/* Bytes of scratch for the backward of T steps of B rows (the formula above): host only, no HIP call.  A negative dn_status for a NULL
 * cfg, a dimension the calls refuse, or T, B or T B out of range. */
int64_t dn_lstm_scratch_bytes(const dn_lstm_config *cfg, int64_t T, int64_t B);
/* h_seq, c_seq [T][B][H] and h_T, c_T [B][H] from x [T][B][I], episode_starts [T][B] or NULL, h0 and c0 [B][H]. */
int32_t dn_lstm_forward(const dn_lstm_config *cfg, const dn_lstm_params *params, const float *x, const uint8_t *episode_starts,
                        const float *h0, const float *c0, int64_t T, int64_t B, float *h_seq, float *c_seq, float *h_T, float *c_T,
                        void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);
/* The four gradient tensors, and d_x [T][B][I] where it is not NULL, from d_hseq [T][B][H]; after the forward, once. */
int32_t dn_lstm_backward(const dn_lstm_config *cfg, const dn_lstm_params *params, const float *x, const uint8_t *episode_starts,
                         const float *h0, const float *h_seq, const float *c_seq, const float *c0, const float *d_hseq, int64_t T,
                         int64_t B, float *d_x, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DRONENAV_H */
