/*
 * dn_oracle.h -- CPU ORACLE for the drone-navigation environment step.
 *
 * TEST INFRASTRUCTURE ONLY.  This is a plain-C restatement of the reference's
 * algorithm (eRGiBi/DRL-DroneNavigation, pure Python + PyBullet) for the hot path
 * PBDroneEnv.step -> BaseAviary.step -> p.stepSimulation, plus the SB3
 * SubprocVecEnv/Monitor auto-reset semantics wrapped around it.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it.  The product
 * (drl-dronenavigation_amd/, include/dronenav.h, libdronenav.so) never does.
 *
 * PARITY STATUS
 *   pinned   : rows A1 A2 A3 A6 A7 A8 A9 A10 A12 of SURVEY.md section 8(a) are checked
 *              against golden vectors produced by importing the reference's own Python
 *              (tests/golden/gen_golden.py, fixtures under tests/golden/).
 *   UNPINNED : row A4 (p.stepSimulation) and the Bullet half of A5
 *              (p.getEulerFromQuaternion) live in the third-party `pybullet` wheel
 *              (Bullet3 C++), which is neither vendored under /root/reference nor pinned
 *              by its requirements.txt / uv.lock, and cannot be installed here.  Those two
 *              functions restate Bullet's published algorithm from memory
 *              (btMultiBody::computeAccelerationsArticulatedBodyAlgorithmMultiDof,
 *              btMultiBody::stepPositionsMultiDof, pybullet.c getEulerFromQuaternion) and
 *              are "parity unpinned".  Stand-in evidence (tests/test_bullet_invariants.py): closed-form one-step
 *              results, an independent world-frame integrator (1e-12), and through it the reference's own
 *              dead explicit model BaseAviary._dynamics (BaseAviary.py:899-973, fixture dead_dynamics.npz,
 *              1e-13 with the damping switched off) -- the structure of the step is tied to a statement the
 *              reference owns; Bullet's damping law and velocity clamp are recall.
 *
 * All arithmetic follows the reference's dtypes: float32 for the action chain
 * (A1-A3, numpy float32 arrays), float64 for everything else.
 */
#ifndef DN_ORACLE_H
#define DN_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORC_MAX_WAYPOINTS 64
#define ORC_OBS_DIM 13

/* Environment configuration == the constructor arguments of PBDroneEnv
 * (Sol/Model/Environments/PBDroneEnv.py:41-65) as passed by
 * PBDroneSimulator.make_env (Sol/Model/PBDroneSimulator.py:154-171). */
typedef struct orc_config {
    int32_t num_waypoints;                      /* len(target_points) */
    double waypoints[ORC_MAX_WAYPOINTS * 3];    /* target_points */
    double spawn[3];                            /* initial_xyzs[0] */
    double dim[6];                              /* aviary_dim: x_low y_low z_low x_high y_high z_high */
    double threshold;                           /* 0.3, PBDroneSimulator.py:116 */
    int32_t max_steps;                          /* args.max_env_steps */
    int32_t circle;                             /* track.is_circle */
    int32_t cylinder;                           /* True in make_env */
    int32_t include_distance;                   /* True in run_full_training */
    int32_t normalize_actions;                  /* True in run_full_training */
    int32_t normalize_obs;                      /* normalize.NormalizeObservation wrapper (always on in make_env) */
    int32_t ground_contact;                     /* approximate len(p.getContactPoints())>0 against plane.urdf */
    int32_t f32_state;                          /* 1: round the stored state to float32 after every vec step
                                                      (mirrors the HIP build's float32 HBM state) */
    /* sim-to-real noise (BASELINE config 5; the reference has none: sigma = 0 is the reference) */
    float act_noise_sigma;
    float obs_noise_sigma;
    uint64_t seed;
    int64_t env_id_offset;                      /* global id of env 0 (rank sharding) */
    /* optional reward wrappers of make_env (PBDroneSimulator.py:191-194), inside Monitor:
     * TransformReward(clip(-10, 10)) if --clip_rew, then gym NormalizeReward() if --norm_rew */
    int32_t clip_rew;
    int32_t norm_rew;
    /* N4 -- options present but unreachable in the reference (BaseAviary.step forces Physics.PYB, BaseAviary.py:411;
     * PBDroneEnv overrides _preprocessAction for ActionType.THRUST only):
     *   physics     0 PYB | 1 PYB_GND | 2 PYB_DRAG | 3 PYB_DW | 4 PYB_GND_DRAG_DW   (enums.py:12-21, BaseAviary.py:412-437;
     *               _downwash sums over OTHER drones of the same Bullet world, NUM_DRONES = 1 -> no force)
     *   action_type 0 THRUST (PBDroneEnv._preprocessAction) | 1 RPM | 2 PID | 3 VEL | 4 ONE_D_RPM | 5 ONE_D_PID
     *               (BaseSingleAgentAviary._preprocessAction, BaseSingleAgentAviary.py:176-222) */
    int32_t physics;
    int32_t action_type;
    /* N4: spawn every episode at a random point around a random track line (PBDroneEnv.py:622-627, dormant in the reference) */
    int32_t random_spawn;
    /* N4: p.changeDynamics(linearDamping=0, angularDamping=0), the line the reference keeps commented out (BaseAviary.py:571-573) */
    int32_t zero_damping;
} orc_config;

/* Every per-env variable the reference keeps, under the reference's names. */
typedef struct orc_env {
    /* Bullet rigid body (world frame), BaseAviary.py:596-598 */
    double pos[3], quat[4], vel[3], ang_v[3];
    double rpy[3];
    /* PBDroneEnv bookkeeping, PBDroneEnv.py:122-145 */
    double cur_pos[3];                          /* _current_position */
    double cur_vel[3], cur_ang_v[3];            /* current_vel, current_ang_v */
    double prev_vel[3], prev_ang_v[3];
    double d, d_prev;                           /* _distance_to_target, _prev_distance_to_target */
    int32_t idx;                                /* _current_target_index */
    int32_t just_found;
    int32_t is_done;                            /* _is_done */
    int32_t steps;                              /* _steps */
    /* SB3 Monitor */
    double ep_ret;
    int32_t ep_len;
    /* normalize.RunningMeanStd, normalize.py:10-31 */
    double rms_mean[ORC_OBS_DIM], rms_var[ORC_OBS_DIM], rms_count;
    /* noise counter (the vector-step counter, 64 bits: it enters the Philox counter whole) */
    uint64_t step_count;
    /* NormalizeReward (normalize.py:100-147): discounted return and its RunningMeanStd(shape=()) */
    double rr_returns, rr_mean, rr_var, rr_count;
    /* BaseAviary.last_clipped_action (BaseAviary.py:442,545): the rpm of the previous control step, zeros after reset */
    double last_clipped_action[4];
    /* DSLPIDControl state (ActionType.PID / VEL / ONE_D_PID): integral_pos_e, last_rpy, integral_rpy_e; never reset */
    double pid[9];
    /* random spawn: global env id (Philox counter word), this episode's INIT_XYZS[0] */
    uint64_t gid;
    double spawn_pt[3];
    int32_t spawn_ready;
} orc_env;

/* Result of one gym-level env.step (PBDroneEnv.step), before vectorisation. */
typedef struct orc_step_out {
    float obs[ORC_OBS_DIM];
    double reward;
    int32_t terminated, truncated, found_targets;
} orc_step_out;

/* ---- A1-A3: action chain, float32 ---------------------------------------- */
void orc_constants(double *out /* [16] */);
void orc_action_bounds(float *a_low, float *a_high);
void orc_rescale_action(const float a[4], float out[4]);
void orc_preprocess_action(const float thrust_cmd[4], float rpm[4]);
void orc_rotor_forces(const float rpm[4], float forces[4], float *z_torque);

/* ---- A4/A5: rigid body (UNPINNED, Bullet recall) ------------------------- */
void orc_bullet_step(double pos[3], double quat[4], double vel[3], double ang_v[3],
                     const double forces[4], double z_torque);
/* same, with an extra LINK_FRAME force on link 4 (centre of mass, BaseAviary._drag) */
void orc_bullet_step_ex(double pos[3], double quat[4], double vel[3], double ang_v[3],
                        const double forces[4], double z_torque, const double body_force[3]);

/* ---- N4: extra force terms and the RPM action type (python halves pinned: extra_physics.npz) ---- */
/* BaseSingleAgentAviary._preprocessAction, ActionType.RPM (BaseSingleAgentAviary.py:176-179) + BaseAviary._physics (:776-780) */
void orc_rpm_action(const float a[4], double rpm[4], double forces[4], double *z_torque);
/* BaseAviary._groundEffect (:800-832): the four forceObj z values, or zeros when the attitude test fails.
 * rpm_is_f32: the rpm array is float32 (THRUST chain) -> numpy works in float32 up to the (PROP_RADIUS/(4h))^2 factor */
void orc_ground_effect(const double pos[3], const double quat[4], const double rpy[3], const double rpm[4], int rpm_is_f32,
                       double out[4]);
/* BaseAviary._drag (:836-862): forceObj handed to link 4 */
void orc_drag(const double quat[4], const double vel[3], const double last_rpm[4], int rpm_is_f32, double out[3]);
void orc_bullet_step_damp(double pos[3], double quat[4], double vel[3], double ang_v[3],
                          const double forces[4], double z_torque, const double body_force[3], double damp);
void orc_euler_from_quat(const double q[4], double rpy[3]);
/* ActionType.PID (2) / VEL (3) / ONE_D_RPM (4) / ONE_D_PID (5): BaseSingleAgentAviary._preprocessAction (:180-222) with
 * DSLPIDControl.computeControl; st[9] = integral_pos_e, last_rpy, integral_rpy_e (python half pinned: pid_control.npz) */
/* position_generator.py:121-152 with the draws supplied; and the Philox-keyed draw of one episode's spawn point */
void orc_point_around_line(const double frm[3], const double to[3], double t, const double rv[3], double offset,
                           const double bounds[6], double out[3]);
void orc_random_spawn(const orc_config *cfg, uint64_t env_id, uint64_t step, double out[3]);
void orc_pid_control(int32_t action_type, const double pos[3], const double quat[4], const double vel[3],
                     const float action[4], double st[9], double rpm[4]);

/* ---- A6-A9: gym-level env -------------------------------------------------- */
void orc_env_construct(const orc_config *cfg, orc_env *e);
void orc_env_reset(const orc_config *cfg, orc_env *e, float obs[ORC_OBS_DIM]);
void orc_env_step(const orc_config *cfg, orc_env *e, const float action[4], orc_step_out *out);
/* pieces, exposed for the golden-vector tests */
void orc_compute_obs(const orc_config *cfg, const orc_env *e, float obs[ORC_OBS_DIM]);
double orc_compute_reward(const orc_config *cfg, orc_env *e);
int32_t orc_compute_terminated(const orc_config *cfg, const orc_env *e);
int32_t orc_compute_truncated(const orc_config *cfg, const orc_env *e);
int32_t orc_has_collision(const orc_config *cfg, const orc_env *e);
void orc_post_step(const orc_config *cfg, orc_env *e);
void orc_normalize_obs(orc_env *e, const float obs_in[ORC_OBS_DIM], double obs_out[ORC_OBS_DIM]);
/* TransformReward(clip) + NormalizeReward.step for one env (normalize.py:132-147); returns the reward Monitor sees */
double orc_reward_wrappers(const orc_config *cfg, orc_env *e, double reward, int32_t done);

/* ---- A10/A11: vectorised (SubprocVecEnv + Monitor + NormalizeObservation) --- */
void orc_vec_create(const orc_config *cfg, orc_env *envs, int64_t n);
void orc_vec_reset(const orc_config *cfg, orc_env *envs, int64_t n, float *obs /* [n,13] */, int threads);
void orc_vec_step(const orc_config *cfg, orc_env *envs, int64_t n, const float *actions /* [n,4] */,
                  float *obs /* [n,13] */, float *reward /* [n] */, uint8_t *done /* [n] */,
                  uint8_t *truncated /* [n] TimeLimit.truncated */, int32_t *found_targets /* [n] */,
                  float *terminal_obs /* [n,13] rows valid where done, may be NULL */,
                  float *ep_ret /* [n] valid where done, may be NULL */,
                  int32_t *ep_len /* [n] valid where done, may be NULL */,
                  uint8_t *terminated /* [n] raw terminated flag, may be NULL */,
                  int threads);

void orc_vec_refresh_rpy(orc_env *envs, int64_t n);   /* teacher-forcing helper: rpy cache <- quat */

/* ---- per-drone dynamics randomisation and wind (dn_enable_dynamics / dn_enable_wind; not in the reference) ----
 * Restated from the documented semantics (include/dronenav.h), not from the kernels.  Kept out of
 * orc_config / orc_env so that their layout, the golden replays and bench.py's cpu_baseline see what they saw before.
 *   body:  mass M s_m (linear acceleration, damping and PYB_DRAG force over M s_m; gravity stays g), inertia I s_I on all three
 *          axes (I w, gyroscopic term, damping), every rotor force after the action chain x s_kf (ground effect included, after
 *          it is added), the yaw torque x s_km.  Action chain, HOVER_RPM and DSLPIDControl stay nominal.
 *   wind:  F_w = (k_xy w_x, k_xy w_y, k_z w_z), w = wbar + g at step entry, world frame, centre of mass, over M s_m; after every
 *          physics step g <- float32(a g + b xi), xi = orc_noise4 on stream 15, a = exp(-dt / tau), b = sigma sqrt(1 - a^2) in float64.
 *   episode starts (orc_vec_reset_dw and the auto-reset of orc_vec_step_dw), keyed (seed; gid, the step the episode starts on,
 *          stream): resample -> new scales (ONE Philox call, stream 13), resample -> new wbar (stream 14); g = float32(sigma xi')
 *          with xi' on stream 16 (0 with the gust off), taken instead of that step's update. */
typedef struct orc_dw_config {
    int32_t dynamics;                           /* 1: the body scales of orc_dw_state.dyn act */
    int32_t dyn_resample;                       /* 1: draw new scales at every episode start */
    float dyn_lo[4], dyn_hi[4];                 /* ranges of (s_m, s_I, s_kf, s_km) */
    int32_t wind;                               /* 1: the wind of orc_dw_state acts */
    int32_t wind_resample;                      /* 1: draw a new steady wind at every episode start */
    float speed[2], azimuth[2], vertical[2];    /* ranges of the steady draw */
    float gust_sigma[2];                        /* stationary gust standard deviation (xy, z); (0, 0): no gust process */
    float gust_tau;                             /* gust correlation time, s */
    float coeff[2];                             /* (k_xy, k_z), N s / m */
} orc_dw_config;

typedef struct orc_dw_state {
    float dyn[4];                               /* s_m, s_I, s_kf, s_km */
    float wind_mean[4];                         /* wbar (x, y, z, 0) */
    float wind_gust[4];                         /* g (x, y, z, 0) */
} orc_dw_state;

/* one physics step with scaled mass and inertia and an extra WORLD-frame force at the centre of mass (may be NULL) */
void orc_bullet_step_dw(double pos[3], double quat[4], double vel[3], double ang_v[3], const double forces[4], double z_torque,
                        const double body_force[3], double damp, double mass_scale, double inertia_scale, const double world_force[3]);
/* orc_env_step with the body and wind of *s (dwc / s NULL: the nominal step) */
void orc_env_step_dw(const orc_config *cfg, const orc_dw_config *dwc, const orc_dw_state *s, orc_env *e, const float action[4],
                     orc_step_out *out);
/* the vec entry points with per-drone state dws[n]; dwc / dws NULL: exactly orc_vec_reset / orc_vec_step */
void orc_vec_reset_dw(const orc_config *cfg, const orc_dw_config *dwc, orc_dw_state *dws, orc_env *envs, int64_t n, float *obs,
                      int threads);
void orc_vec_step_dw(const orc_config *cfg, const orc_dw_config *dwc, orc_dw_state *dws, orc_env *envs, int64_t n,
                     const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *truncated, int32_t *found_targets,
                     float *terminal_obs, float *ep_ret, int32_t *ep_len, uint8_t *terminated, int threads);
int32_t orc_sizeof_dw_config(void);
int32_t orc_sizeof_dw_state(void);

/* ---- per-drone actuator model (dn_enable_actuator; not in the reference: its actuator is ideal) ----
 * Restated from the documented semantics (include/dronenav.h), not from the kernels; kept out of orc_config /
 * orc_env / orc_dw_* like the body and the wind.
 *   latency: at a vector step a drone enters with episode step counter s (orc_env.steps) the chain consumes the action commanded
 *            d vector steps ago if s >= d, else `fill`; the action noise of THIS vector step (stream 0) is added to what is consumed;
 *            after every vector step the history shifts by one and takes the COMMANDED action.
 *   lag:     ActionType.THRUST and a motor_tau range other than [0, 0]: c = the nominal float32 chain's speeds for the consumed action,
 *            r <- float32(a r + (1 - a) c) in float64 in that nesting; forces KF r^2, the yaw torque from KM r^2 (float32, as the chain
 *            forms them from c), the ground effect and last_clipped_action see r; s_kf / s_km scale what comes of it.  a = 0 gives c
 *            bit for bit.  motor_tau = [0, 0]: the nominal path, `coeff` not read, `rpm` only set at episode starts.
 *   episode starts (orc_vec_reset_act and the auto-reset of orc_vec_step_act): r = rpm_fill; with resample ONE Philox call keyed
 *            (seed; gid, the step the episode starts on, stream 17): d = lo + floor((hi - lo + 1) u_0) clamped to hi,
 *            tau = tau lo + (tau hi - tau lo) u_1, a = float32(exp(-dt / tau)), 0 where tau = 0.  The new a acts from the first step
 *            of the new episode; the terminal step has used the old one. */
#define ORC_MAX_LATENCY 8
typedef struct orc_act_config {
    int32_t on;                                 /* 1: the actuator of orc_act_state acts */
    int32_t latency[2];                         /* latency range [lo, hi], control steps, 0 <= lo <= hi <= ORC_MAX_LATENCY */
    float motor_tau[2];                         /* motor time constant range [lo, hi], s; [0, 0]: no lag */
    float fill[4];                              /* the action a fresh episode's pipeline holds */
    int32_t resample;                           /* 1: draw (d, a) at every episode start */
    float rpm_fill[4];                          /* the nominal chain's speeds for `fill` (orc_act_rpm_fill) */
} orc_act_config;

/* the per-drone layout dn_get_actuator returns, 152 bytes */
typedef struct orc_act_state {
    int32_t latency;                            /* d */
    float coeff;                                /* a */
    float rpm[4];                               /* r */
    float history[ORC_MAX_LATENCY][4];          /* history[j] = the action commanded j + 1 vector steps ago */
} orc_act_state;

/* rpm_fill <- orc_preprocess_action of `fill` (after orc_rescale_action when cfg->normalize_actions) */
void orc_act_rpm_fill(const orc_config *cfg, orc_act_config *actc);
/* the state after the first enable: d = 0, a = 0, r = rpm_fill, history = fill */
void orc_act_init(const orc_act_config *actc, orc_act_state *acts, int64_t n);
/* orc_env_step_dw with the motor lag of *as; `action` is the consumed action (actc / as NULL: orc_env_step_dw) */
void orc_env_step_act(const orc_config *cfg, const orc_dw_config *dwc, const orc_dw_state *s, const orc_act_config *actc,
                      orc_act_state *as, orc_env *e, const float action[4], orc_step_out *out);
/* the vec entry points with per-drone state acts[n]; actc / acts NULL: exactly orc_vec_reset_dw / orc_vec_step_dw */
void orc_vec_reset_act(const orc_config *cfg, const orc_dw_config *dwc, orc_dw_state *dws, const orc_act_config *actc,
                       orc_act_state *acts, orc_env *envs, int64_t n, float *obs, int threads);
void orc_vec_step_act(const orc_config *cfg, const orc_dw_config *dwc, orc_dw_state *dws, const orc_act_config *actc,
                      orc_act_state *acts, orc_env *envs, int64_t n, const float *actions, float *obs, float *reward, uint8_t *done,
                      uint8_t *truncated, int32_t *found_targets, float *terminal_obs, float *ep_ret, int32_t *ep_len,
                      uint8_t *terminated, int threads);
int32_t orc_sizeof_act_config(void);
int32_t orc_sizeof_act_state(void);

/* ---- per-drone sensor model (dn_enable_sensor; not in the reference: its observation is the state of this very step) ----
 * Restated from the documented semantics (include/dronenav.h), not from the kernels, and NOT as a ring keyed by the
 * vector step: the state is the logical one dn_get_sensor returns, shifted every step.  Kept out of orc_config / orc_env like the others.
 *   o_k:     the row BEFORE the normaliser (columns + observation noise) after the episode's k-th control step; o_0 the reset row.
 *   step:    o_k enters the history (history[0] = o_k, the rest move down), float32(o_{k - min(d, k)} + b) leaves, one float32 add per
 *            column and no add at all when the bias is off; it is terminal_obs when the step ends the episode.
 *   episode starts (orc_vec_reset_sens and the auto-reset of orc_vec_step_sens): with resample FOUR Philox calls keyed (seed; gid, the
 *            vector step the episode starts on, streams 18..21), u_m = (r_c + 0.5) / 2^32 with m = 4 q + c: b_j = float32(amp_j (2 u_j -
 *            1)) in float64, d = lo + floor((hi - lo + 1) u_13) clamped to hi; the history holds o_0 alone; float32(o_0 + b_new) leaves,
 *            undelayed.  resample = 0 keeps d and b, which are then always applied.
 *   the normaliser is fed the delivered rows, once each, where it was fed the true rows; nothing else reads them. */
#define ORC_SENS_HIST (ORC_MAX_LATENCY + 1)
typedef struct orc_sens_config {
    int32_t latency[2];                         /* dn_sensor_config, member for member (68 bytes) */
    float bias_amp[ORC_OBS_DIM];
    int32_t resample;
    int32_t reserved;
    int32_t lat_on;                             /* orc_sens_rule: the delay is applied and the history maintained */
    int32_t bias_on;                            /* orc_sens_rule: the bias is added; both 0 = the path without the sensor */
} orc_sens_config;

/* the per-drone arrays dn_get_sensor returns, 524 bytes */
typedef struct orc_sens_state {
    int32_t latency;                            /* d */
    float bias[ORC_OBS_DIM];                    /* b */
    float history[ORC_SENS_HIST][ORC_OBS_DIM];  /* history[j] = o_{k - j}, k = orc_env.steps; entries with k - j < 0 are never read */
} orc_sens_state;

/* lat_on / bias_on from the header's "off" rule: resample = 1: latency != [0, 0] / some amplitude > 0; resample = 0: both 1 */
void orc_sens_rule(orc_sens_config *sensc);
/* the state after the first enable: d = 0, b = 0, an all-zero history */
void orc_sens_init(const orc_sens_config *sensc, orc_sens_state *senss, int64_t n);
/* the sensor's part of one env step: row = o_k of the episode's k-th control step on entry, y_k on return */
void orc_env_step_sens(const orc_sens_config *sensc, orc_sens_state *ss, int32_t k, float row[ORC_OBS_DIM]);
/* the vec entry points with per-drone state senss[n]; sensc / senss NULL (or both flags 0): exactly orc_vec_reset_act / orc_vec_step_act */
void orc_vec_reset_sens(const orc_config *cfg, const orc_dw_config *dwc, orc_dw_state *dws, const orc_act_config *actc,
                        orc_act_state *acts, const orc_sens_config *sensc, orc_sens_state *senss, orc_env *envs, int64_t n, float *obs,
                        int threads);
void orc_vec_step_sens(const orc_config *cfg, const orc_dw_config *dwc, orc_dw_state *dws, const orc_act_config *actc,
                       orc_act_state *acts, const orc_sens_config *sensc, orc_sens_state *senss, orc_env *envs, int64_t n,
                       const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *truncated, int32_t *found_targets,
                       float *terminal_obs, float *ep_ret, int32_t *ep_len, uint8_t *terminated, int threads);
int32_t orc_sizeof_sens_config(void);
int32_t orc_sizeof_sens_state(void);

/* ---- N1: GAE (cleanRLPPO.py:234-248 + SB3 truncation bootstrap) ------------ */
void orc_gae(const float *rewards, const float *values, const uint8_t *dones,
             const float *last_values, const uint8_t *last_dones,
             int64_t n_steps, int64_t n_envs, double gamma, double lam,
             float *advantages, float *returns);

/* ---- noise: Philox4x32-10 counter RNG -------------------------------------- */
void orc_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                    uint32_t k0, uint32_t k1, uint32_t out[4]);
void orc_noise4(uint64_t seed, uint64_t env_id, uint64_t step, uint32_t stream, float out[4]);
void orc_noise4_many(uint64_t seed, uint64_t env_id0, int64_t n, uint64_t step, uint32_t stream, float *out);   /* [n][4] */

int32_t orc_sizeof_env(void);
int32_t orc_sizeof_config(void);
int32_t orc_max_threads(void);

#ifdef __cplusplus
}
#endif
#endif
