// dn_internal.h -- shared between the HIP kernels (dn_kernels.hip, dn_glue.hip) and the C-ABI host side (dn_capi.cpp, dn_capi_envfree.cpp).
#ifndef DN_INTERNAL_H
#define DN_INTERNAL_H

#include <hip/hip_runtime.h>
#ifdef __HIP__      // DN_KLAUNCH's hipExtLaunchKernelGGL: HIP translation units only (a plain C++ host compiler cannot parse the header)
#include <hip/hip_ext.h>
#endif
#include <stdint.h>

#include "../../include/dronenav.h"

// 64 drones per workgroup: N = 32768 drones is only 512 tiles, and 512 workgroups spread over all 256 CUs
// (2 per CU, block b -> XCD b % 8) where 128 workgroups of 256 drones would leave half the chip idle.  A
// workgroup is one wave (all phases) or two (flight wave + report wave over the same 64 drones).  Every
// wave-level idiom below (ballot, LDS tile transpose) assumes DN_BLOCK == 64.
#define DN_BLOCK 64

// Every device function of the step and glue units and of the headers they share (dn_action_chain.h, dn_philox.h, dn_policy_draw.h)
#define DN_DEV __device__ __forceinline__

// Layout of one waypoint-table entry (entry k describes waypoint k and the corridor segment that ends
// at it), staged into LDS once per workgroup.  Precomputed on the host in float64 with the reference's
// operation order (PBDroneEnv.is_out_of_cylinder_bounds, PBDroneEnv.py:746-786).
enum {
    DN_T_WP = 0,    // target_points[k]                         (3)
    DN_T_U = 3,     // line_unit_vec of segment k               (3)
    DN_T_E1 = 6,    // extended_point1 = base1 - 0.2*unit       (3)
    DN_T_B1 = 9,    // base1 (spawn for k = 0, else wp[k-1])    (3)
    DN_T_LEXT = 12, // ||extended_point2 - extended_point1||    (1)
    DN_T_LL = 13,   // line_length (0 -> degenerate segment)    (1)
    DN_T_STRIDE = 14
};

// Per-workgroup episode statistics slot (workgroup b always owns drones [64b, 64b+64), so its lane 0
// read-modify-writes the slot without atomics: deterministic, no contended counter).
// The slot also carries the tile's vector-step counter (the Philox counter word of the noise streams and the
// source of dn_stats.env_steps): it advances on the device, so launches replayed from a hipGraph keep counting.
struct DnStatSlot {
    long long episodes, truncated, completed, sum_len, sum_found, sum_ret_fix;
    unsigned long long step_count;
    long long pad_;
};

// Persistent state in HBM: "SoA of float4 groups" -- each group is an array of N float4, lane i reads
// 16 contiguous bytes at i*16 (1 KiB per wave instruction, the full-width coalesced access), instead
// of 26 separate dword arrays.  Field order inside a group is chosen so one drone's step touches six
// groups read + six written; g6 (stale _current_position) is touched only around resets.
struct DnState {
    float4 *g0;  // pos.xyz, d (_distance_to_target)
    float4 *g1;  // quat.xyzw
    float4 *g2;  // vel.xyz, d_prev
    float4 *g3;  // ang_v.xyz, meta bits: steps[0:24) | idx[24:31) | just_found[31]
    float4 *g4;  // prev_vel.xyz, ep_ret (Monitor)
    float4 *g5;  // prev_ang_v.xyz, ep_len bits (Monitor)
    float4 *g6;  // _current_position.xyz (valid while steps == 0; otherwise it equals pos), pad
    float4 *g7;  // BaseAviary.last_clipped_action (previous step's rpm); allocated with Physics.PYB_DRAG only, else NULL
    double *rms_mean;   // [13][N]  normalize.RunningMeanStd.mean
    double *rms_m2;     // [13][N]  RunningMeanStd.var x .count: the second moment (dn_kernels.hip normalize_obs_cols; dn_get_state returns var)
    double *rms_count;  // [N]
    double *rr;         // [4][N]  NormalizeReward: returns, return_rms.mean, .var, .count (norm_rew only)
    double *pid;        // [9][N]  DSLPIDControl: integral_pos_e, last_rpy, integral_rpy_e (action types PID / VEL / ONE_D_PID only)
    DnStatSlot *stats;  // [ceil(N/64)]
};

struct DnStepIO {
    const float *actions;
    float *obs;
    float *reward;
    uint8_t *done;
    uint8_t *truncated;
    int32_t *found_targets;
    float *terminal_obs;
    float *ep_return;
    int32_t *ep_length;
    unsigned long long *done_mask;
    // dn_step_sampled (single-step launches only): the action is drawn in the kernel from the policy's mean instead of read
    const float *mean;                 // [N][4] or nullptr (then `actions` is read)
    float *act_out;                    // [N][4] the sampled, UNclipped action (what SB3 stores in the rollout buffer)
    float *logp_out;                   // [N]    log N(action; mean, std) summed over the four dims
    float log_std[4];
    unsigned long long sample_seed;
    int sample_deterministic;
    int sample_squash;                 // dn_step_squashed: `mean` holds [N][8] rows (mu[4], log_std[4]); action = tanh(mu + sigma z)
};

// Scalars of the environment, in both precisions (the float32 build must not touch float64).
template <typename R>
struct DnConsts {
    R dim[6];
    R spawn[3];
    R threshold;
    R thr_ext;          // threshold + 0.2
    R thr2, thr_ext2;   // squares of the two radii: corridor tests compare squared distances (no sqrt)
    R max_target_dist;
    R inv_max_target_dist;
    R inv_dim[3];       // 1 / (x_high, y_high, z_high): position normalisation as a multiply
    R reset_obs[12];    // observation of the freshly spawned body (BaseAviary.reset, BaseAviary.py:318)
    float reset_obs32[12];   // ... as the float32 words the observation row carries (what the kernels read: half the scalar registers of
                             // the R values, and no float64 -> float32 conversion per column in the reset observation's normaliser pass)
};

struct DnParams {
    DnState st;
    long long n;
    int num_waypoints;
    int max_steps;
    int num_cus;                    // CUs of the device: tile b lands on a CU beside tile b + num_cus (role orders of the multi-wave kernels)
    int circle, cylinder, include_distance, normalize_actions, normalize_obs, ground_contact, clip_rew, norm_rew;
    int gnd, drag, rpm_actions;     // N4: Physics.PYB_GND / PYB_DRAG force terms, ActionType.RPM (1) / ONE_D_RPM (2)
    int pid_mode;                   // N4: 0, or the dn_config.action_type of the DSLPIDControl family: 2 PID | 3 VEL | 5 ONE_D_PID
    int random_spawn;               // N4: episodes start at a Philox-drawn point around a random track line
    int zero_damping;               // N4: changeDynamics(linearDamping=0, angularDamping=0), BaseAviary.py:571-573 (commented out there)
    float act_noise_sigma, obs_noise_sigma;
    int exact_obs_noise;            // DN_EXACT_OBS_NOISE=1 (read by dn_create): the observation-noise draws in the exact float64 form as well
    unsigned long long seed;
    long long env_id_offset;
    const double *tab64;   // [W][DN_T_STRIDE] float64 table
    const float *tab32;    // same, float32
    DnConsts<double> c64;
    DnConsts<float> c32;
};

// The per-drone models as one chain, shallowest first: the one statement of their order.  A step launch has ONE level, the deepest model
// that is on (dn_model_level below); the one-wave option kernel of level M (dn_step_many_1w_kernel<..., M>) carries every model up to M,
// each switched on or off at run time by its null pointers, and takes the first M slices of the argument chain
// DnDyn : DnWind : DnAct : DnSens : DnPriv : DnGoal + DnTrack (dn_kernels.hip StepArg) as its last argument.  DN_M_NONE is the plain kernel: that
// argument is an empty struct.  The structs below and MODELS[] (dn_capi.cpp) follow this order.
enum DnModelLevel { DN_M_NONE = 0, DN_M_DYN, DN_M_WIND, DN_M_ACT, DN_M_SENS, DN_M_PRIV, DN_M_GOAL, DN_M_COUNT };

// Per-drone dynamics randomisation (dn_enable_dynamics): the scale factors of the simulated body and how they are drawn.  Not a field of
// DnParams: DnParams is the first argument of every step kernel, and growing it would move every later kernel argument (a different
// instruction stream for every kernel).  It is the last argument of the kernels that read it: the one-wave step kernels of a level
// >= DN_M_DYN and the reset kernel.
struct DnDyn {
    float4 *dyn;            // [N] s_m, s_I, s_kf, s_km; nullptr = dynamics not enabled (the nominal cf2x body)
    float lo[4], hi[4];     // scale ranges of the draws, in the order of the float4
    int resample;           // 1: draw at every episode start (dn_reset, auto-reset); 0: keep what dn_set_dynamics wrote
    int pad_;
};

// Per-drone wind (dn_enable_wind): a steady part wbar drawn per episode and an Ornstein-Uhlenbeck gust g, both world frame, m/s.  Not a
// field of DnParams for the same reason as DnDyn; it travels with DnDyn in the last argument of the one-wave step kernels of a level
// >= DN_M_WIND and as the last argument of the reset kernel.
struct DnWind {
    float4 *mean;           // [N] wbar (x, y, z, 0); nullptr = wind not enabled
    float4 *gust;           // [N] g (x, y, z, 0): mean + N of the same allocation
    double a;               // exp(-dt / tau): the gust's one-step autocorrelation (float64 on the host, cast to R in the kernel)
    double b[2];            // sigma sqrt(1 - a^2), (xy, z)
    float speed[2], azimuth[2], vertical[2];    // ranges of the steady draw [lo, hi]
    float sigma[2];         // stationary gust standard deviation (xy, z)
    float k[2];             // force per unit wind speed (k_xy, k_z), N s / m
    int resample;           // 1: draw wbar at every episode start; 0: keep what dn_set_wind wrote
    int gust_on;            // sigma != (0, 0): launch-uniform; 0 = no draws, g held between episode starts and 0 from each
};

// Per-drone actuator model (dn_enable_actuator): command latency (an integer number of control steps) and a first-order motor lag on the
// rotor speeds.  Not a field of DnParams for the same reason as DnDyn; it travels behind DnDyn and DnWind in the last argument of the
// one-wave step kernels of a level >= DN_M_ACT and as the last argument of the reset kernel.  The four arrays are one allocation, hist first.
struct DnAct {
    float4 *hist;           // [N][8] hist[8 i + j] = the action commanded j + 1 vector steps ago; nullptr = actuator not enabled
    float4 *rpm;            // [N] effective rotor speeds r
    float *coeff;           // [N] a = exp(-dt / tau)
    int *lat;               // [N] latency d, control steps
    float4 fill;            // the action a fresh episode's pipeline holds
    float4 rpm_fill;        // the chain's speeds for `fill` (device-evaluated once by dn_enable_actuator): r at an episode start
    float tau[2];           // range of the time-constant draw [lo, hi], s
    int lat_lo, lat_hi;     // range of the latency draw
    int resample;           // 1: draw d and a at every episode start; 0: keep what dn_set_actuator wrote
    int lag_on;             // tau range != [0, 0]: launch-uniform; 0 = the filter is skipped (the nominal bits), coeff and rpm are not read
};

// Per-drone sensor model (dn_enable_sensor): the observation row delivered to the normaliser / the output is the pre-normaliser row of d
// control steps ago plus a per-episode bias.  Not a field of DnParams for the same reason as DnDyn; it travels behind DnDyn, DnWind and DnAct
// in the last argument of the one-wave step kernels of a level >= DN_M_SENS and as the last argument of the reset kernel.  The three arrays are one allocation, ring first: (16 * 64 + 64 + 4) = 1092 bytes per drone.
#define DN_SENS_SLOTS 16    // ring depth: a power of two >= DN_MAX_LATENCY + 1
struct DnSens {
    float4 *ring;           // [16][4][N]: quad q of the pre-bias row measured at vector step sc sits at ring[(((sc + base) & 15) * 4 + q) * N + i]
                            // (columns 13..15 of the last quad are padding); nullptr = sensor not enabled
    float4 *bias;           // [4][N]: quad q of drone i's bias row at bias[q * N + i]
    int *lat;               // [N] latency d, control steps
    float amp[13];          // bias amplitudes, observation-column units
    int lat_lo, lat_hi;     // range of the latency draw
    int resample;           // 1: draw d and b at every episode start; 0: keep what dn_set_sensor wrote
    int lat_on;             // launch-uniform: the delay is applied and the ring is maintained (latency != [0, 0], or resample = 0)
    int bias_on;            // launch-uniform: the bias is added (some amplitude > 0, or resample = 0)
    int base;               // host-side ring offset: dn_set_step_count moves it so that the slot of a vector step never changes
};

// Privileged observations (dn_enable_privileged): the true observation and the four models' current values, one row of DN_PRIV_DIM float32
// per drone and step, written by the step kernels of a level >= DN_M_PRIV (argument PrivArg = SensArg + DnPriv) and by the reset kernel.  It owns no memory: the rows are the caller's (dn_bind_privileged).
struct DnPriv {
    float *rows;            // [cap][N][DN_PRIV_DIM] step rows, step-major; nullptr = unbound (nothing is written)
    float *term;            // the terminal rows, same shape, or nullptr
    long long cap;          // steps the two buffers hold (host side: dn_step_many checks k against it)
    int groups;             // mask of DN_PRIV_*; 0 = the feature is not enabled
    int pad_;
};

// Goal observations (dn_enable_goal): the vector to the current target waypoint and the segment after it, one row of DN_GOAL_DIM float32
// per drone and step, written by the step kernels of level DN_M_GOAL (argument GoalArg = PrivArg + DnGoal) and by the reset kernel.  It owns no memory: the rows are the caller's (dn_bind_goal).
struct DnGoal {
    float *rows;            // [cap][N][DN_GOAL_DIM] step rows, step-major; nullptr = unbound (nothing is written)
    float *term;            // the terminal rows, same shape, or nullptr
    long long cap;          // steps the two buffers hold (host side: dn_step_many checks k against it)
    int frame;              // DN_GOAL_FRAME_WORLD / DN_GOAL_FRAME_BODY: launch-uniform
    int on;                 // 0 = the feature is not enabled
};

// Per-drone track bank (dn_enable_tracks): T tracks whose table rows sit one after the other in the corridor table the kernels stage into
// LDS (track t = rows base_t .. base_t + W_t - 1, track 0 first: the rows of dn_config), and each drone's track.  Not a level of its own:
// it rides in the DN_M_GOAL family (GoalArg = PrivArg + DnGoal + DnTrack) and is an argument of the reset kernel.  track and finished are
// one allocation, track first; cdf, bw and count follow them in it.
struct DnTrack {
    int *track;             // [N] the track of the drone's current episode; nullptr = the bank is off (one track: base 0, W = DnParams.num_waypoints)
    int *finished;          // [N] the track of its most recently ended episode, -1 before the first: track + N
    const double *cdf;      // [T] cumulative weights S_k / S_{T-1}, float64 partial sums of the float32 weights formed on the host
    const int *bw;          // [T] base_t | W_t << 8
    unsigned long long *count;  // [T][5] episodes, completed, truncated, sum of found_targets, sum of episode lengths, under the entry track
    int num_tracks;
    int total;              // rows of the whole bank: what stage_table stages
    int resample;           // 1: draw the track at every episode start; 0: keep what dn_set_tracks wrote
    int pad_;
};

// The per-drone models as the host carries them (dn_env, the launchers).  The kernels take them as before: the reset kernel as one argument
// each, the option step kernels as the slice of the chain (DnModelLevel above) their level reads.  A model that is off is its
// value-initialised struct (null pointers, groups 0, on 0).
struct DnModels {
    DnDyn dyn;
    DnWind wind;
    DnAct act;
    DnSens sens;
    DnPriv priv;
    DnGoal goal;
    DnTrack track;
};
// The level a step launch takes: the deepest model that is on.  The two row writers count only when enabled AND bound: unbound, nothing
// would be written, and the level below serves.  The track bank shares the deepest level, whatever the goal rows' binding: unbound, that
// family runs with null rows and writes none.
inline int dn_model_level(const DnModels &m)
{
    if (m.track.track || (m.goal.on && m.goal.rows)) return DN_M_GOAL;
    if (m.priv.groups && m.priv.rows) return DN_M_PRIV;
    if (m.sens.ring) return DN_M_SENS;
    if (m.act.hist) return DN_M_ACT;
    if (m.wind.mean) return DN_M_WIND;
    return m.dyn.dyn ? DN_M_DYN : DN_M_NONE;
}

// dn_set_launch_events (ABI 8): the step kernel of the next dn_step / dn_step_many launch is dispatched with these two hipEvents attached to
// its own dispatch packet (hipExtLaunchKernelGGL) -- they time the kernel itself, like a profiler's kernel trace, where a pair of
// hipEventRecord around the call would also time the host's launch path and add two marker packets to the stream.  One shot: the
// C ABI clears them after the launch.  Thread-local: a dn_env is driven from one host thread at a time (include/dronenav.h).
extern thread_local hipEvent_t dn_tl_ev_start, dn_tl_ev_stop;
#define DN_KLAUNCH(kern, grid, blk, shm, stream, ...)                                                                                   \
    do {                                                                                                                                \
        if (dn_tl_ev_start || dn_tl_ev_stop) hipExtLaunchKernelGGL(kern, grid, blk, shm, stream, dn_tl_ev_start, dn_tl_ev_stop, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, grid, blk, shm, stream, __VA_ARGS__);                                                             \
    } while (0)

int dn_norm_exact_compiled_in();      // 1 in libdronenav_exact.so (-DDN_NORM_EXACT=1: the normaliser's float64 output stage), else 0
// m: the per-drone models of the env.  With one of them on, the launch takes the one-wave option kernel of dn_model_level(*m) (the
// shallower models ride along, on or off), whatever `waves` says.
hipError_t dn_launch_step_many(const DnParams &p, const DnStepIO &io, int k, bool f32, int waves, hipStream_t stream, const DnModels *m = nullptr);
hipError_t dn_launch_step_many_mw(const DnParams &p, const DnStepIO &io, int k, bool f32, int waves, hipStream_t stream);   // dn_kernels_mw.hip
hipError_t dn_launch_reset(const DnParams &p, float *obs, bool f32, hipStream_t stream, const DnModels *m = nullptr);
// dn_set_sensor / dn_get_sensor: history[N][9][13] (logical order, history[i][j] = the row of j control steps ago) <-> the ring
hipError_t dn_launch_sensor_history(const DnParams &p, const DnSens &sn, float *history, int to_ring, hipStream_t stream);
// bias[N][13] <-> the quads
hipError_t dn_launch_sensor_bias(const DnSens &sn, long long n, float *bias, int to_dev, hipStream_t stream);
hipError_t dn_launch_eval_kinematics(const DnParams &p, const DnStepIO &io, const double *kin, bool f32, hipStream_t stream);
hipError_t dn_launch_gae(const float *rewards, const float *values, const uint8_t *dones,
                         const float *last_values, const uint8_t *last_dones, long long T, long long N,
                         float gamma, float gl, float *adv, float *ret, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_action_chain(const float *actions, long long n, int normalize_actions, float *rpm, float *forces,
                                  float *z_torque, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_fill4(float4 *dst, float4 v, long long n, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_filld(double *dst, double v, long long n, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_squashed_sample(const DnParams &p, const float *mu_log_std, unsigned long long seed, int deterministic,
                                     float *actions, float *log_prob, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_policy_sample(const DnParams &p, const float *mean, const float *log_std4, unsigned long long seed, int deterministic,
                                   float *actions, float *clipped, float *log_prob, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_add_bootstrap(float *reward, const float *terminal_value, const uint8_t *truncated, float gamma, long long n,
                                   hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_set_step_count(DnStatSlot *slots, long long blocks, unsigned long long value, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_mlp(const dn_mlp_net *nets, int num_nets, const float *obs, const uint8_t *row_mask, long long n, int obs_dim,
                         hipStream_t stream);
// Layer-1 K-steps (of 16 inputs) a PPO policy kernel runs for rows of obs_dim columns: 1 (the kernels of dn_mlp.hip), 2 or 4 (those of
// dn_mlp_wide.hip; there is no 3: 33..48 columns run 4 with zero fragments for the padding), 0 = refuse.  The SAC actor and
// dn_mlp_step_sampled take rows of KS1 = 1 only.
inline int dn_mlp_ks1(int obs_dim) { return obs_dim < 1 || obs_dim > 64 ? 0 : obs_dim <= 16 ? 1 : obs_dim <= 32 ? 2 : 4; }
// Width W of a history row (dn_stack_history): F observation frames of 13 columns, A action frames of 4 and E extra columns, padded with
// zeros to whole 16-byte quads; 0 = refuse (1 <= F <= 4, 0 <= A <= 4, E >= 0, and W <= 64, the widest row the policy kernels take).
inline int dn_history_row_width(int frames, int actions, int extra_dim)
{
    if (frames < 1 || frames > 4 || actions < 0 || actions > 4 || extra_dim < 0 || extra_dim > 64) return 0;
    const int w = (13 * frames + 4 * actions + extra_dim + 3) / 4 * 4;
    return w <= 64 ? w : 0;
}
hipError_t dn_launch_history(int frames, int actions, int extra_dim, long long k, long long n, const float *prev, const float *obs,
                             const float *act, const uint8_t *done, const float *term_obs, const float *extra, const float *term_extra,
                             float *rows, float *term_rows, hipStream_t stream);                                               // dn_history.hip
// Fleet-wide running normaliser of rows (dn_rownorm, dn_rownorm.hip).  The batch moments of a step are formed per block of
// DN_ROWNORM_BLOCK_ROWS consecutive rows -- a constant: the order of every float64 sum, and so every bit of the statistics, depends on
// (k, n, width) alone, never on the device or the launch shape.  The scratch is doubles only:
//   partials   [k][blocks(n)][2][width]   mean and sum of squared deviations of the block's rows, per column
//   snapshots  [k][2][width]              per step: the mean after the step's update and (a float32 held in a double) 1 / sqrt(var + eps)
// blocks(n) = ceil(n / DN_ROWNORM_BLOCK_ROWS).  0 = refuse (width outside 1..64, k or n < 1, or a size beyond 2^62 bytes).
constexpr long long DN_ROWNORM_BLOCK_ROWS = 1024;
constexpr int DN_ROWNORM_MAX_WIDTH = 64;
inline long long dn_rownorm_blocks(long long n) { return n < 1 ? 0 : (n - 1) / DN_ROWNORM_BLOCK_ROWS + 1; }
inline long long dn_rownorm_scratch_doubles(long long k, long long n, int width)
{
    if (width < 1 || width > DN_ROWNORM_MAX_WIDTH || k < 1 || n < 1) return 0;
    if (dn_rownorm_blocks(n) > (1ll << 50)) return 0;
    const long long per_step = (dn_rownorm_blocks(n) + 1) * 2 * width;         // < 2^58
    return k > (1ll << 59) / per_step ? 0 : k * per_step;
}
hipError_t dn_launch_rownorm_init(int width, double *stats, hipStream_t stream);                                             // dn_rownorm.hip
hipError_t dn_launch_rownorm(int width, float clip, double epsilon, double *stats, long long k, long long n, const float *rows, float *out,
                             int update, double *scratch, hipStream_t stream);                                                  // dn_rownorm.hip
// Fleet-wide running return normaliser of rewards (dn_retnorm, dn_retnorm.hip): one discounted return per drone and one RunningMeanStd of
// the returns over the fleet.  The batch moments of a step are formed per block of DN_ROWNORM_BLOCK_ROWS consecutive drones, the row
// normaliser's constant, so every bit of the statistics depends on (k, n) alone.  The scratch is doubles only:
//   partials   [k][blocks(n)][2]   mean and sum of squared deviations of the block's returns at that step
//   snapshots  [k][2]              per step: (a float32 held in a double) 1 / sqrt(var + eps) after the step's update, and one spare word
//                                  (between the merge's two passes the pair holds the step's batch mean and sum of squared deviations)
// 0 = refuse (k or n < 1, or a size beyond 2^62 bytes).  The scale launch takes DN_RETNORM_CHUNK rewards of one step per workgroup;
// dn_retnorm_grids_ok: both grids, blocks(n) and k chunks(n) workgroups, fit the 2^31 - 1 of a launch.
constexpr long long DN_RETNORM_CHUNK = 4096;
inline long long dn_retnorm_chunks(long long n) { return n < 1 ? 0 : (n - 1) / DN_RETNORM_CHUNK + 1; }
inline long long dn_retnorm_scratch_doubles(long long k, long long n)
{
    if (k < 1 || n < 1) return 0;
    const long long per_step = (dn_rownorm_blocks(n) + 1) * 2;                 // <= 2^54
    return k > (1ll << 59) / per_step ? 0 : k * per_step;
}
inline bool dn_retnorm_grids_ok(long long k, long long n)
{
    if (k < 1 || n < 1 || dn_rownorm_blocks(n) > 0x7fffffffll) return false;
    return k <= 0x7fffffffll / dn_retnorm_chunks(n);
}
hipError_t dn_launch_retnorm_init(double *stats, double *returns, long long n, hipStream_t stream);                           // dn_retnorm.hip
hipError_t dn_launch_retnorm(double gamma, double epsilon, float clip, double *stats, double *returns, long long k, long long n,
                             const float *rewards, const uint8_t *done, float *out, int update, double *scratch,
                             hipStream_t stream);                                                                               // dn_retnorm.hip
// PPO minibatches (dn_minibatch, dn_minibatch.hip): the gather of one minibatch's rows and the advantage normalisation.  The moments of
// the normalised field are formed per block of DN_ROWNORM_BLOCK_ROWS consecutive OUTPUT rows, the normalisers' constant, so every bit of
// them depends on `batch` alone.  The scratch is doubles only:
//   partials   [blocks(batch)][2]   mean and sum of squared deviations of the block's gathered values
//   result     [2]                  the minibatch's mean and std + epsilon
// 0 = refuse (batch < 1 or beyond the 2^31 - 1 samples of a buffer).
struct DnMinibatchArgs {
    dn_minibatch_field fields[DN_MINIBATCH_MAX_FIELDS];
    int num_fields, norm_field;                        // norm_field: the field to normalise, -1 = none (or batch == 1)
    unsigned long long seed, epoch;
    double eps;
    unsigned n_steps, n_envs, m, start, batch, nblk;    // nblk = blocks(batch)
    const long long *indices, *epoch_offset;
    long long *indices_out;
    double *part;
};
inline long long dn_minibatch_scratch_doubles(long long batch)
{
    return batch < 1 || batch > 0x7fffffffll ? 0 : (dn_rownorm_blocks(batch) + 1) * 2;
}
hipError_t dn_launch_minibatch(const DnMinibatchArgs &a, hipStream_t stream);                                                  // dn_minibatch.hip
// The PPO loss head (dn_ppo_loss, dn_ppo_loss.hip): per-row terms and gradients, and 4 + act_dim float64 sums formed per block of
// DN_ROWNORM_BLOCK_ROWS consecutive rows, the normalisers' constant, so every bit depends on (batch, act_dim) alone.  The scratch is
// doubles only:
//   part   [blocks(batch)][4 + act_dim]   the block's sums of min(p1, p2), (returns - vpred)^2, (ratio - 1) - lr, the clip indicator, and
//                                         g (z_j^2 - 1) per column
// 0 = refuse (act_dim outside 1..DN_PPO_MAX_ACT, batch < 1 or beyond 2^31 - 1 rows: the grid of a launch).
struct DnPpoLossArgs {
    const float *mean, *log_std, *value, *actions, *old_log_prob, *advantages, *returns, *old_values;   // old_values: NULL = no value clip
    float *d_mean, *d_log_std, *d_value, *log_prob_out, *loss;                                          // log_prob_out: NULL = not wanted
    double *stats, *part;
    double clip_range, clip_range_vf, ent_coef, vf_coef;
    long long batch, nblk;                             // nblk = blocks(batch)
    int act_dim, vec;                                  // vec: act_dim % 4 == 0 and mean, actions, d_mean are 16-byte aligned
};
inline long long dn_ppo_loss_scratch_doubles(long long batch, int act_dim)
{
    return act_dim < 1 || act_dim > DN_PPO_MAX_ACT || batch < 1 || batch > 0x7fffffffll ? 0 : dn_rownorm_blocks(batch) * (4 + act_dim);
}
hipError_t dn_launch_ppo_loss(const DnPpoLossArgs &a, hipStream_t stream);                                                     // dn_ppo_loss.hip
// The PPO optimiser step (dn_adam_step, dn_adam.hip): the global gradient norm, SB3's clip and Adam over up to DN_ADAM_MAX_TENSORS
// tensors.  Each tensor is cut into chunks of DN_ADAM_CHUNK consecutive elements (its last chunk is short: no chunk straddles two
// tensors), numbered tensor by tensor; a chunk is one workgroup.  The tensor table travels by value as a kernel argument.  The scratch is
// doubles only:
//   part   [chunks]   the chunk's float64 sum of g * g
// so the order of every float64 operation depends on the tensor counts alone.
struct DnAdamArgs {
    dn_adam_tensor t[DN_ADAM_MAX_TENSORS];
    const double *lr;                                  // device [1]
    double *state, *stats, *part;                      // device {step, c1, c2, 0}, {total, coef, lr, step'}, [nchunks]
    double beta1, beta2, eps, max_grad_norm;
    long long nchunks;                                 // sum over the tensors of dn_adam_chunks(count), <= 2^31 - 1: the grid of a launch
    int n_tensors, flags;                              // flags bit 0: zero the gradients after they are read
};
inline long long dn_adam_chunks(long long count) { return count < 1 ? 0 : (count - 1) / DN_ADAM_CHUNK + 1; }
hipError_t dn_launch_adam(const DnAdamArgs &a, hipStream_t stream);                                                            // dn_adam.hip
// SAC replay minibatches (dn_replay_sample, dn_replay.hip): one launch, grid (blocks of DN_REPLAY_BLOCK_ROWS output rows, 3 parts: obs,
// next_obs, and actions | reward | dones).  Everything is checked by the C ABI: 1 <= s, s + (skip >= 0) <= t, n, batch <= 2^31 - 1.
constexpr int DN_REPLAY_BLOCK_ROWS = 16;
struct DnReplayArgs {
    dn_replay_source src;
    float *obs, *next_obs, *actions, *rewards, *dones;
    const long long *indices, *draw_offset;            // NULL = the keyed draw; NULL = no offset
    long long *indices_out;                            // NULL = not wanted
    unsigned long long seed, draw;
    long long skip;                                    // -1 = none
    unsigned t, n, s, batch;
    int obs_dim, act_dim, ring;                        // ring: DN_REPLAY_RING
};
hipError_t dn_launch_replay(const DnReplayArgs &a, hipStream_t stream);                                                        // dn_replay.hip
// The SAC loss heads (dn_sac_policy, dn_sac_policy_backward, dn_sac_critic_loss, dn_sac_actor_loss; dn_sac_loss.hip).  The squashed
// policy head and its backward are one launch each, a row per lane, nothing reduced.  The two losses form float64 sums per block of
// DN_ROWNORM_BLOCK_ROWS consecutive rows, the normalisers' constant, so every bit depends on (batch, n_critics) alone.  The scratch is
// doubles only, and one size serves both losses:
//   part   [blocks(batch)][2 n_critics + 2]   critic: e_c^2 per critic, y, q_c per critic (2 n_critics + 1 used)
//                                             actor:  alpha lp - qmin, lp + target_entropy, lp, qmin (4 used)
// 0 = refuse (n_critics outside 1..DN_SAC_MAX_CRITICS, batch < 1 or beyond 2^31 - 1 rows).
struct DnSacPolicyArgs {
    const float *mean, *raw, *eps;                     // [batch][act_dim]; raw: the log_std head before the clamp
    const float *g_a, *g_lp;                           // backward: [batch][act_dim], [batch]; NULL = zero
    float *actions, *log_prob;                         // forward outputs
    float *d_mean, *d_raw;                             // backward outputs
    double lo, hi;                                     // log_std_min, log_std_max
    long long batch;
    int act_dim, vec;                                  // vec: act_dim % 4 == 0 and every [batch][act_dim] pointer of the call is 16-byte aligned
};
constexpr int DN_SAC_CRITIC = 0, DN_SAC_ACTOR = 1;
struct DnSacLossArgs {
    const float *q[DN_SAC_MAX_CRITICS];                // critic: q_c; actor: q_pi_c
    const float *next_q[DN_SAC_MAX_CRITICS];           // critic only
    float *d_q[DN_SAC_MAX_CRITICS];
    const float *next_log_prob, *rewards, *dones;      // critic only
    const float *log_prob;                             // actor only
    const float *log_ent_coef;                         // device [1]; NULL = the fixed ent_coef
    float *target_q;                                   // critic only
    float *d_log_prob, *d_log_ent_coef, *ent_coef_loss;   // actor only; d_log_ent_coef NULL with a fixed coefficient
    float *loss;                                       // critic_loss or actor_loss
    double *stats, *part;
    double gamma, target_entropy, ent_coef;
    long long batch, nblk;                             // nblk = blocks(batch)
    int n_critics, mode;                               // mode: DN_SAC_CRITIC or DN_SAC_ACTOR
};
inline long long dn_sac_loss_scratch_doubles(long long batch, int n_critics)
{
    return n_critics < 1 || n_critics > DN_SAC_MAX_CRITICS || batch < 1 || batch > 0x7fffffffll ? 0 : dn_rownorm_blocks(batch) * (2 * n_critics + 2);
}
hipError_t dn_launch_sac_policy(const DnSacPolicyArgs &a, bool backward, hipStream_t stream);                                  // dn_sac_loss.hip
hipError_t dn_launch_sac_loss(const DnSacLossArgs &a, hipStream_t stream);                                                     // dn_sac_loss.hip
// The training pass of the Tanh networks (dn_mlp_train_forward / _backward, dn_mlp_train.hip).  The scratch regions of the header, as
// byte offsets: h[l] and dz[l] for the hidden layers l < n_layers - 1, wpart[l] and bpart[l] for every layer.  The dimensions have
// passed the C ABI's checks: in <= 512, out <= 512, batch <= 2^24, so no product here comes near 2^63.
struct DnMlpTrainLayout {
    long long h[DN_MLP_TRAIN_MAX_LAYERS], dz[DN_MLP_TRAIN_MAX_LAYERS], wpart[DN_MLP_TRAIN_MAX_LAYERS], bpart[DN_MLP_TRAIN_MAX_LAYERS];
    long long chunks, total;
};
inline long long dn_mlp_train_chunks(long long batch) { return batch < 1 ? 0 : (batch - 1) / DN_MLP_TRAIN_CHUNK + 1; }
inline DnMlpTrainLayout dn_mlp_train_layout(const dn_mlp_train_layer *layers, int n_layers, long long batch)
{
    const auto r = [](long long b) { return (b + 255) / 256 * 256; };
    DnMlpTrainLayout lay = {};
    lay.chunks = dn_mlp_train_chunks(batch);
    long long at = 0;
    for (int l = 0; l < n_layers - 1; ++l) { lay.h[l] = at; at += r(4 * batch * layers[l].out_dim); }
    for (int l = 0; l < n_layers - 1; ++l) { lay.dz[l] = at; at += r(4 * batch * layers[l].out_dim); }
    for (int l = 0; l < n_layers; ++l) { lay.wpart[l] = at; at += r(4 * lay.chunks * layers[l].out_dim * layers[l].in_dim); }
    for (int l = 0; l < n_layers; ++l) { lay.bpart[l] = at; at += r(8 * lay.chunks * layers[l].out_dim); }
    lay.total = at;
    return lay;
}
struct DnMlpTrainArgs {
    dn_mlp_train_layer layer[DN_MLP_TRAIN_MAX_LAYERS];
    const float *x, *d_out;                            // d_out: backward only
    float *out, *d_x;                                  // out: forward only; d_x: backward only, NULL = not wanted
    char *scratch;
    long long batch;
    int n_layers, flags;
};
hipError_t dn_launch_mlp_train_forward(const DnMlpTrainArgs &a, hipStream_t stream);                                           // dn_mlp_train.hip
hipError_t dn_launch_mlp_train_backward(const DnMlpTrainArgs &a, hipStream_t stream);                                          // dn_mlp_train.hip
// The training pass of the SAC networks (dn_sac_train_forward / _backward, dn_sac_train.hip): n_nets networks of one shape.  A network's
// table entries are its hidden layers and then the parts of its head.  The scratch is n_nets consecutive blocks, network c at
// c * per_net, each block the regions of dn_mlp_train_layout for one network whose layer 0 reads in0 + in1 columns and whose head is its
// parts taken together: `one` holds a block's offsets.  The dimensions have passed the C ABI's checks.
constexpr int DN_SAC_TRAIN_MAX_ENTRIES = DN_MLP_TRAIN_MAX_LAYERS - 1 + DN_SAC_TRAIN_MAX_PARTS;
struct DnSacTrainLayout {
    DnMlpTrainLayout one;
    long long per_net, total;
};
inline DnSacTrainLayout dn_sac_train_layout(const dn_mlp_train_layer *net0, int n_nets, int n_layers, int head_parts, long long batch)
{
    dn_mlp_train_layer whole[DN_MLP_TRAIN_MAX_LAYERS] = {};
    for (int l = 0; l < n_layers - 1; ++l) { whole[l].in_dim = net0[l].in_dim; whole[l].out_dim = net0[l].out_dim; }
    whole[n_layers - 1].in_dim = net0[n_layers - 1].in_dim;
    for (int p = 0; p < head_parts; ++p) whole[n_layers - 1].out_dim += net0[n_layers - 1 + p].out_dim;
    DnSacTrainLayout lay = {};
    lay.one = dn_mlp_train_layout(whole, n_layers, batch);
    lay.per_net = lay.one.total;
    lay.total = lay.per_net * n_nets;
    return lay;
}
struct DnSacTrainArgs {
    dn_mlp_train_layer layer[DN_SAC_TRAIN_MAX_NETS][DN_SAC_TRAIN_MAX_ENTRIES];
    const float *x0, *x1;                              // x1 NULL with in1 = 0
    const float *d_out[DN_SAC_TRAIN_MAX_NETS][DN_SAC_TRAIN_MAX_PARTS];       // backward only
    float *out[DN_SAC_TRAIN_MAX_NETS][DN_SAC_TRAIN_MAX_PARTS];               // forward only
    float *d_x0, *d_x1;                                // backward only, NULL = not wanted
    char *scratch;
    long long batch;
    int n_nets, n_layers, head_parts, activation, in0, in1, flags;
};
hipError_t dn_launch_sac_train_forward(const DnSacTrainArgs &a, hipStream_t stream);                                           // dn_sac_train.hip
hipError_t dn_launch_sac_train_backward(const DnSacTrainArgs &a, hipStream_t stream);                                          // dn_sac_train.hip
// The Polyak update (dn_polyak_update, dn_sac_train.hip): one launch over a table that travels by value, grid y the tensor.
struct DnPolyakArgs {
    const float *source[DN_ADAM_MAX_TENSORS];
    float *target[DN_ADAM_MAX_TENSORS];
    long long count[DN_ADAM_MAX_TENSORS];
    double tau, omt;                                   // omt = 1.0 - tau, formed on the host
    int n_tensors;
};
hipError_t dn_launch_polyak(const DnPolyakArgs &a, hipStream_t stream);                                                        // dn_sac_train.hip
hipError_t dn_launch_mlp_wide(const dn_mlp_net *nets, int num_nets, const float *obs, const uint8_t *row_mask, long long n, int obs_dim,
                              hipStream_t stream);                                                                             // dn_mlp_wide.hip
hipError_t dn_launch_mlp_step(const DnParams &p, const DnStepIO &io, const dn_mlp_net *nets, int num_nets, const float *obs, int obs_dim,
                              hipStream_t stream);                                                                             // dn_fused.hip
hipError_t dn_launch_compact_pack(const unsigned long long *mask, long long n, const float *terminal_obs, const float *ep_return,
                                  const int32_t *ep_length, const uint8_t *truncated, const int32_t *found, int32_t *indices, int32_t *count,
                                  float *packed, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_stream_copy(void *dst, const void *src, long long n16, int num_cus, hipStream_t stream);   // dn_glue.hip
hipError_t dn_launch_compact(const unsigned long long *mask, long long n, int32_t *indices, int32_t *count,
                             hipStream_t stream);   // dn_glue.hip

// The LSTM layer (dn_lstm_forward / _backward, dn_lstm.hip).  The scratch regions of the header as byte offsets: the activated gates
// [T][B][4H] (the backward writes dZ over them), the two carries of the backward [B][H], the weight-gradient partials
// [chunks][4H][I + H] and the float64 bias partials [chunks][4H].  The forward uses the gates alone: the offset carry_h is the bytes it asks for.
// The dimensions have passed the C ABI's checks: I <= 64, H <= 512, T B <= 2^24, so no product here comes near 2^63.
#ifdef __HIP__
#define DN_LSTM_FN __host__ __device__ inline
#else
#define DN_LSTM_FN inline
#endif
constexpr int DN_LSTM_MAX_STEPS = 1024;
struct DnLstmLayout {
    long long gates, carry_h, carry_c, wpart, bpart;
    long long chunks, total;
};
inline DnLstmLayout dn_lstm_layout(int in_dim, int hidden, long long T, long long B)
{
    const auto r = [](long long b) { return (b + 255) / 256 * 256; };
    DnLstmLayout lay = {};
    lay.chunks = dn_mlp_train_chunks(T * B);
    long long at = 0;
    lay.gates = at; at += r(16 * T * B * hidden);
    lay.carry_h = at; at += r(4 * B * hidden);
    lay.carry_c = at; at += r(4 * B * hidden);
    lay.wpart = at; at += r(16 * lay.chunks * hidden * (in_dim + hidden));
    lay.bpart = at; at += r(32 * lay.chunks * hidden);
    lay.total = at;
    return lay;
}
// Where row t B + b of hprev, the recurrent input of step t, comes from: nowhere (+0.0) where the row's episode starts at t, else row b
// of h0 at t = 0 and row (t - 1) B + b of h_seq later.  c_prev follows the same rule with c0 and c_seq.
enum { DN_LSTM_PREV_NONE = 0, DN_LSTM_PREV_INITIAL = 1, DN_LSTM_PREV_SEQ = 2 };
struct DnLstmPrev {
    int source;
    long long row;
};
DN_LSTM_FN DnLstmPrev dn_lstm_prev(long long row, long long B, int episode_start)
{
    if (episode_start) return DnLstmPrev{DN_LSTM_PREV_NONE, 0};
    return row < B ? DnLstmPrev{DN_LSTM_PREV_INITIAL, row} : DnLstmPrev{DN_LSTM_PREV_SEQ, row - B};
}
#undef DN_LSTM_FN
struct DnLstmArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float *d_w_ih, *d_w_hh, *d_b_ih, *d_b_hh;          // backward only
    const float *x, *h0, *c0;
    const uint8_t *episode_starts;                     // [T][B], NULL = no episode starts inside the sequence
    float *h_seq, *c_seq;                              // written by the forward, read by the backward
    float *h_T, *c_T;                                  // forward only; may be h0 and c0
    const float *d_hseq;                               // backward only
    float *d_x;                                        // backward only, NULL = not wanted
    char *scratch;
    long long T, B;
    int in_dim, hidden, flags;
};
hipError_t dn_launch_lstm_forward(const DnLstmArgs &a, hipStream_t stream);                                                    // dn_lstm.hip
hipError_t dn_launch_lstm_backward(const DnLstmArgs &a, hipStream_t stream);                                                   // dn_lstm.hip

#endif
