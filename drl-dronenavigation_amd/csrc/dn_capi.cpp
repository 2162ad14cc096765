// dn_capi.cpp -- host side of the C ABI declared in include/dronenav.h.
//
// Owns the device arena, the waypoint/corridor tables and the launch parameters; every entry point
// validates its arguments, turns HIP failures into dn_status codes + a thread-local message, and
// never falls back to a CPU implementation.
#include "dn_argcheck.h"
#include "dn_capi_fail.h"
#include "dn_internal.h"
#include "dn_second_moment.h"
#include "dn_shapes.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

namespace {

thread_local char g_err[512] = "";

}  // namespace

int32_t fail(dn_status st, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return (int32_t)st;
}

namespace {

inline double norm3d(const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

constexpr double DN_CONTACT_MARGIN = 0.02;          // Bullet's contact-breaking threshold (dn_kernels.hip collision_common)
constexpr double DN_COLL_R = 0.06, DN_COLL_H = 0.025;   // base_link collision cylinder, cf2x.urdf:34

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// An on / off environment switch read by dn_create: 1 / 0, or -1 for a value that is neither (the create then fails: a typo
// must not silently select the other arithmetic).  Unset or empty = off.
int env_switch(const char *name)
{
    const char *x = getenv(name);
    if (!x || !x[0]) return 0;
    char b[8] = "";
    size_t k = 0;
    for (; x[k] && k < sizeof b - 1; ++k) b[k] = (char)((x[k] >= 'A' && x[k] <= 'Z') ? x[k] - 'A' + 'a' : x[k]);
    if (x[k]) return -1;
    if (!strcmp(b, "1") || !strcmp(b, "true") || !strcmp(b, "on") || !strcmp(b, "yes")) return 1;
    if (!strcmp(b, "0") || !strcmp(b, "false") || !strcmp(b, "off") || !strcmp(b, "no")) return 0;
    return -1;
}

}  // namespace

struct dn_env {
    dn_config cfg;
    DnParams p;
    void *arena = nullptr;
    size_t arena_bytes = 0;
    double *tab64 = nullptr;
    float *tab32 = nullptr;
    long long blocks = 0;
    int num_cus = (int)DN_CALIBRATION_CUS;   // hipDeviceProp_t.multiProcessorCount of cfg.device_id
    DnShapes picked = {2, 1};   // dn_create's pick (dn_shapes.h); what a launch takes is kernel_shapes(env), which the models overrule
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // dn_set_launch_events: attached to the next step kernel's dispatch, then cleared
    // dn_enable_*: each model's arrays are one allocation of its own, outside the arena (dn_state_bytes is unchanged): 16 bytes per drone
    // for the dynamics, 32 for the wind, 152 for the actuator, 1092 for the sensor model.  MODELS below names the pointer that owns each.
    DnModels m = {};
    dn_dynamics_config dyn_cfg = {};
    dn_wind_config wind_cfg = {};
    dn_actuator_config act_cfg = {};
    dn_sensor_config sens_cfg = {};
    dn_privileged_config priv_cfg = {};
    dn_goal_config goal_cfg = {};
    dn_track_bank_config track_cfg = {};
    bool ground_contact_auto = false;   // created with DN_GROUND_CONTACT_AUTO: dn_enable_tracks resolves the term again over the bank
};

thread_local hipEvent_t dn_tl_ev_start = nullptr, dn_tl_ev_stop = nullptr;

// Takes the events dn_set_launch_events armed: constructed FIRST THING in every step-family entry point, so that the call they were
// armed for consumes them (the hooked launches) or drops them (a validation failure, an entry point without the hook) -- they never
// survive into a later call, whose caller may have destroyed them by then.  Nests (dn_step_many(k = 1) -> dn_step).
thread_local int dn_tl_ev_depth = 0;
struct LaunchEvents {
    explicit LaunchEvents(dn_env *e)
    {
        if (dn_tl_ev_depth++ == 0) { dn_tl_ev_start = e->ev_start; dn_tl_ev_stop = e->ev_stop; }
        e->ev_start = e->ev_stop = nullptr;
    }
    ~LaunchEvents() { if (--dn_tl_ev_depth == 0) dn_tl_ev_start = dn_tl_ev_stop = nullptr; }
    LaunchEvents(const LaunchEvents &) = delete;
    LaunchEvents &operator=(const LaunchEvents &) = delete;
};
// an armed launch inside a stream capture would record the events into the graph (undefined on replay): refused
static bool armed_while_capturing(hipStream_t stream)
{
    if (!dn_tl_ev_start && !dn_tl_ev_stop) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
#define DN_REFUSE_ARMED_CAPTURE(stream)                                                                                           \
    do {                                                                                                                          \
        if (armed_while_capturing((hipStream_t)(stream)))                                                                         \
            return fail(DN_ERR_INVALID_ARGUMENT, "dn_set_launch_events: an armed launch cannot be captured into a hipGraph");     \
    } while (0)

namespace {

// Device arena: seven float4 groups, optional normaliser statistics, statistics slots, tables.
struct Layout {
    size_t off_g[7], off_g7, off_mean, off_var, off_count, off_rr, off_pid, off_stats, off_tab64, off_tab32, total;
};

Layout make_layout(long long n, int normalize_obs, int norm_rew = 0, int drag = 0, int pid = 0)
{
    Layout L;
    size_t o = 0;
    for (int k = 0; k < 7; ++k) { L.off_g[k] = o; o = align_up(o + (size_t)n * sizeof(float4), 256); }
    L.off_mean = o;  o = align_up(o + (normalize_obs ? (size_t)n * DN_OBS_DIM * sizeof(double) : 0), 256);
    L.off_var = o;   o = align_up(o + (normalize_obs ? (size_t)n * DN_OBS_DIM * sizeof(double) : 0), 256);
    L.off_count = o; o = align_up(o + (normalize_obs ? (size_t)n * sizeof(double) : 0), 256);
    L.off_rr = o;    o = align_up(o + (norm_rew ? (size_t)n * 4 * sizeof(double) : 0), 256);
    L.off_g7 = o;    o = align_up(o + (drag ? (size_t)n * sizeof(float4) : 0), 256);
    L.off_pid = o;   o = align_up(o + (pid ? (size_t)n * 9 * sizeof(double) : 0), 256);
    L.off_stats = o; o = align_up(o + (size_t)((n + DN_BLOCK - 1) / DN_BLOCK) * sizeof(DnStatSlot), 256);
    L.off_tab64 = o; o = align_up(o + DN_MAX_WAYPOINTS * DN_T_STRIDE * sizeof(double), 256);
    L.off_tab32 = o; o = align_up(o + DN_MAX_WAYPOINTS * DN_T_STRIDE * sizeof(float), 256);
    L.total = o;
    return L;
}

// Corridor table, float64, in the reference's operation order (PBDroneEnv.py:746-786).
void build_table(const dn_config &c, double *tab)
{
    const double ext = 0.2;
    for (int k = 0; k < c.num_waypoints; ++k) {
        double *e = tab + k * DN_T_STRIDE;
        const double *b1 = (k == 0) ? c.spawn : &c.waypoints[3 * (k - 1)];
        const double *b2 = &c.waypoints[3 * k];
        double lv[3] = {b2[0] - b1[0], b2[1] - b1[1], b2[2] - b1[2]};
        double ll = norm3d(lv);
        for (int j = 0; j < 3; ++j) { e[DN_T_WP + j] = b2[j]; e[DN_T_B1 + j] = b1[j]; }
        e[DN_T_LL] = ll;
        if (ll == 0.0) {
            for (int j = 0; j < 3; ++j) { e[DN_T_U + j] = 0.0; e[DN_T_E1 + j] = b1[j]; }
            e[DN_T_LEXT] = 0.0;
            continue;
        }
        double u[3] = {lv[0] / ll, lv[1] / ll, lv[2] / ll};
        double e1[3] = {b1[0] - ext * u[0], b1[1] - ext * u[1], b1[2] - ext * u[2]};
        double e2[3] = {b2[0] + ext * u[0], b2[1] + ext * u[1], b2[2] + ext * u[2]};
        double ee[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
        for (int j = 0; j < 3; ++j) { e[DN_T_U + j] = u[j]; e[DN_T_E1 + j] = e1[j]; }
        e[DN_T_LEXT] = norm3d(ee);
    }
}

template <typename R>
void build_consts(const dn_config &c, DnConsts<R> &k)
{
    for (int j = 0; j < 6; ++j) k.dim[j] = (R)c.aviary_dim[j];
    for (int j = 0; j < 3; ++j) k.spawn[j] = (R)c.spawn[j];
    k.threshold = (R)c.threshold;
    k.thr_ext = (R)(c.threshold + 0.2);
    k.thr2 = (R)(c.threshold * c.threshold);
    k.thr_ext2 = (R)((c.threshold + 0.2) * (c.threshold + 0.2));
    double a = std::fabs(c.aviary_dim[0]) + c.aviary_dim[3], b = std::fabs(c.aviary_dim[1]) + c.aviary_dim[4];
    double m = a > b ? a : b;
    k.max_target_dist = (R)(m > c.aviary_dim[5] ? m : c.aviary_dim[5]);           // PBDroneEnv.py:91
    k.inv_max_target_dist = (R)1.0 / k.max_target_dist;
    for (int j = 0; j < 3; ++j) k.inv_dim[j] = (R)1.0 / k.dim[3 + j];
    // BaseAviary.reset -> _computeObs on the freshly loaded body: pos = spawn, quat = (0,0,0,1), at rest.
    // getEulerFromQuaternion(identity) = (atan2(0,1), asin(-0.0), atan2(0,1)) = (0, -0, 0).
    const R pi = (R)3.14159265358979323846;
    k.reset_obs[0] = k.spawn[0] / k.dim[3];
    k.reset_obs[1] = k.spawn[1] / k.dim[4];
    k.reset_obs[2] = k.spawn[2] / k.dim[5];
    k.reset_obs[3] = (R)0.0 / pi;
    k.reset_obs[4] = (R)-0.0 / pi;
    k.reset_obs[5] = (R)0.0 / pi;
    for (int j = 6; j < 12; ++j) k.reset_obs[j] = (R)0.0;
    for (int j = 0; j < 12; ++j) k.reset_obs32[j] = (float)k.reset_obs[j];
}

int32_t validate(const dn_config *c)
{
    if (!c) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (c->num_envs < 1) return fail(DN_ERR_INVALID_ARGUMENT, "num_envs must be >= 1 (got %lld)", (long long)c->num_envs);
    if (c->num_envs > (1ll << 31) - 64) return fail(DN_ERR_INVALID_ARGUMENT, "num_envs too large (got %lld)", (long long)c->num_envs);
    if (c->num_waypoints < 1 || c->num_waypoints > DN_MAX_WAYPOINTS)
        return fail(DN_ERR_INVALID_ARGUMENT, "num_waypoints must be in 1..%d (got %d)", DN_MAX_WAYPOINTS, c->num_waypoints);
    if (c->max_steps < 0 || c->max_steps > (1 << 24) - 2)
        return fail(DN_ERR_INVALID_ARGUMENT, "max_steps must be in 0..%d (got %d)", (1 << 24) - 2, c->max_steps);
    if (!(c->threshold >= 0.0)) return fail(DN_ERR_INVALID_ARGUMENT, "threshold must be >= 0");
    for (int j = 0; j < 3; ++j)
        if (!(c->aviary_dim[3 + j] != 0.0)) return fail(DN_ERR_INVALID_ARGUMENT, "aviary_dim high bounds must be non-zero");
    if (c->act_noise_sigma < 0.0f || c->obs_noise_sigma < 0.0f) return fail(DN_ERR_INVALID_ARGUMENT, "noise sigma must be >= 0");
    if (c->ground_contact < 0 || c->ground_contact > DN_GROUND_CONTACT_AUTO)
        return fail(DN_ERR_INVALID_ARGUMENT, "ground_contact must be 0 (off), 1 (on) or 2 (DN_GROUND_CONTACT_AUTO; got %d)", c->ground_contact);
    if (c->physics < 0 || c->physics > 4) return fail(DN_ERR_INVALID_ARGUMENT, "physics must be 0..4 (PYB, PYB_GND, PYB_DRAG, PYB_DW, PYB_GND_DRAG_DW; got %d)", c->physics);
    if (c->action_type < 0 || c->action_type > 5)
        return fail(DN_ERR_INVALID_ARGUMENT, "action_type must be 0 THRUST | 1 RPM | 2 PID | 3 VEL | 4 ONE_D_RPM | 5 ONE_D_PID (got %d)", c->action_type);
    for (int j = 0; j < c->num_waypoints * 3; ++j)
        if (!std::isfinite(c->waypoints[j])) return fail(DN_ERR_INVALID_ARGUMENT, "waypoint %d is not finite", j / 3);
    return DN_OK;
}

// DN_GROUND_CONTACT_AUTO: is the ground-contact term of _has_collision_occurred (PBDroneEnv.py:699) reachable at all?
// The approximated contact fires when the lowest point of the collision cylinder is within the contact margin of z = 0, i.e.
// only for z <= margin + max over tilt of (H/2 |c| + R s) = margin + sqrt(H^2/4 + R^2).  Every other term of the same
// predicate is evaluated on the same fresh position (:678-707), so if the corridor test is on and every point that low is
// already outside the corridor of EVERY segment (a drone is only ever tested against the segment of its current target), the
// term can never change `terminated`: the predicate is an OR.  Then it is dropped (and the kernels built without it are used);
// otherwise -- corridor off, or a track whose corridor reaches down to the floor (spawn / gates at z = 0.1 ... 0.5 with the
// 0.3 + 0.2 corridor) -- it stays on, as in the reference, which always has it.
bool ground_contact_reachable(const dn_config &c)
{
    if (!c.cylinder) return true;                                      // no corridor: nothing else keeps a drone off the floor
    // random_spawn: segment 0 then starts at this episode's drawn spawn point (rules_commit / dn_reset_kernel), which may sit up to 0.1
    // below the lowest waypoint -- the bound below, on the fixed spawn, does not cover it.  The option is dormant in the reference
    // (PBDroneEnv.py:622-627); keep the term, as the reference does.
    if (c.random_spawn) return true;
    const double z_contact = DN_CONTACT_MARGIN + std::sqrt(0.25 * DN_COLL_H * DN_COLL_H + DN_COLL_R * DN_COLL_R);
    double z_min;                                                       // lowest z inside any corridor
    if (c.circle) z_min = 1.0 - c.threshold;                            // torus around the unit circle at z = 1 (:723-741)
    else {
        z_min = 1e300;
        for (int k = 0; k < c.num_waypoints; ++k) {
            const double *b1 = (k == 0) ? c.spawn : &c.waypoints[3 * (k - 1)];
            const double *b2 = &c.waypoints[3 * k];
            const double lv[3] = {b2[0] - b1[0], b2[1] - b1[1], b2[2] - b1[2]};
            const double ll = norm3d(lv);
            double lo;
            if (ll == 0.0) lo = b1[2] - c.threshold;                    // degenerate segment: a ball of the bare threshold (:756-757)
            else {
                const double uz = lv[2] / ll;                           // capsule around the segment extended by 0.2 at both ends
                const double e1z = b1[2] - 0.2 * uz, e2z = b2[2] + 0.2 * uz;
                lo = (e1z < e2z ? e1z : e2z) - (c.threshold + 0.2);
            }
            if (lo < z_min) z_min = lo;
        }
    }
    return !(z_min > z_contact + 1e-9);
}

int32_t init_state_rms(dn_env *e, hipStream_t s)
{   // normalize.RunningMeanStd.__init__, normalize.py:14-18
    const long long n = e->cfg.num_envs;
    DN_HIP(dn_launch_filld(e->p.st.rms_mean, 0.0, n * DN_OBS_DIM, s));
    DN_HIP(dn_launch_filld(e->p.st.rms_m2, 1.0 * 1e-4, n * DN_OBS_DIM, s));     // var = 1, held as the second moment var x count
    DN_HIP(dn_launch_filld(e->p.st.rms_count, 1e-4, n, s));
    return DN_OK;
}

int32_t init_state(dn_env *e, hipStream_t s)
{
    const dn_config &c = e->cfg;
    const long long n = c.num_envs;
    // PBDroneEnv.__init__ (PBDroneEnv.py:122-145) followed by make_env's env.reset (PBDroneSimulator.py:173)
    double df[3] = {c.spawn[0] - c.waypoints[0], c.spawn[1] - c.waypoints[1], c.spawn[2] - c.waypoints[2]};
    const float d = (float)norm3d(df);
    const float sx = (float)c.spawn[0], sy = (float)c.spawn[1], sz = (float)c.spawn[2];
    DN_HIP(dn_launch_fill4(e->p.st.g0, make_float4(sx, sy, sz, d), n, s));
    DN_HIP(dn_launch_fill4(e->p.st.g1, make_float4(0.f, 0.f, 0.f, 1.f), n, s));
    DN_HIP(dn_launch_fill4(e->p.st.g2, make_float4(0.f, 0.f, 0.f, d), n, s));
    DN_HIP(dn_launch_fill4(e->p.st.g3, make_float4(0.f, 0.f, 0.f, 0.f), n, s));
    DN_HIP(dn_launch_fill4(e->p.st.g4, make_float4(0.f, 0.f, 0.f, 0.f), n, s));
    DN_HIP(dn_launch_fill4(e->p.st.g5, make_float4(0.f, 0.f, 0.f, 0.f), n, s));
    DN_HIP(dn_launch_fill4(e->p.st.g6, make_float4(sx, sy, sz, 0.f), n, s));
    if (c.normalize_obs) { int32_t rc = init_state_rms(e, s); if (rc != DN_OK) return rc; }
    if (c.norm_rew) {                              // NormalizeReward.__init__, normalize.py:124-128
        DN_HIP(dn_launch_filld(e->p.st.rr, 0.0, 2 * n, s));            // returns, return_rms.mean
        DN_HIP(dn_launch_filld(e->p.st.rr + 2 * n, 1.0, n, s));        // .var
        DN_HIP(dn_launch_filld(e->p.st.rr + 3 * n, 1e-4, n, s));       // .count
    }
    if (e->p.drag) DN_HIP(dn_launch_fill4(e->p.st.g7, make_float4(0.f, 0.f, 0.f, 0.f), n, s));   // BaseAviary.py:545
    if (e->p.pid_mode) DN_HIP(dn_launch_filld(e->p.st.pid, 0.0, 9 * n, s));                       // DSLPIDControl.reset(), DSLPIDControl.py:63-76
    DN_HIP(hipMemsetAsync(e->p.st.stats, 0, (size_t)e->blocks * sizeof(DnStatSlot), s));
    return DN_OK;
}

// The per-drone models, one row per DnModelLevel above DN_M_NONE and in its order (dn_internal.h).  dn_destroy and the entry points that
// carry none of them walk this table; a new model is one more level and one more row.  The track bank is a row without a level of its
// own: it shares the deepest one (dn_internal.h dn_model_level).
struct ModelRow {
    int level;
    void *(*slot)(const DnModels &);    // the pointer that owns the model's allocation, nullptr where it owns none
    bool (*on)(const DnModels &);
    const char *phrase, *enable;    // how a refusal names the model, and the entry point that turns it on
    const char *replay;             // what dn_eval_kinematics does that the model would falsify
};
constexpr ModelRow MODELS[] = {
    {DN_M_DYN, [](const DnModels &m) -> void * { return m.dyn.dyn; }, [](const DnModels &m) { return m.dyn.dyn != nullptr; }, "the randomised dynamics",
     "dn_enable_dynamics", "replays a given nominal-body transition"},
    {DN_M_WIND, [](const DnModels &m) -> void * { return m.wind.mean; }, [](const DnModels &m) { return m.wind.mean != nullptr; }, "the wind", "dn_enable_wind",
     "replays a given still-air transition"},
    {DN_M_ACT, [](const DnModels &m) -> void * { return m.act.hist; }, [](const DnModels &m) { return m.act.hist != nullptr; }, "the actuator model",
     "dn_enable_actuator", "replays a given transition"},
    {DN_M_SENS, [](const DnModels &m) -> void * { return m.sens.ring; }, [](const DnModels &m) { return m.sens.ring != nullptr; }, "the sensor model",
     "dn_enable_sensor", "reports the observation of the given transition"},
    // the rows are the caller's memory: nothing to free
    {DN_M_PRIV, [](const DnModels &) -> void * { return nullptr; }, [](const DnModels &m) { return m.priv.groups != 0; }, "the privileged observations",
     "dn_enable_privileged", "writes no privileged rows"},
    {DN_M_GOAL, [](const DnModels &) -> void * { return nullptr; }, [](const DnModels &m) { return m.goal.on != 0; }, "the goal observations", "dn_enable_goal",
     "writes no goal rows"},
    {DN_M_GOAL, [](const DnModels &m) -> void * { return m.track.track; }, [](const DnModels &m) { return m.track.track != nullptr; }, "the track bank",
     "dn_enable_tracks", "flies the one track of dn_config"},
};
constexpr int NUM_MODELS = (int)(sizeof MODELS / sizeof MODELS[0]);
// row k carries level k + 1, and the rows past the last level (the track bank) share it
constexpr bool models_follow_levels(int k = 0)
{
    return k == NUM_MODELS || (MODELS[k].level == (k + 1 < DN_M_COUNT ? k + 1 : DN_M_COUNT - 1) && models_follow_levels(k + 1));
}
static_assert(NUM_MODELS == DN_M_COUNT && models_follow_levels(),
              "MODELS[]: one row per DnModelLevel, in its order, then the track bank, which shares the deepest level");

// DN_OK, or the refusal of entry point `who`, whose kernels carry no model, for the first model that is on.  `instead` names the calls
// that do carry it; nullptr = dn_eval_kinematics, which has a reason per model and no alternative.
int32_t refuse_models(dn_env *env, const char *who, const char *instead)
{
    for (const ModelRow &r : MODELS) {
        if (!r.on(env->m)) continue;
        if (!instead) return fail(DN_ERR_INVALID_ARGUMENT, "%s %s: refused with %s (%s)", who, r.replay, r.phrase, r.enable);
        return fail(DN_ERR_INVALID_ARGUMENT, "%s does not carry %s (%s); %s", who, r.phrase, r.enable, instead);
    }
    return DN_OK;
}

// The kernel shapes a launch of this env takes: dn_create's pick, unless a model is on -- the models live in the one-wave option kernels
// only (as the random spawn does).  On by the row's own predicate, not by dn_model_level: privileged or goal rows that are enabled but
// unbound write nothing and still fly the one-wave kernels.
DnShapes kernel_shapes(const dn_env *env)
{
    for (const ModelRow &r : MODELS)
        if (r.on(env->m)) return {1, 1};
    return env->picked;
}

// The DnStepIO of every step-family entry point, every field set.  Without a sampler (mean, act_out and logp_out null) the kernels read
// `actions`; dn_mlp_step_sampled draws from the mean its policy kernel holds in registers, so it passes act_out / logp_out without `mean`.
DnStepIO make_io(const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *truncated, int32_t *found_targets, float *terminal_obs,
                 float *ep_return, int32_t *ep_length, uint64_t *done_mask, const float *mean = nullptr, float *act_out = nullptr,
                 float *logp_out = nullptr, const float *log_std = nullptr, uint64_t seed = 0, int32_t deterministic = 0, int squash = 0)
{
    DnStepIO io;
    io.actions = actions; io.obs = obs; io.reward = reward; io.done = done; io.truncated = truncated;
    io.found_targets = found_targets; io.terminal_obs = terminal_obs; io.ep_return = ep_return;
    io.ep_length = ep_length; io.done_mask = (unsigned long long *)done_mask;
    io.mean = mean; io.act_out = act_out; io.logp_out = logp_out;
    for (int j = 0; j < 4; ++j) io.log_std[j] = log_std ? log_std[j] : 0.0f;
    io.sample_seed = seed; io.sample_deterministic = deterministic != 0; io.sample_squash = squash;
    return io;
}

// dn_step_sampled and dn_step_squashed: one body.  The caller names what differs: the rows the sampler reads (`src`: the means, or the
// mu | log_std rows, which carry log_std themselves and ask for the squashed action: make_io), whether every pointer ITS signature
// requires is there, and the words of its refusals.
struct SamplerWords { const char *who, *src, *required, *instead; };     // the entry point, its name for `src`, its required pointers as its message lists them, the calls that serve what it refuses
int32_t sampler_step(dn_env *env, const SamplerWords &w, bool given, const float *src, const float *log_std, int squash, uint64_t seed,
                     int32_t deterministic, float *actions_out, float *log_prob_out, float *obs, float *reward, uint8_t *done, uint8_t *truncated,
                     int32_t *found_targets, float *terminal_obs, float *ep_return, int32_t *ep_length, uint64_t *done_mask, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    const LaunchEvents armed(env);                         // dn_set_launch_events: this launch takes the hook as well
    if (!given) return fail(DN_ERR_INVALID_ARGUMENT, "%s are required", w.required);
    if (((uintptr_t)src & 15u) || ((uintptr_t)actions_out & 15u) || ((uintptr_t)obs & 15u))
        return fail(DN_ERR_INVALID_ARGUMENT, "%s, actions_out and obs must be 16-byte aligned", w.src);
    if (!dn_config_is_plain(env->cfg))
        return fail(DN_ERR_INVALID_ARGUMENT, "%s is built for the configuration without reward wrappers / extra physics terms / RPM actions / random spawn / zero damping; "
                                             "%s", w.who, w.instead);
    if (const int32_t rc = refuse_models(env, w.who, w.instead)) return rc;
    const DnStepIO io = make_io(nullptr, obs, reward, done, truncated, found_targets, terminal_obs, ep_return, ep_length, done_mask,
                                src, actions_out, log_prob_out, log_std, seed, deterministic, squash);
    // the sampling lives in the single-step kernels (one wave, or three waves cut by dependency)
    DN_REFUSE_ARMED_CAPTURE(stream);
    DN_HIP(dn_launch_step_many(env->p, io, 1, env->cfg.compute_f32 != 0, kernel_shapes(env).single == 3 ? 3 : 1, (hipStream_t)stream));
    return DN_OK;
}

// dn_bind_privileged and dn_bind_goal: the binding of an enabled row writer.  rows = NULL unbinds both buffers.
int32_t bind_rows(float *&rows_slot, float *&term_slot, long long &cap_slot, float *rows, float *terminal_rows, int64_t capacity_steps)
{
    if (!rows) {
        if (terminal_rows) return fail(DN_ERR_INVALID_ARGUMENT, "terminal_rows without rows: rows = NULL unbinds both");
        rows_slot = term_slot = nullptr;
        cap_slot = 0;
        return DN_OK;
    }
    if (((uintptr_t)rows & 15u) || ((uintptr_t)terminal_rows & 15u)) return fail(DN_ERR_INVALID_ARGUMENT, "rows and terminal_rows must be 16-byte aligned");
    if (capacity_steps < 1) return fail(DN_ERR_INVALID_ARGUMENT, "capacity_steps must be >= 1 (got %lld)", (long long)capacity_steps);
    rows_slot = rows;
    term_slot = terminal_rows;
    cap_slot = capacity_steps;
    return DN_OK;
}

// The checks every dn_*_config shares.
int32_t check_resample_reserved(int32_t resample, int32_t reserved)
{
    if (resample != 0 && resample != 1) return fail(DN_ERR_INVALID_ARGUMENT, "resample must be 0 or 1 (got %d)", resample);
    if (reserved != 0) return fail(DN_ERR_INVALID_ARGUMENT, "reserved must be 0 (got %d)", reserved);
    return DN_OK;
}

// The tail of every dn_enable_* once its configuration is valid: on the first call, the model's allocation (`bytes`, handed to
// init(float4 *) to fill on the null stream, freed again if that fails).  `what` names the allocation in messages.
template <typename Init>
int32_t model_storage(float4 *&slot, size_t bytes, const char *what, Init init)
{
    if (!slot) {
        float4 *d = nullptr;
        const hipError_t he = hipMalloc(&d, bytes);
        if (he != hipSuccess) return fail(DN_ERR_OUT_OF_MEMORY, "hipMalloc(%zu bytes) for %s failed: %s", bytes, what, hipGetErrorString(he));
        if (!init(d) || hipStreamSynchronize(nullptr) != hipSuccess) {
            (void)hipFree(d);
            return fail(DN_ERR_HIP, "initialising %s failed", what);
        }
        slot = d;
    }
    return DN_OK;
}

// dn_set_* (set = true) and dn_get_* of a model share one body: this is its copy, in the direction asked for.  user == nullptr = leave.
hipError_t copy_rows(bool set, void *model, const void *user, size_t bytes, hipStream_t s)
{
    if (!user) return hipSuccess;
    return set ? hipMemcpyAsync(model, user, bytes, hipMemcpyDeviceToDevice, s)
               : hipMemcpyAsync(const_cast<void *>(user), model, bytes, hipMemcpyDeviceToDevice, s);
}

// The single-track configuration of track t of the bank: what build_table and ground_contact_reachable are given for it.
dn_config track_as_config(const dn_config &c, const dn_track_bank_config &b, int t, int base)
{
    dn_config one = c;
    one.num_waypoints = b.num_waypoints[t];
    memcpy(one.waypoints, b.waypoints + 3 * base, sizeof(double) * 3 * (size_t)b.num_waypoints[t]);
    return one;
}
size_t track_off_cdf(long long n) { return align_up((size_t)n * 2 * sizeof(int), 256); }

}  // namespace

extern "C" {

int32_t dn_abi_version(void) { return DN_ABI_VERSION; }

const char *dn_last_error(void) { return g_err; }

int32_t dn_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void dn_config_default(dn_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->num_envs = 1;
    cfg->threshold = 0.3;             // PBDroneSimulator.py:116
    cfg->max_steps = 4096;            // parameter_manager.py:25
    cfg->cylinder = 1;                // PBDroneSimulator.py:167
    cfg->include_distance = 1;        // PBDroneSimulator.py:661
    cfg->normalize_actions = 1;       // PBDroneSimulator.py:662
    cfg->ground_contact = DN_GROUND_CONTACT_AUTO;   // on wherever the term can fire at all (the reference always has it, PBDroneEnv.py:699)
    cfg->aviary_dim[0] = cfg->aviary_dim[1] = -1.0;   // make_env default aviary_dim, PBDroneSimulator.py:141
    cfg->aviary_dim[3] = cfg->aviary_dim[4] = cfg->aviary_dim[5] = 1.0;
}

int64_t dn_state_bytes(int64_t num_envs, int32_t normalize_obs)
{
    if (num_envs < 1) return 0;
    return (int64_t)make_layout(num_envs, normalize_obs).total;
}

int32_t dn_create(const dn_config *cfg, dn_env **out)
{
    if (!out) return fail(DN_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int32_t rc = validate(cfg);
    if (rc != DN_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(DN_ERR_NO_DEVICE, "no HIP device is visible: libdronenav has no CPU fallback");
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(DN_ERR_INVALID_ARGUMENT, "device_id %d out of range (%d devices)", cfg->device_id, ndev);
    DN_HIP(hipSetDevice(cfg->device_id));

    // the half-built env: freed, arena included, on every early return below; released into *out at the end
    struct Unbuild { void operator()(dn_env *h) const { if (h->arena) (void)hipFree(h->arena); delete h; } };
    std::unique_ptr<dn_env, Unbuild> owner(new (std::nothrow) dn_env());
    dn_env *e = owner.get();
    if (!e) return fail(DN_ERR_OUT_OF_MEMORY, "host allocation failed");
    e->cfg = *cfg;
    e->ground_contact_auto = e->cfg.ground_contact == DN_GROUND_CONTACT_AUTO;
    if (e->ground_contact_auto) e->cfg.ground_contact = ground_contact_reachable(*cfg) ? 1 : 0;
    cfg = &e->cfg;                                      // from here on: the resolved configuration (dn_get_config returns it)
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device_id) == hipSuccess && cus > 0) e->num_cus = cus;
    }
    const long long n = cfg->num_envs;
    e->blocks = (n + DN_BLOCK - 1) / DN_BLOCK;
    e->picked = dn_pick_shapes(*cfg, e->num_cus, getenv("DN_WAVES"), getenv("DN_WAVES_SINGLE"));
    const int drag = cfg->physics == 2 || cfg->physics == 4;
    const int pid_mode = (cfg->action_type == 2 || cfg->action_type == 3 || cfg->action_type == 5) ? cfg->action_type : 0;
    const Layout L = make_layout(n, cfg->normalize_obs, cfg->norm_rew, drag, pid_mode);
    const hipError_t he = hipMalloc(&e->arena, L.total);
    if (he != hipSuccess) return fail(DN_ERR_OUT_OF_MEMORY, "hipMalloc(%zu bytes) for %lld drones failed: %s", L.total, n, hipGetErrorString(he));
    e->arena_bytes = L.total;
    char *base = (char *)e->arena;
    DnParams &p = e->p;
    memset(&p, 0, sizeof p);
    p.st.g0 = (float4 *)(base + L.off_g[0]); p.st.g1 = (float4 *)(base + L.off_g[1]);
    p.st.g2 = (float4 *)(base + L.off_g[2]); p.st.g3 = (float4 *)(base + L.off_g[3]);
    p.st.g4 = (float4 *)(base + L.off_g[4]); p.st.g5 = (float4 *)(base + L.off_g[5]);
    p.st.g6 = (float4 *)(base + L.off_g[6]);
    p.st.g7 = drag ? (float4 *)(base + L.off_g7) : nullptr;
    p.st.rms_mean = (double *)(base + L.off_mean);
    p.st.rms_m2 = (double *)(base + L.off_var);
    p.st.rms_count = (double *)(base + L.off_count);
    p.st.rr = (double *)(base + L.off_rr);
    p.st.pid = pid_mode ? (double *)(base + L.off_pid) : nullptr;
    p.st.stats = (DnStatSlot *)(base + L.off_stats);
    e->tab64 = (double *)(base + L.off_tab64);
    e->tab32 = (float *)(base + L.off_tab32);
    p.tab64 = e->tab64;
    p.tab32 = e->tab32;
    p.n = n;
    p.num_waypoints = cfg->num_waypoints;
    p.num_cus = e->num_cus;
    p.max_steps = cfg->max_steps;
    p.circle = cfg->circle != 0; p.cylinder = cfg->cylinder != 0; p.include_distance = cfg->include_distance != 0;
    p.normalize_actions = cfg->normalize_actions != 0; p.normalize_obs = cfg->normalize_obs != 0;
    p.ground_contact = cfg->ground_contact != 0;
    p.clip_rew = cfg->clip_rew != 0; p.norm_rew = cfg->norm_rew != 0;
    p.gnd = cfg->physics == 1 || cfg->physics == 4; p.drag = drag; p.rpm_actions = cfg->action_type == 1 ? 1 : (cfg->action_type == 4 ? 2 : 0);
    p.pid_mode = pid_mode;
    p.random_spawn = cfg->random_spawn != 0;
    p.zero_damping = cfg->zero_damping != 0;
    {   // DN_EXACT_OBS_NOISE=1: observation noise in the exact float64 Box-Muller form (reproducible across GPU generations; ~10 % slower noisy steps)
        // DN_EXACT_NORM=1: the normaliser's output stage in float64 (the float32 nearest to the float64 evaluation instead of <= 3 ulp) -- a
        // compile-time form (dn_kernels.hip, normalize_obs_cols) that lives in libdronenav_exact.so: here the request is only CHECKED against the build.
        // Both are readable back through dn_get_exact_flags; a value that is neither a yes nor a no fails the create.
        int v = env_switch("DN_EXACT_OBS_NOISE");
        if (v < 0) return fail(DN_ERR_INVALID_ARGUMENT, "DN_EXACT_OBS_NOISE=%s: expected 1 | true | on | yes or 0 | false | off | no", getenv("DN_EXACT_OBS_NOISE"));
        p.exact_obs_noise = v;
        v = env_switch("DN_EXACT_NORM");
        if (v < 0) return fail(DN_ERR_INVALID_ARGUMENT, "DN_EXACT_NORM=%s: expected 1 | true | on | yes or 0 | false | off | no", getenv("DN_EXACT_NORM"));
        if (v == 1 && !dn_norm_exact_compiled_in())
            return fail(DN_ERR_INVALID_ARGUMENT, "DN_EXACT_NORM=1 asks for the normaliser's float64 output stage, which is a build of its own: load "
                                                 "libdronenav_exact.so (the Python package does when the variable is set) instead of this library");
    }
    p.act_noise_sigma = cfg->act_noise_sigma; p.obs_noise_sigma = cfg->obs_noise_sigma;
    p.seed = cfg->seed; p.env_id_offset = cfg->env_id_offset;
    build_consts<double>(*cfg, p.c64);
    build_consts<float>(*cfg, p.c32);

    std::vector<double> t64(DN_MAX_WAYPOINTS * DN_T_STRIDE, 0.0);
    std::vector<float> t32(DN_MAX_WAYPOINTS * DN_T_STRIDE, 0.0f);
    build_table(*cfg, t64.data());
    for (size_t j = 0; j < t64.size(); ++j) t32[j] = (float)t64[j];
    if (hipMemcpy(e->tab64, t64.data(), t64.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->tab32, t32.data(), t32.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(DN_ERR_HIP, "uploading the waypoint table failed");

    rc = init_state(e, nullptr);
    if (rc != DN_OK) return rc;
    if (cfg->random_spawn) {                // make_env's env.reset(seed=...) (PBDroneSimulator.py:173) already draws a spawn point
        float *scratch = nullptr;
        if (hipMalloc(&scratch, (size_t)n * DN_OBS_DIM * sizeof(float)) != hipSuccess) return fail(DN_ERR_OUT_OF_MEMORY, "scratch observation buffer");
        const bool launched = dn_launch_reset(e->p, scratch, cfg->compute_f32 != 0, nullptr) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
        (void)hipFree(scratch);
        if (!launched) return fail(DN_ERR_HIP, "initial random spawn failed");
        if (cfg->normalize_obs) {           // that reset happens BEFORE the NormalizeObservation wrapper exists: statistics stay pristine
            rc = init_state_rms(e, nullptr);
            if (rc != DN_OK) return rc;
        }
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail(DN_ERR_HIP, "state initialisation failed");
    *out = owner.release();
    return DN_OK;
}

int32_t dn_destroy(dn_env *env)
{
    if (!env) return DN_OK;
    hipError_t he = hipSuccess;
    void *owned[1 + sizeof MODELS / sizeof MODELS[0]] = {env->arena};
    int k = 1;
    for (const ModelRow &r : MODELS) owned[k++] = r.slot(env->m);
    bool device_set = false;
    for (void *ptr : owned) {               // the first failure is the one reported; the rest are still freed
        if (!ptr) continue;
        if (!device_set) (void)hipSetDevice(env->cfg.device_id);
        device_set = true;
        const hipError_t h = hipFree(ptr);
        if (he == hipSuccess) he = h;
    }
    delete env;
    if (he != hipSuccess) return fail(DN_ERR_HIP, "hipFree failed: %s", hipGetErrorString(he));
    return DN_OK;
}

int64_t dn_num_envs(const dn_env *env) { return env ? env->cfg.num_envs : 0; }

int32_t dn_get_config(const dn_env *env, dn_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    *out = env->cfg;                                  // ground_contact resolved to 0 / 1
    return DN_OK;
}

int32_t dn_get_num_cus(const dn_env *env) { return env ? env->num_cus : 0; }

int32_t dn_get_exact_flags(const dn_env *env)
{
    if (!env) return 0;
    return (env->p.exact_obs_noise ? DN_EXACT_FLAG_OBS_NOISE : 0) | (dn_norm_exact_compiled_in() ? DN_EXACT_FLAG_NORM : 0);
}

int32_t dn_resolve_ground_contact(const dn_config *cfg)
{
    const int32_t rc = validate(cfg);
    if (rc != DN_OK) return rc;
    if (cfg->ground_contact != DN_GROUND_CONTACT_AUTO) return cfg->ground_contact;
    return ground_contact_reachable(*cfg) ? 1 : 0;
}

int32_t dn_reset(dn_env *env, float *obs, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    if (!obs) return fail(DN_ERR_INVALID_ARGUMENT, "obs is NULL");
    DN_HIP(dn_launch_reset(env->p, obs, env->cfg.compute_f32 != 0, (hipStream_t)stream, &env->m));
    return DN_OK;
}

int32_t dn_step(dn_env *env, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *truncated,
                int32_t *found_targets, float *terminal_obs, float *ep_return, int32_t *ep_length,
                uint64_t *done_mask, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    const LaunchEvents armed(env);                         // dn_set_launch_events: consumed by this call, or dropped if it fails below
    if (!actions || !obs || !reward || !done || !truncated || !found_targets)
        return fail(DN_ERR_INVALID_ARGUMENT, "actions, obs, reward, done, truncated and found_targets are required");
    if (((uintptr_t)actions & 15u) || ((uintptr_t)obs & 15u))
        return fail(DN_ERR_INVALID_ARGUMENT, "actions and obs must be 16-byte aligned");
    DN_REFUSE_ARMED_CAPTURE(stream);
    const DnStepIO io = make_io(actions, obs, reward, done, truncated, found_targets, terminal_obs, ep_return, ep_length, done_mask);
    DN_HIP(dn_launch_step_many(env->p, io, 1, env->cfg.compute_f32 != 0, kernel_shapes(env).single, (hipStream_t)stream, &env->m));
    return DN_OK;
}

int32_t dn_step_sampled(dn_env *env, const float *mean, const float *log_std, uint64_t seed, int32_t deterministic,
                        float *actions_out, float *log_prob_out, float *obs, float *reward, uint8_t *done, uint8_t *truncated,
                        int32_t *found_targets, float *terminal_obs, float *ep_return, int32_t *ep_length,
                        uint64_t *done_mask, void *stream)
{
    const SamplerWords w = {"dn_step_sampled", "mean", "mean, log_std, actions_out, log_prob_out, obs, reward, done, truncated and found_targets",
                            "use dn_policy_sample + dn_step there"};
    const bool given = mean && log_std && actions_out && log_prob_out && obs && reward && done && truncated && found_targets;
    return sampler_step(env, w, given, mean, log_std, 0, seed, deterministic, actions_out, log_prob_out, obs, reward, done, truncated, found_targets,
                        terminal_obs, ep_return, ep_length, done_mask, stream);
}

int32_t dn_step_squashed(dn_env *env, const float *mu_log_std, uint64_t seed, int32_t deterministic, float *actions_out,
                         float *log_prob_out, float *obs, float *reward, uint8_t *done, uint8_t *truncated, int32_t *found_targets,
                         float *terminal_obs, float *ep_return, int32_t *ep_length, uint64_t *done_mask, void *stream)
{
    const SamplerWords w = {"dn_step_squashed", "mu_log_std", "mu_log_std, actions_out, obs, reward, done, truncated and found_targets",
                            "use dn_squashed_sample + dn_step there"};
    const bool given = mu_log_std && actions_out && obs && reward && done && truncated && found_targets;
    return sampler_step(env, w, given, mu_log_std, nullptr, 1, seed, deterministic, actions_out, log_prob_out, obs, reward, done, truncated,
                        found_targets, terminal_obs, ep_return, ep_length, done_mask, stream);      // the rows carry log_std
}

int32_t dn_mlp_step_sampled(dn_env *env, const dn_mlp_net *nets, int32_t num_nets, const float *policy_obs, int32_t obs_dim,
                            const float *log_std, uint64_t seed, int32_t deterministic, float *actions_out, float *log_prob_out,
                            float *obs, float *reward, uint8_t *done, uint8_t *truncated, int32_t *found_targets, float *terminal_obs,
                            float *ep_return, int32_t *ep_length, uint64_t *done_mask, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    const LaunchEvents dropped(env);                       // no hook on this launch: armed events are dropped here, not left for a later call
    dn_tl_ev_start = dn_tl_ev_stop = nullptr;
    if (!nets || !policy_obs || !log_std || !actions_out || !log_prob_out || !obs || !reward || !done || !truncated || !found_targets)
        return fail(DN_ERR_INVALID_ARGUMENT, "nets, policy_obs, log_std, actions_out, log_prob_out, obs, reward, done, truncated and found_targets are required");
    if (num_nets < 1 || num_nets > 2) return fail(DN_ERR_INVALID_ARGUMENT, "num_nets must be 1 (actor) or 2 (actor, critic)");
    if (obs_dim < 1 || obs_dim > 16) return fail(DN_ERR_INVALID_ARGUMENT, "obs_dim must be in 1..16 (got %d)", obs_dim);
    if (((uintptr_t)actions_out & 15u) || ((uintptr_t)obs & 15u)) return fail(DN_ERR_INVALID_ARGUMENT, "actions_out and obs must be 16-byte aligned");
    if (const int32_t rc = refuse_models(env, "dn_mlp_step_sampled", "use dn_mlp_forward + dn_policy_sample + dn_step")) return rc;
    const dn_config &c = env->cfg;
    for (int k = 0; k < num_nets; ++k) {
        const dn_mlp_net &n = nets[k];
        if (n.arch != DN_MLP_ARCH_PPO) return fail(DN_ERR_INVALID_ARGUMENT, "net %d: dn_mlp_step_sampled runs the PPO networks (arch 0)", k);
        if (!n.w1 || !n.w2 || !n.w3 || !n.wh || !n.b1 || !n.b2 || !n.b3 || !n.bh || !n.out)
            return fail(DN_ERR_INVALID_ARGUMENT, "net %d: every weight, bias and output pointer is required", k);
        if (n.grade < 0 || n.grade > 2 || n.grade != nets[0].grade) return fail(DN_ERR_INVALID_ARGUMENT, "net %d: grade must be 0 | 1 | 2 and the same for both networks", k);
        if (n.out_dim < 1 || n.out_dim > 32) return fail(DN_ERR_INVALID_ARGUMENT, "net %d: out_dim must be in 1..32", k);
        if (((uintptr_t)n.w1 | (uintptr_t)n.w2 | (uintptr_t)n.w3 | (uintptr_t)n.wh) & 15u)
            return fail(DN_ERR_INVALID_ARGUMENT, "net %d: packed weights must be 16-byte aligned", k);
    }
    if (nets[0].out_dim != DN_ACT_DIM) return fail(DN_ERR_INVALID_ARGUMENT, "nets[0] must be the actor (out_dim 4)");
    {   // one launch: the critic's workgroups and later actor workgroups still READ policy_obs while earlier actor tails already WRITE obs
        // and the networks' outputs -- overlapping buffers would be a silent data race, so they are refused
        const uintptr_t nn = (uintptr_t)c.num_envs, pbytes = nn * obs_dim * sizeof(float), obytes = nn * DN_OBS_DIM * sizeof(float);
        if (dn_ranges_overlap(policy_obs, pbytes, obs, obytes))
            return fail(DN_ERR_INVALID_ARGUMENT, "policy_obs must not overlap obs (the launch reads one while it writes the other)");
        for (int k = 0; k < num_nets; ++k) {
            const uintptr_t nbytes = nn * nets[k].out_dim * sizeof(float);
            if (dn_ranges_overlap(nets[k].out, nbytes, policy_obs, pbytes) || dn_ranges_overlap(nets[k].out, nbytes, obs, obytes))
                return fail(DN_ERR_INVALID_ARGUMENT, "net %d: out must not overlap policy_obs or obs", k);
        }
    }
    // the tail is the three-wave single step: the plain configuration dn_step_sampled covers, without noise and without the
    // ground-contact term, on fleets for which dn_create picked that shape; whole workgroups of the policy kernel only
    if (!dn_config_is_plain(c) || c.ground_contact || dn_config_is_noisy(c) || c.compute_f32 || kernel_shapes(env).single != 3)
        return fail(DN_ERR_INVALID_ARGUMENT, "dn_mlp_step_sampled is built for the float64 reference configuration without noise / reward wrappers / extra "
                                             "physics / ground contact on fleets that take the three-wave single step; use dn_mlp_forward + dn_step_sampled");
    const long long per_wg = nets[0].grade == 1 ? 64 : 128;
    if (c.num_envs % per_wg) return fail(DN_ERR_INVALID_ARGUMENT, "dn_mlp_step_sampled needs num_envs %% %lld == 0 (got %lld)", per_wg, (long long)c.num_envs);
    const DnStepIO io = make_io(nullptr, obs, reward, done, truncated, found_targets, terminal_obs, ep_return, ep_length, done_mask,
                                nullptr, actions_out, log_prob_out, log_std, seed, deterministic, 0);
    DN_HIP(hipSetDevice(c.device_id));
    DN_HIP(dn_launch_mlp_step(env->p, io, nets, num_nets, policy_obs, obs_dim, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_eval_kinematics(dn_env *env, const double *kinematics, float *obs, float *reward, uint8_t *done, uint8_t *truncated,
                           int32_t *found_targets, float *terminal_obs, float *ep_return, int32_t *ep_length, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    const LaunchEvents dropped(env);                       // no hook on this launch: armed events are dropped here, not left for a later call
    dn_tl_ev_start = dn_tl_ev_stop = nullptr;
    if (!kinematics || !obs || !reward || !done || !truncated || !found_targets)
        return fail(DN_ERR_INVALID_ARGUMENT, "kinematics, obs, reward, done, truncated and found_targets are required");
    if (((uintptr_t)kinematics & 7u) || ((uintptr_t)obs & 15u))
        return fail(DN_ERR_INVALID_ARGUMENT, "kinematics must be 8-byte and obs 16-byte aligned");
    const dn_config &c = env->cfg;
    // deliberately not dn_config_is_plain: a replayed transition never meets zero_damping, and noise is refused here as well
    if (c.act_noise_sigma > 0.0f || c.obs_noise_sigma > 0.0f || c.clip_rew || c.norm_rew || c.physics != 0 || c.action_type != 0 || c.random_spawn)
        return fail(DN_ERR_INVALID_ARGUMENT, "dn_eval_kinematics is built for the reference configuration (no noise, no reward wrappers, "
                                             "Physics.PYB, ActionType.THRUST, fixed spawn)");
    if (const int32_t rc = refuse_models(env, "dn_eval_kinematics", nullptr)) return rc;
    const DnStepIO io = make_io(nullptr, obs, reward, done, truncated, found_targets, terminal_obs, ep_return, ep_length, nullptr);
    DN_HIP(dn_launch_eval_kinematics(env->p, io, kinematics, c.compute_f32 != 0, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_step_many(dn_env *env, int64_t k, const float *actions, float *obs, float *reward, uint8_t *done,
                     uint8_t *truncated, int32_t *found_targets, float *terminal_obs, float *ep_return,
                     int32_t *ep_length, uint64_t *done_mask, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    const LaunchEvents armed(env);                         // dn_set_launch_events: consumed by this call, or dropped if it fails below
    if (k < 1) return fail(DN_ERR_INVALID_ARGUMENT, "k must be >= 1 (got %lld)", (long long)k);
    const long long n = env->cfg.num_envs;
    if (k > 1 && (n & 3)) return fail(DN_ERR_INVALID_ARGUMENT, "dn_step_many needs num_envs %% 4 == 0 (got %lld)", n);
    if (k == 1)
        return dn_step(env, actions, obs, reward, done, truncated, found_targets, terminal_obs, ep_return, ep_length,
                       done_mask, stream);
    if (!actions || !obs || !reward || !done || !truncated || !found_targets)
        return fail(DN_ERR_INVALID_ARGUMENT, "actions, obs, reward, done, truncated and found_targets are required");
    if (((uintptr_t)actions & 15u) || ((uintptr_t)obs & 15u))
        return fail(DN_ERR_INVALID_ARGUMENT, "actions and obs must be 16-byte aligned");
    if (k > (1 << 30)) return fail(DN_ERR_INVALID_ARGUMENT, "k too large");
    if (env->m.priv.groups && env->m.priv.rows && k > env->m.priv.cap)
        return fail(DN_ERR_INVALID_ARGUMENT, "dn_step_many: k = %lld exceeds the %lld steps the privileged rows hold (dn_bind_privileged capacity_steps)",
                    (long long)k, env->m.priv.cap);
    if (env->m.goal.on && env->m.goal.rows && k > env->m.goal.cap)
        return fail(DN_ERR_INVALID_ARGUMENT, "dn_step_many: k = %lld exceeds the %lld steps the goal rows hold (dn_bind_goal capacity_steps)",
                    (long long)k, env->m.goal.cap);
    // one fused launch: the state stays in registers for all k steps (dn_step_many_kernel)
    const DnStepIO io = make_io(actions, obs, reward, done, truncated, found_targets, terminal_obs, ep_return, ep_length, done_mask);
    DN_REFUSE_ARMED_CAPTURE(stream);
    DN_HIP(dn_launch_step_many(env->p, io, (int)k, env->cfg.compute_f32 != 0, kernel_shapes(env).fused, (hipStream_t)stream, &env->m));
    return DN_OK;
}

int32_t dn_set_launch_events(dn_env *env, void *start_event, void *stop_event)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    env->ev_start = (hipEvent_t)start_event;
    env->ev_stop = (hipEvent_t)stop_event;
    return DN_OK;
}

// Monitor's running return is held as the float32 hi (g4.w) + k * ulp(hi) / 256 with k the signed top byte of the length
// word (dn_kernels.hip report_scalars); dn_env_state shows the low part as a float.
static float ret_lo_decode(float hi, int k)
{
    uint32_t bits;
    memcpy(&bits, &hi, 4);
    const int eb = (int)((bits >> 23) & 0xFFu);
    return (eb > 31 && eb != 255) ? (float)ldexp((double)k, eb - 127 - 31) : 0.0f;      // inf / NaN carry no low part (ret_lo_encode)
}
static int ret_lo_encode(float hi, float lo)
{
    uint32_t bits;
    memcpy(&bits, &hi, 4);
    const int eb = (int)((bits >> 23) & 0xFFu);
    if (eb <= 31 || eb == 255) return 0;
    const double q = nearbyint(ldexp((double)lo, 127 + 31 - eb));
    return (int)fmin(fmax(q, -128.0), 127.0) & 0xFF;
}

int32_t dn_get_state(dn_env *env, dn_env_state *states, int64_t count)
{
    if (!env || !states) return fail(DN_ERR_INVALID_ARGUMENT, "env and states are required");
    const long long n = env->cfg.num_envs;
    if (count != n) return fail(DN_ERR_INVALID_ARGUMENT, "count (%lld) != num_envs (%lld)", (long long)count, n);
    DN_HIP(hipSetDevice(env->cfg.device_id));
    DN_HIP(hipDeviceSynchronize());
    std::vector<float4> g[7];
    float4 *src[7] = {env->p.st.g0, env->p.st.g1, env->p.st.g2, env->p.st.g3, env->p.st.g4, env->p.st.g5, env->p.st.g6};
    for (int k = 0; k < 7; ++k) {
        g[k].resize((size_t)n);
        DN_HIP(hipMemcpy(g[k].data(), src[k], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    std::vector<double> mean, var, cnt;
    if (env->cfg.normalize_obs) {
        mean.resize((size_t)n * DN_OBS_DIM); var.resize((size_t)n * DN_OBS_DIM); cnt.resize((size_t)n);
        DN_HIP(hipMemcpy(mean.data(), env->p.st.rms_mean, mean.size() * sizeof(double), hipMemcpyDeviceToHost));
        DN_HIP(hipMemcpy(var.data(), env->p.st.rms_m2, var.size() * sizeof(double), hipMemcpyDeviceToHost));
        DN_HIP(hipMemcpy(cnt.data(), env->p.st.rms_count, cnt.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::vector<double> rr;
    if (env->cfg.norm_rew) {
        rr.resize((size_t)n * 4);
        DN_HIP(hipMemcpy(rr.data(), env->p.st.rr, rr.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::vector<float4> g7;
    if (env->p.drag) {
        g7.resize((size_t)n);
        DN_HIP(hipMemcpy(g7.data(), env->p.st.g7, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    std::vector<double> pid;
    if (env->p.pid_mode) {
        pid.resize((size_t)n * 9);
        DN_HIP(hipMemcpy(pid.data(), env->p.st.pid, pid.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (long long i = 0; i < n; ++i) {
        dn_env_state &s = states[i];
        memset(&s, 0, sizeof s);
        if (env->p.pid_mode) for (int k = 0; k < 9; ++k) s.pid[k] = pid[(size_t)k * n + i];
        if (env->p.drag) { s.last_rpm[0] = g7[(size_t)i].x; s.last_rpm[1] = g7[(size_t)i].y; s.last_rpm[2] = g7[(size_t)i].z; s.last_rpm[3] = g7[(size_t)i].w; }
        if (env->cfg.norm_rew) { s.rr_returns = rr[(size_t)i]; s.rr_mean = rr[(size_t)n + i]; s.rr_var = rr[(size_t)2 * n + i]; s.rr_count = rr[(size_t)3 * n + i]; }
        s.pos[0] = g[0][i].x; s.pos[1] = g[0][i].y; s.pos[2] = g[0][i].z; s.d = g[0][i].w;
        s.quat[0] = g[1][i].x; s.quat[1] = g[1][i].y; s.quat[2] = g[1][i].z; s.quat[3] = g[1][i].w;
        s.vel[0] = g[2][i].x; s.vel[1] = g[2][i].y; s.vel[2] = g[2][i].z; s.d_prev = g[2][i].w;
        s.ang_v[0] = g[3][i].x; s.ang_v[1] = g[3][i].y; s.ang_v[2] = g[3][i].z;
        uint32_t meta;
        memcpy(&meta, &g[3][i].w, 4);
        s.steps = (int32_t)(meta & 0xFFFFFFu); s.idx = (int32_t)((meta >> 24) & 0x7Fu); s.just_found = (int32_t)(meta >> 31);
        s.prev_vel[0] = g[4][i].x; s.prev_vel[1] = g[4][i].y; s.prev_vel[2] = g[4][i].z; s.ep_ret = g[4][i].w;
        s.prev_ang_v[0] = g[5][i].x; s.prev_ang_v[1] = g[5][i].y; s.prev_ang_v[2] = g[5][i].z;
        int32_t lenword;
        memcpy(&lenword, &g[5][i].w, 4);
        s.ep_len = lenword & 0xFFFFFF;
        s.ep_ret_lo = ret_lo_decode(s.ep_ret, lenword >> 24);
        // _current_position equals pos once a post-step has run (steps > 0); the stored copy is the stale one
        if (s.steps > 0) { s.cur_pos[0] = s.pos[0]; s.cur_pos[1] = s.pos[1]; s.cur_pos[2] = s.pos[2]; }
        else { s.cur_pos[0] = g[6][i].x; s.cur_pos[1] = g[6][i].y; s.cur_pos[2] = g[6][i].z; }
        if (env->cfg.normalize_obs) {
            for (int k = 0; k < DN_OBS_DIM; ++k) { s.rms_mean[k] = mean[(size_t)k * n + i]; s.rms_m2[k] = var[(size_t)k * n + i]; s.rms_var[k] = s.rms_m2[k] / cnt[(size_t)i]; }      // the device holds the second moment var x count: verbatim, and as var
            s.rms_count = cnt[(size_t)i];
        }
    }
    return DN_OK;
}

int32_t dn_set_state(dn_env *env, const dn_env_state *states, int64_t count)
{
    if (!env || !states) return fail(DN_ERR_INVALID_ARGUMENT, "env and states are required");
    const long long n = env->cfg.num_envs;
    if (count != n) return fail(DN_ERR_INVALID_ARGUMENT, "count (%lld) != num_envs (%lld)", (long long)count, n);
    std::vector<float4> g[7];
    for (int k = 0; k < 7; ++k) g[k].resize((size_t)n);
    std::vector<double> mean, var, cnt;
    if (env->cfg.normalize_obs) { mean.resize((size_t)n * DN_OBS_DIM); var.resize((size_t)n * DN_OBS_DIM); cnt.resize((size_t)n); }
    std::vector<double> rr;
    if (env->cfg.norm_rew) rr.resize((size_t)n * 4);
    std::vector<float4> g7;
    if (env->p.drag) g7.resize((size_t)n);
    std::vector<double> pid;
    if (env->p.pid_mode) pid.resize((size_t)n * 9);
    // dn_enable_tracks: idx is the index within the drone's OWN track, so it is held to that track's count -- the assignment as it stands
    // on the device (a checkpoint is restored as dn_set_tracks, then dn_set_state), an index outside the bank held to it as the kernels do
    std::vector<int32_t> track;
    if (env->m.track.track) {
        track.resize((size_t)n);
        DN_HIP(hipSetDevice(env->cfg.device_id));
        DN_HIP(hipDeviceSynchronize());
        DN_HIP(hipMemcpy(track.data(), env->m.track.track, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    for (long long i = 0; i < n; ++i) {
        const dn_env_state &s = states[i];
        int num_waypoints = env->cfg.num_waypoints;
        if (!track.empty()) {
            const int T = env->track_cfg.num_tracks, t = track[(size_t)i] < 0 ? 0 : (track[(size_t)i] >= T ? T - 1 : track[(size_t)i]);
            num_waypoints = env->track_cfg.num_waypoints[t];
        }
        if (env->p.pid_mode) for (int k = 0; k < 9; ++k) pid[(size_t)k * n + i] = s.pid[k];
        if (env->p.drag) g7[(size_t)i] = make_float4(s.last_rpm[0], s.last_rpm[1], s.last_rpm[2], s.last_rpm[3]);
        if (env->cfg.norm_rew) { rr[(size_t)i] = s.rr_returns; rr[(size_t)n + i] = s.rr_mean; rr[(size_t)2 * n + i] = s.rr_var; rr[(size_t)3 * n + i] = s.rr_count; }
        if (s.idx < 0 || s.idx >= num_waypoints || s.steps < 0 || s.steps > (1 << 24) - 1)
            return fail(DN_ERR_INVALID_ARGUMENT, "state %lld: idx/steps out of range", i);
        if (s.steps > 0 && (s.cur_pos[0] != s.pos[0] || s.cur_pos[1] != s.pos[1] || s.cur_pos[2] != s.pos[2]))
            return fail(DN_ERR_BAD_STATE, "state %lld: _current_position must equal pos once _steps > 0", i);
        uint32_t meta = ((uint32_t)s.steps & 0xFFFFFFu) | (((uint32_t)s.idx & 0x7Fu) << 24) | ((uint32_t)(s.just_found != 0) << 31);
        float fmeta, flen;
        memcpy(&fmeta, &meta, 4);
        if (s.ep_len < 0 || s.ep_len > 0xFFFFFF) return fail(DN_ERR_INVALID_ARGUMENT, "state %lld: ep_len out of range", i);
        const int32_t lenword = s.ep_len | (int32_t)((uint32_t)ret_lo_encode(s.ep_ret, s.ep_ret_lo) << 24);
        memcpy(&flen, &lenword, 4);
        g[0][i] = make_float4(s.pos[0], s.pos[1], s.pos[2], s.d);
        g[1][i] = make_float4(s.quat[0], s.quat[1], s.quat[2], s.quat[3]);
        g[2][i] = make_float4(s.vel[0], s.vel[1], s.vel[2], s.d_prev);
        g[3][i] = make_float4(s.ang_v[0], s.ang_v[1], s.ang_v[2], fmeta);
        g[4][i] = make_float4(s.prev_vel[0], s.prev_vel[1], s.prev_vel[2], s.ep_ret);
        g[5][i] = make_float4(s.prev_ang_v[0], s.prev_ang_v[1], s.prev_ang_v[2], flen);
        g[6][i] = make_float4(s.cur_pos[0], s.cur_pos[1], s.cur_pos[2], 0.0f);
        if (env->cfg.normalize_obs) {
            if (!dn_rms_count_ok(s.rms_count)) return fail(DN_ERR_INVALID_ARGUMENT, "state %lld: rms_count must be > 0 and finite (RunningMeanStd starts at 1e-4)", i);
            for (int k = 0; k < DN_OBS_DIM; ++k) { mean[(size_t)k * n + i] = s.rms_mean[k]; var[(size_t)k * n + i] = dn_restore_second_moment(s.rms_var[k], s.rms_count, s.rms_m2[k]); }
            cnt[(size_t)i] = s.rms_count;
        }
    }
    DN_HIP(hipSetDevice(env->cfg.device_id));
    DN_HIP(hipDeviceSynchronize());
    float4 *dst[7] = {env->p.st.g0, env->p.st.g1, env->p.st.g2, env->p.st.g3, env->p.st.g4, env->p.st.g5, env->p.st.g6};
    for (int k = 0; k < 7; ++k) DN_HIP(hipMemcpy(dst[k], g[k].data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
    if (env->cfg.normalize_obs) {
        DN_HIP(hipMemcpy(env->p.st.rms_mean, mean.data(), mean.size() * sizeof(double), hipMemcpyHostToDevice));
        DN_HIP(hipMemcpy(env->p.st.rms_m2, var.data(), var.size() * sizeof(double), hipMemcpyHostToDevice));
        DN_HIP(hipMemcpy(env->p.st.rms_count, cnt.data(), cnt.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (env->cfg.norm_rew) DN_HIP(hipMemcpy(env->p.st.rr, rr.data(), rr.size() * sizeof(double), hipMemcpyHostToDevice));
    if (env->p.drag) DN_HIP(hipMemcpy(env->p.st.g7, g7.data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
    if (env->p.pid_mode) DN_HIP(hipMemcpy(env->p.st.pid, pid.data(), pid.size() * sizeof(double), hipMemcpyHostToDevice));
    return DN_OK;
}

int32_t dn_get_stats(dn_env *env, dn_stats *out, void *stream)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    std::vector<DnStatSlot> slots((size_t)env->blocks);
    DN_HIP(hipMemcpyAsync(slots.data(), env->p.st.stats, slots.size() * sizeof(DnStatSlot), hipMemcpyDeviceToHost, (hipStream_t)stream));
    DN_HIP(hipStreamSynchronize((hipStream_t)stream));
    memset(out, 0, sizeof *out);
    long long fix = 0;
    for (const DnStatSlot &s : slots) {
        out->episodes += s.episodes; out->truncated += s.truncated; out->completed += s.completed;
        out->sum_ep_len += s.sum_len; out->sum_found_targets += s.sum_found; fix += s.sum_ret_fix;
    }
    out->sum_ep_return = (double)fix * 1e-6;
    out->env_steps = (int64_t)slots[0].step_count * env->cfg.num_envs;
    return DN_OK;
}

int32_t dn_reset_stats(dn_env *env, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    // the slots also hold the vector-step counter, which a statistics reset must not rewind
    uint64_t steps = 0;
    int32_t rc = dn_get_step_count(env, &steps);
    if (rc != DN_OK) return rc;
    DN_HIP(hipMemsetAsync(env->p.st.stats, 0, (size_t)env->blocks * sizeof(DnStatSlot), (hipStream_t)stream));
    DN_HIP(dn_launch_set_step_count(env->p.st.stats, env->blocks, steps, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_get_kernel_waves(const dn_env *env, int32_t fused)
{
    if (!env) return 0;
    return fused ? kernel_shapes(env).fused : kernel_shapes(env).single;
}

int32_t dn_enable_dynamics(dn_env *env, const dn_dynamics_config *cfg)
{
    if (!env || !cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    const float *rng[4] = {cfg->mass, cfg->inertia, cfg->kf, cfg->km};
    const char *names[4] = {"mass", "inertia", "kf", "km"};
    for (int j = 0; j < 4; ++j) {
        const float lo = rng[j][0], hi = rng[j][1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo > 0.0f) || !(lo <= hi))
            return fail(DN_ERR_INVALID_ARGUMENT, "dynamics range %s = [%g, %g]: need finite 0 < lo <= hi", names[j], (double)lo, (double)hi);
    }
    if (const int32_t rc = check_resample_reserved(cfg->resample, cfg->reserved)) return rc;
    DN_HIP(hipSetDevice(env->cfg.device_id));
    const long long n = env->cfg.num_envs;
    DnDyn &d = env->m.dyn;
    // first call: the per-drone scales, all 1 (the nominal body) until a reset draws or dn_set_dynamics writes
    if (const int32_t rc = model_storage(d.dyn, (size_t)n * sizeof(float4), "the dynamics scales", [&](float4 *mem) {
            return dn_launch_fill4(mem, make_float4(1.0f, 1.0f, 1.0f, 1.0f), n, nullptr) == hipSuccess;
        }))
        return rc;
    for (int j = 0; j < 4; ++j) { d.lo[j] = rng[j][0]; d.hi[j] = rng[j][1]; }
    d.resample = cfg->resample;
    env->dyn_cfg = *cfg;
    return DN_OK;
}

static int32_t dynamics_rows(dn_env *env, bool set, const float *scales, void *stream)
{
    if (!env || !scales) return fail(DN_ERR_INVALID_ARGUMENT, "env and scales are required");
    if (!env->m.dyn.dyn) return fail(DN_ERR_BAD_STATE, "dynamics randomisation is not enabled (dn_enable_dynamics)");
    DN_HIP(copy_rows(set, env->m.dyn.dyn, scales, (size_t)env->cfg.num_envs * sizeof(float4), (hipStream_t)stream));
    return DN_OK;
}
int32_t dn_set_dynamics(dn_env *env, const float *scales, void *stream) { return dynamics_rows(env, true, scales, stream); }
int32_t dn_get_dynamics(dn_env *env, float *scales, void *stream) { return dynamics_rows(env, false, scales, stream); }

int32_t dn_get_dynamics_config(const dn_env *env, dn_dynamics_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.dyn.dyn) return 0;
    *out = env->dyn_cfg;
    return 1;
}

int32_t dn_enable_wind(dn_env *env, const dn_wind_config *cfg)
{
    if (!env || !cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    const float *rng[3] = {cfg->speed, cfg->azimuth, cfg->vertical};
    const char *names[3] = {"speed", "azimuth", "vertical"};
    for (int j = 0; j < 3; ++j) {
        const float lo = rng[j][0], hi = rng[j][1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi))
            return fail(DN_ERR_INVALID_ARGUMENT, "wind range %s = [%g, %g]: need finite lo <= hi", names[j], (double)lo, (double)hi);
    }
    if (!(cfg->speed[0] >= 0.0f)) return fail(DN_ERR_INVALID_ARGUMENT, "wind speed lo = %g: need >= 0", (double)cfg->speed[0]);
    for (int j = 0; j < 2; ++j) {
        if (!std::isfinite(cfg->gust_sigma[j]) || !(cfg->gust_sigma[j] >= 0.0f))
            return fail(DN_ERR_INVALID_ARGUMENT, "gust_sigma[%d] = %g: need finite >= 0", j, (double)cfg->gust_sigma[j]);
        if (!std::isfinite(cfg->coeff[j]) || !(cfg->coeff[j] >= 0.0f))
            return fail(DN_ERR_INVALID_ARGUMENT, "coeff[%d] = %g: need finite >= 0", j, (double)cfg->coeff[j]);
    }
    if (!std::isfinite(cfg->gust_tau) || !(cfg->gust_tau > 0.0f))
        return fail(DN_ERR_INVALID_ARGUMENT, "gust_tau = %g: need finite > 0", (double)cfg->gust_tau);
    if (const int32_t rc = check_resample_reserved(cfg->resample, cfg->reserved)) return rc;
    DN_HIP(hipSetDevice(env->cfg.device_id));
    const long long n = env->cfg.num_envs;
    DnWind &w = env->m.wind;
    // first call: wbar and g of every drone, 0 (still air) until an episode start draws or dn_set_wind writes
    if (const int32_t rc = model_storage(w.mean, (size_t)(2 * n) * sizeof(float4), "the wind", [&](float4 *mem) {
            return dn_launch_fill4(mem, make_float4(0.0f, 0.0f, 0.0f, 0.0f), 2 * n, nullptr) == hipSuccess;
        }))
        return rc;
    w.gust = w.mean + n;
    for (int j = 0; j < 2; ++j) {
        w.speed[j] = cfg->speed[j]; w.azimuth[j] = cfg->azimuth[j]; w.vertical[j] = cfg->vertical[j];
        w.sigma[j] = cfg->gust_sigma[j]; w.k[j] = cfg->coeff[j];
    }
    const double dt = 1.0 / 240.0;                              // the control step (PYB_FREQ = CTRL_FREQ = 240)
    w.a = std::exp(-dt / (double)cfg->gust_tau);
    const double root = std::sqrt(1.0 - w.a * w.a);
    w.b[0] = (double)cfg->gust_sigma[0] * root;
    w.b[1] = (double)cfg->gust_sigma[1] * root;
    w.resample = cfg->resample;
    w.gust_on = cfg->gust_sigma[0] > 0.0f || cfg->gust_sigma[1] > 0.0f;
    env->wind_cfg = *cfg;
    return DN_OK;
}

static int32_t wind_rows(dn_env *env, bool set, const float *mean, const float *gust, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is required");
    if (!env->m.wind.mean) return fail(DN_ERR_BAD_STATE, "wind is not enabled (dn_enable_wind)");
    const size_t bytes = (size_t)env->cfg.num_envs * sizeof(float4);
    DN_HIP(copy_rows(set, env->m.wind.mean, mean, bytes, (hipStream_t)stream));
    DN_HIP(copy_rows(set, env->m.wind.gust, gust, bytes, (hipStream_t)stream));
    return DN_OK;
}
int32_t dn_set_wind(dn_env *env, const float *mean, const float *gust, void *stream) { return wind_rows(env, true, mean, gust, stream); }
int32_t dn_get_wind(dn_env *env, float *mean, float *gust, void *stream) { return wind_rows(env, false, mean, gust, stream); }

int32_t dn_get_wind_config(const dn_env *env, dn_wind_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.wind.mean) return 0;
    *out = env->wind_cfg;
    return 1;
}

int32_t dn_enable_actuator(dn_env *env, const dn_actuator_config *cfg)
{
    if (!env || !cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    if (cfg->latency[0] < 0 || cfg->latency[1] > DN_MAX_LATENCY || cfg->latency[0] > cfg->latency[1])
        return fail(DN_ERR_INVALID_ARGUMENT, "actuator latency = [%d, %d]: need 0 <= lo <= hi <= %d", cfg->latency[0], cfg->latency[1], DN_MAX_LATENCY);
    const float tlo = cfg->motor_tau[0], thi = cfg->motor_tau[1];
    if (!std::isfinite(tlo) || !std::isfinite(thi) || !(tlo >= 0.0f) || !(tlo <= thi))
        return fail(DN_ERR_INVALID_ARGUMENT, "actuator motor_tau = [%g, %g]: need finite 0 <= lo <= hi", (double)tlo, (double)thi);
    for (int j = 0; j < 4; ++j)
        if (!std::isfinite(cfg->fill[j])) return fail(DN_ERR_INVALID_ARGUMENT, "actuator fill[%d] = %g: need finite", j, (double)cfg->fill[j]);
    if (const int32_t rc = check_resample_reserved(cfg->resample, cfg->reserved)) return rc;
    const int lag_on = thi > 0.0f;
    if (lag_on && env->cfg.action_type != 0)
        return fail(DN_ERR_INVALID_ARGUMENT, "the motor lag (motor_tau != [0, 0]) is built for ActionType.THRUST (action_type 0, got %d); "
                                             "the command latency works with every action type", env->cfg.action_type);
    DN_HIP(hipSetDevice(env->cfg.device_id));
    // rpm_fill: the speeds the device's own action chain gives for `fill` (dn_preprocess_action's kernel), not host arithmetic
    float4 rpm_fill;
    {
        float *tmp = nullptr;
        if (hipMalloc(&tmp, 8 * sizeof(float)) != hipSuccess) return fail(DN_ERR_OUT_OF_MEMORY, "hipMalloc(32 bytes) for the actuator's fill failed");
        float host[4];
        const bool ok = hipMemcpy(tmp, cfg->fill, 4 * sizeof(float), hipMemcpyHostToDevice) == hipSuccess
                        && dn_launch_action_chain(tmp, 1, env->cfg.normalize_actions, tmp + 4, nullptr, nullptr, nullptr) == hipSuccess
                        && hipMemcpy(host, tmp + 4, 4 * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(tmp);
        if (!ok) return fail(DN_ERR_HIP, "evaluating the action chain for the actuator's fill failed");
        rpm_fill = make_float4(host[0], host[1], host[2], host[3]);
    }
    const float4 fill = make_float4(cfg->fill[0], cfg->fill[1], cfg->fill[2], cfg->fill[3]);
    const long long n = env->cfg.num_envs;
    DnAct &a = env->m.act;
    // first call: d = 0, a = 0, r = rpm_fill, the history holds `fill`
    if (const int32_t rc = model_storage(a.hist, (size_t)n * (9 * sizeof(float4) + sizeof(float) + sizeof(int)), "the actuator", [&](float4 *mem) {
            return dn_launch_fill4(mem, fill, 8 * n, nullptr) == hipSuccess && dn_launch_fill4(mem + 8 * n, rpm_fill, n, nullptr) == hipSuccess
                   && hipMemsetAsync(mem + 9 * n, 0, (size_t)n * (sizeof(float) + sizeof(int)), nullptr) == hipSuccess;
        }))
        return rc;
    a.rpm = a.hist + 8 * n;
    a.coeff = reinterpret_cast<float *>(a.hist + 9 * n);
    a.lat = reinterpret_cast<int *>(a.coeff + n);
    a.fill = fill;
    a.rpm_fill = rpm_fill;
    a.tau[0] = tlo; a.tau[1] = thi;
    a.lat_lo = cfg->latency[0]; a.lat_hi = cfg->latency[1];
    a.resample = cfg->resample;
    a.lag_on = lag_on;
    env->act_cfg = *cfg;
    return DN_OK;
}

static int32_t actuator_rows(dn_env *env, bool set, const int32_t *latency, const float *coeff, const float *rpm, const float *history, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is required");
    const DnAct &a = env->m.act;
    if (!a.hist) return fail(DN_ERR_BAD_STATE, "the actuator is not enabled (dn_enable_actuator)");
    const size_t n = (size_t)env->cfg.num_envs;
    hipStream_t s = (hipStream_t)stream;
    DN_HIP(copy_rows(set, a.lat, latency, n * sizeof(int32_t), s));
    DN_HIP(copy_rows(set, a.coeff, coeff, n * sizeof(float), s));
    DN_HIP(copy_rows(set, a.rpm, rpm, n * sizeof(float4), s));
    DN_HIP(copy_rows(set, a.hist, history, n * 8 * sizeof(float4), s));
    return DN_OK;
}
int32_t dn_set_actuator(dn_env *env, const int32_t *latency, const float *coeff, const float *rpm, const float *history, void *stream)
{
    return actuator_rows(env, true, latency, coeff, rpm, history, stream);
}
int32_t dn_get_actuator(dn_env *env, int32_t *latency, float *coeff, float *rpm, float *history, void *stream)
{
    return actuator_rows(env, false, latency, coeff, rpm, history, stream);
}

int32_t dn_get_actuator_config(const dn_env *env, dn_actuator_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.act.hist) return 0;
    *out = env->act_cfg;
    return 1;
}

int32_t dn_enable_sensor(dn_env *env, const dn_sensor_config *cfg)
{
    if (!env || !cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    if (cfg->latency[0] < 0 || cfg->latency[1] > DN_MAX_LATENCY || cfg->latency[0] > cfg->latency[1])
        return fail(DN_ERR_INVALID_ARGUMENT, "sensor latency = [%d, %d]: need 0 <= lo <= hi <= %d", cfg->latency[0], cfg->latency[1], DN_MAX_LATENCY);
    bool any_amp = false;
    for (int j = 0; j < DN_OBS_DIM; ++j) {
        if (!std::isfinite(cfg->bias_amp[j]) || !(cfg->bias_amp[j] >= 0.0f))
            return fail(DN_ERR_INVALID_ARGUMENT, "sensor bias_amp[%d] = %g: need finite >= 0", j, (double)cfg->bias_amp[j]);
        any_amp = any_amp || cfg->bias_amp[j] > 0.0f;
    }
    if (const int32_t rc = check_resample_reserved(cfg->resample, cfg->reserved)) return rc;
    DN_HIP(hipSetDevice(env->cfg.device_id));
    const long long n = env->cfg.num_envs;
    const size_t quads = (size_t)n * (DN_SENS_SLOTS * 4 + 4);
    const size_t bytes = quads * sizeof(float4) + (size_t)n * sizeof(int);
    DnSens &s = env->m.sens;
    if (s.ring) DN_HIP(hipDeviceSynchronize());     // launches in flight carry the previous configuration
    else s.base = 0;
    // first call: d = 0, b = 0, an all-zero ring
    if (const int32_t rc = model_storage(s.ring, bytes, "the sensor model", [&](float4 *mem) { return hipMemsetAsync(mem, 0, bytes, nullptr) == hipSuccess; }))
        return rc;
    s.bias = s.ring + (size_t)n * DN_SENS_SLOTS * 4;
    s.lat = reinterpret_cast<int *>(s.ring + quads);
    for (int j = 0; j < DN_OBS_DIM; ++j) s.amp[j] = cfg->bias_amp[j];
    s.lat_lo = cfg->latency[0]; s.lat_hi = cfg->latency[1];
    s.resample = cfg->resample;
    s.lat_on = cfg->latency[1] > 0 || !cfg->resample;
    s.bias_on = any_amp || !cfg->resample;
    env->sens_cfg = *cfg;
    return DN_OK;
}

static int32_t sensor_rows(dn_env *env, bool set, const int32_t *latency, const float *bias, const float *history, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is required");
    const DnSens &sn = env->m.sens;
    if (!sn.ring) return fail(DN_ERR_BAD_STATE, "the sensor model is not enabled (dn_enable_sensor)");
    hipStream_t s = (hipStream_t)stream;
    DN_HIP(copy_rows(set, sn.lat, latency, (size_t)env->cfg.num_envs * sizeof(int32_t), s));
    // the bias and the history are laid out for the kernels (quads, a ring): a kernel of their own, which takes the direction
    if (bias) DN_HIP(dn_launch_sensor_bias(sn, env->cfg.num_envs, const_cast<float *>(bias), set, s));
    if (history) DN_HIP(dn_launch_sensor_history(env->p, sn, const_cast<float *>(history), set, s));
    return DN_OK;
}
int32_t dn_set_sensor(dn_env *env, const int32_t *latency, const float *bias, const float *history, void *stream)
{
    return sensor_rows(env, true, latency, bias, history, stream);
}
int32_t dn_get_sensor(dn_env *env, int32_t *latency, float *bias, float *history, void *stream)
{
    return sensor_rows(env, false, latency, bias, history, stream);
}

int32_t dn_get_sensor_config(const dn_env *env, dn_sensor_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.sens.ring) return 0;
    *out = env->sens_cfg;
    return 1;
}

int32_t dn_enable_privileged(dn_env *env, const dn_privileged_config *cfg)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    // the mask first: it needs no env (and no device) to be wrong
    if (cfg->groups == 0 || (cfg->groups & ~DN_PRIV_ALL))
        return fail(DN_ERR_INVALID_ARGUMENT, "privileged groups = 0x%x: need a non-empty mask of DN_PRIV_OBS | DYN | WIND | ACT | SENS (0x%x)",
                    (unsigned)cfg->groups, (unsigned)DN_PRIV_ALL);
    if (cfg->reserved != 0) return fail(DN_ERR_INVALID_ARGUMENT, "reserved must be 0 (got %d)", cfg->reserved);
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    if (env->m.priv.groups) {                       // launches in flight carry the previous mask
        DN_HIP(hipSetDevice(env->cfg.device_id));
        DN_HIP(hipDeviceSynchronize());
    }
    env->m.priv.groups = cfg->groups;
    env->priv_cfg = *cfg;
    return DN_OK;
}

int32_t dn_get_privileged_config(const dn_env *env, dn_privileged_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.priv.groups) return 0;
    *out = env->priv_cfg;
    return 1;
}

int32_t dn_bind_privileged(dn_env *env, float *rows, float *terminal_rows, int64_t capacity_steps)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is required");
    DnPriv &pv = env->m.priv;
    if (!pv.groups) return fail(DN_ERR_BAD_STATE, "the privileged observations are not enabled (dn_enable_privileged)");
    return bind_rows(pv.rows, pv.term, pv.cap, rows, terminal_rows, capacity_steps);
}

int32_t dn_enable_goal(dn_env *env, const dn_goal_config *cfg)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    // the frame first: it needs no env (and no device) to be wrong
    if (cfg->frame != DN_GOAL_FRAME_WORLD && cfg->frame != DN_GOAL_FRAME_BODY)
        return fail(DN_ERR_INVALID_ARGUMENT, "goal frame = %d: need DN_GOAL_FRAME_WORLD (0) or DN_GOAL_FRAME_BODY (1)", cfg->frame);
    if (cfg->reserved != 0) return fail(DN_ERR_INVALID_ARGUMENT, "reserved must be 0 (got %d)", cfg->reserved);
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    if (env->m.goal.on) {                           // launches in flight carry the previous frame
        DN_HIP(hipSetDevice(env->cfg.device_id));
        DN_HIP(hipDeviceSynchronize());
    }
    env->m.goal.on = 1;
    env->m.goal.frame = cfg->frame;
    env->goal_cfg = *cfg;
    return DN_OK;
}

int32_t dn_get_goal_config(const dn_env *env, dn_goal_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.goal.on) return 0;
    *out = env->goal_cfg;
    return 1;
}

int32_t dn_bind_goal(dn_env *env, float *rows, float *terminal_rows, int64_t capacity_steps)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is required");
    DnGoal &g = env->m.goal;
    if (!g.on) return fail(DN_ERR_BAD_STATE, "the goal observations are not enabled (dn_enable_goal)");
    return bind_rows(g.rows, g.term, g.cap, rows, terminal_rows, capacity_steps);
}

// ---- track bank ----
int32_t dn_enable_tracks(dn_env *env, const dn_track_bank_config *cfg)
{
    if (!env || !cfg) return fail(DN_ERR_INVALID_ARGUMENT, "env and cfg are required");
    const dn_config &c = env->cfg;
    if (c.circle) return fail(DN_ERR_INVALID_ARGUMENT, "dn_enable_tracks: a circle env has no waypoint corridor table to bank (circle = %d)", c.circle);
    if (c.random_spawn) return fail(DN_ERR_INVALID_ARGUMENT, "dn_enable_tracks: refused with random_spawn (the spawn draw reads the one track's lines)");
    if (cfg->num_tracks < 1 || cfg->num_tracks > DN_MAX_TRACKS)
        return fail(DN_ERR_INVALID_ARGUMENT, "num_tracks must be in 1..%d (got %d)", DN_MAX_TRACKS, cfg->num_tracks);
    const int T = cfg->num_tracks;
    int total = 0;
    for (int t = 0; t < T; ++t) {
        if (cfg->num_waypoints[t] < 1 || cfg->num_waypoints[t] > DN_MAX_WAYPOINTS)
            return fail(DN_ERR_INVALID_ARGUMENT, "track %d: num_waypoints must be in 1..%d (got %d)", t, DN_MAX_WAYPOINTS, cfg->num_waypoints[t]);
        total += cfg->num_waypoints[t];
    }
    if (total > DN_MAX_WAYPOINTS)
        return fail(DN_ERR_INVALID_ARGUMENT, "the bank has %d waypoints in all: at most %d (the corridor table the kernels stage)", total, DN_MAX_WAYPOINTS);
    for (int j = 0; j < total * 3; ++j)
        if (!std::isfinite(cfg->waypoints[j])) return fail(DN_ERR_INVALID_ARGUMENT, "bank waypoint %d is not finite", j / 3);
    double sum = 0.0, cdf[DN_MAX_TRACKS] = {};
    for (int t = 0; t < T; ++t) {
        const float w = cfg->weight[t];
        if (!std::isfinite(w) || w < 0.0f) return fail(DN_ERR_INVALID_ARGUMENT, "weight[%d] = %g: need finite and >= 0", t, (double)w);
        sum += (double)w;
        cdf[t] = sum;                                   // S_t: float64 partial sums of the float32 weights, in index order
    }
    if (!(sum > 0.0)) return fail(DN_ERR_INVALID_ARGUMENT, "every weight is zero: no track could be drawn");
    for (int t = 0; t < T; ++t) cdf[t] = cdf[t] / sum;
    if (const int32_t rc = check_resample_reserved(cfg->resample, cfg->reserved)) return rc;
    if (cfg->num_waypoints[0] != c.num_waypoints || memcmp(cfg->waypoints, c.waypoints, sizeof(double) * 3 * (size_t)c.num_waypoints) != 0)
        return fail(DN_ERR_INVALID_ARGUMENT, "track 0 of the bank must be the track of dn_config (the same count and bit-equal waypoints)");
    DnTrack &tk = env->m.track;
    if (tk.track) {
        const dn_track_bank_config &was = env->track_cfg;
        if (was.num_tracks != T || memcmp(was.num_waypoints, cfg->num_waypoints, sizeof(int32_t) * (size_t)T) != 0 ||
            memcmp(was.waypoints, cfg->waypoints, sizeof(double) * 3 * (size_t)total) != 0)
            return fail(DN_ERR_INVALID_ARGUMENT, "dn_enable_tracks: the bank's geometry (tracks, counts, waypoints) cannot change once enabled; weights and resample can");
    }
    DN_HIP(hipSetDevice(c.device_id));
    DN_HIP(hipDeviceSynchronize());                     // launches in flight read the table, the weights and the ground-contact switch
    const long long n = c.num_envs;
    const size_t off_cdf = track_off_cdf(n), off_bw = off_cdf + DN_MAX_TRACKS * sizeof(double), off_count = off_bw + DN_MAX_TRACKS * sizeof(int);
    const size_t bytes = off_count + DN_MAX_TRACKS * 5 * sizeof(unsigned long long);
    const bool first = tk.track == nullptr;
    float4 *mem = reinterpret_cast<float4 *>(tk.track);
    // first call: every drone on track 0, no episode finished yet, zero counters
    if (const int32_t rc = model_storage(mem, bytes, "the track bank", [&](float4 *d) {
            char *b = reinterpret_cast<char *>(d);
            return hipMemsetAsync(b, 0, bytes, nullptr) == hipSuccess &&
                   hipMemsetAsync(b + (size_t)n * sizeof(int), 0xFF, (size_t)n * sizeof(int), nullptr) == hipSuccess;
        }))
        return rc;
    char *base = reinterpret_cast<char *>(mem);
    int bw[DN_MAX_TRACKS] = {};
    bool contact = false;
    std::vector<double> t64(DN_MAX_WAYPOINTS * DN_T_STRIDE, 0.0);
    std::vector<float> t32(DN_MAX_WAYPOINTS * DN_T_STRIDE, 0.0f);
    for (int t = 0, row = 0; t < T; row += cfg->num_waypoints[t], ++t) {
        const dn_config one = track_as_config(c, *cfg, t, row);
        build_table(one, t64.data() + (size_t)row * DN_T_STRIDE);       // the rows of the single-track configuration: the definition
        contact = contact || ground_contact_reachable(one);
        bw[t] = row | (cfg->num_waypoints[t] << 8);
    }
    for (size_t j = 0; j < t64.size(); ++j) t32[j] = (float)t64[j];
    if ((first && (hipMemcpy(env->tab64, t64.data(), t64.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                   hipMemcpy(env->tab32, t32.data(), t32.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) ||
        hipMemcpy(base + off_cdf, cdf, sizeof cdf, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + off_bw, bw, sizeof bw, hipMemcpyHostToDevice) != hipSuccess) {
        if (first) (void)hipFree(mem);
        return fail(DN_ERR_HIP, "uploading the track bank failed");
    }
    tk.track = reinterpret_cast<int *>(base);
    tk.finished = tk.track + n;
    tk.cdf = reinterpret_cast<const double *>(base + off_cdf);
    tk.bw = reinterpret_cast<const int *>(base + off_bw);
    tk.count = reinterpret_cast<unsigned long long *>(base + off_count);
    tk.num_tracks = T;
    tk.total = total;
    tk.resample = cfg->resample;
    if (env->ground_contact_auto) {                     // DN_GROUND_CONTACT_AUTO: on if any track of the bank needs the term
        env->cfg.ground_contact = contact ? 1 : 0;
        env->p.ground_contact = contact ? 1 : 0;
    }
    env->track_cfg = *cfg;
    return DN_OK;
}

int32_t dn_set_tracks(dn_env *env, const int32_t *track, void *stream)
{
    if (!env || !track) return fail(DN_ERR_INVALID_ARGUMENT, "env and track are required");
    if (!env->m.track.track) return fail(DN_ERR_BAD_STATE, "the track bank is not enabled (dn_enable_tracks)");
    DN_HIP(copy_rows(true, env->m.track.track, track, (size_t)env->cfg.num_envs * sizeof(int32_t), (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_get_tracks(dn_env *env, int32_t *track, int32_t *finished, void *stream)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is required");
    if (!env->m.track.track) return fail(DN_ERR_BAD_STATE, "the track bank is not enabled (dn_enable_tracks)");
    const size_t bytes = (size_t)env->cfg.num_envs * sizeof(int32_t);
    DN_HIP(copy_rows(false, env->m.track.track, track, bytes, (hipStream_t)stream));
    DN_HIP(copy_rows(false, env->m.track.finished, finished, bytes, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_get_track_stats(dn_env *env, int64_t *out, int32_t reset)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    const DnTrack &tk = env->m.track;
    if (!tk.track) return fail(DN_ERR_BAD_STATE, "the track bank is not enabled (dn_enable_tracks)");
    DN_HIP(hipSetDevice(env->cfg.device_id));
    DN_HIP(hipDeviceSynchronize());
    const size_t bytes = (size_t)tk.num_tracks * 5 * sizeof(int64_t);
    DN_HIP(hipMemcpy(out, tk.count, bytes, hipMemcpyDeviceToHost));
    if (reset) DN_HIP(hipMemset(tk.count, 0, bytes));
    return DN_OK;
}

int32_t dn_get_track_bank_config(const dn_env *env, dn_track_bank_config *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    if (!env->m.track.track) return fail(DN_ERR_BAD_STATE, "the track bank is not enabled (dn_enable_tracks)");
    *out = env->track_cfg;
    return DN_OK;
}

int32_t dn_get_step_count(const dn_env *env, uint64_t *out)
{
    if (!env || !out) return fail(DN_ERR_INVALID_ARGUMENT, "env and out are required");
    // the counter lives on the device (it advances under hipGraph replay too); every tile carries the same value
    DN_HIP(hipSetDevice(env->cfg.device_id));
    DN_HIP(hipDeviceSynchronize());
    unsigned long long v = 0;
    DN_HIP(hipMemcpy(&v, &env->p.st.stats[0].step_count, sizeof v, hipMemcpyDeviceToHost));
    *out = v;
    return DN_OK;
}

int32_t dn_set_step_count(dn_env *env, uint64_t value)
{
    if (!env) return fail(DN_ERR_INVALID_ARGUMENT, "env is NULL");
    DN_HIP(hipSetDevice(env->cfg.device_id));
    DN_HIP(hipDeviceSynchronize());
    if (env->m.sens.ring) {                   // the sensor ring's slots are keyed by the vector step: the rows stay where they are, the offset moves
        unsigned long long old = 0;
        DN_HIP(hipMemcpy(&old, &env->p.st.stats[0].step_count, sizeof old, hipMemcpyDeviceToHost));
        env->m.sens.base = (int)(((unsigned)env->m.sens.base + (unsigned)old - (unsigned)value) & (DN_SENS_SLOTS - 1u));
    }
    DN_HIP(dn_launch_set_step_count(env->p.st.stats, env->blocks, value, nullptr));
    DN_HIP(hipStreamSynchronize(nullptr));
    return DN_OK;
}

int32_t dn_policy_sample(dn_env *env, const float *mean, const float *log_std, uint64_t seed, int32_t deterministic, float *actions,
                         float *clipped, float *log_prob, void *stream)
{
    if (!env || !mean || !log_std || !actions || !clipped || !log_prob)
        return fail(DN_ERR_INVALID_ARGUMENT, "env, mean, log_std, actions, clipped and log_prob are required");
    if (((uintptr_t)mean | (uintptr_t)actions | (uintptr_t)clipped) & 15u)
        return fail(DN_ERR_INVALID_ARGUMENT, "mean, actions and clipped must be 16-byte aligned");
    DN_HIP(dn_launch_policy_sample(env->p, mean, log_std, seed, deterministic, actions, clipped, log_prob, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_squashed_sample(dn_env *env, const float *mu_log_std, uint64_t seed, int32_t deterministic, float *actions, float *log_prob,
                           void *stream)
{
    if (!env || !mu_log_std || !actions) return fail(DN_ERR_INVALID_ARGUMENT, "env, mu_log_std and actions are required");
    if (((uintptr_t)mu_log_std | (uintptr_t)actions) & 15u)
        return fail(DN_ERR_INVALID_ARGUMENT, "mu_log_std and actions must be 16-byte aligned");
    DN_HIP(dn_launch_squashed_sample(env->p, mu_log_std, seed, deterministic, actions, log_prob, (hipStream_t)stream));
    return DN_OK;
}

}  // extern "C"
