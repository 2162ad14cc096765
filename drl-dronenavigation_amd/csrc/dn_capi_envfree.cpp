// dn_capi_envfree.cpp -- the entry points of include/dronenav.h that take a device_id and no dn_env: the rollout glue, the history rows,
// the two fleet normalisers, the minibatches, the PPO loss, the optimiser step, the replay minibatches, the SAC loss heads, the
// training passes of the Tanh and of the SAC networks, the Polyak update and the LSTM layer.
//
// Every entry point validates its arguments, turns HIP failures into dn_status codes + the thread-local message of dn_capi.cpp
// (dn_capi_fail.h), and never falls back to a CPU implementation.
#include "dn_argcheck.h"
#include "dn_capi_fail.h"
#include "dn_internal.h"
#include "dn_permute.h"
#include "dn_replay_draw.h"
#include "dn_row_sums.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

// The refusals that several entry points word alike, each stated once: DN_OK, or the status fail() returns.
static int32_t scratch_too_small(int64_t have, int64_t need, const char *sizer)
{
    return fail(DN_ERR_INVALID_ARGUMENT, "scratch_bytes is too small: %lld, %s gives %lld", (long long)have, sizer, (long long)need);
}
static int32_t steps_ok(int64_t k, int64_t n)
{
    return k < 1 || n < 1 ? fail(DN_ERR_INVALID_ARGUMENT, "k and n must be >= 1 (got %lld, %lld)", (long long)k, (long long)n) : DN_OK;
}
static int32_t clip_ok(float clip)
{
    return !(clip > 0.0f) ? fail(DN_ERR_INVALID_ARGUMENT, "clip must be > 0, +inf for no clip (got %g)", (double)clip) : DN_OK;
}
static int32_t epsilon_ok(double epsilon)
{
    return !(epsilon >= 0.0) ? fail(DN_ERR_INVALID_ARGUMENT, "epsilon must be >= 0 (got %g)", epsilon) : DN_OK;
}
static int32_t reserved_ok(int32_t reserved)
{
    return reserved != 0 ? fail(DN_ERR_INVALID_ARGUMENT, "reserved must be 0 (got %d)", reserved) : DN_OK;
}

extern "C" {

int32_t dn_compact_done(const uint64_t *done_mask, int64_t num_envs, int32_t *indices, int32_t *count,
                        int32_t device_id, void *stream)
{
    if (!done_mask || !indices || !count || num_envs < 1)
        return fail(DN_ERR_INVALID_ARGUMENT, "done_mask, indices, count are required and num_envs >= 1");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_compact((const unsigned long long *)done_mask, num_envs, indices, count, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_pack_done(const uint64_t *done_mask, int64_t num_envs, const float *terminal_obs, const float *ep_return, const int32_t *ep_length,
                     const uint8_t *truncated, const int32_t *found_targets, int32_t *indices, int32_t *count, float *packed,
                     int32_t device_id, void *stream)
{
    if (!done_mask || !terminal_obs || !ep_return || !ep_length || !truncated || !found_targets || !indices || !count || !packed || num_envs < 1)
        return fail(DN_ERR_INVALID_ARGUMENT, "every pointer is required and num_envs >= 1");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_compact_pack((const unsigned long long *)done_mask, num_envs, terminal_obs, ep_return, ep_length, truncated, found_targets,
                                  indices, count, packed, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_stream_copy(void *dst, const void *src, int64_t bytes, int32_t device_id, void *stream)
{
    if (!dst || !src || bytes < 16 || (bytes & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15))
        return fail(DN_ERR_INVALID_ARGUMENT, "dst, src: 16-byte aligned device pointers; bytes: a positive multiple of 16");
    DN_HIP(hipSetDevice(device_id));
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || cus < 1) cus = 256;
    DN_HIP(dn_launch_stream_copy(dst, src, bytes / 16, cus, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_preprocess_action(const float *actions, int64_t num_envs, int32_t normalize_actions, float *rpm, float *forces,
                             float *z_torque, int32_t device_id, void *stream)
{
    if (!actions || num_envs < 1) return fail(DN_ERR_INVALID_ARGUMENT, "actions is required and num_envs >= 1");
    if (!rpm && !forces && !z_torque) return fail(DN_ERR_INVALID_ARGUMENT, "at least one output buffer is required");
    if (((uintptr_t)actions & 15u) || ((uintptr_t)rpm & 15u) || ((uintptr_t)forces & 15u))
        return fail(DN_ERR_INVALID_ARGUMENT, "actions, rpm and forces must be 16-byte aligned");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_action_chain(actions, num_envs, normalize_actions, rpm, forces, z_torque, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_add_bootstrap(float *reward, const float *terminal_value, const uint8_t *truncated, double gamma, int64_t num_envs,
                         int32_t device_id, void *stream)
{
    if (!reward || !terminal_value || !truncated || num_envs < 1)
        return fail(DN_ERR_INVALID_ARGUMENT, "reward, terminal_value, truncated are required and num_envs >= 1");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_add_bootstrap(reward, terminal_value, truncated, (float)gamma, num_envs, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_mlp_forward(const dn_mlp_net *nets, int32_t num_nets, const float *obs, const uint8_t *row_mask, int64_t num_envs,
                       int32_t obs_dim, int32_t device_id, void *stream)
{
    if (!nets || !obs) return fail(DN_ERR_INVALID_ARGUMENT, "nets and obs are required");
    if (num_nets < 1 || num_nets > 2) return fail(DN_ERR_INVALID_ARGUMENT, "num_nets must be 1 or 2 (got %d)", num_nets);
    if (num_envs < 1) return fail(DN_ERR_INVALID_ARGUMENT, "num_envs must be >= 1");
    for (int k = 0; k < num_nets; ++k) {
        const dn_mlp_net &n = nets[k];
        if (n.arch != DN_MLP_ARCH_PPO && n.arch != DN_MLP_ARCH_SAC)
            return fail(DN_ERR_INVALID_ARGUMENT, "net %d: arch must be 0 (PPO 512-512-256 Tanh) or 1 (SAC actor 256-256 ReLU)", k);
        // rows of up to 64 columns for the PPO networks (dn_mlp_wide.hip beyond 16), of up to 16 for the SAC actor
        if (n.arch == DN_MLP_ARCH_PPO ? dn_mlp_ks1(obs_dim) == 0 : dn_mlp_ks1(obs_dim) != 1)
            return fail(DN_ERR_INVALID_ARGUMENT, "obs_dim must be in 1..%d for %s (got %d)", n.arch == DN_MLP_ARCH_PPO ? 64 : 16,
                        n.arch == DN_MLP_ARCH_PPO ? "the PPO networks" : "the SAC actor", obs_dim);
        const bool three = n.arch == DN_MLP_ARCH_PPO;
        if (!n.w1 || !n.w2 || (three && !n.w3) || !n.wh || !n.b1 || !n.b2 || (three && !n.b3) || !n.bh || !n.out)
            return fail(DN_ERR_INVALID_ARGUMENT, "net %d: every weight, bias and output pointer is required", k);
        if (n.out_dim < 1 || n.out_dim > 32) return fail(DN_ERR_INVALID_ARGUMENT, "net %d: out_dim must be in 1..32", k);
        if (n.grade < 0 || n.grade > 2) return fail(DN_ERR_INVALID_ARGUMENT, "net %d: grade must be 0 (bf16), 1 (fp32 grade) or 2 (fp16)", k);
        if (n.grade != nets[0].grade || n.arch != nets[0].arch)
            return fail(DN_ERR_INVALID_ARGUMENT, "all networks of one call must share grade and arch");
        if (((uintptr_t)n.w1 | (uintptr_t)n.w2 | (three ? (uintptr_t)n.w3 : 0) | (uintptr_t)n.wh) & 15u)
            return fail(DN_ERR_INVALID_ARGUMENT, "net %d: packed weights must be 16-byte aligned", k);
    }
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_mlp(nets, num_nets, obs, row_mask, num_envs, obs_dim, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_gae(const float *rewards, const float *values, const uint8_t *dones, const float *last_values,
               const uint8_t *last_dones, int64_t n_steps, int64_t n_envs, double gamma, double gae_lambda,
               float *advantages, float *returns, int32_t device_id, void *stream)
{
    if (!rewards || !values || !dones || !last_values || !last_dones || !advantages || !returns)
        return fail(DN_ERR_INVALID_ARGUMENT, "all buffers are required");
    if (n_steps < 1 || n_envs < 1) return fail(DN_ERR_INVALID_ARGUMENT, "n_steps and n_envs must be >= 1");
    DN_HIP(hipSetDevice(device_id));
    // gamma and gamma*gae_lambda are Python floats multiplied into float32 tensors (cleanRLPPO.py:245-246)
    DN_HIP(dn_launch_gae(rewards, values, dones, last_values, last_dones, n_steps, n_envs, (float)gamma,
                         (float)(gamma * gae_lambda), advantages, returns, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_history_width(const dn_history_config *cfg)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (cfg->reserved != 0) return fail(DN_ERR_INVALID_ARGUMENT, "dn_history_config.reserved must be 0 (got %d)", cfg->reserved);
    if (cfg->frames < 1 || cfg->frames > 4) return fail(DN_ERR_INVALID_ARGUMENT, "frames must be in 1..4 (got %d)", cfg->frames);
    if (cfg->actions < 0 || cfg->actions > 4) return fail(DN_ERR_INVALID_ARGUMENT, "actions must be in 0..4 (got %d)", cfg->actions);
    if (cfg->extra_dim < 0) return fail(DN_ERR_INVALID_ARGUMENT, "extra_dim must be >= 0 (got %d)", cfg->extra_dim);
    const int w = dn_history_row_width(cfg->frames, cfg->actions, cfg->extra_dim);
    if (w == 0)
        return fail(DN_ERR_INVALID_ARGUMENT, "the row of 13 x %d + 4 x %d + %d columns is wider than 64, the policy kernels' limit", cfg->frames,
                    cfg->actions, cfg->extra_dim);
    return w;
}

int32_t dn_stack_history(const dn_history_config *cfg, int64_t k, int64_t n, const float *prev, const float *obs, const float *actions,
                         const uint8_t *done, const float *terminal_obs, const float *extra, const float *terminal_extra, float *rows,
                         float *terminal_rows, int32_t device_id, void *stream)
{
    const int32_t w = dn_history_width(cfg);
    if (w < 0) return w;
    if (const int32_t rc = steps_ok(k, n)) return rc;
    if (k > 1 && n % 4) return fail(DN_ERR_INVALID_ARGUMENT, "n must be a multiple of 4 for k > 1, as for dn_step_many (got %lld)", (long long)n);
    if (!obs || !rows) return fail(DN_ERR_INVALID_ARGUMENT, "obs and rows are required");
    if (((uintptr_t)rows | (uintptr_t)terminal_rows | (uintptr_t)prev) & 15u)
        return fail(DN_ERR_INVALID_ARGUMENT, "prev, rows and terminal_rows must be 16-byte aligned");
    if (terminal_rows && !terminal_obs) return fail(DN_ERR_INVALID_ARGUMENT, "terminal_rows needs terminal_obs");
    if (done && !actions)
        return fail(DN_ERR_INVALID_ARGUMENT, "done needs actions (actions = NULL is the reset call, in which no episode ends)");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_history(cfg->frames, cfg->actions, cfg->extra_dim, k, n, prev, obs, actions, done, terminal_obs, extra, terminal_extra,
                             rows, terminal_rows, (hipStream_t)stream));
    return DN_OK;
}

// ---- dn_rownorm: one RunningMeanStd over the fleet per row kind (Sol/Model/Environments/normalize.py:10-47) ---------------------------
static int32_t rownorm_config_ok(const dn_rownorm_config *cfg)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (cfg->width < 1 || cfg->width > DN_ROWNORM_MAX_WIDTH)
        return fail(DN_ERR_INVALID_ARGUMENT, "width must be in 1..%d (got %d)", DN_ROWNORM_MAX_WIDTH, cfg->width);
    if (const int32_t rc = clip_ok(cfg->clip)) return rc;
    return epsilon_ok(cfg->epsilon);
}

/* normalize.py:10-47: the state of one RunningMeanStd of `width` columns -- count, mean[width], var[width] */
int64_t dn_rownorm_state_doubles(int32_t width)
{
    if (width < 1 || width > DN_ROWNORM_MAX_WIDTH) return fail(DN_ERR_INVALID_ARGUMENT, "width must be in 1..%d (got %d)", DN_ROWNORM_MAX_WIDTH, width);
    return 1 + 2 * (int64_t)width;
}

/* normalize.py:10-47 in batch form: what dn_rownorm keeps between its launches (dn_internal.h dn_rownorm_scratch_doubles) */
int64_t dn_rownorm_scratch_bytes(int64_t k, int64_t n, int32_t width)
{
    const long long d = dn_rownorm_scratch_doubles(k, n, width);
    if (d == 0) return fail(DN_ERR_INVALID_ARGUMENT, "width must be in 1..%d and k, n >= 1 (got width %d, k %lld, n %lld)", DN_ROWNORM_MAX_WIDTH,
                            width, (long long)k, (long long)n);
    return (d * 8 + 15) / 16 * 16;
}

/* RunningMeanStd.__init__ (normalize.py:10-17): count 1e-4, mean 0, var 1 */
int32_t dn_rownorm_init(const dn_rownorm_config *cfg, double *stats, int32_t device_id, void *stream)
{
    if (const int32_t rc = rownorm_config_ok(cfg)) return rc;
    if (!stats) return fail(DN_ERR_INVALID_ARGUMENT, "stats is required");
    if ((uintptr_t)stats & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "stats must be 8-byte aligned");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_rownorm_init(cfg->width, stats, (hipStream_t)stream));
    return DN_OK;
}

/* RunningMeanStd.update + update_mean_var_count_from_moments (normalize.py:10-47) with the N rows of a step as the batch, then the
 * normalised rows */
int32_t dn_rownorm(const dn_rownorm_config *cfg, double *stats, int64_t k, int64_t n, const float *rows, float *out, int32_t update,
                   void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = rownorm_config_ok(cfg)) return rc;
    if (!stats || !rows || !scratch) return fail(DN_ERR_INVALID_ARGUMENT, "stats, rows and scratch are required");
    if (const int32_t rc = steps_ok(k, n)) return rc;
    if (update != 0 && update != 1) return fail(DN_ERR_INVALID_ARGUMENT, "update must be 0 or 1 (got %d)", update);
    if (!update && !out) return fail(DN_ERR_INVALID_ARGUMENT, "out is required with update = 0 (there is nothing else to do)");
    const int64_t need = dn_rownorm_scratch_bytes(k, n, cfg->width);
    if (need <= 0) return fail(DN_ERR_INVALID_ARGUMENT, "k x n = %lld x %lld rows are more than one call takes", (long long)k, (long long)n);
    if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_rownorm_scratch_bytes");
    if (((uintptr_t)stats | (uintptr_t)scratch) & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "stats and scratch must be 8-byte aligned");
    if (((uintptr_t)rows | (uintptr_t)out) & 3u) return fail(DN_ERR_INVALID_ARGUMENT, "rows and out must be 4-byte aligned");
    const uintptr_t bytes = (uintptr_t)k * (uintptr_t)n * (uintptr_t)cfg->width * sizeof(float);
    if (out != rows && dn_ranges_overlap(rows, bytes, out, bytes))
        return fail(DN_ERR_INVALID_ARGUMENT, "out overlaps rows: it must be rows itself (in place) or apart from it");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_rownorm(cfg->width, cfg->clip, cfg->epsilon, stats, k, n, rows, out, update, (double *)scratch, (hipStream_t)stream));
    return DN_OK;
}

// ---- dn_retnorm: one discounted return per drone, one RunningMeanStd of the returns over the fleet (normalize.py:10-47) ----------------
static int32_t retnorm_config_ok(const dn_retnorm_config *cfg)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (!(cfg->gamma >= 0.0 && cfg->gamma <= 1.0)) return fail(DN_ERR_INVALID_ARGUMENT, "gamma must be in [0, 1] (got %g)", cfg->gamma);
    if (const int32_t rc = clip_ok(cfg->clip)) return rc;
    if (const int32_t rc = epsilon_ok(cfg->epsilon)) return rc;
    return reserved_ok(cfg->reserved);
}

/* normalize.py:10-47 in batch form: what dn_retnorm keeps between its launches (dn_internal.h dn_retnorm_scratch_doubles) */
int64_t dn_retnorm_scratch_bytes(int64_t k, int64_t n)
{
    const long long d = dn_retnorm_scratch_doubles(k, n);
    if (d == 0) return fail(DN_ERR_INVALID_ARGUMENT, "k and n must be >= 1 and k x n within one call (got k %lld, n %lld)", (long long)k, (long long)n);
    return d * 8;
}

/* RunningMeanStd.__init__ (normalize.py:10-17): count 1e-4, mean 0, var 1; the returns start at 0 */
int32_t dn_retnorm_init(double *stats, double *returns, int64_t n, int32_t device_id, void *stream)
{
    if (!stats && !returns) return fail(DN_ERR_INVALID_ARGUMENT, "stats or returns is required (there is nothing else to do)");
    if (returns && n < 1) return fail(DN_ERR_INVALID_ARGUMENT, "n must be >= 1 (got %lld)", (long long)n);
    if (returns && n > (1ll << 38)) return fail(DN_ERR_INVALID_ARGUMENT, "n = %lld returns are more than one call takes", (long long)n);
    if (((uintptr_t)stats | (uintptr_t)returns) & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "stats and returns must be 8-byte aligned");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_retnorm_init(stats, returns, n, (hipStream_t)stream));
    return DN_OK;
}

/* The discounted returns, RunningMeanStd.update + update_mean_var_count_from_moments (normalize.py:10-47) with the N returns of a step as
 * the batch, then the scaled rewards */
int32_t dn_retnorm(const dn_retnorm_config *cfg, double *stats, double *returns, int64_t k, int64_t n, const float *rewards,
                   const uint8_t *done, float *out, int32_t update, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = retnorm_config_ok(cfg)) return rc;
    if (update != 0 && update != 1) return fail(DN_ERR_INVALID_ARGUMENT, "update must be 0 or 1 (got %d)", update);
    if (!stats || !rewards) return fail(DN_ERR_INVALID_ARGUMENT, "stats and rewards are required");
    if (update && (!returns || !done || !scratch))
        return fail(DN_ERR_INVALID_ARGUMENT, "returns, done and scratch are required with update = 1");
    if (!update && !out) return fail(DN_ERR_INVALID_ARGUMENT, "out is required with update = 0 (there is nothing else to do)");
    if (const int32_t rc = steps_ok(k, n)) return rc;
    if ((uintptr_t)stats & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "stats must be 8-byte aligned");
    if (update) {
        const int64_t need = dn_retnorm_scratch_bytes(k, n);
        if (need <= 0) return fail(DN_ERR_INVALID_ARGUMENT, "k x n = %lld x %lld rewards are more than one call takes", (long long)k, (long long)n);
        if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_retnorm_scratch_bytes");
        if (((uintptr_t)returns | (uintptr_t)scratch) & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "returns and scratch must be 8-byte aligned");
    }
    if (!dn_retnorm_grids_ok(k, n))
        return fail(DN_ERR_INVALID_ARGUMENT, "k x n = %lld x %lld rewards need a grid of more than 2^31 - 1 workgroups", (long long)k, (long long)n);
    const uintptr_t bytes = (uintptr_t)k * (uintptr_t)n * sizeof(float);
    if (out != rewards && dn_ranges_overlap(rewards, bytes, out, bytes))
        return fail(DN_ERR_INVALID_ARGUMENT, "out overlaps rewards: it must be rewards itself (in place) or apart from it");
    if (((uintptr_t)rewards | (uintptr_t)out) & 3u) return fail(DN_ERR_INVALID_ARGUMENT, "rewards and out must be 4-byte aligned");
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_retnorm(cfg->gamma, cfg->epsilon, cfg->clip, stats, update ? returns : nullptr, k, n, rewards, update ? done : nullptr, out,
                             update, update ? (double *)scratch : nullptr, (hipStream_t)stream));
    return DN_OK;
}

// ---- dn_minibatch: SB3 RolloutBuffer.get and PPO's advantage normalisation [from recall] on the step-major buffers ----------------------
int64_t dn_minibatch_scratch_bytes(int64_t batch)
{
    const long long d = dn_minibatch_scratch_doubles(batch);
    if (d == 0) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^31 - 1 (got %lld)", (long long)batch);
    return d * 8;
}

/* the keyed permutation of csrc/dn_permute.h on the host: no device, no HIP call */
int32_t dn_minibatch_permutation(uint64_t seed, uint64_t epoch, int64_t m, int64_t start, int64_t count, int64_t *out)
{
    if (m < 1 || m > DN_PERMUTE_MAX) return fail(DN_ERR_INVALID_ARGUMENT, "m must be in 1..2^31 - 1 (got %lld)", (long long)m);
    if (start < 0 || count < 0 || start > m || count > m - start)
        return fail(DN_ERR_INVALID_ARGUMENT, "start and count must be >= 0 with start + count <= m (got %lld, %lld, m %lld)", (long long)start,
                    (long long)count, (long long)m);
    if (!out) return fail(DN_ERR_INVALID_ARGUMENT, "out is required");
    const DnPermutation p = dn_permute_make(seed, epoch, (uint32_t)m);
    for (int64_t i = 0; i < count; ++i) out[i] = (int64_t)dn_permute_at(p, (uint32_t)(start + i));
    return DN_OK;
}

int32_t dn_minibatch(const dn_minibatch_config *cfg, const dn_minibatch_field *fields, int64_t n_steps, int64_t n_envs, int64_t start,
                     int64_t batch, const int64_t *indices, const int64_t *epoch_offset, int64_t *indices_out, void *scratch,
                     int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (!cfg || !fields) return fail(DN_ERR_INVALID_ARGUMENT, "cfg and fields are required");
    if (cfg->num_fields < 1 || cfg->num_fields > DN_MINIBATCH_MAX_FIELDS)
        return fail(DN_ERR_INVALID_ARGUMENT, "num_fields must be in 1..%d (got %d)", DN_MINIBATCH_MAX_FIELDS, cfg->num_fields);
    if (const int32_t rc = reserved_ok(cfg->reserved)) return rc;
    if (const int32_t rc = epsilon_ok(cfg->epsilon)) return rc;
    if (n_steps < 1 || n_envs < 1) return fail(DN_ERR_INVALID_ARGUMENT, "n_steps and n_envs must be >= 1 (got %lld, %lld)", (long long)n_steps, (long long)n_envs);
    if (n_steps > DN_PERMUTE_MAX || n_envs > DN_PERMUTE_MAX / n_steps)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_steps x n_envs = %lld x %lld samples are more than the 2^31 - 1 of a buffer", (long long)n_steps,
                    (long long)n_envs);
    const int64_t m = n_steps * n_envs;
    // batch <= m <= 2^31 - 1: the grids, blocks(batch) x num_fields and ceil(batch / 256) workgroups, are far below the 2^31 - 1 of a launch
    if (batch < 1 || start < 0 || start > m || batch > m - start)
        return fail(DN_ERR_INVALID_ARGUMENT, "start must be >= 0 and batch >= 1 with start + batch <= n_steps x n_envs = %lld (got %lld, %lld)",
                    (long long)m, (long long)start, (long long)batch);
    if (indices && start != 0) return fail(DN_ERR_INVALID_ARGUMENT, "start must be 0 with indices (got %lld)", (long long)start);
    DnMinibatchArgs a;
    a.num_fields = cfg->num_fields;
    a.norm_field = -1;
    for (int f = 0; f < cfg->num_fields; ++f) {
        const dn_minibatch_field &fd = fields[f];
        if (!fd.src || !fd.dst) return fail(DN_ERR_INVALID_ARGUMENT, "field %d: src and dst are required", f);
        if (fd.width < 1 || fd.width > DN_ROWNORM_MAX_WIDTH)
            return fail(DN_ERR_INVALID_ARGUMENT, "field %d: width must be in 1..%d (got %d)", f, DN_ROWNORM_MAX_WIDTH, fd.width);
        if (fd.normalize != 0 && fd.normalize != 1) return fail(DN_ERR_INVALID_ARGUMENT, "field %d: normalize must be 0 or 1 (got %d)", f, fd.normalize);
        if (fd.normalize) {
            if (a.norm_field >= 0) return fail(DN_ERR_INVALID_ARGUMENT, "fields %d and %d: at most one field is normalised", a.norm_field, f);
            if (fd.width != 1) return fail(DN_ERR_INVALID_ARGUMENT, "field %d: the normalised field must be of width 1 (got %d)", f, fd.width);
            a.norm_field = f;
        }
        if (fd.dst == fd.src) return fail(DN_ERR_INVALID_ARGUMENT, "field %d: dst must not be src", f);
        if (((uintptr_t)fd.src | (uintptr_t)fd.dst) & 3u) return fail(DN_ERR_INVALID_ARGUMENT, "field %d: src and dst must be 4-byte aligned", f);
        a.fields[f] = fd;
    }
    for (int f = cfg->num_fields; f < DN_MINIBATCH_MAX_FIELDS; ++f) a.fields[f] = dn_minibatch_field{nullptr, nullptr, 0, 0};
    if (!scratch) return fail(DN_ERR_INVALID_ARGUMENT, "scratch is required");
    const int64_t need = dn_minibatch_scratch_bytes(batch);
    if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_minibatch_scratch_bytes");
    if (((uintptr_t)scratch | (uintptr_t)indices | (uintptr_t)epoch_offset | (uintptr_t)indices_out) & 7u)
        return fail(DN_ERR_INVALID_ARGUMENT, "scratch, indices, epoch_offset and indices_out must be 8-byte aligned");
    if (batch == 1) a.norm_field = -1;                 // SB3 skips the normalisation of a minibatch of one
    a.seed = cfg->seed; a.epoch = cfg->epoch; a.eps = cfg->epsilon;
    a.n_steps = (unsigned)n_steps; a.n_envs = (unsigned)n_envs; a.m = (unsigned)m; a.start = (unsigned)start; a.batch = (unsigned)batch;
    a.nblk = (unsigned)dn_rownorm_blocks(batch);
    a.indices = (const long long *)indices; a.epoch_offset = (const long long *)epoch_offset; a.indices_out = (long long *)indices_out;
    a.part = (double *)scratch;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_minibatch(a, (hipStream_t)stream));
    return DN_OK;
}

// ---- dn_ppo_loss: SB3 PPO.train's loss, statistics and the gradients with respect to the head outputs [from recall] ---------------------
int64_t dn_ppo_loss_scratch_bytes(int64_t batch, int32_t act_dim)
{
    if (act_dim < 1 || act_dim > DN_PPO_MAX_ACT) return fail(DN_ERR_INVALID_ARGUMENT, "act_dim must be in 1..%d (got %d)", DN_PPO_MAX_ACT, act_dim);
    const long long d = dn_ppo_loss_scratch_doubles(batch, act_dim);
    if (d == 0) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^31 - 1 (got %lld)", (long long)batch);
    return d * 8;
}

int32_t dn_ppo_loss(const dn_ppo_loss_config *cfg, int64_t batch, const float *mean, const float *log_std, const float *value,
                    const float *actions, const float *old_log_prob, const float *advantages, const float *returns,
                    const float *old_values, float *d_mean, float *d_log_std, float *d_value, float *log_prob_out, float *loss,
                    double *stats, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (cfg->act_dim < 1 || cfg->act_dim > DN_PPO_MAX_ACT)
        return fail(DN_ERR_INVALID_ARGUMENT, "act_dim must be in 1..%d (got %d)", DN_PPO_MAX_ACT, cfg->act_dim);
    if (const int32_t rc = reserved_ok(cfg->reserved)) return rc;
    if (batch < 1 || batch > 0x7fffffffll) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^31 - 1 (got %lld)", (long long)batch);
    if (!std::isfinite(cfg->clip_range) || !(cfg->clip_range > 0.0))
        return fail(DN_ERR_INVALID_ARGUMENT, "clip_range must be finite and > 0 (got %g)", cfg->clip_range);
    if (!std::isfinite(cfg->clip_range_vf))
        return fail(DN_ERR_INVALID_ARGUMENT, "clip_range_vf must be finite: > 0 clips the value step, <= 0 does not (got %g)", cfg->clip_range_vf);
    if (!std::isfinite(cfg->ent_coef) || !(cfg->ent_coef >= 0.0))
        return fail(DN_ERR_INVALID_ARGUMENT, "ent_coef must be finite and >= 0 (got %g)", cfg->ent_coef);
    if (!std::isfinite(cfg->vf_coef) || !(cfg->vf_coef >= 0.0))
        return fail(DN_ERR_INVALID_ARGUMENT, "vf_coef must be finite and >= 0 (got %g)", cfg->vf_coef);
    const bool vclip = cfg->clip_range_vf > 0.0;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float), cells = rows * (uintptr_t)cfg->act_dim, cols = (uintptr_t)cfg->act_dim * sizeof(float);
    const DnArg in[] = {{"mean", mean, cells, false}, {"log_std", log_std, cols, false}, {"value", value, rows, false}, {"actions", actions, cells, false},
                       {"old_log_prob", old_log_prob, rows, false}, {"advantages", advantages, rows, false}, {"returns", returns, rows, false},
                       {"old_values", old_values, rows, true}};
    DnArg out[] = {{"d_mean", d_mean, cells, false}, {"d_log_std", d_log_std, cols, false}, {"d_value", d_value, rows, false},
                        {"loss", loss, sizeof(float), false},
                        {"stats", stats, 8 * sizeof(double), false}, {"scratch", scratch, 0, false}, {"log_prob_out", log_prob_out, rows, true}};
    if (const DnArg *a = dn_first_missing(in)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (vclip && !old_values) return fail(DN_ERR_INVALID_ARGUMENT, "old_values is required with clip_range_vf > 0 (got %g)", cfg->clip_range_vf);
    if (!vclip && old_values) return fail(DN_ERR_INVALID_ARGUMENT, "old_values must be NULL without a value clip (clip_range_vf %g <= 0)", cfg->clip_range_vf);
    if (const DnArg *a = dn_first_missing(out)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    const int64_t need = dn_ppo_loss_scratch_bytes(batch, cfg->act_dim);
    if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_ppo_loss_scratch_bytes");
    if (((uintptr_t)stats | (uintptr_t)scratch) & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "stats and scratch must be 8-byte aligned");
    if (const DnArg *a = dn_first_misaligned(in, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(out, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    for (DnArg &a : out)
        if (a.p == scratch) a.bytes = (uintptr_t)need;      // scratch, and as ever any output given the same address
    const DnArg *o, *i;
    if (dn_first_overlap(out, in, &o, &i)) return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no output may alias an input", o->name, i->name);
    DnPpoLossArgs a;
    a.mean = mean; a.log_std = log_std; a.value = value; a.actions = actions; a.old_log_prob = old_log_prob; a.advantages = advantages;
    a.returns = returns; a.old_values = old_values;
    a.d_mean = d_mean; a.d_log_std = d_log_std; a.d_value = d_value; a.log_prob_out = log_prob_out; a.loss = loss;
    a.stats = stats; a.part = (double *)scratch;
    a.clip_range = cfg->clip_range; a.clip_range_vf = cfg->clip_range_vf; a.ent_coef = cfg->ent_coef; a.vf_coef = cfg->vf_coef;
    a.batch = batch; a.nblk = dn_rownorm_blocks(batch);
    a.act_dim = cfg->act_dim;
    a.vec = dn_rows_vec16(cfg->act_dim, mean, actions, d_mean);
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_ppo_loss(a, (hipStream_t)stream));
    return DN_OK;
}

// ---- dn_adam_step: SB3 PPO.train's clip_grad_norm_ + Adam.step [from recall] ---------------------------------------------------------------
int64_t dn_adam_scratch_bytes(const int64_t *counts, int32_t n_tensors)
{
    if (!counts) return fail(DN_ERR_INVALID_ARGUMENT, "counts is required");
    if (n_tensors < 1 || n_tensors > DN_ADAM_MAX_TENSORS)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_tensors must be in 1..%d (got %d)", DN_ADAM_MAX_TENSORS, n_tensors);
    long long chunks = 0;                              // at most 32 x 2^53: no overflow
    for (int i = 0; i < n_tensors; ++i) {
        if (counts[i] < 1) return fail(DN_ERR_INVALID_ARGUMENT, "counts[%d] must be >= 1 (got %lld)", i, (long long)counts[i]);
        chunks += dn_adam_chunks(counts[i]);
    }
    if (chunks > 0x7fffffffll)
        return fail(DN_ERR_INVALID_ARGUMENT, "the counts make %lld chunks of %d elements; a call takes at most 2^31 - 1", chunks, DN_ADAM_CHUNK);
    return chunks * 8;
}

int32_t dn_adam_step(const dn_adam_config *cfg, const dn_adam_tensor *tensors, const double *lr, double *state, double *stats,
                     void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (!tensors) return fail(DN_ERR_INVALID_ARGUMENT, "tensors is required");
    const DnArg doubles[] = {{"lr", lr, 0, false}, {"state", state, 0, false}, {"stats", stats, 0, false}, {"scratch", scratch, 0, false}};
    if (const DnArg *d = dn_first_missing(doubles)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", d->name);
    if (cfg->n_tensors < 1 || cfg->n_tensors > DN_ADAM_MAX_TENSORS)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_tensors must be in 1..%d (got %d)", DN_ADAM_MAX_TENSORS, cfg->n_tensors);
    if (cfg->flags & ~DN_ADAM_ZERO_GRADS) return fail(DN_ERR_INVALID_ARGUMENT, "flags has unknown bits: 0x%x (bit 0 zeroes the gradients)", cfg->flags);
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return fail(DN_ERR_INVALID_ARGUMENT, "beta1 must be in [0, 1) (got %g)", cfg->beta1);
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return fail(DN_ERR_INVALID_ARGUMENT, "beta2 must be in [0, 1) (got %g)", cfg->beta2);
    if (!std::isfinite(cfg->eps) || !(cfg->eps >= 0.0)) return fail(DN_ERR_INVALID_ARGUMENT, "eps must be finite and >= 0 (got %g)", cfg->eps);
    if (!std::isfinite(cfg->max_grad_norm))
        return fail(DN_ERR_INVALID_ARGUMENT, "max_grad_norm must be finite: > 0 clips the global norm, <= 0 does not (got %g)", cfg->max_grad_norm);
    int64_t counts[DN_ADAM_MAX_TENSORS];
    for (int i = 0; i < cfg->n_tensors; ++i) {
        const dn_adam_tensor &t = tensors[i];
        const DnArg fields[] = {{"param", t.param, 0, false}, {"grad", t.grad, 0, false}, {"exp_avg", t.exp_avg, 0, false},
                                {"exp_avg_sq", t.exp_avg_sq, 0, false}};
        // one refusal per field, in field order: a NULL field is heard of before a misaligned one only if it comes first
        const DnArg *missing = dn_first_missing(fields), *off = dn_first_misaligned(fields, 3u);
        if (missing && (!off || missing < off)) return fail(DN_ERR_INVALID_ARGUMENT, "tensors[%d].%s is required", i, missing->name);
        if (off) return fail(DN_ERR_INVALID_ARGUMENT, "tensors[%d].%s must be 4-byte aligned", i, off->name);
        if (t.count < 1) return fail(DN_ERR_INVALID_ARGUMENT, "tensors[%d].count must be >= 1 (got %lld)", i, (long long)t.count);
        counts[i] = t.count;
    }
    const int64_t need = dn_adam_scratch_bytes(counts, cfg->n_tensors);
    if (need < 0) return (int32_t)need;                // more than 2^31 - 1 chunks: the text is dn_adam_scratch_bytes'
    if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_adam_scratch_bytes");
    if (const DnArg *d = dn_first_misaligned(doubles, 7u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 8-byte aligned", d->name);
    DnAdamArgs a;
    std::memset(&a, 0, sizeof a);
    for (int i = 0; i < cfg->n_tensors; ++i) a.t[i] = tensors[i];
    a.lr = lr; a.state = state; a.stats = stats; a.part = (double *)scratch;
    a.beta1 = cfg->beta1; a.beta2 = cfg->beta2; a.eps = cfg->eps; a.max_grad_norm = cfg->max_grad_norm;
    a.nchunks = need / 8;
    a.n_tensors = cfg->n_tensors; a.flags = cfg->flags;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_adam(a, (hipStream_t)stream));
    return DN_OK;
}

// ---- dn_replay_sample: SB3 ReplayBuffer.sample [from recall] on either replay layout ------------------------------------------------------
/* what dn_replay_indices and dn_replay_sample both ask of the window the draw covers */
static int32_t replay_window_ok(int64_t valid, int64_t n_envs, int64_t skip)
{
    if (valid < 1 || valid > DN_REPLAY_MAX || n_envs < 1 || n_envs > DN_REPLAY_MAX)
        return fail(DN_ERR_INVALID_ARGUMENT, "valid and n_envs must be in 1..2^31 - 1 (got %lld, %lld)", (long long)valid, (long long)n_envs);
    if (skip < -1 || skip > valid)
        return fail(DN_ERR_INVALID_ARGUMENT, "skip must be -1 or in 0..valid = %lld (got %lld)", (long long)valid, (long long)skip);
    return DN_OK;
}

/* the keyed draw of csrc/dn_replay_draw.h on the host: no device, no HIP call */
int32_t dn_replay_indices(uint64_t seed, uint64_t draw, int64_t valid, int64_t n_envs, int64_t skip, int64_t start, int64_t count, int64_t *out)
{
    if (const int32_t rc = replay_window_ok(valid, n_envs, skip)) return rc;
    if (start < 0 || count < 0 || start > DN_REPLAY_MAX || count > DN_REPLAY_MAX - start)
        return fail(DN_ERR_INVALID_ARGUMENT, "start and count must be >= 0 with start + count <= 2^31 - 1 (got %lld, %lld)", (long long)start,
                    (long long)count);
    if (!out) return fail(DN_ERR_INVALID_ARGUMENT, "out is required");
    const uint64_t key = dn_replay_key(seed, draw);
    for (int64_t i = 0; i < count; ++i)
        out[i] = dn_replay_flat(dn_replay_draw_at(key, (uint64_t)(start + i), (uint32_t)valid, (uint32_t)n_envs, skip), (uint32_t)n_envs);
    return DN_OK;
}

/* cells x per bytes, held at 2^62 where the product is larger than any allocation: the overlap walk needs no more */
static uintptr_t replay_bytes(int64_t cells, int64_t per)
{
    return cells > (1ll << 62) / per ? (uintptr_t)1 << 62 : (uintptr_t)cells * (uintptr_t)per;
}

int32_t dn_replay_sample(const dn_replay_config *cfg, const dn_replay_source *src, int64_t batch, const int64_t *indices,
                         const int64_t *draw_offset, float *obs, float *next_obs, float *actions, float *rewards, float *dones,
                         int64_t *indices_out, int32_t device_id, void *stream)
{
    if (!cfg || !src) return fail(DN_ERR_INVALID_ARGUMENT, "cfg and src are required");
    if (const int32_t rc = reserved_ok(cfg->reserved)) return rc;
    if (cfg->layout != DN_REPLAY_PLAIN && cfg->layout != DN_REPLAY_RING)
        return fail(DN_ERR_INVALID_ARGUMENT, "layout must be 0 (DN_REPLAY_PLAIN) or 1 (DN_REPLAY_RING) (got %d)", cfg->layout);
    if (cfg->obs_dim < 1 || cfg->obs_dim > DN_REPLAY_MAX_OBS)
        return fail(DN_ERR_INVALID_ARGUMENT, "obs_dim must be in 1..%d (got %d)", DN_REPLAY_MAX_OBS, cfg->obs_dim);
    if (cfg->act_dim < 1 || cfg->act_dim > DN_REPLAY_MAX_ACT)
        return fail(DN_ERR_INVALID_ARGUMENT, "act_dim must be in 1..%d (got %d)", DN_REPLAY_MAX_ACT, cfg->act_dim);
    if (batch < 1 || batch > DN_REPLAY_MAX) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^31 - 1 (got %lld)", (long long)batch);
    const int64_t T = cfg->buffer_size, N = cfg->n_envs, S = cfg->valid;
    if (T < 1 || T > DN_REPLAY_MAX) return fail(DN_ERR_INVALID_ARGUMENT, "buffer_size must be in 1..2^31 - 1 (got %lld)", (long long)T);
    if (const int32_t rc = replay_window_ok(S, N, cfg->skip)) return rc;
    // T, N <= 2^31 - 1: T N < 2^62 transitions, which the kernel's 64-bit offsets hold
    if (S + (cfg->skip >= 0) > T)
        return fail(DN_ERR_INVALID_ARGUMENT, "valid%s must be <= buffer_size = %lld (got valid %lld, skip %lld)", cfg->skip >= 0 ? " + 1 (the skipped slot)" : "",
                    (long long)T, (long long)S, (long long)cfg->skip);
    const bool ring = cfg->layout == DN_REPLAY_RING;
    if (!ring && cfg->skip != -1)
        return fail(DN_ERR_INVALID_ARGUMENT, "skip must be -1 with DN_REPLAY_PLAIN: every slot below valid is whole (got %lld)", (long long)cfg->skip);
    if (indices && draw_offset) return fail(DN_ERR_INVALID_ARGUMENT, "draw_offset must be NULL with indices: the draw plays no part");
    const int64_t cells = T * N, D = cfg->obs_dim, A = cfg->act_dim, flag = ring ? 1 : 4;
    const DnArg in[] = {{"src.obs", src->obs, replay_bytes(cells + (ring ? N : 0), 4 * D), false}, {"src.next_obs", src->next_obs, replay_bytes(cells, 4 * D), false},
                        {"src.actions", src->actions, replay_bytes(cells, 4 * A), false}, {"src.rewards", src->rewards, replay_bytes(cells, 4), false},
                        {"src.dones", src->dones, replay_bytes(cells, flag), false}, {"src.timeouts", src->timeouts, replay_bytes(cells, flag), false}};
    const DnArg floats[] = {in[0], in[1], in[2], in[3], {"src.dones", ring ? nullptr : src->dones, 0, true}, {"src.timeouts", ring ? nullptr : src->timeouts, 0, true}};
    const DnArg out[] = {{"obs", obs, (uintptr_t)batch * 4u * (uintptr_t)D, false}, {"next_obs", next_obs, (uintptr_t)batch * 4u * (uintptr_t)D, false},
                         {"actions", actions, (uintptr_t)batch * 4u * (uintptr_t)A, false}, {"rewards", rewards, (uintptr_t)batch * 4u, false},
                         {"dones", dones, (uintptr_t)batch * 4u, false}};
    const DnArg longs[] = {{"indices", indices, 0, true}, {"draw_offset", draw_offset, 0, true}, {"indices_out", indices_out, (uintptr_t)batch * 8u, true}};
    if (const DnArg *a = dn_first_missing(in)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_missing(out)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_misaligned(floats, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(out, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(longs, 7u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 8-byte aligned", a->name);
    const DnArg *o, *i;
    if (dn_first_overlap(out, in, &o, &i) || dn_first_overlap(&longs[2], 1, in, 6, &o, &i))
        return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no output may be a source", o->name, i->name);
    DnReplayArgs a;
    a.src = *src;
    a.obs = obs; a.next_obs = next_obs; a.actions = actions; a.rewards = rewards; a.dones = dones;
    a.indices = (const long long *)indices; a.draw_offset = (const long long *)draw_offset; a.indices_out = (long long *)indices_out;
    a.seed = cfg->seed; a.draw = cfg->draw; a.skip = cfg->skip;
    a.t = (unsigned)T; a.n = (unsigned)N; a.s = (unsigned)S; a.batch = (unsigned)batch;
    a.obs_dim = cfg->obs_dim; a.act_dim = cfg->act_dim; a.ring = ring;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_replay(a, (hipStream_t)stream));
    return DN_OK;
}

// ---- the SAC loss heads: SB3 SAC.train's squashed policy, critic, actor and entropy-coefficient losses [from recall] ------------------------
/* what all four entry points ask of cfg and batch */
static int32_t sac_call_ok(const dn_sac_config *cfg, int64_t batch)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (cfg->reserved != 0) return fail(DN_ERR_INVALID_ARGUMENT, "reserved must be 0 (got %lld)", (long long)cfg->reserved);
    if (batch < 1 || batch > 0x7fffffffll) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^31 - 1 (got %lld)", (long long)batch);
    return DN_OK;
}
static int32_t sac_critics_ok(int32_t n_critics)
{
    return n_critics < 1 || n_critics > DN_SAC_MAX_CRITICS
               ? fail(DN_ERR_INVALID_ARGUMENT, "n_critics must be in 1..%d (got %d)", DN_SAC_MAX_CRITICS, n_critics) : DN_OK;
}
/* the policy head's fields */
static int32_t sac_policy_ok(const dn_sac_config *cfg, int64_t batch)
{
    if (const int32_t rc = sac_call_ok(cfg, batch)) return rc;
    if (cfg->act_dim < 1 || cfg->act_dim > DN_SAC_MAX_ACT)
        return fail(DN_ERR_INVALID_ARGUMENT, "act_dim must be in 1..%d (got %d)", DN_SAC_MAX_ACT, cfg->act_dim);
    if (!std::isfinite(cfg->log_std_min) || !std::isfinite(cfg->log_std_max) || !(cfg->log_std_min < cfg->log_std_max))
        return fail(DN_ERR_INVALID_ARGUMENT, "log_std_min and log_std_max must be finite with log_std_min < log_std_max (got %g, %g)", cfg->log_std_min,
                    cfg->log_std_max);
    return DN_OK;
}
/* the coefficient both losses read: the device's log_ent_coef, or the host's ent_coef */
static int32_t sac_ent_coef_ok(const dn_sac_config *cfg, const float *log_ent_coef)
{
    if (!log_ent_coef && (!std::isfinite(cfg->ent_coef) || !(cfg->ent_coef >= 0.0)))
        return fail(DN_ERR_INVALID_ARGUMENT, "ent_coef must be finite and >= 0 when log_ent_coef is NULL (got %g)", cfg->ent_coef);
    return DN_OK;
}
/* required, aligned, and no output on an input or on another output; scratch takes its size first */
static int32_t sac_pointers_ok(const DnArg *in, size_t n_in, DnArg *out, size_t n_out, const void *stats, const void *scratch, int64_t need)
{
    if (const DnArg *a = dn_first_missing(in, n_in)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_missing(out, n_out)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (((uintptr_t)stats | (uintptr_t)scratch) & 7u) return fail(DN_ERR_INVALID_ARGUMENT, "stats and scratch must be 8-byte aligned");
    if (const DnArg *a = dn_first_misaligned(in, n_in, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(out, n_out, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    for (size_t k = 0; k < n_out; ++k)
        if (scratch && out[k].p == scratch) out[k].bytes = (uintptr_t)need;
    const DnArg *o, *i;
    if (dn_first_overlap(out, n_out, in, n_in, &o, &i)) return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no output may alias an input", o->name, i->name);
    for (size_t k = 0; k + 1 < n_out; ++k)
        if (dn_first_overlap(&out[k], 1, &out[k + 1], n_out - k - 1, &o, &i))
            return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no two outputs may share memory", o->name, i->name);
    return DN_OK;
}
static const char *const SAC_Q[] = {"q[0]", "q[1]", "q[2]", "q[3]"}, *const SAC_NEXT_Q[] = {"next_q[0]", "next_q[1]", "next_q[2]", "next_q[3]"},
                  *const SAC_D_Q[] = {"d_q[0]", "d_q[1]", "d_q[2]", "d_q[3]"}, *const SAC_Q_PI[] = {"q_pi[0]", "q_pi[1]", "q_pi[2]", "q_pi[3]"},
                  *const SAC_D_Q_PI[] = {"d_q_pi[0]", "d_q_pi[1]", "d_q_pi[2]", "d_q_pi[3]"};

int64_t dn_sac_loss_scratch_bytes(int64_t batch, int32_t n_critics)
{
    if (const int32_t rc = sac_critics_ok(n_critics)) return rc;
    const long long d = dn_sac_loss_scratch_doubles(batch, n_critics);
    if (d == 0) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^31 - 1 (got %lld)", (long long)batch);
    return d * 8;
}

int32_t dn_sac_policy(const dn_sac_config *cfg, int64_t batch, const float *mean, const float *log_std, const float *noise, float *actions,
                      float *log_prob, int32_t device_id, void *stream)
{
    if (const int32_t rc = sac_policy_ok(cfg, batch)) return rc;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float), cells = rows * (uintptr_t)cfg->act_dim;
    const DnArg in[] = {{"mean", mean, cells, false}, {"log_std", log_std, cells, false}, {"noise", noise, cells, false}};
    DnArg out[] = {{"actions", actions, cells, false}, {"log_prob", log_prob, rows, false}};
    if (const int32_t rc = sac_pointers_ok(in, 3, out, 2, nullptr, nullptr, 0)) return rc;
    DnSacPolicyArgs a;
    std::memset(&a, 0, sizeof a);
    a.mean = mean; a.raw = log_std; a.eps = noise; a.actions = actions; a.log_prob = log_prob;
    a.lo = cfg->log_std_min; a.hi = cfg->log_std_max; a.batch = batch; a.act_dim = cfg->act_dim;
    a.vec = dn_rows_vec16(cfg->act_dim, mean, log_std, noise, actions);
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_sac_policy(a, false, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_sac_policy_backward(const dn_sac_config *cfg, int64_t batch, const float *mean, const float *log_std, const float *noise,
                               const float *g_actions, const float *g_log_prob, float *d_mean, float *d_log_std, int32_t device_id,
                               void *stream)
{
    if (const int32_t rc = sac_policy_ok(cfg, batch)) return rc;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float), cells = rows * (uintptr_t)cfg->act_dim;
    const DnArg in[] = {{"mean", mean, cells, false}, {"log_std", log_std, cells, false}, {"noise", noise, cells, false},
                        {"g_actions", g_actions, cells, true}, {"g_log_prob", g_log_prob, rows, true}};
    DnArg out[] = {{"d_mean", d_mean, cells, false}, {"d_log_std", d_log_std, cells, false}};
    if (const int32_t rc = sac_pointers_ok(in, 5, out, 2, nullptr, nullptr, 0)) return rc;
    DnSacPolicyArgs a;
    std::memset(&a, 0, sizeof a);
    a.mean = mean; a.raw = log_std; a.eps = noise; a.g_a = g_actions; a.g_lp = g_log_prob; a.d_mean = d_mean; a.d_raw = d_log_std;
    a.lo = cfg->log_std_min; a.hi = cfg->log_std_max; a.batch = batch; a.act_dim = cfg->act_dim;
    a.vec = dn_rows_vec16(cfg->act_dim, mean, log_std, noise, g_actions, d_mean, d_log_std);
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_sac_policy(a, true, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_sac_critic_loss(const dn_sac_config *cfg, int64_t batch, const float *const *q, const float *const *next_q,
                           const float *next_log_prob, const float *rewards, const float *dones, const float *log_ent_coef,
                           float *const *d_q, float *target_q, float *loss, double *stats, void *scratch, int64_t scratch_bytes,
                           int32_t device_id, void *stream)
{
    if (const int32_t rc = sac_call_ok(cfg, batch)) return rc;
    if (const int32_t rc = sac_critics_ok(cfg->n_critics)) return rc;
    if (!std::isfinite(cfg->gamma) || !(cfg->gamma >= 0.0 && cfg->gamma <= 1.0))
        return fail(DN_ERR_INVALID_ARGUMENT, "gamma must be finite and in [0, 1] (got %g)", cfg->gamma);
    if (const int32_t rc = sac_ent_coef_ok(cfg, log_ent_coef)) return rc;
    if (!q) return fail(DN_ERR_INVALID_ARGUMENT, "q is required");
    if (!next_q) return fail(DN_ERR_INVALID_ARGUMENT, "next_q is required");
    if (!d_q) return fail(DN_ERR_INVALID_ARGUMENT, "d_q is required");
    const int C = cfg->n_critics;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float);
    DnArg in[2 * DN_SAC_MAX_CRITICS + 4], out[DN_SAC_MAX_CRITICS + 4];
    size_t ni = 0, no = 0;
    for (int c = 0; c < C; ++c) in[ni++] = DnArg{SAC_Q[c], q[c], rows, false};
    for (int c = 0; c < C; ++c) in[ni++] = DnArg{SAC_NEXT_Q[c], next_q[c], rows, false};
    in[ni++] = DnArg{"next_log_prob", next_log_prob, rows, false};
    in[ni++] = DnArg{"rewards", rewards, rows, false};
    in[ni++] = DnArg{"dones", dones, rows, false};
    in[ni++] = DnArg{"log_ent_coef", log_ent_coef, sizeof(float), true};
    for (int c = 0; c < C; ++c) out[no++] = DnArg{SAC_D_Q[c], d_q[c], rows, false};
    out[no++] = DnArg{"target_q", target_q, rows, false};
    out[no++] = DnArg{"loss", loss, sizeof(float), false};
    out[no++] = DnArg{"stats", stats, 8 * sizeof(double), false};
    out[no++] = DnArg{"scratch", scratch, 0, false};
    const int64_t need = dn_sac_loss_scratch_bytes(batch, C);
    if (scratch && dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_sac_loss_scratch_bytes");
    if (const int32_t rc = sac_pointers_ok(in, ni, out, no, stats, scratch, need)) return rc;
    DnSacLossArgs a;
    std::memset(&a, 0, sizeof a);
    for (int c = 0; c < C; ++c) { a.q[c] = q[c]; a.next_q[c] = next_q[c]; a.d_q[c] = d_q[c]; }
    a.next_log_prob = next_log_prob; a.rewards = rewards; a.dones = dones; a.log_ent_coef = log_ent_coef;
    a.target_q = target_q; a.loss = loss; a.stats = stats; a.part = (double *)scratch;
    a.gamma = cfg->gamma; a.ent_coef = cfg->ent_coef;
    a.batch = batch; a.nblk = dn_rownorm_blocks(batch); a.n_critics = C; a.mode = DN_SAC_CRITIC;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_sac_loss(a, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_sac_actor_loss(const dn_sac_config *cfg, int64_t batch, const float *log_prob, const float *const *q_pi,
                          const float *log_ent_coef, float *d_log_prob, float *const *d_q_pi, float *d_log_ent_coef, float *actor_loss,
                          float *ent_coef_loss, double *stats, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = sac_call_ok(cfg, batch)) return rc;
    if (const int32_t rc = sac_critics_ok(cfg->n_critics)) return rc;
    if (!std::isfinite(cfg->target_entropy)) return fail(DN_ERR_INVALID_ARGUMENT, "target_entropy must be finite (got %g)", cfg->target_entropy);
    if (const int32_t rc = sac_ent_coef_ok(cfg, log_ent_coef)) return rc;
    if (!q_pi) return fail(DN_ERR_INVALID_ARGUMENT, "q_pi is required");
    if (!d_q_pi) return fail(DN_ERR_INVALID_ARGUMENT, "d_q_pi is required");
    if (log_ent_coef && !d_log_ent_coef) return fail(DN_ERR_INVALID_ARGUMENT, "d_log_ent_coef is required with log_ent_coef");
    if (!log_ent_coef && d_log_ent_coef)
        return fail(DN_ERR_INVALID_ARGUMENT, "d_log_ent_coef must be NULL without log_ent_coef: a fixed coefficient has no gradient");
    const int C = cfg->n_critics;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float);
    DnArg in[DN_SAC_MAX_CRITICS + 2], out[DN_SAC_MAX_CRITICS + 6];
    size_t ni = 0, no = 0;
    in[ni++] = DnArg{"log_prob", log_prob, rows, false};
    for (int c = 0; c < C; ++c) in[ni++] = DnArg{SAC_Q_PI[c], q_pi[c], rows, false};
    in[ni++] = DnArg{"log_ent_coef", log_ent_coef, sizeof(float), true};
    out[no++] = DnArg{"d_log_prob", d_log_prob, rows, false};
    for (int c = 0; c < C; ++c) out[no++] = DnArg{SAC_D_Q_PI[c], d_q_pi[c], rows, false};
    out[no++] = DnArg{"d_log_ent_coef", d_log_ent_coef, sizeof(float), true};
    out[no++] = DnArg{"actor_loss", actor_loss, sizeof(float), false};
    out[no++] = DnArg{"ent_coef_loss", ent_coef_loss, sizeof(float), false};
    out[no++] = DnArg{"stats", stats, 8 * sizeof(double), false};
    out[no++] = DnArg{"scratch", scratch, 0, false};
    const int64_t need = dn_sac_loss_scratch_bytes(batch, C);
    if (scratch && dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_sac_loss_scratch_bytes");
    if (const int32_t rc = sac_pointers_ok(in, ni, out, no, stats, scratch, need)) return rc;
    DnSacLossArgs a;
    std::memset(&a, 0, sizeof a);
    for (int c = 0; c < C; ++c) { a.q[c] = q_pi[c]; a.d_q[c] = d_q_pi[c]; }
    a.log_prob = log_prob; a.log_ent_coef = log_ent_coef;
    a.d_log_prob = d_log_prob; a.d_log_ent_coef = d_log_ent_coef; a.loss = actor_loss; a.ent_coef_loss = ent_coef_loss;
    a.stats = stats; a.part = (double *)scratch;
    a.target_entropy = cfg->target_entropy; a.ent_coef = cfg->ent_coef;
    a.batch = batch; a.nblk = dn_rownorm_blocks(batch); a.n_critics = C; a.mode = DN_SAC_ACTOR;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_sac_loss(a, (hipStream_t)stream));
    return DN_OK;
}
}  // extern "C"

// ---- dn_mlp_train: the training pass of the reference's Tanh networks (forward with saved activations, backward) ---------------------------
/* what the three entry points ask of cfg, of the dimensions of layers and of batch */
static int32_t mlp_train_shape_ok(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (!layers) return fail(DN_ERR_INVALID_ARGUMENT, "layers is required");
    if (cfg->n_layers < 2 || cfg->n_layers > DN_MLP_TRAIN_MAX_LAYERS)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_layers must be in 2..%d, the head included (got %d)", DN_MLP_TRAIN_MAX_LAYERS, cfg->n_layers);
    if (cfg->activation != DN_MLP_ACT_TANH)
        return fail(DN_ERR_INVALID_ARGUMENT, "activation must be DN_MLP_ACT_TANH = %d (got %d)", DN_MLP_ACT_TANH, cfg->activation);
    if (cfg->flags & ~(DN_MLP_TRAIN_ACCUMULATE | DN_MLP_TRAIN_NO_PARAM_GRADS))
        return fail(DN_ERR_INVALID_ARGUMENT, "flags has unknown bits: 0x%x (bit 0 accumulates, bit 1 skips the parameter gradients)", cfg->flags);
    if (const int32_t rc = reserved_ok(cfg->reserved)) return rc;
    const int L = cfg->n_layers;
    if (layers[0].in_dim < 1 || layers[0].in_dim > 64)
        return fail(DN_ERR_INVALID_ARGUMENT, "layers[0].in_dim must be in 1..64 (got %d)", layers[0].in_dim);
    for (int l = 0; l < L - 1; ++l)
        if (layers[l].out_dim < 32 || layers[l].out_dim > 512 || layers[l].out_dim % 32)
            return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d].out_dim, a hidden width, must be a multiple of 32 in 32..512 (got %d)", l, layers[l].out_dim);
    if (layers[L - 1].out_dim < 1 || layers[L - 1].out_dim > 32)
        return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d].out_dim, the head's, must be in 1..32 (got %d)", L - 1, layers[L - 1].out_dim);
    for (int l = 1; l < L; ++l)
        if (layers[l].in_dim != layers[l - 1].out_dim)
            return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d].in_dim must be layers[%d].out_dim = %d (got %d)", l, l - 1, layers[l - 1].out_dim,
                        layers[l].in_dim);
    if (batch < 1 || batch > (1ll << 24)) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^24 (got %lld)", (long long)batch);
    return DN_OK;
}

/* the pointers of a call: `in` and `out` are the call's own besides the layers'; grads: d_weight and d_bias are written */
static int32_t mlp_train_pointers_ok(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch, const DnArg *in_own,
                                     size_t n_in_own, const DnArg *out_own, size_t n_out_own, bool grads, void *scratch, int64_t scratch_bytes)
{
    static const char *const W[] = {"layers[0].weight", "layers[1].weight", "layers[2].weight", "layers[3].weight"};
    static const char *const B[] = {"layers[0].bias", "layers[1].bias", "layers[2].bias", "layers[3].bias"};
    static const char *const DW[] = {"layers[0].d_weight", "layers[1].d_weight", "layers[2].d_weight", "layers[3].d_weight"};
    static const char *const DB[] = {"layers[0].d_bias", "layers[1].d_bias", "layers[2].d_bias", "layers[3].d_bias"};
    DnArg in[2 * DN_MLP_TRAIN_MAX_LAYERS + 2], out[2 * DN_MLP_TRAIN_MAX_LAYERS + 3];
    size_t ni = 0, no = 0;
    for (size_t i = 0; i < n_in_own; ++i) in[ni++] = in_own[i];
    for (size_t i = 0; i < n_out_own; ++i) out[no++] = out_own[i];
    for (int l = 0; l < cfg->n_layers; ++l) {
        const uintptr_t wb = (uintptr_t)layers[l].out_dim * (uintptr_t)layers[l].in_dim * sizeof(float), bb = (uintptr_t)layers[l].out_dim * sizeof(float);
        in[ni++] = DnArg{W[l], layers[l].weight, wb, false};
        in[ni++] = DnArg{B[l], layers[l].bias, bb, false};
        if (grads) {
            out[no++] = DnArg{DW[l], layers[l].d_weight, wb, false};
            out[no++] = DnArg{DB[l], layers[l].d_bias, bb, false};
        }
    }
    const int64_t need = dn_mlp_train_layout(layers, cfg->n_layers, batch).total;
    out[no++] = DnArg{"scratch", scratch, (uintptr_t)need, false};
    if (const DnArg *a = dn_first_missing(in, ni)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_missing(out, no)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_mlp_train_scratch_bytes");
    if ((uintptr_t)scratch & 15u) return fail(DN_ERR_INVALID_ARGUMENT, "scratch must be 16-byte aligned");
    if (const DnArg *a = dn_first_misaligned(in, ni, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(out, no, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    const DnArg *o, *i;
    if (dn_first_overlap(out, no, in, ni, &o, &i)) return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no output may alias an input", o->name, i->name);
    for (size_t a = 0; a + 1 < no; ++a)
        if (dn_first_overlap(&out[a], 1, &out[a + 1], no - a - 1, &o, &i))
            return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: every output is a tensor of its own", o->name, i->name);
    return DN_OK;
}

static void mlp_train_args(DnMlpTrainArgs &a, const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch, void *scratch)
{
    std::memset(&a, 0, sizeof a);
    for (int l = 0; l < cfg->n_layers; ++l) a.layer[l] = layers[l];
    a.scratch = (char *)scratch;
    a.batch = batch;
    a.n_layers = cfg->n_layers;
    a.flags = cfg->flags;
}

extern "C" {

int64_t dn_mlp_train_scratch_bytes(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch)
{
    if (const int32_t rc = mlp_train_shape_ok(cfg, layers, batch)) return rc;
    return dn_mlp_train_layout(layers, cfg->n_layers, batch).total;
}

int32_t dn_mlp_train_forward(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, const float *x, int64_t batch, float *out,
                             void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = mlp_train_shape_ok(cfg, layers, batch)) return rc;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float);
    const DnArg in[] = {{"x", x, rows * (uintptr_t)layers[0].in_dim, false}};
    const DnArg outs[] = {{"out", out, rows * (uintptr_t)layers[cfg->n_layers - 1].out_dim, false}};
    if (const int32_t rc = mlp_train_pointers_ok(cfg, layers, batch, in, 1, outs, 1, false, scratch, scratch_bytes)) return rc;
    DnMlpTrainArgs a;
    mlp_train_args(a, cfg, layers, batch, scratch);
    a.x = x; a.out = out;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_mlp_train_forward(a, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_mlp_train_backward(const dn_mlp_train_config *cfg, const dn_mlp_train_layer *layers, const float *x, const float *d_out,
                              int64_t batch, float *d_x, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = mlp_train_shape_ok(cfg, layers, batch)) return rc;
    const bool grads = !(cfg->flags & DN_MLP_TRAIN_NO_PARAM_GRADS);
    if (!grads && !d_x)
        return fail(DN_ERR_INVALID_ARGUMENT, "d_x is required with DN_MLP_TRAIN_NO_PARAM_GRADS in flags (there is nothing else to do)");
    const uintptr_t rows = (uintptr_t)batch * sizeof(float);
    const DnArg in[] = {{"x", x, rows * (uintptr_t)layers[0].in_dim, false},
                        {"d_out", d_out, rows * (uintptr_t)layers[cfg->n_layers - 1].out_dim, false}};
    const DnArg outs[] = {{"d_x", d_x, rows * (uintptr_t)layers[0].in_dim, true}};
    if (const int32_t rc = mlp_train_pointers_ok(cfg, layers, batch, in, 2, outs, 1, grads, scratch, scratch_bytes)) return rc;
    DnMlpTrainArgs a;
    mlp_train_args(a, cfg, layers, batch, scratch);
    a.x = x; a.d_out = d_out; a.d_x = d_x;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_mlp_train_backward(a, (hipStream_t)stream));
    return DN_OK;
}

}  // extern "C"

// ---- dn_sac_train: the training pass of the SAC networks, and dn_polyak_update --------------------------------------------------------------
/* a pointer argument whose name is made at run time: layers[c][l].field, out[i] */
struct SacNamed {
    char name[40];
};
__attribute__((format(printf, 4, 5))) static DnArg sac_named(SacNamed &n, const void *p, uintptr_t bytes, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(n.name, sizeof n.name, fmt, ap);
    va_end(ap);
    return DnArg{n.name, p, bytes, false};
}

/* what the three entry points ask of cfg, of the dimensions of layers and of batch */
static int32_t sac_train_shape_ok(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (!layers) return fail(DN_ERR_INVALID_ARGUMENT, "layers is required");
    if (cfg->n_nets < 1 || cfg->n_nets > DN_SAC_TRAIN_MAX_NETS)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_nets must be in 1..%d (got %d)", DN_SAC_TRAIN_MAX_NETS, cfg->n_nets);
    if (cfg->n_layers < 2 || cfg->n_layers > DN_MLP_TRAIN_MAX_LAYERS)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_layers must be in 2..%d, the head counted once (got %d)", DN_MLP_TRAIN_MAX_LAYERS, cfg->n_layers);
    if (cfg->head_parts < 1 || cfg->head_parts > DN_SAC_TRAIN_MAX_PARTS)
        return fail(DN_ERR_INVALID_ARGUMENT, "head_parts must be in 1..%d (got %d)", DN_SAC_TRAIN_MAX_PARTS, cfg->head_parts);
    if (cfg->activation != DN_MLP_ACT_TANH && cfg->activation != DN_MLP_ACT_RELU)
        return fail(DN_ERR_INVALID_ARGUMENT, "activation must be DN_MLP_ACT_TANH = %d or DN_MLP_ACT_RELU = %d (got %d)", DN_MLP_ACT_TANH,
                    DN_MLP_ACT_RELU, cfg->activation);
    if (cfg->in0 < 1 || cfg->in0 > 64) return fail(DN_ERR_INVALID_ARGUMENT, "in0 must be in 1..64 (got %d)", cfg->in0);
    if (cfg->in1 < 0 || cfg->in1 > 63 || cfg->in0 + cfg->in1 > 64)
        return fail(DN_ERR_INVALID_ARGUMENT, "in1 must be in 0..63 with in0 + in1 <= 64 (got %d beside in0 = %d)", cfg->in1, cfg->in0);
    if (cfg->flags & ~(DN_MLP_TRAIN_ACCUMULATE | DN_MLP_TRAIN_NO_PARAM_GRADS))
        return fail(DN_ERR_INVALID_ARGUMENT, "flags has unknown bits: 0x%x (bit 0 accumulates, bit 1 skips the parameter gradients)", cfg->flags);
    if (const int32_t rc = reserved_ok(cfg->reserved)) return rc;
    const int L = cfg->n_layers, P = cfg->head_parts, E = L - 1 + P;
    for (int c = 0; c < cfg->n_nets; ++c) {
        const dn_mlp_train_layer *net = layers + c * E;
        if (net[0].in_dim != cfg->in0 + cfg->in1)
            return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][0].in_dim must be in0 + in1 = %d (got %d)", c, cfg->in0 + cfg->in1, net[0].in_dim);
        for (int l = 0; l < L - 1; ++l)
            if (net[l].out_dim < 32 || net[l].out_dim > 512 || net[l].out_dim % 32)
                return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][%d].out_dim, a hidden width, must be a multiple of 32 in 32..512 (got %d)", c, l,
                            net[l].out_dim);
        for (int l = 1; l < E; ++l) {
            const int before = l < L ? l - 1 : L - 2;                            // every head part reads the last hidden layer
            if (net[l].in_dim != net[before].out_dim)
                return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][%d].in_dim must be layers[%d][%d].out_dim = %d (got %d)", c, l, c, before,
                            net[before].out_dim, net[l].in_dim);
        }
        int head = 0;
        for (int l = L - 1; l < E; ++l) {
            if (net[l].out_dim < 1 || net[l].out_dim > 32)
                return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][%d].out_dim, a head part's, must be in 1..32 (got %d)", c, l, net[l].out_dim);
            head += net[l].out_dim;
        }
        if (head > 32)
            return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][%d].out_dim: the head's parts must have at most 32 outputs together (got %d)", c, E - 1, head);
        for (int l = 0; l < E; ++l) {
            if (net[l].in_dim != layers[l].in_dim)
                return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][%d].in_dim must be layers[0][%d].in_dim = %d, the networks of a group have one shape (got %d)",
                            c, l, l, layers[l].in_dim, net[l].in_dim);
            if (net[l].out_dim != layers[l].out_dim)
                return fail(DN_ERR_INVALID_ARGUMENT, "layers[%d][%d].out_dim must be layers[0][%d].out_dim = %d, the networks of a group have one shape (got %d)",
                            c, l, l, layers[l].out_dim, net[l].out_dim);
        }
    }
    if (batch < 1 || batch > (1ll << 24)) return fail(DN_ERR_INVALID_ARGUMENT, "batch must be in 1..2^24 (got %lld)", (long long)batch);
    return DN_OK;
}

/* every pointer of a call.  table: out (forward) or d_out (backward), n_nets * head_parts pointers; grads: d_weight and d_bias are written */
static int32_t sac_train_pointers_ok(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch, const float *x0,
                                     const float *x1, const void *const *table, const char *table_name, bool table_is_output, float *d_x0,
                                     float *d_x1, bool backward, bool grads, void *scratch, int64_t scratch_bytes)
{
    constexpr int MOST = DN_SAC_TRAIN_MAX_NETS * DN_SAC_TRAIN_MAX_ENTRIES, HEADS = DN_SAC_TRAIN_MAX_NETS * DN_SAC_TRAIN_MAX_PARTS;
    const int L = cfg->n_layers, P = cfg->head_parts, E = L - 1 + P;
    const uintptr_t rows = (uintptr_t)batch * sizeof(float);
    if (!table) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", table_name);
    if ((x1 != nullptr) != (cfg->in1 > 0)) return fail(DN_ERR_INVALID_ARGUMENT, "x1 must be NULL exactly when in1 = 0 (in1 = %d)", cfg->in1);
    SacNamed names[4 * MOST + HEADS];
    DnArg in[2 * MOST + HEADS + 2], out[2 * MOST + HEADS + 3];
    size_t ni = 0, no = 0, nn = 0;
    in[ni++] = DnArg{"x0", x0, rows * (uintptr_t)cfg->in0, false};
    in[ni++] = DnArg{"x1", x1, rows * (uintptr_t)cfg->in1, true};
    if (backward) {
        out[no++] = DnArg{"d_x0", d_x0, rows * (uintptr_t)cfg->in0, true};
        out[no++] = DnArg{"d_x1", d_x1, rows * (uintptr_t)cfg->in1, true};
    }
    for (int c = 0; c < cfg->n_nets; ++c) {
        for (int p = 0; p < P; ++p) {
            const DnArg a = sac_named(names[nn++], table[c * P + p], rows * (uintptr_t)layers[c * E + L - 1 + p].out_dim, "%s[%d]", table_name, c * P + p);
            (table_is_output ? out[no++] : in[ni++]) = a;
        }
        for (int l = 0; l < E; ++l) {
            const dn_mlp_train_layer &T = layers[c * E + l];
            const uintptr_t wb = (uintptr_t)T.out_dim * (uintptr_t)T.in_dim * sizeof(float), bb = (uintptr_t)T.out_dim * sizeof(float);
            in[ni++] = sac_named(names[nn++], T.weight, wb, "layers[%d][%d].%s", c, l, "weight");
            in[ni++] = sac_named(names[nn++], T.bias, bb, "layers[%d][%d].%s", c, l, "bias");
            if (grads) {
                out[no++] = sac_named(names[nn++], T.d_weight, wb, "layers[%d][%d].%s", c, l, "d_weight");
                out[no++] = sac_named(names[nn++], T.d_bias, bb, "layers[%d][%d].%s", c, l, "d_bias");
            }
        }
    }
    const int64_t need = dn_sac_train_layout(layers, cfg->n_nets, L, P, batch).total;
    out[no++] = DnArg{"scratch", scratch, (uintptr_t)need, false};
    if (const DnArg *a = dn_first_missing(in, ni)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_missing(out, no)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (dn_scratch_short(scratch_bytes, need)) return scratch_too_small(scratch_bytes, need, "dn_sac_train_scratch_bytes");
    if ((uintptr_t)scratch & 15u) return fail(DN_ERR_INVALID_ARGUMENT, "scratch must be 16-byte aligned");
    if (const DnArg *a = dn_first_misaligned(in, ni, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(out, no, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    const DnArg *o, *i;
    if (dn_first_overlap(out, no, in, ni, &o, &i)) return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no output may alias an input", o->name, i->name);
    for (size_t a = 0; a + 1 < no; ++a)
        if (dn_first_overlap(&out[a], 1, &out[a + 1], no - a - 1, &o, &i))
            return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: every output is a tensor of its own", o->name, i->name);
    return DN_OK;
}

static void sac_train_args(DnSacTrainArgs &a, const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch, const float *x0,
                           const float *x1, void *scratch)
{
    std::memset(&a, 0, sizeof a);
    const int E = cfg->n_layers - 1 + cfg->head_parts;
    for (int c = 0; c < cfg->n_nets; ++c)
        for (int l = 0; l < E; ++l) a.layer[c][l] = layers[c * E + l];
    a.x0 = x0; a.x1 = x1;
    a.scratch = (char *)scratch;
    a.batch = batch;
    a.n_nets = cfg->n_nets; a.n_layers = cfg->n_layers; a.head_parts = cfg->head_parts; a.activation = cfg->activation;
    a.in0 = cfg->in0; a.in1 = cfg->in1; a.flags = cfg->flags;
}

extern "C" {

int64_t dn_sac_train_scratch_bytes(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, int64_t batch)
{
    if (const int32_t rc = sac_train_shape_ok(cfg, layers, batch)) return rc;
    return dn_sac_train_layout(layers, cfg->n_nets, cfg->n_layers, cfg->head_parts, batch).total;
}

int32_t dn_sac_train_forward(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, const float *x0, const float *x1,
                             int64_t batch, float *const *out, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = sac_train_shape_ok(cfg, layers, batch)) return rc;
    if (const int32_t rc = sac_train_pointers_ok(cfg, layers, batch, x0, x1, (const void *const *)out, "out", true, nullptr, nullptr, false, false,
                                                 scratch, scratch_bytes))
        return rc;
    DnSacTrainArgs a;
    sac_train_args(a, cfg, layers, batch, x0, x1, scratch);
    for (int c = 0; c < cfg->n_nets; ++c)
        for (int p = 0; p < cfg->head_parts; ++p) a.out[c][p] = out[c * cfg->head_parts + p];
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_sac_train_forward(a, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_sac_train_backward(const dn_sac_train_config *cfg, const dn_mlp_train_layer *layers, const float *x0, const float *x1,
                              const float *const *d_out, int64_t batch, float *d_x0, float *d_x1, void *scratch, int64_t scratch_bytes,
                              int32_t device_id, void *stream)
{
    if (const int32_t rc = sac_train_shape_ok(cfg, layers, batch)) return rc;
    const bool grads = !(cfg->flags & DN_MLP_TRAIN_NO_PARAM_GRADS);
    if (!grads && !d_x0 && !d_x1)
        return fail(DN_ERR_INVALID_ARGUMENT, "d_x0 or d_x1 is required with DN_MLP_TRAIN_NO_PARAM_GRADS in flags (there is nothing else to do)");
    if (d_x1 && cfg->in1 == 0) return fail(DN_ERR_INVALID_ARGUMENT, "d_x1 must be NULL when in1 = 0");
    if (const int32_t rc = sac_train_pointers_ok(cfg, layers, batch, x0, x1, (const void *const *)d_out, "d_out", false, d_x0, d_x1, true, grads,
                                                 scratch, scratch_bytes))
        return rc;
    DnSacTrainArgs a;
    sac_train_args(a, cfg, layers, batch, x0, x1, scratch);
    for (int c = 0; c < cfg->n_nets; ++c)
        for (int p = 0; p < cfg->head_parts; ++p) a.d_out[c][p] = d_out[c * cfg->head_parts + p];
    a.d_x0 = d_x0; a.d_x1 = d_x1;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_sac_train_backward(a, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_polyak_update(int32_t n_tensors, const float *const *source, float *const *target, const int64_t *counts, double tau,
                         int32_t device_id, void *stream)
{
    if (n_tensors < 1 || n_tensors > DN_ADAM_MAX_TENSORS)
        return fail(DN_ERR_INVALID_ARGUMENT, "n_tensors must be in 1..%d (got %d)", DN_ADAM_MAX_TENSORS, n_tensors);
    if (!source) return fail(DN_ERR_INVALID_ARGUMENT, "source is required");
    if (!target) return fail(DN_ERR_INVALID_ARGUMENT, "target is required");
    if (!counts) return fail(DN_ERR_INVALID_ARGUMENT, "counts is required");
    if (!(tau >= 0.0 && tau <= 1.0)) return fail(DN_ERR_INVALID_ARGUMENT, "tau must be in [0, 1] (got %g)", tau);
    SacNamed names[2 * DN_ADAM_MAX_TENSORS];
    DnArg in[DN_ADAM_MAX_TENSORS], out[DN_ADAM_MAX_TENSORS];
    for (int i = 0; i < n_tensors; ++i) {
        if (counts[i] < 1 || counts[i] > 0x7fffffffll)
            return fail(DN_ERR_INVALID_ARGUMENT, "counts[%d] must be in 1..2^31 - 1 (got %lld)", i, (long long)counts[i]);
        const uintptr_t bytes = (uintptr_t)counts[i] * sizeof(float);
        in[i] = sac_named(names[2 * i], source[i], bytes, "source[%d]", i);
        out[i] = sac_named(names[2 * i + 1], target[i], bytes, "target[%d]", i);
    }
    const size_t n = (size_t)n_tensors;
    if (const DnArg *a = dn_first_missing(in, n)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_missing(out, n)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_misaligned(in, n, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    if (const DnArg *a = dn_first_misaligned(out, n, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    const DnArg *o, *i;
    if (dn_first_overlap(out, n, in, n, &o, &i)) return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no target may alias a source", o->name, i->name);
    for (size_t a = 0; a + 1 < n; ++a)
        if (dn_first_overlap(&out[a], 1, &out[a + 1], n - a - 1, &o, &i))
            return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: every target is a tensor of its own", o->name, i->name);
    DnPolyakArgs a;
    std::memset(&a, 0, sizeof a);
    for (int k = 0; k < n_tensors; ++k) { a.source[k] = source[k]; a.target[k] = target[k]; a.count[k] = counts[k]; }
    a.tau = tau; a.omt = 1.0 - tau; a.n_tensors = n_tensors;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_polyak(a, (hipStream_t)stream));
    return DN_OK;
}

}  // extern "C"

// ---- dn_lstm: one LSTM layer, the training pass over a sequence and (T = 1) the rollout step -------------------------------------------------
/* what the three entry points ask of cfg, T and B */
static int32_t lstm_shape_ok(const dn_lstm_config *cfg, int64_t T, int64_t B)
{
    if (!cfg) return fail(DN_ERR_INVALID_ARGUMENT, "cfg is required");
    if (cfg->in_dim < 1 || cfg->in_dim > 64) return fail(DN_ERR_INVALID_ARGUMENT, "in_dim must be in 1..64 (got %d)", cfg->in_dim);
    if (cfg->hidden < 32 || cfg->hidden > 512 || cfg->hidden % 32)
        return fail(DN_ERR_INVALID_ARGUMENT, "hidden must be a multiple of 32 in 32..512 (got %d)", cfg->hidden);
    if (cfg->flags & ~(DN_MLP_TRAIN_ACCUMULATE | DN_MLP_TRAIN_NO_PARAM_GRADS))
        return fail(DN_ERR_INVALID_ARGUMENT, "flags has unknown bits: 0x%x (bit 0 accumulates, bit 1 skips the parameter gradients)", cfg->flags);
    if (const int32_t rc = reserved_ok(cfg->reserved)) return rc;
    if (T < 1 || T > DN_LSTM_MAX_STEPS) return fail(DN_ERR_INVALID_ARGUMENT, "T must be in 1..%d (got %lld)", DN_LSTM_MAX_STEPS, (long long)T);
    if (B < 1 || B > (1ll << 24)) return fail(DN_ERR_INVALID_ARGUMENT, "B must be in 1..2^24 (got %lld)", (long long)B);
    if (T * B > (1ll << 24)) return fail(DN_ERR_INVALID_ARGUMENT, "T x B must be <= 2^24 rows (got %lld x %lld)", (long long)T, (long long)B);
    return DN_OK;
}

/* the pointers of a call: required, aligned, the scratch large enough, no output on an input or on another output.  in[LSTM_IN_STARTS]
 * is episode_starts in both calls, bytes that need no alignment; the scratch is the last output, its bytes what the call needs.  `same`:
 * pairs (index into out, index into in) that may be one tensor -- the same address, not a partial overlap. */
constexpr size_t LSTM_IN_STARTS = 1;
static int32_t lstm_pointers_ok(const DnArg *in, size_t ni, const DnArg *out, size_t no, int64_t scratch_bytes, const size_t (*same)[2],
                                size_t n_same)
{
    if (const DnArg *a = dn_first_missing(in, ni)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    if (const DnArg *a = dn_first_missing(out, no)) return fail(DN_ERR_INVALID_ARGUMENT, "%s is required", a->name);
    const DnArg &scratch = out[no - 1];
    if (dn_scratch_short(scratch_bytes, (int64_t)scratch.bytes)) return scratch_too_small(scratch_bytes, (int64_t)scratch.bytes, "dn_lstm_scratch_bytes");
    if ((uintptr_t)scratch.p & 15u) return fail(DN_ERR_INVALID_ARGUMENT, "scratch must be 16-byte aligned");
    for (size_t i = 0; i < ni; ++i)
        if (i != LSTM_IN_STARTS && ((uintptr_t)in[i].p & 3u))
            return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", in[i].name);
    if (const DnArg *a = dn_first_misaligned(out, no, 3u)) return fail(DN_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", a->name);
    for (size_t o = 0; o < no; ++o)
        for (size_t i = 0; i < ni; ++i) {
            if (!dn_ranges_overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) continue;
            bool allowed = false;
            for (size_t s = 0; s < n_same; ++s)
                allowed = allowed || (out[o].p == in[i].p && o == same[s][0] && i == same[s][1]);
            if (!allowed)
                return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: no output may alias an input (h_T may be h0 itself, c_T c0 itself)", out[o].name,
                            in[i].name);
        }
    const DnArg *o, *i;
    for (size_t a = 0; a + 1 < no; ++a)
        if (dn_first_overlap(&out[a], 1, &out[a + 1], no - a - 1, &o, &i))
            return fail(DN_ERR_INVALID_ARGUMENT, "%s overlaps %s: every output is a tensor of its own", o->name, i->name);
    return DN_OK;
}

static void lstm_args(DnLstmArgs &a, const dn_lstm_config *cfg, const dn_lstm_params *p, const float *x, const uint8_t *episode_starts,
                      int64_t T, int64_t B, void *scratch)
{
    std::memset(&a, 0, sizeof a);
    a.w_ih = p->w_ih; a.w_hh = p->w_hh; a.b_ih = p->b_ih; a.b_hh = p->b_hh;
    a.d_w_ih = p->d_w_ih; a.d_w_hh = p->d_w_hh; a.d_b_ih = p->d_b_ih; a.d_b_hh = p->d_b_hh;
    a.x = x; a.episode_starts = episode_starts;
    a.scratch = (char *)scratch;
    a.T = T; a.B = B;
    a.in_dim = cfg->in_dim; a.hidden = cfg->hidden; a.flags = cfg->flags;
}

extern "C" {

int64_t dn_lstm_scratch_bytes(const dn_lstm_config *cfg, int64_t T, int64_t B)
{
    if (const int32_t rc = lstm_shape_ok(cfg, T, B)) return rc;
    return dn_lstm_layout(cfg->in_dim, cfg->hidden, T, B).total;
}

int32_t dn_lstm_forward(const dn_lstm_config *cfg, const dn_lstm_params *params, const float *x, const uint8_t *episode_starts,
                        const float *h0, const float *c0, int64_t T, int64_t B, float *h_seq, float *c_seq, float *h_T, float *c_T,
                        void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = lstm_shape_ok(cfg, T, B)) return rc;
    if (!params) return fail(DN_ERR_INVALID_ARGUMENT, "params is required");
    const uintptr_t I = (uintptr_t)cfg->in_dim, H = (uintptr_t)cfg->hidden, f = sizeof(float), rows = (uintptr_t)(T * B);
    const DnLstmLayout lay = dn_lstm_layout(cfg->in_dim, cfg->hidden, T, B);
    const DnArg in[] = {{"x", x, rows * I * f, false}, {"episode_starts", episode_starts, rows, true}, {"h0", h0, (uintptr_t)B * H * f, false},
                        {"c0", c0, (uintptr_t)B * H * f, false}, {"params.w_ih", params->w_ih, 4 * H * I * f, false},
                        {"params.w_hh", params->w_hh, 4 * H * H * f, false}, {"params.b_ih", params->b_ih, 4 * H * f, false},
                        {"params.b_hh", params->b_hh, 4 * H * f, false}};
    // the forward keeps the activated gates and nothing else: the first region of the scratch is all it asks for
    const DnArg out[] = {{"h_seq", h_seq, rows * H * f, false}, {"c_seq", c_seq, rows * H * f, false}, {"h_T", h_T, (uintptr_t)B * H * f, false},
                         {"c_T", c_T, (uintptr_t)B * H * f, false}, {"scratch", scratch, (uintptr_t)lay.carry_h, false}};
    static const size_t same[][2] = {{2, 2}, {3, 3}};   // (h_T, h0) and (c_T, c0), by their places in out and in
    if (const int32_t rc = lstm_pointers_ok(in, 8, out, 5, scratch_bytes, same, 2)) return rc;
    DnLstmArgs a;
    lstm_args(a, cfg, params, x, episode_starts, T, B, scratch);
    a.h0 = h0; a.c0 = c0; a.h_seq = h_seq; a.c_seq = c_seq; a.h_T = h_T; a.c_T = c_T;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_lstm_forward(a, (hipStream_t)stream));
    return DN_OK;
}

int32_t dn_lstm_backward(const dn_lstm_config *cfg, const dn_lstm_params *params, const float *x, const uint8_t *episode_starts,
                         const float *h0, const float *h_seq, const float *c_seq, const float *c0, const float *d_hseq, int64_t T, int64_t B,
                         float *d_x, void *scratch, int64_t scratch_bytes, int32_t device_id, void *stream)
{
    if (const int32_t rc = lstm_shape_ok(cfg, T, B)) return rc;
    if (!params) return fail(DN_ERR_INVALID_ARGUMENT, "params is required");
    const bool grads = !(cfg->flags & DN_MLP_TRAIN_NO_PARAM_GRADS);
    if (!grads && !d_x)
        return fail(DN_ERR_INVALID_ARGUMENT, "d_x is required with DN_MLP_TRAIN_NO_PARAM_GRADS in flags (there is nothing else to do)");
    const uintptr_t I = (uintptr_t)cfg->in_dim, H = (uintptr_t)cfg->hidden, f = sizeof(float), rows = (uintptr_t)(T * B);
    const DnLstmLayout lay = dn_lstm_layout(cfg->in_dim, cfg->hidden, T, B);
    const DnArg in[] = {{"x", x, rows * I * f, false}, {"episode_starts", episode_starts, rows, true}, {"h0", h0, (uintptr_t)B * H * f, false},
                        {"h_seq", h_seq, rows * H * f, false}, {"c_seq", c_seq, rows * H * f, false}, {"c0", c0, (uintptr_t)B * H * f, false},
                        {"d_hseq", d_hseq, rows * H * f, false}, {"params.w_ih", params->w_ih, 4 * H * I * f, false},
                        {"params.w_hh", params->w_hh, 4 * H * H * f, false}};
    DnArg outs[6];
    size_t no = 0;
    outs[no++] = DnArg{"d_x", d_x, rows * I * f, true};
    if (grads) {                                       // with DN_MLP_TRAIN_NO_PARAM_GRADS the gradient tensors are neither read nor written
        outs[no++] = DnArg{"params.d_w_ih", params->d_w_ih, 4 * H * I * f, false};
        outs[no++] = DnArg{"params.d_w_hh", params->d_w_hh, 4 * H * H * f, false};
        outs[no++] = DnArg{"params.d_b_ih", params->d_b_ih, 4 * H * f, false};
        outs[no++] = DnArg{"params.d_b_hh", params->d_b_hh, 4 * H * f, false};
    }
    outs[no++] = DnArg{"scratch", scratch, (uintptr_t)lay.total, false};
    if (const int32_t rc = lstm_pointers_ok(in, 9, outs, no, scratch_bytes, nullptr, 0)) return rc;
    DnLstmArgs a;
    lstm_args(a, cfg, params, x, episode_starts, T, B, scratch);
    a.h0 = h0; a.c0 = c0; a.h_seq = const_cast<float *>(h_seq); a.c_seq = const_cast<float *>(c_seq); a.d_hseq = d_hseq; a.d_x = d_x;
    DN_HIP(hipSetDevice(device_id));
    DN_HIP(dn_launch_lstm_backward(a, (hipStream_t)stream));
    return DN_OK;
}

}  // extern "C"
