// dn_glue.hip -- the rollout glue around the environment step: GAE, the episode-done compaction, the action chain on its own, the two
// policy samplers, the truncation bootstrap, the step-counter set, the fills and the stream copy.  None of them contains the step body,
// so none needs the step file's two builds (machine LICM on / off, the normaliser's exact output stage): this unit is compiled once, with
// the default flags (build.py), and both libraries link the same object.  What the samplers and the action-chain kernel share with the
// step kernels -- the float32 action chain, the Philox streams, the policy draws -- is in the three headers below, stated once.
//
// Reference citations are file:line of the reference sources, under the names dn_kernels.hip lists.
#include "dn_internal.h"
#include "dn_action_chain.h"
#include "dn_philox.h"
#include "dn_policy_draw.h"

namespace {

// =====================================================================================================
// N1: GAE, one lane per drone, time-reversed scan (cleanRLPPO.py:234-248).  float32, unfused, in the
// reference's operation order so the result is bit-identical to the torch float32 loop.
// =====================================================================================================
__global__ __launch_bounds__(256) void dn_gae_kernel(const float *__restrict__ rewards, const float *__restrict__ values,
                                                     const uint8_t *__restrict__ dones, const float *__restrict__ last_values,
                                                     const uint8_t *__restrict__ last_dones, long long T, long long N,
                                                     float gamma, float gl, float *__restrict__ adv, float *__restrict__ ret)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float last = 0.0f;
    float nnt = 1.0f - (float)last_dones[i];
    float nv = last_values[i];
    for (long long t = T - 1; t >= 0; --t) {
        const float v = values[t * N + i];
        float gv = gamma * nv;
        float delta = rewards[t * N + i] + gv * nnt;
        delta = delta - v;
        float k = gl * nnt;
        last = delta + k * last;
        adv[t * N + i] = last;
        ret[t * N + i] = last + v;
        nnt = 1.0f - (float)dones[t * N + i];
        nv = v;
    }
}

// =====================================================================================================
// Episode-done compaction: ballot words -> ordered index list (popcount + block-wide exclusive scan).
// One workgroup of 1024 lanes per 1024 words (65 536 drones), one word per lane.  A workgroup's place in the list is the
// number of set bits in all earlier words, which it counts itself (coalesced popcount sweep + reduction: at 2 M drones the
// last of 32 workgroups re-reads 256 KB out of L2) -- no second launch, no scratch buffer, no atomics, and the list stays in
// ascending order whatever order the workgroups run in.
// =====================================================================================================
// The scan both compaction kernels start with: this lane's word (index w, bits mword), the list position `pos` of its first set bit and
// the running `total` of set bits up to and including its word.  The kernels keep only their write loops.
struct CompactScan {
    long long w;
    unsigned long long mword;
    int pos, total;
};
DN_DEV CompactScan compact_scan(const unsigned long long *__restrict__ mask, const long long n)
{
    __shared__ int s_wave[16], s_before[16];
    const long long words = (n + 63) / 64;
    const long long w_base = (long long)blockIdx.x * 1024;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before = 0;
    for (long long w = threadIdx.x; w < w_base; w += 1024) before += __popcll(mask[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    const long long w = w_base + threadIdx.x;
    const unsigned long long mword = w < words ? mask[w] : 0ull;
    const int mine = __popcll(mword);
    // exclusive scan: within the wave by shuffles, across the 16 waves through LDS
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    if (lane == 0) s_before[wave] = before;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < 16; ++k) base += s_before[k];
    for (int k = 0; k < wave; ++k) base += s_wave[k];
    return {w, mword, base + incl - mine, base + incl};
}

__global__ __launch_bounds__(1024) void dn_compact_kernel(const unsigned long long *__restrict__ mask, long long n,
                                                          int32_t *__restrict__ indices, int32_t *__restrict__ count)
{
    const CompactScan s = compact_scan(mask, n);
    unsigned long long mword = s.mword;
    int pos = s.pos;
    while (mword) {
        int b = __ffsll((long long)mword) - 1;
        indices[pos++] = (int32_t)(s.w * 64 + b);
        mword &= mword - 1;
    }
    if (threadIdx.x == 1023 && blockIdx.x == gridDim.x - 1) *count = s.total;
}

// dn_pack_done: the compaction above with, next to every index, the episode-end record of that drone as ONE 64-byte row --
// terminal_observation (13), Monitor return, Monitor length (int bits), TimeLimit.truncated | found_targets << 8 (int bits) -- so that
// the NumPy step() brings the few finished drones' records to the host in one short copy instead of four whole per-drone arrays.
__global__ __launch_bounds__(1024) void dn_compact_pack_kernel(const unsigned long long *__restrict__ mask, long long n,
                                                               const float *__restrict__ terminal_obs, const float *__restrict__ ep_return,
                                                               const int32_t *__restrict__ ep_length, const uint8_t *__restrict__ truncated,
                                                               const int32_t *__restrict__ found, int32_t *__restrict__ indices,
                                                               int32_t *__restrict__ count, float *__restrict__ packed)
{
    const CompactScan s = compact_scan(mask, n);
    unsigned long long mword = s.mword;
    int pos = s.pos;
    while (mword) {
        const int b = __ffsll((long long)mword) - 1;
        const long long i = s.w * 64 + b;
        indices[pos] = (int32_t)i;
        float *row = packed + (long long)pos * 16;
#pragma unroll
        for (int k = 0; k < DN_OBS_DIM; ++k) row[k] = terminal_obs[i * DN_OBS_DIM + k];
        row[13] = ep_return[i];
        row[14] = __int_as_float(ep_length[i]);
        row[15] = __int_as_float((int)truncated[i] | (found[i] << 8));
        ++pos;
        mword &= mword - 1;
    }
    if (threadIdx.x == 1023 && blockIdx.x == gridDim.x - 1) *count = s.total;
}

// A1-A3 on their own (dn_preprocess_action): N x PBDroneEnv._preprocessAction + the force/torque lines of
// BaseAviary._physics, so the float32 chain can be checked bit for bit against the reference's golden vectors.
__global__ __launch_bounds__(256) void dn_action_chain_kernel(const float4 *__restrict__ actions, long long n, int normalize_actions,
                                                              float4 *__restrict__ rpm, float4 *__restrict__ forces,
                                                              float *__restrict__ z_torque)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 A = actions[i];
    const float a[4] = {A.x, A.y, A.z, A.w};
    float tq[4], f[4], r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float tq_chain;
        rotor_force_from_action(a[j], normalize_actions != 0, tq_chain, &r[j]);          // the rpm output: the chain itself
        f[j] = rotor_force_sat(a[j], normalize_actions != 0, tq[j]);                     // forces / torque: the path the step kernels take
    }
    if (rpm) rpm[i] = make_float4(r[0], r[1], r[2], r[3]);
    if (forces) forces[i] = make_float4(f[0], f[1], f[2], f[3]);
    if (z_torque) z_torque[i] = z_torque32(tq);
}

// Rollout-step glue around the policy network (the host loop's small element-wise kernels, fused):
//   dn_policy_sample_kernel  -- SB3 DiagGaussianDistribution.sample / log_prob and the np.clip of collect_rollouts
//                               [3P-recall]: actions = mean + exp(log_std) z, z ~ N(0,1) from the environment's Philox
//                               stream (seed, global drone id, the tile's vector-step counter, stream 9), the clipped copy
//                               that goes to dn_step, and log N(actions; mean, std) summed over the four action dims.
//   dn_add_bootstrap_kernel  -- reward += gamma * V(terminal_observation) where TimeLimit.truncated (SB3's
//                               collect_rollouts bootstrap) [3P-recall].
__global__ __launch_bounds__(256) void dn_policy_sample_kernel(const DnParams p, const float4 *__restrict__ mean,
                                                               const float4 log_std, const unsigned long long seed,
                                                               const int deterministic, float4 *__restrict__ actions,
                                                               float4 *__restrict__ clipped, float *__restrict__ log_prob)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const float4 m = mean[i];
    const float mu[4] = {m.x, m.y, m.z, m.w};
    const float ls[4] = {log_std.x, log_std.y, log_std.z, log_std.w};
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!deterministic)
        noise4(seed, (unsigned long long)(p.env_id_offset + i), p.st.stats[i / DN_BLOCK].step_count, 9u, z);
    float a[4], lp;
    gaussian_draw(mu, ls, z, a, lp);
    actions[i] = make_float4(a[0], a[1], a[2], a[3]);
    clipped[i] = make_float4(clipv(a[0], -1.0f, 1.0f), clipv(a[1], -1.0f, 1.0f), clipv(a[2], -1.0f, 1.0f), clipv(a[3], -1.0f, 1.0f));
    log_prob[i] = lp;
}

// dn_squashed_sample_kernel -- SB3 SAC's Actor on top of the (mu | log_std) rows of dn_mlp_forward(arch = SAC) [3P-recall of
// sac/policies.py and SquashedDiagGaussianDistribution]: log_std clamped to [-20, 2], pre = mu + exp(log_std) z with z ~ N(0,1)
// from the environment's Philox stream (seed, global drone id, the tile's vector-step counter, stream 9: as dn_policy_sample),
// action = tanh(pre) -- already inside dn_step's [-1, 1] --, log_prob = sum_j log N(pre_j; mu_j, sigma_j) - log(1 - a_j^2 + 1e-6).
__global__ __launch_bounds__(256) void dn_squashed_sample_kernel(const DnParams p, const float4 *__restrict__ mu_log_std,
                                                                 const unsigned long long seed, const int deterministic,
                                                                 float4 *__restrict__ actions, float *__restrict__ log_prob)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!deterministic)
        noise4(seed, (unsigned long long)(p.env_id_offset + i), p.st.stats[i / DN_BLOCK].step_count, 9u, z);
    float a[4], lp;
    squashed_draw(mu_log_std[2 * i], mu_log_std[2 * i + 1], z, log_prob != nullptr, a, lp);
    actions[i] = make_float4(a[0], a[1], a[2], a[3]);
    if (log_prob) log_prob[i] = lp;
}

__global__ __launch_bounds__(256) void dn_add_bootstrap_kernel(float *__restrict__ reward, const float *__restrict__ terminal_value,
                                                               const uint8_t *__restrict__ truncated, float gamma, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && truncated[i]) reward[i] = reward[i] + gamma * terminal_value[i];
}

__global__ __launch_bounds__(256) void dn_set_step_count_kernel(DnStatSlot *slots, long long blocks, unsigned long long value)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < blocks; i += (long long)gridDim.x * blockDim.x)
        slots[i].step_count = value;
}

__global__ __launch_bounds__(256) void dn_fill4_kernel(float4 *dst, float4 v, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = v;
}
// The copy ceiling of the box (dn_stream_copy): ONE 16-byte load and one 16-byte store per lane, no loop -- the form that measured
// fastest on MI355X (profiles/r04_copy_sweep.txt: 6 237 GB/s read + write over 1 GiB, against 4 100-5 200 for grid-stride loops of
// 4-64 workgroups per CU with or without non-temporal hints, 5 300-5 750 for a contiguous chunk per workgroup, 4 689 for hipMemcpyAsync
// and ~5 500 for torch's copy_): the dispatcher streams workgroups onto CUs as they drain, and every wave has exactly one load in flight.
typedef float dn_v4f __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void dn_stream_copy_kernel(const float4 *__restrict__ src4, float4 *__restrict__ dst4, long long n16)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) reinterpret_cast<dn_v4f *>(dst4)[i] = reinterpret_cast<const dn_v4f *>(src4)[i];
}
__global__ __launch_bounds__(256) void dn_filld_kernel(double *dst, double v, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = v;
}

}  // namespace

hipError_t dn_launch_fill4(float4 *dst, float4 v, long long n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(dn_fill4_kernel, dim3(grid), dim3(256), 0, stream, dst, v, n);
    return hipGetLastError();
}

hipError_t dn_launch_stream_copy(void *dst, const void *src, long long n16, int num_cus, hipStream_t stream)
{
    (void)num_cus;
    const long long per = 256ll * 0x40000000ll;                  // grid.x <= 2^30 workgroups per launch
    for (long long off = 0; off < n16; off += per) {
        const long long m = n16 - off < per ? n16 - off : per;
        hipLaunchKernelGGL(dn_stream_copy_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const float4 *)src + off, (float4 *)dst + off, m);
    }
    return hipGetLastError();
}

hipError_t dn_launch_filld(double *dst, double v, long long n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(dn_filld_kernel, dim3(grid), dim3(256), 0, stream, dst, v, n);
    return hipGetLastError();
}

hipError_t dn_launch_gae(const float *rewards, const float *values, const uint8_t *dones, const float *last_values,
                         const uint8_t *last_dones, long long T, long long N, float gamma, float gl, float *adv,
                         float *ret, hipStream_t stream)
{
    const unsigned grid = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(dn_gae_kernel, dim3(grid), dim3(256), 0, stream, rewards, values, dones, last_values,
                       last_dones, T, N, gamma, gl, adv, ret);
    return hipGetLastError();
}

hipError_t dn_launch_action_chain(const float *actions, long long n, int normalize_actions, float *rpm, float *forces,
                                  float *z_torque, hipStream_t stream)
{
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(dn_action_chain_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4 *>(actions), n,
                       normalize_actions, reinterpret_cast<float4 *>(rpm), reinterpret_cast<float4 *>(forces), z_torque);
    return hipGetLastError();
}

hipError_t dn_launch_squashed_sample(const DnParams &p, const float *mu_log_std, unsigned long long seed, int deterministic,
                                     float *actions, float *log_prob, hipStream_t stream)
{
    const unsigned grid = (unsigned)((p.n + 255) / 256);
    hipLaunchKernelGGL(dn_squashed_sample_kernel, dim3(grid), dim3(256), 0, stream, p, reinterpret_cast<const float4 *>(mu_log_std),
                       seed, deterministic, reinterpret_cast<float4 *>(actions), log_prob);
    return hipGetLastError();
}

hipError_t dn_launch_policy_sample(const DnParams &p, const float *mean, const float *log_std4, unsigned long long seed, int deterministic,
                                   float *actions, float *clipped, float *log_prob, hipStream_t stream)
{
    const unsigned grid = (unsigned)((p.n + 255) / 256);
    hipLaunchKernelGGL(dn_policy_sample_kernel, dim3(grid), dim3(256), 0, stream, p, reinterpret_cast<const float4 *>(mean),
                       make_float4(log_std4[0], log_std4[1], log_std4[2], log_std4[3]), seed, deterministic,
                       reinterpret_cast<float4 *>(actions), reinterpret_cast<float4 *>(clipped), log_prob);
    return hipGetLastError();
}

hipError_t dn_launch_add_bootstrap(float *reward, const float *terminal_value, const uint8_t *truncated, float gamma, long long n,
                                   hipStream_t stream)
{
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(dn_add_bootstrap_kernel, dim3(grid), dim3(256), 0, stream, reward, terminal_value, truncated, gamma, n);
    return hipGetLastError();
}

hipError_t dn_launch_set_step_count(DnStatSlot *slots, long long blocks, unsigned long long value, hipStream_t stream)
{
    const unsigned grid = (unsigned)((blocks + 255) / 256 < 1024 ? (blocks + 255) / 256 : 1024);
    hipLaunchKernelGGL(dn_set_step_count_kernel, dim3(grid), dim3(256), 0, stream, slots, blocks, value);
    return hipGetLastError();
}

hipError_t dn_launch_compact(const unsigned long long *mask, long long n, int32_t *indices, int32_t *count,
                             hipStream_t stream)
{
    const unsigned blocks = (unsigned)(((n + 63) / 64 + 1023) / 1024);
    hipLaunchKernelGGL(dn_compact_kernel, dim3(blocks), dim3(1024), 0, stream, mask, n, indices, count);
    return hipGetLastError();
}
hipError_t dn_launch_compact_pack(const unsigned long long *mask, long long n, const float *terminal_obs, const float *ep_return,
                                  const int32_t *ep_length, const uint8_t *truncated, const int32_t *found, int32_t *indices, int32_t *count,
                                  float *packed, hipStream_t stream)
{
    const unsigned blocks = (unsigned)(((n + 63) / 64 + 1023) / 1024);
    hipLaunchKernelGGL(dn_compact_pack_kernel, dim3(blocks), dim3(1024), 0, stream, mask, n, terminal_obs, ep_return, ep_length, truncated, found,
                       indices, count, packed);
    return hipGetLastError();
}
