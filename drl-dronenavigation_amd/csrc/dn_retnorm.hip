// dn_retnorm.hip -- fleet-wide running return normaliser of rewards for gfx950 (dn_retnorm, include/dronenav.h).
//
// The reward half of SB3's VecNormalize [from recall]: one discounted return per drone, ONE RunningMeanStd of those returns over the whole
// fleet (Sol/Model/Environments/normalize.py:10-47 with the N returns of a step as the batch), and the reward divided by the returns'
// standard deviation.  Per step: returns = returns * gamma + r; update with the N returns; out = clip(r / sqrt(var + eps), +-clip) with the
// updated variance (no mean is subtracted); returns = 0 where done.  Env-free, after the step, on step-major float32 [K][N] rewards.
//
// Three ordinary launches on the caller's stream; no workgroup ever waits for another, nothing is allocated, no atomics:
//   1. rt_scan_kernel    one workgroup per block of DN_ROWNORM_BLOCK_ROWS consecutive drones, one drone per lane: the scan over the K
//                        steps is per drone and independent of the statistics.  Per step the block's mean and sum of squared deviations
//                        of the returns in float64, in the SHIFTED form (sums of x - x0 and (x - x0)^2 with x0 the return of the block's
//                        first drone at that step; never E[x^2] - E[x]^2): across the lanes of a wave by a fixed tree, then the waves in
//                        ascending order.  Rewards and done flags are loaded RT_STEPS steps ahead of the scan.  Writes one (mean, m2) per
//                        (step, block) and the final returns.
//   2. rt_merge_kernel   ONE wave, the merge of dn_fleet_rms.h with a lane per step (a row normaliser's lanes are its columns; here there
//                        is one column, so the steps lie side by side in the lanes): each lane merges the blocks of a step in ascending
//                        block order into the step's batch moments; then lane 0 applies the K steps in sequence with the reference's
//                        update, leaving per step a snapshot of 1 / sqrt(var + eps), and the statistics after step K - 1 in `stats`.
//   3. rt_scale_kernel   every reward of step t times the snapshot of step t, clipped: 16-byte loads and stores when both pointers are
//                        16-byte aligned and N is a multiple of 4 (every step then starts on a 16-byte boundary), 4-byte ones otherwise.
// The order of every float64 operation is a function of (K, N) alone, not of the CU count or a launch shape: the same call gives the same
// bits every time, K steps in one call equal K calls of one step, and a captured graph replays it.
// update = 0 is launch 3 alone, every workgroup taking 1 / sqrt(var + eps) from `stats` itself (which is never written).
#include "dn_internal.h"
#include "dn_fleet_rms.h"

namespace {

constexpr int RT_THREADS = (int)DN_ROWNORM_BLOCK_ROWS;  // launch 1: one drone per lane, 16 waves
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_STEPS = 8;                            // launch 1: steps whose rewards and done flags are in flight ahead of the scan
constexpr int RT_MERGE_THREADS = 64;                   // launch 2: one wave, 64 steps side by side
constexpr int RT_SCALE_THREADS = 256;                  // launch 3
constexpr int RT_CHUNK = (int)DN_RETNORM_CHUNK;        // floats per workgroup of launch 3

typedef float rt_v4f __attribute__((ext_vector_type(4)));

struct RtArgs {
    double gamma, eps;
    float clip;
    long long k, n, nblk;
    const float *rewards;
    const uint8_t *done;
    float *out;
    double *stats, *returns, *part, *snap;             // snap == nullptr (update = 0): `stats`
    long long chunks;                                  // launch 3: workgroups per step
};

__global__ __launch_bounds__(RT_THREADS) void rt_scan_kernel(const RtArgs a)
{
    __shared__ double l1[2][RT_STEPS][RT_WAVES], l2[2][RT_STEPS][RT_WAVES], lx[2][RT_STEPS];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * DN_ROWNORM_BLOCK_ROWS;
    const int nrows = (int)(a.n - row0 < DN_ROWNORM_BLOCK_ROWS ? a.n - row0 : DN_ROWNORM_BLOCK_ROWS);      // >= 1
    const bool on = tid < nrows;
    const long long me = row0 + (on ? tid : 0);        // a lane past the fleet's end walks the block's first drone and adds 0
    const double gamma = a.gamma, nn = (double)nrows;

    // every lane also walks the block's first drone (uniform addresses): its return is the shift of every step, and no lane waits for it
    double ret = a.returns[me], ret0 = a.returns[row0];
    int buf = 0;
    for (long long t0 = 0; t0 < a.k; t0 += RT_STEPS, buf ^= 1) {
        float r[RT_STEPS], r0[RT_STEPS];
        uint8_t d[RT_STEPS], d0[RT_STEPS];
#pragma unroll
        for (int j = 0; j < RT_STEPS; ++j) {           // the loads do not depend on the scan: all in flight before it starts
            const long long t = t0 + j < a.k ? t0 + j : a.k - 1;
            r[j] = a.rewards[t * a.n + me];
            d[j] = a.done[t * a.n + me];
            r0[j] = a.rewards[t * a.n + row0];
            d0[j] = a.done[t * a.n + row0];
        }
#pragma unroll
        for (int j = 0; j < RT_STEPS; ++j) {
            if (t0 + j < a.k) {                        // uniform
                ret = ret * gamma + (double)r[j];      // unfused (-ffp-contract=off), as numpy evaluates it
                ret0 = ret0 * gamma + (double)r0[j];
                const double dv = on ? ret - ret0 : 0.0;
                const double s1 = fr_wave_sum(dv), s2 = fr_wave_sum(dv * dv);
                if (lane == 0) {
                    l1[buf][j][wave] = s1;
                    l2[buf][j][wave] = s2;
                    if (wave == 0) lx[buf][j] = ret0;
                }
                if (d[j]) ret = 0.0;
                if (d0[j]) ret0 = 0.0;
            }
        }
        __syncthreads();
        // Lane j of wave 0 finishes step t0 + j: the waves in ascending order.  Two LDS buffers: the next batch's writes go to the other
        // one, and the batch after that writes behind the next barrier, which these lanes reach only after they have read.
        if (tid < RT_STEPS && t0 + tid < a.k) {
            double t1 = 0.0, t2 = 0.0;
            for (int wv = 0; wv < RT_WAVES; ++wv) {
                t1 += l1[buf][tid][wv];
                t2 += l2[buf][tid][wv];
            }
            double m2 = t2 - t1 * t1 / nn;
            if (m2 < 0.0) m2 = 0.0;                    // a NaN stays a NaN
            double *p = a.part + ((t0 + tid) * a.nblk + (long long)blockIdx.x) * 2;
            p[0] = lx[buf][tid] + t1 / nn;
            p[1] = m2;
        }
    }
    // behind at least one barrier (k >= 1): every lane has read returns[row0] before lane 0 overwrites it
    if (on) a.returns[me] = ret;
}

__global__ __launch_bounds__(RT_MERGE_THREADS) void rt_merge_kernel(const RtArgs a)
{
    const int tid = (int)threadIdx.x;

    // the batch moments of every step: a lane per step, 64 steps side by side
    for (long long t = tid; t < a.k; t += RT_MERGE_THREADS) {
        double mean, m2;
        fr_merge_blocks(a.part + t * a.nblk * 2, 2, 1, a.nblk, a.n, mean, m2);
        a.snap[2 * t] = mean;                          // parked in the step's snapshot until the sequential pass below
        a.snap[2 * t + 1] = m2;
    }
    __syncthreads();

    // the K updates in sequence on lane 0: the snapshot of step t becomes 1 / sqrt(var + eps)
    if (tid == 0) {
        double count = a.stats[0], mean = a.stats[1], var = a.stats[2];
        double *s = a.snap;
        fr_update_steps(s, 2, 1, a.k, a.n, a.eps, count, mean, var, [s](const long long t, const double, const double rstd) { s[2 * t] = rstd; });
        a.stats[0] = count;
        a.stats[1] = mean;
        a.stats[2] = var;
    }
}

// The output stage the project uses (dn_rownorm.hip rn_out, without a mean): the reward times the float32 reciprocal square root of
// float32(var + eps).  The clip is two compares and selects: a NaN fails both and stays (fminf / fmaxf drop it).
__device__ __forceinline__ float rt_out(const float x, const float rstd, const float clip)
{
    float y = x * rstd;
    if (y > clip) y = clip;
    if (y < -clip) y = -clip;
    return y;
}

template <bool VEC>
__global__ __launch_bounds__(RT_SCALE_THREADS) void rt_scale_kernel(const RtArgs a)
{
    const int tid = (int)threadIdx.x;
    const long long t = (long long)blockIdx.x / a.chunks, ch = (long long)blockIdx.x - t * a.chunks;
    // update = 0: the statistics as they are, in the merge kernel's own expression
    const float rstd = a.snap ? (float)a.snap[2 * t] : __builtin_amdgcn_rsqf((float)(a.stats[2] + a.eps));
    const long long e0 = ch * RT_CHUNK;
    const int left = (int)(a.n - e0 < RT_CHUNK ? a.n - e0 : RT_CHUNK);      // floats of this chunk: >= 1
    const float *in = a.rewards + t * a.n + e0;
    float *out = a.out + t * a.n + e0;
    const float clip = a.clip;
    if (VEC) {                                         // N % 4 == 0: `left` is a multiple of 4 and every quad is 16-byte aligned
#pragma unroll
        for (int j = 0; j < RT_CHUNK / 4 / RT_SCALE_THREADS; ++j) {
            const int i = 4 * (tid + RT_SCALE_THREADS * j);
            if (i < left) {
                const rt_v4f x = *reinterpret_cast<const rt_v4f *>(in + i);
                rt_v4f y;
                y.x = rt_out(x.x, rstd, clip);
                y.y = rt_out(x.y, rstd, clip);
                y.z = rt_out(x.z, rstd, clip);
                y.w = rt_out(x.w, rstd, clip);
                *reinterpret_cast<rt_v4f *>(out + i) = y;
            }
        }
    } else {
#pragma unroll 8
        for (int j = 0; j < RT_CHUNK / RT_SCALE_THREADS; ++j) {
            const int i = tid + RT_SCALE_THREADS * j;
            if (i < left) out[i] = rt_out(in[i], rstd, clip);
        }
    }
}

__global__ __launch_bounds__(256) void rt_init_kernel(double *stats, double *returns, const long long n)
{
    // RunningMeanStd.__init__ (normalize.py:13-17): count 1e-4, mean 0, var 1; the returns start at 0
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (stats && i < 3) stats[i] = i == 0 ? 1e-4 : i == 1 ? 0.0 : 1.0;
    if (returns && i < n) returns[i] = 0.0;
}

}  // namespace

hipError_t dn_launch_retnorm_init(double *stats, double *returns, long long n, hipStream_t stream)
{
    const long long blocks = returns ? (n + 255) / 256 : 1;
    if ((returns && n < 1) || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rt_init_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, stats, returns, n);
    return hipGetLastError();
}

hipError_t dn_launch_retnorm(double gamma, double epsilon, float clip, double *stats, double *returns, long long k, long long n,
                             const float *rewards, const uint8_t *done, float *out, int update, double *scratch, hipStream_t stream)
{
    if (dn_retnorm_scratch_doubles(k, n) == 0 || !dn_retnorm_grids_ok(k, n)) return hipErrorInvalidValue;
    RtArgs a;
    a.gamma = gamma; a.eps = epsilon; a.clip = clip;
    a.k = k; a.n = n; a.nblk = dn_rownorm_blocks(n);
    a.rewards = rewards; a.done = done; a.out = out;
    a.stats = stats; a.returns = returns;
    a.part = scratch;
    a.snap = update ? scratch + k * a.nblk * 2 : nullptr;
    a.chunks = dn_retnorm_chunks(n);
    if (update) {
        hipLaunchKernelGGL(rt_scan_kernel, dim3((unsigned)a.nblk), dim3(RT_THREADS), 0, stream, a);
        hipLaunchKernelGGL(rt_merge_kernel, dim3(1), dim3(RT_MERGE_THREADS), 0, stream, a);
    }
    if (out) {
        const bool vec = n % 4 == 0 && (((uintptr_t)rewards | (uintptr_t)out) & 15u) == 0;
        if (vec) hipLaunchKernelGGL(rt_scale_kernel<true>, dim3((unsigned)(k * a.chunks)), dim3(RT_SCALE_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(rt_scale_kernel<false>, dim3((unsigned)(k * a.chunks)), dim3(RT_SCALE_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}
