// dn_rownorm.hip -- fleet-wide running normaliser of policy and critic input rows for gfx950 (dn_rownorm, include/dronenav.h).
//
// One RunningMeanStd over the whole fleet per row kind (Sol/Model/Environments/normalize.py:10-47: RunningMeanStd and
// update_mean_var_count_from_moments), with the N rows of a step as the batch, and SB3's VecNormalize order within a step: update with
// the step's rows, then normalise them with the updated statistics.  Env-free, after the step, on dense float32 rows [K][N][W].
//
// Three ordinary launches on the caller's stream; no workgroup ever waits for another, nothing is allocated, no atomics:
//   1. rn_partial_kernel   one workgroup per (step, block of DN_ROWNORM_BLOCK_ROWS consecutive rows): per column the block's mean and
//                          sum of squared deviations in float64, in the SHIFTED form (sums of x - x0 and (x - x0)^2 with x0 the
//                          block's first row; never E[x^2] - E[x]^2 of the raw values).  4-byte loads, a wave reading whole rows side by
//                          side (rows are 4-byte aligned only, and the pass is a reduction: a row's words go to different columns).
//   2. rn_merge_kernel     ONE workgroup, the merge of dn_fleet_rms.h with a lane per column: 8 steps at a time (one per wave), each
//                          step's blocks merged in ascending block order into the step's batch moments; then the lanes of wave 0 take the
//                          K steps in sequence with the reference's update, leaving per step a snapshot of the mean and of
//                          1 / sqrt(var + eps), and the statistics after step K - 1 in `stats`.
//   3. rn_normalize_kernel every row of step t with the snapshot of step t: 16-byte loads and stores when the width is a multiple of 4 and
//                          both pointers are 16-byte aligned (decided from the pointers at run time), 4-byte ones otherwise.
// The order of every float64 operation is a function of (K, N, W) alone, not of the CU count or a launch shape: the same call gives the
// same bits every time, K steps in one call equal K calls of one step, and a captured graph replays it.
// update = 0 is launch 3 alone, every workgroup taking mean and 1 / sqrt(var + eps) from `stats` itself (which is never written).
#include "dn_internal.h"
#include "dn_fleet_rms.h"

namespace {

constexpr int RN_THREADS = 1024;                       // launch 1: 16 waves
constexpr int RN_WAVES = RN_THREADS / 64;
constexpr int RN_MERGE_THREADS = 512;                  // launch 2: 8 steps side by side (1024 threads leave 128 registers: the batches spill)
constexpr int RN_MERGE_STEPS = RN_MERGE_THREADS / 64;
constexpr int RN_NORM_THREADS = 256;                   // launch 3
constexpr int RN_CHUNK = 4096;                         // floats per workgroup of launch 3

typedef float rn_v4f __attribute__((ext_vector_type(4)));

struct RnArgs {
    int w;
    float clip;
    double eps;
    long long k, n, nblk;
    const float *rows;
    float *out;
    double *stats, *part, *snap;
    long long snap_stride;                             // doubles between the snapshots of two steps; snap == nullptr (update = 0): `stats`
    long long chunks;                                  // launch 3: workgroups per step
};

__global__ __launch_bounds__(RN_THREADS) void rn_partial_kernel(const RnArgs a)
{
    __shared__ double l1[RN_THREADS], l2[RN_THREADS];

    const int w = a.w, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rpw = 64 / w;                            // rows a wave reads with one instruction: 1 (W > 32) .. 64 (W = 1)
    const int sub = lane / w, c = lane - sub * w;
    const bool on = sub < rpw;
    const int groups = RN_WAVES * rpw, gid = wave * rpw + sub;      // row r of the block belongs to group r % groups
    const long long t = (long long)blockIdx.x / a.nblk, b = (long long)blockIdx.x - t * a.nblk;
    const long long row0 = b * DN_ROWNORM_BLOCK_ROWS;
    const int nrows = (int)(a.n - row0 < DN_ROWNORM_BLOCK_ROWS ? a.n - row0 : DN_ROWNORM_BLOCK_ROWS);      // >= 1
    const float *base = a.rows + (t * a.n + row0) * w;

    double s1 = 0.0, s2 = 0.0;
    const double x0 = on ? (double)base[c] : 0.0;      // the shift: the column's value in the block's first row
    if (on) {
#pragma unroll 8
        for (int r = gid; r < nrows; r += groups) {
            const double d = (double)base[r * w + c] - x0;
            s1 += d;
            s2 = __builtin_fma(d, d, s2);
        }
    }
    l1[tid] = s1;
    l2[tid] = s2;
    __syncthreads();
    if (tid < w) {                                     // wave 0, sub 0: c == tid and x0 is this column's
        double t1 = 0.0, t2 = 0.0;
        for (int wv = 0; wv < RN_WAVES; ++wv)          // the groups in ascending order
            for (int sb = 0; sb < rpw; ++sb) {
                t1 += l1[wv * 64 + sb * w + tid];
                t2 += l2[wv * 64 + sb * w + tid];
            }
        const double nn = (double)nrows;
        double m2 = t2 - t1 * t1 / nn;
        if (m2 < 0.0) m2 = 0.0;                        // a NaN stays a NaN
        double *p = a.part + (long long)blockIdx.x * (2 * w);
        p[tid] = x0 + t1 / nn;
        p[w + tid] = m2;
    }
}

__global__ __launch_bounds__(RN_MERGE_THREADS) void rn_merge_kernel(const RnArgs a)
{
    const int w = a.w, tid = (int)threadIdx.x, c = tid & 63, sl = tid >> 6;
    const bool on = c < w;

    // the batch moments of every step: a lane per column, 8 steps side by side
    for (long long t = sl; t < a.k; t += RN_MERGE_STEPS) {
        if (on) {
            double mean, m2;
            fr_merge_blocks(a.part + t * a.nblk * (2 * w) + c, 2 * w, w, a.nblk, a.n, mean, m2);
            a.snap[t * (2 * w) + c] = mean;            // parked in the step's snapshot until the sequential pass below
            a.snap[t * (2 * w) + w + c] = m2;
        }
    }
    __syncthreads();

    // the K updates in sequence, one lane per column: the snapshot of step t becomes its mean and 1 / sqrt(var + eps)
    if (sl == 0 && on) {
        double count = a.stats[0], mean = a.stats[1 + c], var = a.stats[1 + w + c];
        double *s = a.snap + c;
        fr_update_steps(s, 2 * w, w, a.k, a.n, a.eps, count, mean, var, [s, w](const long long t, const double m, const double rstd) {
            s[t * (2 * w)] = m;
            s[t * (2 * w) + w] = rstd;
        });
        if (c == 0) a.stats[0] = count;
        a.stats[1 + c] = mean;
        a.stats[1 + w + c] = var;
    }
}

// The output stage the step kernels use (dn_kernels.hip normalize_obs_cols): x - mean in float64, rounded to float32, times the float32
// reciprocal square root of float32(var + eps).  The clip is two compares and selects: a NaN fails both and stays (fminf / fmaxf drop it).
__device__ __forceinline__ float rn_out(const float x, const double mean, const float rstd, const float clip)
{
    float y = (float)((double)x - mean) * rstd;
    if (y > clip) y = clip;
    if (y < -clip) y = -clip;
    return y;
}

template <bool VEC>
__global__ __launch_bounds__(RN_NORM_THREADS) void rn_normalize_kernel(const RnArgs a)
{
    __shared__ double smean[DN_ROWNORM_MAX_WIDTH];
    __shared__ float srstd[DN_ROWNORM_MAX_WIDTH];

    const int w = a.w, tid = (int)threadIdx.x;
    const long long t = (long long)blockIdx.x / a.chunks, ch = (long long)blockIdx.x - t * a.chunks;
    if (tid < w) {
        if (a.snap) {
            const double *s = a.snap + t * a.snap_stride;
            smean[tid] = s[tid];
            srstd[tid] = (float)s[w + tid];
        } else {                                       // update = 0: the statistics as they are, in the merge kernel's own expression
            smean[tid] = a.stats[1 + tid];
            srstd[tid] = __builtin_amdgcn_rsqf((float)(a.stats[1 + w + tid] + a.eps));
        }
    }
    __syncthreads();
    const long long step_elems = a.n * w, e0 = ch * RN_CHUNK;
    const int left = (int)(step_elems - e0 < RN_CHUNK ? step_elems - e0 : RN_CHUNK);      // floats of this chunk: >= 1
    const int c0 = (int)(e0 % w);                                                         // the column of the chunk's first float
    const float *in = a.rows + t * step_elems + e0;
    float *out = a.out + t * step_elems + e0;
    const float clip = a.clip;
    if (VEC) {                                         // W % 4 == 0: a quad lies in one row, and `left` is a multiple of 4
#pragma unroll
        for (int j = 0; j < RN_CHUNK / 4 / RN_NORM_THREADS; ++j) {
            const int i = 4 * (tid + RN_NORM_THREADS * j);
            if (i < left) {
                const int c = (c0 + i) % w;
                const rn_v4f x = *reinterpret_cast<const rn_v4f *>(in + i);
                rn_v4f y;
                y.x = rn_out(x.x, smean[c], srstd[c], clip);
                y.y = rn_out(x.y, smean[c + 1], srstd[c + 1], clip);
                y.z = rn_out(x.z, smean[c + 2], srstd[c + 2], clip);
                y.w = rn_out(x.w, smean[c + 3], srstd[c + 3], clip);
                *reinterpret_cast<rn_v4f *>(out + i) = y;
            }
        }
    } else {
#pragma unroll 8
        for (int j = 0; j < RN_CHUNK / RN_NORM_THREADS; ++j) {
            const int i = tid + RN_NORM_THREADS * j;
            if (i < left) {
                const int c = (c0 + i) % w;
                out[i] = rn_out(in[i], smean[c], srstd[c], clip);
            }
        }
    }
}

__global__ __launch_bounds__(64) void rn_init_kernel(double *stats, const int w)
{
    // RunningMeanStd.__init__ (normalize.py:13-17): mean 0, var 1, count 1e-4
    for (int i = (int)threadIdx.x; i < 1 + 2 * w; i += 64) stats[i] = i == 0 ? 1e-4 : i <= w ? 0.0 : 1.0;
}

}  // namespace

hipError_t dn_launch_rownorm_init(int width, double *stats, hipStream_t stream)
{
    if (width < 1 || width > DN_ROWNORM_MAX_WIDTH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rn_init_kernel, dim3(1), dim3(64), 0, stream, stats, width);
    return hipGetLastError();
}

hipError_t dn_launch_rownorm(int width, float clip, double epsilon, double *stats, long long k, long long n, const float *rows, float *out,
                             int update, double *scratch, hipStream_t stream)
{
    if (dn_rownorm_scratch_doubles(k, n, width) == 0) return hipErrorInvalidValue;
    RnArgs a;
    a.w = width; a.clip = clip; a.eps = epsilon;
    a.k = k; a.n = n; a.nblk = dn_rownorm_blocks(n);
    a.rows = rows; a.out = out; a.stats = stats;
    a.part = scratch;
    a.snap = update ? scratch + k * a.nblk * 2 * width : nullptr;
    a.snap_stride = 2 * width;
    a.chunks = (n * width + RN_CHUNK - 1) / RN_CHUNK;
    if (k * a.nblk > 0x7fffffffll || k * a.chunks > 0x7fffffffll) return hipErrorInvalidValue;
    if (update) {
        hipLaunchKernelGGL(rn_partial_kernel, dim3((unsigned)(k * a.nblk)), dim3(RN_THREADS), 0, stream, a);
        hipLaunchKernelGGL(rn_merge_kernel, dim3(1), dim3(RN_MERGE_THREADS), 0, stream, a);
    }
    if (out) {
        const bool vec = width % 4 == 0 && (((uintptr_t)rows | (uintptr_t)out) & 15u) == 0;
        if (vec) hipLaunchKernelGGL(rn_normalize_kernel<true>, dim3((unsigned)(k * a.chunks)), dim3(RN_NORM_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(rn_normalize_kernel<false>, dim3((unsigned)(k * a.chunks)), dim3(RN_NORM_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}
