// dn_minibatch.hip -- PPO minibatches on the device for gfx950 (dn_minibatch, include/dronenav.h).
//
// The reading half of SB3's RolloutBuffer [from recall]: one minibatch of a shuffled epoch gathered straight from the step-major
// [n_steps][n_envs] buffers -- no flattened copy, no permutation array -- and PPO's advantage normalisation of that minibatch.  Sample s
// is drone s / n_steps at step s % n_steps (swap-and-flatten order), so its source row is (s % n_steps) n_envs + s / n_steps.
//
// At most three ordinary launches on the caller's stream; no workgroup ever waits for another, nothing is allocated, no atomics:
//   1. mb_gather_kernel  grid (blocks of DN_ROWNORM_BLOCK_ROWS output rows, fields).  Phase 1: one output row per lane -- its sample, the
//                        clamped index or pi(start + j) of dn_permute.h (the key is formed from kernel arguments and one uniform load:
//                        scalar work, once per wave), and the sample's source row into LDS; the workgroups of field 0 also write
//                        indices_out.  Phase 2, after one barrier: the lanes walk the block's output words of the workgroup's field,
//                        word q = row q / width, column q % width: stores fully coalesced, loads coalesced within a row; 16-byte
//                        words when width % 4 == 0 and both pointers are 16-byte aligned, with the same bits.  The workgroups of the
//                        normalised field (width 1) copy the raw advantages and form the block's mean and sum of squared deviations
//                        in float64, in the SHIFTED form of dn_retnorm.hip (sums of x - x0 and (x - x0)^2, x0 the block's first
//                        gathered value): across the lanes of a wave by a fixed tree, then the waves in ascending order.
//   2. mb_merge_kernel   ONE wave, lane 0: the blocks in ascending order by the merge of dn_fleet_rms.h; mean and std + epsilon (the
//                        unbiased standard deviation) into the scratch's last pair.
//   3. mb_divide_kernel  (a - mean) / (std + epsilon) in float64, a true division, rounded once to float32, in place in the field's dst.
// Launches 2 and 3 run only when a field is normalised and batch > 1.  The order of every float64 operation is a function of `batch`
// alone: the same call gives the same bits every time, and a captured graph replays it.
#include "dn_internal.h"
#include "dn_fleet_rms.h"
#include "dn_permute.h"

namespace {

constexpr int MB_THREADS = (int)DN_ROWNORM_BLOCK_ROWS;  // launch 1: one output row per lane in phase 1, 16 waves
constexpr int MB_WAVES = MB_THREADS / 64;
constexpr int MB_DIVIDE_THREADS = 256;                  // launch 3

typedef uint32_t mb_v4u __attribute__((ext_vector_type(4)));

// The block's output words of one field, in units of T (one 32-bit word, or four): unit q is row q / w, column q % w; lane tid takes
// units tid, tid + MB_THREADS, ... and steps (row, column) along without a division.
template <class T>
__device__ __forceinline__ void mb_copy(const T *__restrict__ src, T *__restrict__ dst, const int *rows, const int w, const int nrows,
                                        const int tid)
{
    const int units = nrows * w, dr = MB_THREADS / w, dc = MB_THREADS % w;
    int r = tid / w, c = tid % w;
#pragma unroll 4
    for (int q = tid; q < units; q += MB_THREADS) {
        dst[q] = src[(long long)rows[r] * w + c];
        r += dr;
        c += dc;
        if (c >= w) { c -= w; ++r; }
    }
}

__global__ __launch_bounds__(MB_THREADS) void mb_gather_kernel(const DnMinibatchArgs a)
{
    __shared__ int rows[MB_THREADS];
    __shared__ double l1[MB_WAVES], l2[MB_WAVES];

    const int tid = (int)threadIdx.x, f = (int)blockIdx.y;
    const unsigned row0 = blockIdx.x * (unsigned)MB_THREADS;                   // < batch <= 2^31 - 1
    const int nrows = (int)(a.batch - row0 < (unsigned)MB_THREADS ? a.batch - row0 : (unsigned)MB_THREADS);     // >= 1
    const bool on = tid < nrows;

    // phase 1: the sample of every output row of the block and its source row
    if (on) {
        const unsigned j = row0 + (unsigned)tid;
        unsigned s;
        if (a.indices) {
            const long long v = a.indices[j];
            s = v < 0 ? 0u : v > (long long)a.m - 1 ? a.m - 1u : (unsigned)v;
        } else {
            const DnPermutation p = dn_permute_make(a.seed, a.epoch + (a.epoch_offset ? (unsigned long long)*a.epoch_offset : 0ull), a.m);
            s = dn_permute_at(p, a.start + j);         // start + j < m
        }
        const unsigned env = s / a.n_steps, step = s - env * a.n_steps;
        rows[tid] = (int)(step * a.n_envs + env);      // < m
        if (f == 0 && a.indices_out) a.indices_out[j] = (long long)s;
    }
    __syncthreads();

    // phase 2: the rows of this workgroup's field
    const dn_minibatch_field fd = a.fields[f];
    const int w = fd.width;
    if (f != a.norm_field) {
        if (w % 4 == 0 && (((uintptr_t)fd.src | (uintptr_t)fd.dst) & 15u) == 0)
            mb_copy(static_cast<const mb_v4u *>(fd.src), static_cast<mb_v4u *>(fd.dst) + (long long)row0 * (w / 4), rows, w / 4, nrows, tid);
        else
            mb_copy(static_cast<const uint32_t *>(fd.src), static_cast<uint32_t *>(fd.dst) + (long long)row0 * w, rows, w, nrows, tid);
        return;                                        // uniform: no barrier follows for this workgroup
    }

    // the advantages (width 1): the raw copy, and the block's moments around its first gathered value
    const float *src = static_cast<const float *>(fd.src);
    const float x = src[rows[on ? tid : 0]], x0 = src[rows[0]];
    if (on) static_cast<float *>(fd.dst)[row0 + (unsigned)tid] = x;
    const double dv = on ? (double)x - (double)x0 : 0.0;
    const double s1 = fr_wave_sum(dv), s2 = fr_wave_sum(dv * dv);
    if ((tid & 63) == 0) {
        l1[tid >> 6] = s1;
        l2[tid >> 6] = s2;
    }
    __syncthreads();
    if (tid == 0) {
        const double nn = (double)nrows;
        double t1 = 0.0, t2 = 0.0;
        for (int wv = 0; wv < MB_WAVES; ++wv) {
            t1 += l1[wv];
            t2 += l2[wv];
        }
        double m2 = t2 - t1 * t1 / nn;
        if (m2 < 0.0) m2 = 0.0;                        // a NaN stays a NaN
        a.part[2ll * blockIdx.x] = (double)x0 + t1 / nn;
        a.part[2ll * blockIdx.x + 1] = m2;
    }
}

__global__ __launch_bounds__(64) void mb_merge_kernel(const DnMinibatchArgs a)
{
    if (threadIdx.x != 0) return;
    const long long nblk = a.nblk;
    double mean, m2;
    fr_merge_blocks(a.part, 2, 1, nblk, a.batch, mean, m2);
    a.part[2 * nblk] = mean;
    a.part[2 * nblk + 1] = sqrt(m2 / ((double)a.batch - 1.0)) + a.eps;         // torch.std: unbiased
}

__global__ __launch_bounds__(MB_DIVIDE_THREADS) void mb_divide_kernel(const DnMinibatchArgs a)
{
    const unsigned j = blockIdx.x * (unsigned)MB_DIVIDE_THREADS + threadIdx.x;
    if (j >= a.batch) return;
    const double *res = a.part + 2ll * a.nblk;
    float *out = static_cast<float *>(a.fields[a.norm_field].dst);
    out[j] = (float)(((double)out[j] - res[0]) / res[1]);
}

}  // namespace

hipError_t dn_launch_minibatch(const DnMinibatchArgs &a, hipStream_t stream)
{
    if (dn_minibatch_scratch_doubles(a.batch) == 0 || a.nblk != dn_rownorm_blocks(a.batch) || a.num_fields < 1 || a.num_fields > DN_MINIBATCH_MAX_FIELDS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mb_gather_kernel, dim3(a.nblk, (unsigned)a.num_fields), dim3(MB_THREADS), 0, stream, a);
    if (a.norm_field >= 0) {
        hipLaunchKernelGGL(mb_merge_kernel, dim3(1), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(mb_divide_kernel, dim3((a.batch - 1) / MB_DIVIDE_THREADS + 1), dim3(MB_DIVIDE_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}
