// dn_row_sums.h -- what the loss heads that work a row per lane share (dn_ppo_loss.hip, dn_sac_loss.hip), and the only place that holds it:
// the move of one row of A float32 columns between memory and registers with the host rule that picks its word size, and the order in
// which per-row float64 terms become one sum per column -- lanes, waves, blocks.  Every bit of the losses and statistics depends on the
// order of the float64 additions below (the build uses -ffp-contract=off); it is a function of the shapes alone, so the same call gives
// the same bits every time.  The kernels choose which lane takes which row, the per-row arithmetic and what becomes of the totals,
// nothing else.
//
// The host rule is plain C++ (dn_capi_envfree.cpp); the rest is device code and builds on the wave tree and FR_BATCH of dn_fleet_rms.h.
#pragma once

#include <stdint.h>

// The 16-byte path of dn_load_row / dn_store_row is taken when every row is a whole number of 16-byte words and each of the [batch][act_dim]
// pointers the kernel moves that way is 16-byte aligned (a NULL optional pointer counts as aligned: it is never followed).  The kernel
// has ONE flag for all of them, so a caller names them all.
template <class... P>
inline bool dn_rows_vec16(const int act_dim, const P *...rows)
{
    return act_dim % 4 == 0 && ((... | (uintptr_t)rows) & 15u) == 0;
}

#ifdef __HIP__
#include "dn_fleet_rms.h"

// One row of A float32 columns into registers: 16-byte words (vec: dn_rows_vec16) or 4-byte words, a wave's A loads of a field covering its
// contiguous 256 A bytes between them.  The same values into the same registers either way, so the same bits.
template <int A>
__device__ __forceinline__ void dn_load_row(const float *__restrict__ p, const long long row, const bool vec, float (&x)[A])
{
    if constexpr (A % 4 == 0) {
        if (vec) {
#pragma unroll
            for (int q = 0; q < A / 4; ++q) {
                const float4 v = reinterpret_cast<const float4 *>(p)[row * (A / 4) + q];
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < A; ++j) x[j] = p[row * A + j];
}

template <int A>
__device__ __forceinline__ void dn_store_row(float *__restrict__ p, const long long row, const bool vec, const float (&x)[A])
{
    if constexpr (A % 4 == 0) {
        if (vec) {
#pragma unroll
            for (int q = 0; q < A / 4; ++q)
                reinterpret_cast<float4 *>(p)[row * (A / 4) + q] = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < A; ++j) p[row * A + j] = x[j];
}

// The NS sums of a workgroup of WAVES waves, one lane's terms being s[] (+0.0 from a lane with no row), in two steps around one barrier.
// fr_wave_to_lds: sum q across the lanes of a wave by the fixed tree of fr_wave_sum, lane 0 of each wave leaving it in wsum[wave][q].
// fr_waves_sum: after the barrier, the waves' sums of column q in ascending wave order.  Every lane of the workgroup must take part.
template <int NS, int WAVES>
__device__ __forceinline__ void fr_wave_to_lds(const int q, const double v, double (&wsum)[WAVES][NS])
{
    const int tid = (int)threadIdx.x;
    const double t = fr_wave_sum(v);
    if ((tid & 63) == 0) wsum[tid >> 6][q] = t;
}

template <int NS, int WAVES>
__device__ __forceinline__ double fr_waves_sum(const double (&wsum)[WAVES][NS], const int q)
{
    double t = 0.0;
    for (int wv = 0; wv < WAVES; ++wv) t += wsum[wv][q];
    return t;
}

// Both steps, into part[block][NS].
template <int NS, int WAVES>
__device__ __forceinline__ void fr_block_sums(const double (&s)[NS], double (&wsum)[WAVES][NS], double *__restrict__ part)
{
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int q = 0; q < NS; ++q) fr_wave_to_lds<NS, WAVES>(q, s[q], wsum);
    __syncthreads();
    if (tid < NS) part[(long long)blockIdx.x * NS + tid] = fr_waves_sum<NS, WAVES>(wsum, tid);
}

// One column of the block sums, p[b * ns] for b = 0 .. nblk - 1, added to 0.0 in ascending order: plain sums, one lane, with FR_BATCH
// loads in flight ahead of the chain.  p: the column's entry of block 0.
__device__ __forceinline__ double fr_sum_column(const double *p, const int ns, const long long nblk)
{
    double t = 0.0;
    double cur[FR_BATCH], nxt[FR_BATCH];
#pragma unroll
    for (int j = 0; j < FR_BATCH; ++j) cur[j] = j < nblk ? p[(long long)j * ns] : 0.0;
    for (long long b0 = 0; b0 < nblk; b0 += FR_BATCH) {
#pragma unroll
        for (int j = 0; j < FR_BATCH; ++j) {           // the next batch is on its way while this one is added
            const long long b = b0 + FR_BATCH + j;
            nxt[j] = b < nblk ? p[b * ns] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < FR_BATCH; ++j) {
            if (b0 + j < nblk) t += cur[j];
            cur[j] = nxt[j];
        }
    }
    return t;
}
#endif  // __HIP__
