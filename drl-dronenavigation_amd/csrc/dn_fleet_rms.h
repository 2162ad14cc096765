// dn_fleet_rms.h -- the running-moments merge of the fleet-wide normalisers (dn_rownorm.hip, dn_retnorm.hip), which dn_minibatch.hip uses for
// the blocks of a minibatch: device code only, and the only place that holds it.  Every bit of the statistics depends on the order of the
// float64 operations below (the build uses -ffp-contract=off); the merge kernels choose which lane takes which column or step and where
// its moments lie, nothing else.
//
// One lane works on one sequence of (mean, m2) pairs in global memory: the pair of item i has its mean at p[i * stride] and its sum of
// squared deviations (or, after the update, whatever the caller stores) at p[i * stride + off2].  Both walks are sequential chains, so
// both keep FR_BATCH pairs in flight: the next batch is loaded while this one is worked through.
#pragma once

#include "dn_internal.h"

constexpr int FR_BATCH = 8;                            // pairs in flight ahead of the sequential chain

// The sum over the 64 lanes of a wave in a fixed tree (lane i + lane i + 32, then + 16, ... + 1); lane 0 holds it.  The lane order of the
// block moments that are formed a row per lane (dn_retnorm.hip, dn_minibatch.hip) and of the loss heads' block sums (dn_row_sums.h).
__device__ __forceinline__ double fr_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// 1 / x as the step kernels form it (dn_kernels.hip rcp_f64): v_rcp_f64 and two Newton steps, 5 instructions where an IEEE division is ~35
__device__ __forceinline__ double fr_rcp(const double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
}

// (count, mean, m2) <- merged with the next block: nb values of mean bm and sum of squared deviations b2.  The formula of
// update_mean_var_count_from_moments (normalize.py:32-47) on sums of squared deviations, with nb / tot taken once, by reciprocal: the
// counts do not depend on the data, so it stays off the chain mean -> delta -> mean that one lane walks block by block (a step of
// 2 M rows is 2048 blocks).  The reference has no blocks to be literal about; the K updates below are literal.
__device__ __forceinline__ void fr_merge(double &count, double &mean, double &m2, const double nb, const double bm, const double b2)
{
    const double tot = count + nb;
    const double r = nb * fr_rcp(tot);
    const double delta = bm - mean;
    mean = mean + delta * r;
    m2 = m2 + b2 + delta * delta * (count * r);
    count = tot;
}

// The batch moments of one step of n rows: its nblk blocks of DN_ROWNORM_BLOCK_ROWS rows (the last one of what is left) merged in
// ascending block order.  p: the pair of the step's first block.
__device__ __forceinline__ void fr_merge_blocks(const double *p, const long long stride, const long long off2, const long long nblk,
                                                const long long n, double &mean, double &m2)
{
    const long long last_rows = n - (nblk - 1) * DN_ROWNORM_BLOCK_ROWS;
    double count = 0.0;
    mean = 0.0;
    m2 = 0.0;
    double pm[FR_BATCH], p2[FR_BATCH], qm[FR_BATCH], q2[FR_BATCH];
#pragma unroll
    for (int j = 0; j < FR_BATCH; ++j) {
        const bool in = j < nblk;
        pm[j] = in ? p[(long long)j * stride] : 0.0;
        p2[j] = in ? p[(long long)j * stride + off2] : 0.0;
    }
    for (long long b0 = 0; b0 < nblk; b0 += FR_BATCH) {
#pragma unroll
        for (int j = 0; j < FR_BATCH; ++j) {           // the next batch is on its way while this one is merged
            const long long b = b0 + FR_BATCH + j;
            const bool in = b < nblk;
            qm[j] = in ? p[b * stride] : 0.0;
            q2[j] = in ? p[b * stride + off2] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < FR_BATCH; ++j) {
            const long long b = b0 + j;
            if (b < nblk) {
                const double nb = (double)(b == nblk - 1 ? last_rows : DN_ROWNORM_BLOCK_ROWS);
                if (b == 0) { count = nb; mean = pm[j]; m2 = p2[j]; }
                else fr_merge(count, mean, m2, nb, pm[j], p2[j]);
            }
            pm[j] = qm[j];
            p2[j] = q2[j];
        }
    }
}

// The k updates in sequence: the literal arithmetic of normalize.py:32-47 with the n rows of a step as the batch.  s: the pair of step 0,
// holding the step's batch mean and sum of squared deviations; store(t, mean, rstd) keeps what the caller's output stage needs of step t
// -- the mean and 1 / sqrt(var + eps) after the update -- and may overwrite the pair of step t, which has been loaded by then.
template <class Store>
__device__ __forceinline__ void fr_update_steps(const double *s, const long long stride, const long long off2, const long long k,
                                                const long long n, const double eps, double &count, double &mean, double &var, Store store)
{
    const double nn = (double)n;
    double pm[FR_BATCH], p2[FR_BATCH], qm[FR_BATCH], q2[FR_BATCH];
#pragma unroll
    for (int j = 0; j < FR_BATCH; ++j) {
        const bool in = j < k;
        pm[j] = in ? s[(long long)j * stride] : 0.0;
        p2[j] = in ? s[(long long)j * stride + off2] : 0.0;
    }
    for (long long t0 = 0; t0 < k; t0 += FR_BATCH) {
#pragma unroll
        for (int j = 0; j < FR_BATCH; ++j) {
            const long long t = t0 + FR_BATCH + j;
            const bool in = t < k;
            qm[j] = in ? s[t * stride] : 0.0;
            q2[j] = in ? s[t * stride + off2] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < FR_BATCH; ++j) {
            const long long t = t0 + j;
            if (t < k) {
                const double batch_var = p2[j] / nn;                       // np.var: the population variance
                const double delta = pm[j] - mean;
                const double tot = count + nn;
                mean = mean + delta * nn / tot;
                const double m_a = var * count, m_b = batch_var * nn;
                var = (m_a + m_b + delta * delta * count * nn / tot) / tot;
                count = tot;
                store(t, mean, (double)__builtin_amdgcn_rsqf((float)(var + eps)));
            }
            pm[j] = qm[j];
            p2[j] = q2[j];
        }
    }
}
