// dn_ppo_loss.hip -- the PPO loss head on the device for gfx950 (dn_ppo_loss, include/dronenav.h).
//
// SB3's PPO.train body [from recall] between the three head outputs of a diagonal-Gaussian actor-critic (action means, log_std, values) and
// the scalar loss: the clipped surrogate, the (optionally clipped) value loss, the entropy term, SB3's logged statistics, and the
// gradients of the loss with respect to the three head outputs -- in float64, every input widened once, every output rounded once.
//
// Two ordinary launches on the caller's stream; no workgroup ever waits for another, nothing is allocated, no atomics:
//   1. pl_rows_kernel   one workgroup per block of DN_ROWNORM_BLOCK_ROWS consecutive rows, one row per lane.  Lanes 0 .. A - 1 first
//                       widen log_std and form exp(-log_std) (dn_exp_cr.h) into LDS; after one barrier every lane loads its row (16-byte words when
//                       dn_rows_vec16 holds of mean, actions and d_mean, else 4-byte words: dn_load_row of dn_row_sums.h), evaluates
//                       the expressions of the header and stores d_mean, d_value and log_prob_out.  The block then forms 4 + A float64
//                       sums -- min(p1, p2), (returns - vpred)^2, (ratio - 1) - lr, the clip indicator, and g (z_j^2 - 1) per column --
//                       by fr_block_sums; lanes past the end contribute +0.0.  The sums go to part[block][4 + A].
//   2. pl_merge_kernel  ONE wave: lane q < 4 + A adds column q of the block sums by fr_sum_column; lane 0 then writes stats[8] and the
//                       float32 loss, lanes 4 .. 4 + A - 1 d_log_std.
// The order of every float64 sum is that of dn_row_sums.h, a function of (batch, act_dim) alone: the same call gives the same bits every
// time, and a captured graph replays it.  ratio = exp(lr) is the float64 library function; exp(-log_std) is the correctly rounded one of
// dn_exp_cr.h.
#include "dn_internal.h"
#include "dn_row_sums.h"
#include "dn_exp_cr.h"

namespace {

constexpr int PL_THREADS = (int)DN_ROWNORM_BLOCK_ROWS;  // launch 1: one row per lane, 16 waves
constexpr int PL_WAVES = PL_THREADS / 64;
constexpr double PL_HALF_LOG_2PI = 0.9189385332046727;  // 0.5 log(2 pi)
constexpr double PL_ENTROPY_0 = 1.4189385332046727;     // 0.5 + 0.5 log(2 pi)

template <int A>
__global__ __launch_bounds__(PL_THREADS) void pl_rows_kernel(const DnPpoLossArgs a)
{
    constexpr int NS = 4 + A;
    __shared__ double ls_s[A], inv_s[A];
    __shared__ double wsum[PL_WAVES][NS];

    const int tid = (int)threadIdx.x;
    const long long row0 = (long long)blockIdx.x * PL_THREADS, left = a.batch - row0;                  // left >= 1
    const int nrows = left < PL_THREADS ? (int)left : PL_THREADS;
    const double nb = (double)a.batch;

    if (tid < A) {
        const double ls = (double)a.log_std[tid];
        double inv;
        if (!dn_exp_cr(-ls, inv)) inv = exp(-ls);      // the nearest double to exp(-log_std): logp, and with it every bit of lr, hangs on it
        ls_s[tid] = ls;
        inv_s[tid] = inv;
    }
    __syncthreads();

    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;

    if (tid < nrows) {
        const long long row = row0 + tid;
        float mu[A], ac[A], dm[A];
        dn_load_row<A>(a.mean, row, a.vec != 0, mu);
        dn_load_row<A>(a.actions, row, a.vec != 0, ac);
        const double adv = (double)a.advantages[row], olp = (double)a.old_log_prob[row], ret = (double)a.returns[row];
        const double val = (double)a.value[row];

        double z[A], logp = 0.0;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            z[j] = ((double)ac[j] - (double)mu[j]) * inv_s[j];
            const double t = -0.5 * z[j] * z[j] - ls_s[j] - PL_HALF_LOG_2PI;
            logp = j == 0 ? t : logp + t;
        }
        const double lr = logp - olp, ratio = exp(lr);
        const double lo = 1.0 - a.clip_range, hi = 1.0 + a.clip_range;
        const double rc = ratio < lo ? lo : ratio > hi ? hi : ratio;                                   // a NaN stays a NaN, as in torch.clamp
        const double p1 = adv * ratio, p2 = adv * rc;
        const double pmin = (p1 < p2 || p1 != p1) ? p1 : p2;                                           // torch.min: a NaN on either side wins
        // d min(p1, p2) / d p1, plus what reaches ratio through the clamp: torch.min splits a tie, torch.clamp passes its bounds
        const double w = p1 < p2 ? 1.0 : p1 > p2 ? 0.0 : (ratio >= lo && ratio <= hi) ? 1.0 : 0.5;
        const double g = -adv * w * ratio / nb;                                                        // d loss / d logp

        double vpred = val, inside = 1.0;
        if (a.old_values) {
            const double old = (double)a.old_values[row], d = val - old, cv = a.clip_range_vf;
            const double dc = d < -cv ? -cv : d > cv ? cv : d;
            vpred = old + dc;
            inside = (d >= -cv && d <= cv) ? 1.0 : 0.0;
        }
        const double e = ret - vpred;

#pragma unroll
        for (int j = 0; j < A; ++j) {
            dm[j] = (float)(g * z[j] * inv_s[j]);
            s[4 + j] = g * (z[j] * z[j] - 1.0);
        }
        dn_store_row<A>(a.d_mean, row, a.vec != 0, dm);
        a.d_value[row] = (float)(a.vf_coef * -2.0 * e * inside / nb);
        if (a.log_prob_out) a.log_prob_out[row] = (float)logp;

        s[0] = pmin;
        s[1] = e * e;
        s[2] = (ratio - 1.0) - lr;
        s[3] = fabs(ratio - 1.0) > a.clip_range ? 1.0 : 0.0;
    }

    // fr_block_sums, step by step: handed on as an array, the 12 sums of A = 8 cost the kernel 68 VGPRs for 61, 7 waves per SIMD for 8
#pragma unroll
    for (int q = 0; q < NS; ++q) fr_wave_to_lds<NS, PL_WAVES>(q, s[q], wsum);
    __syncthreads();
    if (tid < NS) a.part[(long long)blockIdx.x * NS + tid] = fr_waves_sum<NS, PL_WAVES>(wsum, tid);
}

__global__ __launch_bounds__(64) void pl_merge_kernel(const DnPpoLossArgs a)
{
    const int q = (int)threadIdx.x, A = a.act_dim, ns = 4 + A;
    const long long nblk = a.nblk;
    double t = 0.0;
    if (q < ns) t = fr_sum_column(a.part + q, ns, nblk);
    const double s0 = __shfl(t, 0, 64), s1 = __shfl(t, 1, 64), s2 = __shfl(t, 2, 64), s3 = __shfl(t, 3, 64);
    const double nb = (double)a.batch;
    if (q == 0) {
        double ent = 0.0;
        for (int j = 0; j < A; ++j) {
            const double h = PL_ENTROPY_0 + (double)a.log_std[j];
            ent = j == 0 ? h : ent + h;
        }
        const double policy_loss = -(s0 / nb), value_loss = s1 / nb, entropy_loss = -ent;
        const double loss = policy_loss + a.ent_coef * entropy_loss + a.vf_coef * value_loss;
        a.stats[0] = loss;
        a.stats[1] = policy_loss;
        a.stats[2] = value_loss;
        a.stats[3] = entropy_loss;
        a.stats[4] = s2 / nb;                          // approx_kl
        a.stats[5] = s3 / nb;                          // clip_fraction
        a.stats[6] = 0.0;
        a.stats[7] = 0.0;
        a.loss[0] = (float)loss;
    }
    if (q >= 4 && q < ns) a.d_log_std[q - 4] = (float)(t - a.ent_coef);
}

template <int A>
void pl_launch_rows(const DnPpoLossArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(pl_rows_kernel<A>, dim3((unsigned)a.nblk), dim3(PL_THREADS), 0, stream, a);
}

}  // namespace

hipError_t dn_launch_ppo_loss(const DnPpoLossArgs &a, hipStream_t stream)
{
    if (dn_ppo_loss_scratch_doubles(a.batch, a.act_dim) == 0 || a.nblk != dn_rownorm_blocks(a.batch)) return hipErrorInvalidValue;
    switch (a.act_dim) {
    case 1: pl_launch_rows<1>(a, stream); break;
    case 2: pl_launch_rows<2>(a, stream); break;
    case 3: pl_launch_rows<3>(a, stream); break;
    case 4: pl_launch_rows<4>(a, stream); break;
    case 5: pl_launch_rows<5>(a, stream); break;
    case 6: pl_launch_rows<6>(a, stream); break;
    case 7: pl_launch_rows<7>(a, stream); break;
    default: pl_launch_rows<8>(a, stream); break;
    }
    hipLaunchKernelGGL(pl_merge_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}
