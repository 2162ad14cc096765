// dn_sac_loss.hip -- the SAC loss heads on the device for gfx950 (dn_sac_policy, dn_sac_policy_backward, dn_sac_critic_loss,
// dn_sac_actor_loss; include/dronenav.h).
//
// SB3's SAC.train body [from recall] between the networks' head outputs and the scalar losses: the squashed Gaussian's reparametrised
// sample with its log-probability and their backward, the TD target with the critic loss, the actor loss and the entropy-coefficient loss,
// and the gradients with respect to every head output -- in float64, every input widened once, every output rounded once.  The per-element
// arithmetic is csrc/dn_sac_math.h, which the host runs as well; this file chooses which lane takes which row and in which order sums
// are added, nothing else.
//
// Ordinary launches on the caller's stream; no workgroup ever waits for another, nothing is allocated, no atomics:
//   sl_policy_kernel<A, BWD>  one row per lane, 256 rows per workgroup, the row's A columns in registers (16-byte words when dn_rows_vec16
//                             holds of every [batch][A] pointer of the call, else 4-byte words: dn_load_row of dn_row_sums.h).  Forward
//                             stores actions and log_prob; backward recomputes the element from mean, log_std and noise and stores d_mean
//                             and d_log_std.  No reduction, no scratch.
//   sl_critic_rows_kernel<C>  one workgroup per block of DN_ROWNORM_BLOCK_ROWS consecutive rows, one row per lane.  Lane 0 first forms alpha
//   sl_actor_rows_kernel<C>   into LDS; after one barrier every lane loads its row, evaluates the expressions of the header and stores its
//                             per-row outputs.  The block then forms its float64 sums by fr_block_sums; lanes past the end contribute
//                             +0.0.  The sums go to part[block][ns]: ns = 2 C + 1 (critic) or 4 (actor).
//   sl_merge_kernel           ONE wave, both losses: lane q < ns adds column q of the block sums by fr_sum_column; lane 0 then writes
//                             stats[8], the float32 losses and d_log_ent_coef.
// The order of every float64 sum is that of dn_row_sums.h, a function of (batch, act_dim, n_critics) alone: the same call gives the same
// bits every time, and a captured graph replays it.
#include "dn_internal.h"
#include "dn_row_sums.h"
#include "dn_sac_math.h"

namespace {

constexpr int SP_THREADS = 256;                          // the policy head: one row per lane, 4 waves
constexpr int SL_THREADS = (int)DN_ROWNORM_BLOCK_ROWS;   // the losses: one row per lane, 16 waves
constexpr int SL_WAVES = SL_THREADS / 64;
constexpr int SL_MAX_SUMS = 2 * DN_SAC_MAX_CRITICS + 1;

template <int A, bool BWD>
__global__ __launch_bounds__(SP_THREADS) void sl_policy_kernel(const DnSacPolicyArgs a)
{
    const long long row = (long long)blockIdx.x * SP_THREADS + (long long)threadIdx.x;
    if (row >= a.batch) return;
    const bool vec = a.vec != 0;
    float mu[A], raw[A], eps[A];
    dn_load_row<A>(a.mean, row, vec, mu);
    dn_load_row<A>(a.raw, row, vec, raw);
    dn_load_row<A>(a.eps, row, vec, eps);
    if constexpr (!BWD) {
        float act[A];
        double lp = 0.0;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const DnSacElem e = dn_sac_elem((double)mu[j], (double)raw[j], (double)eps[j], a.lo, a.hi);
            act[j] = (float)e.a;
            lp = j == 0 ? e.term : lp + e.term;
        }
        dn_store_row<A>(a.actions, row, vec, act);
        a.log_prob[row] = (float)lp;
    } else {
        float ga[A], dm[A], dr[A];
        if (a.g_a) {
            dn_load_row<A>(a.g_a, row, vec, ga);
        } else {
#pragma unroll
            for (int j = 0; j < A; ++j) ga[j] = 0.0f;
        }
        const double glp = a.g_lp ? (double)a.g_lp[row] : 0.0;
#pragma unroll
        for (int j = 0; j < A; ++j) {
            const double r = (double)raw[j], ep = (double)eps[j];
            const DnSacElem e = dn_sac_elem((double)mu[j], r, ep, a.lo, a.hi);
            double d_mean, d_raw;
            dn_sac_elem_backward(e, r, ep, a.lo, a.hi, (double)ga[j], glp, d_mean, d_raw);
            dm[j] = (float)d_mean;
            dr[j] = (float)d_raw;
        }
        dn_store_row<A>(a.d_mean, row, vec, dm);
        dn_store_row<A>(a.d_raw, row, vec, dr);
    }
}

__device__ __forceinline__ double sl_alpha(const DnSacLossArgs &a)
{
    return a.log_ent_coef ? dn_sac_alpha((double)a.log_ent_coef[0]) : a.ent_coef;
}

template <int C>
__global__ __launch_bounds__(SL_THREADS) void sl_critic_rows_kernel(const DnSacLossArgs a)
{
    constexpr int NS = 2 * C + 1;
    __shared__ double alpha_s;
    __shared__ double wsum[SL_WAVES][NS];

    const int tid = (int)threadIdx.x;
    const long long row0 = (long long)blockIdx.x * SL_THREADS, left = a.batch - row0;                  // left >= 1
    const int nrows = left < SL_THREADS ? (int)left : SL_THREADS;
    const double nb = (double)a.batch;

    if (tid == 0) alpha_s = sl_alpha(a);
    __syncthreads();

    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;

    if (tid < nrows) {
        const long long row = row0 + tid;
        double nq = (double)a.next_q[0][row];
        int pick = 0;
#pragma unroll
        for (int c = 1; c < C; ++c) dn_sac_min_step(nq, pick, (double)a.next_q[c][row], c);
        const double y = dn_sac_target((double)a.rewards[row], (double)a.dones[row], a.gamma, nq, alpha_s, (double)a.next_log_prob[row]);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double q = (double)a.q[c][row], e = q - y;
            a.d_q[c][row] = (float)(e / nb);
            s[c] = e * e;
            s[C + 1 + c] = q;
        }
        s[C] = y;
        a.target_q[row] = (float)y;
    }
    fr_block_sums<NS, SL_WAVES>(s, wsum, a.part);
}

template <int C>
__global__ __launch_bounds__(SL_THREADS) void sl_actor_rows_kernel(const DnSacLossArgs a)
{
    constexpr int NS = 4;
    __shared__ double alpha_s;
    __shared__ double wsum[SL_WAVES][NS];

    const int tid = (int)threadIdx.x;
    const long long row0 = (long long)blockIdx.x * SL_THREADS, left = a.batch - row0;                  // left >= 1
    const int nrows = left < SL_THREADS ? (int)left : SL_THREADS;
    const double nb = (double)a.batch;

    if (tid == 0) alpha_s = sl_alpha(a);
    __syncthreads();

    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;

    if (tid < nrows) {
        const long long row = row0 + tid;
        const double alpha = alpha_s, lp = (double)a.log_prob[row];
        double qmin = (double)a.q[0][row];
        int pick = 0;
#pragma unroll
        for (int c = 1; c < C; ++c) dn_sac_min_step(qmin, pick, (double)a.q[c][row], c);
        const float g = (float)(-1.0 / nb);
#pragma unroll
        for (int c = 0; c < C; ++c) a.d_q[c][row] = c == pick ? g : 0.0f;
        a.d_log_prob[row] = (float)(alpha / nb);
        s[0] = alpha * lp - qmin;
        s[1] = lp + a.target_entropy;
        s[2] = lp;
        s[3] = qmin;
    }
    fr_block_sums<NS, SL_WAVES>(s, wsum, a.part);
}

__global__ __launch_bounds__(64) void sl_merge_kernel(const DnSacLossArgs a)
{
    __shared__ double tot[SL_MAX_SUMS];
    const int q = (int)threadIdx.x, C = a.n_critics, ns = a.mode == DN_SAC_CRITIC ? 2 * C + 1 : 4;
    const long long nblk = a.nblk;
    if (q < ns) tot[q] = fr_sum_column(a.part + q, ns, nblk);
    __syncthreads();
    if (q != 0) return;
    const double nb = (double)a.batch, alpha = sl_alpha(a);
    if (a.mode == DN_SAC_CRITIC) {
        double sum = 0.0;
        for (int c = 0; c < C; ++c) {
            const double m = tot[c] / nb;
            sum = c == 0 ? m : sum + m;
        }
        const double loss = 0.5 * sum;
        a.stats[0] = loss;                             // critic_loss
        a.stats[1] = alpha;                            // ent_coef
        a.stats[2] = tot[C] / nb;                      // the mean target
        for (int c = 0; c < DN_SAC_MAX_CRITICS; ++c) a.stats[3 + c] = c < C ? tot[C + 1 + c] / nb : 0.0;       // the mean of q_c
        a.stats[7] = 0.0;
        a.loss[0] = (float)loss;
    } else {
        const double loss = tot[0] / nb;
        double ecl = 0.0, dlec = 0.0;
        if (a.log_ent_coef) {
            const double m = tot[1] / nb;
            ecl = -((double)a.log_ent_coef[0] * m);
            dlec = -m;
            a.d_log_ent_coef[0] = (float)dlec;
        }
        a.stats[0] = loss;                             // actor_loss
        a.stats[1] = ecl;                              // ent_coef_loss
        a.stats[2] = alpha;                            // ent_coef
        a.stats[3] = tot[2] / nb;                      // the mean log-probability
        a.stats[4] = tot[3] / nb;                      // the mean of min_c q_pi_c
        a.stats[5] = dlec;                             // d ent_coef_loss / d log_ent_coef
        a.stats[6] = 0.0;
        a.stats[7] = 0.0;
        a.loss[0] = (float)loss;
        a.ent_coef_loss[0] = (float)ecl;
    }
}

template <int A>
void sl_launch_policy(const DnSacPolicyArgs &a, bool backward, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.batch + SP_THREADS - 1) / SP_THREADS));
    if (backward) hipLaunchKernelGGL((sl_policy_kernel<A, true>), grid, dim3(SP_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((sl_policy_kernel<A, false>), grid, dim3(SP_THREADS), 0, stream, a);
}

template <int C>
void sl_launch_rows(const DnSacLossArgs &a, hipStream_t stream)
{
    if (a.mode == DN_SAC_CRITIC) hipLaunchKernelGGL(sl_critic_rows_kernel<C>, dim3((unsigned)a.nblk), dim3(SL_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(sl_actor_rows_kernel<C>, dim3((unsigned)a.nblk), dim3(SL_THREADS), 0, stream, a);
}

}  // namespace

hipError_t dn_launch_sac_policy(const DnSacPolicyArgs &a, bool backward, hipStream_t stream)
{
    if (a.batch < 1 || a.batch > 0x7fffffffll || a.act_dim < 1 || a.act_dim > DN_SAC_MAX_ACT) return hipErrorInvalidValue;
    switch (a.act_dim) {
    case 1: sl_launch_policy<1>(a, backward, stream); break;
    case 2: sl_launch_policy<2>(a, backward, stream); break;
    case 3: sl_launch_policy<3>(a, backward, stream); break;
    case 4: sl_launch_policy<4>(a, backward, stream); break;
    case 5: sl_launch_policy<5>(a, backward, stream); break;
    case 6: sl_launch_policy<6>(a, backward, stream); break;
    case 7: sl_launch_policy<7>(a, backward, stream); break;
    default: sl_launch_policy<8>(a, backward, stream); break;
    }
    return hipGetLastError();
}

hipError_t dn_launch_sac_loss(const DnSacLossArgs &a, hipStream_t stream)
{
    if (dn_sac_loss_scratch_doubles(a.batch, a.n_critics) == 0 || a.nblk != dn_rownorm_blocks(a.batch)) return hipErrorInvalidValue;
    if (a.mode != DN_SAC_CRITIC && a.mode != DN_SAC_ACTOR) return hipErrorInvalidValue;
    switch (a.n_critics) {
    case 1: sl_launch_rows<1>(a, stream); break;
    case 2: sl_launch_rows<2>(a, stream); break;
    case 3: sl_launch_rows<3>(a, stream); break;
    default: sl_launch_rows<4>(a, stream); break;
    }
    hipLaunchKernelGGL(sl_merge_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}
