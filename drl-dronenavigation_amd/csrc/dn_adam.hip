// dn_adam.hip -- the PPO optimiser step on the device for gfx950 (dn_adam_step, include/dronenav.h).
//
// What SB3's PPO.train [from recall] puts between loss.backward() and the next minibatch: clip_grad_norm_(parameters, max_grad_norm) and
// torch.optim.Adam(eps=1e-5).step(), over up to DN_ADAM_MAX_TENSORS small tensors -- in float64, every input widened once, every output
// rounded once, true division and square root.  The header states the arithmetic line by line.
//
// Each tensor is cut into chunks of DN_ADAM_CHUNK consecutive elements (the last chunk of a tensor is short, so no chunk straddles two
// tensors), numbered tensor by tensor; a chunk is one workgroup of AD_THREADS lanes, AD_PER_LANE consecutive elements per lane.  The tensor
// table is a kernel argument; a workgroup finds its tensor by a uniform walk over the chunk prefix.  A tensor whose four pointers are
// 16-byte aligned moves as 16-byte words (a chunk starts a multiple of 4096 bytes into its tensor), any other as 4-byte words; both fill
// the same registers, so the bits are the same.  Lanes past the end load +0.0 and store nothing.
//
// Two ordinary launches on the caller's stream; no workgroup ever waits for another, nothing is allocated, no atomics:
//   1. ad_partials_kernel   each chunk forms its float64 sum of g * g -- a lane adds its four elements in ascending order, the lanes of a
//                           wave by the fixed tree of dn_fleet_rms.h, the waves in ascending order through LDS -- into part[chunk].  Lane
//                           0 of workgroup 0 also reads `state` and writes the advanced state; no other workgroup of this launch
//                           touches it, and launch 2 only reads it.
//   2. ad_update_kernel     every workgroup forms the total itself from the chunk sums, in an order that depends on the chunk count alone
//                           (lane l of wave 0 adds sums l, l + 64, ... ascending, then the same tree, then a broadcast through LDS), and
//                           applies the update to its chunk; workgroup 0 writes `stats`.
// The order of every float64 operation is a function of the tensor counts alone: the same call gives the same bits every time, and a
// captured graph replays it.
#include "dn_internal.h"
#include "dn_fleet_rms.h"

namespace {

constexpr int AD_PER_LANE = 4;                         // one 16-byte word
constexpr int AD_THREADS = DN_ADAM_CHUNK / AD_PER_LANE;
constexpr int AD_WAVES = AD_THREADS / 64;
static_assert(DN_ADAM_CHUNK % (64 * AD_PER_LANE) == 0 && AD_THREADS <= 1024, "a chunk is whole waves of four elements per lane");
static_assert(sizeof(dn_adam_tensor) == 40, "dn_adam_tensor: four pointers and a count");

// The chunk of this workgroup: its tensor (a uniform walk over the chunk prefix), the first element of the chunk in it, and whether the
// tensor moves as 16-byte words.
struct AdChunk {
    float *p, *g, *m, *v;
    long long e0, count;
    bool wide;
};

__device__ __forceinline__ AdChunk ad_find_chunk(const DnAdamArgs &a)
{
    long long b = (long long)blockIdx.x;
    int t = 0;
    for (; t < a.n_tensors - 1; ++t) {
        const long long nch = (a.t[t].count - 1) / DN_ADAM_CHUNK + 1;             // dn_adam_chunks of a count >= 1
        if (b < nch) break;
        b -= nch;
    }
    AdChunk c;
    c.p = a.t[t].param; c.g = a.t[t].grad; c.m = a.t[t].exp_avg; c.v = a.t[t].exp_avg_sq;
    c.count = a.t[t].count;
    c.e0 = b * DN_ADAM_CHUNK;
    c.wide = (((uintptr_t)c.p | (uintptr_t)c.g | (uintptr_t)c.m | (uintptr_t)c.v) & 15u) == 0;
    return c;
}

// The lane's AD_PER_LANE consecutive elements from element e on, of a tensor of `count`: one 16-byte word when the tensor is wide and the
// word lies inside it, else 4-byte words; elements past the end are +0.0.
__device__ __forceinline__ void ad_load(const float *__restrict__ q, const long long e, const long long count, const bool wide,
                                        float (&x)[AD_PER_LANE])
{
    if (wide && e + AD_PER_LANE <= count) {
        const float4 w = *reinterpret_cast<const float4 *>(q + e);
        x[0] = w.x; x[1] = w.y; x[2] = w.z; x[3] = w.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < AD_PER_LANE; ++j) x[j] = e + j < count ? q[e + j] : 0.0f;
}

__device__ __forceinline__ void ad_store(float *__restrict__ q, const long long e, const long long count, const bool wide,
                                         const float (&x)[AD_PER_LANE])
{
    if (wide && e + AD_PER_LANE <= count) {
        *reinterpret_cast<float4 *>(q + e) = make_float4(x[0], x[1], x[2], x[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < AD_PER_LANE; ++j)
        if (e + j < count) q[e + j] = x[j];
}

__global__ __launch_bounds__(AD_THREADS) void ad_partials_kernel(const DnAdamArgs a)
{
    __shared__ double wsum[AD_WAVES];
    const int tid = (int)threadIdx.x;
    const AdChunk c = ad_find_chunk(a);

    float g[AD_PER_LANE];
    ad_load(c.g, c.e0 + (long long)tid * AD_PER_LANE, c.count, c.wide, g);
    double s = (double)g[0] * (double)g[0];
#pragma unroll
    for (int j = 1; j < AD_PER_LANE; ++j) s += (double)g[j] * (double)g[j];

    const double t = fr_wave_sum(s);
    if ((tid & 63) == 0) wsum[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
        double sum = wsum[0];
#pragma unroll
        for (int wv = 1; wv < AD_WAVES; ++wv) sum += wsum[wv];
        a.part[blockIdx.x] = sum;
        if (blockIdx.x == 0) {                         // the state's advance: running products take the place of beta ** step
            const double step = a.state[0], c1 = a.state[1], c2 = a.state[2];
            a.state[0] = step + 1.0;
            a.state[1] = c1 * a.beta1;
            a.state[2] = c2 * a.beta2;
            a.state[3] = 0.0;
        }
    }
}

__global__ __launch_bounds__(AD_THREADS) void ad_update_kernel(const DnAdamArgs a)
{
    __shared__ double total_s;
    const int tid = (int)threadIdx.x;
    const AdChunk c = ad_find_chunk(a);
    const long long e = c.e0 + (long long)tid * AD_PER_LANE;

    float p[AD_PER_LANE], g[AD_PER_LANE], m[AD_PER_LANE], v[AD_PER_LANE];
    ad_load(c.g, e, c.count, c.wide, g);               // the chunk is on its way while wave 0 adds the chunk sums
    ad_load(c.p, e, c.count, c.wide, p);
    ad_load(c.m, e, c.count, c.wide, m);
    ad_load(c.v, e, c.count, c.wide, v);

    if (tid < 64) {
        double s = 0.0;
        for (long long i0 = tid; i0 < a.nchunks; i0 += 64 * FR_BATCH) {    // FR_BATCH loads in flight ahead of the chain of additions
            double x[FR_BATCH];
#pragma unroll
            for (int j = 0; j < FR_BATCH; ++j) x[j] = i0 + 64 * j < a.nchunks ? a.part[i0 + 64 * j] : 0.0;
#pragma unroll
            for (int j = 0; j < FR_BATCH; ++j)
                if (i0 + 64 * j < a.nchunks) s += x[j];
        }
        s = fr_wave_sum(s);
        if (tid == 0) total_s = s;
    }
    __syncthreads();

    const double total = sqrt(total_s);
    const double cl = a.max_grad_norm / (total + 1e-6);
    const double coef = a.max_grad_norm > 0.0 ? (cl > 1.0 ? 1.0 : cl) : 1.0;                          // a NaN stays a NaN
    const double lr = a.lr[0], step = a.state[0], bc1 = 1.0 - a.state[1], bc2 = 1.0 - a.state[2];      // the advanced state of launch 1
    const double step_size = lr / bc1, sqrt_bc2 = sqrt(bc2);
    const double w1 = 1.0 - a.beta1, w2 = 1.0 - a.beta2;

    if (a.flags & DN_ADAM_ZERO_GRADS) {
        const float zero[AD_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f};
        ad_store(c.g, e, c.count, c.wide, zero);
    }
#pragma unroll
    for (int j = 0; j < AD_PER_LANE; ++j) {
        const double gs = (double)g[j] * coef;
        const double m1 = (double)m[j] + (gs - (double)m[j]) * w1;
        const double v1 = (double)v[j] * a.beta2 + w2 * gs * gs;
        const double denom = sqrt(v1) / sqrt_bc2 + a.eps;
        p[j] = (float)((double)p[j] - step_size * (m1 / denom));
        m[j] = (float)m1;
        v[j] = (float)v1;
    }
    ad_store(c.p, e, c.count, c.wide, p);
    ad_store(c.m, e, c.count, c.wide, m);
    ad_store(c.v, e, c.count, c.wide, v);

    if (blockIdx.x == 0 && tid == 0) {
        a.stats[0] = total;
        a.stats[1] = coef;
        a.stats[2] = lr;
        a.stats[3] = step;
    }
}

}  // namespace

hipError_t dn_launch_adam(const DnAdamArgs &a, hipStream_t stream)
{
    if (a.n_tensors < 1 || a.n_tensors > DN_ADAM_MAX_TENSORS || a.nchunks < 1 || a.nchunks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ad_partials_kernel, dim3((unsigned)a.nchunks), dim3(AD_THREADS), 0, stream, a);
    hipLaunchKernelGGL(ad_update_kernel, dim3((unsigned)a.nchunks), dim3(AD_THREADS), 0, stream, a);
    return hipGetLastError();
}
