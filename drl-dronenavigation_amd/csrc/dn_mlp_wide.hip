// dn_mlp_wide.hip -- the PPO policy / value network for input rows of 17 .. 64 columns (dn_mlp_forward, obs_dim > 16).
//
// The kernels of dn_mlp.hip form layer 1 as ONE MFMA K-step of 16 inputs: enough for the 13-column observation, not for what the
// goal rows (cat(obs, goal): 21 columns) and the privileged rows (52 columns) give a network to read.  Here layer 1 runs
// KS1 = 2 (obs_dim <= 32) or 4 (obs_dim <= 64) K-steps; input k of a drone sits in K-step k >> 4, lane group (k >> 3) & 1, slot k & 7
// -- the layout of load_obs8, once per K-step -- and w1 is packed to match (policy_mfma._k_order(first=True)): per M-tile the KS1
// fragments in K-step order, in the float32 grade the KS1 hi fragments and then the KS1 lo fragments.
//
// Everything after layer 1 is dn_mlp.hip's code, called as it stands (layer_lds_c / layer_x3, the LDS chunk buffers, the staged biases,
// the head, the masked forward, the ragged tail); this unit includes dn_mlp.hip for those device functions (DN_MLP_NO_LAUNCHER, as
// dn_fused.hip does) and adds kernels of its own beside dn_mlp_lds_kernel<F16> and dn_mlp_x3_kernel<NoTail>, so that the tuned
// kernels' code does not move (profiles/mlp_wide_device_code_diff.txt).
//
// Layer 1's fragments come straight from L2, one global_load_dwordx4 per lane and fragment through a register ring, as dn_mlp_kernel reads
// all its layers -- for KS1 = 2 and KS1 = 4 alike.  The LDS path has no room for KS1 = 4 (64 fragments, 128 in hi / lo form, against a
// buffer 0 of CHUNK = 32 / CH3 = 64 with layer 2's chunk 0 already in flight into buffer 1), and one code path is less than two: layer 1
// is 16 KS1 of ~800 MFMAs per tile and network.  These loads share the vector-memory counter with the LDS-DMA pieces of layer 2's chunk 0,
// which the compiler does not see: a wait for a fragment requested after the pieces is computed without them and, loads returning in order,
// also waits for the pieces -- correct, and not free: in the generated code the refills are waited from about M-tile 4 on with counts that
// drain this wave's 8 pieces in the middle of layer 1 instead of at its end.  What the whole of it costs is measured, not argued:
// profiles/time_mlp_wide.txt holds the launch times beside the MFMA-count ratios they should track.
#define DN_MLP_NO_LAUNCHER
#include "dn_mlp.hip"

namespace {

constexpr int WIDE_RING = 16;                               // layer-1 fragments in flight per wave (16 B per lane each)

// This lane's layer-1 inputs of K-step kk: k = 16 kk + 8 g .. + 7 of drone `row`, zero at and beyond obs_dim.  load_obs8's rule: every
// load at a clamped index (never past the row's last float), selected afterwards.
MLP_DEV void load_obs8_at(const MlpArgs &a, const long long row, const int kk, const int g, float (&v)[8])
{
    const float *o = a.obs + row * a.obs_dim;
    const int last = a.obs_dim - 1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * kk + 8 * g + j;
        const float x = o[k < last ? k : last];
        v[j] = k <= last ? x : 0.0f;
    }
}

// grid = (workgroups of 128 drones, networks): dn_mlp_lds_kernel<F16> with KS1 K-steps in layer 1
template <bool F16, int KS1>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(1, 1))) void dn_mlp_wide_lds_kernel(const MlpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint4 lds[NBUF * CHUNK * 64 + (NBIAS + 3) / 4 + 1];     // ONE __shared__ object (see dn_mlp_lds_kernel)
    float *lbias = reinterpret_cast<float *>(lds + NBUF * CHUNK * 64);
    int *s_any = reinterpret_cast<int *>(lds + NBUF * CHUNK * 64 + (NBIAS + 3) / 4);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 5, col = lane & 31;
    const MlpNetDev &net = a.net[blockIdx.y];
    const long long row0 = ((long long)blockIdx.x * WAVES + wave) * TILE;
    const bool live = row0 + col < a.n;
    const long long row = live ? row0 + col : a.n - 1;      // ragged tail: shadow the last drone, never store
    bool tile_wanted = true;
    if (a.row_mask) {                                       // masked forward: as dn_mlp_lds_kernel
        const bool wanted = live && a.row_mask[row0 + col] != 0;
        tile_wanted = __ballot(wanted) != 0ull;
        if (lane == 0) s_any[wave] = tile_wanted;
        __syncthreads();
        if ((s_any[0] | s_any[1] | s_any[2] | s_any[3]) == 0) {
            if (g == 0 && live)
                for (int j = 0; j < net.out_dim; ++j) net.out[(row0 + col) * net.out_dim + j] = 0.0f;
            return;
        }
    }
    for (int i = threadIdx.x; i < NBIAS; i += 64 * WAVES)
        lbias[i] = i < H1 ? net.b1[i] : i < H1 + H2 ? net.b2[i - H1] : i < H1 + H2 + H3 ? net.b3[i - H1 - H2] : net.bh[i - H1 - H2 - H3];
    u32x4 x0[KS1];
#pragma unroll
    for (int kk = 0; kk < KS1; ++kk) {
        float ob[8];
        load_obs8_at(a, row, kk, g, ob);
#pragma unroll
        for (int q = 0; q < 4; ++q) x0[kk][q] = pack2t<F16>(ob[2 * q], ob[2 * q + 1]);
    }
    // layer 1's stream of (H1 / 32) KS1 fragments, from L2: the ring's first fill goes out before layer 2's DMA pieces
    constexpr int T = (H1 / 32) * KS1, P = WIDE_RING < T ? WIDE_RING : T;
    static_assert(P % KS1 == 0, "an M-tile's fragments occupy whole ring slots");
    const uint4 *wl = net.w1 + lane;
    uint4 ring[P];
#pragma unroll
    for (int t = 0; t < P; ++t) ring[t] = wl[t * 64];
    chunk_barrier();                                        // the biases are staged
    // LDS buffers as in dn_mlp_lds_kernel, buffer 0 unused by layer 1: layer 2's chunks start in buffer 1, layer 3's at 2, the head at 1
    constexpr int B2 = 1, B3 = (B2 + H2 / 32) % NBUF, BH = (B3 + H3 / 32) % NBUF;
    u32x4 h1[H1 / 16];
    dma_chunk(net.w2, lds + B2 * CHUNK * 64, CHUNK, wave, lane);             // layer 2, chunk 0 -> buffer 1
#pragma unroll
    for (int m = 0; m < H1 / 32; ++m) {
        f32x16 acc;
        bias_init(lbias, m, g, acc);
#pragma unroll
        for (int kk = 0; kk < KS1; ++kk) {
            const int t = m * KS1 + kk;
            const uint4 w = ring[t % P];
            if (t + P < T) ring[t % P] = wl[(t + P) * 64];
            acc = mfma16<F16>(w, x0[kk], acc);
        }
        MLP_PIN();
        epilogue_t<F16>(acc, h1[2 * m], h1[2 * m + 1]);
    }
    chunk_barrier();
    u32x4 h2[H2 / 16];
    layer_lds_c<F16, H2 / 32, B2, CHUNK>(net.w2, lbias + H1, net.w3, h1, h2, lds, wave, lane);
    u32x4 h3[H3 / 16];
    layer_lds_c<F16, H3 / 32, B3, H3 / 16>(net.w3, lbias + H1 + H2, net.wh, h2, h3, lds, wave, lane);
    // head: one M-tile of H3/16 = 16 fragments; float32 result straight from the accumulator
    f32x16 acc;
    bias_init(lbias + H1 + H2 + H3, 0, g, acc);
    const uint4 *cur = lds + BH * (CHUNK * 64);
#pragma unroll
    for (int kk = 0; kk < H3 / 16; ++kk) {
        const uint4 w = cur[kk * 64 + lane];
        acc = mfma16<F16>(w, h3[kk], acc);
    }
    if (live) {
        float *o = net.out + (row0 + col) * net.out_dim;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = acc_row(0, g, r);
            if (j < net.out_dim) o[j] = tile_wanted ? acc[r] : 0.0f;
        }
    }
}

// mlp_x3_body with KS1 K-steps in layer 1: this half computes its own 8 M-tiles outright, each from KS1 hi and KS1 lo fragments (mfma3 per
// K-step: the order of the three partial products is the 16-column kernel's).  The half's fragments are one contiguous stream of w1.
template <int HALF, int KS1>
MLP_DEV void mlp_wide_x3_body(const MlpArgs &a, const MlpNetDev &net, uint4 *wbuf, float4 *xb, const float *lbias, const int wave,
                              const int lane, const long long row0, const bool live, const long long row, const bool tile_wanted STP_PARAM)
{
    const int g = lane >> 5, col = lane & 31;
    u32x4 x0h[KS1], x0l[KS1];
#pragma unroll
    for (int kk = 0; kk < KS1; ++kk) {
        float ob[8];
        load_obs8_at(a, row, kk, g, ob);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned h, l;
            split2(ob[2 * q], ob[2 * q + 1], h, l);
            x0h[kk][q] = h; x0l[kk][q] = l;
        }
    }
    constexpr int PER = 2 * KS1;                            // fragments per M-tile: KS1 hi, KS1 lo
    constexpr int T = 8 * PER, P = WIDE_RING < T ? WIDE_RING : T;
    static_assert(P % PER == 0, "an M-tile's fragments occupy whole ring slots");
    const uint4 *wl = net.w1 + (size_t)(HALF * 8) * PER * 64 + lane;
    uint4 ring[P];
#pragma unroll
    for (int t = 0; t < P; ++t) ring[t] = wl[t * 64];
    u32x4 h1h[16], h1l[16];
    dma_x3<CH3>(net.w2, wbuf + CH3 * 64, wave, lane);                        // layer 2, chunk 0 -> buffer 1
#pragma unroll
    for (int ml = 0; ml < 8; ++ml) {
        const int m = HALF * 8 + ml;
        f32x16 acc;
        bias_init(lbias, m, g, acc);
        uint4 wh[KS1], wlo[KS1];
#pragma unroll
        for (int kk = 0; kk < KS1; ++kk) {
            wh[kk] = ring[(ml * PER + kk) % P];
            wlo[kk] = ring[(ml * PER + KS1 + kk) % P];
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int t = ml * PER + i;
            if (t + P < T) ring[t % P] = wl[(t + P) * 64];
        }
#pragma unroll
        for (int kk = 0; kk < KS1; ++kk) acc = mfma3(wh[kk], wlo[kk], x0h[kk], x0l[kk], acc);
        MLP_PIN();
        epilogue3(acc, h1h[2 * ml], h1h[2 * ml + 1], h1l[2 * ml], h1l[2 * ml + 1]);
    }
    CHUNK_BARRIER();
    u32x4 h2h[16], h2l[16];
    layer_x3<HALF, H2 / 32, 1, CH3>(net.w2, lbias + H1, net.w3, h1h, h1l, h2h, h2l, wbuf, xb, wave, lane STP_ARG);
    u32x4 h3h[8], h3l[8];
    layer_x3<HALF, H3 / 32, 1, 2 * (H3 / 16)>(net.w3, lbias + H1 + H2, net.wh, h2h, h2l, h3h, h3l, wbuf, xb, wave, lane STP_ARG);
    // head: one tile, K = 256 = 16 K-steps, 8 per half; chunk in buffer 1 as [16 hi][16 lo]
    f32x16 acc;
    if (HALF == 0) bias_init(lbias + H1 + H2 + H3, 0, g, acc);
    else {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    }
    const uint4 *cur = wbuf + CH3 * 64;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const uint4 wh = cur[(HALF * 8 + kk) * 64 + lane], wl2 = cur[(H3 / 16 + HALF * 8 + kk) * 64 + lane];
        acc = mfma3(wh, wl2, h3h[kk], h3l[kk], acc);
    }
    if (HALF == 1) park_partial(xb, 0, lane, acc);
    CHUNK_BARRIER();
    if (HALF == 0) {
        merge_partial(xb, 0, lane, acc);
        if (live) {
            float *o = net.out + (row0 + col) * net.out_dim;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = acc_row(0, g, r);
                if (j < net.out_dim) o[j] = tile_wanted ? acc[r] : 0.0f;
            }
        }
    }
}

// grid = (workgroups of 64 drones, networks): dn_mlp_x3_kernel<NoTail> with KS1 K-steps in layer 1
template <int KS1>
__global__ __launch_bounds__(64 * XWAVES) __attribute__((amdgpu_waves_per_eu(1, 1))) void dn_mlp_wide_x3_kernel(const MlpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint4 lds[LDS_X3_U4];           // ONE __shared__ object (see dn_mlp_lds_kernel)
    uint4 *wbuf = lds;
    float *lbias = reinterpret_cast<float *>(lds + 2 * CH3 * 64 + XB3_U4);
    int *s_any = reinterpret_cast<int *>(lds + LDS_X3_U4 - 1);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = wave & 1, half = wave >> 1;                              // waves p and p + 2 share a tile, on two SIMDs
    float4 *xb = reinterpret_cast<float4 *>(lds + 2 * CH3 * 64) + pair * (2 * 4 * 64);
    const int col = lane & 31;
    const MlpNetDev &net = a.net[blockIdx.y];
    const long long row0 = ((long long)blockIdx.x * 2 + pair) * TILE;
    const bool live = row0 + col < a.n;
    const long long row = live ? row0 + col : a.n - 1;
    bool tile_wanted = true;
    if (a.row_mask) {
        const bool wanted = live && a.row_mask[row0 + col] != 0;
        tile_wanted = __ballot(wanted) != 0ull;
        if (lane == 0 && half == 0) s_any[pair] = tile_wanted;
        __syncthreads();
        if ((s_any[0] | s_any[1]) == 0) {
            if (half == 0 && (lane >> 5) == 0 && live)
                for (int j = 0; j < net.out_dim; ++j) net.out[(row0 + col) * net.out_dim + j] = 0.0f;
            return;
        }
    }
    // biases -> LDS (once); buffer 0 stays empty: layer 1 reads its fragments from L2
    for (int i = threadIdx.x; i < NBIAS; i += 64 * XWAVES)
        lbias[i] = i < H1 ? net.b1[i] : i < H1 + H2 ? net.b2[i - H1] : i < H1 + H2 + H3 ? net.b3[i - H1 - H2] : net.bh[i - H1 - H2 - H3];
#ifdef DN_MLP_STAMP
    Stamp stp{0, wave, blockIdx.x == 0 && blockIdx.y == 0 && lane == 0};
#endif
    CHUNK_BARRIER();
    if (half == 0) mlp_wide_x3_body<0, KS1>(a, net, wbuf, xb, lbias, wave, lane, row0, live, row, tile_wanted STP_ARG);
    else mlp_wide_x3_body<1, KS1>(a, net, wbuf, xb, lbias, wave, lane, row0, live, row, tile_wanted STP_ARG);
}

}  // namespace

// dn_launch_mlp's branch for PPO networks with 16 < obs_dim <= 64 (dn_mlp_ks1(obs_dim) = 2 or 4), whatever DN_MLP_SHAPE says
hipError_t dn_launch_mlp_wide(const dn_mlp_net *nets, int num_nets, const float *obs, const uint8_t *row_mask, long long n, int obs_dim,
                              hipStream_t stream)
{
    const int ks1 = dn_mlp_ks1(obs_dim);
    if (nets[0].arch != DN_MLP_ARCH_PPO || (ks1 != 2 && ks1 != 4)) return hipErrorInvalidValue;
    MlpArgs a;
    for (int k = 0; k < 2; ++k) {
        const dn_mlp_net &s = nets[k < num_nets ? k : 0];
        a.net[k].w1 = (const uint4 *)s.w1; a.net[k].w2 = (const uint4 *)s.w2; a.net[k].w3 = (const uint4 *)s.w3;
        a.net[k].wh = (const uint4 *)s.wh;
        a.net[k].b1 = s.b1; a.net[k].b2 = s.b2; a.net[k].b3 = s.b3; a.net[k].bh = s.bh;
        a.net[k].out = s.out; a.net[k].out_dim = s.out_dim;
    }
    a.obs = obs; a.row_mask = row_mask; a.n = n; a.obs_dim = obs_dim;
    const unsigned tiles = (unsigned)((n + TILE - 1) / TILE);
    if (nets[0].grade == 1) {
        const dim3 grid((tiles + 1) / 2, num_nets), blk(64 * XWAVES);
        if (ks1 == 2) hipLaunchKernelGGL(dn_mlp_wide_x3_kernel<2>, grid, blk, 0, stream, a);
        else hipLaunchKernelGGL(dn_mlp_wide_x3_kernel<4>, grid, blk, 0, stream, a);
        return hipGetLastError();
    }
    const dim3 grid((tiles + WAVES - 1) / WAVES, num_nets), blk(64 * WAVES);
    if (nets[0].grade == 2) {
        if (ks1 == 2) hipLaunchKernelGGL((dn_mlp_wide_lds_kernel<true, 2>), grid, blk, 0, stream, a);
        else hipLaunchKernelGGL((dn_mlp_wide_lds_kernel<true, 4>), grid, blk, 0, stream, a);
    } else {
        if (ks1 == 2) hipLaunchKernelGGL((dn_mlp_wide_lds_kernel<false, 2>), grid, blk, 0, stream, a);
        else hipLaunchKernelGGL((dn_mlp_wide_lds_kernel<false, 4>), grid, blk, 0, stream, a);
    }
    return hipGetLastError();
}
