// dn_sac_train.hip -- the training pass of the SAC networks for gfx950 (dn_sac_train_forward / dn_sac_train_backward) and the Polyak
// update of the target critics (dn_polyak_update), include/dronenav.h.
//
// The product is csrc/dn_mt_gemm.h, the one dn_mlp_train.hip runs: same staging, split, MFMA chain and tile shapes, so a network that
// both families can express gets the same bits from both.  What this unit adds is addressing and the ReLU epilogues:
//   an operand made of blocks (MtOp): up to four dense matrices side by side by columns -- x = (x0 | x1), the head gradient
//     (d_out part 0 | d_out part 1), [dZ0_0 | dZ0_1 | ...] of the networks of a group -- or stacked by rows -- the head's weight
//     (W part 0 over W part 1), the W0_c of a group.  A four-wide load inside one block is the plain one; one that straddles two blocks
//     gathers its elements one by one.  The order of a product's k does not know where the blocks end.
//   an output of up to two column blocks (the head's parts, d_x0 | d_x1); a block whose pointer is NULL is not stored.
//   grid y = network x column tile: the networks of a group advance in the same launches.  Grid z of the weight gradient is the chunk.
//   d_x = sum over the networks of dZ0_c W0_c as ONE product whose K runs over the networks in ascending order.
// No atomics, no workgroup waits for another, plain launches: capturable.
#include "dn_mt_gemm.h"
#include "dn_sac_math.h"

#include <climits>

namespace {

struct MtOp {
    const float *p[4];
    int ld[4];
    int end[4];                                        // block b holds [end[b - 1], end[b]) of the split axis; INT_MAX from the last block on
    int by_rows;                                       // the blocks are stacked by rows (one ld); else side by side by columns

    // The block that holds position `at` of the split axis: its matrix, stride, first position and end.  Selects, not indexed reads: the
    // table stays in scalar registers whatever the lanes ask for.
    struct Block {
        const float *p;
        int ld, first, end;
        __device__ __forceinline__ bool vec() const { return (ld & 3) == 0 && ((uintptr_t)p & 15u) == 0; }
    };
    __device__ __forceinline__ Block block_of(const int at) const
    {
        Block k = {p[0], ld[0], 0, end[0]};
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (at >= end[q]) k = Block{p[q + 1], ld[q + 1], end[q], end[q + 1]};
        return k;
    }

    __device__ __forceinline__ float4 load4(const long long row, const bool row_ok, const int c, const int C) const
    {
        if (by_rows) {
            const Block k = block_of(row_ok ? (int)row : 0);               // stacked rows are weight rows: ints
            return mt_load4(k.p, k.ld, row - k.first, row_ok, c, C, k.vec());
        }
        const Block k = block_of(c);
        if (c >= C || c + 4 <= k.end || C <= k.end)                        // nothing to load, or everything in this block
            return mt_load4(k.p, k.ld, row, row_ok, c - k.first, (C < k.end ? C : k.end) - k.first, k.vec() && ((c - k.first) & 3) == 0);
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row_ok) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < C) {
                    const Block kj = block_of(c + j);
                    e[j] = kj.p[row * kj.ld + (c + j - kj.first)];
                }
        }
        return make_float4(e[0], e[1], e[2], e[3]);
    }
};

struct StNet {
    MtOp A, B;
    float *C[2];                                       // column blocks [0, csplit) and [csplit, N); NULL = not stored
    const float *bias[2];                              // MT_FWD: as C's blocks
    const float *H;                                    // MT_DGRAD with act: the saved activation [M][N]
    double *bpart;                                     // MT_WGRAD: [chunks][M]
};

struct StGemm {
    StNet net[DN_SAC_TRAIN_MAX_NETS];
    long long M, batch;
    int N, K;
    int ldc[2], csplit;                                // csplit = N where C is one block
    int ntn;                                           // column tiles a network: blockIdx.y = network * ntn + tile
    int act;                                           // 0 none, 1 + DN_MLP_ACT_x else
};
constexpr int ST_TANH = 1 + DN_MLP_ACT_TANH, ST_RELU = 1 + DN_MLP_ACT_RELU;

struct StOut {
    const StGemm &g;
    const StNet &nt;
    float *C0;                                         // nt.C[0], at this chunk's partial for the weight gradient
    __device__ __forceinline__ float bias(const int n) const { return n < g.csplit ? nt.bias[0][n] : nt.bias[1][n - g.csplit]; }
    template <int EPI>
    __device__ __forceinline__ void finish(const long long m, const int n, float v, const float bias) const
    {
        if (EPI == MT_FWD) {
            v = v + bias;
            if (g.act == ST_TANH) v = mt_tanh(v);
            if (g.act == ST_RELU) v = mt_relu(v);
        } else if (EPI == MT_DGRAD) {
            if (g.act) {
                const float hh = nt.H[m * g.N + n];
                v = g.act == ST_TANH ? mt_tanh_back(v, hh) : mt_relu_back(v, hh);
            }
        }
        const int b = n >= g.csplit;
        float *P = b ? nt.C[1] : C0;
        if (P) P[m * g.ldc[b] + (b ? n - g.csplit : n)] = v;
    }
    __device__ __forceinline__ void bias_sum(const long long m, const double s) const { nt.bpart[(long long)blockIdx.z * g.M + m] = s; }
};

template <int WM, int WN, int TM, int TN, bool AT, bool BT, int EPI>
__global__ __launch_bounds__(MT_THREADS, 2) void st_gemm_kernel(const StGemm g)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const int net = (int)blockIdx.y / g.ntn, tile = (int)blockIdx.y % g.ntn;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = tile * BN;
    const StNet &nt = g.net[net];

    MtOp A = nt.A, B = nt.B;
    float *C0 = nt.C[0];
    int K = g.K;
    if (EPI == MT_WGRAD) {                             // both operands are column blocks over the batch rows: every block moves to the chunk
        const long long row0 = (long long)blockIdx.z * DN_MLP_TRAIN_CHUNK, left = g.batch - row0;
        K = (int)(left < DN_MLP_TRAIN_CHUNK ? left : DN_MLP_TRAIN_CHUNK);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (A.p[b]) A.p[b] += row0 * A.ld[b];
            if (B.p[b]) B.p[b] += row0 * B.ld[b];
        }
        C0 += (long long)blockIdx.z * g.M * g.N;
    }
    const StOut out = {g, nt, C0};
    mt_gemm_tile<WM, WN, TM, TN, AT, BT, EPI>(A, B, g.M, g.N, K, m0, n0, EPI == MT_WGRAD && tile == 0, out);
}

// The chunks' partials -> the gradient tensors: grid y is the entry (a hidden layer or a head part of a network), a lane an element of
// (d_weight, d_bias).  A head part's rows are a slice of the head's partial, so the stride between chunks is the whole head's.
struct StMergeEntry {
    const float *wpart;
    const double *bpart;
    float *dw, *db;
    int nw, nb, wstride, bstride;
};
struct StMerge {
    StMergeEntry e[DN_SAC_TRAIN_MAX_NETS * DN_SAC_TRAIN_MAX_ENTRIES];
    int chunks, accumulate;
};

__global__ __launch_bounds__(MT_THREADS) void st_merge_kernel(const StMerge g)
{
    const StMergeEntry &t = g.e[blockIdx.y];
    int e = (int)(blockIdx.x * MT_THREADS + threadIdx.x);
    if (e < t.nw) {
        const float v = mt_merge_sum(t.wpart + e, t.wstride, g.chunks);
        t.dw[e] = g.accumulate ? t.dw[e] + v : v;
        return;
    }
    e -= t.nw;
    if (e < t.nb) {
        const float v = mt_merge_sum(t.bpart + e, t.bstride, g.chunks);
        t.db[e] = g.accumulate ? t.db[e] + v : v;
    }
}

__global__ __launch_bounds__(MT_THREADS) void st_polyak_kernel(const DnPolyakArgs g)
{
    const float *s = g.source[blockIdx.y];
    float *t = g.target[blockIdx.y];
    const long long n = g.count[blockIdx.y], step = (long long)gridDim.x * MT_THREADS;
    for (long long i = (long long)blockIdx.x * MT_THREADS + threadIdx.x; i < n; i += step) t[i] = dn_polyak(t[i], s[i], g.tau, g.omt);
}

template <int WM, int WN, int TM, int TN, bool AT, bool BT, int EPI>
void st_launch(StGemm &g, const int n_nets, const long long chunks, hipStream_t stream)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    g.ntn = (g.N + BN - 1) / BN;
    const dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)(g.ntn * n_nets), (unsigned)chunks);
    hipLaunchKernelGGL((st_gemm_kernel<WM, WN, TM, TN, AT, BT, EPI>), grid, dim3(MT_THREADS), 0, stream, g);
}

template <bool AT, bool BT, int EPI>
void st_product(StGemm &g, const int n_nets, const long long chunks, hipStream_t stream)
{
    const int shape = mt_pick(EPI, g.M, g.N);
    if (shape == MT_NARROW) return st_launch<4, 1, 1, 1, AT, BT, EPI>(g, n_nets, chunks, stream);
    if constexpr (EPI == MT_WGRAD)
        if (shape == MT_FLAT) return st_launch<1, 4, 1, 1, AT, BT, EPI>(g, n_nets, chunks, stream);
    st_launch<2, 2, 2, 2, AT, BT, EPI>(g, n_nets, chunks, stream);
}

MtOp st_op(const bool by_rows)
{
    MtOp o = {};
    for (int b = 0; b < 4; ++b) o.end[b] = INT_MAX;
    o.by_rows = by_rows;
    return o;
}
void st_block(MtOp &o, const int b, const float *p, const int ld, const int end, const bool last)
{
    o.p[b] = p;
    o.ld[b] = ld;
    o.end[b] = last ? INT_MAX : end;
}
MtOp st_single(const float *p, const int ld)
{
    MtOp o = st_op(false);
    st_block(o, 0, p, ld, 0, true);
    return o;
}

// What a pass knows of its networks: the dimensions (those of network 0), the scratch regions, and the operands that several products share.
struct StPass {
    const DnSacTrainArgs &a;
    DnSacTrainLayout lay;
    int L, P, in, head_out;

    explicit StPass(const DnSacTrainArgs &args) : a(args), L(args.n_layers), P(args.head_parts), in(args.in0 + args.in1), head_out(0)
    {
        lay = dn_sac_train_layout(a.layer[0], a.n_nets, L, P, a.batch);
        for (int p = 0; p < P; ++p) head_out += a.layer[0][L - 1 + p].out_dim;
    }
    int in_of(const int l) const { return a.layer[0][l].in_dim; }
    int out_of(const int l) const { return l == L - 1 ? head_out : a.layer[0][l].out_dim; }
    float *h(const int c, const int l) const { return reinterpret_cast<float *>(a.scratch + c * lay.per_net + lay.one.h[l]); }
    float *dz(const int c, const int l) const { return reinterpret_cast<float *>(a.scratch + c * lay.per_net + lay.one.dz[l]); }
    float *wpart(const int c, const int l) const { return reinterpret_cast<float *>(a.scratch + c * lay.per_net + lay.one.wpart[l]); }
    double *bpart(const int c, const int l) const { return reinterpret_cast<double *>(a.scratch + c * lay.per_net + lay.one.bpart[l]); }

    MtOp x() const                                     // (x0 | x1)
    {
        MtOp o = st_op(false);
        st_block(o, 0, a.x0, a.in0, a.in0, a.in1 == 0);
        if (a.in1) st_block(o, 1, a.x1, a.in1, in, true);
        return o;
    }
    MtOp input(const int c, const int l) const { return l == 0 ? x() : st_single(h(c, l - 1), in_of(l)); }
    MtOp dz_in(const int c, const int l) const         // dZ_l of network c: the head's is (d_out part 0 | d_out part 1)
    {
        if (l < L - 1) return st_single(dz(c, l), out_of(l));
        MtOp o = st_op(false);
        int end = 0;
        for (int p = 0; p < P; ++p) {
            end += a.layer[c][L - 1 + p].out_dim;
            st_block(o, p, a.d_out[c][p], a.layer[c][L - 1 + p].out_dim, end, p == P - 1);
        }
        return o;
    }
    MtOp weight(const int c, const int l) const        // W_l of network c [out][in]: the head's parts stacked
    {
        MtOp o = st_op(true);
        if (l < L - 1) {
            st_block(o, 0, a.layer[c][l].weight, in_of(l), 0, true);
            return o;
        }
        int end = 0;
        for (int p = 0; p < P; ++p) {
            end += a.layer[c][L - 1 + p].out_dim;
            st_block(o, p, a.layer[c][L - 1 + p].weight, in_of(l), end, p == P - 1);
        }
        return o;
    }
};

// What bounds the tables and loops of this unit, as the C ABI has checked it (the launchers index arrays by these numbers).
bool st_args_ok(const DnSacTrainArgs &a)
{
    return a.n_nets >= 1 && a.n_nets <= DN_SAC_TRAIN_MAX_NETS && a.n_layers >= 2 && a.n_layers <= DN_MLP_TRAIN_MAX_LAYERS && a.head_parts >= 1 &&
           a.head_parts <= DN_SAC_TRAIN_MAX_PARTS && a.batch >= 1 && a.batch <= (1ll << 24) && a.in0 >= 1 && a.in0 <= 64 && a.in1 >= 0 &&
           a.in1 <= 63 && a.in0 + a.in1 <= 64 && (a.activation == DN_MLP_ACT_TANH || a.activation == DN_MLP_ACT_RELU);
}

}  // namespace

hipError_t dn_launch_sac_train_forward(const DnSacTrainArgs &a, hipStream_t stream)
{
    if (!st_args_ok(a)) return hipErrorInvalidValue;
    const StPass s(a);
    for (int l = 0; l < s.L; ++l) {
        const bool head = l == s.L - 1;
        StGemm g = {};
        for (int c = 0; c < a.n_nets; ++c) {
            StNet &nt = g.net[c];
            nt.A = s.input(c, l);
            nt.B = s.weight(c, l);
            if (head) {
                for (int p = 0; p < s.P; ++p) { nt.C[p] = a.out[c][p]; nt.bias[p] = a.layer[c][l + p].bias; }
            } else {
                nt.C[0] = s.h(c, l); nt.bias[0] = a.layer[c][l].bias;
            }
        }
        g.M = a.batch; g.N = s.out_of(l); g.K = s.in_of(l);
        g.csplit = g.N; g.ldc[0] = g.N;
        if (head && s.P == 2) { g.csplit = a.layer[0][l].out_dim; g.ldc[0] = g.csplit; g.ldc[1] = a.layer[0][l + 1].out_dim; }
        g.act = head ? 0 : 1 + a.activation;
        st_product<false, false, MT_FWD>(g, a.n_nets, 1, stream);
    }
    return hipGetLastError();
}

hipError_t dn_launch_sac_train_backward(const DnSacTrainArgs &a, hipStream_t stream)
{
    if (!st_args_ok(a)) return hipErrorInvalidValue;
    const StPass s(a);
    const bool params = !(a.flags & DN_MLP_TRAIN_NO_PARAM_GRADS);
    StMerge mg = {};
    int entries = 0, most = 0;
    for (int l = s.L - 1; l >= 0; --l) {
        const int out = s.out_of(l), in = s.in_of(l);
        if (params) {
            StGemm g = {};
            for (int c = 0; c < a.n_nets; ++c) {
                StNet &nt = g.net[c];
                nt.A = s.dz_in(c, l);
                nt.B = s.input(c, l);
                nt.C[0] = s.wpart(c, l);
                nt.bpart = s.bpart(c, l);
                int row = 0;
                for (int p = 0; p < (l == s.L - 1 ? s.P : 1); ++p) {       // a head part is the rows [row, row + o) of the head's partial
                    const dn_mlp_train_layer &T = a.layer[c][l + p];
                    StMergeEntry &e = mg.e[entries++];
                    e.wpart = nt.C[0] + (long long)row * in; e.bpart = nt.bpart + row;
                    e.dw = T.d_weight; e.db = T.d_bias;
                    e.nw = T.out_dim * in; e.nb = T.out_dim; e.wstride = out * in; e.bstride = out;
                    most = e.nw + e.nb > most ? e.nw + e.nb : most;
                    row += T.out_dim;
                }
            }
            g.M = out; g.N = in; g.batch = a.batch;
            g.csplit = g.N; g.ldc[0] = g.N;
            st_product<true, true, MT_WGRAD>(g, a.n_nets, s.lay.one.chunks, stream);
        }
        if (l > 0) {
            StGemm g = {};
            for (int c = 0; c < a.n_nets; ++c) {
                StNet &nt = g.net[c];
                nt.A = s.dz_in(c, l);
                nt.B = s.weight(c, l);
                nt.C[0] = s.dz(c, l - 1);
                nt.H = s.h(c, l - 1);
            }
            g.M = a.batch; g.N = in; g.K = out;
            g.csplit = g.N; g.ldc[0] = g.N;
            g.act = 1 + a.activation;
            st_product<false, true, MT_DGRAD>(g, a.n_nets, 1, stream);
        } else if (a.d_x0 || a.d_x1) {                 // one product over the networks: [dZ0_0 | dZ0_1 | ...] against the stacked W0_c
            StGemm g = {};
            StNet &nt = g.net[0];
            nt.A = st_op(false);
            nt.B = st_op(true);
            for (int c = 0; c < a.n_nets; ++c) {
                st_block(nt.A, c, s.dz(c, 0), out, (c + 1) * out, c == a.n_nets - 1);
                st_block(nt.B, c, a.layer[c][0].weight, in, (c + 1) * out, c == a.n_nets - 1);
            }
            nt.C[0] = a.d_x0; nt.C[1] = a.d_x1;
            g.M = a.batch; g.N = in; g.K = out * a.n_nets;
            g.csplit = a.in0; g.ldc[0] = a.in0; g.ldc[1] = a.in1;
            st_product<false, true, MT_DGRAD>(g, 1, 1, stream);
        }
    }
    if (params) {
        mg.chunks = (int)s.lay.one.chunks; mg.accumulate = (a.flags & DN_MLP_TRAIN_ACCUMULATE) != 0;
        hipLaunchKernelGGL(st_merge_kernel, dim3((unsigned)((most + MT_THREADS - 1) / MT_THREADS), (unsigned)entries), dim3(MT_THREADS), 0, stream, mg);
    }
    return hipGetLastError();
}

hipError_t dn_launch_polyak(const DnPolyakArgs &a, hipStream_t stream)
{
    if (a.n_tensors < 1 || a.n_tensors > DN_ADAM_MAX_TENSORS) return hipErrorInvalidValue;
    long long most = 1;
    for (int i = 0; i < a.n_tensors; ++i) most = a.count[i] > most ? a.count[i] : most;
    const long long blocks = (most + MT_THREADS - 1) / MT_THREADS;
    hipLaunchKernelGGL(st_polyak_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), (unsigned)a.n_tensors), dim3(MT_THREADS), 0, stream, a);
    return hipGetLastError();
}
