// dn_mlp_train.hip -- the training pass of the reference's Tanh networks for gfx950 (dn_mlp_train_forward / dn_mlp_train_backward,
// include/dronenav.h): forward with the hidden activations saved, backward to every weight and bias gradient and to the input.
//
// The tiled product, its staging, MFMA loop, tile shapes and the arithmetic of its epilogues are csrc/dn_mt_gemm.h, which this unit shares
// with dn_sac_train.hip; what is here is this family's argument struct, its kernels' wrappers and its launches: every operand one dense
// matrix, Tanh, one network a call.  Grid z of the weight gradient is the chunk of DN_MLP_TRAIN_CHUNK rows.
// No atomics, no workgroup waits for another, plain launches: capturable.
#include "dn_mt_gemm.h"

namespace {

struct MtGemm {
    const float *A, *B;
    float *C;
    const float *bias;                                 // MT_FWD: [N]
    const float *H;                                    // MT_DGRAD with act: the activation of C's shape and stride
    double *bpart;                                     // MT_WGRAD: [chunks][M], written by the workgroups of column tile 0
    long long lda, ldb, ldc;
    long long M;                                       // rows of C: the batch (forward, data gradient) or out_dim (weight gradient)
    long long batch;                                   // MT_WGRAD: K is the rows of the chunk
    int N, K;
    int act;                                           // MT_FWD: tanh; MT_DGRAD: the 1 - h^2 factor
};

// What becomes of a finished accumulator element, and of a chunk's bias sums.
struct MtPlainOut {
    const MtGemm &g;
    float *C;
    __device__ __forceinline__ float bias(const int n) const { return g.bias[n]; }
    template <int EPI>
    __device__ __forceinline__ void finish(const long long m, const int n, float v, const float bias) const
    {
        if (EPI == MT_FWD) {
            v = v + bias;
            if (g.act) v = mt_tanh(v);
        } else if (EPI == MT_DGRAD) {
            if (g.act) v = mt_tanh_back(v, g.H[m * g.ldc + n]);
        }
        C[m * g.ldc + n] = v;
    }
    __device__ __forceinline__ void bias_sum(const long long m, const double s) const { g.bpart[(long long)blockIdx.z * g.M + m] = s; }
};

template <int WM, int WN, int TM, int TN, bool AT, bool BT, int EPI>
__global__ __launch_bounds__(MT_THREADS, 2) void mt_gemm_kernel(const MtGemm g)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = (int)blockIdx.y * BN;

    const float *A = g.A, *B = g.B;
    float *C = g.C;
    int K = g.K;
    if (EPI == MT_WGRAD) {
        const long long row0 = (long long)blockIdx.z * DN_MLP_TRAIN_CHUNK, left = g.batch - row0;
        K = (int)(left < DN_MLP_TRAIN_CHUNK ? left : DN_MLP_TRAIN_CHUNK);
        A += row0 * g.lda;
        B += row0 * g.ldb;
        C += (long long)blockIdx.z * g.M * g.N;
    }
    const MtPlainOp opA = {A, g.lda, (g.lda & 3) == 0 && ((uintptr_t)A & 15u) == 0};
    const MtPlainOp opB = {B, g.ldb, (g.ldb & 3) == 0 && ((uintptr_t)B & 15u) == 0};
    const MtPlainOut out = {g, C};
    mt_gemm_tile<WM, WN, TM, TN, AT, BT, EPI>(opA, opB, g.M, g.N, K, m0, n0, EPI == MT_WGRAD && blockIdx.y == 0, out);
}

// The chunks' partials -> the gradient tensors: element e of the concatenation (d_weight_0, d_bias_0, d_weight_1, ...), one per lane.
struct MtMerge {
    const float *wpart[DN_MLP_TRAIN_MAX_LAYERS];
    const double *bpart[DN_MLP_TRAIN_MAX_LAYERS];
    float *dw[DN_MLP_TRAIN_MAX_LAYERS], *db[DN_MLP_TRAIN_MAX_LAYERS];
    int nw[DN_MLP_TRAIN_MAX_LAYERS], nb[DN_MLP_TRAIN_MAX_LAYERS];
    int n_layers, chunks, accumulate;
};

__global__ __launch_bounds__(MT_THREADS) void mt_merge_kernel(const MtMerge g)
{
    long long e = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
    for (int l = 0; l < g.n_layers; ++l) {
        if (e < g.nw[l]) {
            const float v = mt_merge_sum(g.wpart[l] + e, g.nw[l], g.chunks);
            g.dw[l][e] = g.accumulate ? g.dw[l][e] + v : v;
            return;
        }
        e -= g.nw[l];
        if (e < g.nb[l]) {
            const float v = mt_merge_sum(g.bpart[l] + e, g.nb[l], g.chunks);
            g.db[l][e] = g.accumulate ? g.db[l][e] + v : v;
            return;
        }
        e -= g.nb[l];
    }
}

template <int WM, int WN, int TM, int TN, bool AT, bool BT, int EPI>
void mt_launch(const MtGemm &g, const long long chunks, hipStream_t stream)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN), (unsigned)chunks);
    hipLaunchKernelGGL((mt_gemm_kernel<WM, WN, TM, TN, AT, BT, EPI>), grid, dim3(MT_THREADS), 0, stream, g);
}

template <bool AT, bool BT, int EPI>
void mt_product(const MtGemm &g, const long long chunks, hipStream_t stream)
{
    const int shape = mt_pick(EPI, g.M, g.N);
    if (shape == MT_NARROW) return mt_launch<4, 1, 1, 1, AT, BT, EPI>(g, chunks, stream);
    if constexpr (EPI == MT_WGRAD)                     // the only product that has a FLAT kernel
        if (shape == MT_FLAT) return mt_launch<1, 4, 1, 1, AT, BT, EPI>(g, chunks, stream);
    mt_launch<2, 2, 2, 2, AT, BT, EPI>(g, chunks, stream);
}

}  // namespace

hipError_t dn_launch_mlp_train_forward(const DnMlpTrainArgs &a, hipStream_t stream)
{
    if (a.n_layers < 2 || a.n_layers > DN_MLP_TRAIN_MAX_LAYERS || a.batch < 1 || a.batch > (1ll << 24)) return hipErrorInvalidValue;
    const DnMlpTrainLayout lay = dn_mlp_train_layout(a.layer, a.n_layers, a.batch);
    const float *in = a.x;
    for (int l = 0; l < a.n_layers; ++l) {
        const dn_mlp_train_layer &L = a.layer[l];
        const bool head = l == a.n_layers - 1;
        MtGemm g = {};
        g.A = in; g.lda = L.in_dim;
        g.B = L.weight; g.ldb = L.in_dim;
        g.C = head ? a.out : reinterpret_cast<float *>(a.scratch + lay.h[l]); g.ldc = L.out_dim;
        g.bias = L.bias;
        g.M = a.batch; g.N = L.out_dim; g.K = L.in_dim;
        g.act = !head;
        mt_product<false, false, MT_FWD>(g, 1, stream);
        in = g.C;
    }
    return hipGetLastError();
}

hipError_t dn_launch_mlp_train_backward(const DnMlpTrainArgs &a, hipStream_t stream)
{
    if (a.n_layers < 2 || a.n_layers > DN_MLP_TRAIN_MAX_LAYERS || a.batch < 1 || a.batch > (1ll << 24)) return hipErrorInvalidValue;
    const DnMlpTrainLayout lay = dn_mlp_train_layout(a.layer, a.n_layers, a.batch);
    const bool params = !(a.flags & DN_MLP_TRAIN_NO_PARAM_GRADS);
    const auto h_of = [&](int l) { return reinterpret_cast<float *>(a.scratch + lay.h[l]); };      // the output of hidden layer l
    const auto dz_of = [&](int l) { return reinterpret_cast<float *>(a.scratch + lay.dz[l]); };
    MtMerge mg = {};
    long long elements = 0;
    for (int l = a.n_layers - 1; l >= 0; --l) {
        const dn_mlp_train_layer &L = a.layer[l];
        const float *dz = l == a.n_layers - 1 ? a.d_out : dz_of(l);
        const float *in = l == 0 ? a.x : h_of(l - 1);
        if (params) {
            MtGemm g = {};
            g.A = dz; g.lda = L.out_dim;
            g.B = in; g.ldb = L.in_dim;
            g.C = reinterpret_cast<float *>(a.scratch + lay.wpart[l]); g.ldc = L.in_dim;
            g.bpart = reinterpret_cast<double *>(a.scratch + lay.bpart[l]);
            g.M = L.out_dim; g.N = L.in_dim; g.batch = a.batch;
            mt_product<true, true, MT_WGRAD>(g, lay.chunks, stream);
            mg.wpart[l] = g.C; mg.bpart[l] = g.bpart;
            mg.dw[l] = L.d_weight; mg.db[l] = L.d_bias;
            mg.nw[l] = L.out_dim * L.in_dim; mg.nb[l] = L.out_dim;
            elements += mg.nw[l] + mg.nb[l];
        }
        if (l > 0 || a.d_x) {
            MtGemm g = {};
            g.A = dz; g.lda = L.out_dim;
            g.B = L.weight; g.ldb = L.in_dim;
            g.C = l == 0 ? a.d_x : dz_of(l - 1); g.ldc = L.in_dim;
            g.H = l == 0 ? nullptr : h_of(l - 1);
            g.M = a.batch; g.N = L.in_dim; g.K = L.out_dim;
            g.act = l > 0;
            mt_product<false, true, MT_DGRAD>(g, 1, stream);
        }
    }
    if (params) {
        mg.n_layers = a.n_layers; mg.chunks = (int)lay.chunks; mg.accumulate = (a.flags & DN_MLP_TRAIN_ACCUMULATE) != 0;
        hipLaunchKernelGGL(mt_merge_kernel, dim3((unsigned)((elements + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, stream, mg);
    }
    return hipGetLastError();
}
