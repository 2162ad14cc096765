// dn_mlp_train.hip -- the training pass of the reference's Tanh networks for gfx950 (dn_mlp_train_forward / dn_mlp_train_backward,
// include/dronenav.h): forward with the hidden activations saved, backward to every weight and bias gradient and to the input.
//
// One tiled product kernel, mt_gemm_kernel, serves the three product shapes.  C[m][n] = sum over k of A[m][k] B[k][n] with
//   forward          A = h_{l-1} [batch][in]   (k contiguous)   B = W_l [out][in]   (k contiguous)   epilogue: + bias, tanh, store h_l
//   data gradient    A = dZ_l [batch][out]     (k contiguous)   B = W_l [out][in]   (k strided)      epilogue: x (1 - h_{l-1}^2), store dZ_{l-1}
//   weight gradient  A = dZ_l [rows][out]      (k strided)      B = h_{l-1} [rows][in] (k strided)   epilogue: store the chunk's partial
// Every operand is read as the float32 tensor it is, split into bf16 hi and lo words (dn_bf16_split.h) on its way into LDS, and kept
// there as [row or column][k] images of 32 k per step, so that both MFMA fragments are 16-byte reads of 8 consecutive k.  An operand
// whose k is strided in memory is transposed in the staging pass: a lane loads a 4 x 4 block (four rows of k, four consecutive
// columns) and writes four 8-byte words.  The next step's global loads are issued before the MFMAs of the current one.
//   v_mfma_f32_32x32x16_bf16: lane l (r = l & 31, g = l >> 5) holds A[row r][k = 8 g + j], B[k = 8 g + j][col r], j = 0..7, and the
//   accumulator element (row (i & 3) + 8 (i >> 2) + 4 g, col r) in register i.
// A product is lo hi, hi lo, hi hi into one accumulator, K-steps of 16 ascending: the order of a row's sums depends on K alone, not on
// the tile shape or on where the row sits, so the three tile shapes below give the same bits.
//   BIG    128 x 128, four waves as 2 x 2, a wave 2 x 2 MFMA tiles        N > 32
//   NARROW 128 x 32,  four waves as 4 x 1, a wave one tile                N <= 32: the head, the 13 columns of d_weight_0
//   FLAT   32 x 128,  four waves as 1 x 4, a wave one tile                weight gradient with M <= 32: the head's d_weight
// Rows and columns beyond the matrix are staged as exact zeros and never stored.
//
// The weight gradient sums over the batch: grid z is the chunk of DN_MLP_TRAIN_CHUNK rows, and each (chunk, tile) workgroup writes its
// float32 partial to scratch.  The workgroups of column tile 0 also form the chunk's float64 column sums of dZ (the bias gradient)
// from the values they stage: a lane adds its four rows of every K-step in ascending order, and the eight lane groups of a column
// are added in ascending order through LDS.  mt_merge_kernel adds the chunks in ascending order in float64 and rounds once.
// No atomics, no workgroup waits for another, plain launches: capturable.
#include "dn_internal.h"
#include "dn_bf16_split.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT_THREADS = 256;
constexpr int MT_BK = 32;                              // k per staged step: two MFMA K-steps
constexpr int MT_LDK = 40;                             // bf16 per LDS row: 80 bytes keep the 16-byte fragment reads of 16 lanes on distinct slots
static_assert(DN_MLP_TRAIN_CHUNK % MT_BK == 0, "a chunk is whole staged steps");

enum { MT_FWD = 0, MT_DGRAD = 1, MT_WGRAD = 2 };

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

// Four consecutive elements (row, c .. c + 3) of a dense [*][ld] matrix, +0.0 where the row is off or the column is at or beyond C.
__device__ __forceinline__ float4 mt_load4(const float *__restrict__ P, const long long ld, const long long row, const bool row_ok, const int c,
                                           const int C, const bool vec)
{
    float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row_ok) {
        const float *p = P + row * ld + c;
        if (vec && c + 4 <= C) {
            r = *reinterpret_cast<const float4 *>(p);
        } else {
            if (c < C) r.x = p[0];
            if (c + 1 < C) r.y = p[1];
            if (c + 2 < C) r.z = p[2];
            if (c + 3 < C) r.w = p[3];
        }
    }
    return r;
}

__device__ __forceinline__ void mt_split4(const float a, const float b, const float c, const float d, uint2 &hi, uint2 &lo)
{
    uint32_t h0, l0, h1, l1;
    dn_bf16_split_pair(a, b, &h0, &l0);
    dn_bf16_split_pair(c, d, &h1, &l1);
    hi = make_uint2(h0, h1);
    lo = make_uint2(l0, l1);
}

// The staging of one operand tile of BR rows-or-columns x 32 k.  TR = false: k is contiguous in memory, (index, k) at P[index * ld + k];
// a lane takes BR / 32 words of four k.  TR = true: k is strided, (index, k) at P[k * ld + index]; the lanes of the first BR / 32 waves
// take a 4 (k) x 4 (index) block each: lane bits 0..2 and the wave pick the index group, bits 3..5 the k group, so that eight lanes read
// 128 consecutive bytes of a row.
template <int BR, bool TR>
struct MtStage {
    float4 v[4];

    static __device__ __forceinline__ bool active(const int tid) { return !TR || (tid >> 6) < BR / 32; }
    static __device__ __forceinline__ int rg(const int tid) { return (tid & 7) + 8 * (tid >> 6); }
    static __device__ __forceinline__ int kg(const int tid) { return (tid >> 3) & 7; }

    // index0: the tile's first row or column; n_index: how many the matrix has; k0, K: this step's first k and the product's K
    __device__ __forceinline__ void load(const float *__restrict__ P, const long long ld, const long long index0, const long long n_index,
                                         const int k0, const int K, const bool vec, const int tid)
    {
        if (!TR) {
#pragma unroll
            for (int i = 0; i < BR / 32; ++i) {
                const int u = tid + MT_THREADS * i;
                const long long row = index0 + (u >> 3);
                v[i] = mt_load4(P, ld, row, row < n_index, k0 + 4 * (u & 7), K, vec);
            }
        } else if (active(tid)) {
            const long long c = index0 + 4 * rg(tid);
            const int cc = (int)(c < n_index ? c : n_index), nn = (int)n_index;      // columns are ints: at most 512 here
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * kg(tid) + j;
                v[j] = mt_load4(P, ld, k, k < K, cc, nn, vec);
            }
        }
    }

    // into the hi and lo images s[2][BR][MT_LDK]
    __device__ __forceinline__ void store(unsigned short (*__restrict__ s)[BR][MT_LDK], const int tid) const
    {
        uint2 hi, lo;
        if (!TR) {
#pragma unroll
            for (int i = 0; i < BR / 32; ++i) {
                const int u = tid + MT_THREADS * i;
                mt_split4(v[i].x, v[i].y, v[i].z, v[i].w, hi, lo);
                *reinterpret_cast<uint2 *>(&s[0][u >> 3][4 * (u & 7)]) = hi;
                *reinterpret_cast<uint2 *>(&s[1][u >> 3][4 * (u & 7)]) = lo;
            }
        } else if (active(tid)) {
            const int r = 4 * rg(tid), k = 4 * kg(tid);
            mt_split4(v[0].x, v[1].x, v[2].x, v[3].x, hi, lo);
            *reinterpret_cast<uint2 *>(&s[0][r][k]) = hi;
            *reinterpret_cast<uint2 *>(&s[1][r][k]) = lo;
            mt_split4(v[0].y, v[1].y, v[2].y, v[3].y, hi, lo);
            *reinterpret_cast<uint2 *>(&s[0][r + 1][k]) = hi;
            *reinterpret_cast<uint2 *>(&s[1][r + 1][k]) = lo;
            mt_split4(v[0].z, v[1].z, v[2].z, v[3].z, hi, lo);
            *reinterpret_cast<uint2 *>(&s[0][r + 2][k]) = hi;
            *reinterpret_cast<uint2 *>(&s[1][r + 2][k]) = lo;
            mt_split4(v[0].w, v[1].w, v[2].w, v[3].w, hi, lo);
            *reinterpret_cast<uint2 *>(&s[0][r + 3][k]) = hi;
            *reinterpret_cast<uint2 *>(&s[1][r + 3][k]) = lo;
        }
    }
};

__device__ __forceinline__ float mt_tanh(const float z)
{
    const float e = __builtin_amdgcn_exp2f(z * 2.885390081777927f);               // 2 log2(e)
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

template <int WM, int WN, int TM, int TN, bool AT, bool BT, int EPI>
__global__ __launch_bounds__(MT_THREADS, 2) void mt_gemm_kernel(const MtGemm g)
{
    static_assert(WM * WN * 64 == MT_THREADS, "four waves");
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    static_assert(EPI != MT_WGRAD || (AT && BT), "the weight gradient sums over rows: both operands are k-strided");
    static_assert(!AT || 2 * BM * MT_LDK * 2 >= 8 * BM * 8, "the bias sums reuse the A image");
    __shared__ __attribute__((aligned(16))) unsigned short sA[2][BM][MT_LDK];
    __shared__ __attribute__((aligned(16))) unsigned short sB[2][BN][MT_LDK];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
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
    const bool vecA = (g.lda & 3) == 0 && ((uintptr_t)A & 15u) == 0;
    const bool vecB = (g.ldb & 3) == 0 && ((uintptr_t)B & 15u) == 0;
    const bool bias_sums = EPI == MT_WGRAD && blockIdx.y == 0;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    double bsum[4] = {0.0, 0.0, 0.0, 0.0};

    MtStage<BM, AT> stA;
    MtStage<BN, BT> stB;
    stA.load(A, g.lda, m0, g.M, 0, K, vecA, tid);
    stB.load(B, g.ldb, n0, g.N, 0, K, vecB, tid);

    for (int k0 = 0; k0 < K; k0 += MT_BK) {
        stA.store(sA, tid);
        stB.store(sB, tid);
        if (AT && bias_sums && stA.active(tid)) {      // rows k0 + 4 kg .. + 3 of this lane's four columns, ascending
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bsum[0] += (double)stA.v[j].x;
                bsum[1] += (double)stA.v[j].y;
                bsum[2] += (double)stA.v[j].z;
                bsum[3] += (double)stA.v[j].w;
            }
        }
        __syncthreads();
        if (k0 + MT_BK < K) {
            stA.load(A, g.lda, m0, g.M, k0 + MT_BK, K, vecA, tid);
            stB.load(B, g.ldb, n0, g.N, k0 + MT_BK, K, vecB, tid);
        }
        const int steps = K - k0 > 16 ? 2 : 1;         // a second K-step of zeros adds nothing: skipped
        for (int s = 0; s < steps; ++s) {
            const int kk = 16 * s + 8 * h;
            uint4 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = (wm * TM + i) * 32 + r;
                ah[i] = *reinterpret_cast<const uint4 *>(&sA[0][row][kk]);
                al[i] = *reinterpret_cast<const uint4 *>(&sA[1][row][kk]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = (wn * TN + j) * 32 + r;
                bh[j] = *reinterpret_cast<const uint4 *>(&sB[0][col][kk]);
                bl[j] = *reinterpret_cast<const uint4 *>(&sB[1][col][kk]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    f32x16 c = acc[i][j];
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al[i]), __builtin_bit_cast(bf16x8, bh[j]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[i]), __builtin_bit_cast(bf16x8, bl[j]), c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[i]), __builtin_bit_cast(bf16x8, bh[j]), c, 0, 0, 0);
                    acc[i][j] = c;
                }
        }
        __syncthreads();
    }

    if (AT && bias_sums) {                             // the A image is free after the last barrier
        double *red = reinterpret_cast<double *>(&sA[0][0][0]);                  // [8 k groups][BM]
        if (stA.active(tid)) {
            const int c = 4 * stA.rg(tid), kg = stA.kg(tid);
#pragma unroll
            for (int j = 0; j < 4; ++j) red[kg * BM + c + j] = bsum[j];
        }
        __syncthreads();
        if (tid < BM && m0 + tid < g.M) {
            double s = red[tid];
#pragma unroll
            for (int q = 1; q < 8; ++q) s += red[q * BM + tid];
            g.bpart[(long long)blockIdx.z * g.M + m0 + tid] = s;
        }
    }

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + r;
            const bool n_ok = n < g.N;
            float bias = 0.0f;
            if (EPI == MT_FWD && n_ok) bias = g.bias[n];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (n_ok && m < g.M) {
                    float v = acc[i][j][e];
                    if (EPI == MT_FWD) {
                        v = v + bias;
                        if (g.act) v = mt_tanh(v);
                    } else if (EPI == MT_DGRAD) {
                        if (g.act) {
                            const float hh = g.H[m * g.ldc + n];
                            v = v * (1.0f - hh * hh);
                        }
                    }
                    C[m * g.ldc + n] = v;
                }
            }
        }
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
            const float *p = g.wpart[l] + e;
            double s = (double)p[0];
            for (int c = 1; c < g.chunks; ++c) s += (double)p[(long long)c * g.nw[l]];
            const float v = (float)s;
            g.dw[l][e] = g.accumulate ? g.dw[l][e] + v : v;
            return;
        }
        e -= g.nw[l];
        if (e < g.nb[l]) {
            const double *p = g.bpart[l] + e;
            double s = p[0];
            for (int c = 1; c < g.chunks; ++c) s += p[(long long)c * g.nb[l]];
            const float v = (float)s;
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

// The tile shape of a product: by N alone for the products over batch rows (a row's bits do not depend on the shape, and neither
// does the choice on the batch), FLAT for a weight gradient of at most 32 rows.
template <bool AT, bool BT, int EPI>
void mt_product(const MtGemm &g, const long long chunks, hipStream_t stream)
{
    if (g.N <= 32) return mt_launch<4, 1, 1, 1, AT, BT, EPI>(g, chunks, stream);
    if constexpr (EPI == MT_WGRAD)
        if (g.M <= 32) return mt_launch<1, 4, 1, 1, AT, BT, EPI>(g, chunks, stream);
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
