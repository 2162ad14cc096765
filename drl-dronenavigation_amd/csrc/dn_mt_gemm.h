// dn_mt_gemm.h -- the tiled product of the networks' training passes, stated once for dn_mlp_train.hip (the Tanh networks of PPO) and
// dn_sac_train.hip (the SAC networks): the staging with its bf16 split, the MFMA loop, the tile-shape pick and the per-element arithmetic
// of the epilogues and of the merge.  A unit supplies what differs -- where an operand's elements live, and what becomes of a finished
// accumulator element -- as small policy objects, and the __global__ wrapper that builds them from its argument struct.
//
// C[m][n] = sum over k of A[m][k] B[k][n] with
//   forward          A = h_{l-1} [batch][in]   (k contiguous)   B = W_l [out][in]   (k contiguous)   epilogue: + bias, activation, store h_l
//   data gradient    A = dZ_l [batch][out]     (k contiguous)   B = W_l [out][in]   (k strided)      epilogue: x act'(h_{l-1}), store dZ_{l-1}
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
// The weight gradient sums over the batch: each (chunk of DN_MLP_TRAIN_CHUNK rows, tile) workgroup writes its float32 partial to
// scratch.  The workgroups of column tile 0 also form the chunk's float64 column sums of dZ (the bias gradient) from the values they
// stage: a lane adds its four rows of every K-step in ascending order, and the eight lane groups of a column are added in ascending
// order through LDS.  The merge adds the chunks in ascending order in float64 and rounds once.
#pragma once

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

// The tile shape of a product: by N alone for the products over batch rows (a row's bits do not depend on the shape, and neither
// does the choice on the batch), FLAT for a weight gradient of at most 32 rows.
enum { MT_BIG = 0, MT_NARROW = 1, MT_FLAT = 2 };
inline int mt_pick(const int epi, const long long M, const int N) { return N <= 32 ? MT_NARROW : epi == MT_WGRAD && M <= 32 ? MT_FLAT : MT_BIG; }

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

// An operand that is one dense matrix.  vec: ld % 4 == 0 and P is 16-byte aligned.
struct MtPlainOp {
    const float *P;
    long long ld;
    bool vec;
    __device__ __forceinline__ float4 load4(const long long row, const bool row_ok, const int c, const int C) const
    {
        return mt_load4(P, ld, row, row_ok, c, C, vec);
    }
};

__device__ __forceinline__ void mt_split4(const float a, const float b, const float c, const float d, uint2 &hi, uint2 &lo)
{
    uint32_t h0, l0, h1, l1;
    dn_bf16_split_pair(a, b, &h0, &l0);
    dn_bf16_split_pair(c, d, &h1, &l1);
    hi = make_uint2(h0, h1);
    lo = make_uint2(l0, l1);
}

// The staging of one operand tile of BR rows-or-columns x 32 k.  TR = false: k is contiguous in memory, (index, k) is element (index, k)
// of the operand; a lane takes BR / 32 words of four k.  TR = true: k is strided, (index, k) is element (k, index); the lanes of the first
// BR / 32 waves take a 4 (k) x 4 (index) block each: lane bits 0..2 and the wave pick the index group, bits 3..5 the k group, so that
// eight lanes read 128 consecutive bytes of a row.
template <int BR, bool TR>
struct MtStage {
    float4 v[4];

    static __device__ __forceinline__ bool active(const int tid) { return !TR || (tid >> 6) < BR / 32; }
    static __device__ __forceinline__ int rg(const int tid) { return (tid & 7) + 8 * (tid >> 6); }
    static __device__ __forceinline__ int kg(const int tid) { return (tid >> 3) & 7; }

    // index0: the tile's first row or column; n_index: how many the matrix has; k0, K: this step's first k and the product's K
    template <class Op>
    __device__ __forceinline__ void load(const Op &op, const long long index0, const long long n_index, const int k0, const int K, const int tid)
    {
        if (!TR) {
#pragma unroll
            for (int i = 0; i < BR / 32; ++i) {
                const int u = tid + MT_THREADS * i;
                const long long row = index0 + (u >> 3);
                v[i] = op.load4(row, row < n_index, k0 + 4 * (u & 7), K);
            }
        } else if (active(tid)) {
            const long long c = index0 + 4 * rg(tid);
            const int cc = (int)(c < n_index ? c : n_index), nn = (int)n_index;      // columns are ints: at most 512 here
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * kg(tid) + j;
                v[j] = op.load4(k, k < K, cc, nn);
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

// The activations, each with the factor of its derivative taken from the saved activation h.
__device__ __forceinline__ float mt_tanh(const float z)
{
    const float e = __builtin_amdgcn_exp2f(z * 2.885390081777927f);               // 2 log2(e)
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}
__device__ __forceinline__ float mt_tanh_back(const float d, const float h) { return d * (1.0f - h * h); }
__device__ __forceinline__ float mt_relu(const float z) { return z > 0.0f ? z : 0.0f; }                     // a NaN becomes +0: outside the contract
__device__ __forceinline__ float mt_relu_back(const float d, const float h) { return h > 0.0f ? d : 0.0f; }  // torch's threshold_backward

// One output tile of a product, by the workgroup that calls it: rows m0 .., columns n0 .. of the M x N result over K.  bias_sums (weight
// gradient only): this workgroup also forms the float64 column sums of the A operand over its K rows and hands them to out.bias_sum.
// Op: load4(row, row_ok, c, C), four consecutive elements of a row with +0.0 where row_ok is false or the column is at or beyond C.
// Out: bias(n) (forward), finish<EPI>(m, n, v, bias) for every accumulator element inside the matrix, bias_sum(m, s).
template <int WM, int WN, int TM, int TN, bool AT, bool BT, int EPI, class OpA, class OpB, class Out>
__device__ __forceinline__ void mt_gemm_tile(const OpA &A, const OpB &B, const long long M, const int N, const int K, const long long m0,
                                             const int n0, const bool bias_sums, const Out &out)
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
    stA.load(A, m0, M, 0, K, tid);
    stB.load(B, n0, N, 0, K, tid);

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
            stA.load(A, m0, M, k0 + MT_BK, K, tid);
            stB.load(B, n0, N, k0 + MT_BK, K, tid);
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
        if (tid < BM && m0 + tid < M) {
            double s = red[tid];
#pragma unroll
            for (int q = 1; q < 8; ++q) s += red[q * BM + tid];
            out.bias_sum(m0 + tid, s);
        }
    }

#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + r;
            const bool n_ok = n < N;
            float bias = 0.0f;
            if (EPI == MT_FWD && n_ok) bias = out.bias(n);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long long m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (n_ok && m < M) out.template finish<EPI>(m, n, acc[i][j][e], bias);
            }
        }
}

// One gradient element from its chunks' partials (float32 weight partials or float64 bias partials, `stride` apart): added in ascending
// chunk order in float64 and rounded once.  The caller stores it or, to accumulate, adds it to what is there by one float32 add.
template <class T>
__device__ __forceinline__ float mt_merge_sum(const T *p, const long long stride, const int chunks)
{
    double s = (double)p[0];
    for (int c = 1; c < chunks; ++c) s += (double)p[(long long)c * stride];
    return (float)s;
}

}  // namespace
