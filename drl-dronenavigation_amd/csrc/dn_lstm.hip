// dn_lstm.hip -- one LSTM layer with torch.nn.LSTM semantics for gfx950 (dn_lstm_forward / dn_lstm_backward, include/dronenav.h): the
// training pass over a time-major sequence with episode starts inside it, and with T = 1 the rollout step.
//
// The product is csrc/dn_mt_gemm.h, the one dn_mlp_train.hip and dn_sac_train.hip run: same staging, split, MFMA chain and tile shapes.
// What this unit adds is addressing and epilogues:
//   the concatenated operand (LsCat): two column blocks, (x_t | hprev_t) against (W_ih | W_hh) in the forward, (x | hprev) over all T B
//     rows in the weight gradient.  hprev is never materialised: a row of it is a row of h0 or of h_seq, or +0.0 where the row's episode
//     starts at that step (dn_internal.h dn_lstm_prev).  A four-wide load inside one block is the plain one; one that straddles the two
//     gathers its elements one by one.  The order of a product's k does not know where the blocks meet.
//   the forward epilogue: + (b_ih + b_hh), the gate's activation, stored to the gates in scratch;
//   the per-step data gradient's epilogue: +0.0 for the rows whose episode starts at the step, stored to carry_h.
// The pointwise arithmetic of the cell is csrc/dn_lstm_cell.h; it runs in a kernel of its own after the forward product and before the
// step's data-gradient product, a lane an element of [B][H].
// Launches: forward 2 T; backward 2 T - 1, one for d_x where it is wanted, and the weight gradient with its merge where the parameter
// gradients are.  No atomics, no workgroup waits for another, plain launches: capturable.
//
// h_T and c_T may be h0 and c0: h0 is read by step 0's product only and c0 by step 0's cell kernel only, each element by the lane that
// (with T = 1) writes it afterwards; h_T and c_T are written by the last step's cell kernel, which the stream orders behind both.
#include "dn_mt_gemm.h"
#include "dn_lstm_cell.h"

namespace {

template <bool PREV>
struct LsCat {
    const float *p0;                                   // block 0 [*][I]: x or W_ih
    const float *p1;                                   // block 1 [*][H]: W_hh; PREV: h0
    const float *p1_seq;                               // PREV: h_seq
    const uint8_t *starts;                             // PREV: [T B], NULL = none
    long long row_base, B;                             // PREV: the operand's row 0 is row row_base of the T B rows
    int I, H;
    bool vec0, vec1;                                   // I % 4 == 0 and p0 16-byte aligned; p1 (and p1_seq) 16-byte aligned: H % 4 == 0 always

    // the row of block 1 behind `row`, nullptr where it is +0.0
    __device__ __forceinline__ const float *row1(const long long row) const
    {
        if (!PREV) return p1 + row * H;
        const long long at = row_base + row;
        const DnLstmPrev s = dn_lstm_prev(at, B, starts ? (int)starts[at] : 0);
        if (s.source == DN_LSTM_PREV_NONE) return nullptr;
        return (s.source == DN_LSTM_PREV_INITIAL ? p1 : p1_seq) + s.row * H;
    }

    __device__ __forceinline__ float4 load4(const long long row, const bool row_ok, const int c, const int C) const
    {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!row_ok || c >= C) return zero;
        const long long r0 = PREV ? row_base + row : row;
        if (c + 4 <= I || C <= I) return mt_load4(p0, I, r0, true, c, C < I ? C : I, vec0);
        const float *q = row1(row);
        if (c >= I) return q ? mt_load4(q, 0, 0, true, c - I, C - I, vec1 && ((c - I) & 3) == 0) : zero;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < I) e[j] = p0[r0 * I + c + j];
            else if (c + j < C && q) e[j] = q[c + j - I];
        return make_float4(e[0], e[1], e[2], e[3]);
    }
};

struct LsGemm {
    const float *x, *h0, *h_seq;                       // the (x | hprev) operand
    const uint8_t *starts;
    const float *w_ih, *w_hh, *b_ih, *b_hh;            // forward
    const float *A, *W;                                // data gradient: dZ rows [M][K], W [K][N]; weight gradient: A = dZ [rows][M]
    const uint8_t *mask;                               // data gradient: the step's episode starts [M], NULL = none
    float *C;
    double *bpart;                                     // weight gradient: [chunks][M]
    long long M, row_base, B, rows;                    // rows: weight gradient, T B
    int N, K, I, H;
};

struct LsOut {
    const LsGemm &g;
    float *C;
    __device__ __forceinline__ float bias(const int n) const { return g.b_ih[n] + g.b_hh[n]; }
    template <int EPI>
    __device__ __forceinline__ void finish(const long long m, const int n, float v, const float bias) const
    {
        if (EPI == MT_FWD) v = ls_gate(v + bias, n, g.H);
        if (EPI == MT_DGRAD && g.mask && g.mask[m]) v = 0.0f;
        C[m * g.N + n] = v;
    }
    __device__ __forceinline__ void bias_sum(const long long m, const double s) const { g.bpart[(long long)blockIdx.z * g.M + m] = s; }
};

__device__ __forceinline__ bool ls_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
__device__ __forceinline__ LsCat<true> ls_rows(const LsGemm &g, const long long row_base)
{
    return LsCat<true>{g.x, g.h0, g.h_seq, g.starts, row_base, g.B, g.I, g.H, (g.I & 3) == 0 && ls_aligned16(g.x),
                       ls_aligned16(g.h0) && ls_aligned16(g.h_seq)};
}

// gates[row_base + m][n] = act(sum_k (x | hprev)[row_base + m][k] (W_ih | W_hh)[n][k] + (b_ih + b_hh)[n]); C is the step's gates
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(MT_THREADS, 2) void ls_forward_kernel(const LsGemm g)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const LsCat<true> A = ls_rows(g, g.row_base);
    const LsCat<false> W = {g.w_ih, g.w_hh, nullptr, nullptr, 0, 0, g.I, g.H, (g.I & 3) == 0 && ls_aligned16(g.w_ih), ls_aligned16(g.w_hh)};
    const LsOut out = {g, g.C};
    mt_gemm_tile<WM, WN, TM, TN, false, false, MT_FWD>(A, W, g.M, g.N, g.K, (long long)blockIdx.x * BM, (int)blockIdx.y * BN, false, out);
}

// C[m][n] = sum_k A[m][k] W[k][n], +0.0 for the rows the mask names
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(MT_THREADS, 2) void ls_dgrad_kernel(const LsGemm g)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const MtPlainOp A = {g.A, g.K, (g.K & 3) == 0 && ls_aligned16(g.A)};
    const MtPlainOp W = {g.W, g.N, (g.N & 3) == 0 && ls_aligned16(g.W)};
    const LsOut out = {g, g.C};
    mt_gemm_tile<WM, WN, TM, TN, false, true, MT_DGRAD>(A, W, g.M, g.N, g.K, (long long)blockIdx.x * BM, (int)blockIdx.y * BN, false, out);
}

// partial[chunk][m][n] = sum over the chunk's rows of dZ[row][m] (x | hprev)[row][n]; grid z = the chunk
template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(MT_THREADS, 2) void ls_wgrad_kernel(const LsGemm g)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const long long row0 = (long long)blockIdx.z * DN_MLP_TRAIN_CHUNK, left = g.rows - row0;
    const int K = (int)(left < DN_MLP_TRAIN_CHUNK ? left : DN_MLP_TRAIN_CHUNK);
    const float *dz = g.A + row0 * g.M;
    const MtPlainOp A = {dz, g.M, (g.M & 3) == 0 && ls_aligned16(dz)};
    const LsCat<true> R = ls_rows(g, row0);
    const LsOut out = {g, g.C + (long long)blockIdx.z * g.M * g.N};
    mt_gemm_tile<WM, WN, TM, TN, true, true, MT_WGRAD>(A, R, g.M, g.N, K, (long long)blockIdx.x * BM, (int)blockIdx.y * BN, blockIdx.y == 0, out);
}

// The cell of step t, a lane an element (b, j) of [B][H].
struct LsCellArgs {
    float *gates;                                      // [T][B][4H]
    const float *c0;
    const uint8_t *starts;
    float *h_seq, *c_seq, *h_T, *c_T;                  // forward: written (h_T, c_T at the last step); backward: c_seq read
    const float *d_hseq;
    float *carry_h, *carry_c;
    long long t, T, B;
    int H;
};

__device__ __forceinline__ float ls_c_prev(const LsCellArgs &a, const long long row, const int j, bool &start)
{
    start = a.starts && a.starts[row];
    const DnLstmPrev s = dn_lstm_prev(row, a.B, start);
    if (s.source == DN_LSTM_PREV_NONE) return 0.0f;
    return (s.source == DN_LSTM_PREV_INITIAL ? a.c0 : a.c_seq)[s.row * a.H + j];
}

__global__ __launch_bounds__(MT_THREADS) void ls_cell_forward_kernel(const LsCellArgs a)
{
    const long long e = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (e >= a.B * a.H) return;
    const long long b = e / a.H, row = a.t * a.B + b;
    const int j = (int)(e - b * a.H), H = a.H;
    bool start;
    const float cp = ls_c_prev(a, row, j, start);
    const float *z = a.gates + row * 4 * H + j;
    const LsCell r = ls_cell_forward(z[0], z[H], z[2 * H], z[3 * H], cp);
    a.c_seq[row * H + j] = r.c;
    a.h_seq[row * H + j] = r.h;
    if (a.t == a.T - 1) {
        a.c_T[e] = r.c;
        a.h_T[e] = r.h;
    }
}

__global__ __launch_bounds__(MT_THREADS) void ls_cell_backward_kernel(const LsCellArgs a)
{
    const long long e = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
    if (e >= a.B * a.H) return;
    const long long b = e / a.H, row = a.t * a.B + b;
    const int j = (int)(e - b * a.H), H = a.H;
    bool start;
    const float cp = ls_c_prev(a, row, j, start);
    float *z = a.gates + row * 4 * H + j;
    const bool last = a.t == a.T - 1;                  // the carries start at zero
    const LsCellGrad r = ls_cell_backward(z[0], z[H], z[2 * H], z[3 * H], a.c_seq[row * H + j], cp, a.d_hseq[row * H + j],
                                          last ? 0.0f : a.carry_h[e], last ? 0.0f : a.carry_c[e]);
    z[0] = r.dz_i;
    z[H] = r.dz_f;
    z[2 * H] = r.dz_g;
    z[3 * H] = r.dz_o;
    a.carry_c[e] = start ? 0.0f : r.carry_c;
}

// The chunks' partials -> the gradient tensors, a lane an element: [4H][I + H] splits by columns into d_w_ih and d_w_hh, and the bias
// sums go to d_b_ih and d_b_hh alike.
struct LsMerge {
    const float *wpart;
    const double *bpart;
    float *d_w_ih, *d_w_hh, *d_b_ih, *d_b_hh;
    int I, H, chunks, accumulate;
};

__global__ __launch_bounds__(MT_THREADS) void ls_merge_kernel(const LsMerge g)
{
    const int e = (int)(blockIdx.x * MT_THREADS + threadIdx.x), K = g.I + g.H, nw = 4 * g.H * K;
    if (e < nw) {
        const float v = mt_merge_sum(g.wpart + e, nw, g.chunks);
        const int n = e / K, k = e - n * K;
        float *p = k < g.I ? g.d_w_ih + n * g.I + k : g.d_w_hh + n * g.H + (k - g.I);
        *p = g.accumulate ? *p + v : v;
    } else if (e - nw < 4 * g.H) {
        const int n = e - nw;
        const float v = mt_merge_sum(g.bpart + n, 4 * g.H, g.chunks);
        g.d_b_ih[n] = g.accumulate ? g.d_b_ih[n] + v : v;
        g.d_b_hh[n] = g.accumulate ? g.d_b_hh[n] + v : v;
    }
}

template <int WM, int WN, int TM, int TN>
dim3 ls_grid(const long long M, const int N, const long long chunks)
{
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    return dim3((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN), (unsigned)chunks);
}

void ls_dgrad(const LsGemm &g, hipStream_t stream)
{
    if (mt_pick(MT_DGRAD, g.M, g.N) == MT_NARROW)
        hipLaunchKernelGGL((ls_dgrad_kernel<4, 1, 1, 1>), (ls_grid<4, 1, 1, 1>(g.M, g.N, 1)), dim3(MT_THREADS), 0, stream, g);
    else
        hipLaunchKernelGGL((ls_dgrad_kernel<2, 2, 2, 2>), (ls_grid<2, 2, 2, 2>(g.M, g.N, 1)), dim3(MT_THREADS), 0, stream, g);
}

// What bounds the grids and offsets of this unit, as the C ABI has checked it.
bool ls_args_ok(const DnLstmArgs &a)
{
    return a.in_dim >= 1 && a.in_dim <= 64 && a.hidden >= 32 && a.hidden <= 512 && a.hidden % 32 == 0 && a.T >= 1 && a.T <= DN_LSTM_MAX_STEPS &&
           a.B >= 1 && a.B <= (1ll << 24) && a.T * a.B <= (1ll << 24);
}

LsGemm ls_common(const DnLstmArgs &a)
{
    LsGemm g = {};
    g.x = a.x; g.h0 = a.h0; g.h_seq = a.h_seq; g.starts = a.episode_starts;
    g.B = a.B; g.I = a.in_dim; g.H = a.hidden;
    return g;
}

LsCellArgs ls_cell_args(const DnLstmArgs &a, const DnLstmLayout &lay)
{
    LsCellArgs c = {};
    c.gates = reinterpret_cast<float *>(a.scratch + lay.gates);
    c.c0 = a.c0; c.starts = a.episode_starts;
    c.h_seq = a.h_seq; c.c_seq = a.c_seq; c.h_T = a.h_T; c.c_T = a.c_T;
    c.d_hseq = a.d_hseq;
    c.carry_h = reinterpret_cast<float *>(a.scratch + lay.carry_h);
    c.carry_c = reinterpret_cast<float *>(a.scratch + lay.carry_c);
    c.T = a.T; c.B = a.B; c.H = a.hidden;
    return c;
}

}  // namespace

hipError_t dn_launch_lstm_forward(const DnLstmArgs &a, hipStream_t stream)
{
    if (!ls_args_ok(a)) return hipErrorInvalidValue;
    const DnLstmLayout lay = dn_lstm_layout(a.in_dim, a.hidden, a.T, a.B);
    const int H = a.hidden;
    LsCellArgs cell = ls_cell_args(a, lay);
    const unsigned cell_blocks = (unsigned)((a.B * H + MT_THREADS - 1) / MT_THREADS);
    LsGemm g = ls_common(a);
    g.w_ih = a.w_ih; g.w_hh = a.w_hh; g.b_ih = a.b_ih; g.b_hh = a.b_hh;
    g.M = a.B; g.N = 4 * H; g.K = a.in_dim + H;         // N >= 128: the one tile shape
    for (long long t = 0; t < a.T; ++t) {
        g.row_base = t * a.B;
        g.C = cell.gates + g.row_base * 4 * H;
        hipLaunchKernelGGL((ls_forward_kernel<2, 2, 2, 2>), (ls_grid<2, 2, 2, 2>(g.M, g.N, 1)), dim3(MT_THREADS), 0, stream, g);
        cell.t = t;
        hipLaunchKernelGGL(ls_cell_forward_kernel, dim3(cell_blocks), dim3(MT_THREADS), 0, stream, cell);
    }
    return hipGetLastError();
}

hipError_t dn_launch_lstm_backward(const DnLstmArgs &a, hipStream_t stream)
{
    if (!ls_args_ok(a)) return hipErrorInvalidValue;
    const DnLstmLayout lay = dn_lstm_layout(a.in_dim, a.hidden, a.T, a.B);
    const int H = a.hidden, I = a.in_dim;
    LsCellArgs cell = ls_cell_args(a, lay);
    const unsigned cell_blocks = (unsigned)((a.B * H + MT_THREADS - 1) / MT_THREADS);
    for (long long t = a.T - 1; t >= 0; --t) {
        cell.t = t;
        hipLaunchKernelGGL(ls_cell_backward_kernel, dim3(cell_blocks), dim3(MT_THREADS), 0, stream, cell);
        if (t > 0) {                                   // carry_h = keep ? dZ_t W_hh : +0.0, for step t - 1
            LsGemm g = ls_common(a);
            g.A = cell.gates + t * a.B * 4 * H; g.W = a.w_hh; g.C = cell.carry_h;
            g.mask = a.episode_starts ? a.episode_starts + t * a.B : nullptr;
            g.M = a.B; g.N = H; g.K = 4 * H;
            ls_dgrad(g, stream);
        }
    }
    if (a.d_x) {                                       // d_x = dZ W_ih over all T B rows
        LsGemm g = ls_common(a);
        g.A = cell.gates; g.W = a.w_ih; g.C = a.d_x;
        g.M = a.T * a.B; g.N = I; g.K = 4 * H;
        ls_dgrad(g, stream);
    }
    if (!(a.flags & DN_MLP_TRAIN_NO_PARAM_GRADS)) {    // [d_w_ih | d_w_hh] = dZ^T (x | hprev) over all T B rows; M = 4H >= 128, N = I + H > 32
        LsGemm g = ls_common(a);
        g.A = cell.gates; g.C = reinterpret_cast<float *>(a.scratch + lay.wpart);
        g.bpart = reinterpret_cast<double *>(a.scratch + lay.bpart);
        g.M = 4 * H; g.N = I + H; g.rows = a.T * a.B;
        hipLaunchKernelGGL((ls_wgrad_kernel<2, 2, 2, 2>), (ls_grid<2, 2, 2, 2>(g.M, g.N, lay.chunks)), dim3(MT_THREADS), 0, stream, g);
        const LsMerge mg = {g.C, g.bpart, a.d_w_ih, a.d_w_hh, a.d_b_ih, a.d_b_hh, I, H, (int)lay.chunks, (a.flags & DN_MLP_TRAIN_ACCUMULATE) != 0};
        const int elements = 4 * H * (I + H) + 4 * H;
        hipLaunchKernelGGL(ls_merge_kernel, dim3((unsigned)((elements + MT_THREADS - 1) / MT_THREADS)), dim3(MT_THREADS), 0, stream, mg);
    }
    return hipGetLastError();
}
