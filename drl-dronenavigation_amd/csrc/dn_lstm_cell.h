// dn_lstm_cell.h -- the pointwise arithmetic of one LSTM cell, stated once for dn_lstm.hip: the gate activations of the forward
// product's epilogue, the cell update, and the backward through both.  Float32 throughout; the units that include this are compiled
// without contraction, so every operation below rounds on its own.  Include after dn_mt_gemm.h (mt_tanh).
//   forward   i = sig(z_i), f = sig(z_f), g = tanh(z_g), o = sig(z_o);  c = f cp + i g;  h = o tanh(c)
//   backward  dh = d_h + carry_h;  tc = tanh(c) (the forward's bits);  dc = carry_c + dh o (1 - tc tc)
//             dz_i = dc g i (1 - i), dz_f = dc cp f (1 - f), dz_g = dc i (1 - g g), dz_o = dh tc o (1 - o);  carry_c' = dc f
// The products are taken left to right as written.
#pragma once

namespace {

// 1 / (1 + 2^(-log2(e) z)) on v_exp_f32 and v_rcp_f32: 0 for z -> -inf (2^+inf = inf, 1 / inf = 0), 1 for z -> +inf
__device__ __forceinline__ float ls_sigmoid(const float z)
{
    const float e = __builtin_amdgcn_exp2f(z * -1.4426950408889634f);
    return __builtin_amdgcn_rcpf(1.0f + e);
}

// The activation of column n of the 4 H gate columns, torch's order i, f, g, o: tanh for g, the sigmoid for the others.
__device__ __forceinline__ float ls_gate(const float z, const int n, const int hidden)
{
    return n >= 2 * hidden && n < 3 * hidden ? mt_tanh(z) : ls_sigmoid(z);
}

struct LsCell {
    float c, h;
};
__device__ __forceinline__ LsCell ls_cell_forward(const float i, const float f, const float g, const float o, const float cp)
{
    LsCell r;
    r.c = f * cp + i * g;
    r.h = o * mt_tanh(r.c);
    return r;
}

struct LsCellGrad {
    float dz_i, dz_f, dz_g, dz_o, carry_c;             // carry_c: before the mask of the step's episode start
};
__device__ __forceinline__ LsCellGrad ls_cell_backward(const float i, const float f, const float g, const float o, const float c, const float cp,
                                                       const float d_h, const float carry_h, const float carry_c)
{
    const float dh = d_h + carry_h;
    const float tc = mt_tanh(c);
    const float dc = carry_c + dh * o * (1.0f - tc * tc);
    LsCellGrad r;
    r.dz_i = dc * g * i * (1.0f - i);
    r.dz_f = dc * cp * f * (1.0f - f);
    r.dz_g = dc * i * (1.0f - g * g);
    r.dz_o = dh * tc * o * (1.0f - o);
    r.carry_c = dc * f;
    return r;
}

}  // namespace
