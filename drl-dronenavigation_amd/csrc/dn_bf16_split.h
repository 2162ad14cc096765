// dn_bf16_split.h -- the two-word bfloat16 split of a float32 that the training pass of the Tanh networks (dn_mlp_train.hip) applies to
// both operands of every matrix product, stated once for host and device.  tests/tools/check_bf16_split.cpp pins it on the host.
//
//   hi = bf16(x)            round to nearest, ties to even
//   lo = bf16(x - hi)       the float32 difference is exact (Sterbenz-like: hi shares x's leading bits), then rounded the same way
// so x = hi + lo + r with |r| <= 2^-16 |x| for |x| >= 2^-118: |x - hi| <= 2^-8 |x| (half a unit of bf16's 8-bit significand), and lo
// loses at most 2^-8 of that again.  bf16 has float32's exponent range, so below 2^-118 lo is on the subnormal grid of spacing 2^-133
// and |r| <= 2^-134 instead.  A product a b is then taken as hi hi + hi lo + lo hi (three MFMAs into one float32 accumulator); the
// dropped lo lo term is at most 2^-16 |a b|.
//
// Special values, which the callers do not treat specially:
//   +-0                     hi = +-0, lo = +0
//   subnormal float32       hi is the nearest bf16 subnormal (a multiple of 2^-133, possibly 0), lo the rest rounded likewise; the
//                           remainder is at most 2^-134 in magnitude, absolutely, not relative to x
//   |x| >= 2^128 - 2^119    (the largest 2^15 finite float32 of either sign) hi rounds to +-infinity and lo = x - hi = -+infinity:
//                           the three-term product is NaN.  Weights and activations of these networks are nowhere near.
//   +-infinity              hi = +-infinity, lo = NaN (infinity - infinity)
//   NaN                     hi and lo are quiet NaNs
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIP__)                                   // a HIP unit: the host pass must see the device functions' callees too
#define DN_SPLIT_FN __host__ __device__ static inline
#else
#define DN_SPLIT_FN static inline
#endif

// The bits of bf16(x), round to nearest even; a NaN keeps its sign and top payload bits and is made quiet.
DN_SPLIT_FN uint16_t dn_bf16_rne_bits(const float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const __bf16 b = (__bf16)x;                        // v_cvt_pk_bf16_f32: the same rounding in one instruction
    return __builtin_bit_cast(unsigned short, b);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
#endif
}

// A bf16 word widened to float32: exact.
DN_SPLIT_FN float dn_bf16_widen(const uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// Two values at once as the kernels store them: element 0 in the low half of each dword.  The same bits as two dn_bf16_split calls; on
// the device the pair form is one v_cvt_pk_bf16_f32 per dword.
DN_SPLIT_FN void dn_bf16_split_pair(const float a, const float b, uint32_t *hi, uint32_t *lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __bf16 dn_bf16x2 __attribute__((ext_vector_type(2)));
    dn_bf16x2 h, l;
    h[0] = (__bf16)a;
    h[1] = (__bf16)b;
    const uint32_t hb = __builtin_bit_cast(unsigned, h);
    l[0] = (__bf16)(a - __builtin_bit_cast(float, hb << 16));
    l[1] = (__bf16)(b - __builtin_bit_cast(float, hb & 0xffff0000u));
    *hi = hb;
    *lo = __builtin_bit_cast(unsigned, l);
#else
    const uint16_t ha = dn_bf16_rne_bits(a), hb = dn_bf16_rne_bits(b);
    *hi = (uint32_t)ha | ((uint32_t)hb << 16);
    *lo = (uint32_t)dn_bf16_rne_bits(a - dn_bf16_widen(ha)) | ((uint32_t)dn_bf16_rne_bits(b - dn_bf16_widen(hb)) << 16);
#endif
}

// x -> (hi, lo) as bf16 bit patterns.
DN_SPLIT_FN void dn_bf16_split(const float x, uint16_t *hi, uint16_t *lo)
{
    const uint16_t h = dn_bf16_rne_bits(x);
    *hi = h;
    *lo = dn_bf16_rne_bits(x - dn_bf16_widen(h));
}
