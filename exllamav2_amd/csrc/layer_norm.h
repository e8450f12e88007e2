// layer_norm.h -- LayerNorm of one fp16 row held in a workgroup's registers, as ONE device routine.
//
// Reference: layer_norm_kernel (layer_norm.cu:31-159).  Its rounding points, kept here:
//   every element widened to fp32 and clamped to +-65504;
//   mean = sum * (1 / dim), an fp32 number;
//   d = x - mean in fp32; the variance comes from the sum of the squared CENTRED values (never E[x^2] - mean^2: a row with a large mean
//   and a small spread loses every bit of the spread that way);
//   rsvar = rsqrt(sum * (1 / dim) + eps), an fp32 number;
//   y = fp16_rn((d * w) * rsvar), two fp32 products in that order; an optional bias and an optional residual are fp16 adds on the
//   rounded value, in that order.
// The two sums: the reference adds them up in fp32, 1024 threads with 2 columns each per pass, in an order of its own.  An element that
// sits next to the mean carries every bit of the row sum's rounding into its result, so two orders of the same fp32 sum disagree there
// by many fp16 ulps -- with each other and with a float64 restatement.  Here both sums are ACCUMULATED in fp64 and the mean and rsvar
// rounded to fp32 once: the row sum is exact (fp16 terms are multiples of 2^-24 below 2^16, at most 16384 of them), the sum of squares
// is good to 2^-50, so the results do not depend on which thread holds which column and agree with the float64 restatement wherever that
// one's own last fp64 bit does not decide an fp32 rounding.  Cost: 16 fp64 operations per octet and two butterflies of 64-bit values in
// a kernel that waits for memory.
// 256 threads hold 8 columns (16 bytes) per pass, thread t the octets t, t + 256, ..., K of them.  Both kernels of layer_norm.hip go
// through these routines: their results agree bit for bit.
#pragma once
#include "hw.h"

#define LAYER_NORM_MAX_K 8
#define LAYER_NORM_MAX_DIM (256 * 8 * LAYER_NORM_MAX_K)          // 16384

DEV float layer_norm_clampf(float f) { return fmaxf(-65504.0f, fminf(f, 65504.0f)); }

// value held by lane (lane ^ mask): the two halves of the 64-bit value move separately
DEV double layer_norm_shfl_xor_f64(double v, int mask)
{
    const u64 b = __builtin_bit_cast(u64, v);
    const u32 lo = shfl_xor_u32((u32)b, mask), hi = shfl_xor_u32((u32)(b >> 32), mask);
    return __builtin_bit_cast(double, ((u64)hi << 32) | lo);
}

// sum over the 256 threads: butterfly inside each wave (registers), the four wave sums through `part` (one LDS exchange); every thread
// of the workgroup calls, each call with a `part` of its own
DEV double layer_norm_block_sum_f64(double s, double* part)
{
    #pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += layer_norm_shfl_xor_f64(s, m);
    if (lane_id() == 0) part[wave_id()] = s;
    block_sync();
    return part[0] + part[1] + part[2] + part[3];
}

// widen + clamp this thread's octet
DEV void layer_norm_widen(const f16x8 v, float (&f)[8])
{
    #pragma unroll
    for (int e = 0; e < 8; e++) f[e] = layer_norm_clampf((float)v[e]);
}

// f: the clamped values of octets tid() + 256 k (zeros where that octet is beyond dim8); on return the centred values.  Returns rsvar.
template <int K>
DEV float layer_norm_centre(float (&f)[K][8], const int dim8, const float r_dim, const float eps, double* part_sum, double* part_sq)
{
    const int t = tid();
    double s = 0.0;
    #pragma unroll
    for (int k = 0; k < K; k++)
        if (t + 256 * k < dim8)
        {
            #pragma unroll
            for (int e = 0; e < 8; e++) s += (double)f[k][e];
        }
    const float mean = (float)(layer_norm_block_sum_f64(s, part_sum) * (double)r_dim);
    double ss = 0.0;
    #pragma unroll
    for (int k = 0; k < K; k++)
        if (t + 256 * k < dim8)
        {
            #pragma unroll
            for (int e = 0; e < 8; e++) { f[k][e] -= mean; ss = fma((double)f[k][e], (double)f[k][e], ss); }
        }
    ss = layer_norm_block_sum_f64(ss, part_sq);
    return (float)(1.0 / sqrt(ss * (double)r_dim + (double)eps));
}

// (d * w) * rsvar, rounded to nearest fp16
DEV f16x8 layer_norm_scale(const float (&d)[8], const f16x8 w, const float rsvar)
{
    f16x8 y;
    #pragma unroll
    for (int e = 0; e < 8; e++) y[e] = (f16)((d[e] * (float)w[e]) * rsvar);
    return y;
}
