// head_norm.h -- the per-head q / k normalisation (Qwen3, Gemma3, OLMo2, Cohere) as ONE device function.
//
// Reference: head_norm_kernel (head_norm.cu:9-141): every element widened to fp32 and clamped to +-65504; RMS form
// y = fp16_rn(x * w * rsqrt(mean(x^2) + eps)); LayerNorm form with d = x - mean(x) in place of x.  The reference runs a block per
// head with warp-32 shuffles and an LDS round; here a head is held as 8 fp16 per lane over GW adjacent lanes (the layout
// attn_fused_body.h uses for RoPE), the sums are an 8-term fp32 FMA chain per lane and a butterfly over the GW lanes.
// Every kernel that normalises a head -- head_norm.hip's launches and the NORM form of the one-launch decode attention -- calls
// head_norm_frag, and every multiply-add in it is spelled out, so their results agree bit for bit.
#pragma once
#include "hw.h"

#define HEAD_NORM_MAX_DIM 256

// all-reduce (sum) over each aligned group of GW lanes (8, 16 or 32)
template <int GW> DEV float head_norm_group_add(float v)
{
    static_assert(GW == 8 || GW == 16 || GW == 32, "a head spans 8, 16 or 32 lanes");
    if constexpr (GW == 8) return row8_allreduce_add(v);
    else if constexpr (GW == 16) return row16_allreduce_add(v);
    else { v = row16_allreduce_add(v); return v + as_f32(swz_xor_u32<16>(f32_bits(v))); }
}

// x, w: this lane's 8 features of the head and of the head's weight row; r_dim = 1 / head_dim.  `active` = false: a lane of the
// group beyond the head (head_dim / 8 is not the group width) -- it adds nothing to the sums, its result is unused.  Every lane
// of the wave calls (cross-lane exchange).
template <int GW> DEV f16x8 head_norm_frag(const f16x8 x, const f16x8 w, const float eps, const float r_dim, const bool rms, const bool active)
{
    float f[8];
    #pragma unroll
    for (int e = 0; e < 8; e++) f[e] = active ? fmaxf(-65504.0f, fminf((float)x[e], 65504.0f)) : 0.0f;
    if (!rms)
    {
        float s = 0.0f;
        #pragma unroll
        for (int e = 0; e < 8; e++) s += f[e];
        const float mean = head_norm_group_add<GW>(s) * r_dim;
        #pragma unroll
        for (int e = 0; e < 8; e++) f[e] = active ? f[e] - mean : 0.0f;
    }
    float ss = 0.0f;
    #pragma unroll
    for (int e = 0; e < 8; e++) ss = fmaf(f[e], f[e], ss);
    ss = head_norm_group_add<GW>(ss);
    const float r = fast_rsqrt(fmaf(ss, r_dim, eps));
    f16x8 y;
    #pragma unroll
    for (int e = 0; e < 8; e++) y[e] = (f16)((f[e] * (float)w[e]) * r);
    return y;
}
