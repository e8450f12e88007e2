// gemma_ops.hip -- what an fp32 residual stream (Gemma-2 / Gemma-3: architecture.py:576, :601) adds next to elementwise.hip:
// the norm bridge, the logit soft cap and the scaled fp32 embedding gather, + their C ABI.
//
// Reference: rms_norm.cu:33-175 (numerics, as rms_norm_kernel of elementwise.hip restates them), softcap.cu:8-64,
// embedding.py:184-187.  All three are HBM / launch-latency bound: 16-byte accesses, one pass.
#include "hw.h"
#include "errors.h"

// ---- norm bridge ------------------------------------------------------------------------------------------------------
// The two norms that meet at a module boundary of an fp32-residual block, in one launch:
//   x += rmsnorm(t) * w_post      exl2_rms_norm(t, w_post, x, eps, rows, dim, 1, 0, 1), bit for bit: the same clamp of the fp16
//                                 input, the same thread <-> octet mapping and order of the sum of squares, (t * w) * r and the add
//                                 as separate fp32 roundings
//   n  = rmsnorm(x) * w_next      fp16, the contract of exl2_rms_norm(x, w_next, n, eps, rows, dim, 0, 1, 0); its sum of squares runs
//                                 in THIS kernel's mapping (thread t: octets t, t + 256, ...), rms_norm_kernel walks fp32 rows as
//                                 f32x4 vectors, so n may differ from that launch by fp32 sum order
// One 256-thread workgroup per row; thread t keeps octets t + 256 k, k < K, of the row in registers between the halves: x is read
// once, written once and never re-read.  K <= NORM_BRIDGE_MAX_K, i.e. dim <= NORM_BRIDGE_MAX_DIM; the host reports wider rows as
// "not covered" and the caller issues the two launches.  n may alias t: a thread has read its octets of t before it writes them.
#define NORM_BRIDGE_MAX_K 4
#define NORM_BRIDGE_MAX_DIM (256 * 8 * NORM_BRIDGE_MAX_K)          // 8192

struct BridgeArgs
{
    const f16* t; float* x; const f16* w_post; const f16* w_next; f16* n;
    float eps, r_dim;
    int dim;
};

DEV float bridge_clampf(float f) { return fmaxf(-65504.0f, fminf(f, 65504.0f)); }

DEV float bridge_block_sum(float ss, float* part)
{
    ss = wave_allreduce_add(ss);
    if (lane_id() == 0) part[wave_id()] = ss;
    block_sync();
    return part[0] + part[1] + part[2] + part[3];
}

template <int K>
KERNEL void __launch_bounds__(256) norm_bridge_kernel(const BridgeArgs a)
{
    SHARED float part1[4];
    SHARED float part2[4];
    const int row = bid_x();
    const int t = tid();
    const int dim8 = a.dim >> 3;          // host guarantees dim % 8 == 0 and dim8 <= 256 K

    const f16x8* tr = (const f16x8*)(a.t + (size_t)row * a.dim);
    f32x4* xr = (f32x4*)(a.x + (size_t)row * a.dim);
    f16x8 tv[K];
    f32x4 x0[K], x1[K];
    float ss = 0.0f;
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8)
        {
            tv[k] = tr[i];
            x0[k] = xr[2 * i]; x1[k] = xr[2 * i + 1];
            #pragma unroll
            for (int e = 0; e < 8; e++) { const float f = bridge_clampf((float)tv[k][e]); ss = fmaf(f, f, ss); }
        }
    }
    ss = bridge_block_sum(ss, part1);
    const float rmf = fast_rsqrt(ss * a.r_dim + a.eps);

    const f16x8* wp = (const f16x8*)a.w_post;
    float ss2 = 0.0f;
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8)
        {
            // (t * w) * r and the add are the three roundings rms_norm_kernel makes: here the product has no other reader, so keep the
            // compiler from contracting it into the add (the fmaf sums below stay fmaf; the rsqrt arguments are left to it, as there)
            #pragma clang fp contract(off)
            const f16x8 w8 = wp[i];
            float nv[8];
            #pragma unroll
            for (int e = 0; e < 8; e++) nv[e] = bridge_clampf((float)tv[k][e]) * (float)w8[e] * rmf;
            const f32x4 n0 = {nv[0], nv[1], nv[2], nv[3]}, n1 = {nv[4], nv[5], nv[6], nv[7]};
            x0[k] = n0 + x0[k]; x1[k] = n1 + x1[k];
            xr[2 * i] = x0[k]; xr[2 * i + 1] = x1[k];
            #pragma unroll
            for (int e = 0; e < 4; e++) ss2 = fmaf(x0[k][e], x0[k][e], ss2);      // fp32 input is not clamped (rms_norm.cu:92-99)
            #pragma unroll
            for (int e = 0; e < 4; e++) ss2 = fmaf(x1[k][e], x1[k][e], ss2);
        }
    }
    if (!a.w_next) return;                 // (uniform over the launch)
    ss2 = bridge_block_sum(ss2, part2);
    const float rmf2 = fast_rsqrt(ss2 * a.r_dim + a.eps);

    const f16x8* wn = (const f16x8*)a.w_next;
    f16x8* nr = (f16x8*)(a.n + (size_t)row * a.dim);
    #pragma unroll
    for (int k = 0; k < K; k++)
    {
        const int i = t + 256 * k;
        if (i < dim8)
        {
            const f16x8 w8 = wn[i];
            f16x8 o;
            #pragma unroll
            for (int e = 0; e < 4; e++)
            {
                o[e]     = (f16)(x0[k][e] * (float)w8[e] * rmf2);
                o[4 + e] = (f16)(x1[k][e] * (float)w8[4 + e] * rmf2);
            }
            nr[i] = o;
        }
    }
}

// ---- soft cap -----------------------------------------------------------------------------------------------------------
// x = cap * tanhf(x / cap) in place (softcap.cu:8-64): a division, tanhf and a product in fp32; fp16 goes through fp32 and is rounded
// to nearest.  Elements [head, head + 16 nvec bytes) are 16-byte vectors; the up to 7 + 7 elements in front of the first aligned
// address and behind the last whole vector are done one by one by workgroup 0 -- every element of [0, numel), nothing beyond.

DEV float softcap_f(float v, float cap) { return tanhf(v / cap) * cap; }

template <bool FP32>
KERNEL void __launch_bounds__(256) softcap_kernel(void* x_, long long numel, float cap, int head, long long nvec)
{
    const long long i = (long long)bid_x() * 256 + tid();
    if constexpr (FP32)
    {
        float* x = (float*)x_;
        if (i < nvec)
        {
            f32x4* p = (f32x4*)(x + head) + i;
            f32x4 v = *p;
            #pragma unroll
            for (int e = 0; e < 4; e++) v[e] = softcap_f(v[e], cap);
            *p = v;
        }
        if (bid_x() == 0)
        {
            const long long tail0 = head + nvec * 4;
            if (tid() < head) x[tid()] = softcap_f(x[tid()], cap);
            else if (tid() >= 64 && tail0 + (tid() - 64) < numel) x[tail0 + (tid() - 64)] = softcap_f(x[tail0 + (tid() - 64)], cap);
        }
    }
    else
    {
        f16* x = (f16*)x_;
        if (i < nvec)
        {
            f16x8* p = (f16x8*)(x + head) + i;
            f16x8 v = *p;
            #pragma unroll
            for (int e = 0; e < 8; e++) v[e] = (f16)softcap_f((float)v[e], cap);
            *p = v;
        }
        if (bid_x() == 0)
        {
            const long long tail0 = head + nvec * 8;
            if (tid() < head) x[tid()] = (f16)softcap_f((float)x[tid()], cap);
            else if (tid() >= 64 && tail0 + (tid() - 64) < numel) x[tail0 + (tid() - 64)] = (f16)softcap_f((float)x[tail0 + (tid() - 64)], cap);
        }
    }
}

// ---- scaled fp32 embedding ----------------------------------------------------------------------------------------------
// out[r] = float(table[ids[r]]) * scale: `.float()` then `*= hidden_size ** 0.5` (embedding.py:184-187), one fp32 multiply per
// element; ids are clamped to the table as embed_rows_kernel clamps them

KERNEL void __launch_bounds__(256) embed_rows_f32_kernel(const f16* table, const int* ids, float* out, int hidden, int vocab, float scale)
{
    const int row = bid_x();
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const f16x8* src = (const f16x8*)(table + (size_t)id * hidden);
    f32x4* dst = (f32x4*)(out + (size_t)row * hidden);
    for (int i = tid(); i < (hidden >> 3); i += 256)
    {
        const f16x8 v = src[i];
        const f32x4 o0 = {(float)v[0] * scale, (float)v[1] * scale, (float)v[2] * scale, (float)v[3] * scale};
        const f32x4 o1 = {(float)v[4] * scale, (float)v[5] * scale, (float)v[6] * scale, (float)v[7] * scale};
        dst[2 * i] = o0; dst[2 * i + 1] = o1;
    }
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------

extern "C" {

// returns 0 when launched, 1 when dim > NORM_BRIDGE_MAX_DIM ("not covered": nothing was launched, nothing is touched -- the caller runs
// exl2_rms_norm(t, w_post, x, .., 1, 0, 1) and exl2_rms_norm(x, w_next, n, .., 0, 1, 0))
int exl2_norm_bridge(const void* t, void* x, const void* w_post, const void* w_next, void* n, float epsilon, int rows, int dim,
                     void* stream)
{
    EXL2_REQUIRE(t && x && w_post, "norm_bridge: null argument");
    EXL2_REQUIRE(!w_next || n, "norm_bridge: w_next needs n");
    EXL2_REQUIRE(dim > 0 && dim % 8 == 0, "norm_bridge: dim %d must be a multiple of 8", dim);
    EXL2_REQUIRE(((((size_t)t) | ((size_t)x) | ((size_t)w_post) | ((size_t)w_next) | ((size_t)n)) & 15) == 0,
                 "norm_bridge: t / x / w_post / w_next / n must be 16-byte aligned");
    if (dim > NORM_BRIDGE_MAX_DIM) return 1;
    if (rows <= 0) return EXL2_OK;
    BridgeArgs a;
    a.t = (const f16*)t; a.x = (float*)x; a.w_post = (const f16*)w_post; a.w_next = (const f16*)w_next; a.n = (f16*)n;
    a.eps = epsilon; a.r_dim = 1.0f / (float)dim; a.dim = dim;
    const int k = ((dim >> 3) + 255) / 256;
    if (k <= 1)      LAUNCH(norm_bridge_kernel<1>, dim3((unsigned)rows), dim3(256), 0, stream, a);
    else if (k == 2) LAUNCH(norm_bridge_kernel<2>, dim3((unsigned)rows), dim3(256), 0, stream, a);
    else             LAUNCH(norm_bridge_kernel<NORM_BRIDGE_MAX_K>, dim3((unsigned)rows), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

int exl2_softcap(void* x, long long numel, float cap, int is_fp32, void* stream)
{
    EXL2_REQUIRE(x, "softcap: null argument");
    EXL2_REQUIRE(cap > 0.0f, "softcap: cap must be positive");
    const int esize = is_fp32 ? 4 : 2;
    EXL2_REQUIRE((((size_t)x) & (size_t)(esize - 1)) == 0, "softcap: x is not aligned to its element size");
    if (numel <= 0) return EXL2_OK;
    const int per = 16 / esize;
    long long head = (long long)(((16 - (((size_t)x) & 15)) & 15) / (size_t)esize);
    if (head > numel) head = numel;
    const long long nvec = (numel - head) / per;
    const long long blocks = nvec > 0 ? (nvec + 255) / 256 : 1;
    EXL2_REQUIRE(blocks <= 0x7fffffffLL, "softcap: %lld elements exceed one launch", numel);
    if (is_fp32) LAUNCH(softcap_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, x, numel, cap, (int)head, nvec);
    else         LAUNCH(softcap_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, x, numel, cap, (int)head, nvec);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

int exl2_embed_rows_f32(const void* table, const int* ids, void* out, int rows, int hidden, int vocab, float scale, void* stream)
{
    EXL2_REQUIRE(table && ids && out, "embed_rows_f32: null argument");
    EXL2_REQUIRE(hidden > 0 && hidden % 8 == 0, "embed_rows_f32: hidden %d must be a multiple of 8", hidden);
    EXL2_REQUIRE(vocab > 0, "embed_rows_f32: empty table");
    EXL2_REQUIRE(((((size_t)table) | ((size_t)out)) & 15) == 0, "embed_rows_f32: table / out must be 16-byte aligned");
    if (rows <= 0) return EXL2_OK;
    LAUNCH(embed_rows_f32_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (const f16*)table, ids, (float*)out, hidden, vocab, scale);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

}  // extern "C"
