// head_norm.hip -- per-head normalisation of q / k rows (head_norm.h) as launches of its own, + their C ABI.
//
// Reference: head_norm_cuda (head_norm.cu:143-168: a block of head_dim / 2 threads per (row, head), warp-32 shuffles + LDS) as
// ext_norm.cpp:159-212 and q_attn.cu:285-289 call it.  Here ONE kernel, three entry points:
//   exl2_head_norm       x [rows, heads, head_dim] -> y (in place when y == x), optional fp16 bias added afterwards;
//   exl2_head_norm_qk    q and k rows of a step in one grid (the reference: two launches);
//   exl2_head_norm_rope_qk  the same followed by RoPE on the fp16-rounded result (the reference: three launches, q_attn.cu:285-310) --
//                        bit for bit exl2_head_norm then exl2_rope_qk.
// A head sits in GW = 8 / 16 / 32 adjacent lanes (8 fp16 = 16 bytes per lane), 256 / GW heads per workgroup, no LDS: the kernel is
// two 16-byte loads, one 16-byte store and a handful of cross-lane adds per lane -- launch-latency bound at decode sizes.
#include "head_norm.h"
#include "errors.h"
#include <string.h>

struct HeadNormArgs
{
    // segment 0 (q, or the only one) and segment 1 (k; n1 = 0: absent): n head rows each, laid out [batch, rows_pb, head_dim]
    const f16* x0; const f16* x1; f16* y0; f16* y1;
    const f16* w0; const f16* w1; const f16* b0; const f16* b1;      // [heads, head_dim]; bias nullable
    int n0, n1, heads0, heads1;
    int rows_pb0, rows_pb1;                                          // head rows per batch entry (RoPE positions)
    int head_dim, rms;
    float eps, r_dim;
    // RoPE behind the norm (sin == nullptr: none); exl2_rope_qk's arguments
    const f16* sin; const f16* cos; const int* past_lens;
    int past_len, neox, sincos_size;
};

template <int GW>
KERNEL void __launch_bounds__(256) head_norm_kernel(const HeadNormArgs a)
{
    constexpr int HPW = 256 / GW;                                    // heads per workgroup
    const int dl = tid() % GW;
    const long long hr_all = (long long)bid_x() * HPW + tid() / GW;
    const bool seg1 = hr_all >= a.n0;
    const int hr = (int)(seg1 ? hr_all - a.n0 : hr_all);
    const int n = seg1 ? a.n1 : a.n0;
    const int heads = seg1 ? a.heads1 : a.heads0;
    const bool active = hr < n && dl * 8 < a.head_dim;               // (no lane leaves: every lane of a wave takes part in the exchanges)
    const f16* const x = seg1 ? a.x1 : a.x0;
    f16* const y = seg1 ? a.y1 : a.y0;
    const f16* const w = seg1 ? a.w1 : a.w0;
    const f16* const bias = seg1 ? a.b1 : a.b0;
    const int head = active ? hr % heads : 0;
    const size_t xo = active ? (size_t)hr * a.head_dim + dl * 8 : 0;
    const size_t wo = (size_t)head * a.head_dim + (active ? dl * 8 : 0);

    const f16x8 z8 = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f};
    f16x8 xv = z8, wv = z8;
    if (active) { xv = *(const f16x8*)(x + xo); wv = *(const f16x8*)(w + wo); }
    f16x8 o = head_norm_frag<GW>(xv, wv, a.eps, a.r_dim, a.rms != 0, active);
    if (active && bias) o = o + *(const f16x8*)(bias + wo);          // __hadd2(nh, b) (head_norm.cu:76)

    if (a.sin)
    {
        // rope_rows (elementwise.hip) on the rounded values: same operands, same packed fp16 operations
        const int rows_pb = seg1 ? a.rows_pb1 : a.rows_pb0;
        const int bi = active ? hr / rows_pb : 0;
        const int row = active ? hr - bi * rows_pb : 0;
        int past = a.past_len;
        if (past == -1) { past = a.past_lens[bi]; past = past > 0 ? past : 0; }
        else if (a.past_lens) past += a.past_lens[bi];
        int srow = past + row / heads;
        srow = srow > 0 ? srow : 0;
        const f16* const sr = a.sin + (size_t)srow * a.sincos_size;
        const f16* const cr = a.cos + (size_t)srow * a.sincos_size;
        if (a.neox)
        {
            // columns c < half pair with c + half: the partner's 8 columns sit HL lanes away (host: sincos_size % 16 == 0)
            const int HL = a.sincos_size >> 4;
            const bool rot = active && dl < 2 * HL;
            const int lane = lane_id();
            const int src = rot ? (dl < HL ? lane + HL : lane - HL) : lane;
            u32x4 u = __builtin_bit_cast(u32x4, o), pu;
            #pragma unroll
            for (int i = 0; i < 4; i++) pu[i] = shfl_idx_u32(u[i], src);
            if (rot)
            {
                const int col = (dl < HL ? dl : dl - HL) * 8;
                const f16x8 cs = *(const f16x8*)(cr + col);
                f16x8 sn = *(const f16x8*)(sr + col);
                if (dl < HL) sn = -sn;                               // l' = l cos + r (-sin); r' = r cos + l sin
                const f16x8 partner = __builtin_bit_cast(f16x8, pu);
                const f16x8 t = partner * sn;
                #pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const f16x2 v = h2_fma((f16x2){o[2 * i], o[2 * i + 1]}, (f16x2){cs[2 * i], cs[2 * i + 1]}, (f16x2){t[2 * i], t[2 * i + 1]});
                    o[2 * i] = v.x; o[2 * i + 1] = v.y;
                }
            }
        }
        else if (active && dl * 8 + 8 <= a.sincos_size)
        {
            // GPT-J pairs (2i, 2i + 1) (host: sincos_size % 8 == 0)
            const f16x8 cs = *(const f16x8*)(cr + dl * 8);
            const f16x8 sn = *(const f16x8*)(sr + dl * 8);
            #pragma unroll
            for (int i = 0; i < 4; i++)
            {
                const f16x2 c01 = {cs[2 * i], cs[2 * i + 1]};
                const f16x2 s01 = {-sn[2 * i], sn[2 * i + 1]};
                const f16x2 x01 = {o[2 * i], o[2 * i + 1]};
                const f16x2 x10 = {x01.y, x01.x};
                const f16x2 v = h2_fma(x10, s01, x01 * c01);
                o[2 * i] = v.x; o[2 * i + 1] = v.y;
            }
        }
    }
    if (active) *(f16x8*)(y + xo) = o;
}

static int head_norm_launch(const HeadNormArgs& a, void* stream)
{
    const long long total = (long long)a.n0 + a.n1;
    if (total <= 0) return EXL2_OK;
    const int gw = a.head_dim <= 64 ? 8 : (a.head_dim <= 128 ? 16 : 32);
    const long long wgs = (total + 256 / gw - 1) / (256 / gw);
    EXL2_REQUIRE(wgs <= 0x7fffffffLL, "head_norm: %lld head rows", total);
    if (gw == 8) LAUNCH(head_norm_kernel<8>, dim3((unsigned)wgs), dim3(256), 0, stream, a);
    else if (gw == 16) LAUNCH(head_norm_kernel<16>, dim3((unsigned)wgs), dim3(256), 0, stream, a);
    else LAUNCH(head_norm_kernel<32>, dim3((unsigned)wgs), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

static bool aligned16(const void* p) { return (((size_t)p) & 15) == 0; }

extern "C" {

int exl2_rope_qk(void* x_q, void* x_k, const void* sin, const void* cos, int batch_size,
                 int rows_per_batch_q, int rows_per_batch_k, int head_dim, int num_heads_q, int num_heads_k,
                 int past_len, const int* past_lens, int neox_style, int sincos_size, void* stream);

// head_norm / head_norm_ (ext_norm.cpp:159-212 -> head_norm_cuda): y = norm(x) * w (+ b); y == x: in place
int exl2_head_norm(const void* x, const void* w, const void* b, void* y, float epsilon, int rms, int rows, int num_heads,
                   int head_dim, void* stream)
{
    EXL2_REQUIRE(x && w && y, "head_norm: null argument");
    EXL2_REQUIRE(head_dim > 0 && head_dim % 8 == 0 && head_dim <= HEAD_NORM_MAX_DIM, "head_norm: head_dim %d must be a multiple of 8 up to %d", head_dim, HEAD_NORM_MAX_DIM);
    EXL2_REQUIRE(num_heads > 0, "head_norm: %d heads", num_heads);
    EXL2_REQUIRE(aligned16(x) && aligned16(w) && aligned16(b) && aligned16(y), "head_norm: tensors must be 16-byte aligned");
    if (rows <= 0) return EXL2_OK;
    EXL2_REQUIRE((long long)rows * num_heads <= 0x7fffffffLL, "head_norm: %d rows of %d heads", rows, num_heads);
    HeadNormArgs a; memset(&a, 0, sizeof(a));
    a.x0 = (const f16*)x; a.y0 = (f16*)y; a.w0 = (const f16*)w; a.b0 = (const f16*)b;
    a.n0 = rows * num_heads; a.heads0 = num_heads; a.heads1 = 1; a.rows_pb0 = a.rows_pb1 = 1;
    a.head_dim = head_dim; a.rms = rms; a.eps = epsilon; a.r_dim = 1.0f / (float)head_dim;
    return head_norm_launch(a, stream);
}

static int head_norm_qk_args(HeadNormArgs& a, void* q, void* k, const void* q_norm, const void* k_norm, float epsilon, int rms,
                             int batch_size, int rows_per_batch_q, int rows_per_batch_k, int head_dim, int num_heads_q, int num_heads_k)
{
    EXL2_REQUIRE(q && k && q_norm && k_norm, "head_norm_qk: null argument");
    EXL2_REQUIRE(head_dim > 0 && head_dim % 8 == 0 && head_dim <= HEAD_NORM_MAX_DIM, "head_norm_qk: head_dim %d must be a multiple of 8 up to %d", head_dim, HEAD_NORM_MAX_DIM);
    EXL2_REQUIRE(num_heads_q > 0 && num_heads_k > 0 && rows_per_batch_q % num_heads_q == 0 && rows_per_batch_k % num_heads_k == 0,
                 "head_norm_qk: rows per batch (%d, %d) are not whole tokens of (%d, %d) heads", rows_per_batch_q, rows_per_batch_k, num_heads_q, num_heads_k);
    EXL2_REQUIRE(aligned16(q) && aligned16(k) && aligned16(q_norm) && aligned16(k_norm), "head_norm_qk: tensors must be 16-byte aligned");
    EXL2_REQUIRE((long long)batch_size * ((long long)rows_per_batch_q + rows_per_batch_k) <= 0x7fffffffLL, "head_norm_qk: too many head rows");
    memset(&a, 0, sizeof(a));
    a.x0 = (const f16*)q; a.y0 = (f16*)q; a.w0 = (const f16*)q_norm;
    a.x1 = (const f16*)k; a.y1 = (f16*)k; a.w1 = (const f16*)k_norm;
    a.n0 = batch_size * rows_per_batch_q; a.n1 = batch_size * rows_per_batch_k;
    a.heads0 = num_heads_q; a.heads1 = num_heads_k; a.rows_pb0 = rows_per_batch_q; a.rows_pb1 = rows_per_batch_k;
    a.head_dim = head_dim; a.rms = rms; a.eps = epsilon; a.r_dim = 1.0f / (float)head_dim;
    return EXL2_OK;
}

// q [batch, rows_per_batch_q, head_dim] with q_norm [num_heads_q, head_dim] and k likewise, in place, one launch (no bias: q_attn.cu:285-289)
int exl2_head_norm_qk(void* q, void* k, const void* q_norm, const void* k_norm, float epsilon, int rms, int batch_size,
                      int rows_per_batch_q, int rows_per_batch_k, int head_dim, int num_heads_q, int num_heads_k, void* stream)
{
    if (batch_size <= 0) return EXL2_OK;
    HeadNormArgs a;
    const int rc = head_norm_qk_args(a, q, k, q_norm, k_norm, epsilon, rms, batch_size, rows_per_batch_q, rows_per_batch_k, head_dim, num_heads_q, num_heads_k);
    if (rc) return rc;
    return head_norm_launch(a, stream);
}

// the same + RoPE (exl2_rope_qk's arguments and numerics) in one launch.  The rotation partner of a lane's 8 columns must be another
// lane's 8 columns: NeoX with sincos_size % 16 == 0, GPT-J with sincos_size % 8 == 0 -- any other table runs as the two launches.
int exl2_head_norm_rope_qk(void* q, void* k, const void* q_norm, const void* k_norm, float epsilon, int rms,
                           const void* sin, const void* cos, int batch_size, int rows_per_batch_q, int rows_per_batch_k, int head_dim,
                           int num_heads_q, int num_heads_k, int past_len, const int* past_lens, int neox_style, int sincos_size, void* stream)
{
    EXL2_REQUIRE(sin && cos, "head_norm_rope_qk: sin/cos tables missing");
    EXL2_REQUIRE(sincos_size > 0 && sincos_size % 4 == 0 && sincos_size <= head_dim, "head_norm_rope_qk: bad sincos_size %d", sincos_size);
    EXL2_REQUIRE(past_len != -1 || past_lens, "head_norm_rope_qk: past_len == -1 needs past_lens");
    if (batch_size <= 0) return EXL2_OK;
    HeadNormArgs a;
    const int rc = head_norm_qk_args(a, q, k, q_norm, k_norm, epsilon, rms, batch_size, rows_per_batch_q, rows_per_batch_k, head_dim, num_heads_q, num_heads_k);
    if (rc) return rc;
    if (sincos_size % (neox_style ? 16 : 8) != 0 || !aligned16(sin) || !aligned16(cos))
    {
        const int rc2 = head_norm_launch(a, stream);
        if (rc2) return rc2;
        return exl2_rope_qk(q, k, sin, cos, batch_size, rows_per_batch_q, rows_per_batch_k, head_dim, num_heads_q, num_heads_k,
                            past_len, past_lens, neox_style, sincos_size, stream);
    }
    a.sin = (const f16*)sin; a.cos = (const f16*)cos; a.past_lens = past_lens;
    a.past_len = past_len; a.neox = neox_style; a.sincos_size = sincos_size;
    return head_norm_launch(a, stream);
}

}  // extern "C"
