// moe.hip -- MoE routing for the fused expert path: router logits and softmax -> top-k -> renormalise.
//
// Reference: QMoEMLP::forward_ (cuda/q_mlp.cu:318-436): cublasHgemm(temp_state, gate^T) then softmax{4,8,16}_topk_norm_kernel
// (cuda/q_mlp_softmax.cuh) rewrite the logits in place as routing weights (zero outside the top-k); the expert GEMVs
// read them through r_weights and skip zero-weight rows / exit when every row's weight is zero.
#include "hw.h"
#include "errors.h"
#include "moe.h"
#include <string.h>

// logits[r, e] = sum_k x[r, k] * gate[e, k]   (gate = nn.Linear weight [E, hidden]); one workgroup per row, fp32 sums
template <int E>
KERNEL void __launch_bounds__(256) moe_gate_kernel(const f16* x, const f16* gate, f16* logits, int hidden)
{
    SHARED float part[4 * E];
    const int r = bid_x();
    const int t = tid(), lane = lane_id(), wv = wave_id();
    float acc[E];
    #pragma unroll
    for (int e = 0; e < E; e++) acc[e] = 0.0f;
    const f16x8* xr = (const f16x8*)(x + (size_t)r * hidden);
    for (int i = t; i < (hidden >> 3); i += 256)
    {
        const f16x8 xv = xr[i];
        #pragma unroll
        for (int e = 0; e < E; e++)
        {
            const f16x8 gv = ((const f16x8*)(gate + (size_t)e * hidden))[i];
            #pragma unroll
            for (int j = 0; j < 4; j++)
                acc[e] = dot2_f32_f16((f16x2){xv[2 * j], xv[2 * j + 1]}, (f16x2){gv[2 * j], gv[2 * j + 1]}, acc[e]);
        }
    }
    #pragma unroll
    for (int e = 0; e < E; e++)
    {
        const float s = wave_allreduce_add(acc[e]);
        if (lane == 0) part[wv * E + e] = s;
    }
    block_sync();
    if (t < E) logits[(size_t)r * E + t] = (f16)(part[t] + part[E + t] + part[2 * E + t] + part[3 * E + t]);
}

// in place: softmax over E (q_mlp_softmax.cuh arithmetic incl. its epsilon), drop the E - topk smallest, renormalise
template <int E>
KERNEL void __launch_bounds__(64) moe_topk_kernel(f16* x, int rows, int topk)
{
    const int row = bid_x() * 64 + tid();
    if (row >= rows) return;
    f16* p = x + (size_t)row * E;
    float f[E];
    float mx = -3.0e38f;
    #pragma unroll
    for (int i = 0; i < E; i++) { f[i] = (float)p[i]; mx = fmaxf(mx, f[i]); }
    float sum = 0.0f;
    #pragma unroll
    for (int i = 0; i < E; i++) { f[i] = fast_exp(f[i] - mx); sum += f[i]; }
    const float eps = 1e-8f;
    float isum = 1.0f / (sum + E * eps);
    #pragma unroll
    for (int i = 0; i < E; i++) f[i] = f[i] * isum + eps;
    sum = 1.0f;
    for (int d = 0; d < E - topk; d++)
    {
        float mn = 1.0f; int mj = -1;
        #pragma unroll
        for (int j = 0; j < E; j++) if (f[j] > 0.0f && f[j] < mn) { mn = f[j]; mj = j; }
        #pragma unroll
        for (int j = 0; j < E; j++) if (j == mj) { sum -= f[j]; f[j] = 0.0f; }
    }
    isum = 1.0f / sum;
    #pragma unroll
    for (int i = 0; i < E; i++) p[i] = (f16)(f[i] * isum);
}

// Round 5: the front of a sparse-MoE block in ONE launch for decode-sized row counts -- rms_norm_kernel (elementwise.hip), the two
// kernels above and the row gather into the experts' packed order were four launches of 4.7-4.8 us each per layer
// (profiles/history/r05_mixtral_b16_before_kernel_stats.csv: 19 us of a 124 us Mixtral layer at one row).  One workgroup per row; the SAME
// arithmetic in the same order as those kernels (sum of squares per thread -> wave -> four partials; logits per thread over the
// normalised fp16 row -> wave -> four partials; the top-k on one thread), so the routing is bit-identical to the unfused route.
// xn: the normalised row (natural order); xg: the same row gathered through `perm` (nullable = no packed copy).
// Round 6 (one row): `cp` -- the argument blocks of the SELECTED experts' lean launches (qgemv_lean.h: LeanGroupPlan) are copied from
// the per-expert tables to the slots the two launches behind this kernel read (ascending expert index).
template <int E>
KERNEL void __launch_bounds__(256) moe_front_kernel(const f16* x, const f16* w, const f16* gate, const u16* perm, f16* xn, f16* xg,
                                                    f16* logits, int hidden, float eps, float r_dim, int topk, const MoeCopy cp)
{
    DYN_SMEM(smem);
    f16* const row_lds = (f16*)smem;                                   // the normalised row
    float* const part = (float*)(smem + (size_t)hidden * 2);           // 4 E partial sums (4 for the norm)
    int* const sel_lds = (int*)(smem + (size_t)hidden * 2 + 4 * 16 * 4);   // the selected experts (cp.n_sel of them)
    const int r = bid_x();
    const int t = tid(), lane = lane_id(), wv = wave_id();
    const int dim8 = hidden >> 3;
    const f16x8* xr = (const f16x8*)(x + (size_t)r * hidden);
    const f16x8* wr = (const f16x8*)w;
    // Round 6: everything whose address does not depend on a result is requested at entry -- the row, the norm weight, the router's
    // rows (E x 16 bytes per thread and pass) and the gather permutation: the kernel was five dependent round trips to memory
    // (row -> weight -> router rows -> permutation -> ...) of 1-2 us each on one workgroup (profiles/r08c_mixtral_b1_kernel_stats.csv:
    // 12-16 us).  Rows of <= 4096 elements (two passes of the 256 threads); longer rows take the loops below.  The arithmetic and its
    // order are those of the loops: the routing stays bit-identical to the unfused kernels.
    constexpr int NI = 2;
    const bool pre = dim8 <= NI * 256;
    const bool pvec = (((size_t)perm) & 15) == 0;                        // (the permutation as 16-byte vectors)
    const f16x8 z8 = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f};
    f16x8 xv_[NI], wv_[NI], gv_[NI][E];
    u32x4 pv_[NI];
    if (pre)
    {
        #pragma unroll
        for (int k = 0; k < NI; k++)
        {
            const int i = t + 256 * k;
            const bool on = i < dim8;
            xv_[k] = on ? xr[i] : z8;
            wv_[k] = on ? wr[i] : z8;
        }
        #pragma unroll
        for (int k = 0; k < NI; k++)
        {
            const int i = t + 256 * k;
            const bool on = i < dim8;
            #pragma unroll
            for (int e = 0; e < E; e++) gv_[k][e] = on ? ((const f16x8*)(gate + (size_t)e * hidden))[i] : z8;
            const u32x4 zero4 = {0u, 0u, 0u, 0u};
            pv_[k] = (on && xg && perm && pvec) ? ((const u32x4*)perm)[i] : zero4;
        }
    }
    float ss = 0.0f;
    if (pre)
    {
        #pragma unroll
        for (int k = 0; k < NI; k++)
            if (t + 256 * k < dim8)
            {
                #pragma unroll
                for (int e = 0; e < 8; e++) { const float f = fmaxf(-65504.0f, fminf((float)xv_[k][e], 65504.0f)); ss = fmaf(f, f, ss); }
            }
    }
    else
        for (int i = t; i < dim8; i += 256)
        {
            const f16x8 v = xr[i];
            #pragma unroll
            for (int e = 0; e < 8; e++) { const float f = fmaxf(-65504.0f, fminf((float)v[e], 65504.0f)); ss = fmaf(f, f, ss); }
        }
    ss = wave_allreduce_add(ss);
    if (lane == 0) part[wv] = ss;
    block_sync();
    ss = part[0] + part[1] + part[2] + part[3];
    const float rmf = fast_rsqrt(ss * r_dim + eps);
    block_sync();
    if (pre)
    {
        #pragma unroll
        for (int k = 0; k < NI; k++)
        {
            const int i = t + 256 * k;
            if (i < dim8)
            {
                f16x8 o;
                #pragma unroll
                for (int e = 0; e < 8; e++) o[e] = (f16)(fmaxf(-65504.0f, fminf((float)xv_[k][e], 65504.0f)) * (float)wv_[k][e] * rmf);
                ((f16x8*)row_lds)[i] = o;
                ((f16x8*)(xn + (size_t)r * hidden))[i] = o;
                xv_[k] = o;
            }
        }
    }
    else
        for (int i = t; i < dim8; i += 256)
        {
            const f16x8 v = xr[i], wv8 = wr[i];
            f16x8 o;
            #pragma unroll
            for (int e = 0; e < 8; e++) o[e] = (f16)(fmaxf(-65504.0f, fminf((float)v[e], 65504.0f)) * (float)wv8[e] * rmf);
            ((f16x8*)row_lds)[i] = o;
            ((f16x8*)(xn + (size_t)r * hidden))[i] = o;
        }
    block_sync();
    float acc[E];
    #pragma unroll
    for (int e = 0; e < E; e++) acc[e] = 0.0f;
    if (pre)
    {
        // (a thread's logit terms come from the row elements it normalised itself: no read-back)
        #pragma unroll
        for (int k = 0; k < NI; k++)
            if (t + 256 * k < dim8)
            {
                #pragma unroll
                for (int e = 0; e < E; e++)
                {
                    #pragma unroll
                    for (int j = 0; j < 4; j++)
                        acc[e] = dot2_f32_f16((f16x2){xv_[k][2 * j], xv_[k][2 * j + 1]}, (f16x2){gv_[k][e][2 * j], gv_[k][e][2 * j + 1]}, acc[e]);
                }
            }
    }
    else
        for (int i = t; i < dim8; i += 256)
        {
            const f16x8 xv = ((const f16x8*)row_lds)[i];
            #pragma unroll
            for (int e = 0; e < E; e++)
            {
                const f16x8 gv = ((const f16x8*)(gate + (size_t)e * hidden))[i];
                #pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[e] = dot2_f32_f16((f16x2){xv[2 * j], xv[2 * j + 1]}, (f16x2){gv[2 * j], gv[2 * j + 1]}, acc[e]);
            }
        }
    #pragma unroll
    for (int e = 0; e < E; e++)
    {
        const float s = wave_allreduce_add(acc[e]);
        if (lane == 0) part[wv * E + e] = s;
    }
    block_sync();
    // the packed copy of the row does not wait for the routing
    if (xg)
    {
        if (pre && perm && pvec)
        {
            #pragma unroll
            for (int k = 0; k < NI; k++)
            {
                const int i = t + 256 * k;
                if (i < dim8)
                {
                    const u32x4 pv = pv_[k];
                    f16x8 o;
                    o[0] = row_lds[pv.x & 0xFFFFu]; o[1] = row_lds[pv.x >> 16]; o[2] = row_lds[pv.y & 0xFFFFu]; o[3] = row_lds[pv.y >> 16];
                    o[4] = row_lds[pv.z & 0xFFFFu]; o[5] = row_lds[pv.z >> 16]; o[6] = row_lds[pv.w & 0xFFFFu]; o[7] = row_lds[pv.w >> 16];
                    ((f16x8*)(xg + (size_t)r * hidden))[i] = o;
                }
            }
        }
        else
            for (int i = t; i < hidden; i += 256) xg[(size_t)r * hidden + i] = row_lds[perm ? (int)perm[i] : i];
    }
    if (t == 0)
    {
        // moe_topk_kernel's arithmetic on the fp16-rounded logits
        float f[E];
        float mx = -3.0e38f;
        #pragma unroll
        for (int i = 0; i < E; i++) { f[i] = (float)(f16)(part[i] + part[E + i] + part[2 * E + i] + part[3 * E + i]); mx = fmaxf(mx, f[i]); }
        float sum = 0.0f;
        #pragma unroll
        for (int i = 0; i < E; i++) { f[i] = fast_exp(f[i] - mx); sum += f[i]; }
        const float epsn = 1e-8f;
        float isum = 1.0f / (sum + E * epsn);
        #pragma unroll
        for (int i = 0; i < E; i++) f[i] = f[i] * isum + epsn;
        sum = 1.0f;
        for (int d = 0; d < E - topk; d++)
        {
            float mn = 1.0f; int mj = -1;
            #pragma unroll
            for (int j = 0; j < E; j++) if (f[j] > 0.0f && f[j] < mn) { mn = f[j]; mj = j; }
            #pragma unroll
            for (int j = 0; j < E; j++) if (j == mj) { sum -= f[j]; f[j] = 0.0f; }
        }
        isum = 1.0f / sum;
        #pragma unroll
        for (int i = 0; i < E; i++) logits[(size_t)r * E + i] = (f16)(f[i] * isum);
        if (cp.n_sel)
        {
            int ns = 0;
            #pragma unroll
            for (int i = 0; i < E; i++) if (f[i] > 0.0f && ns < cp.n_sel) sel_lds[ns++] = i;
            for (; ns < cp.n_sel; ns++) sel_lds[ns] = ns > 0 ? sel_lds[0] : 0;     // (never: the top-k leaves exactly topk weights)
        }
    }
    if (cp.n_sel && r == 0)
    {
        block_sync();
        // all loads of the copies before their stores (one round trip, not one per block); blocks are <= 256 16-byte units
        // (moe_front_launch checks), MOE_MAX_SEL experts
        u32x4 v[2][MOE_MAX_SEL];
        #pragma unroll
        for (int k = 0; k < 2; k++)
        {
            // (sum: one block, unit t from the first or the second selected expert)
            const bool second = (t >= cp.b_lo[k] && t < cp.b_hi[k]) || (t >= cp.b2_lo[k] && t < cp.b2_hi[k]);
            #pragma unroll
            for (int y = 0; y < MOE_MAX_SEL; y++)
                if (y < (cp.sum[k] ? 1 : cp.n_sel) && t < cp.units[k])
                    v[k][y] = cp.src[k][(size_t)sel_lds[cp.sum[k] ? (second ? 1 : 0) : y] * cp.units[k] + t];
        }
        #pragma unroll
        for (int k = 0; k < 2; k++)
            #pragma unroll
            for (int y = 0; y < MOE_MAX_SEL; y++)
                if (y < (cp.sum[k] ? 1 : cp.n_sel) && t < cp.units[k]) cp.dst[k][(size_t)y * cp.units[k] + t] = v[k][y];
    }
}

// cp (nullable; one row only): the argument-block copies of the selected experts (moe.h)
int moe_front_launch(const void* x, const void* norm_w, const void* gate, const void* perm, void* xn, void* xg, void* logits,
                     int rows, int hidden, int num_experts, int topk, float eps, const MoeCopy* cp_, void* stream)
{
    EXL2_REQUIRE(x && norm_w && gate && xn && logits, "moe_front: null argument");
    if (rows <= 0) return EXL2_OK;
    if (!(num_experts == 4 || num_experts == 8 || num_experts == 16) || hidden % 8 || hidden > 16384 || topk < 1 || topk > num_experts) return 1;
    MoeCopy cp; memset(&cp, 0, sizeof(cp));
    if (cp_) { if (rows != 1 || cp_->n_sel != topk || cp_->n_sel > MOE_MAX_SEL || cp_->units[0] > 256 || cp_->units[1] > 256 || ((cp_->sum[0] || cp_->sum[1]) && topk != 2)) return 1; cp = *cp_; }
    const size_t lds = (size_t)hidden * 2 + 4 * 16 * 4 + MOE_MAX_SEL * 4;
    const dim3 g((unsigned)rows);
#define MOE_FRONT(E_) LAUNCH((moe_front_kernel<E_>), g, dim3(256), lds, stream, (const f16*)x, (const f16*)norm_w, (const f16*)gate, \
                             (const u16*)perm, (f16*)xn, (f16*)xg, (f16*)logits, hidden, eps, 1.0f / (float)hidden, topk, cp)
    switch (num_experts) { case 4: MOE_FRONT(4); break; case 8: MOE_FRONT(8); break; default: MOE_FRONT(16); break; }
#undef MOE_FRONT
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

// ---- wide expert counts (64, 128; Qwen3-MoE: 128 experts, top 8) -----------------------------------------------------------------
// The reference (q_mlp.cu:403-435) runs softmax128_topk_norm_kernel, copies the weights to the host, synchronises and loops over the
// experts with a weight; here everything stays on the device.  The kernels above keep a row's E logits in the registers of every
// thread and the top-k on one thread: neither stretches to 128.  Two launches instead:
//   (1) logits: the 128 x hidden router matrix of ONE row is 512 KB at hidden 2048 -- one expert per WAVE, four per workgroup, E / 4
//       workgroups per row; every workgroup recomputes the row's norm (4 KB of input) instead of waiting for a hand-off;
//   (2) select + hand-out: one workgroup per row -- its first wave holds the row's logits one (E = 64) or two (E = 128) per lane and
//       selects, then all four waves copy the selected experts' argument blocks to the row's job slots (moe.h: MoeWide).
// The fused form (norm inside launch 1) and the unfused one (rms_norm_kernel, then launch 1 on the normalised rows) share every line
// of arithmetic: the routing is bit-identical between them.
#define MOE_WIDE_EPW 4                  // experts per workgroup of the logits launch = its waves
#define MOE_WIDE_NG 8                   // 16-byte pieces of a router row a lane requests at entry (rows of <= 4096 elements)

template <bool NORM>
KERNEL void __launch_bounds__(256) moe_wide_logits_kernel(const f16* x, const f16* w, const f16* gate, const u16* perm, f16* xn, f16* xg,
                                                          f16* logits, int hidden, int E, float eps, float r_dim)
{
    DYN_SMEM(smem);
    f16* const row_lds = (f16*)smem;                                   // the normalised row
    float* const part = (float*)(smem + (size_t)hidden * 2);           // 4 partial sums of squares
    const int r = bid_y();
    const int t = tid(), lane = lane_id(), wv = wave_id();
    const int dim8 = hidden >> 3;
    const int e = bid_x() * MOE_WIDE_EPW + wv;                         // the wave's expert (E is a multiple of MOE_WIDE_EPW)
    const bool first = bid_x() == 0;                                   // the workgroup that writes the row's xn / xg
    const f16x8* xr = (const f16x8*)(x + (size_t)r * hidden);
    const f16x8* gr = (const f16x8*)(gate + (size_t)e * hidden);
    const f16x8 z8 = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f};
    // the wave's router row does not depend on the norm: requested at entry
    const bool pre = dim8 <= MOE_WIDE_NG * 64;
    f16x8 gv_[MOE_WIDE_NG];
    if (pre)
    {
        #pragma unroll
        for (int k = 0; k < MOE_WIDE_NG; k++) { const int i = lane + 64 * k; gv_[k] = i < dim8 ? gr[i] : z8; }
    }
    if constexpr (NORM)
    {
        // rms_norm_kernel's arithmetic in its order (sum of squares per thread -> wave -> four partials), as in moe_front_kernel
        float ss = 0.0f;
        for (int i = t; i < dim8; i += 256)
        {
            const f16x8 v = xr[i];
            #pragma unroll
            for (int j = 0; j < 8; j++) { const float f = fmaxf(-65504.0f, fminf((float)v[j], 65504.0f)); ss = fmaf(f, f, ss); }
        }
        ss = wave_allreduce_add(ss);
        if (lane == 0) part[wv] = ss;
        block_sync();
        ss = part[0] + part[1] + part[2] + part[3];
        const float rmf = fast_rsqrt(ss * r_dim + eps);
        const f16x8* wr = (const f16x8*)w;
        for (int i = t; i < dim8; i += 256)
        {
            const f16x8 v = xr[i], wv8 = wr[i];
            f16x8 o;
            #pragma unroll
            for (int j = 0; j < 8; j++) o[j] = (f16)(fmaxf(-65504.0f, fminf((float)v[j], 65504.0f)) * (float)wv8[j] * rmf);
            ((f16x8*)row_lds)[i] = o;
            if (first) ((f16x8*)(xn + (size_t)r * hidden))[i] = o;
        }
    }
    else
        for (int i = t; i < dim8; i += 256) ((f16x8*)row_lds)[i] = xr[i];
    block_sync();
    // logits[r, e] = fp16(sum_k xn[r, k] gate[e, k]): a lane's pieces in ascending order, then the wave
    float acc = 0.0f;
    if (pre)
    {
        #pragma unroll
        for (int k = 0; k < MOE_WIDE_NG; k++)
        {
            const int i = lane + 64 * k;
            if (i < dim8)
            {
                const f16x8 xv = ((const f16x8*)row_lds)[i];
                #pragma unroll
                for (int j = 0; j < 4; j++) acc = dot2_f32_f16((f16x2){xv[2 * j], xv[2 * j + 1]}, (f16x2){gv_[k][2 * j], gv_[k][2 * j + 1]}, acc);
            }
        }
    }
    else
        for (int i = lane; i < dim8; i += 64)
        {
            const f16x8 xv = ((const f16x8*)row_lds)[i], gv = gr[i];
            #pragma unroll
            for (int j = 0; j < 4; j++) acc = dot2_f32_f16((f16x2){xv[2 * j], xv[2 * j + 1]}, (f16x2){gv[2 * j], gv[2 * j + 1]}, acc);
        }
    acc = wave_allreduce_add(acc);
    if (lane == 0) logits[(size_t)r * E + e] = (f16)acc;
    // the row in the experts' packed order
    if (first && xg)
        for (int i = t; i < hidden; i += 256) xg[(size_t)r * hidden + i] = row_lds[perm ? (int)perm[i] : i];
}

// The selection of ONE row by ONE wave, in place on p[E] (E = 64 NV): q_mlp_softmax.cuh:272- arithmetic -- fp16 logits widened to fp32,
// softmax by max subtraction, p = e / (sum + E 1e-8) + 1e-8, the top-k largest kept, renormalised by what remains, fp16 with exact
// zeros outside the top-k.  Lane l holds experts l and l + 64.
// Tie rule: the reference's drop loop scans ascending with a strict `<`, so among equal values the LOWER index is dropped first and at
// the boundary the HIGHER index survives -- here: of equal candidates the highest index is taken.
// sel (LDS, nullable) / sel_e, sel_w (memory, nullable): the row's selected experts in ascending index and their weights (topk entries).
template <int NV>
DEV void moe_wide_select(f16* p, int topk, int* sel, int* sel_e, f16* sel_w)
{
    constexpr int E = 64 * NV;
    const int lane = lane_id();
    float f[NV];
    float mx = -3.0e38f;
    #pragma unroll
    for (int i = 0; i < NV; i++) { f[i] = (float)p[lane + 64 * i]; mx = fmaxf(mx, f[i]); }
    mx = wave_allreduce_max(mx);
    float sum = 0.0f;
    #pragma unroll
    for (int i = 0; i < NV; i++) { f[i] = fast_exp(f[i] - mx); sum += f[i]; }
    sum = wave_allreduce_add(sum);
    const float eps = 1e-8f;
    const float isum = 1.0f / (sum + E * eps);
    #pragma unroll
    for (int i = 0; i < NV; i++) f[i] = f[i] * isum + eps;
    bool keep[NV];
    #pragma unroll
    for (int i = 0; i < NV; i++) keep[i] = false;
    for (int d = 0; d < topk; d++)
    {
        float bv = -1.0f; int bi = -1;
        #pragma unroll
        for (int i = 0; i < NV; i++) if (!keep[i] && f[i] >= bv) { bv = f[i]; bi = lane + 64 * i; }      // (>=: the lane's higher index on a tie)
        const float m = wave_allreduce_max(bv);
        const int who = (int)wave_allreduce_max(bv == m ? (float)bi : -1.0f);
        #pragma unroll
        for (int i = 0; i < NV; i++) if (lane + 64 * i == who) keep[i] = true;
    }
    float kept = 0.0f;
    #pragma unroll
    for (int i = 0; i < NV; i++) if (keep[i]) kept += f[i];
    kept = wave_allreduce_add(kept);
    const float rk = 1.0f / kept;
    int before = 0;                                                   // selected experts below this lane's
    #pragma unroll
    for (int i = 0; i < NV; i++)
    {
        const f16 wt = keep[i] ? (f16)(f[i] * rk) : (f16)0.0f;
        p[lane + 64 * i] = wt;
        const u64 mask = wave_ballot(keep[i]);
        const int pos = before + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (keep[i] && pos < topk)
        {
            if (sel) sel[pos] = lane + 64 * i;
            if (sel_e) sel_e[pos] = lane + 64 * i;
            if (sel_w) sel_w[pos] = wt;
        }
        before += __builtin_popcountll(mask);
    }
    // (never: the loop above keeps exactly topk values unless the logits are not numbers -- then expert 0 with weight 0)
    if (lane >= before && lane < topk)
    {
        if (sel) sel[lane] = 0;
        if (sel_e) sel_e[lane] = 0;
        if (sel_w) sel_w[lane] = (f16)0.0f;
    }
}

KERNEL void __launch_bounds__(256) moe_wide_select_kernel(f16* logits, int E, int topk, const MoeWide wd)
{
    SHARED int sel_lds[MOE_MAX_SEL];
    const int r = bid_x(), t = tid();
    if (wave_id() == 0)
    {
        f16* const p = logits + (size_t)r * E;
        int* const se = wd.sel_e ? wd.sel_e + (size_t)r * topk : nullptr;
        f16* const sw = wd.sel_w ? wd.sel_w + (size_t)r * topk : nullptr;
        if (E == 64) moe_wide_select<1>(p, topk, sel_lds, se, sw);
        else moe_wide_select<2>(p, topk, sel_lds, se, sw);
    }
    if (!wd.units[0]) return;
    block_sync();
    // the hand-out: every row's workgroup copies ITS top-k blocks (all loads before the stores: one round trip); blocks are <= 256
    // 16-byte units, a pass has <= MOE_WIDE_MAX_JOBS jobs (moe_wide_front_launch checks both)
    u32x4 v[2][MOE_MAX_SEL];
    #pragma unroll
    for (int k = 0; k < 2; k++)
        #pragma unroll
        for (int y = 0; y < MOE_MAX_SEL; y++)
            if (y < topk && t < wd.units[k]) v[k][y] = wd.src[k][(size_t)sel_lds[y] * wd.units[k] + t];
    #pragma unroll
    for (int k = 0; k < 2; k++)
        #pragma unroll
        for (int y = 0; y < MOE_MAX_SEL; y++)
            if (y < topk && t < wd.units[k])
            {
                const u32 j = (u32)(r * topk + y), e = (u32)sel_lds[y];
                u32x4 o = v[k][y];
                #pragma unroll
                for (int q = 0; q < MOE_WIDE_PATCHES; q++)
                {
                    const MoePatch& pt = wd.patch[k][q];
                    if (pt.off >= 0 && (pt.off >> 4) == t)
                    {
                        const u64 a = pt.base + (u64)j * pt.per_job + (u64)(u32)r * pt.per_row + (u64)e * pt.per_expert;
                        if (pt.off & 8) { o.z = (u32)a; o.w = (u32)(a >> 32); } else { o.x = (u32)a; o.y = (u32)(a >> 32); }
                    }
                }
                wd.dst[k][(size_t)j * wd.units[k] + t] = o;
            }
}

int moe_wide_front_launch(const void* x, const void* norm_w, const void* gate, const void* perm, void* xn, void* xg, void* logits,
                          int rows, int hidden, int num_experts, int topk, float eps, const MoeWide* wd_, void* stream)
{
    EXL2_REQUIRE(x && gate && logits && (!norm_w || xn), "moe_wide_front: null argument");
    if (rows <= 0) return EXL2_OK;
    if (!moe_wide_experts(num_experts) || hidden % 8 || hidden > 16384 || topk < 1 || topk > MOE_MAX_SEL || rows > 65535) return 1;
    MoeWide wd; memset(&wd, 0, sizeof(wd));
    if (wd_)
    {
        wd = *wd_;
        if (wd.units[0] || wd.units[1])
        {
            if (rows > MOE_WIDE_MAX_ROWS || wd.units[0] < 1 || wd.units[1] < 1 || wd.units[0] > 256 || wd.units[1] > 256 ||
                !wd.src[0] || !wd.src[1] || !wd.dst[0] || !wd.dst[1]) return 1;
            for (int k = 0; k < 2; k++)
                for (int q = 0; q < MOE_WIDE_PATCHES; q++)
                    if (wd.patch[k][q].off >= 0 && ((wd.patch[k][q].off & 7) || wd.patch[k][q].off + 8 > wd.units[k] * 16)) return 1;
        }
    }
    const size_t lds = (size_t)hidden * 2 + 4 * 4;
    const dim3 g((unsigned)(num_experts / MOE_WIDE_EPW), (unsigned)rows);
    if (norm_w)
        LAUNCH((moe_wide_logits_kernel<true>), g, dim3(256), lds, stream, (const f16*)x, (const f16*)norm_w, (const f16*)gate, (const u16*)perm,
               (f16*)xn, (f16*)xg, (f16*)logits, hidden, num_experts, eps, 1.0f / (float)hidden);
    else
        LAUNCH((moe_wide_logits_kernel<false>), g, dim3(256), lds, stream, (const f16*)x, (const f16*)nullptr, (const f16*)gate, (const u16*)perm,
               (f16*)nullptr, (f16*)xg, (f16*)logits, hidden, num_experts, 0.0f, 0.0f);
    LAUNCH(moe_wide_select_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (f16*)logits, num_experts, topk, wd);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

extern "C" {

// rms_norm (fp16 in / out) + exl2_moe_route + the gather of the normalised rows through `perm`, one launch; 0 = launched,
// 1 = shape outside it (the caller runs the separate kernels)
int exl2_moe_front(const void* x, const void* norm_w, const void* gate, const void* perm, void* xn, void* xg, void* logits,
                   int rows, int hidden, int num_experts, int topk, float eps, void* stream)
{
    if (moe_wide_experts(num_experts))
    {
        EXL2_REQUIRE(x && norm_w && gate && xn && logits, "moe_front: null argument");
        return moe_wide_front_launch(x, norm_w, gate, perm, xn, xg, logits, rows, hidden, num_experts, topk, eps, nullptr, stream);
    }
    return moe_front_launch(x, norm_w, gate, perm, xn, xg, logits, rows, hidden, num_experts, topk, eps, nullptr, stream);
}

int exl2_moe_route(const void* x, const void* gate, void* logits, int rows, int hidden, int num_experts, int topk, void* stream)
{
    EXL2_REQUIRE(x && gate && logits, "moe_route: null argument");
    EXL2_REQUIRE(num_experts == 4 || num_experts == 8 || num_experts == 16 || moe_wide_experts(num_experts),
                 "moe_route: %d experts (the fused path covers 4, 8, 16 like q_mlp.cu:333, and 64, 128)", num_experts);
    EXL2_REQUIRE(topk >= 1 && topk <= num_experts, "moe_route: bad top-k %d", topk);
    EXL2_REQUIRE(hidden % 8 == 0, "moe_route: hidden %d must be a multiple of 8", hidden);
    if (rows <= 0) return EXL2_OK;
    if (moe_wide_experts(num_experts))
    {
        EXL2_REQUIRE(topk <= MOE_MAX_SEL && hidden <= 16384, "moe_route: %d experts take top-k <= %d and hidden <= 16384", num_experts, MOE_MAX_SEL);
        for (int r0 = 0; r0 < rows; r0 += 32768)             // (grid.y)
        {
            const int nr = rows - r0 < 32768 ? rows - r0 : 32768;
            const int rc = moe_wide_front_launch((const f16*)x + (size_t)r0 * hidden, nullptr, gate, nullptr, nullptr, nullptr, (f16*)logits + (size_t)r0 * num_experts,
                                                 nr, hidden, num_experts, topk, 0.0f, nullptr, stream);
            if (rc) return rc < 0 ? rc : EXL2_E_INVALID;
        }
        return EXL2_OK;
    }
    const f16* xp = (const f16*)x; const f16* gp = (const f16*)gate; f16* lp = (f16*)logits;
    const dim3 g1((unsigned)rows), g2((unsigned)((rows + 63) / 64));
    switch (num_experts)
    {
        case 4:  LAUNCH((moe_gate_kernel<4>), g1, dim3(256), 0, stream, xp, gp, lp, hidden);
                 LAUNCH((moe_topk_kernel<4>), g2, dim3(64), 0, stream, lp, rows, topk); break;
        case 8:  LAUNCH((moe_gate_kernel<8>), g1, dim3(256), 0, stream, xp, gp, lp, hidden);
                 LAUNCH((moe_topk_kernel<8>), g2, dim3(64), 0, stream, lp, rows, topk); break;
        default: LAUNCH((moe_gate_kernel<16>), g1, dim3(256), 0, stream, xp, gp, lp, hidden);
                 LAUNCH((moe_topk_kernel<16>), g2, dim3(64), 0, stream, lp, rows, topk); break;
    }
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

}  // extern "C"
