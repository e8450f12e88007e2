// lora.hip -- low-rank adapters: out[rows, N] += sum over the active adapters l of fp16(x[rows, K] A_l[K, r_l]) B_l[r_l, N].
//
// Reference: apply_loras_cuda (cuda/lora.cu:5-34) -- per adapter and projection two hipBLAS / cuBLAS Hgemm calls, the first into a
// fp16 `temp`, the second accumulating into the projection's output (beta = 1); q_attn.cu:281-283,344 and q_mlp.cu:196-197,210,235
// call it once per projection.  Here ONE launch pair serves a whole group of projections that read the same rows (q | k | v,
// gate | up, or a single o / down) times up to 8 adapters:
//   * lora_down_kernel: x A for every (projection, adapter) pair, split along K over workgroups; each slice writes its fp32 partial
//     to scratch (no atomics: the result does not depend on which workgroup arrives first);
//   * lora_up_kernel: adds the partials in slice order, rounds them to fp16 once (the reference's `temp`), multiplies by its column
//     tile of B, sums the adapters in fp32 and adds the fp16 value already in `out` -- one rounding of the output.
// Both products run on the matrix cores (mfma_16x16x32_f16, fp32 accumulate) with operands read straight from memory: at set time
// the group keeps A transposed ([rp, K]) and B transposed ([N, rp]), the rank padded with zeros to rp = a multiple of 32, so a lane's
// eight k-consecutive values of either operand are one 16-byte load.  No LDS, one wave per workgroup: at decode sizes both launches
// are latency bound, and the operands of a step (K * rp + rp * N halves per pair) come from the L2 after the first token.
#include "lora.h"
#include "errors.h"
#include <string.h>
#include <stdlib.h>
#include <vector>

#define LORA_MAX_PAIRS (LORA_MAX_PROJ * LORA_MAX_ACTIVE)
#define LORA_WAVE_TILES 4          // 16-column tiles per wave (both kernels)
#define LORA_MAX_SLICES 32         // K slices of the down kernel (times row tiles: at most this many, or one slice)

struct LoraPair { const f16* at; const f16* bt; float* part; int proj, rp; };       // at [rp, K], bt [N, rp], part [slices, rows16, rp]
struct LoraArgs
{
    LoraPair pair[LORA_MAX_PAIRS];                // in the order of the call's id list, then projection
    const f16* x; f16* out[LORA_MAX_PROJ];
    int N[LORA_MAX_PROJ];
    int up_proj[LORA_MAX_PROJ];                   // lora_up_kernel: blockIdx.z -> projection (those with at least one pair)
    int K, rows, rows16, slices, n_pairs;
};

// blockIdx = (K slice, row tile + row tiles * column group, pair); one wave
KERNEL void __launch_bounds__(64) lora_down_kernel(const LoraArgs a)
{
    const LoraPair p = a.pair[bid_z()];
    const int row_tiles = a.rows16 >> 4;
    const int rt = bid_y() % row_tiles, t0 = (bid_y() / row_tiles) * LORA_WAVE_TILES;
    const int tiles = p.rp >> 4;
    if (t0 >= tiles) return;                                                         // (wave-uniform)
    const int s = bid_x(), k_steps = a.K >> 5;
    const int k_lo = (int)((long long)k_steps * s / a.slices), k_hi = (int)((long long)k_steps * (s + 1) / a.slices);
    const int lane = lane_id(), i = lane & 15, q = lane >> 4;
    const int row = rt * 16 + i;
    const bool row_on = row < a.rows;
    const f16* const xr = a.x + (size_t)(row_on ? row : 0) * a.K + q * 8;
    const f16* const ar = p.at + (size_t)(t0 * 16 + i) * a.K + q * 8;
    const f16x8 z8 = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f};
    f32x4 acc[LORA_WAVE_TILES];
    #pragma unroll
    for (int c = 0; c < LORA_WAVE_TILES; c++) acc[c] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = k_lo; k < k_hi; k++)
    {
        const f16x8 xv = row_on ? *(const f16x8*)(xr + (size_t)k * 32) : z8;
        #pragma unroll
        for (int c = 0; c < LORA_WAVE_TILES; c++)
        {
            if (t0 + c < tiles)
            {
                const f16x8 av = *(const f16x8*)(ar + (size_t)c * 16 * a.K + (size_t)k * 32);
                acc[c] = mfma_16x16x32_f16(xv, av, acc[c]);
            }
        }
    }
    // D: column i, rows 4 q + r.  Rows >= a.rows hold zeros (their x fragment was zero): the scratch covers rows16 rows.
    float* const dst = p.part + ((size_t)s * a.rows16 + rt * 16 + q * 4) * p.rp + t0 * 16 + i;
    #pragma unroll
    for (int c = 0; c < LORA_WAVE_TILES; c++)
    {
        if (t0 + c < tiles)
        {
            #pragma unroll
            for (int r = 0; r < 4; r++) dst[(size_t)r * p.rp + c * 16] = acc[c][r];
        }
    }
}

// blockIdx = (group of LORA_WAVE_TILES column tiles, row tile, projection with pairs); one wave
KERNEL void __launch_bounds__(64) lora_up_kernel(const LoraArgs a)
{
    const int proj = a.up_proj[bid_z()];
    const int N = a.N[proj], tiles = N >> 4;
    const int t0 = bid_x() * LORA_WAVE_TILES;
    if (t0 >= tiles) return;                                                         // (wave-uniform)
    const int rt = bid_y();
    const int lane = lane_id(), i = lane & 15, q = lane >> 4;
    const int row = rt * 16 + i;
    const bool row_on = row < a.rows;
    f32x4 acc[LORA_WAVE_TILES];
    #pragma unroll
    for (int c = 0; c < LORA_WAVE_TILES; c++) acc[c] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int pi = 0; pi < a.n_pairs; pi++)
    {
        const LoraPair p = a.pair[pi];
        if (p.proj != proj) continue;
        const f16* const br = p.bt + (size_t)(t0 * 16 + i) * p.rp + q * 8;
        for (int ks = 0; ks < (p.rp >> 5); ks++)
        {
            // this lane's part of fp16(x A): row `row`, ranks 32 ks + 8 q .. + 7; the slices' partials added in slice order
            f32x4 lo = {0.0f, 0.0f, 0.0f, 0.0f}, hi = {0.0f, 0.0f, 0.0f, 0.0f};
            if (row_on)
            {
                const float* src = p.part + (size_t)row * p.rp + ks * 32 + q * 8;
                for (int s = 0; s < a.slices; s++, src += (size_t)a.rows16 * p.rp)
                {
                    lo += *(const f32x4*)src;
                    hi += *(const f32x4*)(src + 4);
                }
            }
            const f16x8 tv = {(f16)lo[0], (f16)lo[1], (f16)lo[2], (f16)lo[3], (f16)hi[0], (f16)hi[1], (f16)hi[2], (f16)hi[3]};
            #pragma unroll
            for (int c = 0; c < LORA_WAVE_TILES; c++)
            {
                if (t0 + c < tiles)
                {
                    const f16x8 bv = *(const f16x8*)(br + (size_t)c * 16 * p.rp + ks * 32);
                    acc[c] = mfma_16x16x32_f16(tv, bv, acc[c]);
                }
            }
        }
    }
    f16* const out = a.out[proj];
    #pragma unroll
    for (int c = 0; c < LORA_WAVE_TILES; c++)
    {
        if (t0 + c < tiles)
        {
            #pragma unroll
            for (int r = 0; r < 4; r++)
            {
                const int orow = rt * 16 + q * 4 + r;
                if (orow < a.rows)
                {
                    f16* const o = out + (size_t)orow * N + (t0 + c) * 16 + i;
                    *o = (f16)((float)*o + acc[c][r]);
                }
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

struct LoraEntry { f16* at; f16* bt; int r, rp; };                   // owned copies; r == 0: no entry
struct LoraAdapter { u64 id; LoraEntry e[LORA_MAX_PROJ]; };
struct LoraGroup
{
    int n_proj, K, N[LORA_MAX_PROJ], max_rows;
    int rows_cap;                                  // rows x slices the partial scratch of a pair covers
    std::vector<LoraAdapter> tab;
    float* part; size_t part_floats;               // fp32 partials of the down kernel, sized when the table is set
};

static void free_table(std::vector<LoraAdapter>& tab, int n_proj)
{
    for (LoraAdapter& ad : tab)
        for (int p = 0; p < n_proj; p++)
        {
            if (ad.e[p].at) (void)hipFree(ad.e[p].at);
            if (ad.e[p].bt) (void)hipFree(ad.e[p].bt);
        }
    tab.clear();
}

int lora_group_make(LoraGroup** out, int n_proj, int K, const int* N, int max_rows)
{
    EXL2_REQUIRE(out && N, "lora: null argument");
    EXL2_REQUIRE(n_proj >= 1 && n_proj <= LORA_MAX_PROJ, "lora: %d projections in one group (1 .. %d)", n_proj, LORA_MAX_PROJ);
    EXL2_REQUIRE(K > 0 && (K & 31) == 0, "lora: in_features %d is not a multiple of 32", K);
    for (int p = 0; p < n_proj; p++) EXL2_REQUIRE(N[p] > 0 && (N[p] & 31) == 0, "lora: out_features %d is not a multiple of 32", N[p]);
    EXL2_REQUIRE(max_rows >= 1, "lora: max_rows %d", max_rows);
    LoraGroup* g = new LoraGroup();
    g->n_proj = n_proj; g->K = K; g->max_rows = max_rows;
    for (int p = 0; p < LORA_MAX_PROJ; p++) g->N[p] = p < n_proj ? N[p] : 0;
    const int rows16 = (max_rows + 15) & ~15;
    g->rows_cap = rows16 > 16 * LORA_MAX_SLICES ? rows16 : 16 * LORA_MAX_SLICES;
    g->part = nullptr; g->part_floats = 0;
    *out = g;
    return EXL2_OK;
}

void lora_group_free(LoraGroup* g)
{
    if (!g) return;
    free_table(g->tab, g->n_proj);
    if (g->part) (void)hipFree(g->part);
    delete g;
}

// dst [rows_out (>= cols of src, zero rows behind them), ld_out (>= rows of src, zero behind them)] = src [rows_src, cols_src]^T
static int upload_transposed(const void* src_dev, int rows_src, int cols_src, int rows_out, int ld_out, f16** out)
{
    std::vector<u16> h((size_t)rows_src * cols_src), t((size_t)rows_out * ld_out, (u16)0);
    HIP_TRY(hipMemcpy(h.data(), src_dev, h.size() * 2, hipMemcpyDeviceToHost));
    for (int r = 0; r < rows_src; r++)
        for (int c = 0; c < cols_src; c++) t[(size_t)c * ld_out + r] = h[(size_t)r * cols_src + c];
    f16* d = nullptr;
    if (hipMalloc((void**)&d, t.size() * 2) != hipSuccess)
    {
        (void)hipGetLastError();
        EXL2_FAIL(EXL2_E_OOM, "HIP out of memory (LoRA adapter copy: %zu bytes)", t.size() * 2);
    }
    const hipError_t e = hipMemcpy(d, t.data(), t.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); HIP_TRY(e); }
    *out = d;
    return EXL2_OK;
}

int lora_group_set(LoraGroup* g, int n, const u64* ids, const void* const* a, const void* const* b, const int* rank)
{
    EXL2_REQUIRE(g && n >= 0 && (n == 0 || (ids && a && b && rank)), "set_loras: null argument");
    for (int l = 0; l < n * g->n_proj; l++)
    {
        if (!a[l] || !b[l] || rank[l] == 0) continue;
        EXL2_REQUIRE(rank[l] >= 1 && rank[l] <= LORA_MAX_RANK, "set_loras: rank %d exceeds the limit of %d", rank[l], LORA_MAX_RANK);
        EXL2_REQUIRE(!(((size_t)a[l]) & 1) && !(((size_t)b[l]) & 1), "set_loras: misaligned adapter tensor");
    }
    HIP_TRY(hipDeviceSynchronize());               // the caller's tensors are complete; nothing still reads the old table
    std::vector<LoraAdapter> tab;
    size_t floats = 0;
    int max_rank = 0;
    for (int l = 0; l < n; l++)
    {
        LoraAdapter ad; memset(&ad, 0, sizeof(ad));
        ad.id = ids[l];
        tab.push_back(ad);
        for (int p = 0; p < g->n_proj; p++)
        {
            const int i = l * g->n_proj + p, r = rank[i];
            if (!a[i] || !b[i] || r == 0) continue;
            LoraEntry& e = tab.back().e[p];
            e.r = r; e.rp = (r + 31) & ~31;
            int rc = upload_transposed(a[i], g->K, r, e.rp, g->K, &e.at);                       // A [K, r] -> [rp, K]
            if (rc == EXL2_OK) rc = upload_transposed(b[i], r, g->N[p], g->N[p], e.rp, &e.bt);  // B [r, N] -> [N, rp]
            if (rc != EXL2_OK) { free_table(tab, g->n_proj); return rc; }
            floats += (size_t)g->rows_cap * e.rp;
            if (r > max_rank) max_rank = r;
        }
    }
    if (floats > g->part_floats)
    {
        float* fresh = nullptr;
        if (hipMalloc((void**)&fresh, floats * 4) != hipSuccess)
        {
            (void)hipGetLastError();
            free_table(tab, g->n_proj);
            EXL2_FAIL(EXL2_E_OOM, "HIP out of memory (LoRA scratch: %zu bytes)", floats * 4);
        }
        if (g->part) (void)hipFree(g->part);
        g->part = fresh; g->part_floats = floats;
    }
    free_table(g->tab, g->n_proj);
    g->tab.swap(tab);
    return max_rank;
}

int lora_group_apply(LoraGroup* g, int n_ids, const u64* ids, const f16* x, f16* const* out, int rows, void* stream)
{
    if (!g || n_ids <= 0 || rows <= 0 || g->tab.empty()) return EXL2_OK;
    EXL2_REQUIRE(ids && x && out, "apply_loras: null argument");
    EXL2_REQUIRE(rows <= g->max_rows, "apply_loras: %d rows exceed max_rows %d", rows, g->max_rows);
    EXL2_REQUIRE(!(((size_t)x) & 15), "apply_loras: input rows must be 16-byte aligned");
    LoraArgs a; memset(&a, 0, sizeof(a));
    const int row_tiles = (rows + 15) >> 4;
    a.rows = rows; a.rows16 = row_tiles * 16; a.K = g->K; a.x = x;
    a.slices = LORA_MAX_SLICES / row_tiles;
    if (a.slices > (g->K >> 5)) a.slices = g->K >> 5;
    if (a.slices < 1) a.slices = 1;
    int active = 0, max_rp = 0, n_up = 0, max_n = 0;
    bool has[LORA_MAX_PROJ] = {false, false, false};
    size_t off = 0;
    for (int l = 0; l < n_ids; l++)
    {
        const LoraAdapter* ad = nullptr;
        for (const LoraAdapter& t : g->tab) if (t.id == ids[l]) { ad = &t; break; }
        if (!ad) continue;                                                           // (lora.cu:20-21)
        EXL2_REQUIRE(++active <= LORA_MAX_ACTIVE, "apply_loras: more than %d active adapters", LORA_MAX_ACTIVE);
        for (int p = 0; p < g->n_proj; p++)
        {
            const LoraEntry& e = ad->e[p];
            if (!e.r) continue;
            LoraPair& pr = a.pair[a.n_pairs++];
            pr.at = e.at; pr.bt = e.bt; pr.part = g->part + off; pr.proj = p; pr.rp = e.rp;
            off += (size_t)a.slices * a.rows16 * e.rp;
            if (e.rp > max_rp) max_rp = e.rp;
            has[p] = true;
        }
    }
    if (a.n_pairs == 0) return EXL2_OK;
    EXL2_REQUIRE(off <= g->part_floats, "apply_loras: scratch too small (an adapter listed twice?)");
    for (int p = 0; p < g->n_proj; p++)
    {
        a.N[p] = g->N[p]; a.out[p] = out[p];
        if (!has[p]) continue;
        EXL2_REQUIRE(out[p], "apply_loras: null output");
        a.up_proj[n_up++] = p;
        if (g->N[p] > max_n) max_n = g->N[p];
    }
    const int col_groups = ((max_rp >> 4) + LORA_WAVE_TILES - 1) / LORA_WAVE_TILES;
    LAUNCH(lora_down_kernel, dim3((unsigned)a.slices, (unsigned)(row_tiles * col_groups), (unsigned)a.n_pairs), dim3(64), 0, stream, a);
    const int up_groups = ((max_n >> 4) + LORA_WAVE_TILES - 1) / LORA_WAVE_TILES;
    LAUNCH(lora_up_kernel, dim3((unsigned)up_groups, (unsigned)row_tiles, (unsigned)n_up), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

// ---- C ABI: a group on its own (the modules own theirs: modules.hip) -------------------------------------------------------------

extern "C" {

int exl2_make_lora_group(void** handle, int n_proj, int in_features, const int* out_features, int max_rows)
{
    EXL2_REQUIRE(handle, "make_lora_group: null argument");
    LoraGroup* g = nullptr;
    const int rc = lora_group_make(&g, n_proj, in_features, out_features, max_rows);
    if (rc) return rc;
    *handle = g;
    return EXL2_OK;
}

int exl2_free_lora_group(void* handle)
{
    lora_group_free((LoraGroup*)handle);
    return EXL2_OK;
}

int exl2_lora_group_set_loras(void* handle, int n_loras, const u64* ids, const void* const* a, const void* const* b, const int* ranks)
{
    EXL2_REQUIRE(handle, "lora_group_set_loras: null handle");
    return lora_group_set((LoraGroup*)handle, n_loras, ids, a, b, ranks);
}

int exl2_apply_loras(void* handle, int n_loras, const u64* ids, const void* x, void* const* out, int rows, void* stream)
{
    EXL2_REQUIRE(handle, "apply_loras: null handle");
    return lora_group_apply((LoraGroup*)handle, n_loras, ids, (const f16*)x, (f16* const*)out, rows, stream);
}

}  // extern "C"
