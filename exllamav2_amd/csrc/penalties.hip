// penalties.hip -- the reference sampler's repetition / frequency / presence penalties and its token bias on the device.
//
// Replaces apply_rep_penalty (exllamav2_ext/ext_sampling.cpp:32-72 over apply_rep_penalty_cpu, cpp/sampling.cpp:20-110) and the
// token-bias add (fast_fadd_cpu, generator/sampler.py:427-429), which the reference runs on host logits ahead of every other
// sampler stage (sampler.py:408-429).  Here the logits stay in HBM: fp16 as the head projection wrote them (or fp32) in, fp32
// out, bit for bit what the reference leaves for float(logits).  The sequence of a row is read from the decoder's token log at
// launch (history[row, 0 .. hist_pos[row]]), so nothing of the launch changes from token to token and it replays from a graph.
//
// The reference walks the last sustain + decay tokens backwards; per token id that walk is:
//   first encounter (walk step w1):  x = x > 0 ? x / rep(w1) : x * rep(w1);  x -= pres(w1)
//   every encounter (walk step w):   x -= freq(w), in walk order
// with rep / freq / pres constant for w < sustain and moving by sequential fp32 additions behind it.  Those ramp values depend on
// the settings only: the host accumulates them once (ramps[3][decay]: rep, freq, pres at walk step sustain + k), nothing serial is
// left for the device.
//
// One workgroup owns a slice of PEN_SLICE vocabulary entries of one row.  It reads the whole window once and notes, per id that
// falls into its slice, in LDS tables of the slice's size: the first walk step (atomic min) and -- only with a frequency penalty --
// the number of encounters inside the sustain range (their subtractions are all the same value: only the count matters) and the
// first step / count inside the decay range.  No global scratch, no global atomics, no hand-off between workgroups.  Then every
// thread finishes the four entries it loaded.  Encounters inside the decay range subtract different values, so they need walk
// order: the ids that have any are listed, and a WAVE takes one id at a time -- from the id's first decay-range encounter on, 64
// walk steps per ballot, the matching steps subtracted in bit order, until the id's count is used up.  A window of all-different
// ids finds every id in its first ballot; an id's owner thread never scans alone (one thread per id walking the range cost 150-200
// us on text-like windows).  The decay range's ids and frequency values are staged in LDS when they fit (4096), read from memory
// otherwise; the sustain range is only ever read once, from memory: no window length is refused.
#include "hw.h"
#include "errors.h"

// the reference rounds the product and the difference separately (two statements on a float in memory)
#pragma clang fp contract(off)

#define PEN_THREADS 256
#define PEN_SLICE 1024                 // 4 entries per thread
#define PEN_STAGE 4096                 // ids of the decay range held in LDS
#define PEN_NONE 0xFFFFFFFFu

struct PenArgs
{
    const void* logits; float* out;
    const int* history; const int* hist_pos; const int* tail;
    const float* ramps; const float* bias;
    int vocab, ld, hist_stride, share, pos_offset, sustain, decay;
    float penalty, freq, pres;
};

// atomic minimum on an LDS word (ds_min_u32); the compiler builtin, the same in every build of this file
DEV void pen_atomic_min(u32* p, u32 v) { (void)__atomic_fetch_min(p, v, __ATOMIC_RELAXED); }
DEV f32x4 pen_load4(const float* p) { return *(const f32x4*)p; }
DEV f32x4 pen_load4(const f16* p) { const f16x4 h = *(const f16x4*)p; return (f32x4){(float)h.x, (float)h.y, (float)h.z, (float)h.w}; }

template <typename T>
KERNEL void __launch_bounds__(PEN_THREADS) apply_penalties_kernel(const PenArgs a)
{
    SHARED u32   s_first[PEN_SLICE];       // first walk step that meets the id
    SHARED u32   s_cnt[PEN_SLICE];         // encounters at walk steps < sustain
    SHARED u32   s_dfirst[PEN_SLICE];      // first walk step >= sustain that meets the id
    SHARED u32   s_dcnt[PEN_SLICE];        // encounters at walk steps >= sustain
    SHARED float s_val[PEN_SLICE];
    SHARED u32   s_list[PEN_SLICE];        // slice entries with decay-range encounters
    SHARED u32   s_nlist;
    SHARED int   s_ids[PEN_STAGE];
    SHARED float s_freq[PEN_STAGE];        // the frequency penalty in force at the staged steps

    const int row = bid_y(), t = tid(), V = a.vocab;
    const int v0 = bid_x() * PEN_SLICE;
    const int sl = min(PEN_SLICE, V - v0);
    const T* lr = (const T*)a.logits + (size_t)row * a.ld;
    float* orow = a.out + (size_t)row * V;

    // this thread's four entries: requested first, used behind the window pass
    const int li0 = 4 * t, vq = v0 + li0;
    const bool vec = ((V & 3) == 0) && ((a.ld & 3) == 0) && ((((size_t)a.logits) & 15) == 0) && ((((size_t)a.out) & 15) == 0) &&
                     (!a.bias || (((size_t)a.bias) & 15) == 0);
    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec) { if (vq < V) { const f32x4 q = pen_load4(lr + vq); x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w; } }
    else
    {
        #pragma unroll
        for (int c = 0; c < 4; c++) if (vq + c < V) x[c] = (float)lr[vq + c];
    }

    // ---- the row's sequence and its window ------------------------------------------------------------------------------
    const int hrow = a.share ? 0 : row;
    const int* hist = a.history + (size_t)hrow * a.hist_stride;
    const int p = a.hist_pos[hrow] + a.pos_offset;
    // (the host keeps the position inside the log; one outside it penalises nothing rather than read past the end)
    const bool inside = p >= 0 && p < a.hist_stride;
    const int base_len = inside ? p + 1 : 0;
    const int seq_len = inside ? base_len + (a.share ? row : 0) : 0;
    const long long sust = a.sustain == -1 ? (long long)seq_len : (long long)a.sustain;
    long long beg = (long long)seq_len - sust - (long long)a.decay;
    if (beg < 0) beg = 0;
    const int n = seq_len - (int)beg;                               // walk steps 0 .. n - 1, step w = sequence index seq_len - 1 - w
    const int ns = sust < (long long)n ? (int)sust : n;             // steps below ns: the sustain range
    const int nd = n - ns;                                          // the decay range (<= decay steps)
    auto tok = [&](int w) -> int { const int j = seq_len - 1 - w; return j < base_len ? hist[j] : a.tail[j - base_len]; };
    // slice-local index of an id, -1 outside the slice (ids outside [0, vocab) change nothing: sampling.cpp:78)
    auto local = [&](int id) -> int { const u32 li = (u32)id - (u32)v0; return ((u32)id < (u32)V && li < (u32)sl) ? (int)li : -1; };
    auto ramp = [&](int c, u32 w, float start) -> float {
        return (w < (u32)ns || !a.ramps) ? start : a.ramps[(size_t)c * a.decay + (w - (u32)ns)];
    };
    const bool freq_on = a.freq != 0.0f;
    const bool dec_pass = freq_on && nd > 0;
    const bool staged = dec_pass && nd <= PEN_STAGE;

    for (int i = t; i < PEN_SLICE; i += PEN_THREADS) { s_first[i] = PEN_NONE; s_cnt[i] = 0; s_dfirst[i] = PEN_NONE; s_dcnt[i] = 0; }
    if (staged) for (int k = t; k < nd; k += PEN_THREADS) { s_ids[k] = tok(ns + k); s_freq[k] = ramp(1, (u32)(ns + k), a.freq); }
    if (t == 0) s_nlist = 0;
    block_sync();

    // ---- the window, once: four ids in flight per thread ----------------------------------------------------------------
    for (int w0 = t; w0 < n; w0 += 4 * PEN_THREADS)
    {
        int id[4];
        #pragma unroll
        for (int u = 0; u < 4; u++) { const int w = w0 + u * PEN_THREADS; id[u] = w < n ? tok(w) : -1; }
        #pragma unroll
        for (int u = 0; u < 4; u++)
        {
            const int w = w0 + u * PEN_THREADS;
            const int li = local(id[u]);
            if (li < 0) continue;
            pen_atomic_min(&s_first[li], (u32)w);
            if (!freq_on) continue;
            if (w < ns) atomic_add_u32(&s_cnt[li], 1u);
            else { pen_atomic_min(&s_dfirst[li], (u32)w); atomic_add_u32(&s_dcnt[li], 1u); }
        }
    }
    block_sync();

    // ---- first encounter + the sustain range's encounters ----------------------------------------------------------------
    #pragma unroll
    for (int c = 0; c < 4; c++)
    {
        const int li = li0 + c;
        if (li >= sl) continue;
        const u32 w1 = s_first[li];
        if (w1 == PEN_NONE) continue;
        float y = x[c];
        const float rep = ramp(0, w1, a.penalty);
        if (y > 0.0f) y = y / rep; else y = y * rep;
        y = y - ramp(2, w1, a.pres);
        if (freq_on)
        {
            // sequential subtractions of one value; once one of them changes nothing, none of the rest does
            const u32 cnt = s_cnt[li];
            for (u32 k = 0; k < cnt; k++) { const float z = y - a.freq; if (z == y) break; y = z; }
        }
        x[c] = y;
    }

    // ---- the decay range's encounters, in walk order ---------------------------------------------------------------------
    if (dec_pass)
    {
        #pragma unroll
        for (int c = 0; c < 4; c++)
        {
            if (li0 + c >= sl) continue;
            s_val[li0 + c] = x[c];
            if (s_dcnt[li0 + c]) s_list[atomic_add_u32(&s_nlist, 1u)] = (u32)(li0 + c);
        }
        block_sync();
        const int n_list = (int)s_nlist, lane = lane_id();
        for (int e = wave_id(); e < n_list; e += PEN_THREADS / 64)         // (everything the loops below branch on is wave-uniform)
        {
            const int li = (int)s_list[e], id = v0 + li;
            const int k0 = (int)s_dfirst[li] - ns;
            float y = s_val[li];
            u32 left = s_dcnt[li];
            for (int kb = k0 & ~63; left && kb < nd; kb += 64)
            {
                const int k = kb + lane;
                const bool hit = k >= k0 && k < nd && (staged ? s_ids[k] : tok(ns + k)) == id;
                u64 m = wave_ballot(hit);
                while (m)
                {
                    const int kk = kb + __builtin_ctzll(m);
                    m &= m - 1;
                    y = y - (staged ? s_freq[kk] : ramp(1, (u32)(ns + kk), a.freq));
                    left--;
                }
            }
            if (lane == 0) s_val[li] = y;
        }
        block_sync();
        #pragma unroll
        for (int c = 0; c < 4; c++) if (li0 + c < sl) x[c] = s_val[li0 + c];
    }

    // ---- token bias, store ------------------------------------------------------------------------------------------------
    if (vec)
    {
        if (vq >= V) return;
        f32x4 q = (f32x4){x[0], x[1], x[2], x[3]};
        if (a.bias) { const f32x4 b = *(const f32x4*)(a.bias + vq); q.x = q.x + b.x; q.y = q.y + b.y; q.z = q.z + b.z; q.w = q.w + b.w; }
        *(f32x4*)(orow + vq) = q;
    }
    else
    {
        #pragma unroll
        for (int c = 0; c < 4; c++) if (vq + c < V) orow[vq + c] = a.bias ? x[c] + a.bias[vq + c] : x[c];
    }
}

extern "C" {

// out fp32 [rows, vocab] (dense rows; may be the fp32 logits themselves when ld == vocab: every entry is read and written by one
// thread).  history int32 [*, hist_stride], hist_pos int32: row r's sequence is history[r, 0 .. hist_pos[r] + pos_offset]; with
// rows_share_sequence every row takes history row 0 / hist_pos[0] and row r appends tail[0 .. r - 1].  ramps (needed when
// decay > 0): fp32 [3, decay] on the device, made on the host -- ramps[c][k] = the value of penalty (c = 0), frequency (1),
// presence (2) after k sequential fp32 additions of (target - start) / decay.  token_bias: nullable fp32 [vocab].
int exl2_apply_penalties(const void* logits, int logits_f32, int rows, int vocab, int ld, float* out,
                         const int* history, int hist_stride, const int* hist_pos, int pos_offset, int rows_share_sequence,
                         const int* tail, float penalty, int sustain, int decay, float alpha_frequency, float alpha_presence,
                         const float* ramps, const float* token_bias, void* stream)
{
    EXL2_REQUIRE(logits && out && history && hist_pos, "apply_penalties: null argument");
    EXL2_REQUIRE(vocab >= 1 && ld >= vocab, "apply_penalties: vocab %d, row stride %d", vocab, ld);
    EXL2_REQUIRE(hist_stride >= 1, "apply_penalties: hist_stride %d", hist_stride);
    EXL2_REQUIRE(decay >= 0 && sustain >= -1, "apply_penalties: sustain %d, decay %d", sustain, decay);
    EXL2_REQUIRE(decay == 0 || ramps, "apply_penalties: decay %d needs the ramp table", decay);
    EXL2_REQUIRE(!rows_share_sequence || rows <= 1 || tail, "apply_penalties: rows that share a sequence need the tail");
    if (rows <= 0) return EXL2_OK;
    if (rows > 65535) EXL2_FAIL(EXL2_E_UNSUPPORTED, "apply_penalties: %d rows in one launch (at most 65535)", rows);
    PenArgs a;
    a.logits = logits; a.out = out; a.history = history; a.hist_pos = hist_pos; a.tail = tail; a.ramps = decay ? ramps : nullptr;
    a.bias = token_bias; a.vocab = vocab; a.ld = ld; a.hist_stride = hist_stride; a.share = rows_share_sequence ? 1 : 0;
    a.pos_offset = pos_offset; a.sustain = sustain; a.decay = decay;
    a.penalty = penalty; a.freq = alpha_frequency; a.pres = alpha_presence;
    const dim3 grid((unsigned)((vocab + PEN_SLICE - 1) / PEN_SLICE), (unsigned)rows);
    if (logits_f32) LAUNCH((apply_penalties_kernel<float>), grid, dim3(PEN_THREADS), 0, stream, a);
    else            LAUNCH((apply_penalties_kernel<f16>), grid, dim3(PEN_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

}  // extern "C"
