// spec_decode.hip -- the tail of a speculative greedy decode step for gfx950: accept the drafts the model's own arg-max confirms,
// log the tokens, advance the position by a variable amount and draft the next K tokens from the sequence's own n-grams -- one
// launch of one workgroup behind exl2_argmax_rows, so a verify step stays one graph with no host round trip.
//
// Procedure = the reference's n-gram speculation (exllamav2/generator/dynamic.py:1009-1058 drafting, :1139- verification) with
// the reference's count trie replaced by a rule of our own (latest longest suffix match, overlapping copy): greedy verification
// makes the emitted tokens independent of the drafts, only the acceptance rate depends on them.
#include "hw.h"
#include "errors.h"

#define SPEC_MAX_K 15
#define SPEC_MAX_N 7

struct SpecArgs
{
    const int* cand; int* ids; int* history; int* pos; int* stats; const int* forced;
    int* rand_counter;                          // nullable: advanced by the tokens the step emits (sampled verification)
    int forced_len, K, N, hist_len, draft_only;
};

KERNEL void __launch_bounds__(1024) spec_accept_draft_kernel(const SpecArgs a)
{
    SHARED int s_cand[SPEC_MAX_K + 1];          // the tokens this launch logs: sequence indices p + 1 .. p + 1 + n_acc
    SHARED int s_ids[SPEC_MAX_K + 1];
    SHARED int s_pat[SPEC_MAX_N];               // s_pat[k] = seq[L - 1 - k]
    SHARED int s_best[16][SPEC_MAX_N];          // per wave: latest j whose match reaches k + 1 tokens
    const int K = a.K, N = a.N;
    const int t = tid();
    const int p = a.pos[0];
    // the host keeps p inside the log (the decoder's bound); a position outside it changes nothing rather than index past the end
    if (p < 0 || p + (a.draft_only ? 1 : K + 2) > a.hist_len) return;
    if (t <= K)
    {
        s_ids[t] = a.ids[t];
        s_cand[t] = a.draft_only ? 0 : a.cand[t];
    }
    block_sync();
    int n_acc = -1;                             // draft-only: nothing accepted, nothing logged, the position stays
    if (!a.draft_only)
    {
        n_acc = 0;
        while (n_acc < K && s_ids[n_acc + 1] == s_cand[n_acc]) n_acc++;
        if (t <= n_acc) a.history[p + 1 + t] = s_cand[t];
    }
    const int p1 = p + n_acc + 1;               // the new cache length
    const int L = p1 + 1;                       // tokens of the sequence, the next step's input token included
    // the sequence as the search sees it: what this launch logs comes from LDS, never from the stores above
    auto tok = [&](int j) -> int { return j > p ? s_cand[j - p - 1] : a.history[j]; };
    if (t < N) s_pat[t] = L - 1 - t >= 0 ? tok(L - 1 - t) : -1;
    block_sync();

    int best[SPEC_MAX_N];
    #pragma unroll
    for (int k = 0; k < SPEC_MAX_N; k++) best[k] = -1;
    if (!a.forced)
    {
        const int last = s_pat[0];
        // j ascends per thread, so the last hit of a length is the thread's latest; the tokens below j are read only behind a hit
        for (int j = t; j <= L - 2; j += nthreads())
        {
            if (tok(j) != last) continue;
            const int lim = N < j + 1 ? N : j + 1;
            int m = 1;
            while (m < lim && tok(j - m) == s_pat[m]) m++;
            #pragma unroll
            for (int k = 0; k < SPEC_MAX_N; k++) if (k < m) best[k] = j;
        }
        #pragma unroll
        for (int k = 0; k < SPEC_MAX_N; k++)
        {
            int b = best[k];
            for (int mask = 1; mask < 64; mask <<= 1) { const int o = (int)shfl_xor_u32((u32)b, mask); b = o > b ? o : b; }
            if (lane_id() == 0) s_best[wave_id()][k] = b;
        }
    }
    block_sync();
    if (t != 0) return;

    const int tail = s_pat[0];
    int src = -1;                               // the draft continues behind sequence index src - 1
    if (!a.forced)
    {
        const int nw = nthreads() >> 6;
        for (int n = N; n >= 1 && src < 0; n--)
        {
            int b = -1;
            for (int w = 0; w < nw; w++) b = s_best[w][n - 1] > b ? s_best[w][n - 1] : b;
            if (b >= 0) src = b + 1;
        }
    }
    int draft[SPEC_MAX_K];
    for (int i = 0; i < K; i++)
    {
        int d = tail;
        if (a.forced) { if (L + i < a.forced_len) d = a.forced[L + i]; }
        // overlapping copy: src + i < L + i, a source behind the sequence's end is a draft made earlier in this loop
        else if (src >= 0) d = src + i < L ? tok(src + i) : draft[src + i - L];
        draft[i] = d;
        a.ids[1 + i] = d;
    }
    if (a.draft_only) return;
    a.ids[0] = s_cand[n_acc];
    a.pos[0] = p1;
    a.stats[0] += 1;
    a.stats[1] += n_acc;
    a.stats[2 + n_acc] += 1;
    // one random point per emitted token, as unspeculated sampled decoding consumes them (the rows read counter + r)
    if (a.rand_counter) a.rand_counter[0] += n_acc + 1;
}

extern "C" {

int exl2_spec_accept_draft2(const int* cand, int* ids, int* history, int* pos, int* stats, const int* forced, int forced_len,
                            int K, int ngram, int hist_len, int draft_only, int* rand_counter, void* stream)
{
    EXL2_REQUIRE(ids && history && pos, "spec_accept_draft: null argument");
    EXL2_REQUIRE(draft_only || (cand && stats), "spec_accept_draft: the accept step needs cand and stats");
    EXL2_REQUIRE(K >= 1 && K <= SPEC_MAX_K, "spec_accept_draft: K %d must be in 1..%d", K, SPEC_MAX_K);
    EXL2_REQUIRE(ngram >= 1 && ngram <= SPEC_MAX_N, "spec_accept_draft: n-gram context %d must be in 1..%d", ngram, SPEC_MAX_N);
    EXL2_REQUIRE(hist_len >= K + 2, "spec_accept_draft: hist_len %d holds no step of %d rows", hist_len, K + 1);
    EXL2_REQUIRE(!forced || forced_len >= 0, "spec_accept_draft: forced_len %d", forced_len);
    const SpecArgs a{cand, ids, history, pos, stats, forced, rand_counter, forced ? forced_len : 0, K, ngram, hist_len, draft_only ? 1 : 0};
    // every thread takes one j per stride: a short log does not need sixteen waves to meet at the barriers
    LAUNCH(spec_accept_draft_kernel, dim3(1), dim3(hist_len <= 4096 ? 256 : 1024), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return EXL2_OK;
}

int exl2_spec_accept_draft(const int* cand, int* ids, int* history, int* pos, int* stats, const int* forced, int forced_len,
                           int K, int ngram, int hist_len, int draft_only, void* stream)
{
    return exl2_spec_accept_draft2(cand, ids, history, pos, stats, forced, forced_len, K, ngram, hist_len, draft_only, nullptr, stream);
}

}  // extern "C"
