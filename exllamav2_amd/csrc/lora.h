// lora.h -- low-rank adapters next to the quantized projections (lora.hip): the adapter table of one GROUP of projections that read
// the same rows (q | k | v, gate | up, a single o or down) and its two launches.
#pragma once
#include "hw.h"

#define LORA_MAX_PROJ 3            // projections per group
#define LORA_MAX_ACTIVE 8          // adapters per call
#define LORA_MAX_RANK 256

struct LoraGroup;

// a group over n_proj projections [K, N[p]] for calls of up to max_rows rows; owns its copies of the adapters and its scratch
int lora_group_make(LoraGroup** out, int n_proj, int K, const int* N, int max_rows);
void lora_group_free(LoraGroup* g);
// Replaces the table: n adapters, a / b / rank [n * n_proj] (adapter-major; a null pointer or rank 0 = the adapter has no entry for that
// projection), a fp16 [K, rank], b fp16 [rank, N] row-major.  Synchronises (load time).  Returns the largest rank, < 0 on error.
int lora_group_set(LoraGroup* g, int n, const u64* ids, const void* const* a, const void* const* b, const int* rank);
// out[p][rows, N[p]] += sum over the listed adapters that have an entry for p of fp16(x A) B: at most two launches, nothing when no
// listed adapter is in the table.  g may be null (no table: nothing to do).
int lora_group_apply(LoraGroup* g, int n_ids, const u64* ids, const f16* x, f16* const* out, int rows, void* stream);
