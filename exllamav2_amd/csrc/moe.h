// moe.h -- host interface of the MoE front kernel (moe.hip) beyond its C-ABI entry, used by modules.hip
#pragma once
#include "hw.h"

#define MOE_MAX_SEL 8
// argument-block copies made by the front kernel of a ONE-row step: for k = 0, 1 (the gate|up and the down launch) the block of the
// y-th selected expert e (ascending e) is copied from src[k] + e * units[k] to dst[k] + y * units[k] (16-byte units); n_sel = top-k
// sum[k]: table k gets ONE block = the first selected expert's, with units [b_lo, b_hi) and [b2_lo, b2_hi) from the second selected
// expert's (qgemv_lean.h: LeanGroupPlan.pair_sum; n_sel = 2)
struct MoeCopy { const u32x4* src[2]; u32x4* dst[2]; int units[2]; int n_sel; int sum[2], b_lo[2], b_hi[2], b2_lo[2], b2_hi[2]; };

// exl2_moe_front + the copies (cp nullable); 0 = launched, 1 = shape outside it
int moe_front_launch(const void* x, const void* norm_w, const void* gate, const void* perm, void* xn, void* xg, void* logits,
                     int rows, int hidden, int num_experts, int topk, float eps, const MoeCopy* cp, void* stream);

// ---- wide expert counts (64, 128): pair jobs ----------------------------------------------------------------------------------------
#define MOE_WIDE_MAX_ROWS 16                              // rows of one pass
#define MOE_WIDE_MAX_JOBS (MOE_WIDE_MAX_ROWS * MOE_MAX_SEL)
#define MOE_WIDE_PATCHES 3
static inline bool moe_wide_experts(int e) { return e == 64 || e == 128; }
// one pointer field of a job's argument block: the 8 bytes at byte offset `off` (8-byte aligned; < 0 = unused) become
// base + job * per_job + row * per_row + expert * per_expert (bytes)
struct MoePatch { int off; u32 per_job, per_row, per_expert; u64 base; };
// the hand-out of a pass: job j = r * topk + y runs the y-th selected expert e of row r (ascending e) as a one-row launch unit -- for
// k = 0, 1 (the gate|up and the down launch) the expert's planned block src[k] + e * units[k] is copied to dst[k] + j * units[k] with the
// job's pointers patched in.  sel_e / sel_w [rows, topk]: the compact list the combine kernel reads.  units[k] == 0: no copies.
struct MoeWide { const u32x4* src[2]; u32x4* dst[2]; int units[2]; MoePatch patch[2][MOE_WIDE_PATCHES]; int* sel_e; f16* sel_w; };

// the front of a wide block in two launches: logits on E / 4 workgroups per row (norm_w != null: x is the raw residual row, the norm
// is recomputed per workgroup, xn / xg are written; norm_w == null: x is the normalised row), then select + hand-out, one workgroup
// per row.  wd nullable.  0 = launched, 1 = shape outside it
int moe_wide_front_launch(const void* x, const void* norm_w, const void* gate, const void* perm, void* xn, void* xg, void* logits,
                          int rows, int hidden, int num_experts, int topk, float eps, const MoeWide* wd, void* stream);
