// Token-level unlikelihood term of one packed row (Welleck et al. 2019, arXiv:1908.04319) on top of sat_ce_ls.h's label-smoothed
// cross entropy: the arithmetic that ce_rows_ul_kernel (sat_elementwise.hip, f32 gradient) and ce_rows_ul_bf16grad_kernel
// (sat_gemm_bf16.hip, bf16 gradient) share.  Packed rows are time-major: row n = prefix[t] + b is step t of sequence b.  With
// y the row's target, p = softmax(x), lse as in sat_ce_ls.h:
//     C      = { targets[prefix[s] + b] : 0 <= s < t } \ { y }       (a SET: ids clamped into [0, V-1], each counted once)
//     q_c    = 1 - p_c
//     ul     = sum_{c in C} -log(max(q_c, 1e-5))
//     w_c    = q_c > 1e-5 ? p_c / q_c : 0                            (torch's clamp(min=1e-5): no gradient where it clamps)
//     W      = sum_{c in C} w_c
//     loss   = ce_ls_loss(nll, smooth) + alpha * ul
//     g[v]   = (p_v * (1 - alpha * W) - (v == y ? hit : uni) + (v in C ? alpha * w_v : 0)) * inv_denom
// Both sums run over the set's representatives in ascending order of first occurrence s, serially, so a row's outputs depend
// only on its own logits and its own prefix.  alpha == 0 (or t == 0) takes no candidates: the scale is exactly 1 and the addend
// exactly 0, which leaves the bits of sat_ce_ls.h's gradient.
#pragma once
#include "sat_ce_ls.h"

#define SAT_UL_MAX_T 64
#define SAT_UL_QMIN 1e-5f
#define SAT_UL_HASH 2048

// LDS of one workgroup.  `slot[id % SAT_UL_HASH]` is 1 + the lane (= step s) of a representative whose id hashes there, 0 for none:
// a byte per entry, so that the lanes of the one wave that fills it never share a word they modify (no atomics), and the four
// entries of an aligned 16-byte chunk of the row are one 32-bit read.  Two representatives whose ids collide leave either lane and
// set `clash`: only then does ce_ul_addend search `id` (a column that merely aliases a member, v + 2048 k, is a plain miss --
// searching for those cost 24 us per call at [1216, 10000]).
struct CeUlShared {
    alignas(4) unsigned char slot[SAT_UL_HASH];
    int id[SAT_UL_MAX_T];           // id[s]: the representative first seen at step s, -1 where step s adds no member
    float aw[SAT_UL_MAX_T];         // alpha * w_c of that representative
    float ul, W;
    int clash;                      // two candidate ids of this row differ by a multiple of SAT_UL_HASH
};

// (t, b) of packed row `row` from prefix[0..T] (T <= 64, prefix[0] == 0, row < prefix[T]): lane l of every wave holds prefix[l + 1],
// t is the number of those that are <= row.  `pstart` is prefix[lane] afterwards (the first row of step `lane`, for lane < T).
__device__ __forceinline__ int ce_ul_locate(const int32_t* __restrict__ prefix, int T, int row, int& b, int& pstart) {
    const int lane = threadIdx.x & 63;
    const int pe = lane < T ? prefix[lane + 1] : 0x7fffffff;
    const int t = __popcll(__ballot(pe <= row));
    const int up = __shfl_up(pe, 1, 64);
    pstart = lane ? up : 0;
    b = row - (t ? __shfl(pe, t - 1, 64) : 0);
    return t;
}

__device__ __forceinline__ void ce_ul_clear(CeUlShared& u) {
    for (int i = threadIdx.x; i < SAT_UL_HASH / 4; i += 256) ((unsigned*)u.slot)[i] = 0u;
}

// The candidates of one row, by ONE wave (all 64 lanes call it, t >= 1, u.slot cleared and a barrier since): lane s < t gathers the
// target of step s of its sequence and, where it is the first occurrence of an id other than y, that id's logit from x[].  n_rows
// bounds the gather (a prefix that is not PackInfo's must not read outside targets[]).  The caller's barrier after this call
// publishes `u` -- and, with an in-place gradient, is what orders these reads of x[] before any overwrite of the row.
__device__ __forceinline__ void ce_ul_candidates(const float* x, const int64_t* __restrict__ targets, int n_rows, int pstart, int t, int b,
                                                 int y, int V, float lse, float alpha, CeUlShared& u) {
    const int lane = threadIdx.x & 63;
    int c = -1;
    if (lane < t) {
        int r = pstart + b;
        r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
        const long v = targets[r];
        c = (int)(v < 0 ? 0 : (v >= V ? V - 1 : v));
    }
    bool rep = lane < t && c != y, clash = false;
    for (int j = 0; j < t; ++j) {
        const int cj = __shfl(c, j, 64);
        if (j < lane && cj == c) rep = false;
        if (cj != c && ((cj ^ c) & (SAT_UL_HASH - 1)) == 0) clash = true;      // (conservative: cj may be y, which is no member)
    }
    const bool any_clash = __ballot(clash && lane < t) != 0ull;
    float term = 0.0f, w = 0.0f;
    if (rep) {
        const float p = expf(x[c] - lse), q = 1.0f - p;
        term = -logf(fmaxf(q, SAT_UL_QMIN));
        w = q > SAT_UL_QMIN ? p / q : 0.0f;
    }
    float ul = 0.0f, W = 0.0f;                  // serial, ascending s; a lane that adds no member adds an exact 0
    for (int j = 0; j < t; ++j) {
        ul += __shfl(term, j, 64);
        W += __shfl(w, j, 64);
    }
    u.id[lane] = rep ? c : -1;
    u.aw[lane] = alpha * w;
    if (rep) u.slot[c & (SAT_UL_HASH - 1)] = (unsigned char)(lane + 1);
    if (lane == 0) {
        u.ul = ul;
        u.W = W;
        u.clash = any_clash ? 1 : 0;
    }
}

// alpha * w_v of column v if v is a member, else 0; `slot` is u.slot[v % SAT_UL_HASH], `clash` is u.clash
__device__ __forceinline__ float ce_ul_addend(const CeUlShared& u, unsigned slot, int v, int t, bool clash) {
    if (slot == 0u) return 0.0f;
    if (u.id[slot - 1] == v) return u.aw[slot - 1];
    if (!clash) return 0.0f;
    for (int s = 0; s < t; ++s)                 // two members share the hash entry
        if (u.id[s] == v) return u.aw[s];
    return 0.0f;
}

__device__ __forceinline__ float ce_ul_loss(const CeLsCoef& k, float nll, float smooth, float alpha, float ul) {
    const float ce = ce_ls_loss(k, nll, smooth);
    return alpha == 0.0f ? ce : ce + alpha * ul;
}

// scale = 1 - alpha * W (exactly 1 without candidates), addend = ce_ul_addend (exactly 0 there)
__device__ __forceinline__ float ce_ul_grad(const CeLsCoef& k, float x, float lse, bool is_target, float scale, float addend,
                                            float inv_denom) {
    return (expf(x - lse) * scale - (is_target ? k.hit : k.uni) + addend) * inv_denom;
}
