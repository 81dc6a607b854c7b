// Beam decode helpers (the reference has a stub only, model2.py:113-114; greedy loop models.py:56-67).
// One decode step per image = log-softmax of K rows of logits + top-K over the K*V candidates + LSTM state
// re-ordering by parent; the sequences are recovered at the end by walking the (parent, token) back-pointers.
// HBM/L2-bound byte/compare work, two launches per step:
//   beam_row_kernel   one workgroup per (image, hypothesis) row, the row read ONCE into registers: log-sum-exp and the
//                     row's K best continuations (thread-local sorted lists in registers, K rounds of block arg-best);
//   beam_merge_kernel one wave per image: the K best of its K*K row candidates.
//   (beam_merge_groups_kernel in its place for a diverse beam search: the K slots as groups that select in order, each under a
//   penalty for the tokens the groups in front chose at this step)
// The union of per-row top-K lists contains the global top-K, and both kernels order candidates by (score desc, flat
// index k*V+v asc), so the result is the exact top-K with a deterministic tie rule.
#include "sat_decode_state.h"
#include <limits.h>

namespace {

constexpr int KMAX = 8;   // beam width limit (thread-local candidate lists live in registers; K*K <= one wave)
constexpr int RC = 12;    // 16-byte chunks of a logits row a thread keeps in registers (V >> 2 <= 3072, i.e. V <= 12291: read once)

// a better than b: higher score, ties -> lower flat candidate index (k*V + v)
__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// wave-wide arg-best of (value, index) under `better`, the result in every lane: four DPP row rotations (8, 4, 2, 1: an all-reduce
// inside each row of 16 lanes -- the operation is commutative and idempotent) and the four row results by readlane
template <int CTRL>
__device__ __forceinline__ void argbest_step(float& v, int& i) {
    const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
    const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, false);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_argbest(float& v, int& i) {
    argbest_step<0x128>(v, i);      // row_ror:8
    argbest_step<0x124>(v, i);      // row_ror:4
    argbest_step<0x122>(v, i);      // row_ror:2
    argbest_step<0x121>(v, i);      // row_ror:1
    float bv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        const float qv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16 * q));
        const int qi = __builtin_amdgcn_readlane(i, 16 * q);
        if (better(qv, qi, bv, bi)) { bv = qv; bi = qi; }
    }
    v = bv;
    i = bi;
}

template <int NT>
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* sh) {
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];      // wave order: fixed
    return r;
}

// insert (cv, ci) into a list sorted by (value desc, index asc); the caller visits candidates in increasing index
// order, so an equal value goes BEHIND the ones already stored
__device__ __forceinline__ void list_insert(float (&val)[KMAX], int (&idx)[KMAX], float cv, int ci) {
    bool shifted = false;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        const bool sw = shifted || cv > val[j];
        const float tv = val[j];
        const int ti = idx[j];
        if (sw) {
            val[j] = cv;
            idx[j] = ci;
            cv = tv;
            ci = ti;
        }
        shifted = sw;
    }
}

// One workgroup of NT threads per (image, hypothesis) row.  Round 5: the selection no longer keeps a sorted top-K list per thread
// (an insert per element that beats the list's tail: 11 k instructions per wave at V = 10 000, the kernel was instruction-bound at
// 33 us per 320 rows).  Now: a thread keeps only its single best candidate; K rounds of block arg-best; the wave that owned the
// winner strikes it out and finds its threads' next best -- the other waves skip that.  Exactly the same result: the K best
// candidates of the row under (score desc, flat index asc).
//
// CONSTRAINED (sat_beam_step_ex, include/sat_hip.h): the row's banned columns are struck from the candidates AFTER the log-sum-exp
// over the whole row (scores are not renormalised).  The bans live in an LDS bitmap of V bits: every thread clears its words, one
// barrier, then wave 0 alone gathers them -- the suppressed ids, end_id in front of min_length, and the row's own prefix, which it
// recovers by walking the (parents, tokens) records from step i - 1 down (every lane walks the same chain, the loads are wave
// broadcasts, both loads of a level in flight together; lane t keeps y_t in a register and the n-gram compare reads its neighbours
// by ds_bpermute).  sat_beam_decode_ex, which owns a workspace, spares the walk under n-gram blocking: it keeps every slot's prefix
// in two [B*K][64] planes, and a row reads ONE level of the chain plus its parent's prefix row and writes its own (BeamBan::hist_*).
// The other waves meanwhile have their row loads in flight and wait in the first block reduction, whose barriers also publish the
// bitmap.  A thread then tests ONE bitmap word per 16-byte chunk it holds: chunk q is bits 4q..4q+3 = a nibble of
// word q >> 3, so 8 neighbouring lanes read one word (a broadcast) and a wave reads 8 consecutive words: no bank conflict.  The row
// in registers is only ever indexed by unrolled constants.  Finished and dead rows leave before any of this.
struct BeamBan {
    const int64_t* suppress;     // device [n_suppress]
    const int32_t* parents;      // records [T][B*K], rows < i valid
    const int64_t* tokens;
    int n_suppress, min_length, ngram, block_repeat, i;
    const int* hist_in;          // sat_beam_decode_ex only: [B*K][kBanTMax], slot s's prefix as it stood BEFORE step i - 1's selection
    int* hist_out;               //   ... and the prefixes of this step's rows (NULL: the prefix is walked from the records)
};
constexpr int kBanTMax = 64;     // steps a constrained decode may have (lane t of the walking wave keeps y_t)
constexpr int kBanVMax = 65536;  // columns of the LDS ban bitmap (8 KiB)

template <int NT, bool CONSTRAINED>
__device__ __forceinline__ void beam_row_body(const float* __restrict__ logits, long ldl, const float* __restrict__ scores_in,
                                              const int64_t* __restrict__ last_tok, long end_id, int K, int V,
                                              float* __restrict__ cand_val, int* __restrict__ cand_idx, const BeamBan& ban,
                                              unsigned* s_ban) {
    constexpr int NW = NT / 64, RCN = RC * 256 / NT;          // waves; 16-byte chunks of the row a thread keeps in registers
    __shared__ float sh[NW];
    __shared__ float s_rv[NW];
    __shared__ int s_ri[NW];
    __shared__ float s_cv[NW * KMAX];
    __shared__ int s_ci[NW * KMAX];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int k = row % K;
    const float base = scores_in[row];
    const bool frozen = last_tok != nullptr && end_id >= 0 && last_tok[row] == end_id;
    float* cv_out = cand_val + (long)row * K;
    int* ci_out = cand_idx + (long)row * K;
    if (base == -INFINITY || frozen) {              // uniform across the block: a dead or a finished hypothesis
        if (tid < K) {
            // finished: one continuation, end_id again at unchanged score; dead: nothing
            const bool live = frozen && base != -INFINITY && tid == 0 && end_id < V;
            cv_out[tid] = live ? base : -INFINITY;
            ci_out[tid] = live ? k * V + (int)end_id : INT_MAX;
        }
        return;
    }
    const float* x = logits + (long)row * ldl;
    const int nq = V >> 2;                                   // whole 16-byte chunks (rows are 16-byte aligned: ldl % 4 == 0)
    if constexpr (CONSTRAINED) {
        for (int w = tid; w < (V + 31) >> 5; w += NT) s_ban[w] = 0u;
        __syncthreads();
        if (tid < 64) {                                      // wave 0 gathers the bans; the first block reduction publishes them
            auto set = [&](long v) {
                if (v >= 0 && v < V) atomicOr(&s_ban[v >> 5], 1u << (v & 31));
            };
            for (int j = tid; j < ban.n_suppress; j += 64) set((long)ban.suppress[j]);
            if (tid == 0 && ban.i < ban.min_length) set(end_id);
            const int i = ban.i, n = ban.ngram;
            const bool grams = n >= 1 && i >= n;
            const int depth = (grams || (ban.hist_out && i >= 1)) ? i : (ban.block_repeat && i >= 1 ? 1 : 0);
            if (depth > 0) {
                const long BK = gridDim.x, at0 = row - k;    // (b * K)
                int cur = k, y = -1;                         // y: y_t in lane t
                if (ban.hist_out) {
                    // the decode loop keeps every slot's prefix: ONE level of the chain (this row's parent and last token), then the
                    // parent's prefix as one coalesced row -- instead of i dependent levels
                    const long at = (long)(i - 1) * BK + row;
                    const int64_t tk = ban.tokens[at];
                    const int pr = ban.parents[at];
                    cur = pr < 0 ? 0 : (pr >= K ? K - 1 : pr);
                    if (tid < i - 1) y = ban.hist_in[(at0 + cur) * kBanTMax + tid];
                    if (tid == i - 1) y = (tk >= 0 && tk < V) ? (int)tk : -1;
                    if (tid < i) ban.hist_out[(long)row * kBanTMax + tid] = y;
                }
                for (int t = i - 1; t >= i - depth && !ban.hist_out; --t) {
                    const long at = (long)t * BK + at0 + cur;
                    const int64_t tk = ban.tokens[at];
                    const int pr = ban.parents[at];
                    if (tid == t) y = (tk >= 0 && tk < V) ? (int)tk : -1;
                    cur = pr < 0 ? 0 : (pr >= K ? K - 1 : pr);                  // memory safety only: the steps write 0..K-1
                }
                if (ban.block_repeat && tid == i - 1) set(y);
                if (grams) {
                    // lane j: the n-gram that starts at j, 0 <= j <= i - n, bans its last token when its first n - 1 equal the tail
                    bool same = true;
                    for (int m = 0; m + 1 < n; ++m) {        // (both reads by the whole wave: no short-circuit around a bpermute)
                        const int mine = __shfl(y, (tid + m) & 63, 64), tail = __shfl(y, i - n + 1 + m, 64);
                        same = same & (mine == tail);
                    }
                    const int lastv = __shfl(y, (tid + n - 1) & 63, 64);
                    if (tid <= i - n && same) set(lastv);
                }
            }
        }
    }
    // (V < 4 has no whole chunk to clamp the out-of-row chunk indexes to -- nq - 1 would be the 16 bytes IN FRONT of the row: such
    // rows take the long-row path below)
    if ((ldl & 3) == 0 && nq >= 1 && nq <= RCN * NT) {
        // the row lives in registers: ONE pass over memory (every load unconditional, chunk indexes past the row clamped and
        // ignored below: a load under a runtime condition makes the compiler branch around each one and wait for it alone)
        f32x4 rc[RCN];
#pragma unroll
        for (int c = 0; c < RCN; ++c) {
            const int q = tid + c * NT;
            rc[c] = *(const f32x4*)(x + 4 * (q < nq ? q : nq - 1));
        }
        const int tail = (nq << 2) + tid;                    // V % 4 leftover elements, one per thread
        float xt = tail < V ? x[tail] : -INFINITY;
#pragma unroll
        for (int c = 0; c < RCN; ++c)
            if (tid + c * NT >= nq) rc[c] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};       // (a select on the VALUE)
        float m = xt;
#pragma unroll
        for (int c = 0; c < RCN; ++c) m = fmaxf(fmaxf(fmaxf(m, rc[c][0]), fmaxf(rc[c][1], rc[c][2])), rc[c][3]);
        m = block_reduce<NT>(m, true, sh);
        // exp(x - m) as ONE fma and ONE v_exp_f32 per element (2^(x log2e - m log2e); 1 ulp, arguments <= 0, exp(-inf) = 0 for the
        // padding): libm's expf is ~8 instructions per element with its range fix-ups, and this loop is a third of the kernel's
        // instructions
        const float ml = m * 1.44269504088896340736f;
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < RCN; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) s += __builtin_amdgcn_exp2f(__builtin_fmaf(rc[c][e], 1.44269504088896340736f, -ml));
        }
        s += __builtin_amdgcn_exp2f(__builtin_fmaf(xt, 1.44269504088896340736f, -ml));
        s = block_reduce<NT>(s, false, sh);
        const float lse = m + logf(s);
        // candidate scores in place (the f32 expression the step-by-step oracle rounds: base + (x - lse)); -inf stays -inf
#pragma unroll
        for (int c = 0; c < RCN; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) rc[c][e] = base + (rc[c][e] - lse);
        xt = base + (xt - lse);
        if constexpr (CONSTRAINED) {                         // banned columns are no candidates (one bitmap word per chunk)
#pragma unroll
            for (int c = 0; c < RCN; ++c) {
                const int q = tid + c * NT;
                const unsigned nib = s_ban[q < nq ? q >> 3 : 0] >> (4 * (q & 7));
#pragma unroll
                for (int e = 0; e < 4; ++e) rc[c][e] = ((nib >> e) & 1u) ? -INFINITY : rc[c][e];
            }
            if (tail < V && ((s_ban[tail >> 5] >> (tail & 31)) & 1u)) xt = -INFINITY;
        }
        // this thread's best TWO (elements in increasing index order: strict > keeps the lower index among equals in front)
        float v1 = -INFINITY, v2 = -INFINITY;
        int i1 = INT_MAX, i2 = INT_MAX;
        auto offer = [&](float xv, int xi) {
            const bool a = xv > v1, b2 = xv > v2;
            v2 = a ? v1 : (b2 ? xv : v2);
            i2 = a ? i1 : (b2 ? xi : i2);
            v1 = a ? xv : v1;
            i1 = a ? xi : i1;
        };
#pragma unroll
        for (int c = 0; c < RCN; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) offer(rc[c][e], k * V + 4 * (tid + c * NT) + e);
        offer(xt, k * V + tail);
        if (v1 == -INFINITY) i1 = INT_MAX;                   // (padding / -inf logits are no candidates)
        if (v2 == -INFINITY) i2 = INT_MAX;
        // the best element of this thread that comes AFTER (pv, pi) in the order (score desc, index asc): the rare third pop
        auto local_next = [&](float pv, int pi, float& bv, int& bi) {
            bv = -INFINITY;
            bi = INT_MAX;
            auto see = [&](float xv, int xi) {
                const bool after = xv < pv || (xv == pv && xi > pi);
                if (after && xv > bv) { bv = xv; bi = xi; }
            };
#pragma unroll
            for (int c = 0; c < RCN; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) see(rc[c][e], k * V + 4 * (tid + c * NT) + e);
            see(xt, k * V + tail);
        };
        // Selection without block barriers in the rounds (round 5, second form): every WAVE extracts the K best of its own quarter of
        // the row -- K rounds of a wave-wide arg-best over the threads' current heads on DPP row rotations + four readlanes (no LDS
        // crossbar, no barrier); the owner lane pops its head (its second best is at hand; a third pop rescans, rarely) -- then ONE
        // barrier and wave 0 picks the K best of the NW * K survivors the same way.  The union of the waves' lists contains the row's
        // K best, and every comparison uses (score desc, flat index asc): the result is exactly the one of block-wide rounds.
        const int lane = tid & 63, wave = tid >> 6;
        int pops = 0;
        for (int r = 0; r < K; ++r) {
            float bv = v1;
            int bi = i1;
            wave_argbest(bv, bi);
            if (lane == 0) { s_cv[wave * KMAX + r] = bv; s_ci[wave * KMAX + r] = bi; }
            if (i1 == bi && bi != INT_MAX) {                 // the owner lane (candidate indexes are unique)
                if (pops == 0) {
                    v1 = v2;
                    i1 = i2;
                } else {
                    float nv;
                    int ni;
                    local_next(bv, bi, nv, ni);
                    v1 = nv;
                    i1 = ni;
                }
                ++pops;
            }
        }
        __syncthreads();
        if (wave == 0) {
            const bool has = lane < NW * K;
            float cv = has ? s_cv[(lane / K) * KMAX + lane % K] : -INFINITY;
            int ci = has ? s_ci[(lane / K) * KMAX + lane % K] : INT_MAX;
            for (int r = 0; r < K; ++r) {
                float bv = cv;
                int bi = ci;
                wave_argbest(bv, bi);
                if (lane == 0) { cv_out[r] = bv; ci_out[r] = bi; }
                if (ci == bi) { cv = -INFINITY; ci = INT_MAX; }
            }
        }
        return;
    }
    // rows too long for the registers: thread-local sorted lists over three passes
    float val[KMAX];
    int idx[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        val[j] = -INFINITY;
        idx[j] = INT_MAX;
    }
    {
        float m = -INFINITY;
        for (int i = tid; i < V; i += NT) m = fmaxf(m, x[i]);
        m = block_reduce<NT>(m, true, sh);
        float s = 0.0f;
        for (int i = tid; i < V; i += NT) s += expf(x[i] - m);
        s = block_reduce<NT>(s, false, sh);
        const float lse = m + logf(s);
        for (int i = tid; i < V; i += NT) {
            if constexpr (CONSTRAINED) {
                if ((s_ban[i >> 5] >> (i & 31)) & 1u) continue;
            }
            const float cv = base + (x[i] - lse);
            if (cv > val[KMAX - 1]) list_insert(val, idx, cv, k * V + i);
        }
    }
    // K rounds of block arg-best over the list heads; the winner pops its head
    for (int r = 0; r < K; ++r) {
        float bv = val[0];
        int bi = idx[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if ((tid & 63) == 0) {
            s_rv[tid >> 6] = bv;
            s_ri[tid >> 6] = bi;
        }
        __syncthreads();
        bv = s_rv[0];
        bi = s_ri[0];
#pragma unroll
        for (int w = 1; w < NW; ++w)
            if (better(s_rv[w], s_ri[w], bv, bi)) {
                bv = s_rv[w];
                bi = s_ri[w];
            }
        if (idx[0] == bi && bi != INT_MAX) {          // candidate indices are unique across threads
#pragma unroll
            for (int j = 0; j + 1 < KMAX; ++j) {
                val[j] = val[j + 1];
                idx[j] = idx[j + 1];
            }
            val[KMAX - 1] = -INFINITY;
            idx[KMAX - 1] = INT_MAX;
        }
        if (tid == 0) {
            cv_out[r] = bv;
            ci_out[r] = bi;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void beam_row_kernel(const float* __restrict__ logits, long ldl,
                                                      const float* __restrict__ scores_in,
                                                      const int64_t* __restrict__ last_tok, long end_id, int K, int V,
                                                      float* __restrict__ cand_val, int* __restrict__ cand_idx) {
    beam_row_body<NT, false>(logits, ldl, scores_in, last_tok, end_id, K, V, cand_val, cand_idx, BeamBan{}, nullptr);
}

template <int NT>
__global__ __launch_bounds__(NT) void beam_row_ban_kernel(const float* __restrict__ logits, long ldl,
                                                          const float* __restrict__ scores_in,
                                                          const int64_t* __restrict__ last_tok, long end_id, int K, int V,
                                                          float* __restrict__ cand_val, int* __restrict__ cand_idx, BeamBan ban) {
    __shared__ unsigned s_ban[kBanVMax / 32];
    beam_row_body<NT, true>(logits, ldl, scores_in, last_tok, end_id, K, V, cand_val, cand_idx, ban, s_ban);
}

// the second half of both merge kernels: behind ONE barrier all four waves move the rows of the next step -- the embedding row of the
// chosen token and, in the wide decode path, the (h, c) rows of the hypothesis it extends -- every row by its own wave with all its
// loads in flight at once
__device__ __forceinline__ void beam_move_rows(const int* s_par, const int* s_tok, int b, int K, int lane, int wave,
                                               const float* __restrict__ embed, int E, float* __restrict__ x_next, long ldx,
                                               const float* __restrict__ h_src, const float* __restrict__ c_src, int H,
                                               float* __restrict__ h_dst, long ldh, float* __restrict__ c_dst) {
    if (!embed && !h_src) return;                          // (uniform)
    __syncthreads();
    for (int r = wave; r < K; r += 4) {
        const int par = s_par[r], tok = s_tok[r];
        const long to = (long)(b * K + r);
        if (embed) {                                       // the next step's input row: embed(token) (models.py:64)
            const float* src = embed + (long)tok * E;
            for (int e = lane * 4; e < E; e += 256) *(f32x4*)(x_next + to * ldx + e) = *(const f32x4*)(src + e);
        }
        if (h_src) {                                       // ... and the LSTM state of the hypothesis it extends
            const long from = (long)(b * K + par) * H;
            for (int e = lane * 4; e < H; e += 256) {
                const f32x4 hv = *(const f32x4*)(h_src + from + e), cv = *(const f32x4*)(c_src + from + e);
                *(f32x4*)(h_dst + to * ldh + e) = hv;
                *(f32x4*)(c_dst + to * H + e) = cv;
            }
        }
    }
}

// One workgroup of 256 threads per image: wave 0 merges (K rounds of a wave-wide arg-best over the image's K * K row candidates), then
// -- one barrier -- all four waves move the rows of the next step: embedding row of the chosen token and, in the wide decode path, the
// (h, c) rows of the hypothesis it extends, every row by its own wave with all its loads in flight at once (the copies used to sit
// inside the merge rounds, one dependent round trip per hypothesis: 6.2 + 4.8 us per step as two launches, 8.0 as one wave)
__global__ __launch_bounds__(256) void beam_merge_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                         int K, int V, int* __restrict__ parent,
                                                         int64_t* __restrict__ token, float* __restrict__ scores_out,
                                                         const float* __restrict__ embed, int E, float* __restrict__ x_next, long ldx,
                                                         const float* __restrict__ h_src, const float* __restrict__ c_src, int H,
                                                         float* __restrict__ h_dst, long ldh, float* __restrict__ c_dst) {
    __shared__ int s_par[KMAX], s_tok[KMAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        float v = -INFINITY;
        int ix = INT_MAX;
        if (lane < K * K) {
            v = cand_val[(long)b * K * K + lane];
            ix = cand_idx[(long)b * K * K + lane];
        }
        for (int r = 0; r < K; ++r) {
            float bv = v;
            int bi = ix;
            wave_argbest(bv, bi);                          // (bv, bi) are the same in every lane after the reduction
            if (ix == bi && bi != INT_MAX) {             // the winner leaves the pool
                v = -INFINITY;
                ix = INT_MAX;
            }
            const bool ok = bi != INT_MAX;
            const int par = ok ? bi / V : 0, tok = ok ? bi % V : 0;
            if (lane == 0) {
                parent[b * K + r] = par;
                token[b * K + r] = tok;
                scores_out[b * K + r] = ok ? bv : -INFINITY;
                s_par[r] = par;
                s_tok[r] = tok;
            }
        }
    }
    beam_move_rows(s_par, s_tok, b, K, lane, wave, embed, E, x_next, ldx, h_src, c_src, H, h_dst, ldh, c_dst);
}

// the selection key of a candidate that n slots of the groups in front chose at this step: ONE rounded multiply and ONE rounded
// subtract (no contraction into an fma: a plain f32 restatement rounds the same way)
__device__ __forceinline__ float beam_penalised_key(float s, float lambda, int n) {
#pragma clang fp contract(off)
    const float p = lambda * (float)n;
    return s - p;
}

// DIVERSE beam search (sat_beam_step_groups, include/sat_hip.h): beam_merge_kernel with the K slots of an image as G = K / Kg groups
// that select IN ORDER, each under the key s - lambda * n(v), n(v) = how many slots of the groups in front chose token v at this same
// step (finished rows' end_id and surplus slots do not count; a finished row's candidate is not penalised).  The carried score is the
// raw s.  Wave 0 holds the image's K * K row candidates, one per lane, as the plain merge does; lane j < K also keeps the token slot j
// chose (-1: it does not count), so n(v) is at most K compares against readlanes of wave-uniform slots.  Group g's keys are formed
// once, before its rounds -- the tokens of a group are published to the lanes' compares only by the next group's key pass, so they do
// not penalise each other -- then Kg rounds of wave_argbest: K rounds over the step, as many as the plain merge runs.
//
// LEMMA: group g's Kg winners under the key all lie within the raw top-K lists of group g's rows, which is all the row kernels leave.
// Take a candidate c outside its row's raw top K: at least K candidates of that row are ahead of it under (s desc, index asc).  At most
// g * Kg <= K - Kg distinct tokens are penalised, so at least Kg of those ahead are unpenalised and keep key = s; key(c) <= s(c)
// because lambda >= 0; so Kg candidates of its own row alone beat c under (key desc, index asc).
__global__ __launch_bounds__(256) void beam_merge_groups_kernel(const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                                int K, int V, int Kg, float lambda, const int64_t* __restrict__ last_tok,
                                                                long end_id, int* __restrict__ parent, int64_t* __restrict__ token,
                                                                float* __restrict__ scores_out, const float* __restrict__ embed, int E,
                                                                float* __restrict__ x_next, long ldx, const float* __restrict__ h_src,
                                                                const float* __restrict__ c_src, int H, float* __restrict__ h_dst, long ldh,
                                                                float* __restrict__ c_dst) {
    __shared__ int s_par[KMAX], s_tok[KMAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        float v = -INFINITY;
        int ix = INT_MAX;
        if (lane < K * K) {
            v = cand_val[(long)b * K * K + lane];
            ix = cand_idx[(long)b * K * K + lane];
        }
        const bool has = ix != INT_MAX;                    // (the row kernels leave INT_MAX with every -inf)
        const int slot = has ? ix / V : 0, tok = has ? ix - slot * V : -2, group = has ? slot / Kg : -1;
        const bool finished = has && last_tok != nullptr && end_id >= 0 && last_tok[b * K + slot] == end_id;
        int chosen = -1;                                   // lane j < K: the token slot j chose at this step, if it counts
        for (int g = 0; g * Kg < K; ++g) {
            int n = 0;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) n += (__builtin_amdgcn_readlane(chosen, j) == tok) ? 1 : 0;      // (tok >= 0 or -2; -1 matches none)
            const bool mine = group == g;
            float key = mine ? ((n > 0 && !finished) ? beam_penalised_key(v, lambda, n) : v) : -INFINITY;
            int kix = mine ? ix : INT_MAX;
            for (int r = 0; r < Kg; ++r) {
                float bv = key;
                int bi = kix;
                wave_argbest(bv, bi);                      // (bv, bi) are the same in every lane after the reduction
                const bool ok = bi != INT_MAX;
                const bool won = ok && kix == bi;          // at most one lane: candidate indexes are unique
                const unsigned long long who = __ballot(won);
                const int src = ok ? __ffsll((long long)who) - 1 : 0;
                const float raw = __shfl(v, src, 64);      // the carried score is the raw s of the winner, not its key
                const bool counts = ok && __ballot(won && !finished) != 0ull;
                if (won) {                                 // the winner leaves the pool
                    key = -INFINITY;
                    kix = INT_MAX;
                }
                const int to = g * Kg + r;
                const int par = ok ? bi / V : g * Kg, tk = ok ? bi % V : 0;
                if (lane == to) chosen = counts ? tk : -1;
                if (lane == 0) {
                    parent[b * K + to] = par;
                    token[b * K + to] = tk;
                    scores_out[b * K + to] = ok ? raw : -INFINITY;
                    s_par[to] = par;
                    s_tok[to] = tk;
                }
            }
        }
    }
    beam_move_rows(s_par, s_tok, b, K, lane, wave, embed, E, x_next, ldx, h_src, c_src, H, h_dst, ldh, c_dst);
}

// x0 row (b, k) = features[b]; scores: the first slot of every group of Kg live at 0, the others dead (Kg == K: hypothesis 0 alone)
__global__ __launch_bounds__(256) void beam_init_kernel(const float* __restrict__ features, int K, int E, long total,
                                                        float* __restrict__ x0, long ldx, float* __restrict__ scores, int R, int Kg) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / E;
        x0[row * ldx + (i - row * E)] = features[(row / K) * E + (i - row * E)];
    }
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < R) scores[t] = ((t % K) % Kg) == 0 ? 0.0f : -INFINITY;
}

// the (h, c) rows of one layer re-ordered by parent in ONE launch: dst row (b, k) = src row (b, parent[b, k])
__global__ __launch_bounds__(256) void beam_gather2_kernel(const float* __restrict__ h_src, const float* __restrict__ c_src,
                                                           const int* __restrict__ parent, int K, int W, long total,
                                                           float* __restrict__ h_dst, long ldh, float* __restrict__ c_dst) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < 2 * total; i += (long)gridDim.x * 256) {
        const bool second = i >= total;
        const long j = second ? i - total : i;
        const long row = j / W;
        const int col = (int)(j - row * W);
        const long b = row / K;
        const long from = (b * K + parent[row]) * W + col;
        if (second) c_dst[j] = c_src[from];
        else h_dst[row * ldh + col] = h_src[from];
    }
}

// wide decode steps (many rows, one LSTM layer): W_cat [4H][In + H] = [W_ih | W_hh], so that the step's gates are ONE GEMM over the
// concatenated input row [x | h]
__global__ __launch_bounds__(256) void beam_wcat_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, int In, int H,
                                                        long total, float* __restrict__ wcat) {
    const int ld = In + H;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / ld;
        const int col = (int)(i - row * ld);
        wcat[i] = col < In ? w_ih[row * In + col] : w_hh[row * H + (col - In)];
    }
}

// gates [R][4H] (i, f, g, o pre-activations, both biases in) -> c (in place), h_new: the LSTM cell's pointwise half (models.py:52)
// (nslab > 1: the gates arrive as K-split partial sums, slab z `slab` floats further on; summed here in slab order)
__global__ __launch_bounds__(256) void beam_lstm_point_kernel(const float* __restrict__ gates, float* __restrict__ c,
                                                              float* __restrict__ h_new, int H, long total, int nslab, long slab) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / H;
        const int u = (int)(i - row * H);
        const float* g = gates + row * 4 * H;
        float a0 = g[u], a1 = g[H + u], a2 = g[2 * H + u], a3 = g[3 * H + u];
        for (int z = 1; z < nslab; ++z) {
            const float* gz = g + z * slab;
            a0 += gz[u]; a1 += gz[H + u]; a2 += gz[2 * H + u]; a3 += gz[3 * H + u];
        }
        const float gi = sat_sigmoid(a0), gf = sat_sigmoid(a1), gg = sat_tanh(a2), go = sat_sigmoid(a3);
        const float cn = gf * c[i] + gi * gg;
        c[i] = cn;
        h_new[i] = go * sat_tanh(cn);
    }
}

// dst row (b,k) = src row (b, parent[b,k]); W floats per row
__global__ __launch_bounds__(256) void beam_gather_kernel(const float* __restrict__ src, const int* __restrict__ parent, int K,
                                                          int W, long total, float* __restrict__ dst) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / W;
        const int col = (int)(i - row * W);
        const long b = row / K;
        dst[i] = src[(b * K + parent[row]) * W + col];
    }
}

__global__ __launch_bounds__(256) void beam_backtrack_kernel(const int* __restrict__ parents, const int64_t* __restrict__ tokens,
                                                             int T, int BK, int K, int64_t* __restrict__ ids) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= BK) return;
    const int b = row / K;
    int cur = row - b * K;
    for (int t = T - 1; t >= 0; --t) {
        const long at = (long)t * BK + b * K + cur;
        ids[(long)row * T + t] = tokens[at];
        cur = parents[at];
    }
}

// The walk of beam_backtrack_kernel over a per-step record of f32 rows (the attention maps of a beam decode): one workgroup per
// final hypothesis (b, k).  The row of step t was computed BEFORE that step's selection, on the slot the survivor was expanded
// from, so it is read at the survivor's PARENT of step t -- which is also the slot the walk visits next.  Pure gather.
__global__ __launch_bounds__(64) void beam_backtrack_rows_kernel(const int* __restrict__ parents, const float* __restrict__ rows,
                                                                 int T, int BK, int K, int cols, float* __restrict__ out) {
    const int row = blockIdx.x;
    const int b = row / K;
    int cur = row - b * K;
    for (int t = T - 1; t >= 0; --t) {
        cur = parents[(long)t * BK + b * K + cur];
        cur = cur < 0 ? 0 : (cur >= K ? K - 1 : cur);                 // memory safety only: sat_beam_step writes 0..K-1
        const float* src = rows + ((long)t * BK + b * K + cur) * cols;
        float* dst = out + ((long)row * T + t) * cols;
        for (int c = threadIdx.x; c < cols; c += 64) dst[c] = src[c];
    }
}

// eval.py:103-109: the id -> word loop of `evaluation` stops at the first '<end>'.  One thread per caption row: the number of
// ids in front of the first end_id (T when there is none) -- the host then reads ids[b][:kept[b]] only.
__global__ __launch_bounds__(256) void kept_tokens_kernel(const int64_t* __restrict__ ids, long stride, int B, int T, int64_t end_id,
                                                          int32_t* __restrict__ kept) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t* row = ids + (long)b * stride;
    int n = 0;
    while (n < T && row[n] != end_id) ++n;
    kept[b] = n;
}

// Length-penalty re-ranking of a finished beam (sat_beam_rerank): one wave per image, lane k < K owns hypothesis k.  L_k as
// kept_tokens_kernel counts it, plus 1 for the <end> (T without one); norm in f64, rounded once; rank = how many hypotheses come in
// front under (norm desc, previous rank asc) -- a stable sort of K <= 8 keys by counting; then the wave copies the K id rows.
__global__ __launch_bounds__(64) void beam_rerank_kernel(const int64_t* __restrict__ ids, const float* __restrict__ scores, int K, int T,
                                                         int64_t end_id, float alpha, int64_t* __restrict__ ids_out,
                                                         float* __restrict__ scores_out, float* __restrict__ norm_out,
                                                         int32_t* __restrict__ order_out) {
    __shared__ int s_order[KMAX];
    const int b = blockIdx.x, lane = threadIdx.x;
    float sc = -INFINITY, norm = -INFINITY;
    if (lane < K) {
        const int64_t* row = ids + ((long)b * K + lane) * T;
        int n = 0;
        while (n < T && row[n] != end_id) ++n;
        const int len = n < T ? n + 1 : T;
        sc = scores[(long)b * K + lane];
        norm = alpha > 0.0f ? (float)((double)sc / pow((double)len, (double)alpha)) : sc;
    }
    if (lane < K) s_order[lane] = lane;                      // (NaN scores can leave a rank unclaimed: memory safety only)
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < K; ++j) {
        const float nj = __shfl(norm, j, 64);
        rank += (nj > norm || (nj == norm && j < lane)) ? 1 : 0;
    }
    if (lane < K) {
        rank = rank < K ? rank : K - 1;                      // (NaN scores: memory safety only)
        s_order[rank] = lane;
        const long at = (long)b * K + rank;
        scores_out[at] = sc;
        if (norm_out) norm_out[at] = norm;
        if (order_out) order_out[at] = lane;
    }
    __syncthreads();
    for (int r = 0; r < K; ++r) {
        const int64_t* src = ids + ((long)b * K + s_order[r]) * T;
        int64_t* dst = ids_out + ((long)b * K + r) * T;
        for (int t = lane; t < T; t += 64) dst[t] = src[t];
    }
}

// order[b, k] = k
__global__ __launch_bounds__(256) void beam_iota_kernel(int32_t* __restrict__ order, int R, int K) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < R) order[t] = t % K;
}

// the checks every constrained entry point makes before anything is enqueued; *active: a step constraint is on
int beam_constraints_check(const sat_beam_constraints* c, int64_t end_id, bool* active) {
    *active = false;
    if (!c) return SAT_OK;
    if (c->n_suppress < 0 || c->min_length < 0 || c->no_repeat_ngram < 0 || (c->block_repeat != 0 && c->block_repeat != 1))
        return SAT_ERR_ARG;
    if (c->n_suppress > 256 || (c->n_suppress > 0 && !c->suppress_ids)) return SAT_ERR_ARG;
    if (c->min_length > 0 && end_id < 0) return SAT_ERR_ARG;
    if (!(c->length_penalty >= 0.0f) || c->length_penalty == INFINITY) return SAT_ERR_ARG;
    *active = c->n_suppress > 0 || c->min_length > 0 || c->no_repeat_ngram > 0 || c->block_repeat != 0;
    return SAT_OK;
}

// does step i of a decode under c ban anything?  (a step that does not runs the plain row kernel: the same bits)
bool beam_step_bans(const sat_beam_constraints* c, int i) {
    return c->n_suppress > 0 || i < c->min_length || (c->no_repeat_ngram >= 1 && i >= c->no_repeat_ngram) || (c->block_repeat && i >= 1);
}

// the row launch of one step: the constrained kernel where the step bans something, the plain one otherwise
void beam_row_launch(hipStream_t s, const float* logits, long ldl, const float* scores_in, const int64_t* last, long end_id, int R, int K,
                     int V, float* cand_val, int* cand_idx, const sat_beam_constraints* c, const int32_t* parents, const int64_t* tokens,
                     int i, int* hist = nullptr) {
    // (hist: two [R][kBanTMax] planes; with n-gram blocking the constrained kernel then runs from step 1 on, to keep them)
    if (c && (beam_step_bans(c, i) || (hist && i >= 1))) {
        BeamBan ban;
        ban.suppress = c->suppress_ids;
        ban.parents = parents;
        ban.tokens = tokens;
        ban.n_suppress = c->n_suppress;
        ban.min_length = c->min_length;
        ban.ngram = c->no_repeat_ngram;
        ban.block_repeat = c->block_repeat;
        ban.i = i;
        ban.hist_in = hist ? hist + (long)((i + 1) & 1) * R * kBanTMax : nullptr;
        ban.hist_out = hist ? hist + (long)(i & 1) * R * kBanTMax : nullptr;
        hipLaunchKernelGGL(beam_row_ban_kernel<256>, dim3((unsigned)R), dim3(256), 0, s, logits, ldl, scores_in, last, end_id, K, V, cand_val,
                           cand_idx, ban);
    } else {
        hipLaunchKernelGGL(beam_row_kernel<256>, dim3((unsigned)R), dim3(256), 0, s, logits, ldl, scores_in, last, end_id, K, V, cand_val,
                           cand_idx);
    }
}

// the rows a merge wave moves once it has selected (beam_move_rows): the embedding rows of the chosen tokens into x_next and the
// (h, c) rows they extend, by parent.  All zero: the merge only selects; h_src NULL: embedding rows only
struct BeamMove {
    const float* embed;
    int E;
    float* x_next;
    long ldx;
    const float *h_src, *c_src;
    int H;
    float* h_dst;
    long ldh;
    float* c_dst;
};

// the merge launch of one step: the grouped kernel for groups of Kg < K slots, the plain one otherwise
void beam_merge_launch(hipStream_t s, int B, const float* cand_val, const int* cand_idx, int K, int V, int Kg, float lambda,
                       const int64_t* last, long end_id, int32_t* parent, int64_t* token, float* scores_out, const BeamMove& m) {
    if (Kg < K)
        hipLaunchKernelGGL(beam_merge_groups_kernel, dim3(B), dim3(256), 0, s, cand_val, cand_idx, K, V, Kg, lambda, last, end_id, parent,
                           token, scores_out, m.embed, m.E, m.x_next, m.ldx, m.h_src, m.c_src, m.H, m.h_dst, m.ldh, m.c_dst);
    else
        hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(256), 0, s, cand_val, cand_idx, K, V, parent, token, scores_out, m.embed, m.E,
                           m.x_next, m.ldx, m.h_src, m.c_src, m.H, m.h_dst, m.ldh, m.c_dst);
}

// the checks of the grouped entry points, before anything is enqueued (G == 1: lambda is not read)
int beam_groups_check(int K, int G, float lambda) {
    if (G < 1 || K <= 0 || K % G != 0) return SAT_ERR_ARG;
    if (G > 1 && (!(lambda >= 0.0f) || lambda == INFINITY)) return SAT_ERR_ARG;
    return SAT_OK;
}

}  // namespace

extern "C" int sat_kept_tokens(const int64_t* ids, int64_t stride, int B, int T, int64_t end_id, int32_t* kept,
                               sat_stream_t stream) {
    if (!ids || !kept || B <= 0 || T <= 0 || stride < T) return SAT_ERR_ARG;
    hipLaunchKernelGGL(kept_tokens_kernel, dim3(sat_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, ids, (long)stride, B, T,
                       end_id, kept);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int64_t sat_beam_step_ws_bytes(int B, int K) { return (int64_t)B * K * K * 8; }

extern "C" int64_t sat_beam_step_ex_ws_bytes(int B, int K, int V, int T) {
    if (B <= 0 || K <= 0 || V <= 0 || T <= 0) return 0;
    return sat_beam_step_ws_bytes(B, K);                       // the prefix is walked from the records: no state in the workspace
}

extern "C" int64_t sat_beam_step_groups_ws_bytes(int B, int K, int V, int T) { return sat_beam_step_ex_ws_bytes(B, K, V, T); }

// ONE step for sat_beam_step, sat_beam_step_ex and sat_beam_step_groups: the row launch (the constrained kernel where step i of a
// decode under c bans something) and the merge launch (the grouped kernel for G > 1), which here only selects
static int beam_step_impl(const float* logits, int64_t ldl, const float* scores_in, const int64_t* last_tokens, int64_t end_id, int B,
                          int K, int V, const sat_beam_constraints* c, const int32_t* parents, const int64_t* tokens, int i, int T, int G,
                          float lambda, int32_t* parent, int64_t* token, float* scores_out, void* workspace, int64_t ws_bytes,
                          sat_stream_t stream) {
    if (!logits || !scores_in || !parent || !token || !scores_out || !workspace) return SAT_ERR_ARG;
    if (B <= 0 || K <= 0 || V <= 0 || ldl < V || T <= 0 || i < 0 || i >= T) return SAT_ERR_ARG;
    SAT_TRY(beam_groups_check(K, G, lambda));
    if (G > 1 && end_id >= 0 && i > 0 && !last_tokens) return SAT_ERR_ARG;      // which rows are finished decides what is penalised and counted
    bool active = false;
    SAT_TRY(beam_constraints_check(c, end_id, &active));
    if (active && i > 0 && (!parents || !tokens)) return SAT_ERR_ARG;
    if (K > KMAX || (long)K * V > INT_MAX - 1) return SAT_ERR_UNSUPPORTED;
    if (active && (T > kBanTMax || V > kBanVMax)) return SAT_ERR_UNSUPPORTED;
    if (ws_bytes < sat_beam_step_ws_bytes(B, K)) return SAT_ERR_WORKSPACE;
    float* cand_val = (float*)workspace;                       // [B*K rows][K]: deep enough for every group (the lemma at the kernel)
    int* cand_idx = (int*)(cand_val + (long)B * K * K);
    hipStream_t s = (hipStream_t)stream;
    beam_row_launch(s, logits, (long)ldl, scores_in, last_tokens, (long)end_id, B * K, K, V, cand_val, cand_idx, active ? c : nullptr,
                    parents, tokens, i);
    SAT_LAUNCH_CHECK();
    beam_merge_launch(s, B, cand_val, cand_idx, K, V, K / G, lambda, last_tokens, (long)end_id, parent, token, scores_out, BeamMove{});
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

// (no constraints, no step index: one step of a decode of one step)
extern "C" int sat_beam_step(const float* logits, int64_t ldl, const float* scores_in, const int64_t* last_tokens,
                             int64_t end_id, int B, int K, int V, int32_t* parent, int64_t* token, float* scores_out,
                             void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    return beam_step_impl(logits, ldl, scores_in, last_tokens, end_id, B, K, V, nullptr, nullptr, nullptr, 0, 1, 1, 0.0f, parent, token,
                          scores_out, workspace, ws_bytes, stream);
}

extern "C" int sat_beam_step_ex(const float* logits, int64_t ldl, const float* scores_in, const int64_t* last_tokens,
                                int64_t end_id, int B, int K, int V, const sat_beam_constraints* c, const int32_t* parents,
                                const int64_t* tokens, int i, int T, int32_t* parent, int64_t* token, float* scores_out,
                                void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    return beam_step_impl(logits, ldl, scores_in, last_tokens, end_id, B, K, V, c, parents, tokens, i, T, 1, 0.0f, parent, token,
                          scores_out, workspace, ws_bytes, stream);
}

// (num_groups == 1: the launches of sat_beam_step_ex)
extern "C" int sat_beam_step_groups(const float* logits, int64_t ldl, const float* scores_in, const int64_t* last_tokens,
                                    int64_t end_id, int B, int K, int V, const sat_beam_constraints* c, const int32_t* parents,
                                    const int64_t* tokens, int i, int T, int num_groups, float diversity_penalty, int32_t* parent,
                                    int64_t* token, float* scores_out, void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    return beam_step_impl(logits, ldl, scores_in, last_tokens, end_id, B, K, V, c, parents, tokens, i, T, num_groups, diversity_penalty,
                          parent, token, scores_out, workspace, ws_bytes, stream);
}


extern "C" int sat_beam_rerank(const int64_t* ids, const float* scores, int B, int K, int T, int64_t end_id, float length_penalty,
                               int64_t* ids_out, float* scores_out, float* norm_out, int32_t* order_out, sat_stream_t stream) {
    if (!ids || !scores || !ids_out || !scores_out || ids == ids_out || scores == scores_out) return SAT_ERR_ARG;
    if (B <= 0 || K <= 0 || T <= 0) return SAT_ERR_ARG;
    if (!(length_penalty >= 0.0f) || length_penalty == INFINITY) return SAT_ERR_ARG;
    if (K > KMAX) return SAT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(beam_rerank_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, ids, scores, K, T, end_id, length_penalty, ids_out,
                       scores_out, norm_out, order_out);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_beam_gather_rows(const float* src, const int32_t* parent, int B, int K, int width, float* dst,
                                    sat_stream_t stream) {
    if (!src || !parent || !dst || src == dst) return SAT_ERR_ARG;
    if (B <= 0 || K <= 0 || width <= 0) return SAT_ERR_ARG;
    const long total = (long)B * K * width;
    int grid = sat_cdiv(total, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(beam_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, parent, K, width, total, dst);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_beam_backtrack(const int32_t* parents, const int64_t* tokens, int T, int B, int K, int64_t* ids,
                                  sat_stream_t stream) {
    if (!parents || !tokens || !ids) return SAT_ERR_ARG;
    if (T <= 0 || B <= 0 || K <= 0) return SAT_ERR_ARG;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3(sat_cdiv((long)B * K, 256)), dim3(256), 0, (hipStream_t)stream, parents,
                       tokens, T, B * K, K, ids);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_beam_backtrack_rows(const int32_t* parents, const float* rows, int T, int B, int K, int cols, float* out,
                                       sat_stream_t stream) {
    if (!parents || !rows || !out || rows == out) return SAT_ERR_ARG;
    if (T <= 0 || B <= 0 || K <= 0 || cols <= 0) return SAT_ERR_ARG;
    hipLaunchKernelGGL(beam_backtrack_rows_kernel, dim3(B * K), dim3(64), 0, (hipStream_t)stream, parents, rows, T, B * K, K, cols, out);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

// ---- greedy decode (models.py:56-67 `DecoderRNN.sample`) as ONE call: steps x (LSTM step per layer, vocab projection + arg-max,
//      embedding row of the chosen id), enqueued from C.  h / c: [num_layers][B][H] initial state IN, final state OUT (updated in
//      place; h_tmp: scratch of the same size).  ids [B][ids_stride] i64, column i = step i. ----
extern "C" int sat_greedy_decode(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                                 const float* lin_w, const float* lin_b, int B, int E, int H, int V, int steps, float* h, float* c,
                                 float* h_tmp, float* x_tmp /*[B][E]*/, int64_t* ids, int64_t ids_stride, float* workspace,
                                 int64_t ws_bytes, sat_stream_t stream) {
    SAT_TRY(sat_decode_check(features, embed, lstm_w, num_layers, lin_w, lin_b, B, E, H, V, steps, h, c, h_tmp, x_tmp, ids, ids_stride));
    if (!workspace) return SAT_ERR_ARG;
    if (ws_bytes < sat_vocab_argmax_ws_bytes(B, V)) return SAT_ERR_WORKSPACE;
    SatDecodeStack stack(lstm_w, num_layers, B, E, H, h, c, h_tmp, stream);
    const float* x = features;
    for (int i = 0; i < steps; ++i) {
        const float* top;
        SAT_TRY(stack.step(x, &top));
        SAT_TRY(sat_vocab_argmax(top, lin_w, lin_b, B, H, V, ids + i, ids_stride, workspace, ws_bytes, stream));
        SAT_TRY(sat_embed_rows(embed, ids + i, ids_stride, B, E, V, x_tmp, stream));
        x = x_tmp;
    }
    return stack.finish();
}

// ---- ENSEMBLE decode (include/sat_hip.h, sat_ensemble_logprobs): M models' logits rows -> ONE row of combined log-probabilities,
//      which the selection kernels above take as they take a model's logits.  One workgroup of 256 threads per row, two passes over
//      the M rows (the second finds them in L2 / MALL: a row of 10 000 columns is 40 KB per model):
//        pass 1  per model an ONLINE (max, sum) per thread -- one rescale per 16-byte chunk, not per element -- reduced over the wave
//                by __shfl_xor and over the four waves through 2 * M * 4 floats of LDS: lse_m = max + log(sum);
//        pass 2  out[v] from the M values of column v (mode 0: max_m a_m + log sum_m exp(a_m - max), a_m = x_m[v] - lse_m + log w_m;
//                mode 1: sum_m w_m (x_m[v] - lse_m) in model order).
//      exp as ONE fma and ONE v_exp_f32 (beam_row_body's form); the pointers and weights reach the kernel by value.  M is a template
//      argument so that every per-model array is indexed by unrolled constants and lives in registers. ----
namespace {

constexpr int kEnsMax = 8;
struct EnsArgs {
    const float* x[kEnsMax];
    float w[kEnsMax], logw[kEnsMax];
};
constexpr float kLog2e = 1.44269504088896340736f;

// exp(x - m) for x <= m; m == -inf (nothing seen yet) counts as 0, so that exp(-inf - m) is 0 and never NaN
__device__ __forceinline__ float ens_exp(float x, float m) {
    const float mm = m == -INFINITY ? 0.0f : m;
    return __builtin_amdgcn_exp2f(__builtin_fmaf(x, kLog2e, -mm * kLog2e));
}
// (m, s) <- (m, s) + (om, os): the sums rescaled to the larger maximum
__device__ __forceinline__ void ens_join(float& m, float& s, float om, float os) {
    const float nm = fmaxf(m, om);
    s = s * ens_exp(m, nm) + os * ens_exp(om, nm);
    m = nm;
}
template <bool VEC>
__device__ __forceinline__ f32x4 ens_load4(const float* p) {
    if constexpr (VEC) return *(const f32x4*)p;
    else return (f32x4){p[0], p[1], p[2], p[3]};
}

template <int M, bool VEC>
__global__ __launch_bounds__(256) void ensemble_logprobs_kernel(EnsArgs a, long ldl, int mode, int V, float* __restrict__ out, long ldo) {
    __shared__ float s_m[4][M], s_s[4][M];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = V >> 2, tail = (nq << 2) + tid;           // whole 4-column chunks; V % 4 leftover columns, one per thread
    const float* x[M];
#pragma unroll
    for (int j = 0; j < M; ++j) x[j] = a.x[j] + (long)row * ldl;
    float m[M], s[M];
#pragma unroll
    for (int j = 0; j < M; ++j) { m[j] = -INFINITY; s[j] = 0.0f; }
    for (int q = tid; q < nq; q += 256) {
        f32x4 v[M];
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = ens_load4<VEC>(x[j] + 4 * q);      // M loads in flight
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const float cm = fmaxf(fmaxf(v[j][0], v[j][1]), fmaxf(v[j][2], v[j][3]));
            if (cm > m[j]) { s[j] *= ens_exp(m[j], cm); m[j] = cm; }
            s[j] += (ens_exp(v[j][0], m[j]) + ens_exp(v[j][1], m[j])) + (ens_exp(v[j][2], m[j]) + ens_exp(v[j][3], m[j]));
        }
    }
    if (tail < V) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const float xv = x[j][tail];
            if (xv > m[j]) { s[j] *= ens_exp(m[j], xv); m[j] = xv; }
            s[j] += ens_exp(xv, m[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ens_join(m[j], s[j], __shfl_xor(m[j], o, 64), __shfl_xor(s[j], o, 64));
        if (lane == 0) { s_m[wave][j] = m[j]; s_s[wave][j] = s[j]; }
    }
    __syncthreads();
    float lse[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        float bm = s_m[0][j], bs = s_s[0][j];
#pragma unroll
        for (int w = 1; w < 4; ++w) ens_join(bm, bs, s_m[w][j], s_s[w][j]);      // wave order: fixed
        lse[j] = bm + logf(bs);
    }
    auto combine = [&](const float (&xv)[M]) -> float {
        if (mode == 0) {
            float av[M], mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < M; ++j) { av[j] = (xv[j] - lse[j]) + a.logw[j]; mx = fmaxf(mx, av[j]); }
            if (mx == -INFINITY) return -INFINITY;           // every model has -inf here
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < M; ++j) sum += __builtin_amdgcn_exp2f((av[j] - mx) * kLog2e);
            return mx + logf(sum);
        }
        float acc = 0.0f;
        bool dead = false;
#pragma unroll
        for (int j = 0; j < M; ++j) { dead |= xv[j] == -INFINITY; acc += a.w[j] * (xv[j] - lse[j]); }
        return dead ? -INFINITY : acc;                       // (a weight that rounds to 0: no 0 * inf)
    };
    float* o = out + (long)row * ldo;
    for (int q = tid; q < nq; q += 256) {
        f32x4 v[M];
#pragma unroll
        for (int j = 0; j < M; ++j) v[j] = ens_load4<VEC>(x[j] + 4 * q);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float xv[M];
#pragma unroll
            for (int j = 0; j < M; ++j) xv[j] = v[j][e];
            r[e] = combine(xv);
        }
        if constexpr (VEC) *(f32x4*)(o + 4 * q) = r;
        else { o[4 * q] = r[0]; o[4 * q + 1] = r[1]; o[4 * q + 2] = r[2]; o[4 * q + 3] = r[3]; }
    }
    if (tail < V) {
        float xv[M];
#pragma unroll
        for (int j = 0; j < M; ++j) xv[j] = x[j][tail];
        o[tail] = combine(xv);
    }
}

template <int M>
void ensemble_launch_m(hipStream_t s, const EnsArgs& a, long ldl, int mode, int R, int V, float* out, long ldo, bool vec) {
    if (vec) hipLaunchKernelGGL((ensemble_logprobs_kernel<M, true>), dim3((unsigned)R), dim3(256), 0, s, a, ldl, mode, V, out, ldo);
    else hipLaunchKernelGGL((ensemble_logprobs_kernel<M, false>), dim3((unsigned)R), dim3(256), 0, s, a, ldl, mode, V, out, ldo);
}

// the checks of both ensemble entry points on (M, weights, mode), and the weights as the kernel takes them: normalised in double,
// rounded once to f32 (w) and their logarithm likewise (logw); weights NULL: uniform
int ensemble_weights(int M, const float* weights, int mode, EnsArgs* a) {
    if (M < 1 || M > kEnsMax || (mode != 0 && mode != 1)) return SAT_ERR_ARG;
    double sum = 0.0;
    for (int j = 0; j < M; ++j) {
        const float w = weights ? weights[j] : 1.0f;
        if (!(w > 0.0f) || w == INFINITY) return SAT_ERR_ARG;
        sum += (double)w;
    }
    for (int j = 0; j < kEnsMax; ++j) {
        const double wn = j < M ? (double)(weights ? weights[j] : 1.0f) / sum : 0.0;
        a->w[j] = (float)wn;
        a->logw[j] = j < M ? (float)log(wn) : 0.0f;
        a->x[j] = nullptr;
    }
    return SAT_OK;
}

// the launch; the 16-byte path where every row of every matrix is 16-byte aligned, the scalar path otherwise (same values up to
// nothing: both paths do the same arithmetic in the same order)
void ensemble_launch(hipStream_t s, const EnsArgs& a, int M, long ldl, int mode, int R, int V, float* out, long ldo) {
    bool vec = !(ldl & 3) && !(ldo & 3) && !(((uintptr_t)out) & 15);
    for (int j = 0; j < M; ++j) vec = vec && !(((uintptr_t)a.x[j]) & 15);
    switch (M) {
        case 1: ensemble_launch_m<1>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        case 2: ensemble_launch_m<2>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        case 3: ensemble_launch_m<3>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        case 4: ensemble_launch_m<4>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        case 5: ensemble_launch_m<5>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        case 6: ensemble_launch_m<6>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        case 7: ensemble_launch_m<7>(s, a, ldl, mode, R, V, out, ldo, vec); break;
        default: ensemble_launch_m<8>(s, a, ldl, mode, R, V, out, ldo, vec); break;
    }
}

}  // namespace

extern "C" int sat_ensemble_logprobs(const float* const* logits, int M, int64_t ldl, const float* weights, int mode, int R, int V,
                                     float* out, int64_t ldo, sat_stream_t stream) {
    if (!logits || !out || R <= 0 || V <= 0 || ldl < V || ldo < V) return SAT_ERR_ARG;
    EnsArgs a;
    SAT_TRY(ensemble_weights(M, weights, mode, &a));
    for (int j = 0; j < M; ++j) {
        if (!logits[j] || logits[j] == out) return SAT_ERR_ARG;
        a.x[j] = logits[j];
    }
    ensemble_launch((hipStream_t)stream, a, M, (long)ldl, mode, R, V, out, (long)ldo);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

static int ensemble_models_check(const sat_decoder_model* models, int M) {
    if (!models || M < 1 || M > kEnsMax) return SAT_ERR_ARG;
    bool unsupported = false;                                  // (an argument error anywhere comes in front of it)
    for (int j = 0; j < M; ++j) {
        const sat_decoder_model& d = models[j];
        if (!d.features || !d.embed || !d.lstm_w || !d.lin_w || !d.lin_b || d.E <= 0 || d.H <= 0 || d.num_layers < 1) return SAT_ERR_ARG;
        unsupported = unsupported || d.num_layers > 8 || (d.E & 3) || (d.H & 3);      // (sat_lstm_step's 16-byte rows)
        for (int i = 0; i < 4 * (d.num_layers > 8 ? 8 : d.num_layers); ++i)
            if (!d.lstm_w[i]) return SAT_ERR_ARG;
    }
    return unsupported ? SAT_ERR_UNSUPPORTED : SAT_OK;
}

// what beam_merge_kernel's second half does for the model whose rows it moves, for ANY model of an ensemble: one workgroup per image
// reads the step's (parent, token) records and moves the embedding rows of the chosen tokens and the (h, c) rows they extend
__global__ __launch_bounds__(256) void ensemble_move_rows_kernel(const int* __restrict__ parent, const int64_t* __restrict__ token, int K,
                                                                 const float* __restrict__ embed, int E, float* __restrict__ x_next, long ldx,
                                                                 const float* __restrict__ h_src, const float* __restrict__ c_src, int H,
                                                                 float* __restrict__ h_dst, long ldh, float* __restrict__ c_dst) {
    __shared__ int s_par[KMAX], s_tok[KMAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < K) {
        s_par[threadIdx.x] = parent[b * K + threadIdx.x];
        s_tok[threadIdx.x] = (int)token[b * K + threadIdx.x];
    }
    beam_move_rows(s_par, s_tok, b, K, lane, wave, embed, E, x_next, ldx, h_src, c_src, H, h_dst, ldh, c_dst);
}

// ---- the whole beam decode of one batch as ONE call (eval.py:99's `model.sample` loop, models.py:56-67, widened to a beam; the
//      reference's own sample_beam is a stub, model2.py:113-114): the host enqueues every step from C with no Python in between.
//      Two parts carry it.  BeamMember is ONE decoder's state in a beam of R = B*K rows: its plan (which kernels its shape takes),
//      its slice of the workspace, its setup, its step into its own logits matrix, and the two ways its rows follow a selection.
//      BeamSearch is everything that is not per model: scores, candidates, the (parent, token) records, the row and merge launches,
//      the backtrack and the rerank.  beam_decode_impl (sat_beam_decode, _ex, _groups) drives one member, with the member's row
//      moves fused into the merge launch: 5 launches per step at one wide layer.  sat_beam_decode_ensemble drives M members in lock
//      step, with the combine launch between their steps and the selection.  Same kernels, same arithmetic as the step-by-step
//      entry points: bit-identical ids and scores. ----
constexpr int kBeamKSplitMax = 8;      // K-split slices of the wide step's gate GEMM (a wide member's workspace holds that many [R][4H] slabs)

static int beam_grid(long total) { return total > 2048L * 256 ? 2048 : sat_cdiv(total, 256); }

struct BeamMember {
    sat_decoder_model d = {};
    int B = 0, K = 0, V = 0, ksplit = 1;
    int64_t R = 0, ldl = 0;
    bool wide = false, x3 = false;
    float *hc = nullptr, *logits = nullptr;                    // [layer][h0, h1, c0, c1][R][H]; [R][ldl]
    float *x0 = nullptr, *xe = nullptr;                        // narrow: the step-0 input rows and the embedding rows, [R][E]
    float *xh[2] = {}, *wcat = nullptr, *gates = nullptr;      // wide: two [R][E + H] input rows, W_cat [4H][E + H], the gate slabs
    void* lin_split = nullptr;                                 // x3: [V128][H] x 3 bf16, fragment ordered (sat_gemm_f32x3_pack)
    int cur_h[8] = {}, cur_c[8] = {}, xi = 0;                  // which of the two buffers holds a layer's live h / c, the live [x | h]

    BeamMember() = default;
    explicit BeamMember(const sat_decoder_model& d_) : d(d_) {}

    // Which kernels the member's shape takes, decided here and nowhere else.
    // WIDE step: with one LSTM layer and >= 128 rows the gates are ONE LDS-tiled exact-f32 MFMA GEMM over the concatenated row
    // [x | h] (sat_gemm_f32: ~0.5 of the f32 peak) + a pointwise launch, instead of the few-rows kernel, which re-reads the weights
    // once per 64-row chunk (34 -> ~17 us per step at 320 rows; 1.7 -> ~1.0 ms per member of an ensemble, profiles/ensemble_bench.txt).
    // That GEMM is small (160 tiles of 64 x 64 at 320 rows): its K axis is dealt over enough slices to fill the chip's ~512
    // workgroup slots, the pointwise launch sums the slices in order (measured at 320 rows, 20 steps: 1 slice 1.82 ms, 2 1.76,
    // 3 1.685, 4 1.73, 6 1.75, 8 1.85 -- profiles/r05_decode_loop.txt).
    // X3 projection: on the wide path with V % 4 == 0 the vocab projection -- half of a step on the exact-f32 pipe -- runs on the
    // bf16 pipe from a three-way split of both operands (sat_gemm_x3.hip: f32 accuracy, not the f32 pipe's bit pattern).
    // honour_env (the single-model entry points): SAT_BEAM_KSPLIT in 1..8 overrides the slices, SAT_BEAM_X3=0 keeps the exact-f32
    // pipe.  An ensemble's kernels are a function of the shapes alone.
    void plan(int B_, int K_, int V_, bool honour_env) {
        static const int ks_env = [] { const char* e = getenv("SAT_BEAM_KSPLIT"); return e ? atoi(e) : 0; }();
        static const bool x3_env = [] { const char* v = getenv("SAT_BEAM_X3"); return !(v && v[0] == '0'); }();
        B = B_, K = K_, V = V_;
        R = (int64_t)B * K, ldl = (V + 3) / 4 * 4;
        wide = d.num_layers == 1 && R >= 128 && !(d.H & 3);
        x3 = wide && (x3_env || !honour_env) && sat_gemm_f32x3_packed_bytes(V, d.H) > 0 && !(V & 3);
        ksplit = 1;
        if (!wide) return;
        const long tiles = (long)sat_cdiv((int)R, 64) * sat_cdiv(4 * d.H, 64);
        ksplit = (int)(512 / (tiles > 0 ? tiles : 1));
        const int nk = sat_cdiv(d.E + d.H, 32);                // K-steps of the f32 kernel
        if (ksplit > nk / 4) ksplit = nk / 4;
        if (ksplit > kBeamKSplitMax) ksplit = kBeamKSplitMax;
        if (ksplit < 1) ksplit = 1;
        if (honour_env && ks_env >= 1 && ks_env <= kBeamKSplitMax) ksplit = ks_env;
    }

    // the member's slice of the workspace, as carve() takes it
    int64_t bytes() const {
        const int64_t ldx = d.E + d.H;
        const int64_t n = al256(4 * (int64_t)d.num_layers * R * d.H * 4) + al256(R * ldl * 4);
        if (!wide) return n + 2 * al256(R * d.E * 4);
        return n + 2 * al256(R * ldx * 4) + al256(4 * (int64_t)d.H * ldx * 4) + al256(kBeamKSplitMax * R * 4 * (int64_t)d.H * 4) +
               (x3 ? al256(sat_gemm_f32x3_packed_bytes(V, d.H)) : 0);
    }
    void carve(char*& w) {
        const int64_t ldx = d.E + d.H;
        hc = (float*)w; w += al256(4 * (int64_t)d.num_layers * R * d.H * 4);
        logits = (float*)w; w += al256(R * ldl * 4);
        if (!wide) {
            x0 = (float*)w; w += al256(R * d.E * 4);
            xe = (float*)w; w += al256(R * d.E * 4);
            return;
        }
        xh[0] = (float*)w; w += al256(R * ldx * 4);
        xh[1] = (float*)w; w += al256(R * ldx * 4);
        wcat = (float*)w; w += al256(4 * (int64_t)d.H * ldx * 4);
        gates = (float*)w; w += al256(kBeamKSplitMax * R * 4 * (int64_t)d.H * 4);
        if (x3) { lin_split = w; w += al256(sat_gemm_f32x3_packed_bytes(V, d.H)); }
    }

    float* h_buf(int l, int which) const { return hc + ((long)l * 4 + which) * R * d.H; }
    float* c_buf(int l, int which) const { return hc + ((long)l * 4 + 2 + which) * R * d.H; }

    // before step 0: h = c = 0, the weights in the forms the plan needs, the features as every row's first input, and the start
    // scores sc0 (every member of an ensemble writes the same ones)
    int setup(sat_stream_t stream, int Kg, float* sc0) {
        hipStream_t s = (hipStream_t)stream;
        const long ldx = d.E + d.H;
        hipError_t e = hipMemsetAsync(hc, 0, (size_t)(4 * (int64_t)d.num_layers * R * d.H * 4), s);
        if (e != hipSuccess) return (int)e;
        if (x3) SAT_TRY(sat_gemm_f32x3_pack(d.lin_w, V, d.H, lin_split, stream));      // (the weights are split once per call)
        if (wide) {
            e = hipMemsetAsync(xh[0], 0, (size_t)(R * ldx * 4), s);                     // h_{-1} = 0
            if (e != hipSuccess) return (int)e;
            const long total = 4L * d.H * ldx;
            hipLaunchKernelGGL(beam_wcat_kernel, dim3(beam_grid(total)), dim3(256), 0, s, d.lstm_w[0], d.lstm_w[1], d.E, d.H, total, wcat);
            SAT_LAUNCH_CHECK();
        }
        if (ldl > V) {                                         // pad columns of the logits rows: read by nobody, but keep them defined
            e = hipMemsetAsync(logits, 0, (size_t)(R * ldl * 4), s);
            if (e != hipSuccess) return (int)e;
        }
        const long total = R * d.E;                            // (the scores, one per thread, are covered by the same grid)
        int grid = beam_grid(total);
        if ((long)grid * 256 < R) grid = sat_cdiv(R, 256);
        hipLaunchKernelGGL(beam_init_kernel, dim3(grid), dim3(256), 0, s, d.features, K, d.E, total, wide ? xh[0] : x0,
                           wide ? ldx : (long)d.E, sc0, (int)R, Kg);
        SAT_LAUNCH_CHECK();
        return SAT_OK;
    }

    // step i: the LSTM stack on the live input rows, then the vocab projection of the top h into `logits`
    int forward(sat_stream_t stream, int i) {
        const int H = d.H;
        const float* inp = i == 0 ? x0 : xe;
        if (wide) {
            const long ldx = d.E + H, total = R * H;
            float* h_new = h_buf(0, 0);                        // (a wide h never ping-pongs: the row move puts it into the next [x | h])
            SAT_TRY(sat_gemm_f32_splitk(0, 0, xh[xi], ldx, wcat, ldx, gates, 4L * H, d.lstm_w[2], d.lstm_w[3], (int)R, 4 * H, (int)ldx,
                                        ksplit, R * 4L * H, stream));
            hipLaunchKernelGGL(beam_lstm_point_kernel, dim3(beam_grid(total)), dim3(256), 0, (hipStream_t)stream, gates,
                               c_buf(0, cur_c[0]), h_new, H, total, ksplit, R * 4L * H);
            SAT_LAUNCH_CHECK();
            inp = h_new;
        }
        for (int l = 0; l < d.num_layers && !wide; ++l) {
            float* h_out = h_buf(l, 1 - cur_h[l]);
            SAT_TRY(sat_lstm_step(inp, h_buf(l, cur_h[l]), c_buf(l, cur_c[l]), d.lstm_w[4 * l], d.lstm_w[4 * l + 1], d.lstm_w[4 * l + 2],
                                  d.lstm_w[4 * l + 3], (int)R, l == 0 ? d.E : H, H, h_out, stream));
            cur_h[l] = 1 - cur_h[l];
            inp = h_out;
        }
        if (x3) return sat_gemm_f32x3(inp, H, lin_split, d.lin_b, logits, ldl, (int)R, V, H, stream);
        return sat_vocab_logits_fwd(inp, d.lin_w, d.lin_b, (int)R, H, V, logits, ldl, stream);
    }

    // The rows follow a selection in one of two ways.
    // FUSED (one model): the merge wave itself moves them -- wide: the embedding rows and (h, c) by parent, h straight into the next
    // input row's h half (one launch fewer per step); narrow: the embedding rows only, then gather() per layer.
    BeamMove fused_move() const {
        if (!wide) return BeamMove{d.embed, d.E, xe, (long)d.E, nullptr, nullptr, 0, nullptr, 0L, nullptr};
        const long ldx = d.E + d.H;
        float* xn = xh[1 - xi];
        return BeamMove{d.embed, d.E, xn, ldx, h_buf(0, 0), c_buf(0, cur_c[0]), d.H, xn + d.E, ldx, c_buf(0, 1 - cur_c[0])};
    }
    void after_fused_merge() {
        if (!wide) return;
        cur_c[0] = 1 - cur_c[0];
        xi = 1 - xi;
    }
    // a narrow member's (h, c) of every layer re-ordered by parent: one launch per layer (K == 1: every row is its own parent)
    int gather(sat_stream_t stream, const int32_t* par) {
        const long total = R * d.H;
        for (int l = 0; l < d.num_layers && !wide && K > 1; ++l) {
            hipLaunchKernelGGL(beam_gather2_kernel, dim3(beam_grid(2 * total)), dim3(256), 0, (hipStream_t)stream,
                               (const float*)h_buf(l, cur_h[l]), (const float*)c_buf(l, cur_c[l]), par, K, d.H, total,
                               h_buf(l, 1 - cur_h[l]), (long)d.H, c_buf(l, 1 - cur_c[l]));
            SAT_LAUNCH_CHECK();
            cur_h[l] = 1 - cur_h[l];
            cur_c[l] = 1 - cur_c[l];
        }
        return SAT_OK;
    }
    // ON ITS OWN (any member of an ensemble), from the step's records -- wide: ONE launch that does what the fused merge does;
    // narrow: the embedding rows, then gather()
    int move_rows(sat_stream_t stream, const int32_t* par, const int64_t* tok) {
        if (!wide) {
            SAT_TRY(sat_embed_rows(d.embed, tok, 1, (int)R, d.E, V, xe, stream));
            return gather(stream, par);
        }
        const BeamMove m = fused_move();
        hipLaunchKernelGGL(ensemble_move_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const int*)par, tok, K, m.embed, m.E,
                           m.x_next, m.ldx, m.h_src, m.c_src, m.H, m.h_dst, m.ldh, m.c_dst);
        SAT_LAUNCH_CHECK();
        after_fused_merge();
        return SAT_OK;
    }
};

struct BeamSearch {
    int B = 0, K = 0, V = 0, steps = 0, Kg = 0, si = 0;
    int64_t R = 0, end_id = -1;
    float lambda = 0.0f, length_penalty = 0.0f;
    bool ex = false, rerank = false;
    const sat_beam_constraints* c = nullptr;                   // NULL unless a step constraint is on
    float *sc[2] = {}, *cand_val = nullptr;                    // the scores before / after a selection (sc[si]: live), [R][K] candidates
    int* cand_idx = nullptr;
    int32_t* parents = nullptr;                                // records [steps][R]
    int64_t* tokens = nullptr;
    int64_t* ids_search = nullptr;                             // ex: the ids in search order (the rerank writes the caller's), and its
    float *sc_ranked = nullptr, *norm_tmp = nullptr;           //   outputs where the caller passes NULL
    int32_t* order_tmp = nullptr;
    int* hist = nullptr;                                       // ex: the two planes of the per-slot prefix history (beam_row_launch)
    int32_t* par = nullptr;                                    // the step's records, and the tokens of the step before (NULL: no row is
    int64_t* tok = nullptr;                                    //   finished)
    const int64_t* last = nullptr;

    // the checks every whole decode makes before anything is enqueued, in the order of their return codes; sizes_ok / models_ok:
    // what the driver found for its own sizes (SAT_ERR_ARG) and its models' shapes (SAT_ERR_UNSUPPORTED).  ex: with the rerank's
    // buffers and the history planes (every entry point but sat_beam_decode)
    int init(int B_, int K_, int V_, int steps_, int64_t end_id_, const sat_beam_constraints* c_, int G, float lambda_, bool ex_,
             bool sizes_ok, bool models_ok) {
        SAT_TRY(beam_groups_check(K_, G, lambda_));
        if (!sizes_ok) return SAT_ERR_ARG;
        bool active = false;
        SAT_TRY(beam_constraints_check(c_, end_id_, &active));
        if (!models_ok || (long)K_ * V_ > INT_MAX - 1) return SAT_ERR_UNSUPPORTED;
        if (active && (steps_ > kBanTMax || V_ > kBanVMax)) return SAT_ERR_UNSUPPORTED;
        B = B_, K = K_, V = V_, steps = steps_, Kg = K_ / G, end_id = end_id_, lambda = lambda_, ex = ex_;
        R = (int64_t)B * K;
        rerank = (c_ && c_->length_penalty > 0.0f) || G > 1;   // (groups: the results leave in (norm desc, slot asc) order)
        length_penalty = c_ ? c_->length_penalty : 0.0f;
        c = active ? c_ : nullptr;
        return SAT_OK;
    }

    static int64_t bytes(int B, int K, int steps, bool ex) {
        const int64_t R = (int64_t)B * K;
        const int64_t n = 2 * al256(R * 4) + al256(sat_beam_step_ws_bytes(B, K)) + al256((int64_t)steps * R * 4) + al256((int64_t)steps * R * 8);
        return ex ? n + al256(R * steps * 8) + 3 * al256(R * 4) + al256(2 * R * kBanTMax * 4) : n;
    }
    void carve(char*& w) {
        sc[0] = (float*)w; w += al256(R * 4);
        sc[1] = (float*)w; w += al256(R * 4);
        cand_val = (float*)w; w += al256(sat_beam_step_ws_bytes(B, K));
        cand_idx = (int*)(cand_val + (long)B * K * K);
        parents = (int32_t*)w; w += al256((int64_t)steps * R * 4);
        tokens = (int64_t*)w; w += al256((int64_t)steps * R * 8);
        if (!ex) return;
        ids_search = (int64_t*)w; w += al256(R * steps * 8);
        sc_ranked = (float*)w; w += al256(R * 4);
        norm_tmp = (float*)w; w += al256(R * 4);
        order_tmp = (int32_t*)w; w += al256(R * 4);
        static const bool hist_env = [] { const char* v = getenv("SAT_BEAM_HISTORY"); return !(v && v[0] == '0'); }();
        if (c && c->no_repeat_ngram >= 1 && hist_env) hist = (int*)w;      // only n-gram blocking reads the whole prefix
        w += al256(2 * R * kBanTMax * 4);
    }

    // step i on a matrix of logits (or of combined log-probabilities): every row's K best continuations ...
    int select(sat_stream_t stream, const float* logits, long ldl, int i) {
        par = parents + (long)i * R;
        tok = tokens + (long)i * R;
        last = (i > 0 && end_id >= 0) ? tok - R : (const int64_t*)nullptr;
        beam_row_launch((hipStream_t)stream, logits, ldl, sc[si], last, (long)end_id, (int)R, K, V, cand_val, cand_idx, c, parents, tokens, i,
                        hist);
        SAT_LAUNCH_CHECK();
        return SAT_OK;
    }
    // ... and every image's K best of those into the step's records; the merge wave then moves the rows of `move`
    int merge(sat_stream_t stream, const BeamMove& move) {
        beam_merge_launch((hipStream_t)stream, B, cand_val, cand_idx, K, V, Kg, lambda, last, (long)end_id, par, tok, sc[1 - si], move);
        SAT_LAUNCH_CHECK();
        si = 1 - si;
        return SAT_OK;
    }

    // behind the last step: the sequences by walking the records back, then the K hypotheses of an image re-ordered by
    // score / L^alpha -- or, with no rerank, the norm is the score and the order the identity
    int finish(sat_stream_t stream, int64_t* ids, float* scores_out, float* norm_scores, int32_t* order) {
        hipStream_t s = (hipStream_t)stream;
        hipLaunchKernelGGL(beam_backtrack_kernel, dim3(sat_cdiv(R, 256)), dim3(256), 0, s, parents, tokens, steps, (int)R, K,
                           rerank ? ids_search : ids);
        SAT_LAUNCH_CHECK();
        if (rerank) {
            hipLaunchKernelGGL(beam_rerank_kernel, dim3(B), dim3(64), 0, s, (const int64_t*)ids_search, (const float*)sc[si], K, steps,
                               end_id, length_penalty, ids, scores_out ? scores_out : sc_ranked, norm_scores ? norm_scores : norm_tmp,
                               order ? order : order_tmp);
            SAT_LAUNCH_CHECK();
            return SAT_OK;
        }
        for (float* out : {scores_out, norm_scores}) {
            if (!out) continue;
            hipError_t e = hipMemcpyAsync(out, sc[si], (size_t)(R * 4), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return (int)e;
        }
        if (order) {
            hipLaunchKernelGGL(beam_iota_kernel, dim3(sat_cdiv(R, 256)), dim3(256), 0, s, order, (int)R, K);
            SAT_LAUNCH_CHECK();
        }
        return SAT_OK;
    }
};

// the workspace of a single-model decode: the search's buffers and the member's, as its plan sizes them
static int64_t beam_decode_bytes(int B, int K, int E, int H, int V, int num_layers, int steps, bool ex) {
    if (B <= 0 || K <= 0 || K > KMAX || E <= 0 || H <= 0 || V <= 0 || num_layers < 1 || steps < 1) return 0;
    BeamMember m(sat_decoder_model{nullptr, nullptr, nullptr, num_layers, nullptr, nullptr, E, H});
    m.plan(B, K, V, true);
    return BeamSearch::bytes(B, K, steps, ex) + m.bytes();
}

extern "C" int64_t sat_beam_decode_ws_bytes(int B, int K, int E, int H, int V, int num_layers, int steps) {
    return beam_decode_bytes(B, K, E, H, V, num_layers, steps, false);
}
extern "C" int64_t sat_beam_decode_ex_ws_bytes(int B, int K, int E, int H, int V, int num_layers, int steps) {
    return beam_decode_bytes(B, K, E, H, V, num_layers, steps, true);
}
extern "C" int64_t sat_beam_decode_groups_ws_bytes(int B, int K, int E, int H, int V, int num_layers, int steps) {
    return beam_decode_bytes(B, K, E, H, V, num_layers, steps, true);
}

// ONE driver for sat_beam_decode (ex false, c NULL), sat_beam_decode_ex and sat_beam_decode_groups: with constraints the row launch of
// a step that bans something is the constrained kernel; with G > 1 groups the first slot of every group starts live and the merge
// launch of every step is the grouped one; with a length penalty or with groups the rerank runs behind the backtrack
static int beam_decode_impl(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                            const float* lin_w, const float* lin_b, int B, int K, int E, int H, int V, int steps,
                            int64_t end_id, bool ex, const sat_beam_constraints* c, int G, float lambda, int64_t* ids, float* scores_out,
                            float* norm_scores, int32_t* order, void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!features || !embed || !lstm_w || !lin_w || !lin_b || !ids || !workspace) return SAT_ERR_ARG;
    const int64_t need = beam_decode_bytes(B, K, E, H, V, num_layers, steps, ex);
    BeamSearch search;
    SAT_TRY(search.init(B, K, V, steps, end_id, c, G, lambda, ex, need > 0, !(E & 3)));
    if (ws_bytes < need || (((uintptr_t)workspace) & 255)) return SAT_ERR_WORKSPACE;
    for (int i = 0; i < 4 * num_layers; ++i)
        if (!lstm_w[i]) return SAT_ERR_ARG;
    if (num_layers > 8) return SAT_ERR_UNSUPPORTED;
    BeamMember m(sat_decoder_model{features, embed, lstm_w, num_layers, lin_w, lin_b, E, H});
    m.plan(B, K, V, true);
    char* w = (char*)workspace;
    search.carve(w);
    m.carve(w);
    SAT_TRY(m.setup(stream, search.Kg, search.sc[0]));
    for (int i = 0; i < steps; ++i) {
        SAT_TRY(m.forward(stream, i));
        SAT_TRY(search.select(stream, m.logits, (long)m.ldl, i));
        SAT_TRY(search.merge(stream, m.fused_move()));
        m.after_fused_merge();
        if (i + 1 < steps) SAT_TRY(m.gather(stream, search.par));      // (nothing reads the state behind the last selection)
    }
    return search.finish(stream, ids, scores_out, norm_scores, order);
}

extern "C" int sat_beam_decode(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                               const float* lin_w, const float* lin_b, int B, int K, int E, int H, int V, int steps,
                               int64_t end_id, int64_t* ids, float* scores_out, void* workspace, int64_t ws_bytes,
                               sat_stream_t stream) {
    return beam_decode_impl(features, embed, lstm_w, num_layers, lin_w, lin_b, B, K, E, H, V, steps, end_id, false, nullptr, 1, 0.0f, ids,
                            scores_out, nullptr, nullptr, workspace, ws_bytes, stream);
}

extern "C" int sat_beam_decode_ex(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                                  const float* lin_w, const float* lin_b, int B, int K, int E, int H, int V, int steps,
                                  int64_t end_id, const sat_beam_constraints* c, int64_t* ids, float* scores_out, float* norm_scores,
                                  int32_t* order, void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    return beam_decode_impl(features, embed, lstm_w, num_layers, lin_w, lin_b, B, K, E, H, V, steps, end_id, true, c, 1, 0.0f, ids,
                            scores_out, norm_scores, order, workspace, ws_bytes, stream);
}

extern "C" int sat_beam_decode_groups(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                                      const float* lin_w, const float* lin_b, int B, int K, int E, int H, int V, int steps,
                                      int64_t end_id, const sat_beam_constraints* c, int num_groups, float diversity_penalty,
                                      int64_t* ids, float* scores_out, float* norm_scores, int32_t* order, void* workspace,
                                      int64_t ws_bytes, sat_stream_t stream) {
    return beam_decode_impl(features, embed, lstm_w, num_layers, lin_w, lin_b, B, K, E, H, V, steps, end_id, true, c, num_groups,
                            diversity_penalty, ids, scores_out, norm_scores, order, workspace, ws_bytes, stream);
}

// ---- the beam decode of an ENSEMBLE of DecoderRNN models as ONE call: M members in lock step.  Per step: every member's forward
//      into its own [R][pad4(V)] matrix; ONE combine launch; the search's row and merge launches on the combined matrix; then every
//      member moves its own rows by the step's records. ----
static int64_t ensemble_bytes(const sat_decoder_model* models, int M, int B, int K, int V, int steps) {
    int64_t n = al256((int64_t)B * K * ((V + 3) / 4 * 4) * 4) + BeamSearch::bytes(B, K, steps, true);      // the combined matrix, the search
    for (int j = 0; j < M; ++j) {
        BeamMember m(models[j]);
        m.plan(B, K, V, false);
        n += m.bytes();
    }
    return n;
}

extern "C" int64_t sat_beam_decode_ensemble_ws_bytes(const sat_decoder_model* models, int M, int B, int K, int V, int steps) {
    if (ensemble_models_check(models, M) != SAT_OK) return 0;
    if (B <= 0 || K <= 0 || K > KMAX || V <= 0 || steps < 1) return 0;
    return ensemble_bytes(models, M, B, K, V, steps);
}

extern "C" int sat_beam_decode_ensemble(const sat_decoder_model* models, int M, const float* weights, int mode, int B, int K, int V,
                                        int steps, int64_t end_id, const sat_beam_constraints* c, int num_groups, float diversity_penalty,
                                        int64_t* ids, float* scores_out, float* norm_scores, int32_t* order, void* workspace,
                                        int64_t ws_bytes, sat_stream_t stream) {
    if (!models || !ids || !workspace) return SAT_ERR_ARG;
    EnsArgs ens;
    SAT_TRY(ensemble_weights(M, weights, mode, &ens));
    const int models_rc = ensemble_models_check(models, M);
    if (models_rc == SAT_ERR_ARG) return models_rc;
    BeamSearch search;
    SAT_TRY(search.init(B, K, V, steps, end_id, c, num_groups, diversity_penalty, true, B > 0 && K <= KMAX && V > 0 && steps >= 1,
                        models_rc == SAT_OK));
    if (ws_bytes < ensemble_bytes(models, M, B, K, V, steps) || (((uintptr_t)workspace) & 255)) return SAT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t R = search.R, ldl = (V + 3) / 4 * 4;
    char* w = (char*)workspace;
    float* comb = (float*)w; w += al256(R * ldl * 4);
    search.carve(w);
    if (ldl > V) {                                             // pad columns: read by nobody, but keep them defined
        hipError_t e = hipMemsetAsync(comb, 0, (size_t)(R * ldl * 4), s);
        if (e != hipSuccess) return (int)e;
    }
    BeamMember members[kEnsMax];
    for (int j = 0; j < M; ++j) {
        BeamMember& m = members[j] = BeamMember(models[j]);
        m.plan(B, K, V, false);
        m.carve(w);
        SAT_TRY(m.setup(stream, search.Kg, search.sc[0]));
        ens.x[j] = m.logits;
    }
    for (int i = 0; i < steps; ++i) {
        for (int j = 0; j < M; ++j) SAT_TRY(members[j].forward(stream, i));
        ensemble_launch(s, ens, M, (long)ldl, mode, (int)R, V, comb, (long)ldl);
        SAT_LAUNCH_CHECK();
        SAT_TRY(search.select(stream, comb, (long)ldl, i));
        SAT_TRY(search.merge(stream, BeamMove{}));
        if (i + 1 == steps) break;                             // nothing reads the state behind the last selection
        for (int j = 0; j < M; ++j) SAT_TRY(members[j].move_rows(stream, search.par, search.tok));
    }
    return search.finish(stream, ids, scores_out, norm_scores, order);
}

