// BLEU-1..4 and ROUGE-L on the device, beside CIDEr (language_eval, eval.py:17-56; pycocoevalcap/eval.py:39-45): the other two
// plain-arithmetic metrics of `lang_stats` for a batch of decoded id rows against the reference captions of their images, in
// f64, without a host synchronisation.  Neither needs the CIDEr trie: n-grams are compared token by token.
//
// bleu_comps_kernel restates cook_test + compute_score(option='closest') (bleu_scorer.py:60-83, 198-256), one wave per row.  Lane i
// owns the n-grams (orders 1..4) that start at position i of the row: their count inside the row where i is the FIRST occurrence
// (0 at a repeat, so every distinct n-gram is counted once) and, reference by reference, the largest count any reference of the
// image has -- both by direct token comparison, in registers.  correct[k] is the wave's integer sum of min(count, max count);
// the closest reference length minimises (|l - L|, l).  Everything up to here is an integer; lane 0 then does the reference's
// ~40 f64 operations for the per-image `bleu_list` entries.  The batch's components are added into the totals with 64-bit integer
// atomics: the sums are integers, so any order gives the same bits.  bleu_finalize_kernel is the corpus-level `bleus` of the totals.
//
// rouge_l_kernel restates Rouge.calc_score (rouge.py:45-75), one wave per row.  The row is at most 64 tokens, one per lane, so the
// longest common subsequence runs on one 64-bit word (Crochemore et al. 2001; Hyyro 2004): per reference token the match mask M
// is a __ballot over the row's lanes and  U = V & M; V = (V + U) | (V - U);  the LCS is the number of zero bits of V below the
// row's length.  Every lane holds the same V (wave-uniform arithmetic), nothing is exchanged.  The reference splits with
// split(" "), under which an EMPTY caption is ONE token that equals only another empty caption's token: kEmptyTok below.
//
// The reference caption is staged in LDS once per (row, reference); every device-supplied offset and index is clamped; no lane
// waits for another lane's store.  The means are a second launch of one wave that sums in a fixed order: two runs give the same
// bits.
#include <cmath>

#include "sat_internal.h"

namespace {
constexpr int kOrders = 4;
constexpr int kMaxHyp = 64;                  // hypothesis tokens per row: one per lane, one bit of the LCS word each
constexpr int kMaxRef = 128;                 // tokens per reference caption
constexpr int kComps = 10;                   // testlen, reflen, guess[4], correct[4]
constexpr int kNoToken = -1;                 // a row id outside [0, 2^31), and the row's positions past its end
constexpr int kPadTok = -2;                  // a reference's positions past its end (and a negative reference token)
constexpr int kEmptyTok = -3;                // ROUGE-L: the one token of an empty caption

struct ref_corpus_dev {
    const int32_t* ref_tokens;
    const int32_t* ref_offsets;
    const int32_t* image_offsets;
    int64_t n_tokens;
    int32_t n_refs, n_images;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The row of this wave: the lane's token (kNoToken for an id outside [0, 2^31) and past T) and, as the return value, the row's
// length -- kept[b] clamped to [0, T], or the position of the first end_id.  Wave-uniform result, no LDS.
__device__ __forceinline__ int load_row(const int64_t* __restrict__ ids, int64_t stride, int T, const int32_t* __restrict__ kept,
                                        int64_t end_id, int b, int lane, int& tok) {
    const int64_t* row = ids + (int64_t)b * stride;
    const int64_t my = lane < T ? row[lane] : 0;
    tok = lane < T && my >= 0 && my <= 0x7fffffffll ? (int)my : kNoToken;
    if (kept) return clampi(kept[b], 0, T);
    const unsigned long long ends = __ballot(lane < T && my == end_id);
    return ends ? __ffsll(ends) - 1 : T;
}

// reference r into LDS (positions past its end: kPadTok); returns its length, clamped like every offset
__device__ __forceinline__ int load_ref(const ref_corpus_dev& c, int r, int lane, int* rtok) {
    const int64_t lo = min((int64_t)max(c.ref_offsets[r], 0), c.n_tokens);
    const int64_t hi = min(max((int64_t)c.ref_offsets[r + 1], lo), c.n_tokens);
    const int Lr = (int)min((int64_t)kMaxRef, hi - lo);
    for (int i = lane; i < kMaxRef; i += 64) {
        const int t = i < Lr ? c.ref_tokens[lo + i] : kPadTok;
        rtok[i] = t < 0 ? kPadTok : t;
    }
    return Lr;
}

// does the n-gram of `order` + 1 tokens at a[i] equal the one at b[j]?
__device__ __forceinline__ bool same_ngram(const int* a, int i, const int* b, int j, int order) {
    bool eq = true;
    for (int q = 0; q <= order; ++q) eq = eq && a[i + q] == b[j + q];
    return eq;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// bleu_scorer.py:231-239 (per image) and 247-256 (corpus) are the same arithmetic on different integers: the running product of
// (correct + 1e-15) / (guess + 1e-9), its (k+1)-th root, the brevity factor when the length ratio is below 1.
__device__ void bleu_values(int64_t testlen, int64_t reflen, const int64_t* guess, const int64_t* correct, double* out) {
#pragma clang fp contract(off)
    double bleu = 1.0;
    for (int k = 0; k < kOrders; ++k) {
        bleu *= ((double)correct[k] + 1e-15) / ((double)guess[k] + 1e-9);
        out[k] = pow(bleu, 1.0 / (double)(k + 1));
    }
    const double ratio = ((double)testlen + 1e-15) / ((double)reflen + 1e-9);
    if (ratio < 1.0) {
        const double brevity = exp(1.0 - 1.0 / ratio);
        for (int k = 0; k < kOrders; ++k) out[k] *= brevity;
    }
}

__global__ __launch_bounds__(64) void bleu_comps_kernel(ref_corpus_dev c, const int64_t* __restrict__ ids, int64_t stride, int T,
                                                        const int32_t* __restrict__ kept, int64_t end_id,
                                                        const int32_t* __restrict__ image_index, int64_t* __restrict__ comps,
                                                        double* __restrict__ sentence, unsigned long long* totals) {
    __shared__ int htok[kMaxHyp + kOrders];
    __shared__ int rtok[kMaxRef];
    const int b = blockIdx.x, lane = threadIdx.x;
    int tok;
    const int L = load_row(ids, stride, T, kept, end_id, b, lane, tok);
    htok[lane] = lane < L ? tok : kNoToken;
    if (lane < kOrders) htok[kMaxHyp + lane] = kNoToken;
    __syncthreads();

    // the row's own counts.  Two ids outside [0, 2^31) compare equal here (both kNoToken); their n-grams are in no reference, so
    // whether they count as one n-gram or two changes nothing: min(count, 0) = 0 either way
    int hc[kOrders], mx[kOrders];
    for (int k = 0; k < kOrders; ++k) {
        hc[k] = 0;
        mx[k] = 0;
        if (lane + k < L) {
            bool first = true;
            for (int j = 0; j < lane && first; ++j) first = !same_ngram(htok, lane, htok, j, k);
            if (first) {
                hc[k] = 1;
                for (int j = lane + 1; j + k < L; ++j) hc[k] += same_ngram(htok, lane, htok, j, k) ? 1 : 0;
            }
        }
    }

    const int img = clampi(image_index[b], 0, c.n_images - 1);
    const int r0 = clampi(c.image_offsets[img], 0, c.n_refs), r1 = clampi(c.image_offsets[img + 1], r0, c.n_refs);
    int best_d = 0, reflen = 0;
    for (int r = r0; r < r1; ++r) {
        const int Lr = load_ref(c, r, lane, rtok);
        __syncthreads();
        for (int k = 0; k < kOrders; ++k) {
            if (hc[k] > 0) {
                int cnt = 0;
                for (int j = 0; j + k < Lr; ++j) cnt += same_ngram(htok, lane, rtok, j, k) ? 1 : 0;
                mx[k] = max(mx[k], cnt);
            }
        }
        const int d = Lr > L ? Lr - L : L - Lr;
        if (r == r0 || d < best_d || (d == best_d && Lr < reflen)) {
            best_d = d;
            reflen = Lr;
        }
        __syncthreads();                        // rtok is rewritten by the next reference
    }

    int64_t guess[kOrders], correct[kOrders];
    for (int k = 0; k < kOrders; ++k) {
        guess[k] = max(0, L - k);
        correct[k] = wave_sum(min(hc[k], mx[k]));
    }
    if (lane == 0) {
        int64_t* out = comps + (int64_t)b * kComps;
        out[0] = L;
        out[1] = reflen;
        for (int k = 0; k < kOrders; ++k) {
            out[2 + k] = guess[k];
            out[2 + kOrders + k] = correct[k];
        }
        double s[kOrders];
        bleu_values(L, reflen, guess, correct, s);
        for (int k = 0; k < kOrders; ++k) sentence[(int64_t)b * kOrders + k] = s[k];
        if (totals) {
            atomicAdd(totals + 0, (unsigned long long)L);
            atomicAdd(totals + 1, (unsigned long long)reflen);
            for (int k = 0; k < kOrders; ++k) {
                atomicAdd(totals + 2 + k, (unsigned long long)guess[k]);
                atomicAdd(totals + 2 + kOrders + k, (unsigned long long)correct[k]);
            }
        }
    }
}

__global__ __launch_bounds__(64) void bleu_finalize_kernel(const int64_t* __restrict__ totals, double* __restrict__ bleu) {
    if (threadIdx.x != 0) return;
    int64_t guess[kOrders], correct[kOrders];
    for (int k = 0; k < kOrders; ++k) {
        guess[k] = totals[2 + k];
        correct[k] = totals[2 + kOrders + k];
    }
    double s[kOrders];
    bleu_values(totals[0], totals[1], guess, correct, s);
    for (int k = 0; k < kOrders; ++k) bleu[k] = s[k];
}

__global__ __launch_bounds__(64) void rouge_l_kernel(ref_corpus_dev c, const int64_t* __restrict__ ids, int64_t stride, int T,
                                                     const int32_t* __restrict__ kept, int64_t end_id,
                                                     const int32_t* __restrict__ image_index, double beta2,
                                                     double* __restrict__ scores) {
    __shared__ int rtok[kMaxRef];
    const int b = blockIdx.x, lane = threadIdx.x;
    int tok;
    const int L = load_row(ids, stride, T, kept, end_id, b, lane, tok);
    const int Lh = max(L, 1);                   // "".split(" ") == [""]: one token
    const int mine = L == 0 ? (lane == 0 ? kEmptyTok : kNoToken) : (lane < L ? tok : kNoToken);
    const unsigned long long below = Lh >= 64 ? ~0ull : (1ull << Lh) - 1ull;

    const int img = clampi(image_index[b], 0, c.n_images - 1);
    const int r0 = clampi(c.image_offsets[img], 0, c.n_refs), r1 = clampi(c.image_offsets[img + 1], r0, c.n_refs);
    int lcs_max = 0;
    double rec_max = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int Lr = load_ref(c, r, lane, rtok);
        __syncthreads();
        const int Lr1 = max(Lr, 1);
        unsigned long long V = ~0ull;
        for (int j = 0; j < Lr1; ++j) {
            const int rt = Lr == 0 ? kEmptyTok : rtok[j];
            const unsigned long long M = __ballot(lane < Lh && mine == rt);
            const unsigned long long U = V & M;
            V = (V + U) | (V - U);
        }
        const int lcs = __popcll(~V & below);
        lcs_max = max(lcs_max, lcs);
        rec_max = fmax(rec_max, (double)lcs / (double)Lr1);
        __syncthreads();                        // rtok is rewritten by the next reference
    }
    if (lane == 0) {
#pragma clang fp contract(off)
        const double prec_max = (double)lcs_max / (double)Lh;       // the row's length is the same for every reference
        double score = 0.0;
        if (prec_max != 0.0 && rec_max != 0.0) score = ((1.0 + beta2) * prec_max * rec_max) / (rec_max + beta2 * prec_max);
        scores[b] = score;
    }
}

// mean[k] = sum over the B rows of x[b][k] (fixed order) / B, for k < cols <= 4
__global__ __launch_bounds__(64) void column_mean_kernel(const double* __restrict__ x, int B, int cols, double* __restrict__ mean) {
    __shared__ double part[kOrders][64];
    for (int k = 0; k < cols; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < B; i += 64) s += x[(int64_t)i * cols + k];
        part[k][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < cols) {
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += part[threadIdx.x][i];
        mean[threadIdx.x] = t / (double)B;
    }
}

// SAT_OK, or why this corpus cannot be used (host-only: no pointer is dereferenced)
int corpus_check(const sat_ref_corpus* c) {
    if (!c) return SAT_ERR_ARG;
    if (!c->ref_tokens || !c->ref_offsets || !c->image_offsets) return SAT_ERR_ARG;
    if (c->n_refs <= 0 || c->n_images <= 0 || c->n_tokens <= 0 || c->max_ref_tokens <= 0) return SAT_ERR_ARG;
    if (c->max_ref_tokens > kMaxRef) return SAT_ERR_UNSUPPORTED;
    return SAT_OK;
}

int rows_check(const int64_t* ids, int64_t stride, int B, int T, const int32_t* image_index) {
    if (!ids || !image_index || B <= 0 || T <= 0 || stride < T) return SAT_ERR_ARG;
    if (T > kMaxHyp) return SAT_ERR_UNSUPPORTED;
    return SAT_OK;
}

ref_corpus_dev corpus_dev(const sat_ref_corpus* c) {
    ref_corpus_dev d;
    d.ref_tokens = c->ref_tokens;
    d.ref_offsets = c->ref_offsets;
    d.image_offsets = c->image_offsets;
    d.n_tokens = c->n_tokens;
    d.n_refs = c->n_refs;
    d.n_images = c->n_images;
    return d;
}
}  // namespace

extern "C" int sat_bleu_comps(const sat_ref_corpus* corpus, const int64_t* ids, int64_t stride, int B, int T, const int32_t* kept,
                              int64_t end_id, const int32_t* image_index, int64_t* comps, double* sentence, double* mean,
                              int64_t* totals, sat_stream_t stream) {
    SAT_TRY(corpus_check(corpus));
    if (!comps || !sentence) return SAT_ERR_ARG;
    SAT_TRY(rows_check(ids, stride, B, T, image_index));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bleu_comps_kernel, dim3(B), dim3(64), 0, s, corpus_dev(corpus), ids, stride, T, kept, end_id, image_index, comps,
                       sentence, (unsigned long long*)totals);
    SAT_LAUNCH_CHECK();
    if (mean) {
        hipLaunchKernelGGL(column_mean_kernel, dim3(1), dim3(64), 0, s, sentence, B, kOrders, mean);
        SAT_LAUNCH_CHECK();
    }
    return SAT_OK;
}

extern "C" int sat_bleu_finalize(const int64_t* totals, double* bleu, sat_stream_t stream) {
    if (!totals || !bleu) return SAT_ERR_ARG;
    hipLaunchKernelGGL(bleu_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, totals, bleu);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_rouge_l_score(const sat_ref_corpus* corpus, const int64_t* ids, int64_t stride, int B, int T, const int32_t* kept,
                                 int64_t end_id, const int32_t* image_index, double beta, double* scores, double* mean,
                                 sat_stream_t stream) {
    SAT_TRY(corpus_check(corpus));
    if (!scores || !mean) return SAT_ERR_ARG;
    if (!(beta > 0.0) || beta - beta != 0.0) return SAT_ERR_ARG;
    SAT_TRY(rows_check(ids, stride, B, T, image_index));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rouge_l_kernel, dim3(B), dim3(64), 0, s, corpus_dev(corpus), ids, stride, T, kept, end_id, image_index,
                       beta * beta, scores);
    SAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(column_mean_kernel, dim3(1), dim3(64), 0, s, scores, B, 1, mean);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}
