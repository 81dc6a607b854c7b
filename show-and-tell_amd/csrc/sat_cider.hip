// CIDEr on the device (pycocoevalcap/cider/cider_scorer.py:93-181; train.py:169-177 keeps model-best.pth by it): the score of a
// batch of decoded id rows against the reference captions of their images, in f64, without a host synchronisation.
//
// The corpus is a trie of its n-grams (orders 1..4): node 0 is the root, node id(w1..wk) the child of id(w1..wk-1) under wk, so an
// n-gram is found by <= 4 chained probes of an open-addressing table keyed (parent << 32) | token with an EXACT compare -- there
// is no fingerprint and no false match.  The host builds the node list (keys, df) once; sat_cider_table_insert puts the keys into
// the table with a 64-bit compare-and-swap per slot and a plain store of the node id beside it.  Nothing reads the table inside
// that launch, every probe sequence is linear and bounded by the capacity, and a full table or a duplicate key only sets a status
// bit: no lane ever waits for another lane's store.
//
// caption_stats is the one code path of `counts2vec` (cider_scorer.py:107-131) for references and hypotheses alike: the node of
// every (order, position) through the table, the term frequency of every DISTINCT n-gram by direct token comparison inside the
// caption (so an n-gram the corpus does not have is still counted exactly: df = 0, weight tf * log(images)), and the norms.  The
// sums run over the distinct n-grams in order of first occurrence, which is the order the reference's dicts are walked in, one
// lane per order; log(images) and log(df) come from the same device `log`, so an n-gram every image has weighs exactly 0 as it
// does in the reference.
//
// cider_score_kernel: one wave per hypothesis row.  Per reference of the row's image and per distinct hypothesis n-gram the
// reference's term frequency is counted by comparing tokens against the reference's positions; min(vh, vr) * vr is summed per
// order in the same fixed order, divided by the norms where both are non-zero, weighted by the Gaussian of the length difference
// (`length` is the reference's: the sum of tf over BIGRAMS, max(len - 1, 0)) and added up over the references in corpus order.
// The mean is a second launch of one wave that sums in a fixed order: two runs give the same bits.
#include "sat_internal.h"

namespace {
constexpr int kOrders = 4;
constexpr int kMaxHyp = 64;                  // hypothesis tokens per row
constexpr int kMaxRef = 128;                 // tokens per reference caption
constexpr int kAbsent = -1;                  // node of an n-gram the corpus does not have
constexpr uint64_t kEmpty = ~0ull;           // no key is all ones: a parent id is below 2^31
constexpr int kStatusFull = 1, kStatusDuplicate = 2;

// slot of a key: bits 32.. of the Fibonacci product, masked (cider.table_slot is the host's copy for the tests)
__device__ __forceinline__ uint32_t cider_slot(uint64_t key, uint32_t mask) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

__global__ __launch_bounds__(256) void cider_insert_kernel(const uint64_t* __restrict__ keys, int n_keys, unsigned long long* table_keys,
                                                           int32_t* table_nodes, uint32_t mask, int32_t* status) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_keys) return;
    const uint64_t key = keys[j];
    if (key == kEmpty) {
        atomicOr(status, kStatusDuplicate);
        return;
    }
    uint32_t slot = cider_slot(key, mask);
    for (uint32_t p = 0; p <= mask; ++p) {
        const uint64_t old = atomicCAS(table_keys + slot, (unsigned long long)kEmpty, (unsigned long long)key);
        if (old == kEmpty) {
            table_nodes[slot] = j + 1;           // node ids are 1-based: 0 is the root
            return;
        }
        if (old == key) {
            atomicOr(status, kStatusDuplicate);
            return;
        }
        slot = (slot + 1) & mask;
    }
    atomicOr(status, kStatusFull);
}

struct cider_table {
    const uint64_t* keys;
    const int32_t* nodes;
    const int32_t* df;
    uint32_t mask;
    int32_t n_nodes;
};

__device__ __forceinline__ int cider_lookup(const cider_table& t, int parent, int token) {
    const uint64_t key = ((uint64_t)(uint32_t)parent << 32) | (uint32_t)token;
    uint32_t slot = cider_slot(key, t.mask);
    for (uint32_t p = 0; p <= t.mask; ++p) {
        const uint64_t k = t.keys[slot];
        if (k == key) {
            const int node = t.nodes[slot];
            return node >= 1 && node <= t.n_nodes ? node : kAbsent;
        }
        if (k == kEmpty) return kAbsent;
        slot = (slot + 1) & t.mask;
    }
    return kAbsent;
}

// does the n-gram of `order` + 1 tokens at a[i] equal the one at b[j]?
__device__ __forceinline__ bool same_ngram(const int* a, int i, const int* b, int j, int order) {
    bool eq = true;
    for (int q = 0; q <= order; ++q) eq = eq && a[i + q] == b[j + q];
    return eq;
}

// LDS of one caption of up to MAXL tokens
template <int MAXL> struct caption_lds {
    int tok[MAXL];
    int node[kOrders][MAXL];        // trie node of the n-gram that starts at a position, kAbsent where the corpus has none
    int tf[kOrders][MAXL];          // term frequency at the FIRST occurrence of an n-gram, 0 at its repeats and past the end
    double idf[kOrders][MAXL];      // log(images) - log(max(1, df)) at the same places
    double term[kOrders][MAXL];     // scratch of the fixed-order sums
    double norm[kOrders];
};

// counts2vec for the caption in c.tok[0..L): one wave, every lane of it.  Ends with the LDS results visible to the wave.
template <int MAXL> __device__ void caption_stats(caption_lds<MAXL>& c, int L, const cider_table& t, double log_images) {
    const int lane = threadIdx.x;
    for (int i = lane; i < MAXL; i += 64) {
        int parent = 0;
        for (int k = 0; k < kOrders; ++k) {
            int node = kAbsent;
            if (i + k < L && parent != kAbsent && c.tok[i + k] >= 0) node = cider_lookup(t, parent, c.tok[i + k]);
            c.node[k][i] = node;
            parent = node;
        }
    }
    __syncthreads();
    for (int item = lane; item < kOrders * MAXL; item += 64) {
        const int k = item / MAXL, i = item - k * MAXL;
        int tf = 0;
        double idf = 0.0, term = 0.0;
        if (i + k < L) {
            bool first = true;
            for (int j = 0; j < i && first; ++j) first = !same_ngram(c.tok, i, c.tok, j, k);
            if (first) {
                tf = 1;
                for (int j = i + 1; j + k < L; ++j) tf += same_ngram(c.tok, i, c.tok, j, k) ? 1 : 0;
                const int node = c.node[k][i];
                const int df = node != kAbsent ? t.df[node - 1] : 0;
                idf = log_images - log((double)max(1, df));
                const double v = (double)tf * idf;
                term = v * v;
            }
        }
        c.tf[k][i] = tf;
        c.idf[k][i] = idf;
        c.term[k][i] = term;
    }
    __syncthreads();
    if (lane < kOrders) {
        double s = 0.0;
        for (int i = 0; i + lane < L; ++i) s += c.term[lane][i];
        c.norm[lane] = sqrt(s);
    }
    __syncthreads();
}

struct cider_corpus_dev {
    cider_table table;
    const int32_t* ref_tokens;
    const int32_t* ref_offsets;
    const int32_t* image_offsets;
    const double* ref_norm;
    int32_t n_refs, n_images;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void cider_ref_stats_kernel(cider_corpus_dev c, int64_t n_tokens, double* __restrict__ ref_norm) {
    __shared__ caption_lds<kMaxRef> cap;
    const int r = blockIdx.x, lane = threadIdx.x;
    const int64_t lo = min((int64_t)max(c.ref_offsets[r], 0), n_tokens);
    const int64_t hi = min(max((int64_t)c.ref_offsets[r + 1], lo), n_tokens);
    const int L = (int)min((int64_t)kMaxRef, hi - lo);
    for (int i = lane; i < kMaxRef; i += 64) cap.tok[i] = i < L ? c.ref_tokens[lo + i] : -1;
    __syncthreads();
    caption_stats(cap, L, c.table, log((double)c.n_images));
    if (lane < kOrders) ref_norm[(int64_t)r * kOrders + lane] = cap.norm[lane];
}

__global__ __launch_bounds__(64) void cider_score_kernel(cider_corpus_dev c, int64_t n_tokens, const int64_t* __restrict__ ids,
                                                         int64_t stride, int T, const int32_t* __restrict__ kept, int64_t end_id,
                                                         const int32_t* __restrict__ image_index, double inv_two_sigma2,
                                                         double* __restrict__ scores) {
    __shared__ caption_lds<kMaxHyp> hyp;
    __shared__ int rtok[kMaxRef];
    __shared__ int hyp_len;
    __shared__ double total[kOrders];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* row = ids + (int64_t)b * stride;

    // the row: ids outside [0, 2^31) are no corpus token (-1 never equals a reference token and is never looked up)
    int64_t my = lane < T ? row[lane] : 0;
    hyp.tok[lane] = lane < T && my >= 0 && my <= 0x7fffffffll ? (int)my : -1;
    if (kept) {
        if (lane == 0) hyp_len = clampi(kept[b], 0, T);
    } else {
        const unsigned long long ends = __ballot(lane < T && my == end_id);
        if (lane == 0) hyp_len = ends ? __ffsll(ends) - 1 : T;
    }
    if (lane < kOrders) total[lane] = 0.0;
    __syncthreads();
    const int L = hyp_len;
    caption_stats(hyp, L, c.table, log((double)c.n_images));

    const int img = clampi(image_index[b], 0, c.n_images - 1);
    const int r0 = clampi(c.image_offsets[img], 0, c.n_refs), r1 = clampi(c.image_offsets[img + 1], r0, c.n_refs);
    const int len_h = max(L - 1, 0);
    for (int r = r0; r < r1; ++r) {
        const int64_t lo = min((int64_t)max(c.ref_offsets[r], 0), n_tokens);
        const int64_t hi = min(max((int64_t)c.ref_offsets[r + 1], lo), n_tokens);
        const int Lr = (int)min((int64_t)kMaxRef, hi - lo);
        for (int i = lane; i < kMaxRef; i += 64) rtok[i] = i < Lr ? c.ref_tokens[lo + i] : -2;
        __syncthreads();
        for (int item = lane; item < kOrders * kMaxHyp; item += 64) {
            const int k = item / kMaxHyp, i = item - k * kMaxHyp;
            double term = 0.0;
            const int tf = hyp.tf[k][i];
            if (tf > 0 && hyp.node[k][i] != kAbsent) {      // an n-gram the corpus lacks is in no reference
                int tfr = 0;
                for (int j = 0; j + k < Lr; ++j) tfr += same_ngram(hyp.tok, i, rtok, j, k) ? 1 : 0;
                const double vh = (double)tf * hyp.idf[k][i], vr = (double)tfr * hyp.idf[k][i];
                term = fmin(vh, vr) * vr;
            }
            hyp.term[k][i] = term;
        }
        __syncthreads();
        if (lane < kOrders) {
            double val = 0.0;
            for (int i = 0; i + lane < L; ++i) val += hyp.term[lane][i];
            const double nh = hyp.norm[lane], nr = c.ref_norm[(int64_t)r * kOrders + lane];
            if (nh != 0.0 && nr != 0.0) val /= nh * nr;
            const double delta = (double)(len_h - max(Lr - 1, 0));
            val *= exp(-(delta * delta) * inv_two_sigma2);
            total[lane] += val;
        }
        __syncthreads();
    }
    if (lane == 0) {
        double s = ((total[0] + total[1]) + total[2]) + total[3];
        s /= (double)kOrders;
        if (r1 > r0) s /= (double)(r1 - r0);
        scores[b] = s * 10.0;
    }
}

__global__ __launch_bounds__(64) void cider_mean_kernel(const double* __restrict__ scores, int B, double* __restrict__ mean) {
    __shared__ double part[64];
    double s = 0.0;
    for (int i = threadIdx.x; i < B; i += 64) s += scores[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += part[i];
        mean[0] = t / (double)B;
    }
}

bool power_of_two(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// SAT_OK, or why this corpus cannot be used (host-only: no pointer is dereferenced on the device side)
int corpus_check(const sat_cider_corpus* c, bool need_norm) {
    if (!c) return SAT_ERR_ARG;
    if (!c->table_keys || !c->table_nodes || !c->df || !c->ref_tokens || !c->ref_offsets || !c->image_offsets) return SAT_ERR_ARG;
    if (need_norm && !c->ref_norm) return SAT_ERR_ARG;
    if (c->n_nodes <= 0 || c->n_refs <= 0 || c->n_images <= 0 || c->n_tokens <= 0 || c->max_ref_tokens <= 0) return SAT_ERR_ARG;
    if (!power_of_two(c->capacity) || c->capacity < 2 * (int64_t)c->n_nodes) return SAT_ERR_ARG;
    if (c->capacity > (1ll << 32)) return SAT_ERR_UNSUPPORTED;
    if (c->max_ref_tokens > kMaxRef) return SAT_ERR_UNSUPPORTED;
    return SAT_OK;
}

cider_corpus_dev corpus_dev(const sat_cider_corpus* c) {
    cider_corpus_dev d;
    d.table.keys = c->table_keys;
    d.table.nodes = c->table_nodes;
    d.table.df = c->df;
    d.table.mask = (uint32_t)(c->capacity - 1);
    d.table.n_nodes = c->n_nodes;
    d.ref_tokens = c->ref_tokens;
    d.ref_offsets = c->ref_offsets;
    d.image_offsets = c->image_offsets;
    d.ref_norm = c->ref_norm;
    d.n_refs = c->n_refs;
    d.n_images = c->n_images;
    return d;
}
}  // namespace

extern "C" int sat_cider_table_insert(const uint64_t* keys, int n_keys, uint64_t* table_keys, int32_t* table_nodes, int64_t capacity,
                                      int32_t* status, sat_stream_t stream) {
    if (!keys || !table_keys || !table_nodes || !status || n_keys <= 0) return SAT_ERR_ARG;
    if (!power_of_two(capacity) || capacity < 2 * (int64_t)n_keys) return SAT_ERR_ARG;
    if (capacity > (1ll << 32)) return SAT_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(table_keys, 0xff, (size_t)capacity * sizeof(uint64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(table_nodes, 0, (size_t)capacity * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cider_insert_kernel, dim3(sat_cdiv(n_keys, 256)), dim3(256), 0, s, keys, n_keys, (unsigned long long*)table_keys,
                       table_nodes, (uint32_t)(capacity - 1), status);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_cider_ref_stats(const sat_cider_corpus* corpus, double* ref_norm, sat_stream_t stream) {
    SAT_TRY(corpus_check(corpus, false));
    if (!ref_norm) return SAT_ERR_ARG;
    hipLaunchKernelGGL(cider_ref_stats_kernel, dim3(corpus->n_refs), dim3(64), 0, (hipStream_t)stream, corpus_dev(corpus),
                       corpus->n_tokens, ref_norm);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_cider_score(const sat_cider_corpus* corpus, const int64_t* ids, int64_t stride, int B, int T, const int32_t* kept,
                               int64_t end_id, const int32_t* image_index, double sigma, double* scores, double* mean,
                               sat_stream_t stream) {
    SAT_TRY(corpus_check(corpus, true));
    if (!ids || !image_index || !scores || !mean || B <= 0 || T <= 0 || stride < T) return SAT_ERR_ARG;
    if (!(sigma > 0.0) || sigma - sigma != 0.0) return SAT_ERR_ARG;
    if (T > kMaxHyp) return SAT_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cider_score_kernel, dim3(B), dim3(64), 0, s, corpus_dev(corpus), corpus->n_tokens, ids, stride, T, kept, end_id,
                       image_index, 1.0 / (2.0 * sigma * sigma), scores);
    SAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cider_mean_kernel, dim3(1), dim3(64), 0, s, scores, B, mean);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

// Consensus reranking (sat_consensus_rerank in include/sat_hip.h): the candidates of one image scored against each other.  The
// "references" of a row are the other rows of the decode output, so nothing of the corpus but the table and df is read, and an
// n-gram the corpus lacks is matched like any other: by its tokens.
namespace {
constexpr int kMaxCand = 64;                 // candidates per image

// candidate `row` of the grid into c.tok (hypothesis form: -1 for an id that is no token) and its length; then its statistics
__device__ __forceinline__ int consensus_load_row(caption_lds<kMaxHyp>& c, int* len_lds, const int64_t* __restrict__ row, int slot, int T,
                                                  const int32_t* __restrict__ kept, int64_t end_id, const cider_table& t,
                                                  double log_images) {
    const int lane = threadIdx.x;
    const int64_t my = lane < T ? row[lane] : 0;
    c.tok[lane] = lane < T && my >= 0 && my <= 0x7fffffffll ? (int)my : -1;
    if (kept) {
        if (lane == 0) *len_lds = clampi(kept[slot], 0, T);
    } else {
        const unsigned long long ends = __ballot(lane < T && my == end_id);
        if (lane == 0) *len_lds = ends ? __ffsll(ends) - 1 : T;
    }
    __syncthreads();
    const int L = *len_lds;
    caption_stats(c, L, t, log_images);
    return L;
}

// one wave per (image, candidate): norm[slot][4] and len[slot]
__global__ __launch_bounds__(64) void consensus_stats_kernel(cider_table t, int n_images, const int64_t* __restrict__ ids,
                                                             int64_t image_stride, int64_t cand_stride, int K, int T,
                                                             const int32_t* __restrict__ kept, int64_t end_id, double* __restrict__ norm,
                                                             int32_t* __restrict__ len) {
    __shared__ caption_lds<kMaxHyp> cap;
    __shared__ int cap_len;
    const int slot = blockIdx.x, b = slot / K, i = slot - b * K, lane = threadIdx.x;
    const int L = consensus_load_row(cap, &cap_len, ids + (int64_t)b * image_stride + (int64_t)i * cand_stride, slot, T, kept, end_id, t,
                                     log((double)n_images));
    if (lane < kOrders) norm[(int64_t)slot * kOrders + lane] = cap.norm[lane];
    if (lane == 0) len[slot] = L;
}

// one wave per (image, candidate i): the other candidates j of the image as single references, in slot order
__global__ __launch_bounds__(64) void consensus_pair_kernel(cider_table t, int n_images, const int64_t* __restrict__ ids,
                                                            int64_t image_stride, int64_t cand_stride, int K, int T,
                                                            const int32_t* __restrict__ kept, int64_t end_id,
                                                            const double* __restrict__ norm, const int32_t* __restrict__ len,
                                                            const double* __restrict__ weights, double inv_two_sigma2,
                                                            double* __restrict__ utility, double* __restrict__ pair) {
    __shared__ caption_lds<kMaxHyp> hyp;
    __shared__ int rtok[kMaxHyp];
    __shared__ int hyp_len;
    __shared__ double total[kOrders], value[kOrders];
    const int slot = blockIdx.x, b = slot / K, i = slot - b * K, lane = threadIdx.x;
    const int64_t* image = ids + (int64_t)b * image_stride;
    if (lane < kOrders) total[lane] = 0.0;
    const int L = consensus_load_row(hyp, &hyp_len, image + (int64_t)i * cand_stride, slot, T, kept, end_id, t, log((double)n_images));
    const int len_h = max(L - 1, 0);
    const double* w = weights ? weights + (int64_t)b * K : nullptr;
    double den = 0.0;
    for (int j = 0; j < K; ++j) {
        if (j == i) {
            if (pair && lane == 0) pair[(int64_t)slot * K + j] = 0.0;
            continue;
        }
        // reference form: -2 for an id that is no token, so it equals no hypothesis token (-1 included)
        const int64_t other = lane < T ? image[(int64_t)j * cand_stride + lane] : -1;
        rtok[lane] = other >= 0 && other <= 0x7fffffffll ? (int)other : -2;
        const int Lr = clampi(len[b * K + j], 0, T);
        const double wj = w ? w[j] : 1.0;
        den += wj;
        __syncthreads();
        for (int item = lane; item < kOrders * kMaxHyp; item += 64) {
            const int k = item / kMaxHyp, p = item - k * kMaxHyp;
            double term = 0.0;
            const int tf = hyp.tf[k][p];
            if (tf > 0) {
                int tfr = 0;
                for (int q = 0; q + k < Lr; ++q) tfr += same_ngram(hyp.tok, p, rtok, q, k) ? 1 : 0;
                const double vh = (double)tf * hyp.idf[k][p], vr = (double)tfr * hyp.idf[k][p];
                term = fmin(vh, vr) * vr;
            }
            hyp.term[k][p] = term;
        }
        __syncthreads();
        if (lane < kOrders) {
            double val = 0.0;
            for (int p = 0; p + lane < L; ++p) val += hyp.term[lane][p];
            const double nh = hyp.norm[lane], nr = norm[(int64_t)(b * K + j) * kOrders + lane];
            if (nh != 0.0 && nr != 0.0) val /= nh * nr;
            const double delta = (double)(len_h - max(Lr - 1, 0));
            val *= exp(-(delta * delta) * inv_two_sigma2);
            value[lane] = val;
            total[lane] += w ? wj * val : val;
        }
        __syncthreads();
        if (pair && lane == 0) pair[(int64_t)slot * K + j] = (((value[0] + value[1]) + value[2]) + value[3]) / (double)kOrders * 10.0;
    }
    if (lane == 0) {
        double s = (((total[0] + total[1]) + total[2]) + total[3]) / (double)kOrders;
        if (w) s = den != 0.0 ? s / den * 10.0 : 0.0;
        else s = K > 1 ? s / (double)(K - 1) * 10.0 : 0.0;
        utility[slot] = s;
    }
}

// one thread per image: the first slot of maximal utility
__global__ __launch_bounds__(64) void consensus_best_kernel(const double* __restrict__ utility, int B, int K, int64_t* __restrict__ best) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* u = utility + (int64_t)b * K;
    int arg = 0;
    double top = u[0];
    for (int i = 1; i < K; ++i) {
        const double v = u[i];
        if (v > top || (top != top && v == v)) {
            top = v;
            arg = i;
        }
    }
    best[b] = arg;
}
}  // namespace

extern "C" int64_t sat_consensus_ws_bytes(int B, int K) {
    if (B <= 0 || K <= 0) return 0;
    const int64_t rows = (int64_t)B * K;
    return rows * kOrders * (int64_t)sizeof(double) + (rows * (int64_t)sizeof(int32_t) + 7) / 8 * 8;
}

extern "C" int sat_consensus_rerank(const sat_cider_corpus* corpus, const int64_t* ids, int64_t image_stride, int64_t cand_stride, int B,
                                    int K, int T, const int32_t* kept, int64_t end_id, double sigma, const double* weights,
                                    double* utility, int64_t* best, double* pair, void* workspace, int64_t ws_bytes,
                                    sat_stream_t stream) {
    SAT_TRY(corpus_check(corpus, false));
    if (!ids || !utility || !best || !workspace || B <= 0 || K <= 0 || T <= 0 || cand_stride < T) return SAT_ERR_ARG;
    if (B > 1 && image_stride < (int64_t)K * cand_stride) return SAT_ERR_ARG;
    if (!(sigma > 0.0) || sigma - sigma != 0.0) return SAT_ERR_ARG;
    if ((uintptr_t)workspace % 8 != 0) return SAT_ERR_ARG;
    if (T > kMaxHyp || K > kMaxCand || (int64_t)B * K > 0x7fffffffll) return SAT_ERR_UNSUPPORTED;
    if (ws_bytes < sat_consensus_ws_bytes(B, K)) return SAT_ERR_WORKSPACE;
    const int rows = B * K;
    double* norm = (double*)workspace;
    int32_t* len = (int32_t*)(norm + (int64_t)rows * kOrders);
    const cider_table t = corpus_dev(corpus).table;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(consensus_stats_kernel, dim3(rows), dim3(64), 0, s, t, corpus->n_images, ids, image_stride, cand_stride, K, T, kept,
                       end_id, norm, len);
    SAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(consensus_pair_kernel, dim3(rows), dim3(64), 0, s, t, corpus->n_images, ids, image_stride, cand_stride, K, T, kept,
                       end_id, norm, len, weights, 1.0 / (2.0 * sigma * sigma), utility, pair);
    SAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(consensus_best_kernel, dim3(sat_cdiv(B, 64)), dim3(64), 0, s, utility, B, K, best);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}
