// Stochastic decode: one token per row of logits, drawn after temperature, top-k and nucleus (top-p) filtering -- the decode mode
// next to the arg-max (`sample`) and the beam (`sample_beam`).  One workgroup of 256 threads per row, one launch per step:
//   1. the row is read ONCE into registers (16-byte loads; rows that do not fit or are not 16-byte aligned take a looped path with
//      the same arithmetic) and every logit gets an order-preserving 32-bit key (float order, -0.0 == +0.0, NaN = no candidate);
//   2. the top-k cut is a radix select on the keys: four passes of 8 bits over a 256-bin LDS histogram of counts, then -- only
//      when a tie group straddles the cut -- two more passes over the tied columns' indexes (lowest index first);
//   3. the nucleus cut is the same select over a histogram of INTEGER masses: w_v = exp((x_v - x_max) / tau) in f64, kept as
//      floor(w_v * 2^48) in a uint64, so that every sum is exact whatever the order the LDS atomics arrive in;
//   4. the draw is the Gumbel-max of sat_vocab_sample's convention over the kept columns only: Philox runs for kept columns
//      alone (top_k = 5: two or three evaluations per row instead of V / 4).
// Total order of a row's candidates: value descending, equal values by ascending column.  Both cuts keep a PREFIX of it, which a
// pair (threshold key T, index limit I) describes: kept(v) = key_v > T || (key_v == T && v <= I).
//
// Fixed-point loss: every mass loses < 2^-48 to the floor, a prefix sum of at most V masses < V * 2^-48 -- 4.4e-11 at V = 12 289
// and 1.2e-10 at the limit V = 32 768 (SAT_SAMPLE_MAX_V: V masses of at most 2^48 stay below 2^63), against Z >= 1 and a rounding
// band of 1e-6 * Z; f64 exp adds 1 ulp (1e-16) per mass, p * Z is rounded once to f64 (1e-16 * Z).
//
// No sort, no host read, no float accumulation whose order could vary: ids, kept and logp are functions of (row contents,
// temperature, top_k, top_p, seed, rank, r, t) alone.
#include "sat_decode_state.h"
#include <limits.h>
#include <math.h>

namespace {

typedef unsigned long long u64;

constexpr int NT = 256, NW = NT / 64;
constexpr int RC = 12;                       // 16-byte chunks of a row a thread keeps in registers (V >> 2 <= 3072: V <= 12 291)
constexpr int kMaxV = 32768;                 // V masses of <= 2^48 each sum below 2^63; column indexes fit two 8-bit passes
constexpr double kMassScale = 0x1p48;
constexpr unsigned kKeyNegInf = 0x007fffffu; // key of -inf: candidates lie strictly above
constexpr int64_t kWsBytes = 256;            // reserved (nothing is kept off chip today; the ABI carries it for a multi-workgroup row)

static_assert(kMaxV <= 65536, "the tie select runs two 8-bit passes over the column index");

// float order as unsigned order; -0.0 and +0.0 get one key
__device__ __forceinline__ unsigned order_key(float x) {
    unsigned u = __float_as_uint(x);
    if (x == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Cut {
    unsigned T;      // threshold key
    int I;           // columns with key == T stay up to this index
};
__device__ __forceinline__ bool inside(const Cut& c, unsigned key, int v) { return key > c.T || (key == c.T && v <= c.I); }

struct Shared {
    unsigned cnt[256];
    u64 mass[256];
    unsigned wave_cnt[NW];
    u64 wave_w[NW];
    int sel_digit;
    unsigned sel_cnt, sel_above;
    u64 sel_w, sel_rem, acc;
    unsigned acc_cnt;
    float red_f[NW], red_x[NW];
    int red_i[NW];
};

// fixed-point mass of a logit: floor(exp((x - x_max) / tau) * 2^48); 0 for -inf and for anything that is not <= the maximum
__device__ __forceinline__ u64 mass_of(float x, float xmax, double tau) {
    const double a = ((double)x - (double)xmax) / tau;
    return a <= 0.0 ? (u64)(exp(a) * kMassScale) : 0ull;
}

// CONSTRAINED (sat_sample_filtered_ex, include/sat_hip.h): the row x is replaced by x' BEFORE anything else looks at it -- the
// maximum, both cuts, the draw and logp are those of x'.  Two LDS bitmaps of kMaxV bits: `ban` (x'[v] = -inf) and `seen` (the
// prefix tokens: x'[v] = x[v] > 0 ? x[v] / theta : x[v] * theta, one correctly rounded f32 operation, a token penalised once
// however often it occurs).  Every thread clears its words, one barrier, wave 0 asks for the row's prefix (lane j: y_j) and its
// share of the suppressed ids, the row loads follow -- the other waves' are in flight meanwhile -- then wave 0 sets the bits (the
// n-gram compare reads the neighbours' y by ds_bpermute, as the beam's row kernel does) and one barrier publishes them.  The
// register path transforms once behind Row::load() -- one word of each bitmap per 16-byte chunk: chunk q is the nibble 4 (q & 7) of
// word q >> 3, 8 neighbouring lanes read one word -- the looped path at every visit of Row::each.  Bans win over the penalty.
struct SampleBan {
    const int64_t* suppress;     // device [n_suppress]
    const int64_t* prefix;       // row r's tokens y_0 .. y_{t-1} at prefix[r * prefix_stride + j]
    long prefix_stride;
    long end_id;                 // banned at this step when >= 0 (the host has already compared t with min_length)
    int n_suppress;
    int depth;                   // prefix tokens to read: t when a rule of this step reads them, else 0
    int ngram;                   // n when n-gram blocking bans at this step (t >= n), else 0
    int block_repeat;            // y_{t-1} is banned at this step
    float theta;                 // repetition penalty of this step (1: none)
};
constexpr int kBanTMax = 64;     // prefix tokens a constrained step may read (lane j of wave 0 keeps y_j)
constexpr int kBanWords = kMaxV / 32;

__device__ __forceinline__ float penalised(float x, float theta) { return x > 0.0f ? __fdiv_rn(x, theta) : __fmul_rn(x, theta); }

// The row of one workgroup.  REG: 16-byte chunk q = tid + c * NT of the row in rc[c], the V % 4 leftover column 4 * nq + tid in
// xt, columns past V hold -inf (no candidates); masses, once filled, beside them.  !REG: every visit reloads from memory.
template <bool REG, bool CONS = false>
struct Row {
    f32x4 rc[REG ? RC : 1];
    float xt;
    u64 mq[REG ? RC * 4 : 1], mt;
    const float* x;
    int V, nq, tid;
    float xmax;
    double tau;
    const unsigned* ban;         // CONS only: the two bitmaps and the penalty
    const unsigned* seen;
    float theta;

    // x'[v] of the (NaN-free) logit xv in column v < V
    __device__ __forceinline__ float constrained(float xv, int v) const {
        const unsigned bit = 1u << (v & 31);
        if (seen[v >> 5] & bit) xv = penalised(xv, theta);
        return (ban[v >> 5] & bit) ? -INFINITY : xv;
    }
    // REG: the row in registers becomes x' (after load() and the barrier that publishes the bitmaps)
    __device__ __forceinline__ void constrain() {
        if constexpr (REG && CONS) {
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                const int q = tid + c * NT;
                const int w = q < nq ? q >> 3 : 0;           // (chunks past the row hold -inf whatever the bits say)
                const unsigned nb = ban[w] >> (4 * (q & 7)), ns = seen[w] >> (4 * (q & 7));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xv = ((ns >> e) & 1u) ? penalised(rc[c][e], theta) : rc[c][e];
                    rc[c][e] = ((nb >> e) & 1u) ? -INFINITY : xv;
                }
            }
            const int tail = (nq << 2) + tid;
            if (tail < V) xt = constrained(xt, tail);
        }
    }

    __device__ __forceinline__ void load() {
        if constexpr (REG) {
            // every load unconditional, chunk indexes past the row clamped and blanked below (as beam_row_kernel does)
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                const int q = tid + c * NT;
                rc[c] = *(const f32x4*)(x + 4 * (q < nq ? q : nq - 1));
            }
            const int tail = (nq << 2) + tid;
            xt = tail < V ? x[tail] : -INFINITY;
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                if (tid + c * NT >= nq) rc[c] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
                for (int e = 0; e < 4; ++e) rc[c][e] = rc[c][e] == rc[c][e] ? rc[c][e] : -INFINITY;       // NaN: no candidate
            }
            xt = xt == xt ? xt : -INFINITY;
        }
    }
    __device__ __forceinline__ void fill_masses() {
        if constexpr (REG) {
#pragma unroll
            for (int c = 0; c < RC; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) mq[c * 4 + e] = mass_of(rc[c][e], xmax, tau);
            mt = mass_of(xt, xmax, tau);
        }
    }
    // f(x, v, mass) for every column of this thread, v ascending; `mass` is valid only when with_mass
    template <class F>
    __device__ __forceinline__ void each(bool with_mass, F&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int c = 0; c < RC; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) f(rc[c][e], 4 * (tid + c * NT) + e, mq[c * 4 + e]);
            f(xt, (nq << 2) + tid, mt);
        } else {
            for (int v = tid; v < V; v += NT) {
                float xv = x[v];
                xv = xv == xv ? xv : -INFINITY;
                if constexpr (CONS) xv = constrained(xv, v);
                f(xv, v, with_mass ? mass_of(xv, xmax, tau) : 0ull);
            }
        }
    }
};

struct Pick {
    int digit;
    unsigned cnt, above;     // columns in the picked bin; columns in the bins in front of it
    u64 w, rem;              // weight of the picked bin; what is still to be covered inside it
};

// The bin in which the running weight, walking the 256 bins from the top (or, asc, from the bottom), reaches `rem` (>= 1; the
// bins hold at least that much).  weight = mass (by_mass) or count.  Block-wide inclusive scan: shuffles in the wave, wave totals
// through LDS.  Two barriers; the histogram may be cleared after it returns.
__device__ __forceinline__ Pick pick_bin(Shared& sh, bool asc, bool by_mass, u64 rem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bin = asc ? tid : 255 - tid;
    const unsigned c = sh.cnt[bin];
    const u64 w = by_mass ? sh.mass[bin] : (u64)c;
    unsigned ci = c;
    u64 wi = w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned oc = __shfl_up(ci, o, 64);
        const u64 ow = __shfl_up(wi, o, 64);
        if (lane >= o) { ci += oc; wi += ow; }
    }
    if (lane == 63) { sh.wave_cnt[wave] = ci; sh.wave_w[wave] = wi; }
    if (tid == 0) {              // (never read when the bins hold `rem`: keeps a row without a finite logit inside its bounds)
        sh.sel_digit = 0; sh.sel_cnt = 1; sh.sel_above = 0; sh.sel_w = 1; sh.sel_rem = 1;
    }
    __syncthreads();
    for (int q = 0; q < wave; ++q) { ci += sh.wave_cnt[q]; wi += sh.wave_w[q]; }
    if (w > 0 && wi >= rem && wi - w < rem) {          // exactly one bin
        sh.sel_digit = bin; sh.sel_cnt = c; sh.sel_above = ci - c; sh.sel_w = w; sh.sel_rem = rem - (wi - w);
    }
    __syncthreads();
    Pick p;
    p.digit = sh.sel_digit; p.cnt = sh.sel_cnt; p.above = sh.sel_above; p.w = sh.sel_w; p.rem = sh.sel_rem;
    return p;
}

// The shortest prefix of the total order, inside `cut`, whose weight (count, or MASS) reaches `target`: narrows `cut` to it and
// sets n to its size.  target >= 1 and at most the weight inside `cut`.
template <bool MASS, bool REG, bool CONS>
__device__ __forceinline__ void select_prefix(Row<REG, CONS>& row, Shared& sh, Cut& cut, int& n, u64 target) {
    const int tid = threadIdx.x;
    const Cut prior = cut;
    unsigned prefix = 0, above = 0;
    u64 rem = target;
    Pick p;
    for (int shift = 24; shift >= 0; shift -= 8) {
        sh.cnt[tid] = 0;
        if (MASS) sh.mass[tid] = 0;
        __syncthreads();
        // a thread's consecutive columns mostly share a digit in the first pass (same sign and exponent): runs are added once
        int rd = -1;
        unsigned rcnt = 0;
        u64 rm = 0;
        row.each(MASS, [&](float xv, int v, u64 m) {
            const unsigned key = order_key(xv);
            const bool hit = key > kKeyNegInf && inside(prior, key, v) && (shift == 24 || ((key ^ prefix) >> (shift + 8)) == 0);
            if (hit) {
                const int d = (int)((key >> shift) & 255u);
                if (d != rd) {
                    if (rcnt) { atomicAdd(&sh.cnt[rd], rcnt); if (MASS) atomicAdd(&sh.mass[rd], rm); }
                    rd = d; rcnt = 0; rm = 0;
                }
                ++rcnt;
                rm += m;
            }
        });
        if (rcnt) { atomicAdd(&sh.cnt[rd], rcnt); if (MASS) atomicAdd(&sh.mass[rd], rm); }
        __syncthreads();
        p = pick_bin(sh, false, MASS, rem);
        prefix |= (unsigned)p.digit << shift;
        above += p.above;
        rem = p.rem;
    }
    // p.cnt columns share the threshold value (and so the mass): the first `take` of them, by column, complete the prefix
    u64 take = rem;
    if (MASS) {
        const u64 m1 = p.w / (p.cnt ? p.cnt : 1u);
        take = m1 ? (rem + m1 - 1) / m1 : p.cnt;
    }
    if (take < 1) take = 1;
    if (take > p.cnt) take = p.cnt;
    int I = prefix == prior.T ? prior.I : INT_MAX;
    if (take < p.cnt) {
        unsigned ip = 0;
        u64 irem = take;
        for (int shift = 8; shift >= 0; shift -= 8) {
            sh.cnt[tid] = 0;
            __syncthreads();
            row.each(false, [&](float xv, int v, u64) {
                const unsigned key = order_key(xv);
                if (key == prefix && key > kKeyNegInf && inside(prior, key, v) && (shift == 8 || (((unsigned)v ^ ip) >> 8) == 0))
                    atomicAdd(&sh.cnt[((unsigned)v >> shift) & 255u], 1u);
            });
            __syncthreads();
            const Pick q = pick_bin(sh, true, false, irem);
            ip |= (unsigned)q.digit << shift;
            irem = q.rem;
        }
        I = (int)ip;
    }
    cut.T = prefix;
    cut.I = I;
    n = (int)(above + (unsigned)take);
}

// sum of the masses inside `cut` over the block (exact: integers)
template <bool REG, bool CONS>
__device__ __forceinline__ u64 mass_inside(Row<REG, CONS>& row, Shared& sh, const Cut& cut) {
    if (threadIdx.x == 0) sh.acc = 0;
    __syncthreads();
    u64 s = 0;
    row.each(true, [&](float xv, int v, u64 m) {
        const unsigned key = order_key(xv);
        if (key > kKeyNegInf && inside(cut, key, v)) s += m;
    });
    if (s) atomicAdd(&sh.acc, s);
    __syncthreads();
    const u64 r = sh.acc;
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// wave 0, after the barrier behind the clearing: the bits of row r's step.  y: y_lane of the prefix (-1: none, or outside [0, V));
// sup: the suppressed ids lane, lane + 64, .. of this lane
__device__ __forceinline__ void gather_bans(const SampleBan& b, int V, int lane, int y, const int64_t (&sup)[4], unsigned* s_ban,
                                            unsigned* s_seen) {
    auto set = [&](unsigned* map, long v) {
        if (v >= 0 && v < V) atomicOr(&map[v >> 5], 1u << (v & 31));
    };
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < b.n_suppress) set(s_ban, (long)sup[u]);
    if (lane == 0) set(s_ban, b.end_id);
    const int i = b.depth, n = b.ngram;
    if (i <= 0) return;                                      // (uniform)
    if (b.theta != 1.0f && lane < i) set(s_seen, y);
    if (b.block_repeat && lane == i - 1) set(s_ban, y);
    if (n >= 1 && i >= n) {
        // lane j: the n-gram that starts at j, 0 <= j <= i - n, bans its last token when its first n - 1 equal the tail
        bool same = true;
        for (int m = 0; m + 1 < n; ++m) {                    // (both reads by the whole wave: no short-circuit around a bpermute)
            const int mine = __shfl(y, (lane + m) & 63, 64), tail = __shfl(y, i - n + 1 + m, 64);
            same = same & (mine == tail);
        }
        const int lastv = __shfl(y, (lane + n - 1) & 63, 64);
        if (lane <= i - n && same) set(s_ban, lastv);
    }
}

template <bool REG, bool CONS>
__global__ __launch_bounds__(NT) void sample_filtered_kernel(const float* __restrict__ logits, long ldl, int V, float temperature,
                                                             int top_k, float top_p, unsigned key0, unsigned key1, unsigned t,
                                                             unsigned ctr3, int64_t* __restrict__ ids, long ids_stride,
                                                             float* __restrict__ logp, long logp_stride,
                                                             int32_t* __restrict__ kept, long kept_stride, SampleBan ban) {
    __shared__ Shared sh;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Row<REG, CONS> row;
    row.x = logits + (long)r * ldl;
    row.V = V;
    row.nq = V >> 2;
    row.tid = tid;
    row.tau = (double)temperature;
    row.xmax = -INFINITY;
    if constexpr (CONS) {
        __shared__ unsigned s_ban[kBanWords], s_seen[kBanWords];
        for (int w = tid; w < (V + 31) >> 5; w += NT) { s_ban[w] = 0u; s_seen[w] = 0u; }
        __syncthreads();
        int y = -1;
        int64_t sup[4] = {-1, -1, -1, -1};
        if (wave == 0) {                                     // asked for in front of the row: they arrive first
            if (lane < ban.depth) {
                const int64_t tk = ban.prefix[(long)r * ban.prefix_stride + lane];
                y = (tk >= 0 && tk < V) ? (int)tk : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (lane + 64 * u < ban.n_suppress) sup[u] = ban.suppress[lane + 64 * u];
        }
        row.ban = s_ban;
        row.seen = s_seen;
        row.theta = ban.theta;
        row.load();
        if (wave == 0) gather_bans(ban, V, lane, y, sup, s_ban, s_seen);
        __syncthreads();
        row.constrain();
    } else {
        row.load();
    }

    // the maximum and the number of candidates
    {
        float m = -INFINITY;
        unsigned nc = 0;
        row.each(false, [&](float xv, int, u64) {
            m = fmaxf(m, xv);
            nc += order_key(xv) > kKeyNegInf ? 1u : 0u;
        });
        m = wave_max(m);
        if (tid == 0) sh.acc_cnt = 0;
        if (lane == 0) sh.red_f[wave] = m;
        __syncthreads();
        if (nc) atomicAdd(&sh.acc_cnt, nc);
        __syncthreads();
        m = sh.red_f[0];
#pragma unroll
        for (int q = 1; q < NW; ++q) m = fmaxf(m, sh.red_f[q]);
        row.xmax = m;
    }
    const int ncand = (int)sh.acc_cnt;
    __syncthreads();                                          // (red_f is written again by the draw's reduction)
    Cut cut = {kKeyNegInf + 1u, INT_MAX};                     // every candidate
    int n = ncand;
    if (top_k > 0 && top_k < ncand) select_prefix<false, REG>(row, sh, cut, n, (u64)top_k);
    const bool nucleus = top_p < 1.0f && ncand > 0;
    if (nucleus || logp) row.fill_masses();
    if (nucleus) {
        const u64 Z = mass_inside(row, sh, cut);              // over what top-k left
        if (Z > 0) {
            const double want = ceil((double)top_p * (double)Z);
            u64 target = want >= 1.0 ? (u64)want : 1ull;
            if (target > Z) target = Z;
            select_prefix<true, REG>(row, sh, cut, n, target);
        }
    }
    const u64 Zk = logp ? mass_inside(row, sh, cut) : 0ull;

    // Gumbel-max over the kept columns: first arg-max of x / tau + G(r, t, v), G of counter (v >> 2, r, t, 2 * rank), word v & 3
    float bs = -INFINITY, bx = 0.0f;
    int bi = INT_MAX;
    auto offer = [&](float xv, int v, unsigned word) {
        const float s = xv / temperature + sat_gumbel(word);
        if (s > bs) { bs = s; bi = v; bx = xv; }              // columns arrive in ascending order: the first maximum stays
    };
    if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < RC; ++c) {
            const int v0 = 4 * (tid + c * NT);
            bool k[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned key = order_key(row.rc[c][e]);
                k[e] = key > kKeyNegInf && inside(cut, key, v0 + e);
            }
            if (k[0] || k[1] || k[2] || k[3]) {               // one Philox evaluation serves the chunk's four columns
                const u32x4 w = sat_philox4x32_10((unsigned)(v0 >> 2), (unsigned)r, t, ctr3, key0, key1);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k[e]) offer(row.rc[c][e], v0 + e, w[e]);
            }
        }
        const int vt = (row.nq << 2) + tid;
        const unsigned key = order_key(row.xt);
        if (key > kKeyNegInf && inside(cut, key, vt)) {
            const u32x4 w = sat_philox4x32_10((unsigned)(vt >> 2), (unsigned)r, t, ctr3, key0, key1);
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            const int e = vt & 3;
            offer(row.xt, vt, e == 0 ? w0 : e == 1 ? w1 : e == 2 ? w2 : w3);
        }
    } else {
        row.each(false, [&](float xv, int v, u64) {
            const unsigned key = order_key(xv);
            if (key > kKeyNegInf && inside(cut, key, v)) {
                const u32x4 w = sat_philox4x32_10((unsigned)(v >> 2), (unsigned)r, t, ctr3, key0, key1);
                const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
                const int e = v & 3;
                offer(xv, v, e == 0 ? w0 : e == 1 ? w1 : e == 2 ? w2 : w3);
            }
        });
    }
    const int mine = bi;
    {
        float gs = bs;
        int gi = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(gs, o, 64);
            const int oi = __shfl_xor(gi, o, 64);
            if (better(os, oi, gs, gi)) { gs = os; gi = oi; }
        }
        if (lane == 0) { sh.red_f[wave] = gs; sh.red_i[wave] = gi; }
        __syncthreads();
        bs = sh.red_f[0];
        bi = sh.red_i[0];
#pragma unroll
        for (int q = 1; q < NW; ++q)
            if (better(sh.red_f[q], sh.red_i[q], bs, bi)) { bs = sh.red_f[q]; bi = sh.red_i[q]; }
    }
    if (bi == INT_MAX) {                                      // no finite logit in the row: undefined token, inside [0, V)
        if (tid == 0) {
            ids[(long)r * ids_stride] = 0;
            if (kept) kept[(long)r * kept_stride] = n;
            if (logp) logp[(long)r * logp_stride] = -INFINITY;
        }
        return;
    }
    if (mine == bi) {                                         // the thread that holds the drawn column (indexes are unique)
        ids[(long)r * ids_stride] = bi < V ? bi : V - 1;
        if (kept) kept[(long)r * kept_stride] = n;
        // ln(w_tok / Z_kept) in f64, rounded once
        if (logp)
            logp[(long)r * logp_stride] =
                (float)(((double)bx - (double)row.xmax) / row.tau - log((double)Zk * (1.0 / kMassScale)));
    }
}

int filtered_check(const float* logits, int64_t ldl, int R, int V, float temperature, int top_k, float top_p, int t, int rank,
                   const int64_t* ids, const void* workspace, int64_t ws_bytes) {
    if (!logits || !ids || !workspace) return SAT_ERR_ARG;
    if (R < 1 || V < 1 || ldl < V || t < 0 || rank < 0 || top_k < 0) return SAT_ERR_ARG;
    if (!isfinite(temperature) || !(temperature > 0.0f)) return SAT_ERR_ARG;
    if (!(top_p > 0.0f) || !(top_p <= 1.0f)) return SAT_ERR_ARG;
    if (V > kMaxV) return SAT_ERR_UNSUPPORTED;
    if (ws_bytes < kWsBytes) return SAT_ERR_WORKSPACE;
    return SAT_OK;
}

int filtered_launch(const float* logits, int64_t ldl, int R, int V, float temperature, int top_k, float top_p, uint64_t seed, int t,
                    int rank, int64_t* ids, int64_t ids_stride, float* logp, int64_t logp_stride, int32_t* kept, int64_t kept_stride,
                    hipStream_t s, const SampleBan* ban = nullptr) {
    const unsigned key0 = (unsigned)(seed & 0xffffffffu), key1 = (unsigned)(seed >> 32);
    const int nq = V >> 2;
    // the register path: rows start on 16 bytes, hold a whole 16-byte chunk (nq - 1 clamps the loads past the row) and fit
    const bool reg = (ldl & 3) == 0 && (((uintptr_t)logits) & 15) == 0 && nq >= 1 && nq <= RC * NT;
    const SampleBan none = {};
#define SAT_SAMPLE_LAUNCH(REG, CONS)                                                                                                   \
    hipLaunchKernelGGL((sample_filtered_kernel<REG, CONS>), dim3(R), dim3(NT), 0, s, logits, (long)ldl, V, temperature, top_k, top_p,  \
                       key0, key1, (unsigned)t, 2u * (unsigned)rank, ids, (long)ids_stride, logp, (long)logp_stride, kept,             \
                       (long)kept_stride, ban ? *ban : none)
    if (ban) {
        if (reg) SAT_SAMPLE_LAUNCH(true, true);
        else SAT_SAMPLE_LAUNCH(false, true);
    } else {
        if (reg) SAT_SAMPLE_LAUNCH(true, false);
        else SAT_SAMPLE_LAUNCH(false, false);
    }
#undef SAT_SAMPLE_LAUNCH
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

// The constraints of an `_ex` call: SAT_ERR_ARG for what the header lists; *active: some field differs from "off"
int constraints_check(const sat_sample_constraints* c, bool* active) {
    *active = false;
    if (!c) return SAT_OK;
    if (c->n_suppress < 0 || c->min_length < 0 || c->no_repeat_ngram < 0 || (c->block_repeat != 0 && c->block_repeat != 1))
        return SAT_ERR_ARG;
    if (c->n_suppress > 256 || (c->n_suppress > 0 && !c->suppress_ids)) return SAT_ERR_ARG;
    if (!isfinite(c->repetition_penalty) || !(c->repetition_penalty > 0.0f)) return SAT_ERR_ARG;
    if (c->min_length > 0 && c->end_id < 0) return SAT_ERR_ARG;
    *active = c->n_suppress > 0 || c->min_length > 0 || c->no_repeat_ngram > 0 || c->block_repeat != 0 || c->repetition_penalty != 1.0f;
    return SAT_OK;
}

// What `c` does at step t, for the kernel; false: nothing -- the plain kernel serves the step
bool ban_of_step(const sat_sample_constraints* c, int t, const int64_t* prefix, int64_t prefix_stride, SampleBan* b) {
    *b = SampleBan{};
    b->suppress = c->suppress_ids;
    b->n_suppress = c->n_suppress;
    b->end_id = t < c->min_length ? (long)c->end_id : -1;
    b->ngram = (c->no_repeat_ngram >= 1 && t >= c->no_repeat_ngram) ? c->no_repeat_ngram : 0;
    b->block_repeat = (c->block_repeat && t >= 1) ? 1 : 0;
    b->theta = t >= 1 ? c->repetition_penalty : 1.0f;
    b->depth = (b->ngram || b->block_repeat || b->theta != 1.0f) ? t : 0;
    b->prefix = prefix;
    b->prefix_stride = (long)prefix_stride;
    return b->n_suppress > 0 || b->end_id >= 0 || b->depth > 0;
}

}  // namespace

extern "C" int64_t sat_sample_filtered_ws_bytes(int R, int V) { return (R < 1 || V < 1) ? 0 : kWsBytes; }

extern "C" int sat_sample_filtered(const float* logits, int64_t ldl, int R, int V, float temperature, int top_k, float top_p,
                                   uint64_t seed, int t, int rank, int64_t* ids, int64_t ids_stride, float* logp, int32_t* kept,
                                   void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    SAT_TRY(filtered_check(logits, ldl, R, V, temperature, top_k, top_p, t, rank, ids, workspace, ws_bytes));
    if (ids_stride < 1) return SAT_ERR_ARG;
    return filtered_launch(logits, ldl, R, V, temperature, top_k, top_p, seed, t, rank, ids, ids_stride, logp, 1, kept, 1,
                           (hipStream_t)stream);
}

// ---- `DecoderRNN.sample`'s loop (models.py:56-67) with a filtered draw where it takes the arg-max, as ONE call: steps x (LSTM step
//      per layer, exact-f32 vocab projection stored, sat_sample_filtered with t = the step, embedding row of the drawn id), enqueued
//      from C for the reason given at sat_greedy_decode.  State handling is sat_greedy_decode's (SatDecodeStack). ----
extern "C" int64_t sat_sample_decode_ws_bytes(int B, int E, int H, int V, int num_layers) {
    if (B < 1 || E < 1 || H < 1 || V < 1 || num_layers < 1) return 0;
    return al256((int64_t)B * ((V + 3) / 4 * 4) * 4) + al256(sat_sample_filtered_ws_bytes(B, V));
}

namespace {

// sat_sample_decode's loop; cons (NULL: none) is applied with the ids buffer itself as every row's prefix
int sample_decode(const float* features, const float* embed, const float* const* lstm_w, int num_layers, const float* lin_w,
                  const float* lin_b, int B, int E, int H, int V, int steps, float temperature, int top_k, float top_p, uint64_t seed,
                  int rank, float* h, float* c, float* h_tmp, float* x_tmp, int64_t* ids, int64_t ids_stride, float* logp,
                  int32_t* kept, float* logits_out, int64_t ldl, const sat_sample_constraints* cons, void* workspace,
                  int64_t ws_bytes, sat_stream_t stream) {
    SAT_TRY(sat_decode_check(features, embed, lstm_w, num_layers, lin_w, lin_b, B, E, H, V, steps, h, c, h_tmp, x_tmp, ids, ids_stride));
    if (!workspace || (logits_out && ldl < V)) return SAT_ERR_ARG;
    const int64_t lds = (V + 3) / 4 * 4, fws = al256((int64_t)B * lds * 4);
    SAT_TRY(filtered_check(features, V, B, V, temperature, top_k, top_p, 0, rank, ids, workspace, sat_sample_filtered_ws_bytes(B, V)));
    if (cons && steps > kBanTMax) return SAT_ERR_UNSUPPORTED;
    if (ws_bytes < sat_sample_decode_ws_bytes(B, E, H, V, num_layers)) return SAT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* step_logits = (float*)workspace;                    // [B][lds] when the caller keeps no logits
    if (!logits_out && lds > V) {                              // pad columns: no candidates, but keep them defined
        hipError_t e = hipMemsetAsync(step_logits, 0, (size_t)fws, s);
        if (e != hipSuccess) return (int)e;
    }
    SatDecodeStack stack(lstm_w, num_layers, B, E, H, h, c, h_tmp, stream);
    const float* x = features;
    for (int i = 0; i < steps; ++i) {
        const float* top;
        SAT_TRY(stack.step(x, &top));
        float* lg = logits_out ? logits_out + (long)i * B * ldl : step_logits;
        const int64_t ld = logits_out ? ldl : lds;
        SAT_TRY(sat_vocab_logits_fwd(top, lin_w, lin_b, B, H, V, lg, ld, stream));
        SampleBan ban;
        const bool bans = cons && ban_of_step(cons, i, ids, ids_stride, &ban);     // (a step `cons` leaves alone: the plain kernel)
        SAT_TRY(filtered_launch(lg, ld, B, V, temperature, top_k, top_p, seed, i, rank, ids + i, ids_stride, logp ? logp + i : nullptr,
                                steps, kept ? kept + i : nullptr, steps, s, bans ? &ban : nullptr));
        SAT_TRY(sat_embed_rows(embed, ids + i, ids_stride, B, E, V, x_tmp, stream));
        x = x_tmp;
    }
    return stack.finish();
}

}  // namespace

extern "C" int sat_sample_decode(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                                 const float* lin_w, const float* lin_b, int B, int E, int H, int V, int steps, float temperature,
                                 int top_k, float top_p, uint64_t seed, int rank, float* h, float* c, float* h_tmp, float* x_tmp,
                                 int64_t* ids, int64_t ids_stride, float* logp, int32_t* kept, float* logits_out, int64_t ldl,
                                 void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    return sample_decode(features, embed, lstm_w, num_layers, lin_w, lin_b, B, E, H, V, steps, temperature, top_k, top_p, seed, rank, h,
                         c, h_tmp, x_tmp, ids, ids_stride, logp, kept, logits_out, ldl, nullptr, workspace, ws_bytes, stream);
}

// ---- the constrained entry points (include/sat_hip.h): banned ids, n-gram blocking, repetition penalty on the row BEFORE the cuts ----
extern "C" int sat_sample_filtered_ex(const float* logits, int64_t ldl, int R, int V, float temperature, int top_k, float top_p,
                                      uint64_t seed, int t, int rank, int64_t* ids, int64_t ids_stride, float* logp, int32_t* kept,
                                      const sat_sample_constraints* c, const int64_t* prefix, int64_t prefix_stride, void* workspace,
                                      int64_t ws_bytes, sat_stream_t stream) {
    bool active = false;
    SAT_TRY(constraints_check(c, &active));
    SAT_TRY(filtered_check(logits, ldl, R, V, temperature, top_k, top_p, t, rank, ids, workspace, ws_bytes));
    if (ids_stride < 1) return SAT_ERR_ARG;
    SampleBan ban;
    const bool bans = active && ban_of_step(c, t, prefix, prefix_stride, &ban);
    if (bans && ban.depth > 0) {
        if (t >= kBanTMax) return SAT_ERR_UNSUPPORTED;
        if (!prefix || prefix_stride < 0) return SAT_ERR_ARG;
    }
    return filtered_launch(logits, ldl, R, V, temperature, top_k, top_p, seed, t, rank, ids, ids_stride, logp, 1, kept, 1,
                           (hipStream_t)stream, bans ? &ban : nullptr);
}

extern "C" int64_t sat_sample_decode_ex_ws_bytes(int B, int E, int H, int V, int num_layers) {
    return sat_sample_decode_ws_bytes(B, E, H, V, num_layers);
}

extern "C" int sat_sample_decode_ex(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                                    const float* lin_w, const float* lin_b, int B, int E, int H, int V, int steps, float temperature,
                                    int top_k, float top_p, uint64_t seed, int rank, float* h, float* c, float* h_tmp, float* x_tmp,
                                    int64_t* ids, int64_t ids_stride, float* logp, int32_t* kept, float* logits_out, int64_t ldl,
                                    const sat_sample_constraints* cons, void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    bool active = false;
    SAT_TRY(constraints_check(cons, &active));
    return sample_decode(features, embed, lstm_w, num_layers, lin_w, lin_b, B, E, H, V, steps, temperature, top_k, top_p, seed, rank, h,
                         c, h_tmp, x_tmp, ids, ids_stride, logp, kept, logits_out, ldl, active ? cons : nullptr, workspace, ws_bytes,
                         stream);
}
