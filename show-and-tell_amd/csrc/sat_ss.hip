// Scheduled sampling (Bengio et al. 2015) for the Show-and-Tell decoder's training forward: with probability ss_prob the input of
// step t >= 2 is a token DRAWN from softmax(logits of step t-1) instead of the teacher's captions[b][t-1] (the reference keeps
// `DecoderRNN.ss_prob`, models.py:38, and the schedule in train.py:109-113).  Step t+1's input then depends on step t's logits,
// so the teacher-forced forward's batched x-gates GEMM, persistent recurrence and one-shot vocab projection give way to a loop
// of, per step: one fused LSTM step per layer (both products + gates, sat_skinny_lstm), the vocab projection with the Gumbel-max
// draw in its epilogue (skinny_kernel<EPI_SAMPLE>), and one select + embedding-gather launch.  The tapes are exactly those of
// sat_lstm_fwd, so the teacher-forced backward runs unchanged on the tokens actually fed.
//
// Randomness: Philox4x32-10, key (seed lo, seed hi).  Noise of token v for row b of step t: counter (v >> 2, b, t, 2*rank),
// word v & 3, G = -log(-log u); mask: counter (0, b, t, 2*rank + 1), word 0; u = ((x >> 8) + 0.5) * 2^-24.  Every decision is a
// function of (seed, rank, b, t, v) alone, whatever the launch geometry.
#include "sat_internal.h"

int sat_skinny_sample(const float* h, const float* w, const float* b, int M, int H, int V, float* out, long ldo, unsigned key0,
                      unsigned key1, unsigned t, unsigned ctr3, float* pmax, int* pidx, hipStream_t s);

namespace {

// one workgroup per row b: mask(b, t) = u < ss_prob; if set, the arg-max of the Gumbel-max partials is the token fed to step t
// (its embedding row goes to x + b*x_stride), else the teacher's token (x's row already holds it).  teacher == NULL: every row
// samples.
__global__ __launch_bounds__(256) void ss_select_kernel(const float* __restrict__ pmax, const int* __restrict__ pidx, int ncg,
                                                        unsigned t, unsigned ctr3, unsigned key0, unsigned key1, float ss_prob,
                                                        const int64_t* __restrict__ teacher, long teacher_stride, int64_t* ids,
                                                        long ids_stride, const float* __restrict__ embed, int E, int V,
                                                        float* __restrict__ x, long x_stride) {
    __shared__ float sb[256];
    __shared__ int si[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (teacher) {
        const unsigned u = sat_philox4x32_10(0u, (unsigned)row, t, ctr3, key0, key1)[0] >> 8;
        // compared in f64: exact for every 24-bit u, so the decision is reproducible bit for bit off the device
        if (!(((double)u + 0.5) * 0x1p-24 < (double)ss_prob)) {
            if (tid == 0) ids[(long)row * ids_stride] = teacher[(long)row * teacher_stride];
            return;
        }
    }
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int c = tid; c < ncg; c += 256) {
        const float v = pmax[(long)row * ncg + c];
        const int i = pidx[(long)row * ncg + c];
        if (v > best || (v == best && i < bidx)) { best = v; bidx = i; }
    }
    sb[tid] = best; si[tid] = bidx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float ob = sb[tid + s];
            const int oi = si[tid + s];
            if (ob > sb[tid] || (ob == sb[tid] && oi < si[tid])) { sb[tid] = ob; si[tid] = oi; }
        }
        __syncthreads();
    }
    int tok = si[0];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);       // memory safety only (a NaN logit row has no arg-max)
    if (tid == 0) ids[(long)row * ids_stride] = tok;
    if (embed && x) {
        const float* src = embed + (long)tok * E;
        float* dst = x + (long)row * x_stride;
        for (int e = tid; e < E; e += 256) dst[e] = src[e];
    }
}

// used[b][j] = captions[b][j] for j < cols: the teacher's tokens wherever no draw replaces them
__global__ __launch_bounds__(256) void ss_init_used_kernel(const int64_t* __restrict__ captions, long cap_stride, int B, int cols,
                                                           int64_t* __restrict__ used, long used_stride) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * cols) return;
    const long b = i / cols, j = i % cols;
    used[b * used_stride + j] = captions[b * cap_stride + j];
}

// the select of one sampling step for rows 0 .. m_sel-1, from the partials sat_skinny_sample left in `workspace` for M rows
int select_step(int M, int m_sel, int V, float ss_prob, uint64_t seed, int t, int rank, const int64_t* teacher, long teacher_stride,
                int64_t* ids, long ids_stride, const float* embed, int E, float* x, long x_stride, float* workspace, hipStream_t s) {
    if (m_sel < 1) return SAT_OK;
    const int ncg = sat_cdiv(V, 16);
    hipLaunchKernelGGL(ss_select_kernel, dim3(m_sel), dim3(256), 0, s, workspace, (const int*)(workspace + (long)M * ncg), ncg,
                       (unsigned)t, 2u * (unsigned)rank + 1u, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), ss_prob, teacher,
                       teacher_stride, ids, ids_stride, embed, E, V, x, x_stride);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

// the projection of one sampling step: M rows (+ optional logits store), Gumbel-max partials into `workspace`
int sample_project(const float* h, const float* lin_w, const float* lin_b, int M, int H, int V, float* logits, long ldl, uint64_t seed,
                   int t, int rank, float* workspace, hipStream_t s) {
    return sat_skinny_sample(h, lin_w, lin_b, M, H, V, logits, ldl, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)t,
                             2u * (unsigned)rank, workspace, (int*)(workspace + (long)M * sat_cdiv(V, 16)), s);
}

// one sampling step: projection of M rows (+ optional logits store) and the draw for the first m_sel <= M of them
int sample_step(const float* h, const float* lin_w, const float* lin_b, int M, int m_sel, int H, int V, float* logits, long ldl,
                float ss_prob, uint64_t seed, int t, int rank, const int64_t* teacher, long teacher_stride, int64_t* ids,
                long ids_stride, const float* embed, int E, float* x, long x_stride, float* workspace, hipStream_t s) {
    SAT_TRY(sample_project(h, lin_w, lin_b, M, H, V, logits, ldl, seed, t, rank, workspace, s));
    return select_step(M, m_sel, V, ss_prob, seed, t, rank, teacher, teacher_stride, ids, ids_stride, embed, E, x, x_stride, workspace,
                       s);
}

// The LSTM stack of the two training loops below on sat_lstm_fwd's tapes: per layer the tapes GA, CS, HS, HP and the cell state
// (tapes[5l .. 5l+4]) and the weights (w_ih, w_hh, b_ih, b_hh) (lstm_w[4l .. 4l+3]).
struct TapedStack {
    float* const* tapes;
    const float* const* lstm_w;
    int num_layers, E, H;
    hipStream_t s;

    bool complete() const {
        for (int l = 0; l < num_layers; ++l)
            for (int k = 0; k < 5; ++k)
                if (!tapes[5 * l + k] || !lstm_w[4 * l + (k & 3)]) return false;
        return true;
    }

    // h_{-1} = c_{-1} = 0 for B rows
    int zero(int B) const {
        for (int l = 0; l < num_layers; ++l) {
            hipError_t e = hipMemsetAsync(tapes[5 * l + 3], 0, (size_t)B * H * sizeof(float), s);
            if (e == hipSuccess) e = hipMemsetAsync(tapes[5 * l + 4], 0, (size_t)B * H * sizeof(float), s);
            if (e != hipSuccess) return (int)e;
        }
        return SAT_OK;
    }

    // one step of the n rows at packed offset `off`, input rows inp [n][E]; *top = the top layer's h_t (its HS rows).  Per layer,
    // gates = h_{t-1} W_hh^T + x_t W_ih^T + b_ih + b_hh and the cell update in one launch; tapes GA (activated), CS, HS at the rows
    // of step t and h_t into HP's rows of step t+1 (n_next of them), as sat_lstm_fwd's per-step form leaves them
    int step(const float* inp, long off, int n, int n_next, const float** top) const {
        int In = E;
        for (int l = 0; l < num_layers; ++l) {
            float* GA = tapes[5 * l], *CS = tapes[5 * l + 1], *HS = tapes[5 * l + 2], *HP = tapes[5 * l + 3], *cst = tapes[5 * l + 4];
            SAT_TRY(sat_skinny_lstm(HP + off * H, lstm_w[4 * l + 1], inp, lstm_w[4 * l], In, lstm_w[4 * l + 2], lstm_w[4 * l + 3],
                                    nullptr, 0, n, H, cst, GA + off * 4 * H, 4L * H, CS + off * H, HS + off * H,
                                    n_next ? HP + (off + n) * H : nullptr, n_next, s));
            inp = HS + off * H;
            In = H;
        }
        *top = inp;
        return SAT_OK;
    }
};

}  // namespace

extern "C" int64_t sat_ss_decoder_fwd_ws_bytes(int B, int V) { return (int64_t)B * sat_cdiv(V, 16) * 8; }

extern "C" int sat_vocab_sample(const float* h, const float* lin_w, const float* lin_b, int B, int H, int V, float* logits,
                                int64_t ldl, float ss_prob, uint64_t seed, int t, int rank, const int64_t* teacher,
                                int64_t teacher_stride, int64_t* ids, int64_t ids_stride, const float* embed, int E, float* x,
                                float* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!h || !lin_w || !lin_b || !ids || !workspace || B < 1 || H < 4 || (H & 3) || V < 1 || t < 0 || rank < 0) return SAT_ERR_ARG;
    if ((logits && ldl < V) || (x && (!embed || E < 1))) return SAT_ERR_ARG;
    if (ws_bytes < sat_ss_decoder_fwd_ws_bytes(B, V)) return SAT_ERR_WORKSPACE;
    return sample_step(h, lin_w, lin_b, B, B, H, V, logits, ldl, ss_prob, seed, t, rank, teacher, teacher_stride, ids, ids_stride,
                       embed, E, x, E, workspace, (hipStream_t)stream);
}

extern "C" int sat_ss_decoder_fwd(const float* features, const float* embed, const int64_t* captions, int64_t cap_stride,
                                  const int32_t* batch_sizes, const int32_t* prefix, int T, int E, int V,
                                  const float* const* lstm_w, int num_layers, int H, const float* lin_w, const float* lin_b,
                                  float* const* tapes, float* X, float* logits, int64_t ldl, float ss_prob, uint64_t seed, int rank,
                                  int64_t* used, int64_t used_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!features || !embed || !batch_sizes || !prefix || !lstm_w || !lin_w || !lin_b || !tapes || !X || !workspace) return SAT_ERR_ARG;
    if (T < 1 || E < 4 || (E & 3) || H < 4 || (H & 3) || V < 1 || num_layers < 1 || num_layers > 8 || rank < 0) return SAT_ERR_ARG;
    if (T > 1 && (!captions || cap_stride < T - 1 || !used || used_stride < T - 1)) return SAT_ERR_ARG;
    if (logits && ldl < V) return SAT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const TapedStack stack{tapes, lstm_w, num_layers, E, H, s};
    if (!stack.complete()) return SAT_ERR_ARG;
    const int B = batch_sizes[0];
    long N = 0;
    for (int t = 0; t < T; ++t) {
        if (batch_sizes[t] < 1 || (t > 0 && batch_sizes[t] > batch_sizes[t - 1])) return SAT_ERR_ARG;
        N += batch_sizes[t];
    }
    if (ws_bytes < sat_ss_decoder_fwd_ws_bytes(B, V)) return SAT_ERR_WORKSPACE;
    // the teacher-forced inputs of every step (features, then embed[captions[b][t-1]]); draws overwrite rows step by step
    SAT_TRY(sat_embed_concat_fwd(features, embed, T > 1 ? captions : nullptr, cap_stride, prefix, T, (int)N, B, E, V, X, stream));
    if (T > 1) {
        hipLaunchKernelGGL(ss_init_used_kernel, dim3(sat_cdiv((long)B * (T - 1), 256)), dim3(256), 0, s, captions, (long)cap_stride, B,
                           T - 1, used, (long)used_stride);
        SAT_LAUNCH_CHECK();
    }
    SAT_TRY(stack.zero(B));
    long off = 0;
    for (int t = 0; t < T; ++t) {
        const int n = batch_sizes[t];
        const int n_next = (t + 1 < T) ? batch_sizes[t + 1] : 0;
        const float* inp;
        SAT_TRY(stack.step(X + off * E, off, n, n_next, &inp));
        float* lg = logits ? logits + off * ldl : nullptr;
        if (t >= 1 && t + 1 < T) {
            // the input of step t+1 >= 2: a draw from this step's logits where mask(b, t+1) holds, the teacher's token elsewhere
            SAT_TRY(sample_step(inp, lin_w, lin_b, n, n_next, H, V, lg, ldl, ss_prob, seed, t + 1, rank, captions + t, cap_stride,
                                used + t, used_stride, embed, E, X + (off + n) * E, E, workspace, s));
        } else if (lg) {
            // step 0 (its successor's input, <start>, is never replaced) and the last step: logits only
            SAT_TRY(sat_skinny_store(inp, H, lin_w, H, 0, n, V, H, 1, lg, ldl, 0, lin_b, s));
        }
        off += n;
    }
    return SAT_OK;
}

// ---- sampled rollout (self-critical sequence training, Rennie et al. 2017) -------------------------------------------------------
// DecoderRNN.sample (models.py:56-67) in training form, with a draw where the reference takes the arg-max: step 0 feeds the
// features, step t >= 1 feeds embed[ids[b][t-1]], and ids[b][t] = s(b, t) drawn from step t's own logits (counter t: every row
// draws at every step, no mask, no teacher).  All B rows run all `steps` steps, so the packed order is batch_sizes = [B] * steps
// and the tapes, X and the logits are those of a teacher-forced forward on ids[:, :steps-1]: its backward applies unchanged.
extern "C" int64_t sat_rollout_decoder_fwd_ws_bytes(int B, int V) { return sat_ss_decoder_fwd_ws_bytes(B, V); }

extern "C" int sat_rollout_decoder_fwd(const float* features, const float* embed, int B, int steps, int E, int V,
                                       const float* const* lstm_w, int num_layers, int H, const float* lin_w, const float* lin_b,
                                       float* const* tapes, float* X, float* logits, int64_t ldl, uint64_t seed, int rank, int64_t* ids,
                                       int64_t ids_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!features || !embed || !lstm_w || !lin_w || !lin_b || !tapes || !X || !logits || !ids || !workspace) return SAT_ERR_ARG;
    if (B < 1 || steps < 1 || E < 4 || (E & 3) || H < 4 || (H & 3) || V < 1 || num_layers < 1 || num_layers > 8 || rank < 0)
        return SAT_ERR_ARG;
    if (ldl < V || ids_stride < steps || (long)B * steps > 0x7fffffffL) return SAT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const TapedStack stack{tapes, lstm_w, num_layers, E, H, s};
    if (!stack.complete()) return SAT_ERR_ARG;
    if (ws_bytes < sat_rollout_decoder_fwd_ws_bytes(B, V)) return SAT_ERR_WORKSPACE;
    hipError_t e = hipMemcpyAsync(X, features, (size_t)B * E * sizeof(float), hipMemcpyDeviceToDevice, s);    // step 0's input
    if (e != hipSuccess) return (int)e;
    SAT_TRY(stack.zero(B));
    for (int t = 0; t < steps; ++t) {
        const long off = (long)t * B;
        const bool more = t + 1 < steps;
        const float* inp;
        SAT_TRY(stack.step(X + off * E, off, B, more ? B : 0, &inp));
        // ids[b][t] = s(b, t); its embedding row is step t+1's input (the last step's draw is a target only)
        SAT_TRY(sample_step(inp, lin_w, lin_b, B, B, H, V, logits + off * ldl, ldl, 1.0f, seed, t, rank, nullptr, 0, ids + t, ids_stride,
                            more ? embed : nullptr, E, more ? X + (off + B) * E : nullptr, E, workspace, s));
    }
    return SAT_OK;
}

// ---- Show-Attend-Tell (model2.py:38-85, the model train.py:37 builds) with scheduled sampling ------------------------------------
// The input of step t >= 1 is [emb | ctx_t]: with probability ss_prob the embedding half holds a token drawn from softmax(logits of
// step t-1), logits = classifier(context2out(ctx_{t-1}) + hidden2tout(h_{t-1})); the context half is always step t's own context.
// No one-column lag here (the image is not a step of its own): the draw for step t+1 uses counter t+1 and the logits of step t, so
// the output layer runs per step instead of once over all packed rows.  Per step: weight_hh projection (split-K skinny GEMM),
// attention (rows-dot + context, the context straight into X's context half), LSTMCell (tapes GATES / CS / HS), the output layer
// Z = [ctx | h] [W_c2o | W_h2o]^T + (b_c2o + b_h2o) as one two-product skinny GEMM, then the vocab projection with the Gumbel-max
// epilogue and the select (t + 1 < T), or the projection alone (last step).

namespace {

constexpr long kWsAlign = 256;

long ws_round(long n) { return (n + kWsAlign - 1) / kWsAlign * kWsAlign; }

// byte offsets of the pieces of the attention loop's workspace; the last entry is the total
struct SsAttendWs {
    long sample, att, skinny, cell, zbias, total;
};

// draw_bytes: the draw partials [B][cdiv(V,16)] (value, column) of sat_skinny_sample or sat_vocab_argmax
SsAttendWs ss_attend_ws(int B, int P, int C, int E, int H, int V, long draw_bytes) {
    long sk = 0;                                          // split-K slabs of the two per-step GEMMs, for every row count <= B
    for (int m = 1; m <= B; ++m) {
        const long a = sat_skinny_gemm_ws_bytes(m, C, H), b = sat_skinny_gemm_ws_bytes(m, E, C);
        sk = a > sk ? a : sk;
        sk = b > sk ? b : sk;
    }
    SsAttendWs w;
    w.sample = 0;
    w.att = w.sample + ws_round(draw_bytes);
    w.skinny = w.att + ws_round(sat_attention_ws_bytes(B, P));
    w.cell = w.skinny + ws_round(sk);
    w.zbias = w.cell + ws_round((long)B * H * sizeof(float));
    w.total = w.zbias + ws_round((long)E * sizeof(float));
    return w;
}

long rollout_draw_bytes(int B, int V) {
    const long a = sat_ss_decoder_fwd_ws_bytes(B, V), b = sat_vocab_argmax_ws_bytes(B, V);
    return a > b ? a : b;
}

// what sat_attention_fwd would refuse only after earlier steps had been enqueued
bool attention_fits(int P, int C) { return (long)2 * C * 4 <= 60 * 1024 && (long)(((P + 3) & ~3) + 8 + 8 * 64) * 4 <= 60 * 1024; }

// the weights, tapes and workspace pieces of one decoder loop (sat_ss_attend_fwd, sat_rollout_attend_fwd)
struct AttendLoop {
    const float *feats, *ctx_enc, *w_whh, *b_whh, *w_att, *embed, *w_ih, *w_hh, *b_ih, *b_hh, *w_c2o, *w_h2o, *w_cls, *b_cls;
    float *PROJ, *ALPHA, *X, *GATES, *CS, *HS, *Zin, *Z;
    float *sample_ws, *att_ws, *sk_ws, *cell, *zbias;
    long att_bytes, sk_bytes;
    int P, C, E, H, V;
    sat_stream_t stream;
};

AttendLoop attend_loop(const float* feats, const float* ctx_enc, int P, int C, int E, int H, int V, const float* const* w,
                       float* const* tapes, float* workspace, const SsAttendWs& lay, sat_stream_t stream) {
    char* base = (char*)workspace;
    AttendLoop a;
    a.feats = feats; a.ctx_enc = ctx_enc;
    a.w_whh = w[SAT_SSA_WEIGHT_HH_W]; a.b_whh = w[SAT_SSA_WEIGHT_HH_B]; a.w_att = w[SAT_SSA_WEIGHT_ATT];
    a.embed = w[SAT_SSA_EMBEDDING];
    a.w_ih = w[SAT_SSA_CELL_W_IH]; a.w_hh = w[SAT_SSA_CELL_W_HH]; a.b_ih = w[SAT_SSA_CELL_B_IH]; a.b_hh = w[SAT_SSA_CELL_B_HH];
    a.w_c2o = w[SAT_SSA_C2O_W]; a.w_h2o = w[SAT_SSA_H2O_W]; a.w_cls = w[SAT_SSA_CLS_W]; a.b_cls = w[SAT_SSA_CLS_B];
    a.PROJ = tapes[SAT_SSA_PROJ]; a.ALPHA = tapes[SAT_SSA_ALPHA]; a.X = tapes[SAT_SSA_X]; a.GATES = tapes[SAT_SSA_GATES];
    a.CS = tapes[SAT_SSA_CS]; a.HS = tapes[SAT_SSA_HS]; a.Zin = tapes[SAT_SSA_ZIN]; a.Z = tapes[SAT_SSA_Z];
    a.sample_ws = (float*)(base + lay.sample);
    a.att_ws = (float*)(base + lay.att);
    a.sk_ws = (float*)(base + lay.skinny);
    a.cell = (float*)(base + lay.cell);
    a.zbias = (float*)(base + lay.zbias);
    a.att_bytes = lay.skinny - lay.att;
    a.sk_bytes = lay.cell - lay.skinny;
    a.P = P; a.C = C; a.E = E; a.H = H; a.V = V;
    a.stream = stream;
    return a;
}

// One step of the loop for the n rows at packed offset `off`, five launches: weight_hh(h_{t-1}) (model2.py:74), the attention with
// its context into X's context half (model2.py:55-57, 73-78), the LSTMCell, the output layer (model2.py:80-84) Z = ctx W_c2o^T +
// h W_h2o^T + (b_c2o + b_h2o), and the vocab projection into lg -- with the Gumbel-max partials of counter (.., t_draw, 2*rank) left
// in sample_ws (draw), or alone.
int attend_step(const AttendLoop& a, const float* hprev, long off, int n, float* lg, long ldl, bool draw, uint64_t seed, int t_draw,
                int rank) {
    const int P = a.P, C = a.C, E = a.E, H = a.H, Hin = a.H;
    hipStream_t s = (hipStream_t)a.stream;
    float* x = a.X + off * Hin;
    SAT_TRY(sat_skinny_gemm2_f32(hprev, H, a.w_whh, H, H, nullptr, 0, nullptr, 0, 0, 0, n, C, a.b_whh, a.PROJ + off * C, C, a.sk_ws,
                                 a.sk_bytes, a.stream));
    SAT_TRY(sat_attention_fwd(a.ctx_enc, a.feats, a.PROJ + off * C, C, a.w_att, n, P, C, a.ALPHA + off * P, x + E, Hin, a.att_ws,
                              a.att_bytes, a.stream));
    SAT_TRY(sat_lstmcell_fwd(x, hprev, a.cell, a.w_ih, a.w_hh, a.b_ih, a.b_hh, n, Hin, H, a.HS + off * H, a.GATES + off * 4L * H,
                             a.CS + off * H, a.stream));
    SAT_TRY(sat_skinny_gemm2_f32(x + E, Hin, a.w_c2o, C, C, a.HS + off * H, H, a.w_h2o, H, H, 0, n, E, a.zbias, a.Z + off * E, E,
                                 a.sk_ws, a.sk_bytes, a.stream));
    if (draw) return sample_project(a.Z + off * E, a.w_cls, a.b_cls, n, E, a.V, lg, ldl, seed, t_draw, rank, a.sample_ws, s);
    return sat_skinny_store(a.Z + off * E, E, a.w_cls, E, 0, n, a.V, E, 1, lg, ldl, 0, a.b_cls, s);
}

// after the loop: the output layer's input tape [ctx | h] of every row (attend_backward's dWz) and the packed tokens actually fed
// (its embedding scatter)
int attend_finish(const AttendLoop& a, const int64_t* fed, long fed_stride, const int32_t* prefix, int T, long N, int64_t* toks) {
    const int C = a.C, H = a.H;
    SAT_TRY(sat_rows_copy(a.X + a.E, H, nullptr, 0, N, (int)N, C, a.Zin, C + H, a.stream));
    SAT_TRY(sat_rows_copy(a.HS, H, nullptr, 0, N, (int)N, H, a.Zin + C, C + H, a.stream));
    return sat_pack_tokens(fed, fed_stride, prefix, T, (int)N, 0, toks, a.stream);
}

}  // namespace

extern "C" int64_t sat_ss_attend_fwd_ws_bytes(int B, int P, int C, int E, int H, int V) {
    if (B < 1 || P < 1 || C < 1 || E < 1 || H < 1 || V < 1) return 0;
    return ss_attend_ws(B, P, C, E, H, V, sat_ss_decoder_fwd_ws_bytes(B, V)).total;
}

extern "C" int sat_ss_attend_fwd(const float* feats, const float* ctx_enc, const float* h0, const float* c0, const int64_t* captions,
                                 int64_t cap_stride, const int32_t* batch_sizes, const int32_t* prefix, int T, int P, int C, int E,
                                 int H, int V, const float* const* w, float* const* tapes, int64_t* toks, float* logits, int64_t ldl,
                                 float ss_prob, uint64_t seed, int rank, int64_t* used, int64_t used_stride, float* workspace,
                                 int64_t ws_bytes, sat_stream_t stream) {
    if (!feats || !ctx_enc || !h0 || !c0 || !captions || !batch_sizes || !prefix || !w || !tapes || !toks || !logits || !used ||
        !workspace)
        return SAT_ERR_ARG;
    if (T < 1 || P < 1 || C < 4 || (C & 3) || E < 4 || (E & 3) || H != E + C || V < 1 || rank < 0) return SAT_ERR_ARG;
    if (cap_stride < T || used_stride < T || ldl < V || (ldl & 3)) return SAT_ERR_ARG;
    for (int k = 0; k < SAT_SSA_NUM_WEIGHTS; ++k)
        if (!w[k]) return SAT_ERR_ARG;
    for (int k = 0; k < SAT_SSA_NUM_TAPES; ++k)
        if (!tapes[k]) return SAT_ERR_ARG;
    const int B = batch_sizes[0];
    long N = 0;
    for (int t = 0; t < T; ++t) {
        if (batch_sizes[t] < 1 || (t > 0 && batch_sizes[t] > batch_sizes[t - 1])) return SAT_ERR_ARG;
        N += batch_sizes[t];
    }
    if (!attention_fits(P, C)) return SAT_ERR_UNSUPPORTED;
    const SsAttendWs lay = ss_attend_ws(B, P, C, E, H, V, sat_ss_decoder_fwd_ws_bytes(B, V));
    if (ws_bytes < lay.total) return SAT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const AttendLoop a = attend_loop(feats, ctx_enc, P, C, E, H, V, w, tapes, workspace, lay, stream);

    SAT_TRY(sat_rows_add(w[SAT_SSA_C2O_B], E, w[SAT_SSA_H2O_B], E, 1, E, a.zbias, E, stream));
    // used = the teacher's tokens; X's embedding half = their rows (draws overwrite both, step by step)
    hipLaunchKernelGGL(ss_init_used_kernel, dim3(sat_cdiv((long)B * T, 256)), dim3(256), 0, s, captions, (long)cap_stride, B, T, used,
                       (long)used_stride);
    SAT_LAUNCH_CHECK();
    SAT_TRY(sat_pack_tokens(used, used_stride, prefix, T, (int)N, 0, toks, stream));
    SAT_TRY(sat_rows_copy(a.embed, E, toks, 1, V, (int)N, E, a.X, H, stream));
    hipError_t e = hipMemcpyAsync(a.cell, c0, (size_t)B * H * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return (int)e;
    long off = 0, prev = 0;
    for (int t = 0; t < T; ++t) {
        const int n = batch_sizes[t];
        const int n_next = (t + 1 < T) ? batch_sizes[t + 1] : 0;
        // the last step projects only; before it, the input of step t+1 is a draw from this step's logits where mask(b, t+1) holds,
        // the teacher's token elsewhere
        SAT_TRY(attend_step(a, t == 0 ? h0 : a.HS + prev * H, off, n, logits + off * ldl, ldl, n_next > 0, seed, t + 1, rank));
        SAT_TRY(select_step(n, n_next, V, ss_prob, seed, t + 1, rank, captions + t + 1, cap_stride, used + t + 1, used_stride, a.embed,
                            E, a.X + (off + n) * H, H, a.sample_ws, s));
        prev = off;
        off += n;
    }
    return attend_finish(a, used, used_stride, prefix, T, N, toks);
}

// ---- sampled / arg-max rollout of the attention decoder (self-critical sequence training on the model train.py:37 builds) --------
// The loop above with batch_sizes = [B] * steps, <start> at step 0 and ids[b][t-1] fed to step t >= 1, where ids[b][t] comes from step
// t's OWN logits (counter t, as sat_rollout_decoder_fwd): the Gumbel-max draw, or with `greedy` the first maximal column -- the
// greedy decode of the very policy the draws come from (h0 / c0 from init_lstm, no lagging context), which is what a self-critical
// baseline needs.  fed = [start_id | ids[:, :steps-1]]; the tapes are those of the teacher-forced forward on fed.
extern "C" int64_t sat_rollout_attend_fwd_ws_bytes(int B, int P, int C, int E, int H, int V) {
    if (B < 1 || P < 1 || C < 1 || E < 1 || H < 1 || V < 1) return 0;
    return ss_attend_ws(B, P, C, E, H, V, rollout_draw_bytes(B, V)).total;
}

extern "C" int sat_rollout_attend_fwd(const float* feats, const float* ctx_enc, const float* h0, const float* c0,
                                      const int32_t* prefix, int B, int steps, int P, int C, int E, int H, int V,
                                      const float* const* w, float* const* tapes, int64_t* toks, float* logits, int64_t ldl, int greedy,
                                      int64_t start_id, uint64_t seed, int rank, int64_t* ids, int64_t ids_stride, int64_t* fed,
                                      int64_t fed_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!feats || !ctx_enc || !h0 || !c0 || !prefix || !w || !tapes || !toks || !logits || !ids || !fed || !workspace)
        return SAT_ERR_ARG;
    if (B < 1 || steps < 1 || P < 1 || C < 4 || (C & 3) || E < 4 || (E & 3) || H != E + C || V < 1) return SAT_ERR_ARG;
    if (!greedy && rank < 0) return SAT_ERR_ARG;
    if (start_id < 0 || start_id >= V || (long)B * steps > 0x7fffffffL) return SAT_ERR_ARG;
    if (ids_stride < steps || fed_stride < steps || ldl < V || (ldl & 3)) return SAT_ERR_ARG;
    for (int k = 0; k < SAT_SSA_NUM_WEIGHTS; ++k)
        if (!w[k]) return SAT_ERR_ARG;
    for (int k = 0; k < SAT_SSA_NUM_TAPES; ++k)
        if (!tapes[k]) return SAT_ERR_ARG;
    if (!attention_fits(P, C)) return SAT_ERR_UNSUPPORTED;
    const long draw_bytes = rollout_draw_bytes(B, V);
    const SsAttendWs lay = ss_attend_ws(B, P, C, E, H, V, draw_bytes);
    if (ws_bytes < lay.total) return SAT_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const AttendLoop a = attend_loop(feats, ctx_enc, P, C, E, H, V, w, tapes, workspace, lay, stream);
    const long N = (long)B * steps;

    SAT_TRY(sat_rows_add(w[SAT_SSA_C2O_B], E, w[SAT_SSA_H2O_B], E, 1, E, a.zbias, E, stream));
    // step 0 feeds <start>: toks[0 .. B) = start_id (0 + start_id), fed's column 0 = those, X's embedding half = their rows
    hipError_t e = hipMemsetAsync(toks, 0, (size_t)B * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    SAT_TRY(sat_counter_add(toks, B, start_id, stream));
    hipLaunchKernelGGL(ss_init_used_kernel, dim3(sat_cdiv((long)B, 256)), dim3(256), 0, s, toks, 1L, B, 1, fed, (long)fed_stride);
    SAT_LAUNCH_CHECK();
    SAT_TRY(sat_rows_copy(a.embed, E, toks, 1, V, B, E, a.X, H, stream));
    e = hipMemcpyAsync(a.cell, c0, (size_t)B * H * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return (int)e;
    for (int t = 0; t < steps; ++t) {
        const long off = (long)t * B;
        const bool more = t + 1 < steps;
        float* x_next = more ? a.X + (off + B) * H : nullptr;
        SAT_TRY(attend_step(a, t == 0 ? h0 : a.HS + (off - B) * H, off, B, logits + off * ldl, ldl, !greedy, seed, t, rank));
        // ids[b][t]; its embedding row is step t+1's input (the last step's token is a target only)
        if (!greedy) {
            SAT_TRY(select_step(B, B, V, 1.0f, seed, t, rank, nullptr, 0, ids + t, ids_stride, more ? a.embed : nullptr, E, x_next, H,
                                a.sample_ws, s));
        } else {
            SAT_TRY(sat_vocab_argmax(a.Z + off * E, a.w_cls, a.b_cls, B, E, V, ids + t, ids_stride, a.sample_ws, draw_bytes, stream));
            if (more) SAT_TRY(sat_rows_copy(a.embed, E, ids + t, ids_stride, V, B, E, x_next, H, stream));
        }
    }
    if (steps > 1) {                                          // fed[:, 1:] = ids[:, :steps-1]
        hipLaunchKernelGGL(ss_init_used_kernel, dim3(sat_cdiv((long)B * (steps - 1), 256)), dim3(256), 0, s, ids, (long)ids_stride, B,
                           steps - 1, fed + 1, (long)fed_stride);
        SAT_LAUNCH_CHECK();
    }
    return attend_finish(a, fed, fed_stride, prefix, steps, N, toks);
}
