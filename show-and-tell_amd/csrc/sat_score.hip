// Scoring GIVEN captions: log p(token | image, prefix) per token, summed per caption (include/sat_hip.h, "Scoring given captions").
//
//   sat_vocab_logp        tok_logp[n] = x[n][t_n] - logsumexp_v x[n][v],  x = Hs w^T + b, WITHOUT the [N, V] logits in memory
//   sat_caption_logp_sum  packed rows -> captions, f64, one thread per caption, steps ascending
//   sat_score_captions    the Show-and-Tell decoder (models.py:47-53) teacher-forced on R (image, caption) rows, then the two above
//
// sat_vocab_logp, fast path (the shapes sat_gemm_f32x3 takes, V % 4 == 0): gemm_x3_kernel<BM, LOGP = true> (sat_gemm_x3_tile.h) is
// sat_gemm_f32x3's kernel -- same K loop, same tile map -- whose epilogue leaves, per 128-column tile and row, the pair
// (max, sum exp(x - max)) in partials[tile][row] and, from the one tile that holds the target column, the target logit.  A second
// launch, one thread per row, joins the ceil(V / 128) pairs in ascending tile order in f64 and rounds once.  No atomics; a row's
// arithmetic depends neither on the tile's place in the grid nor on the row tile's height, so the same row gives the same bits in
// any batch.  The column-tile form (one workgroup per (row tile, column tile), pairs through memory) was kept over a persistent
// one-workgroup-per-row-tile form with an online log-sum-exp in registers: the latter reads every weight slice once per row tile
// from L2 with no sharing between the row tiles of an XCD, which is what the tile map of sat_gemm_f32x3 exists for, and the pairs
// are 8 bytes per 128 columns (1 / 64 of the logits they replace).
// General path (every other shape): chunks of rows are projected into a BOUNDED scratch by sat_vocab_logits_fwd's GEMM and reduced
// by sat_ce_rows(write_grad = 0); the chunk height comes from the workspace given and changes no row's arithmetic.
#include "sat_decode_state.h"
#include "sat_gemm_x3_tile.h"

namespace {

// one thread per row: the tiles' (max, sum) pairs in ascending tile order, f64, one rounding per output
__global__ __launch_bounds__(256) void logp_merge_kernel(const float* __restrict__ partials, long pstride, int tiles_n,
                                                         const float* __restrict__ tlogit, int N, float* __restrict__ tok_logp,
                                                         float* __restrict__ lse_out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float mm = -INFINITY;
    for (int j = 0; j < tiles_n; ++j) mm = fmaxf(mm, partials[((long)j * pstride + n) * 2]);
    double s = 0.0;
    for (int j = 0; j < tiles_n; ++j) {
        const float mj = partials[((long)j * pstride + n) * 2], sj = partials[((long)j * pstride + n) * 2 + 1];
        if (mj != -INFINITY) s += (double)sj * exp((double)mj - (double)mm);
    }
    const double lse = (double)mm + log(s);
    tok_logp[n] = (float)((double)tlogit[n] - lse);
    if (lse_out) lse_out[n] = (float)lse;
}

// general path, behind sat_ce_rows: tok[row] = -row_loss[row] (in place); lse[row] from the chunk's logits, the sum in f64
__global__ __launch_bounds__(256) void logp_rows_finish_kernel(const float* __restrict__ logits, long ldl, int V, float* __restrict__ tok,
                                                               float* __restrict__ lse) {
    __shared__ float sh_m[4];
    __shared__ double sh_s[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (!lse) {
        if (tid == 0) tok[row] = -tok[row];
        return;
    }
    const float* x = logits + (long)row * ldl;
    float m = -INFINITY;
    for (int i = tid; i < V; i += 256) m = fmaxf(m, x[i]);
    m = wave_max(m);
    if ((tid & 63) == 0) sh_m[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
    double s = 0.0;
    if (m != -INFINITY)
        for (int i = tid; i < V; i += 256) s += (double)expf(x[i] - m);
    sh_s[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += sh_s[i];
        lse[row] = (float)((double)m + log(t));
        tok[row] = -tok[row];
    }
}

__global__ __launch_bounds__(256) void caption_logp_sum_kernel(const float* __restrict__ tok_logp, const int32_t* __restrict__ prefix,
                                                               int T, int R, double* __restrict__ logp, int32_t* __restrict__ len,
                                                               float* __restrict__ tok_out, long tok_stride) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    double s = 0.0;
    int n = 0;
    for (int t = 0; t < T; ++t) {
        const int p0 = prefix[t], bs = prefix[t + 1] - p0;
        float v = 0.0f;
        if (r < bs) {
            v = tok_logp[p0 + r];
            s += (double)v;
            ++n;
        }
        if (tok_out) tok_out[(long)r * tok_stride + t] = v;
    }
    logp[r] = s;
    len[r] = n;
}

// dst[l][r][:] = src[l][row_image[r]][:] for the state tensors h, c [L][B_img][H] -> [L][R][H]; 16-byte chunks
__global__ __launch_bounds__(256) void score_gather_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_image,
                                                                int B_img, int R, int H4, float* __restrict__ dst, long total) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int q = (int)(idx % H4);
        const long r = idx / H4;
        int b = row_image[r];
        b = b < 0 ? 0 : (b >= B_img ? B_img - 1 : b);
        ((f32x4*)dst)[r * H4 + q] = ((const f32x4*)src)[(long)b * H4 + q];
    }
}

// step t of the live rows r < rows: targets[r] = captions[row_caption[r]][t]; with x: x[r] = embed[captions[row_caption[r]][t - 1]].
// Ids and caption indices are clamped for memory safety only (the host wrapper range-checks the caption matrix).
__global__ __launch_bounds__(256) void score_step_inputs_kernel(const float* __restrict__ embed, const int64_t* __restrict__ captions,
                                                                long cap_stride, int C, const int32_t* __restrict__ row_caption, int t,
                                                                int rows, int E4, int V, float* __restrict__ x,
                                                                int64_t* __restrict__ targets) {
    const int r = blockIdx.x;
    int c = row_caption[r];
    c = c < 0 ? 0 : (c >= C ? C - 1 : c);
    const int64_t* cap = captions + (long)c * cap_stride;
    if (threadIdx.x == 0) targets[r] = cap[t];
    if (!x) return;
    long id = cap[t - 1];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    for (int q = threadIdx.x; q < E4; q += 256) ((f32x4*)x)[(long)r * E4 + q] = ((const f32x4*)embed)[id * E4 + q];
}

constexpr long kLogpScratchCap = 64L << 20;       // general path: bytes of logits in flight

inline bool logp_fast_shape(int H, int V) { return sat_gemm_f32x3_packed_bytes(V, H) > 0 && (V & 3) == 0; }
inline long pad4l(long n) { return (n + 3) / 4 * 4; }
// fast path: partials + target logits; general path: `rows` rows of logits
inline int64_t logp_core_bytes(int N, int H, int V, long rows) {
    if (logp_fast_shape(H, V)) return al256((int64_t)sat_cdiv(V, 128) * N * 8) + al256((int64_t)N * 4);
    if (rows > N) rows = N;
    return al256(rows * pad4l(V) * 4);
}
inline long logp_default_rows(int V) {
    const long rows = kLogpScratchCap / (pad4l(V) * 4);
    return rows < 1 ? 1 : rows;
}

}  // namespace

// chunk_rows: the general path's scratch height (TESTS make it small to cross a chunk edge at a small N; no effect on the fast path)
extern "C" int64_t sat_vocab_logp_ws_bytes_rows(int N, int H, int V, int chunk_rows) {
    if (N < 1 || H < 1 || V < 1 || chunk_rows < 1) return 0;
    return logp_core_bytes(N, H, V, chunk_rows) + (logp_fast_shape(H, V) ? al256(sat_gemm_f32x3_packed_bytes(V, H)) : 0);
}

extern "C" int64_t sat_vocab_logp_ws_bytes(int N, int H, int V) {
    if (V < 1) return 0;
    const long rows = logp_default_rows(V);
    return sat_vocab_logp_ws_bytes_rows(N, H, V, rows > N ? N : (int)rows);
}

extern "C" int sat_vocab_logp(const float* Hs, int64_t lda, const float* w, const void* w_packed, const float* b, const int64_t* targets,
                              int N, int H, int V, float* tok_logp, float* lse, void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!Hs || !w || !b || !targets || !tok_logp || !workspace) return SAT_ERR_ARG;
    if (N < 1 || H < 1 || V < 1 || lda < H) return SAT_ERR_ARG;
    if ((((uintptr_t)Hs | (uintptr_t)w | (uintptr_t)workspace) & 15) || (lda & 3) || (H & 3)) return SAT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (logp_fast_shape(H, V)) {
        const int64_t core = logp_core_bytes(N, H, V, 0);
        if (ws_bytes < core + (w_packed ? 0 : al256(sat_gemm_f32x3_packed_bytes(V, H)))) return SAT_ERR_ARG;
        if (w_packed && ((uintptr_t)w_packed & 15)) return SAT_ERR_ARG;
        const int tiles_n = sat_cdiv(V, 128);
        float* partials = (float*)ws;
        float* tlogit = (float*)(ws + al256((int64_t)tiles_n * N * 8));
        if (!w_packed) {
            void* pk = ws + core;
            SAT_TRY(sat_gemm_f32x3_pack(w, V, H, pk, stream));
            w_packed = pk;
        }
        // row chunks: the activation buffer descriptor of a launch spans less than 2^31 bytes
        const long max_rows = (0x7fffffe0L / (lda * 4)) / 128 * 128;
        if (max_rows < 128) return SAT_ERR_UNSUPPORTED;
        for (long row0 = 0; row0 < N; row0 += max_rows) {
            const int M = (int)(N - row0 < max_rows ? N - row0 : max_rows);
            X3Args a = {};
            a.A = Hs + row0 * lda; a.lda = lda; a.Bp = (const char*)w_packed; a.bias = b;
            a.M = M; a.N = V; a.K = H;
            a.a_bytes = (long)M * lda * 4;
            a.targets = targets + row0; a.partials = partials + row0 * 2; a.pstride = N; a.tlogit = tlogit + row0;
            // the row tile's height by sat_gemm_f32x3's rule (without that entry point's SAT_X3_BM override)
            if (x3_tall_tiles(M, tiles_n)) {
                a.tiles_m = sat_cdiv(M, 128);
                hipLaunchKernelGGL((gemm_x3_kernel<128, true>), dim3(a.tiles_m * tiles_n), dim3(256), 0, s, a);
            } else {
                a.tiles_m = sat_cdiv(M, 64);
                hipLaunchKernelGGL((gemm_x3_kernel<64, true>), dim3(a.tiles_m * tiles_n), dim3(256), 0, s, a);
            }
            SAT_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(logp_merge_kernel, dim3(sat_cdiv(N, 256)), dim3(256), 0, s, partials, (long)N, tiles_n, tlogit, N, tok_logp, lse);
        SAT_LAUNCH_CHECK();
        return SAT_OK;
    }
    const long ldl = pad4l(V);
    long rows = ws_bytes / (ldl * 4);
    if (rows < 1) return SAT_ERR_ARG;
    if (rows > N) rows = N;
    float* logits = (float*)ws;
    for (long row0 = 0; row0 < N; row0 += rows) {
        const int M = (int)(N - row0 < rows ? N - row0 : rows);
        if (lda == H) SAT_TRY(sat_vocab_logits_fwd(Hs + row0 * lda, w, b, M, H, V, logits, ldl, stream));
        else SAT_TRY(sat_gemm_f32(0, 0, Hs + row0 * lda, lda, w, H, logits, ldl, b, nullptr, M, V, H, stream));   // the same GEMM, strided rows
        SAT_TRY(sat_ce_rows(logits, ldl, targets + row0, M, V, 1.0f, 0, tok_logp + row0, nullptr, stream));
        hipLaunchKernelGGL(logp_rows_finish_kernel, dim3(M), dim3(256), 0, s, logits, ldl, V, tok_logp + row0, lse ? lse + row0 : nullptr);
        SAT_LAUNCH_CHECK();
    }
    return SAT_OK;
}

extern "C" int sat_caption_logp_sum(const float* tok_logp, const int32_t* prefix, int T, int R, double* logp, int32_t* len, float* tok_out,
                                    int64_t tok_stride, sat_stream_t stream) {
    if (!tok_logp || !prefix || !logp || !len || T < 1 || R < 1 || (tok_out && tok_stride < T)) return SAT_ERR_ARG;
    hipLaunchKernelGGL(caption_logp_sum_kernel, dim3(sat_cdiv(R, 256)), dim3(256), 0, (hipStream_t)stream, tok_logp, prefix, T, R, logp,
                       len, tok_out, (long)tok_stride);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

namespace {

// the pieces of sat_score_captions' workspace, in order
struct ScoreLayout {
    int64_t hs, tok, targets, x, img_h, img_c, low_h, row_c, packed, logp, total;
    ScoreLayout(int B_img, int R, int N, int E, int H, int V, int L) {
        int64_t o = 0;
        auto take = [&](int64_t bytes) { const int64_t at = o; o += al256(bytes); return at; };
        hs = take((int64_t)N * H * 4);                    // top layer's h of every live (step, row): the projection's operand
        tok = take((int64_t)N * 4);
        targets = take((int64_t)N * 8);
        x = take((int64_t)R * E * 4);                     // a step's embedding rows
        img_h = take((int64_t)L * B_img * H * 4 * 2);     // step 0 on the image rows: zero h (in), h (out)
        img_c = take((int64_t)L * B_img * H * 4);
        low_h = take((int64_t)(L - 1) * R * H * 4 * 2);   // layers below the top: two copies (sat_lstm_step reads one, writes the other)
        row_c = take((int64_t)L * R * H * 4);
        packed = take(logp_fast_shape(H, V) ? sat_gemm_f32x3_packed_bytes(V, H) : 0);
        logp = take(logp_core_bytes(N, H, V, logp_default_rows(V)));
        total = o;
    }
};

}  // namespace

extern "C" int64_t sat_score_captions_ws_bytes(int B_img, int R, int N, int E, int H, int V, int num_layers) {
    if (B_img < 1 || R < 1 || N < R || E < 1 || H < 1 || V < 1 || num_layers < 1 || num_layers > 8) return 0;
    return ScoreLayout(B_img, R, N, E, H, V, num_layers).total;
}

extern "C" int sat_score_captions(const float* features, const float* embed, const float* const* lstm_w, int num_layers,
                                  const float* lin_w, const float* lin_b, const int64_t* captions, int64_t cap_stride, int C,
                                  const int32_t* row_image, const int32_t* row_caption, const int32_t* batch_sizes,
                                  const int32_t* prefix, int T, int B_img, int R, int N, int E, int H, int V, double* logp, int32_t* len,
                                  float* tok_out, int64_t tok_stride, void* workspace, int64_t ws_bytes, sat_stream_t stream) {
    if (!features || !embed || !lstm_w || !lin_w || !lin_b || !captions || !row_image || !row_caption || !batch_sizes || !prefix ||
        !logp || !len || !workspace)
        return SAT_ERR_ARG;
    if (B_img < 1 || R < 1 || C < 1 || T < 1 || E < 1 || H < 1 || V < 1 || num_layers < 1 || num_layers > 8) return SAT_ERR_ARG;
    if ((E & 3) || (H & 3) || cap_stride < T || (tok_out && tok_stride < T) || ((uintptr_t)workspace & 255)) return SAT_ERR_ARG;
    for (int i = 0; i < 4 * num_layers; ++i)
        if (!lstm_w[i]) return SAT_ERR_ARG;
    long sum = 0;
    for (int t = 0; t < T; ++t) {
        if (batch_sizes[t] < 1 || batch_sizes[t] > (t ? batch_sizes[t - 1] : R)) return SAT_ERR_ARG;
        sum += batch_sizes[t];
    }
    if (batch_sizes[0] != R || sum != N) return SAT_ERR_ARG;
    const ScoreLayout lay(B_img, R, N, E, H, V, num_layers);
    if (ws_bytes < lay.total) return SAT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* Hs = (float*)(ws + lay.hs);
    float* tok = (float*)(ws + lay.tok);
    int64_t* targets = (int64_t*)(ws + lay.targets);
    float* x = (float*)(ws + lay.x);
    const long LB = (long)num_layers * B_img * H;
    float* img_h0 = (float*)(ws + lay.img_h);
    float* img_h1 = img_h0 + LB;
    float* img_c = (float*)(ws + lay.img_c);
    float* low_h = (float*)(ws + lay.low_h);
    float* row_c = (float*)(ws + lay.row_c);

    // step 0 feeds the features: every caption of an image shares that state, so it runs on the B_img image rows only
    hipError_t e = hipMemsetAsync(img_h0, 0, (size_t)LB * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(img_c, 0, (size_t)LB * 4, s);
    if (e != hipSuccess) return (int)e;
    {
        SatDecodeStack img(lstm_w, num_layers, B_img, E, H, img_h0, img_c, img_h1, stream);
        const float* top;
        SAT_TRY(img.step(features, &top));               // every layer's new h now sits in img_h1
    }
    SatScoreStack stack(lstm_w, num_layers, R, E, H, low_h, row_c, stream);
    const int H4 = H / 4;
    auto gather = [&](const float* src, float* dst) -> int {
        const long total = (long)R * H4;
        int grid = sat_cdiv(total, 256);
        if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(score_gather_rows_kernel, dim3(grid), dim3(256), 0, s, src, row_image, B_img, R, H4, dst, total);
        SAT_LAUNCH_CHECK();
        return SAT_OK;
    };
    for (int l = 0; l < num_layers; ++l) {
        SAT_TRY(gather(img_h1 + (long)l * B_img * H, l == num_layers - 1 ? Hs : stack.h_live(l)));
        SAT_TRY(gather(img_c + (long)l * B_img * H, row_c + (long)l * R * H));
    }
    hipLaunchKernelGGL(score_step_inputs_kernel, dim3(R), dim3(256), 0, s, embed, captions, (long)cap_stride, C, row_caption, 0, R, E / 4, V,
                       (float*)nullptr, targets);
    SAT_LAUNCH_CHECK();
    // steps t >= 1: the live rows are a prefix (captions ordered by length, descending); the top layer reads its previous h from
    // Hs's rows of step t - 1 and writes step t's rows there
    long p0 = 0;
    for (int t = 1; t < T; ++t) {
        const int rows = batch_sizes[t];
        const long p1 = p0 + batch_sizes[t - 1];
        hipLaunchKernelGGL(score_step_inputs_kernel, dim3(rows), dim3(256), 0, s, embed, captions, (long)cap_stride, C, row_caption, t, rows,
                           E / 4, V, x, targets + p1);
        SAT_LAUNCH_CHECK();
        SAT_TRY(stack.step(x, rows, Hs + p0 * H, Hs + p1 * H));
        p0 = p1;
    }
    const void* packed = nullptr;
    if (logp_fast_shape(H, V)) {
        SAT_TRY(sat_gemm_f32x3_pack(lin_w, V, H, ws + lay.packed, stream));
        packed = ws + lay.packed;
    }
    SAT_TRY(sat_vocab_logp(Hs, H, lin_w, packed, lin_b, targets, N, H, V, tok, nullptr, ws + lay.logp, lay.total - lay.logp, stream));
    return sat_caption_logp_sum(tok, prefix, T, R, logp, len, tok_out, tok_stride, stream);
}
