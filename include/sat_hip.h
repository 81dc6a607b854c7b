/*
 * sat_hip.h -- C ABI of libsat_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the Show-and-Tell
 * training hot path of incredible-vision/show-and-tell.
 *
 * The reference has NO native code and NO FFI: its hot path is a chain of torch operator
 * call sites.  Each entry point below replaces the call site cited next to it, so a maintainer can bind
 * it from Python with ctypes.  Conventions:
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless marked [host];
 *   - the caller owns every buffer (inputs, outputs, tapes, workspaces): nothing here allocates or frees;
 *   - every launch goes to `stream` (a hipStream_t); no host synchronisation, safe to capture in a hipGraph;
 *   - return 0 on success, SAT_ERR_* (>= 1001) for argument errors, otherwise a hipError_t value;
 *   - packed sequences are TIME-MAJOR: rows of step t are [prefix[t], prefix[t]+batch_sizes[t]),
 *     batch_sizes non-increasing (pack_padded_sequence with lengths sorted descending, models.py:51).
 */
#ifndef SAT_HIP_H
#define SAT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAT_ABI_VERSION 18

#define SAT_OK 0
#define SAT_ERR_ARG 1001
#define SAT_ERR_WORKSPACE 1002
#define SAT_ERR_UNSUPPORTED 1003

#define SAT_F32 0
#define SAT_BF16 1

typedef void* sat_stream_t; /* hipStream_t */

int sat_version(void);
const char* sat_error_string(int code);

/* ------------------------------------------------------------------------------------------------
 * Generic dense f32 GEMM on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32): C[M,N] = op(A) op(B) + bias + bias2
 *   amode 0: A[m*lda + k]          amode 2: A[k*lda + m]
 *   bmode 0: B[n*ldb + k]  ("NT")  bmode 1: B[k*ldb + n]
 * Replaces the cuBLAS/MKL GEMMs under nn.Linear / nn.LSTM (models.py:52-53) and their backward.
 * Requires K%4==0, lda/ldb%4==0 (+ M%4 for amode 2, N%4 for bmode 1), 16-byte aligned bases.
 */
int sat_gemm_f32(int amode, int bmode, const float* A, int64_t lda, const float* B, int64_t ldb,
                 float* C, int64_t ldc, const float* bias, const float* bias2,
                 int M, int N, int K, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Encoder op program (models.py:25-29 `self.resnet(images)`): the host describes the frozen conv stack
 * as an array of sat_op and one call launches all of it.  Activations are NHWC, dtype f32 or bf16.
 */
enum {
    SAT_OP_IMAGE_PREP = 1, /* NCHW f32 image -> zero-padded NHWC4 (in0 -> out); H/W = Hin/Win, pad = border; Cout = 8 (bf16):
                            * NHWC8 instead, one 16-byte chunk per pixel (3x3 stems: VGG conv1_1, model2.py:15) */
    SAT_OP_CONV = 2,       /* implicit-GEMM conv: in0 (NHWC) * w [Cout][KH*KW*Cin] -> out [M][Cout] (+ stat_partial) */
    SAT_OP_BN_FINALIZE = 3,/* partials -> scale/shift (+ running stats update); with stat_acc set ("acc mode"):
                            * partials -> the fixed-point integer accumulators stat_acc (parity half), consumers derive */
    SAT_OP_BN_RELU = 4,    /* out = relu(in0*scale0 + shift0) */
    SAT_OP_BN_ADD_RELU = 5,/* out = relu(in0*scale0+shift0 + (in1*scale1+shift1 | in1)) */
    SAT_OP_BN_RELU_MAXPOOL = 6, /* out = maxpool3x3/2(relu(in0*scale0+shift0)) */
    SAT_OP_AVGPOOL = 7,    /* out f32 [N][C] = mean over Hin*Win of in0 */
    SAT_OP_MAXPOOL3S2 = 10,/* out = maxpool 3x3 / stride 2 / no padding of in0 (NHWC, Cout channels; ldc = output row pitch) */
    SAT_OP_AVGPOOL3 = 11,  /* out = avgpool 3x3 / stride 1 / pad 1, count_include_pad (divide by 9) of in0 (NHWC, Cout channels) */
    SAT_OP_MAXPOOL2 = 9,   /* out = maxpool 2x2 / stride 2 of in0 (NHWC; Hin, Win even; Cout channels): VGG16, model2.py:15-16 */
    SAT_OP_BN_EVAL_BATCH = 8,/* eval mode: in0 = DEVICE array of `count` sat_bn_eval_item; every item's (scale, shift)
                              * from its running statistics in ONE launch (replaces one BN_FINALIZE per layer); eps */
    /* Train-mode bn3 of a bottleneck WITHOUT a pass over conv3's output (models.py:27, BatchNorm2d with batch statistics): mean and
     * variance of c3 = a2 W3^T are a linear / quadratic form of conv3's INPUT a2 = relu(bn2(c2)): mean_c = w_c . mu,
     * var_c = w_c^T (G / M - mu mu^T) w_c with G = a2^T a2 (P x P, P = planes).  Four ops in front of conv3, which then runs with
     * the inference epilogue (scale1 / shift1 = the table, in1 = the residual, flags bit 0 = ReLU; SAT_CONV_GROUP_TABLE when grouped):
     * the raw conv3 tensor and the SAT_OP_BN_ADD_RELU launch (42 % of the stack's memory traffic in round 4) never exist.
     * bf16 only; P in {128, 256, 384, 512}.  All honour `groups`. */
    SAT_OP_GRAM = 12,        /* in0 = raw conv2 output [G][M = N*Hout*Wout][P = Cout]; its BatchNorm + ReLU as on a conv's fused input
                              * (stat_acc1 / gamma1 / beta1 / count / eps, or scale0 / shift0): read only, nothing cleared or updated;
                              * out = f32 slabs [G][sat_gram_slab_floats(M, P)]: per row slab the partial 128 x 128 tiles of G (upper
                              * triangle of tile pairs) and the P column sums, f32 MFMA accumulate */
    SAT_OP_GRAM_COV = 13,    /* in0 = those slabs (same N / Hout / Wout / Cout); slabs summed in slab order in f64, cov = G / M - mu mu^T
                              * rounded to f32 and split exactly into three bf16 terms: out = bf16 [G][3][P][P]; scale_out = mu as
                              * DOUBLE [G][P] */
    SAT_OP_GEMM_BF16_NT = 14,/* out f32 [M = N*Hout*Wout][Cout] = in0 bf16 [M][K = Cin] x w bf16 [Cout][K]^T (sat_gemm_bf16_nt); here:
                              * T [G * 3 P][Cout] = cov3 x conv3's weight matrix */
    SAT_OP_BN_FROM_GRAM = 15 /* in0 = T f32 [G][3 P][Cout], w = conv3's weights bf16 [Cout][P = Cin], in1 = mu f64 [G][P]; gamma / beta /
                              * running_mean / running_var / momentum / eps / count (= M) of bn3: var_c = sum_i w[c][i] (T0+T1+T2)[i][c],
                              * mean_c = w_c . mu in f64 -> scale_out = f32 table [G][2][Cout] (scale row, shift row); running statistics
                              * updated in place (grouped: the deferred log [G][2][Cout]) */
};

/* one BatchNorm of an eval-mode stack (all pointers device memory, C floats each) */
typedef struct sat_bn_eval_item {
    const float* gamma;
    const float* beta;
    const float* running_mean;
    const float* running_var;
    float* scale_out;
    float* shift_out;
    int32_t C;
    int32_t reserved;
} sat_bn_eval_item;

/* one BatchNorm of a train-mode stack whose running-statistics update was deferred (sat_bn_running_apply) */
typedef struct sat_bn_running_item {
    float* running_mean;          /* the model's buffers (models.py:14 resnet152 BatchNorm2d), C floats */
    float* running_var;
    const float* batch_mean;      /* this batch's mean / unbiased variance as the program left them (f32) */
    const float* batch_var;
    int32_t C;
    int32_t reserved;
} sat_bn_running_item;

typedef struct sat_op {
    int32_t kind;
    int32_t dtype;            /* SAT_F32 / SAT_BF16 : element type of in0/in1/out/w */
    const void* in0;
    const void* in1;
    void* out;
    const void* w;
    const float* scale0;
    const float* shift0;
    const float* scale1;      /* NULL => in1 used as is */
    const float* shift1;
    float* stat_partial;      /* [tiles_m][2][Cout] f32 : per-tile column sum / sum of squares */
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* scale_out;
    float* shift_out;
    int32_t N, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad;
    int32_t training;         /* BN_FINALIZE: 1 = batch statistics (+running update), 0 = running statistics */
    int32_t tiles_m;          /* number of partial rows in stat_partial (= ceil(M/128)) */
    int64_t sN, sH, sW;       /* element strides of in0 for SAT_OP_CONV (lets the stem read a padded NHWC4 image) */
    int64_t count;            /* BN_FINALIZE: elements per channel (N*Hout*Wout) */
    float momentum, eps;
    int32_t variant;          /* SAT_OP_CONV: 0 = built-in heuristic, >0 = kernel variant chosen by sat_conv_autotune; < 0 on entry to
                               * sat_conv_autotune: choose among the variants of statistics signature -variant only */
    int32_t flags;            /* SAT_OP_CONV, bf16, inference: scale1/shift1 [Cout] set => the epilogue writes
                               * out = acc*scale1[n] + shift1[n] (+ in1[m][n], a residual shaped like out) and, with
                               * bit 0 of flags, ReLU -- BatchNorm (eval) + add + ReLU of a bottleneck without a
                               * separate launch (models.py:27 under eval.py:65 `model.eval()`) */
    /* Integer-atomic BatchNorm statistics (bf16, training, few M-tiles): stat_acc = int64 [2 step parities][2][C]
     * fixed-point (2^22) column sums, zero before first use.  On a SAT_OP_CONV the kernel ADDS this tile's sums into
     * parity p's half; on the consuming SAT_OP_BN_RELU / SAT_OP_BN_ADD_RELU (same pointer, plus gamma, beta, running_mean, running_var,
     * count, momentum, eps) every workgroup derives scale/shift from them, workgroup 0 updates the running statistics
     * and clears parity 1-p's half: no SAT_OP_BN_FINALIZE launch.  p is sat_run_ops_parity's argument and must
     * alternate between consecutive runs of the program.  The *1 fields describe in1's BatchNorm (BN_ADD_RELU). */
    void* stat_acc;
    void* stat_acc1;
    const float* gamma1;
    const float* beta1;
    float* running_mean1;
    float* running_var1;
    const void* w_packed;     /* SAT_OP_CONV, bf16, Cin % 64 == 0, Cout % 128 == 0, 3x3 / stride 1 / pad 1 or 1x1 / pad 0: the weights once more in
                               * MFMA fragment order (sat_conv_pack_weights) -- lets the tuner pick conv_pw_kernel (3x3) / conv_aw_kernel
                               * (1x1), which stream them straight into registers; NULL = not provided */
    int32_t reserved1[2];     /* (were stat_shards / stat_shards1: sharded accumulators, removed in ABI 13 -- a measured wash) */
    /* SAT_OP_CONV extras for Inception-style stacks (BASELINE configs[3]): flags bit 1 (SAT_CONV_PADW) = the padding differs per
     * axis: `pad` is the vertical one, pad_w the horizontal one (1x7 / 7x1 / 1x3 / 3x1 kernels); ldc = row pitch of `out` in
     * elements (0 = Cout): a conv / activation may write its channels into a slice of a wider (concatenated) NHWC tensor.
     * SAT_OP_BN_RELU honours ldc the same way for its output. */
    int32_t pad_w;
    /* GROUPED program (bf16, training): groups = G > 1 runs G independent BATCHES in every launch of the op (grid.y = group) --
     * the frozen conv stack of G look-ahead batches as ONE program, half (1/G) the launch boundaries and twice (G x) the
     * workgroups per launch.  N stays the batch of ONE group; every per-batch buffer is G consecutive copies of the ungrouped
     * one: in0 / in1 / out [G][N][H][W][C] (out: G x N*Hout*Wout rows of pitch ldc), stat_partial [G][tiles_m][2][Cout],
     * stat_acc / stat_acc1 [G][2 parities][2][C], running_mean / running_var of a DEFERRED program (sat_bn_running_apply)
     * [G][2][C] (mean row, then variance row: running_var == running_mean + C).  Weights, gamma / beta are shared.  Each group
     * keeps its own batch statistics and is, instruction for instruction, the ungrouped launch on its batch.  Honoured by
     * SAT_OP_CONV, SAT_OP_BN_FINALIZE (acc mode), SAT_OP_BN_RELU, SAT_OP_BN_ADD_RELU, SAT_OP_BN_RELU_MAXPOOL; SAT_OP_IMAGE_PREP
     * and SAT_OP_AVGPOOL are per image: give them N = G * batch.  0 / 1 = ungrouped. */
    int32_t groups;
    int64_t ldc;
    /* SAT_OP_CONV with flags bit 3 (SAT_CONV_IN_RESIDUAL; bf16, 1x1 / stride 1 on a dense NHWC tensor, w_packed, Cin a multiple of 128
     * in [256, 2048], Cout of 128): this conv ALSO finishes the bottleneck in front of it.  Its operand is
     *     y = relu(bn(in0) + in1)        (bn = the input BatchNorm of scale0 / shift0 or stat_acc1 / gamma1 / ...; in1 shaped like in0)
     * built on its way to LDS -- bit for bit what SAT_OP_BN_ADD_RELU writes -- and y is written to out1 (shaped like in0, per group like
     * in0) as well: the normalise + add + ReLU launch between conv3 of one bottleneck and conv1 of the next disappears
     * (models.py:27, train-mode BatchNorm).  out1 may alias in0 when Cout == 128 (or == 256 and the eight-wave variant runs it: the
     * library checks); it must not alias in1. */
    void* out1;
} sat_op;
#define SAT_CONV_PADW 2
#define SAT_CONV_IN_RESIDUAL 8
#define SAT_CONV_GROUP_TABLE 4   /* SAT_OP_CONV flags: scale1 / shift1 are PER GROUP, [G][2][Cout] apart (the table SAT_OP_BN_FROM_GRAM writes), and
                                  * in1 (the residual) is per group like `out`: lets a grouped train-mode program run conv3 with the
                                  * inference epilogue */
/* slab geometry of SAT_OP_GRAM: rows per slab and slab count are functions of (M, P) only -- never of `groups` -- so a batch's
 * statistics are summed in the same order in the grouped and the ungrouped program; floats of ONE group's slab buffer */
int sat_gram_rows_per_slab(int64_t M, int P);
int sat_gram_slabs(int64_t M, int P);
int64_t sat_gram_slab_floats(int64_t M, int P);
int sat_run_ops(const sat_op* ops /*[host]*/, int n_ops, sat_stream_t stream);
/* same, with the step parity (0/1) that selects the half of every stat_acc buffer in use */
/* Deferred running statistics.  A program built with its sat_op running_mean / running_var pointers aimed at PRIVATE, zeroed
 * buffers and momentum 1 leaves each layer's batch (mean, unbiased variance) there and touches no model state, so two batches'
 * frozen conv stacks may be in flight at once (TrainStep.prefetch_encoder).  This applies one finished batch to the model:
 * running = (1-momentum)*running + momentum*batch for every item, one launch, bit-identical to the in-kernel update.  The
 * caller orders the calls like the batches (nn.BatchNorm2d momentum update, train.py:128 `encoder.train()`). */
int sat_bn_running_apply(const sat_bn_running_item* items /*[device]*/, int n_items, float momentum, sat_stream_t stream);
/* counters[i] += value for n int64 counters [device]: `num_batches_tracked += 1` of every BatchNorm of a stack in one launch
 * (nn.BatchNorm2d / BatchNorm1d forward in training mode, models.py:27-28 under train.py:128 `encoder.train()`). */
int sat_counter_add(int64_t* counters /*[device]*/, int n, int64_t value, sat_stream_t stream);
int sat_run_ops_parity(const sat_op* ops /*[host]*/, int n_ops, int parity, sat_stream_t stream);
/* The same program as ONE hipGraph launch (the reference's `self.resnet(images)` issues ~1500 eager kernels per
 * forward, models.py:27; here the host enqueues one graph).  sat_graph_create records ops[0..n) for the given step
 * parity on an internal capture stream (nothing executes) and instantiates it; all pointers and shapes in ops[] are
 * frozen into the graph.  sat_graph_launch replays it on `stream`; sat_graph_destroy frees it.  No host sync. */
typedef struct sat_graph sat_graph;
int sat_graph_create(const sat_op* ops /*[host]*/, int n_ops, int parity, sat_graph** graph_out);
int sat_graph_launch(sat_graph* graph, sat_stream_t stream);
int sat_graph_destroy(sat_graph* graph);
/* conv -> train-mode BatchNorm -> ReLU of one bottleneck stage (models.py:27) as one call over three op records:
 * conv (statistics in its epilogue), finalize (scale/shift + running statistics), bnrelu (in0 must be conv->out) */
int sat_conv_bn_relu_fwd(const sat_op* conv, const sat_op* finalize, const sat_op* bnrelu, sat_stream_t stream);
/* rows of SAT_OP_CONV partials the conv kernel writes for M output pixels */
int sat_conv_tiles_m(int64_t M);
/* Build-time tuner (NOT for the hot path: it times launches with HIP events and synchronises): for every bf16
 * SAT_OP_CONV in ops[] run each kernel variant `reps` times on the op's own buffers and record the fastest in
 * ops[i].variant.  Results are cached per conv geometry inside the library (mutex-protected).  `scratch`: >= 16384
 * bytes of device memory owned by the caller (a neutral BatchNorm table for the input-fused convs lives there while
 * the tuner runs): like every other entry point, this one allocates no device memory. */
int sat_conv_autotune(sat_op* ops /*[host]*/, int n_ops, int reps, float* scratch, int64_t scratch_bytes,
                      sat_stream_t stream);
/* The same, and in cand[n_ops][topk] [host] the `topk` fastest variants of every op (1-based, fastest first, 0 = no more; all 0
 * for ops the tuner does not handle).  A replayed launch finds its operand warm, a launch inside the program does not, and the two
 * rankings differ by a few microseconds either way: a caller that can time its whole program (sat_run_ops_timed) makes the final
 * choice among the candidates IN the program (resnet.ConvStackProgram._autotune). */
int sat_conv_autotune_topk(sat_op* ops /*[host]*/, int n_ops, int reps, float* scratch, int64_t scratch_bytes,
                           sat_stream_t stream, int topk, int32_t* cand /*[host]*/);
/* What fixes the BITS of the BatchNorm column sums a kernel variant (sat_op.variant, 1-based) leaves: two variants with the
 * same signature give bit-identical statistics (the conv output is bit-identical across the ring variants anyway).  A caller
 * that runs one model through several programs (ungrouped, grouped look-ahead copies) lets its FIRST program tune freely, reads
 * the signatures of the variants it got, and hands them to the tuner for every other program (sat_op.variant = -signature on
 * entry to sat_conv_autotune): every batch then gets, bit for bit, the same statistics whichever program runs it.  -1: no such
 * variant. */
int sat_conv_variant_signature(int variant);
/* The same for the conv OUTPUT alone (inference programs: no statistics): 100000 + the order in which the variant walks the K axis
 * (0: tap major -- ring, expansion and stem kernels; 1: channel-block major -- the two LDS-patch 3x3 kernels).  Outputs are
 * bit-identical within a family; accepted by sat_conv_autotune as a constraint like a statistics signature. */
int sat_conv_variant_family(int variant);
/* Kernel selection WITHOUT timing (the default since ABI 16: the arithmetic of a run must not depend on a stopwatch).  A tuned
 * choice is a variant NUMBER, valid for the build it was measured on: sat_conv_num_variants() stamps a saved table
 * (show-and-tell_amd/tune/gfx950.json).  For a geometry no table names, sat_conv_default_variant gives the variant (1-based) the op
 * runs: the built-in heuristic, or -- want_sig >= 0 (a statistics signature / output family as above) and the heuristic's choice
 * has another one -- the first variant of that signature the op can run; 0 if there is none.  A function of the op's geometry
 * only: every process, rank and box gets the same answer (config.py:15 `random_seed`: same seed, same bits). */
int sat_conv_num_variants(void);
int sat_conv_default_variant(const sat_op* op /*[host]*/, int want_sig);
/* The variant (1-based) sat_run_ops would launch for this bf16 SAT_OP_CONV: op->variant when the op can run it, else the built-in
 * choice (a variant the op cannot run is replaced silently at launch: a caller that depends on WHICH kernel runs -- a test of one
 * kernel, a table of tuned choices -- asks here).  0 when the op is rejected, is not a bf16 conv, or has a Cout that is not a
 * multiple of 8 (the register-staged kernel: no variants).  Host only: reads no device memory, launches nothing. */
int sat_conv_resolved_variant(const sat_op* op /*[host]*/);
/* bf16 weights [Cout][taps][Cin] (the kernels' layout; Cout % 32 == 0, Cin % 64 == 0) -> `packed` (same element count) in the
 * MFMA fragment order conv_pw_kernel streams into registers: [Cout/32][Cin/64][taps][4][64 lanes][8].  Once per weight version
 * of a frozen stack (`self.resnet(images)`, models.py:14-15,27). */
int sat_conv_pack_weights(const void* w, void* packed, int Cout, int Cin, int taps, sat_stream_t stream);
/* Diagnostics, NOT the hot path (creates events, synchronises `stream`): run ops[0..n) once, in order, and return in
 * op_us[i] [host] the duration in microseconds of every bf16 SAT_OP_CONV launch taken from its own dispatch
 * timestamps (what rocprofv3 --kernel-trace reports for that launch); 0 for the other ops.  bench.py uses it for the
 * roofline figure of the dominant kernel. */
int sat_run_ops_timed(const sat_op* ops /*[host]*/, int n_ops, int parity, sat_stream_t stream, float* op_us /*[host]*/);

/* ------------------------------------------------------------------------------------------------
 * Encoder head: resnet.fc (Linear 2048->E) + BatchNorm1d(E, momentum=0.01)  (models.py:16-17,27-28)
 */
int sat_fc_bn1d_fwd(const float* pooled /*[B,F]*/, const float* w_fc /*[E,F]*/, const float* b_fc /*[E]*/,
                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, int training, int B, int F, int E,
                    float* feats /*[B,E]*/, float* xhat /*[B,E]*/, float* rstd /*[E]*/,
                    float* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_fc_bn1d_ws_bytes(int B, int F, int E);
int sat_fc_bn1d_bwd(const float* dy /*[B,E]*/, const float* pooled, const float* xhat, const float* rstd,
                    const float* gamma, int B, int F, int E,
                    float* dw_fc /*[E,F]*/, float* db_fc, float* dgamma, float* dbeta,
                    float* workspace /* >= B*E floats */, int64_t ws_bytes, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Decoder (models.py:47-54).
 */
/* embed + cat(features) + pack (models.py:49-51): X[N,E], row (t,b): t==0 ? features[b] : embed[captions[b][t-1]] */
int sat_embed_concat_fwd(const float* features /*[B,E]*/, const float* embed /*[V,E]*/,
                         const int64_t* captions /*[B][cap_stride]*/, int64_t cap_stride,
                         const int32_t* prefix /*[T+1] device*/, int T, int N /*=prefix[T]*/, int B, int E, int V,
                         float* X /*[N,E]*/, sat_stream_t stream);
/* backward of the above: d_embed (dense, zeroed here, deterministic order) and d_features */
int sat_embed_concat_bwd(const float* dX /*[N,E]*/, const int64_t* captions, int64_t cap_stride,
                         const int32_t* prefix /*device*/, int T, int N, int B, int E, int V,
                         float* d_embed /*[V,E]*/, float* d_features /*[B,E]*/, sat_stream_t stream);

/* Range check of an id matrix ids[rows][row_stride] (first `cols` columns): status[0] |= 1 when any id is outside
 * [lo, hi).  nn.Embedding (models.py:49) and nn.CrossEntropyLoss (train.py:143) raise on such ids; the kernels below
 * clamp them for memory safety only, the host wrappers launch this check on the caption matrix and raise when the
 * status word (device int32, zero-initialised by the caller) comes back set. */
int sat_validate_ids(const int64_t* ids, int64_t row_stride, int rows, int cols, int64_t lo, int64_t hi,
                     int32_t* status, sat_stream_t stream);

/* targets = pack_padded_sequence(captions[:,1:], lengths-1).data (train.py:134-135); prefix/T/N describe lengths-1 */
int sat_pack_targets(const int64_t* captions /*[B][cap_stride]*/, int64_t cap_stride, const int32_t* prefix /*device*/,
                     int T, int N, int64_t* targets /*[N]*/, sat_stream_t stream);

/* one nn.LSTM layer over a packed batch (models.py:52), zero initial state, gate order i,f,g,o.
 * Tapes for the backward: GA[N,4H] post-activation gates, CS[N,H] cell states, HS[N,H] outputs,
 * HP[N,H] previous hidden state per row.  c_state/h_state: [B,H] scratch. */
int sat_lstm_fwd(const float* X /*[N,In]*/, const float* w_ih /*[4H,In]*/, const float* w_hh /*[4H,H]*/,
                 const float* b_ih, const float* b_hh, const int32_t* batch_sizes /*[T] host*/, int T,
                 int In, int H, float* GA, float* CS, float* HS, float* HP, float* c_state,
                 void* workspace, int64_t ws_bytes, sat_stream_t stream);
/* workspace of the persistent recurrence (hidden-state exchange: [2 parities][groups of 8 rows][8][H] self-tagged 4-byte words --
 * bit 30 of |h| <= 1 carries the hand-off phase -- + an error word; the call zeroes it itself).  With it (and H in
 * {32,64,96,128,256,512}, T <= 64, ceil(B/8) * H/16 <= CUs) all T steps run in ONE launch with W_hh register-resident;
 * workspace NULL / too small, or a shape outside that envelope, falls back to one launch per step (same results). */
int64_t sat_lstm_fwd_ws_bytes(int B, int H);
/* Byte offset of the recurrence's STATUS WORD (uint32) in that workspace, or -1 when the shape has no persistent form.
 * sat_lstm_fwd zeroes it; the persistent launch sets it non-zero when a workgroup gave up waiting for its group (every wait
 * is bounded: co-tenants that keep its workgroups from being resident together).  The tapes and HS of such a call are
 * INVALID: the caller must copy the word out behind the call (hipMemcpyAsync to pinned memory) and treat non-zero as an
 * error -- `show-and-tell_amd.watch.ResidencyWatch` raises RuntimeError and switches the process to per-step launches. */
int64_t sat_lstm_fwd_status_offset(int B, int H);
/* Which form of the recurrence a call would run on the current device -- what sat_lstm_fwd / sat_lstm_bwd themselves decide
 * (SAT_LSTM_PERSIST, SAT_LSTM_PERSIST_BWD and sat_lstm_persist_enable included), so a test can prove the form it means to check.
 * fwd: rows per group of the persistent forward given a workspace of sat_lstm_fwd_ws_bytes: 8 or 16, 0 = one launch per step.
 * bwd: 1 = the backward recurrence runs as one persistent launch given the full workspace, 0 = one launch per step. */
int sat_lstm_fwd_plan(int B, int H, int T);
int sat_lstm_bwd_plan(int B, int H, int T);
/* process-wide switch of the persistent recurrence (default on); returns the previous setting.  Off: one launch per step. */
int sat_lstm_persist_enable(int on);
int64_t sat_lstm_bwd_ws_bytes(int B, int H);          /* minimum */
/* size that also lets the batched dW_ih / dX GEMMs run split-K when they would leave most CUs idle (N = packed rows), and the
 * recurrence as ONE persistent launch.  Layout (ABI 16): the granule-exchange region of the persistent recurrence and its status
 * word come FIRST, at offsets that depend on (B, H) only; the N-dependent slabs follow.  So ONE buffer sized with
 * sat_lstm_bwd_ws_bytes_max for the longest batch serves every call (any N <= n_max).  The exchange region is never cleared per
 * call -- granules carry a per-call epoch tag -- and the invariant "no foreign bit pattern in it" is the LIBRARY's: it clears the
 * region the first time it sees the buffer's address (and when its 24-bit epoch counter wraps) and remembers the address; an owner
 * that frees the buffer (or reuses the memory for something else) says so with sat_lstm_ws_release.  The caller zeroes nothing. */
int64_t sat_lstm_bwd_ws_bytes_full(int N, int B, int In, int H);
int64_t sat_lstm_bwd_ws_bytes_max(int n_max, int B, int In, int H);
int sat_lstm_ws_release(void* workspace);
/* With the FULL workspace (and the forward's envelope: H in {32,...,512}, T <= 64, ceil(B/8) * H/16 <= CUs) the backward
 * recurrence runs as ONE persistent launch too (SAT_LSTM_PERSIST_BWD=0: one launch per step).  Its STATUS WORD (uint32) sits at
 * this byte offset of the workspace (a function of B and H only): zeroed by every such call, non-zero when a bounded wait of the
 * persistent launch ran out -- DG and every gradient of that call are then INVALID; read it back behind the call as for
 * sat_lstm_fwd_status_offset. */
int64_t sat_lstm_bwd_status_offset(int N, int B, int In, int H);
int sat_lstm_bwd(const float* dHS /*[N,H]*/, const float* X, const float* w_ih, const float* w_hh,
                 const float* GA, const float* CS, const float* HP,
                 const int32_t* batch_sizes /*[T] host*/, int T, int In, int H,
                 float* DG /*[N,4H] out*/, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                 float* dX /*[N,In] or NULL*/, float* workspace, int64_t ws_bytes, sat_stream_t stream);

/* bf16 THROUGHPUT mode of an LSTM layer's batched GEMMs (BASELINE configs[1] names bf16): sat_lstm_fwd / sat_lstm_bwd with the
 * x-gates product and dW_ih / dW_hh / dX on v_mfma_f32_32x32x16_bf16 (f32 accumulate and outputs) from bf16 copies of the f32
 * operands made in `mixed_ws` (sat_lstm_mixed_ws_bytes, 256-byte aligned); the recurrence, the gate arithmetic, the bias
 * gradients and the master weights stay f32.  A too small mixed_ws silently keeps the exact-f32 GEMMs. */
int64_t sat_lstm_mixed_ws_bytes(int N /*packed rows*/, int In, int H);
int sat_lstm_fwd_bf16(const float* X, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                      const int32_t* batch_sizes /*[T] host*/, int T, int In, int H, float* GA, float* CS, float* HS, float* HP,
                      float* c_state, void* workspace, int64_t ws_bytes, void* mixed_ws, int64_t mixed_bytes, sat_stream_t stream);
int sat_lstm_bwd_bf16(const float* dHS, const float* X, const float* w_ih, const float* w_hh, const float* GA, const float* CS,
                      const float* HP, const int32_t* batch_sizes /*[T] host*/, int T, int In, int H, float* DG, float* dw_ih,
                      float* dw_hh, float* db_ih, float* db_hh, float* dX, float* workspace, int64_t ws_bytes, void* mixed_ws,
                      int64_t mixed_bytes, sat_stream_t stream);

/* vocab projection (models.py:53) */
/* logits rows have stride ldl >= V floats.  For the backward (sat_vocab_ce_bwd) ldl must be a multiple of 4 and the
 * pad columns [V, ldl) must hold zeros (allocate the buffer zero-filled: no kernel here writes the pad). */
int sat_vocab_logits_fwd(const float* Hs /*[N,H]*/, const float* w /*[V,H]*/, const float* b /*[V]*/,
                         int N, int H, int V, float* logits /*[N,ldl]*/, int64_t ldl, sat_stream_t stream);
/* row-wise softmax cross entropy (train.py:53,143): row_loss[n] = lse - logit[target]; loss_out[0] =
 * inv_denom * sum(row_loss) (fixed-order reduction).  write_grad: logits are overwritten IN PLACE with
 * d(loss)/d(logits) = (softmax - onehot) * inv_denom. */
int sat_ce_rows(float* logits /*[N,ldl]*/, int64_t ldl, const int64_t* targets /*[N]*/, int N, int V, float inv_denom,
                int write_grad, float* row_loss /*[N]*/, float* loss_out /*[1]*/, sat_stream_t stream);
/* ---- bf16 THROUGHPUT mode of the vocab projection and its backward (models.py:53, train.py:143-144; BASELINE configs[1]
 * names bf16): the three GEMMs run on v_mfma_f32_32x32x16_bf16 with f32 accumulate from bf16 COPIES of Hs / W / d(logits)
 * made per step inside `workspace`; logits, CE arithmetic, bias gradient, all outputs and the master weights stay f32.
 * d(loss)/d(logits) exists only as bf16, in the workspace, between the two calls.  Needs H % 64 == 0, V % 4 == 0,
 * V <= 12288 (SAT_ERR_UNSUPPORTED otherwise: use sat_vocab_logits_fwd / sat_ce_rows / sat_vocab_ce_bwd).
 * sat_vocab_ce_fwd_bf16: logits[N,ldl] = Hs W^T + b; row_loss[n] = lse - logit[target]; loss_out[0] = inv_denom * sum.
 * sat_vocab_ce_bwd_bf16: dw[V,H] = G^T Hs, db[V] = colsum(G), dHs[N,H] = G W with G = (softmax - onehot) * inv_denom. */
int64_t sat_vocab_bf16_ws_bytes(int N, int H, int V);     /* 0: shape unsupported */
int sat_vocab_ce_fwd_bf16(const float* Hs /*[N,H]*/, const float* w /*[V,H]*/, const float* b /*[V]*/, const int64_t* targets /*[N]*/,
                          int N, int H, int V, float inv_denom, float* logits /*[N,ldl]*/, int64_t ldl, float* row_loss /*[N]*/,
                          float* loss_out /*[1] or NULL*/, void* workspace /*256-byte aligned*/, int64_t ws_bytes, sat_stream_t stream);
int sat_vocab_ce_bwd_bf16(int N, int H, int V, float* dw /*[V,H]*/, float* db /*[V]*/, float* dHs /*[N,H]*/, void* workspace,
                          int64_t ws_bytes, sat_stream_t stream);
/* the kernel under them: C[M,N] f32 = A[M,K] B[N,K]^T (+ bias[N]); A, B bf16 with K contiguous, K % 64 == 0 (zero padded),
 * N % 4 == 0, lda / ldb % 8 == 0.  ksplit > 1: K slice z writes C + z * slab_stride, no bias (sum with sat_sum_slabs_f32). */
int sat_gemm_bf16_nt(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                     int M, int N, int K, int ksplit, int64_t slab_stride, sat_stream_t stream);
/* out bf16 [C][ldo] = in^T for in f32 [R][ldi]; columns [R, ldo) zero (ldo % 4 == 0) */
int sat_transpose_f32_bf16(const float* in, int64_t ldi, int R, int C, void* out, int64_t ldo, sat_stream_t stream);
/* Vocab projection + cross entropy (models.py:53 + train.py:53,143) as ONE call, exact f32: logits = Hs w^T + b, then
 * row_loss[n] = logsumexp(logits[n]) - logits[n][targets[n]], loss_out[0] = inv_denom * sum(row_loss), and the logits are
 * overwritten IN PLACE with d(loss)/d(logits) = (softmax - onehot) * inv_denom, ready for sat_vocab_ce_bwd (= sat_vocab_logits_fwd
 * followed by sat_ce_rows with write_grad).  ldl >= V; pad columns [V, ldl) are left alone (zero-fill once when ldl > V). */
int sat_vocab_ce_fwd(const float* Hs /*[N,H]*/, const float* w /*[V,H]*/, const float* b /*[V]*/, const int64_t* targets /*[N]*/,
                     int N, int H, int V, float inv_denom, float* logits /*[N,ldl]*/, int64_t ldl,
                     float* row_loss /*[N]*/, float* loss_out /*[1]*/, sat_stream_t stream);
/* backward of the projection given dlogits: dW[V,H], db[V], dHs[N,H] */
int sat_vocab_ce_bwd(const float* dlogits /*[N,ldl]*/, int64_t ldl, const float* Hs, const float* w, int N, int H, int V,
                     float* dw, float* db, float* dHs, float* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_vocab_ce_bwd_ws_bytes(int N, int H, int V);
/* f32 GEMM on the bf16 matrix pipe by a three-way bf16 split of both operands (hi + mid + lo, six products, hi*hi and the corrections
 * in separate f32 accumulators): the accuracy of an f32 GEMM -- not its bit pattern -- at 6 / 16 of the f32 pipe's cost.  For weights
 * that stay fixed over many calls (the vocab projection of the beam decode loop, models.py:53 / :63): sat_gemm_f32x3_pack splits W
 * [N][K] f32 once into its fragment-ordered copy (sat_gemm_f32x3_packed_bytes(N, K) bytes; 0 = shape not supported: K % 128 == 0,
 * K >= 256), sat_gemm_f32x3 computes C[M][ldc] = A[M][lda] * W^T + bias (N % 4 == 0, lda % 4 == 0, ldc % 4 == 0). */
int64_t sat_gemm_f32x3_packed_bytes(int N, int K);
int sat_gemm_f32x3_pack(const float* W, int N, int K, void* packed, sat_stream_t stream);
int sat_gemm_f32x3(const float* A, int64_t lda, const void* packed, const float* bias, float* C, int64_t ldc, int M, int N, int K,
                   sat_stream_t stream);

/* split-K variant of sat_gemm_f32: K-steps dealt to ksplit slices, slice z writes C + z*slab_stride (bias in slice 0);
 * sat_sum_slabs_f32 adds the slices in fixed order. */
int sat_gemm_f32_splitk(int amode, int bmode, const float* A, int64_t lda, const float* B, int64_t ldb,
                        float* C, int64_t ldc, const float* bias, const float* bias2, int M, int N, int K,
                        int ksplit, int64_t slab_stride, sat_stream_t stream);
int sat_sum_slabs_f32(const float* in, int nslab, int64_t slab_stride, int64_t n, float* out, sat_stream_t stream);
/* out[M,N] = A[M,K] * op(W) + bias for FEW rows (a decode / recurrence step: M <= a few hundred): K is split over the waves of
 * a workgroup and over grid slices so that 64 rows still fill the chip (the per-step GEMMs of model2.py:54-62 and their
 * backward).  w_kmajor 0: W[n*ldw + k]; 1: W[k*ldw + n].  K % 4 == 0, lda % 4 == 0.  Exact f32 (v_mfma_f32_16x16x4_f32). */
int sat_skinny_gemm_f32(const float* A, int64_t lda, const float* W, int64_t ldw, int w_kmajor, int M, int N, int K,
                        const float* bias, float* out, int64_t ldo, float* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_skinny_gemm_ws_bytes(int M, int N, int K);
/* ... with an optional second product into the same output: out = A W + A2 W2 + bias (both W in the layout w_kmajor names);
 * workspace as for (M, N, K). */
int sat_skinny_gemm2_f32(const float* A, int64_t lda, const float* W, int64_t ldw, int K, const float* A2, int64_t lda2,
                         const float* W2, int64_t ldw2, int K2, int w_kmajor, int M, int N, const float* bias, float* out,
                         int64_t ldo, float* workspace, int64_t ws_bytes, sat_stream_t stream);
/* greedy argmax of one decode step (models.py:61-63): ids[b*ids_stride] = first argmax_v (h[b] . w[v] + b[v]) */
int sat_vocab_argmax(const float* h /*[B,H]*/, const float* w, const float* b, int B, int H, int V,
                     int64_t* ids, int64_t ids_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_vocab_argmax_ws_bytes(int B, int V);
/* one greedy decode step of one LSTM layer, state in place: x[B,In] -> h_out[B,H]; c[B,H] updated */
int sat_lstm_step(const float* x, const float* h_in, float* c, const float* w_ih, const float* w_hh,
                  const float* b_ih, const float* b_hh, int B, int In, int H, float* h_out, sat_stream_t stream);
/* rows of an embedding table: out[b] = embed[ids[b*ids_stride]] */
int sat_embed_rows(const float* embed, const int64_t* ids, int64_t ids_stride, int B, int E, int V,
                   float* out, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Show-Attend-Tell decoder (model2.py:38-111: the model train.py:37 constructs).  f32, rows = batch rows of one step.
 * sat_attention_fwd: `attention_layer` (model2.py:73-78) for `rows` batch rows:
 *   h_att = tanh(ctx_enc[b] + proj[b][None,:]); alpha[b] = softmax_p(h_att . w_att); context[b] = mean_p(alpha[b,p] feats[b,p,:])
 *   ctx_enc, feats: [rows][P][C] (context_encode / features, model2.py:45-46); proj = weight_hh(hidden) [rows][ld_proj];
 *   alpha [rows][P] (nullable); context [rows][ld_ctx] (ld_ctx lets it land inside the LSTMCell input row).
 * sat_attention_bwd: its backward given d_context (h_att recomputed): d_ctx_enc[rows][P][C] += ..., d_proj [rows][C],
 *   d_watt_part [rows][C] (sum over rows = d weight_att; kept per row for a fixed-order reduction); d_feats (fine-tuning only):
 *   the gradient the weighted mean sends back into the features, accumulated.
 *   Both run as two launches (a per-position row-dot over (rows x position chunks) workgroups, then a per-channel pass over
 *   (rows x C/64) workgroups) so that a 64-row step fills the chip; the workspace carries the P-long vector between them.
 * sat_lstmcell_fwd: one nn.LSTMCell step (model2.py:58), c in place, optional tapes (activated gates, new c).
 * sat_rows_copy: out[r] = in[idx ? idx[r*idx_stride] : r] (embedding rows into a strided destination, state slices).
 * sat_rows_sum: out[c] (+)= sum_r in[r][c] in fixed order.
 */
int sat_attention_fwd(const float* ctx_enc, const float* feats, const float* proj, int64_t ld_proj, const float* w_att,
                      int rows, int P, int C, float* alpha, float* context, int64_t ld_ctx, float* workspace, int64_t ws_bytes,
                      sat_stream_t stream);
int64_t sat_attention_ws_bytes(int rows, int P);     /* raw scores (forward) / d_alpha (backward) between the two launches */
int sat_attention_bwd(const float* ctx_enc, const float* feats, const float* proj, int64_t ld_proj, const float* w_att,
                      const float* alpha, const float* d_ctx, int64_t ld_dctx,
                      const float* d_ctx2 /* nullable: d_context = d_ctx + d_ctx2 (its two consumers, model2.py:58 and :82) */,
                      int64_t ld_dctx2, int rows, int P, int C,
                      float* d_ctx_enc, float* d_proj, float* d_watt_part, float* d_feats /*[rows][P][C] += , or NULL*/,
                      float* workspace, int64_t ws_bytes, sat_stream_t stream);
/* Doubly stochastic attention (Xu et al. 2015, section 4.2.1; added within ABI 18).  The training forward leaves the packed tape
 * alpha [N][P] (rows time-major: step t holds images 0 .. prefix[t+1]-prefix[t]-1 at rows prefix[t] ..).
 * sat_attention_coverage: cov[b][p] = sum over the steps t image b is alive in (b < prefix[t+1] - prefix[t]), ascending t, of
 *   alpha[prefix[t] + b][p]   (cov nullable);   grad[b][p] = 2 coef (cov[b][p] - 1)   [B][P];
 *   penalty[0] = coef * sum_b sum_p (cov[b][p] - 1)^2, per-wave partials in the workspace added in index order (no atomics: the
 *   same input gives the same bits).  prefix: DEVICE int32 [T+1], as for sat_pack_tokens.  Any P >= 1; B <= 65535.  Two launches.
 * sat_attention_bwd_ex: sat_attention_bwd whose row-dot launch writes
 *   d_alpha[b][p] = feats[b,p,:] . d_ctx[b,:] / P + d_alpha_scale[0] * d_alpha_extra[b][p]
 *   d_alpha_extra [rows][ld_extra] (ld_extra >= P); d_alpha_scale: DEVICE pointer to one float (the upstream gradient of the penalty
 *   inside a backward pass: no host read).  Both NULL: exactly sat_attention_bwd, same kernels, same bits; one NULL: SAT_ERR_ARG.
 *   Row index = image index within a step, so the grad [B][P] of sat_attention_coverage serves every step (rows = batch_sizes[t]).
 */
int64_t sat_attention_coverage_ws_bytes(int B, int P);
int sat_attention_coverage(const float* alpha /*[N][P]*/, const int32_t* prefix /*device [T+1]*/, int T, int B, int P, float coef,
                           float* cov /*[B][P] or NULL*/, float* grad /*[B][P]*/, float* penalty /*[1]*/, float* workspace,
                           int64_t ws_bytes, sat_stream_t stream);
int sat_attention_bwd_ex(const float* ctx_enc, const float* feats, const float* proj, int64_t ld_proj, const float* w_att,
                         const float* alpha, const float* d_ctx, int64_t ld_dctx, const float* d_ctx2, int64_t ld_dctx2,
                         const float* d_alpha_extra /*[rows][ld_extra] or NULL*/, int64_t ld_extra,
                         const float* d_alpha_scale /*device [1] or NULL*/, int rows, int P, int C,
                         float* d_ctx_enc, float* d_proj, float* d_watt_part, float* d_feats /*[rows][P][C] += , or NULL*/,
                         float* workspace, int64_t ws_bytes, sat_stream_t stream);
int sat_lstmcell_fwd(const float* x /*[B,In]*/, const float* h_in /*[B,H]*/, float* c /*[B,H] in place*/, const float* w_ih,
                     const float* w_hh, const float* b_ih, const float* b_hh, int B, int In, int H, float* h_out,
                     float* gates /*[B,4H] or NULL*/, float* c_tape /*[B,H] or NULL*/, sat_stream_t stream);
int sat_rows_copy(const float* in, int64_t ldi, const int64_t* idx, int64_t idx_stride, int64_t nrows_in, int rows, int cols,
                  float* out, int64_t ldo, sat_stream_t stream);
int sat_rows_sum(const float* in, int64_t ld, int rows, int cols, float* out, int accumulate, sat_stream_t stream);
/* out[r] = a[r] + b[r] over `cols` columns of strided rows */
int sat_rows_add(const float* a, int64_t lda, const float* b, int64_t ldb, int rows, int cols, float* out, int64_t ldo,
                 sat_stream_t stream);
/* packed token ids out[row(t,b)] = captions[b][t + col0] (prefix/T/N as for sat_pack_targets: the embedding rows a step uses) */
int sat_pack_tokens(const int64_t* captions, int64_t cap_stride, const int32_t* prefix /*device*/, int T, int N, int col0,
                    int64_t* out, sat_stream_t stream);
/* dense embedding gradient (nn.Embedding, sparse=False; model2.py:28): table[V,E] = 0, then table[ids[n]] += rows[n] with a
 * fixed summation order (first occurrence sums its duplicates in row order) */
int sat_scatter_rows_add(const float* rows /*[N,E]*/, const int64_t* ids /*[N]*/, int N, int E, int V, float* table,
                         sat_stream_t stream);
/* pointwise backward of one nn.LSTMCell step: dh = dh_out (+ dh_carry for rows < n_carry), dc from dc_state (rows < n_carry);
 * DG[n,4H] = d(pre-activation gates); dc_state = d c_prev.  gates/c: the step's tapes; c_prev NULL = zeros. */
int sat_lstmcell_bwd_point(const float* dh_out /*[n,H]*/, const float* dh_carry /*[>=n_carry,H] or NULL*/, int n_carry,
                           const float* gates /*[n,4H]*/, const float* c /*[n,H]*/, const float* c_prev /*[n,H] or NULL*/,
                           float* dc_state /*[n,H]*/, float* DG /*[n,4H]*/, int n, int H, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Conv-stack backward for fine-tuning (model2.py:87-89 `finetune(allow=True)`), f32 NHWC.  A 3x3/s1/p1 conv layer
 * y = relu(conv(x, W) + b) is differentiated with the kernels the forward already has:
 *   dZp = sat_pad_nhwc_f32(dY, mask = y)          zero-bordered d(pre-activation)               [N][H+2][W+2][Cout]
 *   db  = sat_colsum_f32(dZp)                     (the border rows are zeros)
 *   dW[:, kh, kw, :] = dZp^T . shift(Xp, kh, kw)  nine sat_gemm_f32_splitk (amode 2, bmode 1) over the flat padded pixel index:
 *                                                 with BOTH operands in the zero-bordered layout a tap is a constant flat offset
 *   dX  = SAT_OP_CONV(dZp as a pre-padded image, W flipped and transposed)                       (the forward conv kernel)
 * sat_maxpool2_bwd_f32: gradient of SAT_OP_MAXPOOL2 (first maximum in scan order, torch's tie rule).
 * sat_bcast_add_f32: out[b][p][:] += scale * v[b][:] (backward of the mean over positions, model2.py:68).
 */
int sat_pad_nhwc_f32(const float* in, const float* relu_mask_of /*or NULL*/, int N, int H, int W, int C, int pad, float* out,
                     sat_stream_t stream);
int sat_maxpool2_bwd_f32(const float* x, const float* dy, int N, int Hin, int Win, int C, float* dx, sat_stream_t stream);
int sat_bcast_add_f32(const float* v, int B, int P, int C, float scale, float* out, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * On-device collate (data_loader.py:48-62 `collate_fn`): the batch arrives in dataset order -- images
 * [B][3*H*W] f32 and ragged captions (flat ids + offsets[B+1]) already in HBM; `order[r]` [device int32] is the sample that
 * lands in row r (decreasing caption length, ties in dataset order: the host derives it from the host-side lengths, which
 * it needs anyway for the packed-sequence bookkeeping).
 * sat_collate_captions: out[r][t] = t < len(order[r]) ? flat[offsets[order[r]] + t] : 0   (the zero-padded LongTensor)
 * sat_gather_rows_f32:  out row r = in row order[r]                                          (torch.stack in sorted order)
 */
int sat_collate_captions(const int64_t* flat, const int64_t* offsets /*[B+1]*/, const int32_t* order /*[B]*/, int B, int Tmax,
                         int64_t* out /*[B][Tmax]*/, sat_stream_t stream);
int sat_gather_rows_f32(const float* in, const int32_t* order, int rows, int64_t cols, float* out, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * On-device image augmentation (added within ABI 18).
 * main.py:26-36: RandomCrop/CenterCrop + RandomHorizontalFlip + ToTensor + Normalize of B images in one launch.
 * src   uint8 [Bsrc][Hs][Ws][3]  (HWC, RGB: what PIL / numpy decode to)
 * params int32 [B][3] = (top, left, flip) per OUTPUT image   [device]
 * order  int32 [B] or NULL: output image b is made from src image order[b] (NULL: b) -- collate's length sort rides along
 * out   f32 [B][3][Hc][Wc]  (NCHW, what every encoder entry point takes)
 * out[b][c][y][x] = ((float)src[order[b]][top+y][left + (flip ? Wc-1-x : x)][c] / 255.0f - mean[c]) / std[c]
 * evaluated in f32 with correctly rounded divisions, i.e. bit for bit ToTensor().div(255) then sub_(mean).div_(std).
 * The kernel clamps top into [0, Hs-Hc], left into [0, Ws-Wc] and order[b] into [0, Bsrc): a bad parameter never addresses
 * memory outside src (a safety net; callers validate on the host).  No allocation, no host sync, capturable.
 * SAT_ERR_ARG before any launch: src, params, out, mean or std NULL; B, Bsrc, Hc or Wc <= 0; Hc > Hs or Wc > Ws; a std entry
 * that is 0; a mean or std entry that is not finite.  SAT_ERR_UNSUPPORTED: Hc > 524280 or Wc > 2^28 (the launch grid; int indices inside a row).
 */
int sat_image_augment_u8(const uint8_t* src, int Bsrc, int Hs, int Ws, const int32_t* params, const int32_t* order,
                         int B, int Hc, int Wc, const float mean[3] /*[host]*/, const float std[3] /*[host]*/,
                         float* out, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Beam decode (the reference has only a stub, model2.py:113-114, next to the greedy loop
 * models.py:56-67).  Rows are (image b, hypothesis k) = b*K + k, K <= 8.
 * sat_beam_step: candidates (k, v) score scores_in[b,k] + log_softmax(logits[b*K+k])[v]; the best K of the K*V per
 *   image (ties: lower k*V+v) give parent[b,r] (k), token[b,r] (v), scores_out[b,r], r best-first.  A hypothesis with
 *   scores_in = -inf is dead.  last_tokens/end_id (NULL / <0 to disable): a hypothesis whose last token is end_id
 *   only continues with end_id, at unchanged score.  -inf logits are no candidates; a live, unfinished row needs at least one
 *   finite logit (all -inf: its log-softmax is NaN, results undefined).  Fewer than K finite candidates in an image: the
 *   surplus slots get score -inf, parent 0, token 0.
 * sat_beam_gather_rows: dst[b*K+k] = src[b*K+parent[b,k]] (LSTM h/c re-ordering), width floats per row, dst != src.
 * sat_beam_backtrack: parents/tokens [T][B*K] back-pointers -> ids [B*K][T].
 * sat_beam_backtrack_rows (added within ABI 18): the same walk over a per-step record rows [T][B*K][cols] f32 (the attention maps
 *   of a beam decode) -> out [B*K][T][cols].  The row of step t was computed before that step's selection, on the slot the
 *   survivor was expanded from: it is taken at the survivor's PARENT of step t, not at its own slot.  Pure gather, any cols >= 1.
 */
int sat_beam_step(const float* logits /*[B*K, ldl]*/, int64_t ldl, const float* scores_in /*[B*K]*/,
                  const int64_t* last_tokens /*[B*K] or NULL*/, int64_t end_id, int B, int K, int V,
                  int32_t* parent /*[B*K]*/, int64_t* token /*[B*K]*/, float* scores_out /*[B*K]*/,
                  void* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_beam_step_ws_bytes(int B, int K);
int sat_beam_gather_rows(const float* src, const int32_t* parent, int B, int K, int width, float* dst,
                         sat_stream_t stream);
int sat_beam_backtrack(const int32_t* parents, const int64_t* tokens, int T, int B, int K, int64_t* ids,
                       sat_stream_t stream);
int sat_beam_backtrack_rows(const int32_t* parents, const float* rows, int T, int B, int K, int cols, float* out,
                            sat_stream_t stream);
/* The whole decode loop of one batch as ONE call -- the 20 steps of `DecoderRNN.sample` (models.py:56-67; eval.py:99) enqueued from
 * C instead of step by step from the host language (round 4: seven launches per step through the FFI made the beam loop host-bound,
 * 2.44 ms per 20 steps for ~1.3 ms of GPU work).  Same kernels, same order as the step entry points: bit-identical results.
 * lstm_w: HOST array of 4 * num_layers device pointers (w_ih, w_hh, b_ih, b_hh per layer).
 * sat_beam_decode: beam width K <= 8 (the reference's sample_beam is a stub, model2.py:113-114); end_id < 0: none.  ids [B][K][steps]
 *   best first, scores [B][K] (nullable).  workspace: sat_beam_decode_ws_bytes, 256-byte aligned.
 * sat_greedy_decode: h / c [num_layers][B][H] = the initial LSTM state in, the final one out (models.py:61 hands `states` to the
 *   LSTM); h_tmp same size, x_tmp [B][E] scratch; ids [B][ids_stride], column i = step i; workspace: sat_vocab_argmax_ws_bytes. */
int64_t sat_beam_decode_ws_bytes(int B, int K, int E, int H, int V, int num_layers, int steps);
int sat_beam_decode(const float* features /*[B,E]*/, const float* embed /*[V,E]*/, const float* const* lstm_w /*[host]*/, int num_layers,
                    const float* lin_w /*[V,H]*/, const float* lin_b, int B, int K, int E, int H, int V, int steps, int64_t end_id,
                    int64_t* ids, float* scores, void* workspace, int64_t ws_bytes, sat_stream_t stream);
int sat_greedy_decode(const float* features, const float* embed, const float* const* lstm_w /*[host]*/, int num_layers,
                      const float* lin_w, const float* lin_b, int B, int E, int H, int V, int steps, float* h, float* c, float* h_tmp,
                      float* x_tmp, int64_t* ids, int64_t ids_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream);
/* Constrained beam search (added within ABI 18): n-gram blocking, banned ids, a minimum length, and a length penalty on the final
 * ranking.  Step i = 0..T-1.  The PREFIX of row (b, k) at step i is the i tokens y_0..y_{i-1} that hypothesis has emitted, recovered
 * through the back-pointer records `parents` / `tokens` [T][B*K] that the beam loops keep (rows 0..i-1 valid at step i): slot
 * s_{i-1} = k, y_t = tokens[t][b*K + s_t], s_{t-1} = parents[t][b*K + s_t].  Nothing else is carried from step to step: the
 * entry points are stateless.
 * For a LIVE, UNFINISHED row the banned set at step i is the union of
 *   1. suppress_ids[0..n_suppress), at every step (ids outside [0, V) are ignored);
 *   2. end_id, while i < min_length (needs end_id >= 0);
 *   3. y_{i-1}, if block_repeat and i >= 1;
 *   4. if no_repeat_ngram = n >= 1 and i >= n: every y_{j+n-1} with 0 <= j <= i-n and y[j..j+n-2] == y[i-n+1..i-1] (the rule of the
 *      common NoRepeatNGram processors: with n = 1 every token already emitted; an n-gram that overlaps the tail counts).
 * Scores are NOT renormalised: candidate (k, v) scores scores_in[b,k] + (logit[v] - lse) with lse over ALL V columns of the row,
 * exactly as in sat_beam_step; a banned v is no candidate.  (Renormalising would raise a hypothesis's score because probability
 * mass was banned from it; `scores` stays the sum of the model's token log-probabilities.)
 * A FINISHED row (last token == end_id) is untouched by every constraint: its one continuation is end_id at unchanged score.  A
 * DEAD row (-inf) has no candidate.  Everything else is sat_beam_step's contract: order (score desc, flat index k*V+v asc), -inf
 * logits are no candidates, fewer than K candidates leave -inf / parent 0 / token 0 in the surplus slots, a live row needs one
 * finite, unbanned logit (none: the row has no candidate, as if dead).
 * LENGTH PENALTY (length_penalty = alpha; 0: off) is applied ONCE, after the last step, per image: L_k = the number of tokens in
 * front of the first end_id plus 1 for it, T for a row without one (sat_kept_tokens' rule); norm_k = (double)score_k /
 * pow((double)L_k, (double)alpha), rounded once to f32; the K hypotheses are re-ordered by (norm desc, previous rank asc); dead
 * hypotheses stay last.  The search itself still selects by raw score: the fixed-width beam keeps finished hypotheses in their
 * slots, so the final pool is the set a finished-heap implementation would rank.  A re-ranking, not a per-step normalisation.
 * sat_beam_step_ex: sat_beam_step under `c`.  c == NULL or every step field off: the launches of sat_beam_step, bit-identical
 *   outputs (so is a step at which `c` bans nothing).  parents / tokens may be NULL at i == 0 or without active constraints.
 *   workspace: sat_beam_step_ex_ws_bytes (the prefix is walked from the records: no history in the workspace).
 * sat_beam_rerank: ids [B][K][T], scores [B][K] -> ids_out, scores_out (raw, new order), norm_out (nullable), order_out (nullable;
 *   [B][K]: the previous rank of the hypothesis now at r); ids_out != ids, scores_out != scores.  K <= 8, any T >= 1.
 * sat_beam_decode_ex: sat_beam_decode's loop -- the same wide and narrow paths, the same projection -- with the constrained row
 *   kernel at the steps that ban something and the rerank behind the backtrack when length_penalty > 0.  c == NULL or all fields
 *   off: the launches of sat_beam_decode, bit-identical ids and scores.  norm_scores [B][K] and order [B][K] are nullable (without
 *   a penalty: the scores and 0..K-1).  workspace: sat_beam_decode_ex_ws_bytes, 256-byte aligned.  With n-gram blocking the loop
 *   keeps every slot's prefix in its workspace instead of walking the records at every step (same results; SAT_BEAM_HISTORY=0: walk).
 * Errors, before anything is enqueued.  SAT_ERR_ARG: a NULL buffer, a negative field, block_repeat not 0 / 1, n_suppress > 256 or
 *   > 0 with suppress_ids NULL, min_length > 0 with end_id < 0, a length_penalty that is negative or not finite, T < 1, i outside
 *   [0, T), active constraints at i > 0 without records.  SAT_ERR_UNSUPPORTED: K > 8; with active step constraints T (steps) > 64
 *   or V > 65536 (lane t of one wave keeps y_t; the ban bitmap is 8 KiB of LDS).  SAT_ERR_WORKSPACE as elsewhere. */
typedef struct {
    const int64_t* suppress_ids;   /* device, or NULL with n_suppress 0 */
    int n_suppress;                /* 0..256 */
    int min_length;                /* >= 0; > 0 needs end_id >= 0 */
    int no_repeat_ngram;           /* 0 off, n >= 1 */
    int block_repeat;              /* 0 / 1 */
    float length_penalty;          /* finite, >= 0; 0 off; read by the rerank only */
} sat_beam_constraints;
int sat_beam_step_ex(const float* logits /*[B*K, ldl]*/, int64_t ldl, const float* scores_in /*[B*K]*/,
                     const int64_t* last_tokens /*[B*K] or NULL*/, int64_t end_id, int B, int K, int V,
                     const sat_beam_constraints* c /*[host], nullable*/, const int32_t* parents, const int64_t* tokens, int i, int T,
                     int32_t* parent /*[B*K]*/, int64_t* token /*[B*K]*/, float* scores_out /*[B*K]*/,
                     void* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_beam_step_ex_ws_bytes(int B, int K, int V, int T);
int sat_beam_rerank(const int64_t* ids, const float* scores, int B, int K, int T, int64_t end_id, float length_penalty,
                    int64_t* ids_out, float* scores_out, float* norm_out, int32_t* order_out, sat_stream_t stream);
int64_t sat_beam_decode_ex_ws_bytes(int B, int K, int E, int H, int V, int num_layers, int steps);
int sat_beam_decode_ex(const float* features /*[B,E]*/, const float* embed /*[V,E]*/, const float* const* lstm_w /*[host]*/, int num_layers,
                       const float* lin_w /*[V,H]*/, const float* lin_b, int B, int K, int E, int H, int V, int steps, int64_t end_id,
                       const sat_beam_constraints* c /*[host], nullable*/, int64_t* ids, float* scores, float* norm_scores,
                       int32_t* order, void* workspace, int64_t ws_bytes, sat_stream_t stream);
/* Diverse beam search (added within ABI 18; Vijayakumar et al. 2016, arXiv:1610.02424: beam groups with a Hamming diversity penalty).
 * K = beam width <= 8, G = num_groups, 1 <= G <= K, K % G == 0, Kg = K / G.  Slots g*Kg .. g*Kg + Kg - 1 are GROUP g, and a hypothesis
 * never leaves its group: every parent of a slot of group g is a slot of group g.  lambda = diversity_penalty, finite, >= 0.
 * START: slot g*Kg of every group is live at score 0, the other slots are dead (-inf).  G == 1 is the plain start.
 * SELECTION at step i, per image, the groups in order g = 0 .. G-1.  The candidates of group g are the (k, v) with k in group g;
 *   s(k, v) = scores_in[b,k] + (logit[v] - lse), the f32 expression of sat_beam_step / sat_beam_step_ex: lse over ALL V columns, a
 *   banned column is no candidate, nothing is renormalised.  The selection KEY is key = s - lambda * n(v), n(v) = the number of slots
 *   in groups h < g whose token chosen AT THIS SAME STEP is v and counts (below).  The key is formed in f32 as one rounded multiply
 *   and one rounded subtract (no fused multiply-add); n == 0 leaves key = s bit for bit.  The Kg best keys win under (key desc, flat
 *   index k*V+v asc) and become slots g*Kg + r, r = 0 .. Kg-1, best first.  scores_out is the RAW s of the winner, not the key.
 * WHY RAW: `scores` stays the sum of the model's token log-probabilities, as under constraints.  This is eq. 5 of the paper: the
 *   diversity term belongs to the current step's objective only.  Some other implementations fold the penalty into the carried
 *   score; this one does not.
 * A FINISHED row (last token == end_id) has its one continuation, end_id at unchanged score; it is not penalised and its token does
 *   not count.  A DEAD row has no candidate.  A group with fewer than Kg candidates leaves score -inf, parent g*Kg, token 0 in its
 *   surplus slots; these do not count.  WHAT COUNTS: every other chosen token, once per slot that chose it -- two slots of earlier
 *   groups that both chose v give n(v) = 2, and a live row choosing end_id counts.  Tokens chosen within one group do not penalise
 *   each other.
 * The row pass is sat_beam_step_ex's, unchanged: every row's K best raw candidates are deep enough for an exact group selection
 *   (at most K - Kg tokens are penalised, so Kg unpenalised candidates of a row beat everything behind its K-th; the lemma is
 *   written out at beam_merge_groups_kernel).  Constraints compose: bans are per row and applied before the selection.
 * G == 1: the launches of sat_beam_step_ex / sat_beam_decode_ex, bit-identical outputs; diversity_penalty is not read.
 * sat_beam_step_groups: sat_beam_step_ex's arguments with num_groups and diversity_penalty behind T.  scores_in carries the start
 *   above at i == 0 (the caller's).  With G > 1 and end_id >= 0, last_tokens is required at i > 0.  workspace:
 *   sat_beam_step_groups_ws_bytes (= sat_beam_step_ex_ws_bytes).
 * sat_beam_decode_groups: sat_beam_decode_ex's loop and arguments with the two behind `c`.  The search keeps its results in group
 *   order; with G > 1 the result ALWAYS passes through the rerank: order (norm desc, search slot asc), norm = score / L^alpha or the
 *   score itself at length_penalty 0 (c may be NULL); order[b][r] is the search slot of the hypothesis now at rank r, its group is
 *   order / Kg.  workspace: sat_beam_decode_groups_ws_bytes (= sat_beam_decode_ex_ws_bytes), 256-byte aligned.
 * Errors, before anything is enqueued, beside those of the _ex entry points.  SAT_ERR_ARG: G < 1, K % G != 0; with G > 1 a
 *   diversity_penalty that is negative, NaN or infinite, and (step call) end_id >= 0 at i > 0 with last_tokens NULL.
 *   SAT_ERR_UNSUPPORTED: K > 8. */
int sat_beam_step_groups(const float* logits /*[B*K, ldl]*/, int64_t ldl, const float* scores_in /*[B*K]*/,
                         const int64_t* last_tokens /*[B*K] or NULL*/, int64_t end_id, int B, int K, int V,
                         const sat_beam_constraints* c /*[host], nullable*/, const int32_t* parents, const int64_t* tokens, int i, int T,
                         int num_groups, float diversity_penalty, int32_t* parent /*[B*K]*/, int64_t* token /*[B*K]*/,
                         float* scores_out /*[B*K]*/, void* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_beam_step_groups_ws_bytes(int B, int K, int V, int T);
int64_t sat_beam_decode_groups_ws_bytes(int B, int K, int E, int H, int V, int num_layers, int steps);
int sat_beam_decode_groups(const float* features /*[B,E]*/, const float* embed /*[V,E]*/, const float* const* lstm_w /*[host]*/,
                           int num_layers, const float* lin_w /*[V,H]*/, const float* lin_b, int B, int K, int E, int H, int V, int steps,
                           int64_t end_id, const sat_beam_constraints* c /*[host], nullable*/, int num_groups, float diversity_penalty,
                           int64_t* ids, float* scores, float* norm_scores, int32_t* order, void* workspace, int64_t ws_bytes,
                           sat_stream_t stream);
/* Ensemble decode (added within ABI 18): a beam search over the mixed distribution of M models (the ensembles of several checkpoints
 * that Show-and-Tell and the self-critical paper report).  ONE kernel in front of the unchanged selection kernels.
 * sat_ensemble_logprobs: logits is a HOST array of M device pointers, each an [R][ldl] f32 matrix of one model's logits; out [R][ldo]
 *   receives one row of combined log-probabilities per input row.  lse_m = the log-sum-exp of model m's row over all V columns;
 *   w_m = weights[m] / sum(weights), normalised on the host in double and rounded once to f32 (weights NULL: uniform, 1 / M).
 *   mode 0 (probability mean, the usual captioning ensemble): out[v] = log(sum_m w_m * exp(x_m[v] - lse_m)), evaluated as
 *     a_m = x_m[v] - lse_m + log w_m, out = max_m a_m + log(sum_m exp(a_m - max)).
 *   mode 1 (log-probability mean, a product of experts): out[v] = sum_m w_m * (x_m[v] - lse_m), summed in model order; NOT
 *     renormalised here -- the selection kernels subtract the row's lse anyway.
 *   1 <= M <= 8; the pointers reach the kernel by value, there is no device-side pointer table.  A -inf column gives -inf in mode 0
 *   only if every model has -inf there, in mode 1 if any model has (no NaN from 0 * inf).  A row that is all -inf in some model is
 *   undefined (sat_beam_step's rule).  Columns V .. ldo-1 of out are not written.  Any ldl >= V and ldo >= V, odd ones included:
 *   alignment only selects between the 16-byte path (ldl % 4 == 0, ldo % 4 == 0, every base 16-byte aligned) and the scalar path
 *   and never changes a value.  out may not alias an input.  No allocation, no host sync: the call is capturable.
 *   The result goes unchanged into sat_beam_step, sat_beam_step_ex, sat_beam_step_groups and sat_sample_filtered as their `logits`.
 *   In mode 0 the lse those kernels subtract is 0 up to rounding.  The `scores` of an ensemble hypothesis are the sum of
 *   log_softmax(out) as the step kernel forms it.
 *   SAT_ERR_ARG before any launch: a NULL pointer; M outside 1..8; mode not 0 or 1; R or V <= 0; ldl < V or ldo < V; a weight that is
 *   not finite or is <= 0; out equal to an input.
 * sat_beam_decode_ensemble: sat_beam_decode_groups's loop for M DecoderRNN models in lock step.  models is a HOST array of M structs
 *   of device pointers (lstm_w: a host array of 4 * num_layers device pointers, as above).  The models share V; they may differ in
 *   E, H, num_layers and features (every model has its own encoder).  Per step and model: sat_lstm_step per layer on the R = B*K
 *   rows and sat_vocab_logits_fwd (exact f32) into the model's own [R][pad4(V)] matrix; then the combine, the row launch and the
 *   merge launch of sat_beam_decode_groups on the combined matrix (the plain, ban and group variants as there), and per model the
 *   embedding rows of the chosen tokens and the (h, c) re-ordering by parent.  Backtrack, and the rerank under a length penalty or
 *   with G > 1, as there.  K = 1 is the greedy ensemble decode.  A model with ONE layer takes sat_beam_decode's wide step from 128
 *   rows on -- the gates as one split-K exact-f32 GEMM over [x | h], and for V % 4 == 0 the projection from a three-way bf16 split
 *   (f32 accuracy, not the f32 pipe's bit pattern) -- and one launch then moves its embedding rows and (h, c).  The kernels that
 *   run are a function of the shapes alone: the same inputs give the same bits in every process.
 *   ids [B][K][steps], scores / norm_scores / order [B][K] (nullable) as sat_beam_decode_groups.  workspace:
 *   sat_beam_decode_ensemble_ws_bytes (0 for arguments the call refuses), 256-byte aligned.
 *   Errors, before anything is enqueued: those of sat_beam_decode_groups and of sat_ensemble_logprobs's (M, weights, mode);
 *   SAT_ERR_ARG for a NULL field or a non-positive size in a model; SAT_ERR_UNSUPPORTED for a model with E % 4 != 0, H % 4 != 0 or
 *   more than 8 layers. */
typedef struct {
    const float* features;         /* [B][E] */
    const float* embed;            /* [V][E] */
    const float* const* lstm_w;    /* HOST array of 4 * num_layers device pointers (w_ih, w_hh, b_ih, b_hh per layer) */
    int num_layers;
    const float* lin_w;            /* [V][H] */
    const float* lin_b;            /* [V] */
    int E;
    int H;
} sat_decoder_model;               /* host struct, device pointers */
int sat_ensemble_logprobs(const float* const* logits /*[host] M device pointers, each [R][ldl]*/, int M, int64_t ldl,
                          const float* weights /*[host] M, or NULL = uniform*/, int mode, int R, int V, float* out /*[R][ldo]*/,
                          int64_t ldo, sat_stream_t stream);
int64_t sat_beam_decode_ensemble_ws_bytes(const sat_decoder_model* models /*[host]*/, int M, int B, int K, int V, int steps);
int sat_beam_decode_ensemble(const sat_decoder_model* models /*[host]*/, int M, const float* weights /*[host] M or NULL*/, int mode,
                             int B, int K, int V, int steps, int64_t end_id, const sat_beam_constraints* c /*[host], nullable*/,
                             int num_groups, float diversity_penalty, int64_t* ids, float* scores, float* norm_scores, int32_t* order,
                             void* workspace, int64_t ws_bytes, sat_stream_t stream);
/* Scheduled sampling (the reference's DecoderRNN.ss_prob, models.py:38, and its schedule, train.py:109-113) in the training forward.
 * Random numbers: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), u = ((x >> 8) + 0.5) * 2^-24.  The draw for row b of step t is
 * s(b, t) = first argmax_v (logit[b][v] + G(b, t, v)), G = -log(-log u) of counter (v >> 2, b, t, 2*rank), word v & 3 (Gumbel-max: an
 * exact draw from softmax(logits)); mask(b, t) = u < ss_prob of counter (0, b, t, 2*rank + 1), word 0.
 * sat_vocab_sample: ONE step over B rows: logits = h lin_w^T + lin_b (stored when `logits` != NULL); ids[b*ids_stride] = mask(b, t) ?
 *   s(b, t) : teacher[b*teacher_stride] (teacher NULL: s(b, t) for every row); where a draw was taken and embed / x are given,
 *   x[b*E..] = embed[ids[b]] (other rows of x are not written).  workspace: sat_ss_decoder_fwd_ws_bytes(B, V).
 * sat_ss_decoder_fwd: the whole decoder forward (models.py:47-53) with scheduled sampling, as ONE call: captions [B][cap_stride] are
 *   the teacher's inputs (train.py's captions[:, :-1]), step t = 0..T-1 feeds features (t = 0), embed[used[b][t-1]] after, with
 *   used[b][0] = captions[b][0] and, for t >= 2, used[b][t-1] = mask(b, t) ? s(b, t) from the logits of step t-1 : captions[b][t-1];
 *   used [B][used_stride] (>= T-1 columns) out, the teacher's tokens in every column a row does not reach.  lstm_w: HOST array of
 *   4 * num_layers device pointers (w_ih, w_hh, b_ih, b_hh per layer); tapes: HOST array of 5 * num_layers device pointers per
 *   layer (GA [N,4H], CS [N,H], HS [N,H], HP [N,H], c_state [B,H]) that receive exactly what sat_lstm_fwd leaves there, so
 *   sat_lstm_bwd / sat_lstm_bwd_bf16 and sat_embed_concat_bwd (on `used`) are its backward; X [N,E] the layer-0 input out; logits
 *   [N,ldl] (exact f32) or NULL (draws only; the caller projects all rows afterwards, e.g. sat_vocab_ce_fwd_bf16).  ss_prob and
 *   seed are kernel arguments: no host synchronisation.  workspace: sat_ss_decoder_fwd_ws_bytes(batch_sizes[0], V). */
int64_t sat_ss_decoder_fwd_ws_bytes(int B, int V);
int sat_vocab_sample(const float* h /*[B,H]*/, const float* lin_w, const float* lin_b, int B, int H, int V, float* logits, int64_t ldl,
                     float ss_prob, uint64_t seed, int t, int rank, const int64_t* teacher, int64_t teacher_stride, int64_t* ids,
                     int64_t ids_stride, const float* embed, int E, float* x, float* workspace, int64_t ws_bytes, sat_stream_t stream);
int sat_ss_decoder_fwd(const float* features /*[B,E]*/, const float* embed /*[V,E]*/, const int64_t* captions, int64_t cap_stride,
                       const int32_t* batch_sizes /*[host] T*/, const int32_t* prefix /*[T+1] device*/, int T, int E, int V,
                       const float* const* lstm_w /*[host]*/, int num_layers, int H, const float* lin_w, const float* lin_b,
                       float* const* tapes /*[host]*/, float* X, float* logits, int64_t ldl, float ss_prob, uint64_t seed, int rank,
                       int64_t* used, int64_t used_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream);
/* Dropout on a dense f32 tape, forward and backward: y[r][j] = keep(r, j) ? x[r][j] * scale : 0 for r < rows, j < cols; x rows ldx
 * floats apart, y rows ldy apart, columns [cols, ld) of y untouched; y == x (in place) is allowed, any other overlap is not.  The
 * backward is the same call with the same (p, seed, rank, site) on the gradient: the mask is regenerated, never stored.
 * Random numbers: Philox4x32-10 as above, key (seed & 0xffffffff, seed >> 32); element (r, j) reads word j & 3 of counter
 * (j >> 2, r, 0x80000000 | site, 2*rank).  The high bit of counter word 2 keeps these streams apart from every scheduled-sampling,
 * rollout and stochastic-decode draw (those carry the step index t there), so a seed reused by accident cannot correlate a mask
 * with a token draw.  keep(r, j) = (word >> 8) >= thr, thr = (uint32_t)lrint((double)p * 16777216.0), computed once on the host
 * side of the call: an integer comparison, so a host reference and the device cannot differ by a rounding.  scale =
 * (float)(1.0 / (1.0 - (double)p)); the product is one f32 multiply.  p == 0: thr = 0, scale = 1, an exact copy (in place: returns
 * without a launch).  site: which activation of a model (the models' numbering: DESIGN.md); rank: the data-parallel rank.
 * SAT_ERR_ARG, before anything is enqueued, unless 0 <= p < 1 (finite), rows, cols >= 0, ldx, ldy >= cols, 0 <= site < 2^31 and
 * rank >= 0; rows == 0 or cols == 0: SAT_OK without a launch.  Any cols and any leading dimension work: rows whose bases are
 * 16-byte aligned (pointers and leading dimensions) move as 16-byte loads and stores, the rest element by element. */
int sat_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int cols, float p, uint64_t seed, int rank, int site,
                    sat_stream_t stream);
/* Scheduled sampling in the Show-Attend-Tell training forward (model2.py:38-85, the model train.py:37 builds; schedule
 * train.py:109-113).  Same random numbers as above; rows b < batch_sizes[t+1] of step t+1 >= 1 are fed, in the embedding half of
 * the LSTMCell input [emb | ctx], used[b][t+1] = mask(b, t+1) ? s(b, t+1) : captions[b][t+1], s drawn from the logits of step t
 * (classifier(context2out(ctx_t) + hidden2tout(h_t))); used[b][0] = captions[b][0] (<start>) and the context half is always step
 * t+1's own attention context.
 * sat_ss_attend_fwd: the decoder loop as ONE call, no host synchronisation.  Given feats [B*P,C] (the encoder features, rows
 *   (b, p)), ctx_enc = feats image_att_w, h0 / c0 [B,H] (init_lstm), captions [B][cap_stride >= T] (train.py's captions[:, :-1]),
 *   batch_sizes [host] / prefix [device, T+1] of the packed order; H == E + C.  w: HOST array of SAT_SSA_NUM_WEIGHTS device
 *   pointers (SAT_SSA_* order below); tapes: HOST array of SAT_SSA_NUM_TAPES device pointers that receive what the teacher-forced
 *   forward leaves in them: PROJ [N,C] (weight_hh(h_{t-1})), ALPHA [N,P], X [N,H] (= [emb | ctx] of every packed row), GATES [N,4H]
 *   (activated), CS [N,H], HS [N,H] (h_t), Zin [N,C+H] (= [ctx | h]), Z [N,E] (the output layer before the classifier).
 *   toks [N] int64 out: the packed tokens fed; logits [N,ldl] out (exact f32, ldl % 4 == 0, pad columns untouched);
 *   used [B][used_stride >= T] out.  Null or impossible arguments: SAT_ERR_ARG before anything is enqueued.
 *   workspace: sat_ss_attend_fwd_ws_bytes(batch_sizes[0], P, C, E, H, V) = the sum, each rounded up to 256 bytes, of
 *   sat_ss_decoder_fwd_ws_bytes(B, V) (draw partials), sat_attention_ws_bytes(B, P), max over M <= B of
 *   sat_skinny_gemm_ws_bytes(M, C, H) and (M, E, C) (split-K slabs), B*H*4 (cell state) and E*4 (b_c2o + b_h2o); 0 for
 *   non-positive sizes. */
enum {
    SAT_SSA_WEIGHT_HH_W, SAT_SSA_WEIGHT_HH_B, SAT_SSA_WEIGHT_ATT, SAT_SSA_EMBEDDING, SAT_SSA_CELL_W_IH, SAT_SSA_CELL_W_HH,
    SAT_SSA_CELL_B_IH, SAT_SSA_CELL_B_HH, SAT_SSA_C2O_W, SAT_SSA_C2O_B, SAT_SSA_H2O_W, SAT_SSA_H2O_B, SAT_SSA_CLS_W, SAT_SSA_CLS_B,
    SAT_SSA_NUM_WEIGHTS
};
enum { SAT_SSA_PROJ, SAT_SSA_ALPHA, SAT_SSA_X, SAT_SSA_GATES, SAT_SSA_CS, SAT_SSA_HS, SAT_SSA_ZIN, SAT_SSA_Z, SAT_SSA_NUM_TAPES };
int64_t sat_ss_attend_fwd_ws_bytes(int B, int P, int C, int E, int H, int V);
int sat_ss_attend_fwd(const float* feats, const float* ctx_enc, const float* h0, const float* c0, const int64_t* captions,
                      int64_t cap_stride, const int32_t* batch_sizes /*[host] T*/, const int32_t* prefix /*[T+1] device*/, int T, int P,
                      int C, int E, int H, int V, const float* const* w /*[host]*/, float* const* tapes /*[host]*/, int64_t* toks,
                      float* logits, int64_t ldl, float ss_prob, uint64_t seed, int rank, int64_t* used, int64_t used_stride,
                      float* workspace, int64_t ws_bytes, sat_stream_t stream);
/* The truncation rule of the reference's id -> word loop (`evaluation`, eval.py:103-109: `if word == '<end>': break`):
 * kept[b] = number of ids of row b in front of the first end_id (T when the row has none).  ids: [B] rows of T int64 with
 * `stride` elements between rows (model.sample's [B,20], or one hypothesis plane of the beam ids). */
int sat_kept_tokens(const int64_t* ids, int64_t stride, int B, int T, int64_t end_id, int32_t* kept /*[B]*/,
                    sat_stream_t stream);
/* Stochastic decode (added within ABI 18): a token per row drawn after temperature, top-k and nucleus (top-p) filtering -- the
 * decode mode beside the arg-max (sat_greedy_decode) and the beam (sat_beam_decode).  No sort, no host read.
 * sat_sample_filtered: R rows of V logits (row stride ldl >= V floats; columns [V, ldl) are never candidates, whatever they hold).
 *   Total order of a row: its candidates -- columns with a logit above -inf (a NaN is no candidate) -- by float value descending,
 *     equal values by ascending column; +0.0 and -0.0 are equal.
 *   top-k: with 0 < top_k < number of candidates only the first top_k of that order stay (0 or >= V: off).
 *   nucleus: tau = (double)temperature, w_v = exp((x_v - x_max) / tau), Z = sum of w over what top-k left; with top_p < 1 the
 *     shortest prefix of the order whose cumulative w reaches (double)top_p * Z stays, at least one token (top_p == 1: off).  The
 *     masses are summed as integers floor(w * 2^48): a prefix sum loses < V * 2^-48 (1.2e-10 at the largest V), so a decision
 *     further than 1e-6 * Z from top_p * Z is that of exact arithmetic; closer, the one boundary token may go either way.
 *   draw: ids[r*ids_stride] = first argmax over the KEPT columns of x_v / temperature + G(r, t, v), G as for sat_vocab_sample below
 *     (Philox4x32-10, counter (v >> 2, r, t, 2*rank), word v & 3, key from seed); evaluated for kept columns only.  With
 *     temperature 1, top_k 0, top_p 1 this is s(r, t) of sat_vocab_sample / the rollouts on the same logits.
 *   kept[r] (nullable) = size of the kept set (a prefix of the total order: the count identifies it); logp[r] (nullable) =
 *     ln(w_tok / sum of w over the kept set), evaluated in f64 and rounded once.
 *   A row needs one finite logit; without one the token is undefined but inside [0, V).  ids, kept and logp depend on (row
 *   contents, temperature, top_k, top_p, seed, rank, r, t) only -- not on R, ldl or the launch -- and are the same in every run.
 *   SAT_ERR_ARG: logits, ids or workspace NULL; R < 1; V < 1; ldl < V; ids_stride < 1; temperature not finite or <= 0; top_k < 0;
 *   top_p outside (0, 1]; t < 0; rank < 0.  SAT_ERR_UNSUPPORTED: V > 32768.  SAT_ERR_WORKSPACE: ws_bytes <
 *   sat_sample_filtered_ws_bytes(R, V) (0 for non-positive sizes).  All before anything is enqueued.
 * sat_sample_decode: sat_greedy_decode's loop and state handling (h / c in and out, h_tmp, x_tmp) with sat_sample_filtered (t = the
 *   step, row r = b) where it takes the arg-max: per step sat_lstm_step per layer, sat_vocab_logits_fwd (exact f32, stored),
 *   the filtered draw, sat_embed_rows.  Nullable outputs: logp [B][steps], kept [B][steps], logits_out [steps*B][ldl] (row t*B + b =
 *   step t of row b; ldl >= V).  Rows keep running behind <end> (sat_kept_tokens truncates).  Errors as above and as
 *   sat_greedy_decode's, before anything is enqueued; workspace: sat_sample_decode_ws_bytes (0 for non-positive sizes). */
int64_t sat_sample_filtered_ws_bytes(int R, int V);
int sat_sample_filtered(const float* logits /*[R, ldl]*/, int64_t ldl, int R, int V, float temperature, int top_k, float top_p,
                        uint64_t seed, int t, int rank, int64_t* ids, int64_t ids_stride, float* logp /*[R] or NULL*/,
                        int32_t* kept /*[R] or NULL*/, void* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_sample_decode_ws_bytes(int B, int E, int H, int V, int num_layers);
int sat_sample_decode(const float* features, const float* embed, const float* const* lstm_w /*[host]*/, int num_layers,
                      const float* lin_w, const float* lin_b, int B, int E, int H, int V, int steps, float temperature, int top_k,
                      float top_p, uint64_t seed, int rank, float* h, float* c, float* h_tmp, float* x_tmp, int64_t* ids,
                      int64_t ids_stride, float* logp, int32_t* kept, float* logits_out, int64_t ldl, void* workspace,
                      int64_t ws_bytes, sat_stream_t stream);
/* Constrained sampling (added within ABI 18): banned ids, n-gram blocking and a repetition penalty on the filtered draw.
 * At step t row r has the prefix y_0 .. y_{t-1}, the tokens this decode drew for the row at earlier steps (the start token is not
 * part of it), read from prefix[r*prefix_stride + j], j < t.  The row of logits x[0..V) is replaced by x', and EVERYTHING ELSE IS
 * sat_sample_filtered's CONTRACT APPLIED TO x': candidates, total order, top-k, nucleus, the Gumbel-max draw with the same Philox
 * counters, kept, and logp under the filtered distribution of x'.  The kernel never writes the row: a caller's logits stay raw.
 *   penalty: repetition_penalty = theta (finite, > 0; 1: off).  For every v among the prefix tokens, once however often it
 *     occurs: x'[v] = x[v] > 0 ? x[v] / theta : x[v] * theta -- ONE correctly rounded f32 division or multiplication.  -inf and NaN
 *     stay what they are.
 *   bans: x'[v] = -inf (no candidate) for v in the banned set of sat_beam_step_ex's four rules with i = t: (1) suppress_ids;
 *     (2) end_id while t < min_length; (3) y_{t-1} if block_repeat and t >= 1; (4) if no_repeat_ngram = n >= 1 and t >= n: every
 *     y_{j+n-1} with 0 <= j <= t-n and y[j..j+n-2] == y[t-n+1..t-1] (n = 1: every token already drawn; overlap with the tail
 *     counts).  A ban wins over the penalty.
 *   scope: every step of every row, also behind the row's end_id (rows keep running there; sat_kept_tokens truncates): there is no
 *     finished row.  A row whose every candidate is banned is a row without a finite logit: id 0, kept 0, logp -inf.
 *   memory safety: prefix tokens and suppressed ids outside [0, V) set nothing; in the n-gram compare every such prefix token is
 *     one and the same "no token".
 * sat_sample_filtered_ex: sat_sample_filtered under `c` at step t.  c == NULL, every field off, or a step at which `c` changes
 *   nothing (no suppressed id, t >= min_length, and t == 0 or no rule that reads the prefix, or t < n with n-gram blocking alone):
 *   the launch of sat_sample_filtered, bit-identical outputs; prefix is then not read and may be NULL.  workspace:
 *   sat_sample_filtered_ws_bytes.
 * sat_sample_decode_ex: sat_sample_decode's loop with the ids buffer itself as the prefix (row b: ids[b*ids_stride + j]);
 *   workspace: sat_sample_decode_ex_ws_bytes (= sat_sample_decode_ws_bytes).
 * Errors beside those of the plain entry points, before anything is enqueued.  SAT_ERR_ARG: n_suppress > 256 or > 0 with
 *   suppress_ids NULL, a negative field, block_repeat not 0 / 1, repetition_penalty not finite or <= 0, min_length > 0 with
 *   end_id < 0, prefix NULL (or prefix_stride < 0) at a step t > 0 whose rules read it.  SAT_ERR_UNSUPPORTED: a step whose rules
 *   read the prefix with t >= 64 (lane j of one wave keeps y_j); steps > 64 in the loop under active constraints; V > 32768. */
typedef struct {
    const int64_t* suppress_ids;   /* device, or NULL with n_suppress 0 */
    int n_suppress;                /* 0..256 */
    int min_length;                /* >= 0; > 0 needs end_id >= 0 */
    int no_repeat_ngram;           /* 0 off, n >= 1 */
    int block_repeat;              /* 0 / 1 */
    float repetition_penalty;      /* finite, > 0; 1 off */
    int64_t end_id;                /* < 0: none */
} sat_sample_constraints;
int sat_sample_filtered_ex(const float* logits /*[R, ldl]*/, int64_t ldl, int R, int V, float temperature, int top_k, float top_p,
                           uint64_t seed, int t, int rank, int64_t* ids, int64_t ids_stride, float* logp /*[R] or NULL*/,
                           int32_t* kept /*[R] or NULL*/, const sat_sample_constraints* c /*[host], nullable*/,
                           const int64_t* prefix, int64_t prefix_stride, void* workspace, int64_t ws_bytes, sat_stream_t stream);
int64_t sat_sample_decode_ex_ws_bytes(int B, int E, int H, int V, int num_layers);
int sat_sample_decode_ex(const float* features, const float* embed, const float* const* lstm_w /*[host]*/, int num_layers,
                         const float* lin_w, const float* lin_b, int B, int E, int H, int V, int steps, float temperature, int top_k,
                         float top_p, uint64_t seed, int rank, float* h, float* c, float* h_tmp, float* x_tmp, int64_t* ids,
                         int64_t ids_stride, float* logp, int32_t* kept, float* logits_out, int64_t ldl,
                         const sat_sample_constraints* cons /*[host], nullable*/, void* workspace, int64_t ws_bytes,
                         sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * CIDEr of decoded id rows against reference captions (added within ABI 18).
 * pycocoevalcap/cider/cider_scorer.py:93-181, `CiderScorer.compute_score()` with n = 4, the number train.py:169-177 keeps
 * model-best.pth by.  Tokens are opaque int32 ids >= 0; everything below is f64.
 *   df[g]    = number of corpus images whose reference set holds n-gram g (orders 1..4) at least once
 *   ref_len  = log(number of corpus images)
 *   w(g)     = tf(g) * (ref_len - log(max(1, df[g])))      an n-gram the corpus lacks: df = 0, w = tf * ref_len (it still counts
 *                                                           in the hypothesis norm)
 *   norm[o]  = sqrt(sum over the caption's distinct n-grams of order o of w^2)
 *   length   = sum of tf over BIGRAMS = max(tokens - 1, 0)  (cider_scorer.py:128 tests the 0-based order against 1)
 *   val[o]   = sum over the hypothesis's distinct n-grams of min(w_hyp, w_ref) * w_ref, / (norm_hyp[o] * norm_ref[o]) only when
 *              both are non-zero, * exp(-(length_hyp - length_ref)^2 / (2 sigma^2))          per reference
 *   score    = mean over the 4 orders of (sum over the image's references of val[o]) / references * 10
 *   mean     = sum of the B scores (fixed order) / B
 * Every sum runs in the order the reference walks its dicts (first occurrence in the caption); two calls give the same bits.
 *
 * The corpus n-grams are the nodes of a trie: node 0 is the root, node j + 1 has key keys[j] = (parent node << 32) | token, and
 * df[j] is its document frequency.  The table is open addressing with linear probing, slot(key) = ((key * 0x9E3779B97F4A7C15)
 * >> 32) & (capacity - 1), compares whole keys and is probed at most `capacity` times: a lookup is exact and always ends.
 * sat_cider_table_insert: clears table_keys / table_nodes / status and inserts keys[0..n_keys) (one 64-bit compare-and-swap per
 *   probed slot, node id stored beside the key; nothing reads the table in that launch).  *status (device i32) becomes non-zero
 *   when the table filled up (bit 0) or a key came twice (bit 1); the caller reads it once.  capacity: a power of two >=
 *   2 * n_keys.
 * sat_cider_ref_stats: ref_norm[n_refs][4], the norms of every reference caption -- the same device function that the scoring
 *   kernel runs over a hypothesis (one `log`, one code path).
 * sat_cider_score: scores[b] for row b of ids ([B] rows of T int64, `stride` elements apart) against the references of image
 *   image_index[b] (device i32 [B]; an image may come several times; clamped into the corpus in the kernel as a safety net), and
 *   mean[0].  The row ends at kept[b] (device i32 [B] as sat_kept_tokens writes it, clamped to [0, T]) or, with kept NULL, in
 *   front of its first end_id.  An id outside [0, 2^31) is no corpus token.  One wave per row; no allocation, no host sync.
 * SAT_ERR_ARG before anything is enqueued: a NULL pointer (kept excepted); n_keys, n_nodes, n_refs, n_images, n_tokens,
 * max_ref_tokens, B or T <= 0; stride < T; capacity not a power of two or below 2 * n_nodes; sigma not finite or <= 0.
 * SAT_ERR_UNSUPPORTED: T > 64, max_ref_tokens > 128, capacity > 2^32.
 */
typedef struct sat_cider_corpus {
    const uint64_t* table_keys;    /* [capacity] device */
    const int32_t* table_nodes;    /* [capacity] device */
    const int32_t* df;             /* [n_nodes] device */
    const int32_t* ref_tokens;     /* [n_tokens] device: the reference captions back to back */
    const int32_t* ref_offsets;    /* [n_refs + 1] device: caption r is ref_tokens[ref_offsets[r] .. ref_offsets[r+1]) */
    const int32_t* image_offsets;  /* [n_images + 1] device: image i owns captions image_offsets[i] .. image_offsets[i+1] */
    const double* ref_norm;        /* [n_refs][4] device (sat_cider_ref_stats writes it; may be NULL there) */
    int64_t capacity, n_tokens;
    int32_t n_nodes, n_refs, n_images;
    int32_t max_ref_tokens;        /* the longest reference caption, as the host counted it */
} sat_cider_corpus;
int sat_cider_table_insert(const uint64_t* keys, int n_keys, uint64_t* table_keys, int32_t* table_nodes, int64_t capacity,
                           int32_t* status, sat_stream_t stream);
int sat_cider_ref_stats(const sat_cider_corpus* corpus /*[host]*/, double* ref_norm, sat_stream_t stream);
int sat_cider_score(const sat_cider_corpus* corpus /*[host]*/, const int64_t* ids, int64_t stride, int B, int T,
                    const int32_t* kept /*[B] or NULL*/, int64_t end_id, const int32_t* image_index /*[B]*/, double sigma,
                    double* scores /*[B]*/, double* mean /*[1]*/, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Consensus (minimum-Bayes-risk) reranking of decoded candidates by pairwise CIDEr (added within ABI 18): every candidate of an
 * image is scored against the OTHER candidates of the same image with the corpus's document frequencies, and the candidate the
 * rest agree with most is picked -- the selection for images that have no reference captions.
 *
 * Image b has K candidates ids[b][i][0..T): candidate i of image b starts at ids + b * image_stride + i * cand_stride.
 * Candidate i has L_i tokens: kept[b*K+i] clamped to [0, T], or with kept == NULL the position of its first end_id (T without
 * one).  The corpus gives log_images = log(n_images) and df: exactly sat_cider_score's corpus, nothing new is built on the host
 * (its reference captions and ref_norm are not read).
 *
 * For candidate i as hypothesis and candidate j != i as the single reference, with w_x(g) = tf_x(g) * (log_images -
 * log(max(1, df[g]))):
 *   val_ij[o] = sum over the DISTINCT order-o n-grams g of i, in order of first occurrence, of  min(w_i(g), w_j(g)) * w_j(g)
 *               / (norm_i[o] * norm_j[o])   only when both are non-zero
 *               * exp(-(len_i - len_j)^2 / (2 sigma^2)),        len_x = max(L_x - 1, 0)
 *   pair[b][i][j] = (((val_ij[0] + val_ij[1]) + val_ij[2]) + val_ij[3]) / 4 * 10           pair[b][i][i] = +0.0 (not computed)
 * Utility with weights == NULL (uniform):
 *   tot[o] = sum over j != i, in slot order, of val_ij[o]
 *   utility[b][i] = (((tot[0] + tot[1]) + tot[2]) + tot[3]) / 4 / (K - 1) * 10;   K == 1: utility 0.
 * This is CiderScorer.compute_cider() of candidate i with the other K - 1 candidates as its reference set, operation for operation.
 * Utility with weights (device f64 [B][K], finite and >= 0, not checked on the device):
 *   tot[o] = sum over j != i, in slot order, of w_j * val_ij[o];   den = sum over j != i, in slot order, of w_j
 *   utility = (((tot[0] + tot[1]) + tot[2]) + tot[3]) / 4 / den * 10, or 0 when den == 0.
 * best[b] is the first slot of maximal utility (int64; a NaN utility is never picked over a number).
 *
 * Unlike sat_cider_score, an n-gram the corpus lacks (df = 0, weight tf * log_images) DOES match the same n-gram in another
 * candidate: matches are by token comparison, never by node id.  An id outside [0, 2^31) is no token: it becomes -1 where its row
 * is the hypothesis and -2 where it is the reference, so it never matches anything across rows, itself included; it still counts
 * in L.  Every sum has the fixed order stated above: two calls give the same bits, and row b's results do not depend on B.
 *
 * Three launches: one wave per (image, candidate) leaves the candidate's norms and length in the workspace; one wave per (image,
 * candidate) walks the other candidates of its image and writes pair and utility; one thread per image picks best.  No
 * allocation, no host read, no workgroup waits for another.  workspace: sat_consensus_ws_bytes(B, K) bytes at an 8-byte aligned
 * address (0 for non-positive sizes).
 * SAT_ERR_ARG before anything is enqueued: a NULL pointer (kept, weights and pair excepted); B, K or T <= 0; cand_stride < T;
 * image_stride < K * cand_stride when B > 1; sigma not finite or <= 0; a corpus that sat_cider_score refuses (ref_norm may be
 * NULL); a workspace that is not 8-byte aligned.  SAT_ERR_UNSUPPORTED: T > 64, K > 64, B * K >= 2^31.  SAT_ERR_WORKSPACE:
 * ws_bytes < sat_consensus_ws_bytes(B, K).
 */
int64_t sat_consensus_ws_bytes(int B, int K);
int sat_consensus_rerank(const sat_cider_corpus* corpus /*[host]*/, const int64_t* ids, int64_t image_stride, int64_t cand_stride,
                         int B, int K, int T, const int32_t* kept /*[B*K] or NULL*/, int64_t end_id, double sigma,
                         const double* weights /*[B][K] or NULL*/, double* utility /*[B][K]*/, int64_t* best /*[B]*/,
                         double* pair /*[B][K][K] or NULL*/, void* workspace, int64_t ws_bytes, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * BLEU-1..4 and ROUGE-L of decoded id rows against reference captions (added within ABI 18): the other plain-arithmetic metrics
 * of language_eval (eval.py:17-56).  Rows, `kept` / end_id, image_index and the flat corpus are those of sat_cider_score: ids is
 * [B] rows of T <= 64 int64, `stride` elements apart; row b has L tokens, L = kept[b] clamped to [0, T] or, with kept NULL, the
 * position of its first end_id; image_index[b] is clamped into the corpus; an id outside [0, 2^31) equals no reference token and
 * still counts in L.  One wave per row, n-grams compared token by token (no trie, no table); no allocation, no host sync.
 *
 * sat_bleu_comps: cook_test + compute_score(option='closest') (pycocoevalcap/bleu/bleu_scorer.py:60-83, 198-256), per row
 *   testlen    = L
 *   reflen     = the length l of a reference of the image that minimises (|l - L|, l): a tie goes to the shorter
 *   guess[k]   = max(0, L - k)                                                            k = 0..3, (k+1)-grams
 *   correct[k] = sum over the row's DISTINCT (k+1)-grams g of min(count of g in the row, max over the image's references of
 *                the count of g in that reference) -- the maximum may come from another reference for each g
 *   comps[b]   = { testlen, reflen, guess[0..3], correct[0..3] }                         int64 [B][10]: exact
 *   p          = 1;  for k = 0..3:  p = p * ((correct[k] + 1e-15) / (guess[k] + 1e-9));  s[k] = pow(p, 1 / (k + 1))
 *   ratio      = (testlen + 1e-15) / (reflen + 1e-9);  if ratio < 1:  s[k] = s[k] * exp(1 - 1 / ratio)
 *   sentence[b] = s                                                                      f64 [B][4]: the per-image bleu_list
 *   mean[k]    = sum over b of sentence[b][k] (fixed order) / B                          f64 [4], or NULL: not computed
 *   totals[j] += sum over b of comps[b][j]                                               device int64 [10], or NULL: untouched
 *   (64-bit integer atomics: integer sums, so the same bits in any order.  The caller zeroes totals where a corpus begins.)
 * sat_bleu_finalize: bleu[k], f64 [4], the same p / pow / ratio / exp arithmetic on totals: the corpus-level Bleu_1..4 of every
 *   row added since totals was zeroed.  One wave.
 * sat_rouge_l_score: Rouge.calc_score (pycocoevalcap/rouge/rouge.py:45-75).  The reference splits with split(" "), so an EMPTY
 *   caption (row or reference) is ONE token, which equals only the token of another empty caption; with len() counted that way
 *   lcs(r)   = length of the longest common subsequence of the row and reference r      an integer: exact
 *   prec_max = max over the image's references of lcs(r) / len(row);  rec_max = max over them of lcs(r) / len(r)
 *   score    = ((1 + beta*beta) * prec_max * rec_max) / (rec_max + beta*beta * prec_max), or 0 when either maximum is 0
 *   scores[b] = score, f64 [B];  mean[0] = sum of the B scores (fixed order) / B.
 *   The LCS is bit-parallel: the row's positions are the bits of one 64-bit word V (all ones at first); per reference token with
 *   match mask M:  U = V & M;  V = (V + U) | (V - U);  lcs = zero bits of V below len(row).
 * Two calls give the same bits.
 * SAT_ERR_ARG before anything is enqueued: a NULL pointer (kept, and sat_bleu_comps's mean and totals, excepted); n_refs,
 * n_images, n_tokens, max_ref_tokens, B or T <= 0; stride < T; beta not finite or <= 0.  SAT_ERR_UNSUPPORTED: T > 64,
 * max_ref_tokens > 128.
 */
typedef struct sat_ref_corpus {
    const int32_t* ref_tokens;     /* [n_tokens] device: the reference captions back to back (sat_cider_corpus's array) */
    const int32_t* ref_offsets;    /* [n_refs + 1] device: caption r is ref_tokens[ref_offsets[r] .. ref_offsets[r+1]) */
    const int32_t* image_offsets;  /* [n_images + 1] device: image i owns captions image_offsets[i] .. image_offsets[i+1] */
    int64_t n_tokens;
    int32_t n_refs, n_images;
    int32_t max_ref_tokens;        /* the longest reference caption, as the host counted it */
    int32_t reserved;
} sat_ref_corpus;
int sat_bleu_comps(const sat_ref_corpus* corpus /*[host]*/, const int64_t* ids, int64_t stride, int B, int T,
                   const int32_t* kept /*[B] or NULL*/, int64_t end_id, const int32_t* image_index /*[B]*/,
                   int64_t* comps /*[B][10]*/, double* sentence /*[B][4]*/, double* mean /*[4] or NULL*/,
                   int64_t* totals /*[10] or NULL*/, sat_stream_t stream);
int sat_bleu_finalize(const int64_t* totals /*[10]*/, double* bleu /*[4]*/, sat_stream_t stream);
int sat_rouge_l_score(const sat_ref_corpus* corpus /*[host]*/, const int64_t* ids, int64_t stride, int B, int T,
                      const int32_t* kept /*[B] or NULL*/, int64_t end_id, const int32_t* image_index /*[B]*/, double beta,
                      double* scores /*[B]*/, double* mean /*[1]*/, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Self-critical sequence training (Rennie et al. 2017; added within ABI 18): a caption SAMPLED from the model is trained with its
 * cross entropy weighted by CIDEr(sampled) - CIDEr(greedy).  Nothing here synchronises or reads back; every entry point returns
 * SAT_ERR_ARG for null or impossible arguments and SAT_ERR_WORKSPACE for a short workspace before anything is enqueued.
 * sat_rollout_decoder_fwd: DecoderRNN.sample (models.py:56-67) in training form, ONE call for `steps` steps of all B rows: step 0
 *   feeds features, step t >= 1 feeds embed[ids[b][t-1]]; every step runs the fused LSTM step per layer from a zero initial state
 *   and the exact-f32 vocab projection, and ids[b][t] = s(b, t) of sat_vocab_sample's convention, drawn from step t's own logits
 *   (counter (v >> 2, b, t, 2*rank), word v & 3: every row draws at every step, t = 0 included; no mask draw, no teacher).  Rows keep
 *   running after they emit <end>; they are masked by sat_scst_weights.  Packed rows are n = t*B + b (batch_sizes = [B] * steps):
 *   tapes (HOST array of 5 * num_layers device pointers, as for sat_ss_decoder_fwd) receive exactly what sat_lstm_fwd leaves there,
 *   X [steps*B, E] the layer-0 input, logits [steps*B, ldl >= V] (pad columns untouched), ids [B][ids_stride >= steps].  Its
 *   backward is sat_vocab_ce_bwd -> sat_lstm_bwd -> sat_embed_concat_bwd on ids[:, :steps-1].  E, H multiples of 4;
 *   num_layers <= 8; lstm_w as for sat_ss_decoder_fwd.  workspace: sat_rollout_decoder_fwd_ws_bytes(B, V).
 * sat_scst_weights: len[b] = min(kept[b] + 1, T) with kept[b] as sat_kept_tokens defines it (the <end> token itself is trained);
 *   M = sum_b len[b] (an integer sum: exact in any order), or *denom when denom != NULL (a global token count);
 *   w[t*B + b] = (float)((reward[b] - baseline[b]) / M) for t < len[b], +0.0f after -- f64 arithmetic, rounded once.  reward,
 *   baseline (NULL: 0), denom: device f64.  Outputs w f32 [T*B], len i32 [B], m_out f64 [1].  One launch, one workgroup.
 * sat_ce_rows_weighted: sat_ce_rows with the device weight w[n] of packed row n = t*B + b in place of inv_denom and the target
 *   ids[b*ids_stride + t] (N a multiple of B, ids_stride >= N / B): row_loss[n] = lse_n - logit_n[target]; loss_out[0] (NULL: no
 *   sum) = sum_n w[n] * row_loss[n] in a fixed order; write_grad: logits are overwritten IN PLACE with w[n] * (softmax - onehot).
 *   A row with w[n] == 0 gets an all-zero gradient row and adds exactly 0 to the loss whatever its logits hold (a non-finite
 *   logit of a masked row never becomes NaN * 0; its row_loss[n] is then non-finite).  Pad columns [V, ldl) are left alone. */
int64_t sat_rollout_decoder_fwd_ws_bytes(int B, int V);
int sat_rollout_decoder_fwd(const float* features /*[B,E]*/, const float* embed /*[V,E]*/, int B, int steps, int E, int V,
                            const float* const* lstm_w /*[host]*/, int num_layers, int H, const float* lin_w, const float* lin_b,
                            float* const* tapes /*[host]*/, float* X, float* logits, int64_t ldl, uint64_t seed, int rank, int64_t* ids,
                            int64_t ids_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream);
int sat_scst_weights(const int64_t* ids, int64_t stride, int B, int T, int64_t end_id, const double* reward /*[B]*/,
                     const double* baseline /*[B] or NULL*/, const double* denom /*[1] or NULL*/, float* w /*[T*B]*/,
                     int32_t* len /*[B]*/, double* m_out /*[1]*/, sat_stream_t stream);
int sat_ce_rows_weighted(float* logits /*[N,ldl]*/, int64_t ldl, const int64_t* ids, int64_t ids_stride, int B, int N, int V,
                         const float* w /*[N]*/, int write_grad, float* row_loss /*[N]*/, float* loss_out /*[1] or NULL*/,
                         sat_stream_t stream);
/* Self-critical training with S sampled captions per image and a leave-one-out baseline (Luo 2020, arXiv:2003.09971; added within
 * ABI 18).  Rows are image-major: R = B*S rows, row r = b*S + s is sample s of image b, packed logits row n = t*R + r (the rollouts
 * run on R rows; nothing in them changes).
 * sat_scst_weights_group: len[r] and M exactly as sat_scst_weights over the R rows (len[r] = min(kept[r] + 1, T); M = the integer
 *   sum of all R lengths, or *denom when denom != NULL).
 *   mode 0 (a baseline per image): advantage[r] = reward[r] - (baseline_img ? baseline_img[r / S] : 0.0); baseline_out[r] is that
 *     baseline.  With S == 1 this is sat_scst_weights, bit for bit.
 *   mode 1 (leave-one-out): advantage[r] = (sum over s' = 0..S-1, s' != s, ascending, starting from 0.0, of
 *     (reward[r] - reward[b*S + s'])) / (S - 1).  The sum is of DIFFERENCES on purpose: S identical rewards give exactly +0.0,
 *     which reward - mean(others) does not (0.1 + 0.1 + 0.1 = 0.30000000000000004).  baseline_out[r] = (sum over s' != s,
 *     ascending, from 0.0, of reward[b*S + s']) / (S - 1), for logging only.
 *   w[t*R + r] = (float)(advantage[r] / M) for t < len[r], +0.0f after.  All arithmetic is f64, rounded once, in a fixed order: the
 *   bits are the same in every call and for every B.  Plain vector stores, no atomics; one launch of one workgroup whose threads
 *   stride over the rows, so any R (and any B) is served.  reward f64 [B*S], baseline_img f64 [B] or NULL, denom f64 [1] or NULL:
 *   device.  Outputs w f32 [T*B*S], len i32 [B*S], m_out f64 [1], advantage f64 [B*S], baseline_out f64 [B*S] or NULL.
 *   SAT_ERR_ARG before anything is enqueued: a NULL required pointer; B, S or T < 1; mode outside {0, 1}; mode 1 with S < 2 or
 *   with a non-NULL baseline_img; stride < T; B*S*T > INT_MAX.  SAT_ERR_UNSUPPORTED: S > 256.
 * sat_group_sum_rows: out[b][j] = (((in[b*S][j] + in[b*S+1][j]) + in[b*S+2][j]) + ...) in f32, ascending s, j < W; S == 1 is a copy.
 *   The backward of "one image's features feed S rows", here so that the autograd path and the fused step give the same bits.  A
 *   16-byte path runs on the first W - W % 4 columns where both strides are multiples of 4 and both pointers 16-byte aligned; a
 *   scalar path takes the other columns, or all of them.  SAT_ERR_ARG: NULL pointers, B, S or W < 1, ld_in < W, ld_out < W, or
 *   `in` and `out` overlapping. */
int sat_scst_weights_group(const int64_t* ids, int64_t stride, int B, int S, int T, int64_t end_id, const double* reward /*[B*S]*/,
                           const double* baseline_img /*[B] or NULL*/, int mode, const double* denom /*[1] or NULL*/,
                           float* w /*[T*B*S]*/, int32_t* len /*[B*S]*/, double* m_out /*[1]*/, double* advantage /*[B*S]*/,
                           double* baseline_out /*[B*S] or NULL*/, sat_stream_t stream);
int sat_group_sum_rows(const float* in /*[B*S][ld_in]*/, int64_t ld_in, int B, int S, int64_t W, float* out /*[B][ld_out]*/,
                       int64_t ld_out, sat_stream_t stream);
/* The rollout of the Show-Attend-Tell decoder (added within ABI 18): the training-form recurrence of model2.py:38-85 for all B rows
 * over all `steps` steps as ONE call, no host synchronisation -- sat_ss_attend_fwd's loop (the same five launches per step: weight_hh
 * projection from h_{t-1} with h_{-1} = h0, attention with its context written into X's context half, LSTMCell, output layer, vocab
 * projection with exact-f32 logits stored) with batch_sizes = [B] * steps, packed row n = t*B + b.  The embedding half of step 0 is
 * embed[start_id], of step t >= 1 embed[ids[b][t-1]].
 *   greedy == 0: ids[b][t] = s(b, t) drawn from step t's own logits with sat_rollout_decoder_fwd's convention exactly (counter
 *     (v >> 2, b, t, 2*rank), word v & 3; every row draws at every step, no mask draw, no teacher).
 *   greedy != 0: ids[b][t] = the first maximal column of step t's logits (sat_vocab_argmax's rule); seed and rank are ignored.  This
 *     is the greedy decode of the policy the draws come from (h0 / c0 from init_lstm, every step its own context), not model2.py's
 *     `sample` (zero state, lagging context): the baseline of a self-critical loss.
 * Rows keep running behind <end>; sat_scst_weights masks them.  feats, ctx_enc, h0, c0, w (SAT_SSA_* order), tapes as for
 * sat_ss_attend_fwd; prefix: DEVICE int32 [steps+1], prefix[t] = t*B (as for sat_pack_tokens).  Outputs: ids [B][ids_stride >=
 * steps]; fed [B][fed_stride >= steps] = [start_id | ids[:, :steps-1]], the tokens fed; toks [steps*B], fed packed; logits [steps*B,
 * ldl] (ldl % 4 == 0, pad columns untouched); the eight SAT_SSA_* tapes holding exactly what the teacher-forced forward on `fed`
 * leaves in them (Zin included; Z as sat_ss_attend_fwd leaves it, the per-step output-layer rows), so that forward's backward
 * applies unchanged.  ids and fed must not overlap.
 * SAT_ERR_ARG (null pointers; steps < 1; start_id outside [0, V); B*steps > INT_MAX; the size rules of sat_ss_attend_fwd),
 * SAT_ERR_UNSUPPORTED and SAT_ERR_WORKSPACE come back before anything is enqueued.  workspace:
 * sat_rollout_attend_fwd_ws_bytes(B, P, C, E, H, V) = sat_ss_attend_fwd's layout with the draw region max(sat_ss_decoder_fwd_ws_bytes,
 * sat_vocab_argmax_ws_bytes)(B, V); 0 for non-positive sizes. */
int64_t sat_rollout_attend_fwd_ws_bytes(int B, int P, int C, int E, int H, int V);
int sat_rollout_attend_fwd(const float* feats, const float* ctx_enc, const float* h0, const float* c0,
                           const int32_t* prefix /*[steps+1] device*/, int B, int steps, int P, int C, int E, int H, int V,
                           const float* const* w /*[host]*/, float* const* tapes /*[host]*/, int64_t* toks, float* logits, int64_t ldl,
                           int greedy, int64_t start_id, uint64_t seed, int rank, int64_t* ids, int64_t ids_stride, int64_t* fed,
                           int64_t fed_stride, float* workspace, int64_t ws_bytes, sat_stream_t stream);
/* Label smoothing for the cross entropy (added within ABI 18): torch's F.cross_entropy(..., label_smoothing = smoothing).  For a row
 * x[0..V) with target t (clamped into [0, V-1] as sat_ce_rows clamps it), m = max(x), s = sum exp(x - m), lse = m + log s:
 *     row_nll[n]  = lse - x[t]
 *     row_loss[n] = (1 - smoothing) * row_nll[n] + smoothing * (log s - mean(x - m))      (= (smoothing / V) * sum_v (lse - x[v]))
 *     g[n][v]     = (softmax(x)[v] - (1 - smoothing) * [v == t] - smoothing / V) * inv_denom
 *     loss_out[0] = inv_denom * sum_n row_loss[n],  nll_out[0] = inv_denom * sum_n row_nll[n]      (sat_ce_rows's fixed order)
 * The smoothing term is formed from values centred on the row maximum.  Non-finite logits are outside the contract.
 * sat_ce_rows_ls: one workgroup per row, one read of the logits and one write of the gradient (sat_ce_rows's register path for
 *   V <= 12288 with 16-byte aligned bases and ldl % 4 == 0 -- and, with a gradient, ldg % 4 == 0 --, its strided path otherwise).
 *   grad: f32 [N, ldg] (ldg >= V), or NULL for none; grad == logits with ldg == ldl is sat_ce_rows's in-place form, any other grad
 *   must not overlap the logits, which are then left untouched.  Pad columns [V, ldg) are left alone.  row_nll, loss_out, nll_out may
 *   be NULL (nll_out needs row_nll).  smoothing == 0: row_loss, loss_out and grad are bit for bit sat_ce_rows's.
 *   SAT_ERR_ARG before any launch: NULL logits / targets / row_loss, smoothing outside [0, 1) or NaN, N < 1, V < 1, ldl < V,
 *   ldg < V with a gradient, nll_out without row_nll.
 * sat_vocab_ce_fwd_bf16_ls: sat_vocab_ce_fwd_bf16 (same workspace, size query and shape limits; logits written as f32 and not
 *   modified) with the smoothed loss in row_loss / loss_out, the plain one in row_nll / nll_out (either may be NULL, nll_out needs
 *   row_nll) and the smoothed gradient rounded once to bf16 where sat_vocab_ce_bwd_bf16 expects it, pad columns zero.
 *   smoothing == 0: the same bits as sat_vocab_ce_fwd_bf16.  smoothing outside [0, 1) or NaN: SAT_ERR_ARG. */
int sat_ce_rows_ls(const float* logits /*[N,ldl]*/, int64_t ldl, const int64_t* targets /*[N]*/, int N, int V, float inv_denom,
                   float smoothing, float* grad /*[N,ldg], NULL, or == logits*/, int64_t ldg, float* row_loss /*[N]*/,
                   float* row_nll /*[N] or NULL*/, float* loss_out /*[1] or NULL*/, float* nll_out /*[1] or NULL*/, sat_stream_t stream);
int sat_vocab_ce_fwd_bf16_ls(const float* Hs /*[N,H]*/, const float* w /*[V,H]*/, const float* b /*[V]*/, const int64_t* targets /*[N]*/,
                             int N, int H, int V, float inv_denom, float smoothing, float* logits /*[N,ldl]*/, int64_t ldl,
                             float* row_loss /*[N]*/, float* row_nll /*[N] or NULL*/, float* loss_out /*[1] or NULL*/,
                             float* nll_out /*[1] or NULL*/, void* workspace /*256-byte aligned*/, int64_t ws_bytes, sat_stream_t stream);
/* Token-level unlikelihood training (added within ABI 18; Welleck et al. 2019, arXiv:1908.04319, fairseq's
 * candidate_penalty_cross_entropy): every target row also pays for the probability it gives to the tokens already emitted in its own
 * caption.  Packed rows are time-major: row n = prefix[t] + b is step t of sequence b (b < prefix[t+1] - prefix[t]); prefix is the
 * DEVICE int32 [T+1] of pack_padded_sequence's batch sizes (prefix[0] = 0, prefix[T] = N, batch sizes non-increasing -- trusted).
 * For row n with logits x[0..V), target y (clamped as sat_ce_rows clamps it), p = softmax(x), and m, s, lse, nll and the smoothing
 * term exactly as sat_ce_rows_ls defines them:
 *     C_n         = { targets[prefix[s] + b] : 0 <= s < t } \ { y }      a SET: ids clamped the same way, a repeated id counts once
 *     q_c         = 1 - p_c
 *     row_ul[n]   = sum_{c in C_n} -log(max(q_c, 1e-5))
 *     w_c         = q_c > 1e-5 ? p_c / q_c : 0                           (torch's clamp(min=1e-5): gradient 0 where it clamps)
 *     W_n         = sum_{c in C_n} w_c
 *     row_loss[n] = (sat_ce_rows_ls's row_loss[n]) + alpha * row_ul[n]
 *     g[n][v]     = (p_v * (1 - alpha * W_n) - (1 - smoothing) * [v == y] - smoothing / V + (v in C_n ? alpha * w_v : 0)) * inv_denom
 *     loss_out[0] = inv_denom * sum_n row_loss[n],  nll_out[0] = inv_denom * sum_n row_nll[n],  ul_out[0] = inv_denom * sum_n row_ul[n]
 *                   (ul_out is NOT weighted by alpha; all three in sat_ce_rows's fixed order)
 * Both sums over C_n run over the set's representatives in ascending order of first occurrence s, so a row's outputs depend only on
 * its own logits and its own prefix: the same bits in any batch and in every replay.  Rows of step 0 have no candidates.
 * alpha == 0: row_loss, row_nll, loss_out, nll_out and the gradient are bit for bit sat_ce_rows_ls's / sat_vocab_ce_fwd_bf16_ls's
 * (and, with smoothing == 0 too, sat_ce_rows's / sat_vocab_ce_fwd_bf16's), row_ul is 0.
 * sat_ce_rows_ul: sat_ce_rows_ls's two paths, grad forms (out of place, NULL, or == logits in place) and pad rule; one read of the
 *   logits and one write of the gradient.  row_nll, row_ul, loss_out, nll_out, ul_out may be NULL.
 *   SAT_ERR_ARG before any launch: everything sat_ce_rows_ls rejects, NULL prefix, T < 1, alpha < 0 or NaN, ul_out without row_ul.
 *   SAT_ERR_UNSUPPORTED: T > 64.
 * sat_vocab_ce_fwd_bf16_ul: sat_vocab_ce_fwd_bf16_ls (same workspace, size query and shape limits) with the term above; the gradient
 *   is rounded once to bf16 where sat_vocab_ce_bwd_bf16 expects it, pad columns zero.  The same argument errors. */
int sat_ce_rows_ul(const float* logits /*[N,ldl]*/, int64_t ldl, const int64_t* targets /*[N] packed*/,
                   const int32_t* prefix /*[T+1] device*/, int T, int N, int V, float inv_denom, float smoothing, float alpha,
                   float* grad /*[N,ldg], NULL, or == logits*/, int64_t ldg, float* row_loss /*[N]*/, float* row_nll /*[N] or NULL*/,
                   float* row_ul /*[N] or NULL*/, float* loss_out /*[1] or NULL*/, float* nll_out /*[1] or NULL*/,
                   float* ul_out /*[1] or NULL*/, sat_stream_t stream);
int sat_vocab_ce_fwd_bf16_ul(const float* Hs /*[N,H]*/, const float* w /*[V,H]*/, const float* b /*[V]*/,
                             const int64_t* targets /*[N] packed*/, const int32_t* prefix /*[T+1] device*/, int T, int N, int H, int V,
                             float inv_denom, float smoothing, float alpha, float* logits /*[N,ldl]*/, int64_t ldl,
                             float* row_loss /*[N]*/, float* row_nll /*[N] or NULL*/, float* row_ul /*[N] or NULL*/,
                             float* loss_out /*[1] or NULL*/, float* nll_out /*[1] or NULL*/, float* ul_out /*[1] or NULL*/,
                             void* workspace /*256-byte aligned*/, int64_t ws_bytes, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * clip_gradient (train.py:88-91) + optim.Adam step (train.py:56,146) over one flat buffer.
 * clip <= 0 disables the clamp.  step is the 1-based Adam step count.
 */
int sat_clamp_adam_step(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1,
                        float beta2, float eps, float clip, int step, sat_stream_t stream);
/* The same update behind a device-side guard: `skip_if_nonzero` (device f32 word, may be NULL) is read by the kernel, and a
 * non-zero value drops the WHOLE update -- p, g, m, v stay bit for bit what they were.  The fused trainer aims it at the step's
 * fault slot (below), so a step whose persistent LSTM recurrence gave up never reaches the parameters. */
int sat_clamp_adam_step_guarded(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1,
                                float beta2, float eps, float clip, int step, const float* skip_if_nonzero,
                                sat_stream_t stream);
/* One step's fault flag: *slot = *sticky = (*sticky != 0 || any of the n_words (<= 8) u32 device status words != 0) ? 1.0f : 0.0f
 * (`status_words`: HOST array of device pointers -- sat_lstm_fwd_status_offset / sat_lstm_bwd_status_offset words of the
 * workspaces this step's calls ran with; `sticky`: device f32 the caller keeps across steps and clears once it has seen the
 * fault, may be NULL).  The trainer puts `slot` into the flat gradient buffer's trailing floats, so that in data-parallel
 * training the flag rides the last bucket's all-reduce(sum) and EVERY rank skips the update of a step one rank lost. */
int sat_step_fault_flag(const void* const* status_words, int n_words, float* sticky, float* slot, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Global-norm clipping (torch.nn.utils.clip_grad_norm_) + decoupled weight decay (torch.optim.AdamW) over one flat buffer
 * (sat_optim.hip).  No atomics; every sum in one fixed order, so the results are bitwise reproducible.
 * sat_grad_sumsq: one read of g [n] (16-byte aligned).  Writes sat_grad_sumsq_partials(n) pairs {double sumsq, double nonfinite}
 *   -- one per workgroup; the count depends on n only, at most 768 -- at pair index partial_offset of `partials` (16-byte aligned,
 *   room for partial_capacity pairs), so several segments of a buffer fill one array.  sumsq: f64 sum of the f64 squares of the
 *   elements, CLAMPED to [-clip, clip] first when clip > 0 (the gradient Adam will use); nonfinite: the count of RAW elements that
 *   are Inf or NaN.  sat_grad_sumsq_ws_bytes(n): 16 bytes per pair.
 *   SAT_ERR_ARG before any launch: NULL or misaligned g / partials, n < 1, NaN clip, partial_offset < 0, pairs beyond the capacity.
 * sat_adamw_step: sat_clamp_adam_step_guarded with, per element: clamp (clip > 0), g *= coef, the scaled gradient written back,
 *   p *= 1 - lr * weight_decay unless the element lies in an exempt range, then the same Adam arithmetic.
 *   partials != NULL (n_partials pairs, all of them summed): total = sum of sumsq, norm = sqrt(total),
 *   coef = min(max_norm / (norm + 1e-6), 1) -- clip_grad_norm_'s clip_coef_clamped; max_norm = +inf only measures.  When any
 *   nonfinite count is non-zero or total is not finite the WHOLE update is dropped: p, g, m, v stay bit for bit what they were.
 *   norm_out (2 doubles, may be NULL) receives {norm, sum of the nonfinite counts} either way (not when the skip word dropped the
 *   step).  partials == NULL: no norm, coef = 1, no non-finite check, norm_out untouched.  coef == 1, weight_decay == 0: the
 *   bits of sat_clamp_adam_step_guarded.
 *   exempt: HOST array of n_exempt (<= 32) pairs [lo, hi) of element offsets, sorted and disjoint, every lo a multiple of 4 (the
 *   slices of a flat buffer start on multiples of 4: a 16-byte chunk belongs to one parameter and is exempt as a whole when its
 *   first element lies in a range -- what follows a slice up to the next multiple of 4 is padding; the n % 4 tail elements are
 *   looked up one by one).
 *   SAT_ERR_ARG before any launch: NULL or misaligned buffers, n < 1, step < 1, weight_decay < 0 or NaN, more than 32 ranges, an
 *   unsorted, overlapping or empty range, a lo that is negative or no multiple of 4, and with partials: max_norm <= 0 or NaN,
 *   n_partials < 1. */
int sat_grad_sumsq_partials(int64_t n);
int64_t sat_grad_sumsq_ws_bytes(int64_t n);
int sat_grad_sumsq(const float* g, int64_t n, float clip, double* partials, int partial_offset, int partial_capacity,
                   sat_stream_t stream);
int sat_adamw_step(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float clip,
                   int step, float weight_decay, const int64_t* exempt, int n_exempt, float max_norm, const double* partials,
                   int n_partials, double* norm_out, const float* skip_if_nonzero, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exponential moving average of the parameters (Polyak averaging; added within ABI 18; sat_optim.hip), one launch behind the
 * update on the same stream, and the exchange that puts the average into the model and takes it out again.
 * sat_ema_update: ema[i] = fma(w, p[i] - ema[i], ema[i]) with w = (float)(1.0 - (double)decay) formed on the host, the difference
 *   rounded to f32, then ONE fused multiply-add: two roundings per element, the same in the 16-byte loop and in the n % 4 tail,
 *   so an element's bits do not depend on n, the grid or the pointer offset.  12 B per parameter.
 *   The whole launch does nothing -- ema keeps every bit -- when the update in front of it was dropped:
 *     skip_if_nonzero (device f32 word, may be NULL) is non-zero: the step's fault word, which sat_clamp_adam_step_guarded and
 *       sat_adamw_step read and neither of them writes;
 *     norm_state (2 device doubles, may be NULL) has norm_state[1] > 0 or a norm_state[0] that is not finite: the
 *       {norm, non-finite elements} pair sat_adamw_step wrote to norm_out in front of this launch.
 *   SAT_ERR_ARG before any launch: NULL ema / p, n < 1, ema or p not 16-byte aligned, norm_state not 8-byte aligned, decay NaN or
 *   outside (0, 1).  ema and p must not overlap.
 * sat_swap_f32: a[i] <-> b[i], exact, no third buffer.  SAT_ERR_ARG before any launch: NULL or misaligned (16 bytes) a / b,
 *   n < 1, overlapping ranges (a == b included).
 * Both: 256 threads, 16-byte accesses, a grid that depends on n only (at most 768 workgroups), no atomics, no LDS. */
int sat_ema_update(float* ema, const float* p, int64_t n, float decay, const float* skip_if_nonzero, const double* norm_state,
                   sat_stream_t stream);
int sat_swap_f32(float* a, float* b, int64_t n, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient accumulation (added within ABI 18; sat_optim.hip): one finished backward folded into a second flat buffer, so that K
 * micro-batches (or a cross-entropy and a self-critical backward) make ONE update.  acc and g hold n + 2 floats each in the layout
 * of the flat gradient buffer: n gradients, the loss slot, the step's fault word.
 *   elements i <= n (gradients and the loss slot):
 *     first != 0: acc[i] = weight * g[i]              (one rounding; the old acc[i] is never read: stale NaN cannot leak)
 *     first == 0: acc[i] = fma(weight, g[i], acc[i])  (one rounding)
 *   element n + 1 (the fault word): acc = ((first ? 0 : acc != 0) || g != 0) ? 1.0f : 0.0f -- a micro-batch whose fault word is
 *     set poisons the whole accumulated update, which sat_clamp_adam_step_guarded / sat_adamw_step / sat_ema_update then drop
 *     when handed acc + n + 1 as their skip word.
 *   Contracts: weight == 1 gives exactly the f32 sum in call order; first with weight == 1 gives exactly a copy; the result is a
 *   function of (acc, g, weight, first) only -- the same arithmetic in the 16-byte loop and in the tail, no atomics, nothing
 *   depends on the grid: the same bits in every launch shape.  Inf / NaN take no special path: they go through the fma, and
 *   sat_adamw_step's count drops the update when a norm is set.
 *   SAT_ERR_ARG before any launch: NULL acc / g, n < 0, acc or g not 16-byte aligned, weight not finite, overlapping ranges.
 *   256 threads, 16-byte accesses, a grid that depends on n only (at most 768 workgroups), no LDS.  12 B per parameter (8 with
 *   first). */
int sat_grad_accumulate(float* acc, const float* g, int64_t n, float weight, int first, sat_stream_t stream);

/* column sums: out[c] = sum_r x[r*ld + c]  (bias gradients) */
int sat_colsum_f32(const float* x, int64_t ld, int rows, int cols, float* out, sat_stream_t stream);
/* f32 -> bf16 / bf16 -> f32 casts (weight shadow copies) */
int sat_cast_f32_bf16(const float* in, void* out, int64_t n, sat_stream_t stream);
int sat_cast_bf16_f32(const void* in, float* out, int64_t n, sat_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Scoring given captions (added within ABI 18): the model's log-probability of captions somebody hands it -- per-caption
 * likelihood, likelihood reranking, image-sentence ranking by p(S|I) (Vinyals et al. 2015, section 4.3.5).
 *
 * sat_vocab_logp: the vocab projection (models.py:53), log-softmax and the pick of one column per row, WITHOUT the [N, V] logits:
 *   tok_logp[n] = (Hs[n] . w[t_n] + b[t_n]) - logsumexp_v (Hs[n] . w[v] + b[v]),  t_n = targets[n] clamped into [0, V-1] (as
 *   sat_ce_rows clamps it);  lse[n] (nullable) = that logsumexp.  Hs rows have pitch lda >= H floats.
 *   Shapes sat_gemm_f32x3 takes (sat_gemm_f32x3_packed_bytes(V, H) > 0) with V % 4 == 0: sat_gemm_f32x3's tile loop with an
 *   epilogue that leaves a (max, sum exp) pair per row and 128-column tile (8 bytes where the logits would be 512), joined per
 *   row in ascending tile order in f64; w_packed = sat_gemm_f32x3_pack's copy of w, or NULL (the call then packs w into the
 *   workspace itself).  Every other shape: chunks of rows through sat_vocab_logits_fwd's GEMM into a bounded scratch, then
 *   sat_ce_rows(write_grad = 0).  No atomics: the same input gives the same bits, and a row gives the same bits in any batch.
 *   workspace: sat_vocab_logp_ws_bytes(N, H, V) bytes (never N * V elements; the general path works in any workspace that holds
 *   one row of logits and takes as many rows per chunk as fit -- sat_vocab_logp_ws_bytes_rows names the chunk height, for tests).
 *   SAT_ERR_ARG before any launch: NULL pointers, N < 1, lda < H, lda or H no multiple of 4, Hs / w / workspace not 16-byte
 *   aligned, a workspace too small.
 * sat_caption_logp_sum: packed rows (time-major, rows of step t at [prefix[t], prefix[t+1]), row r present at step t while
 *   r < prefix[t+1] - prefix[t]) to captions: logp[r] = f64 sum over t ascending (one thread per caption), len[r] = its steps,
 *   tok_out[r][t] (nullable, pitch tok_stride >= T) = the token's log-probability, +0.0f beyond the caption's length.
 * sat_score_captions: the decoder (models.py:47-53) teacher-forced on R rows, row r = (image row_image[r], caption
 *   row_caption[r]) -- paired scoring and the B_img x C cross matrix are both this call.  Rows are ordered by caption length,
 *   descending: batch_sizes [T] HOST, non-increasing, batch_sizes[0] = R, sum N; prefix [T+1] DEVICE, its running sum.  Step 0
 *   feeds features and runs on the B_img image rows only (the state is then gathered to the rows); step t >= 1 feeds
 *   embed[captions[c][t-1]] to the live rows through sat_lstm_step; step t is scored against captions[c][t] -- the rows
 *   `decoder(features, captions, lengths)` is trained on against pack_padded_sequence(captions, lengths).  The top layer's h
 *   of every live (step, row) goes through ONE sat_vocab_logp (weights packed once per call), then sat_caption_logp_sum.
 *   captions [C][cap_stride] i64 (ids clamped for memory safety only: range-check them with sat_validate_ids); lstm_w: HOST
 *   array of 4 * num_layers device pointers (w_ih, w_hh, b_ih, b_hh per layer), num_layers <= 8; E, H multiples of 4;
 *   workspace 256-byte aligned, sat_score_captions_ws_bytes(...) bytes -- about N * (4 H + 8 ceil(V / 128)) plus state and
 *   the packed weights.  SAT_ERR_ARG before any launch as above, and for batch_sizes that do not describe R rows / N steps. */
int64_t sat_vocab_logp_ws_bytes(int N, int H, int V);
int64_t sat_vocab_logp_ws_bytes_rows(int N, int H, int V, int chunk_rows);
int sat_vocab_logp(const float* Hs /*[N,lda]*/, int64_t lda, const float* w /*[V,H]*/, const void* w_packed, const float* b /*[V]*/,
                   const int64_t* targets /*[N]*/, int N, int H, int V, float* tok_logp /*[N]*/, float* lse /*[N] or NULL*/,
                   void* workspace, int64_t ws_bytes, sat_stream_t stream);
int sat_caption_logp_sum(const float* tok_logp /*[N]*/, const int32_t* prefix /*[T+1] device*/, int T, int R, double* logp /*[R]*/,
                         int32_t* len /*[R]*/, float* tok_out /*[R][tok_stride] or NULL*/, int64_t tok_stride, sat_stream_t stream);
int64_t sat_score_captions_ws_bytes(int B_img, int R, int N, int E, int H, int V, int num_layers);
int sat_score_captions(const float* features /*[B_img,E]*/, const float* embed /*[V,E]*/, const float* const* lstm_w /*[host]*/,
                       int num_layers, const float* lin_w /*[V,H]*/, const float* lin_b /*[V]*/, const int64_t* captions, int64_t cap_stride,
                       int C, const int32_t* row_image /*[R] device*/, const int32_t* row_caption /*[R] device*/,
                       const int32_t* batch_sizes /*[T] host*/, const int32_t* prefix /*[T+1] device*/, int T, int B_img, int R, int N,
                       int E, int H, int V, double* logp /*[R]*/, int32_t* len /*[R]*/, float* tok_out /*[R][tok_stride] or NULL*/,
                       int64_t tok_stride, void* workspace, int64_t ws_bytes, sat_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
