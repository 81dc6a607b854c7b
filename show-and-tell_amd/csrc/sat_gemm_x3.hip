// f32 GEMM on the bf16 matrix pipe by a THREE-WAY SPLIT of both operands (beam decode: the vocab projection `self.linear(hiddens)`,
// models.py:53 / :63, of 320 hypothesis rows per step -- half of the decode step's time on the exact-f32 pipe).
//
//   C[M,N] = A[M,K] * W[N,K]^T + bias,   A, W, C f32
//
// Every f32 operand x is written as hi + mid + lo with three bf16 terms (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); the
// two subtractions are exact in f32, so |x - hi - mid - lo| <= 2^-25 |x|).  A product of two bf16 numbers is exact in f32, and
// v_mfma_f32_32x32x16_bf16 accumulates in f32, so with the six products of weight >= 2^-16
//     hi*hi  +  (hi*mid + mid*hi + hi*lo + lo*hi + mid*mid)
// the result carries the accuracy of an f32 GEMM (the dropped products are below 2^-24 of |a||b|) at 6 / 16 of the f32 pipe's cost
// per product: the bf16 pipe is 16 x the f32 one.  hi*hi and the five corrections go to SEPARATE accumulators (added once, at the end),
// so that the small terms are not rounded away against the large sum.  Not the bit pattern of the f32-pipe GEMM (another summation
// order, like any two f32 GEMMs), hence used where ids / scores are checked against an oracle to a tolerance: the beam decode's
// projection (tests/test_gpu_gemm_x3.py: against f64, relative to sum |a||b|; tests/test_gpu_parity.py: decode ids bit-exact).
//
// Kernel = conv_aw_kernel's structure (sat_conv_aw.inc): 128 x 128 tiles, four waves, wave w owns 32 columns x 128 rows; the WEIGHTS are
// split and put in MFMA fragment order ONCE per decode call (sat_gemm_f32x3_pack: 3 x [N][K] bf16) and stream straight into registers
// (12 KB per wave and K-step of 64, two K-steps ahead); the activations go global (f32) -> registers -> split -> three XOR-swizzled LDS
// row images per K-step (two buffers, one raw barrier per K-step); 96 MFMAs per wave and K-step.  Column tiles are the slow index of the
// XCD-aware tile map: the row tiles that share a weight slice run on one XCD and hit in its L2.  The kernel template lives in
// sat_gemm_x3_tile.h: sat_vocab_logp (sat_score.hip) instantiates the same K loop with another epilogue.
#include "sat_internal.h"
#include "sat_gemm_x3_tile.h"
#include <stdlib.h>

namespace {

// W f32 [N][K] -> packed[nb][cb][s][ks][lane = h*32 + r][e] = split_s(W[32 nb + r][64 cb + 16 ks + 8 h + e]); columns >= N are zeros
__global__ __launch_bounds__(256) void x3_pack_kernel(const float* __restrict__ W, u32x4* __restrict__ P, int N, int K, long total) {
    const int ncb = K >> 6;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int lane = (int)(idx & 63), ks = (int)((idx >> 6) & 3);
        const long blk = idx >> 8;
        const int cb = (int)(blk % ncb);
        const long nb = blk / ncb;
        const long col = 32 * nb + (lane & 31);
        const int k0 = 64 * cb + 16 * ks + 8 * (lane >> 5);
        u32x4 hi = {0u, 0u, 0u, 0u}, mid = hi, lo = hi;
        if (col < N) {
            const f32x4 a = *(const f32x4*)(W + col * K + k0), b = *(const f32x4*)(W + col * K + k0 + 4);
            unsigned th, tm, tl;
            split2(a[0], a[1], th, tm, tl); hi[0] = th; mid[0] = tm; lo[0] = tl;
            split2(a[2], a[3], th, tm, tl); hi[1] = th; mid[1] = tm; lo[1] = tl;
            split2(b[0], b[1], th, tm, tl); hi[2] = th; mid[2] = tm; lo[2] = tl;
            split2(b[2], b[3], th, tm, tl); hi[3] = th; mid[3] = tm; lo[3] = tl;
        }
        u32x4* dst = P + ((blk * 3) * 4 + ks) * 64 + lane;      // split s: + s * 4 * 64 chunks
        dst[0] = hi;
        dst[4 * 64] = mid;
        dst[8 * 64] = lo;
    }
}

}  // namespace

// bytes of the split, fragment-ordered copy of W [N][K] (N rounded up to 128 columns); 0: shape not supported (K % 128, K >= 256)
extern "C" int64_t sat_gemm_f32x3_packed_bytes(int N, int K) {
    if (N <= 0 || K < 256 || (K & 127)) return 0;
    return (int64_t)sat_cdiv(N, 128) * 128 * K * 3 * 2;
}

extern "C" int sat_gemm_f32x3_pack(const float* W, int N, int K, void* packed, sat_stream_t stream) {
    if (!W || !packed || sat_gemm_f32x3_packed_bytes(N, K) == 0 || (((uintptr_t)W | (uintptr_t)packed) & 15)) return SAT_ERR_ARG;
    const long total = (long)sat_cdiv(N, 128) * 4 * (K >> 6) * 256;      // one thread per (32-column block, K-step, substep, lane)
    int grid = sat_cdiv(total, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(x3_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, W, (u32x4*)packed, N, K, total);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

// C[M][ldc] = A[M][lda] * W^T + bias with W given as its packed split copy; N % 4 == 0, ldc % 4 == 0, lda % 4 == 0, K % 128 == 0, K >= 256
extern "C" int sat_gemm_f32x3(const float* A, int64_t lda, const void* packed, const float* bias, float* C, int64_t ldc, int M, int N,
                              int K, sat_stream_t stream) {
    if (!A || !packed || !C || M <= 0 || N <= 0) return SAT_ERR_ARG;
    if (sat_gemm_f32x3_packed_bytes(N, K) == 0 || (N & 3) || (ldc & 3) || (lda & 3) || lda < K || ldc < N) return SAT_ERR_UNSUPPORTED;
    if ((((uintptr_t)A | (uintptr_t)packed | (uintptr_t)C) & 15) || (long)M * lda * 4 >= 0x7fffffe0L) return SAT_ERR_ARG;
    X3Args a = {};
    a.A = A; a.lda = lda; a.Bp = (const char*)packed; a.bias = bias; a.C = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K;
    a.a_bytes = (long)M * lda * 4;
    // the tile height of x3_tall_tiles, unless SAT_X3_BM (64 / 128, for A/B runs of this entry point) names one
    static const int bm_env = [] { const char* e = getenv("SAT_X3_BM"); return e ? atoi(e) : 0; }();
    const bool big = bm_env ? bm_env == 128 : x3_tall_tiles(M, sat_cdiv(N, 128));
    const dim3 block(256);
    if (big) {
        a.tiles_m = sat_cdiv(M, 128);
        hipLaunchKernelGGL(gemm_x3_kernel<128>, dim3(a.tiles_m * sat_cdiv(N, 128)), block, 0, (hipStream_t)stream, a);
    } else {
        a.tiles_m = sat_cdiv(M, 64);
        hipLaunchKernelGGL(gemm_x3_kernel<64>, dim3(a.tiles_m * sat_cdiv(N, 128)), block, 0, (hipStream_t)stream, a);
    }
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}
