// Dropout (inverted: kept activations are scaled by 1 / (1 - p)) on a dense f32 [rows, cols] tape, forward and backward: the mask is
// a pure function of (seed, rank, site, row, column), so the backward REGENERATES it from the same arguments on the gradient and
// no mask tensor is ever stored.  Both decoders apply it to the packed activations that feed their word classifier (Vinyals et
// al. 2015; Xu et al. 2015, section 4.2.1 -- the reference builds `nn.Dropout(p=0.5)` there, model2.py:34, and never calls it), and
// the Show-and-Tell decoder between stacked LSTM layers (nn.LSTM(dropout=)).
//
// Randomness: Philox4x32-10, key (seed lo, seed hi), counter (j >> 2, r, 0x80000000 | site, 2*rank), word j & 3 for element (r, j):
// one evaluation serves four neighbouring columns.  The high bit of counter word 2 is never set by the scheduled-sampling, rollout
// and stochastic-decode draws (they put the step index there), so a seed used twice cannot correlate a mask with a token draw.
// keep(r, j) = (word >> 8) >= thr with thr = lrint(p * 2^24) computed once on the host: an integer comparison, identical off the
// device.  A streaming kernel: 8 bytes of traffic per element, no LDS, no scratch.
#include "sat_internal.h"

#include <cmath>

namespace {

// One thread per (row, group of 4 columns).  VEC: both row bases are 16-byte aligned (pointers and leading dimensions), so a whole
// group moves as one 16-byte load and store; the last group of a row with cols % 4 != 0, and everything when !VEC, goes element
// by element.  In place (y == x) is safe: a thread reads its group before it writes it and no other thread touches it.
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, long ldx, float* y, long ldy,
                                                      long total, int ngroups, int cols, unsigned thr, float scale, unsigned key0,
                                                      unsigned key1, unsigned ctr2, unsigned ctr3) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long r = i / ngroups;
        const int q = (int)(i - r * ngroups);
        const u32x4 w = sat_philox4x32_10((unsigned)q, (unsigned)r, ctr2, ctr3, key0, key1);
        const int j0 = q * 4;
        const float* xr = x + r * ldx + j0;
        float* yr = y + r * ldy + j0;
        if (VEC && j0 + 4 <= cols) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(xr);
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (w[k] >> 8) >= thr ? v[k] * scale : 0.0f;
            *reinterpret_cast<f32x4*>(yr) = o;
        } else {
            const int n = cols - j0 < 4 ? cols - j0 : 4;
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = k < n ? xr[k] : 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) yr[k] = (w[k] >> 8) >= thr ? v[k] * scale : 0.0f;
        }
    }
}

}  // namespace

extern "C" int sat_dropout_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int cols, float p, uint64_t seed,
                               int rank, int site, sat_stream_t stream) {
    if (!(p >= 0.0f && p < 1.0f)) return SAT_ERR_ARG;                         // (NaN and the infinities fail the comparison)
    if (rows < 0 || cols < 0 || ldx < cols || ldy < cols || site < 0 || rank < 0) return SAT_ERR_ARG;
    if (rows == 0 || cols == 0) return SAT_OK;
    if (!x || !y) return SAT_ERR_ARG;
    if (p == 0.0f && x == y) return SAT_OK;                                   // an exact copy onto itself
    const unsigned thr = (unsigned)lrint((double)p * 16777216.0);
    const float scale = (float)(1.0 / (1.0 - (double)p));
    const int ngroups = sat_cdiv(cols, 4);
    const long total = (long)rows * ngroups;
    const bool vec = cols >= 4 && !(((uintptr_t)x | (uintptr_t)y) & 15) && !((ldx | ldy) & 3);
    const unsigned grid = (unsigned)(total + 255 < (1l << 28) ? (total + 255) / 256 : (1l << 20));
    hipStream_t s = (hipStream_t)stream;
    const unsigned key0 = (unsigned)(seed & 0xffffffffu), key1 = (unsigned)(seed >> 32);
    const unsigned ctr2 = 0x80000000u | (unsigned)site, ctr3 = 2u * (unsigned)rank;
    if (vec)
        hipLaunchKernelGGL(dropout_kernel<true>, dim3(grid), dim3(256), 0, s, x, (long)ldx, y, (long)ldy, total, ngroups, cols, thr, scale,
                           key0, key1, ctr2, ctr3);
    else
        hipLaunchKernelGGL(dropout_kernel<false>, dim3(grid), dim3(256), 0, s, x, (long)ldx, y, (long)ldy, total, ngroups, cols, thr,
                           scale, key0, key1, ctr2, ctr3);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}
