// Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) and decoupled weight decay (torch.optim.AdamW) for the flat
// optimizer: two HBM-bound kernels over the flat f32 buffers, no atomics, every reduction in one fixed order (bitwise reproducible).
//
//   grad_sumsq_kernel : one streaming read of the gradient (4 B/param).  Each lane accumulates g*g in f64 -- the product of two f32
//                       values is exact in f64, so nothing overflows at |g| ~ 1e19 or underflows at 1e-30 -- and counts the RAW
//                       elements that are not finite.  With clip > 0 the value squared is the clamped one: the norm is that of the
//                       gradient Adam will use (the reference's clamp comes first).  Each workgroup writes ONE pair
//                       {double sumsq, double nonfinite}.  The grid is a function of n only, so the summation order is too.
//   adamw_kernel      : clamp_adam_kernel (sat_elementwise.hip; same 28 B/param, same guard word) with the gradient scaled by
//                       clip_coef_clamped and p *= 1 - lr * weight_decay in front of the Adam arithmetic, which is unchanged in
//                       form and order.  Every workgroup first re-sums the partial pairs (a few KB, L2-resident) in one order that
//                       is the same in every workgroup: all of them hold the same bits of `total` and `nonfinite` and so take the
//                       same decision with no second launch and no host read.  nonfinite > 0 or a non-finite total: the kernel
//                       returns without touching p, g, m, v -- the contract of the skip word.
//   ema_kernel        : the exponential moving average of the parameters, ema += (1 - decay) (p - ema), one launch behind the update
//                       (12 B/param: read p and ema, write ema).  It reads the two things that say "the update was dropped" -- the
//                       skip word, and the {norm, nonfinite} pair adamw_kernel wrote -- and then leaves ema alone as well.
//   swap_kernel       : a <-> b element by element (the averaged weights in and out of the model, no third buffer).
//   grad_accumulate_kernel : acc (+)= weight * g over the n gradients and the loss slot of a flat gradient buffer, and the OR of the
//                       two fault words behind them (12 B/param; 8 on the first fold, which does not read acc): micro-batches are
//                       folded into one update.  One fma per element, the same in the 16-byte loop and in the tail.
#include "sat_internal.h"

#include <cmath>

namespace {

constexpr int OPT_BLOCK = 256;
constexpr int OPT_GRID_CAP = 768;       // sat_elementwise.hip's ew_grid: at most 3 workgroups per CU
constexpr int OPT_MAX_EXEMPT = 32;

// workgroups (= partial pairs) of a sum of squares over n elements: one per 256 16-byte chunks, at least 1, at most 768
inline int sumsq_grid(long n) {
    const long b = ((n >> 2) + OPT_BLOCK - 1) / OPT_BLOCK;
    return (int)(b < 1 ? 1 : (b > OPT_GRID_CAP ? OPT_GRID_CAP : b));
}

__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// Sum of (a, b) over the 256 threads of the workgroup, the same bits in every thread: xor butterfly over the 64 lanes (both partners
// of an exchange form the same commutative sum), then the four waves' sums from LDS, added in wave order.
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*sh)[2]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave][0] = a; sh[wave][1] = b; }
    __syncthreads();
    a = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
    b = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
}

__global__ __launch_bounds__(OPT_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, long n, float clip,
                                                               double* __restrict__ partials) {
    __shared__ double sh[4][2];
    double sum = 0.0, bad = 0.0;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_BLOCK) {
        const f32x4 gg = ((const f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gk = gg[k];
            if (not_finite(gk)) bad += 1.0;
            if (clip > 0.0f) gk = fminf(fmaxf(gk, -clip), clip);
            sum += (double)gk * (double)gk;
        }
    }
    // tail (n % 4): the first lanes of workgroup 0
    const long i = (n4 << 2) + (long)blockIdx.x * OPT_BLOCK + threadIdx.x;
    if (i < n) {
        float gk = g[i];
        if (not_finite(gk)) bad += 1.0;
        if (clip > 0.0f) gk = fminf(fmaxf(gk, -clip), clip);
        sum += (double)gk * (double)gk;
    }
    block_sum2(sum, bad, sh);
    if (threadIdx.x == 0) {
        partials[2 * (long)blockIdx.x] = sum;
        partials[2 * (long)blockIdx.x + 1] = bad;
    }
}

// parameters that do not decay: sorted, disjoint [lo, hi) element ranges, every lo a multiple of 4 -- by value in the kernel arguments
struct ExemptTable {
    int n;
    long lo[OPT_MAX_EXEMPT], hi[OPT_MAX_EXEMPT];
};

__device__ __forceinline__ bool exempt_at(const ExemptTable& t, long e) {
    bool ex = false;
    for (int k = 0; k < t.n; ++k) ex = ex || (e >= t.lo[k] && e < t.hi[k]);
    return ex;
}

// `partials` NULL: no norm (coef 1, no non-finite check).  decay == 1: no decay and no look at the table.  With both, and with
// coef == 1 in general, the arithmetic on an element is clamp_adam_kernel's, bit for bit: m + w1 (g - m) and v beta2 + (w2 g) g are
// written there as plain expressions that the compiler contracts: in the 16-byte loop into one fma each (the product (w2 g) g
// rounded), in the scalar tail m into an fma and v into two rounded products and a sum.  Here the same roundings are spelt out,
// because with the branches around them the compiler contracted otherwise (tests/test_gpu_optim.py pins the bits against that kernel).
__global__ __launch_bounds__(OPT_BLOCK) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long n, float beta1, float beta2, float eps,
                                                          float clip, float step_size, float bc2_sqrt, float decay,
                                                          ExemptTable exempt, double max_norm, const double* __restrict__ partials,
                                                          int n_partials, double* __restrict__ norm_out,
                                                          const float* __restrict__ skip) {
    __shared__ double sh[4][2];
    if (skip && *skip != 0.0f) return;
    float coef = 1.0f;
    if (partials) {
        double total = 0.0, bad = 0.0;
        for (int i = threadIdx.x; i < n_partials; i += OPT_BLOCK) {
            total += partials[2 * (long)i];
            bad += partials[2 * (long)i + 1];
        }
        block_sum2(total, bad, sh);
        const double norm = sqrt(total);
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) {
            norm_out[0] = norm;
            norm_out[1] = bad;
        }
        if (bad > 0.0 || !(fabs(total) <= 1.79769313486231570815e+308)) return;      // the whole update is dropped
        coef = (float)fmin(max_norm / (norm + 1e-6), 1.0);
    }
    const bool scale = coef != 1.0f, decays = decay != 1.0f;
    const float w1 = 1.0f - beta1, w2 = 1.0f - beta2;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = ((f32x4*)p)[i], gg = ((f32x4*)g)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        const bool dk = decays && !exempt_at(exempt, i << 2);       // a 16-byte chunk belongs to one parameter
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gk = gg[k];
            if (clip > 0.0f) gk = fminf(fmaxf(gk, -clip), clip);
            if (scale) gk = __fmul_rn(gk, coef);                    // (rounded products, as torch's mul_: never fused into what follows)
            if (dk) pp[k] = __fmul_rn(pp[k], decay);
            gg[k] = gk;
            mm[k] = __fmaf_rn(w1, gk - mm[k], mm[k]);
            vv[k] = __fmaf_rn(vv[k], beta2, __fmul_rn(__fmul_rn(w2, gk), gk));
            const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
            pp[k] = pp[k] + (-step_size * mm[k]) / denom;
        }
        ((f32x4*)p)[i] = pp; ((f32x4*)g)[i] = gg; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
    }
    // tail (n % 4)
    const long base = n4 << 2;
    const long i = base + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float gk = g[i];
        if (clip > 0.0f) gk = fminf(fmaxf(gk, -clip), clip);
        if (scale) gk = __fmul_rn(gk, coef);
        g[i] = gk;
        float pk = p[i];
        if (decays && !exempt_at(exempt, i)) pk = __fmul_rn(pk, decay);
        const float mk = __fmaf_rn(w1, gk - m[i], m[i]);
        const float vk = __fadd_rn(__fmul_rn(v[i], beta2), __fmul_rn(__fmul_rn(w2, gk), gk));    // (not contracted there: see above)
        m[i] = mk; v[i] = vk;
        p[i] = pk + (-step_size * mk) / (sqrtf(vk) / bc2_sqrt + eps);
    }
}

// The difference rounded, then one fma: every element sees the same two roundings in the 16-byte loop and in the scalar tail.
__device__ __forceinline__ float ema_one(float e, float p, float w) { return __fmaf_rn(w, __fsub_rn(p, e), e); }

// `skip`, `norm_state` (either may be NULL): the conditions under which clamp_adam_kernel / adamw_kernel returned without touching
// p -- a non-zero fault word; a non-finite-element count > 0 or a norm that is not finite (norm = sqrt(total): finite exactly when
// adamw_kernel's `total` is).  Then nothing is written here either.
__global__ __launch_bounds__(OPT_BLOCK) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float w,
                                                        const float* __restrict__ skip, const double* __restrict__ norm_state) {
    if (skip && *skip != 0.0f) return;
    if (norm_state && (norm_state[1] > 0.0 || !(fabs(norm_state[0]) <= 1.79769313486231570815e+308))) return;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_BLOCK) {
        f32x4 ee = ((f32x4*)ema)[i];
        const f32x4 pp = ((const f32x4*)p)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) ee[k] = ema_one(ee[k], pp[k], w);
        ((f32x4*)ema)[i] = ee;
    }
    // tail (n % 4): the first lanes of workgroup 0
    const long i = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && i < n) ema[i] = ema_one(ema[i], p[i], w);
}

// the host has checked that the two ranges do not overlap
__global__ __launch_bounds__(OPT_BLOCK) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_BLOCK) {
        const f32x4 x = ((f32x4*)a)[i], y = ((f32x4*)b)[i];
        ((f32x4*)a)[i] = y;
        ((f32x4*)b)[i] = x;
    }
    const long i = (n4 << 2) + threadIdx.x;
    if (blockIdx.x == 0 && i < n) {
        const float x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

// One rounding per element: the product on the first fold (acc is NOT read: stale bits, NaN included, cannot leak), one fma after it.
__device__ __forceinline__ float acc_one(float a, float g, float w, bool first) { return first ? __fmul_rn(w, g) : __fmaf_rn(w, g, a); }

// Elements 0 .. n (the n gradients and the loss slot) take the rule above; element n + 1 is the fault word: it stays set once any
// fold has brought a non-zero one, and the update kernels drop on it.  The 16-byte chunks end at or in front of n + 1, the tail
// (at most 3 elements) and the fault word belong to workgroup 0.  The host has checked that the two ranges do not overlap.
__global__ __launch_bounds__(OPT_BLOCK) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n,
                                                                    float w, int first) {
    const long n1 = n + 1;
    const long n4 = n1 >> 2;
    for (long i = (long)blockIdx.x * OPT_BLOCK + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_BLOCK) {
        const f32x4 gg = ((const f32x4*)g)[i];
        f32x4 aa = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!first) aa = ((f32x4*)acc)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) aa[k] = acc_one(aa[k], gg[k], w, first != 0);
        ((f32x4*)acc)[i] = aa;
    }
    if (blockIdx.x != 0) return;
    const long i = (n4 << 2) + threadIdx.x;
    if (i < n1) acc[i] = acc_one(first ? 0.0f : acc[i], g[i], w, first != 0);
    if (threadIdx.x == OPT_BLOCK - 1) acc[n1] = ((!first && acc[n1] != 0.0f) || g[n1] != 0.0f) ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int sat_grad_sumsq_partials(int64_t n) { return n < 1 ? 0 : sumsq_grid((long)n); }

extern "C" int64_t sat_grad_sumsq_ws_bytes(int64_t n) { return n < 1 ? 0 : (int64_t)sumsq_grid((long)n) * 2 * (int64_t)sizeof(double); }

extern "C" int sat_grad_sumsq(const float* g, int64_t n, float clip, double* partials, int partial_offset, int partial_capacity,
                              sat_stream_t stream) {
    if (!g || !partials || n < 1 || partial_offset < 0 || clip != clip) return SAT_ERR_ARG;
    if (((uintptr_t)g & 15) != 0 || ((uintptr_t)partials & 15) != 0) return SAT_ERR_ARG;
    const int grid = sumsq_grid((long)n);
    if ((long)partial_offset + grid > (long)partial_capacity) return SAT_ERR_ARG;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(OPT_BLOCK), 0, (hipStream_t)stream, g, (long)n, clip,
                       partials + 2 * (long)partial_offset);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_adamw_step(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                              float clip, int step, float weight_decay, const int64_t* exempt, int n_exempt, float max_norm,
                              const double* partials, int n_partials, double* norm_out, const float* skip_if_nonzero,
                              sat_stream_t stream) {
    if (!p || !g || !m || !v || n < 1 || step < 1) return SAT_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return SAT_ERR_ARG;
    if (!(weight_decay >= 0.0f)) return SAT_ERR_ARG;                                   // (NaN fails the comparison)
    if (partials && (!(max_norm > 0.0f) || n_partials < 1 || ((uintptr_t)partials & 15) != 0)) return SAT_ERR_ARG;
    if (((uintptr_t)norm_out & 7) != 0) return SAT_ERR_ARG;
    if (n_exempt < 0 || n_exempt > OPT_MAX_EXEMPT || (n_exempt > 0 && !exempt)) return SAT_ERR_ARG;
    ExemptTable table = {};
    table.n = n_exempt;
    for (int k = 0; k < n_exempt; ++k) {
        const int64_t lo = exempt[2 * k], hi = exempt[2 * k + 1];
        if (lo < 0 || (lo & 3) != 0 || hi <= lo || (k > 0 && lo < exempt[2 * k - 1])) return SAT_ERR_ARG;
        table.lo[k] = (long)lo;
        table.hi[k] = (long)hi;
    }
    // bias corrections and the decay factor in double on the host, exactly as torch.optim.AdamW forms them with python floats
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    const float decay = (float)(1.0 - (double)lr * (double)weight_decay);
    const long items = (long)(n / 4 + 1);
    const long blocks = (items + OPT_BLOCK - 1) / OPT_BLOCK;
    const int grid = (int)(blocks > OPT_GRID_CAP ? OPT_GRID_CAP : blocks);             // clamp_adam_kernel's grid
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(OPT_BLOCK), 0, (hipStream_t)stream, p, g, m, v, (long)n, beta1, beta2, eps,
                       clip, step_size, bc2_sqrt, decay, table, (double)max_norm, partials, n_partials, norm_out, skip_if_nonzero);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_ema_update(float* ema, const float* p, int64_t n, float decay, const float* skip_if_nonzero,
                              const double* norm_state, sat_stream_t stream) {
    if (!ema || !p || n < 1) return SAT_ERR_ARG;
    if ((((uintptr_t)ema | (uintptr_t)p) & 15) != 0 || ((uintptr_t)norm_state & 7) != 0) return SAT_ERR_ARG;
    if (!(decay > 0.0f && decay < 1.0f)) return SAT_ERR_ARG;                           // (NaN fails the comparison)
    const float w = (float)(1.0 - (double)decay);
    hipLaunchKernelGGL(ema_kernel, dim3(sumsq_grid((long)n)), dim3(OPT_BLOCK), 0, (hipStream_t)stream, ema, p, (long)n, w,
                       skip_if_nonzero, norm_state);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_swap_f32(float* a, float* b, int64_t n, sat_stream_t stream) {
    if (!a || !b || n < 1) return SAT_ERR_ARG;
    if ((((uintptr_t)a | (uintptr_t)b) & 15) != 0) return SAT_ERR_ARG;
    const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b;
    const uintptr_t hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
    if ((hi - lo) / sizeof(float) < (uintptr_t)n) return SAT_ERR_ARG;                   // the ranges overlap
    hipLaunchKernelGGL(swap_kernel, dim3(sumsq_grid((long)n)), dim3(OPT_BLOCK), 0, (hipStream_t)stream, a, b, (long)n);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}

extern "C" int sat_grad_accumulate(float* acc, const float* g, int64_t n, float weight, int first, sat_stream_t stream) {
    if (!acc || !g || n < 0) return SAT_ERR_ARG;
    if ((((uintptr_t)acc | (uintptr_t)g) & 15) != 0) return SAT_ERR_ARG;
    if (!(fabsf(weight) <= 3.402823466e+38f)) return SAT_ERR_ARG;                      // (NaN fails the comparison)
    const uintptr_t lo = (uintptr_t)acc < (uintptr_t)g ? (uintptr_t)acc : (uintptr_t)g;
    const uintptr_t hi = (uintptr_t)acc < (uintptr_t)g ? (uintptr_t)g : (uintptr_t)acc;
    if ((hi - lo) / sizeof(float) < (uintptr_t)n + 2) return SAT_ERR_ARG;               // the ranges (n + 2 floats each) overlap
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(sumsq_grid((long)n + 1)), dim3(OPT_BLOCK), 0, (hipStream_t)stream, acc, g,
                       (long)n, weight, first);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}
