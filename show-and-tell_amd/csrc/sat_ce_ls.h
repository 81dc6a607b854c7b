// Label-smoothed softmax cross entropy of one row (torch's F.cross_entropy(..., label_smoothing=eps)): the arithmetic that
// ce_rows_ls_kernel (sat_elementwise.hip, f32 gradient) and ce_rows_ls_bf16grad_kernel (sat_gemm_bf16.hip, bf16 gradient) share.
// With lse = m + log s, m = max(x), s = sum exp(x - m):
//     nll    = lse - x[t]
//     loss   = (1 - eps) * nll + eps * (log s - mean(x - m))          (= (eps / V) * sum_v (lse - x[v]), centred on the row maximum:
//                                                                       lse - mean(x) would cancel for rows shifted by +60 / -80)
//     g[v]   = (softmax(x)[v] - (v == t ? (1 - eps) + eps / V : eps / V)) * inv_denom
// eps == 0 gives bit for bit what ce_rows_kernel / ce_rows_bf16grad_kernel give: the same operations in the same order, with
// hit = 1 and uni = 0, and the loss taken as the nll itself.
#pragma once
#include "sat_common.h"

struct CeLsRow {
    float lse, smooth;              // smooth = log s - mean(x - m)
};

struct CeLsCoef {
    float eps, hit, uni;            // hit = (1 - eps) + eps / V at the target, uni = eps / V elsewhere
};

__device__ __forceinline__ CeLsCoef ce_ls_coef(float eps, int V) {
    CeLsCoef k;
    k.eps = eps;
    k.uni = eps / (float)V;
    k.hit = (1.0f - eps) + k.uni;
    return k;
}

// max, sum of exponentials and centred sum of a row held as RC 16-byte chunks per thread (chunk c of thread tid is elements
// 4 * (tid + 256 c) ..., live while tid + 256 c < nq) plus one scalar-tail element xt per thread (`has_tail`; else pass -INFINITY).
// `reduce(v, is_max)` is the calling file's block reduction over the 256 threads: three calls, in this order.
template <int RC, typename Reduce>
__device__ __forceinline__ CeLsRow ce_ls_row_stats(const f32x4 (&rc)[RC], int nq, float xt, bool has_tail, int V, Reduce reduce) {
    const int tid = threadIdx.x;
    float m = xt;
#pragma unroll
    for (int c = 0; c < RC; ++c)
        if (tid + c * 256 < nq) m = fmaxf(fmaxf(fmaxf(m, rc[c][0]), fmaxf(rc[c][1], rc[c][2])), rc[c][3]);
    m = reduce(m, true);
    float s = 0.0f, d = 0.0f;
#pragma unroll
    for (int c = 0; c < RC; ++c)
        if (tid + c * 256 < nq) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s += expf(rc[c][e] - m);
                d += rc[c][e] - m;
            }
        }
    if (has_tail) {
        s += expf(xt - m);
        d += xt - m;
    }
    s = reduce(s, false);
    d = reduce(d, false);
    const float logs = logf(s);
    CeLsRow r;
    r.lse = m + logs;
    r.smooth = logs - d / (float)V;
    return r;
}

__device__ __forceinline__ float ce_ls_loss(const CeLsCoef& k, float nll, float smooth) {
    return k.eps == 0.0f ? nll : (1.0f - k.eps) * nll + k.eps * smooth;
}

__device__ __forceinline__ float ce_ls_grad(const CeLsCoef& k, float x, float lse, bool is_target, float inv_denom) {
    return (expf(x - lse) - (is_target ? k.hit : k.uni)) * inv_denom;
}
