// The fixed-point BatchNorm statistics that the conv epilogues produce and the BatchNorm consumers read (the conv kernels' input
// side, bn_act, bn_relu_maxpool): one definition of the format for both translation units.
//
// A column's (sum, sum of squares) is added to acc[2][N] as 64-bit INTEGERS, scaled by SAT_STAT_SCALE = 2^22.  Integer addition is
// associative, so the totals are bitwise reproducible whatever the arrival order.  Many-tile launches store f32 per-tile slabs
// partial[tiles][2][N] instead, which a reducer turns into the same integers.
#pragma once
#include "sat_internal.h"

// 1 / (2^22 * count): the factor that turns the integer sums into (mean, E[x^2])
__host__ __device__ inline double sat_stat_inv(double count) { return 1.0 / (SAT_STAT_SCALE * count); }

// column n0 + c's (sum, sum of squares) into the integer accumulators acc[2][N]
__device__ __forceinline__ void stat_acc_add(long long* acc, int N, double s, double q, int n0, int c = 0) {
    atomicAdd((unsigned long long*)(acc + n0 + c), (unsigned long long)__double2ll_rn(s * SAT_STAT_SCALE));
    atomicAdd((unsigned long long*)(acc + N + n0 + c), (unsigned long long)__double2ll_rn(q * SAT_STAT_SCALE));
}

// ... or into row `tile` of the per-tile slabs partial[tiles][2][N]
__device__ __forceinline__ void stat_slab_store(float* partial, long tile, int N, float s, float q, int n0, int c = 0) {
    partial[(tile * 2 + 0) * N + n0 + c] = s;
    partial[(tile * 2 + 1) * N + n0 + c] = q;
}

// Where a BatchNorm's (scale, shift) comes from: either a precomputed table, or -- `acc` set -- the integer sums the producing conv
// accumulated.  Then every workgroup derives the table itself (a few KB of loads, f64 arithmetic identical to bn_finalize_kernel),
// and the lead workgroup also updates the running statistics and clears the OTHER step-parity's accumulators for the next step.
struct BnSrc {
    const float* scale;
    const float* shift;
    const long long* acc;     // [2][C] (this step's parity)
    long long* acc_clear;     // [2][C] (other parity) or NULL
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
};

// (scale, shift) of channels t, t + NT, ... < C into sc[] / sh[], NT threads per workgroup (0: blockDim.x, read where the loop steps);
// inv = sat_stat_inv(count), `lead`: this workgroup updates the running statistics and clears acc_clear.  The caller owns the barrier
// after it.
template <int NT> __device__ __forceinline__ auto bn_table_step() {
    if constexpr (NT > 0) return NT;
    else return (unsigned)blockDim.x;
}
template <int NT>
__device__ __forceinline__ void bn_table(const BnSrc& b, int C, double count, double inv, float momentum, float eps, int t, bool lead,
                                         float* sc, float* sh) {
    for (int c = t; c < C; c += bn_table_step<NT>()) {
        if (b.acc) {
            const long long s1 = b.acc[c], s2 = b.acc[C + c];
            const double mean = (double)s1 * inv;
            double var = (double)s2 * inv - mean * mean;
            if (var < 0.0) var = 0.0;
            const float invstd = 1.0f / sqrtf((float)var + eps);
            const float s = b.gamma[c] * invstd;
            sc[c] = s;
            sh[c] = b.beta[c] - (float)mean * s;
            if (lead) {
                if (b.running_mean) {
                    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
                    // the batch statistic enters as an f32 value: a deferred update (sat_bn_running_apply) is then bit-identical
                    b.running_mean[c] = (float)((1.0 - momentum) * b.running_mean[c] + momentum * (double)(float)mean);
                    b.running_var[c] = (float)((1.0 - momentum) * b.running_var[c] + momentum * (double)(float)unbiased);
                }
                if (b.acc_clear) { b.acc_clear[c] = 0; b.acc_clear[C + c] = 0; }
            }
        } else {
            sc[c] = b.scale[c];
            sh[c] = b.shift[c];
        }
    }
}
