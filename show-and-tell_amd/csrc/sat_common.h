// Shared device/host helpers for the gfx950 (MI355X, CDNA4) kernels of the Show-and-Tell hot path.
// wave = 64 lanes; MFMA fragment maps follow the CDNA4 ISA (32x32x16 bf16 / 32x32x2 f32 / 16x16x4 f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SAT_OK 0
#define SAT_ERR_ARG 1001          // bad shape / alignment / null pointer
#define SAT_ERR_WORKSPACE 1002    // workspace too small
#define SAT_ERR_UNSUPPORTED 1003

#define SAT_LAUNCH_CHECK()                         \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

typedef __bf16 bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

enum { SAT_F32 = 0, SAT_BF16 = 1 };

static inline int sat_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// accurate (ocml) exp/tanh: these sit on the serial LSTM chain and in CE, never on a throughput path
__device__ __forceinline__ float sat_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float sat_tanh(float x) { return tanhf(x); }

// 16-byte global store, write-through to memory at system scope (sc0 sc1).  For a kernel's bulk OUTPUT that the NEXT launch reads:
// every XCD has its own L2 and a launch ends with a write-back of the dirty lines its workgroups left there; lines that went
// through already shorten that tail (conv output tiles: 19.8 -> 18.7 us for the 25.7 MB of a layer-3 conv3, -2 % on the step).
__device__ __forceinline__ void store16_wt(void* dst, u32x4 v) {
    // s_nop: a VMEM store of more than 64 bits needs wait states before its data VGPRs may be overwritten; the compiler's hazard
    // recognizer does not look inside inline asm
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return (bf16_t)v; }

// Philox4x32-10 (Salmon et al., SC'11; the Random123 / rocRAND / torch generator): 4 x u32 of a counter -> 4 random u32 words.
// Scheduled sampling keys every decision by (token group, row, step, stream) so that a draw does not depend on launch geometry.
__device__ __forceinline__ u32x4 sat_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
    }
    return (u32x4){c0, c1, c2, c3};
}

// Gumbel(0,1) noise -log(-log u) of the uniform u = ((x >> 8) + 0.5) * 2^-24 in (0, 1).  u itself is exact in f32 below 1/2 and
// 1 - u is exact at and above it, so -log u is taken as -log1p(-(1 - u)) there: the large noise values (u -> 1) that decide a
// Gumbel-max draw keep full f32 accuracy instead of collapsing to +inf at the top uniform.
__device__ __forceinline__ float sat_gumbel(unsigned x) {
    const unsigned m = x >> 8;
    const float nl = m < (1u << 23) ? -logf(((float)m + 0.5f) * 0x1p-24f)
                                    : -log1pf(-(((float)((1u << 24) - 1u - m) + 0.5f) * 0x1p-24f));
    return -logf(nl);
}
