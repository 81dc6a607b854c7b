// Pieces shared by the conv kernel families of sat_conv_glds.hip.  Each owns ONE contract that tests and the tuning table rely on:
//   * bn_relu_chunk (+ in_tab_fetch): the operand transform, bit for bit the normalise+ReLU kernel (conv_aw / ap / pw / pr / xp; conv_ay's
//     residual form and the ring kernel's scalar form are their own);
//   * swz_of / swz_chunk / frag_off: the XOR swizzle of the 128-byte LDS row image.  Every fragment READ goes through them; of the
//     WRITERS the ring kernel's loaders, conv_ay and conv_pw do, while conv_aw / conv_ap (`sw0`), conv_pr's loaders and conv_xp still
//     spell `(row >> 1) & 7` by hand (the helper moved their instructions): whoever changes swz_of changes those sites with it;
//   * lane_halves: the last step of every family's BatchNorm column sums;
//   * acc_row: the MFMA C/D row map of the accumulator-to-LDS staging loops;
//   * lds_barrier / raw_barrier / wait_vmcnt: the waits in front of a barrier.
#pragma once
#include "sat_bn_stats.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

// ---- waits and barriers ----
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// a RAW barrier: the loads in flight stay in flight (__syncthreads would wait for every one of them); nothing moves across it
__device__ __forceinline__ void raw_barrier() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// ... behind this wave's own LDS traffic: what it wrote is visible to everybody, what it read has arrived
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
}

// ---- the XOR-swizzled row image: rows of 128 B (one K-step of 64 channels), logical 16-byte chunk c of row `row` in slot c ^ swz_of(row) ----
__device__ __forceinline__ int swz_of(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swz_chunk(int c, int row) { return c ^ swz_of(row); }      // slot <-> chunk (an involution)
// the reader's side: byte offset of the MFMA fragment of lane (r, h), substep ks: row r, chunk 2 ks + h
__device__ __forceinline__ int frag_off(int r, int h, int ks) { return r * 128 + (swz_chunk(2 * ks + h, r) << 4); }

// ---- operand transform: relu(x * scale + shift) of 8 packed bf16, bit for bit the scalar fmaxf((float)x * s + t, 0) -> bf16 of
//      the normalise+ReLU kernel.  Word q = channels (2q, 2q+1): unpack by shift / mask, one packed fma, ONE packed convert (round to
//      nearest even, what the scalar cast does) and the ReLU AFTER the rounding, on the bf16 pair as int16 (rounding is monotonic and keeps
//      the sign, so max(round(x), 0) == round(max(x, 0))).  keep == false: zeros (rows past M stay zero) ----
struct InTab { f32x4 s0, s1, t0, t1; };      // (scale, shift) of eight consecutive channels
__device__ __forceinline__ InTab in_tab_fetch(const float* ts, int cin) {      // ts = table + first channel; the shifts sit cin floats on
    return {*(const f32x4*)ts, *(const f32x4*)(ts + 4), *(const f32x4*)(ts + cin), *(const f32x4*)(ts + cin + 4)};
}
__device__ __forceinline__ u32x4 bn_relu_chunk(u32x4 w, const InTab& t, bool keep = true) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x2 sc2, sh2, f;
        sc2[0] = q < 2 ? t.s0[2 * q] : t.s1[2 * q - 4]; sc2[1] = q < 2 ? t.s0[2 * q + 1] : t.s1[2 * q - 3];
        sh2[0] = q < 2 ? t.t0[2 * q] : t.t1[2 * q - 4]; sh2[1] = q < 2 ? t.t0[2 * q + 1] : t.t1[2 * q - 3];
        f[0] = __uint_as_float(w[q] << 16);
        f[1] = __uint_as_float(w[q] & 0xffff0000u);
        f = __builtin_elementwise_fma(f, sc2, sh2);
        const s16x2 pk = __builtin_bit_cast(s16x2, __builtin_convertvector(f, bf16x2));
        const s16x2 zero2 = {0, 0};
        w[q] = keep ? __builtin_bit_cast(unsigned int, __builtin_elementwise_max(pk, zero2)) : 0u;
    }
    return w;
}

// ---- BatchNorm column sums: the fold of the two lane halves (rows 4 h + ...) that ends every family's per-lane sums.  The per-lane loop
//      itself (a lane's rows in element order: `s += v; q += v * v`) stays spelled out in each kernel: inside a helper the compiler fuses
//      the multiply-adds of the chain the other way round, which changes the bits of the statistics ----
__device__ __forceinline__ void lane_halves(float& s, float& q) {
    s += __shfl_xor(s, 32, 64);
    q += __shfl_xor(q, 32, 64);
}

// ---- MFMA 32 x 32 C/D map: element e of lane (column lane & 31, h = lane >> 5) of row block i holds row ... ----
__device__ __forceinline__ int acc_row(int i, int e, int h) { return i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h; }
