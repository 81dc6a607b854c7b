// The tile loop of the three-way-split f32 GEMM (sat_gemm_x3.hip: the design notes are there) with its two epilogues: the C tile
// store of sat_gemm_f32x3, and the per-row (max, sum exp) reduction of sat_vocab_logp (sat_score.hip), which stores no C tile.
// Both instantiate ONE kernel template, so the K loop -- split, six products, two accumulators, tile map -- is the same code.
#pragma once
#include "sat_internal.h"
#include <type_traits>

namespace {

struct X3Args {
    const float* A;
    long lda;
    const char* Bp;          // packed split weights: [N128 / 32][K / 64][3 splits][4 ks][64 lanes][8 bf16]
    const float* bias;
    float* C;
    long ldc;
    int M, N, K, tiles_m;
    long a_bytes;
    // the log-probability epilogue (LOGP) only: nothing of C / ldc is used there
    const int64_t* targets;  // [M]
    float* partials;         // [tiles_n][pstride][2]: (max, sum exp(x - max)) of every row over the tile's valid columns
    long pstride;
    float* tlogit;           // [M]: the target column's logit, written by the one tile that holds it
};

// the row tile's height for M rows and tiles_n column tiles: 64-row tiles (two workgroups per CU) unless 128-row ones waste no more
// rows and still fill the chip's 256 CUs.  A row's result does not depend on it.
inline bool x3_tall_tiles(int M, int tiles_n) {
    return sat_cdiv(M, 128) * 128 == sat_cdiv(M, 64) * 64 && (long)sat_cdiv(M, 128) * tiles_n >= 512;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// v of lane (lane ^ X) within the 32-lane half of the wave: ds_swizzle in bit mode (and 0x1f, or 0, xor X), no LDS memory touched
template <int X>
__device__ __forceinline__ float x3_swz_xor(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1f | (X << 10)));
}
// max / sum over the 32 lanes that hold one accumulator row's columns (col = lane & 31); every lane of the half gets the result, and
// the same bits: each butterfly stage adds the same two numbers on both sides
__device__ __forceinline__ float x3_half_max(float v) {
    v = fmaxf(v, x3_swz_xor<1>(v));
    v = fmaxf(v, x3_swz_xor<2>(v));
    v = fmaxf(v, x3_swz_xor<4>(v));
    v = fmaxf(v, x3_swz_xor<8>(v));
    return fmaxf(v, x3_swz_xor<16>(v));
}
__device__ __forceinline__ float x3_half_sum(float v) {
    v += x3_swz_xor<1>(v);
    v += x3_swz_xor<2>(v);
    v += x3_swz_xor<4>(v);
    v += x3_swz_xor<8>(v);
    return v + x3_swz_xor<16>(v);
}

// (x0, x1) -> the three bf16 pairs
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& mid, unsigned& lo) {
    f32x2 v = {x0, x1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    f32x2 r = {x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u)};
    mid = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
    f32x2 q = {r[0] - __uint_as_float(mid << 16), r[1] - __uint_as_float(mid & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(q, bf16x2));
}

// BM = 128: one workgroup per CU (96 KB of LDS, 128 + 234 registers); BM = 64: two per CU (48 KB, <= 256 registers) -- twice the
// weight bytes through L2 -> CU per flop, but two waves per SIMD cover each other's barriers and split work, and 320 rows are exactly 5 tiles
// LOGP = false: sat_gemm_f32x3's kernel (the C tile through LDS).  LOGP = true: sat_vocab_logp's, the same K loop with the epilogue
// at the end of this function
template <int BM, bool LOGP = false>
__global__ __launch_bounds__(256, BM == 128 ? 1 : 2) void gemm_x3_kernel(const X3Args p) {
    constexpr int BN = 128, NT = 256, TI = BM / 32;
    constexpr int ABUF = BM * 128;                          // one K-step of one split image: BM rows x 64 bf16
    constexpr int NJ = BM / 32, RJ = 32;                    // 8-element chunks of a stage per thread, rows RJ apart
    constexpr int CROW = BN * 4 + 16;                       // epilogue: f32 tile rows
    constexpr int SMEM = (6 * ABUF > BM * CROW) ? 6 * ABUF : BM * CROW;
    __shared__ __attribute__((aligned(16))) char smem[SMEM];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    const int tile_n = swz / p.tiles_m, tile_m = swz - tile_n * p.tiles_m;      // the row tiles of a column tile share an XCD's L2
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk = p.K >> 6;                                  // K-steps of 64: even, >= 4 (the launcher checks)

    // ---- this thread's share of an A stage: chunk slot lc (8 k-elements = 32 bytes of f32) of rows r0 + 32 j; it fetches logical
    //      chunk lc ^ ((row >> 1) & 7), so each split image is the ring kernel's XOR-swizzled row image.  Rows past M: an offset past
    //      the buffer (reads zeros) ----
    const int lc = tid & 7, r0 = tid >> 3;
    const int sw0 = (r0 >> 1) & 7;
    const __amdgpu_buffer_rsrc_t asrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    int a_voff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int grow = m0 + r0 + RJ * j;
        a_voff[j] = grow < p.M ? (int)(((long)grow * p.lda + ((lc ^ sw0) << 3)) * 4) : 0x7fffffe0;
    }
    u32x4 ax[2][NJ][2];
    auto load_stage = [&](int g, u32x4 (&d)[NJ][2]) {
        const int gs = g * 256;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            d[j][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(asrc, a_voff[j], gs, 0));
            d[j][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(asrc, a_voff[j] + 16, gs, 0));
        }
    };
    // ---- this wave's weight stream: nk K-steps of 12 KB (3 splits x 4 substeps x 1 KB), two K-steps ahead ----
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(p.Bp + (long)((n0 >> 5) + wave) * nk * 12288), 0, nk * 12288, 0x00020000);
    const int wlane = lane * 16;
    auto load_b = [&](int g, int s, int ks) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wsrc, wlane, g * 12288 + s * 4096 + ks * 1024, 0));
    };

    load_stage(0, ax[0]);
    load_stage(1, ax[1]);
    bf16x8 bq[2][3][4];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) bq[g][s][ks] = load_b(g, s, ks);

    f32x16 acc0[TI], acc1[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            acc0[i][e] = 0.0f;
            acc1[i][e] = 0.0f;
        }

    // a landed stage: split into the three bf16 terms, 16 bytes per row and image into slot lc of rows r0 + 32 j of buffer `buf`
    auto store_stage = [&](int buf, u32x4 (&sx)[NJ][2]) {
        char* at0 = smem + buf * 3 * ABUF + r0 * 128 + (lc << 4);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            u32x4 hi, mid, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 w = sx[j][q >> 1];
                unsigned th, tm, tl;
                split2(__uint_as_float(w[2 * (q & 1)]), __uint_as_float(w[2 * (q & 1) + 1]), th, tm, tl);
                hi[q] = th;
                mid[q] = tm;
                lo[q] = tl;
            }
            *(u32x4*)(at0 + j * (RJ * 128)) = hi;
            *(u32x4*)(at0 + ABUF + j * (RJ * 128)) = mid;
            *(u32x4*)(at0 + 2 * ABUF + j * (RJ * 128)) = lo;
        }
    };

    int a_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a_off[ks] = r * 128 + (((2 * ks + h) ^ ((r >> 1) & 7)) << 4);

    store_stage(0, ax[0]);
    load_stage(2, ax[0]);

    // K-step g, U = g & 1 (compile time): stage g sits in LDS buffer U; stage g + 1 leaves register slot U ^ 1 for the other buffer
    // (its last readers, K-step g - 1, are behind this step's barrier) and the slot takes stage g + 3; the weight registers of K-step
    // g (slot U) are refilled with K-step g + 2 as they are used
    auto step = [&](int g, auto u_tag, auto st_tag, auto al_tag, auto bl_tag) {
        constexpr int U = decltype(u_tag)::value;
        constexpr bool ST = decltype(st_tag)::value, AL = decltype(al_tag)::value, BL = decltype(bl_tag)::value;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (ST) store_stage(U ^ 1, ax[U ^ 1]);
        if constexpr (AL) load_stage(g + 3, ax[U ^ 1]);
        const char* st = smem + U * 3 * ABUF;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 fh[TI], fm[TI], fl[TI];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                fh[i] = *(const bf16x8*)(st + a_off[ks] + i * 4096);
                fm[i] = *(const bf16x8*)(st + ABUF + a_off[ks] + i * 4096);
                fl[i] = *(const bf16x8*)(st + 2 * ABUF + a_off[ks] + i * 4096);
            }
            const bf16x8 bh = bq[U][0][ks], bm = bq[U][1][ks], bl = bq[U][2][ks];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                acc0[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[i], bh, acc0[i], 0, 0, 0);
                acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl[i], bh, acc1[i], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[i], bl, acc1[i], 0, 0, 0);
                acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fm[i], bm, acc1[i], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fm[i], bh, acc1[i], 0, 0, 0);
                acc1[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[i], bm, acc1[i], 0, 0, 0);
            }
            if constexpr (BL) {
                bq[U][0][ks] = load_b(g + 2, 0, ks);
                bq[U][1][ks] = load_b(g + 2, 1, ks);
                bq[U][2][ks] = load_b(g + 2, 2, ks);
            }
        }
    };
    using T = std::true_type;
    using F = std::false_type;
    int g = 0;
    for (; g < nk - 4; g += 2) {
        step(g, std::integral_constant<int, 0>{}, T{}, T{}, T{});
        step(g + 1, std::integral_constant<int, 1>{}, T{}, T{}, T{});
    }
    step(g, std::integral_constant<int, 0>{}, T{}, T{}, T{});            // K-step nk - 4: requests stage nk - 1, the last
    step(g + 1, std::integral_constant<int, 1>{}, T{}, F{}, T{});        // nk - 3
    step(g + 2, std::integral_constant<int, 0>{}, T{}, F{}, F{});        // nk - 2: stores stage nk - 1
    step(g + 3, std::integral_constant<int, 1>{}, F{}, F{}, F{});        // nk - 1

    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // every wave's LDS traffic is done before the buffers become the tile
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    const int colw = wave * 32 + r;
    const float badd = (p.bias && n0 + colw < p.N) ? p.bias[n0 + colw] : 0.0f;
    if constexpr (LOGP) {
        // ---- epilogue of sat_vocab_logp: no C tile.  x = hi*hi + corrections + bias as below; per row of the tile the pair
        //      (max, sum exp(x - max)) over the tile's valid columns, and the target column's x from the tile that holds it.
        //      A lane holds column colw of the rows (reg & 3) + 8 (reg >> 2) + 4 h of each 32-row block: a row's 32 columns of this
        //      wave sit in the 32 lanes of one half, so max and sum go over the half by ds_swizzle; lane r of the half keeps the
        //      pair of accumulator slot (i * 16 + e) & 31 == r and writes it to LDS, and BM threads join the four waves' pairs in
        //      wave order.  Nothing here depends on which tile of the grid this is, or on BM. ----
        int* s_tcol = (int*)smem;                             // [BM] target column within the tile, -1: not in this tile
        float* s_tlog = (float*)(smem + BM * 4);              // [BM]
        f32x2* s_pair = (f32x2*)(smem + BM * 8);              // [4 waves][BM]
        if (tid < BM) {
            int tc = -1;
            if (m0 + tid < p.M) {
                long t = p.targets[m0 + tid];
                t = t < 0 ? 0 : (t >= p.N ? p.N - 1 : t);
                t -= n0;
                tc = (t >= 0 && t < BN) ? (int)t : -1;
            }
            s_tcol[tid] = tc;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool cvalid = n0 + colw < p.N;
        float own_m[TI * 16 / 32], own_s[TI * 16 / 32];
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
                const int rowb = i * 32 + 8 * e4 + 4 * h;
                const i32x4 tc4 = *(const i32x4*)(s_tcol + rowb);
#pragma unroll
                for (int e1 = 0; e1 < 4; ++e1) {
                    const int e = e4 * 4 + e1;
                    const float x = cvalid ? (acc0[i][e] + acc1[i][e]) + badd : -INFINITY;
                    if (tc4[e1] == colw) s_tlog[rowb + e1] = x;
                    const float m = x3_half_max(x);
                    const float s = x3_half_sum(m == -INFINITY ? 0.0f : expf(x - m));
                    const int idx = i * 16 + e;
                    if (r == (idx & 31)) {
                        own_m[idx >> 5] = m;
                        own_s[idx >> 5] = s;
                    }
                }
            }
#pragma unroll
        for (int k = 0; k < TI * 16 / 32; ++k) {
            const int idx = k * 32 + r, e = idx & 15;
            const int row = (idx >> 4) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            s_pair[wave * BM + row] = (f32x2){own_m[k], own_s[k]};
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (tid < BM && m0 + tid < p.M) {
            const f32x2 p0 = s_pair[tid], p1 = s_pair[BM + tid], p2 = s_pair[2 * BM + tid], p3 = s_pair[3 * BM + tid];
            const float mm = fmaxf(fmaxf(p0[0], p1[0]), fmaxf(p2[0], p3[0]));
            float ss = 0.0f;
            if (mm != -INFINITY) {
                ss = p0[1] * expf(p0[0] - mm);               // exp(-inf) = 0: a wave without a valid column adds nothing
                ss += p1[1] * expf(p1[0] - mm);
                ss += p2[1] * expf(p2[0] - mm);
                ss += p3[1] * expf(p3[0] - mm);
            }
            *(f32x2*)(p.partials + ((long)tile_n * p.pstride + m0 + tid) * 2) = (f32x2){mm, ss};
            if (s_tcol[tid] >= 0) p.tlogit[m0 + tid] = s_tlog[tid];
        }
        return;
    }
    // ---- epilogue: hi*hi + corrections + bias, f32 tile through LDS, 16-byte stores ----
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            *(float*)(smem + row * CROW + colw * 4) = (acc0[i][e] + acc1[i][e]) + badd;
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    constexpr int ITS = BM * (BN / 4) / NT;
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
        const int qid = tid + it * NT;
        const int row = qid / (BN / 4), cc = qid % (BN / 4);
        const int grow = m0 + row, gcol = n0 + cc * 4;
        if (grow < p.M && gcol < p.N) *(u32x4*)(p.C + (long)grow * p.ldc + gcol) = *(const u32x4*)(smem + row * CROW + cc * 16);
    }
}

}  // namespace
