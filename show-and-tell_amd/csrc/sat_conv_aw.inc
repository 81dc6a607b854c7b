// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the variant table and the pieces of sat_conv_tile.h).
//
// 1x1 convolution (conv1 / conv3 / the projection of a bottleneck, `self.resnet(images)`, models.py:27) as a 128 x 128-tile GEMM with
// the WEIGHTS STRAIGHT INTO REGISTERS from the fragment-ordered copy (sat_conv_pack_weights, taps = 1) -- conv_pw_kernel's other half:
//   * 4 waves, all alike: wave w owns columns [32 w, 32 w + 32) x 128 rows (four 32 x 32 accumulators); its B fragment of a substep
//     is one coalesced 1 KB buffer load, three K-steps ahead, and nobody else reads that slice: no LDS, no barrier for the weights;
//   * the activations go global -> registers -> LDS (16 KB per K-step, the ring kernel's XOR-swizzled row image, three buffers):
//     three K-steps in flight in registers, written to LDS one K-step before use; ONE barrier per K-step.  Everything is a plain
//     load the compiler counts (no LDS-DMA: with register loads in the same wave LLVM's wait insertion would drain the queue,
//     sat_conv_pw.inc); rows past M read zeros through the buffer bounds;
//   * the A fragment addresses are K-invariant (row r, chunk (2 ks + h) ^ swizzle) + an immediate (buffer, row block): no address
//     arithmetic in the K loop -- ~60 instructions per wave and K-step against 16 MFMAs (the ring kernel's unified waves: ~110);
//   * the operand's BatchNorm + ReLU (bn2 in front of conv3) is applied to the registers on their way to LDS (AFF);
//   * 48 KB of LDS, <= 256 registers: two workgroups per CU, so a launch of 196 G tiles is one round for G <= 2.
// K order = the ring kernel's: the conv output is bit-identical to it; the BatchNorm column sums are conv_pw_kernel's (a lane sums
// 64 of a column's 128 rows, then the two halves).
// NW = 4: 128-column tiles, two workgroups per CU.  NW = 8: 256-column tiles -- the activations of a row tile are staged ONCE for
// 256 output columns (half the bytes through L2 -> CU per flop on the A side), one workgroup of eight waves per CU.
// RES: the inference epilogue with a residual (conv3 of a bottleneck in eval mode): its 16 bytes per thread and store are requested
// before the last K-steps, so their latency hides under those and the tile staging instead of sitting in the store phase.
template <bool AFF, int NW, bool RES>
__global__ __launch_bounds__(NW * 64, 2) void conv_aw_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = NW * 32, NT = NW * 64, PD = 3;
    constexpr int ABUF = BM * 128;                          // one K-step of A: 128 rows x 64 channels
    constexpr int CROW = BN * 2 + 16;
    constexpr int NJ = BM * 8 / NT;                         // 16-byte chunks of an A stage per thread (4 / 2), rows NT / 8 apart
    constexpr int RJ = NT / 8;
    constexpr int TAB = (3 * ABUF > BM * CROW) ? 3 * ABUF : BM * CROW;      // the epilogue's bf16 tile lives in the A buffers
    __shared__ __attribute__((aligned(16))) char smem[TAB + (AFF ? 4096 : 0)];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int tile = xcd_tile();
    const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk = p.Cin >> 6;                                // K-steps of 64 channels

    // ---- this thread's share of an A stage: 16-byte chunk slot lc of rows r0 + 32 j; it fetches logical chunk lc ^ ((row >> 1) & 7)
    //      (the same for its four rows), so the LDS image is the ring kernel's.  Rows past M: an offset past the buffer (reads 0). ----
    const int lc = tid & 7, r0 = tid >> 3;
    const int sw0 = (r0 >> 1) & 7;
    const __amdgpu_buffer_rsrc_t asrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.A), 0, (int)(p.in_bytes), 0x00020000);
    int a_voff[NJ];
    unsigned a_ok = 0u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int grow = m0 + r0 + RJ * j;
        long pix;
        if (p.linear) {
            pix = (long)grow * p.sW;
        } else {
            const int hw = p.Hout * p.Wout;
            const int n = grow / hw;
            const int rem = grow - n * hw;
            const int ho = rem / p.Wout;
            const int wo = rem - ho * p.Wout;
            pix = (long)n * p.sN + (long)(ho * p.stride) * p.sH + (long)(wo * p.stride) * p.sW;
        }
        const bool ok = grow < p.M;
        a_voff[j] = ok ? (int)((pix + ((lc ^ sw0) << 3)) * 2) : 0x7ffffff0;
        if (ok) a_ok |= 1u << j;
    }
    // (K-steps past the end re-read the last one: never used, and no reliance on how the bounds check treats the scalar offset)
    auto load_a_stage = [&](int g, u32x4 (&dst)[NJ]) {
        const int gs = (g < nk ? g : nk - 1) * 128;
#pragma unroll
        for (int j = 0; j < NJ; ++j) dst[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(asrc, a_voff[j], gs, 0));
    };

    // ---- this wave's weight stream: nk K-steps of 4 KB, fragment ordered ----
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>((const char*)p.Bp + (long)((n0 >> 5) + wave) * nk * 4096), 0, nk * 4096, 0x00020000);
    const int wlane = lane * 16;
    auto load_b = [&](int g, int ks) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wsrc, wlane, (g < nk ? g : nk - 1) * 4096 + ks * 1024, 0));
    };

    // ---- prologue: everything is requested first ----
    u32x4 ar[3][NJ];
    load_a_stage(0, ar[0]);
    load_a_stage(1, ar[1]);
    load_a_stage(2, ar[2]);
    bf16x8 bq[PD][4];
#pragma unroll
    for (int s = 0; s < PD; ++s)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bq[s][ks] = load_b(s, ks);

    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;

    // AFF: BatchNorm + ReLU of the operand (bn2 in front of conv3): (scale, shift) of all Cin channels into LDS once
    float* in_tab = (float*)(smem + TAB);
    if constexpr (AFF) {
        conv_in_table<NT>(p, in_tab);
        lds_barrier();      // (not __syncthreads: that would also wait for every load in flight)
    }
    // a landed stage on its way to LDS: (AFF: relu(x * scale + shift) per channel, bit for bit the normalise+ReLU kernel; rows past M
    // stay zero) then 16 bytes per row into slot lc of rows r0 + 32 j of buffer `buf`
    auto store_a_stage = [&](int g, int buf, u32x4 (&src)[NJ]) {
        char* at0 = smem + buf * ABUF + r0 * 128 + (lc << 4);
        if constexpr (AFF) {
            const float* ts = in_tab + g * 64 + ((lc ^ sw0) << 3);
            const bool live = g < nk;                           // (past the end: whatever, nobody reads it; keep the table reads in bounds)
            const float* tq = live ? ts : in_tab;
            const InTab tab = in_tab_fetch(tq, p.Cin);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                u32x4 w = src[j];
                w = bn_relu_chunk(w, tab, (a_ok >> j) & 1u);
                *(u32x4*)(at0 + j * (RJ * 128)) = w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) *(u32x4*)(at0 + j * (RJ * 128)) = src[j];
        }
    };

    // A fragment addresses, K-invariant: row i*32 + r (the four row blocks 4096 B apart, same swizzle), chunk (2 ks + h) ^ ((r >> 1) & 7)
    int a_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a_off[ks] = frag_off(r, h, ks);

    store_a_stage(0, 0, ar[0]);
    load_a_stage(3, ar[0]);

    // K-step g, U = g % 3 (compile time): stage g sits in LDS buffer U; stage g + 1 leaves registers (slot (U + 1) % 3) for buffer
    // (U + 1) % 3, whose last readers (K-step g - 2) are two barriers back; its slot takes stage g + 4; the weight registers of
    // K-step g (slot U) are refilled with K-step g + 3 as they are used
    auto step = [&](int g, auto u_tag, auto tail_tag) {
        constexpr int U = decltype(u_tag)::value, U1 = (U + 1) % 3;
        constexpr bool TAIL = decltype(tail_tag)::value;       // one of the last three K-steps: nothing it could request would be used
        // this wave's LDS writes of stage g and everybody's; everybody is done with K-step g - 1 (the loads in flight stay in flight)
        lds_barrier();
        store_a_stage(g + 1, U1, ar[U1]);
        if constexpr (!TAIL) load_a_stage(g + 4, ar[U1]);
        const char* st = smem + U * ABUF;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 fa[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = *(const bf16x8*)(st + a_off[ks] + i * 4096);
            const bf16x8 b = bq[U][ks];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], b, acc[i], 0, 0, 0);
            if constexpr (!TAIL) bq[U][ks] = load_b(g + PD, ks);
        }
    };
    // RES: this thread's chunks of the residual tile (rows past M read zeros through the buffer bounds)
    constexpr int ITS = BM * (BN / 8) / NT;
    u32x4 resv[RES ? ITS : 1];
    auto fetch_residual = [&]() {
        if constexpr (RES) {
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.residual), 0, (int)((long)p.M * p.ldc * 2), 0x00020000);
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                const int qid = tid + it * NT;
                const int row = qid / (BN / 8), cc = qid % (BN / 8);
                resv[it] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(((long)(m0 + row) * p.ldc + n0 + cc * 8) * 2), 0, 0));
            }
        }
    };
    // the last one to three K-steps are peeled: they request nothing (stage g + 4 and K-step g + 3 lie past the end), and the residual
    // of the inference epilogue is requested in front of them
    const int rem = nk % 3 == 0 ? 3 : nk % 3;
    int g = 0;
    for (; g + 3 <= nk - rem; g += 3) {
        step(g, std::integral_constant<int, 0>{}, std::false_type{});
        step(g + 1, std::integral_constant<int, 1>{}, std::false_type{});
        step(g + 2, std::integral_constant<int, 2>{}, std::false_type{});
    }
    // (the epilogue's per-column affine is requested first: in the in-order load queue it must not sit behind the residual)
    const int colw = wave * 32 + r;
    float osc = 1.0f, osh = 0.0f;
    if (p.out_scale && n0 + colw < p.N) { osc = p.out_scale[n0 + colw]; osh = p.out_shift[n0 + colw]; }
    fetch_residual();
    step(g, std::integral_constant<int, 0>{}, std::true_type{});
    if (rem > 1) step(g + 1, std::integral_constant<int, 1>{}, std::true_type{});
    if (rem > 2) step(g + 2, std::integral_constant<int, 2>{}, std::true_type{});
    // (stages requested past the end by the steps before the peeled ones are plain loads the compiler tracks, register reuse included;
    // RES: the residual stays in flight across the statistics / tile staging)
    lds_barrier();      // every wave's LDS traffic is done before the A buffers become the tile

    // ---- epilogue: BatchNorm column sums (a lane holds 64 of a column's 128 rows), bf16 tile through LDS ----
    if (p.stat_partial || p.acc) {
        float s = 0.0f, q = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float v = acc[i][e];
                s += v;
                q += v * v;
            }
        lane_halves(s, q);
        const int col = n0 + colw;
        if (h == 0 && col < p.N) {
            if (p.acc) {
                stat_acc_add(p.acc, p.N, s, q, col);
            }
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, tile_m, p.N, s, q, col);
            }
        }
    }
    {
        const bool relu_now = p.out_relu && !RES;             // with a residual the ReLU follows the add (store phase)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = acc_row(i, e, h);
                float v = acc[i][e];
                if (p.out_scale) v = v * osc + osh;
                if (relu_now) v = fmaxf(v, 0.0f);
                *(bf16_t*)(smem + row * CROW + colw * 2) = (bf16_t)v;
            }
    }
    lds_barrier();
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
        const int qid = tid + it * NT;
        const int row = qid / (BN / 8), cc = qid % (BN / 8);
        const int grow = m0 + row, gcol = n0 + cc * 8;
        if (grow < p.M && gcol < p.N) {
            if constexpr (RES) {                  // out = [relu](affine(acc) + residual), 16 bytes of each per thread
                const bf16x8 c = *(const bf16x8*)(smem + row * CROW + cc * 16);
                const bf16x8 z = __builtin_bit_cast(bf16x8, resv[it]);
                bf16x8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float v = (float)c[k] + (float)z[k];
                    if (p.out_relu) v = fmaxf(v, 0.0f);
                    o[k] = (bf16_t)v;
                }
                store16_wt(p.C + (long)grow * p.ldc + gcol, __builtin_bit_cast(u32x4, o));
            } else {
                store16_wt(p.C + (long)grow * p.ldc + gcol, *(const u32x4*)(smem + row * CROW + cc * 16));
            }
        }
    }
}

// 1x1, no padding, Cin a multiple of 64, Cout of 128 (256 for the eight-wave form), the fragment-ordered copy of the weights, an input
// tensor a 32-bit byte offset can address
bool aw_ok(const ConvArgs& a, int nw) {
    return a.Bp != nullptr && a.KH == 1 && a.KW == 1 && a.pad == 0 && a.padw == 0 && (a.Cin % 64) == 0 && a.K == a.Cin && (a.N % (nw * 32)) == 0 &&
           (!a.in_affine || (a.Cin <= 512 && a.linear)) && a.in_bytes > 0 && a.in_bytes < 0x7ffffff0L;
}

template <int NW>
int launch_aw(ConvArgs& a, int groups, hipStream_t s) {
    if (!aw_ok(a, NW)) return SAT_ERR_UNSUPPORTED;
    a.tiles_n = a.N / (NW * 32);
    static constexpr ConvKernel kKernel[2][2] = {{conv_aw_kernel<false, NW, false>, conv_aw_kernel<true, NW, false>},      // [residual][in_affine]
                                                 {conv_aw_kernel<false, NW, true>, conv_aw_kernel<true, NW, true>}};
    const bool res = a.residual != nullptr;
    const bool fits = !res || (long)a.M * a.ldc * 2 < 0x7ffffff0L;      // the residual is read through a 32-bit buffer offset
    return launch_conv(fits ? kKernel[res][a.in_affine] : nullptr, dim3(sat_cdiv(a.M, 128) * a.tiles_n, groups), dim3(NW * 64), 0, s, a);
}
