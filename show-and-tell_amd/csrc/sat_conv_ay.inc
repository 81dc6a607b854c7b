// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the variant table and the pieces of sat_conv_tile.h).
//
// conv1 of a bottleneck that ALSO FINISHES THE PREVIOUS BOTTLENECK (`self.resnet(images)`, models.py:27, train-mode BatchNorm):
//     y_k   = relu(bn3_k(c3_k) + y_{k-1})          (what the normalise + add + ReLU launch computed and wrote)
//     c1    = conv1_{k+1}(y_k)                     (what conv1 then read back)
// in ONE launch (SAT_CONV_IN_RESIDUAL): the A operand of the 1x1 conv is built on its way to LDS from the RAW conv3 tensor and the
// residual -- bn3's (scale, shift) derived here from conv3's integer column sums, exactly as the normalise + add kernel derives them --
// and the workgroups of column tile 0 write y_k out as they go (the next bottleneck's residual).  Why (round 5): in the grouped
// look-ahead program the 43 normalise + add launches are 8 of 23 GB per pass and run at the HBM roof (38 us per two-batch launch in
// layer 3) while conv1 right behind them re-reads the tensor they just wrote (24 us): fused, the tensor is read twice and written once
// instead of read three times and written once, one launch of 155 + 43 disappears per bottleneck, and the bytes stream under the MFMAs.
//
// Structure = conv_aw_kernel's (sat_conv_aw.inc: 128-row tiles, wave w owns 32 columns, the weights straight into registers from the
// fragment-ordered copy, the activations global -> registers -> LDS in the ring kernel's XOR-swizzled row image, one raw barrier per
// K-step) with
//   * TWO operand streams (16 bytes of c3 and of the residual per thread and chunk), PDA stages of both in flight in registers, two
//     LDS buffers; with two workgroups per CU that is 128-256 KB in flight per CU -- the launch is bound by HBM, not by the MFMAs;
//   * the transform of a landed stage: f = fma(x, scale, shift) + z per element in f32, rounded to bf16, ReLU on the bf16 bits --
//     bit for bit bn_act_kernel<ADD>'s `fmaxf(x * s + t + z, 0)` -> bf16 -- then 16 bytes to LDS and (column tile 0) 16 bytes to y_k;
//   * (scale, shift) of all Cin <= 2048 channels in LDS (16 KB), workgroup 0 updates bn3's running statistics / clears the other
//     parity's accumulators (what the normalise + add launch did).
// K order, MFMA, epilogue and BatchNorm column sums are conv_aw_kernel's: given the same y_k the output tensor and the statistics are
// bit-identical to it (statistics signature 5000).  y_k may alias the raw conv3 tensor (in place) when one column tile covers Cout:
// every chunk is then read and written by the same thread, in that order.
template <int NW, int PDA>
__global__ __launch_bounds__(NW * 64, 2) void conv_ay_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = NW * 32, NT = NW * 64;
    constexpr int ABUF = BM * 128;                          // one K-step of A: 128 rows x 64 channels
    constexpr int CROW = BN * 2 + 16;
    constexpr int NJ = BM * 8 / NT;                         // 16-byte chunks of a stage per thread and stream (4 / 2), rows RJ apart
    constexpr int RJ = NT / 8;
    constexpr int TABB = 2 * 2048 * 4;                      // (scale, shift) of up to 2048 input channels
    constexpr int SMEM = (2 * ABUF + TABB > BM * CROW) ? 2 * ABUF + TABB : BM * CROW;      // the epilogue's bf16 tile overlays everything
    __shared__ __attribute__((aligned(16))) char smem[SMEM];
    float* in_tab = (float*)(smem + 2 * ABUF);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int tile = xcd_tile();
    const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;      // the column tiles of a row tile share an XCD's L2
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int nk = p.Cin >> 6;                                // K-steps of 64 channels: a multiple of PDA, >= 2 PDA (ay_ok)
    const bool write_y = tile_n == 0;                         // (uniform per workgroup)

    // ---- this thread's share of a stage: 16-byte chunk slot lc of rows r0 + RJ j; it fetches logical chunk lc ^ ((row >> 1) & 7)
    //      (the same for all its rows), so the LDS image is the ring kernel's.  Rows past M: an offset past the buffers (loads read 0,
    //      stores are dropped) ----
    const int lc = tid & 7, r0 = tid >> 3;
    const int sw0 = swz_of(r0);
    const __amdgpu_buffer_rsrc_t xsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.A), 0, (int)(p.in_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t zsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.in_res), 0, (int)(p.in_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t ysrc = __builtin_amdgcn_make_buffer_rsrc(p.Y, 0, (int)(p.in_bytes), 0x00020000);
    int a_voff[NJ];
    unsigned a_ok = 0u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int grow = m0 + r0 + RJ * j;
        const bool ok = grow < p.M;
        a_voff[j] = ok ? (int)(((long)grow * p.Cin + ((lc ^ sw0) << 3)) * 2) : 0x7ffffff0;
        if (ok) a_ok |= 1u << j;
    }
    u32x4 ax[PDA][NJ], az[PDA][NJ];
    auto load_stage = [&](int g, u32x4 (&dx)[NJ], u32x4 (&dz)[NJ]) {
        const int gs = g * 128;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            dx[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrc, a_voff[j], gs, 0));
            dz[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(zsrc, a_voff[j], gs, 0));
        }
    };

    // ---- this wave's weight stream: nk K-steps of 4 KB, fragment ordered; two K-steps ahead ----
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>((const char*)p.Bp + (long)((n0 >> 5) + wave) * nk * 4096), 0, nk * 4096, 0x00020000);
    const int wlane = lane * 16;
    auto load_b = [&](int g, int ks) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wsrc, wlane, g * 4096 + ks * 1024, 0));
    };

    // ---- prologue: everything is requested first ----
#pragma unroll
    for (int s = 0; s < PDA; ++s) load_stage(s, ax[s], az[s]);
    bf16x8 bq[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bq[s][ks] = load_b(s, ks);

    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;

    // bn3's (scale, shift) of all Cin channels into LDS once (bn_table's arithmetic, sat_bn_stats.h)
    {
        conv_in_table<NT>(p, in_tab);
        lds_barrier();      // (not __syncthreads: that would also wait for every load in flight)
    }
    // a landed stage on its way to LDS (and to y): relu(x * scale + shift + z) per channel; rows past M stay zero
    auto store_stage = [&](int g, int buf, u32x4 (&sx)[NJ], u32x4 (&sz)[NJ]) {
        char* at0 = smem + buf * ABUF + r0 * 128 + (lc << 4);
        const float* ts = in_tab + g * 64 + ((lc ^ sw0) << 3);
        const f32x4 s0 = *(const f32x4*)ts, s1 = *(const f32x4*)(ts + 4);
        const f32x4 t0 = *(const f32x4*)(ts + p.Cin), t1 = *(const f32x4*)(ts + p.Cin + 4);
        const int gs = g * 128;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            u32x4 w = sx[j];
            const u32x4 z = sz[j];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x2 sc2, sh2, f, zz;
                sc2[0] = q < 2 ? s0[2 * q] : s1[2 * q - 4]; sc2[1] = q < 2 ? s0[2 * q + 1] : s1[2 * q - 3];
                sh2[0] = q < 2 ? t0[2 * q] : t1[2 * q - 4]; sh2[1] = q < 2 ? t0[2 * q + 1] : t1[2 * q - 3];
                f[0] = __uint_as_float(w[q] << 16);
                f[1] = __uint_as_float(w[q] & 0xffff0000u);
                zz[0] = __uint_as_float(z[q] << 16);
                zz[1] = __uint_as_float(z[q] & 0xffff0000u);
                f = __builtin_elementwise_fma(f, sc2, sh2);
                f[0] = f[0] + zz[0];
                f[1] = f[1] + zz[1];
                const s16x2 pk = __builtin_bit_cast(s16x2, __builtin_convertvector(f, bf16x2));
                const s16x2 zero2 = {0, 0};
                w[q] = ((a_ok >> j) & 1u) ? __builtin_bit_cast(unsigned int, __builtin_elementwise_max(pk, zero2)) : 0u;
            }
            *(u32x4*)(at0 + j * (RJ * 128)) = w;
            if (write_y) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int, w), ysrc, a_voff[j], gs, 17);
        }
    };

    // A fragment addresses, K-invariant: row i*32 + r (the four row blocks 4096 B apart, same swizzle), chunk (2 ks + h) ^ ((r >> 1) & 7)
    int a_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a_off[ks] = frag_off(r, h, ks);

    store_stage(0, 0, ax[0], az[0]);
    load_stage(PDA, ax[0], az[0]);

    // K-step g, U = g % PDA (compile time): stage g sits in LDS buffer U & 1 (its last readers, K-step g - 2 ... no: the OTHER buffer's
    // last readers, K-step g - 1, are behind this step's barrier); stage g + 1 leaves register slot (U + 1) % PDA for the other
    // buffer, and the slot takes stage g + 1 + PDA; the weight registers of K-step g (slot U & 1) are refilled with K-step g + 2
    auto step = [&](int g, auto u_tag, auto st_tag, auto al_tag, auto bl_tag) {
        constexpr int U = decltype(u_tag)::value, LB = U & 1, S1 = (U + 1) % PDA;
        constexpr bool ST = decltype(st_tag)::value, AL = decltype(al_tag)::value, BL = decltype(bl_tag)::value;
        lds_barrier();      // this wave's LDS writes of stage g and everybody's; everybody is done reading K-step g - 1
        if constexpr (ST) store_stage(g + 1, LB ^ 1, ax[S1], az[S1]);
        if constexpr (AL) load_stage(g + 1 + PDA, ax[S1], az[S1]);
        const char* st = smem + LB * ABUF;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 fa[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[i] = *(const bf16x8*)(st + a_off[ks] + i * 4096);
            const bf16x8 b = bq[LB][ks];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], b, acc[i], 0, 0, 0);
            if constexpr (BL) bq[LB][ks] = load_b(g + 2, ks);
        }
    };
    // groups of PDA K-steps; kind 0: everything it requests exists; 1: the second-to-last group (its last step's stage g + 1 + PDA
    // lies past the end); 2: the last group (no stages to request, no stage nk to store, no weights past K-step nk - 1)
    auto group = [&](int g, auto kind_tag) {
        constexpr int KIND = decltype(kind_tag)::value;
        auto one = [&](auto u_tag) {
            constexpr int U = decltype(u_tag)::value;
            step(g + U, u_tag, std::integral_constant<bool, (KIND < 2 || U < PDA - 1)>{},
                 std::integral_constant<bool, (KIND == 0 || (KIND == 1 && U < PDA - 1))>{},
                 std::integral_constant<bool, (KIND < 2 || U < PDA - 2)>{});
        };
        one(std::integral_constant<int, 0>{});
        one(std::integral_constant<int, 1>{});
        if constexpr (PDA == 4) {
            one(std::integral_constant<int, 2>{});
            one(std::integral_constant<int, 3>{});
        }
    };
    int g = 0;
    for (; g < nk - 2 * PDA; g += PDA) group(g, std::integral_constant<int, 0>{});
    group(g, std::integral_constant<int, 1>{});
    group(g + PDA, std::integral_constant<int, 2>{});

    lds_barrier();      // every wave's LDS traffic is done before the buffers become the tile

    // ---- epilogue: BatchNorm column sums (a lane holds 64 of a column's 128 rows, then lane_halves), bf16 tile through LDS (acc_row) ----
    const int colw = wave * 32 + r;
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
        s += __shfl_xor(s, 32, 64);
        q += __shfl_xor(q, 32, 64);
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
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = acc_row(i, e, h);
            *(bf16_t*)(smem + row * CROW + colw * 2) = (bf16_t)acc[i][e];
        }
    lds_barrier();
    constexpr int ITS = BM * (BN / 8) / NT;
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
        const int qid = tid + it * NT;
        const int row = qid / (BN / 8), cc = qid % (BN / 8);
        const int grow = m0 + row, gcol = n0 + cc * 8;
        if (grow < p.M && gcol < p.N) store16_wt(p.C + (long)grow * p.ldc + gcol, *(const u32x4*)(smem + row * CROW + cc * 16));
    }
}

// 1x1 / stride 1 / no padding on a dense NHWC tensor, the operand = relu(bn(in0) + in1) written to out1 as well; Cin a multiple of
// 64 PDA in [128 PDA, 2048], Cout a multiple of the tile width, the fragment-ordered copy of the weights, tensors a 32-bit byte offset
// can address; y may alias the raw tensor only when one column tile covers Cout
bool ay_ok(const ConvArgs& a, int nw) {
    const int pda = nw == 8 ? 4 : 2;
    return a.in_res != nullptr && a.Y != nullptr && a.Bp != nullptr && a.KH == 1 && a.KW == 1 && a.linear && a.K == a.Cin &&
           (a.Cin % (64 * pda)) == 0 && a.Cin >= 128 * pda && a.Cin <= 2048 && (a.N % (nw * 32)) == 0 && a.in_affine && !a.out_scale &&
           !a.residual && a.in_bytes > 0 && a.in_bytes < 0x7ffffff0L && ((const void*)a.Y != (const void*)a.A || a.N == nw * 32) &&
           (const void*)a.Y != (const void*)a.in_res;
}

template <int NW>
int launch_ay(ConvArgs& a, int groups, hipStream_t s) {
    if (!ay_ok(a, NW)) return SAT_ERR_UNSUPPORTED;
    a.tiles_n = a.N / (NW * 32);
    return launch_conv(conv_ay_kernel<NW, NW == 8 ? 4 : 2>, dim3(sat_cdiv(a.M, 128) * a.tiles_n, groups), dim3(NW * 64), 0, s, a);
}
