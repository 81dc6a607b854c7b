// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the LDS-DMA helpers and the variant table).
//
// "Expansion" 1x1 convolution (conv3 of a bottleneck, `self.resnet(images)`, models.py:27: K = planes <= 256 input channels,
// N = 4 * planes output channels) with the ACTIVATION PANEL RESIDENT IN REGISTERS.
//
// Why: as a 128x128-tile GEMM this conv is four K-steps long.  A workgroup of conv_glds_kernel lives ~14 us for < 1 us of
// matrix work: table build, ring prologue, four exposed load round trips, the in-LDS BatchNorm+ReLU pass of the operand per
// K-step per column tile, epilogue -- none of it overlapped with anything but a second workgroup on the CU (22.4 us, 293
// TFLOP/s at M = 12544, N = 1024, K = 256).  Here a workgroup owns 128 rows x CT column tiles:
//   * its A operand (128 x K, at most 64 KB) is loaded ONCE, straight from global memory into MFMA fragment registers
//     (lane (r, h) of a 32x32x16 fragment holds 16 contiguous bytes of row r: one global_load_dwordx4), the fused
//     BatchNorm + ReLU of the operand (bn2) is applied ONCE in registers, and it never touches LDS;
//   * the weights stream through a 5-slot x 16 KB LDS ring (LDS-DMA, XOR-swizzled image, counted vmcnt, one raw barrier per
//     K-step) that keeps running ACROSS column tiles, so only the first K-step of a workgroup sees a cold load;
//   * LDS traffic per MFMA halves (only B fragments are read), and there is no per-K-step transform pass or second barrier;
//   * the epilogue of a column tile (BatchNorm column sums -> integer atomics, bf16 tile -> write-through stores) uses the
//     three ring slots that are idle at that moment and is issued by waves 2-3 only, while waves 0-1 own every LDS-DMA and
//     its counted wait: a wave's memory counter retires in order, so a store acknowledgement never sits in front of a
//     prefetch (the rule the dual-source kernel established);
//   * 80 KB of LDS and <= 256 registers: two workgroups per CU, one wave of each per SIMD.
// Arithmetic is that of conv_glds_kernel on the same geometry: the same MFMA, the same K order, the same per-tile column-sum
// order as its 128-row tiles, the same operand transform expression -- the output tensor is bit-identical.
template <int NK, bool AFF>      // K / 64; AFF: BatchNorm + ReLU of the operand (a template flag keeps the panel's registers in place)
__global__ __launch_bounds__(256, 2) void conv_xp_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = 128, NT = 256, RS = 5, D = 2, SLOT = BN * 128, KS = NK * 4;
    __shared__ __attribute__((aligned(16))) char smem[RS * SLOT];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_loader = wave < 2;
    const int lw = wave & 1;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int CT = p.ct;

    const int tile = xcd_tile();
    const int tile_m = tile / p.tiles_n, ns = tile - tile_m * p.tiles_n;      // tiles_n = column splits: N / (CT * 128)
    const int m0 = tile_m * BM, nbase = ns * CT * BN;
    const int G = CT * NK;                                                   // weight stages of this workgroup

    // ---- weight loader state (waves 0-1): piece i = rows lw*64 + i*8 .. +7 of the stage, lane = (row l>>3, LDS chunk slot l&7);
    //      it fetches logical chunk (l&7) ^ ((row>>1)&7) and (row>>1)&7 = ((i&1)*4 + (l>>4)) for these rows ----
    const int ch_even = (lane & 7) ^ (lane >> 4);
    const bf16_t* b_even = p.B + ((long)(nbase + lw * 64 + (lane >> 3)) * p.ldb + ch_even * 8);
    const bf16_t* b_odd = p.B + ((long)(nbase + lw * 64 + (lane >> 3)) * p.ldb + (ch_even ^ 4) * 8);
    auto issue = [&](int slot, long koff) {
        char* dst = smem + slot * SLOT + lw * 64 * 128;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bf16_t* src = ((i & 1) ? b_odd : b_even) + koff + (long)(i * 8) * p.ldb;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + i * 8 * 128), 16, 0, 0);
        }
    };
    // offset of stage g = (column tile g / NK, K-step g % NK) inside the weight matrix, walked incrementally
    int is_ct = 0, is_kt = 0;
    auto issue_next = [&](int slot) {
        issue(slot, (long)is_ct * BN * p.ldb + is_kt * 64);
        if (++is_kt == NK) { is_kt = 0; ++is_ct; }
    };
    // ---- the A panel goes global -> LDS by LDS-DMA (coalesced: 8 rows x 128 B per wave instruction; a per-lane gather of MFMA
    //      fragments costs the texture path ~64 clocks per instruction, 4 us per workgroup, and starves the weight ring of the
    //      OTHER workgroup on the CU), K-step kt into slot kt with the ring's XOR-swizzled image; rows past M read the zero word ----
    const bf16_t* zero = (const bf16_t*)&g_zero16;
    constexpr int NAP = NK * 16 / 4;                     // 8-row pieces per wave
    // the kernel is instruction-issue bound (two workgroups share every SIMD), so the address work is kept off the vector ALU:
    // (row>>1)&7 of row pr*8 + (lane>>3) is (pr&1)*4 + (lane>>4) -- two lane bases, everything else is a scalar offset
    const bool full_tile = m0 + BM <= p.M;               // uniform
    const bf16_t* a_even = p.A + ((long)(m0 + (lane >> 3)) * p.sW + ch_even * 8);
    const bf16_t* a_odd = p.A + ((long)(m0 + (lane >> 3)) * p.sW + (ch_even ^ 4) * 8);
#pragma unroll
    for (int i = 0; i < NAP; ++i) {
        const int piece = wave * NAP + i;                // wave-uniform
        const int kt = piece >> 4, pr = piece & 15;
        const bf16_t* src = ((pr & 1) ? a_odd : a_even) + ((long)(pr * 8) * p.sW + kt * 64);
        if (!full_tile && m0 + pr * 8 + (lane >> 3) >= p.M) src = zero;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(smem + kt * SLOT + pr * 8 * 128), 16, 0, 0);
    }
    // ---- (scale, shift) of the operand's BatchNorm into slot 4 (same arithmetic as conv_glds_kernel) while the panel is in flight ----
    float* in_tab = (float*)(smem + 4 * SLOT);
    if constexpr (AFF) conv_in_table<NT>(p, in_tab);
    // the panel has landed and the table is visible
    wait_vmcnt<0>();
    lds_barrier();
    if constexpr (AFF) {
        // BatchNorm + ReLU of the panel, ONCE, in LDS, every thread on one 16-byte channel group (logical chunk lc of the K axis)
        // for 128 / RPT rows: its eight (scale, shift) pairs live in registers
        constexpr int LCN = NK * 8, RPT = NT / LCN;      // channel groups; row stride of a thread
        const int lc = tid % LCN, row0 = tid / LCN;
        // (not in_tab_fetch: its shift address, table + lc * 8 + Cin, is summed in another order than this one and costs the kernel an instruction)
        const InTab tab = {*(const f32x4*)(in_tab + lc * 8), *(const f32x4*)(in_tab + lc * 8 + 4), *(const f32x4*)(in_tab + p.Cin + lc * 8),
                           *(const f32x4*)(in_tab + p.Cin + lc * 8 + 4)};
        lds_barrier();      // every thread holds its table entries: slot 4 may take weight stage 0
        if (is_loader) issue_next(4);
        // rows row0 + jr*RPT: for RPT = 8 the swizzle term ((row>>1)&7) alternates between two values, for RPT >= 16 it is
        // constant -- two lane bases and immediate offsets, no per-row address arithmetic
        char* at_e = smem + (lc >> 3) * SLOT + row0 * 128 + (((lc & 7) ^ ((row0 >> 1) & 7)) << 4);
        char* at_o = smem + (lc >> 3) * SLOT + row0 * 128 + (((lc & 7) ^ (((row0 + RPT) >> 1) & 7)) << 4);
        auto xform = [&](u32x4 w) { return bn_relu_chunk(w, tab); };
        constexpr int NCH = BM / RPT;                    // chunks per thread
        if (full_tile) {                                 // uniform: straight-line code, all the reads in flight at once
            u32x4 w[NCH];
#pragma unroll
            for (int jr = 0; jr < NCH; ++jr) w[jr] = *(const u32x4*)(((jr & 1) ? at_o : at_e) + jr * RPT * 128);
#pragma unroll
            for (int jr = 0; jr < NCH; ++jr) *(u32x4*)(((jr & 1) ? at_o : at_e) + jr * RPT * 128) = xform(w[jr]);
        } else {
#pragma unroll 1
            for (int jr = 0; jr < NCH; ++jr) {
                char* at = ((jr & 1) ? at_o : at_e) + jr * RPT * 128;
                if (m0 + row0 + jr * RPT < p.M) *(u32x4*)at = xform(*(const u32x4*)at);      // rows past M stay exact zeros
            }
        }
        lds_barrier();
    } else {
        if (is_loader) issue_next(4);
    }
    // ---- fragments: lane (r, h) of tile i holds row wm*64 + i*32 + r, chunk 2*ks + h of K-step kt ----
    bf16x8 af[2][KS];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + i * 32 + r;
#pragma unroll
        for (int kt = 0; kt < NK; ++kt)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                af[i][kt * 4 + ks] = *(const bf16x8*)(smem + kt * SLOT + frag_off(row, h, ks));
    }
    lds_barrier();      // the panel's slots are free: the ring takes them
    if (is_loader && G > 1) issue_next(0);

    // B fragment read offsets inside a slot: row*128 + ((chunk ^ ((row>>1)&7)) * 16), chunk = 2*ks + h
    // (row = wn*64 + j*32 + r: (row>>1)&7 = (r>>1)&7 for both j, and j only adds 4096 bytes)
    int b_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) b_off[ks] = wn * 64 * 128 + frag_off(r, h, ks);

    f32x16 acc[2][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    };
    zero_acc();

    // stage g lives in slot (g + 4) % 5: stage 0 went into slot 4 while the panel occupied 0..3
    int slot = 4;
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int kt = 0; kt < NK; ++kt) {
            const int g = ct * NK + kt;
            // Ring protocol: loader waits until ITS pieces of stage g have landed (stage g+1 may still be in flight) -> barrier
            // (everybody's pieces have; everybody's reads of stage g-1 and of the previous epilogue's slots are done) ->
            // stage g+2 goes into the slot (g+2) % 5, free since stage g-3 / the epilogue scratch
            if (is_loader) {
                if (g + 1 < G) wait_vmcnt<8>();
                else wait_vmcnt<0>();
            }
            raw_barrier();
            if (is_loader && g + D < G) issue_next(slot + D >= RS ? slot + D - RS : slot + D);
            {
                const char* st = smem + slot * SLOT;
                bf16x8 b0 = *(const bf16x8*)(st + b_off[0]), b1 = *(const bf16x8*)(st + b_off[0] + 4096);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    bf16x8 n0 = b0, n1 = b1;
                    if (ks < 3) {
                        n0 = *(const bf16x8*)(st + b_off[ks + 1]);
                        n1 = *(const bf16x8*)(st + b_off[ks + 1] + 4096);
                    }
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][kt * 4 + ks], b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0][kt * 4 + ks], b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][kt * 4 + ks], b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1][kt * 4 + ks], b1, acc[1][1], 0, 0, 0);
                    b0 = n0; b1 = n1;
                }
            }
            const int cslot = slot;                          // the slot this step consumed
            slot = (slot + 1 == RS) ? 0 : slot + 1;
            if (kt == NK - 1) {
                // ---- epilogue of column tile ct: slots cslot, cslot-1 (C tile halves by wm) and cslot-2 (column-sum scratch) are
                //      idle; cslot+1 / cslot+2 hold the stages in flight ----
                char* c_half = smem + (wm == 0 ? cslot : (cslot + 4) % RS) * SLOT;
                float* red = (float*)(smem + ((cslot + 3) % RS) * SLOT);       // [2 (wm)][2][BN]
                lds_barrier();      // every wave has finished its reads of stage g
                if (p.stat_partial || p.acc) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        // two rows per instruction (v_pk_add_f32 / v_pk_fma_f32): even and odd rows are summed apart and joined
                        // once -- a fixed order, but not the ring kernel's (the totals differ in the last bits, like any other tile shape)
                        f32x2 s2 = {0.0f, 0.0f}, q2 = {0.0f, 0.0f};
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int e = 0; e < 16; e += 2) {
                                f32x2 v;
                                v[0] = acc[i][j][e];
                                v[1] = acc[i][j][e + 1];
                                s2 += v;
                                q2 = __builtin_elementwise_fma(v, v, q2);
                            }
                        float s = s2[0] + s2[1], q = q2[0] + q2[1];
                        lane_halves(s, q);
                        if (h == 0) {
                            red[(wm * 2 + 0) * BN + wn * 64 + j * 32 + r] = s;
                            red[(wm * 2 + 1) * BN + wn * 64 + j * 32 + r] = q;
                        }
                    }
                }
                // bf16 tile: 64 rows x 256 B per half.  Instead of padding, bit 2 of the 16-byte chunk index is XORed with bit 2 of
                // the row (= h for every element of a lane: rows are i*32 + (e&3) + 8*(e>>2) + 4h), so the two half-waves of a
                // write land 64 B apart and EVERYTHING lane-dependent is one base address: each element is a convert (two rows
                // per packed convert) and a ds_write_b16 with an immediate offset -- the kernel is VALU-issue bound, not LDS bound
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    char* cb = c_half + h * 1024 + ((wn * 8 + ((j ^ h) << 2) + (r >> 3)) << 4) + (r & 7) * 2;
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int e = 0; e < 16; e += 2) {
                            f32x2 f;
                            f[0] = acc[i][j][e];
                            f[1] = acc[i][j][e + 1];
                            const bf16x2 pk = __builtin_convertvector(f, bf16x2);
                            *(bf16_t*)(cb + i * 8192 + (e & 3) * 256 + (e >> 2) * 2048) = pk[0];
                            *(bf16_t*)(cb + i * 8192 + ((e + 1) & 3) * 256 + (e >> 2) * 2048) = pk[1];
                        }
                }
                zero_acc();
                lds_barrier();
                if (!is_loader) {
                    const int t = tid - 128;                 // 0..127
                    const int n0 = nbase + ct * BN;
                    {
                        float s = 0.0f, q = 0.0f;
#pragma unroll
                        for (int gm = 0; gm < 2; ++gm) {     // fixed order over the M-waves
                            s += red[(gm * 2 + 0) * BN + t];
                            q += red[(gm * 2 + 1) * BN + t];
                        }
                        if (p.acc) {
                            stat_acc_add(p.acc, p.N, s, q, n0, t);
                        }
                        if (p.stat_partial) {
                            stat_slab_store(p.stat_partial, tile_m, p.N, s, q, n0, t);
                        }
                    }
                    const char* c_lo = smem + cslot * SLOT;
                    const char* c_hi = smem + ((cslot + 4) % RS) * SLOT;
#pragma unroll 1
                    for (int io = 0; io < 16; io += 4) {      // four 16-byte pieces in flight per lane (registers are the A panel's)
                        u32x4 v[4];
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii) {
                            const int qd = t + (io + ii) * 128;
                            const int row = qd >> 4, cc = qd & 15;
                            const int rowl = row & 63;
                            v[ii] = *(const u32x4*)((row < 64 ? c_lo : c_hi) + rowl * 256 + ((cc ^ (rowl & 4)) << 4));
                        }
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii) {
                            const int qd = t + (io + ii) * 128;
                            const int row = qd >> 4, cc = qd & 15;
                            if (full_tile || m0 + row < p.M) {
                                // write-through: 17.6-18.0 us against 19.9 (write-back) and 18.6-18.9 (non-temporal) at the layer-3 geometry
                                store16_wt(p.C + (long)(m0 + row) * p.ldc + n0 + cc * 8, v[ii]);
                            }
                        }
                    }
                }
            }
        }
    }
}

// CT column tiles per workgroup; K in {64, 128, 256}; a dense 1x1 geometry whose N is a multiple of CT * 128
bool xp_ok(const ConvArgs& a, int ct) {
    return a.linear && (a.K == 64 || a.K == 128 || a.K == 256) && a.K == a.Cin && a.ldb == a.K && ct >= 1 &&
           a.N % (ct * 128) == 0 && !a.residual && !a.out_scale && (!a.in_affine || a.Cin <= 512);
}

template <int CT>
int launch_xp(ConvArgs& a, int groups, hipStream_t s) {
    if (!xp_ok(a, CT)) return SAT_ERR_UNSUPPORTED;
    a.ct = CT;
    a.tiles_n = a.N / (CT * 128);
    static constexpr ConvKernel kKernel[3][2] = {{conv_xp_kernel<1, false>, conv_xp_kernel<1, true>},      // [K / 128][in_affine]
                                                 {conv_xp_kernel<2, false>, conv_xp_kernel<2, true>},
                                                 {conv_xp_kernel<4, false>, conv_xp_kernel<4, true>}};
    return launch_conv(kKernel[a.K / 128][a.in_affine], dim3(sat_cdiv(a.M, 128) * a.tiles_n, groups), dim3(256), 0, s, a);
}
