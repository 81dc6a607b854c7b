// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the LDS-DMA helpers and the variant table).
//
// 3x3 / stride 1 / pad 1 convolution (conv2 of a bottleneck, `self.resnet(images)`, models.py:27) with the INPUT PATCH RESIDENT IN LDS.
//
// Why: conv_glds_kernel stages, for every K-step (one filter tap x 64 input channels), 16 KB of activations next to 16 KB of
// weights, and its K loop runs at the rate the LDS-DMA ring can keep bytes in flight (~0.6 us per K-step at 96 KB in flight,
// 25 us / 582 TFLOP/s for the layer-3 conv2) -- but the nine taps of a channel block read the SAME pixels, shifted.  On a dense
// NHWC tensor the input pixel of output row m (flattened n, h, w) and tap (kh, kw) is row m + (kh-1) W + (kw-1): the rows a
// 128-row tile needs form ONE contiguous range of 128 + 2W + 2 pixels.  So:
//   * a 64-channel slice of that range (the "patch", <= 192 rows x 128 B = 24 KB) is loaded ONCE per channel block by LDS-DMA,
//     double buffered, in the ring's XOR-swizzled row image; the A fragments of tap (kh, kw) are read from it at row
//     r + kh W + kw -- consecutive lanes still read consecutive rows, so the reads stay conflict free;
//   * zero padding and image borders: a per-row 9-bit tap mask (computed once) redirects the lane to a 128-byte row of zeros;
//   * only the weights stream through the ring (16 KB per K-step, 6 slots, 5 in flight): L2 -> LDS traffic per K-step drops
//     from 32 KB to 16 KB + 24/9 KB;
//   * the K axis is walked channel block major (all nine taps of block 0, then block 1, ...) instead of tap major: the same
//     products, another f32 summation order than conv_glds_kernel (results equal to rounding, not bitwise);
//   * 4 consumer waves (64x64 accumulators each) + 4 loader waves, one raw barrier per K-step, counted vmcnt -- the protocol of
//     the wave-specialised ring kernel; the patch pieces of the next channel block ride in the loaders' queue behind the weight
//     stage of the block's first K-step (the counted wait accounts for them for the next D steps).
template <int S, int PRP, bool AFF>      // ring slots; patch pieces of 8 rows (20: W <= 15, seven slots fit; 24: W <= 31, six); AFF: BatchNorm + ReLU of the input
__global__ __launch_bounds__(512) void conv_pr_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = 128, NT = 512, D = S - 1, SLOT = BN * 128;
    constexpr int PBUF = PRP * 8 * 128;                    // patch buffer: PRP pieces of 8 rows x 128 B
    constexpr int NBI = 4, PPL = PRP / 4;                   // LDS-DMA pieces per loader wave: weight stage / patch slice
    constexpr int ZROW = 2 * PBUF, RING = 2 * PBUF + 128;
    constexpr int CROW = BN * 2 + 16;
    static_assert(BM * CROW + 4 * 2 * BN * 4 <= S * SLOT, "epilogue tile + stat scratch must fit the ring");
    static_assert(D >= 2 && D <= 7, "the next patch must land (and be transformed) within its nine K-steps");
    constexpr int TAB = RING + S * SLOT;                    // AFF: (scale, shift) of up to 512 input channels
    __shared__ __attribute__((aligned(16))) char smem[TAB + (AFF ? 4096 : 0)];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool is_loader = wave >= 4;
    const int lw = wave & 3;
    const int wm = (wave >> 1) & 1, wn = wave & 1;           // consumers (waves 0-3): 2 x 2
    const int r = lane & 31, h = lane >> 5;

    const int tile = xcd_tile();
    const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int W = p.Win;
    const int NCB = p.Cin >> 6;                               // 64-channel blocks
    const int G = NCB * 9;                                    // K-steps
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    if (tid < 8) *(u32x4*)(smem + ZROW + tid * 16) = u32x4{0u, 0u, 0u, 0u};

    // ---- loader state ----
    const bf16_t* b_ptr[NBI];
    const bf16_t* p_ptr[PPL];
    int p_step[PPL];
#pragma unroll
    for (int i = 0; i < NBI; ++i) {
        const int row = (lw * NBI + i) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((row >> 1) & 7);
        b_ptr[i] = (n0 + row < p.N) ? p.B + ((long)(n0 + row) * p.ldb + ch * 8) : nullptr;
    }
    const int PR = BM + 2 * W + 2;                            // patch rows in use: flat pixels m0 - (W+1) .. m0 + BM + W
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int prow = (lw * PPL + j) * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((prow >> 1) & 7);
        const long flat = (long)m0 - (W + 1) + prow;
        const bool ok = prow < PR && flat >= 0 && flat < p.M;
        p_ptr[j] = ok ? p.A + (flat * p.sW + ch * 8) : zero;
        p_step[j] = ok ? 64 : 0;
    }
    auto issue_patch = [&](int buf) {                          // the next 64-channel slice of the patch
        char* dst = smem + buf * PBUF + lw * PPL * 8 * 128;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            __builtin_amdgcn_global_load_lds((gptr_t)p_ptr[j], (lptr_t)(dst + j * 8 * 128), 16, 0, 0);
            p_ptr[j] += p_step[j];
        }
    };
    int is_g = 0, is_tap = 0, is_cb = 0;                      // the next weight stage to issue: K-step is_g = (block is_cb, tap is_tap)
    auto issue_b = [&](int slot) {
        char* dst = smem + RING + slot * SLOT + lw * NBI * 8 * 128;
        const long koff = (long)is_tap * p.Cin + is_cb * 64;
        const bool live = is_g < G;                           // beyond the K range: zero-source dummies keep the counts uniform
#pragma unroll
        for (int i = 0; i < NBI; ++i) {
            const bf16_t* src = (live && b_ptr[i]) ? b_ptr[i] + koff : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(dst + i * 8 * 128), 16, 0, 0);
        }
        ++is_g;
        if (++is_tap == 9) { is_tap = 0; ++is_cb; }
    };

    // ---- consumer state: tap validity per row (bit t = tap t inside the image), patch row of tap (0, 0) ----
    unsigned a_mask[2];
    int a_row[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + i * 32 + r;
        const int grow = m0 + row;
        a_row[i] = row;
        a_mask[i] = 0u;
        if (grow < p.M) {
            const int hw = p.Hout * p.Wout;
            const int n = grow / hw;
            const int rem = grow - n * hw;
            const int ho = rem / p.Wout;
            const int wo = rem - ho * p.Wout;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const bool in = ((unsigned)(ho + kh - 1) < (unsigned)p.Hin) && ((unsigned)(wo + kw - 1) < (unsigned)p.Win);
                    a_mask[i] |= (in ? 1u : 0u) << (kh * 3 + kw);
                }
        }
    }
    int b_off[4];                                              // B fragment offsets: row = wn*64 + j*32 + r, (row>>1)&7 = (r>>1)&7
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) b_off[ks] = (wn * 64 + r) * 128 + (swz_chunk(2 * ks + h, r) << 4);      // frag_off of row wn*64 + r, whose swizzle is r's

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // AFF (bn1 + ReLU of the operand, `self.resnet(images)`: torchvision Bottleneck's relu(bn1(conv1(x))) feeding conv2): the raw conv1
    // output is the patch source and the transform is applied to each 64-channel slice ONCE, in LDS, by the loader waves (idle
    // otherwise) -- 20-24 KB per channel block instead of the 16 KB per K-step (nine times more) an in-ring transform touches.
    // Zero padding stays zero: padded taps read the zero row, never the patch.
    float* in_tab = (float*)(smem + (AFF ? TAB : 0));
    if constexpr (AFF) conv_in_table<NT>(p, in_tab);
    // loader lane ll = tid - 256 owns the 16-byte channel group lc = ll & 7 of rows (ll >> 3) + 32 j: (row >> 1) & 7 is the same for
    // all of them, so every address is one base plus an immediate
    auto xform_patch = [&](int buf, int cb) {
        const int ll = tid - 256, lc = ll & 7, r0 = ll >> 3;
        const float* ts = in_tab + cb * 64 + lc * 8;
        const InTab tab = in_tab_fetch(ts, p.Cin);
        char* at0 = smem + buf * PBUF + r0 * 128 + ((lc ^ ((r0 >> 1) & 7)) << 4);
        u32x4 w[PRP / 4];
#pragma unroll
        for (int j = 0; j < PRP / 4; ++j) w[j] = *(const u32x4*)(at0 + j * 4096);
#pragma unroll
        for (int j = 0; j < PRP / 4; ++j) {
            w[j] = bn_relu_chunk(w[j], tab);
            *(u32x4*)(at0 + j * 4096) = w[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };

    // Protocol (one raw s_barrier per K-step, loaders and consumers in SEPARATE loops with the same barrier count):
    //   loader  : wait until its pieces of stage g+1 have landed -> barrier g -> issue stage g+D into the slot stage g-1 occupied
    //             (+ the next patch slice behind the first stage of a channel block)
    //   consumer: barrier g -> MFMAs of stage g, every fragment read one substep ahead; the LAST substep prefetches the first
    //             fragments of stage g+1 (landed: that is what the loaders' wait covers), so no LDS latency follows a barrier
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the zero row
    if (is_loader) {
        issue_patch(0);
#pragma unroll
        for (int s = 0; s < D; ++s) issue_b(s);
        wait_vmcnt<(D - 1) * NBI>();                           // the patch and stage 0
        raw_barrier();
        if constexpr (AFF) {                                   // slice 0 (every loader's pieces have landed) before anybody reads it
            xform_patch(0, 0);
            raw_barrier();
        }
        int slot = 0;
        for (int cb = 0; cb < NCB; ++cb) {
            const bool has_next = cb + 1 < NCB;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                // the patch pieces queue behind stage g_p + D (g_p = the block's first K-step): they are YOUNGER than the stage
                // this wait is about (g + 1) for t = 1 .. D-1, older (hence covered) from t = D on
                if (t >= 1 && t <= D - 1 && has_next) wait_vmcnt<(D - 2) * NBI + PPL>();
                else wait_vmcnt<(D - 2) * NBI>();
                raw_barrier();
                issue_b(slot == 0 ? S - 1 : slot - 1);
                if (t == 0 && has_next) issue_patch((cb + 1) & 1);
                // the next slice has landed for EVERY loader once barrier t = D is passed (each covered its own pieces in the wait
                // before it); the consumers first read it after barrier t = 8
                if constexpr (AFF) { if (t == D && has_next) xform_patch((cb + 1) & 1, cb + 1); }
                slot = (slot + 1 == S) ? 0 : slot + 1;
            }
        }
    } else {
        raw_barrier();
        if constexpr (AFF) {
            raw_barrier();
        }
        // fragment addresses of (patch buffer, tap): the A row of lane (r, h) is patch row r + kh W + kw, or the zero row
        auto a_addr = [&](const char* pb, int t, int i, const char*& base, int& sw) {
            const bool ok = (a_mask[i] >> t) & 1u;
            const int prow = a_row[i] + (t / 3) * W + (t % 3);
            base = ok ? pb + prow * 128 : smem + ZROW;
            sw = ok ? ((prow >> 1) & 7) : 0;
        };
        const char* ab0; const char* ab1; int sw0, sw1;
        a_addr(smem, 0, 0, ab0, sw0);
        a_addr(smem, 0, 1, ab1, sw1);
        // fragments are read TWO substeps (8 MFMAs, ~256 matrix-pipe clocks) ahead of their use: one substep (128 clocks) does
        // not cover a ds_read_b128 under four consumer waves and the loaders' LDS-DMA writes
        struct Frag { bf16x8 a0, a1, b0, b1; };
        auto load_frag = [&](const char* a0p, int s0, const char* a1p, int s1, const char* bp, int ks) {
            Frag f;
            f.a0 = *(const bf16x8*)(a0p + (((2 * ks + h) ^ s0) << 4));
            f.a1 = *(const bf16x8*)(a1p + (((2 * ks + h) ^ s1) << 4));
            f.b0 = *(const bf16x8*)(bp + b_off[ks]);
            f.b1 = *(const bf16x8*)(bp + b_off[ks] + 4096);
            return f;
        };
        Frag f0 = load_frag(ab0, sw0, ab1, sw1, smem + RING, 0), f1 = load_frag(ab0, sw0, ab1, sw1, smem + RING, 1);
        int slot = 0;
        for (int cb = 0; cb < NCB; ++cb) {
            const char* pb = smem + (cb & 1) * PBUF;
            const char* pbn = smem + ((cb + 1) & 1) * PBUF;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                raw_barrier();
                const char* sb = smem + RING + slot * SLOT;
                const int nslot = (slot + 1 == S) ? 0 : slot + 1;
                const char* sbn = smem + RING + nslot * SLOT;
                // next step's A rows (tap t+1 of this block, or tap 0 of the next block's buffer)
                const char* nb0; const char* nb1; int nsw0, nsw1;
                a_addr(t == 8 ? pbn : pb, t == 8 ? 0 : t + 1, 0, nb0, nsw0);
                a_addr(t == 8 ? pbn : pb, t == 8 ? 0 : t + 1, 1, nb1, nsw1);
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const Frag f2 = ks < 2 ? load_frag(ab0, sw0, ab1, sw1, sb, ks + 2) : load_frag(nb0, nsw0, nb1, nsw1, sbn, ks - 2);
                    // (the scheduler would sink the reads back under the MFMAs that use them: fewer registers, exposed LDS latency)
                    __builtin_amdgcn_sched_barrier(0);
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0.a0, f0.b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0.a0, f0.b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0.a1, f0.b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0.a1, f0.b1, acc[1][1], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    f0 = f1; f1 = f2;
                }
                ab0 = nb0; ab1 = nb1; sw0 = nsw0; sw1 = nsw1;
                slot = nslot;
            }
        }
    }
    // drain the dummy prefetches and let every wave finish its last reads before the ring is reused
    wait_vmcnt<0>();
    __syncthreads();

    // ---- epilogue: BatchNorm column sums from the f32 accumulators (lane_halves, then the M-waves in order), bf16 tile through LDS (acc_row) ----
    char* ring = smem + RING;
    float* red = (float*)(ring + BM * CROW);                  // [2 (wm)][2][BN]
    if ((p.stat_partial || p.acc) && !is_loader) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = acc[i][j][e];
                    s += v;
                    q += v * v;
                }
            s += __shfl_xor(s, 32, 64);
            q += __shfl_xor(q, 32, 64);
            if (h == 0) {
                red[(wm * 2 + 0) * BN + wn * 64 + j * 32 + r] = s;
                red[(wm * 2 + 1) * BN + wn * 64 + j * 32 + r] = q;
            }
        }
    }
    if (!is_loader) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wn * 64 + j * 32 + r;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = wm * 64 + acc_row(i, e, h);
                    *(bf16_t*)(ring + row * CROW + col * 2) = (bf16_t)acc[i][j][e];
                }
        }
    }
    __syncthreads();
    for (int c = tid; c < BN; c += NT) {
        const int col = n0 + c;
        if (col < p.N && (p.acc || p.stat_partial)) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int g = 0; g < 2; ++g) {                      // fixed order over the M-waves
                s += red[(g * 2 + 0) * BN + c];
                q += red[(g * 2 + 1) * BN + c];
            }
            if (p.acc) {
                stat_acc_add(p.acc, p.N, s, q, col);
            }
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, tile_m, p.N, s, q, col);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < BM * 16 / NT; ++it) {
        const int qid = tid + it * NT;
        const int row = qid >> 4, cc = qid & 15;
        const int grow = m0 + row, gcol = n0 + cc * 8;
        if (grow < p.M && gcol < p.N) store16_wt(p.C + (long)grow * p.ldc + gcol, *(const u32x4*)(ring + row * CROW + cc * 16));
    }
}

// dense NHWC 3x3 / stride 1 / pad 1, Cin a multiple of 64, a patch of 128 + 2W + 2 rows within the 192-row buffer
bool pr_ok(const ConvArgs& a) {
    return a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.padw == 1 && a.Hout == a.Hin && a.Wout == a.Win &&
           (a.Cin % 64) == 0 && a.K == 9 * a.Cin && a.ldb == a.K && a.sW == a.Cin && a.sH == (long)a.Win * a.sW &&
           a.sN == (long)a.Hin * a.sH && 128 + 2 * a.Win + 2 <= 192 && a.N >= 128 && (a.N % 8) == 0 && (!a.in_affine || a.Cin <= 512) &&
           !a.residual && !a.out_scale;
}

int launch_pr(ConvArgs& a, int groups, hipStream_t s) {
    if (!pr_ok(a)) return SAT_ERR_UNSUPPORTED;
    a.tiles_n = sat_cdiv(a.N, 128);
    const bool small = 128 + 2 * a.Win + 2 <= 160;      // the smaller patch leaves room for a seventh ring slot: one more weight stage in flight
    const ConvKernel k = small ? (a.in_affine ? conv_pr_kernel<7, 20, true> : conv_pr_kernel<7, 20, false>)
                               : (a.in_affine ? conv_pr_kernel<6, 24, true> : conv_pr_kernel<6, 24, false>);
    return launch_conv(k, dim3(sat_cdiv(a.M, 128) * a.tiles_n, groups), dim3(512), 0, s, a);
}
