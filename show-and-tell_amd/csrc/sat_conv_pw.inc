// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the LDS-DMA helpers and the variant table).
//
// 3x3 / stride 1 / pad 1 convolution (conv2 of a bottleneck, `self.resnet(images)`, models.py:27): the input patch resident in LDS
// (conv_pr_kernel's idea) and the WEIGHTS STRAIGHT INTO REGISTERS from a fragment-ordered copy.
//
// Why: conv_pr_kernel stages 16 KB of weights per K-step through a 6-7 slot LDS ring: 150 KB of LDS, one workgroup per CU, one
// consumer wave per SIMD -- and a launch of 196 G workgroups of equal length on 256 CUs runs in ceil(196 G / 256) rounds (measured,
// tools/microbench.py quant: 26 us at 256 workgroups, 44 us at 258; G = 2: 392 workgroups = 1.53 rounds cost 2).  The conv stack is
// frozen, so its weights can be laid out ONCE (sat_conv_pack_weights) exactly as the MFMA wants them:
//   packed[column block of 32][K-step g = (channel block, tap)][substep ks][lane][8 bf16]      (lane = (column r, K half h))
// -- the B fragment of a wave is one coalesced 1 KB global_load_dwordx4 (buffer form: scalar offset, no address arithmetic), and a
// wave that owns 32 columns and ALL 128 rows of the tile is the only reader of its slice: no LDS for the weights, no barrier per
// K-step, PD K-steps (PD x 4 KB per wave) in flight in registers.  What is left in LDS is the double-buffered input patch
// (40-48 KB): two workgroups per CU, two waves per SIMD that cover each other's LDS latency, barriers and BatchNorm transform, and a
// launch of up to 512 workgroups is ONE round.
//   * 4 waves, all alike: wave w owns columns [32 w, 32 w + 32) x 128 rows (four 32 x 32 accumulators); per substep 4 A fragments
//     from the patch (one row base + 4096 i: the four row blocks share the XOR swizzle) and 4 MFMAs against one B fragment;
//   * the patch is triple buffered (the slice being read, the next one, the one in flight): one barrier per channel block (nine
//     K-steps) hands the buffers over, a second one (AFF) follows the BatchNorm + ReLU transform of the next slice;
//   * K order = conv_pr_kernel's (channel block major, taps, substeps): the conv OUTPUT is bit-identical to conv_pr_kernel's;
//     the BatchNorm column sums are taken per lane over the 64 values of a column half, then across the halves (own signature).
//   * inference epilogue (fixed BatchNorm affine + ReLU, no residual: conv2 of a bottleneck) like the ring kernel's.
template <int PRP, bool AFF, int PD>      // patch pieces of 8 rows (20: W <= 15; 24: W <= 31); BatchNorm + ReLU of the input; K-steps of weights in flight
__global__ __launch_bounds__(256, 2) void conv_pw_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = 128, NT = 256;
    constexpr int PBUF = PRP * 8 * 128;                    // patch buffer: PRP pieces of 8 rows x 128 B
    constexpr int PPL = PRP / 4;                            // LDS-DMA pieces per wave and patch slice
    constexpr int NPB = 3;                                  // patch buffers: the slice being read, the next (transformed meanwhile) and the one after (in flight)
    constexpr int ZROW = NPB * PBUF, TAB = ZROW + 128;
    constexpr int CROW = BN * 2 + 16;
    static_assert(BM * CROW <= NPB * PBUF, "the epilogue's bf16 tile lives in the patch buffers");
    static_assert(PD == 3, "the nine-tap body keeps the weight registers of K-step g in slot g % PD");
    __shared__ __attribute__((aligned(16))) char smem[TAB + (AFF ? 4096 : 0)];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int tile = xcd_tile();
    const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int W = p.Win;
    const int NCB = p.Cin >> 6;                               // 64-channel blocks
    const int G = NCB * 9;                                    // K-steps
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    if (tid < 8) *(u32x4*)(smem + ZROW + tid * 16) = u32x4{0u, 0u, 0u, 0u};

    // ---- the patch slice of a channel block: PRP pieces of 8 rows, PPL per wave.  Piece j of this wave covers patch rows
    //      (wave PPL + j) 8 + (lane >> 3); its swizzle term (row >> 1) & 7 only depends on the parity of wave PPL + j, so two base
    //      pointers (even / odd piece) + a validity bit per piece describe all of them ----
    const int PR = BM + 2 * W + 2;                            // patch rows in use: flat pixels m0 - (W+1) .. m0 + BM + W
    const bf16_t* p_base[2];
    unsigned p_ok = 0u;
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int prow = (wave * PPL + j) * 8 + (lane >> 3);
        const long flat = (long)m0 - (W + 1) + prow;
        if (prow < PR && flat >= 0 && flat < p.M) p_ok |= 1u << j;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int prow = (wave * PPL + e) * 8 + (lane >> 3);       // piece e; pieces e + 2, e + 4 sit 16, 32 rows further on
        const int ch = swz_chunk(lane & 7, prow);
        p_base[e] = p.A + (((long)m0 - (W + 1) + prow) * p.sW + ch * 8);
    }
    const long p_pitch = 8 * p.sW;                            // elements between consecutive pieces
    int p_cb = 0;                                              // channel offset of the next slice

    // The LDS-DMA is issued from inline asm, out of the compiler's sight: global_load_lds is FLAT-encoded, and LLVM's waitcnt
    // insertion treats a pending FLAT operation that touches both LDS and memory as "may complete out of order" -- every wait on a
    // weight register or an A fragment while a slice is in flight becomes vmcnt(0) lgkmcnt(0), which drains the weight prefetch once
    // per channel block.  Unseen, the pieces only make the compiler's counted waits for the weight registers stricter than needed
    // (more operations are in the in-order queue than it knows of), never laxer.  No branch around the pieces of a slice that does
    // not exist either (a conditional VMEM issue has the same effect at the join): past the last channel block they fetch the zero
    // word into the buffer nobody reads any more.  (m0 is reserved: the compiler loads it right before each use of its own -- there
    // is none in this kernel -- and never expects it to survive.)
    auto issue_patch = [&](int buf, bool real) {
        const unsigned dst = (unsigned)(size_t)(lptr_t)(smem + buf * PBUF + wave * PPL * 8 * 128);
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const bf16_t* src = (real && ((p_ok >> j) & 1u)) ? p_base[j & 1] + ((j >> 1) * 2 * p_pitch + p_cb) : zero;
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(dst + j * 8 * 128) : "memory");
        }
        p_cb += 64;
    };

    // ---- this wave's weight stream: G K-steps of 4 KB, fragment ordered (a K-step past the end re-reads the last one) ----
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>((const char*)p.Bp + (long)((n0 >> 5) + wave) * G * 4096), 0, G * 4096, 0x00020000);
    const int wlane = lane * 16;
    auto load_b = [&](int g, int ks) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wsrc, wlane, (g < G ? g : G - 1) * 4096 + ks * 1024, 0));
    };

    // ---- prologue: slices 0 and 1 and the first PD K-steps of weights are requested FIRST; the tap masks (integer divisions) and
    //      the BatchNorm table are worked out while they fly ----
    issue_patch(0, true);
    issue_patch(1, NCB > 1);
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 bq[PD][4];
#pragma unroll
    for (int s = 0; s < PD; ++s)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) bq[s][ks] = load_b(s, ks);
    __builtin_amdgcn_sched_barrier(0);

    // ---- tap validity per row block (bit t = tap t inside the image) ----
    unsigned a_mask[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int grow = m0 + i * 32 + r;
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

    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;

    // AFF: bn1 + ReLU of the operand (torchvision Bottleneck's relu(bn1(conv1(x))) feeding conv2), applied to each 64-channel slice
    // of the patch ONCE, in LDS, by all four waves; padded taps read the zero row, so zero padding stays zero
    float* in_tab = (float*)(smem + TAB);
    if constexpr (AFF) conv_in_table<NT>(p, in_tab);
    // thread tid owns the 16-byte channel group lc = tid & 7 of rows (tid >> 3) + 32 j: (row >> 1) & 7 is the same for all of
    // them, so every address is one base plus an immediate
    auto xform_patch = [&](int buf, int cb) {
        const int lc = tid & 7, r0 = tid >> 3;
        const float* ts = in_tab + cb * 64 + lc * 8;
        const InTab tab = in_tab_fetch(ts, p.Cin);
        char* at0 = smem + buf * PBUF + r0 * 128 + (swz_chunk(lc, r0) << 4);
        // (three pieces at a time: the transform runs in the middle of the K loop, where registers are scarce)
#pragma unroll
        for (int j0 = 0; j0 < PRP / 4; j0 += 3) {
            u32x4 w[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j0 + j < PRP / 4) w[j] = *(const u32x4*)(at0 + (j0 + j) * 4096);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j0 + j >= PRP / 4) continue;
                w[j] = bn_relu_chunk(w[j], tab);
                *(u32x4*)(at0 + (j0 + j) * 4096) = w[j];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };

    wait_vmcnt<PD * 4 + PPL>();                                // this wave's pieces of slice 0 (older than slice 1 and the weight loads)
    __syncthreads();                                           // ... everybody's, the zero row, the table
    if constexpr (AFF) {
        xform_patch(0, 0);
        __syncthreads();
    }

    // A fragment addresses of (patch buffer, tap): the row of lane (r, h) in row block i is patch row i*32 + r + kh W + kw; the four
    // row blocks are 4096 B apart and share the swizzle ((row >> 1) & 7 does not see a multiple of 32); padded taps read the zero row
    struct Tap { int off[4]; int sw; };
    auto tap_addr = [&](int buf, int t) {
        Tap a;
        const int prow = r + (t / 3) * W + (t % 3);
        a.sw = swz_of(prow);
        const int base = buf * PBUF + prow * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // (opaque to the optimiser: left alone it hoists all 36 (row block, tap) tests out of the K loop, and their lane masks
            // overflow the scalar registers into vector ones -- the kernel then spills)
            unsigned m = a_mask[i];
            asm volatile("" : "+v"(m));
            a.off[i] = ((m >> t) & 1u) ? base + i * 4096 : ZROW;
        }
        return a;
    };
    auto load_a = [&](const Tap& a, int ks, bf16x8 (&f)[4]) {
        const int c = ((2 * ks + h) ^ a.sw) << 4;              // (the zero row is 128 B of zeros: any chunk of it will do)
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = *(const bf16x8*)(smem + a.off[i] + c);
    };

    // A fragments are read one substep (4 MFMAs) ahead of their use (two ahead costs 16 registers and measured no faster: with two
    // workgroups per CU the other wave of the SIMD covers the read)
    Tap cur = tap_addr(0, 0);
    bf16x8 f0[4], f1[4];
    load_a(cur, 0, f0);
    int g = 0, b0 = 0, b1 = 1, b2 = 2;
    // one channel block; LAST (compile time): no further slice to fetch / transform, no fragments of a next block, and no weight
    // loads past the end of the stream -- nothing useless is in flight when the K loop ends (a dummy load issued in the last tap
    // would have to be waited for, a microsecond, before its registers may be reused)
    auto block = [&](int cb, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if constexpr (!LAST) {
                if (t == 5) {
                    // slice cb + 1 is older than the weight loads of nine taps: any count below that many proves it landed
                    wait_vmcnt<24>();
                    raw_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    issue_patch(b2, cb + 2 < NCB);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (AFF) xform_patch(b1, cb + 1);
                }
            }
            const Tap nxt = tap_addr((!LAST && t == 8) ? b1 : b0, t == 8 ? 0 : t + 1);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if constexpr (AFF && !LAST) {
                    if (t == 8 && ks == 3) {
                        // the first fragments of the next channel block come from the other buffer: everybody's transform is done
                        raw_barrier();
                    }
                }
                if (ks < 3) load_a(cur, ks + 1, f1);
                else if (!(LAST && t == 8)) load_a(nxt, 0, f1);
                __builtin_amdgcn_sched_barrier(0);
                const bf16x8 b = bq[t % PD][ks];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0[i], b, acc[i], 0, 0, 0);
                if (!(LAST && t + PD >= 9)) bq[t % PD][ks] = load_b(g + PD, ks);      // the same registers, PD K-steps on
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) f0[i] = f1[i];
            }
            cur = nxt;
            ++g;
        }
        const int bt = b0;
        b0 = b1; b1 = b2; b2 = bt;
    };
    for (int cb = 0; cb + 1 < NCB; ++cb) block(cb, std::false_type{});
    block(NCB - 1, std::true_type{});
    // (nothing but a zero-source slice of the second to last block can still be in flight;) every wave is done with its patch reads
    // before the buffers are reused
    wait_vmcnt<0>();
    __syncthreads();

    // ---- epilogue: BatchNorm column sums (a lane holds 64 of a column's 128 rows), bf16 tile through LDS ----
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
        float osc = 1.0f, osh = 0.0f;
        if (p.out_scale && n0 + colw < p.N) { osc = p.out_scale[n0 + colw]; osh = p.out_shift[n0 + colw]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = acc_row(i, e, h);
                float v = acc[i][e];
                if (p.out_scale) v = v * osc + osh;
                if (p.out_relu) v = fmaxf(v, 0.0f);
                *(bf16_t*)(smem + row * CROW + colw * 2) = (bf16_t)v;
            }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < BM * 16 / NT; ++it) {
        const int qid = tid + it * NT;
        const int row = qid >> 4, cc = qid & 15;
        const int grow = m0 + row, gcol = n0 + cc * 8;
        if (grow < p.M && gcol < p.N) store16_wt(p.C + (long)grow * p.ldc + gcol, *(const u32x4*)(smem + row * CROW + cc * 16));
    }
}

// dense NHWC 3x3 / stride 1 / pad 1, Cin a multiple of 64, Cout of 128, a patch of 128 + 2W + 2 rows within the 192-row buffer, and
// the fragment-ordered copy of the weights (sat_conv_pack_weights)
bool pw_ok(const ConvArgs& a) {
    return a.Bp != nullptr && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.padw == 1 && a.Hout == a.Hin && a.Wout == a.Win &&
           (a.Cin % 64) == 0 && a.K == 9 * a.Cin && a.sW == a.Cin && a.sH == (long)a.Win * a.sW &&
           a.sN == (long)a.Hin * a.sH && 128 + 2 * a.Win + 2 <= 192 && (a.N % 128) == 0 && (!a.in_affine || a.Cin <= 512) &&
           !a.residual;
}

int launch_pw(ConvArgs& a, int groups, hipStream_t s) {
    if (!pw_ok(a)) return SAT_ERR_UNSUPPORTED;
    a.tiles_n = a.N / 128;
    const bool small = 128 + 2 * a.Win + 2 <= 160;
    const ConvKernel k = small ? (a.in_affine ? conv_pw_kernel<20, true, 3> : conv_pw_kernel<20, false, 3>)
                               : (a.in_affine ? conv_pw_kernel<24, true, 3> : conv_pw_kernel<24, false, 3>);
    return launch_conv(k, dim3(sat_cdiv(a.M, 128) * a.tiles_n, groups), dim3(256), 0, s, a);
}

// weights [Cout][KH*KW][Cin] (the kernels' OHWI layout) -> the fragment order conv_pw_kernel streams:
// [Cout / 32][Cin / 64 (cb)][KH*KW (tap)][4 (ks)][64 lanes: h * 32 + r][8]  <-  w[32 nb + r][tap][64 cb + 16 ks + 8 h + e]
__global__ void pack_weights_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ out, int Cout, int Cin, int taps) {
    const long n16 = (long)Cout * taps * Cin / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        long q = i >> 6;
        const int ks = (int)(q & 3); q >>= 2;
        const int tap = (int)(q % taps); q /= taps;
        const int ncb = Cin >> 6;
        const int cb = (int)(q % ncb);
        const int nb = (int)(q / ncb);
        const int r = lane & 31, h = lane >> 5;
        const long src = ((long)(nb * 32 + r) * taps + tap) * Cin + cb * 64 + ks * 16 + h * 8;
        *(u32x4*)(out + i * 8) = *(const u32x4*)(w + src);
    }
}
