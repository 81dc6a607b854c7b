// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the variant table and the pieces of sat_conv_tile.h).
//
// "Expansion" 1x1 convolution (conv3 of a bottleneck, `self.resnet(images)`, models.py:27: K = planes = 256 input channels, N = 4 K
// output channels) with the WEIGHTS RESIDENT IN REGISTERS and the workgroup PERSISTENT over row tiles.
//
// Why (round 5): as a GEMM this conv is four K-steps long.  conv_xp_kernel keeps the activation panel in registers and streams the
// weights, but every one of its 784 workgroups (two batches, layer 3) pays a prologue -- panel load round trip, table build, the
// operand's BatchNorm pass in LDS, 32 fragment reads behind barriers -- and an epilogue per column tile as long as its K loop: 30.9 us
// per launch for 6 us of matrix work, at 19 GB/s of L2 -> CU intake per CU (a third of what the path gives): it is bound by its own
// serial structure, not by bytes.  Here the roles are swapped:
//   * a workgroup owns ONE 128-column block of the weights for good: wave w holds its 32 columns x K = 256 as sixteen MFMA B fragments
//     (64 VGPRs), loaded once from the fragment-ordered copy (sat_conv_pack_weights) -- no weight traffic after the prologue;
//   * it walks the row tiles worker, worker + W, ... of its column block: the activations stream global -> registers -> LDS as one
//     CONTINUOUS sequence of 16 KB stages (four stages in flight in registers, two LDS buffers, one barrier per K-step, the operand's
//     BatchNorm + ReLU applied on the way: conv_aw_kernel's path) -- a tile boundary is just another K-step, its loads were requested
//     four K-steps earlier, under the previous tile's MFMAs and epilogue;
//   * the epilogue of a tile (bf16 tile through LDS, full-row write-through stores) runs while the other workgroup of the CU computes;
//     the BatchNorm column sums are kept in registers ACROSS the workgroup's tiles and leave once (integer atomics), or per tile (slabs);
//   * 68 KB of LDS, <= 256 registers: two workgroups per CU.
// Output tensor bit-identical to the ring kernel / conv_aw_kernel / conv_xp_kernel (same MFMA, same K order).  The column sums are this
// kernel's own (a lane sums its 64 rows of a tile, tiles of a worker in order, then the two lane halves): statistics signature 6000.
// Work split: W workers per column block, a function of (M, N) only -- never of the group count -- so a batch's sums are added in the
// same order in the grouped and the ungrouped program.
template <bool AFF>
__global__ __launch_bounds__(256, 2) void conv_ap_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = 128, NT = 256, NKS = 4;
    constexpr int ABUF = BM * 128;                          // one K-step of A: 128 rows x 64 channels
    constexpr int CROW = BN * 2 + 16;
    constexpr int CTILE = BM * CROW;
    constexpr int NJ = 4, RJ = 32;                          // 16-byte chunks of an A stage per thread, rows RJ apart
    __shared__ __attribute__((aligned(16))) char smem[2 * ABUF + CTILE + (AFF ? 2048 : 0)];
    char* ctile = smem + 2 * ABUF;
    float* in_tab = (float*)(smem + 2 * ABUF + CTILE);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    const int tile = xcd_tile();
    const int W = gridDim.x / p.tiles_n;                          // workers per column block
    const int worker = tile / p.tiles_n, tile_n = tile - worker * p.tiles_n;      // the column blocks of a row tile share an XCD's L2
    const int n0 = tile_n * BN;
    const int RT = (p.M + BM - 1) / BM;
    const int n_my = worker < RT ? (RT - worker + W - 1) / W : 0;               // row tiles worker, worker + W, ...
    if (n_my == 0) return;                                  // (uniform per workgroup)
    const int S = n_my * NKS;                               // stages of this workgroup's activation stream

    // ---- this thread's share of an A stage: 16-byte chunk slot lc of rows r0 + 32 j (the ring kernel's XOR-swizzled image) ----
    const int lc = tid & 7, r0 = tid >> 3;
    const int sw0 = (r0 >> 1) & 7;
    const __amdgpu_buffer_rsrc_t asrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.A), 0, (int)(p.in_bytes), 0x00020000);
    const int a_voff = (r0 * p.Cin + ((lc ^ sw0) << 3)) * 2;      // rows r0 + 32 j: + j * 32 rows, a SCALAR offset (registers are scarce here)
    const int a_jstep = RJ * p.Cin * 2;
    // stage g = (tile g >> 2 of this worker, K-step g & 3); rows past M lie past the buffer and read zeros; stages past the end
    // re-read the last one (never used)
    auto load_a_stage = [&](int g, u32x4 (&dst)[NJ]) {
        const int gg = g < S ? g : S - 1;
        const int m0 = (worker + (gg >> 2) * W) * BM;
        const int so = (m0 * p.Cin + (gg & 3) * 64) * 2;
#pragma unroll
        for (int j = 0; j < NJ; ++j) dst[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(asrc, a_voff, so + j * a_jstep, 0));
    };
    auto rows_ok = [&](int tile_seq) {                      // bit j: row r0 + 32 j of that tile exists
        const int m0 = (worker + tile_seq * W) * BM;
        unsigned ok = 0u;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (m0 + r0 + RJ * j < p.M) ok |= 1u << j;
        return ok;
    };

    // ---- prologue: the first four stages, then this wave's weights: 32 columns x K, sixteen fragments, for good ----
    u32x4 ar[4][NJ];
    load_a_stage(0, ar[0]);
    load_a_stage(1, ar[1]);
    load_a_stage(2, ar[2]);
    load_a_stage(3, ar[3]);
    bf16x8 wreg[NKS][4];
    {
        const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>((const char*)p.Bp + (long)((n0 >> 5) + wave) * NKS * 4096), 0, NKS * 4096, 0x00020000);
#pragma unroll
        for (int kt = 0; kt < NKS; ++kt)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                wreg[kt][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wsrc, lane * 16, kt * 4096 + ks * 1024, 0));
    }
    f32x16 acc[4];
    const f32x16 kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    if constexpr (AFF) {
        conv_in_table<NT>(p, in_tab);
        lds_barrier();      // (not __syncthreads: that would also wait for every load in flight)
    }
    // a landed stage (K-step kt of some tile) on its way to LDS buffer `buf`: relu(x * scale + shift) per channel, bit for bit the
    // normalise+ReLU kernel (rows past M stay zero)
    auto store_a_stage = [&](int kt, int buf, u32x4 (&src)[NJ], unsigned ok) {
        char* at0 = smem + buf * ABUF + r0 * 128 + (lc << 4);
        if constexpr (AFF) {
            const float* ts = in_tab + kt * 64 + ((lc ^ sw0) << 3);
            const InTab tab = in_tab_fetch(ts, p.Cin);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                u32x4 w = src[j];
                w = bn_relu_chunk(w, tab, (ok >> j) & 1u);
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

    const __amdgpu_buffer_rsrc_t csrc = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, (int)((long)p.M * p.ldc * 2), 0x00020000);
    // this thread's eight 16-byte pieces of an output tile: piece `it` = row (tid >> 4) + 16 it, chunk tid & 15 -- one lane offset,
    // the row step as a scalar offset
    const int c_voff = ((tid >> 4) * (int)p.ldc + n0 + (tid & 15) * 8) * 2;
    const int c_istep = 16 * (int)p.ldc * 2;
    const int colw = wave * 32 + r;
    float s_run = 0.0f, q_run = 0.0f;                       // this lane's column sums over the tiles of this worker (atomic mode)
    unsigned ok_cur = rows_ok(0);
    store_a_stage(0, 0, ar[0], ok_cur);
    load_a_stage(4, ar[0]);

    for (int ts_ = 0; ts_ < n_my; ++ts_) {
        const unsigned ok_next = rows_ok(ts_ + 1);
        const int tile_m = worker + ts_ * W;
        const int m0 = tile_m * BM;
        // K-step kt of this tile = stage g = 4 ts_ + kt: in LDS buffer kt & 1; stage g + 1 leaves register set (kt + 1) & 3 for buffer
        // (kt + 1) & 1, whose last readers (stage g - 1) finished before this step's barrier; its set takes stage g + 5
        auto step = [&](auto kt_tag) {
            constexpr int KT = decltype(kt_tag)::value, K1 = (KT + 1) & 3;
            const int g = ts_ * NKS + KT;
            lds_barrier();      // this wave's LDS writes of stage g and everybody's; everybody is done with stage g - 1
            if (g + 1 < S) store_a_stage(K1, K1 & 1, ar[K1], KT == 3 ? ok_next : ok_cur);      // (uniform branch)
            load_a_stage(g + 5, ar[K1]);
            const char* st = smem + (KT & 1) * ABUF;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                bf16x8 fa[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = *(const bf16x8*)(st + a_off[ks] + i * 4096);
                // (the first MFMA of a tile starts from a literal zero C operand: no 64 v_mov per tile to clear the accumulators)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], wreg[KT][ks], (KT == 0 && ks == 0) ? kZero16 : acc[i], 0, 0, 0);
            }
        };
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{});

        // ---- epilogue of this tile: column sums (a lane holds 64 of a column's 128 rows), bf16 tile through LDS ----
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
            if (p.stat_partial) {
                const float s2 = s + __shfl_xor(s, 32, 64), q2 = q + __shfl_xor(q, 32, 64);
                if (h == 0) {
                    stat_slab_store(p.stat_partial, tile_m, p.N, s2, q2, n0, colw);
                }
            }
            s_run += s;                                       // tiles of this worker in order
            q_run += q;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = acc_row(i, e, h);
                *(bf16_t*)(ctile + row * CROW + colw * 2) = (bf16_t)acc[i][e];
            }
        lds_barrier();      // (the next tile's first K-step barrier keeps the tile region safe)
        // write-through (sc0 sc1) stores the compiler counts itself (a raw buffer store, not store16_wt's inline asm: uncounted stores
        // in the loop would make every counted wait on a younger activation stage wait for them too); rows past M fall outside the
        // buffer and are dropped
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int qid = tid + it * NT;
            const int row = qid >> 4, cc = qid & 15;
            const u32x4 v = *(const u32x4*)(ctile + row * CROW + cc * 16);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, v), csrc,
                                                   c_voff, m0 * (int)p.ldc * 2 + it * c_istep, 17);
        }
        ok_cur = ok_next;
    }
    if (p.acc) {
        const float s2 = s_run + __shfl_xor(s_run, 32, 64), q2 = q_run + __shfl_xor(q_run, 32, 64);
        if (h == 0) {
            stat_acc_add(p.acc, p.N, s2, q2, n0, colw);
        }
    }
}

// dense 1x1 / stride 1 with K = 256, the fragment-ordered copy of the weights, N a multiple of 128, batch statistics (or none) in the
// epilogue; an input tensor a 32-bit byte offset can address
bool ap_ok(const ConvArgs& a) {
    return a.Bp != nullptr && a.linear && a.K == 256 && a.Cin == 256 && (a.N % 128) == 0 && !a.residual && !a.out_scale &&
           a.in_bytes > 0 && a.in_bytes < 0x7ffffff0L && a.ldc == a.N && (long)a.M * a.ldc * 2 < 0x7ffffff0L;
}

// workers per column block: a function of (M, N) only.  At most 256 / tiles_n (two groups then fill the chip's 512 slots), and as
// few as give every worker the same number of row tiles (98 row tiles: 25 workers x 4 tiles instead of 32 workers x 3.06)
int ap_workers(const ConvArgs& a) {
    const int tiles_n = a.N / 128, rt = sat_cdiv(a.M, 128);
    int wmax = 256 / tiles_n;
    if (wmax < 1) wmax = 1;
    const int tpw = sat_cdiv(rt, wmax);
    return sat_cdiv(rt, tpw);
}

int launch_ap(ConvArgs& a, int groups, hipStream_t s) {
    if (!ap_ok(a)) return SAT_ERR_UNSUPPORTED;
    a.tiles_n = a.N / 128;
    return launch_conv(a.in_affine ? conv_ap_kernel<true> : conv_ap_kernel<false>, dim3(ap_workers(a) * a.tiles_n, groups), dim3(256), 0, s, a);
}
