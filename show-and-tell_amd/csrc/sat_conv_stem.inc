// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the LDS-DMA helpers and the variant table).
//
// The STEM of the frozen stack (`self.resnet(images)`, models.py:27: torchvision's 7x7 / stride 2 conv1) as the op program lays
// it out: a zero-bordered NHWC4 image and a "7 x 1" kernel over 32-element rows of 8 pixels x 4 channels (K = 7 x 32 = 224, the
// eighth pixel and the fourth channel carry zero weights), 64 output channels.
//
// Why a kernel of its own: as a ring-kernel GEMM this conv is 6272 workgroups (batch 64) of 3.5 K-steps each -- every one
// re-loads the same 28 KB of weights, pays a prologue and an epilogue for 0.4 us of matrix work, and stages 56 KB of activations
// per 128-row tile of which three quarters are the neighbouring output pixels' bytes again (stride 2 under an 8-pixel window):
// 91-96 us, 0.06 of the bf16 peak.  Here
//   * a workgroup is PERSISTENT over its share of the 128-row tiles (two workgroups per CU);
//   * the weights live in REGISTERS for the whole launch: lane (c, h) of a 32x32x16 B fragment holds 16 contiguous bytes of
//     output channel c -- 2 column tiles x 14 K-steps = 112 VGPRs, loaded once;
//   * the activations of a tile come as INPUT ROW SEGMENTS: the 128 output rows of a tile belong to at most three (image, output
//     row) pairs, each needs 7 whole input rows of Win pixels (1856 B at 224 x 224) -- 13 KB per pair by LDS-DMA, contiguous, instead
//     of 56 KB of overlapping windows; the A fragment of output pixel wo, kernel row kh is the 64 bytes at pixel 2 wo of input row
//     kh: consecutive lanes read 16 bytes apart, conflict free, no swizzle;
//   * epilogue = the ring kernel's: per-tile BatchNorm column sums (fixed order) and a bf16 tile staged through LDS for 16-byte
//     write-through stores.
// Arithmetic is the ring kernel's on the same geometry (same MFMA, same K order): the output tensor is bit-identical.
constexpr int kStemSeg = 3;            // (image, output row) pairs a 128-row tile can touch when Wout >= 64

// NLOAD > 0: the patch buffer is DOUBLE BUFFERED -- every wave issues exactly NLOAD LDS-DMA instructions per tile (the pieces of
// the NEXT tile, zero-source dummies beyond them) before it waits for all but those, so a tile's load latency hides under the
// previous tile's matrix work and epilogue; NLOAD = 0: one buffer of kStemSeg segments (any geometry stem_ok admits).
template <int NLOAD>
__global__ __launch_bounds__(256, 2) void conv_stem_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BM = 128, BN = 64, NT = 256, KS = 14;              // K-steps of 16 elements: 7 kernel rows x 2 halves
    constexpr int CROW = BN * 2 + 16;                                  // bf16 C-tile row stride in LDS
    extern __shared__ __attribute__((aligned(16))) char smem[];      // patch buffer(s) | C tile | column-sum scratch
    const int rowb = p.Win * 8;                                        // bytes of one input row (Win pixels x 4 channels x bf16)
    const int segb = 7 * rowb;
    const int patchb = NLOAD ? NLOAD * NT * 16 : kStemSeg * segb;      // one patch buffer
    char* ctile = smem + (NLOAD ? 2 : 1) * patchb;
    float* red = (float*)(ctile + BM * CROW);                          // [4 waves][2][BN]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    // ---- weights -> registers, once ----
    bf16x8 bf[2][KS];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            bf[j][ks] = *(const bf16x8*)(p.B + (long)(j * 32 + r) * p.ldb + ks * 16 + h * 8);

    const int tiles = (p.M + BM - 1) / BM;
    const int rowchunks = rowb >> 4;                                   // 16-byte pieces per input row
    const int segchunks = 7 * rowchunks;
    // input row segments of a tile -> LDS (lane-linear LDS-DMA: piece i lands at byte 16 i of the buffer)
    auto issue_tile = [&](int tile, char* buf) {
        int total = 0, nh0 = 0;
        if (tile < tiles) {
            const int m0 = tile * BM;
            const int mlast = (m0 + BM <= p.M ? m0 + BM : p.M) - 1;
            nh0 = m0 / p.Wout;
            total = (mlast / p.Wout - nh0 + 1) * segchunks;
        }
        auto piece = [&](int it) {
            const int i = it * NT + tid;
            const bf16_t* src = zero;
            if (i < total) {
                const int seg = i / segchunks, rem = i - seg * segchunks;
                const int kh = rem / rowchunks, off = rem - kh * rowchunks;
                const int nh = nh0 + seg, n = nh / p.Hout, ho = nh - n * p.Hout;
                src = p.A + ((long)n * p.sN + (long)(ho * p.stride + kh) * p.sH + off * 8);
            }
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(buf + (it * NT + wave * 64) * 16), 16, 0, 0);
        };
        if constexpr (NLOAD > 0) {
#pragma unroll
            for (int it = 0; it < NLOAD; ++it) piece(it);              // exactly NLOAD instructions per wave, whatever the tile needs
        } else {
            for (int it = 0; it * NT < total; ++it) piece(it);
        }
    };

    int cur = 0;
    if constexpr (NLOAD > 0) issue_tile(blockIdx.x, smem);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * BM;
        const int mlast = (m0 + BM <= p.M ? m0 + BM : p.M) - 1;
        const int nh0 = m0 / p.Wout;                                   // first (image, output row) pair of the tile
        char* patch = smem + cur * patchb;
        if constexpr (NLOAD > 0) {
            issue_tile(tile + gridDim.x, smem + (cur ^ 1) * patchb);   // the next tile (dummies past the end: uniform counts)
            wait_vmcnt<NLOAD>();                                       // everything older than those: this tile's pieces
        } else {
            issue_tile(tile, patch);
            wait_vmcnt<0>();
        }
        // ---- this lane's A row: output pixel m0 + wave*32 + r -> (segment, wo); rows past M read row m0 (their results are dropped) ----
        int m = m0 + wave * 32 + r;
        if (m > mlast) m = m0;
        const int nh = m / p.Wout, wo = m - nh * p.Wout;
        const char* arow = patch + (nh - nh0) * segb + wo * (p.stride * p.sW * 2) + h * 16;
        __syncthreads();

        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 af = *(const bf16x8*)(arow + (ks >> 1) * rowb + (ks & 1) * 32);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[0][ks], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[1][ks], acc[1], 0, 0, 0);
        }
        // rows past M (last tile only): exact zeros, so that they add nothing to the statistics
        if (m0 + BM > p.M) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wave * 32 + acc_row(0, e, h);
                if (m0 + row >= p.M) { acc[0][e] = 0.0f; acc[1][e] = 0.0f; }
            }
        }
        // ---- epilogue: column sums of the f32 accumulators (this wave's 32 rows), bf16 tile through LDS ----
        if (p.stat_partial || p.acc) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float s = 0.0f, q = 0.0f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = acc[j][e];
                    s += v;
                    q += v * v;
                }
                lane_halves(s, q);
                if (h == 0) {
                    red[(wave * 2 + 0) * BN + j * 32 + r] = s;
                    red[(wave * 2 + 1) * BN + j * 32 + r] = q;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wave * 32 + acc_row(0, e, h);
                *(bf16_t*)(ctile + row * CROW + (j * 32 + r) * 2) = (bf16_t)acc[j][e];
            }
        __syncthreads();
        if ((p.stat_partial || p.acc) && tid < BN) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {                              // fixed order over the waves
                s += red[(g * 2 + 0) * BN + tid];
                q += red[(g * 2 + 1) * BN + tid];
            }
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, tile, p.N, s, q, tid);
            }
            if (p.acc) {                                               // few-tile programs: the integer accumulators directly
                stat_acc_add(p.acc, p.N, s, q, tid);
            }
        }
#pragma unroll
        for (int it = 0; it < BM * 8 / NT; ++it) {
            const int qid = tid + it * NT;
            const int row = qid >> 3, cc = qid & 7;
            if (m0 + row < p.M) store16_wt(p.C + (long)(m0 + row) * p.ldc + cc * 8, *(const u32x4*)(ctile + row * CROW + cc * 16));
        }
        __syncthreads();                                               // the patch and the C tile are rewritten by the next tile
        cur ^= (NLOAD ? 1 : 0);
    }
    if constexpr (NLOAD > 0) wait_vmcnt<0>();                          // the trailing dummies
}

// the op program's stem layout: 7 x 1 kernel over rows of 32 elements (8 pixels x 4 channels), pixel stride sW = 4 elements, 64
// output channels, no padding (the image carries its border), statistics as per-tile slabs or none
bool stem_ok(const ConvArgs& a) {
    return a.KH == 7 && a.KW == 1 && a.Cin == 32 && a.N == 64 && a.K == 224 && a.ldb == 224 && a.sW == 4 && a.pad == 0 && a.padw == 0 &&
           a.stride >= 1 && a.stride <= 2 && a.sH == (long)a.Win * 4 && a.sN == (long)a.Hin * a.sH && (a.Win % 2) == 0 && a.Wout >= 64 &&
           (long)(a.Wout - 1) * a.stride + 8 <= a.Win && (long)(a.Hout - 1) * a.stride + 7 <= a.Hin && !a.in_affine && !a.out_scale &&
           !a.residual && a.ldc == 64 && kStemSeg * 7 * a.Win * 8 + 128 * (64 * 2 + 16) + 4 * 2 * 64 * 4 <= 64 * 1024;
}

// (image, output row) pairs the widest tile touches: tile offsets inside an output row repeat with period Wout
static int stem_max_segments(const ConvArgs& a) {
    const int tiles = sat_cdiv(a.M, 128);
    int worst = 1;
    for (int t = 0; t < tiles && t < a.Wout; ++t) {
        const long m0 = (long)t * 128, ml = (m0 + 128 <= a.M ? m0 + 128 : a.M) - 1;
        const int n = (int)(ml / a.Wout - m0 / a.Wout) + 1;
        if (n > worst) worst = n;
    }
    return worst;
}

template <int NLOAD>
static int launch_stem_t(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    static bool raised = false;
    return launch_conv(conv_stem_kernel<NLOAD>, grid, dim3(256), lds, s, a, &raised, 96 * 1024);
}

int launch_stem(ConvArgs& a, int groups, hipStream_t s) {
    if (!stem_ok(a)) return SAT_ERR_UNSUPPORTED;
    const int tiles = sat_cdiv(a.M, 128);
    const int grid_x = tiles < 512 ? tiles : 512;                     // persistent: two workgroups per CU
    const dim3 grid(grid_x, groups);
    const int tail = 128 * (64 * 2 + 16) + 4 * 2 * 64 * 4;            // C tile + column-sum scratch
    const int nload = sat_cdiv((long)stem_max_segments(a) * 7 * (a.Win / 2), 256);
    const size_t lds2 = (size_t)2 * nload * 4096 + tail;             // double buffered: two workgroups of <= 78 KB per CU
    if (nload >= 4 && nload <= 8 && lds2 <= 78 * 1024) {
        switch (nload) {
            case 4: return launch_stem_t<4>(a, grid, lds2, s);
            case 5: return launch_stem_t<5>(a, grid, lds2, s);
            case 6: return launch_stem_t<6>(a, grid, lds2, s);
            case 7: return launch_stem_t<7>(a, grid, lds2, s);
            default: return launch_stem_t<8>(a, grid, lds2, s);
        }
    }
    return launch_stem_t<0>(a, grid, (size_t)kStemSeg * 7 * a.Win * 8 + tail, s);
}
