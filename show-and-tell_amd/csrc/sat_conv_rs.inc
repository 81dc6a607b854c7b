// Included by sat_conv_glds.hip inside its anonymous namespace (shares ConvArgs, the LDS-DMA helpers and the variant table).
//
// 3 x 3 / stride 1 convolutions over 32 input channels on LARGE maps -- Conv2d_2a_3x3 (32 -> 32, 149 x 149, no padding) and Conv2d_2b_3x3
// (32 -> 64, 147 x 147, padding 1) of the Inception-v3 stem (BASELINE configs[3]; `self.resnet(images)`, models.py:27, with the encoder
// variant of SURVEY 8f.3).  As ring-kernel GEMMs these are 10 805 workgroups per batch of 4.5 K-steps each (K = 288, N = 32 / 64): every
// one re-loads the weights, pays a prologue and an epilogue for half a microsecond of matrix work and gathers its 3 x 3 windows as 64-byte
// snippets -- 484 + 496 us per three-batch launch (158 / 308 TFLOP/s) for tensors that stream in ~120 us: a sixth of that program's conv
// time in two launches.  Here (conv_stem_kernel's idea, sat_conv_stem.inc, taken one step further):
//   * a workgroup is PERSISTENT over a contiguous run of OUTPUT ROWS (two workgroups of four waves per CU); wave w computes pixels
//     32 w .. 32 w + 31 of the row, wave 0 also the tail 128 .. Wout - 1 (128 <= Wout <= 160);
//   * the weights live in REGISTERS for the whole launch: 18 K-steps of 16 x N / 32 column tiles = 72 / 144 VGPRs, loaded once;
//   * the activations are a ROLLING WINDOW of whole input rows in LDS: output row ho needs input rows ho - pad .. ho - pad + 2, of which
//     two are already there from row ho - 1; the third was requested by LDS-DMA while row ho - 1 was being computed (a ring of four row
//     slots: three in use, one landing) -- every input byte enters LDS once per workgroup, and the load of a row hides under the previous
//     row's MFMAs and epilogue.  A kernel row's 3 pixels x 32 channels are 192 contiguous bytes of an input row, so the A fragment of
//     output pixel wo, kernel row kh, K-step s is the 16 bytes at LDS pixel wo + 1 - pad, byte 32 s + 16 h of that row's slot -- no
//     gather, no swizzle.  Every LDS row carries a zero pixel in front and behind (the horizontal padding); rows above / below the image
//     are slots filled from a zero chunk (the vertical padding);
//   * epilogue per output row: BatchNorm column sums (a wave's pixels, then the four waves in order) into slab `row` of stat_partial
//     (there are at least as many 128-pixel slabs as output rows: the rest are written as zeros) or the integer accumulators, and a bf16
//     row staged through LDS for 16-byte write-through stores.
// K order = the ring kernel's (kernel row, kernel column, channel: 16-element MFMA steps over the flattened K): the output tensor is
// bit-identical to it; the column sums are this kernel's own: statistics signature 7000.
template <int NJ>
__global__ __launch_bounds__(256, 2) void conv_rs_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BN = 32 * NJ, NT = 256, NWV = 4, KH = 3, RS = 6, KS = KH * RS;      // K-steps of 16 elements: 3 kernel rows x 6
    constexpr int ITS = (160 * (BN / 8) + NT - 1) / NT;                // 16-byte output chunks per thread and row (store instructions per wave): 3 / 5
    constexpr int CROW = BN * 2 + 16;                                  // bf16 C-row stride in LDS (per pixel)
    extern __shared__ __attribute__((aligned(16))) char smem[];      // four row slots | C row (160 pixels) | column-sum scratch
    const int rowp = p.Win * 4;                                        // 16-byte pieces of one input row (64 bytes per pixel)
    const int ppw = (rowp + 8 + 63) >> 6;                              // LDS row = [zero pixel][the row][>= one zero pixel], a whole number of
    const int pitchb = ppw * 1024;                                     // 1 KB wave-instructions: an LDS-DMA instruction never straddles two rows
    char* ctile = smem + 4 * pitchb;
    float* red = (float*)(ctile + 160 * CROW);                         // [4 waves][2][BN]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    // ---- weights -> registers, once: [Cout][3][3][32] = [Cout][288], K-step ks = 16 contiguous elements ----
    bf16x8 bf[NJ][KS];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            bf[j][ks] = *(const bf16x8*)(p.B + (long)(j * 32 + r) * p.ldb + ks * 16 + h * 8);

    // input row hi of image n -> its slot (hi & 3 of the ring; hi = -1 is slot 3): wave-instruction k of the row fills pieces 64 k .. 64 k + 63,
    // the waves share the ppw instructions of a row
    auto issue_row = [&](int n, int hi) {
        char* slot = smem + ((hi + 4) & 3) * pitchb;
        const bool inside = hi >= 0 && hi < p.Hin;
        const bf16_t* rowsrc = p.A + ((long)n * p.sN + (long)(inside ? hi : 0) * p.sH);
        for (int k = wave; k < ppw; k += NWV) {
            // LDS piece q = 64 k + lane = (LDS pixel q >> 2, chunk slot q & 3); LDS pixel 0 is the zero pixel, LDS pixel x + 1 is input pixel x.
            // A pixel's four 16-byte chunks sit XOR-swizzled by bits 2-3 of its LDS pixel index (chunk c in slot c ^ ((pixel >> 2) & 3)): the
            // fragment reads of 16 consecutive pixels, 64 bytes apart, then touch 16 different 16-byte bank groups (unswizzled: four)
            const int q = k * 64 + lane, pl = q >> 2;
            const int d = (pl - 1) * 4 + ((q & 3) ^ ((pl >> 2) & 3));
            const bf16_t* src = (inside && pl >= 1 && pl <= p.Win) ? rowsrc + d * 8 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(slot + k * 1024), 16, 0, 0);
        }
    };

    const int rows = p.M / p.Wout;                                     // output rows of the launch (all images): M = images x Hout x Wout
    const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t0 = blockIdx.x * per, t1 = t0 + per < rows ? t0 + per : rows;
    const int ntask = (p.Wout + 31) >> 5;                              // 32-pixel tasks of a row: wave w takes w, w + 4

    bool fresh = true;                                                 // the window has to be loaded whole (first row of the run / of an image)
    for (int t = t0; t < t1; ++t) {
        const int n = t / p.Hout, ho = t - n * p.Hout;
        const int hi0 = ho - p.pad;
        if (fresh) {
            issue_row(n, hi0);
            issue_row(n, hi0 + 1);
            issue_row(n, hi0 + 2);
            wait_vmcnt<0>();
        } else {
            wait_vmcnt<ITS>();                                         // all but row t - 1's output stores: the prefetched input row has landed
        }
        __syncthreads();                                               // everybody's pieces; and everybody is done with row t - 1 (its slots, the C row)
        fresh = ho + 1 == p.Hout;                                      // the next output row starts a new image
        if (!fresh && t + 1 < t1) issue_row(n, hi0 + 3);               // the next row's new input row lands under this row's work: its slot held row hi0 - 1

        float ssum[NJ], qsum[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) { ssum[j] = 0.0f; qsum[j] = 0.0f; }
        for (int task = wave; task < ntask; task += NWV) {
            // this lane's pixel; lanes past the row's end compute pixel 0 again (their results are zeroed)
            const int px0 = task * 32 + r;
            const int pl0 = (px0 < p.Wout ? px0 : 0) + 1 - p.pad;      // LDS pixel of the window's first column
            int aoffs[RS];                                             // K-step s of a kernel row: LDS pixel pl0 + (s >> 1), chunk 2 (s & 1) + h, swizzled
#pragma unroll
            for (int s = 0; s < RS; ++s) {
                const int pl = pl0 + (s >> 1);
                aoffs[s] = pl * 64 + (((2 * (s & 1) + h) ^ ((pl >> 2) & 3)) << 4);
            }
            f32x16 acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
#pragma unroll
            for (int kh = 0; kh < KH; ++kh) {
                const char* arow = smem + ((hi0 + kh + 4) & 3) * pitchb;
#pragma unroll
                for (int s = 0; s < RS; ++s) {
                    const bf16x8 af = *(const bf16x8*)(arow + aoffs[s]);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[j][kh * RS + s], acc[j], 0, 0, 0);
                }
            }
            // pixels past the row's end: exact zeros, so that they add nothing to the statistics (C/D map: row = (e&3) + 8*(e>>2) + 4*h)
            if (task * 32 + 31 >= p.Wout) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int px = task * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (px >= p.Wout) {
#pragma unroll
                        for (int j = 0; j < NJ; ++j) acc[j][e] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                // (inference: BatchNorm as a fixed affine of the column, then ReLU -- the ring kernel's epilogue arithmetic)
                const float osc = p.out_scale ? p.out_scale[j * 32 + r] : 1.0f, osh = p.out_scale ? p.out_shift[j * 32 + r] : 0.0f;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float v = acc[j][e];
                    ssum[j] += v;
                    qsum[j] += v * v;
                    if (p.out_scale) v = v * osc + osh;
                    if (p.out_relu) v = fmaxf(v, 0.0f);
                    const int px = task * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    *(bf16_t*)(ctile + px * CROW + (j * 32 + r) * 2) = (bf16_t)v;
                }
            }
        }
        // ---- epilogue: column sums (this wave's pixels: a lane's 16 per task, the tasks in order, then the two lane halves) ----
        if (p.stat_partial || p.acc) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float s = ssum[j] + __shfl_xor(ssum[j], 32, 64), q = qsum[j] + __shfl_xor(qsum[j], 32, 64);
                if (h == 0) {
                    red[(wave * 2 + 0) * BN + j * 32 + r] = s;
                    red[(wave * 2 + 1) * BN + j * 32 + r] = q;
                }
            }
        }
        __syncthreads();
        if ((p.stat_partial || p.acc) && tid < BN) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int g = 0; g < NWV; ++g) {                            // fixed order over the waves
                s += red[(g * 2 + 0) * BN + tid];
                q += red[(g * 2 + 1) * BN + tid];
            }
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, t, p.N, s, q, tid);
            }
            if (p.acc) {                                               // few-tile programs: the integer accumulators directly
                stat_acc_add(p.acc, p.N, s, q, tid);
            }
        }
        {
            // exactly ITS store instructions per wave and row (the wait above counts them); chunks past the row's end go to the same
            // address as the row's last chunk with the same bytes -- no lane is switched off, no address is out of bounds
            bf16_t* crow = p.C + (long)t * p.Wout * p.ldc;
            const int nq = p.Wout * (BN / 8);                          // 16-byte chunks of the output row
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                int qid = tid + it * NT;
                if (qid >= nq) qid = nq - 1;
                const int px = qid / (BN / 8), cc = qid % (BN / 8);
                store16_wt(crow + (long)px * p.ldc + cc * 8, *(const u32x4*)(ctile + px * CROW + cc * 16));
            }
        }
    }
    // the statistics slabs beyond the output rows (the consumer sums all sat_cdiv(M, 128) of them): zeros, by the last workgroups' spare lanes
    if (p.stat_partial) {
        const int slabs = (p.M + 127) / 128;
        for (long i = (long)rows * 2 * p.N + (long)blockIdx.x * NT + tid; i < (long)slabs * 2 * p.N; i += (long)gridDim.x * NT) p.stat_partial[i] = 0.0f;
    }
}

static size_t rs_lds_bytes(const ConvArgs& a) {
    return (size_t)4 * ((a.Win * 4 + 8 + 63) / 64) * 1024 + 160 * ((size_t)a.N * 2 + 16) + 4 * 2 * (size_t)a.N * 4;
}

// 3 x 3 / stride 1 / padding 0 or 1 (both axes) over 32 channels of a dense NHWC tensor, 32 or 64 output channels, output rows of 128 to
// 160 pixels (at most five 32-pixel tasks per row), statistics as per-tile slabs (at least as many 128-pixel slabs as output rows), integer sums or none,
// two workgroups per CU
bool rs_ok(const ConvArgs& a) {
    return a.KH == 3 && a.KW == 3 && a.Cin == 32 && (a.N == 32 || a.N == 64) && a.K == 288 && a.ldb == 288 && a.stride == 1 &&
           (a.pad == 0 || a.pad == 1) && a.padw == a.pad && a.sW == 32 && a.sH == (long)a.Win * 32 && a.sN == (long)a.Hin * a.sH &&
           a.Wout >= 128 && a.Wout <= 160 && a.Wout == a.Win + 2 * a.pad - 2 && a.Hout == a.Hin + 2 * a.pad - 2 && a.Hout >= 1 &&
           (long)a.M == (long)(a.M / a.Wout) * a.Wout && !a.in_affine && !a.residual && a.ldc == a.N &&
           rs_lds_bytes(a) <= 80 * 1024;
}

template <int NJ>
static int launch_rs_t(const ConvArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    static bool raised = false;
    return launch_conv(conv_rs_kernel<NJ>, grid, dim3(256), lds, s, a, &raised, 80 * 1024);
}

int launch_rs(ConvArgs& a, int groups, hipStream_t s) {
    if (!rs_ok(a)) return SAT_ERR_UNSUPPORTED;
    const int rows = a.M / a.Wout;
    const dim3 grid(rows < 512 ? rows : 512, groups);                // persistent over runs of output rows: two workgroups per CU
    return a.N == 64 ? launch_rs_t<2>(a, grid, rs_lds_bytes(a), s) : launch_rs_t<1>(a, grid, rs_lds_bytes(a), s);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same rolling window for conv2 of ResNet's layer 1 (`self.resnet(images)`, models.py:27: 3 x 3 / stride 1 / padding 1, 64 -> 64
// channels on 56 x 56 maps; three launches per pass at 62 us each for two batches, 1.6 TB/s of tensors that stream in ~25 us -- as
// ring-kernel GEMMs of 3136 workgroups with nine K-steps each).  Differences to conv_rs_kernel: a step computes TWO output rows (112
// pixels: four 32-pixel tasks), the four waves are 2 (pixel tasks p, p + 2) x 2 (column halves of 32), so a wave keeps the weights of
// its 32 columns x K = 576 in registers (144 VGPRs); the window is a ring of six row slots (four in use, two landing); and the
// BatchNorm column sums stay in registers over ALL the steps of a workgroup and leave once, into slab `blockIdx.x` (the run of steps a
// workgroup gets is a function of the geometry alone: grid = min(steps, 256)) -- statistics signature 7001.  Output bit-identical to the
// ring kernel (same K order).
__global__ __launch_bounds__(256, 2) void conv_rs64_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BN = 64, NT = 256, KH = 3, RS = 12, KS = KH * RS, NSLOT = 6;      // K-steps of 16 elements: 3 kernel rows x 12
    constexpr int ITS = 4;                                             // 16-byte output chunks per thread and step (128 pixels x 8 / 256)
    constexpr int CROW = BN * 2 + 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // six row slots | C rows (128 pixels) | column-sum scratch
    const int rowp = p.Win * 8;                                        // 16-byte pieces of one input row (128 bytes per pixel)
    const int ppw = (rowp + 16 + 63) >> 6;                             // LDS row = [zero pixel][the row][>= one zero pixel] in whole 1 KB instructions
    const int pitchb = ppw * 1024;
    char* ctile = smem + NSLOT * pitchb;
    float* red = (float*)(ctile + 128 * CROW);                         // [4 waves][2][32]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ph = wave & 1, ch = wave >> 1;                           // pixel-task parity, column half
    const int r = lane & 31, h = lane >> 5;
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    bf16x8 bf[KS];                                                     // this wave's 32 columns x 576, once
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) bf[ks] = *(const bf16x8*)(p.B + (long)(ch * 32 + r) * p.ldb + ks * 16 + h * 8);

    auto issue_row = [&](int n, int hi) {
        char* slot = smem + ((hi + NSLOT) % NSLOT) * pitchb;
        const bool inside = hi >= 0 && hi < p.Hin;
        const bf16_t* rowsrc = p.A + ((long)n * p.sN + (long)(inside ? hi : 0) * p.sH);
        for (int k = wave; k < ppw; k += 4) {
            // LDS piece q = (LDS pixel q >> 3, chunk slot q & 7); a pixel's eight chunks sit XOR-swizzled by the low bits of its LDS pixel index
            // (chunk c in slot c ^ (pixel & 7)): fragment reads of consecutive pixels, 128 bytes apart, spread over all bank groups (unswizzled: two)
            const int q = k * 64 + lane, pl = q >> 3;
            const int d = (pl - 1) * 8 + ((q & 7) ^ (pl & 7));
            const bf16_t* src = (inside && pl >= 1 && pl <= p.Win) ? rowsrc + d * 8 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(slot + k * 1024), 16, 0, 0);
        }
    };

    const int spi = p.Hout >> 1;                                       // steps per image
    const int steps = (p.M / (p.Hout * p.Wout)) * spi;
    const int per = (steps + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t0 = blockIdx.x * per, t1 = t0 + per < steps ? t0 + per : steps;
    const int pps = 2 * p.Wout;                                        // pixels of a step
    float ssum = 0.0f, qsum = 0.0f;                                    // column ch*32 + r over this wave's pixels of all its steps

    bool fresh = true;
    for (int t = t0; t < t1; ++t) {
        const int n = t / spi, st = t - n * spi;
        const int hi0 = 2 * st - 1;                                    // first input row of the step's window (four rows)
        if (fresh) {
            issue_row(n, hi0);
            issue_row(n, hi0 + 1);
            issue_row(n, hi0 + 2);
            issue_row(n, hi0 + 3);
            wait_vmcnt<0>();
        } else {
            wait_vmcnt<ITS>();                                         // all but step t - 1's output stores: the two prefetched rows have landed
        }
        __syncthreads();
        fresh = st + 1 == spi;                                         // the next step starts a new image
        if (!fresh && t + 1 < t1) {
            issue_row(n, hi0 + 4);
            issue_row(n, hi0 + 5);
        }
        const int base = (hi0 + NSLOT) % NSLOT;
        for (int task = ph; task * 32 < pps; task += 2) {
            int px = task * 32 + r;
            if (px >= pps) px = 0;                                     // lanes past the step's end compute pixel 0 again (zeroed below)
            const int orow = px >= p.Wout ? 1 : 0, col = px - orow * p.Wout;
            int aoffs[RS];                                             // K-step s of a kernel row: LDS pixel col + (s >> 2), chunk 2 (s & 3) + h, swizzled
#pragma unroll
            for (int s = 0; s < RS; ++s) {
                const int pl = col + (s >> 2);                         // (LDS pixel col + 1 - pad = col: the window starts one pixel left)
                aoffs[s] = pl * 128 + (((2 * (s & 3) + h) ^ (pl & 7)) << 4);
            }
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
            for (int kh = 0; kh < KH; ++kh) {
                int sl = base + orow + kh;
                if (sl >= NSLOT) sl -= NSLOT;
                const char* arow = smem + sl * pitchb;
#pragma unroll
                for (int s = 0; s < RS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(arow + aoffs[s]), bf[kh * RS + s], acc, 0, 0, 0);
            }
            const float osc = p.out_scale ? p.out_scale[ch * 32 + r] : 1.0f, osh = p.out_scale ? p.out_shift[ch * 32 + r] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int q = task * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float v = q < pps ? acc[e] : 0.0f;
                ssum += v;
                qsum += v * v;
                if (p.out_scale) v = v * osc + osh;                    // (inference epilogue: the ring kernel's arithmetic)
                if (p.out_relu) v = fmaxf(v, 0.0f);
                *(bf16_t*)(ctile + q * CROW + (ch * 32 + r) * 2) = (bf16_t)v;
            }
        }
        __syncthreads();
        {
            bf16_t* crow = p.C + (long)t * pps * p.ldc;                // the step's two output rows are contiguous
            const int nq = pps * (BN / 8);
#pragma unroll
            for (int it = 0; it < ITS; ++it) {                         // exactly ITS store instructions per wave and step (the wait above counts them)
                int qid = tid + it * NT;
                if (qid >= nq) qid = nq - 1;
                const int px = qid >> 3, cc = qid & 7;
                store16_wt(crow + (long)px * p.ldc + cc * 8, *(const u32x4*)(ctile + px * CROW + cc * 16));
            }
        }
    }
    // ---- the workgroup's column sums: lane halves, then the two pixel-task waves of a column half in order ----
    if (p.stat_partial || p.acc) {
        const float s = ssum + __shfl_xor(ssum, 32, 64), q = qsum + __shfl_xor(qsum, 32, 64);
        __syncthreads();
        if (h == 0) {
            red[(wave * 2 + 0) * 32 + r] = s;
            red[(wave * 2 + 1) * 32 + r] = q;
        }
        __syncthreads();
        if (tid < BN) {
            const int c2 = tid >> 5, rr = tid & 31;                    // column half, column in it: waves (0, c2) then (1, c2)
            const float cs = red[((2 * c2) * 2 + 0) * 32 + rr] + red[((2 * c2 + 1) * 2 + 0) * 32 + rr];
            const float cq = red[((2 * c2) * 2 + 1) * 32 + rr] + red[((2 * c2 + 1) * 2 + 1) * 32 + rr];
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, blockIdx.x, p.N, cs, cq, tid);
            }
            if (p.acc) {
                stat_acc_add(p.acc, p.N, cs, cq, tid);
            }
        }
        if (p.stat_partial) {                                          // the slabs no workgroup owns: zeros
            const int slabs = (p.M + 127) / 128;
            for (long i = (long)gridDim.x * 2 * p.N + (long)blockIdx.x * NT + tid; i < (long)slabs * 2 * p.N; i += (long)gridDim.x * NT) p.stat_partial[i] = 0.0f;
        }
    }
}

static size_t rs64_lds_bytes(const ConvArgs& a) {
    return (size_t)6 * ((a.Win * 8 + 16 + 63) / 64) * 1024 + 128 * (64 * 2 + 16) + 4 * 2 * 32 * 4;
}
static int rs64_grid(const ConvArgs& a) {
    // 256 workgroups whatever the group count (a batch's column sums must not depend on it): two batches per launch are then one round of
    // 512 workgroups with 7 steps each at 56 x 56 / batch 64 -- with 512 per batch a workgroup got 3.5 steps for its 5 us of start-up
    // (weights, first window) and a two-batch launch two rounds: 52.7 us against 67 for the ring kernel; so: 
    const int steps = (a.M / (a.Hout * a.Wout)) * (a.Hout / 2);
    return steps < 256 ? steps : 256;
}

// 3 x 3 / stride 1 / padding 1 over 64 channels of a dense NHWC tensor, 64 output channels, an even number of output rows of 49 to 64
// pixels (two rows = four 32-pixel tasks), at least as many 128-pixel statistics slabs as workgroups
bool rs64_ok(const ConvArgs& a) {
    return a.KH == 3 && a.KW == 3 && a.Cin == 64 && a.N == 64 && a.K == 576 && a.ldb == 576 && a.stride == 1 && a.pad == 1 && a.padw == 1 &&
           a.sW == 64 && a.sH == (long)a.Win * 64 && a.sN == (long)a.Hin * a.sH && a.Wout == a.Win && a.Hout == a.Hin && (a.Hout & 1) == 0 &&
           a.Wout > 48 && a.Wout <= 64 && (long)a.M == (long)(a.M / (a.Hout * a.Wout)) * a.Hout * a.Wout && !a.in_affine &&
           !a.residual && a.ldc == a.N && rs64_lds_bytes(a) <= 80 * 1024 && (!a.stat_partial || sat_cdiv(a.M, 128) >= rs64_grid(a));
}

int launch_rs64(ConvArgs& a, int groups, hipStream_t s) {
    if (!rs64_ok(a)) return SAT_ERR_UNSUPPORTED;
    static bool raised = false;
    return launch_conv(conv_rs64_kernel, dim3(rs64_grid(a), groups), dim3(256), rs64_lds_bytes(a), s, a, &raised, 80 * 1024);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ... and for the FIRST conv of the Inception-v3 stem (Conv2d_1a_3x3: 3 x 3 / stride 2, no padding, the image's 3 channels padded to one
// 16-byte chunk per pixel -> 32 channels, 299 x 299 -> 149 x 149): K = 72, a GEMM of 1.1 K-steps per workgroup as the ring kernel runs it
// (311 us per three-batch launch, 62 TFLOP/s, for 550 MB that stream in ~130 us).  One output row per step, a window of three input rows of
// which two are new per step (stride 2): a ring of eight row slots (three in use, two landing).  The ring kernel's K order is kept EXACTLY:
// its 16-element MFMA steps over the flattened K = (kernel row, kernel column, channel) are pairs of pixels t = 2 j + h of the 3 x 3 window
// (t = 9: the zero half of the fifth step) -- one 16-byte read per lane, the pixel's chunk of its input row's slot -- so the output tensor
// is bit-identical to it.  Column sums per output row as in conv_rs_kernel: statistics signature 7000.
__global__ __launch_bounds__(256, 2) void conv_rs8_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BN = 32, NT = 256, NWV = 4, KS = 5, NSLOT = 8;
    constexpr int ITS = (160 * (BN / 8) + NT - 1) / NT;                // 3
    constexpr int CROW = BN * 2 + 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // eight row slots | C row (160 pixels) | column-sum scratch
    const int rowp = p.Win;                                            // 16-byte pieces of one input row (one per pixel)
    const int ppw = (rowp + 2 + 63) >> 6;                              // LDS row = [zero pixel][the row][>= one zero pixel] in whole 1 KB instructions
    const int pitchb = ppw * 1024;
    char* ctile = smem + NSLOT * pitchb;
    float* red = (float*)(ctile + 160 * CROW);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    // weights: [32][72]; K-step j, half h = elements 16 j + 8 h .. + 7 (past 72: zeros)
    bf16x8 bf[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        const int k0 = 16 * j + 8 * h;
        const u32x4 z = {0u, 0u, 0u, 0u};
        bf[j] = k0 < 72 ? *(const bf16x8*)(p.B + (long)r * p.ldb + k0) : __builtin_bit_cast(bf16x8, z);
    }

    auto issue_row = [&](int n, int hi) {
        char* slot = smem + (hi & (NSLOT - 1)) * pitchb;
        const bf16_t* rowsrc = p.A + ((long)n * p.sN + (long)hi * p.sH);
        for (int k = wave; k < ppw; k += NWV) {
            const int d = k * 64 + lane - 1;                           // input pixel of this piece (piece 0 is the zero pixel)
            const bf16_t* src = (d >= 0 && d < rowp) ? rowsrc + d * 8 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(slot + k * 1024), 16, 0, 0);
        }
    };

    const int rows = p.M / p.Wout;
    const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t0 = blockIdx.x * per, t1 = t0 + per < rows ? t0 + per : rows;
    const int ntask = (p.Wout + 31) >> 5;

    bool fresh = true;
    for (int t = t0; t < t1; ++t) {
        const int n = t / p.Hout, ho = t - n * p.Hout;
        const int hi0 = 2 * ho;
        if (fresh) {
            issue_row(n, hi0);
            issue_row(n, hi0 + 1);
            issue_row(n, hi0 + 2);
            wait_vmcnt<0>();
        } else {
            wait_vmcnt<ITS>();                                         // all but row t - 1's output stores: the two prefetched input rows have landed
        }
        __syncthreads();
        fresh = ho + 1 == p.Hout;
        if (!fresh && t + 1 < t1) {
            issue_row(n, hi0 + 3);                                     // (their slots held rows hi0 - 5 and hi0 - 4)
            issue_row(n, hi0 + 4);
        }
        float ssum = 0.0f, qsum = 0.0f;
        for (int task = wave; task < ntask; task += NWV) {
            const int px0 = task * 32 + r;
            const int wo = px0 < p.Wout ? px0 : 0;
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
            for (int j = 0; j < KS; ++j) {
                const int tpx = 2 * j + h;                             // pixel of the 3 x 3 window (9: none -- the zero pixel of a slot)
                const int kh = tpx / 3, kw = tpx - kh * 3;
                const char* src = smem + ((hi0 + (tpx < 9 ? kh : 0)) & (NSLOT - 1)) * pitchb + (tpx < 9 ? (2 * wo + kw + 1) * 16 : 0);      // (t = 9: the zero pixel in front of this step's first row)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)src, bf[j], acc, 0, 0, 0);
            }
            const float osc = p.out_scale ? p.out_scale[r] : 1.0f, osh = p.out_scale ? p.out_shift[r] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int px = task * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float v = px < p.Wout ? acc[e] : 0.0f;
                ssum += v;
                qsum += v * v;
                if (p.out_scale) v = v * osc + osh;                    // (inference epilogue: the ring kernel's arithmetic)
                if (p.out_relu) v = fmaxf(v, 0.0f);
                *(bf16_t*)(ctile + px * CROW + r * 2) = (bf16_t)v;
            }
        }
        if (p.stat_partial || p.acc) {
            const float s = ssum + __shfl_xor(ssum, 32, 64), q = qsum + __shfl_xor(qsum, 32, 64);
            if (h == 0) {
                red[(wave * 2 + 0) * BN + r] = s;
                red[(wave * 2 + 1) * BN + r] = q;
            }
        }
        __syncthreads();
        if ((p.stat_partial || p.acc) && tid < BN) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int g = 0; g < NWV; ++g) {
                s += red[(g * 2 + 0) * BN + tid];
                q += red[(g * 2 + 1) * BN + tid];
            }
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, t, p.N, s, q, tid);
            }
            if (p.acc) {
                stat_acc_add(p.acc, p.N, s, q, tid);
            }
        }
        {
            bf16_t* crow = p.C + (long)t * p.Wout * p.ldc;
            const int nq = p.Wout * (BN / 8);
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                int qid = tid + it * NT;
                if (qid >= nq) qid = nq - 1;
                const int px = qid >> 2, cc = qid & 3;
                store16_wt(crow + (long)px * p.ldc + cc * 8, *(const u32x4*)(ctile + px * CROW + cc * 16));
            }
        }
    }
    if (p.stat_partial) {
        const int slabs = (p.M + 127) / 128;
        for (long i = (long)rows * 2 * p.N + (long)blockIdx.x * NT + tid; i < (long)slabs * 2 * p.N; i += (long)gridDim.x * NT) p.stat_partial[i] = 0.0f;
    }
}

static size_t rs8_lds_bytes(const ConvArgs& a) { return (size_t)8 * ((a.Win + 2 + 63) / 64) * 1024 + 160 * (32 * 2 + 16) + 4 * 2 * 32 * 4; }

// 3 x 3 / stride 2 / no padding over 8 channels (one 16-byte chunk per pixel) of a dense NHWC tensor, 32 output channels, output rows of
// 128 to 160 pixels, at least as many 128-pixel statistics slabs as output rows
bool rs8_ok(const ConvArgs& a) {
    return a.KH == 3 && a.KW == 3 && a.Cin == 8 && a.N == 32 && a.K == 72 && a.ldb == 72 && a.stride == 2 && a.pad == 0 && a.padw == 0 &&
           a.sW == 8 && a.sH == (long)a.Win * 8 && a.sN == (long)a.Hin * a.sH && a.Wout >= 128 && a.Wout <= 160 && a.Wout == (a.Win - 3) / 2 + 1 &&
           a.Hout == (a.Hin - 3) / 2 + 1 && a.Hout >= 1 && (long)a.M == (long)(a.M / a.Wout) * a.Wout && !a.in_affine &&
           !a.residual && a.ldc == a.N && rs8_lds_bytes(a) <= 64 * 1024;
}

int launch_rs8(ConvArgs& a, int groups, hipStream_t s) {
    if (!rs8_ok(a)) return SAT_ERR_UNSUPPORTED;
    const int rows = a.M / a.Wout;
    return launch_conv(conv_rs8_kernel, dim3(rows < 512 ? rows : 512, groups), dim3(256), rs8_lds_bytes(a), s, a);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ... and for ResNet's own stem in the op program's layout (conv_stem_kernel's geometry, sat_conv_stem.inc: a "7 x 1" kernel over 32-element
// rows of 8 pixels x 4 channels of the zero-bordered NHWC4 image, stride 2, 64 output channels; `self.resnet(images)`, models.py:27).  The
// stem kernel loads the seven input rows of every output row afresh (3.5 x the input through L2 -> LDS, per-tile bookkeeping of up to three
// row segments): 95 us per two-batch launch for 260 MB = 2.7 TB/s.  Here one output row per step, a window of seven input rows of which
// two are new per step (a ring of sixteen 2 KB slots), wave w computes pixels 32 w .. 32 w + 31, the column sums stay in registers over a
// workgroup's whole run of rows (there are more output rows than 128-pixel statistics slabs): statistics signature 7002.  K order = the stem
// kernel's = the ring kernel's: bit-identical output.
__global__ __launch_bounds__(256, 2) void conv_rs_stem_kernel(const ConvArgs p_) {
    const ConvArgs p = group_args(p_);
    constexpr int BN = 64, NT = 256, KH = 7, KS = 14, NSLOT = 16, ITS = 4;
    constexpr int CROW = BN * 2 + 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // sixteen row slots | C row (128 pixels) | column-sum scratch
    const int rowp = p.Win >> 1;                                       // 16-byte pieces of one input row (8 bytes per pixel)
    const int ppw = (rowp + 63) >> 6;
    const int pitchb = ppw * 1024;
    char* ctile = smem + NSLOT * pitchb;
    float* red = (float*)(ctile + 128 * CROW);                         // [4 waves][2][64]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const bf16_t* zero = (const bf16_t*)&g_zero16;

    bf16x8 bf[2][KS];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bf[j][ks] = *(const bf16x8*)(p.B + (long)(j * 32 + r) * p.ldb + ks * 16 + h * 8);

    auto issue_row = [&](int n, int hi) {
        char* slot = smem + (hi & (NSLOT - 1)) * pitchb;
        const bf16_t* rowsrc = p.A + ((long)n * p.sN + (long)hi * p.sH);
        for (int k = wave; k < ppw; k += 4) {
            const int d = k * 64 + lane;
            const bf16_t* src = d < rowp ? rowsrc + d * 8 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(slot + k * 1024), 16, 0, 0);
        }
    };

    const int rows = p.M / p.Wout;
    const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t0 = blockIdx.x * per, t1 = t0 + per < rows ? t0 + per : rows;
    const int px0 = wave * 32 + r;
    const int aoff = (px0 < p.Wout ? px0 : 0) * (p.stride * p.sW * 2) + h * 16;
    float ssum[2] = {0.0f, 0.0f}, qsum[2] = {0.0f, 0.0f};

    bool fresh = true;
    for (int t = t0; t < t1; ++t) {
        const int n = t / p.Hout, ho = t - n * p.Hout;
        const int hi0 = ho * p.stride;
        if (fresh) {
            for (int kh = 0; kh < KH; ++kh) issue_row(n, hi0 + kh);
            wait_vmcnt<0>();
        } else {
            wait_vmcnt<ITS>();
        }
        __syncthreads();
        fresh = ho + 1 == p.Hout;
        if (!fresh && t + 1 < t1)
            for (int q = 0; q < p.stride; ++q) issue_row(n, hi0 + KH + q);      // (their slots held rows the window left at least seven rows ago)
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
        if (wave * 32 < p.Wout) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 af = *(const bf16x8*)(smem + ((hi0 + (ks >> 1)) & (NSLOT - 1)) * pitchb + aoff + (ks & 1) * 32);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[0][ks], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[1][ks], acc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float osc = p.out_scale ? p.out_scale[j * 32 + r] : 1.0f, osh = p.out_scale ? p.out_shift[j * 32 + r] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int px = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float v = px < p.Wout ? acc[j][e] : 0.0f;
                ssum[j] += v;
                qsum[j] += v * v;
                if (p.out_scale) v = v * osc + osh;                    // (inference epilogue: the ring kernel's arithmetic)
                if (p.out_relu) v = fmaxf(v, 0.0f);
                *(bf16_t*)(ctile + px * CROW + (j * 32 + r) * 2) = (bf16_t)v;
            }
        }
        __syncthreads();
        {
            bf16_t* crow = p.C + (long)t * p.Wout * p.ldc;
            const int nq = p.Wout * (BN / 8);
#pragma unroll
            for (int it = 0; it < ITS; ++it) {
                int qid = tid + it * NT;
                if (qid >= nq) qid = nq - 1;
                const int px = qid >> 3, cc = qid & 7;
                store16_wt(crow + (long)px * p.ldc + cc * 8, *(const u32x4*)(ctile + px * CROW + cc * 16));
            }
        }
    }
    if (p.stat_partial || p.acc) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float s = ssum[j] + __shfl_xor(ssum[j], 32, 64), q = qsum[j] + __shfl_xor(qsum[j], 32, 64);
            if (h == 0) {
                red[(wave * 2 + 0) * BN + j * 32 + r] = s;
                red[(wave * 2 + 1) * BN + j * 32 + r] = q;
            }
        }
        __syncthreads();
        if (tid < BN) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                s += red[(g * 2 + 0) * BN + tid];
                q += red[(g * 2 + 1) * BN + tid];
            }
            if (p.stat_partial) {
                stat_slab_store(p.stat_partial, blockIdx.x, p.N, s, q, tid);
            }
            if (p.acc) {
                stat_acc_add(p.acc, p.N, s, q, tid);
            }
        }
        if (p.stat_partial) {
            const int slabs = (p.M + 127) / 128;
            for (long i = (long)gridDim.x * 2 * p.N + (long)blockIdx.x * NT + tid; i < (long)slabs * 2 * p.N; i += (long)gridDim.x * NT) p.stat_partial[i] = 0.0f;
        }
    }
}

static size_t rs_stem_lds_bytes(const ConvArgs& a) { return (size_t)16 * ((a.Win / 2 + 63) / 64) * 1024 + 128 * (64 * 2 + 16) + 4 * 2 * 64 * 4; }
static int rs_stem_grid(const ConvArgs& a) { const int rows = a.M / a.Wout; return rows < 512 ? rows : 512; }

// conv_stem_kernel's geometry with output rows of at most 128 pixels and stride 1 or 2 (a window of seven rows, at most two new per step)
bool rs_stem_ok(const ConvArgs& a) {
    return a.KH == 7 && a.KW == 1 && a.Cin == 32 && a.N == 64 && a.K == 224 && a.ldb == 224 && a.sW == 4 && a.pad == 0 && a.padw == 0 &&
           a.stride >= 1 && a.stride <= 2 && a.sH == (long)a.Win * 4 && a.sN == (long)a.Hin * a.sH && (a.Win % 2) == 0 && a.Wout >= 64 &&
           a.Wout <= 128 && (long)(a.Wout - 1) * a.stride + 8 <= a.Win && (long)(a.Hout - 1) * a.stride + 7 <= a.Hin && !a.in_affine &&
           !a.residual && a.ldc == 64 && (long)a.M == (long)(a.M / a.Wout) * a.Wout && rs_stem_lds_bytes(a) <= 64 * 1024 &&
           (!a.stat_partial || sat_cdiv(a.M, 128) >= rs_stem_grid(a));          // (conv_stem_kernel's geometry; the inference epilogue is run here too)
}

int launch_rs_stem(ConvArgs& a, int groups, hipStream_t s) {
    if (!rs_stem_ok(a)) return SAT_ERR_UNSUPPORTED;
    return launch_conv(conv_rs_stem_kernel, dim3(rs_stem_grid(a), groups), dim3(256), rs_stem_lds_bytes(a), s, a);
}
