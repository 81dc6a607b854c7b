// On-device image augmentation (main.py:26-36, data_loader.py:29-32): RandomCrop / CenterCrop + RandomHorizontalFlip +
// ToTensor + Normalize of a batch of uint8 HWC images in one launch -- the host hands over the decoded bytes (3.06x fewer than
// the f32 tensor over PCIe) and the f32 NCHW tensor every encoder entry point takes is made in HBM.
//
// There are only 3 x 256 possible outputs, so every workgroup first builds the table ((v / 255) - mean[c]) / std[c] in LDS with
// the two IEEE divisions torch's CPU kernels do (ToTensor's div(255), Normalize's sub_(mean).div_(std)); this file is compiled
// without fast-math and neither division is a multiplication by a reciprocal, so the result is bit for bit the reference's.
// The inner loop is then a byte load, a table lookup and a store.
//
// Thread-to-pixel map: a workgroup owns kRows output rows of one image, i.e. 3 * kRows row segments of Wc floats (one per plane).
// A segment is cut where its OUTPUT address is 16-byte aligned: a scalar head of 0..3 floats, 16-byte stores, a scalar tail;
// consecutive lanes take consecutive 16-byte groups of one segment, so the stores of a wave are one contiguous run.  Wc % 4 != 0
// (Inception's 299) gives every row its own head, which is why the cut is made per segment and not per workgroup.  The four
// source bytes of a group sit 3 apart (HWC) at an offset of any alignment: they are loaded per lane as bytes, so no load is wider
// than the byte it needs and none can reach outside the source allocation, first and last row included; the three planes'
// segments of a row follow each other in the workgroup, so the 3 * Wc bytes of a source row come from L1 after their first
// use.  The mirror reverses the index on the read side only.
#include "sat_internal.h"

namespace {
constexpr int kRows = 8;        // output rows per workgroup: amortises the table (768 entries, 6 divisions per thread)

struct rgb_f32 { float v[3]; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// G = Wc / 4 + 2 work items per segment (item 0: head, 1..nvec: 16-byte groups, nvec + 1: tail); step_q / step_r = 256 / G, 256 % G
__global__ __launch_bounds__(256) void image_augment_u8_kernel(const uint8_t* __restrict__ src, int Bsrc, int Hs, int Ws,
                                                               const int32_t* __restrict__ params, const int32_t* __restrict__ order,
                                                               int Hc, int Wc, rgb_f32 mean, rgb_f32 sd, float* __restrict__ out,
                                                               int G, int step_q, int step_r) {
    __shared__ float tab[3 * 256];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (float)threadIdx.x / 255.0f;        // ToTensor: byte -> float, div(255)
        tab[c * 256 + threadIdx.x] = (v - mean.v[c]) / sd.v[c];  // Normalize: sub_(mean).div_(std)
    }
    __syncthreads();

    const int b = blockIdx.x, y0 = blockIdx.y * kRows;
    const int rows = min(kRows, Hc - y0);
    const int sb = clampi(order ? order[b] : b, 0, Bsrc - 1);
    const int top = clampi(params[3 * b], 0, Hs - Hc), left = clampi(params[3 * b + 1], 0, Ws - Wc);
    const bool flip = params[3 * b + 2] != 0;
    const long plane = (long)Hc * Wc, srow_bytes = 3L * Ws;
    const uint8_t* img = src + ((long)sb * Hs + top + y0) * srow_bytes + 3L * left;
    float* ob = out + (long)b * 3 * plane + (long)y0 * Wc;
    const int dp = flip ? -3 : 3;

    const int nseg = rows * 3;
    int seg = threadIdx.x / G, j = threadIdx.x - seg * G;
    while (seg < nseg) {
        const int r = seg / 3, c = seg - r * 3;
        const uint8_t* s = img + r * srow_bytes + c;
        float* o = ob + c * plane + (long)r * Wc;
        const float* t = tab + c * 256;
        const int head = min((int)((0 - ((uintptr_t)o >> 2)) & 3), Wc);
        const int nvec = (Wc - head) >> 2;
        if (j >= 1 && j <= nvec) {
            const int x = head + 4 * (j - 1);
            const uint8_t* p = s + 3L * (flip ? Wc - 1 - x : x);
            const int v0 = p[0], v1 = p[dp], v2 = p[2 * dp], v3 = p[3 * dp];
            *(f32x4*)(o + x) = (f32x4){t[v0], t[v1], t[v2], t[v3]};
        } else if (j == 0 || j == nvec + 1) {
            const int x0 = j ? head + 4 * nvec : 0, x1 = j ? Wc : head;
            for (int x = x0; x < x1; ++x) o[x] = t[s[3L * (flip ? Wc - 1 - x : x)]];
        }
        seg += step_q;
        j += step_r;
        if (j >= G) {
            j -= G;
            ++seg;
        }
    }
}
}  // namespace

extern "C" int sat_image_augment_u8(const uint8_t* src, int Bsrc, int Hs, int Ws, const int32_t* params, const int32_t* order,
                                    int B, int Hc, int Wc, const float* mean, const float* sd, float* out, sat_stream_t stream) {
    if (!src || !params || !out || !mean || !sd || ((uintptr_t)out & 3)) return SAT_ERR_ARG;
    if (B <= 0 || Bsrc <= 0 || Hc <= 0 || Wc <= 0 || Hc > Hs || Wc > Ws) return SAT_ERR_ARG;
    rgb_f32 m, s;
    for (int c = 0; c < 3; ++c) {
        if (mean[c] - mean[c] != 0.0f || sd[c] - sd[c] != 0.0f || sd[c] == 0.0f) return SAT_ERR_ARG;      // x - x: NaN for inf and NaN
        m.v[c] = mean[c];
        s.v[c] = sd[c];
    }
    const int gy = sat_cdiv(Hc, kRows);
    if (gy > 65535 || Wc > (1 << 28)) return SAT_ERR_UNSUPPORTED;       // grid y limit; 3 * Wc and 4 * G stay far inside int
    const int G = Wc / 4 + 2;
    hipLaunchKernelGGL(image_augment_u8_kernel, dim3(B, gy), dim3(256), 0, (hipStream_t)stream, src, Bsrc, Hs, Ws, params, order, Hc,
                       Wc, m, s, out, G, 256 / G, 256 % G);
    SAT_LAUNCH_CHECK();
    return SAT_OK;
}
