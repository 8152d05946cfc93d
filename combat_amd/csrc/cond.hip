// Label conditioning of the multi-label generator (CUnetGeneratorv1, networks/models.py:472-555).  The reference
// concatenates num_classes constant one-hot planes to conv0_0's output (:525-530) and runs conv0_1 over nf + num_classes
// channels.  The planes are constant over space and LeakyReLU leaves 0 and 1 alone, so their share of conv0_1's raw
// output depends on the label, the output channel and on which taps of the 3 x 3 window are inside the map only:
//
//   conv0_1(cat(lrelu(f0), onehot))[n][y][x][o] = conv(lrelu(f0), W_f)[n][y][x][o] + cond[n][y][x][o]
//   cond[n][y][x][o] = sum over the taps (r, s) with 0 <= y + r - 1 < hw and 0 <= x + s - 1 < hw of W_y[o][y_n][r][s]
//
// with W_f = weight[:, :nf] and W_y = weight[:, nf:].  combat_cond_fwd writes cond (the add_pre operand of conv0_1's
// 64-channel launch), combat_cond_wgrad the gradient of W_y from the gradient of conv0_1's raw output, and merges the
// 64-channel launch's W_f gradient into the parameter's [nf][9][nf + num_classes] gradient.  DESIGN.md section 12.
//
// A pixel belongs to one of nine regions (yr, xr), yr = 0 (y == 0), 1 (0 < y < hw - 1), 2 (y == hw - 1), xr alike:
// tap (r, s) is inside the map on the regions with yr != r's excluded row (r == 0 excludes yr == 0, r == 2 excludes
// yr == 2) and the same for the columns.  hw >= 2, so the first and the last row differ.
#include "common.hpp"
#include "plan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxNf = 256;

__device__ __forceinline__ int border_class(int i, int hw) { return i == 0 ? 0 : (i == hw - 1 ? 2 : 1); }
// is tap index r (0..2) of a window centred on a pixel of border class yr inside the map?
__device__ __forceinline__ bool tap_inside(int r, int yr) { return !(r == 0 && yr == 0) && !(r == 2 && yr == 2); }

// One workgroup per image.  table[region][o] = bf16(fp32 sum of the inside taps of W_y[o][label], tap index ascending
// from 0.0f) in LDS, then every thread copies 16-byte groups of 8 channels: consecutive threads write consecutive
// 16 bytes.  A label outside 0..num_classes-1 (F.one_hot raises on it) conditions on nothing: zeros.
__global__ __launch_bounds__(kThreads) void cond_fwd_kernel(const float *__restrict__ wy, const int32_t *__restrict__ labels,
                                                            int hw, int nf, int classes, uint4 *__restrict__ cond) {
    __shared__ __attribute__((aligned(16))) __bf16 table[9 * kMaxNf];
    const int img = blockIdx.x, t = threadIdx.x;
    const int label = labels[img];
    const bool known = label >= 0 && label < classes;
    const int pitch = nf + classes;
    for (int e = t; e < 9 * nf; e += kThreads) {
        const int region = e / nf, o = e - region * nf;
        const int yr = region / 3, xr = region - yr * 3;
        float s = 0.0f;
        if (known) {
            const float *w = wy + (long)o * 9 * pitch + label;
            for (int tap = 0; tap < 9; ++tap) {
                const int r = tap / 3, c = tap - r * 3;
                if (tap_inside(r, yr) && tap_inside(c, xr)) s += w[tap * pitch];
            }
        }
        table[e] = (__bf16)s;
    }
    __syncthreads();
    const int G = nf / 8;
    uint4 *dst = cond + (long)img * hw * hw * G;
    const uint4 *tab = reinterpret_cast<const uint4 *>(table);
    for (int e = t; e < hw * hw * G; e += kThreads) {
        const int p = e / G, g = e - p * G;
        const int y = p / hw, x = p - y * hw;
        dst[e] = tab[(border_class(y, hw) * 3 + border_class(x, hw)) * G + g];
    }
}

// Stage 1 of the weight gradient, one workgroup per image: taps[img][tap][o] = sum of d[img][y][x][o] over the pixels
// where the tap is inside the map.  With G = nf / 8 and L = 256 / G, thread (g, l) = (t % G, t / G) adds the pixels
// l, l + L, ... of its 8 channels into nine region sums (a pixel adds +0.0f to the eight regions it is not in); the L
// lane sums of a region and channel meet in LDS and are added in lane order; a tap's sum is its regions' sums added in
// region order.  Additions only: no difference of large sums.
__global__ __launch_bounds__(kThreads) void cond_taps_kernel(const u32x4_t *__restrict__ d, int hw, int nf,
                                                             float *__restrict__ taps) {
    __shared__ float part[kThreads * 8];      // [L][nf]: L * nf = 2048
    __shared__ float region[9 * kMaxNf];
    const int img = blockIdx.x, t = threadIdx.x;
    const int P = hw * hw, G = nf / 8, L = kThreads / G;
    const int g = t % G, l = t / G;
    const u32x4_t *src = d + (long)img * P * G;
    float acc[9][8];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.0f;
    for (int p = l; p < P; p += L) {
        float v[8];
        unpack8v(src[(long)p * G + g], v);
        const int y = p / hw, x = p - y * hw;
        const int rid = border_class(y, hw) * 3 + border_class(x, hw);
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[k][j] += rid == k ? v[j] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part[l * nf + g * 8 + j] = acc[k][j];
        __syncthreads();
        for (int c = t; c < nf; c += kThreads) {
            float s = 0.0f;
            for (int q = 0; q < L; ++q) s += part[q * nf + c];
            region[k * nf + c] = s;
        }
        __syncthreads();
    }
    float *dst = taps + (long)img * 9 * nf;
    for (int e = t; e < 9 * nf; e += kThreads) {
        const int tap = e / nf, c = e - tap * nf;
        const int r = tap / 3, s = tap - r * 3;
        float sum = 0.0f;
        bool first = true;
        for (int k = 0; k < 9; ++k) {
            const int yr = k / 3, xr = k - yr * 3;
            if (!tap_inside(r, yr) || !tap_inside(s, xr)) continue;
            sum = first ? region[k * nf + c] : sum + region[k * nf + c];
            first = false;
        }
        dst[e] = sum;
    }
}

// Stage 2: dw[o][tap][nf + c] = sum over the images with label c, image index ascending from 0.0f, of taps[img][tap][o]
// (a class no image carries gets exactly 0), and dw[o][tap][i] = dwf[o][tap][i] for i < nf if dwf is given.  One thread
// per written element; o is the fastest index of the class part (the reads of `taps` are consecutive).
__global__ __launch_bounds__(kThreads) void cond_wgrad_merge_kernel(const float *__restrict__ taps,
                                                                    const int32_t *__restrict__ labels, int n, int nf,
                                                                    int classes, const float *__restrict__ dwf,
                                                                    float *__restrict__ dw) {
    const int pitch = nf + classes;
    const int ny = classes * 9 * nf, nw = dwf ? nf * 9 * nf : 0;
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e < ny) {
        const int c = e / (9 * nf), rem = e - c * 9 * nf;
        const int tap = rem / nf, o = rem - tap * nf;
        float s = 0.0f;
        for (int img = 0; img < n; ++img)
            if (labels[img] == c) s += taps[((long)img * 9 + tap) * nf + o];
        dw[((long)o * 9 + tap) * pitch + nf + c] = s;
    } else if (e < ny + nw) {
        const int f = e - ny;
        const int row = f / nf, i = f - row * nf;      // row = o * 9 + tap
        dw[(long)row * pitch + i] = dwf[f];
    }
}

bool misaligned(const void *p, uintptr_t a) { return !p || ((uintptr_t)p & (a - 1)); }

bool bad_shape(int n, int hw, int nf, int classes) {
    // nf: 8 channels per 16-byte group and a whole number of pixel lanes per workgroup (256 / (nf / 8))
    return n < 0 || hw < 2 || hw > 1024 || (nf != 8 && nf != 16 && nf != 32 && nf != 64 && nf != 128 && nf != 256) ||
           classes < 1 || classes > 1024;
}

}  // namespace

extern "C" int combat_cond_fwd(const float *W_y, const int32_t *labels, int32_t n, int32_t hw_map, int32_t nf,
                               int32_t num_classes, void *cond_out, void *stream) {
    COMBAT_PLAN_HOOK(combat_cond_fwd, W_y, labels, n, hw_map, nf, num_classes, cond_out);
    if (bad_shape(n, hw_map, nf, num_classes)) return COMBAT_EINVAL;
    if (misaligned(W_y, 4) || misaligned(labels, 4) || misaligned(cond_out, 16)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    COMBAT_LAUNCH(cond_fwd_kernel, dim3(n), dim3(kThreads), 0, as_stream(stream), W_y, labels, hw_map, nf, num_classes,
                  static_cast<uint4 *>(cond_out));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_cond_wgrad(const void *d, const int32_t *labels, int32_t n, int32_t hw_map, int32_t nf,
                                 int32_t num_classes, const float *dwf, float *dw, float *scratch, void *stream) {
    COMBAT_PLAN_HOOK(combat_cond_wgrad, d, labels, n, hw_map, nf, num_classes, dwf, dw, scratch);
    if (bad_shape(n, hw_map, nf, num_classes)) return COMBAT_EINVAL;
    if (misaligned(d, 16) || misaligned(labels, 4) || misaligned(dw, 4) || misaligned(scratch, 4)) return COMBAT_EINVAL;
    if (dwf && ((uintptr_t)dwf & 3)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;      // (nothing written: the caller's zeroed gradient stays zero)
    COMBAT_LAUNCH(cond_taps_kernel, dim3(n), dim3(kThreads), 0, as_stream(stream), static_cast<const u32x4_t *>(d), hw_map, nf,
                  scratch);
    CB_LAUNCH_CHECK();
    const int total = num_classes * 9 * nf + (dwf ? nf * 9 * nf : 0);
    COMBAT_LAUNCH(cond_wgrad_merge_kernel, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0, as_stream(stream),
                  scratch, labels, n, nf, num_classes, dwf, dw);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}
