// Grad-CAM defense (defenses/gradcam/gradcam.py; Selvaraju et al., ICCV 2017): the map of one image is the ReLU of the
// tapped block's activations weighted by the pixel means of the chosen logit's gradient with respect to them, resized to
// the image and stretched to [0, 1].
//
// Replaces: the one-hot, sum(one_hot * output) and autograd's walk through `linear` and `avgpool` (gradcam.py:168-181) by
// one launch that writes the engine's 'g.feat' buffer (combat_gradcam_seed), and the two host copies, the Python loop
// over the channels, cv2.resize and the normalisation of :183-197 by one workgroup per image (combat_gradcam_map): only
// the finished [n][32][32] maps leave the device.  DESIGN.md section 11.
#include "common.hpp"
#include "plan.hpp"

namespace {

constexpr int kMaxClasses = 16;
constexpr int kThreads = 256;
constexpr int kOut = 32;                       // the maps are 32 x 32: the only classifier input the reference's get_model knows
constexpr int kMaxC = 512;
constexpr int kMaxPixels = 32 * 32;
constexpr int kChunkPasses = 32;               // map: workgroup passes (256 partial sums each) per LDS chunk
constexpr int kRed = kChunkPasses * (kThreads + 32);   // floats: pixels * (G + 1) of a chunk, L <= 32 pixels per pass

// The first maximal class of a row; a NaN never wins against a number (a row of NaNs gives class 0).
__device__ __forceinline__ int first_max(const float *__restrict__ row, int classes) {
    int best = 0;
    float mx = row[0];
    for (int j = 1; j < classes; ++j) {
        const float v = row[j];
        if (v > mx || (mx != mx && v == v)) {
            mx = v;
            best = j;
        }
    }
    return best;
}

// One workgroup per row of the slot.  d(logit k) / d(feat[y][x][c]) = W[k][c] / 16 for each of the 4 x 4 pixels avgpool(4)
// averages: a thread writes 16-byte groups of 8 channels, 16 * C / 8 of them per row.
__global__ __launch_bounds__(kThreads) void gradcam_seed_kernel(const float *__restrict__ logits,
                                                                const int32_t *__restrict__ index, int n, int classes, int C,
                                                                const float *__restrict__ W, int32_t *__restrict__ chosen,
                                                                uint4 *__restrict__ d_feat) {
    const int img = blockIdx.x;
    const int G = C / 8;
    uint4 *dst = d_feat + (long)img * 16 * G;
    if (img >= n) {                                              // padding of a ragged batch: no class, zero gradients
        if (threadIdx.x == 0) chosen[img] = -1;
        for (int s = threadIdx.x; s < 16 * G; s += kThreads) dst[s] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    int k = index ? index[img] : -1;
    if (k < 0 || k >= classes) k = first_max(logits + (long)img * classes, classes);     // (uniform over the workgroup)
    if (threadIdx.x == 0) chosen[img] = k;
    const float *w = W + (long)k * C;
    for (int s = threadIdx.x; s < 16 * G; s += kThreads) {
        const int g = s % G;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w[g * 8 + j] * 0.0625f;      // / 16.0f, exactly
        dst[s] = pack8(v);
    }
}

// NaN-propagating minimum / maximum (np.min / np.max): a NaN on either side is the result.
__device__ __forceinline__ float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// cv2.resize's INTER_LINEAR taps of source coordinate s in a row of f cells: the two neighbours and the weight of the
// second; beyond the first or the last cell the border cell alone (weight 0).
struct Tap {
    int i0, i1;
    float w;
};

__device__ __forceinline__ Tap tap(float s, int f) {
    const float fl = floorf(s);
    Tap r = {(int)fl, 0, s - fl};
    if (r.i0 < 0) {
        r.i0 = 0;
        r.w = 0.0f;
    }
    if (r.i0 >= f - 1) {
        r.i0 = f - 1;
        r.w = 0.0f;
    }
    r.i1 = min(r.i0 + 1, f - 1);
    return r;
}

// One workgroup per image, 256 threads.  With G = C / 8 groups of 8 channels (16 bytes) per pixel and L = 256 / G "pixel
// lanes", thread t is (g, l) = (t % G, t / G): consecutive threads read consecutive 16 bytes, a pass of the workgroup
// 4 KB = L whole pixels.  All sums fp32 in the order the header states (combat_gradcam_map); no atomics.
//   1. weights: thread (g, l) adds the gradient pixels l, l + L, ... of its 8 channels; the L lane sums of a channel
//      meet in LDS and are added in lane order, times 1 / (f * f) (a power of two).
//   2. raw map: thread (g, l) takes the pixels l, l + L, ... and folds its 8 channels into one fused multiply-add chain;
//      the G chains of a pixel meet in LDS (row stride G + 1: the reading threads hit different banks) and are added in
//      group order.  LDS holds kChunkPasses passes at a time; every tapped layer of the classifier (f * C = 2048) is one
//      chunk.
//   3. ReLU, the bilinear resize (4 consecutive output pixels of a row per thread), minimum and maximum through an LDS
//      tree, the division.
__global__ __launch_bounds__(kThreads) void gradcam_map_kernel(const u32x4_t *__restrict__ act, const u32x4_t *__restrict__ grad,
                                                               int f, int C, float *__restrict__ cam, float *__restrict__ raw_out,
                                                               float *__restrict__ weights_out) {
    __shared__ float part[kThreads * 8];          // [L][C]: L * C = 2048
    __shared__ float w[kMaxC];
    __shared__ float red[kRed];
    __shared__ float rawmap[kMaxPixels];
    __shared__ float lo[kThreads], hi[kThreads];

    const int img = blockIdx.x, t = threadIdx.x;
    const int P = f * f, G = C / 8, L = kThreads / G;
    const int g = t % G, l = t / G;
    const u32x4_t *a_img = act + (long)img * P * G;
    const u32x4_t *g_img = grad + (long)img * P * G;

    // ---- 1. channel weights
    {
        float s[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int p = l; p < P; p += L) {
            float v[8];
            unpack8v(g_img[(long)p * G + g], v);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += v[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) part[l * C + g * 8 + j] = s[j];
    }
    __syncthreads();
    const float inv_p = 1.0f / (float)P;
    for (int c = t; c < C; c += kThreads) {
        float s = 0.0f;
        for (int k = 0; k < L; ++k) s += part[k * C + c];
        s *= inv_p;
        w[c] = s;
        if (weights_out) weights_out[(long)img * C + c] = s;
    }
    __syncthreads();

    // ---- 2. the map before ReLU
    float wr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = w[g * 8 + j];
    const int chunk = kChunkPasses * L, stride = G + 1;
    for (int c0 = 0; c0 < P; c0 += chunk) {
        const int end = min(P, c0 + chunk);
        for (int p = c0 + l; p < end; p += L) {
            float v[8];
            unpack8v(a_img[(long)p * G + g], v);
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s = fmaf(wr[j], v[j], s);
            red[(p - c0) * stride + g] = s;
        }
        __syncthreads();
        for (int p = c0 + t; p < end; p += kThreads) {
            const float *row = red + (p - c0) * stride;
            float s = 0.0f;
            for (int k = 0; k < G; ++k) s += row[k];
            rawmap[p] = s;
            if (raw_out) raw_out[(long)img * P + p] = s;
        }
        __syncthreads();
    }

    // ---- 3. ReLU, resize, normalise.  Thread t: row t / 8, columns 4 * (t % 8) .. + 3.
    const float scale = (float)f / (float)kOut;
    const int dy = t / 8;
    const float sy = ((float)dy + 0.5f) * scale - 0.5f;
    const Tap ty = tap(sy, f);
    float u[4];
    float mn = 0.0f, mx = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dx = (t % 8) * 4 + j;
        const float sx = ((float)dx + 0.5f) * scale - 0.5f;
        const Tap tx = tap(sx, f);
        const float wx = tx.w, wy = ty.w;
        float r[4] = {rawmap[ty.i0 * f + tx.i0], rawmap[ty.i0 * f + tx.i1], rawmap[ty.i1 * f + tx.i0], rawmap[ty.i1 * f + tx.i1]};
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = r[q] < 0.0f ? 0.0f : r[q];      // np.maximum(cam, 0): a NaN stays
        const float top = (1.0f - wx) * r[0] + wx * r[1];
        const float bot = (1.0f - wx) * r[2] + wx * r[3];
        u[j] = (1.0f - wy) * top + wy * bot;
        mn = j == 0 ? u[j] : min_nan(mn, u[j]);
        mx = j == 0 ? u[j] : max_nan(mx, u[j]);
    }
    lo[t] = mn;
    hi[t] = mx;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            lo[t] = min_nan(lo[t], lo[t + s]);
            hi[t] = max_nan(hi[t], hi[t + s]);
        }
        __syncthreads();
    }
    mn = lo[0];
    const float den = hi[0] - mn;                // max(u - min): subtraction is monotonic
    float *dst = cam + (long)img * kOut * kOut + t * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = (u[j] - mn) / den;      // a constant map: 0 / 0 = NaN, as the reference's
}

bool misaligned(const void *p, uintptr_t a) { return !p || ((uintptr_t)p & (a - 1)); }

}  // namespace

extern "C" int combat_gradcam_seed(const float *logits, const int32_t *index, int32_t n, int32_t N, int32_t classes, int32_t C,
                                   const float *W, int32_t *chosen, void *d_feat, void *stream) {
    COMBAT_PLAN_HOOK(combat_gradcam_seed, logits, index, n, N, classes, C, W, chosen, d_feat);
    if (classes < 1 || classes > kMaxClasses || C < 8 || (C & 7) || n < 0 || N < 1 || n > N) return COMBAT_EINVAL;
    if (misaligned(logits, 4) || misaligned(W, 4) || misaligned(chosen, 4) || misaligned(d_feat, 16)) return COMBAT_EINVAL;
    if (index && ((uintptr_t)index & 3)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    COMBAT_LAUNCH(gradcam_seed_kernel, dim3(N), dim3(kThreads), 0, as_stream(stream), logits, index, n, classes, C, W, chosen,
                  static_cast<uint4 *>(d_feat));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_gradcam_map(const void *act, const void *grad, int32_t n, int32_t f, int32_t C, int32_t out_hw, float *cam,
                                  float *raw, float *weights, void *stream) {
    COMBAT_PLAN_HOOK(combat_gradcam_map, act, grad, n, f, C, out_hw, cam, raw, weights);
    if (f != 4 && f != 8 && f != 16 && f != 32) return COMBAT_EINVAL;
    if (C != 64 && C != 128 && C != 256 && C != 512) return COMBAT_EINVAL;
    if (out_hw != kOut || n < 0) return COMBAT_EINVAL;
    if (misaligned(act, 16) || misaligned(grad, 16) || misaligned(cam, 4)) return COMBAT_EINVAL;
    if ((raw && ((uintptr_t)raw & 3)) || (weights && ((uintptr_t)weights & 3))) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    COMBAT_LAUNCH(gradcam_map_kernel, dim3(n), dim3(kThreads), 0, as_stream(stream), static_cast<const u32x4_t *>(act),
                  static_cast<const u32x4_t *>(grad), f, C, cam, raw, weights);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}
