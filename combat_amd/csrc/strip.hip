// STRIP defense (defenses/STRIP/STRIP.py; Gao et al., ACSAC 2019): every background image is superimposed with S images
// drawn from the test set, the classifier sees the B * S blends, and the mean entropy of a background's S predictions is
// its score.
//
// Replaces: the per-image cv2.addWeighted + ToTensor + Normalize + torch.stack(...).to(device) of STRIP.py:60-75 by one
// launch that writes the classifier's input buffer from uint8 sources (combat_strip_superimpose; no float image ever
// exists), and torch.sigmoid(...).cpu().numpy() + np.nansum(p * np.log2(p)) / n_sample of :76-78 by one launch on the
// head's logits (combat_strip_entropy).  DESIGN.md section 9.
#include "common.hpp"
#include "plan.hpp"

namespace {

constexpr int kMaxClasses = 16;
constexpr int kTilePixels = 1024;   // pixels of ONE image per workgroup pass: 256 threads x 4 pixels

struct u8x12 {   // four RGB pixels = three aligned dwords
    uint32_t a, b, c;
};

// saturating per-byte add of two packed dwords: cv2.addWeighted(a, 1, b, 1, 0) on uint8 = min(a + b, 255)
__device__ __forceinline__ void sat_add12(const u8x12 &p, const u8x12 &q, int (&s)[12]) {
    const uint32_t pw[3] = {p.a, p.b, p.c}, qw[3] = {q.a, q.b, q.c};
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int v = (int)((pw[w] >> (8 * k)) & 0xffu) + (int)((qw[w] >> (8 * k)) & 0xffu);
            s[w * 4 + k] = v < 255 ? v : 255;
        }
}

// A workgroup pass covers 1024 consecutive pixels of one blended image, so the image number, its background and its
// overlay index are the same for the whole workgroup.  A thread reads 12 bytes = 4 pixels of each source as three
// dwords (hw * hw is a multiple of 4 and hw a multiple of 4: the four pixels share a row) and writes four 16-byte c8
// pixels.  float(s) / 255.0f is a true division (ToTensor): s * (1 / 255.0f) differs in the last bit for some s.
__global__ __launch_bounds__(256) void strip_superimpose_kernel(const uint8_t *__restrict__ backgrounds, int S,
                                                                const uint8_t *__restrict__ dataset, int n_data,
                                                                const int32_t *__restrict__ index, int hw, int norm_cols,
                                                                long tiles, int tiles_per_image,
                                                                uint4 *__restrict__ out) {
    const int hw2 = hw * hw;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int img = (int)(t / tiles_per_image);
        const int p0 = ((int)(t - (long)img * tiles_per_image) * 256 + (int)threadIdx.x) * 4;   // first of this thread's pixels
        if (p0 >= hw2) continue;
        const int ov = index[img];
        const u8x12 bg = *reinterpret_cast<const u8x12 *>(backgrounds + (long)(img / S) * hw2 * 3 + (long)p0 * 3);
        u8x12 od = {0u, 0u, 0u};                                 // an index outside the dataset: nothing is added
        if ((unsigned)ov < (unsigned)n_data) od = *reinterpret_cast<const u8x12 *>(dataset + (long)ov * hw2 * 3 + (long)p0 * 3);
        int s[12];
        sat_add12(bg, od, s);
        const int x0 = p0 % hw;
        uint4 *dst = out + (long)img * hw2 + p0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = (float)s[j * 3 + c] / 255.0f;
                if (x0 + j < norm_cols) v[c] = (v[c] - 0.5f) / 0.5f;
            }
            dst[j] = hilo_pixel(v[0], v[1], v[2]);
        }
    }
}

// One wave per background: lane l takes cells l, l + 64, ... of the background's S * classes logits (consecutive in
// memory), each term p * log2(p) in fp32 as the reference computes it, the sum in fp64 (lane partial sums, then a
// butterfly over the wave: a fixed order, so two runs give the same bits).  0 * -inf (p == 0) and NaN logits give a
// NaN term, which np.nansum leaves out: so does the test below.
__global__ __launch_bounds__(64) void strip_entropy_kernel(const float *__restrict__ logits, int S, int classes,
                                                           float *__restrict__ out) {
    const int b = blockIdx.x;
    const long cells = (long)S * classes;
    const float *row = logits + (long)b * cells;
    double acc = 0.0;
    for (long i = threadIdx.x; i < cells; i += 64) {
        const float p = 1.0f / (1.0f + expf(-row[i]));
        const float term = p * log2f(p);
        if (term == term) acc += (double)term;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (threadIdx.x == 0) out[b] = (float)(-acc / (double)S);
}

}  // namespace

extern "C" int combat_strip_superimpose(const void *backgrounds, int32_t B, const void *dataset, int32_t n_data,
                                        const int32_t *index, int32_t S, int32_t hw, int32_t norm_cols, void *out_c8,
                                        void *stream) {
    COMBAT_PLAN_HOOK(combat_strip_superimpose, backgrounds, B, dataset, n_data, index, S, hw, norm_cols, out_c8);
    if (B < 0 || S < 0 || n_data < 0) return COMBAT_EINVAL;
    if (hw != 32 && hw != 64 && hw != 224) return COMBAT_EINVAL;
    if (norm_cols < 0 || norm_cols > hw) return COMBAT_EINVAL;
    if ((long)B * S > INT32_MAX) return COMBAT_EINVAL;
    if (!backgrounds || !dataset || !index || !out_c8) return COMBAT_EINVAL;
    if (((uintptr_t)backgrounds | (uintptr_t)dataset | (uintptr_t)index) & 3 || (uintptr_t)out_c8 & 15) return COMBAT_EINVAL;
    if (B == 0 || S == 0) return COMBAT_OK;
    const int tiles_per_image = (hw * hw + kTilePixels - 1) / kTilePixels;
    const long tiles = (long)B * S * tiles_per_image;
    const int grid = (int)(tiles < 8192 ? tiles : 8192);
    COMBAT_LAUNCH(strip_superimpose_kernel, dim3(grid), dim3(256), 0, as_stream(stream),
                  static_cast<const uint8_t *>(backgrounds), S, static_cast<const uint8_t *>(dataset), n_data, index, hw,
                  norm_cols, tiles, tiles_per_image, static_cast<uint4 *>(out_c8));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_strip_entropy(const float *logits, int32_t B, int32_t S, int32_t classes, float *out, void *stream) {
    COMBAT_PLAN_HOOK(combat_strip_entropy, logits, B, S, classes, out);
    if (B < 0 || S < 1 || classes < 1 || classes > kMaxClasses) return COMBAT_EINVAL;
    if ((long)B * S > INT32_MAX) return COMBAT_EINVAL;
    if (!logits || !out) return COMBAT_EINVAL;
    if (B == 0) return COMBAT_OK;
    COMBAT_LAUNCH(strip_entropy_kernel, dim3(B), dim3(64), 0, as_stream(stream), logits, S, classes, out);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}
