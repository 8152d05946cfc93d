// Neural Cleanse defense (defenses/neural_cleanse/detecting.py; Wang et al., IEEE S&P 2019): for one target label a mask
// and a pattern are optimised so that every test image, blended with them, is classified as that label; the L1 norm
// of the mask is the label's score.
//
// Replaces: RegressionModel.forward's blend (detecting.py:27-41) by one launch that writes the classifier's input buffer
// from the uint8 test set (combat_nc_blend; no float image exists), and autograd's walk from the classifier's input
// gradient back to mask_tanh / pattern_tanh, the L1 term, optimizerR.step() (Adam, :151, :192-196) and the mini-batch
// record of :199-205 by one entry point on the engine's 'g.img' (combat_nc_update).  Both read the step within the epoch
// from a device cell, so the arguments of a recorded plan are the same for every step.  DESIGN.md section 10.
#include "common.hpp"
#include "plan.hpp"

namespace {

constexpr int kMaxClasses = 16;
constexpr int kTilePixels = 1024;   // blend: pixels of ONE image per workgroup pass, 256 threads x 4 pixels
constexpr int kPix = 16;            // update: consecutive pixels per workgroup ...
constexpr int kLanes = 16;          // ... times image lanes (image i goes to lane i % 16)

struct u8x12 {   // four RGB pixels = three aligned dwords
    uint32_t a, b, c;
};

// The pattern's Normalize (detecting.py:29-31, :76-78; networks/models.py:22-26) indexes x[:, channel] of the [3][hw][hw]
// pattern, which has no batch axis: the ROW axis.  Row y < 3 of every colour plane becomes (raw - mean[y]) / std[y] and
// rows 3.. stay raw.  Published numbers come from that arithmetic, so it is the arithmetic here.
struct NcNorm {
    float mean[3], std[3];
};

struct NcRow {   // p = (raw - shift) / scale for the pixels of one row
    float shift, scale;
};

__device__ __forceinline__ NcRow row_norm(const NcNorm &nm, int y) {
    NcRow r = {0.0f, 1.0f};
    if (y < 3) {
        r.shift = y == 0 ? nm.mean[0] : y == 1 ? nm.mean[1] : nm.mean[2];
        r.scale = y == 0 ? nm.std[0] : y == 1 ? nm.std[1] : nm.std[2];
    }
    return r;
}

__device__ __forceinline__ NcNorm load_norm(const float *norm) {
    NcNorm r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.mean[c] = norm[c];
        r.std[c] = norm[3 + c];
    }
    return r;
}

// the dataset row of image `img` of step `cur`, or -1: an entry beyond the index, or outside the dataset, reads nothing
__device__ __forceinline__ int source_row(const int32_t *__restrict__ index, int n_index, int n_data, int cur, int bs, int img) {
    const long at = (long)cur * bs + img;
    if (cur < 0 || at >= n_index) return -1;
    const int src = index[at];
    return (unsigned)src < (unsigned)n_data ? src : -1;
}

// ToTensor (a true division by 255) and the test loader's Normalize(0.5, 0.5)
__device__ __forceinline__ float pixel_value(uint32_t byte) { return ((float)byte / 255.0f - 0.5f) / 0.5f; }

// A workgroup pass covers 1024 consecutive pixels of one image; a thread reads 12 bytes = 4 pixels of the source as three
// dwords (hw * hw and hw are multiples of 4), the four mask and 3 x 4 pattern values as 16-byte loads, and writes four
// 16-byte c8 pixels.  tanhf is recomputed per image: 4 * hw * hw values against the classifier pass that follows.
__global__ __launch_bounds__(256) void nc_blend_kernel(const uint8_t *__restrict__ dataset, int n_data,
                                                       const int32_t *__restrict__ index, int n_index,
                                                       const int32_t *__restrict__ cursor, int bs, int n, int hw,
                                                       const float *__restrict__ mask_tanh,
                                                       const float *__restrict__ pattern_tanh, float den,
                                                       const float *__restrict__ norm, long tiles, int tiles_per_image,
                                                       uint4 *__restrict__ out) {
    const int hw2 = hw * hw;
    const int cur = *cursor;
    const NcNorm nm = load_norm(norm);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int img = (int)(t / tiles_per_image);
        const int p0 = ((int)(t - (long)img * tiles_per_image) * 256 + (int)threadIdx.x) * 4;   // first of this thread's pixels
        if (p0 >= hw2) continue;
        uint4 *dst = out + (long)img * hw2 + p0;
        if (img >= n) {                                          // padding of a ragged batch: zero pixels
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const int src = source_row(index, n_index, n_data, cur, bs, img);
        u8x12 px = {0u, 0u, 0u};
        if (src >= 0) px = *reinterpret_cast<const u8x12 *>(dataset + (long)src * hw2 * 3 + (long)p0 * 3);
        const uint32_t pw[3] = {px.a, px.b, px.c};
        const NcRow rn = row_norm(nm, p0 / hw);                  // the four pixels share a row
        const float4 mt4 = *reinterpret_cast<const float4 *>(mask_tanh + p0);
        const float mt[4] = {mt4.x, mt4.y, mt4.z, mt4.w};
        float pt[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 v = *reinterpret_cast<const float4 *>(pattern_tanh + (long)c * hw2 + p0);
            pt[c][0] = v.x; pt[c][1] = v.y; pt[c][2] = v.z; pt[c][3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m = tanhf(mt[j]) / den + 0.5f;
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = j * 3 + c;
                const float x = src >= 0 ? pixel_value((pw[k >> 2] >> (8 * (k & 3))) & 0xffu) : 0.0f;
                const float p = (tanhf(pt[c][j]) / den + 0.5f - rn.shift) / rn.scale;
                v[c] = (1.0f - m) * x + m * p;
            }
            dst[j] = hilo_pixel(v[0], v[1], v[2]);
        }
    }
}

// A workgroup owns 16 consecutive pixels.  Phase 1: thread (pixel, lane) adds the images lane, lane + 16, ... < n in index
// order -- one 16-byte load of the c8 gradient pixel and three bytes of the source per image.  Phase 2: the 16 lane sums of
// a (pixel, parameter) cell are added in lane order by the thread that owns the cell (64 threads: mask + 3 pattern
// channels), which applies the tanh chain, the L1 term and Adam.  No atomics: the same bits every run.  The raw mask
// values of the 16 pixels (before the update) are summed into reg_partial[block] for the statistics row.
__global__ __launch_bounds__(256) void nc_update_kernel(const uint4 *__restrict__ g_img, const uint8_t *__restrict__ dataset,
                                                        int n_data, const int32_t *__restrict__ index, int n_index,
                                                        const int32_t *__restrict__ cursor, int bs, int n, int hw,
                                                        float *__restrict__ mask_tanh, float *__restrict__ pattern_tanh,
                                                        float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                        float den, const float *__restrict__ norm, float lr, float beta1,
                                                        float beta2, float adam_eps, const int32_t *__restrict__ t_cell,
                                                        const float *__restrict__ cost_cell, int steps,
                                                        float *__restrict__ grad_out, float *__restrict__ reg_partial) {
    __shared__ float part[kLanes][kPix][4];
    const int cur = *cursor;
    if (cur < 0 || cur >= steps) return;                         // no statistics row exists for this step: nothing moves
    const int hw2 = hw * hw;
    const int px = (int)threadIdx.x % kPix, lane = (int)threadIdx.x / kPix;
    const int p = (int)blockIdx.x * kPix + px;                   // < hw2: the grid is hw2 / 16 workgroups
    const NcRow rn = row_norm(load_norm(norm), p / hw);
    const float tm = tanhf(mask_tanh[p]);
    const float m = tm / den + 0.5f;
    float tp[3], pn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        tp[c] = tanhf(pattern_tanh[(long)c * hw2 + p]);
        pn[c] = (tp[c] / den + 0.5f - rn.shift) / rn.scale;
    }
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};                     // gm, then the plain sums of g over the images per channel
    for (int i = lane; i < n; i += kLanes) {
        const int src = source_row(index, n_index, n_data, cur, bs, i);
        float x[3] = {0.0f, 0.0f, 0.0f};
        if (src >= 0) {
            const uint8_t *s = dataset + (long)src * hw2 * 3 + (long)p * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = pixel_value(s[c]);
        }
        const uint4 gq = g_img[(long)i * hw2 + p];
        const float g[3] = {bf16_bits_to_f32(gq.x & 0xffffu), bf16_bits_to_f32(gq.x >> 16), bf16_bits_to_f32(gq.y & 0xffffu)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[0] += g[c] * (pn[c] - x[c]);
            acc[1 + c] += g[c];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[lane][px][k] = acc[k];
    __syncthreads();
    if (lane >= 4) return;
    const int k = lane;                                          // 0: the mask, 1..3: pattern channel k - 1
    float sum = 0.0f;
#pragma unroll
    for (int l = 0; l < kLanes; ++l) sum += part[l][px][k];
    const float th = k == 0 ? tm : tp[k - 1];
    const float chain = (1.0f - th * th) / den;
    // d mask_tanh = (gm + cost) * (1 - tanh^2) / (2 + EPSILON): the raw mask is positive, so |.|'s slope is 1
    const float grad = (k == 0 ? sum + *cost_cell : sum * m / rn.scale) * chain;
    const long cell = (long)k * hw2 + p;
    if (grad_out) grad_out[cell] = grad;
    // torch.optim.Adam (no weight decay, no amsgrad); the bias corrections in fp64 like the host's Python floats
    const int t = *t_cell + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const float m1 = beta1 * exp_avg[cell] + (1.0f - beta1) * grad;
    const float m2 = beta2 * exp_avg_sq[cell] + (1.0f - beta2) * grad * grad;
    exp_avg[cell] = m1;
    exp_avg_sq[cell] = m2;
    float *param = k == 0 ? mask_tanh + p : pattern_tanh + (long)(k - 1) * hw2 + p;
    *param = *param - step_size * (m1 / (sqrtf(m2) / bc2_sqrt + adam_eps));
    if (k == 0) {                                                // threads 0..15 of wave 0
        float reg = m;
#pragma unroll
        for (int off = kPix / 2; off > 0; off >>= 1) reg += __shfl_xor(reg, off, kPix);
        if (px == 0) reg_partial[blockIdx.x] = reg;
    }
}

// One wave, after nc_update_kernel in stream order: the statistics row of the step from the logits of rows < n (index
// order per lane, then a butterfly: a fixed order) and the workgroups' mask sums, then the cursor and Adam's step count.
__global__ __launch_bounds__(64) void nc_tail_kernel(const float *__restrict__ logits, int n, int classes, int target,
                                                     const float *__restrict__ reg_partial, int blocks,
                                                     int32_t *__restrict__ cursor, int32_t *__restrict__ t_cell, int steps,
                                                     float *__restrict__ stats) {
    const int cur = *cursor;
    if (cur < 0 || cur >= steps) return;
    float ce = 0.0f, reg = 0.0f;
    int hit = 0;
    for (int i = threadIdx.x; i < n; i += 64) {
        const float *row = logits + (long)i * classes;
        float mx = row[0];
        int arg = 0;
        for (int j = 1; j < classes; ++j)
            if (row[j] > mx) {                                   // the first maximal class: torch.argmax
                mx = row[j];
                arg = j;
            }
        float se = 0.0f;
        for (int j = 0; j < classes; ++j) se += expf(row[j] - mx);
        ce += mx + logf(se) - row[target];
        hit += arg == target;
    }
    for (int b = threadIdx.x; b < blocks; b += 64) reg += reg_partial[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ce += __shfl_xor(ce, off, 64);
        reg += __shfl_xor(reg, off, 64);
        hit += __shfl_xor(hit, off, 64);
    }
    if (threadIdx.x == 0) {
        float *row = stats + (long)cur * 4;
        row[0] = ce / (float)n;
        row[1] = (float)hit;
        row[2] = reg;
        row[3] = (float)n;
        *cursor = cur + 1;
        *t_cell = *t_cell + 1;
    }
}

bool bad_shape(int32_t n_data, int32_t n_index, int32_t bs, int32_t n, int32_t N, int32_t hw) {
    if (hw != 32 && hw != 64 && hw != 224) return true;
    return n_data < 0 || n_index < 0 || bs < 1 || n < 0 || N < 1 || n > N;
}

bool misaligned(const void *p, uintptr_t a) { return !p || ((uintptr_t)p & (a - 1)); }

}  // namespace

extern "C" int combat_nc_blend(const void *dataset, int32_t n_data, const int32_t *index, int32_t n_index,
                               const int32_t *cursor, int32_t bs, int32_t n, int32_t N, int32_t hw, const float *mask_tanh,
                               const float *pattern_tanh, float epsilon, const float *norm, void *out_c8, void *stream) {
    COMBAT_PLAN_HOOK(combat_nc_blend, dataset, n_data, index, n_index, cursor, bs, n, N, hw, mask_tanh, pattern_tanh, epsilon,
                     norm, out_c8);
    if (bad_shape(n_data, n_index, bs, n, N, hw)) return COMBAT_EINVAL;
    if (misaligned(dataset, 4) || misaligned(index, 4) || misaligned(cursor, 4) || misaligned(norm, 4)) return COMBAT_EINVAL;
    if (misaligned(mask_tanh, 16) || misaligned(pattern_tanh, 16) || misaligned(out_c8, 16)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    const int tiles_per_image = (hw * hw + kTilePixels - 1) / kTilePixels;
    const long tiles = (long)N * tiles_per_image;
    const int grid = (int)(tiles < 8192 ? tiles : 8192);
    COMBAT_LAUNCH(nc_blend_kernel, dim3(grid), dim3(256), 0, as_stream(stream), static_cast<const uint8_t *>(dataset), n_data,
                  index, n_index, cursor, bs, n, hw, mask_tanh, pattern_tanh, 2.0f + epsilon, norm, tiles, tiles_per_image,
                  static_cast<uint4 *>(out_c8));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_nc_update(const void *g_img, const void *dataset, int32_t n_data, const int32_t *index, int32_t n_index,
                                int32_t *cursor, int32_t bs, int32_t n, int32_t N, int32_t hw, const float *logits,
                                int32_t classes, int32_t target_label, float *mask_tanh, float *pattern_tanh, float *exp_avg,
                                float *exp_avg_sq, float epsilon, const float *norm, float lr, float beta1, float beta2,
                                float adam_eps, int32_t *t, const float *cost, float *stats, int32_t steps, float *grad_out,
                                void *stream) {
    COMBAT_PLAN_HOOK(combat_nc_update, g_img, dataset, n_data, index, n_index, cursor, bs, n, N, hw, logits, classes,
                     target_label, mask_tanh, pattern_tanh, exp_avg, exp_avg_sq, epsilon, norm, lr, beta1, beta2, adam_eps, t,
                     cost, stats, steps, grad_out);
    if (bad_shape(n_data, n_index, bs, n, N, hw)) return COMBAT_EINVAL;
    if (classes < 1 || classes > kMaxClasses || target_label < 0 || target_label >= classes || steps < 1) return COMBAT_EINVAL;
    if (misaligned(dataset, 4) || misaligned(index, 4) || misaligned(cursor, 4) || misaligned(norm, 4) || misaligned(logits, 4) ||
        misaligned(t, 4) || misaligned(cost, 4) || misaligned(stats, 4))
        return COMBAT_EINVAL;
    if (misaligned(g_img, 16) || misaligned(mask_tanh, 16) || misaligned(pattern_tanh, 16) || misaligned(exp_avg, 16) ||
        misaligned(exp_avg_sq, 16))
        return COMBAT_EINVAL;
    if (grad_out && ((uintptr_t)grad_out & 3)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    const int blocks = hw * hw / kPix;
    float *reg_partial = combat_stream_scratch(stream, (size_t)blocks * sizeof(float));
    if (!reg_partial) return COMBAT_ELAUNCH;
    hipStream_t st = as_stream(stream);
    COMBAT_LAUNCH(nc_update_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint4 *>(g_img),
                  static_cast<const uint8_t *>(dataset), n_data, index, n_index, (const int32_t *)cursor, bs, n, hw, mask_tanh,
                  pattern_tanh, exp_avg, exp_avg_sq, 2.0f + epsilon, norm, lr, beta1, beta2, adam_eps, (const int32_t *)t, cost,
                  steps, grad_out, reg_partial);
    CB_LAUNCH_CHECK();
    COMBAT_LAUNCH(nc_tail_kernel, dim3(1), dim3(64), 0, st, logits, n, classes, target_label, (const float *)reg_partial, blocks,
                  cursor, t, steps, stats);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}
