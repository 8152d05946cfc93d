// Fine-pruning defense (defenses/fine_pruning/fine-pruning.py): the whole accuracy-under-pruning curve from the
// UNPRUNED network's pooled features, and the per-channel activation sums that give the pruning order.
//
// Replaces: the 512 x (copy.deepcopy + rebuilt layer4[1].conv2 / linear + a full evaluation pass) of
// fine-pruning.py:166-214 by one walk over the pruning order per image (combat_prune_sweep), and the
// torch.cat of every layer4 output + torch.mean(dim=[0, 2, 3]) of :145-161 by a running fp64 column sum of the
// pooled features (combat_feature_colsum).  DESIGN.md section 8 has the equivalence argument.
#include "common.hpp"
#include "plan.hpp"

namespace {

constexpr int kMaxClasses = 16;
constexpr int kImages = 64;    // images per workgroup: one per lane of its single wave
constexpr int kEntries = 64;   // (channel, cell) entries staged per chunk: 64 / 16 / 1 channels for per = 1 / 4 / 49
constexpr int kPitch = kImages + 1;   // entry rows of the staged pooled tile: lane e writes [e][r], lane i reads [e][i]

struct SweepArgs {
    const float *pooled, *W, *b;
    const int32_t *order;
    int n, C, per;
    const int64_t *targets, *targets2;
    int32_t *correct, *correct2;
};

// One wave, one image per lane, CLS logits in registers.  The pruning order is walked from its END (the channel pruned
// last) to its start in chunks of T = kEntries / per channels: the chunk's columns of W (permuted by `order`) and of the
// 64 pooled rows go to LDS first -- lane e fetches entry e of every image, so a load instruction touches one 2-KB row
// instead of 64 -- and are fetched into registers one chunk ahead of the arithmetic.  After channel order[k] has been
// added the lane holds the level-k logits: first-maximum argmax, a wave ballot per label set, the popcount into an LDS
// cell, and one integer atomic per level and workgroup at the end of the chunk (integer adds: the same counts whatever
// the order the workgroups arrive in).
template <int CLS>
__global__ __launch_bounds__(kImages) void prune_sweep_kernel(const SweepArgs a) {
    __shared__ float sp[kEntries * kPitch];
    __shared__ float sw[kEntries * CLS];
    __shared__ int cnt[kEntries], cnt2[kEntries];
    const int lane = threadIdx.x;
    const int img0 = blockIdx.x * kImages;
    const int img = img0 + lane;
    const bool valid = img < a.n;
    const int rows = a.n - img0 < kImages ? a.n - img0 : kImages;
    const int in = a.C * a.per;
    const int T = kEntries / a.per;            // channels per chunk (>= 1: per <= 49)
    const int t1 = valid ? (int)a.targets[img] : -1;
    const int t2 = valid && a.targets2 ? (int)a.targets2[img] : -1;
    const bool second = a.targets2 != nullptr;

    float s[CLS];
#pragma unroll
    for (int j = 0; j < CLS; ++j) s[j] = a.b[j];

    float pre[kImages], prew[CLS];
    // entry `lane` of the chunk whose first (highest) level is k_hi: channel order[k_hi - lane / per], cell lane % per
    auto fetch = [&](int k_hi) {
        const int kc = lane / a.per, k = k_hi - kc;
        int f = -1;
        if (kc < T && k >= 0) {
            const int ch = a.order[k];
            if ((unsigned)ch < (unsigned)a.C) f = ch * a.per + (lane - kc * a.per);   // an index outside the network adds nothing
        }
#pragma unroll
        for (int r = 0; r < kImages; ++r) pre[r] = (f >= 0 && r < rows) ? a.pooled[(long)(img0 + r) * in + f] : 0.f;
#pragma unroll
        for (int j = 0; j < CLS; ++j) prew[j] = f >= 0 ? a.W[(long)j * in + f] : 0.f;
    };

    fetch(a.C - 1);
    for (int k_hi = a.C - 1; k_hi >= 0; k_hi -= T) {
        const int tn = k_hi + 1 < T ? k_hi + 1 : T;     // channels in this chunk
        __syncthreads();                                 // the previous chunk's reads and counter flush are done
#pragma unroll
        for (int r = 0; r < kImages; ++r) sp[lane * kPitch + r] = pre[r];
#pragma unroll
        for (int j = 0; j < CLS; ++j) sw[lane * CLS + j] = prew[j];
        __syncthreads();
        if (k_hi - T >= 0) fetch(k_hi - T);              // in flight during the arithmetic below
        for (int kc = 0; kc < tn; ++kc) {
            for (int q = 0; q < a.per; ++q) {
                const int e = kc * a.per + q;
                const float p = sp[e * kPitch + lane];
#pragma unroll
                for (int j = 0; j < CLS; ++j) s[j] = fmaf(p, sw[e * CLS + j], s[j]);
            }
            float mx = s[0];
            int am = 0;
#pragma unroll
            for (int j = 1; j < CLS; ++j)
                if (s[j] > mx) {
                    mx = s[j];
                    am = j;
                }
            const int hits = __popcll(__ballot(valid && am == t1));
            const int hits2 = second ? __popcll(__ballot(valid && am == t2)) : 0;
            if (lane == 0) {
                cnt[kc] = hits;
                cnt2[kc] = hits2;
            }
        }
        __syncthreads();
        if (lane < tn) {
            if (cnt[lane]) atomicAdd(a.correct + (k_hi - lane), cnt[lane]);
            if (second && cnt2[lane]) atomicAdd(a.correct2 + (k_hi - lane), cnt2[lane]);
        }
    }
}

template <int CLS>
void launch_sweep(const SweepArgs &a, hipStream_t st) {
    COMBAT_LAUNCH(prune_sweep_kernel<CLS>, dim3((a.n + kImages - 1) / kImages), dim3(kImages), 0, st, a);
}

// acc[f] += sum_i pooled[i][f]: one thread per feature, the rows in index order, fp64 (adjacent threads read adjacent
// floats of a row)
__global__ __launch_bounds__(256) void feature_colsum_kernel(const float *__restrict__ pooled, int n, int in,
                                                             double *__restrict__ acc) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= in) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)pooled[(long)i * in + f];
    acc[f] += s;
}

}  // namespace

extern "C" int combat_prune_sweep(const float *pooled, int32_t n, const float *W, const float *b, const int32_t *order,
                                  int32_t C, int32_t per, int32_t classes, const int64_t *targets,
                                  const int64_t *targets2, int32_t *correct, int32_t *correct2, void *stream) {
    COMBAT_PLAN_HOOK(combat_prune_sweep, pooled, n, W, b, order, C, per, classes, targets, targets2, correct, correct2);
    if (classes < 1 || classes > kMaxClasses || C < 1 || n < 0) return COMBAT_EINVAL;
    if (per != 1 && per != 4 && per != 49) return COMBAT_EINVAL;
    if ((long)C * per > INT32_MAX) return COMBAT_EINVAL;
    if (!pooled || !W || !b || !order || !targets || !correct) return COMBAT_EINVAL;
    if ((targets2 == nullptr) != (correct2 == nullptr)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    const SweepArgs a{pooled, W, b, order, n, C, per, targets, targets2, correct, correct2};
    hipStream_t st = as_stream(stream);
    switch (classes) {
#define COMBAT_SWEEP_CASE(c) case c: launch_sweep<c>(a, st); break;
        COMBAT_SWEEP_CASE(1) COMBAT_SWEEP_CASE(2) COMBAT_SWEEP_CASE(3) COMBAT_SWEEP_CASE(4)
        COMBAT_SWEEP_CASE(5) COMBAT_SWEEP_CASE(6) COMBAT_SWEEP_CASE(7) COMBAT_SWEEP_CASE(8)
        COMBAT_SWEEP_CASE(9) COMBAT_SWEEP_CASE(10) COMBAT_SWEEP_CASE(11) COMBAT_SWEEP_CASE(12)
        COMBAT_SWEEP_CASE(13) COMBAT_SWEEP_CASE(14) COMBAT_SWEEP_CASE(15) COMBAT_SWEEP_CASE(16)
#undef COMBAT_SWEEP_CASE
    }
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_feature_colsum(const float *pooled, int32_t n, int32_t in, double *acc, void *stream) {
    COMBAT_PLAN_HOOK(combat_feature_colsum, pooled, n, in, acc);
    if (!pooled || !acc || n < 0 || in < 1) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    COMBAT_LAUNCH(feature_colsum_kernel, dim3((in + 255) / 256), dim3(256), 0, as_stream(stream), pooled, n, in, acc);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}
