// Trigger synthesis, on-device augmentation and the detector's DCT input: the image-sized
// (B x 3 x hw x hw) part of the step.  One workgroup per image; everything is staged in LDS as
// fp32 planes and expressed with dense hw x hw matrix products (low-pass P, reflect-padded blur
// Kb, DCT D), which makes every backward the same kernel with transposed factors.
//
//   out = Kb * clamp(x + rate * (P * noise * P^T), -1, 1) * Kb^T
//
// Replaces: low_freq (train_generator.py:47-55 + utils/dct.py:13-111), torch.clamp mix (:192,:225),
// T.GaussianBlur (:165,:194,:226), MSELoss term (:234), PostTensorTransform (utils/dataloader.py:45-60,
// kornia), dct_2d(byte()) (train_generator.py:245).
#include "common.hpp"
#include "plan.hpp"

namespace {

// ---- dense hw x hw fp32 products in LDS, 256 threads.  A thread owns 4 consecutive outputs of one row:
// per k one (broadcast) scalar of the left operand and one float4 of the right operand feed 4 FMAs.
// The left operand has row pitch LP (hw + 1 keeps the 8 rows a wave touches on distinct banks), the
// right operand pitch hw; the output pitch OP is chosen by what the result is used as next.  The
// k-order is ascending with one fma per term, as a plain dot-product loop.
__device__ __forceinline__ void mm4(const float *__restrict__ L, int LP, const float *__restrict__ Rm,
                                    float *__restrict__ O, int OP, int hw, int tid) {
    const int q = hw >> 2;
    for (int o = tid; o < hw * q; o += 256) {
        const int i = o / q, j0 = (o - i * q) << 2;
        f32x4_t s = {0.f, 0.f, 0.f, 0.f};
        const float *lp = L + i * LP;
        for (int k = 0; k < hw; ++k) {
            const float a = lp[k];
            const f32x4_t b = *reinterpret_cast<const f32x4_t *>(Rm + k * hw + j0);
            s[0] = fmaf(a, b[0], s[0]);
            s[1] = fmaf(a, b[1], s[1]);
            s[2] = fmaf(a, b[2], s[2]);
            s[3] = fmaf(a, b[3], s[3]);
        }
        float *op = O + i * OP + j0;
        op[0] = s[0]; op[1] = s[1]; op[2] = s[2]; op[3] = s[3];
    }
}

// entry (i, k) of the reflect-padded 3-tap blur matrix: out[i] = k0*in[r(i-1)] + k1*in[i] + k2*in[r(i+1)]
__device__ __forceinline__ float blur_coef(const float (&kk)[3], int hw, int i, int k) {
    const int im = i > 0 ? i - 1 : 1, ip = i + 1 < hw ? i + 1 : hw - 2;
    float c = 0.f;
    if (k == im) c += kk[0];
    if (k == i) c += kk[1];
    if (k == ip) c += kk[2];
    return c;
}

// Kb * X (ROWS) or X * Kb^T (!ROWS), or with the transposed matrix (TR): three-term stencils evaluated in
// ascending index order, i.e. the dense product's fma chain without its zero terms.
template <bool ROWS, bool TR>
__device__ __forceinline__ void blur_pass(const float *__restrict__ X, float *__restrict__ O, const float (&kk)[3],
                                          int hw, int tid) {
    for (int o = tid; o < hw * hw; o += 256) {
        const int i = o / hw, j = o - i * hw;
        const int t = ROWS ? i : j;            // the blurred index
        float s = 0.f;
        for (int k = t > 0 ? t - 1 : 0; k <= (t + 1 < hw ? t + 1 : hw - 1); ++k) {
            const float c = TR ? blur_coef(kk, hw, k, t) : blur_coef(kk, hw, t, k);
            s = fmaf(c, ROWS ? X[k * hw + j] : X[i * hw + k], s);
        }
        O[o] = s;
    }
}

__device__ __forceinline__ uint4 hilo_px(float r, float g, float b) {
    const float hr = round_bf16(r), hg = round_bf16(g), hb = round_bf16(b);
    uint4 u;
    u.x = pack_bf16x2(hr, hg);
    u.y = pack_bf16x2(hb, r - hr);
    u.z = pack_bf16x2(g - hg, b - hb);
    u.w = 0;
    return u;
}

__device__ __forceinline__ void store_hilo(__bf16 *px8, int c, float v) {   // hi/lo halves of channel c of a c8 pixel
    const float h = round_bf16(v);
    px8[c] = (__bf16)h;
    px8[3 + c] = (__bf16)(v - h);
    if (c == 0) *reinterpret_cast<unsigned int *>(px8 + 6) = 0u;
}

// One workgroup per (channel, image): 3n workgroups.  LDS (floats): Pl [hw][hw+1], Pr [hw][hw], A [hw][hw],
// B [hw][hw+1].  P is symmetric (D^T diag(mask) D), so P N P^T = (P N) P needs no transposed operand.
// The per-(channel, image) body, shared by trigger_fwd_kernel and trigger_pair_fwd_kernel: xi is the image's plane
// of channel c, nz its noise pixels (c8), outp its output plane (the image's row `img` of out_c8 / mse).
// TV (the imperceptible step, train_generator_imperceptible.py:228): the plane's total variation
// sum |out[y+1][x] - out[y][x]| + sum |out[y][x+1] - out[y][x]| -> tv[3 img + c], taken from the blurred plane while it
// is still in LDS (unit-stride reads of the pitch-hw plane A: no bank conflict).  Each thread adds its pixels in index
// order, the 64 lanes of a wave are folded by shuffles and the four wave sums added in wave order: the same bits every
// run.  out and mse are computed by the same instructions with and without TV.
template <bool TV>
__device__ __forceinline__ void trigger_fwd_plane(float *sm, const float *__restrict__ xi, const __bf16 *__restrict__ nz,
                                                  const float *__restrict__ P, const float *__restrict__ k1, float rate,
                                                  int hw, int c, long img, float *__restrict__ outp,
                                                  __bf16 *__restrict__ out_c8, float *__restrict__ mse,
                                                  float *__restrict__ tv) {
    const int hw2 = hw * hw, lp = hw + 1, tid = threadIdx.x;
    float *Pl = sm, *Pr = Pl + hw * lp, *A = Pr + hw2, *B = A + hw2;
    const float kk[3] = {k1[0], k1[1], k1[2]};
    for (int o = tid; o < hw2; o += 256) {
        const float pv = P[o];
        Pr[o] = pv;
        Pl[(o / hw) * lp + (o % hw)] = pv;
        A[o] = (float)nz[(long)o * 8 + c];
    }
    __syncthreads();
    mm4(Pl, lp, A, B, lp, hw, tid);            // B = P N
    __syncthreads();
    mm4(B, lp, Pr, A, hw, hw, tid);            // A = (P N) P
    __syncthreads();
    for (int o = tid; o < hw2; o += 256) A[o] = fminf(fmaxf(fmaf(A[o], rate, xi[o]), -1.f), 1.f);
    __syncthreads();
    blur_pass<true, false>(A, B, kk, hw, tid);   // Kb * bd
    __syncthreads();
    blur_pass<false, false>(B, A, kk, hw, tid);  // ... * Kb^T
    __syncthreads();
    float se = 0.f, tvs = 0.f;
    for (int o = tid; o < hw2; o += 256) {
        const float v = A[o];
        outp[o] = v;
        const float d = v - xi[o];
        se = fmaf(d, d, se);
        if (out_c8) store_hilo(out_c8 + (img * hw2 + o) * 8, c, v);
        if (TV) {
            const int y = o / hw, xx = o - y * hw;
            if (y + 1 < hw) tvs += fabsf(A[o + hw] - v);
            if (xx + 1 < hw) tvs += fabsf(A[o + 1] - v);
        }
    }
    if (mse) {
        __syncthreads();
        B[tid] = se;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) B[tid] += B[tid + s];
            __syncthreads();
        }
        if (tid == 0) mse[img * 3 + c] = B[0];
    }
    if (TV) {
        for (int d = 32; d > 0; d >>= 1) tvs += __shfl_down(tvs, d, 64);
        if ((tid & 63) == 0) Pl[tid >> 6] = tvs;      // Pl: last read by the first product
        __syncthreads();
        if (tid == 0) tv[img * 3 + c] = ((Pl[0] + Pl[1]) + Pl[2]) + Pl[3];
    }
}

__global__ __launch_bounds__(256) void trigger_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                          const float *__restrict__ P, const float *__restrict__ k1,
                                                          float rate, int hw, const int *__restrict__ src_index,
                                                          float *__restrict__ out,
                                                          __bf16 *__restrict__ out_c8, float *__restrict__ mse) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, img = blockIdx.y;
    const long src = src_index ? src_index[img] : img;   // row of x / noise this output image is made from
    trigger_fwd_plane<false>(sm, x + (src * 3 + c) * hw2, noise + src * hw2 * 8, P, k1, rate, hw, c, img,
                             out + ((long)img * 3 + c) * hw2, out_c8, mse, nullptr);
}

// trigger_fwd_kernel + the per-plane total variation of `out` (no src_index / out_c8: Phase G mixes the whole batch).
__global__ __launch_bounds__(256) void trigger_tv_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                             const float *__restrict__ P, const float *__restrict__ k1,
                                                             float rate, int hw, float *__restrict__ out,
                                                             float *__restrict__ mse, float *__restrict__ tv) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, img = blockIdx.y;
    trigger_fwd_plane<true>(sm, x + ((long)img * 3 + c) * hw2, noise + (long)img * hw2 * 8, P, k1, rate, hw, c, img,
                            out + ((long)img * 3 + c) * hw2, nullptr, mse, tv);
}

// The paired trigger of the input-aware step: 2n workgroup rows over ONE batch of images x [n] and the generator's
// output for 2n images.  Row i < n: out_bd[i] = T(x[i], noise[i], k1[0]) with its squared-error partials; row n + i:
// out_cross[i] = T(x[i], noise[n + i], k1[1]) (the noise of another image on x[i]).  Per image the same body as
// trigger_fwd_kernel, so the results are those of two calls of it.
__global__ __launch_bounds__(256) void trigger_pair_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                               const float *__restrict__ P, const float *__restrict__ k1,
                                                               float rate, int n, int hw, float *__restrict__ out_bd,
                                                               float *__restrict__ out_cross, float *__restrict__ mse) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, row = blockIdx.y;
    const int cross = row >= n, img = cross ? row - n : row;
    trigger_fwd_plane<false>(sm, x + ((long)img * 3 + c) * hw2, noise + (long)row * hw2 * 8, P, k1 + 3 * cross, rate, hw,
                             c, img, (cross ? out_cross : out_bd) + ((long)img * 3 + c) * hw2, nullptr,
                             cross ? nullptr : mse, nullptr);
}

// d_noise = rate * P * ( clampmask .* (Kb^T * (d_out + 2*l2*(out-x)) * Kb) ) * P      (P symmetric)
// LDS (floats): Pl, Pr, A, B as above + G [hw][hw]
// The per-(channel, image) body, shared by trigger_bwd_kernel and trigger_pair_bwd_kernel: xi / nz / dn are the
// image's plane of x, noise pixels and gradient pixels (c8); d_out, d_out2, outp point at its plane of channel c.
// TV (train_generator_imperceptible.py:228, :234-237): the gradient of tv_scale * TV(out) joins g before the blur
// adjoint.  d|a - b| = sgn(a - b) with sgn(0) = 0, so pixel (y, x) collects
//   sgn(o[y][x] - o[y-1][x]) - sgn(o[y+1][x] - o[y][x]) + sgn(o[y][x] - o[y][x-1]) - sgn(o[y][x+1] - o[y][x]),
// terms past the border absent.  The out plane is staged in B (free until the first product writes it), so the five
// reads per pixel are unit-stride LDS reads; g without the term is computed by the same instructions as without TV.
__device__ __forceinline__ float sgnf(float d) { return (float)((d > 0.f) - (d < 0.f)); }

template <bool TV>
__device__ __forceinline__ void trigger_bwd_plane(float *sm, const float *__restrict__ xi, const __bf16 *__restrict__ nz,
                                                  const float *__restrict__ P, const float *__restrict__ k1, float rate,
                                                  int hw, int c, const float *__restrict__ d_out,
                                                  const float *__restrict__ d_out2, const float *__restrict__ outp,
                                                  float l2_scale, float tv_scale, int pre_tanh, __bf16 *__restrict__ dn) {
    const int hw2 = hw * hw, lp = hw + 1, tid = threadIdx.x;
    float *Pl = sm, *Pr = Pl + hw * lp, *A = Pr + hw2, *B = A + hw2, *G = B + hw * lp;
    const float kk[3] = {k1[0], k1[1], k1[2]};
    for (int o = tid; o < hw2; o += 256) {
        const float pv = P[o];
        Pr[o] = pv;
        Pl[(o / hw) * lp + (o % hw)] = pv;
        A[o] = (float)nz[(long)o * 8 + c];
        float g = d_out ? d_out[o] : 0.f;
        if (d_out2) g += d_out2[o];      // a second gradient of the same tensor (another classifier's share)
        if (l2_scale != 0.f) g = fmaf(2.f * l2_scale, outp[o] - xi[o], g);
        G[o] = g;
        if (TV) B[o] = outp[o];
    }
    __syncthreads();
    if (TV) {
        for (int o = tid; o < hw2; o += 256) {
            const int y = o / hw, xx = o - y * hw;
            const float v = B[o];
            float s = 0.f;
            if (y > 0) s += sgnf(v - B[o - hw]);
            if (y + 1 < hw) s -= sgnf(B[o + hw] - v);
            if (xx > 0) s += sgnf(v - B[o - 1]);
            if (xx + 1 < hw) s -= sgnf(B[o + 1] - v);
            G[o] = fmaf(tv_scale, s, G[o]);
        }
        __syncthreads();
    }
    mm4(Pl, lp, A, B, lp, hw, tid);
    __syncthreads();
    mm4(B, lp, Pr, A, hw, hw, tid);              // A = P N P  (pre-clamp value is x + rate*A)
    __syncthreads();
    blur_pass<true, true>(G, B, kk, hw, tid);    // B = Kb^T g      (pitch hw: a stencil operand)
    __syncthreads();
    blur_pass<false, true>(B, G, kk, hw, tid);   // G = Kb^T g Kb
    __syncthreads();
    for (int o = tid; o < hw2; o += 256) {
        const float v = fmaf(A[o], rate, xi[o]);
        G[o] = (v >= -1.f && v <= 1.f) ? G[o] * rate : 0.f;
    }
    __syncthreads();
    mm4(Pl, lp, G, B, lp, hw, tid);              // B = P g
    __syncthreads();
    mm4(B, lp, Pr, A, hw, hw, tid);              // A = P g P
    __syncthreads();
    for (int o = tid; o < hw2; o += 256) {
        __bf16 *px = dn + (long)o * 8;
        float r = A[o];
        if (pre_tanh) {  // noise = tanh(z): hand back the gradient w.r.t. z
            const float t = (float)nz[(long)o * 8 + c];
            r *= 1.f - t * t;
        }
        px[c] = (__bf16)r;
        if (c == 0) {   // channels 3..7 of the c8 pixel carry no gradient
            px[3] = (__bf16)0.f;
            *reinterpret_cast<uint2 *>(px + 4) = make_uint2(0u, 0u);
        }
    }
}

__global__ __launch_bounds__(256) void trigger_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                          const float *__restrict__ P, const float *__restrict__ k1,
                                                          float rate, int hw, const float *__restrict__ d_out,
                                                          const float *__restrict__ d_out2,
                                                          const float *__restrict__ outp, float l2_scale,
                                                          int pre_tanh, __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, img = blockIdx.y;
    const long pl = ((long)img * 3 + c) * hw2;
    trigger_bwd_plane<false>(sm, x + pl, noise + (long)img * hw2 * 8, P, k1, rate, hw, c, d_out ? d_out + pl : nullptr,
                             d_out2 ? d_out2 + pl : nullptr, outp ? outp + pl : nullptr, l2_scale, 0.f, pre_tanh,
                             d_noise + (long)img * hw2 * 8);
}

// trigger_bwd_kernel + tv_scale * d TV(out) / d out in the image gradient (outp is required).
__global__ __launch_bounds__(256) void trigger_tv_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                             const float *__restrict__ P, const float *__restrict__ k1,
                                                             float rate, int hw, const float *__restrict__ d_out,
                                                             const float *__restrict__ d_out2,
                                                             const float *__restrict__ outp, float l2_scale,
                                                             float tv_scale, int pre_tanh, __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, img = blockIdx.y;
    const long pl = ((long)img * 3 + c) * hw2;
    trigger_bwd_plane<true>(sm, x + pl, noise + (long)img * hw2 * 8, P, k1, rate, hw, c, d_out ? d_out + pl : nullptr,
                            d_out2 ? d_out2 + pl : nullptr, outp + pl, l2_scale, tv_scale, pre_tanh,
                            d_noise + (long)img * hw2 * 8);
}

// Backward of trigger_pair_fwd_kernel, one launch over 2n workgroup rows.  Row i < n: the gradient of noise[i] from
// d_bd (+ d_bd2) and the L2 term on out_bd, blur k1[0]; row n + i: the gradient of noise[n + i] from d_cross alone
// (no L2 term), blur k1[1].  Per image the same body as trigger_bwd_kernel.
__global__ __launch_bounds__(256) void trigger_pair_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                               const float *__restrict__ P, const float *__restrict__ k1,
                                                               float rate, int n, int hw, const float *__restrict__ d_bd,
                                                               const float *__restrict__ d_bd2,
                                                               const float *__restrict__ out_bd, float l2_scale,
                                                               const float *__restrict__ d_cross, int pre_tanh,
                                                               __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, row = blockIdx.y;
    const int cross = row >= n, img = cross ? row - n : row;
    const long pl = ((long)img * 3 + c) * hw2;
    const float *g1 = cross ? d_cross : d_bd, *g2 = cross ? nullptr : d_bd2;
    trigger_bwd_plane<false>(sm, x + pl, noise + (long)row * hw2 * 8, P, k1 + 3 * cross, rate, hw, c,
                             g1 ? g1 + pl : nullptr, g2 ? g2 + pl : nullptr, cross || !out_bd ? nullptr : out_bd + pl,
                             cross ? 0.f : l2_scale, 0.f, pre_tanh, d_noise + (long)row * hw2 * 8);
}

// The grouped trigger of the multi-label step (train_generator_multilabel.py:203-224): the batch is cut into chunks of
// `ps` images, one target class and one draw of the blur each.  Image i is blurred with k1[i / ps] (the last group may be
// short).  Per image the same body as trigger_fwd_kernel / trigger_bwd_kernel, so the results are those of one call of
// them per chunk.
__global__ __launch_bounds__(256) void trigger_groups_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                 const float *__restrict__ P, const float *__restrict__ k1,
                                                                 float rate, int hw, int ps, float *__restrict__ out,
                                                                 float *__restrict__ mse) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, img = blockIdx.y;
    trigger_fwd_plane<false>(sm, x + ((long)img * 3 + c) * hw2, noise + (long)img * hw2 * 8, P, k1 + 3 * (img / ps), rate, hw,
                             c, img, out + ((long)img * 3 + c) * hw2, nullptr, mse, nullptr);
}

__global__ __launch_bounds__(256) void trigger_groups_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                 const float *__restrict__ P, const float *__restrict__ k1,
                                                                 float rate, int hw, int ps, const float *__restrict__ d_out,
                                                                 const float *__restrict__ d_out2,
                                                                 const float *__restrict__ outp, float l2_scale,
                                                                 int pre_tanh, __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.x, img = blockIdx.y;
    const long pl = ((long)img * 3 + c) * hw2;
    trigger_bwd_plane<false>(sm, x + pl, noise + (long)img * hw2 * 8, P, k1 + 3 * (img / ps), rate, hw, c,
                             d_out ? d_out + pl : nullptr, d_out2 ? d_out2 + pl : nullptr, outp ? outp + pl : nullptr, l2_scale,
                             0.f, pre_tanh, d_noise + (long)img * hw2 * 8);
}

// ------------------------------------------------------------------ planes too large for LDS (64 < hw <= 256: ImageNet-10)
// One workgroup per (16-row strip, channel, image), as dct_u8_big_kernel; thread j owns column j of the strip (hw <= 256
// threads work, all 256 reach the barriers).  No whole plane is ever in LDS: only one [R][hw] strip of an intermediate.
//
// strip_sandwich: m[r] = (P[rows] * W * P)[r][j] for the R rows row0 .. row0 + R - 1 (clamped into the plane: a clamped
// row is a duplicate its caller ignores), where W[k][j] = right(k), asked for k = 0 .. hw - 1 in ascending order.
//   T = P[rows] * W : the row of P is the same for every thread (read straight from global memory, a wave-uniform
//                     load), W's column element comes from `right`; T goes to LDS (Ts, [R][hw])
//   m = T * P       : P symmetric, so column j of P^T is read as P[k][j], unit stride across the threads
// k ascends with one fma per term, as mm4.
template <int R, typename F>
__device__ __forceinline__ void strip_sandwich(float *Ts, const float *__restrict__ P, int hw, int row0, int j, bool on,
                                               F right, float (&m)[R]) {
    const float *prow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) prow[r] = P + (long)min(max(row0 + r, 0), hw - 1) * hw;
#pragma unroll
    for (int r = 0; r < R; ++r) m[r] = 0.f;
#pragma unroll 4
    for (int k = 0; k < hw; ++k) {
        const float w = right(k);
#pragma unroll
        for (int r = 0; r < R; ++r) m[r] = fmaf(prow[r][k], w, m[r]);
    }
    if (on) {
#pragma unroll
        for (int r = 0; r < R; ++r) Ts[r * hw + j] = m[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) m[r] = 0.f;
    for (int k = 0; k < hw; k += 4) {         // hw % 16 == 0
        const float p0 = P[(long)k * hw + j], p1 = P[(long)(k + 1) * hw + j], p2 = P[(long)(k + 2) * hw + j],
                    p3 = P[(long)(k + 3) * hw + j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const f32x4_t t = *reinterpret_cast<const f32x4_t *>(Ts + r * hw + k);
            m[r] = fmaf(t[0], p0, m[r]);
            m[r] = fmaf(t[1], p1, m[r]);
            m[r] = fmaf(t[2], p2, m[r]);
            m[r] = fmaf(t[3], p3, m[r]);
        }
    }
    __syncthreads();      // Ts is free again
}

// What one (strip, channel, output row) of the strip kernels works on.  The plain, paired and grouped kernels differ only
// in how they fill it from their block index (as the whole-plane wrappers differ around trigger_fwd_plane /
// trigger_bwd_plane), so a paired launch writes the bits of two plain calls and a grouped one the bits of one plain call
// per chunk.  Every field is the same for all threads of a workgroup: the pointers stay in scalar registers and the
// blur coefficients the threads derive from k1 stay loop-invariant.
struct StripRow {
    const float *xi;             // channel c's plane of the image of x this row is made from
    const __bf16 *nz;            // this row's noise pixels (c8)
    const float *k1;             // its blur triple
    float *out;                  // forward: channel c's plane of its output image
    __bf16 *out_c8;              // forward: its output pixels as hi/lo c8 (may be null)
    const float *g1, *g2;        // backward: channel c's planes of its gradients (either may be null)
    const float *op;             // backward: channel c's plane of its output, null without the L2 term
    float l2_scale;
    const float *tvo;            // backward with the total-variation term: channel c's plane of its output (the stencil's)
    float tv_scale;
    unsigned short *mask;        // backward: its clamp-mask plane in the scratch, [hw / 16][hw]
    __bf16 *dn;                  // backward: its gradient pixels (c8)
};

// Forward.  The blur crosses the strip's seams, so the strip computes the clamp-mix for its 16 rows and one halo row on
// either side (rows r0 - 1 .. r0 + 16: 18/16 of the products; past the plane's edge the blur reflects onto rows the strip
// holds anyway).  The rows' blur (Kb * bd) stays in the thread's registers -- it only combines values of one column --
// and the columns' blur (* Kb^T) goes through LDS.  LDS: Ts [18][hw] floats.
__device__ __forceinline__ void trigger_big_fwd_strip(float *sm, const float *__restrict__ P, float rate, int hw, int r0, int c,
                                                      const StripRow &w) {
    const int tid = threadIdx.x;
    const bool on = tid < hw;
    const int j = on ? tid : hw - 1;
    const float *xi = w.xi;
    const __bf16 *nz = w.nz + c;
    const float kk[3] = {w.k1[0], w.k1[1], w.k1[2]};
    float m[18];
    strip_sandwich<18>(sm, P, hw, r0 - 1, j, on, [&](int k) { return (float)nz[((long)k * hw + j) * 8]; }, m);
#pragma unroll
    for (int r = 0; r < 18; ++r) {
        const int row = min(max(r0 - 1 + r, 0), hw - 1);
        m[r] = fminf(fmaxf(fmaf(m[r], rate, xi[row * hw + j]), -1.f), 1.f);
    }
    if (on) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {          // Kb * bd, row i = r0 + r: rows i - 1, i, i + 1 are m[r], m[r + 1], m[r + 2]
            const int i = r0 + r;
            float s = 0.f;
            if (i > 0) s = fmaf(blur_coef(kk, hw, i, i - 1), m[r], s);
            s = fmaf(blur_coef(kk, hw, i, i), m[r + 1], s);
            if (i + 1 < hw) s = fmaf(blur_coef(kk, hw, i, i + 1), m[r + 2], s);
            sm[r * hw + j] = s;
        }
    }
    __syncthreads();
    if (on) {
        const float cm = j > 0 ? blur_coef(kk, hw, j, j - 1) : 0.f, c0 = blur_coef(kk, hw, j, j),
                    cp = j + 1 < hw ? blur_coef(kk, hw, j, j + 1) : 0.f;
        const int jm = j > 0 ? j - 1 : j, jp = j + 1 < hw ? j + 1 : j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {          // ... * Kb^T
            const float *row = sm + r * hw;
            float s = 0.f;
            if (j > 0) s = fmaf(cm, row[jm], s);
            s = fmaf(c0, row[j], s);
            if (j + 1 < hw) s = fmaf(cp, row[jp], s);
            const long o = (long)(r0 + r) * hw + j;
            w.out[o] = s;
            if (w.out_c8) store_hilo(w.out_c8 + o * 8, c, s);
        }
    }
}

__global__ __launch_bounds__(256) void trigger_big_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                              const float *__restrict__ P, const float *__restrict__ k1,
                                                              float rate, int hw, const int *__restrict__ src_index,
                                                              float *__restrict__ out, __bf16 *__restrict__ out_c8) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, img = blockIdx.z;
    const long src = src_index ? src_index[img] : img;      // row of x / noise this output image is made from
    StripRow w = {};
    w.xi = x + (src * 3 + c) * hw2;
    w.nz = noise + src * hw2 * 8;
    w.k1 = k1;
    w.out = out + ((long)img * 3 + c) * hw2;
    w.out_c8 = out_c8 ? out_c8 + (long)img * hw2 * 8 : nullptr;
    trigger_big_fwd_strip(sm, P, rate, hw, blockIdx.x * 16, c, w);
}

// The paired trigger (trigger_pair_fwd_kernel) on strips: grid z = 2n rows, row i < n -> out_bd[i] with k1[0], row n + i
// -> out_cross[i] = T(x[i], noise[n + i], k1[1]).  The squared-error partials of the first half come from
// trigger_big_mse_kernel over out_bd.
__global__ __launch_bounds__(256) void trigger_big_pair_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                   const float *__restrict__ P, const float *__restrict__ k1,
                                                                   float rate, int n, int hw, float *__restrict__ out_bd,
                                                                   float *__restrict__ out_cross) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, row = blockIdx.z;
    const int cross = row >= n, img = cross ? row - n : row;
    StripRow w = {};
    w.xi = x + ((long)img * 3 + c) * hw2;
    w.nz = noise + (long)row * hw2 * 8;
    w.k1 = k1 + 3 * cross;
    w.out = (cross ? out_cross : out_bd) + ((long)img * 3 + c) * hw2;
    trigger_big_fwd_strip(sm, P, rate, hw, blockIdx.x * 16, c, w);
}

// The grouped trigger (trigger_groups_fwd_kernel) on strips: image i is blurred with k1[i / ps].
__global__ __launch_bounds__(256) void trigger_big_groups_fwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                     const float *__restrict__ P, const float *__restrict__ k1,
                                                                     float rate, int hw, int ps, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, img = blockIdx.z;
    StripRow w = {};
    w.xi = x + ((long)img * 3 + c) * hw2;
    w.nz = noise + (long)img * hw2 * 8;
    w.k1 = k1 + 3 * (img / ps);
    w.out = out + ((long)img * 3 + c) * hw2;
    trigger_big_fwd_strip(sm, P, rate, hw, blockIdx.x * 16, c, w);
}

// mse[3 img + c] = sum (out - x)^2 over the plane, a launch of its own behind trigger_big_fwd_kernel: one workgroup of
// 1024 threads per plane, so the strips' shares meet in a fixed order (each thread adds its pixels in index order -- the
// loads of seven of them in flight at a time --, the 64 lanes of a wave are folded by shuffles, the sixteen wave sums
// added in wave order): the same bits on every run.
__global__ __launch_bounds__(1024) void trigger_big_mse_kernel(const float *__restrict__ x, const float *__restrict__ out, int hw,
                                                               const int *__restrict__ src_index, float *__restrict__ mse) {
    __shared__ float ws[16];
    const int hw2 = hw * hw, tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    const long src = src_index ? src_index[img] : img;
    const float *xi = x + (src * 3 + c) * hw2, *oi = out + ((long)img * 3 + c) * hw2;
    float se = 0.f;
#pragma unroll 7
    for (int o = tid; o < hw2; o += 1024) {
        const float d = oi[o] - xi[o];
        se = fmaf(d, d, se);
    }
    for (int d = 32; d > 0; d >>= 1) se += __shfl_down(se, d, 64);
    if ((tid & 63) == 0) ws[tid >> 6] = se;
    __syncthreads();
    if (tid == 0) {
        float t = ws[0];
        for (int w = 1; w < 16; ++w) t += ws[w];
        mse[img * 3 + c] = t;
    }
}

// The imperceptible step's reduction behind trigger_big_fwd_kernel (train_generator_imperceptible.py:228): the plane's
// total variation tv[3 img + c] = sum |out[y+1][x] - out[y][x]| + sum |out[y][x+1] - out[y][x]|, and with `mse` the squared
// error of trigger_big_mse_kernel -- the same subtraction and fma per pixel, the same order, so the same bits.  The TV
// sum is ordered likewise: a thread adds its pixels in index order (vertical term, then horizontal term), the lanes are
// folded by shuffles, the sixteen wave sums added in wave order.  The neighbours are read from global memory: a strip
// kernel never holds the row below its last one.  Neither neighbour leaves the plane (y + 1 < hw, x + 1 < hw).
__global__ __launch_bounds__(1024) void trigger_big_tv_kernel(const float *__restrict__ x, const float *__restrict__ out, int hw,
                                                              float *__restrict__ mse, float *__restrict__ tv) {
    __shared__ float ws[16], wt[16];
    const int hw2 = hw * hw, tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    const float *xi = x + ((long)img * 3 + c) * hw2, *oi = out + ((long)img * 3 + c) * hw2;
    float se = 0.f, tvs = 0.f;
#pragma unroll 7
    for (int o = tid; o < hw2; o += 1024) {
        const float v = oi[o];
        const float d = v - xi[o];
        se = fmaf(d, d, se);
        const int y = o / hw, xx = o - y * hw;
        if (y + 1 < hw) tvs += fabsf(oi[o + hw] - v);
        if (xx + 1 < hw) tvs += fabsf(oi[o + 1] - v);
    }
    for (int d = 32; d > 0; d >>= 1) {
        se += __shfl_down(se, d, 64);
        tvs += __shfl_down(tvs, d, 64);
    }
    if ((tid & 63) == 0) {
        ws[tid >> 6] = se;
        wt[tid >> 6] = tvs;
    }
    __syncthreads();
    if (tid == 0) {
        float t = ws[0], u = wt[0];
        for (int w = 1; w < 16; ++w) {
            t += ws[w];
            u += wt[w];
        }
        if (mse) mse[img * 3 + c] = t;
        tv[img * 3 + c] = u;
    }
}

// Backward, first launch: the clamp mask.  P * noise * P is recomputed (as trigger_bwd_kernel does), strip by strip, and
// only whether x + rate * (...) lies inside [-1, 1] is kept: bit r of mask[((3 row + c) * hw / 16 + strip) * hw + j] is
// pixel (16 strip + r, j) of the launch's row `row` (grid z).  hw^2 / 8 bytes per plane.  LDS: Ts [16][hw].
__device__ __forceinline__ void trigger_big_mask_strip(float *sm, const float *__restrict__ P, float rate, int hw, int strip,
                                                       int c, const StripRow &w) {
    const int tid = threadIdx.x, r0 = strip * 16;
    const bool on = tid < hw;
    const int j = on ? tid : hw - 1;
    const float *xi = w.xi;
    const __bf16 *nz = w.nz + c;
    float m[16];
    strip_sandwich<16>(sm, P, hw, r0, j, on, [&](int k) { return (float)nz[((long)k * hw + j) * 8]; }, m);
    unsigned bits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = fmaf(m[r], rate, xi[(r0 + r) * hw + j]);
        bits |= (v >= -1.f && v <= 1.f ? 1u : 0u) << r;
    }
    if (on) w.mask[(long)strip * hw + j] = (unsigned short)bits;
}

__global__ __launch_bounds__(256) void trigger_big_mask_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                               const float *__restrict__ P, float rate, int hw,
                                                               unsigned short *__restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, img = blockIdx.z;
    StripRow w = {};
    w.xi = x + ((long)img * 3 + c) * hw2;
    w.nz = noise + (long)img * hw2 * 8;
    w.mask = mask + ((long)img * 3 + c) * (hw >> 4) * hw;
    trigger_big_mask_strip(sm, P, rate, hw, blockIdx.x, c, w);
}

// The mask of rows row0 .. row0 + gridDim.z - 1 of the paired trigger's 2n rows: one run of the launcher.  x and noise
// are the call's own pointers, because a run may begin in the first half and end in the cross half: x is indexed by
// row mod n, the noise by row, the mask plane by the row's place in the run.
__global__ __launch_bounds__(256) void trigger_big_pair_mask_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                    const float *__restrict__ P, float rate, int n, int row0,
                                                                    int hw, unsigned short *__restrict__ mask) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, row = row0 + blockIdx.z;
    const int img = row >= n ? row - n : row;
    StripRow w = {};
    w.xi = x + ((long)img * 3 + c) * hw2;
    w.nz = noise + (long)row * hw2 * 8;
    w.mask = mask + ((long)blockIdx.z * 3 + c) * (hw >> 4) * hw;
    trigger_big_mask_strip(sm, P, rate, hw, blockIdx.x, c, w);
}

// Backward, second launch: d_noise[strip] = P[strip] * W * P with W = rate * mask .* (Kb^T g Kb), g = d_out + d_out2 +
// 2 l2 (out - x).  W is never stored: thread j walks down column j and forms W[k][j] from the mask bit and the 3 x 3
// blur adjoint of g, whose three row terms (g Kb)[k - 1 .. k + 1][j] slide along in registers (one new row of three
// pixels per k).  LDS: Ts [16][hw].
// TV (the imperceptible step, train_generator_imperceptible.py:228, :234-237): g gains tv_scale * the sign stencil of
// trigger_bwd_plane<true>, in its order and with its sgnf.  The stencil's neighbours of `out` (w.tvo) come from global
// memory: out is complete before the backward starts, so they cross the strips' seams freely; the guards on the row a and
// the column b keep them inside the plane.  Without TV the body is the one it was.
template <bool TV>
__device__ __forceinline__ void trigger_big_bwd_strip(float *sm, const float *__restrict__ P, float rate, int hw, int r0, int c,
                                                      int pre_tanh, const StripRow &w) {
    const int tid = threadIdx.x;
    const bool on = tid < hw;
    const int j = on ? tid : hw - 1;
    const float *xi = w.xi, *g1 = w.g1, *g2 = w.g2, *op = w.op;
    const float l2_scale = w.l2_scale;
    const unsigned short *mk = w.mask + j;
    const float kk[3] = {w.k1[0], w.k1[1], w.k1[2]};
    // (g Kb)[a][j] = sum_b g[a][b] Kb[b][j], b = j - 1 .. j + 1 inside the plane, ascending
    const int jm = j > 0 ? j - 1 : j, jp = j + 1 < hw ? j + 1 : j;
    const float cm = j > 0 ? blur_coef(kk, hw, j - 1, j) : 0.f, c0 = blur_coef(kk, hw, j, j),
                cp = j + 1 < hw ? blur_coef(kk, hw, j + 1, j) : 0.f;
    const float *tvo = w.tvo;
    const float tv_scale = w.tv_scale;
    auto g_at = [&](int a, int b) {
        const int o = a * hw + b;
        float g = g1 ? g1[o] : 0.f;
        if (g2) g += g2[o];
        if (op) g = fmaf(2.f * l2_scale, op[o] - xi[o], g);
        if (TV) {
            const float v = tvo[o];
            float s = 0.f;
            if (a > 0) s += sgnf(v - tvo[o - hw]);
            if (a + 1 < hw) s -= sgnf(tvo[o + hw] - v);
            if (b > 0) s += sgnf(v - tvo[o - 1]);
            if (b + 1 < hw) s -= sgnf(tvo[o + 1] - v);
            g = fmaf(tv_scale, s, g);
        }
        return g;
    };
    auto h_row = [&](int a) {
        float s = 0.f;
        if (j > 0) s = fmaf(cm, g_at(a, jm), s);
        s = fmaf(c0, g_at(a, j), s);
        if (j + 1 < hw) s = fmaf(cp, g_at(a, jp), s);
        return s;
    };
    float hm = 0.f, h0 = h_row(0), hp = h_row(1);
    unsigned bits = 0;
    float m[16];
    strip_sandwich<16>(sm, P, hw, r0, j, on,
                       [&](int k) {
                           if ((k & 15) == 0) bits = mk[(long)(k >> 4) * hw];
                           float s = 0.f;        // (Kb^T h)[k][j] = sum_a Kb[a][k] h[a][j], a = k - 1 .. k + 1, ascending
                           if (k > 0) s = fmaf(blur_coef(kk, hw, k - 1, k), hm, s);
                           s = fmaf(blur_coef(kk, hw, k, k), h0, s);
                           if (k + 1 < hw) s = fmaf(blur_coef(kk, hw, k + 1, k), hp, s);
                           const float wv = (bits >> (k & 15)) & 1u ? s * rate : 0.f;
                           hm = h0;
                           h0 = hp;
                           hp = k + 2 < hw ? h_row(k + 2) : 0.f;
                           return wv;
                       },
                       m);
    if (on) {
        const __bf16 *nz = w.nz;
        __bf16 *dn = w.dn;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long o = (long)(r0 + r) * hw + j;
            __bf16 *px = dn + o * 8;
            float v = m[r];
            if (pre_tanh) {  // noise = tanh(z): hand back the gradient w.r.t. z
                const float t = (float)nz[o * 8 + c];
                v *= 1.f - t * t;
            }
            px[c] = (__bf16)v;
            if (c == 0) {   // channels 3..7 of the c8 pixel carry no gradient
                px[3] = (__bf16)0.f;
                *reinterpret_cast<uint2 *>(px + 4) = make_uint2(0u, 0u);
            }
        }
    }
}

__global__ __launch_bounds__(256) void trigger_big_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                              const float *__restrict__ P, const float *__restrict__ k1,
                                                              float rate, int hw, const float *__restrict__ d_out,
                                                              const float *__restrict__ d_out2,
                                                              const float *__restrict__ outp, float l2_scale, int pre_tanh,
                                                              const unsigned short *__restrict__ mask,
                                                              __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, img = blockIdx.z;
    const long pl = ((long)img * 3 + c) * hw2;
    StripRow w = {};
    w.xi = x + pl;
    w.nz = noise + (long)img * hw2 * 8;
    w.k1 = k1;
    w.g1 = d_out ? d_out + pl : nullptr;
    w.g2 = d_out2 ? d_out2 + pl : nullptr;
    w.op = l2_scale != 0.f ? outp + pl : nullptr;
    w.l2_scale = l2_scale;
    w.mask = const_cast<unsigned short *>(mask) + ((long)img * 3 + c) * (hw >> 4) * hw;
    w.dn = d_noise + (long)img * hw2 * 8;
    trigger_big_bwd_strip<false>(sm, P, rate, hw, blockIdx.x * 16, c, pre_tanh, w);
}

// trigger_big_bwd_kernel + tv_scale * d TV(out) / d out in the image gradient (trigger_tv_bwd_kernel on strips; outp is
// required, whatever l2_scale is).
__global__ __launch_bounds__(256) void trigger_big_tv_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                 const float *__restrict__ P, const float *__restrict__ k1,
                                                                 float rate, int hw, const float *__restrict__ d_out,
                                                                 const float *__restrict__ d_out2,
                                                                 const float *__restrict__ outp, float l2_scale,
                                                                 float tv_scale, int pre_tanh,
                                                                 const unsigned short *__restrict__ mask,
                                                                 __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, img = blockIdx.z;
    const long pl = ((long)img * 3 + c) * hw2;
    StripRow w = {};
    w.xi = x + pl;
    w.nz = noise + (long)img * hw2 * 8;
    w.k1 = k1;
    w.g1 = d_out ? d_out + pl : nullptr;
    w.g2 = d_out2 ? d_out2 + pl : nullptr;
    w.op = l2_scale != 0.f ? outp + pl : nullptr;
    w.l2_scale = l2_scale;
    w.tvo = outp + pl;
    w.tv_scale = tv_scale;
    w.mask = const_cast<unsigned short *>(mask) + ((long)img * 3 + c) * (hw >> 4) * hw;
    w.dn = d_noise + (long)img * hw2 * 8;
    trigger_big_bwd_strip<true>(sm, P, rate, hw, blockIdx.x * 16, c, pre_tanh, w);
}

// Rows row0 .. row0 + gridDim.z - 1 of the paired backward (trigger_pair_bwd_kernel on strips), behind
// trigger_big_pair_mask_kernel over the same rows.  Row i < n: d_bd (+ d_bd2) and the L2 term on out_bd, blur k1[0];
// row n + i: d_cross alone, blur k1[1].
__global__ __launch_bounds__(256) void trigger_big_pair_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                   const float *__restrict__ P, const float *__restrict__ k1,
                                                                   float rate, int n, int row0, int hw,
                                                                   const float *__restrict__ d_bd, const float *__restrict__ d_bd2,
                                                                   const float *__restrict__ out_bd, float l2_scale,
                                                                   const float *__restrict__ d_cross, int pre_tanh,
                                                                   const unsigned short *__restrict__ mask,
                                                                   __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, row = row0 + blockIdx.z;
    const int cross = row >= n, img = cross ? row - n : row;
    const long pl = ((long)img * 3 + c) * hw2;
    const float *g1 = cross ? d_cross : d_bd, *g2 = cross ? nullptr : d_bd2;
    StripRow w = {};
    w.xi = x + pl;
    w.nz = noise + (long)row * hw2 * 8;
    w.k1 = k1 + 3 * cross;
    w.g1 = g1 ? g1 + pl : nullptr;
    w.g2 = g2 ? g2 + pl : nullptr;
    w.l2_scale = cross ? 0.f : l2_scale;
    w.op = w.l2_scale != 0.f ? out_bd + pl : nullptr;
    w.mask = const_cast<unsigned short *>(mask) + ((long)blockIdx.z * 3 + c) * (hw >> 4) * hw;
    w.dn = d_noise + (long)row * hw2 * 8;
    trigger_big_bwd_strip<false>(sm, P, rate, hw, blockIdx.x * 16, c, pre_tanh, w);
}

// Images img0 .. img0 + gridDim.z - 1 of the grouped backward (trigger_groups_bwd_kernel on strips), behind
// trigger_big_mask_kernel over the same images: image i is blurred with k1[i / ps], i counted over the whole call.
__global__ __launch_bounds__(256) void trigger_big_groups_bwd_kernel(const float *__restrict__ x, const __bf16 *__restrict__ noise,
                                                                     const float *__restrict__ P, const float *__restrict__ k1,
                                                                     float rate, int hw, int ps, int img0,
                                                                     const float *__restrict__ d_out,
                                                                     const float *__restrict__ d_out2,
                                                                     const float *__restrict__ outp, float l2_scale,
                                                                     int pre_tanh, const unsigned short *__restrict__ mask,
                                                                     __bf16 *__restrict__ d_noise) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, c = blockIdx.y, img = img0 + blockIdx.z;
    const long pl = ((long)img * 3 + c) * hw2;
    StripRow w = {};
    w.xi = x + pl;
    w.nz = noise + (long)img * hw2 * 8;
    w.k1 = k1 + 3 * (img / ps);
    w.g1 = d_out ? d_out + pl : nullptr;
    w.g2 = d_out2 ? d_out2 + pl : nullptr;
    w.op = l2_scale != 0.f ? outp + pl : nullptr;
    w.l2_scale = l2_scale;
    w.mask = const_cast<unsigned short *>(mask) + ((long)blockIdx.z * 3 + c) * (hw >> 4) * hw;
    w.dn = d_noise + (long)img * hw2 * 8;
    trigger_big_bwd_strip<false>(sm, P, rate, hw, blockIdx.x * 16, c, pre_tanh, w);
}

// ------------------------------------------------------------------ augmentation
struct AugGeom {
    float ca, sa, cx, cy;
    int ox, oy, flip, rot;
};

__device__ __forceinline__ AugGeom aug_geom(const float *params, int img, int hw) {
    AugGeom g;
    g.ox = g.oy = g.flip = g.rot = 0;
    g.ca = 1.f;
    g.sa = 0.f;
    g.cx = g.cy = 0.5f * (hw - 1);
    if (params) {
        const float *q = params + 4 * img;
        g.ox = (int)q[0];
        g.oy = (int)q[1];
        g.rot = q[2] != 0.f;
        g.ca = cosf(q[2]);
        g.sa = sinf(q[2]);
        g.flip = q[3] != 0.f;
    }
    return g;
}

// value of the cropped image Ic(u, v) = I(u + ox, v + oy) inside the hw window, zero outside
__device__ __forceinline__ float crop_at(const float *plane, int hw, const AugGeom &g, int u, int v) {
    if ((unsigned)u >= (unsigned)hw || (unsigned)v >= (unsigned)hw) return 0.f;
    const int sx = u + g.ox, sy = v + g.oy;
    if ((unsigned)sx >= (unsigned)hw || (unsigned)sy >= (unsigned)hw) return 0.f;
    return plane[sy * hw + sx];
}

__global__ __launch_bounds__(256) void augment_fwd_kernel(const float *__restrict__ x, const int *__restrict__ index,
                                                          const float *__restrict__ params, int hw,
                                                          uint4 *__restrict__ out_c8, float *__restrict__ out_f32) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, tid = threadIdx.x, img = blockIdx.x;
    const int srci = index ? index[img] : img;
    for (int o = tid; o < 3 * hw2; o += 256) sm[o] = x[(long)srci * 3 * hw2 + o];
    __syncthreads();
    const AugGeom g = aug_geom(params, img, hw);
    for (int o = tid; o < hw2; o += 256) {
        const int yo = o / hw, xo0 = o - yo * hw;
        const int xo = g.flip ? hw - 1 - xo0 : xo0;  // flip is the last stage
        float v[3];
        if (g.rot) {
            const float dx = xo - g.cx, dy = yo - g.cy;
            const float sx = g.ca * dx - g.sa * dy + g.cx, sy = g.sa * dx + g.ca * dy + g.cy;
            const float fx = floorf(sx), fy = floorf(sy);
            const int x0 = (int)fx, y0 = (int)fy;
            const float ax = sx - fx, ay = sy - fy;
            for (int c = 0; c < 3; ++c) {
                const float *pl = sm + c * hw2;
                v[c] = (1.f - ay) * ((1.f - ax) * crop_at(pl, hw, g, x0, y0) + ax * crop_at(pl, hw, g, x0 + 1, y0)) +
                       ay * ((1.f - ax) * crop_at(pl, hw, g, x0, y0 + 1) + ax * crop_at(pl, hw, g, x0 + 1, y0 + 1));
            }
        } else {
            for (int c = 0; c < 3; ++c) v[c] = crop_at(sm + c * hw2, hw, g, xo, yo);
        }
        out_c8[(long)img * hw2 + o] = hilo_px(v[0], v[1], v[2]);
        if (out_f32)
            for (int c = 0; c < 3; ++c) out_f32[((long)img * 3 + c) * hw2 + o] = v[c];
    }
}

// Images too large for one workgroup's LDS (hw > 96: ImageNet-10's 224 x 224): the same geometry, one thread per
// output pixel, gathering from global memory.
__global__ __launch_bounds__(256) void augment_fwd_big_kernel(const float *__restrict__ x, const int *__restrict__ index,
                                                              const float *__restrict__ params, int hw,
                                                              uint4 *__restrict__ out_c8, float *__restrict__ out_f32) {
    const int hw2 = hw * hw, img = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
    if (o >= hw2) return;
    const float *src = x + (long)(index ? index[img] : img) * 3 * hw2;
    const AugGeom g = aug_geom(params, img, hw);
    const int yo = o / hw, xo0 = o - yo * hw;
    const int xo = g.flip ? hw - 1 - xo0 : xo0;
    float v[3];
    if (g.rot) {
        const float dx = xo - g.cx, dy = yo - g.cy;
        const float sx = g.ca * dx - g.sa * dy + g.cx, sy = g.sa * dx + g.ca * dy + g.cy;
        const float fx = floorf(sx), fy = floorf(sy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float ax = sx - fx, ay = sy - fy;
        for (int c = 0; c < 3; ++c) {
            const float *pl = src + c * hw2;
            v[c] = (1.f - ay) * ((1.f - ax) * crop_at(pl, hw, g, x0, y0) + ax * crop_at(pl, hw, g, x0 + 1, y0)) +
                   ay * ((1.f - ax) * crop_at(pl, hw, g, x0, y0 + 1) + ax * crop_at(pl, hw, g, x0 + 1, y0 + 1));
        }
    } else {
        for (int c = 0; c < 3; ++c) v[c] = crop_at(src + c * hw2, hw, g, xo, yo);
    }
    out_c8[(long)img * hw2 + o] = hilo_px(v[0], v[1], v[2]);
    if (out_f32)
        for (int c = 0; c < 3; ++c) out_f32[((long)img * 3 + c) * hw2 + o] = v[c];
}

__device__ __forceinline__ void crop_scatter(float *plane, int hw, const AugGeom &g, int u, int v, float val) {
    if ((unsigned)u >= (unsigned)hw || (unsigned)v >= (unsigned)hw) return;
    const int sx = u + g.ox, sy = v + g.oy;
    if ((unsigned)sx >= (unsigned)hw || (unsigned)sy >= (unsigned)hw) return;
    atomicAdd(plane + sy * hw + sx, val);  // LDS atomic (global in the big-image variant)
}

// The adjoint as a GATHER: no atomics, a fixed summation order (the scatter form -- every output pixel adding its four
// weighted shares to an LDS image with ds_add_f32 -- cost the same 15 us and summed in whatever order the waves ran:
// the generator's gradient differed in the last bits from run to run).  The gradient image is
// staged in LDS; every source pixel (X, Y) -- crop-space pixel (u, v) = (X - ox, Y - oy) -- visits the output pixels
// whose bilinear footprint can contain (u, v): the rotation maps output pixel o to s = R (o - c) + c and (u, v) is one
// of its four taps iff s lies in [u - 1, u + 1) x [v - 1, v + 1), so o lies within (|cos| + |sin|) <= 1.415 of
// q = R^T ((u, v) - c) + c in either axis: the 6 x 6 window [floor(q) - 2, floor(q) + 3] holds them all with 0.58
// pixels to spare.  Each candidate recomputes s, the tap corner and the weights with the forward kernel's own
// expressions (the same products the scatter adds), and the matches are summed in window order.
__global__ __launch_bounds__(256) void augment_bwd_gather_kernel(const __bf16 *__restrict__ d_c8, int cch,
                                                                 const float *__restrict__ params, int hw,
                                                                 float *__restrict__ d_x, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, tid = threadIdx.x, img = blockIdx.x;
    for (int o = tid; o < hw2; o += 256) {
        const __bf16 *gp = d_c8 + ((long)img * hw2 + o) * cch;
        sm[o] = (float)gp[0], sm[hw2 + o] = (float)gp[1], sm[2 * hw2 + o] = (float)gp[2];
    }
    __syncthreads();
    const AugGeom g = aug_geom(params, img, hw);
    for (int o = tid; o < hw2; o += 256) {
        const int Y = o / hw, X = o - Y * hw;
        const int u = X - g.ox, v = Y - g.oy;
        float acc[3] = {0.f, 0.f, 0.f};
        if ((unsigned)u < (unsigned)hw && (unsigned)v < (unsigned)hw) {
            if (g.rot) {
                const float qx = g.ca * (u - g.cx) + g.sa * (v - g.cy) + g.cx, qy = -g.sa * (u - g.cx) + g.ca * (v - g.cy) + g.cy;
                const int bx = (int)floorf(qx) - 2, by = (int)floorf(qy) - 2;
                for (int jy = 0; jy < 6; ++jy) {
                    const int yo = by + jy;
                    if ((unsigned)yo >= (unsigned)hw) continue;
                    for (int jx = 0; jx < 6; ++jx) {
                        const int xo = bx + jx;
                        if ((unsigned)xo >= (unsigned)hw) continue;
                        const float dx = xo - g.cx, dy = yo - g.cy;
                        const float sx = g.ca * dx - g.sa * dy + g.cx, sy = g.sa * dx + g.ca * dy + g.cy;
                        const float fx = floorf(sx), fy = floorf(sy);
                        const int x0 = (int)fx, y0 = (int)fy;
                        if ((u != x0 && u != x0 + 1) || (v != y0 && v != y0 + 1)) continue;
                        const float ax = sx - fx, ay = sy - fy;
                        const float w = (v == y0 ? 1.f - ay : ay) * (u == x0 ? 1.f - ax : ax);
                        const int m = yo * hw + (g.flip ? hw - 1 - xo : xo);
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[c] += w * sm[c * hw2 + m];
                    }
                }
            } else {
                const int m = v * hw + (g.flip ? hw - 1 - u : u);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = sm[c * hw2 + m];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *d = d_x + ((long)img * 3 + c) * hw2 + o;
            *d = accumulate ? *d + acc[c] : acc[c];
        }
    }
}

// hw > 96: scatter with global fp32 atomics into d_x (zeroed by the launcher unless `accumulate`)
__global__ __launch_bounds__(256) void augment_bwd_big_kernel(const __bf16 *__restrict__ d_c8, int cch,
                                                              const float *__restrict__ params, int hw,
                                                              float *__restrict__ d_x) {
    const int hw2 = hw * hw, img = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
    if (o >= hw2) return;
    const AugGeom g = aug_geom(params, img, hw);
    const int yo = o / hw, xo0 = o - yo * hw;
    const int xo = g.flip ? hw - 1 - xo0 : xo0;
    const __bf16 *gp = d_c8 + ((long)img * hw2 + o) * cch;
    const float gv[3] = {(float)gp[0], (float)gp[1], (float)gp[2]};
    float *dst = d_x + (long)img * 3 * hw2;
    if (g.rot) {
        const float dx = xo - g.cx, dy = yo - g.cy;
        const float sx = g.ca * dx - g.sa * dy + g.cx, sy = g.sa * dx + g.ca * dy + g.cy;
        const float fx = floorf(sx), fy = floorf(sy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float ax = sx - fx, ay = sy - fy;
        for (int c = 0; c < 3; ++c) {
            float *pl = dst + c * hw2;
            crop_scatter(pl, hw, g, x0, y0, (1.f - ay) * (1.f - ax) * gv[c]);
            crop_scatter(pl, hw, g, x0 + 1, y0, (1.f - ay) * ax * gv[c]);
            crop_scatter(pl, hw, g, x0, y0 + 1, ay * (1.f - ax) * gv[c]);
            crop_scatter(pl, hw, g, x0 + 1, y0 + 1, ay * ax * gv[c]);
        }
    } else {
        for (int c = 0; c < 3; ++c) crop_scatter(dst + c * hw2, hw, g, xo, yo, gv[c]);
    }
}

// ------------------------------------------------------------------ DCT of the uint8-truncated image
// one workgroup per (channel, image); LDS (floats): Dl [hw][hw+1] = D, Dr [hw][hw] = D^T, A, B [hw][hw+1]
__global__ __launch_bounds__(256) void dct_u8_kernel(const float *__restrict__ x, const float *__restrict__ D, int hw,
                                                     __bf16 *__restrict__ out_c8) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, lp = hw + 1, tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
    float *Dl = sm, *Dr = Dl + hw * lp, *A = Dr + hw2, *B = A + hw2;
    for (int o = tid; o < hw2; o += 256) {
        const int i = o / hw, j = o - i * hw;
        const float dv = D[o];
        Dl[i * lp + j] = dv;
        Dr[j * hw + i] = dv;
        const float q = (x[((long)img * 3 + c) * hw2 + o] + 1.f) / 2.f * 255.f;
        A[o] = (float)(unsigned char)(int)q;  // .byte(): truncate toward zero, wrap mod 256
    }
    __syncthreads();
    mm4(Dl, lp, A, B, lp, hw, tid);     // B = D q
    __syncthreads();
    mm4(B, lp, Dr, A, hw, hw, tid);     // A = D q D^T
    __syncthreads();
    for (int o = tid; o < hw2; o += 256) store_hilo(out_c8 + ((long)img * hw2 + o) * 8, c, A[o]);
}

// hw > 64 (224): one workgroup per (16-row strip, channel, image).  T = D[strip] q in LDS, then Y[strip] = T D^T.
// LDS: Ds [16][hw] (the strip of D), Ts [16][hw].  Metric only (the detector's accuracy), ~4 GFLOP fp32 per 32 images.
__global__ __launch_bounds__(256) void dct_u8_big_kernel(const float *__restrict__ x, const float *__restrict__ D, int hw,
                                                         __bf16 *__restrict__ out_c8) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hw2 = hw * hw, tid = threadIdx.x, r0 = blockIdx.x * 16, c = blockIdx.y, img = blockIdx.z;
    float *Ds = sm, *Ts = sm + 16 * hw;
    for (int o = tid; o < 16 * hw; o += 256) Ds[o] = D[r0 * hw + o];
    __syncthreads();
    const float *plane = x + ((long)img * 3 + c) * hw2;
    for (int j = tid; j < hw; j += 256) {     // column j of the strip: T[r][j] = sum_k D[r0 + r][k] q[k][j]
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k = 0; k < hw; ++k) {
            const float q = (float)(unsigned char)(int)((plane[k * hw + j] + 1.f) / 2.f * 255.f);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaf(Ds[r * hw + k], q, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Ts[r * hw + j] = acc[r];
    }
    __syncthreads();
    for (int j = tid; j < hw; j += 256) {     // Y[r][j] = sum_k T[r][k] D[j][k]
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float *dj = D + (long)j * hw;
        for (int k = 0; k < hw; ++k) {
            const float d = dj[k];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaf(Ts[r * hw + k], d, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) store_hilo(out_c8 + ((long)img * hw2 + (r0 + r) * hw + j) * 8, c, acc[r]);
    }
}

template <typename K>
int set_smem(K kern, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               bytes) == hipSuccess
               ? COMBAT_OK
               : COMBAT_ELAUNCH;
}

// The strip backwards' clamp mask (3 hw^2 / 8 bytes per image row) in the stream's 2 MB scratch: how many of `rows` rows
// one run takes (all of them, or as many as fit).  mask is null if the scratch could not be had.
struct BigRuns {
    unsigned short *mask;
    int run;
};

BigRuns big_runs(void *stream, int hw, size_t rows) {
    constexpr size_t kScratch = 2u << 20;
    const size_t per_row = 3 * (size_t)hw * hw / 8;
    const int run = (int)(kScratch / per_row < rows ? kScratch / per_row : rows);
    return {reinterpret_cast<unsigned short *>(combat_stream_scratch(stream, (size_t)run * per_row)), run};
}

}  // namespace

extern "C" int combat_trigger_fwd(const float *x, const void *noise, const float *P, const float *k1,
                                  float noise_rate, int32_t n, int32_t hw, const int32_t *src_index, float *out,
                                  void *out_c8, float *mse_partial, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_fwd, x, noise, P, k1, noise_rate, n, hw, src_index, out, out_c8, mse_partial);
    if (!x || !noise || !P || !k1 || !out || n < 0 || hw < 16 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {      // strips: only the last launch of the call may carry a replayed plan's hand-off event
        hipStream_t st = as_stream(stream);
        if (mse_partial) {
            hipLaunchKernelGGL(trigger_big_fwd_kernel, dim3(hw / 16, 3, n), dim3(256), 18 * hw * 4, st, x,
                               reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, src_index, out,
                               reinterpret_cast<__bf16 *>(out_c8));
            CB_LAUNCH_CHECK();
            COMBAT_LAUNCH(trigger_big_mse_kernel, dim3(3, n), dim3(1024), 0, st, x, (const float *)out, hw, src_index, mse_partial);
        } else {
            COMBAT_LAUNCH(trigger_big_fwd_kernel, dim3(hw / 16, 3, n), dim3(256), 18 * hw * 4, st, x,
                          reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, src_index, out,
                          reinterpret_cast<__bf16 *>(out_c8));
        }
        CB_LAUNCH_CHECK();
        return COMBAT_OK;
    }
    const int bytes = (4 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_fwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_fwd_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, src_index, out,
                       reinterpret_cast<__bf16 *>(out_c8), mse_partial);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_trigger_bwd(const float *x, const void *noise, const float *P, const float *k1,
                                  float noise_rate, int32_t n, int32_t hw, const float *d_out, const float *d_out2,
                                  const float *out, float l2_scale, int32_t pre_tanh, void *d_noise, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_bwd, x, noise, P, k1, noise_rate, n, hw, d_out, d_out2, out, l2_scale, pre_tanh, d_noise);
    if (!x || !noise || !P || !k1 || !d_noise || n < 0 || hw < 16 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (l2_scale != 0.f && !out) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {
        // the clamp mask (one bit per pixel) lives in this stream's scratch between the two launches; a batch whose mask
        // does not fit is taken in runs of images, one pair of launches each (224 x 224: 111 images per run)
        hipStream_t st = as_stream(stream);
        const size_t plane = (size_t)hw * hw;
        const BigRuns rn = big_runs(stream, hw, (size_t)n);
        unsigned short *mask = rn.mask;
        const int run = rn.run;
        if (!mask) return COMBAT_ELAUNCH;
        for (int i0 = 0; i0 < n; i0 += run) {
            const int ni = n - i0 < run ? n - i0 : run;
            const size_t o3 = (size_t)i0 * 3 * plane, o8 = (size_t)i0 * plane * 8;
            const __bf16 *nz = reinterpret_cast<const __bf16 *>(noise) + o8;
            hipLaunchKernelGGL(trigger_big_mask_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x + o3, nz, P,
                               noise_rate, hw, mask);
            CB_LAUNCH_CHECK();
            if (i0 + ni < n)
                hipLaunchKernelGGL(trigger_big_bwd_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x + o3, nz, P, k1,
                                   noise_rate, hw, d_out ? d_out + o3 : nullptr, d_out2 ? d_out2 + o3 : nullptr,
                                   out ? out + o3 : nullptr, l2_scale, pre_tanh, (const unsigned short *)mask,
                                   reinterpret_cast<__bf16 *>(d_noise) + o8);
            else
                COMBAT_LAUNCH(trigger_big_bwd_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x + o3, nz, P, k1,
                              noise_rate, hw, d_out ? d_out + o3 : nullptr, d_out2 ? d_out2 + o3 : nullptr,
                              out ? out + o3 : nullptr, l2_scale, pre_tanh, (const unsigned short *)mask,
                              reinterpret_cast<__bf16 *>(d_noise) + o8);
            CB_LAUNCH_CHECK();
        }
        return COMBAT_OK;
    }
    const int bytes = (5 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_bwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_bwd_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, d_out, d_out2, out, l2_scale,
                       pre_tanh, reinterpret_cast<__bf16 *>(d_noise));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_trigger_tv_fwd(const float *x, const void *noise, const float *P, const float *k1,
                                     float noise_rate, int32_t n, int32_t hw, float *out, float *mse_partial,
                                     float *tv_partial, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_tv_fwd, x, noise, P, k1, noise_rate, n, hw, out, mse_partial, tv_partial);
    if (!x || !noise || !P || !k1 || !out || !tv_partial || n < 0 || hw < 16 || hw > 64 || (hw & 3)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    const int bytes = (4 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_tv_fwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_tv_fwd_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, out, mse_partial, tv_partial);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_trigger_tv_bwd(const float *x, const void *noise, const float *P, const float *k1,
                                     float noise_rate, int32_t n, int32_t hw, const float *d_out, const float *d_out2,
                                     const float *out, float l2_scale, float tv_scale, int32_t pre_tanh, void *d_noise,
                                     void *stream) {
    if (hw > 64) return COMBAT_EINVAL;      // (combat_trigger_bwd's strip route has no total-variation form)
    if (tv_scale == 0.f)      // nothing to add: the launch of combat_trigger_bwd itself
        return combat_trigger_bwd(x, noise, P, k1, noise_rate, n, hw, d_out, d_out2, out, l2_scale, pre_tanh, d_noise, stream);
    COMBAT_PLAN_HOOK(combat_trigger_tv_bwd, x, noise, P, k1, noise_rate, n, hw, d_out, d_out2, out, l2_scale, tv_scale,
                     pre_tanh, d_noise);
    if (!x || !noise || !P || !k1 || !out || !d_noise || n < 0 || hw < 16 || hw > 64 || (hw & 3)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    const int bytes = (5 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_tv_bwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_tv_bwd_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, d_out, d_out2, out, l2_scale,
                       tv_scale, pre_tanh, reinterpret_cast<__bf16 *>(d_noise));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

// The total-variation trigger on the strip route (80 <= hw <= 256, hw % 16 == 0; smaller planes belong to
// combat_trigger_tv_fwd / _bwd).  Forward: trigger_big_fwd_kernel as combat_trigger_fwd launches it, then one reduction
// over the finished planes for the squared-error and total-variation partials.
extern "C" int combat_trigger_tv_big_fwd(const float *x, const void *noise, const float *P, const float *k1,
                                         float noise_rate, int32_t n, int32_t hw, float *out, float *mse_partial,
                                         float *tv_partial, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_tv_big_fwd, x, noise, P, k1, noise_rate, n, hw, out, mse_partial, tv_partial);
    if (!x || !noise || !P || !k1 || !out || !tv_partial || n < 0 || hw < 80 || hw > 256 || (hw & 15)) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(trigger_big_fwd_kernel, dim3(hw / 16, 3, n), dim3(256), 18 * hw * 4, st, x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, (const int *)nullptr, out,
                       (__bf16 *)nullptr);
    CB_LAUNCH_CHECK();
    COMBAT_LAUNCH(trigger_big_tv_kernel, dim3(3, n), dim3(1024), 0, st, x, (const float *)out, hw, mse_partial, tv_partial);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

// Backward: combat_trigger_bwd's runs of images (mask launch, gradient launch), the gradient launch with the stencil.
extern "C" int combat_trigger_tv_big_bwd(const float *x, const void *noise, const float *P, const float *k1,
                                         float noise_rate, int32_t n, int32_t hw, const float *d_out, const float *d_out2,
                                         const float *out, float l2_scale, float tv_scale, int32_t pre_tanh, void *d_noise,
                                         void *stream) {
    if (hw < 80 || hw > 256 || (hw & 15)) return COMBAT_EINVAL;
    if (tv_scale == 0.f)      // nothing to add: the launches of combat_trigger_bwd itself
        return combat_trigger_bwd(x, noise, P, k1, noise_rate, n, hw, d_out, d_out2, out, l2_scale, pre_tanh, d_noise, stream);
    COMBAT_PLAN_HOOK(combat_trigger_tv_big_bwd, x, noise, P, k1, noise_rate, n, hw, d_out, d_out2, out, l2_scale, tv_scale,
                     pre_tanh, d_noise);
    if (!x || !noise || !P || !k1 || !out || !d_noise || n < 0) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    hipStream_t st = as_stream(stream);
    const size_t plane = (size_t)hw * hw;
    const BigRuns rn = big_runs(stream, hw, (size_t)n);
    unsigned short *mask = rn.mask;
    const int run = rn.run;
    if (!mask) return COMBAT_ELAUNCH;
    for (int i0 = 0; i0 < n; i0 += run) {
        const int ni = n - i0 < run ? n - i0 : run;
        const size_t o3 = (size_t)i0 * 3 * plane, o8 = (size_t)i0 * plane * 8;
        const __bf16 *nz = reinterpret_cast<const __bf16 *>(noise) + o8;
        hipLaunchKernelGGL(trigger_big_mask_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x + o3, nz, P,
                           noise_rate, hw, mask);
        CB_LAUNCH_CHECK();
        if (i0 + ni < n)
            hipLaunchKernelGGL(trigger_big_tv_bwd_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x + o3, nz, P, k1,
                               noise_rate, hw, d_out ? d_out + o3 : nullptr, d_out2 ? d_out2 + o3 : nullptr, out + o3,
                               l2_scale, tv_scale, pre_tanh, (const unsigned short *)mask,
                               reinterpret_cast<__bf16 *>(d_noise) + o8);
        else
            COMBAT_LAUNCH(trigger_big_tv_bwd_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x + o3, nz, P, k1,
                          noise_rate, hw, d_out ? d_out + o3 : nullptr, d_out2 ? d_out2 + o3 : nullptr, out + o3,
                          l2_scale, tv_scale, pre_tanh, (const unsigned short *)mask,
                          reinterpret_cast<__bf16 *>(d_noise) + o8);
        CB_LAUNCH_CHECK();
    }
    return COMBAT_OK;
}

extern "C" int combat_trigger_pair_fwd(const float *x, const void *noise, const float *P, const float *k1,
                                       float noise_rate, int32_t n, int32_t hw, float *out_bd, float *out_cross,
                                       float *mse_partial, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_pair_fwd, x, noise, P, k1, noise_rate, n, hw, out_bd, out_cross, mse_partial);
    if (!x || !noise || !P || !k1 || !out_bd || !out_cross || n < 0 || hw < 16 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {      // strips, as combat_trigger_fwd: 2n rows in one launch, the partials of the first n behind it
        hipStream_t st = as_stream(stream);
        if (mse_partial) {
            hipLaunchKernelGGL(trigger_big_pair_fwd_kernel, dim3(hw / 16, 3, 2 * n), dim3(256), 18 * hw * 4, st, x,
                               reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, n, hw, out_bd, out_cross);
            CB_LAUNCH_CHECK();
            COMBAT_LAUNCH(trigger_big_mse_kernel, dim3(3, n), dim3(1024), 0, st, x, (const float *)out_bd, hw,
                          (const int *)nullptr, mse_partial);
        } else {
            COMBAT_LAUNCH(trigger_big_pair_fwd_kernel, dim3(hw / 16, 3, 2 * n), dim3(256), 18 * hw * 4, st, x,
                          reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, n, hw, out_bd, out_cross);
        }
        CB_LAUNCH_CHECK();
        return COMBAT_OK;
    }
    const int bytes = (4 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_pair_fwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_pair_fwd_kernel, dim3(3, 2 * n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, n, hw, out_bd, out_cross, mse_partial);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_trigger_pair_bwd(const float *x, const void *noise, const float *P, const float *k1,
                                       float noise_rate, int32_t n, int32_t hw, const float *d_bd, const float *d_bd2,
                                       const float *out_bd, float l2_scale, const float *d_cross, int32_t pre_tanh,
                                       void *d_noise, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_pair_bwd, x, noise, P, k1, noise_rate, n, hw, d_bd, d_bd2, out_bd, l2_scale, d_cross,
                     pre_tanh, d_noise);
    if (!x || !noise || !P || !k1 || !d_noise || n < 0 || hw < 16 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (l2_scale != 0.f && !out_bd) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {
        // as combat_trigger_bwd, over the 2n rows: the clamp mask of a run of rows in this stream's scratch, one pair of
        // launches per run (224 x 224: 111 rows per run).  A run may straddle the two halves, so the kernels take the
        // call's own pointers and the run's first row.
        hipStream_t st = as_stream(stream);
        const BigRuns rn = big_runs(stream, hw, 2 * (size_t)n);
        if (!rn.mask) return COMBAT_ELAUNCH;
        const __bf16 *nz = reinterpret_cast<const __bf16 *>(noise);
        const int rows = 2 * n;
        for (int r0 = 0; r0 < rows; r0 += rn.run) {
            const int nr = rows - r0 < rn.run ? rows - r0 : rn.run;
            hipLaunchKernelGGL(trigger_big_pair_mask_kernel, dim3(hw / 16, 3, nr), dim3(256), 16 * hw * 4, st, x, nz, P,
                               noise_rate, n, r0, hw, rn.mask);
            CB_LAUNCH_CHECK();
            if (r0 + nr < rows)
                hipLaunchKernelGGL(trigger_big_pair_bwd_kernel, dim3(hw / 16, 3, nr), dim3(256), 16 * hw * 4, st, x, nz, P, k1,
                                   noise_rate, n, r0, hw, d_bd, d_bd2, out_bd, l2_scale, d_cross, pre_tanh,
                                   (const unsigned short *)rn.mask, reinterpret_cast<__bf16 *>(d_noise));
            else
                COMBAT_LAUNCH(trigger_big_pair_bwd_kernel, dim3(hw / 16, 3, nr), dim3(256), 16 * hw * 4, st, x, nz, P, k1,
                              noise_rate, n, r0, hw, d_bd, d_bd2, out_bd, l2_scale, d_cross, pre_tanh,
                              (const unsigned short *)rn.mask, reinterpret_cast<__bf16 *>(d_noise));
            CB_LAUNCH_CHECK();
        }
        return COMBAT_OK;
    }
    const int bytes = (5 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_pair_bwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_pair_bwd_kernel, dim3(3, 2 * n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, n, hw, d_bd, d_bd2, out_bd, l2_scale,
                       d_cross, pre_tanh, reinterpret_cast<__bf16 *>(d_noise));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_trigger_groups_fwd(const float *x, const void *noise, const float *P, const float *k1,
                                         float noise_rate, int32_t n, int32_t hw, int32_t ps, float *out,
                                         float *mse_partial, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_groups_fwd, x, noise, P, k1, noise_rate, n, hw, ps, out, mse_partial);
    if (!x || !noise || !P || !k1 || !out || n < 0 || ps < 1 || hw < 16 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {      // strips, as combat_trigger_fwd
        hipStream_t st = as_stream(stream);
        if (mse_partial) {
            hipLaunchKernelGGL(trigger_big_groups_fwd_kernel, dim3(hw / 16, 3, n), dim3(256), 18 * hw * 4, st, x,
                               reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, ps, out);
            CB_LAUNCH_CHECK();
            COMBAT_LAUNCH(trigger_big_mse_kernel, dim3(3, n), dim3(1024), 0, st, x, (const float *)out, hw,
                          (const int *)nullptr, mse_partial);
        } else {
            COMBAT_LAUNCH(trigger_big_groups_fwd_kernel, dim3(hw / 16, 3, n), dim3(256), 18 * hw * 4, st, x,
                          reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, ps, out);
        }
        CB_LAUNCH_CHECK();
        return COMBAT_OK;
    }
    const int bytes = (4 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_groups_fwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_groups_fwd_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, ps, out, mse_partial);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_trigger_groups_bwd(const float *x, const void *noise, const float *P, const float *k1,
                                         float noise_rate, int32_t n, int32_t hw, int32_t ps, const float *d_out,
                                         const float *d_out2, const float *out, float l2_scale, int32_t pre_tanh,
                                         void *d_noise, void *stream) {
    COMBAT_PLAN_HOOK(combat_trigger_groups_bwd, x, noise, P, k1, noise_rate, n, hw, ps, d_out, d_out2, out, l2_scale, pre_tanh,
                     d_noise);
    if (!x || !noise || !P || !k1 || !d_noise || n < 0 || ps < 1 || hw < 16 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (l2_scale != 0.f && !out) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {
        // as combat_trigger_bwd: runs of images whose clamp mask fits this stream's scratch, one pair of launches each.
        // The mask does not depend on the blur, so its kernel is the plain one on the run's images; the second launch
        // takes the call's own pointers and the run's first image, which its choice of k1 counts from.
        hipStream_t st = as_stream(stream);
        const BigRuns rn = big_runs(stream, hw, (size_t)n);
        if (!rn.mask) return COMBAT_ELAUNCH;
        const size_t plane = (size_t)hw * hw;
        const __bf16 *nz = reinterpret_cast<const __bf16 *>(noise);
        for (int i0 = 0; i0 < n; i0 += rn.run) {
            const int ni = n - i0 < rn.run ? n - i0 : rn.run;
            hipLaunchKernelGGL(trigger_big_mask_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st,
                               x + (size_t)i0 * 3 * plane, nz + (size_t)i0 * plane * 8, P, noise_rate, hw, rn.mask);
            CB_LAUNCH_CHECK();
            if (i0 + ni < n)
                hipLaunchKernelGGL(trigger_big_groups_bwd_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x, nz, P, k1,
                                   noise_rate, hw, ps, i0, d_out, d_out2, out, l2_scale, pre_tanh,
                                   (const unsigned short *)rn.mask, reinterpret_cast<__bf16 *>(d_noise));
            else
                COMBAT_LAUNCH(trigger_big_groups_bwd_kernel, dim3(hw / 16, 3, ni), dim3(256), 16 * hw * 4, st, x, nz, P, k1,
                              noise_rate, hw, ps, i0, d_out, d_out2, out, l2_scale, pre_tanh,
                              (const unsigned short *)rn.mask, reinterpret_cast<__bf16 *>(d_noise));
            CB_LAUNCH_CHECK();
        }
        return COMBAT_OK;
    }
    const int bytes = (5 * hw * hw + 2 * hw) * 4;
    if (set_smem(trigger_groups_bwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(trigger_groups_bwd_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x,
                       reinterpret_cast<const __bf16 *>(noise), P, k1, noise_rate, hw, ps, d_out, d_out2, out, l2_scale,
                       pre_tanh, reinterpret_cast<__bf16 *>(d_noise));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_augment_fwd(const float *x, const int32_t *src_index, const float *params, int32_t n,
                                  int32_t hw, void *out_c8, float *out_f32, void *stream) {
    COMBAT_PLAN_HOOK(combat_augment_fwd, x, src_index, params, n, hw, out_c8, out_f32);
    if (!x || !out_c8 || n < 0 || hw < 2 || hw > 1024) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 96) {
        COMBAT_LAUNCH(augment_fwd_big_kernel, dim3((hw * hw + 255) / 256, n), dim3(256), 0, as_stream(stream), x, src_index,
                           params, hw, reinterpret_cast<uint4 *>(out_c8), out_f32);
        CB_LAUNCH_CHECK();
        return COMBAT_OK;
    }
    const int bytes = 3 * hw * hw * 4;
    if (set_smem(augment_fwd_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(augment_fwd_kernel, dim3(n), dim3(256), bytes, as_stream(stream), x, src_index, params, hw,
                       reinterpret_cast<uint4 *>(out_c8), out_f32);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_augment_bwd(const void *d_c8, int32_t c8_channels, const float *params, int32_t n, int32_t hw,
                                  float *d_x, int32_t accumulate, void *stream) {
    COMBAT_PLAN_HOOK(combat_augment_bwd, d_c8, c8_channels, params, n, hw, d_x, accumulate);
    if (!d_c8 || !d_x || c8_channels < 3 || n < 0 || hw < 2 || hw > 1024) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 96) {
        hipStream_t st = as_stream(stream);
        if (!accumulate && hipMemsetAsync(d_x, 0, (size_t)n * 3 * hw * hw * sizeof(float), st) != hipSuccess) return COMBAT_ELAUNCH;
        COMBAT_LAUNCH(augment_bwd_big_kernel, dim3((hw * hw + 255) / 256, n), dim3(256), 0, st,
                           reinterpret_cast<const __bf16 *>(d_c8), c8_channels, params, hw, d_x);
        CB_LAUNCH_CHECK();
        return COMBAT_OK;
    }
    const int bytes = 3 * hw * hw * 4;
    if (set_smem(augment_bwd_gather_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(augment_bwd_gather_kernel, dim3(n), dim3(256), bytes, as_stream(stream),
                       reinterpret_cast<const __bf16 *>(d_c8), c8_channels, params, hw, d_x, accumulate);
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}

extern "C" int combat_dct_u8(const float *x, const float *D, int32_t n, int32_t hw, void *out_c8, void *stream) {
    COMBAT_PLAN_HOOK(combat_dct_u8, x, D, n, hw, out_c8);
    if (!x || !D || !out_c8 || n < 0 || hw < 4 || hw > 256 || (hw & 3) || (hw > 64 && (hw & 15))) return COMBAT_EINVAL;
    if (n == 0) return COMBAT_OK;
    if (hw > 64) {
        COMBAT_LAUNCH(dct_u8_big_kernel, dim3(hw / 16, 3, n), dim3(256), 2 * 16 * hw * 4, as_stream(stream), x, D, hw,
                           reinterpret_cast<__bf16 *>(out_c8));
        CB_LAUNCH_CHECK();
        return COMBAT_OK;
    }
    const int bytes = (4 * hw * hw + 2 * hw) * 4;
    if (set_smem(dct_u8_kernel, bytes)) return COMBAT_ELAUNCH;
    COMBAT_LAUNCH(dct_u8_kernel, dim3(3, n), dim3(256), bytes, as_stream(stream), x, D, hw,
                       reinterpret_cast<__bf16 *>(out_c8));
    CB_LAUNCH_CHECK();
    return COMBAT_OK;
}
