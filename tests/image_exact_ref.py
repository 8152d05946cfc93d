"""Exact and element-wise references for the image-side kernels (trigger.hip, warp.hip): numpy float64 written from
include/combat_hip.h and the kernels' formula comments, no project code.  The third user of the exact-test kit
(conv_exact_ref.py), whose guard bands, lattice helpers and comparisons are re-used as they are.

    out     = Kb clamp(x + rate P N P^T, -1, 1) Kb^T                 Kb: dense reflect-padded 3-tap matrix
    d_noise = rate P (mask o (Kb^T g Kb)) P^T [o (1 - t^2)]          g = d_out + d_out2 + 2 l2 (out - x) + tv_scale stencil(out)
    dct     = D q D^T, q = trunc((x + 1) / 2 * 255) in float32       (the kernel's own IEEE operations: q is bit-equal)
    augment = crop / flip copy and its adjoint;  warp = bilinear sample (align_corners, zeros), d/dgrid, d/dx

Every function takes `mut`, a set of names of deliberately wrong variants (test_image_exact_cpu.py shows that the
case tables reject each of them); the empty set is the reference.

Lattice data (exact mode): P symmetric in multiples of 1/4 with |row| sums <= 3/4, noise in multiples of 1/4, x in
multiples of 1/128, rate = 1/8 and the asymmetric triple (1/2, 1/4, 1/4) put `out` on a 2^-13 grid with every
intermediate of every summation order an fp32 number (range_check on the absolute-value chain, not a tolerance).
Bound mode: E = k 2^-24 (the element's absolute-value chain), k counted from the source beside each formula.
"""
from types import SimpleNamespace

import numpy as np
import torch

from conv_exact_ref import (_PATTERN, SLACK, TWO24, Guarded, assert_not_vacuous, assert_within_bound, bf16, gen,  # noqa: F401
                            half_ulp_bf16, is_f32, is_multiple, lattice, pick, range_check, report_mismatch, rne_bf16,
                            summation_bound, trunc_bf16)

U24 = 2.0 ** -24


def t64(a):
    """numpy -> torch float64 (the kit's comparisons take torch tensors)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def f32_exact(a):
    return bool((np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64) == a).all())


# ------------------------------------------------------------------------------------------------ matrices
def blur_matrix(k, hw, mut=()):
    """out[i] = k0 in[r(i - 1)] + k1 in[i] + k2 in[r(i + 1)] with reflect padding r(-1) = 1, r(hw) = hw - 2: rows 0 and
    hw - 1 carry k0 + k2 on one entry, so Kb != Kb^T whatever the triple."""
    k0, k1, k2 = (float(v) for v in k)
    if "swap_k" in mut:
        k0, k2 = k2, k0
    Kb = np.zeros((hw, hw))
    for i in range(hw):
        Kb[i, i - 1 if i > 0 else 1] += k0
        Kb[i, i] += k1
        Kb[i, i + 1 if i + 1 < hw else hw - 2] += k2
    return Kb


def blur_stack(k1, ki, hw, mut=()):
    """[rows][1][hw][hw]: row r blurs with triple k1[ki[r]]."""
    mats = np.stack([blur_matrix(k, hw, mut) for k in np.atleast_2d(np.asarray(k1, dtype=np.float64))])
    return mats[np.asarray(ki)][:, None]


def dct_matrix(n):
    """Orthonormal DCT-II, D[k][i] = c_k cos(pi (2 i + 1) k / (2 n))."""
    k, i = np.arange(n)[:, None], np.arange(n)[None, :]
    d = np.cos(np.pi * (2 * i + 1) * k / (2 * n)) * np.sqrt(2.0 / n)
    d[0] *= np.sqrt(0.5)
    return d


def lowpass_matrix(n, ratio=0.65):
    """P = D[:K]^T D[:K], K = int(n ratio), as the fp32 matrix the kernels are handed (returned in float64)."""
    d = dct_matrix(n)[:int(n * ratio)]
    return (d.T @ d).astype(np.float32).astype(np.float64)


def gaussian_triple(sigma):
    """Normalised 3-tap Gaussian in float32 (the operand), returned in float64."""
    xs = np.array([-1.0, 0.0, 1.0], dtype=np.float32)
    pdf = np.exp(-0.5 * (xs / np.float32(sigma)) ** 2).astype(np.float32)
    return (pdf / pdf.sum(dtype=np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ row selection
def plain_rows(n, src_index=None):
    """combat_trigger_fwd: output row i is made from row src_index[i] of x and of the noise, one triple."""
    src = np.arange(n) if src_index is None else np.asarray(src_index)
    return src, src, np.zeros(len(src), dtype=np.int64)


def pair_rows(n, mut=()):
    """combat_trigger_pair_*: 2n rows over ONE batch x [n]; row reads x[row mod n], noise[row], triple k1[row >= n]."""
    row = np.arange(2 * n)
    return row % n, (row % n if "cross_noise" in mut else row), (row >= n).astype(np.int64)


def groups_rows(n, ps, groups, mut=()):
    """combat_trigger_groups_*: image i is blurred with k1[i / ps]; the last group may be short."""
    i = np.arange(n)
    ki = np.minimum((i + 1) // ps, groups - 1) if "group_shift" in mut else i // ps
    return i, i, ki


# ------------------------------------------------------------------------------------------------ trigger forward
def trigger_fwd(x, noise, P, k1, rate, xi, ni, ki, mut=()):
    """x [*][3][hw][hw], noise [*][3][hw][hw] (the bf16 values), P [hw][hw], k1 [G][3]; rows as xi / ni / ki.
    Returns pre, out and their absolute-value chains [rows][3][hw][hw]."""
    hw = x.shape[-1]
    xr, nr, Kb = x[xi], noise[ni], blur_stack(k1, ki, hw, mut)
    KbT = np.swapaxes(Kb, -1, -2)
    pre = xr + rate * (P @ nr @ P.T)
    bd = np.clip(pre, -1.0, 1.0)
    out = KbT @ bd @ Kb if "kb_T" in mut else Kb @ bd @ KbT
    aP, aK = np.abs(P), np.abs(Kb)
    pre_abs = np.abs(xr) + abs(rate) * (aP @ np.abs(nr) @ aP.T)
    out_abs = aK @ pre_abs @ np.swapaxes(aK, -1, -2)
    return SimpleNamespace(xr=xr, nr=nr, Kb=Kb, pre=pre, out=out, pre_abs=pre_abs, out_abs=out_abs, hw=hw)


def fwd_bounds(f):
    """E_pre: two mm4 chains of hw fma terms each and the fma that adds x: k = 2 hw + 1 on |x| + rate |P||N||P|.
    E_out: the two 3-term blur passes on top: k = 2 hw + 7 on |Kb| (|x| + rate |P||N||P|) |Kb|^T (the clamp is
    1-Lipschitz and exact)."""
    return (2 * f.hw + 1) * U24 * f.pre_abs, (2 * f.hw + 7) * U24 * f.out_abs


def fwd_range_check(f, P, noise_rows, rate, qx, qn, qp, qk):
    """The lattice condition of the forward chain; returns the quantum of `out`."""
    aP = np.abs(P)
    range_check(t64(aP @ np.abs(noise_rows)), qp * qn, "|P||N|")
    range_check(t64(aP @ np.abs(noise_rows) @ aP.T), qp * qp * qn, "|P||N||P|")
    q = min(qx, rate * qp * qp * qn)
    range_check(t64(f.pre_abs), q, "|x| + rate |P||N||P|")
    aK = np.abs(f.Kb)
    range_check(t64(aK @ f.pre_abs), q * qk, "|Kb| |pre|")
    range_check(t64(f.out_abs), q * qk * qk, "|Kb| |pre| |Kb|^T")
    assert f32_exact(f.pre) and f32_exact(f.out) and is_multiple(t64(f.out), q * qk * qk)
    return q * qk * qk


def plane_sums(hw, strip):
    """Additions a plane's sum passes through per term stream: the thread's chain, the lane fold, the wave sums.
    Whole plane (256 threads): ceil(hw^2 / 256) + 8 tree levels (mse) / + 6 shuffles + 3 (tv).  Strip route (1024
    threads): ceil(hw^2 / 1024) + 6 shuffles + 15."""
    if strip:
        c = -(-hw * hw // 1024)
        return c + 21, 2 * c + 21
    c = -(-hw * hw // 256)
    return c + 8, 2 * c + 9


def mse_tv(out, xr, e_out, hw, strip, exact=False):
    """Per-(row, channel) sums with their bounds: (mse, E_mse, tv, E_tv, tv_abs).  e_out: the error of `out` (0 in exact
    mode, where the differences are exact too).  mse term d^2 with d = out - x (one rounding of d, the fma's rounding is the
    chain's); tv terms |a - b| (one rounding each)."""
    k_mse, k_tv = plane_sums(hw, strip)
    d = out - xr
    r = 0.0 if exact else U24
    e_d = e_out + r * np.abs(d)
    d2_err = 2 * np.abs(d) * e_d + e_d * e_d
    mse = (d * d).sum((-1, -2))
    e_mse = d2_err.sum((-1, -2)) + k_mse * U24 * (d * d + d2_err).sum((-1, -2))
    dv, dh = np.abs(out[..., 1:, :] - out[..., :-1, :]), np.abs(out[..., :, 1:] - out[..., :, :-1])
    tv = dv.sum((-1, -2)) + dh.sum((-1, -2))
    ev = e_out[..., 1:, :] + e_out[..., :-1, :] + r * dv
    eh = e_out[..., :, 1:] + e_out[..., :, :-1] + r * dh
    prop = ev.sum((-1, -2)) + eh.sum((-1, -2))
    return mse, e_mse, tv, prop + k_tv * U24 * (tv + prop), tv


def stencil(out, mut=()):
    """d TV / d out: sgn(o - up) - sgn(down - o) + sgn(o - left) - sgn(right - o), terms past the border absent,
    sgn(0) = 0."""
    def sgn(d):
        s = np.sign(d)
        return np.where(d == 0, 1.0, s) if "sgn0" in mut else s
    s = np.zeros_like(out)
    s[..., 1:, :] += sgn(out[..., 1:, :] - out[..., :-1, :])
    s[..., :-1, :] -= sgn(out[..., 1:, :] - out[..., :-1, :])
    s[..., :, 1:] += sgn(out[..., :, 1:] - out[..., :, :-1])
    s[..., :, :-1] -= sgn(out[..., :, 1:] - out[..., :, :-1])
    return s


# ------------------------------------------------------------------------------------------------ trigger backward
def image_gradient(xr, d_out, d_out2, out, l2, tv_scale, mut=()):
    """g and sum of its terms' magnitudes; any of d_out / d_out2 may be None, l2 / tv_scale 0."""
    g, a = np.zeros_like(xr), np.zeros_like(xr)
    for t in (d_out, d_out2):
        if t is not None:
            g, a = g + t, a + np.abs(t)
    if l2 != 0:
        g, a = g + 2 * l2 * (out - xr), a + 2 * abs(l2) * np.abs(out - xr)
    if tv_scale != 0:
        s = stencil(out, mut)
        g, a = g + tv_scale * s, a + abs(tv_scale) * np.abs(s)
    return g, a


def pair_gradient(x, n, d_bd, d_bd2, out_bd, l2, d_cross, mut=()):
    """Rows [0, n): d_bd + d_bd2 + the L2 term on out_bd; rows [n, 2n): d_cross alone (None: zero), no L2 term."""
    g1, a1 = image_gradient(x, d_bd, d_bd2, out_bd, l2, 0.0)
    g2, a2 = image_gradient(x, d_cross, None, out_bd, l2 if "cross_l2" in mut else 0.0, 0.0)
    return np.concatenate([g1, g2]), np.concatenate([a1, a2])


def trigger_bwd(x, noise, P, k1, rate, xi, ni, ki, g, g_abs, pre_tanh, mut=()):
    """d_noise [rows][3][hw][hw] (before the bf16 store) and its absolute-value chain.  The clamp passes the gradient
    at the bounds, as torch.clamp does."""
    hw = x.shape[-1]
    xr, nr, Kb = x[xi], noise[ni], blur_stack(k1, ki, hw, mut)
    KbT = np.swapaxes(Kb, -1, -2)
    pre = xr + rate * (P @ nr @ P.T)
    mask = (pre > -1) & (pre < 1) if "strict_mask" in mut else (pre >= -1) & (pre <= 1)
    if "mask_row" in mut:
        mask = np.roll(mask, 1, axis=-2)
    inner = Kb @ g @ KbT if "kb_T" in mut else KbT @ g @ Kb
    d = P @ (rate * mask * inner) @ P.T
    aP, aK = np.abs(P), np.abs(Kb)
    inner_abs = np.swapaxes(aK, -1, -2) @ g_abs @ aK
    r_abs = aP @ (abs(rate) * mask * inner_abs) @ aP.T
    t2 = 1 - nr * nr
    # g: the sum of the two gradients, out - x, its fma and the stencil's fma round once each: 4; g Kb and Kb^T (.):
    # 3 terms each; the product with rate: 1; two mm4 chains of hw terms: k = 2 hw + 11
    e = (2 * hw + 11) * U24 * r_abs
    if pre_tanh:
        # t^2, 1 - t^2 and the product round once each on magnitudes <= r_abs: 3 more
        d, e = d * t2, e * t2 + 3 * U24 * r_abs
    return SimpleNamespace(d=d, e=e, r_abs=r_abs, inner_abs=inner_abs, mask=mask, pre=pre, g_abs=g_abs, Kb=Kb, nr=nr, hw=hw)


def bwd_range_check(b, P, rate, qg, qn, qp, qk, pre_tanh):
    aP, aK = np.abs(P), np.abs(b.Kb)
    range_check(t64(b.g_abs), qg, "|g|")
    range_check(t64(b.g_abs @ aK), qg * qk, "|g||Kb|")
    range_check(t64(b.inner_abs), qg * qk * qk, "|Kb|^T|g||Kb|")
    w = rate * b.mask * b.inner_abs
    q = qg * qk * qk * rate
    range_check(t64(w), q, "rate |inner|")
    range_check(t64(aP @ w), q * qp, "|P||w|")
    range_check(t64(b.r_abs), q * qp * qp, "|P||w||P|")
    q = q * qp * qp
    if pre_tanh:
        q = q * qn * qn
        range_check(t64(b.r_abs * (1 - b.nr * b.nr)), q, "|r| (1 - t^2)")
    assert f32_exact(b.d) and is_multiple(t64(b.d), q)
    return q


# ------------------------------------------------------------------------------------------------ c8 images
def hilo(v):
    """(hi, lo) = (RNE_bf16(v), RNE_bf16(v - hi)) of fp32 values v (asserted), as float64 tensors."""
    v = t64(v)
    hi = rne_bf16(v)
    return hi, rne_bf16(v - hi)


def c8_expect(v, mut=()):
    """v [rows][3][hw][hw] fp32 values -> the NHWC c8 image [rows][hw][hw][8]: hi, lo, two zero channels."""
    v = t64(v)
    hi = trunc_bf16(v) if "hi_trunc" in mut else rne_bf16(v)
    lo = torch.zeros_like(hi) if "lo_drop" in mut else rne_bf16(v - hi)
    pad = torch.zeros_like(hi[:, :2])
    if "pad" in mut:
        pad[:, 0, 0, 0] = 2.0 ** -20
    return torch.cat([hi, lo, pad], 1).permute(0, 2, 3, 1).contiguous()


def nhwc3(planes, channels=8, fill=float("nan")):
    """[rows][3][hw][hw] -> the NHWC source [rows][hw][hw][channels] a kernel reads channels 0..2 of; the other
    channels hold NaN (a kernel that read one would show it)."""
    p = t64(planes)
    out = torch.full((p.shape[0], p.shape[2], p.shape[3], channels), fill, dtype=torch.float64)
    out[..., :3] = p.permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------ DCT input
def quantise(x32, mut=()):
    """q = trunc((x + 1) / 2 * 255) in float32, operation by operation as the kernel; x32 float32 in [-1, 1]."""
    assert x32.dtype == np.float32
    q = (x32 + np.float32(1)) / np.float32(2) * np.float32(255)
    if "round_q" in mut:
        q = np.floor(q + np.float32(0.5))
    return np.trunc(q).astype(np.float64)


def dct_u8(x32, D, mut=()):
    """(D q D^T, |D| q |D|^T, q) per plane."""
    q = quantise(x32, mut)
    y = D.T @ q @ D if "dct_T" in mut else D @ q @ D.T
    return y, np.abs(D) @ q @ np.abs(D).T, q


# ------------------------------------------------------------------------------------------------ augmentation (copy paths)
def augment_copy(x, src_index, params, mut=()):
    """out[i][c][y][xo] = I(u + ox, y + oy) of image src_index[i], u = hw - 1 - xo when flipped, zero outside the
    image.  params [n][4] = (ox, oy, 0, flip)."""
    n, hw = len(params), x.shape[-1]
    out = np.zeros((n, 3, hw, hw))
    yy, xo = np.meshgrid(np.arange(hw), np.arange(hw), indexing="ij")
    for i in range(n):
        ox, oy, flip = int(params[i][0]), int(params[i][1]), params[i][3] != 0
        u = hw - 1 - xo if flip else xo
        sx, sy = u + ox, yy + oy
        ok = (sx >= 0) & (sx < hw) & (sy >= 0) & (sy < hw)
        src = x[i if src_index is None else int(src_index[i])]
        out[i][:, ok] = src[:, sy[ok], sx[ok]]
    return out


def augment_adjoint(d, params):
    """d [n][3][hw][hw] (gradient of the augmented image) -> gradient of the source image: the transpose of the copy."""
    n, hw = len(params), d.shape[-1]
    dx = np.zeros((n, 3, hw, hw))
    yy, xo = np.meshgrid(np.arange(hw), np.arange(hw), indexing="ij")
    for i in range(n):
        ox, oy, flip = int(params[i][0]), int(params[i][1]), params[i][3] != 0
        u = hw - 1 - xo if flip else xo
        sx, sy = u + ox, yy + oy
        ok = (sx >= 0) & (sx < hw) & (sy >= 0) & (sy < hw)
        dx[i][:, sy[ok], sx[ok]] += d[i][:, yy[ok], xo[ok]]
    return dx


# ------------------------------------------------------------------------------------------------ warp
def _taps(grid, H):
    ix, iy = (grid[..., 0] + 1) * 0.5 * (H - 1), (grid[..., 1] + 1) * 0.5 * (H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    return x0, y0, ix - x0, iy - y0


def _tap(plane, xx, yy, H, mut=()):
    """plane [3][H][H] at integer taps (arrays [H][H]); zero outside."""
    lim = H - 1 if "drop_last_tap" in mut else H
    ok = (xx >= 0) & (xx < lim) & (yy >= 0) & (yy < lim)
    v = plane[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, H - 1)]
    return np.where(ok[None], v, 0.0)


def warp_fwd(x, src_index, grid, n, mut=()):
    """F.grid_sample(bilinear, zeros, align_corners=True); grid [H][H][2] shared or [n][H][H][2]."""
    H = x.shape[-1]
    out = np.zeros((n, 3, H, H))
    for i in range(n):
        x0, y0, tx, ty = _taps(grid if grid.ndim == 3 else grid[i], H)
        p = x[i if src_index is None else int(src_index[i])]
        out[i] = ((1 - tx) * (1 - ty) * _tap(p, x0, y0, H, mut) + tx * (1 - ty) * _tap(p, x0 + 1, y0, H, mut)
                  + (1 - tx) * ty * _tap(p, x0, y0 + 1, H, mut) + tx * ty * _tap(p, x0 + 1, y0 + 1, H, mut))
    return out


def warp_bwd(x, d, grid, n, groups, mut=()):
    """partial [groups][H][H][2] = 0.5 (H - 1) sum over the group's images and the channels of d dsample/dgrid, and
    the same sum of magnitudes.  Group g owns images [g per, (g + 1) per), per = ceil(n / groups)."""
    H = x.shape[-1]
    per = -(-n // groups)
    part, mag = np.zeros((groups, H, H, 2)), np.zeros((groups, H, H, 2))
    for i in range(n):
        x0, y0, tx, ty = _taps(grid if grid.ndim == 3 else grid[i], H)
        v00, v10 = _tap(x[i], x0, y0, H, mut), _tap(x[i], x0 + 1, y0, H, mut)
        v01, v11 = _tap(x[i], x0, y0 + 1, H, mut), _tap(x[i], x0 + 1, y0 + 1, H, mut)
        k = 0.5 * (H - 1)
        gx, gy = (1 - ty) * (v10 - v00) + ty * (v11 - v01), (1 - tx) * (v01 - v00) + tx * (v11 - v10)
        ax = (1 - ty) * (np.abs(v10) + np.abs(v00)) + ty * (np.abs(v11) + np.abs(v01))
        ay = (1 - tx) * (np.abs(v01) + np.abs(v00)) + tx * (np.abs(v11) + np.abs(v10))
        part[i // per, ..., 0] += k * (d[i] * gx).sum(0)
        part[i // per, ..., 1] += k * (d[i] * gy).sum(0)
        mag[i // per, ..., 0] += k * (np.abs(d[i]) * ax).sum(0)
        mag[i // per, ..., 1] += k * (np.abs(d[i]) * ay).sum(0)
    return part, mag


def warp_bwd_input(d, grid, n):
    """d_x = transpose of warp_fwd applied to d, and the sum of the magnitudes that meet in each element."""
    H = d.shape[-1]
    dx, mag = np.zeros((n, 3, H, H)), np.zeros((n, 3, H, H))
    for i in range(n):
        x0, y0, tx, ty = _taps(grid if grid.ndim == 3 else grid[i], H)
        for ddx, ddy, w in ((0, 0, (1 - tx) * (1 - ty)), (1, 0, tx * (1 - ty)), (0, 1, (1 - tx) * ty), (1, 1, tx * ty)):
            xx, yy = x0 + ddx, y0 + ddy
            ok = (xx >= 0) & (xx < H) & (yy >= 0) & (yy < H)
            for c in range(3):
                np.add.at(dx[i, c], (yy[ok], xx[ok]), (w * d[i, c])[ok])
                np.add.at(mag[i, c], (yy[ok], xx[ok]), np.abs(w * d[i, c])[ok])
    return dx, mag


# ------------------------------------------------------------------------------------------------ comparisons
def assert_elementwise(got, ref, e, name, stored_bf16=False):
    """|got - ref| <= E (fp32 output) or half_ulp_bf16(|ref| + E) + E (bf16 output), E given per element; prints the
    worst |err| / bound.  For a bf16 output that ratio is ruled by the half ulp (some element of thousands sits next to
    a tie), so the share of E the worst element uses, (|err| - half ulp) / E, is printed too: documentation, not a
    criterion."""
    if stored_bf16:
        over = ((t64(got) - t64(ref)).abs() - half_ulp_bf16(t64(ref).abs() + t64(e))) / t64(e).clamp_min(1e-300)
        print("%s: worst (|err| - half ulp) / E = %.3f" % (name, float(over.max())))
    assert_within_bound(t64(got), t64(ref), t64(e) * TWO24, -3, name, stored_bf16=stored_bf16)


def edge_report(got, ref, bound, hw, name):
    """Worst |err| / bound on the rows and columns where the strip kernels change behaviour: the reflect edges, the
    first seam and the rows on either side of it."""
    r = np.abs(np.asarray(got) - np.asarray(ref)) / np.maximum(np.asarray(bound), 1e-300)
    rows = {i: float(r[..., i, :].max()) for i in (0, 15, 16, 17, hw - 1) if i < hw}
    cols = {j: float(r[..., :, j].max()) for j in (0, hw - 1)}
    print("%s: worst |err| / bound on rows %s, columns %s" % (name, rows, cols))
