"""Case tables and host-side builders of test_norm_exact_gpu.py (checked without a GPU by test_norm_exact_cpu.py).

A NormCase is one (groups, pixels per group, C, partial rows per group) shape of the normalisation family; rows = 0 is
the direct form (sums from the tensor itself).  The same case drives the fused forward (combat_norm_act_fused /
combat_norm_add_act_fused), the forward chain (combat_norm_finalize + combat_affine_act), the fused backward
(combat_norm_bwd_fused) and the backward chain (combat_norm_bwd_finalize + combat_norm_bwd_apply).  An UpCase is one
shape of the UNet decoder glue.  Shapes are the smallest that reach a path; which path is asserted in the CPU file.
"""
from collections import namedtuple
from types import SimpleNamespace

import torch

import norm_exact_ref as R

NormCase = namedtuple("NormCase", "id groups px C rows eps slope add running const seed")
UpCase = namedtuple("UpCase", "id N H W C skip rows eps seed")


def nc(groups, px, C, rows, eps=0.0, slope=0.25, add=0, running=None, const=(), seed=0):
    """add: 0 none, 1 the residual alone, 2 with add_scale / add_shift.  running: BatchNorm's running statistics and
    num_batches_tracked (default: whenever there is one group)."""
    running = groups == 1 if running is None else running
    cid = "g%d_px%d_c%d_r%d" % (groups, px, C, rows)
    cid += ("_eps" if eps else "") + ("_s0" if slope == 0 else "") + ("", "_add", "_addtab")[add] + ("_const" if const else "")
    return NormCase(cid, groups, px, C, rows, eps, slope, add, running, tuple(const),
                    seed or (groups * 7919 + px * 31 + C * 13 + rows) % 100003)


def uc(N, H, W, C, skip, rows=0, eps=0.0):
    cid = "n%d_%dx%d_c%d%s_r%d" % (N, H, W, C, "_skip" if skip else "", rows)
    return UpCase(cid, N, H, W, C, skip, rows, eps, (N * 7919 + H * 131 + W * 31 + C * 13 + rows + skip) % 100003)


# row reductions: every unroll boundary of fused_reduce_rows (4 x 32 rows), reduce_rows (8 x 4 rows), the stage-1 switch
# (256 | 257: 5 rows per slice, 12 empty slices) and 65 rows per stage-1 slice (4160)
_ROWS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4160)
_GC = ((1, 8), (3, 72), (1, 72), (3, 8))
_PX = (255, 256, 257, 300)
ROW_CASES = [nc(_GC[i % 4][0], _PX[i % 4], _GC[i % 4][1], rows) for i, rows in enumerate(_ROWS)]
ROW_CASES += [nc(1, 300, 8, 257), nc(3, 255, 8, 4160), nc(3, 256, 72, 256)]

# one ragged pass of the pixel chunk (chunk 256), with partial rows
ONEPASS_CASES = [nc(3, 1, 8, 2, eps=0.25), nc(1, 37, 72, 7), nc(3, 255, 8, 2), nc(1, 256, 72, 2), nc(3, 257, 72, 7)]

# more than one load_pass per workgroup: chunk 512 (513 chunks, the last of 37 pixels), 512 at two channel workgroups,
# the InstanceNorm form, chunk 1024
MULTIPASS_CASES = [nc(1, 262181, 8, 33), nc(1, 131109, 72, 129), nc(5, 52261, 8, 7), nc(1, 524325, 8, 257)]

# direct form: the group is one chunk of px pixels (1024: four passes), no partial rows
DIRECT_CASES = [nc(3, px, C, 0, eps=0.25 if px == 1 else 0.0)
                for px, C in zip((1, 4, 33, 49, 196, 784, 1023, 1024), (8, 64, 72, 8, 64, 72, 8, 64))]

# combat_norm_add_act_fused: bn2 + shortcut (+ the shortcut's own BatchNorm) + ReLU
ADD_CASES = [nc(1, 300, 72, 33, slope=0.0, add=1), nc(1, 257, 8, 2, add=2), nc(3, 49, 64, 0, add=1),
             nc(1, 196, 72, 0, slope=0.0, add=2), nc(1, 262181, 8, 31, slope=0.0, add=2), nc(3, 37, 8, 2, add=1)]

# a constant channel among live ones (var = 0, eps = 0.25), and a single pixel with running statistics
DEGENERATE_CASES = [nc(1, 256, 72, 3, eps=0.25, const=(2, 66)), nc(3, 256, 8, 0, eps=0.25, const=(5,)),
                    nc(1, 1, 8, 1, eps=0.25), nc(1, 1, 8, 0, eps=0.25)]

FORWARD_CASES = ROW_CASES + ONEPASS_CASES + MULTIPASS_CASES + DIRECT_CASES + ADD_CASES + DEGENERATE_CASES
# the backward takes an optional `add` (no tables); the residual cases that differ only in the tables fold into one
BACKWARD_CASES = ROW_CASES + ONEPASS_CASES + MULTIPASS_CASES + DIRECT_CASES + [c for c in ADD_CASES if c.add == 1] \
    + DEGENERATE_CASES
# the stand-alone chains (finalize + element-wise pass) need partial rows and take no residual in the forward
CHAIN_CASES = [c for c in ROW_CASES + ONEPASS_CASES + DEGENERATE_CASES if c.rows] + MULTIPASS_CASES[:1]

# Gaussian data: non-dyadic gamma / beta (none with several groups: InstanceNorm as the UNet uses it), eps = 1e-5,
# slope 0.2, odd pixel counts
BOUND_CASES = [nc(1, 300, 72, 33, eps=1e-5, slope=0.2), nc(3, 49, 8, 0, eps=1e-5, slope=0.2),
               nc(3, 9, 72, 0, eps=1e-5, slope=0.2), nc(1, 257, 8, 257, eps=1e-5, slope=0.2, add=2),
               nc(1, 49, 64, 0, eps=1e-5, slope=0.2, add=1), nc(1, 2085, 8, 5, eps=1e-5, slope=0.2),
               nc(3, 49, 8, 2, eps=1e-5, slope=0.2)]

# upsample: 1x1 (both output rows read the one input row), H != W, the UNet's 7 / 14 / 28 maps (ragged bands at 7 and
# 14), 32 x 32 = the 1024-pixel limit; fused with 0 (direct), 1, 7, 256 partial rows
UP_CASES = [uc(3, 1, 1, 8, 1, 0, eps=0.25), uc(1, 1, 1, 72, 0, 1, eps=0.25), uc(1, 2, 2, 72, 0, 7), uc(3, 3, 5, 64, 1, 0),
            uc(1, 5, 3, 8, 0, 256), uc(1, 7, 7, 72, 1, 7), uc(3, 7, 7, 8, 0, 0), uc(3, 14, 14, 8, 0, 1),
            uc(1, 14, 14, 72, 1, 0), uc(1, 28, 28, 64, 1, 256), uc(3, 28, 28, 8, 0, 0), uc(3, 32, 32, 8, 1, 0),
            uc(1, 32, 32, 8, 0, 7)]
UP_BOUND_CASES = [uc(3, 3, 5, 8, 1, 0, eps=1e-5), uc(1, 7, 7, 72, 1, 7, eps=1e-5), uc(1, 14, 14, 64, 0, 0, eps=1e-5)]

# combat_bn_eval_fold_batch launches 2 x 256 threads per descriptor in a grid-stride loop
FOLD_CHANNELS = (1, 63, 512, 513)


# ------------------------------------------------------------------------------------------------ restated from norm.hip
def fused_chunk(pxg, groups, C):
    """Restated from norm.hip (fused_chunk): pixels per workgroup of the fused kernels with partial rows."""
    chunk = 256
    while -(-pxg // chunk) * groups * ((C + 63) // 64) > 1024:
        chunk *= 2
    return chunk


def stage1(rows):
    """Restated from norm.hip (maybe_stage1, kStageRows = 64): (rows per slice, empty slices) or None without stage 1."""
    if rows <= 256:
        return None
    per = -(-rows // 64)
    return per, 64 - -(-rows // per)


def up_bands(N, H, W, C):
    """Restated from norm.hip (combat_unet_up_fused): (output rows per band, number of bands)."""
    Ho, Wo, bands = 2 * H, 2 * W, 1
    while N * ((C + 63) // 64) * bands < 512 and bands * 2 <= Ho and (Ho // (bands * 2)) * Wo >= 32:
        bands *= 2
    band = -(-Ho // bands)
    return band, -(-Ho // band)


# ------------------------------------------------------------------------------------------------ builders: lattice
def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=R.gen(seed)).double()


def affine(C, seed):
    """Dyadic gamma; integer beta: odd channels around zero (both branches of the activation), the others high enough
    that the outputs land in [256, 512), where odd integers are ties between bf16 neighbours."""
    gamma = R.pick((-0.5, 0.5, 1.0, 2.0), (C,), seed)
    beta = torch.where(torch.arange(C) % 2 == 1, ints((C,), -3, 3, seed + 1), ints((C,), 290, 470, seed + 2))
    return gamma, beta


def build_forward(case):
    """Lattice inputs and exact expectations of the forward forms of a NormCase."""
    L = R.norm_lattice(case.groups, case.px, case.C, case.eps, case.seed, case.const)
    gamma, beta = affine(case.C, case.seed + 10)
    add = add_scale = add_shift = None
    if case.add:
        add = ints(L.x.shape, -4, 4, case.seed + 20)
    if case.add == 2:
        add_scale, add_shift = R.pick((0.5, 1.0, 2.0), (case.C,), case.seed + 21), ints((case.C,), -3, 3, case.seed + 22)
    scale, shift, act, exact = R.forward_expect(L, gamma, beta, case.slope, add, add_scale, add_shift)
    b = SimpleNamespace(L=L, x=L.x, gamma=gamma, beta=beta, add=add, add_scale=add_scale, add_shift=add_shift,
                        mean=L.mean, rstd=L.rstd, scale=scale, shift=shift, act=act, exact=exact, rows=None)
    if case.rows:
        b.rows = R.partial_rows(L.s1, L.s2, case.rows, case.seed + 30)
    else:
        R.direct_range_check(L.x, L.x * L.x)
    if case.running:
        g = R.gen(case.seed + 40)
        b.rm0 = torch.randn(case.C, generator=g).float()
        b.rv0 = (torch.rand(case.C, generator=g) + 0.5).float()
        b.rm, b.rv = R.running_expect(b.rm0.numpy(), b.rv0.numpy(), L.mean[0].numpy(), L.var[0].numpy(), case.px)
    return b


def build_backward(case):
    """Lattice inputs and exact expectations of the backward forms of a NormCase."""
    L = R.norm_lattice(case.groups, case.px, case.C, case.eps, case.seed, case.const)
    gamma, _ = affine(case.C, case.seed + 10)
    dz = R.lattice_dz(L, case.seed + 50)
    add = None
    if case.add:       # even integers (bf16 numbers); every other channel in [256, 512) so that dx needs rounding there
        add = 2 * ints(L.x.shape, -2, 2, case.seed + 51) + torch.where(torch.arange(case.C) % 2 == 0, 300.0, 0.0)
    E = R.backward_expect(L, dz, gamma, add)
    b = SimpleNamespace(L=L, x=L.x, dz=dz, add=add, gamma=gamma, mean=L.mean, rstd=L.rstd, E=E, rows=None)
    if case.rows:
        b.rows = R.partial_rows(E.s1, E.s2, case.rows, case.seed + 60)
    else:
        xh = (L.x - L.mean[:, None, :]) * L.rstd[:, None, :]
        R.direct_range_check(dz, dz * xh)
    return b


def build_up(case, fused):
    """Lattice inputs of the upsample family.  fused: y is a normalisation lattice and sy / ty are its rstd /
    -mean rstd; plain: integer y with dyadic sy and integer ty (sign-mixed u).  The skip's argument is >= 0."""
    N, H, W, C = case.N, case.H, case.W, case.C
    b = SimpleNamespace(s=None, ss=None, ts=None, rows=None, L=None)
    if fused:
        L = R.norm_lattice(N, H * W, C, case.eps, case.seed)
        b.L, b.y = L, L.x.view(N, H, W, C)
        b.sy, b.ty = L.rstd, -L.mean * L.rstd
        assert R.is_f32(b.ty)
        if case.rows:
            b.rows = R.partial_rows(L.s1, L.s2, case.rows, case.seed + 30)
        else:
            R.direct_range_check(L.x, L.x * L.x)
    else:
        b.y = ints((N, H, W, C), 0, 40, case.seed)
        b.sy = R.pick((0.5, 1.0, 2.0), (N, C), case.seed + 1)
        b.ty = ints((N, C), -40, 8, case.seed + 2)
    if case.skip:
        b.s = ints((N, H, W, C), -4, 4, case.seed + 3)
        b.ss = R.pick((0.5, 1.0, 2.0), (N, C), case.seed + 4)
        b.ts = ints((N, C), 8, 12, case.seed + 5)
    b.out, b.exact = R.up_forward_expect(b.y, b.sy, b.ty, b.s, b.ss, b.ts)
    return b


def build_up_bwd(case):
    """out > 0 (any positive bf16 tensor: the kernels read only its sign), integer d_out, and for the fused form a
    normalisation lattice y with its mean / rstd."""
    N, H, W, C = case.N, case.H, case.W, case.C
    b = SimpleNamespace()
    b.out = ints((N, 2 * H, 2 * W, C), 1, 9, case.seed + 6) * 0.5
    b.d_out = ints((N, 2 * H, 2 * W, C), -40, 40, case.seed + 7)
    b.du, b.exact = R.up_backward_expect(b.d_out, b.out)
    b.L = R.norm_lattice(N, H * W, C, case.eps, case.seed)
    b.y = b.L.x.view(N, H, W, C)
    # dx of the fused form, from the STORED du: the sums of bf16 numbers on a 1/32 grid are exact in fp32 (asserted), the
    # coefficients are one fp32 rounding of fp64 expressions, the two fmas round once each: k = 3
    du = b.du.reshape(N, H * W, C)
    xh = (b.L.x - b.L.mean[:, None, :]) * b.L.rstd[:, None, :]
    R.direct_range_check(du, du * xh, quantum=1.0 / 32)
    s1, s2 = R.bwd_sums(b.L.x, du, b.L.mean, b.L.rstd)
    ca, cb, cc = R.bwd_coefficients(s1, s2, H * W, None, b.L.mean, b.L.rstd)
    terms = (ca[:, None, :] * du, cb[:, None, :] * b.L.x, cc[:, None, :].expand_as(du))
    b.dx = sum(terms).reshape(N, H, W, C)
    b.dx_e = ((3 * 2.0 ** -24 + 2.0 ** -45) * sum(t.abs() for t in terms)).reshape(N, H, W, C)
    return b


# ------------------------------------------------------------------------------------------------ builders: Gaussian
def build_forward_bound(case):
    """Gaussian x (bf16 bits), non-dyadic gamma / beta.  Partial rows are the fp64 sums of `rows` contiguous runs of
    pixels rounded to fp32: one rounding per row, so terms = 1 in the summation bound; the direct form adds
    ceil(px / 32) pixels per lane in fp32."""
    g = R.gen(case.seed + 70)
    shape = (case.groups, case.px, case.C)
    x = R.gaussian_bf16(shape, case.seed + 71, 1.5, 0.5)
    gamma = (torch.randn(case.C, generator=g) * 0.5 + 1).float().double()
    beta = (torch.randn(case.C, generator=g) * 0.3).float().double()
    if case.groups > 1:
        gamma = beta = None
    b = SimpleNamespace(x=x, gamma=gamma, beta=beta, add=None, add_scale=None, add_shift=None, rows=None)
    if case.add:
        b.add = R.gaussian_bf16(shape, case.seed + 72)
    if case.add == 2:
        b.add_scale = (torch.randn(case.C, generator=g) * 0.5 + 1).float().double()
        b.add_shift = (torch.randn(case.C, generator=g) * 0.3).float().double()
    if case.rows:
        b.rows = run_sums(x, x * x, case.rows)
        b.terms = 1
    else:
        b.terms = -(-case.px // 32)
    b.mean, b.var, b.e_mean, b.e_var = R.stats_bound(x, b.terms)
    if case.running:
        b.rm0 = torch.randn(case.C, generator=g).float()
        b.rv0 = (torch.rand(case.C, generator=g) + 0.5).float()
    return b


def affine_or_identity(b, C):
    """(gamma, beta) of a built case, ones / zeros where it has none (NULL is passed to the kernels)."""
    one, zero = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    return (one if b.gamma is None else b.gamma), (zero if b.beta is None else b.beta)


def run_sums(u, v, rows):
    """[groups][rows][2][C]: fp64 sums of u / v over `rows` contiguous runs of pixels, rounded to fp32."""
    groups, px, C = u.shape
    edges = [px * i // rows for i in range(rows + 1)]
    out = torch.zeros(groups, rows, 2, C, dtype=torch.float64)
    for k, t in enumerate((u, v)):
        cs = torch.cat([torch.zeros(groups, 1, C, dtype=torch.float64), t.cumsum(1)], 1)
        out[:, :, k] = cs[:, edges[1:]] - cs[:, edges[:-1]]
    return out.float().double()


def rstd_interval(var, e_var, eps):
    """[lo, hi] of 1 / sqrt(var' + eps) over |var' - var| <= e_var, var' >= 0, widened by one fp32 rounding."""
    lo = 1.0 / torch.sqrt(var + e_var + eps)
    hi = 1.0 / torch.sqrt((var - e_var).clamp_min(0) + eps)
    return lo * (1 - 2.0 ** -24), hi * (1 + 2.0 ** -24)


def forward_bound_expect(b, case, scale, shift):
    """Teacher-forced on the kernel's published scale / shift (fp64 tensors [groups][C]): (ref, E, undecided).
    Roundings of norm_act_fused_kernel / affine_act_kernel: the fma (1); with a residual its own fma and the addition
    (3); the slope's multiplication on the negative branch (+1, counted everywhere)."""
    main = b.x * scale[:, None, :]
    mag = main.abs() + shift.abs()[:, None, :]
    k = 2
    if b.add is not None:
        asc = 1.0 if b.add_scale is None else b.add_scale[None, None, :]
        ash = 0.0 if b.add_shift is None else b.add_shift[None, None, :]
        mag = mag + (b.add * asc).abs() + abs(ash)
        k = 4
    arg = R.forward_arg(b.x, scale, shift, b.add, b.add_scale, b.add_shift)
    e = k * 2.0 ** -24 * mag
    slope = float(torch.tensor(case.slope, dtype=torch.float32))
    return R.lrelu(arg, slope), e, R.undecided(arg, e)


def build_backward_bound(case):
    """Gaussian dz / x; mean / rstd are fp32 inputs of the backward (the fp64 statistics of x rounded once).  Sums over
    fp32 rows (terms = 1) or per-lane (ceil(px / 32), each term one more rounding for xhat and one for the product
    being fused or not: covered by the + 4 of summation_bound)."""
    g = R.gen(case.seed + 80)
    shape = (case.groups, case.px, case.C)
    x = R.gaussian_bf16(shape, case.seed + 81, 1.5, 0.5)
    dz = R.gaussian_bf16(shape, case.seed + 82)
    gamma = None if case.groups > 1 else (torch.randn(case.C, generator=g) * 0.5 + 1).float().double()
    mean = (x.sum(1) / case.px).float().double()
    var = (x * x).sum(1) / case.px - (x.sum(1) / case.px) ** 2
    rstd = (1.0 / torch.sqrt(var.clamp_min(0) + case.eps)).float().double()
    b = SimpleNamespace(x=x, dz=dz, gamma=gamma, mean=mean, rstd=rstd, add=None, rows=None)
    if case.add:
        b.add = R.gaussian_bf16(shape, case.seed + 83)
    xh = (x - mean[:, None, :]) * rstd[:, None, :]
    if case.rows:
        b.rows = run_sums(dz, dz * xh, case.rows)
        terms, extra = 1, 0.0
    else:
        # per lane: xhat = (x - mean) * rstd rounds twice before the fma: 2^-23 of each |dz xhat| on top of the sum's own
        terms, extra = -(-case.px // 32), 2.0 ** -23 * (dz * xh).abs().sum(1)
    b.s1, b.s2 = dz.sum(1), (dz * xh).sum(1)
    b.e1 = R.summation_bound(terms, dz.abs().sum(1))
    b.e2 = R.summation_bound(terms, (dz * xh).abs().sum(1)) + extra
    return b


def backward_bound_expect(b, case, ca=None, cb=None, cc=None):
    """(ref dx, E).  With the kernel's published ca / cb / cc (the chain): teacher-forced, two fmas and the residual's
    addition (k = 3).  Without (the fused form publishes none): the fp64 coefficients, their error from the sums'
    bounds e1 / e2 and one fp32 rounding each, then the same three roundings."""
    n = case.px
    if ca is None:
        ca, cb, cc = R.bwd_coefficients(b.s1, b.s2, n, b.gamma, b.mean, b.rstd)
        gr = ca.abs()
        d_cb = gr * b.rstd * b.e2 / n + 2.0 ** -24 * cb.abs()
        d_cc = gr * ((b.mean * b.rstd).abs() * b.e2 / n + b.e1 / n) + 2.0 ** -24 * cc.abs() + 2.0 ** -24 * gr * (
            (b.mean * b.rstd * b.s2 / n).abs() + (b.s1 / n).abs())
        d_ca = 2.0 ** -24 * ca.abs()
    else:
        d_ca = d_cb = d_cc = torch.zeros_like(ca)
    t1, t2, t3 = ca[:, None, :] * b.dz, cb[:, None, :] * b.x, cc[:, None, :]
    ref = t1 + t2 + t3
    mag = t1.abs() + t2.abs() + t3.abs()
    e = d_ca[:, None, :] * b.dz.abs() + d_cb[:, None, :] * b.x.abs() + d_cc[:, None, :]
    if b.add is not None:
        ref, mag = ref + b.add, mag + b.add.abs()
    return ref, e + 3 * 2.0 ** -24 * mag


def build_up_bound(case):
    """Gaussian y / s with Gaussian tables: sign-mixed LeakyReLU arguments at the hard-coded 0.2 slope."""
    N, H, W, C = case.N, case.H, case.W, case.C
    g = R.gen(case.seed + 90)
    b = SimpleNamespace(s=None, ss=None, ts=None)
    b.y = R.gaussian_bf16((N, H, W, C), case.seed + 91, 1.5, 0.5)
    b.sy = (torch.randn(N, C, generator=g) * 0.5 + 1).float().double()
    b.ty = (torch.randn(N, C, generator=g) * 0.3).float().double()
    if case.skip:
        b.s = R.gaussian_bf16((N, H, W, C), case.seed + 92)
        b.ss = (torch.randn(N, C, generator=g) * 0.5 + 1).float().double()
        b.ts = (torch.randn(N, C, generator=g) * 0.3).float().double()
    b.d_out = R.gaussian_bf16((N, 2 * H, 2 * W, C), case.seed + 93)
    return b


def up_forward_bound_expect(b, sy, ty):
    """(ref out, E, undecided) for the given sy / ty (the caller's tables, or the fused kernel's published ones).
    Roundings of u_value / u_at: the fma (1), the skip's fma (1), its slope (1), the addition (1): e_u = 4 2^-24 of the
    magnitudes; an element of s whose argument is within its own rounding of zero may take either branch: the two
    differ by 0.8 |q| <= 0.8 2^-24 |terms of q|, added to e_u.  The blend rounds 7 times (4 products, 3 sums; fewer
    when contracted) and the final slope once: E = up2x(e_u) + 8 2^-24 up2x(|u|)."""
    tab = lambda t: t.double()[:, None, None, :]
    u, q = R.up_u(b.y, sy, ty, b.s, b.ss, b.ts)
    mag = (b.y * tab(sy)).abs() + tab(ty).abs()
    if q is not None:
        qmag = (b.s * tab(b.ss)).abs() + tab(b.ts).abs()
        mag = mag + qmag
    e_u = 4 * 2.0 ** -24 * mag + (0.8 * 2.0 ** -24 * qmag if q is not None else 0.0)
    v = R.up2x(u)
    e = R.up2x(e_u) + 8 * 2.0 ** -24 * R.up2x(u.abs())
    return R.lrelu(v, R.F32_02), e, R.undecided(v, e)


def up_backward_bound_expect(d_out, out):
    """(ref du, E): sixteen taps at most, each a product weight * slope (1 rounding) and an fma (1): 32 2^-24 of the
    adjoint of |d_out lrelu'|."""
    d = d_out * torch.where(out > 0, 1.0, R.F32_02)
    return R.up2x_adjoint(d), 32 * 2.0 ** -24 * R.up2x_adjoint(d.abs())
