"""Exact and element-wise references for the normalisation kernels (csrc/norm.hip) and the UNet decoder glue
(csrc/elementwise.hip): plain fp64 on the CPU, no project code.  The shared pieces (guard bands, bf16 roundings, the
summation bound, the comparisons) come from conv_exact_ref.

Tensors here are fp64 on the CPU in the kernels' own layouts: [groups][pixels][C] for the normalisation family,
[N][H][W][C] for the upsample family, [groups][C] / [C] for the tables, [groups][rows][2][C] for partial rows.

Lattice data.  Per (group, channel) x = m + a t with an integer m, a in {0.5, 1, 2} and integers t with sum t = 0 and
sum t^2 / count = v in {1/4, 1, 4} (3/4 with eps = 0.25; 0 for a constant channel).  Then mean = m, var = a^2 v,
var + eps is a power of four, rstd a power of two, and with dyadic gamma and integer beta every published number and
every argument of the activation is an fp32 number whatever the order of the sums; the stored bf16 must EQUAL
RNE_bf16(exact).  t stays in {-2 .. 2} for even counts; an odd count has no such t with a dyadic variance (sum t^2 is
even when sum t = 0, so count v must be even), so odd counts take v = 4 with t in {-3 .. 3}.  Every builder asserts its
conditions (is_f32 / range_check): they are conditions on the inputs, not tolerances.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from conv_exact_ref import (_PATTERN, SLACK, TWO24, Guarded, assert_not_vacuous, assert_within_bound, bf16, gen,  # noqa: F401
                            half_away_bf16, half_ulp_bf16, is_bf16, is_f32, is_multiple, pick, range_check,
                            report_mismatch, rne_bf16, summation_bound, tie_share, trunc_bf16)

_PATTERN.setdefault(torch.int64, (torch.int64, 0x5A5A5A5A5A5A5A5A))     # num_batches_tracked gets guard bands too
F32_02 = float(np.float32(0.2))          # the slope the upsample kernels hard-code, as the fp32 number it is
MOMENTUM = float(np.float32(0.1))


# ------------------------------------------------------------------------------------------------ lattice
def t_pairs(px, v4):
    """(p1, p2, p3): numbers of +-1, +-2, +-3 pairs with sum t^2 = (v4 / 4) px inside px pixels, or None.  p3 is kept as
    small as possible (0 for every even count) and the +-2 pairs take about half of what +-1 could."""
    if px < 2 or (v4 * px) % 8:
        return None
    half, cap = v4 * px // 8, px // 2             # p1 + 4 p2 + 9 p3 = half, p1 + p2 + p3 <= cap
    for p3 in range(0, min(cap, 64) + 1):
        rest = half - 9 * p3
        if rest < 0:
            break
        lo = max(0, -((cap - p3 - rest) // 3))    # p1 + p2 = rest - 3 p2 <= cap - p3
        if 4 * lo <= rest:
            p2 = (lo + rest // 4) // 2 if p3 == 0 else lo
            return rest - 4 * p2, p2, p3
    return None


def t_vector(px, v4):
    """(t, r): px integers with sum t = 0, sum t^2 = (v4 / 4) px, and r in {-1, 0, 1} with +1 / -1 on pairs of pixels
    of equal t (sum r = 0, sum r t = 0).  v4 = 0: the constant channel.  None where no such t exists."""
    if v4 == 0:
        pairs = (0, 0, 0)
    else:
        pairs = t_pairs(px, v4)
        if pairs is None:
            return None
    t, r = [], []
    for k, p in zip((1, 2, 3), pairs):
        for sign in (k, -k):
            t += [sign] * p
            r += [1, -1] * (p // 2) + [0] * (p % 2)
    zeros = px - len(t)
    t += [0] * zeros
    r += [1, -1] * (zeros // 2) + [0] * (zeros % 2)
    t, r = torch.tensor(t, dtype=torch.float64), torch.tensor(r, dtype=torch.float64)
    assert t.numel() == px and float(t.sum()) == 0 and float((t * t).sum()) * 4 == v4 * px
    assert float(r.sum()) == 0 and float((r * t).sum()) == 0
    return t, r


def choices(px, eps):
    """The (a, v4) pairs a channel may take at this count and eps: var + eps = a^2 v4 / 4 + eps a power of four."""
    out = []
    for a in (0.5, 1.0, 2.0):
        for v4 in (1, 3, 4, 16):
            s = a * a * v4 / 4 + eps
            e = math.log2(s)
            if e == round(e) and round(e) % 2 == 0 and t_vector(px, v4) is not None:
                out.append((a, v4))
    return out


def norm_lattice(groups, px, C, eps, seed, const=(), m_lim=3):
    """x [groups][px][C] = m + a t on the lattice, with everything the expectations need.  `const`: channels that are
    constant (t = 0; needs eps > 0).  Returns a namespace: x, t, r, m, a, v (all [groups][C] but x, t, r), mean, var,
    rstd, eps, count."""
    g = gen(seed)
    opts = choices(px, eps)
    if not opts:
        assert eps > 0, "no lattice at %d pixels with eps = 0" % px
        opts = []
    base = {v4: t_vector(px, v4) for v4 in set([o[1] for o in opts] + [0])}
    perm = torch.randperm(px, generator=g)
    x = torch.empty(groups, px, C, dtype=torch.float64)
    t, r = torch.empty_like(x), torch.empty_like(x)
    m = torch.randint(-m_lim, m_lim + 1, (groups, C), generator=g).double()
    a, v = torch.ones(groups, C, dtype=torch.float64), torch.zeros(groups, C, dtype=torch.float64)
    for gi in range(groups):
        for c in range(C):
            dead = c in const or not opts
            ai, v4 = (1.0, 0) if dead else opts[int(torch.randint(0, len(opts), (1,), generator=g))]
            roll = int(torch.randint(0, px, (1,), generator=g))
            sign = 1.0 if int(torch.randint(0, 2, (1,), generator=g)) else -1.0
            bt, br = base[v4]
            t[gi, :, c] = sign * torch.roll(bt[perm], roll)
            r[gi, :, c] = torch.roll(br[perm], roll)
            a[gi, c], v[gi, c] = ai, v4 / 4
    x = m[:, None, :] + a[:, None, :] * t
    var = a * a * v
    assert eps > 0 or bool((var > 0).all()), "a constant channel needs eps > 0"
    rstd = 1.0 / torch.sqrt(var + eps)
    assert bool((torch.log2(rstd) == torch.log2(rstd).round()).all()), "rstd is not a power of two"
    assert is_bf16(x), "x is not a bf16 number"
    # the sums themselves, in fp64 (exact: dyadic terms far below 2^53), must give mean and var back exactly
    s1, s2 = x.sum(1), (x * x).sum(1)
    assert torch.equal(s1 / px, m) and torch.equal(s2 / px - m * m, var)
    return SimpleNamespace(x=x, t=t, r=r, m=m, a=a, v=v, mean=m, var=var, rstd=rstd, eps=eps, count=px, s1=s1, s2=s2,
                           groups=groups, C=C)


def direct_range_check(*terms, quantum=1.0 / 16):
    """Direct form: a lane adds its pixels in fp32.  sum |term| over the whole group below 2^24 quanta keeps every
    partial sum of every split exact."""
    for term in terms:
        assert is_multiple(term, quantum)
        range_check(term.abs().sum(1), quantum, "per-group sum of the direct form's terms")


def partial_rows(tot1, tot2, rows, seed, stage_rows=64):
    """[groups][rows][2][C] fp64 rows for the totals tot1 / tot2 ([groups][C]): integer-valued, all different within a
    column, the last one = total - the rest.  Asserted: every row an fp32 number, and so is every stage-1 slice sum
    (ceil(rows / 64) consecutive rows), so the fp64 row sums of the kernels and the fp32 stage-1 array are exact."""
    g = gen(seed)
    groups, C = tot1.shape
    out = torch.empty(groups, rows, 2, C, dtype=torch.float64)
    for k, tot in enumerate((tot1, tot2)):
        if rows > 1:
            order = torch.argsort(torch.rand(groups, rows - 1, C, generator=g), dim=1).double()
            centre = torch.floor(tot / rows)[:, None, :]
            out[:, :-1, k] = centre + (order - (rows - 2) // 2) * (3 + 2 * k)      # distinct integers around total / rows
        out[:, -1, k] = tot - out[:, :-1, k].sum(1)
    assert torch.equal(out[:, :, 0].sum(1), tot1) and torch.equal(out[:, :, 1].sum(1), tot2)
    assert is_f32(out), "a partial row is not an fp32 number"
    assert not bool(torch.isnan(out).any())
    if rows > 2:
        body = out[:, :-1]
        assert bool((body.sort(dim=1).values.diff(dim=1) != 0).all()), "partial rows repeat"
    per = -(-rows // stage_rows)
    pad = torch.zeros(groups, per * stage_rows, 2, C, dtype=torch.float64)
    pad[:, :rows] = out
    assert is_f32(pad.view(groups, stage_rows, per, 2, C).sum(2)), "a stage-1 slice sum is not an fp32 number"
    return out


# ------------------------------------------------------------------------------------------------ forward
def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def norm_tables(L, gamma, beta):
    """scale / shift [groups][C] from the exact statistics; gamma / beta [C] or None."""
    gm = torch.ones(L.C, dtype=torch.float64) if gamma is None else gamma.double()
    bt = torch.zeros(L.C, dtype=torch.float64) if beta is None else beta.double()
    scale = gm[None] * L.rstd
    shift = bt[None] - L.mean * gm[None] * L.rstd
    for name, tab in (("mean", L.mean), ("rstd", L.rstd), ("scale", scale), ("shift", shift)):
        assert is_f32(tab), name + " is not an fp32 number"
    return scale, shift


def forward_arg(x, scale, shift, add=None, add_scale=None, add_shift=None):
    """x scale + shift [+ add add_scale + add_shift] in fp64: the argument of the activation."""
    v = x * scale[:, None, :] + shift[:, None, :]
    if add is not None:
        asc = 1.0 if add_scale is None else add_scale.double()[None, None, :]
        ash = 0.0 if add_shift is None else add_shift.double()[None, None, :]
        v = v + (add * asc + ash)
    return v


def forward_expect(L, gamma, beta, slope, add=None, add_scale=None, add_shift=None):
    """(scale, shift, act): act = RNE_bf16(lrelu(arg)), every intermediate asserted an fp32 number."""
    scale, shift = norm_tables(L, gamma, beta)
    assert is_f32(L.x * scale[:, None, :] + shift[:, None, :])
    if add is not None:
        assert is_bf16(add) and is_f32(forward_arg(torch.zeros_like(add), scale * 0, shift * 0, add, add_scale, add_shift))
    arg = forward_arg(L.x, scale, shift, add, add_scale, add_shift)
    assert is_f32(arg)
    v = lrelu(arg, slope)
    return scale, shift, rne_bf16(v), v


def running_expect(rm, rv, mean, var, count, momentum=MOMENTUM):
    """The kernels' running-statistics expression in numpy float64, rounded to float32: rm / rv float32 [C] before the
    launch, mean / var the batch statistics (fp64).  The unbiased variance uses count - 1 only where count > 1."""
    rm64, rv64 = np.asarray(rm, dtype=np.float32).astype(np.float64), np.asarray(rv, dtype=np.float32).astype(np.float64)
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    cnt = float(np.float32(count))
    unb = var * cnt / (cnt - 1.0) if cnt > 1.0 else var
    return (((1.0 - momentum) * rm64 + momentum * mean).astype(np.float32),
            ((1.0 - momentum) * rv64 + momentum * unb).astype(np.float32))


def assert_within_ulps(got, exp, ulps, name):
    """fp32 arrays: |got - exp| <= ulps spacings of exp (np.spacing), NaN never passes."""
    got, exp = np.asarray(got, dtype=np.float32), np.asarray(exp, dtype=np.float32)
    ok = np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= ulps * np.spacing(np.abs(exp)).astype(np.float64)
    assert ok.all(), "%s: %d of %d beyond %d ulp, first at %s: got %r expected %r" % (
        name, int((~ok).sum()), ok.size, ulps, np.argwhere(~ok)[0], got[~ok][0], exp[~ok][0])


# ------------------------------------------------------------------------------------------------ backward
def lattice_dz(L, seed, k_lim=2):
    """dz = k1 + k2 t + q r per (group, channel), integers: sum dz = k1 count and sum dz xhat = k2 a rstd sum t^2."""
    g = gen(seed)
    shape = (L.groups, L.C)
    k1 = torch.randint(-k_lim, k_lim + 1, shape, generator=g).double()
    k2 = torch.randint(-k_lim, k_lim + 1, shape, generator=g).double()
    q = torch.randint(1, 3, shape, generator=g).double()
    dz = k1[:, None, :] + k2[:, None, :] * L.t + q[:, None, :] * L.r
    assert is_bf16(dz)
    return dz


def bwd_sums(x, dz, mean, rstd):
    """(sum dz, sum dz xhat) [groups][C] in fp64, xhat = (x - mean) rstd."""
    xh = (x - mean[:, None, :]) * rstd[:, None, :]
    return dz.sum(1), (dz * xh).sum(1)


def bwd_coefficients(s1, s2, count, gamma, mean, rstd):
    """ca, cb, cc [groups][C]: dx = ca dz + cb x + cc is the normalisation's input gradient."""
    gm = 1.0 if gamma is None else gamma.double()[None]
    m1, m2 = s1 / count, s2 / count
    return gm * rstd, -gm * rstd * rstd * m2, gm * rstd * (mean * rstd * m2 - m1)


def backward_expect(L, dz, gamma, add=None):
    """(ca, cb, cc, dgamma, dbeta, dx, exact dx): all asserted fp32 numbers; dgamma / dbeta are the sums over ALL groups'
    pixels only when there is one group (the kernels refuse them otherwise)."""
    s1, s2 = bwd_sums(L.x, dz, L.mean, L.rstd)
    ca, cb, cc = bwd_coefficients(s1, s2, L.count, gamma, L.mean, L.rstd)
    for name, tab in (("ca", ca), ("cb", cb), ("cc", cc), ("sum dz", s1), ("sum dz xhat", s2)):
        assert is_f32(tab), name + " is not an fp32 number"
    inner = cb[:, None, :] * L.x + cc[:, None, :]
    assert is_f32(inner)
    v = ca[:, None, :] * dz + inner
    assert is_f32(v)
    if add is not None:
        assert is_bf16(add)
        v = v + add
        assert is_f32(v)
    return SimpleNamespace(ca=ca, cb=cb, cc=cc, dgamma=s2[0], dbeta=s1[0], dx=rne_bf16(v), exact=v, s1=s1, s2=s2)


# ------------------------------------------------------------------------------------------------ upsample
def up_matrix(n):
    """[2n][n] fp64: the 2x bilinear upsample of nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)
    along one axis: out[2i] = .25 u[max(i - 1, 0)] + .75 u[i], out[2i + 1] = .75 u[i] + .25 u[min(i + 1, n - 1)]."""
    m = torch.zeros(2 * n, n, dtype=torch.float64)
    for i in range(n):
        m[2 * i, max(i - 1, 0)] += 0.25
        m[2 * i, i] += 0.75
        m[2 * i + 1, i] += 0.75
        m[2 * i + 1, min(i + 1, n - 1)] += 0.25
    return m


def up2x(u):
    """[N][H][W][C] -> [N][2H][2W][C]."""
    return torch.einsum("ph,nhwc,qw->npqc", up_matrix(u.shape[1]), u.double(), up_matrix(u.shape[2]))


def up2x_adjoint(d):
    """[N][2H][2W][C] -> [N][H][W][C]: the transpose of up2x."""
    return torch.einsum("ph,npqc,qw->nhwc", up_matrix(d.shape[1] // 2), d.double(), up_matrix(d.shape[2] // 2))


def lrelu02_f32(v):
    """v > 0 ? v : 0.2f * v as the device computes it from an fp32 v: ONE fp32 rounding of the exact product."""
    assert is_f32(v)
    return torch.where(v > 0, v, (v * F32_02).float().double())


def up_u(y, sy, ty, s=None, ss=None, ts=None):
    """u = y sy + ty [+ lrelu_0.2(s ss + ts)] in fp64 (tables [N][C]); returns (u, q) with q the skip's argument."""
    tab = lambda t: t.double()[:, None, None, :]
    u = y * tab(sy) + tab(ty)
    q = None
    if s is not None:
        q = s * tab(ss) + tab(ts)
        u = u + lrelu(q, F32_02)
    return u, q


def up_forward_expect(y, sy, ty, s=None, ss=None, ts=None):
    """Lattice: the skip's argument is >= 0 (asserted) and u a small multiple of 1/2, so the blend with 1/16 weights is
    exact in any association; the final LeakyReLU's negative branch is one fp32 rounding of 0.2f v.  Returns
    (stored out, exact blend)."""
    u, q = up_u(y, sy, ty, s, ss, ts)
    assert q is None or bool((q >= 0).all()), "the skip's LeakyReLU argument must not be negative on the lattice"
    assert is_multiple(u, 0.5) and float(u.abs().max()) < 2.0 ** 15
    v = up2x(u)
    assert is_f32(v)
    return rne_bf16(lrelu02_f32(v)), v


def up_backward_expect(d_out, out):
    """du = RNE_bf16(adjoint_up(d_out lrelu'(out))); on the lattice out > 0 everywhere (asserted), d_out integers."""
    assert bool((out > 0).all()), "out must be positive on the lattice (the 0.2 slope is not dyadic)"
    assert is_multiple(d_out, 1.0) and float(d_out.abs().max()) < 2.0 ** 12
    v = up2x_adjoint(d_out)
    assert is_f32(v)
    return rne_bf16(v), v


# ------------------------------------------------------------------------------------------------ bound mode
def gaussian_bf16(shape, seed, scale=1.0, shift=0.0):
    """Gaussian data as the bf16 numbers the kernels read, in fp64."""
    return (torch.randn(tuple(shape), generator=gen(seed), dtype=torch.float64) * scale + shift).to(bf16).double()


def stats_bound(x, terms):
    """(mean, var, E_mean, E_var) [groups][C] in fp64 over the same bf16 bits.  E1 / E2 = summation_bound(terms, sum |x|
    / sum x^2): |mean - ref| <= E1 / count, |var - ref| <= (E2 + 2 |mean| E1) / count + (E1 / count)^2."""
    n = x.shape[1]
    mean = x.sum(1) / n
    var = ((x * x).sum(1) / n - mean * mean).clamp_min(0)
    e1, e2 = summation_bound(terms, x.abs().sum(1)), summation_bound(terms, (x * x).sum(1))
    return mean, var, e1 / n, (e2 + 2 * mean.abs() * e1) / n + (e1 / n) ** 2      # (the last term: second order, kept)


def undecided(arg, e):
    """Elements whose LeakyReLU argument lies within its own error of zero: they may take either branch."""
    return arg.abs() <= e


def assert_elementwise(got, ref, e, name, exclude=None, stored_bf16=True):
    """|got - ref| <= half_ulp_bf16(|ref| + E) + E with an explicit per-element E (assert_within_bound with the
    summation bound already evaluated: terms + 4 = 1, mag = E 2^24).  For a bf16 output the ratio that
    assert_within_bound prints is ruled by the half ulp (some element of thousands sits next to a tie), so the share of
    E that the worst element uses, (|err| - half ulp) / E, is printed too: documentation, not a criterion."""
    if stored_bf16:
        over = ((got.double() - ref).abs() - half_ulp_bf16(ref.abs() + e)) / e.clamp_min(1e-300)
        if exclude is not None:
            over = over[~exclude]
        print("%s: worst (|err| - half ulp) / E = %.3f" % (name, float(over.max())))
    assert_within_bound(got, ref, e * TWO24, -3, name, stored_bf16=stored_bf16, exclude=exclude)
