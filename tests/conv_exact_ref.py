"""Exact and element-wise references for the convolution kernels: plain torch on the CPU in fp64, no project code.

Lattice data.  Inputs are small integers (wide lattice: [-4, 4]; narrow: [-1, 1]) and the prologue / epilogue
parameters are dyadic (integer bias, shifts and residuals, scales in {+-0.5, +-1, +-2}, slopes in {0, 0.25, 0.5}).
Every bf16 product is then exact in fp32 and the MFMA accumulates as an fp32 fmaf chain, so as long as
sum |x||w| + |bias| + |residuals| stays below 2^24 quanta for an output, EVERY summation order, split, atomic
order and tiling gives the same exact number.  The range condition is asserted on the inputs (range_check); it is
not a tolerance.  The expected stored value is RNE_bf16(exact): on the wide lattice the odd integers of
[256, 512) are exact ties between bf16 neighbours, so the same expectation pins the rounding mode and catches a
second rounding.

Tensors here are logical NCHW fp64 on the CPU (the tests' nhwc() convention turns them into what the kernels
read); tables are [K] (per channel) or [N][K] (per image and channel).
"""
import torch
import torch.nn.functional as F

bf16 = torch.bfloat16
TWO24 = float(1 << 24)
SLACK = 4096                    # guard elements in front of and behind a carved tensor (16-byte aligned for every dtype)
SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lattice(shape, lim, seed):
    """fp64 integers in [-lim, lim]."""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=gen(seed)).double()


def pick(values, shape, seed):
    """fp64 tensor of `shape` drawn from the list `values`."""
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=gen(seed))]


def table(t):
    """[K] or [N][K] table -> broadcastable against NCHW."""
    return t.view(1, -1, 1, 1) if t.dim() == 1 else t.view(t.shape[0], t.shape[1], 1, 1)


def is_f32(v):
    return bool((v.float().double() == v).all())


def is_bf16(v):
    return bool((v.to(bf16).double() == v).all())


def rne_bf16(v):
    """fp64 -> fp32 (asserted exact) -> bf16 round-to-nearest-even, back as fp64."""
    assert is_f32(v), "value not representable in fp32: the lattice condition is broken"
    return v.float().to(bf16).double()


def trunc_bf16(v):
    """Round towards zero to bf16 (what a kernel that drops the low 16 bits stores)."""
    bits = v.float().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


def half_away_bf16(v):
    """Round to nearest, ties away from zero."""
    f = v.float()
    bits = f.abs().view(torch.int32) + 0x8000
    return (torch.sign(f) * (bits & ~0xFFFF).view(torch.float32)).double()


def range_check(abs_sum, quantum=1.0, what="sum |x||w|"):
    """The lattice condition: abs_sum (every term a multiple of quantum) below 2^24 quanta everywhere, so that every
    partial sum in every order is an exact fp32 number.  Returns the largest value seen."""
    top = float(abs_sum.max())
    assert top / quantum < TWO24, "%s = %g exceeds 2^24 quanta of %g" % (what, top, quantum)
    return top


def is_multiple(v, quantum):
    return bool(((v / quantum).round() * quantum == v).all())


# ------------------------------------------------------------------------------------------------ convolutions
def conv_fwd(x, w, stride, pad):
    return F.conv2d(x.double(), w.double(), stride=stride, padding=pad)


def conv_dgrad(dy, w, in_hw, stride, pad):
    n, (k, c) = dy.shape[0], w.shape[:2]
    return torch.nn.grad.conv2d_input((n, c, in_hw, in_hw), w.double(), dy.double(), stride=stride, padding=pad)


def conv_wgrad(x, dy, k, r, stride, pad):
    """fp64 weight gradient in the kernels' [K][R*S][C] order."""
    c = x.shape[1]
    g = torch.nn.grad.conv2d_weight(x.double(), (k, c, r, r), dy.double(), stride=stride, padding=pad)
    return g.permute(0, 2, 3, 1).reshape(k, r * r, c).contiguous()


def conv_abs(src, w, mode, in_hw, stride, pad):
    """sum |src||w| of every output.  fp32 is enough: the sum is monotone, so a result below 2^24 quanta had every
    partial sum below it and is exact (range_check asserts the result)."""
    s, ww = src.abs().float(), w.abs().float()
    if mode == 0:
        return F.conv2d(s, ww, stride=stride, padding=pad).double()
    n, c = s.shape[0], ww.shape[1]
    return torch.nn.grad.conv2d_input((n, c, in_hw, in_hw), ww, s, stride=stride, padding=pad).double()


def wgrad_abs(x, dy, k, r, stride, pad):
    c = x.shape[1]
    g = torch.nn.grad.conv2d_weight(x.abs().float(), (k, c, r, r), dy.abs().float(), stride=stride, padding=pad)
    return g.permute(0, 2, 3, 1).reshape(k, r * r, c).double()


def prologue(x, scale, shift, act, slope):
    """combat_conv_args.pro_*: v = fma(x, scale, shift) in fp32, leaky activation in fp32, bf16 operand.  On lattice
    data every step is exact (asserted); on other data this is the kernels' documented arithmetic restated."""
    v = x.double()
    if scale is not None:
        v = (v * table(scale).double() + table(shift).double()).float().double()     # one fp32 rounding: fmaf
    if act:
        v = torch.where(v > 0, v, (v.float() * torch.tensor(slope, dtype=torch.float32)).double())
    return v.float().to(bf16).double()


def lattice_prologue(x, scale, shift, act, slope):
    """The same with every step asserted exact; returns the activated operand (exactly a bf16 number)."""
    v = x.double()
    if scale is not None:
        v = v * table(scale).double() + table(shift).double()
    if act:
        v = torch.where(v > 0, v, v * slope)
    assert is_bf16(v), "activated operand is not a bf16 number: the lattice condition is broken"
    return v


def epilogue(acc, *, bias=None, add_pre=None, mask_x=None, mask_scale=None, mask_shift=None, mask_activated=False,
             mask_slope=0.0, mask_mul_scale=False, add_post=None, exact=True):
    """combat_conv_args' epilogue in the header's order on the exact accumulator `acc` (fp64 NCHW): bias, add_pre,
    mask, mask_mul_scale, add_post.  Returns (v, abs_terms, q): the value BEFORE the one rounding, the sum of the
    magnitudes that entered it beside the reduction (|bias| + |add_pre| + |add_post|), and the mask argument (None
    without a mask).  exact=True asserts that every intermediate is an fp32 number (lattice data)."""
    v = acc.double()
    mag = torch.zeros_like(v)
    q = None

    def step(t):
        if exact:
            assert is_f32(t), "epilogue intermediate not representable in fp32: the lattice condition is broken"
        return t

    if bias is not None:
        v = step(v + table(bias).double())
        mag = mag + table(bias).double().abs()
    if add_pre is not None:
        v = step(v + add_pre.double())
        mag = mag + add_pre.double().abs()
    if mask_x is not None:
        if mask_scale is not None and not mask_activated:
            q = mask_x.double() * table(mask_scale).double() + table(mask_shift).double()
            if not exact:
                q = q.float().double()
        else:
            q = mask_x.double()
        d = torch.where(q > 0, torch.ones_like(q), torch.full_like(q, mask_slope))
        if mask_mul_scale:
            d = d * table(mask_scale).double()
        v = step(v * d)
    if add_post is not None:
        v = step(v + add_post.double())
        mag = mag + add_post.double().abs()
    return v, mag, q


def activated(y, scale, shift, slope):
    """act_dst from the STORED value y: bf16(lrelu(fma(y, scale, shift), slope)); exact fp64 then one rounding."""
    t = y.double() * table(scale).double() + table(shift).double()
    t = torch.where(t > 0, t, t * slope)
    return rne_bf16(t)


def stats_totals(y, kind, mask_x=None, xh_mean=None, xh_rstd=None, quantum=1.0):
    """Exact per-(image, channel) statistics of the stored tensor y (NCHW fp64): [N][2][K] = (sum y, sum y*y) for
    kind 1, (sum y, sum y*xh), xh = (mask_x - mean) * rstd, for kind 2.  Asserts that every term is a multiple of
    `quantum` and that the per-channel sum of magnitudes over the WHOLE tensor stays below 2^24 quanta: every row of
    the statistics array, in any grouping, is then an exact fp32 number."""
    second = y * y if kind == 1 else y * ((mask_x.double() - table(xh_mean).double()) * table(xh_rstd).double())
    out = []
    for t in (y, second):
        assert is_multiple(t, quantum), "statistics term off the lattice"
        range_check(t.abs().sum((0, 2, 3)), quantum, "per-channel sum of statistics terms")
        out.append(t.sum((2, 3)))
    return torch.stack(out, 1)


def tie_share(v):
    """Share of the exact values that are NOT bf16 numbers (each is then rounded: on integer data below 512 these
    are exact ties)."""
    return float((v.float().to(bf16).double() != v).double().mean())


def assert_not_vacuous(v, what=""):
    share = tie_share(v)
    assert share >= 0.02, "%s: only %.2f %% of the expected outputs need rounding: the case is vacuous" % (what, 100 * share)
    return share


# ------------------------------------------------------------------------------------------------ guard bands
_PATTERN = {torch.bfloat16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A),
            torch.uint8: (torch.uint8, 0x5A)}


class Guarded:
    """A tensor carved out of a larger 1-D buffer with SLACK elements in front of and behind it.  role 'dst': the
    whole buffer holds a fixed bit pattern (the interior too, unless `zero`) and check() verifies, comparing integers,
    that the bands still hold it.  role 'src': the bands hold NaN (a row past the end that reaches an output shows)."""

    def __init__(self, shape, dtype, role, device, zero=False):
        numel = 1
        for s in shape:
            numel *= int(s)
        self.role, self.numel, self.dtype = role, numel, dtype
        self.buf = torch.empty(numel + 2 * SLACK, dtype=dtype, device=device)
        if role == "dst":
            it, pat = _PATTERN[dtype]
            self.buf.view(it).fill_(pat)
        else:
            assert dtype.is_floating_point
            self.buf.fill_(float("nan"))
        self.t = self.buf[SLACK:SLACK + numel].view(tuple(shape))
        if zero:
            self.t.zero_()
        assert self.t.data_ptr() % 16 == 0

    @classmethod
    def source(cls, value, device):
        g = cls(value.shape, value.dtype, "src", device)
        g.t.copy_(value)
        return g

    def bands(self):
        it, _ = _PATTERN[self.dtype]
        b = self.buf.view(it)
        return b[:SLACK], b[SLACK + self.numel:]

    def check(self, name):
        """Destination bands untouched (integers compared).  Returns nothing; raises AssertionError naming the band."""
        if self.role != "dst":
            return
        _, pat = _PATTERN[self.dtype]
        for side, band in zip(("before", "after"), self.bands()):
            bad = (band != pat).nonzero().flatten().cpu()
            if bad.numel():
                first = [int(i) for i in bad[:4]]
                off = [i - SLACK for i in first] if side == "before" else first
                raise AssertionError("guard band %s %s was written: %d elements, first at offsets %s from the tensor's %s"
                                     % (side, name, bad.numel(), off, "start" if side == "before" else "end"))


# ------------------------------------------------------------------------------------------------ comparison
def report_mismatch(got, exp, name, tile=None, limit=6):
    """got / exp: NCHW tensors on the CPU, compared as VALUES (-0 == +0; a NaN in got never equals).  Raises an
    AssertionError with the number of wrong elements, the first (image, y, x, channel) coordinates with got /
    expected, and the picked tile id."""
    got, exp = got.double(), exp.double()
    assert got.shape == exp.shape, (name, tuple(got.shape), tuple(exp.shape))
    bad = (got != exp)
    count = int(bad.sum())
    if not count:
        return
    idx = bad.nonzero()[:limit]
    lines = []
    for i in idx:
        c = [int(v) for v in i]
        where = (c[0], c[2], c[3], c[1]) if len(c) == 4 else tuple(c)
        lines.append("%s got %r expected %r" % (where, float(got[tuple(c)]), float(exp[tuple(c)])))
    nan = int(torch.isnan(got).sum())
    kind = "(image, y, x, channel)" if got.dim() == 4 else "index"
    raise AssertionError("%s: %d of %d elements wrong (%d NaN), tile %s; first %s:\n  %s"
                         % (name, count, got.numel(), nan, tile, kind, "\n  ".join(lines)))


# ------------------------------------------------------------------------------------------------ element-wise bound
def summation_bound(terms, mag):
    """E = (T + 4) * 2^-24 * S: the worst-case error of an fp32 sum of T products in ANY order (each partial sum
    rounded once, relative error 2^-24 of a magnitude bounded by S), plus four more roundings for the epilogue's
    additions.  `mag` is S, the fp64 sum of magnitudes at each element."""
    return (terms + 4) * 2.0 ** -24 * mag


def half_ulp_bf16(a):
    """Half the spacing of bf16 numbers (8 significant bits) in the binade of a >= 0: 2^(floor(log2 a) - 8); 0 at 0.
    Between 2^-9 a (top of a binade) and 2^-8 a (bottom)."""
    a = a.double()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 8), torch.zeros_like(a))


def assert_within_bound(got, ref, mag, terms, name, *, stored_bf16=True, tanh=False, extra=None, exclude=None, tile=None,
                        limit=6):
    """|got - ref| <= half_ulp_bf16(|ref| + E) + E (+ extra) for a bf16 output, E alone for fp32: the worst-case fp32
    summation error of any order plus half a bf16 ulp of whatever the sum came to.  (Half an ulp is 2^-9 of the value
    only at the top of a binade and 2^-8 at its bottom: a flat 2^-9 (|ref| + E) rejects the correctly rounded fp64
    reference itself -- test_conv_exact_cpu.py shows it -- so the ulp is taken from the binade.)  tanh: `ref` is the
    PRE-tanh value; the expectation is t = tanh(ref) and E becomes (1 - t^2) E + 2^-21 (the slope of tanh at the
    reference, plus eight fp32 ulps at 1.0 for the fp32 tanh itself).  `exclude`: boolean tensor of elements whose
    mask branch is undecided (at most 0.1 % of the elements, asserted)."""
    got, ref = got.double(), ref.double()
    e = summation_bound(terms, mag.double())
    if tanh:
        ref = torch.tanh(ref)
        e = (1 - ref * ref) * e + 2.0 ** -21
    bound = half_ulp_bf16(ref.abs() + e) + e if stored_bf16 else e
    if extra is not None:
        bound = bound + extra
    bad = ~((got - ref).abs() <= bound)          # (a NaN compares false: it is reported)
    if exclude is not None:
        assert float(exclude.double().mean()) <= 1e-3, "%s: too many undecided mask elements" % name
        bad = bad & ~exclude
    count = int(bad.sum())
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())
    print("%s: worst |err| / bound = %.3f over %d elements (tile %s)" % (name, worst, got.numel(), tile))
    if count:
        lines = []
        for i in bad.nonzero()[:limit]:
            c = tuple(int(v) for v in i)
            where = (c[0], c[2], c[3], c[1]) if len(c) == 4 else c
            lines.append("%s got %r expected %r bound %.3g" % (where, float(got[c]), float(ref[c]), float(bound[c])))
        raise AssertionError("%s: %d of %d elements outside the bound, tile %s:\n  %s"
                             % (name, count, got.numel(), tile, "\n  ".join(lines)))
