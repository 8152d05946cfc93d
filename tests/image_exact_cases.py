"""Case tables, host-side builders and the comparison functions of test_image_exact_gpu.py (checked without a GPU by
test_image_exact_cpu.py, which also feeds the comparisons deliberately wrong outputs).

A TrigCase is one launch shape of the trigger family: kind plain (combat_trigger_fwd / _bwd and the total-variation
entry points), pair (combat_trigger_pair_*) or groups (combat_trigger_groups_*); hw <= 64 is the whole-plane route,
hw >= 80 the strip route.  Every case exists in two modes, `exact` (lattice operands) and `bound` (the real low-pass
matrix, Gaussian triples, uint8-derived images, tanh noise).  expect_* build the float64 expectation, got_* turn an
expectation into what a kernel that computed it would store (the CPU file's stand-in for the device), check_* compare.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import image_exact_ref as R

TrigCase = namedtuple("TrigCase", "id kind hw n ps seed")
f32 = np.float32


def tc(kind, hw, n, ps=0):
    cid = "%s_hw%d_n%d%s" % (kind, hw, n, "_ps%d" % ps if ps else "")
    return TrigCase(cid, kind, hw, n, ps, (hw * 131 + n * 17 + ps * 7 + len(kind)) % 10007)


# whole plane: 16 (the reduction scratch B[256] just fits), 20 (q = 5 in mm4), 64 (the maximum); strips: 80 (five strips,
# idle lanes), 256 (every lane on, the largest P)
PLAIN_CASES = [tc("plain", 16, 3), tc("plain", 20, 3), tc("plain", 64, 3), tc("plain", 80, 3), tc("plain", 256, 1)]
PAIR_CASES = [tc("pair", 16, 2), tc("pair", 80, 2)]
# five images in groups of two (the last group short), and ps >= n (one group)
GROUPS_CASES = [tc("groups", 16, 5, 2), tc("groups", 80, 5, 2), tc("groups", 16, 5, 7)]
TRIGGER_CASES = PLAIN_CASES + PAIR_CASES + GROUPS_CASES

# exact mode: every triple asymmetric (k0 != k2), entries in multiples of 1/4
EXACT_TRIPLES = np.array([[0.5, 0.25, 0.25], [0.25, 0.25, 0.5], [0.75, 0.5, -0.25]])
BOUND_SIGMAS = (0.35, 0.9, 0.6)
QX, QN, QP, QK, RATE_EXACT = 1.0 / 128, 0.25, 0.25, 0.25, 0.125
Q_OUT = RATE_EXACT * QP * QP * QN * QK * QK         # 2^-13
RATE_BOUND = float(f32(0.08))
EDGE_ROWS = (0, 15, 16)


def src_index(case):
    """A repeated and a permuted entry (one image: itself)."""
    return np.array([case.n - 1, 0, 0], dtype=np.int32) if case.n > 1 else np.array([0], dtype=np.int32)


def counts(case):
    """(images of x, rows of noise, triples)."""
    if case.kind == "pair":
        return case.n, 2 * case.n, 2
    if case.kind == "groups":
        return case.n, case.n, -(-case.n // case.ps)
    return case.n, case.n, 1


def rows_of(case, src=None, mut=()):
    if case.kind == "pair":
        return R.pair_rows(case.n, mut)
    if case.kind == "groups":
        return R.groups_rows(case.n, case.ps, counts(case)[2], mut)
    return R.plain_rows(case.n, src)


# ------------------------------------------------------------------------------------------------ operands
def lattice_P(hw, rng):
    """Symmetric, entries in multiples of 1/4, |row| sums <= 3/4: a random symmetric permutation pattern (an involution
    without fixed points) plus a +-1/4 band."""
    P = np.zeros((hw, hw))
    perm = rng.permutation(hw)
    for a, b in zip(perm[0::2], perm[1::2]):
        P[a, b] = P[b, a] = rng.choice((-0.25, 0.25))
    for i in range(hw - 1):
        s = rng.choice((-0.25, 0.25))
        P[i, i + 1] += s
        P[i + 1, i] += s
    assert (P == P.T).all() and np.abs(P).sum(1).max() <= 0.75
    return P


@functools.lru_cache(maxsize=None)
def exact_data(case):
    """Lattice operands.  x: multiples of 1/128, 60 % of them within 3/32 of +-1 so that the noise carries them over the
    bounds; two over-saturated corner blocks (|x| = 9/8: clamped whatever the noise, so `out` is flat inside them and the
    total-variation stencil meets equal neighbours, at the plane's border too); and pixels planted exactly on +-1 by
    solving x = +-1 - rate (P N P) wherever that is a multiple of 1/128, on the rows 0, 15, 16, hw - 1 and the columns 0,
    hw - 1 without exception and on a tenth of the rest."""
    nx, nn, nk = counts(case)
    hw, rng = case.hw, np.random.default_rng(case.seed)
    P = lattice_P(hw, rng)
    noise = rng.integers(-4, 5, (nn, 3, hw, hw)) / 4.0
    u = rng.random((nx, 3, hw, hw))
    wide, near = rng.integers(-128, 129, u.shape) / 128.0, rng.integers(116, 129, u.shape) / 128.0
    x = np.where(u < 0.4, wide, np.where(u < 0.7, near, -near))
    B = max(7, hw // 3)
    block = np.zeros((hw, hw), dtype=bool)
    block[:B, :B] = block[hw - B:, hw - B:] = True
    x[..., :B, :B] = 1.125
    x[..., hw - B:, hw - B:] = -1.125
    lf = P @ noise[:nx] @ P.T
    forced = np.zeros((hw, hw), dtype=bool)
    for r in EDGE_ROWS + (hw - 1,):
        if r < hw:
            forced[r, :] = True
    forced[:, 0] = forced[:, hw - 1] = True
    plant = (lf * 16 == np.round(lf * 16)) & ~block & (forced | (rng.random(u.shape) < 0.1))
    sign = rng.choice((-1.0, 1.0), u.shape)
    x = np.where(plant, sign - RATE_EXACT * lf, x)
    assert R.is_multiple(R.t64(x), QX) and R.is_multiple(R.t64(noise), QN) and R.is_multiple(R.t64(P), QP)
    return SimpleNamespace(x=x, noise=noise, P=P, k1=EXACT_TRIPLES[:nk], rate=RATE_EXACT, plant=plant, exact=True)


def e_pre_of(x, noise, P, rate, xi, ni):
    f = R.trigger_fwd(x, noise, P, np.array([[0.0, 1.0, 0.0]]), rate, xi, ni, np.zeros(len(xi), dtype=np.int64))
    return f.pre, R.fwd_bounds(f)[0]


@functools.lru_cache(maxsize=None)
def bound_data(case):
    """The real operands.  x: the data pipeline's (k / 255 - 0.5) / 0.5 in float32 with 15 % of the pixels exactly on
    +-1 (what images with 0 and 255 give); noise: tanh of a wide Gaussian as bf16.  A pixel whose pre-clamp value lies
    within twice its bound E_pre of +-1 gets x = 0 (it then sits near 0): the clamp mask is decided everywhere, no
    element is excluded from any comparison.  The pre-clamp value of a pixel depends on x at that pixel only."""
    nx, nn, nk = counts(case)
    hw, rng = case.hw, np.random.default_rng(case.seed + 1)
    x = ((rng.integers(0, 256, (nx, 3, hw, hw)).astype(f32) / f32(255)) - f32(0.5)) / f32(0.5)
    sat = rng.random(x.shape)
    x[sat < 0.075], x[sat > 0.925] = f32(-1), f32(1)
    x = x.astype(np.float64)
    z = torch.from_numpy(rng.standard_normal((nn, 3, hw, hw)) * 3)
    noise = torch.tanh(z).to(torch.bfloat16).double().numpy()
    P = R.lowpass_matrix(hw, 0.65)
    xi, ni, _ = rows_of(case)
    pre, e_pre = e_pre_of(x, noise, P, RATE_BOUND, xi, ni)
    close = np.abs(np.abs(pre) - 1) <= 2 * e_pre
    bad = np.zeros(x.shape, dtype=bool)
    np.logical_or.at(bad, xi, close)
    x[bad] = 0.0
    k1 = np.stack([R.gaussian_triple(s) for s in BOUND_SIGMAS[:nk]])
    return SimpleNamespace(x=x, noise=noise, P=P, k1=k1, rate=RATE_BOUND, repaired=int(bad.sum()), exact=False)


def data(case, mode):
    return exact_data(case) if mode == "exact" else bound_data(case)


def mask_margin(case):
    """(nearest distance of a pre-clamp value to +-1 in units of its E_pre, share of clamped pixels) of a bound case."""
    d = bound_data(case)
    xi, ni, _ = rows_of(case)
    pre, e_pre = e_pre_of(d.x, d.noise, d.P, d.rate, xi, ni)
    return float((np.abs(np.abs(pre) - 1) / e_pre).min()), float((np.abs(pre) > 1).mean())


# ------------------------------------------------------------------------------------------------ forward
def expect_fwd(case, mode, src=None, mut=()):
    d = data(case, mode)
    xi, ni, ki = rows_of(case, src, mut)
    f = R.trigger_fwd(d.x, d.noise, d.P, d.k1, d.rate, xi, ni, ki, mut)
    e_out = np.zeros_like(f.out) if d.exact else R.fwd_bounds(f)[1]
    mse, e_mse, tv, e_tv, _ = R.mse_tv(f.out, f.xr, e_out, case.hw, case.hw > 64, d.exact)
    if case.kind == "pair":      # the cross rows write no squared error
        mse, e_mse = mse[:case.n], e_mse[:case.n]
    return SimpleNamespace(f=f, out=f.out, e_out=e_out, mse=mse, e_mse=e_mse, tv=tv, e_tv=e_tv, exact=d.exact, hw=case.hw)


def to_f32(a):
    return R.t64(np.asarray(a, dtype=np.float64).astype(f32))


def got_fwd(E, mut=()):
    """What a kernel that computed E stores: fp32 out / mse / tv, the c8 image of the stored out."""
    out = to_f32(E.out)
    return SimpleNamespace(out=out, c8=R.c8_expect(out, mut), mse=to_f32(E.mse), tv=to_f32(E.tv))


def check_fwd(E, got, name):
    """out EQUAL (exact) or within E_out; the c8 image EQUAL to (RNE_bf16(v), RNE_bf16(v - hi), 0, 0) of the fp32 value v
    the same launch stored in `out` (in exact mode that is the exact value); mse within the summation bound; tv EQUAL
    where its sum of magnitudes stays below 2^24 quanta of 2^-13, else within the bound."""
    if E.exact:
        R.report_mismatch(got.out, R.t64(E.out), "out of " + name)
    else:
        R.assert_elementwise(got.out, E.out, E.e_out, "out of " + name)
        if E.hw > 64:
            R.edge_report(got.out.numpy(), E.out, E.e_out, E.hw, "out of " + name)
    if got.c8 is not None:
        R.report_mismatch(got.c8, R.c8_expect(got.out), "out_c8 [row][y][x][channel] of " + name)
        if E.exact:
            R.assert_not_vacuous(got.out, "out_c8 of " + name)
    if got.mse is not None:
        R.assert_elementwise(got.mse, E.mse, E.e_mse, "mse of " + name)
    if got.tv is not None:
        if E.exact and float(E.tv.max()) / Q_OUT < R.TWO24:
            R.report_mismatch(got.tv, R.t64(E.tv), "tv of " + name)
        else:
            R.assert_elementwise(got.tv, E.tv, E.e_tv, "tv of " + name)


# ------------------------------------------------------------------------------------------------ backward
def halves(shape, lim, rng):
    """Multiples of 1/2 in [-lim, lim]."""
    return rng.integers(-2 * lim, 2 * lim + 1, shape) / 2.0


@functools.lru_cache(maxsize=None)
def bwd_config(case, mode, name):
    """Gradient operands of one backward launch.  exact: `grad` (d_out + d_out2 [+ d_cross] in multiples of 1/2 up to +-16, l2 = 0, pre_tanh),
    `l2` (the L2 term alone, 2 l2 = 1, no gradient operand at all: 2^-24 quanta, so without pre_tanh), `tv` (d_out + tv_scale stencil, tv_scale =
    1/2; plain cases).  bound: `mixed` / `mixed_tanh`: d_out + d_out2 + L2 (+ TV on plain cases) (+ d_cross)."""
    nx = counts(case)[0]
    shape, rng = (nx, 3, case.hw, case.hw), np.random.default_rng(case.seed + 2 + len(name))
    c = SimpleNamespace(d_out=None, d_out2=None, d_cross=None, l2=0.0, tv=0.0, pre_tanh=0, qg=0.5, name=name)
    if mode == "exact":
        if name == "l2":
            c.l2, c.qg = 0.5, Q_OUT
        else:
            c.d_out, c.d_out2 = halves(shape, 8, rng), halves(shape, 8, rng)
            c.pre_tanh = int(name == "grad")
            if name == "tv":
                c.d_out2, c.tv = None, 0.5
            if case.kind == "pair":
                c.d_cross = halves(shape, 16, rng)
    else:
        c.d_out, c.d_out2 = (rng.standard_normal(shape).astype(f32).astype(np.float64) for _ in range(2))
        c.l2 = float(f32(0.25))       # (far above a training run's: the term must stand out of the bound)
        c.tv = float(f32(0.1)) if case.kind == "plain" else 0.0
        c.pre_tanh = int(name == "mixed_tanh")
        if case.kind == "pair":
            c.d_cross = rng.standard_normal(shape).astype(f32).astype(np.float64)
    return c


def bwd_configs(case, mode):
    if mode == "exact":
        return ("grad", "l2") + (("tv",) if case.kind == "plain" else ())
    return ("mixed", "mixed_tanh")


@functools.lru_cache(maxsize=None)
def out_operand(case, mode):
    """The `out` tensor handed to the backward: the forward's expectation as fp32 (first half of a pair).  Shared,
    never modified."""
    E = expect_fwd(case, mode)
    return to_f32(E.out[:counts(case)[0]]).numpy()


def expect_bwd(case, mode, cfg, mut=()):
    d = data(case, mode)
    xi, ni, ki = rows_of(case, None, mut)
    out = out_operand(case, mode)
    if case.kind == "pair":
        g, ga = R.pair_gradient(d.x, case.n, cfg.d_out, cfg.d_out2, out, cfg.l2, cfg.d_cross, mut)
    else:
        g, ga = R.image_gradient(d.x, cfg.d_out, cfg.d_out2, out, cfg.l2, cfg.tv, mut)
    b = R.trigger_bwd(d.x, d.noise, d.P, d.k1, d.rate, xi, ni, ki, g, ga, cfg.pre_tanh, mut)
    return SimpleNamespace(b=b, d=b.d, e=b.e, exact=d.exact, hw=case.hw, out=out)


def got_bwd(E, mut=()):
    """The c8 gradient [rows][hw][hw][8] a kernel that computed E stores: bf16 of the fp32 value, channels 3..7 zero."""
    dn = R.t64(E.d).float().to(torch.bfloat16).double()
    c8 = torch.zeros(dn.shape[0], E.hw, E.hw, 8, dtype=torch.float64)
    c8[..., :3] = dn.permute(0, 2, 3, 1)
    if "pad" in mut:
        c8[0, 0, 0, 5] = 2.0 ** -20
    return c8


def check_bwd(E, got, name):
    """d_noise EQUAL RNE_bf16(exact), or within half_ulp_bf16(|ref| + E) + E; channels 3..7 exactly zero."""
    planes = got[..., :3].permute(0, 3, 1, 2)
    if E.exact:
        R.report_mismatch(planes, R.rne_bf16(R.t64(E.d)), "d_noise of " + name)
    else:
        R.assert_elementwise(planes, E.d, E.e, "d_noise of " + name, stored_bf16=True)
        if E.hw > 64:
            bound = R.half_ulp_bf16(R.t64(np.abs(E.d) + E.e)).numpy() + E.e
            R.edge_report(planes.numpy(), E.d, bound, E.hw, "d_noise of " + name)
    R.report_mismatch(got[..., 3:], torch.zeros_like(got[..., 3:]), "channels 3..7 of d_noise of " + name)


# ------------------------------------------------------------------------------------------------ DCT input
DCT_SHAPES = (4, 32, 64, 80)          # whole plane: the minimum, the detector's 32, the maximum; the strip route
DCT_KINDS = ("identity", "dyadic", "real")
DCT_N = 2


@functools.lru_cache(maxsize=None)
def dct_data(hw, kind):
    """x float32 [2][3][hw][hw]: the 256 pipeline levels (k / 255 - 0.5) / 0.5, unscaled, then arbitrary values of
    [-1, 1] with +-1 themselves.  D: the identity, a non-symmetric matrix of multiples of 1/2 in [-1, 1] (|D| q |D|^T <=
    hw^2 255 < 2^24 quanta of 1/4 up to hw = 80), or the real DCT-II matrix as fp32."""
    rng = np.random.default_rng(hw * 3 + len(kind))
    levels = ((np.arange(256, dtype=f32) / f32(255)) - f32(0.5)) / f32(0.5)
    x = rng.uniform(-1, 1, DCT_N * 3 * hw * hw).astype(f32)
    x[:min(256, x.size // 2)] = levels[:min(256, x.size // 2)]
    x[-2:] = (-1, 1)
    x = np.clip(x, -1, 1).reshape(DCT_N, 3, hw, hw)
    if kind == "identity":
        D = np.eye(hw)
    elif kind == "dyadic":
        D = rng.integers(-2, 3, (hw, hw)) / 2.0
        assert not (D == D.T).all()
    else:
        D = R.dct_matrix(hw).astype(f32).astype(np.float64)
    return x, D


def expect_dct(hw, kind, mut=()):
    x, D = dct_data(hw, kind)
    y, mag, q = R.dct_u8(x, D, mut)
    # two chains of hw fma terms each: k = 2 hw on |D| q |D|^T
    return SimpleNamespace(y=y, e=2 * hw * R.U24 * mag, mag=mag, q=q, exact=kind != "real", kind=kind, hw=hw)


def got_dct(E):
    return R.c8_expect(to_f32(E.y))


def check_dct(E, got, name):
    """exact: hi / lo / pad EQUAL the c8 image of the exact value (identity: hi = q, lo = 0).  real D: hi within
    half_ulp_bf16(|ref| + E) + E, hi + lo within E + 2^-17 (|ref| + E) (lo = RNE_bf16(v - hi) with |v - hi| <= 2^-8 |v|
    leaves at most 2^-17 |v|), pad zero."""
    hi, lo = got[..., :3].permute(0, 3, 1, 2), got[..., 3:6].permute(0, 3, 1, 2)
    if E.exact:
        R.report_mismatch(got, R.c8_expect(E.y), "dct c8 [image][y][x][channel] of " + name)
        if E.kind == "identity":
            R.report_mismatch(hi, R.t64(E.q), "hi = q of " + name)
            assert float(lo.abs().max()) == 0.0
        return
    R.assert_elementwise(hi, E.y, E.e, "dct hi of " + name, stored_bf16=True)
    R.assert_elementwise(hi + lo, E.y, E.e + 2.0 ** -17 * (np.abs(E.y) + E.e), "dct hi + lo of " + name)
    R.report_mismatch(got[..., 6:], torch.zeros_like(got[..., 6:]), "channels 6..7 of " + name)


# ------------------------------------------------------------------------------------------------ augmentation
AUG_SHAPES = (16, 112)            # the LDS gather, the global route (hw > 96)
AUG_NX = 5


@functools.lru_cache(maxsize=None)
def aug_data(hw):
    """18 images: offsets -5, 0, +5 in each axis, each with and without the flip (so: no crop and no flip, crop alone,
    flip alone, both); the source batch has 5 images, picked by a src_index with repeats.  x: arbitrary fp32 values (a
    copy is exact on any data; their low bits exercise both roundings of the hi / lo split).  d: bf16 gradient values;
    prior: multiples of 1/4 for the accumulating launch."""
    rng = np.random.default_rng(hw)
    params = np.array([[ox, oy, 0.0, fl] for fl in (0.0, 1.0) for oy in (-5, 0, 5) for ox in (-5, 0, 5)], dtype=f32)
    n = len(params)
    x = rng.uniform(-1, 1, (AUG_NX, 3, hw, hw)).astype(f32).astype(np.float64)
    src = rng.permutation(n).astype(np.int32) % AUG_NX
    d = rng.integers(-32, 33, (n, 3, hw, hw)) / 8.0
    prior = rng.integers(-16, 17, (n, 3, hw, hw)) / 4.0
    return SimpleNamespace(x=x, params=params, src=src, d=d, prior=prior, n=n, hw=hw)


# ------------------------------------------------------------------------------------------------ warp
WARP_H, WARP_N = 17, 5


@functools.lru_cache(maxsize=None)
def warp_data():
    """H = 17: 0.5 (H - 1) = 8, so a grid in multiples of 1/32 has tap coordinates in multiples of 1/4 and weights in
    multiples of 1/16.  The grids hold +-1 exactly (the tap at H - 1 with a zero-weight neighbour outside, and at 0),
    integer and half-integer coordinates.  x: integers in [-8, 8]; gradients: multiples of 1/2."""
    H, n, rng = WARP_H, WARP_N, np.random.default_rng(17)
    grids = rng.integers(-32, 33, (n, H, H, 2)) / 32.0
    grids[:, 0, :, :] = rng.choice((-1.0, 1.0), (n, H, 2))                 # exactly +-1
    grids[:, 1, :, :] = rng.integers(-8, 9, (n, H, 2)) / 8.0              # integer coordinates
    grids[:, 2, :, :] = (2 * rng.integers(-8, 8, (n, H, 2)) + 1) / 16.0   # half-integers
    grids[:, 3, :, 0], grids[:, 3, :, 1] = 1.0, rng.integers(-32, 33, (n, H)) / 32.0     # x at H - 1, y anywhere
    x = rng.integers(-8, 9, (n, 3, H, H)).astype(np.float64)
    d, d2 = halves((n, 3, H, H), 2, rng), halves((n, 3, H, H), 2, rng)
    src = np.array([3, 0, 0, 4, 1], dtype=np.int32)
    return SimpleNamespace(H=H, n=n, grids=grids, x=x, d=d, d2=d2, src=src)


# (groups, with d_out2): n = 5 in 2 ragged groups (per = 3); 7 groups > n (the last two empty: zeros); with d_out2
WARP_BWD = ((2, False), (7, False), (3, True))
