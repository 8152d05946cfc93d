"""CPU checks of the exact normalisation / upsample test kit (norm_exact_ref.py, norm_exact_cases.py): the references
against exact rational arithmetic and against autograd, the lattice / tie-share / undecided-branch conditions of every
case the GPU file launches, the paths the case tables reach (from a restatement of the launch rules of norm.hip), and
-- so that each comparison is known to be able to fail -- deliberately corrupted expectations."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_exact_cases as NC
import norm_exact_ref as R


def frac(t):
    return [Fraction(float(v)) for v in t.flatten()]


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("px,eps", [(4, 0.0), (8, 0.0), (9, 0.25), (33, 0.0), (16, 0.25)])
def test_lattice_statistics_in_rational_arithmetic(px, eps):
    """mean, var and rstd^2 (var + eps) = 1 of every channel, in fractions.Fraction: no floating point at all."""
    const = (1,) if eps else ()
    L = R.norm_lattice(2, px, 3, eps, 5, const)
    for g in range(2):
        for c in range(3):
            xs = frac(L.x[g, :, c])
            mean = sum(xs) / px
            var = sum(v * v for v in xs) / px - mean * mean
            assert mean == Fraction(float(L.mean[g, c])) and var == Fraction(float(L.var[g, c]))
            rstd = Fraction(float(L.rstd[g, c]))
            assert rstd * rstd * (var + Fraction(eps)) == 1
            ts, rs = frac(L.t[g, :, c]), frac(L.r[g, :, c])
            assert sum(ts) == 0 and sum(rs) == 0 and sum(a * b for a, b in zip(ts, rs)) == 0


def test_odd_counts_need_the_wider_lattice():
    """sum t = 0 makes sum t^2 even, so count * v must be even: no v in {1/4, 1} at an odd count, and v = 4 needs a
    +-3 pair (documented in norm_exact_ref)."""
    for px in (33, 37, 49, 255, 257, 1023):
        assert R.t_pairs(px, 1) is None and R.t_pairs(px, 4) is None
        p1, p2, p3 = R.t_pairs(px, 16)
        assert p3 == 1 and 2 * (p1 + p2 + p3) <= px
    for px in (4, 196, 256, 300, 784, 1024):
        assert R.t_pairs(px, 4)[2] == 0 and R.t_pairs(px, 16)[2] == 0          # even counts stay in {-2 .. 2}


def test_forward_and_backward_against_autograd():
    """The exact expectations against the normalisation written out with torch.mean / torch.var + leaky_relu and its
    autograd in fp64 (equal up to fp64 rounding; the lattice values themselves are exact, so 1e-12 is generous)."""
    for groups, px, C, eps in ((1, 16, 8, 0.0), (3, 8, 8, 0.0), (1, 16, 8, 0.25)):
        L = R.norm_lattice(groups, px, C, eps, 3, (2,) if eps else ())
        gamma, beta = NC.affine(C, 4)
        add = NC.ints(L.x.shape, -4, 4, 6)
        _, _, act, exact = R.forward_expect(L, gamma, beta, 0.25, add)
        x = L.x.permute(0, 2, 1).clone().requires_grad_(True)               # [g][C][px]
        mu, var = x.mean(2, keepdim=True), x.var(2, unbiased=False, keepdim=True)     # (torch's batch_norm refuses eps = 0)
        y = (x - mu) / torch.sqrt(var + eps) * gamma[None, :, None] + beta[None, :, None]
        ref = F.leaky_relu(y + add.permute(0, 2, 1), 0.25)
        assert float((ref.detach().permute(0, 2, 1) - exact).abs().max()) < 1e-12       # (`exact` is the activated value)
        dz = R.lattice_dz(L, 7)
        y.backward(dz.permute(0, 2, 1))
        E = R.backward_expect(L, dz, gamma)
        assert float((x.grad.permute(0, 2, 1) - E.exact).abs().max()) < 1e-12
        xh = (L.x - L.mean[:, None, :]) * L.rstd[:, None, :]
        if groups == 1:
            assert torch.equal(E.dbeta, dz.sum((0, 1))) and torch.equal(E.dgamma, (dz * xh).sum((0, 1)))


def test_partial_rows_conditions():
    L = R.norm_lattice(3, 300, 8, 0.0, 1)
    for rows in (1, 2, 31, 257, 4160):
        p = R.partial_rows(L.s1, L.s2, rows, 2)
        assert p.shape == (3, rows, 2, 8) and torch.equal(p.sum(1)[:, 0], L.s1) and torch.equal(p.sum(1)[:, 1], L.s2)
        assert R.is_multiple(p[:, :-1], 1.0) and R.is_f32(p)
    with pytest.raises(AssertionError, match="fp32"):          # a total beyond 2^24 quanta cannot sit in one row
        R.partial_rows(torch.full((1, 8), 2.0 ** 26 + 0.25, dtype=torch.float64), L.s2[:1], 1, 3)


def test_running_expectation_in_rational_arithmetic():
    """running_expect against Fractions of the same fp32 inputs: equal after rounding to fp32, or one ulp apart where
    the exact value sits next to a tie (fp64 then fp32 is a double rounding)."""
    rm0, rv0 = np.float32([0.3, -1.7, 2.5]), np.float32([0.9, 1.1, 0.5])
    mean, var = np.float64([1.0, -2.0, 3.0]), np.float64([0.25, 4.0, 16.0])
    for count in (1, 2, 300):
        rm, rv = R.running_expect(rm0, rv0, mean, var, count)
        mom = Fraction(R.MOMENTUM)
        for i in range(3):
            unb = Fraction(float(var[i])) * count / (count - 1) if count > 1 else Fraction(float(var[i]))
            for got, old, new in ((rm[i], rm0[i], Fraction(float(mean[i]))), (rv[i], rv0[i], unb)):
                exact = (1 - mom) * Fraction(float(old)) + mom * new
                assert abs(Fraction(float(got)) - exact) <= Fraction(float(np.spacing(np.abs(got))))
    R.assert_within_ulps(rm, rm, 1, "same")
    with pytest.raises(AssertionError, match="ulp"):
        R.assert_within_ulps(rm + 2 * np.spacing(rm), rm, 1, "two ulps")
    with pytest.raises(AssertionError, match="ulp"):
        R.assert_within_ulps(np.float32([np.nan, 0, 0]), rm, 1, "nan")


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (7, 7)])
def test_upsample_reference(h, w):
    """up2x against nn.functional.interpolate (bilinear, align_corners=False) and up2x_adjoint against its autograd;
    the weights are sixteenths, so fp64 is exact on integers."""
    u = NC.ints((2, h, w, 3), -9, 9, h * 10 + w).requires_grad_(True)
    ref = F.interpolate(u.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.equal(R.up2x(u.detach()), ref.permute(0, 2, 3, 1).detach())
    d = NC.ints((2, 2 * h, 2 * w, 3), -9, 9, 99)
    ref.backward(d.permute(0, 3, 1, 2))
    assert torch.equal(R.up2x_adjoint(d), u.grad)
    m = R.up_matrix(h)
    assert torch.equal(m.sum(1), torch.ones(2 * h, dtype=torch.float64)) and R.is_multiple(m, 0.25)
    if h > 1:       # the clamped edges carry both weights
        assert float(m[0, 0]) == 1.0 and float(m[2 * h - 1, h - 1]) == 1.0


def test_lrelu02_is_one_fp32_rounding():
    v = torch.tensor([-3.0625, -0.5, 0.0, 7.25], dtype=torch.float64)
    got = R.lrelu02_f32(v)
    exp = torch.where(v > 0, v.float(), torch.tensor(0.2, dtype=torch.float32) * v.float()).double()
    assert torch.equal(got, exp)


# ------------------------------------------------------------------------------------------------ per-case conditions
@pytest.mark.parametrize("case", NC.FORWARD_CASES, ids=lambda c: c.id)
def test_forward_case_conditions(case):
    """The builder's own assertions (lattice, fp32-representable intermediates, partial rows, direct-form range), the
    tie share of the case and the shape of its expectation."""
    b = NC.build_forward(case)
    assert R.assert_not_vacuous(b.exact, case.id) >= 0.02
    assert b.act.shape == (case.groups, case.px, case.C) and R.is_bf16(b.act)
    if case.const:
        assert bool((b.L.var[:, list(case.const)] == 0).all()) and bool((b.L.var > 0).any())
    if case.slope == 0.25:
        assert bool((b.exact < 0).any()) or case.px == 1, "no negative argument: the slope is not exercised"
    if case.running:
        assert np.isfinite(b.rm).all() and np.isfinite(b.rv).all()


@pytest.mark.parametrize("case", NC.BACKWARD_CASES, ids=lambda c: c.id)
def test_backward_case_conditions(case):
    b = NC.build_backward(case)
    assert R.is_bf16(b.E.dx) and b.E.dx.shape == b.x.shape
    assert bool((b.E.s2 != 0).any()) or case.px == 1
    if case.add:
        assert R.tie_share(b.E.exact) >= 0.02


@pytest.mark.parametrize("case", NC.UP_CASES, ids=lambda c: c.id)
def test_up_case_conditions(case):
    plain, fused, bwd = NC.build_up(case, False), NC.build_up(case, True), NC.build_up_bwd(case)
    if case.H * case.W >= 4:
        assert R.assert_not_vacuous(plain.exact, case.id) >= 0.02 and R.assert_not_vacuous(bwd.exact, case.id) >= 0.02
        assert bool((plain.exact < 0).any()) and bool((fused.exact < 0).any() or case.skip)
        if case.skip:
            assert R.assert_not_vacuous(fused.exact, case.id) >= 0.02
    assert plain.out.shape == (case.N, 2 * case.H, 2 * case.W, case.C)


@pytest.mark.parametrize("case", NC.BOUND_CASES, ids=lambda c: c.id)
def test_bound_case_undecided_share(case):
    """At most 0.1 % of a Gaussian case's elements may take either LeakyReLU branch, counted from the reference alone
    (fp64 statistics of the same bits)."""
    b = NC.build_forward_bound(case)
    rstd = 1.0 / torch.sqrt(b.var + case.eps)
    gamma, beta = NC.affine_or_identity(b, case.C)
    scale = gamma[None] * rstd
    shift = beta[None] - b.mean * scale
    _, e, und = NC.forward_bound_expect(b, case, scale, shift)
    assert float(und.double().mean()) <= 1e-3 and bool((e > 0).all())
    NC.build_backward_bound(case)


@pytest.mark.parametrize("case", NC.UP_BOUND_CASES, ids=lambda c: c.id)
def test_up_bound_case_undecided_share(case):
    b = NC.build_up_bound(case)
    _, e, und = NC.up_forward_bound_expect(b, b.sy, b.ty)
    assert float(und.double().mean()) <= 1e-3
    assert bool((b.y < 0).any()) and bool((b.s is None) or (b.s < 0).any())


# ------------------------------------------------------------------------------------------------ path coverage
def test_case_tables_reach_every_path():
    """From the launch rules restated in norm_exact_cases (fused_chunk, stage1, up_bands): the tables still reach chunk
    256 / 512 / 1024, a ragged last chunk, several chunks of several groups, stage 1 with empty slices and with more
    than 32 rows per slice, every row-unroll boundary, a dead octet, a second channel workgroup, and ragged bands."""
    with_rows = [c for c in NC.FORWARD_CASES if c.rows]
    chunks = {NC.fused_chunk(c.px, c.groups, c.C) for c in with_rows}
    assert {256, 512, 1024} <= chunks
    multi = [c for c in with_rows if NC.fused_chunk(c.px, c.groups, c.C) > 256]
    assert any(c.px % NC.fused_chunk(c.px, c.groups, c.C) for c in multi)                       # ragged last chunk
    assert any(c.groups > 1 for c in multi) and any(c.C > 64 for c in multi) and any(c.add for c in multi)
    assert all(-(-c.px // NC.fused_chunk(c.px, c.groups, c.C)) * c.groups * ((c.C + 63) // 64) <= 1024 for c in with_rows)
    assert NC.fused_chunk(262181, 1, 8) == 512 and 262181 % 512 == 37 and -(-262181 // 512) == 513
    # a last pass of a later load_pass that is ragged against 32 * 8 pixels: the i1 - 1 clamp is live
    assert any((c.px % NC.fused_chunk(c.px, c.groups, c.C)) % 256 for c in multi)
    assert any(c.px % 256 and c.px > 256 for c in NC.DIRECT_CASES) and any(c.px == 1024 for c in NC.DIRECT_CASES)
    rows = {c.rows for c in with_rows}
    assert {1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 4160} <= rows
    assert NC.stage1(256) is None and NC.stage1(257) == (5, 12) and NC.stage1(4160) == (65, 0)
    for name, table in (("forward", NC.FORWARD_CASES), ("backward", NC.BACKWARD_CASES), ("chain", NC.CHAIN_CASES)):
        st = [NC.stage1(c.rows) for c in table if c.rows and NC.stage1(c.rows)]
        assert any(empty > 0 for _, empty in st) and any(per > 32 for per, _ in st), name
        assert any(c.groups > 1 and c.rows > 256 for c in table), name              # a non-zero group offset in stage 1
        assert any(c.C % 64 for c in table) and any(c.C > 64 for c in table), name  # dead octets, second workgroup
    assert {c.px for c in NC.ONEPASS_CASES} == {1, 37, 255, 256, 257}
    assert {c.px for c in NC.DIRECT_CASES} == {1, 4, 33, 49, 196, 784, 1023, 1024}
    bands = [NC.up_bands(c.N, c.H, c.W, c.C) + (2 * c.H,) for c in NC.UP_CASES]
    assert any(n > 1 and ho % band for band, n, ho in bands), "no ragged last band"
    assert any(n > 1 and ho % band == 0 for band, n, ho in bands) and any(n == 1 for band, n, ho in bands)
    assert any(c.H != c.W for c in NC.UP_CASES) and {(c.H, c.W) for c in NC.UP_CASES} >= {(1, 1), (7, 7), (14, 14), (28, 28), (32, 32)}
    assert {c.rows for c in NC.UP_CASES} == {0, 1, 7, 256}


# ------------------------------------------------------------------------------------------------ comparisons can fail
def test_exact_comparison_fails_on_corruptions():
    case = NC.nc(1, 300, 72, 33, add=2)
    b = NC.build_forward(case)
    R.report_mismatch(b.act.clone(), b.act, "same")
    flipped = b.act.clone()
    flipped[0, 299, 71] += float(R.half_ulp_bf16(flipped[0, 299, 71].abs().clamp_min(1.0))) * 2     # one bf16 ulp
    with pytest.raises(AssertionError, match="1 of"):
        R.report_mismatch(flipped, b.act, "one element")
    nan = b.act.clone()
    nan[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 NaN"):
        R.report_mismatch(nan, b.act, "nan")
    for name, other in (("truncation", R.trunc_bf16(b.exact)),
                        ("ties away", R.half_away_bf16(b.exact))):
        with pytest.raises(AssertionError, match="wrong"):
            R.report_mismatch(other, b.act, name)
    # a second rounding: the normalised value stored as bf16 before the residual is added
    main = R.rne_bf16(R.forward_arg(b.x, b.scale, b.shift))
    twice = R.rne_bf16(R.lrelu(main + R.forward_arg(torch.zeros_like(b.x), b.scale * 0, b.shift * 0, b.add, b.add_scale,
                                                     b.add_shift), case.slope))
    with pytest.raises(AssertionError, match="wrong"):
        R.report_mismatch(twice, b.act, "second rounding")
    # a row read twice / skipped changes the statistics: the rows are all different
    rows = b.rows.clone()
    rows[0, 5] = rows[0, 4]
    assert not torch.equal(rows.sum(1), b.rows.sum(1))


def test_guard_band_detects_one_element():
    for dtype in (torch.bfloat16, torch.float32, torch.int64):
        g = R.Guarded((3, 8), dtype, "dst", "cpu")
        g.t.zero_()
        g.check("clean")
        g.buf[R.SLACK + 24] = 1
        with pytest.raises(AssertionError, match="after"):
            g.check("one behind")
        g = R.Guarded((3, 8), dtype, "dst", "cpu")
        g.buf[R.SLACK - 1] = 1
        with pytest.raises(AssertionError, match="before"):
            g.check("one in front")
    s = R.Guarded.source(torch.ones(3, 8), "cpu")
    assert bool(torch.isnan(s.buf[:R.SLACK]).all()) and bool(torch.isnan(s.buf[R.SLACK + 24:]).all())


def test_bound_comparison_fails_on_corruptions():
    case = NC.BOUND_CASES[0]
    b = NC.build_forward_bound(case)
    rstd = 1.0 / torch.sqrt(b.var + case.eps)
    scale = (b.gamma[None] * rstd).float().double()
    shift = (b.beta[None] - b.mean * scale).float().double()
    ref, e, und = NC.forward_bound_expect(b, case, scale, shift)
    good = ref.float().to(torch.bfloat16).double()
    R.assert_elementwise(good, ref, e, "correctly rounded", exclude=und)
    bad = good.clone()
    i = (0, 7, 3)
    bad[i] += 4 * float(R.half_ulp_bf16(bad[i].abs()))             # two bf16 ulps
    with pytest.raises(AssertionError, match="1 of"):
        R.assert_elementwise(bad, ref, e, "one element", exclude=und)
    with pytest.raises(AssertionError, match="outside"):           # truncation is up to a whole ulp off
        R.assert_elementwise(R.trunc_bf16(ref), ref, e, "truncation", exclude=und)
    other = NC.forward_bound_expect(b, case, scale, shift * 1.001)[0].float().to(torch.bfloat16).double()
    with pytest.raises(AssertionError, match="outside"):
        R.assert_elementwise(other, ref, e, "another shift", exclude=und)


def test_upsample_comparison_fails_on_swapped_axes():
    case = [c for c in NC.UP_CASES if c.H != c.W][0]
    b = NC.build_up(case, False)
    N, H, W, C = case.N, case.H, case.W, case.C
    swapped, _ = R.up_forward_expect(b.y.reshape(N, W, H, C), b.sy, b.ty, None if b.s is None else b.s.reshape(N, W, H, C),
                                     b.ss, b.ts)
    with pytest.raises(AssertionError, match="wrong"):
        R.report_mismatch(swapped.reshape(-1), b.out.reshape(-1), "H and W swapped")
    bb = NC.build_up_bwd(case)
    du, _ = R.up_backward_expect(bb.d_out.reshape(N, 2 * W, 2 * H, C), bb.out.reshape(N, 2 * W, 2 * H, C))
    with pytest.raises(AssertionError, match="wrong"):
        R.report_mismatch(du.reshape(-1), bb.du.reshape(-1), "H and W swapped (adjoint)")
    # the edge weight: an adjoint that gives the last row 0.75 where it takes 1 differs on the last row only
    m = R.up_matrix(H)
    m[2 * H - 1, H - 1] = 0.75
    wrong = torch.einsum("ph,npqc,qw->nhwc", m, bb.d_out, R.up_matrix(W))
    assert not torch.equal(wrong[:, H - 1], bb.exact[:, H - 1]) and torch.equal(wrong[:, :H - 1], bb.exact[:, :H - 1])
