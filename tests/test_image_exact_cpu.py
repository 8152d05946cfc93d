"""CPU checks of the exact image-kernel test kit (image_exact_ref.py, image_exact_cases.py): the lattice and margin
conditions of every case test_image_exact_gpu.py launches, the float64 reference against the oracle's spelling (and
autograd), the comparisons accepting the reference's own output, and -- so that each comparison is known to be able
to fail on these tables -- the comparisons rejecting the output of fourteen deliberately wrong variants."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_exact_cases as IC
import image_exact_ref as R


# ------------------------------------------------------------------------------------------------ table integrity
@pytest.mark.parametrize("case", IC.TRIGGER_CASES, ids=lambda c: c.id)
def test_exact_cases_hold_the_lattice_conditions(case):
    d = IC.exact_data(case)
    E = IC.expect_fwd(case, "exact")
    q = R.fwd_range_check(E.f, d.P, E.f.nr, d.rate, IC.QX, IC.QN, IC.QP, IC.QK)
    assert q == IC.Q_OUT == 2.0 ** -13
    pre = E.f.pre
    outside, on = float((np.abs(pre) > 1).mean()), float((np.abs(pre) == 1).mean())
    print("%s: %.1f %% of the pre-clamp values outside [-1, 1], %.2f %% exactly on +-1" % (case.id, 100 * outside, 100 * on))
    assert outside >= 0.10 and (pre > 1).any() and (pre < -1).any()
    assert on >= 0.01
    nx, hw = IC.counts(case)[0], case.hw
    planted = (np.abs(pre[:nx]) == 1) & d.plant
    assert (planted == d.plant).all()
    for r in {0, 15, 16, hw - 1} - {hw}:
        if r < hw:
            assert planted[..., r, :].any(), "no pixel exactly on a bound in row %d" % r
    assert planted[..., :, 0].any() and planted[..., :, hw - 1].any()
    for k in d.k1:
        assert k[0] != k[2]
    # total variation: equal neighbours, both signs
    dv, dh = np.diff(E.out, axis=-2), np.diff(E.out, axis=-1)
    zero = (float((dv == 0).sum()) + float((dh == 0).sum())) / (dv.size + dh.size)
    assert zero >= 0.05 and (dv > 0).any() and (dv < 0).any() and (dh > 0).any() and (dh < 0).any()
    if hw <= 64:
        assert float(E.tv.max()) / IC.Q_OUT < R.TWO24       # tv is compared for equality on the whole-plane route
    for name in IC.bwd_configs(case, "exact"):
        cfg = IC.bwd_config(case, "exact", name)
        B = IC.expect_bwd(case, "exact", cfg)
        R.bwd_range_check(B.b, d.P, d.rate, cfg.qg, IC.QN, IC.QP, IC.QK, cfg.pre_tanh)
        share = R.assert_not_vacuous(R.t64(B.d), "%s %s" % (case.id, name))
        print("%s %s: %.1f %% of d_noise needs rounding" % (case.id, name, 100 * share))


@pytest.mark.parametrize("case", IC.TRIGGER_CASES, ids=lambda c: c.id)
def test_bound_cases_decide_the_clamp_mask(case):
    """No pre-clamp value within its own bound E_pre of +-1 (so the kernel's fp32 mask is the reference's, without
    exclusions), at least 5 % of the pixels clamped, a share of x exactly on +-1."""
    margin, clamped = IC.mask_margin(case)
    d = IC.bound_data(case)
    print("%s: nearest pre-clamp value %.2f E_pre from a bound, %.1f %% clamped, %d pixels moved to 0"
          % (case.id, margin, 100 * clamped, d.repaired))
    assert margin > 1.0 and clamped >= 0.05
    assert float((np.abs(d.x) == 1).mean()) >= 0.10
    assert d.repaired < 0.01 * d.x.size


def test_dct_tables():
    for hw in IC.DCT_SHAPES:
        for kind in ("identity", "dyadic"):
            E = IC.expect_dct(hw, kind)
            R.range_check(R.t64(E.mag), 0.25, "|D| q |D|^T")
            assert R.f32_exact(E.y)
        x, _ = IC.dct_data(hw, "identity")
        assert float(np.abs(x).max()) <= 1.0 and (x == 1).any() and (x == -1).any()
        if hw >= 32:        # all 256 pipeline levels: most land exactly on an integer before the truncation, the rest just below
            v = (x.flatten()[:256] + np.float32(1)) / np.float32(2) * np.float32(255)
            q = IC.expect_dct(hw, "identity").q.flatten()[:256]
            assert float((v == np.round(v)).mean()) >= 0.5 and (np.arange(256) - q).min() == 0 and (np.arange(256) - q).max() <= 1
    assert R.assert_not_vacuous(R.t64(IC.expect_dct(32, "dyadic").y), "dyadic DCT") > 0.02


def test_warp_tables():
    w = IC.warp_data()
    ix = (w.grids + 1) * 0.5 * (w.H - 1)
    assert (ix == np.round(ix * 4) / 4).all() and (w.grids == 1).any() and (w.grids == -1).any()
    assert (ix == np.round(ix)).mean() > 0.1 and (ix * 2 % 2 == 1).any()
    for groups, second in IC.WARP_BWD:
        d = w.d + w.d2 if second else w.d
        _, mag = R.warp_bwd(w.x, d, w.grids, w.n, groups)
        R.range_check(R.t64(mag), 1.0 / 512, "sum |d| |dsample/dgrid|")
    _, mag = R.warp_bwd_input(w.d, w.grids, w.n)
    R.range_check(R.t64(mag), 1.0 / 512, "sum |w d|")


# ------------------------------------------------------------------------------------------------ reference against the oracle
def test_reference_against_oracle_trigger_mix_and_autograd():
    from oracle import combat_oracle as O
    hw, n, sigma, rate = 16, 2, 0.7, 0.08
    g = torch.Generator().manual_seed(3)
    x = torch.rand(n, 3, hw, hw, generator=g, dtype=torch.float64) * 2.4 - 1.2
    noise = torch.tanh(torch.randn(n, 3, hw, hw, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    d_out = torch.randn(n, 3, hw, hw, generator=g, dtype=torch.float64)
    ref = O.trigger_mix(x, noise, rate, 0.65, sigma)
    l2, tvs = 0.3, 0.2
    tv = (ref[..., 1:, :] - ref[..., :-1, :]).abs().sum() + (ref[..., :, 1:] - ref[..., :, :-1]).abs().sum()
    ((ref * d_out).sum() + l2 * ((ref - x) ** 2).sum() + tvs * tv).backward()
    P = O.lowpass_matrix(hw, 0.65, torch.float64).numpy()
    k1 = O.gaussian_kernel1d(sigma).double().numpy()[None]
    xi, ni, ki = R.plain_rows(n)
    f = R.trigger_fwd(x.numpy(), noise.detach().numpy(), P, k1, rate, xi, ni, ki)
    assert float(np.abs(f.out - ref.detach().numpy()).max()) < 1e-12
    assert (np.abs(f.pre) > 1).mean() > 0.05
    gg, ga = R.image_gradient(x.numpy(), d_out.numpy(), None, f.out, l2, tvs)
    b = R.trigger_bwd(x.numpy(), noise.detach().numpy(), P, k1, rate, xi, ni, ki, gg, ga, 0)
    assert float(np.abs(b.d - noise.grad.numpy()).max()) < 1e-12
    mse, _, tvp, _, _ = R.mse_tv(f.out, f.xr, np.zeros_like(f.out), hw, False, True)
    assert abs(tvp.sum() - float(tv.detach())) < 1e-9
    assert abs(mse.sum() - float(((ref.detach() - x) ** 2).sum())) < 1e-9


def test_reference_against_oracle_frequency_input():
    from oracle import combat_oracle as O
    x, _ = IC.dct_data(32, "real")
    ref = O.frequency_input(torch.from_numpy(x)).double().numpy()
    y, _, q = R.dct_u8(x, R.dct_matrix(32))
    assert (q == ((torch.from_numpy(x) + 1) / 2 * 255).to(torch.uint8).double().numpy()).all()
    assert float(np.abs(y - ref).max()) < 2e-3 * 32          # (the oracle multiplies in fp32)
    assert np.allclose(R.lowpass_matrix(32), O.lowpass_matrix(32, 0.65).double().numpy(), atol=1e-7)
    assert np.allclose(R.gaussian_triple(0.6), O.gaussian_kernel1d(0.6).double().numpy(), atol=1e-7)


def test_reference_against_grid_sample():
    w = IC.warp_data()
    x = torch.from_numpy(w.x).requires_grad_(True)
    grid = torch.from_numpy(w.grids).requires_grad_(True)
    ref = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    assert np.array_equal(R.warp_fwd(w.x, None, w.grids, w.n), ref.detach().numpy())
    ref.backward(torch.from_numpy(w.d))
    part, _ = R.warp_bwd(w.x, w.d, w.grids, w.n, w.n)       # one image per group: the per-image grid gradient
    # (where a coordinate is an integer the two one-sided slopes differ: both spellings take the cell floor() picks)
    assert np.array_equal(part, grid.grad.numpy())
    dx, _ = R.warp_bwd_input(w.d, w.grids, w.n)
    assert np.array_equal(dx, x.grad.numpy())


def test_augment_reference_is_its_own_adjoint_and_matches_a_shift():
    a = IC.aug_data(16)
    out = R.augment_copy(a.x, a.src, a.params)
    dx = R.augment_adjoint(a.d, a.params)
    assert abs((out * a.d).sum() - (a.x[a.src] * dx).sum()) < 1e-9
    i = int(np.where((a.params[:, 0] == 5) & (a.params[:, 1] == -5) & (a.params[:, 3] == 0))[0][0])
    img = a.x[a.src[i]]
    assert np.array_equal(out[i][:, 5:, :11], img[:, :11, 5:]) and not out[i][:, :5].any() and not out[i][:, :, 11:].any()
    j = int(np.where((a.params[:, 0] == 0) & (a.params[:, 1] == 0) & (a.params[:, 3] == 1))[0][0])
    assert np.array_equal(out[j], a.x[a.src[j]][:, :, ::-1])


# ------------------------------------------------------------------------------------------------ the comparisons accept the reference
SMALL = [c for c in IC.TRIGGER_CASES if c.hw <= 20] + [IC.PLAIN_CASES[3]]


@pytest.mark.parametrize("mode", ["exact", "bound"])
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_comparisons_accept_the_reference(case, mode):
    E = IC.expect_fwd(case, mode)
    IC.check_fwd(E, IC.got_fwd(E), case.id)
    for name in IC.bwd_configs(case, mode):
        B = IC.expect_bwd(case, mode, IC.bwd_config(case, mode, name))
        IC.check_bwd(B, IC.got_bwd(B), "%s %s" % (case.id, name))
    for kind in IC.DCT_KINDS:
        D = IC.expect_dct(32, kind)
        IC.check_dct(D, IC.got_dct(D), kind)


# ------------------------------------------------------------------------------------------------ mutants
P16, P20, P80 = IC.PLAIN_CASES[0], IC.PLAIN_CASES[1], IC.PLAIN_CASES[3]
PAIR16, GROUPS16 = IC.PAIR_CASES[0], IC.GROUPS_CASES[0]


def fwd_rejects(case, mode, mut):
    E = IC.expect_fwd(case, mode)
    with pytest.raises(AssertionError):
        IC.check_fwd(E, IC.got_fwd(IC.expect_fwd(case, mode, mut=mut), mut), case.id)


def bwd_rejects(case, mode, name, mut):
    cfg = IC.bwd_config(case, mode, name)
    E = IC.expect_bwd(case, mode, cfg)
    with pytest.raises(AssertionError):
        IC.check_bwd(E, IC.got_bwd(IC.expect_bwd(case, mode, cfg, mut), mut), case.id)


@pytest.mark.parametrize("mut,mode", [("kb_T", "exact"), ("kb_T", "bound"), ("swap_k", "exact")])
def test_mutant_blur_transposed_or_reversed(mut, mode):
    """Kb where Kb^T belongs (both modes); k0 and k2 swapped (the exact mode's asymmetric triples alone can tell: a
    Gaussian is symmetric): both directions, both routes' tables."""
    for case in (P16, P80):
        fwd_rejects(case, mode, {mut})
        bwd_rejects(case, mode, IC.bwd_configs(case, mode)[0], {mut})


@pytest.mark.parametrize("mut", ["strict_mask", "mask_row"])
def test_mutant_clamp_mask(mut):
    """A strict mask at the bounds (only the planted pixels tell); a mask shifted by one row."""
    for case in (P16, P20, P80):
        bwd_rejects(case, "exact", "grad", {mut})
    bwd_rejects(P80, "bound", "mixed", {"mask_row"})


def test_mutant_sign_of_zero():
    for case in (P16, P80):
        bwd_rejects(case, "exact", "tv", {"sgn0"})


@pytest.mark.parametrize("mut", ["hi_trunc", "lo_drop", "pad"])
def test_mutant_c8_stores(mut):
    """hi truncated, lo dropped, pad channels non-zero: the hi / lo image of the forward, the DCT and (pad) d_noise."""
    for mode in ("exact", "bound"):
        E = IC.expect_fwd(P16, mode)
        with pytest.raises(AssertionError):
            IC.check_fwd(E, IC.got_fwd(E, {mut}), P16.id)
    for kind in ("dyadic", "real"):
        D = IC.expect_dct(32, kind)
        with pytest.raises(AssertionError):
            IC.check_dct(D, R.c8_expect(IC.to_f32(D.y), {mut}), kind)
    if mut == "pad":
        B = IC.expect_bwd(P16, "exact", IC.bwd_config(P16, "exact", "grad"))
        with pytest.raises(AssertionError):
            IC.check_bwd(B, IC.got_bwd(B, {"pad"}), P16.id)


def test_mutant_group_triple_index():
    """k1[(i + 1) / ps]."""
    for mode in ("exact", "bound"):
        fwd_rejects(GROUPS16, mode, {"group_shift"})
        bwd_rejects(GROUPS16, mode, IC.bwd_configs(GROUPS16, mode)[0], {"group_shift"})


@pytest.mark.parametrize("mut", ["cross_noise", "cross_l2"])
def test_mutant_pair_rows(mut):
    """The cross rows reading noise[i] instead of noise[n + i]; an L2 term on the cross rows."""
    if mut == "cross_noise":
        fwd_rejects(PAIR16, "exact", {mut})
        bwd_rejects(PAIR16, "exact", "grad", {mut})
    else:
        bwd_rejects(PAIR16, "exact", "l2", {mut})
    bwd_rejects(PAIR16, "bound", "mixed", {mut})


@pytest.mark.parametrize("mut,kinds", [("round_q", ("identity", "dyadic", "real")), ("dct_T", ("dyadic", "real"))])
def test_mutant_dct(mut, kinds):
    """A floor(q + 0.5) quantiser; D^T q D."""
    for kind in kinds:
        for hw in (4, 32):
            E = IC.expect_dct(hw, kind)
            with pytest.raises(AssertionError):
                IC.check_dct(E, IC.got_dct(IC.expect_dct(hw, kind, {mut})), kind)


def test_mutant_warp_last_tap():
    """The tap at H - 1 dropped (a `< H - 1` bound): the grid values exactly on +1 tell."""
    w = IC.warp_data()
    for grid in (w.grids[0], w.grids):
        with pytest.raises(AssertionError):
            R.report_mismatch(R.t64(R.warp_fwd(w.x, None, grid, w.n, {"drop_last_tap"})), R.t64(R.warp_fwd(w.x, None, grid, w.n)),
                              "warp out")
    with pytest.raises(AssertionError):
        R.report_mismatch(R.t64(R.warp_bwd(w.x, w.d, w.grids, w.n, 2, {"drop_last_tap"})[0]),
                          R.t64(R.warp_bwd(w.x, w.d, w.grids, w.n, 2)[0]), "warp partial")
