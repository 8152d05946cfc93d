"""CPU checks of the exact-convolution test kit (conv_exact_ref.py, conv_exact_cases.py): the references against an
independent integer restatement, the range / tie-share conditions and the tile choice of every case the GPU file
launches, and -- so that each comparison is known to be able to fail -- deliberately corrupted expectations: one
element, one guard-band element, a second rounding, another rounding mode."""
import re

import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as CC
import conv_exact_ref as R


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


def int_conv(x, w, stride, pad):
    """Convolution of integer tensors in int64 arithmetic (unfold + matmul): no floating point at all."""
    n, c, h, _ = x.shape
    k, _, r, _ = w.shape
    cols = F.unfold(x.double(), r, padding=pad, stride=stride).round().long()      # [n][c*r*r][p*q]
    p = (h + 2 * pad - r) // stride + 1
    return torch.einsum("kj,njm->nkm", w.long().reshape(k, -1), cols).view(n, k, p, p)


@pytest.mark.parametrize("n,hw,c,k,r,stride", [(2, 6, 8, 16, 3, 1), (3, 7, 16, 8, 3, 2), (2, 8, 8, 8, 1, 2), (1, 5, 24, 8, 3, 1)])
def test_references_against_integer_arithmetic(n, hw, c, k, r, stride):
    pad = 1 if r == 3 else 0
    x, w = R.lattice((n, c, hw, hw), 4, 1), R.lattice((k, c, r, r), 4, 2)
    y = R.conv_fwd(x, w, stride, pad)
    assert torch.equal(y.long(), int_conv(x, w, stride, pad)) and torch.equal(y, y.round())
    assert torch.equal(R.conv_abs(x, w, 0, hw, stride, pad).long(), int_conv(x.abs(), w.abs(), stride, pad))
    # the gradients against autograd of F.conv2d in fp64 (exact on integers of this size)
    dy = R.lattice(tuple(y.shape), 4, 3)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(xr, wr, stride=stride, padding=pad).backward(dy)
    assert torch.equal(R.conv_dgrad(dy, w, hw, stride, pad), xr.grad)
    assert torch.equal(R.conv_wgrad(x, dy, k, r, stride, pad), wr.grad.permute(0, 2, 3, 1).reshape(k, r * r, c))
    xa, da = x.abs().clone().requires_grad_(True), dy.abs()
    wa = w.abs().clone().requires_grad_(True)
    F.conv2d(xa, wa, stride=stride, padding=pad).backward(da)
    assert torch.equal(R.conv_abs(dy, w, 1, hw, stride, pad), xa.grad)
    assert torch.equal(R.wgrad_abs(x, dy, k, r, stride, pad), wa.grad.permute(0, 2, 3, 1).reshape(k, r * r, c))


def test_range_assertions():
    R.range_check(torch.tensor([3322.0, 23725.0]))
    with pytest.raises(AssertionError, match="2\\^24"):
        R.range_check(torch.tensor([2.0 ** 24]))
    with pytest.raises(AssertionError, match="2\\^24"):
        R.range_check(torch.tensor([2.0 ** 21]), 1.0 / 8)
    with pytest.raises(AssertionError, match="fp32"):
        R.rne_bf16(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64))
    with pytest.raises(AssertionError, match="bf16"):
        R.lattice_prologue(torch.tensor([[[[257.0]]]], dtype=torch.float64), None, None, False, 0.0)
    with pytest.raises(AssertionError, match="fp32"):       # a residual that pushes an intermediate off the fp32 grid
        R.epilogue(torch.full((1, 1, 1, 1), 2.0 ** 24, dtype=torch.float64), add_post=torch.ones(1, 1, 1, 1))
    with pytest.raises(AssertionError, match="vacuous"):
        R.assert_not_vacuous(R.lattice((1000,), 100, 1))
    with pytest.raises(AssertionError, match="statistics"):
        R.stats_totals(torch.full((1, 1, 64, 64), 100.0, dtype=torch.float64), 1)     # 4096 * 1e4 > 2^24


def test_rounding_expectation_can_tell_the_modes_apart():
    """On the wide lattice the odd integers of [256, 512) are ties: RNE, truncation and round-half-away all differ."""
    x, w = R.lattice((4, 64, 32, 32), 4, 5), R.lattice((64, 64, 3, 3), 4, 6)
    v = R.conv_fwd(x, w, 1, 1)
    top = R.range_check(R.conv_abs(x, w, 0, 32, 1, 1))
    assert top < 5000 and 0.03 < R.assert_not_vacuous(v) < 0.08      # (sum |x||w| ~ 3300, ~5 % ties at this shape)
    rne, tr, away = R.rne_bf16(v), R.trunc_bf16(v), R.half_away_bf16(v)
    assert int((rne != tr).sum()) > 1000 and int((rne != away).sum()) > 1000
    for wrong in (tr, away):
        with pytest.raises(AssertionError, match="elements wrong"):
            R.report_mismatch(wrong, rne, "rounding mode")
    # exact values: ties go to the even neighbour
    t = torch.tensor([257.0, 259.0, 261.0, -257.0, -259.0, 256.0, 300.0, 301.0], dtype=torch.float64)
    assert R.rne_bf16(t).tolist() == [256.0, 260.0, 260.0, -256.0, -260.0, 256.0, 300.0, 300.0]
    assert R.trunc_bf16(t).tolist() == [256.0, 258.0, 260.0, -256.0, -258.0, 256.0, 300.0, 300.0]
    assert R.half_away_bf16(t).tolist() == [258.0, 260.0, 262.0, -258.0, -260.0, 256.0, 300.0, 302.0]


def test_a_second_rounding_fails_the_comparison():
    """accumulator -> bf16 -> + residual -> bf16 instead of one rounding behind the residual."""
    x, w = R.lattice((2, 64, 16, 16), 4, 7), R.lattice((64, 64, 3, 3), 4, 8)
    res = R.lattice((2, 64, 16, 16), 256, 9)
    acc = R.conv_fwd(x, w, 1, 1)
    v, _, _ = R.epilogue(acc, add_post=res)
    once, twice = R.rne_bf16(v), R.rne_bf16(R.rne_bf16(acc) + res)
    with pytest.raises(AssertionError, match="elements wrong"):
        R.report_mismatch(twice, once, "double rounding")
    # ... while the rel-L2 gate of the older tests lets it pass
    assert float((twice - once).norm() / once.norm()) < 4e-3


def test_one_wrong_element_is_found_and_located():
    exp = R.rne_bf16(R.conv_fwd(R.lattice((3, 64, 8, 8), 4, 10), R.lattice((64, 64, 3, 3), 4, 11), 1, 1))
    got = exp.clone()
    got[2, 17, 5, 3] = 0.0 if float(exp[2, 17, 5, 3]) != 0.0 else 1.0
    with pytest.raises(AssertionError) as e:
        R.report_mismatch(got, exp, "dst", tile=10)
    msg = str(e.value)
    assert "1 of %d elements wrong" % exp.numel() in msg and "(2, 5, 3, 17)" in msg and "tile 10" in msg
    assert "expected %r" % float(exp[2, 17, 5, 3]) in msg
    got = exp.clone()
    got[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 NaN"):
        R.report_mismatch(got, exp, "dst")
    R.report_mismatch(exp.clone(), exp, "dst")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
def test_guard_bands(dtype):
    g = R.Guarded((3, 5, 7), dtype, "dst", "cpu", zero=True)
    assert g.t.data_ptr() % 16 == 0 and g.buf.numel() == 105 + 2 * R.SLACK and float(g.t.float().abs().max()) == 0.0
    g.t.fill_(3)
    g.check("dst")
    g.buf[R.SLACK + 105 + 2] = 0          # a store two elements past the end
    with pytest.raises(AssertionError, match=r"after dst was written: 1 elements, first at offsets \[2\]"):
        g.check("dst")
    g = R.Guarded((4, 4), dtype, "dst", "cpu")
    g.buf[R.SLACK - 1] = 1
    with pytest.raises(AssertionError, match=r"before dw was written: 1 elements, first at offsets \[-1\]"):
        g.check("dw")
    if dtype.is_floating_point:
        s = R.Guarded.source(torch.ones(2, 3, dtype=dtype), "cpu")
        assert bool(s.buf[: R.SLACK].isnan().all()) and bool(s.buf[R.SLACK + 6:].isnan().all()) and float(s.t.sum()) == 6.0


def test_statistics_reference_and_its_failure():
    y = R.lattice((3, 8, 4, 4), 50, 12)
    mx, mean, rstd = R.lattice((3, 8, 4, 4), 4, 13), R.lattice((3, 8), 1, 14), R.pick((0.5, 1.0, 2.0), (3, 8), 15)
    t1, t2 = R.stats_totals(y, 1), R.stats_totals(y, 2, mx, mean, rstd, 0.5)
    assert torch.equal(t1[:, 0], y.sum((2, 3))) and torch.equal(t1[:, 1], (y * y).sum((2, 3)))
    xh = (mx - mean[:, :, None, None]) * rstd[:, :, None, None]
    assert torch.equal(t2[:, 1], (y * xh).sum((2, 3)))
    bad = t1.clone()
    bad[1, 1, 5] += 1
    with pytest.raises(AssertionError, match=r"\(1, 1, 5\)"):
        R.report_mismatch(bad, t1, "statistics")


def test_elementwise_bound_passes_fp32_arithmetic_and_fails_a_local_error():
    x = torch.randn(2, 64, 8, 8, generator=R.gen(16)).to(torch.bfloat16).double()
    w = (torch.randn(64, 64, 3, 3, generator=R.gen(17)) / 24).to(torch.bfloat16).double()
    ref, mag = R.conv_fwd(x, w, 1, 1), R.conv_fwd(x.abs(), w.abs(), 1, 1)
    got = F.conv2d(x.float(), w.float(), padding=1).to(torch.bfloat16).double()        # an fp32 sum in torch's order, one rounding
    R.assert_within_bound(got, ref, mag, 576, "fp32 conv")
    # half a bf16 ulp is 2^-8 of the value at the bottom of a binade: a flat 2^-9 (|ref| + E) + E would reject even
    # the correctly rounded fp64 reference, so the bound takes the ulp from the binade
    e = R.summation_bound(576, mag)
    best = ref.float().to(torch.bfloat16).double()
    assert int(((best - ref).abs() > 2.0 ** -9 * (ref.abs() + e) + e).sum()) > 0
    assert bool(((best - ref).abs() <= R.half_ulp_bf16(ref.abs())).all())
    assert R.half_ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 300.0, 0.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 1.0, 0.0]
    twice = (F.conv2d(x.float(), w.float(), padding=1) * 1.005).to(torch.bfloat16).double()
    with pytest.raises(AssertionError, match="outside the bound"):
        R.assert_within_bound(twice, ref, mag, 576, "perturbed")
    one = got.clone()
    one[1, 3, 2, 7] = 0.0
    with pytest.raises(AssertionError, match=r"1 of \d+ elements outside the bound"):
        R.assert_within_bound(one, ref, mag, 576, "one zeroed")
    # fp32 outputs: E alone is some 1e-5 of the magnitudes -- the rel-L2 2e-3 gate was two orders looser
    g32 = F.conv2d(x.float(), w.float(), padding=1).double()
    R.assert_within_bound(g32, ref, mag, 576, "fp32 output", stored_bf16=False)
    with pytest.raises(AssertionError, match="outside the bound"):
        R.assert_within_bound(g32 * (1 + 1e-4), ref, mag, 576, "fp32 output off by 1e-4", stored_bf16=False)
    # tanh: the reference is the pre-tanh value
    R.assert_within_bound(torch.tanh(F.conv2d(x.float(), w.float(), padding=1)).to(torch.bfloat16).double(), ref, mag, 576,
                          "tanh", tanh=True)


# ---- the GPU file's case tables: everything but the launch ------------------------------------------------------
@pytest.mark.parametrize("case", CC.ALL_CASES, ids=lambda c: c.id)
def test_case_reaches_its_kernel_on_the_lattice(ops, case):
    """build() asserts the range condition, that the mask argument has exact zeros and (wide lattices) that >= 2 % of
    the expected outputs need rounding; combat_conv_pick_tile is host code, so the tile is checked here too."""
    b = CC.build(case, ops, "cpu")
    assert b.picked == case.expect, (case.id, b.picked)
    for _, (g, exp) in b.outputs.items():
        assert tuple(CC.from_nhwc(g.t).shape) == tuple(exp.shape) and not bool(exp.isnan().any())
    if case.lim == 1 and b.stats is not None:
        assert float(b.stats[2].abs().max()) > 0


def test_pairs_and_weight_gradient_cases_are_on_the_lattice(ops):
    import ctypes
    from combat_amd._lib import lib
    for i, (n, hw, c, k) in enumerate(CC.CHAIN_SHAPES):     # every launch of the reduce_first chain leaves slabs behind
        b = CC.wgrad_build(CC.WCase("chain%d" % i, n, hw, c, k, 3, 1), 4, "cpu")
        dw = R.Guarded(b.shape, torch.float32, "dst", "cpu", zero=True)
        assert lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(CC.wgrad_args(b, dw))) > 0, i
    for pa, pb in CC.PAIR_CASES:
        a, b = CC.build(pa, ops, "cpu"), CC.build(pb, ops, "cpu")
        assert a.picked == pa.expect == b.picked == pb.expect
    ids = set()
    for wc in CC.WGRAD_CASES:
        assert wc.id not in ids
        ids.add(wc.id)
        for lim in (4, 1):
            b = CC.wgrad_build(wc, lim, "cpu")
            assert tuple(b.exp.shape) == b.shape and float(b.exp.abs().max()) > 0
    # explicit pixel ranges include counts that do not divide the pixel count
    px = lambda wc: wc.n * ((wc.hw + (2 if wc.r == 3 else 0) - wc.r) // wc.stride + 1) ** 2
    assert any(s > 1 and px(wc) % s for wc in CC.WGRAD_CASES for s, _ in wc.variants)
    assert any(ws for wc in CC.WGRAD_CASES for _, ws in wc.variants) and any(s < 0 for wc in CC.WGRAD_CASES for s, _ in wc.variants)


def test_every_tile_and_property_is_named_by_a_case():
    ids = [c.id for c in CC.ALL_CASES]
    assert len(set(ids)) == len(ids)
    plain = [c.id for c in CC.PLAIN_CASES]
    for tile in list(range(1, 19)):
        for mode in ("fwd", "dgrad"):
            assert any(i.startswith("t%02d-%s-" % (tile, mode)) for i in plain), (tile, mode)
    for family, props in {
        "t0[1-5]": ["raggedN", "stride2-3x3", "stride2-1x1", "K3-padded-to-8", "odd5"],
        "t0[6-9]": ["raggedN", "images-per-tile-8x8", "images-per-tile-4x4", "images-per-tile-2x2"],
        "t1[0146]": ["raggedN", "images-per-tile-8x8", "images-per-tile-4x4"],
        "t17": ["tiles-per-workgroup-n40", "tiles-per-workgroup-n81"],
        "t1[23]": ["raggedN", "stride2-3x3", "stride2-1x1", "odd5", "odd6", "odd10", "images-per-tile-2x2"],
        "t15": ["raggedN", "dup_hilo", "odd6", "odd10", "stride2"],
        "t18": ["K3-padded-to-8", "stem-gradient"],
    }.items():
        for prop in props:
            assert any(re.match(family, i) and prop in i for i in plain), (family, prop)
    feats = set()
    for c in CC.FEATURE_CASES + CC.STATS_CASES:
        feats |= set(c.feat)
    assert feats >= {"post", "bias", "pre", "mask", "mul", "maskact", "maskimg", "act", "nodst", "pro", "proimg", "prolds",
                     "prodst", "src2", "ws", "stats1", "stats2", "wg"}
    kinds = {w.kernel.split("-")[0] for w in CC.WGRAD_CASES}
    assert kinds == {"generic", "lds", "dma", "c8"}
