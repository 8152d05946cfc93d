"""Bit-exact and element-wise tests of the convolution kernels (conv_gemm, conv3x3, conv3x3_dma, conv_gather_dma,
conv_k8 and the conv_wgrad* files) on the MI355X.

The rel-L2 gates of test_kernels_gpu.py cannot see a local error: a few zeroed outputs, a row of a ragged last tile, a
second rounding all fit under 4e-3.  Here every stored element is compared.

  exact     lattice inputs (conv_exact_ref.py): small integers and dyadic parameters, for which every summation order
            gives the same exact number; the stored bf16 must EQUAL RNE_bf16(exact) and fp32 weight gradients must
            equal the integers.  No tolerance anywhere.  Each case asserts the picked tile, the range condition
            (in the builder), untouched guard bands around every destination (outputs, statistics, weight gradients,
            workspaces) and no NaN in any output although NaN surrounds every source tensor.  Values are compared as
            numbers, so -0 and +0 are the same.
  bound     Gaussian inputs, every element within the worst-case fp32 summation bound of any order plus half a bf16
            ulp: |got - ref64| <= 2^-9 (|ref64| + E) + E, E = (T + 4) 2^-24 S (fp32 outputs: E alone).

The case tables live in conv_exact_cases.py; test_conv_exact_cpu.py checks them without a GPU.
"""
import ctypes
import math

import pytest
import torch

import conv_exact_cases as CC
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from combat_amd._lib import lib as l
    return l


def check_built(b, case):
    """After the launch: guard bands, outputs (NaN included), statistics rows."""
    torch.cuda.synchronize()
    for name, g in b.guards:
        g.check("%s of %s" % (name, case.id))
    for name, (g, exp) in b.outputs.items():
        R.report_mismatch(CC.from_nhwc(g.t), exp, "%s of %s" % (name, case.id), b.picked)
    if b.stats is not None:
        sg, rpi, totals = b.stats
        got = sg.t.double().cpu()
        assert not bool(torch.isnan(got).any()), "NaN in the statistics rows of %s" % case.id
        R.report_mismatch(got.sum(0), totals.sum(0), "statistics totals [2][K] of %s" % case.id, b.picked)
        if rpi:
            n = totals.shape[0]
            assert got.shape[0] >= n * rpi
            R.report_mismatch(got[: n * rpi].view(n, rpi, 2, -1).sum(1), totals, "per-image statistics [N][2][K] of %s" % case.id,
                              b.picked)


def run_exact(ops, case):
    b = CC.build(case, ops, DEV)
    assert b.picked == case.expect, (case.id, b.picked)
    ops.conv_launch(b.a)
    check_built(b, case)


@pytest.mark.parametrize("case", CC.PLAIN_CASES, ids=lambda c: c.id)
def test_exact_plain(ops, case):
    """Plain forward / input gradient on every tile id, wide lattice: the stored bf16 equals RNE_bf16(exact)."""
    run_exact(ops, case)


@pytest.mark.parametrize("case", CC.FEATURE_CASES, ids=lambda c: c.id)
def test_exact_epilogue_and_prologue(ops, case):
    """Residuals, bias, masks (tables per channel / per image, activated, with the scale multiplied in), the second
    output, prologues (in registers and in LDS, with pro_act_dst), the second reduction source and the split reduction
    with a workspace: one rounding, in the header's order."""
    run_exact(ops, case)


@pytest.mark.parametrize("case", CC.STATS_CASES, ids=lambda c: c.id)
def test_exact_statistics(ops, case):
    """stats_kind 1 and 2 on the narrow lattice, with and without COMBAT_STATS_PER_WORKGROUP: the rows, summed in fp64
    on the host, give the exact per-channel (per-image where the layout says so) totals of the stored output."""
    run_exact(ops, case)


@pytest.mark.parametrize("pa,pb", CC.PAIR_CASES, ids=lambda c: c.id)
def test_exact_pair(ops, lib, pa, pb):
    """combat_conv_gemm_pair against the exact expectation of both convolutions (not only against two launches)."""
    a, b = CC.build(pa, ops, DEV), CC.build(pb, ops, DEV)
    assert a.picked == pa.expect and b.picked == pb.expect, (a.picked, b.picked)
    ops.check(lib.combat_conv_gemm_pair(ctypes.byref(b.a), ctypes.byref(a.a), torch.cuda.current_stream().cuda_stream),
              "combat_conv_gemm_pair")
    check_built(a, pa)
    check_built(b, pb)


# ------------------------------------------------------------------------------------------------ weight gradients
def launch_wgrad(ops, lib, b, split, use_ws, name, defer=False):
    st = torch.cuda.current_stream().cuda_stream
    dw = R.Guarded(b.shape, torch.float32, "dst", DEV, zero=True)
    ws = None
    need = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(CC.wgrad_args(b, dw, split))))
    if use_ws and need:
        ws = R.Guarded((need,), torch.uint8, "dst", DEV)
    a = CC.wgrad_args(b, dw, split, ws, defer=int(defer))
    ops.check(lib.combat_conv_wgrad(ctypes.byref(a), st), "combat_conv_wgrad", name)
    if defer:
        ops.check(lib.combat_conv_wgrad_reduce(ctypes.byref(a), st), "combat_conv_wgrad_reduce", name)
    torch.cuda.synchronize()
    dw.check("dw of " + name)
    if ws is not None:
        ws.check("workspace of " + name)
    R.report_mismatch(dw.t.double().cpu(), b.exp, "dw [k][tap][c] of " + name)
    return ws is not None


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("lim", [4, 1], ids=["wide", "narrow"])
@pytest.mark.parametrize("wc", CC.WGRAD_CASES, ids=lambda c: c.id)
def test_exact_wgrad(ops, lib, wc, lim, det):
    """fp32 dw equals the integer reference for every kernel, pixel-range split, atomics or workspace, and with the
    reduction deferred to combat_conv_wgrad_reduce -- in both settings of combat_set_deterministic (on: every split
    launch needs its workspace, and a 3x3 launch with a prologue takes the generic kernel)."""
    b = CC.wgrad_build(wc, lim, DEV)
    before = lib.combat_get_deterministic()
    lib.combat_set_deterministic(det)
    try:
        for split, use_ws in wc.variants:
            name = "%s split=%d workspace=%s deterministic=%d" % (wc.id, split, use_ws, det)
            had_ws = launch_wgrad(ops, lib, b, split, use_ws or bool(det), name)
            if had_ws and split >= 0:
                launch_wgrad(ops, lib, b, split, True, name + " defer_reduce", defer=True)
    finally:
        lib.combat_set_deterministic(before)


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "deterministic"])
def test_exact_wgrad_reduce_first_chain(ops, lib, det):
    """Three weight-gradient launches of different shapes, each leaving its slabs (defer_reduce) for the next one to
    fold into the earlier dw first (reduce_first); the last one reduced by combat_conv_wgrad_reduce: every dw exact."""
    st = torch.cuda.current_stream().cuda_stream
    before = lib.combat_get_deterministic()
    lib.combat_set_deterministic(det)
    try:
        built, prev, keep = [], None, []
        for i, (n, hw, c, k) in enumerate(CC.CHAIN_SHAPES):
            b = CC.wgrad_build(CC.WCase("chain%d" % i, n, hw, c, k, 3, 1), 4, DEV)
            dw = R.Guarded(b.shape, torch.float32, "dst", DEV, zero=True)
            need = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(CC.wgrad_args(b, dw))))
            assert need > 0, i
            ws = R.Guarded((need,), torch.uint8, "dst", DEV)
            a = CC.wgrad_args(b, dw, 0, ws, defer=1, first=prev)
            ops.check(lib.combat_conv_wgrad(ctypes.byref(a), st), "combat_conv_wgrad", "chain %d" % i)
            built.append((b, dw, ws))
            keep.append(a)
            prev = a
        ops.check(lib.combat_conv_wgrad_reduce(ctypes.byref(prev), st), "combat_conv_wgrad_reduce", "chain end")
        torch.cuda.synchronize()
        for i, (b, dw, ws) in enumerate(built):
            dw.check("dw of chain %d" % i)
            ws.check("workspace of chain %d" % i)
            R.report_mismatch(dw.t.double().cpu(), b.exp, "dw of chain launch %d" % i)
    finally:
        lib.combat_set_deterministic(before)


# ------------------------------------------------------------------------------------------------ Gaussian data, bound
def rb(x):
    return x.to(bf16).double()


def randn(shape, seed, scale=1.0):
    return torch.randn(tuple(shape), generator=R.gen(seed)) * scale


GAUSS_CASES = [
    # name, n, hw, c, k, r, stride, mode, tile, expect, features
    ("t01", 2, 16, 128, 128, 3, 1, 0, 1, 1, ""), ("t02", 3, 10, 64, 64, 3, 2, 0, 2, 2, "post"),
    ("t03", 4, 16, 64, 128, 3, 2, 1, 3, 3, "mask+mul"), ("t04", 5, 16, 64, 3, 3, 1, 0, 4, 4, "bias"),
    ("t05", 3, 5, 64, 128, 3, 1, 0, 5, 5, ""), ("t06", 3, 8, 64, 64, 3, 1, 0, 6, 6, "post"),
    ("t07", 3, 8, 128, 128, 3, 1, 1, 7, 7, ""), ("t08-unet-instnorm-prologue-bias", 5, 16, 64, 64, 3, 1, 0, 8, 8, "proimg+bias"),
    ("t09-unet-instnorm-prologue-bias-4x4", 9, 4, 256, 256, 3, 1, 0, 9, 9, "proimg+bias"),
    ("t10", 5, 8, 128, 64, 3, 1, 0, 10, 10, "post"), ("t10-mask", 5, 8, 128, 64, 3, 1, 1, 10, 10, "mask+mul+pre"),
    ("t11", 9, 4, 512, 512, 3, 1, 0, 11, 11, ""), ("t12", 6, 64, 64, 256, 3, 2, 0, 0, 12, ""),
    ("t13", 5, 6, 64, 64, 3, 2, 1, 13, 13, "post"), ("t14", 7, 8, 128, 64, 3, 1, 0, 14, 14, ""),
    ("t15-hilo-stem", 3, 10, 3, 64, 3, 2, 0, 0, 15, "bias"), ("t16", 3, 16, 128, 128, 3, 1, 1, 16, 16, ""),
    ("t17", 3, 32, 64, 64, 3, 1, 0, 17, 17, "post"),
    ("t18-tanh_out-instnorm-prologue-bias", 5, 16, 64, 3, 3, 1, 0, 0, 18, "proimg+bias+tanh"),
    ("t18-stem-gradient", 3, 16, 3, 64, 3, 1, 1, 0, 18, ""),
    ("t13-src2-shortcut", 4, 16, 128, 256, 3, 2, 1, 0, 13, "src2+mask+mul"),
    ("t13-split-workspace", 16, 2, 512, 512, 3, 1, 0, 0, 13, "ws+post"),
    ("t13-src2-split-workspace", 3, 8, 256, 512, 3, 2, 1, 0, 13, "src2+ws"),
]


@pytest.mark.parametrize("name,n,hw,c,k,r,stride,mode,tile,expect,feat", GAUSS_CASES, ids=[g[0] for g in GAUSS_CASES])
def test_bound_gaussian(ops, lib, name, n, hw, c, k, r, stride, mode, tile, expect, feat):
    """One case per tile id on Gaussian data: non-dyadic scales, tanh, real accumulation error.  The prologue is the
    kernels' documented arithmetic restated (fmaf, leaky activation in fp32, bf16 operand), so no intermediate-rounding
    term is needed; tanh_out adds (1 - t^2) E + 2^-21 (eight fp32 ulps at 1.0 for tanhf itself)."""
    f = set(feat.split("+")) if feat else set()
    pad = 1 if r == 3 else 0
    c_pad, k_pad = (8 if c == 3 else c), CC.round_up(k, 8)
    p = (hw + 2 * pad - r) // stride + 1
    w = rb(randn((k, c, r, r), 11, 1.0 / math.sqrt(c * r * r)))
    pc = CC.packed(ops, w, stride, pad, c_pad, c == 3, DEV)
    pro = None
    if mode == 0:
        if c == 3:      # hi/lo split image: channels 0..2 = bf16(x), 3..5 = bf16(x - bf16(x))
            img = torch.rand(n, 3, hw, hw, generator=R.gen(12)).double() * 2 - 1
            hi = rb(img)
            lo = rb(img - hi)
            x = torch.cat([hi, lo, torch.zeros(n, 2, hw, hw, dtype=torch.float64)], 1)
            x_eff = hi + lo
        else:
            x = x_eff = rb(randn((n, c, hw, hw), 12))
        if "proimg" in f:
            psc, psh = torch.rand(n, c, generator=R.gen(13)) + 0.5, randn((n, c), 14, 0.3)
            x_eff = R.prologue(x, psc.double(), psh.double(), True, 0.2)
            pro = ops.Affine(psc.to(DEV), psh.to(DEV), c, True, 0.2)
        ref = CC.pad_channels(R.conv_fwd(x_eff, w, stride, pad), k_pad)
        mag = CC.pad_channels(R.conv_fwd(x_eff.abs(), w.abs(), stride, pad), k_pad)
        src, oshape, real, terms = x, (n, k_pad, p, p), k, r * r * c * (2 if c == 3 else 1)
    else:
        dy = rb(randn((n, k, p, p), 12))
        ref = CC.pad_channels(R.conv_dgrad(dy, w, hw, stride, pad), c_pad)
        mag = CC.pad_channels(R.conv_dgrad(dy.abs(), w.abs(), hw, stride, pad), c_pad)
        src, oshape, real, terms = CC.pad_channels(dy, k_pad), (n, c_pad, hw, hw), c, r * r * k
    k_out = oshape[1]
    kw, ep = {}, {}
    if "src2" in f:     # the block's 1x1 / stride-2 shortcut as second reduction source: k more terms on the centre tap
        w1, dy1 = rb(randn((k, c, 1, 1), 21, 1.0 / math.sqrt(c))), rb(randn((n, k, p, p), 22))
        pc1 = CC.packed(ops, w1, 2, 0, c_pad, False, DEV)
        ref = ref + R.conv_dgrad(dy1, w1, hw, 2, 0)
        mag = mag + R.conv_dgrad(dy1.abs(), w1.abs(), hw, 2, 0)
        src2 = R.Guarded.source(CC.nhwc_bf16(dy1), DEV)
        kw["shortcut"] = (src2.t, pc1)
        terms += k
    if "bias" in f:
        bias = randn((k_out,), 15, 0.1).double()
        bias[real:] = 0
        ep["bias"], kw["bias"] = bias, bias.float().to(DEV)
    for nm, key, sd in (("pre", "add_pre", 16), ("post", "add_post", 17)):
        if nm in f:
            t = rb(randn(oshape, sd))
            ep[key], kw[key] = t, CC.nhwc_bf16(t).to(DEV)
    exclude = None
    if "mask" in f:
        mx = rb(randn(oshape, 18))
        msc, msh = (torch.rand(k_out, generator=R.gen(19)) - 0.3).double(), randn((k_out,), 20, 0.3).double()
        ep.update(mask_x=mx, mask_scale=msc.float().double(), mask_shift=msh.float().double(), mask_slope=0.0, mask_mul_scale=True)
        kw.update(mask_x=CC.nhwc_bf16(mx).to(DEV), mask=ops.Affine(msc.float().to(DEV), msh.float().to(DEV), 0, True, 0.0),
                  mask_mul_scale=True)
    v, emag, q = R.epilogue(ref, exact=False, **ep)
    if q is not None:   # an argument within its own rounding error of zero may take either branch: counted from the reference
        q64 = ep["mask_x"] * R.table(ep["mask_scale"]) + R.table(ep["mask_shift"])
        exclude = q64.abs() <= 2.0 ** -23 * ((ep["mask_x"] * R.table(ep["mask_scale"])).abs() + R.table(ep["mask_shift"]).abs())
        assert float(ep["mask_scale"].abs().max()) <= 1.0     # (the scale multiplied in shrinks the error: S stays a bound)
    if "tanh" in f:
        kw["tanh_out"] = True
    dst = R.Guarded((n, oshape[2], oshape[3], k_out), bf16, "dst", DEV)
    srcg = R.Guarded.source(CC.nhwc_bf16(src), DEV)
    a = ops.conv_args(srcg.t, dst.t, pc, mode, pro=pro, tile=tile, **kw)
    ws = None
    if "ws" in f:
        need = int(lib.combat_conv_workspace_bytes(ctypes.byref(a)))
        assert need > 0
        ws = R.Guarded((need,), torch.uint8, "dst", DEV)
        a.workspace, a.workspace_bytes = ws.t.data_ptr(), need
    assert lib.combat_conv_pick_tile(ctypes.byref(a)) == expect
    ops.conv_launch(a)
    torch.cuda.synchronize()
    dst.check("dst of " + name)
    if ws is not None:
        ws.check("workspace of " + name)
    R.assert_within_bound(CC.from_nhwc(dst.t), v, mag + emag, terms, name, tanh="tanh" in f, exclude=exclude, tile=expect)


GAUSS_WGRAD = [CC.WGRAD_CASES[i] for i in (0, 1, 5, 9, 12, 14, 15)]


@pytest.mark.parametrize("wc", GAUSS_WGRAD, ids=lambda c: c.id)
def test_bound_gaussian_wgrad(ops, lib, wc):
    """One case per weight-gradient kernel on Gaussian data: every fp32 element within E = (T + 4) 2^-24 S of the fp64
    reference, T = the number of pixels summed, S = sum |x||dy| -- the gate these sums had before was rel-L2 2e-3."""
    n, hw, c, k, r, stride = wc.n, wc.hw, wc.c, wc.k, wc.r, wc.stride
    pad = 1 if r == 3 else 0
    c_pad, k_pad = (8 if c == 3 else c), CC.round_up(k, 8)
    p = (hw + 2 * pad - r) // stride + 1
    dy = rb(randn((n, k, p, p), 31))
    if c == 3:
        img = torch.rand(n, 3, hw, hw, generator=R.gen(32)).double() * 2 - 1
        hi = rb(img)
        lo = rb(img - hi)
        x = torch.cat([hi, lo, torch.zeros(n, 2, hw, hw, dtype=torch.float64)], 1)
        x_eff = hi + lo
    else:
        x = x_eff = rb(randn((n, c, hw, hw), 32))
    pro = None
    if wc.pro:
        shape = (n, c) if wc.pro == "img" else (c,)
        psc, psh = torch.rand(shape, generator=R.gen(33)) + 0.5, randn(shape, 34, 0.3)
        x_eff = R.prologue(x, psc.double(), psh.double(), True, 0.2)
        pro = ops.Affine(psc.to(DEV), psh.to(DEV), c if wc.pro == "img" else 0, True, 0.2)
    from types import SimpleNamespace
    b = SimpleNamespace(src=R.Guarded.source(CC.nhwc_bf16(x), DEV), dy=R.Guarded.source(CC.nhwc_bf16(CC.pad_channels(dy, k_pad)), DEV),
                        pro=pro, shape=(k, r * r, c), r=r, stride=stride, pad=pad, k=k, c=c)
    ref = R.conv_wgrad(x_eff, dy, k, r, stride, pad)
    mag = R.conv_wgrad(x_eff.abs(), dy.abs(), k, r, stride, pad)
    st = torch.cuda.current_stream().cuda_stream
    for split, use_ws in wc.variants[:2]:
        dw = R.Guarded(b.shape, torch.float32, "dst", DEV, zero=True)
        need = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(CC.wgrad_args(b, dw, split))))
        ws = R.Guarded((need,), torch.uint8, "dst", DEV) if (use_ws and need) else None
        ops.check(lib.combat_conv_wgrad(ctypes.byref(CC.wgrad_args(b, dw, split, ws)), st), "combat_conv_wgrad", wc.id)
        torch.cuda.synchronize()
        dw.check("dw of " + wc.id)
        R.assert_within_bound(dw.t.double().cpu(), ref, mag, n * p * p * (2 if c == 3 else 1), "%s split=%d" % (wc.id, split),
                              stored_bf16=False)
