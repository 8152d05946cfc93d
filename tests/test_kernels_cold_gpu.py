"""The counted-wait convolution kernels in the state the training step puts them in: caches evicted, queued directly
behind a large kernel -- not warm and alone as in test_kernels_gpu.py.

Both known breaks of the counted vmcnt waits gave wrong values on about
half the elements of SOME launches of a step while 2 800 isolated launches were right: a weight tile read before it
had landed is only wrong when the load is slow.  So every case here

  1. launches warm once and checks that result against the fp32 CPU reference of the same operator at the bounds of
     test_kernels_gpu.py (bf16 outputs 4e-3, fp32 weight gradients 2e-3, statistics 1e-4), so that "cold equals warm"
     cannot pass with both wrong;
  2. then three times (a fixed count, no retry): poisons the outputs (7.0; statistics and accumulated weight
     gradients zeroed), evicts L2 and the Infinity Cache with an add_(1) over 768 MiB on the launch stream -- no host
     synchronisation between the eviction and the launch -- launches, synchronises and compares with the warm
     result: bit for bit where the launch is deterministic (forward, input gradient, statistics rows), rel-L2 <= 1e-6
     where fp32 atomics order the sum (split reductions; weight gradients outside the carried reduction).

All cases are at N = 128, where the grids fill the chip and the dispatcher takes its production branches.  The CPU
references are computed once per shape and shared by tiles and launch forms.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import B128_SHAPES, LDS_PRO_CASES, bf16, dev, g, make_conv, nchw, nhwc, rb, rel_l2

pytestmark = pytest.mark.gpu

N = 128
POISON = 7.0
ROUNDS = 3
EVICT_BYTES = 768 << 20     # three times the 256 MiB Infinity Cache plus all the L2s (tools/conv_bench.py::flush_caches)


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


@pytest.fixture(scope="module")
def evict():
    buf = torch.zeros(EVICT_BYTES, dtype=torch.uint8, device="cuda")

    def run():
        buf.add_(1)     # on the current stream: the launch under test queues directly behind it

    yield run
    del buf
    torch.cuda.empty_cache()


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bc(v):      # per-channel vector against NCHW
    return v.view(1, -1, 1, 1)


class Out:
    """One tensor a launch writes.  exact: compared bit for bit (else rel-L2 <= 1e-6); zero: cleared, not poisoned,
    before a launch (statistics rows, accumulated weight gradients)."""

    def __init__(self, t, exact=True, zero=False):
        self.t, self.exact, self.zero = t, exact, zero

    def reset(self):
        if self.zero:
            self.t.zero_()
        else:
            self.t.fill_(POISON)


def warm_then_cold(label, outs, launch, evict, check_warm):
    """The protocol of the module docstring.  outs: {name: Out}; launch(): queues the launch(es) under test;
    check_warm(): asserts the warm result against the CPU reference."""
    for o in outs.values():
        o.reset()
    launch()
    torch.cuda.synchronize()
    warm = {k: o.t.clone() for k, o in outs.items()}
    check_warm()
    for rnd in range(ROUNDS):
        for o in outs.values():
            o.reset()
        evict()
        launch()
        torch.cuda.synchronize()
        for k, o in outs.items():
            if o.exact:
                if not torch.equal(o.t, warm[k]):
                    diff = o.t != warm[k]
                    raise AssertionError("%s: cold round %d, output '%s': %d of %d elements differ from the warm launch, %d of them still "
                                         "hold the poison" % (label, rnd, k, int(diff.sum()), diff.numel(),
                                                              int((diff & (o.t == POISON)).sum())))
            else:
                err = rel_l2(o.t, warm[k])
                if not err <= 1e-6:
                    diff = o.t != warm[k]
                    raise AssertionError("%s: cold round %d, output '%s': rel-L2 %.3g to the warm launch (bound 1e-6), %d of %d elements "
                                         "differ, %d of them still hold the poison" % (label, rnd, k, err, int(diff.sum()), diff.numel(),
                                                                                       int((diff & (o.t == POISON)).sum())))


def with_stats(ops, a, k, outs, exact=True):
    rows, rpi = ops.conv_stats_layout(a)
    st = torch.zeros(rows, 2, k, device="cuda")
    a.stats = st.data_ptr()
    outs["stats"] = Out(st, exact, zero=True)
    return st


# ------------------------------------------------------------------------------------------ ring / weight-stationary
RING_SHAPES = [(hw, c, k) for hw, c, k, r, s in B128_SHAPES if r == 3 and s == 1 and c >= 64 and k >= 64]
# The forced tiles' geometry (conv3x3_dma.hip geo_tw / geo_th): 2 x 2 maps have no DMA-staged tile at all, the 64-pixel
# wave tile 16 needs 16-wide tiles (maps >= 16), the 256-pixel tile 14 does not exist on 4 x 4 maps.  Every pair listed
# here must be PICKED (asserted below); a pair not listed is one combat_conv_pick_tile refuses (asserted as well).
RING_CASES = [(t, hw, c, k) for hw, c, k in RING_SHAPES for t in (10, 11, 14, 16)
              if (t in (10, 11) and hw >= 4) or (t == 14 and hw >= 8) or (t == 16 and hw >= 16)] + [(17, 32, 64, 64)]
RING_REFUSED = [(t, hw, c, k) for hw, c, k in RING_SHAPES for t in (10, 11, 14, 16) if (t, hw, c, k) not in RING_CASES]
FORMS = ("plain+residual", "activated output", "activated output only", "statistics", "eval backward", "train backward")


def ring_operands(hw, c, k):
    """CPU tensors and the two base references of one shape (shared by tiles and forms)."""
    def make():
        o = dict(x=rb(torch.randn(N, c, hw, hw, generator=g(41))), dy=rb(torch.randn(N, k, hw, hw, generator=g(42))),
                 res_k=rb(torch.randn(N, k, hw, hw, generator=g(43))), res_c=rb(torch.randn(N, c, hw, hw, generator=g(50))),
                 xact=rb(torch.relu(torch.randn(N, c, hw, hw, generator=g(44)))), xpre=rb(torch.randn(N, c, hw, hw, generator=g(51))))
        for tag, ch, s in (("k", k, 45), ("c", c, 52)):
            o["sc_" + tag] = (torch.rand(ch, generator=g(s)) + 0.5) * torch.where(torch.rand(ch, generator=g(s + 1)) < 0.2, -1.0, 1.0)
            o["sh_" + tag] = torch.randn(ch, generator=g(s + 2)) * 0.3
        o["mean"], o["rstd"] = torch.randn(c, generator=g(48)) * 0.1, torch.rand(c, generator=g(49)) + 0.5
        o["w"] = torch.randn(k, c, 3, 3, generator=g(40)) * (1.0 / (c * 9) ** 0.5)
        o["fwd"] = F.conv2d(o["x"], rb(o["w"]), padding=1)
        o["dgrad"] = torch.nn.grad.conv2d_input((N, c, hw, hw), rb(o["w"]), o["dy"], padding=1)
        return o
    return cached(("ring", hw, c, k), make)


def act_ref(stored, sc, sh):     # fused multiply-add (one rounding) of the STORED value, as the epilogue computes it
    return rb(torch.relu((stored.double() * bc(sc).double() + bc(sh).double()).float()))


@pytest.mark.parametrize("tile,hw,c,k", RING_CASES)
def test_ring_and_weight_stationary_kernels_cold(ops, evict, tile, hw, c, k):
    """conv3x3_dma_kernel (tiles 10, 11, 14, 16) and conv3x3_ws_kernel (17) in the six launch forms of
    test_conv3x3_weight_stationary_equals_ring_kernel, which together reach every one-flavour (FLX) instantiation."""
    from combat_amd._lib import lib
    o = ring_operands(hw, c, k)
    pc = ops.PackedConv(dev(o["w"]).contiguous(memory_format=torch.channels_last), 1, 1, c)
    pc.pack()
    x, dy, res_k, res_c, xact, xpre = (nhwc(o[n]) for n in ("x", "dy", "res_k", "res_c", "xact", "xpre"))
    aff_k = ops.Affine(dev(o["sc_k"]), dev(o["sh_k"]), 0, True, 0.0)
    aff_c = ops.Affine(dev(o["sc_c"]), dev(o["sh_c"]), 0, True, 0.0)
    mean, rstd = dev(o["mean"]), dev(o["rstd"])
    for form in FORMS:
        fwd = "backward" not in form
        ch = k if fwd else c
        y = torch.empty(N, hw, hw, ch, dtype=bf16, device="cuda")
        act = torch.empty(N, hw, hw, ch, dtype=bf16, device="cuda")
        outs = {"y": Out(y)}
        if form == "plain+residual":
            a = ops.conv_args(x, y, pc, 0, add_post=res_k, tile=tile)
        elif form == "activated output":
            a = ops.conv_args(x, y, pc, 0, add_post=res_k, act_dst=act, act=aff_k, tile=tile)
            outs["act"] = Out(act)
        elif form == "activated output only":
            a = ops.conv_args(x, None, pc, 0, act_dst=act, act=aff_k, tile=tile)
            outs = {"act": Out(act)}
        elif form == "statistics":
            a = ops.conv_args(x, y, pc, 0, add_post=res_k, stats_kind=1, tile=tile)
        elif form == "eval backward":
            a = ops.conv_args(dy, y, pc, 1, add_pre=res_c, mask_x=xact, mask=aff_c, mask_mul_scale=True, mask_activated=True,
                              add_post=res_c, tile=tile)
        else:
            a = ops.conv_args(dy, y, pc, 1, add_pre=res_c, mask_x=xpre, mask=aff_c, stats_kind=2, xh_mean=mean, xh_rstd=rstd, tile=tile)
        label = "tile %d, form '%s', %dx%dx%dx%d -> %d" % (tile, form, N, hw, hw, c, k)
        assert lib.combat_conv_pick_tile(ctypes.byref(a)) == tile, label
        stats = with_stats(ops, a, ch, outs) if a.stats_kind else None

        def check_warm():
            if form == "activated output only":
                assert rel_l2(nchw(act), act_ref(rb(o["fwd"]), o["sc_k"], o["sh_k"])) < 6e-3, label     # (from an unrounded y: as the warm test)
                return
            got = nchw(y)
            if fwd:
                assert rel_l2(got, o["fwd"] + o["res_k"]) < 4e-3, label
                if form == "activated output":      # exact: computed from the stored bf16 value
                    assert int((nchw(act) != act_ref(got, o["sc_k"], o["sh_k"])).sum()) <= 2, label
                if stats is not None:
                    s = stats.sum(0).cpu()
                    assert rel_l2(s[0], got.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got * got).sum((0, 2, 3))) < 1e-4, label
            elif form == "eval backward":
                ref = (o["dgrad"] + o["res_c"]) * (o["xact"] > 0).float() * bc(o["sc_c"]) + o["res_c"]
                assert rel_l2(got, ref) < 4e-3, label
            else:
                keep = ((o["xpre"] * bc(o["sc_c"]) + bc(o["sh_c"])) > 0).float()
                assert rel_l2(got, (o["dgrad"] + o["res_c"]) * keep) < 4e-3, label
                s = stats.sum(0).cpu()
                xhat = (o["xpre"] - bc(o["mean"])) * bc(o["rstd"])
                assert rel_l2(s[0], got.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got * xhat).sum((0, 2, 3))) < 1e-4, label

        warm_then_cold(label, outs, lambda: ops.conv_launch(a), evict, check_warm)


@pytest.mark.parametrize("tile,hw,c,k", RING_REFUSED)
def test_refused_ring_tiles_stay_refused(ops, tile, hw, c, k):
    """The (tile, shape) pairs left out above are exactly those the dispatcher refuses: if one starts to apply, it
    belongs in RING_CASES."""
    from combat_amd._lib import lib
    w, pc = make_conv(ops, k, c, 3, 1, 1, 40)
    x = torch.empty(N, hw, hw, c, dtype=bf16, device="cuda")
    a = ops.conv_args(x, torch.empty(N, hw, hw, k, dtype=bf16, device="cuda"), pc, 0, tile=tile)
    assert lib.combat_conv_pick_tile(ctypes.byref(a)) == 0


# ------------------------------------------------------------------------------------------ in-LDS prologue
@pytest.mark.parametrize("n,hw,c,k,tile", [case for case in LDS_PRO_CASES if case[0] == N])
def test_lds_prologue_kernel_cold(ops, evict, n, hw, c, k, tile):
    """conv3x3_dma_pro_kernel: BatchNorm + ReLU applied in LDS, with the activated side tensor (pro_act_dst), in the
    three epilogue forms of test_conv_lds_prologue_equals_norm_act_then_conv."""
    from combat_amd._lib import lib

    def make():
        o = dict(x=rb(torch.randn(n, c, hw, hw, generator=g(900)) * 1.5 + 0.3), res=rb(torch.randn(n, k, hw, hw, generator=g(901))),
                 w=torch.randn(k, c, 3, 3, generator=g(902)) * (1.0 / (c * 9) ** 0.5),
                 sc=(torch.rand(c, generator=g(903)) + 0.5) * torch.where(torch.rand(c, generator=g(904)) < 0.2, -1.0, 1.0),
                 sh=torch.randn(c, generator=g(905)) * 0.3)
        o["side"] = rb(torch.relu((o["x"].double() * bc(o["sc"]).double() + bc(o["sh"]).double()).float()))
        o["fwd"] = F.conv2d(o["side"], rb(o["w"]), padding=1)
        return o
    o = cached(("pro", hw, c, k), make)
    pc = ops.PackedConv(dev(o["w"]).contiguous(memory_format=torch.channels_last), 1, 1, c)
    pc.pack()
    x, res = nhwc(o["x"]), nhwc(o["res"])
    aff = ops.Affine(dev(o["sc"]), dev(o["sh"]), 0, True, 0.0)
    for form, kw in (("plain + residual", dict(add_post=res)), ("statistics + residual", dict(add_post=res, stats_kind=1 | 4)),
                     ("statistics", dict(stats_kind=1))):
        y = torch.empty(n, hw, hw, k, dtype=bf16, device="cuda")
        side = torch.empty_like(x)
        a = ops.conv_args(x, y, pc, 0, pro=aff, pro_act_dst=side, tile=tile, **kw)
        label = "prologue kernel, tile %d, form '%s', %dx%dx%dx%d -> %d" % (tile, form, n, hw, hw, c, k)
        assert lib.combat_conv_pick_tile(ctypes.byref(a)) == tile, label
        outs = {"y": Out(y), "side": Out(side)}
        stats = with_stats(ops, a, k, outs) if a.stats_kind else None

        def check_warm():
            got = nchw(y)
            assert rel_l2(nchw(side), o["side"]) < 4e-3, label
            assert rel_l2(got, o["fwd"] + (o["res"] if "add_post" in kw else 0)) < 4e-3, label
            if stats is not None:
                s = stats.sum(0).cpu()
                assert rel_l2(s[0], got.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got * got).sum((0, 2, 3))) < 1e-4, label

        warm_then_cold(label, outs, lambda: ops.conv_launch(a), evict, check_warm)


# ------------------------------------------------------------------------------------------ gather kernels
GATHER_SHAPES = [(hw, c, k) for hw, c, k, r, s in B128_SHAPES if r == 3 and s == 2 and c >= 64]
assert len(GATHER_SHAPES) == 6     # three of PreActResNet18, three of the UnetGenerator


def gather_operands(hw, c, k):
    def make():
        p = hw // 2
        o = dict(x=rb(torch.relu(torch.randn(N, c, hw, hw, generator=g(400)))), dy3=rb(torch.randn(N, k, p, p, generator=g(503))),
                 dy1=rb(torch.randn(N, k, p, p, generator=g(504))), xpre=rb(torch.randn(N, c, hw, hw, generator=g(505))),
                 w3=torch.randn(k, c, 3, 3, generator=g(401)) * (1.0 / (9 * c) ** 0.5), w1=torch.randn(k, c, 1, 1, generator=g(402)) * (1.0 / c ** 0.5),
                 sc=torch.rand(c, generator=g(506)) - 0.3, sh=torch.randn(c, generator=g(507)) * 0.3,
                 mean=torch.randn(c, generator=g(508)) * 0.1, rstd=torch.rand(c, generator=g(509)) + 0.5,
                 asc=torch.rand(k, generator=g(510)) + 0.5, ash=torch.randn(k, generator=g(511)))
        o["f3"] = F.conv2d(o["x"], rb(o["w3"]), stride=2, padding=1)
        o["f1"] = F.conv2d(o["x"], rb(o["w1"]), stride=2)
        o["g3"] = torch.nn.grad.conv2d_input((N, c, hw, hw), rb(o["w3"]), o["dy3"], stride=2, padding=1)
        o["g1"] = torch.nn.grad.conv2d_input((N, c, hw, hw), rb(o["w1"]), o["dy1"], stride=2, padding=0)
        return o
    return cached(("gather", hw, c, k), make)


@pytest.mark.parametrize("hw,c,k", GATHER_SHAPES)
def test_gather_kernels_cold(ops, evict, hw, c, k):
    """conv_gather_dma*: the stride-2 3x3 forward with statistics, the 1x1 stride-2 shortcut, the stride-2 input
    gradient plain and with the shortcut as second source (mask + norm-backward sums), and the paired launch.  A
    skinny layer given a workspace splits its reduction; such a launch is compared at 1e-6."""
    from combat_amd._lib import lib
    o = gather_operands(hw, c, k)
    p = hw // 2
    pc3 = ops.PackedConv(dev(o["w3"]).contiguous(memory_format=torch.channels_last), 2, 1, c)
    pc1 = ops.PackedConv(dev(o["w1"]).contiguous(memory_format=torch.channels_last), 2, 0, c)
    pc3.pack()
    pc1.pack()
    x, dy3, dy1, xpre = (nhwc(o[n]) for n in ("x", "dy3", "dy1", "xpre"))
    ws = torch.empty(32 << 20, dtype=torch.uint8, device="cuda")
    where = "%dx%dx%dx%d -> %d" % (N, hw, hw, c, k)

    def fwd_case(name, pc, ref, stats_on):
        y = torch.empty(N, p, p, k, dtype=bf16, device="cuda")
        a = ops.conv_args(x, y, pc, 0, stats_kind=1 if stats_on else 0, workspace=ws)
        label = "gather kernel, %s, %s" % (name, where)
        assert lib.combat_conv_pick_tile(ctypes.byref(a)) in (12, 13), label
        exact = not a.workspace
        outs = {"y": Out(y, exact)}
        stats = with_stats(ops, a, k, outs, exact) if stats_on else None

        def check_warm():
            got = nchw(y)
            assert rel_l2(got, ref) < 4e-3, label
            if stats is not None:
                s = stats.sum(0).cpu()
                assert rel_l2(s[0], got.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got * got).sum((0, 2, 3))) < 1e-4, label

        warm_then_cold(label, outs, lambda: ops.conv_launch(a), evict, check_warm)

    fwd_case("3x3 stride-2 forward + statistics", pc3, o["f3"], True)
    fwd_case("1x1 stride-2 shortcut", pc1, o["f1"], False)

    # input gradient, plain
    dx = torch.empty(N, hw, hw, c, dtype=bf16, device="cuda")
    a = ops.conv_args(dy3, dx, pc3, 1, workspace=ws)
    label = "gather kernel, stride-2 input gradient, " + where
    assert lib.combat_conv_pick_tile(ctypes.byref(a)) in (12, 13), label

    def check_plain():
        assert rel_l2(nchw(dx), o["g3"]) < 4e-3, label

    warm_then_cold(label, {"dx": Out(dx, not a.workspace)}, lambda: ops.conv_launch(a), evict, check_plain)

    # input gradient with the shortcut as second source, mask + norm-backward sums in the epilogue
    dx2 = torch.empty(N, hw, hw, c, dtype=bf16, device="cuda")
    a2 = ops.conv_args(dy3, dx2, pc3, 1, mask_x=xpre, mask=ops.Affine(dev(o["sc"]), dev(o["sh"]), 0, True, 0.0), stats_kind=2,
                       xh_mean=dev(o["mean"]), xh_rstd=dev(o["rstd"]), workspace=ws, shortcut=(dy1, pc1))
    label2 = "gather kernel, stride-2 input gradient with the shortcut as second source, " + where
    assert lib.combat_conv_pick_tile(ctypes.byref(a2)) in (12, 13), label2
    exact2 = not a2.workspace
    outs2 = {"dx": Out(dx2, exact2)}
    stats2 = with_stats(ops, a2, c, outs2, exact2)

    def check_src2():
        got = nchw(dx2)
        keep = (o["xpre"] * bc(o["sc"]) + bc(o["sh"])) > 0
        gin = o["g3"] + o["g1"]
        assert rel_l2(got, torch.where(keep, gin, torch.zeros_like(gin))) < 4e-3, label2
        s = stats2.sum(0).cpu()
        xhat = (o["xpre"] - bc(o["mean"])) * bc(o["rstd"])
        assert rel_l2(s[0], got.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got * xhat).sum((0, 2, 3))) < 1e-4, label2

    warm_then_cold(label2, outs2, lambda: ops.conv_launch(a2), evict, check_src2)

    # the paired launch: 3x3 (statistics + activated output) and the 1x1 shortcut over the same input
    y3 = torch.empty(N, p, p, k, dtype=bf16, device="cuda")
    a3t, y1 = torch.empty_like(y3), torch.empty_like(y3)
    pa = ops.conv_args(x, y3, pc3, 0, stats_kind=1, act_dst=a3t, act=ops.Affine(dev(o["asc"]), dev(o["ash"]), 0, True, 0.0))
    outs3 = {"y3": Out(y3), "act3": Out(a3t), "y1": Out(y1)}
    st3 = with_stats(ops, pa, k, outs3)
    pb = ops.conv_args(x, y1, pc1, 0)
    label3 = "gather kernel, paired launch, " + where
    assert lib.combat_conv_pick_tile(ctypes.byref(pa)) in (12, 13) and lib.combat_conv_pick_tile(ctypes.byref(pb)) in (12, 13), label3

    def check_pair():
        got = nchw(y3)
        assert rel_l2(got, o["f3"]) < 4e-3 and rel_l2(nchw(y1), o["f1"]) < 4e-3, label3
        assert rel_l2(nchw(a3t), act_ref(got, o["asc"], o["ash"])) < 4e-3, label3
        s = st3.sum(0).cpu()
        assert rel_l2(s[0], got.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got * got).sum((0, 2, 3))) < 1e-4, label3

    warm_then_cold(label3, outs3, lambda: ops.check(lib.combat_conv_gemm_pair(ctypes.byref(pb), ctypes.byref(pa), _stream()), "pair"),
                   evict, check_pair)


# ------------------------------------------------------------------------------------------ weight gradient
def wgrad_args(x, dy, dw, k, c, ws=None, defer=0, first=None):
    from combat_amd._lib import WgradArgs
    a = WgradArgs()
    a.N, a.H, a.W, a.C = x.shape
    _, a.P, a.Q, a.K = dy.shape
    a.R = a.S = 3
    a.stride, a.pad = 1, 1
    a.src, a.dy, a.dw, a.k_real, a.c_real = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), k, c
    if ws is not None:
        a.workspace, a.workspace_bytes, a.defer_reduce = ws.data_ptr(), ws.numel(), defer
    if first is not None:
        a.reduce_first = ctypes.addressof(first)
    return a


def wgrad_ref(hw, c, k):
    def make():
        o = ring_operands(hw, c, k)
        return torch.nn.grad.conv2d_weight(o["xact"], (k, c, 3, 3), o["dy"], padding=1).permute(0, 2, 3, 1).reshape(k, 9, c)
    return cached(("wgrad", hw, c, k), make)


@pytest.mark.parametrize("hw,c,k", RING_SHAPES)
def test_wgrad3x3_dma_kernel_cold(ops, evict, hw, c, k):
    """conv_wgrad3x3_dma with a slab workspace (what the engines pass): partial sums by plain stores, then the
    stand-alone reduction, which orders its sum with fp32 atomics: 1e-6."""
    from combat_amd._lib import lib
    o = ring_operands(hw, c, k)
    x, dy = nhwc(o["xact"]), nhwc(o["dy"])
    dw = torch.zeros(k, 9, c, device="cuda")
    need = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(wgrad_args(x, dy, dw, k, c))))
    label = "weight gradient, %dx%dx%dx%d -> %d" % (N, hw, hw, c, k)
    assert need > 0, label      # (no slab workspace offered: not the DMA-staged weight-gradient kernel)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    a = wgrad_args(x, dy, dw, k, c, ws)

    def check_warm():
        assert rel_l2(dw, wgrad_ref(hw, c, k)) < 2e-3, label

    warm_then_cold(label, {"dw": Out(dw, exact=False, zero=True)}, lambda: ops.check(lib.combat_conv_wgrad(ctypes.byref(a), _stream()), "wgrad"),
                   evict, check_warm)


def test_wgrad_carried_reduction_chain_cold(ops, evict):
    """Three layers whose slabs ride in the next launch (reduce_first): the carried reduction has a fixed order and no
    atomics, so the first two weight gradients are compared bit for bit; the last gets the stand-alone reduction."""
    from combat_amd._lib import lib
    shapes = [(32, 64, 64), (16, 128, 128), (8, 256, 256)]
    layers, need = [], 4
    for hw, c, k in shapes:
        o = ring_operands(hw, c, k)
        x, dy, dw = nhwc(o["xact"]), nhwc(o["dy"]), torch.zeros(k, 9, c, device="cuda")
        nb = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(wgrad_args(x, dy, dw, k, c))))
        assert nb > 0, (hw, c, k)
        need = max(need, nb)
        layers.append((x, dy, dw, k, c))
    regions = [torch.empty(need, dtype=torch.uint8, device="cuda") for _ in range(2)]
    args, prev = [], None
    for i, (x, dy, dw, k, c) in enumerate(layers):
        prev = wgrad_args(x, dy, dw, k, c, regions[i % 2], defer=1, first=prev)
        args.append(prev)

    def launch():
        for i, a in enumerate(args):
            ops.check(lib.combat_conv_wgrad(ctypes.byref(a), _stream()), "wgrad chain %d" % i)
        ops.check(lib.combat_conv_wgrad_reduce(ctypes.byref(args[-1]), _stream()), "last reduce")

    def check_warm():
        for (hw, c, k), layer in zip(shapes, layers):
            assert rel_l2(layer[2], wgrad_ref(hw, c, k)) < 2e-3, (hw, c, k)

    outs = {"dw%d" % i: Out(layer[2], exact=i + 1 < len(layers), zero=True) for i, layer in enumerate(layers)}
    warm_then_cold("carried weight-gradient reduction, three layers", outs, launch, evict, check_warm)


# ------------------------------------------------------------------------------------------ back to back
@pytest.mark.parametrize("net,hw,ch", [("PreActResNet18", 32, 64), ("UnetGenerator", 16, 64)])
def test_block_chain_cold(ops, evict, net, hw, ch):
    """One pre-activation block's launches queued back to back behind a single eviction, no host synchronisation in
    between: convolution + statistics, combat_norm_act_fused, the in-LDS-prologue convolution, then the block's input
    and weight gradients -- different kernels, cold, as only the engine tests reach today."""
    from combat_amd._lib import lib
    c = k = ch
    o = ring_operands(hw, c, k)
    pc = ops.PackedConv(dev(o["w"]).contiguous(memory_format=torch.channels_last), 1, 1, c)
    pc.pack()
    x, dy = nhwc(o["x"]), nhwc(o["dy"])
    gamma, beta = dev(o["sc_k"]), dev(o["sh_k"])
    m = N * hw * hw
    y1, y2, side, dx = (torch.empty(N, hw, hw, k, dtype=bf16, device="cuda") for _ in range(4))
    act = torch.empty_like(y1)
    dw = torch.zeros(k, 9, c, device="cuda")
    mean, rstd, scale, shift = (torch.zeros(k, device="cuda") for _ in range(4))
    scratch = torch.zeros(ops.norm_scratch_bytes(1, k) // 4, device="cuda")
    outs = {"y1": Out(y1), "act": Out(act), "y2": Out(y2), "side": Out(side), "dx": Out(dx), "dw": Out(dw, exact=False, zero=True),
            "mean": Out(mean), "rstd": Out(rstd), "scale": Out(scale), "shift": Out(shift)}
    a1 = ops.conv_args(x, y1, pc, 0, stats_kind=1)
    st1 = with_stats(ops, a1, k, outs)
    parts = st1.shape[0]
    a2 = ops.conv_args(y1, y2, pc, 0, pro=ops.Affine(scale, shift, 0, True, 0.0), pro_act_dst=side, stats_kind=1)
    st2 = torch.zeros(ops.conv_stats_layout(a2)[0], 2, k, device="cuda")
    a2.stats = st2.data_ptr()
    outs["stats2"] = Out(st2, zero=True)
    a3 = ops.conv_args(dy, dx, pc, 1)
    need = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(wgrad_args(side, dy, dw, k, c))))
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    a4 = wgrad_args(side, dy, dw, k, c, ws if need else None)
    label = "%s block chain, %dx%dx%dx%d" % (net, N, hw, hw, c)
    assert lib.combat_conv_pick_tile(ctypes.byref(a1)) in (10, 11, 17) and lib.combat_conv_pick_tile(ctypes.byref(a2)) in (10, 11), label
    assert lib.combat_conv_pick_tile(ctypes.byref(a3)) in (10, 11, 17), label

    def launch():
        ops.conv_launch(a1)
        ops.check(lib.combat_norm_act_fused(y1.data_ptr(), st1.data_ptr(), 1, parts, m, k, 1e-5, 0.0, gamma.data_ptr(), beta.data_ptr(),
                                            mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None, 0.1, None,
                                            scratch.data_ptr(), scratch.numel() * 4, act.data_ptr(), _stream()), "norm_act_fused")
        ops.conv_launch(a2)
        ops.conv_launch(a3)
        ops.check(lib.combat_conv_wgrad(ctypes.byref(a4), _stream()), "wgrad")

    def check_warm():
        got1 = nchw(y1)
        assert rel_l2(got1, o["fwd"]) < 4e-3, label
        mu, var = got1.mean((0, 2, 3)), got1.var((0, 2, 3), unbiased=False)
        assert rel_l2(mean, mu) < 1e-4 and rel_l2(rstd, 1.0 / torch.sqrt(var + 1e-5)) < 1e-4, label
        assert torch.equal(side, act), label        # the in-LDS prologue against the materialised activation: same bits
        xa = rb(torch.relu(got1 * bc(scale.cpu()) + bc(shift.cpu())))
        assert rel_l2(nchw(side), xa) < 4e-3, label
        got2 = nchw(y2)
        assert rel_l2(got2, F.conv2d(xa, rb(o["w"]), padding=1)) < 4e-3, label
        s = st2.sum(0).cpu()
        assert rel_l2(s[0], got2.sum((0, 2, 3))) < 1e-4 and rel_l2(s[1], (got2 * got2).sum((0, 2, 3))) < 1e-4, label
        assert rel_l2(nchw(dx), o["dgrad"]) < 4e-3, label
        dw_ref = torch.nn.grad.conv2d_weight(nchw(side), (k, c, 3, 3), o["dy"], padding=1).permute(0, 2, 3, 1).reshape(k, 9, c)
        assert rel_l2(dw, dw_ref) < 2e-3, label

    warm_then_cold(label, outs, launch, evict, check_warm)
