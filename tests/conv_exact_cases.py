"""Case tables of tests/test_conv_exact_gpu.py and the builder that turns a case into launch arguments plus the exact
expectation (tests/conv_exact_ref.py).  The builder works on any device: tests/test_conv_exact_cpu.py runs it on the
CPU, where everything but the launch itself is checked -- the range condition, the share of outputs that need
rounding, and (combat_conv_pick_tile is host code) that each case reaches the kernel it is meant for.

A case's convolution is c -> k channels, r x r, on hw x hw maps; mode 1 computes its input gradient.  c == 3 is the
8-channel hi/lo stem (dup_hilo weights, channels 6..7 carry values the zero weights must drop); k == 3 is padded to
8 output channels.  `lim` is the lattice half-width: 4 (wide) by default, 16 for reductions so short (a few dozen
terms) that [-4, 4] would never reach the tie range [256, 512) -- products stay exact (<= 256), the range condition
is asserted all the same -- and 1 (narrow) for the statistics cases.
"""
import ctypes
from dataclasses import dataclass
from types import SimpleNamespace

import torch

import conv_exact_ref as R

bf16 = torch.bfloat16


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    hw: int
    c: int
    k: int
    r: int
    stride: int
    mode: int            # 0 forward, 1 input gradient
    tile: int            # forced tile (0: automatic)
    expect: int          # the tile combat_conv_pick_tile must report
    feat: tuple = ()
    lim: int = 4

    @property
    def id(self):
        return "t%02d-%s-%s%s" % (self.expect, "dgrad" if self.mode else "fwd", self.name,
                                  ("-" + "+".join(self.feat)) if self.feat else "")


def _both(name, n, hw, c, k, r, stride, tile, expect, lim=4, lim_bwd=None):
    return [Case(name, n, hw, c, k, r, stride, m, tile, expect, (), lim_bwd if m and lim_bwd else lim) for m in (0, 1)]


# ---- plain forward and input gradient on every tile id ------------------------------------------------------
PLAIN_CASES = (
    # generic gather tiles 1-5 (forced: the automatic choice prefers the DMA kernels)
    _both("128x128", 2, 16, 128, 128, 3, 1, 1, 1)
    + _both("128x64-stride2-3x3-odd5-raggedN", 3, 10, 64, 64, 3, 2, 2, 2, lim_bwd=16)
    + [Case("64x64-stride2-1x1", 2, 12, 64, 64, 1, 2, 0, 3, 3, lim=16),
       Case("64x64-stride2-3x3-parity-classes", 4, 16, 64, 128, 3, 2, 1, 3, 3, lim=16),
       Case("128x16-K3-padded-to-8", 5, 16, 64, 3, 3, 1, 0, 4, 4),
       Case("128x16-stem-gradient", 2, 12, 3, 64, 3, 1, 1, 4, 4),
       Case("64x128-raggedN-odd5", 3, 5, 64, 128, 3, 1, 0, 5, 5),
       Case("64x128-raggedN-odd5", 3, 5, 128, 64, 3, 1, 1, 5, 5)]
    # halo tiles 6-9 (3x3 / stride 1, patch in LDS)
    + _both("H256x64", 2, 16, 64, 64, 3, 1, 6, 6)
    + _both("H256x64-4-images-per-tile-8x8-raggedN", 3, 8, 64, 64, 3, 1, 6, 6)
    + _both("H128x128-2-images-per-tile-8x8-raggedN", 3, 8, 128, 128, 3, 1, 7, 7)
    + _both("H128x64-2-images-per-tile-8x8-raggedN", 5, 8, 64, 64, 3, 1, 8, 8)
    + _both("H64x64-4-images-per-tile-4x4-raggedN", 9, 4, 128, 128, 3, 1, 9, 9)
    + _both("H64x64-16-images-per-tile-2x2-raggedN", 6, 2, 512, 512, 3, 1, 9, 9)
    # DMA-staged tiles 10, 11, 14, 16 and the weight-stationary persistent kernel 17
    + _both("D128x64-2-images-per-tile-8x8-raggedN", 5, 8, 128, 64, 3, 1, 10, 10)
    + _both("D128x64-8-images-per-tile-4x4-raggedN", 3, 4, 64, 64, 3, 1, 10, 10)
    + _both("D128x64-16wide", 3, 16, 128, 128, 3, 1, 10, 10)
    + _both("D128x32-8-images-per-tile-4x4-raggedN", 9, 4, 512, 512, 3, 1, 11, 11)
    + _both("D128x32-16wide", 2, 32, 64, 64, 3, 1, 11, 11)
    + _both("D256x64-4-images-per-tile-8x8-raggedN", 7, 8, 128, 64, 3, 1, 14, 14)
    + _both("D256x64-16wide", 3, 32, 64, 64, 3, 1, 14, 14)
    + _both("D256W64", 3, 32, 64, 64, 3, 1, 16, 16)
    + _both("D256W64-16x16", 3, 16, 128, 128, 3, 1, 16, 16)
    + _both("S128x64-1-tile-per-workgroup", 3, 32, 64, 64, 3, 1, 17, 17)
    + _both("S128x64-2-tiles-per-workgroup-n40", 40, 32, 64, 64, 3, 1, 17, 17)
    + [Case("S128x64-3-tiles-per-workgroup-n81", 81, 32, 64, 64, 3, 1, 0, 17, 17)]
    # gathered-DMA tiles 12 / 13
    + _both("G128x64-stride2-3x3", 6, 64, 64, 256, 3, 2, 0, 12)
    + _both("G128x32-stride2-3x3-odd6-raggedN", 5, 6, 64, 64, 3, 2, 13, 13, lim_bwd=16)
    + _both("G128x32-stride2-1x1", 3, 12, 64, 128, 1, 2, 13, 13, lim=16)
    + _both("G128x32-stride1-odd10", 2, 10, 64, 64, 3, 1, 13, 13)
    + _both("G128x32-stride1-odd5-raggedN", 3, 5, 64, 64, 3, 1, 13, 13)
    + _both("G128x32-16-images-per-tile-2x2-raggedN", 9, 2, 512, 512, 3, 1, 13, 13)
    # C = 8 kernel 15: the hi/lo stem with dup_hilo weights; input gradient of an 8-output-channel convolution
    + [Case("C8-hilo-stem-dup_hilo", 5, 32, 3, 64, 3, 1, 0, 0, 15, lim=16),
       Case("C8-hilo-stem-dup_hilo-stride2-odd10-raggedN", 3, 10, 3, 64, 3, 2, 0, 0, 15, lim=16),
       Case("C8-hilo-stem-dup_hilo-odd6-raggedN", 2, 6, 3, 64, 3, 1, 0, 15, 15, lim=16),
       Case("C8-gradient-of-8-channel-conv", 3, 16, 64, 8, 3, 1, 1, 15, 15, lim=16),
       Case("C8-gradient-of-8-channel-conv-odd6-raggedN", 2, 6, 64, 8, 3, 1, 1, 15, 15, lim=16)]
    # K8 kernel 18: eight output channels (K = 3 padded to 8; a stem's input gradient)
    + [Case("K8-K3-padded-to-8", 5, 16, 64, 3, 3, 1, 0, 0, 18),
       Case("K8-K3-padded-to-8-128ch", 2, 32, 128, 3, 3, 1, 0, 18, 18),
       Case("K8-stem-gradient", 3, 16, 3, 64, 3, 1, 1, 0, 18)]
    # the benchmarked batch, automatic tile: the dispatcher's thresholds on the workgroup count (4 tiles per persistent
    # workgroup, channel-tile-fastest / pixel-tile-fastest order, 32-channel tiles on skinny layers) are only reached here
    + _both("B128-automatic-4-tiles-per-workgroup", 128, 32, 64, 64, 3, 1, 0, 17)
    + _both("B128-automatic", 128, 16, 128, 128, 3, 1, 0, 10)
    + _both("B128-automatic-8x8", 128, 8, 256, 256, 3, 1, 0, 11)
    + _both("B128-automatic-4x4", 128, 4, 512, 512, 3, 1, 0, 11)
    + _both("B128-automatic-2x2", 128, 2, 512, 512, 3, 1, 0, 9)
    + _both("B128-automatic-stride2-3x3", 128, 32, 64, 128, 3, 2, 0, 12, lim_bwd=16)
    + _both("B128-automatic-stride2-1x1", 128, 16, 128, 256, 1, 2, 0, 12, lim=16)
)


def _feats(name, shape, tile, expect, fwd, bwd, lim=4, lim_bwd=None):
    n, hw, c, k, r, stride = shape
    out = [Case(name, n, hw, c, k, r, stride, 0, tile, expect, tuple(f.split("+")), lim) for f in fwd]
    return out + [Case(name, n, hw, c, k, r, stride, 1, tile, expect, tuple(f.split("+")), lim_bwd or lim) for f in bwd]


_FWD = ["post", "bias+pre", "act", "act+nodst"]
_BWD = ["mask", "mask+mul", "maskact+mul", "masknotab+pre+post"]

# ---- epilogue / prologue features, wide lattice, one representative shape per kernel family ------------------
FEATURE_CASES = (
    _feats("generic", (3, 10, 64, 64, 3, 2), 2, 2, _FWD + ["pro", "proimg+bias"], _BWD + ["maskimg"], lim_bwd=16)
    + _feats("halo", (5, 8, 64, 64, 3, 1), 8, 8, _FWD + ["pro", "proimg+post"], _BWD + ["maskimg"])
    + _feats("halo-2x2", (6, 2, 512, 512, 3, 1), 9, 9, ["post", "proimg"], ["maskimg+mul"])
    + _feats("dma", (5, 8, 128, 128, 3, 1), 10, 10, _FWD + ["prolds+prodst", "prolds+prodst+post", "prolds"], _BWD)
    + _feats("dma-32", (9, 4, 128, 64, 3, 1), 11, 11, ["bias+pre+post", "prolds+prodst"], ["mask+mul+post"])
    + _feats("dma-256", (7, 8, 64, 64, 3, 1), 14, 14, ["post", "act"], ["mask"])
    + _feats("dma-w64", (3, 16, 64, 64, 3, 1), 16, 16, ["post", "act"], ["maskact+mul"])
    + _feats("ws", (3, 32, 64, 64, 3, 1), 17, 17, _FWD, ["maskact+mul", "maskact+mul+pre+post"])
    + _feats("gather", (5, 6, 64, 64, 3, 2), 13, 13, _FWD, _BWD + ["maskimg", "src2", "src2+mask+mul"], lim_bwd=16)
    + _feats("gather-split-workspace", (16, 2, 512, 512, 3, 1), 0, 13, ["ws", "ws+post"], ["ws", "ws+mask"])
    + _feats("gather-split-workspace-stride2", (32, 8, 256, 512, 3, 2), 0, 13, ["ws+post"], [])
    + _feats("gather-src2-parity-classes", (4, 16, 128, 256, 3, 2), 0, 13, [], ["src2"])
    + _feats("B128-gather-src2-parity-classes", (128, 32, 64, 128, 3, 2), 0, 12, [], ["src2+mask+mul"], lim=16)
    + _feats("gather-src2-split-workspace", (3, 8, 256, 512, 3, 2), 0, 13, [], ["src2+ws", "src2+ws+mask"])
    + _feats("c8-stem", (3, 10, 3, 64, 3, 2), 15, 15, ["post", "bias+pre", "act"], [], lim=16)
    + _feats("c8-gradient", (2, 6, 64, 8, 3, 1), 15, 15, [], ["mask", "maskimg+mul", "masknotab+post"], lim=16)
    + _feats("k8", (5, 16, 64, 3, 3, 1), 0, 18, ["bias", "proimg+bias", "pro"], [])
)

# ---- statistics, narrow lattice -----------------------------------------------------------------------------
_S1 = ["stats1+post", "stats1+wg+post"]
_S2 = ["stats2+mask", "stats2+wg+mask+pre"]
STATS_CASES = (
    _feats("generic", (3, 10, 64, 64, 3, 2), 2, 2, ["stats1+post"], ["stats2+mask", "stats2+maskimg"], lim=1)
    + _feats("halo-per-image-rows", (3, 8, 128, 128, 3, 1), 7, 7, ["stats1"], ["stats2+maskimg"], lim=1)
    + _feats("halo-4x4", (9, 4, 128, 128, 3, 1), 9, 9, ["stats1+post"], ["stats2+maskimg"], lim=1)
    + _feats("dma", (5, 8, 128, 64, 3, 1), 10, 10, _S1, _S2, lim=1)
    + _feats("dma-32-4x4", (9, 4, 256, 256, 3, 1), 11, 11, _S1, _S2, lim=1)
    + _feats("dma-256", (7, 8, 128, 64, 3, 1), 14, 14, _S1, [], lim=1)
    + _feats("dma-w64", (3, 32, 64, 64, 3, 1), 16, 16, _S1, [], lim=1)
    + _feats("dma-lds-prologue", (5, 8, 128, 64, 3, 1), 10, 10, ["stats1+prolds+prodst", "stats1+wg+prolds+prodst+post"], [], lim=1)
    + _feats("ws", (3, 32, 64, 64, 3, 1), 17, 17, _S1, _S2, lim=1)
    + _feats("ws-2-tiles-per-workgroup-n40", (40, 32, 64, 64, 3, 1), 17, 17, ["stats1+wg+post"], ["stats2+wg+mask"], lim=1)
    + _feats("gather-raggedN", (3, 10, 64, 64, 3, 2), 13, 13, _S1, _S2, lim=1)
    + _feats("gather-split-workspace", (16, 2, 512, 512, 3, 1), 0, 13, ["stats1+ws+post"], [], lim=1)
    + _feats("c8-stem", (5, 32, 3, 64, 3, 1), 15, 15, _S1, [], lim=1)
    + _feats("c8-gradient-per-image", (2, 16, 64, 8, 3, 1), 15, 15, [], ["stats2+maskimg", "stats2+wg+maskimg"], lim=1)
)

ALL_CASES = PLAIN_CASES + FEATURE_CASES + STATS_CASES


def round_up(v, m):
    return (v + m - 1) // m * m


def nhwc_bf16(t):
    return t.permute(0, 2, 3, 1).contiguous().to(bf16)


def from_nhwc(t):
    return t.double().cpu().permute(0, 3, 1, 2).contiguous()


def pad_channels(t, to):
    if t.shape[1] == to:
        return t
    out = torch.zeros(t.shape[0], to, t.shape[2], t.shape[3], dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def packed(ops, w, stride, pad, c_pad, dup, device):
    wd = w.float().to(device).contiguous(memory_format=torch.channels_last)
    pc = ops.PackedConv(wd, stride, pad, c_pad, dup_hilo=dup)
    if device != "cpu":
        pc.pack()
    return pc


def build(case, ops, device):
    """Inputs, launch arguments and the exact expectation of `case`.  Returns a namespace with
       a         the ConvArgs (every guarded tensor kept alive by the namespace)
       picked    what combat_conv_pick_tile says for them
       outputs   {name: (Guarded, expected NCHW fp64)} for dst / act_dst / pro_act_dst
       guards    every destination Guarded (outputs, statistics, workspace)
       stats     None or (Guarded [rows][2][K], rows_per_image, expected [N][2][K])
       share     share of the real outputs that need rounding (wide lattices: asserted >= 2 %)"""
    from combat_amd._lib import lib
    f = set(case.feat)
    n, hw, c, k, r, stride, lim = case.n, case.hw, case.c, case.k, case.r, case.stride, case.lim
    pad = 1 if r == 3 else 0
    c_pad, k_pad = (8 if c == 3 else c), round_up(k, 8)
    p = (hw + 2 * pad - r) // stride + 1
    seed = iter(range(1000 + 97 * (sum(map(ord, case.id)) % 1000), 10 ** 9))
    big = 256 if lim >= 4 else 1
    G = lambda t: R.Guarded.source(t, device)
    D = lambda shape, dt=bf16, zero=False: R.Guarded(shape, dt, "dst", device, zero=zero)
    dev = lambda t: None if t is None else t.float().to(device)
    keep, guards, outputs = [], [], {}

    w = R.lattice((k, c, r, r), lim, next(seed))
    pc = packed(ops, w, stride, pad, c_pad, c == 3, device)
    pro = None
    quantum = 1.0
    if case.mode == 0:
        x = R.lattice((n, c_pad, hw, hw), lim, next(seed))
        x_eff = x[:, :3] + x[:, 3:6] if c == 3 else x
        if f & {"pro", "proimg", "prolds"}:
            shape = (n, c) if "proimg" in f else (c,)
            # (narrow lattice: integer scales and a plain ReLU keep the operand, hence the statistics, on the integers)
            psc, psh = R.pick(R.SCALES if lim > 1 else (-2.0, -1.0, 1.0, 2.0), shape, next(seed)), R.lattice(shape, 2, next(seed))
            slope = 0.0 if lim == 1 else 0.25
            x_eff = R.lattice_prologue(x, psc, psh, True, slope)
            pro = ops.Affine(dev(psc), dev(psh), c if "proimg" in f else 0, True, slope)
            quantum = 1.0 / 8 if lim > 1 else 1.0
        acc = pad_channels(R.conv_fwd(x_eff, w, stride, pad), k_pad)
        mag = pad_channels(R.conv_abs(x_eff, w, 0, hw, stride, pad), k_pad)
        src = G(nhwc_bf16(x))
        oshape, k_out, real = (n, k_pad, p, p), k_pad, k
        terms = r * r * c * (2 if c == 3 else 1)
    else:
        dy = R.lattice((n, k, p, p), lim, next(seed))
        acc = pad_channels(R.conv_dgrad(dy, w, hw, stride, pad), c_pad)
        mag = pad_channels(R.conv_abs(dy, w, 1, hw, stride, pad), c_pad)
        src = G(nhwc_bf16(pad_channels(dy, k_pad)))
        oshape, k_out, real = (n, c_pad, hw, hw), c_pad, c
        terms = r * r * k
    shortcut = None
    if "src2" in f:
        assert case.mode == 1 and r == 3 and stride == 2
        w1, dy1 = R.lattice((k, c, 1, 1), lim, next(seed)), R.lattice((n, k, p, p), lim, next(seed))
        pc1 = packed(ops, w1, 2, 0, c_pad, False, device)
        acc = acc + R.conv_dgrad(dy1, w1, hw, 2, 0)
        mag = mag + R.conv_abs(dy1, w1, 1, hw, 2, 0)
        src2 = G(nhwc_bf16(dy1))
        shortcut = (src2.t, pc1)
        keep.append(src2)
        terms += k

    def chan(shape_lim, per_image=False, values=None):
        shape = (n, k_out) if per_image else (k_out,)
        t = R.pick(values, shape, next(seed)) if values else R.lattice(shape, shape_lim, next(seed))
        return t

    kw, ep = {}, {}
    if "bias" in f:
        b = chan(8)
        b[real:] = 0
        ep["bias"], kw["bias"] = b, dev(b)
    for name, key in (("pre", "add_pre"), ("post", "add_post")):
        if name in f:
            t = R.lattice(oshape, big, next(seed))
            g = G(nhwc_bf16(t))
            ep[key], kw[key] = t, g.t
            keep.append(g)
    mask_x = None
    img = "maskimg" in f
    if f & {"mask", "maskimg", "maskact", "masknotab"}:
        mask_x = R.lattice(oshape, max(lim, 1) if lim < 16 else 4, next(seed))
        if "maskact" in f:
            mask_x = mask_x.clamp_min(0)
        g = G(nhwc_bf16(mask_x))
        keep.append(g)
        kw["mask_x"] = g.t
        slope = 0.0 if lim == 1 else 0.25
        ep.update(mask_x=mask_x, mask_slope=slope, mask_activated="maskact" in f, mask_mul_scale="mul" in f)
        if "masknotab" in f:
            kw["mask"] = ops.Affine(None, None, 0, True, slope)
        else:
            msc, msh = chan(0, img, R.SCALES), chan(2, img)
            ep.update(mask_scale=msc, mask_shift=msh)
            kw["mask"] = ops.Affine(dev(msc), dev(msh), k_out if img else 0, True, slope)
        kw["mask_activated"], kw["mask_mul_scale"] = "maskact" in f, "mul" in f
    v, emag, q = R.epilogue(acc, **ep)
    if mask_x is not None and "maskact" not in f:
        assert bool((q == 0).any()), "the mask argument must include exact zeros"
    R.range_check(mag + emag, quantum)
    y = R.rne_bf16(v)
    share = R.tie_share(v[:, :real])
    if lim >= 4:
        R.assert_not_vacuous(v[:, :real], case.id)

    dst = None
    if "nodst" not in f:
        dst = D((n, oshape[2], oshape[3], k_out))
        outputs["dst"] = (dst, y)
    act = None
    if "act" in f:
        asc, ash = chan(0, False, R.SCALES), chan(2)
        act = D((n, oshape[2], oshape[3], k_out))
        outputs["act_dst"] = (act, R.activated(y, asc, ash, 0.25))
        kw["act_dst"], kw["act"] = act.t, ops.Affine(dev(asc), dev(ash), 0, True, 0.25)
    if "prodst" in f:
        side = D((n, hw, hw, c_pad))
        outputs["pro_act_dst"] = (side, x_eff)
        kw["pro_act_dst"] = side.t
    kind = 1 if "stats1" in f else (2 if "stats2" in f else 0)
    totals = None
    if kind:
        if kind == 2:
            mean, rstd = chan(1, img), chan(0, img, (0.5, 1.0, 2.0))
            kw["xh_mean"], kw["xh_rstd"] = dev(mean), dev(rstd)
            totals = R.stats_totals(y, 2, mask_x, mean, rstd, 0.5)
        else:
            totals = R.stats_totals(y, 1)
        kw["stats_kind"] = kind | (4 if "wg" in f else 0)
    a = ops.conv_args(src.t, dst.t if dst is not None else None, pc, case.mode, pro=pro, tile=case.tile, shortcut=shortcut, **kw)
    if "ws" in f:
        need = int(lib.combat_conv_workspace_bytes(ctypes.byref(a)))
        assert need > 0, "no split reduction for this shape"
        ws = D((need,), torch.uint8)
        a.workspace, a.workspace_bytes = ws.t.data_ptr(), need
        guards.append(("workspace", ws))
    picked = lib.combat_conv_pick_tile(ctypes.byref(a))
    stats = None
    if kind:
        rows, rpi = ops.conv_stats_layout(a)
        sg = D((rows, 2, k_out), torch.float32, zero=True)
        a.stats = sg.t.data_ptr()
        guards.append(("stats", sg))
        stats = (sg, rpi, totals)
    guards += [(name, g) for name, (g, _) in outputs.items()]
    return SimpleNamespace(a=a, picked=picked, outputs=outputs, guards=guards, stats=stats, share=share, terms=terms,
                           keep=(keep, src, pc, kw, shortcut))


# ---- pairs for combat_conv_gemm_pair: a block's stride-2 3x3 convolution and its 1x1 shortcut, automatic tiles ----
PAIR_CASES = [
    (Case("pair-3x3", 6, 16, 128, 256, 3, 2, 0, 0, 13, ("act",)), Case("pair-1x1", 6, 16, 128, 256, 1, 2, 0, 0, 13, (), 16)),
    (Case("pair-3x3-odd10-raggedN", 3, 10, 64, 64, 3, 2, 0, 0, 13, ("post",)),
     Case("pair-1x1-odd10-raggedN", 3, 10, 64, 64, 1, 2, 0, 0, 13, ("bias", "post"), 16)),
]


# ---- weight gradients ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class WCase:
    kernel: str          # the kernel the arguments select (combat_conv_wgrad has no query for it: see `variants`)
    n: int
    hw: int
    c: int
    k: int
    r: int
    stride: int
    pro: str = ""        # "", "chan" (per-channel prologue) or "img" (per-image)
    variants: tuple = ((0, False),)      # (split, workspace) launches that must all give the same bits

    @property
    def id(self):
        return "%s-n%d-hw%d-c%d-k%d-r%d-s%d%s" % (self.kernel, self.n, self.hw, self.c, self.k, self.r, self.stride,
                                                ("-pro" + self.pro) if self.pro else "")


_ALL = ((0, False), (0, True), (3, False), (5, True), (7, False))     # automatic / explicit pixel ranges (5 and 7 do not
#                                                                       divide the pixel counts below), atomics / workspace
WGRAD_CASES = [
    # split < 0 forces the generic per-tap kernel: 64x64, 128x128, 16x64 (K = 3) and 64x16 (C = 8 with a prologue) tiles
    WCase("generic-per-tap", 4, 16, 64, 64, 3, 1, "", ((-1, False), (-1, True))),
    WCase("generic-per-tap-stride2-3x3-odd6", 3, 6, 128, 256, 3, 2, "", ((0, False), (3, False), (0, True))),
    WCase("generic-per-tap-stride2-1x1", 3, 12, 64, 128, 1, 2, "", ((0, False), (5, False))),
    WCase("generic-per-tap-K3-padded-to-8", 4, 16, 64, 3, 3, 1, "", ((-1, False), (7, False))),
    WCase("generic-per-tap-prologue-stride2", 4, 16, 64, 128, 3, 2, "img", ((0, False), (3, False))),
    # 3x3 / stride 1 with a prologue: the LDS-patch kernel, all nine taps per workgroup
    WCase("lds-patch-3x3", 3, 16, 128, 64, 3, 1, "img", ((0, False), (3, False), (7, False))),
    WCase("lds-patch-3x3-2-images-per-tile-raggedN", 5, 8, 64, 128, 3, 1, "chan", ((0, False), (5, False))),
    WCase("lds-patch-3x3-4x4-raggedN", 9, 4, 64, 64, 3, 1, "img", ((0, False), (7, False))),
    WCase("lds-patch-3x3-2x2-raggedN", 33, 2, 64, 64, 3, 1, "chan", ((0, False), (5, False))),
    # 3x3 / stride 1 without one: the DMA-staged kernel
    WCase("dma-3x3-16wide", 3, 16, 128, 64, 3, 1, "", _ALL),
    WCase("dma-3x3-32x32", 2, 32, 64, 64, 3, 1, "", _ALL),
    WCase("dma-3x3-2-images-per-tile-raggedN", 5, 8, 64, 128, 3, 1, "", _ALL),
    WCase("dma-3x3-4x4-raggedN", 9, 4, 64, 64, 3, 1, "", _ALL),
    WCase("dma-3x3-2x2-raggedN", 7, 2, 128, 64, 3, 1, "", _ALL),
    # C = 8 all-taps kernel (hi/lo stem: channels c and c + 3 fold onto dw channel c)
    WCase("c8-all-taps-hilo-stem", 2, 12, 3, 64, 3, 1, "", _ALL),
    WCase("c8-all-taps-hilo-stem-stride2-odd10", 3, 10, 3, 64, 3, 2, "", _ALL),
    WCase("c8-all-taps-hilo-stem-stride2-k128", 5, 16, 3, 128, 3, 2, "", ((0, False), (0, True), (7, True))),
    # the benchmarked batch: workgroup-count sizing of the pixel ranges, slab workspaces
    WCase("dma-3x3-B128", 128, 32, 64, 64, 3, 1, "", ((0, False), (0, True))),
    WCase("dma-3x3-B128-4x4", 128, 4, 512, 512, 3, 1, "", ((0, False), (0, True))),
    WCase("generic-per-tap-stride2-B128", 128, 32, 64, 128, 3, 2, "", ((0, False), (0, True))),
    WCase("c8-all-taps-hilo-stem-B128", 128, 32, 3, 64, 3, 1, "", ((0, False), (0, True))),
]

# a reduce_first chain: three DMA-staged launches that leave their slabs for the next one, one reduction at the end
CHAIN_SHAPES = [(3, 16, 128, 64), (5, 8, 64, 128), (2, 32, 64, 64)]


def wgrad_build(wc, lim, device, seed0=0):
    """Guarded src / dy (NaN bands), the prologue and the exact fp64 weight gradient [k][r*r][c] of a WCase."""
    from combat_amd import ops
    n, hw, c, k, r, stride = wc.n, wc.hw, wc.c, wc.k, wc.r, wc.stride
    pad = 1 if r == 3 else 0
    c_pad, k_pad = (8 if c == 3 else c), round_up(k, 8)
    p = (hw + 2 * pad - r) // stride + 1
    seed = iter(range(5000 + seed0 + 97 * (sum(map(ord, wc.id)) % 1000), 10 ** 9))
    x = R.lattice((n, c_pad, hw, hw), lim, next(seed))
    dy = R.lattice((n, k, p, p), lim, next(seed))
    x_eff = x[:, :3] + x[:, 3:6] if c == 3 else x
    pro, quantum = None, 1.0
    if wc.pro:
        shape = (n, c) if wc.pro == "img" else (c,)
        psc, psh = R.pick(R.SCALES, shape, next(seed)), R.lattice(shape, 2, next(seed))
        x_eff = R.lattice_prologue(x, psc, psh, True, 0.25)
        pro = ops.Affine(psc.float().to(device), psh.float().to(device), c if wc.pro == "img" else 0, True, 0.25)
        quantum = 1.0 / 8
    exp = R.conv_wgrad(x_eff, dy, k, r, stride, pad)
    R.range_check(R.wgrad_abs(x_eff, dy, k, r, stride, pad), quantum, "sum |x||dy|")
    assert R.is_f32(exp)
    return SimpleNamespace(src=R.Guarded.source(nhwc_bf16(x), device), dy=R.Guarded.source(nhwc_bf16(pad_channels(dy, k_pad)), device),
                           pro=pro, exp=exp, shape=(k, r * r, c), r=r, stride=stride, pad=pad, k=k, c=c)


def wgrad_args(b, dw, split=0, workspace=None, defer=0, first=None):
    """combat_wgrad_args for a built case; dw / workspace are Guarded destinations."""
    from combat_amd._lib import WgradArgs
    a = WgradArgs()
    a.N, a.H, a.W, a.C = b.src.t.shape
    _, a.P, a.Q, a.K = b.dy.t.shape
    a.R = a.S = b.r
    a.stride, a.pad = b.stride, b.pad
    a.src, a.dy, a.dw, a.k_real, a.c_real = b.src.t.data_ptr(), b.dy.t.data_ptr(), dw.t.data_ptr(), b.k, b.c
    if b.pro is not None:
        a.pro_scale, a.pro_shift = b.pro.scale.data_ptr(), b.pro.shift.data_ptr()
        a.pro_group_stride, a.pro_act, a.pro_slope = b.pro.group_stride, 1, b.pro.slope
    a.split = split
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.t.data_ptr(), workspace.numel
    a.defer_reduce = defer
    if first is not None:
        a.reduce_first = ctypes.addressof(first)
    return a
