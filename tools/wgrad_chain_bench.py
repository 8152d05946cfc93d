"""Weight-gradient slab reductions at B = 128, back to back: the kernel alone (slabs left behind), + its stand-alone
reduction launch (deterministic / round-3 atomics form: COMBAT_WGRAD_ATOMIC_REDUCE=1 in the environment), and the kernel
carrying the previous launch's reduction (combat_wgrad_args.reduce_first).  Last rows: the members of a stage as ONE
combat_conv_wgrad_group call against the same members as single launches back to back, in both modes of
combat_set_deterministic (the chip is empty apart from them, as at the end of a training backward).

    python tools/wgrad_chain_bench.py
"""
import ctypes
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from combat_amd import ops  # noqa: E402
from combat_amd._lib import WgradArgs, lib  # noqa: E402

bf16 = torch.bfloat16
g = lambda s: torch.Generator().manual_seed(s)
st = torch.cuda.current_stream().cuda_stream


def timed(fn, reps=40):
    for _ in range(4):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


N = 128
for (hw, c, k) in [(32, 64, 64), (16, 128, 128), (8, 256, 256), (4, 512, 512)]:
    x = torch.randn(N, hw, hw, c, generator=g(1)).to(bf16).cuda()
    dy = torch.randn(N, hw, hw, k, generator=g(2)).to(bf16).cuda()
    w = torch.randn(k, c, 3, 3, generator=g(3)) / math.sqrt(c * 9)
    pc = ops.PackedConv(w.cuda().contiguous(memory_format=torch.channels_last), 1, 1, c)
    dw = torch.zeros(k, 9, c, device="cuda")
    regions = [torch.empty(24 << 20, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def mk(region, defer, first=None):
        a = WgradArgs()
        a.N, a.H, a.W, a.C = x.shape
        _, a.P, a.Q, a.K = dy.shape
        a.R = a.S = 3
        a.stride, a.pad = 1, 1
        a.src, a.dy, a.dw, a.k_real, a.c_real = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), k, c
        a.workspace, a.workspace_bytes, a.defer_reduce = region.data_ptr(), region.numel(), defer
        if first is not None:
            a.reduce_first = ctypes.addressof(first)
        return a

    a_def = mk(regions[0], 1)
    a_own = mk(regions[0], 0)
    a_behind = mk(regions[1], 1, a_def)
    t_kernel = timed(lambda: lib.combat_conv_wgrad(ctypes.byref(a_def), st))
    t_own = timed(lambda: lib.combat_conv_wgrad(ctypes.byref(a_own), st))
    t_red = timed(lambda: lib.combat_conv_wgrad_reduce(ctypes.byref(a_def), st))
    t_behind = timed(lambda: lib.combat_conv_wgrad(ctypes.byref(a_behind), st))
    print("%2dx%-2d %3d->%-3d  kernel alone %.1f  kernel + reduction launch %.1f (reduction alone %.1f)  kernel carrying a reduction %.1f us" % (
        hw, hw, c, k, t_kernel, t_own, t_red, t_behind), flush=True)


# ---- a stage's same-geometry weight gradients: one group call against n single launches, both modes
PP = ctypes.POINTER(WgradArgs)
before = lib.combat_get_deterministic()
for (n, hw, c, k) in [(4, 32, 64, 64), (2, 32, 64, 64), (3, 16, 128, 128), (3, 8, 256, 256), (3, 4, 512, 512)]:
    xs = [torch.randn(N, hw, hw, c, generator=g(10 + i)).to(bf16).cuda() for i in range(n)]
    dys = [torch.randn(N, hw, hw, k, generator=g(20 + i)).to(bf16).cuda() for i in range(n)]
    dws = [torch.zeros(k, 9, c, device="cuda") for _ in range(n)]
    single_ws = torch.empty(48 << 20, dtype=torch.uint8, device="cuda")
    members = []
    for x, dy, dw in zip(xs, dys, dws):
        a = WgradArgs()
        a.N, a.H, a.W, a.C = x.shape
        _, a.P, a.Q, a.K = dy.shape
        a.R = a.S = 3
        a.stride, a.pad = 1, 1
        a.src, a.dy, a.dw, a.k_real, a.c_real = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), k, c
        a.workspace, a.workspace_bytes = single_ws.data_ptr(), single_ws.numel()
        members.append(a)
    arr = (PP * n)(*[ctypes.pointer(a) for a in members])
    need = int(lib.combat_conv_wgrad_group_workspace_bytes(arr, n))
    assert need >= 0
    gws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

    def singles():
        for a in members:
            assert lib.combat_conv_wgrad(ctypes.byref(a), st) == 0

    def group():
        assert lib.combat_conv_wgrad_group(arr, n, gws.data_ptr(), gws.numel(), st) == 0

    row = []
    for det in (0, 1):
        lib.combat_set_deterministic(det)
        row.append((timed(singles), timed(group)))
    lib.combat_set_deterministic(before)
    print("%d x %2dx%-2d %3d->%-3d  default: %d single launches %.1f, one group %.1f us   deterministic: single %.1f, group %.1f us  (%.1f MB of slabs)" % (
        n, hw, hw, c, k, n, row[0][0], row[0][1], row[1][0], row[1][1], need / 2 ** 20), flush=True)
