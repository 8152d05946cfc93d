"""combat_conv_wgrad_group on the MI355X: up to four same-geometry 3x3 weight gradients in ONE kernel launch and ONE
reduction launch (csrc/conv_wgrad3x3_dma.hip).

Every member keeps the pixel ranges, slab layout and per-element summation order it has alone, so the criterion in
deterministic mode is equality of bits with combat_conv_wgrad(member).  Shapes: the geometries of
test_kernels_gpu.py::test_wgrad3x3_dma_kernel (16-, 8-, 4- and 2-pixel-wide patches, several images per patch, ragged
N), one and four tiles, i.e. both reduction forms.  Members have different inputs: a workgroup that read another
member's operands or slabs cannot pass.
"""
import ctypes

import pytest
import torch

import conv_exact_cases as CC
import conv_exact_ref as R

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
DEV = "cuda"
EINVAL = -1
# (members; N, HW, C, K)
SHAPES = [(4, 4, 32, 64, 64),       # one tile: reduce_slabs in deterministic mode
          (3, 3, 16, 128, 128),     # four tiles: the single-group range reduction, two halo pieces per wave
          (2, 5, 8, 64, 128),       # three halo pieces per wave
          (3, 6, 4, 128, 128),      # several images per patch
          (2, 9, 4, 64, 64),        # ragged N
          (2, 33, 2, 64, 64)]       # 2-pixel-wide patches, ragged
IDS = ["%dx-n%d-hw%d-c%d-k%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def lib():
    from combat_amd._lib import lib as l
    return l


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


@pytest.fixture
def det(lib):
    """Deterministic mode for the test, the process's setting restored behind it."""
    before = lib.combat_get_deterministic()
    lib.combat_set_deterministic(1)
    yield
    lib.combat_set_deterministic(before)


def stream():
    return torch.cuda.current_stream().cuda_stream


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def wargs(x, dy, dw, ws=None, stride=1, pro=None):
    from combat_amd._lib import WgradArgs
    a = WgradArgs()
    a.N, a.H, a.W, a.C = x.shape
    _, a.P, a.Q, a.K = dy.shape
    a.R = a.S = 3
    a.stride, a.pad = stride, 1
    a.src, a.dy, a.dw, a.k_real, a.c_real = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dy.shape[-1], x.shape[-1]
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if pro is not None:
        a.pro_scale, a.pro_shift, a.pro_act, a.pro_slope = pro[0].data_ptr(), pro[1].data_ptr(), 1, 0.2
    return a


def member_array(members):
    from combat_amd._lib import WgradArgs
    return (ctypes.POINTER(WgradArgs) * len(members))(*[ctypes.pointer(a) for a in members])


def group_need(lib, members):
    return int(lib.combat_conv_wgrad_group_workspace_bytes(member_array(members), len(members)))


def run_group(lib, members, ws):
    return lib.combat_conv_wgrad_group(member_array(members), len(members), ws.data_ptr() if ws is not None else None,
                                       ws.numel() if ws is not None else 0, stream())


_CACHE = {}


def operands(shape):
    """Per member: bf16 NHWC x and dy on the GPU, the non-zero start value of an accumulating run, and the fp32
    reference of torch.nn.grad.conv2d_weight on the rounded inputs.  Built once per shape."""
    if ("op", shape) not in _CACHE:
        nm, n, hw, c, k = shape
        out = []
        for m in range(nm):
            gen = torch.Generator().manual_seed(7000 + 31 * m + 1000 * SHAPES.index(shape))
            x = torch.randn(n, c, hw, hw, generator=gen).to(bf16)
            dy = torch.randn(n, k, hw, hw, generator=gen).to(bf16)
            start = torch.randn(k, 9, c, generator=gen)
            ref = torch.nn.grad.conv2d_weight(x.float(), (k, c, 3, 3), dy.float(), padding=1).permute(0, 2, 3, 1).reshape(k, 9, c)
            out.append((x.permute(0, 2, 3, 1).contiguous().to(DEV), dy.permute(0, 2, 3, 1).contiguous().to(DEV), start.to(DEV), ref))
        _CACHE[("op", shape)] = out
    return _CACHE[("op", shape)]


def alone(lib, ops, shape, accumulate):
    """Every member through combat_conv_wgrad by itself, in deterministic mode (the caller sets it): the bits the group
    must reproduce.  Computed once per (shape, accumulate) and never modified."""
    key = ("alone", shape, accumulate)
    if key not in _CACHE:
        assert lib.combat_get_deterministic() == 1
        res = []
        for x, dy, start, _ in operands(shape):
            dw = start.clone() if accumulate else torch.zeros_like(start)
            need = int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(wargs(x, dy, dw))))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
            ops.check(lib.combat_conv_wgrad(ctypes.byref(wargs(x, dy, dw, ws)), stream()), "combat_conv_wgrad", str(shape))
            res.append(dw)
        torch.cuda.synchronize()
        _CACHE[key] = res
    return _CACHE[key]


def grouped(lib, ops, shape, accumulate, between=None):
    ops_ = operands(shape)
    dws = [(start.clone() if accumulate else torch.zeros_like(start)) for _, _, start, _ in ops_]
    members = [wargs(x, dy, dw) for (x, dy, _, _), dw in zip(ops_, dws)]
    need = group_need(lib, members)
    assert need >= 0, shape
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    if between is not None:
        between()
    ops.check(run_group(lib, members, ws), "combat_conv_wgrad_group", str(shape))
    torch.cuda.synchronize()
    return dws


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_group_members_equal_single_launches_bitwise(lib, ops, det, shape):
    """Deterministic mode: every member's dw from the group call is bit-identical to the member launched alone -- into
    zeroed buffers and accumulating into non-zero ones -- and a second group call gives the same bits."""
    for accumulate in (False, True):
        want = alone(lib, ops, shape, accumulate)
        first = grouped(lib, ops, shape, accumulate)
        second = grouped(lib, ops, shape, accumulate)
        for m, (w, a, b) in enumerate(zip(want, first, second)):
            assert torch.equal(a, w), ("member %d differs from its single launch" % m, shape, accumulate, rel_l2(a, w))
            assert torch.equal(a, b), ("two group calls differ in member %d" % m, shape, accumulate)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_group_default_mode_against_deterministic_and_fp32(lib, ops, shape):
    """Default mode (ranges may meet through a few fp32 atomics): rel-L2 < 2e-6 against the deterministic result (the
    bound of test_deterministic_gpu.py) and < 2e-3 against conv2d_weight in fp32 (the bound of test_kernels_gpu.py)."""
    before = lib.combat_get_deterministic()
    try:
        lib.combat_set_deterministic(1)
        want = alone(lib, ops, shape, False)
        lib.combat_set_deterministic(0)
        got = grouped(lib, ops, shape, False)
    finally:
        lib.combat_set_deterministic(before)
    for m, (g, w, (_, _, _, ref)) in enumerate(zip(got, want, operands(shape))):
        e_det, e_ref = rel_l2(g, w), rel_l2(g, ref)
        print("member %d of %s: rel_l2 vs deterministic %.3g, vs fp32 conv2d_weight %.3g" % (m, shape, e_det, e_ref))
        assert e_det < 2e-6, (m, shape, e_det)
        assert e_ref < 2e-3, (m, shape, e_ref)


@pytest.mark.parametrize("mode", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("nm,n,hw,c,k", [(3, 2, 32, 64, 64), (2, 3, 16, 128, 128)], ids=["one-tile", "four-tiles"])
def test_group_exact_on_lattice_inputs(lib, ops, mode, nm, n, hw, c, k):
    """Lattice inputs (conv_exact_cases.wgrad_build): every summation order gives the same integers, so each member's
    dw EQUALS the integer reference in both modes; guard bands around every dw and the workspace stay untouched."""
    built = [CC.wgrad_build(CC.WCase("group%d" % m, n, hw, c, k, 3, 1), 4, DEV, seed0=11 * m) for m in range(nm)]
    dws = [R.Guarded(b.shape, torch.float32, "dst", DEV, zero=True) for b in built]
    members = [CC.wgrad_args(b, dw) for b, dw in zip(built, dws)]
    need = group_need(lib, members)
    assert need > 0
    ws = R.Guarded((need,), torch.uint8, "dst", DEV)
    before = lib.combat_get_deterministic()
    lib.combat_set_deterministic(mode)
    try:
        ops.check(lib.combat_conv_wgrad_group(member_array(members), nm, ws.t.data_ptr(), need, stream()), "combat_conv_wgrad_group")
        torch.cuda.synchronize()
    finally:
        lib.combat_set_deterministic(before)
    ws.check("group workspace")
    for m, (b, dw) in enumerate(zip(built, dws)):
        dw.check("dw of member %d" % m)
        R.report_mismatch(dw.t.double().cpu(), b.exp, "dw [k][tap][c] of group member %d" % m)


def test_group_of_one_equals_plain_call(lib, ops, det):
    shape = SHAPES[0]
    x, dy, start, _ = operands(shape)[0]
    want = alone(lib, ops, shape, True)[0]
    dw = start.clone()
    members = [wargs(x, dy, dw)]
    need = group_need(lib, members)
    assert need == int(lib.combat_conv_wgrad_workspace_bytes(ctypes.byref(members[0]))) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    ops.check(run_group(lib, members, ws), "combat_conv_wgrad_group", "one member")
    torch.cuda.synchronize()
    assert torch.equal(dw, want)


def test_group_refuses_what_does_not_fit_and_launches_nothing(lib, det):
    """Mixed geometry, a stride-2 member, a member with a prologue and a short workspace: COMBAT_EINVAL, every dw as it
    was.  (Also reduce_first / defer_reduce on a member, more than four members.)"""
    n, hw, c, k = 4, 16, 64, 64
    gen = torch.Generator().manual_seed(99)
    mk = lambda *s: torch.randn(*s, generator=gen).to(bf16).to(DEV)
    x0, x1, dy0, dy1 = mk(n, hw, hw, c), mk(n, hw, hw, c), mk(n, hw, hw, k), mk(n, hw, hw, k)
    sentinel = torch.randn(k, 9, c, generator=gen).to(DEV)
    dw0, dw1 = sentinel.clone(), sentinel.clone()
    good = [wargs(x0, dy0, dw0), wargs(x1, dy1, dw1)]
    need = group_need(lib, good)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    other = wargs(mk(n, hw, hw, 2 * c), dy1, torch.zeros(k, 9, 2 * c, device=DEV))            # C differs
    strided = wargs(x1, mk(n, hw // 2, hw // 2, k), dw1, stride=2)
    strided0 = wargs(x0, mk(n, hw // 2, hw // 2, k), dw0, stride=2)
    pro = (torch.ones(c, device=DEV), torch.zeros(c, device=DEV))
    with_pro = [wargs(x0, dy0, dw0, pro=pro), wargs(x1, dy1, dw1, pro=pro)]
    deferred = wargs(x1, dy1, dw1)
    deferred.defer_reduce = 1
    carried = wargs(x1, dy1, dw1)
    carried.reduce_first = ctypes.addressof(good[0])
    bad = {"mixed geometry": [good[0], other], "stride-2 member": [good[0], strided], "stride-2 group": [strided0, strided],
           "prologue": with_pro, "defer_reduce": [good[0], deferred], "reduce_first": [good[0], carried],
           "same dw twice": [good[0], wargs(x1, dy1, dw0)]}
    for name, members in bad.items():
        assert group_need(lib, members) == EINVAL, name
        assert run_group(lib, members, ws) == EINVAL, name
    short = torch.empty(need - 1, dtype=torch.uint8, device=DEV)
    assert run_group(lib, good, short) == EINVAL, "short workspace"
    assert run_group(lib, good, None) == EINVAL, "no workspace"
    five = [wargs(x0, dy0, sentinel.clone()) for _ in range(5)]
    assert group_need(lib, five) == EINVAL and run_group(lib, five, ws) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(dw0, sentinel) and torch.equal(dw1, sentinel)
    assert run_group(lib, good, ws) == 0        # (and the same members with enough workspace are a group)
    torch.cuda.synchronize()
    assert not torch.equal(dw0, sentinel) and not torch.equal(dw1, sentinel)


def test_group_cold_cache(lib, ops, det):
    """Operands and slabs out of the caches: 512 MB are written between operand set-up and the group launch (the
    Infinity Cache holds 256 MB); same equality as above."""
    shape = SHAPES[0]
    want = alone(lib, ops, shape, False)
    scratch = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    got = grouped(lib, ops, shape, False, between=lambda: scratch.fill_(1))
    for m, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), ("member %d" % m, rel_l2(g, w))
