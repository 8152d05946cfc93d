"""The VGG13 victim's three entry points on the MI355X, compared for EQUALITY with tests/vgg13_ref.py's restatements:
inputs are bf16 values on small integer lattices, so every product and every fp32 sum is exact and no summation order or
rounding can hide a wrong index.  Only the cross-entropy terms (expf / logf) carry a tolerance: the existing head's."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgg13_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
GUARD = 64          # elements in front of and behind every output / input buffer
CANARY = -77.0


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def guarded(shape, dtype, fill=None):
    """(whole buffer, view of `shape` inside it) on the GPU with GUARD canary elements on both sides."""
    numel = 1
    for s in shape:
        numel *= s
    whole = torch.full((numel + 2 * GUARD,), CANARY, dtype=dtype, device="cuda")
    view = whole[GUARD:GUARD + numel].view(shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all())


# ---------------------------------------------------------------- combat_maxpool2_relu_bwd

POOL_SHAPES = [(n, h, w, c) for n in (1, 3) for (h, w) in ((2, 2), (4, 4), (6, 2), (32, 32)) for c in (8, 24, 64)]
# 5 x 128 x 128 x 512: 1 310 720 threads' worth of windows, more than the 4096 x 256 the launch's grid holds (the
# grid-stride loop wraps); 3 x 6 x 2 x 24 = 27 threads and 1 x 2 x 2 x 8 = 1 are no multiple of the workgroup size
POOL_SHAPES.append((5, 128, 128, 512))


@pytest.mark.parametrize("n,h,w,c", POOL_SHAPES)
def test_maxpool2_relu_bwd_lattice(ops, n, h, w, c):
    a = torch.randint(0, 4, (n, h, w, c), generator=g(n * 1000 + h * 10 + c)).float()       # post-ReLU: zeros and ties abound
    gr = torch.randint(-8, 9, (n, h // 2, w // 2, c), generator=g(n * 1000 + h * 10 + c + 1)).float()
    wa, da = guarded(a.shape, bf16, a)
    wg, dg = guarded(gr.shape, bf16, gr)
    wo, do = guarded(a.shape, bf16)
    ops.maxpool2_relu_bwd(da, dg, do)
    torch.cuda.synchronize()
    assert torch.equal(do.float().cpu(), R.pool_relu_bwd(a, gr))
    assert guards_intact(wa) and guards_intact(wg) and guards_intact(wo)
    assert torch.equal(da.float().cpu(), a) and torch.equal(dg.float().cpu(), gr)     # inputs untouched


def test_maxpool2_relu_bwd_hand_built_windows(ops):
    """One window per case along w, 8 channels each carrying the same case; [dy][dx] -> value, gradient 5."""
    cases = [
        ([[2, 2], [2, 2]], [[5, 0], [0, 0]]),       # four equal, positive: (0,0) only
        ([[1, 3], [3, 1]], [[0, 5], [0, 0]]),       # tie between (0,1) and (1,0): the earlier one
        ([[0, 0], [0, 0]], [[0, 0], [0, 0]]),       # all zero: nothing passes
        ([[-1, -2], [0, -3]], [[0, 0], [0, 0]]),    # maximum zero: nothing passes
        ([[-1, -2], [-4, -3]], [[0, 0], [0, 0]]),   # maximum negative
        ([[7, 1], [2, 3]], [[5, 0], [0, 0]]),       # maximum in each of the four positions
        ([[1, 7], [2, 3]], [[0, 5], [0, 0]]),
        ([[1, 2], [7, 3]], [[0, 0], [5, 0]]),
        ([[1, 2], [3, 7]], [[0, 0], [0, 5]]),
        ([[1, 2], [3, 3]], [[0, 0], [5, 0]]),       # tie between (1,0) and (1,1)
    ]
    k = len(cases)
    a, want = torch.zeros(1, 2, 2 * k, 8), torch.zeros(1, 2, 2 * k, 8)
    for i, (vals, exp) in enumerate(cases):
        a[0, :, 2 * i:2 * i + 2, :] = torch.tensor(vals, dtype=torch.float32).unsqueeze(-1)
        want[0, :, 2 * i:2 * i + 2, :] = torch.tensor(exp, dtype=torch.float32).unsqueeze(-1)
    gr = torch.full((1, 1, k, 8), 5.0)
    out = torch.empty(a.shape, dtype=bf16, device="cuda")
    ops.maxpool2_relu_bwd(a.to(bf16).cuda(), gr.to(bf16).cuda(), out)
    assert torch.equal(out.float().cpu(), want)
    assert torch.equal(R.pool_relu_bwd(a, gr), want)          # (the restatement agrees with the hand-built answer)


# ---------------------------------------------------------------- flat head

HEAD_SHAPES = [(1, 1, 8, 2), (3, 2, 8, 8), (16, 1, 512, 10), (16, 2, 512, 8), (3, 2, 512, 10), (1, 2, 8, 10), (16, 1, 8, 2)]


def head_inputs(n, hw, c, classes, seed):
    """Lattice operands: features in {-2..2}, weights in {-4..4} / 8, bias in {-8..8} / 8, the logits' gradient in
    {-4..4} / 16: every product is a multiple of 2^-7 below 2^3 and every sum of <= 2048 of them stays below 2^14, exact
    in fp32 (24 bits); d_feat <= 16 * 4 * 4 / 128 = 2 in multiples of 2^-7: <= 8 significant bits, exact in bf16."""
    feat = torch.randint(-2, 3, (n, hw, hw, c), generator=g(seed)).float()
    w = torch.randint(-4, 5, (classes, c * hw * hw), generator=g(seed + 1)).float() / 8
    b = torch.randint(-8, 9, (classes,), generator=g(seed + 2)).float() / 8
    t = torch.randint(0, classes, (n,), generator=g(seed + 3))
    dl = torch.randint(-4, 5, (n, classes), generator=g(seed + 4)).float() / 16
    return feat, w, b, t, dl


@pytest.mark.parametrize("n,hw,c,classes", HEAD_SHAPES)
def test_flat_head_lattice(ops, n, hw, c, classes):
    feat, w, b, t, dl = head_inputs(n, hw, c, classes, 7000 + n * 100 + hw * 10 + classes)
    # small logits for the softmax part: scale the weights down by an exact power of two (still a lattice)
    w = w / 64 if c == 512 else w
    fd, wd, bd, td = feat.to(bf16).cuda(), w.cuda(), b.cuda(), t.cuda()
    wl, logits = guarded((n, classes), torch.float32)
    wdl, dlog = guarded((n, classes), torch.float32)
    loss, correct = torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.flat_head_fwd(fd, wd, bd, logits, targets=td, loss_weight=0.8, dlogits=dlog, loss=loss, correct=correct)
    torch.cuda.synchronize()
    ref = R.flat_head(feat, w, b)
    assert torch.equal(logits.cpu(), ref)                      # exact: pins the NCHW column order at hw = 2
    assert guards_intact(wl) and guards_intact(wdl)
    # loss / dlogits against fp64 softmax: the existing head test's bounds (tests/test_kernels_gpu.py::test_head_forward_backward)
    r64 = ref.double().requires_grad_(True)
    ls = 0.8 * F.cross_entropy(r64, t)
    ls.backward()
    assert abs(float(loss) - float(ls.detach())) < 1e-5
    assert int(correct) == int((ref.argmax(1) == t).sum())
    assert float((dlog.cpu().double() - r64.grad).norm()) <= 1e-5 * max(float(r64.grad.norm()), 1e-30)
    # second call: same bits (the accumulators add the same amounts again)
    logits2, dlog2 = torch.empty_like(logits), torch.empty_like(dlog)
    ops.flat_head_fwd(fd, wd, bd, logits2, targets=td, loss_weight=0.8, dlogits=dlog2, loss=loss, correct=correct)
    assert torch.equal(logits2, logits) and torch.equal(dlog2, dlog) and int(correct) == 2 * int((ref.argmax(1) == t).sum())
    # logits only
    logits3 = torch.empty_like(logits)
    ops.flat_head_fwd(fd, wd, bd, logits3)
    assert torch.equal(logits3, logits)
    # backward from a lattice gradient of the logits
    wf, d_feat = guarded(feat.shape, bf16)
    ww, dw = guarded(w.shape, torch.float32)
    wb, db = guarded((classes,), torch.float32)
    dld = dl.cuda()
    ops.flat_head_bwd(fd, wd, dld, d_feat, dw, db)
    torch.cuda.synchronize()
    e_feat, e_w, e_b = R.flat_head_bwd(feat, w, dl)
    assert torch.equal(d_feat.float().cpu(), e_feat)
    assert torch.equal(dw.cpu(), e_w) and torch.equal(db.cpu(), e_b)
    assert guards_intact(wf) and guards_intact(ww) and guards_intact(wb)
    d_feat2, dw2, db2 = torch.empty_like(d_feat), torch.empty_like(dw), torch.empty_like(db)
    ops.flat_head_bwd(fd, wd, dld, d_feat2, dw2, db2)
    assert torch.equal(d_feat2, d_feat) and torch.equal(dw2, dw) and torch.equal(db2, db)
    # each half alone
    d_feat3, dw3, db3 = torch.empty_like(d_feat), torch.empty_like(dw), torch.empty_like(db)
    ops.flat_head_bwd(fd, wd, dld, d_feat3)
    ops.flat_head_bwd(fd, wd, dld, None, dw3, db3)
    assert torch.equal(d_feat3, d_feat) and torch.equal(dw3, dw) and torch.equal(db3, db)
