"""The input-aware and multi-label attacks at ImageNet-10's 224 x 224 on the MI355X: the paired and the grouped trigger
on the strip route (64 < hw <= 256, hw % 16 == 0), InputAwareStep / MultiLabelStep at hw = 224 and the four scripts
with --dataset imagenet10.

Shapes of the kernel tests: hw = 80 is the smallest size on the strip route (five strips, an odd count), 224 the real
size, 256 the size at which every thread of a workgroup owns a column -- and the only one at which the clamp mask of
a modest batch does not fit the stream's 2 MB scratch (85 mask rows of 24 KB per run).  Bounds against the oracle
are those of tests/test_trigger_big_gpu.py (out 2e-5, mse rel-L2 1e-4, d_noise rel-L2 4e-3); everything else is
torch.equal against the plain combat_trigger_fwd / _bwd calls the paired / grouped launch stands for.

DESIGN.md section 14 records what these tests measured on the MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402
import inputaware_ref as IR  # noqa: E402
import multilabel_ref as MR  # noqa: E402
from test_engine_gpu import _oracle_state, flat_grads, rel_l2, seeded, stored  # noqa: E402
from test_imagenet10_unet_gpu import _nets224, _opt224  # noqa: E402
from test_oracle_golden import synth_images  # noqa: E402

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, RATIO = 0.08, 0.65
EINVAL, OK = -1, 0


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return t.to("cuda")


def c8(noise):
    """NCHW noise -> the generator's c8 output layout on the device (channels 3..7 zero)."""
    n, _, hw, _ = noise.shape
    out = torch.zeros(n, hw, hw, 8, dtype=bf16, device="cuda")
    out[..., :3] = dev(noise.to(bf16)).permute(0, 2, 3, 1)
    return out


def bits(t):
    return t.view(torch.int16) if t.dtype == bf16 else t


def k1_of(sigmas):
    from combat_amd import trigger
    return torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(s, 3)) for s in sigmas]).cuda()


# ------------------------------------------------------------------ 1, 2: the bits of the plain calls
@functools.lru_cache(maxsize=None)
def clamp_case(hw, rows_x, rows_noise):
    """Images whose half-planes sit at +-0.999 (both clamp branches are taken), noise rows and three gradients; shared
    by the tests of one shape, never modified."""
    from combat_amd import trigger
    gen = g(hw + rows_x)
    x = torch.rand(rows_x, 3, hw, hw, generator=gen) * 2 - 1
    x[0, :, : hw // 2] = 0.999                  # saturates the clamp where the noise is positive
    x[1, :, :, : hw // 2] = -0.999
    noise = torch.tanh(torch.randn(rows_noise, 3, hw, hw, generator=gen)).to(bf16).float()
    grads = tuple(dev(torch.randn(rows_x, 3, hw, hw, generator=gen)) for _ in range(3))
    return x, noise, c8(noise), trigger.lowpass_matrix(hw, RATIO).cuda(), grads


@pytest.mark.parametrize("hw,n", [(80, 3), (224, 2)])
def test_pair_equals_two_plain_calls(ops, hw, n):
    from oracle import combat_oracle as O
    x, noise, n8, pm, (d_bd, d_bd2, d_cross) = clamp_case(hw, n, 2 * n)
    pre = x.double().repeat(2, 1, 1, 1) + RATE * O.low_freq(noise.double(), RATIO)
    frac = float((pre.abs() > 1).double().mean())
    print("pre-clamp values outside [-1, 1]: %.3f" % frac)
    assert frac > 0.02                                            # both clamp branches are taken
    k1, xc = k1_of((0.4, 0.8)), dev(x)
    bd, bd2 = torch.full((n, 3, hw, hw), 7.0, device="cuda"), torch.full((n, 3, hw, hw), 7.0, device="cuda")
    mse = torch.full((3 * n,), 7.0, device="cuda")
    ops.trigger_pair_fwd(xc, n8, pm, k1, RATE, bd, bd2, mse)
    r_bd, r_bd2, r_mse = torch.empty_like(bd), torch.empty_like(bd), torch.empty_like(mse)
    ops.trigger_fwd(xc, n8[:n], pm, k1[0], RATE, r_bd, mse_partial=r_mse)
    ops.trigger_fwd(xc, n8[n:], pm, k1[1], RATE, r_bd2)
    torch.cuda.synchronize()
    assert torch.equal(bd, r_bd) and torch.equal(bd2, r_bd2) and torch.equal(mse, r_mse)
    assert not torch.equal(bd, bd2)
    nomse = torch.empty_like(bd), torch.empty_like(bd)
    ops.trigger_pair_fwd(xc, n8, pm, k1, RATE, *nomse)          # without the partials: one launch, the same images
    assert torch.equal(nomse[0], bd) and torch.equal(nomse[1], bd2)
    l2 = 0.3
    for with2 in (False, True):
        dn = torch.full((2 * n, hw, hw, 8), 7.0, dtype=bf16, device="cuda")
        ops.trigger_pair_bwd(xc, n8, pm, k1, RATE, d_bd, bd, l2, d_cross, dn, pre_tanh=True, d_bd2=d_bd2 if with2 else None)
        ref = torch.full_like(dn, 7.0)
        ops.trigger_bwd(xc, n8[:n], pm, k1[0], RATE, d_bd, bd, l2, ref[:n], pre_tanh=True, d_out2=d_bd2 if with2 else None)
        ops.trigger_bwd(xc, n8[n:], pm, k1[1], RATE, d_cross, None, 0.0, ref[n:], pre_tanh=True)
        torch.cuda.synchronize()
        assert torch.equal(bits(dn), bits(ref)), with2
        assert bool(torch.isfinite(dn.float()).all()) and float(dn[..., 3:].float().abs().max()) == 0.0


@pytest.mark.parametrize("n,ps,hw", [(5, 2, 80), (3, 3, 80), (4, 1, 224)])
def test_groups_equal_per_chunk_plain_calls(ops, n, ps, hw):
    from oracle import combat_oracle as O
    x, noise, n8, pm, (d1, d2, _) = clamp_case(hw, n, n)
    pre = x.double() + RATE * O.low_freq(noise.double(), RATIO)
    assert float((pre.abs() > 1).double().mean()) > 0.02
    groups = (n + ps - 1) // ps
    k1 = k1_of([0.15 + 0.8 * i / max(groups - 1, 1) for i in range(groups)])
    xc, l2 = dev(x), 0.3
    chunks = [(ci, ci * ps, min(ci * ps + ps, n)) for ci in range(groups)]
    bd, mse = torch.full((n, 3, hw, hw), 7.0, device="cuda"), torch.full((3 * n,), 7.0, device="cuda")
    ops.trigger_groups_fwd(xc, n8, pm, k1, ps, RATE, bd, mse)
    r_bd, r_mse = torch.empty_like(bd), torch.empty_like(mse)
    for ci, si, ei in chunks:
        ops.trigger_fwd(xc[si:ei], n8[si:ei], pm, k1[ci], RATE, r_bd[si:ei], mse_partial=r_mse[3 * si:3 * ei])
    torch.cuda.synchronize()
    assert torch.equal(bd, r_bd) and torch.equal(mse, r_mse)
    if groups > 1:       # the groups differ: image 0 under the last group's kernel is another image
        other = torch.empty(1, 3, hw, hw, device="cuda")
        ops.trigger_fwd(xc[:1], n8[:1], pm, k1[-1], RATE, other)
        assert not torch.equal(other, bd[:1])
    for with2 in (False, True):
        dn = torch.full((n, hw, hw, 8), 7.0, dtype=bf16, device="cuda")
        ops.trigger_groups_bwd(xc, n8, pm, k1, ps, RATE, d1, bd, l2, dn, pre_tanh=True, d_out2=d2 if with2 else None)
        ref = torch.full_like(dn, 7.0)
        for ci, si, ei in chunks:
            ops.trigger_bwd(xc[si:ei], n8[si:ei], pm, k1[ci], RATE, d1[si:ei], bd[si:ei], l2, ref[si:ei], pre_tanh=True,
                            d_out2=d2[si:ei] if with2 else None)
        torch.cuda.synchronize()
        assert torch.equal(bits(dn), bits(ref)), with2


# ------------------------------------------------------------------ 3: against the oracle
@functools.lru_cache(maxsize=None)
def oracle_case():
    """The operands of tests/test_trigger_big_gpu.py::case at (80, 3) -- the same draws for the images, six noise rows
    from its noise seed -- and the nearest pre-clamp value to +-1 of the pair's six rows and of the groups' three.
    Checked on the CPU: per noise row 1.8e-5, 1.9e-5, 5.7e-6 (that file's figure), 7.5e-5, 1.5e-5, 2.8e-5."""
    from oracle import combat_oracle as O
    hw, n = 80, 3
    x = ((torch.randint(0, 256, (n, 3, hw, hw), generator=g(190)).float() / 255) - 0.5) / 0.5
    noise = torch.tanh(torch.randn(2 * n, 3, hw, hw, generator=g(191)) * 3).to(bf16).float()
    pre = x.double().repeat(2, 1, 1, 1) + O.low_freq(noise.double(), RATIO) * RATE
    margin = torch.minimum((pre - 1).abs(), (pre + 1).abs()).flatten(1).min(1).values
    d = [torch.randn(n, 3, hw, hw, generator=g(192 + i)) for i in range(3)]
    return x, noise, c8(noise), dev(O.lowpass_matrix(hw, RATIO)), d, margin


def test_pair_against_the_oracle(ops):
    from oracle import combat_oracle as O
    hw, n, sg, sx = 80, 3, 0.35, 0.9
    x, noise, n8, pm, (d_bd, d_bd2, d_cross), margin = oracle_case()
    print("nearest pre-clamp value to +-1: %.3g" % float(margin.min()))
    assert float(margin.min()) > 1e-6
    leaf = noise.clone().requires_grad_(True)
    o1, o2 = O.trigger_mix(x, leaf[:n], RATE, RATIO, sg), O.trigger_mix(x, leaf[n:], RATE, RATIO, sx)
    l2s = 0.02 / o1.numel()
    (gr,) = torch.autograd.grad((o1 * (d_bd + d_bd2)).sum() + l2s * ((o1 - x) ** 2).sum() + (o2 * d_cross).sum(), leaf)
    k1 = dev(torch.stack([O.gaussian_kernel1d(sg), O.gaussian_kernel1d(sx)]))
    xc = dev(x)
    bd, bd2, mse = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(3 * n, device="cuda")
    ops.trigger_pair_fwd(xc, n8, pm, k1, RATE, bd, bd2, mse)
    e1, e2 = float((bd.cpu() - o1.detach()).abs().max()), float((bd2.cpu() - o2.detach()).abs().max())
    e_mse = rel_l2(mse.view(n, 3), ((o1.detach() - x) ** 2).sum((2, 3)))
    dn = torch.full((2 * n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ops.trigger_pair_bwd(xc, n8, pm, k1, RATE, dev(d_bd), bd, l2s, dev(d_cross), dn, d_bd2=dev(d_bd2))
    e_dn = rel_l2(dn[..., :3].float().permute(0, 3, 1, 2), gr)
    e_halves = [rel_l2(dn[a:b, ..., :3].float().permute(0, 3, 1, 2), gr[a:b]) for a, b in ((0, n), (n, 2 * n))]
    print("pair vs oracle: out %.3g / %.3g, mse %.3g, d_noise %.3g (halves %.3g, %.3g)" % (e1, e2, e_mse, e_dn, *e_halves))
    assert e1 < 2e-5 and e2 < 2e-5
    assert e_mse < 1e-4
    assert e_dn < 4e-3 and max(e_halves) < 4e-3
    assert float(dn[..., 3:].float().abs().max()) == 0.0


def test_groups_against_the_oracle(ops):
    from oracle import combat_oracle as O
    hw, n, ps, sig = 80, 3, 2, (0.35, 0.9)
    x, noise, n8, pm, (d1, d2, _), margin = oracle_case()
    assert float(margin[:n].min()) > 1e-6
    chunks = [(0, 0, 2), (1, 2, 3)]
    leaf = noise[:n].clone().requires_grad_(True)
    ref = torch.cat([O.trigger_mix(x[si:ei], leaf[si:ei], RATE, RATIO, sig[ci]) for ci, si, ei in chunks])
    l2s = 0.02 / ref.numel()
    (gr,) = torch.autograd.grad((ref * (d1 + d2)).sum() + l2s * ((ref - x) ** 2).sum(), leaf)
    k1 = dev(torch.stack([O.gaussian_kernel1d(s) for s in sig]))
    xc = dev(x)
    out, mse = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(3 * n, device="cuda")
    ops.trigger_groups_fwd(xc, n8[:n], pm, k1, ps, RATE, out, mse)
    e_out = float((out.cpu() - ref.detach()).abs().max())
    e_mse = rel_l2(mse.view(n, 3), ((ref.detach() - x) ** 2).sum((2, 3)))
    dn = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ops.trigger_groups_bwd(xc, n8[:n], pm, k1, ps, RATE, dev(d1), out, l2s, dn, d_out2=dev(d2))
    e_dn = rel_l2(dn[..., :3].float().permute(0, 3, 1, 2), gr)
    print("groups vs oracle: out %.3g, mse %.3g, d_noise %.3g" % (e_out, e_mse, e_dn))
    assert e_out < 2e-5
    assert e_mse < 1e-4
    assert e_dn < 4e-3
    assert float(dn[..., 3:].float().abs().max()) == 0.0


# ------------------------------------------------------------------ 4: batches whose clamp mask does not fit one run
@functools.lru_cache(maxsize=None)
def runs_case():
    """hw = 256: 86 images, 100 noise rows and two gradients of 86 images, made on the device; never modified."""
    from oracle import combat_oracle as O
    hw = 256
    gen = torch.Generator(device="cuda").manual_seed(256)
    x = torch.rand(86, 3, hw, hw, generator=gen, device="cuda") * 2 - 1
    n8 = torch.zeros(100, hw, hw, 8, dtype=bf16, device="cuda")
    n8[..., :3] = torch.tanh(torch.randn(100, hw, hw, 3, generator=gen, device="cuda") * 3).to(bf16)
    d = [torch.randn(86, 3, hw, hw, generator=gen, device="cuda") for _ in range(2)]
    return x, n8, dev(O.lowpass_matrix(hw, RATIO)), d


@pytest.mark.parametrize("n", [43, 50])
def test_pair_backward_in_runs(ops, n):
    """2n = 86 rows: runs of 85 + 1, the second one inside the cross half.  2n = 100 rows: the first run ends at row 85,
    inside the cross half (rows 50 .. 84 of it read x[0 .. 34])."""
    hw = 256
    x, n8, pm, (d_bd, d_cross) = runs_case()
    x, rows, d_bd, d_cross = x[:n], n8[:2 * n], d_bd[:n], d_cross[:n]
    k1 = k1_of((0.4, 0.8))
    bd, bd2 = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(n, 3, hw, hw, device="cuda")
    ops.trigger_pair_fwd(x, rows, pm, k1, RATE, bd, bd2)
    l2s = 0.02 / bd.numel()
    dn = torch.full((2 * n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ref = torch.full_like(dn, float("nan"))
    ops.trigger_pair_bwd(x, rows, pm, k1, RATE, d_bd, bd, l2s, d_cross, dn, pre_tanh=True)
    ops.trigger_bwd(x, rows[:n], pm, k1[0], RATE, d_bd, bd, l2s, ref[:n], pre_tanh=True)
    ops.trigger_bwd(x, rows[n:], pm, k1[1], RATE, d_cross, None, 0.0, ref[n:], pre_tanh=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dn.float()).all())
    assert torch.equal(bits(dn), bits(ref))


def test_groups_backward_in_runs(ops):
    """86 images in chunks of 9 (ten groups, the last of 5): runs of 85 + 1 images, the second run's image takes the
    last group's kernel."""
    hw, n, ps = 256, 86, 9
    x, n8, pm, (d1, _) = runs_case()
    rows = n8[:n]
    groups = (n + ps - 1) // ps
    k1 = k1_of([0.15 + 0.8 * i / (groups - 1) for i in range(groups)])
    bd = torch.empty(n, 3, hw, hw, device="cuda")
    ops.trigger_groups_fwd(x, rows, pm, k1, ps, RATE, bd)
    l2s = 0.02 / bd.numel()
    dn = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ref = torch.full_like(dn, float("nan"))
    ops.trigger_groups_bwd(x, rows, pm, k1, ps, RATE, d1, bd, l2s, dn, pre_tanh=True)
    for ci in range(groups):
        si, ei = ci * ps, min(ci * ps + ps, n)
        ops.trigger_bwd(x[si:ei], rows[si:ei], pm, k1[ci], RATE, d1[si:ei], bd[si:ei], l2s, ref[si:ei], pre_tanh=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dn.float()).all())
    assert torch.equal(bits(dn), bits(ref))


# ------------------------------------------------------------------ 5: determinism
def test_pair_and_groups_deterministic(ops):
    """The same bits across four launches on the same operands, the library's deterministic mode off / on / off / on."""
    from combat_amd import engine
    from combat_amd._lib import lib
    hw, n, ps = 80, 3, 2
    x, _, n8, pm, (d_bd, d_bd2, d_cross) = clamp_case(hw, n, 2 * n)
    xc, k1 = dev(x), k1_of((0.4, 0.8))
    prev = bool(lib.combat_get_deterministic())
    got = []
    try:
        for mode in (False, True, False, True):
            engine.set_deterministic(mode)
            bd, bd2, out = (torch.empty(n, 3, hw, hw, device="cuda") for _ in range(3))
            mse, mse_g = torch.empty(3 * n, device="cuda"), torch.empty(3 * n, device="cuda")
            dn = torch.empty(2 * n, hw, hw, 8, dtype=bf16, device="cuda")
            dn_g = torch.empty(n, hw, hw, 8, dtype=bf16, device="cuda")
            ops.trigger_pair_fwd(xc, n8, pm, k1, RATE, bd, bd2, mse)
            ops.trigger_pair_bwd(xc, n8, pm, k1, RATE, d_bd, bd, 0.3, d_cross, dn, d_bd2=d_bd2)
            ops.trigger_groups_fwd(xc, n8[:n], pm, k1, ps, RATE, out, mse_g)
            ops.trigger_groups_bwd(xc, n8[:n], pm, k1, ps, RATE, d_bd, out, 0.3, dn_g, d_out2=d_bd2)
            got.append((bd, bd2, mse, bits(dn), out, mse_g, bits(dn_g)))
    finally:
        engine.set_deterministic(prev)
    torch.cuda.synchronize()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 6: refusals launch nothing
def test_refusals_launch_nothing():
    from combat_amd._lib import lib
    st = torch.cuda.current_stream().cuda_stream
    hw, n = 272, 1
    x = torch.zeros(n, 3, hw, hw, device="cuda")
    n8 = torch.zeros(2 * n, hw, hw, 8, dtype=bf16, device="cuda")
    pm = torch.zeros(hw, hw, device="cuda")
    k1 = torch.tensor([[0.25, 0.5, 0.25], [0.25, 0.5, 0.25]], device="cuda")
    out, out2, dn, mse = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(n8), torch.zeros(3 * n, device="cuda")
    p = lambda t: t.data_ptr()

    def pair_fwd(n, hw):
        return lib.combat_trigger_pair_fwd(p(x), p(n8), p(pm), p(k1), RATE, n, hw, p(out), p(out2), p(mse), st)

    def pair_bwd(n, hw, o=out, l2=0.0):
        return lib.combat_trigger_pair_bwd(p(x), p(n8), p(pm), p(k1), RATE, n, hw, p(out), None, p(o) if o is not None else None,
                                           l2, p(out2), 0, p(dn), st)

    def groups_fwd(n, hw, ps=1):
        return lib.combat_trigger_groups_fwd(p(x), p(n8), p(pm), p(k1), RATE, n, hw, ps, p(out), p(mse), st)

    def groups_bwd(n, hw, ps=1, o=out, l2=0.0):
        return lib.combat_trigger_groups_bwd(p(x), p(n8), p(pm), p(k1), RATE, n, hw, ps, p(out), None,
                                             p(o) if o is not None else None, l2, 0, p(dn), st)

    for call in (pair_fwd, pair_bwd, groups_fwd, groups_bwd):
        assert call(1, 72) == EINVAL        # on the strip route and not a multiple of 16
        assert call(1, 272) == EINVAL       # more columns than a workgroup has threads
        assert call(-1, 224) == EINVAL
        assert call(0, 224) == OK
    assert groups_fwd(1, 224, ps=0) == EINVAL and groups_bwd(1, 224, ps=0) == EINVAL
    assert pair_bwd(1, 224, o=None, l2=0.5) == EINVAL and groups_bwd(1, 224, o=None, l2=0.5) == EINVAL      # L2 term without out
    torch.cuda.synchronize()
    for t in (out, out2, dn, mse):
        assert float(t.float().abs().max()) == 0.0       # nothing was launched


# ------------------------------------------------------------------ 7: the steps against the CPU restatements
def _cunet224():
    from combat_amd import nets
    return seeded(lambda: nets.CUnetGeneratorv1(_opt224()), 3)


UNET_KEYS = ["up0", "up1", "up2", "up3", "noise"]
tol = lambda r: 1e-2 * max(1.0, abs(r))


def _gen_grad(total, pg, names_g):
    gr = torch.autograd.grad(total, [pg[k] for k in names_g], allow_unused=True)
    return torch.cat([(torch.zeros_like(pg[k]) if a is None else a).reshape(-1) for k, a in zip(names_g, gr)])


def test_inputaware_step_imagenet10_shape_b2():
    """One input-aware step at 3 x 224 x 224, ResNet18(input_size=224), b = 2 (second batch b = 2: the generator slot
    holds four images) against tests/inputaware_ref.py driven with the bf16-emulating networks.  Method of
    test_inputaware_gpu.py::test_inputaware_step_vs_restatement, tolerances of
    test_imagenet10_unet_gpu.py::test_alternated_step_imagenet10_shape_b4: Phase C from the identical start (loss 1e-2,
    gradient norm 3e-2); Phase G from the engine's post-Phase-C classifier with the generator emulation teacher-forced
    (triggered images bd and bd2 3e-5, losses 1e-2 * max(1, |ref|), loss_l2 1e-3, counters +-1, image gradients 0.25,
    generator gradient 5e-2)."""
    from combat_amd import nets, step as step_mod
    from oracle import combat_oracle as O
    b = 2
    netc, clean, netg, netf = _nets224()
    oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
    old_g = _oracle_state(netg)
    x, x2 = synth_images(b, 224, 5), synth_images(b, 224, 7)
    t = torch.tensor([0, 7])
    nb, sc, sg, sx, cw = 1, 0.5, 0.9, 0.3, 0.2
    cfg = O.StepConfig(num_classes=10, classifier="resnet18", lr_g=1e-3)
    ref = IR.inputaware_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)),
                             x, x2, t, IR.Randomness(nb, sc, sg, sx), cfg, cw,
                             clf_fn=E.resnet_forward_emu, gen_fn=E.unet_forward_emu)
    opt = _opt224()
    opt.cross_weight = cw
    st = step_mod.InputAwareStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), opt)
    st.keep_grads = True
    st.run(x.cuda(), t, x2.cuda(), step_mod.InputAwareRandomness(nb, sc, sg, [None] * 6, sigma_x=sx), lr_g=1e-3)
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    # ---- Phase C
    gn_c = float(st.eC.fp.grad.double().norm())
    print("loss_c %.5f / %.5f, gnorm_c %.5f / %.5f" % (m["loss_c_sum"], ref["loss_c"], gn_c, ref["gnorm_c"]))
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"])
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G, teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    names_g = O.trainable_names(old_g)
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + nm for nm, *_ in nets.UNET_LAYERS] + UNET_KEYS
    noise = E.unet_forward_emu(pg, torch.cat([x, x2]), force=stored(st.sG, keys, 3))
    ibd, ibd2 = O.trigger_mix(x, noise[:b], RATE, RATIO, sg), O.trigger_mix(x, noise[b:], RATE, RATIO, sx)
    e_bd, e_bd2 = float((st.bd.cpu() - ibd.detach()).abs().max()), float((st.bd2.cpu() - ibd2.detach()).abs().max())
    print("bd %.3g, bd2 %.3g" % (e_bd, e_bd2))
    assert e_bd < 3e-5 and e_bd2 < 3e-5
    bd_t = torch.zeros_like(t)
    leaf, leaf2 = ibd.detach().clone().requires_grad_(True), ibd2.detach().clone().requires_grad_(True)
    pred_bd, pred_cross = E.resnet_forward_emu(oc2, leaf, False), E.resnet_forward_emu(oc2, leaf2, False)
    cm_pred = E.resnet_forward_emu(ok, leaf, False)
    loss_ce, loss_cross, cm_loss = F.cross_entropy(pred_bd, bd_t), F.cross_entropy(pred_cross, t), F.cross_entropy(cm_pred, t)
    for ours, r in (("loss_ce_sum", loss_ce), ("loss_cross_sum", loss_cross), ("clean_model_loss_sum", cm_loss)):
        r = float(r.detach())
        print("%s %.5f / %.5f" % (ours, m[ours], r))
        assert abs(m[ours] - r) < tol(r), (ours, m[ours], r)
    l2 = float(F.mse_loss(ibd.detach(), x))
    assert abs(m["loss_l2_sum"] - l2) < 1e-3 * l2 + 1e-7
    assert abs(m["cross_correct"] - int((pred_cross.argmax(1) == t).sum())) <= 1
    assert abs(m["bd_correct"] - int((pred_bd.argmax(1) == bd_t).sum())) <= 1
    assert abs(m["clean_model_bd_ba"] - int((cm_pred.argmax(1) == t).sum())) <= 1
    assert abs(m["clean_model_bd_asr"] - int((cm_pred.argmax(1) == bd_t).sum())) <= 1
    (d_bd,) = torch.autograd.grad(loss_ce + cfg.clean_model_weight * cm_loss, leaf)
    (d_cross,) = torch.autograd.grad(cw * loss_cross, leaf2)
    e_dbd, e_dcross = rel_l2((st.d_bd + st.d_bd2).cpu(), d_bd), rel_l2(st.d_cross.cpu(), d_cross)
    print("image gradients: bd %.3g, cross %.3g" % (e_dbd, e_dcross))
    assert e_dbd < 0.25 and e_dcross < 0.25          # un-forced classifiers: mask-flip bound
    total = (ibd * (st.d_bd + st.d_bd2).cpu()).sum() + (ibd2 * st.d_cross.cpu()).sum() + cfg.l2_weight * F.mse_loss(ibd, x)
    e_g = rel_l2(flat_grads(st.eG.fp, names_g), _gen_grad(total, pg, names_g))
    print("generator gradient vs teacher-forced emulation %.3g" % e_g)
    assert e_g < 5e-2      # teacher-forced: pins the paired strip backward + the UNet backward of both halves


def test_multilabel_step_imagenet10_shape_b4():
    """One multi-label step at 3 x 224 x 224, b = 4 (four chunks of one image, classes 0 .. 3), num_bd = 1, against
    tests/multilabel_ref.py driven with the bf16-emulating networks; method of
    test_multilabel_gpu.py::test_multilabel_step_vs_restatement, tolerances as in the input-aware test above."""
    from combat_amd import nets, step as step_mod
    from oracle import combat_oracle as O
    b, nb, sc = 4, 1, 0.5
    netc, clean, _, netf = _nets224()
    netg = _cunet224()
    oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
    old_g = _oracle_state(netg)
    x = synth_images(b, 224, 5)
    t = torch.randint(0, 10, (b,), generator=g(6))
    bounds = MR.chunk_bounds(b, 10)
    assert bounds == [(0, 0, 1), (1, 1, 2), (2, 2, 3), (3, 3, 4)]
    sig = [0.7, 0.3, 0.9, 0.2]
    chunk = torch.arange(b)
    cfg = O.StepConfig(num_classes=10, classifier="resnet18", lr_g=1e-3)
    emu_gen = lambda p, xx, yy: MR.cunet_forward_emu(p, xx, yy, 10)
    ref = MR.multilabel_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)),
                             x, t, MR.Randomness(nb, sc, sig), cfg, clf_fn=E.resnet_forward_emu, gen_fn=emu_gen)
    st = step_mod.MultiLabelStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _opt224())
    st.keep_grads = True
    st.run(x.cuda(), t, step_mod.MultiLabelRandomness(nb, sc, sig[0], [None] * 5, sigma_chunks=sig), lr_g=1e-3)
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    # ---- Phase C
    gn_c = float(st.eC.fp.grad.double().norm())
    print("loss_c %.5f / %.5f, gnorm_c %.5f / %.5f" % (m["loss_c_sum"], ref["loss_c"], gn_c, ref["gnorm_c"]))
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"])
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G, teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    names_g = O.trainable_names(old_g)
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + nm for nm, *_ in nets.UNET_LAYERS] + UNET_KEYS
    assert st.eG.labels(st.sG).cpu().tolist() == chunk.tolist()
    noise = MR.cunet_forward_emu(pg, x, chunk, 10, force=stored(st.sG, keys, 3))
    ibd = torch.cat([O.trigger_mix(x[si:ei], noise[si:ei], RATE, RATIO, sig[ci]) for ci, si, ei in bounds])
    e_bd = float((st.bd.cpu() - ibd.detach()).abs().max())
    print("bd %.3g" % e_bd)
    assert e_bd < 3e-5
    leaf = ibd.detach().clone().requires_grad_(True)
    pred_bd, cm_pred = E.resnet_forward_emu(oc2, leaf, False), E.resnet_forward_emu(ok, leaf, False)
    loss_ce, cm_loss = F.cross_entropy(pred_bd, chunk), F.cross_entropy(cm_pred, t)
    for ours, r in (("loss_ce_sum", loss_ce), ("clean_model_loss_sum", cm_loss)):
        r = float(r.detach())
        print("%s %.5f / %.5f" % (ours, m[ours], r))
        assert abs(m[ours] - r) < tol(r), (ours, m[ours], r)
    l2 = float(F.mse_loss(ibd.detach(), x))
    assert abs(m["loss_l2_sum"] - l2) < 1e-3 * l2 + 1e-7
    assert abs(m["bd_correct"] - int((pred_bd.argmax(1) == chunk).sum())) <= 1
    assert abs(m["clean_model_bd_asr"] - int((cm_pred.argmax(1) == chunk).sum())) <= 1
    assert abs(m["clean_model_bd_ba"] - int((cm_pred.argmax(1) == t).sum())) <= 1
    (d_bd,) = torch.autograd.grad(loss_ce + cfg.clean_model_weight * cm_loss, leaf)
    e_dbd = rel_l2((st.d_bd + st.d_bd2).cpu(), d_bd)
    print("image gradient %.3g" % e_dbd)
    assert e_dbd < 0.25          # un-forced classifiers: mask-flip bound
    total = (ibd * (st.d_bd + st.d_bd2).cpu()).sum() + cfg.l2_weight * F.mse_loss(ibd, x)
    e_g = rel_l2(flat_grads(st.eG.fp, names_g), _gen_grad(total, pg, names_g))
    print("generator gradient vs teacher-forced emulation %.3g" % e_g)
    assert e_g < 5e-2      # teacher-forced: pins the grouped strip backward + the conditional UNet backward at 224 x 224


# ------------------------------------------------------------------ 8: the configuration's batch


def _finite_params(*mods):
    return all(bool(torch.isfinite(p).all()) for m in mods for p in m.parameters())


def test_inputaware_step_imagenet10_shape_b32():
    """One input-aware step at the configuration's batch of 32: the generator (slot G.pair) and netC (slot C.cross2)
    run over 64 images of 224 x 224.  Finite metrics and parameters; bd and bd2 within 2e-5 of oracle.trigger_mix
    applied to the engine's own generator output, each half under its own sigma."""
    from combat_amd import step as step_mod
    from oracle import combat_oracle as O
    b, sg, sx = 32, 0.9, 0.3
    netc, clean, netg, netf = _nets224()
    x, x2 = synth_images(b, 224, 5), synth_images(b, 224, 7)
    t = torch.randint(0, 10, (b,), generator=g(6))
    opt = _opt224()
    opt.cross_weight = 0.2
    st = step_mod.InputAwareStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), opt)
    st.run(x.cuda(), t, x2.cuda(), step_mod.InputAwareRandomness(3, 0.5, sg, [None] * 6, sigma_x=sx))
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    assert m["loss_cross_sum"] > 0
    noise = st.eG.output(st.sG)[..., :3].float().cpu().permute(0, 3, 1, 2)
    assert tuple(noise.shape) == (2 * b, 3, 224, 224) and bool(torch.isfinite(noise).all())
    e_bd = float((st.bd.cpu() - O.trigger_mix(x, noise[:b], RATE, RATIO, sg)).abs().max())
    e_bd2 = float((st.bd2.cpu() - O.trigger_mix(x, noise[b:], RATE, RATIO, sx)).abs().max())
    print("bd %.3g bd2 %.3g" % (e_bd, e_bd2))
    assert e_bd < 2e-5 and e_bd2 < 2e-5
    assert not torch.equal(noise[:b], noise[b:])
    assert _finite_params(netg, netc)


def test_multilabel_step_imagenet10_shape_b32():
    """One multi-label step at the configuration's batch of 32 (chunks of 4: eight classes).  Finite metrics and
    parameters; bd within 2e-5 of oracle.trigger_mix applied per chunk, with the chunk's sigma, to the engine's own
    generator output."""
    from combat_amd import step as step_mod
    from oracle import combat_oracle as O
    b = 32
    netc, clean, _, netf = _nets224()
    netg = _cunet224()
    x = synth_images(b, 224, 5)
    t = torch.randint(0, 10, (b,), generator=g(6))
    bounds = MR.chunk_bounds(b, 10)
    sig = [0.7, 0.3, 0.9, 0.2, 0.55, 0.15, 0.8, 0.45][:len(bounds)]
    assert len(bounds) == 8 and bounds[-1][2] == b
    st = step_mod.MultiLabelStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _opt224())
    st.run(x.cuda(), t, step_mod.MultiLabelRandomness(3, 0.5, sig[0], [None] * 5, sigma_chunks=sig))
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    noise = st.eG.output(st.sG)[..., :3].float().cpu().permute(0, 3, 1, 2)
    assert bool(torch.isfinite(noise).all())
    ibd = torch.cat([O.trigger_mix(x[si:ei], noise[si:ei], RATE, RATIO, sig[ci]) for ci, si, ei in bounds])
    e_bd = float((st.bd.cpu() - ibd).abs().max())
    print("bd %.3g" % e_bd)
    assert e_bd < 2e-5
    assert _finite_params(netg, netc)


# ------------------------------------------------------------------ 9: the scripts
def _script(script, *args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--dataset", "imagenet10", "--synthetic_size", "64",
           "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1", "--n_iters", "1"] + list(args)
    r = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def _clean_checkpoint(cwd):
    """The clean model's checkpoint the generator scripts load (--load_checkpoint_clean classifier_clean), written
    here from a seeded network: training one is tests/test_imagenet10_unet_gpu.py's workflow test."""
    from combat_amd import nets
    folder = os.path.join(cwd, "ckpt", "classifier_clean", "imagenet10")
    os.makedirs(folder)
    net = seeded(lambda: nets.ResNet18(num_classes=10, input_size=224), 2)
    torch.save({"netC": net.state_dict()}, os.path.join(folder, "imagenet10_classifier_clean.pth.tar"))
    return ("--load_checkpoint_clean", "classifier_clean")


def _ckpt(cwd, mode):
    return torch.load(os.path.join(cwd, "ckpt", mode, "imagenet10", "imagenet10_%s.pth.tar" % mode), map_location="cpu",
                      weights_only=True)


def _finite(sd):
    return all(bool(torch.isfinite(v.float()).all()) for v in sd.values())


def test_inputaware_workflow_imagenet10(tmp_path):
    """train_generator_inputaware.py, then train_victim_inputaware.py on its checkpoint, with --dataset imagenet10
    (bs forced to 32; 64 synthetic images: two batches for each of the two train loaders).  Checkpoint keys as
    tests/test_inputaware_gpu.py::test_inputaware_workflow_on_synthetic_data asserts them at 32 x 32."""
    from test_inputaware_gpu import GEN_KEYS
    cwd = str(tmp_path)
    clean = _clean_checkpoint(cwd)
    out = _script("train_generator_inputaware.py", "--saving_prefix", "inputaware", *clean, cwd=cwd)
    assert "Cross Acc:" in out and "Saving..." in out
    sd = _ckpt(cwd, "inputaware_clean")
    assert set(sd) == GEN_KEYS
    assert 0.0 <= sd["best_cross_acc"] <= 100.0
    assert sd["mask"].shape == (224, 224) and sd["pattern"].shape == (3, 224, 224)
    assert len(sd["netG"]) == 32 and len(sd["netC"]) == 122 and sd["netC"]["linear.weight"].shape == (10, 512 * 49)
    assert sd["optimizerG"]["param_groups"][0]["lr"] == pytest.approx(1e-3)      # lr_C * 0.1
    assert _finite(sd["netG"]) and _finite(sd["netC"]) and _finite(sd["clean_model"])
    out = _script("train_victim_inputaware.py", "--saving_prefix", "victim_ia", "--load_checkpoint", "inputaware_clean", cwd=cwd)
    assert "Cross Acc:" in out
    sd = _ckpt(cwd, "victim_ia_clean")
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "best_cross_acc",
                       "epoch_current"}
    assert sd["netC"]["linear.weight"].shape == (10, 512 * 49) and _finite(sd["netC"]) and _finite(sd["netG"])


def test_multilabel_workflow_imagenet10(tmp_path):
    """train_generator_multilabel.py, then train_victim_multilabel.py, with --dataset imagenet10: the checkpoint layout
    tests/test_multilabel_gpu.py::test_multilabel_workflow_on_synthetic_data asserts at 32 x 32."""
    from test_multilabel_cpu import GEN_KEYS
    cwd = str(tmp_path)
    clean = _clean_checkpoint(cwd)
    for script, prefix in (("train_generator_multilabel.py", "multilabel"), ("train_victim_multilabel.py", "victim_multilabel")):
        out = _script(script, "--saving_prefix", prefix, *clean, cwd=cwd)
        assert "Clean Model Bd ASR:" in out and "Saving..." in out, out[-2000:]
        sd = _ckpt(cwd, prefix + "_clean")
        assert set(sd) == GEN_KEYS
        for k in ("best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
                  "best_clean_model_bd_asr"):
            assert np.isfinite(sd[k]) and 0.0 <= sd[k] <= 100.0, (k, sd[k])
        assert sd["mask"].shape == (224, 224) and sd["pattern"].shape == (3, 224, 224)
        assert tuple(sd["netG"]["conv0_1.weight"].shape) == (64, 74, 3, 3)
        assert sd["netC"]["linear.weight"].shape == (10, 512 * 49)
        assert sd["optimizerG"]["param_groups"][0]["lr"] == pytest.approx(1e-3)      # lr_C * 0.1
        assert _finite(sd["netG"])
        assert all(bool(torch.isfinite(v).all()) for v in sd["netC"].values() if v.dtype.is_floating_point)
