"""The strip form of the trigger kernels (64 < hw <= 256: ImageNet-10's 224 x 224) against oracle.trigger_mix.

Shapes: (hw, n) = (80, 3) is the smallest size on the strip route (five strips, an odd count, K = 52 kept DCT rows);
(224, 2) is the real size (14 strips, K = 145).  Bounds are those of test_kernels_gpu.py::test_trigger_forward_backward.

The clamp mask is recomputed by the backward in fp32.  It can only differ from the oracle's where a pre-clamp value lies
closer to +-1 than the fp32 error of P noise P (2.4e-6 at 224, before the factor 0.08), so every case first asserts, on
the fp64 oracle, that no pre-clamp value lies within 1e-6 of +-1 (nearest: 5.7e-6 at (80, 3), 3.7e-6 at (224, 2)).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
RATE, RATIO = 0.08, 0.65
EINVAL, OK = -1, 0


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


def dev(t):
    return t.to("cuda")


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def g(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def case(hw, n):
    """Inputs shared by every test of one shape (never modified): images, bf16-rounded noise, the c8 noise on the device."""
    from oracle import combat_oracle as O
    x = ((torch.randint(0, 256, (n, 3, hw, hw), generator=g(190)).float() / 255) - 0.5) / 0.5
    noise = torch.tanh(torch.randn(n, 3, hw, hw, generator=g(191)) * 3).to(bf16).float()
    n8 = torch.zeros(n, hw, hw, 8, dtype=bf16, device="cuda")
    n8[..., :3] = dev(noise.permute(0, 2, 3, 1).contiguous().to(bf16))
    pre = x.double() + O.low_freq(noise.double(), RATIO) * RATE
    margin = float(torch.minimum((pre - 1).abs(), (pre + 1).abs()).min())
    return x, noise, n8, dev(O.lowpass_matrix(hw, RATIO)), margin


@functools.lru_cache(maxsize=None)
def reference(hw, n, sigma):
    """oracle.trigger_mix and the gradient of sum(ref * d_out) + l2s * sum((ref - x)^2) with respect to the noise."""
    from oracle import combat_oracle as O
    x, noise, _, _, _ = case(hw, n)
    nz = noise.clone().requires_grad_(True)
    ref = O.trigger_mix(x, nz, RATE, RATIO, sigma)
    d_out = torch.randn(n, 3, hw, hw, generator=g(192))
    l2s = 0.02 / ref.numel()
    (ref * d_out).sum().add(l2s * ((ref - x) ** 2).sum()).backward()
    return ref.detach(), d_out, l2s, nz.grad


SHAPES = [(80, 3), (224, 2)]


@pytest.mark.parametrize("sigma", [0.35, 0.9])
@pytest.mark.parametrize("hw,n", SHAPES)
def test_trigger_big_forward_backward(ops, hw, n, sigma):
    from oracle import combat_oracle as O
    x, noise, n8, pm, margin = case(hw, n)
    print("nearest pre-clamp value to +-1: %.3g" % margin)
    assert margin > 1e-6
    ref, d_out, l2s, d_ref = reference(hw, n, sigma)
    k1 = dev(O.gaussian_kernel1d(sigma))
    out = torch.empty(n, 3, hw, hw, device="cuda")
    out8 = torch.empty(n, hw, hw, 8, dtype=bf16, device="cuda")
    mse = torch.empty(3 * n, device="cuda")
    ops.trigger_fwd(dev(x), n8, pm, k1, RATE, out, out8, mse)
    err = (out.cpu() - ref).abs()
    rows = {r: float(err[:, :, r].max()) for r in (0, 15, 16, hw - 1)}       # the reflect edges and a seam
    e_mse = rel_l2(mse.view(n, 3), ((ref - x) ** 2).sum((2, 3)))
    hi, lo = out8[..., :3].float().cpu(), out8[..., 3:6].float().cpu()
    e_c8 = float(((hi + lo).permute(0, 3, 1, 2) - ref).abs().max())
    print("out %.3g rows %s mse %.3g c8 %.3g" % (float(err.max()), rows, e_mse, e_c8))
    assert float(err.max()) < 2e-5
    for r, e in rows.items():
        assert e < 2e-5, r
    assert e_mse < 1e-4
    assert e_c8 < 3e-5
    assert float(out8[..., 6:].float().abs().max()) == 0.0
    # the poisoned sub-batch: output image i from row src_index[i] of the images and of the generator output
    idx = torch.tensor([n - 1, 0], dtype=torch.int32)
    sub = torch.empty(2, 3, hw, hw, device="cuda")
    sub_mse = torch.empty(6, device="cuda")
    ops.trigger_fwd(dev(x), n8, pm, k1, RATE, sub, mse_partial=sub_mse, src_index=dev(idx))
    assert torch.equal(sub, out[idx.long().cuda()])
    assert torch.equal(sub_mse.view(2, 3), mse.view(n, 3)[idx.long().cuda()])
    dn = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ops.trigger_bwd(dev(x), n8, pm, k1, RATE, dev(d_out * 0.25), out, l2s, dn, d_out2=dev(d_out * 0.75))   # two shares of one gradient
    e_dn = rel_l2(dn.float().cpu().permute(0, 3, 1, 2)[:, :3], d_ref)
    print("d_noise %.3g" % e_dn)
    assert e_dn < 4e-3
    assert float(dn[..., 3:].float().abs().max()) == 0.0
    # pre_tanh: the gradient with respect to z, noise = tanh(z)
    dz = torch.empty_like(dn)
    ops.trigger_bwd(dev(x), n8, pm, k1, RATE, dev(d_out), out, l2s, dz, pre_tanh=True)
    assert rel_l2(dz.float().cpu().permute(0, 3, 1, 2)[:, :3], d_ref * (1 - noise ** 2)) < 4e-3


@pytest.mark.parametrize("hw,n", SHAPES)
def test_trigger_big_deterministic(ops, hw, n):
    """Two launches on the same operands give the same bits, with the library's deterministic mode off and on."""
    from combat_amd import engine
    from combat_amd._lib import lib
    from oracle import combat_oracle as O
    x, _, n8, pm, _ = case(hw, n)
    _, d_out, l2s, _ = reference(hw, n, 0.9)
    xd, k1, gd = dev(x), dev(O.gaussian_kernel1d(0.9)), dev(d_out)
    prev = bool(lib.combat_get_deterministic())
    got = []
    try:
        for mode in (False, True, False, True):
            engine.set_deterministic(mode)
            out = torch.empty(n, 3, hw, hw, device="cuda")
            mse = torch.empty(3 * n, device="cuda")
            dn = torch.empty(n, hw, hw, 8, dtype=bf16, device="cuda")
            ops.trigger_fwd(xd, n8, pm, k1, RATE, out, None, mse)
            ops.trigger_bwd(xd, n8, pm, k1, RATE, gd, out, l2s, dn)
            got.append((out, mse, dn))
    finally:
        engine.set_deterministic(prev)
    for o, m, d in got[1:]:
        assert torch.equal(o, got[0][0]) and torch.equal(m, got[0][1]) and torch.equal(d.view(torch.int16), got[0][2].view(torch.int16))


def test_trigger_big_hw256_and_runs_of_images(ops):
    """hw = 256, the largest size (every thread of a workgroup owns a column): the forward against the oracle on two
    images, bound as above.  And a backward over 86 images: the clamp mask of one 256 x 256 image is 24 KB, so 85 fit the
    2 MB scratch of a stream and the launcher takes the batch as runs of 85 and 1 images -- which must write the bits of
    two separate calls on those runs."""
    from oracle import combat_oracle as O
    hw, n, run = 256, 86, 85
    x = ((torch.randint(0, 256, (n, 3, hw, hw), generator=g(193), dtype=torch.uint8).float() / 255) - 0.5) / 0.5
    noise = torch.tanh(torch.randn(n, 3, hw, hw, generator=g(194)) * 3).to(bf16)
    xd = dev(x)
    n8 = torch.zeros(n, hw, hw, 8, dtype=bf16, device="cuda")
    n8[..., :3] = dev(noise).permute(0, 2, 3, 1)
    pm, k1 = dev(O.lowpass_matrix(hw, RATIO)), dev(O.gaussian_kernel1d(0.6))
    out = torch.empty(n, 3, hw, hw, device="cuda")
    ops.trigger_fwd(xd, n8, pm, k1, RATE, out)
    ref = O.trigger_mix(x[:2], noise[:2].float(), RATE, RATIO, 0.6)
    assert float((out[:2].cpu() - ref).abs().max()) < 2e-5
    d_out = torch.randn(n, 3, hw, hw, generator=g(195), device="cpu").cuda()
    l2s = 0.02 / out.numel()
    whole = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    parts = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ops.trigger_bwd(xd, n8, pm, k1, RATE, d_out, out, l2s, whole, pre_tanh=True)
    for lo, hi in ((0, run), (run, n)):
        ops.trigger_bwd(xd[lo:hi], n8[lo:hi], pm, k1, RATE, d_out[lo:hi], out[lo:hi], l2s, parts[lo:hi], pre_tanh=True)
    assert bool(torch.isfinite(whole.float()).all())
    assert torch.equal(whole.view(torch.int16), parts.view(torch.int16))


def test_trigger_big_argument_checks():
    from combat_amd._lib import lib
    st = torch.cuda.current_stream().cuda_stream
    hw, n = 272, 1
    x = torch.zeros(n, 3, hw, hw, device="cuda")
    n8 = torch.zeros(n, hw, hw, 8, dtype=bf16, device="cuda")
    pm = torch.zeros(hw, hw, device="cuda")
    k1 = torch.tensor([0.25, 0.5, 0.25], device="cuda")
    out, dn, mse = torch.zeros_like(x), torch.zeros_like(n8), torch.zeros(3 * n, device="cuda")

    def fwd(n, hw):
        return lib.combat_trigger_fwd(x.data_ptr(), n8.data_ptr(), pm.data_ptr(), k1.data_ptr(), RATE, n, hw, None,
                                      out.data_ptr(), None, mse.data_ptr(), st)

    def bwd(n, hw):
        return lib.combat_trigger_bwd(x.data_ptr(), n8.data_ptr(), pm.data_ptr(), k1.data_ptr(), RATE, n, hw, out.data_ptr(),
                                      None, out.data_ptr(), 0.0, 0, dn.data_ptr(), st)

    for call in (fwd, bwd):
        assert call(1, 72) == EINVAL        # on the strip route and not a multiple of 16
        assert call(1, 272) == EINVAL       # more columns than a workgroup has threads
        assert call(-1, 224) == EINVAL
        assert call(0, 224) == OK
    # the variants that stay whole-plane keep their limit
    assert lib.combat_trigger_tv_bwd(x.data_ptr(), n8.data_ptr(), pm.data_ptr(), k1.data_ptr(), RATE, 1, 224, out.data_ptr(), None,
                                     out.data_ptr(), 0.0, 0.0, 0, dn.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(dn.float().abs().max()) == 0.0       # nothing was launched
