"""Grad-CAM oracle for the tests (test infrastructure): torch autograd in fp32 on the pre-activation classifier with the
tapped block's output kept, and the same under the classifier's bf16 dataflow -- tests/bf16_emu.py::preact_forward_emu
restated with a tap, which that function does not offer.  The fixture is the one the constants of
tests/test_gradcam_cpu.py were measured on: torch.manual_seed(3) weights, BatchNorm buffers from seed 11, eight uniform
uint8 noise images from default_rng(5)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import bf16_emu as E

TAPS = (5, 3, 4)        # layer3[1] (the reference's); layer2[1]: its successor has a convolutional shortcut, 16 x 16 x 128;
#                         layer3[0]: an identity successor
N_IMAGES = 8


def randomize_bn_buffers(net, seed):
    """tests/golden/make_golden.py::randomize_bn_buffers."""
    i = 0
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.05, generator=torch.Generator().manual_seed(seed + i))
                mod.running_var.uniform_(0.6, 1.4, generator=torch.Generator().manual_seed(seed + 1000 + i))
                i += 1
    return net


def make_net():
    """The fixture's classifier (on the CPU, eval mode)."""
    from combat_amd import nets
    torch.manual_seed(3)
    return randomize_bn_buffers(nets.PreActResNet18(), 11).eval()


@functools.lru_cache(maxsize=None)
def fixture():
    """(state dict, uint8 images [8][32][32][3], float32 NCHW batch in [-1, 1])."""
    p = {k: v.detach().clone() for k, v in make_net().state_dict().items()}
    u8 = np.random.default_rng(5).integers(0, 256, (N_IMAGES, 32, 32, 3), dtype=np.uint8)
    x = (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5
    return p, u8, x.contiguous()


def tapped_forward(p, x, tap, rounded):
    """(logits, the raw output of block `tap`) -- bf16_emu.preact_forward_emu's dataflow in eval mode; rounded=False: no
    rounding anywhere, the fp32 oracle (oracle/combat_oracle.py::preact_resnet18_forward)."""
    q = E.q if rounded else (lambda t: t)
    t = q(F.conv2d(x, q(p["conv1.weight"]), padding=1))
    b, kept = 0, None
    for layer, stride0 in ((1, 1), (2, 2), (3, 2), (4, 2)):
        for blk in (0, 1):
            pre = "layer%d.%d." % (layer, blk)
            stride = stride0 if blk == 0 else 1
            a1 = q(F.relu(E._bn_affine(p, pre + "bn1", t, False)))
            sck = pre + "shortcut.0.weight"
            sc = q(F.conv2d(a1, q(p[sck]), stride=stride)) if sck in p else t
            y1 = q(F.conv2d(a1, q(p[pre + "conv1.weight"]), stride=stride, padding=1))
            a2 = q(F.relu(E._bn_affine(p, pre + "bn2", y1, False)))
            t = q(F.conv2d(a2, q(p[pre + "conv2.weight"]), padding=1) + sc)
            if b == tap:
                kept = t
            b += 1
    feat = F.avg_pool2d(t, 4).flatten(1)
    return F.linear(feat, p["linear.weight"], p["linear.bias"]), kept


@functools.lru_cache(maxsize=None)
def gradcam(tap, rounded):
    """Grad-CAM of the fixture at block `tap`: dict of logits [n][10], chosen [n] (the FP32 oracle's argmax, also where
    rounded: the parity tests always pass the index), act / grad float32 NHWC [n][f][f][C], raw [n][f][f] and cam
    [n][32][32] (fp64, combat_amd.defenses.gradcam_map_reference)."""
    from combat_amd import defenses as D
    p, _, x = fixture()
    x = x.clone().requires_grad_(True)        # (the weights need no gradient; the input makes the graph)
    logits, kept = tapped_forward(p, x, tap, rounded)
    chosen = logits.detach().argmax(1) if not rounded else torch.from_numpy(gradcam(tap, False)["chosen"]).long()
    grad, = torch.autograd.grad(logits.gather(1, chosen[:, None]).sum(), kept)
    act = kept.detach().permute(0, 2, 3, 1).contiguous().numpy()
    grad = grad.permute(0, 2, 3, 1).contiguous().numpy()
    cam, raw, weights = D.gradcam_map_reference(act, grad)
    return dict(logits=logits.detach().numpy(), chosen=chosen.numpy().astype(np.int32), act=act, grad=grad, raw=raw, cam=cam,
                weights=weights)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def raw_distance(got, want):
    """Largest error of the pre-ReLU maps [n][f][f], per image relative to the image's own max |raw|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))).max())


def map_bounds(act, grad):
    """(bound on |raw - exact| [n], bound on |cam - exact| [n]) for fp32 arithmetic on act, grad [n][f][f][C], with
    u = 2^-24 and every sum of k terms carrying at most k * u of the sum of its terms' magnitudes, in any order:
      weights[c]: P = f * f terms and the scaling -- (P + 1) * u * mean_p |grad[p][c]|;
      raw[p]:     C products (rounded or fused) and C additions on top of the weights' error --
                  (P + 1 + 2 * C) * u * S[p],  S[p] = sum_c mean_p' |grad[p'][c]| * |act[p][c]|;  bound_raw = its maximum;
      resize:     ReLU moves nothing further apart; two blends of two products and a sum each, 6 roundings of values
                  within max |raw|: bound_u = bound_raw + 6 * u * max |raw|;
      cam:        (u - min) / (max - min): numerator and denominator each off by 2 * bound_u (+ a rounding), a quotient
                  in [0, 1] over the exact range R: (4 * bound_u) / (R - 2 * bound_u) + 3 * u."""
    act, grad = np.asarray(act, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    n, f, _, c = act.shape
    u, P = 2.0 ** -24, f * f
    mean_abs = np.abs(grad).reshape(n, P, c).mean(axis=1)
    S = (mean_abs[:, None, :] * np.abs(act).reshape(n, P, c)).sum(axis=2)
    bound_raw = (P + 1 + 2 * c) * u * S.max(axis=1)
    from combat_amd import defenses as D
    _, raw, _ = D.gradcam_map_reference(act, grad)
    up = D.gradcam_resize_reference(np.maximum(raw, 0))
    R = up.max(axis=(1, 2)) - up.min(axis=(1, 2))
    bound_u = bound_raw + 6 * u * np.abs(raw).max(axis=(1, 2))
    return bound_raw, 4 * bound_u / (R - 2 * bound_u) + 3 * u
