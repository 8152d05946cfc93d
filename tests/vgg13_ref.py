"""CPU restatements for the VGG13 victim (test infrastructure; the reference module is classifier_models/vgg.py).

  * forward(p, x, train): the module's dataflow over a state dict, functional (torch.autograd gives the gradients).
    emu=True rounds to bf16 exactly where combat_amd.engine.VggEngine stores bf16 (tests/bf16_emu.py's conventions:
    straight-through rounding, `force` = teacher forcing with the engine's stored tensors).
  * pool_relu_bwd / flat_head / flat_head_bwd: what the three new entry points compute, element for element.
  * sgd_nesterov: torch.optim.SGD(momentum, weight_decay, nesterov=True) on tensors.
  * fixture plumbing shared by the tests and tests/golden/make_golden_vgg13.py (batches, seeds, checksum).
"""
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402

CONV_IDX = (0, 3, 7, 10, 14, 17, 21, 24, 28, 31)     # features.<i> of the ten convolutions; the BatchNorm is i + 1
POOL_AFTER = (1, 3, 5, 7, 9)                         # layers (0-based) followed by the 2x2 max-pool
CASES = {"c32": dict(hw=32, classes=10), "c64": dict(hw=64, classes=8)}
SEED_NET, SEED_BN, N = 0, 500, 16
SEEDS = {"c32": 4100, "c64": 4200}                   # base of a case's image / label seeds
TRACE_STEPS, TRACE_POOL = 10, 2                      # the trace alternates over two batches (fresh random labels every
#                                                      step make the fp32 reference itself diverge within five steps)
SGD = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)


def rng(seed):
    return torch.Generator().manual_seed(seed)


def synth_images(b, hw, seed):
    """tests/golden/make_golden.py::synth_images."""
    u8 = torch.randint(0, 256, (b, 3, hw, hw), generator=rng(seed), dtype=torch.uint8)
    return (u8.float() / 255 - 0.5) / 0.5


def randomize_bn_buffers(net, seed):
    """tests/golden/make_golden.py::randomize_bn_buffers."""
    i = 0
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.05, generator=rng(seed + i))
                m.running_var.uniform_(0.6, 1.4, generator=rng(seed + 1000 + i))
                i += 1
    return net


def batch(case, k):
    """Batch k of a case: 0 = the train batch, 1 = the eval batch, 2 and 3 = the pool the loss trace alternates over."""
    c = CASES[case]
    x = synth_images(N, c["hw"], SEEDS[case] + 2 * k)
    t = torch.randint(0, c["classes"], (N,), generator=rng(SEEDS[case] + 2 * k + 1))
    return x, t


def checksum(state_dict):
    """sha256 over the fp32 / int64 bytes of every entry in order: pins bit-identical seeded initialisation."""
    h = hashlib.sha256()
    for k, v in state_dict.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def engine_image(x):
    """The image as the engine's first convolution reads it: the hi/lo split of its input buffer, bf16(x) + bf16(x -
    bf16(x)) (include/combat_hip.h, "images that enter a network").  A rounding point like the stored tensors: ten
    BatchNorm layers at 16 images amplify this 2^-17 difference to 4e-3 in the loss of the 64 x 64 case, more than the whole
    distance between the emulation and fp32, so an emulated pass that is compared with the engine starts from it."""
    hi = x.to(torch.bfloat16).float()
    return hi + (x - hi).to(torch.bfloat16).float()


def forward(p, x, train, emu=False, force=None, taps=None):
    """logits of VGG13 over the state dict `p` (train mode updates p's running statistics in place).
    emu: bf16 rounding of the stored tensors ('l%d.y' raw conv output + bias, 'l%d.a' = relu(bn(.))) and of the conv
    weights, as the engine computes it; force: {engine slot buffer name: NCHW fp32 tensor} (bf16_emu.q)."""
    qq = (lambda t, key=None: E.q(t, force, key)) if emu else (lambda t, key=None: t)
    cur = x
    for l, i in enumerate(CONV_IDX):
        conv, bn = "features.%d" % i, "features.%d" % (i + 1)
        w = E.q(p[conv + ".weight"]) if emu else p[conv + ".weight"]
        y = qq(F.conv2d(cur, w, p[conv + ".bias"], padding=1), "l%d.y" % l)
        if train:
            z = E._bn_affine(p, bn, y, True)
        else:
            s, t = E._bn_eval_tables(p, bn)
            z = y * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
        cur = qq(F.relu(z), "l%d.a" % l)
        if taps is not None:
            taps["l%d.y" % l], taps["l%d.a" % l] = y, cur
        if l in POOL_AFTER:
            cur = F.max_pool2d(cur, 2, 2)
    return F.linear(cur.flatten(1), p["classifier.weight"], p["classifier.bias"])


def loss_and_grads(p, names, x, t, train=True, **kw):
    """(logits, loss, [gradient per name]) of mean cross-entropy; p's named entries must require grad."""
    logits = forward(p, x, train, **kw)
    loss = F.cross_entropy(logits, t)
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return logits.detach(), loss.detach(), [torch.zeros_like(p[k]) if g is None else g for k, g in zip(names, grads)]


def sgd_nesterov(param, grad, buf, lr, momentum, weight_decay):
    """One torch.optim.SGD(nesterov=True) update; buf None = the first step.  Returns (param, buf)."""
    g = grad + weight_decay * param
    buf = g.clone() if buf is None else momentum * buf + g
    return param - lr * (g + momentum * buf), buf


def loss_trace(p, names, case, steps=TRACE_STEPS, **kw):
    """Losses of `steps` SGD steps over batch(case, 2 + s % TRACE_POOL) from the state dict p (modified in place)."""
    bufs, out = {k: None for k in names}, []
    for s in range(steps):
        x, t = batch(case, 2 + s % TRACE_POOL)
        for k in names:
            p[k] = p[k].detach().requires_grad_(True)
        _, loss, grads = loss_and_grads(p, names, x, t, True, **kw)
        out.append(float(loss))
        with torch.no_grad():
            for k, g in zip(names, grads):
                p[k], bufs[k] = sgd_nesterov(p[k].detach(), g, bufs[k], **SGD)
    return np.array(out)


# ---------------------------------------------------------------- the new entry points, element for element


def pool_relu_bwd(a, g):
    """combat_maxpool2_relu_bwd: a [n][h][w][C] (post-ReLU), g [n][h/2][w/2][C] -> d_a like a.  The pooled gradient
    goes to the first maximum in the order (0,0), (0,1), (1,0), (1,1) (strict `>` scan) if it is > 0."""
    n, h, w, c = a.shape
    win = a.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)
    best, arg = win[..., 0, :].clone(), torch.zeros(n, h // 2, w // 2, c, dtype=torch.int64)
    for k in range(1, 4):
        better = win[..., k, :] > best
        best = torch.where(better, win[..., k, :], best)
        arg = torch.where(better, torch.full_like(arg, k), arg)
    out = torch.zeros_like(win)
    out.scatter_(3, arg.unsqueeze(3), torch.where(best > 0, g, torch.zeros_like(g)).unsqueeze(3))
    return out.reshape(n, h // 2, w // 2, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, h, w, c)


def flat_nchw(feat):
    """[n][hw][hw][C] -> [n][C*hw*hw] in torch's NCHW flatten order (out.view(out.size(0), -1), vgg.py:27)."""
    return feat.permute(0, 3, 1, 2).reshape(feat.shape[0], -1)


def flat_head(feat, W, b):
    return flat_nchw(feat) @ W.t() + b


def flat_head_bwd(feat, W, dlogits):
    """(d_feat [n][hw][hw][C], dW, db) of logits = flat_head(feat, W, b) for the logits' gradient dlogits."""
    n, hw, _, c = feat.shape
    d_feat = (dlogits @ W).reshape(n, c, hw, hw).permute(0, 2, 3, 1)
    return d_feat, dlogits.t() @ flat_nchw(feat), dlogits.sum(0)
