"""Defenses evaluated against a trained backdoor.  Fine-pruning (reference defenses/fine_pruning/fine-pruning.py;
Liu et al., RAID 2018, without the fine-tuning half, as the reference: ":166 no-tuning after pruning a channel").

The reference forwards the test set once with a hook on ``layer4`` (:144-157), sorts the channels by mean activation
(:160-163) and then, for each of the C = 512 pruning levels, rebuilds ``layer4[1].conv2`` and ``linear`` without the
pruned channels (:168-211) and evaluates the whole test set, clean and backdoored (:213).  The pruned network's logits
are ``b + sum over kept c of W[:, c] . pooled[:, c]`` of the UNPRUNED network's pooled features,
so here the curve costs one clean pass, one backdoor pass and combat_prune_sweep per batch.

STRIP (reference defenses/STRIP/STRIP.py; Gao et al., ACSAC 2019): a background image is superimposed with n_sample test
images and scored by the mean entropy of the classifier's predictions on the blends.  The reference builds every blend on
the host (:60-75); here combat_strip_superimpose writes the classifier's input buffer from the uint8 sources and
combat_strip_entropy reads the head's logits, a group of backgrounds per classifier pass."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import api, ops


def require_single_process(what: str = "fine-pruning") -> None:
    """The defense scripts keep their counters on one GPU; under a multi-process launch every rank would write the same
    outfile from its own copy of the whole test set.  `what` names the defense in the message."""
    world = int(os.environ.get("WORLD_SIZE", 1))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        world = max(world, torch.distributed.get_world_size())
    if world > 1:
        raise RuntimeError("%s runs on a single GPU: started with world size %d (launch one process, "
                           "without torchrun)" % (what, world))


def stable_order(activation: np.ndarray) -> np.ndarray:
    """seq_sort (fine-pruning.py:162): channel indices by ascending mean activation; equal means keep index order."""
    return np.argsort(np.asarray(activation, dtype=np.float64), kind="stable").astype(np.int64)


def sweep_reference(pooled: np.ndarray, weight: np.ndarray, bias: np.ndarray, order: np.ndarray, per: int,
                    dtype=np.float64) -> np.ndarray:
    """combat_prune_sweep's arithmetic restated on the host: logits [C][n][classes] of every pruning level, summed in the
    kernel's order (from the channel pruned last to the one pruned first) in `dtype`.  Products are exact in fp64 for
    fp32 inputs, so dtype=float64 is the reference sum; for inputs on a grid coarse enough that every partial sum is
    exact in fp32 it equals the kernel bit for bit."""
    pooled, weight = np.asarray(pooled, dtype=dtype), np.asarray(weight, dtype=dtype)
    c = len(order)
    s = np.broadcast_to(np.asarray(bias, dtype=dtype), (pooled.shape[0], weight.shape[0])).copy()
    out = np.empty((c,) + s.shape, dtype=dtype)
    for k in range(c - 1, -1, -1):
        for q in range(per):
            f = int(order[k]) * per + q
            s = s + pooled[:, f:f + 1] * weight[None, :, f]
        out[k] = s
    return out


def write_curve(path: str, acc_clean, acc_bd) -> None:
    """One line per pruning level, fine-pruning.py:214."""
    with open(path, "w") as outs:
        for index, (clean, bd) in enumerate(zip(acc_clean, acc_bd)):
            outs.write("%d %0.4f %0.4f\n" % (index, clean, bd))


class FinePruning:
    """observe() every test batch (pass 1), then sweep() the clean and the backdoored pooled features of every batch
    (pass 2); curve() is the reference's outfile.  The classifier is a combat_amd.nets PreActResNet18 / ResNet18 in
    eval mode; its last block's C output channels are the prunable ones and `linear` sees per = in / C cells of each."""

    def __init__(self, netC, opt=None):
        self.netC, self.opt = netC, opt
        self.C = netC.layer4[1].conv2.out_channels
        self.fin = netC.linear.in_features
        self.classes = netC.linear.out_features
        if self.fin % self.C:
            raise ValueError("linear.in_features %d is not a multiple of layer4's %d channels" % (self.fin, self.C))
        self.per = self.fin // self.C
        dev = netC.linear.weight.device
        self.sums = torch.zeros(self.fin, dtype=torch.float64, device=dev)
        self.seen = 0
        # [clean | backdoor][labels | second label set][level]
        self.correct = torch.zeros(2, 2, self.C, dtype=torch.int32, device=dev)
        self.swept = [0, 0]
        self._order_dev = None

    # ---- pass 1
    def observe(self, inputs: torch.Tensor) -> None:
        pooled = api.pooled_features(self.netC, inputs)
        ops.feature_colsum(pooled, self.sums)
        self.seen += pooled.shape[0]
        self._order_dev = None

    def activation(self) -> np.ndarray:
        """fp64 [C]: torch.mean(layer4 output, dim=[0, 2, 3]) (:161) -- the mean of a 4 x 4 window mean over the windows
        of a channel and the images is the mean over all of the channel's pixels."""
        if not self.seen:
            raise RuntimeError("FinePruning.activation: observe() the test set first")
        sums = self.sums.cpu().numpy().reshape(self.C, self.per)
        total = sums[:, 0].copy()
        for q in range(1, self.per):
            total += sums[:, q]
        return total / (float(self.seen) * self.per)

    def order(self) -> torch.Tensor:
        return torch.from_numpy(stable_order(self.activation()))

    # ---- pass 2
    def sweep(self, pooled: torch.Tensor, targets: torch.Tensor, targets2: Optional[torch.Tensor] = None,
              order: Optional[torch.Tensor] = None, backdoor: bool = False) -> None:
        """Add this batch to the per-level counters of the clean (default) or the backdoor set: predictions against
        `targets`, and against `targets2` if given (the true labels of backdoored images, say)."""
        if order is None:
            if self._order_dev is None:
                self._order_dev = self.order().to(device=pooled.device, dtype=torch.int32)
            order_dev = self._order_dev
        else:
            order_dev = torch.as_tensor(order).to(device=pooled.device, dtype=torch.int32).contiguous()
        if order_dev.numel() != self.C:
            raise ValueError("sweep: order has %d entries, the layer %d channels" % (order_dev.numel(), self.C))
        if tuple(pooled.shape[1:]) != (self.fin,) or pooled.dtype != torch.float32:
            raise ValueError("sweep: pooled must be fp32 [n][%d], got %s %s" % (self.fin, pooled.dtype, tuple(pooled.shape)))
        which = int(bool(backdoor))
        lin = self.netC.linear
        cells = self.correct[which]
        ops.prune_sweep(pooled.contiguous(), lin.weight.data.contiguous(), lin.bias.data, order_dev, self.per,
                        targets.to(device=pooled.device, dtype=torch.int64), cells[0],
                        None if targets2 is None else targets2.to(device=pooled.device, dtype=torch.int64),
                        None if targets2 is None else cells[1])
        self.swept[which] += pooled.shape[0]

    def counts(self) -> np.ndarray:
        """int64 [2][2][C] copy of the counters ([clean | backdoor][targets | targets2][level])."""
        return self.correct.cpu().numpy().astype(np.int64)

    def curve(self) -> Tuple[np.ndarray, np.ndarray]:
        """(acc_clean[C], acc_bd[C]) in percent (:81-82, per level)."""
        c = self.counts()
        return c[0, 0] * 100.0 / max(self.swept[0], 1), c[1, 0] * 100.0 / max(self.swept[1], 1)


# ---------------------------------------------------------------------------------------------- STRIP


def strip_blend_reference(bg: np.ndarray, overlay: np.ndarray, norm_cols: int = 3) -> np.ndarray:
    """combat_strip_superimpose's arithmetic restated on the host for uint8 [..., H, W, 3] images: float32 [..., 3, H, W].
    cv2.addWeighted(bg, 1, overlay, 1, 0) on uint8 is min(bg + overlay, 255) (STRIP.py:61); ToTensor is HWC -> CHW and a
    true division by 255; Normalize.__call__ (:27-31) indexes x[:, :, channel] of that CHW tensor, the width axis, so
    columns < norm_cols (3 in the reference) become (v - 0.5) / 0.5 and the others stay in [0, 1]."""
    s = np.minimum(np.asarray(bg).astype(np.int32) + np.asarray(overlay).astype(np.int32), 255)
    v = np.moveaxis(s.astype(np.float32) / np.float32(255.0), -1, -3).copy()
    v[..., :norm_cols] = (v[..., :norm_cols] - np.float32(0.5)) / np.float32(0.5)
    return v


def strip_entropy_reference(logits: np.ndarray, S: int) -> np.ndarray:
    """float64 [B] for logits [B * S][classes]: -nansum(p * log2(p)) / S over each background's S rows with
    p = sigmoid(logit) in fp64 (STRIP.py:76-78; a term with p == 0 or a NaN logit adds nothing)."""
    x = np.asarray(logits, dtype=np.float64)
    x = x.reshape(-1, S * x.shape[-1])
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        return -np.nansum(p * np.log2(p), axis=1) / S


def strip_draw_index(n_test: int, n_sample: int, n_data: int) -> np.ndarray:
    """int64 [n_test][n_sample]: the reference's draws, one np.random.randint(0, len(dataset), size=n_sample) per
    background from numpy's global generator (STRIP.py:69), backgrounds in order."""
    return np.stack([np.random.randint(0, n_data, size=n_sample) for _ in range(n_test)]).astype(np.int64)


def write_strip_result(path: str, trojan, benign) -> None:
    """The reference's result file (STRIP.py:237-250): the trojan entropies, a newline, the benign ones; space separated,
    no trailing newline, the first line empty in clean mode.  Values are written as Python floats."""
    with open(path, "w+") as f:
        f.write(" ".join("{}".format(float(v)) for v in trojan))
        f.write("\n")
        f.write(" ".join("{}".format(float(v)) for v in benign))


def strip_verdict(trojan, benign, detection_boundary: float) -> Tuple[float, bool, str]:
    """(min entropy, backdoored?, the two console lines of STRIP.py:252-259)."""
    min_entropy = min([float(v) for v in trojan] + [float(v) for v in benign])
    backdoored = min_entropy < detection_boundary
    text = "Min entropy trojan: {}, Detection boundary: {}\n".format(min_entropy, detection_boundary)
    text += "A backdoored model\n" if backdoored else "Not a backdoor model\n"
    return min_entropy, backdoored, text


@torch.no_grad()
def backdoor_backgrounds(netG, inputs: torch.Tensor, opt, sigma: Optional[float] = None) -> torch.Tensor:
    """uint8 NHWC device images of the backdoored `inputs` (float32 NCHW on the device), STRIP.py:167-173 in its order
    and in fp32: create_backdoor -> x * 0.5 + 0.5 (Denormalizer) -> * 255.0 -> clip to [0, 255] -> truncation to uint8
    -> NHWC."""
    bd = api.create_backdoor(netG, inputs, opt, sigma=sigma)
    bd = (bd * 0.5 + 0.5) * 255.0
    return torch.clamp(bd, 0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class Strip:
    """entropies() of background images under the classifier `netC` (a combat_amd.nets PreActResNet18 / ResNet18 in eval
    mode) with overlays taken from `dataset_u8`, the test set as uint8 [n][3][hw][hw] (combat_amd.data's layout) or
    [n][hw][hw][3]; it is uploaded once and stays on the device.  norm_cols: columns the normalisation reaches -- 3, the
    reference's arithmetic, unless given or opt.full_normalize is set (then hw, the whole image)."""

    # backgrounds per classifier pass, measured (tools/strip_time.py, DESIGN.md section 9: a clean CIFAR round of 100 x 100
    # takes 29.1 / 18.7 / 15.5 / 14.9 ms at G = 1 / 4 / 16 / 32 -- the classifier's own batch efficiency, flat beyond
    # 1600 images); group() lowers it where G * S images of the input size would exceed PIXELS (activation memory
    # grows with the slot)
    G = 16
    PIXELS = 1600 * 32 * 32

    def __init__(self, netC, dataset_u8, opt=None, norm_cols: Optional[int] = None):
        if netC.training:
            raise ValueError("Strip: the classifier must be in eval mode")
        self.netC, self.opt = netC, opt
        dev = netC.linear.weight.device
        data = torch.as_tensor(dataset_u8)
        if data.dtype != torch.uint8 or data.dim() != 4:
            raise ValueError("Strip: the dataset must be uint8 [n][3][hw][hw] or [n][hw][hw][3], got %s %s"
                             % (data.dtype, tuple(data.shape)))
        if data.shape[1] == 3 and data.shape[2] == data.shape[3]:
            data = data.permute(0, 2, 3, 1)                                   # NCHW -> NHWC, once
        if data.shape[3] != 3 or data.shape[1] != data.shape[2] or data.shape[1] not in (32, 64, 224):
            raise ValueError("Strip: images must be 32, 64 or 224 pixels square with 3 channels, got %s" % (tuple(data.shape),))
        if data.shape[0] < 1:
            raise ValueError("Strip: the dataset is empty")
        self.data = data.contiguous().to(dev)
        self.n_data, self.hw = int(data.shape[0]), int(data.shape[1])
        self.classes = netC.linear.out_features
        if norm_cols is None:
            norm_cols = self.hw if getattr(opt, "full_normalize", False) else 3
        if not 0 <= norm_cols <= self.hw:
            raise ValueError("Strip: norm_cols %d outside 0..%d" % (norm_cols, self.hw))
        self.norm_cols = int(norm_cols)

    def group(self, S: int) -> int:
        """Backgrounds per classifier pass for S overlays each."""
        return max(1, min(self.G, self.PIXELS // (S * self.hw * self.hw)))

    @torch.no_grad()
    def entropies(self, backgrounds_u8, index) -> torch.Tensor:
        """fp32 [B] on the device: the STRIP entropy of each background (uint8 [B][hw][hw][3], host or device) under the
        overlays dataset[index[b][s]] (integers [B][S] on the host: checked here, before the upload).  Nothing in here
        waits for the device; the caller's copy of the result does."""
        from .engine import pad_batch
        dev = self.data.device
        bg = torch.as_tensor(backgrounds_u8)
        if bg.dtype != torch.uint8 or bg.dim() != 4 or tuple(bg.shape[1:]) != (self.hw, self.hw, 3):
            raise ValueError("entropies: backgrounds must be uint8 [B][%d][%d][3], got %s %s"
                             % (self.hw, self.hw, bg.dtype, tuple(bg.shape)))
        idx = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index)
        if idx.ndim != 2 or idx.shape[0] != bg.shape[0] or idx.dtype.kind not in "iu":
            raise ValueError("entropies: index must be integers [B = %d][S], got %s %s" % (bg.shape[0], idx.dtype, idx.shape))
        B, S = idx.shape
        if S < 1:
            raise ValueError("entropies: every background needs at least one overlay")
        if B and (idx.min() < 0 or idx.max() >= self.n_data):
            raise ValueError("entropies: index outside the dataset's %d images" % self.n_data)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        if B == 0:
            return out
        if self.netC.training:
            raise ValueError("entropies: the classifier must be in eval mode")
        bg = bg.contiguous().to(dev)
        idx_dev = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
        eng = self.netC._net_engine()
        eng.refresh()
        G = self.group(S)
        for g0 in range(0, B, G):
            g = min(G, B - g0)
            slot = eng.slot("module.eval", pad_batch(g * S), self.hw)
            ops.strip_superimpose(bg[g0:g0 + g], self.data, idx_dev[g0:g0 + g], self.norm_cols, eng.input(slot))
            eng.forward_plan(slot, False).run()
            ops.strip_entropy(eng.head_bufs(slot)["logits"], g, S, out[g0:g0 + g])
        return out
