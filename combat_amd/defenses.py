"""Defenses evaluated against a trained backdoor.  Fine-pruning (reference defenses/fine_pruning/fine-pruning.py;
Liu et al., RAID 2018, without the fine-tuning half, as the reference: ":166 no-tuning after pruning a channel").

The reference forwards the test set once with a hook on ``layer4`` (:144-157), sorts the channels by mean activation
(:160-163) and then, for each of the C = 512 pruning levels, rebuilds ``layer4[1].conv2`` and ``linear`` without the
pruned channels (:168-211) and evaluates the whole test set, clean and backdoored (:213).  The pruned network's logits
are ``b + sum over kept c of W[:, c] . pooled[:, c]`` of the UNPRUNED network's pooled features,
so here the curve costs one clean pass, one backdoor pass and combat_prune_sweep per batch."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import api, ops


def require_single_process() -> None:
    """The defense scripts keep their counters on one GPU; under a multi-process launch every rank would write the same
    outfile from its own copy of the whole test set."""
    world = int(os.environ.get("WORLD_SIZE", 1))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        world = max(world, torch.distributed.get_world_size())
    if world > 1:
        raise RuntimeError("fine-pruning runs on a single GPU: started with world size %d (launch one process, "
                           "without torchrun)" % world)


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
