"""Time the Neural Cleanse optimisation on CIFAR-shaped data: one label-epoch (10 000 images at batch size 64 = 157 steps,
the last of 16 images) through NeuralCleanse.run_epoch -- one replayed plan per step, the permutation uploaded before and
the statistics rows read after -- against the same loop written with stock PyTorch-ROCm autograd on the same GPU: a plain
torch PreActResNet18 with the same weights in eval mode, the blend, cross entropy + cost * L1, backward, torch.optim.Adam
(betas 0.5 / 0.9) and the per-batch records of the reference's train_step (detecting.py:182-205), its test set already on
the device as normalised fp32 (the reference's loader works on the host: this baseline is faster than the reference).
The baseline is never the code under test.

    python tools/neural_cleanse_time.py [--images 10000] [--bs 64] [--repeats 3]

Prints one JSON line.  Epoch figures are medians of wall-clock times that end with the statistics on the host; the two
paths alternate within one session (ours, baseline, ours, ...) after one untimed epoch of each.  ms per step is the
epoch time over its number of steps."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class PreActBlock(nn.Module):
    def __init__(self, in_planes, planes, stride):
        super().__init__()
        self.bn1, self.conv1 = nn.BatchNorm2d(in_planes), nn.Conv2d(in_planes, planes, 3, stride, 1, bias=False)
        self.bn2, self.conv2 = nn.BatchNorm2d(planes), nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        if stride != 1 or in_planes != planes:
            self.shortcut = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride, bias=False))

    def forward(self, x):
        out = F.relu(self.bn1(x))
        shortcut = self.shortcut(out) if hasattr(self, "shortcut") else x
        out = self.conv1(out)
        return self.conv2(F.relu(self.bn2(out))) + shortcut


class TorchPreActResNet18(nn.Module):
    """PreActResNet18 in stock torch modules, state_dict-compatible with combat_amd.nets.PreActResNet18."""

    def __init__(self, num_classes=10):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 3, 1, 1, bias=False)
        planes, layers = 64, []
        for out, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):
            layers.append(nn.Sequential(PreActBlock(planes, out, stride), PreActBlock(out, out, 1)))
            planes = out
        self.layer1, self.layer2, self.layer3, self.layer4 = layers
        self.linear = nn.Linear(512, num_classes)

    def forward(self, x):
        out = self.layer4(self.layer3(self.layer2(self.layer1(self.conv1(x)))))
        return self.linear(F.avg_pool2d(out, 4).flatten(1))


class TorchCleanse:
    """The reference's RegressionModel + train_step loop on device tensors."""

    def __init__(self, net, data_u8, bs, lr, epsilon, mean, std):
        self.net, self.bs, self.eps = net, bs, epsilon
        x = torch.from_numpy(data_u8).cuda().permute(0, 3, 1, 2).float()
        self.x = ((x / 255 - 0.5) / 0.5).contiguous()
        hw = self.x.shape[-1]
        self.mask_tanh = nn.Parameter(torch.ones(1, hw, hw, device="cuda"))
        self.pattern_tanh = nn.Parameter(torch.ones(3, hw, hw, device="cuda"))
        self.optim = torch.optim.Adam([self.mask_tanh, self.pattern_tanh], lr=lr, betas=(0.5, 0.9))
        self.shift, self.scale = torch.zeros(1, hw, 1, device="cuda"), torch.ones(1, hw, 1, device="cuda")
        for row in range(3):                                             # the reference normalises rows 0..2
            self.shift[0, row, 0], self.scale[0, row, 0] = mean[row], std[row]

    def raw(self, t):
        return torch.tanh(t) / (2 + self.eps) + 0.5

    def epoch(self, target, order, cost):
        order = order.cuda()
        ce_list, reg_list, acc_list = [], [], []
        for s in range(0, len(order), self.bs):
            self.optim.zero_grad()
            x = self.x[order[s:s + self.bs]]
            labels = torch.full((x.shape[0],), target, dtype=torch.int64, device="cuda")
            mask = self.raw(self.mask_tanh)
            pattern = (self.raw(self.pattern_tanh) - self.shift) / self.scale
            pred = self.net((1 - mask) * x + mask * pattern)
            loss_ce = F.cross_entropy(pred, labels)
            loss_reg = torch.norm(self.raw(self.mask_tanh), 1)
            (loss_ce + cost * loss_reg).backward()
            self.optim.step()
            ce_list.append(loss_ce.detach())
            reg_list.append(loss_reg.detach())
            acc_list.append(torch.sum(torch.argmax(pred, dim=1) == labels).detach() * 100.0 / x.shape[0])
        return torch.stack([torch.stack(ce_list), torch.stack(reg_list), torch.stack(acc_list)]).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--target", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/neural_cleanse_time.py measures on the GPU; none found")
    from combat_amd import defenses, nets

    torch.manual_seed(0)
    netC = nets.PreActResNet18().cuda().eval().requires_grad_(False)
    plain = TorchPreActResNet18().cuda()
    plain.load_state_dict(netC.state_dict())
    plain.eval().requires_grad_(False)
    data = np.random.default_rng(1).integers(0, 256, (a.images, 32, 32, 3), dtype=np.uint8)
    opt = types.SimpleNamespace(bs=a.bs, lr=0.1, EPSILON=1e-7, epoch=1, init_cost=1e-3)
    ours = defenses.NeuralCleanse(netC, data, opt)
    ours.reset(np.ones((1, 32, 32), np.float32), np.ones((3, 32, 32), np.float32))
    base = TorchCleanse(plain, data, a.bs, 0.1, 1e-7, defenses.NC_MEAN, defenses.NC_STD)
    gen = torch.Generator().manual_seed(2)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    order = torch.randperm(a.images, generator=gen)
    _, s_ours = clock(lambda: ours.run_epoch(a.target, order, 1e-3))    # untimed: plans, slots, code objects, autotuning
    _, s_base = clock(lambda: base.epoch(a.target, order, 1e-3))
    t_ours, t_base = [], []
    for _ in range(a.repeats):
        order = torch.randperm(a.images, generator=gen)
        t_ours.append(clock(lambda: ours.run_epoch(a.target, order, 1e-3))[0])
        t_base.append(clock(lambda: base.epoch(a.target, order, 1e-3))[0])
    steps = ours.steps
    med = lambda v: statistics.median(v) * 1e3
    out = {"device": torch.cuda.get_device_name(0), "images": a.images, "bs": a.bs, "steps": steps, "repeats": a.repeats,
           "epoch_ms": round(med(t_ours), 2), "epoch_ms_minmax": [round(min(t_ours) * 1e3, 2), round(max(t_ours) * 1e3, 2)],
           "step_ms": round(med(t_ours) / steps, 4),
           "torch_epoch_ms": round(med(t_base), 2),
           "torch_epoch_ms_minmax": [round(min(t_base) * 1e3, 2), round(max(t_base) * 1e3, 2)],
           "torch_step_ms": round(med(t_base) / steps, 4),
           "speedup": round(med(t_base) / med(t_ours), 3),
           # the first epoch of both, same order, same start: bf16 engine against fp32 autograd
           "first_epoch_loss_ce_ours_vs_torch": [float(s_ours[:, 0].mean()), float(s_base[0].mean())],
           "first_epoch_loss_reg_ours_vs_torch": [float(s_ours[:, 2].mean()), float(s_base[1].mean())]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
