"""Generate tests/golden/vgg13.npz and tests/golden/vgg13_keys.json from the reference's own VGG module.

Run in the build container only (``python tests/golden/make_golden_vgg13.py``), like make_golden.py: it imports
``/root/reference`` (read-only), which does not exist on the GPU box.  The files it writes are committed; tests read only
those.

Parameters and images are never stored: the fixture records seeds (tests/vgg13_ref.py holds them and rebuilds the same
batches), and the tests rebuild identical parameters by constructing combat_amd's mirror module under the same seed.
Recorded per case (c32: 32 x 32, 10 classes; c64: 64 x 64, 8 classes; 16 images each):
  train/   logits, loss, parameter gradients (make_golden.summarize: sum, L2, sampled entries), BatchNorm buffers after
           the forward, of a train-mode pass on batch 0
  eval/    logits of an eval-mode pass on batch 1 with randomize_bn_buffers' running statistics
  trace    the losses of 10 steps of torch.optim.SGD(lr 1e-2, momentum 0.9, wd 5e-4, nesterov) alternating over batches 2 and 3, train mode,
           no augmentation, no poisoning
and in the JSON the state-dict keys with shapes and the sha256 of the seeded initial parameters."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))

from classifier_models.vgg import VGG  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import save, summarize  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import vgg13_ref as R  # noqa: E402


def make(case):
    c = R.CASES[case]
    torch.manual_seed(R.SEED_NET)
    return VGG("VGG13", num_classes=c["classes"], n_input=3, input_size=c["hw"])


def golden_vgg13():
    out = {"seeds": np.array([R.SEED_NET, R.SEED_BN] + [R.SEEDS[k] for k in sorted(R.SEEDS)])}
    keys = {}
    for case in sorted(R.CASES):
        net = make(case)
        keys[case] = {"keys": [[k, list(v.shape)] for k, v in net.state_dict().items()], "sha256": R.checksum(net.state_dict())}
        names = [k for k, _ in net.named_parameters()]
        x, t = R.batch(case, 0)
        out[case + "/train/t"], out[case + "/train/x_sum"] = t.numpy(), np.float64(x.double().sum())
        net.train()
        logits = net(x)
        loss = F.cross_entropy(logits, t)
        grads = torch.autograd.grad(loss, list(net.parameters()))
        out[case + "/train/logits"], out[case + "/train/loss"] = logits.detach().numpy(), np.float64(loss.detach())
        summarize(zip(names, grads), out, case + "/train/gp")
        for k, v in net.state_dict().items():
            if "running" in k or "num_batches" in k:
                out["%s/train/buf/%s" % (case, k)] = v.numpy().copy()
        net = R.randomize_bn_buffers(make(case), R.SEED_BN).eval()
        x, t = R.batch(case, 1)
        with torch.no_grad():
            out[case + "/eval/logits"] = net(x).numpy()
        out[case + "/eval/t"] = t.numpy()
        net = make(case).train()
        opt = torch.optim.SGD(net.parameters(), nesterov=True, **R.SGD)
        trace = []
        for s in range(R.TRACE_STEPS):
            x, t = R.batch(case, 2 + s % R.TRACE_POOL)
            opt.zero_grad()
            loss = F.cross_entropy(net(x), t)
            loss.backward()
            opt.step()
            trace.append(float(loss))
        out[case + "/trace"] = np.array(trace)
        print(case, "train loss %.4f, trace %s" % (float(out[case + "/train/loss"]), np.round(trace, 3).tolist()), flush=True)
    save("vgg13.npz", out)
    with open(os.path.join(HERE, "vgg13_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
    print("wrote vgg13_keys.json")


if __name__ == "__main__":
    torch.set_num_threads(8)
    golden_vgg13()
