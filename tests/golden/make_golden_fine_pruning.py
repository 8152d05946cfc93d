"""Generate tests/golden/fine_pruning.npz and tests/golden/fine_pruning_flags.json from the reference's own modules.

Run in the build container only (``python tests/golden/make_golden_fine_pruning.py``), like make_golden.py: it imports
``/root/reference`` (read-only), which does not exist on the GPU box.  The files it writes are committed; tests read
only those.

The reference's defenses/fine_pruning/fine-pruning.py is not importable (torchvision is absent), so the pruning loop of
its :168-190 is written out here over the reference's PreActResNet18: for every level a copy of the network gets a
``layer4[1].conv2`` with the surviving output channels only, the block's ``ind`` mask for the residual
(preact_resnet.py:36-37) and a ``linear`` over the surviving columns.  The generator plays no part in what is pinned
here (the pruned CLASSIFIER against the one-pass sweep), so it is left out.

Parameters are never stored: the fixture records the seeds, and the tests rebuild identical parameters by constructing
combat_amd's mirror module under the same seed and applying make_golden.randomize_bn_buffers' calls."""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.modules.setdefault("torchvision", types.ModuleType("torchvision"))

from classifier_models.preact_resnet import PreActResNet18  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import randomize_bn_buffers, synth_images  # noqa: E402

SEED_NET, SEED_BN, SEED_IMG, N_IMG = 0, 500, 8800, 32
LOGIT_LEVELS = (0, 1, 2, 255, 256, 510, 511)


def pruned_copy(net, keep):
    """The network of fine-pruning.py:169-190 for the boolean channel mask `keep` (True = survives)."""
    pruned = copy.deepcopy(net)
    n_keep = int(keep.sum())
    blk = pruned.layer4[1]
    conv = torch.nn.Conv2d(keep.numel(), n_keep, (3, 3), stride=1, padding=1, bias=False)
    conv.weight.data = net.layer4[1].conv2.weight.data[keep]
    blk.conv2 = conv
    blk.ind = keep
    lin = torch.nn.Linear(n_keep, net.linear.out_features)
    lin.weight.data = net.linear.weight.data[:, keep]
    lin.bias.data = net.linear.bias.data
    pruned.linear = lin
    return pruned.eval()


def excluded_pairs(pooled, weight, bias, order):
    """(image, level) pairs whose fp64 top-two margin is below the fp32 summation bound 2 * in * 2^-24 * sum|terms|
    (every logit is a sum of at most in + 1 terms; a difference of two logits carries twice one logit's bound),
    and the fp64 logits [C][n][classes] -- the same restatement the tests make."""
    p, w = pooled.astype(np.float64), weight.astype(np.float64)
    c = len(order)
    s = np.broadcast_to(bias.astype(np.float64), (p.shape[0], w.shape[0])).copy()
    a = np.broadcast_to(np.abs(bias.astype(np.float64)), s.shape).copy()
    logits = np.empty((c,) + s.shape)
    excl = np.zeros((c, p.shape[0]), dtype=bool)
    for k in range(c - 1, -1, -1):
        t = p[:, order[k]:order[k] + 1] * w[None, :, order[k]]
        s, a = s + t, a + np.abs(t)
        logits[k] = s
        top = np.sort(s, axis=1)
        excl[k] = (top[:, -1] - top[:, -2]) < 2 * c * 2.0 ** -24 * a.max(axis=1)
    return excl, logits


def golden_fine_pruning():
    torch.manual_seed(SEED_NET)
    net = randomize_bn_buffers(PreActResNet18(), SEED_BN).eval()
    x = synth_images(N_IMG, 32, SEED_IMG)
    out = {"seeds": np.array([SEED_NET, SEED_BN, SEED_IMG]), "n_images": np.int64(N_IMG)}
    taken = []
    hook = net.layer4.register_forward_hook(lambda module, inputs, output: taken.append(output))
    with torch.no_grad():
        net(x)
        hook.remove()
        feat = taken[0]
        activation = torch.mean(feat, dim=[0, 2, 3])                       # fine-pruning.py:161
        seq_sort = torch.argsort(activation)                               # :162
        pooled = net.avgpool(feat).view(N_IMG, -1)
        c = seq_sort.shape[0]
        keep = torch.ones(c, dtype=bool)
        preds = np.empty((c, N_IMG), dtype=np.int8)
        for index in range(c):                                             # :168-173: level `index` has index channels pruned
            if index:
                keep[seq_sort[index - 1]] = False
            logits = pruned_copy(net, keep)(x)
            preds[index] = torch.argmax(logits, 1).numpy()
            if index in LOGIT_LEVELS:
                out["logits/%d" % index] = logits.numpy()
            if index % 64 == 0:
                print("  level %d" % index, flush=True)
    out["activation"], out["seq_sort"] = activation.numpy(), seq_sort.numpy().astype(np.int64)
    out["pred"], out["pooled"] = preds, pooled.numpy()
    out["logit_levels"] = np.array(LOGIT_LEVELS)
    excl, logits64 = excluded_pairs(out["pooled"], net.linear.weight.detach().numpy(), net.linear.bias.detach().numpy(),
                                     out["seq_sort"])
    wrong = (logits64.argmax(2) != preds) & ~excl
    out["n_excluded"] = np.int64(excl.sum())
    print("excluded %d of %d pairs (%.3f %%), mismatches outside them: %d; distinct predictions %s" % (
        excl.sum(), excl.size, 100.0 * excl.mean(), wrong.sum(), np.unique(preds).tolist()))
    assert excl.mean() <= 0.01 and not wrong.any(), "pick other seeds"
    path = os.path.join(HERE, "fine_pruning.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def golden_flags():
    """Flag names, defaults and types of the reference parser (defenses/fine_pruning/config.py:4-42)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_fp_config", os.path.join(REF, "defenses/fine_pruning/config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    flags = {}
    for a in mod.get_arguments()._actions:
        if a.dest == "help":
            continue
        d = a.default
        flags[a.dest] = {"default": list(d) if isinstance(d, (list, tuple)) else d,
                         "type": getattr(a.type, "__name__", None), "choices": a.choices, "store_true": a.nargs == 0}
    with open(os.path.join(HERE, "fine_pruning_flags.json"), "w") as f:
        json.dump(flags, f, indent=1, sort_keys=True)
    print("wrote fine_pruning_flags.json (%d flags)" % len(flags))


if __name__ == "__main__":
    torch.set_num_threads(8)
    golden_flags()
    golden_fine_pruning()
