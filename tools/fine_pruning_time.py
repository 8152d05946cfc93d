"""Time the fine-pruning defense on CIFAR-shaped data: pass 1 (one eval forward of the classifier per batch + the
activation sums), the two sweeps per batch (combat_prune_sweep on the clean and the backdoored pooled features), and one
pass of the repository's eval.py loop -- the unit the reference's script pays 512 times (fine-pruning.py:168-213).

    python tools/fine_pruning_time.py [--images 10000] [--bs 100] [--repeats 5]

Prints one JSON line; every figure is the median over --repeats timed runs after one untimed run, wall clock around a
device synchronisation.  The 512 x eval figure is an extrapolation from one measured pass, reported as such."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--bs", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    from combat_amd import api, nets
    from combat_amd.defenses import FinePruning
    from combat_amd.dist import NullWriter
    spec = importlib.util.spec_from_file_location("eval_script", os.path.join(ROOT, "eval.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)

    class Opt:
        noise_rate, ratio, kernel_size, sigma = 0.08, 0.65, 3, (0.1, 1.0)
        target_label, attack_mode, num_classes, device = 0, "all2one", 10, "cuda"

    torch.manual_seed(0)
    netC = nets.PreActResNet18().cuda().eval()
    netG = nets.UnetGenerator(None).cuda().eval()
    g = torch.Generator().manual_seed(1)
    batches = []
    for i in range(0, a.images, a.bs):
        n = min(a.bs, a.images - i)
        x = ((torch.randint(0, 256, (n, 3, 32, 32), generator=g).float() / 255) - 0.5) / 0.5
        batches.append((x.cuda(), torch.randint(0, 10, (n,), generator=g).cuda()))
    fp = FinePruning(netC, Opt)

    def pass1():
        for x, _ in batches:
            fp.observe(x)

    t_pass1 = timed(pass1, a.repeats)
    with torch.no_grad():
        pooled = [(api.pooled_features(netC, x), api.pooled_features(netC, api.create_backdoor(netG, x, Opt)))
                  for x, _ in batches]
    bd = [torch.zeros_like(t) for _, t in batches]
    fp.order()

    def sweeps():
        for (pc, pb), (_, t), tb in zip(pooled, batches, bd):
            fp.sweep(pc, t)
            fp.sweep(pb, tb, targets2=t, backdoor=True)

    t_sweeps = timed(sweeps, a.repeats)

    def one_sweep():
        fp.sweep(pooled[0][0], batches[0][1])

    t_one = timed(one_sweep, a.repeats * 4)

    def pass2():
        with torch.no_grad():
            for x, t in batches:
                fp.sweep(api.pooled_features(netC, x), t)
                fp.sweep(api.pooled_features(netC, api.create_backdoor(netG, x, Opt)), torch.zeros_like(t), targets2=t,
                         backdoor=True)

    t_pass2 = timed(pass2, a.repeats)
    stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        t_eval = timed(lambda: ev.eval(netC, netG, batches, NullWriter(), Opt), max(2, a.repeats // 2))
    finally:
        sys.stdout = stdout
    print(json.dumps({
        "images": a.images, "bs": a.bs, "device": torch.cuda.get_device_name(0),
        "pass1_ms": round(t_pass1, 2), "two_sweeps_all_batches_ms": round(t_sweeps, 2),
        "one_sweep_call_ms": round(t_one, 4), "pass2_ms": round(t_pass2, 2),
        "sweeps_over_pass1": round(t_sweeps / t_pass1, 4), "eval_loop_ms": round(t_eval, 2),
        "curve_ms": round(t_pass1 + t_pass2, 2),
        "eval_x512_over_curve": round(512 * t_eval / (t_pass1 + t_pass2), 1)}))


if __name__ == "__main__":
    main()
