"""Time the STRIP defense on CIFAR-shaped data: one round (n_test backgrounds x n_sample overlays; attack mode scores
n_test backdoored backgrounds, made by the generator, and then n_test clean ones) through Strip.entropies for several
group sizes G, against the slow path on the same classifier -- the reference's structure (STRIP.py:66-78): every blend
built on the host (saturating add, / 255, the three-column normalisation), stacked and uploaded, netC(x) once per
background, sigmoid and entropy on the host -- and combat_strip_superimpose alone against its byte count.

    python tools/strip_time.py [--n_test 100] [--n_sample 100] [--groups 1,4,16,32] [--repeats 5] [--slow_repeats 2]

Prints one JSON line.  Round figures are medians of wall-clock times that end in the copy of the result to the host;
the fast and the slow path alternate within one session (fast, slow, fast, slow, ...) after one untimed run of each.
The kernel figure is the median of device-event times around --kernel_reps back-to-back launches."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Opt:
    noise_rate, ratio, kernel_size, sigma = 0.08, 0.65, 3, (0.1, 1.0)


def slow_entropies(netC, backgrounds, data, index, blend):
    """The reference's _get_entropy per background with host blends; float list."""
    out = []
    for b in range(len(index)):
        x = torch.from_numpy(np.stack([blend(backgrounds[b], data[i], 3) for i in index[b]]))
        p = torch.sigmoid(netC(x.cuda())).cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(float(-np.nansum(p * np.log2(p)) / index.shape[1]))
    return out


def median_ms(samples):
    return round(statistics.median(samples) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_test", type=int, default=100)
    ap.add_argument("--n_sample", type=int, default=100)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--groups", type=str, default="1,4,16,32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow_repeats", type=int, default=2)
    ap.add_argument("--kernel_reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/strip_time.py measures on the GPU; none found")
    from combat_amd import defenses, nets, ops

    torch.manual_seed(0)
    netC = nets.PreActResNet18().cuda().eval().requires_grad_(False)
    netG = nets.UnetGenerator(None).cuda().eval().requires_grad_(False)
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, (a.images, 32, 32, 3), dtype=np.uint8)
    clean = data[:a.n_test]
    floats = torch.from_numpy(((clean.transpose(0, 3, 1, 2).astype(np.float32) / 255) - 0.5) / 0.5).cuda()
    index = np.stack([rng.integers(0, a.images, a.n_sample) for _ in range(2 * a.n_test)])
    groups = [int(g) for g in a.groups.split(",")]

    def detector(g):
        return type("Strip%d" % g, (defenses.Strip,), {"G": g, "PIXELS": 1 << 40})(netC, data)   # G as asked, uncapped

    dets = {g: detector(g) for g in groups}

    def fast_round(det, attack):
        res = []
        if attack:
            bg = defenses.backdoor_backgrounds(netG, floats, Opt, sigma=0.5)
            res.append(det.entropies(bg, index[:a.n_test]).cpu())
        res.append(det.entropies(det.data[:a.n_test], index[a.n_test:]).cpu())
        return res

    def slow_round(attack):
        res = []
        if attack:
            bg = defenses.backdoor_backgrounds(netG, floats, Opt, sigma=0.5).cpu().numpy()
            res.append(slow_entropies(netC, bg, data, index[:a.n_test], defenses.strip_blend_reference))
        res.append(slow_entropies(netC, clean, data, index[a.n_test:], defenses.strip_blend_reference))
        return res

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    out = {"device": torch.cuda.get_device_name(0), "n_test": a.n_test, "n_sample": a.n_sample, "images": a.images,
           "repeats": a.repeats, "slow_repeats": a.slow_repeats}
    for attack in (False, True):
        mode = "attack" if attack else "clean"
        fast = {g: [] for g in groups}
        slow = []
        for g in groups:                                   # untimed: plans, slots, code objects
            fast_round(dets[g], attack)
        _, slow_vals = clock(lambda: slow_round(attack))
        _, fast_vals = clock(lambda: fast_round(dets[groups[-1]], attack))
        worst = max(float(np.abs(np.asarray(s) - f.numpy()).max()) for s, f in zip(slow_vals, fast_vals))
        out["%s_fast_vs_slow_max_abs" % mode] = worst
        for r in range(a.repeats):
            for g in groups:
                fast[g].append(clock(lambda: fast_round(dets[g], attack))[0])
            if r < a.slow_repeats:
                slow.append(clock(lambda: slow_round(attack))[0])
        for g in groups:
            out["%s_round_ms_G%d" % (mode, g)] = median_ms(fast[g])
            out["%s_round_ms_G%d_minmax" % (mode, g)] = [round(min(fast[g]) * 1e3, 3), round(max(fast[g]) * 1e3, 3)]
        out["%s_round_slow_ms" % mode] = median_ms(slow)
        out["%s_round_slow_ms_minmax" % mode] = [round(min(slow) * 1e3, 1), round(max(slow) * 1e3, 1)]

    # the classifier pass alone at the slot sizes the groups use, and the superimpose kernel alone (into a buffer of its
    # own, so that the whole round's 10 000 images can be timed without a classifier slot of that size)
    from combat_amd.engine import pad_batch
    eng = netC._net_engine()
    det = dets[groups[-1]]
    idx_dev = torch.from_numpy(index[:a.n_test].astype(np.int32)).cuda()
    for g in groups:
        slot = eng.slot("module.eval", pad_batch(g * a.n_sample), 32)
        plan = eng.forward_plan(slot, False)
        plan.run()
        out["classifier_pass_ms_%d_images" % (g * a.n_sample)] = median_ms([clock(plan.run)[0] for _ in range(a.repeats)])
    for g in sorted(set(groups + [a.n_test])):
        n = g * a.n_sample
        buf = torch.empty(n, 32, 32, 8, dtype=torch.bfloat16, device="cuda")
        bgs = det.data[:g]
        ops.strip_superimpose(bgs, det.data, idx_dev[:g], 3, buf)
        ev = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_reps):
                ops.strip_superimpose(bgs, det.data, idx_dev[:g], 3, buf)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1) / a.kernel_reps)
        us = statistics.median(ev) * 1e3
        nbytes = n * 32 * 32 * (16 + 3 + 3) + n * 4           # written c8 pixels, the two uint8 sources as addressed, the table
        out["superimpose_us_%d_images" % n] = round(us, 2)
        out["superimpose_GBps_%d_images" % n] = round(nbytes / us / 1e3, 1)
        out["superimpose_bytes_%d_images" % n] = nbytes
    print(json.dumps(out))


if __name__ == "__main__":
    with torch.no_grad():
        main()
