"""ms/step of AlternatedStep and ImperceptibleStep in one process (CIFAR-10 shape, bench.py's networks and synthetic
batches, bs 128), in default and in deterministic mode, and the ratio of the two.

    python tools/imperceptible_step_time.py [--steps 60] [--warmup 10] [--bs 128] [--reps 3] [--only alternated|imperceptible]

The pair is timed --reps times in alternating order (A B A B ...) and the median per class is reported beside the
single runs, so that a drift of the box between the two classes shows.  --only times one step class once in default
mode (for a kernel trace of that step alone:
rocprofv3 --kernel-trace --stats -- python tools/imperceptible_step_time.py --only imperceptible).

tv_weight is config.py's default (0.01).  Sampled randomness (the steps draw their own num_bd, blur sigmas and
augmentation tables)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from combat_amd import engine, step as step_mod  # noqa: E402


def time_step(cls, deterministic, args, device):
    engine.set_deterministic(deterministic)
    opt = bench.Opt()
    opt.tv_weight = 0.01
    np.random.seed(0)
    torch.manual_seed(100)
    st = cls(*bench.build_nets(device), opt)
    batches = bench.synth_batches(8, args.bs, 0, device)
    for i in range(args.warmup):
        st.run(*batches[i % 8])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        st.run(*batches[i % 8])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    m = st.read_metrics()
    assert np.isfinite(m["loss_ce_sum"]) and np.isfinite(m.get("loss_tv_sum", 0.0)), m
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=("alternated", "imperceptible"), default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    prev = engine.deterministic()
    if args.only:
        cls = step_mod.AlternatedStep if args.only == "alternated" else step_mod.ImperceptibleStep
        print("%s %.3f ms/step" % (cls.__name__, time_step(cls, False, args, device)), flush=True)
        engine.set_deterministic(prev)
        return
    try:
        for det in (False, True):
            a, b = [], []
            for _ in range(args.reps):
                a.append(time_step(step_mod.AlternatedStep, det, args, device))
                b.append(time_step(step_mod.ImperceptibleStep, det, args, device))
            ma, mb = statistics.median(a), statistics.median(b)
            print("%-13s AlternatedStep %.3f ms/step (%s)  ImperceptibleStep %.3f ms/step (%s)  ratio %.3f"
                  % ("deterministic" if det else "default", ma, " ".join("%.3f" % v for v in a), mb,
                     " ".join("%.3f" % v for v in b), mb / ma), flush=True)
    finally:
        engine.set_deterministic(prev)


if __name__ == "__main__":
    main()
