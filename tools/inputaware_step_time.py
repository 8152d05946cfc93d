"""ms/step of AlternatedStep and InputAwareStep in one process (CIFAR-10 shape, bench.py's networks and synthetic
batches, bs 128), in default and in deterministic mode, and the ratio of the two.

    python tools/inputaware_step_time.py [--steps 60] [--warmup 10] [--bs 128] [--only alternated|inputaware]

--only times one step class in default mode (for a kernel trace of that step alone:
rocprofv3 --kernel-trace --stats -- python tools/inputaware_step_time.py --only inputaware).

The input-aware step's second batch is the next batch of the same synthetic pool.  Sampled randomness (the steps
draw their own num_bd, blur sigmas and augmentation tables)."""
import argparse
import os
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
    opt.cross_weight = 0.2
    np.random.seed(0)
    torch.manual_seed(100)
    st = cls(*bench.build_nets(device), opt)
    batches = bench.synth_batches(8, args.bs, 0, device)
    if cls is step_mod.InputAwareStep:
        run = lambda i: st.run(*batches[i % 8], batches[(i + 1) % 8][0])
    else:
        run = lambda i: st.run(*batches[i % 8])
    for i in range(args.warmup):
        run(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        run(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    m = st.read_metrics()
    assert np.isfinite(m["loss_ce_sum"]), m
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--only", choices=("alternated", "inputaware"), default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    prev = engine.deterministic()
    if args.only:
        cls = step_mod.AlternatedStep if args.only == "alternated" else step_mod.InputAwareStep
        print("%s %.3f ms/step" % (cls.__name__, time_step(cls, False, args, device)), flush=True)
        engine.set_deterministic(prev)
        return
    try:
        for det in (False, True):
            a = time_step(step_mod.AlternatedStep, det, args, device)
            b = time_step(step_mod.InputAwareStep, det, args, device)
            print("%-13s AlternatedStep %.3f ms/step  InputAwareStep %.3f ms/step  ratio %.3f"
                  % ("deterministic" if det else "default", a, b, b / a), flush=True)
    finally:
        engine.set_deterministic(prev)


if __name__ == "__main__":
    main()
