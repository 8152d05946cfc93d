"""ms/step and plan launches per step of AlternatedStep and MultiLabelStep in one process (CIFAR-10 shape, bench.py's
classifiers, detector and synthetic batches, bs 128; the multi-label step with nets.CUnetGeneratorv1), and the new
kernels' own times at that shape.

    python tools/multilabel_step_time.py [--steps 60] [--warmup 10] [--bs 128] [--only alternated|multilabel|kernels]

Sampled randomness (the steps draw their own num_bd, blur sigmas and augmentation tables).  "plan launches": the calls
recorded in the step's plans (a combat_cond_wgrad call is two kernel launches); the multi-label step's count includes
the Phase C generator forward ('Gc_f'), which runs only in steps with num_bd > 0.  Both steps issue the same direct
launches besides (copies, c8 conversion, trigger, augmentation, log terms, SGD)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from combat_amd import nets, ops, step as step_mod, trigger  # noqa: E402


def time_step(cls, args, device):
    opt = bench.Opt()
    np.random.seed(0)
    torch.manual_seed(100)
    netc, netg, clean, netf = bench.build_nets(device)
    if cls is step_mod.MultiLabelStep:
        torch.manual_seed(2)
        netg = nets.CUnetGeneratorv1(opt).to(device)
    st = cls(netc, netg, clean, netf, opt)
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
    assert np.isfinite(m["loss_ce_sum"]), m
    return ms, sum(len(p) for p in st.pl.values())


def time_kernels(args, device, reps=200):
    n, hw, nf, classes = args.bs, 32, 64, 10
    s = hw // 2
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(nf, 9, nf + classes, generator=g) * 0.05).to(device)
    y = torch.randint(0, classes, (n,), generator=g, dtype=torch.int32).to(device)
    cond = torch.empty(n, s, s, nf, dtype=torch.bfloat16, device=device)
    d = torch.randn(n, s, s, nf, generator=g).to(torch.bfloat16).to(device)
    dw, dwf, scratch = torch.empty_like(w), torch.randn(nf, 9, nf, generator=g).to(device), torch.empty(n * 9 * nf, device=device)
    x = (torch.rand(n, 3, hw, hw, generator=g) * 2 - 1).to(device)
    noise = torch.zeros(n, hw, hw, 8, dtype=torch.bfloat16, device=device)
    noise[..., :3] = torch.tanh(torch.randn(n, hw, hw, 3, generator=g)).to(torch.bfloat16).to(device)
    ps = step_mod.chunk_size(n, classes)
    groups = (n + ps - 1) // ps
    k1 = torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(0.1 + 0.09 * i, 3)) for i in range(groups)]).to(device)
    pm = trigger.lowpass_matrix(hw, 0.65).to(device)
    bd, mse = torch.empty_like(x), torch.empty(3 * n, device=device)
    dn, dout = torch.empty_like(noise), torch.randn(n, 3, hw, hw, generator=g).to(device)
    cases = (
        ("combat_cond_fwd", lambda: ops.cond_fwd(w, y, classes, cond)),
        ("combat_cond_wgrad (two launches, with the merge)", lambda: ops.cond_wgrad(d, y, classes, dw, scratch, dwf)),
        ("combat_trigger_groups_fwd", lambda: ops.trigger_groups_fwd(x, noise, pm, k1, ps, 0.08, bd, mse)),
        ("combat_trigger_fwd (one kernel)", lambda: ops.trigger_fwd(x, noise, pm, k1[0], 0.08, bd, mse_partial=mse)),
        ("combat_trigger_groups_bwd", lambda: ops.trigger_groups_bwd(x, noise, pm, k1, ps, 0.08, dout, bd, 1e-6, dn, pre_tanh=True)),
        ("combat_trigger_bwd (one kernel)", lambda: ops.trigger_bwd(x, noise, pm, k1[0], 0.08, dout, bd, 1e-6, dn, pre_tanh=True)),
    )
    for name, fn in cases:
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print("%-52s %7.2f us per call, back to back (n = %d)" % (name, e0.elapsed_time(e1) / reps * 1e3, n), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--only", choices=("alternated", "multilabel", "kernels"), default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    classes = {"alternated": step_mod.AlternatedStep, "multilabel": step_mod.MultiLabelStep}
    for name, cls in classes.items():
        if args.only in (None, name):
            ms, launches = time_step(cls, args, device)
            print("%-16s %.3f ms/step  %d plan launches per step" % (cls.__name__, ms, launches), flush=True)
    if args.only in (None, "kernels"):
        time_kernels(args, device)


if __name__ == "__main__":
    main()
