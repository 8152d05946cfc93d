"""Worker of tests/test_entrypoints_gpu.py::test_data_parallel_attack_steps_two_ranks_one_gpu (not a test module).

Launched like tests/dp_rehearsal.py (two ranks on the one GPU, exchange over gloo), for the two step classes whose
all-reduce that worker does not reach:
  InputAwareStep      two half-batch generator backward plans into one flat buffer, the cross half set aside in
                      `_g_cross` and added back, then ONE synchronous all-reduce of the whole buffer;
  ImperceptibleStep   the bucketed all-reduce at the plan's marks, with a TV term scaled by the rank-local batch size.
Per class, b = 16 images per rank, every rank with its own images, second batch, labels and draws (six / five
augmentation tables with crop, rotation and flip active):
  1. the reduced generator gradient against the sum of the ranks' single-process gradients at lr_c = 0.0, and the
     optimiser applying their mean (dp_rehearsal.gen_grad_check);
  2. at the default lr_c: netC's reduced gradient of step 1 against the sum of the singles, its update against the mean;
  3. a second step with num_bd = 1 on rank 0 and 0 on rank 1 (rank 1 skips Phase C's trigger launch and still takes
     part in every exchange): parameters and momentum of both networks bit-identical across ranks, metrics finite,
     the class's own loss sum (cross / TV) positive.
Every rank writes OUT/rank<r>.json."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dp_rehearsal import Opt, aug_table, build, gather, gen_grad_check, rel  # noqa: E402


class IAOpt(Opt):
    cross_weight = 0.2          # tests/test_inputaware_gpu.py::IAOpt


class TVOpt(Opt):               # tests/test_imperceptible_gpu.py: the fixture's weight
    tv_weight = float(np.load(os.path.join(ROOT, "tests", "golden", "imperceptible_step.npz"))["tv_weight"])


def main():
    out_dir = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    from combat_amd import engine, nets, step as step_mod
    b = 16
    gen = torch.Generator().manual_seed(1700 + rank)         # every rank its own shard, second batch and labels
    image = lambda: ((torch.randint(0, 256, (b, 3, 32, 32), generator=gen, dtype=torch.uint8).float() / 255) - 0.5) / 0.5
    x, x2 = image().cuda(), image().cuda()
    t = torch.randint(0, 10, (b,), generator=gen)
    t[:3] = 0
    rng = np.random.default_rng(4100 + rank)
    tables = lambda k: [aug_table(b, rng) for _ in range(k)]
    # step 1: own poison count and sigmas; step 2: one poisoned image on rank 0, none on rank 1
    draws = dict(
        inputaware=[step_mod.InputAwareRandomness(2 + rank, 0.4 + 0.1 * rank, 0.7 - 0.2 * rank, tables(6), sigma_x=0.3 + 0.4 * rank),
                    step_mod.InputAwareRandomness(1 - rank, 0.6 if rank == 0 else 0.5, 0.5 + 0.2 * rank, tables(6),
                                                  sigma_x=0.8 - 0.3 * rank)],
        imperceptible=[step_mod.StepRandomness(2 + rank, 0.4 + 0.1 * rank, 0.7 - 0.2 * rank, tables(5)),
                       step_mod.StepRandomness(1 - rank, 0.6 if rank == 0 else 0.5, 0.5 + 0.2 * rank, tables(5))])
    res = {"deterministic": engine.deterministic()}

    def gather_equal(buf):
        got = gather(buf, world)
        return bool(torch.equal(got[0], got[1]))

    for tag, cls, opt, own_sum, lr_g in (("inputaware", step_mod.InputAwareStep, IAOpt(), "loss_cross_sum", Opt.lr_C * 0.1),
                                         ("imperceptible", step_mod.ImperceptibleStep, TVOpt(), "loss_tv_sum", Opt.lr_G)):
        def make(pg):
            netc, netg, clean, netf = build(nets)
            return cls(netc, netg, clean, netf, opt, process_group=pg)

        def run(st, lr_c, i=0):
            if cls is step_mod.InputAwareStep:
                st.run(x, t, x2, draws[tag][i], lr_c=lr_c)
            else:
                st.run(x, t, draws[tag][i], lr_c=lr_c)

        # ---- 1. the reduced generator gradient (single-process runs and the data-parallel one at lr_c = 0.0)
        gc_single = gen_grad_check(res, tag, make, run, world, lr_g)

        # ---- 2. the default lr_c: netC's reduced gradient of step 1 and the update
        st = make(dist.group.WORLD)
        st.keep_grads = True
        p0 = {k: v.detach().clone() for k, v in st.netC.named_parameters()}
        run(st, None)
        torch.cuda.synchronize()
        singles = gather(gc_single, world)
        res[tag + "_gradC_sum_vs_singles"] = rel(st.eC.fp.grad.cpu(), singles[0] + singles[1])
        fp = st.eC.fp
        mean = (singles[0] + singles[1]).cuda() * 0.5
        now = dict(st.netC.named_parameters())
        res[tag + "_paramC_update_vs_mean_grad"] = max(
            rel(now[k].detach(), p0[k] - Opt.lr_C * 1.9 * (fp.logical(mean, k) + 5e-4 * p0[k]))
            for k in ("conv1.weight", "layer2.0.shortcut.0.weight", "layer4.1.conv2.weight", "linear.weight"))

        # ---- 3. the unequal second step
        run(st, None, 1)
        torch.cuda.synchronize()
        res[tag + "_replicas_bit_identical_after_unequal_step"] = all(
            gather_equal(buf) for eng in (st.eC, st.eG) for buf in (eng.fp.flat, eng.fp.mom))
        m = st.read_metrics()
        res[tag + "_finite"] = bool(all(np.isfinite(v) for v in m.values()))
        res[tag + "_" + own_sum] = float(m[own_sum])
        res[tag + "_samples"] = float(m["samples"])
        del st

    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
