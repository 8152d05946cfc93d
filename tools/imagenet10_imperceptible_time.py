"""Times of the imperceptible (total-variation) attack at ImageNet-10's shape (B = 32, 224 x 224, ResNet18(input_size=224))
on one GPU: python tools/imagenet10_imperceptible_time.py [--steps 20] [--windows 3] [--out profiles/imagenet10_imperceptible_time.json]

One JSON line (also written to --out), measured as tools/imagenet10_attacks_time.py measures its attacks:
  * ms/step of ImperceptibleStep (tv_weight = config.py's default 0.01) in windows interleaved with AlternatedStep at the
    same shape;
  * device time of combat_trigger_tv_big_fwd next to combat_trigger_fwd with mse_partial, and of
    combat_trigger_tv_big_bwd next to combat_trigger_bwd, on the same operands (the step's own generator output, 32
    images): windows of `calls` launches between two device events, the two sides alternating in one process; the ratio
    (TV over plain) of each pair of neighbouring windows, with its min .. max.  The plain calls are this tree's, which
    the TV entry points leave as they were;
  * the strip forward launch without a reduction behind it, from the same kind of windows: what is left of either
    forward call is its reduction launch.
Times are from device events (launch sequences) or a host clock around work that ends in a device synchronise (steps)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from combat_amd import nets, ops, step as step_mod, trigger  # noqa: E402
from imagenet10_attacks_time import Opt as BaseOpt, versus, window  # noqa: E402

bf16 = torch.bfloat16


class Opt(BaseOpt):
    tv_weight = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    opt = Opt()
    nets.configure_dataset(opt)
    hw, bs = opt.input_height, opt.bs
    torch.manual_seed(0)
    np.random.seed(0)
    mk = lambda: nets.default_classifier(opt).cuda()
    netf = nets.FrequencyModel(2, 3, hw).cuda().eval()
    steps = {
        "alternated": step_mod.AlternatedStep(mk(), nets.UnetGenerator(opt).cuda(), mk().eval(), netf, opt),
        "imperceptible": step_mod.ImperceptibleStep(mk(), nets.UnetGenerator(opt).cuda(), mk().eval(), netf, opt),
    }
    gen = torch.Generator().manual_seed(1234)
    pool, tg = [], []
    for _ in range(4):
        u8 = torch.randint(0, 256, (bs, 3, hw, hw), generator=gen, dtype=torch.uint8)
        pool.append((((u8.float() / 255) - 0.5) / 0.5).cuda())
        tg.append(torch.randint(0, opt.num_classes, (bs,), generator=gen))

    out = {"machine": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "shape": "B=%d %dx%d ResNet18" % (bs, hw, hw), "steps": args.steps, "windows": args.windows,
           "tv_weight": opt.tv_weight}
    for tag in steps:
        for i in range(3):
            steps[tag].run(pool[i % 4], tg[i % 4])
    torch.cuda.synchronize()
    acc = {tag: [] for tag in steps}
    for _ in range(args.windows):        # interleaved: alternated, imperceptible, alternated, ...
        for tag in steps:
            t0 = time.perf_counter()
            for i in range(args.steps):
                steps[tag].run(pool[i % 4], tg[i % 4])
            torch.cuda.synchronize()
            acc[tag].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
    for tag in steps:
        out[tag + "_step_ms"] = acc[tag]
        out[tag + "_finite"] = bool(all(np.isfinite(v) for v in steps[tag].read_metrics().values()))
    out["imperceptible_over_alternated"] = round(float(np.median(acc["imperceptible"])) / float(np.median(acc["alternated"])), 3)

    # ---- the trigger launches by themselves, on the imperceptible step's own generator output
    st = steps["imperceptible"]
    s, x, pm = st.cur, pool[0], st.P
    noise = st.eG.output(s.sG)
    k1 = torch.from_numpy(trigger.gaussian_kernel1d(0.6, 3)).float().cuda()
    l2s = 0.02 / float(bs * 3 * hw * hw)
    tvs = opt.tv_weight / bs
    bd, mse, tv = torch.empty_like(s.bd), torch.empty(3 * bs, device="cuda"), torch.empty(3 * bs, device="cuda")
    d1, d2 = (torch.randn(bs, 3, hw, hw, device="cuda") * 1e-3 for _ in range(2))
    dn = torch.empty(bs, hw, hw, 8, dtype=bf16, device="cuda")
    c, w = args.calls, args.windows
    plain_fwd = lambda: ops.trigger_fwd(x, noise, pm, k1, 0.08, bd, None, mse)
    plain_bwd = lambda: ops.trigger_bwd(x, noise, pm, k1, 0.08, d1, bd, l2s, dn, True, d2)
    out["tv_fwd_vs_plain"] = versus(lambda: ops.trigger_tv_fwd(x, noise, pm, k1, 0.08, bd, tv, mse), plain_fwd, c, w)
    out["tv_bwd_vs_plain"] = versus(lambda: ops.trigger_tv_bwd(x, noise, pm, k1, 0.08, d1, bd, l2s, tvs, dn, True, d2),
                                    plain_bwd, c, w)
    # the strip forward alone (no reduction behind it): what is left of either forward call is its reduction launch
    window(lambda: ops.trigger_fwd(x, noise, pm, k1, 0.08, bd), 3)
    ts = [window(lambda: ops.trigger_fwd(x, noise, pm, k1, 0.08, bd), c) for _ in range(w)]
    out["strip_fwd_alone"] = {"ms": [round(t, 4) for t in ts], "calls_per_window": c}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
