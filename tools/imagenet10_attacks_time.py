"""Times of the input-aware and multi-label attacks at ImageNet-10's shape (B = 32, 224 x 224, ResNet18(input_size=224))
on one GPU: python tools/imagenet10_attacks_time.py [--steps 20] [--windows 3] [--out profiles/imagenet10_attacks_time.json]

One JSON line (also written to --out):
  * ms/step of InputAwareStep and of MultiLabelStep in windows interleaved with AlternatedStep at the same shape (context:
    the input-aware step runs the generator and netC's differentiated eval pass over 64 images, the multi-label step
    runs the generator forward twice);
  * device time of combat_trigger_pair_fwd / _bwd next to the two plain combat_trigger_fwd / _bwd calls they replace, and
    of combat_trigger_groups_fwd / _bwd next to one plain call over the same 32 images: windows of `calls` launches
    between two device events, the two sides alternating in one process; the ratio (paired or grouped over plain) of
    each pair of neighbouring windows, with its min .. max;
  * combat_cond_fwd and combat_cond_wgrad on a 224 x 224 map, alone.
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
from combat_amd import nets, ops, step as step_mod, trigger  # noqa: E402

bf16 = torch.bfloat16


class Opt:
    noise_rate, ratio, kernel_size, sigma = 0.08, 0.65, 3, (0.1, 1.0)
    pc, target_label, attack_mode, num_classes = 0.5, 0, "all2one", 10
    L2_weight, clean_model_weight, lr_C, lr_G = 0.02, 0.8, 1e-2, 1e-2
    dataset, post_transform_option, random_crop, random_rotation = "imagenet10", "use", 5, 10
    s, grid_rescale, bs, cross_weight = 2, 0.15, 32, 0.2


def window(fn, calls):
    """ms per call of `calls` calls of fn between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def versus(new, plain, calls, windows):
    """Alternating windows of the two launch sequences after a warm-up window of each."""
    window(new, 3), window(plain, 3)
    a, b = [], []
    for _ in range(windows):
        a.append(window(new, calls))
        b.append(window(plain, calls))
    r = [x / y for x, y in zip(a, b)]
    rd = lambda v: [round(t, 4) for t in v]
    return {"ms": rd(a), "plain_ms": rd(b), "ratio": round(float(np.median(r)), 3), "ratio_min": round(min(r), 3),
            "ratio_max": round(max(r), 3), "calls_per_window": calls}


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
        "inputaware": step_mod.InputAwareStep(mk(), nets.UnetGenerator(opt).cuda(), mk().eval(), netf, opt),
        "multilabel": step_mod.MultiLabelStep(mk(), nets.CUnetGeneratorv1(opt).cuda(), mk().eval(), netf, opt),
    }
    gen = torch.Generator().manual_seed(1234)
    pool, tg = [], []
    for _ in range(4):
        u8 = torch.randint(0, 256, (bs, 3, hw, hw), generator=gen, dtype=torch.uint8)
        pool.append((((u8.float() / 255) - 0.5) / 0.5).cuda())
        tg.append(torch.randint(0, opt.num_classes, (bs,), generator=gen))

    def run(tag, i):
        if tag == "inputaware":
            steps[tag].run(pool[i % 4], tg[i % 4], pool[(i + 1) % 4])
        else:
            steps[tag].run(pool[i % 4], tg[i % 4])

    out = {"machine": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "shape": "B=%d %dx%d ResNet18" % (bs, hw, hw), "steps": args.steps, "windows": args.windows}
    for tag in steps:
        for i in range(3):
            run(tag, i)
    torch.cuda.synchronize()
    acc = {tag: [] for tag in steps}
    for _ in range(args.windows):        # interleaved: alternated, inputaware, multilabel, alternated, ...
        for tag in steps:
            t0 = time.perf_counter()
            for i in range(args.steps):
                run(tag, i)
            torch.cuda.synchronize()
            acc[tag].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))
    for tag in steps:
        out[tag + "_step_ms"] = acc[tag]
        out[tag + "_finite"] = bool(all(np.isfinite(v) for v in steps[tag].read_metrics().values()))
    for tag in ("inputaware", "multilabel"):
        out[tag + "_over_alternated"] = round(float(np.median(acc[tag])) / float(np.median(acc["alternated"])), 3)

    # ---- the trigger launches by themselves, on the input-aware step's own buffers (64 generator rows)
    st = steps["inputaware"]
    s, x, pm = st.cur, pool[0], st.P
    noise = st.eG.output(s.sG)
    k1 = torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(sg, 3)) for sg in (0.6, 0.3)]).float().cuda()
    l2s = 0.02 / float(bs * 3 * hw * hw)
    bd, bd2, mse = torch.empty_like(s.bd), torch.empty_like(s.bd), torch.empty(3 * bs, device="cuda")
    d1, d2, dx = (torch.randn(bs, 3, hw, hw, device="cuda") * 1e-3 for _ in range(3))
    dn = torch.empty(2 * bs, hw, hw, 8, dtype=bf16, device="cuda")

    def plain_fwd2():
        ops.trigger_fwd(x, noise[:bs], pm, k1[0], 0.08, bd, None, mse)
        ops.trigger_fwd(x, noise[bs:], pm, k1[1], 0.08, bd2)

    def plain_bwd2():
        ops.trigger_bwd(x, noise[:bs], pm, k1[0], 0.08, d1, bd, l2s, dn[:bs], True, d2)
        ops.trigger_bwd(x, noise[bs:], pm, k1[1], 0.08, dx, None, 0.0, dn[bs:], True)

    c, w = args.calls, args.windows
    out["pair_fwd_vs_two_plain"] = versus(lambda: ops.trigger_pair_fwd(x, noise, pm, k1, 0.08, bd, bd2, mse), plain_fwd2, c, w)
    out["pair_bwd_vs_two_plain"] = versus(lambda: ops.trigger_pair_bwd(x, noise, pm, k1, 0.08, d1, bd, l2s, dx, dn, True, d2),
                                          plain_bwd2, c, w)
    ps = step_mod.chunk_size(bs, opt.num_classes)
    groups = (bs + ps - 1) // ps
    kg = torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(0.15 + 0.1 * i, 3)) for i in range(groups)]).float().cuda()
    n1, dn1 = noise[:bs], dn[:bs]
    out["groups_fwd_vs_one_plain"] = versus(lambda: ops.trigger_groups_fwd(x, n1, pm, kg, ps, 0.08, bd, mse),
                                            lambda: ops.trigger_fwd(x, n1, pm, kg[0], 0.08, bd, None, mse), c, w)
    out["groups_bwd_vs_one_plain"] = versus(lambda: ops.trigger_groups_bwd(x, n1, pm, kg, ps, 0.08, d1, bd, l2s, dn1, True, d2),
                                            lambda: ops.trigger_bwd(x, n1, pm, kg[0], 0.08, d1, bd, l2s, dn1, True, d2), c, w)

    # ---- the label conditioning at a 224 x 224 map (one workgroup per image), alone
    nf, classes = 64, opt.num_classes
    wt = (torch.randn(nf, 9, nf + classes, device="cuda") * 0.05).contiguous()
    labels = tg[0].to(torch.int32).cuda()
    cond = torch.empty(bs, hw, hw, nf, dtype=bf16, device="cuda")
    dgrad = (torch.randn(bs, hw, hw, nf, device="cuda") * 0.01).to(bf16)
    dw, scratch = torch.zeros(nf, 9, nf + classes, device="cuda"), torch.empty(bs * 9 * nf, device="cuda")
    for name, fn in (("cond_fwd", lambda: ops.cond_fwd(wt, labels, classes, cond)),
                     ("cond_wgrad", lambda: ops.cond_wgrad(dgrad, labels, classes, dw, scratch))):
        window(fn, 3)
        ts = [window(fn, 20) for _ in range(w)]
        out[name] = {"ms": [round(t, 4) for t in ts], "calls_per_window": 20}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
