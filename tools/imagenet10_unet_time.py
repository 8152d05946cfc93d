"""Times of the UNet-trigger attack at ImageNet-10's shape (B = 32, 224 x 224, ResNet18(input_size=224)) on one GPU:
python tools/imagenet10_unet_time.py [--steps 20] [--quick]

One JSON line: ms/step of AlternatedStep and, interleaved with it, of WanetStep at the same shape; the generator's
forward and backward plans; the strip trigger launches (forward with the squared-error partials, backward with both
gradient shares and the L2 term) and combat_dct_u8 -- existing code with the same two 224^3 products per plane, the
yardstick of the new forward -- at n = 32, by device events; and the same step as the reference writes it in stock
PyTorch-ROCm eager (the oracle's functional restatement on the GPU, fp32, as bench.py's baseline leg does at 32 x 32).
--quick: few steps and no eager leg (for a profiler around the process)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from combat_amd import nets, ops, step as step_mod, trigger  # noqa: E402


class Opt:
    noise_rate, ratio, kernel_size, sigma = 0.08, 0.65, 3, (0.1, 1.0)
    pc, target_label, attack_mode, num_classes = 0.5, 0, "all2one", 10
    L2_weight, clean_model_weight, lr_C, lr_G = 0.02, 0.8, 1e-2, 1e-2
    dataset, post_transform_option, random_crop, random_rotation = "imagenet10", "use", 5, 10
    s, grid_rescale, bs = 2, 0.15, 32


def events(fn, reps):
    """Median and range (ms) of `reps` calls of fn, each bracketed by device events, after two warm-up calls."""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    steps = 4 if args.quick else args.steps
    opt = Opt()
    nets.configure_dataset(opt)
    hw, bs = opt.input_height, opt.bs
    torch.manual_seed(0)
    np.random.seed(0)
    mk = lambda: nets.default_classifier(opt).cuda()
    netf = nets.FrequencyModel(2, 3, hw).cuda().eval()
    st_u = step_mod.AlternatedStep(mk(), nets.UnetGenerator(opt).cuda(), mk().eval(), netf, opt)
    st_w = step_mod.WanetStep(mk(), nets.GridGenerator(opt).cuda(), mk().eval(), netf, opt)
    gen = torch.Generator().manual_seed(1234)
    pool, tg = [], []
    for _ in range(4):
        u8 = torch.randint(0, 256, (bs, 3, hw, hw), generator=gen, dtype=torch.uint8)
        pool.append((((u8.float() / 255) - 0.5) / 0.5).cuda())
        tg.append(torch.randint(0, opt.num_classes, (bs,), generator=gen))
    out = {"shape": "B=%d %dx%d ResNet18" % (bs, hw, hw), "steps": steps}
    for st in (st_u, st_w):
        for i in range(3):
            st.run(pool[i % 4], tg[i % 4])
    torch.cuda.synchronize()
    acc = {"unet": [], "wanet": []}
    for rep in range(2):        # interleaved: unet, wanet, unet, wanet
        for tag, st in (("unet", st_u), ("wanet", st_w)):
            t0 = time.perf_counter()
            for i in range(steps):
                st.run(pool[i % 4], tg[i % 4])
            torch.cuda.synchronize()
            acc[tag].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
    out["unet_step_ms"], out["wanet_step_ms"] = acc["unet"], acc["wanet"]
    m = st_u.read_metrics()
    out["finite"] = bool(all(np.isfinite(v) for v in m.values()))
    reps = 5 if args.quick else 20
    out["generator_forward"] = events(lambda: st_u.pl["G_f"].run(), reps)
    out["generator_backward"] = events(lambda: st_u.pl["G_b"].run(), reps)
    # the launches by themselves, on the step's own buffers
    s, x = st_u.cur, pool[0]
    noise = st_u.eG.output(s.sG)
    k1 = torch.tensor(trigger.gaussian_kernel1d(0.6, 3)).float().cuda()
    dn = torch.empty(bs, hw, hw, 8, dtype=torch.bfloat16, device="cuda")
    l2s = 0.02 / float(bs * 3 * hw * hw)
    out["trigger_fwd"] = events(lambda: ops.trigger_fwd(x, noise, st_u.P, k1, 0.08, s.bd, None, s.mse), reps)
    out["trigger_bwd"] = events(lambda: ops.trigger_bwd(x, noise, st_u.P, k1, 0.08, s.d_bd, s.bd, l2s, dn, True, s.d_bd2), reps)
    d8 = torch.empty(bs, hw, hw, 8, dtype=torch.bfloat16, device="cuda")
    out["dct_u8"] = events(lambda: ops.dct_u8(s.bd, st_u.D, d8), reps)
    out["trigger_fwd_over_dct_u8"] = round(out["trigger_fwd"]["ms"] / out["dct_u8"]["ms"], 2)
    if not args.quick:
        print("before the eager leg: " + json.dumps(out), file=sys.stderr, flush=True)
        out["torch_eager_fp32"] = eager(opt, pool[0], tg[0])
        if out["torch_eager_fp32"].get("ms_per_step"):
            out["speedup_over_eager"] = round(out["torch_eager_fp32"]["ms_per_step"] / min(out["unet_step_ms"]), 1)
    print(json.dumps(out))


def eager(opt, x, t, steps=5):
    """The reference step as written, by stock PyTorch-ROCm (ATen + MIOpen) in fp32 on this GPU."""
    from oracle import combat_oracle as O
    try:
        sds = []
        for seed, ctor in ((0, lambda: nets.default_classifier(opt)), (1, lambda: nets.default_classifier(opt)),
                           (2, lambda: nets.UnetGenerator(None)), (3, lambda: nets.FrequencyModel(2, 3, opt.input_height))):
            torch.manual_seed(seed)
            sds.append({k: v.detach().clone().cuda() for k, v in ctor().state_dict().items()})
        netc, clean, netg, netf = sds
        bufs_c, bufs_g = [None] * len(O.trainable_names(netc)), [None] * len(O.trainable_names(netg))
        cfg = O.StepConfig(num_classes=opt.num_classes, classifier="resnet18")
        rng = np.random.default_rng(0)
        td = t.cuda()
        n_trg = int((t == 0).sum())
        n = x.shape[0]

        def aug():
            return O.AugParams(rng.integers(0, 11, n).astype(np.int32), rng.integers(0, 11, n).astype(np.int32),
                               np.where(rng.random(n) < 0.5, rng.uniform(-10, 10, n), 0).astype(np.float32),
                               (rng.random(n) < 0.5).astype(np.int32))

        def one():
            rnd = O.StepRandomness(min(2, n_trg), 0.5, 0.6, [aug() for _ in range(5)])
            O.alternated_step(netc, netg, clean, netf, bufs_c, bufs_g, x, td, rnd, cfg, as_written=True,
                              aug_fn=O.post_tensor_transform_batched)

        for _ in range(3):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        return {"ms_per_step": round((time.perf_counter() - t0) / steps * 1e3, 2), "steps": steps}
    except Exception as e:      # a baseline leg never takes the measurement down with it
        return {"ms_per_step": None, "why": "%s: %s" % (type(e).__name__, str(e)[:300])}


if __name__ == "__main__":
    main()
