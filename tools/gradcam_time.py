"""Time Grad-CAM on CIFAR-shaped data: one GradCam.maps call over n = 20 images (the reference's count) -- the tapped eval
forward, combat_gradcam_seed, the input-gradient launches of layer4 and combat_gradcam_map -- and its split into those
parts, against the reference-style procedure on the same GPU: per image a batch-1 forward of a plain torch PreActResNet18
with the same weights and a hook on layer3[1], the one-hot backward through the whole network by stock PyTorch-ROCm
autograd, both tensors copied to the host, the Python loop over the 256 channels, the resize and the normalisation
(gradcam.py:162-198; cv2.resize is not available: combat_amd.defenses.gradcam_resize_reference in fp32 stands in), 20
times.  The baseline is never the code under test.

    python tools/gradcam_time.py [--images 20] [--repeats 200] [--torch_repeats 5]

Prints one JSON line.  "maps_ms" and the parts are medians of device-event times around the launches alone (the call does
not wait for the device; its host time is "maps_host_ms", a wall clock around the un-synchronised call); "torch_ms" is the
median wall-clock time of the 20-image loop, which ends with its maps on the host.  The paths alternate in one session after
untimed runs of each."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plain_classifier():
    """tools/neural_cleanse_time.py's stock-torch PreActResNet18 (state_dict-compatible with combat_amd.nets')."""
    spec = importlib.util.spec_from_file_location("neural_cleanse_time", os.path.join(ROOT, "tools", "neural_cleanse_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TorchPreActResNet18()


def reference_style(plain, x, resize):
    """gradcam.py:162-198 for every image of x, one at a time; the maps [n][32][32] on the host."""
    kept = {}
    handle = plain.layer3[1].register_forward_hook(lambda mod, inp, out: kept.update(out=out))
    maps = []
    try:
        for i in range(x.shape[0]):
            single = x[i:i + 1].clone().requires_grad_(True)
            output = plain(single)
            features = kept["out"]
            grads = []
            features.register_hook(grads.append)
            index = int(np.argmax(output.cpu().data.numpy()))
            one_hot = np.zeros((1, output.size()[-1]), dtype=np.float32)
            one_hot[0][index] = 1
            one_hot = torch.sum(torch.from_numpy(one_hot).cuda() * output)
            plain.zero_grad()
            one_hot.backward()
            grads_val = grads[-1].cpu().data.numpy()
            target = features.cpu().data.numpy()[0, :]
            weights = np.mean(grads_val, axis=(2, 3))[0, :]
            cam = np.zeros(target.shape[1:], dtype=np.float32)
            for k, w in enumerate(weights):
                cam += w * target[k, :, :]
            cam = resize(np.maximum(cam, 0), 32)
            cam = cam - np.min(cam)
            with np.errstate(invalid="ignore"):
                maps.append(cam / np.max(cam))
    finally:
        handle.remove()
    return np.stack(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--torch_repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gradcam_time.py measures on the GPU; none found")
    from combat_amd import defenses, nets, ops
    from combat_amd.engine import pad_batch

    torch.manual_seed(0)
    netC = nets.PreActResNet18().cuda().eval().requires_grad_(False)
    plain = plain_classifier().cuda()
    plain.load_state_dict(netC.state_dict())
    plain.eval()
    n = a.images
    u8 = np.random.default_rng(1).integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    x = ((torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5).contiguous().cuda()
    cam_obj = defenses.GradCam(netC, 5)

    cam, chosen = cam_obj.maps(x)                                          # untimed: plans, slots, code objects
    ref = reference_style(plain, x, defenses.gradcam_resize_reference)
    torch.cuda.synchronize()
    ours = cam.cpu().numpy()
    both = ~(np.isnan(ours).any(axis=(1, 2)) | np.isnan(ref).any(axis=(1, 2)))

    def events(fn, repeats):
        """Median device time (ms) of fn's launches, one event pair per call."""
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), min(times), max(times)

    # the parts of maps(), as maps() issues them
    eng, N = cam_obj.eng, pad_batch(n)
    slot = eng.slot("gradcam", N, 32)
    fwd = eng.forward_plan(slot, False, keep_raw_blocks=(5,))
    bwd = eng.backward_eval_plan(slot, 1.0, head_done=True, stop_before=6)
    logits, d_feat = eng.head_bufs(slot)["logits"], slot.bufs["g.feat"]
    picked = torch.empty(N, dtype=torch.int32, device="cuda")
    act, grad = cam_obj.tapped(n)
    out = torch.empty(n, 32, 32, device="cuda")

    def part_forward():
        ops.image_to_c8(x, eng.input(slot))
        fwd.run()

    def part_backward():
        ops.gradcam_seed(logits, None, n, eng.lin_w, picked, d_feat)
        bwd.run()

    t_maps, t_base, host = [], [], []
    for r in range(a.torch_repeats):
        t_maps.append(events(lambda: cam_obj.maps(x), a.repeats // a.torch_repeats))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            cam_obj.maps(x)
        host.append((time.perf_counter() - t0) / 20)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_style(plain, x, defenses.gradcam_resize_reference)
        torch.cuda.synchronize()
        t_base.append(time.perf_counter() - t0)
    maps_ms = statistics.median(t[0] for t in t_maps)
    f_ms, b_ms, m_ms = (events(fn, a.repeats) for fn in (part_forward, part_backward, lambda: ops.gradcam_map(act, grad, n, out)))
    out_json = {"device": torch.cuda.get_device_name(0), "images": n, "slot_rows": N, "repeats": a.repeats,
                "maps_ms": round(maps_ms, 4), "maps_ms_minmax": [round(min(t[1] for t in t_maps), 4), round(max(t[2] for t in t_maps), 4)],
                "maps_host_ms": round(statistics.median(host) * 1e3, 4),
                "forward_ms": round(f_ms[0], 4), "seed_and_backward_ms": round(b_ms[0], 4), "map_kernel_ms": round(m_ms[0], 4),
                "forward_calls": len(fwd.calls), "backward_calls": len(bwd.calls),
                "torch_ms": round(statistics.median(t_base) * 1e3, 2),
                "torch_ms_minmax": [round(min(t_base) * 1e3, 2), round(max(t_base) * 1e3, 2)],
                "speedup": round(statistics.median(t_base) * 1e3 / maps_ms, 1),
                # same weights, same images: the bf16 engine against fp32 autograd (maps that are NaN on either side left out)
                "images_compared": int(both.sum()),
                "classes_agree": int((chosen.cpu().numpy() == np.array([int(np.argmax(r)) for r in plain(x).detach().cpu().numpy()])).sum()),
                "max_abs_map_difference": float(np.abs(ours[both] - ref[both]).max()) if both.any() else None}
    print(json.dumps(out_json))


if __name__ == "__main__":
    main()
