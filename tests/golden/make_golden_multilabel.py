"""Generate tests/golden/multilabel_step.npz through the reference's own nn.Modules (CUnetGeneratorv1,
networks/models.py:472-555; PreActResNet18) with torch.optim.SGD:

  * cunet/...   CUnetGeneratorv1's output and parameter gradients for 3 images with labels [0, 9, 4] on a fixed seed
  * step.../trace/final   two multi-label steps (train_generator_multilabel.py:160-242), b = 16, no augmentation
                (--post_transform_option no_use), recorded num_bd (0, then 3) and per-chunk sigmas

Like make_golden.py it needs the reference tree, which the GPU machines do not have; the .npz it writes is data.  Blur
and low-pass: make_golden.py's restatements (torchvision is absent here).  The generator's rate is the reference's
lr_C * 0.1 (:115)."""
import numpy as np
import torch
import torch.nn.functional as F

from make_golden import Opt, PreActResNet18, _blur, _low_freq, rng, save, summarize, synth_images  # noqa: F401
from networks.models import CUnetGeneratorv1

B, STEPS, LR_C, CLASSES = 16, 2, 1e-2, 10
NUM_BD, SIG_C = [0, 3], [0.5, 0.35]
PS = int((B - 1) / CLASSES) + 1
SIG_G = [[0.9, 0.2, 0.55, 0.15, 0.7, 0.4, 0.95, 0.3], [0.25, 0.8, 0.6, 0.12, 0.45, 0.99, 0.33, 0.5]]   # one per chunk


def make_opt():
    o = Opt()
    o.num_classes = CLASSES
    return o


def batches(s):
    inputs = synth_images(B, 32, 4234 + s)
    targets = torch.randint(0, CLASSES, (B,), generator=rng(6321 + s))
    return inputs, targets


def mix(x, noise, sigma):
    return _blur(torch.clamp(x + _low_freq(noise) * 0.08, -1, 1), sigma)


def golden_cunet(out):
    torch.manual_seed(3)
    net = CUnetGeneratorv1(make_opt())
    out["cunet/seed"] = np.int64(3)
    x = synth_images(3, 32, 77)
    y = torch.tensor([0, 9, 4])
    g = torch.randn(3, 3, 32, 32, generator=rng(78))
    noise = net(x, y)
    grads = torch.autograd.grad(noise, list(net.parameters()), g)
    out["cunet/x"], out["cunet/labels"], out["cunet/g"] = x.numpy(), y.numpy(), g.numpy()
    out["cunet/y"] = noise.detach().numpy()
    # conv0_1.weight's gradient in full (its W_y columns are what the new kernels produce), the rest as summaries
    names = [k for k, _ in net.named_parameters()]
    out["cunet/g_conv0_1_weight"] = grads[names.index("conv0_1.weight")].numpy()
    summarize(zip(names, grads), out, "cunet/gp")


def main():
    out = {"seeds": np.array([0, 1, 2]), "lr_c": np.float64(LR_C), "lr_g": np.float64(LR_C * 0.1), "ps": np.int64(PS),
           "num_bd": np.array(NUM_BD), "sigma_c": np.array(SIG_C), "sigma_g": np.array(SIG_G)}
    golden_cunet(out)
    torch.manual_seed(0)
    netc = PreActResNet18()
    torch.manual_seed(1)
    clean = PreActResNet18().eval()
    torch.manual_seed(2)
    netg = CUnetGeneratorv1(make_opt())
    opt_c = torch.optim.SGD(netc.parameters(), LR_C, momentum=0.9, weight_decay=5e-4, nesterov=True)
    opt_g = torch.optim.SGD(netg.parameters(), LR_C * 0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    ce = torch.nn.CrossEntropyLoss()
    keys = ("loss_c", "loss_ce", "loss_l2", "clean_model_loss", "clean_correct", "bd_correct", "clean_model_correct",
            "clean_model_bd_ba", "clean_model_bd_asr")
    trace = {k: [] for k in keys}
    for s in range(STEPS):
        inputs, targets = batches(s)
        out["step%d/x_sum" % s] = np.float64(inputs.double().sum())
        out["step%d/targets" % s] = targets.numpy()
        # ---- Phase C (:164-190)
        netg.eval(); netc.train(); opt_c.zero_grad()
        nb = NUM_BD[s]
        chg, chg_t = inputs[:nb], targets[:nb]
        ibd = mix(chg, netg(chg, chg_t), SIG_C[s]) if nb else chg
        loss_c = ce(netc(torch.cat([ibd, inputs[nb:]], 0)), targets)
        loss_c.backward()
        opt_c.step()
        with torch.no_grad():
            clean_preds = clean(inputs)
        # ---- Phase G (:192-242)
        netc.eval(); netg.train(); opt_g.zero_grad()
        with torch.no_grad():
            pred_clean = netc(inputs)
        bds, tmps = [], []
        for ci in range(CLASSES):
            si = ci * PS
            ei = min(si + PS, B)
            if si >= ei:
                break
            tmp = targets[si:ei] * 0 + ci
            bds.append(mix(inputs[si:ei], netg(inputs[si:ei], tmp), SIG_G[s][ci]))
            tmps.append(tmp)
        bd, tmp = torch.cat(bds, 0), torch.cat(tmps, 0)
        out["step%d/chunk_classes" % s] = tmp.numpy()
        pred_bd = netc(bd)
        loss_ce = ce(pred_bd, tmp)
        loss_l2 = F.mse_loss(bd, inputs)
        cm_preds = clean(bd)
        cm_loss = ce(cm_preds, targets)
        loss = loss_ce + 0.02 * loss_l2 + 0.8 * cm_loss
        loss.backward()
        opt_g.step()
        for k, v in (("loss_c", loss_c), ("loss_ce", loss_ce), ("loss_l2", loss_l2), ("clean_model_loss", cm_loss)):
            trace[k].append(float(v.detach()))
        for k, p, t in (("clean_correct", pred_clean, targets), ("bd_correct", pred_bd, tmp),
                        ("clean_model_correct", clean_preds, targets), ("clean_model_bd_ba", cm_preds, targets),
                        ("clean_model_bd_asr", cm_preds, tmp)):
            trace[k].append(int((p.argmax(1) == t).sum()))
        out["step%d/bd_sum" % s] = np.float64(bd.detach().double().sum())
    for k, v in trace.items():
        out["trace/" + k] = np.array(v, dtype=np.float64)
    summarize(netc.state_dict().items(), out, "final/netc")
    summarize(netg.state_dict().items(), out, "final/netg")
    save("multilabel_step.npz", out)


if __name__ == "__main__":
    main()
