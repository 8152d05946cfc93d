"""Generate tests/golden/inputaware_step.npz: two input-aware steps (reference train_generator_inputaware.py:170-266)
driven through the reference's own nn.Modules with torch.optim.SGD, b = 16, no augmentation (--post_transform_option
no_use), recorded num_bd / sigmas / cross_weight.  Like make_golden.py it needs the reference tree, which the GPU
machines do not have; the .npz it writes is data.  Blur and low-pass: make_golden.py's restatements (torchvision is
absent here).  The generator's rate is the reference's lr_C * 0.1 (:120-126)."""
import numpy as np
import torch
import torch.nn.functional as F

from make_golden import (Opt, PreActResNet18, UnetGenerator, _blur, _low_freq, rng, save, summarize,  # noqa: F401
                         synth_images)

B, STEPS, LR_C, CROSS_WEIGHT = 16, 2, 1e-2, 0.2
NUM_BD, SIG_C, SIG_G, SIG_X = [3, 0], [0.35, 0.8], [0.9, 0.2], [0.45, 0.7]


def batches(s):
    inputs = synth_images(B, 32, 2234 + s)
    inputs2 = synth_images(B, 32, 3234 + s)
    targets = torch.randint(0, 10, (B,), generator=rng(5321 + s))
    targets[:4] = 0
    return inputs, inputs2, targets


def mix(x, noise, sigma):
    return _blur(torch.clamp(x + _low_freq(noise) * 0.08, -1, 1), sigma)


def main():
    out = {"seeds": np.array([0, 1, 2]), "lr_c": np.float64(LR_C), "lr_g": np.float64(LR_C * 0.1),
           "cross_weight": np.float64(CROSS_WEIGHT), "num_bd": np.array(NUM_BD), "sigma_c": np.array(SIG_C),
           "sigma_g": np.array(SIG_G), "sigma_x": np.array(SIG_X)}
    torch.manual_seed(0)
    netc = PreActResNet18()
    torch.manual_seed(1)
    clean = PreActResNet18().eval()
    torch.manual_seed(2)
    netg = UnetGenerator(Opt())
    opt_c = torch.optim.SGD(netc.parameters(), LR_C, momentum=0.9, weight_decay=5e-4, nesterov=True)
    opt_g = torch.optim.SGD(netg.parameters(), LR_C * 0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    ce = torch.nn.CrossEntropyLoss()
    keys = ("loss_c", "loss_ce", "loss_cross", "loss_l2", "clean_model_loss", "clean_correct", "bd_correct",
            "cross_correct", "clean_model_correct", "clean_model_bd_ba", "clean_model_bd_asr")
    trace = {k: [] for k in keys}
    for s in range(STEPS):
        inputs, inputs2, targets = batches(s)
        # the batches are regenerated from their seeds by the test (synth_images): only their sums are kept
        out["step%d/x_sum" % s], out["step%d/x2_sum" % s] = np.float64(inputs.double().sum()), np.float64(inputs2.double().sum())
        out["step%d/targets" % s] = targets.numpy()
        bd_targets = torch.zeros_like(targets)
        # ---- Phase C (:189-223)
        netg.eval(); netc.train(); opt_c.zero_grad()
        trg = (targets == bd_targets).nonzero()[:, 0]
        ntrg = (targets != bd_targets).nonzero()[:, 0]
        nb = NUM_BD[s]
        chg = inputs[trg[:nb]]
        ibd = mix(chg, netg(chg), SIG_C[s]) if nb else chg
        tot_in = torch.cat([ibd, inputs[trg[nb:]], inputs[ntrg]], 0)
        tot_t = torch.cat([bd_targets[trg[:nb]], targets[trg[nb:]], targets[ntrg]], 0)
        loss_c = ce(netc(tot_in), tot_t)
        loss_c.backward()
        opt_c.step()
        with torch.no_grad():
            clean_preds = clean(inputs)
        # ---- Phase G (:227-266)
        netc.eval(); netg.train(); opt_g.zero_grad()
        bd = mix(inputs, netg(inputs), SIG_G[s])
        bd2 = mix(inputs, netg(inputs2), SIG_X[s])
        with torch.no_grad():
            pred_clean = netc(inputs)
        pred_cross = netc(bd2)
        pred_bd = netc(bd)
        loss_ce, loss_cross = ce(pred_bd, bd_targets), ce(pred_cross, targets)
        loss_l2 = F.mse_loss(bd, inputs)
        cm_preds = clean(bd)
        cm_loss = ce(cm_preds, targets)
        loss = loss_ce + CROSS_WEIGHT * loss_cross + 0.02 * loss_l2 + 0.8 * cm_loss
        loss.backward()
        opt_g.step()
        for k, v in (("loss_c", loss_c), ("loss_ce", loss_ce), ("loss_cross", loss_cross), ("loss_l2", loss_l2),
                     ("clean_model_loss", cm_loss)):
            trace[k].append(float(v.detach()))
        for k, p, t in (("clean_correct", pred_clean, targets), ("bd_correct", pred_bd, bd_targets),
                        ("cross_correct", pred_cross, targets), ("clean_model_correct", clean_preds, targets),
                        ("clean_model_bd_ba", cm_preds, targets), ("clean_model_bd_asr", cm_preds, bd_targets)):
            trace[k].append(int((p.argmax(1) == t).sum()))
        out["step%d/bd2_sum" % s] = np.float64(bd2.detach().double().sum())
    for k, v in trace.items():
        out["trace/" + k] = np.array(v, dtype=np.float64)
    summarize(netc.state_dict().items(), out, "final/netc")
    summarize(netg.state_dict().items(), out, "final/netg")
    save("inputaware_step.npz", out)


if __name__ == "__main__":
    main()
