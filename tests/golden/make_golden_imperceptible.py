"""Generate tests/golden/imperceptible_step.npz: two steps of the imperceptible configuration (reference
train_generator_imperceptible.py:160-277) driven through the reference's own nn.Modules with torch.optim.SGD, b = 16,
no augmentation (--post_transform_option no_use), recorded num_bd / sigmas and a non-default tv_weight.  Like
make_golden.py it needs the reference tree, which the GPU machines do not have; the .npz it writes is data.  Blur and
low-pass: make_golden.py's restatements (torchvision is absent here); total_variation: kornia 0.6.6's semantics
restated below (kornia is absent too, so its parity is unpinned).  The loss line is the reference's (:234-237)."""
import numpy as np
import torch
import torch.nn.functional as F

from make_golden import (Opt, PreActResNet18, UnetGenerator, _blur, _low_freq, rng, save, summarize,  # noqa: F401
                         synth_images)

B, STEPS, LR, TV_WEIGHT, L2_WEIGHT, CM_WEIGHT = 16, 2, 1e-2, 1e-4, 0.02, 0.8
NUM_BD, SIG_C, SIG_G = [3, 0], [0.35, 0.8], [0.9, 0.2]


def total_variation(x):
    """kornia.losses.total_variation of release 0.6.6: one value per image."""
    return (x[..., 1:, :] - x[..., :-1, :]).abs().sum((1, 2, 3)) + (x[..., :, 1:] - x[..., :, :-1]).abs().sum((1, 2, 3))


def batch(s):
    inputs = synth_images(B, 32, 4234 + s)
    targets = torch.randint(0, 10, (B,), generator=rng(6321 + s))
    targets[:4] = 0
    return inputs, targets


def create_inputs_bd(inputs, netg, sigma):
    """:67-75 (the blur's sigma is the recorded draw)."""
    noise_bd = netg(inputs)
    if inputs.shape[0] != 0:
        noise_bd = _low_freq(noise_bd)
    inputs_bd = torch.clamp(inputs + noise_bd * 0.08, -1, 1)
    if inputs_bd.shape[0] != 0:
        inputs_bd = _blur(inputs_bd, sigma)
    return inputs_bd


def main():
    out = {"seeds": np.array([0, 1, 2]), "lr_c": np.float64(LR), "lr_g": np.float64(LR), "tv_weight": np.float64(TV_WEIGHT),
           "num_bd": np.array(NUM_BD), "sigma_c": np.array(SIG_C), "sigma_g": np.array(SIG_G)}
    torch.manual_seed(0)
    netc = PreActResNet18()
    torch.manual_seed(1)
    clean = PreActResNet18().eval()
    torch.manual_seed(2)
    netg = UnetGenerator(Opt())
    opt_c = torch.optim.SGD(netc.parameters(), LR, momentum=0.9, weight_decay=5e-4, nesterov=True)
    opt_g = torch.optim.SGD(netg.parameters(), LR, momentum=0.9, weight_decay=5e-4, nesterov=True)
    ce = torch.nn.CrossEntropyLoss()
    keys = ("loss_c", "loss_ce", "loss_l2", "loss_tv", "clean_model_loss", "gnorm_g", "tv_grad_share", "clean_correct", "bd_correct",
            "clean_model_correct", "clean_model_bd_ba", "clean_model_bd_asr")
    trace = {k: [] for k in keys}
    for s in range(STEPS):
        inputs, targets = batch(s)
        # the batch is regenerated from its seed by the test (synth_images): only its sum is kept
        out["step%d/x_sum" % s] = np.float64(inputs.double().sum())
        out["step%d/targets" % s] = targets.numpy()
        bd_targets = torch.zeros_like(targets)
        # ---- Phase C (:164-201)
        netg.eval(); netc.train(); opt_c.zero_grad()
        trg = (targets == bd_targets).nonzero()[:, 0]
        ntrg = (targets != bd_targets).nonzero()[:, 0]
        nb = NUM_BD[s]
        chg = inputs[trg[:nb]]
        ibd = create_inputs_bd(chg, netg, SIG_C[s])
        tot_in = torch.cat([ibd, inputs[trg[nb:]], inputs[ntrg]], 0)
        tot_t = torch.cat([bd_targets[trg[:nb]], targets[trg[nb:]], targets[ntrg]], 0)
        loss_c = ce(netc(tot_in), tot_t)
        loss_c.backward()
        opt_c.step()
        with torch.no_grad():
            clean_preds = clean(inputs)
        # ---- Phase G (:203-243)
        netc.eval(); netg.train(); opt_g.zero_grad()
        bd = create_inputs_bd(inputs, netg, SIG_G[s])
        with torch.no_grad():
            pred_clean = netc(inputs)
        pred_bd = netc(bd)
        loss_ce = ce(pred_bd, bd_targets)
        loss_l2 = F.mse_loss(bd, inputs)
        loss_tv = total_variation(bd).mean()
        cm_preds = clean(bd)
        cm_loss = ce(cm_preds, targets)
        loss = loss_ce + L2_WEIGHT * loss_l2 + TV_WEIGHT * loss_tv + CM_WEIGHT * cm_loss
        (g_tv,) = torch.autograd.grad(TV_WEIGHT * loss_tv, bd, retain_graph=True)
        (g_all,) = torch.autograd.grad(loss, bd, retain_graph=True)
        loss.backward()
        trace["gnorm_g"].append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in netg.parameters()))))
        opt_g.step()
        trace["tv_grad_share"].append(float(g_tv.norm() / g_all.norm()))     # |TV part| / |whole image gradient|
        for k, v in (("loss_c", loss_c), ("loss_ce", loss_ce), ("loss_l2", loss_l2), ("loss_tv", loss_tv),
                     ("clean_model_loss", cm_loss)):
            trace[k].append(float(v.detach()))
        for k, p, t in (("clean_correct", pred_clean, targets), ("bd_correct", pred_bd, bd_targets),
                        ("clean_model_correct", clean_preds, targets), ("clean_model_bd_ba", cm_preds, targets),
                        ("clean_model_bd_asr", cm_preds, bd_targets)):
            trace[k].append(int((p.argmax(1) == t).sum()))
        d = bd.detach()
        diffs = torch.cat([(d[..., 1:, :] - d[..., :-1, :]).flatten(), (d[..., :, 1:] - d[..., :, :-1]).flatten()]).abs()
        out["step%d/near_zero_share" % s] = np.float64((diffs < 1e-3).double().mean())
    for k, v in trace.items():
        out["trace/" + k] = np.array(v, dtype=np.float64)
    print({k: v for k, v in trace.items()})
    summarize(netc.state_dict().items(), out, "final/netc")
    summarize(netg.state_dict().items(), out, "final/netg")
    save("imperceptible_step.npz", out)


if __name__ == "__main__":
    main()
