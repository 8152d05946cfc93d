"""Test-side restatement of one input-aware step (reference train_generator_inputaware.py:170-266), composed of
oracle.combat_oracle's pieces.  Phase C is the alternated step's; Phase G runs the generator on a second batch too
and mixes that noise onto the FIRST batch's images (the cross images), which netC must keep on their clean label:

    loss = CE(netC(aug3(bd)), bd_targets) + cross_weight * CE(netC(aug5(bd2)), targets)
           + L2_weight * MSE(bd, inputs) + clean_model_weight * CE(clean(aug4(bd)), targets)

with bd = T(inputs, netG(inputs), sigma_g) and bd2 = T(inputs, netG(inputs2), sigma_x)."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import combat_oracle as O


@dataclass
class Randomness:
    """Draws of one step.  aug: [aug0 .. aug5] (aug5: the cross images' transform)."""

    num_bd: int
    sigma_c: float
    sigma_g: float
    sigma_x: float
    aug: List = field(default_factory=lambda: [None] * 6)


def inputaware_step(netc, netg, clean, netf, bufs_c, bufs_g, inputs, inputs2, targets, rnd: Randomness,
                    cfg: O.StepConfig, cross_weight: float, clf_fn=None, gen_fn=None) -> Dict[str, float]:
    """Updates netc / netg (parameters, BN statistics, momentum buffers) in place; returns the step's scalars.
    cfg.lr_g is the generator's rate (the reference's lr_C * 0.1)."""
    clf = clf_fn or O._classifier(cfg)
    unet = gen_fn or O.unet_forward
    tr = O.post_tensor_transform
    mix = lambda x, noise, s: O.trigger_mix(x, noise, cfg.noise_rate, cfg.ratio, s, cfg.kernel_size)
    names_c, names_g = O.trainable_names(netc), O.trainable_names(netg)
    for d in (netc, netg, clean):
        for k in O.trainable_names(d):
            d[k].requires_grad_(True)
            d[k].grad = None
    bd_targets = O.create_targets_bd(targets, cfg.attack_mode, cfg.target_label, cfg.num_classes)

    # ---- Phase C (:175-212)
    perm, total_targets = O.poison_order(targets, bd_targets, rnd.num_bd)
    to_change = inputs[perm[:rnd.num_bd]]
    inputs_bd = mix(to_change, unet(netg, to_change), rnd.sigma_c) if to_change.shape[0] else to_change
    total_inputs = tr(torch.cat([inputs_bd, inputs[perm[rnd.num_bd:]]], dim=0), rnd.aug[0])
    loss_c = F.cross_entropy(clf(netc, total_inputs, True), total_targets)
    grads = O._grads(loss_c, [netc[k] for k in names_c], False)
    gnorm_c = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    O.sgd_nesterov_step([netc[k] for k in names_c], grads, bufs_c, cfg.lr_c)
    with torch.no_grad():
        clean_preds = clf(clean, tr(inputs, rnd.aug[1]), False)

    # ---- Phase G (:227-266)
    bd = mix(inputs, unet(netg, inputs), rnd.sigma_g)
    bd2 = mix(inputs, unet(netg, inputs2), rnd.sigma_x)
    with torch.no_grad():
        pred_clean = clf(netc, tr(inputs, rnd.aug[2]), False)
    pred_cross = clf(netc, tr(bd2, rnd.aug[5]), False)
    pred_bd = clf(netc, tr(bd, rnd.aug[3]), False)
    loss_ce = F.cross_entropy(pred_bd, bd_targets)
    loss_cross = F.cross_entropy(pred_cross, targets)
    loss_l2 = F.mse_loss(bd, inputs)
    f_correct = 0
    if netf is not None:
        with torch.no_grad():
            f_correct = int((O.frequency_model_forward(netf, O.frequency_input(bd)).argmax(1) == 1).sum())
    clean_model_preds = clf(clean, tr(bd, rnd.aug[4]), False)
    clean_model_loss = F.cross_entropy(clean_model_preds, targets)
    loss = loss_ce + cross_weight * loss_cross + cfg.l2_weight * loss_l2 + cfg.clean_model_weight * clean_model_loss
    for d in (netc, netg, clean):
        for k in O.trainable_names(d):
            d[k].grad = None
    grads = O._grads(loss, [netg[k] for k in names_g], False)
    gnorm_g = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    O.sgd_nesterov_step([netg[k] for k in names_g], grads, bufs_g, cfg.lr_g)
    for d in (netc, netg, clean):
        for k in O.trainable_names(d):
            d[k].requires_grad_(False)
    return {
        "loss_c": float(loss_c.detach()), "loss_ce": float(loss_ce.detach()), "loss_cross": float(loss_cross.detach()),
        "loss_l2": float(loss_l2.detach()), "clean_model_loss": float(clean_model_loss.detach()),
        "loss_g": float(loss.detach()), "gnorm_c": gnorm_c, "gnorm_g": gnorm_g,
        "clean_correct": int((pred_clean.argmax(1) == targets).sum()),
        "bd_correct": int((pred_bd.argmax(1) == bd_targets).sum()),
        "cross_correct": int((pred_cross.argmax(1) == targets).sum()),
        "f_correct": f_correct,
        "clean_model_correct": int((clean_preds.argmax(1) == targets).sum()),
        "clean_model_bd_ba": int((clean_model_preds.argmax(1) == targets).sum()),
        "clean_model_bd_asr": int((clean_model_preds.argmax(1) == bd_targets).sum()),
    }
