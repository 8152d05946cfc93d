"""Test-side restatement of one step of the imperceptible configuration (reference
train_generator_imperceptible.py:160-277), composed of oracle.combat_oracle's pieces.  It is the alternated step with
the smoothness of the triggered images in the generator's loss (:228, :234-237):

    loss = CE(netC(aug3(bd)), bd_targets) + L2_weight * MSE(bd, inputs) + tv_weight * TV(bd).mean()
           + clean_model_weight * CE(clean(aug4(bd)), targets),          bd = T(inputs, netG(inputs), sigma_g)

The blur is the reference's module-level 3-tap one (:52): cfg.kernel_size must be 3.

``total_variation`` restates kornia 0.6.6's ``kornia.losses.total_variation`` from its documented semantics -- per image,
the sum over C, H, W of |x[..., 1:, :] - x[..., :-1, :]| plus the same sum along W; one value per image.  kornia is not
available to these tests, so the parity of this restatement with kornia itself is NOT pinned."""
from typing import Dict

import torch
import torch.nn.functional as F

from oracle import combat_oracle as O


def total_variation(x: torch.Tensor) -> torch.Tensor:
    """[n, C, H, W] -> [n] (kornia 0.6.6 semantics, restated: parity with kornia unpinned)."""
    dh = (x[..., 1:, :] - x[..., :-1, :]).abs().sum((1, 2, 3))
    dw = (x[..., :, 1:] - x[..., :, :-1]).abs().sum((1, 2, 3))
    return dh + dw


def tv_sign_stencil(x: torch.Tensor) -> torch.Tensor:
    """d sum_i TV(x)[i] / d x in closed form: per pixel
    sgn(x[y,x] - x[y-1,x]) - sgn(x[y+1,x] - x[y,x]) + sgn(x[y,x] - x[y,x-1]) - sgn(x[y,x+1] - x[y,x]),
    terms past the border absent, sgn(0) = 0."""
    sh = torch.sign(x[..., 1:, :] - x[..., :-1, :])
    sw = torch.sign(x[..., :, 1:] - x[..., :, :-1])
    g = torch.zeros_like(x)
    g[..., 1:, :] += sh
    g[..., :-1, :] -= sh
    g[..., :, 1:] += sw
    g[..., :, :-1] -= sw
    return g


def imperceptible_step(netc, netg, clean, netf, bufs_c, bufs_g, inputs, targets, rnd: O.StepRandomness,
                       cfg: O.StepConfig, tv_weight: float, clf_fn=None, gen_fn=None, keep=None) -> Dict[str, float]:
    """Updates netc / netg (parameters, BN statistics, momentum buffers) in place; returns the step's scalars.
    keep: optional dict that receives the Phase-G inputs_bd ("bd", detached)."""
    assert cfg.kernel_size == 3, "the imperceptible step blurs with the fixed 3-tap kernel"
    clf = clf_fn or O._classifier(cfg)
    unet = gen_fn or O.unet_forward
    tr = O.post_tensor_transform
    mix = lambda x, noise, s: O.trigger_mix(x, noise, cfg.noise_rate, cfg.ratio, s, 3)
    names_c, names_g = O.trainable_names(netc), O.trainable_names(netg)
    for d in (netc, netg, clean):
        for k in O.trainable_names(d):
            d[k].requires_grad_(True)
            d[k].grad = None
    bd_targets = O.create_targets_bd(targets, cfg.attack_mode, cfg.target_label, cfg.num_classes)

    # ---- Phase C (:164-201)
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

    # ---- Phase G (:203-243)
    bd = mix(inputs, unet(netg, inputs), rnd.sigma_g)
    if keep is not None:
        keep["bd"] = bd.detach().clone()
    with torch.no_grad():
        pred_clean = clf(netc, tr(inputs, rnd.aug[2]), False)
    pred_bd = clf(netc, tr(bd, rnd.aug[3]), False)
    loss_ce = F.cross_entropy(pred_bd, bd_targets)
    loss_l2 = F.mse_loss(bd, inputs)
    loss_tv = total_variation(bd).mean()
    f_correct = 0
    if netf is not None:
        with torch.no_grad():
            f_correct = int((O.frequency_model_forward(netf, O.frequency_input(bd)).argmax(1) == 1).sum())
    clean_model_preds = clf(clean, tr(bd, rnd.aug[4]), False)
    clean_model_loss = F.cross_entropy(clean_model_preds, targets)
    loss = loss_ce + cfg.l2_weight * loss_l2 + tv_weight * loss_tv + cfg.clean_model_weight * clean_model_loss
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
        "loss_c": float(loss_c.detach()), "loss_ce": float(loss_ce.detach()), "loss_l2": float(loss_l2.detach()),
        "loss_tv": float(loss_tv.detach()), "clean_model_loss": float(clean_model_loss.detach()),
        "loss_g": float(loss.detach()), "gnorm_c": gnorm_c, "gnorm_g": gnorm_g,
        "clean_correct": int((pred_clean.argmax(1) == targets).sum()),
        "bd_correct": int((pred_bd.argmax(1) == bd_targets).sum()),
        "f_correct": f_correct,
        "clean_model_correct": int((clean_preds.argmax(1) == targets).sum()),
        "clean_model_bd_ba": int((clean_model_preds.argmax(1) == targets).sum()),
        "clean_model_bd_asr": int((clean_model_preds.argmax(1) == bd_targets).sum()),
    }
