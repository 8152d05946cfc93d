"""Test-side restatements for the label-conditioned generator of the multi-label attack (reference
networks/models.py:472-555 CUnetGeneratorv1), composed of oracle.combat_oracle's and tests/bf16_emu.py's pieces:

  * cunet_forward      the fp32 forward with the one-hot planes written out, as the reference computes it
  * cunet_forward_emu  the engine's dataflow: conv0_1 over W_f only, the planes' share added as one bf16 tensor
  * cond_ref / cond_wgrad_ref   host restatements of combat_cond_fwd / combat_cond_wgrad in the kernels' own summation
                       order (include/combat_hip.h): fp32 element-wise adds on the CPU are IEEE, so these are bit exact
  * cond_planes_f64    fp64 F.conv2d over explicit one-hot planes, for autograd references
  * trigger_groups_ref / trigger_groups_bwd_ref   the grouped trigger (image i blurred with k1[i // ps]) as dense products
  * chunk_bounds       the chunk arithmetic of the generator phase (train_generator_multilabel.py:203-213)
  * multilabel_step    one step of train_generator_multilabel.py:160-242 (tests/inputaware_ref.py is the model)
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402

bf16 = torch.bfloat16


def onehot_planes(y, num_classes, s, dtype=torch.float32):
    """networks/models.py:525-529."""
    return F.one_hot(y.long(), num_classes=num_classes).to(dtype)[:, :, None, None].expand(-1, -1, s, s)


def cunet_forward(p, x, y, num_classes):
    """CUnetGeneratorv1.forward (networks/models.py:523-555) in fp32: oracle.unet_forward with the planes concatenated
    in front of conv0_1."""
    lr = lambda t: F.leaky_relu(t, 0.2)
    inorm = lambda t: F.instance_norm(t, eps=1e-5)
    conv = lambda name, t, stride=1: F.conv2d(t, p[name + ".weight"], p[name + ".bias"], stride=stride, padding=1)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    f0 = conv("conv0_0", x, 2)
    f0 = torch.cat((f0, onehot_planes(y, num_classes, f0.shape[2], f0.dtype)), 1)
    f0 = lr(inorm(conv("conv0_1", lr(f0))))
    f1 = inorm(conv("conv1_0", f0, 2))
    f1 = lr(inorm(conv("conv1_1", lr(f1))))
    f2 = inorm(conv("conv2_0", f1, 2))
    f2 = lr(inorm(conv("conv2_1", lr(f2))))
    f3 = inorm(conv("conv3_0", f2, 2))
    f3 = inorm(conv("conv3_1", lr(f3)))
    u3 = inorm(conv("upconv3_1", lr(up(f3))))
    u3 = inorm(conv("upconv3_0", lr(u3))) + f2
    u2 = inorm(conv("upconv2_1", lr(up(u3))))
    u2 = inorm(conv("upconv2_0", lr(u2))) + f1
    u1 = inorm(conv("upconv1_1", lr(up(u2))))
    u1 = inorm(conv("upconv1_0", lr(u1))) + f0
    u0 = inorm(conv("upconv0_1", lr(up(u1))))
    return torch.tanh(conv("upconv0_0", lr(u0)))


def stored_image(x):
    """The image as a generator's input buffer holds it (include/combat_hip.h, "images entering a network";
    combat_image_to_c8): channels hi = bf16(x) and lo = bf16(x - hi), which conv0_0 reads through duplicated bf16 weights,
    i.e. as the fp32 value hi + lo -- x to 16 significant bits, not to 24."""
    hi = x.to(bf16).float()
    return hi + (x - hi).to(bf16).float()


def cunet_forward_emu(p, x, y, num_classes, taps=None, force=None):
    """bf16_emu.unet_forward_emu with CUnetEngine's conv0_1: the bf16 operand of W_f = weight[:, :nf] over
    bf16(lrelu(t00)), plus cond = bf16(conv(one-hot planes, fp32 W_y)) (combat_cond_fwd sums fp32 weights and rounds
    once), the sum rounded to bf16 when stored.

    The input is taken as the engine stores it (stored_image): like every other bf16 tensor of the dataflow.  It matters:
    the UNet's 2 x 2 and 4 x 4 InstanceNorms make its output chaotic in the last bits of its input -- at the golden point
    of tests/test_multilabel_gpu.py this emulation moves by 3.4e-2 (relative L2 of the output) when fp32 x is replaced by
    hi + lo, and by 1.4e-2 .. 2.0e-2 under a relative perturbation of 1e-7 (measured on the CPU) -- so an emulation fed
    the unrounded image is compared with the engine across a difference the engine does not have."""
    if E.ROUND:
        x = stored_image(x)
    f, q = force, E.q
    nf = p["conv0_0.weight"].shape[0]
    lr = lambda t: F.leaky_relu(t, 0.2)
    inorm = lambda t: F.instance_norm(t, eps=1e-5)

    def conv(name, t, stride=1, bias=False):
        return F.conv2d(t, E.qw(p, name + ".weight"), p[name + ".bias"] if bias else None, stride=stride, padding=1)

    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    t00 = q(conv("conv0_0", x, 2, True), f, "t.conv0_0")
    w01 = p["conv0_1.weight"]
    cond = q(F.conv2d(onehot_planes(y, num_classes, t00.shape[2]), w01[:, nf:], padding=1))
    t01 = q(F.conv2d(q(lr(t00)), q(w01[:, :nf]), padding=1) + cond, f, "t.conv0_1")
    t10 = q(conv("conv1_0", q(lr(inorm(t01))), 2), f, "t.conv1_0")
    t11 = q(conv("conv1_1", q(lr(inorm(t10)))), f, "t.conv1_1")
    t20 = q(conv("conv2_0", q(lr(inorm(t11))), 2), f, "t.conv2_0")
    t21 = q(conv("conv2_1", q(lr(inorm(t20)))), f, "t.conv2_1")
    t30 = q(conv("conv3_0", q(lr(inorm(t21))), 2), f, "t.conv3_0")
    t31 = q(conv("conv3_1", q(lr(inorm(t30)))), f, "t.conv3_1")
    u3 = q(lr(up(inorm(t31))), f, "up3")
    tu31 = q(conv("upconv3_1", u3), f, "t.upconv3_1")
    tu30 = q(conv("upconv3_0", q(lr(inorm(tu31)))), f, "t.upconv3_0")
    u2 = q(lr(up(inorm(tu30) + lr(inorm(t21)))), f, "up2")
    tu21 = q(conv("upconv2_1", u2), f, "t.upconv2_1")
    tu20 = q(conv("upconv2_0", q(lr(inorm(tu21)))), f, "t.upconv2_0")
    u1 = q(lr(up(inorm(tu20) + lr(inorm(t11)))), f, "up1")
    tu11 = q(conv("upconv1_1", u1), f, "t.upconv1_1")
    tu10 = q(conv("upconv1_0", q(lr(inorm(tu11)))), f, "t.upconv1_0")
    u0 = q(lr(up(inorm(tu10) + lr(inorm(t01)))), f, "up0")
    tu01 = q(conv("upconv0_1", u0), f, "t.upconv0_1")
    if taps is not None:
        taps.update({"conv0_0": t00, "conv0_1": t01, "conv1_0": t10, "conv1_1": t11, "conv2_0": t20, "conv2_1": t21,
                     "conv3_0": t30, "conv3_1": t31, "upconv3_1": tu31, "upconv3_0": tu30, "upconv2_1": tu21,
                     "upconv2_0": tu20, "upconv1_1": tu11, "upconv1_0": tu10, "upconv0_1": tu01})
    return q(torch.tanh(conv("upconv0_0", q(lr(inorm(tu01))), 1, True)), f, "noise")


# ---------------------------------------------------------------- the kernels' own order


def border_class(s):
    """[s] int: 0 for index 0, 2 for index s - 1, 1 between (s >= 2)."""
    c = torch.ones(s, dtype=torch.long)
    c[0], c[s - 1] = 0, 2
    return c


def tap_inside(r, yr):
    return not (r == 0 and yr == 0) and not (r == 2 and yr == 2)


def region_taps(k):
    """The taps (3 r + s) inside the map on region k = 3 yr + xr, ascending."""
    yr, xr = divmod(k, 3)
    return [3 * r + s for r in range(3) for s in range(3) if tap_inside(r, yr) and tap_inside(s, xr)]


def tap_regions(tap):
    r, s = divmod(tap, 3)
    return [k for k in range(9) if tap_inside(r, k // 3) and tap_inside(s, k % 3)]


def physical(w):
    """OIHW [K][C][3][3] -> the flat parameter buffer's [K][9][C], contiguous."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous()


def cond_ref(w, labels, s):
    """combat_cond_fwd: w fp32 [nf][9][nf + classes] -> bf16 [n][s][s][nf]."""
    nf = w.shape[0]
    classes = w.shape[2] - nf
    wy = w[:, :, nf:].float()                                   # [o][tap][c]
    table = torch.zeros(9, classes + 1, nf, dtype=bf16)         # (row `classes`: a label outside the range)
    for k in range(9):
        acc = torch.zeros(classes, nf, dtype=torch.float32)
        for tap in region_taps(k):
            acc = acc + wy[:, tap, :].t()
        table[k, :classes] = acc.to(bf16)
    bc = border_class(s)
    region = (bc[:, None] * 3 + bc[None, :])                    # [s][s]
    lab = labels.long().clone()
    lab[(lab < 0) | (lab >= classes)] = classes
    return table[region[None, :, :], lab[:, None, None]]        # [n][s][s][nf]


def cond_taps_ref(d):
    """Stage 1 of combat_cond_wgrad: d bf16 [n][s][s][nf] -> fp32 [n][9][nf] in the kernel's order."""
    n, s, _, nf = d.shape
    P, G = s * s, nf // 8
    L = 256 // G
    bc = border_class(s)
    rid = (bc[:, None] * 3 + bc[None, :]).reshape(P)
    x = d.float().reshape(n, P, nf)
    steps = (P + L - 1) // L
    zero = torch.zeros((), dtype=torch.float32)
    region = []
    for k in range(9):
        m = torch.where((rid == k)[None, :, None], x, zero)
        m = torch.cat([m, torch.zeros(n, steps * L - P, nf)], 1).reshape(n, steps, L, nf)
        lane = torch.zeros(n, L, nf)
        for i in range(steps):
            lane = lane + m[:, i]
        acc = torch.zeros(n, nf)
        for l in range(L):
            acc = acc + lane[:, l]
        region.append(acc)
    taps = torch.zeros(n, 9, nf)
    for tap in range(9):
        ks = tap_regions(tap)
        acc = region[ks[0]]
        for k in ks[1:]:
            acc = acc + region[k]
        taps[:, tap] = acc
    return taps


def cond_wgrad_ref(d, labels, classes, dwf=None):
    """combat_cond_wgrad: fp32 [nf][9][nf + classes]; input channels < nf are dwf's (zeros without it)."""
    n, _, _, nf = d.shape
    taps = cond_taps_ref(d)
    dw = torch.zeros(nf, 9, nf + classes)
    for c in range(classes):
        acc = torch.zeros(9, nf)
        for i in range(n):
            if int(labels[i]) == c:
                acc = acc + taps[i]
        dw[:, :, nf + c] = acc.t()
    if dwf is not None:
        dw[:, :, :nf] = dwf.reshape(nf, 9, nf)
    return dw


def cond_planes_f64(wy, labels, s):
    """fp64 F.conv2d of the explicit one-hot planes with W_y (OIHW [nf][classes][3][3]) -> NCHW [n][nf][s][s]."""
    return F.conv2d(onehot_planes(labels, wy.shape[1], s, torch.float64), wy.double(), padding=1)


# ---------------------------------------------------------------- grouped trigger


def blur_matrix(k1, hw):
    """[hw][hw] matrix of the reflect-padded 3-tap blur: out[i] = k1[0] in[r(i-1)] + k1[1] in[i] + k1[2] in[r(i+1)]."""
    m = torch.zeros(hw, hw, dtype=k1.dtype)
    for i in range(hw):
        m[i, i - 1 if i > 0 else 1] += k1[0]
        m[i, i] += k1[1]
        m[i, i + 1 if i + 1 < hw else hw - 2] += k1[2]
    return m


def _group_blur(k1, n, ps, hw):
    """[n][1][hw][hw]: the blur matrix of image i is that of kernel k1[i // ps]."""
    return torch.stack([blur_matrix(k1[i // ps], hw) for i in range(n)])[:, None]


def trigger_groups_ref(x, noise, pm, k1, ps, rate):
    """combat_trigger_groups_fwd as dense fp32 products (include/combat_hip.h): out = Kb_i clamp(x + rate P N P^T) Kb_i^T
    with Kb_i from k1[i // ps]; returns (out, mse_partial [3n])."""
    n, _, hw, _ = x.shape
    kb = _group_blur(k1, n, ps, hw)
    bd = torch.clamp(x + rate * (pm @ noise @ pm.t()), -1, 1)
    out = kb @ bd @ kb.transpose(-1, -2)
    return out, ((out - x) ** 2).sum((2, 3)).reshape(-1)


def trigger_groups_bwd_ref(x, noise, pm, k1, ps, rate, d_out, out, l2_scale, pre_tanh):
    """combat_trigger_groups_bwd: d_noise = rate P (mask .* (Kb_i^T (d_out + 2 l2_scale (out - x)) Kb_i)) P^T, times
    (1 - noise^2) with pre_tanh."""
    n, _, hw, _ = x.shape
    kb = _group_blur(k1, n, ps, hw)
    g = kb.transpose(-1, -2) @ (d_out + 2 * l2_scale * (out - x)) @ kb
    pre = x + rate * (pm @ noise @ pm.t())
    g = torch.where((pre >= -1) & (pre <= 1), g * rate, torch.zeros_like(g))
    d = pm.t() @ g @ pm
    return d * (1 - noise * noise) if pre_tanh else d


# ---------------------------------------------------------------- chunk arithmetic


def chunk_size(bs, num_classes):
    """ps of train_generator_multilabel.py:203."""
    return int((bs - 1) / num_classes) + 1


def chunk_bounds(bs, num_classes):
    """[(class, start, end)] of the generator phase: a literal transcription of train_generator_multilabel.py:203-213."""
    ps = int((bs - 1) / num_classes) + 1
    out = []
    for ci in range(num_classes):
        si = ci * ps
        ei = si + ps
        if ei > bs:
            ei = bs
        if si >= ei:
            break
        out.append((ci, si, ei))
    return out


# ---------------------------------------------------------------- one step


class Randomness:
    """Draws of one multi-label step, in the reference's order (train_generator_multilabel.py): num_bd (:171, numpy),
    sigma_c (:176, skipped when num_bd == 0), aug0 (:179), aug1 (:190), aug2 (:199, pred_clean's transform: BEFORE the
    chunks' blur draws), one sigma per chunk (:217), aug3 (:225), aug4 (:236)."""

    def __init__(self, num_bd, sigma_c, sigma_g, aug=None):
        self.num_bd, self.sigma_c, self.sigma_g = int(num_bd), float(sigma_c), [float(v) for v in sigma_g]
        self.aug = list(aug) if aug is not None else [None] * 5


def multilabel_step(netc, netg, clean, netf, bufs_c, bufs_g, inputs, targets, rnd, cfg, clf_fn=None, gen_fn=None):
    """One step of train_generator_multilabel.py:160-242 composed of oracle.combat_oracle's pieces.  Updates netc / netg
    (parameters, BN statistics, momentum buffers) in place; returns the step's scalars.  cfg.lr_g is the generator's
    rate (the reference's lr_C * 0.1, :115).  gen_fn(p, x, y)."""
    from oracle import combat_oracle as O
    clf = clf_fn or O._classifier(cfg)
    gen = gen_fn or (lambda p, x, y: cunet_forward(p, x, y, cfg.num_classes))
    tr = O.post_tensor_transform
    mix = lambda x, noise, s: O.trigger_mix(x, noise, cfg.noise_rate, cfg.ratio, s, cfg.kernel_size)
    names_c, names_g = O.trainable_names(netc), O.trainable_names(netg)
    for d in (netc, netg, clean):
        for k in O.trainable_names(d):
            d[k].requires_grad_(True)
            d[k].grad = None
    bs, nb = inputs.shape[0], rnd.num_bd

    # ---- Phase C (:164-190): the first num_bd images, conditioned on their own labels; targets unchanged
    to_change = inputs[:nb]
    inputs_bd = mix(to_change, gen(netg, to_change, targets[:nb]), rnd.sigma_c) if nb else to_change
    total_inputs = tr(torch.cat([inputs_bd, inputs[nb:]], dim=0), rnd.aug[0])
    loss_c = F.cross_entropy(clf(netc, total_inputs, True), targets)
    grads = O._grads(loss_c, [netc[k] for k in names_c], False)
    gnorm_c = float(torch.sqrt(sum((t.double() ** 2).sum() for t in grads)))
    O.sgd_nesterov_step([netc[k] for k in names_c], grads, bufs_c, cfg.lr_c)
    with torch.no_grad():
        clean_preds = clf(clean, tr(inputs, rnd.aug[1]), False)

    # ---- Phase G (:192-242)
    with torch.no_grad():
        pred_clean = clf(netc, tr(inputs, rnd.aug[2]), False)
    bds, tmps = [], []
    for ci, si, ei in chunk_bounds(bs, cfg.num_classes):
        tmp = targets[si:ei] * 0 + ci
        bds.append(mix(inputs[si:ei], gen(netg, inputs[si:ei], tmp), rnd.sigma_g[ci]))
        tmps.append(tmp)
    bd, tmp = torch.cat(bds, 0), torch.cat(tmps, 0)
    pred_bd = clf(netc, tr(bd, rnd.aug[3]), False)
    loss_ce = F.cross_entropy(pred_bd, tmp)
    loss_l2 = F.mse_loss(bd, inputs)
    f_correct = 0
    if netf is not None:
        with torch.no_grad():
            f_correct = int((O.frequency_model_forward(netf, O.frequency_input(bd)).argmax(1) == 1).sum())
    clean_model_preds = clf(clean, tr(bd, rnd.aug[4]), False)
    clean_model_loss = F.cross_entropy(clean_model_preds, targets)
    loss = loss_ce + cfg.l2_weight * loss_l2 + cfg.clean_model_weight * clean_model_loss      # (:240: no gradient-L2 term)
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
        "clean_model_loss": float(clean_model_loss.detach()), "loss_g": float(loss.detach()), "gnorm_c": gnorm_c,
        "gnorm_g": gnorm_g, "bd_sum": float(bd.detach().double().sum()),
        "clean_correct": int((pred_clean.argmax(1) == targets).sum()),
        "bd_correct": int((pred_bd.argmax(1) == tmp).sum()),
        "f_correct": f_correct,
        "clean_model_correct": int((clean_preds.argmax(1) == targets).sum()),
        "clean_model_bd_ba": int((clean_model_preds.argmax(1) == targets).sum()),
        "clean_model_bd_asr": int((clean_model_preds.argmax(1) == tmp).sum()),
    }
