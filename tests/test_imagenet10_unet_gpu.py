"""The UNet-trigger attack at ImageNet-10's shape (3 x 224 x 224, 10 classes, ResNet18(input_size=224), batch 32) on the
MI355X: the generator engine at hw = 224, the alternated step and the four entry scripts.

The reference cannot run this configuration (its input_size2scaler table has no 224 entry: SURVEY D4), so, as for the
WaNet trigger at this shape (tests/test_wanet_gpu.py::test_wanet_step_imagenet10_shape), parity is "unpinned" against
the reference: the checks are against the CPU oracle and the size-generic modules, with the methods and tolerances of
the 32 x 32 and 64 x 64 tests."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402
from test_engine_gpu import Opt, _oracle_state, flat_grads, rel_l2, seeded, stored  # noqa: E402
from test_oracle_golden import synth_images  # noqa: E402

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what UnetEngine's forward and backward plans record at hw = 32, n = 2, on the commit before the 224 x 224 work
PLAN_NAMES_HW32 = (
    "conv0_0 conv0_1.conv conv0_1.finact conv1_0.conv conv1_0.finact conv1_1.conv conv1_1.finact conv2_0.conv "
    "conv2_0.finact conv2_1.conv conv2_1.finact conv3_0.conv conv3_0.finact conv3_1.conv up3.fin upconv3_1.conv "
    "upconv3_1.finact upconv3_0.conv up2.fin upconv2_1.conv upconv2_1.finact upconv2_0.conv up1.fin upconv1_1.conv "
    "upconv1_1.finact upconv1_0.conv up0.fin upconv0_1.conv upconv0_1.finalize upconv0_0",
    "zero_grad g.upconv0_1.dgrad db.upconv0_0 upconv0_0.wgrad g.upconv0_1.bfused upconv0_1.wgrad upconv0_1.dgrad up0.bwd "
    "g.upconv1_0.bfused upconv1_0.wgrad g.upconv1_1.dgrad g.upconv1_1.bfused upconv1_1.wgrad upconv1_1.dgrad up1.bwd.norm "
    "upconv2_0.wgrad g.upconv2_1.dgrad g.upconv2_1.bfused upconv2_1.wgrad upconv2_1.dgrad up2.bwd.norm upconv3_0.wgrad "
    "g.upconv3_1.dgrad g.upconv3_1.bfused upconv3_1.wgrad upconv3_1.dgrad up3.bwd.norm conv3_1.wgrad g.conv3_0.dgrad "
    "g.conv3_0.bfused conv3_0.wgrad g.conv2_1.dgrad g.conv2_1.bfused conv2_1.wgrad g.conv2_0.dgrad g.conv2_0.bfused "
    "conv2_0.wgrad g.conv1_1.dgrad g.conv1_1.bfused conv1_1.wgrad g.conv1_0.dgrad g.conv1_0.bfused conv1_0.wgrad "
    "g.conv0_1.dgrad g.conv0_1.bfused conv0_1.wgrad conv0_1.dgrad db.conv0_0 conv0_0.wgrad")


def test_unet_plan_names_unchanged_at_hw32():
    """The launches recorded for 32 x 32 images are those of the parent commit (the 224 x 224 routes add none)."""
    from combat_amd import nets
    eng = seeded(lambda: nets.UnetGenerator(None), 3).cuda()._net_engine()
    slot = eng.slot("names", 2, 32)
    got = tuple(" ".join(c.what for c in p.calls) for p in (eng.forward_plan(slot), eng.backward_plan(slot)))
    assert got == PLAN_NAMES_HW32


def test_unet_engine_224():
    """UnetEngine at hw = 224 (maps 112 / 56 / 28 / 14), n = 2, with the method and bounds of
    tests/test_engine_gpu.py::test_unet_forward_backward; the fp32 reference is the generator's fp32 forward
    (oracle.unet_forward on the module's state dict) and its autograd gradients.

    Measured on the CPU at this test point: the bf16 emulation is 1.76e-2 (forward) and 0.176 (parameter gradients,
    rel-L2 over all of them) from fp32; the bounds are the existing ones (forward 5e-2 and 1.25 x emulation + 1e-3,
    gradients 0.5 and 1.6 x emulation), with the emulation's distance taken in the test itself."""
    from combat_amd import nets, ops
    from oracle import combat_oracle as O
    hw, n = 224, 2
    m = seeded(lambda: nets.UnetGenerator(None), 7)
    names = [k for k, _ in m.named_parameters()]
    g = torch.Generator().manual_seed(230)
    x = torch.rand(n, 3, hw, hw, generator=g) * 2 - 1
    cot = torch.randn(n, 3, hw, hw, generator=g)

    def run(fwd, **kw):
        p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
        y = fwd(p, x, **kw)
        gr = torch.autograd.grad(y, [p[k] for k in names], cot, allow_unused=True)
        return y.detach(), torch.cat([(torch.zeros_like(p[k]) if a is None else a).reshape(-1) for k, a in zip(names, gr)])

    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    y_ref, g_ref = run(O.unet_forward)
    taps = {}
    y_emu, g_emu = run(E.unet_forward_emu, taps=taps)
    m = m.cuda()
    eng = m._net_engine()
    eng.refresh()
    slot = eng.slot("t224", n, hw)
    ops.image_to_c8(x.cuda(), eng.input(slot))
    eng.forward_plan(slot).run()
    y = eng.output(slot)[..., :3].float().permute(0, 3, 1, 2)
    errs = {k: rel_l2(slot.bufs["t." + k].float().permute(0, 3, 1, 2), v.detach()) for k, v in taps.items()}
    e_fp32, emu_fp32 = rel_l2(y, y_ref), rel_l2(y_emu, y_ref)
    print("layers", {k: "%.2g" % v for k, v in errs.items()}, "forward vs emulation %.3g, vs fp32 %.3g (emulation %.3g)"
          % (rel_l2(y, y_emu), e_fp32, emu_fp32))
    assert errs["conv0_0"] < 1e-3 and errs["conv0_1"] < 3e-3 and errs["conv1_0"] < 5e-3, errs
    assert max(errs.values()) < 4e-2, errs
    assert rel_l2(y, y_emu) < 3e-2, errs
    assert e_fp32 < 5e-2 and e_fp32 < 1.25 * emu_fp32 + 1e-3, (e_fp32, emu_fp32)
    z = slot.buf("g.z", (n, hw, hw, 8))
    z.zero_()
    z[..., :3] = (cot.cuda() * (1 - y * y)).permute(0, 2, 3, 1).to(bf16)
    eng.backward_plan(slot).run()
    torch.cuda.synchronize()
    ours = flat_grads(eng.fp, names)
    assert bool(torch.isfinite(ours).all())
    force = stored(slot, ["t." + k for k in taps] + ["up0", "up1", "up2", "up3", "noise"], 3)
    _, g_tf = run(E.unet_forward_emu, force=force)
    e_tf, e_fp32, emu_fp32 = rel_l2(ours, g_tf), rel_l2(ours, g_ref), rel_l2(g_emu, g_ref)
    print("gradients vs teacher-forced emulation %.3g, vs fp32 %.3g (emulation %.3g)" % (e_tf, e_fp32, emu_fp32))
    assert e_tf < 4e-2, e_tf                                      # vs teacher-forced emulation
    assert e_fp32 < 0.5 and e_fp32 < 1.6 * emu_fp32, (e_fp32, emu_fp32)


def _opt224():
    opt = Opt()
    opt.num_classes, opt.input_height, opt.input_width, opt.dataset = 10, 224, 224, "imagenet10"
    return opt


def _nets224():
    from combat_amd import nets
    mk = lambda: nets.ResNet18(num_classes=10, input_size=224)
    return (seeded(mk, 1), seeded(mk, 2), seeded(lambda: nets.UnetGenerator(None), 3),
            seeded(lambda: nets.FrequencyModel(2, 3, 224), 4).eval())


def test_alternated_step_imagenet10_shape_b4():
    """One alternated UNet step at 3 x 224 x 224, 10 classes, ResNet18(input_size=224), b = 4, against the CPU oracle
    driven with the bf16-emulating networks; method and tolerances of test_wanet_step_imagenet10_shape, with the
    generator's part as in test_alternated_step_celeba_shape_resnet18: Phase C from the identical start state (loss
    1e-2, gradient norm 3e-2), Phase G from the engine's own post-Phase-C classifier with the generator emulation
    teacher-forced (triggered images 3e-5, losses 1e-2 * max(1, |ref|), loss_l2 1e-3, counters +-1, image gradient
    0.25, generator gradient 5e-2)."""
    from combat_amd import nets, step as step_mod
    from oracle import combat_oracle as O
    b = 4
    netc, clean, netg, netf = _nets224()
    oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
    old_g = _oracle_state(netg)
    x = synth_images(b, 224, 5)
    t = torch.randint(0, 10, (b,), generator=torch.Generator().manual_seed(6))
    t[::2][:2] = 0
    nb, sc, sg = 1, 0.5, 0.9
    cfg = O.StepConfig(num_classes=10, classifier="resnet18")
    ref = O.alternated_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)), x, t,
                            O.StepRandomness(nb, sc, sg, [None] * 5), cfg, clf_fn=E.resnet_forward_emu,
                            gen_fn=E.unet_forward_emu)
    st = step_mod.AlternatedStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _opt224())
    st.keep_grads = True
    st.run(x.cuda(), t, step_mod.StepRandomness(nb, sc, sg, [None] * 5))
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    tol = lambda r: 1e-2 * max(1.0, abs(r))
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"]), (m["loss_c_sum"], ref["loss_c"])
    gn_c = float(st.eC.fp.grad.double().norm())
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G from the engine's post-Phase-C classifier, the generator emulation teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    names_g = O.trainable_names(old_g)
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + n for n, *_ in nets.UNET_LAYERS] + ["up0", "up1", "up2", "up3", "noise"]
    noise = E.unet_forward_emu(pg, x, force=stored(st.sG, keys, 3))
    ibd = O.trigger_mix(x, noise, 0.08, 0.65, sg)
    assert float((st.bd.cpu() - ibd.detach()).abs().max()) < 3e-5
    bd_t = torch.zeros_like(t)
    leaf = ibd.detach().clone().requires_grad_(True)
    pred_bd = E.resnet_forward_emu(oc2, leaf, False)
    cm_pred = E.resnet_forward_emu(ok, leaf, False)
    loss_ce, cm_loss = F.cross_entropy(pred_bd, bd_t), F.cross_entropy(cm_pred, t)
    assert abs(m["loss_ce_sum"] - float(loss_ce.detach())) < tol(float(loss_ce.detach())), (m["loss_ce_sum"], float(loss_ce.detach()))
    assert abs(m["clean_model_loss_sum"] - float(cm_loss.detach())) < tol(float(cm_loss.detach()))
    l2 = float(F.mse_loss(ibd.detach(), x))
    assert abs(m["loss_l2_sum"] - l2) < 1e-3 * l2 + 1e-7
    assert abs(m["bd_correct"] - int((pred_bd.argmax(1) == bd_t).sum())) <= 1
    assert abs(m["clean_model_bd_ba"] - int((cm_pred.argmax(1) == t).sum())) <= 1
    assert abs(m["clean_model_bd_asr"] - int((cm_pred.argmax(1) == bd_t).sum())) <= 1
    (d_bd,) = torch.autograd.grad(loss_ce + 0.8 * cm_loss, leaf)
    assert rel_l2((st.d_bd + st.d_bd2).cpu(), d_bd) < 0.25            # un-forced classifiers: mask-flip bound
    # (the detector's hit count is not compared: the oracle's triggered images come from its own, un-forced generator,
    # and the untrained detector decides on them by margins smaller than that difference)
    total = (ibd * (st.d_bd + st.d_bd2).cpu()).sum() + 0.02 * F.mse_loss(ibd, x)
    gr = torch.autograd.grad(total, [pg[k] for k in names_g], allow_unused=True)
    gr = torch.cat([(torch.zeros_like(pg[k]) if a is None else a).reshape(-1) for k, a in zip(names_g, gr)])
    e_g = rel_l2(flat_grads(st.eG.fp, names_g), gr)
    print("generator gradient vs teacher-forced emulation %.3g" % e_g)
    assert e_g < 5e-2    # teacher-forced: pins the strip trigger backward + the UNet backward at 224 x 224


def test_alternated_step_imagenet10_shape_b32():
    """The configuration's batch of 32 (train_generator.py:480-485): one step, finite metrics, and the triggered images
    within 2e-5 of oracle.trigger_mix applied to the engine's own generator output."""
    from combat_amd import step as step_mod
    from oracle import combat_oracle as O
    b, sg = 32, 0.9
    netc, clean, netg, netf = _nets224()
    x = synth_images(b, 224, 5)
    t = torch.randint(0, 10, (b,), generator=torch.Generator().manual_seed(6))
    st = step_mod.AlternatedStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _opt224())
    st.run(x.cuda(), t, step_mod.StepRandomness(3, 0.5, sg, [None] * 5))
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    noise = st.eG.output(st.sG)[..., :3].float().cpu().permute(0, 3, 1, 2)
    assert bool(torch.isfinite(noise).all())
    ibd = O.trigger_mix(x, noise, 0.08, 0.65, sg)
    assert float((st.bd.cpu() - ibd).abs().max()) < 2e-5
    assert all(bool(torch.isfinite(p).all()) for p in list(netg.parameters()) + list(netc.parameters()))


def _script(script, *args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--dataset", "imagenet10", "--synthetic_size", "64",
           "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1", "--n_iters", "1"] + list(args)
    r = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_imagenet10_workflow_on_synthetic_data(tmp_path):
    """train_clean_classifier -> train_generator -> train_victim -> eval with --dataset imagenet10 (224 x 224, 10
    classes, ResNet18(input_size=224) surrogate and clean model, bs forced to 32; no detector checkpoint ships for this
    data set, so --allow_missing_F as for train_generator_wanet.py): checkpoint keys as for CIFAR-10."""
    cwd = str(tmp_path)
    ck = lambda mode: os.path.join(cwd, "ckpt", mode, "imagenet10", "imagenet10_%s.pth.tar" % mode)
    finite = lambda sd: all(bool(torch.isfinite(v.float()).all()) for v in sd.values())
    _script("train_clean_classifier.py", "--saving_prefix", "classifier_clean", cwd=cwd)
    sd = torch.load(ck("classifier_clean"), map_location="cpu", weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "best_clean_acc", "epoch_current"}
    assert len(sd["netC"]) == 122 and sd["netC"]["linear.weight"].shape == (10, 512 * 49) and finite(sd["netC"])
    out = _script("train_generator.py", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "classifier_clean", cwd=cwd)
    assert "Clean Acc:" in out and "Saving..." in out
    sd = torch.load(ck("train_generator_clean"), map_location="cpu", weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model",
                       "best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
                       "best_clean_model_bd_asr", "epoch_current"}
    assert len(sd["netG"]) == 32 and len(sd["netC"]) == 122 and sd["netC"]["linear.weight"].shape == (10, 512 * 49)
    assert finite(sd["netG"]) and finite(sd["netC"]) and finite(sd["clean_model"])
    _script("train_victim.py", "--saving_prefix", "train_victim", "--load_checkpoint", "train_generator_clean", cwd=cwd)
    sd = torch.load(ck("train_victim"), map_location="cpu", weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "epoch_current"}
    assert sd["netC"]["linear.weight"].shape == (10, 512 * 49) and finite(sd["netC"]) and finite(sd["netG"])
    out = _script("eval.py", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "train_victim",
                  "--load_checkpoint", "train_generator_clean", cwd=cwd)
    assert "Bd ASR:" in out
