"""The VGG13 victim on the MI355X: engine passes against tests/vgg13_ref.py's bf16 emulation (teacher-forced for the
gradients) and the fp32 goldens of the reference module, the victim step (ClassifierStep), deterministic mode, and the
three entry scripts with --model vgg13.  Bound forms and numbers are tests/test_engine_gpu.py::test_resnet18_train_eval's
(see that module's docstring) unless a comment says otherwise."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vgg13_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.asarray(a))
BUFS = ["l%d.%s" % (l, s) for l in range(10) for s in ("y", "a")]


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def make(case):
    from combat_amd import nets
    c = R.CASES[case]
    torch.manual_seed(R.SEED_NET)
    return nets.VGG("VGG13", num_classes=c["classes"], n_input=3, input_size=c["hw"])


def stored(slot, names=BUFS):
    return {k: slot.bufs[k].float().cpu().permute(0, 3, 1, 2).contiguous() for k in names if k in slot.bufs}


def is_conv_bias(k):
    return k.startswith("features.") and k.endswith(".bias") and int(k.split(".")[1]) in R.CONV_IDX


def sampled_err(g, prefix, named):
    num = den = 0.0
    for k, v in named:
        if is_conv_bias(k):     # the reference's values there are rounding noise around zero
            continue
        idx, ref = g["%s/%s/idx" % (prefix, k)], g["%s/%s/val" % (prefix, k)]
        d = v.double().flatten()[idx].numpy() - ref
        num, den = num + float((d ** 2).sum()), den + float((ref ** 2).sum())
    return (num / max(den, 1e-30)) ** 0.5


def state(m):
    p = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for k, _ in m.named_parameters():
        p[k].requires_grad_(True)
    return p


def engine_input(eng, slot):
    """The fp32 NCHW images the classifier saw: hi + lo of the c8 input buffer."""
    x = eng.input(slot).float()
    return (x[..., :3] + x[..., 3:6]).permute(0, 3, 1, 2).contiguous().cpu()


@pytest.mark.parametrize("hw", [32, 64])
def test_vgg13_train_eval(hw, golden):
    from combat_amd import ops
    g = golden("vgg13")
    case = "c%d" % hw
    m = make(case)
    names = [k for k, _ in m.named_parameters()]
    wnames = [k for k in names if not is_conv_bias(k)]
    pe = state(m)
    m = m.cuda()
    eng = m._net_engine()
    eng.refresh()
    x, t = R.batch(case, 0)
    pe_before = {k: v.clone() for k, v in pe.items() if "running" in k or "num_batches" in k}
    lg_e, loss_e, gr_e = R.loss_and_grads(pe, names, R.engine_image(x), t, True, emu=True)
    slot = eng.slot("train", R.N, hw)
    ops.image_to_c8(x.cuda(), eng.input(slot))
    h = eng.head_bufs(slot)
    h["targets"].copy_(t.cuda())
    h["loss"].zero_()
    h["correct"].zero_()
    eng.forward_plan(slot, True).run()
    torch.cuda.synchronize()
    print(case, "train logits vs emu %.3g, vs fp32 %.3g (emu vs fp32 %.3g)" % (
        rel_l2(h["logits"], lg_e), rel_l2(h["logits"], T(g[case + "/train/logits"])), rel_l2(lg_e, T(g[case + "/train/logits"]))))
    # The emulation starts from the image as the engine's first convolution reads it (vgg13_ref.engine_image): with the plain
    # fp32 image its 64 x 64 loss sat 6.8e-3 from the engine's, 4.3e-3 of that from this one rounding point.
    # Two of test_resnet18_train_eval's numbers are too tight for the EMULATION itself here (ten BatchNorms in a chain, the
    # last over 64 values per channel at 32 x 32): there the bound is its own error against the fp32 golden, computed here on
    # the CPU, x 1.6 -- measured: logits 2.8e-2 (32 x 32) / 3.1e-2 (64 x 64), running_mean of the last BatchNorm 5.1e-3 /
    # 3.0e-3; never below the ResNet numbers.  The loss keeps the ResNet numbers (emulation against fp32: 2.4e-3 / 0.8e-3).
    emu_logits = rel_l2(lg_e, T(g[case + "/train/logits"]))
    assert rel_l2(h["logits"], lg_e) < 2e-2                                       # vs emulation
    print(case, "train loss: engine - emu %.3g, engine - fp32 %.3g, emu - fp32 %.3g" % (
        float(h["loss"]) - float(loss_e), float(h["loss"]) - float(g[case + "/train/loss"]), float(loss_e) - float(g[case + "/train/loss"])))
    assert abs(float(h["loss"]) - float(loss_e)) < 5e-3
    assert rel_l2(h["logits"], T(g[case + "/train/logits"])) < max(3e-2, 1.6 * emu_logits)   # vs fp32
    assert abs(float(h["loss"]) - float(g[case + "/train/loss"])) < 1e-2
    pf = dict(pe)
    pf.update({k: v.clone() for k, v in pe_before.items()})
    lg_f, _, gr_f = R.loss_and_grads(pf, names, R.engine_image(x), t, True, emu=True, force=stored(slot))
    assert rel_l2(h["logits"], lg_f) < 2e-3
    eng.backward_train_plan(slot).run()
    torch.cuda.synchronize()
    fp = eng.fp
    ours = {k: fp.logical(fp.grad, k).float().cpu() for k in names}
    e_tf = rel_l2(torch.cat([ours[k].reshape(-1) for k in wnames]), torch.cat([a.reshape(-1) for k, a in zip(names, gr_f) if k in wnames]))
    e = sampled_err(g, case + "/train/gp", [(k, ours[k]) for k in names])
    emu = sampled_err(g, case + "/train/gp", zip(names, gr_e))
    print(case, "gradients vs teacher-forced %.3g, vs fp32 %.3g (emu vs fp32 %.3g)" % (e_tf, e, emu))
    assert e_tf < 4e-2, e_tf                                                      # vs teacher-forced
    assert e < 0.5 and e < 1.6 * emu, (e, emu)                                    # vs fp32
    for k in names:
        if is_conv_bias(k):
            assert float(ours[k].abs().max()) == 0.0, k                           # exactly zero
    for k, v in m.state_dict().items():
        if "running" in k:
            ref = T(g["%s/train/buf/%s" % (case, k)])
            assert rel_l2(v, ref) < max(5e-3, 1.6 * rel_l2(pe[k], ref)), k            # (pe: the emulation's buffers after its pass)
        if "num_batches" in k:
            assert int(v) == int(g["%s/train/buf/%s" % (case, k)])
    # eval: folded BatchNorms with non-trivial running statistics, the bias in the launch's epilogue, through module(x)
    me = R.randomize_bn_buffers(make(case), R.SEED_BN).eval()
    pev = {k: v.clone() for k, v in me.state_dict().items()}
    xe, _ = R.batch(case, 1)
    with torch.no_grad():
        lg_emu = R.forward(pev, R.engine_image(xe), False, emu=True)
        ours_e = me.cuda()(xe.cuda())
    print(case, "eval logits vs emu %.3g, vs fp32 %.3g" % (rel_l2(ours_e, lg_emu), rel_l2(ours_e, T(g[case + "/eval/logits"]))))
    assert rel_l2(ours_e, lg_emu) < 2e-2
    assert rel_l2(ours_e, T(g[case + "/eval/logits"])) < max(3e-2, 1.6 * rel_l2(lg_emu, T(g[case + "/eval/logits"])))
    with pytest.raises(NotImplementedError, match="victim-only"):
        eng.backward_eval_plan(slot, 1.0)
    with pytest.raises(NotImplementedError, match="victim-only"):
        eng.forward_plan(slot, False, 1.0, False, split_head=True)      # (a surrogate's call shapes get the message, not a TypeError)
    with pytest.raises(NotImplementedError, match="victim-only"):
        eng.forward_plan(slot, False, 1.0, True)
    assert eng.forward_plan(slot, True, 1.0, False) is eng.forward_plan(slot, True)
    with pytest.raises(ValueError, match="forward_plan"):
        eng.backward_train_plan(eng.slot("no forward yet", R.N, hw))
    with pytest.raises(ValueError, match="forward_plan"):
        eng.backward_train_plan(slot, 0.5)                              # the forward that ran left dlogits of weight 1


class Opt:
    noise_rate, ratio, kernel_size, sigma = 0.08, 0.65, 3, (0.1, 1.0)
    pc, target_label, attack_mode, num_classes = 0.5, 0, "all2one", 10
    L2_weight, clean_model_weight, lr_C, lr_G = 0.02, 0.8, 1e-2, 1e-2
    input_height = input_width = 32
    dataset, post_transform_option, random_crop, random_rotation = "cifar10", "no_use", 5, 10


@pytest.mark.parametrize("variant", ["plain", "poisoned", "no_aug"])
def test_victim_step(variant):
    """ClassifierStep with a VGG netC: without a generator (augmentation on), with a frozen seeded UnetGenerator and a
    poisoned subset, and with post_transform_option = "no_use".  The restatement is driven with the images and labels the
    step itself fed the classifier and teacher-forced with its stored tensors: gradients as in test_vgg13_train_eval, and
    the parameters after the step are the restated SGD update."""
    from combat_amd import nets, step as step_mod
    opt = Opt()
    opt.post_transform_option = "use" if variant == "plain" else "no_use"
    m = make("c32")
    names = [k for k, _ in m.named_parameters()]
    wnames = [k for k in names if not is_conv_bias(k)]
    p0 = state(m)
    m = m.cuda()
    netg = None
    if variant == "poisoned":
        torch.manual_seed(7)
        netg = nets.UnetGenerator(None).cuda().eval()
    x, t = R.batch("c32", 2)
    poisoned = None
    if netg is not None:
        poisoned = torch.zeros(R.N, dtype=torch.bool)
        poisoned[[1, 4, 5, 11]] = True
    random_state = np.random.get_state()
    np.random.seed(3)
    st = step_mod.ClassifierStep(m, opt, netg)
    st.run(x.cuda(), t, poisoned)
    np.random.set_state(random_state)
    torch.cuda.synchronize()
    eng, slot = st.eC, st.cur.slot
    h = eng.head_bufs(slot)
    x_in, t_in = engine_input(eng, slot), h["targets"].cpu()
    if variant == "no_aug":
        assert torch.equal(t_in, t) and float((x_in - x).abs().max()) < 4e-5
    if variant == "poisoned":
        assert int((t_in[:4] == 0).sum()) == 4 and float((x_in[:4] - x[[1, 4, 5, 11]]).abs().max()) > 1e-3
    lg_f, loss_f, gr_f = R.loss_and_grads(p0, names, x_in, t_in, True, emu=True, force=stored(slot))
    mt = st.read_metrics()
    assert abs(mt["loss_sum"] - float(loss_f)) < 5e-3 and abs(mt["correct"] - int((lg_f.argmax(1) == t_in).sum())) <= 1
    fp = eng.fp
    ours = {k: fp.logical(fp.grad, k).float().cpu() for k in names}
    e_tf = rel_l2(torch.cat([ours[k].reshape(-1) for k in wnames]), torch.cat([a.reshape(-1) for k, a in zip(names, gr_f) if k in wnames]))
    assert e_tf < 4e-2, e_tf
    after = {k: v.detach().cpu() for k, v in m.named_parameters()}
    num = den = 0.0
    for k, gf in zip(names, gr_f):
        mine, _ = R.sgd_nesterov(p0[k].detach(), ours[k], None, **R.SGD)          # from the engine's own gradient: exact arithmetic
        assert rel_l2(after[k], mine) < 1e-6, k
        if k in wnames:
            ref, _ = R.sgd_nesterov(p0[k].detach(), gf, None, **R.SGD)            # from the teacher-forced gradient
            num += float(((after[k] - ref).double() ** 2).sum())
            den += float(((ref - p0[k].detach()).double() ** 2).sum())
        else:   # zero gradient: weight decay alone moves a convolution bias
            assert torch.equal(mine, p0[k].detach() - 1e-2 * 1.9 * (5e-4 * p0[k].detach()))
    assert (num / den) ** 0.5 < 4e-2, (num / den) ** 0.5                          # the update inherits the gradient's bound


def _trace(steps=R.TRACE_STEPS):
    from combat_amd import step as step_mod
    m = make("c32").cuda()
    st = step_mod.ClassifierStep(m, Opt())
    out, prev = [], 0.0
    for s in range(steps):
        x, t = R.batch("c32", 2 + s % R.TRACE_POOL)
        st.run(x.cuda(), t)
        cur = st.read_metrics()["loss_sum"]
        out.append(cur - prev)
        prev = cur
    torch.cuda.synchronize()
    return np.array(out), [v.detach().clone() for v in list(m.parameters()) + list(m.buffers())]


def _ema(v, a=0.1):
    """tests/test_engine_gpu.py::_ema."""
    out, m = [], float(v[0])
    for x in v:
        m = (1 - a) * m + a * float(x)
        out.append(m)
    return np.array(out)


# The bound form of tests/test_engine_gpu.py::trajectory_check: the exponential moving average (alpha 0.1) of the loss
# within a relative distance of the reference trace's at every step.  The number: the bf16 emulation's own worst distance
# in that form, measured on the CPU with vgg13_ref.loss_trace(emu=True) against tests/golden/vgg13.npz, x 1.6.  The ten
# steps (two alternating batches, lr 1e-2, momentum 0.9; the loss climbs to 3.0, then falls 2.2 -> 1.2 -> 0.65 -> 0.11) amplify
# last-bit differences: the SAME emulation run with 1 .. 8 and 12 CPU threads (another fp32 summation order inside the
# convolutions, nothing else) lands 0.9 % (8 threads), 1.4-2.8 % (seven of the nine runs) and 4.3 % (5 threads) from the
# reference, and two fp32 evaluations already differ by 0.023 in the loss of step 7 (test_vgg13_cpu.py).  The worst of the
# nine is the emulation's error here.
EMU_TRACE_EMA_DEV = 0.0432


def test_loss_trace_follows_the_reference(golden):
    """Ten victim steps (no augmentation, no poisoning) against the loss trace of the reference module under torch's SGD,
    in deterministic mode (one reproducible run: the default form's fp32 atomics alone moved the worst step's loss by 0.12
    between two runs), and the loss comes down."""
    from combat_amd import engine
    ref = golden("vgg13")["c32/trace"]
    engine.set_deterministic(True)
    try:
        ours, _ = _trace()
    finally:
        engine.set_deterministic(False)
    dev = np.abs(_ema(ours) - _ema(ref)) / _ema(ref)
    print("vgg13 trace: ours", np.round(ours, 4).tolist(), "max relative EMA deviation %.4f (step %d)" % (dev.max(), dev.argmax()))
    assert np.all(dev <= 1.6 * EMU_TRACE_EMA_DEV), (dev, ours, ref)
    assert ours[-1] < 0.25 * ours[0]


def test_two_runs_of_the_victim_step_give_the_same_bits():
    """Deterministic mode: three steps twice from the same seed and batches, bit-identical parameters and buffers."""
    from combat_amd import engine
    engine.set_deterministic(True)
    try:
        ta, pa = _trace(3)
        tb, pb = _trace(3)
    finally:
        engine.set_deterministic(False)
    assert len(pa) == len(pb) == 72
    for u, v in zip(pa, pb):
        assert torch.equal(u, v)
    assert np.array_equal(ta, tb)


# ---------------------------------------------------------------- scripts


def run(script, *args, cwd, **env):
    """Every child is seeded (initialisation, the loader's permutation, the augmentation draws), as the other script
    tests that assert an outcome are."""
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--synthetic_size", "256", "--bs", "64", "--seed", "1",
           "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1"] + list(args)
    r = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_scripts_with_model_vgg13(tmp_path):
    from combat_amd import nets
    cwd = str(tmp_path)
    keys = [k for k, _ in make("c32").state_dict().items()]
    # seeded and in deterministic mode: ONE reproducible run.  The assertion is the issue's sentence -- the loss goes down
    # on the structured set: the last of eight epochs' mean loss below the first's -- with no margin of its own: VGG13 at
    # lr 1e-2 first climbs, so how far a short run has come down by its end is not derivable.
    out = run("train_clean_classifier.py", "--model", "vgg13", "--saving_prefix", "vgg_clean", "--synthetic_kind", "structured",
              "--synthetic_size", "512", "--n_iters", "8", cwd=cwd, COMBAT_DETERMINISTIC="1")
    losses = [float(v) for v in re.findall(r"CE Loss: ([0-9.]+)", out)]
    epochs = losses[7::8]            # 8 batches of 64 per epoch; the last line of an epoch is its running mean / 64
    print("vgg13 clean classifier, CE loss per epoch:", [round(64 * v, 3) for v in epochs])
    assert len(losses) == 64 and epochs[-1] < epochs[0], epochs
    sd = torch.load(os.path.join(cwd, "ckpt", "vgg_clean", "cifar10", "cifar10_vgg_clean.pth.tar"), map_location="cpu",
                    weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "best_clean_acc", "epoch_current"} and list(sd["netC"]) == keys
    nets.VGG("VGG13").load_state_dict(sd["netC"], strict=True)
    assert all(torch.isfinite(v.float()).all() for v in sd["netC"].values())
    # the generator comes from the default surrogate's run; the victim and its evaluation are VGG13
    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", "--n_iters", "1", "--max_steps", "2", cwd=cwd)
    run("train_generator.py", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "classifier_clean", "--n_iters", "1",
        "--max_steps", "2", cwd=cwd)
    out = run("train_victim.py", "--model", "vgg13", "--saving_prefix", "train_victim", "--load_checkpoint", "train_generator_clean",
              "--n_iters", "1", cwd=cwd)
    assert "Bd Acc:" in out
    sd = torch.load(os.path.join(cwd, "ckpt", "train_victim", "cifar10", "cifar10_train_victim.pth.tar"), map_location="cpu",
                    weights_only=True)
    assert set(sd) == {"netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "epoch_current"}
    assert list(sd["netC"]) == keys and len(sd["optimizerC"]["state"]) == 42
    out = run("eval.py", "--model", "vgg13", "--saving_prefix", "train_generator", "--load_checkpoint_clean", "train_victim",
              "--load_checkpoint", "train_generator_clean", cwd=cwd)
    assert "Clean Acc:" in out and "Bd BA:" in out and "Bd ASR:" in out


def test_celeba_clean_classifier_with_model_vgg13(tmp_path):
    """--dataset celeba: 64 x 64 inputs, the 2 x 2 x 512 head (classifier.weight [8][2048])."""
    cwd = str(tmp_path)
    run("train_clean_classifier.py", "--model", "vgg13", "--dataset", "celeba", "--saving_prefix", "vgg_clean", "--n_iters", "1",
        "--max_steps", "3", cwd=cwd)
    sd = torch.load(os.path.join(cwd, "ckpt", "vgg_clean", "celeba", "celeba_vgg_clean.pth.tar"), map_location="cpu", weights_only=True)
    assert sd["netC"]["classifier.weight"].shape == (8, 2048) and len(sd["netC"]) == 72
    assert all(torch.isfinite(v.float()).all() for v in sd["netC"].values())
