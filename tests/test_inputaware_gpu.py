"""The input-aware (cross-trigger) step on the MI355X (reference train_generator_inputaware.py): the paired trigger
kernels, netC's two-loss-half eval pass, InputAwareStep against the test-side restatement (tests/inputaware_ref.py),
its reduction to AlternatedStep at cross_weight 0, deterministic mode, and the two scripts on synthetic data."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402
import inputaware_ref as IR  # noqa: E402
from test_engine_gpu import Opt, _build, _oracle_state, bench_batch, flat_grads, rel_l2, stored  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    from combat_amd import engine, nets, ops, step, trigger
    return dict(engine=engine, nets=nets, ops=ops, step=step, trigger=trigger)


class IAOpt(Opt):
    cross_weight = 0.2


# ------------------------------------------------------------------ paired trigger kernels
@pytest.mark.parametrize("hw,n", [(32, 7), (64, 5)])
def test_trigger_pair_equals_two_single_calls(mods, hw, n):
    from oracle import combat_oracle as O
    ops, trigger = mods["ops"], mods["trigger"]
    gen = torch.Generator().manual_seed(hw + n)
    x = torch.rand(n, 3, hw, hw, generator=gen) * 2 - 1
    x[0, :, : hw // 2] = 0.999                  # saturates the clamp where the noise is positive
    x[1, :, :, : hw // 2] = -0.999
    z = torch.randn(2 * n, 3, hw, hw, generator=gen)
    noise = torch.tanh(z)
    noise_c8 = torch.zeros(2 * n, hw, hw, 8, dtype=torch.bfloat16)
    noise_c8[..., :3] = noise.permute(0, 2, 3, 1).to(torch.bfloat16)
    noise_c8 = noise_c8.cuda()
    noise_q = noise_c8[..., :3].float().permute(0, 3, 1, 2).cpu()         # what the kernels read
    rate, ratio, sg, sx = 0.08, 0.65, 0.4, 0.8
    pm = trigger.lowpass_matrix(hw, ratio).cuda()
    k1 = torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(s, 3)) for s in (sg, sx)]).cuda()
    xc = x.cuda()
    bd, bd2 = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(n, 3, hw, hw, device="cuda")
    mse = torch.empty(3 * n, device="cuda")
    ops.trigger_pair_fwd(xc, noise_c8, pm, k1, rate, bd, bd2, mse)
    r_bd, r_bd2, r_mse = torch.empty_like(bd), torch.empty_like(bd), torch.empty_like(mse)
    ops.trigger_fwd(xc, noise_c8[:n], pm, k1[0], rate, r_bd, mse_partial=r_mse)
    ops.trigger_fwd(xc, noise_c8[n:], pm, k1[1], rate, r_bd2)
    torch.cuda.synchronize()
    assert torch.equal(bd, r_bd) and torch.equal(bd2, r_bd2) and torch.equal(mse, r_mse)
    tol = 2e-5      # test_kernels_gpu.py::test_trigger_forward_backward's
    assert float((bd.cpu() - O.trigger_mix(x, noise_q[:n], rate, ratio, sg)).abs().max()) < tol
    assert float((bd2.cpu() - O.trigger_mix(x, noise_q[n:], rate, ratio, sx)).abs().max()) < tol
    pre = x.repeat(2, 1, 1, 1) + rate * O.low_freq(noise_q, ratio)
    assert (pre.abs() > 1).float().mean() > 0.02                               # both clamp branches are taken

    d_bd, d_bd2, d_cross = (torch.randn(n, 3, hw, hw, generator=gen).cuda() for _ in range(3))
    l2 = 0.3
    for with2 in (False, True):
        dn = torch.full((2 * n, hw, hw, 8), 7.0, dtype=torch.bfloat16, device="cuda")
        ops.trigger_pair_bwd(xc, noise_c8, pm, k1, rate, d_bd, bd, l2, d_cross, dn, pre_tanh=True,
                             d_bd2=d_bd2 if with2 else None)
        ref = torch.full_like(dn, 7.0)
        ops.trigger_bwd(xc, noise_c8[:n], pm, k1[0], rate, d_bd, bd, l2, ref[:n], pre_tanh=True,
                        d_out2=d_bd2 if with2 else None)
        ops.trigger_bwd(xc, noise_c8[n:], pm, k1[1], rate, d_cross, None, 0.0, ref[n:], pre_tanh=True)
        torch.cuda.synchronize()
        assert torch.equal(dn, ref), with2
    # backward against autograd through the oracle (w.r.t. the tanh output: pre_tanh off)
    dn = torch.empty(2 * n, hw, hw, 8, dtype=torch.bfloat16, device="cuda")
    ops.trigger_pair_bwd(xc, noise_c8, pm, k1, rate, d_bd, bd, l2, d_cross, dn, d_bd2=d_bd2)
    leaf = noise_q.clone().requires_grad_(True)
    o1 = O.trigger_mix(x, leaf[:n], rate, ratio, sg)
    o2 = O.trigger_mix(x, leaf[n:], rate, ratio, sx)
    tot = (o1 * (d_bd + d_bd2).cpu()).sum() + l2 * ((o1 - x) ** 2).sum() + (o2 * d_cross.cpu()).sum()
    (g,) = torch.autograd.grad(tot, leaf)
    assert rel_l2(dn[..., :3].float().permute(0, 3, 1, 2), g) < 4e-3


# ------------------------------------------------------------------ two-loss-half classifier pass
@pytest.mark.parametrize("arch,n", [("preact", 16), ("preact", 128), ("resnet", 16)])
def test_two_half_plan_equals_two_separate_passes(mods, arch, n):
    """forward_plan(two_loss=True) + backward_eval_plan(half_weights=...) over a 2n slot against two separate n-image
    eval passes: each half runs the n-image plan, so logits and input gradients are equal bit for bit (losses up to
    the order of the head's loss accumulation, counters exact).  ResNet18 at CelebA's 64 x 64, 8 classes."""
    nets, ops, engine = mods["nets"], mods["ops"], mods["engine"]
    hw = 32 if arch == "preact" else 64
    gen = torch.Generator().manual_seed(n)
    x = torch.rand(2 * n, 3, hw, hw, generator=gen) * 2 - 1
    t = torch.randint(0, 10 if arch == "preact" else 8, (2 * n,), generator=gen)
    cw = 0.2
    torch.manual_seed(0)
    m = (nets.PreActResNet18() if arch == "preact" else nets.ResNet18(num_classes=8, input_size=64)).cuda().eval()
    eng = m._net_engine()
    eng.refresh()
    s2 = eng.slot("tl", 2 * n, hw)
    ops.image_to_c8(x.cuda(), eng.input(s2))
    eng.head_bufs(s2)["targets"].copy_(t.cuda())
    eng.forward_plan(s2, False, 1.0, False, two_loss=True).run()
    eng.backward_eval_plan(s2, 1.0, half_weights=(1.0, cw)).run()
    outs = []
    for k, w in ((0, 1.0), (1, cw)):
        s1 = eng.slot("tl.sep%d" % k, n, hw)
        ops.image_to_c8(x[k * n:(k + 1) * n].cuda(), eng.input(s1))
        eng.head_bufs(s1)["targets"].copy_(t[k * n:(k + 1) * n].cuda())
        eng.forward_plan(s1, False, 1.0, False).run()
        eng.backward_eval_plan(s1, w).run()
        outs.append(s1)
    torch.cuda.synchronize()
    h2 = eng.head_bufs(s2)
    cells = ((h2["loss"], h2["correct"]), (s2.bufs["loss1"], s2.bufs["correct1"]))
    for k, s1 in enumerate(outs):
        h1 = eng.head_bufs(s1)
        r = float(h1["loss"])
        assert abs(float(cells[k][0]) - r) <= 2e-3 * max(1.0, abs(r)), (k, float(cells[k][0]), r)
        if engine.deterministic():
            assert float(cells[k][0]) == r
        assert torch.equal(cells[k][1], h1["correct"])
        assert torch.equal(h2["logits"][k * n:(k + 1) * n], h1["logits"])
        assert torch.equal(s2.bufs["g.img"][k * n:(k + 1) * n, ..., :3], s1.bufs["g.img"][..., :3])


# ------------------------------------------------------------------ the step against the restatement
@pytest.mark.parametrize("b", [16, 128])
def test_inputaware_step_vs_restatement(mods, b):
    """Phase C from the identical start; Phase G teacher-forced from the engine's post-Phase-C state (as
    test_engine_gpu.py::test_alternated_step_vs_oracle, whose tolerances these are)."""
    from oracle import combat_oracle as O
    step_mod, nets = mods["step"], mods["nets"]
    seeds = [0, 1, 2, 3]
    netc, clean, netg, netf = _build(mods, seeds)
    oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
    old_g = _oracle_state(netg)
    if b == 16:
        gen = torch.Generator().manual_seed(5)
        x = (torch.randint(0, 256, (b, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
        t = torch.randint(0, 10, (b,), generator=gen)
        t[:4] = 0
        x2 = (torch.randint(0, 256, (b, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    else:
        x, t = bench_batch(0)
        x2, _ = bench_batch(1)
    nb, sc, sg, sx, cw = (3 if b == 16 else 6), 0.4, 0.7, 0.3, 0.2
    cfg = O.StepConfig(lr_g=1e-3)
    ref = IR.inputaware_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)),
                             x, x2, t, IR.Randomness(nb, sc, sg, sx), cfg, cw,
                             clf_fn=E.preact_forward_emu, gen_fn=E.unet_forward_emu)
    netc, clean, netg, netf = netc.cuda(), clean.cuda().eval(), netg.cuda(), netf.cuda().eval()
    st = step_mod.InputAwareStep(netc, netg, clean, netf, IAOpt())
    st.keep_grads = True
    st.run(x.cuda(), t, x2.cuda(), step_mod.InputAwareRandomness(nb, sc, sg, [None] * 6, sigma_x=sx), lr_g=1e-3)
    torch.cuda.synchronize()
    m = st.read_metrics()
    tol = lambda r: 1e-2 * max(1.0, abs(r))
    # ---- Phase C
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"])
    gn_c = float(st.eC.fp.grad.double().norm())
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G, teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    names_g = O.trainable_names(old_g)
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + nm for nm, *_ in nets.UNET_LAYERS] + ["up0", "up1", "up2", "up3", "noise"]
    noise = E.unet_forward_emu(pg, torch.cat([x, x2]), force=stored(st.sG, keys, 3))
    ibd = O.trigger_mix(x, noise[:b], 0.08, 0.65, sg)
    ibd2 = O.trigger_mix(x, noise[b:], 0.08, 0.65, sx)
    assert float((st.bd.cpu() - ibd.detach()).abs().max()) < 3e-5
    assert float((st.bd2.cpu() - ibd2.detach()).abs().max()) < 3e-5
    bd_t = torch.zeros_like(t)
    leaf, leaf2 = ibd.detach().clone().requires_grad_(True), ibd2.detach().clone().requires_grad_(True)
    pred_bd = E.preact_forward_emu(oc2, leaf, False)
    pred_cross = E.preact_forward_emu(oc2, leaf2, False)
    cm_pred = E.preact_forward_emu(ok, leaf, False)
    loss_ce, loss_cross, cm_loss = F.cross_entropy(pred_bd, bd_t), F.cross_entropy(pred_cross, t), F.cross_entropy(cm_pred, t)
    for ours, r in (("loss_ce_sum", loss_ce), ("loss_cross_sum", loss_cross), ("clean_model_loss_sum", cm_loss)):
        r = float(r.detach())
        assert abs(m[ours] - r) < tol(r), (ours, m[ours], r)
    assert abs(m["cross_correct"] - int((pred_cross.argmax(1) == t).sum())) <= 1
    assert abs(m["bd_correct"] - int((pred_bd.argmax(1) == bd_t).sum())) <= 1
    (d_cross,) = torch.autograd.grad(cw * loss_cross, leaf2)
    assert rel_l2(st.d_cross.cpu(), d_cross) < 0.25
    total = (ibd * (st.d_bd + st.d_bd2).cpu()).sum() + (ibd2 * st.d_cross.cpu()).sum() + 0.02 * F.mse_loss(ibd, x)
    gr = torch.autograd.grad(total, [pg[k] for k in names_g], allow_unused=True)
    gr = torch.cat([(torch.zeros_like(pg[k]) if a is None else a).reshape(-1) for k, a in zip(names_g, gr)])
    assert rel_l2(flat_grads(st.eG.fp, names_g), gr) < 5e-2
    fp = st.eG.fp
    for k in ("conv0_0.weight", "conv3_1.weight", "upconv0_0.bias", "upconv1_0.bias"):
        exp = old_g[k] - 1e-3 * 1.9 * (fp.logical(fp.grad, k).cpu() + 5e-4 * old_g[k])
        assert rel_l2(netg.state_dict()[k].detach().cpu(), exp) < 1e-6, k

    # ---- the first half of the 2n generator output is AlternatedStep's n-image forward
    netc1, clean1, netg1, netf1 = (mm.cuda() for mm in _build(mods, seeds))
    st1 = step_mod.AlternatedStep(netc1, netg1, clean1.eval(), netf1.eval(), IAOpt())
    st1.run(x.cuda(), t, step_mod.StepRandomness(nb, sc, sg, [None] * 5))
    torch.cuda.synchronize()
    # The first step's generator forward reads the same weights in both objects, and InputAwareStep runs the n-image
    # plan on each half of its 2n slot: the same launches with the same tile / partition parameters, bit for bit.
    assert torch.equal(st.eG.output(st.sG)[:b, ..., :3], st1.eG.output(st1.sG)[..., :3])


# ------------------------------------------------------------------ cross_weight 0 == the alternated step
def _two_steps(mods, cls, cw, x, t, x2):
    step_mod = mods["step"]
    netc, clean, netg, netf = (mm.cuda() for mm in _build(mods, [0, 1, 2, 3]))
    g0 = torch.cat([p.detach().flatten() for p in netg.parameters()]).clone()
    o = IAOpt()
    o.cross_weight = cw
    st = cls(netc, netg, clean.eval(), netf.eval(), o)
    for i in range(2):
        if cls is step_mod.AlternatedStep:
            st.run(x.cuda(), t, step_mod.StepRandomness(3, 0.4, 0.7, [None] * 5), lr_g=1e-3)
        else:
            st.run(x.cuda(), t, x2.cuda(), step_mod.InputAwareRandomness(3, 0.4, 0.7, [None] * 6, sigma_x=0.5), lr_g=1e-3)
    torch.cuda.synchronize()
    g1 = torch.cat([p.detach().flatten() for p in netg.parameters()]).clone()
    return st.read_metrics(), torch.cat([p.detach().flatten() for p in netc.parameters()]).clone(), g1 - g0


def test_cross_weight_zero_reduces_to_the_alternated_step(mods):
    step_mod, engine = mods["step"], mods["engine"]
    gen = torch.Generator().manual_seed(11)
    x = (torch.randint(0, 256, (32, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    x2 = (torch.randint(0, 256, (32, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    t = torch.randint(0, 10, (32,), generator=gen)
    t[:5] = 0
    prev = engine.deterministic()
    engine.set_deterministic(True)
    try:
        m0, c0, u0 = _two_steps(mods, step_mod.AlternatedStep, 0.0, x, t, x2)
        m1, c1, u1 = _two_steps(mods, step_mod.InputAwareStep, 0.0, x, t, x2)
        _, _, u2 = _two_steps(mods, step_mod.InputAwareStep, 0.2, x, t, x2)
    finally:
        engine.set_deterministic(prev)
    d_noise, d_cross = float((u1 - u0).norm()), float((u2 - u0).norm())
    assert d_noise < 0.1 * d_cross, (d_noise, d_cross)
    for k in ("loss_c_sum", "loss_ce_sum", "clean_model_loss_sum", "loss_l2_sum"):
        assert abs(m0[k] - m1[k]) <= 2e-3 * max(1.0, abs(m0[k])), (k, m0[k], m1[k])
    for k in ("clean_correct", "bd_correct", "clean_model_correct", "clean_model_bd_ba", "clean_model_bd_asr", "train_correct"):
        assert abs(m0[k] - m1[k]) <= 1, (k, m0[k], m1[k])
    assert rel_l2(c1, c0) < 2e-3


def test_inputaware_step_is_deterministic(mods):
    """Two runs from the same state and draws, with a ragged second batch size and an empty poison set."""
    step_mod, engine = mods["step"], mods["engine"]
    gen = torch.Generator().manual_seed(12)
    x = (torch.randint(0, 256, (40, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    x2 = (torch.randint(0, 256, (40, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    t = torch.randint(0, 10, (40,), generator=gen)
    prev = engine.deterministic()
    engine.set_deterministic(True)
    out = []
    try:
        for _ in range(2):
            netc, clean, netg, netf = (mm.cuda() for mm in _build(mods, [0, 1, 2, 3]))
            o = IAOpt()
            o.kernel_size = 5          # ignored: the step's blur is the reference's fixed 3-tap one
            st = step_mod.InputAwareStep(netc, netg, clean.eval(), netf.eval(), o)
            assert st.opt.kernel_size == 3 and o.kernel_size == 5
            st.run(x.cuda(), t, x2.cuda(), step_mod.InputAwareRandomness(4, 0.4, 0.7, [None] * 6, sigma_x=0.5))
            st.run(x[:24].cuda(), t[:24], x2[:24].cuda(), step_mod.InputAwareRandomness(0, 0.5, 0.6, [None] * 6, sigma_x=0.9))
            torch.cuda.synchronize()
            out.append((st.read_metrics(), torch.cat([p.detach().flatten() for p in netc.parameters()]).clone(),
                        torch.cat([p.detach().flatten() for p in netg.parameters()]).clone()))
    finally:
        engine.set_deterministic(prev)
    (m0, c0, g0), (m1, c1, g1) = out
    assert m0 == m1
    assert torch.equal(c0, c1) and torch.equal(g0, g1)
    assert m0["samples"] == 64 and np.isfinite(m0["loss_cross_sum"]) and m0["loss_cross_sum"] > 0


# ------------------------------------------------------------------ the two scripts on synthetic data
def run(script, *args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--synthetic_size", "256", "--bs", "64",
           "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1"] + list(args)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


GEN_KEYS = {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model", "best_clean_acc",
            "best_bd_acc", "best_cross_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
            "best_clean_model_bd_asr", "epoch_current", "mask", "pattern"}


def test_inputaware_workflow_on_synthetic_data(tmp_path):
    cwd = str(tmp_path)
    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", "--n_iters", "1", cwd=cwd)
    out = run("train_generator_inputaware.py", "--saving_prefix", "inputaware", "--load_checkpoint_clean",
              "classifier_clean", "--n_iters", "1", cwd=cwd)
    assert "Cross Acc:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "inputaware_clean", "cifar10", "cifar10_inputaware_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert set(sd) == GEN_KEYS
    assert 0.0 <= sd["best_cross_acc"] <= 100.0
    assert sd["mask"].shape == (32, 32) and float(sd["mask"].sum()) == pytest.approx(1.6)
    assert sd["pattern"].shape == (3, 32, 32)
    assert sd["optimizerG"]["param_groups"][0]["lr"] == pytest.approx(1e-3)      # lr_C * 0.1
    assert all(torch.isfinite(v).all() for v in sd["netG"].values())
    # resume: lower the stored best so that the resumed epoch saves again -- its checkpoint must carry the RESTORED
    # mask / pattern (a fresh run would draw another pattern)
    sd["best_clean_acc"] = -1.0
    torch.save(sd, gen)
    out = run("train_generator_inputaware.py", "--saving_prefix", "inputaware", "--load_checkpoint_clean",
              "classifier_clean", "--n_iters", "2", "--continue_training", cwd=cwd)
    assert "Continue training!!" in out and "Cross Acc:" in out and "Saving..." in out
    sd2 = torch.load(gen, map_location="cpu", weights_only=True)
    assert set(sd2) == GEN_KEYS
    assert torch.equal(sd2["pattern"], sd["pattern"]) and torch.equal(sd2["mask"], sd["mask"])
    out = run("train_victim_inputaware.py", "--saving_prefix", "victim_ia", "--load_checkpoint", "inputaware_clean",
              "--n_iters", "1", cwd=cwd)
    assert "Cross Acc:" in out
    vic = os.path.join(cwd, "ckpt", "victim_ia_clean", "cifar10", "cifar10_victim_ia_clean.pth.tar")
    assert set(torch.load(vic, map_location="cpu", weights_only=True)) == {
        "netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "best_cross_acc", "epoch_current"}


def test_inputaware_script_on_two_ranks(tmp_path):
    """train_generator_inputaware.py under torch.distributed.run with two ranks on this box's one GPU (exchange over
    gloo, as tests/test_entrypoints_gpu.py's rehearsal): two sharded train loaders per rank (100 of 200 images each:
    batches of 64 and 36), the evaluation loaders' shards ending in a 36-image batch, the counters summed and
    the BatchNorm statistics averaged over the ranks, and rank 0 alone writing the checkpoint.  16 s on the MI355X,
    the clean classifier's epoch included."""
    import glob
    import socket
    cwd = str(tmp_path)
    common = ["--synthetic", "--synthetic_size", "200", "--bs", "64", "--checkpoints", os.path.join(cwd, "ckpt"),
              "--allow_missing_F", "--log_interval", "1", "--n_iters", "1", "--seed", "1"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_clean_classifier.py"), "--saving_prefix", "classifier_clean"]
                       + common, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "--log-dir", os.path.join(cwd, "ranks"), "--tee", "3",
           os.path.join(ROOT, "train_generator_inputaware.py"), "--saving_prefix", "inputaware", "--load_checkpoint_clean",
           "classifier_clean"] + common
    env = dict(env, COMBAT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    logs = glob.glob(os.path.join(cwd, "ranks", "**", "stdout.log"), recursive=True)
    rank0 = [f for f in logs if os.path.basename(os.path.dirname(f)) == "0"]
    assert len(logs) == 2 and len(rank0) == 1, logs
    out0 = open(rank0[0]).read()
    assert "Cross Acc:" in out0 and "Saving..." in out0, out0[-3000:]
    written = glob.glob(os.path.join(cwd, "ckpt", "inputaware_clean", "**", "*.pth.tar"), recursive=True)
    assert written == [os.path.join(cwd, "ckpt", "inputaware_clean", "cifar10", "cifar10_inputaware_clean.pth.tar")], written
    sd = torch.load(written[0], map_location="cpu", weights_only=True)
    assert set(sd) == GEN_KEYS
    for net in ("netC", "netG"):
        assert all(torch.isfinite(v.float()).all() for v in sd[net].values()), net
