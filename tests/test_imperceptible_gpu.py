"""The imperceptible (total-variation) step on the MI355X (reference train_generator_imperceptible.py): the TV
trigger kernels, ImperceptibleStep against AlternatedStep at tv_weight 0 and against the test-side restatement
(tests/imperceptible_ref.py), the wiring of the TV term, deterministic mode, and the two scripts on synthetic data."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402
import imperceptible_ref as R  # noqa: E402
from test_engine_gpu import Opt, _build, _oracle_state, flat_grads, rel_l2, stored  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imperceptible_step.npz")


@pytest.fixture(scope="module")
def mods():
    from combat_amd import engine, nets, ops, step, trigger
    return dict(engine=engine, nets=nets, ops=ops, step=step, trigger=trigger)


def fixture_tv_weight():
    return float(np.load(GOLDEN)["tv_weight"])


class TVOpt(Opt):
    tv_weight = 0.0


def continuous_batch(b, seed):
    """Continuous random images (uniform in (-1, 1)): no flat or saturated regions, so few neighbour differences of
    inputs_bd sit on the sign's jump."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(b, 3, 32, 32, generator=gen) * 2 - 1
    t = torch.randint(0, 10, (b,), generator=gen)
    t[: max(4, b // 8)] = 0
    return x, t


# ------------------------------------------------------------------ kernels
def _kernel_case(mods, hw, n):
    trigger = mods["trigger"]
    gen = torch.Generator().manual_seed(hw * 1000 + n)
    x = torch.rand(n, 3, hw, hw, generator=gen) * 2 - 1
    x[0, :, : hw // 2] = 2.0                    # beyond the clamp whatever the noise: half an image of equal neighbours
    x[1, :, :, : hw // 2] = 0.999               # saturates the clamp where the noise is positive
    noise = torch.tanh(torch.randn(n, 3, hw, hw, generator=gen) * 3)
    noise_c8 = torch.zeros(n, hw, hw, 8, dtype=torch.bfloat16)
    noise_c8[..., :3] = noise.permute(0, 2, 3, 1).to(torch.bfloat16)
    noise_q = noise_c8[..., :3].float().permute(0, 3, 1, 2).contiguous()      # what the kernels read
    sigma = 0.6
    pm = trigger.lowpass_matrix(hw, 0.65).cuda()
    k1 = torch.from_numpy(trigger.gaussian_kernel1d(sigma, 3)).cuda()
    return x, noise_c8.cuda(), noise_q, pm, k1, sigma, gen


@pytest.mark.parametrize("hw,n", [(32, 16), (32, 128), (64, 16), (64, 128)])
def test_tv_forward(mods, hw, n):
    """out and mse_partial carry combat_trigger_fwd's bits; tv_partial against an fp64 sum over the same out bits, at the
    relative bound test_kernels_gpu.py::test_trigger_forward_backward applies to mse_partial."""
    ops = mods["ops"]
    x, n8, _, pm, k1, _, _ = _kernel_case(mods, hw, n)
    xc = x.cuda()
    out, mse, tv = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(3 * n, device="cuda"), torch.empty(3 * n, device="cuda")
    r_out, r_mse = torch.empty_like(out), torch.empty_like(mse)
    ops.trigger_tv_fwd(xc, n8, pm, k1, 0.08, out, tv, mse_partial=mse)
    ops.trigger_fwd(xc, n8, pm, k1, 0.08, r_out, mse_partial=r_mse)
    torch.cuda.synchronize()
    assert torch.equal(out, r_out) and torch.equal(mse, r_mse)
    o = out.cpu().double()
    ref = (o[..., 1:, :] - o[..., :-1, :]).abs().sum((2, 3)) + (o[..., :, 1:] - o[..., :, :-1]).abs().sum((2, 3))
    e = rel_l2(tv.view(n, 3), ref)
    print("tv_partial rel_l2 hw=%d n=%d: %.3g" % (hw, n, e))
    assert e < 1e-4
    torch.testing.assert_close(ref.sum(1), R.total_variation(o), rtol=1e-12, atol=0)
    tv2 = torch.empty_like(tv)                         # without mse_partial
    ops.trigger_tv_fwd(xc, n8, pm, k1, 0.08, r_out, tv2)
    torch.cuda.synchronize()
    assert torch.equal(tv2, tv) and torch.equal(r_out, out)


@pytest.mark.parametrize("hw,n", [(32, 16), (32, 128), (64, 16), (64, 128)])
def test_tv_backward_teacher_forced(mods, hw, n):
    """The sign decisions are taken from the HIP forward's own out bits on both sides, so every pixel is compared; the
    restated blur / clamp / DCT adjoint (autograd through oracle.trigger_mix) follows.  Bound: test_trigger_forward_backward's."""
    from oracle import combat_oracle as O
    ops = mods["ops"]
    x, n8, noise_q, pm, k1, sigma, gen = _kernel_case(mods, hw, n)
    xc = x.cuda()
    out, tv = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(3 * n, device="cuda")
    ops.trigger_tv_fwd(xc, n8, pm, k1, 0.08, out, tv)
    torch.cuda.synchronize()
    sign_map = R.tv_sign_stencil(out.cpu())                  # the same bits the kernel decides on
    ties = float(((out[..., 1:, :] - out[..., :-1, :]) == 0).float().mean())
    assert ties > 1e-3                                       # the saturated half image: sgn(0) = 0 is exercised
    leaf = noise_q.clone().requires_grad_(True)
    o_ref = O.trigger_mix(x, leaf, 0.08, 0.65, sigma)
    tv_scale, l2 = 0.5, 0.3
    # ---- the TV term alone: d_out = 0, l2_scale = 0
    dn = torch.full((n, hw, hw, 8), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.trigger_tv_bwd(xc, n8, pm, k1, 0.08, torch.zeros_like(out), out, 0.0, tv_scale, dn)
    (g_tv,) = torch.autograd.grad((o_ref * (tv_scale * sign_map)).sum(), leaf, retain_graph=True)
    e = rel_l2(dn[..., :3].float().permute(0, 3, 1, 2), g_tv)
    print("tv-only bwd rel_l2 hw=%d n=%d: %.3g" % (hw, n, e))
    assert e < 4e-3
    assert float(dn[..., 3:].float().abs().max()) == 0.0
    dn0 = torch.empty_like(dn)
    ops.trigger_tv_bwd(xc, n8, pm, k1, 0.08, None, out, 0.0, tv_scale, dn0)       # d_out absent == zero
    torch.cuda.synchronize()
    assert torch.equal(dn0, dn)
    # ---- all terms on: the sum of the parts
    d_out, d_out2 = (torch.randn(n, 3, hw, hw, generator=gen) for _ in range(2))
    ops.trigger_tv_bwd(xc, n8, pm, k1, 0.08, d_out.cuda(), out, l2, tv_scale, dn, pre_tanh=False, d_out2=d_out2.cuda())
    (g_rest,) = torch.autograd.grad((o_ref * (d_out + d_out2)).sum() + l2 * ((o_ref - x) ** 2).sum(), leaf, retain_graph=True)
    e = rel_l2(dn[..., :3].float().permute(0, 3, 1, 2), g_rest + g_tv)
    print("all-terms bwd rel_l2 hw=%d n=%d: %.3g  (|tv part| / |rest| = %.3g)" % (hw, n, e, float(g_tv.norm() / g_rest.norm())))
    assert e < 4e-3
    assert rel_l2(g_rest + g_tv, g_rest) > 0.2              # the TV part is no rounding error of the whole
    # ---- tv_scale = 0 is combat_trigger_bwd
    for pre in (False, True):
        a = torch.full_like(dn, 3.0)
        b = torch.full_like(dn, 3.0)
        ops.trigger_tv_bwd(xc, n8, pm, k1, 0.08, d_out.cuda(), out, l2, 0.0, a, pre_tanh=pre, d_out2=d_out2.cuda())
        ops.trigger_bwd(xc, n8, pm, k1, 0.08, d_out.cuda(), out, l2, b, pre_tanh=pre, d_out2=d_out2.cuda())
        torch.cuda.synchronize()
        assert torch.equal(a, b), pre
    # pre_tanh: the gradient w.r.t. the generator's pre-tanh output
    ops.trigger_tv_bwd(xc, n8, pm, k1, 0.08, None, out, 0.0, tv_scale, dn, pre_tanh=True)
    assert rel_l2(dn[..., :3].float().permute(0, 3, 1, 2), g_tv * (1 - noise_q ** 2)) < 4e-3


# ------------------------------------------------------------------ the step
def _run_steps(mods, cls, tv_weight, batches, draws, lr_g=1e-2, kernel_size=3):
    step_mod = mods["step"]
    netc, clean, netg, netf = (mm.cuda() for mm in _build(mods, [0, 1, 2, 3]))
    g0 = torch.cat([p.detach().flatten() for p in netg.parameters()]).clone()
    o = TVOpt()
    o.tv_weight, o.kernel_size = tv_weight, kernel_size
    st = cls(netc, netg, clean.eval(), netf.eval(), o)
    for (x, t), (nb, sc, sg) in zip(batches, draws):
        st.run(x.cuda(), t, step_mod.StepRandomness(nb, sc, sg, [None] * 5), lr_g=lr_g)
    torch.cuda.synchronize()
    return dict(m=st.read_metrics(), c=torch.cat([p.detach().flatten() for p in netc.parameters()]).clone(),
                g=torch.cat([p.detach().flatten() for p in netg.parameters()]).clone(), g0=g0,
                mom_c=st.eC.fp.mom.clone(), mom_g=st.eG.fp.mom.clone(), st=st)


def test_tv_weight_zero_is_the_alternated_step(mods):
    """Deterministic mode, default --kernel_size 3: parameters, momentum buffers and every parent metric bit for bit."""
    step_mod, engine = mods["step"], mods["engine"]
    batches = [continuous_batch(32, 21), continuous_batch(32, 22)]
    draws = [(3, 0.4, 0.7), (0, 0.5, 0.3)]
    prev = engine.deterministic()
    engine.set_deterministic(True)
    try:
        a = _run_steps(mods, step_mod.AlternatedStep, 0.0, batches, draws)
        b = _run_steps(mods, step_mod.ImperceptibleStep, 0.0, batches, draws)
    finally:
        engine.set_deterministic(prev)
    for k in ("c", "g", "mom_c", "mom_g"):
        assert torch.equal(a[k], b[k]), k
    assert float((a["g"] - a["g0"]).abs().max()) > 0
    for k, v in a["m"].items():
        assert b["m"][k] == v, (k, b["m"][k], v)
    assert b["m"]["loss_tv_sum"] > 0 and "loss_tv_sum" not in a["m"]


@pytest.mark.parametrize("b", [16, 128])
def test_imperceptible_step_vs_restatement(mods, b):
    """Phase C from the identical start; Phase G teacher-forced from the engine's post-Phase-C state (the comparators
    and tolerances of test_inputaware_gpu.py::test_inputaware_step_vs_restatement), with the TV term in the total.

    Sign flips: the generator runs in bf16, so inputs_bd differs from the fp32 restatement and some signs of the TV
    gradient flip.  The yardstick is the reference side alone: the restatement run in fp32 and run with the bf16
    emulation of tests/bf16_emu.py (networks' outputs rounded as the engines round them); the distance of the
    engine's generator update from the fp32 one may be 1.6 x the emulation's distance from it (test_engine_gpu.py's
    factor)."""
    from oracle import combat_oracle as O
    step_mod, nets = mods["step"], mods["nets"]
    tvw = fixture_tv_weight()
    seeds = [0, 1, 2, 3]
    x, t = continuous_batch(b, 31 + b)
    nb, sc, sg = (3 if b == 16 else 6), 0.4, 0.6
    cfg = O.StepConfig(lr_g=1e-2)
    names_g = O.trainable_names(_oracle_state(_build(mods, seeds)[2]))

    def restate(clf_fn, gen_fn):
        netc, clean, netg, netf = _build(mods, seeds)
        oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
        before = torch.cat([og[k].flatten() for k in names_g]).clone()
        keep = {}
        out = R.imperceptible_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(names_g), x, t,
                                   O.StepRandomness(nb, sc, sg), cfg, tvw, clf_fn=clf_fn, gen_fn=gen_fn, keep=keep)
        return out, torch.cat([og[k].detach().flatten() for k in names_g]) - before, keep["bd"]

    ref32, upd32, bd32 = restate(None, None)
    ref, upd_emu, _ = restate(E.preact_forward_emu, E.unet_forward_emu)
    d = torch.cat([(bd32[..., 1:, :] - bd32[..., :-1, :]).flatten(), (bd32[..., :, 1:] - bd32[..., :, :-1]).flatten()]).abs()
    share = float((d < 1e-3).float().mean())
    print("share of neighbour differences under 1e-3: %.4f %%" % (100 * share))
    assert share <= 0.01

    netc, clean, netg, netf = _build(mods, seeds)
    ok, old_g = _oracle_state(clean), _oracle_state(netg)
    netc, clean, netg, netf = netc.cuda(), clean.cuda().eval(), netg.cuda(), netf.cuda().eval()
    o = TVOpt()
    o.tv_weight = tvw
    st = step_mod.ImperceptibleStep(netc, netg, clean, netf, o)
    st.keep_grads = True
    st.run(x.cuda(), t, step_mod.StepRandomness(nb, sc, sg, [None] * 5))
    torch.cuda.synchronize()
    m = st.read_metrics()
    tol = lambda r: 1e-2 * max(1.0, abs(r))
    # ---- Phase C
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"])
    gn_c = float(st.eC.fp.grad.double().norm())
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G, teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + nm for nm, *_ in nets.UNET_LAYERS] + ["up0", "up1", "up2", "up3", "noise"]
    noise = E.unet_forward_emu(pg, x, force=stored(st.sG, keys, 3))
    ibd = O.trigger_mix(x, noise, 0.08, 0.65, sg)
    assert float((st.bd.cpu() - ibd.detach()).abs().max()) < 3e-5
    bd_t = torch.zeros_like(t)
    leaf = ibd.detach().clone().requires_grad_(True)
    pred_bd = E.preact_forward_emu(oc2, leaf, False)
    cm_pred = E.preact_forward_emu(ok, leaf, False)
    loss_ce, cm_loss = F.cross_entropy(pred_bd, bd_t), F.cross_entropy(cm_pred, t)
    for ours, r in (("loss_ce_sum", loss_ce), ("clean_model_loss_sum", cm_loss)):
        r = float(r.detach())
        assert abs(m[ours] - r) < tol(r), (ours, m[ours], r)
    assert abs(m["bd_correct"] - int((pred_bd.argmax(1) == bd_t).sum())) <= 1
    tv_ref = float(R.total_variation(ibd.detach().double()).mean())
    print("loss_tv: step %.6f restatement (teacher-forced) %.6f" % (m["loss_tv_sum"], tv_ref))
    assert abs(m["loss_tv_sum"] - tv_ref) < 1e-3 * tv_ref          # as loss_l2_sum in test_alternated_step_vs_oracle
    # the engine's own classifier gradients as cotangent, the sign map from the engine's own inputs_bd bits
    cot = (st.d_bd + st.d_bd2).cpu() + (tvw / b) * R.tv_sign_stencil(st.bd.cpu())
    total = (ibd * cot).sum() + 0.02 * F.mse_loss(ibd, x)
    gr = torch.autograd.grad(total, [pg[k] for k in names_g], allow_unused=True)
    gr = torch.cat([(torch.zeros_like(pg[k]) if a is None else a).reshape(-1) for k, a in zip(names_g, gr)])
    e_tf = rel_l2(flat_grads(st.eG.fp, names_g), gr)
    print("generator gradient, teacher-forced rel_l2: %.4g" % e_tf)
    assert e_tf < 5e-2
    fp = st.eG.fp
    for k in ("conv0_0.weight", "conv3_1.weight", "upconv0_0.bias", "upconv1_0.bias"):
        exp = old_g[k] - 1e-2 * 1.9 * (fp.logical(fp.grad, k).cpu() + 5e-4 * old_g[k])
        assert rel_l2(netg.state_dict()[k].detach().cpu(), exp) < 1e-6, k
    # ---- the whole generator update against the fp32 restatement, measured by the emulation's own distance
    upd = torch.cat([netg.state_dict()[k].detach().cpu().flatten() - old_g[k].flatten() for k in names_g])
    base, e = rel_l2(upd_emu, upd32), rel_l2(upd, upd32)
    print("generator update vs fp32 restatement: engine %.4g, bf16 emulation (base) %.4g, ratio %.3f" % (e, base, e / base))
    assert e < 1.6 * base, (e, base)


def test_tv_term_is_wired(mods):
    """The generator update at the fixture's tv_weight differs from the tv_weight 0 update by what the restatement
    says: direction and size of the difference, at the bound of the step test (1.6 x the bf16 emulation's own distance
    from the fp32 restatement); loss_tv_sum equals the restatement's."""
    from oracle import combat_oracle as O
    step_mod, engine = mods["step"], mods["engine"]
    tvw = fixture_tv_weight()
    b = 16
    x, t = continuous_batch(b, 41)
    nb, sc, sg = 3, 0.4, 0.6
    seeds = [0, 1, 2, 3]
    names_g = O.trainable_names(_oracle_state(_build(mods, seeds)[2]))

    def restate(w, clf_fn, gen_fn):
        netc, clean, netg, netf = _build(mods, seeds)
        oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
        before = torch.cat([og[k].flatten() for k in names_g]).clone()
        out = R.imperceptible_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(names_g), x, t,
                                   O.StepRandomness(nb, sc, sg), O.StepConfig(lr_g=1e-2), w, clf_fn=clf_fn, gen_fn=gen_fn)
        return out, torch.cat([og[k].detach().flatten() for k in names_g]) - before

    r32, u32 = restate(tvw, None, None)
    _, u32_0 = restate(0.0, None, None)
    remu, uemu = restate(tvw, E.preact_forward_emu, E.unet_forward_emu)
    _, uemu_0 = restate(0.0, E.preact_forward_emu, E.unet_forward_emu)
    prev = engine.deterministic()
    engine.set_deterministic(True)
    try:
        a = _run_steps(mods, step_mod.ImperceptibleStep, tvw, [(x, t)], [(nb, sc, sg)])
        z = _run_steps(mods, step_mod.ImperceptibleStep, 0.0, [(x, t)], [(nb, sc, sg)])
    finally:
        engine.set_deterministic(prev)
    d_eng, d_32, d_emu = a["g"].cpu() - z["g"].cpu(), u32 - u32_0, uemu - uemu_0
    # _run_steps concatenates netg.parameters() in module order: the restatement's names_g order
    assert d_eng.numel() == d_32.numel()
    base, e = rel_l2(d_emu, d_32), rel_l2(d_eng, d_32)
    cos = float(torch.dot(d_eng.double(), d_32.double()) / (d_eng.double().norm() * d_32.double().norm()))
    size = float(d_eng.double().norm() / d_32.double().norm())
    print("TV part of the update: engine vs fp32 %.4g, emulation vs fp32 (base) %.4g, cosine %.4f, size ratio %.4f; "
          "|TV part| / |update| = %.3f" % (e, base, cos, size, float(d_32.norm() / u32.norm())))
    assert float(d_32.norm()) > 0.2 * float(u32.norm())          # the term is a visible share of the update
    assert e < 1.6 * base, (e, base)
    assert cos > 1 - (1.6 * base) ** 2 / 2 and abs(size - 1) < 1.6 * base      # direction and size, the same bound
    # loss_tv: the engine's bf16 generator against the bf16-emulating restatement (the bf16 design's own distance
    # from fp32 as the yardstick, x 1.6)
    tv_eng, tv_emu, tv_32 = a["m"]["loss_tv_sum"], remu["loss_tv"], r32["loss_tv"]
    print("loss_tv: engine %.6f emulation %.6f fp32 %.6f" % (tv_eng, tv_emu, tv_32))
    assert abs(tv_eng - tv_32) <= 1.6 * abs(tv_emu - tv_32) + 1e-4 * tv_32
    assert z["m"]["loss_tv_sum"] == a["m"]["loss_tv_sum"]       # the logged value does not depend on the weight


def test_imperceptible_step_is_deterministic(mods):
    """Two runs from the same state and draws, with a ragged second batch size and an empty poison set; --kernel_size is
    ignored (the reference's fixed 3-tap blur)."""
    step_mod, engine = mods["step"], mods["engine"]
    (x, t), (x2, t2) = continuous_batch(40, 51), continuous_batch(24, 52)
    prev = engine.deterministic()
    engine.set_deterministic(True)
    out = []
    try:
        for _ in range(2):
            r = _run_steps(mods, step_mod.ImperceptibleStep, fixture_tv_weight(), [(x, t), (x2, t2), (x, t)],
                           [(4, 0.4, 0.7), (0, 0.5, 0.6), (2, 0.3, 0.9)], kernel_size=5)
            assert r["st"].opt.kernel_size == 3
            out.append(r)
    finally:
        engine.set_deterministic(prev)
    a, b = out
    assert a["m"] == b["m"]
    for k in ("c", "g", "mom_c", "mom_g"):
        assert torch.equal(a[k], b[k]), k
    assert a["m"]["samples"] == 104 and np.isfinite(a["m"]["loss_tv_sum"]) and a["m"]["loss_tv_sum"] > 0
    a["st"].reset_metrics()
    assert a["st"].read_metrics()["loss_tv_sum"] == 0.0


# ------------------------------------------------------------------ the scripts on synthetic data
def run(script, *args, cwd):
    cmd = [sys.executable, os.path.join(ROOT, script), "--synthetic", "--synthetic_size", "256", "--bs", "64",
           "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1"] + list(args)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


GEN_KEYS = {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model", "best_clean_acc",
            "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba", "best_clean_model_bd_asr",
            "epoch_current"}


def _tv_loss_rows(cwd):
    import json
    log_dir = os.path.join(cwd, "ckpt", "imperceptible_clean", "cifar10", "log_dir")
    path = os.path.join(log_dir, "scalars.jsonl")
    if not os.path.exists(path):       # tensorboard present: the event files hold the scalars
        return None
    return [json.loads(line)["values"] for line in open(path) if '"Clean Accuracy"' in line]


def test_imperceptible_workflow_on_synthetic_data(tmp_path):
    cwd = str(tmp_path)
    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", "--n_iters", "1", cwd=cwd)
    out = run("train_generator_imperceptible.py", "--saving_prefix", "imperceptible", "--load_checkpoint_clean",
              "classifier_clean", "--n_iters", "1", "--tv_weight", "0.001", "--kernel_size", "5", cwd=cwd)
    assert "Clean Model Bd ASR:" in out and "Saving..." in out
    gen = os.path.join(cwd, "ckpt", "imperceptible_clean", "cifar10", "cifar10_imperceptible_clean.pth.tar")
    sd = torch.load(gen, map_location="cpu", weights_only=True)
    assert set(sd) == GEN_KEYS
    assert all(torch.isfinite(v).all() for v in sd["netG"].values())
    rows = _tv_loss_rows(cwd)
    if rows is not None:
        assert len(rows) == 1 and rows[0]["TV Loss"] > 0 and np.isfinite(rows[0]["TV Loss"])
    # resume: the stored best is lowered so that the resumed epoch saves again; the checkpoint's clean_model is NOT what
    # the resumed run uses (reference :518-534) -- it is poisoned here, and the run must still load and finish
    sd["best_clean_acc"] = -1.0
    clean_ref = {k: v.clone() for k, v in sd["clean_model"].items()}
    sd["clean_model"] = {k: (v * 0 if v.is_floating_point() else v) for k, v in sd["clean_model"].items()}
    torch.save(sd, gen)
    out = run("train_generator_imperceptible.py", "--saving_prefix", "imperceptible", "--load_checkpoint_clean",
              "classifier_clean", "--n_iters", "2", "--continue_training", "--tv_weight", "0.001", cwd=cwd)
    assert "Continue training!!" in out and "Saving..." in out
    sd2 = torch.load(gen, map_location="cpu", weights_only=True)
    assert set(sd2) == GEN_KEYS
    for k, v in clean_ref.items():       # the saved clean model is the one --load_checkpoint_clean named
        assert torch.equal(sd2["clean_model"][k], v), k
    run("train_victim_imperceptible.py", "--saving_prefix", "victim_tv", "--load_checkpoint", "imperceptible_clean",
        "--n_iters", "1", cwd=cwd)
    vic = os.path.join(cwd, "ckpt", "victim_tv", "cifar10", "cifar10_victim_tv.pth.tar")
    assert set(torch.load(vic, map_location="cpu", weights_only=True)) == {
        "netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "epoch_current"}
    out = run("eval.py", "--saving_prefix", "imperceptible", "--load_checkpoint_clean", "victim_tv",
              "--load_checkpoint", "imperceptible_clean", cwd=cwd)
    assert "Bd ASR:" in out
