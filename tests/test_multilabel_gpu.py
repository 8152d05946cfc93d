"""The multi-label attack's new HIP on the MI355X: combat_cond_fwd / combat_cond_wgrad bit for bit against their host
restatements (tests/multilabel_ref.py, the kernels' own summation order) and against fp64 autograd over explicit
one-hot planes, the grouped trigger bit-identical to per-chunk calls of the single-kernel trigger, and CUnetEngine
against the golden recorded from the reference's CUnetGeneratorv1 (the tolerance scheme of
test_engine_gpu.py::test_unet_forward_backward, from tests/bf16_emu.py) and against UnetEngine on shared weights."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402
import multilabel_ref as MR  # noqa: E402
from test_multilabel_cpu import wgrad_bound  # noqa: E402

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


class Opt:
    num_classes = 10


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel_l2(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def seeded(ctor, seed):
    torch.manual_seed(seed)
    return ctor()


@pytest.fixture(scope="module")
def mods():
    from combat_amd import engine, nets, ops, trigger
    return dict(engine=engine, nets=nets, ops=ops, trigger=trigger)


def _labels(n, classes):
    """0 and classes - 1 always occur."""
    return torch.tensor(([0, classes - 1, 3, classes - 1, 0, 2])[:n] if n > 1 else [classes - 1], dtype=torch.int32)


# ---------------------------------------------------------------- combat_cond_fwd


@pytest.mark.parametrize("s", [2, 3, 16])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("classes", [8, 10])
def test_cond_fwd_bit_exact(mods, s, n, classes):
    ops, nf = mods["ops"], 64
    w = MR.physical(torch.randn(nf, nf + classes, 3, 3, generator=torch.Generator().manual_seed(s + n)) * 0.05)
    labels = _labels(n, classes)
    cond = torch.full((n, s, s, nf), 7.0, dtype=bf16, device="cuda")
    ops.cond_fwd(w.cuda(), labels.cuda(), classes, cond)
    torch.cuda.synchronize()
    ref = MR.cond_ref(w, labels, s)
    assert torch.equal(cond.cpu().view(torch.int16), ref.view(torch.int16))
    assert float(ref.float().abs().max()) > 0.01


def test_cond_entry_points_refuse_map_size_one(mods):
    ops = mods["ops"]
    from combat_amd._lib import CombatHipError
    w = torch.zeros(64, 9, 74, device="cuda")
    y = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(CombatHipError):
        ops.cond_fwd(w, y, 10, torch.zeros(2, 1, 1, 64, dtype=bf16, device="cuda"))
    with pytest.raises(CombatHipError):
        ops.cond_wgrad(torch.zeros(2, 1, 1, 64, dtype=bf16, device="cuda"), y, 10, w, torch.zeros(2 * 9 * 64, device="cuda"))


# ---------------------------------------------------------------- combat_cond_wgrad


@pytest.mark.parametrize("s,labels,classes", [(2, [3], 10), (3, [0, 7, 7, 2, 0], 8), (16, [0, 9, 4, 9, 0], 10),
                                              (16, [5, 5, 5, 5, 5], 10)])
def test_cond_wgrad_bit_exact_and_vs_fp64(mods, s, labels, classes):
    """Cases: one image on a 2 x 2 map (every pixel a corner), classes absent from the batch (their rows exactly zero),
    all images of one class.  Bit for bit against the restatement, twice (no atomics: the same bits run to run), and
    against fp64 autograd within wgrad_bound (test_multilabel_cpu.py: the fp32 summation bound of the restatement's
    order; measured there at n = 5, s = 16: 4.8e-7 absolute, 5e-8 of max |dW_y|)."""
    ops, nf, n = mods["ops"], 64, len(labels)
    labels = torch.tensor(labels, dtype=torch.int32)
    d = (torch.randn(n, s, s, nf, generator=torch.Generator().manual_seed(9)) * 0.1).to(bf16)
    dwf = torch.randn(nf, 9, nf, generator=torch.Generator().manual_seed(10))
    ref = MR.cond_wgrad_ref(d, labels, classes, dwf)
    outs = []
    for with_dwf in (True, True, False):
        dw = torch.full((nf, 9, nf + classes), 7.0, device="cuda")
        scratch = torch.empty(n * 9 * nf, device="cuda")
        ops.cond_wgrad(d.cuda(), labels.cuda(), classes, dw, scratch, dwf.cuda() if with_dwf else None)
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    assert torch.equal(outs[0], ref) and torch.equal(outs[1], ref)
    assert torch.equal(outs[2][:, :, nf:], ref[:, :, nf:])
    assert float((outs[2][:, :, :nf] - 7.0).abs().max()) == 0.0          # without dwf the W_f columns are not touched
    wy = torch.zeros(nf, classes, 3, 3, dtype=torch.float64, requires_grad=True)
    (gy,) = torch.autograd.grad(MR.cond_planes_f64(wy, labels, s), wy, d.double().permute(0, 3, 1, 2))
    err = float((outs[0][:, :, nf:].double() - MR.physical(gy)).abs().max())
    bound = wgrad_bound(n, s, nf, float(d.float().abs().max()))
    print("cond_wgrad vs fp64: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    for c in range(classes):
        if c not in labels.tolist():
            assert float(outs[0][:, :, nf + c].abs().max()) == 0.0


# ---------------------------------------------------------------- grouped trigger


@pytest.mark.parametrize("n,ps,hw", [(13, 2, 32), (16, 16, 32), (13, 2, 64), (16, 16, 64)])
def test_trigger_groups_equal_per_chunk_calls(mods, n, ps, hw):
    ops, trigger = mods["ops"], mods["trigger"]
    gen = torch.Generator().manual_seed(hw + n)
    x = torch.rand(n, 3, hw, hw, generator=gen) * 2 - 1
    x[0, :, : hw // 2] = 0.999                  # saturates the clamp where the noise is positive
    x[1, :, :, : hw // 2] = -0.999
    noise_c8 = torch.zeros(n, hw, hw, 8, dtype=bf16)
    noise_c8[..., :3] = torch.tanh(torch.randn(n, 3, hw, hw, generator=gen)).permute(0, 2, 3, 1).to(bf16)
    noise_c8, xc = noise_c8.cuda(), x.cuda()
    groups = (n + ps - 1) // ps
    sig = [0.15 + 0.8 * i / max(groups - 1, 1) for i in range(groups)]
    pm = trigger.lowpass_matrix(hw, 0.65).cuda()
    k1 = torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(s, 3)) for s in sig]).cuda()
    rate, l2 = 0.08, 0.3
    bd, mse = torch.full((n, 3, hw, hw), 7.0, device="cuda"), torch.full((3 * n,), 7.0, device="cuda")
    ops.trigger_groups_fwd(xc, noise_c8, pm, k1, ps, rate, bd, mse)
    r_bd, r_mse = torch.empty_like(bd), torch.empty_like(mse)
    for ci in range(groups):
        si, ei = ci * ps, min(ci * ps + ps, n)
        ops.trigger_fwd(xc[si:ei], noise_c8[si:ei], pm, k1[ci], rate, r_bd[si:ei], mse_partial=r_mse[3 * si:3 * ei])
    torch.cuda.synchronize()
    assert torch.equal(bd, r_bd) and torch.equal(mse, r_mse)
    # against the host restatement of the groups rule (test_multilabel_cpu.py checks that one against fp64 autograd);
    # 2e-5: test_kernels_gpu.py::test_trigger_forward_backward's bound for the single-kernel trigger
    noise_q = noise_c8[..., :3].float().permute(0, 3, 1, 2).cpu()
    r_out, _ = MR.trigger_groups_ref(x, noise_q, pm.cpu(), k1.cpu(), ps, rate)
    assert float((bd.cpu() - r_out).abs().max()) < 2e-5
    if groups > 1:
        assert not torch.equal(bd[:1], r_bd[-1:])
    d1, d2 = (torch.randn(n, 3, hw, hw, generator=gen).cuda() for _ in range(2))
    for with2 in (False, True):
        dn = torch.full((n, hw, hw, 8), 7.0, dtype=bf16, device="cuda")
        ops.trigger_groups_bwd(xc, noise_c8, pm, k1, ps, rate, d1, bd, l2, dn, pre_tanh=True, d_out2=d2 if with2 else None)
        ref = torch.full_like(dn, 7.0)
        for ci in range(groups):
            si, ei = ci * ps, min(ci * ps + ps, n)
            ops.trigger_bwd(xc[si:ei], noise_c8[si:ei], pm, k1[ci], rate, d1[si:ei], bd[si:ei], l2, ref[si:ei], pre_tanh=True,
                            d_out2=d2[si:ei] if with2 else None)
        torch.cuda.synchronize()
        assert torch.equal(dn.view(torch.int16), ref.view(torch.int16)), with2


# ---------------------------------------------------------------- CUnetEngine


def _run_engine(mods, m, x, labels, cot=None):
    """Forward (and backward with cotangent `cot` of the tanh output) of module m (on the GPU) through its engine's
    plans on a slot of exactly n images.  Returns (noise NCHW fp32 on the GPU, slot, engine)."""
    ops = mods["ops"]
    eng = m._net_engine()
    eng.refresh()
    n, _, hw, _ = x.shape
    slot = eng.slot("t", n, hw)
    ops.image_to_c8(x.cuda(), eng.input(slot))
    if labels is not None:
        eng.labels(slot).copy_(labels.to(torch.int32))
    eng.forward_plan(slot).run()
    y = eng.output(slot)[..., :3].float().permute(0, 3, 1, 2)
    if cot is not None:
        z = slot.buf("g.z", (n, hw, hw, 8))
        z.zero_()
        z[..., :3] = (cot.cuda() * (1 - y * y)).permute(0, 2, 3, 1).to(bf16)
        eng.backward_plan(slot).run()
    torch.cuda.synchronize()
    return y, slot, eng


def test_cunet_forward_backward_vs_golden(mods, golden):
    """test_engine_gpu.py::test_unet_forward_backward's checks and constants for the conditional generator: layer by
    layer and output against the bf16 emulation, output against the fp32 golden no further than the emulation (x 1.25),
    gradients against the teacher-forced emulation (4e-2) and against the golden (0.5, and x 1.6 of the emulation).

    The emulation reads the image as the engine stores it (multilabel_ref.stored_image: bf16 hi + bf16 lo); fed the
    unrounded fp32 image it sits 3.4e-2 from itself at this point (the UNet's small InstanceNorms are chaotic in the last
    bits of the input).  bf16_emu.unet_forward_emu, the UNet test's emulation, does not do this: the two emulations differ
    in that one point.  Measured on the
    MI355X (3 images, labels [0, 9, 4]): conv0_0 and the conditioned conv0_1 equal the emulation to four decimals,
    then a smooth rise to 1.7e-2 (upconv1_0); output against the emulation 1.77e-2, against fp32 3.90e-2 (emulation
    3.93e-2); gradients against the teacher-forced emulation 8.6e-3, against fp32 0.374 (emulation 0.354)."""
    from test_engine_gpu import flat_grads, sampled_err, stored
    g = golden("multilabel_step")
    nets = mods["nets"]
    m = seeded(lambda: nets.CUnetGeneratorv1(Opt()), int(g["cunet/seed"]))
    names = [k for k, _ in m.named_parameters()]
    p = {k: v.clone().requires_grad_(True) for k, v in m.state_dict().items()}
    x, labels, cot = T(g["cunet/x"]), T(g["cunet/labels"]), T(g["cunet/g"])
    taps = {}
    y_emu = MR.cunet_forward_emu(p, x, labels, 10, taps)
    ge = torch.autograd.grad(y_emu, [p[k] for k in names], cot, allow_unused=True)
    ge = [torch.zeros_like(p[k]) if a is None else a for k, a in zip(names, ge)]
    m = m.cuda()
    y, slot, eng = _run_engine(mods, m, x, labels, cot)
    errs = {k: rel_l2(slot.bufs["t." + k].float().permute(0, 3, 1, 2), v.detach()) for k, v in taps.items()}
    e_out = rel_l2(y, y_emu.detach())
    e_fp32, emu_fp32 = rel_l2(y, T(g["cunet/y"])), rel_l2(y_emu.detach(), T(g["cunet/y"]))
    ours = flat_grads(eng.fp, names)
    force = stored(slot, ["t." + k for k in taps] + ["up0", "up1", "up2", "up3", "noise"], 3)
    pf = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    y_f = MR.cunet_forward_emu(pf, x, labels, 10, force=force)
    gf = torch.autograd.grad(y_f, [pf[k] for k in names], cot, allow_unused=True)
    gf = [torch.zeros_like(pf[k]) if a is None else a for k, a in zip(names, gf)]
    e_tf = rel_l2(ours, torch.cat([a.reshape(-1) for a in gf]))
    g_fp32 = sampled_err(g, "cunet/gp", [(k, eng.fp.logical(eng.fp.grad, k).cpu()) for k in names])
    g_emu_fp32 = sampled_err(g, "cunet/gp", zip(names, ge))
    # every figure before the first assertion
    print("cunet layers vs emulation: " + " ".join("%s %.4f" % kv for kv in errs.items()))
    print("cunet forward: engine vs emulation %.4f, engine vs fp32 %.4f, emulation vs fp32 %.4f" % (e_out, e_fp32, emu_fp32))
    print("cunet gradients: vs teacher-forced emulation %.4f, engine vs fp32 %.4f, emulation vs fp32 %.4f" % (e_tf, g_fp32, g_emu_fp32))
    assert errs["conv0_0"] < 1e-3 and errs["conv0_1"] < 3e-3 and errs["conv1_0"] < 5e-3, errs
    assert max(errs.values()) < 4e-2, errs
    assert e_out < 3e-2, (e_out, errs)                                # vs emulation
    assert e_fp32 < 5e-2 and e_fp32 < 1.25 * emu_fp32 + 1e-3, (e_fp32, emu_fp32)
    assert e_tf < 4e-2, e_tf                                          # vs teacher-forced emulation
    assert g_fp32 < 0.5 and g_fp32 < 1.6 * g_emu_fp32, (g_fp32, g_emu_fp32)
    # the merged parameter gradient: both parts against the teacher-forced emulation, absent classes exactly zero
    gw = eng.fp.logical(eng.fp.grad, "conv0_1.weight").cpu()
    gw_f = gf[names.index("conv0_1.weight")]
    assert rel_l2(gw[:, :64], gw_f[:, :64]) < 4e-2 and rel_l2(gw[:, 64:], gw_f[:, 64:]) < 4e-2
    for c in range(10):
        if c not in labels.tolist():
            assert float(gw[:, 64 + c].abs().max()) == 0.0
    assert float(gw[:, 64 + 9].abs().max()) > 0.0


def test_cunet_with_zero_label_weights_is_the_unet(mods):
    """With weight[:, nf:] zeroed, the output and the gradients of all shared parameters are UnetEngine's on the same
    weights, bit for bit: cond is an all-zero add_pre operand (a run-time feature of the launch: the same tile, the same
    kernel flavour), and conv0_1's W_f gradient is the same launch writing a scratch instead of the parameter's rows."""
    nets = mods["nets"]
    c = seeded(lambda: nets.CUnetGeneratorv1(Opt()), 21)
    u = seeded(lambda: nets.UnetGenerator(None), 22)
    with torch.no_grad():
        c.conv0_1.weight[:, 64:] = 0
        sd = {k: v.clone() for k, v in c.state_dict().items()}
        sd["conv0_1.weight"] = sd["conv0_1.weight"][:, :64].contiguous()
    u.load_state_dict(sd)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(5, 3, 32, 32, generator=gen) * 2 - 1
    cot = torch.randn(5, 3, 32, 32, generator=gen)
    labels = torch.tensor([0, 9, 4, 4, 7])
    engine = mods["engine"]
    was = engine.deterministic()
    engine.set_deterministic(True)      # weight gradients in a fixed summation order: comparable bit for bit
    try:
        yc, _, ec = _run_engine(mods, c.cuda(), x, labels, cot)
        yu, _, eu = _run_engine(mods, u.cuda(), x, None, cot)
    finally:
        engine.set_deterministic(was)
    assert torch.equal(yc, yu)
    for k, _ in u.named_parameters():
        a, b = ec.fp.logical(ec.fp.grad, k), eu.fp.logical(eu.fp.grad, k)
        if k == "conv0_1.weight":
            a = a[:, :64]
        assert torch.equal(a, b), k
    assert float(eu.fp.logical(eu.fp.grad, "conv1_0.weight").abs().max()) > 0.0


def test_cunet_module_call_conditions_on_the_label(mods):
    """netG(x, y) from Python: against the fp32 restatement, the same image under two labels gives different noise,
    padding rows and an empty batch are handled, a label outside the range is refused."""
    nets = mods["nets"]
    m = seeded(lambda: nets.CUnetGeneratorv1(Opt()), 5).cuda()
    x1 = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
    x = x1.repeat(3, 1, 1, 1)
    y = torch.tensor([2, 7, 2])
    out = m(x.cuda(), y.cuda())
    ref = MR.cunet_forward({k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}, x, y, 10)
    assert rel_l2(out, ref) < 5e-2          # vs fp32 (test_engine_gpu.py's module docstring)
    assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])
    assert rel_l2(out[1], out[0]) > 1e-2 and rel_l2(ref[1], ref[0]) > 1e-2
    assert tuple(m(torch.zeros(0, 3, 32, 32, device="cuda"), torch.zeros(0, dtype=torch.long)).shape) == (0, 3, 32, 32)
    with pytest.raises(ValueError):
        m(x.cuda(), torch.tensor([0, 10, 1]))
    with pytest.raises(Exception):
        m(x, y)  # CPU tensor: no fallback path


# ---------------------------------------------------------------- MultiLabelStep


def _step_nets(mods):
    from test_engine_gpu import _build
    netc, clean, _, netf = _build(mods, [0, 1, 2, 3])
    return netc, clean, seeded(lambda: mods["nets"].CUnetGeneratorv1(Opt()), 2), netf


def _step_opt():
    from test_engine_gpu import Opt as StepOpt
    return StepOpt()


SIGMAS = [0.7, 0.3, 0.9, 0.2, 0.55, 0.15, 0.8, 0.45]


def _packed_wf(mods, state):
    """conv0_1's packed forward operand of a generator with the given state_dict (on the CPU)."""
    m = mods["nets"].CUnetGeneratorv1(Opt())
    m.load_state_dict({k: v.clone() for k, v in state.items()})
    eng = m.cuda()._net_engine()
    eng.refresh()
    torch.cuda.synchronize()
    return eng.pc["conv0_1"].wf.cpu()


@pytest.mark.parametrize("b,nb", [(16, 3), (13, 0)])
def test_multilabel_step_vs_restatement(mods, b, nb):
    """Phase C from the identical start; Phase G teacher-forced from the engine's post-Phase-C state (as
    test_inputaware_gpu.py::test_inputaware_step_vs_restatement and test_engine_gpu.py::test_alternated_step_vs_oracle,
    whose tolerances these are).  b = 16: eight chunks of two; b = 13: ps = 2, a short last chunk; num_bd 3 and 0."""
    import torch.nn.functional as F
    from oracle import combat_oracle as O
    from combat_amd import step as step_mod
    from test_engine_gpu import _oracle_state, flat_grads, stored
    nets = mods["nets"]
    netc, clean, netg, netf = _step_nets(mods)
    oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
    old_g = _oracle_state(netg)
    gen = torch.Generator().manual_seed(5 + b)
    x = (torch.randint(0, 256, (b, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    t = torch.randint(0, 10, (b,), generator=gen)
    sc = 0.4
    bounds = MR.chunk_bounds(b, 10)
    sig = SIGMAS[:len(bounds)]
    chunk = torch.cat([torch.full((ei - si,), ci, dtype=torch.long) for ci, si, ei in bounds])
    cfg = O.StepConfig(lr_g=1e-3)
    emu_gen = lambda p, xx, yy: MR.cunet_forward_emu(p, xx, yy, 10)
    ref = MR.multilabel_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)),
                             x, t, MR.Randomness(nb, sc, sig), cfg, clf_fn=E.preact_forward_emu, gen_fn=emu_gen)
    netc, clean, netg, netf = netc.cuda(), clean.cuda().eval(), netg.cuda(), netf.cuda().eval()
    st = step_mod.MultiLabelStep(netc, netg, clean, netf, _step_opt())
    st.keep_grads = True
    st.run(x.cuda(), t, step_mod.MultiLabelRandomness(nb, sc, sig[0], [None] * 5, sigma_chunks=sig), lr_g=1e-3)
    torch.cuda.synchronize()
    m = st.read_metrics()
    tol = lambda r: 1e-2 * max(1.0, abs(r))
    # ---- Phase C
    print("loss_c %.5f / %.5f" % (m["loss_c_sum"], ref["loss_c"]))
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"])
    gn_c = float(st.eC.fp.grad.double().norm())
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G, teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    names_g = O.trainable_names(old_g)
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + nm for nm, *_ in nets.UNET_LAYERS] + ["up0", "up1", "up2", "up3", "noise"]
    assert st.eG.labels(st.sG).cpu().tolist() == chunk.tolist()
    noise = MR.cunet_forward_emu(pg, x, chunk, 10, force=stored(st.sG, keys, 3))
    ibd = torch.cat([O.trigger_mix(x[si:ei], noise[si:ei], 0.08, 0.65, sig[ci]) for ci, si, ei in bounds])
    assert float((st.bd.cpu() - ibd.detach()).abs().max()) < 3e-5
    leaf = ibd.detach().clone().requires_grad_(True)
    pred_bd = E.preact_forward_emu(oc2, leaf, False)
    cm_pred = E.preact_forward_emu(ok, leaf, False)
    loss_ce, cm_loss = F.cross_entropy(pred_bd, chunk), F.cross_entropy(cm_pred, t)
    for ours, r in (("loss_ce_sum", loss_ce), ("clean_model_loss_sum", cm_loss)):
        r = float(r.detach())
        print("%s %.5f / %.5f" % (ours, m[ours], r))
        assert abs(m[ours] - r) < tol(r), (ours, m[ours], r)
    assert abs(m["loss_l2_sum"] - float(F.mse_loss(ibd, x))) < 1e-5
    assert abs(m["bd_correct"] - int((pred_bd.argmax(1) == chunk).sum())) <= 1
    assert abs(m["clean_model_bd_asr"] - int((cm_pred.argmax(1) == chunk).sum())) <= 1
    assert abs(m["clean_model_bd_ba"] - int((cm_pred.argmax(1) == t).sum())) <= 1
    total = (ibd * (st.d_bd + st.d_bd2).cpu()).sum() + 0.02 * F.mse_loss(ibd, x)
    gr = torch.autograd.grad(total, [pg[k] for k in names_g], allow_unused=True)
    gr = torch.cat([(torch.zeros_like(pg[k]) if a is None else a).reshape(-1) for k, a in zip(names_g, gr)])
    e = rel_l2(flat_grads(st.eG.fp, names_g), gr)
    print("generator gradient vs teacher-forced emulation: %.3e" % e)
    assert e < 5e-2
    fp = st.eG.fp
    for k in ("conv0_0.weight", "conv0_1.weight", "conv3_1.weight", "upconv0_0.bias", "upconv1_0.bias"):
        exp = old_g[k] - 1e-3 * 1.9 * (fp.logical(fp.grad, k).cpu() + 5e-4 * old_g[k])
        assert rel_l2(netg.state_dict()[k].detach().cpu(), exp) < 1e-6, k
    # ---- after the update: W_f's packed operand must come from the NEW weights (CUnetEngine.refresh copies
    # weight[:, :nf] into the operand's master).  The stepped generator against a module built fresh from its
    # state_dict, same images and labels: the same launches over the same operands, bit for bit; and not the old noise.
    noise_before = st.eG.output(st.sG)[..., :3].float().permute(0, 3, 1, 2).clone()
    fresh = nets.CUnetGeneratorv1(Opt())
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in netg.state_dict().items()})
    y_new, _, eng_new = _run_engine(mods, netg, x, chunk)
    y_fresh, _, eng_fresh = _run_engine(mods, fresh.cuda(), x, chunk)
    w_new = netg.state_dict()["conv0_1.weight"]
    assert torch.equal(eng_new.wf01.permute(0, 3, 1, 2), w_new[:, :64]) and not torch.equal(w_new.cpu(), old_g["conv0_1.weight"])
    assert torch.equal(eng_new.pc["conv0_1"].wf, eng_fresh.pc["conv0_1"].wf)
    assert not torch.equal(eng_new.pc["conv0_1"].wf.cpu(), _packed_wf(mods, old_g))
    assert torch.equal(y_new, y_fresh) and not torch.equal(y_new, noise_before)
    ref_new = MR.cunet_forward({k: v.detach().cpu().contiguous() for k, v in netg.state_dict().items()}, x, chunk, 10)
    assert rel_l2(y_new, ref_new) < 5e-2          # vs fp32 (test_engine_gpu.py's module docstring)


def test_multilabel_step_is_deterministic(mods):
    """Two steps (40 images with num_bd 4, then 24 with num_bd 0) twice from the same seeds in deterministic mode: the
    same metrics and bit-identical parameters."""
    from combat_amd import step as step_mod
    engine = mods["engine"]
    gen = torch.Generator().manual_seed(9)
    x = (torch.randint(0, 256, (40, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    t = torch.randint(0, 10, (40,), generator=gen)
    prev = engine.deterministic()
    engine.set_deterministic(True)
    out = []
    try:
        for _ in range(2):
            netc, clean, netg, netf = (mm.cuda() for mm in _step_nets(mods))
            o = _step_opt()
            o.kernel_size = 5          # ignored: the step's blur is the reference's fixed 3-tap one
            st = step_mod.MultiLabelStep(netc, netg, clean.eval(), netf.eval(), o)
            assert st.opt.kernel_size == 3 and o.kernel_size == 5
            sig = [0.2 + 0.07 * i for i in range(10)]
            st.run(x.cuda(), t, step_mod.MultiLabelRandomness(4, 0.4, sig[0], [None] * 5, sigma_chunks=sig))
            st.run(x[:24].cuda(), t[:24], step_mod.MultiLabelRandomness(0, 0.5, sig[1], [None] * 5, sigma_chunks=sig[1:9]))
            torch.cuda.synchronize()
            out.append((st.read_metrics(), torch.cat([p.detach().flatten() for p in netc.parameters()]).clone(),
                        torch.cat([p.detach().flatten() for p in netg.parameters()]).clone()))
    finally:
        engine.set_deterministic(prev)
    (m0, c0, g0), (m1, c1, g1) = out
    assert m0 == m1
    assert torch.equal(c0, c1) and torch.equal(g0, g1)
    assert m0["samples"] == 64 and np.isfinite(m0["loss_ce_sum"]) and m0["loss_ce_sum"] > 0


# ---------------------------------------------------------------- the two scripts on synthetic data


def test_multilabel_workflow_on_synthetic_data(tmp_path):
    """One short --synthetic run of train_generator_multilabel.py and of train_victim_multilabel.py (training epoch +
    the per-class evaluation): the checkpoint layout and finite metrics."""
    import subprocess
    from test_multilabel_cpu import GEN_KEYS
    cwd = str(tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(script, *args, cwd):
        cmd = [sys.executable, os.path.join(root, script), "--synthetic", "--synthetic_size", "128", "--bs", "64",
               "--checkpoints", os.path.join(cwd, "ckpt"), "--allow_missing_F", "--log_interval", "1"] + list(args)
        r = subprocess.run(cmd, cwd=cwd, env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
        return r.stdout

    run("train_clean_classifier.py", "--saving_prefix", "classifier_clean", "--n_iters", "1", cwd=cwd)
    for script, prefix in (("train_generator_multilabel.py", "multilabel"), ("train_victim_multilabel.py", "victim_multilabel")):
        out = run(script, "--saving_prefix", prefix, "--load_checkpoint_clean", "classifier_clean", "--n_iters", "1", cwd=cwd)
        assert "Clean Model Bd ASR:" in out and "Saving..." in out, out[-2000:]
        sd = torch.load(os.path.join(cwd, "ckpt", prefix + "_clean", "cifar10", "cifar10_%s_clean.pth.tar" % prefix),
                        map_location="cpu", weights_only=True)
        assert set(sd) == GEN_KEYS
        for k in ("best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
                  "best_clean_model_bd_asr"):
            assert np.isfinite(sd[k]) and 0.0 <= sd[k] <= 100.0, (k, sd[k])
        assert sd["mask"].shape == (32, 32) and float(sd["mask"].sum()) == pytest.approx(1.6)
        assert sd["pattern"].shape == (3, 32, 32)
        assert tuple(sd["netG"]["conv0_1.weight"].shape) == (64, 74, 3, 3)
        assert sd["optimizerG"]["param_groups"][0]["lr"] == pytest.approx(1e-3)      # lr_C * 0.1
        assert all(torch.isfinite(v).all() for v in sd["netG"].values())
        assert all(torch.isfinite(v).all() for v in sd["netC"].values() if v.dtype.is_floating_point)
