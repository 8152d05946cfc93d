"""The imperceptible (total-variation) attack at ImageNet-10's 224 x 224 on the MI355X: combat_trigger_tv_big_fwd / _bwd
(the strip route, 80 <= hw <= 256, hw % 16 == 0), ImperceptibleStep at hw = 224 and train_generator_imperceptible.py with
--dataset imagenet10.

Shapes of the kernel tests: (hw, n) = (80, 3) is the smallest strip size (five strips, seams at rows 16 .. 64), (224, 2)
the real size; 256 is used for the runs of images only (85 clamp-mask rows fit a stream's 2 MB scratch).

Inputs of the kernel tests (kernel_case): x = (rand * 2 - 1) * 0.8 -- the low-pass of the noise reaches |L| of about 2.0,
so 0.8 + 0.08 * 2.0 stays clear of the clamp -- with one half plane at +2.0 and one at -2.0: saturated whatever the noise,
their blurred output is constant and sgn(0) = 0 decides on many seam rows and columns.  On the CPU oracle in fp64 the
nearest pre-clamp value to +-1 is 0.067 at (80, 3) and 0.076 at (224, 2), so the fp32 clamp mask cannot differ from the
oracle's; exact ties among the neighbour differences of the oracle's fp32 `out` are 32 % and 49 %; the TV share of the
noise gradient has 0.93 of the norm of the rest (tv_scale 0.5, l2 0.3, Gaussian d_out).  Every kernel test asserts the
margin, the tie share on the kernel's own `out` bits and a non-tie on a seam row before it relies on them.

Bounds: tv_partial rel-L2 1e-4 (test_imperceptible_gpu.py::test_tv_forward), d_noise rel-L2 4e-3
(test_trigger_big_gpu.py::test_trigger_big_forward_backward), the step's as in
test_imagenet10_unet_gpu.py::test_alternated_step_imagenet10_shape_b4; everything else is torch.equal against the plain
combat_trigger_fwd / _bwd calls.  DESIGN.md section 15 records what these tests measured on the MI355X."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402
import imperceptible_ref as R  # noqa: E402
from test_engine_gpu import _oracle_state, flat_grads, rel_l2, stored  # noqa: E402
from test_imagenet10_unet_gpu import _nets224, _opt224  # noqa: E402
from test_oracle_golden import synth_images  # noqa: E402

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imperceptible_step.npz")
RATE, RATIO, SIGMA = 0.08, 0.65, 0.6
TV_SCALE, L2 = 0.5, 0.3
EINVAL, OK = -1, 0
SHAPES = [(80, 3), (224, 2)]


@pytest.fixture(scope="module")
def ops():
    from combat_amd import ops as o
    return o


def bits(t):
    return t.view(torch.int16) if t.dtype == bf16 else t.view(torch.int32)


def nchw(dn):
    """Channels 0..2 of a c8 gradient as fp32 NCHW on the host."""
    return dn[..., :3].float().permute(0, 3, 1, 2).cpu()


def fixture_tv_weight():
    return float(np.load(GOLDEN)["tv_weight"])


# ------------------------------------------------------------------ the kernels
@functools.lru_cache(maxsize=None)
def kernel_case(hw, n):
    """Inputs shared by the kernel tests of one shape, never modified: the operands on the host and on the device, the
    fp64 clamp margin, and the forward's results (out, mse_partial, tv_partial of combat_trigger_tv_big_fwd)."""
    from combat_amd import ops, trigger
    from oracle import combat_oracle as O
    gen = torch.Generator().manual_seed(hw * 1000 + n)
    x = (torch.rand(n, 3, hw, hw, generator=gen) * 2 - 1) * 0.8
    x[0, :, : hw // 2] = 2.0
    x[1, :, :, : hw // 2] = -2.0
    noise = torch.tanh(torch.randn(n, 3, hw, hw, generator=gen) * 3).to(bf16).float()
    d_out, d_out2 = (torch.randn(n, 3, hw, hw, generator=gen) for _ in range(2))
    n8 = torch.zeros(n, hw, hw, 8, dtype=bf16, device="cuda")
    n8[..., :3] = noise.cuda().permute(0, 2, 3, 1).to(bf16)
    pre = x.double() + O.low_freq(noise.double(), RATIO) * RATE
    margin = float(torch.minimum((pre - 1).abs(), (pre + 1).abs()).min())
    pm = trigger.lowpass_matrix(hw, RATIO).cuda()
    k1 = torch.from_numpy(trigger.gaussian_kernel1d(SIGMA, 3)).cuda()
    xc = x.cuda()
    out, mse, tv = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(3 * n, device="cuda"), torch.empty(3 * n, device="cuda")
    ops.trigger_tv_fwd(xc, n8, pm, k1, RATE, out, tv, mse_partial=mse)
    torch.cuda.synchronize()
    return dict(x=x, xc=xc, noise=noise, n8=n8, pm=pm, k1=k1, margin=margin, out=out, mse=mse, tv=tv,
                d_out=d_out.cuda(), d_out2=d_out2.cuda())


def check_case(c, hw):
    """What the tests rely on: the clamp mask cannot differ from the oracle's, sgn(0) = 0 is exercised, and the sign
    stencil has work to do across a strip seam."""
    out = c["out"]
    dv, dh = out[..., 1:, :] - out[..., :-1, :], out[..., :, 1:] - out[..., :, :-1]
    ties = float(torch.cat([(dv == 0).flatten(), (dh == 0).flatten()]).float().mean())
    seam = int(sum(int((dv[..., r - 1, :] != 0).sum()) for r in range(16, hw, 16)))      # dv[r - 1] = out[r] - out[r - 1]
    print("fp64 clamp margin %.3g, ties %.3g, non-ties on seam rows %d" % (c["margin"], ties, seam))
    assert bool(torch.isfinite(out).all())
    assert c["margin"] > 1e-3
    assert ties > 1e-3
    assert seam >= 1


@functools.lru_cache(maxsize=None)
def sign_map(hw, n):
    """imperceptible_ref.tv_sign_stencil on the kernel's own out bits (device tensor, small integers: exact)."""
    return R.tv_sign_stencil(kernel_case(hw, n)["out"])


@pytest.mark.parametrize("hw,n", SHAPES)
def test_tv_big_forward(ops, hw, n):
    """out and mse_partial carry combat_trigger_fwd's bits; tv_partial against the fp64 sum over the kernel's own out
    bits; the same tv_partial bits without mse_partial, on a second launch and in both deterministic modes."""
    from combat_amd import engine
    c = kernel_case(hw, n)
    check_case(c, hw)
    xc, n8, pm, k1, out, mse, tv = (c[k] for k in ("xc", "n8", "pm", "k1", "out", "mse", "tv"))
    r_out, r_mse = torch.empty_like(out), torch.empty_like(mse)
    ops.trigger_fwd(xc, n8, pm, k1, RATE, r_out, mse_partial=r_mse)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(r_out)) and torch.equal(bits(mse), bits(r_mse))
    o = out.cpu().double()
    ref = (o[..., 1:, :] - o[..., :-1, :]).abs().sum((2, 3)) + (o[..., :, 1:] - o[..., :, :-1]).abs().sum((2, 3))
    e = rel_l2(tv.view(n, 3), ref)
    print("tv_partial rel_l2 hw=%d n=%d: %.3g" % (hw, n, e))
    assert e < 1e-4
    torch.testing.assert_close(ref.sum(1), R.total_variation(o), rtol=1e-12, atol=0)
    tv2, o2 = torch.full_like(tv, float("nan")), torch.empty_like(out)        # without mse_partial
    ops.trigger_tv_fwd(xc, n8, pm, k1, RATE, o2, tv2)
    torch.cuda.synchronize()
    assert torch.equal(bits(tv2), bits(tv)) and torch.equal(bits(o2), bits(out))
    prev = engine.deterministic()
    try:
        for mode in (False, True, False, True):
            engine.set_deterministic(mode)
            tv3, m3, o3 = torch.full_like(tv, float("nan")), torch.full_like(mse, float("nan")), torch.empty_like(out)
            ops.trigger_tv_fwd(xc, n8, pm, k1, RATE, o3, tv3, mse_partial=m3)
            torch.cuda.synchronize()
            assert torch.equal(bits(tv3), bits(tv)) and torch.equal(bits(m3), bits(mse)) and torch.equal(bits(o3), bits(out)), mode
    finally:
        engine.set_deterministic(prev)


@pytest.mark.parametrize("hw,n", SHAPES)
def test_tv_big_backward_exact(ops, hw, n):
    """tv_scale = 0.5, l2_scale = 0: 0.5 * S is exact in fp32 and the kernel's one fma rounds once, so the launch must
    write the bits of combat_trigger_bwd fed the explicit cotangent (the sign map S from the kernel's own out bits)."""
    c = kernel_case(hw, n)
    check_case(c, hw)
    xc, n8, pm, k1, out, d1, d2 = (c[k] for k in ("xc", "n8", "pm", "k1", "out", "d_out", "d_out2"))
    s = sign_map(hw, n)
    assert float(s.abs().max()) <= 4.0 and bool((s == s.round()).all())
    half_s = TV_SCALE * s
    both = (d1 + d2) + half_s                 # the kernel: fma(0.5, S, d_out + d_out2), one rounding after the sum's
    for pre in (False, True):
        a, b = (torch.full((n, hw, hw, 8), 7.0, dtype=bf16, device="cuda") for _ in range(2))
        ops.trigger_tv_bwd(xc, n8, pm, k1, RATE, None, out, 0.0, TV_SCALE, a, pre_tanh=pre)
        ops.trigger_bwd(xc, n8, pm, k1, RATE, half_s, None, 0.0, b, pre_tanh=pre)
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b)), ("tv alone", pre)
        assert float(a[..., :3].float().abs().max()) > 0 and float(a[..., 3:].float().abs().max()) == 0.0
        a, b = (torch.full((n, hw, hw, 8), 7.0, dtype=bf16, device="cuda") for _ in range(2))
        ops.trigger_tv_bwd(xc, n8, pm, k1, RATE, d1, out, 0.0, TV_SCALE, a, pre_tanh=pre, d_out2=d2)
        ops.trigger_bwd(xc, n8, pm, k1, RATE, both, None, 0.0, b, pre_tanh=pre)
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b)), ("two gradients", pre)
        assert float(a[..., 3:].float().abs().max()) == 0.0


@pytest.mark.parametrize("hw,n", SHAPES)
def test_tv_big_backward_vs_oracle(ops, hw, n):
    """All terms on, against autograd through oracle.trigger_mix with the cotangent d_out + d_out2 + 0.5 * S plus the L2
    term; tv_scale = 0 is combat_trigger_bwd."""
    from oracle import combat_oracle as O
    c = kernel_case(hw, n)
    check_case(c, hw)
    xc, n8, pm, k1, out, d1, d2 = (c[k] for k in ("xc", "n8", "pm", "k1", "out", "d_out", "d_out2"))
    x = c["x"]
    s = sign_map(hw, n).cpu()
    leaf = c["noise"].clone().requires_grad_(True)
    o_ref = O.trigger_mix(x, leaf, RATE, RATIO, SIGMA)
    (g_tv,) = torch.autograd.grad((o_ref * (TV_SCALE * s)).sum(), leaf, retain_graph=True)
    (g_rest,) = torch.autograd.grad((o_ref * (d1 + d2).cpu()).sum() + L2 * ((o_ref - x) ** 2).sum(), leaf)
    dn = torch.full((n, hw, hw, 8), 7.0, dtype=bf16, device="cuda")
    ops.trigger_tv_bwd(xc, n8, pm, k1, RATE, d1, out, L2, TV_SCALE, dn, d_out2=d2)
    e, share = rel_l2(nchw(dn), g_rest + g_tv), rel_l2(g_rest + g_tv, g_rest)
    print("all-terms bwd rel_l2 hw=%d n=%d: %.3g  (|tv part| / |rest| = %.3g, moves the result by %.3g)"
          % (hw, n, e, float(g_tv.norm() / g_rest.norm()), share))
    assert e < 4e-3
    assert share > 0.2                               # the TV part is no rounding error of the whole
    assert float(dn[..., 3:].float().abs().max()) == 0.0
    for pre in (False, True):
        a, b = torch.full_like(dn, 3.0), torch.full_like(dn, 3.0)
        ops.trigger_tv_bwd(xc, n8, pm, k1, RATE, d1, out, L2, 0.0, a, pre_tanh=pre, d_out2=d2)
        ops.trigger_bwd(xc, n8, pm, k1, RATE, d1, out, L2, b, pre_tanh=pre, d_out2=d2)
        torch.cuda.synchronize()
        assert torch.equal(bits(a), bits(b)), pre


def test_tv_big_runs_of_images(ops):
    """hw = 256, n = 86: the clamp mask of one image is 24 KB, so the launcher takes the batch as runs of 85 and 1 images,
    which must write the bits of two separate calls on those runs (the stencil's `out` offset per run included)."""
    from combat_amd import trigger
    hw, n, run = 256, 86, 85
    gen = torch.Generator(device="cuda").manual_seed(256086)
    x = (torch.rand(n, 3, hw, hw, generator=gen, device="cuda") * 2 - 1) * 0.8
    n8 = torch.zeros(n, hw, hw, 8, dtype=bf16, device="cuda")
    n8[..., :3] = torch.tanh(torch.randn(n, hw, hw, 3, generator=gen, device="cuda") * 3).to(bf16)
    d_out = torch.randn(n, 3, hw, hw, generator=gen, device="cuda")
    pm = trigger.lowpass_matrix(hw, RATIO).cuda()
    k1 = torch.from_numpy(trigger.gaussian_kernel1d(SIGMA, 3)).cuda()
    out, tv = torch.empty(n, 3, hw, hw, device="cuda"), torch.empty(3 * n, device="cuda")
    ops.trigger_tv_fwd(x, n8, pm, k1, RATE, out, tv)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tv).all()) and float(tv.min()) > 0
    l2s = 0.02 / out.numel()
    whole = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    parts = torch.full((n, hw, hw, 8), float("nan"), dtype=bf16, device="cuda")
    ops.trigger_tv_bwd(x, n8, pm, k1, RATE, d_out, out, l2s, TV_SCALE, whole, pre_tanh=True)
    for lo, hi in ((0, run), (run, n)):
        ops.trigger_tv_bwd(x[lo:hi], n8[lo:hi], pm, k1, RATE, d_out[lo:hi], out[lo:hi], l2s, TV_SCALE, parts[lo:hi], pre_tanh=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole.float()).all())
    assert torch.equal(bits(whole), bits(parts))


def test_tv_big_refusals():
    """COMBAT_EINVAL with nothing launched (the buffers keep their NaN / sentinel fill, and are sized for the largest hw
    asked for), n == 0 is COMBAT_OK, and the whole-plane entry point keeps refusing 224."""
    from combat_amd._lib import lib
    st = torch.cuda.current_stream().cuda_stream
    hw = 272
    x = torch.zeros(1, 3, hw, hw, device="cuda")
    n8 = torch.zeros(1, hw, hw, 8, dtype=bf16, device="cuda")
    pm = torch.zeros(hw, hw, device="cuda")
    k1 = torch.tensor([0.25, 0.5, 0.25], device="cuda")
    out = torch.full_like(x, float("nan"))
    dn = torch.full_like(n8, 5.0)
    mse, tv = torch.full((3,), -7.0, device="cuda"), torch.full((3,), float("nan"), device="cuda")
    before = [bits(t).clone() for t in (out, dn, mse, tv)]
    p = lambda t: t.data_ptr() if t is not None else None

    def fwd(n, hw, o=out, t=tv):
        return lib.combat_trigger_tv_big_fwd(p(x), p(n8), p(pm), p(k1), RATE, n, hw, p(o), p(mse), p(t), st)

    def bwd(n, hw, o=out, tvs=TV_SCALE):
        return lib.combat_trigger_tv_big_bwd(p(x), p(n8), p(pm), p(k1), RATE, n, hw, p(x), None, p(o), 0.0, tvs, 0, p(dn), st)

    for call in (fwd, bwd):
        assert call(1, 64) == EINVAL        # the whole-plane entry points' size
        assert call(1, 72) == EINVAL        # not a multiple of 16
        assert call(1, 272) == EINVAL       # more columns than a workgroup has threads
        assert call(-1, 224) == EINVAL
        assert call(1, 224, o=None) == EINVAL
        assert call(0, 224) == OK and call(0, 80) == OK and call(0, 256) == OK
    assert fwd(1, 224, t=None) == EINVAL
    assert bwd(1, 64, tvs=0.0) == EINVAL    # the size rule comes before the tv_scale == 0 delegation
    assert lib.combat_trigger_tv_bwd(p(x), p(n8), p(pm), p(k1), RATE, 1, 224, p(x), None, p(out), 0.0, TV_SCALE, 0, p(dn), st) == EINVAL
    assert lib.combat_trigger_tv_fwd(p(x), p(n8), p(pm), p(k1), RATE, 1, 224, p(out), p(mse), p(tv), st) == EINVAL
    torch.cuda.synchronize()
    for t, b in zip((out, dn, mse, tv), before):
        assert torch.equal(bits(t), b)       # nothing was launched


# ------------------------------------------------------------------ the step
def _tv_opt(tv_weight):
    opt = _opt224()
    opt.tv_weight = tv_weight
    return opt


def _params(net):
    return torch.cat([p.detach().flatten() for p in net.parameters()]).clone()


def test_imperceptible_step_imagenet10_shape_b4():
    """One imperceptible step at 3 x 224 x 224, 10 classes, ResNet18(input_size=224), b = 4, against
    tests/imperceptible_ref.py driven with the bf16-emulating networks.  Method of
    test_imperceptible_gpu.py::test_imperceptible_step_vs_restatement, tolerances of
    test_imagenet10_unet_gpu.py::test_alternated_step_imagenet10_shape_b4: Phase C from the identical start (loss 1e-2,
    gradient norm 3e-2); Phase G from the engine's post-Phase-C classifier with the generator emulation teacher-forced
    (triggered images 3e-5, losses 1e-2 * max(1, |ref|), loss_tv 1e-3, generator gradient 5e-2).  The sign map of the
    cotangent comes from the engine's own inputs_bd bits, so every pixel is compared and no sign-flip allowance exists."""
    from combat_amd import nets, step as step_mod
    from oracle import combat_oracle as O
    b, tvw = 4, fixture_tv_weight()
    netc, clean, netg, netf = _nets224()
    oc, ok, og, of = (_oracle_state(m) for m in (netc, clean, netg, netf))
    old_g = _oracle_state(netg)
    x = synth_images(b, 224, 5)
    t = torch.randint(0, 10, (b,), generator=torch.Generator().manual_seed(6))
    t[::2][:2] = 0
    nb, sc, sg = 1, 0.5, 0.9
    cfg = O.StepConfig(num_classes=10, classifier="resnet18")
    ref = R.imperceptible_step(oc, og, ok, of, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)), x, t,
                               O.StepRandomness(nb, sc, sg, [None] * 5), cfg, tvw, clf_fn=E.resnet_forward_emu,
                               gen_fn=E.unet_forward_emu)
    st = step_mod.ImperceptibleStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _tv_opt(tvw))
    st.keep_grads = True
    st.run(x.cuda(), t, step_mod.StepRandomness(nb, sc, sg, [None] * 5))
    torch.cuda.synchronize()
    m = st.read_metrics()
    assert all(np.isfinite(v) for v in m.values()), m
    tol = lambda r: 1e-2 * max(1.0, abs(r))
    gn_c = float(st.eC.fp.grad.double().norm())
    print("loss_c %.5f / %.5f, gnorm_c %.5f / %.5f" % (m["loss_c_sum"], ref["loss_c"], gn_c, ref["gnorm_c"]))
    assert abs(m["loss_c_sum"] - ref["loss_c"]) < tol(ref["loss_c"]), (m["loss_c_sum"], ref["loss_c"])
    assert abs(gn_c - ref["gnorm_c"]) < 3e-2 * ref["gnorm_c"], (gn_c, ref["gnorm_c"])
    # ---- Phase G from the engine's post-Phase-C classifier, the generator emulation teacher-forced
    oc2 = {k: v.detach().cpu().clone() for k, v in netc.state_dict().items()}
    names_g = O.trainable_names(old_g)
    pg = {k: v.clone().requires_grad_(k in names_g) for k, v in old_g.items()}
    keys = ["t." + nm for nm, *_ in nets.UNET_LAYERS] + ["up0", "up1", "up2", "up3", "noise"]
    noise = E.unet_forward_emu(pg, x, force=stored(st.sG, keys, 3))
    ibd = O.trigger_mix(x, noise, RATE, RATIO, sg)
    e_bd = float((st.bd.cpu() - ibd.detach()).abs().max())
    print("bd %.3g" % e_bd)
    assert e_bd < 3e-5
    bd_t = torch.zeros_like(t)
    with torch.no_grad():
        pred_bd = E.resnet_forward_emu(oc2, ibd.detach(), False)
        cm_pred = E.resnet_forward_emu(ok, ibd.detach(), False)
    for ours, r in (("loss_ce_sum", F.cross_entropy(pred_bd, bd_t)), ("clean_model_loss_sum", F.cross_entropy(cm_pred, t))):
        r = float(r)
        print("%s %.5f / %.5f" % (ours, m[ours], r))
        assert abs(m[ours] - r) < tol(r), (ours, m[ours], r)
    l2 = float(F.mse_loss(ibd.detach(), x))
    assert abs(m["loss_l2_sum"] - l2) < 1e-3 * l2 + 1e-7
    tv_ref = float(R.total_variation(ibd.detach().double()).mean())
    print("loss_tv: step %.6f restatement (teacher-forced) %.6f" % (m["loss_tv_sum"], tv_ref))
    assert abs(m["loss_tv_sum"] - tv_ref) < 1e-3 * tv_ref
    # the engine's own classifier gradients as cotangent, the sign map from the engine's own inputs_bd bits
    tv_cot = (tvw / b) * R.tv_sign_stencil(st.bd.cpu())
    cot = (st.d_bd + st.d_bd2).cpu() + tv_cot
    print("|tv cotangent| / |classifier cotangent| = %.3g" % float(tv_cot.norm() / (st.d_bd + st.d_bd2).cpu().norm()))
    total = (ibd * cot).sum() + 0.02 * F.mse_loss(ibd, x)
    gr = torch.autograd.grad(total, [pg[k] for k in names_g], allow_unused=True)
    gr = torch.cat([(torch.zeros_like(pg[k]) if a is None else a).reshape(-1) for k, a in zip(names_g, gr)])
    e_g = rel_l2(flat_grads(st.eG.fp, names_g), gr)
    print("generator gradient vs teacher-forced emulation %.3g" % e_g)
    assert e_g < 5e-2      # teacher-forced: pins the strip TV backward + the UNet backward at 224 x 224


def test_tv_weight_zero_is_the_alternated_step_at_224():
    """b = 4, deterministic mode: parameters, momentum buffers and every parent metric bit for bit, and loss_tv_sum is
    reported (the forward's TV partials do not depend on the weight)."""
    from combat_amd import engine, step as step_mod
    b = 4
    x = synth_images(b, 224, 5).cuda()
    t = torch.randint(0, 10, (b,), generator=torch.Generator().manual_seed(6))
    t[::2][:2] = 0
    prev = engine.deterministic()
    engine.set_deterministic(True)
    got = []
    try:
        for cls in (step_mod.AlternatedStep, step_mod.ImperceptibleStep):
            netc, clean, netg, netf = _nets224()
            g0 = _params(netg)
            st = cls(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _tv_opt(0.0))
            st.run(x, t, step_mod.StepRandomness(1, 0.5, 0.9, [None] * 5))
            torch.cuda.synchronize()
            got.append(dict(m=st.read_metrics(), c=_params(netc), g=_params(netg), g0=g0, mom_c=st.eC.fp.mom.clone(),
                            mom_g=st.eG.fp.mom.clone()))
    finally:
        engine.set_deterministic(prev)
    a, z = got
    for k in ("c", "g", "mom_c", "mom_g"):
        assert torch.equal(a[k], z[k]), k
    assert float((a["g"].cpu() - a["g0"]).abs().max()) > 0
    for k, v in a["m"].items():
        assert z["m"][k] == v, (k, z["m"][k], v)
    assert z["m"]["loss_tv_sum"] > 0 and "loss_tv_sum" not in a["m"]


def test_imperceptible_step_imagenet10_shape_b32():
    """The configuration's batch of 32: bd within 2e-5 of oracle.trigger_mix on the engine's own generator output,
    loss_tv_sum against the fp64 TV of the engine's own bd, finite parameters, and a second identical run in
    deterministic mode leaves the same parameter bits."""
    from combat_amd import engine, step as step_mod
    from oracle import combat_oracle as O
    b, sg, tvw = 32, 0.9, fixture_tv_weight()
    x = synth_images(b, 224, 5)
    t = torch.randint(0, 10, (b,), generator=torch.Generator().manual_seed(6))
    prev = engine.deterministic()
    engine.set_deterministic(True)
    got = []
    try:
        for i in range(2):
            netc, clean, netg, netf = _nets224()
            st = step_mod.ImperceptibleStep(netc.cuda(), netg.cuda(), clean.cuda().eval(), netf.cuda().eval(), _tv_opt(tvw))
            st.run(x.cuda(), t, step_mod.StepRandomness(3, 0.5, sg, [None] * 5))
            torch.cuda.synchronize()
            m = st.read_metrics()
            assert all(np.isfinite(v) for v in m.values()), m
            got.append((_params(netc), _params(netg)))
            if i == 0:
                noise = st.eG.output(st.sG)[..., :3].float().cpu().permute(0, 3, 1, 2)
                assert bool(torch.isfinite(noise).all())
                e_bd = float((st.bd.cpu() - O.trigger_mix(x, noise, RATE, RATIO, sg)).abs().max())
                tv_ref = float(R.total_variation(st.bd.double()).mean())
                print("bd %.3g, loss_tv %.6f / %.6f" % (e_bd, m["loss_tv_sum"], tv_ref))
                assert e_bd < 2e-5
                assert abs(m["loss_tv_sum"] - tv_ref) < 1e-4 * tv_ref
            del st
    finally:
        engine.set_deterministic(prev)
    for p in got[0]:
        assert bool(torch.isfinite(p).all())
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ------------------------------------------------------------------ the script
def test_imperceptible_workflow_imagenet10(tmp_path):
    """train_generator_imperceptible.py with --dataset imagenet10 (bs forced to 32; 64 synthetic images, one epoch): the
    epoch's scalars hold "TV Loss", the checkpoint layout is the one
    test_imperceptible_gpu.py::test_imperceptible_workflow_on_synthetic_data asserts at 32 x 32."""
    from test_attacks224_gpu import _ckpt, _clean_checkpoint, _finite, _script
    from test_imperceptible_gpu import GEN_KEYS
    cwd = str(tmp_path)
    clean = _clean_checkpoint(cwd)
    out = _script("train_generator_imperceptible.py", "--saving_prefix", "imperceptible", "--tv_weight", "0.001", *clean, cwd=cwd)
    assert "Clean Model Bd ASR:" in out and "Saving..." in out, out[-2000:]
    log_dir = os.path.join(cwd, "ckpt", "imperceptible_clean", "imagenet10", "log_dir")
    logged = out.encode()
    for folder, _, files in os.walk(log_dir):      # scalars.jsonl, or tensorboard's event files
        for f in files:
            logged += open(os.path.join(folder, f), "rb").read()
    assert b"TV Loss" in logged
    path = os.path.join(log_dir, "scalars.jsonl")
    if os.path.exists(path):
        import json
        rows = [json.loads(line)["values"] for line in open(path) if '"Clean Accuracy"' in line]
        assert len(rows) == 1 and rows[0]["TV Loss"] > 0 and np.isfinite(rows[0]["TV Loss"])
    sd = _ckpt(cwd, "imperceptible_clean")
    assert set(sd) == GEN_KEYS
    assert len(sd["netG"]) == 32 and len(sd["netC"]) == 122 and sd["netC"]["linear.weight"].shape == (10, 512 * 49)
    assert _finite(sd["netG"]) and _finite(sd["netC"]) and _finite(sd["clean_model"])
