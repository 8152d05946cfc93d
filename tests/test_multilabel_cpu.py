"""Host-side pieces of the multi-label attack's label-conditioned generator (reference networks/models.py:472-555,
train_generator_multilabel.py): the restatements of tests/multilabel_ref.py against the golden recorded from the
reference's own modules, the chunk arithmetic of the generator phase, the host restatements of the new kernels against
fp64 autograd over explicit one-hot planes, the module's state_dict layout and the entry points' place in the C ABI."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multilabel_ref as MR  # noqa: E402

bf16 = torch.bfloat16


class Opt:
    num_classes = 10


def T(a):
    return torch.from_numpy(np.asarray(a))


def _synth(b, seed):
    """tests/golden/make_golden.py::synth_images."""
    u8 = torch.randint(0, 256, (b, 3, 32, 32), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return (u8.float() / 255 - 0.5) / 0.5


def _state(ctor, seed):
    torch.manual_seed(seed)
    return {k: v.detach().clone() for k, v in ctor().state_dict().items()}


# ---------------------------------------------------------------- the module


def test_module_has_the_references_state_dict():
    """Keys, shapes and initial values of networks/models.py:472-521 under the same seed: conv0_1.weight is ONE
    [nf][nf + num_classes][3][3] parameter."""
    from combat_amd import nets
    g = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "multilabel_step.npz")))
    sd = _state(lambda: nets.CUnetGeneratorv1(Opt()), int(g["cunet/seed"]))
    assert tuple(sd["conv0_1.weight"].shape) == (64, 74, 3, 3)
    names = [k for k, _ in nets.CUnetGeneratorv1(Opt()).named_parameters()]
    assert names == [n + s for n, *_ in nets.UNET_LAYERS for s in (".weight", ".bias")]
    assert sorted(k[len("cunet/gp/"):-len("/l2")] for k in g if k.startswith("cunet/gp/") and k.endswith("/l2")) == sorted(names)

    class Opt8:
        num_classes = 8
    assert tuple(nets.CUnetGeneratorv1(Opt8()).conv0_1.weight.shape) == (64, 72, 3, 3)       # CelebA


def test_restated_forward_vs_reference_module(golden):
    """cunet_forward (fp32, explicit planes) against CUnetGeneratorv1's recorded output and parameter gradients for
    labels [0, 9, 4]: the same arithmetic in the same order, so fp32 round-off only."""
    from combat_amd import nets
    g = golden("multilabel_step")
    p = _state(lambda: nets.CUnetGeneratorv1(Opt()), int(g["cunet/seed"]))
    names = [k for k in p]
    for k in names:
        p[k].requires_grad_(True)
    x, y, cot = T(g["cunet/x"]), T(g["cunet/labels"]), T(g["cunet/g"])
    assert y.tolist() == [0, 9, 4]
    out = MR.cunet_forward(p, x, y, 10)
    torch.testing.assert_close(out.detach(), T(g["cunet/y"]), rtol=1e-5, atol=1e-6)
    grads = torch.autograd.grad(out, [p[k] for k in names], cot)
    gw = grads[names.index("conv0_1.weight")]
    ref = T(g["cunet/g_conv0_1_weight"])
    assert float((gw - ref).norm() / ref.norm()) < 1e-4
    # rows of the classes no image carries are exactly zero in the reference too
    absent = [c for c in range(10) if c not in (0, 9, 4)]
    assert float(ref[:, [64 + c for c in absent]].abs().max()) == 0.0
    for k, gk in zip(names, grads):
        idx, val = g["cunet/gp/%s/idx" % k], g["cunet/gp/%s/val" % k]
        scale = max(float(g["cunet/gp/%s/l2" % k]) / max(gk.numel(), 1) ** 0.5, 1e-12)
        assert np.abs(gk.double().flatten()[idx].numpy() - val).max() < 1e-3 * scale + 1e-7, k


def test_restated_step_vs_reference_modules(golden):
    """Two multi-label steps of tests/multilabel_ref.py::multilabel_step against the trace recorded from the reference's
    nn.Modules and torch.optim.SGD (tests/golden/make_golden_multilabel.py): b = 16, no augmentation, recorded num_bd (0,
    then 3) and per-chunk sigmas; the tolerances of test_inputaware_cpu.py::test_restatement_vs_reference_modules."""
    from oracle import combat_oracle as O
    from combat_amd import nets
    g = golden("multilabel_step")
    s0, s1, s2 = [int(s) for s in g["seeds"]]
    netc, clean = _state(nets.PreActResNet18, s0), _state(nets.PreActResNet18, s1)
    netg = _state(lambda: nets.CUnetGeneratorv1(Opt()), s2)
    bufs_c, bufs_g = [None] * len(O.trainable_names(netc)), [None] * len(O.trainable_names(netg))
    cfg = O.StepConfig(lr_c=float(g["lr_c"]), lr_g=float(g["lr_g"]))
    assert cfg.lr_g == pytest.approx(cfg.lr_c * 0.1) and int(g["ps"]) == MR.chunk_size(16, 10)
    assert g["num_bd"].tolist() == [0, 3]
    for s in range(2):
        x = _synth(16, 4234 + s)
        assert abs(float(x.double().sum()) - float(g["step%d/x_sum" % s])) < 1e-6
        t = T(g["step%d/targets" % s])
        assert T(g["step%d/chunk_classes" % s]).tolist() == [i // 2 for i in range(16)]
        rnd = MR.Randomness(int(g["num_bd"][s]), float(g["sigma_c"][s]), g["sigma_g"][s].tolist())
        out = MR.multilabel_step(netc, netg, clean, None, bufs_c, bufs_g, x, t, rnd, cfg)
        for k in ("loss_c", "loss_ce", "loss_l2", "clean_model_loss"):
            ref = float(g["trace/" + k][s])
            assert abs(out[k] - ref) <= 2e-4 * max(1.0, abs(ref)), (s, k, out[k], ref)
        for k in ("clean_correct", "bd_correct", "clean_model_correct", "clean_model_bd_ba", "clean_model_bd_asr"):
            assert out[k] == int(g["trace/" + k][s]), (s, k)
        ref = float(g["step%d/bd_sum" % s])
        assert abs(out["bd_sum"] - ref) <= 2e-4 * max(1.0, abs(ref)), (s, out["bd_sum"], ref)
    for prefix, named in (("final/netc", netc), ("final/netg", netg)):
        for k, v in named.items():
            idx, ref = g["%s/%s/idx" % (prefix, k)], g["%s/%s/val" % (prefix, k)]
            np.testing.assert_allclose(v.double().flatten()[idx].numpy(), ref, rtol=5e-3, atol=4e-4, err_msg=k)


def test_emulation_without_rounding_is_the_restatement():
    """cunet_forward_emu with bf16 rounding off is cunet_forward: the W_f / W_y split computes the concatenation."""
    from combat_amd import nets
    import bf16_emu as E
    p = _state(lambda: nets.CUnetGeneratorv1(Opt()), 11)
    x, y = _synth(2, 5), torch.tensor([7, 2])
    E.ROUND = False
    try:
        a = MR.cunet_forward_emu(p, x, y, 10)
    finally:
        E.ROUND = True
    b = MR.cunet_forward(p, x, y, 10)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=2e-5)


# ---------------------------------------------------------------- chunk arithmetic


@pytest.mark.parametrize("bs", [1, 10, 13, 16, 128])
def test_chunks_follow_the_references_loop(bs):
    """ps and the chunk list against a literal transcription of train_generator_multilabel.py:203-213, and what
    image i / ps says (the grouped trigger's and the label row's rule)."""
    for classes in (10, 8):
        ps = MR.chunk_size(bs, classes)
        assert ps == int((bs - 1) / classes) + 1 == (bs - 1) // classes + 1
        bounds = MR.chunk_bounds(bs, classes)
        assert bounds[0][1] == 0 and bounds[-1][2] == bs
        assert all(a[2] == b[1] for a, b in zip(bounds, bounds[1:]))
        assert len(bounds) == (bs + ps - 1) // ps <= classes
        for ci, si, ei in bounds:
            assert all(i // ps == ci for i in range(si, ei))
    if bs == 16:
        assert [c for c, _, _ in MR.chunk_bounds(16, 10)] == list(range(8))     # classes 8 and 9 never occur
    if bs == 13:
        assert MR.chunk_bounds(13, 10)[-1] == (6, 12, 13)                        # a short last chunk


# ---------------------------------------------------------------- host restatements of the kernels


def _weight(nf, classes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(nf, nf + classes, 3, 3, generator=g) * 0.05


@pytest.mark.parametrize("s,n,classes", [(2, 1, 10), (3, 5, 8), (16, 5, 10)])
def test_cond_restatement_vs_fp64_planes(s, n, classes):
    """cond_ref against fp64 F.conv2d over explicit one-hot planes: at most nine fp32 adds and one bf16 rounding, so
    within half a bf16 ulp (2^-8 relative: 8 significant bits) plus the fp32 sum's error."""
    nf = 64
    w = _weight(nf, classes, 3)
    labels = torch.tensor(([0, classes - 1, 3, classes - 1, 0] * 2)[:n])
    got = MR.cond_ref(MR.physical(w), labels, s).float().permute(0, 3, 1, 2)
    ref = MR.cond_planes_f64(w[:, nf:], labels, s)
    err = (got.double() - ref).abs()
    assert float((err - (2.0 ** -8 + 9 * 2.0 ** -24) * ref.abs()).max()) <= 1e-30
    assert float(ref.abs().max()) > 0.01


def test_cond_restatement_out_of_range_label_is_zero():
    w = MR.physical(_weight(64, 10, 4))
    out = MR.cond_ref(w, torch.tensor([10, -1, 2]), 4)
    assert float(out[:2].abs().max()) == 0.0 and float(out[2].abs().max()) > 0.0


# fp32 summation bound of cond_wgrad_ref against fp64, stated for the GPU test as well.  Every output is a sum of
# at most n * s * s bf16 values (exact in fp32) added in a tree of depth <= steps + L + 9 + n; with |d| <= A the error
# of such a sum is <= depth * 2^-24 * (n * s * s * A).  Measured here on the CPU (this test prints it) at n = 5, s = 16:
# 4.8e-7 absolute, 5e-8 of max |dW_y|, against a bound of 2.0e-3 (the bound is the worst case of the order, not a fit).
def wgrad_bound(n, s, nf, amax):
    L = 256 // (nf // 8)
    depth = (s * s + L - 1) // L + L + 9 + n
    return depth * 2.0 ** -24 * n * s * s * amax


@pytest.mark.parametrize("s,labels,classes", [(2, [3], 10), (3, [0, 7, 7, 2, 0], 8), (16, [0, 9, 4, 9, 0], 10),
                                              (16, [5, 5, 5, 5, 5], 10)])
def test_cond_wgrad_restatement_vs_fp64_autograd(s, labels, classes):
    nf, n = 64, len(labels)
    labels = torch.tensor(labels)
    d = (torch.randn(n, s, s, nf, generator=torch.Generator().manual_seed(9)) * 0.1).to(bf16)
    dwf = torch.randn(nf, 9, nf, generator=torch.Generator().manual_seed(10))
    got = MR.cond_wgrad_ref(d, labels, classes, dwf)
    assert torch.equal(got[:, :, :nf], dwf)
    wy = torch.zeros(nf, classes, 3, 3, dtype=torch.float64, requires_grad=True)
    (gy,) = torch.autograd.grad(MR.cond_planes_f64(wy, labels, s), wy, d.double().permute(0, 3, 1, 2))
    ref = MR.physical(gy)                                        # [nf][9][classes]
    err = float((got[:, :, nf:].double() - ref).abs().max())
    print("cond_wgrad_ref vs fp64: max err %.3e, max |ref| %.3e, bound %.3e" % (err, float(ref.abs().max()),
                                                                                wgrad_bound(n, s, nf, float(d.float().abs().max()))))
    assert err <= wgrad_bound(n, s, nf, float(d.float().abs().max()))
    for c in range(classes):
        if c not in labels.tolist():
            assert float(got[:, :, nf + c].abs().max()) == 0.0      # an absent class: exactly zero
    assert float(ref.abs().max()) > 0.0


@pytest.mark.parametrize("n,ps", [(13, 2), (16, 16)])
def test_grouped_trigger_restatement_vs_fp64_autograd(n, ps):
    """trigger_groups_ref / _bwd_ref (image i blurred with k1[i // ps], a short last group at n = 13) against fp64 and
    its autograd through the oracle's per-chunk trigger_mix calls concatenated, as the reference's loop builds inputs_bd
    (train_generator_multilabel.py:207-222), with the MSE term's gradient and the tanh factor.
    Bound: every value is at most four nested fp32 dot products of length hw whose left factors are rows of P (an
    orthogonal projection: |row|_1 <= sqrt(hw)) or of a blur matrix (|row|_1 = 1), so the error is at most
    4 * hw * 2^-24 * hw * max |value|: 2.4e-4 of the largest entry at hw = 32."""
    from oracle import combat_oracle as O
    from combat_amd import trigger
    hw, rate, ratio, l2 = 32, 0.08, 0.65, 0.3
    gen = torch.Generator().manual_seed(n)
    x = _synth(n, 40 + n)
    noise = torch.tanh(torch.randn(n, 3, hw, hw, generator=gen))
    d_out = torch.randn(n, 3, hw, hw, generator=gen)
    groups = (n + ps - 1) // ps
    sig = [0.15 + 0.8 * i / max(groups - 1, 1) for i in range(groups)]
    k1 = torch.stack([torch.from_numpy(trigger.gaussian_kernel1d(s, 3)) for s in sig]).float()
    pm = trigger.lowpass_matrix(hw, ratio).float()
    out, mse = MR.trigger_groups_ref(x, noise, pm, k1, ps, rate)
    dn = MR.trigger_groups_bwd_ref(x, noise, pm, k1, ps, rate, d_out, out, l2, True)
    z = torch.atanh(noise.double()).requires_grad_(True)
    nz = torch.tanh(z)
    x64 = x.double()
    ref = torch.cat([O.trigger_mix(x64[si:min(si + ps, n)], nz[si:min(si + ps, n)], rate, ratio, sig[si // ps])
                     for si in range(0, n, ps)])
    assert ref.dtype == torch.float64
    (gz,) = torch.autograd.grad((ref * d_out.double()).sum() + l2 * ((ref - x64) ** 2).sum(), z)
    eps = 4 * hw * 2.0 ** -24 * hw
    e_out, e_mse, e_dn = (float((a.double() - b).abs().max()) for a, b in
                          ((out, ref.detach()), (mse, ((ref.detach() - x64) ** 2).sum((2, 3)).reshape(-1)), (dn, gz)))
    print("grouped trigger vs fp64: out %.2e, mse %.2e, d_noise %.2e" % (e_out, e_mse, e_dn))
    ref = ref.detach()
    assert e_out <= eps * float(ref.abs().max())
    assert e_mse <= hw * hw * 2 * eps * float(ref.abs().max()) * 2.0      # hw^2 squared differences |out - x| <= 2
    assert e_dn <= eps * max(float(gz.abs().max()), float(d_out.abs().max()))
    if groups > 1:       # the groups differ: image 0 under the last group's kernel is another image
        other, _ = MR.trigger_groups_ref(x[:1], noise[:1], pm, k1[-1:], 1, rate)
        assert float((other - out[:1]).abs().max()) > 1e-3


# ---------------------------------------------------------------- C ABI


def test_entry_points_and_abi():
    from combat_amd import _lib
    for name in ("combat_cond_fwd", "combat_cond_wgrad", "combat_trigger_groups_fwd", "combat_trigger_groups_bwd"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.combat_abi_version() >= 20


def test_entry_points_refuse_without_a_gpu():
    """The argument checks run before anything is launched (tools/cond_refusals.cpp runs the full list under sanitizers)."""
    from combat_amd._lib import lib
    A = 4096
    assert lib.combat_cond_fwd(A, A, 4, 1, 64, 10, A, None) == -1          # map size 1
    assert lib.combat_cond_fwd(A, A, 4, 16, 48, 10, A, None) == -1         # nf outside the set
    assert lib.combat_cond_fwd(A, A, 0, 16, 64, 10, A, None) == 0          # n == 0
    assert lib.combat_cond_wgrad(A, A, 4, 1, 64, 10, None, A, A, None) == -1
    assert lib.combat_cond_wgrad(A, A, 4, 16, 64, 10, None, A, None, None) == -1   # no scratch
    assert lib.combat_cond_wgrad(A, A, 0, 16, 64, 10, None, A, A, None) == 0
    assert lib.combat_trigger_groups_fwd(A, A, A, A, 0.08, 4, 32, 0, A, None, None) == -1    # ps < 1
    assert lib.combat_trigger_groups_bwd(A, A, A, A, 0.08, 4, 32, 2, A, None, None, 0.5, 1, A, None) == -1   # L2 term without out
    assert lib.combat_trigger_groups_fwd(A, A, A, A, 0.08, 0, 32, 2, A, None, None) == 0


def test_labels_are_checked_on_the_host():
    from combat_amd.engine import check_labels
    assert check_labels(torch.tensor([0, 9, 4]), 3, 10).dtype == torch.int32
    for bad in (torch.tensor([0, 10, 4]), torch.tensor([-1, 0, 0]), torch.tensor([0.0, 1.0, 2.0]), torch.tensor([0, 1])):
        with pytest.raises(ValueError):
            check_labels(bad, 3, 10)
    from combat_amd import api, nets
    with pytest.raises(ValueError):      # labels are required by the conditional generator, refused by the others
        api.create_backdoor(nets.CUnetGeneratorv1(Opt()), torch.zeros(2, 3, 32, 32), None)
    with pytest.raises(ValueError):
        api.create_backdoor(nets.UnetGenerator(None), torch.zeros(2, 3, 32, 32), None, labels=torch.tensor([0, 1]))


# ---------------------------------------------------------------- the step's host side


def _opt(*argv):
    import config
    from combat_amd.nets import configure_dataset
    opt = config.get_arguments().parse_args(list(argv))
    configure_dataset(opt)
    opt.device = "cpu"
    return opt


def _seed(s):
    import random
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def test_draw_follows_the_reference_order():
    """num_bd over the whole batch (:171), sigma_c only if num_bd > 0 (:176), aug0 (:179), aug1 (:190), aug2 (:199, BEFORE
    the chunks' blur draws), one sigma per chunk (:217), aug3 (:225), aug4 (:236)."""
    from combat_amd import trigger
    from combat_amd.augment import PostTensorTransform
    from combat_amd.step import MultiLabelStep
    opt = _opt("--post_transform_option", "use", "--pc", "0.5")
    st = object.__new__(MultiLabelStep)         # _draw needs only the options and the transform (no device)
    st.opt, st.transforms = opt, PostTensorTransform(opt)
    targets = torch.tensor([0, 0, 0, 0, 3, 5, 7, 0, 1, 2, 0, 4, 9])
    n = 13
    seen_zero = seen_pos = False
    for seed, pc in ((1, 0.5), (2, 0.5), (3, 0.5), (4, 0.0)):
        opt.pc = pc
        _seed(seed)
        r = st._draw(targets, targets.clone())
        _seed(seed)
        tf = PostTensorTransform(opt)
        num_bd = int(np.sum(np.random.rand(n) < pc))
        sigma_c = trigger.sample_sigma((0.1, 1.0)) if num_bd else 0.5
        aug0, aug1, aug2 = tf.sample(n), tf.sample(n), tf.sample(n)
        sig = [trigger.sample_sigma((0.1, 1.0)) for _ in range(7)]        # ps = 2: seven chunks
        aug3, aug4 = tf.sample(n), tf.sample(n)
        assert (r.num_bd, r.sigma_c, list(r.sigma_chunks)) == (num_bd, sigma_c, sig)
        for ours, ref in zip(r.aug, [aug0, aug1, aug2, aug3, aug4]):
            np.testing.assert_array_equal(ours, ref)
        assert len({a.tobytes() for a in r.aug}) == 5 and len(set(sig)) == 7
        seen_zero, seen_pos = seen_zero or num_bd == 0, seen_pos or num_bd > 0
    assert seen_zero and seen_pos


def test_step_table_holds_the_labels_and_the_chunk_kernels():
    from combat_amd.step import LAB_Y, chunk_size, step_table
    for n, classes in ((1, 10), (13, 10), (16, 8), (128, 10)):
        raw, aug, idx, k1, lab = step_table(n, 5, 1 + classes, 8)
        assert aug.shape == (5, n, 4) and idx.shape == (2, n) and k1.shape == (1 + classes, 3) and lab.shape == (8, n)
        assert lab[LAB_Y].view(torch.int32).shape == (2 * n,)
        assert lab.data_ptr() % 8 == 0 or raw.data_ptr() % 8 != 0
        ps = chunk_size(n, classes)
        assert ps == MR.chunk_size(n, classes) and (n + ps - 1) // ps <= classes


def test_step_refuses_a_process_group_and_a_plain_generator(monkeypatch):
    from combat_amd import nets
    from combat_amd.step import MultiLabelStep
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="one rank"):
        MultiLabelStep(None, None, None, None, None, process_group=object())
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 1)
    with pytest.raises(ValueError, match="label-conditioned"):
        MultiLabelStep(None, nets.UnetGenerator(None), None, None, Opt(), process_group=None)


# ---------------------------------------------------------------- the scripts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# reference train_generator_multilabel.py:427-443 (train_victim_multilabel.py: the same file)
GEN_KEYS = {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model", "best_clean_acc",
            "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba", "best_clean_model_bd_asr",
            "epoch_current", "mask", "pattern"}


def test_checkpoint_keys_are_the_references():
    from test_inputaware_cpu import _saved_keys
    assert _saved_keys("train_generator_multilabel.py", "eval") == GEN_KEYS
    import train_generator_multilabel as G
    import train_victim_multilabel as V
    assert V.eval is G.eval and V.main is G.main and V.get_model is G.get_model


def test_script_configuration():
    import train_generator_multilabel as S
    from combat_amd import nets
    opt = _opt("--lr_C", "0.02", "--lr_G", "0.5", "--kernel_size", "5", "--sigma", "23")
    netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model = S.get_model(opt)
    assert opt.kernel_size == 3 and tuple(opt.sigma) == (0.1, 1.0)                 # :53
    assert isinstance(netG, nets.CUnetGeneratorv1) and netG.num_classes == 10
    assert optimizerG.param_groups[0]["lr"] == pytest.approx(0.02 * 0.1)          # :115
    assert optimizerG.param_groups[0]["nesterov"] and optimizerG.param_groups[0]["momentum"] == 0.9
    assert dict(schedulerG.milestones) == dict(schedulerC.milestones)            # :116: the C milestones
    assert schedulerG.gamma == schedulerC.gamma == opt.schedulerC_lambda
    celeba = _opt("--dataset", "celeba")
    assert tuple(S.get_model(celeba)[3].conv0_1.weight.shape) == (64, 72, 3, 3)   # built from opt (the reference: a TypeError)
    for f_model in ("original_dropout", "resnet18", "densenet121"):
        bad = _opt()
        bad.F_model = f_model
        with pytest.raises(Exception, match="F_model"):
            S.get_model(bad)
