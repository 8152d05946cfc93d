"""Host-side pieces of the imperceptible (total-variation) attack (reference train_generator_imperceptible.py,
train_victim_imperceptible.py): the restatement of the step against a fixture recorded from the reference's modules,
the closed-form TV gradient, the step's random draws, and the scripts' configuration, log keys and checkpoint layout."""
import ast
import os
import random

import numpy as np
import pytest
import torch

import config
from combat_amd import trigger
from combat_amd.augment import PostTensorTransform
from combat_amd.nets import configure_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# reference train_generator_imperceptible.py:417-436 (train_generator.py's keys) and train_victim.py:221-229
GEN_KEYS = {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model", "best_clean_acc",
            "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba", "best_clean_model_bd_asr",
            "epoch_current"}
# :293-308
LOG_KEYS = {"Clean", "Bd", "F", "CleanModel Acc", "CleanModel Bd BA", "CleanModel Bd ASR", "L2 Loss", "Grad L2 Loss",
            "TV Loss", "CleanModel Loss"}


def _opt(*argv):
    opt = config.get_arguments().parse_args(list(argv))
    configure_dataset(opt)
    opt.device = "cpu"
    return opt


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


# ------------------------------------------------------------------ the TV term
def test_tv_matches_its_definition_on_a_small_plane():
    import imperceptible_ref as R
    x = torch.tensor([[[[0.0, 1.0, 1.0], [2.0, -1.0, 1.0]]]], dtype=torch.float64)
    # along H: |2-0| + |-1-1| + |1-1| = 4; along W: |1-0| + |1-1| + |-1-2| + |1+1| = 6
    assert R.total_variation(x).tolist() == [10.0]
    assert R.total_variation(torch.cat([x, 2 * x])).tolist() == [10.0, 20.0]


def test_tv_closed_form_gradient_equals_autograd():
    """Exact in fp64, on random planes and on planes with equal neighbours, where sgn(0) = 0 decides (ATen's abs
    backward gives 0 there, and so does the stencil)."""
    import imperceptible_ref as R
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(4, 3, 9, 7, generator=gen, dtype=torch.float64) * 2 - 1
    x[1, :, 2:6, 1:5] = 0.25                   # a flat patch: zero differences inside, one-sided ones on its rim
    x[2] = torch.round(x[2] * 2) / 2           # a quantised image: many ties
    x[3, 0] = -1.0                             # a saturated plane
    assert float(((x[..., 1:, :] - x[..., :-1, :]) == 0).double().mean()) > 0.1
    leaf = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(R.total_variation(leaf).sum(), leaf)
    s = R.tv_sign_stencil(x)
    assert torch.equal(g, s)
    assert torch.equal(s[3, 0], torch.zeros(9, 7, dtype=torch.float64))
    assert float(s[1, :, 3:5, 2:4].abs().max()) == 0.0      # interior of the flat patch
    # the batch mean and the weight scale it as the step's tv_scale = tv_weight / n
    leaf = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(0.3 * R.total_variation(leaf).mean(), leaf)
    torch.testing.assert_close(g, s * (0.3 / 4), rtol=0, atol=1e-15)


# ------------------------------------------------------------------ draws
def test_draw_follows_the_reference_order():
    """num_bd, sigma_c (only if num_bd > 0), aug0, aug1, sigma_g, aug2, aug3, aug4: one sigma per create_inputs_bd
    call (:172-174, :203), the order of train_generator.py."""
    from combat_amd.step import ImperceptibleStep
    opt = _opt("--post_transform_option", "use", "--pc", "0.5")
    st = object.__new__(ImperceptibleStep)         # _draw needs only the options and the transform (no device)
    st.opt, st.transforms = opt, PostTensorTransform(opt)
    targets = torch.tensor([0, 0, 0, 0, 3, 5, 7, 0, 1, 2, 0, 4])
    bd = torch.zeros_like(targets)
    for seed in (1, 2, 3):
        _seed(seed)
        r = st._draw(targets, bd)
        _seed(seed)
        tf = PostTensorTransform(opt)
        num_bd = int(np.sum(np.random.rand(int((targets == bd).sum())) < opt.pc))
        sigma_c = trigger.sample_sigma((0.1, 1.0)) if num_bd else 0.5
        aug0, aug1 = tf.sample(12), tf.sample(12)
        sigma_g = trigger.sample_sigma((0.1, 1.0))
        aug2, aug3, aug4 = tf.sample(12), tf.sample(12), tf.sample(12)
        assert (r.num_bd, r.sigma_c, r.sigma_g) == (num_bd, sigma_c, sigma_g)
        for ours, ref in zip(r.aug, [aug0, aug1, aug2, aug3, aug4]):
            np.testing.assert_array_equal(ours, ref)
        assert len({a.tobytes() for a in r.aug}) == 5


def test_draw_ignores_the_blur_flags():
    """The reference's module-level GaussianBlur (:52) draws from (0.1, 1) whatever --sigma says."""
    from combat_amd.step import ImperceptibleStep
    opt = _opt()
    opt.sigma = (5.0, 6.0)
    st = object.__new__(ImperceptibleStep)
    st.opt, st.transforms = opt, PostTensorTransform(opt)
    _seed(0)
    r = st._draw(torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long))
    assert all(0.1 <= s <= 1.0 for s in (r.sigma_c, r.sigma_g))


# ------------------------------------------------------------------ scripts
def test_tv_weight_flag_is_the_references():
    assert _opt().tv_weight == 0.01
    assert _opt("--tv_weight", "0.5").tv_weight == 0.5


def test_generator_script_configuration():
    import train_generator_imperceptible as S
    opt = _opt("--lr_C", "0.02", "--lr_G", "0.5", "--kernel_size", "5", "--sigma", "23")
    S.fix_blur(opt)
    assert opt.kernel_size == 3 and tuple(opt.sigma) == (0.1, 1.0)
    netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model = S.get_model(opt)
    assert optimizerG.param_groups[0]["lr"] == pytest.approx(0.5)                # :106-108: lr_G, the main script's
    assert dict(schedulerG.milestones) == {m: 1 for m in opt.schedulerG_milestones}
    assert schedulerG.gamma == opt.schedulerG_lambda
    opt.F_model = "original_dropout"        # :19-23: no detector zoo
    with pytest.raises(Exception):
        S.get_model(opt)


def _func(path, func):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == func)


def test_log_keys_are_the_references(monkeypatch, capsys):
    """:293-308: the epoch's scalars are train_generator.py's plus "TV Loss" = the epoch's TV sum over its samples;
    :266-277: the progress line is the main script's, without a TV column."""
    from test_entry_scripts_cpu import METRICS, _run_train
    st, writer, _, lines, _, _ = _run_train("train_generator_imperceptible", monkeypatch, capsys)
    ((tag, items, _),) = writer.scalars
    assert tag == "Clean Accuracy" and {k for k, _ in items} == LOG_KEYS and len(items) == len(LOG_KEYS)
    assert dict(items)["TV Loss"] == METRICS["loss_tv_sum"] / st.samples
    _, _, _, base_lines, _, _ = _run_train("train_generator", monkeypatch, capsys)
    assert [c[0] for c in lines[-1]] == [c[0] for c in base_lines[-1]] and len(lines[-1]) == 6
    assert not any("TV" in label for line in lines for label, _ in line)


def test_checkpoint_keys_and_eval_are_the_main_scripts():
    import train_generator as base
    import train_generator_imperceptible as S
    assert S.eval is base.eval
    fn = _func("train_generator.py", "eval")
    saved = next(n.args[0] for n in ast.walk(fn) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "save"
                 and isinstance(n.args[0], ast.Dict))
    assert {k.value for k in saved.keys} == GEN_KEYS


def test_resume_keeps_the_loaded_clean_model(tmp_path, monkeypatch):
    """:518-534 restore netC / netG / optimisers / schedulers and not clean_model; train_generator.py restores it."""
    from test_entry_scripts_cpu import Run, _resume_checkpoint, _same
    seen = {}
    for script in ("train_generator_imperceptible", "train_generator"):
        (tmp_path / script).mkdir()
        run = Run(script, tmp_path / script, monkeypatch, "--n_iters", "3", "--continue_training", "--allow_missing_F",
                  "--kernel_size", "5")
        sd = _resume_checkpoint(run, 2)
        run.main()
        (call,) = run.train_calls
        assert _same(call["args"][0], sd["netC"]) and _same(call["args"][3], sd["netG"])
        seen[script] = (call["clean_model_is_clean"], _same(call["args"][7], sd["clean_model"]), call["opt"].kernel_size)
    assert seen["train_generator_imperceptible"] == (True, False, 3)       # --load_checkpoint_clean's copy; the fixed blur
    assert seen["train_generator"] == (False, True, 5)


def test_victim_script_delegates_to_train_victim():
    import train_victim as base
    import train_victim_imperceptible as V
    for name in ("get_model", "train", "eval", "main"):
        assert getattr(V, name) is getattr(base, name), name


# ------------------------------------------------------------------ the restatement
def _states():
    from combat_amd import nets
    out = []
    for seed, ctor in ((0, nets.PreActResNet18), (1, nets.PreActResNet18), (2, lambda: nets.UnetGenerator(None))):
        torch.manual_seed(seed)
        out.append({n: v.detach().clone() for n, v in ctor().state_dict().items()})
    return out


def test_restatement_reduces_to_the_oracle_step_at_tv_weight_zero():
    import imperceptible_ref as R
    from oracle import combat_oracle as O
    gen = torch.Generator().manual_seed(4)
    x = (torch.randint(0, 256, (8, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    t = torch.randint(0, 10, (8,), generator=gen)
    t[:3] = 0
    cfg = O.StepConfig()
    oc, ok, og = _states()
    a = O.alternated_step(oc, og, ok, None, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)),
                          x, t, O.StepRandomness(2, 0.4, 0.7), cfg)
    ic, ik, ig = _states()
    b = R.imperceptible_step(ic, ig, ik, None, [None] * len(O.trainable_names(ic)), [None] * len(O.trainable_names(ig)),
                             x, t, O.StepRandomness(2, 0.4, 0.7), cfg, 0.0)
    for k in ("loss_c", "loss_ce", "loss_l2", "clean_model_loss", "loss_g", "gnorm_c", "gnorm_g"):
        assert a[k] == pytest.approx(b[k], rel=1e-6), k
    for n in O.trainable_names(og):
        torch.testing.assert_close(og[n], ig[n], rtol=1e-5, atol=1e-7)
    assert b["loss_tv"] > 0


def _synth(b, seed):
    """tests/golden/make_golden.py::synth_images."""
    u8 = torch.randint(0, 256, (b, 3, 32, 32), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return (u8.float() / 255 - 0.5) / 0.5


def test_restatement_vs_reference_modules(golden):
    """Two steps of tests/imperceptible_ref.py against the trace recorded from the reference's nn.Modules and
    torch.optim.SGD with the reference's loss line (tests/golden/make_golden_imperceptible.py): b = 16, no augmentation,
    recorded draws, tv_weight 1e-4 (the TV term is 81-88 % of the image gradient's norm there, so both it and the rest
    show); the tolerances of test_inputaware_cpu.py::test_restatement_vs_reference_modules."""
    import imperceptible_ref as R
    from oracle import combat_oracle as O
    g = golden("imperceptible_step")
    assert float(g["tv_weight"]) != 0.01 and all(0.2 < s < 0.95 for s in g["trace/tv_grad_share"])
    netc, clean, netg = _states()
    assert [int(s) for s in g["seeds"]] == [0, 1, 2]
    bufs_c, bufs_g = [None] * len(O.trainable_names(netc)), [None] * len(O.trainable_names(netg))
    cfg = O.StepConfig(lr_c=float(g["lr_c"]), lr_g=float(g["lr_g"]))
    for s in range(2):
        x = _synth(16, 4234 + s)
        assert abs(float(x.double().sum()) - float(g["step%d/x_sum" % s])) < 1e-6
        t = torch.from_numpy(g["step%d/targets" % s])
        rnd = O.StepRandomness(int(g["num_bd"][s]), float(g["sigma_c"][s]), float(g["sigma_g"][s]))
        out = R.imperceptible_step(netc, netg, clean, None, bufs_c, bufs_g, x, t, rnd, cfg, float(g["tv_weight"]))
        for k in ("loss_c", "loss_ce", "loss_l2", "loss_tv", "clean_model_loss", "gnorm_g"):   # gnorm_g: the norm of the
            ref = float(g["trace/" + k][s])                                                    # generator's gradient
            assert abs(out[k] - ref) <= 2e-4 * max(1.0, abs(ref)), (s, k, out[k], ref)
        for k in ("clean_correct", "bd_correct", "clean_model_correct", "clean_model_bd_ba", "clean_model_bd_asr"):
            assert out[k] == int(g["trace/" + k][s]), (s, k)
    for prefix, named in (("final/netc", netc), ("final/netg", netg)):
        for k, v in named.items():
            idx, ref = g["%s/%s/idx" % (prefix, k)], g["%s/%s/val" % (prefix, k)]
            np.testing.assert_allclose(v.double().flatten()[idx].numpy(), ref, rtol=5e-3, atol=4e-4, err_msg=k)
