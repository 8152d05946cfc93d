"""Host-side pieces of the input-aware attack (reference train_generator_inputaware.py, train_victim_inputaware.py):
the step's random draws, the scripts' optimiser / scheduler configuration, blur and checkpoint layout, and the
second-batch option of api.create_backdoor."""
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

# reference train_generator_inputaware.py:480-498 and train_victim_inputaware.py:242-251
GEN_KEYS = {"netC", "schedulerC", "optimizerC", "netG", "schedulerG", "optimizerG", "clean_model", "best_clean_acc",
            "best_bd_acc", "best_cross_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
            "best_clean_model_bd_asr", "epoch_current", "mask", "pattern"}
VICTIM_KEYS = {"netC", "schedulerC", "optimizerC", "netG", "best_clean_acc", "best_bd_acc", "best_cross_acc",
               "epoch_current"}


def _opt(*argv):
    opt = config.get_arguments().parse_args(list(argv))
    configure_dataset(opt)
    opt.device = "cpu"
    return opt


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def test_draw_follows_the_reference_order():
    """sigma_c, aug0, aug1, sigma_g, sigma_x, aug2, aug5, aug3, aug4 (:189-252; the cross augmentation before aug3)."""
    from combat_amd.step import InputAwareStep
    opt = _opt("--post_transform_option", "use", "--pc", "0.5")
    st = object.__new__(InputAwareStep)         # _draw needs only the options and the transform (no device)
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
        sigma_g, sigma_x = trigger.sample_sigma((0.1, 1.0)), trigger.sample_sigma((0.1, 1.0))
        aug2, aug5, aug3, aug4 = tf.sample(12), tf.sample(12), tf.sample(12), tf.sample(12)
        assert (r.num_bd, r.sigma_c, r.sigma_g, r.sigma_x) == (num_bd, sigma_c, sigma_g, sigma_x)
        for ours, ref in zip(r.aug, [aug0, aug1, aug2, aug3, aug4, aug5]):
            np.testing.assert_array_equal(ours, ref)
        assert len({a.tobytes() for a in r.aug}) == 6       # six distinct tables: the order is observable


def test_draw_ignores_the_blur_flags():
    """The reference's module-level GaussianBlur (:53) draws from (0.1, 1) whatever --sigma says."""
    from combat_amd.step import InputAwareStep
    opt = _opt()
    opt.sigma = (5.0, 6.0)
    st = object.__new__(InputAwareStep)
    st.opt, st.transforms = opt, PostTensorTransform(opt)
    _seed(0)
    r = st._draw(torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long))
    assert all(0.1 <= s <= 1.0 for s in (r.sigma_c, r.sigma_g, r.sigma_x))


def test_step_table_layout():
    from combat_amd.step import InputAwareStep, step_table
    for n in (1, 7, 16, 128):
        raw, aug, idx, k1, lab = step_table(n, *InputAwareStep.TABLE)
        assert aug.shape == (6, n, 4) and idx.shape == (2, n) and k1.shape == (3, 3) and lab.shape == (9, n)
        spans = sorted((t.data_ptr() - raw.data_ptr(), t.data_ptr() - raw.data_ptr() + t.numel() * t.element_size())
                       for t in (aug, idx, k1, lab))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == raw.numel()


def test_generator_script_configuration():
    import train_generator_inputaware as S
    opt = _opt("--lr_C", "0.02", "--lr_G", "0.5", "--kernel_size", "5", "--sigma", "23")
    S.fix_blur(opt)
    assert opt.kernel_size == 3 and tuple(opt.sigma) == (0.1, 1.0)
    netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model = S.get_model(opt)
    assert optimizerG.param_groups[0]["lr"] == pytest.approx(0.02 * 0.1)          # :120-126
    assert all(p is q for p, q in zip(optimizerG.param_groups[0]["params"], netG.parameters()))
    assert optimizerG.param_groups[0]["nesterov"] and optimizerG.param_groups[0]["momentum"] == 0.9
    assert dict(schedulerG.milestones) == dict(schedulerC.milestones)            # :127: the C milestones
    assert schedulerG.gamma == schedulerC.gamma == opt.schedulerC_lambda


def _saved_keys(path, func):
    """Keys of the dict literal handed to torch.save inside `func` of a script."""
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == func)
    for node in ast.walk(fn):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "save" and isinstance(node.args[0], ast.Dict):
            return {k.value for k in node.args[0].keys}
    raise AssertionError("no torch.save({...}) in %s:%s" % (path, func))


def test_checkpoint_keys_are_the_references():
    assert _saved_keys("train_generator_inputaware.py", "eval") == GEN_KEYS
    assert _saved_keys("train_victim_inputaware.py", "eval") == VICTIM_KEYS


def test_victim_script_fixes_the_blur():
    import train_victim_inputaware as V
    opt = _opt("--kernel_size", "7")
    V.get_model(opt)
    assert opt.kernel_size == 3 and tuple(opt.sigma) == (0.1, 1.0)


def test_rows_like_matches_the_batch_size():
    from train_generator_inputaware import _rows_like
    x = torch.arange(5.0)[:, None]
    assert torch.equal(_rows_like(x, 5), x)
    assert torch.equal(_rows_like(x, 3), x[:3])
    assert torch.equal(_rows_like(x, 7)[:, 0], torch.tensor([0.0, 1, 2, 3, 4, 0, 1]))


def test_create_backdoor_rejects_a_mismatched_second_batch():
    from combat_amd import api
    with pytest.raises(ValueError):
        api.create_backdoor(None, torch.zeros(4, 3, 32, 32), _opt(), noise_from=torch.zeros(3, 3, 32, 32))


def test_restatement_reduces_to_the_oracle_step_at_cross_weight_zero():
    """tests/inputaware_ref.py with cross_weight 0 and inputs2 = inputs is oracle.alternated_step (same draws)."""
    import inputaware_ref as IR
    from oracle import combat_oracle as O
    from combat_amd import nets

    def build():
        torch.manual_seed(0)
        c = nets.PreActResNet18()
        torch.manual_seed(1)
        k = nets.PreActResNet18()
        torch.manual_seed(2)
        g = nets.UnetGenerator(None)
        return [{n: v.detach().clone() for n, v in m.state_dict().items()} for m in (c, k, g)]

    gen = torch.Generator().manual_seed(4)
    x = (torch.randint(0, 256, (8, 3, 32, 32), generator=gen).float() / 255 - 0.5) / 0.5
    t = torch.randint(0, 10, (8,), generator=gen)
    t[:3] = 0
    cfg = O.StepConfig()
    oc, ok, og = build()
    a = O.alternated_step(oc, og, ok, None, [None] * len(O.trainable_names(oc)), [None] * len(O.trainable_names(og)),
                          x, t, O.StepRandomness(2, 0.4, 0.7), cfg)
    ic, ik, ig = build()
    b = IR.inputaware_step(ic, ig, ik, None, [None] * len(O.trainable_names(ic)), [None] * len(O.trainable_names(ig)),
                           x, x, t, IR.Randomness(2, 0.4, 0.7, 0.7), cfg, 0.0)
    for k in ("loss_c", "loss_ce", "loss_l2", "clean_model_loss", "loss_g", "gnorm_c"):
        assert a[k] == pytest.approx(b[k], rel=1e-6), k
    assert a["gnorm_g"] == pytest.approx(b["gnorm_g"], rel=1e-4)
    for n in O.trainable_names(og):
        torch.testing.assert_close(og[n], ig[n], rtol=1e-5, atol=1e-7)
    assert b["cross_correct"] == b["clean_correct"] or b["loss_cross"] > 0


def _synth(b, seed):
    """tests/golden/make_golden.py::synth_images."""
    u8 = torch.randint(0, 256, (b, 3, 32, 32), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return (u8.float() / 255 - 0.5) / 0.5


def test_restatement_vs_reference_modules(golden):
    """Two input-aware steps of tests/inputaware_ref.py against the trace recorded from the reference's nn.Modules
    and torch.optim.SGD (tests/golden/make_golden_inputaware.py): b = 16, no augmentation, recorded draws; the
    tolerances of test_oracle_golden.py::test_alternated_step_trace."""
    import inputaware_ref as IR
    from oracle import combat_oracle as O
    from combat_amd import nets
    g = golden("inputaware_step")

    def state(ctor, seed):
        torch.manual_seed(seed)
        return {k: v.detach().clone() for k, v in ctor().state_dict().items()}

    s0, s1, s2 = [int(s) for s in g["seeds"]]
    netc, clean, netg = state(nets.PreActResNet18, s0), state(nets.PreActResNet18, s1), state(lambda: nets.UnetGenerator(None), s2)
    bufs_c, bufs_g = [None] * len(O.trainable_names(netc)), [None] * len(O.trainable_names(netg))
    cfg = O.StepConfig(lr_c=float(g["lr_c"]), lr_g=float(g["lr_g"]))
    for s in range(2):
        x, x2 = _synth(16, 2234 + s), _synth(16, 3234 + s)
        assert abs(float(x.double().sum()) - float(g["step%d/x_sum" % s])) < 1e-6
        assert abs(float(x2.double().sum()) - float(g["step%d/x2_sum" % s])) < 1e-6
        t = torch.from_numpy(g["step%d/targets" % s])
        rnd = IR.Randomness(int(g["num_bd"][s]), float(g["sigma_c"][s]), float(g["sigma_g"][s]), float(g["sigma_x"][s]))
        out = IR.inputaware_step(netc, netg, clean, None, bufs_c, bufs_g, x, x2, t, rnd, cfg, float(g["cross_weight"]))
        for k in ("loss_c", "loss_ce", "loss_cross", "loss_l2", "clean_model_loss"):
            ref = float(g["trace/" + k][s])
            assert abs(out[k] - ref) <= 2e-4 * max(1.0, abs(ref)), (s, k, out[k], ref)
        for k in ("clean_correct", "bd_correct", "cross_correct", "clean_model_correct", "clean_model_bd_ba",
                  "clean_model_bd_asr"):
            assert out[k] == int(g["trace/" + k][s]), (s, k)
    for prefix, named in (("final/netc", netc), ("final/netg", netg)):
        for k, v in named.items():
            idx, ref = g["%s/%s/idx" % (prefix, k)], g["%s/%s/val" % (prefix, k)]
            np.testing.assert_allclose(v.double().flatten()[idx].numpy(), ref, rtol=5e-3, atol=4e-4, err_msg=k)
