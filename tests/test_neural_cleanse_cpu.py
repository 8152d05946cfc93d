"""CPU-only tests of the Neural Cleanse defense: the recorder, the outlier test, the result file and the flag table against
the reference's own code (tests/golden/neural_cleanse.npz and neural_cleanse_flags.json, written by
tests/golden/make_golden_neural_cleanse.py), the host restatements of combat_nc_blend / combat_nc_update
(combat_amd/defenses.py) against the reference's recorded optimisation steps, the same steps under the bf16 emulation of
the classifier (the two distances the GPU tests scale), and the two entry points' place in the C ABI."""
import importlib.util
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCRIPT_DIR = os.path.join(ROOT, "defenses", "neural_cleanse")

# The two distances between the reference's fp32 steps and the same steps with the classifier's bf16 dataflow
# (tests/bf16_emu.py), measured once by test_bf16_emulation_distances below; tests/test_neural_cleanse_gpu.py allows the
# engine twice as much.  The same constants stand in that file and in DESIGN.md section 10.
E_GRAD = 2.0e-2            # measured 1.975e-2 (the pattern's gradient; the mask's: 5.1e-3)
E_TRAJ = 2.8e-5            # measured 2.705e-5
LR_CAP = 0.02            # share of parameter elements that may sit more than lr away from the reference after 8 steps


def randomize_bn_buffers(net, seed):
    """tests/golden/make_golden.py::randomize_bn_buffers."""
    i = 0
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.05, generator=torch.Generator().manual_seed(seed + i))
                mod.running_var.uniform_(0.6, 1.4, generator=torch.Generator().manual_seed(seed + 1000 + i))
                i += 1
    return net


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def host_trajectory(g, images, steps, forward):
    """The optimisation steps of the fixture from the host restatements: nc_blend_reference, `forward(params, x)` under
    autograd for the classifier's input gradient, nc_gradients_reference, nc_adam_reference.  Per step: gradients,
    parameters after the step, loss_ce, loss_reg (before the step), accuracy."""
    from combat_amd import defenses as D
    from combat_amd import nets
    torch.manual_seed(int(g["seeds"][0]))
    net = randomize_bn_buffers(nets.PreActResNet18(), int(g["seeds"][1])).eval()
    p = {k: v.detach().clone() for k, v in net.state_dict().items()}
    target, cost, lr, eps = int(g["target_label"]), float(g["cost"]), float(g["lr"]), float(g["epsilon"])
    mask, pattern = np.ones((32, 32), np.float32), np.ones((3, 32, 32), np.float32)
    m1, m2 = np.zeros((4, 32, 32), np.float32), np.zeros((4, 32, 32), np.float32)
    rows = []
    for t in range(steps):
        x = torch.from_numpy(D.nc_blend_reference(images, mask, pattern, eps)).requires_grad_(True)
        logits = forward(p, x)
        labels = torch.full((len(images),), target, dtype=torch.int64)
        loss_ce = F.cross_entropy(logits, labels)
        g_img, = torch.autograd.grad(loss_ce, x)
        gm, gp = D.nc_gradients_reference(g_img.numpy(), images, mask, pattern, cost, eps)
        grad = np.concatenate([gm[None], gp]).astype(np.float32)
        loss_reg = float(torch.sum(torch.tanh(torch.from_numpy(mask)) / (2 + eps) + 0.5))     # the raw mask, before the step
        new, m1, m2 = D.nc_adam_reference(np.concatenate([mask[None], pattern]), grad, m1, m2, t, lr)
        mask, pattern = new[0], new[1:]
        acc = float((logits.argmax(1) == labels).sum()) * 100.0 / len(images)
        rows.append(dict(grad_mask=grad[0:1], grad_pattern=grad[1:], mask_tanh=mask[None].copy(), pattern_tanh=pattern.copy(),
                         loss_ce=float(loss_ce.detach()), loss_reg=loss_reg, acc=acc))
    return rows


@pytest.fixture(scope="module")
def fp32_rows(golden):
    from oracle import combat_oracle as O
    g = golden("neural_cleanse")
    return host_trajectory(g, g["images"], 8, lambda p, x: O.preact_resnet18_forward(p, x, False))


@pytest.fixture(scope="module")
def emu_rows(golden):
    import bf16_emu as E
    g = golden("neural_cleanse")
    return host_trajectory(g, g["images"], 8, lambda p, x: E.preact_forward_emu(p, x, False))


def far_share(rows, g, lr):
    """Share of the 4096 parameter elements more than lr away from the reference's after the last step."""
    got = np.concatenate([rows[-1]["mask_tanh"].ravel(), rows[-1]["pattern_tanh"].ravel()])
    want = np.concatenate([g["b_mask_tanh"][-1].ravel(), g["b_pattern_tanh"][-1].ravel()])
    return float((np.abs(got - want) > lr).mean())


def forced_gradients(g, prefix, images, t, forward):
    """The restatements' gradients of step t from the REFERENCE's parameters before that step (all ones before step 0):
    a like-for-like comparison at every step, whatever the trajectories have done before."""
    from combat_amd import defenses as D
    from combat_amd import nets
    torch.manual_seed(int(g["seeds"][0]))
    net = randomize_bn_buffers(nets.PreActResNet18(), int(g["seeds"][1])).eval()
    p = {k: v.detach().clone() for k, v in net.state_dict().items()}
    mask = np.ones((32, 32), np.float32) if t == 0 else g[prefix + "mask_tanh"][t - 1][0]
    pattern = np.ones((3, 32, 32), np.float32) if t == 0 else g[prefix + "pattern_tanh"][t - 1]
    x = torch.from_numpy(D.nc_blend_reference(images, mask, pattern, float(g["epsilon"]))).requires_grad_(True)
    labels = torch.full((len(images),), int(g["target_label"]), dtype=torch.int64)
    g_img, = torch.autograd.grad(F.cross_entropy(forward(p, x), labels), x)
    gm, gp = D.nc_gradients_reference(g_img.numpy(), images, mask, pattern, float(g["cost"]), float(g["epsilon"]))
    return gm[None], gp


def test_host_restatements_reproduce_the_fp32_steps(golden, fp32_rows):
    """Same library, same fp32 convolutions: what differs from the reference's autograd is the tail from the input
    gradient to the parameters, in fp64 here and in fp32 there.  A gradient element is a sum of 3n = 48 products behind
    about ten elementwise fp32 operations: (48 + 10) * 2^-24 = 3.5e-6 of the sum of the terms' magnitudes; the terms of a
    pixel have both signs, so three times that, 1e-5, is allowed on the relative L2 norm of step 0 (and of the ragged batch),
    where the all-ones parameters make the classifier's input the reference's bit for bit.  From step 1 on the gradients
    are taken from the reference's own parameters before the step, and an ulp of difference in the blended input can put an
    activation on the other side of a ReLU: one unit of the deepest layer (512 x 4 x 4 = 8192 units, the fewest) carries
    1 / 8192 of the squared gradient norm on average, sqrt(1 / 8192) = 1.1e-2 of the norm.  Adam from the reference's gradients: an update is within 0.16
    (lr * (1 - beta1) / sqrt(1 - beta2)) and carries a few 1e-7 of itself (fp32 betas, the moments' rounding order), the
    parameter one rounding at magnitude 1 to 2: 1e-6 absolute.  The free-running 8 steps are compared through loss_ce and
    loss_reg at 1e-5 and through the share of elements more than lr away: Adam's first steps move every element by about
    lr whatever the size of its gradient, so the few elements whose gradient is within the 1e-5 of zero may land 0.2
    away and take their neighbourhood's later gradients along; a quarter of the GPU test's cap is allowed."""
    from oracle import combat_oracle as O
    from combat_amd import defenses as D
    g = golden("neural_cleanse")
    fwd = lambda p, x: O.preact_resnet18_forward(p, x, False)
    m1, m2 = np.zeros((4, 32, 32), np.float32), np.zeros((4, 32, 32), np.float32)
    for t in range(8):
        gm, gp = forced_gradients(g, "b_", g["images"], t, fwd)
        eg = max(rel_l2(gm, g["b_grad_mask"][t]), rel_l2(gp, g["b_grad_pattern"][t]))
        before = np.ones((4, 32, 32), np.float32) if t == 0 else np.concatenate([g["b_mask_tanh"][t - 1], g["b_pattern_tanh"][t - 1]])
        ref_grad = np.concatenate([g["b_grad_mask"][t], g["b_grad_pattern"][t]])
        new, m1, m2 = D.nc_adam_reference(before, ref_grad, m1, m2, t, float(g["lr"]))
        ea = np.abs(new - np.concatenate([g["b_mask_tanh"][t], g["b_pattern_tanh"][t]])).max()
        row = fp32_rows[t]
        ece = abs(row["loss_ce"] - g["b_loss_ce"][t]) / g["b_loss_ce"][t]
        ereg = abs(row["loss_reg"] - g["b_loss_reg"][t]) / g["b_loss_reg"][t]
        print("step %d: gradient %.2e adam %.2e | free-running loss_ce %.2e loss_reg %.2e" % (t, eg, ea, ece, ereg))
        assert eg <= (1e-5 if t == 0 else 1.1e-2) and ea <= 1e-6
        assert ece <= 1e-5 and ereg <= 1e-5 and row["acc"] == g["b_acc"][t]
    share = far_share(fp32_rows, g, float(g["lr"]))
    print("elements more than lr away after 8 steps: %.4f" % share)
    assert share <= LR_CAP / 4
    # the first step moves every element by lr against the sign of its gradient
    assert np.abs(np.abs(g["b_mask_tanh"][0] - 1.0) - float(g["lr"])).max() < 1e-4


def test_ragged_batch_step(golden):
    from oracle import combat_oracle as O
    g = golden("neural_cleanse")
    fwd = lambda p, x: O.preact_resnet18_forward(p, x, False)
    gm, gp = forced_gradients(g, "c_", g["images_ragged"], 0, fwd)
    assert rel_l2(gm, g["c_grad_mask"][0]) <= 1e-5 and rel_l2(gp, g["c_grad_pattern"][0]) <= 1e-5
    row = host_trajectory(g, g["images_ragged"], 1, fwd)[0]
    assert abs(row["loss_ce"] - g["c_loss_ce"][0]) <= 1e-5 * g["c_loss_ce"][0]
    assert np.abs(row["mask_tanh"] - g["c_mask_tanh"][0]).max() <= 1e-6


def test_bf16_emulation_distances(golden, emu_rows):
    """E_grad: relative L2 error of the step-1 gradients (the larger of the mask's and the pattern's); E_traj: the largest
    relative error of loss_ce and loss_reg over the 8 steps -- of the reference's steps with the classifier's tensors
    rounded to bf16 where the engine stores them.  Printed, and held against the constants the GPU tests scale."""
    g = golden("neural_cleanse")
    e_mask = rel_l2(emu_rows[0]["grad_mask"], g["b_grad_mask"][0])
    e_pattern = rel_l2(emu_rows[0]["grad_pattern"], g["b_grad_pattern"][0])
    e_grad = max(e_mask, e_pattern)
    e_traj = max(max(abs(r["loss_ce"] - g["b_loss_ce"][t]) / g["b_loss_ce"][t],
                     abs(r["loss_reg"] - g["b_loss_reg"][t]) / g["b_loss_reg"][t]) for t, r in enumerate(emu_rows))
    share = far_share(emu_rows, g, float(g["lr"]))
    print("E_grad %.3e (mask %.3e, pattern %.3e)  E_traj %.3e  share of elements more than lr away %.4f"
          % (e_grad, e_mask, e_pattern, e_traj, share))
    assert e_grad <= E_GRAD and e_traj <= E_TRAJ
    assert share <= 0.75 * LR_CAP     # measured 1.32 %: a quarter of the GPU test's cap is left for what the emulation does not model


# ---------------------------------------------------------------- recorder


def _settings(g):
    patience, es_patience, es_threshold, atk, init_cost, mult = g["d_settings"].tolist()
    return types.SimpleNamespace(patience=int(patience), early_stop_patience=int(es_patience), early_stop=True,
                                 early_stop_threshold=es_threshold, atk_succ_threshold=atk, init_cost=init_cost,
                                 cost_multiplier=int(mult))


@pytest.mark.parametrize("which,epochs", [("d_a_", 6), ("d_b_", 2)])
def test_recorder_follows_the_reference_exactly(golden, which, epochs, capsys):
    from combat_amd.defenses import NeuralCleanseRecorder
    g = golden("neural_cleanse")
    rec = NeuralCleanseRecorder(_settings(g))
    assert len(g[which + "cost"]) == epochs
    for e in range(epochs):
        if g[which + "force_zero"][e]:
            rec.cost = 0.0
        reg = g[which + "avg_reg"][e]
        snap = lambda: (np.full((1, 32, 32), 0, np.float32) + np.float32(reg) * (np.arange(1024).reshape(1, 32, 32) == 0),
                        np.full((3, 32, 32), 0.5, np.float32))
        stop = rec.end_epoch(g[which + "avg_ce"][e], reg, g[which + "avg_acc"][e], snap)
        assert rec.cost == g[which + "cost"][e], e                      # exactly: the same Python float arithmetic
        for k in ("cost_up_flag", "cost_down_flag", "cost_up_counter", "cost_down_counter", "cost_set_counter",
                  "early_stop_counter"):
            assert int(getattr(rec, k)) == g[which + k][e], (e, k)
        assert float(rec.reg_best) == g[which + "reg_best"][e] and float(rec.early_stop_reg_best) == g[which + "early_stop_reg_best"][e]
        assert float(np.abs(rec.mask_best).sum()) == g[which + "mask_best_l1"][e], e
        assert stop == bool(g[which + "stop"][e]) and rec.stopped == stop
    assert rec.epochs == epochs
    printed = capsys.readouterr().out
    if which == "d_a_":
        assert stop and "Early_stop !!!" in printed and "Initialize cost to 0.001000" in printed
        assert "Up cost from 0.001 to 0.002" in printed and "Down cost from 0.002 to" in printed
        assert g[which + "stop"].tolist() == [0, 0, 0, 0, 0, 1]
    else:
        assert not stop and g[which + "reg_best"][0] == np.inf and g[which + "mask_best_l1"].tolist() == [40.0, 50.0]


def test_epoch_averages():
    from combat_amd.defenses import nc_epoch_averages
    stats = np.array([[2.0, 16, 100.0, 16], [1.0, 5, 90.0, 10]], np.float32)
    ce, reg, acc, acc_all = nc_epoch_averages(stats)
    assert (ce, reg, acc) == (np.float32(1.5), np.float32(95.0), np.float32(75.0))   # the mean of 100 % and 50 %
    assert acc_all == 2100.0 / 26


# ---------------------------------------------------------------- outlier test, result file, flags


@pytest.mark.parametrize("name,backdoored,flagged", [("outlier", True, [3]), ("none", False, []), ("ties", True, [3, 8, 6])])
def test_outlier_detection_equals_the_reference(golden, tmp_path, name, backdoored, flagged):
    from combat_amd import defenses as D
    g = golden("neural_cleanse")
    norms = g["e_%s_norms" % name]
    console = bytes(g["e_%s_console" % name]).decode()
    median, mad, index = D.nc_anomaly_index(norms)
    assert "Median: {}, MAD: {}\n".format(float(median), float(mad)) in console
    assert "Anomaly index: {}\n".format(float(index)) in console
    assert median.dtype == np.float32 and median == 40.0               # torch.median: the lower middle value of ten
    assert [label for label, _ in D.nc_flagged_labels(norms)] == flagged
    assert D.nc_flagged_labels(norms, {"a": 3}) == ([("a", norms[3])] if flagged else [])
    bad, text = D.nc_verdict(norms)
    assert bad is backdoored and text == console
    path = str(tmp_path / "cifar10_t_output.txt")
    with open(path, "w+") as f:
        f.write("head\n")
    D.write_nc_result(path, norms)
    assert open(path, "rb").read() == b"head\n" + bytes(g["e_%s_file" % name])   # appended, byte for byte
    with pytest.raises(ValueError):
        D.nc_anomaly_index([])


def _script_config():
    spec = importlib.util.spec_from_file_location("nc_config_t", os.path.join(SCRIPT_DIR, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_table_matches_the_reference():
    ref = json.load(open(os.path.join(GOLDEN, "neural_cleanse_flags.json")))
    cfg = _script_config()
    parser = cfg.get_argument()
    added = {f.lstrip("-") for f, _ in cfg._EXTRA}
    assert added == {"synthetic", "synthetic_size", "seed"}
    ours = {}
    for a in parser._actions:
        if a.dest == "help" or a.dest in added:
            continue
        d = a.default
        ours[a.dest] = {"default": list(d) if isinstance(d, (list, tuple)) else d, "type": getattr(a.type, "__name__", None),
                        "choices": a.choices, "store_true": a.nargs == 0, "flag": a.option_strings[0]}
    assert ours == ref
    opt = parser.parse_args([])
    assert (opt.bs, opt.lr, opt.epoch, opt.patience, opt.early_stop_patience, opt.EPSILON) == (64, 0.1, 50, 5, 25, 1e-7)
    assert opt.grid_rescale == 1 and opt.lnoise == 8 and opt.saving_prefix is None     # the unused WaNet flags parse
    assert parser.parse_args(["--grid-rescale", "0.98", "--clamp", "--S2", "4"]).grid_rescale == 0.98


def test_world_size_above_one_is_refused_under_the_defense_name(monkeypatch):
    from combat_amd import defenses
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="^Neural Cleanse runs on a single GPU.*world size 2"):
        defenses.require_single_process("Neural Cleanse")


def test_blend_reference_arithmetic():
    from combat_amd import defenses as D
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 32, 32, 3), dtype=np.uint8)
    mt, pt = rng.normal(size=(32, 32)).astype(np.float32), rng.normal(size=(3, 32, 32)).astype(np.float32)
    out = D.nc_blend_reference(img, mt, pt, 1e-7)
    assert out.dtype == np.float32 and out.shape == (2, 3, 32, 32)
    m = np.tanh(mt.astype(np.float64)) / (2 + 1e-7) + 0.5
    p = np.tanh(pt.astype(np.float64)) / (2 + 1e-7) + 0.5
    for row in range(3):                                                 # the reference normalises ROWS 0..2, all colours
        p[:, row] = (p[:, row] - D.NC_MEAN[row]) / D.NC_STD[row]
    assert p[:, 3:].min() >= 0 and p[:, 3:].max() <= 1 and p[:, :3].min() < 0
    x = (img.transpose(0, 3, 1, 2) / 255.0 - 0.5) / 0.5
    assert np.abs(out - ((1 - m) * x + m * p)).max() <= 2e-6           # values up to ~2.2: a few fp32 ulp
    # a saturated mask shows the pattern alone, a mask of -inf the image alone
    assert np.abs(D.nc_blend_reference(img, np.full((32, 32), 30.0, np.float32), pt)[0] - p).max() <= 2e-6
    assert np.abs(D.nc_blend_reference(img, np.full((32, 32), -30.0, np.float32), pt) - x).max() <= 2e-6


def test_adam_reference_equals_torch():
    """torch.optim.Adam itself, three steps: the restatement rounds m1 differently (b1 * m1 + (1 - b1) * g against torch's
    lerp) and takes fp32 betas, a few ulp of a value near 1."""
    from combat_amd import defenses as D
    rng = np.random.default_rng(5)
    p0 = rng.normal(size=(4, 8, 8)).astype(np.float32)
    grads = [rng.normal(size=(4, 8, 8)).astype(np.float32) * s for s in (1.0, 1e-3, 10.0)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    optim = torch.optim.Adam([tp], lr=0.1, betas=(0.5, 0.9))
    p, m1, m2 = p0, np.zeros_like(p0), np.zeros_like(p0)
    for t, gr in enumerate(grads):
        tp.grad = torch.from_numpy(gr.copy())
        optim.step()
        p, m1, m2 = D.nc_adam_reference(p, gr, m1, m2, t, 0.1)
        assert np.abs(p - tp.detach().numpy()).max() <= 4 * 2.0 ** -23 * 4   # 4 ulp at magnitude < 4
    assert p.dtype == np.float32


# ---------------------------------------------------------------- C ABI


def test_entry_points_are_exported_with_the_declared_arguments():
    from combat_amd import _lib
    header = open(os.path.join(ROOT, "include", "combat_hip.h")).read()
    for name, count in (("combat_nc_blend", 15), ("combat_nc_update", 29)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == count
        res, args = _lib.SIGNATURES[name]
        assert len(args) == count and getattr(_lib.lib, name).argtypes == args
    assert _lib.lib.combat_abi_version() >= 18
