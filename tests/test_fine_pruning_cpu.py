"""CPU-only tests of the fine-pruning defense: the one-pass sweep (combat_amd/defenses.py, combat_prune_sweep's
arithmetic restated on the host) against the reference's own pruned networks (tests/golden/fine_pruning.npz, written by
tests/golden/make_golden_fine_pruning.py), the flag table, the pruning order, the outfile format, and the refusal of a
multi-process launch."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCRIPT_DIR = os.path.join(ROOT, "defenses", "fine_pruning")


def seeded_linear(seed):
    """linear.weight / linear.bias of the fixture's network: the mirror module under the recorded seed."""
    from combat_amd import nets
    torch.manual_seed(seed)
    net = nets.PreActResNet18()
    return net.linear.weight.detach().numpy(), net.linear.bias.detach().numpy()


def margin_bound(pooled, weight, bias, order, per=1):
    """fp32 summation bound of a logit DIFFERENCE per (level, image): 2 * in * 2^-24 * sum|terms| -- a logit of level k is
    a sum of at most in + 1 terms, each partial sum rounds once (relative 2^-24), and two logits are compared; sum|terms|
    is taken for the class where it is largest."""
    p, w = np.abs(pooled.astype(np.float64)), np.abs(weight.astype(np.float64))
    c = len(order)
    a = np.broadcast_to(np.abs(bias.astype(np.float64)), (p.shape[0], w.shape[0])).copy()
    out = np.empty((c, p.shape[0]))
    for k in range(c - 1, -1, -1):
        for q in range(per):
            f = int(order[k]) * per + q
            a = a + p[:, f:f + 1] * w[None, :, f]
        out[k] = a.max(axis=1)
    return 2 * c * per * 2.0 ** -24 * out


def test_sweep_equals_the_reference_pruned_networks(golden):
    from combat_amd import defenses
    g = golden("fine_pruning")
    weight, bias = seeded_linear(int(g["seeds"][0]))
    pooled, order, pred = g["pooled"], g["seq_sort"], g["pred"]
    c, n = pred.shape
    assert pooled.shape == (n, c) == (32, 512) and sorted(order.tolist()) == list(range(c))
    logits = defenses.sweep_reference(pooled, weight, bias, order, 1)              # fp64 [C][n][classes]
    bound = margin_bound(pooled, weight, bias, order)
    top = np.sort(logits, axis=2)
    excluded = (top[:, :, -1] - top[:, :, -2]) < bound
    assert int(excluded.sum()) == int(g["n_excluded"]) and excluded.mean() <= 0.01, (excluded.sum(), g["n_excluded"])
    wrong = (logits.argmax(axis=2) != pred) & ~excluded
    assert not wrong.any(), "levels %s" % sorted(set(np.nonzero(wrong)[0].tolist()))[:10]
    for k in g["logit_levels"].tolist():
        d = np.abs(logits[k] - g["logits/%d" % k].astype(np.float64)).max(axis=1)
        assert (d <= bound[k]).all(), (k, float(d.max()), float(bound[k].min()))
    # fine-pruning.py:161 from the pooled features: the mean of the window means
    act = pooled.astype(np.float64).mean(axis=0)
    np.testing.assert_allclose(act, g["activation"].astype(np.float64), rtol=1e-5, atol=0)
    assert np.array_equal(defenses.stable_order(g["activation"]), order)


def test_level_zero_is_the_intact_network_and_pruning_changes_predictions(golden):
    """The fixture is not vacuous: the predictions move as channels go, and level 0 holds every channel."""
    from combat_amd import defenses
    g = golden("fine_pruning")
    weight, bias = seeded_linear(int(g["seeds"][0]))
    logits = defenses.sweep_reference(g["pooled"], weight, bias, g["seq_sort"], 1)
    full = g["pooled"].astype(np.float64) @ weight.astype(np.float64).T + bias
    assert np.abs(logits[0] - full).max() < 1e-9
    assert (g["pred"] != g["pred"][0]).any()


def test_sweep_reference_cells_and_forced_order():
    """per > 1: feature c * per + q belongs to channel c (convert(), fine-pruning.py:40-50); the level-k logits keep
    exactly the channels order[k:]."""
    from combat_amd import defenses
    r = np.random.default_rng(3)
    n, c, per, classes = 5, 6, 4, 3
    pooled, weight, bias = r.standard_normal((n, c * per)), r.standard_normal((classes, c * per)), r.standard_normal(classes)
    order = r.permutation(c)
    logits = defenses.sweep_reference(pooled, weight, bias, order, per)
    for k in range(c):
        keep = np.zeros(c * per, dtype=bool)
        for ch in order[k:]:
            keep[ch * per:(ch + 1) * per] = True
        np.testing.assert_allclose(logits[k], pooled[:, keep] @ weight[:, keep].T + bias, rtol=0, atol=1e-12)


def test_order_is_the_stable_ascending_argsort():
    from combat_amd import defenses
    act = np.array([0.5, -1.0, 0.5, 0.25, -1.0, 0.5, 2.0, 0.25])
    assert defenses.stable_order(act).tolist() == [1, 4, 3, 7, 0, 2, 5, 6]
    assert defenses.stable_order(act).dtype == np.int64
    r = np.random.default_rng(0).standard_normal(512)
    assert np.array_equal(defenses.stable_order(r), np.argsort(r, kind="stable"))


def _script_config():
    spec = importlib.util.spec_from_file_location("fine_pruning_config_t", os.path.join(SCRIPT_DIR, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_table_matches_the_reference():
    ref = json.load(open(os.path.join(GOLDEN, "fine_pruning_flags.json")))
    cfg = _script_config()
    ours = {}
    parser = cfg.get_arguments()
    extra = {f.lstrip("-").replace("-", "_") for f, _ in cfg._EXTRA}
    for a in parser._actions:
        if a.dest == "help" or a.dest in extra:
            continue
        d = a.default
        ours[a.dest] = {"default": list(d) if isinstance(d, (list, tuple)) else d, "type": getattr(a.type, "__name__", None),
                        "choices": a.choices, "store_true": a.nargs == 0}
    assert ours == ref
    assert [f for f, _ in cfg._FLAGS][:2] == ["--data_root", "--checkpoints"]
    opt = parser.parse_args(["--synthetic"])
    assert opt.synthetic and opt.bs == 100 and opt.outfile == "./results.txt" and opt.grid_rescale == 1


def test_outfile_format(tmp_path):
    from combat_amd import defenses
    path = str(tmp_path / "results.txt")
    defenses.write_curve(path, np.array([93.5, 10.0, 0.0]), np.array([99.98765, 100.0, 12.34564]))
    assert open(path).read() == "0 93.5000 99.9877\n1 10.0000 100.0000\n2 0.0000 12.3456\n"


def test_world_size_above_one_is_refused(monkeypatch):
    from combat_amd import defenses
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    defenses.require_single_process()
    monkeypatch.setenv("WORLD_SIZE", "1")
    defenses.require_single_process()
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single GPU.*world size 2"):
        defenses.require_single_process()
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 4)
    with pytest.raises(RuntimeError, match="world size 4"):
        defenses.require_single_process()
