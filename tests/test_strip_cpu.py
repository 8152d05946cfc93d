"""CPU-only tests of the STRIP defense: the host restatements of combat_strip_superimpose / combat_strip_entropy
(combat_amd/defenses.py) against the reference's own STRIP class (tests/golden/strip.npz, written by
tests/golden/make_golden_strip.py), the flag table, the result file and verdict lines, the order of the random draws, and
the refusal of a multi-process launch under the defense's own name."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCRIPT_DIR = os.path.join(ROOT, "defenses", "STRIP")


def test_blend_equals_the_reference_bit_for_bit(golden):
    from combat_amd import defenses
    g = golden("strip")
    images, index, blended = g["images"], g["index"], g["blended"]
    nb, s = index.shape
    assert images.dtype == np.uint8 and blended.shape == (nb, s, 3, 32, 32) and blended.dtype == np.float32
    for b in range(nb):
        ours = defenses.strip_blend_reference(images[g["backgrounds"][b]][None], images[index[b]], 3)
        assert ours.dtype == np.float32 and ours.shape == (s, 3, 32, 32)
        assert np.array_equal(ours.view(np.uint32), blended[b].view(np.uint32))
    # the reference's arithmetic reaches three COLUMNS: 0..2 are in [-1, 1] and go below 0, column 3 on stays in [0, 1]
    assert blended[..., :3].min() >= -1.0 and blended[..., :3].max() <= 1.0 and blended[..., :3].min() < 0.0
    assert blended[..., 3:].min() >= 0.0 and blended[..., 3:].max() <= 1.0
    assert blended[..., 3].min() >= 0.0 and blended[..., 2].min() < 0.0
    # every saturated value 0..255 occurs in the fixture: image 0 + image 1 walks every sum 0..510
    sums = images[0].astype(np.int32) + images[1].astype(np.int32)
    assert set(np.unique(sums).tolist()) == set(range(511))
    # the whole-image switch is the usual Normalize(0.5, 0.5)
    full = defenses.strip_blend_reference(images[0], images[1], 32)
    want = (np.minimum(sums, 255).astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    assert np.array_equal(full, want.transpose(2, 0, 1))
    none = defenses.strip_blend_reference(images[0], images[1], 0)
    assert np.array_equal(none, (np.minimum(sums, 255).astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def test_entropy_equals_the_reference(golden):
    """2e-5: a term p * log2(p) is at most 0.531 and carries a few ulp of p times |log2 p + 1.44| in fp32, under about
    1e-6; the division by S cancels the row count, so at most `classes` = 16 such errors add."""
    from combat_amd import defenses
    g = golden("strip")
    nb, s = g["index"].shape
    logits = g["logits"]
    assert logits.shape == (nb, s, 10)
    ours = defenses.strip_entropy_reference(logits.reshape(nb * s, 10), s)
    assert ours.dtype == np.float64 and ours.shape == (nb,)
    err = np.abs(ours - g["entropy"])
    print("entropy: ours %s reference %s max error %.3e" % (ours.tolist(), g["entropy"].tolist(), err.max()))
    assert (err <= 2e-5).all()
    assert np.ptp(g["entropy"]) > 2e-5                                   # the backgrounds are told apart at that bound


def test_entropy_reference_leaves_out_what_nansum_leaves_out():
    from combat_amd import defenses
    x = np.zeros((4, 10), dtype=np.float32)
    assert defenses.strip_entropy_reference(x, 2).tolist() == [5.0, 5.0]
    x[0, 0], x[1, 3], x[2, 5] = -2000.0, 200.0, np.nan                   # p == 0, p == 1, NaN: no contribution
    assert defenses.strip_entropy_reference(x, 2).tolist() == [4.5, 4.75]
    assert defenses.strip_entropy_reference(x, 4).tolist() == [(9 * 0.5 + 9.5 * 0.5) / 2]


def _script_config():
    spec = importlib.util.spec_from_file_location("strip_config_t", os.path.join(SCRIPT_DIR, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_table_matches_the_reference():
    ref = json.load(open(os.path.join(GOLDEN, "strip_flags.json")))
    cfg = _script_config()
    parser = cfg.get_arguments()
    added = {f.lstrip("-") for f, _ in cfg._MISSING + cfg._EXTRA}
    assert added == {"saving_prefix", "num_classes", "bs", "synthetic", "synthetic_size", "seed", "full_normalize"}
    ours = {}
    for a in parser._actions:
        if a.dest == "help" or a.dest in added:
            continue
        d = a.default
        ours[a.dest] = {"default": list(d) if isinstance(d, (list, tuple)) else d, "type": getattr(a.type, "__name__", None),
                        "choices": a.choices, "store_true": a.nargs == 0}
    assert ours == ref
    assert [f for f, _ in cfg._FLAGS] == ["--" + k for k in
                                          ("data_root", "checkpoints", "device", "results", "dataset", "attack_mode",
                                           "temps", "noise_rate", "ratio", "kernel_size", "sigma", "n_sample", "n_test",
                                           "detection_boundary", "num_workers", "test_rounds")]
    opt = parser.parse_args([])
    assert (opt.n_sample, opt.n_test, opt.test_rounds, opt.detection_boundary) == (100, 100, 10, 0.2)
    assert opt.num_classes == 10 and opt.saving_prefix is None and not opt.full_normalize and not opt.synthetic


def test_result_file_and_verdict_lines(tmp_path):
    from combat_amd import defenses
    path = str(tmp_path / "cifar10_result.txt")
    trojan = [np.float32(0.125), 0.5, np.float32(0.1)]
    benign = [1.25, np.float32(0.75)]
    defenses.write_strip_result(path, trojan, benign)
    assert open(path).read() == "0.125 0.5 %r\n1.25 0.75" % float(np.float32(0.1))
    defenses.write_strip_result(path, [], benign)                        # clean mode: the trojan line is empty
    text = open(path).read()
    assert text == "\n1.25 0.75" and len(text.split("\n")) == 2
    low, bad, lines = defenses.strip_verdict(trojan, benign, 0.2)
    assert low == float(np.float32(0.1)) and bad is True
    assert lines == "Min entropy trojan: %r, Detection boundary: 0.2\nA backdoored model\n" % low
    low, bad, lines = defenses.strip_verdict([], benign, 0.2)
    assert low == 0.75 and bad is False
    assert lines == "Min entropy trojan: 0.75, Detection boundary: 0.2\nNot a backdoor model\n"
    assert defenses.strip_verdict([], [0.2], 0.2)[1] is False            # min < boundary, strictly


def test_draws_follow_the_reference_order():
    from combat_amd import defenses
    np.random.seed(123)
    table = defenses.strip_draw_index(5, 7, 10000)
    np.random.seed(123)
    want = [np.random.randint(0, 10000, size=7) for _ in range(5)]
    assert table.shape == (5, 7) and table.dtype == np.int64 and np.array_equal(table, np.stack(want))
    # attack mode: the backdoored backgrounds draw first, the clean ones continue the same stream
    np.random.seed(9)
    first, second = defenses.strip_draw_index(3, 4, 50), defenses.strip_draw_index(3, 4, 50)
    np.random.seed(9)
    assert np.array_equal(np.concatenate([first, second]), defenses.strip_draw_index(6, 4, 50))
    assert first.min() >= 0 and first.max() < 50


def test_world_size_above_one_is_refused_under_the_defense_name(monkeypatch):
    from combat_amd import defenses
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="^STRIP runs on a single GPU.*world size 2"):
        defenses.require_single_process("STRIP")
    with pytest.raises(RuntimeError, match="^fine-pruning runs on a single GPU.*world size 2"):
        defenses.require_single_process()
    monkeypatch.setenv("WORLD_SIZE", "1")
    defenses.require_single_process("STRIP")
