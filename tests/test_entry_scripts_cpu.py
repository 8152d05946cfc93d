"""The training entry scripts on the CPU: what each script's ``train()`` prints, logs and steps, with a stub step class
patched into the script's namespace, and what each script's ``main()`` sets up and hands to ``train`` / ``eval`` on a
fresh start, on --continue_training and on its refusals, with ``train`` / ``eval`` stubbed.  Everything here is a fact
of the scripts' call surface (the reference's positional signatures, the printed columns, the scalar keys, the
checkpoint layout): none of it depends on where the shared code lives."""
import importlib
import os
import re
import sys

import pytest
import torch

import config
from combat_amd import api, dist as cdist
from combat_amd.data import ArrayLoader
from combat_amd.nets import UnetGenerator, configure_dataset, default_classifier

# ------------------------------------------------------------------ train()
METRIC_KEYS = ["clean_correct", "bd_correct", "f_correct", "cross_correct", "clean_model_correct", "clean_model_bd_ba",
               "clean_model_bd_asr", "loss_l2_sum", "loss_grad_l2_sum", "loss_tv_sum", "clean_model_loss_sum"]
METRICS = {k: float(i + 1) for i, k in enumerate(METRIC_KEYS)}      # fixed and distinct
P6 = [("Clean Acc", "clean_correct"), ("Bd Acc", "bd_correct"), ("F Acc", "f_correct"),
      ("Clean Model Acc", "clean_model_correct"), ("Clean Model Bd BA", "clean_model_bd_ba"),
      ("Clean Model Bd ASR", "clean_model_bd_asr")]
P7 = P6[:3] + [("Cross Acc", "cross_correct")] + P6[3:]
ACC = [("Clean", "clean_correct"), ("Bd", "bd_correct"), ("F", "f_correct"), ("CleanModel Acc", "clean_model_correct"),
       ("CleanModel Bd BA", "clean_model_bd_ba"), ("CleanModel Bd ASR", "clean_model_bd_asr")]
L2, GRAD, TV, CM = (("L2 Loss", "loss_l2_sum"), ("Grad L2 Loss", "loss_grad_l2_sum"), ("TV Loss", "loss_tv_sum"),
                    ("CleanModel Loss", "clean_model_loss_sum"))
# script -> (modules whose step classes are stubbed, the names stubbed there, extras after train_dl, progress columns,
#            scalar columns in order, epochs between image grids, grid withheld from a NullWriter)
TRAIN = {
    "train_generator": ("train_generator", ("AlternatedStep", "WanetStep"), "", P6, ACC + [L2, GRAD, CM], 20, True),
    "train_generator_wanet": ("train_generator", ("AlternatedStep", "WanetStep"), "i", P6, ACC + [L2, GRAD, CM], 20, True),
    "train_generator_imperceptible": ("train_generator_imperceptible", ("ImperceptibleStep",), "", P6,
                                      ACC + [L2, GRAD, TV, CM], 1, True),
    "train_generator_inputaware": ("train_generator_inputaware", ("InputAwareStep",), "lmp", P7,
                                   ACC[:2] + [("Cross", "cross_correct")] + ACC[2:] + [L2, CM], 1, True),
    "train_generator_multilabel": ("train_generator_multilabel", ("MultiLabelStep",), "mp", P6, ACC + [L2, CM], 1, False),
}


class RecordingWriter:
    def __init__(self):
        self.scalars, self.images = [], []

    def add_scalars(self, tag, values, step):
        self.scalars.append((tag, list(values.items()), step))

    def add_image(self, tag, img, global_step=None):
        self.images.append((tag, tuple(img.shape), global_step))


class RecordingNullWriter(cdist.NullWriter):
    def __init__(self):
        self.scalars, self.images = [], []

    def add_image(self, tag, img, global_step=None):
        self.images.append((tag, global_step))


class Scheduler:
    def __init__(self):
        self.steps = 0

    def step(self):
        self.steps += 1


class Optimizer:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}, {"lr": -1.0}]


def _stub_step_class(made):
    class StubStep:
        def __init__(self, *a, **k):
            self.samples, self.runs, self.reads, self.resets = 0, [], 0, 0
            made.append(self)

        def reset_metrics(self):
            self.samples = 0
            self.resets += 1

        def run(self, inputs, targets, *rest, **kw):
            self.samples += len(inputs)
            self.inputs, self.bd = inputs, inputs * 0.5
            self.runs.append((inputs, targets, rest, kw))

        def read_metrics(self, reset=False):
            self.reads += 1
            return dict(METRICS, samples=self.samples)
    return StubStep


def _batches(n, rows=(4, 4, 4), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(r, 3, 32, 32, generator=g), torch.zeros(r, dtype=torch.long)) for r in rows[:n]]


def _progress_columns(out):
    """[(label, value), ...] of every progress line in the captured stdout."""
    lines = []
    for chunk in re.split(r"[\r\n]", out):
        if "] | " in chunk:
            lines.append([(a.strip(), float(b)) for a, b in re.findall(r"\| ([^|:]+): (-?\d+\.\d+)", chunk.split("]", 1)[1])])
    return lines


def _run_train(script, monkeypatch, capsys, epoch=0, flags=(), writer=None, n_batches=3):
    mod_name, names, extras, *_ = TRAIN[script]
    mod = importlib.import_module(script)
    made = []
    stub = _stub_step_class(made)
    for name in names:
        monkeypatch.setattr(importlib.import_module(mod_name), name, stub)
    opt = config.get_arguments().parse_args(["--device", "cpu", *flags])
    configure_dataset(opt)
    dl, dl2 = _batches(n_batches), _batches(n_batches, rows=(5, 3, 4), seed=1)
    extra = [{"i": "identity grid", "l": dl2, "m": None, "p": None}[c] for c in extras]
    writer = writer or RecordingWriter()
    sched = Scheduler(), Scheduler()
    net = lambda: torch.nn.Linear(1, 1)
    capsys.readouterr()
    mod.train(net(), Optimizer(0.25), sched[0], net(), Optimizer(0.125), sched[1], None, net(), dl, *extra, writer, epoch,
              opt)
    (st,) = made
    return st, writer, sched, _progress_columns(capsys.readouterr().out), dl, dl2


@pytest.mark.parametrize("script", sorted(TRAIN))
def test_train_prints_logs_and_steps(script, monkeypatch, capsys):
    _, _, extras, progress, scalars, _, _ = TRAIN[script]
    st, writer, sched, lines, dl, dl2 = _run_train(script, monkeypatch, capsys, flags=("--log_interval", "2"))
    assert st.resets == 1 and len(st.runs) == 3 and st.samples == 12
    assert st.reads == 2 and len(lines) == 2        # batches 0 and 2 of three at --log_interval 2
    assert [c[0] for c in lines[-1]] == [label for label, _ in progress]
    for (label, value), (_, key) in zip(lines[-1], progress):
        assert value == pytest.approx(METRICS[key] * 100.0 / 12, abs=1e-4), label
    assert [c[1] for c in lines[0]] == [pytest.approx(METRICS[key] * 100.0 / 4, abs=1e-4) for _, key in progress]
    ((tag, items, step),) = writer.scalars
    assert (tag, step) == ("Clean Accuracy", 0)
    assert [k for k, _ in items] == [name for name, _ in scalars]
    for (name, value), (_, key) in zip(items, scalars):
        want = METRICS[key] / 12 if key.endswith("_sum") else METRICS[key] * 100.0 / 12
        assert value == pytest.approx(want, rel=1e-12), name
    for i, (inputs, targets, rest, kw) in enumerate(st.runs):
        assert torch.equal(inputs, dl[i][0]) and targets is dl[i][1]
        assert kw == {"lr_c": 0.25, "lr_g": 0.125}          # the optimisers' first param group
        assert len(rest) == (1 if "l" in extras else 0)
    assert (sched[0].steps, sched[1].steps) == (1, 1)


def test_inputaware_train_cuts_the_second_batch_to_the_first(monkeypatch, capsys):
    from train_generator_inputaware import _rows_like
    st, _, _, _, dl, dl2 = _run_train("train_generator_inputaware", monkeypatch, capsys)
    for i, (inputs, _, rest, _) in enumerate(st.runs):
        assert rest[0].shape == inputs.shape and torch.equal(rest[0], _rows_like(dl2[i][0], 4))
    assert torch.equal(st.runs[0][2][0], dl2[0][0][:4])                                     # five rows: cut
    assert torch.equal(st.runs[1][2][0], torch.cat([dl2[1][0], dl2[1][0][:1]]))            # three rows: wrapped


@pytest.mark.parametrize("script", sorted(TRAIN))
def test_train_image_grid_cadence(script, monkeypatch, capsys):
    every, guarded = TRAIN[script][5:]
    for epoch in (0, 1, 20):
        _, writer, _, _, _, _ = _run_train(script, monkeypatch, capsys, epoch=epoch)
        want = [("Images", epoch)] if epoch % every == 0 else []
        assert [(tag, step) for tag, _, step in writer.images] == want, epoch
        assert all(len(shape) == 3 and shape[0] == 3 for _, shape, _ in writer.images)
        assert [s[2] for s in writer.scalars] == [epoch]
        if guarded:
            _, null, _, _, _, _ = _run_train(script, monkeypatch, capsys, epoch=epoch, writer=RecordingNullWriter())
            assert null.images == []


@pytest.mark.parametrize("script", sorted(TRAIN))
def test_train_read_cadence_and_max_steps(script, monkeypatch, capsys):
    st, *_ = _run_train(script, monkeypatch, capsys, flags=("--log_interval", "1"))
    assert st.reads == 3
    st, *_ = _run_train(script, monkeypatch, capsys)         # the default interval: the first batch and the last
    assert st.reads == 2
    st, writer, sched, lines, _, _ = _run_train(script, monkeypatch, capsys, flags=("--max_steps", "2", "--log_interval", "5"))
    assert len(st.runs) == 2 and st.reads == 2 and len(lines) == 2
    ((_, items, _),) = writer.scalars
    assert items[0] == ("Clean", pytest.approx(METRICS["clean_correct"] * 100.0 / 8))
    assert (sched[0].steps, sched[1].steps) == (1, 1)


def test_multilabel_train_refuses_an_empty_loader(monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        _run_train("train_generator_multilabel", monkeypatch, capsys, n_batches=0)
    assert "train_generator_multilabel.py" in str(e.value) and "no batch" in str(e.value)


# ------------------------------------------------------------------ main()
GEN6 = ("best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
        "best_clean_model_bd_asr")
GEN7 = GEN6[:2] + ("best_cross_acc",) + GEN6[2:]
# script -> (networks / optimisers / schedulers ahead of the loaders, extras after train_dl, extras after test_dl, best
#            keys, checkpoint mode for --saving_prefix run, module whose train / eval are stubbed)
#   l: a loader, m: mask (H, W), p: pattern (C, H, W)
MAIN = {
    "train_generator": (8, "", "", GEN6, "run_clean", None),
    "train_generator_imperceptible": (8, "", "", GEN6, "run_clean", None),
    "train_generator_inputaware": (8, "lmp", "lmp", GEN7, "run_clean", None),
    "train_generator_multilabel": (8, "mp", "mp", GEN6, "run_clean", None),
    "train_victim": (4, "", "", ("best_clean_acc", "best_bd_acc"), "run", None),
    "train_victim_inputaware": (4, "", "l", ("best_clean_acc", "best_bd_acc", "best_cross_acc"), "run_clean", "train_victim"),
    "train_clean_classifier": (3, "", "", ("best_clean_acc",), "run", None),
}
GENERATORS = [s for s in sorted(MAIN) if s.startswith("train_generator")]


def _opt(*flags):
    opt = config.get_arguments().parse_args(["--device", "cpu", *flags])
    configure_dataset(opt)
    return opt


def _seeded(ctor, seed):
    torch.manual_seed(seed)
    return ctor()


def _same(module, state):
    own = module.state_dict()
    return own.keys() == state.keys() and all(torch.equal(own[k], state[k]) for k in own)


class Run:
    """One call of a script's main() in a scratch directory with train / eval replaced by recorders."""

    def __init__(self, script, tmp_path, monkeypatch, *flags, clean=True, seed="3"):
        self.script, self.spec = script, MAIN[script]
        self.mod = importlib.import_module(script)
        self.train_calls, self.eval_calls, self.momentum = [], [], []
        monkeypatch.chdir(tmp_path)
        n_models, _, _, keys, mode, train_mod = self.spec
        self.folder = os.path.join("ck", mode, "cifar10")
        self.path = os.path.join(self.folder, "cifar10_%s.pth.tar" % mode)
        opt = _opt()
        self.clean_state = _seeded(lambda: default_classifier(opt), 100).state_dict()
        if clean:
            os.makedirs("ck/clean/cifar10", exist_ok=True)
            torch.save({"netC": self.clean_state}, "ck/clean/cifar10/cifar10_clean.pth.tar")
        os.makedirs("ck/gen/cifar10", exist_ok=True)
        torch.save({"netG": _seeded(lambda: UnetGenerator(opt), 101).state_dict()}, "ck/gen/cifar10/cifar10_gen.pth.tar")
        monkeypatch.setattr(importlib.import_module(train_mod) if train_mod else self.mod, "train", self._train)
        monkeypatch.setattr(self.mod, "eval", self._eval)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
        monkeypatch.setattr(api, "load_momentum_from_optimizer", lambda o, m: self.momentum.append((o, m)))
        monkeypatch.setattr(sys, "argv", [
            script + ".py", "--device", "cpu", "--synthetic", "--synthetic_size", "64", "--bs", "16", "--checkpoints", "ck",
            "--saving_prefix", "run", "--load_checkpoint_clean", "clean", "--load_checkpoint", "gen", *flags]
            + (["--seed", seed] if seed else []))

    def _train(self, *a):
        n = self.spec[0]
        loaders = [x for x in a[n:-3] if isinstance(x, ArrayLoader)]
        self.train_calls.append(dict(args=a, epoch=a[-2], opt=a[-1], loader_epochs=[dl.epoch for dl in loaders],
                                     clean_model_is_clean=len(a) > 7 and n == 8 and _same(a[7], self.clean_state)))

    def _eval(self, *a):
        n, _, extras, keys, _, _ = self.spec
        lo = n + 1 + len(extras)
        best = a[lo:lo + len(keys)]
        self.eval_calls.append(dict(args=a, best=best, epoch=a[-2]))
        out = tuple(100.0 * (a[-2] + 1) + i for i in range(len(keys)))
        return out if len(keys) > 1 else out[0]

    def main(self):
        self.mod.main()
        return self


def _check_extras(args, start, kinds, opt):
    for x, kind in zip(args[start:start + len(kinds)], kinds):
        if kind == "l":
            assert isinstance(x, ArrayLoader)
        elif kind == "m":
            assert tuple(x.shape) == (opt.input_height, opt.input_width)
        else:
            assert tuple(x.shape) == (opt.input_channel, opt.input_height, opt.input_width)


@pytest.mark.parametrize("script", sorted(MAIN))
def test_main_fresh_start(script, tmp_path, monkeypatch, capsys):
    n, train_extra, eval_extra, keys, mode, _ = MAIN[script]
    flags = ["--n_iters", "2"] + (["--allow_missing_F"] if n == 8 else [])
    run = Run(script, tmp_path, monkeypatch, *flags)
    os.makedirs(run.folder)
    stale = os.path.join(run.folder, "stale.txt")
    open(stale, "w").close()
    run.main()
    out = capsys.readouterr().out
    assert not os.path.exists(stale)
    assert [c["epoch"] for c in run.train_calls] == [0, 1] == [c["epoch"] for c in run.eval_calls]
    assert out.count("Epoch ") == 2 and "Epoch 1:" in out and "Epoch 2:" in out
    assert len(re.findall(r" train \d+\.\d\d s, eval \+ checkpoint \d+\.\d\d s", out)) == 2
    if n == 8:
        assert "Train from scratch!!!" in out and "Loading original at " in out and "Done" in out
    t, e = run.train_calls[0], run.eval_calls[0]
    opt = t["opt"]
    # the reference's positional signatures
    assert len(t["args"]) == n + 1 + len(train_extra) + 3
    assert len(e["args"]) == n + 1 + len(eval_extra) + len(keys) + 3
    assert isinstance(t["args"][n], ArrayLoader) and isinstance(e["args"][n], ArrayLoader)
    assert t["args"][n].shuffle and not e["args"][n].shuffle
    _check_extras(t["args"], n + 1, train_extra, opt)
    _check_extras(e["args"], n + 1, eval_extra, opt)
    assert t["args"][:n] == e["args"][:n] and all(t["args"][i] is run.train_calls[1]["args"][i] for i in range(n))
    assert hasattr(t["args"][-3], "add_scalars") and not isinstance(t["args"][-3], cdist.NullWriter)
    if n == 8:
        assert t["clean_model_is_clean"]
    loaders = [x for x in t["args"][n:] + e["args"][n:] if isinstance(x, ArrayLoader)]
    assert len({id(x) for x in loaders}) == len(loaders) == 2 + train_extra.count("l") + eval_extra.count("l")
    if "l" in eval_extra:       # the second test loader is shuffled; with --seed the second loaders' orders are kept apart
        assert e["args"][n + 1].shuffle
    if "l" in train_extra:
        assert t["args"][n + 1].base_seed == t["args"][n].base_seed + 104729
        assert e["args"][n + 1].base_seed == e["args"][n].base_seed + 104729
    if "m" in train_extra:
        mask = t["args"][n + 1 + train_extra.index("m")]
        want = torch.zeros(opt.input_height, opt.input_width)
        want[2:6, 2:6] = 0.1
        assert torch.equal(mask, want) and mask is e["args"][n + 1 + eval_extra.index("m")]
    # the checkpoint layout
    assert os.path.normpath(opt.ckpt_folder) == os.path.normpath(run.folder)
    assert os.path.normpath(opt.ckpt_path) == os.path.normpath(run.path)
    assert os.path.normpath(opt.log_dir) == os.path.normpath(os.path.join(run.folder, "log_dir"))
    assert os.path.isdir(opt.log_dir)
    # bests start at zero and travel from one eval to the next
    assert list(e["best"]) == [0.0] * len(keys)
    assert list(run.eval_calls[1]["best"]) == [100.0 + i for i in range(len(keys))]
    assert t["loader_epochs"] == [0] * (1 + train_extra.count("l"))


def _resume_checkpoint(run, epoch):
    """A checkpoint as the script's eval() writes it, from differently seeded networks."""
    n, train_extra, _, keys, _, _ = run.spec
    opt = _opt("--saving_prefix", "run")
    torch.manual_seed(200)
    models = run.mod.get_model(opt)
    sd = {"netC": models[0].state_dict(), "optimizerC": models[1].state_dict(), "schedulerC": models[2].state_dict(),
          "epoch_current": epoch}
    if n >= 4:
        sd["netG"] = models[3].state_dict()
    if n == 8:
        sd.update(optimizerG=models[4].state_dict(), schedulerG=models[5].state_dict(), clean_model=models[7].state_dict())
    if "m" in train_extra:
        sd.update(mask=torch.full((opt.input_height, opt.input_width), 0.25),
                  pattern=torch.full((opt.input_channel, opt.input_height, opt.input_width), 0.75))
    sd.update({k: 11.0 + i for i, k in enumerate(keys)})
    os.makedirs(run.folder, exist_ok=True)
    torch.save(sd, run.path)
    return sd


@pytest.mark.parametrize("script", sorted(MAIN))
def test_main_resume(script, tmp_path, monkeypatch, capsys):
    n, train_extra, eval_extra, keys, _, _ = MAIN[script]
    flags = ["--n_iters", "3", "--continue_training"] + (["--allow_missing_F"] if n == 8 else [])
    run = Run(script, tmp_path, monkeypatch, *flags)
    sd = _resume_checkpoint(run, 2)
    run.main()
    out = capsys.readouterr().out
    assert os.path.exists(run.path)                                   # no wipe
    assert [c["epoch"] for c in run.train_calls] == [2] == [c["epoch"] for c in run.eval_calls]
    assert "Epoch 3:" in out and out.count("Epoch ") == 1
    t, e = run.train_calls[0], run.eval_calls[0]
    assert t["loader_epochs"] == [2] * (1 + train_extra.count("l"))   # every training loader
    assert all(x.epoch == 0 for x in e["args"][n:] if isinstance(x, ArrayLoader))
    assert list(e["best"]) == [11.0 + i for i in range(len(keys))]
    assert _same(t["args"][0], sd["netC"])
    assert t["args"][2].state_dict() == sd["schedulerC"]
    assert [m for _, m in run.momentum] == [t["args"][0]] + ([t["args"][3]] if n == 8 else [])
    assert [o for o, _ in run.momentum] == [t["args"][1]] + ([t["args"][4]] if n == 8 else [])
    if n == 8:
        assert "Continue training!!" in out
        assert _same(t["args"][3], sd["netG"]) and t["args"][5].state_dict() == sd["schedulerG"]
        assert not _same(t["args"][7], sd["clean_model"]) or not t["clean_model_is_clean"]    # the two copies differ
        if script == "train_generator_imperceptible":
            assert t["clean_model_is_clean"]          # --load_checkpoint_clean's copy stays
        else:
            assert _same(t["args"][7], sd["clean_model"])
    if "m" in train_extra:
        mask, pattern = (t["args"][n + 1 + train_extra.index(c)] for c in "mp")
        assert torch.equal(mask, sd["mask"]) and torch.equal(pattern, sd["pattern"])
        assert pattern is e["args"][n + 1 + eval_extra.index("p")]


@pytest.mark.parametrize("script", ["train_victim", "train_victim_inputaware", "train_clean_classifier"])
def test_classifier_scripts_start_fresh_without_a_checkpoint(script, tmp_path, monkeypatch, capsys):
    """--continue_training with no file: a silent fresh start (the generator scripts exit instead)."""
    run = Run(script, tmp_path, monkeypatch, "--n_iters", "1", "--continue_training")
    os.makedirs(run.folder)
    stale = os.path.join(run.folder, "stale.txt")
    open(stale, "w").close()
    run.main()
    assert not os.path.exists(stale)
    assert [c["epoch"] for c in run.train_calls] == [0] and list(run.eval_calls[0]["best"]) == [0.0] * len(run.spec[3])
    assert "doesnt exist" not in capsys.readouterr().out


@pytest.mark.parametrize("script", GENERATORS)
def test_generator_scripts_three_exits(script, tmp_path, monkeypatch, capsys):
    def refused(run):
        with pytest.raises(SystemExit) as e:
            run.main()
        assert e.value.code is None and run.train_calls == []        # exit(), not SystemExit(message)
        return capsys.readouterr().out

    (tmp_path / "a").mkdir()
    out = refused(Run(script, tmp_path / "a", monkeypatch, "--allow_missing_F", clean=False))
    assert "Error: %s not found\n" % os.path.join("ck", "clean", "cifar10", "cifar10_clean.pth.tar") in out
    (tmp_path / "b").mkdir()
    out = refused(Run(script, tmp_path / "b", monkeypatch))
    detector = os.path.join("./defenses/frequency_based/checkpoints", "cifar10", "original", "cifar10_original_detector.pth.tar")
    assert "Loading original at %s\n" % detector in out
    assert "Error: %s not found (pass --allow_missing_F to run with an untrained detector)\n" % detector in out
    assert "Done" not in out
    (tmp_path / "c").mkdir()
    out = refused(Run(script, tmp_path / "c", monkeypatch, "--allow_missing_F", "--continue_training"))
    assert "Pretrained model doesnt exist\n" in out and "Continue training" not in out


@pytest.mark.parametrize("script", ["train_victim", "train_victim_inputaware"])
def test_victim_scripts_exit_without_the_generator(script, tmp_path, monkeypatch, capsys):
    run = Run(script, tmp_path, monkeypatch)
    os.remove("ck/gen/cifar10/cifar10_gen.pth.tar")
    with pytest.raises(SystemExit) as e:
        run.main()
    assert e.value.code is None and run.train_calls == []
    assert "Error: %s not found\n" % os.path.join("ck", "gen", "cifar10", "cifar10_gen.pth.tar") in capsys.readouterr().out


def test_multilabel_main_refuses_more_than_one_rank(tmp_path, monkeypatch):
    run = Run("train_generator_multilabel", tmp_path, monkeypatch, "--allow_missing_F")
    monkeypatch.setattr(cdist, "init", lambda *a, **k: (0, 0, 2))      # no WORLD_SIZE: that would start a rendezvous
    with pytest.raises(SystemExit) as e:
        run.main()
    assert str(e.value) == ("train_generator_multilabel.py runs as one process: the multi-label step has no "
                            "data-parallel path")
    assert run.train_calls == []


def test_seeding_policies(tmp_path, monkeypatch):
    """Generator family: numpy and random offset by the rank; victim family: random NOT offset (one poisoned index set);
    train_clean_classifier.py: torch only.  The process is told it is rank 1 of 2 without a process group: nothing here
    communicates before the (empty) epoch loop once the replicas' broadcast is patched out."""
    import random
    import numpy as np
    seen = {}
    monkeypatch.setattr(cdist, "init", lambda *a, **k: (1, 0, 2))
    monkeypatch.setattr(cdist, "broadcast_module", lambda *a, **k: None)
    for script in ("train_generator", "train_victim", "train_clean_classifier"):
        (tmp_path / script).mkdir()
        run = Run(script, tmp_path / script, monkeypatch, "--allow_missing_F", "--n_iters", "0", seed="5")
        calls = []
        with monkeypatch.context() as m:
            m.setattr(torch, "manual_seed", lambda s: calls.append(("torch", s)))
            m.setattr(np.random, "seed", lambda s: calls.append(("numpy", s)))
            m.setattr(random, "seed", lambda s: calls.append(("random", s)))
            run.main()
        seen[script] = calls
    assert seen["train_generator"] == [("torch", 5), ("numpy", 6), ("random", 6)]
    assert seen["train_victim"] == [("torch", 5), ("numpy", 6), ("random", 5)]
    assert seen["train_clean_classifier"] == [("torch", 5)]
