"""Generate tests/golden/neural_cleanse.npz and tests/golden/neural_cleanse_flags.json from the reference's own Neural
Cleanse code.

Run in the build container only (``python tests/golden/make_golden_neural_cleanse.py``), like make_golden_strip.py: it
imports ``/root/reference`` (read-only), which does not exist on the GPU box.  The files it writes are committed; tests
read only those.

The reference's defenses/neural_cleanse/{detecting,neural_cleanse,config}.py are imported unchanged, with stub modules
for what is absent here:
  * ``torchvision``: ``utils.save_image`` does nothing (Recorder.save_result_to_dir calls it on every new best);
  * ``utils.dataloader``: ``get_dataloader`` is never reached -- train_step is handed a list of batches, so the batch
    order is fixed;
  * ``classifier_models``: detecting.py:6 imports ``PreActResNet18`` from the package, whose ``__init__.py`` is empty; the
    package's own class (preact_resnet.py) is set on it under that name.
What is recorded comes from the reference's own ``RegressionModel`` (which loads its classifier from a checkpoint: a
seeded reference ``PreActResNet18`` with perturbed BatchNorm statistics, written to a temporary folder), ``train_step``,
``Recorder`` and ``outlier_detection`` on the CPU.

Parameters of the classifier are never stored: the fixture records the seeds, the uint8 images and what the reference
computed from them.

Sections of the .npz:
  (a) images [16][32][32][3] uint8, images_ragged [10][32][32][3], target_label;
  (b) b_*: 8 consecutive optimisation steps on the 16 images at cost 1e-3, lr 0.1 (gradients of mask_tanh /
      pattern_tanh, the parameters after the step, loss_ce, loss_reg, accuracy), from all-ones parameters;
  (c) c_*: one such step on the 10 ragged images;
  (d) d_*: scripted epochs through train_step with a scripted model (patience 1, early_stop_patience 2,
      early_stop_threshold 1, atk_succ_threshold 50): averages in, cost / flags / counters / reg_best / stop out;
  (e) e_*: outlier_detection's console and file output for three L1-norm lists."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
NC = os.path.join(REF, "defenses", "neural_cleanse")
HERE = os.path.dirname(os.path.abspath(__file__))

# image seed and target label: of 24 (seed, label) pairs tried, the pair whose 8-step bf16-emulated trajectory leaves the
# fewest elements more than lr away from the fp32 one (tests/test_neural_cleanse_cpu.py::test_bf16_emulation_distances)
SEED_NET, SEED_BN, SEED_IMG, SEED_RAGGED = 0, 500, 9310, 9301
TARGET, STEPS, COST, LR = 1, 8, 1e-3, 0.1


def randomize_bn_buffers(net, seed):
    """make_golden.py::randomize_bn_buffers (not imported: that module binds the reference's root `config`)."""
    i = 0
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.05, generator=torch.Generator().manual_seed(seed + i))
                mod.running_var.uniform_(0.6, 1.4, generator=torch.Generator().manual_seed(seed + 1000 + i))
                i += 1
    return net


def install_stubs():
    tv = types.ModuleType("torchvision")
    tvu = types.ModuleType("torchvision.utils")
    tvu.save_image = lambda *a, **k: None
    tv.utils = tvu
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tvu
    sys.modules["torchvision.transforms"] = tv.transforms
    dl = types.ModuleType("utils.dataloader")

    def get_dataloader(*a, **k):
        raise AssertionError("the fixture hands train_step its batches; no loader is built")

    dl.get_dataloader = get_dataloader
    sys.path.insert(0, REF)
    import utils                                                         # the reference's package
    sys.modules["utils.dataloader"] = dl
    utils.dataloader = dl


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    install_stubs()
    import classifier_models
    from classifier_models.preact_resnet import PreActResNet18
    classifier_models.PreActResNet18 = PreActResNet18
    sys.modules.pop("config", None)
    config = _load(os.path.join(NC, "config.py"), "config")              # neural_cleanse.py's `import config`
    detecting = _load(os.path.join(NC, "detecting.py"), "detecting")
    script = _load(os.path.join(NC, "neural_cleanse.py"), "ref_neural_cleanse")
    return config, detecting, script, PreActResNet18


def make_opt(config, tmp, **over):
    opt = config.get_argument().parse_args([])
    opt.device, opt.dataset, opt.saving_prefix = "cpu", "cifar10", "fixture"
    opt.checkpoints, opt.result = os.path.join(tmp, "ck"), os.path.join(tmp, "results")
    opt.input_height = opt.input_width = 32
    opt.input_channel, opt.total_label, opt.target_label = 3, 10, TARGET
    for k, v in over.items():
        setattr(opt, k, v)
    return opt


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def to_inputs(images_u8):
    """The reference's test transform: ToTensor (a true division by 255) and Normalize(0.5, 0.5)."""
    x = torch.from_numpy(images_u8).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    return (x - 0.5) / 0.5


def trajectory(detecting, opt, images_u8, steps, prefix, out):
    """`steps` optimisation steps on one batch.  The reference's train_step drives one model; a twin, stepped here with
    the same calls in the same order (detecting.py:184-196), gives the per-step values train_step only prints -- and must
    land on the same bits."""
    ones_m, ones_p = np.ones((1, 32, 32), np.float32), np.ones((3, 32, 32), np.float32)
    inputs = to_inputs(images_u8)
    labels = torch.zeros(len(images_u8), dtype=torch.int64)
    ref_model = detecting.RegressionModel(opt, ones_m, ones_p)
    ref_optim = torch.optim.Adam(ref_model.parameters(), lr=opt.lr, betas=(0.5, 0.9))
    ref_rec = detecting.Recorder(opt)
    twin = detecting.RegressionModel(opt, ones_m, ones_p)
    optim = torch.optim.Adam(twin.parameters(), lr=opt.lr, betas=(0.5, 0.9))
    ce_fn = torch.nn.CrossEntropyLoss()
    rows = {k: [] for k in ("grad_mask", "grad_pattern", "mask_tanh", "pattern_tanh", "loss_ce", "loss_reg", "acc")}
    for step in range(steps):
        quiet(detecting.train_step, ref_model, ref_optim, [(inputs, labels)], ref_rec, step, opt)
        assert ref_rec.cost == COST
        optim.zero_grad()
        target = torch.ones(len(inputs), dtype=torch.int64) * opt.target_label
        pred = twin(inputs)
        loss_ce = ce_fn(pred, target)
        loss_reg = torch.norm(twin.get_raw_mask(), 1)
        (loss_ce + COST * loss_reg).backward()
        optim.step()
        assert torch.equal(twin.mask_tanh, ref_model.mask_tanh) and torch.equal(twin.pattern_tanh, ref_model.pattern_tanh)
        assert torch.equal(twin.mask_tanh.grad, ref_model.mask_tanh.grad)
        rows["grad_mask"].append(twin.mask_tanh.grad.numpy().copy())
        rows["grad_pattern"].append(twin.pattern_tanh.grad.numpy().copy())
        rows["mask_tanh"].append(twin.mask_tanh.detach().numpy().copy())
        rows["pattern_tanh"].append(twin.pattern_tanh.detach().numpy().copy())
        rows["loss_ce"].append(loss_ce.item())
        rows["loss_reg"].append(loss_reg.item())
        rows["acc"].append((torch.sum(torch.argmax(pred, dim=1) == target) * 100.0 / len(inputs)).item())
    for k, v in rows.items():
        out[prefix + k] = np.asarray(v, dtype=np.float32)
    print(prefix, "loss_ce", rows["loss_ce"], "loss_reg", rows["loss_reg"], "acc", rows["acc"])


class ScriptedModel(torch.nn.Module):
    """What train_step needs of a model, with scripted outcomes: batch b of the current epoch has `hits[b]` rows
    classified as the target and a raw mask whose L1 norm is `reg`."""

    def __init__(self, target):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.target, self.hits, self.reg, self.batch = target, [], 0.0, 0

    def forward(self, x):
        n = x.shape[0]
        logits = torch.zeros(n, 10)
        other = (self.target + 1) % 10
        k = self.hits[self.batch]
        logits[:k, self.target] = 4.0
        logits[k:, other] = 4.0
        self.batch += 1
        return logits * self.w

    def get_raw_mask(self):
        m = torch.zeros(1, 32, 32)
        m[0, 0, 0] = self.reg
        return m * self.w

    def get_raw_pattern(self):
        return torch.full((3, 32, 32), 0.5) * self.w


# (hits per batch of 16 and 10 images, mask L1, force the cost to 0 before the epoch)
SCRIPT_A = [((16, 10), 100.0, False),      # success, first best: cost up
            ((16, 9), 90.0, True),         # cost forced to 0: reset to init_cost (flags cleared), new best, cost up
            ((2, 1), 95.0, False),         # failure: cost down
            ((12, 6), 80.0, False),        # success (68.75 / 60 %), new best: early-stop counter back to 0
            ((16, 10), 85.0, False),       # success, no new best: counter 1
            ((0, 0), 70.0, False),         # failure: counter 2, both flags set: early stop
            ((16, 10), 60.0, False)]       # (never reached)
SCRIPT_B = [((3, 2), 40.0, False),         # failure first: nothing is best yet, the "final version" is kept
            ((16, 10), 50.0, False)]       # success: the first best replaces it


def scripted(detecting, opt, script, prefix, out):
    model = ScriptedModel(opt.target_label)
    optim = torch.optim.SGD(model.parameters(), lr=0.0)
    rec = detecting.Recorder(opt)
    batches = [(torch.zeros(16, 3, 32, 32), torch.zeros(16, dtype=torch.int64)),
               (torch.zeros(10, 3, 32, 32), torch.zeros(10, dtype=torch.int64))]
    ce_fn = torch.nn.CrossEntropyLoss()
    rows = {k: [] for k in ("avg_ce", "avg_reg", "avg_acc", "force_zero", "cost", "cost_up_flag", "cost_down_flag",
                            "cost_up_counter", "cost_down_counter", "cost_set_counter", "early_stop_counter", "reg_best",
                            "early_stop_reg_best", "mask_best_l1", "stop")}
    for epoch, (hits, reg, force_zero) in enumerate(script):
        if force_zero:
            rec.cost = 0.0
        model.hits, model.reg, model.batch = list(hits), reg, 0
        # the averages train_step forms (detecting.py:199-216), formed the same way from the scripted outcomes
        ces, accs = [], []
        with torch.no_grad():
            for (x, _), k in zip(batches, hits):
                pred = model(x)
                target = torch.ones(len(x), dtype=torch.int64) * opt.target_label
                ces.append(ce_fn(pred, target))
                accs.append(torch.sum(torch.argmax(pred, dim=1) == target) * 100.0 / len(x))
        model.batch = 0
        stop = quiet(detecting.train_step, model, optim, batches, rec, epoch, opt)
        rows["avg_ce"].append(torch.mean(torch.stack(ces)).item())
        rows["avg_reg"].append(torch.mean(torch.stack([torch.tensor(reg), torch.tensor(reg)])).item())
        rows["avg_acc"].append(torch.mean(torch.stack(accs)).item())
        rows["force_zero"].append(force_zero)
        rows["cost"].append(rec.cost)
        for k in ("cost_up_flag", "cost_down_flag", "cost_up_counter", "cost_down_counter", "cost_set_counter",
                  "early_stop_counter"):
            rows[k].append(getattr(rec, k))
        rows["reg_best"].append(float(rec.reg_best))
        rows["early_stop_reg_best"].append(float(rec.early_stop_reg_best))
        rows["mask_best_l1"].append(float(rec.mask_best.abs().sum()))
        rows["stop"].append(bool(stop))
        if stop:
            break
    for k, v in rows.items():
        dtype = np.float64 if k in ("cost", "reg_best", "early_stop_reg_best", "mask_best_l1") else \
            np.float32 if k.startswith("avg") else np.int64
        out[prefix + k] = np.asarray(v, dtype=dtype)
    print(prefix, "cost", rows["cost"], "stop", rows["stop"], "acc", rows["avg_acc"])


NORMS = {"outlier": [41.5, 38.25, 44.0, 3.5, 40.75, 39.5, 43.25, 37.0, 42.5, 40.0],
         "none": [41.5, 38.25, 44.0, 36.5, 40.75, 39.5, 43.25, 37.0, 42.5, 40.0],
         "ties": [40.0, 40.0, 40.0, 12.0, 40.0, 41.0, 39.0, 40.0, 12.0, 40.0]}


def outliers(script, opt, out):
    folder = os.path.join(opt.result, "{}_clean".format(opt.saving_prefix), opt.dataset)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, "{}_{}_output.txt".format(opt.dataset, opt.saving_prefix))
    for name, norms in NORMS.items():
        if os.path.exists(path):
            os.remove(path)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            script.outlier_detection(torch.tensor(norms, dtype=torch.float32), {i: i for i in range(len(norms))}, opt)
        out["e_%s_norms" % name] = np.asarray(norms, dtype=np.float32)
        out["e_%s_console" % name] = np.frombuffer(buf.getvalue().encode(), dtype=np.uint8)
        out["e_%s_file" % name] = np.frombuffer(open(path, "rb").read(), dtype=np.uint8)
        print(name, buf.getvalue().strip().split("\n")[2:])


def golden_flags(config):
    """Flag names, defaults and types of the reference parser (defenses/neural_cleanse/config.py:4-56)."""
    flags = {}
    for a in config.get_argument()._actions:
        if a.dest == "help":
            continue
        d = a.default
        flags[a.dest] = {"default": list(d) if isinstance(d, (list, tuple)) else d, "type": getattr(a.type, "__name__", None),
                         "choices": a.choices, "store_true": a.nargs == 0, "flag": a.option_strings[0]}
    with open(os.path.join(HERE, "neural_cleanse_flags.json"), "w") as f:
        json.dump(flags, f, indent=1, sort_keys=True)
    print("wrote neural_cleanse_flags.json (%d flags)" % len(flags))


def main():
    config, detecting, script, PreActResNet18 = import_reference()
    golden_flags(config)
    with tempfile.TemporaryDirectory() as tmp:
        opt = make_opt(config, tmp, lr=LR, init_cost=COST, patience=10 ** 6, early_stop=False)
        torch.manual_seed(SEED_NET)
        net = randomize_bn_buffers(PreActResNet18(), SEED_BN).eval()
        folder = os.path.join(opt.checkpoints, "fixture_clean", "cifar10")
        os.makedirs(folder)
        torch.save({"netC": net.state_dict()}, os.path.join(folder, "cifar10_fixture_clean.pth.tar"))
        images = np.random.default_rng(SEED_IMG).integers(0, 256, (16, 32, 32, 3), dtype=np.uint8)
        ragged = np.random.default_rng(SEED_RAGGED).integers(0, 256, (10, 32, 32, 3), dtype=np.uint8)
        out = {"seeds": np.array([SEED_NET, SEED_BN, SEED_IMG, SEED_RAGGED]), "images": images, "images_ragged": ragged,
               "target_label": np.int64(TARGET), "cost": np.float64(COST), "lr": np.float64(LR),
               "epsilon": np.float64(opt.EPSILON)}
        trajectory(detecting, opt, images, STEPS, "b_", out)
        trajectory(detecting, opt, ragged, 1, "c_", out)
        sopt = make_opt(config, tmp, patience=1, early_stop_patience=2, early_stop_threshold=1.0, atk_succ_threshold=50.0,
                        init_cost=1e-3, cost_multiplier=2)
        out["d_settings"] = np.array([sopt.patience, sopt.early_stop_patience, sopt.early_stop_threshold,
                                      sopt.atk_succ_threshold, sopt.init_cost, sopt.cost_multiplier], dtype=np.float64)
        scripted(detecting, sopt, SCRIPT_A, "d_a_", out)
        scripted(detecting, sopt, SCRIPT_B, "d_b_", out)
        assert out["d_a_stop"].tolist() == [0, 0, 0, 0, 0, 1] and out["d_a_cost_up_flag"][-1] and out["d_a_cost_down_flag"][-1]
        outliers(script, make_opt(config, tmp), out)
    path = os.path.join(HERE, "neural_cleanse.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
