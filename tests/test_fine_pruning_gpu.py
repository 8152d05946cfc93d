"""Fine-pruning defense on the MI355X: combat_prune_sweep / combat_feature_colsum against host restatements (exactly
on grid data, after the fp32-margin exclusion on Gaussian data), the sweep against the slow path (pruned columns of
`linear` zeroed, the module's own eval forward) on the HIP engine, the activation order against the reference's
(tests/golden/fine_pruning.npz), and defenses/fine_pruning/fine-pruning.py end to end on synthetic data."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emu as E  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def m():
    from combat_amd import _lib, api, defenses, nets, ops
    return dict(lib=_lib.lib, api=api, defenses=defenses, nets=nets, ops=ops)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def levels_fp64(pooled, weight, bias, order, per):
    """Logits [C][n][classes] of every pruning level in fp64, added from the channel pruned last to the one pruned
    first (combat_prune_sweep's order), and sum|terms| [C][n] for the class where it is largest."""
    p, w = pooled.astype(np.float64), weight.astype(np.float64)
    c = len(order)
    s = np.broadcast_to(bias.astype(np.float64), (p.shape[0], w.shape[0])).copy()
    a = np.abs(s)
    logits, mass = np.empty((c,) + s.shape), np.empty((c, p.shape[0]))
    for k in range(c - 1, -1, -1):
        for q in range(per):
            f = int(order[k]) * per + q
            t = p[:, f:f + 1] * w[None, :, f]
            s, a = s + t, a + np.abs(t)
        logits[k], mass[k] = s, a.max(axis=1)
    return logits, mass


def fp32_margin(mass, fin):
    """Two fp32 logits of at most fin + 1 terms each, every partial sum rounded once: their difference is off the exact
    one by less than 2 * fin * 2^-24 * sum|terms|."""
    return 2 * fin * 2.0 ** -24 * mass


def margins(logits):
    top = np.sort(logits, axis=-1)
    return top[..., -1] - top[..., -2] if logits.shape[-1] > 1 else np.full(logits.shape[:-1], np.inf)


def sweep(m, pooled, weight, bias, order, per, targets, targets2=None, correct=None, correct2=None):
    c = len(order)
    correct = torch.zeros(c, dtype=torch.int32, device="cuda") if correct is None else correct
    if targets2 is not None and correct2 is None:
        correct2 = torch.zeros(c, dtype=torch.int32, device="cuda")
    m["ops"].prune_sweep(dev(pooled, torch.float32), dev(weight, torch.float32), dev(bias, torch.float32),
                         dev(order, torch.int32), per, dev(targets, torch.int64), correct,
                         None if targets2 is None else dev(targets2, torch.int64), correct2)
    return correct, correct2


def grid_case(seed, n, c, per, classes):
    """Multiples of 1/64 in [-1, 1]: every product is a multiple of 2^-12 and every partial sum below 2^12, exact in
    fp32.  Classes 1 and classes-1 copy class 0, and W is coarse (multiples of 1/4), so exact ties are everywhere."""
    r = np.random.default_rng(seed)
    fin = c * per
    pooled = r.integers(-64, 65, (n, fin)).astype(np.float32) / 64
    weight = (r.integers(-4, 5, (classes, fin)) * 16).astype(np.float32) / 64
    bias = r.integers(-64, 65, classes).astype(np.float32) / 64
    if classes > 1:
        weight[[1, classes - 1]], bias[[1, classes - 1]] = weight[0], bias[0]
    return pooled, weight, bias, r


@pytest.mark.parametrize("n,c,per,classes", [(1, 8, 1, 2), (70, 512, 1, 10), (130, 512, 4, 8), (64, 64, 49, 10)])
def test_prune_sweep_exact_on_grid_data(m, n, c, per, classes):
    pooled, weight, bias, r = grid_case(11 + n, n, c, per, classes)
    ties = 0
    for order in (r.permutation(c), np.arange(c)):
        logits, _ = levels_fp64(pooled, weight, bias, order, per)
        pred = logits.argmax(axis=2)                                     # numpy: the first maximal class, as torch.argmax
        ties += int((margins(logits) == 0).sum())
        targets = pred[r.integers(0, c, n), np.arange(n)]                # each image's prediction at a level of its own
        targets2 = r.integers(0, classes, n)
        want, want2 = (pred == targets).sum(axis=1), (pred == targets2).sum(axis=1)
        got, got2 = sweep(m, pooled, weight, bias, order, per, targets, targets2)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got2.cpu().numpy(), want2)
        got1, none = sweep(m, pooled, weight, bias, order, per, targets)          # targets2 = NULL
        assert none is None and np.array_equal(got1.cpu().numpy(), want)
        if n > 1:       # two calls on the halves of the batch add up to one call on the whole
            h = n // 2
            acc, acc2 = sweep(m, pooled[:h], weight, bias, order, per, targets[:h], targets2[:h])
            sweep(m, pooled[h:], weight, bias, order, per, targets[h:], targets2[h:], acc, acc2)
            assert np.array_equal(acc.cpu().numpy(), want) and np.array_equal(acc2.cpu().numpy(), want2)
    assert ties * 16 > n * c, ties                                         # exact ties at the top are common, not rare


def test_prune_sweep_refusals_and_empty_batch(m):
    lib = m["lib"]
    n, c, per, classes = 4, 8, 1, 3
    pooled, weight, bias, r = grid_case(5, n, c, per, classes)
    p, w, b = dev(pooled), dev(weight), dev(bias)
    order, t = dev(np.arange(c), torch.int32), dev(np.zeros(n), torch.int64)
    cells = torch.full((2, c), 7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n=n, c=c, per=per, classes=classes, t2=t.data_ptr(), c2=cells[1].data_ptr()):
        return lib.combat_prune_sweep(p.data_ptr(), n, w.data_ptr(), b.data_ptr(), order.data_ptr(), c, per, classes,
                                      t.data_ptr(), t2, cells[0].data_ptr(), c2, st)

    assert call(classes=17) == EINVAL and call(classes=0) == EINVAL
    assert call(c=0) == EINVAL and call(n=-1) == EINVAL
    for bad in (0, 2, 3, 16, 48, 50):
        assert call(per=bad) == EINVAL
    assert call(t2=None) == EINVAL and call(c2=None) == EINVAL           # one of the second pair without the other
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (cells == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (cells[0] >= 7).all() and int(cells[0].sum()) > 7 * c


def test_prune_sweep_gaussian_and_bitwise_repeatable(m):
    n, c, per, classes = 70, 512, 1, 10
    r = np.random.default_rng(2024)
    pooled = r.standard_normal((n, c)).astype(np.float32)
    weight = (r.standard_normal((classes, c)) / np.sqrt(c)).astype(np.float32)
    bias = (0.1 * r.standard_normal(classes)).astype(np.float32)
    order = r.permutation(c)
    logits, mass = levels_fp64(pooled, weight, bias, order, per)
    excluded = margins(logits) < fp32_margin(mass, c * per)              # [C][n]
    print("excluded %d of %d pairs" % (excluded.sum(), excluded.size))
    assert excluded.mean() <= 0.01
    pred = logits.argmax(axis=2)
    targets = pred[r.integers(0, c, n), np.arange(n)]
    hit = pred == targets
    lib = m["lib"]
    was = lib.combat_get_deterministic()
    lib.combat_set_deterministic(0)
    try:
        # one image per call: the per-pair outcomes, so that exactly the excluded pairs can be left out
        per_image = torch.zeros(n, c, dtype=torch.int32, device="cuda")
        for i in range(n):
            sweep(m, pooled[i:i + 1], weight, bias, order, per, targets[i:i + 1], correct=per_image[i])
        got = per_image.cpu().numpy().T.astype(bool)                     # [C][n]
        assert np.array_equal(got[~excluded], hit[~excluded])
        a, _ = sweep(m, pooled, weight, bias, order, per, targets)
        b, _ = sweep(m, pooled, weight, bias, order, per, targets)
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got.sum(axis=1))
    finally:
        lib.combat_set_deterministic(was)


@pytest.mark.parametrize("n,fin", [(1, 8), (70, 512), (33, 2048)])
def test_feature_colsum(m, n, fin):
    r = np.random.default_rng(n)
    x = (r.standard_normal((n, fin)) * 10 ** r.uniform(-3, 3, (1, fin))).astype(np.float32)
    acc = torch.zeros(fin, dtype=torch.float64, device="cuda")
    m["ops"].feature_colsum(dev(x), acc)
    want = x.astype(np.float64).sum(axis=0)
    scale = np.abs(x.astype(np.float64)).sum(axis=0)
    assert (np.abs(acc.cpu().numpy() - want) <= 1e-12 * scale).all()
    m["ops"].feature_colsum(dev(x[: n // 2 + 1]), acc)                   # accumulates
    want2 = want + x[: n // 2 + 1].astype(np.float64).sum(axis=0)
    assert (np.abs(acc.cpu().numpy() - want2) <= 1e-12 * 2 * scale).all()
    assert m["lib"].combat_feature_colsum(dev(x).data_ptr(), -1, fin, acc.data_ptr(), None) == EINVAL


def synth_images(b, hw, seed):
    """tests/golden/make_golden.py::synth_images."""
    u8 = torch.randint(0, 256, (b, 3, hw, hw), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return (u8.float() / 255 - 0.5) / 0.5


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


@pytest.fixture(scope="module")
def fixture_net(m, golden):
    g = golden("fine_pruning")
    torch.manual_seed(int(g["seeds"][0]))
    net = randomize_bn_buffers(m["nets"].PreActResNet18(), int(g["seeds"][1])).eval()
    return net, synth_images(int(g["n_images"]), 32, int(g["seeds"][2]))


@torch.no_grad()
def check_against_slow_path(m, net, x, order, levels):
    """The sweep's counters against the module's own eval forward with the pruned columns of `linear` zeroed."""
    net = net.cuda()
    fp = m["defenses"].FinePruning(net)
    per, c = fp.per, fp.C
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    w0 = state["linear.weight"].cpu().numpy()
    xg = x.cuda()
    pooled = m["api"].pooled_features(net, xg)
    p64 = np.abs(pooled.cpu().numpy().astype(np.float64))
    base = net(xg).argmax(1).cpu()
    targets = base.clone()
    targets[::3] = torch.randint(0, w0.shape[0], (len(targets[::3]),), generator=torch.Generator().manual_seed(1))
    fp.sweep(pooled, targets.cuda(), order=torch.from_numpy(order))
    all_counts = fp.counts()[0, 0]
    try:
        for k in levels:
            cols = (order[:k, None] * per + np.arange(per)[None, :]).reshape(-1)
            wk = w0.copy()
            wk[:, cols] = 0
            net.load_state_dict(dict(state, **{"linear.weight": torch.from_numpy(wk).cuda()}))
            slow = net(xg).cpu().numpy().astype(np.float64)
            mass = (np.abs(state["linear.bias"].cpu().numpy().astype(np.float64))[None, :]
                    + p64 @ np.abs(wk.astype(np.float64)).T).max(axis=1)
            keep = np.nonzero(margins(slow) >= fp32_margin(mass, c * per))[0]
            want = int((slow[keep].argmax(axis=1) == targets.numpy()[keep]).sum())
            if len(keep) == len(x):
                got = int(all_counts[k])
            else:
                sub = m["defenses"].FinePruning(net)
                sub.sweep(pooled[torch.from_numpy(keep).cuda()], targets[keep].cuda(), order=torch.from_numpy(order))
                got = int(sub.counts()[0, 0][k])
            assert got == want, (k, got, want)
    finally:
        net.load_state_dict(state)
    assert 0 < all_counts[0] <= len(x)


def test_sweep_equals_slow_path_preact(m, golden, fixture_net):
    net, x = fixture_net
    check_against_slow_path(m, net, x, golden("fine_pruning")["seq_sort"], (0, 1, 2, 255, 511))


def test_sweep_equals_slow_path_resnet64(m):
    torch.manual_seed(4)
    net = randomize_bn_buffers(m["nets"].ResNet18(num_classes=8), 900).eval()
    order = np.random.default_rng(9).permutation(512).astype(np.int64)
    check_against_slow_path(m, net, synth_images(16, 64, 8900), order, (0, 1, 2, 255, 511))


@torch.no_grad()
def test_pooled_features_is_the_eval_pass(m, fixture_net):
    net, x = fixture_net
    net = net.cuda()
    xg = x.cuda()[:19]                                                   # a ragged batch: padded to 32 inside
    logits = net(xg)
    eng = net._net_engine()
    slots = {k: set(s.plans) for k, s in eng.slots.items()}
    sizes = {k: {name: len(p) for name, p in s.plans.items() if hasattr(p, "calls")} for k, s in eng.slots.items()}
    pooled = m["api"].pooled_features(net, xg)
    assert pooled.shape == (19, 512) and pooled.dtype == torch.float32
    assert {k: set(s.plans) for k, s in eng.slots.items()} == slots          # no slot, no plan, no launch added
    assert {k: {name: len(p) for name, p in s.plans.items() if hasattr(p, "calls")} for k, s in eng.slots.items()} == sizes
    again = pooled.double() @ net.linear.weight.double().T + net.linear.bias.double()
    assert (again - logits.double()).abs().max() < 1e-4
    net.train()
    with pytest.raises(ValueError, match="eval mode"):
        m["api"].pooled_features(net, xg)
    net.eval()


@torch.no_grad()
def test_activation_and_order_against_the_reference(m, golden, fixture_net):
    g = golden("fine_pruning")
    net, x = fixture_net
    ref = g["activation"].astype(np.float64)
    # the bf16 emulation of the same forward: an identity `linear` hands the pooled features through unchanged
    p = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    p["linear.weight"], p["linear.bias"] = torch.eye(512), torch.zeros(512)
    with torch.no_grad():
        emu = E.preact_forward_emu(p, x, False).double().mean(0).numpy()
    fp = m["defenses"].FinePruning(net.cuda())
    fp.observe(x[:20].cuda())
    fp.observe(x[20:].cuda())
    assert fp.seen == 32
    ours = fp.activation()
    norm = float(np.linalg.norm(ref))
    e, e_emu = float(np.linalg.norm(ours - ref)) / norm, float(np.linalg.norm(emu - ref)) / norm
    print("activation: engine vs fp32 %.3e, emulation vs fp32 %.3e, ratio %.3f" % (e, e_emu, e / e_emu))
    assert e < 1.6 * e_emu, (e, e_emu)
    # the order: only where the reference's own gaps are wider than twice the emulation's distance
    order, seq = fp.order().numpy(), g["seq_sort"]
    assert order.dtype == np.int64 and np.array_equal(order, np.argsort(ours, kind="stable"))
    srt = ref[seq]
    gap = np.minimum(np.diff(srt, prepend=-np.inf), np.diff(srt, append=np.inf))     # to the nearest neighbour, by rank
    sure = np.nonzero(gap > 2 * e_emu * norm)[0]
    print("channels with a decided rank: %d" % len(sure))
    assert np.array_equal(order[sure], seq[sure])


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_end_to_end_on_synthetic_data(m, tmp_path, capsys):
    nets = m["nets"]
    script = _load(os.path.join(ROOT, "defenses", "fine_pruning", "fine-pruning.py"), "fine_pruning_script")
    torch.manual_seed(21)
    netC = randomize_bn_buffers(nets.PreActResNet18(), 300)
    torch.manual_seed(22)
    netG = nets.UnetGenerator(None)
    folder = tmp_path / "ck" / "t_clean" / "cifar10"
    folder.mkdir(parents=True)
    torch.save({"netC": netC.state_dict(), "netG": netG.state_dict(), "best_clean_acc": 12.5, "best_bd_acc": 99.0},
               str(folder / "cifar10_t_clean.pth.tar"))
    outs = [str(tmp_path / ("results%d.txt" % i)) for i in range(2)]
    argv = ["--dataset", "cifar10", "--saving_prefix", "t", "--checkpoints", str(tmp_path / "ck"), "--synthetic",
            "--synthetic_size", "200", "--bs", "100", "--seed", "5"]
    fp = script.main(argv + ["--outfile", outs[0]])
    printed = capsys.readouterr().out
    assert "12.5 99.0" in printed and "Pruned 0 filters" in printed and "Pruned 511 filters" in printed
    assert fp.seen == 200 and fp.swept == [200, 200]
    script.main(argv + ["--outfile", outs[1]])
    capsys.readouterr()
    text = open(outs[0]).read()
    assert text == open(outs[1]).read()                                   # same seed, same file
    rows = [l.split() for l in text.splitlines()]
    assert len(rows) == 512 and [int(r[0]) for r in rows] == list(range(512))
    assert all(len(r) == 3 and len(r[1].split(".")[1]) == 4 and len(r[2].split(".")[1]) == 4 for r in rows)
    # line 0 is the intact network: the repository's eval loop on the same data
    ev = _load(os.path.join(ROOT, "eval.py"), "eval_script")
    from combat_amd.data import get_dataloader
    from combat_amd.dist import NullWriter
    opt = script.get_arguments().parse_args(argv)
    script.configure_dataset(opt)
    acc_clean = ev.eval(fp.netC, netG.cuda().eval(), get_dataloader(opt, False, shuffle=False), NullWriter(), opt)[0]
    capsys.readouterr()
    assert rows[0][1] == "%0.4f" % acc_clean
    assert int(fp.counts()[0, 0][0]) == round(acc_clean * 2)
    last = float(rows[511][1])
    assert 0.0 <= last <= 100.0 and abs(last * 2 - round(last * 2)) < 1e-9   # a count out of 200 images
