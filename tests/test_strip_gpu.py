"""STRIP defense on the MI355X: combat_strip_superimpose bit for bit against the host restatement of the reference's
blend (packed by combat_image_to_c8), its refusals, combat_strip_entropy against exact cases and the fp64 restatement,
Strip.entropies against the slow path (host blends, the module's own eval forward), backdoor_backgrounds against numpy,
and defenses/STRIP/STRIP.py end to end on synthetic data."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
EINVAL = -1
ENTROPY_TOL = 2e-5   # derived, not measured: a term p * log2(p) is at most 0.531, its fp32 error a few ulp of p times
#                      |log2 p + 1.44|, under about 1e-6; the division by S cancels the row count, so at most
#                      classes = 16 such errors add


@pytest.fixture(scope="module")
def m():
    from combat_amd import _lib, api, defenses, engine, nets, ops
    return dict(lib=_lib.lib, api=api, defenses=defenses, engine=engine, nets=nets, ops=ops)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def strip_images(n, hw, seed):
    """uint8 [n][hw][hw][3] noise; image 0 walks every byte value in each run of 256 bytes and image 1 is constant over
    such a run (0, then 255, then other steps), so image 0 + image 1 takes every sum 0..510."""
    x = np.random.default_rng(seed).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    k = np.arange(hw * hw * 3, dtype=np.int64).reshape(hw, hw, 3)
    x[0] = (k % 256).astype(np.uint8)
    steps = np.array([0, 255] + [(23 * j) % 256 for j in range(2, hw * hw * 3 // 256)])
    x[1] = steps[k // 256].astype(np.uint8)
    return x


def packed_reference(m, backgrounds, dataset, index, norm_cols):
    """int16 view of combat_image_to_c8 applied to the host restatement's float32 batch, image b * S + s."""
    b, s = index.shape
    blends = np.concatenate([m["defenses"].strip_blend_reference(backgrounds[i][None], dataset[index[i]], norm_cols)
                             for i in range(b)])
    hw = blends.shape[-1]
    out = torch.zeros(b * s, hw, hw, 8, dtype=torch.bfloat16, device="cuda")
    m["ops"].image_to_c8(dev(blends), out)
    return out.view(torch.int16).cpu()


SENTINEL = 0x1234


def superimpose(m, backgrounds, dataset, index, norm_cols, rows):
    hw = backgrounds.shape[1]
    out = torch.full((rows, hw, hw, 8), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    m["ops"].strip_superimpose(dev(backgrounds), dev(dataset), dev(index, torch.int32), norm_cols, out)
    return out.view(torch.int16).cpu()


@pytest.mark.parametrize("norm_cols", [0, 3, 32])
def test_superimpose_bit_exact_cifar_shape(m, norm_cols):
    data = strip_images(37, 32, 31)
    backgrounds = np.stack([data[0], strip_images(3, 32, 32)[2], data[36]])      # the ramp on top of dataset[1]: all sums
    index = np.array([[1, 0, 36, 36, 5], [0, 36, 17, 17, 1], [36, 0, 0, 9, 20]])
    sums = backgrounds[0].astype(np.int32) + data[1].astype(np.int32)
    assert set(np.unique(sums).tolist()) == set(range(511))
    got = superimpose(m, backgrounds, data, index, norm_cols, 16)                # B * S = 15 in a slot of 16
    want = packed_reference(m, backgrounds, data, index, norm_cols)
    assert torch.equal(got[:15], want)
    assert (got[15] == SENTINEL).all()                                           # the padding image is not written
    assert (got[:15, :, :, 6:] == 0).all()


@pytest.mark.parametrize("hw,b,s", [(64, 1, 2), (224, 1, 1)])
def test_superimpose_bit_exact_large_images(m, hw, b, s):
    data = strip_images(3, hw, 40 + hw)
    backgrounds = data[:1]
    index = np.array([[1, 2][:s]])
    got = superimpose(m, backgrounds, data, index, 3, b * s)
    assert torch.equal(got, packed_reference(m, backgrounds, data, index, 3))


def test_superimpose_refusals_and_empty_cases(m):
    lib = m["lib"]
    hw, b, s, n_data = 32, 2, 3, 5
    data = strip_images(n_data, hw, 7)
    bg, ds, idx = dev(data[:b]), dev(data), dev(np.array([[0, 1, 2], [4, 4, 0]]), torch.int32)
    out = torch.full((16, hw, hw, 8), SENTINEL, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(bg=bg.data_ptr(), b=b, ds=ds.data_ptr(), n_data=n_data, idx=idx.data_ptr(), s=s, hw=hw, norm_cols=3,
             out=out.data_ptr()):
        return lib.combat_strip_superimpose(bg, b, ds, n_data, idx, s, hw, norm_cols, out, st)

    assert call(bg=None) == EINVAL and call(ds=None) == EINVAL and call(idx=None) == EINVAL and call(out=None) == EINVAL
    for bad in (0, 16, 31, 33, 128, 223, 256):
        assert call(hw=bad) == EINVAL
    assert call(norm_cols=-1) == EINVAL and call(norm_cols=33) == EINVAL
    assert call(b=1 << 16, s=1 << 15) == EINVAL                                  # B * S = 2^31
    assert call(b=-1) == EINVAL and call(s=-1) == EINVAL and call(n_data=-1) == EINVAL
    assert call(b=0) == 0 and call(s=0) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                               # nothing was launched
    # an index outside the dataset adds nothing: the blend is the background itself, and nothing outside is read
    wild = dev(np.array([[-1, n_data, 2], [1 << 30, -(1 << 31), 0]]), torch.int32)
    assert call(idx=wild.data_ptr()) == 0 and call(norm_cols=0) == 0 and call(norm_cols=32) == 0
    assert call(idx=wild.data_ptr()) == 0
    torch.cuda.synchronize()
    zero = np.zeros_like(data[:1])
    want = packed_reference(m, data[:b], np.concatenate([data, zero]), np.array([[5, 5, 2], [5, 5, 0]]), 3)
    assert torch.equal(out[:6].cpu(), want) and (out[6:] == SENTINEL).all()


def entropy(m, logits, b, s):
    out = torch.full((b,), -1.0, dtype=torch.float32, device="cuda")
    m["ops"].strip_entropy(dev(logits, torch.float32), b, s, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("classes", [1, 8, 10, 16])
def test_entropy_of_zero_logits_is_exact(m, classes):
    for b, s in ((1, 1), (3, 5), (2, 100)):
        got = entropy(m, np.zeros((b * s, classes), np.float32), b, s)
        assert got.tolist() == [classes * 0.5] * b                                # every term is -0.5: exact sums


def test_entropy_skips_what_nansum_skips_and_refuses_bad_shapes(m):
    x = np.zeros((4, 10), np.float32)
    x[0, 0], x[1, 3], x[2, 5], x[3, 9] = -200.0, 200.0, np.nan, -np.inf
    assert entropy(m, x, 2, 2).tolist() == [4.5, 4.5]
    assert entropy(m, x, 1, 4).tolist() == [4.5]
    lib, st = m["lib"], torch.cuda.current_stream().cuda_stream
    lg, out = dev(x), torch.full((2,), 7.0, dtype=torch.float32, device="cuda")
    for b, s, classes in ((2, 2, 0), (2, 2, 17), (2, 0, 10), (-1, 2, 10), (1 << 16, 1 << 15, 10)):
        assert lib.combat_strip_entropy(lg.data_ptr(), b, s, classes, out.data_ptr(), st) == EINVAL
    assert lib.combat_strip_entropy(None, 2, 2, 10, out.data_ptr(), st) == EINVAL
    assert lib.combat_strip_entropy(lg.data_ptr(), 2, 2, 10, None, st) == EINVAL
    assert lib.combat_strip_entropy(lg.data_ptr(), 0, 2, 10, out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [7.0, 7.0]


@pytest.mark.parametrize("s", [1, 5, 100])
def test_entropy_gaussian_logits_and_bitwise_repeatable(m, s):
    b, classes = 3, 10
    x = (4.0 * np.random.default_rng(50 + s).standard_normal((b * s, classes))).astype(np.float32)
    want = m["defenses"].strip_entropy_reference(x, s)
    first, again = entropy(m, x, b, s), entropy(m, x, b, s)
    err = np.abs(first.astype(np.float64) - want)
    print("S = %d: entropy %s, max error %.3e" % (s, first.tolist(), err.max()))
    assert (err <= ENTROPY_TOL).all()
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))


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


def host_blends(m, backgrounds, data, index, norm_cols=3):
    return torch.from_numpy(np.concatenate([m["defenses"].strip_blend_reference(backgrounds[i][None], data[index[i]],
                                                                                norm_cols) for i in range(len(index))]))


@torch.no_grad()
def strip_logits(m, net, det, n):
    """The logits Strip.entropies left in the classifier's buffer: the last group's n images."""
    eng = net._net_engine()
    slot = eng.slot("module.eval", m["engine"].pad_batch(n), det.hw)
    return eng.head_bufs(slot)["logits"][:n].clone()


@torch.no_grad()
def test_entropies_equal_the_slow_path_preact(m):
    D = m["defenses"]
    torch.manual_seed(0)
    net = randomize_bn_buffers(m["nets"].PreActResNet18(), 500).cuda().eval()
    data = strip_images(37, 32, 61)
    backgrounds = strip_images(3, 32, 62)
    index = np.array([[0, 36, 36, 5, 12], [1, 0, 17, 17, 30], [36, 2, 0, 9, 20]])
    b, s = index.shape

    class Det(D.Strip):
        G = 3

    det = Det(net, data.transpose(0, 3, 1, 2))                                   # NCHW, as combat_amd.data holds it
    assert det.norm_cols == 3 and det.n_data == 37 and det.group(s) == 3
    got = det.entropies(backgrounds, index)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (b,)
    fast_logits = strip_logits(m, net, det, b * s)
    x = host_blends(m, backgrounds, data, index).cuda()
    slow_logits = net(x)                                                          # 15 images: the same slot of 16
    assert torch.equal(fast_logits, slow_logits)                                  # same input bits, same plan, no atomics
    want = D.strip_entropy_reference(slow_logits.cpu().numpy(), s)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print("entropies %s, max error against fp64 %.3e" % (got.tolist(), err.max()))
    assert (err <= ENTROPY_TOL).all()

    # a ragged last group: two passes that may pick other plans than the one above.  What that can cost is what the
    # slow path itself pays between a slot of 16 and a slot of 32 for the same 15 images, plus the two entropy
    # kernels' own bound
    wide = net(torch.cat([x, x[:2]]))[:b * s]                                      # 17 images: a slot of 32
    plan_gap = np.abs(D.strip_entropy_reference(wide.cpu().numpy(), s) - want).max()

    class Det2(D.Strip):
        G = 2

    det2 = Det2(net, data)                                                        # NHWC is taken as it is
    assert det2.group(s) == 2
    ragged = det2.entropies(torch.from_numpy(backgrounds).cuda(), torch.from_numpy(index))
    gap = np.abs(ragged.cpu().numpy().astype(np.float64) - got.cpu().numpy().astype(np.float64)).max()
    print("G = 2 against G = 3: %.3e (slot 16 against slot 32 on the slow path: %.3e)" % (gap, plan_gap))
    assert gap <= plan_gap + 2 * ENTROPY_TOL

    # the switch: the whole image normalised is another input, and the validation happens before any launch
    full = D.Strip(net, data, norm_cols=32).entropies(backgrounds, index)
    assert not torch.equal(full, got)
    x_full = host_blends(m, backgrounds, data, index, 32).cuda()
    assert (np.abs(full.cpu().numpy() - D.strip_entropy_reference(net(x_full).cpu().numpy(), s)) <= ENTROPY_TOL).all()
    with pytest.raises(ValueError, match="outside the dataset"):
        det.entropies(backgrounds, np.array([[0, 1, 2, 3, 37]] * 3))
    with pytest.raises(ValueError, match="outside the dataset"):
        det.entropies(backgrounds, np.array([[0, 1, 2, 3, -1]] * 3))
    assert tuple(det.entropies(backgrounds[:0], index[:0]).shape) == (0,)
    net.train()
    with pytest.raises(ValueError, match="eval mode"):
        D.Strip(net, data)
    net.eval()


@torch.no_grad()
def test_entropies_equal_the_slow_path_resnet64(m):
    D = m["defenses"]
    torch.manual_seed(4)
    net = randomize_bn_buffers(m["nets"].ResNet18(num_classes=8), 900).cuda().eval()
    data = strip_images(6, 64, 71)
    backgrounds = strip_images(3, 64, 72)[2:]
    index = np.array([[0, 5, 5, 3]])
    det = D.Strip(net, data)
    assert det.classes == 8 and det.group(4) == det.G
    got = det.entropies(backgrounds, index)
    slow = net(host_blends(m, backgrounds, data, index).cuda())
    assert torch.equal(strip_logits(m, net, det, 4), slow)
    want = D.strip_entropy_reference(slow.cpu().numpy(), 4)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= ENTROPY_TOL).all()


class Opt:
    noise_rate, ratio, kernel_size, sigma = 0.08, 0.65, 3, (0.1, 1.0)


@torch.no_grad()
def test_backdoor_backgrounds_equal_numpy(m):
    torch.manual_seed(22)
    netG = m["nets"].UnetGenerator(None).cuda().eval()
    u8 = torch.randint(0, 256, (5, 3, 32, 32), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    x = ((u8.float() / 255 - 0.5) / 0.5).cuda()
    got = m["defenses"].backdoor_backgrounds(netG, x, Opt, sigma=0.6)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (5, 32, 32, 3) and got.is_contiguous()
    bd = m["api"].create_backdoor(netG, x, Opt, sigma=0.6).cpu().numpy()
    assert bd.dtype == np.float32
    want = (bd * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0)           # STRIP.py:171, fp32
    want = np.clip(want, 0, 255).astype(np.uint8).transpose((0, 2, 3, 1))         # :173
    assert np.array_equal(got.cpu().numpy(), want)
    assert (got.cpu().numpy() != u8.permute(0, 2, 3, 1).numpy()).any()            # the trigger moved some bytes


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_end_to_end_on_synthetic_data(m, tmp_path, capsys, monkeypatch):
    nets, D = m["nets"], m["defenses"]
    script = _load(os.path.join(ROOT, "defenses", "STRIP", "STRIP.py"), "strip_script")
    torch.manual_seed(21)
    netC = randomize_bn_buffers(nets.PreActResNet18(), 300)
    torch.manual_seed(22)
    netG = nets.UnetGenerator(None)
    folder = tmp_path / "ck" / "t_clean" / "cifar10"
    folder.mkdir(parents=True)
    torch.save({"netC": netC.state_dict(), "netG": netG.state_dict()}, str(folder / "cifar10_t_clean.pth.tar"))
    argv = ["--dataset", "cifar10", "--saving_prefix", "t", "--checkpoints", str(tmp_path / "ck"), "--synthetic",
            "--synthetic_size", "40", "--seed", "5", "--n_test", "4", "--n_sample", "6", "--test_rounds", "2"]

    def run(name, extra):
        results = str(tmp_path / name)
        troj, ben = script.main(argv + ["--results", results] + extra)
        printed = capsys.readouterr().out
        lines = open(os.path.join(results, "cifar10", "cifar10_result.txt")).read().split("\n")
        assert len(lines) == 2
        rows = [[float(v) for v in line.split(" ")] if line else [] for line in lines]
        assert rows == [troj, ben]
        low = min(troj + ben)
        assert "Min entropy trojan: {}, Detection boundary: {}".format(low, script.get_arguments().parse_args(
            argv + extra).detection_boundary) in printed
        return rows, printed

    (troj, ben), printed = run("attack", [])                                     # "2" in "all2one": attack mode
    assert printed.startswith("attack\n") and len(troj) == 8 and len(ben) == 8
    assert "Not a backdoor model" in printed and "A backdoored model" not in printed   # entropies near 5 >= 0.2
    (_, _), printed = run("boundary", ["--detection_boundary", "100"])
    assert "A backdoored model" in printed and "Not a backdoor model" not in printed
    (troj_c, ben_c), printed = run("clean", ["--attack_mode", "clean"])
    assert printed.startswith("clean\n") and troj_c == [] and len(ben_c) == 8
    (troj_f, ben_f), _ = run("full", ["--full_normalize"])
    assert troj_f != troj and ben_f != ben

    # the same values from Strip.entropies, with the script's seeds and its order of draws
    opt = script.get_arguments().parse_args(argv)
    script.configure_dataset(opt)
    torch.manual_seed(5)
    np.random.seed(5)
    random.seed(5)
    c2, g2 = script.get_model(opt, "attack")
    state = torch.load(script.checkpoint_path(opt), map_location="cuda", weights_only=True)
    c2.load_state_dict(state["netC"])
    g2.load_state_dict(state["netG"])
    c2.eval()
    g2.eval()
    from combat_amd.data import get_dataloader
    dl = get_dataloader(opt, False)
    det = D.Strip(c2, dl.x, opt)
    want_t, want_b = [], []
    for _ in range(2):
        inputs, _labels = next(iter(dl))
        bg = D.backdoor_backgrounds(g2, inputs.cuda(), opt)
        idx = np.stack([np.random.randint(0, 40, size=6) for _ in range(4)])
        want_t += det.entropies(bg, idx).cpu().tolist()
        idx = np.stack([np.random.randint(0, 40, size=6) for _ in range(4)])
        want_b += det.entropies(det.data[:4], idx).cpu().tolist()
    assert want_t == troj and want_b == ben
    capsys.readouterr()

    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="^STRIP runs on a single GPU.*world size 2"):
        script.main(argv + ["--results", str(tmp_path / "refused")])
    assert not os.path.exists(str(tmp_path / "refused"))
