"""Neural Cleanse defense on the MI355X: combat_nc_blend against the host restatement (packed by combat_image_to_c8), its
refusals, combat_nc_update's gradients against the fp64 restatement, its Adam step, statistics row and cells, the
NeuralCleanse step against the reference's recorded steps (tests/golden/neural_cleanse.npz), replay against eager calls,
an epoch with a tail batch, and defenses/neural_cleanse/neural_cleanse.py end to end on synthetic data."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = 0x1234

# Measured on the CPU by tests/test_neural_cleanse_cpu.py::test_bf16_emulation_distances (the reference's fp32 steps
# against the same steps under the bf16 emulation of the classifier); the same constants stand there and in DESIGN.md
# section 10.  The engine is allowed twice as much: the emulation models neither the bf16 rounding of gradient tensors and
# of 'g.img' nor the kernels' summation order.
E_GRAD = 2.0e-2            # measured 1.975e-2 (the pattern's gradient; the mask's: 5.1e-3)
E_TRAJ = 2.8e-5            # measured 2.705e-5
LR_CAP = 0.02

# combat_nc_blend against the host restatement, both read as hi + lo.  |value| <= 2.3: x is in [-1, 1] and the normalised
# pattern of rows 0..2 within (0 - 0.4914) / 0.247 = -2.0 .. (1 - 0.4465) / 0.261 = 2.2.  The hi / lo split keeps a value
# to 2^-8 (hi) * 2^-9 (lo, rounded to nearest) = 2^-17 of itself, on either side of the comparison: 2 * 2.3 * 2^-17 = 3.5e-5.
# The two sides' fp32 values differ by a few ulp of tanhf (4 * 2^-24, times 1 / (2 * 0.243) through the normalisation) and
# a few fp32 roundings of a value up to 2.3 (fused multiply-adds on the device): under 2e-6.
BLEND_TOL = 2 * 2.3 * 2.0 ** -17 + 2e-6


@pytest.fixture(scope="module")
def m():
    from combat_amd import _lib, defenses, engine, nets, ops
    return dict(lib=_lib.lib, defenses=defenses, engine=engine, nets=nets, ops=ops)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


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


def images(n, hw, seed):
    x = np.random.default_rng(seed).integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    x[0].reshape(-1)[:256] = np.arange(256)                              # every byte value
    return x


def params(hw, seed):
    g = np.random.default_rng(seed)
    return (g.normal(0, 1.5, (hw, hw)).astype(np.float32), g.normal(0, 1.5, (3, hw, hw)).astype(np.float32))


def norm_cells(m):
    D = m["defenses"]
    return torch.tensor(D.NC_MEAN + D.NC_STD, dtype=torch.float32, device="cuda")


def hi_plus_lo(c8):
    """float32 [n][3][hw][hw] of a c8 hi/lo buffer."""
    v = c8.float()
    return (v[..., 0:3] + v[..., 3:6]).permute(0, 3, 1, 2).cpu().numpy()


def packed(m, x):
    out = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 8, dtype=torch.bfloat16, device="cuda")
    m["ops"].image_to_c8(dev(x), out)
    return out


# ---------------------------------------------------------------- combat_nc_blend


@pytest.mark.parametrize("hw,n,N", [(32, 5, 16), (32, 16, 16), (64, 3, 16), (224, 1, 16)])
def test_blend_equals_the_host_restatement(m, hw, n, N):
    D, ops = m["defenses"], m["ops"]
    data = images(7, hw, 100 + hw)
    bs = 16
    order = np.random.default_rng(5).integers(0, 7, 2 * bs).astype(np.int32)          # two steps' worth; step 1 is blended
    mt, pt = params(hw, 200 + hw)
    buf = torch.full((N + 1, hw, hw, 8), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    cursor = torch.tensor([1], dtype=torch.int32, device="cuda")
    ops.nc_blend(dev(data), dev(order), cursor, bs, n, dev(mt), dev(pt), 1e-7, norm_cells(m), buf[:N])
    got = buf.view(torch.int16)
    want = D.nc_blend_reference(data[order[bs:bs + n]], mt, pt, 1e-7)
    err = np.abs(hi_plus_lo(buf[:n]) - hi_plus_lo(packed(m, want))).max()
    print("hw %d n %d: max error %.3e (allowed %.3e), values within %.2f" % (hw, n, err, BLEND_TOL, np.abs(want).max()))
    assert err <= BLEND_TOL and np.abs(want).max() <= 2.3
    assert (got[:n, :, :, 6:] == 0).all()
    assert (got[n:N] == 0).all()                                                    # the padding rows: zero pixels
    assert (got[N] == SENTINEL).all()                                               # beyond the slot: untouched
    assert int(cursor.item()) == 1
    # rows 0..2 of the pattern are normalised, rows 3.. are not: a saturated mask shows the pattern alone
    ops.nc_blend(dev(data), dev(order), cursor, bs, n, dev(np.full((hw, hw), 30.0, np.float32)), dev(pt), 1e-7, norm_cells(m),
                 buf[:N])
    alone = hi_plus_lo(buf[:1])[0]
    assert alone[:, 3:].min() >= 0.0 and alone[:, 3:].max() <= 1.0 and alone[:, :3].min() < -0.5


def test_blend_refusals_and_wild_indices(m):
    lib, D = m["lib"], m["defenses"]
    hw, n_data, bs, N = 32, 5, 16, 16
    data = images(n_data, hw, 7)
    mt, pt = params(hw, 8)
    ds, idx, cur = dev(data), dev(np.arange(16) % n_data, torch.int32), torch.zeros(1, dtype=torch.int32, device="cuda")
    dmt, dpt, nm = dev(mt), dev(pt), norm_cells(m)
    out = torch.full((N, hw, hw, 8), SENTINEL, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(ds=ds.data_ptr(), n_data=n_data, idx=idx.data_ptr(), n_index=16, cur=cur.data_ptr(), bs=bs, n=4, N=N, hw=hw,
             mt=dmt.data_ptr(), pt=dpt.data_ptr(), nm=nm.data_ptr(), out=out.data_ptr()):
        return lib.combat_nc_blend(ds, n_data, idx, n_index, cur, bs, n, N, hw, mt, pt, 1e-7, nm, out, st)

    for bad in (0, 16, 31, 33, 128, 223, 256):
        assert call(hw=bad) == EINVAL
    assert call(n=N + 1) == EINVAL and call(n=-1) == EINVAL and call(bs=0) == EINVAL and call(N=0, n=0) == EINVAL
    for name in ("ds", "idx", "cur", "mt", "pt", "nm", "out"):
        assert call(**{name: None}) == EINVAL, name
    assert call(ds=ds.data_ptr() + 1) == EINVAL and call(idx=idx.data_ptr() + 2) == EINVAL
    assert call(mt=dmt.data_ptr() + 4) == EINVAL and call(pt=dpt.data_ptr() + 8) == EINVAL and call(out=out.data_ptr() + 8) == EINVAL
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                                   # nothing was launched
    # an index outside the dataset, or past the end of the index, reads nothing: x = 0, the blend is m * p
    wild = dev(np.array([-1, n_data, 1 << 30, 2]), torch.int32)
    assert call(idx=wild.data_ptr(), n_index=4, n=6) == 0                            # rows 4, 5 lie past the index
    torch.cuda.synchronize()
    black = D.nc_blend_reference(np.zeros((1, hw, hw, 3), np.uint8), mt, pt)
    white = D.nc_blend_reference(np.full((1, hw, hw, 3), 255, np.uint8), mt, pt)
    m_times_p = (black + white) / 2                                                  # x = -1 and x = +1 average to x = 0
    got = hi_plus_lo(out.view(torch.bfloat16)[:6])
    for row in (0, 1, 2, 4, 5):
        assert np.abs(got[row] - m_times_p[0]).max() <= BLEND_TOL, row
    assert np.abs(got[3] - D.nc_blend_reference(data[2:3], mt, pt)[0]).max() <= BLEND_TOL
    assert (out[6:] == 0).all()


# ---------------------------------------------------------------- combat_nc_update


class UpdateCase:
    """Device state of a stand-alone combat_nc_update: a synthetic gradient on a coarse bf16 grid (k / 64, |k| <= 32: exact
    in bf16), huge finite values in the padding rows of g_img and logits, which must not count."""

    def __init__(self, m, hw, n, N=16, bs=16, steps=3, classes=10, target=3, seed=1):
        self.m, self.hw, self.n, self.N, self.bs, self.steps, self.classes, self.target = m, hw, n, N, bs, steps, classes, target
        g = np.random.default_rng(seed)
        self.data = images(9, hw, seed + 10)
        self.order = g.integers(0, 9, steps * bs).astype(np.int32)
        self.g_img = (g.integers(-32, 33, (N, 3, hw, hw)) / 64.0).astype(np.float32)
        c8 = g.normal(0, 1, (N, hw, hw, 8)).astype(np.float32)           # channels 3..7: never read
        c8[..., 0:3] = self.g_img.transpose(0, 2, 3, 1)
        c8[n:] = 1e30
        self.logits = g.normal(0, 2, (N, classes)).astype(np.float32)
        self.logits[n:] = 1e30
        self.logits[0, target] = self.logits[0].max() + 1                # at least one hit, one exact tie elsewhere
        if n > 1:
            self.logits[1, :] = 0.5                                      # all equal: the first class is the argmax
        self.mt, self.pt = params(hw, seed + 20)
        self.cost, self.lr = 1e-3, 0.1
        self.d = dict(g_img=dev(c8, torch.bfloat16), data=dev(self.data), index=dev(self.order), logits=dev(self.logits),
                      norm=norm_cells(m))
        self.reset()

    def reset(self, cursor=0, t=0):
        hw = self.hw
        d = self.d
        d["params"] = dev(np.concatenate([self.mt[None], self.pt]))
        d["m1"], d["m2"] = torch.zeros(4, hw, hw, device="cuda"), torch.zeros(4, hw, hw, device="cuda")
        d["cells"] = torch.tensor([cursor, t], dtype=torch.int32, device="cuda")
        d["cost"] = torch.tensor([self.cost], dtype=torch.float32, device="cuda")
        d["stats"] = torch.full((self.steps, 4), -7.0, device="cuda")
        d["grad"] = torch.full((4, hw, hw), -7.0, device="cuda")

    def run(self, grad=True):
        d = self.d
        self.m["ops"].nc_update(d["g_img"], d["data"], d["index"], d["cells"][0:1], self.bs, self.n, d["logits"], self.target,
                                d["params"][0], d["params"][1:], d["m1"], d["m2"], 1e-7, d["norm"], self.lr, 0.5, 0.9, 1e-8,
                                d["cells"][1:2], d["cost"], d["stats"], d["grad"] if grad else None)

    def state(self):
        torch.cuda.synchronize()
        return {k: self.d[k].cpu().numpy().copy() for k in ("params", "m1", "m2", "cells", "stats", "grad")}

    def batch(self, step):
        return self.data[self.order[step * self.bs:step * self.bs + self.n]]


@pytest.mark.parametrize("hw,n", [(32, 5), (32, 16), (64, 3)])
def test_update_gradients_adam_and_statistics(m, hw, n):
    D = m["defenses"]
    case = UpdateCase(m, hw, n)
    g_before = case.d["g_img"].clone()
    data_before = case.d["data"].clone()
    ulp = 2.0 ** -23
    # an fp32 sum of 3n products |g| <= 0.5 times |p - x| <= 3.3, behind about 16 elementwise fp32 operations, plus the cost,
    # times the tanh chain (<= 0.5): every partial sum is within 3n * 1.65, so the error is within (3n + 16) roundings of that
    grad_tol = (3 * n + 16) * 2.0 ** -24 * (3 * n * 0.5 * 3.3 + case.cost) * 0.5
    mask, pattern = case.mt, case.pt
    m1, m2 = np.zeros((4, hw, hw), np.float32), np.zeros((4, hw, hw), np.float32)
    for step in range(3):
        case.run()
        s = case.state()
        gm, gp = D.nc_gradients_reference(case.g_img[:n], case.batch(step), mask, pattern, case.cost)
        want = np.concatenate([gm[None], gp])
        err = np.abs(s["grad"] - want).max()
        print("hw %d n %d step %d: gradient error %.3e (allowed %.3e, largest gradient %.3e)" % (hw, n, step, err, grad_tol,
                                                                                              np.abs(want).max()))
        assert err <= grad_tol and np.abs(want).max() > 100 * grad_tol
        # Adam from the launch's own gradient: a few ulp per quantity and step (fused multiply-adds, the order of the
        # update's operations); the parameters are within 8 in magnitude
        new, m1, m2 = D.nc_adam_reference(np.concatenate([mask[None], pattern]), s["grad"], m1, m2, step, case.lr)
        assert np.abs(s["params"] - new).max() <= 4 * ulp * 8 * (step + 1)
        assert (np.abs(s["m1"] - m1) <= 4 * ulp * (step + 1) * np.abs(m1) + 1e-30).all()
        assert (np.abs(s["m2"] - m2) <= 4 * ulp * (step + 1) * np.abs(m2) + 1e-30).all()
        # the statistics row: numpy in fp64 over the rows < n
        lg = case.logits[:n].astype(np.float64)
        ce = (np.log(np.exp(lg - lg.max(1, keepdims=True)).sum(1)) + lg.max(1) - lg[:, case.target]).mean()
        reg = (np.tanh(mask.astype(np.float64)) / (2 + 1e-7) + 0.5).sum()
        row = s["stats"][step]
        assert abs(row[0] - ce) <= 1e-6 * abs(ce) + 1e-6 and row[1] == float((lg.argmax(1) == case.target).sum())
        assert row[1] >= 1 and abs(row[2] - reg) <= 2e-6 * reg and row[3] == n
        assert (s["stats"][step + 1:] == -7.0).all()
        assert s["cells"].tolist() == [step + 1, step + 1]                       # cursor and t advance by one
        mask, pattern = s["params"][0], s["params"][1:]
    assert torch.equal(case.d["g_img"], g_before) and torch.equal(case.d["data"], data_before)   # read only
    # a cursor outside [0, steps) has no statistics row: nothing moves
    case.run()
    after = case.state()
    assert after["cells"].tolist() == [3, 3] and np.array_equal(after["params"], s["params"])
    # two runs from the same state give the same bits; without grad_out the same parameters
    case.reset()
    case.run()
    first = case.state()
    case.reset()
    case.run()
    second = case.state()
    case.reset()
    case.run(grad=False)
    third = case.state()
    for k in first:
        assert np.array_equal(first[k], second[k]), k
        assert k == "grad" or np.array_equal(first[k], third[k]), k
    assert (third["grad"] == -7.0).all()


def test_update_refusals(m):
    case = UpdateCase(m, 32, 4)
    d, lib = case.d, m["lib"]
    st = torch.cuda.current_stream().cuda_stream
    before = case.state()

    def call(hw=32, classes=10, n=4, N=16, target=3, steps=3, g=d["g_img"].data_ptr(), logits=d["logits"].data_ptr(),
             mt=d["params"].data_ptr(), t=d["cells"][1:2].data_ptr()):
        return lib.combat_nc_update(g, d["data"].data_ptr(), 9, d["index"].data_ptr(), 48, d["cells"].data_ptr(), 16, n, N, hw,
                                    logits, classes, target, mt, d["params"][1:].data_ptr(), d["m1"].data_ptr(),
                                    d["m2"].data_ptr(), 1e-7, d["norm"].data_ptr(), 0.1, 0.5, 0.9, 1e-8, t, d["cost"].data_ptr(),
                                    d["stats"].data_ptr(), steps, None, st)

    for bad in (0, 16, 31, 33, 128, 223, 256):
        assert call(hw=bad) == EINVAL
    assert call(classes=0) == EINVAL and call(classes=17) == EINVAL and call(target=10) == EINVAL and call(target=-1) == EINVAL
    assert call(n=17) == EINVAL and call(n=-1) == EINVAL and call(steps=0) == EINVAL
    assert call(g=None) == EINVAL and call(logits=None) == EINVAL and call(mt=None) == EINVAL and call(t=None) == EINVAL
    assert call(g=d["g_img"].data_ptr() + 8) == EINVAL and call(mt=d["params"].data_ptr() + 4) == EINVAL
    assert call(n=0) == 0
    after = case.state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k                            # nothing was launched
    with pytest.raises(ValueError, match="does not hold"):
        case.n = 17
        case.run()


# ---------------------------------------------------------------- the step through NeuralCleanse


def nc_opt(**over):
    opt = types.SimpleNamespace(bs=16, lr=0.1, EPSILON=1e-7, epoch=2, init_cost=1e-3, atk_succ_threshold=99.0, early_stop=True,
                                early_stop_threshold=99.0, early_stop_patience=25, patience=5, cost_multiplier=2,
                                dataset="cifar10", attack_mode="all2one")
    for k, v in over.items():
        setattr(opt, k, v)
    return opt


@pytest.fixture(scope="module")
def fixture_net(m, golden):
    g = golden("neural_cleanse")
    torch.manual_seed(int(g["seeds"][0]))
    return randomize_bn_buffers(m["nets"].PreActResNet18(), int(g["seeds"][1])).cuda().eval()


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("which,key", [("b_", "images"), ("c_", "images_ragged")])
def test_step_gradients_against_the_reference(m, golden, fixture_net, which, key):
    g = golden("neural_cleanse")
    data = g[key]
    n = len(data)
    nc = m["defenses"].NeuralCleanse(fixture_net, data, nc_opt())
    assert nc.steps == 1 and nc.batch_size(0) == n and nc.n_data == n
    nc.reset(np.ones((1, 32, 32), np.float32), np.ones((3, 32, 32), np.float32), float(g["cost"]))
    nc.set_index(np.arange(n))
    grad = torch.zeros(4, 32, 32, device="cuda")
    nc.step_plan(n, int(g["target_label"]), grad).run()
    got = grad.cpu().numpy()
    e_mask, e_pattern = rel_l2(got[0:1], g[which + "grad_mask"][0]), rel_l2(got[1:], g[which + "grad_pattern"][0])
    stats = nc.stats.cpu().numpy()[0]
    print("%s step-1 gradients: mask %.3e pattern %.3e (allowed %.3e); loss_ce %.6f (reference %.6f)"
          % (key, e_mask, e_pattern, 2 * E_GRAD, stats[0], g[which + "loss_ce"][0]))
    assert max(e_mask, e_pattern) <= 2 * E_GRAD
    assert abs(stats[0] - g[which + "loss_ce"][0]) <= 2 * E_TRAJ * g[which + "loss_ce"][0]
    assert abs(stats[2] - g[which + "loss_reg"][0]) <= 2 * E_TRAJ * g[which + "loss_reg"][0] and stats[3] == n
    assert nc.cells.cpu().tolist() == [1, 1]


def test_eight_steps_against_the_reference(m, golden, fixture_net):
    """loss_ce and loss_reg of every step within 2 * E_traj of the reference's.  Parameters are deliberately not compared
    element by element: Adam's first steps move every element by lr times the sign of its gradient, so an element whose
    gradient is near zero may legitimately land 0.2 away; instead at most 2 % of the elements may differ from the
    reference's by more than lr (the bf16 emulation stays under half of that on the CPU)."""
    g = golden("neural_cleanse")
    lr = float(g["lr"])
    nc = m["defenses"].NeuralCleanse(fixture_net, g["images"], nc_opt(lr=lr))
    nc.reset(np.ones((1, 32, 32), np.float32), np.ones((3, 32, 32), np.float32))
    worst = 0.0
    for step in range(8):
        row = nc.run_epoch(int(g["target_label"]), np.arange(16), float(g["cost"]))[0]
        e_ce = abs(row[0] - g["b_loss_ce"][step]) / g["b_loss_ce"][step]
        e_reg = abs(row[2] - g["b_loss_reg"][step]) / g["b_loss_reg"][step]
        print("step %d: loss_ce %.6f (%.2e) loss_reg %.4f (%.2e)" % (step, row[0], e_ce, row[2], e_reg))
        worst = max(worst, e_ce, e_reg)
        assert row[1] * 100.0 / row[3] == g["b_acc"][step] and row[3] == 16
    assert worst <= 2 * E_TRAJ
    got = nc.params.cpu().numpy().ravel()
    want = np.concatenate([g["b_mask_tanh"][-1].ravel(), g["b_pattern_tanh"][-1].ravel()])
    share = float((np.abs(got - want) > lr).mean())
    print("elements more than lr away: %.4f" % share)
    assert share <= LR_CAP
    assert nc.cells.cpu().tolist() == [1, 8]                                     # the cursor restarts, Adam's count does not


def snapshot(nc):
    torch.cuda.synchronize()
    return [t.clone() for t in (nc.params, nc.exp_avg, nc.exp_avg_sq, nc.cells, nc.stats)]


def test_replay_equals_eager_calls_and_tail_batch(m, fixture_net):
    D = m["defenses"]
    data = images(58, 32, 77)                                                    # 16 + 16 + 16 + 10
    nc = D.NeuralCleanse(fixture_net, data.transpose(0, 3, 1, 2), nc_opt())      # NCHW, as combat_amd.data holds it
    assert nc.steps == 4 and [nc.batch_size(s) for s in range(4)] == [16, 16, 16, 10]
    order = np.random.default_rng(3).permutation(58)
    ones = np.ones((1, 32, 32), np.float32), np.ones((3, 32, 32), np.float32)
    nc.reset(*ones, cost=1e-3)
    nc.set_index(order)
    plan = nc.step_plan(16, 4)
    for _ in range(3):
        plan.run()
    replayed = snapshot(nc)
    nc.reset(*ones, cost=1e-3)
    nc.set_index(order)
    for _ in range(3):
        nc.step_eager(16, 4)
    for a, b in zip(replayed, snapshot(nc)):
        assert torch.equal(a, b)                                                 # bit for bit
    assert replayed[3].tolist() == [3, 3] and not torch.equal(replayed[0], torch.ones_like(replayed[0]))
    # a whole epoch: three full steps and the tail of 10 in its own slot
    nc.reset(*ones)
    stats = nc.run_epoch(4, order, 1e-3)
    assert stats[:, 3].tolist() == [16, 16, 16, 10] and nc.cells.cpu().tolist() == [4, 4]
    assert np.isfinite(stats).all() and (stats[:, 0] > 0).all() and (np.diff(stats[:, 2]) < 0).all()   # the mask shrinks
    with pytest.raises(ValueError, match="indices into the dataset"):
        nc.set_index(np.arange(57))
    with pytest.raises(ValueError, match="outside the classifier"):
        nc.step_plan(16, 10)


def test_only_the_supported_classifier_is_taken(m, fixture_net):
    D, nets = m["defenses"], m["nets"]
    data = images(4, 32, 1)
    with pytest.raises(ValueError, match="only combat_amd.nets.PreActResNet18 is supported"):
        D.NeuralCleanse(nets.ResNet18(num_classes=8).cuda().eval(), images(4, 64, 1), nc_opt())
    with pytest.raises(ValueError, match="only combat_amd.nets.PreActResNet18 is supported"):
        D.NeuralCleanse(torch.nn.Linear(2, 2), data, nc_opt())
    fixture_net.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            D.NeuralCleanse(fixture_net, data, nc_opt())
    finally:
        fixture_net.eval()
    with pytest.raises(ValueError, match="uint8"):
        D.NeuralCleanse(fixture_net, data.astype(np.float32), nc_opt())


# ---------------------------------------------------------------- the script


def test_script_end_to_end_on_synthetic_data(m, tmp_path):
    torch.manual_seed(21)
    netC = randomize_bn_buffers(m["nets"].PreActResNet18(), 300)
    folder = tmp_path / "ck" / "t_clean" / "cifar10"
    folder.mkdir(parents=True)
    torch.save({"netC": netC.state_dict()}, str(folder / "cifar10_t_clean.pth.tar"))
    script = os.path.join(ROOT, "defenses", "neural_cleanse", "neural_cleanse.py")
    argv = [sys.executable, script, "--dataset", "cifar10", "--saving_prefix", "t", "--checkpoints", str(tmp_path / "ck"),
            "--result", str(tmp_path / "results"), "--synthetic", "--synthetic_size", "64", "--seed", "5", "--total_label", "2",
            "--epoch", "2", "--bs", "24"]
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    run = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    out = run.stdout
    assert "Test 0:" in out and "----------------- Analyzing label: 1 -----------------" in out and "2 labels found" in out
    assert out.count("  Result: Accuracy: ") == 4                                # 2 labels x 2 epochs
    assert ("Not a backdoor model" in out) != ("This is a backdoor model" in out)
    assert "Flagged label list: " in out
    base = tmp_path / "results" / "t_clean" / "cifar10"
    lines = open(str(base / "cifar10_t_output.txt")).read().split("\n")
    assert lines[0] == "Output for neural cleanse: cifar10 - t" and lines[1] == "-" * 30 and lines[2] == "Test 0:"
    assert len(lines[3].split(", ")) == 3 and lines[5:] == [""]
    norms = [float(v) for v in lines[4].split(", ")]
    assert len(norms) == 2 and all(0 < v < 1024 for v in norms)
    for label in (0, 1):
        mask, pattern = np.load(str(base / str(label) / "mask.npy")), np.load(str(base / str(label) / "pattern.npy"))
        assert mask.shape == (1, 32, 32) and pattern.shape == (3, 32, 32) and mask.dtype == np.float32
        assert 0 <= mask.min() and mask.max() <= 1 and abs(float(np.abs(mask).sum()) - norms[label]) <= 1e-3 * norms[label]
    # a two-process launch is refused before anything is loaded
    refused = subprocess.run(argv, cwd=str(tmp_path), env=dict(env, WORLD_SIZE="2"), capture_output=True, text=True, timeout=240)
    assert refused.returncode != 0 and "Neural Cleanse runs on a single GPU" in refused.stderr
