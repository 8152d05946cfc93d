"""Grad-CAM defense on the MI355X: combat_gradcam_seed and combat_gradcam_map against their host restatements (bit for bit
where the arithmetic is exact), their refusals, the engine's tapped forward and partial backward against the plans built
without them, GradCam.maps against torch autograd in fp32 (tests/gradcam_ref.py) for a tap with a convolutional-shortcut
successor and two with an identity successor, and defenses/gradcam/gradcam.py end to end on synthetic data."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradcam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = 0x1234

# Measured on the CPU by tests/test_gradcam_cpu.py::test_bf16_distance (Grad-CAM under fp32 autograd against the same under
# the bf16 emulation of the classifier); the same constants stand there and in DESIGN.md section 11.  The engine is allowed
# twice as much: the emulation models neither the bf16 rounding of the gradient tensors nor the kernels' summation order.
E_RAW = 4.2e-2             # measured 4.057e-2 (tap 3; taps 5 / 4: 1.89e-2 / 1.94e-2): pre-ReLU map, relative to its max |.|
E_CAM = 6.8e-2             # measured 6.604e-2 (tap 4; taps 5 / 3: 4.43e-2 / 3.39e-2): the final map, absolute
E_GRAD = 8.0e-2            # measured 7.794e-2 (tap 3; taps 5 / 4: 5.07e-2 / 5.19e-2): the tapped gradient, relative L2
E_ACT = 6.2e-3             # measured 6.078e-3 (tap 5; taps 3 / 4: 5.01e-3 / 5.98e-3): the tapped activations, relative L2


@pytest.fixture(scope="module")
def m():
    from combat_amd import _lib, defenses, engine, nets, ops
    return dict(lib=_lib.lib, defenses=defenses, engine=engine, nets=nets, ops=ops)


@pytest.fixture(scope="module")
def net():
    return R.make_net().cuda()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- combat_gradcam_seed


def seed_case(classes=10, C=512, N=16, seed=1):
    g = np.random.default_rng(seed)
    logits = g.normal(0, 2, (N, classes)).astype(np.float32)
    logits[1, 4] = logits[1, 7] = logits[1].max() + 1                     # a tie: the first maximal class wins
    logits[2, 0] = np.nan                                                # a NaN never wins against a number
    logits[3, :] = np.nan                                                # a row of NaNs: class 0
    logits[4, 5] = np.nan
    W = g.normal(0, 1, (classes, C)).astype(np.float32)
    return logits, W


@pytest.mark.parametrize("which", ["index", "argmax", "mixed"])
@pytest.mark.parametrize("n,C", [(16, 512), (5, 512), (7, 64)])
def test_seed_equals_the_host_restatement(m, which, n, C):
    D, ops = m["defenses"], m["ops"]
    N, classes = 16, 10
    logits, W = seed_case(classes, C, N)
    index = None
    if which != "argmax":
        index = np.random.default_rng(3).integers(0, classes, N).astype(np.int32)
        if which == "mixed":
            index[::2] = -1
    want_chosen, want_d = D.gradcam_seed_reference(logits[:n], None if index is None else index[:n], W)
    if which == "argmax":
        assert want_chosen[1] == 4 and want_chosen[3] == 0 and want_chosen[2] != 0
    d_feat = torch.full((N + 1, 4, 4, C), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    chosen = torch.full((N + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    ops.gradcam_seed(dev(logits), None if index is None else dev(index), n, dev(W), chosen, d_feat[:N])
    torch.cuda.synchronize()
    got_c, got_d = chosen.cpu().numpy(), d_feat.float().cpu().numpy()
    assert np.array_equal(got_c[:n], want_chosen) and (got_c[n:N] == -1).all() and got_c[N] == SENTINEL
    assert same_bits(got_d[:n], want_d)
    assert (d_feat.view(torch.int16)[n:N] == 0).all()                     # the padding rows: zero gradients
    assert (d_feat.view(torch.int16)[N] == SENTINEL).all()                # beyond the slot: untouched


def test_seed_refusals(m):
    lib, ops = m["lib"], m["ops"]
    N, classes, C = 16, 10, 512
    logits, W = seed_case(classes, C, N)
    dl, dw, di = dev(logits), dev(W), dev(np.zeros(N, np.int32))
    chosen = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
    d_feat = torch.full((N, 4, 4, C), SENTINEL, dtype=torch.int16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(logits=dl.data_ptr(), index=di.data_ptr(), n=4, N=N, classes=classes, C=C, W=dw.data_ptr(), chosen=chosen.data_ptr(),
             d_feat=d_feat.data_ptr()):
        return lib.combat_gradcam_seed(logits, index, n, N, classes, C, W, chosen, d_feat, st)

    assert call(classes=0) == EINVAL and call(classes=17) == EINVAL
    assert call(C=0) == EINVAL and call(C=12) == EINVAL and call(C=-8) == EINVAL
    assert call(n=-1) == EINVAL and call(n=N + 1) == EINVAL and call(N=0, n=0) == EINVAL
    for name in ("logits", "W", "chosen", "d_feat"):
        assert call(**{name: None}) == EINVAL, name
    assert call(logits=dl.data_ptr() + 2) == EINVAL and call(W=dw.data_ptr() + 1) == EINVAL
    assert call(index=di.data_ptr() + 2) == EINVAL and call(chosen=chosen.data_ptr() + 2) == EINVAL
    assert call(d_feat=d_feat.data_ptr() + 8) == EINVAL
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (chosen == SENTINEL).all() and (d_feat == SENTINEL).all()       # nothing was launched
    with pytest.raises(ValueError, match="gradcam_seed"):
        ops.gradcam_seed(dl, di, 4, dw, chosen, d_feat.view(torch.bfloat16)[:8])
    with pytest.raises(ValueError, match="index"):
        ops.gradcam_seed(dl, di.long(), 4, dw, chosen, d_feat.view(torch.bfloat16))


# ---------------------------------------------------------------- combat_gradcam_map

SHAPES = [(8, 256), (16, 128), (4, 512), (32, 64)]


def run_map(m, act, grad, n, with_raw=True, with_weights=True):
    """(cam [n + 1][32][32] with a sentinel image behind, raw, weights) of combat_gradcam_map on float arrays."""
    f, c = act.shape[1], act.shape[3]
    cam = torch.full((n + 1, 32, 32), -7.0, device="cuda")
    raw = torch.full((n, f, f), -7.0, device="cuda") if with_raw else None
    weights = torch.full((n, c), -7.0, device="cuda") if with_weights else None
    m["ops"].gradcam_map(dev(act, torch.bfloat16), dev(grad, torch.bfloat16), n, cam[:n], raw, weights)
    torch.cuda.synchronize()
    return cam.cpu().numpy(), None if raw is None else raw.cpu().numpy(), None if weights is None else weights.cpu().numpy()


def grid_inputs(f, c, n, N, seed):
    """Inputs on a grid coarse enough that every partial sum is exact in fp32 (small integers times a power of two, as
    combat_amd.defenses.sweep_reference's docstring describes): gradients in -2..2 (a weight is a multiple of 1 / (f * f)
    within 2), activations in -4..4 (a pixel's sum: multiples of 2^-10 below 2^12), resize weights multiples of 1 / 16."""
    g = np.random.default_rng(seed)
    act = g.integers(-4, 5, (N, f, f, c)).astype(np.float32)
    grad = g.integers(-2, 3, (N, f, f, c)).astype(np.float32)
    act[n:], grad[n:] = 1e30, 1e30                                        # rows beyond n: never read
    return act, grad


@pytest.mark.parametrize("f,c", SHAPES)
def test_map_equals_the_host_restatement_bit_for_bit(m, f, c):
    D = m["defenses"]
    n, N = 3, 16
    act, grad = grid_inputs(f, c, n, N, 10 * f + 1)
    want_cam, want_raw, want_w = D.gradcam_map_reference(act[:n], grad[:n], dtype=np.float32)
    exact_cam, exact_raw, exact_w = D.gradcam_map_reference(act[:n], grad[:n], dtype=np.float64)
    assert np.array_equal(want_raw, exact_raw) and np.array_equal(want_w, exact_w)       # the grid IS coarse enough
    assert (want_raw > 0).any() and (want_raw < 0).any() and not np.isnan(want_cam).any()
    cam, raw, weights = run_map(m, act, grad, n)
    assert same_bits(weights, want_w)
    assert same_bits(raw, want_raw)
    assert same_bits(cam[:n], want_cam)
    assert np.abs(cam[:n] - exact_cam).max() <= 2.0 ** -23                               # one division's rounding
    assert (cam[n] == -7.0).all()                                                      # memory after cam[n - 1]: untouched
    assert cam[:n].min() == 0.0 and cam[:n].max() == 1.0
    # the optional outputs are optional, and two runs give the same bits
    cam2, raw2, w2 = run_map(m, act, grad, n, with_raw=False, with_weights=False)
    assert raw2 is None and w2 is None and same_bits(cam2, cam)


@pytest.mark.parametrize("f,c", SHAPES + [(4, 64), (32, 128)])
def test_map_on_random_inputs_within_the_rounding_bound(m, f, c):
    """Random bf16 inputs against the fp64 restatement (bf16 products are exact in fp64): the kernel's fp32 sums may be off
    by gradcam_ref.map_bounds, derived from the term counts.  (4, 64): more pixel lanes (32) than pixels (16);
    (32, 128): a map of more than one LDS chunk."""
    D = m["defenses"]
    n = 2
    g = np.random.default_rng(7 * f + c)
    act = torch.from_numpy(g.normal(0, 1, (n, f, f, c)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    grad = torch.from_numpy(g.normal(0, 1, (n, f, f, c)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    want_cam, want_raw, want_w = D.gradcam_map_reference(act, grad)
    b_raw, b_cam = R.map_bounds(act, grad)
    cam, raw, weights = run_map(m, act, grad, n)
    for i in range(n):
        e_raw, e_cam = np.abs(raw[i] - want_raw[i]).max(), np.abs(cam[i] - want_cam[i]).max()
        print("f %d C %d image %d: raw %.3e (allowed %.3e)  cam %.3e (allowed %.3e)" % (f, c, i, e_raw, b_raw[i], e_cam, b_cam[i]))
        assert e_raw <= b_raw[i] and e_cam <= b_cam[i]
    assert np.abs(weights - want_w).max() <= (f * f + 1) * 2.0 ** -24 * np.abs(grad).mean(axis=(1, 2)).max()
    again = run_map(m, act, grad, n)
    assert same_bits(again[0], cam) and same_bits(again[1], raw) and same_bits(again[2], weights)


def test_map_all_negative_is_nan_and_a_corner_maximum(m):
    D = m["defenses"]
    f, c, n = 8, 256, 3
    g = np.random.default_rng(2)
    act = g.integers(1, 5, (n, f, f, c)).astype(np.float32)
    grad = g.integers(1, 3, (n, f, f, c)).astype(np.float32)
    grad[0] = -grad[0]                                                     # image 0: every weight negative, the map nowhere positive
    act[1] = 1.0
    act[1, f - 1, f - 1] = 4.0                                             # image 1: the maximum in the last corner pixel
    act[2] = 1.0
    act[2, 0, 0] = 4.0                                                     # image 2: in the first
    cam, raw, _ = run_map(m, act, grad, n)
    want_cam, want_raw, _ = D.gradcam_map_reference(act, grad, dtype=np.float32)
    assert (raw[0] < 0).all() and np.isnan(cam[0]).all() and np.isnan(want_cam[0]).all()
    assert same_bits(raw, want_raw) and same_bits(cam[1:n], want_cam[1:])
    # the border clamp: beyond the centre of the corner cell the map stays at the corner's value
    assert (cam[1, 30:, 30:] == 1.0).all() and cam[1, 29, 29] < 1.0 and cam[1, 0, 0] == 0.0
    assert (cam[2, :2, :2] == 1.0).all() and cam[2, 2, 2] < 1.0 and cam[2, 31, 31] == 0.0
    assert (cam[n] == -7.0).all()


def test_map_refusals(m):
    lib = m["lib"]
    f, c, n = 8, 256, 2
    act = torch.zeros(n, f, f, c, dtype=torch.bfloat16, device="cuda")
    grad = torch.zeros_like(act)
    cam = torch.full((n, 32, 32), -7.0, device="cuda")
    raw, weights = torch.full((n, f, f), -7.0, device="cuda"), torch.full((n, c), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(act=act.data_ptr(), grad=grad.data_ptr(), n=n, f=f, c=c, out_hw=32, cam=cam.data_ptr(), raw=raw.data_ptr(),
             weights=weights.data_ptr()):
        return lib.combat_gradcam_map(act, grad, n, f, c, out_hw, cam, raw, weights, st)

    for bad in (0, 2, 3, 7, 12, 64):
        assert call(f=bad) == EINVAL
    for bad in (0, 8, 32, 96, 192, 1024):
        assert call(c=bad) == EINVAL
    assert call(out_hw=16) == EINVAL and call(out_hw=64) == EINVAL and call(n=-1) == EINVAL
    for name in ("act", "grad", "cam"):
        assert call(**{name: None}) == EINVAL, name
    assert call(act=act.data_ptr() + 8) == EINVAL and call(grad=grad.data_ptr() + 4) == EINVAL
    assert call(cam=cam.data_ptr() + 2) == EINVAL and call(raw=raw.data_ptr() + 1) == EINVAL
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert (cam == -7.0).all() and (raw == -7.0).all() and (weights == -7.0).all()     # nothing was launched
    with pytest.raises(ValueError, match="gradcam_map"):
        m["ops"].gradcam_map(act, grad[:1], n, cam)
    with pytest.raises(ValueError, match="cam"):
        m["ops"].gradcam_map(act, grad, n, cam[:1])


# ---------------------------------------------------------------- engine

FWD_NAMES = ["stem"] + [name for b in range(8) for name in
                        (("b%d.sc+b%d.c1" % (b, b)) if b in (2, 4, 6) else "b%d.c1" % b, "b%d.c2" % b)] + ["head"]


def names(plan):
    return [call.what for call in plan.calls]


def test_default_plans_are_built_as_before(m, net):
    """The new keywords at their defaults are the old signature: the same plan object under the same key, the same calls;
    the tapped forward adds no launch (a second destination of one convolution) and the partial backward is the full
    one's beginning."""
    eng = net._net_engine()
    eng.refresh()
    slot = eng.slot("gradcam.t.default", 16, 32)
    old = eng.forward_plan(slot, False)
    assert eng.forward_plan(slot, False, keep_raw_blocks=()) is old and list(slot.plans) == ["fwd.eval.1.0.0"]
    assert names(old) == FWD_NAMES
    assert "b5.out" not in slot.bufs and "b3.out" not in slot.bufs and "b4.out" in slot.bufs
    old_b = eng.backward_eval_plan(slot, 1.0)
    assert eng.backward_eval_plan(slot, 1.0, stop_before=None) is old_b and sorted(slot.plans) == ["bwd.eval.1", "fwd.eval.1.0.0"]
    full = names(old_b)
    assert full[0] == "head_bwd" and full[-1] == "stem.dgrad" and full.count("b6.c1.dgrad") == 1
    assert [x for x in full if x.endswith("c2.dgrad")] == ["b%d.c2.dgrad" % b for b in reversed(range(8))]

    other = eng.slot("gradcam.t.tapped", 16, 32)
    tapped = eng.forward_plan(other, False, keep_raw_blocks=(5, 3))
    assert names(tapped) == FWD_NAMES and "b5.out" in other.bufs and "b3.out" in other.bufs
    assert sorted(other.plans) == ["fwd.eval.1.0.0.kr3,5"]
    assert names(eng.forward_plan(other, False)) == FWD_NAMES and len(other.plans) == 2
    part = eng.backward_eval_plan(other, 1.0, head_done=True, stop_before=6)
    assert names(part) == full[1:full.index("b6.c1.dgrad") + 1] and "g.img" not in other.bufs
    assert names(eng.backward_eval_plan(other, 1.0, head_done=True)) == full[1:]
    with pytest.raises(ValueError, match="keep_raw_blocks"):
        eng.forward_plan(other, True, keep_raw_blocks=(5,))
    with pytest.raises(ValueError, match="keep_raw_blocks"):
        eng.forward_plan(other, False, keep_raw_blocks=(8,))
    with pytest.raises(ValueError, match="stop_before"):
        eng.backward_eval_plan(other, 1.0, head_done=True, stop_before=8)
    resnet = m["nets"].ResNet18().cuda().eval()
    with pytest.raises(ValueError, match="keep_raw_blocks"):
        resnet._net_engine().forward_plan(resnet._net_engine().slot("t", 16, 64), False, keep_raw_blocks=(5,))


def test_tapped_forward_gives_the_untapped_logits(m, net):
    eng, ops = net._net_engine(), m["ops"]
    eng.refresh()
    x = R.fixture()[2].cuda()
    logits = []
    for name, keep in (("gradcam.t.plain", ()), ("gradcam.t.kept", (5,)), ("gradcam.t.kept2", (3, 4))):
        slot = eng.slot(name, 16, 32)
        eng.input(slot).zero_()
        ops.image_to_c8(x, eng.input(slot))
        eng.forward_plan(slot, False, keep_raw_blocks=keep).run()
        logits.append(eng.head_bufs(slot)["logits"][:8].cpu().numpy())
    assert same_bits(logits[0], logits[1]) and same_bits(logits[0], logits[2])
    assert np.abs(logits[0] - R.gradcam(5, False)["logits"]).max() < 0.05


# ---------------------------------------------------------------- GradCam.maps


def nhwc(t, n):
    return t[:n].float().cpu().numpy()


@pytest.mark.parametrize("tap", R.TAPS)
def test_maps_against_fp32_autograd(m, net, tap):
    """Block 5 (the reference's tap) and block 3 have a successor with a convolutional shortcut, block 4 an identity one:
    the tapped gradient must be autograd's in both arrangements."""
    D = m["defenses"]
    o = R.gradcam(tap, False)
    x = R.fixture()[2].cuda()
    cam_obj = D.GradCam(net, tap)
    f = o["act"].shape[1]
    raw = torch.zeros(R.N_IMAGES, f, f, device="cuda")
    cam, chosen = cam_obj.maps(x, index=o["chosen"], raw_out=raw)
    assert cam.dtype == torch.float32 and tuple(cam.shape) == (8, 32, 32) and chosen.dtype == torch.int32 and cam.is_cuda
    assert np.array_equal(chosen.cpu().numpy(), o["chosen"])
    act, grad = cam_obj.tapped(R.N_IMAGES)
    assert tuple(act.shape) == (16,) + o["act"].shape[1:] and tuple(grad.shape) == tuple(act.shape)
    e_act, e_grad = R.rel_l2(nhwc(act, 8), o["act"]), R.rel_l2(nhwc(grad, 8), o["grad"])
    e_raw = R.raw_distance(raw.cpu().numpy(), o["raw"])
    got = cam.cpu().numpy()
    e_cam = float(np.abs(got - o["cam"]).max())
    print("tap %d: activations %.3e (allowed %.3e)  gradient %.3e (allowed %.3e)  raw %.3e (allowed %.3e)  cam %.3e (allowed %.3e)"
          % (tap, e_act, 2 * E_ACT, e_grad, 2 * E_GRAD, e_raw, 2 * E_RAW, e_cam, 2 * E_CAM))
    assert not np.isnan(got).any()                                        # no image is left out of the comparison
    assert e_act <= 2 * E_ACT and e_grad <= 2 * E_GRAD
    assert e_raw <= 2 * E_RAW
    assert e_cam <= 2 * E_CAM
    assert got.min() == 0.0 and got.max() == 1.0
    # the map kernel on the engine's own buffers is the host restatement of them
    want_cam, want_raw, _ = D.gradcam_map_reference(nhwc(act, 8), nhwc(grad, 8))
    b_raw, b_cam = R.map_bounds(nhwc(act, 8), nhwc(grad, 8))
    assert (np.abs(raw.cpu().numpy() - want_raw).max(axis=(1, 2)) <= b_raw).all()
    assert (np.abs(got - want_cam).max(axis=(1, 2)) <= b_cam).all()


def test_maps_without_index_explains_the_engines_argmax(m, net):
    D = m["defenses"]
    x = R.fixture()[2].cuda()
    cam_obj = D.GradCam(net)
    assert cam_obj.target_block == 5
    cam, chosen = cam_obj.maps(x)
    eng = net._net_engine()
    logits = eng.head_bufs(eng.slot("gradcam", 16, 32))["logits"][:8].cpu().numpy()
    assert np.array_equal(chosen.cpu().numpy(), logits.argmax(axis=1).astype(np.int32))
    mixed = np.array([-1, 2, -1, 9, 0, -1, -1, 5])
    cam2, chosen2 = cam_obj.maps(x, index=mixed)
    want = np.where(mixed < 0, logits.argmax(axis=1), mixed)
    assert np.array_equal(chosen2.cpu().numpy(), want)
    same = chosen2.cpu().numpy() == chosen.cpu().numpy()
    assert same.any() and not same.all()
    assert same_bits(cam2.cpu().numpy()[same], cam.cpu().numpy()[same])
    cam3, chosen3 = cam_obj.maps(x, index=torch.from_numpy(mixed).cuda())              # a device index: taken as it is
    assert np.array_equal(chosen3.cpu().numpy(), want) and same_bits(cam3.cpu().numpy(), cam2.cpu().numpy())
    for bad in (np.full(8, 10), np.full(8, -2), np.zeros(7, np.int64), np.zeros(8, np.float32)):
        with pytest.raises(ValueError, match="index"):
            cam_obj.maps(x, index=bad)
    with pytest.raises(ValueError, match="inputs"):
        cam_obj.maps(x.cpu())
    with pytest.raises(ValueError, match="inputs"):
        cam_obj.maps(x[:, :, :16])
    empty_cam, empty_chosen = cam_obj.maps(x[:0])
    assert tuple(empty_cam.shape) == (0, 32, 32) and tuple(empty_chosen.shape) == (0,) and empty_chosen.dtype == torch.int32


def test_maps_do_not_depend_on_the_batch(m, net):
    """Eval rows are independent and both batch sizes run in the 16-row slot: the shared images' maps are the same bits."""
    D = m["defenses"]
    x = R.fixture()[2].cuda()
    index = R.gradcam(5, False)["chosen"]
    cam_obj = D.GradCam(net, 5)
    cam8, _ = cam_obj.maps(x, index=index)
    cam8 = cam8.cpu().numpy()
    cam3, chosen3 = cam_obj.maps(x[:3], index=index[:3])
    assert tuple(cam3.shape) == (3, 32, 32) and np.array_equal(chosen3.cpu().numpy(), index[:3])
    assert same_bits(cam3.cpu().numpy(), cam8[:3])


# ---------------------------------------------------------------- the script


def test_script_end_to_end_on_synthetic_data(m, tmp_path):
    nets = m["nets"]
    torch.manual_seed(21)
    netC, netG = R.randomize_bn_buffers(nets.PreActResNet18(), 300), nets.UnetGenerator(None)
    clean = R.randomize_bn_buffers(nets.PreActResNet18(), 400)
    folder = tmp_path / "ck" / "t_clean" / "cifar10"
    folder.mkdir(parents=True)
    torch.save({"netC": netC.state_dict(), "netG": netG.state_dict()}, str(folder / "cifar10_t_clean.pth.tar"))
    folder = tmp_path / "ck" / "c" / "cifar10"
    folder.mkdir(parents=True)
    torch.save({"netC": clean.state_dict()}, str(folder / "cifar10_c.pth.tar"))
    script = os.path.join(ROOT, "defenses", "gradcam", "gradcam.py")
    argv = [sys.executable, script, "--dataset", "cifar10", "--saving_prefix", "t", "--load_checkpoint_clean", "c",
            "--checkpoints", str(tmp_path / "ck"), "--results", str(tmp_path / "results"), "--synthetic", "--synthetic_size", "64",
            "--seed", "5", "--n_images", "4"]
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    run = subprocess.run(argv, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    base = tmp_path / "results" / "cifar10"
    for name in ("cam.npy", "cleancam.npy"):
        cam = np.load(str(base / name))
        assert cam.shape == (4, 32, 32) and cam.dtype == np.float32
        ok = np.isnan(cam) | ((cam >= 0) & (cam <= 1))
        assert ok.all()
        for i in range(4):                                                 # an image's map is NaN as a whole or not at all
            assert np.isnan(cam[i]).all() or (not np.isnan(cam[i]).any() and cam[i].max() == 1.0 and cam[i].min() == 0.0)
    for name in ("chosen.npy", "cleanchosen.npy"):
        chosen = np.load(str(base / name))
        assert chosen.shape == (4,) and chosen.dtype == np.int32 and (chosen >= 0).all() and (chosen < 10).all()
    try:
        from PIL import Image
    except ImportError:                                                    # the script writes PNG files when PIL imports
        Image = None
        assert "no PNG files" in run.stdout
    for family in ("bd", "cam", "cleanbd", "cleancam"):
        for i in range(4 if Image is not None else 0):
            img = Image.open(str(base / ("%s%d.png" % (family, i))))
            assert img.size == (32, 32) and img.mode == "RGB"
    assert not (base / "bd4.png").exists() and not (tmp_path / "heatmap.png").exists()
    # a two-process launch is refused before anything is loaded
    refused = subprocess.run(argv, cwd=str(tmp_path), env=dict(env, WORLD_SIZE="2"), capture_output=True, text=True, timeout=240)
    assert refused.returncode != 0 and "Grad-CAM runs on a single GPU" in refused.stderr
