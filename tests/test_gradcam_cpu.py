"""CPU-only tests of the Grad-CAM defense: the host restatements of combat_gradcam_seed / combat_gradcam_map
(combat_amd/defenses.py) against torch's bilinear resize and a line-by-line restatement of the reference's numpy code,
the overlay arithmetic, the flag table, the fixture's conditioning, the distances between the fp32 oracle and the
classifier's bf16 dataflow (the constants the GPU tests scale), and the two entry points' place in the C ABI."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gradcam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT_DIR = os.path.join(ROOT, "defenses", "gradcam")

# The distances between Grad-CAM under fp32 autograd and under the classifier's bf16 dataflow (tests/gradcam_ref.py), the
# largest over the fixture's eight images and the taps 5, 3, 4, measured once by test_bf16_distance below;
# tests/test_gradcam_gpu.py allows the engine twice as much.  The same constants stand in that file and in DESIGN.md
# section 11.
E_RAW = 4.2e-2             # measured 4.057e-2 (tap 3; taps 5 / 4: 1.89e-2 / 1.94e-2): pre-ReLU map, relative to its max |.|
E_CAM = 6.8e-2             # measured 6.604e-2 (tap 4; taps 5 / 3: 4.43e-2 / 3.39e-2): the final map, absolute
E_GRAD = 8.0e-2            # measured 7.794e-2 (tap 3; taps 5 / 4: 5.07e-2 / 5.19e-2): the tapped gradient, relative L2
E_ACT = 6.2e-3             # measured 6.078e-3 (tap 5; taps 3 / 4: 5.01e-3 / 5.98e-3): the tapped activations, relative L2


# ---------------------------------------------------------------- resize, map, seed


@pytest.mark.parametrize("f", [4, 8, 16, 32])
def test_resize_equals_torch_bilinear_on_integer_maps(f):
    """The taps' weights are multiples of 1 / 16 and the maps small integers: every product and sum is exact, so the two
    must agree bit for bit whatever order they blend in."""
    from combat_amd import defenses as D
    r = np.random.default_rng(f).integers(-8, 9, (3, f, f)).astype(np.float32)
    got = D.gradcam_resize_reference(r)
    want = F.interpolate(torch.from_numpy(r)[None], size=(32, 32), mode="bilinear", align_corners=False)[0].numpy()
    assert got.dtype == np.float32 and got.shape == (3, 32, 32)
    assert np.array_equal(got, want)
    if f == 32:
        assert np.array_equal(got, r)
    # the border clamp: the corner pixels are the source's corners
    assert got[0, 0, 0] == r[0, 0, 0] and got[0, -1, -1] == r[0, -1, -1] and got[0, 0, -1] == r[0, 0, -1]
    assert D.gradcam_resize_reference(r.astype(np.float64)).dtype == np.float64


def reference_lines(act_nhwc, grad_nhwc):
    """gradcam.py:183-197 for one image, line by line in fp32 (cv2.resize: gradcam_resize_reference)."""
    from combat_amd import defenses as D
    grads_val = np.ascontiguousarray(grad_nhwc.transpose(2, 0, 1))[None].astype(np.float32)
    target = np.ascontiguousarray(act_nhwc.transpose(2, 0, 1)).astype(np.float32)
    weights = np.mean(grads_val, axis=(2, 3))[0, :]
    cam = np.zeros(target.shape[1:], dtype=np.float32)
    for i, w in enumerate(weights):
        cam += w * target[i, :, :]
    raw = cam.copy()
    cam = np.maximum(cam, 0)
    cam = D.gradcam_resize_reference(cam, 32)
    cam = cam - np.min(cam)
    with np.errstate(invalid="ignore"):
        cam = cam / np.max(cam)
    return cam, raw


@pytest.mark.parametrize("f,c", [(8, 256), (16, 128), (4, 512), (32, 64)])
def test_map_reference_equals_the_reference_lines(f, c):
    """fp64 in the kernel's order against the reference's fp32 numpy lines: the distance is the fp32 side's rounding, bounded
    by gradcam_ref.map_bounds from the term counts (C products and additions per pixel, f * f terms per weight)."""
    from combat_amd import defenses as D
    g = np.random.default_rng(100 + f)
    act, grad = g.normal(0, 1, (3, f, f, c)).astype(np.float32), g.normal(0, 1, (3, f, f, c)).astype(np.float32)
    cam, raw, weights = D.gradcam_map_reference(act, grad)
    assert cam.dtype == np.float64 and cam.shape == (3, 32, 32) and raw.shape == (3, f, f) and weights.shape == (3, c)
    b_raw, b_cam = R.map_bounds(act, grad)
    for i in range(3):
        want_cam, want_raw = reference_lines(act[i], grad[i])
        e_raw, e_cam = np.abs(raw[i] - want_raw).max(), np.abs(cam[i] - want_cam).max()
        print("f %d C %d image %d: raw %.3e (allowed %.3e)  cam %.3e (allowed %.3e)" % (f, c, i, e_raw, b_raw[i], e_cam, b_cam[i]))
        assert e_raw <= b_raw[i] and e_cam <= b_cam[i]
        assert np.nanmin(cam[i]) == 0.0 and np.nanmax(cam[i]) == 1.0
    assert np.abs(weights - grad.astype(np.float64).mean(axis=(1, 2))).max() <= 1e-15
    # the fp32 form follows the same order
    cam32, raw32, w32 = D.gradcam_map_reference(act, grad, dtype=np.float32)
    assert cam32.dtype == raw32.dtype == w32.dtype == np.float32
    assert (np.abs(raw32 - raw).max(axis=(1, 2)) <= b_raw).all() and (np.abs(cam32 - cam).max(axis=(1, 2)) <= b_cam).all()


def test_constant_map_is_nan_in_both():
    from combat_amd import defenses as D
    g = np.random.default_rng(1)
    act = np.abs(g.normal(0, 1, (2, 8, 8, 256))).astype(np.float32)
    grad = -np.abs(g.normal(0, 1, (2, 8, 8, 256))).astype(np.float32)      # every weight negative: the map is nowhere positive
    grad[1] = -grad[1]
    cam, raw, _ = D.gradcam_map_reference(act, grad)
    assert (raw[0] < 0).all() and np.isnan(cam[0]).all() and not np.isnan(cam[1]).any()
    want, _ = reference_lines(act[0], grad[0])
    assert np.isnan(want).all()
    flat = np.ones((1, 4, 4, 64), np.float32)                             # positive and constant: 0 / 0 as well
    assert np.isnan(D.gradcam_map_reference(flat, flat)[0]).all() and np.isnan(reference_lines(flat[0], flat[0])[0]).all()


def test_seed_reference_ties_nan_and_index():
    from combat_amd import defenses as D
    nan = np.nan
    logits = np.array([[1, 3, 3, 2], [nan, 1, 2, 0], [nan, nan, nan, nan], [nan, -np.inf, -np.inf, nan], [2, nan, 5, 5],
                       [0, 0, 0, 0]], np.float32)
    W = (np.arange(4 * 16).reshape(4, 16) * 1.001).astype(np.float32)
    chosen, d = D.gradcam_seed_reference(logits, None, W)
    assert chosen.dtype == np.int32 and chosen.tolist() == [1, 2, 0, 1, 2, 0]
    assert chosen[:1].tolist() == [int(np.argmax(logits[0]))]
    assert d.shape == (6, 4, 4, 16) and d.dtype == np.float32
    want = torch.from_numpy(W[chosen] / np.float32(16)).to(torch.bfloat16).float().numpy()
    assert np.array_equal(d, np.broadcast_to(want[:, None, None, :], d.shape))
    chosen2, d2 = D.gradcam_seed_reference(logits, np.array([3, -1, 2, -1, 0, 9]), W)       # >= classes: the argmax, as the kernel
    assert chosen2.tolist() == [3, 2, 2, 1, 0, 0]
    assert np.array_equal(d2[0, 1, 2], want[0] * 0 + torch.from_numpy(W[3] / np.float32(16)).to(torch.bfloat16).float().numpy())


def test_overlay_arithmetic_by_hand():
    """2 x 2: levels uint8(255 * cam) = 0, 63, 127, 255 -> v = 0, 0.2471, 0.4980, 1 -> jet (R, G, B) =
    clip(1.5 - |4v - (3, 2, 1)|, 0, 1): (0, 0, 0.5), (0, 0.4882, 1), (0.4922, 1, 0.5078), (0.5, 0, 0) -> uint8 by rounding."""
    from combat_amd import defenses as D
    cam = np.array([[0.0, 0.25], [0.5, 1.0]], np.float32)
    img = np.zeros((2, 2, 3), np.uint8)
    heat, overlay = D.gradcam_overlay(img, cam)
    assert heat.dtype == overlay.dtype == np.uint8 and heat.shape == overlay.shape == (2, 2, 3)
    assert heat.tolist() == [[[0, 0, 128], [0, 124, 255]], [[126, 255, 130], [128, 0, 0]]]
    assert overlay.tolist() == heat.tolist()                 # a black picture, maximum 255 / 255 = 1: the heat map itself
    img2 = np.full((2, 2, 3), 255, np.uint8)
    _, overlay2 = D.gradcam_overlay(img2, cam)               # heat / 255 + 1, divided by the maximum 2
    want = np.uint8(np.float32(255) * ((heat.astype(np.float32) / np.float32(255) + np.float32(1)) / np.float32(2)))
    assert np.array_equal(overlay2, want) and overlay2[0, 1, 2] == 255 and overlay2[0, 0, 0] == 127
    # a NaN map counts as zero: deep blue everywhere
    heat3, _ = D.gradcam_overlay(img, np.full((2, 2), np.nan, np.float32))
    assert (heat3 == np.array([0, 0, 128], np.uint8)).all()
    jet = D.gradcam_jet(np.array([0.0, 0.125, 0.375, 0.625, 0.875, 1.0]))
    assert jet.tolist() == [[0, 0, 0.5], [0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0], [0.5, 0, 0]]


# ---------------------------------------------------------------- script


def _script_config():
    spec = importlib.util.spec_from_file_location("gradcam_config_t", os.path.join(SCRIPT_DIR, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# (flag, type, default) of the reference's parser, defenses/gradcam/config.py:7-31
REFERENCE_FLAGS = [
    ("--data_root", "str", "../../data/"), ("--checkpoints", "str", "../../checkpoints/"), ("--temps", "str", "./temps"),
    ("--device", "str", "cuda"), ("--saving_prefix", "str", None), ("--load_checkpoint_clean", "str", None),
    ("--results", "str", "./results"), ("--dataset", "str", "cifar10"), ("--input_height", "int", 32),
    ("--input_width", "int", 32), ("--input_channel", "int", 3), ("--num_classes", "int", 10), ("--num_workers", "int", 2),
    ("--bs", "int", 128), ("--noise_rate", "float", 0.08), ("--target_label", "int", 0), ("--ratio", "float", 0.65),
    ("--kernel_size", "int", 3), ("--sigma", "tuple", (0.1, 1.0)), ("--random_rotation", "int", 10), ("--random_crop", "int", 5),
    ("--attack_mode", "str", "all2one"),
]


def test_flag_table_matches_the_reference():
    cfg = _script_config()
    parser = cfg.get_arguments()
    added = {f.lstrip("-") for f, _ in cfg._EXTRA}
    assert added == {"synthetic", "synthetic_size", "seed", "n_images"}
    ours = [(a.option_strings[0], a.type.__name__, a.default) for a in parser._actions
            if a.dest != "help" and a.dest not in added]
    assert ours == REFERENCE_FLAGS
    opt = parser.parse_args([])
    assert opt.n_images == 20 and opt.synthetic is False and opt.synthetic_size == 0 and opt.seed is None


def test_script_paths_and_cifar10_only():
    spec = importlib.util.spec_from_file_location("gradcam_script_t", os.path.join(SCRIPT_DIR, "gradcam.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = mod.get_arguments().parse_args(["--saving_prefix", "p", "--load_checkpoint_clean", "c", "--checkpoints", "/ck"])
    assert mod.checkpoint_path(opt) == "/ck/p_clean/cifar10/cifar10_p_clean.pth.tar"
    assert mod.clean_checkpoint_path(opt) == "/ck/c/cifar10/cifar10_c.pth.tar"
    assert mod.TARGET_BLOCK == 5
    opt.dataset = "celeba"
    with pytest.raises(Exception, match="Invalid Dataset"):
        mod.configure_dataset(opt)


def test_world_size_above_one_is_refused_under_the_defense_name(monkeypatch):
    from combat_amd import defenses
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="^Grad-CAM runs on a single GPU.*world size 2"):
        defenses.require_single_process("Grad-CAM")


def test_gradcam_refuses_other_classifiers_and_blocks():
    """The checks that come before anything touches the device."""
    from combat_amd import defenses as D
    from combat_amd import nets
    with pytest.raises(ValueError, match="only combat_amd.nets.PreActResNet18"):
        D.GradCam(nets.ResNet18().eval())
    with pytest.raises(ValueError, match="eval mode"):
        D.GradCam(nets.PreActResNet18().train())
    with pytest.raises(ValueError, match="32 x 32"):
        D.GradCam(nets.PreActResNet18(input_size=64).eval())
    for bad in (-1, 7, 2.5, True):
        with pytest.raises(ValueError, match="target_block"):
            D.GradCam(nets.PreActResNet18().eval(), bad)


# ---------------------------------------------------------------- oracle, fixture, distances


def test_tapped_forward_is_the_oracle():
    """gradcam_ref.tapped_forward without rounding is oracle/combat_oracle.py's classifier (the same operators; built under
    autograd here, so a few ulp of a logit of magnitude < 1 are allowed), and with rounding bf16_emu's."""
    import bf16_emu as E
    from oracle import combat_oracle as O
    p, _, x = R.fixture()
    with torch.no_grad():
        want = O.preact_resnet18_forward(p, x, False).numpy()
        emu = E.preact_forward_emu(p, x, False).numpy()
        got_emu, kept = R.tapped_forward(p, x, 5, True)
    assert np.abs(R.gradcam(5, False)["logits"] - want).max() <= 1e-5 and np.abs(want).max() < 1
    assert np.array_equal(got_emu.numpy(), emu) and tuple(kept.shape) == (8, 256, 8, 8)


def test_fixture_is_well_enough_conditioned():
    """Random weights on noise images: the top-two margin is 0.011-0.019 (hence `index` is always passed in parity tests)
    and at the 8 x 8 taps only 3-14 % of the pre-ReLU map is positive; what the final map's normalisation divides by must
    not be tiny: for EVERY image and tap the oracle's post-ReLU range is at least 5 % of max |raw| (measured 13-100 %)."""
    for tap in R.TAPS:
        o = R.gradcam(tap, False)
        f, c = {5: (8, 256), 3: (16, 128), 4: (8, 256)}[tap]
        assert o["act"].shape == (R.N_IMAGES, f, f, c) and o["grad"].shape == o["act"].shape
        r = np.maximum(o["raw"], 0).reshape(R.N_IMAGES, -1)
        share = (r.max(axis=1) - r.min(axis=1)) / np.abs(o["raw"]).reshape(R.N_IMAGES, -1).max(axis=1)
        print("tap %d: post-ReLU range / max |raw| %s" % (tap, np.round(share, 3)))
        assert (share >= 0.05).all() and not np.isnan(o["cam"]).any()
        assert np.array_equal(o["chosen"], o["logits"].argmax(1))
    s = np.sort(R.gradcam(5, False)["logits"], axis=1)
    assert (s[:, -1] - s[:, -2]).min() > 1e-3


def test_bf16_distance():
    """E_RAW, E_CAM, E_GRAD, E_ACT: Grad-CAM of the fixture under the classifier's bf16 dataflow against fp32 autograd, the same
    class explained (the oracle's argmax).  Printed, and held against the constants the GPU tests scale."""
    e_raw = e_cam = e_grad = e_act = 0.0
    for tap in R.TAPS:
        a, b = R.gradcam(tap, False), R.gradcam(tap, True)
        assert np.array_equal(a["chosen"], b["chosen"])
        raw, cam, grad = R.raw_distance(b["raw"], a["raw"]), float(np.abs(b["cam"] - a["cam"]).max()), R.rel_l2(b["grad"], a["grad"])
        print("tap %d: E_RAW %.3e  E_CAM %.3e  E_GRAD %.3e  (activations %.3e)" % (tap, raw, cam, grad, R.rel_l2(b["act"], a["act"])))
        e_raw, e_cam, e_grad, e_act = max(e_raw, raw), max(e_cam, cam), max(e_grad, grad), max(e_act, R.rel_l2(b["act"], a["act"]))
    assert e_raw <= E_RAW and e_cam <= E_CAM and e_grad <= E_GRAD and e_act <= E_ACT
    # the constants are the measured ones, not slack
    assert e_raw >= E_RAW / 2 and e_cam >= E_CAM / 2 and e_grad >= E_GRAD / 2 and e_act >= E_ACT / 2


# ---------------------------------------------------------------- C ABI


def test_entry_points_are_exported_with_the_declared_arguments():
    from combat_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "combat_hip.h")).read()
    for name, count in (("combat_gradcam_seed", 10), ("combat_gradcam_map", 10)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == count
        res, args = _lib.SIGNATURES[name]
        assert len(args) == count and getattr(_lib.lib, name).argtypes == args
    assert _lib.lib.combat_abi_version() >= 19
    for name in ("gradcam_seed", "gradcam_map"):
        assert callable(getattr(ops, name))
    from combat_amd import defenses as D
    for name in ("GradCam", "gradcam_map_reference", "gradcam_resize_reference", "gradcam_seed_reference", "gradcam_overlay"):
        assert hasattr(D, name)
