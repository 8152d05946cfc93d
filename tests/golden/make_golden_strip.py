"""Generate tests/golden/strip.npz and tests/golden/strip_flags.json from the reference's own STRIP class.

Run in the build container only (``python tests/golden/make_golden_strip.py``), like make_golden.py: it imports
``/root/reference`` (read-only), which does not exist on the GPU box.  The files it writes are committed; tests read
only those.

The reference's defenses/STRIP/STRIP.py is imported unchanged, with stub modules for what is absent here:
  * ``cv2``: ``addWeighted(a, alpha, b, beta, gamma)`` as the saturating uint8 add it is for alpha = beta = 1, gamma = 0
    (cv2 computes saturate_cast<uchar>(a * alpha + b * beta + gamma); the stub asserts those weights);
  * ``torchvision`` / ``torchvision.transforms``: ``ToTensor`` (HWC uint8 -> CHW float32, a true division by 255, as
    torchvision's ``img.permute(2, 0, 1).contiguous().to(float32).div(255)``) and ``Compose``; ``GaussianBlur``, ``Resize``
    and the rest are never reached by the three methods recorded here.
  * ``classifier_models``: STRIP.py:9 imports ``PreActResNet18`` and ``ResNet18`` from the package, whose ``__init__.py`` is
    empty; the package's own classes (preact_resnet.py, resnet.py) are set on it under those names.
What is recorded comes from the reference's own ``STRIP._superimpose``, ``STRIP.normalize`` and ``STRIP._get_entropy``
(hence its own ``Normalize.__call__``, ``torch.sigmoid`` and numpy entropy) over a seeded reference ``PreActResNet18``
on the CPU.

Parameters are never stored: the fixture records the seeds, the uint8 images, the index draws, the blended tensors and
the entropies; the tests compare combat_amd.defenses' host restatements with them."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

SEED_NET, SEED_BN, SEED_IMG, SEED_DRAW = 0, 500, 9100, 77
N_DATA, N_BG, N_SAMPLE = 24, 4, 6


def install_stubs():
    cv2 = types.ModuleType("cv2")

    def add_weighted(a, alpha, b, beta, gamma):
        assert (alpha, beta, gamma) == (1, 1, 0) and a.dtype == np.uint8 and b.dtype == np.uint8
        return np.minimum(a.astype(np.uint16) + b.astype(np.uint16), 255).astype(np.uint8)

    cv2.addWeighted = add_weighted
    sys.modules["cv2"] = cv2

    class ToTensor:
        def __call__(self, pic):
            assert isinstance(pic, np.ndarray) and pic.dtype == np.uint8 and pic.ndim == 3
            return torch.from_numpy(pic.transpose((2, 0, 1))).contiguous().to(dtype=torch.float32).div(255)

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):
            for t in self.transforms:
                img = t(img)
            return img

    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Compose = ToTensor, Compose
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr


def import_reference_strip():
    install_stubs()
    # the module's own `import config` / `import dataloader` are its folder's; classifier_models, networks and utils the root's
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "defenses", "STRIP"))
    for name in ("config", "dataloader"):
        sys.modules.pop(name, None)
    # STRIP.py:9 imports the two classifiers from the package, whose __init__.py is empty: hand it the package's own
    # classes under those names (one more reason the reference's script cannot start as it stands)
    import classifier_models
    from classifier_models.preact_resnet import PreActResNet18
    from classifier_models.resnet import ResNet18
    classifier_models.PreActResNet18, classifier_models.ResNet18 = PreActResNet18, ResNet18
    spec = importlib.util.spec_from_file_location("ref_strip", os.path.join(REF, "defenses", "STRIP", "STRIP.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class ListDataset:
    """dataset[i] -> (HWC uint8 image, label), what the reference's get_dataset(...) with ToNumpy() yields."""

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], 0


def covering_images(n, hw, seed):
    """uint8 [n][hw][hw][3] noise whose first two images are ramps: image 0 + image 1 covers every sum 0..510."""
    g = np.random.default_rng(seed)
    x = g.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8)
    k = np.arange(hw * hw * 3, dtype=np.int64).reshape(hw, hw, 3)
    x[0] = (k % 256).astype(np.uint8)                                    # every byte value in each run of 256 bytes ...
    steps = np.array([0, 255] + [(23 * j) % 256 for j in range(2, hw * hw * 3 // 256)])
    x[1] = steps[k // 256].astype(np.uint8)                              # ... over a constant: sums 0..255, 255..510, ...
    return x


def golden_strip(ref):
    sys.path.insert(0, HERE)
    from make_golden import randomize_bn_buffers

    class Opt:
        dataset, input_channel, n_sample, device = "cifar10", 3, N_SAMPLE, "cpu"

    torch.manual_seed(SEED_NET)
    net = randomize_bn_buffers(ref.PreActResNet18(), SEED_BN).eval()
    images = covering_images(N_DATA, 32, SEED_IMG)
    dataset = ListDataset(images)
    detector = ref.STRIP(Opt)
    out = {"seeds": np.array([SEED_NET, SEED_BN, SEED_IMG, SEED_DRAW]), "images": images,
           "n_sample": np.int64(N_SAMPLE), "backgrounds": np.arange(N_BG, dtype=np.int64)}

    # the draws _get_entropy makes (STRIP.py:69), replayed so that the blends can be recorded beside the entropies
    np.random.seed(SEED_DRAW)
    index = np.stack([np.random.randint(0, len(dataset), size=N_SAMPLE) for _ in range(N_BG)])
    blended = np.empty((N_BG, N_SAMPLE, 3, 32, 32), dtype=np.float32)
    for b in range(N_BG):
        for s in range(N_SAMPLE):
            blended[b, s] = detector.normalize(detector._superimpose(images[b], dataset[index[b, s]][0])).numpy()
    np.random.seed(SEED_DRAW)
    with torch.no_grad():
        entropy = np.array([detector(images[b], dataset, net) for b in range(N_BG)], dtype=np.float64)
    # the classifier's outputs on the recorded blends (the same call _get_entropy makes), for the entropy restatement
    with torch.no_grad():
        logits = np.stack([net(torch.from_numpy(blended[b])).numpy() for b in range(N_BG)])
    out.update(index=index.astype(np.int64), blended=blended, entropy=entropy, logits=logits.astype(np.float32))
    assert blended[..., :3].min() < 0 and blended[..., :3].min() >= -1 and blended[..., 3:].min() >= 0, "column quirk not shown"
    path = os.path.join(HERE, "strip.npz")
    np.savez_compressed(path, **out)
    print("entropies", entropy.tolist())
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def golden_flags():
    """Flag names, defaults and types of the reference parser (defenses/STRIP/config.py:4-28)."""
    spec = importlib.util.spec_from_file_location("ref_strip_config", os.path.join(REF, "defenses/STRIP/config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    flags = {}
    for a in mod.get_argument()._actions:
        if a.dest == "help":
            continue
        d = a.default
        flags[a.dest] = {"default": list(d) if isinstance(d, (list, tuple)) else d,
                         "type": getattr(a.type, "__name__", None), "choices": a.choices, "store_true": a.nargs == 0}
    with open(os.path.join(HERE, "strip_flags.json"), "w") as f:
        json.dump(flags, f, indent=1, sort_keys=True)
    print("wrote strip_flags.json (%d flags)" % len(flags))


if __name__ == "__main__":
    torch.set_num_threads(8)
    golden_flags()
    golden_strip(import_reference_strip())
