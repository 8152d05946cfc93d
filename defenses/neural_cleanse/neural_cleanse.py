"""Neural Cleanse model-level defense against a trained COMBAT backdoor (reference defenses/neural_cleanse/neural_cleanse.py
and detecting.py; Wang et al., IEEE S&P 2019): for every label a mask and a pattern are optimised so that the blended test
images are classified as that label, with the mask's L1 norm as small as the attack-success threshold allows; a label
whose mask is an outlier on the small side (median absolute deviation) is a backdoor target.

    cd defenses/neural_cleanse && python neural_cleanse.py --dataset cifar10 --saving_prefix <prefix>

Same flags and defaults (config.get_argument), checkpoint path
({checkpoints}/{saving_prefix}_clean/{dataset}/{dataset}_{saving_prefix}_clean.pth.tar, key netC), result file
({result}/{saving_prefix}_clean/{dataset}/{dataset}_{saving_prefix}_output.txt), per-label folders and console verdict lines
as the reference; n_times_test x total_label optimisations from all-ones mask_tanh / pattern_tanh.

How it differs from the reference, on purpose:
  * The reference builds a RegressionModel, reloads the checkpoint and the test set for every label (detecting.py:143-148)
    and runs every mini-batch through autograd; here the classifier and the uint8 test set are loaded once and a whole
    optimisation step (blend, eval forward, input gradient, mask / pattern gradients, Adam, the mini-batch record) is one
    replayed plan over device cells (combat_amd/defenses.py::NeuralCleanse).  The host uploads a
    permutation before an epoch and reads the statistics rows after it.
  * The pattern is normalised with CIFAR's mean / std although the images are in [-1, 1] (detecting.py:76-78): kept, since
    published numbers come from that arithmetic.
  * Shuffling: one torch.randperm per epoch from torch's global generator, as a shuffling DataLoader draws its order; the
    reference's 8 worker processes do not change the order.
  * Only cifar10 runs, as in the reference (its main() accepts celeba and imagenet10, its RegressionModel then raises
    "Invalid Dataset", detecting.py:43-51): here the same exception is raised before anything is loaded.
  * Besides mask.png, pattern.png and trigger.png the best mask and pattern are always written as mask.npy [1][32][32] and
    pattern.npy [3][32][32] (raw values in [0, 1]); the PNGs need an image writer (torchvision, else PIL) and are left
    out without one.
  * --total_label, which the reference's main() overwrites with 10, is kept if given: the first total_label labels are
    analysed (a quick look at a few labels; the outlier test then sees only those).
  * --synthetic / --synthetic_size / --seed, as in the other defense scripts.
Single GPU only."""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.append(ROOT)

from combat_amd.data import get_dataloader  # noqa: E402
from combat_amd.defenses import NeuralCleanse, nc_verdict, require_single_process, write_nc_result  # noqa: E402
from combat_amd.nets import PreActResNet18  # noqa: E402


def _local_config():
    """This folder's config.py by path: the repository root has a `config` module of its own."""
    spec = importlib.util.spec_from_file_location("neural_cleanse_config", os.path.join(HERE, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


get_argument = _local_config().get_argument


def configure_dataset(opt) -> None:
    """neural_cleanse.py:58-79 and detecting.py:43-51: of the datasets main() names only cifar10 has a classifier."""
    if opt.dataset != "cifar10":
        raise Exception("Invalid Dataset")
    if opt.total_label is None:
        opt.total_label = 10
    if not 1 <= opt.total_label <= 10:
        raise ValueError("--total_label must be in 1..10 for cifar10")
    opt.input_height, opt.input_width, opt.input_channel = 32, 32, 3
    opt.num_classes = 10


def checkpoint_path(opt) -> str:
    return os.path.join(opt.checkpoints, "{}_clean".format(opt.saving_prefix), opt.dataset,
                        "{}_{}_clean.pth.tar".format(opt.dataset, opt.saving_prefix))


def result_folder(opt) -> str:
    return os.path.join(opt.result, "{}_clean".format(opt.saving_prefix), opt.dataset)


def _image_writer():
    """save(array [C][H][W] float, path) with torchvision.utils.save_image(normalize=True)'s arithmetic, or None."""
    try:
        import torchvision

        def save(img, path):
            torchvision.utils.save_image(torch.from_numpy(np.ascontiguousarray(img)), path, normalize=True)
        return save
    except ImportError:
        pass
    try:
        from PIL import Image
    except ImportError:
        return None

    def save(img, path):
        img = np.asarray(img, dtype=np.float32)
        lo, hi = float(img.min()), float(img.max())
        img = np.clip((np.clip(img, lo, hi) - lo) / max(hi - lo, 1e-5), 0.0, 1.0)       # make_grid(normalize=True)
        if img.shape[0] == 1:
            img = np.repeat(img, 3, axis=0)
        Image.fromarray(np.clip(img * 255.0 + 0.5, 0, 255).astype(np.uint8).transpose(1, 2, 0)).save(path)
    return save


def save_result_to_dir(opt, target_label, recorder, writer=None) -> str:
    """Recorder.save_result_to_dir (detecting.py:122-140) plus the two .npy files."""
    folder = os.path.join(result_folder(opt), str(target_label))
    os.makedirs(folder, exist_ok=True)
    mask, pattern = recorder.mask_best, recorder.pattern_best
    np.save(os.path.join(folder, "mask.npy"), mask)
    np.save(os.path.join(folder, "pattern.npy"), pattern)
    if writer is not None:
        writer(mask, os.path.join(folder, "mask.png"))
        writer(pattern, os.path.join(folder, "pattern.png"))
        writer(pattern * mask, os.path.join(folder, "trigger.png"))
    return folder


def main(argv=None):
    opt = get_argument().parse_args(argv)
    require_single_process("Neural Cleanse")
    configure_dataset(opt)
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
        np.random.seed(opt.seed)
        random.seed(opt.seed)

    os.makedirs(result_folder(opt), exist_ok=True)
    output_path = os.path.join(result_folder(opt), "{}_{}_output.txt".format(opt.dataset, opt.saving_prefix))
    if opt.to_file:
        with open(output_path, "w+") as f:
            f.write("Output for neural cleanse: {} - {}".format(opt.dataset, opt.saving_prefix) + "\n")

    netC = PreActResNet18().to(opt.device)
    state_dict = torch.load(checkpoint_path(opt), map_location=opt.device, weights_only=True)
    netC.load_state_dict(state_dict["netC"])
    netC.requires_grad_(False)
    netC.eval()
    test_dl = get_dataloader(opt, False)
    cleanse = NeuralCleanse(netC, test_dl.x, opt)
    writer = _image_writer()

    init_mask = np.ones((1, opt.input_height, opt.input_width)).astype(np.float32)
    init_pattern = np.ones((opt.input_channel, opt.input_height, opt.input_width)).astype(np.float32)

    results = []
    for test in range(opt.n_times_test):
        print("Test {}:".format(test))
        if opt.to_file:
            with open(output_path, "a+") as f:
                f.write("-" * 30 + "\n")
                f.write("Test {}:".format(str(test)) + "\n")
        masks, idx_mapping = [], {}
        for target_label in range(opt.total_label):
            print("----------------- Analyzing label: {} -----------------".format(target_label))
            opt.target_label = target_label
            recorder = cleanse.optimise(target_label, init_mask, init_pattern,
                                        on_best=lambda rec: save_result_to_dir(opt, target_label, rec, writer))
            save_result_to_dir(opt, target_label, recorder, writer)
            masks.append(recorder.mask_best)
            idx_mapping[target_label] = len(masks) - 1
        l1_norm_list = np.array([float(torch.sum(torch.abs(torch.from_numpy(m)))) for m in masks], dtype=np.float32)
        print("{} labels found".format(len(l1_norm_list)))
        print("Norm values: {}".format(l1_norm_list))
        backdoored, text = nc_verdict(l1_norm_list, idx_mapping)
        if opt.to_file:
            write_nc_result(output_path, l1_norm_list)
        print(text, end="")
        results.append((l1_norm_list, backdoored))
    return results


if __name__ == "__main__":
    main()
