"""Grad-CAM look at a trained COMBAT backdoor (reference defenses/gradcam/gradcam.py; Selvaraju et al., ICCV 2017): the
class-activation maps of backdoored images under the backdoored classifier next to those of the clean images under a
clean classifier -- the figure with which the paper argues that the trigger does not pull the classifier's attention
away from the object.

    cd defenses/gradcam && python gradcam.py --dataset cifar10 --saving_prefix <prefix> --load_checkpoint_clean <name>

Same flags and defaults (config.get_arguments), checkpoint paths
({checkpoints}/{saving_prefix}_clean/{dataset}/{dataset}_{saving_prefix}_clean.pth.tar, keys netG and netC;
{checkpoints}/{load_checkpoint_clean}/{dataset}/{dataset}_{load_checkpoint_clean}.pth.tar, key netC), tapped layer
(layer3[1]), explained class (each image's highest logit) and output names under {results}/{dataset}/ -- bd{i}.png,
cam{i}.png, cleanbd{i}.png, cleancam{i}.png -- as the reference; only cifar10 runs, as there.

How it differs from the reference, on purpose:
  * It is batched.  The reference explains one image at a time -- a batch-1 forward, a full backward, two host copies, a
    Python loop over 256 channels, cv2.resize -- 20 times per model (:387-429); here each model gets ONE
    combat_amd.defenses.GradCam.maps call over the --n_images images (default 20: the first images of the first test
    batch, as :374): one eval forward that keeps layer3[1]'s output, the seed of the chosen logit, two blocks of input
    gradient and one map kernel.
  * The reference prints tensor shapes at every layer (:144, :375, :389, :396) and writes heatmap.png into the working
    directory at every image (:333): dropped.
  * The reference adds the RGB image to OpenCV's BGR heat map (:325-327), so its cam*.png show the picture with red and
    blue swapped (bd*.png are converted, :330).  Here heat map and picture are both RGB: colours are right.
  * The reference colours with OpenCV's COLORMAP_JET table.  OpenCV is not a dependency here; the piecewise-linear jet
    formula (combat_amd.defenses.gradcam_jet) stands in.  The PNGs are therefore not pixel-equal to the reference's, and
    the closeness of the two colour maps is unverified.
  * cv2.resize (:195) is restated from its documented INTER_LINEAR geometry (include/combat_hip.h, combat_gradcam_map);
    likewise unverified against OpenCV itself.
  * cam.npy and cleancam.npy (float32 [n][32][32]; a constant map is NaN, as the reference's division gives) and
    chosen.npy / cleanchosen.npy (the explained classes) are always written; the PNGs need PIL and are left out without it.
  * --synthetic / --synthetic_size / --seed as in the other defense scripts, --n_images.
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

from combat_amd import api  # noqa: E402
from combat_amd.data import get_dataloader  # noqa: E402
from combat_amd.defenses import GradCam, gradcam_overlay, require_single_process  # noqa: E402
from combat_amd.nets import PreActResNet18, UnetGenerator  # noqa: E402

TARGET_BLOCK = 5         # layer3[1] (gradcam.py:377): the sixth pre-activation block


def _local_config():
    """This folder's config.py by path: the repository root has a `config` module of its own."""
    spec = importlib.util.spec_from_file_location("gradcam_config", os.path.join(HERE, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


get_arguments = _local_config().get_arguments


def configure_dataset(opt) -> None:
    """gradcam.py:354-359."""
    if opt.dataset != "cifar10":
        raise Exception("Invalid Dataset")
    opt.input_height, opt.input_width, opt.input_channel = 32, 32, 3
    if opt.n_images < 0:
        raise ValueError("--n_images must not be negative")


def checkpoint_path(opt) -> str:
    """get_model, :284-289."""
    return os.path.join(opt.checkpoints, "{}_clean".format(opt.saving_prefix), opt.dataset,
                        "{}_{}_clean.pth.tar".format(opt.dataset, opt.saving_prefix))


def clean_checkpoint_path(opt) -> str:
    """get_clean_model, :310-315."""
    return os.path.join(opt.checkpoints, opt.load_checkpoint_clean, opt.dataset,
                        "{}_{}.pth.tar".format(opt.dataset, opt.load_checkpoint_clean))


def get_model(opt):
    """(netC, netG) of the backdoored checkpoint, :274-301."""
    netC, netG = PreActResNet18().to(opt.device), UnetGenerator(opt).to(opt.device)
    state_dict = torch.load(checkpoint_path(opt), map_location=opt.device, weights_only=True)
    netG.load_state_dict(state_dict["netG"])
    netC.load_state_dict(state_dict["netC"])
    netG.requires_grad_(False)
    netC.requires_grad_(False)
    return netC.eval(), netG.eval()


def get_clean_model(opt):
    """:304-321."""
    classifier = PreActResNet18().to(opt.device)
    state_dict = torch.load(clean_checkpoint_path(opt), map_location=opt.device, weights_only=True)
    classifier.load_state_dict(state_dict["netC"])
    classifier.requires_grad_(False)
    return classifier.eval()


def images_u8(inputs: torch.Tensor) -> np.ndarray:
    """uint8 [n][hw][hw][3] of a batch in [-1, 1]: the denormalizer, * 255 and np.uint8's truncation (:390-397, :331)."""
    img = (inputs * 0.5 + 0.5) * 255.0
    return torch.clamp(img, 0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def save_figures(result_dir: str, images: np.ndarray, cams: np.ndarray, prefix: str = "") -> int:
    """show_cam_on_image's two files per image (:331-332); returns the number of PNG pairs written (0 without PIL)."""
    try:
        from PIL import Image
    except ImportError:
        return 0
    for i, (img, cam) in enumerate(zip(images, cams)):
        _, overlay = gradcam_overlay(img, cam)
        Image.fromarray(img).save(os.path.join(result_dir, prefix + "bd{}.png".format(i)))
        Image.fromarray(overlay).save(os.path.join(result_dir, prefix + "cam{}.png".format(i)))
    return len(images)


def main(argv=None):
    opt = get_arguments().parse_args(argv)
    require_single_process("Grad-CAM")
    configure_dataset(opt)
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
        np.random.seed(opt.seed)
        random.seed(opt.seed)

    model, generator = get_model(opt)
    model_clean = get_clean_model(opt)

    inputs, _ = next(iter(get_dataloader(opt, False)))
    inputs = inputs[:opt.n_images].to(opt.device)
    inputs_bd = api.create_backdoor(generator, inputs, opt)

    cam, chosen = GradCam(model, TARGET_BLOCK).maps(inputs_bd)
    cam_clean, chosen_clean = GradCam(model_clean, TARGET_BLOCK).maps(inputs)

    result_dir = os.path.join(opt.results, opt.dataset)
    os.makedirs(result_dir, exist_ok=True)
    cam, cam_clean = cam.cpu().numpy(), cam_clean.cpu().numpy()
    np.save(os.path.join(result_dir, "cam.npy"), cam)
    np.save(os.path.join(result_dir, "cleancam.npy"), cam_clean)
    np.save(os.path.join(result_dir, "chosen.npy"), chosen.cpu().numpy())
    np.save(os.path.join(result_dir, "cleanchosen.npy"), chosen_clean.cpu().numpy())
    written = save_figures(result_dir, images_u8(inputs_bd), cam)
    save_figures(result_dir, images_u8(inputs), cam_clean, prefix="clean")
    print("{} images: maps in {} ({})".format(len(cam), result_dir,
                                              "PNG files written" if written or not len(cam) else "no PNG files: PIL is missing"))
    return cam, cam_clean


if __name__ == "__main__":
    main()
