"""STRIP run-time defense against a trained COMBAT backdoor (reference defenses/STRIP/STRIP.py; Gao et al., ACSAC 2019):
every one of n_test background images is superimposed with n_sample random test images, and the mean entropy of the
classifier's predictions on the blends is its score -- a backdoored background keeps its target prediction under any
overlay, so its entropy is low.  test_rounds rounds; in attack mode ("2" in --attack_mode, as the reference) a round
scores n_test backdoored backgrounds and then n_test clean ones, otherwise only the clean ones.

    cd defenses/STRIP && python STRIP.py --dataset cifar10 --saving_prefix <prefix> [--attack_mode all2one]

Same flags and defaults, checkpoint path ({checkpoints}/{saving_prefix}_clean/{dataset}/{dataset}_{saving_prefix}_clean.pth.tar,
keys netC / netG), result file ({results}/{dataset}/{dataset}_result.txt: the trojan entropies, then the benign ones,
space separated, the first line empty in clean mode) and final console lines as the reference.  Random draws in the
reference's order: per background one np.random.randint(0, len(testset), size=n_sample) from numpy's global generator,
backdoored backgrounds first; the attack batch is the first batch of a shuffled test loader of batch size n_test.

How it differs from the reference, on purpose:
  * The reference's script cannot start: main() calls config.get_arguments() where config.py defines get_argument
    (:198), its parser lacks --saving_prefix, --num_classes and --bs, which the script reads (:123, :136, :150), it
    imports the classifiers from a package whose __init__.py exports none (:9), and networks.models.Denormalizer raises
    for imagenet10.  The parser here keeps every reference flag with its default and
    adds the missing ones; imagenet10 is denormalised with 0.5 / 0.5 like the other two sets (which is what the
    module's own Denormalize, :80-85, does).
  * The reference's Normalize.__call__ (:27-31) runs after ToTensor, on a CHW tensor, and indexes x[:, :, channel]: the
    width axis.  Only columns 0, 1, 2 of every blended image become (v - 0.5) / 0.5; columns 3.. stay in [0, 1].  The
    published entropies come from that arithmetic, so it is the default here; --full_normalize normalises the whole image.
  * The reference builds every blend on the host, one cv2.addWeighted + ToTensor + Normalize per image (:60-75), and
    forwards n_sample images at a time.  Here combat_strip_superimpose writes the classifier's input from the uint8
    images on the device and a group of backgrounds shares one classifier pass (combat_amd/defenses.py, DESIGN.md
    section 9); the arithmetic per image is the reference's, bit for bit up to the classifier's input.
  * The reference reloads the dataset, the checkpoint and the networks in every round (strip(), :119-152); here once.
    Every round still takes the first batch of a newly shuffled loader.
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
from combat_amd.defenses import (Strip, backdoor_backgrounds, require_single_process, strip_draw_index,  # noqa: E402
                                 strip_verdict, write_strip_result)
from combat_amd.log import progress_bar  # noqa: E402
from combat_amd.nets import PreActResNet18, ResNet18, UnetGenerator  # noqa: E402


def _local_config():
    """This folder's config.py by path: the repository root has a `config` module of its own."""
    spec = importlib.util.spec_from_file_location("strip_config", os.path.join(HERE, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


get_arguments = _local_config().get_arguments


def configure_dataset(opt) -> None:
    """STRIP.py:199-216."""
    if opt.dataset == "cifar10":
        opt.input_height, opt.input_width, opt.input_channel = 32, 32, 3
    elif opt.dataset == "celeba":
        opt.input_height, opt.input_width, opt.input_channel = 64, 64, 3
        opt.num_workers = 40
        opt.num_classes = 8
    elif opt.dataset == "imagenet10":
        opt.input_height, opt.input_width, opt.input_channel = 224, 224, 3
        opt.num_classes = 10
    else:
        raise Exception("Invalid Dataset")
    opt.bs = opt.n_test                                                   # :150


def get_model(opt, mode):
    """STRIP.py:122-133."""
    if opt.dataset == "cifar10":
        netC = PreActResNet18(num_classes=opt.num_classes)
    elif opt.dataset == "celeba":
        netC = ResNet18(num_classes=opt.num_classes)
    else:
        netC = ResNet18(num_classes=opt.num_classes, n_input=opt.input_channel, input_size=opt.input_height)
    netG = UnetGenerator(opt).to(opt.device) if mode != "clean" else None
    return netC.to(opt.device), netG


def checkpoint_path(opt) -> str:
    return os.path.join(opt.checkpoints, "{}_clean".format(opt.saving_prefix), opt.dataset,
                        "{}_{}_clean.pth.tar".format(opt.dataset, opt.saving_prefix))


def strip_round(detector: Strip, netG, test_dl, opt, mode):
    """One round (strip(), :157-194): (trojan entropies, benign entropies) as lists of Python floats."""
    n_data = detector.n_data
    trojan = []
    if mode == "attack":
        print("Testing with bd data !!!!")
        inputs, _ = next(iter(test_dl))
        backgrounds = backdoor_backgrounds(netG, inputs.to(opt.device), opt)
        n_bd = backgrounds.shape[0]                                      # n_test, or the whole set if it is smaller
        index = strip_draw_index(n_bd, opt.n_sample, n_data)
        trojan = [float(v) for v in detector.entropies(backgrounds, index).cpu().numpy()]
        progress_bar(n_bd - 1, n_bd)
    else:
        print("Testing with clean data !!!!")
    n_clean = min(opt.n_test, n_data)
    index = strip_draw_index(n_clean, opt.n_sample, n_data)
    benign = [float(v) for v in detector.entropies(detector.data[:n_clean], index).cpu().numpy()]
    if mode != "attack":
        progress_bar(n_clean - 1, n_clean)
    return trojan, benign


def main(argv=None):
    opt = get_arguments().parse_args(argv)
    require_single_process("STRIP")
    configure_dataset(opt)
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
        np.random.seed(opt.seed)
        random.seed(opt.seed)
    mode = "attack" if "2" in opt.attack_mode else "clean"
    print(mode)

    netC, netG = get_model(opt, mode)
    state_dict = torch.load(checkpoint_path(opt), map_location=opt.device, weights_only=True)
    netC.load_state_dict(state_dict["netC"])
    if netG is not None:
        netG.load_state_dict(state_dict["netG"])
        netG.requires_grad_(False)
        netG.eval()
    netC.requires_grad_(False)
    netC.eval()

    test_dl = get_dataloader(opt, False)                                 # shuffled, bs = n_test (:150-151)
    detector = Strip(netC, test_dl.x, opt)

    lists_entropy_trojan, lists_entropy_benign = [], []
    for test_round in range(opt.test_rounds):
        trojan, benign = strip_round(detector, netG, test_dl, opt, mode)
        lists_entropy_trojan += trojan
        lists_entropy_benign += benign

    result_dir = os.path.join(opt.results, opt.dataset)
    os.makedirs(result_dir, exist_ok=True)
    result_path = os.path.join(result_dir, "{}_result.txt".format(opt.dataset))
    write_strip_result(result_path, lists_entropy_trojan, lists_entropy_benign)

    _, _, text = strip_verdict(lists_entropy_trojan, lists_entropy_benign, opt.detection_boundary)
    print(text)
    return lists_entropy_trojan, lists_entropy_benign


if __name__ == "__main__":
    main()
