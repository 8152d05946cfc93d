"""Fine-pruning defense against a trained COMBAT backdoor (reference defenses/fine_pruning/fine-pruning.py): prune the
channels of the classifier's last convolution in ascending order of their mean activation on the test set and report,
for each of the 512 levels, the clean accuracy and the accuracy of the backdoored images against the attack's labels.

    cd defenses/fine_pruning && python fine-pruning.py --dataset cifar10 --saving_prefix <prefix> [--outfile results.txt]

Same flags, checkpoint path ({checkpoints}/{saving_prefix}_clean/{dataset}/{dataset}_{saving_prefix}_clean.pth.tar,
keys netG / netC), console lines and outfile format ("%d %0.4f %0.4f" per level) as the reference.

How it differs from the reference, on purpose:
  * The reference rebuilds and re-evaluates the network 512 times (:166-214).  Here the test set is forwarded once clean
    and once backdoored, and combat_prune_sweep computes every level's predictions from the unpruned network's pooled
    features (combat_amd/defenses.py, DESIGN.md section 8: the pruned logits are a sum over the kept channels).
  * The reference's eval() draws a new blur sigma for every batch of every level (:61, :76), so its 512 levels see 512
    different backdoored test sets.  Here each batch's backdoored images are made once, with one draw, and serve all
    levels: the curve is over one fixed backdoored set.
  * celeba / imagenet10 (ResNet18): the reference's script fails on them -- its BasicBlock never reads `ind`
    (classifier_models/resnet.py:27-33), so `out += self.shortcut(x)` meets a pruned `out` and an unpruned shortcut.
    What that code intends is the same channel mask as PreActResNet's: the block's ReLU follows the sum, so masking the
    block output removes the channel from bn2(conv2) and from the shortcut alike.  That is what runs here, with each
    channel's 4 (64 x 64) or 49 (224 x 224) pooled cells removed from `linear` together (convert(), :40-50).
Single GPU only."""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.append(ROOT)

from combat_amd import api  # noqa: E402
from combat_amd.data import get_dataloader  # noqa: E402
from combat_amd.defenses import FinePruning, require_single_process, write_curve  # noqa: E402
from combat_amd.log import progress_bar  # noqa: E402
from combat_amd.nets import PreActResNet18, ResNet18, UnetGenerator  # noqa: E402
from combat_amd.step import create_targets_bd  # noqa: E402


def _local_config():
    """This folder's config.py by path: the repository root has a `config` module of its own."""
    spec = importlib.util.spec_from_file_location("fine_pruning_config", os.path.join(HERE, "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


get_arguments = _local_config().get_arguments


def configure_dataset(opt) -> None:
    """fine-pruning.py:91-106."""
    if opt.dataset == "cifar10":
        opt.input_height, opt.input_width, opt.input_channel = 32, 32, 3
    elif opt.dataset == "celeba":
        opt.num_classes = 8
        opt.input_height, opt.input_width, opt.input_channel = 64, 64, 3
    elif opt.dataset == "imagenet10":
        opt.num_classes = 10
        opt.input_height, opt.input_width, opt.input_channel = 224, 224, 3
    else:
        raise Exception("Invalid Dataset")


def get_model(opt):
    """fine-pruning.py:109-121."""
    if opt.dataset == "cifar10":
        netC = PreActResNet18()
    elif opt.dataset == "celeba":
        netC = ResNet18(num_classes=opt.num_classes)
    else:
        netC = ResNet18(num_classes=opt.num_classes, n_input=opt.input_channel, input_size=opt.input_height)
    return netC.to(opt.device), UnetGenerator(opt).to(opt.device)


def checkpoint_path(opt) -> str:
    return os.path.join(opt.checkpoints, "{}_clean".format(opt.saving_prefix), opt.dataset,
                        "{}_{}_clean.pth.tar".format(opt.dataset, opt.saving_prefix))


def fine_prune(netC, netG, test_dl, opt) -> FinePruning:
    """Pass 1 (:152-163) and the curve (:166-214) over `test_dl`; returns the filled FinePruning."""
    fp = FinePruning(netC, opt)
    print("Forwarding all the validation dataset:")
    with torch.no_grad():
        for batch_idx, (inputs, _) in enumerate(test_dl):
            fp.observe(inputs.to(opt.device))
            progress_bar(batch_idx, len(test_dl))
        for batch_idx, (inputs, targets) in enumerate(test_dl):
            inputs, targets = inputs.to(opt.device), targets.to(opt.device)
            fp.sweep(api.pooled_features(netC, inputs), targets)
            # every image, target-class ones included (:73-79), one blur draw per batch for all levels
            inputs_bd = api.create_backdoor(netG, inputs, opt)
            targets_bd = create_targets_bd(targets, opt).to(opt.device)
            fp.sweep(api.pooled_features(netC, inputs_bd), targets_bd, targets2=targets, backdoor=True)
            progress_bar(batch_idx, len(test_dl))
    return fp


def main(argv=None):
    opt = get_arguments().parse_args(argv)
    require_single_process()
    configure_dataset(opt)
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
    netC, netG = get_model(opt)
    state_dict = torch.load(checkpoint_path(opt), map_location=opt.device, weights_only=True)
    print("load G")
    netG.load_state_dict(state_dict["netG"])
    netG.eval()
    print("load C")
    netC.load_state_dict(state_dict["netC"])
    netC.eval()
    netC.requires_grad_(False)
    print(state_dict["best_clean_acc"], state_dict["best_bd_acc"])

    test_dl = get_dataloader(opt, False, shuffle=False)
    fp = fine_prune(netC, netG, test_dl, opt)
    acc_clean, acc_bd = fp.curve()
    for index in range(fp.C):
        print("Pruned {} filters".format(index))
        print(" Eval: Acc Clean: {:.3f} | Acc Bd: {:.3f}".format(acc_clean[index], acc_bd[index]))
    write_curve(opt.outfile, acc_clean, acc_bd)
    return fp


if __name__ == "__main__":
    main()
