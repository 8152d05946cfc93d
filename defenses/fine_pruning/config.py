"""Command-line flags of the fine-pruning script -- same names, types and defaults as the reference's parser
(reference defenses/fine_pruning/config.py:4-42), held as data like the root config.py; extra flags for this
implementation are grouped at the end."""
import argparse

# (flag, kwargs) -- order follows the reference for diff-ability of `--help`
_FLAGS = [
    ("--data_root", dict(type=str, default="../../data/")),
    ("--checkpoints", dict(type=str, default="../../checkpoints")),
    ("--temps", dict(type=str, default="./temps")),
    ("--device", dict(type=str, default="cuda")),
    ("--saving_prefix", dict(type=str, help="Folder in /checkpoints for saving ckpt")),
    # the reference's default is a dataset its own main() rejects ("Invalid Dataset"): --dataset is effectively required
    ("--dataset", dict(type=str, default="mnist")),
    ("--input_height", dict(type=int, default=None)),
    ("--input_width", dict(type=int, default=None)),
    ("--input_channel", dict(type=int, default=None)),
    ("--num_classes", dict(type=int, default=10)),
    ("--noise_rate", dict(type=float, default=0.08)),
    ("--ratio", dict(type=float, default=0.65, help="scale ratio for DCT of noise")),
    ("--kernel_size", dict(type=int, default=3, help="kernel size for Gaussian blur")),
    # type=tuple splits a command-line value into characters: only the default is usable (as in the root config.py)
    ("--sigma", dict(type=tuple, default=(0.1, 1.0), help="sigma for Gaussian blur")),
    ("--bs", dict(type=int, default=100)),
    ("--num_workers", dict(type=int, default=2)),
    ("--attack_mode", dict(type=str, default="all2one", help="all2one or all2all")),
    ("--target_label", dict(type=int, default=0)),
    ("--outfile", dict(type=str, default="./results.txt")),
    ("--S2", dict(type=int, default=4)),
    ("--scale", dict(type=float, default=1)),
    ("--grid-rescale", dict(type=float, default=1)),
    ("--clamp", dict(action="store_true")),
    ("--nearest", dict(type=float, default=0)),
]

_EXTRA = [
    ("--synthetic", dict(action="store_true", help="CIFAR-10-shaped random data instead of --data_root")),
    ("--synthetic_size", dict(type=int, default=0, help="images per synthetic split (0 = dataset size)")),
    ("--seed", dict(type=int, default=None, help="seed torch / numpy / random (the reference never seeds)")),
]


def get_arguments():
    parser = argparse.ArgumentParser()
    for flag, kw in _FLAGS + _EXTRA:
        parser.add_argument(flag, **kw)
    return parser
