"""Command-line flags of the STRIP script -- same names, types and defaults as the reference's parser (reference
defenses/STRIP/config.py:4-28), held as data like defenses/fine_pruning/config.py.  The reference's script reads
opt.saving_prefix, opt.num_classes and opt.bs, which its parser never defines: they are in _MISSING; flags of this
implementation are in _EXTRA."""
import argparse

# (flag, kwargs) -- order follows the reference for diff-ability of `--help`
_FLAGS = [
    ("--data_root", dict(type=str, default="../../data/")),
    ("--checkpoints", dict(type=str, default="../../checkpoints")),
    ("--device", dict(type=str, default="cuda")),
    ("--results", dict(type=str, default="./results")),
    ("--dataset", dict(type=str, default="cifar10")),
    ("--attack_mode", dict(type=str, default="all2one")),
    ("--temps", dict(type=str, default="./temps")),
    ("--noise_rate", dict(type=float, default=0.08)),
    ("--ratio", dict(type=float, default=0.65, help="scale ratio for DCT of noise")),
    ("--kernel_size", dict(type=int, default=3, help="kernel size for Gaussian blur")),
    # type=tuple splits a command-line value into characters: only the default is usable (as in the root config.py)
    ("--sigma", dict(type=tuple, default=(0.1, 1.0), help="sigma for Gaussian blur")),
    ("--n_sample", dict(type=int, default=100)),
    ("--n_test", dict(type=int, default=100)),
    ("--detection_boundary", dict(type=float, default=0.2)),   # according to the original paper
    ("--num_workers", dict(type=int, default=2)),
    ("--test_rounds", dict(type=int, default=10)),
]

# read by the reference's script (STRIP.py:123, :136, :150), absent from its parser
_MISSING = [
    ("--saving_prefix", dict(type=str, help="Folder in /checkpoints for saving ckpt")),
    ("--num_classes", dict(type=int, default=10)),
    ("--bs", dict(type=int, default=100, help="overwritten by --n_test, as in the reference (STRIP.py:150)")),
]

_EXTRA = [
    ("--synthetic", dict(action="store_true", help="CIFAR-10-shaped random data instead of --data_root")),
    ("--synthetic_size", dict(type=int, default=0, help="images per synthetic split (0 = dataset size)")),
    ("--seed", dict(type=int, default=None, help="seed torch / numpy / random (the reference never seeds)")),
    ("--full_normalize", dict(action="store_true",
                              help="normalise the whole blended image, not only the three columns the reference reaches")),
]


def get_arguments():
    parser = argparse.ArgumentParser()
    for flag, kw in _FLAGS + _MISSING + _EXTRA:
        parser.add_argument(flag, **kw)
    return parser

