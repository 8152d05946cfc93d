"""Command-line flags of the Grad-CAM script -- same names, types and defaults as the reference's parser (reference
defenses/gradcam/config.py:4-33), held as data like defenses/STRIP/config.py; flags of this implementation are in
_EXTRA."""
import argparse

# (flag, kwargs) -- order follows the reference for diff-ability of `--help`
_FLAGS = [
    ("--data_root", dict(type=str, default="../../data/")),
    ("--checkpoints", dict(type=str, default="../../checkpoints/")),
    ("--temps", dict(type=str, default="./temps")),
    ("--device", dict(type=str, default="cuda")),
    ("--saving_prefix", dict(type=str, help="Folder in /checkpoints for saving ckpt")),
    ("--load_checkpoint_clean", dict(type=str)),
    ("--results", dict(type=str, default="./results")),
    ("--dataset", dict(type=str, default="cifar10")),
    ("--input_height", dict(type=int, default=32)),
    ("--input_width", dict(type=int, default=32)),
    ("--input_channel", dict(type=int, default=3)),
    ("--num_classes", dict(type=int, default=10)),
    ("--num_workers", dict(type=int, default=2)),
    ("--bs", dict(type=int, default=128)),
    ("--noise_rate", dict(type=float, default=0.08)),
    ("--target_label", dict(type=int, default=0)),
    ("--ratio", dict(type=float, default=0.65, help="scale ratio for DCT of noise")),
    ("--kernel_size", dict(type=int, default=3, help="kernel size for Gaussian blur")),
    # type=tuple splits a command-line value into characters: only the default is usable (as in the root config.py)
    ("--sigma", dict(type=tuple, default=(0.1, 1.0), help="sigma for Gaussian blur")),
    ("--random_rotation", dict(type=int, default=10)),
    ("--random_crop", dict(type=int, default=5)),
    ("--attack_mode", dict(type=str, default="all2one", help="all2one or all2all")),
]

_EXTRA = [
    ("--synthetic", dict(action="store_true", help="CIFAR-10-shaped random data instead of --data_root")),
    ("--synthetic_size", dict(type=int, default=0, help="images per synthetic split (0 = dataset size)")),
    ("--seed", dict(type=int, default=None, help="seed torch / numpy / random (the reference never seeds)")),
    ("--n_images", dict(type=int, default=20, help="images of the first test batch to explain (the reference: 20, fixed)")),
]


def get_arguments():
    parser = argparse.ArgumentParser()
    for flag, kw in _FLAGS + _EXTRA:
        parser.add_argument(flag, **kw)
    return parser
