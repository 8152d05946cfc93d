"""Command-line flags of the Neural Cleanse script -- same names, types and defaults as the reference's parser
(reference defenses/neural_cleanse/config.py:4-56), held as data like defenses/STRIP/config.py.  The WaNet flags at the
end of the reference's table are read by nothing in the defense; they stay so that existing command lines parse.  Flags
of this implementation are in _EXTRA."""
import argparse

# (flag, kwargs) -- order follows the reference for diff-ability of `--help`
_FLAGS = [
    ("--checkpoints", dict(type=str, default="../../checkpoints/")),
    ("--data_root", dict(type=str, default="../../data/")),
    ("--device", dict(type=str, default="cuda")),
    ("--result", dict(type=str, default="./results")),
    ("--dataset", dict(type=str, default="cifar10")),
    ("--attack_mode", dict(type=str, default="all2one")),
    ("--temps", dict(type=str, default="./temps")),
    ("--saving_prefix", dict(type=str, help="Folder in /checkpoints for saving ckpt")),
    ("--bs", dict(type=int, default=64)),
    ("--lr", dict(type=float, default=1e-1)),
    ("--input_height", dict(type=int, default=None)),
    ("--input_width", dict(type=int, default=None)),
    ("--input_channel", dict(type=int, default=None)),
    ("--init_cost", dict(type=float, default=1e-3)),
    ("--atk_succ_threshold", dict(type=float, default=99.0)),
    # type=bool makes any non-empty value True ("--early_stop False" included): only the default is usable
    ("--early_stop", dict(type=bool, default=True)),
    ("--early_stop_threshold", dict(type=float, default=99.0)),
    ("--early_stop_patience", dict(type=int, default=25)),
    ("--patience", dict(type=int, default=5)),
    ("--cost_multiplier", dict(type=float, default=2)),
    ("--epoch", dict(type=int, default=50)),
    ("--num_workers", dict(type=int, default=8)),
    ("--target_label", dict(type=int)),
    ("--total_label", dict(type=int)),
    ("--EPSILON", dict(type=float, default=1e-7)),
    ("--to_file", dict(type=bool, default=True)),
    ("--n_times_test", dict(type=int, default=1)),
    # WaNet's flags: unused here, as in the reference
    ("--scale", dict(type=float, default=1)),
    ("--S2", dict(type=int, default=8)),
    ("--grid-rescale", dict(type=float, default=1)),
    ("--clamp", dict(action="store_true")),
    ("--nearest", dict(type=int, default=0)),
    ("--lnoise", dict(type=int, default=8)),
]

_EXTRA = [
    ("--synthetic", dict(action="store_true", help="CIFAR-10-shaped random data instead of --data_root")),
    ("--synthetic_size", dict(type=int, default=0, help="images per synthetic split (0 = dataset size)")),
    ("--seed", dict(type=int, default=None, help="seed torch / numpy / random (the reference never seeds)")),
]


def get_argument():
    parser = argparse.ArgumentParser()
    for flag, kw in _FLAGS + _EXTRA:
        parser.add_argument(flag, **kw)
    return parser
