"""The frame the training entry scripts share, as pieces their ``main()`` and ``train()`` compose (host only: nothing
here touches a kernel or the per-batch path, which is ``combat_amd.step``).

A script's ``main()`` reads top to bottom as: ``start`` (options, process, seeds) -> its loaders and ``get_model`` ->
``checkpoint_layout`` -> ``load_detector`` / ``saved_checkpoint`` -> ``resume_or_start`` (generator family) or
``resume_classifier`` -> ``broadcast`` -> ``epoch_loop`` with ``writer``.  What differs between two scripts is passed
in as one argument or stays in the script; its docstring lists it."""
import os
import random
import time

import numpy as np
import torch

import config
from combat_amd import api, dist as cdist
from combat_amd.log import SummaryWriter, image_grid, progress_bar
from combat_amd.nets import configure_dataset


def fix_blur(opt):
    """gauss_smooth = T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) at module level in the reference's input-aware,
    imperceptible and multi-label scripts, whatever the flags say."""
    opt.kernel_size = 3
    opt.sigma = (0.1, 1.0)


# ------------------------------------------------------------------ options and process
def seed_ranks_apart(seed, rank):
    """The generator family: one model initialisation, rank-local poison and augmentation draws."""
    torch.manual_seed(seed)
    np.random.seed(seed + rank)
    random.seed(seed + rank)


def seed_shared_poison(seed, rank):
    """The victim family: ``random`` draws the poisoned index set, which must be the same on every rank (it is also
    broadcast)."""
    torch.manual_seed(seed)
    np.random.seed(seed + rank)
    random.seed(seed)


def start(seed, prepare=None, one_process=None):
    """Parsed options and (rank, world).  ``prepare(opt)`` runs before anything reads the options; ``seed(seed, rank)``
    is the script's seeding policy under --seed; ``one_process`` is the refusal of a script without a data-parallel
    path."""
    opt = config.get_arguments().parse_args()
    configure_dataset(opt)
    if prepare is not None:
        prepare(opt)
    rank, local_rank, world = cdist.init()
    if one_process and world > 1:
        raise SystemExit(one_process)
    if opt.device == "cuda":
        opt.device = "cuda:%d" % local_rank
    if opt.seed is not None:
        seed(opt.seed, rank)
    return opt, rank, world


def checkpoint_layout(opt, mode):
    """<checkpoints>/<mode>/<dataset>/<dataset>_<mode>.pth.tar with log_dir beside it: the generator family saves
    under mode <saving_prefix>_clean (reference train_generator.py:497-499), train_victim.py and
    train_clean_classifier.py under <saving_prefix>."""
    opt.ckpt_folder = os.path.join(opt.checkpoints, mode, opt.dataset)
    opt.ckpt_path = os.path.join(opt.ckpt_folder, "{}_{}.pth.tar".format(opt.dataset, mode))
    opt.log_dir = os.path.join(opt.ckpt_folder, "log_dir")


# ------------------------------------------------------------------ what a run loads
def detector_checkpoint_path(opt):
    """The reference looks under <F_checkpoints>/<dataset>/<F_model>/ (train_generator.py:504-507) while its shipped
    files sit one level up as <dataset>_original_detector.pth.tar: probe both."""
    folder = os.path.join(opt.F_checkpoints, opt.dataset)
    name = "{}_{}_detector.pth.tar".format(opt.dataset, opt.F_model)
    for p in (os.path.join(folder, opt.F_model, name), os.path.join(folder, name)):
        if os.path.exists(p):
            return p
    return os.path.join(folder, opt.F_model, name)


def load_detector(netF, opt):
    opt.F_ckpt_path = detector_checkpoint_path(opt)
    print(f"Loading {opt.F_model} at {opt.F_ckpt_path}")
    if os.path.exists(opt.F_ckpt_path):
        netF.load_state_dict(torch.load(opt.F_ckpt_path, map_location=opt.device, weights_only=True)["netC"])
    elif not opt.allow_missing_F:
        print("Error: {} not found (pass --allow_missing_F to run with an untrained detector)".format(opt.F_ckpt_path))
        exit()
    netF.eval()
    print("Done")


def saved_checkpoint(opt, name):
    """Path of the checkpoint an earlier script saved under --saving_prefix ``name`` (--load_checkpoint_clean: the
    clean model, --load_checkpoint: the generator); exits if it is not there."""
    path = os.path.join(opt.checkpoints, name or "", opt.dataset, "{}_{}.pth.tar".format(opt.dataset, name))
    if not os.path.exists(path):
        print("Error: {} not found".format(path))
        exit()
    return path


def load_clean_model(clean_model, opt):
    path = saved_checkpoint(opt, opt.load_checkpoint_clean)
    clean_model.load_state_dict(torch.load(path, map_location=opt.device, weights_only=True)["netC"])
    clean_model.eval()


def _restore(sd, tag, net, optimizer, scheduler):
    net.load_state_dict(sd["net" + tag])
    optimizer.load_state_dict(sd["optimizer" + tag])
    scheduler.load_state_dict(sd["scheduler" + tag])


def resume_or_start(opt, rank, models, best_keys, restore_clean_model=True, mask_pattern=False):
    """The generator family's --continue_training (a missing checkpoint is an error) or fresh start (the checkpoint
    folder is wiped, as the reference does at train_generator.py:562).  ``models`` is get_model()'s tuple.  Returns
    (best values in the order of ``best_keys``, first epoch, extras), extras being () or the (mask, pattern) pair the
    input-aware and multi-label checkpoints carry (saved, never used)."""
    netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model = models
    if opt.continue_training:
        if not os.path.exists(opt.ckpt_path):
            print("Pretrained model doesnt exist")
            exit()
        print("Continue training!!")
        sd = torch.load(opt.ckpt_path, map_location=opt.device, weights_only=True)
        _restore(sd, "C", netC, optimizerC, schedulerC)
        _restore(sd, "G", netG, optimizerG, schedulerG)
        if restore_clean_model:
            clean_model.load_state_dict(sd["clean_model"])
        api.load_momentum_from_optimizer(optimizerC, netC)
        api.load_momentum_from_optimizer(optimizerG, netG)
        extras = (sd["mask"].to(opt.device), sd["pattern"].to(opt.device)) if mask_pattern else ()
        return [sd[k] for k in best_keys], sd["epoch_current"], extras
    print("Train from scratch!!!")
    extras = ()
    if mask_pattern:
        mask = torch.zeros(opt.input_height, opt.input_width, device=opt.device)
        mask[2:6, 2:6] = 0.1
        extras = (mask, torch.rand(opt.input_channel, opt.input_height, opt.input_width).to(opt.device))
    cdist.fresh_start(opt.ckpt_folder, rank)     # rank 0 wipes, then a barrier
    return [0.0] * len(best_keys), 0, extras


def resume_classifier(opt, rank, netC, optimizerC, schedulerC, best_keys):
    """train_victim*.py and train_clean_classifier.py: --continue_training resumes only if the checkpoint exists, and
    otherwise starts fresh without a word.  Returns (best values, first epoch)."""
    if opt.continue_training and os.path.exists(opt.ckpt_path):
        sd = torch.load(opt.ckpt_path, map_location=opt.device, weights_only=True)
        _restore(sd, "C", netC, optimizerC, schedulerC)
        api.load_momentum_from_optimizer(optimizerC, netC)
        return [sd[k] for k in best_keys], sd["epoch_current"]
    cdist.fresh_start(opt.ckpt_folder, rank)
    return [0.0] * len(best_keys), 0


def broadcast(world, *modules):
    """Identical replicas before the first batch: rank 0's, in the order given."""
    if world > 1:
        for m in modules:
            cdist.broadcast_module(m)


def writer(opt, rank):
    """One writer, one checkpoint file: rank 0's (every rank holds the same replicas)."""
    if rank != 0:
        return cdist.NullWriter()
    os.makedirs(opt.log_dir, exist_ok=True)
    return SummaryWriter(log_dir=opt.log_dir)


# ------------------------------------------------------------------ epochs
def epoch_loop(opt, train, eval, models, train_dls, test_dls, extras, best, epoch_current, tf_writer):
    """The reference's positional signatures: ``train(*models, *train_dls, *extras, tf_writer, epoch, opt)`` and
    ``eval(*models, *test_dls, *extras, *best, tf_writer, epoch, opt)``, which returns the new best values."""
    for dl in train_dls:
        dl.epoch = epoch_current      # a seeded, resumed run continues the sequence of epoch permutations
    for epoch in range(epoch_current, opt.n_iters):
        print("Epoch {}:".format(epoch + 1))
        t0 = time.perf_counter()
        train(*models, *train_dls, *extras, tf_writer, epoch, opt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        best = eval(*models, *test_dls, *extras, *best, tf_writer, epoch, opt)
        best = list(best) if isinstance(best, (tuple, list)) else [best]
        print(" train {:.2f} s, eval + checkpoint {:.2f} s".format(t1 - t0, time.perf_counter() - t1))


def step_of(cls, netC, netG, clean_model, netF, opt):
    """The step object of one run, built on first use and kept on netC.  ``cls`` is looked up by the calling script in
    its own namespace at call time (each script re-exports its step class, as the reference does its loop body)."""
    key = "_step_" + cls.__name__
    st = netC.__dict__.get(key)
    if st is None:
        pg = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
        st = netC.__dict__[key] = cls(netC, netG, clean_model, netF, opt, process_group=pg)
    return st


def rows_like(x2, n):
    """The second loader's batch cut (or wrapped) to n rows: under data parallel a shuffled loader pads its shard
    while the evaluation loader keeps exact shards, so the last batches may differ in size."""
    if x2.shape[0] == n:
        return x2
    reps = (n + x2.shape[0] - 1) // x2.shape[0]
    return torch.cat([x2] * reps)[:n]


def _column(m, key):
    """Counters as a percentage of the epoch's samples, ``*_sum`` losses as their mean per sample."""
    return m[key] / m["samples"] if key.endswith("_sum") else m[key] * 100.0 / m["samples"]


def alternated_epoch(script, step_cls, models, loaders, progress, scalars, grid_every, tf_writer, epoch, opt):
    """One training epoch of the generator family (reference train_generator.py:131-318) as ``step_cls`` on the HIP
    kernels.  ``models``: get_model()'s tuple; ``loaders``: the train loader, then the loaders whose images ride along
    as further positional batches (input-aware: one); ``progress`` / ``scalars``: the (label, metric key) columns of
    the progress line and of the epoch's "Clean Accuracy" scalars, in order; the last batch and its backdoored copy
    are logged as an image grid every ``grid_every`` epochs.  The reference formats device tensors every step (one sync
    each); here the metrics are read every --log_interval batches and on the last."""
    netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model = models
    print(" Train:")
    netC.train()
    netG.train()
    clean_model.eval()
    st = step_of(step_cls, netC, netG, clean_model, netF, opt)
    st.reset_metrics()
    n_batches = len(loaders[0])
    every = max(1, int(getattr(opt, "log_interval", 20)))
    m = None
    for batch_idx, (inputs, targets), *more in zip(range(n_batches), *loaders):
        more = [rows_like(b[0], inputs.shape[0]) for b in more]
        st.run(inputs.to(opt.device, non_blocking=True), targets, *[x.to(opt.device, non_blocking=True) for x in more],
               lr_c=optimizerC.param_groups[0]["lr"], lr_g=optimizerG.param_groups[0]["lr"])
        last = batch_idx == n_batches - 1 or (opt.max_steps and batch_idx + 1 >= opt.max_steps)
        if batch_idx % every == 0 or last:
            m = st.read_metrics()
            progress_bar(batch_idx, n_batches,
                         " | ".join("{}: {:.4f}".format(label, _column(m, key)) for label, key in progress))
        if last:
            break
    if m is None:
        raise SystemExit("%s: the train loader yielded no batch (dataset smaller than one batch?)" % script)
    tf_writer.add_scalars("Clean Accuracy", {name: _column(m, key) for name, key in scalars}, epoch)
    if not epoch % grid_every and not isinstance(tf_writer, cdist.NullWriter):
        tf_writer.add_image("Images", image_grid(st.inputs, st.bd, opt), global_step=epoch)
    schedulerC.step()
    schedulerG.step()
