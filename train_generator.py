"""Alternated training of the trigger generator and the surrogate classifier on MI355X.

Drop-in for the reference script of the same name: same flags (config.py), same
``get_model`` / ``train`` / ``eval`` / ``main`` call signatures, same checkpoint path and keys
(reference train_generator.py:80-128, 131-318, 321-465, 468-609) -- the per-batch loop body
(:170-290) runs as ``combat_amd.step.AlternatedStep`` on the HIP kernels.  CIFAR-10 + the default
default classifier of the dataset (PreActResNet18 for cifar10, ResNet18 for celeba and for imagenet10 at 224 x 224,
bs 32) / UNet / "original" detector (imagenet10: none ships, pass --allow_missing_F);
other --model / --dataset values raise.  ``main()`` and ``train()`` are composed from ``combat_amd.run``, the frame
every training script shares; what is this script's own is its tables, ``get_model`` and ``eval``.

Data parallel: ``python -m torch.distributed.run --nproc-per-node N train_generator.py ...`` gives
every rank a disjoint shard of each epoch and averages the gradients over RCCL (combat_amd.dist).
"""
import os

import torch

from combat_amd import api, dist as cdist, run
from combat_amd.data import get_dataloader
from combat_amd.log import progress_bar
from combat_amd.nets import FrequencyModel, UnetGenerator, default_classifier
from combat_amd.step import AlternatedStep, WanetStep, create_targets_bd  # noqa: F401  (re-exported like the reference)

# the progress line's columns and the epoch's "Clean Accuracy" scalars (:264-277, :293-308), as (label, metric key)
PROGRESS = (("Clean Acc", "clean_correct"), ("Bd Acc", "bd_correct"), ("F Acc", "f_correct"),
            ("Clean Model Acc", "clean_model_correct"), ("Clean Model Bd BA", "clean_model_bd_ba"),
            ("Clean Model Bd ASR", "clean_model_bd_asr"))
ACCURACIES = (("Clean", "clean_correct"), ("Bd", "bd_correct"), ("F", "f_correct"), ("CleanModel Acc", "clean_model_correct"),
              ("CleanModel Bd BA", "clean_model_bd_ba"), ("CleanModel Bd ASR", "clean_model_bd_asr"))
SCALARS = ACCURACIES + (("L2 Loss", "loss_l2_sum"), ("Grad L2 Loss", "loss_grad_l2_sum"),
                        ("CleanModel Loss", "clean_model_loss_sum"))
BEST_KEYS = ("best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
             "best_clean_model_bd_asr")


def create_dir(path_dir):
    os.makedirs(path_dir, exist_ok=True)


def get_model(opt):
    if opt.model != "default" or opt.model_clean != "default" or opt.F_model not in ("original", "original_holdout"):
        raise Exception("only the default classifier / UNet / 'original' detector run on the HIP path")
    netC = default_classifier(opt).to(opt.device)
    clean_model = default_classifier(opt).to(opt.device)
    netG = UnetGenerator(opt).to(opt.device)
    netF = FrequencyModel(num_classes=2, n_input=opt.input_channel, input_size=opt.input_height).to(opt.device)
    optimizerC = torch.optim.SGD(netC.parameters(), opt.lr_C, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerC = torch.optim.lr_scheduler.MultiStepLR(optimizerC, opt.schedulerC_milestones, opt.schedulerC_lambda)
    optimizerG = torch.optim.SGD(netG.parameters(), opt.lr_G, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerG = torch.optim.lr_scheduler.MultiStepLR(optimizerG, opt.schedulerG_milestones, opt.schedulerG_lambda)
    return netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model


def train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, tf_writer, epoch, opt):
    step_cls = WanetStep if getattr(netG, "arch", "") == "gridgen" else AlternatedStep
    run.alternated_epoch("train_generator.py", step_cls,
                         (netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model), (train_dl,),
                         PROGRESS, SCALARS, 20, tf_writer, epoch, opt)     # :310-315: the image grid every 20th epoch


def eval(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, test_dl, best_clean_acc, best_bd_acc,
         best_F_acc, best_clean_model_acc, best_clean_model_bd_ba, best_clean_model_bd_asr, tf_writer, epoch, opt):
    print(" Eval:")
    netC.eval()
    cdist.average_bn_buffers(netC)    # data parallel: one model on every rank and in the checkpoint (combat_amd/dist.py)
    netG.eval()
    clean_model.eval()
    c = dict(clean_n=0, bd_n=0, clean=0, bd=0, F=0, cm=0, cm_ba=0, cm_asr=0)
    for batch_idx, (inputs, targets) in enumerate(test_dl):
        with torch.no_grad():
            inputs, targets = inputs.to(opt.device), targets.to(opt.device)
            preds_clean = netC(inputs)
            c["clean_n"] += len(inputs)
            ntrg = (targets != opt.target_label).nonzero()[:, 0]
            inputs_toChange, targets_toChange = inputs[ntrg], targets[ntrg]
            inputs_bd = api.create_backdoor(netG, inputs_toChange, opt)     # random sigma at eval too (:353,:373)
            targets_bd = create_targets_bd(targets_toChange, opt).to(opt.device)
            c["bd_n"] += len(ntrg)
            # the six counters of this batch in ONE device->host read (the reference reads each one separately)
            cnt = [(preds_clean.argmax(1) == targets).sum(), (clean_model(inputs).argmax(1) == targets).sum()]
            if len(ntrg):
                preds_bd = netC(inputs_bd)
                cm_bd = clean_model(inputs_bd).argmax(1)
                cnt += [(preds_bd.argmax(1) == targets_bd).sum(),
                        (api.frequency_logits(netF, inputs_bd, opt).argmax(1) == 1).sum(),
                        (cm_bd == targets_toChange).sum(), (cm_bd == targets_bd).sum()]
            cnt = torch.stack(cnt).cpu().tolist()
            c["clean"] += int(cnt[0])
            c["cm"] += int(cnt[1])
            if len(ntrg):
                c["bd"] += int(cnt[2])
                c["F"] += int(cnt[3])
                c["cm_ba"] += int(cnt[4])
                c["cm_asr"] += int(cnt[5])
        acc_clean = c["clean"] * 100.0 / c["clean_n"]
        bd_n = max(c["bd_n"], 1)
        acc_bd, acc_F = c["bd"] * 100.0 / bd_n, c["F"] * 100.0 / bd_n
        acc_clean_model = c["cm"] * 100.0 / c["clean_n"]
        bd_ba_clean_model, bd_asr_clean_model = c["cm_ba"] * 100.0 / bd_n, c["cm_asr"] * 100.0 / bd_n
        progress_bar(batch_idx, len(test_dl),
                     "Clean Acc: {:.4f} - Best: {:.4f} | Bd Acc: {:.4f} - Best: {:.4f} | F Acc: {:.4f} - Best: {:.4f} | "
                     "Clean Model Acc: {:.4f} - Best: {:.4f} | Clean Model Bd BA: {:.4f} - Best: {:.4f} | "
                     "Clean Model Bd ASR: {:.4f} - Best: {:.4f}".format(
                         acc_clean, best_clean_acc, acc_bd, best_bd_acc, acc_F, best_F_acc, acc_clean_model,
                         best_clean_model_acc, bd_ba_clean_model, best_clean_model_bd_ba, bd_asr_clean_model,
                         best_clean_model_bd_asr))
    if torch.distributed.is_initialized():   # every rank evaluated its shard of the test set
        vals = cdist.all_reduce_counters([c[k] for k in sorted(c)], device=opt.device)
        c = dict(zip(sorted(c), vals))
        bd_n = max(c["bd_n"], 1)
        acc_clean, acc_bd, acc_F = c["clean"] * 100.0 / c["clean_n"], c["bd"] * 100.0 / bd_n, c["F"] * 100.0 / bd_n
        acc_clean_model = c["cm"] * 100.0 / c["clean_n"]
        bd_ba_clean_model, bd_asr_clean_model = c["cm_ba"] * 100.0 / bd_n, c["cm_asr"] * 100.0 / bd_n
    if not epoch % 1:
        tf_writer.add_scalars("Test Accuracy", {
            "Clean": acc_clean, "Bd": acc_bd, "F": acc_F, "Clean Model Acc": acc_clean_model,
            "Clean Model Bd BA": bd_ba_clean_model, "Clean Model Bd ASR": bd_asr_clean_model}, epoch)
    if acc_clean > best_clean_acc or (acc_clean == best_clean_acc and acc_bd > best_bd_acc):
        print(" Saving...")
        best_clean_acc, best_bd_acc, best_F_acc = acc_clean, acc_bd, acc_F
        best_clean_model_acc, best_clean_model_bd_ba = acc_clean_model, bd_ba_clean_model
        best_clean_model_bd_asr = bd_asr_clean_model
        if int(os.environ.get("RANK", 0)) == 0:
            api.sync_momentum_to_optimizer(optimizerC, netC)
            api.sync_momentum_to_optimizer(optimizerG, netG)
            torch.save({
                "netC": netC.state_dict(), "schedulerC": schedulerC.state_dict(), "optimizerC": optimizerC.state_dict(),
                "netG": netG.state_dict(), "schedulerG": schedulerG.state_dict(), "optimizerG": optimizerG.state_dict(),
                "clean_model": clean_model.state_dict(), "best_clean_acc": acc_clean, "best_bd_acc": acc_bd,
                "best_F_acc": acc_F, "best_clean_model_acc": best_clean_model_acc,
                "best_clean_model_bd_ba": best_clean_model_bd_ba, "best_clean_model_bd_asr": best_clean_model_bd_asr,
                "epoch_current": epoch}, opt.ckpt_path)
    return (best_clean_acc, best_bd_acc, best_F_acc, best_clean_model_acc, best_clean_model_bd_ba,
            best_clean_model_bd_asr)


def main(get_model=None, train=None, eval=None, prepare=None, resume_clean_model=True):
    """``get_model`` / ``train`` / ``eval`` default to this module's; train_generator_wanet.py passes its own.
    ``prepare(opt)`` runs on the parsed options before anything reads them; ``resume_clean_model=False`` keeps the
    clean model of --load_checkpoint_clean on --continue_training (train_generator_imperceptible.py:527 and around
    do not load the checkpoint's copy)."""
    get_model = get_model or globals()["get_model"]
    train = train or globals()["train"]
    eval = eval or globals()["eval"]
    opt, rank, world = run.start(run.seed_ranks_apart, prepare)
    train_dl = get_dataloader(opt, True, rank=rank, world=world)
    test_dl = get_dataloader(opt, False, shuffle=False, rank=rank, world=world)
    models = netC, _, _, netG, _, _, netF, clean_model = get_model(opt)
    run.checkpoint_layout(opt, "{}_clean".format(opt.saving_prefix))
    run.load_detector(netF, opt)
    run.load_clean_model(clean_model, opt)
    best, epoch_current, _ = run.resume_or_start(opt, rank, models, BEST_KEYS, restore_clean_model=resume_clean_model)
    run.broadcast(world, netC, netG, clean_model, netF)
    run.epoch_loop(opt, train, eval, models, (train_dl,), (test_dl,), (), best, epoch_current, run.writer(opt, rank))


if __name__ == "__main__":
    main()
