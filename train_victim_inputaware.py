"""Victim training on data poisoned by the frozen input-aware generator on MI355X.

Drop-in for the reference script of the same name, which is train_victim.py with three changes, and so is this
delegate to train_victim.py:
  * the blur is the module-level T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (reference
    train_victim_inputaware.py:37): --kernel_size / --sigma are ignored;
  * a second, shuffled test loader (:281-283);
  * eval adds the cross-trigger accuracy (:162-236): the noise of the second loader's batch mixed onto the batch,
    counted on the non-target-class rows and divided by their number; the info string gains
    "Cross Acc: ... - Best: ..." and the checkpoint the key best_cross_acc.
The checkpoint lives under ``<saving_prefix>_clean/`` (:289-291).
--dataset cifar10 | celeba | imagenet10 (224 x 224, bs 32), as train_generator_inputaware.py.
"""
import os

import torch

import train_victim as base
from combat_amd import api, dist as cdist, run
from combat_amd.data import get_dataloader
from combat_amd.log import progress_bar
from combat_amd.step import create_targets_bd
from train_generator_inputaware import _rows_like, fix_blur

BEST_KEYS = ("best_clean_acc", "best_bd_acc", "best_cross_acc")


def get_model(opt):
    fix_blur(opt)      # before anything draws a blur
    return base.get_model(opt)


def eval(netC, optimizerC, schedulerC, netG, test_dl, test_dl2, best_clean_acc, best_bd_acc, best_cross_acc, tf_writer, epoch,
         opt):
    print(" Eval:")
    netC.eval()
    cdist.average_bn_buffers(netC)
    n = nb = correct = bd = cross = 0
    for batch_idx, batch, batch2 in zip(range(len(test_dl)), test_dl, test_dl2):
        inputs, targets = batch[0].to(opt.device), batch[1].to(opt.device)
        inputs2 = _rows_like(batch2[0], inputs.shape[0]).to(opt.device)
        with torch.no_grad():
            correct += int((netC(inputs).argmax(1) == targets).sum())
            n += len(inputs)
            ntrg = (targets != opt.target_label).nonzero()[:, 0]
            inputs_bd = api.create_backdoor(netG, inputs[ntrg], opt)
            inputs_cross = api.create_backdoor(netG, inputs, opt, noise_from=inputs2)
            if len(ntrg):
                targets_bd = create_targets_bd(targets[ntrg], opt).to(opt.device)
                bd += int((netC(inputs_bd).argmax(1) == targets_bd).sum())
                cross += int((netC(inputs_cross)[ntrg].argmax(1) == targets[ntrg]).sum())
                nb += len(ntrg)
        acc_clean, acc_bd, acc_cross = correct * 100.0 / n, bd * 100.0 / max(nb, 1), cross * 100.0 / max(nb, 1)
        progress_bar(batch_idx, len(test_dl),
                     "Clean Acc: {:.4f} - Best: {:.4f} | Bd Acc: {:.4f} - Best: {:.4f} | Cross Acc: {:.4f} - Best: {:.4f}"
                     .format(acc_clean, best_clean_acc, acc_bd, best_bd_acc, acc_cross, best_cross_acc))
    if torch.distributed.is_initialized():
        n, nb, correct, bd, cross = cdist.all_reduce_counters([n, nb, correct, bd, cross], device=opt.device)
        acc_clean, acc_bd, acc_cross = correct * 100.0 / n, bd * 100.0 / max(nb, 1), cross * 100.0 / max(nb, 1)
    tf_writer.add_scalars("Test Accuracy", {"Clean": acc_clean, "Bd": acc_bd, "Cross": acc_cross}, epoch)
    if acc_clean > best_clean_acc:
        print(" Saving...")
        best_clean_acc, best_bd_acc, best_cross_acc = acc_clean, acc_bd, acc_cross
        if int(os.environ.get("RANK", 0)) == 0:
            api.sync_momentum_to_optimizer(optimizerC, netC)
            torch.save({"netC": netC.state_dict(), "schedulerC": schedulerC.state_dict(),
                        "optimizerC": optimizerC.state_dict(), "netG": netG.state_dict(), "best_clean_acc": acc_clean,
                        "best_bd_acc": acc_bd, "best_cross_acc": acc_cross, "epoch_current": epoch}, opt.ckpt_path)
    return best_clean_acc, best_bd_acc, best_cross_acc


def main():
    opt, rank, world = run.start(run.seed_shared_poison)
    train_dl = get_dataloader(opt, True, poisoned=True, rank=rank, world=world)
    test_dl = get_dataloader(opt, False, shuffle=False, poisoned=True, rank=rank, world=world)
    test_dl2 = get_dataloader(opt, False, rank=rank, world=world)     # shuffled, as the reference's (:281-283)
    models = netC, optimizerC, schedulerC, netG = get_model(opt)
    run.checkpoint_layout(opt, "{}_clean".format(opt.saving_prefix))      # :289-291
    base.load_generator(netG, run.saved_checkpoint(opt, opt.load_checkpoint), opt)
    best, epoch_current = run.resume_classifier(opt, rank, netC, optimizerC, schedulerC, BEST_KEYS)
    run.broadcast(world, netC)
    run.epoch_loop(opt, base.train, eval, models, (train_dl,), (test_dl, test_dl2), (), best, epoch_current,
                   run.writer(opt, rank))


if __name__ == "__main__":
    main()
