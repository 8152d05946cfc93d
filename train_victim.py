"""Victim training on data poisoned by the frozen generator (reference train_victim.py:93-165 loop,
:168-231 eval, :221-229 checkpoint keys; dataset flags from utils/dataloader_cleanbd.py:131-158)."""
import os

import torch

from combat_amd import api, dist as cdist, run
from combat_amd.data import get_dataloader
from combat_amd.log import image_grid, progress_bar
from combat_amd.nets import UnetGenerator, classifier_for
from combat_amd.step import ClassifierStep, create_targets_bd


def get_model(opt):
    netC = classifier_for(opt).to(opt.device)
    netG = UnetGenerator(opt).to(opt.device)
    optimizerC = torch.optim.SGD(netC.parameters(), opt.lr_C, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerC = torch.optim.lr_scheduler.MultiStepLR(optimizerC, opt.schedulerC_milestones, opt.schedulerC_lambda)
    return netC, optimizerC, schedulerC, netG


def train(netC, optimizerC, schedulerC, netG, train_dl, tf_writer, epoch, opt):
    print(" Train:")
    netC.train()
    step = netC.__dict__.get("_clf_step")
    if step is None:
        pg = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
        step = netC.__dict__["_clf_step"] = ClassifierStep(netC, opt, netG, process_group=pg)
    if step.N:
        step.read_metrics(reset=True)
    total = 0
    pair = None
    for batch_idx, (inputs, targets, poisoned) in enumerate(train_dl):
        step.run(inputs.to(opt.device, non_blocking=True), targets, poisoned, lr=optimizerC.param_groups[0]["lr"])
        total += inputs.shape[0]
        if step.wanet and (not batch_idx % 5 or pair is None):   # train_victim_wanet.py:127-133: every fifth batch with a poisoned
            pair = step.poisoned_pair() or pair                   # image (until one is found: any batch, so that an epoch logs a grid)
        last = batch_idx == len(train_dl) - 1 or (opt.max_steps and batch_idx + 1 >= opt.max_steps)
        if batch_idx % max(1, opt.log_interval) == 0 or last:
            m = step.read_metrics()
            progress_bar(batch_idx, len(train_dl), "CE Loss: {:.4f} | Clean Acc: {:.4f}".format(
                m["loss_sum"] / total, m["correct"] * 100.0 / total))
        if last:
            break
    tf_writer.add_scalars("Clean Accuracy", {"Clean": m["correct"] * 100.0 / total}, epoch)
    if step.wanet and pair is not None and not isinstance(tf_writer, cdist.NullWriter):   # train_victim_wanet.py:136
        tf_writer.add_image("Images", image_grid(pair[0], pair[1], opt), global_step=epoch)
    schedulerC.step()


def eval(netC, optimizerC, schedulerC, netG, test_dl, best_clean_acc, best_bd_acc, tf_writer, epoch, opt):
    print(" Eval:")
    netC.eval()
    cdist.average_bn_buffers(netC)    # data parallel: one model on every rank and in the checkpoint (combat_amd/dist.py)
    n = nb = correct = bd = 0
    for batch_idx, batch in enumerate(test_dl):
        inputs, targets = batch[0].to(opt.device), batch[1].to(opt.device)
        with torch.no_grad():
            correct += int((netC(inputs).argmax(1) == targets).sum())
            n += len(inputs)
            ntrg = (targets != opt.target_label).nonzero()[:, 0]
            if len(ntrg):
                inputs_bd = api.create_backdoor(netG, inputs[ntrg], opt)
                targets_bd = create_targets_bd(targets[ntrg], opt).to(opt.device)
                bd += int((netC(inputs_bd).argmax(1) == targets_bd).sum())
                nb += len(ntrg)
        acc_clean, acc_bd = correct * 100.0 / n, bd * 100.0 / max(nb, 1)
        progress_bar(batch_idx, len(test_dl), "Clean Acc: {:.4f} - Best: {:.4f} | Bd Acc: {:.4f} - Best: {:.4f}".format(
            acc_clean, best_clean_acc, acc_bd, best_bd_acc))
    if torch.distributed.is_initialized():   # every rank evaluated its shard of the test set
        n, nb, correct, bd = cdist.all_reduce_counters([n, nb, correct, bd], device=opt.device)
        acc_clean, acc_bd = correct * 100.0 / n, bd * 100.0 / max(nb, 1)
    tf_writer.add_scalars("Test Accuracy", {"Clean": acc_clean, "Bd": acc_bd}, epoch)
    if acc_clean > best_clean_acc:
        print(" Saving...")
        best_clean_acc, best_bd_acc = acc_clean, acc_bd
        if int(os.environ.get("RANK", 0)) == 0:
            api.sync_momentum_to_optimizer(optimizerC, netC)
            state = {"netC": netC.state_dict(), "schedulerC": schedulerC.state_dict(), "optimizerC": optimizerC.state_dict(),
                     "netG": netG.state_dict(), "best_clean_acc": acc_clean, "best_bd_acc": acc_bd, "epoch_current": epoch}
            if getattr(netG, "arch", "") == "gridgen":          # train_victim_wanet.py:199
                state["grid_rescale"] = opt.grid_rescale
            torch.save(state, opt.ckpt_path)
    return best_clean_acc, best_bd_acc


def load_generator(netG, load_path, opt):
    """The frozen generator of the attack (:262-280).  A checkpoint of the other trigger family is refused by name
    instead of by a state-dict key mismatch deep inside torch."""
    sd = torch.load(load_path, map_location=opt.device, weights_only=True)["netG"]
    is_grid = any(k.startswith("fc1.") for k in sd)
    want_grid = getattr(netG, "arch", "") == "gridgen"
    if is_grid != want_grid:
        raise SystemExit("Error: {} holds a {} generator; use {}".format(
            load_path, "GridGenerator (WaNet)" if is_grid else "UnetGenerator",
            "train_victim_wanet.py" if is_grid else "train_victim.py"))
    netG.load_state_dict(sd)
    netG.eval()
    netG.requires_grad_(False)      # :279-280


def main(get_model=None, wanet=False, eval=None, clean_folder=None):
    """``get_model`` / ``eval`` default to this module's: train_victim_wanet.py passes its own get_model.  clean_folder
    (default: wanet): the checkpoint lives under <saving_prefix>_clean/.  train_victim_inputaware.py, with its second
    test loader and third best value, composes its own main() from the same pieces."""
    get_model = get_model or globals()["get_model"]
    eval = eval or globals()["eval"]
    clean_folder = wanet if clean_folder is None else clean_folder
    opt, rank, world = run.start(run.seed_shared_poison)
    train_dl = get_dataloader(opt, True, poisoned=True, rank=rank, world=world)
    test_dl = get_dataloader(opt, False, shuffle=False, poisoned=True, rank=rank, world=world)
    models = netC, optimizerC, schedulerC, netG = get_model(opt)
    # train_victim.py:255-257 saves under <prefix>/, train_victim_wanet.py:241-243 under <prefix>_clean/
    run.checkpoint_layout(opt, "{}_clean".format(opt.saving_prefix) if clean_folder else opt.saving_prefix)
    load_generator(netG, run.saved_checkpoint(opt, opt.load_checkpoint), opt)
    best, epoch_current = run.resume_classifier(opt, rank, netC, optimizerC, schedulerC, ("best_clean_acc", "best_bd_acc"))
    run.broadcast(world, netC)
    run.epoch_loop(opt, train, eval, models, (train_dl,), (test_dl,), (), best, epoch_current, run.writer(opt, rank))


if __name__ == "__main__":
    main()
