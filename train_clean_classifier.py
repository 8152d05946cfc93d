"""Plain supervised training of the classifier that `train_generator.py` later loads as `clean_model`
(reference train_clean_classifier.py:75-121 loop, :153-160 checkpoint keys, :191-193 path
<checkpoints>/<saving_prefix>/<dataset>/<dataset>_<saving_prefix>.pth.tar)."""
import os

import torch

from combat_amd import api, dist as cdist, run
from combat_amd.data import get_dataloader
from combat_amd.log import progress_bar
from combat_amd.nets import classifier_for
from combat_amd.step import ClassifierStep


def get_model(opt):
    netC = classifier_for(opt).to(opt.device)
    optimizerC = torch.optim.SGD(netC.parameters(), opt.lr_clean, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerC = torch.optim.lr_scheduler.MultiStepLR(optimizerC, opt.scheduler_clean_milestones, opt.scheduler_clean_lambda)
    return netC, optimizerC, schedulerC


def train(netC, optimizerC, schedulerC, train_dl, tf_writer, epoch, opt, step=None):
    print(" Train:")
    netC.train()
    step = step or netC.__dict__.get("_clf_step")
    if step is None:
        pg = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
        step = netC.__dict__["_clf_step"] = ClassifierStep(netC, opt, process_group=pg)
    step.read_metrics(reset=True) if step.N else None
    total = 0
    for batch_idx, (inputs, targets) in enumerate(train_dl):
        step.run(inputs.to(opt.device, non_blocking=True), targets, lr=optimizerC.param_groups[0]["lr"])
        total += inputs.shape[0]
        last = batch_idx == len(train_dl) - 1 or (opt.max_steps and batch_idx + 1 >= opt.max_steps)
        if batch_idx % max(1, opt.log_interval) == 0 or last:
            m = step.read_metrics()
            progress_bar(batch_idx, len(train_dl), "CE Loss: {:.4f} | Clean Acc: {:.4f}".format(
                m["loss_sum"] / total, m["correct"] * 100.0 / total))
        if last:
            break
    tf_writer.add_scalars("Clean Accuracy", {"Clean": m["correct"] * 100.0 / total}, epoch)
    schedulerC.step()


def eval(netC, optimizerC, schedulerC, test_dl, best_clean_acc, tf_writer, epoch, opt):
    print(" Eval:")
    netC.eval()
    cdist.average_bn_buffers(netC)    # data parallel: one model on every rank and in the checkpoint (combat_amd/dist.py)
    n = correct = 0
    for batch_idx, (inputs, targets) in enumerate(test_dl):
        with torch.no_grad():
            preds = netC(inputs.to(opt.device))
        n += len(inputs)
        correct += int((preds.argmax(1).cpu() == targets).sum())
        progress_bar(batch_idx, len(test_dl), "Clean Acc: {:.4f} - Best: {:.4f}".format(correct * 100.0 / n, best_clean_acc))
    if torch.distributed.is_initialized():   # every rank evaluated its shard of the test set
        n, correct = cdist.all_reduce_counters([n, correct], device=opt.device)
    acc = correct * 100.0 / n
    tf_writer.add_scalars("Test Accuracy", {"Clean": acc}, epoch)
    if acc > best_clean_acc:
        print(" Saving...")
        best_clean_acc = acc
        if int(os.environ.get("RANK", 0)) == 0:
            api.sync_momentum_to_optimizer(optimizerC, netC)
            torch.save({"netC": netC.state_dict(), "schedulerC": schedulerC.state_dict(),
                        "optimizerC": optimizerC.state_dict(), "best_clean_acc": acc, "epoch_current": epoch}, opt.ckpt_path)
    return best_clean_acc


def main():
    opt, rank, world = run.start(lambda seed, rank: torch.manual_seed(seed))     # torch only, as before any data parallelism
    train_dl = get_dataloader(opt, True, rank=rank, world=world)
    test_dl = get_dataloader(opt, False, shuffle=False, rank=rank, world=world)
    models = netC, optimizerC, schedulerC = get_model(opt)
    run.checkpoint_layout(opt, opt.saving_prefix)
    best, epoch_current = run.resume_classifier(opt, rank, netC, optimizerC, schedulerC, ("best_clean_acc",))
    run.broadcast(world, netC)
    run.epoch_loop(opt, train, eval, models, (train_dl,), (test_dl,), (), best, epoch_current, run.writer(opt, rank))


if __name__ == "__main__":
    main()
