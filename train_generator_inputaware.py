"""Alternated training with the input-aware (cross-trigger) objective on MI355X.

Drop-in for the reference script of the same name (reference train_generator_inputaware.py:81-138 get_model,
:141-336 train, :339-508 eval, :511-686 main): the networks, trigger, augmentation and detector are
train_generator.py's.  What differs, and is added here:
  * a second, independently shuffled train loader and a second (shuffled) test loader (:535-538); the generator
    also runs on their batches and that noise is mixed onto the FIRST batch's images ("cross" images, which the
    surrogate must keep on their clean label: loss weight --cross_weight);
  * optimizerG is SGD at lr_C * 0.1 and schedulerG steps on the C milestones (:120-127);
  * the blur is the module-level T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (:53): --kernel_size / --sigma are
    ignored, as they are there;
  * "Cross Acc" in the progress line, tensorboard ("Cross") and eval (counted on the non-target-class rows,
    divided by the number of those rows, :405-414);
  * the checkpoint adds best_cross_acc and the (unused) mask / pattern tensors (:480-498), restored on
    --continue_training (:597-618).
The per-batch body (:170-290) runs as ``combat_amd.step.InputAwareStep`` on the HIP kernels.

--dataset cifar10 | celeba | imagenet10 (reference :100-103, :523-528).  imagenet10: 224 x 224, 10 classes,
ResNet18(input_size=224), bs forced to 32 (the generator and netC's differentiated pass run over 64 images); the paired
trigger runs as 16-row strips; no detector checkpoint ships, so pass --allow_missing_F, as for
train_generator.py.

Data parallel: ``python -m torch.distributed.run --nproc-per-node N ...`` shards BOTH train loaders like the first
(combat_amd.dist).  Run with two ranks on one GPU over gloo (COMBAT_DIST_BACKEND=gloo: tests/test_inputaware_gpu.py);
not run over RCCL on several GPUs.
"""
import os

import torch

import train_generator as base
from combat_amd import api, dist as cdist, run
from combat_amd.data import get_dataloader
from combat_amd.log import progress_bar
from combat_amd.step import InputAwareStep, create_targets_bd  # noqa: F401  (re-exported like the reference)

create_dir = base.create_dir
fix_blur = run.fix_blur
_rows_like = run.rows_like
SECOND_LOADER_SEED = 104729    # offset of the second train loader's permutation seed when --seed is given
PROGRESS = base.PROGRESS[:3] + (("Cross Acc", "cross_correct"),) + base.PROGRESS[3:]       # :293-304
SCALARS = (base.ACCURACIES[:2] + (("Cross", "cross_correct"),) + base.ACCURACIES[2:]       # :310-326
           + (("L2 Loss", "loss_l2_sum"), ("CleanModel Loss", "clean_model_loss_sum")))
BEST_KEYS = base.BEST_KEYS[:2] + ("best_cross_acc",) + base.BEST_KEYS[2:]


def get_model(opt):
    netC, optimizerC, schedulerC, netG, _, _, netF, clean_model = base.get_model(opt)
    optimizerG = torch.optim.SGD(netG.parameters(), opt.lr_C * 0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerG = torch.optim.lr_scheduler.MultiStepLR(optimizerG, opt.schedulerC_milestones, opt.schedulerC_lambda)
    return netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model


def train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, train_dl2, mask,
          pattern, tf_writer, epoch, opt):
    run.alternated_epoch("train_generator_inputaware.py", InputAwareStep,
                         (netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model),
                         (train_dl, train_dl2), PROGRESS, SCALARS, 1, tf_writer, epoch, opt)     # :310-331: the grid every epoch


def eval(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, test_dl, test_dl2, mask, pattern,
         best_clean_acc, best_bd_acc, best_cross_acc, best_F_acc, best_clean_model_acc, best_clean_model_bd_ba,
         best_clean_model_bd_asr, tf_writer, epoch, opt):
    print(" Eval:")
    netC.eval()
    cdist.average_bn_buffers(netC)
    netG.eval()
    clean_model.eval()
    c = dict(clean_n=0, bd_n=0, clean=0, bd=0, cross=0, F=0, cm=0, cm_ba=0, cm_asr=0)
    n_batches = len(test_dl)
    for batch_idx, (inputs, targets), (inputs2, _) in zip(range(n_batches), test_dl, test_dl2):
        with torch.no_grad():
            inputs, targets = inputs.to(opt.device), targets.to(opt.device)
            inputs2 = _rows_like(inputs2, inputs.shape[0]).to(opt.device)
            preds_clean = netC(inputs)
            c["clean_n"] += len(inputs)
            ntrg = (targets != opt.target_label).nonzero()[:, 0]
            inputs_toChange, targets_toChange = inputs[ntrg], targets[ntrg]
            inputs_bd = api.create_backdoor(netG, inputs_toChange, opt)                 # :395-397
            targets_bd = create_targets_bd(targets_toChange, opt).to(opt.device)
            c["bd_n"] += len(ntrg)
            inputs_cross = api.create_backdoor(netG, inputs, opt, noise_from=inputs2)    # :405-407: the WHOLE batch
            cnt = [(preds_clean.argmax(1) == targets).sum(), (clean_model(inputs).argmax(1) == targets).sum()]
            if len(ntrg):
                preds_bd = netC(inputs_bd)
                cm_bd = clean_model(inputs_bd).argmax(1)
                preds_cross = netC(inputs_cross)
                cnt += [(preds_bd.argmax(1) == targets_bd).sum(),
                        (api.frequency_logits(netF, inputs_bd, opt).argmax(1) == 1).sum(),
                        (cm_bd == targets_toChange).sum(), (cm_bd == targets_bd).sum(),
                        (preds_cross[ntrg].argmax(1) == targets[ntrg]).sum()]         # :410-414: non-target rows only
            cnt = torch.stack(cnt).cpu().tolist()
            c["clean"] += int(cnt[0])
            c["cm"] += int(cnt[1])
            if len(ntrg):
                c["bd"] += int(cnt[2])
                c["F"] += int(cnt[3])
                c["cm_ba"] += int(cnt[4])
                c["cm_asr"] += int(cnt[5])
                c["cross"] += int(cnt[6])
        acc = _accuracies(c)
        progress_bar(batch_idx, n_batches,
                     "Clean Acc: {:.4f} - Best: {:.4f} | Bd Acc: {:.4f} - Best: {:.4f} | Cross Acc: {:.4f} - Best: {:.4f} | "
                     "F Acc: {:.4f} - Best: {:.4f} | Clean Model BA: {:.4f} - Best: {:.4f} | Clean Model Bd BA: {:.4f} - "
                     "Best: {:.4f} | Clean Model Bd ASR: {:.4f} - Best: {:.4f}".format(
                         acc["clean"], best_clean_acc, acc["bd"], best_bd_acc, acc["cross"], best_cross_acc, acc["F"],
                         best_F_acc, acc["cm"], best_clean_model_acc, acc["cm_ba"], best_clean_model_bd_ba,
                         acc["cm_asr"], best_clean_model_bd_asr))
    if torch.distributed.is_initialized():
        vals = cdist.all_reduce_counters([c[k] for k in sorted(c)], device=opt.device)
        c = dict(zip(sorted(c), vals))
        acc = _accuracies(c)
    if not epoch % 1:
        tf_writer.add_scalars("Test Accuracy", {
            "Clean": acc["clean"], "Bd": acc["bd"], "Cross": acc["cross"], "F": acc["F"], "Clean Model Acc": acc["cm"],
            "Clean Model Bd BA": acc["cm_ba"], "Clean Model Bd ASR": acc["cm_asr"]}, epoch)
    if acc["clean"] > best_clean_acc:     # :471 (no tie-break, unlike train_generator.py)
        print(" Saving...")
        best_clean_acc, best_bd_acc, best_cross_acc, best_F_acc = acc["clean"], acc["bd"], acc["cross"], acc["F"]
        best_clean_model_acc, best_clean_model_bd_ba, best_clean_model_bd_asr = acc["cm"], acc["cm_ba"], acc["cm_asr"]
        if int(os.environ.get("RANK", 0)) == 0:
            api.sync_momentum_to_optimizer(optimizerC, netC)
            api.sync_momentum_to_optimizer(optimizerG, netG)
            torch.save({
                "netC": netC.state_dict(), "schedulerC": schedulerC.state_dict(), "optimizerC": optimizerC.state_dict(),
                "netG": netG.state_dict(), "schedulerG": schedulerG.state_dict(), "optimizerG": optimizerG.state_dict(),
                "clean_model": clean_model.state_dict(), "best_clean_acc": best_clean_acc, "best_bd_acc": best_bd_acc,
                "best_cross_acc": best_cross_acc, "best_F_acc": best_F_acc, "best_clean_model_acc": best_clean_model_acc,
                "best_clean_model_bd_ba": best_clean_model_bd_ba, "best_clean_model_bd_asr": best_clean_model_bd_asr,
                "epoch_current": epoch, "mask": mask, "pattern": pattern}, opt.ckpt_path)
    return (best_clean_acc, best_bd_acc, best_cross_acc, best_F_acc, best_clean_model_acc, best_clean_model_bd_ba,
            best_clean_model_bd_asr)


def _accuracies(c):
    bd_n = max(c["bd_n"], 1)
    return dict(clean=c["clean"] * 100.0 / c["clean_n"], bd=c["bd"] * 100.0 / bd_n, cross=c["cross"] * 100.0 / bd_n,
                F=c["F"] * 100.0 / bd_n, cm=c["cm"] * 100.0 / c["clean_n"], cm_ba=c["cm_ba"] * 100.0 / bd_n,
                cm_asr=c["cm_asr"] * 100.0 / bd_n)


def main():
    opt, rank, world = run.start(run.seed_ranks_apart, fix_blur)
    train_dl = get_dataloader(opt, True, rank=rank, world=world)
    test_dl = get_dataloader(opt, False, shuffle=False, rank=rank, world=world)
    train_dl2 = get_dataloader(opt, True, rank=rank, world=world)
    test_dl2 = get_dataloader(opt, False, rank=rank, world=world)      # shuffled, as the reference's (:538)
    if opt.seed is not None:     # a seeded loader derives its permutations from --seed: keep the two train orders apart
        train_dl2.base_seed += SECOND_LOADER_SEED
        test_dl2.base_seed += SECOND_LOADER_SEED
    models = netC, _, _, netG, _, _, netF, clean_model = get_model(opt)
    run.checkpoint_layout(opt, "{}_clean".format(opt.saving_prefix))
    run.load_detector(netF, opt)
    run.load_clean_model(clean_model, opt)
    best, epoch_current, mask_pattern = run.resume_or_start(opt, rank, models, BEST_KEYS, mask_pattern=True)   # :597-623
    run.broadcast(world, netC, netG, clean_model, netF)
    run.epoch_loop(opt, train, eval, models, (train_dl, train_dl2), (test_dl, test_dl2), mask_pattern, best, epoch_current,
                   run.writer(opt, rank))


if __name__ == "__main__":
    main()
