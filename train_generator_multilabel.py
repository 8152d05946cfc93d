"""Alternated training of the multi-target-label attack on MI355X.

Drop-in for the reference script of the same name (reference train_generator_multilabel.py:78-118 get_model, :121-305
train, :308-455 eval, :458-612 main): classifier, clean model, low-pass trigger, augmentation and detector are
train_generator.py's.  What differs, and is implemented here:
  * the generator is the label-conditioned CUnetGeneratorv1 (networks/models.py:472-555; nets.CUnetGeneratorv1), called
    as netG(inputs, labels).  The reference constructs CelebA's with a keyword its constructor does not have
    (``n_classes=``, :96: a TypeError there); here it is built from ``opt`` for every dataset;
  * optimizerG is SGD at lr_C * 0.1 and schedulerG steps on the C milestones (:115-116);
  * the blur is the module-level T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (:53): --kernel_size / --sigma are ignored;
  * Phase C poisons the first num_bd images of the batch towards their OWN labels, Phase G cuts the batch into per-class
    chunks (:171-224): ``combat_amd.step.MultiLabelStep``;
  * evaluation makes one pass per target class over every test batch, each with its own blur draw; images whose clean
    label is the target are left out of the backdoor and clean-model counts, the detector's accuracy is over
    total_clean_sample * num_classes (:355-386);
  * the checkpoint carries the (unused) mask / pattern tensors drawn at start-up (:557-560, :440-441), restored on
    --continue_training.
The reference's F-model table (:19-28) names detectors this repository has no engine for: every --F_model other than
'original' / 'original_holdout' is refused.  Its dataloader is train_generator.py's (utils.dataloader).

--dataset cifar10 | celeba | imagenet10 (reference :97-100, :469-): at ImageNet-10's 224 x 224 (10 classes,
ResNet18(input_size=224), bs forced to 32: eight chunks of four images) the grouped trigger runs as 16-row strips and the
label conditioning on a 224 x 224 map; pass --allow_missing_F there, as for train_generator.py.

Single process only: MultiLabelStep has no data-parallel path and refuses a process group of more than one rank.
"""
import torch

import train_generator as base
from combat_amd import api, run
from combat_amd.data import get_dataloader
from combat_amd.log import progress_bar
from combat_amd.nets import CUnetGeneratorv1, FrequencyModel, default_classifier
from combat_amd.step import MultiLabelStep, create_targets_bd  # noqa: F401  (re-exported like the reference)

create_dir = base.create_dir
fix_blur = run.fix_blur
BEST_KEYS = base.BEST_KEYS
SCALARS = base.ACCURACIES + (("L2 Loss", "loss_l2_sum"), ("CleanModel Loss", "clean_model_loss_sum"))     # :288-302


def create_inputs_bd(inputs, targets, netG, opt):
    """:67-75: netG(inputs, targets) -> low_freq -> clamp-mix -> GaussianBlur (one sigma per call)."""
    return api.create_backdoor(netG, inputs, opt, labels=targets)


def get_model(opt):
    if opt.model != "default" or opt.model_clean != "default":
        raise Exception("only the default classifier of each dataset runs on the HIP path")
    if opt.F_model not in ("original", "original_holdout"):
        raise Exception("--F_model %s: only the 'original' frequency detector has a HIP engine; the reference's other "
                        "table entries (dropout, ensemble, vgg13, densenet121, mobilenetv2, resnet18) are not implemented"
                        % opt.F_model)
    fix_blur(opt)
    netC = default_classifier(opt).to(opt.device)
    clean_model = default_classifier(opt).to(opt.device)
    netG = CUnetGeneratorv1(opt).to(opt.device)
    netF = FrequencyModel(num_classes=2, n_input=opt.input_channel, input_size=opt.input_height).to(opt.device)
    optimizerC = torch.optim.SGD(netC.parameters(), opt.lr_C, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerC = torch.optim.lr_scheduler.MultiStepLR(optimizerC, opt.schedulerC_milestones, opt.schedulerC_lambda)
    optimizerG = torch.optim.SGD(netG.parameters(), opt.lr_C * 0.1, momentum=0.9, weight_decay=5e-4, nesterov=True)
    schedulerG = torch.optim.lr_scheduler.MultiStepLR(optimizerG, opt.schedulerC_milestones, opt.schedulerC_lambda)
    return netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model


def train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, mask, pattern, tf_writer,
          epoch, opt):
    run.alternated_epoch("train_generator_multilabel.py", MultiLabelStep,
                         (netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model), (train_dl,),
                         base.PROGRESS, SCALARS, 1, tf_writer, epoch, opt)


def _accuracies(c, num_classes):
    bd_n = max(c["bd_n"], 1)
    return dict(clean=c["clean"] * 100.0 / c["clean_n"], bd=c["bd"] * 100.0 / bd_n,
                F=c["F"] * 100.0 / (c["clean_n"] * num_classes), cm=c["cm"] * 100.0 / c["clean_n"],
                cm_ba=c["cm_ba"] * 100.0 / bd_n, cm_asr=c["cm_asr"] * 100.0 / bd_n)


def eval(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, test_dl, mask, pattern, best_clean_acc,
         best_bd_acc, best_F_acc, best_clean_model_acc, best_clean_model_bd_ba, best_clean_model_bd_asr, tf_writer, epoch, opt):
    print(" Eval:")
    netC.eval()
    netG.eval()
    clean_model.eval()
    c = dict(clean_n=0, bd_n=0, clean=0, bd=0, F=0, cm=0, cm_ba=0, cm_asr=0)
    n_batches = len(test_dl)
    for batch_idx, (inputs, targets) in enumerate(test_dl):
        with torch.no_grad():
            targets_host = targets.cpu()
            inputs, targets = inputs.to(opt.device), targets.to(opt.device)
            cnt = [(netC(inputs).argmax(1) == targets).sum(), (clean_model(inputs).argmax(1) == targets).sum()]
            c["clean_n"] += len(inputs)
            for ci in range(opt.num_classes):            # :355-378: the whole batch towards every class in turn
                tmp = targets * 0 + ci
                inputs_bd = create_inputs_bd(inputs, tmp, netG, opt)
                ntrg = targets != tmp                      # clean label == target label: not counted
                c["bd_n"] += int((targets_host != ci).sum())
                cm_bd = clean_model(inputs_bd).argmax(1)
                cnt += [((netC(inputs_bd).argmax(1) == tmp) & ntrg).sum(), ((cm_bd == targets) & ntrg).sum(),
                        ((cm_bd == tmp) & ntrg).sum(), (api.frequency_logits(netF, inputs_bd, opt).argmax(1) == 1).sum()]
            cnt = torch.stack(cnt).cpu().tolist()          # the batch's counters in one device->host read
            c["clean"] += int(cnt[0])
            c["cm"] += int(cnt[1])
            for ci in range(opt.num_classes):
                bd, ba, asr, f = cnt[2 + 4 * ci: 6 + 4 * ci]
                c["bd"] += int(bd)
                c["cm_ba"] += int(ba)
                c["cm_asr"] += int(asr)
                c["F"] += int(f)
        acc = _accuracies(c, opt.num_classes)
        progress_bar(batch_idx, n_batches,
                     "Clean Acc: {:.4f} - Best: {:.4f} | Bd Acc: {:.4f} - Best: {:.4f} | F Acc: {:.4f} - Best: {:.4f} | "
                     "Clean Model Acc: {:.4f} - Best: {:.4f} | Clean Model Bd BA: {:.4f} - Best: {:.4f} | "
                     "Clean Model Bd ASR: {:.4f} - Best: {:.4f}".format(
                         acc["clean"], best_clean_acc, acc["bd"], best_bd_acc, acc["F"], best_F_acc, acc["cm"],
                         best_clean_model_acc, acc["cm_ba"], best_clean_model_bd_ba, acc["cm_asr"], best_clean_model_bd_asr))
    if not epoch % 1:
        tf_writer.add_scalars("Test Accuracy", {
            "Clean": acc["clean"], "Bd": acc["bd"], "F": acc["F"], "Clean Model Acc": acc["cm"],
            "Clean Model Bd BA": acc["cm_ba"], "Clean Model Bd ASR": acc["cm_asr"]}, epoch)
    if acc["clean"] > best_clean_acc or (acc["clean"] == best_clean_acc and acc["bd"] > best_bd_acc):     # :420
        print(" Saving...")
        best_clean_acc, best_bd_acc, best_F_acc = acc["clean"], acc["bd"], acc["F"]
        best_clean_model_acc, best_clean_model_bd_ba, best_clean_model_bd_asr = acc["cm"], acc["cm_ba"], acc["cm_asr"]
        api.sync_momentum_to_optimizer(optimizerC, netC)
        api.sync_momentum_to_optimizer(optimizerG, netG)
        torch.save({
            "netC": netC.state_dict(), "schedulerC": schedulerC.state_dict(), "optimizerC": optimizerC.state_dict(),
            "netG": netG.state_dict(), "schedulerG": schedulerG.state_dict(), "optimizerG": optimizerG.state_dict(),
            "clean_model": clean_model.state_dict(), "best_clean_acc": best_clean_acc, "best_bd_acc": best_bd_acc,
            "best_F_acc": best_F_acc, "best_clean_model_acc": best_clean_model_acc,
            "best_clean_model_bd_ba": best_clean_model_bd_ba, "best_clean_model_bd_asr": best_clean_model_bd_asr,
            "epoch_current": epoch, "mask": mask, "pattern": pattern}, opt.ckpt_path)
    return (best_clean_acc, best_bd_acc, best_F_acc, best_clean_model_acc, best_clean_model_bd_ba,
            best_clean_model_bd_asr)


def main():
    opt, rank, world = run.start(run.seed_ranks_apart, fix_blur, one_process="train_generator_multilabel.py runs as one "
                                 "process: the multi-label step has no data-parallel path")
    train_dl = get_dataloader(opt, True)
    test_dl = get_dataloader(opt, False, shuffle=False)
    models = _, _, _, _, _, _, netF, clean_model = get_model(opt)
    run.checkpoint_layout(opt, "{}_clean".format(opt.saving_prefix))
    run.load_detector(netF, opt)
    run.load_clean_model(clean_model, opt)
    best, epoch_current, mask_pattern = run.resume_or_start(opt, rank, models, BEST_KEYS, mask_pattern=True)   # :557-560
    run.epoch_loop(opt, train, eval, models, (train_dl,), (test_dl,), mask_pattern, best, epoch_current,
                   run.writer(opt, rank))


if __name__ == "__main__":
    main()
