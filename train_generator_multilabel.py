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

Single process only: MultiLabelStep has no data-parallel path and refuses a process group of more than one rank.
"""
import os
import random
import time

import numpy as np
import torch

import config
import train_generator as base
from combat_amd import api, dist as cdist
from combat_amd.data import get_dataloader
from combat_amd.log import SummaryWriter, image_grid, progress_bar
from combat_amd.nets import CUnetGeneratorv1, FrequencyModel, configure_dataset, default_classifier
from combat_amd.step import MultiLabelStep, create_targets_bd  # noqa: F401  (re-exported like the reference)

create_dir = base.create_dir


def fix_blur(opt):
    """gauss_smooth = T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (:53), whatever the flags say."""
    opt.kernel_size = 3
    opt.sigma = (0.1, 1.0)


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


def _step_of(netC, netG, clean_model, netF, opt) -> MultiLabelStep:
    st = netC.__dict__.get("_ml_step")
    if st is None:
        pg = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
        st = MultiLabelStep(netC, netG, clean_model, netF, opt, process_group=pg)
        netC.__dict__["_ml_step"] = st
    return st


def train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, mask, pattern, tf_writer,
          epoch, opt):
    print(" Train:")
    netC.train()
    netG.train()
    clean_model.eval()
    st = _step_of(netC, netG, clean_model, netF, opt)
    st.reset_metrics()
    n_batches = len(train_dl)
    every = max(1, int(getattr(opt, "log_interval", 20)))
    m = None
    for batch_idx, (inputs, targets) in enumerate(train_dl):
        st.run(inputs.to(opt.device, non_blocking=True), targets,
               lr_c=optimizerC.param_groups[0]["lr"], lr_g=optimizerG.param_groups[0]["lr"])
        last = batch_idx == n_batches - 1 or (opt.max_steps and batch_idx + 1 >= opt.max_steps)
        if batch_idx % every == 0 or last:
            m = st.read_metrics()
            ts = m["samples"]
            progress_bar(
                batch_idx, n_batches,
                "Clean Acc: {:.4f} | Bd Acc: {:.4f} | F Acc: {:.4f} | Clean Model Acc: {:.4f} | Clean Model Bd BA: {:.4f} | "
                "Clean Model Bd ASR: {:.4f}".format(
                    m["clean_correct"] * 100.0 / ts, m["bd_correct"] * 100.0 / ts, m["f_correct"] * 100.0 / ts,
                    m["clean_model_correct"] * 100.0 / ts, m["clean_model_bd_ba"] * 100.0 / ts,
                    m["clean_model_bd_asr"] * 100.0 / ts))
        if last:
            break
    if m is None:
        raise SystemExit("train_generator_multilabel.py: the train loader yielded no batch (dataset smaller than one batch?)")
    ts = m["samples"]
    if not epoch % 1:
        tf_writer.add_scalars("Clean Accuracy", {
            "Clean": m["clean_correct"] * 100.0 / ts, "Bd": m["bd_correct"] * 100.0 / ts, "F": m["f_correct"] * 100.0 / ts,
            "CleanModel Acc": m["clean_model_correct"] * 100.0 / ts,
            "CleanModel Bd BA": m["clean_model_bd_ba"] * 100.0 / ts,
            "CleanModel Bd ASR": m["clean_model_bd_asr"] * 100.0 / ts,
            "L2 Loss": m["loss_l2_sum"] / ts, "CleanModel Loss": m["clean_model_loss_sum"] / ts}, epoch)
        tf_writer.add_image("Images", image_grid(st.inputs, st.bd, opt), global_step=epoch)
    schedulerC.step()
    schedulerG.step()


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


BEST_KEYS = ("best_clean_acc", "best_bd_acc", "best_F_acc", "best_clean_model_acc", "best_clean_model_bd_ba",
             "best_clean_model_bd_asr")


def main():
    opt = config.get_arguments().parse_args()
    configure_dataset(opt)
    fix_blur(opt)
    rank, local_rank, world = cdist.init()
    if world > 1:
        raise SystemExit("train_generator_multilabel.py runs as one process: the multi-label step has no data-parallel path")
    if opt.device == "cuda":
        opt.device = "cuda:%d" % local_rank
    if opt.seed is not None:
        torch.manual_seed(opt.seed)
        np.random.seed(opt.seed)
        random.seed(opt.seed)

    train_dl = get_dataloader(opt, True)
    test_dl = get_dataloader(opt, False, shuffle=False)
    netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model = get_model(opt)

    mode = opt.saving_prefix
    opt.ckpt_folder = os.path.join(opt.checkpoints, "{}_clean".format(mode), opt.dataset)
    opt.ckpt_path = os.path.join(opt.ckpt_folder, "{}_{}_clean.pth.tar".format(opt.dataset, mode))
    opt.log_dir = os.path.join(opt.ckpt_folder, "log_dir")

    opt.F_ckpt_path = base.detector_checkpoint_path(opt)
    print(f"Loading {opt.F_model} at {opt.F_ckpt_path}")
    if os.path.exists(opt.F_ckpt_path):
        netF.load_state_dict(torch.load(opt.F_ckpt_path, map_location=opt.device, weights_only=True)["netC"])
    elif not opt.allow_missing_F:
        print("Error: {} not found (pass --allow_missing_F to run with an untrained detector)".format(opt.F_ckpt_path))
        exit()
    netF.eval()
    print("Done")

    load_path = os.path.join(opt.checkpoints, opt.load_checkpoint_clean or "", opt.dataset,
                             "{}_{}.pth.tar".format(opt.dataset, opt.load_checkpoint_clean))
    if not os.path.exists(load_path):
        print("Error: {} not found".format(load_path))
        exit()
    clean_model.load_state_dict(torch.load(load_path, map_location=opt.device, weights_only=True)["netC"])
    clean_model.eval()

    if opt.continue_training:
        if not os.path.exists(opt.ckpt_path):
            print("Pretrained model doesnt exist")
            exit()
        print("Continue training!!")
        sd = torch.load(opt.ckpt_path, map_location=opt.device, weights_only=True)
        netC.load_state_dict(sd["netC"])
        optimizerC.load_state_dict(sd["optimizerC"])
        schedulerC.load_state_dict(sd["schedulerC"])
        netG.load_state_dict(sd["netG"])
        optimizerG.load_state_dict(sd["optimizerG"])
        schedulerG.load_state_dict(sd["schedulerG"])
        clean_model.load_state_dict(sd["clean_model"])
        api.load_momentum_from_optimizer(optimizerC, netC)
        api.load_momentum_from_optimizer(optimizerG, netG)
        best = [sd[k] for k in BEST_KEYS]
        epoch_current = sd["epoch_current"]
        mask, pattern = sd["mask"].to(opt.device), sd["pattern"].to(opt.device)
    else:
        print("Train from scratch!!!")
        best = [0.0] * len(BEST_KEYS)
        epoch_current = 0
        mask = torch.zeros(opt.input_height, opt.input_width, device=opt.device)     # :557-560 (saved, never used)
        mask[2:6, 2:6] = 0.1
        pattern = torch.rand(opt.input_channel, opt.input_height, opt.input_width).to(opt.device)
        cdist.fresh_start(opt.ckpt_folder, rank)
    create_dir(opt.log_dir)
    tf_writer = SummaryWriter(log_dir=opt.log_dir)

    train_dl.epoch = epoch_current
    for epoch in range(epoch_current, opt.n_iters):
        print("Epoch {}:".format(epoch + 1))
        t0 = time.perf_counter()
        train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, mask, pattern,
              tf_writer, epoch, opt)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        best = list(eval(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, test_dl, mask, pattern,
                         *best, tf_writer, epoch, opt))
        print(" train {:.2f} s, eval + checkpoint {:.2f} s".format(t1 - t0, time.perf_counter() - t1))


if __name__ == "__main__":
    main()
