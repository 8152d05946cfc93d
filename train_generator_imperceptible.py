"""Alternated training with the imperceptible (total-variation) objective on MI355X.

Drop-in for the reference script of the same name (reference train_generator_imperceptible.py:78-120 get_model,
:123-310 train, :313-440 eval, :443-585 main): the networks, trigger, augmentation, detector, optimisers and
checkpoint are train_generator.py's.  What differs, and is added here:
  * the smoothness of the triggered images joins the generator's loss (:228, :234-237):
    loss = loss_ce + L2_weight * loss_l2 + tv_weight * total_variation(inputs_bd).mean() + clean_model_weight * ...;
    the epoch's scalars gain "TV Loss" (:263, :304); the progress line is train_generator.py's (:266-277);
  * the blur is the module-level T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (:52), in training and in eval:
    --kernel_size / --sigma are ignored, as they are there;
  * no --model / --model_clean zoo and the "original" detector only (:19-23, :78-104);
  * --continue_training restores netC, netG, their optimisers and schedulers, but NOT the checkpoint's clean_model
    (:518-534): the clean model stays the one --load_checkpoint_clean names;
  * the image grid of the last batch is logged every epoch (:306).  The reference also overwrites
    <temps>/samples.png every fifth batch (:279-290); that file is not written here.
The per-batch body (:160-277) runs as ``combat_amd.step.ImperceptibleStep`` on the HIP kernels.

Data parallel: ``python -m torch.distributed.run --nproc-per-node N ...`` as train_generator.py.  That path has not
been run on more than one GPU with this step.
"""
import torch

import train_generator as base
from combat_amd import dist as cdist
from combat_amd.log import image_grid, progress_bar
from combat_amd.step import ImperceptibleStep, create_targets_bd  # noqa: F401  (re-exported like the reference)

create_dir = base.create_dir
eval = base.eval      # :313-440: train_generator.py's, with create_inputs_bd's fixed blur (fix_blur)


def fix_blur(opt):
    """gauss_smooth = T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (:52), whatever the flags say."""
    opt.kernel_size = 3
    opt.sigma = (0.1, 1.0)


def get_model(opt):
    if opt.F_model != "original":       # :19-23: F_MAPPING_NAMES holds "original" only
        raise Exception("train_generator_imperceptible.py knows the 'original' detector only")
    return base.get_model(opt)


def _step_of(netC, netG, clean_model, netF, opt) -> ImperceptibleStep:
    st = netC.__dict__.get("_tv_step")
    if st is None:
        pg = torch.distributed.group.WORLD if torch.distributed.is_initialized() else None
        st = ImperceptibleStep(netC, netG, clean_model, netF, opt, process_group=pg)
        netC.__dict__["_tv_step"] = st
    return st


def train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, tf_writer, epoch, opt):
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
                "Clean Acc: {:.4f} | Bd Acc: {:.4f} | F Acc: {:.4f} | Clean Model Acc: {:.4f} | Clean Model Bd BA: {:.4f} "
                "| Clean Model Bd ASR: {:.4f}".format(
                    m["clean_correct"] * 100.0 / ts, m["bd_correct"] * 100.0 / ts, m["f_correct"] * 100.0 / ts,
                    m["clean_model_correct"] * 100.0 / ts, m["clean_model_bd_ba"] * 100.0 / ts,
                    m["clean_model_bd_asr"] * 100.0 / ts))
        if last:
            break
    ts = m["samples"]
    if not epoch % 1:
        tf_writer.add_scalars("Clean Accuracy", {
            "Clean": m["clean_correct"] * 100.0 / ts, "Bd": m["bd_correct"] * 100.0 / ts, "F": m["f_correct"] * 100.0 / ts,
            "CleanModel Acc": m["clean_model_correct"] * 100.0 / ts,
            "CleanModel Bd BA": m["clean_model_bd_ba"] * 100.0 / ts,
            "CleanModel Bd ASR": m["clean_model_bd_asr"] * 100.0 / ts,
            "L2 Loss": m["loss_l2_sum"] / ts, "Grad L2 Loss": m["loss_grad_l2_sum"] / ts,
            "TV Loss": m["loss_tv_sum"] / ts, "CleanModel Loss": m["clean_model_loss_sum"] / ts}, epoch)
        if not isinstance(tf_writer, cdist.NullWriter):     # :306: the last batch and its backdoored copy
            tf_writer.add_image("Images", image_grid(st.inputs, st.bd, opt), global_step=epoch)
    schedulerC.step()
    schedulerG.step()


def main():
    base.main(get_model=get_model, train=train, eval=eval, prepare=fix_blur, resume_clean_model=False)


if __name__ == "__main__":
    main()
