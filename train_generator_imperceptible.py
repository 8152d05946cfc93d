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
import train_generator as base
from combat_amd import run
from combat_amd.step import ImperceptibleStep, create_targets_bd  # noqa: F401  (re-exported like the reference)

create_dir = base.create_dir
eval = base.eval      # :313-440: train_generator.py's, with create_inputs_bd's fixed blur (fix_blur)
fix_blur = run.fix_blur
SCALARS = base.SCALARS[:-1] + (("TV Loss", "loss_tv_sum"),) + base.SCALARS[-1:]      # :293-308


def get_model(opt):
    if opt.F_model != "original":       # :19-23: F_MAPPING_NAMES holds "original" only
        raise Exception("train_generator_imperceptible.py knows the 'original' detector only")
    return base.get_model(opt)


def train(netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model, train_dl, tf_writer, epoch, opt):
    run.alternated_epoch("train_generator_imperceptible.py", ImperceptibleStep,
                         (netC, optimizerC, schedulerC, netG, optimizerG, schedulerG, netF, clean_model), (train_dl,),
                         base.PROGRESS, SCALARS, 1, tf_writer, epoch, opt)      # :306: the image grid every epoch


def main():
    base.main(get_model=get_model, train=train, eval=eval, prepare=fix_blur, resume_clean_model=False)


if __name__ == "__main__":
    main()
