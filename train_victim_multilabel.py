"""Drop-in for the reference's train_victim_multilabel.py.

The reference file is train_generator_multilabel.py over again -- the two differ in two comment lines only (:298, :483-484):
the same get_model / train / eval / main, the same dataloader (utils.dataloader) and F-model table, the same flags, the
same checkpoint.  So this script runs train_generator_multilabel.py's code under its own name (``--saving_prefix`` keeps
the two runs' checkpoints apart, as it does there).  Like the reference's file it reads --load_checkpoint_clean (the
clean model) and never --load_checkpoint, which the reference README's victim command passes: that flag is accepted and
unused, and without --load_checkpoint_clean the script stops with "not found" (the reference: a TypeError in os.path.join).
--dataset cifar10 | celeba | imagenet10 (224 x 224, bs 32, --allow_missing_F), as train_generator_multilabel.py."""
from train_generator_multilabel import (BEST_KEYS, create_inputs_bd, create_targets_bd, eval, fix_blur, get_model, main,  # noqa: F401
                                        train)

if __name__ == "__main__":
    main()
