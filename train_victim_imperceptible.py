"""Victim training on data poisoned by the frozen generator of the imperceptible configuration on MI355X.

The reference's train_victim_imperceptible.py is a symbolic link to its train_victim.py: the same flags, blur
(--kernel_size / --sigma), loop, eval and checkpoint keys.  So this is train_victim.py under the other name.
"""
import train_victim as base
from train_victim import *  # noqa: F401,F403  (the reference module's names: get_model, train, eval, main, ...)

main = base.main

if __name__ == "__main__":
    main()
