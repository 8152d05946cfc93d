"""tests/golden/lowfreq224.npz: the reference's low-pass (train_generator.py:47-55, through its utils/dct.py) of one
224 x 224 generator-like image, the size of the ImageNet-10 configuration.

Run in the build container only (``python tests/golden/make_golden_lowfreq224.py``): it imports ``/root/reference``
(read-only), which does not exist on the GPU box.  train_generator.py itself is not importable there (see
make_golden.py), so its five lines are restated around the reference's own dct_2d / idct_2d, as make_golden.py does for
the 32 and 64 pixel fixtures in dct.npz.

The image is tanh(3 * randn) rounded to bf16 -- what the trigger kernels read from the generator -- and is stored as its
bf16 bit patterns (``x_bf16_bits``, uint16 [1, 3, 224, 224]); ``y`` is the fp32 result."""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from utils import dct as ref_dct  # noqa: E402

HW, RATIO, SEED = 224, 0.65, 2240


def main():
    x = torch.tanh(torch.randn(1, 3, HW, HW, generator=torch.Generator().manual_seed(SEED)) * 3).to(torch.bfloat16)
    xf = x.float()
    keep = int(HW * RATIO)
    mask = torch.zeros_like(xf)
    mask[:, :, :keep, :keep] = 1
    y = ref_dct.idct_2d(ref_dct.dct_2d((xf + 1) / 2 * 255) * mask) / 255 * 2 - 1
    path = os.path.join(HERE, "lowfreq224.npz")
    np.savez_compressed(path, x_bf16_bits=x.view(torch.int16).numpy().view(np.uint16), y=y.numpy(),
                        ratio=np.float64(RATIO), seed=np.int64(SEED))
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
