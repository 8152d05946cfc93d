"""The 224 x 224 low-pass pinned to the reference's own code (tests/golden/lowfreq224.npz, made by
tests/golden/make_golden_lowfreq224.py from the reference's utils/dct.py): until now only 32 and 64 were pinned
(tests/golden/dct.npz).

Bound 1e-5 absolute on values in [-1, 1]: the reference takes the transform through an FFT and the oracle / the
trigger kernels through dense matrices, which round differently; measured 3.1e-6 (oracle.low_freq) and 2.7e-6
(P @ X @ P^T with trigger.lowpass_matrix), the bound is about three times that."""
import numpy as np
import torch

from combat_amd import trigger
from oracle import combat_oracle as O


def _fixture(golden):
    g = golden("lowfreq224")
    x = torch.from_numpy(g["x_bf16_bits"].view(np.int16)).view(torch.bfloat16).float()
    return x, torch.from_numpy(g["y"]), float(g["ratio"])


def test_oracle_low_freq_224_matches_reference(golden):
    x, y, ratio = _fixture(golden)
    assert tuple(x.shape) == (1, 3, 224, 224) and float(x.abs().max()) <= 1.0
    err = float((O.low_freq(x, ratio) - y).abs().max())
    print("oracle.low_freq vs reference: %.3g" % err)
    assert err < 1e-5


def test_lowpass_matrix_224_matches_reference(golden):
    x, y, ratio = _fixture(golden)
    p = trigger.lowpass_matrix(224, ratio)
    assert p.dtype == torch.float32 and tuple(p.shape) == (224, 224)
    err = float((p @ x @ p.T - y).abs().max())
    print("P @ X @ P^T vs reference: %.3g" % err)
    assert err < 1e-5
    assert float((p - O.lowpass_matrix(224, ratio)).abs().max()) == 0.0     # the matrix the kernels are handed
