"""Argument checks of the paired and grouped trigger entry points on the strip route (64 < hw <= 256, hw % 16 == 0:
ImageNet-10's 224 x 224).  Every check runs before anything is launched, so dummy pointers do (as
tests/test_multilabel_cpu.py::test_entry_points_refuse_without_a_gpu)."""
import pytest

EINVAL, OK = -1, 0
A = 4096      # a non-null "pointer" that is never dereferenced
RATE = 0.08


def pair_fwd(lib, n, hw):
    return lib.combat_trigger_pair_fwd(A, A, A, A, RATE, n, hw, A, A, A, None)


def pair_bwd(lib, n, hw, out=A, l2=0.0):
    return lib.combat_trigger_pair_bwd(A, A, A, A, RATE, n, hw, A, None, out, l2, A, 1, A, None)


def groups_fwd(lib, n, hw, ps=2):
    return lib.combat_trigger_groups_fwd(A, A, A, A, RATE, n, hw, ps, A, A, None)


def groups_bwd(lib, n, hw, ps=2, out=A, l2=0.0):
    return lib.combat_trigger_groups_bwd(A, A, A, A, RATE, n, hw, ps, A, None, out, l2, 1, A, None)


@pytest.mark.parametrize("call", [pair_fwd, pair_bwd, groups_fwd, groups_bwd])
def test_size_rule(call):
    from combat_amd._lib import lib
    assert call(lib, 1, 72) == EINVAL       # on the strip route and not a multiple of 16
    assert call(lib, 1, 272) == EINVAL      # more columns than a workgroup has threads
    assert call(lib, 0, 224) == OK          # nothing to do at a valid size
    assert call(lib, 0, 80) == OK and call(lib, 0, 256) == OK
    assert call(lib, -1, 224) == EINVAL
    assert call(lib, 0, 32) == OK and call(lib, 0, 64) == OK      # the whole-plane sizes keep their rule
    assert call(lib, 1, 12) == EINVAL and call(lib, 1, 30) == EINVAL


def test_refusals_at_224():
    from combat_amd._lib import lib
    assert groups_fwd(lib, 4, 224, ps=0) == EINVAL
    assert groups_bwd(lib, 4, 224, ps=0) == EINVAL
    assert groups_bwd(lib, 4, 224, out=None, l2=0.5) == EINVAL      # L2 term without `out`
    assert pair_bwd(lib, 4, 224, out=None, l2=0.5) == EINVAL
    assert lib.combat_trigger_pair_fwd(A, A, A, A, RATE, 4, 224, A, None, A, None) == EINVAL     # no out_cross
    assert lib.combat_trigger_groups_fwd(A, A, A, None, RATE, 4, 224, 2, A, A, None) == EINVAL   # no k1
