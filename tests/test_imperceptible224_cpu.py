"""The imperceptible (total-variation) attack at ImageNet-10's 224 x 224, host side: the two entry points of the strip
route (combat_trigger_tv_big_fwd / _bwd) are declared in include/combat_hip.h and bound in combat_amd/_lib.py with the
argument lists of the whole-plane entry points they stand beside."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "combat_hip.h")
PAIRS = {"combat_trigger_tv_big_fwd": "combat_trigger_tv_fwd", "combat_trigger_tv_big_bwd": "combat_trigger_tv_bwd"}


def _declared_params(name):
    """The parameter types of `int name(...);` in the header, comments and parameter names stripped."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/combat_hip.h" % name
    return [re.sub(r"\s+", " ", re.sub(r"\w+\s*$", "", p.strip())).strip() for p in m.group(1).split(",")]


def test_tv_big_entry_points_are_declared_and_bound():
    from combat_amd import _lib
    for new, old in PAIRS.items():
        assert new in _lib.SIGNATURES, new
        res, args = _lib.SIGNATURES[new]
        res_old, args_old = _lib.SIGNATURES[old]
        assert res is res_old and len(args) == len(args_old)
        assert all(a is b for a, b in zip(args, args_old)), new
        assert _declared_params(new) == _declared_params(old), new
        assert len(_declared_params(new)) == len(args)


def test_header_cites_the_reference_lines():
    text = open(HEADER).read()
    at = text.index("combat_trigger_tv_big_fwd")
    block = text[text.rindex("/*", 0, at):at]
    assert "train_generator_imperceptible.py:228, :234-237" in block
