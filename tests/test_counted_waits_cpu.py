"""The counted s_waitcnt vmcnt(N) waits of the DMA-staged convolution kernels against the loads the compiler kept
(tools/check_counted_waits.py): on the library that was built, on an object compiled WITHOUT epi_touch() / ws_touch()
(COMBAT_ABL_NOTOUCH: the defect of DESIGN.md section 5, round 4 (c) -- it must be rejected), and on a hand-written
event stream.  No GPU: the ablated object is only disassembled, never linked, loaded or run."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernels for which one rule cannot be derived from a linear walk of the disassembly (the checker names them; this
# list may shrink, not grow)
NOT_CHECKED = sorted("%s<%d,3>: DMA unit per step (alternative DMA groups between two barriers); immediates checked against the "
                     "merged main-loop and tail set, not per loop" % (k, bn)
                     for k in ("conv_gather_dma_pair_kernel", "conv_gather_dma_src2_kernel") for bn in (32, 64))


@pytest.fixture(scope="module")
def ccw():
    spec = importlib.util.spec_from_file_location("check_counted_waits", os.path.join(ROOT, "tools", "check_counted_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_built_library_passes_and_not_checked_list_is_the_committed_one(ccw):
    from combat_amd import build as b
    lib = b.build(force=False, verbose=False)
    res = ccw.check_file(lib)
    print(res.report())
    assert not res.errors, res.report()
    assert sorted(res.not_checked) == NOT_CHECKED
    # every family is there, with every instantiation the dispatcher can launch, and the ring rule really ran
    assert res.families["conv3x3_dma"] >= 42 and res.families["conv3x3_ws"] == 5
    assert res.families["conv_gather_dma"] >= 6 and res.families["conv_wgrad3x3_dma"] >= 6
    assert res.waits["conv3x3_dma"] >= 20 * res.families["conv3x3_dma"]


def test_object_without_touch_is_rejected(ccw, tmp_path):
    from combat_amd import build as b
    out = str(tmp_path / "conv3x3_dma_notouch.co")
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    subprocess.run([b.HIPCC] + flags + ["--cuda-device-only", "-DCOMBAT_ABL_NOTOUCH", "-c",
                                        os.path.join(b.CSRC, "conv3x3_dma.hip"), "-o", out], check=True)
    res = ccw.check_file(out)
    one_flavour = [e for e in res.errors if e.kernel.startswith("conv3x3_dma_pro_kernel<") and int(e.kernel.rstrip(">").split(",")[-1]) >= 0]
    assert one_flavour, res.report()
    # the error names the kernel, the position and the wait: taps PF_T + 1 / PF_T + 2 of the HB = 1 schedule wait vmcnt(18)
    assert any(e.addr and "vmcnt(18)" in e.text for e in one_flavour), res.report()
    # ... and the kernels that carry every flavour (FLX = -2: nothing is dead) are as in the shipped build
    assert not [e for e in res.errors if e.kernel.startswith("conv3x3_dma_kernel<")], res.report()


def test_slot_rule_on_a_hand_written_stream(ccw):
    """One last chunk of a ring kernel with WPW = 2, NPF = 16 (the HB = 1 schedule), then the same with one immediate
    too large, one too small, and with two epilogue fetches dropped."""
    def stream(text):
        ev, addr = [], 0
        for tok in text.split():
            addr += 4
            if tok[0] == "W":
                ev.append(ccw.Event("W", int(tok[1:]), addr))
            else:
                ev.extend(ccw.Event(c, 0, addr) for c in tok)
        return ev

    good = "DDDDDDDDDD W0 | W2 | DD W2 | DD W2 | DD W2 | DDss W2 | DD LLLLLLLLLLLLLLLL ss W18 | DDss W18 | W0 | W0 | ssss"

    def run(text):
        res = ccw.Result()
        counts = ccw.check_slots("hand<64,16,1,0>", stream(text), 2, 16, res)
        return res, counts

    res, (checked, boundary, trivial) = run(good)
    assert not res.errors and not res.warnings and boundary == 0 and checked == 8 and trivial == 2, (res.report(), checked, boundary, trivial)
    res, _ = run(good.replace("ss W18 | DDss W18", "ss W18 | DDss W19"))
    assert len(res.errors) == 1 and "vmcnt(19)" in res.errors[0].text and res.errors[0].addr
    res, _ = run(good.replace("DD W2 | DDss", "DD W1 | DDss"))
    assert not res.errors and len(res.warnings) == 1 and "over-wait" in res.warnings[0].text
    res, _ = run(good.replace("LLLLLLLLLLLLLLLL", "LLLLLLLLLLLLLL"))
    assert len(res.errors) == 3, res.report()       # both waits too large, and the fetch slot short of NPF
