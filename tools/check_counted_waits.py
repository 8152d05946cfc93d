"""Static check of the counted `s_waitcnt vmcnt(N)` waits in the DMA-staged convolution kernels.

    python tools/check_counted_waits.py [combat_amd/libcombat_hip.so | file.o | file.co] [--dump KERNEL_SUBSTRING]

The four kernel families of the hot path (conv3x3_dma[_pro]_kernel, conv3x3_ws_kernel, conv_gather_dma*,
conv_wgrad3x3_dma) synchronise with counted waits whose immediates are right only while the compiler keeps an exact
number of vector-memory loads in flight.  This tool reads the gfx950 code
object out of the library that was actually built, disassembles it with llvm-objdump and walks every kernel's
instruction stream as a list of events:

    D  buffer_load ... lds (LDS-DMA)          L  a load with a register destination
    s  a store / atomic without return        Wn s_waitcnt with vmcnt(n)          |  s_barrier

Ring kernels: a "slot" is what lies between a barrier and the next counted wait.  At a counted wait that is followed
by a barrier, with S1 loads in the slot before it, S2 in the slot before that and WPW = the weight tile's DMA group
that leads a slot, the immediate N must satisfy N <= (S2 - WPW) + S1: the tile issued at the head of slot S2 is what
the wait is for, and only LOADS issued behind it may stay in flight (stores are acknowledged out of order with
loads).  N greater is an error (a weight tile can be read before it lands), N smaller a warning (over-wait).  A slot
that holds register loads holds the epilogue fetches: their number must be EpiCfg::NPF = 3 * (BN / 16) + 4.

The other families keep their waits in run-time loops; there the counted immediates must belong to the set the
source declares, every stretch between two barriers must issue zero or one unit of DMA loads, and the
weight-stationary kernel must carry the operand loads its flavour declares.

Limits of a linear walk, stated rather than hidden:
  * conv3x3_ws_kernel: the operand loads are counted over everything behind the first drain, epilogue included, and
    the position rule looks only at the LAST of them (a wait must stand between it and the next DMA group).  That
    does not locate the ws_touch site per loop iteration: if only some operand loads moved behind the touch while a
    later load kept its wait, the kernel would still pass.  The count catches a dropped load, not every moved one.
  * conv_gather_dma*: the immediates of the main loop ({0, NDMA .. 4 NDMA}) and of the tail ({0, 4 .. 16}) are checked
    as ONE merged set per kernel, not per loop: an immediate of the tail's set inside the main loop would pass.  For
    the second-source and pair kernels the DMA-unit rule is off as well (listed as "not checked").  These kernels
    are covered in the cold state by tests/test_kernels_cold_gpu.py.

A wait whose slots cross a branch or a branch target cannot be attributed by a linear walk; it is counted as
"boundary" and reported, never silently passed.  A kernel for which no rule could be derived at all is listed as
"not checked: <reason>".
"""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
DEFAULT_LIB = os.path.join(ROOT, "combat_amd", "libcombat_hip.so")
EPILOGUE_HPP = os.path.join(ROOT, "combat_amd", "csrc", "conv_dma_epilogue.hpp")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FAMILIES = ("conv3x3_dma", "conv3x3_ws", "conv_gather_dma", "conv_wgrad3x3_dma")

Event = collections.namedtuple("Event", "kind n addr")     # kind: D L s W | B (branch) T (branch target); w: a W without lgkmcnt(0)
Finding = collections.namedtuple("Finding", "kernel addr text")


# ---------------------------------------------------------------------------------------------- code objects
def _elf_sections(blob):
    """{name: bytes} of a 64-bit little-endian ELF image."""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = heads[shstrndx]
    strtab = blob[names[4]:names[4] + names[5]]
    out = {}
    for h in heads:
        name = strtab[h[0]:strtab.index(b"\0", h[0])].decode()
        if h[1] != 8:       # SHT_NOBITS
            out[name] = blob[h[4]:h[4] + h[5]]
    return out


def _unbundle(blob):
    """gfx950 code objects of every clang offload bundle in `blob`."""
    out = []
    for m in re.finditer(re.escape(BUNDLE_MAGIC), blob):
        base = m.start()
        count, = struct.unpack_from("<Q", blob, base + len(BUNDLE_MAGIC))
        p = base + len(BUNDLE_MAGIC) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", blob, p)
            p += 24
            target = blob[p:p + idlen].decode()
            p += idlen
            if target.startswith("hip") and target.endswith("gfx950") and size:
                out.append(blob[base + off:base + off + size])
    return out


def code_objects(path):
    """The gfx950 code objects shipped in `path`: a shared library or host object with a .hip_fatbin section, an
    offload bundle, or a bare device ELF (a --cuda-device-only compile)."""
    with open(path, "rb") as f:
        blob = f.read()
    if blob.startswith(BUNDLE_MAGIC):
        return _unbundle(blob)
    if blob[:4] != b"\x7fELF":
        raise ValueError("%s: neither an ELF image nor an offload bundle" % path)
    machine, = struct.unpack_from("<H", blob, 0x12)
    if machine == 224:      # EM_AMDGPU
        return [blob]
    fat = _elf_sections(blob).get(".hip_fatbin")
    if fat is None:
        raise ValueError("%s: no .hip_fatbin section" % path)
    return _unbundle(fat)


def disassemble(code_object):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object)
        f.flush()
        return subprocess.run([OBJDUMP, "-d", "--symbolize-operands", f.name], check=True, capture_output=True, text=True).stdout


# ---------------------------------------------------------------------------------------------- event streams
_SYM = re.compile(r"^([0-9a-f]{8,16}) <([^>]+)>:\s*$")
_INSN = re.compile(r"^\s+(\S+)(?:\s+(.*?))?\s*//\s*([0-9A-Fa-f]+):")
_VMCNT = re.compile(r"vmcnt\((\d+)\)")


def kernel_streams(text):
    """{symbol: [Event]} from llvm-objdump -d --symbolize-operands output."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _SYM.match(line)
        if m:
            if re.match(r"L\d+$", m.group(2)):
                if cur is not None:
                    cur.append(Event("T", 0, int(m.group(1), 16)))
            else:
                cur = out.setdefault(m.group(2), [])
            continue
        m = _INSN.match(line)
        if not m or cur is None:
            continue
        op, args, addr = m.group(1), m.group(2) or "", int(m.group(3), 16)
        ev = classify(op, args)
        if ev:
            cur.append(Event(ev[0], ev[1], addr))
    return out


def classify(op, args):
    """(kind, n) of one instruction, or None if it neither moves the vector-memory counter nor synchronises."""
    if op == "s_waitcnt":
        m = _VMCNT.search(args)
        if not m:
            return None
        # the kernels' own waits are "s_waitcnt vmcnt(N) lgkmcnt(0)" in ONE instruction; the compiler's for a register's
        # load or a store carry vmcnt alone
        return ("W" if "lgkmcnt(0)" in args else "w", int(m.group(1)))
    if op == "s_barrier":
        return ("|", 0)
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm")):
        return ("B", 0)
    fam = op.split("_")[0]
    if fam in ("buffer", "global", "flat", "scratch", "tbuffer", "image"):
        rest = op[len(fam) + 1:]
        if rest.startswith("load"):
            return ("D", 0) if re.search(r"\blds\b", args) else ("L", 0)
        if rest.startswith("store"):
            return ("s", 0)
        if rest.startswith("atomic"):
            return ("L", 0) if re.search(r"\b(glc|sc0)\b", args) else ("s", 0)
    return None


def render(events):
    out = []
    for e in events:
        out.append({"W": " W%d " % e.n, "w": " w%d " % e.n, "|": "|", "B": " b ", "T": " : "}.get(e.kind, e.kind))
    return re.sub(r" +", " ", "".join(out))


_TEMPLATE = re.compile(r"\d(conv[a-z0-9_]+_kernel)I((?:L[a-z]n?\d+E)+)E")


def demangle(symbol):
    """(kernel name, [template arguments]) of an Itanium-mangled kernel symbol with integral template arguments."""
    m = _TEMPLATE.search(symbol)
    if not m or not m.group(1).startswith(FAMILIES):
        return None, []
    return m.group(1), [(-int(v) if neg else int(v)) for neg, v in re.findall(r"L[a-z](n?)(\d+)E", m.group(2))]


def pretty(symbol):
    name, args = demangle(symbol)
    return "%s<%s>" % (name, ",".join(map(str, args))) if name else symbol


# ---------------------------------------------------------------------------------------------- the ring rule
def check_slots(kernel, events, wpw, npf, res):
    """The slot rule on one linear event stream (see the module docstring).  Returns (checked, boundary, trivial)."""
    slots = [None]              # load counts of the slots since the last drain; None = unknown (control flow)
    regs = 0                    # register-destination loads in the current slot
    checked = boundary = trivial = 0
    for i, e in enumerate(events):
        if e.kind in "DL":
            if slots[-1] is not None:
                slots[-1] += 1
            regs += e.kind == "L"
        elif e.kind in "BT":
            slots, regs = [None], 0
        elif e.kind == "|":
            slots.append(0)
            regs = 0
        elif e.kind in "Ww":
            nxt = events[i + 1].kind if i + 1 < len(events) else ""
            if nxt == "|":
                s1 = slots[-1]
                s2 = slots[-2] if len(slots) > 1 else None
                if e.n == 0:
                    checked += 1                        # a drain can never be too weak
                elif s1 is None or s2 is None:
                    boundary += 1
                elif s2 < wpw:
                    trivial += 1                        # nothing issued at the head of S2 since the last drain
                else:
                    checked += 1
                    bound = s2 - wpw + s1
                    if e.n > bound:
                        res.errors.append(Finding(kernel, e.addr, "vmcnt(%d) allows more than the %d loads issued behind "
                                                  "the awaited weight tile (S2 = %d, WPW = %d, S1 = %d)" % (e.n, bound, s2, wpw, s1)))
                    elif e.n < bound:
                        res.warnings.append(Finding(kernel, e.addr, "over-wait: vmcnt(%d), %d loads could stay in flight" % (e.n, bound)))
                if regs and npf is not None and regs != npf:
                    res.errors.append(Finding(kernel, e.addr, "the slot before this wait holds %d epilogue fetches, EpiCfg::NPF is %d"
                                              % (regs, npf)))
            if e.n == 0:
                slots = [0]     # everything older has landed
    return checked, boundary, trivial


def check_ring(symbol, name, args, events, res):
    if name == "conv3x3_dma_kernel":
        bn, _tw, _hb, nw, rpw = args
    else:
        (bn, _tw, _hb, _flx), nw, rpw = args, 4, 32
    wpw = bn // (8 * nw)
    npf = 0 if rpw == 64 else 3 * (bn // 16) + 4        # EpiCfg<TileCfg<128, BN, 4>>::NPF; wide tiles fetch behind the loop
    checked, boundary, trivial = check_slots(pretty(symbol), events, wpw, npf, res)
    if rpw != 64:
        got = [e.n for i, e in enumerate(events) if e.kind in "Ww" and e.n > npf and i + 1 < len(events) and events[i + 1].kind == "|"]
        if not got or any(n != npf + wpw for n in got) or len(got) % 2:
            res.errors.append(Finding(pretty(symbol), 0, "expected pairs of waits vmcnt(NPF + WPW = %d) at taps PF_T + 1, PF_T + 2 of every "
                                      "last chunk, found %s" % (npf + wpw, got)))
    if checked < 6:
        res.not_checked.append("%s: only %d waits could be attributed (%d at block boundaries)" % (pretty(symbol), checked, boundary))
    return checked, boundary, trivial


# ---------------------------------------------------------------------------------------------- run-time loops
def barrier_waits(events):
    """The kernels' counted waits: vmcnt(N) lgkmcnt(0) in one instruction, directly in front of a barrier."""
    return [e for i, e in enumerate(events) if e.kind == "W" and i + 1 < len(events) and events[i + 1].kind == "|"]


def dma_stretches(events, every=False):
    """Numbers of LDS-DMA loads between the barrier of a counted wait and the next barrier (instruction order);
    every: between any two barriers behind the first counted wait (a loop whose barriers stand alone)."""
    runs, n, inside, seen = [], 0, False, False
    for i, e in enumerate(events):
        if e.kind == "|":
            if inside:
                runs.append((n, e.addr))
            seen = seen or (i > 0 and events[i - 1].kind == "W")
            n, inside = 0, seen if every else (i > 0 and events[i - 1].kind == "W")
        elif e.kind == "D":
            n += 1
    return runs


def check_set(symbol, events, allowed, unit, res, every=False):
    kernel = pretty(symbol)
    waits = barrier_waits(events)
    for e in waits:
        if e.n not in allowed:
            res.errors.append(Finding(kernel, e.addr, "vmcnt(%d) in front of a barrier is not one of the declared %s" % (e.n, sorted(allowed))))
    missing = allowed - {e.n for e in waits}
    if missing:
        res.not_checked.append("%s: declared immediates %s do not occur in front of a barrier" % (kernel, sorted(missing)))
    if unit:
        runs = dma_stretches(events, every)
        if not any(n for n, _ in runs):
            res.not_checked.append("%s: no DMA stretch between two barriers" % kernel)
        for n, addr in runs:
            if n not in (0, unit):
                res.errors.append(Finding(kernel, addr, "the stretch in front of this barrier issues %d DMA loads, the waits count in units of %d" % (n, unit)))
    return len(waits)


def epilogue_flavours():
    """kEpiFlavours of conv_dma_epilogue.hpp as integers."""
    with open(EPILOGUE_HPP) as f:
        src = f.read()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(EF_[A-Z0-9_]+) = (\d+),", src)}
    body = re.search(r"kEpiFlavours\[\] = \{(.*?)\};", src, re.S).group(1)
    out = []
    for line in body.splitlines():
        expr = line.split("//")[0].strip().rstrip(",")
        if expr:
            out.append(sum(bits[t.strip()] for t in expr.split("|")) if expr != "0" else 0)
    return out, bits


def check_ws(symbol, args, events, res):
    """conv3x3_ws_kernel<FLI>: every counted wait is a drain, a half-period issues one halo patch (HPW = 6 pieces), and
    the loop -- everything behind the first drain -- carries the EQ operand loads of each tensor its flavour reads (all
    3 * EQ = NPF - 4 with a mask; the four table loads sit in front of the loop, where a flavour may not need them all)."""
    kernel = pretty(symbol)
    flavours, bits = epilogue_flavours()
    fl = -1 if args[0] < 0 else flavours[args[0]]
    eq = 64 // 16
    want = eq * (2 + (fl < 0 or bool(fl & bits["EF_MASK"])))
    first = next((i for i, e in enumerate(events) if e.kind in "Ww" and e.n == 0), None)
    if first is None:
        res.not_checked.append("%s: no drain in front of the loop" % kernel)
        return 0
    got = sum(e.kind == "L" for e in events[first:])
    if got != want:
        res.errors.append(Finding(kernel, events[first].addr, "%d operand loads in front of ws_touch, the flavour declares %d (NPF = %d with the tables)"
                                  % (got, want, 3 * eq + 4)))
    # (this takes the LAST load behind the first drain and asks for some wait in front of the next DMA: it does not
    # locate the touch site per iteration -- see "Limits" in the module docstring)
    # position: ws_touch is what makes the compiler wait for these registers, so a wait must stand between the last
    # operand load and the next halo patch's DMA group -- a load moved behind the touch site has no such wait
    loads = [i for i in range(first, len(events)) if events[i].kind == "L"]
    if loads:
        rest = events[loads[-1] + 1:]
        touch = next((i for i, e in enumerate(rest) if e.kind in "Ww"), None)
        dma = next((i for i, e in enumerate(rest) if e.kind == "D"), None)
        if touch is None or (dma is not None and dma < touch):
            res.errors.append(Finding(kernel, events[loads[-1]].addr, "no wait (ws_touch) between the last operand load and the next DMA group"))
    tabs = sum(e.kind == "L" for e in events[:first])
    if tabs > 4:
        res.errors.append(Finding(kernel, 0, "%d table loads in front of the loop, at most 4 declared" % tabs))
    return check_set(symbol, events, {0}, 6, res, every=True)


def check_gather(symbol, name, args, events, res):
    """conv_gather_dma*<BN, NS>: NDMA = 4 + BN / 32 DMA loads per step, up to NS - 2 younger steps in flight; the wait
    in front of the loop counts the 4 pixel-row pieces of each younger step."""
    bn, ns = args[0], args[1]
    ndma = 4 + bn // 32
    # (main loop and tail are not told apart by a linear walk: ONE merged set, see the module docstring)
    allowed = {0} | {k * ndma for k in range(1, 5) if ns > k + 1} | {4 * k for k in range(1, 5) if ns > k + 1}
    if name != "conv_gather_dma_kernel":    # the second source's DMA groups are alternatives behind a uniform branch
        res.not_checked.append("%s: DMA unit per step (alternative DMA groups between two barriers); immediates checked "
                               "against the merged main-loop and tail set, not per loop" % pretty(symbol))
        ndma = 0
    return check_set(symbol, events, allowed, ndma, res)


def check_wgrad(symbol, args, events, res):
    """conv_wgrad3x3_dma_kernel<HPW, NS, RED>: NDMA = 1 + HPW per patch; a ring of two stages only ever drains."""
    hpw, ns = args[0], args[1]
    ndma = 1 + hpw
    allowed = {0, ndma, (ns - 2) * ndma} if ns > 2 else {0}
    return check_set(symbol, events, allowed, ndma, res)


# ---------------------------------------------------------------------------------------------- driver
class Result:
    def __init__(self):
        self.errors, self.warnings, self.not_checked = [], [], []
        self.families = collections.OrderedDict((f, 0) for f in FAMILIES)
        self.waits = collections.Counter()

    def ok(self):
        return not self.errors

    def summary(self):
        lines = []
        for fam, n in self.families.items():
            skipped = [s for s in self.not_checked if s.startswith(fam)]
            lines.append("counted waits: %-18s %2d instantiations, %3d waits attributed, %d warnings, not checked: %s"
                         % (fam, n, self.waits[fam], sum(w.kernel.startswith(fam) for w in self.warnings),
                            "; ".join(skipped) if skipped else "none"))
        return lines

    def report(self):
        lines = self.summary()
        for tag, items in (("error", self.errors), ("warning", self.warnings)):
            for f in items:
                lines.append("%s: %s at 0x%x: %s" % (tag, f.kernel, f.addr, f.text))
        return "\n".join(lines)


def family_of(name):
    if name.startswith("conv_wgrad3x3_dma"):
        return "conv_wgrad3x3_dma"
    if name.startswith("conv_gather_dma"):
        return "conv_gather_dma"
    if name.startswith("conv3x3_ws"):
        return "conv3x3_ws"
    return "conv3x3_dma"


def check_streams(streams, res=None):
    res = res or Result()
    for symbol, events in streams.items():
        name, args = demangle(symbol)
        if name is None:
            continue
        fam = family_of(name)
        if name in ("conv3x3_dma_kernel", "conv3x3_dma_pro_kernel"):
            n = check_ring(symbol, name, args, events, res)[0]
        elif name == "conv3x3_ws_kernel":
            n = check_ws(symbol, args, events, res)
        elif name in ("conv_gather_dma_kernel", "conv_gather_dma_src2_kernel", "conv_gather_dma_pair_kernel"):
            n = check_gather(symbol, name, args, events, res)
        elif name in ("conv_wgrad3x3_dma_kernel", "conv_wgrad3x3_dma_group_kernel"):   # (the grouped form: same patch loop)
            n = check_wgrad(symbol, args, events, res)
        else:
            continue
        res.families[fam] += 1
        res.waits[fam] += n
    return res


def check_file(path):
    res = Result()
    for co in code_objects(path):
        if any(f.encode() in co for f in FAMILIES):
            check_streams(kernel_streams(disassemble(co)), res)
    for fam, n in res.families.items():
        if n == 0:
            res.not_checked.append("%s: no kernel of this family in %s" % (fam, os.path.basename(path)))
    return res


def main(argv):
    paths = [a for a in argv if not a.startswith("--")]
    path = paths[0] if paths else DEFAULT_LIB
    if "--dump" in argv:
        want = argv[argv.index("--dump") + 1]
        paths = [p for p in paths if p != want]
        path = paths[0] if paths else DEFAULT_LIB
        for co in code_objects(path):
            for symbol, events in kernel_streams(disassemble(co)).items():
                if demangle(symbol)[0] and want in pretty(symbol):
                    print(pretty(symbol))
                    print("   ", render(events))
        return 0
    res = check_file(path)
    print(res.report())
    return 0 if res.ok() else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
