"""Per-network forward/backward schedules over the combat_hip C ABI.

A network is executed as a *plan*: the ordered list of C-ABI calls (arguments marshalled once,
buffers pre-allocated in a ``Slot``) that the reference's ``module(x)`` / ``loss.backward()``
expand to, with the normalisation / activation / residual element-wise work folded into the
convolution prologues and epilogues.  Plans are replayed with no Python work per kernel beyond
one ctypes call, and are what gets captured into a HIP graph.

Reference call sites: PreActResNet forward classifier_models/preact_resnet.py:32-40, 93-102;
UnetGenerator forward networks/models.py:321-341; FrequencyModel forward
defenses/frequency_based/model.py:49-52; their backward passes are what autograd derives.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from ._lib import STATS_PER_WORKGROUP, TILE_D128x64, TILE_S128x64, CombatHipError, ConvArgs, lib  # noqa: F401  (ConvArgs: re-exported)
from .nets import UNET_LAYERS
from .ops import Affine, PackedConv, bf16

# Statistics over the whole batch (BatchNorm) ask the convolution for one partial row per workgroup instead of one per
# wave: 256 rows instead of 1024-4096 on the 32 x 32 and 16 x 16 layers, so the fused normalisation launches reduce them
# themselves and no norm_stage1 launch stands between a convolution and its normalisation (18 launches per alternated
# step).
BATCH_STATS_ROWS = STATS_PER_WORKGROUP

f32 = torch.float32


def _p(t):
    return None if t is None else t.data_ptr()


class Call:
    """One recorded call of a plan, with everything the replay needs to know about it."""

    __slots__ = ("func", "args", "what", "queue", "after", "mark", "wgrad")

    def __init__(self, func, args, what: str, queue: Optional[int] = None, after: Optional["Call"] = None):
        self.func, self.args, self.what = func, args, what
        self.queue = queue    # None: the plan's own stream; k: auxiliary queue k (the call may run beside the calls that follow it)
        self.after = after    # an earlier Call this one waits for (on whatever queue that ran)
        self.mark = None      # flat-gradient offset that is complete once this call has been enqueued
        self.wgrad = None     # combat_conv_wgrad: its WgradArgs; combat_conv_wgrad_group: its members', as recorded


class Plan:
    """An ordered list of C-ABI calls with pre-marshalled arguments (stream appended at run)."""

    serial = False   # True: auxiliary-stream calls run in line (kernel-level measurements: one kernel at a time)
    serial_shortcuts = False   # True: shortcut input gradients as launches of their own (per-launch profiling, A/B)
    default_aux_queues = 1   # auxiliary queues a new plan deals its aux calls to (see aux_queues below)
    # Same-geometry weight gradients that follow each other on an auxiliary queue as ONE combat_conv_wgrad_group call
    # (group_wgrads below).  COMBAT_WGRAD_GROUP = off | tail (only the plan's last run of layers: PreActResNet18's four
    # layer1 convolutions) | pairs (two members at most, last stage only) | stages (every run inside a stage).  The
    # default is what measured best on the alternated step: DESIGN.md section 5.
    wgrad_groups = os.environ.get("COMBAT_WGRAD_GROUP", "stages")

    def __init__(self, name: str):
        self.name = name
        self.calls: List[Call] = []       # the schedule: queue, dependency, mark and weight-gradient arguments travel with each call
        self._keep: List = []
        self.aux_queues = Plan.default_aux_queues   # auxiliary queues the aux calls are dealt to, round-robin (each with its own
        #                                   weight-gradient scratch).  Measured: 2 for the generator's backward 4.19 -> 4.23
        #                                   ms/step, 2 for the surrogate's 4.14 -> 4.17: one queue it stays
        self._ws = None
        self._cplan = None                # combat_plan* of the compiled form (built on first run)
        self._prog = None

    def add(self, what: str, cfunc, *args, aux: bool = False, after: Optional[Call] = None) -> Call:
        """aux: the call's result is only consumed after the plan (weight gradients: by the optimiser /
        all-reduce), so it may run on the auxiliary stream beside the calls that follow it.
        after: an earlier call (typically an aux one) this call must wait for."""
        call = Call(cfunc, args, what, self.next_aux_queue() if aux else None, after)
        self.calls.append(call)
        self._changed()
        return call

    def _changed(self) -> None:       # the call list was edited: the compiled form is rebuilt on the next run
        self._prog = None

    @property
    def mark_offsets(self) -> List[int]:
        """The all-reduce marks' flat-gradient offsets, in call order."""
        return [c.mark for c in self.calls if c.mark is not None]

    @property
    def wgrads(self) -> List:
        """Every WgradArgs of the plan in recorded order (the members of a grouped call one by one)."""
        return [a for c in self.calls if c.wgrad is not None for a in (c.wgrad if isinstance(c.wgrad, list) else [c.wgrad])]

    def next_aux_queue(self) -> int:
        """Queue the next aux call will be given (round-robin over `aux_queues`)."""
        return sum(1 for c in self.calls if c.queue is not None) % self.aux_queues

    def hold(self, *objs) -> None:
        self._keep.extend(objs)

    def merge_convs(self, i: int) -> None:
        """Calls i and i + 1 are two combat_conv_gemm launches with no data dependence between them (a residual
        block's shortcut and its first convolution over the same input): make them ONE combat_conv_gemm_pair call.
        Both are plain in-line calls: no queue, no mark, no dependency of or on another call."""
        two = self.calls[i:i + 2]
        assert all(c.func is lib.combat_conv_gemm and c.queue is None and c.after is None and c.mark is None for c in two)
        assert not any(c.after in two for c in self.calls)
        self.calls[i:i + 2] = [Call(lib.combat_conv_gemm_pair, (two[0].args[0], two[1].args[0]), two[0].what + "+" + two[1].what)]
        self._changed()

    def workspace(self, device) -> torch.Tensor:
        """Scratch of this plan's convolutions (split reductions of skinny layers).  Per plan: the calls of
        one plan run one after the other on one stream, two plans may run concurrently."""
        if self._ws is None:
            self._ws = torch.empty(32 << 20, dtype=torch.uint8, device=device)
        return self._ws

    def mark(self, grad_offset: int) -> None:
        """Every gradient at flat offset >= grad_offset is final once the calls recorded so far ran."""
        self.calls[-1].mark = grad_offset
        self._changed()

    compiled = os.environ.get("COMBAT_PLAN_PY", "0") != "1"   # False: replay every plan from Python (debugging / A-B timing)

    def _program(self):
        """The C-side form of this plan (csrc/plan.cpp), built on first use: every C-ABI call is captured into a
        combat_plan with its queue; Python callables (the gradient-zeroing hand-off) and the all-reduce marks split
        it into ranges.  Returns [("c", begin, end) | ("py", func, args, what) | ("mark", offset)]."""
        if self._prog is not None:
            return self._prog
        if self._cplan:
            lib.combat_plan_destroy(self._cplan)
        cp = self._cplan = lib.combat_plan_create()
        if not cp:
            raise CombatHipError("combat_plan_create failed")
        items, names = [], []             # one item per call and per mark; runs of C-ABI calls are joined below
        cindex: Dict[Call, int] = {}      # call -> its index inside the combat_plan
        for call in self.calls:
            captured = False
            if getattr(call.func, "argtypes", None) is not None:       # a ctypes entry point
                ops.check(lib.combat_plan_record(cp, -1 if call.queue is None else call.queue), "combat_plan_record")
                try:
                    rc = call.func(*call.args, None)
                finally:
                    captured = not lib.combat_plan_record_cancel()
                if captured and rc:
                    raise CombatHipError("%s/%s: recording failed (%d)" % (self.name, call.what, rc))
            if captured:
                cindex[call] = len(names)
                names.append(call.what)
                if call.after is not None:
                    ops.check(lib.combat_plan_set_after(cp, cindex[call.after]), "combat_plan_set_after")
                items.append(("c", len(names) - 1, len(names)))
            else:
                assert call.queue is None and call.after is None, "only C-ABI calls can run on an auxiliary queue / wait for a call"
                items.append(("py", call.func, call.args, call.what))
            if call.mark is not None:
                items.append(("mark", call.mark))
        assert lib.combat_plan_size(cp) == len(names)

        def ranges(items):                # neighbouring C-ABI calls become one foreign call (no all-reduce callback: the marks drop out first)
            out = []
            for it in items:
                if it[0] == "c" and out and out[-1][0] == "c":
                    out[-1] = ("c", out[-1][1], it[2])
                else:
                    out.append(it)
            return out

        self._prog, self._prog_nomark, self._cnames = ranges(items), ranges([it for it in items if it[0] != "mark"]), names
        self._has_aux = any(c.queue is not None for c in self.calls)
        return self._prog

    def run(self, prof: Optional[list] = None, on_mark=None) -> None:
        """Replay.  The launch list is walked in C (combat_plan_run: one foreign call per plan, or per range between
        two all-reduce marks / Python hand-offs), with the auxiliary-queue hand-off events created once per plan.
        `prof` (a list) selects the Python replay with per-launch HIP-event bracketing instead (`_run_py`).
        `on_mark(offset)` is called right after the call that completes the gradients above `offset`
        has been enqueued (data-parallel bucketed all-reduce overlapping the rest of the backward)."""
        if prof is not None or not Plan.compiled:
            return self._run_py(prof, on_mark)
        prog = self._program()
        if on_mark is None:
            prog = self._prog_nomark
        stream = torch.cuda.current_stream()
        st = stream.cuda_stream
        n_aux = self.aux_queues if (self._has_aux and not Plan.serial) else 0
        auxp = _aux_pointers(stream, n_aux) if n_aux else None
        cp = self._cplan
        for it in prog:
            kind = it[0]
            if kind == "c":
                rc = lib.combat_plan_run(cp, it[1], it[2], st, auxp, n_aux)
                if rc:
                    what = self._cnames[lib.combat_plan_failed_call(cp)]
                    kindname = {-1: "invalid shape/argument", -2: "HIP launch failed"}.get(rc, "status %d" % rc)
                    raise CombatHipError("%s/%s: %s" % (self.name, what, kindname))
            elif kind == "py":
                rc = it[1](*it[2], st)
                if rc:
                    raise CombatHipError("%s/%s: status %d" % (self.name, it[3], rc))
            else:
                if n_aux:   # the gradients above the mark include auxiliary-stream results
                    ops.check(lib.combat_plan_join(cp, st, auxp, n_aux), "combat_plan_join")
                on_mark(it[1])
        if n_aux:           # join: whoever runs after the plan sees every result
            ops.check(lib.combat_plan_join(cp, st, auxp, n_aux), "combat_plan_join")

    def __del__(self):
        try:
            if self._cplan:
                lib.combat_plan_destroy(self._cplan)
        except Exception:
            pass

    def _run_py(self, prof: Optional[list] = None, on_mark=None) -> None:
        """Replay from Python, one foreign call per launch (the instrumented form).  `prof` (a list) switches on per-launch HIP-event bracketing of the convolution and
        weight-gradient launches on the launch stream: it receives (plan/what, ConvArgs | WgradArgs,
        start_event, end_event).
        `on_mark(offset)` is called right after the call that completes the gradients above `offset`
        has been enqueued (data-parallel bucketed all-reduce overlapping the rest of the backward)."""
        stream = torch.cuda.current_stream()
        st = stream.cuda_stream
        auxs = []
        if any(c.queue is not None for c in self.calls) and not Plan.serial:
            auxs = [_aux_stream(stream, k) for k in range(self.aux_queues)]
        used = set()
        awaited = {c.after for c in self.calls if c.after is not None} if auxs else set()
        done: Dict[Call, torch.cuda.Event] = {}
        for call in self.calls:
            cfunc, args, what = call.func, call.args, call.what
            own = auxs[call.queue] if auxs and call.queue is not None else stream     # the queue this call belongs to
            if call.after in done:
                own.wait_event(done[call.after])
            if prof is not None and cfunc is lib.combat_conv_gemm_pair:     # measured one kernel at a time
                rc = 0
                for sub, arg in zip(what.split("+"), args):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    rc = rc or lib.combat_conv_gemm(arg, st)
                    e1.record(stream)
                    prof.append((self.name + "/" + sub, arg._obj, e0, e1))
            elif prof is not None and cfunc is lib.combat_conv_wgrad_group:   # its members' single launches, one at a time
                rc = 0
                for sub, arg in zip(what.split("+"), args[0]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    rc = rc or lib.combat_conv_wgrad(arg, st)
                    e1.record(stream)
                    prof.append((self.name + "/" + sub, arg.contents, e0, e1))
            elif prof is not None and (cfunc is lib.combat_conv_gemm or cfunc is lib.combat_conv_wgrad or
                                       cfunc is lib.combat_conv_wgrad_reduce):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = cfunc(*args, st)
                e1.record(stream)
                prof.append((self.name + "/" + what, args[0]._obj, e0, e1))
            elif own is not stream:
                # everything enqueued so far (the producers of this call's operands) happens-before it
                own.wait_stream(stream)
                rc = cfunc(*args, own.cuda_stream)
                used.add(call.queue)
            else:
                rc = cfunc(*args, st)
            if rc:
                kind = {-1: "invalid shape/argument", -2: "HIP launch failed"}.get(rc, "status %d" % rc)
                raise CombatHipError("%s/%s: %s" % (self.name, what, kind))
            if call in awaited:
                done[call] = torch.cuda.Event()
                done[call].record(own)
            if on_mark is not None and call.mark is not None:
                for q in used:   # the gradients above the mark include auxiliary-stream results
                    stream.wait_stream(auxs[q])
                on_mark(call.mark)
        for q in used:           # join: whoever runs after the plan sees every result
            stream.wait_stream(auxs[q])

    def __len__(self):
        return len(self.calls)


_AUX_STREAMS: Dict = {}
_AUX_POINTERS: Dict = {}


class PlanSeq:
    """Plans run one after the other as one pass (the two halves of a two_loss pass)."""

    def __init__(self, name: str, plans):
        self.name, self.plans = name, list(plans)

    @property
    def calls(self):
        return [c for p in self.plans for c in p.calls]

    def run(self, prof: Optional[list] = None, on_mark=None) -> None:
        for p in self.plans:
            p.run(prof, on_mark=on_mark)

    def __len__(self):
        return sum(len(p) for p in self.plans)


def _aux_pointers(parent: torch.cuda.Stream, n: int):
    """void*[n] of the parent stream's auxiliary streams, for combat_plan_run (built once per parent stream)."""
    key = (parent.device, parent.cuda_stream, n)
    arr = _AUX_POINTERS.get(key)
    if arr is None:
        arr = (ctypes.c_void_p * n)(*[_aux_stream(parent, k).cuda_stream for k in range(n)])
        _AUX_POINTERS[key] = arr
    return arr


def _aux_stream(parent: torch.cuda.Stream, k: int = 0) -> torch.cuda.Stream:
    """The auxiliary stream of the stream a plan runs on, for calls marked aux (weight gradients beside
    the input-gradient chain).  Per parent stream: two chains that run concurrently must not order each
    other through a shared auxiliary queue.  (Tried and dropped: a second auxiliary stream for the
    shortcut convolutions with a join in front of their consumer -- each cross-stream wait costs the
    critical path more than the 15 us convolution it hides: 5.63 -> 5.93 ms/step.)"""
    key = (parent.device, parent.cuda_stream, k)
    s = _AUX_STREAMS.get(key)
    if s is None:
        s = torch.cuda.Stream(device=parent.device)
        _AUX_STREAMS[key] = s
    return s


class Slot:
    """Named device buffers of one forward(+backward) instance at a fixed batch size."""

    def __init__(self, device, n: int, hw: int):
        self.device, self.N, self.hw = device, n, hw
        self.bufs: Dict[str, torch.Tensor] = {}
        self.norm: Dict[str, "NormState"] = {}
        self.plans: Dict[str, Plan] = {}

    def half_view(self, lo: int, n: int, share: Tuple[str, ...]) -> "Slot":
        """A slot over images [lo, lo+n) of this one: the named buffers are views (batch-major
        layouts make any image range contiguous), everything else is allocated on demand.  Used to run
        the backward of only the triggered half of a merged eval forward."""
        s = Slot(self.device, n, self.hw)
        for k in share:
            if k in self.bufs:
                s.bufs[k] = self.bufs[k][lo:lo + n]
        s.feat_hw = getattr(self, "feat_hw", None)
        return s

    def buf(self, name: str, shape, dtype=bf16, zero: bool = False) -> torch.Tensor:
        t = self.bufs.get(name)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=self.device)
            self.bufs[name] = t
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, (name, t.shape, shape)
        return t


class NormState:
    """Statistics of one normalised tensor: per-channel (groups=1) or per-(image, channel)."""

    def __init__(self, slot: Slot, key: str, groups: int, c: int):
        mk = lambda s: slot.buf("%s.%s" % (key, s), (groups, c), f32)
        self.groups, self.C = groups, c
        self.mean, self.rstd, self.scale, self.shift = mk("mean"), mk("rstd"), mk("scale"), mk("shift")
        self.pending = self.bpending = None    # statistics waiting for their fused finalize+apply launch
        self._slot, self._key = slot, key


class FlatParams:
    """All parameters of a module re-homed into one fp32 buffer, with same-layout gradient and
    momentum buffers.  Conv weights are stored [K][R][S][C] (the module keeps seeing them as OIHW
    tensors with channels_last strides), so the wgrad kernel writes gradients in place, SGD is one
    launch and the data-parallel all-reduce is one flat tensor (bucketed by offset ranges)."""

    ALIGN = 64  # floats

    def __init__(self, module: torch.nn.Module):
        params = list(module.named_parameters())
        dev = params[0][1].device
        self.offsets: Dict[str, Tuple[int, int, tuple]] = {}
        off = 0
        for name, p in params:
            self.offsets[name] = (off, p.numel(), tuple(p.shape))
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.total = off
        self.flat = torch.zeros(off, dtype=f32, device=dev)
        self.grad = torch.zeros(off, dtype=f32, device=dev)
        self.mom = torch.zeros(off, dtype=f32, device=dev)
        with torch.no_grad():
            for name, p in params:
                o, n, shape = self.offsets[name]
                dst = self.flat[o:o + n]
                if p.dim() == 4:
                    k, c, r, s = shape
                    dst.copy_(p.detach().permute(0, 2, 3, 1).reshape(-1))
                    p.data = dst.view(k, r, s, c).permute(0, 3, 1, 2)
                else:
                    dst.copy_(p.detach().reshape(-1))
                    p.data = dst.view(shape)
        self.sgd_ptrs = torch.tensor([[self.flat.data_ptr(), self.grad.data_ptr(), self.mom.data_ptr()]],
                                     dtype=torch.int64, device=dev)
        self.sgd_sizes = torch.tensor([self.total], dtype=torch.int64, device=dev)

    def _slice(self, base: torch.Tensor, name: str) -> torch.Tensor:
        o, n, _ = self.offsets[name]
        return base[o:o + n]

    def grad_phys(self, name: str) -> torch.Tensor:
        """Gradient in the kernel's physical layout ([K][taps][C] for conv weights)."""
        o, n, shape = self.offsets[name]
        g = self.grad[o:o + n]
        if len(shape) == 4:
            k, c, r, s = shape
            return g.view(k, r * s, c)
        return g.view(shape)

    def logical(self, base: torch.Tensor, name: str) -> torch.Tensor:
        """`base` (grad / momentum) slice viewed with the parameter's logical shape."""
        o, n, shape = self.offsets[name]
        g = base[o:o + n]
        if len(shape) == 4:
            k, c, r, s = shape
            return g.view(k, r, s, c).permute(0, 3, 1, 2)
        return g.view(shape)

    zero_ev = None   # set while an early zeroing of `grad` is in flight on the auxiliary stream

    def zero_grad_behind(self) -> None:
        """Call right after the optimiser consumed the gradients: the buffer is zeroed on the auxiliary stream
        now, instead of by the first call of the next backward plan on the critical queue (9 us + a launch
        gap per network and step).  The plan's `zero_grad` entry then only waits for the event."""
        if Plan.serial:
            return
        main = torch.cuda.current_stream()
        aux = _aux_stream(main)
        ev = torch.cuda.Event()
        ev.record(main)
        aux.wait_event(ev)
        ops.check(lib.combat_memset_zero(self.grad.data_ptr(), self.total * 4, aux.cuda_stream), "zero_grad")
        self.zero_ev = torch.cuda.Event()
        self.zero_ev.record(aux)

    def sgd_step(self, lr: float, momentum: float = 0.9, weight_decay: float = 5e-4, grad_scale: float = 1.0):
        """torch.optim.SGD(nesterov=True) on the whole buffer: the momentum buffer starts at zero,
        so `buf = mu*buf + g` equals torch's first-step `buf = g`."""
        ops.sgd_nesterov(self.sgd_ptrs, self.sgd_sizes, 1, self.total, lr, momentum, weight_decay, grad_scale, False)


# --------------------------------------------------------------------------------------------
# recording helpers
# --------------------------------------------------------------------------------------------


def _zero_grad_call(fp, st):
    """First call of a backward plan: zero the flat gradient buffer -- or, if FlatParams.zero_grad_behind()
    already did that behind the previous optimiser step, just order this stream after it."""
    ev = fp.zero_ev
    if ev is not None:
        fp.zero_ev = None
        torch.cuda.current_stream().wait_event(ev)
        return 0
    return lib.combat_memset_zero(fp.grad.data_ptr(), fp.total * 4, st)


_SHORT_WORKGROUPS = False


class short_workgroups:
    """Plans recorded inside this context keep to one tile per workgroup: the weight-stationary persistent kernel
    (COMBAT_TILE_S128x64) is replaced by the ring kernel on the same tiles.  For passes that run BESIDE the critical
    queue: a persistent workgroup holds its CU (and 141 KB of its LDS) for 4-8 tiles, 17-34 us at 128-256 images, and
    the critical queue's launches wait for CUs that long."""

    def __enter__(self):
        global _SHORT_WORKGROUPS
        self.prev, _SHORT_WORKGROUPS = _SHORT_WORKGROUPS, True

    def __exit__(self, *exc):
        global _SHORT_WORKGROUPS
        _SHORT_WORKGROUPS = self.prev


def _tile_preference(a) -> None:
    if _SHORT_WORKGROUPS and a.tile == 0 and lib.combat_conv_pick_tile(ctypes.byref(a)) == TILE_S128x64:
        a.tile = TILE_D128x64


FUSE_SHORTCUT = os.environ.get("COMBAT_NO_FUSED_SHORTCUT", "0") != "1"


def fuse_shortcut(dy, dx, pc: PackedConv, dy_sc, pc_sc: PackedConv):
    """The `shortcut=` argument of the block's first convolution's input gradient (dy -> dx through `pc`, 3x3 / stride
    2) if the 1x1 / stride-2 shortcut's input gradient (dy_sc through `pc_sc`) can ride along as a second reduction
    source (combat_conv_args.src2: one launch, no intermediate tensor), else None (two launches)."""
    if FUSE_SHORTCUT and not Plan.serial_shortcuts and ops.shortcut_fusable(dy, dx, pc, pc_sc) and tuple(dy_sc.shape) == tuple(dy.shape):
        return (dy_sc, pc_sc)
    return None


def rec_conv(plan: Plan, what: str, src, dst, pc: PackedConv, mode: int, **kw):
    a = ops.conv_args(src, dst, pc, mode, workspace=plan.workspace(src.device), **kw)
    _tile_preference(a)
    plan.hold(a)
    plan.add(what, lib.combat_conv_gemm, ctypes.byref(a))
    return a


def rec_wgrad(plan: Plan, what: str, src, dy, pc: PackedConv, dw, pro: Optional[Affine] = None, aux: bool = True):
    """aux=False: the LAST weight gradient of a backward pass stays on the plan's own stream, beside the
    second-to-last one on the auxiliary stream (nothing is left to hide it behind)."""
    a = ops.WgradArgs()
    a.N, a.H, a.W, a.C = src.shape
    _, a.P, a.Q, a.K = dy.shape
    a.R = a.S = pc.R
    a.stride, a.pad = pc.stride, pc.pad
    a.src, a.dy, a.dw, a.k_real, a.c_real = src.data_ptr(), dy.data_ptr(), dw.data_ptr(), pc.K, pc.c_real
    if pro is not None:
        a.pro_scale, a.pro_shift = _p(pro.scale), _p(pro.shift)
        a.pro_group_stride, a.pro_act, a.pro_slope = pro.group_stride, int(pro.act), pro.slope
    a.split = 0
    queue = plan.next_aux_queue() if aux else -1
    ws = _wgrad_workspace(src.device, queue)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    plan.hold(a, src, dy, dw, pro, ws)
    plan.add(what, lib.combat_conv_wgrad, ctypes.byref(a), aux=aux).wgrad = a


def set_deterministic(on: bool) -> None:
    """Process-wide deterministic mode of the kernel library (include/combat_hip.h, combat_set_deterministic; default:
    COMBAT_DETERMINISTIC=1 in the environment): every parameter-gradient reduction and the augmentation adjoint in
    a fixed summation order, so two runs on the same inputs and draws give bit-identical parameters.  The launches
    read the switch when they run, so recorded plans follow it; weight-gradient calls always carry the per-queue
    workspace the ordered reductions need."""
    lib.combat_set_deterministic(1 if on else 0)


def deterministic() -> bool:
    return bool(lib.combat_get_deterministic())


_WGRAD_GROUP_WS: Dict = {}


def _wgrad_group_workspace(device, queue: int, need: int) -> torch.Tensor:
    """The n slab regions of a queue's grouped weight gradients, sized from combat_conv_wgrad_group_workspace_bytes
    (four members of 18.9 MB do not fit the 48 MB of _wgrad_workspace).  Per queue, like that one: the launches of a
    queue run one after the other.  A plan holds the tensor it was built with, so growing never frees a region in use."""
    key = (device, int(queue))
    ws = _WGRAD_GROUP_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        _WGRAD_GROUP_WS[key] = ws
    return ws


def group_wgrads(plan: Plan, device) -> None:
    """Post-pass of a backward plan: runs of auxiliary-queue weight gradients of one geometry that the DMA-staged 3x3
    kernel takes (the library decides: combat_conv_wgrad_group_workspace_bytes) become ONE combat_conv_wgrad_group
    call -- one kernel launch of n x 128 workgroups and one reduction launch instead of n of each with a hand-off gap
    between them.  The weight-gradient queue is what both training backward passes wait for at their end, when nothing
    else is left to run beside it.
    A run never crosses an all-reduce mark (the gradients above a mark must be final there) and holds only calls that
    follow each other on their queue.  The group call takes the place of its LAST member, so its hand-off waits for the
    last producer; the earlier members' operands are read later than they used to be, which is safe because they are
    named Slot buffers (activations, 'g.*' gradients) that are written once per pass and never recycled inside a plan.
    Each member keeps its own WgradArgs (plan.wgrads, the profiled replay), whose workspace field the group ignores."""
    mode = Plan.wgrad_groups
    if mode not in ("tail", "pairs", "stages") or Plan.serial:
        return
    cap = 2 if mode == "pairs" else 4
    stage, n = {}, 0      # call -> all-reduce marks before it
    for c in plan.calls:
        stage[c], n = n, n + (c.mark is not None)
    linked = {x for c in plan.calls if c.after is not None for x in (c, c.after)}
    PP = ctypes.POINTER(ops.WgradArgs)

    def query(members):
        arr = (PP * len(members))(*[ctypes.pointer(c.wgrad) for c in members])
        return arr, int(lib.combat_conv_wgrad_group_workspace_bytes(arr, len(members)))

    runs, run = [], []
    for c in (c for c in plan.calls if c.queue is not None):
        ok = c.func is lib.combat_conv_wgrad and c not in linked
        if ok and run and len(run) < cap and run[-1].queue == c.queue and stage[run[0]] == stage[c] and query(run + [c])[1] >= 0:
            run.append(c)
            continue
        if len(run) > 1:
            runs.append(run)
        run = [c] if ok and query([c])[1] >= 0 else []
    if len(run) > 1:
        runs.append(run)
    if mode == "tail":
        runs = runs[-1:]
    elif mode == "pairs":
        runs = [r for r in runs if stage[r[0]] == stage[runs[-1][0]]]
    dropped = set()       # members that leave the list
    for r in runs:
        arr, need = query(r)
        last = r[-1]      # becomes the group call: its place, queue and mark stay
        ws = _wgrad_group_workspace(device, last.queue, need)
        plan.hold(arr, ws)
        last.func, last.args = lib.combat_conv_wgrad_group, (arr, len(r), ws.data_ptr(), ws.numel())
        last.what, last.wgrad = "+".join(c.what for c in r), [c.wgrad for c in r]
        dropped.update(r[:-1])
    assert all(c.mark is None for c in dropped), "an all-reduce mark on a weight-gradient call"
    plan.calls = [c for c in plan.calls if c not in dropped]
    plan._changed()


_WGRAD_WS: Dict = {}


def _wgrad_workspace(device, queue: int = 0) -> torch.Tensor:
    """Scratch for the weight-gradient partial sums (pixel ranges x tiles <= ~256 + tiles slabs of 147 KB; a
    launch that would need more falls back to fp32 atomics by itself).  One buffer per device AND per queue
    the launch is recorded for: launches of one queue run one after the other, but the last weight gradient of
    a backward plan (queue -1) runs on the plan's own stream while its predecessors may still be writing /
    reducing their slabs on an auxiliary stream (queue 0, 1, ...) -- sharing one base pointer between two queues let
    those launches overwrite each other's partial sums."""
    key = (device, int(queue))
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = torch.empty(48 << 20, dtype=torch.uint8, device=device)
        _WGRAD_WS[key] = ws
    return ws


def rec_act(plan: Plan, what: str, src, dst, aff: Affine):
    """dst = lrelu(src * scale + shift) as a tensor (what a convolution prologue with `aff` computes)."""
    c = src.shape[-1]
    rows = src.numel() // c
    group_rows = (src.shape[1] * src.shape[2]) if aff.group_stride else 0
    assert aff.act and aff.group_stride in (0, c)
    plan.hold(src, dst, aff)
    plan.add(what, lib.combat_affine_act, src.data_ptr(), rows, c, _p(aff.scale), _p(aff.shift), group_rows,
             float(aff.slope), dst.data_ptr())


def _pow2_part(pq: int, cap: int = 32) -> int:
    g = 1
    while g * 2 <= cap and pq % (g * 2) == 0:
        g *= 2
    return g


class NetEngine:
    """Shared machinery: parameters, packed operands, scratch, slots."""

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.device = next(module.parameters()).device
        if self.device.type != "cuda":
            raise CombatHipError("combat_amd engines run on the GPU only (module is on %s); there is no CPU path"
                                 % self.device)
        self.fp = FlatParams(module)
        self.convs: List[PackedConv] = []
        self.slots: Dict[Tuple, Slot] = {}
        self._scratch = torch.empty(ops.norm_scratch_bytes(1, 512) // 4, dtype=f32, device=self.device)
        self.weights_dirty = True

    def mark_weights_dirty(self) -> None:
        self.weights_dirty = True

    def slot(self, name: str, n: int, hw: int) -> Slot:
        key = (name, n, hw)
        s = self.slots.get(key)
        if s is None:
            s = Slot(self.device, n, hw)
            self.slots[key] = s
        return s

    def _pc(self, weight, stride, pad, cin_pad, dup=False, need_dgrad=True, row_scale=None) -> PackedConv:
        pc = PackedConv(weight, stride, pad, cin_pad, dup_hilo=dup, need_dgrad=need_dgrad, row_scale=row_scale)
        self.convs.append(pc)
        return pc

    def refresh(self) -> None:
        """Re-derive bf16 operands (and folded eval-BN) after a parameter update: one launch packs every
        convolution of the network (device-side descriptor table, rebuilt if a weight tensor moved)."""
        if not self.weights_dirty:
            return
        self._pack_all()
        self._refresh_extra()
        self.weights_dirty = False

    def _pack_all(self) -> None:
        ptrs = tuple(pc.weight.data_ptr() for pc in self.convs)
        if getattr(self, "_pack_ptrs", None) != ptrs:
            masters = [pc.master() for pc in self.convs]
            if any(m.data_ptr() != q for m, q in zip(masters, ptrs)):   # a weight is not channels_last: no stable view
                self._pack_ptrs = None
                for pc in self.convs:
                    pc.pack()
                return
            from ._lib import PackDesc
            tab = (PackDesc * len(self.convs))()
            for d, pc, m in zip(tab, self.convs, masters):
                pc.fill_desc(d, m)
            self._pack_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
            self._pack_ptrs = ptrs
        ops.check(lib.combat_pack_weights_batch(self._pack_tab.data_ptr(), len(self.convs),
                                                torch.cuda.current_stream().cuda_stream), "combat_pack_weights_batch")

    def _refresh_extra(self) -> None:
        pass

    # ---- normalisation plumbing -----------------------------------------------------------
    FUSED_DIRECT_PX = 1024   # pixels per group the fused norm kernels reduce themselves (kFusedMaxDirect, norm.hip)
    FUSED_MAX_ROWS = 256     # partial rows per group they reduce themselves (kFusedMaxRows); more go through a first stage

    def _norm_scratch(self, plan: Plan, groups: int, c: int, rows: int) -> torch.Tensor:
        """Scratch for a finalize / fused launch over `rows` partial rows per group.  More than FUSED_MAX_ROWS rows
        are first folded into combat_norm_scratch_bytes(groups, c) of it: instance statistics of 112 x 112 and
        224 x 224 maps (392 and 1568 rows per image) at a batch size the engine's default region cannot hold get a
        larger one, kept from then on.  (The launches of one engine run one after the other.)"""
        if rows > self.FUSED_MAX_ROWS and ops.norm_scratch_bytes(groups, c) > self._scratch.numel() * 4:
            self._scratch = torch.empty(ops.norm_scratch_bytes(groups, c) // 4, dtype=f32, device=self.device)
        plan.hold(self._scratch)
        return self._scratch

    def _conv_norm(self, plan: Plan, slot: Slot, key: str, src, dst, pc: PackedConv, *, groups: int,
                   gamma=None, beta=None, running=None, act_dst=None, slope: float = 0.0, defer: bool = False,
                   **conv_kw) -> NormState:
        """conv + statistics of its raw output + finalize.  groups == 1: batch statistics
        (optionally updating running stats); groups == N: instance statistics.
        act_dst: also materialise lrelu(norm(dst), slope) -- finalize and activation are then ONE launch
        (combat_norm_act_fused).  defer: leave the finalize to the consumer's `_norm_act` (the activation
        buffer belongs to the consuming layer)."""
        n, p, q, c = dst.shape
        pq, m = p * q, n * p * q
        a = ops.conv_args(src, dst, pc, 0, workspace=plan.workspace(src.device), **conv_kw)
        a.stats_kind = 1 | (BATCH_STATS_ROWS if groups == 1 else 0)    # (the row layout depends on it)
        _tile_preference(a)      # (after every field the tile choice reads -- the epilogue flavour -- is final)
        rows, rpi = ops.conv_stats_layout(a)
        fused = (groups == 1) or (rpi > 0)
        st = slot.norm.get(key)
        if st is None:
            st = NormState(slot, key, groups, c)
            slot.norm[key] = st
        part = None
        if fused:
            part = slot.buf(key + ".part", (rows, 2, c), f32)
            a.stats = part.data_ptr()
            rpg = rows if groups == 1 else rpi
        else:
            a.stats_kind = 0
        plan.hold(a, part)
        plan.add(key + ".conv", lib.combat_conv_gemm, ctypes.byref(a))
        one_launch = act_dst is not None or defer
        if not fused and not (one_launch and pq <= self.FUSED_DIRECT_PX):
            g = _pow2_part(pq)
            parts = m // g
            part = slot.buf(key + ".part", (parts, 2, c), f32)
            plan.add(key + ".stats", lib.combat_group_stats, dst.data_ptr(), parts, g, c, part.data_ptr())
            rpg = pq // g
        rm = rv = nbt = None
        if running is not None:
            rm, rv, nbt = running
        plan.hold(gamma, beta, rm, rv, nbt)
        if one_launch:
            st.pending = dict(x=dst, part=part, rpg=rpg if part is not None else 0, pxg=m // groups, key=key,
                              gamma=gamma, beta=beta, rm=rm, rv=rv, nbt=nbt)
            if act_dst is not None:
                self._norm_act(plan, st, act_dst, slope)
            return st
        scr = self._norm_scratch(plan, groups, c, rpg)
        plan.add(key + ".finalize", lib.combat_norm_finalize, part.data_ptr(), groups, rpg, c, float(m // groups),
                 1e-5, _p(gamma), _p(beta), st.mean.data_ptr(), st.rstd.data_ptr(), st.scale.data_ptr(),
                 st.shift.data_ptr(), _p(rm), _p(rv), 0.1, _p(nbt), scr.data_ptr(), scr.numel() * 4)
        return st

    def _norm_act(self, plan: Plan, st: NormState, act_dst, slope: float):
        """The deferred finalize of `st` + its activation tensor, one launch."""
        q = st.pending
        st.pending = None
        x = q["x"]
        plan.hold(x, act_dst, q["part"])
        scr = self._norm_scratch(plan, st.groups, st.C, q["rpg"])
        plan.add(q["key"] + ".finact", lib.combat_norm_act_fused, x.data_ptr(), _p(q["part"]), st.groups, q["rpg"],
                 q["pxg"], st.C, 1e-5, float(slope), _p(q["gamma"]), _p(q["beta"]), st.mean.data_ptr(),
                 st.rstd.data_ptr(), st.scale.data_ptr(), st.shift.data_ptr(), _p(q["rm"]), _p(q["rv"]), 0.1,
                 _p(q["nbt"]), scr.data_ptr(), scr.numel() * 4, act_dst.data_ptr())

    def _dgrad_norm(self, plan: Plan, slot: Slot, key: str, dy, dz, pc: PackedConv, x_pre, st: NormState, *,
                    group_stride: int, slope: float, gamma=None, dgamma=None, dbeta=None, add_pre=None, shortcut=None):
        """dgrad whose epilogue applies the activation mask of the conv input (recomputed from the
        saved pre-norm tensor x_pre) and emits the two norm-backward reductions.  The caller's
        `_bwd_apply` turns them into coefficients and applies those in one launch."""
        n, p, q, c = dz.shape
        pq, m = p * q, n * p * q
        groups = st.groups
        mask = Affine(st.scale, st.shift, group_stride, True, slope)
        a = ops.conv_args(dy, dz, pc, 1, add_pre=add_pre, mask_x=x_pre, mask=mask, workspace=plan.workspace(dy.device),
                          shortcut=shortcut)
        a.stats_kind = 2 | (BATCH_STATS_ROWS if groups == 1 else 0)
        a.xh_mean, a.xh_rstd = st.mean.data_ptr(), st.rstd.data_ptr()
        _tile_preference(a)      # (after stats_kind / xh_*: the tile query and the launch must see the same flavour)
        rows, rpi = ops.conv_stats_layout(a)
        fused = (groups == 1) or (rpi > 0)
        part, rpg = None, 0
        if fused:
            part = slot.buf(key + ".bpart", (rows, 2, c), f32)
            a.stats = part.data_ptr()
            rpg = rows if groups == 1 else rpi
        else:
            a.stats_kind, a.xh_mean, a.xh_rstd = 0, None, None
        plan.hold(a, part)
        plan.add(key + ".dgrad", lib.combat_conv_gemm, ctypes.byref(a))
        if not fused and pq > self.FUSED_DIRECT_PX:
            part, rpg = self._stats_bwd(plan, slot, key, dz, x_pre, st)
        st.bpending = dict(part=part, rpg=rpg, gamma=gamma, dgamma=dgamma, dbeta=dbeta)

    def _stats_bwd(self, plan: Plan, slot: Slot, key: str, dz, x_pre, st: NormState):
        n, p, q, c = dz.shape
        pq, m = p * q, n * p * q
        g = _pow2_part(pq if st.groups > 1 else m)
        parts = m // g
        part = slot.buf(key + ".bpart", (parts, 2, c), f32)
        ppi = (pq // g) if st.groups > 1 else 0
        plan.add(key + ".bstats", lib.combat_group_stats_bwd, dz.data_ptr(), x_pre.data_ptr(), parts, g, c, ppi,
                 st.mean.data_ptr(), st.rstd.data_ptr(), part.data_ptr())
        return part, (pq // g if st.groups > 1 else parts)

    def _bwd_apply(self, plan: Plan, slot: Slot, key: str, dz, x_pre, dx, st: NormState, add=None):
        """Norm backward: (sum dz, sum dz*xhat) -> coefficients -> dx = ca*dz + cb*x + cc (+ add), one launch.
        The sums come from the rows `_dgrad_norm` left behind, or (no such rows) from dz / x_pre directly."""
        n, p, q, c = dz.shape
        pq, m = p * q, n * p * q
        pend = getattr(st, "bpending", None) or dict(part=None, rpg=0, gamma=None, dgamma=None, dbeta=None)
        st.bpending = None
        part, rpg = pend["part"], pend["rpg"]
        pxg = m // st.groups
        if part is None and (st.groups == 1 or pq > self.FUSED_DIRECT_PX):
            part, rpg = self._stats_bwd(plan, slot, key, dz, x_pre, st)
        plan.hold(dz, x_pre, dx, add, part, pend["gamma"], pend["dgamma"], pend["dbeta"])
        scr = self._norm_scratch(plan, st.groups, c, rpg)
        plan.add(key + ".bfused", lib.combat_norm_bwd_fused, dz.data_ptr(), x_pre.data_ptr(), _p(add), _p(part),
                 st.groups, rpg, pxg, c, _p(pend["gamma"]), st.mean.data_ptr(), st.rstd.data_ptr(),
                 _p(pend["dgamma"]), _p(pend["dbeta"]), scr.data_ptr(), scr.numel() * 4, dx.data_ptr())


# --------------------------------------------------------------------------------------------
# classifiers
# --------------------------------------------------------------------------------------------


class _BN:
    def __init__(self, eng: "NetEngine", mod: torch.nn.BatchNorm2d, prefix: str):
        self.prefix, self.C = prefix, mod.num_features
        self.gamma, self.beta = mod.weight.data, mod.bias.data
        self.rm, self.rv, self.nbt = mod.running_mean, mod.running_var, mod.num_batches_tracked
        self.escale = torch.empty(self.C, dtype=f32, device=eng.device)
        self.eshift = torch.empty(self.C, dtype=f32, device=eng.device)

    def fold(self):
        ops.bn_eval_fold(self.gamma, self.beta, self.rm, self.rv, self.escale, self.eshift)

    def eval_affine(self) -> Affine:
        return Affine(self.escale, self.eshift, 0, True, 0.0)


class _Blk:
    pass


class PreActEngine(NetEngine):
    """PreActResNet18 (classifier_models/preact_resnet.py): stem conv, 8 pre-activation blocks,
    avg-pool + linear + cross-entropy head."""

    def __init__(self, module):
        super().__init__(module)
        m = module
        self.classes = m.linear.out_features
        self.stem = self._pc(m.conv1.weight.data, 1, 1, 8, dup=True)
        self.blocks: List[_Blk] = []
        self.bns: List[_BN] = []
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(m, "layer%d" % li)):
                e = _Blk()
                e.prefix = "layer%d.%d." % (li, bi)
                e.stride, e.cin, e.planes = blk.stride, blk.conv1.in_channels, blk.conv1.out_channels
                e.bn1, e.bn2 = _BN(self, blk.bn1, e.prefix + "bn1"), _BN(self, blk.bn2, e.prefix + "bn2")
                e.conv1 = self._pc(blk.conv1.weight.data, blk.stride, 1, e.cin)
                e.conv2 = self._pc(blk.conv2.weight.data, 1, 1, e.planes)
                e.sc = self._pc(blk.shortcut[0].weight.data, blk.stride, 0, e.cin) if hasattr(blk, "shortcut") else None
                self.blocks.append(e)
                self.bns += [e.bn1, e.bn2]
        self.lin_w, self.lin_b = m.linear.weight.data, m.linear.bias.data

    def _refresh_extra(self):
        self.fold_bn()

    def fold_bn(self):
        """Parameters or running stats changed: refresh every folded eval scale/shift (one launch)."""
        ptrs = tuple(t.data_ptr() for bn in self.bns for t in (bn.gamma, bn.beta, bn.rm, bn.rv))
        if getattr(self, "_bn_ptrs", None) != ptrs:
            from ._lib import BnDesc
            tab = (BnDesc * len(self.bns))()
            for d, bn in zip(tab, self.bns):
                d.gamma, d.beta, d.running_mean, d.running_var = (t.data_ptr() for t in (bn.gamma, bn.beta, bn.rm, bn.rv))
                d.scale, d.shift, d.C = bn.escale.data_ptr(), bn.eshift.data_ptr(), bn.C
            self._bn_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
            self._bn_ptrs = ptrs
        ops.check(lib.combat_bn_eval_fold_batch(self._bn_tab.data_ptr(), len(self.bns), 1e-5,
                                                torch.cuda.current_stream().cuda_stream), "combat_bn_eval_fold_batch")

    # ---- buffers of the head
    def head_bufs(self, slot: Slot):
        n = slot.N
        return dict(
            logits=slot.buf("logits", (n, self.classes), f32), dlogits=slot.buf("dlogits", (n, self.classes), f32),
            pooled=slot.buf("pooled", (n, self.lin_w.shape[1]), f32), loss=slot.buf("loss", (1,), f32, zero=True),
            correct=slot.buf("correct", (2,), torch.int32, zero=True),
            targets=slot.buf("targets", (n,), torch.int64, zero=True),
            targets2=slot.buf("targets2", (n,), torch.int64, zero=True))

    def input(self, slot: Slot) -> torch.Tensor:
        return slot.buf("x", (slot.N, slot.hw, slot.hw, 8))

    FWD_SHARED = ("stem", "logits", "dlogits", "pooled", "targets", "targets2") + tuple(
        "b%d.%s" % (b, s) for b in range(8) for s in ("y1", "out", "sc", "a1", "act")) + ("stem.act",)

    def forward_plan(self, slot: Slot, train: bool, loss_weight: float = 1.0, with_targets2: bool = False,
                     split_head: bool = False, head_bwd: bool = False, two_loss: bool = False, keep_raw_blocks=()) -> Plan:
        """split_head (eval only): the batch is two independent halves [metric-only images ; images whose
        loss is differentiated]; the head runs once per half with separate loss / counter cells
        (first half -> correct[0] of slot 'loss0/correct0' cells, second half -> the usual ones).
        head_bwd (eval only): the head launch also produces dlogits and the gradient w.r.t. the feature map ('g.feat':
        combat_head_fwd_bwd), for a pass whose backward plan (backward_eval_plan(head_done=True)) follows at once; a
        train-mode pass has no such backward and raises ValueError.
        two_loss (eval only): the batch is two halves whose losses are BOTH differentiated (the input-aware step's
        [aug(bd) ; aug(bd2)], labels targets[:n] / targets[n:]): first half -> the usual cells, second half ->
        'loss1' / 'correct1'; the matching backward is backward_eval_plan(half_weights=...).  Each half runs as the
        n-image plan over views of this slot's input, head and 'g.img' buffers (two_loss_halves): the results are
        those of two separate n-image passes, bit for bit -- a 2n-image plan picks other tile / partition
        parameters and rounds differently.
        keep_raw_blocks (eval only, PreActEngine only): blocks whose raw output 'b%d.out' is written although no identity
        shortcut reads it (Grad-CAM taps it, combat_amd/defenses.py::GradCam); everything else is computed as without."""
        if train and head_bwd:
            raise ValueError("head_bwd: only an eval pass has a backward plan that starts behind the head (backward_eval_plan(head_done=True))")
        keep_raw_blocks = tuple(sorted(set(int(b) for b in keep_raw_blocks)))
        if keep_raw_blocks:
            if type(self) is not PreActEngine or train or two_loss:
                raise ValueError("keep_raw_blocks: only an eval pass of the pre-activation classifier keeps extra raw outputs")
            if keep_raw_blocks[0] < 0 or keep_raw_blocks[-1] >= len(self.blocks):
                raise ValueError("keep_raw_blocks: blocks %s outside 0..%d" % (keep_raw_blocks, len(self.blocks) - 1))
        if two_loss:
            assert not train and not split_head and not with_targets2 and not head_bwd
            key = "fwd.eval.%g.tl" % loss_weight
            if key not in slot.plans:
                halves = self.two_loss_halves(slot)
                slot.plans[key] = PlanSeq("%s.%s" % (type(self).__name__, key),
                                          [self.forward_plan(s, False, loss_weight) for s in halves])
                slot.feat_hw = halves[0].feat_hw
            return slot.plans[key]
        key = "fwd.%s.%g.%d.%d%s" % ("train" if train else "eval", loss_weight, with_targets2, split_head, ".hb" if head_bwd else "")
        if keep_raw_blocks:
            key += ".kr" + ",".join(str(b) for b in keep_raw_blocks)
        if key in slot.plans:
            return slot.plans[key]
        P = Plan("preact." + key)
        n, hw = slot.N, slot.hw
        x = self.input(slot)
        if keep_raw_blocks:
            cur, chw = self._forward_eval_body(P, slot, x, keep_raw_blocks)
        elif not train:
            cur, chw = self._forward_eval_body(P, slot, x)
        else:
            cur, chw = self._forward_train_body(P, slot, x)
        h = self.head_bufs(slot)
        P.hold(h)
        if head_bwd:
            assert not split_head and type(self) is PreActEngine
            d_feat = slot.buf("g.feat", cur.shape)
            P.hold(d_feat)
            P.add("head+bwd", lib.combat_head_fwd_bwd, cur.data_ptr(), n, chw, cur.shape[-1], self.lin_w.data_ptr(),
                  self.lin_b.data_ptr(), self.classes, h["targets"].data_ptr(), loss_weight, h["pooled"].data_ptr(),
                  h["logits"].data_ptr(), h["loss"].data_ptr(), h["correct"].data_ptr(),
                  h["targets2"].data_ptr() if with_targets2 else None,
                  h["correct"][1:].data_ptr() if with_targets2 else None, h["dlogits"].data_ptr(), d_feat.data_ptr())
        elif not split_head:
            P.add("head", lib.combat_head_fwd, cur.data_ptr(), n, chw, cur.shape[-1], self.lin_w.data_ptr(),
                  self.lin_b.data_ptr(), self.classes, h["targets"].data_ptr(), loss_weight, h["pooled"].data_ptr(),
                  h["logits"].data_ptr(), h["loss"].data_ptr(), h["correct"].data_ptr(),
                  h["targets2"].data_ptr() if with_targets2 else None,
                  h["correct"][1:].data_ptr() if with_targets2 else None)
        else:
            assert not train and n % 2 == 0
            m = n // 2
            loss0 = slot.buf("loss0", (1,), f32, zero=True)
            correct0 = slot.buf("correct0", (2,), torch.int32, zero=True)
            views = [cur[:m], cur[m:], h["targets"][:m], h["targets"][m:], h["pooled"][:m], h["pooled"][m:],
                     h["logits"][:m], h["logits"][m:], h["targets2"][m:]]
            P.hold(views, loss0, correct0)
            P.add("head.metric", lib.combat_head_fwd, views[0].data_ptr(), m, chw, cur.shape[-1], self.lin_w.data_ptr(),
                  self.lin_b.data_ptr(), self.classes, views[2].data_ptr(), 1.0, views[4].data_ptr(),
                  views[6].data_ptr(), loss0.data_ptr(), correct0.data_ptr(), None, None)
            P.add("head.loss", lib.combat_head_fwd, views[1].data_ptr(), m, chw, cur.shape[-1], self.lin_w.data_ptr(),
                  self.lin_b.data_ptr(), self.classes, views[3].data_ptr(), loss_weight, views[5].data_ptr(),
                  views[7].data_ptr(), h["loss"].data_ptr(), h["correct"].data_ptr(),
                  views[8].data_ptr() if with_targets2 else None,
                  h["correct"][1:].data_ptr() if with_targets2 else None)
        slot.plans[key] = P
        slot.feat_hw = chw
        return P

    def _forward_train_body(self, P: Plan, slot: Slot, x):
        """Train mode: BatchNorm uses batch statistics, produced by the epilogue of the convolution that
        writes the normalised tensor.  relu(bn(.)) is then materialised once per BatchNorm by its
        combat_norm_act_fused launch ('b%d.a0' = block input through bn1, 'b%d.a1t' = conv1 output through
        bn2): the forward convolutions and the weight-gradient passes that read it need no prologue and take
        their operands by LDS-DMA."""
        n, hw = slot.N, slot.hw
        cur = slot.buf("stem", (n, hw, hw, 64))
        bnk = lambda bn: dict(groups=1, gamma=bn.gamma, beta=bn.beta, running=(bn.rm, bn.rv, bn.nbt))
        a0 = slot.buf("b0.a0", cur.shape)
        self._conv_norm(P, slot, self.blocks[0].bn1.prefix, x, cur, self.stem, act_dst=a0, **bnk(self.blocks[0].bn1))
        chw = hw
        for b, blk in enumerate(self.blocks):
            ohw = chw // blk.stride
            i_sc = len(P.calls)
            if blk.sc is not None:
                resid = slot.buf("b%d.sc" % b, (n, ohw, ohw, blk.planes))
                rec_conv(P, "b%d.sc" % b, a0, resid, blk.sc, 0)
            else:
                resid = cur
            y1 = slot.buf("b%d.y1" % b, (n, ohw, ohw, blk.planes))
            out = slot.buf("b%d.out" % b, (n, ohw, ohw, blk.planes))
            a1 = slot.buf("b%d.a1t" % b, y1.shape)
            self._conv_norm(P, slot, blk.bn2.prefix, a0, y1, blk.conv1, act_dst=a1, **bnk(blk.bn2))
            if blk.sc is not None:      # shortcut + first convolution: one launch (both read a0)
                P.merge_convs(i_sc)
            if b + 1 < len(self.blocks):
                nxt = self.blocks[b + 1].bn1
                a0 = slot.buf("b%d.a0" % (b + 1), out.shape)
                self._conv_norm(P, slot, nxt.prefix, a1, out, blk.conv2, act_dst=a0, add_post=resid, **bnk(nxt))
            else:
                rec_conv(P, "b%d.c2" % b, a1, out, blk.conv2, 0, add_post=resid)
            cur, chw = out, ohw
        return cur, chw

    def _forward_eval_body(self, P: Plan, slot: Slot, x, keep_raw_blocks=()):
        """Eval mode: every BatchNorm is a fixed per-channel affine known before its producer runs, so the
        producing convolution writes relu(bn(.)) itself (second epilogue output) and no convolution
        needs a prologue -- the 3x3 / stride-1 layers then run on the DMA-staged kernel.  Tensors:
        'stem.act' / 'b%d.act' = relu(bn1_next(block output)), 'b%d.a1' = relu(bn2(conv1 output));
        the raw block output ('stem' / 'b%d.out') is kept only where an identity shortcut or the head
        reads it, or the caller names the block in keep_raw_blocks."""
        n, hw = slot.N, slot.hw
        blocks = self.blocks
        raw = slot.buf("stem", (n, hw, hw, 64)) if blocks[0].sc is None else None
        act = slot.buf("stem.act", (n, hw, hw, 64))
        rec_conv(P, "stem", x, raw, self.stem, 0, act_dst=act, act=blocks[0].bn1.eval_affine())
        chw = hw
        for b, blk in enumerate(blocks):
            ohw = chw // blk.stride
            shape = (n, ohw, ohw, blk.planes)
            if blk.sc is not None:
                resid = slot.buf("b%d.sc" % b, shape)
                rec_conv(P, "b%d.sc" % b, act, resid, blk.sc, 0)
            else:
                resid = raw
            a1 = slot.buf("b%d.a1" % b, shape)
            rec_conv(P, "b%d.c1" % b, act, None, blk.conv1, 0, act_dst=a1, act=blk.bn2.eval_affine())
            if blk.sc is not None:
                P.merge_convs(len(P.calls) - 2)
            nxt = blocks[b + 1] if b + 1 < len(blocks) else None
            keep_raw = nxt is None or nxt.sc is None or b in keep_raw_blocks
            out = slot.buf("b%d.out" % b, shape) if keep_raw else None
            if nxt is not None:
                nact = slot.buf("b%d.act" % b, shape)
                rec_conv(P, "b%d.c2" % b, a1, out, blk.conv2, 0, add_post=resid, act_dst=nact, act=nxt.bn1.eval_affine())
            else:
                nact = None
                rec_conv(P, "b%d.c2" % b, a1, out, blk.conv2, 0, add_post=resid)
            raw, act, chw = out, nact, ohw
        return raw, chw

    def _block_io(self, slot: Slot, b: int):
        xin = slot.bufs["stem"] if b == 0 else slot.bufs["b%d.out" % (b - 1)]
        return xin, slot.bufs["b%d.y1" % b], slot.bufs["b%d.out" % b]

    def backward_train_plan(self, slot: Slot, loss_weight: float = 1.0) -> Plan:
        """Backward of a train-mode forward: all parameter gradients (into fp.grad, which the plan
        zeroes first); no input gradient (Phase C never needs it, train_generator.py:220)."""
        key = "bwd.train.%g" % loss_weight
        if key in slot.plans:
            return slot.plans[key]
        P = Plan("preact." + key)
        fp, n = self.fp, slot.N
        h = self.head_bufs(slot)
        P.add("zero_grad", _zero_grad_call, fp)
        feat = slot.bufs["b%d.out" % (len(self.blocks) - 1)]
        d_out = slot.buf("g.feat", feat.shape)
        P.add("head_bwd", lib.combat_head_bwd, h["pooled"].data_ptr(), n, slot.feat_hw, feat.shape[-1],
              self.lin_w.data_ptr(), self.classes, h["logits"].data_ptr(), h["targets"].data_ptr(), loss_weight,
              h["dlogits"].data_ptr(), d_out.data_ptr(), fp.grad_phys("linear.weight").data_ptr(),
              fp.grad_phys("linear.bias").data_ptr())
        for b in reversed(range(len(self.blocks))):
            blk = self.blocks[b]
            xin, y1, _ = self._block_io(slot, b)
            st1, st2 = slot.norm[blk.bn1.prefix], slot.norm[blk.bn2.prefix]
            a0, a1 = slot.bufs["b%d.a0" % b], slot.bufs["b%d.a1t" % b]   # relu(bn1(xin)), relu(bn2(y1)) of the forward
            pre = blk.prefix
            rec_wgrad(P, "b%d.c2.wgrad" % b, a1, d_out, blk.conv2, fp.grad_phys(pre + "conv2.weight"))
            dz2 = slot.buf("g.b%d.dz2" % b, y1.shape)
            self._dgrad_norm(P, slot, "g." + blk.bn2.prefix, d_out, dz2, blk.conv2, y1, st2, group_stride=0,
                             slope=0.0, gamma=blk.bn2.gamma, dgamma=fp.grad_phys(pre + "bn2.weight"),
                             dbeta=fp.grad_phys(pre + "bn2.bias"))
            dy1 = slot.buf("g.b%d.dy1" % b, y1.shape)
            self._bwd_apply(P, slot, "g." + blk.bn2.prefix, dz2, y1, dy1, st2)
            tsc, fused = None, None
            dz1 = slot.buf("g.b%d.dz1" % b, xin.shape)
            if blk.sc is not None:
                rec_wgrad(P, "b%d.sc.wgrad" % b, a0, d_out, blk.sc, fp.grad_phys(pre + "shortcut.0.weight"))
                fused = fuse_shortcut(dy1, dz1, blk.conv1, d_out, blk.sc)    # the shortcut's input gradient rides along below
                if fused is None:
                    tsc = slot.buf("g.b%d.tsc" % b, xin.shape)
                    rec_conv(P, "b%d.sc.dgrad" % b, d_out, tsc, blk.sc, 1)
            rec_wgrad(P, "b%d.c1.wgrad" % b, a0, dy1, blk.conv1, fp.grad_phys(pre + "conv1.weight"))
            self._dgrad_norm(P, slot, "g." + blk.bn1.prefix, dy1, dz1, blk.conv1, xin, st1, group_stride=0,
                             slope=0.0, gamma=blk.bn1.gamma, dgamma=fp.grad_phys(pre + "bn1.weight"),
                             dbeta=fp.grad_phys(pre + "bn1.bias"), add_pre=tsc, shortcut=fused)
            dxin = slot.buf("g.b%d.dx" % b, xin.shape)
            self._bwd_apply(P, slot, "g." + blk.bn1.prefix, dz1, xin, dxin, st1,
                            add=None if blk.sc is not None else d_out)
            d_out = dxin
            if b in (6, 4, 2):   # layer4 / layer3 / layer2 complete: their gradient range can travel
                P.mark(fp.offsets[pre + "bn1.weight"][0])
        rec_wgrad(P, "stem.wgrad", self.input(slot), d_out, self.stem, fp.grad_phys("conv1.weight"), aux=False)
        P.mark(0)
        group_wgrads(P, self.device)
        slot.plans[key] = P
        return P

    def two_loss_halves(self, slot: Slot):
        """The two n-image slots of a two_loss pass over `slot` (2n images): their input, head buffers and 'g.img'
        are views of `slot`'s; the second half's loss / counter cells are `slot`'s 'loss1' / 'correct1'."""
        halves = getattr(slot, "two_loss_halves", None)
        if halves is None:
            assert slot.N % 2 == 0
            m = slot.N // 2
            h, x = self.head_bufs(slot), self.input(slot)
            gimg = slot.buf("g.img", (slot.N, slot.hw, slot.hw, 8))
            cells = ((h["loss"], h["correct"]),
                     (slot.buf("loss1", (1,), f32, zero=True), slot.buf("correct1", (2,), torch.int32, zero=True)))
            halves = []
            for k in range(2):
                s = Slot(slot.device, m, slot.hw)
                for name in ("logits", "dlogits", "pooled", "targets", "targets2"):
                    s.bufs[name] = h[name][k * m:(k + 1) * m]
                s.bufs["x"], s.bufs["g.img"] = x[k * m:(k + 1) * m], gimg[k * m:(k + 1) * m]
                s.bufs["loss"], s.bufs["correct"] = cells[k]
                halves.append(s)
            slot.two_loss_halves = halves
        return halves

    def _two_loss_backward(self, slot: Slot, half_weights) -> PlanSeq:
        key = "bwd.eval.tl%g,%g" % tuple(half_weights)
        if key not in slot.plans:
            slot.plans[key] = PlanSeq("%s.%s" % (type(self).__name__, key),
                                      [self.backward_eval_plan(s, float(w)) for s, w in zip(self.two_loss_halves(slot),
                                                                                            half_weights)])
        return slot.plans[key]

    def backward_eval_plan(self, slot: Slot, loss_weight: float, head_done: bool = False, half_weights=None,
                           stop_before: Optional[int] = None) -> Plan:
        """Backward of an eval-mode forward w.r.t. the input image only (Phase G: the classifier
        and clean-model weight gradients are never consumed, train_generator.py:179,254).
        Result: slot buffer 'g.img' (bf16 NHWC c8, channels 0..2).  head_done: the forward plan was built with
        head_bwd=True -- dlogits and 'g.feat' exist, and the plan records no head launch.
        half_weights (w0, w1): the backward of a two_loss forward -- each half's mean loss with its weight (loss_weight
        is then unused), each half through its n-image plan.
        stop_before b: the plan ends after block b's input-gradient launch and runs no stem dgrad.  Result: 'g.b%d.dx' % b,
        the gradient w.r.t. the RAW output of block b - 1 ('b%d.out' % (b - 1); the stem's for b == 0): that launch applies
        block b's bn1 scale and ReLU mask, adds the shortcut's gradient before the mask and the identity path after it."""
        if half_weights is not None:
            assert not head_done and stop_before is None
            return self._two_loss_backward(slot, half_weights)
        key = "bwd.eval.%g%s" % (loss_weight, ".hd" if head_done else "")
        if stop_before is not None:
            if not 0 <= int(stop_before) < len(self.blocks):
                raise ValueError("stop_before: block %s outside 0..%d" % (stop_before, len(self.blocks) - 1))
            stop_before = int(stop_before)
            key += ".sb%d" % stop_before
        if key in slot.plans:
            return slot.plans[key]
        P = Plan("preact." + key)
        n = slot.N
        h = self.head_bufs(slot)
        feat = slot.bufs["b%d.out" % (len(self.blocks) - 1)]
        d_out = slot.buf("g.feat", feat.shape)
        if not head_done:
            P.add("head_bwd", lib.combat_head_bwd, None, n, slot.feat_hw, feat.shape[-1], self.lin_w.data_ptr(),
                  self.classes, h["logits"].data_ptr(), h["targets"].data_ptr(), loss_weight, h["dlogits"].data_ptr(),
                  d_out.data_ptr(), None, None)
        for b in reversed(range(len(self.blocks))):
            blk = self.blocks[b]
            # activated tensors of the eval forward: the ReLU mask is (act > 0), the BatchNorm scale multiplies
            xact = slot.bufs["stem.act"] if b == 0 else slot.bufs["b%d.act" % (b - 1)]
            a1 = slot.bufs["b%d.a1" % b]
            dy1 = slot.buf("g.b%d.dy1" % b, a1.shape)
            rec_conv(P, "b%d.c2.dgrad" % b, d_out, dy1, blk.conv2, 1, mask_x=a1, mask=blk.bn2.eval_affine(),
                     mask_mul_scale=True, mask_activated=True)
            tsc, fused = None, None
            dxin = slot.buf("g.b%d.dx" % b, xact.shape)
            if blk.sc is not None:
                fused = fuse_shortcut(dy1, dxin, blk.conv1, d_out, blk.sc)
                if fused is None:
                    tsc = slot.buf("g.b%d.tsc" % b, xact.shape)
                    rec_conv(P, "b%d.sc.dgrad" % b, d_out, tsc, blk.sc, 1)
            rec_conv(P, "b%d.c1.dgrad" % b, dy1, dxin, blk.conv1, 1, shortcut=fused, add_pre=tsc, mask_x=xact,
                     mask=blk.bn1.eval_affine(), mask_mul_scale=True, mask_activated=True,
                     add_post=None if blk.sc is not None else d_out)
            d_out = dxin
            if b == stop_before:
                slot.plans[key] = P
                return P
        gimg = slot.buf("g.img", (n, slot.hw, slot.hw, 8))
        rec_conv(P, "stem.dgrad", d_out, gimg, self.stem, 1)
        slot.plans[key] = P
        return P


class ResNetEngine(PreActEngine):
    """ResNet18 (classifier_models/resnet.py:15-37, 68-106; the CelebA classifier): post-activation
    BasicBlocks  out = relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x)),  shortcut = conv1x1 + BatchNorm
    where the shape changes, stem conv + BatchNorm + ReLU, avg_pool2d(4) + Linear.

    A BatchNorm here FOLLOWS its convolution, so
      * eval mode: bn1 / the stem's norm are the producing convolution's activated-output epilogue, as in
        the pre-activation net; bn2 and the shortcut's norm sit in front of the residual sum and are folded
        into the packed weights (row_scale = gamma * rstd, the shift travels as the bias): every block is
        three launches and no tensor is stored raw;
      * train mode: batch statistics from the conv epilogues; bn2 + residual (+ the shortcut's own,
        separately finalised norm) + ReLU are one fused launch (combat_norm_add_act_fused).
    Tensors: 'stem.a' = relu(bn(conv(x))), 'b%d.a1' = relu(bn1(conv1(.))), 'b%d.out' = the block output
    (activated); train only: raw 'stem', 'b%d.y1', 'b%d.y2', 'b%d.ys' for the norm backward passes."""

    def __init__(self, module):
        NetEngine.__init__(self, module)
        m = module
        self.classes = m.linear.out_features
        self.stem = self._pc(m.conv1.weight.data, 1, 1, 8, dup=True)
        self.bn0 = _BN(self, m.bn1, "bn1")
        self.blocks: List[_Blk] = []
        self.bns: List[_BN] = [self.bn0]
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(m, "layer%d" % li)):
                e = _Blk()
                e.prefix = "layer%d.%d." % (li, bi)
                e.stride, e.cin, e.planes = blk.stride, blk.conv1.in_channels, blk.conv1.out_channels
                e.bn1, e.bn2 = _BN(self, blk.bn1, e.prefix + "bn1"), _BN(self, blk.bn2, e.prefix + "bn2")
                e.conv1 = self._pc(blk.conv1.weight.data, blk.stride, 1, e.cin)
                e.conv2 = self._pc(blk.conv2.weight.data, 1, 1, e.planes)
                e.conv2e = self._pc(blk.conv2.weight.data, 1, 1, e.planes, row_scale=e.bn2.escale)
                e.sc = e.sce = e.bns = None
                if len(blk.shortcut):      # (an empty nn.Sequential for identity shortcuts, resnet.py:24)
                    e.bns = _BN(self, blk.shortcut[1], e.prefix + "shortcut.1")
                    e.sc = self._pc(blk.shortcut[0].weight.data, blk.stride, 0, e.cin)
                    e.sce = self._pc(blk.shortcut[0].weight.data, blk.stride, 0, e.cin, row_scale=e.bns.escale)
                    self.bns.append(e.bns)
                self.blocks.append(e)
                self.bns += [e.bn1, e.bn2]
        self.lin_w, self.lin_b = m.linear.weight.data, m.linear.bias.data
        self.ones = torch.ones(512, dtype=f32, device=self.device)
        self.zeros = torch.zeros(512, dtype=f32, device=self.device)

    def refresh(self) -> None:
        """The folded eval operands read the eval scale of their BatchNorm: fold first, then pack."""
        if not self.weights_dirty:
            return
        self.fold_bn()
        self._pack_all()
        self.weights_dirty = False

    FWD_SHARED = ("stem.a", "logits", "dlogits", "pooled", "targets", "targets2") + tuple(
        "b%d.%s" % (b, s) for b in range(8) for s in ("a1", "out", "scv"))

    def _block_in(self, slot: Slot, b: int):
        return slot.bufs["stem.a"] if b == 0 else slot.bufs["b%d.out" % (b - 1)]

    # ---- forward
    def _forward_eval_body(self, P: Plan, slot: Slot, x):
        n, hw = slot.N, slot.hw
        cur = slot.buf("stem.a", (n, hw, hw, 64))
        rec_conv(P, "stem", x, None, self.stem, 0, act_dst=cur, act=self.bn0.eval_affine())
        relu = Affine(self.ones, self.zeros, 0, True, 0.0)
        chw = hw
        for b, blk in enumerate(self.blocks):
            ohw = chw // blk.stride
            shape = (n, ohw, ohw, blk.planes)
            a1 = slot.buf("b%d.a1" % b, shape)
            rec_conv(P, "b%d.c1" % b, cur, None, blk.conv1, 0, act_dst=a1, act=blk.bn1.eval_affine())
            if blk.sc is not None:
                resid = slot.buf("b%d.scv" % b, shape)
                rec_conv(P, "b%d.sc" % b, cur, resid, blk.sce, 0, bias=blk.bns.eshift)
                P.merge_convs(len(P.calls) - 2)
            else:
                resid = cur
            out = slot.buf("b%d.out" % b, shape)
            rec_conv(P, "b%d.c2" % b, a1, None, blk.conv2e, 0, bias=blk.bn2.eshift, add_post=resid, act_dst=out, act=relu)
            cur, chw = out, ohw
        return cur, chw

    def _norm_add_act(self, plan: Plan, st: NormState, act_dst, add, add_scale, add_shift):
        q = st.pending
        st.pending = None
        x = q["x"]
        plan.hold(x, act_dst, q["part"], add, add_scale, add_shift)
        plan.add(q["key"] + ".finaddact", lib.combat_norm_add_act_fused, x.data_ptr(), _p(q["part"]), st.groups, q["rpg"],
                 q["pxg"], st.C, 1e-5, 0.0, _p(q["gamma"]), _p(q["beta"]), st.mean.data_ptr(), st.rstd.data_ptr(),
                 st.scale.data_ptr(), st.shift.data_ptr(), _p(q["rm"]), _p(q["rv"]), 0.1, _p(q["nbt"]),
                 self._scratch.data_ptr(), self._scratch.numel() * 4, add.data_ptr(), _p(add_scale), _p(add_shift),
                 act_dst.data_ptr())

    def _forward_train_body(self, P: Plan, slot: Slot, x):
        n, hw = slot.N, slot.hw
        bnk = lambda bn: dict(gamma=bn.gamma, beta=bn.beta, running=(bn.rm, bn.rv, bn.nbt))
        y0 = slot.buf("stem", (n, hw, hw, 64))
        cur = slot.buf("stem.a", y0.shape)
        self._conv_norm(P, slot, self.bn0.prefix, x, y0, self.stem, groups=1, act_dst=cur, **bnk(self.bn0))
        chw = hw
        for b, blk in enumerate(self.blocks):
            ohw = chw // blk.stride
            shape = (n, ohw, ohw, blk.planes)
            y1, a1 = slot.buf("b%d.y1" % b, shape), slot.buf("b%d.a1" % b, shape)
            self._conv_norm(P, slot, blk.bn1.prefix, cur, y1, blk.conv1, groups=1, act_dst=a1, **bnk(blk.bn1))
            y2 = slot.buf("b%d.y2" % b, shape)
            st2 = self._conv_norm(P, slot, blk.bn2.prefix, a1, y2, blk.conv2, groups=1, defer=True, **bnk(blk.bn2))
            out = slot.buf("b%d.out" % b, shape)
            if blk.sc is not None:
                ys = slot.buf("b%d.ys" % b, shape)
                sts = self._conv_norm(P, slot, blk.bns.prefix, cur, ys, blk.sc, groups=1, **bnk(blk.bns))
                self._norm_add_act(P, st2, out, ys, sts.scale, sts.shift)
            else:
                self._norm_add_act(P, st2, out, cur, None, None)
            cur, chw = out, ohw
        return cur, chw

    # ---- backward
    def _head_grad(self, P: Plan, slot: Slot, loss_weight: float, train: bool):
        """Gradient w.r.t. the last block's output, through its ReLU."""
        fp, n = self.fp, slot.N
        h = self.head_bufs(slot)
        feat = slot.bufs["b%d.out" % (len(self.blocks) - 1)]
        d_feat = slot.buf("g.feat", feat.shape)
        P.add("head_bwd", lib.combat_head_bwd, h["pooled"].data_ptr() if train else None, n, slot.feat_hw, feat.shape[-1],
              self.lin_w.data_ptr(), self.classes, h["logits"].data_ptr(), h["targets"].data_ptr(), loss_weight,
              h["dlogits"].data_ptr(), d_feat.data_ptr(), fp.grad_phys("linear.weight").data_ptr() if train else None,
              fp.grad_phys("linear.bias").data_ptr() if train else None)
        d_out = slot.buf("g.feat.m", feat.shape)
        P.add("head_bwd.relu", lib.combat_relu_mask, d_feat.data_ptr(), feat.data_ptr(), feat.numel(), d_out.data_ptr())
        return d_out

    def backward_train_plan(self, slot: Slot, loss_weight: float = 1.0) -> Plan:
        key = "bwd.train.%g" % loss_weight
        if key in slot.plans:
            return slot.plans[key]
        P = Plan("resnet." + key)
        fp = self.fp
        G = lambda name, like: slot.buf("g." + name, like.shape)
        P.add("zero_grad", _zero_grad_call, fp)
        d_out = self._head_grad(P, slot, loss_weight, True)

        def bn_bwd(bn, key_, dz, x_pre, name):
            """BatchNorm backward of dz w.r.t. the raw tensor x_pre (sums taken from the tensors)."""
            st = slot.norm[bn.prefix]
            st.bpending = dict(part=None, rpg=0, gamma=bn.gamma, dgamma=fp.grad_phys(bn.prefix + ".weight"),
                               dbeta=fp.grad_phys(bn.prefix + ".bias"))
            dx = G(name, x_pre)
            self._bwd_apply(P, slot, key_, dz, x_pre, dx, st)
            return dx

        for b in reversed(range(len(self.blocks))):
            blk, pre = self.blocks[b], self.blocks[b].prefix
            cur_in = self._block_in(slot, b)
            y1, a1, y2 = slot.bufs["b%d.y1" % b], slot.bufs["b%d.a1" % b], slot.bufs["b%d.y2" % b]
            dy2 = bn_bwd(blk.bn2, "g." + blk.bn2.prefix, d_out, y2, "b%d.dy2" % b)
            tsc, dys = None, None
            if blk.sc is not None:
                dys = bn_bwd(blk.bns, "g." + blk.bns.prefix, d_out, slot.bufs["b%d.ys" % b], "b%d.dys" % b)
                rec_wgrad(P, "b%d.sc.wgrad" % b, cur_in, dys, blk.sc, fp.grad_phys(pre + "shortcut.0.weight"))
            rec_wgrad(P, "b%d.c2.wgrad" % b, a1, dy2, blk.conv2, fp.grad_phys(pre + "conv2.weight"))
            st1 = slot.norm[blk.bn1.prefix]
            dz1 = G("b%d.dz1" % b, y1)
            self._dgrad_norm(P, slot, "g." + blk.bn1.prefix, dy2, dz1, blk.conv2, y1, st1, group_stride=0, slope=0.0,
                             gamma=blk.bn1.gamma, dgamma=fp.grad_phys(pre + "bn1.weight"),
                             dbeta=fp.grad_phys(pre + "bn1.bias"))
            dy1 = G("b%d.dy1" % b, y1)
            self._bwd_apply(P, slot, "g." + blk.bn1.prefix, dz1, y1, dy1, st1)
            rec_wgrad(P, "b%d.c1.wgrad" % b, cur_in, dy1, blk.conv1, fp.grad_phys(pre + "conv1.weight"))
            dxin = G("b%d.dx" % b, cur_in) if b > 0 else None
            fused = None
            if blk.sc is not None:       # the shortcut's share of the block-input gradient: along with conv1's, or a launch
                fused = fuse_shortcut(dy1, dxin, blk.conv1, dys, blk.sc) if b > 0 else None
                if fused is None:
                    tsc = G("b%d.tsc" % b, cur_in)
                    rec_conv(P, "b%d.sc.dgrad" % b, dys, tsc, blk.sc, 1)
            other = (None if fused is not None else tsc) if blk.sc is not None else d_out
            if b > 0:   # through the previous block's final ReLU
                rec_conv(P, "b%d.c1.dgrad" % b, dy1, dxin, blk.conv1, 1, shortcut=fused, add_pre=other, mask_x=cur_in,
                         mask_activated=True)
                d_out = dxin
                if b in (6, 4, 2):
                    P.mark(fp.offsets[pre + "conv1.weight"][0])
            else:       # into the stem: ReLU + BatchNorm of the raw stem output
                y0, st0 = slot.bufs["stem"], slot.norm[self.bn0.prefix]
                dz0 = G("stem.dz", y0)
                self._dgrad_norm(P, slot, "g." + self.bn0.prefix, dy1, dz0, blk.conv1, y0, st0, group_stride=0, slope=0.0,
                                 gamma=self.bn0.gamma, dgamma=fp.grad_phys("bn1.weight"), dbeta=fp.grad_phys("bn1.bias"),
                                 add_pre=other)
                dy0 = G("stem.dy", y0)
                self._bwd_apply(P, slot, "g." + self.bn0.prefix, dz0, y0, dy0, st0)
                rec_wgrad(P, "stem.wgrad", self.input(slot), dy0, self.stem, fp.grad_phys("conv1.weight"), aux=False)
        P.mark(0)
        group_wgrads(P, self.device)
        slot.plans[key] = P
        return P

    def backward_eval_plan(self, slot: Slot, loss_weight: float, half_weights=None) -> Plan:
        """Input gradient of an eval-mode forward (result: 'g.img'); masks from the activated tensors, the
        BatchNorm scales from the folded operands (bn2, shortcut) or the mask tables (bn1, stem).
        half_weights: as PreActEngine.backward_eval_plan."""
        if half_weights is not None:
            return self._two_loss_backward(slot, half_weights)
        key = "bwd.eval.%g" % loss_weight
        if key in slot.plans:
            return slot.plans[key]
        P = Plan("resnet." + key)
        n = slot.N
        d_out = self._head_grad(P, slot, loss_weight, False)
        for b in reversed(range(len(self.blocks))):
            blk = self.blocks[b]
            cur_in, a1 = self._block_in(slot, b), slot.bufs["b%d.a1" % b]
            dy1 = slot.buf("g.b%d.dy1" % b, a1.shape)
            rec_conv(P, "b%d.c2.dgrad" % b, d_out, dy1, blk.conv2e, 1, mask_x=a1, mask=blk.bn1.eval_affine(),
                     mask_mul_scale=True, mask_activated=True)
            other, fused = d_out, None
            dxin = slot.buf("g.b%d.dx" % b, cur_in.shape)
            if blk.sc is not None:
                fused = fuse_shortcut(dy1, dxin, blk.conv1, d_out, blk.sce) if b > 0 else None
                other = None
                if fused is None:
                    other = slot.buf("g.b%d.tsc" % b, cur_in.shape)
                    rec_conv(P, "b%d.sc.dgrad" % b, d_out, other, blk.sce, 1)
            if b > 0:
                rec_conv(P, "b%d.c1.dgrad" % b, dy1, dxin, blk.conv1, 1, shortcut=fused, add_pre=other, mask_x=cur_in,
                         mask_activated=True)
            else:
                rec_conv(P, "b%d.c1.dgrad" % b, dy1, dxin, blk.conv1, 1, add_pre=other, mask_x=cur_in,
                         mask=self.bn0.eval_affine(), mask_mul_scale=True, mask_activated=True)
            d_out = dxin
        gimg = slot.buf("g.img", (n, slot.hw, slot.hw, 8))
        rec_conv(P, "stem.dgrad", d_out, gimg, self.stem, 1)
        slot.plans[key] = P
        return P


class VggEngine(NetEngine):
    """VGG13 (classifier_models/vgg.py:18-45) as a VICTIM: train-mode forward + parameter gradients (ClassifierStep) and
    the eval-mode forward.  Five stages of two conv(3x3, bias) -> BatchNorm -> ReLU layers, a 2x2 max-pool behind each
    stage, view + Linear + cross-entropy on the 1 x 1 (32 x 32 inputs) or 2 x 2 (64 x 64) map that is left.

    The convolution bias is the launch's own epilogue term in both modes: the stored tensor and its batch statistics
    include it, so running_mean is mean(conv) + b with no launch added, and an eval pass needs no fold of its own.  Its
    gradient is mathematically zero under a train-mode BatchNorm (the norm's backward output sums to zero per channel):
    no launch writes it and the zeroed gradient buffer keeps exact zeros there.
    Tensors (layer l = 0..9): 'l%d.y' raw conv output (train), 'l%d.a' = relu(bn(.)), 'l%d.p' the pooled tensor behind
    the odd layers.  There is no input-gradient plan: VGG13 as the generator's surrogate is out of scope."""

    def __init__(self, module):
        if getattr(module, "vgg_name", None) != "VGG13":
            raise NotImplementedError("only VGG13 of the VGG table has a HIP engine, not %r" % getattr(module, "vgg_name", None))
        super().__init__(module)
        m = module
        self.classes = m.classifier.out_features
        self.layers: List[_Blk] = []
        self.bns: List[_BN] = []
        idx, cin = 0, 8
        for widths in ((64, 64), (128, 128), (256, 256), (512, 512), (512, 512)):
            for j, width in enumerate(widths):
                conv, bn = m.features[idx], m.features[idx + 1]
                assert conv.out_channels == width and isinstance(bn, torch.nn.BatchNorm2d)
                e = _Blk()
                e.prefix, e.width, e.pool = "features.%d" % idx, width, j == len(widths) - 1
                e.pc = self._pc(conv.weight.data, 1, 1, cin, dup=not self.layers, need_dgrad=bool(self.layers))
                e.bias = conv.bias.data
                e.bn = _BN(self, bn, "features.%d" % (idx + 1))
                self.layers.append(e)
                self.bns.append(e.bn)
                idx, cin = idx + 3, width
            idx += 1     # the stage's MaxPool2d
        self.lin_w, self.lin_b = m.classifier.weight.data, m.classifier.bias.data

    fold_bn = PreActEngine.fold_bn
    input = PreActEngine.input
    head_bufs = PreActEngine.head_bufs

    def _refresh_extra(self):
        self.fold_bn()

    def forward_plan(self, slot: Slot, train: bool, loss_weight: float = 1.0, with_targets2: bool = False,
                     split_head: bool = False, head_bwd: bool = False, two_loss: bool = False, keep_raw_blocks=()) -> Plan:
        """PreActEngine.forward_plan's argument list, so that a step written for the surrogates gets a message and not a
        TypeError: every form beyond the plain pass belongs to a generator step or a defense and is refused."""
        if with_targets2 or split_head or head_bwd or two_loss or tuple(keep_raw_blocks):
            raise NotImplementedError("VGG13 is victim-only on the HIP path: its forward plan has no second-label counter, "
                                      "split / two-loss head, head gradient or raw taps (DESIGN.md section 16)")
        key = "fwd.%s.%g" % ("train" if train else "eval", loss_weight)
        if key in slot.plans:
            return slot.plans[key]
        P = Plan("vgg." + key)
        n, s = slot.N, slot.hw
        cur = self.input(slot)
        for li, e in enumerate(self.layers):
            act = slot.buf("l%d.a" % li, (n, s, s, e.width))
            if train:
                y = slot.buf("l%d.y" % li, act.shape)
                self._conv_norm(P, slot, e.bn.prefix, cur, y, e.pc, groups=1, gamma=e.bn.gamma, beta=e.bn.beta,
                                running=(e.bn.rm, e.bn.rv, e.bn.nbt), act_dst=act, bias=e.bias)
            else:
                rec_conv(P, "l%d" % li, cur, None, e.pc, 0, bias=e.bias, act_dst=act, act=e.bn.eval_affine())
            cur = act
            if e.pool:
                pooled = slot.buf("l%d.p" % li, (n, s // 2, s // 2, e.width))
                P.hold(cur, pooled)
                P.add("l%d.pool" % li, lib.combat_maxpool2, cur.data_ptr(), n, s, s, e.width, pooled.data_ptr())
                cur, s = pooled, s // 2
        h = self.head_bufs(slot)
        P.hold(h, cur)
        P.add("head", lib.combat_flat_head_fwd, cur.data_ptr(), n, s, cur.shape[-1], self.lin_w.data_ptr(),
              self.lin_b.data_ptr(), self.classes, h["targets"].data_ptr(), loss_weight, h["logits"].data_ptr(),
              h["dlogits"].data_ptr(), h["loss"].data_ptr(), h["correct"].data_ptr())
        slot.plans[key] = P
        slot.feat_hw = s
        return P

    def backward_train_plan(self, slot: Slot, loss_weight: float = 1.0) -> Plan:
        """Backward of a train-mode forward_plan(slot, True, loss_weight) (whose head launch left dlogits): every
        parameter gradient into fp.grad, which the plan zeroes first; no image gradient."""
        key = "bwd.train.%g" % loss_weight
        if key in slot.plans:
            return slot.plans[key]
        if "fwd.train.%g" % loss_weight not in slot.plans:    # the loss weight lives in that forward's dlogits
            raise ValueError("backward_train_plan(loss_weight=%g) needs forward_plan(slot, True, %g) of the same slot first"
                             % (loss_weight, loss_weight))
        P = Plan("vgg." + key)
        fp, n = self.fp, slot.N
        h = self.head_bufs(slot)
        G = lambda name, like: slot.buf("g." + name, like.shape)
        P.add("zero_grad", _zero_grad_call, fp)
        feat = slot.bufs["l%d.p" % (len(self.layers) - 1)]
        d_cur = G("feat", feat)
        P.hold(h, feat, d_cur)
        P.add("head_bwd", lib.combat_flat_head_bwd, feat.data_ptr(), n, slot.feat_hw, feat.shape[-1], self.lin_w.data_ptr(),
              self.classes, h["dlogits"].data_ptr(), d_cur.data_ptr(), fp.grad_phys("classifier.weight").data_ptr(),
              fp.grad_phys("classifier.bias").data_ptr())
        bnk = lambda bn: dict(gamma=bn.gamma, dgamma=fp.grad_phys(bn.prefix + ".weight"), dbeta=fp.grad_phys(bn.prefix + ".bias"))
        for l1 in range(len(self.layers) - 1, 0, -2):
            l0 = l1 - 1
            e0, e1 = self.layers[l0], self.layers[l1]
            y0, a0, y1, a1 = (slot.bufs["l%d.%s" % (l, t)] for l in (l0, l1) for t in ("y", "a"))
            st0, st1 = slot.norm[e0.bn.prefix], slot.norm[e1.bn.prefix]
            # through the pool and the second layer's ReLU, then its BatchNorm (sums taken from the tensors)
            dz1 = G("l%d.dz" % l1, y1)
            P.hold(a1, d_cur, dz1)
            P.add("l%d.pool_bwd" % l1, lib.combat_maxpool2_relu_bwd, a1.data_ptr(), d_cur.data_ptr(), n, a1.shape[1],
                  a1.shape[2], e1.width, dz1.data_ptr())
            st1.bpending = dict(part=None, rpg=0, **bnk(e1.bn))
            dy1 = G("l%d.dy" % l1, y1)
            self._bwd_apply(P, slot, "g." + e1.bn.prefix, dz1, y1, dy1, st1)
            rec_wgrad(P, "l%d.wgrad" % l1, a0, dy1, e1.pc, fp.grad_phys(e1.prefix + ".weight"))
            # into the first layer: ReLU mask + BatchNorm sums in the input gradient's epilogue
            dz0 = G("l%d.dz" % l0, y0)
            self._dgrad_norm(P, slot, "g." + e0.bn.prefix, dy1, dz0, e1.pc, y0, st0, group_stride=0, slope=0.0, **bnk(e0.bn))
            dy0 = G("l%d.dy" % l0, y0)
            self._bwd_apply(P, slot, "g." + e0.bn.prefix, dz0, y0, dy0, st0)
            src0 = slot.bufs["l%d.p" % (l0 - 1)] if l0 else self.input(slot)
            rec_wgrad(P, "l%d.wgrad" % l0, src0, dy0, e0.pc, fp.grad_phys(e0.prefix + ".weight"), aux=l0 > 0)
            if l0:      # to the previous stage's pooled tensor (the first layer has no image gradient)
                d_cur = G("l%d.dp" % (l0 - 1), src0)
                rec_conv(P, "l%d.dgrad" % l0, dy0, d_cur, e0.pc, 1)
                if l0 in (8, 6, 4):   # stages 5 / 4 / 3 complete: their gradient range can travel
                    P.mark(fp.offsets[e0.prefix + ".weight"][0])
        P.mark(0)
        group_wgrads(P, self.device)
        slot.plans[key] = P
        return P

    def backward_eval_plan(self, *a, **k):
        raise NotImplementedError("VGG13 is victim-only on the HIP path: there is no eval-mode input gradient, so it cannot "
                                  "be the surrogate of a generator step (DESIGN.md section 16)")


# --------------------------------------------------------------------------------------------
# UNet generator
# --------------------------------------------------------------------------------------------


class UnetEngine(NetEngine):
    """UnetGenerator (networks/models.py:268-341).  Tensors: t[name] = raw conv outputs,
    up[level] = LeakyReLU(bilinear_up(...)) decoder inputs; InstanceNorm + LeakyReLU live in the
    prologue of the consuming convolution."""

    LR = 0.2

    def __init__(self, module):
        super().__init__(module)
        m = module
        self.nf = m.nf
        self.pc: Dict[str, PackedConv] = {}
        self.bias: Dict[str, torch.Tensor] = {}
        for name, ci, co, stride, _ in UNET_LAYERS:
            conv = getattr(m, name)
            weight, cin = self._conv_operand(name, conv)
            cin_pad = 8 if ci == 0 else cin
            self.pc[name] = self._pc(weight, stride, 1, cin_pad, dup=(ci == 0), need_dgrad=(ci != 0))
            self.bias[name] = conv.bias.data if conv.bias is not None else None
        self.out_bias8 = torch.zeros(8, dtype=f32, device=self.device)
        self.ones = torch.ones(64 * 8, dtype=f32, device=self.device)
        self.zeros = torch.zeros(64 * 8, dtype=f32, device=self.device)

    def _conv_operand(self, name: str, conv):
        """(fp32 master weight, input channels) the packed operand of layer `name` is built from."""
        return conv.weight.data, conv.in_channels

    def _cond_forward(self, P: Plan, slot: Slot, s: int) -> dict:
        """Extra arguments of conv0_1's forward launch (CUnetEngine: the label term); records what produces them."""
        return {}

    def _conv0_1_wgrad(self, P: Plan, slot: Slot, d) -> None:
        """The weight gradient of conv0_1 from d, the gradient w.r.t. its raw output."""
        rec_wgrad(P, "conv0_1.wgrad", slot.bufs["a.conv0_1"], d, self.pc["conv0_1"], self.fp.grad_phys("conv0_1.weight"))

    def _refresh_extra(self):
        if self.bias8_taken:          # the caller copied it with its own small copies (small_refresh_copy)
            self.bias8_taken = False
            return
        b = self.bias["upconv0_0"]
        if b is not None:
            self.out_bias8[: b.numel()].copy_(b)

    bias8_taken = False

    def small_refresh_copy(self):
        """(dst pointer, src pointer, bytes) of the one small copy the next refresh() would issue by itself (the output
        layer's bias into its 8-channel form), for a caller that batches it with copies of its own (combat_copy3) --
        or None if the operands are current.  The next refresh() then skips it."""
        b = self.bias["upconv0_0"]
        if not self.weights_dirty or b is None:
            return None
        self.bias8_taken = True
        return self.out_bias8.data_ptr(), b.data_ptr(), 4 * b.numel()

    def input(self, slot: Slot) -> torch.Tensor:
        return slot.buf("x", (slot.N, slot.hw, slot.hw, 8))

    def output(self, slot: Slot) -> torch.Tensor:
        return slot.buf("noise", (slot.N, slot.hw, slot.hw, 8))

    def _in_aff(self, st: NormState) -> Affine:
        return Affine(st.scale, st.shift, st.C, True, self.LR)

    def forward_plan(self, slot: Slot) -> Plan:
        if "fwd" in slot.plans:
            return slot.plans["fwd"]
        P = Plan("unet.fwd")
        n, hw, nf = slot.N, slot.hw, self.nf
        T = lambda name, s, c: slot.buf("t." + name, (n, s, s, c))
        x = self.input(slot)
        h1, h2, h3, h4 = hw // 2, hw // 4, hw // 8, hw // 16
        pc, bs = self.pc, self.bias
        t00 = T("conv0_0", h1, nf)
        # conv0_1 reads LeakyReLU(conv0_0 output), no norm in between: the activation is conv0_0's second output
        a01 = slot.buf("a.conv0_1", t00.shape)
        rec_conv(P, "conv0_0", x, t00, pc["conv0_0"], 0, bias=bs["conv0_0"], act_dst=a01,
                 act=Affine(self.ones, self.zeros, 0, True, self.LR))

        def cn(name, src, s, c, pro, defer=False, **conv_kw):
            # pro: None (src is used as is), an Affine (activation only), or the NormState of src whose
            # finalize was deferred to here.  No bias: InstanceNorm removes any per-(image, channel) constant, so
            # IN(conv(x) + b) == IN(conv(x)) exactly, and leaving b out keeps the stored bf16
            # tensor better centred (less rounding error amplified by 1/sigma)
            dst = T(name, s, c)
            if pro is not None:   # materialise the activated input once ('a.<conv>'): forward and wgrad then need no prologue
                act = slot.buf("a." + name, src.shape)
                if isinstance(pro, NormState):
                    self._norm_act(P, pro, act, self.LR)
                else:
                    rec_act(P, name + ".act", src, act, pro)
                src = act
            st = self._conv_norm(P, slot, name, src, dst, pc[name], groups=n, defer=defer, **conv_kw)
            return dst, st

        # defer=True: the layer's InstanceNorm is finalised by the launch that writes the next conv's input
        t01, s01 = cn("conv0_1", a01, h1, nf, None, True, **self._cond_forward(P, slot, h1))
        t10, s10 = cn("conv1_0", t01, h2, nf * 2, s01, True)
        t11, s11 = cn("conv1_1", t10, h2, nf * 2, s10, True)
        t20, s20 = cn("conv2_0", t11, h3, nf * 4, s11, True)
        t21, s21 = cn("conv2_1", t20, h3, nf * 4, s20, True)
        t30, s30 = cn("conv3_0", t21, h4, nf * 8, s21, True)
        t31, s31 = cn("conv3_1", t30, h4, nf * 8, s30, True)

        def up(level, y, sy, skip, ss, s_in, c):
            o = slot.buf("up%d" % level, (n, 2 * s_in, 2 * s_in, c))
            P.hold(y, skip)
            if sy.pending is not None and sy.pending["rpg"] > self.FUSED_MAX_ROWS:
                # more partial rows than the fused launch takes (112 x 112 maps of 224 x 224 images: 392 per image):
                # the statistics are finalised by a launch of their own, the upsampling reads scale / shift below
                q = sy.pending
                sy.pending = None
                scr = self._norm_scratch(P, n, c, q["rpg"])
                P.hold(q["part"])
                P.add("up%d.finalize" % level, lib.combat_norm_finalize, q["part"].data_ptr(), n, q["rpg"], c,
                      float(s_in * s_in), 1e-5, None, None, sy.mean.data_ptr(), sy.rstd.data_ptr(), sy.scale.data_ptr(),
                      sy.shift.data_ptr(), None, None, 0.1, None, scr.data_ptr(), scr.numel() * 4)
            if sy.pending is not None:   # y's InstanceNorm is finalised by the launch that upsamples it
                q = sy.pending
                sy.pending = None
                P.hold(q["part"])
                P.add("up%d.fin" % level, lib.combat_unet_up_fused, y.data_ptr(), _p(q["part"]), q["rpg"], _p(skip),
                      ss.scale.data_ptr() if ss else None, ss.shift.data_ptr() if ss else None, n, s_in, s_in, c, 1e-5,
                      sy.mean.data_ptr(), sy.rstd.data_ptr(), sy.scale.data_ptr(), sy.shift.data_ptr(), o.data_ptr())
                return o
            P.add("up%d" % level, lib.combat_unet_up_fwd, y.data_ptr(), sy.scale.data_ptr(), sy.shift.data_ptr(),
                  _p(skip), ss.scale.data_ptr() if ss else None, ss.shift.data_ptr() if ss else None, n, s_in, s_in, c,
                  o.data_ptr())
            return o

        u3 = up(3, t31, s31, None, None, h4, nf * 8)
        tu31, su31 = cn("upconv3_1", u3, h3, nf * 8, None, True)
        tu30, su30 = cn("upconv3_0", tu31, h3, nf * 4, su31, True)
        u2 = up(2, tu30, su30, t21, s21, h3, nf * 4)
        tu21, su21 = cn("upconv2_1", u2, h2, nf * 4, None, True)
        tu20, su20 = cn("upconv2_0", tu21, h2, nf * 2, su21, True)
        u1 = up(1, tu20, su20, t11, s11, h2, nf * 2)
        tu11, su11 = cn("upconv1_1", u1, h1, nf * 2, None, True)
        tu10, su10 = cn("upconv1_0", tu11, h1, nf, su11, True)
        u0 = up(0, tu10, su10, t01, s01, h1, nf)
        tu01, su01 = cn("upconv0_1", u0, hw, nf, None)
        rec_conv(P, "upconv0_0", tu01, self.output(slot), pc["upconv0_0"], 0, pro=self._in_aff(su01),
                 bias=self.out_bias8, tanh_out=True)
        slot.plans["fwd"] = P
        return P

    def backward_plan(self, slot: Slot) -> Plan:
        """Given slot buffer 'g.z' (gradient w.r.t. the pre-tanh output, bf16 NHWC c8) produce all
        parameter gradients in fp.grad (zeroed first).  Conv biases that feed an InstanceNorm get
        an exactly-zero gradient (the norm removes any per-channel constant)."""
        if "bwd" in slot.plans:
            return slot.plans["bwd"]
        P = Plan("unet.bwd")
        fp, n, hw, nf = self.fp, slot.N, slot.hw, self.nf
        pc = self.pc
        t = lambda name: slot.bufs["t." + name]
        stn = lambda name: slot.norm[name]
        G = lambda name, like: slot.buf("g." + name, like.shape)
        P.add("zero_grad", _zero_grad_call, fp)
        gz = slot.buf("g.z", (n, hw, hw, 8))

        def through_norm(name, dy, pcv, src_name, add_pre=None, first=False):
            """dy = gradient w.r.t. raw output of conv `pcv` whose input is LR(IN(t[src_name])).
            wgrad of pcv, then gradient w.r.t. t[src_name] (returned).  first: the plan's first layer -- its auxiliary
            calls are recorded BEHIND its input-gradient launch, so that they are handed the plan stream's state by that
            launch's completion event: an auxiliary call that opens a plan needs an event record in the plan's queue,
            which held the first kernel of the generator's backward back by ~20 us (tools/timeline.py)."""
            src, st = t(src_name), stn(src_name)
            act = slot.bufs.get("a." + name)   # LR(IN(src)) of the forward (all but the K = 8 output layer)

            def wgrad():
                if act is not None:
                    rec_wgrad(P, name + ".wgrad", act, dy, pcv, fp.grad_phys(name + ".weight"))
                else:
                    rec_wgrad(P, name + ".wgrad", src, dy, pcv, fp.grad_phys(name + ".weight"), self._in_aff(st))
            if not first:
                wgrad()
            dz = G(src_name + ".dz", src)
            self._dgrad_norm(P, slot, "g." + src_name, dy, dz, pcv, src, st, group_stride=st.C, slope=self.LR,
                             add_pre=add_pre)
            if first:
                P.add("db.upconv0_0", lib.combat_colsum, gz.data_ptr(), n * hw * hw, 8, 3,
                      fp.grad_phys("upconv0_0.bias").data_ptr(), aux=True)
                wgrad()
            dx = G(src_name + ".dx", src)
            self._bwd_apply(P, slot, "g." + src_name, dz, src, dx, st)
            return dx

        def through_up(name, dy, pcv, level, y_name):
            """dy = gradient w.r.t. raw output of conv `pcv` whose input is up[level].  Returns
            (du, d_y): du = gradient w.r.t. the pre-upsample sum, d_y = gradient w.r.t. t[y_name]."""
            u = slot.bufs["up%d" % level]
            rec_wgrad(P, name + ".wgrad", u, dy, pcv, fp.grad_phys(name + ".weight"), None)
            du_full = G("up%d.d" % level, u)
            rec_conv(P, name + ".dgrad", dy, du_full, pcv, 1)
            y, st = t(y_name), stn(y_name)
            du = G("u%d" % level, y)
            dy_out = G(y_name + ".dx", y)
            if y.shape[1] * y.shape[2] <= 64:   # upsample adjoint + InstanceNorm backward, one launch (one workgroup per
                # (image, 64 channels): on 16 x 16 maps that is half the chip doing all the work -- two launches there)
                P.hold(du_full, u, y, du, dy_out)
                P.add("up%d.bwd.norm" % level, lib.combat_unet_up_bwd_fused, du_full.data_ptr(), u.data_ptr(), y.data_ptr(),
                      st.mean.data_ptr(), st.rstd.data_ptr(), n, y.shape[1], y.shape[2], y.shape[3], du.data_ptr(),
                      dy_out.data_ptr())
                return du, dy_out
            P.add("up%d.bwd" % level, lib.combat_unet_up_bwd, du_full.data_ptr(), u.data_ptr(), n, y.shape[1],
                  y.shape[2], y.shape[3], du.data_ptr())
            self._bwd_apply(P, slot, "g." + y_name, du, y, dy_out, st)    # sums taken from du / y directly
            return du, dy_out

        d = through_norm("upconv0_0", gz, pc["upconv0_0"], "upconv0_1", first=True)
        du0, d = through_up("upconv0_1", d, pc["upconv0_1"], 0, "upconv1_0")
        d = through_norm("upconv1_0", d, pc["upconv1_0"], "upconv1_1")
        du1, d = through_up("upconv1_1", d, pc["upconv1_1"], 1, "upconv2_0")
        d = through_norm("upconv2_0", d, pc["upconv2_0"], "upconv2_1")
        du2, d = through_up("upconv2_1", d, pc["upconv2_1"], 2, "upconv3_0")
        d = through_norm("upconv3_0", d, pc["upconv3_0"], "upconv3_1")
        _, d = through_up("upconv3_1", d, pc["upconv3_1"], 3, "conv3_1")
        P.mark(fp.offsets["upconv3_1.weight"][0])          # decoder gradients complete
        d = through_norm("conv3_1", d, pc["conv3_1"], "conv3_0")
        d = through_norm("conv3_0", d, pc["conv3_0"], "conv2_1", add_pre=du2)
        P.mark(fp.offsets["conv3_0.weight"][0])            # + the two 512-channel encoder layers (14 MB of the rest)
        d = through_norm("conv2_1", d, pc["conv2_1"], "conv2_0")
        d = through_norm("conv2_0", d, pc["conv2_0"], "conv1_1", add_pre=du1)
        d = through_norm("conv1_1", d, pc["conv1_1"], "conv1_0")
        d = through_norm("conv1_0", d, pc["conv1_0"], "conv0_1", add_pre=du0)
        # conv0_1 reads LeakyReLU(conv0_0 output): no norm in between
        t00 = t("conv0_0")
        lr_only = Affine(None, None, 0, True, self.LR)
        self._conv0_1_wgrad(P, slot, d)
        d00 = G("conv0_0.dx", t00)
        rec_conv(P, "conv0_1.dgrad", d, d00, pc["conv0_1"], 1, mask_x=t00, mask=Affine(None, None, 0, True, self.LR))
        P.add("db.conv0_0", lib.combat_colsum, d00.data_ptr(), d00.numel() // d00.shape[-1], d00.shape[-1],
              d00.shape[-1], fp.grad_phys("conv0_0.bias").data_ptr(), aux=True)
        rec_wgrad(P, "conv0_0.wgrad", self.input(slot), d00, pc["conv0_0"], fp.grad_phys("conv0_0.weight"), aux=False)
        P.mark(0)
        group_wgrads(P, self.device)
        slot.plans["bwd"] = P
        return P


class CUnetEngine(UnetEngine):
    """CUnetGeneratorv1 (networks/models.py:472-555): UnetGenerator whose conv0_1 also reads num_classes constant one-hot
    planes of the image's label (:525-530).  The planes never exist here: conv0_1 stays the nf-channel launch over
    W_f = weight[:, :nf], and the planes' share of its raw output -- which depends on the label, the output channel and
    the border case of the pixel only -- is the `add_pre` operand of that launch (combat_cond_fwd).
    Labels: slot buffer 'y', int32 [N] (`labels(slot)`), read by the launches when the plans run.

    The parameter stays one [nf][nf + num_classes][3][3] tensor.  Its gradient has two producers: the nf-channel
    weight-gradient launch writes W_f's part to the scratch `dwf01` (it addresses rows of c_real contiguous channels,
    the parameter's rows hold nf + num_classes), and combat_cond_wgrad -- which has to run behind that launch on the same
    gradient tensor anyway -- computes W_y's part and copies the scratch into the parameter's gradient rows: the merge
    costs no launch of its own and no convolution kernel changes.  For the same reason W_f's packed operand is built
    from `wf01`, a contiguous copy of weight[:, :nf] taken at every refresh()."""

    def __init__(self, module):
        self.num_classes = int(module.num_classes)
        super().__init__(module)

    def _w01(self) -> torch.Tensor:
        """conv0_1.weight in the flat buffer: [nf][3][3][nf + num_classes]."""
        return self.fp._slice(self.fp.flat, "conv0_1.weight").view(self.nf, 3, 3, self.nf + self.num_classes)

    def _conv_operand(self, name: str, conv):
        if name != "conv0_1":
            return super()._conv_operand(name, conv)
        nf = self.nf
        self.wf01 = torch.empty(nf, 3, 3, nf, dtype=f32, device=self.device)
        self.dwf01 = torch.zeros(nf, 9, nf, dtype=f32, device=self.device)
        return self.wf01.permute(0, 3, 1, 2), nf

    def refresh(self) -> None:
        if self.weights_dirty:
            self.wf01.copy_(self._w01()[..., :self.nf])
        super().refresh()

    def labels(self, slot: Slot) -> torch.Tensor:
        """The labels the plans of `slot` condition on (int32 [N], zeros until written)."""
        return slot.buf("y", (slot.N,), torch.int32, zero=True)

    def _cond_forward(self, P: Plan, slot: Slot, s: int) -> dict:
        y = self.labels(slot)
        cond = slot.buf("cond", (slot.N, s, s, self.nf))
        P.hold(y, cond)
        P.add("cond", lib.combat_cond_fwd, self._w01().data_ptr() + 4 * self.nf, y.data_ptr(), slot.N, s, self.nf,
              self.num_classes, cond.data_ptr())
        return dict(add_pre=cond)

    def _conv0_1_wgrad(self, P: Plan, slot: Slot, d) -> None:
        nf = self.nf
        # (the weight-gradient launch adds to a zeroed tensor; zeroed on the plan's stream, which the auxiliary queue follows)
        P.add("conv0_1.dwf.zero", lib.combat_memset_zero, self.dwf01.data_ptr(), self.dwf01.numel() * 4)
        rec_wgrad(P, "conv0_1.wgrad", slot.bufs["a.conv0_1"], d, self.pc["conv0_1"], self.dwf01)
        taps = slot.buf("cond.taps", (slot.N, 9, nf), f32)
        y = self.labels(slot)
        dw = self.fp.grad_phys("conv0_1.weight")
        P.hold(taps, y, dw, d)
        # auxiliary like the bias column sums: consumed by the optimiser only
        P.add("cond.wgrad", lib.combat_cond_wgrad, d.data_ptr(), y.data_ptr(), slot.N, d.shape[1], nf, self.num_classes,
              self.dwf01.data_ptr(), dw.data_ptr(), taps.data_ptr(), aux=True, after=P.calls[-1])


# --------------------------------------------------------------------------------------------
# WaNet grid generator
# --------------------------------------------------------------------------------------------


class GridEngine(NetEngine):
    """GridGenerator (networks/models.py:344-385) + the warp of train_generator_wanet.py:151-157.

    The reference pools an affine-free InstanceNorm output -- spatial mean exactly 0 -- so the network's output
    is tanh(fc2(lrelu(fc1.bias))) for every input and its encoder receives no gradient (pinned against the
    reference module: tests/test_oracle_golden.py::test_grid_generator_is_a_constant_field...).  The engine
    therefore computes the [2][S][S] field from the three head tensors, the [H][H][2] sampling grid shared by the
    batch, and in the backward the gradients of fc1.bias, fc2.weight and fc2.bias; every other parameter keeps a
    zero gradient (weight decay still applies in the optimiser, as in the reference)."""

    def __init__(self, module):
        super().__init__(module)
        m = module
        self.S, self.nf = int(m.S), int(m.fc1.out_features)
        self.nout = 2 * self.S * self.S
        self.field = torch.zeros(self.nout, dtype=f32, device=self.device)
        self._grids: Dict[int, dict] = {}

    def refresh(self) -> None:   # no packed operands
        self.weights_dirty = False

    def grid_bufs(self, hw: int) -> dict:
        g = self._grids.get(hw)
        if g is None:
            # U[H][S]: the linear map of F.upsample(size=H, mode="bicubic", align_corners=True) along one axis
            # (train_generator_wanet.py:152), taken from the operator itself on the basis vectors
            eye = torch.eye(self.S, dtype=f32).view(self.S, 1, self.S, 1)
            u = torch.nn.functional.interpolate(eye, size=(hw, 1), mode="bicubic", align_corners=True)   # [S,1,H,1]
            U = u[:, 0, :, 0].t().contiguous()
            g = dict(U=U.to(self.device), noise_grid=torch.zeros(hw, hw, 2, dtype=f32, device=self.device),
                     grid=torch.zeros(hw, hw, 2, dtype=f32, device=self.device))
            self._grids[hw] = g
        return g

    def _head(self):
        fp = self.fp
        return (fp._slice(fp.flat, "fc1.bias"), fp._slice(fp.flat, "fc2.weight"), fp._slice(fp.flat, "fc2.bias"))

    def forward_grid(self, hw: int, rescale: float, st=None) -> dict:
        """field, noise_grid and the sampling grid for H = hw (two launches)."""
        st = torch.cuda.current_stream().cuda_stream if st is None else st
        g = self.grid_bufs(hw)
        b1, w2, b2 = self._head()
        ops.check(lib.combat_grid_head_fwd(b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), self.nf, self.nout,
                                           self.field.data_ptr(), st), "combat_grid_head_fwd")
        ops.check(lib.combat_wanet_grid(self.field.data_ptr(), g["U"].data_ptr(), self.S, hw, float(rescale),
                                        g["noise_grid"].data_ptr(), g["grid"].data_ptr(), st), "combat_wanet_grid")
        return g

    def head_grad_range(self) -> Tuple[int, int]:
        """[lo, hi) of the flat gradient buffer that holds every gradient this engine ever writes (fc1.bias,
        fc2.weight, fc2.bias are consecutive parameters); the rest of fp.grad stays exactly zero."""
        offs = [self.fp.offsets[k] for k in ("fc1.bias", "fc2.weight", "fc2.bias")]
        lo = min(o for o, _, _ in offs)
        hi = max(o + n for o, n, _ in offs)
        inside = sum(n for o, n, _ in self.fp.offsets.values() if lo <= o < hi)
        assert inside == sum(n for _, n, _ in offs), "head parameters are not contiguous in the flat buffer"
        return lo, hi

    def backward_field(self, partial: torch.Tensor, groups: int, hw: int, rescale: float, l2_scale: float, st=None) -> None:
        """d(loss)/d(grid) partial sums -> gradients of the head in fp.grad (the rest of fp.grad must be zero)."""
        st = torch.cuda.current_stream().cuda_stream if st is None else st
        g, fp = self.grid_bufs(hw), self.fp
        b1, w2, _ = self._head()
        ops.check(lib.combat_wanet_field_bwd(partial.data_ptr(), groups, g["noise_grid"].data_ptr(), g["U"].data_ptr(), self.S, hw,
                                             float(rescale), float(l2_scale), self.field.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                             self.nf, fp._slice(fp.grad, "fc1.bias").data_ptr(),
                                             fp._slice(fp.grad, "fc2.weight").data_ptr(),
                                             fp._slice(fp.grad, "fc2.bias").data_ptr(), None, st), "combat_wanet_field_bwd")


# --------------------------------------------------------------------------------------------
# Frequency detector (metric only)
# --------------------------------------------------------------------------------------------


class FreqEngine(NetEngine):
    """FrequencyModel (defenses/frequency_based/model.py:8-52) in eval mode: 6 x
    (conv+bias -> ELU -> BatchNorm(running stats)), 2x2 max-pool after every second, Linear."""

    def __init__(self, module):
        super().__init__(module)
        m = module
        self.layers = []
        cin = 8
        for i, w in enumerate(m.WIDTHS, start=1):
            conv, bn = getattr(m, "conv%d" % i), getattr(m, "bn%d" % i)
            self.layers.append((self._pc(conv.weight.data, 1, 1, cin, dup=(i == 1), need_dgrad=False), conv.bias.data,
                                _BN(self, bn, "bn%d" % i)))
            cin = w
        self.lin_w, self.lin_b = m.linear6.weight.data, m.linear6.bias.data
        self.classes = m.linear6.out_features

    def _refresh_extra(self):
        for _, _, bn in self.layers:
            bn.fold()

    def input(self, slot: Slot) -> torch.Tensor:
        return slot.buf("x", (slot.N, slot.hw, slot.hw, 8))

    def forward_plan(self, slot: Slot) -> Plan:
        if "fwd" in slot.plans:
            return slot.plans["fwd"]
        P = Plan("freq.fwd")
        n, s = slot.N, slot.hw
        cur = self.input(slot)
        for i, (pc, bias, bn) in enumerate(self.layers, start=1):
            raw = slot.buf("c%d" % i, (n, s, s, pc.K))
            rec_conv(P, "conv%d" % i, cur, raw, pc, 0, bias=bias)
            act = slot.buf("a%d" % i, (n, s, s, pc.K))
            P.add("elu_bn%d" % i, lib.combat_elu_affine, raw.data_ptr(), n * s * s, pc.K, bn.escale.data_ptr(),
                  bn.eshift.data_ptr(), act.data_ptr())
            cur = act
            if i % 2 == 0:
                pooled = slot.buf("p%d" % i, (n, s // 2, s // 2, pc.K))
                P.add("pool%d" % i, lib.combat_maxpool2, cur.data_ptr(), n, s, s, pc.K, pooled.data_ptr())
                cur, s = pooled, s // 2
        logits = slot.buf("logits", (n, self.classes), f32)
        P.add("linear", lib.combat_linear_nhwc, cur.data_ptr(), n, s, s, cur.shape[-1], self.lin_w.data_ptr(),
              self.lin_b.data_ptr(), self.classes, logits.data_ptr())
        slot.plans["fwd"] = P
        return P


# --------------------------------------------------------------------------------------------
# drop-in module(x) with autograd (reference call signature; not the fast path)
# --------------------------------------------------------------------------------------------

ENGINES = {"preact_resnet18": PreActEngine, "resnet18": ResNetEngine, "unet": UnetEngine, "cunet": CUnetEngine,
           "freq": FreqEngine, "gridgen": GridEngine, "vgg": VggEngine}


def build_engine(module) -> NetEngine:
    cls = ENGINES.get(module.arch)
    if cls is None:
        raise NotImplementedError("no HIP engine for architecture %r yet" % module.arch)
    return cls(module)


def _images_to_c8(x: torch.Tensor, dst: torch.Tensor) -> None:
    ops.image_to_c8(x.contiguous().float(), dst)


def pad_batch(n: int) -> int:
    """Inference batches are rounded up to a multiple of 16 so that ragged sizes (the non-target subset
    of a test batch) share slots and plans; every sample is independent in eval mode (BatchNorm uses
    running statistics, InstanceNorm is per sample), so the padding rows change nothing."""
    return max(16, (n + 15) // 16 * 16)


class _ClassifierFn(torch.autograd.Function):
    """logits = netC(x) through the HIP plans.  Backward supports the two uses the reference
    makes of a classifier: train mode -> parameter gradients; eval mode -> input gradient."""

    @staticmethod
    def forward(ctx, module, x, *params):
        eng: PreActEngine = module._net_engine()
        eng.refresh()
        n, _, hw, _ = x.shape
        train = module.training
        slot = eng.slot("module.train" if train else "module.eval", n if train else pad_batch(n), hw)
        _images_to_c8(x, eng.input(slot))
        eng.forward_plan(slot, train).run()
        if train:
            eng.fold_bn()
        ctx.module, ctx.slot, ctx.train = module, slot, train
        return eng.head_bufs(slot)["logits"][:n].clone()

    @staticmethod
    def backward(ctx, dlogits):
        raise NotImplementedError(
            "differentiate through combat_amd.step.AlternatedStep (fused loss heads); module(x) is inference-only")


class _GeneratorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, *params):
        eng: UnetEngine = module._net_engine()
        eng.refresh()
        n, _, hw, _ = x.shape
        if n == 0:
            return x.new_zeros(x.shape)
        slot = eng.slot("module", pad_batch(n), hw)
        _images_to_c8(x, eng.input(slot))
        eng.forward_plan(slot).run()
        out = torch.empty(slot.N, 3, hw, hw, dtype=f32, device=x.device)
        ops.nhwc_to_nchw_f32(eng.output(slot), 3, out)
        return out[:n]

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError(
            "differentiate through combat_amd.step.AlternatedStep; module(x) is inference-only")


class _CondGeneratorFn(torch.autograd.Function):
    """noise = netG(x, y) of a CUnetGeneratorv1 (networks/models.py:523-555); inference-only like _GeneratorFn."""

    @staticmethod
    def forward(ctx, module, x, y, *params):
        eng: CUnetEngine = module._net_engine()
        eng.refresh()
        n, _, hw, _ = x.shape
        if n == 0:
            return x.new_zeros(x.shape)
        slot = eng.slot("module", pad_batch(n), hw)
        _images_to_c8(x, eng.input(slot))
        eng.labels(slot)[:n].copy_(y)
        eng.forward_plan(slot).run()
        out = torch.empty(slot.N, 3, hw, hw, dtype=f32, device=x.device)
        ops.nhwc_to_nchw_f32(eng.output(slot), 3, out)
        return out[:n]

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError("module(x, y) is inference-only; the parameter gradients come from CUnetEngine.backward_plan")


class _GridFn(torch.autograd.Function):
    """[B, 2, S, S] field of a GridGenerator: the same for every sample (see GridEngine).  Like the other modules'
    `module(x)` it is inference-only: a backward through it raises instead of handing the caller's own training
    loop a silent zero gradient (the differentiated path is combat_amd.step.WanetStep)."""

    @staticmethod
    def forward(ctx, module, x, *params):
        eng = module._net_engine()
        st = torch.cuda.current_stream().cuda_stream
        b1, w2, b2 = eng._head()
        ops.check(lib.combat_grid_head_fwd(b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), eng.nf, eng.nout,
                                           eng.field.data_ptr(), st), "combat_grid_head_fwd")
        return eng.field.view(1, 2, eng.S, eng.S).expand(x.shape[0], -1, -1, -1).clone()

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError(
            "differentiate through combat_amd.step.WanetStep; module(x) is inference-only")


def check_labels(y, n: int, num_classes: int) -> torch.Tensor:
    """The labels of n images as F.one_hot takes them (networks/models.py:526): an integer tensor [n] with every entry
    in 0..num_classes-1, else ValueError.  The range is checked on the host for a host tensor; for a device tensor it
    is not read back (the kernels condition an out-of-range label on nothing)."""
    y = torch.as_tensor(y)
    if y.dim() != 1 or y.numel() != n or y.dtype.is_floating_point or y.dtype == torch.bool:
        raise ValueError("labels must be an integer tensor [%d], got %s %s" % (n, y.dtype, tuple(y.shape)))
    if y.device.type == "cpu" and n and (int(y.min()) < 0 or int(y.max()) >= num_classes):
        raise ValueError("labels must lie in 0..%d, got %d..%d" % (num_classes - 1, int(y.min()), int(y.max())))
    return y.to(torch.int32)


def cond_module_forward(module, x: torch.Tensor, y) -> torch.Tensor:
    """The reference's `netG(x, y)` (networks/models.py:523) on the HIP path."""
    if x.device.type != "cuda":
        raise CombatHipError("combat_amd modules run on the GPU only; got a %s tensor" % x.device)
    y = check_labels(y, x.shape[0], module.num_classes)
    return _CondGeneratorFn.apply(module, x, y, *tuple(module.parameters()))


def module_forward(module, x: torch.Tensor) -> torch.Tensor:
    """The reference's `module(x)` call signature (float32 NCHW in, float32 out) on the HIP path."""
    if x.device.type != "cuda":
        raise CombatHipError("combat_amd modules run on the GPU only; got a %s tensor" % x.device)
    params = tuple(module.parameters())
    if module.arch == "unet":
        return _GeneratorFn.apply(module, x, *params)
    if module.arch in ("preact_resnet18", "resnet18", "vgg"):
        return _ClassifierFn.apply(module, x, *params)
    if module.arch == "gridgen":
        return _GridFn.apply(module, x, *params)
    if module.arch == "freq":
        eng = module._net_engine()
        eng.refresh()
        n, _, hw, _ = x.shape
        slot = eng.slot("module", pad_batch(n), hw)
        ops.image_to_c8(x.contiguous().float(), eng.input(slot))  # hi/lo split keeps the DCT's dynamic range
        eng.forward_plan(slot).run()
        return slot.bufs["logits"][:n].clone()
    raise NotImplementedError(module.arch)
