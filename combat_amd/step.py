"""The alternated generator/surrogate training step on the HIP engines
(reference: the loop body train_generator.py:170-290).

Phase C updates the surrogate classifier ``netC`` on a batch whose first ``num_bd`` target-class
images carry the generator's trigger; Phase G updates the generator ``netG`` against the just
updated (eval-mode) ``netC`` and the frozen ``clean_model``.  Work whose results the reference
discards is not launched: the generator backward of Phase C (:220 zeroes it),
the classifier / clean-model weight gradients of Phase G (:179 zeroes netC's; clean_model has no
optimiser), and autograd graphs for the three metric-only forwards (:214, :227, :245-247).

Every random draw the reference makes is taken on the host *before* anything is launched
(``StepRandomness``) and shipped to the device as small tables, so a step is a fixed sequence of
kernel launches with no host synchronisation; metric counters stay on the device until
``read_metrics``.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Dict, List, Optional

import os

import numpy as np
import torch

from . import ops, trigger
from ._lib import lib
from .augment import PostTensorTransform
from .dist import GradReducer, bucket_ranges
from .engine import FreqEngine, PlanSeq, PreActEngine, UnetEngine, _zero_grad_call, f32, short_workgroups

BUCKETS = (8, 16, 32, 64, 128, 256, 512, 1024)


def bucket(n: int) -> int:
    for b in BUCKETS:
        if n <= b:
            return b
    raise ValueError("poisoned sub-batch of %d images exceeds the largest bucket" % n)


@dataclass
class StepRandomness:
    """The draws of one step, in the order the reference makes them (train_generator.py:183,
    194, 196, 214, 226-228, 250): num_bd (numpy global RNG), the two blur sigmas (torch global
    RNG) and five augmentation tables (Python ``random`` + torch RNG)."""

    num_bd: int
    sigma_c: float
    sigma_g: float
    aug: List[Optional[np.ndarray]] = field(default_factory=lambda: [None] * 5)


def create_targets_bd(targets: torch.Tensor, opt) -> torch.Tensor:
    """train_generator.py:70-77."""
    if opt.attack_mode == "all2one":
        return torch.ones_like(targets) * opt.target_label
    if opt.attack_mode == "all2all":
        return (targets + 1) % opt.num_classes
    raise Exception("{} attack mode is not implemented".format(opt.attack_mode))


def draw_num_bd(targets_cpu: torch.Tensor, bd_targets_cpu: torch.Tensor, pc: float) -> int:
    """How many of the batch's target-class images are poisoned (train_generator.py:183; numpy global RNG)."""
    n_trg = int((targets_cpu == bd_targets_cpu).sum())
    return int(np.sum(np.random.rand(n_trg) < pc))


def draw_randomness(targets_cpu: torch.Tensor, bd_targets_cpu: torch.Tensor, opt, transforms: PostTensorTransform,
                    sigma_range=(0.1, 1.0)) -> StepRandomness:
    """Consume the three RNG streams exactly where the reference does."""
    n = targets_cpu.shape[0]
    num_bd = draw_num_bd(targets_cpu, bd_targets_cpu, opt.pc)           # :183
    sigma_c = trigger.sample_sigma(sigma_range) if num_bd else 0.5      # :194 (skipped when empty)
    aug0 = transforms.sample(n)                                         # :196
    aug1 = transforms.sample(n)                                         # :214
    sigma_g = trigger.sample_sigma(sigma_range)                         # :226
    aug2, aug3 = transforms.sample(n), transforms.sample(n)             # :227, :228
    aug4 = transforms.sample(n)                                         # :250
    return StepRandomness(num_bd, sigma_c, sigma_g, [aug0, aug1, aug2, aug3, aug4])


def poison_tables(targets: torch.Tensor, bd_targets: torch.Tensor, num_bd: int):
    """Host-side index tables of Phase C (train_generator.py:181-204).  The batch is re-ordered
    [first num_bd target-class images (poisoned), remaining target-class images, all others]:
      perm         int32 [n]  source image of every row of the re-ordered batch
      total_targets int64 [n] labels of the re-ordered batch (poisoned rows carry bd_targets)
      idx_small    int32 [n]  first num_bd entries = images handed to the generator
      idx_total    int32 [n]  gather indices into the [inputs ; triggered images] staging buffer
                               (rows < num_bd read the triggered copies at n + i)"""
    perm, idx_small, idx_total = order_tables((targets == bd_targets).nonzero()[:, 0], (targets != bd_targets).nonzero()[:, 0], num_bd)
    total_targets = targets[perm.long()].clone()
    total_targets[:num_bd] = bd_targets[perm[:num_bd].long()]
    return perm, total_targets, idx_small, idx_total


def order_tables(first: torch.Tensor, rest: torch.Tensor, num_bd: int):
    """perm, idx_small and idx_total (see poison_tables) of the batch order [first ; rest] whose first num_bd rows are poisoned."""
    perm = torch.cat([first, rest]).to(torch.int32)
    n = perm.shape[0]
    idx_small = torch.zeros(n, dtype=torch.int32)
    idx_small[:num_bd] = perm[:num_bd]
    idx_total = perm.clone()
    if num_bd:
        idx_total[:num_bd] = torch.arange(n, n + num_bd, dtype=torch.int32)
    return perm, idx_small, idx_total


_STREAMS: Dict = {}


def shared_stream(device, kind: str) -> torch.cuda.Stream:
    """The process-wide stream of a kind ("side") on a device.  Streams are NOT per step object: the HIP
    runtime multiplexes a process's streams onto a handful of hardware queues, and with the nine streams that two
    step objects with private streams add up to (bench.py's golden gate + the timed step) launches started to block on
    the host -- 10.6 instead of 4.3 ms/step, 9 ms of it inside the enqueue calls."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), kind)
    s = _STREAMS.get(key)
    if s is None:
        s = torch.cuda.Stream(device=dev)
        _STREAMS[key] = s
    return s


FORCE_ALLREDUCE = os.environ.get("COMBAT_FORCE_ALLREDUCE", "0") == "1"   # issue the bucketed all-reduces even at world size 1
#                                                                          (tests: RCCL's streams beside the step's on ONE GPU)


def backward_allreduce(plan, eng, pg, world: int, reducers: dict, prof=None) -> None:
    """Run a backward plan; with several ranks, all-reduce the flat gradient buffer in buckets, each launched as
    soon as the plan has enqueued the kernels that complete it (`Plan.mark`), so that the first buckets travel
    while the rest of the backward still runs.  `reducers` caches the GradReducer per plan."""
    if world == 1 and not (FORCE_ALLREDUCE and pg is not None):
        plan.run(prof)
        return
    red = reducers.get(id(plan))
    if red is None:
        ranges = bucket_ranges(eng.fp.total, plan.mark_offsets)
        red = (GradReducer(eng.fp.grad, ranges, pg), ranges)
        reducers[id(plan)] = red
    reducer, ranges = red
    launched = set()

    def on_mark(offset):
        for i, (lo, hi) in enumerate(ranges):
            if lo >= offset and i not in launched:
                launched.add(i)
                reducer.launch(i)

    plan.run(prof, on_mark=on_mark)
    on_mark(0)
    reducer.wait()


# Label rows of the step table (int64 [n] each).  The heads' label buffers are views of these rows, bound where the
# slots are made; AlternatedStep._run and InputAwareStep._fill_table_extra fill them.
LAB_TARGETS, LAB_BD, LAB_TOTAL = 0, 1, 2   # targets, bd_targets, total_targets (labels of Phase C's re-ordered batch)
LAB_K = slice(3, 5)       # the clean model's 2n batch [aug(inputs) ; aug(inputs_bd)]: targets twice
LAB_K2 = slice(5, 7)      # its second label set: the metric half's row is unused, the loss half's holds bd_targets
LAB_CROSS = slice(7, 9)   # input-aware only, netC's two-half pass [aug3(bd) ; aug5(bd2)]: bd_targets, targets


def step_table(n: int, n_aug: int, n_blur: int, n_lab: int, **alloc):
    """The step's ONE host->device table (one copy instead of a dozen 10-us ones in front of the generator forward) as
    zeroed bytes and its typed views: [n_aug augmentation tables | index_small, index_total | n_blur 3-tap blur kernels |
    n_lab label rows] -> (raw, float32 [n_aug, n, 4], int32 [2, n], float32 [n_blur, 3], int64 [n_lab, n]).  The blur
    section holds the kernels in pairs of 24 bytes (an odd count leaves 12 bytes of padding), which keeps the label
    rows 8-byte aligned.  `alloc` goes to torch.zeros (device=..., pin_memory=True)."""
    o1 = n_aug * n * 16
    o2 = o1 + 2 * n * 4
    o3 = o2 + 24 * ((n_blur + 1) // 2)
    raw = torch.zeros(o3 + n_lab * n * 8, dtype=torch.uint8, **alloc)
    return (raw, raw[:o1].view(f32).view(n_aug, n, 4), raw[o1:o2].view(torch.int32).view(2, n),
            raw[o2:o2 + 12 * n_blur].view(f32).view(n_blur, 3), raw[o3:].view(torch.int64).view(n_lab, n))


class PerBatchSize:
    """Buffers, slots and plans of a step are per batch size and cached, one object each (`_build_set`), in `_sets`: the
    ragged last batch of an epoch (80 images for CIFAR-10) gets its own set once, and the metric cells of every set
    survive until `read_metrics` sums them.  `cur` is the set of the batch size `N` that ran last."""

    N = 0
    cur = None

    def _setup(self, n: int):
        if n != self.N:
            if n not in self._sets:
                self._sets[n] = self._build_set(n)
            self.cur, self.N = self._sets[n], n
        return self.cur

    def __getattr__(self, name):
        """Readers outside the step (bench.py, the training scripts, tests, tools) spell a field of the current set as an
        attribute of the step: `st.bd`, `st.sG`, `st.pl`.  (Only reached when the normal lookup misses; the step itself
        reads the set.)"""
        if self.cur is None or not hasattr(self.cur, name):
            raise AttributeError("%s has no attribute %r" % (type(self).__name__, name))
        return getattr(self.cur, name)


class AlternatedStep(PerBatchSize):
    """Owns the engines, slots and small device tables of one rank's step."""

    serial = False   # True: no second stream (bench.py's instrumented replay times one kernel at a time)
    keep_grads = False   # True: leave the flat gradient buffers as the step computed them (tests inspect them);
    #                      default: they are zeroed behind each optimiser step, off the critical queue
    kStage = 4   # pinned staging sets (host steps in flight before it has to wait for the device)
    TABLE = (5, 2, 7)   # augmentation tables, blur kernels (sigma_c, sigma_g) and label rows of the step table
    FIXED_BLUR = False   # True: the blur is the reference script's module-level GaussianBlur -- kernel 3, sigma in
    #                      (0.1, 1) -- whatever --kernel_size / --sigma say

    def __init__(self, netC, netG, clean_model, netF, opt, process_group=None):
        if self.FIXED_BLUR:
            opt = copy.copy(opt)     # every blur kernel of the step is built from opt.kernel_size
            opt.kernel_size = 3
        self.opt = opt
        self.dev = next(netC.parameters()).device
        self.eC: PreActEngine = netC._net_engine()
        self.eG: UnetEngine = netG._net_engine()
        self.eK: PreActEngine = clean_model._net_engine()
        self.eF: Optional[FreqEngine] = netF._net_engine() if netF is not None else None
        self.netC, self.netG, self.clean_model, self.netF = netC, netG, clean_model, netF
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.hw = opt.input_height
        dev = self.dev
        self.P = trigger.lowpass_matrix(self.hw, opt.ratio).to(dev)
        self.D = trigger.dct_matrix(self.hw).float().to(dev)
        self.transforms = PostTensorTransform(opt)
        self.acc = torch.zeros(8, dtype=torch.float64, device=dev)  # running sums for logging
        self.acc_side = torch.zeros((), dtype=torch.float64, device=dev)   # detector hits (counted on the second stream)
        self._side = None
        self._host = None
        self.steps_done = 0
        self.samples = 0                 # images since the last metric reset
        self._reducers = {}
        self._sets: Dict[int, SimpleNamespace] = {}

    @property
    def sigma_range(self):
        return (0.1, 1.0) if self.FIXED_BLUR else getattr(self.opt, "sigma", (0.1, 1.0))

    # ------------------------------------------------------------------ buffers per batch size
    def _build_set(self, n: int) -> SimpleNamespace:
        """The set of one batch size; a subclass adds its own fields to what this returns."""
        dev, hw = self.dev, self.hw
        s = SimpleNamespace(n=n)
        s.cat_src = torch.zeros(2 * n, 3, hw, hw, dtype=f32, device=dev)   # [inputs ; poisoned images]
        s.inputs = s.cat_src[:n]
        s.bd = torch.empty(n, 3, hw, hw, dtype=f32, device=dev)
        s.d_bd = torch.empty(n, 3, hw, hw, dtype=f32, device=dev)
        s.d_bd2 = torch.empty(n, 3, hw, hw, dtype=f32, device=dev)   # clean-model share (second stream)
        s.mse = torch.empty(3 * n, dtype=f32, device=dev)   # per (image, channel)
        s.tab, s.tab_f, s.tab_i, s.k1, s.d_targets = step_table(n, *self.TABLE, device=dev)
        # pinned staging, a ring of kStage sets: the host runs several steps ahead of the device, and an
        # asynchronous copy reads its pinned source when the DEVICE gets to it -- a set is rewritten only
        # after the event behind its last copy has completed
        s._stage = []
        for _ in range(self.kStage):
            raw, tf, ti, k1, tg = step_table(n, *self.TABLE, pin_memory=True)
            s._stage.append(dict(raw=raw, tab_f=tf, tab_i=ti, k1=k1, targets=tg, done=None))
        s._stage_i = 0
        eC, eK = self.eC, self.eK
        # The eval-mode forwards of one network are independent per sample.  clean_model (off the critical
        # path, second stream): the metric-only forward and the differentiated one run as ONE 2n-image batch
        # [aug(inputs) ; aug(inputs_bd)] (train_generator.py:214+250 -- clean_model is frozen and :214
        # reads only `inputs`, so running it in Phase G changes nothing), backward on the triggered half
        # through a view slot.  netC (:227+228): the differentiated forward is on the critical path and runs
        # alone; the accuracy-only forward on the clean images goes to the second stream.
        # The heads read their labels straight out of the step table (bound before the plans marshal pointers).
        lab = s.d_targets
        s.sC_train = eC.slot("C.train", n, hw)
        s.sC_train.bufs["targets"] = lab[LAB_TOTAL]
        self._c_eval_slots(s)
        s.sK_eval = eK.slot("K.eval2", 2 * n, hw)
        s.sK_eval.bufs["targets"], s.sK_eval.bufs["targets2"] = lab[LAB_K].view(-1), lab[LAB_K2].view(-1)
        s.sG = self._gen_slot(n)
        s.sF = self.eF.slot("F", n, hw) if self.eF is not None else None
        w_cm = float(self.opt.clean_model_weight)
        s.pl = dict(
            C_train_f=eC.forward_plan(s.sC_train, True),
            C_train_b=eC.backward_train_plan(s.sC_train),
            C_eval_f=self._c_eval_fwd_plan(s),
        )
        s.pl.update(self._gen_plans(s))
        s.sC_bd, s.pl["C_bd_b"] = self._c_eval_bwd_plan(s)
        # the second stream's passes run beside the critical queue: one tile per workgroup (engine.short_workgroups)
        with short_workgroups():
            s.pl["C_met_f"] = eC.forward_plan(s.sC_met, False, 1.0, False)
            s.pl["K_eval_f"] = eK.forward_plan(s.sK_eval, False, w_cm, True, split_head=True)
            s.sK_bd = s.sK_eval.half_view(n, n, eK.FWD_SHARED)
            s.pl["K_bd_b"] = eK.backward_eval_plan(s.sK_bd, w_cm)
            if s.sF is not None:
                s.pl["F_f"] = self.eF.forward_plan(s.sF)
        return s

    # ---- netC's eval-mode passes of Phase G (train_generator.py:227-231): slots with their labels, forward, input-gradient backward
    def _c_eval_slots(self, s) -> None:
        eC, hw, n, lab = self.eC, self.hw, s.n, s.d_targets
        s.sC_eval = eC.slot("C.evalbd", n, hw)      # netC on the triggered images: on the critical path, so on its own
        s.sC_met = eC.slot("C.metric", n, hw)       # netC on the clean images (accuracy only): second stream
        s.sC_eval.bufs["targets"], s.sC_met.bufs["targets"] = lab[LAB_BD], lab[LAB_TARGETS]

    def _c_eval_fwd_plan(self, s):
        return self.eC.forward_plan(s.sC_eval, False, 1.0, False)

    def _c_eval_bwd_plan(self, s):
        return s.sC_eval, self.eC.backward_eval_plan(s.sC_eval, 1.0)

    def _c_eval_inputs(self, x_ptr, bd_ptr, xC, aug_ptr, n, st) -> None:
        """The augmented images of netC's differentiated eval pass (:228)."""
        ops.check(lib.combat_augment_fwd(bd_ptr, None, aug_ptr[3], n, self.hw, xC.data_ptr(), None, st), "augment 3")

    def _c_eval_grads(self, aug_ptr, n, st) -> None:
        """Image gradient of that pass through the augmentation -> d_bd."""
        s = self.cur
        ops.check(lib.combat_augment_bwd(s.sC_bd.bufs["g.img"].data_ptr(), 8, aug_ptr[3], n, self.hw,
                                         s.d_bd.data_ptr(), 0, st), "augment 3 bwd")

    def _fill_table_extra(self, hs, rnd, targets_cpu, bd_targets_cpu) -> None:
        """Entries of the step table a subclass adds (staging set `hs`, before its copy)."""

    def _bd_targets(self, targets_cpu: torch.Tensor) -> torch.Tensor:
        """The labels the poisoned images of Phase C are trained towards (train_generator.py:70-77, :181)."""
        return create_targets_bd(targets_cpu, self.opt).cpu()

    def _gen_slot(self, n):
        return self.eG.slot("G", n, self.hw)

    def _gen_plans(self, s) -> dict:
        return dict(G_f=self.eG.forward_plan(s.sG), G_b=self.eG.backward_plan(s.sG))

    def _side_stream(self) -> torch.cuda.Stream:
        if self.serial:            # kernel-level measurements: everything in line on the caller's stream
            return torch.cuda.current_stream()
        if self._side is None:
            self._side = shared_stream(self.dev, "side")
        return self._side

    # ------------------------------------------------------------------ one step
    def run(self, inputs: torch.Tensor, targets_cpu: torch.Tensor, rnd: Optional[StepRandomness] = None,
            lr_c: Optional[float] = None, lr_g: Optional[float] = None, prof: Optional[list] = None) -> None:
        """inputs: float32 [B,3,H,W] (device or pinned host); targets_cpu: int64 [B] on the host,
        as the DataLoader yields them (train_generator.py:170-171).

        The step runs on the caller's stream plus two process-wide ones (second stream, auxiliary weight-gradient
        queue); it tolerates four foreign streams in the process (4.28-4.33 ms/step; 5.4 at six: DESIGN.md section 5)."""
        self._run(inputs, targets_cpu, rnd, lr_c, lr_g, prof)

    def _run(self, inputs, targets_cpu, rnd, lr_c, lr_g, prof) -> None:
        opt = self.opt
        n = inputs.shape[0]
        s = self._setup(n)
        hw, st = self.hw, torch.cuda.current_stream().cuda_stream
        targets_cpu = targets_cpu.cpu()
        bd_targets_cpu = self._bd_targets(targets_cpu)
        if rnd is None:
            rnd = self._draw(targets_cpu, bd_targets_cpu)
        nb = rnd.num_bd
        # ---- host tables (train_generator.py:181-204: batch order [poisoned, rest of target class, others])
        perm, tot, idx_small, idx_total = poison_tables(targets_cpu, bd_targets_cpu, nb)
        hs = s._stage[s._stage_i]
        s._stage_i = (s._stage_i + 1) % self.kStage
        if hs["done"] is not None:
            hs["done"].synchronize()       # (only ever waits if the device is kStage steps behind)
        h_targets, h_tab_i, h_tab_f, h_k1 = hs["targets"], hs["tab_i"], hs["tab_f"], hs["k1"]
        h_targets[LAB_TARGETS].copy_(targets_cpu)
        h_targets[LAB_BD].copy_(bd_targets_cpu)
        h_targets[LAB_TOTAL].copy_(tot)
        h_targets[LAB_K].copy_(targets_cpu)        # (both rows)
        h_targets[LAB_K2][1].copy_(bd_targets_cpu)
        h_tab_i[0].copy_(idx_small)
        h_tab_i[1].copy_(idx_total)
        aug_ptr = []
        for i, a in enumerate(rnd.aug):
            if a is not None:
                h_tab_f[i].copy_(torch.from_numpy(a))
            aug_ptr.append(s.tab_f[i].data_ptr() if a is not None else None)
        h_k1[0].copy_(torch.from_numpy(trigger.gaussian_kernel1d(rnd.sigma_c, opt.kernel_size)))
        h_k1[1].copy_(torch.from_numpy(trigger.gaussian_kernel1d(rnd.sigma_g, opt.kernel_size)))
        self._fill_table_extra(hs, rnd, targets_cpu, bd_targets_cpu)
        # ---- the step's small copies as ONE launch (combat_copy3): table (pinned host memory, read through its device
        # mapping), batch, and the generator's re-packed output bias
        extra = self.eG.small_refresh_copy() if hasattr(self.eG, "small_refresh_copy") else None
        direct = inputs.dtype == f32 and inputs.is_contiguous() and (inputs.is_cuda or inputs.is_pinned()) and \
            tuple(inputs.shape) == tuple(s.inputs.shape)
        ops.check(lib.combat_copy3(s.tab.data_ptr(), hs["raw"].data_ptr(), hs["raw"].numel(),
                                   s.inputs.data_ptr() if direct else None, inputs.data_ptr() if direct else None,
                                   inputs.numel() * 4 if direct else 0,
                                   extra[0] if extra else None, extra[1] if extra else None, extra[2] if extra else 0, st),
                  "combat_copy3")
        hs["done"] = torch.cuda.Event()
        hs["done"].record()
        # combat_copy3 reads a pinned host batch through its device mapping, which torch's caching host allocator cannot
        # see (no event is recorded against the block, unlike copy_(non_blocking=True)): keep the batch alive in this
        # staging set until `done` has completed, so a caller may drop its pinned tensor right after run()
        hs["inputs_ref"] = inputs if direct and not inputs.is_cuda else None
        if not direct:
            s.inputs.copy_(inputs, non_blocking=True)
        eC, eG, eK, eF, pl = self.eC, self.eG, self.eK, self.eF, s.pl
        for e in (eC, eG, eK) + ((eF,) if eF is not None else ()):
            e.refresh()
        k1c, k1g = s.k1[0].data_ptr(), s.k1[1].data_ptr()
        x_ptr = s.inputs.data_ptr()

        # ---- generator forward of the whole batch, ONCE for both phases.  The reference runs netG twice
        # (train_generator.py:187 on the poisoned images in eval mode, :216 on the batch in train mode);
        # the UNet has InstanceNorm without running statistics and no dropout, and its weights only
        # change at the end of Phase G, so the first call's outputs are rows of the second's.
        self._gen_forward(x_ptr, n, st, prof)
        ev_fork = torch.cuda.Event()           # what the second stream's chain depends on (see the fork below)
        ev_fork.record()

        # ================= Phase C (train_generator.py:175-212) =================
        if nb:   # the poisoned images: rows index_small[:nb] of the batch and of the generator output (:186-194)
            self._trigger_c(x_ptr, nb, k1c, st)
        ops.check(lib.combat_augment_fwd(s.cat_src.data_ptr(), s.tab_i[1].data_ptr(), aug_ptr[0], n, hw,
                                         eC.input(s.sC_train).data_ptr(), None, st), "augment 0")
        pl["C_train_f"].run(prof)
        # ---- fork (enqueued after the surrogate forward so that the main queue is never short of work while the
        # host feeds the second stream).  Everything Phase G does with the clean model and the detector depends only on the
        # generator forward above -- not on Phase C -- so that chain (trigger, two augmentations,
        # clean-model forward + input-gradient backward: ~1.3 ms of launches that individually
        # leave most of the chip idle) runs on a second stream underneath Phase C.  It owns the clean
        # model's and the detector's engines and the buffers bd / mse / d_bd2; main waits for `ev_bd`
        # before it reads the poisoned images and for `ev_side` before the generator backward.
        side = self._side_stream()
        side.wait_event(ev_fork)
        xK, xC = eK.input(s.sK_eval), eC.input(s.sC_eval)     # [2n, ...]: metric half, loss half / netC's loss images
        bd_ptr = s.bd.data_ptr()
        with torch.cuda.stream(side):
            s2 = side.cuda_stream
            self._trigger_g(x_ptr, n, k1g, s2)                                                    # :224-226
            ev_bd = torch.cuda.Event()
            ev_bd.record()
            ops.check(lib.combat_augment_fwd(x_ptr, None, aug_ptr[1], n, hw, xK.data_ptr(), None, s2), "augment 1")  # :214
            ops.check(lib.combat_augment_fwd(bd_ptr, None, aug_ptr[4], n, hw, xK[n:].data_ptr(), None, s2), "augment 4")
            pl["K_eval_f"].run(prof)               # :214 (metric half) + :250-251 (loss half)
            pl["K_bd_b"].run(prof)
            ops.check(lib.combat_augment_bwd(s.sK_bd.bufs["g.img"].data_ptr(), 8, aug_ptr[4], n, hw,
                                             s.d_bd2.data_ptr(), 0, s2), "augment 4 bwd")
            ev_side = torch.cuda.Event()
            ev_side.record()

        self._backward_allreduce(pl["C_train_b"], eC, prof)
        eC.fp.sgd_step(float(lr_c if lr_c is not None else opt.lr_C), grad_scale=1.0 / self.world)
        if not self.keep_grads:
            eC.fp.zero_grad_behind()
        eC.mark_weights_dirty()
        eC.refresh()                       # re-pack bf16 operands, fold the new running stats

        # ================= Phase G (train_generator.py:216-255; generator forward and clean-model chain: above) =====
        torch.cuda.current_stream().wait_event(ev_bd)
        self._c_eval_inputs(x_ptr, bd_ptr, xC, aug_ptr, n, st)
        pl["C_eval_f"].run(prof)               # :228, :231
        # ---- everything that is only logged (:227 accuracy of the updated netC on the clean images, :245-247
        # detector, :234-243 L2 / gradient-L2 terms) is forked to the second stream HERE: underneath the surrogate's
        # input-gradient pass and the generator backward.  Measured on one box (ms/step): forked after the
        # input-gradient pass 4.26, here 4.18, before the surrogate's eval forward 4.23.
        ev_late = torch.cuda.Event()
        ev_late.record()
        pl["C_bd_b"].run(prof)
        self._c_eval_grads(aug_ptr, n, st)
        with torch.cuda.stream(side):
            side.wait_event(ev_late)
            s2 = side.cuda_stream
            ops.check(lib.combat_augment_fwd(x_ptr, None, aug_ptr[2], n, hw, eC.input(s.sC_met).data_ptr(), None, s2),
                      "augment 2")
            pl["C_met_f"].run(prof)
            if eF is not None:
                ops.check(lib.combat_dct_u8(bd_ptr, self.D.data_ptr(), n, hw, eF.input(s.sF).data_ptr(), s2), "dct")
                pl["F_f"].run(prof)
            self._log_terms(n, s2, s.sF.bufs["logits"] if eF is not None else None)
            ev_met = torch.cuda.Event()
            ev_met.record()
        torch.cuda.current_stream().wait_event(ev_side)     # ---- join
        self._gen_backward(x_ptr, n, k1g, st, prof)
        eG.fp.sgd_step(float(lr_g if lr_g is not None else opt.lr_G), grad_scale=1.0 / self.world)
        if not self.keep_grads:
            eG.fp.zero_grad_behind()
        eG.mark_weights_dirty()
        # the next step rewrites the images, the step table and netC's operands under the second stream's readers
        torch.cuda.current_stream().wait_event(ev_met)
        self.samples += n
        self.steps_done += 1

    # ------------------------------------------------------------------ trigger-specific pieces (UNet + low-pass / clamp-mix / blur)
    def _draw(self, targets_cpu, bd_targets_cpu) -> StepRandomness:
        return draw_randomness(targets_cpu, bd_targets_cpu, self.opt, self.transforms, self.sigma_range)

    def _gen_forward(self, x_ptr, n, st, prof) -> None:
        s = self.cur
        ops.check(lib.combat_image_to_c8(x_ptr, n, self.hw, self.eG.input(s.sG).data_ptr(), st), "c8 G")
        s.pl["G_f"].run(prof)

    def _trigger_c(self, x_ptr, nb, k1c, st) -> None:
        """Poisoned images of Phase C -> cat_src[n:] (train_generator.py:186-194)."""
        s = self.cur
        ops.check(lib.combat_trigger_fwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1c, float(self.opt.noise_rate),
                                         nb, self.hw, s.tab_i[0].data_ptr(), s.cat_src[s.n:].data_ptr(), None, None, st),
                  "trigger C")

    def _trigger_g(self, x_ptr, n, k1g, s2) -> None:
        """Triggered copy of the whole batch -> self.bd (+ per-plane squared error) (train_generator.py:224-226)."""
        s = self.cur
        ops.check(lib.combat_trigger_fwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g, float(self.opt.noise_rate),
                                         n, self.hw, None, s.bd.data_ptr(), None, s.mse.data_ptr(), s2), "trigger G")

    def _log_terms(self, n, s2, f_logits) -> None:
        """loss_l2 / loss_grad_l2 running sums (train_generator.py:234-243; the second is logged only) and the
        detector's hit count (:245-247), in one launch (the ATen spelling of the same is _grad_l2 below: 14 launches)."""
        s = self.cur
        ops.check(lib.combat_log_terms(s.inputs.data_ptr(), s.bd.data_ptr(), s.mse.data_ptr(), n, self.hw,
                                       f_logits.data_ptr() if f_logits is not None else None, self.acc.data_ptr(),
                                       self.acc_side.data_ptr(), s2), "log terms")

    def _gen_backward(self, x_ptr, n, k1g, st, prof) -> None:
        """Image gradient (d_bd + d_bd2) + the L2 term -> generator parameter gradients (train_generator.py:253-254)."""
        s, hw = self.cur, self.hw
        l2_scale = float(self.opt.L2_weight) / float(n * 3 * hw * hw)          # :234, :253
        ops.check(lib.combat_trigger_bwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g, float(self.opt.noise_rate),
                                         n, hw, s.d_bd.data_ptr(), s.d_bd2.data_ptr(), s.bd.data_ptr(), l2_scale, 1,
                                         s.sG.buf("g.z", (n, hw, hw, 8)).data_ptr(), st), "trigger bwd")   # d_bd + d_bd2
        self._backward_allreduce(s.pl["G_b"], self.eG, prof)

    @staticmethod
    def _grad_l2(x: torch.Tensor, xb: torch.Tensor) -> torch.Tensor:
        """train_generator.py:235-243 (logged, not part of the loss)."""
        F = torch.nn.functional
        e, eb = F.pad(x, (1, 1, 2, 1)), F.pad(xb, (1, 1, 2, 1))
        return F.mse_loss(e[:, :, 1:] - e[:, :, :-1], eb[:, :, 1:] - eb[:, :, :-1]) + \
            F.mse_loss(e[:, :, :, 1:] - e[:, :, :, :-1], eb[:, :, :, 1:] - eb[:, :, :, :-1])

    def _backward_allreduce(self, plan, eng, prof) -> None:
        backward_allreduce(plan, eng, self.pg, self.world, self._reducers, prof)

    # ------------------------------------------------------------------ metrics
    def read_metrics(self, reset: bool = False) -> Dict[str, float]:
        """One host sync: the running sums the reference prints each step (:257-290), over every
        batch size run since the last reset."""
        acc = self.acc.cpu()
        total = max(float(self.samples), 1.0)
        w_cm = float(self.opt.clean_model_weight) or 1.0
        out = {"samples": total, "loss_c_sum": 0.0, "loss_ce_sum": 0.0, "clean_model_loss_sum": 0.0,
               "loss_l2_sum": float(acc[0]), "loss_grad_l2_sum": float(acc[1]), "clean_correct": 0, "bd_correct": 0,
               "f_correct": int(self.acc_side.cpu()), "clean_model_correct": 0, "clean_model_bd_ba": 0, "clean_model_bd_asr": 0,
               "train_correct": 0}
        for s in self._sets.values():
            sKe, sCm = s.sK_eval, s.sC_met
            cC, cE, kE = self.eC.head_bufs(s.sC_train), self.eC.head_bufs(s.sC_eval), self.eK.head_bufs(sKe)
            out["loss_c_sum"] += float(cC["loss"])
            out["loss_ce_sum"] += float(cE["loss"])
            out["clean_model_loss_sum"] += float(kE["loss"]) / w_cm
            out["clean_correct"] += int(self.eC.head_bufs(sCm)["correct"][0])
            out["bd_correct"] += int(cE["correct"][0])
            out["clean_model_correct"] += int(sKe.bufs["correct0"][0])
            out["clean_model_bd_ba"] += int(kE["correct"][0])
            out["clean_model_bd_asr"] += int(kE["correct"][1])
            out["train_correct"] += int(cC["correct"][0])
        if reset:
            self.reset_metrics()
        return out

    def reset_metrics(self) -> None:
        self.samples = 0
        self.acc.zero_()
        self.acc_side.zero_()
        for s in self._sets.values():
            for eng, slot in ((self.eC, s.sC_train), (self.eC, s.sC_eval), (self.eK, s.sK_eval), (self.eC, s.sC_met)):
                h = eng.head_bufs(slot)
                h["loss"].zero_()
                h["correct"].zero_()
                for k in ("loss0", "correct0"):
                    if k in slot.bufs:
                        slot.bufs[k].zero_()


class WanetStep(AlternatedStep):
    """The alternated step with the warping trigger (reference train_generator_wanet.py:132-237): the generator is a
    GridGenerator whose [2][S][S] field is bicubically upsampled, blended with the identity grid at ``grid_rescale``
    and used to ``grid_sample`` the images (:151-157, :196-202); loss_l2 = MSE(noise_grid, 0) (:212).  Phase
    structure, streams, poison selection, augmentation, classifiers and optimisers are AlternatedStep's.  No Gaussian
    blur is drawn (the reference's WaNet loop has none), so the torch RNG stream is consumed by the augmentation only."""

    WARP_GROUPS = 8     # image ranges of the warp backward (partial sums: deterministic, no atomics)

    def __init__(self, netC, netG, clean_model, netF, opt, process_group=None):
        super().__init__(netC, netG, clean_model, netF, opt, process_group)
        self._wpartial = torch.zeros(self.WARP_GROUPS, self.hw, self.hw, 2, dtype=f32, device=self.dev)   # (shared by all batch sizes)

    def _draw(self, targets_cpu, bd_targets_cpu) -> StepRandomness:
        """train_generator_wanet.py:148, :159, :182, :203-204, :226: num_bd and five augmentation calls -- no blur."""
        num_bd = draw_num_bd(targets_cpu, bd_targets_cpu, self.opt.pc)
        return StepRandomness(num_bd, 0.5, 0.5, [self.transforms.sample(targets_cpu.shape[0]) for _ in range(5)])

    def _gen_slot(self, n):
        return None

    def _gen_plans(self, s) -> dict:
        return {}

    def _gen_forward(self, x_ptr, n, st, prof) -> None:
        self.g = self.eG.forward_grid(self.hw, float(self.opt.grid_rescale), st)

    def _trigger_c(self, x_ptr, nb, k1c, st) -> None:
        s = self.cur
        ops.check(lib.combat_warp_fwd(x_ptr, s.tab_i[0].data_ptr(), self.g["grid"].data_ptr(), 0, nb, self.hw,
                                      s.cat_src[s.n:].data_ptr(), st), "warp C")

    def _trigger_g(self, x_ptr, n, k1g, s2) -> None:
        ops.check(lib.combat_warp_fwd(x_ptr, None, self.g["grid"].data_ptr(), 0, n, self.hw, self.cur.bd.data_ptr(), s2), "warp G")

    def _log_terms(self, n, s2, f_logits) -> None:
        if f_logits is not None:
            self.acc_side += (f_logits.argmax(1) == 1).sum()
        ng = self.g["noise_grid"]                      # [H][H][2]; the reference's noise_grid is B equal copies
        self.acc[0] += ng.pow(2).mean()
        F = torch.nn.functional
        e = F.pad(ng[None], (1, 1, 2, 1))              # F.pad of the [B, H, H, 2] tensor pads (H, 2): reproduce that (:214)
        self.acc[1] += (e[:, :, 1:] - e[:, :, :-1]).pow(2).mean() + (e[:, :, :, 1:] - e[:, :, :, :-1]).pow(2).mean()

    def _gen_backward(self, x_ptr, n, k1g, st, prof) -> None:
        eG, s = self.eG, self.cur
        ops.check(_zero_grad_call(eG.fp, st), "zero_grad G")
        ops.check(lib.combat_warp_bwd(x_ptr, s.d_bd.data_ptr(), s.d_bd2.data_ptr(), self.g["grid"].data_ptr(), 0, n, self.hw,
                                      self.WARP_GROUPS, self._wpartial.data_ptr(), st), "warp bwd")
        eG.backward_field(self._wpartial, self.WARP_GROUPS, self.hw, float(self.opt.grid_rescale), float(self.opt.L2_weight), st)
        if self.world > 1:
            # only fc1.bias, fc2.weight and fc2.bias ever receive a gradient (GridEngine): one contiguous range of
            # ~640 floats travels, not the 19-MB flat buffer whose remainder is exactly zero on every rank
            lo, hi = eG.head_grad_range()
            torch.distributed.all_reduce(eG.fp.grad[lo:hi], group=self.pg)


@dataclass
class InputAwareRandomness(StepRandomness):
    """The draws of one input-aware step (train_generator_inputaware.py:189-252): StepRandomness plus the blur of the
    cross images (sigma_x) and a sixth augmentation table, aug[5] (the cross images' transform, :241)."""

    sigma_x: float = 0.5


class InputAwareStep(AlternatedStep):
    """The alternated step of the input-aware trigger (reference train_generator_inputaware.py:170-266).  Phase C is
    AlternatedStep's.  In Phase G the generator also runs on a second, independently shuffled batch ``inputs2``; its
    noise is mixed onto the FIRST batch's images (``bd2``) and the surrogate is trained to keep their clean labels
    (loss ``cross_weight * CE(netC(aug5(bd2)), targets)``, :245, :250-253).

    The generator runs over [inputs ; inputs2] in one 2n slot (InstanceNorm is per sample and the UNet has no dropout,
    so this is the reference's two calls, :231 and :236, and Phase C reads rows of the first half); its forward runs
    the n-image plan on each half (see _gen_plans), its backward is one 2n pass.  netC's two differentiated eval
    passes [aug3(bd) ; aug5(bd2)] share one 2n slot with two loss halves (engine two_loss / half_weights: the n-image
    plans over its halves, so d_bd is AlternatedStep's for the same images); the paired trigger (combat_trigger_pair_fwd / _bwd) makes bd and bd2 in one launch and returns
    the gradient of both noises in one launch.  The blur is the reference's module-level GaussianBlur (:53): kernel 3,
    sigma in (0.1, 1), whatever --kernel_size / --sigma say (FIXED_BLUR)."""

    TABLE = (6, 3, 9)   # + the cross images' augmentation table, the blur kernel of sigma_x, the LAB_CROSS rows
    FIXED_BLUR = True
    _inputs2_src = None

    def run(self, inputs: torch.Tensor, targets_cpu: torch.Tensor, inputs2: torch.Tensor,
            rnd: Optional[InputAwareRandomness] = None, lr_c: Optional[float] = None, lr_g: Optional[float] = None,
            prof: Optional[list] = None) -> None:
        """inputs2: the second loader's batch (same size as inputs; device or pinned host).  lr_g defaults to the
        reference's generator rate lr_C * 0.1 (:122)."""
        if tuple(inputs2.shape) != tuple(inputs.shape):
            raise ValueError("InputAwareStep: inputs2 %s must have the shape of inputs %s"
                             % (tuple(inputs2.shape), tuple(inputs.shape)))
        self._inputs2_src = inputs2
        if lr_g is None:
            lr_g = float(self.opt.lr_C) * 0.1
        try:
            super().run(inputs, targets_cpu, rnd, lr_c, lr_g, prof)
        finally:
            self._inputs2_src = None

    # ---- buffers, table, plans
    def _build_set(self, n: int):
        s = super()._build_set(n)
        dev, hw = self.dev, self.hw
        s.inputs2 = torch.empty(n, 3, hw, hw, dtype=f32, device=dev)
        s.bd2 = torch.empty(n, 3, hw, hw, dtype=f32, device=dev)       # inputs_bd2 (:238)
        s.d_cross = torch.empty(n, 3, hw, hw, dtype=f32, device=dev)   # its gradient
        return s

    def _fill_table_extra(self, hs, rnd, targets_cpu, bd_targets_cpu) -> None:
        hs["k1"][2].copy_(torch.from_numpy(trigger.gaussian_kernel1d(rnd.sigma_x, self.opt.kernel_size)))
        hs["targets"][LAB_CROSS][0].copy_(bd_targets_cpu)
        hs["targets"][LAB_CROSS][1].copy_(targets_cpu)

    def _gen_slot(self, n):
        return self.eG.slot("G.pair", 2 * n, self.hw)

    def _gen_plans(self, s) -> dict:
        """The generator over [inputs ; inputs2] runs the n-image plans on the two halves of the 2n slot (views of its
        buffers), forward and backward.  A 2n-image plan picks other tile and statistics partitions, and the UNet's
        bf16 activations and 2 x 2 / 4 x 4 InstanceNorms amplify the different rounding to ~1 % of its output; with the
        n-image plans the first half is AlternatedStep's generator pass bit for bit.  The 2n forward plan is only built
        (it allocates the 2n buffers the halves view), never run."""
        eG, sG = self.eG, s.sG
        n, hw = s.n, self.hw
        eG.forward_plan(sG)
        sG.buf("g.z", (2 * n, hw, hw, 8))
        share = tuple(k for k, v in sG.bufs.items() if v.dim() and v.shape[0] == sG.N)
        halves = [sG.half_view(k * n, n, share) for k in range(2)]
        fwd = PlanSeq("unet.fwd.halves", [eG.forward_plan(h) for h in halves])
        s._gen_bwd = [eG.backward_plan(h) for h in halves]
        # a half's output must land in the 2n slot ('<layer>.part': statistics partials of the half's own forward)
        for h in halves:
            bad = [k for k in h.bufs if k in sG.bufs and k not in share and not k.endswith(".part")]
            assert not bad, "generator buffers not batch-major: %s" % bad
        if getattr(self, "_g_cross", None) is None:
            self._g_cross = torch.zeros_like(eG.fp.grad)     # the cross half's generator gradient (shared by all batch sizes)
        return dict(G_f=fwd)

    def _c_eval_slots(self, s) -> None:
        s.sC_eval = self.eC.slot("C.cross2", 2 * s.n, self.hw)   # [aug3(bd) ; aug5(bd2)]: both halves differentiated
        s.sC_met = self.eC.slot("C.metric", s.n, self.hw)
        s.sC_eval.bufs["targets"], s.sC_met.bufs["targets"] = s.d_targets[LAB_CROSS].view(-1), s.d_targets[LAB_TARGETS]

    def _c_eval_fwd_plan(self, s):
        return self.eC.forward_plan(s.sC_eval, False, 1.0, False, two_loss=True)

    def _c_eval_bwd_plan(self, s):
        return s.sC_eval, self.eC.backward_eval_plan(s.sC_eval, 1.0, half_weights=(1.0, float(self.opt.cross_weight)))

    # ---- the step's pieces
    def _draw(self, targets_cpu, bd_targets_cpu) -> InputAwareRandomness:
        """Reference order (:189-252): num_bd, sigma_c (only if num_bd > 0), aug0, aug1, sigma_g, sigma_x, aug2, aug5
        (cross images, :241), aug3, aug4."""
        n = targets_cpu.shape[0]
        num_bd = draw_num_bd(targets_cpu, bd_targets_cpu, self.opt.pc)
        sigma_c = trigger.sample_sigma(self.sigma_range) if num_bd else 0.5
        aug0, aug1 = self.transforms.sample(n), self.transforms.sample(n)
        sigma_g = trigger.sample_sigma(self.sigma_range)
        sigma_x = trigger.sample_sigma(self.sigma_range)
        aug2, aug5, aug3, aug4 = (self.transforms.sample(n) for _ in range(4))
        return InputAwareRandomness(num_bd, sigma_c, sigma_g, [aug0, aug1, aug2, aug3, aug4, aug5], sigma_x=sigma_x)

    def _gen_forward(self, x_ptr, n, st, prof) -> None:
        """netG over [inputs ; inputs2].  The second batch's copy sits next to the step's combat_copy3 (it comes from
        its own loader's pinned ring)."""
        s = self.cur
        s.inputs2.copy_(self._inputs2_src, non_blocking=True)
        gin = self.eG.input(s.sG)
        ops.check(lib.combat_image_to_c8(x_ptr, n, self.hw, gin.data_ptr(), st), "c8 G")
        ops.check(lib.combat_image_to_c8(s.inputs2.data_ptr(), n, self.hw, gin[n:].data_ptr(), st), "c8 G2")
        s.pl["G_f"].run(prof)

    def _trigger_g(self, x_ptr, n, k1g, s2) -> None:
        """inputs_bd (blur sigma_g, + squared-error partials) and inputs_bd2 (sigma_x), both on the first batch's
        images (:231-238): one launch."""
        s = self.cur
        ops.check(lib.combat_trigger_pair_fwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g,
                                              float(self.opt.noise_rate), n, self.hw, s.bd.data_ptr(),
                                              s.bd2.data_ptr(), s.mse.data_ptr(), s2), "trigger pair")

    def _c_eval_inputs(self, x_ptr, bd_ptr, xC, aug_ptr, n, st) -> None:
        hw = self.hw
        ops.check(lib.combat_augment_fwd(bd_ptr, None, aug_ptr[3], n, hw, xC.data_ptr(), None, st), "augment 3")
        ops.check(lib.combat_augment_fwd(self.cur.bd2.data_ptr(), None, aug_ptr[5], n, hw, xC[n:].data_ptr(), None, st),
                  "augment 5")

    def _c_eval_grads(self, aug_ptr, n, st) -> None:
        s = self.cur
        g = s.sC_eval.bufs["g.img"]
        ops.check(lib.combat_augment_bwd(g.data_ptr(), 8, aug_ptr[3], n, self.hw, s.d_bd.data_ptr(), 0, st),
                  "augment 3 bwd")
        ops.check(lib.combat_augment_bwd(g[n:].data_ptr(), 8, aug_ptr[5], n, self.hw, s.d_cross.data_ptr(), 0, st),
                  "augment 5 bwd")

    def _gen_backward(self, x_ptr, n, k1g, st, prof) -> None:
        """Both noises' gradients in one launch (rows [0, n): d_bd + d_bd2 + the L2 term; rows [n, 2n): d_cross), then
        the generator backward of each half (:253-254).  A backward plan starts by zeroing the gradient buffer, so the
        cross half runs first and its gradient is set aside; the first half's backward is then AlternatedStep's, and
        the cross gradient is added to it (exactly nothing at cross_weight 0)."""
        s, hw = self.cur, self.hw
        l2_scale = float(self.opt.L2_weight) / float(n * 3 * hw * hw)
        ops.check(lib.combat_trigger_pair_bwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g,
                                              float(self.opt.noise_rate), n, hw, s.d_bd.data_ptr(),
                                              s.d_bd2.data_ptr(), s.bd.data_ptr(), l2_scale, s.d_cross.data_ptr(),
                                              1, s.sG.buf("g.z", (2 * n, hw, hw, 8)).data_ptr(), st), "trigger pair bwd")
        grad = self.eG.fp.grad
        s._gen_bwd[1].run(prof)
        self._g_cross.copy_(grad)
        s._gen_bwd[0].run(prof)
        grad.add_(self._g_cross)
        if self.world > 1 or (FORCE_ALLREDUCE and self.pg is not None):
            torch.distributed.all_reduce(grad, group=self.pg)   # one flat all-reduce

    # ---- metrics
    def read_metrics(self, reset: bool = False) -> Dict[str, float]:
        """AlternatedStep's keys plus loss_cross_sum (sum of the per-step CE(pred_cross, targets)) and cross_correct
        (#argmax(pred_cross) == targets, :275)."""
        out = super().read_metrics(reset=False)
        out["loss_cross_sum"], out["cross_correct"] = 0.0, 0
        for s in self._sets.values():
            out["loss_cross_sum"] += float(s.sC_eval.bufs["loss1"])
            out["cross_correct"] += int(s.sC_eval.bufs["correct1"][0])
        if reset:
            self.reset_metrics()
        return out

    def reset_metrics(self) -> None:
        super().reset_metrics()
        for s in self._sets.values():
            for k in ("loss1", "correct1"):
                if k in s.sC_eval.bufs:
                    s.sC_eval.bufs[k].zero_()


LAB_Y = 7   # multi-label only: one int64 row read as int32 [2n] -- the generator's labels of Phase C, then of Phase G


def chunk_size(bs: int, num_classes: int) -> int:
    """ps of train_generator_multilabel.py:203: the generator phase cuts the batch into chunks of ps images."""
    return (bs - 1) // num_classes + 1


@dataclass
class MultiLabelRandomness(StepRandomness):
    """The draws of one multi-label step (train_generator_multilabel.py:171-236): StepRandomness with one blur sigma per
    chunk of the generator phase (sigma_chunks[ci], :217) in place of sigma_g, which is unused."""

    sigma_chunks: List[float] = field(default_factory=list)


class MultiLabelStep(AlternatedStep):
    """The alternated step of the multi-target-label attack (reference train_generator_multilabel.py:160-262) around the
    label-conditioned generator (nets.CUnetGeneratorv1, engine.CUnetEngine).

    Phase C (:164-190): num_bd = sum(rand(bs) < pc) over the whole batch, the poisoned images are the FIRST num_bd of
    the batch in order, the generator is conditioned on their own labels and the targets stay as they are.
    Phase G (:192-242): the batch is cut into chunks of ps = (bs - 1) // num_classes + 1 images; chunk ci is conditioned
    on class ci and blurred with its own draw of the module-level GaussianBlur (:53; FIXED_BLUR); the loop ends with the
    batch (bs = 16 on CIFAR-10: classes 0..7).  loss = CE(netC(bd), chunk classes) + L2_weight * MSE(bd, inputs)
    + clean_model_weight * CE(clean(bd), targets) (:240; the gradient-L2 term of train_generator.py is absent).  bd_correct
    and the clean model's ASR are scored against the chunk classes, its Bd BA against the clean labels (:226, :250-251).

    Unlike AlternatedStep the two phases condition the generator differently, so it runs twice: an n-image forward
    over the targets (slot 'G.c', only when num_bd > 0; the reference runs it on the num_bd images alone) and the
    n-image forward + backward over the chunk classes (slot 'G').  Both read the same input buffer.  Labels travel in
    the step table (row LAB_Y as int32 [2n]); the per-chunk blur kernels are rows 1.. of its blur section, consumed by
    ONE combat_trigger_groups_fwd / _bwd launch.  Single rank only."""

    FIXED_BLUR = True

    def __init__(self, netC, netG, clean_model, netF, opt, process_group=None):
        if process_group is not None and torch.distributed.get_world_size(process_group) > 1:
            raise ValueError("MultiLabelStep runs on one rank only: data parallelism is not implemented for the "
                             "multi-label attack (got a process group of %d ranks)"
                             % torch.distributed.get_world_size(process_group))
        if getattr(netG, "arch", "") != "cunet":
            raise ValueError("MultiLabelStep needs the label-conditioned generator (nets.CUnetGeneratorv1), got %s"
                             % type(netG).__name__)
        if int(netG.num_classes) != int(opt.num_classes):
            raise ValueError("MultiLabelStep: the generator conditions on %d classes, opt.num_classes is %d"
                             % (netG.num_classes, opt.num_classes))
        # augmentation tables, blur kernels (sigma_c + one per chunk, at most num_classes), label rows (+ LAB_Y)
        self.TABLE = (5, 1 + int(opt.num_classes), 8)
        super().__init__(netC, netG, clean_model, netF, opt, None)

    def run(self, inputs: torch.Tensor, targets_cpu: torch.Tensor, rnd: Optional[MultiLabelRandomness] = None,
            lr_c: Optional[float] = None, lr_g: Optional[float] = None, prof: Optional[list] = None) -> None:
        """lr_g defaults to the reference's generator rate lr_C * 0.1 (:115)."""
        if lr_g is None:
            lr_g = float(self.opt.lr_C) * 0.1
        super().run(inputs, targets_cpu, rnd, lr_c, lr_g, prof)

    # ---- table, slots, plans
    def _bd_targets(self, targets_cpu: torch.Tensor) -> torch.Tensor:
        """Phase C leaves the targets unchanged (:180): every image is 'of its target class', so the poisoned ones are
        the first num_bd of the batch in order and total_targets == targets."""
        return targets_cpu.clone()

    def _fill_table_extra(self, hs, rnd, targets_cpu, bd_targets_cpu) -> None:
        n = targets_cpu.shape[0]
        ps = chunk_size(n, int(self.opt.num_classes))
        groups = (n + ps - 1) // ps
        if len(rnd.sigma_chunks) < groups:
            raise ValueError("MultiLabelStep: %d chunks need %d blur sigmas, got %d" % (groups, groups, len(rnd.sigma_chunks)))
        chunk = torch.arange(n, dtype=torch.int64) // ps          # (:214: tmp = targets[si:ei] * 0 + ci)
        lab = hs["targets"]
        lab[LAB_BD].copy_(chunk)                                   # netC's loss and bd_correct (:226-228)
        lab[LAB_K2][1].copy_(chunk)                                # the clean model's ASR (:251)
        y = lab[LAB_Y].view(torch.int32)
        y[:n].copy_(targets_cpu)                                   # Phase C: the images' own labels (:173-176)
        y[n:].copy_(chunk)                                         # Phase G
        for ci in range(groups):
            hs["k1"][1 + ci].copy_(torch.from_numpy(trigger.gaussian_kernel1d(rnd.sigma_chunks[ci], self.opt.kernel_size)))
        self.cur.nb, self.cur.ps = rnd.num_bd, ps      # (read by this step's hooks below, from the set they run on)

    def _gen_plans(self, s) -> dict:
        eG, n = self.eG, s.n
        y = s.d_targets[LAB_Y].view(torch.int32)
        s.sG.bufs["y"] = y[n:]
        s.sGc = eG.slot("G.c", n, self.hw)
        s.sGc.bufs["y"] = y[:n]
        s.sGc.bufs["x"] = eG.input(s.sG)                           # one image buffer for both passes
        return dict(G_f=eG.forward_plan(s.sG), G_b=eG.backward_plan(s.sG), Gc_f=eG.forward_plan(s.sGc))

    # ---- the step's pieces
    def _draw(self, targets_cpu, bd_targets_cpu) -> MultiLabelRandomness:
        """Reference order: num_bd (:171), sigma_c (:176, only if num_bd > 0), aug0 (:179), aug1 (:190), aug2 (:199:
        pred_clean's transform comes first in Phase G), one sigma per chunk (:217), aug3 (:225), aug4 (:236)."""
        n = targets_cpu.shape[0]
        num_bd = int(np.sum(np.random.rand(n) < self.opt.pc))
        sigma_c = trigger.sample_sigma(self.sigma_range) if num_bd else 0.5
        aug0, aug1, aug2 = (self.transforms.sample(n) for _ in range(3))
        ps = chunk_size(n, int(self.opt.num_classes))
        sig = [trigger.sample_sigma(self.sigma_range) for _ in range((n + ps - 1) // ps)]
        aug3, aug4 = self.transforms.sample(n), self.transforms.sample(n)
        return MultiLabelRandomness(num_bd, sigma_c, sig[0], [aug0, aug1, aug2, aug3, aug4], sigma_chunks=sig)

    def _gen_forward(self, x_ptr, n, st, prof) -> None:
        s = self.cur
        ops.check(lib.combat_image_to_c8(x_ptr, n, self.hw, self.eG.input(s.sG).data_ptr(), st), "c8 G")
        if s.nb:
            s.pl["Gc_f"].run(prof)      # conditioned on the targets: Phase C's poisoned images
        s.pl["G_f"].run(prof)           # conditioned on the chunk classes: Phase G

    def _trigger_c(self, x_ptr, nb, k1c, st) -> None:
        s = self.cur
        ops.check(lib.combat_trigger_fwd(x_ptr, self.eG.output(s.sGc).data_ptr(), self.P.data_ptr(), k1c, float(self.opt.noise_rate),
                                         nb, self.hw, s.tab_i[0].data_ptr(), s.cat_src[s.n:].data_ptr(), None, None, st),
                  "trigger C")

    def _trigger_g(self, x_ptr, n, k1g, s2) -> None:
        s = self.cur
        ops.check(lib.combat_trigger_groups_fwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g,
                                                float(self.opt.noise_rate), n, self.hw, s.ps, s.bd.data_ptr(),
                                                s.mse.data_ptr(), s2), "trigger groups")

    def _gen_backward(self, x_ptr, n, k1g, st, prof) -> None:
        s, hw = self.cur, self.hw
        l2_scale = float(self.opt.L2_weight) / float(n * 3 * hw * hw)          # :229, :240
        ops.check(lib.combat_trigger_groups_bwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g,
                                                float(self.opt.noise_rate), n, hw, s.ps, s.d_bd.data_ptr(),
                                                s.d_bd2.data_ptr(), s.bd.data_ptr(), l2_scale, 1,
                                                s.sG.buf("g.z", (n, hw, hw, 8)).data_ptr(), st), "trigger groups bwd")
        self._backward_allreduce(s.pl["G_b"], self.eG, prof)


class ImperceptibleStep(AlternatedStep):
    """The alternated step of the reference's imperceptible configuration (train_generator_imperceptible.py:160-277):
    AlternatedStep with the smoothness of the triggered images in the generator's loss,

        loss = loss_ce + L2_weight * loss_l2 + tv_weight * loss_tv + clean_model_weight * clean_model_loss   (:234-237)
        loss_tv = total_variation(inputs_bd).mean()                                                           (:228)

    total_variation (kornia 0.6.6) is, per image, the sum over C, H, W of |x[..., 1:, :] - x[..., :-1, :]| plus the same
    along W.  It is restated in the kernels (combat_trigger_tv_fwd / _bwd), not pinned against kornia.  The per-plane
    sums come out of the Phase-G trigger launch, the sign stencil of the gradient joins the image gradient inside the
    trigger backward launch, and the logged sum rides in the log-terms launch: the step's launch count is the parent's.
    Phase C, the draws' order and the networks are the parent's; like the input-aware script, the reference blurs with
    the module-level T.GaussianBlur(kernel_size=3, sigma=(0.1, 1)) (:52), whatever --kernel_size / --sigma say.  At
    tv_weight 0 the trigger backward is the parent's launch, and the step leaves the parent's bits.  Images larger
    than 64 pixels (ImageNet-10's 224 x 224) take combat_trigger_tv_big_fwd / _bwd, the strip route: the sums come from
    the reduction launch behind the strip forward (where the parent has its squared-error launch), the stencil reads
    inputs_bd across the strips' seams; the launch count is the parent's there too."""

    FIXED_BLUR = True    # (the draws keep the parent's order: one sigma per create_inputs_bd call, :172-174 and :203)

    def _build_set(self, n: int):
        s = super()._build_set(n)
        s.tv = torch.empty(3 * n, dtype=f32, device=self.dev)   # per (image, channel) total variation of inputs_bd
        return s

    def _trigger_g(self, x_ptr, n, k1g, s2) -> None:
        """inputs_bd of the whole batch (:203) with its squared-error and total-variation partials."""
        s = self.cur
        fwd = lib.combat_trigger_tv_big_fwd if self.hw > 64 else lib.combat_trigger_tv_fwd      # strips / whole planes
        ops.check(fwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g, float(self.opt.noise_rate), n,
                      self.hw, s.bd.data_ptr(), s.mse.data_ptr(), s.tv.data_ptr(), s2), "trigger tv G")

    def _log_terms(self, n, s2, f_logits) -> None:
        """The parent's logged terms + loss_tv (:228, :245) -> acc[2]."""
        s = self.cur
        ops.check(lib.combat_log_terms_tv(s.inputs.data_ptr(), s.bd.data_ptr(), s.mse.data_ptr(), s.tv.data_ptr(),
                                          n, self.hw, f_logits.data_ptr() if f_logits is not None else None,
                                          self.acc.data_ptr(), self.acc_side.data_ptr(), s2), "log terms tv")

    def _gen_backward(self, x_ptr, n, k1g, st, prof) -> None:
        """The parent's, with tv_weight * d loss_tv / d inputs_bd in the image gradient (:234-239)."""
        s, hw = self.cur, self.hw
        l2_scale = float(self.opt.L2_weight) / float(n * 3 * hw * hw)
        tv_scale = float(self.opt.tv_weight) / float(n)                        # .mean() over the batch (:228)
        bwd = lib.combat_trigger_tv_big_bwd if hw > 64 else lib.combat_trigger_tv_bwd
        ops.check(bwd(x_ptr, self.eG.output(s.sG).data_ptr(), self.P.data_ptr(), k1g, float(self.opt.noise_rate), n, hw,
                      s.d_bd.data_ptr(), s.d_bd2.data_ptr(), s.bd.data_ptr(), l2_scale, tv_scale, 1,
                      s.sG.buf("g.z", (n, hw, hw, 8)).data_ptr(), st), "trigger tv bwd")
        self._backward_allreduce(s.pl["G_b"], self.eG, prof)

    def read_metrics(self, reset: bool = False) -> Dict[str, float]:
        """AlternatedStep's keys plus loss_tv_sum, the sum of the per-step loss_tv (:245; "TV Loss" = / samples)."""
        out = super().read_metrics(reset=False)
        out["loss_tv_sum"] = float(self.acc[2])
        if reset:
            self.reset_metrics()
        return out


class ClassifierStep(PerBatchSize):
    """Phase-C-only training step: the loop bodies of train_clean_classifier.py:75-121 (no generator) and
    train_victim.py:102-141 (frozen generator poisons the images the dataset flags).  Batch order as in
    the victim script: [poisoned images with the trigger, all other images] (:125-127)."""

    def __init__(self, netC, opt, netG=None, process_group=None):
        self.opt, self.netC, self.netG = opt, netC, netG
        self.dev = next(netC.parameters()).device
        self.eC: PreActEngine = netC._net_engine()
        self.eG = netG._net_engine() if netG is not None else None      # UnetEngine, or GridEngine (WaNet)
        # train_victim_wanet.py:85-96: the frozen GridGenerator's field warps the poisoned images (no low-pass, no blur)
        self.wanet = netG is not None and getattr(netG, "arch", "") == "gridgen"
        if netG is not None and getattr(netG, "arch", "") not in ("unet", "gridgen"):
            raise ValueError("ClassifierStep: unsupported generator %r (UnetGenerator or GridGenerator expected)" % type(netG).__name__)
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.hw = opt.input_height
        self.P = trigger.lowpass_matrix(self.hw, opt.ratio).to(self.dev)
        self.k1 = torch.zeros(3, dtype=f32, device=self.dev)
        self.transforms = PostTensorTransform(opt)
        self._sets: Dict[int, SimpleNamespace] = {}
        self._small: Dict[int, tuple] = {}
        self._reducers: Dict = {}

    def _build_set(self, n: int) -> SimpleNamespace:
        hw, dev = self.hw, self.dev
        s = SimpleNamespace(n=n)
        s.cat_src = torch.zeros(2 * n, 3, hw, hw, dtype=f32, device=dev)
        s.tab_i = torch.zeros(2, n, dtype=torch.int32, device=dev)
        s.tab_f = torch.zeros(n, 4, dtype=f32, device=dev)
        s.slot = self.eC.slot("V.train", n, hw)
        s.fwd = self.eC.forward_plan(s.slot, True)
        s.bwd = self.eC.backward_train_plan(s.slot)
        return s

    def run(self, inputs: torch.Tensor, targets_cpu: torch.Tensor, poisoned_cpu: Optional[torch.Tensor] = None,
            lr: Optional[float] = None) -> None:
        opt = self.opt
        n = inputs.shape[0]
        s = self._setup(n)
        hw, st = self.hw, torch.cuda.current_stream().cuda_stream
        targets_cpu = targets_cpu.cpu()
        if poisoned_cpu is None or self.eG is None:
            poisoned_cpu = torch.zeros(n, dtype=torch.bool)
        trg = poisoned_cpu.cpu().nonzero()[:, 0]
        ntrg = (~poisoned_cpu.cpu()).nonzero()[:, 0]      # intent of train_victim.py:121
        nb = int(trg.numel())
        perm, idx_small, idx_total = order_tables(trg, ntrg, nb)
        tot = targets_cpu[perm.long()].clone()
        if nb:
            tot[:nb] = create_targets_bd(targets_cpu[trg], opt)
        s.tab_i.copy_(torch.stack([idx_small, idx_total]))
        self.last_poisoned = (trg, nb)     # (image logging: train_victim_wanet.py:127-133)
        aug = self.transforms.sample(n)
        if aug is not None:
            s.tab_f.copy_(torch.from_numpy(aug))
        s.cat_src[:n].copy_(inputs)
        h = self.eC.head_bufs(s.slot)
        h["targets"].copy_(tot)
        self.eC.refresh()
        if nb and self.wanet:
            g = self.eG.forward_grid(hw, float(opt.grid_rescale), st)
            ops.check(lib.combat_warp_fwd(s.cat_src.data_ptr(), s.tab_i[0].data_ptr(), g["grid"].data_ptr(), 0, nb, hw,
                                          s.cat_src[n:].data_ptr(), st), "warp")
        elif nb:
            self.eG.refresh()
            nbk = min(bucket(nb), n)
            if nbk not in self._small:
                small = self.eG.slot("V.small", nbk, hw)
                self._small[nbk] = (small, self.eG.forward_plan(small), torch.zeros(nbk, 3, hw, hw, dtype=f32, device=self.dev))
            sS, plan_small, tochange = self._small[nbk]
            self.k1.copy_(torch.from_numpy(trigger.gaussian_kernel1d(
                trigger.sample_sigma(getattr(opt, "sigma", (0.1, 1.0))), opt.kernel_size)))
            ops.check(lib.combat_augment_fwd(s.cat_src.data_ptr(), s.tab_i[0].data_ptr(), None, nbk, hw,
                                             self.eG.input(sS).data_ptr(), tochange.data_ptr(), st), "gather poisoned")
            plan_small.run()
            ops.check(lib.combat_trigger_fwd(tochange.data_ptr(), self.eG.output(sS).data_ptr(), self.P.data_ptr(),
                                             self.k1.data_ptr(), float(opt.noise_rate), nb, hw, None,
                                             s.cat_src[n:].data_ptr(), None, None, st), "trigger")
        ops.check(lib.combat_augment_fwd(s.cat_src.data_ptr(), s.tab_i[1].data_ptr(),
                                         s.tab_f.data_ptr() if aug is not None else None, n, hw,
                                         self.eC.input(s.slot).data_ptr(), None, st), "augment")
        s.fwd.run()
        backward_allreduce(s.bwd, self.eC, self.pg, self.world, self._reducers)   # buckets overlap the backward
        self.eC.fp.sgd_step(float(lr if lr is not None else opt.lr_C), grad_scale=1.0 / self.world)
        self.eC.mark_weights_dirty()

    def poisoned_pair(self):
        """(inputs_toChange, inputs_bd) of the last batch -- the two tensors the reference's debugging image stacks
        (train_victim_wanet.py:129) -- or None if that batch had no poisoned image."""
        trg, nb = getattr(self, "last_poisoned", (None, 0))
        if not nb:
            return None
        s = self.cur
        return s.cat_src[:s.n][trg.to(self.dev)].clone(), s.cat_src[s.n:s.n + nb].clone()

    def read_metrics(self, reset=False):
        """Running loss sum / correct count over every batch size run since the last reset (one host sync)."""
        out = {"loss_sum": 0.0, "correct": 0}
        for s in self._sets.values():
            h = self.eC.head_bufs(s.slot)
            out["loss_sum"] += float(h["loss"])
            out["correct"] += int(h["correct"][0])
            if reset:
                h["loss"].zero_()
                h["correct"].zero_()
        return out
