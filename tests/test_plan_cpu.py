"""engine.Plan as a list of Call records, on the host: recording, the post-passes that edit the list (group_wgrads,
merge_convs), splicing two plans and the compiled form.  Nothing is launched: the plans are recorded over CPU tensors
(the library's host queries and combat_plan_record only look at the arguments) and Plan.run is never called."""
import ctypes
import types

import pytest
import torch

N = 8
OFF_128 = 1000          # flat-gradient offset of the mark between the 128-channel and the 64-channel layers
CPU = torch.device("cpu")
W64 = ["w64.%d" % i for i in range(4)]
W128 = ["w128.%d" % i for i in range(3)]
GROUPS = {"off": [], "tail": [W64], "pairs": [W64[:2], W64[2:]], "stages": [W128, W64]}


@pytest.fixture(scope="module")
def E():
    """The engine module, in deterministic mode for the module (as the grouping test on the GPU)."""
    from combat_amd import engine
    from combat_amd._lib import lib
    before = lib.combat_get_deterministic()
    lib.combat_set_deterministic(1)
    yield engine
    lib.combat_set_deterministic(before)


def bf(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


def wgrad(E, plan, what, c, k, hw, r=3, stride=1):
    """One weight gradient c -> k over an N x hw x hw input, recorded with rec_wgrad as an engine does."""
    conv = types.SimpleNamespace(R=r, stride=stride, pad=r // 2, K=k, c_real=c)
    dw = torch.zeros(k, r, r, c)
    E.rec_wgrad(plan, what, bf(N, hw, hw, c), bf(N, hw // stride, hw // stride, k), conv, dw)
    return plan.calls[-1]


def inline(E, plan, what, **kw):
    return plan.add(what, E.lib.combat_memset_zero, 4096, 16, **kw)


def backward(E, aux_queues=1):
    """A plan shaped like PreActResNet18's training backward at batch 8: the 1x1 / stride-2 shortcut and the three
    128 -> 128 weight gradients of layer2 (16 x 16), a mark -- on the last of them --, a weight gradient that an in-line
    call waits for, the four 64 -> 64 ones of layer1 (32 x 32), mark(0) on the last.  Plain calls stand between them."""
    p = E.Plan("cpu.backward")
    p.aux_queues = aux_queues
    inline(E, p, "zero_grad")
    wgrad(E, p, "sc", 64, 128, 32, r=1, stride=2)
    for i, what in enumerate(W128):
        if i:
            inline(E, p, "dx128.%d" % i)
        wgrad(E, p, what, 128, 128, 16)
    p.mark(OFF_128)
    inline(E, p, "dx64")
    dep = wgrad(E, p, "w64.dep", 64, 64, 32)
    inline(E, p, "dep.copy", after=dep)
    for what in W64:
        inline(E, p, "dx." + what)
        wgrad(E, p, what, 64, 64, 32)
    p.mark(0)
    return p


def grouped(E, monkeypatch, mode, **kw):
    p = backward(E, **kw)
    monkeypatch.setattr(E.Plan, "wgrad_groups", mode)
    monkeypatch.setattr(E.Plan, "serial", False)
    E.group_wgrads(p, CPU)
    return p


def test_recording(E):
    p = E.Plan("cpu.rec")
    p.aux_queues = 2
    first = inline(E, p, "a")
    assert type(first) is E.Call and p.calls == [first]
    assert (first.func, first.args, first.what) == (E.lib.combat_memset_zero, (4096, 16), "a")
    assert (first.queue, first.after, first.mark, first.wgrad) == (None, None, None, None)
    aux = [inline(E, p, "x%d" % i, aux=True) for i in range(2)] + [wgrad(E, p, "w", 64, 64, 32)] + [inline(E, p, "x3", aux=True)]
    assert [c.queue for c in aux] == [0, 1, 0, 1] and p.next_aux_queue() == 0
    assert type(aux[2].wgrad).__name__ == "WgradArgs" and aux[2].func is E.lib.combat_conv_wgrad
    waiter = inline(E, p, "b", after=aux[2])
    assert waiter.after is aux[2] and waiter.queue is None
    p.mark(7)
    assert waiter.mark == 7 and [c.mark for c in p.calls[:-1]] == [None] * (len(p.calls) - 1)
    p.mark(5)                                 # a later mark on the same call wins
    assert waiter.mark == 5 and p.mark_offsets == [5]
    last = wgrad(E, p, "w2", 64, 64, 32)
    p.mark(0)
    assert last.mark == 0 and p.mark_offsets == [5, 0] and p.calls[-1] is last and len(p) == 7
    assert [a.dw for a in p.wgrads] == [aux[2].wgrad.dw, last.wgrad.dw] and p.wgrads[0] is aux[2].wgrad
    # the training-shaped plan of the tests below
    b = backward(E)
    assert [c.what for c in b.calls if c.wgrad is not None] == ["sc"] + W128 + ["w64.dep"] + W64
    assert b.mark_offsets == [OFF_128, 0] and len(b.wgrads) == 9 and all(c.queue == 0 for c in b.calls if c.wgrad is not None)


@pytest.mark.parametrize("mode", ["off", "tail", "pairs", "stages"])
def test_grouping(E, monkeypatch, mode):
    ref = backward(E)
    stage_of, n = {}, 0
    for c in ref.calls:
        stage_of[c.what] = n
        n += c.mark is not None
    p = backward(E)
    marked = [(c, c.mark) for c in p.calls if c.mark is not None]
    dw_of = {c.what: c.wgrad.dw for c in p.calls if c.wgrad is not None}
    recorded = [a.dw for a in p.wgrads]
    assert [c.what for c, _ in marked] == [W128[-1], W64[-1]]           # both marks stand on a group's last member
    monkeypatch.setattr(E.Plan, "wgrad_groups", mode)
    monkeypatch.setattr(E.Plan, "serial", False)
    E.group_wgrads(p, CPU)
    groups = [c for c in p.calls if c.func is E.lib.combat_conv_wgrad_group]
    assert [c.what.split("+") for c in groups] == GROUPS[mode]
    members = sum(len(g) for g in GROUPS[mode])
    assert len(p.calls) == len(ref.calls) - (members - len(groups))
    for g in groups:
        names = g.what.split("+")
        assert len({stage_of[w] for w in names}) == 1, names            # no group on both sides of the mark
        assert "sc" not in names and "w64.dep" not in names
        assert g.queue == 0 and g.args[1] == len(names) == len(g.wgrad)
        assert [a.dw for a in g.wgrad] == [dw_of[w] for w in names]
    singles = [c.what for c in p.calls if c.func is E.lib.combat_conv_wgrad]
    assert singles == [w for w in ["sc"] + W128 + ["w64.dep"] + W64 if not any(w in g for g in GROUPS[mode])]
    # the marks stay on the same records, the dependencies still point into the list
    for c, off in marked:
        assert any(c is x for x in p.calls) and c.mark == off
    assert p.mark_offsets == ref.mark_offsets == [OFF_128, 0]
    waiters = [c for c in p.calls if c.after is not None]
    assert [c.what for c in waiters] == ["dep.copy"]
    assert all(any(c.after is x for x in p.calls) for c in waiters) and waiters[0].after.what == "w64.dep"
    assert [a.dw for a in p.wgrads] == recorded and len(set(recorded)) == 9
    # everything else is where it was
    assert [c.what for c in p.calls if c.wgrad is None] == [c.what for c in ref.calls if c.wgrad is None]


def test_grouping_keeps_to_one_queue(E, monkeypatch):
    """Two auxiliary queues deal neighbouring weight gradients to different queues: nothing follows its like."""
    p = grouped(E, monkeypatch, "stages", aux_queues=2)
    assert {c.queue for c in p.calls if c.queue is not None} == {0, 1}
    assert not any(c.func is E.lib.combat_conv_wgrad_group for c in p.calls) and len(p.calls) == len(backward(E).calls)


def conv_pair_plan(E, aux=False, mark=False, awaited=False):
    """A mark and an auxiliary call, then two convolutions; the flags put the second convolution in the way."""
    p = E.Plan("cpu.merge")
    side = inline(E, p, "side", aux=True)
    inline(E, p, "m")
    p.mark(64)
    a0, a1 = E.ConvArgs(), E.ConvArgs()
    p.hold(a0, a1)
    p.add("sc", E.lib.combat_conv_gemm, ctypes.byref(a0))
    p.add("c1", E.lib.combat_conv_gemm, ctypes.byref(a1), aux=aux)
    if mark:
        p.mark(32)
    if awaited:
        inline(E, p, "waiter", after=p.calls[3])
    return p, side, (a0, a1)


def test_merge_convs(E):
    p, side, (a0, a1) = conv_pair_plan(E)
    tail = inline(E, p, "tail", after=side)
    before = list(p.calls)
    p.merge_convs(2)
    assert len(p.calls) == 4 and p.calls[:2] == before[:2] and p.calls[3] is tail
    pair = p.calls[2]
    assert pair.func is E.lib.combat_conv_gemm_pair and pair.what == "sc+c1"
    assert len(pair.args) == 2 and pair.args[0]._obj is a0 and pair.args[1]._obj is a1
    assert (pair.queue, pair.after, pair.mark, pair.wgrad) == (None, None, None, None)
    assert side.queue == 0 and before[1].mark == 64 and p.mark_offsets == [64] and tail.after is side
    for kw in (dict(aux=True), dict(mark=True), dict(awaited=True)):
        q = conv_pair_plan(E, **kw)[0]
        with pytest.raises(AssertionError):
            q.merge_convs(2)
        assert [c.what for c in q.calls[2:4]] == ["sc", "c1"]


def test_splicing(E):
    p, q = E.Plan("cpu.p"), E.Plan("cpu.q")
    inline(E, p, "p0")
    p.mark(9)
    side = inline(E, q, "q.side", aux=True)
    inline(E, q, "q.mid")
    q.mark(3)
    waiter = inline(E, q, "q.waiter", after=side)
    p.calls += q.calls
    end = inline(E, p, "p1")
    assert [c.what for c in p.calls] == ["p0", "q.side", "q.mid", "q.waiter", "p1"]
    assert all(a is b for a, b in zip(p.calls[1:4], q.calls))
    assert p.calls[1].queue == 0 and p.calls[3].after is p.calls[1] and p.mark_offsets == [9, 3] and end.queue is None
    # ... and the compiled form follows: the dependency resolves inside p, the ranges split at both marks
    assert p._program() == [("c", 0, 1), ("mark", 9), ("c", 1, 3), ("mark", 3), ("c", 3, 5)]
    assert waiter.after is side


def test_compiled_form(E, monkeypatch):
    p = grouped(E, monkeypatch, "stages")
    n = len(p.calls)
    assert all(getattr(c.func, "argtypes", None) is not None for c in p.calls)
    cut = 1 + [c.what for c in p.calls].index("+".join(W128))
    prog = p._program()
    assert E.lib.combat_plan_size(p._cplan) == n == len(p._cnames) and p._cnames == [c.what for c in p.calls]
    assert prog == [("c", 0, cut), ("mark", OFF_128), ("c", cut, n), ("mark", 0)]
    assert p._prog_nomark == [("c", 0, n)]
    assert p._program() is prog                       # built once ...
    inline(E, p, "more")
    assert p._program() == prog + [("c", n, n + 1)]   # ... and again after an edit of the list
    # a Python callable in the middle
    q = E.Plan("cpu.py")
    hand_off = lambda *a: 0
    inline(E, q, "a")
    q.add("py", hand_off, 1, 2)
    inline(E, q, "b")
    assert q._program() == [("c", 0, 1), ("py", hand_off, (1, 2), "py"), ("c", 1, 2)]
    assert q._prog_nomark == q._program() and E.lib.combat_plan_size(q._cplan) == 2
