"""engine.group_wgrads on the MI355X: PreActResNet18's training backward with its same-geometry weight gradients as
combat_conv_wgrad_group calls, against the same plan without grouping (Plan.wgrad_groups = "off").

Deterministic mode: a member of a group keeps its summation order, so the flat gradient must be EQUAL, not close.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 8
MARK_BLOCKS = (6, 4, 2)     # an all-reduce mark follows the backward of these blocks (layer4 / layer3 / layer2 complete)


@pytest.fixture(scope="module")
def net():
    """One PreActResNet18, one batch, and per grouping mode a slot whose train forward has run and whose backward plan
    is built (build(mode) -> (slot, plan)); deterministic mode for the module."""
    from combat_amd import engine, nets, ops
    from combat_amd._lib import lib
    before = lib.combat_get_deterministic()
    lib.combat_set_deterministic(1)
    torch.manual_seed(0)
    m = nets.PreActResNet18().cuda()
    eng = m._net_engine()
    eng.refresh()
    gen = torch.Generator().manual_seed(4)
    x = (torch.rand(N, 3, 32, 32, generator=gen) * 2 - 1).cuda()
    t = torch.randint(0, 10, (N,), generator=gen).cuda()
    built = {}

    def build(mode):
        if mode not in built:
            saved = engine.Plan.wgrad_groups
            engine.Plan.wgrad_groups = mode
            try:
                slot = eng.slot("group.%s" % mode, N, 32)
                ops.image_to_c8(x, eng.input(slot))
                eng.head_bufs(slot)["targets"].copy_(t)
                eng.forward_plan(slot, True).run()
                built[mode] = (slot, eng.backward_train_plan(slot))
            finally:
                engine.Plan.wgrad_groups = saved
        return built[mode]

    yield dict(engine=engine, lib=lib, eng=eng, build=build)
    lib.combat_set_deterministic(before)


def flat_grad(eng, plan, **kw):
    plan.run(**kw)
    torch.cuda.synchronize()
    return eng.fp.grad.detach().clone()


def groups_of(lib, plan):
    return [(i, c.what.split("+")) for i, c in enumerate(plan.calls) if c.func is lib.combat_conv_wgrad_group]


@pytest.mark.parametrize("mode", ["tail", "pairs", "stages"])
def test_grouped_backward_equals_ungrouped_bitwise(net, mode):
    lib, eng = net["lib"], net["eng"]
    _, off = net["build"]("off")
    _, on = net["build"](mode)
    assert not groups_of(lib, off)
    groups = groups_of(lib, on)
    members = sum(len(g) for _, g in groups)
    assert groups and len(on.calls) == len(off.calls) - (members - len(groups)) < len(off.calls), (mode, groups)
    layer1 = ["b1.c2.wgrad", "b1.c1.wgrad", "b0.c2.wgrad", "b0.c1.wgrad"]
    want = {"tail": [layer1], "pairs": [layer1[:2], layer1[2:]],
            "stages": [["b7.c2.wgrad", "b7.c1.wgrad", "b6.c2.wgrad"], ["b5.c2.wgrad", "b5.c1.wgrad", "b4.c2.wgrad"],
                       ["b3.c2.wgrad", "b3.c1.wgrad", "b2.c2.wgrad"], layer1]}[mode]
    assert [g for _, g in groups] == want
    ref = flat_grad(eng, off)
    assert float(ref.abs().sum()) > 0
    for rep in range(2):
        assert torch.equal(flat_grad(eng, on), ref), (mode, rep)
    # the plan still lists every weight gradient, in the order it was recorded, with the gradient it writes
    assert [a.dw for a in on.wgrads] == [a.dw for a in off.wgrads]


def test_grouped_backward_python_and_inline_replay(net):
    """The replay from Python (COMBAT_PLAN_PY) and the in-line replay (Plan.serial) take the group call as it is."""
    engine, eng = net["engine"], net["eng"]
    _, off = net["build"]("off")
    _, on = net["build"]("stages")
    ref = flat_grad(eng, off)
    for compiled, serial in ((False, False), (True, True)):
        engine.Plan.compiled, engine.Plan.serial = compiled, serial
        try:
            got = flat_grad(eng, on)
        finally:
            engine.Plan.compiled, engine.Plan.serial = True, False
        assert torch.equal(got, ref), (compiled, serial)


def test_profiled_replay_lists_every_weight_gradient(net):
    """prof=[]: a group is replayed as its members' single launches, so the list holds the same weight-gradient
    entries (names and count) with grouping on as off, and the gradient is the same."""
    eng = net["eng"]
    _, off = net["build"]("off")
    _, on = net["build"]("stages")
    p_off, p_on = [], []
    g_off = flat_grad(eng, off, prof=p_off)
    g_on = flat_grad(eng, on, prof=p_on)
    names = lambda prof, plan: sorted(w[len(plan.name) + 1:] for w, _, _, _ in prof if "wgrad" in w)
    n_off, n_on = names(p_off, off), names(p_on, on)
    assert n_off == n_on and len(n_off) == len(off.wgrads) == 20
    assert all(type(a).__name__ == "WgradArgs" for w, a, _, _ in p_on if "wgrad" in w)
    assert torch.equal(g_on, g_off)


def test_no_group_spans_an_all_reduce_mark(net):
    """Data parallel: the gradients above a mark are final there, so every member of a group lies in the stage its
    group call is recorded in -- read off the recorded plan, no second rank needed."""
    lib, eng = net["lib"], net["eng"]
    _, off = net["build"]("off")
    _, on = net["build"]("stages")
    assert len(on.mark_offsets) == len(off.mark_offsets) == len(MARK_BLOCKS) + 1
    where = {c.what: i for i, c in enumerate(off.calls)}
    stage = lambda plan, i: sum(1 for c in plan.calls[:i] if c.mark is not None)
    groups = groups_of(lib, on)
    assert len(groups) == 4
    for i, members in groups:
        assert len({stage(off, where[w]) for w in members}) == 1, members
        assert stage(on, i) == stage(off, where[members[0]]), members
        assert where[members[-1]] == max(where[w] for w in members)
    # the marks keep their gradient offsets and their order
    assert on.mark_offsets == off.mark_offsets
    seen = []
    ref = flat_grad(eng, off)
    got = flat_grad(eng, on, on_mark=seen.append)
    assert torch.equal(got, ref) and seen == on.mark_offsets
