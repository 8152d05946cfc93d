"""Bit-exact and element-wise tests of the normalisation kernels (norm.hip) and the UNet decoder glue (elementwise.hip)
on the MI355X: the second user of the exact-test kit (conv_exact_ref.py), through norm_exact_ref.py.

  exact     lattice inputs for which every published statistic, coefficient and activation argument is an fp32 number
            in any summation order: mean / rstd / scale / shift / ca / cb / cc / dgamma / dbeta must EQUAL the exact
            values and every stored bf16 must EQUAL RNE_bf16(exact).  Running statistics (not dyadic) within 1 fp32 ulp
            of the same expression in numpy float64; num_batches_tracked + 1 exactly.
  bound     Gaussian inputs: statistics within the fp32 summation bound of the fp64 statistics of the same bf16 bits;
            outputs teacher-forced on the kernel's own published tables, every element within
            half_ulp_bf16(|ref| + E) + E, E = k 2^-24 (sum of the element's absolute terms), k counted from the source.

Both modes: a fixed bit pattern around (and inside) every destination, unchanged outside after the launch; NaN around
every source, none in any output.  The case tables live in norm_exact_cases.py; test_norm_exact_cpu.py checks them and
the kit without a GPU.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import norm_exact_cases as NC
import norm_exact_ref as R

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
DEV = "cuda"
EINVAL = -1
NBT0 = 5


@pytest.fixture(scope="module")
def lib():
    from combat_amd._lib import lib as l
    return l


def stream():
    return torch.cuda.current_stream().cuda_stream


def S(v, dtype):
    """A source tensor on the device with NaN in front of and behind it (None stays None)."""
    return None if v is None else R.Guarded.source(v.to(dtype).contiguous(), DEV)


def D(shape, dtype, fill=None):
    g = R.Guarded(shape, dtype, "dst", DEV)
    if fill is not None:
        g.t.copy_(torch.as_tensor(fill).to(dtype))
    return g


def P(g):
    return None if g is None else ctypes.c_void_p(g.t.data_ptr())


def host(g):
    return g.t.double().cpu()


def untouched(g):
    """A destination that still holds the fill pattern everywhere, interior included."""
    it, pat = R._PATTERN[g.dtype]
    return bool((g.buf.view(it) == pat).all())


def check_all(d, case_id):
    """Guard bands of every destination of the launch; no NaN in any of them."""
    torch.cuda.synchronize()
    for name, g in vars(d).items():
        if isinstance(g, R.Guarded) and g.role == "dst":
            g.check("%s of %s" % (name, case_id))
            if g.dtype.is_floating_point:
                assert not bool(torch.isnan(g.t).any()), "NaN in %s of %s" % (name, case_id)


def scratch_for(lib, case, short=0):
    if not case.rows or case.rows <= 256:
        return None, 0
    need = int(lib.combat_norm_scratch_bytes(case.groups, case.C))
    assert need == case.groups * 64 * 2 * case.C * 4
    return D((need // 4,), f32), need - short


# ------------------------------------------------------------------------------------------------ forward
def launch_forward(lib, case, b, form, short=0):
    """form 'fused': combat_norm_act_fused / combat_norm_add_act_fused; 'chain': combat_norm_finalize +
    combat_affine_act.  Returns (status, destinations)."""
    G, px, C = case.groups, case.px, case.C
    d = SimpleNamespace(x=S(b.x, bf16), add=S(b.add, bf16), rows=S(b.rows, f32), gamma=S(b.gamma, f32), beta=S(b.beta, f32),
                        add_scale=S(b.add_scale, f32), add_shift=S(b.add_shift, f32))
    for name in ("mean", "rstd", "scale", "shift"):
        setattr(d, name, D((G, C), f32))
    d.act = D((G, px, C), bf16)
    d.rm = d.rv = None
    if case.running:
        d.rm, d.rv = D((C,), f32, b.rm0), D((C,), f32, b.rv0)
    d.nbt = D((1,), torch.int64, NBT0)
    d.scratch, nbytes = scratch_for(lib, case, short)
    stats = (P(d.gamma), P(d.beta), P(d.mean), P(d.rstd), P(d.scale), P(d.shift), P(d.rm), P(d.rv), R.MOMENTUM, P(d.nbt),
             P(d.scratch), nbytes)
    if form == "fused":
        head = (P(d.x), P(d.rows), G, case.rows, px, C, case.eps, case.slope)
        if case.add:
            rc = lib.combat_norm_add_act_fused(*head, *stats, P(d.add), P(d.add_scale), P(d.add_shift), P(d.act), stream())
        else:
            rc = lib.combat_norm_act_fused(*head, *stats, P(d.act), stream())
    else:
        assert not case.add and case.rows
        rc = lib.combat_norm_finalize(P(d.rows), G, case.rows, C, float(px), case.eps, *stats, stream())
        if rc == 0:
            rc = lib.combat_affine_act(P(d.x), G * px, C, P(d.scale), P(d.shift), px if G > 1 else 0, case.slope, P(d.act),
                                       stream())
    return rc, d


def check_running(d, b, case):
    assert int(d.nbt.t.item()) == NBT0 + 1, "num_batches_tracked of %s: %d" % (case.id, int(d.nbt.t.item()))
    if case.running:
        R.assert_within_ulps(d.rm.t.cpu().numpy(), b.rm, 1, "running_mean of " + case.id)
        R.assert_within_ulps(d.rv.t.cpu().numpy(), b.rv, 1, "running_var of " + case.id)


def run_forward_exact(lib, case, form):
    b = NC.build_forward(case)
    rc, d = launch_forward(lib, case, b, form)
    assert rc == 0, (case.id, rc)
    check_all(d, case.id)
    for name in ("mean", "rstd", "scale", "shift"):
        R.report_mismatch(host(getattr(d, name)), getattr(b, name), "%s [g][c] of %s" % (name, case.id))
    R.report_mismatch(host(d.act), b.act, "act [g][pixel][c] of %s" % case.id)
    check_running(d, b, case)


@pytest.mark.parametrize("case", NC.FORWARD_CASES, ids=lambda c: c.id)
def test_exact_forward_fused(lib, case):
    """combat_norm_act_fused / combat_norm_add_act_fused, partial rows (every unroll boundary, stage 1), one ragged pass,
    several passes per chunk, the direct form, residuals, constant channels, one pixel."""
    run_forward_exact(lib, case, "fused")


@pytest.mark.parametrize("case", NC.CHAIN_CASES, ids=lambda c: c.id)
def test_exact_forward_chain(lib, case):
    """combat_norm_finalize (with stage 1) + combat_affine_act against the same exact expectation."""
    run_forward_exact(lib, case, "chain")


def run_forward_bound(lib, case, form):
    b = NC.build_forward_bound(case)
    if case.running:
        b.rm, b.rv = None, None
    rc, d = launch_forward(lib, case, b, form)
    assert rc == 0, (case.id, rc)
    check_all(d, case.id)
    mean, rstd, scale, shift = (host(getattr(d, n)) for n in ("mean", "rstd", "scale", "shift"))
    assert bool(((mean - b.mean).abs() <= b.e_mean + 2.0 ** -24 * b.mean.abs()).all()), "mean of " + case.id
    lo, hi = NC.rstd_interval(b.var, b.e_var, case.eps)
    assert bool(((rstd >= lo) & (rstd <= hi)).all()), "rstd of " + case.id
    print("%s: worst |mean - ref| / bound = %.3f" % (case.id, float(((mean - b.mean).abs() / (b.e_mean + 2.0 ** -24 * b.mean.abs())).max())))
    # scale / shift against the kernel's own mean / rstd: fp64 expressions rounded once
    gamma, beta = NC.affine_or_identity(b, case.C)
    gs = gamma[None] * rstd
    assert bool(((scale - gs).abs() <= 2.0 ** -23 * gs.abs()).all()), "scale of " + case.id
    sh = beta[None] - mean * gs
    # (mean, rstd and the product's own rounding, then the difference's: 4 roundings on |mean gamma rstd|, 1 on |beta|)
    tol = 2.0 ** -24 * beta[None].abs() + 2.0 ** -22 * (1 + 2.0 ** -20) * (mean * gs).abs()
    assert bool(((shift - sh).abs() <= tol).all()), "shift of " + case.id
    ref, e, und = NC.forward_bound_expect(b, case, scale, shift)
    R.assert_elementwise(host(d.act), ref, e, "act of %s (%s)" % (case.id, form), exclude=und)
    assert int(d.nbt.t.item()) == NBT0 + 1
    if case.running:
        rm, rv = R.running_expect(b.rm0.numpy(), b.rv0.numpy(), b.mean[0].numpy(), b.var[0].numpy(), case.px)
        n = case.px
        tol_m = R.MOMENTUM * b.e_mean[0].numpy() + np.spacing(np.abs(rm))
        tol_v = R.MOMENTUM * b.e_var[0].numpy() * n / max(n - 1, 1) + np.spacing(np.abs(rv))
        assert (np.abs(d.rm.t.cpu().numpy().astype(np.float64) - rm) <= tol_m).all(), "running_mean of " + case.id
        assert (np.abs(d.rv.t.cpu().numpy().astype(np.float64) - rv) <= tol_v).all(), "running_var of " + case.id


@pytest.mark.parametrize("case", NC.BOUND_CASES, ids=lambda c: c.id)
def test_bound_forward_fused(lib, case):
    run_forward_bound(lib, case, "fused")


@pytest.mark.parametrize("case", [c for c in NC.BOUND_CASES if c.rows and not c.add], ids=lambda c: c.id)
def test_bound_forward_chain(lib, case):
    run_forward_bound(lib, case, "chain")


# ------------------------------------------------------------------------------------------------ backward
def launch_backward(lib, case, b, form, short=0):
    G, px, C = case.groups, case.px, case.C
    d = SimpleNamespace(x=S(b.x, bf16), dz=S(b.dz, bf16), add=S(b.add, bf16), rows=S(b.rows, f32), gamma=S(b.gamma, f32),
                        mean=S(b.mean, f32), rstd=S(b.rstd, f32))
    d.dx = D((G, px, C), bf16)
    d.dgamma = D((C,), f32) if G == 1 else None
    d.dbeta = D((C,), f32) if G == 1 else None
    d.scratch, nbytes = scratch_for(lib, case, short)
    if form == "fused":
        rc = lib.combat_norm_bwd_fused(P(d.dz), P(d.x), P(d.add), P(d.rows), G, case.rows, px, C, P(d.gamma), P(d.mean),
                                       P(d.rstd), P(d.dgamma), P(d.dbeta), P(d.scratch), nbytes, P(d.dx), stream())
    else:
        assert case.rows
        for name in ("ca", "cb", "cc"):
            setattr(d, name, D((G, C), f32))
        rc = lib.combat_norm_bwd_finalize(P(d.rows), G, case.rows, C, float(px), P(d.gamma), P(d.mean), P(d.rstd), P(d.ca),
                                          P(d.cb), P(d.cc), P(d.dgamma), P(d.dbeta), P(d.scratch), nbytes, stream())
        if rc == 0:
            rc = lib.combat_norm_bwd_apply(P(d.dz), P(d.x), P(d.add), P(d.dx), G * px, C, px, int(G > 1), P(d.ca), P(d.cb),
                                           P(d.cc), stream())
    return rc, d


def run_backward_exact(lib, case, form):
    b = NC.build_backward(case)
    rc, d = launch_backward(lib, case, b, form)
    assert rc == 0, (case.id, rc)
    check_all(d, case.id)
    if form == "chain":
        for name in ("ca", "cb", "cc"):
            R.report_mismatch(host(getattr(d, name)), getattr(b.E, name), "%s [g][c] of %s" % (name, case.id))
    if case.groups == 1:
        R.report_mismatch(host(d.dgamma), b.E.dgamma, "dgamma of " + case.id)
        R.report_mismatch(host(d.dbeta), b.E.dbeta, "dbeta of " + case.id)
    R.report_mismatch(host(d.dx), b.E.dx, "dx [g][pixel][c] of %s" % case.id)


@pytest.mark.parametrize("case", NC.BACKWARD_CASES, ids=lambda c: c.id)
def test_exact_backward_fused(lib, case):
    """combat_norm_bwd_fused over the same shapes as the forward, with and without `add`."""
    run_backward_exact(lib, case, "fused")


@pytest.mark.parametrize("case", NC.CHAIN_CASES + [c for c in NC.ADD_CASES if c.add == 1 and c.rows], ids=lambda c: c.id)
def test_exact_backward_chain(lib, case):
    """combat_norm_bwd_finalize (with stage 1) + combat_norm_bwd_apply (plain and grouped, with `add`)."""
    run_backward_exact(lib, case, "chain")


def run_backward_bound(lib, case, form):
    b = NC.build_backward_bound(case)
    rc, d = launch_backward(lib, case, b, form)
    assert rc == 0, (case.id, rc)
    check_all(d, case.id)
    if case.groups == 1:
        got_b, got_g = host(d.dbeta), host(d.dgamma)
        assert bool(((got_b - b.s1[0]).abs() <= b.e1[0] + 2.0 ** -24 * b.s1[0].abs()).all()), "dbeta of " + case.id
        assert bool(((got_g - b.s2[0]).abs() <= b.e2[0] + 2.0 ** -24 * b.s2[0].abs()).all()), "dgamma of " + case.id
    # against the fp64 coefficients (their error derived from the sums' bounds): both forms
    ref, e = NC.backward_bound_expect(b, case)
    R.assert_elementwise(host(d.dx), ref, e, "dx of %s (%s)" % (case.id, form))
    if form == "chain":     # and teacher-forced on the published ca / cb / cc: only the apply's three roundings
        ref, e = NC.backward_bound_expect(b, case, *(host(getattr(d, n)) for n in ("ca", "cb", "cc")))
        R.assert_elementwise(host(d.dx), ref, e, "dx of %s (teacher-forced)" % case.id)


@pytest.mark.parametrize("case", NC.BOUND_CASES, ids=lambda c: c.id)
def test_bound_backward_fused(lib, case):
    run_backward_bound(lib, case, "fused")


@pytest.mark.parametrize("case", [c for c in NC.BOUND_CASES if c.rows], ids=lambda c: c.id)
def test_bound_backward_chain(lib, case):
    run_backward_bound(lib, case, "chain")


# ------------------------------------------------------------------------------------------------ refusals
def test_scratch_one_byte_short(lib):
    """More than 256 rows with a scratch one byte short: COMBAT_EINVAL from all four entry points, nothing written."""
    case = NC.nc(3, 255, 8, 257)
    fb, bb = NC.build_forward(case), NC.build_backward(case)
    for form in ("fused", "chain"):
        rc, d = launch_forward(lib, case, fb, form, short=1)
        assert rc == EINVAL, (form, rc)
        torch.cuda.synchronize()
        for name in ("mean", "rstd", "scale", "shift", "act", "scratch"):
            assert untouched(getattr(d, name)), "%s written by a refused forward launch (%s)" % (name, form)
        assert int(d.nbt.t.item()) == NBT0
        rc, d = launch_backward(lib, case, bb, form, short=1)
        assert rc == EINVAL, (form, rc)
        torch.cuda.synchronize()
        for name in ("dx", "scratch") + (("ca", "cb", "cc") if form == "chain" else ()):
            assert untouched(getattr(d, name)), "%s written by a refused backward launch (%s)" % (name, form)


def test_refusals(lib):
    """The direct form stops at 1024 pixels; combat_norm_add_act_fused needs `add`; its tables need `add` and one group."""
    case = NC.nc(3, 1025, 8, 0)
    x = torch.zeros(3, 1025, 8, dtype=torch.float64)
    b = SimpleNamespace(x=x, add=None, rows=None, gamma=None, beta=None, add_scale=None, add_shift=None, rm0=None, rv0=None)
    rc, d = launch_forward(lib, case, b, "fused")
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert untouched(d.act) and untouched(d.mean) and int(d.nbt.t.item()) == NBT0
    bb = SimpleNamespace(x=x, dz=x, add=None, rows=None, gamma=None, mean=torch.zeros(3, 8), rstd=torch.ones(3, 8))
    rc, d = launch_backward(lib, case, bb, "fused")
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert untouched(d.dx)
    small = torch.zeros(3, 16, 8, dtype=torch.float64)
    tab = torch.ones(8, dtype=torch.float64)
    for groups, add, tabs in ((1, None, None), (1, None, tab), (3, small, tab)):
        case = NC.nc(groups, 16, 8, 0, add=1)
        b = SimpleNamespace(x=small[:groups], add=None if add is None else add[:groups], rows=None, gamma=None, beta=None,
                            add_scale=tabs, add_shift=tabs, rm0=torch.zeros(8), rv0=torch.ones(8))
        rc, d = launch_forward(lib, case, b, "fused")
        assert rc == EINVAL, (groups, rc)
        torch.cuda.synchronize()
        assert untouched(d.act) and untouched(d.scale) and int(d.nbt.t.item()) == NBT0


@pytest.mark.parametrize("rows,C,slope", [(1, 8, 0.25), (300, 72, 0.0), (8191, 8, 0.25)])
def test_exact_affine_act_alone(lib, rows, C, slope):
    """combat_affine_act without tables: the activation alone, on multiples of 1/4 (exact under both slopes); 8191 rows
    x 1 octet leaves the last workgroup ragged."""
    x = NC.ints((rows, C), -255, 255, rows) * 0.25
    assert R.is_bf16(x)
    d = SimpleNamespace(x=S(x, bf16), out=D((rows, C), bf16))
    assert lib.combat_affine_act(P(d.x), rows, C, None, None, 0, slope, P(d.out), stream()) == 0
    check_all(d, "affine_act alone")
    R.report_mismatch(host(d.out), R.rne_bf16(R.lrelu(x, slope)), "out of affine_act alone, %d x %d" % (rows, C))
    assert lib.combat_affine_act(P(d.x), rows, C, P(d.x), None, 0, slope, P(d.out), stream()) == EINVAL


# ------------------------------------------------------------------------------------------------ group statistics
@pytest.mark.parametrize("groups,rpg,C,ppi", [(1, 1, 8, 0), (6, 33, 72, 2), (70, 64, 72, 0), (9, 31, 8, 3)])
def test_exact_group_stats(lib, groups, rpg, C, ppi):
    """combat_group_stats / combat_group_stats_bwd on integers: every row [2][C] equals the exact sums (70 groups x 9
    octets: a second workgroup)."""
    name = "group_stats g%d r%d c%d" % (groups, rpg, C)
    x = NC.ints((groups, rpg, C), -4, 4, groups + rpg)
    dz = NC.ints((groups, rpg, C), -4, 4, groups + rpg + 1)
    images = -(-groups // ppi) if ppi else 1
    mean = NC.ints((images, C), -3, 3, groups + 2)
    rstd = R.pick((0.5, 1.0, 2.0), (images, C), groups + 3)
    img = torch.arange(groups) // ppi if ppi else torch.zeros(groups, dtype=torch.long)
    xh = (x - mean[img][:, None, :]) * rstd[img][:, None, :]
    R.direct_range_check(x, x * x, dz, dz * xh)
    d = SimpleNamespace(x=S(x, bf16), dz=S(dz, bf16), mean=S(mean, f32), rstd=S(rstd, f32), part=D((groups, 2, C), f32),
                        part_b=D((groups, 2, C), f32))
    assert lib.combat_group_stats(P(d.x), groups, rpg, C, P(d.part), stream()) == 0
    assert lib.combat_group_stats_bwd(P(d.dz), P(d.x), groups, rpg, C, ppi, P(d.mean), P(d.rstd), P(d.part_b), stream()) == 0
    check_all(d, name)
    R.report_mismatch(host(d.part), torch.stack([x.sum(1), (x * x).sum(1)], 1), "partials of " + name)
    R.report_mismatch(host(d.part_b), torch.stack([dz.sum(1), (dz * xh).sum(1)], 1), "backward partials of " + name)


@pytest.mark.parametrize("groups,rpg,C", [(5, 49, 72), (3, 64, 8)])
def test_bound_group_stats(lib, groups, rpg, C):
    """Gaussian data: each row within the summation bound of rows_per_group fp32 terms."""
    name = "group_stats (Gaussian) g%d r%d c%d" % (groups, rpg, C)
    x, dz = R.gaussian_bf16((groups, rpg, C), 11, 1.5, 0.5), R.gaussian_bf16((groups, rpg, C), 12)
    mean = (x.sum(1) / rpg).float().double()
    rstd = (1 / torch.sqrt(((x * x).sum(1) / rpg - mean * mean).clamp_min(0) + 1e-5)).float().double()
    xh = (x - mean[:, None, :]) * rstd[:, None, :]
    d = SimpleNamespace(x=S(x, bf16), dz=S(dz, bf16), mean=S(mean, f32), rstd=S(rstd, f32), part=D((groups, 2, C), f32),
                        part_b=D((groups, 2, C), f32))
    assert lib.combat_group_stats(P(d.x), groups, rpg, C, P(d.part), stream()) == 0
    assert lib.combat_group_stats_bwd(P(d.dz), P(d.x), groups, rpg, C, 1, P(d.mean), P(d.rstd), P(d.part_b), stream()) == 0
    check_all(d, name)
    for got, terms, extra in ((host(d.part), (x, x * x), 0.0), (host(d.part_b), (dz, dz * xh), 2.0 ** -23)):
        for k, t in enumerate(terms):
            e = R.summation_bound(rpg, t.abs().sum(1)) + (extra * t.abs().sum(1) if k else 0.0)
            R.assert_elementwise(got[:, k], t.sum(1), e, "%s row %d" % (name, k), stored_bf16=False)


# ------------------------------------------------------------------------------------------------ eval-mode fold
def fold_tables(C, seed, exact):
    if exact:
        return (R.pick((-0.5, 0.5, 1.0, 2.0), (C,), seed), NC.ints((C,), -5, 5, seed + 1), NC.ints((C,), -4, 4, seed + 2),
                R.pick((0.25, 1.0, 4.0, 16.0), (C,), seed + 3))
    g = R.gen(seed)
    return tuple(t.float().double() for t in (torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g),
                                              torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.1))


def check_fold(d, tabs, eps, exact, name):
    gamma, beta, rm, rv = tabs
    s = gamma / torch.sqrt(rv + eps)
    sh = beta - rm * s
    if exact:
        R.report_mismatch(host(d.scale), s, "scale of " + name)
        R.report_mismatch(host(d.shift), sh, "shift of " + name)
    else:       # the addition, the square root and the division round once each; then the product and the difference
        e_s = 3 * 2.0 ** -24 * s.abs()
        R.assert_elementwise(host(d.scale), s, e_s, "scale of " + name, stored_bf16=False)
        R.assert_elementwise(host(d.shift), sh, rm.abs() * e_s + 2 * 2.0 ** -24 * (beta.abs() + (rm * s).abs()), "shift of " + name,
                             stored_bf16=False)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bound"])
def test_bn_eval_fold(lib, exact):
    """combat_bn_eval_fold at C = 1, 63, 512, 513 and combat_bn_eval_fold_batch over the four as one descriptor table
    (2 x 256 threads per descriptor: 513 needs the grid-stride loop's second trip)."""
    eps = 0.0 if exact else 1e-5
    single, batch, rows = [], [], []
    for i, C in enumerate(NC.FOLD_CHANNELS):
        tabs = fold_tables(C, 100 + i, exact)
        for store in (single, batch):
            d = SimpleNamespace(**{n: S(t, f32) for n, t in zip(("gamma", "beta", "rm", "rv"), tabs)}, scale=D((C,), f32),
                                shift=D((C,), f32), tabs=tabs, C=C)
            store.append(d)
        d = single[-1]
        assert lib.combat_bn_eval_fold(P(d.gamma), P(d.beta), P(d.rm), P(d.rv), eps, C, P(d.scale), P(d.shift), stream()) == 0
        d = batch[-1]
        rows.append([g.t.data_ptr() for g in (d.gamma, d.beta, d.rm, d.rv, d.scale, d.shift)] + [C])   # C | reserved << 32
    descs = torch.tensor(rows, dtype=torch.int64, device=DEV)
    assert descs.element_size() * descs.shape[1] == 56
    assert lib.combat_bn_eval_fold_batch(ctypes.c_void_p(descs.data_ptr()), len(rows), eps, stream()) == 0
    for kind, store in (("single", single), ("batch", batch)):
        for d in store:
            name = "bn_eval_fold (%s) C=%d" % (kind, d.C)
            check_all(d, name)
            check_fold(d, d.tabs, eps, exact, name)


# ------------------------------------------------------------------------------------------------ upsample
def launch_up(lib, case, b, fused):
    N, H, W, C = case.N, case.H, case.W, case.C
    d = SimpleNamespace(y=S(b.y, bf16), s=S(b.s, bf16), ss=S(b.ss, f32), ts=S(b.ts, f32), out=D((N, 2 * H, 2 * W, C), bf16))
    if fused:
        d.rows = S(getattr(b, "rows", None), f32)
        for name in ("mean", "rstd", "scale", "shift"):
            setattr(d, name, D((N, C), f32))
        rows = case.rows if d.rows is not None else 0
        rc = lib.combat_unet_up_fused(P(d.y), P(d.rows), rows, P(d.s), P(d.ss), P(d.ts), N, H, W, C, case.eps, P(d.mean),
                                      P(d.rstd), P(d.scale), P(d.shift), P(d.out), stream())
    else:
        d.sy, d.ty = S(b.sy, f32), S(b.ty, f32)
        rc = lib.combat_unet_up_fwd(P(d.y), P(d.sy), P(d.ty), P(d.s), P(d.ss), P(d.ts), N, H, W, C, P(d.out), stream())
    return rc, d


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("case", NC.UP_CASES, ids=lambda c: c.id)
def test_exact_up_forward(lib, case, fused):
    """combat_unet_up_fwd and combat_unet_up_fused (direct and with partial rows): out equals RNE_bf16 of the exact
    blend (negative values: of the one fp32 rounding of 0.2f v); the fused form's mean / rstd / scale / shift equal the
    exact statistics."""
    b = NC.build_up(case, fused)
    rc, d = launch_up(lib, case, b, fused)
    assert rc == 0, (case.id, rc)
    check_all(d, case.id)
    if fused:
        for name, exp in (("mean", b.L.mean), ("rstd", b.L.rstd), ("scale", b.sy), ("shift", b.ty)):
            R.report_mismatch(host(getattr(d, name)), exp, "%s [n][c] of %s" % (name, case.id))
    R.report_mismatch(host(d.out).permute(0, 3, 1, 2), b.out.permute(0, 3, 1, 2), "out of %s" % case.id)


def launch_up_bwd(lib, case, b, fused):
    N, H, W, C = case.N, case.H, case.W, case.C
    d = SimpleNamespace(d_out=S(b.d_out, bf16), out=S(b.out, bf16), du=D((N, H, W, C), bf16))
    if fused:
        d.y, d.mean, d.rstd, d.dx = S(b.y, bf16), S(b.mean, f32), S(b.rstd, f32), D((N, H, W, C), bf16)
        rc = lib.combat_unet_up_bwd_fused(P(d.d_out), P(d.out), P(d.y), P(d.mean), P(d.rstd), N, H, W, C, P(d.du), P(d.dx),
                                          stream())
    else:
        rc = lib.combat_unet_up_bwd(P(d.d_out), P(d.out), N, H, W, C, P(d.du), stream())
    return rc, d


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("case", NC.UP_CASES, ids=lambda c: c.id)
def test_exact_up_backward(lib, case, fused):
    """combat_unet_up_bwd and combat_unet_up_bwd_fused: du equals RNE_bf16(adjoint) on positive `out`; the fused form's
    dx, whose coefficients are not dyadic, within its three fp32 roundings of the fp64 value from the stored du."""
    b = NC.build_up_bwd(case)
    b.mean, b.rstd = b.L.mean, b.L.rstd
    rc, d = launch_up_bwd(lib, case, b, fused)
    assert rc == 0, (case.id, rc)
    check_all(d, case.id)
    R.report_mismatch(host(d.du).permute(0, 3, 1, 2), b.du.permute(0, 3, 1, 2), "du of %s" % case.id)
    if fused:
        R.assert_elementwise(host(d.dx), b.dx, b.dx_e, "dx of %s" % case.id)


@pytest.mark.parametrize("case", NC.UP_BOUND_CASES, ids=lambda c: c.id)
def test_bound_up(lib, case):
    """Sign-mixed Gaussian data through all four upsample entry points (the 0.2 slope is not dyadic)."""
    b = NC.build_up_bound(case)
    N, H, W, C = case.N, case.H, case.W, case.C
    rc, d = launch_up(lib, case, b, False)
    assert rc == 0
    check_all(d, case.id)
    ref, e, und = NC.up_forward_bound_expect(b, b.sy, b.ty)
    R.assert_elementwise(host(d.out), ref, e, "out of %s (plain)" % case.id, exclude=und)
    # fused: statistics of y within the direct form's bound, out teacher-forced on the published scale / shift
    x = b.y.reshape(N, H * W, C)
    if case.rows:
        b.rows, terms = NC.run_sums(x, x * x, case.rows), 1
    else:
        terms = -(-H * W // 32)
    rc, f = launch_up(lib, case, b, True)
    assert rc == 0
    check_all(f, case.id)
    mean, var, e_mean, e_var = R.stats_bound(x, terms)
    got_mean, got_rstd, sy, ty = (host(getattr(f, n)) for n in ("mean", "rstd", "scale", "shift"))
    assert bool(((got_mean - mean).abs() <= e_mean + 2.0 ** -24 * mean.abs()).all()), "mean of " + case.id
    lo, hi = NC.rstd_interval(var, e_var, case.eps)
    assert bool(((got_rstd >= lo) & (got_rstd <= hi)).all()), "rstd of " + case.id
    R.report_mismatch(sy, got_rstd, "scale (= rstd) of " + case.id)
    assert bool(((ty + got_mean * got_rstd).abs() <= 2.0 ** -22 * (got_mean * got_rstd).abs()).all()), "shift of " + case.id
    ref, e, und = NC.up_forward_bound_expect(b, sy, ty)
    R.assert_elementwise(host(f.out), ref, e, "out of %s (fused)" % case.id, exclude=und)
    # backward on the plain kernel's own stored out
    out = host(d.out)
    bb = SimpleNamespace(d_out=b.d_out, out=out, y=b.y, mean=got_mean, rstd=got_rstd)
    ref, e = NC.up_backward_bound_expect(b.d_out, out)
    for fused in (False, True):
        rc, g = launch_up_bwd(lib, case, bb, fused)
        assert rc == 0
        check_all(g, case.id)
        R.assert_elementwise(host(g.du), ref, e, "du of %s (%s)" % (case.id, "fused" if fused else "plain"))
    # dx of the fused form from ITS stored du: per-lane fp32 sums, then the three roundings of the apply
    du = host(g.du).reshape(N, H * W, C)
    xh = (x - got_mean[:, None, :]) * got_rstd[:, None, :]
    lanes = -(-H * W // 32)
    sb = SimpleNamespace(x=x, dz=du, gamma=torch.ones(C, dtype=torch.float64), mean=got_mean, rstd=got_rstd, add=None,
                         s1=du.sum(1), s2=(du * xh).sum(1), e1=R.summation_bound(lanes, du.abs().sum(1)),
                         e2=R.summation_bound(lanes, (du * xh).abs().sum(1)) + 2.0 ** -23 * (du * xh).abs().sum(1))
    ref, e = NC.backward_bound_expect(sb, SimpleNamespace(px=H * W))
    R.assert_elementwise(host(g.dx).reshape(N, H * W, C), ref, e, "dx of %s (fused)" % case.id)


def test_up_refusals(lib):
    """257 partial rows and 1025 pixels without rows are refused by the fused forms, and nothing is written."""
    case = NC.uc(1, 2, 2, 8, 0, 257)
    y = torch.zeros(1, 2, 2, 8, dtype=torch.float64)
    b = SimpleNamespace(y=y, s=None, ss=None, ts=None, rows=torch.zeros(1, 257, 2, 8, dtype=torch.float64))
    rc, d = launch_up(lib, case, b, True)
    assert rc == EINVAL
    case = NC.uc(1, 25, 41, 8, 0, 0)
    b = SimpleNamespace(y=torch.zeros(1, 25, 41, 8, dtype=torch.float64), s=None, ss=None, ts=None, rows=None)
    rc, e = launch_up(lib, case, b, True)
    assert rc == EINVAL
    bb = SimpleNamespace(d_out=torch.zeros(1, 50, 82, 8), out=torch.ones(1, 50, 82, 8), y=b.y, mean=torch.zeros(1, 8),
                         rstd=torch.ones(1, 8))
    rc, g = launch_up_bwd(lib, case, bb, True)
    assert rc == EINVAL
    torch.cuda.synchronize()
    for t in (d.out, d.mean, d.scale, e.out, e.mean, g.du, g.dx):
        assert untouched(t)
