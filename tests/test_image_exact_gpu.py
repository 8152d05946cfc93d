"""Bit-exact and element-wise tests of the image-side kernels (trigger.hip, warp.hip) on the MI355X: the third user of
the exact-test kit (conv_exact_ref.py), through image_exact_ref.py.

  exact     lattice operands (P, k1 and D are arguments of the ABI, so the tests hand in dyadic ones) for which every
            intermediate is an fp32 number in any summation order: out must EQUAL the exact value, the c8 image
            (RNE_bf16(v), RNE_bf16(v - hi), 0, 0), d_noise RNE_bf16(exact) with channels 3..7 zero, tv the exact sum
            where it stays below 2^24 quanta; mse within the summation bound (its terms carry 2^-26 quanta).  The copy
            paths of the augmentation and the three warp entry points are exact on their data as they are.
  bound     the real low-pass matrix, Gaussian triples, the real DCT matrix, uint8-derived images, tanh noise as bf16:
            every element within E = k 2^-24 (its absolute-value chain) of the float64 reference of the same operand
            bits, k counted from the source (image_exact_ref.py); bf16 outputs within half_ulp_bf16(|ref| + E) + E.
            The clamp mask is decided on every pixel (image_exact_cases.bound_data): no element is excluded.

Both modes: a fixed bit pattern around (and inside) every destination, unchanged outside after the launch; NaN around
every source and in the c8 channels a kernel must not read, none in any output.  The case tables live in
image_exact_cases.py; test_image_exact_cpu.py checks them, the reference and the comparisons without a GPU.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import image_exact_cases as IC
import image_exact_ref as R

pytestmark = pytest.mark.gpu

bf16, f32 = torch.bfloat16, torch.float32
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from combat_amd._lib import lib as l
    return l


def stream():
    return torch.cuda.current_stream().cuda_stream


def S(v, dtype=f32):
    """A source tensor on the device with NaN in front of and behind it (None stays None)."""
    return None if v is None else R.Guarded.source(R.t64(v).to(dtype).contiguous(), DEV)


def D(shape, dtype=f32, fill=None):
    g = R.Guarded(shape, dtype, "dst", DEV)
    if fill is not None:
        g.t.copy_(R.t64(fill).to(dtype))
    return g


def P(g):
    return None if g is None else ctypes.c_void_p(g.t.data_ptr())


def I(v):
    """int32 index tensor on the device (None stays None); returns (tensor kept alive, pointer)."""
    if v is None:
        return None, None
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(DEV)
    return t, ctypes.c_void_p(t.data_ptr())


def host(g):
    return None if g is None else g.t.double().cpu()


def check_all(d, case_id):
    """Guard bands of every destination of the launch; no NaN in any of them."""
    torch.cuda.synchronize()
    for name, g in vars(d).items():
        if isinstance(g, R.Guarded) and g.role == "dst":
            g.check("%s of %s" % (name, case_id))
            assert not bool(torch.isnan(g.t).any()), "NaN in %s of %s" % (name, case_id)


def operands(case, mode):
    d = IC.data(case, mode)
    return d, SimpleNamespace(x=S(d.x), noise=S(R.nhwc3(d.noise), bf16), P=S(d.P), k1=S(d.k1.reshape(-1)))


# ------------------------------------------------------------------------------------------------ trigger forward
def launch_fwd(lib, case, mode, variant):
    """variant `full`: every optional output (and src_index on plain cases); `bare`: out alone; `tv` / `tv_bare`:
    the total-variation entry point of the route with and without mse_partial (plain cases).  Returns (expectation,
    stored outputs)."""
    d, s = operands(case, mode)
    hw, n = case.hw, case.n
    src = IC.src_index(case) if case.kind == "plain" and variant == "full" else None
    E = IC.expect_fwd(case, mode, src)
    rows = E.out.shape[0]
    head = (P(s.x), P(s.noise), P(s.P), P(s.k1), d.rate, n if src is None else len(src), hw)
    full = variant in ("full", "tv")
    s.mse = D((E.mse.shape[0] * 3,)) if full else None
    s.c8 = s.tv = None
    if case.kind == "pair":
        s.out, s.cross = D((n, 3, hw, hw)), D((n, 3, hw, hw))
        rc = lib.combat_trigger_pair_fwd(*head, P(s.out), P(s.cross), P(s.mse), stream())
    elif case.kind == "groups":
        s.out = D((rows, 3, hw, hw))
        rc = lib.combat_trigger_groups_fwd(*head, case.ps, P(s.out), P(s.mse), stream())
    elif variant in ("tv", "tv_bare"):
        s.out, s.tv = D((rows, 3, hw, hw)), D((rows * 3,))
        entry = lib.combat_trigger_tv_fwd if hw <= 64 else lib.combat_trigger_tv_big_fwd
        rc = entry(*head, P(s.out), P(s.mse), P(s.tv), stream())
    else:
        s.out = D((rows, 3, hw, hw))
        s.c8 = D((rows, hw, hw, 8), bf16) if full else None
        keep, idx = I(src)
        rc = lib.combat_trigger_fwd(*head, idx, P(s.out), P(s.c8), P(s.mse), stream())
    assert rc == 0, (case.id, variant, rc)
    check_all(s, case.id)
    out = host(s.out) if case.kind != "pair" else torch.cat([host(s.out), host(s.cross)])
    got = SimpleNamespace(out=out, c8=host(s.c8), mse=None if s.mse is None else host(s.mse).view(-1, 3),
                          tv=None if s.tv is None else host(s.tv).view(-1, 3))
    return E, got


@pytest.mark.parametrize("mode", ["exact", "bound"])
@pytest.mark.parametrize("case", IC.TRIGGER_CASES, ids=lambda c: c.id)
def test_trigger_forward(lib, case, mode):
    """combat_trigger_fwd (with and without out_c8 / mse_partial / src_index), combat_trigger_tv_fwd /
    combat_trigger_tv_big_fwd, combat_trigger_pair_fwd, combat_trigger_groups_fwd."""
    for variant in ("full", "bare") + (("tv", "tv_bare") if case.kind == "plain" else ()):
        E, got = launch_fwd(lib, case, mode, variant)
        IC.check_fwd(E, got, "%s (%s, %s)" % (case.id, mode, variant))


# ------------------------------------------------------------------------------------------------ trigger backward
def launch_bwd(lib, case, mode, name):
    d, s = operands(case, mode)
    cfg = IC.bwd_config(case, mode, name)
    E = IC.expect_bwd(case, mode, cfg)
    hw, n = case.hw, case.n
    s.d_out, s.d_out2, s.d_cross = S(cfg.d_out), S(cfg.d_out2), S(cfg.d_cross)
    s.out = S(E.out) if (cfg.l2 != 0 or cfg.tv != 0) else None
    s.dn = D((E.d.shape[0], hw, hw, 8), bf16)
    head = (P(s.x), P(s.noise), P(s.P), P(s.k1), d.rate, n, hw)
    if case.kind == "pair":
        rc = lib.combat_trigger_pair_bwd(*head, P(s.d_out), P(s.d_out2), P(s.out), cfg.l2, P(s.d_cross), cfg.pre_tanh,
                                         P(s.dn), stream())
    elif case.kind == "groups":
        rc = lib.combat_trigger_groups_bwd(*head, case.ps, P(s.d_out), P(s.d_out2), P(s.out), cfg.l2, cfg.pre_tanh, P(s.dn),
                                           stream())
    elif cfg.tv != 0:
        entry = lib.combat_trigger_tv_bwd if hw <= 64 else lib.combat_trigger_tv_big_bwd
        rc = entry(*head, P(s.d_out), P(s.d_out2), P(s.out), cfg.l2, cfg.tv, cfg.pre_tanh, P(s.dn), stream())
    else:
        rc = lib.combat_trigger_bwd(*head, P(s.d_out), P(s.d_out2), P(s.out), cfg.l2, cfg.pre_tanh, P(s.dn), stream())
    assert rc == 0, (case.id, name, rc)
    check_all(s, case.id)
    return E, host(s.dn)


@pytest.mark.parametrize("mode", ["exact", "bound"])
@pytest.mark.parametrize("case", IC.TRIGGER_CASES, ids=lambda c: c.id)
def test_trigger_backward(lib, case, mode):
    """combat_trigger_bwd, combat_trigger_tv_bwd / combat_trigger_tv_big_bwd, combat_trigger_pair_bwd (d_bd2 on the first
    half only, d_cross = NULL in the `l2` configuration), combat_trigger_groups_bwd; the configurations of
    image_exact_cases.bwd_config."""
    for name in IC.bwd_configs(case, mode):
        E, got = launch_bwd(lib, case, mode, name)
        IC.check_bwd(E, got, "%s (%s, %s)" % (case.id, mode, name))


def test_trigger_bound_mixed_without_tv(lib):
    """The plain entry point on the mixed gradient (the bound tables' plain cases carry a TV term and so take the
    total-variation entry points): one whole-plane and one strip case with tv_scale = 0."""
    for case in (IC.PLAIN_CASES[1], IC.PLAIN_CASES[3]):
        cfg = IC.bwd_config(case, "bound", "mixed")
        plain = SimpleNamespace(**{**vars(cfg), "tv": 0.0})
        d, s = operands(case, "bound")
        E = IC.expect_bwd(case, "bound", plain)
        s.d_out, s.d_out2, s.out = S(plain.d_out), S(plain.d_out2), S(E.out)
        s.dn = D((case.n, case.hw, case.hw, 8), bf16)
        assert lib.combat_trigger_bwd(P(s.x), P(s.noise), P(s.P), P(s.k1), d.rate, case.n, case.hw, P(s.d_out), P(s.d_out2),
                                      P(s.out), plain.l2, 0, P(s.dn), stream()) == 0
        check_all(s, case.id)
        IC.check_bwd(E, host(s.dn), "%s (bound, mixed without TV)" % case.id)


# ------------------------------------------------------------------------------------------------ DCT input
@pytest.mark.parametrize("kind", IC.DCT_KINDS)
@pytest.mark.parametrize("hw", IC.DCT_SHAPES)
def test_dct_u8(lib, hw, kind):
    """combat_dct_u8 with D = identity (hi = q exactly, lo = 0: the quantiser alone, on all 256 pipeline levels), a
    non-symmetric dyadic D (D q D^T exact: D against D^T) and the real DCT matrix (bound)."""
    x, Dm = IC.dct_data(hw, kind)
    E = IC.expect_dct(hw, kind)
    s = SimpleNamespace(x=S(x.astype(np.float64)), D=S(Dm), out=D((IC.DCT_N, hw, hw, 8), bf16))
    assert lib.combat_dct_u8(P(s.x), P(s.D), IC.DCT_N, hw, P(s.out), stream()) == 0
    check_all(s, "dct %d %s" % (hw, kind))
    IC.check_dct(E, host(s.out), "dct_u8 hw=%d %s" % (hw, kind))


# ------------------------------------------------------------------------------------------------ augmentation (copy paths)
@pytest.mark.parametrize("hw", IC.AUG_SHAPES)
def test_augment_copy_paths(lib, hw):
    """combat_augment_fwd / combat_augment_bwd without rotation: out_f32 equals the shifted / flipped source with zeros
    outside, out_c8 its hi / lo image with a zero w word, d_x the adjoint copy (c8_channels 8 and 16), `accumulate`
    adds onto a prior lattice value exactly; src_index; params = NULL is the identity."""
    a = IC.aug_data(hw)
    name = "augment hw=%d" % hw
    s = SimpleNamespace(x=S(a.x), params=S(a.params.astype(np.float64)), c8=D((a.n, hw, hw, 8), bf16), out=D((a.n, 3, hw, hw)))
    keep, idx = I(a.src)
    assert lib.combat_augment_fwd(P(s.x), idx, P(s.params), a.n, hw, P(s.c8), P(s.out), stream()) == 0
    check_all(s, name)
    R.report_mismatch(host(s.out), R.t64(R.augment_copy(a.x, a.src, a.params)), "out_f32 of " + name)
    R.report_mismatch(host(s.c8), R.c8_expect(host(s.out)), "out_c8 of " + name)
    R.assert_not_vacuous(host(s.out), "out_c8 of " + name)
    # the identity: no parameters, no index, no fp32 output
    s = SimpleNamespace(x=S(a.x), c8=D((IC.AUG_NX, hw, hw, 8), bf16))
    assert lib.combat_augment_fwd(P(s.x), None, None, IC.AUG_NX, hw, P(s.c8), None, stream()) == 0
    check_all(s, name)
    R.report_mismatch(host(s.c8), R.c8_expect(a.x), "out_c8 of %s (identity)" % name)
    adj = R.augment_adjoint(a.d, a.params)
    for cch, accumulate in ((8, 0), (16, 1), (16, 0), (8, 1)):
        s = SimpleNamespace(d=S(R.nhwc3(a.d, cch), bf16), params=S(a.params.astype(np.float64)),
                            dx=D((a.n, 3, hw, hw), f32, a.prior if accumulate else None))
        assert lib.combat_augment_bwd(P(s.d), cch, P(s.params), a.n, hw, P(s.dx), accumulate, stream()) == 0
        check_all(s, name)
        R.report_mismatch(host(s.dx), R.t64(adj + a.prior if accumulate else adj),
                          "d_x of %s (%d channels, accumulate %d)" % (name, cch, accumulate))


# ------------------------------------------------------------------------------------------------ warp
def test_warp_forward(lib):
    """combat_warp_fwd with a shared grid + src_index and with per-image grids: EQUAL on the lattice."""
    w = IC.warp_data()
    for grid, src in ((w.grids[0], w.src), (w.grids, None), (w.grids, w.src)):
        s = SimpleNamespace(x=S(w.x), grid=S(grid), out=D((w.n, 3, w.H, w.H)))
        keep, idx = I(src)
        assert lib.combat_warp_fwd(P(s.x), idx, P(s.grid), int(grid.ndim == 4), w.n, w.H, P(s.out), stream()) == 0
        check_all(s, "warp_fwd")
        R.report_mismatch(host(s.out), R.t64(R.warp_fwd(w.x, src, grid, w.n)), "out of warp_fwd (per-image grid %d)" % (grid.ndim == 4))


@pytest.mark.parametrize("groups,second", IC.WARP_BWD)
def test_warp_backward_grid(lib, groups, second):
    """combat_warp_bwd: 5 images in 2 ragged groups, 7 groups (the empty ones write zeros), with d_out2."""
    w = IC.warp_data()
    for grid in (w.grids, w.grids[1]):
        s = SimpleNamespace(x=S(w.x), d=S(w.d), d2=S(w.d2) if second else None, grid=S(grid), part=D((groups, w.H, w.H, 2)))
        assert lib.combat_warp_bwd(P(s.x), P(s.d), P(s.d2), P(s.grid), int(grid.ndim == 4), w.n, w.H, groups, P(s.part),
                                   stream()) == 0
        check_all(s, "warp_bwd")
        exp, _ = R.warp_bwd(w.x, w.d + w.d2 if second else w.d, grid, w.n, groups)
        R.report_mismatch(host(s.part), R.t64(exp), "partial [group][y][x][2] of warp_bwd (%d groups)" % groups)
        if groups > w.n:
            assert float(host(s.part)[w.n:].abs().max()) == 0.0


def test_warp_backward_input(lib):
    """combat_warp_bwd_input: the atomic sums are exact in any order on the lattice."""
    w = IC.warp_data()
    for grid in (w.grids, w.grids[0]):
        s = SimpleNamespace(d=S(w.d), grid=S(grid), dx=D((w.n, 3, w.H, w.H)))
        assert lib.combat_warp_bwd_input(P(s.d), P(s.grid), int(grid.ndim == 4), w.n, w.H, P(s.dx), stream()) == 0
        check_all(s, "warp_bwd_input")
        R.report_mismatch(host(s.dx), R.t64(R.warp_bwd_input(w.d, grid, w.n)[0]), "d_x of warp_bwd_input")
