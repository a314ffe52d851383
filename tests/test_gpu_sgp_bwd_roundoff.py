"""The temporal stage's backward kernels (sgp_bwd.hip behind ops_bwd.py) against fp64 references of the operands as each launch
receives them, element by element, within the first-order rounding bound of tests/roundoff.py: zero violations, every
activation gradient in a guarded NaN-filled buffer, both stream types, parameter gradients included.  The weight-gradient
forms are also held to BIT EQUALITY on exact operands (sgp_bwd_cases.exact_operand), plain, accumulating and through the
partials-only path.  Operands and their asserted conditions: tests/sgp_bwd_cases.py.  tests/test_roundoff_sgp_bwd_host.py proves
the bound and shows what falls outside it.  The assertions of test_gpu_bwd.py stay.  -m gpu only, `pytest -s` prints every
figure."""
import pytest
import torch

import roundoff as R
import sgp_cases as S
import sgp_bwd_cases as Bc
from helpers import GUARD, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
STREAMS = [BF, F32]


@pytest.fixture(scope="module")
def bops():
    from tdeed_amd import ops_bwd as o, _lib
    _lib.load()
    return o


def dev(x):
    return None if x is None else x.to(DEV).contiguous()


def enough_for_bias(ref):
    return int((ref.ref.abs() > 2.0 ** -10 * ref.ref.abs().max()).sum()) >= 10000


def check_stored(out, ref, dt, name):
    """`out` against the fp32 value `ref` stored as dt; the bias check where dt is bf16 and the case supplies the elements"""
    want = R.as_stored(ref, dt)
    R.assert_within(out, want, name)
    if dt == BF and enough_for_bias(want):
        R.assert_unbiased(out, want, name)


def guarded_with(shape, dt, base):
    """a guarded output that holds `base` (the old contents under `accumulate`) or NaN"""
    g = Guarded(shape, dt)
    if base is not None:
        g.view.copy_(base.to(DEV))
    return g


# ----------------------------------------------------------------------------- LayerNorm backward
LN_CASES = [(r, c, 0.0, False, False) for r, c in Bc.LN_SHAPES] + [(200, 368, S.OFFSET_RATIO, False, False), (200, 368, 0.0, True, False),
                                                                   (77, 32, 0.0, False, True), (77, 32, 0.0, True, True)]


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("rows,C,offset,acc,padded", LN_CASES)
def test_layernorm_bwd(bops, rows, C, offset, acc, padded, dt):
    """Rounding points of layernorm_bwd_kernel, as read there: x and dy are widened on load (Chunk<T>::load), the two passes,
    s1, s2 and rstd (g - s1 - xhat s2) run in fp32, the old value is added in fp32 under `accumulate`, ONE rounding in
    Chunk<T>::store.  dw / db: fp32 per lane over the wave's rows, per workgroup through LDS, then reduce_partials (the wide
    form at (520, 40): 65 partials); never rounded to bf16.  padded: ldx = ldy = C + 8 inside wider buffers, whose padding
    columns must stay untouched."""
    x, dy, w, base = Bc.ln_bwd_case(rows, C, dt, offset, acc)
    (dx_r, dw_r, db_r), st = R.layernorm_bwd_ref(x, dy, w, EPS, base)
    name = f"layernorm_bwd {(rows, C)} {dt} offset {offset} accumulate {acc} padded {padded}"
    Bc.check_norm_conditions(st, name)
    if not padded:
        g = guarded_with((rows, C), dt, base)
        _, dw, db = bops.layernorm_bwd(dev(x), dev(dy), dev(w), EPS, dx=g.view, accumulate=acc)
        dx = g.check(name)
    else:
        ld = C + 8
        wide = lambda v: torch.cat([v, torch.full((rows, 8), 3.0, dtype=dt)], 1).to(DEV).contiguous()    # noqa: E731
        g = Guarded((rows, ld), dt)
        if base is not None:
            g.view[:, :C].copy_(base.to(DEV))
        _, dw, db = bops.layernorm_bwd(wide(x), wide(dy), dev(w), EPS, dx=g.view, accumulate=acc, ldx=ld, ldy=ld, rows=rows, C=C)
        torch.cuda.synchronize()
        n = rows * ld
        assert bool(torch.isnan(g.flat[:GUARD]).all()) and bool(torch.isnan(g.flat[GUARD + n:]).all()), name + ": store outside"
        assert bool(torch.isnan(g.view[:, C:]).all()), name + ": store into the padding columns"
        dx = g.view[:, :C]
    check_stored(dx, dx_r, dt, name + " dx")
    R.assert_within(dw, dw_r, name + " dw")
    R.assert_within(db, db_r, name + " db")


# ----------------------------------------------------------------------------- GroupNorm backward
GN_CASES = [(s, 0.0, a) for s in Bc.GN_SHAPES for a in (False, True)] + [(Bc.GN_OFFSET_SHAPE, S.OFFSET_RATIO, True)]


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("shape,offset,acc", GN_CASES)
def test_groupnorm_bwd(bops, shape, offset, acc, dt):
    """Rounding points of groupnorm_bwd_kernel: the [T][cg] slabs of x and dy are widened into LDS, mean, the variance around
    it, s1, s2 are block sums in fp32, the old value is added in fp32 under `accumulate` (the only way temporal_train.py calls
    it), ONE rounding in `(T)o`.  dw / db: one fp32 chain over T per channel, then the clips in reduce_partials."""
    B, T, C = shape
    x, dy, w, base = Bc.gn_bwd_case(B, T, C, dt, offset, acc)
    (dx_r, dw_r, db_r), st = R.groupnorm_bwd_ref(x, dy, Bc.GN_G, w, EPS, base)
    name = f"groupnorm_bwd {shape} {dt} offset {offset} accumulate {acc}"
    Bc.check_norm_conditions(st, name)
    g = guarded_with(shape, dt, base)
    _, dw, db = bops.groupnorm_bwd(dev(x), dev(dy), Bc.GN_G, dev(w), EPS, dx=g.view, accumulate=acc)
    check_stored(g.check(name), dx_r, dt, name + " dx")
    R.assert_within(dw, dw_r, name + " dw")
    R.assert_within(db, db_r, name + " db")


# ----------------------------------------------------------------------------- depthwise-branch backward
@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("slabs", [False, True], ids=["one-gradient", "three-slabs"])
@pytest.mark.parametrize("shape", Bc.BRANCH_SHAPES)
def test_sgp_branch_bwd(bops, shape, slabs, dt):
    """Rounding points of sgp_branch_bwd_kernel / branch_bwd_core: o and the gradient tiles are widened into LDS, the forward
    products, d psi, d s, the five sums, the input gradient (one fma chain) and the weight gradients are fp32, ONE rounding in
    store_tile.  d_dw / d_db: fp32 per clip, the clips folded by reduce_partials.  three-slabs is the mixer's call: o slab 4
    of one (B, T, 6C) tensor, the gradients slabs 0, 2, 4 of another, every row stride 6C."""
    B, T, C, ks, up = shape
    got = Bc.branch_bwd_case(shape, dt, slabs)
    o, gs, dw, db = (*got[1], got[2], got[3]) if slabs else got
    d_o_r, dw_r, db_r, parts, unsure = R.branch_bwd_ref(o, *gs, ks, up, dw, db)
    name = f"sgp_branch_bwd {shape} {dt} {'three slabs' if slabs else 'one gradient'}"
    Bc.check_branch_conditions(parts, unsure, T, name)
    g = Guarded((B, T, C), dt)
    if slabs:
        cat, dcat = dev(got[0][0]).view(-1), dev(got[0][1]).view(-1)
        sl = lambda buf, i: buf[i * C:]                                        # noqa: E731  (row stride stays 6C)
        _, ddw, ddb = bops.sgp_branch_bwd(sl(cat, 4), (sl(dcat, 0), sl(dcat, 2), sl(dcat, 4)), ks, up, dev(dw), dev(db), d_o=g.view,
                                          ldo=6 * C, ldg=6 * C, B=B, T=T, C=C)
    else:
        _, ddw, ddb = bops.sgp_branch_bwd(dev(o), dev(gs[0]), ks, up, dev(dw), dev(db), d_o=g.view)
    check_stored(g.check(name), d_o_r, dt, name + " d_o")
    R.assert_within(ddw, dw_r, name + " d_dw")
    R.assert_within(ddb, db_r, name + " d_db")
    assert torch.equal(ddb[1], ddb[2]), name + ": the convw and convkw bias gradients are the same sum"


# ----------------------------------------------------------------------------- up-sampling backward
@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("T_hi,T_lo,wide", [(a, b, False) for a, b in Bc.UPSAMPLE_T] + [(25, 13, True)])
def test_upsample_bwd(bops, T_hi, T_lo, wide, dt):
    """Rounding points of upsample_bwd_kernel: the positions are fp32 (scale * t, as in the forward), a node gathers its
    contributions in one fp32 fma chain over t, ONE rounding in Chunk<T>::store.  wide: d_xu is a slab of a (B, T_hi, 6C)
    tensor (ld = 6C)."""
    B, C = 2, 24
    d_xu = Bc.upsample_bwd_case(T_hi, T_lo, dt, B, C, wide)
    ref = R.upsample_bwd_ref(d_xu, T_lo)
    name = f"upsample_bwd {T_hi} -> {T_lo} {dt} {'ld 6C' if wide else ''}"
    g = Guarded((B, T_lo, C), dt)
    if wide:
        full = dev(Bc.grad(171, f"w{T_hi}", (B, T_hi, 6 * C), dt)).view(-1)
        bops.upsample_bwd(full[5 * C:], T_lo, ld=6 * C, B=B, T_hi=T_hi, C=C, out=g.view)
    else:
        bops.upsample_bwd(dev(d_xu), T_lo, out=g.view)
    check_stored(g.check(name), ref, dt, name)


# ----------------------------------------------------------------------------- max-pool backward
@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("T_in,T_out,how", Bc.POOL_CASES)
def test_maxpool_bwd(bops, T_in, T_out, how, dt):
    """Rounding points of maxpool_bwd_kernel: comparisons on the widened values (exact), at most 3 fp32 adds, ONE rounding
    in Chunk<T>::store.  quarters: ties inside windows (the first maximum takes the gradient)."""
    x, dy = Bc.maxpool_bwd_case(T_in, T_out, dt, how)
    if how == "quarters" and T_in > T_out:
        assert Bc.count_ties(x, T_out) >= 10
    name = f"maxpool_bwd {T_in} -> {T_out} {how} {dt}"
    g = Guarded(tuple(x.shape), dt)
    bops.maxpool_bwd(dev(x), dev(dy), out=g.view)
    check_stored(g.check(name), R.maxpool_bwd_ref(x, dy), dt, name)


# ----------------------------------------------------------------------------- element-wise
@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("n", Bc.ELTWISE_N)
def test_eltwise(bops, n, dt):
    """Rounding points of eltwise_kernel: widened loads, fp32 arithmetic (erff, expf), ONE rounding in Chunk<T>::store.
    n = 8: one chunk (bf16); 8 * 257: one chunk beyond a workgroup; 64 * 96: several workgroups."""
    x, dy = Bc.eltwise_case(n, dt)
    for mode in (bops.GELU_FWD, bops.GELU_BWD, bops.ADD, bops.MUL):
        name = f"eltwise mode {mode} n {n} {dt}"
        g = Guarded((n,), dt)
        bops.eltwise(dev(x), None if mode == bops.GELU_FWD else dev(dy), mode, out=g.view)
        check_stored(g.check(name), R.eltwise_ref(x, dy, mode), dt, name)


# ----------------------------------------------------------------------------- weight gradient
def run_wgrad(bops, case, dY, X, X0, base=None):
    kern, M, N, K, bias, k0 = case
    if base is not None:
        dW, db = dev(base[0]).clone(), (dev(base[1]).clone() if bias else None)
        return bops.wgrad(dev(dY), dev(X), with_bias=bias, dW=dW, db=db, accumulate=True, X0=dev(X0), k0=k0)
    return bops.wgrad(dev(dY), dev(X), with_bias=bias, X0=dev(X0), k0=k0)


@pytest.mark.parametrize("case", Bc.WGRAD_CASES, ids=Bc.wgrad_id)
def test_wgrad(bops, case, monkeypatch):
    """Every dispatch branch of tdeed_wgrad, named in the id (sgp_bwd_cases.wgrad_branch restates the dispatch).  No rounding
    point but the fp32 accumulation: bf16 operands are exact in the MFMA, the M slices land in fp32 partials, reduce_partials
    folds them in order, `accumulate` adds the old value in fp32.
    On exact operands (m / 4, |m| <= 15) every partial sum is an fp32 number, so dW and db must EQUAL the fp64 product bit for
    bit: plain, accumulating onto an exact base, and through the partials-only path (LAZY_WGRAD, then materialize).
    On random operands the M-term bound (M + 4) 2^-23 sum |a| |b| is applied: sharp for M <= 1000; at M >= 4096 it is about
    2 % of a typical element, looser than the older 1e-4 max -- there the equality above is the check that bites."""
    kern, M, N, K, bias, k0 = case
    name = "wgrad " + Bc.wgrad_id(case)
    dY, X, X0, base = Bc.wgrad_operands(case, exact=True)
    for how in ("plain", "accumulate", "partials only"):
        want_W, want_b = R.wgrad_ref(dY, X, X0, k0, base if how == "accumulate" else None)
        if how == "partials only":
            monkeypatch.setattr(bops, "LAZY_WGRAD", True)
            lw, lb = run_wgrad(bops, case, dY, X, X0)
            monkeypatch.setattr(bops, "LAZY_WGRAD", False)
            assert isinstance(lw, bops.LazyFold) and (not bias or isinstance(lb, bops.LazyFold)), name
            dW, db = bops.materialize(lw), bops.materialize(lb)
        else:
            dW, db = run_wgrad(bops, case, dY, X, X0, base if how == "accumulate" else None)
        assert dW.shape == (N, K)
        assert torch.equal(dW.cpu().double(), want_W.ref), f"{name} {how}: dW differs from the exact product, worst " \
            f"{float((dW.cpu().double() - want_W.ref).abs().max()):.3e}"
        if bias:
            assert torch.equal(db.cpu().double(), want_b.ref), f"{name} {how}: db differs from the exact sum, worst " \
                f"{float((db.cpu().double() - want_b.ref).abs().max()):.3e}"
        else:
            assert db is None
    dY, X, X0, _ = Bc.wgrad_operands(case, exact=False)
    want_W, want_b = R.wgrad_ref(dY, X, X0, k0)
    dW, db = run_wgrad(bops, case, dY, X, X0)
    R.assert_within(dW, want_W, name + " random dW")
    if bias:
        R.assert_within(db, want_b, name + " random db")
