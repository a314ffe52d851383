"""The backward rules of tests/roundoff.py proved on the CPU.  Emulations of the temporal stage's backward kernels (sgp_bwd.hip:
layernorm_bwd, groupnorm_bwd, sgp_branch_bwd, upsample_bwd, maxpool_bwd, eltwise, the weight-gradient forms) in fp32 torch
arithmetic in the kernels' order, with a bf16 cast exactly where a kernel rounds -- its one store -- stay inside the bound with
zero violations in both stream types on every case of test_gpu_sgp_bwd_roundoff.py, parameter gradients included; each defect
of the lists below falls outside it on the SAME operands, and the test prints whether the older expressions of
test_gpu_bwd.py (`max|out - ref| / max|ref|` < 4e-2 for bf16 activation gradients, 2e-2 for parameter gradients under the bf16
stream, 2e-4 under fp32, 1e-4 for the weight gradient) would have let it pass.  No GPU."""
import numpy as np
import pytest
import torch

import roundoff as R
import sgp_cases as S
import sgp_bwd_cases as Bc
from test_roundoff_host import rne, truncate
from test_roundoff_sgp_host import emu_dw

BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
STREAMS = [BF, F32]


def old_act(out, ref, dt):
    return R.old_metric(out, ref) < (4e-2 if dt == BF else 2e-4)


def old_par(out, ref, dt):
    return R.old_metric(out, ref) < (2e-2 if dt == BF else 2e-4)


def must_fail(name, out, ref, old_pass):
    print(f"[defect] {name}: the older expressions {'LET IT PASS' if old_pass else 'catch it'}")
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(out, ref, name)


def store(v, dt, defects=()):
    if dt == BF:
        return truncate(v) if "truncating store" in defects else rne(v)
    return v


# ----------------------------------------------------------------------------- LayerNorm backward
def emu_layernorm_bwd(x, dy, w, base=None, defects=()):
    """layernorm_bwd_kernel: two passes, everything fp32, `old` added in fp32, ONE rounding at the store"""
    dt = x.dtype
    xf, g0 = x.float(), dy.float()
    rows, C = xf.shape
    mu = xf.sum(-1, keepdim=True) / C
    xc = xf - mu
    q = (xc * xc).sum(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(q / (C - 1 if "unbiased variance" in defects else C) + EPS)
    if "the neighbouring row's rstd" in defects:
        rstd = rstd.roll(1, 0)
    xh = xc * rstd
    wr = w.clone()
    if "previous chunk's w in the last chunk" in defects:
        wr[C - 8:] = w[C - 16:C - 8]
    g = g0 * wr
    s1 = torch.zeros(rows, 1) if "mean(g) dropped" in defects else g.sum(-1, keepdim=True) / C
    s2 = (g * xh).sum(-1, keepdim=True) / C
    o = rstd * (g - s1 - xh * s2)
    if base is not None and "old added behind the rounding" in defects:
        o = store(o, dt).float() + base.float()
    elif base is not None:
        o = o + base.float()
    p = g0 * xh
    return store(o, dt, defects), (p[:-1] if "dw without its last row" in defects else p).sum(0), g0.sum(0)


def ln_refs(x, dy, w, base=None):
    (dx, dw, db), st = R.layernorm_bwd_ref(x, dy, w, EPS, base)
    return R.as_stored(dx, x.dtype), dw, db, st


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("rows,C", Bc.LN_SHAPES)
def test_faithful_layernorm_bwd(rows, C, dt):
    for offset, acc in ((0.0, False), (S.OFFSET_RATIO, False), (0.0, True)):
        x, dy, w, base = Bc.ln_bwd_case(rows, C, dt, offset, acc)
        dx_r, dw_r, db_r, st = ln_refs(x, dy, w, base)
        Bc.check_norm_conditions(st, f"layernorm_bwd {(rows, C)} offset {offset}")
        dx, dw, db = emu_layernorm_bwd(x, dy, w, base)
        name = f"layernorm_bwd {(rows, C)} {dt} offset {offset} accumulate {acc}"
        R.assert_within(dx, dx_r, name + " dx")
        R.assert_within(dw, dw_r, name + " dw")
        R.assert_within(db, db_r, name + " db")
        if dt == BF and rows * C >= 12000:
            R.assert_unbiased(dx, dx_r, name)


LN_DEFECTS = [("truncating store", (200, 368), False), ("mean(g) dropped", (200, 368), False), ("mean(g) dropped", (64, 768), False),
              ("old added behind the rounding", (200, 368), True), ("the neighbouring row's rstd", (200, 368), False),
              ("unbiased variance", (7, 24), False), ("previous chunk's w in the last chunk", (200, 368), False),
              ("dw without its last row", (200, 368), False)]


@pytest.mark.parametrize("defect,shape,acc", LN_DEFECTS)
def test_layernorm_bwd_defects_fail(defect, shape, acc):
    x, dy, w, base = Bc.ln_bwd_case(*shape, BF, 0.0, acc)
    dx_r, dw_r, db_r, _ = ln_refs(x, dy, w, base)
    good, bad = emu_layernorm_bwd(x, dy, w, base), emu_layernorm_bwd(x, dy, w, base, (defect,))
    R.assert_within(good[0], dx_r, "faithful dx")
    R.assert_within(good[1], dw_r, "faithful dw")
    if defect == "dw without its last row":
        must_fail(defect, bad[1], dw_r, old_par(bad[1], dw_r.ref, BF))
    else:
        must_fail(defect, bad[0], dx_r, old_act(bad[0], dx_r.ref, BF))
    if defect == "truncating store":
        R.assert_unbiased(good[0], dx_r, "faithful")
        with pytest.raises(AssertionError, match="mean signed error"):
            R.assert_unbiased(bad[0], dx_r, defect)


# ----------------------------------------------------------------------------- GroupNorm backward
def emu_groupnorm_bwd(x, dy, G, w, base=None, defects=()):
    """groupnorm_bwd_kernel: the slab's mean, the variance around it, s1, s2 as block sums over n = T cg; (T) o at the store"""
    dt = x.dtype
    xf, g0 = x.float(), dy.float()
    B, T, C = xf.shape
    cg = C // G
    gi = torch.arange(C) // cg
    if "group boundary off by one channel" in defects:
        gi = ((torch.arange(C) + 1) // cg).clamp(max=G - 1)
    onehot = torch.zeros(C, G).index_put_((torch.arange(C), gi), torch.ones(C))
    cnt = onehot.sum(0)                                                         # channels per group
    n = cnt * (-(-T // 16) * 16 if "n of a full 16-row tile" in defects else T)
    gsum = lambda v: (v.sum(1) @ onehot)                                        # noqa: E731  (B, T, C) -> (B, G)
    per_c = lambda s: s[:, gi].unsqueeze(1)                                     # noqa: E731  (B, G) -> (B, 1, C)
    mean = per_c(gsum(xf) / n)
    xc = xf - mean
    rstd = per_c(1.0 / torch.sqrt(gsum(xc * xc) / n + EPS))
    xh = xc * rstd
    wr = w.clone()
    if "the next group's w on a group's last channel" in defects:
        last = torch.arange(cg - 1, C - 1, cg)
        wr[last] = w[last + 1]
    g = g0 * wr
    s1, s2 = per_c(gsum(g) / n), per_c(gsum(g * xh) / n)
    o = rstd * (g - s1 - xh * s2)
    if base is not None and "accumulate ignored" not in defects:
        o = o + base.float()
    return store(o, dt, defects), (g0 * xh).sum(1).sum(0), g0.sum(1).sum(0)


def gn_refs(x, dy, w, base=None):
    (dx, dw, db), st = R.groupnorm_bwd_ref(x, dy, Bc.GN_G, w, EPS, base)
    return R.as_stored(dx, x.dtype), dw, db, st


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("B,T,C", Bc.GN_SHAPES)
def test_faithful_groupnorm_bwd(B, T, C, dt):
    for offset, acc in ((0.0, False), (0.0, True)) + (((S.OFFSET_RATIO, True),) if (B, T, C) == Bc.GN_OFFSET_SHAPE else ()):
        x, dy, w, base = Bc.gn_bwd_case(B, T, C, dt, offset, acc)
        dx_r, dw_r, db_r, st = gn_refs(x, dy, w, base)
        Bc.check_norm_conditions(st, f"groupnorm_bwd {(B, T, C)} offset {offset}")
        dx, dw, db = emu_groupnorm_bwd(x, dy, Bc.GN_G, w, base)
        name = f"groupnorm_bwd {(B, T, C)} {dt} offset {offset} accumulate {acc}"
        R.assert_within(dx, dx_r, name + " dx")
        R.assert_within(dw, dw_r, name + " dw")
        R.assert_within(db, db_r, name + " db")
        if dt == BF and B * T * C >= 12000:
            R.assert_unbiased(dx, dx_r, name)


@pytest.mark.parametrize("defect,shape", [("n of a full 16-row tile", (2, 13, 368)), ("group boundary off by one channel", (2, 13, 368)),
                                          ("the next group's w on a group's last channel", (2, 13, 368)),
                                          ("accumulate ignored", (2, 13, 368))])
def test_groupnorm_bwd_defects_fail(defect, shape):
    x, dy, w, base = Bc.gn_bwd_case(*shape, BF, 0.0, True)
    dx_r, _, _, _ = gn_refs(x, dy, w, base)
    R.assert_within(emu_groupnorm_bwd(x, dy, Bc.GN_G, w, base)[0], dx_r, "faithful")
    bad = emu_groupnorm_bwd(x, dy, Bc.GN_G, w, base, (defect,))[0]
    must_fail(defect, bad, dx_r, old_act(bad, dx_r.ref, BF))


# ----------------------------------------------------------------------------- depthwise-branch backward
def corr(a, v, w, defects=(), which=""):
    """a += sum_k w[c][k] v[t + K // 2 - k] over the zero-haloed v (B, T, C), taps in order (fp32 fma chain)"""
    B, T, C = v.shape
    K = w.shape[1]
    h = K // 2
    pad = torch.zeros(B, T + 2 * h, C)
    pad[:, h:h + T] = v
    if which == "ckw" and "a halo row holding the neighbouring clip's row" in defects:
        pad[1:, h - 1] = v[:-1, T - 1]
    for k in range(K):
        off = (k - h) if (which == "psi" and "a correlation with k - hk" in defects) else (h - k)
        a = a + w[:, k] * pad[:, h + off:h + off + T]
    return a


def emu_branch_bwd(o, gs, ks, up, dw, db, defects=()):
    """branch_bwd_core: phases A (forward products, d psi, d s, the five sums), B (the input gradient, one chain), C (the
    weight gradients: one chain over T per tap and channel), the clips folded by reduce_partials.  One rounding: d_o's store"""
    dt = o.dtype
    of = o.float()
    gc, gi, gd = (g.float() for g in gs)
    if "g_inst and g_id swapped" in defects:
        gi, gd = gd, gi
    B, T, C = of.shape
    dwu = dw
    if "the previous channel's weights in the half-empty last tile" in defects:
        assert C % 16 == 8
        dwu = dw.clone()
        dwu[C - 8:] = dw[C - 9:C - 1]
    p = R.dw_split(dwu, db, ks, up)
    psi, cw, ckw = emu_dw(of, *p["psi"]), emu_dw(of, *p["cw"]), emu_dw(of, *p["ckw"])
    wf, bf_ = p["fc"]
    wg, bg = p["g"]
    mean_c = of.sum(1) / T
    pre = wg * mean_c + bg
    phi = torch.relu(pre)
    fc = wf * of + bf_
    vdpsi, vds = gc * (cw + ckw), gc * psi
    dphi, s_dpsi, s_ds, s_g, s_go = (gi * fc).sum(1), vdpsi.sum(1), vds.sum(1), gi.sum(1), (gi * of).sum(1)
    dpre = dphi if "dpre = dphi whatever the sign of pre" in defects else torch.where(pre > 0, dphi, torch.zeros_like(dphi))
    dmean = dpre * wg / (T + 2 * (up // 2) if "dmean over T + 2 halo" in defects else T)
    a = gd + gi * (wf * phi).unsqueeze(1) + dmean.unsqueeze(1)
    a = corr(a, vdpsi, p["psi"][0], defects, "psi")
    a = corr(a, vds, p["cw"][0], defects, "cw")
    a = corr(a, vds, p["ckw"][0], defects, "ckw")
    cols = []
    for src, K in ((vdpsi, ks), (vds, ks), (vds, up)):
        for k in range(K):
            cols.append((src * R.shifted(of, k - K // 2)).sum(1).sum(0))
    cols += [(phi * s_go).sum(0), (dpre * mean_c).sum(0)]
    rows5 = [s_dpsi.sum(0), s_ds.sum(0), (s_dpsi if "the convkw bias gradient from s_dpsi" in defects else s_ds).sum(0),
             (phi * s_g).sum(0), dpre.sum(0)]
    return store(a, dt, defects), torch.stack(cols, 1), torch.stack(rows5)


def branch_case(shape, dt, slabs):
    got = Bc.branch_bwd_case(shape, dt, slabs)
    return (*got[1], got[2], got[3]) if slabs else got


def branch_refs(o, gs, ks, up, dw, db):
    d_o, d_dw, d_db, parts, unsure = R.branch_bwd_ref(o, *gs, ks, up, dw, db)
    return R.as_stored(d_o, o.dtype), d_dw, d_db, parts, unsure


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("slabs", [False, True])
@pytest.mark.parametrize("shape", Bc.BRANCH_SHAPES)
def test_faithful_branch_bwd(shape, slabs, dt):
    B, T, C, ks, up = shape
    o, gs, dw, db = branch_case(shape, dt, slabs)
    d_o_r, dw_r, db_r, parts, unsure = branch_refs(o, gs, ks, up, dw, db)
    name = f"sgp_branch_bwd {shape} {dt} {'three slabs' if slabs else 'one gradient'}"
    Bc.check_branch_conditions(parts, unsure, T, name)
    d_o, d_dw, d_db = emu_branch_bwd(o, gs, ks, up, dw, db)
    R.assert_within(d_o, d_o_r, name + " d_o")
    R.assert_within(d_dw, dw_r, name + " d_dw")
    R.assert_within(d_db, db_r, name + " d_db")
    assert torch.equal(d_db[1], d_db[2]) and torch.equal(db_r.ref[1], db_r.ref[2])


BRANCH_DEFECTS = [("a halo row holding the neighbouring clip's row", 0, False), ("a correlation with k - hk", 2, False),
                  ("dpre = dphi whatever the sign of pre", 2, False), ("dmean over T + 2 halo", 2, False),
                  ("the convkw bias gradient from s_dpsi", 2, False),
                  ("the previous channel's weights in the half-empty last tile", 0, False), ("g_inst and g_id swapped", 2, True),
                  ("truncating store", 2, False)]


@pytest.mark.parametrize("defect,case,slabs", BRANCH_DEFECTS)
def test_branch_bwd_defects_fail(defect, case, slabs):
    shape = Bc.BRANCH_SHAPES[case]                            # (2, 13, 24, 5, 13): C % 16 == 8, two clips; (3, 25, 48, 7, 33)
    B, T, C, ks, up = shape
    o, gs, dw, db = branch_case(shape, BF, slabs)
    d_o_r, dw_r, db_r, _, _ = branch_refs(o, gs, ks, up, dw, db)
    R.assert_within(emu_branch_bwd(o, gs, ks, up, dw, db)[0], d_o_r, "faithful")
    bad = emu_branch_bwd(o, gs, ks, up, dw, db, (defect,))
    if defect == "the convkw bias gradient from s_dpsi":
        must_fail(defect, bad[2], db_r, old_par(bad[2], db_r.ref, BF))
    else:
        must_fail(defect, bad[0], d_o_r, old_act(bad[0], d_o_r.ref, BF))


# ----------------------------------------------------------------------------- up-sampling backward
def emu_upsample_bwd(g, T_lo, defects=()):
    """upsample_bwd_kernel: the fp32 positions of the forward, one fma chain over t per node, one store"""
    dt = g.dtype
    gf = g.float()
    B, T_hi, C = gf.shape
    if T_hi == T_lo:
        return g.clone()
    if "align_corners=False positions" in defects:
        xr = torch.zeros(B, C, T_lo, requires_grad=True)
        torch.nn.functional.interpolate(xr, size=T_hi, mode="linear", align_corners=False).backward(gf.transpose(1, 2))
        return store(xr.grad.transpose(1, 2), dt)
    f32 = np.float32
    scale = f32(T_lo - 1) / f32(T_hi - 1) if T_hi > 1 else f32(0)
    out = torch.zeros(B, T_lo, C)
    last = T_hi - 1 if "the last node without t = T_hi - 1" in defects else T_hi
    for t_ in range(last):
        src = f32(scale * f32(t_))
        i0 = int(src)
        i1 = i0 + (1 if i0 < T_lo - 1 else 0)
        l1 = f32(min(max(src - f32(i0), f32(0)), f32(1)))
        wgt = {}
        wgt[i0] = wgt.get(i0, f32(0)) + (f32(1) - l1)
        wgt[i1] = wgt.get(i1, f32(0)) + l1
        for j, wv in wgt.items():
            if wv != 0:
                out[:, j] = out[:, j] + float(wv) * gf[:, t_]
    return store(out, dt, defects)


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("T_hi,T_lo", Bc.UPSAMPLE_T)
def test_faithful_upsample_bwd(T_hi, T_lo, dt):
    g = Bc.upsample_bwd_case(T_hi, T_lo, dt)
    ref = R.upsample_bwd_ref(g, T_lo)
    xr = torch.zeros(2, 24, T_lo, dtype=torch.float64, requires_grad=True)
    if T_hi != T_lo:                                          # the reference is the transpose of nn.Upsample's forward
        torch.nn.functional.interpolate(xr, size=T_hi, mode="linear", align_corners=True).backward(g.double().transpose(1, 2))
        assert float((ref.ref - xr.grad.transpose(1, 2)).abs().max()) < 1e-12
    R.assert_within(emu_upsample_bwd(g, T_lo), R.as_stored(ref, dt), f"upsample_bwd {T_hi} -> {T_lo} {dt}")


@pytest.mark.parametrize("defect", ["the last node without t = T_hi - 1", "align_corners=False positions", "truncating store"])
def test_upsample_bwd_defects_fail(defect):
    g = Bc.upsample_bwd_case(100, 50, BF)
    ref = R.as_stored(R.upsample_bwd_ref(g, 50), BF)
    R.assert_within(emu_upsample_bwd(g, 50), ref, "faithful")
    bad = emu_upsample_bwd(g, 50, (defect,))
    must_fail(defect, bad, ref, old_act(bad, ref.ref, BF))


# ----------------------------------------------------------------------------- max-pool backward
def emu_maxpool_bwd(x, dy, defects=()):
    """maxpool_bwd_kernel: an input gathers the windows whose first maximum it is; fp32 adds, one store"""
    dt = x.dtype
    xf, g = x.float(), dy.float()
    B, T_in, C = xf.shape
    T_out = g.shape[1]
    out = torch.zeros(B, T_in, C)
    for i in range(T_out):
        lo = (i * T_in) // T_out
        hi = ((i + 1) * T_in) // T_out if "a window end computed with floor" in defects else -((-(i + 1) * T_in) // T_out)
        w = xf[:, lo:hi]
        at_max = w == w.amax(1, keepdim=True)
        pick = at_max.flip(1) if "a tie going to the last maximum" in defects else at_max
        first = pick & pick.float().cumsum(1).eq(1)
        first = first.flip(1) if "a tie going to the last maximum" in defects else first
        out[:, lo:hi] = out[:, lo:hi] + first * g[:, i:i + 1]
    return store(out, dt, defects)


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("T_in,T_out,how", Bc.POOL_CASES)
def test_faithful_maxpool_bwd(T_in, T_out, how, dt):
    x, dy = Bc.maxpool_bwd_case(T_in, T_out, dt, how)
    ref = R.maxpool_bwd_ref(x, dy)
    if how == "quarters" and T_in > T_out:
        assert Bc.count_ties(x, T_out) >= 10, Bc.count_ties(x, T_out)
    xr = x.double().transpose(1, 2).clone().requires_grad_(True)
    if how == "preimage":                                     # no ties: torch's own backward is the same function
        torch.nn.functional.adaptive_max_pool1d(xr, T_out).backward(dy.double().transpose(1, 2))
        assert torch.equal(ref.ref, xr.grad.transpose(1, 2))
    R.assert_within(emu_maxpool_bwd(x, dy), R.as_stored(ref, dt), f"maxpool_bwd {T_in} -> {T_out} {how} {dt}")


@pytest.mark.parametrize("defect,T", [("a tie going to the last maximum", (25, 13)), ("a window end computed with floor", (25, 13)),
                                      ("a window end computed with floor", (125, 63))])
def test_maxpool_bwd_defects_fail(defect, T):
    x, dy = Bc.maxpool_bwd_case(*T, BF, "quarters")
    ref = R.as_stored(R.maxpool_bwd_ref(x, dy), BF)
    R.assert_within(emu_maxpool_bwd(x, dy), ref, "faithful")
    bad = emu_maxpool_bwd(x, dy, (defect,))
    must_fail(defect, bad, ref, old_act(bad, ref.ref, BF))


# ----------------------------------------------------------------------------- element-wise
def emu_eltwise(x, dy, mode, defects=()):
    """eltwise_kernel: fp32 arithmetic on the loaded values, one store"""
    dt = x.dtype
    a, b = x.float(), dy.float()
    c = lambda v: torch.tensor(v, dtype=F32)                                    # noqa: E731
    if mode == 0:
        o = 0.5 * a * (1.0 + torch.erf(a * c(0.70710678118654752440)))
    elif mode == 1:
        if "the tanh form's derivative" in defects:
            ar = a.clone().requires_grad_(True)
            torch.nn.functional.gelu(ar, approximate="tanh").backward(b)
            return store(ar.grad, dt)
        cdf = 0.5 * (1.0 + torch.erf(a * c(0.70710678118654752440)))
        pdf = c(0.39894228040143267794) * torch.exp(-0.5 * a * a)
        o = b * (cdf + (pdf if "pdf without its factor x" in defects else a * pdf))
    else:
        o = a + b if mode == 2 else a * b
    return store(o, dt, defects)


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("n", Bc.ELTWISE_N)
def test_faithful_eltwise(n, dt):
    x, dy = Bc.eltwise_case(n, dt)
    for mode in range(4):
        R.assert_within(emu_eltwise(x, dy, mode), R.as_stored(R.eltwise_ref(x, dy, mode), dt), f"eltwise mode {mode} n {n} {dt}")
    xr = x.double().clone().requires_grad_(True)
    torch.nn.functional.gelu(xr).backward(dy.double())
    assert float((R.gelu_bwd(x, dy).ref - xr.grad).abs().max()) < 1e-12


@pytest.mark.parametrize("defect,dt", [("the tanh form's derivative", F32), ("pdf without its factor x", BF),
                                       ("pdf without its factor x", F32), ("truncating store", BF)])
def test_gelu_bwd_defects_fail(defect, dt):
    x, dy = Bc.eltwise_case(64 * 96, dt)
    ref = R.as_stored(R.eltwise_ref(x, dy, 1), dt)
    R.assert_within(emu_eltwise(x, dy, 1), ref, "faithful")
    bad = emu_eltwise(x, dy, 1, (defect,))
    must_fail(defect, bad, ref, old_act(bad, ref.ref, dt))


# ----------------------------------------------------------------------------- weight gradient
def emu_wgrad(dY, X, X0=None, k0=0, base=None, bias=True, defects=(), X0_wide=None):
    """the weight-gradient forms: fp32 accumulation of exact products over 64-row chunks and M slices, then the ordered fold"""
    M = dY.shape[0]
    Xe = X.float().clone()
    if X0 is not None:
        Xe[:, :k0] = X0.float()[:, :k0]
        if "column k0 of the splice from the wrong operand" in defects:
            Xe[:, k0] = X0_wide.float()[:, k0]
    Mu = M - M % 64 if "the rows of the last partial chunk dropped" in defects else M
    Yf = dY.float()
    dW, db = torch.zeros(Yf.shape[1], Xe.shape[1]), torch.zeros(Yf.shape[1])
    slices = list(range(0, Mu, 1024))
    for z, m0 in enumerate(slices):
        m1 = min(Mu, m0 + 1024)
        dW = dW + Yf[m0:m1].T @ Xe[m0:m1]
        if z == 0 or "the bias from the first slice only" not in defects:
            db = db + Yf[m0:m1].sum(0)
    if base is not None:
        dW, db = dW + base[0], db + base[1]
    return dW, (db if bias else None)


def exact_want(case, acc):
    dY, X, X0, base = Bc.wgrad_operands(case, exact=True)
    dW, db = R.wgrad_ref(dY, X, X0, case[5], base if acc else None)
    assert torch.equal(dW.ref.float().double(), dW.ref) and torch.equal(db.ref.float().double(), db.ref), "not fp32 numbers"
    return (dY, X, X0, base), dW.ref.float(), db.ref.float()


@pytest.mark.parametrize("case", Bc.WGRAD_CASES, ids=Bc.wgrad_id)
def test_faithful_wgrad(case):
    kern, M, N, K, bias, k0 = case
    for acc in (False, True):
        (dY, X, X0, base), dW, db = exact_want(case, acc)
        got = emu_wgrad(dY, X, X0, k0, base if acc else None, bias)
        assert torch.equal(got[0], dW) and (not bias or torch.equal(got[1], db)), (case, acc)
    dY, X, X0, base = Bc.wgrad_operands(case, exact=False)
    dW_r, db_r = R.wgrad_ref(dY, X, X0, k0)
    got = emu_wgrad(dY, X, X0, k0, None, bias)
    R.assert_within(got[0], dW_r, f"wgrad {Bc.wgrad_id(case)} random dW")
    if bias:
        R.assert_within(got[1], db_r, f"wgrad {Bc.wgrad_id(case)} random db")


def test_wgrad_ids_name_every_dispatch_branch():
    assert len({Bc.wgrad_id(c) for c in Bc.WGRAD_CASES}) == len(Bc.WGRAD_CASES)
    assert {c[0] for c in Bc.WGRAD_CASES} == {"wgrad_kernel_f32", "wgrad_kernel_bf16", "wgrad_mfma", "wgrad_tr", "wgrad_tr128",
                                              "wgrad_tr160"}
    for c in Bc.WGRAD_CASES:
        assert Bc.wgrad_branch(c[1], c[2], c[3], Bc.wgrad_dtype(c), c[4]) == c[0], c


@pytest.mark.parametrize("defect,case", [("the rows of the last partial chunk dropped", ("wgrad_tr", 4099, 152, 56, True, 0)),
                                         ("column k0 of the splice from the wrong operand", ("wgrad_tr", 4099, 152, 56, True, 8)),
                                         ("the bias from the first slice only", ("wgrad_tr128", 4099, 320, 320, True, 0))])
def test_wgrad_defects_are_unequal_on_exact_operands(defect, case):
    """equality on exact operands catches them; on random operands at M >= 4096 the derived bound is too loose to (printed)"""
    kern, M, N, K, bias, k0 = case
    (dY, X, X0, base), dW, db = exact_want(case, False)
    X0w = None if X0 is None else torch.cat([X0, Bc.exact_operand(139, "X0w", (M, 8), BF)], 1)
    bad = emu_wgrad(dY, X, X0, k0, None, bias, (defect,), X0w)
    which = 1 if "bias" in defect else 0
    want = (dW, db)[which]
    print(f"[defect] {defect}: the older expression (1e-4) {'LET IT PASS' if R.old_metric(bad[which], want) < 1e-4 else 'catches it'} "
          f"on exact operands")
    assert not torch.equal(bad[which], want)
    dYr, Xr, X0r, _ = Bc.wgrad_operands(case, exact=False)
    X0rw = None if X0r is None else torch.cat([X0r, S.rnd(139, "X0rw", (M, 8)).to(BF)], 1)
    badr = emu_wgrad(dYr, Xr, X0r, k0, None, bias, (defect,), X0rw)
    ref = R.wgrad_ref(dYr, Xr, X0r, k0)[which]
    err = (R.f64(badr[which]) - ref.ref).abs()
    print(f"[defect] {defect}: on random operands {int((err > ref.d).sum())} of {err.numel()} elements outside the M-term bound, "
          f"old metric {R.old_metric(badr[which], ref.ref):.2e}")
