"""The SGP stage's part of tests/roundoff.py proved on the CPU.  Emulations of the five launches (sgp_front, mixer_front and
the three modes of sgp_gemm) in fp32 torch arithmetic in the kernels' order, with bf16 casts exactly where the kernels round,
stay inside the bound with zero violations in both stream types; each defect of the list below falls outside it on the SAME
operands, and the test prints whether the older expressions (test_gpu_r5.py: `max|out - ref| < 2e-2 max(1, max|ref|)`, 2e-3
for fp32 outputs, sums within `1e-3 sqrt(C) max|out|`; the golden tolerance 4e-2 / 1e-4) would have let it pass.  No GPU."""
import numpy as np
import pytest
import torch

import roundoff as R
import sgp_cases as S
from test_roundoff_host import rne, truncate

BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5


def old_r5(out, ref, dt):
    o, r = R.f64(out), R.f64(ref)
    return float((o - r).abs().max()) < (2e-2 if dt == BF else 2e-3) * max(1.0, float(r.abs().max()))


def old_golden(out, ref, dt):
    o, r = R.f64(out), R.f64(ref)
    return float((o - r).abs().max()) < (4e-2 if dt == BF else 1e-4) * max(1.0, float(r.abs().max()))


def old_sums(got, v, dims):
    vv, n = R.f64(v), v.shape[-1]
    return float((R.f64(got)[..., 0] - vv.sum(dims)).abs().max()) < 1e-3 * n ** 0.5 * max(1.0, float(vv.abs().max()))


def must_fail(name, out, ref, old_pass, match="outside the rounding bound"):
    print(f"[defect] {name}: the older expressions {'LET IT PASS' if old_pass else 'catch it'}")
    with pytest.raises(AssertionError, match=match):
        R.assert_within(out, ref, name)


def store(v, dt, defects=()):
    if dt == BF:
        return truncate(v) if "truncating store" in defects else rne(v)
    return v


# ----------------------------------------------------------------------------- emulations
def emu_row_stats(xf, eps, rowstat=None, defects=()):
    """ln_row_stats / ln_row_stats_load: one pass, fp32"""
    C = xf.shape[-1]
    if rowstat is not None and rowstat.dim() == 2:
        r = rowstat.view(*xf.shape[:-1], 2)
        return r[..., 0], r[..., 1]
    if rowstat is not None:
        s, q = torch.zeros(rowstat.shape[1]), torch.zeros(rowstat.shape[1])
        for p in rowstat:                                  # a row's parts in order
            s, q = s + p[:, 0], q + p[:, 1]
        s, q = s.view(xf.shape[:-1]), q.view(xf.shape[:-1])
    else:
        s, q = xf.sum(-1), (xf * xf).sum(-1)
    m = s / C
    var = (q / C - m * m).clamp_min(0.0)
    if "unbiased variance" in defects:
        var = var * (C / (C - 1.0))
    m, rs = m, 1.0 / torch.sqrt(var + eps)
    if "statistics of the neighbouring row" in defects:
        m, rs = m.roll(1, -1), rs.roll(1, -1)
    return m, rs


def emu_dw(o, w, b, defects=(), which=""):
    """one depthwise branch: bias, then the taps in order (fp32)"""
    B, T, C = o.shape
    K = w.shape[1]
    h = K // 2
    pad = torch.zeros(B, T + 2 * h + 1, C)
    pad[:, h:h + T] = o
    shift = 0
    if which == "ckw" and "neighbouring clip's row in one tap" in defects:
        pad[1:, h - 1] = o[:-1, T - 1]                     # the row in front of a clip is the previous clip's last row
    if which == "ckw" and "window shifted by one row" in defects:
        shift = 1
    acc = b.expand(B, T, C).clone()
    for k in range(K):
        acc = acc + w[:, k] * pad[:, k + shift:k + shift + T]
    return acc


def emu_branches(o, dw, db, ks, up, defects=()):
    B, T, C = o.shape
    if "previous channel's weight in the last half tile" in defects:
        assert C % 16 == 8
        dw = dw.clone()
        dw[C - 8:] = dw[C - 9:C - 1].clone()
    p = R.dw_split(dw, db, ks, up)
    psi, cw, ckw = emu_dw(o, *p["psi"]), emu_dw(o, *p["cw"]), emu_dw(o, *p["ckw"], defects, "ckw")
    nmean = T + 2 * (up // 2) if "phi from a mean over T + 2 halo rows" in defects else T
    mean_c = o.sum(1) / nmean
    phi = torch.relu(p["g"][0] * mean_c + p["g"][1])
    inst = (p["fc"][0] * o + p["fc"][1]) * phi.unsqueeze(1)
    if "instant branch dropped" in defects:
        inst = torch.zeros_like(inst)
    return (cw + ckw) * psi, inst


def emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db, rowstat=None, defects=()):
    """-> (y in the stream's type, y16, chsum (B, C, 2))"""
    xf = x.float()
    m, rs = emu_row_stats(xf, EPS, rowstat, defects)
    o = (xf - m.unsqueeze(-1)) * rs.unsqueeze(-1) * ln_w + ln_b              # not rounded in either stream type
    gate, inst = emu_branches(o, dw, db, ks, up, defects)
    res = xf + ((inst + gate) + o)
    y = store(res, x.dtype, defects)
    v = res if "sums of un-rounded values" in defects else y.float()
    return y, rne(res), torch.stack([v.sum(1), (v * v).sum(1)], -1)


def emu_upsample(xn, T_hi, defects=()):
    B, T_lo, C = xn.shape
    if T_hi == T_lo:
        return xn
    if "align_corners=False" in defects:
        return torch.nn.functional.interpolate(xn.transpose(1, 2), size=T_hi, mode="linear", align_corners=False).transpose(1, 2)
    f32 = np.float32
    scale = f32(T_lo - 1) / f32(T_hi - 1) if T_hi > 1 else f32(0)
    sp = (scale * np.arange(T_hi, dtype=np.float32)).astype(np.float32)
    i0 = sp.astype(np.int64)
    i1 = i0 + (i0 < T_lo - 1)
    l1 = torch.from_numpy(np.clip(sp - i0.astype(np.float32), 0, 1).astype(np.float32)).view(1, -1, 1)
    l0 = 1.0 - l1
    return l0 * xn[:, torch.from_numpy(i0)] + l1 * xn[:, torch.from_numpy(i1)]


def emu_mixer_front(z, xlo, cat_dt, ks, up, ln1, ln2, dwb1, dwb2, rowstat_z=None, rowstat_x=None, defects=()):
    sdt, T_hi = z.dtype, z.shape[1]
    sr = lambda v: v.to(sdt).float()                                           # noqa: E731  round_to<T>
    ln = lambda v, p, rst: (v - emu_row_stats(v, EPS, rst)[0].unsqueeze(-1)) * emu_row_stats(v, EPS, rst)[1].unsqueeze(-1) * p[0] + p[1]   # noqa: E731
    zn = sr(ln(z.float(), ln1, rowstat_z))
    if "LN2 after the up-sampling" in defects:
        xu = sr(ln(sr(emu_upsample(xlo.float(), T_hi)), ln2, None))
    else:
        xu = sr(emu_upsample(sr(ln(xlo.float(), ln2, rowstat_x)), T_hi, defects))
    g1, i1 = emu_branches(zn, *dwb1, ks, up)
    g2, i2 = emu_branches(xu, *dwb2, ks, up)
    slabs = [g2, g1, i1, i2, zn, xu] if "out1 and out2 swapped" in defects else [g1, g2, i1, i2, zn, xu]
    return store(torch.cat(slabs, -1), cat_dt, defects)


def sg_gelu(x, rcp=0.0, ex=0.0):
    """sg_gelu of sgp_gemm.hip in fp32; rcp / ex: relative error pushed into rcpf / exp2f"""
    c = lambda v: torch.tensor(v, dtype=F32)                                    # noqa: E731
    z = x.abs() * c(0.70710678118654752440)
    tt = (1.0 / (c(0.3275911) * z + 1.0)) * c(1.0 + rcp)
    poly = tt * (tt * (tt * (tt * (tt * c(1.061405429) + c(-1.453152027)) + c(1.421413741)) + c(-0.284496736)) + c(0.254829592))
    e = 1.0 - poly * torch.exp2(c(-1.44269504088896341) * z * z) * c(1.0 + ex)
    return 0.5 * x * (1.0 + torch.copysign(e, x))


def emu_gn_fc1(y, chs, gn_w, gn_b, W, bias, G=16, defects=()):
    """MODE 0: chs (parts, B, K, 2)"""
    B, T, K = y.shape
    cg = K // G
    s = torch.zeros(B, K, 2)
    for p in chs:
        s = s + p
    gi = torch.arange(K) // cg
    if "group boundaries off by one channel" in defects:
        gi = ((torch.arange(K) + 1) // cg).clamp(max=G - 1)
    sg = torch.zeros(B, G, 2).index_add_(1, gi, s)
    n = float(cg * (-(-T // 16) * 16 if "n of a full 16-row tile" in defects else T))
    mean = sg[..., 0] / n
    rstd = 1.0 / torch.sqrt((sg[..., 1] / n - mean * mean).clamp_min(0.0) + EPS)
    sc = rstd[:, gi] * gn_w
    sh = -mean[:, gi] * sc + gn_b
    a = rne(y.float() * sc.unsqueeze(1) + sh.unsqueeze(1)).float()                # the MFMA's B operand
    Ku = K - K % 128 if "last k-chunk dropped" in defects else K
    b = bias
    if "neighbouring feature tile's bias" in defects:
        N = W.shape[0]
        assert N % 64
        b = bias.clone()
        b[N - N % 64:] = bias[N - N % 64 - 16:N - 16]
    return store(sg_gelu(a[..., :Ku] @ W[:, :Ku].T + b), BF, defects)


def tile_sums(v, width, dim):
    """(sum, sum of squares) of v over consecutive tiles of `width` along dim -> (tiles, ..., 2)"""
    return torch.stack([torch.stack([c.sum(dim), (c * c).sum(dim)], -1) for c in v.split(width, dim)])


def emu_fc2(H, W, bias, resid, pool=False, defects=()):
    """MODE 1 -> (out, rowstat_part (nct, B*T, 2), pooled, rowstat_pool_part)"""
    B, T, K = H.shape
    N = W.shape[0]
    v = H.float() @ W.T + bias + resid.float()
    out = store(v, resid.dtype, defects)
    vs = v if "sums of un-rounded values" in defects else out.float()
    rsp = tile_sums(vs.reshape(B * T, N), 64, -1)
    if not pool:
        return out, rsp, None, None
    a, b = out[:, 0::2], out[:, 1::2]
    if "pooled rows paired as (2i - 1, 2i)" in defects:
        b = torch.cat([out[:, :1], out[:, 1:-1:2]], 1)
    pooled = torch.maximum(a, b)
    return out, rsp, pooled, tile_sums(pooled.float().reshape(B * (T // 2), N), 64, -1)


def emu_cat_fc(A, W, bias, odt, MT=1, defects=()):
    """MODE 2 -> (out, out16, chs_out (NJ, B, N, 2))"""
    v = sg_gelu(A.float() @ W.T + bias)
    out = store(v, odt, defects)
    vs = v if "sums of un-rounded values" in defects else out.float()
    return out, rne(out.float()), tile_sums(vs, 16 * MT, 1)


# ----------------------------------------------------------------------------- sgp_front
def front_case(shape, dt, offset=0.0):
    B, T, C, ks, up = shape
    x = S.stream_input(71, f"x{shape}", (B, T, C), dt, offset)
    ln_w, ln_b = S.ln_params(72, f"ln{C}", C)
    dw, db = S.branch_params(73, f"dw{C}", C, ks, up)
    return x, ln_w, ln_b, dw, db


def front_ref(x, ks, up, ln_w, ln_b, dw, db, rowstat=None):
    y, parts = R.sgp_front_ref(x, ks, up, ln_w, ln_b, dw, db, EPS, rowstat)
    return R.as_stored(y, x.dtype), parts


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("shape", S.FRONT_SHAPES[:4])
def test_faithful_sgp_front(shape, dt):
    B, T, C, ks, up = shape
    for offset in (0.0, S.OFFSET_RATIO):
        x, ln_w, ln_b, dw, db = front_case(shape, dt, offset)
        sums = S.row_sums(x)
        for how, rst in (("in-kernel", None), ("mean rstd", S.row_mean_rstd(x)), ("1 part", S.split_parts(sums, 1)),
                         ("3 parts", S.split_parts(sums, 3))):
            ref, parts = front_ref(x, ks, up, ln_w, ln_b, dw, db, rst)
            if not offset:
                S.check_front_conditions(x.float(), parts, f"{shape}")
            y, y16, chs = emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db, rst)
            R.assert_within(y, ref, f"sgp_front {shape} {dt} offset {offset} {how}")
            assert torch.equal(y16, y.to(BF))
            R.assert_sums_consistent(chs, y, (1,), "chsum")


FRONT_DEFECTS = [("instant branch dropped", 2), ("neighbouring clip's row in one tap", 0), ("window shifted by one row", 2),
                 ("previous channel's weight in the last half tile", 0), ("phi from a mean over T + 2 halo rows", 2),
                 ("statistics of the neighbouring row", 2), ("unbiased variance", 0), ("truncating store", 2)]


@pytest.mark.parametrize("defect,case", FRONT_DEFECTS)
def test_sgp_front_defects_fail(defect, case):
    shape = S.FRONT_SHAPES[case]                              # (2, 13, 24, 5, 13): C % 16 == 8, C = 24; (3, 25, 48, 7, 33)
    B, T, C, ks, up = shape
    x, ln_w, ln_b, dw, db = front_case(shape, BF)
    ref, _ = front_ref(x, ks, up, ln_w, ln_b, dw, db)
    R.assert_within(emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db)[0], ref, "faithful")
    bad = emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db, defects=(defect,))[0]
    must_fail(defect, bad, ref, old_golden(bad, ref.ref, BF))


def test_sgp_front_channel_sums_of_unrounded_values_fail():
    shape = S.FRONT_SHAPES[2]
    B, T, C, ks, up = shape
    x, ln_w, ln_b, dw, db = front_case(shape, BF)
    y, _, chs = emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db, defects=("sums of un-rounded values",))
    print(f"[defect] channel sums of un-rounded values: the older expressions "
          f"{'LET IT PASS' if old_sums(chs, y.float(), (1,)) else 'catch it'}")
    with pytest.raises(AssertionError, match="not those of the stored"):
        R.assert_sums_consistent(chs, y, (1,), "chsum of un-rounded values")


# ----------------------------------------------------------------------------- mixer_front
def mixer_case(T_hi, T_lo, sdt, B=2, C=24, ks=5, up=13, offset=0.0):
    z = S.stream_input(81, f"z{T_hi}", (B, T_hi, C), sdt, offset)
    xlo = S.stream_input(82, f"x{T_lo}", (B, T_lo, C), sdt, offset)
    return z, xlo, S.ln_params(83, "l1", C), S.ln_params(84, "l2", C), S.branch_params(85, "d1", C, ks, up), \
        S.branch_params(86, "d2", C, ks, up)


def mixer_ref(z, xlo, ks, up, ln1, ln2, dwb1, dwb2, cat_dt, rz=None, rx=None):
    cat, parts = R.mixer_front_ref(z, xlo, ks, up, *ln1, *ln2, *dwb1, *dwb2, EPS, rz, rx)
    return R.as_stored(cat, cat_dt), parts


@pytest.mark.parametrize("sdt,cdt", [(F32, BF), (BF, BF), (F32, F32)])
@pytest.mark.parametrize("T_hi,T_lo", S.MIXER_T)
def test_faithful_mixer_front(T_hi, T_lo, sdt, cdt):
    ks, up = 5, 13
    for offset in (0.0, S.OFFSET_RATIO):
        z, xlo, ln1, ln2, d1, d2 = mixer_case(T_hi, T_lo, sdt, offset=offset)
        for rz, rx in ((None, None), (S.row_mean_rstd(z), S.split_parts(S.row_sums(xlo), 3))):
            ref, _ = mixer_ref(z, xlo, ks, up, ln1, ln2, d1, d2, cdt, rz, rx)
            cat = emu_mixer_front(z, xlo, cdt, ks, up, ln1, ln2, d1, d2, rz, rx)
            R.assert_within(cat, ref, f"mixer_front {T_hi} <- {T_lo} {sdt} -> {cdt} offset {offset}")


@pytest.mark.parametrize("defect", ["align_corners=False", "LN2 after the up-sampling", "out1 and out2 swapped", "truncating store"])
def test_mixer_front_defects_fail(defect):
    ks, up = 5, 13
    z, xlo, ln1, ln2, d1, d2 = mixer_case(25, 13, F32)
    ref, _ = mixer_ref(z, xlo, ks, up, ln1, ln2, d1, d2, BF)
    R.assert_within(emu_mixer_front(z, xlo, BF, ks, up, ln1, ln2, d1, d2), ref, "faithful")
    bad = emu_mixer_front(z, xlo, BF, ks, up, ln1, ln2, d1, d2, defects=(defect,))
    must_fail(defect, bad, ref, old_golden(bad, ref.ref, BF))


# ----------------------------------------------------------------------------- sgp_gemm
@pytest.mark.parametrize("adt", [BF, F32])
@pytest.mark.parametrize("B,T,K,N", [(2, 13, 48, 192), (1, 25, 368, 112), (1, 13, 1024, 64)])
def test_faithful_gn_fc1(B, T, K, N, adt):
    for offset in (0.0, S.OFFSET_RATIO):
        y, W, bias, gw, gb = S.gemm_operands(91, B, T, K, N, adt, offset)
        for parts in (1, 3, 7):
            chs = S.split_parts(S.channel_sums(y), parts)
            ref, st = R.gn_fc1_ref(y, chs, gw, gb, W, bias)
            assert R.first_order(st) >= 1.0 / 32
            R.assert_within(emu_gn_fc1(y, chs, gw, gb, W, bias), ref, f"MODE 0 {(B, T, K, N)} {adt} offset {offset} {parts} parts")


@pytest.mark.parametrize("defect", ["group boundaries off by one channel", "n of a full 16-row tile", "last k-chunk dropped",
                                    "neighbouring feature tile's bias", "truncating store"])
def test_gn_fc1_defects_fail(defect):
    B, T, K, N = 1, 25, 368, 112                              # 23 channels per group, a row tail, K % 128 != 0, N % 64 != 0
    y, W, bias, gw, gb = S.gemm_operands(91, B, T, K, N, BF)
    chs = S.split_parts(S.channel_sums(y), 1)
    ref, _ = R.gn_fc1_ref(y, chs, gw, gb, W, bias)
    R.assert_within(emu_gn_fc1(y, chs, gw, gb, W, bias), ref, "faithful")
    bad = emu_gn_fc1(y, chs, gw, gb, W, bias, defects=(defect,))
    must_fail(defect, bad, ref, old_r5(bad, ref.ref, BF))


def fc2_case(B, T, C, odt):
    H = S.rnd(101, f"h{T}x{C}", (B, T, 4 * C), 0.7).to(BF)
    W = R.bf16_weights(S.rnd(102, f"w{C}", (C, 4 * C), (4 * C) ** -0.5))
    return H, W, S.signed(103, f"b{C}", C, 0.3, 1.0), S.stream_input(104, f"r{T}x{C}", (B, T, C), odt)


@pytest.mark.parametrize("odt", [BF, F32])
@pytest.mark.parametrize("B,T,C", [(2, 13, 48), (2, 34, 112)])
def test_faithful_fc2_and_its_defects(B, T, C, odt):
    H, W, bias, resid = fc2_case(B, T, C, odt)
    pool = T % 2 == 0
    ref = R.as_stored(R.fc2_ref(H, W, bias, resid), odt)
    out, rsp, pooled, rpp = emu_fc2(H, W, bias, resid, pool)
    R.assert_within(out, ref, f"MODE 1 {(B, T, C)} {odt}")
    R.assert_sums_consistent(rsp.sum(0), out.reshape(B * T, C), (1,), "rowstat_part")
    if odt == BF:
        R.assert_unbiased(out, ref, "MODE 1") if B * T * C >= 12000 else None
        bad = emu_fc2(H, W, bias, resid, pool, defects=("sums of un-rounded values",))
        print(f"[defect] row sums of un-rounded values: the older expressions "
              f"{'LET IT PASS' if old_sums(bad[1].sum(0), bad[0].float().reshape(B * T, C), (1,)) else 'catch it'}")
        with pytest.raises(AssertionError, match="not those of the stored"):
            R.assert_sums_consistent(bad[1].sum(0), bad[0].reshape(B * T, C), (1,), "row sums of un-rounded values")
    if pool:
        want = R.maxpool(R.exact(out), T // 2)
        assert torch.equal(R.f64(pooled), want.ref)
        R.assert_sums_consistent(rpp.sum(0), pooled.reshape(-1, C), (1,), "rowstat_pool_part")
        bad = emu_fc2(H, W, bias, resid, pool, defects=("pooled rows paired as (2i - 1, 2i)",))[2]
        print("[defect] pooled rows paired as (2i - 1, 2i): test_gpu_r5.py compares the pooled rows exactly and catches it")
        assert not torch.equal(R.f64(bad), want.ref)


@pytest.mark.parametrize("odt", [BF, F32])
@pytest.mark.parametrize("B,T,C", [(2, 13, 48), (2, 34, 112)])
def test_faithful_concat_fc_and_its_defects(B, T, C, odt):
    A = S.rnd(111, f"a{T}x{C}", (B, T, 6 * C), 0.8).to(BF)
    W = R.bf16_weights(S.rnd(112, f"w{C}", (C, 6 * C), (6 * C) ** -0.5))
    bias = S.signed(113, f"b{C}", C, 0.3, 1.0)
    ref = R.as_stored(R.cat_fc_ref(A, W, bias), odt)
    out, o16, chs = emu_cat_fc(A, W, bias, odt)
    R.assert_within(out, ref, f"MODE 2 {(B, T, C)} {odt}")
    assert torch.equal(o16, out.to(BF))
    R.assert_sums_consistent(chs.sum(0), out, (1,), "chs_out")
    if odt == BF:
        bad = emu_cat_fc(A, W, bias, odt, defects=("truncating store",))[0]
        must_fail("truncating store", bad, ref, old_r5(bad, ref.ref, BF))
        bad = emu_cat_fc(A, W, bias, odt, defects=("sums of un-rounded values",))
        print(f"[defect] channel sums of un-rounded values: the older expressions "
              f"{'LET IT PASS' if old_sums(bad[2].sum(0), bad[0].float(), (1,)) else 'catch it'}")
        with pytest.raises(AssertionError, match="not those of the stored"):
            R.assert_sums_consistent(bad[2].sum(0), bad[0], (1,), "channel sums of un-rounded values")


def test_truncating_store_fails_the_bias_check():
    shape = S.FRONT_SHAPES[5]
    B, T, C, ks, up = shape
    x, ln_w, ln_b, dw, db = front_case(shape, BF)
    ref, _ = front_ref(x, ks, up, ln_w, ln_b, dw, db)
    R.assert_unbiased(emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db)[0], ref, "faithful")
    with pytest.raises(AssertionError, match="mean signed error"):
        R.assert_unbiased(emu_sgp_front(x, ks, up, ln_w, ln_b, dw, db, defects=("truncating store",))[0], ref, "truncating")


# ----------------------------------------------------------------------------- the pieces
def test_gelu_of_sgp_gemm_is_inside_the_transcendental_term():
    """Abramowitz-Stegun erf with rcpf and exp2f one ulp off in either direction: the term 16 * 2^-24 (|x| + |f(x)|) covers it"""
    x = torch.cat([S.rnd(51, "x", (20000,), 3.0), torch.linspace(-9, 9, 20001), torch.tensor([0.0, 1e-6, -1e-6, 1e-20])])
    v = R.RB(x.double(), torch.zeros(x.numel(), dtype=torch.float64))
    worst = 0.0
    for rcp in (-2.0 ** -23, 0.0, 2.0 ** -23):
        for ex in (-2.0 ** -23, 0.0, 2.0 ** -23):
            worst = max(worst, R.assert_within(sg_gelu(x, rcp, ex), R.gelu(v), f"sg_gelu rcp {rcp:+.1e} exp2 {ex:+.1e}"))
    print(f"[roundoff] sg_gelu uses {worst:.3f} of the transcendental term")
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(sg_gelu(x.to(BF).float()), R.gelu(v), "bf16-grade argument")


def test_upsampling_and_maxpool_rules():
    x = S.rnd(61, "x", (2, 13, 24))
    for T_hi in (25, 26, 13, 100):
        want = torch.nn.functional.interpolate(x.double().transpose(1, 2), size=T_hi, mode="linear", align_corners=True)
        ref = R.upsample_linear(R.exact(x), T_hi)
        assert float((ref.ref - want.transpose(1, 2)).abs().max()) < 1e-12
        R.assert_within(emu_upsample(x, T_hi), ref, f"up-sampling 13 -> {T_hi}")
    for T_out in (7, 13, 6):
        want = torch.nn.functional.adaptive_max_pool1d(x.double().transpose(1, 2), T_out).transpose(1, 2)
        got = R.maxpool(R.exact(x), T_out)
        assert torch.equal(got.ref, want) and float(got.d.max()) == 0.0


def test_first_order_rule_states_its_limit():
    """a row with var << E[x^2]: outside the regime the tests keep (var >= E[x^2] / 32), and `first_order` says so"""
    x = S.stream_input(62, "x", (1, 4, 48), F32, offset=64.0)
    assert R.first_order(R.layernorm_stats(R.exact(x), EPS)) < 1.0 / 32
    x = S.stream_input(62, "x", (1, 4, 48), F32, offset=S.OFFSET_RATIO)
    assert R.first_order(R.layernorm_stats(R.exact(x), EPS)) >= 1.0 / 32
