"""The SGP stage's kernels (sgp_fused.hip on sgp_tile.h, the three modes of sgp_gemm.hip, sgp.hip) against fp64 references of
the operands as each launch receives them, element by element, within the first-order rounding bound of tests/roundoff.py:
zero violations, every output in a guarded NaN-filled buffer, both stream types, every tile form, statistics computed in the
kernel and handed in.  The statistics a launch hands on are checked against the fp64 sums of the tensor that launch itself
stored.  Operands of tests/sgp_cases.py: every branch visible, normalisation in the first-order regime, one offset case
(|mean| / std = sgp_cases.OFFSET_RATIO) per normalising launch.  tests/test_roundoff_sgp_host.py proves the bound and shows
what falls outside it.  The assertions of test_gpu_r5.py stay.  -m gpu only, `pytest -s` prints every figure."""
from collections import OrderedDict

import pytest
import torch

import roundoff as R
import sgp_cases as S
from helpers import Guarded
from test_gpu_r5 import FORMS

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-5
STREAMS = [BF, F32]


@pytest.fixture(scope="module")
def ops():
    from tdeed_amd import ops as o, _lib
    _lib.load()
    return o


def dev(x):
    return None if x is None else x.to(DEV)


def pack(W):
    from tdeed_amd.engine import pack_mfma_frags
    return pack_mfma_frags(W.numpy(), DEV, ks_mult=12)


def enough_for_bias(ref):
    return int((ref.ref.abs() > 2.0 ** -10 * ref.ref.abs().max()).sum()) >= 10000


def check_stored(out, ref, dt, name, bias=True):
    """`out` against the fp32 value `ref` stored as dt; the bias check where dt is bf16 and the case supplies the elements"""
    want = R.as_stored(ref, dt)
    R.assert_within(out, want, name)
    if bias and dt == BF and enough_for_bias(want):
        R.assert_unbiased(out, want, name)


# ----------------------------------------------------------------------------- sgp_front
def front_case(shape, dt, offset=0.0):
    B, T, C, ks, up = shape
    return (S.stream_input(71, f"x{shape}", (B, T, C), dt, offset), *S.ln_params(72, f"ln{C}", C),
            *S.branch_params(73, f"dw{C}", C, ks, up))


def stat_forms(x):
    sums = S.row_sums(x)
    return [("in-kernel", None), ("mean rstd", S.row_mean_rstd(x)), ("1 part", S.split_parts(sums, 1)),
            ("3 parts", S.split_parts(sums, 3))]


@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("shape", S.FRONT_SHAPES)
def test_sgp_front(ops, shape, dt):
    """Rounding points of sgp_front_kernel, as read there: none in front of the store (LN(x) stays fp32 in the LDS tile in
    both stream types), the store of y, the bf16 copy y16 (of the same fp32 value); chsum sums the values rounded like the
    store."""
    B, T, C, ks, up = shape
    for offset in (0.0, S.OFFSET_RATIO):
        x, ln_w, ln_b, dw, db = front_case(shape, dt, offset)
        for how, rst in stat_forms(x)[::1 if not offset else 3]:
            name = f"sgp_front {shape} {dt} offset {offset} {how}"
            ref, parts = R.sgp_front_ref(x, ks, up, ln_w, ln_b, dw, db, EPS, rst)
            if not offset:
                S.check_front_conditions(x.float(), parts, name)
            gy, gc = Guarded((B, T, C), dt), Guarded((B, C, 2), F32)
            g16 = Guarded((B, T, C), BF) if dt == F32 else None
            ops.sgp_front(dev(x), ks, up, dev(ln_w), dev(ln_b), dev(dw), dev(db), EPS, out=gy.view, chsum=gc.view,
                          rowstat=dev(rst), out16=None if g16 is None else g16.view)
            y, chs = gy.check(name), gc.check(name + " chsum")
            check_stored(y, ref, dt, name)
            R.assert_sums_consistent(chs, y, (1,), name + " chsum")
            if g16 is not None:
                assert torch.equal(g16.check(name + " y16"), y.to(BF)), name + ": y16 is not the bf16 rounding of y"


# ----------------------------------------------------------------------------- mixer_front
def mixer_case(T_hi, T_lo, sdt, B, C, ks, up, offset=0.0):
    return (S.stream_input(81, f"z{T_hi}", (B, T_hi, C), sdt, offset), S.stream_input(82, f"x{T_lo}", (B, T_lo, C), sdt, offset),
            S.ln_params(83, "l1", C), S.ln_params(84, "l2", C), S.branch_params(85, "d1", C, ks, up),
            S.branch_params(86, "d2", C, ks, up))


@pytest.mark.parametrize("sdt,cdt", [(F32, BF), (BF, BF), (F32, F32)])
@pytest.mark.parametrize("T_hi,T_lo", S.MIXER_T)
def test_mixer_front(ops, T_hi, T_lo, sdt, cdt):
    """Rounding points of mixer_front_kernel: zn = LN1(z) and xn = LN2(x_lo) rounded to the stream's type in the LDS tile,
    xu = up(xn) rounded to it again, then the store of the six slabs.  Under the fp32 stream with the bf16 concat (the timed
    instantiation) every slab is ONE bf16 rounding of an fp32 value."""
    B = 2
    C, ks, up = (40, 7, 33) if T_hi >= 25 else (24, 5, 13)             # the unrolled run loop / the generic tap loop
    for offset in (0.0, S.OFFSET_RATIO):
        z, xlo, ln1, ln2, d1, d2 = mixer_case(T_hi, T_lo, sdt, B, C, ks, up, offset)
        for how, rz, rx in (("in-kernel", None, None), ("handed", S.row_mean_rstd(z), S.split_parts(S.row_sums(xlo), 3))):
            name = f"mixer_front {T_hi} <- {T_lo} {sdt} -> {cdt} offset {offset} {how}"
            ref, parts = R.mixer_front_ref(z, xlo, ks, up, *ln1, *ln2, *d1, *d2, EPS, rz, rx)
            if how == "in-kernel":
                assert min(R.first_order(s_) for s_ in parts["stats"]) >= 1.0 / 32
            g = Guarded((B, T_hi, 6 * C), cdt)
            ops.mixer_front(dev(z), dev(xlo), g.view, ks, up, *map(dev, ln1 + ln2), *map(dev, d1 + d2), EPS,
                            rowstat_z=dev(rz), rowstat_x=dev(rx))
            check_stored(g.check(name), ref, cdt, name, bias=(sdt == F32))


# ----------------------------------------------------------------------------- sgp_gemm
def forms_for(adt=None):
    return [f for f in FORMS if not (adt == F32 and f == (4, 2))]      # the launcher refuses (4, 2) on fp32 rows


@pytest.mark.parametrize("adt", STREAMS)
@pytest.mark.parametrize("B,T,K,N", [(b, t_, c, 4 * c) for b, t_, c in S.GEMM_SHAPES] + [(1, 13, 1024, 64)])
def test_gn_fc1_gelu(ops, B, T, K, N, adt):
    """MODE 0.  Rounding points: the normalised operand fmaf(x, rstd w, fmaf(-mean, rstd w, b)) -> bf16 (the MFMA's B operand),
    the bf16 store of H behind the GELU.  No bias check: H is a rounding of an fp32 value, but the reference differs from that
    value by the operand's roundings, which are not its own."""
    y, W, bias, gw, gb = S.gemm_operands(91, B, T, K, N, adt)
    Wp = pack(W)
    full = S.channel_sums(y)
    refs = {}
    for parts in (1, 3, 7):
        chs = S.split_parts(full, parts)
        refs[parts], st = R.gn_fc1_ref(y, chs, gw, gb, W, bias)
        assert R.first_order(st) >= 1.0 / 32
        for form in (forms_for(adt) if parts == 1 else [None]):
            name = f"MODE 0 {(B, T, K, N)} {adt} form {form} {parts} parts"
            g = Guarded((B, T, N))
            ops.sgp_gemm_gn_gelu(dev(y), dev(chs), dev(gw), dev(gb), Wp, dev(bias), N, out=g.view, form=form)
            R.assert_within(g.check(name), refs[parts], name)
    y = S.stream_input(91, f"y{B}x{T}x{K}", (B, T, K), adt, S.OFFSET_RATIO)
    chs = S.split_parts(S.channel_sums(y), 3)
    ref, st = R.gn_fc1_ref(y, chs, gw, gb, W, bias)
    assert R.first_order(st) >= 1.0 / 32
    g = Guarded((B, T, N))
    ops.sgp_gemm_gn_gelu(dev(y), dev(chs), dev(gw), dev(gb), Wp, dev(bias), N, out=g.view)
    R.assert_within(g.check("MODE 0 offset"), ref, f"MODE 0 {(B, T, K, N)} {adt} offset {S.OFFSET_RATIO}")


def check_fc2(ops, H, Wp, bias, resid, ref, form, name, rowstat_of=None):
    """one MODE 1 launch into guarded buffers -> (out, rowstat_part, pooled, rowstat_pool_part), everything checked"""
    B, T, K = H.shape
    N, odt = resid.shape[-1], resid.dtype
    f = form or ops.sgp_gemm_form(1, B, T, N, K)
    nct = ops.sgp_gemm_tiles(T, N, f)[1]
    pool = T % 2 == 0
    go, gr = Guarded((B, T, N), odt), Guarded((nct, B * T, 2), F32)
    gp = Guarded((B, T // 2, N), odt) if pool else None
    gq = Guarded((nct, B * (T // 2), 2), F32) if pool else None
    ops.sgp_gemm_residual(dev(H), Wp, dev(bias), dev(resid), out=go.view, rowstat_part=gr.view,
                          pooled=gp.view if pool else None, rowstat_pool_part=gq.view if pool else None, form=f)
    out, rsp = go.check(name), gr.check(name + " rowstat_part")
    check_stored(out, ref, odt, name)
    R.assert_sums_consistent(rsp.sum(0), out.reshape(B * T, N), (1,), name + " rowstat_part")
    if not pool:
        return out, rsp, None, None
    pooled, rpp = gp.check(name + " pooled"), gq.check(name + " rowstat_pool_part")
    assert torch.equal(R.f64(pooled), R.maxpool(R.exact(out), T // 2).ref), name + ": pooled rows are not the maxima of the stored rows"
    R.assert_sums_consistent(rpp.sum(0), pooled.reshape(-1, N), (1,), name + " rowstat_pool_part")
    return out, rsp, pooled, rpp


@pytest.mark.parametrize("odt", STREAMS)
@pytest.mark.parametrize("B,T,C", S.GEMM_SHAPES)
def test_fc2_residual_rowsums_pool(ops, B, T, C, odt):
    """MODE 1.  One rounding point: the store of resid + H W^T + b (fp32 in front of it); the row sums and the pooled rows
    are taken from the values rounded like the store; T = 34 pools to 17 inside the launch."""
    H = S.rnd(101, f"h{T}x{C}", (B, T, 4 * C), 0.7).to(BF)
    W = R.bf16_weights(S.rnd(102, f"w{C}", (C, 4 * C), (4 * C) ** -0.5))
    bias, resid = S.signed(103, f"b{C}", C, 0.3, 1.0), S.stream_input(104, f"r{T}x{C}", (B, T, C), odt)
    Wp, ref = pack(W), R.fc2_ref(H, W, bias, resid)
    for form in FORMS:
        check_fc2(ops, H, Wp, bias, resid, ref, form, f"MODE 1 {(B, T, C)} {odt} form {form}")


def check_cat_fc(ops, A, Wp, bias, N, odt, ref, form, name, with16=True):
    B, T, K = A.shape
    f = form or ops.sgp_gemm_form(2, B, T, N, K)
    NJ = ops.sgp_gemm_tiles(T, N, f)[0]
    go, gc = Guarded((B, T, N), odt), Guarded((NJ, B, N, 2), F32)
    g16 = Guarded((B, T, N), BF) if with16 else None
    ops.sgp_gemm_gelu_chsum(dev(A), Wp, dev(bias), N, go.view, gc.view, form=f, out16=g16.view if with16 else None)
    out, chs = go.check(name), gc.check(name + " chs_out")
    check_stored(out, ref, odt, name)
    R.assert_sums_consistent(chs.sum(0), out, (1,), name + " chs_out")
    if with16:
        assert torch.equal(g16.check(name + " out16"), out.to(BF)), name + ": out16 is not the bf16 rounding of out"
    return out, chs


@pytest.mark.parametrize("odt", STREAMS)
@pytest.mark.parametrize("B,T,C", S.GEMM_SHAPES)
def test_concat_fc_gelu_channel_sums(ops, B, T, C, odt):
    """MODE 2.  One rounding point: the store of GELU(cat Wc^T + b); out16 is the bf16 rounding of the stored value; the
    channel sums are those of the stored rows."""
    A = S.rnd(111, f"a{T}x{C}", (B, T, 6 * C), 0.8).to(BF)
    W = R.bf16_weights(S.rnd(112, f"w{C}", (C, 6 * C), (6 * C) ** -0.5))
    bias = S.signed(113, f"b{C}", C, 0.3, 1.0)
    Wp, ref = pack(W), R.cat_fc_ref(A, W, bias)
    for form in FORMS:
        check_cat_fc(ops, A, Wp, bias, C, odt, ref, form, f"MODE 2 {(B, T, C)} {odt} form {form}")


# ----------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("C", [48, 768])
@pytest.mark.parametrize("T_in,T_out", [(25, 13), (13, 7), (125, 63)])
def test_maxpool_rowstat(ops, T_in, T_out, C, dt):
    """pooled rows are the maxima of the inputs exactly; (mean, rstd) are those of the pooled rows the kernel stored"""
    B = 2
    for offset in (0.0, S.OFFSET_RATIO):
        if offset:      # pooled rows with the offset's |mean| / std: the input is built from them (sgp_cases.pool_preimage)
            P = S.stream_input(122, f"p{T_out}x{C}", (B, T_out, C), dt, offset)
            x = S.pool_preimage(P, T_in, 123)
            assert torch.equal(R.maxpool(R.exact(x), T_out).ref, R.f64(P))
        else:
            x = S.stream_input(121, f"x{T_in}x{C}", (B, T_in, C), dt)
        name = f"maxpool_rowstat {T_in} -> {T_out} C {C} {dt} offset {offset}"
        want = R.maxpool(R.exact(x), T_out)
        go, gs = Guarded((B, T_out, C), dt), Guarded((B * T_out, 2), F32)
        ops.maxpool_rowstat(dev(x), T_out, out=go.view, rowstat=gs.view, eps=EPS)
        out, rs = go.check(name), gs.check(name + " rowstat")
        assert torch.equal(R.f64(out), want.ref), name
        st = R.layernorm_stats(R.exact(out.reshape(B * T_out, C)), EPS)
        assert R.first_order(st) >= 1.0 / 32
        R.assert_within(rs[:, 0], R.RB(st.m, st.d_m), name + " mean")
        R.assert_within(rs[:, 1], R.RB(st.rstd, st.d_rstd), name + " rstd")
        g2 = Guarded((B, T_out, C), dt)
        ops.maxpool(dev(x), T_out, out=g2.view)
        assert torch.equal(R.f64(g2.check(name + " maxpool")), want.ref), name + " (maxpool)"


# ----------------------------------------------------------------------------- the launch-per-op kernels
@pytest.mark.parametrize("dt", STREAMS)
@pytest.mark.parametrize("shape", S.FRONT_SHAPES[:3])
def test_launch_per_op_kernels(ops, shape, dt):
    """layernorm, sgp_branch, mixer_branch and groupnorm (the fp32 engine and the TDEED_SGP_FUSED=0 chain) share the
    references: each launch against its own operands, its output rounded once to the tensor's type.  layernorm and groupnorm
    compute their variance in two passes, which stays inside the one-pass bound."""
    B, T, C, ks, up = shape
    x, ln_w, ln_b, dw, db = front_case(shape, dt)
    name = f"{shape} {dt}"
    ln_ref, _ = R.layernorm(R.exact(x), ln_w, ln_b, EPS)
    g = Guarded((B, T, C), dt)
    ops.layernorm(dev(x), dev(ln_w), dev(ln_b), EPS, out=g.view)
    o = g.check("layernorm " + name).clone()
    check_stored(o, ln_ref, dt, "layernorm " + name)
    oe = R.exact(o)                                                    # sgp_branch receives the stored LayerNorm output
    gate, inst, _ = R.branches(oe, dw, db, ks, up)
    g = Guarded((B, T, C), dt)
    ops.sgp_branch(o, dev(x), ks, up, dev(dw), dev(db), out=g.view)
    check_stored(g.check("sgp_branch " + name), R.total(R.exact(x), oe, inst, gate), dt, "sgp_branch " + name)
    G = 16 if C % 16 == 0 else 8                                       # (C = 24, 40: 3 and 5 channels per group)
    gw, gb = (1.0 + S.rnd(131, f"gw{C}", (C,), 0.2)).float(), S.signed(132, f"gb{C}", C, 0.1, 0.5)
    gn_ref, st = R.groupnorm(R.exact(x), G, gw, gb, EPS)
    assert R.first_order(st) >= 1.0 / 32
    g = Guarded((B, T, C), dt)
    ops.groupnorm(dev(x), G, dev(gw), dev(gb), EPS, out=g.view)
    check_stored(g.check("groupnorm " + name), gn_ref, dt, "groupnorm " + name)
    # mixer_branch: zn already in slab 4 of cat, xn at T_lo; it writes slabs 0 .. 3 and 5
    T_lo = (T + 1) // 2
    xn = S.stream_input(133, f"xn{T_lo}x{C}", (B, T_lo, C), dt)
    dw2, db2 = S.branch_params(134, f"dw2{C}", C, ks, up)
    g = Guarded((B, T, 6 * C), dt)
    g.view[..., 4 * C:5 * C] = o
    ops.mixer_branch(dev(xn), g.view, T, ks, up, dev(dw), dev(db), dev(dw2), dev(db2))
    cat = g.check("mixer_branch " + name)
    xu = R.as_stream(R.upsample_linear(R.exact(xn), T), dt)
    g1, i1, _ = R.branches(oe, dw, db, ks, up)
    g2_, i2, _ = R.branches(xu, dw2, db2, ks, up)
    slabs = [g1, g2_, i1, i2, oe, xu]
    ref = R.RB(torch.cat([s_.ref for s_ in slabs], -1), torch.cat([s_.d for s_ in slabs], -1))
    keep = [i for i in range(6 * C) if not 4 * C <= i < 5 * C]
    check_stored(cat[..., keep], R.RB(ref.ref[..., keep], ref.d[..., keep]), dt, "mixer_branch " + name)
    assert torch.equal(cat[..., 4 * C:5 * C], o)


# ----------------------------------------------------------------------------- a block and a mixer, launch by launch
def stage_state(C, ks, up):
    """an SGPBlock "blk" and an SGPMixer "mix" in the reference's state-dict layout, with the operands of sgp_cases; the
    dense weights are rounded to bf16 first, so the packed fragments hold the reference's values"""
    sd = OrderedDict()

    def branch(pre, tag, seed, sfx=""):
        dw, db = S.branch_params(seed, tag, C, ks, up)
        p = R.dw_split(dw, db, ks, up)
        for key, nm in (("psi", "psi"), ("cw", "convw"), ("ckw", "convkw"), ("fc", "fc"), ("g", "global_fc")):
            sd[f"{pre}.{nm}{sfx}.weight"] = p[key][0].reshape(C, 1, -1).numpy()
            sd[f"{pre}.{nm}{sfx}.bias"] = p[key][1].numpy()
        return dw, db

    def mlp(pre, seed):
        sd[pre + ".gn.weight"] = (1.0 + S.rnd(seed, "gw", (C,), 0.2)).numpy()
        sd[pre + ".gn.bias"] = S.signed(seed, "gb", C, 0.1, 0.5).numpy()
        sd[pre + ".mlp.0.weight"] = R.bf16_weights(S.rnd(seed, "w1", (4 * C, C), C ** -0.5)).reshape(4 * C, C, 1).numpy()
        sd[pre + ".mlp.0.bias"] = S.signed(seed, "b1", 4 * C, 0.3, 1.0).numpy()
        sd[pre + ".mlp.2.weight"] = R.bf16_weights(S.rnd(seed, "w2", (C, 4 * C), (4 * C) ** -0.5)).reshape(C, 4 * C, 1).numpy()
        sd[pre + ".mlp.2.bias"] = S.signed(seed, "b2", C, 0.3, 1.0).numpy()

    par = {}
    for pre, n, seed in (("blk", "ln", 141), ("mix", "ln1", 142), ("mix", "ln2", 143)):
        w, b = S.ln_params(seed, n, C)
        sd[f"{pre}.{n}.weight"], sd[f"{pre}.{n}.bias"] = w.reshape(1, C, 1).numpy(), b.reshape(1, C, 1).numpy()
        par[n] = (w, b)
    par["blk"] = branch("blk", "bd", 144)
    par["mix1"], par["mix2"] = branch("mix", "m1", 145, "1"), branch("mix", "m2", 146, "2")
    mlp("blk", 147)
    mlp("mix", 148)
    sd["mix.concat_fc.weight"] = R.bf16_weights(S.rnd(149, "wc", (C, 6 * C), (6 * C) ** -0.5)).reshape(C, 6 * C, 1).numpy()
    sd["mix.concat_fc.bias"] = S.signed(149, "bc", C, 0.3, 1.0).numpy()
    return sd, par


def run_and_snapshot(steps):
    """run the plan launch by launch; after each launch, copies of every tensor its closure names (buffers are recycled)"""
    snaps = OrderedDict()
    for s_ in steps:
        s_.fn()
        torch.cuda.synchronize()
        cells = dict(zip(s_.fn.__code__.co_freevars, (c.cell_contents for c in s_.fn.__closure__)))
        snaps[s_.name] = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in cells.items()}
    return snaps


@pytest.mark.parametrize("stream", STREAMS)
def test_block_then_mixer_launch_by_launch(stream):
    """A block whose fc2 launch pools (26 -> 13), then the mixer that takes the block's output as z and the pooled rows as
    x_lo, built through SgpBuilder.  The reference of each launch takes the previous launch's ACTUAL output (and the
    statistics handed with it) as its operands: bounds do not compound, and each handed statistic is checked against the
    tensor its producer stored."""
    from tdeed_amd.engine import SgpBuilder, pack_sgp_block, pack_sgp_mixer, _Pool
    B, T, C, ks, up = 2, 26, 48, 7, 33
    sd, par = stage_state(C, ks, up)
    blk, mix = pack_sgp_block(sd, "blk", C, BF, DEV), pack_sgp_mixer(sd, "mix", C, BF, DEV)
    x = S.stream_input(150, "x", (B, T, C), stream)
    steps, keep = [], {}
    sb = SgpBuilder(_Pool(DEV), steps, keep, set(), B, BF)
    z = sb.block(x.to(DEV), T, blk, "blk", pool_to=T // 2)
    assert sb.last_pooled is not None
    out = sb.mixer(sb.last_pooled, T // 2, z, T, mix, "mix")
    assert [s_.name for s_ in steps] == ["blk.front", "blk.fc1", "blk.fc2", "mix.front", "mix.cat", "mix.fc1", "mix.fc2"]
    assert out.dtype == stream
    sn = run_and_snapshot(steps)
    w = lambda k: t_(sd[k]).reshape(sd[k].shape[0], -1)                            # noqa: E731
    t_ = torch.from_numpy
    tag = f"chain {stream} "
    # blk.front
    s0 = sn["blk.front"]
    ref, parts = R.sgp_front_ref(s0["xin"], ks, up, *par["ln"], *par["blk"], EPS, s0["rs_in"])
    S.check_front_conditions(s0["xin"].float(), parts, tag + "blk.front")
    check_stored(s0["y"], ref, stream, tag + "blk.front")
    R.assert_sums_consistent(s0["chs"], s0["y"], (1,), tag + "blk.front chsum")
    # blk.fc1: the rows and the channel sums the front launch left
    s1 = sn["blk.fc1"]
    assert torch.equal(s1["ya"], s0["y"]) and torch.equal(s1["chsum"], s0["chs"])
    ref, st = R.gn_fc1_ref(s1["ya"], s1["chsum"], t_(sd["blk.gn.weight"]), t_(sd["blk.gn.bias"]), w("blk.mlp.0.weight"),
                           t_(sd["blk.mlp.0.bias"]))
    assert R.first_order(st) >= 1.0 / 32
    R.assert_within(s1["H"], ref, tag + "blk.fc1")
    # blk.fc2 with the pool
    s2 = sn["blk.fc2"]
    assert torch.equal(s2["H"], s1["H"]) and torch.equal(s2["y"], s0["y"])
    check_stored(s2["outb"], R.fc2_ref(s2["H"], w("blk.mlp.2.weight"), t_(sd["blk.mlp.2.bias"]), s2["y"]), stream, tag + "blk.fc2")
    R.assert_sums_consistent(s2["rsp"].sum(0), s2["outb"].reshape(B * T, C), (1,), tag + "blk.fc2 rowstat_part")
    assert torch.equal(R.f64(s2["pooled"]), R.maxpool(R.exact(s2["outb"]), T // 2).ref)
    R.assert_sums_consistent(s2["rpp"].sum(0), s2["pooled"].reshape(-1, C), (1,), tag + "blk.fc2 rowstat_pool_part")
    # mix.front: z, x_lo and both sets of partial row sums as the block left them
    s3 = sn["mix.front"]
    assert torch.equal(s3["z"], s2["outb"]) and torch.equal(s3["xlo"], s2["pooled"])
    assert torch.equal(s3["rs_z"], s2["rsp"]) and torch.equal(s3["rs_x"], s2["rpp"])
    ref, mp = R.mixer_front_ref(s3["z"], s3["xlo"], ks, up, *par["ln1"], *par["ln2"], *par["mix1"], *par["mix2"], EPS,
                                s3["rs_z"], s3["rs_x"])
    assert min(R.first_order(s_) for s_ in mp["stats"]) >= 1.0 / 32
    check_stored(s3["cat"], ref, BF, tag + "mix.front", bias=(stream == F32))
    # mix.cat
    s4 = sn["mix.cat"]
    assert torch.equal(s4["cat"], s3["cat"])
    check_stored(s4["mo"], R.cat_fc_ref(s4["cat"], w("mix.concat_fc.weight"), t_(sd["mix.concat_fc.bias"])), stream, tag + "mix.cat")
    R.assert_sums_consistent(s4["chs"].sum(0), s4["mo"], (1,), tag + "mix.cat chs_out")
    # mix.fc1 / mix.fc2
    s5, s6 = sn["mix.fc1"], sn["mix.fc2"]
    assert torch.equal(s5["ya"], s4["mo"]) and torch.equal(s5["chsum"], s4["chs"])
    ref, st = R.gn_fc1_ref(s5["ya"], s5["chsum"], t_(sd["mix.gn.weight"]), t_(sd["mix.gn.bias"]), w("mix.mlp.0.weight"),
                           t_(sd["mix.mlp.0.bias"]))
    assert R.first_order(st) >= 1.0 / 32
    R.assert_within(s5["H"], ref, tag + "mix.fc1")
    check_stored(s6["outb"], R.fc2_ref(s6["H"], w("mix.mlp.2.weight"), t_(sd["mix.mlp.2.bias"]), s6["y"]), stream, tag + "mix.fc2")
    R.assert_sums_consistent(s6["rsp"].sum(0), s6["outb"].reshape(B * T, C), (1,), tag + "mix.fc2 rowstat_part")
    assert torch.equal(out.cpu(), s6["outb"])
