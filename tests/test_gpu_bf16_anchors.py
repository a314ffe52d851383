"""The bf16 anchor kernels (the base kernels under the bit-identity tower of the fused launches) against fp64 references,
element by element, within the first-order rounding bound of tests/roundoff.py: fp32 accumulation and ONE round-to-nearest-even
bf16 rounding at each rounding point the kernel's header names; zero violations.  Where the output is a single rounding of an
fp32 value (the gemm family, the grouped conv, the stem) the store must also be unbiased (a truncating store is -0.5 ulp).
The older anchors of test_gpu_ops.py (`max|out - ref| / max|ref| < 3e-2`) stay; tests/test_roundoff_host.py shows on the CPU what
they let through.  Every output is written into a guarded buffer.  -m gpu only, bf16 only, `pytest -s` prints every figure."""
import numpy as np
import pytest
import torch

import roundoff as R
from helpers import Guarded, act, t
from tdeed_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from tdeed_amd import ops as o, _lib
    _lib.load()
    return o


def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


def enough_for_bias(ref):
    """the bias check needs 10 000 elements above 2^-10 max|ref| (a property of the case, decided on the reference)"""
    r = ref.ref if isinstance(ref, R.RB) else ref
    return int((r.abs() > 2.0 ** -10 * r.abs().max()).sum()) >= 10000


def dev(x):
    return None if x is None else x.to(DEV)


# ----------------------------------------------------------------------------- the gemm family
def gemm_operands(seed, M, K, N):
    """bf16 activations; weights rounded to bf16 BEFORE packing, so the dense bf16 copy (gemm, gemm_splitk) and the bf16
    fragments of pack_ws_weights hold exactly the reference's values; folds with scales of both signs and shifts of order 1"""
    A = rnd(seed, f"A{M}x{K}", (M, K)).to(BF)
    W = R.bf16_weights(rnd(seed + 1, f"W{N}x{K}", (N, K), 1.0 / np.sqrt(K)))
    sc, sh = R.fold(seed + 2, f"f{N}", N)
    res = rnd(seed + 3, f"R{M}x{N}", (M, N)).to(BF)
    return A, W, sc, sh, res


def check_epilogue_forms(run, A, W, sc, sh, res, name, bias=True):
    """run(scale, shift, act, residual, out) launches the op on the operand pair.  Plain with scale and shift; residual with
    ReLU; residual with GELU; no scale."""
    M, N = A.shape[0], W.shape[0]
    c = R.contraction(R.exact(A), W)
    forms = [("plain", sc, sh, 0, None), ("residual relu", sc, sh, 1, res), ("residual gelu", sc, sh, 2, res),
             ("no scale", None, sh, 0, None)]
    checked_bias = False
    for form, s_, h_, actn, r_ in forms:
        ref = R.store_bf16(R.activation(R.affine(c, s_, h_, None if r_ is None else R.exact(r_)), actn))
        g = Guarded((M, N))
        run(dev(s_), dev(h_), actn, dev(r_), g.view)
        out = g.check(f"{name} {form}")
        R.assert_within(out, ref, f"{name} {form}")
        if actn == 1:
            frac = R.relu_open(ref.ref)
            assert 0.2 < frac < 0.8, frac
        if bias and actn != 1 and enough_for_bias(ref):
            R.assert_unbiased(out, ref, f"{name} {form}")
            checked_bias = True
    return checked_bias


def check_operand_forms(run, seed, K, N, W, sc, sh, name, Fr, hw, k0, hi, wi):
    """the SE operand scale (rounded to bf16: scaled_operand_bf16), the gate-shift splice and the stride-2 row gather, each
    with scale and shift.  run(A, out, **operand keywords)."""
    M = Fr * hw
    A = rnd(seed + 10, f"A{M}", (M, K)).to(BF)
    gate = torch.sigmoid(rnd(seed + 11, "g", (Fr, K)))
    assert not torch.equal(gate[0], gate[1])
    ref = R.store_bf16(R.linear(R.scaled_operand_bf16(A, gate, hw), W, sc, sh))
    g = Guarded((M, N))
    run(A.to(DEV), g.view, a_scale=gate.to(DEV), a_scale_rows=hw)
    R.assert_within(g.check(f"{name} a_scale"), ref, f"{name} a_scale")
    A0 = rnd(seed + 12, "A0", (M, k0)).to(BF)
    ref = R.store_bf16(R.linear(R.exact(torch.cat([A0, A[:, k0:]], dim=1)), W, sc, sh))
    g = Guarded((M, N))
    run(A.to(DEV), g.view, A0=A0.to(DEV), k0=k0)
    R.assert_within(g.check(f"{name} splice"), ref, f"{name} splice")
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    X = rnd(seed + 13, "X", (3, hi, wi, K)).to(BF)
    ref = R.store_bf16(R.linear(R.exact(X[:, ::2, ::2, :].reshape(-1, K)), W, sc, sh))
    g = Guarded((3 * ho * wo, N))
    run(X.to(DEV), g.view, gather=(2, hi, wi, ho, wo))
    R.assert_within(g.check(f"{name} gather"), ref, f"{name} gather")


# (257,24,56): row tail, K < 32, N % 16 = 8; (75,2208,368): deep K
@pytest.mark.parametrize("M,K,N", [(257, 24, 56), (300, 32, 24), (129, 152, 368), (75, 2208, 368)])
def test_gemm_tiled(ops, M, K, N):
    A, W, sc, sh, res = gemm_operands(300, M, K, N)
    Ad, Wd = A.to(DEV), W.to(BF).to(DEV)
    assert torch.equal(Wd.float().cpu(), W)                       # the dense copy is exact
    checked = check_epilogue_forms(lambda s_, h_, a_, r_, out: ops.gemm(Ad, Wd, s_, h_, a_, residual=r_, out=out),
                                   A, W, sc, sh, res, f"gemm {M}x{K}x{N}")
    assert checked == (M * N >= 12000)                            # the bias check ran wherever the shape supplies the elements


def test_gemm_tiled_operand_forms(ops):
    Fr, hw, K, N = 6, 49, 152, 368
    _, W, sc, sh, _ = gemm_operands(320, Fr * hw, K, N)
    Wd = W.to(BF).to(DEV)
    check_operand_forms(lambda A, out, **kw: ops.gemm(A, Wd, dev(sc), dev(sh), ops.ACT_NONE, out=out, **kw),
                        320, K, N, W, sc, sh, "gemm", Fr, hw, 48, 7, 9)


# (4097,152,152): the persistent loop; (300,152,368): a wide W streamed in slices (mode 2)
@pytest.mark.parametrize("M,K,N,mode", [(300, 32, 24, 1), (257, 24, 56, 1), (263, 56, 152, 1), (130, 128, 128, 1),
                                        (300, 152, 368, 2), (4097, 152, 152, 1)])
def test_gemm_ws(ops, M, K, N, mode):
    from tdeed_amd.packing import pack_ws_weights
    assert ops.gemm_ws_fits_mode(K, N, BF) == mode
    A, W, sc, sh, res = gemm_operands(340, M, K, N)
    Wf = pack_ws_weights(W.numpy(), BF, DEV)
    assert set(Wf.float().unique().tolist()) <= set(W.unique().tolist()) | {0.0}          # the fragments hold W's values
    Ad = A.to(DEV)
    name = f"gemm_ws {M}x{K}x{N}"
    checked = check_epilogue_forms(lambda s_, h_, a_, r_, out: ops.gemm_ws(Ad, Wf, K, N, s_, h_, a_, residual=r_, out=out),
                                   A, W, sc, sh, res, name)
    assert checked == (M * N >= 12000)
    rows = 7                                                       # (rows per frame of the existing anchor)
    check_operand_forms(lambda A_, out, **kw: ops.gemm_ws(A_, Wf, K, N, dev(sc), dev(sh), ops.ACT_NONE, out=out, **kw),
                        360, K, N, W, sc, sh, name, (M // rows), rows, 8, 6, 10)


@pytest.mark.parametrize("M,K,N", [(37, 40, 24), (200, 2208, 368), (400, 368, 1472)])
def test_gemm_splitk(ops, M, K, N):
    """fp32 partials in the workspace add no bf16 rounding: the contraction term covers any summation order"""
    A, W, sc, sh, res = gemm_operands(380, M, K, N)
    Ad, Wd = A.to(DEV), W.to(BF).to(DEV)
    c = R.contraction(R.exact(A), W)
    for actn in (0, 1, 2):
        for form, s_, h_, r_ in (("scale shift residual", sc, sh, res), ("bare", None, None, None)):
            ref = R.store_bf16(R.activation(R.affine(c, s_, h_, None if r_ is None else R.exact(r_)), actn))
            g = Guarded((M, N))
            ops.gemm_splitk(Ad, Wd, dev(s_), dev(h_), actn, residual=dev(r_), out=g.view)
            name = f"gemm_splitk {M}x{K}x{N} act {actn} {form}"
            out = g.check(name)
            R.assert_within(out, ref, name)
            if actn == 1:
                frac = R.relu_open(ref.ref)
                assert 0.2 < frac < 0.8, frac
            elif M * N >= 12000:
                R.assert_unbiased(out, ref, name)


# ----------------------------------------------------------------------------- grouped 3 x 3: VALU and MFMA
# (56,8,2,15,13): odd map, masked tail tile
@pytest.mark.parametrize("C,gw,stride,H,W", [(24, 8, 2, 20, 22), (56, 8, 1, 9, 7), (56, 8, 2, 15, 13), (64, 16, 2, 16, 16),
                                             (368, 8, 1, 7, 7), (152, 8, 2, 28, 28), (768, 16, 2, 14, 14)])
def test_gconv3x3(ops, C, gw, stride, H, W):
    from tdeed_amd.packing import pack_gconv_frags
    N, G = 3, C // gw
    x = rnd(400, f"x{C}", (N, C, H, W)).to(BF)
    # rounded to bf16 first: the MFMA fragments (pack_gconv_frags ends in a bf16 cast) and the VALU kernel's fp32 table then
    # hold the same values, those of the reference
    w = R.bf16_weights(rnd(401, f"w{C}", (C, gw, 3, 3), 1.0 / np.sqrt(9 * gw)))
    sc, sh = R.fold(402, f"g{C}", C)
    ref = R.permute(R.store_bf16(R.relu(R.conv2d(R.exact(x), w, stride, G, sc, sh))), 0, 2, 3, 1)       # NHWC
    frac = R.relu_open(ref.ref)
    assert 0.2 < frac < 0.8, frac
    wp = w.reshape(G, gw, gw, 3, 3).permute(0, 3, 4, 2, 1).reshape(G, 9, gw, gw).contiguous().to(DEV)
    wfrag = pack_gconv_frags(w, gw, DEV)
    assert set(wfrag.float().unique().tolist()) <= set(w.unique().tolist()) | {0.0}
    assert ops.gconv3x3_mfma_fits(H, W, C, stride)                 # (otherwise the launcher takes the VALU kernel for both)
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for kind, wf in (("VALU", None), ("MFMA", wfrag)):
        name = f"gconv3x3 {kind} C{C} gw{gw} s{stride} {H}x{W}"
        parts = ops.gconv3x3_parts(H, W, C, stride, BF) if wf is not None else 1
        g = Guarded((N, Ho, Wo, C))
        gp = Guarded((N, parts, C), torch.float32)
        ops.gconv3x3(xin, wp, sc.to(DEV), sh.to(DEV), gw, stride, wfrag=wf, out=g.view, pooled=gp.view)
        y, pooled = g.check(name), gp.check(name + " pooled")
        R.assert_within(y, ref, name, nhwc=True)
        # both kernels sum the ROUNDED outputs (conv.hip: psum += round_to<T>(v) / (float)o[r]): the squeeze sums are those of
        # the y the kernel itself wrote
        R.assert_pooled_consistent(pooled, y, name)
        if enough_for_bias(ref):
            R.assert_unbiased(y, ref, name)
        else:
            assert N * Ho * Wo * C < 50000                          # (a ReLU open on > 20 % leaves 10 000 of 50 000)


# ----------------------------------------------------------------------------- stem
STEM_GEOMS = [(2, 64, 64, None, False), (1, 72, 80, (4, 8, 64, 64), True), (1, 50, 37, None, False)]


def stem_operands(geom):
    N, H, W, crop, flip = geom
    fr = t(synth.uint8_clip(21, (N, 3, H, W)))
    w = rnd(420, "w", (32, 3, 3, 3), 0.3)
    sc, sh = R.fold(421, "stem", 32)
    return fr, w, sc, sh


@pytest.mark.parametrize("geom", STEM_GEOMS)
def test_stem(ops, geom):
    """VALU stem: fp32 weights, the normalisation in fp32 (roundoff.normalised_f32), one bf16 store behind the ReLU"""
    N, H, W, crop, flip = geom
    fr, w, sc, sh = stem_operands(geom)
    ref = R.permute(R.store_bf16(R.relu(R.conv2d(R.normalised_f32(fr, crop, flip), w, 2, 1, sc, sh))), 0, 2, 3, 1)
    frac = R.relu_open(ref.ref)
    assert 0.2 < frac < 0.8, frac
    g = Guarded(tuple(ref.ref.shape))
    ops.stem(fr.to(DEV), w.reshape(32, 27).contiguous().to(DEV), sc.to(DEV), sh.to(DEV), BF, crop, flip, out=g.view)
    name = f"stem {geom}"
    out = g.check(name)
    R.assert_within(out, ref, name, nhwc=True)
    assert enough_for_bias(ref) or ref.ref.numel() < 50000       # (a ReLU open on > 20 % leaves 10 000 of 50 000)
    if enough_for_bias(ref):
        R.assert_unbiased(out, ref, name)


@pytest.mark.parametrize("geom", STEM_GEOMS)
def test_stem_mfma(ops, geom):
    """Training stem on the MFMA pipe: the raw conv output.  The input is fmaf(u, na, nb) in fp32 (emulated exactly); input
    and weight are split into a bf16 head and a bf16 tail and the tail x tail product is dropped (front.hip): each split leaves
    2^-9 2^-9 = 2^-18 of its value, the dropped product 2^-18 of the term, together 3 2^-18 < 2^-16 per term, carried as the
    operand's error.  Then fp32 accumulation and one bf16 store."""
    from tdeed_amd.packing import stem_frags_on_device
    N, H, W, crop, flip = geom
    fr, w, _, _ = stem_operands(geom)
    ch, cw = (crop[2], crop[3]) if crop else (H, W)
    parts = ops.stem_mfma_parts(ch, cw)
    assert parts > 0                                               # every geometry of the stem anchor is served
    _, x32 = R.normalised_bf16(fr, crop, flip)
    x = R.RB(x32.double(), 2.0 ** -16 * x32.double().abs())
    ref = R.permute(R.store_bf16(R.conv2d(x, w, 2, 1)), 0, 2, 3, 1)
    z, colpart = ops.stem_mfma(fr.to(DEV), stem_frags_on_device(w.to(DEV)), crop, flip)
    torch.cuda.synchronize()
    name = f"stem_mfma {geom}"
    R.assert_within(z, ref, name, nhwc=True)
    assert enough_for_bias(ref)
    R.assert_unbiased(z, ref, name)
    R.assert_pooled_consistent(colpart.view(N, parts, 2, 32)[:, :, 0, :], z, name)      # column sums of what it stored


# ----------------------------------------------------------------------------- fused front: three stages, bf16 in between
FRONT_GEOMS = [(2, 64, 64, None, False, 24, 8), (1, 72, 80, (4, 8, 64, 64), True, 24, 8), (1, 96, 64, None, False, 64, 16),
               # pipelined strip kernel: aligned crop + flip, one-tile width (C1 = 16), ragged last strip, odd crop (rolling)
               (1, 96, 112, (16, 16, 64, 96), True, 24, 8), (2, 64, 64, None, True, 16, 8),
               (1, 240, 224, None, False, 24, 8), (1, 70, 90, (3, 5, 61, 77), True, 24, 8)]


@pytest.mark.parametrize("geom", FRONT_GEOMS)
def test_s1_front(ops, geom):
    """Rounding points of front.hip, as read there: the normalised input patch (fmaf in fp32, then bf16: emulated exactly),
    the stem output (bf16 B operand of conv1 and of the shortcut conv), y1 (the bf16 LDS band), y2 and the shortcut map (bf16
    stores); every weight is a bf16 fragment.  The squeeze sums are those of the rounded y2 (psum += (float)o[r] in all three
    forms of the kernel)."""
    from tdeed_amd.packing import pack_front_weights
    N, H, W, crop, flip, C1, gw = geom
    fr = t(synth.uint8_clip(81, (N, 3, H, W)))
    sw = R.bf16_weights(rnd(440, "sw", (32, 3, 3, 3), 0.3))
    w1 = R.bf16_weights(rnd(441, "w1", (C1, 32), 0.25))
    wd = R.bf16_weights(rnd(442, "wd", (C1, 32), 0.25))
    w2 = R.bf16_weights(rnd(443, "w2", (C1, gw, 3, 3), 1.0 / np.sqrt(9 * gw)))
    (ss, hs), (s1, h1), (sd_, hd), (s2, h2) = (R.fold(444, "fs", 32), R.fold(445, f"f1{C1}", C1), R.fold(446, f"fd{C1}", C1),
                                               R.fold(447, f"f2{C1}", C1))
    xb, _ = R.normalised_bf16(fr, crop, flip)
    st = R.store_bf16(R.relu(R.conv2d(R.exact(xb), sw, 2, 1, ss, hs)))                      # (N, 32, Hs, Ws)
    Hs, Ws = st.ref.shape[2:]
    st_rows = R.reshape(R.permute(st, 0, 2, 3, 1), -1, 32)
    y1 = R.store_bf16(R.relu(R.linear(st_rows, w1, s1, h1)))
    y1 = R.permute(R.reshape(y1, N, Hs, Ws, C1), 0, 3, 1, 2)
    y2 = R.permute(R.store_bf16(R.relu(R.conv2d(y1, w2, 2, C1 // gw, s2, h2))), 0, 2, 3, 1)     # NHWC
    st_even = R.permute(R.RB(st.ref[:, :, ::2, ::2], st.d[:, :, ::2, ::2]), 0, 2, 3, 1)
    Ho, Wo = st_even.ref.shape[1:3]
    scut = R.reshape(R.store_bf16(R.linear(R.reshape(st_even, -1, 32), wd, sd_, hd)), N, Ho, Wo, C1)
    assert tuple(y2.ref.shape) == (N, Ho, Wo, C1)
    frac = R.relu_open(y2.ref)
    assert 0.2 < frac < 0.8, frac
    fw = pack_front_weights(sw, ss, hs, w1, s1, h1, wd, sd_, hd, w2, gw, s2, h2, DEV)
    ch, cw = (crop[2], crop[3]) if crop else (H, W)
    parts = ops.s1_front_parts(ch, cw, C1)
    assert parts > 0
    g2, gs, gp = Guarded((N, Ho, Wo, C1)), Guarded((N, Ho, Wo, C1)), Guarded((N, parts, C1), torch.float32)
    ops.s1_front(fr.to(DEV), fw, crop, flip, y2=g2.view, shortcut=gs.view, pooled=gp.view)
    name = f"s1_front {geom}"
    o2, os_, op = g2.check(name + " y2"), gs.check(name + " shortcut"), gp.check(name + " pooled")
    R.assert_within(o2, y2, name + " y2", nhwc=True)
    R.assert_within(os_, scut, name + " shortcut", nhwc=True)
    R.assert_pooled_consistent(op, o2, name)


# ----------------------------------------------------------------------------- average pool + positional encoding
def test_avgpool_posenc(ops):
    """mean over the 7 x 7 pixels (a contraction of K = 49 ones, scale 1 / 49) + the frame's encoding, one bf16 store"""
    B, T, hw, C = 2, 5, 49, 368
    x = rnd(460, "x", (B * T, 7, 7, C)).to(BF)
    te = rnd(461, "te", (T, C))
    xd, te_rows = R.f64(x).view(B * T, hw, C), R.f64(te).repeat(B, 1)
    mean = R.RB(xd.sum(1) / hw + te_rows, (hw + 4) * 2.0 ** -23 * (xd.abs().sum(1) / hw + te_rows.abs()))
    ref = R.reshape(R.store_bf16(mean), B, T, C)
    g = Guarded((B, T, C))
    ops.avgpool_posenc(x.to(DEV), B, T, te.to(DEV), out=g.view)
    out = g.check("avgpool_posenc")
    R.assert_within(out, ref, "avgpool_posenc")
