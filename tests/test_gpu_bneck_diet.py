"""GPU: the one-launch bottleneck after its vector-instruction diet (walked piece offsets in the staging passes, the tap masks
and stepped tap offsets of conv2, the squeeze sums as one running sum that is banked at the frame boundary, the clamped residual
offsets of conv3) -- the comparisons of test_gpu_r3.py / test_gpu_r6.py at shapes chosen for the new paths: a tile that holds
both frames, a frame boundary on a tile boundary, ragged last tiles of 1 / 2 / 4 / 6 rows, whole tiles only, a last workgroup
with one frame, the LDS maximum of the one-frame form."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# h, w, C, R, N
SHAPES = [(7, 7, 368, 92, 5),        # tile 3 holds both frames, tile 6 is ragged; odd N: the last workgroup has one frame
          (6, 8, 368, 92, 4),        # 48 pixels: frame 1 starts on a tile boundary
          (5, 5, 368, 92, 3),        # the tile with both frames has 9 rows of frame 0
          (8, 8, 152, 38, 4),        # <5, 2, 8>, exactly 8 whole tiles
          (7, 7, 152, 38, 3),        # <5, 2, 8>, ragged
          (14, 14, 152, 38, 2),      # last tile of 4 rows
          (13, 14, 152, 38, 2),      # last tile of 6 rows
          (5, 13, 152, 38, 2),       # 65 pixels: last tile of 1 row
          (13, 16, 152, 38, 1)]      # 208 pixels = 13 whole tiles: the LDS maximum of the one-frame form


@functools.lru_cache(maxsize=None)
def _case(h, w, C, R, N):
    """operands of one shape (seeded), made once and shared by the tests below; nothing writes to them"""
    from tdeed_amd.engine import pack_mfma_frags, pack_gconv_frags, pack_se_mfma
    from tdeed_amd.regnet_spec import gsf_fold_dim
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + C + N)
    gw, F = 8, gsf_fold_dim(C)
    Fp = (F + 7) // 8 * 8
    x = torch.relu(torch.randn(N, h, w, C, generator=g)).to(torch.bfloat16).to(DEV)
    G = torch.randn(N * h * w, Fp, generator=g).to(torch.bfloat16).to(DEV)
    W1, W3 = torch.randn(C, C, generator=g) / C ** 0.5, torch.randn(C, C, generator=g) / C ** 0.5
    W2 = torch.randn(C, gw, 3, 3, generator=g) / (gw * 9) ** 0.5
    fc1, fc2 = torch.randn(R, C, generator=g) / C ** 0.5, torch.randn(C, R, generator=g) / R ** 0.5
    vec = lambda n, s_=0.1, o=0.0: (torch.randn(n, generator=g) * s_ + o).to(DEV)          # noqa: E731
    s1, h1, s2, h2, s3, h3 = vec(C, 0.1, 1.0), vec(C), vec(C, 0.1, 1.0), vec(C), vec(C, 0.1, 0.5), vec(C)
    b1, b2 = vec(R), vec(C)
    se = pack_se_mfma(fc1.numpy(), fc2.numpy(), DEV)
    blk = (pack_mfma_frags(W1.numpy(), DEV), s1, h1, pack_gconv_frags(W2.numpy(), gw, DEV, tap_major=True), s2, h2,
           se["w1f"], b1, se["w2f"], b2, R, pack_mfma_frags(W3.numpy(), DEV), s3, h3)
    chain = dict(W1d=W1.to(torch.bfloat16).to(DEV), W3d=W3.to(torch.bfloat16).to(DEV), w2f=pack_gconv_frags(W2.numpy(), gw, DEV),
                 se=se, bn=(s1, h1, s2, h2, s3, h3), b=(b1, b2))

    def site():
        from tdeed_amd.engine import pack_gsf_q_frags, pack_gsf_p_frags
        w3d = torch.randn(2, F // 2, 3, 3, 3, generator=g) * 0.1
        f32 = lambda *s: (torch.randn(s, generator=g) * 0.3).to(DEV)      # noqa: E731
        return dict(bn_s=f32(F).abs() + 0.5, bn_b=f32(F), b3d=f32(2), cw=[f32(18), f32(1), f32(18), f32(1)],
                    wq=w3d.reshape(F, 27).t().contiguous().to(DEV), wqf=pack_gsf_q_frags(w3d.numpy(), DEV),
                    wpf=pack_gsf_p_frags(w3d.numpy(), DEV))
    return dict(x=x, G=G, F=F, Fp=Fp, gw=gw, blk=blk, chain=chain, s0=site(), s1=site())


@pytest.mark.parametrize("h,w,C,R,N", SHAPES)
def test_one_launch_equals_the_chain(h, w, C, R, N):
    """tdeed_bneck_fwd (with the gate-shift splice) against gemm -> gconv3x3 -> se_gate_mfma -> gemm on the same operands:
    `out` and the compact `out2` bit for bit."""
    from tdeed_amd import ops
    assert ops.bneck_fits(h, w, C, R)
    c = _case(h, w, C, R, N)
    x, G, Fp, ch = c["x"], c["G"], c["Fp"], c["chain"]
    s1, h1, s2, h2, s3, h3 = ch["bn"]
    b1, b2 = ch["b"]
    hw, M = h * w, N * h * w
    y1 = ops.gemm(x.view(M, C), ch["W1d"], s1, h1, ops.ACT_RELU, A0=G, k0=Fp)
    y2, pooled = ops.gconv3x3(y1.view(N, h, w, C), None, s2, h2, c["gw"], 1, wfrag=ch["w2f"])
    gate = ops.se_gate_mfma(pooled, 1.0 / hw, ch["se"]["w1f"], b1, ch["se"]["w2f"], b2, R)
    ref2 = torch.empty((M, 48), dtype=torch.bfloat16, device=DEV)
    ref = ops.gemm(y2.view(M, C), ch["W3d"], s3, h3, ops.ACT_RELU, residual=x.view(M, C), a_scale=gate, a_scale_rows=hw, out2=ref2)
    out2 = torch.empty_like(ref2)
    out = ops.bneck(x, *c["blk"], G=G, out2=out2, w2_tap_major=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out.view(M, C), ref), float((out.view(M, C).float() - ref.float()).abs().max())
    assert torch.equal(out2, ref2)


def _blend_cases():
    # every shape as one clip; the two shipped shapes also as one-frame clips (no neighbour on either side) and as two clips
    # of three frames (a workgroup's two frames in different clips)
    cases = [(h, w, C, R, 1, N) for (h, w, C, R, N) in SHAPES]
    for h, w, C, R in ((7, 7, 368, 92), (14, 14, 152, 38)):
        cases += [(h, w, C, R, 3, 1), (h, w, C, R, 2, 3)]
    return cases


@pytest.mark.parametrize("h,w,C,R,B,T", _blend_cases())
def test_blend_inside_equals_blend_then_bottleneck(h, w, C, R, B, T):
    """tdeed_bneck_gs_fwd against tdeed_gsf_blend_src_fwd -> tdeed_bneck_fwd: bit for bit."""
    from tdeed_amd import ops
    N = B * T
    assert ops.bneck_fits(h, w, C, R)
    c = _case(h, w, C, R, N)
    x, F, Fp, s0 = c["x"], c["F"], c["Fp"], c["s0"]
    G = ops.gate_shift(x, B, T, F, Fp, s0["bn_s"], s0["bn_b"], s0["wq"], s0["b3d"], *s0["cw"], wqf=s0["wqf"], src_order=True)
    o2r = torch.empty((N * h * w, 40), dtype=torch.bfloat16, device=DEV)
    ref = ops.bneck(x, *c["blk"], G=G, out2=o2r)
    gate, ysum, xsum = ops.gate_shift(x, B, T, F, Fp, s0["bn_s"], s0["bn_b"], s0["wq"], s0["b3d"], *s0["cw"], wqf=s0["wqf"],
                                      gates_only=True)
    o2 = torch.empty_like(o2r)
    out = ops.bneck_gs(x, x, gate, ysum, xsum, *s0["cw"], T, F, Fp, *c["blk"], out2=o2)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(o2, o2r)


# the table's shapes whose tap-map tail fits region A (tdeed_bneck_qtail_fits by hand: pixels * ((nch | 1) * 16 + 224) + the
# fragments <= pixels * RS, RS = 736 at C = 368 and 352 at C = 152); the two-frame 152-wide forms and 5 x 13 do not
TAIL_FITS = {(7, 7, 368), (6, 8, 368), (5, 5, 368), (14, 14, 152), (13, 14, 152), (13, 16, 152)}


@pytest.mark.parametrize("h,w,C,R,B,T", _blend_cases())
def test_tap_maps_from_the_tail_equal_the_gate_launch(h, w, C, R, B, T):
    """Q of the launch's tail against the stand-alone tap-map launch on the block's output, to test_gpu_r6.py's tolerance (2e-6 of
    the largest map value: the same bf16 products in fp32, another summation order); the block's outputs are unchanged by it.
    Every shape of the table where the tail fits (one clip), the two shipped shapes also as one-frame clips and as two clips of
    three frames; where it does not fit, that is what is asserted."""
    from tdeed_amd import ops
    from tdeed_amd.regnet_spec import gsf_fold_dim
    assert ops.bneck_qtail_fits(h, w, C, gsf_fold_dim(C)) == ((h, w, C) in TAIL_FITS)
    if (h, w, C) not in TAIL_FITS:
        return
    N = B * T
    c = _case(h, w, C, R, N)
    x, F, Fp, s0, s1 = c["x"], c["F"], c["Fp"], c["s0"], c["s1"]
    assert ops.bneck_fits(h, w, C, R) and ops.bneck_qtail_fits(h, w, C, F)
    gate, ysum, xsum = ops.gate_shift(x, B, T, F, Fp, s0["bn_s"], s0["bn_b"], s0["wq"], s0["b3d"], *s0["cw"], wqf=s0["wqf"],
                                      gates_only=True)
    o2a, o2b = (torch.empty((N * h * w, Fp), dtype=torch.bfloat16, device=DEV) for _ in range(2))
    ref = ops.bneck_gs(x, x, gate, ysum, xsum, *s0["cw"], T, F, Fp, *c["blk"], out2=o2a)
    Q = torch.full((N, h, w, 6), float("nan"), device=DEV)
    out = ops.bneck_gs(x, x, gate, ysum, xsum, *s0["cw"], T, F, Fp, *c["blk"], out2=o2b,
                       qtail=(s1["wpf"], ops.gsq_bn_table(s1["bn_s"], s1["bn_b"]), F, Q))
    assert torch.equal(out, ref) and torch.equal(o2a, o2b)
    bufs = dict(q=torch.empty((N, h, w, 6), device=DEV))
    ops.gate_shift(o2a.view(N, h, w, Fp), B, T, F, Fp, s1["bn_s"], s1["bn_b"], s1["wq"], s1["b3d"], *s1["cw"], wqf=s1["wqf"],
                   bufs=bufs, gates_only=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Q).all())
    err, top = float((Q - bufs["q"]).abs().max()), float(bufs["q"].abs().max())
    print(f"tap maps {h}x{w}x{C} B={B} T={T}: max abs difference {err:.3g}, largest map value {top:.3g}")
    assert err <= 2e-6 * top, err
