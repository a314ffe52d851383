"""The producer's conv3 inside the conv1 + grouped-conv launch of a stride-2 block (tdeed_c1_gconv_c3in_fwd,
engine.S1_CONV3_IN_C1G): the fused launch gives the bits of the two launches it replaces and of the stride-2 pixels of the
map it no longer writes, at the kernel and over a whole forward.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import load_golden, model_state, t, act
from tdeed_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (Hi, Wi, Cp, C, gw, N frames)
CASES = [(56, 56, 24, 56, 8, 3),       # the timed geometry per frame, 14 bands
         (10, 56, 24, 56, 8, 2),       # three bands, the last of one row: compact-row ownership at a short band
         (15, 13, 24, 56, 8, 2),       # odd map, one band, a masked tail tile
         (12, 20, 32, 64, 16, 2),      # Cp = 32: no zero k-chunk, group width 16
         (8, 6, 8, 32, 8, 2)]          # Cp = 8: three zero k-chunks, 32-channel slab
SENTINEL = -7.0                        # every defined output is behind a ReLU
GUARD = 4096                           # elements in front of and behind each output buffer


def _fold(seed, name, n):
    """a random BatchNorm fold: scales of both signs, magnitudes 0.5 .. 1.5"""
    a = t(act(seed, name + "s", (n,)))
    sc = torch.where(a >= 0, 1.0, -1.0) * (0.5 + t(act(seed, name + "m", (n,))).abs().clamp(max=1.0))
    return sc.to(DEV), t(act(seed, name + "h", (n,))).to(DEV)


def _guarded(shape):
    """(flat buffer, view of `shape` in its middle), all SENTINEL"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=BF, device=DEV)
    return flat, flat[GUARD:GUARD + n].view(*shape)


@pytest.mark.parametrize("Hi,Wi,Cp,C,gw,N", CASES)
def test_fused_launch_equals_the_chain(Hi, Wi, Cp, C, gw, N):
    from tdeed_amd import ops
    from tdeed_amd.packing import pack_ws_weights, pack_mfma_frags, pack_gconv_frags
    assert ops.c1_gconv_c3in_fits(Hi, Wi, Cp, C)
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    M = N * Hi * Wi
    seed = Hi * 100 + Wi
    y2p = t(act(seed, "y2p", (N, Hi, Wi, Cp))).to(BF).to(DEV)
    scp = t(act(seed, "scp", (N, Hi, Wi, Cp))).to(BF).to(DEV)
    gate = torch.sigmoid(t(act(seed, "g", (N, Cp)))).to(DEV)                 # (0, 1), one row per frame
    assert not torch.equal(gate[0], gate[1])
    W3 = pack_ws_weights(act(seed, "w3", (Cp, Cp), 1.0 / np.sqrt(Cp)), BF, DEV)
    s3, h3 = _fold(seed, "3", Cp)
    W1 = act(seed, "w1", (C, Cp), 1.0 / np.sqrt(Cp))
    W2 = act(seed, "w2", (C, gw, 3, 3), 1.0 / np.sqrt(gw * 9))
    s1, h1 = _fold(seed, "1", C)
    s2, h2 = _fold(seed, "2", C)
    w1f = pack_mfma_frags(W1, DEV, rows=16 * ops.c1_gconv_slab_tiles(Hi, Wi, C, 2))
    w2f = pack_gconv_frags(W2, gw, DEV)
    # the chain
    out = ops.gemm_ws(y2p, W3, Cp, Cp, s3, h3, ops.ACT_RELU, residual=scp, a_scale=gate, a_scale_rows=Hi * Wi).view(N, Hi, Wi, Cp)
    y_ref, p_ref = ops.c1_gconv(out, w1f, s1, h1, w2f, s2, h2, gw, 2, C)
    xs_ref = out[:, ::2, ::2, :].contiguous()
    # the fused launch, into guarded sentinel buffers
    y_flat, y = _guarded((N, Ho, Wo, C))
    xs_flat, xs2 = _guarded((N, Ho, Wo, Cp))
    pooled = torch.full_like(p_ref, float("nan"))
    ops.c1_gconv_c3in(y2p, scp, gate, W3, s3, h3, w1f, s1, h1, w2f, s2, h2, gw, C, xs2=xs2, out=y, pooled=pooled)
    torch.cuda.synchronize()
    # the operands exercise the residual and the ReLU of conv3 (and the ReLU is not always open)
    pre = ops.gemm_ws(y2p, W3, Cp, Cp, s3, h3, ops.ACT_NONE, a_scale=gate, a_scale_rows=Hi * Wi).view(N, Hi, Wi, Cp)
    assert float(scp.float().abs().max()) > 0.5 and not torch.equal(torch.relu(pre), out)
    frac = float((out > 0).float().mean())
    assert 0.2 < frac < 0.8, frac
    assert xs_ref.shape == xs2.shape
    assert torch.equal(y, y_ref), float((y.float() - y_ref.float()).abs().max())
    assert torch.equal(pooled, p_ref)
    assert torch.equal(xs2, xs_ref), float((xs2.float() - xs_ref.float()).abs().max())
    for flat, view in ((y_flat, y), (xs_flat, xs2)):
        assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + view.numel():] == SENTINEL).all())
        assert not bool((view == SENTINEL).any())
    # without the compact map the other outputs are the same
    y_b, p_b = ops.c1_gconv_c3in(y2p, scp, gate, W3, s3, h3, w1f, s1, h1, w2f, s2, h2, gw, C)
    torch.cuda.synchronize()
    assert torch.equal(y_b, y_ref) and torch.equal(p_b, p_ref)


def test_whole_forward_is_bit_identical_without_the_conv3_launch(monkeypatch):
    from tdeed_amd import engine as E
    meta, g = load_golden("tiny_rny002_gsf")
    cfg = meta["cfg"]
    sd = model_state(cfg, meta["seed_w"])
    clip = t(synth.uint8_clip(meta["seed_x"], (meta["B"], cfg["clip_len"], 3, meta["H"], meta["W"]))).to(DEV)
    real, seen = E.block_forms, {}
    heads, names = {}, {}
    for on in (True, False):
        monkeypatch.setattr(E, "S1_CONV3_IN_C1G", on)

        def recorded(blocks, *a, on=on):
            forms = real(blocks, *a)
            seen.setdefault(on, []).append(([bw.spec.name for bw in blocks], forms))
            return forms
        monkeypatch.setattr(E, "block_forms", recorded)
        eng = E.ForwardEngine(cfg, sd, BF, DEV, use_graph=False)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            head, plan = eng.forward(clip)
            st.synchronize()
        heads[on], names[on] = head.clone(), [s.name for s in plan.steps]
    # not vacuous: the fused front is taken at this size, and with the switch on the block behind it takes the form
    assert "s1_front" in names[True] and "s1_front" in names[False]
    first = lambda on: [(bl[0], fs[0].conv3_in) for bl, fs in seen[on] if bl and bl[0] == "s2.b1"]   # noqa: E731
    assert first(True) and all(c for _, c in first(True))
    assert first(False) and not any(c for _, c in first(False))
    assert torch.equal(heads[True], heads[False])
    assert "s1.b1.conv3" not in names[True] and "s1.b1.se" in names[True]
    # (a plan lists the trunk once per sub-batch)
    per = names[False].count("s1.b1.conv3")
    assert per >= 1 and len(names[True]) == len(names[False]) - per
    # off: the chain's names, conv3 behind the front block's SE; on: the same list without it
    assert [n for n in names[False] if n != "s1.b1.conv3"] == names[True]
    assert all(names[False][i + 1] == "s1.b1.conv3" for i, n in enumerate(names[False]) if n == "s1.b1.se")
