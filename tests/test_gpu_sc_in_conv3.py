"""The shortcut conv of a strided bottleneck inside conv3's launch (tdeed_gemm_ws_sc_fwd, engine.SC_IN_CONV3): the fused launch
gives the bits of the two launches it replaces, at the kernel and over a whole forward.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import load_golden, model_state, t, act
from tdeed_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (Hi, Wi, Cin, C, N frames, n2): input map of the block, its input / output channels, columns of the compact second output
CASES = [(8, 6, 24, 56, 3, 16),        # one shortcut k-step, even map
         (7, 9, 24, 56, 5, 16),        # odd map: output 4 x 5, M2 = 100 < one 128-row chunk (masked tail)
         (10, 14, 56, 152, 5, 40),     # five + two k-steps; M2 = 175 crosses a chunk, frames inside one; half-empty last tile pair
         (6, 6, 64, 144, 2, 0)]        # the RegNetY-800MF s2.b1 widths, no second output


def _fold(seed, name, n):
    """a random BatchNorm fold: scales of both signs, magnitudes 0.5 .. 1.5"""
    a = t(act(seed, name + "s", (n,)))
    sc = torch.where(a >= 0, 1.0, -1.0) * (0.5 + t(act(seed, name + "m", (n,))).abs().clamp(max=1.0))
    return sc.to(DEV), t(act(seed, name + "h", (n,))).to(DEV)


@pytest.mark.parametrize("Hi,Wi,Cin,C,N,n2", CASES)
def test_fused_launch_equals_the_two_launches(Hi, Wi, Cin, C, N, n2):
    from tdeed_amd import ops
    from tdeed_amd.packing import pack_ws_weights
    assert ops.gemm_ws_sc_fits(C, Cin, C, BF)
    h2, w2 = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    M2 = N * h2 * w2
    seed = Hi * 100 + Wi
    x = t(act(seed, "x", (N, Hi, Wi, Cin))).to(BF).to(DEV)
    y2 = t(act(seed, "y2", (M2, C))).to(BF).to(DEV)
    gate = torch.sigmoid(t(act(seed, "g", (N, C)))).to(DEV)                   # (0, 1), one row per frame
    Wd = pack_ws_weights(act(seed, "wd", (C, Cin), 1.0 / np.sqrt(Cin)), BF, DEV)
    W3 = pack_ws_weights(act(seed, "w3", (C, C), 1.0 / np.sqrt(C)), BF, DEV)
    sd, hd = _fold(seed, "d", C)
    s3, h3 = _fold(seed, "3", C)
    gather = (2, Hi, Wi, h2, w2)
    sc = ops.gemm_ws(x, Wd, Cin, C, sd, hd, ops.ACT_NONE, gather=gather)
    ref2 = torch.zeros((M2, n2), dtype=BF, device=DEV) if n2 else None
    ref = ops.gemm_ws(y2, W3, C, C, s3, h3, ops.ACT_RELU, residual=sc, a_scale=gate, a_scale_rows=h2 * w2, out2=ref2)
    got2 = torch.zeros((M2, n2), dtype=BF, device=DEV) if n2 else None
    got = ops.gemm_ws_sc(y2, W3, C, C, s3, h3, x, Wd, Cin, sd, hd, ops.ACT_RELU, a_scale=gate, a_scale_rows=h2 * w2,
                         gather=gather, out2=got2)
    torch.cuda.synchronize()
    assert float(sc.float().abs().max()) > 0.5 and float((ref > 0).float().mean()) > 0.2      # the operands exercise both terms
    assert torch.equal(got, ref)
    if n2:
        assert torch.equal(got2, ref2) and torch.equal(got2, ref[:, :n2])


def test_whole_forward_is_bit_identical_and_has_no_downsample_launch(monkeypatch):
    from tdeed_amd import engine as E
    meta, g = load_golden("tiny_rny002_gsf")
    cfg = meta["cfg"]
    sd = model_state(cfg, meta["seed_w"])
    clip = t(synth.uint8_clip(meta["seed_x"], (meta["B"], cfg["clip_len"], 3, meta["H"], meta["W"]))).to(DEV)
    heads, names = {}, {}
    for on in (True, False):
        monkeypatch.setattr(E, "SC_IN_CONV3", on)
        eng = E.ForwardEngine(cfg, sd, BF, DEV, use_graph=False)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            head, plan = eng.forward(clip)
            st.synchronize()
        heads[on], names[on] = head.clone(), [s.name for s in plan.steps]
    assert torch.equal(heads[True], heads[False])
    ds = lambda ns: sorted(set(n for n in ns if n.endswith(".downsample")))   # noqa: E731
    # s1.b1's shortcut comes from the front kernel; s2.b1 and s3.b1 take the fused form; s4.b1 (368 wide) keeps its launch
    assert ds(names[False]) == ["s2.b1.downsample", "s3.b1.downsample", "s4.b1.downsample"]
    assert ds(names[True]) == ["s4.b1.downsample"]
    # (a plan lists the trunk once per sub-batch)
    assert len(names[True]) == len(names[False]) - 2 * names[False].count("s2.b1.downsample")
