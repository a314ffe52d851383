"""The band walk of the conv3-in c1_gconv launch (c1_gconv_c3in_walk_kernel, tdeed_c1_gconv_c3in_set_walk): a workgroup that
owns a run of bands of a frame gives the bits of a workgroup per band (runs of one band: the same kernel since the per-band
kernel left), of the two launches the form replaced -- the independent reference -- and of the stride-2 pixels of the map
nobody writes -- at every run length, 1 included, at the shapes where the walk can go wrong (a re-zeroed bottom row, a short
last band, an odd frame count, one band), and over a whole forward.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import model_state, t, act
from tdeed_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (Hi, Wi, Cp, C, gw, N frames, bands per frame)
CASES = [(19, 56, 24, 56, 8, 2, 5),    # five bands, the last one's bottom row outside the map (the re-zero)
         (18, 56, 24, 56, 8, 2, 5),    # five bands, the last of one output row (short last band, compact-row ownership)
         (10, 56, 24, 56, 8, 3, 3),    # three bands, an odd frame count
         (15, 13, 24, 56, 8, 2, 1),    # one band: a run of one band at every setting
         (12, 20, 32, 64, 16, 2, 1),
         (8, 6, 8, 32, 8, 2, 1)]
SENTINEL = -7.0                        # every defined output is behind a ReLU
GUARD = 4096                           # elements in front of and behind each output buffer


@pytest.fixture(autouse=True)
def routed_walk_again():
    from tdeed_amd import ops
    yield
    ops.c1_gconv_c3in_set_walk(0)


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


@pytest.mark.parametrize("Hi,Wi,Cp,C,gw,N,bands", CASES)
def test_every_run_length_gives_the_bits_of_the_per_band_kernel_and_of_the_chain(Hi, Wi, Cp, C, gw, N, bands):
    from tdeed_amd import ops
    from tdeed_amd.packing import pack_ws_weights, pack_mfma_frags, pack_gconv_frags
    assert ops.c1_gconv_c3in_fits(Hi, Wi, Cp, C)
    assert ops.gconv3x3_parts(Hi, Wi, C, 2, BF) == bands
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
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
    # the references, once: the chain, the stride-2 pixels of its map, the launch in runs of one band
    out = ops.gemm_ws(y2p, W3, Cp, Cp, s3, h3, ops.ACT_RELU, residual=scp, a_scale=gate, a_scale_rows=Hi * Wi).view(N, Hi, Wi, Cp)
    y_ref, p_ref = ops.c1_gconv(out, w1f, s1, h1, w2f, s2, h2, gw, 2, C)
    xs_ref = out[:, ::2, ::2, :].contiguous()
    ops.c1_gconv_c3in_set_walk(1)
    assert ops.c1_gconv_c3in_workgroups(N, Hi, Wi, Cp, C) == N * bands
    xs_1 = torch.full_like(xs_ref, SENTINEL)
    y_1, p_1 = ops.c1_gconv_c3in(y2p, scp, gate, W3, s3, h3, w1f, s1, h1, w2f, s2, h2, gw, C, xs2=xs_1)
    torch.cuda.synchronize()
    assert torch.equal(y_1, y_ref) and torch.equal(p_1, p_ref) and torch.equal(xs_1, xs_ref)
    frac = float((out > 0).float().mean())
    assert 0.2 < frac < 0.8, frac                                            # conv3's ReLU is neither always open nor shut
    routed = ops.c1_gconv_c3in_walk(Hi, Wi, Cp, C)
    assert 1 <= routed <= bands
    for walk in sorted({1, 2, 3, bands, routed}) + [0]:                      # (0: as routed, through the default setting)
        ops.c1_gconv_c3in_set_walk(walk)
        eff = min(walk if walk else routed, bands)
        assert ops.c1_gconv_c3in_workgroups(N, Hi, Wi, Cp, C) == N * -(-bands // eff), walk
        y_flat, y = _guarded((N, Ho, Wo, C))
        xs_flat, xs2 = _guarded((N, Ho, Wo, Cp))
        pooled = torch.full_like(p_ref, float("nan"))
        ops.c1_gconv_c3in(y2p, scp, gate, W3, s3, h3, w1f, s1, h1, w2f, s2, h2, gw, C, xs2=xs2, out=y, pooled=pooled)
        torch.cuda.synchronize()
        for ref_y, ref_p, ref_x in ((y_1, p_1, xs_1), (y_ref, p_ref, xs_ref)):
            assert torch.equal(y, ref_y), (walk, float((y.float() - ref_y.float()).abs().max()))
            assert torch.equal(pooled, ref_p), walk
            assert torch.equal(xs2, ref_x), (walk, float((xs2.float() - ref_x.float()).abs().max()))
        for flat, view in ((y_flat, y), (xs_flat, xs2)):
            assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + view.numel():] == SENTINEL).all()), walk
            assert not bool((view == SENTINEL).any()), walk
        # without the compact map the other outputs are the same
        y_b, p_b = ops.c1_gconv_c3in(y2p, scp, gate, W3, s3, h3, w1f, s1, h1, w2f, s2, h2, gw, C)
        torch.cuda.synchronize()
        assert torch.equal(y_b, y_ref) and torch.equal(p_b, p_ref), walk


def test_whole_forward_is_bit_identical_under_the_walk():
    """224 x 224, B = 1, T = 4, bf16, synthetic weights, no graph: s2.b1's launch runs at 56 x 56 (14 bands per frame)"""
    from tdeed_amd import engine as E, ops
    cfg = dict(feature_arch="rny002_gsf", clip_len=4, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
               radi_displacement=2)
    sd = model_state(cfg, 5)
    clip = t(synth.uint8_clip(77, (1, 4, 3, 224, 224))).to(DEV)
    eng = E.ForwardEngine(cfg, sd, BF, DEV, use_graph=False)
    heads, grids = {}, {}
    for walk in (1, 0, 14):
        ops.c1_gconv_c3in_set_walk(walk)
        grids[walk] = ops.c1_gconv_c3in_workgroups(4, 56, 56, 24, 56)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            head, plan = eng.forward(clip)
            st.synchronize()
        heads[walk] = head.clone()
        assert "s1.b1.conv3" not in [s.name for s in plan.steps]            # the conv3-in form is the one that runs
    assert grids[1] == 4 * 14 and grids[14] == 4
    assert torch.equal(heads[1], heads[14])
    assert torch.equal(heads[1], heads[0])
    # not vacuous for the routed setting wherever a walk is routed: the grids of the two settings differ at this size
    routed = ops.c1_gconv_c3in_walk(56, 56, 24, 56)
    assert grids[0] == 4 * -(-14 // routed) and (routed == 1 or grids[0] != grids[1])
