"""The slab-loop form of tdeed_c1_gconv_fwd (one workgroup per (frame, band) keeps its x / G fragments in registers and walks
the channel slabs) gives the bits of the per-slab form: output rows and squeeze partial sums at the kernel, the head output
over a whole forward.  -m gpu only."""
import pytest
import torch

from helpers import Guarded, load_golden, model_state, t, act
from tdeed_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (N, Hi, Wi, Cin, C, gw, Fp)
CASES = [(3, 28, 28, 56, 152, 8, 16),     # cfg2 s3.b1: 3 slabs (the last of 24 channels), bands 5 + 5 + 4, the splice
         (3, 28, 28, 56, 152, 8, 0),      # the same without G
         (3, 14, 14, 152, 368, 8, 40),    # cfg2 s4.b1: 6 slabs (the last of 48 channels), one band, five k-steps
         (2, 13, 13, 152, 368, 8, 40),    # odd map -> 7 x 7, a partial pixel tile
         (2, 27, 27, 56, 152, 8, 16),     # odd map -> 14 x 14
         (1, 28, 28, 56, 152, 8, 16),     # one frame
         (1, 14, 14, 152, 368, 8, 0)]


@pytest.fixture(autouse=True)
def routed_form_afterwards():
    from tdeed_amd import ops
    yield
    ops.c1_gconv_set_form(-1)


@pytest.mark.parametrize("N,Hi,Wi,Cin,C,gw,Fp", CASES)
def test_slab_loop_equals_the_per_slab_form(N, Hi, Wi, Cin, C, gw, Fp):
    import numpy as np
    from tdeed_amd import ops
    from tdeed_amd.packing import pack_mfma_frags, pack_gconv_frags
    assert ops.c1_gconv_slab_loop_fits(Hi, Wi, Cin, C, 2)
    seed = Hi * 1000 + C + Fp
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    x = torch.relu(t(act(seed, "x", (N, Hi, Wi, Cin)))).to(BF).to(DEV)
    G = t(act(seed, "G", (N * Hi * Wi, Fp))).to(BF).to(DEV) if Fp else None
    W1 = act(seed, "w1", (C, Cin), 1.0 / np.sqrt(Cin))
    W2 = act(seed, "w2", (C, gw, 3, 3), 1.0 / np.sqrt(gw * 9))
    vec = lambda name, o=0.0: (0.1 * t(act(seed, name, (C,))) + o).to(DEV)          # noqa: E731
    s1, h1, s2, h2 = vec("s1", 1.0), vec("h1"), vec("s2", 1.0), vec("h2")
    w1f = pack_mfma_frags(W1, DEV, rows=16 * ops.c1_gconv_slab_tiles(Hi, Wi, C, 2))
    w2f = pack_gconv_frags(W2, gw, DEV)
    parts = ops.gconv3x3_parts(Hi, Wi, C, 2, BF)
    nslabs = (C + 63) // 64
    res = {}
    for form in (0, 1):
        ops.c1_gconv_set_form(form)
        assert ops.c1_gconv_workgroups(N, Hi, Wi, Cin, C, 2) == N * parts * (1 if form else nslabs)
        y, pooled = Guarded((N, Ho, Wo, C)), Guarded((N, parts, C), dtype=torch.float32)
        ops.c1_gconv(x, w1f, s1, h1, w2f, s2, h2, gw, 2, C, G=G, out=y.view, pooled=pooled.view)
        res[form] = (y.check(f"y, form {form}"), pooled.check(f"pooled, form {form}"))
    # the operands exercise the ReLU behind the grouped conv
    frac = float((res[0][0] > 0).float().mean())
    assert 0.1 < frac < 0.9, frac
    assert torch.equal(res[1][0], res[0][0]), float((res[1][0].float() - res[0][0].float()).abs().max())
    assert torch.equal(res[1][1], res[0][1])


def test_whole_forward_is_bit_identical_in_either_form(monkeypatch):
    from tdeed_amd import engine as E, ops
    meta, g = load_golden("tiny_rny002_gsf")
    cfg = meta["cfg"]
    sd = model_state(cfg, meta["seed_w"])
    clip = t(synth.uint8_clip(meta["seed_x"], (meta["B"], cfg["clip_len"], 3, meta["H"], meta["W"]))).to(DEV)
    real, taken = ops.c1_gconv, []

    def recorded(x, w1f, s1, h1, wfrag, scale, shift, gw, stride, C, **kw):
        N, Hi, Wi, Cin = x.shape
        taken.append(ops.c1_gconv_slab_loop_fits(Hi, Wi, Cin, C, stride)
                     and ops.c1_gconv_workgroups(N, Hi, Wi, Cin, C, stride) == N * ops.gconv3x3_parts(Hi, Wi, C, stride, BF))
        return real(x, w1f, s1, h1, wfrag, scale, shift, gw, stride, C, **kw)
    monkeypatch.setattr(ops, "c1_gconv", recorded)
    heads, used, steps = {}, {}, {}
    for form in (1, 0):
        ops.c1_gconv_set_form(form)
        del taken[:]
        eng = E.ForwardEngine(cfg, sd, BF, DEV, use_graph=False)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            head, plan = eng.forward(clip)
            st.synchronize()
        heads[form], used[form], steps[form] = head.clone(), list(taken), [s.name for s in plan.steps]
    # not vacuous: forced on, launches of this forward take the slab loop; forced off, none does; the plan is the same
    assert any(used[1]) and used[0] and not any(used[0])
    assert steps[1] == steps[0]
    assert torch.isfinite(heads[0].float()).all()
    assert torch.equal(heads[1], heads[0])
