"""Round-3 parity tests on the MI355X (through the C ABI): the configurations VERDICT r2 listed as untested -- the
SoccerNetBall long-clip train step (BASELINE configs[4]: 800MF, T=250) against autograd on the oracle, the bf16 train step
of BASELINE configs[2] at its real batch (B=16) eager vs captured, and captured training graphs that share an engine
with eager steps and with each other.  -m gpu only."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import t
from tdeed_amd import synth, state_layout
from tdeed_amd.regnet_spec import regnet_spec
from test_gpu_r2 import _oracle_train_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"

CFG5 = dict(feature_arch="rny008_gsf", clip_len=250, crop_dim=None, n_layers=2, sgp_ks=9, sgp_r=4, num_classes=12,
            radi_displacement=4)          # config/SoccerNetBall/SoccerNetBall_challenge2.json:16,21-23 at clip_len 250
CFG3 = dict(feature_arch="rny008_gsf", clip_len=100, crop_dim=224, n_layers=3, sgp_ks=7, sgp_r=4, num_classes=4,
            radi_displacement=2)


def test_cfg5_long_clip_800mf_train_step_matches_autograd():
    """BASELINE configs[4] per-GPU share (RegNetY-800MF, SoccerNetBall hyper-parameters n_layers=2 ks=9 K=12 radi=4,
    T=250; B=1, 64x64 frames): loss and EVERY gradient of one train-mode forward / backward in fp32 against autograd on
    the CPU oracle.  The trunk and gate-shift backward (model/impl/gsf.py:38-93 through autograd in the reference) had
    only run at T <= 100 in a test before."""
    from oracle import tdeed_oracle as O
    from tdeed_amd.trainer import TrainEngine
    cfg = CFG5
    B, T, H, W = 1, 250, 64, 64
    sd0 = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 23).items()}
    frames = t(synth.uint8_clip(711, (B, T, 3, H, W)))
    lab_np, labD_np = synth.labels(712, B, T, cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.2)
    lab, labD = t(lab_np).long(), t(labD_np).float()
    par = [k for k in sd0 if state_layout.is_parameter(k)]
    sdr = {k: (v.clone().requires_grad_(True) if k in par else v.clone()) for k, v in sd0.items()}
    ref, cls_ref, _ = _oracle_train_loss(O, frames, sdr, cfg, regnet_spec(cfg["feature_arch"]), lab, labD)
    ref.backward()
    eng = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=1e-4)
    loss, grads = eng.loss_and_grads(frames.to(DEV), lab.to(DEV), labD.to(DEV))
    torch.cuda.synchronize()
    assert set(grads) == set(par)
    assert abs(float(loss[0]) - float(ref.detach())) < 5e-4 * max(1.0, abs(float(ref.detach())))
    ga = torch.cat([grads[k].detach().cpu().double().reshape(-1) for k in par])
    gr = torch.cat([sdr[k].grad.double().reshape(-1) for k in par])
    gn = float(gr.norm())
    assert float((ga - gr).norm()) / gn < 5e-3
    worst = max(((float((grads[k].detach().cpu().double() - sdr[k].grad.double()).norm())
                  - 3e-2 * float(sdr[k].grad.double().norm())) / gn, k) for k in par)
    assert worst[0] <= 2e-4, worst
    # the gate-shift tensors on their own (the part that is new at T=250): relative error per site
    for k in par:
        if ".gs." in k and float(sdr[k].grad.double().norm()) > 1e-4 * gn:
            a, b = grads[k].detach().cpu().double(), sdr[k].grad.double()
            assert float((a - b).norm()) <= 2e-2 * float(b.norm()) + 1e-5 * gn, k
    # one optimisation step through the captured graph at this geometry reproduces the eager step bit for bit
    eng_a = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=1e-4)
    eng_b = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=1e-4)
    fr, lb, ld = frames.to(DEV), lab.to(DEV), labD.to(DEV)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        eng_a.step(fr, lb, ld)
        step = eng_b.make_step(B, H, W, fr, lb, ld, None, use_graph=True)
        step()
        st.synchronize()
    assert torch.equal(eng_a.params.grad, eng_b.params.grad)
    assert torch.equal(eng_a.params.flat, eng_b.params.flat)


@pytest.mark.parametrize("name", ["cfg3_b16", "cfg5_t250_b4"])
def test_full_size_bf16_step_eager_equals_graph_and_tracks_fp32(name):
    """BASELINE configs[2] as it is benchmarked (800MF, n_layers=3, L=100, 224x224, B=16, bf16) and configs[4]'s per-GPU share
    at its real size (SoccerNetBall hyper-parameters, T=250, 224x224, B=4): the captured step gives
    the same loss and the same temporal-stack / head gradients as the eager step on the same clips (bitwise: no float
    atomics anywhere), and the bf16 loss lies within 5 % of the fp32 engine's loss on those clips.  No oracle at this size
    (an autograd pass over 16 clips of 800MF takes minutes on the host)."""
    from tdeed_amd.trainer import TrainEngine
    cfg, B = (CFG3, 16) if name == "cfg3_b16" else (CFG5, 4)
    T, H, W = cfg["clip_len"], 224, 224
    from tdeed_amd import ops
    sd0 = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 0).items()}
    frames = ops.fill_u8_hash((B, T, 3, H, W), 1000, DEV)
    lab_np, labD_np = synth.labels(5, B, T, cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.1)
    lab, labD = t(lab_np).to(DEV), t(labD_np).float().to(DEV)
    C = regnet_spec(cfg["feature_arch"]).feat_dim
    gen = torch.Generator(device="cpu").manual_seed(3)
    masks = [((torch.rand((B, T, C), generator=gen) >= 0.5).to(torch.bfloat16) * 2.0).to(DEV) for _ in range(2)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        e1 = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.bfloat16, lr=1e-4)
        loss_e = e1.accumulate(frames, lab, labD, drop_masks=masks).clone()
        g_e = e1.params.grad.clone()
        e2 = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.bfloat16, lr=1e-4)
        h = e2.build_graph(B, H, W)
        loss_g = e2.step_graph(h, frames, lab, labD, drop_masks=masks).clone()
        st.synchronize()
        g_g = e2.params.grad.clone()
        lo = min(o for k, (o, n) in e1.params.index.items() if k.startswith(("_temp_fine.", "_pred_")))
        assert torch.isfinite(g_e).all() and torch.isfinite(loss_e).all()
        assert torch.equal(loss_e, loss_g)
        assert torch.equal(g_e[lo:], g_g[lo:])                       # _temp_fine.* and head gradients
        assert torch.equal(g_e[:lo], g_g[:lo])                       # ... and the trunk's
        del e2, h
        torch.cuda.empty_cache()
        # fp32 engine on the same clips (masks in fp32)
        e3 = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=1e-4)
        loss32 = e3.accumulate(frames, lab, labD, drop_masks=[m.float() for m in masks]).clone()
        st.synchronize()
        g32 = e3.params.grad
        assert abs(float(loss_e[0]) - float(loss32[0])) < 5e-2 * max(1.0, abs(float(loss32[0]))), (loss_e, loss32)
        # gradient direction of the temporal stack + heads (92 % of the parameters) against the fp32 engine
        a, b = g_e[lo:].double(), g32[lo:].double()
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        assert cos > 0.9 and 0.7 < float(a.norm() / b.norm()) < 1.4, cos


def _tiny_batch(cfg, seed, B, H, W):
    T = cfg["clip_len"]
    frames = t(synth.uint8_clip(seed, (B, T, 3, H, W))).to(DEV)
    lab, labD = synth.labels(seed + 1, B, T, cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.4)
    return frames, t(lab).to(DEV), t(labD).float().to(DEV)


def test_captured_training_graphs_survive_eager_steps_and_each_other():
    """ADVICE r2 (ops_bwd.PinnedTables): the gradient write-out launches of a captured step read their record tables from
    pinned host memory at every replay.  (a) build_graph, five eager steps (more than the eager table ring is deep), then a
    replay must still write this graph's gradients; (b) two graphs of different batch geometries on ONE engine must each
    keep folding their own buffers."""
    from tdeed_amd.trainer import TrainEngine
    cfg = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
               radi_displacement=2)
    sd0 = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 61).items()}
    fa, la, da = _tiny_batch(cfg, 2100, 2, 64, 64)
    fb, lb, db = _tiny_batch(cfg, 2200, 3, 48, 80)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        # reference gradients of both batches from a fresh engine (no optimizer step in between: accumulate only)
        ref = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=0.0)
        ref.accumulate(fa, la, da)
        ga = ref.params.grad.clone()
        ref.accumulate(fb, lb, db)
        gb = ref.params.grad.clone()
        st.synchronize()
        eng = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=0.0)
        eng.opt.wd = 0.0                                              # lr 0, no decay: the weights never move
        ha = eng.build_graph(2, 64, 64)
        hb = eng.build_graph(3, 48, 80)
        assert ha.keep is not hb.keep
        for _ in range(5):                                           # eager steps cycle the engine's own table ring
            eng.accumulate(fb, lb, db)
        eng.step_graph(ha, fa, la, da)
        st.synchronize()
        assert torch.equal(eng.params.grad, ga)
        eng.step_graph(hb, fb, lb, db)
        st.synchronize()
        assert torch.equal(eng.params.grad, gb)
        eng.accumulate(fa, la, da)
        eng.step_graph(ha, fa, la, da)                               # first graph again, after the second one and an eager step
        st.synchronize()
        assert torch.equal(eng.params.grad, ga)


def test_apply_reduces_gradients_that_were_accumulated_without_reduce():
    """ADVICE r2 (trainer.apply): with a reducer attached, accumulate(reduce=False) followed by apply() must not scale
    un-reduced gradients by 1/world -- it reduces them first.  World 1 stand-in reducer that records what it was asked."""
    from tdeed_amd.trainer import TrainEngine
    cfg = dict(feature_arch="rny002_gsf", clip_len=4, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
               radi_displacement=2)
    sd0 = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 62).items()}
    fa, la, da = _tiny_batch(cfg, 2300, 2, 64, 64)

    class FakeReducer:
        scale, world, backend, capturable = 0.5, 2, "torch", False

        def __init__(self, flat, buckets):
            self.flat, self.buckets, self.calls = flat, buckets, []

        def reduce_bucket(self, i):
            lo, hi = self.buckets[i]
            self.flat[lo:hi].mul_(2.0)                               # "sum over two ranks holding the same gradients"
            self.calls.append(i)

        def reduce_all(self):
            for i in range(len(self.buckets)):
                self.reduce_bucket(i)

        def join(self):
            self.calls.append("join")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=1e-3)
        b = TrainEngine(cfg, {k: v.clone() for k, v in sd0.items()}, act_dtype=torch.float32, lr=1e-3)
        a.step(fa, la, da)                                           # single process
        b.reducer = FakeReducer(b.params.grad, b.grad_buckets())
        b.accumulate(fa, la, da)                                     # reduce=False
        b.apply()
        st.synchronize()
        assert b.reducer.calls == [0, 1, "join"]
        assert torch.allclose(a.params.flat, b.params.flat, rtol=0, atol=1e-7)
        b.reducer.calls.clear()
        b.accumulate(fa, la, da, reduce=True)
        b.apply()
        st.synchronize()
        assert b.reducer.calls == [0, 1, "join"]                    # reduced inside the backward, not a second time


@pytest.mark.parametrize("M,K,N,hw", [(70000 - 70000 % 196, 320, 320, 196), (60025, 320, 768, 49), (61152, 368, 368, 49)])
def test_sliced_weight_stationary_contraction_of_the_wide_layers(M, K, N, hw):
    """gemm_ws with W cut into equal column slices (8 waves per workgroup; what engine.DenseW picks for the 320-wide layers of
    RegNetY-800MF above engine.WS_WIDE_MIN_ROWS rows) against the tiled contraction on the same operands: bitwise, with every operand feature
    of a bottleneck's conv1 / conv3 (gate-shift splice, SE re-scale, residual, second compact output)."""
    from tdeed_amd import ops
    from tdeed_amd.engine import pack_ws_weights, DenseW
    assert ops.gemm_ws_fits_mode(K, N, torch.bfloat16) == 2
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    A0 = torch.randn(M, 80, generator=g).to(torch.bfloat16).to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    sc, sh = (torch.rand(N, generator=g) + 0.5).to(DEV), (torch.randn(N, generator=g) * 0.1).to(DEV)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    gate = torch.rand(M // hw, K, generator=g).to(DEV)
    Wd, Wf = W.to(DEV), pack_ws_weights(W.float().numpy(), torch.bfloat16, DEV)
    for kw in (dict(), dict(A0=A0, k0=80), dict(residual=res, a_scale=gate, a_scale_rows=hw)):
        o2a = torch.empty((M, 32), dtype=torch.bfloat16, device=DEV)
        o2b = torch.empty_like(o2a)
        ref = ops.gemm(A, Wd, sc, sh, ops.ACT_RELU, out2=o2a, **kw)
        got = ops.gemm_ws(A, Wf, K, N, sc, sh, ops.ACT_RELU, out2=o2b, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref) and torch.equal(o2a, o2b), kw.keys()
    from tdeed_amd import engine
    d = DenseW(W.float().numpy(), torch.bfloat16, DEV)
    assert d.kern(engine.WS_WIDE_MIN_ROWS) == "gemm_ws" and d.kern(1000) == "gemm"
    old, engine.WS_WIDE_MIN_ROWS = engine.WS_WIDE_MIN_ROWS, 1000
    try:
        assert torch.equal(d.run(A, sc, sh, ops.ACT_RELU, M=M), ops.gemm(A, Wd, sc, sh, ops.ACT_RELU))
    finally:
        engine.WS_WIDE_MIN_ROWS = old


# ------------------------------------------------------------------------------------ whole bottleneck in one launch
@pytest.mark.parametrize("h,w,C,gw,R,Fp,N", [(7, 7, 368, 8, 92, 96, 37), (14, 14, 152, 8, 38, 40, 5), (7, 7, 152, 8, 38, 0, 6),
                                              (7, 7, 368, 16, 38, 0, 4), (5, 5, 368, 8, 92, 96, 3), (13, 7, 368, 8, 92, 96, 3),
                                              (10, 10, 152, 8, 38, 40, 2)])
def test_one_launch_bottleneck_equals_the_launch_per_layer_chain(h, w, C, gw, R, Fp, N):
    """tdeed_bneck_fwd (conv1 + gate-shift splice -> grouped 3x3 -> SE -> conv3 + shortcut, a workgroup's frames resident in
    LDS) against the four launches it replaces on the same operands -- bitwise, including the compact second output -- and
    against the block in torch fp32 (timm Bottleneck.forward with the splice of shift.py:89-93)."""
    import torch.nn.functional as Fn
    from tdeed_amd import ops
    from tdeed_amd.engine import pack_mfma_frags, pack_gconv_frags, pack_se_mfma
    assert ops.bneck_fits(h, w, C, R)
    g = torch.Generator().manual_seed(h * 100 + C + R + Fp)
    hw = h * w
    M = N * hw
    x = torch.relu(torch.randn(N, h, w, C, generator=g)).to(torch.bfloat16)
    G = torch.randn(M, Fp, generator=g).to(torch.bfloat16) if Fp else None
    W1 = torch.randn(C, C, generator=g) / C ** 0.5
    W3 = torch.randn(C, C, generator=g) / C ** 0.5
    W2 = torch.randn(C, gw, 3, 3, generator=g) / (gw * 9) ** 0.5
    fc1 = torch.randn(R, C, generator=g) / C ** 0.5
    fc2 = torch.randn(C, R, generator=g) / R ** 0.5
    vec = lambda n, s=0.1, o=0.0: (torch.randn(n, generator=g) * s + o).to(DEV)          # noqa: E731
    s1, h1, s2, h2, s3, h3 = vec(C, 0.1, 1.0), vec(C), vec(C, 0.1, 1.0), vec(C), vec(C, 0.1, 0.5), vec(C)
    b1, b2 = vec(R), vec(C)
    bf = lambda t: t.to(torch.bfloat16)                                                     # noqa: E731
    W1d, W3d = bf(W1).to(DEV), bf(W3).to(DEV)
    w2f = pack_gconv_frags(W2.numpy(), gw, DEV)
    se = pack_se_mfma(fc1.numpy(), fc2.numpy(), DEV)
    xd, Gd = x.to(DEV), (G.to(DEV) if Fp else None)
    # the chain
    y1 = ops.gemm(xd.view(M, C), W1d, s1, h1, ops.ACT_RELU, **(dict(A0=Gd, k0=Fp) if Fp else {}))
    y2, pooled = ops.gconv3x3(y1.view(N, h, w, C), None, s2, h2, gw, 1, wfrag=w2f)
    gate = ops.se_gate_mfma(pooled, 1.0 / hw, se["w1f"], b1, se["w2f"], b2, R)
    n2 = 48
    ref2 = torch.empty((M, n2), dtype=torch.bfloat16, device=DEV)
    ref = ops.gemm(y2.view(M, C), W3d, s3, h3, ops.ACT_RELU, residual=xd.view(M, C), a_scale=gate, a_scale_rows=hw, out2=ref2)
    # one launch
    out2 = torch.empty_like(ref2)
    out = ops.bneck(xd, pack_mfma_frags(W1.numpy(), DEV), s1, h1, pack_gconv_frags(W2.numpy(), gw, DEV, tap_major=(gw == 8)), s2, h2,
                    se["w1f"], b1, se["w2f"], b2, R,
                    pack_mfma_frags(W3.numpy(), DEV), s3, h3, G=Gd, out2=out2, w2_tap_major=(gw == 8))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out.view(M, C), ref), float((out.view(M, C).float() - ref.float()).abs().max())
    assert torch.equal(out2, ref2)
    # torch fp32 on the bf16-rounded weights
    xin = x.float().view(M, C).clone()
    if Fp:
        xin[:, :Fp] = G.float()
    t1 = torch.relu(xin @ bf(W1).float().t() * s1.cpu() + h1.cpu()).to(torch.bfloat16).float()
    t2 = Fn.conv2d(t1.view(N, h, w, C).permute(0, 3, 1, 2), bf(W2).float(), None, 1, 1, 1, C // gw)
    t2 = torch.relu(t2 * s2.cpu()[None, :, None, None] + h2.cpu()[None, :, None, None]).to(torch.bfloat16).float()
    gt = torch.sigmoid(torch.relu(t2.mean((2, 3)) @ bf(fc1).float().t() + b1.cpu()) @ bf(fc2).float().t() + b2.cpu())
    t3 = (t2 * gt[:, :, None, None]).permute(0, 2, 3, 1).reshape(M, C).to(torch.bfloat16).float()
    want = torch.relu(t3 @ bf(W3).float().t() * s3.cpu() + h3.cpu() + x.float().view(M, C))
    err = (out.view(M, C).float().cpu() - want).abs().max() / want.abs().max()
    assert float(err) < 2e-2, float(err)


def test_debug_flavour_runs_the_hot_path_without_a_trap(tmp_path):
    """The asserting build (TDEED_LIB_FLAVOUR=debug: LDS offsets and table indices checked on the device) runs a small
    forward through the one-launch bottleneck, the SGP stage and the heads in a child process, and agrees with the release
    library on the logits."""
    import importlib.util
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_tdeed_build_dbg", os.path.join(root, "t-deed_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(flavour="debug", verbose=False)
    code = (
        "import sys, torch; sys.path.insert(0, %r)\n"
        "import tdeed_amd\n"
        "from tdeed_amd import synth, state_layout, _lib\n"
        "from tdeed_amd.engine import ForwardEngine\n"
        "assert _lib.load()._name.endswith(sys.argv[1]), _lib.load()._name\n"
        "cfg = dict(feature_arch='rny002_gsf', clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3, radi_displacement=2)\n"
        "sd = synth.make_state(state_layout.model_state_shapes(cfg), 0)\n"
        "clip = torch.from_numpy(synth.uint8_clip(5, (2, 8, 3, 224, 224))).cuda()\n"
        "st = torch.cuda.Stream()\n"
        "with torch.cuda.stream(st):\n"
        "    eng = ForwardEngine(cfg, sd, torch.bfloat16, 'cuda', use_graph=False)\n"
        "    plan = eng.plan(2, 224, 224)\n"
        "    assert any(s.kernel == 'bneck' for s in plan.steps)\n"
        "    out, _ = eng.forward(clip)\n"
        "    st.synchronize()\n"
        "torch.save(out.cpu(), sys.argv[2])\n" % root)
    outs = []
    for flav, suffix in (("debug", "libtdeed_hip_dbg.so"), ("release", "libtdeed_hip.so")):
        path = str(tmp_path / f"tdeed_flavour_{flav}.pt")
        env = dict(os.environ, TDEED_LIB_FLAVOUR=flav)
        r = subprocess.run([sys.executable, "-c", code, suffix, path], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (flav, r.stdout[-2000:], r.stderr[-2000:])
        outs.append(torch.load(path))
    assert torch.isfinite(outs[0]).all()
    # -O1 contracts floating point differently from -O3; in bf16 that moves logits by the usual bf16 noise
    assert float((outs[0] - outs[1]).abs().max()) < 0.1 * float(outs[1].abs().max())


@pytest.mark.parametrize("H,W,Cin,C,gw,stride,Fp,N", [(56, 56, 24, 56, 8, 2, 0, 3), (28, 28, 56, 152, 8, 2, 16, 4),
                                                       (20, 12, 32, 64, 16, 1, 8, 2), (28, 28, 64, 152, 8, 2, 0, 2),
                                                       (14, 14, 152, 368, 8, 2, 40, 3), (28, 28, 128, 320, 16, 2, 32, 2),
                                                       (15, 13, 24, 56, 8, 2, 0, 2)])
def test_conv1_in_front_of_the_grouped_conv_equals_the_two_launches(H, W, Cin, C, gw, stride, Fp, N):
    """tdeed_c1_gconv_fwd (the y1 band computed in LDS from the block input) against conv1 (tdeed_gemm_fwd with the gate-shift
    splice) followed by tdeed_gconv3x3_fwd: output rows and squeeze partial sums bitwise."""
    from tdeed_amd import ops
    from tdeed_amd.engine import pack_mfma_frags, pack_gconv_frags
    assert ops.c1_gconv_fits(H, W, Cin, C, stride)
    g = torch.Generator().manual_seed(H * 10 + C)
    M = N * H * W
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g)).to(torch.bfloat16).to(DEV)
    G = torch.randn(M, Fp, generator=g).to(torch.bfloat16).to(DEV) if Fp else None
    W1 = torch.randn(C, Cin, generator=g) / Cin ** 0.5
    W2 = torch.randn(C, gw, 3, 3, generator=g) / (gw * 9) ** 0.5
    vec = lambda n, s=0.1, o=0.0: (torch.randn(n, generator=g) * s + o).to(DEV)          # noqa: E731
    s1, h1, s2, h2 = vec(C, 0.1, 1.0), vec(C), vec(C, 0.1, 1.0), vec(C)
    w2f = pack_gconv_frags(W2.numpy(), gw, DEV)
    y1 = ops.gemm(x.view(M, Cin), W1.to(torch.bfloat16).to(DEV), s1, h1, ops.ACT_RELU, **(dict(A0=G, k0=Fp) if Fp else {}))
    ref, pref = ops.gconv3x3(y1.view(N, H, W, C), None, s2, h2, gw, stride, wfrag=w2f)
    tiles = ops.c1_gconv_slab_tiles(H, W, C, stride)
    w1f = pack_mfma_frags(W1.numpy(), DEV, rows=tiles * 16)
    out, pooled = ops.c1_gconv(x, w1f, s1, h1, w2f, s2, h2, gw, stride, C, G=G)
    torch.cuda.synchronize()
    assert torch.equal(out, ref), float((out.float() - ref.float()).abs().max())
    assert torch.equal(pooled, pref)


@pytest.mark.parametrize("M", [196 * 7, 196 * 40 + 0, 64 * 3 + 17])
def test_register_stationary_contraction_equals_the_tiled_one(M):
    """tdeed_gemm_rs_fwd (K = N = 320: the whole W in the registers of a 10-wave workgroup, 64-row activation tiles through
    LDS) against tdeed_gemm_fwd on the same operands, bitwise: plain, with the gate-shift splice, and as conv3 (SE re-scale,
    residual, ReLU, second compact output)."""
    from tdeed_amd import ops
    from tdeed_amd.engine import pack_ws_weights
    K = N = 320
    hw = 196
    assert ops.gemm_rs_fits(M, K, N)
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    A0 = torch.randn(M, 80, generator=g).to(torch.bfloat16).to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    sc, sh = (torch.rand(N, generator=g) + 0.5).to(DEV), (torch.randn(N, generator=g) * 0.1).to(DEV)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    gate = torch.rand((M + hw - 1) // hw, K, generator=g).to(DEV)
    Wd, Wf = W.to(DEV), pack_ws_weights(W.float().numpy(), torch.bfloat16, DEV)
    for kw in (dict(), dict(A0=A0, k0=80), dict(residual=res, a_scale=gate, a_scale_rows=hw)):
        o2a = torch.empty((M, 80), dtype=torch.bfloat16, device=DEV)
        o2b = torch.empty_like(o2a)
        ref = ops.gemm(A, Wd, sc, sh, ops.ACT_RELU, out2=o2a, **kw)
        got = ops.gemm_rs(A, Wf, K, N, sc, sh, ops.ACT_RELU, out2=o2b, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref) and torch.equal(o2a, o2b), (list(kw), float((got.float() - ref.float()).abs().max()))


@pytest.mark.parametrize("env", [{"TDEED_FRONT_ROLL": "5"}, {"TDEED_FRONT_PIPE": "0"}, {"TDEED_FRONT_PIPE": "0", "TDEED_FRONT_ROLL": "3"},
                                 {"TDEED_FRONT_ROLL": "0"}])
def test_s1_front_forms_agree(env):
    """The three forms of the stage-1 front launch (row bands, rolling strips, pipelined strips) are selected per process:
    each passes the same fused-vs-unfused comparison, at strip heights that leave ragged last strips."""
    import subprocess
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(os.path.dirname(__file__), "test_gpu_ops.py"), "-q", "-m", "gpu",
                        "-k", "s1_front", "-p", "no:cacheprovider"], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "8 passed" in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("flags", [[], ["--cu-mask", "interleave", "--inflight", "4"]])
def test_bench_line_contract(flags):
    """`bench.py --full` prints ONE JSON line with the contract's fields and the roofline (short run, the long side
    measurements off); the same with every in-flight batch's stream confined to its own XCDs (`--cu-mask`)."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "2", "--repeats", "1", "--full",
                        "--no-train", "--no-feed", "--no-cpu-baseline", *flags], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["config"]["workload"].startswith("rny002_b8") and d["dtype"] == "bf16" and d["data"] == "synthetic"
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert abs(d["value"] - d["config"]["clips_per_gpu"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert d["timed_output_check"]["finite"] is True and d["latency_ms_inflight1"] > 0


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` without `--full`: ONE JSON line with the contract's fields, computed from the
    timed regions alone -- none of the side measurements or checks of `--full` has run -- and `--dump-outputs` still writes
    the last timed step's logits.  The run spends at most 30 s outside its steps."""
    import json
    import subprocess
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900, cwd=root)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "clips/s" and d["dtype"] == "bf16" and d["config"]["workload"].startswith("rny002_b8")
    assert abs(d["value"] - d["config"]["clips_per_gpu"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    for k in ("timed_output_check", "latency_ms_inflight1", "fed_from_host", "roofline_step", "roofline_sgp", "infer_800mf",
              "infer_snb_t250", "train", "logit_max_abs_err_bf16"):
        assert k not in d, k
    assert d.get("roofline") is None and d.get("cpu_baseline") is None
    # the whole process, start to exit, less its warm-up and timed steps: at most 30 s (measured: under 3 s)
    outside = wall - (4 + 2) * d["ms_per_step"] * 1e-3
    print(f"plain bench run: {wall:.2f} s in all, {outside:.2f} s outside its steps")
    assert outside <= 30.0, outside
    h = np.load(os.path.join(str(tmp_path), "head_out.npy"))
    assert h.shape[:2] == (8, 100) and h.dtype == np.float32 and np.isfinite(h).all()
