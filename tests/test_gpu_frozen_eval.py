"""The frozen eval-mode prefix of the trunk on the MI355X (`set_groups(..., frozen_stats='eval')`): loss and gradients of the
step against autograd on the CPU oracle composed per stage (eval mode inside the prefix, train mode behind it), what a step
leaves in the buffers, block k's input map, eager against captured, which scopes launch, the bf16 engine, a tiny epoch
through TDEEDModel, and the eval instance of the MFMA stem alone against its rounding bound.  -m gpu only; `pytest -s`
prints every figure.  The cases and their references: tests/frozen_eval_cases.py."""
import collections
import functools
import random

import pytest
import torch

import frozen_eval_cases as C
import roundoff as R
from helpers import Guarded, cfg_ns, drop_masks, max_abs
from tdeed_amd import state_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CASES = [(p, g) for p in C.PREFIXES for g in C.GEOMS]


def _engine(prefix=None, frozen_stats="eval", dtype=torch.float32):
    from tdeed_amd.trainer import TrainEngine
    eng = TrainEngine(C.CFG, C.start_state(), act_dtype=dtype, device=DEV, lr=1e-3)
    if prefix is not None:
        eng.set_groups(C.groups(prefix), frozen_stats=frozen_stats)
    return eng


def _inputs(geom, rank=0):
    frames, lab, labD = (x.to(DEV) for x in C.batch(geom, rank))
    _, _, crop, flips = C.GEOMS[geom]
    flip = torch.tensor(flips, dtype=torch.bool, device=DEV) if flips else False
    return frames, lab, labD, crop, flip


def _masks(dtype=torch.float32):
    return [m.to(DEV).to(dtype) for m in C.masks()]


def _buffers(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.state.items() if not state_layout.is_parameter(k)}


def _prefix_stage(eng, key):
    from tdeed_amd.optim import stage_of
    return key.startswith("_features.") and stage_of(key) in eng.eval_prefix


@functools.lru_cache(maxsize=None)
def _run(prefix, geom):
    """One fp32 engine per case, everything measured once and left unchanged: block k's input map, loss and gradients of
    loss_and_grads, then (buffers put back to the start state) one eager step under the scope profile."""
    from tdeed_amd import _lib
    eng = _engine(prefix)
    frames, lab, labD, crop, flip = _inputs(geom)
    fr = frames.reshape(-1, *frames.shape[2:])
    cut = eng.prefix.run(fr, crop, eng._frame_flip(flip, *frames.shape[:2])).float().cpu()
    start_flat, start_buf = eng.params.flat.cpu(), _buffers(eng)
    loss, grads = eng.loss_and_grads(frames, lab, labD, crop=crop, flip=flip, drop_masks=_masks())
    torch.cuda.synchronize()
    out = dict(cut=cut, loss=float(loss[0]), grads={k: g.detach().cpu() for k, g in grads.items()},
               eval_prefix=eng.eval_prefix, frozen=eng.frozen)
    for k, v in start_buf.items():
        eng.state[k].copy_(v)
    with _lib.profile() as prof:
        eng.step(frames, lab, labD, crop=crop, flip=flip, drop_masks=_masks())
    torch.cuda.synchronize()
    out.update(start_flat=start_flat, start_buf=start_buf, flat=eng.params.flat.cpu(), buf=_buffers(eng),
               index=dict(eng.params.index), prefix_keys={k for k in eng.state if _prefix_stage(eng, k)},
               calls=collections.Counter(rec[4] for rec in prof.rec))
    return out


def _calls(prefix, frozen_stats, dtype):
    """launches per scope (and per scope and entry point) of one eager step on the 64 x 64 batch"""
    from tdeed_amd import _lib
    eng = _engine(prefix, frozen_stats=frozen_stats, dtype=dtype)
    frames, lab, labD, crop, flip = _inputs("full")
    with _lib.profile() as prof:
        eng.step(frames, lab, labD, crop=crop, flip=flip, drop_masks=_masks(dtype))
    torch.cuda.synchronize()
    assert (eng.prefix is None) == (frozen_stats == "batch")
    return (collections.Counter(rec[4] for rec in prof.rec), collections.Counter((rec[4], rec[0]) for rec in prof.rec),
            eng.eval_prefix)


@functools.lru_cache(maxsize=None)
def _batch_calls(prefix, dtype=torch.float32):
    """... with the same freeze set under 'batch' (today's forward)"""
    return _calls(prefix, "batch", dtype)[:2]


# ----------------------------------------------------------------------------- 1. loss and gradients against autograd
@pytest.mark.parametrize("prefix,geom", CASES)
def test_fp32_step_matches_autograd(prefix, geom):
    """Bounds of test_gpu_r2.py::test_cfg3_full_length_800mf_train_step_matches_autograd: loss 5e-4 relative, the whole
    gradient 5e-3 of its norm, per tensor (|diff| - 3e-2 |ref|) / |whole| <= 2e-4."""
    got, ref = _run(prefix, geom), C.reference(prefix, geom)
    par = ref["train"]
    assert set(got["grads"]) == set(par) and len(par) > 50
    assert got["eval_prefix"] and len(got["eval_prefix"]) == C.n_eval_stages(prefix)
    rel = abs(got["loss"] - ref["loss"]) / max(1.0, abs(ref["loss"]))
    ga = torch.cat([got["grads"][k].double().reshape(-1) for k in par])
    gr = torch.cat([ref["grads"][k].double().reshape(-1) for k in par])
    gn = float(gr.norm())
    whole = float((ga - gr).norm()) / gn
    worst = max(((float((got["grads"][k].double().reshape(-1) - ref["grads"][k].double().reshape(-1)).norm())
                  - 3e-2 * float(ref["grads"][k].double().norm())) / gn, k) for k in par)
    print(f"[frozen_eval] {prefix} {geom}: loss {got['loss']:.6f} ref {ref['loss']:.6f} rel {rel:.2e}; gradient {whole:.2e} "
          f"of its norm; worst tensor {worst[0]:.2e} {worst[1]}")
    assert rel < 5e-4
    assert whole < 5e-3
    assert worst[0] <= 2e-4, worst


# ----------------------------------------------------------------------------- 2. what one step leaves behind
@pytest.mark.parametrize("prefix,geom", CASES)
def test_buffers_after_one_step(prefix, geom):
    got, ref = _run(prefix, geom), C.reference(prefix, geom)
    moved = 0
    for k, (o, n) in got["index"].items():
        if k in got["frozen"]:
            assert torch.equal(got["flat"][o:o + n], got["start_flat"][o:o + n]), k
        else:
            moved += int(not torch.equal(got["flat"][o:o + n], got["start_flat"][o:o + n]))
    assert moved > 0.9 * (len(got["index"]) - len(got["frozen"]))
    n_prefix = n_behind = 0
    for k, v in got["buf"].items():
        if k in got["prefix_keys"]:
            assert torch.equal(v, got["start_buf"][k]), k        # running statistics and step counters of the prefix: bits
            assert k not in ref["bn"], k
            n_prefix += 1
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(got["start_buf"][k]) + 1 == int(ref["bn"][k]), k
        else:
            want = ref["bn"][k].double()
            err = float((v.double() - want).abs().max() / want.abs().max().clamp_min(1e-6))
            assert err < 1e-4, (k, err)                          # (tests/test_gpu_bwd.py rel_err and its bound)
            assert not torch.equal(v, got["start_buf"][k]), k
            n_behind += 1
    assert n_prefix >= 3 and n_prefix + n_behind + len([k for k in ref["bn"] if k.endswith("tracked")]) == len(got["buf"])
    assert (n_behind == 0) == (prefix == "trunk")


# ----------------------------------------------------------------------------- 3. block k's input map
@pytest.mark.parametrize("prefix,geom", CASES)
def test_block_k_input_map(prefix, geom):
    got, ref = _run(prefix, geom), C.reference(prefix, geom)
    want = ref["cut"]
    assert tuple(got["cut"].shape) == tuple(want.shape)
    err, bound = max_abs(got["cut"], want), 2e-3 * max(1.0, float(want.abs().max()))
    print(f"[frozen_eval] {prefix} {geom}: map {tuple(want.shape)} max|err| {err:.3e} bound {bound:.3e}")
    assert err < bound
    assert float(want.abs().max()) > 0.1


# ----------------------------------------------------------------------------- 4. eager == captured
def _two_steps(eng, graph):
    losses = []
    for rank in (0, 1):
        frames, lab, labD, _, _ = _inputs("full", rank)
        if graph:
            step = eng.make_step(C.B, 64, 64, frames, lab, labD, _masks(), use_graph=True)
        else:
            step = eng.make_step(C.B, 64, 64, frames, lab, labD, _masks(), use_graph=False)
        losses.append(step().clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), eng.params.grad.cpu(), eng.params.flat.cpu()


@pytest.mark.parametrize("prefix", ["s2", "trunk"])
def test_eager_step_equals_captured_step(prefix):
    eager = _two_steps(_engine(prefix), False)
    eng = _engine(prefix)
    captured = _two_steps(eng, True)
    for a, b, what in zip(eager, captured, ("loss", "gradient buffer", "parameters")):
        assert torch.equal(a, b), what
    assert eng.last_graph is not None and eng.last_graph.prefix[0] == eng.eval_prefix
    assert not torch.equal(captured[2], _engine(prefix).params.flat.cpu())


def test_a_graph_belongs_to_its_eval_prefix():
    eng = _engine("s2", frozen_stats="batch")
    frames, lab, labD, _, _ = _inputs("full")
    step = eng.make_step(C.B, 64, 64, frames, lab, labD, None, use_graph=True)
    h_batch = eng.last_graph
    step()
    eng.set_groups(C.groups("s2"), frozen_stats="eval")          # the same freeze set, another forward
    assert eng.last_graph is None
    with pytest.raises(RuntimeError, match="eval prefix"):
        eng.step_graph(h_batch, frames, lab, labD)
    step_e = eng.make_step(C.B, 64, 64, frames, lab, labD, None, use_graph=True)
    h_eval = eng.last_graph
    assert h_eval is not h_batch and h_eval.prefix == (eng.eval_prefix, eng.prefix_gen)
    step_e()
    assert eng.make_step(C.B, 64, 64, frames, lab, labD, None, use_graph=True) is not None and eng.last_graph is h_eval
    eng.set_groups(C.groups("s2"), frozen_stats="batch")
    with pytest.raises(RuntimeError, match="eval prefix"):
        eng.step_graph(h_eval, frames, lab, labD)
    with pytest.raises(RuntimeError, match="eval prefix"):
        step_e()
    eng.set_groups(C.groups("s2"), frozen_stats="eval")
    eng.make_step(C.B, 64, 64, frames, lab, labD, None, use_graph=True)()
    h2 = eng.last_graph
    eng.reload_prefix()                                          # what load() / load_state_dict do: new packed copies
    with pytest.raises(RuntimeError, match="rebuilt"):
        eng.step_graph(h2, frames, lab, labD)
    eng.make_step(C.B, 64, 64, frames, lab, labD, None, use_graph=True)()
    torch.cuda.synchronize()
    assert eng.last_graph is not h2
    with pytest.raises(ValueError, match="empty eval prefix"):
        eng.set_groups([{"params": ("_features.s1.*",), "frozen": True}], frozen_stats="eval")
    with pytest.raises(ValueError, match="frozen_stats"):
        eng.set_groups(C.groups("s2"), frozen_stats="running")


# ----------------------------------------------------------------------------- 5. launch census
def _first_behind(stages):
    """the first block behind the prefix (None: the prefix is the whole trunk)"""
    from tdeed_amd.regnet_spec import regnet_spec
    blocks = regnet_spec(C.CFG["feature_arch"]).blocks
    return blocks[len(stages) - 1] if len(stages) - 1 < len(blocks) else None


def _census(prefix, got, stages, batch, batch_by_entry, got_by_entry, slice_written_by_producer):
    """No launch under a prefix stage's scopes, launches under prefix.fwd, and behind the prefix the same scopes as under
    'batch' with the same number of launches in EVERY one of them -- with one stated exception: where the train-mode
    producer of a gate-shift block's input writes that block's compact slice along (bf16: tdeed_bn_apply_slice), the first
    block behind the prefix, handed xs=None, launches exactly one tdeed_gsf_slice more in its .fwd scope."""
    own = {s + sfx for s in stages for sfx in (".fwd", ".bwd")}
    assert not own & set(got), own & set(got)
    assert got["prefix.fwd"] > 0 and "prefix.fwd" not in batch
    assert own & set(batch) == {s + ".fwd" for s in stages}       # 'batch' does run their forward (and no backward)
    behind = set(batch) - own
    assert set(got) - {"prefix.fwd"} == behind
    first = _first_behind(stages)
    extra = {}
    if first is not None and first.gsf_fold > 0 and slice_written_by_producer:
        extra[first.name + ".fwd"] = 1
        key = (first.name + ".fwd", "tdeed_gsf_slice")
        assert got_by_entry[key] == batch_by_entry[key] + 1 == 1, (got_by_entry[key], batch_by_entry[key])
    for s in sorted(behind):
        assert got[s] == batch[s] + extra.get(s, 0), (prefix, s, got[s], batch[s], extra.get(s, 0))
    if first is not None:
        assert got[first.name + ".bwd"] == batch[first.name + ".bwd"] > 0
        # the same entry points, too: the first block's backward is the form it has under 'batch'
        for (scope, entry), n in batch_by_entry.items():
            if scope == first.name + ".bwd":
                assert got_by_entry[(scope, entry)] == n, (scope, entry)
    print(f"[frozen_eval] {prefix}: {got['prefix.fwd']} launches under prefix.fwd for {sum(batch[s + '.fwd'] for s in stages)} "
          f"under the stages' .fwd scopes in 'batch'; first block behind: {first.name if first is not None else None}, "
          f"extra {extra}")


@pytest.mark.parametrize("prefix", list(C.PREFIXES))
def test_launch_census(prefix):
    """fp32, the scope profile of test_trunk_frozen_launches_no_trunk_backward: no train-mode producer writes a slice (that
    needs the bf16 statistics epilogues), so every scope behind the prefix has exactly its 'batch' count."""
    run = _run(prefix, "full")
    batch, batch_by_entry = _batch_calls(prefix)
    # (per entry point: a fresh step of the same engine kind; _run's profile keeps the scope only)
    got, got_by_entry, stages = _calls(prefix, "eval", torch.float32)
    assert got == run["calls"] and stages == run["eval_prefix"]
    _census(prefix, got, stages, batch, batch_by_entry, got_by_entry, slice_written_by_producer=False)


@pytest.mark.parametrize("prefix", list(C.PREFIXES))
def test_launch_census_bf16(prefix):
    """bf16: the one stated difference -- +1 tdeed_gsf_slice in the first block's .fwd where it is a gate-shift block
    (cuts s2 and s3mid), nothing else anywhere."""
    batch, batch_by_entry = _batch_calls(prefix, BF)
    got, got_by_entry, stages = _calls(prefix, "eval", BF)
    first = _first_behind(stages)
    assert (first is not None and first.gsf_fold > 0) == (prefix in ("s2", "s3mid"))
    _census(prefix, got, stages, batch, batch_by_entry, got_by_entry, slice_written_by_producer=True)
    if prefix == "stem":
        # the stem-only prefix on plain uint8 frames has no fused front to take: the eval instance of the MFMA stem
        assert got_by_entry[("prefix.fwd", "tdeed_stem_mfma_eval_fwd")] == 1 and got["prefix.fwd"] == 1


def test_the_map_belongs_to_one_forward_and_the_plans_are_bounded(monkeypatch):
    """Block k's input map is a buffer of the prefix's plan: a second forward of the same geometry in front of the first
    one's backward is an error, not a silent gradient through the wrong batch; with the whole trunk in the prefix nothing
    re-reads the map.  Eager plans are kept for the two most recently used forms.  A capture that fails leaves no static
    plan and no note of the static buffer behind."""
    eng = _engine("s2")
    frames, lab, labD, _, _ = _inputs("full")
    frames1 = _inputs("full", 1)[0]
    head0, ctx0 = eng.forward_train(frames, drop_masks=_masks())
    head1, ctx1 = eng.forward_train(frames1, drop_masks=_masks())
    assert ctx0.pmap[1] is ctx1.pmap[1] and ctx1.pmap[2] == ctx0.pmap[2] + 1
    with pytest.raises(RuntimeError, match="overwritten"):
        eng.backward_train(ctx0, torch.ones_like(head0))
    assert set(eng.backward_train(ctx1, torch.ones_like(head1))) == set(C.reference("s2", "full")["train"])
    trunk = _engine("trunk")
    head0, ctx0 = trunk.forward_train(frames, drop_masks=_masks())
    trunk.forward_train(frames1, drop_masks=_masks())
    assert "temp_enc" in trunk.backward_train(ctx0, torch.ones_like(head0))
    # plans: no flip, per-clip flags, fp32 frames -> the first form is dropped, its map lives on in its ctx
    flags = torch.tensor([True, False], device=DEV)
    eng.forward_train(frames, flip=flags, drop_masks=_masks())
    assert len(eng.prefix._plans) == 2
    _, ctx_f = eng.forward_train(frames.float(), drop_masks=_masks())
    assert len(eng.prefix._plans) == 2 and ctx1.pmap[1] not in eng.prefix._plans.values()
    assert ctx_f.pmap[1] in eng.prefix._plans.values() and bool(torch.isfinite(ctx1.pmap[0].float()).all())
    # a failing capture
    def boom(*a, **k):
        eng.prefix.run(frames.reshape(-1, *frames.shape[2:]), None, False, static=True)
        eng._static_frames = frames
        raise RuntimeError("capture failed")
    monkeypatch.setattr(eng, "_build_graph", boom)
    with pytest.raises(RuntimeError, match="capture failed"):
        eng.build_graph(C.B, 64, 64)
    assert eng._static_frames is None and all(k[-1] is None for k in eng.prefix._plans)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 6. the bf16 engine
@pytest.mark.parametrize("prefix,geom", [(p, g) for p in ("s2", "trunk") for g in C.GEOMS])
def test_bf16_step(prefix, geom):
    """Loss within the 5e-2 relative of tests/test_gpu_r2.py:144; per trainable tensor the direction bounds of
    test_gpu_r2.py::test_bf16_train_step_per_tensor_direction, its numbers.  ('crop': per-clip flips, so the prefix takes the
    eval instance of the MFMA stem; 'full': uint8 frames without flips keep the fused front.)"""
    ref = C.reference(prefix, geom)
    eng = _engine(prefix, dtype=BF)
    frames, lab, labD, crop, flip = _inputs(geom)
    loss, grads = eng.loss_and_grads(frames, lab, labD, crop=crop, flip=flip, drop_masks=_masks(BF))
    torch.cuda.synchronize()
    par = ref["train"]
    assert set(grads) == set(par)
    rel = abs(float(loss[0]) - ref["loss"]) / max(1.0, abs(ref["loss"]))
    print(f"[frozen_eval] bf16 {prefix} {geom}: loss {float(loss[0]):.5f} ref {ref['loss']:.5f} rel {rel:.2e}")
    assert rel < 5e-2
    gn = float(torch.cat([ref["grads"][k].double().reshape(-1) for k in par]).norm())
    bad, figs = [], []
    for k in par:
        a, b = grads[k].detach().cpu().double().reshape(-1), ref["grads"][k].double().reshape(-1)
        if float(b.norm()) < 2e-3 * gn:
            assert float(a.norm()) < 1e-2 * gn, k
            continue
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        ratio = float(a.norm() / b.norm())
        lo, hi = (0.4, 2.5) if k.endswith("conv3D.bias") else (0.6, 1.6)
        min_cos = 0.7
        if float(b.norm()) < 1e-2 * gn:
            min_cos, lo, hi = 0.2, min(lo, 0.45), max(hi, 2.2)
        figs.append((cos, ratio, k))
        if not (cos > min_cos and lo < ratio < hi):
            bad.append((k, round(cos, 3), round(ratio, 3)))
    print(f"[frozen_eval] bf16 {prefix} {geom}: worst cosine {min(figs)[:1]} {min(figs)[2]}, ratios "
          f"{min(f[1] for f in figs):.3f} .. {max(f[1] for f in figs):.3f} over {len(figs)} tensors")
    assert not bad, bad


# ----------------------------------------------------------------------------- 7. a tiny epoch through TDEEDModel
def _model(state=None):
    from tdeed_amd import augment
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(C.CFG))
    m._train_dtype = torch.float32
    m.load(C.start_state() if state is None else state)
    m._model.augment_fn = augment.crop_only
    m._model.dropout_mask_fn = lambda B, T, Cc, n: drop_masks(77, B, T, Cc, n)
    return m


def _mixup_batches():
    out = []
    for rank in (0, 1):
        f1, l1, d1 = C.batch("full", rank)
        f2, l2, d2 = C.batch("full", rank + 2)
        out.append(dict(frame=f1, label=l1, labelD=d1, frame2=f2, label2=l2, labelD2=d2))
    return out


def test_epoch_with_an_eval_prefix_and_state_dict_round_trip():
    from tdeed_amd.optim import forward_stages
    batches = _mixup_batches()
    m = _model()
    with pytest.raises(ValueError, match="frozen_stats"):
        m.get_optimizer({"lr": 3e-4, "groups": C.groups("s2"), "frozen_stats": "running"})
    optimizer, _ = m.get_optimizer({"lr": 3e-4, "frozen_stats": "eval", "groups": C.groups("s2")})
    eng = optimizer.engine
    stages = forward_stages(eng.spec)
    assert optimizer.param_groups[0]["frozen_stats"] == "eval" and eng.eval_prefix == tuple(stages[:C.n_eval_stages("s2")])
    start_flat, start_buf = eng.params.flat.cpu(), _buffers(eng)
    random.seed(5)
    m.epoch(batches, optimizer=optimizer)
    torch.cuda.synchronize()
    assert eng.opt.t == 2
    flat, buf = eng.params.flat.cpu(), _buffers(eng)
    for k, (o, n) in eng.params.index.items():
        assert torch.equal(flat[o:o + n], start_flat[o:o + n]) == (k in eng.frozen), k
    for k, v in buf.items():
        if _prefix_stage(eng, k):
            assert torch.equal(v, start_buf[k]), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(start_buf[k]) + 2, k
        else:
            assert not torch.equal(v, start_buf[k]), k
    # the key travels in state_dict() into an optimizer built without it, on a model holding the same state
    sd = optimizer.state_dict()
    assert sd["param_groups"][0]["frozen_stats"] == "eval"
    m2 = _model({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    opt2, _ = m2.get_optimizer({"lr": 3e-4})
    assert "frozen_stats" not in opt2.param_groups[0] and opt2.engine.eval_prefix == () and opt2.engine.prefix is None
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["frozen_stats"] == "eval" and opt2.engine.eval_prefix == eng.eval_prefix
    assert opt2.engine.frozen == eng.frozen and opt2.engine.prefix is not None
    # load() on the first model re-packs the prefix from the tensors it is handed (the same values here)
    gen = eng.prefix_gen
    m.load({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    assert eng.prefix_gen == gen + 1
    for mm, oo in ((m, optimizer), (m2, opt2)):
        random.seed(6)
        mm.epoch(batches[:1], optimizer=oo)
    torch.cuda.synchronize()
    assert torch.equal(opt2.engine.params.flat, eng.params.flat) and torch.equal(opt2.engine.opt.exp_avg_sq, eng.opt.exp_avg_sq)
    assert not torch.equal(eng.params.flat.cpu(), flat) and eng.opt.t == 3 and opt2.engine.opt.t == 3
    for k in buf:
        assert torch.equal(m.state_dict()[k], m2.state_dict()[k]), k
    optimizer.set_groups(None)
    assert "frozen_stats" not in optimizer.param_groups[0] and eng.eval_prefix == () and eng.prefix is None


# ----------------------------------------------------------------------------- 8. the stem's eval instance alone
@pytest.mark.parametrize("f32_frames", [False, True])
@pytest.mark.parametrize("gi", range(len(C.STEM_GEOMS)))
def test_stem_mfma_eval(gi, f32_frames):
    """tdeed_stem_mfma_eval_fwd element by element within the bound of frozen_eval_cases.stem_case (proved to contain the
    fp32 reference rounded once in tests/test_frozen_eval_host.py); the output sits in a guarded buffer."""
    from tdeed_amd import ops, _lib
    from tdeed_amd.packing import stem_frags_on_device
    _lib.load()
    c = C.stem_case(gi, f32_frames)
    N, H, W, crop = C.STEM_GEOMS[gi]
    ch, cw = (crop[2], crop[3]) if crop else (H, W)
    assert ops.stem_mfma_parts(ch, cw) > 0
    g = Guarded(tuple(c["ref"].ref.shape))
    ops.stem_mfma_eval(c["frames"].to(DEV), stem_frags_on_device(c["w"].to(DEV)), c["sc"].to(DEV), c["sh"].to(DEV), crop,
                       c["flips"].to(DEV), out=g.view)
    name = f"stem_mfma_eval {C.STEM_GEOMS[gi]} f32={f32_frames}"
    out = g.check(name)
    R.assert_within(out, c["ref"], name, nhwc=True)
    frac = R.relu_open(c["ref"].ref)
    assert 0.2 < frac < 0.8, frac
    R.assert_unbiased(out, c["ref"], name)                       # one rounding of an fp32 value
    # the flags are read per frame: all-plain and all-flipped launches agree with the mixed one frame by frame
    for flag in (False, True):
        y = ops.stem_mfma_eval(c["frames"].to(DEV), stem_frags_on_device(c["w"].to(DEV)), c["sc"].to(DEV), c["sh"].to(DEV),
                               crop, flag)
        torch.cuda.synchronize()
        sel = c["flips"].bool() == flag
        assert torch.equal(y[sel.to(DEV)], out[sel.to(DEV)])
        assert not torch.equal(y[(~sel).to(DEV)], out[(~sel).to(DEV)])
