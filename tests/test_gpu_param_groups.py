"""Parameter groups and frozen tensors on the MI355X: tdeed_adamw_step_groups against the plain and the guarded launch, run
by run and bit for bit, and against torch.optim.AdamW with real param groups; then the same through TrainEngine (eager
and captured: which backward stages run, what reaches the flat gradient buffer, what a step changes), the public
get_optimizer / epoch / state_dict interface and a two-rank job.  -m gpu only."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import act, cfg_ns, drop_masks, max_abs, model_state, t
from tdeed_amd import synth, state_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 100003                     # tests/test_gpu_ops.py::test_adamw_step_matches_torch_optim: scalar tail of 3
LR = 8e-4
WD = 0.01
TRIP = 4096 * 256 * 4          # elements the capped grid covers in one trip of the grid-stride loop
N_WRAP = TRIP + 3075           # a second trip of 768 chunks and a scalar tail of 3 (tests/test_gpu_guarded_step.py)
# the CFG of tests/test_gpu_guarded_step.py: 200MF, clip_len 6; batches of two 64 x 64 clips, fp32
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
TRUNK = [{"params": ("_features.*",), "frozen": True}]
FRONT = [{"params": ("_features.stem.*", "_features.s1.*", "_features.s2.*"), "frozen": True}]
# settings the runs of the kernel tests cycle through: (lr_scale, weight_decay | None = the launch's, frozen)
SETTINGS = [(0.5, 0.0, False), (1.0, None, True), (1.0, None, False), (0.1, 0.05, False), (0.25, None, False)]


@pytest.fixture(scope="module")
def ops():
    from tdeed_amd import ops as o, _lib
    _lib.load()
    return o


def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


@functools.lru_cache(maxsize=None)
def _host(n):
    """(param, three gradients) for a size, drawn once and left unchanged"""
    rng = np.random.default_rng(7000 + n % 1000)
    return (torch.from_numpy(rng.standard_normal(n).astype(np.float32)),
            [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for _ in range(3)])


def _boundaries(n):
    """Run boundaries for a buffer of n elements: element 4 (a one-chunk first run), the middle of a workgroup's 1024
    elements, an exact workgroup boundary, (n > TRIP) a run that crosses the grid-stride wrap, and the last full chunk's
    end, so that the last run holds the scalar tail alone."""
    b = [4, 512 if n < 4096 else 3 * 1024 + 512]
    if n > TRIP:
        b += [TRIP - 2 * 1024, TRIP + 1028]                      # [TRIP - 2048, TRIP + 1028) spans the wrap
    elif n >= 65536:
        b += [50 * 1024]
    b.append(n >> 2 << 2)                                        # (n = 1027: 1024, the workgroup boundary itself)
    assert b == sorted(set(b)) and all(x % 4 == 0 and 0 < x < n for x in b) and n & 3
    return b


def _runs(n, settings=SETTINGS, bounds=None):
    ends = (bounds if bounds is not None else _boundaries(n)) + [n]
    return [(e,) + settings[i % len(settings)] for i, e in enumerate(ends)]


def _new_guard(ops, n):
    return torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=DEV), ops.grad_guard_ws(n, DEV)


def _grouped_vs_slices(ops, n, runs, guard_kw=None, nan_frozen=False, steps=3):
    """`steps` steps of the grouped launch over the whole buffer; every run's p, m, v must equal, bit for bit, the plain
    launch (or, with guard_kw, the guarded launch given the SAME record) on that run's slice alone at
    float32(lr) * float32(scale) and the run's decay; frozen runs keep their bits."""
    p0, grads = _host(n)
    table = ops.adamw_run_table(runs, n, DEV)
    assert tuple(table.shape) == (len(runs), 4)
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    if any(r[3] for r in runs):                                  # non-zero moments, so that "keeps its bits" says something
        m.copy_(rnd(31, "m", (n,), 1e-3))
        v.copy_(rnd(32, "v", (n,), 1e-3).abs())
    m0, v0 = m.clone(), v.clone()
    spans = [(lo, hi) + r[1:] for lo, hi, r in zip([0] + [r[0] for r in runs[:-1]], [r[0] for r in runs], runs)]
    ref = [(p[lo:hi].clone(), m[lo:hi].clone(), v[lo:hi].clone()) for lo, hi, *_ in spans]
    guard, ws = _new_guard(ops, n) if guard_kw is not None else (None, None)
    for step in range(1, steps + 1):
        g = grads[step - 1].clone().to(DEV)
        for lo, hi, _, _, frozen in spans:
            if frozen:
                g[lo:hi] = float("nan") if nan_frozen else 0.0   # the engine keeps frozen ranges at zero
        if guard is not None:
            ops.grad_guard(g, guard, ws, guard_kw.get("skip_nonfinite", False))
        ops.adamw_step_groups(p, g, m, v, step, LR, table, weight_decay=WD, guard=guard, **(guard_kw or {}))
        for (lo, hi, scale, wd, frozen), (rp, rm, rv) in zip(spans, ref):
            if frozen:
                continue
            lr_s = float(np.float32(LR) * np.float32(scale))
            gs = g[lo:hi].clone()                                # a fresh allocation: 16-byte aligned like the slice's twin
            if guard is None:
                ops.adamw_step(rp, gs, rm, rv, step, lr_s, weight_decay=WD if wd is None else wd)
            else:
                ops.adamw_step_guarded(rp, gs, rm, rv, step, lr_s, weight_decay=WD if wd is None else wd, guard=guard,
                                       **guard_kw)
    torch.cuda.synchronize()
    for i, ((lo, hi, scale, wd, frozen), (rp, rm, rv)) in enumerate(zip(spans, ref)):
        what = (n, i, lo, hi, scale, wd, frozen)
        if frozen:
            assert torch.equal(p[lo:hi].cpu(), p0[lo:hi]) and torch.equal(m[lo:hi], m0[lo:hi]) \
                and torch.equal(v[lo:hi], v0[lo:hi]), what
        else:
            assert torch.equal(p[lo:hi], rp) and torch.equal(m[lo:hi], rm) and torch.equal(v[lo:hi], rv), what
            assert not torch.equal(p[lo:hi].cpu(), p0[lo:hi]), what
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
    return p, m, v, guard


# ----------------------------------------------------------------------------- 1. the kernel, run by run
@pytest.mark.parametrize("n", [1027, N, N_WRAP])
def test_every_run_equals_the_plain_launch_on_its_slice(ops, n):
    """Unguarded form.  The frozen runs' gradient ranges hold NaN: they are not read into anything."""
    runs = _runs(n)
    assert runs[0][0] == 4 and runs[-1][0] - runs[-2][0] == 3 and sum(r[3] for r in runs) >= 1
    _grouped_vs_slices(ops, n, runs, nan_frozen=True)


def test_frozen_last_run_leaves_the_scalar_tail_alone(ops):
    n = 1027
    runs = _runs(n, settings=[(0.5, 0.0, False), (1.0, None, True)], bounds=[512, 1024])
    assert runs[-1] == (n, 0.5, 0.0, False)
    _grouped_vs_slices(ops, n, runs, nan_frozen=True)
    runs = _runs(n, settings=[(1.0, None, True), (0.5, 0.0, False)], bounds=[512, 1024])
    assert runs[-1] == (n, 1.0, None, True)
    _grouped_vs_slices(ops, n, runs, nan_frozen=True)


@pytest.mark.parametrize("n", [1027, N, N_WRAP])
def test_neutral_runs_are_bit_identical_to_the_plain_and_the_guarded_launch(ops, n):
    """Every run at lr_scale 1, the launch's decay (or the same value spelled out), not frozen -- a table of one run and
    one cut at every boundary of _boundaries: the whole buffer equals tdeed_adamw_step's, and with a record
    tdeed_adamw_step_guarded's."""
    p0, grads = _host(n)
    for runs in ([(n, 1.0, None, False)], _runs(n, settings=[(1.0, None, False), (1.0, WD, False)])):
        table = ops.adamw_run_table(runs, n, DEV)
        bufs = [[p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for _ in range(4)]
        guard, ws = _new_guard(ops, n)
        for step, g in enumerate(grads, 1):
            g = g.to(DEV)
            ops.adamw_step(*bufs[0][:1], g, *bufs[0][1:], step, LR, weight_decay=WD)
            ops.adamw_step_groups(*bufs[1][:1], g, *bufs[1][1:], step, LR, table, weight_decay=WD)
            ops.grad_guard(g, guard, ws, True)
            ops.adamw_step_guarded(*bufs[2][:1], g, *bufs[2][1:], step, LR, weight_decay=WD, guard=guard,
                                   skip_nonfinite=True)
            ops.adamw_step_groups(*bufs[3][:1], g, *bufs[3][1:], step, LR, table, weight_decay=WD, guard=guard,
                                  skip_nonfinite=True)
        for a, b in zip(bufs[0] + bufs[2], bufs[1] + bufs[3]):
            assert torch.equal(a, b), (n, len(runs))
        assert torch.equal(bufs[0][0], bufs[2][0]) and not torch.equal(bufs[0][0].cpu(), p0)


def test_a_table_of_431_runs(ops):
    """As many runs as the 200MF model has tensors, 232 elements each, settings cycling (frozen ones included)."""
    bounds = [232 * (i + 1) for i in range(430)]
    assert bounds[-1] < N - 3
    runs = _runs(N, bounds=bounds)
    assert len(runs) == 431
    _grouped_vs_slices(ops, N, runs, nan_frozen=True)


# ----------------------------------------------------------------------------- 2. with the guard
@pytest.mark.parametrize("n", [N, N_WRAP])
def test_clipped_steps_equal_the_guarded_launch_per_slice_given_the_same_record(ops, n):
    """max_grad_norm at half the first gradient's norm: ONE global coefficient, from the record over the whole buffer
    (frozen ranges hold zeros, as in the engine)."""
    p0, grads = _host(n)
    runs = _runs(n)
    trainable = torch.ones(n, dtype=torch.bool)
    lo = 0
    for end, _, _, frozen in runs:
        trainable[lo:end] = not frozen
        lo = end
    max_norm = 0.5 * float((grads[0] * trainable).double().norm())
    _, _, _, guard = _grouped_vs_slices(ops, n, runs, guard_kw=dict(skip_nonfinite=True, max_grad_norm=max_norm))
    rec = guard.cpu()
    want = float((grads[2] * trainable).double().norm())
    assert abs(float(rec[:2].view(torch.float64)[0]) ** 0.5 - want) <= 1e-6 * want and int(rec[2]) == 0 and int(rec[3]) == 0


@pytest.mark.parametrize("n", [1027, N_WRAP])
def test_a_skipped_step_changes_no_bit_in_any_run(ops, n):
    p0, grads = _host(n)
    runs = _runs(n)
    table = ops.adamw_run_table(runs, n, DEV)
    p, m, v = p0.clone().to(DEV), rnd(31, "m", (n,), 1e-3).to(DEV), rnd(32, "v", (n,), 1e-3).abs().to(DEV)
    before = (p.clone(), m.clone(), v.clone())
    guard, ws = _new_guard(ops, n)
    g = grads[0].clone().to(DEV)
    g[runs[1][0] + 1] = float("nan")                             # one NaN, in the third run (the second is frozen)
    ops.grad_guard(g, guard, ws, True)
    ops.adamw_step_groups(p, g, m, v, 1, LR, table, weight_decay=WD, guard=guard, skip_nonfinite=True)
    torch.cuda.synchronize()
    assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
    assert int(guard.cpu()[3]) == 1
    g = grads[1].to(DEV)                                         # and the next, finite step goes through
    ops.grad_guard(g, guard, ws, True)
    ops.adamw_step_groups(p, g, m, v, 2, LR, table, weight_decay=WD, guard=guard, skip_nonfinite=True)
    assert not torch.equal(p, before[0]) and bool(torch.isfinite(p).all()) and int(guard.cpu()[3]) == 1


# ----------------------------------------------------------------------------- 3. against torch
def test_matches_torch_adamw_with_param_groups_and_a_frozen_tensor(ops):
    """torch.optim.AdamW with one param group per run and one requires_grad_(False) tensor, three steps on the CPU.
    Bound: max abs 2e-6 at lr 8e-4 on unit-scale parameters, what tests/test_gpu_ops.py::
    test_adamw_step_matches_torch_optim holds the plain launch to; every lr_scale is <= 1, so it carries over."""
    p0, grads = _host(N)
    runs = _runs(N)
    spans = [(lo, hi) + r[1:] for lo, hi, r in zip([0] + [r[0] for r in runs[:-1]], [r[0] for r in runs], runs)]
    parts = [p0[lo:hi].clone().requires_grad_(not frozen) for lo, hi, _, _, frozen in spans]
    ref = torch.optim.AdamW([dict(params=[x], lr=LR * scale, weight_decay=WD if wd is None else wd)
                             for x, (_, _, scale, wd, frozen) in zip(parts, spans) if not frozen], lr=LR)
    table = ops.adamw_run_table(runs, N, DEV)
    p, m, v = p0.clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    for step, g in enumerate(grads, 1):
        for x, (lo, hi, *_rest) in zip(parts, spans):
            x.grad = g[lo:hi].clone() if x.requires_grad else None
        ref.step()
        ops.adamw_step_groups(p, g.to(DEV), m, v, step, LR, table, weight_decay=WD)
    err = max_abs(p.cpu(), torch.cat([x.detach() for x in parts]))
    print(f"grouped launch vs torch.optim.AdamW with param groups: max |param diff| = {err:.3e}")
    assert err < 2e-6
    assert any(frozen for *_x, frozen in spans)
    for lo, hi, _, _, frozen in spans:
        if frozen:
            assert torch.equal(p[lo:hi].cpu(), p0[lo:hi]) and float(m[lo:hi].abs().sum()) == 0.0


def test_run_table_argument_errors(ops):
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.adamw_run_table([(6, 1.0, None, False), (1027, 1.0, None, False)], 1027, DEV)
    with pytest.raises(ValueError, match="ascend"):
        ops.adamw_run_table([(512, 1.0, None, False), (512, 1.0, None, False), (1027, 1.0, None, False)], 1027, DEV)
    with pytest.raises(ValueError, match="the buffer at"):
        ops.adamw_run_table([(512, 1.0, None, False)], 1027, DEV)
    with pytest.raises(ValueError, match="finite"):
        ops.adamw_run_table([(1027, -1.0, None, False)], 1027, DEV)
    p = torch.zeros(1027, device=DEV)
    table = ops.adamw_run_table([(1027, 1.0, None, False)], 1027, DEV)
    with pytest.raises(ValueError, match="one length"):
        ops.adamw_step_groups(p, torch.zeros(1024, device=DEV), p.clone(), p.clone(), 1, LR, table)
    with pytest.raises(ValueError, match="run table"):
        ops.adamw_step_groups(p, p.clone(), p.clone(), p.clone(), 1, LR, table.view(-1))


# ----------------------------------------------------------------------------- 4. engine, eager and captured
def _batch(rank=0):
    B, T = 2, CFG["clip_len"]
    frames = t(synth.uint8_clip(1300 + rank, (B, T, 3, 64, 64)))
    lab, labD = synth.labels(1400 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
    return frames, t(lab).long(), t(labD).float()


def _engine(device=DEV, groups=None):
    from tdeed_amd.trainer import TrainEngine
    sd = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}
    eng = TrainEngine(CFG, sd, act_dtype=torch.float32, device=device, lr=1e-3)
    if groups is not None:
        eng.set_groups(groups)
    return eng


def _one_step(eng, graph, rank=0, profile=False):
    """one optimisation step on _batch(rank) -> the set of _lib.SCOPE labels its launches carried (eager + profile only)"""
    from tdeed_amd import _lib
    frames, lab, labD = (x.to(DEV) for x in _batch(rank))
    scopes = None
    if graph:
        eng.make_step(frames.shape[0], 64, 64, frames, lab, labD, None, use_graph=True)()
    elif profile:
        with _lib.profile() as prof:
            eng.step(frames, lab, labD)
        scopes = {rec[4] for rec in prof.rec}
    else:
        eng.step(frames, lab, labD)
    torch.cuda.synchronize()
    return scopes


def _snapshot(eng):
    return dict(grad=eng.params.grad.cpu(), flat=eng.params.flat.cpu(), m=eng.opt.exp_avg.cpu(), v=eng.opt.exp_avg_sq.cpu(),
                buffers={k: v.detach().cpu().clone() for k, v in eng.state.items() if not state_layout.is_parameter(k)},
                index=dict(eng.params.index))


@functools.lru_cache(maxsize=None)
def _run(kind, graph):
    """One step of a fresh engine, computed once per (freeze set, eager | captured) and left unchanged:
    kind "twin" (nothing frozen), "trunk" (_features.* frozen) or "front" (stem, s1, s2 frozen)."""
    eng = _engine(groups={"twin": None, "trunk": TRUNK, "front": FRONT}[kind])
    start = eng.params.flat.cpu()
    scopes = _one_step(eng, graph, profile=not graph)
    out = _snapshot(eng)
    out.update(start=start, scopes=scopes, frozen=eng.frozen, stages=eng.stages,
               mode=(eng.last_graph.mode if graph else None))
    return out


def _ranges(index, pred):
    return [(k, o, n) for k, (o, n) in index.items() if pred(k)]


@pytest.mark.parametrize("graph", [False, True])
def test_trunk_frozen_gradient_buffer(graph):
    """_features.* frozen: the trainable ranges of the flat gradient buffer equal the unfrozen twin's bit for bit, the
    frozen ranges (and all padding) are zero."""
    got, twin = _run("trunk", graph), _run("twin", graph)
    assert got["stages"] == ["temporal", "temp_enc"] and len(got["frozen"]) > 100 and "temp_enc" not in got["frozen"]
    keep = torch.zeros_like(got["grad"], dtype=torch.bool)
    for k, o, n in _ranges(got["index"], lambda k: k not in got["frozen"]):
        assert torch.equal(got["grad"][o:o + n], twin["grad"][o:o + n]), k
        keep[o:o + n] = True
    assert float(got["grad"][keep].abs().max()) > 0.0
    assert float(got["grad"][~keep].abs().max()) == 0.0
    assert float(twin["grad"][~keep].abs().max()) > 0.0           # the twin did write trunk gradients there


@pytest.mark.parametrize("graph", [False, True])
def test_trunk_frozen_state_after_the_step(graph):
    """Frozen parameters and their moments keep their bits; trainable ones equal the twin's bit for bit; the BatchNorm
    running statistics and num_batches_tracked moved exactly as in the twin (the forward is untouched)."""
    got, twin = _run("trunk", graph), _run("twin", graph)
    changed = dict(twin_trunk=0, trainable=0)
    for k, o, n in _ranges(got["index"], lambda k: True):
        sl = slice(o, o + n)
        if k in got["frozen"]:
            assert torch.equal(got["flat"][sl], got["start"][sl]), k
            assert float(got["m"][sl].abs().max()) == 0.0 and float(got["v"][sl].abs().max()) == 0.0, k
            changed["twin_trunk"] += int(not torch.equal(twin["flat"][sl], twin["start"][sl]))
        else:
            assert torch.equal(got["flat"][sl], twin["flat"][sl]) and torch.equal(got["m"][sl], twin["m"][sl]) \
                and torch.equal(got["v"][sl], twin["v"][sl]), k
            changed["trainable"] += int(not torch.equal(got["flat"][sl], got["start"][sl]))
    # the step did move (nearly) every tensor it may move, and the twin did train the trunk
    assert changed["twin_trunk"] > 0.9 * len(got["frozen"])
    assert changed["trainable"] > 0.9 * (len(got["index"]) - len(got["frozen"]))
    start_buffers = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}
    moved = 0
    for k, v in got["buffers"].items():
        assert torch.equal(v, twin["buffers"][k]), k
        moved += int(not torch.equal(v.float(), start_buffers[k].float()))
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(start_buffers[k]) + 1, k
    assert moved == len(got["buffers"])                          # frozen BatchNorms still move their running statistics


def test_trunk_frozen_launches_no_trunk_backward():
    got, twin = _run("trunk", False), _run("twin", False)
    bwd = {s for s in got["scopes"] if s.endswith(".bwd")}
    assert bwd == {"temporal.bwd"}, bwd                          # avgpool_posenc_bwd runs under the temporal scope
    assert {"stem.bwd", "s1.b1.bwd", "s4.b7.bwd"} <= twin["scopes"] and len({s for s in twin["scopes"] if s.endswith(".bwd")}) == 15
    assert {s for s in got["scopes"] if s.endswith(".fwd")} == {s for s in twin["scopes"] if s.endswith(".fwd")}
    o, n = got["index"]["temp_enc"]
    assert float(got["grad"][o:o + n].abs().max()) > 0 and torch.equal(got["grad"][o:o + n], twin["grad"][o:o + n])


@pytest.mark.parametrize("graph", [False, True])
def test_front_frozen_stops_behind_s3_b1(graph):
    """Stem, s1, s2 frozen: their backward is not launched; the gradients of s3, s4 and the temporal stack equal the twin's
    bit for bit."""
    got, twin = _run("front", graph), _run("twin", graph)
    assert got["stages"][-1] == "s3.b1" and len(got["stages"]) == 13
    if not graph:
        bwd = {s for s in got["scopes"] if s.endswith(".bwd")}
        assert not bwd & {"stem.bwd", "s1.b1.bwd", "s2.b1.bwd"} and {"s3.b1.bwd", "s4.b7.bwd", "temporal.bwd"} <= bwd
        assert len(bwd) == 12
    for k, o, n in _ranges(got["index"], lambda k: True):
        sl = slice(o, o + n)
        if k.startswith(("_features.stem.", "_features.s1.", "_features.s2.")):
            assert float(got["grad"][sl].abs().max()) == 0.0 and torch.equal(got["flat"][sl], got["start"][sl]), k
        else:
            assert torch.equal(got["grad"][sl], twin["grad"][sl]) and torch.equal(got["flat"][sl], twin["flat"][sl]), k


def test_freezing_after_a_step_zeroes_the_stale_gradients():
    """Step 1 unfrozen (with the guard's statistics on), then set_groups: the trunk's ranges of the gradient buffer, written
    by step 1, are zero at once; after step 2 last_norm is the norm of the trainable gradients; the trunk keeps the bits
    step 1 left, moments included."""
    eng = _engine()
    eng.opt.set_guard(skip_nonfinite=True)
    _one_step(eng, False)
    eng.set_groups(TRUNK)
    trunk = _ranges(eng.params.index, lambda k: k in eng.frozen)
    assert all(float(eng.params.grad[o:o + n].abs().max()) == 0.0 for _, o, n in trunk)
    after1 = _snapshot(eng)
    _one_step(eng, False, rank=1)
    grad = eng.params.grad.double()
    want = float(torch.cat([grad[o:o + n] for k, (o, n) in eng.params.index.items() if k not in eng.frozen]).norm())
    st = eng.opt.guard_stats()
    assert abs(st["last_norm"] - want) <= eng.params.numel * 2.0 ** -52 * want and st["skipped"] == 0
    after2 = _snapshot(eng)
    for k, o, n in trunk:
        sl = slice(o, o + n)
        assert torch.equal(after2["flat"][sl], after1["flat"][sl]) and torch.equal(after2["m"][sl], after1["m"][sl]) \
            and torch.equal(after2["v"][sl], after1["v"][sl]), k
        assert float(after1["m"][sl].abs().max()) > 0, k
    o, n = eng.params.index["_pred_fine._fc_out.weight"]
    assert not torch.equal(after2["flat"][o:o + n], after1["flat"][o:o + n])
    # and back: None returns to the plain launch, the trunk trains again
    eng.set_groups(None)
    assert eng.frozen == frozenset() and eng.stages is None and eng.opt.run_table is None
    _one_step(eng, False)
    k, o, n = trunk[0]
    assert not torch.equal(eng.params.flat[o:o + n].cpu(), after2["flat"][o:o + n])


def test_a_graph_belongs_to_its_freeze_set():
    eng = _engine()
    frames, lab, labD = (x.to(DEV) for x in _batch())
    step = eng.make_step(2, 64, 64, frames, lab, labD, None, use_graph=True)
    h = eng.last_graph
    assert h.frozen == frozenset()
    step()
    eng.set_groups(TRUNK)
    assert eng.last_graph is None                                # set_groups drops the handle make_step kept
    with pytest.raises(RuntimeError, match="frozen"):
        eng.step_graph(h, frames, lab, labD)
    with pytest.raises(RuntimeError, match="frozen"):
        step()                                                   # the callable of the old handle, too
    step2 = eng.make_step(2, 64, 64, frames, lab, labD, None, use_graph=True)
    assert eng.last_graph is not h and eng.last_graph.frozen == eng.frozen
    before = eng.params.flat.clone()
    step2()
    torch.cuda.synchronize()
    o, n = eng.params.index["_features.stem.conv.weight"]
    assert torch.equal(eng.params.flat[o:o + n], before[o:o + n]) and not torch.equal(eng.params.flat, before)
    assert eng.make_step(2, 64, 64, frames, lab, labD, None, use_graph=True) is not None and eng.last_graph.frozen == eng.frozen
    with pytest.raises(ValueError, match="nothing left to train"):
        eng.set_groups([{"params": ("*",), "frozen": True}])


# ----------------------------------------------------------------------------- 5. public interface
EXAMPLE = [
    {"params": ("_features.stem.*", "_features.s1.*", "_features.s2.*"), "frozen": True},
    {"params": ("_features.*",), "lr_scale": 0.1},
    {"params": ("*.bn.*", "*.ln*", "*.gn.*", "*.bias"), "weight_decay": 0.0},
]


def _model(state=None):
    from tdeed_amd import augment
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(CFG))
    m._train_dtype = torch.float32
    m.load({k: t(v) for k, v in model_state(CFG, 17).items()} if state is None else state)
    m._model.augment_fn = augment.crop_only
    m._model.dropout_mask_fn = lambda B, T, C, n: drop_masks(77, B, T, C, n)
    return m


def test_get_optimizer_groups_epoch_and_state_dict_round_trip():
    """get_optimizer({'lr', 'groups'}) + epoch() over two batches with a LinearLR equals a twin engine driven by hand (same
    groups, the scheduler's lr values, accumulate + apply) bit for bit; state_dict() carries the groups and the moments
    into an optimizer built without them, and both then take the same step bit for bit."""
    lr = 3e-4
    batches = []
    for rank in (0, 1):
        frames, lab, labD = _batch(rank)
        batches.append(dict(frame=frames, label=lab, labelD=labD))
    m = _model()
    with pytest.raises(ValueError, match="matches no parameter"):
        m.get_optimizer({"lr": lr, "groups": [{"params": ("_featurs.*",), "frozen": True}]})
    optimizer, scaler = m.get_optimizer({"lr": lr, "groups": EXAMPLE})
    assert scaler is None and len(optimizer.param_groups) == 1
    g0 = optimizer.param_groups[0]
    assert g0["groups"][0]["frozen"] is True and g0["groups"][1]["lr_scale"] == 0.1 and g0["groups"][2]["weight_decay"] == 0.0
    assert g0["skip_nonfinite"] is False and g0["lr"] == lr
    sched = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=0.01, end_factor=1.0, total_iters=4)
    m.epoch(batches, optimizer=optimizer, lr_scheduler=sched)
    torch.cuda.synchronize()
    assert sched.last_epoch == 2 and optimizer.engine.opt.t == 2
    # the twin: a TrainEngine driven by hand with the lr values the same scheduler gives a dummy optimizer
    dummy = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
    sched_d = torch.optim.lr_scheduler.LinearLR(dummy, start_factor=0.01, end_factor=1.0, total_iters=4)
    twin = _engine(groups=EXAMPLE)
    for b in batches:
        masks = [x.to(DEV).float() for x in drop_masks(77, 2, CFG["clip_len"], twin.spec.feat_dim, 2)]
        twin.accumulate(b["frame"].to(DEV), b["label"].to(DEV), b["labelD"].to(DEV), drop_masks=masks)
        twin.apply(lr=dummy.param_groups[0]["lr"])
        dummy.step()
        sched_d.step()
    torch.cuda.synchronize()
    eng = optimizer.engine
    assert torch.equal(eng.params.flat, twin.params.flat) and torch.equal(eng.opt.exp_avg, twin.opt.exp_avg)
    assert torch.equal(eng.opt.exp_avg_sq, twin.opt.exp_avg_sq)
    start = {k: t(v) for k, v in model_state(CFG, 17).items()}
    assert torch.equal(eng.state["_features.s1.b1.conv1.conv.weight"].cpu(), start["_features.s1.b1.conv1.conv.weight"])
    assert not torch.equal(eng.state["_features.s3.b1.conv2.conv.weight"].cpu(), start["_features.s3.b1.conv2.conv.weight"])
    # set_groups on the optimizer: the torch side follows
    sd = optimizer.state_dict()
    assert sd["param_groups"][0]["groups"] == g0["groups"] and sd["fused"]["t"] == 2
    # round trip into an optimizer built WITHOUT groups, on a model holding the same state
    m2 = _model({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    opt2, _ = m2.get_optimizer({"lr": lr})
    assert "groups" not in opt2.param_groups[0] and opt2.engine.opt.run_table is None
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["groups"] == g0["groups"] and opt2.engine.frozen == eng.frozen
    assert opt2.engine.stages == eng.stages and opt2.param_groups[0]["lr"] == g0["lr"]
    assert torch.equal(opt2.engine.opt.exp_avg, eng.opt.exp_avg)
    for mm, oo in ((m, optimizer), (m2, opt2)):
        mm.epoch(batches[:1], optimizer=oo)
    torch.cuda.synchronize()
    assert torch.equal(opt2.engine.params.flat, eng.params.flat) and torch.equal(opt2.engine.opt.exp_avg_sq, eng.opt.exp_avg_sq)
    assert eng.opt.t == 3 and opt2.engine.opt.t == 3
    # None returns to the plain launch
    optimizer.set_groups(None)
    assert "groups" not in optimizer.param_groups[0] and eng.opt.run_table is None and eng.frozen == frozenset()


# ----------------------------------------------------------------------------- 6. two ranks on one GPU over gloo
BOTH = [{"params": ("_features.*", "temp_enc"), "frozen": True}]


def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from tdeed_amd import dist as tdist
    torch.cuda.set_device(0)                                     # both ranks share the one GPU
    tdist.init(backend="gloo")
    out = {}
    for name, groups in (("trunk", TRUNK), ("both", BOTH)):
        eng = _engine("cuda:0")
        red = eng.set_reducer("auto")
        assert red is not None and red.world == world and len(red.buckets) == 2
        eng.set_groups(groups)
        frames, lab, labD = (x.to("cuda:0") for x in _batch(rank))
        eng.step(frames, lab, labD)
        torch.cuda.synchronize()
        out[name] = dict(flat=eng.params.flat.detach().cpu().numpy(), grad=eng.params.grad.detach().cpu().numpy(),
                         launched=[i for i, _ in red.launched], describe=red.describe())
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_a_frozen_trunk():
    """Two ranks and this process: three processes hold the GPU.  _features.* frozen: both ranks end with equal parameters,
    within tests/test_gpu_dp.py's bound (2e-7 + 1e-6 max|w|) of one process stepping on the mean gradient.  The bucket rule
    is the engine's: a bucket whose tensors are ALL frozen is not reduced, a partly frozen one is reduced as before.
    temp_enc lives in the trunk's bucket, so with _features.* alone frozen that bucket still goes out (its trunk ranges are
    zeros on every rank); with temp_enc frozen as well it does not, and describe() says so."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for name, groups in (("trunk", TRUNK), ("both", BOTH)):
        a, b = res[0][1][name], res[1][1][name]
        assert np.array_equal(a["flat"], b["flat"]) and np.array_equal(a["grad"], b["grad"]), name
        grads = []
        for rank in range(2):
            eng = _engine(groups=groups)
            frames, lab, labD = (x.to(DEV) for x in _batch(rank))
            eng.accumulate(frames, lab, labD)
            grads.append(eng.params.grad.clone())
        eng.params.grad.copy_((grads[0] + grads[1]) * 0.5)
        eng.apply()
        torch.cuda.synchronize()
        for k, (o, n) in eng.params.index.items():
            want = eng.params.flat[o:o + n].cpu().numpy()
            assert np.abs(a["flat"][o:o + n] - want).max() <= 2e-7 + 1e-6 * np.abs(want).max(), (name, k)
            if k in eng.frozen:
                assert float(np.abs(a["grad"][o:o + n]).max()) == 0.0, (name, k)
        if name == "trunk":
            assert a["launched"] == [0, 1] and "bucket_frozen" not in a["describe"]
        else:
            assert a["launched"] == [0] and b["launched"] == [0]            # the trunk bucket was not reduced
            assert a["describe"]["bucket_frozen"] == [False, True]
            assert a["describe"]["bucket_collectives"][1] == "none (frozen)"
