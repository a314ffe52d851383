"""Weight EMA on the MI355X: tdeed_adamw_step_ema against the launches without EMA (parameters and moments bit for bit) and
against `optim.ema_ref` (the shadow bit for bit), tdeed_ema_tensors row by row, then the same through TrainEngine (eager and
captured), the public get_optimizer / averaged() / state_dict interface and a two-rank job.  -m gpu only.
Sizes and run boundaries are those of tests/test_gpu_param_groups.py."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import cfg_ns, drop_masks, model_state, t
from tdeed_amd import synth, state_layout
from tdeed_amd.optim import ema_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 100003                     # scalar tail of 3
LR = 8e-4
WD = 0.01
TRIP = 4096 * 256 * 4          # elements the capped grid covers in one trip of the grid-stride loop
N_WRAP = TRIP + 3075           # a second trip of 768 chunks and a scalar tail of 3
SIZES = [1027, N, N_WRAP]
DECAY = 0.999
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
TRUNK = [{"params": ("_features.*",), "frozen": True}]
# settings the runs of the kernel tests cycle through: (lr_scale, weight_decay | None = the launch's, frozen)
SETTINGS = [(0.5, 0.0, False), (1.0, None, True), (1.0, None, False), (0.1, 0.05, False), (0.25, None, False)]
SENTINEL = 0x7FC12345          # a NaN with a payload: arithmetic on it would not give it back


@pytest.fixture(scope="module")
def ops():
    from tdeed_amd import ops as o, _lib
    _lib.load()
    return o


@functools.lru_cache(maxsize=None)
def _host(n):
    """(param, three gradients, a shadow start that differs from param) for a size, drawn once and left unchanged"""
    rng = np.random.default_rng(7000 + n % 1000)
    p = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    grads = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for _ in range(3)]
    return p, grads


def _boundaries(n):
    """tests/test_gpu_param_groups.py: element 4 (a one-chunk first run), the middle of a workgroup's 1024 elements, an
    exact workgroup boundary, (n > TRIP) a run across the grid-stride wrap, and the last full chunk's end, so that the last
    run holds the scalar tail alone."""
    b = [4, 512 if n < 4096 else 3 * 1024 + 512]
    if n > TRIP:
        b += [TRIP - 2 * 1024, TRIP + 1028]
    elif n >= 65536:
        b += [50 * 1024]
    b.append(n >> 2 << 2)
    assert b == sorted(set(b)) and all(x % 4 == 0 and 0 < x < n for x in b) and n & 3
    return b


def _runs(n, settings=SETTINGS, bounds=None):
    ends = (bounds if bounds is not None else _boundaries(n)) + [n]
    return [(e,) + settings[i % len(settings)] for i, e in enumerate(ends)]


def _spans(runs):
    return [(lo, hi, r[3]) for lo, hi, r in zip([0] + [r[0] for r in runs[:-1]], [r[0] for r in runs], runs)]


def _new_guard(ops, n):
    return torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=DEV), ops.grad_guard_ws(n, DEV)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Pair:
    """The EMA launch and its twin without EMA on the same inputs, for one mode of {plain, guarded, grouped, grouped +
    guarded}: .step(g, step) runs both, .check() compares p, m, v bit for bit."""

    def __init__(self, ops, n, mode, warmup, runs=None, step0=0):
        self.ops, self.n, self.mode, self.warmup, self.step0 = ops, n, mode, warmup, step0
        p0, _ = _host(n)
        self.bufs = [[p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)] for _ in range(2)]
        self.ema = p0.clone().to(DEV)                            # the shadow starts as a copy of the parameters
        self.runs = (runs if runs is not None else _runs(n)) if "grouped" in mode else None
        self.table = ops.adamw_run_table(self.runs, n, DEV) if self.runs else None
        self.guards = [_new_guard(ops, n) for _ in range(2)] if "guarded" in mode else [(None, None)] * 2
        self.kw = dict(skip_nonfinite=True) if "guarded" in mode else {}

    def grad(self, g):
        g = g.clone().to(DEV)
        for lo, hi, frozen in (_spans(self.runs) if self.runs else ()):
            if frozen:
                g[lo:hi] = 0.0                                   # the engine keeps frozen ranges at zero
        return g

    def step(self, g, step):
        o = self.ops
        (p, m, v), (q, mq, vq) = self.bufs
        (ga, wa), (gb, wb) = self.guards
        if ga is not None:
            o.grad_guard(g, ga, wa, True)
            o.grad_guard(g, gb, wb, True)
        o.adamw_step_ema(p, g, m, v, step, LR, self.ema, DECAY, self.warmup, self.step0, self.table, weight_decay=WD,
                         guard=ga, **self.kw)
        if self.table is not None:
            o.adamw_step_groups(q, g, mq, vq, step, LR, self.table, weight_decay=WD, guard=gb, **self.kw)
        elif gb is not None:
            o.adamw_step_guarded(q, g, mq, vq, step, LR, weight_decay=WD, guard=gb, **self.kw)
        else:
            o.adamw_step(q, g, mq, vq, step, LR, weight_decay=WD)
        torch.cuda.synchronize()
        return p.cpu()

    def check(self):
        for a, b, what in zip(self.bufs[0], self.bufs[1], "pmv"):
            assert _same_bits(a, b), (self.n, self.mode, what)


MODES = ["plain", "guarded", "grouped", "grouped+guarded"]


# ----------------------------------------------------------------------------- 1. the launch
@pytest.mark.parametrize("n", SIZES)
def test_launch_equals_the_launch_without_ema_and_the_shadow_equals_ema_ref(ops, n):
    """Three steps, every mode, warmup on and off: p, m, v bit-equal to the corresponding launch without EMA on the same
    inputs; the shadow bit-equal to ema_ref fed the parameter snapshots."""
    p0, grads = _host(n)
    for mode in MODES:
        for warmup in (False, True):
            pair = _Pair(ops, n, mode, warmup)
            ref = p0.clone()
            for step, g in enumerate(grads, 1):
                snap = pair.step(pair.grad(g), step)
                ema_ref(ref, snap, step, DECAY, warmup)
                pair.check()
                assert _same_bits(pair.ema, ref), (n, mode, warmup, step)
            assert not torch.equal(pair.bufs[0][0].cpu(), p0) and not _same_bits(pair.ema, p0), (n, mode, warmup)
            assert not _same_bits(pair.ema, pair.bufs[0][0])
            if pair.runs:
                for lo, hi, frozen in _spans(pair.runs):
                    if frozen:
                        assert _same_bits(pair.ema[lo:hi], p0[lo:hi]) and _same_bits(pair.bufs[0][0][lo:hi], p0[lo:hi])


# ----------------------------------------------------------------------------- 2. a skipped step
@pytest.mark.parametrize("mode", ["guarded", "grouped+guarded"])
@pytest.mark.parametrize("n", [1027, N_WRAP])
def test_a_skipped_step_leaves_the_shadow_and_does_not_advance_n(ops, n, mode):
    """Step 2's gradient holds an inf: no bit of the shadow (or of p, m, v) changes, and step 3 is update n = 2, not 3 --
    with warmup on d_2 = 3/12 and d_3 = 4/13, so a wrong n changes bits."""
    p0, grads = _host(n)
    pair = _Pair(ops, n, mode, True)
    ref = p0.clone()
    ema_ref(ref, pair.step(pair.grad(grads[0]), 1), 1, DECAY, True)
    assert _same_bits(pair.ema, ref)
    before = [x.clone() for x in pair.bufs[0]] + [pair.ema.clone()]
    g = pair.grad(grads[1])
    g[n - 1] = float("inf")                                      # in the scalar tail: the last run is not frozen
    pair.step(g, 2)
    for a, b in zip(before, pair.bufs[0] + [pair.ema]):
        assert _same_bits(a, b), (n, mode)
    assert int(pair.guards[0][0].cpu()[3]) == 1
    snap = pair.step(pair.grad(grads[2]), 3)
    ema_ref(ref, snap, 2, DECAY, True)
    pair.check()
    assert _same_bits(pair.ema, ref), (n, mode)
    wrong = ema_ref(ema_ref(p0.clone(), before[0].cpu(), 1, DECAY, True), snap, 3, DECAY, True)
    assert not _same_bits(wrong, ref)                            # the test can tell n = 2 from n = 3


# ----------------------------------------------------------------------------- 3. frozen runs
@pytest.mark.parametrize("mode", ["grouped", "grouped+guarded"])
def test_a_frozen_run_neither_loads_nor_stores_its_shadow_slice(ops, mode):
    """The frozen runs' shadow slices hold a sentinel bit pattern (a NaN with a payload) and keep it -- also when the frozen
    run is the last one and owns the scalar tail."""
    for n, runs in ((N_WRAP, _runs(N_WRAP)),
                    (1027, _runs(1027, settings=[(0.5, 0.0, False), (1.0, None, True)], bounds=[512, 1024])),
                    (1027, _runs(1027, settings=[(1.0, None, True), (0.5, 0.0, False)], bounds=[512, 1024]))):
        p0, grads = _host(n)
        pair = _Pair(ops, n, mode, True, runs=runs)
        frozen = [(lo, hi) for lo, hi, fr in _spans(runs) if fr]
        assert frozen
        ema_i = pair.ema.view(torch.int32)
        for lo, hi in frozen:
            ema_i[lo:hi] = SENTINEL
        ref = p0.clone()
        for step, g in enumerate(grads, 1):
            ema_ref(ref, pair.step(pair.grad(g), step), step, DECAY, True)
        pair.check()
        got = _bits(pair.ema)
        keep = torch.ones(n, dtype=torch.bool)
        for lo, hi in frozen:
            assert bool((got[lo:hi] == SENTINEL).all()), (n, lo, hi)
            keep[lo:hi] = False
        assert torch.equal(got[keep], _bits(ref)[keep]), n
    assert runs[-1][3] is True and frozen[-1] == (1024, 1027)    # the last case: the scalar tail in a frozen run


# ----------------------------------------------------------------------------- 4. switched on late
@pytest.mark.parametrize("mode", ["plain", "grouped+guarded"])
def test_ema_step0_equals_the_reference_started_at_that_step(ops, mode):
    p0, grads = _host(N)
    pair = _Pair(ops, N, mode, True, step0=5)
    ref = p0.clone()
    for i, g in enumerate(grads, 1):
        ema_ref(ref, pair.step(pair.grad(g), 5 + i), i, DECAY, True)
        assert _same_bits(pair.ema, ref), (mode, i)
    pair.check()


# ----------------------------------------------------------------------------- 5. argument errors of the C entry
def test_argument_errors_are_error_codes(ops):
    from tdeed_amd._lib import HipCallError
    n = 1027
    p, g, m, v, e = (torch.zeros(n, device=DEV) for _ in range(5))
    for kw, msg in ((dict(ema_decay=0.0), "0 < ema_decay < 1"), (dict(ema_decay=1.0), "0 < ema_decay < 1"),
                    (dict(ema_decay=float("nan")), "0 < ema_decay < 1"), (dict(ema_step0=-1), "ema_step0"),
                    (dict(ema_step0=3), "step - ema_step0 >= 1")):
        args = dict(ema_decay=DECAY, ema_step0=0)
        args.update(kw)
        with pytest.raises(HipCallError, match=msg):
            ops.adamw_step_ema(p, g, m, v, 3, LR, e, args["ema_decay"], False, args["ema_step0"])
    big = torch.zeros(n + 4, device=DEV)
    with pytest.raises(HipCallError, match="16-byte aligned"):
        ops.adamw_step_ema(p, g, m, v, 1, LR, big[1:n + 1], DECAY)
    with pytest.raises(ValueError, match="one length"):
        ops.adamw_step_ema(p, g, m, v, 1, LR, big, DECAY)
    with pytest.raises(HipCallError, match="bad n/step"):
        ops.adamw_step_ema(p, g, m, v, 0, LR, e, DECAY)
    torch.cuda.synchronize()
    assert float(p.abs().sum()) == 0.0 and float(e.abs().sum()) == 0.0      # nothing was launched


# ----------------------------------------------------------------------------- 6. ema_tensors
COUNTS = [1, 3, 24, 368, 1000]


def _rows(seed=3):
    """sources at 4-byte-aligned ODD element offsets of one larger buffer"""
    rng = np.random.default_rng(seed)
    big = torch.from_numpy(rng.standard_normal(4096).astype(np.float32)).to(DEV)
    offs, cur = [], 1
    for c in COUNTS:
        offs.append(cur)
        cur += c + (2 if (cur + c) % 2 else 1)                   # the next start is odd again
    assert all(o % 2 == 1 for o in offs) and cur < 4096
    return big, [big[o:o + c] for o, c in zip(offs, COUNTS)], offs


def test_ema_tensors_rows_equal_ema_ref(ops):
    big, srcs, offs = _rows()
    table = ops.ema_tensor_table(srcs)
    assert table.total == sum(COUNTS) and table.offsets == [0, 1, 4, 28, 396] and tuple(table.dev.shape) == (5, 4)
    rng = np.random.default_rng(4)
    start = torch.from_numpy(rng.standard_normal(table.total).astype(np.float32))
    for warmup in (False, True):
        shadow, ref = start.clone().to(DEV), start.clone()
        for step in (1, 2, 3):
            big.copy_(torch.from_numpy(rng.standard_normal(4096).astype(np.float32)))
            ops.ema_tensors(table, shadow, step, DECAY, warmup)
            torch.cuda.synchronize()
            for s, o, c in zip(srcs, table.offsets, COUNTS):
                ema_ref(ref[o:o + c], s.cpu(), step, DECAY, warmup)
            assert _same_bits(shadow, ref), (warmup, step)
        assert not _same_bits(shadow, start)
    # rows placed by hand, with gaps: the gaps keep their bits
    gaps = [5, 10, 20, 60, 500]
    table2 = ops.ema_tensor_table(srcs, offsets=gaps)
    shadow = torch.zeros(1500, device=DEV)
    shadow.view(torch.int32).fill_(SENTINEL)
    for o, c in zip(gaps, COUNTS):
        shadow[o:o + c] = 0.0
    ops.ema_tensors(table2, shadow, 1, DECAY, True)
    got = _bits(shadow)
    used = torch.zeros(1500, dtype=torch.bool)
    for s, o, c in zip(srcs, gaps, COUNTS):
        assert _same_bits(shadow[o:o + c], ema_ref(torch.zeros(c), s.cpu(), 1, DECAY, True)), c
        used[o:o + c] = True
    assert bool((got[~used] == SENTINEL).all())


def test_ema_tensors_skipped_record_and_overrun(ops):
    from tdeed_amd._lib import HipCallError
    big, srcs, offs = _rows()
    table = ops.ema_tensor_table(srcs)
    start = torch.from_numpy(np.random.default_rng(4).standard_normal(table.total).astype(np.float32))
    shadow = start.clone().to(DEV)
    # the record of a step that was skipped: nonfinite = 1, skipped = 1
    rec = torch.tensor([0, 0, 1, 1, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    ops.ema_tensors(table, shadow, 1, DECAY, True, guard=rec, skip_nonfinite=True)
    torch.cuda.synchronize()
    assert _same_bits(shadow, start)
    # the next, applied step is update n = 2 - 1 = 1
    rec = torch.tensor([0, 0, 0, 1, 0, 0, 0, 0], dtype=torch.int32, device=DEV)
    ops.ema_tensors(table, shadow, 2, DECAY, True, guard=rec, skip_nonfinite=True)
    ref = start.clone()
    for s, o, c in zip(srcs, table.offsets, COUNTS):
        ema_ref(ref[o:o + c], s.cpu(), 1, DECAY, True)
    assert _same_bits(shadow, ref) and not _same_bits(shadow, start)
    # a row that overruns the shadow is refused, nothing is launched
    short = start[:table.total - 1].clone().to(DEV)
    with pytest.raises(HipCallError, match="overruns the shadow"):
        ops.ema_tensors(table, short, 1, DECAY)
    torch.cuda.synchronize()
    assert _same_bits(short, start[:table.total - 1])
    with pytest.raises(HipCallError, match="0 < ema_decay < 1"):
        ops.ema_tensors(table, shadow, 1, 1.0)
    with pytest.raises(HipCallError, match="step - ema_step0 >= 1"):
        ops.ema_tensors(table, shadow, 2, DECAY, False, 2)


# ----------------------------------------------------------------------------- 7. engine, eager and captured
def _batch(rank=0):
    B, T = 2, CFG["clip_len"]
    frames = t(synth.uint8_clip(1300 + rank, (B, T, 3, 64, 64)))
    lab, labD = synth.labels(1400 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
    return frames, t(lab).long(), t(labD).float()


def _engine(device=DEV, groups=None, frozen_stats="batch", ema=(DECAY, True)):
    from tdeed_amd.trainer import TrainEngine
    sd = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}
    eng = TrainEngine(CFG, sd, act_dtype=torch.float32, device=device, lr=1e-3)
    if groups is not None:
        eng.set_groups(groups, frozen_stats=frozen_stats)
    if ema is not None:
        eng.set_ema(*ema)
    return eng


def _stats(eng):
    return torch.cat([eng.state[k].reshape(-1) for k in eng.ema_stat_index]).cpu()


def _one_step(eng, graph, rank=0):
    frames, lab, labD = (x.to(DEV) for x in _batch(rank))
    if graph:
        eng.make_step(frames.shape[0], 64, 64, frames, lab, labD, None, use_graph=True)()
    else:
        eng.step(frames, lab, labD)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _three_steps(graph):
    """Three steps of a fresh engine with EMA (warmup on), eager or captured: the shadows after them, and ema_ref run over
    the snapshots of the live buffers taken after each step.  Computed once, left unchanged."""
    eng = _engine()
    assert eng.opt.ema_step0 == 0 and _same_bits(eng.opt.ema, eng.params.flat) and _same_bits(eng.ema_stats, _stats(eng))
    ref_p, ref_s = eng.params.flat.cpu().clone(), _stats(eng).clone()
    start = ref_p.clone()
    for step, rank in enumerate((0, 1, 0), 1):
        _one_step(eng, graph, rank)
        ema_ref(ref_p, eng.params.flat.cpu(), step, DECAY, True)
        ema_ref(ref_s, _stats(eng), step, DECAY, True)
    return dict(ema=eng.opt.ema.cpu(), stats=eng.ema_stats.cpu(), ref_p=ref_p, ref_s=ref_s, start=start,
                flat=eng.params.flat.cpu(), mode=eng.last_graph.mode if graph else None)


@pytest.mark.parametrize("graph", [False, True])
def test_engine_shadows_equal_ema_ref_over_the_snapshots(graph):
    got = _three_steps(graph)
    assert _same_bits(got["ema"], got["ref_p"]) and _same_bits(got["stats"], got["ref_s"])
    assert not _same_bits(got["ema"], got["start"]) and not _same_bits(got["ema"], got["flat"])
    assert graph == (got["mode"] is not None)


def test_engine_shadows_agree_between_the_eager_and_the_captured_step():
    a, b = _three_steps(False), _three_steps(True)
    assert _same_bits(a["ema"], b["ema"]) and _same_bits(a["stats"], b["stats"])


# ----------------------------------------------------------------------------- 8. frozen trunk in eval mode
def test_frozen_eval_trunk_keeps_its_part_of_both_shadows():
    eng = _engine(groups=TRUNK, frozen_stats="eval")
    p0, s0 = eng.opt.ema.cpu().clone(), eng.ema_stats.cpu().clone()
    for rank in (0, 1, 0):
        _one_step(eng, False, rank)
    ema, stats = eng.opt.ema.cpu(), eng.ema_stats.cpu()
    moved = 0
    for k, (o, n) in eng.params.index.items():
        if k in eng.frozen:
            assert k.startswith("_features.") and _same_bits(ema[o:o + n], p0[o:o + n]), k
        else:
            moved += int(not _same_bits(ema[o:o + n], p0[o:o + n]))
    assert len(eng.frozen) > 100 and moved > 0.9 * (len(eng.params.index) - len(eng.frozen))
    trunk_stats = [k for k in eng.ema_stat_index if k.startswith("_features.")]
    assert len(trunk_stats) > 50
    for k in trunk_stats:
        o, n = eng.ema_stat_index[k]
        assert _same_bits(stats[o:o + n], s0[o:o + n]), k


# ----------------------------------------------------------------------------- 9 - 11. the public interface
def _model(state=None):
    from tdeed_amd import augment
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(CFG))
    m._train_dtype = torch.float32
    m.load({k: t(v) for k, v in model_state(CFG, 17).items()} if state is None else state)
    m._model.augment_fn = augment.crop_only
    m._model.dropout_mask_fn = lambda B, T, C, n: drop_masks(77, B, T, C, n)
    return m


def _batches():
    out = []
    for rank in (0, 1):
        frames, lab, labD = _batch(rank)
        out.append(dict(frame=frames, label=lab, labelD=labD))
    return out


def test_averaged_scores_with_the_shadow_and_touches_no_live_bit():
    batches = _batches()
    m = _model()
    opt, _ = m.get_optimizer({"lr": 1e-3, "ema_decay": 0.9, "ema_warmup": True})
    g0 = opt.param_groups[0]
    assert g0["ema_decay"] == 0.9 and g0["ema_warmup"] is True
    m.epoch(batches, optimizer=opt)
    torch.cuda.synchronize()
    assert opt.engine.opt.t == 2
    clip = batches[0]["frame"]
    live_before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    _, before = m.predict(clip, use_amp=False)
    with m.averaged():
        _, inside = m.predict(clip, use_amp=False)
        eng_a = m._model.engine(torch.float32)
        _, again = m.predict(clip, use_amp=False)
        assert m._model.engine(torch.float32) is eng_a           # the cache: no step since, no rebuild
        with pytest.raises(RuntimeError, match="inside averaged"):
            m.epoch(batches, optimizer=opt)
        m._model.train()
        with pytest.raises(RuntimeError, match="inside averaged"):
            m._model(clip.to(DEV), inference=False)
        m._model.eval()
    _, after = m.predict(clip, use_amp=False)
    assert m._model.engine(torch.float32) is not eng_a
    ema_sd = m.ema_state_dict()
    assert list(ema_sd) == list(m.state_dict())
    fresh = _model({k: v.detach().cpu().clone() for k, v in ema_sd.items()})
    _, want = fresh.predict(clip, use_amp=False)
    assert np.array_equal(inside.view(np.int32), want.view(np.int32)) and np.array_equal(inside.view(np.int32), again.view(np.int32))
    assert not np.array_equal(inside, before)
    assert np.array_equal(before.view(np.int32), after.view(np.int32))
    # the whole-video route and the validation pass take the same engines
    video = torch.cat([b["frame"].reshape(-1, 3, 64, 64) for b in batches])       # 24 frames
    live_track, _ = m.predict_video(video, use_amp=False)
    live_loss = m.epoch(batches)
    with m.averaged():
        track, support = m.predict_video(video, use_amp=False)
        loss = m.epoch(batches)
    want_track, want_support = fresh.predict_video(video, use_amp=False)
    assert np.array_equal(track.view(np.int32), want_track.view(np.int32)) and np.array_equal(support, want_support)
    assert not np.array_equal(track, live_track)
    assert loss == fresh.epoch(batches) and loss != live_loss
    for k, v in m.state_dict().items():
        assert torch.equal(v, live_before[k]), k
    # one more step: the averaged engines are rebuilt, the scores move
    m.epoch(batches[:1], optimizer=opt)
    with m.averaged():
        assert m._model.engine(torch.float32) is not eng_a
        _, later = m.predict(clip, use_amp=False)
    assert not np.array_equal(later, inside)


def test_averaged_without_ema_raises():
    m = _model()
    with pytest.raises(RuntimeError, match="no EMA"):
        with m.averaged():
            pass
    opt, _ = m.get_optimizer({"lr": 1e-3})
    with pytest.raises(RuntimeError, match="no EMA"):
        with m.averaged():
            pass
    with pytest.raises(RuntimeError, match="no EMA"):
        m.ema_state_dict()
    with pytest.raises(ValueError, match="ema_decay"):
        _model().get_optimizer({"lr": 1e-3, "ema_decay": 1.0})


def test_state_dict_round_trip_carries_the_shadows():
    """Save after two steps, load into a fresh model + an optimizer built WITHOUT EMA, one more step on both: every
    parameter, moment and shadow bit is equal."""
    batches = _batches()
    m = _model()
    opt, _ = m.get_optimizer({"lr": 3e-4, "ema_decay": DECAY, "ema_warmup": True, "skip_nonfinite": True})
    m.epoch(batches, optimizer=opt)
    torch.cuda.synchronize()
    sd = opt.state_dict()
    f = sd["fused"]
    assert f["ema_step0"] == 0 and f["ema_decay"] == DECAY and f["ema_warmup"] is True and f["t"] == 2
    assert _same_bits(f["ema"], opt.engine.opt.ema) and _same_bits(f["ema_stats"], opt.engine.ema_stats)
    assert sd["param_groups"][0]["ema_decay"] == DECAY and sd["param_groups"][0]["ema_warmup"] is True
    m2 = _model({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    opt2, _ = m2.get_optimizer({"lr": 3e-4})
    assert "ema_decay" not in opt2.param_groups[0] and opt2.engine.opt.ema is None and opt2.engine.ema_stats is None
    opt2.load_state_dict(sd)
    a, b = opt.engine, opt2.engine
    assert opt2.param_groups[0]["ema_decay"] == DECAY and b.opt.ema_step0 == 0
    assert _same_bits(a.opt.ema, b.opt.ema) and _same_bits(a.ema_stats, b.ema_stats)
    for mm, oo in ((m, opt), (m2, opt2)):
        mm.epoch(batches[:1], optimizer=oo)
    torch.cuda.synchronize()
    assert a.opt.t == 3 and b.opt.t == 3
    for x, y, what in ((a.params.flat, b.params.flat, "flat"), (a.opt.exp_avg, b.opt.exp_avg, "m"),
                       (a.opt.exp_avg_sq, b.opt.exp_avg_sq, "v"), (a.opt.ema, b.opt.ema, "ema"),
                       (a.ema_stats, b.ema_stats, "ema_stats")):
        assert _same_bits(x, y), what
    assert not _same_bits(a.opt.ema, f["ema"]) and not _same_bits(a.ema_stats, f["ema_stats"])
    # switching it off through param_groups[0] drops the buffers at the next step
    opt2.param_groups[0].pop("ema_decay")
    opt2.param_groups[0].pop("ema_warmup")
    m2.epoch(batches[:1], optimizer=opt2)
    assert b.opt.ema is None and b.ema_stats is None and "ema" not in opt2.state_dict()["fused"]


# ----------------------------------------------------------------------------- 12. without the keyword nothing differs
def test_without_ema_decay_nothing_differs(ops):
    from tdeed_amd import _lib
    m = _model()
    opt, _ = m.get_optimizer({"lr": 1e-3})
    eng = opt.engine
    assert eng.opt.ema is None and eng.ema_stats is None and eng.opt.ema_hook is None
    assert "ema_decay" not in opt.param_groups[0] and "ema_warmup" not in opt.param_groups[0]
    assert set(eng.opt.state_dict()) == {"exp_avg", "exp_avg_sq", "t", "skipped"}
    frames, lab, labD = (x.to(DEV) for x in _batch())
    a, b = _engine(ema=None), _engine(ema=None)
    with _lib.profile() as prof:
        a.step(frames, lab, labD)
    names = {rec[0] for rec in prof.rec}
    assert "tdeed_adamw_step" in names and not names & {"tdeed_adamw_step_ema", "tdeed_ema_tensors"}, sorted(names)
    assert a.opt.ema is None and a.ema_stats is None
    # the twin: the same accumulate, then the plain launch called directly, as FusedAdamW.step() does without EMA
    b.accumulate(frames, lab, labD)
    ops.adamw_step(b.params.flat, b.params.grad, b.opt.exp_avg, b.opt.exp_avg_sq, 1, 1e-3, weight_decay=0.01)
    torch.cuda.synchronize()
    assert _same_bits(a.params.flat, b.params.flat) and _same_bits(a.opt.exp_avg, b.opt.exp_avg)
    assert _same_bits(a.opt.exp_avg_sq, b.opt.exp_avg_sq)
    # with EMA on, the census names both new entries and not the plain one
    c = _engine()
    with _lib.profile() as prof:
        c.step(frames, lab, labD)
    names = {rec[0] for rec in prof.rec}
    assert {"tdeed_adamw_step_ema", "tdeed_ema_tensors"} <= names and "tdeed_adamw_step" not in names
    assert _same_bits(c.params.flat, a.params.flat)              # and the parameters are the same bits


# ----------------------------------------------------------------------------- 13. two ranks on one GPU over gloo
def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from tdeed_amd import dist as tdist
    torch.cuda.set_device(0)                                     # both ranks share the one GPU
    tdist.init(backend="gloo")
    eng = _engine("cuda:0")
    red = eng.set_reducer("auto")
    assert red is not None and red.world == world
    start = eng.opt.ema.detach().cpu().numpy().copy()
    for _ in range(2):
        frames, lab, labD = (x.to("cuda:0") for x in _batch(rank))
        eng.step(frames, lab, labD)
    torch.cuda.synchronize()
    q.put((rank, dict(ema=eng.opt.ema.detach().cpu().numpy(), flat=eng.params.flat.detach().cpu().numpy(), start=start,
                      stats=eng.ema_stats.detach().cpu().numpy())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_the_same_parameter_shadow():
    """Two ranks and this process: three processes hold the GPU.  The ranks see different batches; their parameters and
    the scalars of the EMA agree, so the parameter shadows are equal bit for bit without a collective.  The statistics
    shadows are per rank, like the live running statistics."""
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
    a, b = res[0][1], res[1][1]
    assert np.array_equal(a["flat"].view(np.int32), b["flat"].view(np.int32))
    assert np.array_equal(a["ema"].view(np.int32), b["ema"].view(np.int32))
    assert not np.array_equal(a["ema"], a["start"]) and not np.array_equal(a["ema"], a["flat"])
    assert not np.array_equal(a["stats"], b["stats"])            # different batches: per-rank statistics
