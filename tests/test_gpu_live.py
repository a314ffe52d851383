"""Live scoring on the MI355X: the incremental stitch kernel (ops.stitch_live) bit for bit against its numpy twin
(`liveplan.live_stitch_ref`) and against ONE ops.stitch_scores_seg launch over the whole clip list, with the score ring at its
minimum; and `TDEEDModel.live_scorer` bit for bit against `predict_video` on the complete video, for several ways of cutting
the video into pushes, with both rings at their minimum.  Every comparison is exact.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import model_state, t, cfg_ns
from tdeed_amd import evalutil as E
from tdeed_amd import liveplan as LP
from tdeed_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _patterns(L):
    out = {"ones": [1] * L, "fives": [5] * (L // 5) + ([L % 5] if L % 5 else []), "all": [L]}
    if L > 7:
        out["tail7"] = [L - 7, 7]
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------- 1. the kernel
def _clip_scores(n, V, T, K1, seed):
    rng = np.random.default_rng(seed)
    sc = rng.standard_normal((V, n, T, K1)).astype(np.float32) * np.float32(3)
    sc[rng.random((V, n, T)) < 0.25] = 0                          # all-zero rows: not counted when count_all = 0
    return sc


def _whole_list(scores, starts, L, count_all):
    """one stitch_scores_seg launch over the whole clip list -> (sums, support, mean) numpy"""
    sd = torch.tensor(starts, dtype=torch.int32, device=DEV)
    seg, coff = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in ([0, L], [0, len(starts)]))
    out = ops.stitch_scores_seg(torch.from_numpy(scores).to(DEV), sd, seg, coff, L, count_all=count_all, mean=True)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def _live(scores, L, T, ov, pad, bs, pattern, count_all, R=None):
    """the launches of liveplan.LiveSchedule through ops.stitch_live, every launch compared with the twin on its own numpy
    rings -> (sums, support, mean) concatenated, the launches"""
    V, n, _, K1 = scores.shape
    R = LP.track_ring_rows(bs, T, ov) if R is None else R
    ring_sum = torch.zeros((R, K1), dtype=torch.float32, device=DEV)
    ring_sup = torch.zeros((R,), dtype=torch.int32, device=DEV)
    ref_sum, ref_sup = np.zeros((R, K1), np.float32), np.zeros(R, np.int32)
    dev_scores = torch.from_numpy(scores).to(DEV)
    sched = LP.LiveSchedule(T, ov, pad, bs)
    parts, launches = [], []

    def run(todo):
        for x in todo:
            B, a = len(x["starts"]), x["first"]
            batch = dev_scores[:, a:a + B].contiguous() if B else None
            sd = torch.tensor(x["starts"], dtype=torch.int32, device=DEV) if B else None
            got = ops.stitch_live(ring_sum, ring_sup, batch, sd, count_all, x["lo"], x["final_hi"], x["limit"], T=T)
            torch.cuda.synchronize()
            got = tuple(g.cpu().numpy() for g in got)
            want = LP.live_stitch_ref(ref_sum, ref_sup, scores[:, a:a + B] if B else None, x["starts"], count_all, x["lo"],
                                      x["final_hi"], x["limit"])
            for g, w in zip(got, want):
                assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)), x
            assert np.array_equal(_bits(ring_sum.cpu().numpy()), _bits(ref_sum)) and np.array_equal(ring_sup.cpu().numpy(), ref_sup)
            parts.append(got)
            launches.append(x)
    for m in pattern:
        run(sched.push(m))
    run(sched.close())
    assert sched.scored == n and sched.rows_final == L
    assert not ref_sum.any() and not ref_sup.any()
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), launches


def _check_live(T, ov, pad, bs, L, V, K1, seed, patterns=None):
    starts = E.video_clip_starts(L, T, ov, pad_len=pad)
    scores = _clip_scores(len(starts), V, T, K1, seed)
    count_all = V > 1
    want = _whole_list(scores, starts, L, count_all)
    assert want[0].any() and int(want[1].max()) >= 1
    seen = []
    for name, pattern in _patterns(L).items():
        if patterns is not None and name not in patterns:
            continue
        got, launches = _live(scores, L, T, ov, pad, bs, pattern, count_all)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), name
        seen.append(launches)
    return seen


@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("ov,pad,bs", [(4, 5, 1), (3, 0, 3), (0, 2, 2)])
def test_stitch_live_equals_its_twin_and_one_launch_over_the_whole_list(ov, pad, bs, V):
    T, L = 6, 41
    assert L >= 3 * LP.track_ring_rows(bs, T, ov)                 # every ring row is reused at least three times
    _check_live(T, ov, pad, bs, L, V, 4, 100 * ov + V)


def test_stitch_live_300_rows_per_launch_across_a_workgroup_boundary():
    T, ov, bs = 6, 0, 50
    assert LP.track_ring_rows(bs, T, ov) == 300 > 256
    for launches in _check_live(T, ov, 0, bs, 700, 2, 4, 5, patterns=("fives", "all")):
        full = [x for x in launches if len(x["starts"]) == bs]
        assert len(full) == 2 and all(x["final_hi"] - x["lo"] == 300 for x in full)


def test_stitch_live_with_no_clips_emits_the_rows_left_at_close():
    # T = 6, overlap 3, no padding, 12 frames: the clips 0, 3, 6 are all complete at the last push, rows 9..11 are still open
    for launches in _check_live(6, 3, 0, 1, 12, 1, 4, 9):
        assert launches[-1]["starts"] == [] and (launches[-1]["lo"], launches[-1]["final_hi"]) == (9, 12)
    # rows no clip has touched come out as zeros with support 0, from a ring that is all zero
    ring_sum = torch.zeros((6, 4), dtype=torch.float32, device=DEV)
    ring_sup = torch.zeros((6,), dtype=torch.int32, device=DEV)
    sums, sup, mean = ops.stitch_live(ring_sum, ring_sup, None, None, False, 2, 5, 7, T=6)
    torch.cuda.synchronize()
    assert sums.shape == (3, 4) and not sums.any() and not sup.any() and not mean.any()


def test_stitch_live_single_column():
    _check_live(6, 4, 5, 2, 41, 1, 1, 17)
    _check_live(6, 4, 5, 2, 41, 2, 1, 18, patterns=("fives",))


def test_stitch_live_checks_its_arguments(monkeypatch):
    from tdeed_amd import _lib
    launched = []
    real = _lib.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    ring_sum = torch.zeros((8, 4), dtype=torch.float32, device=DEV)
    ring_sup = torch.zeros((8,), dtype=torch.int32, device=DEV)
    sc = torch.zeros((1, 2, 6, 4), dtype=torch.float32, device=DEV)
    sd = torch.zeros((2,), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="become final"):
        ops.stitch_live(ring_sum, ring_sup, sc, sd, False, 3, 2, 9)               # final_hi < lo
    with pytest.raises(ValueError, match="become final"):
        ops.stitch_live(ring_sum, ring_sup, sc, sd, False, 0, 9, 9)               # more rows than the ring has
    with pytest.raises(ValueError, match="become final"):
        ops.stitch_live(ring_sum, ring_sup, sc, sd, False, 0, 4, 3)               # final rows past the frames that exist
    with pytest.raises(ValueError):
        ops.stitch_live(ring_sum, ring_sup[:7], sc, sd, False, 0, 2, 9)
    with pytest.raises(ValueError):
        ops.stitch_live(ring_sum, ring_sup, sc, sd[:1], False, 0, 2, 9)
    with pytest.raises(ValueError):
        ops.stitch_live(ring_sum, ring_sup, sc[..., :3].contiguous(), sd, False, 0, 2, 9)
    with pytest.raises(TypeError):
        ops.stitch_live(ring_sum, ring_sup, sc.double(), sd, False, 0, 2, 9)
    with pytest.raises(ValueError):
        ops.stitch_live(ring_sum, ring_sup, None, None, False, 0, 2, 9)           # no scores: T is needed
    assert not launched


# ----------------------------------------------------------------------------- 2. the model
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)                          # the configuration of test_gpu_video.py
T8 = 8
SHAPE = (3, 64, 64)
FB = 3 * 64 * 64
PER = 3                                                   # frames per staged chunk
LEN = 37


@pytest.fixture(scope="module")
def tiny_model():
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(TINY))
    m.load({k: t(v) for k, v in model_state(TINY, 0).items()})
    m.video_chunk_bytes = PER * FB
    return m


def _video(L, seed):
    """every byte non-zero: a stale ring row cannot pass for padding"""
    return (ops.fill_u8_hash((L,) + SHAPE, seed, DEV) % 255 + 1).to(torch.uint8).cpu()


@pytest.fixture(scope="module")
def tiny_video():
    v = _video(LEN, 23)
    assert int(v.min()) >= 1
    return v


_REFS = {}


def _whole(m, video, key, **kw):
    """predict_video on the complete video, once per setting"""
    if key not in _REFS:
        _REFS[key] = m.predict_video(video, **kw)
    return _REFS[key]


def _ov(overlap_len):
    return T8 // 4 * 3 if overlap_len is None else overlap_len


def _min_ring(bs, overlap_len):
    return LP.frame_ring_rows(bs, PER, T8, _ov(overlap_len))


def _push_all(sc, video, pattern, bs, ov, pad):
    """the pushes of `pattern` and close() -> the concatenated (sums, support, mean); checks the bookkeeping after every push"""
    parts, rows, at = [], 0, 0
    for k in pattern:
        first, sums, sup, mean = sc.push(video[at:at + k])
        at += k
        assert first == rows and sums.shape[0] == sup.shape[0] == mean.shape[0]       # consecutive: nothing comes back twice
        rows += sums.shape[0]
        scored = LP.clips_ready(at, T8, ov, pad) // bs * bs
        assert sc.frames_pushed == at and sc.rows_final == rows == LP.final_rows(scored, T8, ov, pad)
        assert rows >= at - sc.latency_frames
        stats = sc.last_push_stats
        assert stats["rows"] == sums.shape[0] and stats["host_syncs"] == (1 if stats["batches"] else 0)
        assert stats["frames_h2d_bytes"] == (0 if video.is_cuda else k * FB)
        parts.append((sums, sup, mean))
    first, sums, sup, mean = sc.close()
    assert first == rows and rows + sums.shape[0] == sc.rows_final == at
    parts.append((sums, sup, mean))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def _same_track(got, want):
    sums, sup, mean = got
    assert sums.dtype == np.float32 and sup.dtype == np.int32 and mean.dtype == np.float32
    assert sums.shape == want[0].shape and np.array_equal(sup, want[1])
    assert np.array_equal(_bits(sums), _bits(want[0])), float(np.abs(sums - want[0]).max())
    want_mean = want[0] / np.maximum(want[1], 1)[:, None].astype(np.float32)       # what stitch_scores(mean=True) divides
    assert np.array_equal(_bits(mean), _bits(want_mean))
    assert float(np.abs(sums).sum()) > 0 and int(sup.max()) >= 1


# every value of every axis at least once: batch_size 1 / 2 / 4, augment, use_amp, the three (overlap_len, pad_len), host
# (pageable and pinned) and device frames, the four ways of cutting the video
SWEEP = [
    (1, False, True, (None, 5), "pageable", "ones"),
    (2, True, True, (0, 0), "device", "fives"),
    (4, False, False, (6, 5), "pinned", "tail7"),
    (4, True, True, (None, 5), "pageable", "all"),
    (2, False, False, (6, 5), "device", "ones"),
    (1, True, False, (0, 0), "pageable", "fives"),
    (2, False, True, (0, 0), "pinned", "all"),
]


@pytest.mark.parametrize("bs,augment,use_amp,grid,source,pattern", SWEEP,
                         ids=[f"b{c[0]}-{'aug' if c[1] else 'plain'}-{'bf16' if c[2] else 'fp32'}-ov{c[3][0]}-pad{c[3][1]}-{c[4]}-{c[5]}"
                              for c in SWEEP])
def test_live_rows_equal_predict_video_bit_for_bit(tiny_model, tiny_video, bs, augment, use_amp, grid, source, pattern):
    m = tiny_model
    overlap_len, pad = grid
    kw = dict(overlap_len=overlap_len, pad_len=pad, batch_size=bs, augment=augment, use_amp=use_amp)
    want = _whole(m, tiny_video, (bs, augment, use_amp, grid), **kw)
    video = {"pageable": tiny_video, "pinned": tiny_video.pin_memory(), "device": tiny_video.to(DEV)}[source]
    sc = m.live_scorer(SHAPE, ring_frames=_min_ring(bs, overlap_len), **kw)
    assert sc.ring_frames == _min_ring(bs, overlap_len) < LEN
    assert sc.track_rows == LP.track_ring_rows(bs, T8, _ov(overlap_len))
    assert sc.latency_frames == T8 - 1 + (bs - 1) * (T8 - _ov(overlap_len))
    got = _push_all(sc, video, _patterns(LEN)[pattern], bs, _ov(overlap_len), pad)
    _same_track(got, want)


def test_a_video_shorter_than_the_first_clip_comes_back_at_close(tiny_model):
    m = tiny_model
    video = _video(2, 31)                                              # T - pad_len = 3 frames complete the first clip
    want = m.predict_video(video, batch_size=2)
    sc = m.live_scorer(SHAPE, batch_size=2, ring_frames=_min_ring(2, None))
    for k in range(2):
        first, sums, sup, mean = sc.push(video[k:k + 1])
        assert first == 0 and sums.shape == (0, 4) and sup.shape == (0,) and mean.shape == (0, 4)
        assert sc.last_push_stats["host_syncs"] == 0 and sc.rows_final == 0
    first, sums, sup, mean = sc.close()
    assert first == 0 and sc.rows_final == 2 and sc.last_push_stats["batches"] == 2    # clips -5, -3, -1: a batch of 2 and one of 1
    _same_track((sums, sup, mean), want)
    with pytest.raises(RuntimeError):
        sc.push(video)
    with pytest.raises(RuntimeError):
        sc.close()


def test_reset_gives_the_bits_of_a_fresh_scorer(tiny_model, tiny_video):
    m = tiny_model
    second = _video(29, 41)
    kw = dict(batch_size=2, augment=True)
    want = m.predict_video(second, **kw)
    sc = m.live_scorer(SHAPE, ring_frames=_min_ring(2, None), **kw)
    _same_track(_push_all(sc, tiny_video, _patterns(LEN)["fives"], 2, 6, 5), _whole(m, tiny_video, ("reset", 2), **kw))
    for _ in range(2):                                                 # also from the middle of a stream
        sc.reset()
        assert sc.frames_pushed == 0 and sc.rows_final == 0
        _same_track(_push_all(sc, second, _patterns(29)["fives"], 2, 6, 5), want)
        sc.reset()
        sc.push(tiny_video[:20])
    fresh = m.live_scorer(SHAPE, ring_frames=_min_ring(2, None), **kw)
    _same_track(_push_all(fresh, second, [29], 2, 6, 5), want)


def _count_syncs(monkeypatch):
    calls = []
    real_sync, real_dev_sync, real_ev = torch.cuda.Stream.synchronize, torch.cuda.synchronize, torch.cuda.Event.synchronize
    real_item, real_cpu = torch.Tensor.item, torch.Tensor.cpu
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append("stream"), real_sync(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("device"), real_dev_sync(*a, **k))[1])
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: (calls.append("event"), real_ev(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None,
                                                                   real_cpu(self, *a, **k))[1])
    return calls


def test_a_push_that_completes_no_batch_does_not_synchronise(tiny_model, tiny_video, monkeypatch):
    m = tiny_model
    sc = m.live_scorer(SHAPE, batch_size=2, ring_frames=_min_ring(2, None))
    _push_all(sc, tiny_video, [LEN], 2, 6, 5)                          # the warm-up: plans and graphs of this geometry
    sc.reset()
    calls = _count_syncs(monkeypatch)
    for video in (tiny_video, tiny_video.to(DEV)):
        sc.reset()
        sc.push(video[:4])                                             # clip -5 is complete, a batch of 2 is not
        assert sc.last_push_stats == dict(host_syncs=0, batches=0, rows=0, frames_h2d_bytes=0 if video.is_cuda else 4 * FB)
        assert calls == []
        sc.push(video[4:5])                                            # frame 4 completes clip -3 and with it the batch
        assert sc.last_push_stats["host_syncs"] == 1 and sc.last_push_stats["batches"] == 1
        assert calls == ["stream"]
        sc.push(video[5:6])
        assert sc.last_push_stats["host_syncs"] == 0 and calls == ["stream"]
        sc.push(video[6:33])                                           # many batches, fed in pieces: still one synchronisation
        assert sc.last_push_stats["batches"] > 3 and calls == ["stream", "stream"]
        sc.close()
        assert calls == ["stream"] * 3
        del calls[:]


LAUNCHERS = ("clip_gather", "clip_gather_seg", "clip_gather_ring", "rows_gather", "rows_gather_seg", "stitch_live",
             "stitch_scores_seg", "process_prediction")


def test_wrong_arguments_raise_before_any_launch(tiny_model, tiny_video, monkeypatch):
    m = tiny_model
    launched = []
    for name in LAUNCHERS:
        monkeypatch.setattr(ops, name, lambda *a, **k: launched.append(1))
    need = _min_ring(2, None)
    with pytest.raises(ValueError, match=f"ring_frames={need}") as e:
        m.live_scorer(SHAPE, batch_size=2, ring_frames=need - 1)
    assert "live_scorer" in str(e.value)
    for bad in ((64, 64), (1, 64, 64), (3, 0, 64)):
        with pytest.raises(ValueError):
            m.live_scorer(bad)
    with pytest.raises(ValueError):
        m.live_scorer(SHAPE, overlap_len=T8)
    with pytest.raises(ValueError):
        m.live_scorer(SHAPE, pad_len=-1)
    with pytest.raises(ValueError):
        m.live_scorer(SHAPE, batch_size=0)
    with pytest.raises(TypeError):
        m.live_scorer(SHAPE, clip_starts=[0, 2])                           # not offered
    sc = m.live_scorer(SHAPE, batch_size=2, ring_frames=need)
    with pytest.raises(ValueError, match="empty"):
        sc.close()                                                         # nothing pushed: predict_video's "empty video"
    with pytest.raises(TypeError):
        sc.push(tiny_video.float())
    with pytest.raises(TypeError):
        sc.push(tiny_video[0])
    with pytest.raises(ValueError):
        sc.push(tiny_video[:, :, :32])
    with pytest.raises(ValueError):
        sc.push(tiny_video[:0])
    assert sc.frames_pushed == 0 and sc.rows_final == 0
    # a stream predict_video refuses: no padding and no more frames than the overlap -> no clips
    sc = m.live_scorer(SHAPE, overlap_len=6, pad_len=0, batch_size=2)
    sc.push(tiny_video[:6])
    with pytest.raises(ValueError, match="no clips"):
        sc.close()
    with pytest.raises(ValueError, match="no clips"):
        m.predict_video(tiny_video[:6], overlap_len=6, pad_len=0, batch_size=2)
    assert not launched
