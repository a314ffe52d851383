"""Videos longer than the device budget on the MI355X: the ring gather kernel bit for bit against its numpy twin
(`evalutil.clip_gather_ring_ref`), and `predict_video` / `predict_video_group` / `spot_video` with stream_frames=True at the
smallest ring `evalutil.ring_plan` accepts, bit for bit against the resident route.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import model_state, t, cfg_ns
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


def _tables(lengths, clips):
    """clips: (video, local start) pairs -> (starts, clip_base, clip_len_v) as int32 arrays"""
    off = np.concatenate([[0], np.cumsum(lengths)])
    return (np.asarray([s for _, s in clips], np.int32), np.asarray([off[v] for v, _ in clips], np.int32),
            np.asarray([lengths[v] for v, _ in clips], np.int32))


def _video(lengths, shape, seed):
    """every byte non-zero: a byte of a neighbouring video, or of a stale ring row, cannot pass for padding"""
    return (ops.fill_u8_hash((sum(lengths),) + shape, seed, DEV) % 255 + 1).to(torch.uint8).cpu().numpy()


def _run_ring(video, lo, rf, tabs, T):
    ref, ring = E.clip_gather_ring_ref(video, lo, rf, tabs[0], T, tabs[1], tabs[2])
    B = len(tabs[0])
    out = torch.full((B * T,) + video.shape[1:], 9, dtype=torch.uint8, device=DEV)
    ops.clip_gather_ring(torch.from_numpy(ring).to(DEV), rf, video.shape[0], _dev(tabs[0]), _dev(tabs[1]), _dev(tabs[2]), T, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(ref.shape), ref


# ----------------------------------------------------------------------------- 1. the kernel
# L_total = 23 in three videos (packed 0..8 | 9..11 | 12..22), a ring of 6 rows (6 does not divide 23), T = 4.  Per live
# window [lo, lo + 6): clips whose real frames are live -- over a video's front and end (zeros, never the neighbour's
# frames, which ARE in the ring next to them), wholly outside, and across the wrap from row 5 to row 0.
RING_CASES = [
    (8, [(0, 8), (0, 9), (1, -2), (1, 0), (1, 2), (2, -2), (2, -4), (1, -4), (1, 3)]),      # both boundaries inside the window
    (3, [(0, 4), (0, 3), (0, 5), (0, 6), (0, 8)]),                     # packed 4..7 = rows 4, 5, 0, 1; 6..8 + the end of video 0
    (15, [(2, 3), (2, 4), (2, 5)]),                                    # packed 15..18 = rows 3, 4, 5, 0
    (17, [(2, 5), (2, 7), (2, 9), (2, 10), (2, 11)]),                  # the end of the last video: p < L_total
]


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 8, 8)], ids=["bytes_105B", "v16_192B"])
def test_clip_gather_ring_equals_its_numpy_twin(shape):
    lengths, T, rf = [9, 3, 11], 4, 6
    video = _video(lengths, shape, 11)
    assert int(video.min()) >= 1 and video[0].size in (105, 192)
    n_pad = n_real = 0
    for lo, clips in RING_CASES:
        assert lo > 0
        tabs = _tables(lengths, clips)
        got, ref = _run_ring(video, lo, rf, tabs, T)
        assert np.array_equal(got, ref), lo
        pad = sum(1 for b in range(len(clips)) for k in range(T) if int(ref[b, k].max()) == 0)
        n_pad, n_real = n_pad + pad, n_real + len(clips) * T - pad
    assert n_pad > 20 and n_real > 40
    # the windows that straddle the wrap did read rows 5 and 0 one after the other
    got, ref = _run_ring(video, 15, rf, _tables(lengths, [(2, 3)]), T)
    assert np.array_equal(got[0], video[15:19]) and np.array_equal(got, ref)
    # B = 1, T = 1
    got, ref = _run_ring(video, 5, rf, _tables(lengths, [(0, 5)]), 1)
    assert np.array_equal(got, ref) and np.array_equal(got[0, 0], video[5])
    got, ref = _run_ring(video, 5, rf, _tables(lengths, [(1, 3)]), 1)
    assert np.array_equal(got, ref) and int(got.max()) == 0


def test_clip_gather_ring_at_224():
    lengths, T, rf = [5, 14, 4], 8, 12                                # packed 0..4 | 5..18 | 19..22
    video = _video(lengths, (3, 224, 224), 13)
    clips = [(1, 3), (1, 8), (2, -7), (1, 12), (1, 6)]                # 8..15 = rows 8..11, 0..3; the end of video 1; the front of 2
    got, ref = _run_ring(video, 8, rf, _tables(lengths, clips), T)
    assert np.array_equal(got, ref)
    assert np.array_equal(got[0], video[8:16]) and int(got[1, 6:].max()) == 0 and int(got[2, :7].max()) == 0
    assert np.array_equal(got[2, 7], video[19])


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 8, 8)], ids=["bytes_105B", "v16_192B"])
def test_a_ring_that_holds_everything_equals_clip_gather_seg(shape):
    lengths, T = [9, 3, 11], 4
    video = _video(lengths, shape, 17)
    clips = [(v, s) for v, L in enumerate(lengths) for s in (-T, -3, 0, L - 2, L - 1, L, L + 2, 1)]
    tabs = _tables(lengths, clips)
    B = len(clips)
    seg = torch.full((B * T,) + shape, 9, dtype=torch.uint8, device=DEV)
    ops.clip_gather_seg(torch.from_numpy(video).to(DEV), _dev(tabs[0]), _dev(tabs[1]), _dev(tabs[2]), T, seg)
    torch.cuda.synchronize()
    seg = seg.cpu().numpy().reshape((B, T) + shape)
    for rf in (23, 30):
        got, ref = _run_ring(video, 0, rf, tabs, T)
        assert np.array_equal(got, ref) and np.array_equal(got, seg), rf


def test_clip_gather_ring_checks_its_arguments():
    from tdeed_amd._lib import HipCallError
    ring = torch.zeros((6, 3, 4, 4), dtype=torch.uint8, device=DEV)
    tab = torch.zeros((2,), dtype=torch.int32, device=DEV)
    out = torch.empty((2 * 4, 3, 4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="ring_frames"):
        ops.clip_gather_ring(ring, 7, 23, tab, tab, tab, 4, out)                  # the ring has 6 rows
    with pytest.raises(ValueError):
        ops.clip_gather_ring(ring, 6, 23, tab, tab[:1], tab, 4, out)
    with pytest.raises(ValueError):
        ops.clip_gather_ring(ring, 6, 23, tab, tab, tab, 4, out[:5])
    with pytest.raises(TypeError):
        ops.clip_gather_ring(ring, 6, 23, tab.long(), tab, tab, 4, out)
    big = torch.zeros((700,), dtype=torch.int32, device=DEV)
    with pytest.raises(HipCallError, match="65535"):
        ops.clip_gather_ring(ring, 6, 23, big, big, big, 100, torch.empty((700 * 100, 3, 4, 4), dtype=torch.uint8, device=DEV))


# ----------------------------------------------------------------------------- 2. end to end, tiny model
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)                          # the configuration of test_gpu_video.py
CLASSES = {"c1": 1, "c2": 2, "c3": 3}
FB = 3 * 64 * 64
PER = 3                                                   # frames per upload chunk
GROUP = [19, 5, 30]                                       # the 5-frame video is shorter than the clip


def _model(cfg, seed=0):
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m.load({k: t(v) for k, v in model_state(cfg, seed).items()})
    m.video_chunk_bytes = PER * FB
    return m


@pytest.fixture(scope="module")
def tiny_model():
    return _model(TINY)


@pytest.fixture(scope="module")
def tiny_video():
    return t(synth.uint8_clip(4100, (37, 3, 64, 64)))


@pytest.fixture(scope="module")
def tiny_group():
    return [t(synth.uint8_clip(4300 + 100 * i, (L, 3, 64, 64))) for i, L in enumerate(GROUP)]


def _smallest_budget(lengths, batch_size):
    """the smallest budget ring_plan accepts: the widest batch plus the chunk uploaded ahead, in whole chunks"""
    _, _, starts, base, len_v = E.group_clip_table(lengths, 8, 6)
    plan = E.ring_plan(lengths, FB, PER, sum(lengths) * FB - 1, starts, base, len_v, 8, batch_size)
    need = int((plan.last - plan.first).max()) + 2
    budget = need * PER * FB
    assert E.ring_plan(lengths, FB, PER, budget, starts, base, len_v, 8, batch_size).ring_chunks == need
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.ring_plan(lengths, FB, PER, budget - 1, starts, base, len_v, 8, batch_size)
    return budget, need


_REFS = {}


def _resident(m, video, batch_size, augment, use_amp):
    """predict_video with the default budget, once per setting"""
    key = (batch_size, augment, use_amp)
    if key not in _REFS:
        _REFS[key] = m.predict_video(video, batch_size=batch_size, augment=augment, use_amp=use_amp), dict(m.last_video_stats)
    return _REFS[key]


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


@pytest.mark.parametrize("source", ["pageable", "pinned"])
@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("batch_size", [4, 5])
def test_streamed_predict_video_is_bit_identical_to_the_resident_route(tiny_model, tiny_video, batch_size, use_amp, augment,
                                                                        source, monkeypatch):
    m = tiny_model
    (ref_sums, ref_sup), ref_stats = _resident(m, tiny_video, batch_size, augment, use_amp)       # (also the warm-up)
    assert "ring_frames" not in ref_stats
    budget, need = _smallest_budget([37], batch_size)
    assert budget < 37 * FB
    video = tiny_video.pin_memory() if source == "pinned" else tiny_video
    calls = _count_syncs(monkeypatch)
    sums, sup = m.predict_video(video, batch_size=batch_size, augment=augment, use_amp=use_amp, max_resident_bytes=budget,
                                stream_frames=True)
    assert calls == ["stream"]                                        # once per video, like the resident route
    stats = dict(m.last_video_stats)
    assert np.array_equal(sup, ref_sup)
    assert np.array_equal(sums, ref_sums), float(np.abs(sums - ref_sums).max())
    assert float(sums.sum()) > 0 and int(sup.max()) >= 1
    assert stats["ring_chunks"] == need and stats["ring_frames"] == need * PER < 37
    assert stats["resident_bytes"] == need * PER * FB <= budget
    assert stats["frames_h2d_bytes"] == 37 * FB
    ring_keys = ("ring_frames", "ring_chunks", "resident_bytes")
    assert {k: v for k, v in stats.items() if k not in ring_keys} == ref_stats


def test_streamed_group_and_spot_equal_the_resident_routes(tiny_model, tiny_group, tiny_video, monkeypatch):
    m = tiny_model
    ref = m.predict_video_group(tiny_group, batch_size=4, augment=True)
    ref_stats = dict(m.last_video_stats)
    budget, need = _smallest_budget(GROUP, 4)
    assert budget < sum(GROUP) * FB
    mixed = [tiny_group[0], tiny_group[1].pin_memory(), tiny_group[2]]
    for videos in (tiny_group, mixed):
        got = m.predict_video_group(videos, batch_size=4, augment=True, max_resident_bytes=budget, stream_frames=True)
        stats = dict(m.last_video_stats)
        assert len(got) == 3
        for (s0, n0), (s1, n1) in zip(ref, got):
            assert np.array_equal(s0, s1) and np.array_equal(n0, n1)
        assert stats["ring_chunks"] == need and stats["ring_frames"] < sum(GROUP) and stats["resident_bytes"] <= budget
        assert stats["frames_h2d_bytes"] == sum(GROUP) * FB and stats["host_syncs"] == ref_stats["host_syncs"] == 1
        assert stats["batches"] == ref_stats["batches"] and stats["clips"] == ref_stats["clips"]
    # spot_video: identical event lists, two host synchronisations as for the resident route
    want = m.spot_video(tiny_video, CLASSES, batch_size=4, augment=True)
    b1, _ = _smallest_budget([37], 4)
    calls = _count_syncs(monkeypatch)
    out = m.spot_video(tiny_video, CLASSES, batch_size=4, augment=True, max_resident_bytes=b1, stream_frames=True)
    assert calls == ["stream", "stream"]
    assert "ring_frames" in m.last_video_stats and m.last_video_stats["frames_h2d_bytes"] == 37 * FB
    assert np.array_equal(out["pred"], want["pred"]) and out["events"] == want["events"]
    assert out["suppressed"] == want["suppressed"] and sum(len(x) for x in out["suppressed"]) > 0
    # the group form of it, and the mAP-free tail on the streamed group
    want_g = m.spot_video_group(tiny_group, CLASSES, batch_size=4)
    out_g = m.spot_video_group(tiny_group, CLASSES, batch_size=4, max_resident_bytes=budget, stream_frames=True)
    for a, b in zip(want_g, out_g):
        assert np.array_equal(a["pred"], b["pred"]) and a["events"] == b["events"] and a["suppressed"] == b["suppressed"]


def test_evalutil_routes_stream_the_video_over_the_budget(tiny_model, tiny_video):
    m = tiny_model
    lens = {"b": 37, "a": 23, "c": 30}
    frames = {"b": tiny_video, "a": t(synth.uint8_clip(4200, (23, 3, 64, 64))), "c": t(synth.uint8_clip(4300, (30, 3, 64, 64)))}
    vids = [("b", 37, 25.0, frames["b"]), ("a", 23, 30.0, lambda: frames["a"]), ("c", 30, 25.0, frames["c"])]
    truth = [{"video": v, "events": [{"label": "c1", "frame": 3}, {"label": "c2", "frame": 10}, {"label": "c3", "frame": 17},
                                     {"label": "c1", "frame": n - 1}]} for v, n in lens.items()]
    suppress = (("raw",), ("nms", 1, 0.01), ("snms", [3, 1, 2], 0.01))
    kw = dict(augment=True, batch_size=4)
    budget = 30 * FB                                      # "b" is over it, "a" and "c" fit: video by video either way
    want = E.map_videos(m, vids, CLASSES, truth, suppress, [0, 1, 2], **kw)
    ref_stats = dict(m.last_video_stats)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.map_videos(m, vids, CLASSES, truth, suppress, [0, 1, 2], max_resident_bytes=budget, **kw)
    got = E.map_videos(m, vids, CLASSES, truth, suppress, [0, 1, 2], max_resident_bytes=budget, stream_frames=True, **kw)
    stats = dict(m.last_video_stats)
    assert got == want and max(got[0][0]) > 0               # the same tracks: the same APs, bit for bit
    assert stats["ring_chunks"] == 10 and stats["ring_frames"] == 30 and stats["resident_bytes"] == budget
    assert {k: v for k, v in stats.items() if k not in ("ring_frames", "ring_chunks", "resident_bytes")} == ref_stats
    assert stats["host_syncs"] == 4 and stats["groups"] == 3 and stats["frames_h2d_bytes"] == 90 * FB
    st0 = E.stitch_videos(m, vids, 4, **kw)
    st1 = E.stitch_videos(m, vids, 4, max_resident_bytes=budget, stream_frames=True, **kw)
    for name in st0.tracks:
        assert np.array_equal(st0.tracks[name][0], st1.tracks[name][0]) and np.array_equal(st0.tracks[name][1], st1.tracks[name][1])


GATHERS = ("clip_gather", "clip_gather_seg", "clip_gather_ring", "rows_gather", "rows_gather_seg")     # every gather the model may call


def test_a_budget_one_chunk_too_small_raises_before_any_launch(tiny_model, tiny_video, tiny_group, monkeypatch):
    launched = []
    for gather in GATHERS:
        monkeypatch.setattr(ops, gather, lambda *a, **k: launched.append(1))
    budget, need = _smallest_budget([37], 4)
    with pytest.raises(ValueError, match="max_resident_bytes") as e:
        tiny_model.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget - PER * FB, stream_frames=True)
    assert str(budget) in str(e.value) and "predict_video" in str(e.value)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        tiny_model.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget)              # not asked to stream
    with pytest.raises(ValueError, match="ascending order"):
        tiny_model.predict_video(tiny_video, clip_starts=[20, 22, 24, 26, -5, -3, -1, 1], batch_size=4,
                                 max_resident_bytes=30 * FB, stream_frames=True)
    bg, _ = _smallest_budget(GROUP, 4)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        tiny_model.spot_video_group(tiny_group, CLASSES, batch_size=4, max_resident_bytes=bg - 1, stream_frames=True)
    # a video that is on the device already is used where it is: nothing to stream, the budget check stays
    with pytest.raises(ValueError, match="max_resident_bytes"):
        tiny_model.predict_video(tiny_video.to(DEV), batch_size=4, max_resident_bytes=budget, stream_frames=True)
    assert not launched


def test_frames_that_fit_take_the_resident_route(tiny_model, tiny_video, monkeypatch):
    m = tiny_model
    (ref_sums, ref_sup), ref_stats = _resident(m, tiny_video, 4, False, True)
    ring_calls = []
    real = ops.clip_gather_ring
    monkeypatch.setattr(ops, "clip_gather_ring", lambda *a, **k: (ring_calls.append(1), real(*a, **k))[1])
    for budget in (16 << 30, 37 * FB):
        sums, sup = m.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget, stream_frames=True)
        assert dict(m.last_video_stats) == ref_stats and not ring_calls
        assert np.array_equal(sums, ref_sums) and np.array_equal(sup, ref_sup)
    m.predict_video(tiny_video, batch_size=4, max_resident_bytes=37 * FB - 1, stream_frames=True)
    assert ring_calls                                                 # one byte less: the ring


def test_stream_frames_and_reuse_frames_are_not_combined_over_the_budget(tiny_model, tiny_video, monkeypatch):
    m = tiny_model
    launched = []
    budget, _ = _smallest_budget([37], 4)
    with monkeypatch.context() as mp:
        for gather in GATHERS:
            mp.setattr(ops, gather, lambda *a, **k: launched.append(1))
        with pytest.raises(ValueError, match="not combined"):
            m.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget, stream_frames=True, reuse_frames=True)
        with pytest.raises(ValueError, match="not combined"):             # the frames fit, frames + maps do not
            m.predict_video(tiny_video, batch_size=4, max_resident_bytes=37 * FB, stream_frames=True, reuse_frames=True)
        assert not launched
    # everything fits: reuse_frames works as without the keyword
    a = m.predict_video(tiny_video, batch_size=4, reuse_frames=True)
    stats = dict(m.last_video_stats)
    b = m.predict_video(tiny_video, batch_size=4, reuse_frames=True, stream_frames=True)
    assert dict(m.last_video_stats) == stats and "ring_frames" not in stats
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
