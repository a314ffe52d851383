"""A group of videos scored as one packed job on the MI355X: the segmented gather / stitch / event / suppression kernels
against the same video scored alone (a group of one, through the one-video wrappers) and the host chain, `TDEEDModel.predict_video_group` / `spot_video_group` bit for bit against
the clip-batch route on the same packed batches, and `evalutil.spot_videos(group_videos=...)`.  -m gpu only."""
import math

import numpy as np
import pytest
import torch

from helpers import model_state, t, cfg_ns
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth
from test_video_host import stitch_inputs
import test_spot_host as H

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


# ----------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("shape", [(3, 4, 4), (2, 5, 5)], ids=["v16_48B", "bytes_50B"])
def test_clip_gather_seg_pads_at_the_videos_own_ends(shape):
    lengths, T = [1, 5, 37], 4
    mine = [[-3, L - 1, L, L + 2, 0, -T, L - 2] for L in lengths]
    seg_off, clip_off, starts, base, len_v = E.group_clip_table(lengths, T, 3, clip_starts=mine)
    Ltot = int(seg_off[-1])
    # every byte of every frame is non-zero: a byte of the neighbouring video in a window could not pass for padding
    video = (ops.fill_u8_hash((Ltot,) + shape, 5, DEV) % 255 + 1).to(torch.uint8).contiguous()
    assert int(video.min()) >= 1 and video[0].numel() in (48, 50)
    B = len(starts)
    out = torch.full((B * T,) + shape, 9, dtype=torch.uint8, device=DEV)
    ops.clip_gather_seg(video, _dev(starts), _dev(base), _dev(len_v), T, out)
    torch.cuda.synchronize()
    got = out.cpu().view(B, T, *shape)
    host = video.cpu()
    n_pad = 0
    for b in range(B):
        for k in range(T):
            f = int(starts[b]) + k
            if 0 <= f < int(len_v[b]):
                assert torch.equal(got[b, k], host[int(base[b]) + f]), (b, k)
            else:
                assert int(got[b, k].max()) == 0, (b, k, "bytes of another video in the padding")
                n_pad += 1
    assert n_pad > B                                                  # windows over both ends, some wholly outside
    with pytest.raises(ValueError):
        ops.clip_gather_seg(video, _dev(starts), _dev(base)[:3], _dev(len_v), T, out)
    with pytest.raises(ValueError):
        ops.clip_gather_seg(video, _dev(starts), _dev(base), _dev(len_v), T, out[:5])


# ----------------------------------------------------------------------------- 2. stitch
@pytest.mark.parametrize("V", [1, 2])
def test_stitch_scores_seg_equals_the_score_stitcher_per_video(V):
    lengths, T = [1, 63, 64, 65, 300], 8                              # boundaries inside and across 256-thread workgroups
    rs = np.random.RandomState(3)
    mine = []
    for L in lengths:
        s = E.video_clip_starts(L, T, 6) + [L - 3, -T, L]            # over the end, wholly outside
        mine.append([s[i] for i in rs.permutation(len(s))])
    seg_off, clip_off, starts, _, _ = E.group_clip_table(lengths, T, 6, clip_starts=mine)
    n = len(starts)
    _, plain, flip = stitch_inputs(0, starts=list(range(n)), seed=11)
    videos = [(f"v{i}", L, 25.0) for i, L in enumerate(lengths)]
    st = E.ScoreStitcher(videos, 4)
    for v, (name, _, _) in enumerate(videos):
        for i in range(clip_off[v], clip_off[v + 1]):
            if V == 1:
                st.add(name, starts[i], plain[i])
            else:
                st.add_views(name, starts[i], plain[i][None])
                st.add_views(name, starts[i], flip[i][None])
    sc = torch.from_numpy(np.stack([plain, flip][:V])).to(DEV)
    sums, sup, mean = ops.stitch_scores_seg(sc, _dev(starts), _dev(seg_off), _dev(clip_off), int(seg_off[-1]), mean=True)
    torch.cuda.synchronize()
    norm = st.normalised()
    for v, (name, _, _) in enumerate(videos):
        a, b = seg_off[v], seg_off[v + 1]
        assert torch.equal(sums[a:b].cpu(), t(st.tracks[name][0])), name
        assert torch.equal(sup[a:b].cpu(), t(st.tracks[name][1])), name
        assert torch.equal(mean[a:b].cpu(), t(norm[name])), name
    assert float(sums.sum()) > 0
    tw, tw_sup = E.stitch_clip_scores_seg(plain, starts, seg_off, clip_off, flip_scores=flip if V == 2 else None)
    assert np.array_equal(sums.cpu().numpy(), tw) and np.array_equal(sup.cpu().numpy(), tw_sup)


# ----------------------------------------------------------------------------- 3. frame events
def _pack(tracks):
    seg_off = np.concatenate([[0], np.cumsum([x.shape[0] for x in tracks])]).astype(np.int32)
    return torch.from_numpy(np.concatenate(tracks)).to(DEV), seg_off


@pytest.mark.parametrize("K1", [2, 5, 18])
def test_frame_events_seg_equals_frame_events_per_video(K1):
    lengths = [1, 63, 65, 130]                                        # video boundaries inside waves
    n_none = n_some = 0
    for variant, hr in (("uniform", 0.01), ("sharp", 0.3), ("zero_rows", 0.0), ("sharp", 0.6)):
        tracks = [H.make_track(L, K1, variant, 13 * L + K1) for L in lengths]
        mean, seg_off = _pack(tracks)
        pred8 = torch.full((mean.shape[0],), 255, dtype=torch.uint8, device=DEV)
        pred, score, first, count = ops.frame_events_seg(mean, _dev(seg_off), max(lengths), hr, pred_u8=pred8)
        torch.cuda.synchronize()
        assert first.shape == (4, K1) and count.shape == (4, K1)
        for v, L in enumerate(lengths):
            a, b = seg_off[v], seg_off[v + 1]
            p1, s1, f1, c1 = ops.frame_events(mean[a:b].contiguous(), hr)
            assert torch.equal(pred[a:b], p1) and torch.equal(score[a:b], s1), (variant, v)
            assert torch.equal(pred8[a:b].to(torch.int32), p1)
            assert torch.equal(first[v], f1), (variant, v, first[v], f1)
            assert torch.equal(count[v], c1), (variant, v)
            n_none += int((f1[1:] == L).sum())
            n_some += int((f1[1:] < L).sum())
    assert n_none > 0 and n_some > 0                                  # classes without candidates in some videos


# ----------------------------------------------------------------------------- 4. suppression + compaction
def _seg_route(tracks, window, thr, soft, hr):
    mean, seg_off = _pack(tracks)
    sd = _dev(seg_off)
    max_len = max(x.shape[0] for x in tracks)
    first = ops.frame_events_seg(mean, sd, max_len, hr)[2]
    frames, classes, scores, event_off, rounds = ops.nms_track_seg(mean, sd, max_len, window, thr, soft, first, hr)
    torch.cuda.synchronize()
    off = event_off.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= frames.numel()
    assert classes.dtype == torch.uint8 and scores.dtype == torch.float64
    out = []
    for v in range(len(tracks)):
        sl = slice(int(off[v]), int(off[v + 1]))
        out.append((frames[sl].cpu().numpy(), classes[sl].cpu().numpy().astype(np.int32), scores[sl].cpu().numpy(),
                    rounds[v].cpu().numpy()))
    return out, mean, seg_off


def _check_group(tracks, window, thr, soft, hr, tag, host=True):
    got, mean, seg_off = _seg_route(tracks, window, thr, soft, hr)
    n = 0
    for v, x in enumerate(tracks):
        a, b = seg_off[v], seg_off[v + 1]
        one = ops.nms_track(mean[a:b].contiguous(), window, thr, soft, hr)
        torch.cuda.synchronize()
        m = int(one[3].cpu()[0])
        assert np.array_equal(got[v][0], one[0][:m].cpu().numpy()), (tag, v)
        assert np.array_equal(got[v][1], one[1][:m].cpu().numpy()), (tag, v)
        assert np.array_equal(got[v][2], one[2][:m].cpu().numpy()), (tag, v)
        assert np.array_equal(got[v][3], one[4].cpu().numpy()), (tag, v, got[v][3], one[4])
        if host:
            H.check_equal(got[v], H.host_chain(x, window, thr, soft, hr), (tag, v))
        n += m
    return n


@pytest.mark.parametrize("variant", H.VARIANTS)
def test_nms_track_seg_equals_nms_track_and_the_host_chain(variant):
    lengths, K1 = [1, 37, 257, 1025], 5
    tracks = [H.make_track(L, K1, variant, 17 * L + H.VARIANTS.index(variant)) for L in lengths]
    n = 0
    for window, hr in ((3, 0.01), (H.windows_for(K1)[3], 0.2)):        # a scalar and a list window
        for soft in (False, True):
            n += _check_group(tracks, window, 0.05, soft, hr, (variant, window, soft))
    assert n > 0


def test_nms_track_seg_workgroup_sizes_and_single_video():
    """groups whose longest video selects each workgroup size, and a group of one video"""
    lib = ops._lib.load()
    n = 0
    for lengths in ([101, 66, 128], [37, 220, 1], [300, 512, 129], [90]):
        assert lib.tdeed_nms_track_seg_threads(max(lengths)) == {128: 128, 220: 256, 512: 512, 90: 128}[max(lengths)]
        tracks = [H.make_track(L, 5, "sharp", 3 * L + 1) for L in lengths]
        for soft in (False, True):
            n += _check_group(tracks, 2, 0.02, soft, 0.01, (lengths, soft))
    assert n > 0


def test_nms_track_seg_workspace_form():
    """a video longer than the LDS-resident state next to a 37-frame one; a peaky track keeps the rounds short"""
    L = 16001
    assert ops._lib.load().tdeed_nms_track_seg_workspace(L + 37, L, 2) > 0
    rs = np.random.RandomState(5)
    long_track = np.zeros((L, 2), np.float32)
    peaks = rs.choice(L, 400, replace=False)
    long_track[peaks, 1] = rs.rand(400).astype(np.float32) * np.float32(0.9) + np.float32(0.05)
    long_track[peaks[:50] // 2 * 2, 1] = np.float32(0.5)                # ties
    long_track[:, 0] = np.float32(1) - long_track[:, 1]
    tracks = [H.make_track(37, 2, "uniform", 4), long_track]
    n = _check_group(tracks, 5, 0.02, False, 0.01, "workspace hard") + _check_group(tracks, 5, 0.02, True, 0.01, "workspace soft")
    assert n > 100


def test_group_ops_check_their_arguments():
    mean = torch.rand((9, 4), device=DEV)
    seg = _dev([0, 4, 9])
    first = ops.frame_events_seg(mean, seg, 5)[2]
    with pytest.raises(ValueError):
        ops.frame_events_seg(mean, seg, 10)                                               # max_len > packed length
    with pytest.raises(ValueError):
        ops.frame_events_seg(mean, _dev([0]), 5)
    with pytest.raises(TypeError):
        ops.frame_events_seg(mean, seg.long(), 5)
    with pytest.raises(TypeError):
        ops.nms_track_seg(mean.double(), seg, 5, 1, 0.01, False, first)
    with pytest.raises(ValueError):
        ops.nms_track_seg(mean, seg, 5, 0, 0.01, True, first)                             # soft needs a window >= 1
    with pytest.raises(ValueError):
        ops.nms_track_seg(mean, seg, 5, [1, 2], 0.01, False, first)                       # 3 classes, 2 windows
    with pytest.raises(ValueError):
        ops.nms_track_seg(mean, seg, 5, 1, 0.01, False, first[0])                         # one row of first_frame
    with pytest.raises(ValueError, match="65535"):
        ops.nms_track_seg(torch.rand((70000, 2), device=DEV), torch.arange(65537, dtype=torch.int32, device=DEV), 5, 1, 0.01,
                          False, first)
    sc = torch.rand((1, 3, 8, 4), device=DEV)
    with pytest.raises(ValueError):
        ops.stitch_scores_seg(sc, _dev([0, 1]), seg, _dev([0, 1, 3]), 9)                  # 2 starts for 3 clips
    with pytest.raises(ValueError):
        ops.stitch_scores_seg(sc, _dev([0, 1, 2]), seg, _dev([0, 3]), 9)                  # clip_off of another group


# ----------------------------------------------------------------------------- 5. - 8. end to end, tiny model
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)
CLASSES = {"c1": 1, "c2": 2, "c3": 3}
LENGTHS = [37, 23, 9, 1]


def _model(cfg, seed=0):
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m.load({k: t(v) for k, v in model_state(cfg, seed).items()})
    return m


@pytest.fixture(scope="module")
def tiny_model():
    return _model(TINY)


@pytest.fixture(scope="module")
def tiny_videos():
    return [t(synth.uint8_clip(4100 + 100 * i, (L, 3, 64, 64))) for i, L in enumerate(LENGTHS)]


def _window(video, start, T):
    out = torch.zeros((T,) + tuple(video.shape[1:]), dtype=torch.uint8)
    for k in range(T):
        if 0 <= start + k < video.shape[0]:
            out[k] = video[start + k]
    return out


def _yardstick(m, videos, batch_size, augment, use_amp, overlap=None):
    """The existing public path on the SAME packed batches: the group's clip list (video-major) materialised on the host,
    `predict` on batches of `batch_size` cut across the videos, ScoreStitcher.add per clip (plain) or add_views per view,
    plain first (augmented), into the clip's own video.  -> (ScoreStitcher, number of batches)"""
    T = m._args.clip_len
    lengths = [int(v.shape[0]) for v in videos]
    _, clip_off, starts, _, _ = E.group_clip_table(lengths, T, T // 4 * 3 if overlap is None else overlap)
    owner = np.repeat(np.arange(len(videos)), np.diff(clip_off))
    st, batches = None, 0
    for lo in range(0, len(starts), batch_size):
        idx = range(lo, min(lo + batch_size, len(starts)))
        batch = torch.stack([_window(videos[owner[i]], int(starts[i]), T) for i in idx])
        _, sc = m.predict(batch, use_amp=use_amp)
        if st is None:
            st = E.ScoreStitcher([(f"v{v}", L, 25.0) for v, L in enumerate(lengths)], sc.shape[-1])
        if augment:
            _, sf = m.predict(batch, use_amp=use_amp, augment_inference=True)
        for j, i in enumerate(idx):
            if augment:
                st.add_views(f"v{owner[i]}", int(starts[i]), sc[j][None])
                st.add_views(f"v{owner[i]}", int(starts[i]), sf[j][None])
            else:
                st.add(f"v{owner[i]}", int(starts[i]), sc[j])
        batches += 1
    return st, batches


_REFS = {}


def _reference(m, videos, augment, use_amp):
    """the yardstick of one (augment, use_amp) setting, computed once and shared by the tests below"""
    key = (augment, use_amp)
    if key not in _REFS:
        _REFS[key] = _yardstick(m, videos, 4, augment, use_amp)
    return _REFS[key]


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
def test_predict_video_group_is_bit_identical_to_the_clip_route(tiny_model, tiny_videos, use_amp, augment):
    m = tiny_model
    m.video_chunk_bytes = 7 * 3 * 64 * 64                  # several upload chunks, some spanning two videos
    out = m.predict_video_group(tiny_videos, batch_size=4, augment=augment, use_amp=use_amp)
    stats = dict(m.last_video_stats)
    st, batches = _reference(m, tiny_videos, augment, use_amp)
    n_v = [len(E.video_clip_starts(L, 8, 6)) for L in LENGTHS]
    assert n_v == [18, 11, 4, 3]
    assert len(out) == 4
    for v, (sums, sup) in enumerate(out):
        ref_sums, ref_sup = st.tracks[f"v{v}"]
        assert sums.dtype == np.float32 and sums.shape == (LENGTHS[v], 4) and sup.dtype == np.int32 and sup.shape == (LENGTHS[v],)
        assert np.array_equal(sup, ref_sup), v
        assert np.array_equal(sums, ref_sums), (v, float(np.abs(sums - ref_sums).max()))
        assert float(sums.sum()) > 0 and int(sup.max()) >= 1
    assert stats["batches"] == batches == math.ceil(sum(n_v) / 4) == 9 < sum(math.ceil(x / 4) for x in n_v) == 10
    assert stats == dict(frames=70, clips=36, batches=9, views=2 if augment else 1, frames_h2d_bytes=70 * 3 * 64 * 64,
                         videos=4, host_syncs=1)


def test_predict_video_group_frame_sources_clip_starts_and_repeat(tiny_model, tiny_videos):
    m = tiny_model
    m.video_chunk_bytes = 5 * 3 * 64 * 64
    a = m.predict_video_group(tiny_videos, batch_size=4, augment=True)
    b = m.predict_video_group([v.pin_memory() for v in tiny_videos], batch_size=4, augment=True)
    assert m.last_video_stats["frames_h2d_bytes"] == sum(v.numel() for v in tiny_videos)
    c = m.predict_video_group([v.to(DEV) for v in tiny_videos], batch_size=4, augment=True)
    assert m.last_video_stats["frames_h2d_bytes"] == 0
    mixed = [tiny_videos[0], tiny_videos[1].pin_memory(), tiny_videos[2].to(DEV), tiny_videos[3]]
    d = m.predict_video_group(mixed, batch_size=4, augment=True)
    assert m.last_video_stats["frames_h2d_bytes"] == sum(v.numel() for v in tiny_videos) - tiny_videos[2].numel()
    for other in (b, c, d):
        for (s0, n0), (s1, n1) in zip(a, other):
            assert np.array_equal(s0, s1) and np.array_equal(n0, n1)
    # a group of one video with batch size 4 runs predict_video's batches: the same bits
    one = m.predict_video_group(tiny_videos[:1], batch_size=4, augment=True)
    s, n = m.predict_video(tiny_videos[0], batch_size=4, augment=True)
    assert np.array_equal(one[0][0], s) and np.array_equal(one[0][1], n)
    # explicit clip starts per video, in another order
    mine = [[20, -5, 31, 3, 12, 36], [0, 16, 8], [1], [-7, 0]]
    got = m.predict_video_group(tiny_videos, clip_starts=mine, batch_size=4)
    assert m.last_video_stats["clips"] == 12 and m.last_video_stats["batches"] == 3
    T = 8
    flat = [(v, s_) for v, ss in enumerate(mine) for s_ in ss]
    st = E.ScoreStitcher([(f"v{v}", L, 25.0) for v, L in enumerate(LENGTHS)], 4)
    for lo in range(0, 12, 4):
        _, sc = m.predict(torch.stack([_window(tiny_videos[v], s_, T) for v, s_ in flat[lo:lo + 4]]))
        for j, (v, s_) in enumerate(flat[lo:lo + 4]):
            st.add(f"v{v}", s_, sc[j])
    for v in range(4):
        assert np.array_equal(got[v][0], st.tracks[f"v{v}"][0]) and np.array_equal(got[v][1], st.tracks[f"v{v}"][1])


def _host_chain(st, classes, suppress, hr=0.01):
    """ScoreStitcher -> normalised -> frame_events -> both suppressions: (norm, arg-max records, [suppressed records])"""
    norm = st.normalised()
    pe, recall, _ = E.frame_events(norm, classes, st.fps, high_recall_score_threshold=hr)
    lists = [(E.soft_non_maximum_suppression if kind == "snms" else E.non_maximum_suppression)(recall, w, thr)
             for kind, w, thr in suppress]
    return norm, pe, lists


@pytest.mark.parametrize("windows", [(1, 3), ([2, 1, 3], [3, 1, 2])], ids=["scalar", "list"])
@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_spot_video_group_equals_the_host_chain(tiny_model, tiny_videos, augment, windows):
    m = tiny_model
    suppress = (("nms", windows[0], 0.01), ("snms", windows[1], 0.01))
    st, _ = _reference(m, tiny_videos, augment, True)
    norm, pe, lists = _host_chain(st, CLASSES, suppress)
    out = m.spot_video_group(tiny_videos, CLASSES, suppress=suppress, batch_size=4, augment=augment)
    stats = dict(m.last_video_stats)
    assert len(out) == 4
    kept = 0
    for v, r in enumerate(out):
        name = f"v{v}"                                                # sorted order = video order here
        assert r["pred"].dtype == np.int32 and np.array_equal(r["pred"], norm[name].argmax(axis=1)), v
        assert r["events"] == pe[v]["events"], v
        assert len(r["suppressed"]) == 2
        for got, want in zip(r["suppressed"], lists):
            assert want[v]["video"] == name and got == want[v]["events"] and len(got) == want[v]["num_events"], v
            kept += len(got)
    assert kept > 0
    assert stats["frames"] == 70 and stats["clips"] == 36 and stats["batches"] == 9 and stats["videos"] == 4
    assert stats["host_syncs"] == 2
    assert stats["events_d2h_bytes"] == 70 * 5 + 2 * (4 + 4 * 4) * 4 + 13 * kept       # per entry: 4 list ends, 4 x 4 rounds
    assert len(stats["nms_rounds"]) == 2 and all(1 <= x <= 37 for x in stats["nms_rounds"])


def test_group_routes_synchronise_once_and_twice(tiny_model, tiny_videos, monkeypatch):
    m = tiny_model
    m.predict_video_group(tiny_videos, batch_size=4, augment=True)                    # warm-up: graphs of B = 4, both views
    m.spot_video_group(tiny_videos, CLASSES, batch_size=4, augment=True)
    calls = []
    real_sync, real_item, real_cpu, real_dev_sync = (torch.cuda.Stream.synchronize, torch.Tensor.item, torch.Tensor.cpu,
                                                     torch.cuda.synchronize)
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (calls.append("stream"), real_sync(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("device"), real_dev_sync(*a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append("cpu") if self.is_cuda else None,
                                                                   real_cpu(self, *a, **k))[1])
    m.predict_video_group(tiny_videos, batch_size=4, augment=True)
    assert calls == ["stream"] and m.last_video_stats["host_syncs"] == 1
    del calls[:]
    out = m.spot_video_group(tiny_videos, CLASSES, batch_size=4, augment=True)
    assert calls == ["stream", "stream"] and m.last_video_stats["host_syncs"] == 2
    assert sum(len(x) for r in out for x in r["suppressed"]) > 0


def test_group_route_stays_within_the_fp32_bound_of_the_per_video_route(tiny_model, tiny_videos):
    """The two routes cut different batches and the engine does not promise batch-invariant bits.  The project holds fp32
    logits within 1e-3 of the reference, so two routes that each meet that are within 2e-3 of each other, and softmax does
    not widen it: per-frame mean scores within 2e-3, support equal."""
    m = tiny_model
    out = m.predict_video_group(tiny_videos, batch_size=4, use_amp=False)
    worst = 0.0
    for v, video in enumerate(tiny_videos):
        sums, sup = m.predict_video(video, batch_size=4, use_amp=False)
        assert np.array_equal(sup, out[v][1]), v
        d = np.maximum(sup, 1)[:, None].astype(np.float32)
        worst = max(worst, float(np.abs(sums / d - out[v][0] / d).max()))
    print(f"group route against per-video route, fp32, tiny: max |mean difference| {worst:.3e}")
    assert worst <= 2e-3, worst


def test_spot_videos_in_groups(tiny_model, tiny_videos):
    m = tiny_model
    fifth = t(synth.uint8_clip(4900, (14, 3, 64, 64)))
    vids = [("d", 37, 25.0, tiny_videos[0]), ("b", 23, 30.0, lambda: tiny_videos[1]), ("e", 9, 25.0, tiny_videos[2]),
            ("a", 1, 25.0, tiny_videos[3]), ("c", 14, 12.5, fifth)]
    suppress = (("nms", 1, 0.01), ("snms", [3, 1, 2], 0.01))
    got_pe, got_lists, preds = E.spot_videos(m, vids, CLASSES, suppress, augment=True, batch_size=4, group_videos=3)
    one_pe, one_lists, one_preds = E.spot_videos(m, vids, CLASSES, suppress, augment=True, batch_size=4, group_videos=1)
    # the same structure and order as video by video
    assert [x["video"] for x in got_pe] == [x["video"] for x in one_pe] == ["a", "b", "c", "d", "e"]
    assert [x["fps"] for x in got_pe] == [x["fps"] for x in one_pe]
    assert len(got_lists) == len(one_lists) == 2
    for a, b in zip(got_lists, one_lists):
        assert [(x["video"], x["fps"], sorted(x)) for x in a] == [(x["video"], x["fps"], sorted(x)) for x in b]
    assert sorted(preds) == sorted(one_preds) and all(preds[k].shape == one_preds[k].shape for k in preds)
    # exactly the host chain on the grouped tracks
    st = E.stitch_videos(m, vids, 4, augment=True, batch_size=4, group_videos=3)
    norm, pe, lists = _host_chain(st, CLASSES, suppress)
    assert got_pe == pe and got_lists[0] == lists[0] and got_lists[1] == lists[1]
    assert all(np.array_equal(preds[v], norm[v].argmax(axis=1)) for v in preds)
    assert sum(x["num_events"] for x in got_lists[0]) > 0
    truth = [{"video": v, "events": [{"label": "c1", "frame": 0}, {"label": "c2", "frame": 5}, {"label": "c3", "frame": 8}]}
             for v in "abcde"]
    for lst, ref in zip(got_lists, lists):
        assert E.mean_average_precisions(truth, lst, [1, 2])[0] == E.mean_average_precisions(truth, ref, [1, 2])[0]


# ----------------------------------------------------------------------------- 9. end to end, full size
CFG2 = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4, num_classes=4,
            radi_displacement=2)


def test_group_full_size_once():
    m = _model(CFG2, seed=5)
    lengths = [101, 101, 130, 66, 220, 101]
    packed = ops.fill_u8_hash((sum(lengths), 3, 224, 224), 77, DEV).cpu()
    off = np.concatenate([[0], np.cumsum(lengths)])
    videos = [packed[off[v]:off[v + 1]] for v in range(6)]
    classes = {f"c{k}": k for k in range(1, 5)}
    w0, w1 = E.WINDOWS["default"]
    suppress = (("nms", w0, 0.01), ("snms", w1, 0.01))
    out = m.predict_video_group(videos, batch_size=8, augment=True)
    stats = dict(m.last_video_stats)
    assert [len(E.video_clip_starts(L, 100, 75)) for L in lengths] == [2, 2, 3, 1, 6, 2]
    assert stats["clips"] == 16 and stats["batches"] == 2 and stats["views"] == 2 and stats["videos"] == 6
    assert stats["frames_h2d_bytes"] == sum(lengths) * 150528
    st, batches = _yardstick(m, videos, 8, True, True)
    assert batches == 2
    for v in range(6):
        assert np.array_equal(out[v][1], st.tracks[f"v{v}"][1]), v
        assert np.array_equal(out[v][0], st.tracks[f"v{v}"][0]), (v, float(np.abs(out[v][0] - st.tracks[f"v{v}"][0]).max()))
    norm, pe, lists = _host_chain(st, classes, suppress)
    spot = m.spot_video_group(videos, classes, suppress=suppress, batch_size=8, augment=True)
    kept = 0
    for v, r in enumerate(spot):
        assert np.array_equal(r["pred"], norm[f"v{v}"].argmax(axis=1)) and r["events"] == pe[v]["events"], v
        for got, want in zip(r["suppressed"], lists):
            assert got == want[v]["events"], v
            kept += len(got)
    assert kept > 0 and m.last_video_stats["host_syncs"] == 2 and m.last_video_stats["batches"] == 2


# ----------------------------------------------------------------------------- 10. refusals
def test_group_refusals_launch_nothing(tiny_model, tiny_videos, monkeypatch):
    m = tiny_model
    launched = []
    for gather in ("clip_gather", "clip_gather_seg", "rows_gather", "rows_gather_seg"):       # every gather the model may call
        monkeypatch.setattr(ops, gather, lambda *a, **k: launched.append(1))
    small = t(synth.uint8_clip(7, (5, 3, 32, 32)))
    with pytest.raises(ValueError, match="geometry"):
        m.predict_video_group([tiny_videos[1], small])
    total = sum(v.numel() for v in tiny_videos)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        m.predict_video_group(tiny_videos, max_resident_bytes=total - 1)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        m.spot_video_group(tiny_videos, CLASSES, max_resident_bytes=total - 1)
    with pytest.raises(ValueError, match="no videos"):
        m.predict_video_group([])
    with pytest.raises(ValueError, match="empty"):
        m.predict_video_group([tiny_videos[0], tiny_videos[0][:0]])
    with pytest.raises(ValueError, match="classes"):
        m.spot_video_group(tiny_videos, {"c1": 1, "c2": 2})
    with pytest.raises(ValueError, match="classes"):
        m.spot_video_group(tiny_videos, {"c1": 1, "c2": 2, "c3": 4})
    with pytest.raises(ValueError, match="kind"):
        m.spot_video_group(tiny_videos, CLASSES, suppress=(("soft", 1, 0.01),))
    with pytest.raises(TypeError):
        m.predict_video_group([tiny_videos[0].float()])
    assert not launched
