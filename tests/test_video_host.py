"""Host side of whole-video scoring: the evaluation dataset's clip list, the stitch order, decoding a video once and
`stitch_videos` (no GPU needed)."""
import json
import math
import os
import threading

import numpy as np
import pytest
import torch

from helpers import ROOT, load_golden
from tdeed_amd import evalutil as E
from tdeed_amd import feeder


# ----------------------------------------------------------------------------- 1. clip starts
def test_video_clip_starts_match_the_reference_dataset():
    """tests/golden/video_clips.npz holds the `_clips` and `.videos` of the reference's ActionSpotVideoDataset
    (tools/make_goldens.py:video_clips) for strides 1, 2 and 12."""
    meta, g = load_golden("video_clips")
    lengths = meta["lengths"]
    assert {c["stride"] for c in meta["cases"]} == {1, 2, 12}
    for ci, c in enumerate(meta["cases"]):
        T, ov, stride, pad = c["clip_len"], c["overlap_len"], c["stride"], c["pad_len"]
        want_v, want_s = g[f"clip_video__{ci}"], g[f"clip_start_sampled__{ci}"]
        got_v, got_s = [], []
        for vi, n in enumerate(lengths):
            s = E.video_clip_starts(n, T, ov, stride, pad)
            assert len(s) >= 1, (c, n)
            # predict_video works on the sampled frames: the same list from their count alone
            assert s == E.video_clip_starts(math.ceil(n / stride), T, ov, 1, pad), (c, n)
            got_v += [vi] * len(s)
            got_s += s
        assert got_v == want_v.tolist() and got_s == want_s.tolist(), c
        # `.videos` is sorted by name = by length here (zero-padded names)
        assert g[f"videos_len__{ci}"].tolist() == [math.ceil(n / stride) for n in sorted(lengths)], c
    # the cases the fixture must contain
    assert any(n < c["clip_len"] for c in meta["cases"] for n in lengths)
    assert any(n <= c["overlap_len"] * c["stride"] for c in meta["cases"] for n in lengths)
    assert any(n % c["stride"] for c in meta["cases"] for n in lengths if c["stride"] > 1)


def _coverage(starts, T, L):
    cov = np.zeros(L, np.int64)
    for s in starts:
        cov[max(s, 0):max(min(s + T, L), 0)] += 1
    return cov


def test_video_clip_starts_literals_and_coverage():
    s = E.video_clip_starts(37, 8, 6, 1)
    assert s == list(range(-5, 30, 2)) and len(s) == 18
    assert _coverage(s, 8, 37).min() >= 1 and _coverage(s, 8, 37).max() <= 4
    s = E.video_clip_starts(37, 8, 6, 2)
    assert s == list(range(-5, 12, 2)) and len(s) == 9 and s == E.video_clip_starts(19, 8, 6, 1)
    assert _coverage(s, 8, 19).min() >= 1 and _coverage(s, 8, 19).max() <= 4
    s = E.video_clip_starts(430, 100, 75, 1)
    assert s == list(range(-5, 346, 25)) and len(s) == 15
    assert _coverage(s, 100, 430).min() >= 1 and _coverage(s, 100, 430).max() <= 4
    assert E.video_clip_starts(3, 8, 6, 1) == [-5, -3, -1]
    s = E.video_clip_starts(67500, 100, 50, 12)
    assert len(s) == 112 and s[0] == -5 and s[-1] == 5545 and s == E.video_clip_starts(5625, 100, 50, 1)
    cov = _coverage(s, 100, 5625)
    assert cov.min() >= 1 and cov.max() <= 2
    s = E.video_clip_starts(100, 100, 75, 1)
    assert s == [-5, 20]
    cov = _coverage(s, 100, 100)
    assert cov.min() >= 1 and cov.max() <= 2


# ----------------------------------------------------------------------------- 2. stitch order
def stitch_inputs(L, T=8, K1=4, starts=None, seed=0):
    """random fp32 clip scores (two views) with ~30 % all-zero rows"""
    rs = np.random.RandomState(seed)
    if starts is None:
        starts = [-5, -3, -1, 0, 2, 4, 4, 9, 17, 25, 30, 33, 36, -8, L]
    n = len(starts)
    out = []
    for _ in range(2):
        p = rs.rand(n, T, K1).astype(np.float32)
        p[rs.rand(n, T) < 0.3] = 0.0
        out.append(p)
    return starts, out[0], out[1]


STITCH_CASES = [dict(L=37, seed=1), dict(L=5, seed=2, starts=[-5, -3, -1, 0, 2, 4, -8, 5]),       # L < T
                dict(L=37, seed=3, starts=E.video_clip_starts(37, 8, 6))]


@pytest.mark.parametrize("case", STITCH_CASES)
def test_stitch_clip_scores_equals_the_score_stitcher(case):
    L = case["L"]
    starts, plain, flip = stitch_inputs(L, starts=case.get("starts"), seed=case["seed"])
    assert min(starts) < 0 and (max(s + 8 for s in starts) > L or case["seed"] == 3)     # the dataset's own list ends at L
    # one view: ScoreStitcher.add per clip
    st = E.ScoreStitcher([("v", L, 25.0)], 4)
    for i, s in enumerate(starts):
        st.add("v", s, plain[i])
    sums, sup = E.stitch_clip_scores(plain, starts, L)
    assert sums.dtype == np.float32 and sup.dtype == np.int32
    assert np.array_equal(sums, st.tracks["v"][0]) and np.array_equal(sup, st.tracks["v"][1])
    assert np.array_equal(sums / np.maximum(sup, 1)[:, None].astype(np.float32), st.normalised()["v"])
    assert (sup < _coverage(starts, 8, L)).any()          # the all-zero rows were not counted
    # two views: add_views once per view, plain first (the order of stitch_predictions(augment=True))
    st2 = E.ScoreStitcher([("v", L, 25.0)], 4)
    for i, s in enumerate(starts):
        st2.add_views("v", s, plain[i][None])
        st2.add_views("v", s, flip[i][None])
    sums2, sup2 = E.stitch_clip_scores(plain, starts, L, flip_scores=flip)
    assert np.array_equal(sums2, st2.tracks["v"][0]) and np.array_equal(sup2, st2.tracks["v"][1])
    assert np.array_equal(sup2, 2 * _coverage(starts, 8, L))
    assert np.array_equal(sums2 / np.maximum(sup2, 1)[:, None].astype(np.float32), st2.normalised()["v"])


# ----------------------------------------------------------------------------- 3. decoding a video once
def _frame_dirs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "frame_reader.npz"))
    meta = json.loads(str(g["meta"]))
    base = os.path.join(ROOT, "tests", "golden", "frames")
    return meta, [(ds, os.path.join(base, ds), v[0], meta["source_info"].get(ds)) for ds, v in meta["layouts"].items()]


def test_load_video_decodes_each_frame_once(monkeypatch):
    meta, dirs = _frame_dirs()
    n = meta["n_frames"]
    assert n == 7 and len(dirs) == 4
    real_read = feeder.read_frame
    pool = feeder.DecodePool(3)
    for ds, fdir, vname, si in dirs:
        _, _, _, path_fn = feeder.frame_locator(fdir, ds, vname, si)
        opened = []
        monkeypatch.setattr(feeder, "read_frame", lambda p, out=None: (opened.append(p), real_read(p, out=out))[1])
        vid = feeder.load_video(fdir, ds, vname, n, source_info=si)
        assert sorted(opened) == sorted(path_fn(j) for j in range(n)), ds          # every file exactly once
        opened.clear()
        buf = torch.full((9, 3, meta["h"], meta["w"]), 7, dtype=torch.uint8)
        vid2 = feeder.load_video(fdir, ds, vname, n, source_info=si, out=buf, pool=pool)
        assert sorted(opened) == sorted(path_fn(j) for j in range(n)), ds
        monkeypatch.setattr(feeder, "read_frame", real_read)
        assert vid.dtype == torch.uint8 and vid.shape == (n, 3, meta["h"], meta["w"]) and torch.equal(vid, vid2)
        for j in range(n):
            assert torch.equal(vid[j], real_read(path_fn(j))), (ds, j)
        # every evaluation clip is a zero-padded window of it
        starts = E.video_clip_starts(n, 4, 3)
        assert starts[0] == -5
        checked = 0
        for s in starts:
            ref = feeder.load_clip_video(fdir, ds, vname, s, s + 4, pad=True, source_info=si)
            if isinstance(ref, int):
                assert ref == -1 and s + 4 <= 0          # a window of padding only
                continue
            win = torch.zeros((4,) + tuple(vid.shape[1:]), dtype=torch.uint8)
            for t_ in range(4):
                if 0 <= s + t_ < n:
                    win[t_] = vid[s + t_]
            assert torch.equal(win, ref), (ds, s)
            checked += 1
        assert checked == sum(1 for s in starts if s + 4 > 0) >= n
        # stride 2: sampled frames 0, 2, 4, 6
        v2 = feeder.load_video(fdir, ds, vname, n, stride=2, source_info=si)
        assert v2.shape[0] == 4 and all(torch.equal(v2[j], vid[2 * j]) for j in range(4))
        # the label announces more frames than there are files: trailing zero frames
        v9 = feeder.load_video(fdir, ds, vname, n + 2, source_info=si)
        assert v9.shape[0] == n + 2 and torch.equal(v9[:n], vid) and int(v9[n:].sum()) == 0
    pool.close()


def test_load_video_raises_on_a_hole(tmp_path):
    from PIL import Image
    d = tmp_path / "vid"
    d.mkdir()
    rs = np.random.RandomState(0)
    for i in (0, 1, 3, 4):
        Image.fromarray(rs.randint(0, 256, (8, 8, 3), dtype=np.uint8)).save(str(d / f"frame{i}.jpg"))
    with pytest.raises(FileNotFoundError, match="frame2.jpg"):
        feeder.load_video(str(tmp_path), "soccernetball", "vid", 5)
    assert feeder.load_video(str(tmp_path), "soccernetball", "vid", 2).shape[0] == 2
    with pytest.raises(FileNotFoundError):
        feeder.load_video(str(tmp_path), "soccernetball", "nothing_here", 2)


# ----------------------------------------------------------------------------- 4. stitch_videos
class FakeModel:
    """Scores that depend on (video id, clip index) only; the clip / video identity travels in the frames' first bytes."""
    T, K1 = 8, 3

    def __init__(self):
        self.video_calls = []

    def clip_scores(self, vid, i, flip):
        rs = np.random.RandomState(1000 * vid + 2 * i + int(flip))
        p = rs.rand(self.T, self.K1).astype(np.float32)
        p[rs.rand(self.T) < 0.25] = 0.0
        return p

    def predict(self, frames, augment_inference=False):
        frames = np.asarray(frames)
        sc = np.stack([self.clip_scores(int(c[0, 0, 0, 0]), int(c[0, 1, 0, 0]), augment_inference) for c in frames])
        return sc.argmax(-1), sc

    def predict_video(self, frames, overlap_len=None, batch_size=8, augment=False, **kw):
        frames = np.asarray(frames)
        vid, L = int(frames[0, 0, 0, 0]), frames.shape[0]
        self.video_calls.append((vid, threading.current_thread().name, batch_size))
        starts = E.video_clip_starts(L, self.T, self.T // 4 * 3 if overlap_len is None else overlap_len)
        plain = np.stack([self.clip_scores(vid, i, False) for i in range(len(starts))])
        flip = np.stack([self.clip_scores(vid, i, True) for i in range(len(starts))]) if augment else None
        return E.stitch_clip_scores(plain, starts, L, flip_scores=flip)

    def predict_video_group(self, frames_list, max_resident_bytes=None, **kw):
        """what stitch_videos calls, also for single videos: the per-video route applied to every video of the group"""
        return [self.predict_video(f, **kw) for f in frames_list]


@pytest.mark.parametrize("augment", [False, True])
def test_stitch_videos_fills_the_tracks_like_stitch_predictions(augment):
    T = FakeModel.T
    videos = [("b_vid", 21, 25.0), ("a_vid", 37, 12.5), ("c_vid", 5, 25.0)]
    ids = {"b_vid": 1, "a_vid": 2, "c_vid": 3}
    # route A: the clip loader of the reference's evaluation (batch size 1 when augmenting)
    clips = []
    for name, L, _ in videos:
        for i, s in enumerate(E.video_clip_starts(L, T, 6)):
            fr = np.zeros((T, 3, 1, 1), np.uint8)
            fr[0, 0, 0, 0], fr[0, 1, 0, 0] = ids[name], i
            clips.append((name, s, fr))
    bs = 1 if augment else 4
    loader = [dict(frame=np.stack([c[2] for c in clips[lo:lo + bs]]), video=[c[0] for c in clips[lo:lo + bs]],
                   start=np.array([c[1] for c in clips[lo:lo + bs]])) for lo in range(0, len(clips), bs)]
    st_a = E.stitch_predictions(FakeModel(), loader, videos, FakeModel.K1, augment=augment)
    # route B: one predict_video per video; two videos arrive through callables
    decoded = []

    def frames_of(name, L):
        fr = torch.zeros((L, 3, 1, 1), dtype=torch.uint8)
        fr[0, 0, 0, 0] = ids[name]
        return fr

    def lazy(name, L):
        def run():
            decoded.append((name, threading.current_thread().name))
            return frames_of(name, L)
        return run
    m = FakeModel()
    src = [(videos[0][0], 21, 25.0, lazy("b_vid", 21)), (videos[1][0], 37, 12.5, frames_of("a_vid", 37)),
           (videos[2][0], 5, 25.0, lazy("c_vid", 5))]
    st_b = E.stitch_videos(m, src, FakeModel.K1, augment=augment, batch_size=5, overlap_len=6)
    assert [c[0] for c in m.video_calls] == [1, 2, 3] and all(c[2] == 5 for c in m.video_calls)
    assert [d[0] for d in decoded] == ["b_vid", "c_vid"]
    assert all(d[1] != threading.current_thread().name for d in decoded)            # decoded on the worker thread
    assert st_b.fps == st_a.fps
    for name, _, _ in videos:
        assert np.array_equal(st_a.tracks[name][0], st_b.tracks[name][0]), name
        assert np.array_equal(st_a.tracks[name][1], st_b.tracks[name][1]), name
    classes = {"x": 1, "y": 2}
    na, nb = st_a.normalised(), st_b.normalised()
    ea, eb = E.frame_events(na, classes, st_a.fps), E.frame_events(nb, classes, st_b.fps)
    assert ea[0] == eb[0] and ea[1] == eb[1] and sum(len(v["events"]) for v in ea[0]) > 0
    assert E.non_maximum_suppression(ea[0], 2) == E.non_maximum_suppression(eb[0], 2)
    with pytest.raises(ValueError, match="announced"):
        E.stitch_videos(FakeModel(), [("a_vid", 36, 25.0, frames_of("a_vid", 37))], FakeModel.K1)


# ----------------------------------------------------------------------------- the C entries check their arguments
def test_video_entry_points_validate_before_launching():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd._lib import call, HipCallError
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_clip_gather_u8", None, 4, 48, None, 1, 1, None, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_clip_gather_u8", 1 << 20, 4, 48, 1 << 20, 700, 100, 1 << 20, None)
    P = 1 << 20
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_stitch_scores_seg", None, 1, 1, 8, 4, None, P, P, 1, 0, 10, None, None, None, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_stitch_scores_seg", P, 1, 1, 8, 4, P, P, P, 1, 0, 10, P, None, None, None)       # no support
    with pytest.raises(HipCallError, match="count_all"):
        call("tdeed_stitch_scores_seg", P, 1, 1, 8, 4, P, P, P, 1, 2, 10, P, P, None, None)
