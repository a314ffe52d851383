"""Host side of scoring a group of videos as one packed job: the group's tables, the grouping rule, the order of the
segmented stitch, `stitch_videos` / `spot_videos` with group_videos > 1 on a fake model, and the argument checks of the new C
entry points (no GPU needed)."""
import threading

import numpy as np
import pytest
import torch

from tdeed_amd import evalutil as E
from test_video_host import FakeModel, stitch_inputs


# ----------------------------------------------------------------------------- 1. the tables of a group
def test_group_clip_table_literals():
    seg_off, clip_off, starts, base, len_v = E.group_clip_table([101, 66, 130], 100, 75)
    for a in (seg_off, clip_off, starts, base, len_v):
        assert a.dtype == np.int32
    assert starts.tolist() == [-5, 20, -5, -5, 20, 45]
    assert clip_off.tolist() == [0, 2, 3, 6]
    assert seg_off.tolist() == [0, 101, 167, 297]
    assert base.tolist() == [0, 0, 101, 167, 167, 167]
    assert len_v.tolist() == [101, 101, 66, 130, 130, 130]
    # per video it is video_clip_starts
    for v, L in enumerate([101, 66, 130]):
        assert starts[clip_off[v]:clip_off[v + 1]].tolist() == E.video_clip_starts(L, 100, 75)
    # pad_len travels
    assert E.group_clip_table([37], 8, 6, pad_len=3)[2].tolist() == E.video_clip_starts(37, 8, 6, pad_len=3)


def test_group_clip_table_keeps_the_order_of_explicit_starts():
    mine = [[20, -5, 31, 3], [4], [7, 7, -8, 30, 0]]
    seg_off, clip_off, starts, base, len_v = E.group_clip_table([37, 5, 30], 8, 6, clip_starts=mine)
    assert starts.tolist() == [20, -5, 31, 3, 4, 7, 7, -8, 30, 0]
    assert clip_off.tolist() == [0, 4, 5, 10] and seg_off.tolist() == [0, 37, 42, 72]
    assert base.tolist() == [0] * 4 + [37] + [42] * 5 and len_v.tolist() == [37] * 4 + [5] + [30] * 5


def test_group_clip_table_refuses_empty_videos():
    with pytest.raises(ValueError, match="empty"):
        E.group_clip_table([10, 0, 4], 8, 6)
    with pytest.raises(ValueError, match="no clips"):
        E.group_clip_table([10, 4], 8, 6, clip_starts=[[0], []])
    with pytest.raises(ValueError):
        E.group_clip_table([10, 4], 8, 6, clip_starts=[[0]])


# ----------------------------------------------------------------------------- 2. grouping
def test_video_groups_close_on_count_budget_and_geometry():
    g64, g32 = (3, 64, 64), (3, 32, 32)
    fb = 3 * 64 * 64
    assert E.video_groups([5] * 7, [g64] * 7, 3, 1 << 40) == [[0, 1, 2], [3, 4, 5], [6]]                    # count
    assert E.video_groups([5, 5, 5, 9, 2], [g64] * 5, 8, 12 * fb) == [[0, 1], [2], [3, 4]]                   # budget: 10, 5, 11
    assert E.video_groups([5, 7], [g64] * 2, 8, 12 * fb) == [[0, 1]]                                        # exactly the budget
    assert E.video_groups([5, 5, 5, 5], [g64, g64, g32, g64], 8, 1 << 40) == [[0, 1], [2], [3]]              # geometry
    assert E.video_groups([5, 5], [g64] * 2, 1, 1 << 40) == [[0], [1]]
    assert E.video_groups([], [], 4, 1 << 40) == []
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.video_groups([5, 13, 5], [g64] * 3, 8, 12 * fb)
    with pytest.raises(ValueError):
        E.video_groups([5], [g64], 0, 1 << 40)


# ----------------------------------------------------------------------------- 3. the order of the segmented stitch
@pytest.mark.parametrize("views", [1, 2])
def test_stitch_clip_scores_seg_equals_stitch_clip_scores_per_video(views):
    lengths = [37, 5, 1, 21]
    mine = [E.video_clip_starts(37, 8, 6), [-5, -3, -1, 0, 2, 4, -8, 5], [-7, 0, 1, -3], [9, -2, 14, 20, 3]]
    seg_off, clip_off, starts, _, _ = E.group_clip_table(lengths, 8, 6, clip_starts=mine)
    n = len(starts)
    _, plain, flip = stitch_inputs(0, starts=list(range(n)), seed=7)
    flip = flip if views == 2 else None
    sums, sup = E.stitch_clip_scores_seg(plain, starts, seg_off, clip_off, flip_scores=flip)
    assert sums.dtype == np.float32 and sums.shape == (64, 4) and sup.dtype == np.int32 and sup.shape == (64,)
    for v, L in enumerate(lengths):
        lo, hi = clip_off[v], clip_off[v + 1]
        ref = E.stitch_clip_scores(plain[lo:hi], mine[v], L, flip_scores=None if flip is None else flip[lo:hi])
        assert np.array_equal(sums[seg_off[v]:seg_off[v + 1]], ref[0]), v
        assert np.array_equal(sup[seg_off[v]:seg_off[v + 1]], ref[1]), v
    assert float(sums.sum()) > 0 and int(sup.max()) >= 2


# ----------------------------------------------------------------------------- 4. stitch_videos / spot_videos in groups
class FakeGroupModel(FakeModel):
    """FakeModel whose group entry points are the per-video ones applied to every video of the group"""

    def __init__(self):
        super().__init__()
        self.group_calls = []

    def predict_video_group(self, frames_list, **kw):
        self.group_calls.append(([int(np.asarray(f)[0, 0, 0, 0]) for f in frames_list], threading.current_thread().name))
        return super().predict_video_group(frames_list, **kw)

    def _spot(self, frames, classes, suppress, hr, **kw):
        sums, sup = self.predict_video(frames, **kw)
        norm = {"v": sums / np.maximum(sup, 1)[:, None].astype(np.float32)}
        pe, recall, _ = E.frame_events(norm, classes, {"v": 25.0}, high_recall_score_threshold=hr)
        lists = [(E.soft_non_maximum_suppression if kind == "snms" else E.non_maximum_suppression)(recall, w, thr)[0]["events"]
                 for kind, w, thr in suppress]
        return dict(pred=norm["v"].argmax(axis=1).astype(np.int32), events=pe[0]["events"], suppressed=lists)

    def spot_video(self, frames, classes, suppress=(), high_recall_score_threshold=0.01, overlap_len=None, batch_size=8,
                   augment=False, **kw):
        return self._spot(frames, classes, suppress, high_recall_score_threshold, overlap_len=overlap_len,
                          batch_size=batch_size, augment=augment)

    def spot_video_group(self, frames_list, classes, suppress=(), high_recall_score_threshold=0.01, overlap_len=None,
                         batch_size=8, augment=False, max_resident_bytes=None, **kw):
        self.group_calls.append(([int(np.asarray(f)[0, 0, 0, 0]) for f in frames_list], threading.current_thread().name))
        return [self._spot(f, classes, suppress, high_recall_score_threshold, overlap_len=overlap_len, batch_size=batch_size,
                           augment=augment) for f in frames_list]


def _sources(decoded, shapes=None):
    names = [("d_vid", 21, 25.0), ("a_vid", 37, 12.5), ("e_vid", 5, 25.0), ("b_vid", 9, 30.0), ("c_vid", 14, 25.0)]
    ids = {n: i + 1 for i, (n, _, _) in enumerate(names)}

    def frames_of(name, L):
        hw = (shapes or {}).get(name, 1)
        fr = torch.zeros((L, 3, hw, hw), dtype=torch.uint8)
        fr[0, 0, 0, 0] = ids[name]
        return fr

    def lazy(name, L):
        def run():
            decoded.append((name, threading.current_thread().name))
            return frames_of(name, L)
        return run
    return [(n, L, fps, lazy(n, L) if i in (0, 3) else frames_of(n, L)) for i, (n, L, fps) in enumerate(names)], ids


@pytest.mark.parametrize("augment", [False, True])
def test_stitch_videos_in_groups_equals_video_by_video(augment):
    decoded = []
    src, ids = _sources(decoded)
    ref = E.stitch_videos(FakeGroupModel(), src, FakeModel.K1, augment=augment, batch_size=5, overlap_len=6)
    del decoded[:]
    m = FakeGroupModel()
    st = E.stitch_videos(m, src, FakeModel.K1, augment=augment, batch_size=5, overlap_len=6, group_videos=3)
    assert [c[0] for c in m.group_calls] == [[1, 2, 3], [4, 5]]                     # the order given, not the sorted one
    assert all(c[1] == threading.current_thread().name for c in m.group_calls)
    assert [d[0] for d in decoded] == ["d_vid", "b_vid"]
    assert all(d[1] != threading.current_thread().name for d in decoded)            # decoded on the worker thread
    assert st.fps == ref.fps and sorted(st.tracks) == sorted(ref.tracks)
    for name in ref.tracks:
        assert np.array_equal(st.tracks[name][0], ref.tracks[name][0]) and np.array_equal(st.tracks[name][1], ref.tracks[name][1])
    # a geometry change inside a batch of group_videos videos closes the group
    m2 = FakeGroupModel()
    src2, _ = _sources([], shapes={"e_vid": 2})
    E.stitch_videos(m2, src2, FakeModel.K1, augment=augment, batch_size=5, overlap_len=6, group_videos=4)
    assert [c[0] for c in m2.group_calls] == [[1, 2], [3], [4], [5]]
    with pytest.raises(ValueError, match="announced"):
        E.stitch_videos(FakeGroupModel(), [("a_vid", 36, 25.0, torch.zeros((37, 3, 1, 1), dtype=torch.uint8))], FakeModel.K1,
                        group_videos=2)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.stitch_videos(FakeGroupModel(), src, FakeModel.K1, group_videos=3, max_resident_bytes=36 * 3)


def test_spot_videos_in_groups_equals_video_by_video():
    classes = {"x": 1, "y": 2}
    suppress = (("nms", 1, 0.01), ("snms", [3, 1], 0.01))
    src, _ = _sources([])
    ref = E.spot_videos(FakeGroupModel(), src, classes, suppress, batch_size=5, overlap_len=6)
    m = FakeGroupModel()
    got = E.spot_videos(m, src, classes, suppress, batch_size=5, overlap_len=6, group_videos=2)
    assert [c[0] for c in m.group_calls] == [[1, 2], [3, 4], [5]]
    assert [x["video"] for x in got[0]] == ["a_vid", "b_vid", "c_vid", "d_vid", "e_vid"]
    assert got[0] == ref[0] and got[1] == ref[1]
    assert sorted(got[2]) == sorted(ref[2]) and all(np.array_equal(got[2][k], ref[2][k]) for k in ref[2])
    assert sum(len(v["events"]) for lst in got[1] for v in lst) > 0
    assert all(v["num_events"] == len(v["events"]) for lst in got[1] for v in lst)


# ----------------------------------------------------------------------------- 5. the C entries check their arguments
def test_group_entry_points_validate_before_launching():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd._lib import call, load, HipCallError
    P = 1 << 20
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_clip_gather_seg_u8", P, 4, 48, P, None, P, 1, 1, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_clip_gather_seg_u8", P, 0, 48, P, P, P, 1, 1, P, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_clip_gather_seg_u8", P, 4, 48, P, P, P, 700, 100, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_stitch_scores_seg", P, 1, 1, 8, 4, P, None, P, 1, 0, 10, P, P, None, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_stitch_scores_seg", P, 1, 1, 8, 4, P, P, P, 0, 0, 10, P, P, None, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_stitch_scores_seg", P, 1, 1, 8, 4, P, P, P, 65536, 0, 70000, P, P, None, None)
    with pytest.raises(HipCallError, match="count_all"):
        call("tdeed_stitch_scores_seg", P, 1, 1, 8, 4, P, P, P, 1, 2, 10, P, P, None, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_frame_events_seg", P, None, 1, 10, 10, 4, 0.01, P, None, P, P, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_frame_events_seg", P, P, 1, 10, 11, 4, 0.01, P, None, P, P, P, None)          # max_len > L_total
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_frame_events_seg", P, P, 65536, 70000, 10, 4, 0.01, P, None, P, P, P, None)
    with pytest.raises(HipCallError, match="one-byte"):
        call("tdeed_frame_events_seg", P, P, 1, 10, 10, 300, 0.01, P, P, P, P, P, None)
    win = (__import__("ctypes").c_int * 3)(1, 1, 0)

    def nms(**kw):
        a = dict(mean=P, seg_off=P, nv=2, L=10, max_len=6, K1=4, hr=0.01, thr=0.01, soft=0, windows=win, nw=1, first=P, ws=None,
                 em=P, kept=P, sf=P, sc=P, ss=P, scnt=P, of=P, oc=P, os=P, eo=P, rounds=P)
        a.update(kw)
        call("tdeed_nms_track_seg", *a.values(), None)
    with pytest.raises(HipCallError, match="null pointer"):
        nms(eo=None)
    with pytest.raises(HipCallError, match="bad sizes"):
        nms(max_len=11)
    with pytest.raises(HipCallError, match="65535"):
        nms(nv=65536, L=70000)
    with pytest.raises(HipCallError, match="classes"):
        nms(K1=66)
    with pytest.raises(HipCallError, match="soft"):
        nms(soft=2)
    with pytest.raises(HipCallError, match="windows"):
        nms(nw=2)
    with pytest.raises(HipCallError, match="window 0"):
        nms(soft=1, nw=3)
    with pytest.raises(HipCallError, match="workspace"):
        nms(L=40000, max_len=20000)
    lib = load()
    assert lib.tdeed_nms_track_seg_workspace(20037, 20000, 2) == 20037 * 9
    assert lib.tdeed_nms_track_seg_workspace(20037, 16000, 18) == 0 and lib.tdeed_nms_track_seg_workspace(16000, 16000, 18) == 0
    assert lib.tdeed_nms_track_seg_workspace(16001, 16001, 2) == 16001 * 9                # one video over the LDS-resident state
    assert [lib.tdeed_nms_track_seg_threads(x) for x in (1, 101, 128, 129, 256, 257, 512, 513, 1 << 20)] == \
        [128, 128, 128, 256, 256, 512, 512, 1024, 1024]
