"""Host side of scoring videos longer than the device budget through a frame ring: `evalutil.ring_plan` against a brute
force over every batch's frames, the property that makes the upload's wait rule deadlock-free, the numpy twin of the ring
gather, `video_groups(stream_frames=True)` and the argument checks of the new C entry (no GPU needed)."""
import numpy as np
import pytest
import torch

from tdeed_amd import evalutil as E
from test_video_host import FakeModel

FB = 12                                                    # bytes per frame: any number does for the arithmetic


def _brute(lengths, T, ov, pad, per, bs, clip_starts=None):
    """The tables of the group and, in plain Python, per batch the set of real packed frames its clips read."""
    seg_off, clip_off, starts, base, len_v = E.group_clip_table(lengths, T, ov, pad, clip_starts)
    frames = []
    for lo in range(0, len(starts), bs):
        mine = set()
        for i in range(lo, min(lo + bs, len(starts))):
            for t in range(T):
                f = int(starts[i]) + t
                if 0 <= f < int(len_v[i]):
                    mine.add(int(base[i]) + f)
        frames.append(mine)
    first = [min(m) // per if m else -1 for m in frames]
    last = [max(m) // per if m else -1 for m in frames]
    n_chunks = -(-sum(lengths) // per)
    readers = [[b for b, m in enumerate(frames) if any(p // per == c for p in m)] for c in range(n_chunks)]
    need = max(z - a + 1 for a, z in zip(first, last) if a >= 0) + 1
    return (starts, base, len_v), frames, first, last, readers, need


def _check_plan(lengths, T, ov, pad, per, bs, clip_starts=None):
    tabs, frames, first, last, readers, need = _brute(lengths, T, ov, pad, per, bs, clip_starts)
    budget = need * per * FB                               # the smallest budget that passes, by the brute force
    assert budget < sum(lengths) * FB
    plan = E.ring_plan(lengths, FB, per, budget, *tabs, T, bs)
    assert plan.ring_chunks == need and plan.ring_frames == need * per
    assert plan.first.tolist() == first and plan.last.tolist() == last
    assert plan.last_reader.tolist() == [max(r) if r else -1 for r in readers]
    # a few bytes more change nothing, a whole chunk more is a longer ring
    assert E.ring_plan(lengths, FB, per, budget + per * FB - 1, *tabs, T, bs).ring_chunks == need
    assert E.ring_plan(lengths, FB, per, budget + per * FB, *tabs, T, bs).ring_chunks == need + 1
    for small in (budget - 1, budget - per * FB, per * FB - 1):
        with pytest.raises(ValueError, match="max_resident_bytes") as e:
            E.ring_plan(lengths, FB, per, small, *tabs, T, bs)
        assert str(budget) in str(e.value)
    # the wait rule: the chunk that chunk c overwrites was last read by a batch BEFORE the first one that reads c (the batch
    # for which the host queues c, at the latest), so the release event the copy waits for exists and nothing waits in a circle
    for rc in (need, need + 1, need + 3):
        p = E.ring_plan(lengths, FB, per, rc * per * FB, *tabs, T, bs)
        if p is None:
            continue
        checked = 0
        for c in range(p.ring_chunks, len(readers)):
            if readers[c]:
                assert p.last_reader[c - p.ring_chunks] < min(readers[c]), (rc, c)
                # and one chunk further: the upload runs one chunk ahead of the batch
                if c + 1 < len(readers):
                    assert p.last_reader[c + 1 - p.ring_chunks] < min(readers[c]), (rc, c)
                checked += 1
        assert checked or rc > need
        # all frames of one batch sit in distinct ring rows
        for m in frames:
            assert len({q % p.ring_frames for q in m}) == len(m)
    return need, plan, frames


# ----------------------------------------------------------------------------- 1. the plan
def test_ring_plan_is_none_exactly_when_the_frames_fit():
    seg_off, clip_off, starts, base, len_v = E.group_clip_table([37], 8, 6)
    total = 37 * FB
    for per in (3, 5, 37, 100):
        assert E.ring_plan([37], FB, per, total, starts, base, len_v, 8, 4) is None
        assert E.ring_plan([37], FB, per, total + 1, starts, base, len_v, 8, 4) is None
    assert E.ring_plan([37], FB, 3, total - 1, starts, base, len_v, 8, 4) is not None
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.ring_plan([37], FB, 37, total - 1, starts, base, len_v, 8, 4)        # one chunk is the whole video: no ring
    with pytest.raises(ValueError):
        E.ring_plan([37], 0, 3, total, starts, base, len_v, 8, 4)


@pytest.mark.parametrize("bs", [4, 5])
def test_ring_plan_equals_the_brute_force_on_the_tiny_video(bs):
    need, plan, frames = _check_plan([37], 8, 6, 5, 3, bs)
    assert all(frames) and len(frames) == -(-18 // bs)
    assert plan.ring_frames < 37


@pytest.mark.parametrize("bs", [4, 5])
def test_ring_plan_group_with_a_video_shorter_than_the_clip(bs):
    lengths = [19, 5, 30]
    need, plan, frames = _check_plan(lengths, 8, 6, 5, 3, bs)
    # chunk 6 (frames 18..20) spans the boundary at 19: the batch of video 0's last clip AND that of video 1's clips read it
    (starts, base, len_v), _, _, _, readers, _ = _brute(lengths, 8, 6, 5, 3, bs)
    clip_off = E.group_clip_table(lengths, 8, 6)[1]
    assert (clip_off[1] - 1) // bs in readers[6] and (clip_off[2] - 1) // bs in readers[6]
    assert plan.last_reader[6] == (clip_off[2] - 1) // bs
    # clip by clip (batches of one): a window hanging over the end of the 5-frame video never counts the next video's
    # frames, one hanging over its front never the previous one's -- its chunks are 6 (19, 20) and 7 (21..23) only
    one = E.ring_plan(lengths, FB, 3, 10 * 3 * FB, starts, base, len_v, 8, 1)
    short = [i for i in range(len(starts)) if int(len_v[i]) == 5]
    assert len(short) == 3 and all(int(starts[i]) < 0 for i in short) and int(starts[short[-1]]) + 8 > 5
    assert all(one.first[i] == 6 and one.last[i] in (6, 7) for i in short) and one.last[short[-1]] == 7
    assert one.first[short[-1] + 1] == 8                                       # video 2 starts in chunk 8 (frame 24)


def test_ring_plan_refuses_clips_that_go_backwards():
    lengths = [37]
    mine = [[20, 22, 24, 26, -5, -3, -1, 1]]
    seg_off, clip_off, starts, base, len_v = E.group_clip_table(lengths, 8, 6, clip_starts=mine)
    with pytest.raises(ValueError, match="ascending order"):
        E.ring_plan(lengths, FB, 3, 30 * FB, starts, base, len_v, 8, 4)
    # the same clips in ascending order pass, and so does disorder INSIDE a batch
    up = [sorted(mine[0])]
    assert E.ring_plan(lengths, FB, 3, 30 * FB, *E.group_clip_table(lengths, 8, 6, clip_starts=up)[2:], 8, 4) is not None
    inside = [[-1, -5, 1, -3, 26, 20, 24, 22]]
    assert E.ring_plan(lengths, FB, 3, 30 * FB, *E.group_clip_table(lengths, 8, 6, clip_starts=inside)[2:], 8, 4) is not None


def test_ring_plan_batches_of_nothing_but_padding_read_nothing():
    mine = [[-8, -9, 0, 2, 40, 50, 29, 28]]
    tabs = E.group_clip_table([37], 8, 6, clip_starts=mine)[2:]
    plan = E.ring_plan([37], FB, 3, 30 * FB, *tabs, 8, 2)
    assert plan.first.tolist() == [-1, 0, -1, 9] and plan.last.tolist() == [-1, 3, -1, 12]
    assert plan.last_reader.tolist() == [1, 1, 1, 1, -1, -1, -1, -1, -1, 3, 3, 3, 3]


# ----------------------------------------------------------------------------- 2. the numpy twin of the ring gather
def test_clip_gather_ring_ref_equals_the_segmented_reference_when_the_ring_holds_everything():
    rs = np.random.RandomState(3)
    lengths = [9, 3, 11]
    L, T = sum(lengths), 4
    video = rs.randint(1, 256, (L, 3, 2, 2)).astype(np.uint8)
    mine = [[-4, -2, 0, 6, 8], [-3, 0, 2], [-1, 5, 9, 10, 11]]
    _, _, starts, base, len_v = E.group_clip_table(lengths, T, 3, clip_starts=mine)
    maps = np.concatenate([video, np.zeros((1,) + video.shape[1:], np.uint8)])
    ref = E.rows_gather_ref(maps, starts, L, L, T, base, len_v)           # the plain segmented gather: zero row as padding
    for rf in (L, L + 1, 2 * L + 3):
        out, ring = E.clip_gather_ring_ref(video, 0, rf, starts, T, base, len_v)
        assert out.dtype == np.uint8 and np.array_equal(out, ref), rf
        assert ring.shape[0] == rf and np.array_equal(ring[:L], video) and np.all(ring[L:] == 0xA5)
    assert int(ref[0].sum()) == 0 and int(ref[-1].sum()) == 0              # clips of nothing but padding


def test_clip_gather_ring_ref_wraps_and_refuses_dead_frames():
    video = (np.arange(23, dtype=np.uint8) + 1).reshape(23, 1)
    starts, base, len_v = [9, 10, 12], [0, 0, 0], [23, 23, 23]
    out, ring = E.clip_gather_ring_ref(video, 9, 6, starts[:2], 4, base[:2], len_v[:2])
    assert ring[:, 0].tolist() == [13, 14, 15, 10, 11, 12]                   # frame p (value p + 1) in row p % 6
    assert out[:, :, 0].tolist() == [[10, 11, 12, 13], [11, 12, 13, 14]]     # rows 3, 4, 5, 0: the window straddles the wrap
    with pytest.raises(ValueError, match="live"):
        E.clip_gather_ring_ref(video, 9, 6, starts, 4, base, len_v)          # frame 15 is not in [9, 15)
    with pytest.raises(ValueError, match="live"):
        E.clip_gather_ring_ref(video, 9, 6, [7], 4, [0], [23])


# ----------------------------------------------------------------------------- 3. grouping
def test_video_groups_isolate_a_video_over_the_budget_when_streaming():
    g64 = (3, 64, 64)
    fb = 3 * 64 * 64
    lengths = [5, 5, 13, 5, 7, 5, 20]
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.video_groups(lengths, [g64] * 7, 8, 12 * fb)
    with pytest.raises(ValueError, match="stream_frames"):
        E.video_groups(lengths, [g64] * 7, 8, 12 * fb, stream_frames=False)
    got = E.video_groups(lengths, [g64] * 7, 8, 12 * fb, stream_frames=True)
    assert got == [[0, 1], [2], [3, 4], [5], [6]]
    # the others: as stream_frames=False cuts the runs between the long videos
    head = E.video_groups(lengths[:2], [g64] * 2, 8, 12 * fb)
    mid = [[j + 3 for j in g] for g in E.video_groups(lengths[3:6], [g64] * 3, 8, 12 * fb)]
    assert got == head + [[2]] + mid + [[6]]
    # nothing over the budget: the keyword changes nothing
    for gv in (1, 2, 8):
        assert E.video_groups(lengths[:2] + lengths[3:6], [g64] * 5, gv, 12 * fb, stream_frames=True) == \
            E.video_groups(lengths[:2] + lengths[3:6], [g64] * 5, gv, 12 * fb)


class RecordingModel(FakeModel):
    def __init__(self):
        super().__init__()
        self.group_kw = []

    def predict_video_group(self, frames_list, max_resident_bytes=None, stream_frames=False, **kw):
        self.group_kw.append(([int(f.shape[0]) for f in frames_list], stream_frames))
        return super().predict_video_group(frames_list, **kw)


def test_stitch_videos_passes_stream_frames_on():
    def frames_of(i, L):
        fr = torch.zeros((L, 3, 1, 1), dtype=torch.uint8)
        fr[0, 0, 0, 0] = i
        return fr
    src = [(f"v{i}", L, 25.0, frames_of(i + 1, L)) for i, L in enumerate([5, 21, 9])]
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.stitch_videos(RecordingModel(), src, FakeModel.K1, group_videos=3, max_resident_bytes=15 * 3, overlap_len=6)
    m = RecordingModel()
    st = E.stitch_videos(m, src, FakeModel.K1, group_videos=3, max_resident_bytes=15 * 3, overlap_len=6, stream_frames=True)
    assert m.group_kw == [([5], True), ([21], True), ([9], True)]
    m2 = RecordingModel()
    ref = E.stitch_videos(m2, src, FakeModel.K1, group_videos=3, overlap_len=6)
    assert m2.group_kw == [([5, 21, 9], False)]
    for name in ref.tracks:
        assert np.array_equal(st.tracks[name][0], ref.tracks[name][0]) and np.array_equal(st.tracks[name][1], ref.tracks[name][1])


# ----------------------------------------------------------------------------- 4. the C entry checks its arguments
def test_ring_entry_point_validates_before_launching():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd._lib import call, HipCallError
    P = 1 << 20
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_clip_gather_ring_u8", P, 6, 23, 48, P, None, P, 1, 1, P, None)       # no clip_base table
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_clip_gather_ring_u8", None, 6, 23, 48, P, P, P, 1, 1, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_clip_gather_ring_u8", P, 0, 23, 48, P, P, P, 1, 1, P, None)          # ring_frames = 0
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_clip_gather_ring_u8", P, 6, 0, 48, P, P, P, 1, 1, P, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_clip_gather_ring_u8", P, 6, 23, 48, P, P, P, 700, 100, P, None)
