"""Joint datasets without a GPU: `trainclips.JointDraws`, the joined clip table and the per-clip-stride label rule against
tests/golden/train_clips_joint.npz (the reference's own ActionSpotDatasetJoint), `join_resident_jpegs`, and `stream_plan` /
`stage_batch` with a stride per clip against a brute-force range computation and a byte-level simulation."""
import random

import numpy as np
import pytest

import joint_cases as JC
import test_stream_clips_host as SC
from tdeed_amd import trainclips as TC

META, G = JC.golden()
CASES = list(range(len(META["cases"])))


def _recorded(ci, key):
    return G[f"{key}__{ci}"]


# ----------------------------------------------------------------------------- 1. the draws
@pytest.mark.parametrize("ci", CASES)
def test_joint_draws_reproduce_the_references_parts_and_indices(ci):
    case = META["cases"][ci]
    mixup = case["mixup"]
    state = random.getstate()
    draws = TC.JointDraws(case["n_clips"], case["dataset_len"], 5, mixup, case["seed"])
    assert len(draws) == 5 and draws.dataset_len == META["n_items"] == 24
    got = list(draws)
    assert [len(p) for p, _, _ in got] == [5, 5, 5, 5, 4]                    # the short last batch
    assert np.array_equal(np.concatenate([p for p, _, _ in got]), _recorded(ci, "part"))
    assert np.array_equal(np.concatenate([a for _, a, _ in got]), _recorded(ci, "idx"))
    if mixup:
        assert np.array_equal(np.concatenate([b for _, _, b in got]), _recorded(ci, "idx2"))
    else:
        assert all(b is None for _, _, b in got)
    assert all(p.dtype == a.dtype == np.int64 for p, a, _ in got) and set(np.concatenate([p for p, _, _ in got])) == {1, 2}
    assert random.getstate() == state                                       # a private generator
    # over a pass boundary: two passes of 10 items are the first 20 of the one stream; the sum as an int does the same
    short = TC.JointDraws(case["n_clips"], 10, 4, mixup, case["seed"])
    two = list(short) + list(short)
    assert [len(p) for p, _, _ in two] == [4, 4, 2, 4, 4, 2]
    assert np.array_equal(np.concatenate([p for p, _, _ in two]), _recorded(ci, "part")[:20])
    assert np.array_equal(np.concatenate([a for _, a, _ in two]), _recorded(ci, "idx")[:20])
    if mixup:
        assert np.array_equal(np.concatenate([b for _, _, b in two]), _recorded(ci, "idx2")[:20])
    short.reseed(case["seed"])
    p, a, _ = next(iter(short))
    assert np.array_equal(p, _recorded(ci, "part")[:4]) and np.array_equal(a, _recorded(ci, "idx")[:4])
    # drop_last: the short batch is neither yielded nor drawn
    dl = TC.JointDraws(case["n_clips"], 10, 4, mixup, case["seed"], drop_last=True)
    two = list(dl) + list(dl)
    assert len(dl) == 2 and np.array_equal(np.concatenate([a for _, a, _ in two]), _recorded(ci, "idx")[:16])


def test_joint_draws_refuse_bad_arguments():
    for bad in (dict(n_clips=(3,)), dict(n_clips=(3, 0)), dict(dataset_len=0), dict(batch_size=0), dict(n_clips=(3, 4, 5))):
        with pytest.raises(ValueError):
            TC.JointDraws(**dict(dict(n_clips=(3, 4), dataset_len=4, batch_size=2, mixup=False, seed=0), **bad))


# ----------------------------------------------------------------------------- 2. the joined table
def _bare_loader(parts, lengths, clip_len, radius, mixup, joint, batch_size=4, seed=0):
    ld = TC._ClipLoader()
    ld._init_parts(parts, lengths, clip_len, radius, mixup, batch_size, seed, TC.DEFAULT_PAD_LEN, False, "cpu", 3, joint)
    return ld


@pytest.mark.parametrize("ci", CASES)
def test_joined_clip_table_is_the_parts_tables_with_shifted_indices(ci):
    case = META["cases"][ci]
    parts = JC.parts_of(case, frames=False)
    T, r = case["clip_len"], case["radi_displacement"]
    tables, tab = JC.joined_table(parts, T, r)
    nv = [len(p["videos"]) for p in parts]
    for k, t in enumerate(tables):                                          # each part is the reference's own list
        assert np.array_equal(t.clip_video, G[f"clip_video__{ci}__p{k}"]) and np.array_equal(t.clip_base, G[f"clip_base__{ci}__p{k}"])
        assert len(t.clip_video) == case["n_clips"][k]
    n1, e1 = len(tables[0].clip_video), len(tables[0].ev_frame)
    assert tab.part_clips.tolist() == [0, n1, n1 + len(tables[1].clip_video)] and tab.part_videos.tolist() == [0, nv[0], sum(nv)]
    assert np.array_equal(tab.clip_video[:n1], tables[0].clip_video) and np.array_equal(tab.clip_video[n1:], tables[1].clip_video + nv[0])
    assert np.array_equal(tab.clip_base, np.concatenate([t.clip_base for t in tables]))
    assert np.array_equal(tab.clip_part, np.repeat([1, 2], [n1, len(tab.clip_video) - n1]))
    assert np.array_equal(tab.ev_off[:nv[0] + 1], tables[0].ev_off) and np.array_equal(tab.ev_off[nv[0]:], tables[1].ev_off + e1)
    assert np.array_equal(tab.ev_frame, np.concatenate([t.ev_frame for t in tables]))
    assert np.array_equal(tab.ev_class, np.concatenate([t.ev_class for t in tables]))      # each part's OWN class numbers
    assert tab.ev_class[:e1].max() == 3 and tab.ev_class[e1:].max() == 5
    assert tab.clip_video.dtype == np.int32 and tab.ev_off.dtype == np.int32 and tab.clip_base.dtype == np.int64
    # the loader's rows: first packed frame and video shifted by the part in front, a stride and a part per clip
    lengths = [v["num_frames"] for p in parts for v in p["videos"]]
    ld = _bare_loader(parts, lengths, T, r, case["mixup"], joint=True)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    cv = tab.clip_video.astype(np.int64)
    assert np.array_equal(ld._rows, np.stack([offs[cv], tab.clip_base, np.asarray(lengths)[cv], cv]))
    assert ld._rows[0, n1:].min() >= sum(lengths[:nv[0]]) and ld._rows[3, n1:].min() == nv[0]
    assert ld._clip_stride.dtype == np.int32 and ld._clip_stride.tolist() == [case["strides"][0]] * n1 + [case["strides"][1]] * (len(cv) - n1)
    assert ld._nrows == (8 if case["mixup"] else 4) + 2 and ld.strides == tuple(case["strides"]) and ld.stride is None
    assert isinstance(ld.draws, TC.JointDraws) and len(ld) == 6
    ld.reseed(case["seed"])
    part, ia, ib = next(iter(ld.draws))
    ga, gb, gp = ld._drawn((part, ia, ib))
    assert np.array_equal(gp, _recorded(ci, "part")[:4]) and np.array_equal(ga, tab.part_clips[part - 1] + _recorded(ci, "idx")[:4])
    assert (gb is None) == (not case["mixup"])


# ----------------------------------------------------------------------------- 3. labels and frames of the recorded items
@pytest.mark.parametrize("ci", CASES)
def test_labels_with_each_clips_own_stride_equal_the_recorded_rows(ci):
    case = META["cases"][ci]
    parts = JC.parts_of(case)
    T, r = case["clip_len"], case["radi_displacement"]
    _, tab = JC.joined_table(parts, T, r)
    part = _recorded(ci, "part")
    S = np.asarray(case["strides"])[part - 1]
    assert len(set(S.tolist())) == len(set(case["strides"]))
    for sfx, idx in (("", "idx"), ("2", "idx2")) if case["mixup"] else (("", "idx"),):
        ids = tab.part_clips[part - 1] + _recorded(ci, idx)
        label, labelD = TC.rasterise_labels(tab, ids, T, S, r)
        assert np.array_equal(label, _recorded(ci, "label" + sfx)), (ci, sfx)
        if r > 0:
            assert np.array_equal(labelD, _recorded(ci, "labelD" + sfx)), (ci, sfx)
        if case["frame_keys"]:                                   # the padding rule, pinned to the reference's own reader
            frames = [f for p in parts for f in p["frames"]]
            want = _recorded(ci, "frame" + sfx)
            got = JC.gather(frames, tab, ids, S, T).numpy()
            assert np.array_equal(got, want)
            assert (want.reshape(len(ids), T, -1).max(axis=2) == 0).any()       # some slot is padding
    assert "labelD" in case["keys"] or r == 0
    assert _recorded(ci, "label").any() and (part == 2).any() and _recorded(ci, "label")[part == 2].max() <= 5


def test_a_stride_that_is_not_positive_is_refused_on_the_host():
    case = META["cases"][0]
    parts = JC.parts_of(case, frames=False)
    _, tab = JC.joined_table(parts, 8)
    with pytest.raises(ValueError, match="positive"):
        TC.rasterise_labels(tab, [0, 1], 8, [1, 0], 2)
    with pytest.raises(ValueError, match="strides"):
        TC.rasterise_labels(tab, [0, 1], 8, [1, 2, 3], 2)
    rows = np.asarray([[0, 0], [0, 2], [5, 5]], np.int64)
    z = np.zeros(5, np.int64)
    with pytest.raises(ValueError, match="positive"):
        TC.batch_tables(rows, 4, [1, -2], z.astype(np.int32), z.astype(np.int32) - 1, z, z)
    with pytest.raises(ValueError, match="positive"):
        TC._two_parts([dict(parts[0], frames=[], stride=0), dict(parts[1], frames=[])], "frames", "JointResidentClips")
    with pytest.raises(ValueError, match="two"):
        TC._two_parts([dict(parts[0], frames=[])], "frames", "JointResidentClips")
    with pytest.raises(ValueError, match="lacks"):
        TC._two_parts([dict(parts[0]), dict(parts[1])], "frames", "JointResidentClips")


# ----------------------------------------------------------------------------- 4. a single-part loader
@pytest.mark.parametrize("mixup", [False, True])
def test_a_single_part_loader_builds_the_tables_it_always_built(mixup):
    p = META["parts"][0]
    lengths = [v["num_frames"] for v in p["videos"]]
    ld = TC._ClipLoader()
    part = dict(videos=p["videos"], classes=p["classes"], stride=2, overlap=0.5, require_events=False, dataset_len=11)
    ld._init_parts([part], lengths, 8, 2, mixup, 4, 9, TC.DEFAULT_PAD_LEN, False, "cpu", 3, joint=False)
    tab = TC.train_clip_table(p["videos"], p["classes"], 8, 2, 0.5, TC.DEFAULT_PAD_LEN, False, 2)
    for key in ("clip_video", "clip_base", "ev_frame", "ev_class", "ev_off", "num_frames"):
        assert np.array_equal(getattr(ld.table, key), getattr(tab, key)) and getattr(ld.table, key).dtype == getattr(tab, key).dtype
    assert not hasattr(ld.table, "clip_part") and not ld.joint and ld.stride == 2 and ld._nrows == (8 if mixup else 4)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    cv = tab.clip_video.astype(np.int64)
    assert np.array_equal(ld._rows, np.stack([offs[cv], tab.clip_base, np.asarray(lengths)[cv], cv])) and ld._rows.dtype == np.int64
    want = list(TC.ClipDraws(len(cv), 11, 4, mixup, 9))
    assert type(ld.draws) is TC.ClipDraws
    for (a, b), (wa, wb) in zip(ld.draws, want):
        ga, gb, part = ld._drawn((a, b))
        assert part is None and np.array_equal(ga, wa) and (gb is None if wb is None else np.array_equal(gb, wb))
    ld.reseed(9)
    assert type(ld.draws) is TC.ClipDraws and np.array_equal(next(iter(ld.draws))[0], want[0][0])


# ----------------------------------------------------------------------------- 5. joining packed sets
def _load(tree):
    return [TC.load_resident_jpegs(d, "soccernetball", videos, pinned=False, shard_bytes=512) for d, videos in tree]


def test_join_resident_jpegs_renumbers_sets_and_frames_and_reuses_the_streams(tmp_path):
    a, b = _load(JC.write_trees(str(tmp_path)))
    assert a.n_sets >= 1 and b.n_sets >= 1 and a.samp == b.samp and (a.width, a.height) == (32, 24)
    assert not any(np.array_equal(x, y) for x in a.table_sets for y in b.table_sets)          # other tables, as written
    b_seg = [s.packed.segments.copy() for s in b.shards]
    j = TC.join_resident_jpegs(a, b)
    na = a.n_frames
    assert j.n_frames == na + b.n_frames == 29 and j.names == a.names + b.names and j.n_sets == a.n_sets + b.n_sets
    assert np.array_equal(j.table_sets[:a.n_sets], a.table_sets) and np.array_equal(j.table_sets[a.n_sets:], b.table_sets)
    assert j.video_first.tolist() == [0, 9, 14, 18] and j.video_len.tolist() == [9, 5, 4, 11] and j.fallback == []
    assert np.array_equal(j.frame_set[:na], a.frame_set) and np.array_equal(j.frame_set[na:], b.frame_set + a.n_sets)
    assert (j.width, j.height, j.samp, j.stride) == (a.width, a.height, a.samp, 1)
    assert len(j.shards) == len(a.shards) + len(b.shards) and len(b.shards) >= 2
    for s, o in zip(j.shards[:len(a.shards)], a.shards):
        assert s is o and s.packed.table_sets is j.table_sets
    for s, o, seg in zip(j.shards[len(a.shards):], b.shards, b_seg):
        assert s.packed.stream_np is o.packed.stream_np and s.packed.table_sets is j.table_sets          # reused, not copied
        assert np.array_equal(s.frames, o.frames + na)
        assert np.array_equal(s.packed.segments[:, :5], seg[:, :5]) and np.array_equal(s.packed.segments[:, 5], seg[:, 5] + a.n_sets)
        assert np.array_equal(o.packed.segments, seg)                                          # b itself is left alone
    ext = TC.frame_extents(j.shards)                                          # consecutive runs, in set order
    assert ext.shard_first[-1] == 29 and np.all(ext.hi > ext.lo)
    # a set b shares with a keeps a's number
    twice = TC.join_resident_jpegs(a, a)
    assert twice.n_sets == a.n_sets and np.array_equal(twice.frame_set[na:], a.frame_set)


def test_join_resident_jpegs_geometry_and_sampling(tmp_path):
    a, b = _load(JC.write_trees(str(tmp_path / "same")))
    _, b444 = _load(JC.write_trees(str(tmp_path / "s444"), subsampling2=0))
    _, wide = _load(JC.write_trees(str(tmp_path / "wide"), w=40))
    with pytest.raises(ValueError, match="24x40"):
        TC.join_resident_jpegs(a, wide)
    assert b444.samp != a.samp
    j = TC.join_resident_jpegs(a, b444)                                       # another sampling: all of b through the side buffer
    na = a.n_frames
    assert j.fallback == list(range(na, na + b444.n_frames)) and np.all(j.frame_set[na:] == -1) and j.n_sets == a.n_sets
    assert (j.width, j.height, j.samp) == (a.width, a.height, a.samp)
    assert all(s.packed.n_segments == 0 and len(s.frames) for s in j.shards[len(a.shards):])
    assert sum(len(s.frames) for s in j.shards) == j.n_frames
    ext = TC.frame_extents(j.shards)
    assert np.all(ext.hi[na:] <= ext.lo[na:]) and np.all(ext.hi[:na] > ext.lo[:na])
    b2 =TC.ResidentJpegs(b.shards, b.table_sets, b.frame_set, b.fallback, b.video_first, b.video_len, b.names, b.width, b.height,
                          b.samp, stride=2)
    with pytest.raises(ValueError, match="strides"):
        TC.join_resident_jpegs(a, b2)


# ----------------------------------------------------------------------------- 6. streamed sets with a stride per clip
def _mixed_rows(T, strides):
    """SC's hand-made set as two parts: videos 0 and 1 at strides[0], video 2 at strides[1] -> (rows, stride per clip)"""
    _, videos, _ = SC._set()
    parts = [dict(videos=videos[:2], classes={}, stride=strides[0], dataset_len=3),
             dict(videos=videos[2:], classes={}, stride=strides[1], dataset_len=3)]
    ld = _bare_loader(parts, SC.LENGTHS, T, 0, False, joint=True)
    return ld._rows, ld._clip_stride.astype(np.int64)


def _needs_brute(ext, rows, T, S, per_batch, depth):
    firsts = np.concatenate([[0], np.cumsum(SC.LENGTHS)])
    res, region = [], []
    for v in range(len(SC.LENGTHS) + 1):
        F = int(firsts[v])
        res.append(sum(SC._r16(max([int(ext.hi[g]) for g in range(F) if ext.shard[g] == s], default=0)) for s in range(2)))
        clip = 0
        for (first, base, nfr, vid), s in zip(rows.T.tolist(), S.tolist()):
            if vid >= v:
                clip = max(clip, sum(SC._r16(hi) - lo for _, lo, hi in SC._clip_ranges_brute(ext, first, base, nfr, T, s)))
        region.append(per_batch * clip)
    return [r + SC.FIXED + depth * region[0] for r in res], region


@pytest.mark.parametrize("strides", [(2, 1), (1, 3), (3, 2)])
def test_stream_plan_with_a_stride_per_clip_equals_the_brute_force_ranges(strides):
    ext, _, _ = SC._set()
    T, B, depth, nops = 4, 3, 2, 2
    rows, S = _mixed_rows(T, strides)
    assert set(S[rows[3] < 2].tolist()) == {strides[0]} and set(S[rows[3] == 2].tolist()) == {strides[1]}
    want, region = _needs_brute(ext, rows, T, S, nops * B, depth)
    plan = TC.stream_plan(ext, [0, 5, 9], SC.LENGTHS, rows, T, S, nops, B, depth, SC.FIXED, 1 << 40)
    assert plan.needs.tolist() == want and plan.min_budget == want[0]
    for v in range(4):
        p = TC.stream_plan(ext, [0, 5, 9], SC.LENGTHS, rows, T, S, nops, B, depth, SC.FIXED, want[v])
        assert p.resident_videos == v and p.region_bytes == region[v]
    with pytest.raises(ValueError, match=f"smallest max_resident_bytes that would do is {want[0]}$"):
        TC.stream_plan(ext, [0, 5, 9], SC.LENGTHS, rows, T, S, nops, B, depth, SC.FIXED, want[0] - 1)
    # every clip's ranges, one by one
    clip, shard, lo16, hi = TC._clip_ranges(ext, rows, T, S)
    for c, ((first, base, nfr, _), s) in enumerate(zip(rows.T.tolist(), S.tolist())):
        got = [(int(a), int(b), int(d)) for a, b, d in zip(shard[clip == c], lo16[clip == c], hi[clip == c])]
        assert got == SC._clip_ranges_brute(ext, first, base, nfr, T, s), (c, s)
    if strides[0] != strides[1]:                                # one stride for all would plan something else
        flat = TC._clip_ranges(ext, rows, T, strides[0])
        assert len(flat[3]) != len(hi) or not np.array_equal(flat[3], hi)


@pytest.mark.parametrize("resident", [0, 1, 2])
def test_staged_joint_batches_put_every_frames_bytes_where_its_slot_looks(resident):
    """SC's byte-level simulation of the device buffer with mixup batches whose clips differ in stride; a clip and its
    partner share the stride, as a joint batch's do."""
    strides = (2, 3)
    ext, _, shard_size = SC._set()
    T, B, depth, nops = 4, 3, 2, 2
    rows, S = _mixed_rows(T, strides)
    want, _ = _needs_brute(ext, rows, T, S, nops * B, depth)
    plan = TC.stream_plan(ext, [0, 5, 9], SC.LENGTHS, rows, T, S, nops, B, depth, SC.FIXED, want[resident])
    assert plan.resident_videos == resident
    rs = np.random.RandomState(11)
    host = [rs.randint(1, 255, n).astype(np.uint8) for n in shard_size]
    dev = np.zeros(plan.buffer_bytes, np.uint8)
    for k in range(2):
        n = min(int(plan.shard_bytes[k]), shard_size[k])
        dev[plan.shard_base[k]:plan.shard_base[k] + n] = host[k][:n]
    by_stride = {s: np.flatnonzero(S == s) for s in strides}
    seen, mixed = 0, 0
    at = np.concatenate([np.arange(B), B + np.arange(B)]) * T
    for i in range(12):
        sa = np.asarray(strides)[rs.randint(0, 2, B)]
        ids = np.concatenate([[rs.choice(by_stride[s]) for s in sa], [rs.choice(by_stride[s]) for s in sa]])
        mixed += len(set(sa.tolist())) == 2
        region = plan.stage_lo + (i % depth) * plan.region_bytes
        copies, reloc = TC.stage_batch(plan, ext, rows[:, ids], T, S[ids], region, n_slots=nops * B * T, clip_slot=at)
        dev[region:region + plan.region_bytes] = 0
        brute = []
        for c in ids[rows[3, ids] >= plan.resident_videos]:
            first, base, nfr, _ = rows[:, c].tolist()
            brute += SC._clip_ranges_brute(ext, first, base, nfr, T, int(S[c]))
        assert [c[:3] for c in copies] == brute                                 # per clip and shard, in batch order
        for k, b_lo, b_hi, d in copies:
            assert b_lo % 16 == 0 and d % 16 == 0 and region <= d and d + b_hi - b_lo <= region + plan.region_bytes
            dev[d:d + b_hi - b_lo] = host[k][b_lo:b_hi]
        for c, (first, base, nfr, vid) in enumerate(rows[:, ids].T.tolist()):
            for t in range(T):
                f = base + t * int(S[ids[c]])
                delta, w_lo, w_hi = reloc[at[c] + t].tolist()
                empty = not 0 <= f < nfr or ext.hi[first + f] <= ext.lo[first + f]
                if empty or vid < plan.resident_videos:
                    assert (delta, w_lo, w_hi) == (0, 0, plan.stream_bytes)
                    if empty:
                        continue
                g = first + f
                s = int(ext.shard[g])
                pos = int(plan.shard_base[s]) + int(ext.lo[g])
                n = int(ext.hi[g] - ext.lo[g])
                assert 0 <= w_lo <= pos - delta and pos - delta + n <= w_hi <= dev.size
                assert np.array_equal(dev[pos - delta:pos - delta + n], host[s][ext.lo[g]:ext.hi[g]]), (ids, c, t)
                seen += 1
    assert seen > 100 and mixed >= 4


def test_batch_tables_with_a_stride_per_clip():
    """two clips over one 12-frame video at strides 1 and 3: the slots show first + base + t * stride of their own clip"""
    n = 12
    frame_set = np.zeros(n, np.int32)
    side_row = np.full(n, -1, np.int32)
    piece_lo, piece_n = np.arange(n, dtype=np.int64), np.ones(n, np.int64)
    rows = np.asarray([[0, 0], [2, -3], [n, n]], np.int64)
    tb = TC.batch_tables(rows, 4, [1, 3], frame_set, side_row, piece_lo, piece_n)
    shown = {int(slot): int(piece) for piece, slot in tb.items}
    assert shown == {0: 2, 1: 3, 2: 4, 3: 5, 5: 0, 6: 3, 7: 6} and tb.fill[4] == -1 and tb.slot_set[4] == -1
    one = TC.batch_tables(rows, 4, 3, frame_set, side_row, piece_lo, piece_n)
    both = TC.batch_tables(rows, 4, [3, 3], frame_set, side_row, piece_lo, piece_n)
    assert np.array_equal(one.items, both.items) and np.array_equal(one.fill, both.fill) and np.array_equal(one.waves, both.waves)
