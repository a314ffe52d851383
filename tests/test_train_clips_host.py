"""Host side of the resident training loader (tdeed_amd.trainclips) against the reference's ActionSpotDataset, recorded in
tests/golden/train_clips.npz (tools/make_goldens.py train_clips): the clip list, the label rule and the draw order.  No GPU."""
import random

import numpy as np
import pytest

from helpers import load_golden
from tdeed_amd import trainclips as TC


@pytest.fixture(scope="module")
def gold():
    return load_golden("train_clips")


def table_of(meta, case, **kw):
    return TC.train_clip_table(meta["videos"], meta["classes"], case["clip_len"], case["stride"], case["overlap"],
                               case["pad_len"], **kw)


def test_fixture_holds_the_cases_the_kernels_must_survive(gold):
    meta, _ = gold
    got = {(c["clip_len"], c["stride"], c["overlap"], c["radi_displacement"]) for c in meta["cases"]}
    assert {(8, 1, 1, 0), (8, 1, 1, 2), (8, 2, 1, 2), (8, 3, 0.5, 1), (100, 1, 1, 4), (100, 12, 1, 2)} <= got
    assert [v["num_frames"] for v in meta["videos"]] == [3, 6, 7, 37, 101, 430]


def test_clip_table_equals_the_reference_clip_list(gold):
    meta, arr = gold
    for ci, case in enumerate(meta["cases"]):
        tab = table_of(meta, case)
        assert tab.clip_video.dtype == np.int32 and tab.clip_base.dtype == np.int64
        assert np.array_equal(tab.clip_video, arr[f"clip_video__{ci}"]), case
        assert np.array_equal(tab.clip_base, arr[f"clip_base__{ci}"]), case
        assert len(tab.clip_video) == case["n_clips"]
    # stride 12: some windows of the 3-frame video sample no existing frame and are dropped
    ci = [i for i, c in enumerate(meta["cases"]) if c["stride"] == 12][0]
    case = meta["cases"][ci]
    step = TC.clip_step(case["clip_len"], case["overlap"])
    assert meta["videos"][0]["num_frames"] == 3
    bases = range(-case["pad_len"] * 12, max(0, 3 - 1 + (2 * case["pad_len"] - case["clip_len"]) * 12), step)
    hits = [b for b in bases if any(0 <= b + 12 * j < 3 for j in range(case["clip_len"]))]
    kept = arr[f"clip_base__{ci}"][arr[f"clip_video__{ci}"] == 0].tolist()
    assert kept == hits and 0 < len(kept) < len(bases)


def test_event_arrays_keep_file_order(gold):
    meta, _ = gold
    tab = table_of(meta, meta["cases"][0])
    assert tab.ev_off.dtype == tab.ev_frame.dtype == tab.ev_class.dtype == np.int32
    assert tab.ev_off.tolist() == np.concatenate([[0], np.cumsum([len(v["events"]) for v in meta["videos"]])]).tolist()
    flat = [e for v in meta["videos"] for e in v["events"]]
    assert tab.ev_frame.tolist() == [e["frame"] for e in flat]
    assert tab.ev_class.tolist() == [meta["classes"][e["label"]] for e in flat]
    assert any(a["frame"] > b["frame"] for v in meta["videos"] for a, b in zip(v["events"], v["events"][1:]))   # unsorted lists


def test_labels_and_draw_order_reproduce_the_reference_items(gold):
    meta, arr = gold
    seen_displ = set()
    for ci, case in enumerate(meta["cases"]):
        tab = table_of(meta, case)
        draws = TC.ClipDraws(len(tab.clip_video), meta["n_items"], 5, case["mixup"], case["seed"])
        ia, ib = zip(*list(draws))
        ia = np.concatenate(ia)
        assert len(ia) == meta["n_items"]
        T, S, r = case["clip_len"], case["stride"], case["radi_displacement"]
        lab, labD = TC.rasterise_labels(tab, ia, T, S, r)
        assert lab.dtype == labD.dtype == np.int64 and lab.shape == (meta["n_items"], T)
        assert np.array_equal(lab, arr[f"label__{ci}"]), case
        if r > 0:
            assert np.array_equal(labD, arr[f"labelD__{ci}"]), case
            seen_displ |= set(np.unique(labD).tolist())
        if case["mixup"]:
            lab2, labD2 = TC.rasterise_labels(tab, np.concatenate(ib), T, S, r)
            assert np.array_equal(lab2, arr[f"label2__{ci}"]), case
            if r > 0:
                assert np.array_equal(labD2, arr[f"labelD2__{ci}"]), case
        else:
            assert all(b is None for b in ib)
        assert sorted(k.split("__")[0] for k in arr if k.endswith(f"__{ci}") and k.startswith("label")) == sorted(case["keys"])
    assert min(seen_displ) < 0 < max(seen_displ)
    assert sum(int(arr[f"label__{ci}"].any()) for ci in range(len(meta["cases"]))) >= 4      # the recorded items carry events


def test_label_rule_details(gold):
    meta, _ = gold
    case = [c for c in meta["cases"] if (c["clip_len"], c["stride"], c["radi_displacement"]) == (8, 2, 2)][0]
    tab = table_of(meta, case)
    v37 = [v["num_frames"] for v in meta["videos"]].index(37)
    # events 17 (class 3) and 19 (class 1) of the 37-frame video, base 18, stride 2: idx = floor(-1/2) = -1 and 0
    c = int(np.where((tab.clip_video == v37) & (tab.clip_base == 18))[0][0])
    lab, labD = TC.rasterise_labels(tab, [c], 8, 2, 2)
    assert lab[0, :3].tolist() == [1, 1, 1] and labD[0, :3].tolist() == [0, 1, 2]           # the later event overwrites
    only17 = TC.train_clip_table([dict(video="x", num_frames=37, events=[dict(frame=17, label="land")])], meta["classes"], 8, 2)
    c = int(np.where(only17.clip_base == 18)[0][0])
    lab, labD = TC.rasterise_labels(only17, [c], 8, 2, 2)
    assert lab[0].tolist() == [3, 3, 0, 0, 0, 0, 0, 0] and labD[0, :2].tolist() == [1, 2]   # idx -1, not C's truncated 0


def test_clip_draws_leave_the_global_generator_alone():
    random.seed(123)
    before = random.getstate()
    d = TC.ClipDraws(50, 23, 4, True, 9)
    batches = list(d) + list(d)
    assert random.getstate() == before
    assert len(batches) == 12 and all(a.dtype == np.int64 and b.dtype == np.int64 for a, b in batches)
    # the stream of random.seed(9): one draw per item and one for its partner, continued over the second pass
    rng = random.Random(9)
    want = [(rng.randint(0, 49), rng.randint(0, 49)) for _ in range(46)]
    got = [(int(x), int(y)) for a, b in batches for x, y in zip(a, b)]
    assert got == want


def test_last_batch_is_short_or_dropped():
    sizes = [len(a) for a, _ in TC.ClipDraws(50, 23, 4, False, 1)]
    assert sizes == [4, 4, 4, 4, 4, 3] and len(TC.ClipDraws(50, 23, 4, False, 1)) == 6
    d = TC.ClipDraws(50, 23, 4, False, 1, drop_last=True)
    assert [len(a) for a, _ in d] == [4] * 5 and len(d) == 5
    assert [len(a) for a, _ in TC.ClipDraws(50, 8, 4, False, 1)] == [4, 4]
    # a dropped batch is not drawn: the next pass continues where a DataLoader's sampler would
    rng = random.Random(1)
    want = [rng.randint(0, 49) for _ in range(60)]
    assert [int(x) for _ in range(2) for a, _ in d for x in a] == want[20:]


def test_require_events_keeps_the_clips_with_a_label(gold):
    meta, _ = gold
    dropped = 0
    for case in meta["cases"]:
        T, S, r = case["clip_len"], case["stride"], case["radi_displacement"]
        full = table_of(meta, case)
        lab, _ = TC.rasterise_labels(full, np.arange(len(full.clip_video)), T, S, r)
        keep = lab.any(axis=1)
        some = table_of(meta, case, require_events=True, radi_displacement=r)
        assert keep.sum() > 0
        dropped += int((~keep).sum())
        assert np.array_equal(some.clip_video, full.clip_video[keep]) and np.array_equal(some.clip_base, full.clip_base[keep])
    assert dropped > 100                       # (every window of 100 frames holds an event, most windows of 8 do not)


def test_negative_radius_and_bad_overlap_raise(gold):
    meta, _ = gold
    tab = table_of(meta, meta["cases"][0])
    with pytest.raises(ValueError):
        TC.rasterise_labels(tab, [0], 8, 1, -1)
    with pytest.raises(ValueError):
        table_of(meta, meta["cases"][0], radi_displacement=-1)
    with pytest.raises(ValueError):
        TC.clip_step(8, 1.5)
    with pytest.raises(ValueError):
        TC.train_clip_table(meta["videos"], meta["classes"], 8, 1, 0.95)       # int(0.05 * 8) = 0: no step


def test_load_resident_videos_decodes_each_frame_once_and_insists_on_existing_frames(tmp_path):
    import torch
    from PIL import Image
    from tdeed_amd import feeder, synth
    lengths = {"va": 5, "vb": 3}
    for name, n in lengths.items():
        (tmp_path / name).mkdir()
        for i in range(n):
            Image.fromarray(synth.uint8_clip(900 + i, (8, 12, 3))).save(str(tmp_path / name / f"frame{i}.jpg"), quality=92)
    videos = [dict(video=k, num_frames=n, events=[]) for k, n in lengths.items()]
    pool = feeder.DecodePool(2)
    try:
        frames = TC.load_resident_videos(str(tmp_path), "fs_comp", videos, pool=pool)
    finally:
        pool.close()
    assert [tuple(f.shape) for f in frames] == [(5, 3, 8, 12), (3, 3, 8, 12)] and all(f.dtype == torch.uint8 for f in frames)
    for v, f in zip(videos, frames):
        for i in range(v["num_frames"]):
            assert torch.equal(f[i], feeder.read_frame(str(tmp_path / v["video"] / f"frame{i}.jpg"))), (v["video"], i)
    # the reader's windows agree with plain indexing into the resident tensor (stride 2, padded at both ends)
    paths = feeder.load_paths(str(tmp_path), "fs_comp", "va", -2, 8, stride=2)
    clip = feeder.load_frames(paths, pad=True, stride=2)
    want = torch.zeros((5, 3, 8, 12), dtype=torch.uint8)
    for j in range(5):
        if 0 <= -2 + 2 * j < 5:
            want[j] = frames[0][-2 + 2 * j]
    assert torch.equal(clip, want)
    # a label that counts more frames than exist would keep clips the reference drops: refused
    with pytest.raises(ValueError, match="number of frames that exist"):
        TC.load_resident_videos(str(tmp_path), "fs_comp", [dict(video="vb", num_frames=4, events=[])])
