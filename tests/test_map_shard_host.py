"""The host side of a validation pass sharded over ranks: who scores what (`evalutil.shard_videos`), the numpy restatement of
the state exchange (`ap_pack_ref` / `ap_unpack_ref`) on hand-made stores of pretend ranks, the ownership check, the frame
counters against the reference's recorded numbers, and the argument errors of `map_videos` that come before any launch.
Pure CPU.  The store builder is shared with tests/test_gpu_map_shard.py."""
import numpy as np
import pytest

from helpers import load_golden
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth
import test_spot_host as H


# ----------------------------------------------------------------------------- shard_videos
def _loads(lengths, table):
    return [sum(lengths[o] for o in own) for own in table]


SHARD_CASES = {
    "world_1": ([37, 23, 30], 1),
    "more_ranks_than_videos": ([37, 23, 30], 5),
    "equal_lengths": ([10] * 7, 3),
    "one_dominant": ([1000, 3, 5, 2, 4, 1, 6], 3),
    "mixed": ([90, 64, 37, 90, 12, 64, 1, 200, 17], 4),
    "no_videos": ([], 2),
}


@pytest.mark.parametrize("case", sorted(SHARD_CASES))
def test_shard_videos_is_a_deterministic_partition(case):
    lengths, world = SHARD_CASES[case]
    table = E.shard_videos(lengths, world)
    assert len(table) == world
    assert sorted(o for own in table for o in own) == list(range(len(lengths)))        # every ordinal exactly once
    assert all(own == sorted(own) for own in table)
    assert table == E.shard_videos(list(lengths), world) == E.shard_videos(np.asarray(lengths, np.int64), world)
    if world == 1:
        assert table == [list(range(len(lengths)))]
    if lengths and len(lengths) >= world:
        loads = _loads(lengths, table)
        assert max(loads) - min(loads) <= max(lengths), (loads, lengths)
        assert all(table)
    if len(lengths) < world:
        assert sum(1 for own in table if not own) == world - len(lengths)


def test_shard_videos_rule_longest_first_to_the_least_loaded_rank():
    # ties: equal lengths go out in ordinal order, equal loads to the lower rank
    assert E.shard_videos([10, 10, 10, 10], 2) == [[0, 2], [1, 3]]
    assert E.shard_videos([5, 9, 5], 2) == [[1], [0, 2]]
    assert E.shard_videos([1000, 3, 5, 2], 2) == [[0], [1, 2, 3]]
    assert E.shard_videos([37, 23, 30], 2) == [[0], [1, 2]]
    with pytest.raises(ValueError):
        E.shard_videos([1, 2], 0)


# ----------------------------------------------------------------------------- pack / unpack on hand-made stores
def make_stores(lengths, K1, E_, T, seed, gt_counts=None):
    """a filled one-rank store set: dict(ev_score (E,K1-1,LT) f64, ev_count (E,K1-1,NV), hit_pos (E,T,G), hit_count
    (E,T,NV*K1), vid_off, gt_off); counts include empty segments, the unused parts of the stores hold garbage (NaN / -7)"""
    rng = np.random.RandomState(seed)
    NV, LT = len(lengths), sum(lengths)
    vid_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if gt_counts is None:
        gt_counts = rng.randint(0, 4, size=NV * K1)
    gt_counts = np.asarray(gt_counts).copy()
    gt_counts.reshape(NV, K1)[:, 0] = 0                                   # the background column has no truth
    gt_off = np.concatenate([[0], np.cumsum(gt_counts)]).astype(np.int64)
    G = max(int(gt_off[-1]), 1)
    ev_score = np.full((E_, K1 - 1, LT), np.nan)
    ev_count = np.zeros((E_, K1 - 1, NV), np.int32)
    hit_pos = np.full((E_, T, G), -7, np.int32)
    hit_count = np.zeros((E_, T, NV * K1), np.int32)
    for e in range(E_):
        for c in range(K1 - 1):
            for o in range(NV):
                n = int(rng.randint(0, lengths[o] + 1)) if rng.rand() < 0.7 else 0
                ev_count[e, c, o] = n
                ev_score[e, c, vid_off[o]:vid_off[o] + n] = np.sort(rng.randint(0, 7, size=n) / 6.0)[::-1]
        for ti in range(T):
            for oc in range(NV * K1):
                n = int(rng.randint(0, gt_counts[oc] + 1))
                hit_count[e, ti, oc] = n
                hit_pos[e, ti, gt_off[oc]:gt_off[oc] + n] = np.sort(rng.randint(0, 1000, size=n))
    return dict(ev_score=ev_score, ev_count=ev_count, hit_pos=hit_pos, hit_count=hit_count, vid_off=vid_off, gt_off=gt_off)


def rank_share(full, own, K1):
    """what a rank that matched only `own` holds: its segments and counts, zeros in the foreign counts, garbage elsewhere"""
    NV = full["ev_count"].shape[2]
    s = dict(full, ev_score=np.full_like(full["ev_score"], np.nan), ev_count=np.zeros_like(full["ev_count"]),
             hit_pos=np.full_like(full["hit_pos"], -7), hit_count=np.zeros_like(full["hit_count"]))
    for o in own:
        a, b = int(full["vid_off"][o]), int(full["vid_off"][o + 1])
        s["ev_score"][:, :, a:b] = full["ev_score"][:, :, a:b]
        s["ev_count"][:, :, o] = full["ev_count"][:, :, o]
        a, b = int(full["gt_off"][o * K1]), int(full["gt_off"][(o + 1) * K1])
        s["hit_pos"][:, :, a:b] = full["hit_pos"][:, :, a:b]
        s["hit_count"][:, :, o * K1:(o + 1) * K1] = full["hit_count"][:, :, o * K1:(o + 1) * K1]
    assert NV == len(full["vid_off"]) - 1
    return s


def used_parts(s, K1):
    """the parts of the stores the rank launch reads: per score segment its first ev_count entries, per hit segment its first
    hit_count entries"""
    E_, C, NV = s["ev_count"].shape
    T = s["hit_count"].shape[1]
    sc = [s["ev_score"][e, c, s["vid_off"][o]:s["vid_off"][o] + s["ev_count"][e, c, o]].tolist()
          for e in range(E_) for c in range(C) for o in range(NV)]
    hp = [s["hit_pos"][e, t, s["gt_off"][oc]:s["gt_off"][oc] + s["hit_count"][e, t, oc]].tolist()
          for e in range(E_) for t in range(T) for oc in range(NV * K1)]
    return sc, hp


def exchange_ref(shares, split, K1):
    """the three phases over pretend ranks with numpy sums in between, in place"""
    ev_count = sum(s["ev_count"] for s in shares)
    hit_count = sum(s["hit_count"] for s in shares)
    pays = []
    for s, own in zip(shares, split):
        s["ev_count"], s["hit_count"] = ev_count.copy(), hit_count.copy()
        pays.append(E.ap_pack_ref(s["ev_score"], s["ev_count"], s["hit_pos"], s["hit_count"], s["vid_off"], s["gt_off"], K1, own))
    scores, hits = sum(p[0] for p in pays), sum(p[1] for p in pays)
    for s, own in zip(shares, split):
        E.ap_unpack_ref(s["ev_score"], s["ev_count"], s["hit_pos"], s["hit_count"], s["vid_off"], s["gt_off"], K1, own, scores, hits)
    return scores, hits


PACK_CASES = {
    "two_ranks": ([5, 3, 4], 5, 2, 3, [[0], [1, 2]]),
    "two_ranks_not_in_order": ([5, 3, 4], 5, 2, 3, [[2, 0], [1]]),
    "a_rank_with_no_video": ([5, 3, 4], 5, 1, 2, [[], [0, 1, 2]]),
    "three_ranks": ([5, 3, 4], 5, 2, 3, [[0], [1], [2]]),
    "one_class": ([6, 1, 2, 9], 2, 2, 1, [[3], [0, 1], [2]]),
}


@pytest.mark.parametrize("case", sorted(PACK_CASES))
def test_pack_and_unpack_of_pretend_ranks_reproduce_the_one_rank_stores(case):
    lengths, K1, E_, T, split = PACK_CASES[case]
    full = make_stores(lengths, K1, E_, T, seed=len(case))
    assert (full["ev_count"] == 0).any() and (full["hit_count"] == 0).any()            # empty segments are among the cases
    shares = [rank_share(full, own, K1) for own in split]
    scores, hits = exchange_ref(shares, split, K1)
    assert scores.dtype == np.float64 and hits.dtype == np.int32
    assert scores.shape == (int(full["ev_count"].sum()),) and hits.shape == (int(full["hit_count"].sum()),)
    assert not np.isnan(scores).any() and (hits >= 0).all()                              # nothing unused travelled
    want = used_parts(full, K1)
    for s in shares:
        assert np.array_equal(s["ev_count"], full["ev_count"]) and np.array_equal(s["hit_count"], full["hit_count"])
        assert used_parts(s, K1) == want
    # a rank's own payload holds its own segments and zeros: the sum has one writer per element
    own0 = E.ap_pack_ref(shares[0]["ev_score"], full["ev_count"], shares[0]["hit_pos"], full["hit_count"], full["vid_off"],
                         full["gt_off"], K1, split[0])
    if not split[0]:
        assert not own0[0].any() and not own0[1].any()


def test_unpack_does_not_write_own_segments():
    lengths, K1 = [4, 4], 3
    full = make_stores(lengths, K1, 1, 1, seed=3)
    share = rank_share(full, [0], K1)
    share["ev_count"], share["hit_count"] = full["ev_count"].copy(), full["hit_count"].copy()
    before = share["ev_score"][:, :, :4].copy()
    S, Hh = int(full["ev_count"].sum()), int(full["hit_count"].sum())
    E.ap_unpack_ref(share["ev_score"], share["ev_count"], share["hit_pos"], share["hit_count"], share["vid_off"], share["gt_off"],
                    K1, [0], np.full(S, 99.0), np.full(Hh, 99, np.int32))
    assert np.array_equal(share["ev_score"][:, :, :4], before, equal_nan=True)
    assert (share["ev_score"][0, 0, 4:4 + full["ev_count"][0, 0, 1]] == 99.0).all()


# ----------------------------------------------------------------------------- ownership
def test_ownership_errors_name_the_ordinals():
    assert ops.ap_owner_errors(np.ones(5, np.int32)) is None
    err = ops.ap_owner_errors(np.array([1, 2, 1, 0, 1, 0]))
    assert isinstance(err, RuntimeError)
    assert "twice [1]" in str(err) and "never [3, 5]" in str(err)
    assert "twice []" in str(ops.ap_owner_errors(np.array([1, 0]))) and "never [1]" in str(ops.ap_owner_errors(np.array([1, 0])))
    assert "twice [0]" in str(ops.ap_owner_errors(np.array([3, 1]))) and "never []" in str(ops.ap_owner_errors(np.array([3, 1])))


# ----------------------------------------------------------------------------- frame counters against the reference's numbers
def golden_labels(meta, videos):
    return {v: synth.labels(meta["seed"] + vi, 1, L, meta["K1"] - 1, 1, fg_frac=0.15)[0][0] for vi, (v, L, _) in enumerate(videos)}


def test_frame_counters_give_the_reference_error_and_f1():
    meta, g = load_golden("eval_utils")
    videos, classes, norm, _ = H.golden_inputs(meta)
    labels = golden_labels(meta, videos)
    K1 = meta["K1"]
    counters = sum(E.frame_stats_ref(norm[v], labels[v]) for v, _, _ in videos)
    assert counters.dtype == np.int64 and counters.shape == (2 + 3 * K1,)
    assert counters[0] == sum(L for _, L, _ in videos)
    stats = E.frame_stats_dict(counters, classes)
    assert abs(stats["err"] - float(g["err"])) < 1e-12
    assert abs(stats["f1"][None] - float(g["f1_any"])) < 1e-12
    assert np.allclose([stats["f1"][k] for k in range(1, K1)], g["f1_cls"], atol=1e-12)
    assert np.array_equal(np.array([stats["tp_fp_fn"][k] for k in [None] + list(range(1, K1))]), g["tpfpfn"])
    assert np.array_equal(counters[2:].reshape(K1, 3), g["tpfpfn"])                     # the layout itself
    want = E.frame_events(norm, classes, {v: f for v, _, f in videos}, meta["hr_thr"], labels=labels)[2]
    assert stats == want


# ----------------------------------------------------------------------------- argument errors before any launch
def test_shard_and_label_argument_errors_come_before_any_launch():
    """model=None: nothing below may reach the model, let alone a launch"""
    classes = {"c1": 1, "c2": 2}
    truth = [{"video": "a", "events": [{"label": "c1", "frame": 1}]}, {"video": "b", "events": []}]
    src = np.zeros((1,), np.uint8)                                        # a source that is never looked at
    vids = [("a", 5, 25.0, src), ("b", 7, 25.0, None)]
    # shard_videos([5, 7], 1) gives rank 0 both videos: "b" is its own and has no source
    with pytest.raises(ValueError, match=r"\['b'\].*no frame source"):
        E.map_videos(None, vids, classes, truth, [("raw",)], shard=(0, 1))
    with pytest.raises(ValueError, match=r"\['b'\].*no frame source"):
        E.map_videos(None, vids, classes, truth, [("raw",)])
    both = [("a", 5, 25.0, src), ("b", 7, 25.0, src)]
    good = {"a": np.zeros(5, np.int64), "b": np.zeros(7, np.int64)}
    for bad, what in ((dict(good, a=np.zeros(4, np.int64)), "5 integers"), (dict(good, b=np.full(7, 3)), r"0\.\.2"),
                      (dict(good, b=np.full(7, -1)), r"0\.\.2"), (dict(good, a=np.zeros(5, np.float32)), "5 integers"),
                      ({"a": good["a"]}, r"no labels for the videos \['b'\]")):
        with pytest.raises(ValueError, match=what):
            E.map_videos(None, both, classes, truth, [("raw",)], labels=bad)
    for shard in ("rank0", (2, 2), (-1, 2), (0, 0), (0.5, 2), 3, (0, 1, 2)):
        with pytest.raises(ValueError, match="shard must be"):
            E.map_videos(None, both, classes, truth, [("raw",)], shard=shard)
    with pytest.raises(ValueError, match="process group of 2 ranks"):
        E.map_videos(None, both, classes, truth, [("raw",)], shard=(1, 2))             # no process group in this process
    assert E.parse_shard(None) is None and E.parse_shard("auto") == (0, 1) and E.parse_shard((1, 4)) == (1, 4)
    with pytest.raises(ValueError, match="3 integers"):
        E.check_labels([np.zeros(2, np.int64)], [3], 4, "map_video_group")
