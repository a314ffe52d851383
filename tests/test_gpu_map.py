"""mAP on the MI355X: `ops.ap_match_seg` / `ops.ap_rank` against the host restatement (`evalutil.ap_restated`), exactly in
every integer and within summation order in the APs; against `mean_average_precisions` on the lists the device suppression
returns; order independence; the reference golden; a video beyond the in-LDS capacity; `evalutil.map_videos` end to end.
-m gpu only."""
import functools

import numpy as np
import pytest
import torch

from helpers import t, load_golden
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth
import test_spot_host as H
import test_ap_host as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENTRIES = (("raw",), ("nms", 1, 0.10), ("snms", 3, 0.01))


def ap_bound(total):
    """an AP differs from the host's only by summation order: h <= total terms <= 1 and one division"""
    return max(1, total) * 2.0 ** -52


def device_route(tracks, ords, entries, tols, truth, hr=0.01, groups=None):
    """tracks: normalised (L_v,K1) fp32 tracks; ords[v] the ordinal of track v; truth: {(ordinal, class): [frames]};
    groups: lists of track indices, one packed track and one launch series each (default: one group).
    -> (state, ap, nhits, rank) with the three tables on the host"""
    K1 = tracks[0].shape[1]
    by_ord = {o: i for i, o in enumerate(ords)}
    state = ops.ap_state([tracks[by_ord[o]].shape[0] for o in range(len(tracks))], truth, K1, len(entries), tols, DEV)
    for idx in groups or [list(range(len(tracks)))]:
        lens = [tracks[i].shape[0] for i in idx]
        mean = torch.from_numpy(np.concatenate([tracks[i] for i in idx])).to(DEV)
        seg_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)
        od = torch.tensor([ords[i] for i in idx], dtype=torch.int32, device=DEV)
        first = ops.frame_events_seg(mean, seg_off, max(lens), hr)[2]
        for e, entry in enumerate(entries):
            planes = None
            if entry[0] != "raw":
                planes = ops.nms_track_seg(mean, seg_off, max(lens), entry[1], entry[2], entry[0] == "snms", first, hr,
                                           planes=True)[5:]
            ops.ap_match_seg(state, e, mean, seg_off, od, max(lens), hr, planes=planes)
    ap, nhits, rank = ops.ap_rank(state)
    torch.cuda.synchronize()
    return state, ap.cpu().numpy(), nhits.cpu().numpy(), rank.cpu().numpy()


def host_route(tracks, ords, entries, tols, truth, hr=0.01):
    """{(entry index, class, tolerance index): ap_restated's dict}, videos in ordinal order"""
    K1, nv = tracks[0].shape[1], len(tracks)
    by_ord = {o: i for i, o in enumerate(ords)}
    out = {}
    for e, entry in enumerate(entries):
        lists = [A.track_lists(tracks[by_ord[o]], entry, hr) for o in range(nv)]
        for c in range(1, K1):
            for ti, tol in enumerate(tols):
                out[e, c, ti] = E.ap_restated([lists[o][c] for o in range(nv)], [truth.get((o, c), []) for o in range(nv)], tol)
    return out


def check_against_restatement(state, ap, nhits, rank, want, tag):
    """every integer exactly, the APs within the summation bound"""
    K1, NV = state.K1, state.NV
    ev_count = state.ev_count.cpu().numpy()
    ev_frame, ev_score = state.ev_frame.cpu().numpy(), state.ev_score.cpu().numpy()
    hit_count, hit_pos = state.hit_count.cpu().numpy(), state.hit_pos.cpu().numpy()
    gt_off, vid_off = state.gt_off.cpu().numpy(), state.vid_off_host
    n_hits = 0
    for (e, c, ti), d in want.items():
        for o in range(NV):
            n = len(d["frames"][o])
            assert ev_count[e, c - 1, o] == n, (tag, e, c, o)
            assert np.array_equal(ev_frame[e, c - 1, vid_off[o]:vid_off[o] + n], d["frames"][o]), (tag, e, c, o)
            assert np.array_equal(ev_score[e, c - 1, vid_off[o]:vid_off[o] + n], d["scores"][o]), (tag, e, c, o)
            nh, g0 = len(d["hits"][o]), gt_off[o * K1 + c]
            assert hit_count[e, ti, o * K1 + c] == nh, (tag, e, c, ti, o, hit_count[e, ti, o * K1 + c], nh)
            assert hit_pos[e, ti, g0:g0 + nh].tolist() == d["hits"][o], (tag, e, c, ti, o)
            assert rank[e, ti, g0:g0 + nh].tolist() == d["ranks"][o], (tag, e, c, ti, o)
            n_hits += nh
        assert nhits[e, ti, c] == sum(len(h) for h in d["hits"]), (tag, e, c, ti)
        assert state.totals[c] == d["total"]
        assert abs(ap[e, ti, c] - d["ap"]) <= ap_bound(d["total"]), (tag, e, c, ti, ap[e, ti, c], d["ap"])
    assert (ap[:, :, 0] == 0).all() and (nhits[:, :, 0] == 0).all()
    return n_hits


@functools.lru_cache(maxsize=None)
def grid_case(L, K1, nv, variant):
    """tracks (the middle one of three shorter), ordinals that are not the arrival order, the truth of A.truth_cases"""
    lens = [L] if nv == 1 else [L, (L + 1) // 2, L]
    tracks = [H.make_track(n, K1, variant, 31 * L + 7 * K1 + v) for v, n in enumerate(lens)]
    ords = [0] if nv == 1 else [2, 0, 1]
    truth = {}
    for v, o in enumerate(ords):
        for c in range(1, K1):
            g = A.truth_cases(lens[v], c, o)
            if g:
                truth[o, c] = g
    tols = (0, 1, 2, L)
    return tracks, ords, truth, tols, host_route(tracks, ords, ENTRIES, tols, truth)


@pytest.mark.parametrize("nv", [1, 3])
@pytest.mark.parametrize("K1", [2, 5])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 257, 1025])
def test_match_and_rank_equal_the_restatement(L, K1, nv):
    """"sixths" is make_track's quantised variant: scores tie within and across videos"""
    n_hits = 0
    for variant in ("uniform", "sixths"):
        tracks, ords, truth, tols, want = grid_case(L, K1, nv, variant)
        got = device_route(tracks, ords, ENTRIES, tols, truth)
        n_hits += check_against_restatement(*got, want, (L, K1, nv, variant))
        again = device_route(tracks, ords, ENTRIES, tols, truth)
        for a, b in zip(got[1:], again[1:]):
            assert np.array_equal(a, b)                                 # two runs: identical bits
    assert n_hits > 0


def _records(tracks, ords, lists_per_track):
    """per-track {c: (frames, scores)} -> the reference's records in ordinal order (events by frame, then class)"""
    by_ord = {o: i for i, o in enumerate(ords)}
    out = []
    for o in range(len(tracks)):
        evs = [(int(f), c, float(s)) for c, (fr, sc) in lists_per_track[by_ord[o]].items() for f, s in zip(fr, sc)]
        out.append({"video": f"v{o:02d}", "events": [{"label": f"c{c}", "frame": f, "score": s} for f, c, s in sorted(evs)]})
    return out


def test_ap_table_against_mean_average_precisions_on_the_device_lists():
    """the lists `ops.nms_track_seg` returns, as records through `mean_average_precisions`, against the device table"""
    L, K1 = 257, 5
    tracks, ords, truth, tols, _ = grid_case(L, K1, 3, "sixths")
    entries = ENTRIES[1:]
    _, ap, _, _ = device_route(tracks, ords, entries, tols, truth)
    truth_rec = [{"video": f"v{o:02d}", "events": [{"label": f"c{c}", "frame": f} for c in range(1, K1) for f in truth.get((o, c), [])]}
                 for o in range(3)]
    for e, (kind, w, thr) in enumerate(entries):
        lists = []
        for m in tracks:
            fr, cl, sc, cnt, _ = ops.nms_track(torch.from_numpy(m).to(DEV), w, thr, kind == "snms", 0.01)
            n = int(cnt.cpu()[0])
            fr, cl, sc = fr[:n].cpu().numpy(), cl[:n].cpu().numpy(), sc[:n].cpu().numpy()
            lists.append({c: (fr[cl == c], sc[cl == c]) for c in range(1, K1)})
        maps, aps = E.mean_average_precisions(truth_rec, _records(tracks, ords, lists), list(tols))
        assert sorted(aps) == [f"c{c}" for c in range(1, K1)]
        for c in range(1, K1):
            total = sum(len(truth.get((o, c), [])) for o in range(3))
            for ti in range(len(tols)):
                assert abs(ap[e, ti, c] - aps[f"c{c}"][ti]) <= ap_bound(total), (e, c, ti)
        assert max(maps) > 0


def test_groups_in_any_order_give_identical_bits():
    """four videos whose scores tie across videos: one group; groups of two arriving in reversed order; the first again"""
    K1, lens = 5, [90, 64, 37, 90]
    tracks = [H.make_track(n, K1, "sixths", 500 + v) for v, n in enumerate(lens)]
    ords = [0, 1, 2, 3]
    truth = {(o, c): A.truth_cases(lens[o], c, o + 1) for o in range(4) for c in range(1, K1) if A.truth_cases(lens[o], c, o + 1)}
    tols = (0, 1, 2, 90)
    one = device_route(tracks, ords, ENTRIES, tols, truth)
    two = device_route(tracks, ords, ENTRIES, tols, truth, groups=[[3, 2], [1, 0]])
    again = device_route(tracks, ords, ENTRIES, tols, truth)
    for a, b, c in zip(one[1:], two[1:], again[1:]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert one[2].sum() > 0
    check_against_restatement(*two, host_route(tracks, ords, ENTRIES, tols, truth), "groups of two")


def test_the_reference_goldens_through_the_device_route():
    meta, g = load_golden("eval_utils")
    videos, classes, norm, _ = H.golden_inputs(meta)
    names = sorted(v for v, _, _ in videos)
    tracks = [np.ascontiguousarray(norm[v]) for v in names]
    ords = list(range(len(names)))
    ordinal = {v: i for i, v in enumerate(names)}
    table = E.truth_table(A.golden_truth(meta, videos), ordinal, classes)
    labelled = sorted({c for _, c in table})
    for entry, tols, key in ((("raw",), [0, 1, 2, 4], "maps_hr"), (("nms", 2, 0.10), [1, 2, 4], "maps_nms")):
        _, ap, _, _ = device_route(tracks, ords, [entry], tols, table, hr=meta["hr_thr"])
        maps = [float(np.mean([ap[0, ti, c] for c in labelled])) for ti in range(len(tols))]
        assert np.allclose(maps, g[key], atol=1e-12), (key, maps, g[key])


@pytest.mark.parametrize("beyond", [0, 1], ids=["largest_in_lds", "first_in_the_store"])
def test_a_video_at_and_beyond_the_in_lds_capacity(beyond):
    """the longest video the kernel orders in LDS and one frame more (ordered in place in the store), every frame an event
    (hr 0), scores from 97 levels: ties everywhere"""
    L = ops.ap_lds_frames() + beyond
    mean = np.zeros((L, 2), np.float32)
    mean[:, 1] = (np.random.RandomState(5).randint(0, 97, size=L) / np.float32(97)).astype(np.float32)
    truth = {(0, 1): [int(f) for f in np.random.RandomState(6).permutation(L)[:130]]}
    tols = (0, 1, 2, L)
    entries = [("raw",)]
    got = device_route([mean], [0], entries, tols, truth, hr=0.0)
    assert got[0].ev_count.cpu().numpy()[0, 0, 0] == L
    n = check_against_restatement(*got, host_route([mean], [0], entries, tols, truth, hr=0.0), f"capacity + {beyond}")
    assert n == 4 * 130


# ----------------------------------------------------------------------------- end to end, tiny model
def test_map_videos_equals_spot_videos_and_mean_average_precisions():
    from test_gpu_spot import TINY, CLASSES, _model
    m = _model(TINY)
    lens = {"b": 37, "a": 23, "c": 30}
    frames = {v: t(synth.uint8_clip(4100 + 100 * i, (n, 3, 64, 64))) for i, (v, n) in enumerate(lens.items())}
    vids = [("b", 37, 25.0, frames["b"]), ("a", 23, 30.0, lambda: frames["a"]), ("c", 30, 25.0, frames["c"])]
    truth = [{"video": v, "events": [{"label": "c1", "frame": 3}, {"label": "c2", "frame": 10}, {"label": "c2", "frame": 10},
                                     {"label": "c3", "frame": 17}, {"label": "c1", "frame": n - 1}]} for v, n in lens.items()]
    suppress = (("raw",), ("nms", 1, 0.01), ("snms", [3, 1, 2], 0.01))
    tols = [0, 1, 2, 4]
    kw = dict(augment=True, batch_size=4, group_videos=2)
    _, lists, _ = E.spot_videos(m, vids, CLASSES, suppress[1:], **kw)
    st = E.stitch_videos(m, vids, 4, **kw)
    recall = E.frame_events(st.normalised(), CLASSES, st.fps, high_recall_score_threshold=0.01)[1]
    got = E.map_videos(m, vids, CLASSES, truth, suppress, tols, **kw)
    stats = dict(m.last_video_stats)
    assert len(got) == 3
    for (maps, aps), ref in zip(got, [recall] + lists):
        want_maps, want_aps = E.mean_average_precisions(truth, ref, tols)
        assert sorted(aps) == sorted(want_aps) == ["c1", "c2", "c3"]
        for lab in aps:
            for a, b in zip(aps[lab], want_aps[lab]):
                assert abs(a - b) <= ap_bound({"c1": 6, "c2": 6, "c3": 3}[lab]), (lab, a, b)
        assert np.allclose(maps, want_maps, rtol=0, atol=ap_bound(6) + 2.0 ** -52)      # the mean of APs within ap_bound each
    assert max(got[0][0]) > 0
    assert stats["groups"] == 2 and stats["host_syncs"] <= stats["groups"] + 1
    assert stats["frames"] == 90 and stats["videos"] == 3
    assert stats["ap_d2h_bytes"] == 3 * 4 * 4 * 12
    # far fewer events (a high-recall threshold most scores miss): the same bytes come back
    E.map_videos(m, vids, CLASSES, truth, suppress, tols, high_recall_score_threshold=0.3, **kw)
    assert m.last_video_stats["ap_d2h_bytes"] == stats["ap_d2h_bytes"]


def test_map_argument_errors_come_before_any_launch():
    """model=None: nothing below may reach the model, let alone a launch"""
    vids = [("a", 5, 25.0, None), ("b", 7, 25.0, None)]
    classes = {"c1": 1, "c2": 2}
    truth = [{"video": "a", "events": [{"label": "c1", "frame": 1}]}, {"video": "b", "events": []}]
    with pytest.raises(ValueError, match="suppress entry"):
        E.map_videos(None, vids, classes, truth, [("median", 1, 0.1)])
    with pytest.raises(AssertionError, match="Video set mismatch!"):
        E.map_videos(None, vids, classes, truth + [{"video": "z", "events": []}], [("raw",)])
    with pytest.raises(ValueError, match="tolerances"):
        E.map_videos(None, vids, classes, truth, [("raw",)], tolerances=[])
    with pytest.raises(ValueError, match="tolerances"):
        E.map_videos(None, vids, classes, truth, [("raw",)], tolerances=list(range(ops.ap_max_tolerances() + 1)))
    with pytest.raises(ValueError, match="tolerances"):
        E.map_videos(None, vids, classes, truth, [("raw",)], tolerances=[0.5])
    state = ops.ap_state([5, 7], {(0, 1): [1]}, 3, 1, [0, 1], DEV)
    mean = torch.rand((12, 3), device=DEV)
    seg = torch.tensor([0, 5, 12], dtype=torch.int32, device=DEV)
    od = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.ap_match_seg(state, 1, mean, seg, od, 7)                    # one entry: index 1 does not exist
    with pytest.raises(ValueError):
        ops.ap_match_seg(state, 0, mean, seg, od[:1], 7)
    with pytest.raises(ValueError):
        ops.ap_match_seg(state, 0, mean, seg, od, 7, planes=(torch.zeros((3, 12), device=DEV), torch.zeros((3, 12), device=DEV)))
    with pytest.raises(ValueError):
        ops.ap_state([5, 7], {(0, 1): list(range(ops.ap_max_truth(2) + 1))}, 3, 1, [0, 1], DEV)
    with pytest.raises(ValueError):
        ops.ap_state([5, 7], {(2, 1): [1]}, 3, 1, [0], DEV)
