"""The decomposition of `evalutil.average_precision` that the device route computes -- matching per video, hit ranks by
counting, AP from the hits (`ap_match_video`, `ap_hit_ranks`, `ap_from_ranks`) -- against `average_precision` /
`mean_average_precisions` themselves.  Pure CPU.  The case builders are shared with tests/test_gpu_map.py, which runs the device
route on the same kind of cases."""
import numpy as np
import pytest

from helpers import load_golden
from tdeed_amd import synth, evalutil as E
import test_spot_host as H


def random_records(seed, nv, labels, L, quant, extra_pred_label=True):
    """truth / pred records of nv videos "v0".. of L frames: per label and video a random subset of frames with scores from
    `quant` levels (ties within and across videos), an empty video now and then, truth lists unsorted with duplicates, one truth
    label nobody predicts ("only_truth") and one predicted label the truth does not know ("only_pred")."""
    rng = np.random.RandomState(seed)
    truth, pred = [], []
    for v in range(nv):
        evs, gts = [], []
        empty = rng.rand() < 0.2
        for lab in labels:
            if not empty:
                frames = np.sort(rng.choice(L, size=rng.randint(0, L + 1), replace=False))
                for f in frames:
                    evs.append({"label": lab, "frame": int(f), "score": float(rng.randint(1, quant + 1)) / quant})
            g = rng.randint(0, L, size=rng.randint(1 if v == 0 else 0, 7)).tolist()      # every label is in the truth
            if g and rng.rand() < 0.5:
                g += [g[0]] * rng.randint(1, 3)                        # duplicates of a frame
            for f in rng.permutation(g).tolist():                       # list order is not frame order
                gts.append({"label": lab, "frame": int(f)})
        if extra_pred_label and not empty:
            evs.append({"label": "only_pred", "frame": int(rng.randint(L)), "score": 0.5})
        gts.append({"label": "only_truth", "frame": int(rng.randint(L))})
        evs.sort(key=lambda e: e["frame"])                              # stable: the order the suppression functions leave
        pred.append({"video": f"v{v}", "events": evs})
        truth.append({"video": f"v{v}", "events": gts})
    return truth, pred


@pytest.mark.parametrize("seed", range(24))
def test_counting_equals_average_precision_on_random_cases(seed):
    rng = np.random.RandomState(1000 + seed)
    nv, L, quant = int(rng.randint(1, 6)), int(rng.choice([1, 5, 23, 60])), int(rng.choice([1, 3, 1000]))
    truth, pred = random_records(seed, nv, ["a", "b", "c"], L, quant)
    tols = [0, 1, 2, 50]
    maps, aps = E.mean_average_precisions(truth, pred, tols)
    maps2, aps2, detail = E.mean_average_precisions_by_counting(truth, pred, tols)
    assert sorted(aps2) == sorted(aps) == ["a", "b", "c", "only_truth"]
    assert aps2["only_truth"] == [0.0] * 4                              # a truth label without predictions
    for lab in aps:
        assert aps2[lab] == aps[lab], (lab, aps[lab], aps2[lab])        # difference 0.0
    assert maps2 == maps
    # the ranks are positions in the list `mean_average_precisions` sorts: distinct, and at most the label's predictions
    for (lab, tol), d in detail.items():
        ranks = [r for rv in d["ranks"] for r in rv]
        n_pred = sum(1 for x in pred for e in x["events"] if e["label"] == lab)
        assert len(set(ranks)) == len(ranks) and all(1 <= r <= n_pred for r in ranks)
        assert len(ranks) <= d["total"]


def test_equidistant_truth_on_both_sides_list_order_decides():
    pred = [(0, 10, 0.9), (0, 12, 0.8)]
    for gt, first in (([11, 9], 11), ([9, 11], 9)):
        order, hits = E.ap_match_video([10, 12], [0.9, 0.8], gt, 1)
        assert order.tolist() == [0, 1]
        # frame 10 takes the first of the two at distance 1; frame 12 then reaches 11 only if 11 is still open
        assert hits == ([0] if first == 11 else [0, 1])
        want = E.average_precision([("v", f, s) for _, f, s in pred], {"v": gt}, 1)
        got = E.ap_restated([([10, 12], [0.9, 0.8])], [gt], 1)
        assert got["ap"] == want


def test_a_hit_closes_every_duplicate_and_total_counts_them():
    got = E.ap_restated([([5, 6], [0.9, 0.8])], [[5, 5, 5]], 0)
    assert got["hits"] == [[0]] and got["total"] == 3 and got["ap"] == 1.0 / 3.0
    assert got["ap"] == E.average_precision([("v", 5, 0.9), ("v", 6, 0.8)], {"v": [5, 5, 5]}, 0)


def test_ties_across_videos_go_to_the_earlier_ordinal():
    # both videos predict frame 3 with score 0.5; only the second one hits: its rank is 2
    d = E.ap_restated([([3], [0.5]), ([3], [0.5])], [[], [3]], 0)
    assert d["ranks"] == [[], [2]] and d["ap"] == 0.5
    d = E.ap_restated([([3], [0.5]), ([3], [0.5])], [[3], []], 0)
    assert d["ranks"] == [[1], []] and d["ap"] == 1.0


def test_video_set_mismatch_is_the_reference_assertion():
    truth, pred = random_records(3, 2, ["a"], 5, 3)
    with pytest.raises(AssertionError, match="Video set mismatch!"):
        E.mean_average_precisions_by_counting(truth[:1], pred, [0])


def test_map_videos_refuses_bad_arguments_before_it_touches_the_model():
    """model=None: every check below comes before the first use of the model (and so before any launch)"""
    vids = [("a", 5, 25.0, None), ("b", 7, 25.0, None)]
    classes = {"c1": 1, "c2": 2}
    truth = [{"video": "a", "events": [{"label": "c1", "frame": 1}]}, {"video": "b", "events": []}]
    with pytest.raises(ValueError, match="suppress entry"):
        E.map_videos(None, vids, classes, truth, [("median", 1, 0.1)])
    with pytest.raises(AssertionError, match="Video set mismatch!"):
        E.map_videos(None, vids, classes, truth[:1], [("raw",)])
    for tols in ([], list(range(9)), [0.5], [-1]):
        with pytest.raises(ValueError, match="tolerances"):
            E.map_videos(None, vids, classes, truth, [("raw",)], tolerances=tols)
    with pytest.raises(ValueError, match="not one of the model's classes"):
        E.map_videos(None, vids, classes, [truth[0], {"video": "b", "events": [{"label": "zz", "frame": 0}]}], [("raw",)])


def test_counting_reproduces_the_reference_goldens():
    """the route of tests/test_evalutil.py with the restated mAP: pins the decomposition to the reference's numbers"""
    meta, g = load_golden("eval_utils")
    videos, classes, norm, fps = H.golden_inputs(meta)
    truth = golden_truth(meta, videos)
    _, pehr, _ = E.frame_events(norm, classes, fps, high_recall_score_threshold=meta["hr_thr"])
    nms1 = E.non_maximum_suppression(pehr, window=2, threshold=0.10)
    assert np.allclose(E.mean_average_precisions_by_counting(truth, pehr, [0, 1, 2, 4])[0], g["maps_hr"], atol=1e-12)
    assert np.allclose(E.mean_average_precisions_by_counting(truth, nms1, [1, 2, 4])[0], g["maps_nms"], atol=1e-12)


def golden_truth(meta, videos):
    """the truth records of tests/test_evalutil.py: every foreground frame of the golden's synthetic labels"""
    labels = {v: synth.labels(meta["seed"] + vi, 1, L, meta["K1"] - 1, 1, fg_frac=0.15)[0][0] for vi, (v, L, _) in enumerate(videos)}
    return [{"video": v, "events": [{"label": f"c{int(k)}", "frame": int(i)} for i, k in enumerate(labels[v]) if k != 0]}
            for v, _, _ in videos]


# ----------------------------------------------------------------------------- shared with tests/test_gpu_map.py
def track_lists(mean, entry, hr=0.01):
    """the event list of one video's normalised track under a suppress entry, per class: {c: (frames, scores)} -- `nms_rounds`
    for the suppressions, the high-recall list of `frame_events` for ("raw",)"""
    K1 = mean.shape[1]
    if entry[0] == "raw":
        out = {}
        for c in range(1, K1):
            f = np.nonzero(mean[:, c] >= np.float32(hr))[0]
            out[c] = (f.astype(np.int64), mean[f, c].astype(np.float64))
        return out
    frames, classes, scores, _ = E.nms_rounds(mean, entry[1], entry[2], entry[0] == "snms", hr)
    return {c: (frames[classes == c].astype(np.int64), scores[classes == c]) for c in range(1, K1)}


def truth_cases(L, c, v):
    """ground truth of (class, video), chosen by (c + v) % 5: none; one frame; duplicates of a frame; two frames at equal
    distance from frame L // 2, the later one first in the list; 130 frames (more than two waves of lanes) where L allows"""
    k = (c + v) % 5
    mid = L // 2
    if k == 0:
        return []
    if k == 1:
        return [min(L - 1, mid + 1)]
    if k == 2:
        return [mid, mid, max(0, mid - 3), mid]
    if k == 3:
        return [min(L - 1, mid + 2), max(0, mid - 2)]
    n = min(130, L)
    return [int(f) for f in np.random.RandomState(L + 7 * c + v).permutation(L)[:n]]
