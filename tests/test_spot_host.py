"""`evalutil.nms_rounds` (the written statement of the suppression kernel's order) against the host chain it replaces:
`frame_events` -> `non_maximum_suppression` / `soft_non_maximum_suppression`, bit for bit.  Pure CPU.  The track builders
and the case lists are shared with tests/test_gpu_spot.py, which runs the device route on the same cases."""
import numpy as np
import pytest

from helpers import load_golden, act
from tdeed_amd import evalutil as E

LENGTHS = (1, 2, 37, 90)
COLS = (2, 5)
VARIANTS = ("uniform", "sixths", "sharp", "zero_rows")
THRESHOLDS = (0.0, 0.01, 0.05, 0.1)
HR_THRESHOLDS = (0.01, 0.0, 0.2)


def make_track(L, K1, variant, seed):
    """(L,K1) fp32, every row finite.  Rows are normalised BEFORE rows are zeroed (an all-zero row would divide 0 by 0)."""
    rng = np.random.RandomState(seed)
    x = rng.rand(L, K1).astype(np.float32)
    if variant == "sixths":
        x = np.floor(x * 6).astype(np.float32) + np.float32(1)            # 1..6: rows full of ties
    if variant == "sharp":
        x = x ** 6
        x[:, 0] += np.float32(1e-3)
    x /= x.sum(axis=1, keepdims=True)
    if variant == "sixths":
        x = (np.round(x * 6) / 6).astype(np.float32)                      # exact sixths, 0 included
    if variant == "zero_rows":
        x[rng.rand(L) < 0.3] = 0.0                                        # frames with support 0
    if K1 >= 4 and L >= 3:
        x[0, 1] = 0.0                                                     # labels appear in the order 2, 4, 1, 3:
        x[:2, 3] = 0.0                                                    # not the class order
    assert np.isfinite(x).all()
    return np.ascontiguousarray(x, np.float32)


def windows_for(K1):
    """1, 3, larger than every L above, and a list (indexed by label appearance, K1-1 entries)"""
    return [1, 3, 100, [3, 1, 2, 4, 6, 5, 2, 1, 3, 2, 7, 1, 4, 2, 3, 1, 5][:K1 - 1]]


def host_chain(mean, window, threshold, soft, hr):
    """the host route -> (frames, classes, scores) lists of the suppressed events, in the host's order"""
    K1 = mean.shape[1]
    classes = {f"c{k}": k for k in range(1, K1)}
    _, recall, _ = E.frame_events({"v": mean}, classes, {"v": 25.0}, high_recall_score_threshold=hr)
    fn = E.soft_non_maximum_suppression if soft else E.non_maximum_suppression
    out = fn(recall, window, threshold)[0]
    assert out["num_events"] == len(out["events"])
    evs = out["events"]
    return [e["frame"] for e in evs], [classes[e["label"]] for e in evs], [e["score"] for e in evs]


def grid_cases(L, K1, variant):
    """every (window, threshold, soft, hr) combination tested on one random track"""
    mean = make_track(L, K1, variant, 1000 * L + 10 * K1 + VARIANTS.index(variant))
    for wi, window in enumerate(windows_for(K1)):
        hr = HR_THRESHOLDS[(wi + VARIANTS.index(variant)) % 3]
        for thr in THRESHOLDS:
            for soft in (False, True):
                yield mean, window, thr, soft, hr


def _track_1class(L, values):
    m = np.zeros((L, 2), np.float32)
    for f, v in values.items():
        m[f, 1] = v
    return m


def boundary_cases():
    """id -> (mean, window, threshold, soft, hr, expected frames of class 1 | None)"""
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(0))
    out = {}
    # fp32 comparison against float32(0.01): the score that IS float32(0.01) is a candidate (as a double it is below 0.01)
    assert float(f32(0.01)) < 0.01
    out["hr_exact_fp32"] = (_track_1class(12, {2: f32(0.01), 7: below(0.01), 10: f32(0.5)}), 1, 0.0, False, 0.01, [2, 10])
    # double comparison against 0.1: float32(0.1) is above it, its predecessor below
    out["thr_exact_double"] = (_track_1class(12, {2: f32(0.1), 7: below(0.1), 10: f32(0.5)}), 1, 0.1, False, 0.01, [2, 10])
    out["thr_exact_double_soft"] = (_track_1class(12, {2: f32(0.1), 7: below(0.1), 10: f32(0.5)}), 1, 0.1, True, 0.01, [2, 10])
    # 0.5 * 1 / 9 < 0.1: decayed below the threshold, never emitted; frame 14 (distance 3) keeps its score
    out["soft_decay_drops"] = (_track_1class(20, {10: f32(0.9), 11: f32(0.5), 14: f32(0.3)}), 3, 0.1, True, 0.01, [10, 14])
    # class 2 has no candidate: class 3 is the second label to appear and takes the list's second window
    m = np.zeros((30, 4), np.float32)
    m[3:28, 1] = np.linspace(0.2, 0.6, 25, dtype=np.float32)
    m[5:25, 3] = np.linspace(0.7, 0.3, 20, dtype=np.float32)
    m[:, 2] = f32(0.001)
    out["rank_skips_empty_class"] = (m, [1, 5, 9], 0.01, False, 0.01, None)
    out["rank_skips_empty_class_soft"] = (m, [1, 5, 9], 0.01, True, 0.01, None)
    # monotone ramp: one winner per round
    ramp = _track_1class(400, {f: f32(0.02 + 0.9 * f / 400) for f in range(400)})
    out["ramp_hard"] = (ramp, 3, 0.01, False, 0.01, None)
    out["ramp_soft"] = (ramp, 3, 0.01, True, 0.01, None)
    return out


def check_equal(got, want, tag):
    frames, classes, scores = got[:3]
    assert [int(f) for f in frames] == want[0], tag
    assert [int(c) for c in classes] == want[1], tag
    assert [float(s) for s in scores] == want[2], tag


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K1", COLS)
@pytest.mark.parametrize("L", LENGTHS)
def test_nms_rounds_equals_the_host_chain(L, K1, variant):
    n_events = 0
    for mean, window, thr, soft, hr in grid_cases(L, K1, variant):
        got = E.nms_rounds(mean, window, thr, soft, hr)
        want = host_chain(mean, window, thr, soft, hr)
        check_equal(got, want, (window, thr, soft, hr))
        n_cand = (mean[:, 1:] >= np.float32(hr)).sum(axis=0)
        assert (got[3][1:] <= n_cand).all() and got[3][0] == 0
        n_events += len(want[0])
    assert n_events > 0


def test_list_window_follows_label_appearance_not_class_order():
    mean = make_track(37, 5, "uniform", 5)
    first = [37] + [int(np.nonzero(mean[:, c] >= np.float32(0.01))[0][0]) for c in range(1, 5)]
    assert E.label_order(first, 37) == [2, 4, 1, 3]
    by_rank = E.nms_rounds(mean, [3, 1, 2, 4], 0.01, False, 0.01)
    by_class = E.nms_rounds(mean, [2, 3, 4, 1], 0.01, False, 0.01)          # the same windows, had the list been per class
    check_equal(by_class, host_chain(mean, [2, 3, 4, 1], 0.01, False, 0.01), "by_class")
    assert by_rank[0].tolist() != by_class[0].tolist() or by_rank[1].tolist() != by_class[1].tolist()


@pytest.mark.parametrize("name", sorted(boundary_cases()))
def test_nms_rounds_boundaries(name):
    mean, window, thr, soft, hr, frames1 = boundary_cases()[name]
    got = E.nms_rounds(mean, window, thr, soft, hr)
    check_equal(got, host_chain(mean, window, thr, soft, hr), name)
    if frames1 is not None:
        assert got[0][got[1] == 1].tolist() == frames1
    if name.startswith("rank_skips"):
        assert set(got[1].tolist()) == {1, 3}
    if name.startswith("ramp"):
        # hard: the top of the ramp wins, removes itself and 3 below it -> 400 / 4 rounds; soft takes more
        assert got[3][1] == 100 if not soft else got[3][1] > 100
        assert got[3][1] <= 400


def test_nms_rounds_refuses_a_soft_window_of_zero():
    with pytest.raises(ValueError):
        E.nms_rounds(make_track(5, 2, "uniform", 0), 0, 0.01, True, 0.01)
    assert len(E.nms_rounds(make_track(5, 2, "uniform", 0), 0, 0.0, False, 0.0)[0]) == 5     # hard, w = 0: every candidate


# ----------------------------------------------------------------------------- the golden inputs of test_evalutil
def golden_inputs(meta):
    """the inputs of tests/test_evalutil.py::_inputs, built the same way -> (videos, classes, normalised tracks, fps)"""
    seed, K1, T = meta["seed"], meta["K1"], meta["T"]
    videos = [tuple(v) for v in meta["videos"]]
    classes = {f"c{k}": k for k in range(1, K1)}
    st = E.ScoreStitcher(videos, K1)
    for vi, (v, L, _) in enumerate(videos):
        for ci, start in enumerate(range(-T // 2, L, T // 2)):
            sc = np.abs(act(seed + 10 * vi + ci, f"clip{vi}_{ci}", (T, K1))).astype(np.float32)
            sc[:, 0] *= 2.5
            sc /= sc.sum(axis=1, keepdims=True)
            sc[(ci * 7) % T] = 0.0
            st.add(v, start, sc)
    return videos, classes, st.normalised(), st.fps


GOLDEN_NMS = {"nms1": (2, 0.10, False), "nms2": ([1, 3, 2, 4], 0.0, False), "snms": (3, 0.05, True)}


def check_golden(g, tag, video, frames, classes, scores):
    want = g[f"{tag}__{video}"]
    assert want.shape == (len(frames), 3), (tag, video, len(frames), want.shape)
    if want.size:
        assert np.array_equal(np.asarray(frames, np.float64), want[:, 0]), (tag, video)
        assert np.array_equal(np.asarray(classes, np.float64), want[:, 1]), (tag, video)
        assert np.allclose(np.asarray(scores, np.float64), want[:, 2], rtol=1e-6, atol=1e-9), (tag, video)


def test_nms_rounds_reproduces_the_reference_goldens():
    meta, g = load_golden("eval_utils")
    videos, _, norm, _ = golden_inputs(meta)
    n = 0
    for tag, (window, thr, soft) in GOLDEN_NMS.items():
        for v, _, _ in videos:
            frames, classes, scores, _ = E.nms_rounds(norm[v], window, thr, soft, meta["hr_thr"])
            check_golden(g, tag, v, frames, classes, scores)
            n += len(frames)
    assert n > 0
