"""The rules of live scoring (tdeed_amd.liveplan) on the host: the closed forms against brute force, the schedule against
`predict_video`'s batches, and the numpy twin of the incremental stitch kernel bit for bit against
`evalutil.stitch_clip_scores` at the smallest score ring.  No GPU, no torch."""
import itertools

import numpy as np
import pytest

from tdeed_amd import evalutil as E
from tdeed_amd import liveplan as LP

GRID = [(T, ov, pad) for T in (1, 2, 6, 8) for ov in (0, 1, 3, 6) if ov < T for pad in (0, 2, 5)]


def _start(j, T, ov, pad):
    return -pad + j * (T - ov)


# ----------------------------------------------------------------------------- 1. the closed forms
@pytest.mark.parametrize("T,ov,pad", GRID)
def test_closed_forms_equal_brute_force(T, ov, pad):
    far = 200                                                   # clips well past every frame of the sweep
    for pushed in range(40):
        ready = LP.clips_ready(pushed, T, ov, pad)
        assert ready == sum(1 for j in range(far) if _start(j, T, ov, pad) + T - 1 < pushed)
        for L in range(max(pushed, 1), 40):
            starts = E.video_clip_starts(L, T, ov, pad_len=pad)
            assert LP.close_clips(L, T, ov, pad) == len(starts)
            # the ready clips are a prefix of the clip list of every video that is at least as long
            assert ready <= len(starts)
            assert starts[:ready] == [_start(j, T, ov, pad) for j in range(ready)]
            assert all(LP.clip_start(j, T, ov, pad) == s for j, s in enumerate(starts))
            # no clip outside the scored prefix covers a final row, and the first row that is not final is covered by one
            # (or lies behind everything the grid could still cover: it is the next clip's start)
            for scored in {0, ready // 2, ready}:
                fin = LP.final_rows(scored, T, ov, pad)
                assert fin == sum(1 for r in range(far) if all(_start(j, T, ov, pad) > r for j in range(scored, far)))
                assert all(not (s <= r < s + T) for s in starts[scored:] for r in range(min(fin, L)))
    assert LP.final_rows(0, T, ov, pad) == 0


def test_wrong_grids_and_sizes_are_refused():
    for T, ov, pad in ((0, 0, 0), (4, 4, 0), (4, -1, 0), (4, 1, -1)):
        with pytest.raises(ValueError):
            LP.clips_ready(3, T, ov, pad)
        with pytest.raises(ValueError):
            LP.LiveSchedule(T, ov, pad, 1)
    with pytest.raises(ValueError):
        LP.clips_ready(-1, 4, 1, 0)
    with pytest.raises(ValueError):
        LP.track_ring_rows(0, 4, 1)
    with pytest.raises(ValueError):
        LP.frame_ring_rows(2, 0, 4, 1)
    with pytest.raises(ValueError):
        LP.LiveSchedule(4, 1, 0, 0)


# ----------------------------------------------------------------------------- 2. the schedule
def _patterns(L, rng):
    yield [1] * L
    yield [L]
    yield [5] * (L // 5) + ([L % 5] if L % 5 else [])
    if L > 7:
        yield [L - 7, 7]
    for _ in range(3):
        cuts = sorted(set(rng.integers(1, L, size=rng.integers(1, 6)).tolist())) if L > 1 else []
        yield [b - a for a, b in zip([0] + cuts, cuts + [L])]


@pytest.mark.parametrize("T,ov,pad", [(6, 4, 5), (6, 3, 0), (6, 0, 2), (8, 6, 5), (1, 0, 0), (2, 1, 5)])
@pytest.mark.parametrize("bs", [1, 2, 3, 50])
def test_the_schedule_runs_predict_videos_batches_and_emits_every_row_once(T, ov, pad, bs):
    rng = np.random.default_rng(7)
    W = LP.track_ring_rows(bs, T, ov)
    for L in (1, 2, 5, 6, 7, 13, 37, 41):
        starts = E.video_clip_starts(L, T, ov, pad_len=pad)
        if not starts:
            continue
        want = [starts[i:i + bs] for i in range(0, len(starts), bs)]
        for pattern in _patterns(L, rng):
            sc = LP.LiveSchedule(T, ov, pad, bs)
            got, rows, open_batches = [], 0, 0
            for m in pattern:
                for x in sc.push(m):
                    assert len(x["starts"]) == bs and x["limit"] == sc.pushed
                    assert x["starts"][-1] + T <= x["limit"]               # complete: the window needs no frame that is missing
                    got.append(x)
                    open_batches += 1
                # everything that can run has run, and the rows that are final are liveplan's
                assert 0 <= LP.clips_ready(sc.pushed, T, ov, pad) - sc.scored < bs
                assert sc.rows_final == LP.final_rows(sc.scored, T, ov, pad) <= sc.pushed
                # latency: the row of frame p is final when frame p + latency_frames is in
                assert sc.rows_final >= sc.pushed - LP.latency_frames(bs, T, ov)
            assert sc.pushed == L
            got += sc.close()
            assert sc.closed and sc.rows_final == L
            assert [x["starts"] for x in got if x["starts"]] == want
            for x in got:
                assert x["lo"] == rows and x["lo"] <= x["final_hi"] <= x["limit"]
                hi = min(x["limit"], max(x["final_hi"], x["starts"][-1] + T if x["starts"] else 0))
                assert hi - x["lo"] <= W                                    # the rows of one launch fit the smallest ring
                assert not x["starts"] or max(x["starts"][0], 0) >= x["lo"]
                rows = x["final_hi"]
            assert rows == L
            with pytest.raises(RuntimeError):
                sc.push(1)
            with pytest.raises(RuntimeError):
                sc.close()


def test_close_refuses_what_predict_video_refuses():
    sc = LP.LiveSchedule(8, 6, 5, 2)
    with pytest.raises(ValueError, match="empty"):
        sc.close()
    with pytest.raises(ValueError):
        sc.push(0)
    sc = LP.LiveSchedule(8, 6, 0, 2)                             # pad_len = 0 and L <= overlap_len: no clips
    sc.push(6)
    assert E.video_clip_starts(6, 8, 6, pad_len=0) == []
    with pytest.raises(ValueError, match="no clips"):
        sc.close()
    assert not sc.closed
    sc.push(1)                                                   # the stream is still open, and 7 frames have a clip
    assert [x["starts"] for x in sc.close()] == [[0]]


def test_latency_bound_is_reached_and_never_exceeded():
    """Frame p is final once clip c = the first one that starts after p has been scored; with batches run only when full that
    is when clip ceil((c + 1) / bs) * bs - 1 is complete, at most T - 1 + (bs - 1) * s frames after p."""
    for (T, ov, pad), bs in itertools.product([(6, 4, 5), (6, 0, 0), (8, 6, 2), (1, 0, 0)], (1, 2, 4)):
        sc, tight = LP.LiveSchedule(T, ov, pad, bs), False
        bound = LP.latency_frames(bs, T, ov)
        assert bound == T - 1 + (bs - 1) * (T - ov)
        for _ in range(120):
            sc.push(1)
            assert sc.rows_final >= sc.pushed - bound             # frame pushed - 1 - bound and everything before it
            tight |= sc.rows_final == sc.pushed - bound
        assert tight


# ----------------------------------------------------------------------------- 3. the twin of the kernel
def _scores(n, V, T, K1, seed):
    rng = np.random.default_rng(seed)
    sc = rng.standard_normal((V, n, T, K1)).astype(np.float32) * np.float32(3)
    sc[rng.random((V, n, T)) < 0.25] = 0                          # rows that are all zero: not counted when count_all = 0
    sc[:, :, :, 0][rng.random((V, n, T)) < 0.1] = 0
    return sc


def _live_stitch(scores, L, T, ov, pad, bs, pattern, R, count_all):
    V, n, _, K1 = scores.shape
    ring_sum, ring_sup = np.zeros((R, K1), np.float32), np.zeros(R, np.int32)
    sc = LP.LiveSchedule(T, ov, pad, bs)
    parts = []

    def run(launches):
        for x in launches:
            B = len(x["starts"])
            batch = scores[:, x["first"]:x["first"] + B] if B else None
            parts.append(LP.live_stitch_ref(ring_sum, ring_sup, batch, x["starts"], count_all, x["lo"], x["final_hi"], x["limit"]))
    for m in pattern:
        run(sc.push(m))
    run(sc.close())
    assert sc.scored == n
    assert not ring_sum.any() and not ring_sup.any()             # every row was handed out and cleared
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


@pytest.mark.parametrize("T,ov,pad,bs", [(6, 4, 5, 1), (6, 3, 0, 3), (6, 0, 2, 2), (8, 6, 5, 4), (2, 1, 0, 1), (1, 0, 0, 3)])
@pytest.mark.parametrize("V,count_all", [(1, 0), (2, 1), (1, 1)])
def test_the_twin_equals_stitch_clip_scores_bit_for_bit(T, ov, pad, bs, V, count_all):
    rng = np.random.default_rng(T * 100 + ov * 10 + bs)
    R = LP.track_ring_rows(bs, T, ov)
    for L in (3, 7, 41):
        starts = E.video_clip_starts(L, T, ov, pad_len=pad)
        if not starts:
            continue                                             # (pad_len = 0 and L <= overlap_len: refused, see above)
        scores = _scores(len(starts), V, T, 4, L + V)
        assert scores.dtype == np.float32
        if V == 2:
            want_sum, want_sup = E.stitch_clip_scores(scores[0], starts, L, flip_scores=scores[1])
        elif count_all:
            want_sum, _ = E.stitch_clip_scores(scores[0], starts, L)
            want_sup = np.zeros(L, np.int32)
            for s in starts:
                want_sup[max(s, 0):max(min(s + T, L), 0)] += 1
        else:
            want_sum, want_sup = E.stitch_clip_scores(scores[0], starts, L)
        want_mean = want_sum / np.maximum(want_sup, 1)[:, None].astype(np.float32)
        for pattern in _patterns(L, rng):
            sums, sup, mean = _live_stitch(scores, L, T, ov, pad, bs, pattern, R, count_all)
            assert sums.dtype == np.float32 and sup.dtype == np.int32 and mean.dtype == np.float32
            assert sums.shape == (L, 4) and np.array_equal(sup, want_sup)
            assert np.array_equal(sums.view(np.uint32), want_sum.view(np.uint32))
            assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))
    if not count_all:
        # the support rule was exercised: some covered frame has an all-zero row that was not counted
        cover = np.zeros(L, np.int32)
        for s in starts:
            cover[max(s, 0):max(min(s + T, L), 0)] += 1
        assert (want_sup < cover).any()


# ----------------------------------------------------------------------------- 4. the ring minima
def test_one_row_fewer_breaks_the_twin_and_the_check_reports_it():
    T, ov, pad, bs, L = 6, 4, 5, 2, 41
    R = LP.track_ring_rows(bs, T, ov)
    assert R == 8 == T + (bs - 1) * (T - ov)
    starts = E.video_clip_starts(L, T, ov, pad_len=pad)
    scores = np.random.default_rng(3).standard_normal((1, len(starts), T, 4)).astype(np.float32) + np.float32(4)   # no zeros
    want_sum, want_sup = E.stitch_clip_scores(scores[0], starts, L)
    sums, sup, _ = _live_stitch(scores, L, T, ov, pad, bs, [1] * L, R, 0)
    assert np.array_equal(sums, want_sum) and np.array_equal(sup, want_sup)
    assert LP.check_track_ring(R, bs, T, ov) == R
    # one row fewer: the first and the last frame of a launch share a row, a sum that is not the frame's own is handed out
    bad_sum, bad_sup, _ = _live_stitch(scores, L, T, ov, pad, bs, [1] * L, R - 1, 0)
    assert not np.array_equal(bad_sum, want_sum) and not np.array_equal(bad_sup, want_sup)
    with pytest.raises(ValueError, match=f"at least {R} rows"):
        LP.check_track_ring(R - 1, bs, T, ov)


@pytest.mark.parametrize("T,ov,pad", [(6, 4, 5), (6, 0, 0), (8, 6, 2), (100, 75, 5)])
@pytest.mark.parametrize("bs", [1, 2, 8])
@pytest.mark.parametrize("chunk", [1, 3, 25])
def test_the_frame_ring_minimum_holds_a_batch_and_a_chunk(T, ov, pad, bs, chunk):
    """Fed in pieces of at most `chunk` frames, batches run as soon as they are complete: the frames some unscored clip still
    reads plus the piece being staged never exceed frame_ring_rows, and they come within a frame of it."""
    need = LP.frame_ring_rows(bs, chunk, T, ov)
    assert need == LP.track_ring_rows(bs, T, ov) + chunk
    sc, worst = LP.LiveSchedule(T, ov, pad, bs), 0
    for _ in range(20 * need // chunk):
        live = sc.pushed - sc.first_live_frame()
        assert live < LP.track_ring_rows(bs, T, ov)              # no batch is complete: less than a batch's span is live
        worst = max(worst, live + chunk)
        sc.push(chunk)
    assert need - chunk <= worst <= need
    assert LP.check_frame_ring(need, bs, chunk, T, ov) == need
    with pytest.raises(ValueError, match=f"at least ring_frames={need}"):
        LP.check_frame_ring(need - 1, bs, chunk, T, ov)
