"""Event spotting on the MI355X: `ops.frame_events` against numpy, `ops.nms_track` bit for bit against the host chain
(`frame_events` -> `non_maximum_suppression` / `soft_non_maximum_suppression`) on every case of tests/test_spot_host.py and
on larger tracks, `TDEEDModel.spot_video` / `evalutil.spot_videos` against `predict_video` + the host chain.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import model_state, t, cfg_ns, load_golden
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth
import test_spot_host as H

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- frame events
@pytest.mark.parametrize("K1", [2, 5, 18])
@pytest.mark.parametrize("L", [1, 37, 257, 1025])
def test_frame_events_equals_numpy(L, K1):
    for variant, hr in (("uniform", 0.01), ("sixths", 0.2), ("zero_rows", 0.0), ("sharp", 0.3)):
        mean = H.make_track(L, K1, variant, 7 * L + K1)
        pred8 = torch.full((L,), 255, dtype=torch.uint8, device=DEV)
        pred, score, first, count = ops.frame_events(torch.from_numpy(mean).to(DEV), hr, pred_u8=pred8)
        torch.cuda.synchronize()
        want = mean.argmax(axis=1)
        assert np.array_equal(pred8.cpu().numpy(), want.astype(np.uint8))       # the one-byte form spot_video copies
        assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), want), (variant, hr)
        assert np.array_equal(score.cpu().numpy(), mean[np.arange(L), want])
        cand = mean >= hr                                             # numpy: fp32 array against a python float
        cand[:, 0] = False
        assert np.array_equal(count.cpu().numpy(), cand.sum(axis=0)), (variant, hr)
        assert np.array_equal(first.cpu().numpy(), np.where(cand.any(axis=0), cand.argmax(axis=0), L)), (variant, hr)


# ----------------------------------------------------------------------------- suppression
def _device_route(mean, window, thr, soft, hr, first_frame=None):
    d = torch.from_numpy(mean).to(DEV)
    c8 = torch.full((d.shape[0] * (d.shape[1] - 1),), 255, dtype=torch.uint8, device=DEV)
    frames, classes, scores, count, rounds = ops.nms_track(d, window, thr, soft, hr, first_frame=first_frame, classes_u8=c8)
    torch.cuda.synchronize()
    n = int(count.cpu()[0])
    assert torch.equal(c8[:n].to(torch.int32), classes[:n])                     # the one-byte form spot_video copies
    assert 0 <= n <= frames.numel() and scores.dtype == torch.float64
    return frames[:n].cpu().numpy(), classes[:n].cpu().numpy(), scores[:n].cpu().numpy(), rounds.cpu().numpy()


def _check_case(mean, window, thr, soft, hr, tag):
    want = H.host_chain(mean, window, thr, soft, hr)
    got = _device_route(mean, window, thr, soft, hr)
    H.check_equal(got, want, tag)
    again = _device_route(mean, window, thr, soft, hr)
    for a, b in zip(got, again):
        assert np.array_equal(a, b), tag
    n_cand = (mean[:, 1:] >= np.float32(hr)).sum(axis=0)
    assert (got[3][1:] <= n_cand).all() and got[3][0] == 0, (tag, got[3], n_cand)
    return len(want[0]), got[3]


@pytest.mark.parametrize("variant", H.VARIANTS)
@pytest.mark.parametrize("K1", H.COLS)
@pytest.mark.parametrize("L", H.LENGTHS)
def test_nms_track_equals_the_host_chain(L, K1, variant):
    n_events = 0
    for mean, window, thr, soft, hr in H.grid_cases(L, K1, variant):
        n_events += _check_case(mean, window, thr, soft, hr, (window, thr, soft, hr))[0]
    assert n_events > 0


@pytest.mark.parametrize("name", sorted(H.boundary_cases()))
def test_nms_track_boundaries(name):
    mean, window, thr, soft, hr, frames1 = H.boundary_cases()[name]
    _, rounds = _check_case(mean, window, thr, soft, hr, name)
    got = _device_route(mean, window, thr, soft, hr)
    if frames1 is not None:
        assert got[0][got[1] == 1].tolist() == frames1
    assert np.array_equal(rounds, E.nms_rounds(mean, window, thr, soft, hr)[3])
    if name.startswith("ramp"):
        assert rounds[1] >= 100


@pytest.mark.parametrize("variant", ["sixths", "sharp"])
@pytest.mark.parametrize("L", [257, 1025])
def test_nms_track_many_classes(L, variant):
    """K1 = 18, more frames than a workgroup has threads (1025), a list window of 17 entries"""
    mean = H.make_track(L, 18, variant, L + 3)
    n = 0
    for window in (3, H.windows_for(18)[3]):
        for soft in (False, True):
            n += _check_case(mean, window, 0.05, soft, 0.01, (L, variant, window, soft))[0]
    assert n > 0


def test_nms_track_dense_long_track():
    """one class, every one of 20 000 frames a candidate (hr_threshold 0): beyond the LDS-resident state of the kernel"""
    L = 20000
    ws_bytes = ops._lib.load().tdeed_nms_track_seg_workspace
    assert ws_bytes(L, L, 2) > 0 and ws_bytes(1025, 1025, 18) == 0
    mean = np.zeros((L, 2), np.float32)
    mean[:, 1] = np.random.RandomState(11).rand(L).astype(np.float32)
    mean[::7, 1] = np.float32(0.5)                                    # ties across the whole track
    n_hard, _ = _check_case(mean, 5, 0.0, False, 0.0, "dense hard")
    n_soft, _ = _check_case(mean, 5, 0.3, True, 0.0, "dense soft")
    assert n_hard > L // 11 and n_soft > 0


def test_nms_track_single_video_workgroup_sizes():
    """A single video gets the workgroup size its length selects (128 / 256 / 512 / 1024 threads): both sides of every
    threshold above the 128-thread form that the grid's lengths stay in."""
    threads = ops._lib.load().tdeed_nms_track_seg_threads
    assert [threads(L) for L in (128, 129, 256, 257, 512, 513)] == [128, 256, 256, 512, 512, 1024]
    n = 0
    for L in (128, 129, 256, 257, 512, 513):
        mean = H.make_track(L, 5, "sharp", 3 * L + 1)
        for soft in (False, True):
            got = _device_route(mean, 2, 0.02, soft, 0.01)
            H.check_equal(got, H.host_chain(mean, 2, 0.02, soft, 0.01), (L, soft))
            n += len(got[0])
    assert n > 0


def test_nms_track_golden_inputs():
    meta, g = load_golden("eval_utils")
    videos, _, norm, _ = H.golden_inputs(meta)
    n = 0
    for tag, (window, thr, soft) in H.GOLDEN_NMS.items():
        for v, _, _ in videos:
            frames, classes, scores, _ = _device_route(np.ascontiguousarray(norm[v]), window, thr, soft, meta["hr_thr"])
            H.check_golden(g, tag, v, frames, classes, scores)
            n += len(frames)
    assert n > 0


def test_spot_argument_checks():
    mean = torch.rand((9, 4), device=DEV)
    with pytest.raises(ValueError):
        ops.nms_track(mean, 0, 0.01, True, 0.01)                      # soft needs a window >= 1
    with pytest.raises(ValueError):
        ops.nms_track(mean, [1, 2, 0], 0.01, True, 0.01)
    with pytest.raises(ValueError):
        ops.nms_track(mean, [1, 2], 0.01, False, 0.01)                # 3 classes, 2 windows
    with pytest.raises(TypeError):
        ops.nms_track(mean.double(), 1, 0.01, False, 0.01)
    with pytest.raises(TypeError):
        ops.frame_events(mean.to(torch.bfloat16), 0.01)
    with pytest.raises(ValueError):
        ops.frame_events(mean.t(), 0.01)                              # not contiguous
    with pytest.raises(ValueError):
        ops.frame_events(torch.rand((3, 300), device=DEV), 0.01, pred_u8=torch.empty((3,), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.nms_track(mean, 1, 0.01, False, 0.01, classes_u8=torch.empty((5,), dtype=torch.uint8, device=DEV))
    assert int(ops.nms_track(mean, 0, 0.0, False, 0.0)[3].cpu()[0]) == 27      # hard, w = 0: every candidate is kept


# ----------------------------------------------------------------------------- end to end, tiny model
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)
CLASSES = {"c1": 1, "c2": 2, "c3": 3}


def _model(cfg, seed=0):
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m.load({k: t(v) for k, v in model_state(cfg, seed).items()})
    return m


@pytest.fixture(scope="module")
def tiny_model():
    return _model(TINY)


@pytest.fixture(scope="module")
def tiny_video():
    return t(synth.uint8_clip(4100, (37, 3, 64, 64)))


def _host_route(m, video, classes, suppress, hr=0.01, fps=25.0, **kw):
    """predict_video -> ScoreStitcher.normalised -> the host chain; -> (pred, arg-max events, [suppressed records], stats)"""
    sums, sup = m.predict_video(video, **kw)
    stats = dict(m.last_video_stats)
    st = E.ScoreStitcher([("v", video.shape[0], fps)], sums.shape[1])
    st.tracks["v"][0][...] = sums
    st.tracks["v"][1][...] = sup
    norm = st.normalised()
    pe, recall, _ = E.frame_events(norm, classes, st.fps, high_recall_score_threshold=hr)
    out = [(E.soft_non_maximum_suppression if kind == "snms" else E.non_maximum_suppression)(recall, w, thr)[0]
           for kind, w, thr in suppress]
    return norm["v"].argmax(axis=1), pe[0]["events"], out, stats


@pytest.mark.parametrize("windows", [(1, 3), ([2, 1, 3], [3, 1, 2])], ids=["scalar", "list"])
@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
def test_spot_video_equals_predict_video_and_the_host_chain(tiny_model, tiny_video, use_amp, augment, windows):
    m = tiny_model
    suppress = (("nms", windows[0], 0.01), ("snms", windows[1], 0.01))
    kw = dict(batch_size=4, augment=augment, use_amp=use_amp)
    pred, events, sup_lists, stats0 = _host_route(m, tiny_video, CLASSES, suppress, **kw)
    r = m.spot_video(tiny_video, CLASSES, suppress=suppress, **kw)
    stats = dict(m.last_video_stats)
    assert r["pred"].dtype == np.int32 and np.array_equal(r["pred"], pred)
    assert r["events"] == events
    assert len(r["suppressed"]) == 2
    for got, want in zip(r["suppressed"], sup_lists):
        assert got == want["events"] and len(got) == want["num_events"]
    assert sum(len(x) for x in r["suppressed"]) > 0
    for k in ("frames", "clips", "batches", "views", "frames_h2d_bytes"):
        assert stats[k] == stats0[k], k
    assert stats0["frames"] == 37 and stats0["clips"] == 18 and stats0["views"] == (2 if augment else 1)
    assert stats["events_d2h_bytes"] == 37 * 5 + 2 * 5 * 4 + 13 * sum(len(x) for x in r["suppressed"])
    assert len(stats["nms_rounds"]) == 2 and all(1 <= x <= 37 for x in stats["nms_rounds"])


def test_spot_videos_equals_stitch_videos_and_the_host_chain(tiny_model, tiny_video):
    m = tiny_model
    second = t(synth.uint8_clip(4200, (23, 3, 64, 64)))
    vids = [("b", 37, 25.0, tiny_video), ("a", 23, 30.0, lambda: second)]
    suppress = (("nms", 1, 0.01), ("snms", [3, 1, 2], 0.01))
    st = E.stitch_videos(m, vids, 4, augment=True, batch_size=4)
    pe, recall, _ = E.frame_events(st.normalised(), CLASSES, st.fps, high_recall_score_threshold=0.01)
    nms = E.non_maximum_suppression(recall, 1, 0.01)
    snms = E.soft_non_maximum_suppression(recall, [3, 1, 2], 0.01)
    got_pe, got_lists, preds = E.spot_videos(m, vids, CLASSES, suppress, augment=True, batch_size=4)
    assert [x["video"] for x in got_pe] == ["a", "b"]
    assert got_pe == pe and got_lists[0] == nms and got_lists[1] == snms
    norm = st.normalised()
    assert sorted(preds) == ["a", "b"] and all(np.array_equal(preds[v], norm[v].argmax(axis=1)) for v in preds)
    truth = [{"video": v, "events": [{"label": "c1", "frame": 3}, {"label": "c2", "frame": 10}, {"label": "c3", "frame": 17}]}
             for v in ("a", "b")]
    for lst, ref in zip(got_lists, (nms, snms)):
        assert E.mean_average_precisions(truth, lst, [1, 2])[0] == E.mean_average_precisions(truth, ref, [1, 2])[0]


# ----------------------------------------------------------------------------- end to end, full size
CFG2 = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4, num_classes=4,
            radi_displacement=2)


@pytest.fixture(scope="module")
def full_size_run():
    """224 x 224, clip length 100, 430 frames, augmented, batch size 8 (the full-size case of tests/test_gpu_video.py), spotted
    the way the reference's `evaluate` calls the two suppressions (util/eval.py:386-391) with WINDOWS['soccernetball']."""
    m = _model(CFG2, seed=5)
    L = 430
    video = ops.fill_u8_hash((L, 3, 224, 224), 77, DEV).cpu()
    classes = {f"c{k}": k for k in range(1, 5)}
    w0, w1 = E.WINDOWS["soccernetball"]
    suppress = (("nms", w0, 0.01), ("snms", w1, 0.01))
    kw = dict(batch_size=8, augment=True)
    host = _host_route(m, video, classes, suppress, **kw)
    r = m.spot_video(video, classes, suppress=suppress, **kw)
    return L, w0, host, r, dict(m.last_video_stats)


def test_spot_video_full_size_equals_the_host_chain(full_size_run):
    L, w0, (pred, events, sup_lists, stats0), r, stats = full_size_run
    assert np.array_equal(r["pred"], pred) and r["events"] == events
    for got, want in zip(r["suppressed"], sup_lists):
        assert got == want["events"] and len(got) == want["num_events"]
    assert 0 < len(r["suppressed"][0]) <= 4 * -(-L // (w0 + 1))       # hard: kept events of a class are more than w0 apart
    for k in ("frames", "clips", "batches", "views", "frames_h2d_bytes"):
        assert stats[k] == stats0[k], k
    assert stats["clips"] == 15 and stats["batches"] == 2 and stats["views"] == 2


def test_spot_video_full_size_moves_less_than_the_track(full_size_run):
    """events_d2h_bytes against the L * K1 * 4 bytes of the track.  What comes back is 5 bytes per frame (pred as one byte,
    its score as fp32), counts and rounds, and 13 bytes per kept event (frame int32, class one byte, score float64).  The
    untrained model's track is flat (every class near 1 / K1 on every frame), so suppression keeps about one event per 9
    frames and class, where a trained model's peaky track has a handful per class."""
    L, _, _, r, stats = full_size_run
    print(f"events_d2h_bytes {stats['events_d2h_bytes']} track bytes {L * 5 * 4} events {[len(x) for x in r['suppressed']]} "
          f"rounds {stats['nms_rounds']}")
    assert stats["events_d2h_bytes"] == L * 5 + 2 * 6 * 4 + 13 * sum(len(x) for x in r["suppressed"])
    assert stats["events_d2h_bytes"] < L * 5 * 4, (stats["events_d2h_bytes"], L * 5 * 4)
