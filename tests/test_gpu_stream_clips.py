"""Streamed JPEG sets on the MI355X: the relocating instance of the per-piece decode (ops.jpeg_entropy_items(..., reloc=...))
against the absolute one bit for bit, `trainclips.ResidentJpegClips(stream_clips=True)` and `evalutil.ResidentJpegVideos(
stream_videos=True)` at budgets below the set against the all-resident objects -- every field of every batch, every frame
of every video, a training epoch's loss and parameters, the APs of a validation pass.  -m gpu only.

On the 18-frame tree of test_gpu_resident_jpeg a batch's staging (3 ring entries of 3 or 6 clip ranges) is larger than the
whole set's streams, so the smallest streamed budget lies ABOVE the all-resident size there: the loaders are held to
`stream_plan`'s budgets (everything streamed at `needs[0]`, the first video resident at `needs[1]`), and today's error
without the keyword is checked one byte below the all-resident size."""
import numpy as np
import pytest
import torch

import jpeg_cases as J
from tdeed_amd import evalutil as E
from tdeed_amd import jpegdev, ops
from tdeed_amd import trainclips as TC
import test_gpu_resident_jpeg as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- 1. the kernel
def _pack():
    pk = jpegdev.pack_frames([J.data(n) for n in R.ENC])
    dj, stream, waves = R._resident(pk)
    pieces, status, off = R._index(pk, 2, dj, stream, waves)
    rows = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1).copy()
    assert not status.cpu().numpy().any()
    return pk, dj, stream, pieces, rows


def _decode(pk, dj, buf, pieces, rows, perm, reloc, keep=None):
    """every piece (of `keep`) into the slot perm[frame] through the relocation rows; -> (coefficients per slot, error word)"""
    fc = ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp)
    order = np.argsort(rows["set"], kind="stable")
    if keep is not None:
        order = order[np.isin(order, keep)]
    items = np.stack([order, perm[pk.segments[rows["segment"][order], 0]]], 1).astype(np.int32)
    wv = TC._cut_waves(rows["set"][order])
    coeff = torch.zeros(pk.n_frames * fc, dtype=torch.int16, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.jpeg_entropy_items(buf, pieces, torch.from_numpy(items).to(DEV), torch.from_numpy(wv).to(DEV), dj.table_sets,
                           pk.width, pk.height, pk.samp, 0, pk.n_frames, coeff, err,
                           reloc=None if reloc is None else torch.from_numpy(np.asarray(reloc, np.int64)).to(DEV))
    torch.cuda.synchronize()
    return coeff.view(pk.n_frames, fc), int(err.item())


def test_pieces_decode_from_a_shifted_copy_and_from_two_ranges():
    pk, dj, stream, pieces, rows = _pack()
    n = stream.numel()
    perm = np.array([2, 0, 3, 1])
    want, word = _decode(pk, dj, stream, pieces, rows, perm, None)
    assert word == 0 and all(want[s].any() for s in range(4))
    # delta 0 and the whole buffer as the window: the absolute entry
    got, word = _decode(pk, dj, stream, pieces, rows, perm, [[0, 0, n]] * 4)
    assert word == 0 and torch.equal(got, want)
    # the stream 4096 + 48 bytes into a buffer of 0xFF: the positions stay, every slot's delta moves them
    for shift in (48, 4096 + 48):
        buf = torch.full((shift + n + 32,), 0xFF, dtype=torch.uint8, device=DEV)
        buf[shift:shift + n].copy_(stream)
        got, word = _decode(pk, dj, buf, pieces, rows, perm, [[-shift, shift, shift + n]] * 4)
        assert word == 0 and torch.equal(got, want), shift
    # two ranges, cut at a frame boundary of the segment rows (rows lie in byte order), the second one staged in FRONT of
    # the first, each from a multiple of 16: per slot the delta and window of the range that holds its frame
    seg = pk.segments
    cut = next(i for i in range(len(seg) // 2, len(seg)) if seg[i, 0] != seg[i - 1, 0])
    lo_b = int(seg[cut, 3]) & ~15
    hi_a, hi_b = int((seg[:cut, 3] + seg[:cut, 4]).max()), int((seg[cut:, 3] + seg[cut:, 4]).max())
    at_b, at_a = 32, 32 + ((hi_b - lo_b + 15) & ~15) + 160
    buf = torch.full((at_a + hi_a + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[at_b:at_b + hi_b - lo_b].copy_(stream[lo_b:hi_b])
    buf[at_a:at_a + hi_a].copy_(stream[:hi_a])
    reloc = np.zeros((4, 3), np.int64)
    for f in range(4):
        in_a = f in seg[:cut, 0]
        assert in_a != (f in seg[cut:, 0])
        reloc[perm[f]] = (0 - at_a, at_a, at_a + hi_a) if in_a else (lo_b - at_b, at_b, at_b + hi_b - lo_b)
    assert not np.any(reloc[:, 0] % 16)
    got, word = _decode(pk, dj, buf, pieces, rows, perm, reloc)
    assert word == 0 and torch.equal(got, want)


def test_pieces_that_leave_their_window_count_as_errors_and_touch_nothing():
    pk, dj, stream, pieces, rows = _pack()
    n = stream.numel()
    perm = np.arange(4)
    frame = pk.segments[rows["segment"], 0]
    k = int(np.flatnonzero((rows["left"] > 8) & (rows["pos"] > 64) & (frame >= 1))[0])          # a piece in the middle of the stream
    f = int(frame[k])
    pos, left = int(rows["pos"][k]), int(rows["left"][k])

    def run(row, n_rows=4):
        reloc = np.asarray([[0, 0, n]] * n_rows, np.int64)
        reloc[min(f, n_rows - 1)] = row
        return _decode(pk, dj, stream, pieces, rows, perm, reloc, keep=[k])
    good, word = run([0, pos, pos + left])                                     # the tightest window
    assert word == 0 and good[f].any()
    for row in ([0, pos + 1, n], [0, 0, pos + left - 1], [0, pos, pos + left - 1],            # starts before / ends behind the window
                [pos + 16, 0, n], [1 << 40, 0, n], [-n, 0, n], [-(1 << 40), 0, n],           # before / behind the buffer
                [0, 0, n + 16], [0, -16, n], [0, pos + left, pos], [16, 0, n + 16]):         # a window that leaves the buffer
        coeff, word = run(row)
        assert word == 1 << 7 and not coeff.any(), row
    coeff, word = run([0, 0, n], n_rows=f)                                      # no relocation row for the slot
    assert word == 1 << 7 and not coeff.any()
    # a piece that is refused leaves the others alone
    other = int(np.flatnonzero(frame != f)[0])
    reloc = np.asarray([[0, 0, n]] * 4, np.int64)
    reloc[f] = [0, 0, pos]
    coeff, word = _decode(pk, dj, stream, pieces, rows, perm, reloc, keep=[k, other])
    assert word == 1 << 7 and coeff[int(frame[other])].any() and not coeff[f].any()
    with pytest.raises(TypeError, match="reloc"):
        ops.jpeg_entropy_items(stream, pieces, torch.zeros((1, 2), dtype=torch.int32, device=DEV),
                               torch.tensor([[0, 1]], dtype=torch.int32, device=DEV), dj.table_sets, pk.width, pk.height, pk.samp,
                               0, 4, torch.zeros(4 * ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp), dtype=torch.int16, device=DEV),
                               torch.zeros(1, dtype=torch.int32, device=DEV), reloc=torch.zeros((4, 3), dtype=torch.int32, device=DEV))


# ----------------------------------------------------------------------------- 2. the loader against the all-resident one
def _pair(root, videos, resident, load_kw=None, **kw):
    """(all-resident loader, streamed loader at the budget that keeps `resident` videos, that budget)"""
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, **(load_kw or {}))
    ref = TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, **kw)
    probe = TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, stream_clips=True, **kw)       # ample: the plan's numbers
    assert probe.stats["resident_videos"] == len(videos) and probe.stats["stage_bytes"] == 0
    assert probe.stats["resident_bytes"] == ref.stats["resident_bytes"]
    budget = int(probe._plan.needs[resident])
    got = TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, stream_clips=True, max_resident_bytes=budget, **kw)
    return ref, got, budget


@pytest.mark.parametrize("resident", [0, 1], ids=["all_streamed", "first_resident"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mixup", [False, True], ids=["plain", "mixup"])
def test_streamed_clips_equal_the_all_resident_loader_over_two_passes(tmp_path, mixup, stride, resident):
    """shards of 1024 bytes: nine of them, clips straddling up to four; CMYK / progressive / grey / 4:4:4 files in the side
    buffer.  Budget: `stream_plan`'s minimum (everything streamed), or that plus the first video's streams."""
    videos = R._tree(str(tmp_path))
    kw = dict(clip_len=6, stride=stride, overlap=1, mixup=mixup, radi_displacement=2, dataset_len=7, batch_size=3, seed=21)
    ref, got, budget = _pair(str(tmp_path), videos, resident, load_kw=dict(shard_bytes=1024), **kw)
    assert "resident_videos" not in ref.stats
    st = got.stats
    assert st["shards"] >= 2 and (st["resident_videos"], st["streamed_videos"]) == (resident, 2 - resident)
    assert st["resident_bytes"] <= budget and st["stage_bytes"] == 3 * got._plan.region_bytes > 0
    assert st["host_stream_bytes"] == st["stream_bytes"] - got._plan.stream_bytes > 0
    assert got.jstream.numel() == max(got._plan.buffer_bytes, 16)
    got.stage_log = []
    assert R._compare(ref, got) == 6
    assert len(got.stage_log) == 6 and max(got.stage_log) > 0 and max(got.stage_log) <= got._plan.region_bytes
    assert (st["device_frames"], st["fallback_frames"]) == (14, 4)


def test_streamed_clips_from_one_shard_and_in_coefficient_chunks(tmp_path):
    """the whole set in one shard, indexed through the staging memory; the batch decoded in chunks of five slots"""
    videos = R._tree(str(tmp_path))
    kw = dict(clip_len=6, stride=1, overlap=1, mixup=True, radi_displacement=0, dataset_len=7, batch_size=3, seed=5,
              max_coeff_bytes=5 * 2 * ops.jpeg_frame_coeffs(32, 24, 3))
    ref, got, budget = _pair(str(tmp_path), videos, 0, **kw)
    assert got.stats["shards"] == 1 and got._chunk == 5 and got.stats["streamed_videos"] == 2
    assert R._compare(ref, got) == 6


def test_streamed_clips_from_pageable_shards(tmp_path):
    """`load_resident_jpegs(pinned=False)`: the range copies block the host instead of running behind it; same batches"""
    videos = R._tree(str(tmp_path))
    kw = dict(clip_len=6, stride=2, overlap=1, mixup=False, radi_displacement=2, dataset_len=7, batch_size=3, seed=8)
    ref, got, budget = _pair(str(tmp_path), videos, 1, load_kw=dict(shard_bytes=1024, pinned=False), **kw)
    assert got._host_streams and not any(h.is_pinned() for h in got._host_streams)
    assert got.stats["streamed_videos"] == 1 and R._compare(ref, got) == 6


def test_budget_boundaries(tmp_path, monkeypatch):
    root = str(tmp_path)
    videos = R._tree(root, other={})
    kw = dict(clip_len=6, stride=1, overlap=1, mixup=False, radi_displacement=2, dataset_len=7, batch_size=3, seed=4)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, shard_bytes=1024)
    free = TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, stream_clips=True, **kw)
    low, compressed = free._plan.min_budget, free.stats["resident_bytes"]
    one = TC.load_resident_jpegs(root, "soccernetball", videos)
    kw1 = dict(kw, clip_len=1, batch_size=1, depth=1, pad_len=0)
    low1 = TC.ResidentJpegClips(videos, one, R.CLASSES, device=DEV, stream_clips=True, **kw1)._plan.min_budget
    from tdeed_amd import streams

    def no_upload(*a, **k):
        raise AssertionError("uploaded before the check")
    monkeypatch.setattr(streams, "new_stream", no_upload)
    with pytest.raises(ValueError, match=f"smallest max_resident_bytes that would do is {low}$"):
        TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, stream_clips=True, max_resident_bytes=low - 1, **kw)
    with pytest.raises(AssertionError, match="uploaded before"):
        TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, stream_clips=True, max_resident_bytes=low, **kw)
    # without the keyword nothing changes: a budget below the all-resident size raises today's error, whatever it would stream
    for budget in (compressed - 1, min(low - 1, compressed - 1)):
        with pytest.raises(ValueError, match=r"ResidentJpegClips: the set needs \d+ bytes on the device \(\d+ of entropy streams, 0 "
                                             r"frames kept decoded\), more than max_resident_bytes="):
            TC.ResidentJpegClips(videos, jpegs, R.CLASSES, device=DEV, max_resident_bytes=budget, **kw)
    # a streamed shard larger than the staging memory: the caller is told to cut smaller shards
    with pytest.raises(ValueError, match="smaller shard_bytes"):
        TC.ResidentJpegClips(videos, one, R.CLASSES, device=DEV, stream_clips=True, max_resident_bytes=low1, **kw1)


# ----------------------------------------------------------------------------- 3. epoch()
def test_training_epoch_fed_by_streamed_clips_equals_the_all_resident_fed_epoch(tmp_path):
    """Mixup, the tiny 200MF model, 64 x 64 4:2:0 frames, every video streamed: the batches are the same bits, so are the loss
    and every parameter."""
    meta, _ = R.load_golden("tiny_rny002_gsf")
    cfg = meta["cfg"]
    root = str(tmp_path)
    videos = R._write_videos(root, meta["H"], meta["W"])
    kw = dict(clip_len=cfg["clip_len"], stride=1, overlap=1, mixup=True, dataset_len=4, batch_size=2, seed=31,
              radi_displacement=cfg["radi_displacement"], device=DEV)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, shard_bytes=48 << 10)
    made = {}

    def res():
        return TC.ResidentJpegClips(videos, jpegs, R.CLASSES, **kw)

    def streamed():
        low = TC.ResidentJpegClips(videos, jpegs, R.CLASSES, stream_clips=True, **kw)._plan.min_budget
        made["l"] = TC.ResidentJpegClips(videos, jpegs, R.CLASSES, stream_clips=True, max_resident_bytes=low, **kw)
        return made["l"]
    l_res, p_res = R._train_once(res)
    l_str, p_str = R._train_once(streamed)
    print(f"loss all-resident-fed {l_res!r}, streamed-fed {l_str!r}")
    st = made["l"].stats
    assert (st["resident_videos"], st["streamed_videos"], st["fallback_frames"]) == (0, 3, 0) and st["shards"] >= 2
    assert np.isfinite(l_res) and l_str == l_res
    assert all(torch.equal(p_str[k], p_res[k]) for k in p_res)


# ----------------------------------------------------------------------------- 4. validation videos
def test_streamed_videos_equal_the_all_resident_object_and_score_the_same_aps(tmp_path):
    """videos of 20, 37 and 9 frames, the first one resident; coefficient chunks of 8 frames, which are the staging region's
    size too: the two streamed videos are staged in 5 and 2 chunks"""
    import test_gpu_resident_video as RV
    root = str(tmp_path)
    videos = RV._videos_with_fps(R._write_videos(root, 64, 64))
    truth = [{"video": v["video"], "events": [{"label": "c1", "frame": 3}, {"label": "c2", "frame": 5}, {"label": "c3", "frame": 7},
                                              {"label": "c1", "frame": v["num_frames"] - 1}]} for v in videos]
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, shard_bytes=8 << 10)
    fc = ops.jpeg_frame_coeffs(64, 64, jpegs.samp)
    m = RV._model(RV.TINY)
    for crop in (None, 48):
        kw = dict(crop=crop, max_coeff_bytes=8 * 2 * fc, device=DEV)
        ref = E.ResidentJpegVideos(videos, jpegs, **kw)
        probe = E.ResidentJpegVideos(videos, jpegs, stream_videos=True, **kw)
        assert probe.stats["resident_videos"] == 3 and probe.stats["resident_bytes"] == ref.stats["resident_bytes"]
        budget = int(probe._plan.needs[1])
        rv = E.ResidentJpegVideos(videos, jpegs, stream_videos=True, max_resident_bytes=budget, **kw)
        st = rv.stats
        assert (st["resident_videos"], st["streamed_videos"]) == (1, 2) and st["resident_bytes"] <= budget < ref.stats["resident_bytes"]
        assert rv._chunk == 8 and st["stage_bytes"] == rv._plan.region_bytes and "stage_bytes" not in ref.stats
        # the longest video's streams do not fit the region: it is staged chunk by chunk
        first, n = rv.video_first[1], rv.video_len[1]
        assert int((rv._rs.ext.hi[first:first + n] - rv._rs.ext.lo[first:first + n]).sum()) > rv._plan.region_bytes
        for _ in range(2):
            for i in range(3):
                assert torch.equal(rv.frames(i), ref.frames(i)), (crop, i)
        assert len(rv._tabs[1][5]) == 5 and len(rv._tabs[2][5]) == 2 and all(rv._tabs[1][5].values()) and not any(rv._tabs[0][5].values())
        if crop is None:
            got = E.map_videos(m, rv.sources(), RV.CLASSES, truth, RV.SUPPRESS, [0, 1, 2], **RV.KW)
            want = E.map_videos(m, ref.sources(), RV.CLASSES, truth, RV.SUPPRESS, [0, 1, 2], **RV.KW)
            assert got == want and max(got[0][0]) > 0                     # mAP and AP floats, bit for bit
    with pytest.raises(ValueError, match="smallest max_resident_bytes that would do"):
        E.ResidentJpegVideos(videos, jpegs, stream_videos=True, max_resident_bytes=int(probe._plan.min_budget) - 1, **kw)
