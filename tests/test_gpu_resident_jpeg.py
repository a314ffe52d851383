"""Resident JPEG streams on the MI355X: the index pass and the per-piece decode (ops.jpeg_entropy_index / jpeg_entropy_items)
against ops.jpeg_entropy bit for bit, `trainclips.ResidentJpegClips` against `trainclips.ResidentClips` fed Pillow-decoded
frames of the same tree -- every field of every batch over two passes -- and `TDEEDModel.epoch()` fed by either.
-m gpu only."""
import itertools
import os
import random
import shutil

import numpy as np
import pytest
import torch

import jpeg_cases as J
from helpers import cfg_ns, load_golden
from tdeed_amd import feeder, jpegdev, ops
from tdeed_amd import trainclips as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENC = ["24x32_420_q90.jpg", "24x32_420_q100.jpg", "24x32_420_q30opt.jpg", "24x32_420_q75rst3.jpg"]
SIZES = [(24, 32), (23, 37), (17, 49), (40, 56), (8, 8), (1, 1)]
GROUPS = [f"{h}x{w}_{s}" for h, w in SIZES for s in J.SAMPLINGS] + ["24x32_grey"]


# ----------------------------------------------------------------------------- 1. the kernels
def _resident(pk, base=0, tail=0, fill=False):
    """the pack's stream `base` bytes into a resident buffer, and its tables on the device"""
    dj = feeder.DeviceJpegs(pk, torch.device(DEV), pk.n_frames)
    n = pk.stream_np.size
    stream = torch.empty(base + n + tail, dtype=torch.uint8, device=DEV)
    if fill:
        stream.fill_(0xFF)
    stream[base:base + n].copy_(torch.from_numpy(pk.stream_np))
    (_, _, waves), = dj.chunks
    return dj, stream, waves


def _index(pk, split, dj, stream, waves, base=0, seg_base=0):
    cnt = jpegdev.piece_counts(pk.segments, split)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    pieces = torch.zeros((int(off[-1]), jpegdev.PIECE_BYTES), dtype=torch.uint8, device=DEV)
    status = torch.full((pk.n_segments,), -1, dtype=torch.int32, device=DEV)
    ops.jpeg_entropy_index(stream, base, dj.segments, waves, dj.table_sets, pk.width, pk.height, pk.samp, split,
                           torch.from_numpy(off).to(DEV), seg_base, pieces, status)
    return pieces, status, off


def _items_decode(pk, dj, stream, pieces, rows, perm):
    """every piece into the slot perm[frame]; -> (coefficients per slot, error word)"""
    fc = ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp)
    order = np.argsort(rows["set"], kind="stable")
    items = np.stack([order, perm[pk.segments[rows["segment"][order], 0]]], 1).astype(np.int32)
    wv = TC._cut_waves(rows["set"][order])
    coeff = torch.zeros(pk.n_frames * fc, dtype=torch.int16, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.jpeg_entropy_items(stream, pieces, torch.from_numpy(items).to(DEV), torch.from_numpy(wv).to(DEV), dj.table_sets,
                           pk.width, pk.height, pk.samp, 0, pk.n_frames, coeff, err)
    return coeff.view(pk.n_frames, fc), err


def _whole(pk, dj, waves):
    fc = ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp)
    coeff = torch.zeros(pk.n_frames * fc, dtype=torch.int16, device=DEV)
    dj.stream_through(pk.stream_np.size)
    ops.jpeg_entropy(dj.stream, dj.segments, waves, dj.table_sets, pk.width, pk.height, pk.samp, 0, pk.n_frames, coeff, dj.status)
    return coeff.view(pk.n_frames, fc)


@pytest.mark.parametrize("row_split", [False, True], ids=["per_mcu", "per_row"])
@pytest.mark.parametrize("gid", GROUPS)
def test_pieces_decode_to_the_whole_segment_coefficients(gid, row_split):
    names = J.groups()[gid]
    pk = jpegdev.pack_frames([J.data(n) for n in names])
    assert pk.fallback == []
    split = pk.geom.mcus_x if row_split else 1
    base = 0 if row_split else 48                                          # the shard's offsets count from a base
    dj, stream, waves = _resident(pk, base=base, tail=16, fill=True)
    pieces, status, off = _index(pk, split, dj, stream, waves, base=base, seg_base=5)
    want = _whole(pk, dj, waves)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any() and not dj.status.cpu().numpy()[:pk.n_segments].any()
    rows = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1)
    assert rows.size == off[-1] == sum(len(jpegdev.split_points(m0, nm, split)) + 1 for m0, nm in pk.segments[:, 1:3].tolist())
    assert rows["first_mcu"].tolist() == [m for m0, nm in pk.segments[:, 1:3].tolist()
                                          for m in [m0] + jpegdev.split_points(m0, nm, split)]
    assert rows["segment"].tolist() == [5 + i for i, c in enumerate(np.diff(off)) for _ in range(c)]
    rows = rows.copy()
    rows["segment"] -= 5
    seg = pk.segments[rows["segment"]]
    assert np.all(rows["pos"] == base + seg[:, 3] + rows["st"]["byte_off"]) and np.all(rows["set"] == seg[:, 5])
    assert np.all(rows["left"] == seg[:, 4] - rows["st"]["byte_off"])
    perm = np.random.RandomState(len(gid)).permutation(pk.n_frames)
    got, err = _items_decode(pk, dj, stream, pieces, rows, perm)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for f, n in enumerate(names):
        assert torch.equal(got[perm[f]], want[f]), (n, split)
        assert np.array_equal(want[f].cpu().numpy(), J.reference(n).flat), n


def test_wide_frames_fourteen_pieces_each_and_the_reference_pixels():
    pk = jpegdev.pack_frames([J.data(n) for n in J.WIDE])
    assert (pk.geom.mcus_x, pk.geom.mcus_y) == (25, 14) and pk.n_segments == 3
    dj, stream, waves = _resident(pk)
    pieces, status, off = _index(pk, pk.geom.mcus_x, dj, stream, waves)
    rows = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1)
    assert np.diff(off).tolist() == [14, 14, 14] and not status.cpu().numpy().any() and rows["n_mcu"].tolist() == [25] * 42
    perm = np.array([2, 0, 1])
    coeff, err = _items_decode(pk, dj, stream, pieces, rows, perm)
    out = torch.zeros((3, 3, 224, 398), dtype=torch.uint8, device=DEV)
    slot_set = torch.zeros(3, dtype=torch.int32, device=DEV)
    ops.jpeg_pixels_rows(coeff.view(-1), slot_set, dj.table_sets, out, torch.arange(3, dtype=torch.int32, device=DEV), 0, 3, pk.samp)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for f, n in enumerate(J.WIDE):
        assert np.array_equal(out[perm[f]].cpu().numpy(), J.reference(n).rgb), n


def test_a_shard_behind_two_gib_of_stream():
    """piece positions and the stream length are 64-bit: the shard sits past byte 2^31 of the resident buffer"""
    pk = jpegdev.pack_frames([J.data(n) for n in ENC])
    base = (1 << 31) + 4096
    dj, stream, waves = _resident(pk, base=base)
    assert stream.numel() > 1 << 31
    pieces, status, off = _index(pk, 1, dj, stream, waves, base=base)
    want = _whole(pk, dj, waves)
    rows = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1)
    assert not status.cpu().numpy().any() and rows["pos"].min() >= base and rows.size == 16
    got, err = _items_decode(pk, dj, stream, pieces, rows, np.arange(4)[::-1].copy())
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and all(torch.equal(got[3 - f], want[f]) for f in range(4))


def test_rows_that_point_outside_count_as_errors_and_touch_nothing():
    pk = jpegdev.pack_frames([J.data(n) for n in ENC])
    dj, stream, waves = _resident(pk)
    pieces, status, off = _index(pk, 2, dj, stream, waves)
    rows = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1).copy()
    bad = rows.copy()
    bad["pos"][1] = stream.numel() - 4                      # byte range past the stream
    bad["n_mcu"][3] = 9                                     # MCUs past the frame
    bad["set"][4] = 4                                       # no such table set
    bad["st"]["n"][5] = 64                                  # a bit buffer no decode leaves
    bad["st"]["pad"][6] = bad["st"]["n"][6] + 1
    d_bad = torch.from_numpy(bad.view(np.uint8).reshape(-1, jpegdev.PIECE_BYTES)).to(DEV)
    fc = ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp)

    def run(items, n_waves=1):
        coeff = torch.zeros(4 * fc, dtype=torch.int16, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        wv = torch.tensor([[0, len(items)]][:n_waves], dtype=torch.int32, device=DEV)
        ops.jpeg_entropy_items(stream, d_bad, torch.tensor(items, dtype=torch.int32, device=DEV), wv, dj.table_sets,
                               pk.width, pk.height, pk.samp, 0, 4, coeff, err)
        torch.cuda.synchronize()
        return coeff.view(4, fc), int(err.item())
    for piece, slot in ((1, 0), (3, 0), (4, 0), (5, 0), (6, 0), (0, 4), (0, -1), (9, 0), (-1, 0)):
        coeff, word = run([[piece, slot]])
        assert word == 1 << 7 and not coeff.any(), (piece, slot)
    # a lane whose piece is of another table set than its wave's: flagged and skipped, its neighbour decodes
    coeff, word = run([[0, 2], [2, 1]])
    assert word == 1 << 7 and coeff[2].any() and not coeff[[0, 1, 3]].any()
    coeff, word = run([[0, 2], [7, 1]])
    assert word == 1 << 7 and coeff[2].any() and not coeff[[0, 1, 3]].any()
    coeff, word = run([[0, 2]])
    assert word == 0 and coeff[2].any()
    # the index pass: a segment row outside the stream, and piece offsets outside the table
    segs = pk.segments.copy()
    segs[1, 4] = stream.numel()
    st = torch.zeros(pk.n_segments, dtype=torch.int32, device=DEV)
    off2 = off.copy()
    off2[-1] = off[-1] + 1
    p2 = torch.zeros_like(pieces)
    ops.jpeg_entropy_index(stream, 0, torch.from_numpy(segs).to(DEV), waves, dj.table_sets, pk.width, pk.height, pk.samp, 2,
                           torch.from_numpy(off2).to(DEV), 0, p2, st)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 7, 0, 0, 7]
    got = p2.cpu().numpy().view(jpegdev.PIECE).reshape(-1)
    assert got[:off[1]].tobytes() == rows[:off[1]].tobytes() and not np.frombuffer(got[off[1]:off[2]].tobytes(), np.uint8).any()


def test_resident_entries_validate_their_tensors():
    pk = jpegdev.pack_frames([J.data(ENC[0])])
    dj, stream, waves = _resident(pk)
    pieces, status, off = _index(pk, 1, dj, stream, waves)
    d_off = torch.from_numpy(off).to(DEV)
    a = (stream, 0, dj.segments, waves, dj.table_sets, 32, 24, pk.samp, 1, d_off, 0, pieces, status)

    def index(**kw):
        names = ["stream", "base", "segments", "waves", "table_sets", "W", "H", "sampling", "split_mcus", "piece_off", "seg_base",
                 "pieces", "status"]
        return ops.jpeg_entropy_index(*[kw.get(n, v) for n, v in zip(names, a)])
    with pytest.raises(TypeError, match="piece_off"):
        index(piece_off=d_off.long())
    with pytest.raises(TypeError, match="piece_off"):
        index(piece_off=d_off.cpu())
    with pytest.raises(TypeError, match="segments"):
        index(segments=dj.segments.cpu())
    with pytest.raises(ValueError, match="piece offsets"):
        index(piece_off=d_off[:-1].contiguous())
    with pytest.raises(ValueError, match="pieces"):
        index(pieces=pieces.view(-1, 36))
    with pytest.raises(ValueError, match="base"):
        index(base=stream.numel() + 1)
    with pytest.raises(ValueError, match="split_mcus"):
        index(split_mcus=0)
    fc = ops.jpeg_frame_coeffs(32, 24, pk.samp)
    coeff = torch.zeros(fc, dtype=torch.int16, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    items = torch.tensor([[0, 0]], dtype=torch.int32, device=DEV)
    wv = torch.tensor([[0, 1]], dtype=torch.int32, device=DEV)
    b = (stream, pieces, items, wv, dj.table_sets, 32, 24, pk.samp, 0, 1, coeff, err)

    def run(**kw):
        names = ["stream", "pieces", "items", "waves", "table_sets", "W", "H", "sampling", "slot_lo", "n_slots", "coeff", "err"]
        return ops.jpeg_entropy_items(*[kw.get(n, v) for n, v in zip(names, b)])
    with pytest.raises(TypeError, match="items"):
        run(items=items.long())
    with pytest.raises(TypeError, match="items"):
        run(items=items.cpu())
    with pytest.raises(TypeError, match="err"):
        run(err=err.cpu())
    with pytest.raises(ValueError, match="items"):
        run(items=items.view(-1))
    with pytest.raises(ValueError, match="coeff holds"):
        run(n_slots=2)
    with pytest.raises(ValueError, match="slots"):
        run(slot_lo=-1)
    with pytest.raises(TypeError):
        run(coeff=coeff.int())
    out = torch.zeros((2, 3, 24, 32), dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError, match="fill"):
        ops.jpeg_slot_fill(None, torch.zeros(2, dtype=torch.int64, device=DEV), out)
    with pytest.raises(ValueError, match="side"):
        ops.jpeg_slot_fill(torch.zeros(7, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), out)
    # what the fill does: leave, zero, copy, and a side row that does not exist
    for shape in ((3, 24, 32), (3, 5, 7)):
        out = torch.full((5,) + shape, 9, dtype=torch.uint8, device=DEV)
        side = (torch.arange(2 * int(np.prod(shape)), device=DEV) % 251 + 1).to(torch.uint8).view((2,) + shape)
        ops.jpeg_slot_fill(side, torch.tensor([-2, -1, 1, 2, 0], dtype=torch.int32, device=DEV), out)
        assert bool((out[0] == 9).all()) and not out[1].any() and torch.equal(out[2], side[1]) and bool((out[3] == 9).all())
        assert torch.equal(out[4], side[0])
    run()
    torch.cuda.synchronize()
    assert int(err.item()) == 0


# ----------------------------------------------------------------------------- 2. the loader against ResidentClips
CLASSES = {"dive": 1, "turn": 2}
OTHER = {("va", 2): "24x32_444_q90.jpg", ("va", 5): "24x32_cmyk.jpg", ("va", 7): "24x32_grey_q90.jpg",
         ("vb", 3): "24x32_progressive.jpg"}


def _tree(root, other=OTHER):
    """va: ten frames, vb: eight; both cycle the four table sets, `other` replaces some by files the device does not decode"""
    ev = lambda *pairs: [dict(frame=f, label=l) for f, l in pairs]     # noqa: E731
    videos = []
    for video, n, shift, events in (("va", 10, 0, ev((1, "dive"), (8, "turn"))), ("vb", 8, 1, ev((0, "turn"), (4, "dive"), (7, "turn")))):
        os.makedirs(os.path.join(root, video))
        for i in range(n):
            shutil.copy(J.fixture_path(other.get((video, i), ENC[(i + shift) % 4])), os.path.join(root, video, f"frame{i}.jpg"))
        videos.append(dict(video=video, num_frames=n, events=events))
    return videos


def _loaders(root, videos, jkw=None, load_kw=None, **kw):
    frames = TC.load_resident_videos(root, "soccernetball", videos)                     # Pillow-decoded
    ref = TC.ResidentClips(videos, frames, CLASSES, device=DEV, **kw)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, **(load_kw or {}))
    return ref, TC.ResidentJpegClips(videos, jpegs, CLASSES, device=DEV, **dict(kw, **(jkw or {})))


def _compare(ref, got, passes=2, lam_seed=3):
    rs = np.random.RandomState(lam_seed)
    n = 0
    for _ in range(passes):
        for w, g in itertools.zip_longest(feeder.prefetch(ref, DEV), feeder.prefetch(got, DEV)):
            assert w is not None and g is not None
            assert {k for k in w if not k.startswith("_")} == {k for k in g if not k.startswith("_")}
            for k in w:
                if k.startswith("label"):
                    assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), (n, k)
            B = w["label"].shape[0]
            if "mix" in w:
                lam = torch.from_numpy(rs.beta(0.2, 0.2, B).astype(np.float32)).to(DEV)
                a, b = g["mix"](lam), w["mix"](lam)
                assert a.dtype == torch.float32 and torch.equal(a, b), n
            else:
                assert g["frame"].dtype == torch.uint8 and g["frame"].shape == w["frame"].shape
                assert torch.equal(g["frame"], w["frame"]), n
            n += 1
    torch.cuda.synchronize()
    return n


@pytest.mark.parametrize("per_mcu", [False, True], ids=["per_row", "per_mcu"])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mixup", [False, True], ids=["plain", "mixup"])
def test_resident_jpeg_clips_equal_resident_clips_over_two_passes(tmp_path, mixup, stride, radius, per_mcu):
    videos = _tree(str(tmp_path))
    kw = dict(clip_len=6, stride=stride, overlap=1, mixup=mixup, radi_displacement=radius, dataset_len=7, batch_size=3, seed=21)
    ref, got = _loaders(str(tmp_path), videos, jkw=dict(split_mcus=1 if per_mcu else None), **kw)
    assert len(got) == len(ref) == 3 and got.depth == 3                       # 6 batches (the third is short) through 3 entries
    assert _compare(ref, got) == 6
    st = got.stats
    assert (st["frames"], st["device_frames"], st["fallback_frames"]) == (18, 14, 4) and st["index_flagged"] == []
    assert (st["shards"], st["table_sets"], st["segments"]) == (1, 4, 14 + 3)     # the restart file has two segments
    assert st["pieces"] == (14 * 4 if per_mcu else 11 * 2 + 3 * 3)            # 2 x 2 MCUs; the restart file: (0, 3) and (3, 1)
    assert st["decoded_bytes"] == 18 * 3 * 24 * 32 and st["resident_bytes"] == \
        st["stream_bytes"] + 17 * 24 + st["pieces"] * 72 + 4 * 4240 + 4 * 2304


def test_resident_jpeg_clips_in_shards_and_coefficient_chunks(tmp_path):
    videos = _tree(str(tmp_path))
    kw = dict(clip_len=6, stride=1, overlap=1, mixup=True, radi_displacement=2, dataset_len=7, batch_size=3, seed=5)
    ref, got = _loaders(str(tmp_path), videos, load_kw=dict(shard_bytes=1024),
                        jkw=dict(max_coeff_bytes=5 * 2 * ops.jpeg_frame_coeffs(32, 24, 3)), **kw)
    assert got.stats["shards"] >= 2 and got._chunk == 5
    assert _compare(ref, got) == 6
    assert (got.stats["device_frames"], got.stats["fallback_frames"]) == (14, 4)


def test_truncated_frame_is_flagged_by_the_index_pass_and_served_as_pillow_serves_it(tmp_path):
    root = str(tmp_path)
    videos = _tree(root, other={})
    name = os.path.join(root, "va", "frame5.jpg")
    data = open(name, "rb").read()
    info = jpegdev.parse(data)
    with open(name, "wb") as f:
        f.write(data[:info.scan_start + (info.scan_end - info.scan_start) // 2])          # truncated in the middle of its scan
    kw = dict(clip_len=6, stride=1, overlap=1, mixup=False, radi_displacement=0, dataset_len=6, batch_size=3, seed=9)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos)
    assert jpegs.fallback == []
    try:
        feeder.read_frame(name)
        exc = None
    except Exception as e:          # noqa: BLE001  (whatever the installed Pillow raises is what the loader must raise)
        exc = e
    if exc is not None:
        with pytest.raises(type(exc)):
            TC.ResidentJpegClips(videos, jpegs, CLASSES, device=DEV, **kw)
        torch.cuda.synchronize()
        return
    ref, got = _loaders(root, videos, **kw)
    assert got.stats["index_flagged"] == [5] and (got.stats["device_frames"], got.stats["fallback_frames"]) == (17, 1)
    assert _compare(ref, got, passes=1) == 2


def test_unreleased_slot_and_explicit_wait_and_done_on_the_consumers_stream(tmp_path):
    videos = _tree(str(tmp_path))
    kw = dict(clip_len=6, stride=1, overlap=0.5, mixup=False, radi_displacement=0, dataset_len=10, batch_size=2, seed=2,
              drop_last=True)
    ref, got = _loaders(str(tmp_path), videos, **kw)
    want = [(b["frame"].clone(), b["label"].clone()) for b in feeder.prefetch(ref, DEV)]
    st = torch.cuda.Stream()
    held = []
    with torch.cuda.stream(st):
        for b in got:
            assert "_slot" in b and "labelD" not in b
            feeder.wait(b)
            held.append((b["frame"].clone(), b["label"].clone()))         # queued on st, after the arrival event
            feeder.done(b)
        st.synchronize()
    assert len(held) == len(want) == 5
    for (fr, lab), (wf, wl) in zip(held, want):
        assert torch.equal(fr, wf) and torch.equal(lab, wl)
    with pytest.raises(RuntimeError, match="never released"):
        list(got)                                                         # batches kept and never released


def test_a_set_too_large_decoded_fits_compressed(tmp_path, monkeypatch):
    root = str(tmp_path)
    videos = _tree(root, other={})
    kw = dict(clip_len=6, stride=1, overlap=1, mixup=False, radi_displacement=2, dataset_len=7, batch_size=3, seed=4)
    frames = TC.load_resident_videos(root, "soccernetball", videos)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos)
    free = TC.ResidentJpegClips(videos, jpegs, CLASSES, device=DEV, **kw)
    compressed, decoded = free.stats["resident_bytes"], free.stats["decoded_bytes"]
    assert decoded == 18 * 2304 == sum(f.numel() for f in frames) and compressed < decoded
    budget = (compressed + decoded) // 2
    with pytest.raises(ValueError, match="sharded epochs"):
        TC.ResidentClips(videos, frames, CLASSES, device=DEV, max_resident_bytes=budget, **kw)
    got = TC.ResidentJpegClips(videos, jpegs, CLASSES, device=DEV, max_resident_bytes=budget, **kw)
    ref = TC.ResidentClips(videos, frames, CLASSES, device=DEV, **kw)
    assert _compare(ref, got) == 6 and got.stats["resident_bytes"] == compressed <= budget
    from tdeed_amd import streams

    def no_upload(*a, **k):
        raise AssertionError("uploaded before the check")
    monkeypatch.setattr(streams, "new_stream", no_upload)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        TC.ResidentJpegClips(videos, jpegs, CLASSES, device=DEV, max_resident_bytes=compressed - 1, **kw)
    with pytest.raises(AssertionError, match="uploaded before"):
        TC.ResidentJpegClips(videos, jpegs, CLASSES, device=DEV, max_resident_bytes=compressed, **kw)   # fitting: goes on


# ----------------------------------------------------------------------------- 3. epoch()
def _write_videos(root, h, w, lengths=(20, 37, 9)):
    from PIL import Image
    ev = lambda *pairs: [dict(frame=f, label=l) for f, l in pairs]     # noqa: E731
    events = [ev((1, "dive"), (12, "turn")), ev((0, "turn"), (6, "dive"), (17, "turn"), (36, "dive")), ev((4, "dive"))]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    videos = []
    for v, n in enumerate(lengths):
        d = os.path.join(root, f"v{v}")
        os.makedirs(d)
        rng = np.random.default_rng(700 + v)
        for i in range(n):
            base = np.stack([30 + 180 * xx / (w - 1), 40 + 170 * yy / (h - 1), 128 + 90 * np.sin(0.11 * xx + i + v) * np.cos(0.07 * yy)], -1)
            px = np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(px).save(os.path.join(d, f"frame{i}.jpg"), "JPEG", quality=90, subsampling=2)
        videos.append(dict(video=f"v{v}", num_frames=n, events=events[v]))
    return videos


def _tiny_model():
    from tdeed_amd.model import TDEEDModel
    meta, _ = load_golden("tiny_rny002_gsf")
    torch.manual_seed(11)
    return TDEEDModel(device=DEV, args=cfg_ns(meta["cfg"])), meta


def _train_once(make_loader):
    m, meta = _tiny_model()
    opt, _ = m.get_optimizer({"lr": 3e-4})
    loader = make_loader()
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    loss = m.epoch(loader, optimizer=opt)
    torch.cuda.synchronize()
    after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(before[k], after[k]) for k in after)          # the epoch trained
    return loss, after


def test_training_epoch_fed_by_resident_jpeg_clips_equals_the_resident_clips_fed_epoch(tmp_path):
    """Mixup, radi_displacement of the tiny 200MF model, 64 x 64 4:2:0 frames: the batches are the same bits, so are the
    loss and every parameter."""
    meta, _ = load_golden("tiny_rny002_gsf")
    cfg = meta["cfg"]
    root = str(tmp_path)
    videos = _write_videos(root, meta["H"], meta["W"])
    kw = dict(clip_len=cfg["clip_len"], stride=1, overlap=1, mixup=True, dataset_len=4, batch_size=2, seed=31,
              radi_displacement=cfg["radi_displacement"], device=DEV)
    made = {}

    def res():
        return TC.ResidentClips(videos, TC.load_resident_videos(root, "soccernetball", videos), CLASSES, **kw)

    def jpg():
        made["l"] = TC.ResidentJpegClips(videos, TC.load_resident_jpegs(root, "soccernetball", videos), CLASSES, **kw)
        return made["l"]
    l_res, p_res = _train_once(res)
    l_jpg, p_jpg = _train_once(jpg)
    print(f"loss ResidentClips-fed {l_res!r}, ResidentJpegClips-fed {l_jpg!r}")
    assert made["l"].stats["fallback_frames"] == 0 and made["l"].stats["pieces"] == 66 * 4
    assert np.isfinite(l_res) and l_jpg == l_res
    assert all(torch.equal(p_jpg[k], p_res[k]) for k in p_res)


def test_validation_epoch_fed_by_resident_jpeg_clips_equals_the_resident_clips_fed_one(tmp_path):
    m, meta = _tiny_model()
    cfg = meta["cfg"]
    root = str(tmp_path)
    videos = _write_videos(root, meta["H"], meta["W"])
    kw = dict(clip_len=cfg["clip_len"], stride=2, overlap=1, mixup=False, dataset_len=5, batch_size=2, seed=33,
              radi_displacement=cfg["radi_displacement"], device=DEV)
    want = m.epoch(TC.ResidentClips(videos, TC.load_resident_videos(root, "soccernetball", videos), CLASSES, **kw))
    got = m.epoch(TC.ResidentJpegClips(videos, TC.load_resident_jpegs(root, "soccernetball", videos), CLASSES, **kw))
    assert np.isfinite(want) and got == want
