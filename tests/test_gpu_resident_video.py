"""Validation videos from resident JPEG streams on the MI355X: the windowed pixel kernel (ops.jpeg_pixels_window) against the
numpy model's pixels and against ops.jpeg_pixels_rows, the MCU-row filter of the item tables, `evalutil.ResidentJpegVideos.
frames` against `feeder.load_video`, and stitch_videos / spot_videos / map_videos over its sources against the same calls
over Pillow-decoded tensors, bit for bit.  -m gpu only."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as J
from tdeed_amd import evalutil as E
from tdeed_amd import feeder, jpegdev, ops
from tdeed_amd import trainclips as TC
import test_gpu_resident_jpeg as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- 1. the kernel
def _windows(H, W):
    """block-aligned, mid-block even left, odd left, one pixel wide, touching the right and bottom edges, one row across a
    band border, from (16, 1) to the far corner, the full frame -- those that fit"""
    cand = [(8, 16, 16, 16), (3, 10, 9, 13), (1, 5, 7, 16), (0, W // 2, H, 1), (H - 5, W - 7, 5, 7), (15, 0, 2, W),
            (16, 1, H - 16, W - 1), (0, 0, H, W)]
    out = []
    for top, left, wh, ww in cand:
        if top >= 0 and left >= 0 and wh > 0 and ww > 0 and top + wh <= H and left + ww <= W and (top, left, wh, ww) not in out:
            out.append((top, left, wh, ww))
    return out


def _decoded(names, split=None):
    """the files' coefficients on the device, frame f in slot perm[f] -> (pack, tables, coeff (n, fc), perm)"""
    pk = jpegdev.pack_frames([J.data(n) for n in names])
    assert pk.fallback == []
    dj, stream, waves = R._resident(pk)
    pieces, status, _ = R._index(pk, split or pk.geom.mcus_x, dj, stream, waves)
    rows = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1)
    perm = np.random.RandomState(len(names) + pk.width).permutation(pk.n_frames)
    coeff, err = R._items_decode(pk, dj, stream, pieces, rows, perm)
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and not status.cpu().numpy().any()
    return pk, dj, coeff, perm


def _window_launch(pk, dj, coeff, slot_set, dst_row, win, rows=None):
    top, left, wh, ww = win
    n = pk.n_frames
    out = torch.full((rows or n, 3, wh, ww), 0xA5, dtype=torch.uint8, device=DEV)
    ops.jpeg_pixels_window(coeff.view(-1), slot_set, dj.table_sets, out, dst_row, 0, n, pk.samp, pk.height, pk.width, top, left)
    return out


@pytest.mark.parametrize("gid", R.GROUPS)
def test_window_kernel_equals_the_reference_window(gid):
    names = J.groups()[gid]
    pk, dj, coeff, perm = _decoded(names)
    H, W, n = pk.height, pk.width, pk.n_frames
    slot_set = torch.zeros(n, dtype=torch.int32, device=DEV)
    slot_set[torch.from_numpy(perm).to(DEV)] = torch.from_numpy(pk.frame_set).to(DEV)
    ident = torch.arange(n, dtype=torch.int32, device=DEV)
    wins = _windows(H, W)
    assert (0, 0, H, W) in wins
    for win in wins:
        top, left, wh, ww = win
        out = _window_launch(pk, dj, coeff, slot_set, ident, win)
        torch.cuda.synchronize()
        for f, nm in enumerate(names):
            assert np.array_equal(out[perm[f]].cpu().numpy(), J.reference(nm).rgb[:, top:top + wh, left:left + ww]), (nm, win)
    # the full window: the bits of jpeg_pixels_rows
    full = torch.zeros((n, 3, H, W), dtype=torch.uint8, device=DEV)
    ops.jpeg_pixels_rows(coeff.view(-1), slot_set, dj.table_sets, full, ident, 0, n, pk.samp)
    assert torch.equal(_window_launch(pk, dj, coeff, slot_set, ident, (0, 0, H, W)), full)
    # a frame whose set is -1 and a frame whose row is out of range store nothing; rows are a table, not the identity
    win = wins[0]
    sets2 = slot_set.clone()
    sets2[0] = -1
    rows2 = torch.arange(n, dtype=torch.int32, device=DEV) + 1
    rows2[n - 1] = -1 if n > 1 else n + 1
    out = _window_launch(pk, dj, coeff, sets2, rows2, win, rows=n + 1)
    ref = _window_launch(pk, dj, coeff, slot_set, ident, win)
    torch.cuda.synchronize()
    assert bool((out[0] == 0xA5).all()) and bool((out[1] == 0xA5).all())
    for s in range(1, n - 1):
        assert torch.equal(out[s + 1], ref[s])
    if n > 1:
        assert bool((out[n] == 0xA5).all())


def test_window_kernel_on_the_dataset_geometry():
    """224 x 398 4:2:0, the centre 224 x 224 (16-byte stores, left = 87 odd) and an unaligned width (byte stores)"""
    pk, dj, coeff, perm = _decoded(J.WIDE)
    slot_set = torch.zeros(3, dtype=torch.int32, device=DEV)
    ident = torch.arange(3, dtype=torch.int32, device=DEV)
    for win in ((0, 87, 224, 224), (33, 86, 100, 225), (0, 0, 224, 398)):
        top, left, wh, ww = win
        out = _window_launch(pk, dj, coeff, slot_set, ident, win)
        torch.cuda.synchronize()
        for f, nm in enumerate(J.WIDE):
            assert np.array_equal(out[perm[f]].cpu().numpy(), J.reference(nm).rgb[:, top:top + wh, left:left + ww]), (nm, win)


def test_window_entry_validates_its_arguments():
    from tdeed_amd._lib import call, HipCallError
    pk, dj, coeff, perm = _decoded(J.groups()["24x32_420"])
    n = pk.n_frames
    slot_set = torch.zeros(n, dtype=torch.int32, device=DEV)
    ident = torch.arange(n, dtype=torch.int32, device=DEV)
    out = torch.zeros((n, 3, 8, 16), dtype=torch.uint8, device=DEV)
    a = (coeff.view(-1), slot_set, dj.table_sets, out, ident, 0, n, pk.samp, 24, 32, 0, 0)
    ops.jpeg_pixels_window(*a)
    for top, left in ((17, 0), (0, 17), (-1, 0), (0, -1)):
        with pytest.raises(ValueError, match="leaves"):
            ops.jpeg_pixels_window(*a[:10], top, left)
    with pytest.raises(TypeError, match="dst_row"):
        ops.jpeg_pixels_window(*a[:4], ident.long(), *a[5:])
    with pytest.raises(ValueError, match="coeff holds"):
        ops.jpeg_pixels_window(coeff.view(-1)[:-1].clone(), *a[1:])
    with pytest.raises(ValueError, match="out must be"):
        ops.jpeg_pixels_window(*a[:3], out.view(n, 3, -1), *a[4:])
    # the launcher's own check (TD_CHECK), behind the wrapper's
    P = ops.ptr
    for top, left, wh, ww in ((17, 0, 8, 16), (0, 17, 8, 16), (0, 0, 0, 16), (0, 0, 8, 0), (-1, 0, 8, 16)):
        with pytest.raises(HipCallError, match="empty or leaves"):
            call("tdeed_jpeg_pixels_window", P(coeff), P(slot_set), P(dj.table_sets), dj.table_sets.shape[0], P(out), n, P(ident), 0, n,
                 24, 32, pk.samp, top, left, wh, ww, ops.stream_ptr())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 2. unlisted pieces are never read
@pytest.mark.parametrize("split", [1, 4], ids=["per_mcu", "per_row"])
def test_coefficients_of_unlisted_pieces_are_never_read(split):
    """40 x 56 4:2:0 (3 x 4 MCUs), a window inside the middle MCU row: the items leave out the pieces of the other rows, whose
    coefficient ranges hold 0x7FFF when the pixel pass runs"""
    names = J.groups()["40x56_420"]
    pk = jpegdev.pack_frames([J.data(n) for n in names])
    g, n = pk.geom, pk.n_frames
    dj, stream, waves = R._resident(pk)
    pieces, status, off = R._index(pk, split, dj, stream, waves)
    win = (17, 9, 14, 31)
    wb = jpegdev.window_blocks(g, *win)
    assert wb.mcu_rows == (1, 2)
    pm = jpegdev.piece_ranges(pk.segments, split)
    cnt = jpegdev.piece_counts(pk.segments, split)
    fr_of_piece = np.repeat(pk.segments[:, 0], cnt)
    lo, hi = wb.mcu_rows
    listed = ((pm[:, 0] + pm[:, 1] - 1) // g.mcus_x >= lo) & (pm[:, 0] // g.mcus_x < hi)
    fc = ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp)
    host = np.zeros((n, fc), np.int16)
    bw0 = g.bw[0]
    for p in np.flatnonzero(~listed):
        f = int(fr_of_piece[p])
        for m in range(int(pm[p, 0]), int(pm[p, 0] + pm[p, 1])):
            my, mx = divmod(m, g.mcus_x)
            assert not lo <= my < hi
            for v in range(2):
                for h in range(2):
                    b = (my * 2 + v) * bw0 + mx * 2 + h
                    host[f, b * 64:(b + 1) * 64] = 0x7FFF
            for c in (1, 2):
                b = g.boff[c] + my * g.mcus_x + mx
                host[f, b * 64:(b + 1) * 64] = 0x7FFF
    assert (host == 0x7FFF).any()
    coeff = torch.from_numpy(host).to(DEV).view(-1)
    keep = np.flatnonzero(listed)
    sets = pieces.cpu().numpy().view(jpegdev.PIECE).reshape(-1)["set"]
    keep = keep[np.argsort(sets[keep], kind="stable")]
    items = np.stack([keep, fr_of_piece[keep]], 1).astype(np.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.jpeg_entropy_items(stream, pieces, torch.from_numpy(items).to(DEV), torch.from_numpy(TC._cut_waves(sets[keep])).to(DEV),
                           dj.table_sets, pk.width, pk.height, pk.samp, 0, n, coeff, err)
    slot_set = torch.from_numpy(pk.frame_set).to(DEV)
    out = _window_launch(pk, dj, coeff.view(n, fc), slot_set, torch.arange(n, dtype=torch.int32, device=DEV), win)
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and not status.cpu().numpy().any()
    top, left, wh, ww = win
    for f, nm in enumerate(names):
        assert np.array_equal(out[f].cpu().numpy(), J.reference(nm).rgb[:, top:top + wh, left:left + ww]), nm
    # the whole frame over the same buffer does read them: the poison is where the test says it is
    full = _window_launch(pk, dj, coeff.view(n, fc), slot_set, torch.arange(n, dtype=torch.int32, device=DEV), (0, 0, 40, 56))
    assert not np.array_equal(full[0].cpu().numpy(), J.reference(names[0]).rgb)


# ----------------------------------------------------------------------------- 3. frames(i) against feeder.load_video
def _videos_with_fps(videos):
    return [dict(v, fps=25.0 + i) for i, v in enumerate(videos)]


def _want(root, videos, stride, window):
    out = []
    for v in videos:
        fr = feeder.load_video(root, "soccernetball", v["video"], v["num_frames"], stride=stride)
        if window is not None:
            top, left, wh, ww = window
            fr = fr[:, :, top:top + wh, left:left + ww]
        out.append(fr)
    return out


@pytest.mark.parametrize("crop", [None, (16, 24), 23], ids=["full", "crop16x24", "crop23"])
@pytest.mark.parametrize("per_mcu", [False, True], ids=["per_row", "per_mcu"])
@pytest.mark.parametrize("stride", [1, 2])
def test_frames_equal_load_video(tmp_path, stride, per_mcu, crop):
    """four table sets, a restart file, CMYK / progressive / grey / 4:4:4 files in the side buffer; every video twice"""
    root = str(tmp_path)
    videos = _videos_with_fps(R._tree(root))
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, stride=stride)
    rv = E.ResidentJpegVideos(videos, jpegs, crop=crop, split_mcus=1 if per_mcu else None, device=DEV)
    window = {None: None, (16, 24): (4, 4, 16, 24), 23: (0, 4, 23, 23)}[crop]
    assert rv.window == window
    want = _want(root, videos, stride, window)
    for _ in range(2):
        for i, w in enumerate(want):
            got = rv.frames(i)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(w.shape)
            assert torch.equal(got.cpu(), w), (i, stride, per_mcu, crop)
    out = torch.zeros_like(rv.frames(1))
    assert rv.frames(1, out=out) is out and torch.equal(out.cpu(), want[1])
    with pytest.raises(ValueError, match="out must be"):
        rv.frames(0, out=out)
    src = rv.sources()
    assert [(s[0], s[1], s[2]) for s in src] == [(v["video"], w.shape[0], v["fps"]) for v, w in zip(videos, want)]
    assert torch.equal(src[0][3]().cpu(), want[0])
    st = rv.stats
    side_bytes = 3 * (24 * 32 if window is None else window[2] * window[3])
    assert st["frame_shape"] == (3,) + tuple(want[0].shape[2:]) and st["decoded_bytes_per_frame"] == side_bytes
    if stride == 1:
        assert (st["frames"], st["device_frames"], st["fallback_frames"]) == (18, 14, 4) and st["index_flagged"] == []
        assert (st["shards"], st["table_sets"], st["segments"]) == (1, 4, 14 + 3)
        assert st["pieces"] == (14 * 4 if per_mcu else 11 * 2 + 3 * 3)
        assert st["decoded_bytes"] == 18 * 2304 and st["resident_bytes"] == \
            st["stream_bytes"] + 17 * 24 + st["pieces"] * 72 + 4 * 4240 + 4 * side_bytes
    else:
        assert (st["frames"], st["device_frames"], st["fallback_frames"]) == (9, 8, 1) and st["index_flagged"] == []
    if window is not None and not per_mcu:
        tb = rv.video_tables(0)                                   # 24 x 32 4:2:0 is 2 x 2 MCUs; rows 4..19 read both MCU rows
        assert tb.items.shape[0] == int(rv._rs.piece_n[:rv.video_len[0]].sum())


def test_frames_in_shards_and_coefficient_chunks(tmp_path):
    root = str(tmp_path)
    videos = _videos_with_fps(R._tree(root))
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, shard_bytes=1024)
    fc = ops.jpeg_frame_coeffs(32, 24, 3)
    for crop in (None, (9, 17)):
        rv = E.ResidentJpegVideos(videos, jpegs, crop=crop, max_coeff_bytes=3 * 2 * fc, device=DEV)
        assert rv.stats["shards"] >= 2 and rv._chunk == 3 and len(rv.video_tables(0).chunks) == 4
        want = _want(root, videos, 1, rv.window)
        for _ in range(2):
            for i, w in enumerate(want):
                assert torch.equal(rv.frames(i).cpu(), w), (crop, i)
        assert (rv.stats["device_frames"], rv.stats["fallback_frames"]) == (14, 4)


def test_truncated_frame_is_served_as_pillow_serves_it(tmp_path):
    root = str(tmp_path)
    videos = _videos_with_fps(R._tree(root, other={}))
    name = os.path.join(root, "va", "frame5.jpg")
    data = open(name, "rb").read()
    info = jpegdev.parse(data)
    with open(name, "wb") as f:
        f.write(data[:info.scan_start + (info.scan_end - info.scan_start) // 2])
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos)
    try:
        feeder.read_frame(name)
        exc = None
    except Exception as e:          # noqa: BLE001  (whatever the installed Pillow raises is what the loader must raise)
        exc = e
    if exc is not None:
        with pytest.raises(type(exc)):
            E.ResidentJpegVideos(videos, jpegs, device=DEV)
        torch.cuda.synchronize()
        return
    for crop in (None, 16):
        rv = E.ResidentJpegVideos(videos, jpegs, crop=crop, device=DEV)
        assert rv.stats["index_flagged"] == [5] and (rv.stats["device_frames"], rv.stats["fallback_frames"]) == (17, 1)
        for i, w in enumerate(_want(root, videos, 1, rv.window)):
            assert torch.equal(rv.frames(i).cpu(), w)


@pytest.mark.parametrize("samp", [2, 1], ids=["420", "422"])
@pytest.mark.parametrize("W", [72, 580, 1220])
def test_frames_wider_padded_grid_than_frame(tmp_path, W, samp):
    """W % 16 in 1..8 with 2:1 chroma: the padded MCU grid is one luma block column wider than the frame, and the frame
    instances' LDS planes are as wide as the grid (at these widths the two sizes fall into different allocation units of
    512 or 1280 bytes).  17 rows: two bands of 4:2:0.  Both frame instances, and the window instance on a centre window."""
    from PIL import Image
    root, H = str(tmp_path), 17
    os.makedirs(os.path.join(root, "v"))
    rng = np.random.default_rng(W + samp)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(3):
        px = np.stack([40 + 170 * xx / (W - 1), 30 + 12 * yy, 128 + 90 * np.sin(0.13 * xx + i)], -1) + rng.integers(-20, 21, (H, W, 3))
        Image.fromarray(np.clip(px, 0, 255).astype(np.uint8)).save(os.path.join(root, "v", f"frame{i}.jpg"), "JPEG", quality=92,
                                                                     subsampling=samp)
    videos = [dict(video="v", num_frames=3, fps=25.0)]
    want = feeder.load_video(root, "soccernetball", "v", 3)
    got = feeder.load_video_device(root, "soccernetball", "v", 3, device=DEV)          # tdeed_jpeg_pixels
    assert feeder.last_decode_stats["fallback_frames"] == 0 and torch.equal(got.cpu(), want)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos)
    rv = E.ResidentJpegVideos(videos, jpegs, device=DEV)                               # tdeed_jpeg_pixels_rows
    assert rv.stats["fallback_frames"] == 0 and torch.equal(rv.frames(0).cpu(), want)
    rc = E.ResidentJpegVideos(videos, jpegs, crop=(9, W - 40), device=DEV)              # the window instance
    top, left, wh, ww = rc.window
    assert torch.equal(rc.frames(0).cpu(), want[:, :, top:top + wh, left:left + ww])


# ----------------------------------------------------------------------------- 4-7. the consumers, tiny model
from test_gpu_spot import TINY, CLASSES, _model          # noqa: E402

SUPPRESS = (("nms", 1, 0.01), ("snms", [3, 1, 2], 0.01))
KW = dict(augment=True, batch_size=4, group_videos=2)


@pytest.fixture(scope="module")
def tiny_set(tmp_path_factory):
    """64 x 64 4:2:0 videos of 20, 37 and 9 frames; Pillow's decode of each"""
    root = str(tmp_path_factory.mktemp("resident_video"))
    videos = _videos_with_fps(R._write_videos(root, 64, 64))
    decoded = [feeder.load_video(root, "soccernetball", v["video"], v["num_frames"]) for v in videos]
    truth = [{"video": v["video"], "events": [{"label": "c1", "frame": 3}, {"label": "c2", "frame": 5}, {"label": "c2", "frame": 5},
                                              {"label": "c3", "frame": 7}, {"label": "c1", "frame": v["num_frames"] - 1}]}
             for v in videos]
    return root, videos, decoded, truth


def _tensor_sources(videos, frames):
    return [(v["video"], int(f.shape[0]), v["fps"], f) for v, f in zip(videos, frames)]


def _all_three(m, vids, truth):
    st = E.stitch_videos(m, vids, 4, **KW)
    s_stats = dict(m.last_video_stats)
    spot = E.spot_videos(m, vids, CLASSES, SUPPRESS, **KW)
    p_stats = dict(m.last_video_stats)
    maps = E.map_videos(m, vids, CLASSES, truth, (("raw",),) + SUPPRESS, [0, 1, 2, 4], **KW)
    return st, spot, maps, (s_stats, p_stats, dict(m.last_video_stats))


def test_consumers_over_sources_equal_the_pillow_fed_ones(tiny_set, monkeypatch):
    root, videos, decoded, truth = tiny_set
    m = _model(TINY)
    want = _all_three(m, _tensor_sources(videos, decoded), truth)
    rv = E.ResidentJpegVideos(videos, TC.load_resident_jpegs(root, "soccernetball", videos), device=DEV)
    assert rv.stats["fallback_frames"] == 0 and rv.stats["frames"] == 66 and rv.stats["pieces"] == 66 * 4

    def no_file(*a, **k):
        raise AssertionError("a file was read after construction")
    for name in ("read_frame", "_read_file", "_read_file_stat", "load_video", "load_video_device"):
        monkeypatch.setattr(feeder, name, no_file)
    got = _all_three(m, rv.sources(), truth)                        # no host decode after construction: a full pass each
    for v in videos:
        for a, b in zip(got[0].tracks[v["video"]], want[0].tracks[v["video"]]):
            assert np.array_equal(a, b), v["video"]
    assert got[0].fps == want[0].fps
    assert got[1][0] == want[1][0] and got[1][1] == want[1][1]
    assert sorted(got[1][2]) == sorted(want[1][2]) and all(np.array_equal(got[1][2][k], want[1][2][k]) for k in want[1][2])
    assert got[2] == want[2] and max(got[2][0][0]) > 0              # mAP and AP floats, bit for bit
    for g, w in zip(got[3], want[3]):
        assert all(g[k] == w[k] for k in ("host_syncs", "frames", "clips"))
    assert got[3][2]["frames"] == 66 and got[3][2]["groups"] == 2


def test_crop_end_to_end(tiny_set):
    root, videos, decoded, truth = tiny_set
    m = _model(dict(TINY, crop_dim=48))
    rv = E.ResidentJpegVideos(videos, TC.load_resident_jpegs(root, "soccernetball", videos), crop=48, device=DEV)
    assert rv.window == (8, 8, 48, 48) and rv.stats["frame_shape"] == (3, 48, 48)
    for i, f in enumerate(decoded):
        assert torch.equal(rv.frames(i).cpu(), f[..., 8:56, 8:56])
    host_cropped = [f[..., 8:56, 8:56].contiguous() for f in decoded]
    want = E.stitch_videos(m, _tensor_sources(videos, host_cropped), 4, **KW)
    got = E.stitch_videos(m, rv.sources(), 4, **KW)
    for v in videos:
        for a, b in zip(got.tracks[v["video"]], want.tracks[v["video"]]):
            assert np.array_equal(a, b), v["video"]
    assert E.map_videos(m, rv.sources(), CLASSES, truth, SUPPRESS, [0, 1, 2], **KW) == \
        E.map_videos(m, _tensor_sources(videos, host_cropped), CLASSES, truth, SUPPRESS, [0, 1, 2], **KW)
    # the uncropped route: the first launch reads the same window through its rectangle
    whole = E.stitch_videos(m, _tensor_sources(videos, decoded), 4, **KW)
    for v in videos:
        for a, b in zip(got.tracks[v["video"]], whole.tracks[v["video"]]):
            assert np.array_equal(a, b), v["video"]


def test_budgets(tiny_set, monkeypatch):
    root, videos, decoded, truth = tiny_set
    m = _model(TINY)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos)
    free = E.ResidentJpegVideos(videos, jpegs, device=DEV)
    compressed, dec = free.stats["resident_bytes"], free.stats["decoded_bytes"]
    assert dec == 66 * 3 * 64 * 64 == sum(f.numel() for f in decoded) and compressed < dec
    # a set that does not fit decoded fits compressed, and is scored
    budget = (compressed + dec) // 2
    rv = E.ResidentJpegVideos(videos, jpegs, max_resident_bytes=budget, device=DEV)
    assert rv.stats["resident_bytes"] == compressed <= budget < dec
    got = E.stitch_videos(m, rv.sources(), 4, augment=True, batch_size=4)
    want = E.stitch_videos(m, _tensor_sources(videos, decoded), 4, augment=True, batch_size=4)
    for v in videos:
        for a, b in zip(got.tracks[v["video"]], want.tracks[v["video"]]):
            assert np.array_equal(a, b)
    from tdeed_amd import streams

    def no_upload(*a, **k):
        raise AssertionError("uploaded before the check")
    monkeypatch.setattr(streams, "new_stream", no_upload)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.ResidentJpegVideos(videos, jpegs, max_resident_bytes=compressed - 1, device=DEV)
    with pytest.raises(AssertionError, match="uploaded before"):
        E.ResidentJpegVideos(videos, jpegs, max_resident_bytes=compressed, device=DEV)       # fitting: goes on
