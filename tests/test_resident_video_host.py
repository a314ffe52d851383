"""Validation videos from resident JPEG streams, without a GPU: `jpegdev.window_blocks` (and the launcher's jc_window behind
ops.jpeg_window_blocks) against a brute-force walk of the samples jc_pixel's rule touches, `trainclips.video_tables` against
a loop, `load_resident_jpegs(stride=...)`, the argument errors of `evalutil.ResidentJpegVideos`, and
tools/jpeg_window_check.cpp -- the windowed band loop on the host, over exact-size buffers and, where the compiler has
them, under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import jpeg_cases as J
from helpers import ROOT
from tdeed_amd import evalutil as E
from tdeed_amd import jpegdev
from tdeed_amd import trainclips as TC

SIZES = [(24, 32), (23, 37), (17, 49), (40, 56), (8, 8), (1, 1)]
GEOMS = [(h, w, s) for h, w in SIZES for s in (jpegdev.S444, jpegdev.S422, jpegdev.S420)] + \
    [(24, 32, jpegdev.GREY), (224, 398, jpegdev.S420)]
TOPS, WIDTHS, HEIGHTS = [0, 1, 7, 8, 15, 16], [1, 2, 15, 16, 17, None], [1, 9, None]


def windows(H, W):
    """the grid: every left in 0..17, widths 1, 2, 15, 16, 17 and to the right edge, tops 0, 1, 7, 8, 15, 16, heights 1, 9 and
    to the bottom edge -- those that fit the frame"""
    out = []
    for top in TOPS:
        for hh in HEIGHTS:
            for left in range(18):
                for wd in WIDTHS:
                    wh, ww = H - top if hh is None else hh, W - left if wd is None else wd
                    if wh > 0 and ww > 0 and top + wh <= H and left + ww <= W:
                        out.append((top, left, wh, ww))
    return out


# ----------------------------------------------------------------------------- 1. window_blocks
def touched_columns(g, left, ww):
    """csrc/jpeg_core.h jc_pixel, the columns: pixel x reads luma column x and, with 2:1 chroma, chroma sample i = x >> 1 and
    its neighbour i + 1 for an odd x, i - 1 for an even x, clamped to [0, cw) -> (luma columns, chroma columns | None)"""
    x = np.arange(left, left + ww)
    if g.ncomp == 1:
        return x, None
    if g.hs == 1:
        return x, x
    i = x >> 1
    nx = np.where(x & 1, np.minimum(i + 1, g.cw[1] - 1), np.maximum(i - 1, 0))
    return x, np.concatenate([i, nx])


def touched_rows(g, top, wh):
    """the rows: luma row y; chroma row y (1:1 vertically) or, 4:2:0, rr = y >> 1 and rr + 1 for an odd y, rr - 1 for an even
    one, clamped to [0, ch)"""
    y = np.arange(top, top + wh)
    if g.ncomp == 1:
        return y, None
    if g.vs == 1:
        return y, y
    rr = y >> 1
    ny = np.where(y & 1, np.minimum(rr + 1, g.ch[1] - 1), np.maximum(rr - 1, 0))
    return y, np.concatenate([rr, ny])


def blocks_of(samples):
    return (int(samples.min()) // 8, int(samples.max()) // 8 + 1)


@pytest.mark.parametrize("H,W,samp", GEOMS, ids=[f"{h}x{w}_{jpegdev.SAMPLING_NAMES[s]}" for h, w, s in GEOMS])
def test_window_blocks_are_the_blocks_of_the_samples_jc_pixel_touches(H, W, samp):
    g = jpegdev.geometry(W, H, samp)
    n = 0
    for top, left, wh, ww in windows(H, W):
        wb = jpegdev.window_blocks(g, top, left, wh, ww)
        ycol, ccol = touched_columns(g, left, ww)
        yrow, crow = touched_rows(g, top, wh)
        # the ranges are exactly the blocks that contain the touched samples: they cover the set and hold no block beyond
        assert wb.y_cols == blocks_of(ycol) and wb.y_rows == blocks_of(yrow), (top, left, wh, ww)
        assert wb.bands == (int(yrow.min()) // (8 * g.vs), int(yrow.max()) // (8 * g.vs) + 1)
        if g.ncomp == 1:
            assert wb.c_cols is None and wb.mcu_rows == wb.bands
        else:
            assert wb.c_cols == blocks_of(ccol), (top, left, wh, ww)
            rows = (min(wb.bands[0], int(crow.min()) // 8), max(wb.bands[1], int(crow.max()) // 8 + 1))
            assert wb.mcu_rows == rows, (top, left, wh, ww)
            assert 0 <= wb.c_cols[0] < wb.c_cols[1] <= g.mcus_x
        assert 0 <= wb.mcu_rows[0] <= wb.bands[0] < wb.bands[1] <= wb.mcu_rows[1] <= g.mcus_y
        assert 0 <= wb.y_cols[0] < wb.y_cols[1] <= g.bw[0] and 0 <= wb.y_rows[0] < wb.y_rows[1] <= g.bh[0]
        n += 1
    assert n > 0
    full = jpegdev.window_blocks(g, 0, 0, H, W)
    assert full.bands == full.mcu_rows == (0, g.mcus_y) and full.y_cols == (0, -(-W // 8)) and full.y_rows == (0, -(-H // 8))
    for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, H + 1, 1), (0, 1, 1, W), (H, 0, 1, 1)):
        with pytest.raises(ValueError, match="window"):
            jpegdev.window_blocks(g, *bad)


def test_the_dataset_window_in_numbers():
    """224 x 398 4:2:0, the centre 224 x 224: 14 of 14 bands, luma block columns 10..38 of 50, chroma 5..19 of 25"""
    wb = jpegdev.window_blocks(jpegdev.geometry(398, 224, jpegdev.S420), 0, 87, 224, 224)
    assert (wb.bands, wb.mcu_rows, wb.y_cols, wb.c_cols) == ((0, 14), (0, 14), (10, 39), (5, 20))
    assert E._crop_window(224, 224, 398) == (0, 87, 224, 224) and E._crop_window((224, 398), 224, 398) is None


def test_the_launchers_ranges_are_window_blocks():
    """csrc/jpeg_core.h jc_window through the built library (no launch): the same ten numbers"""
    import __graft_entry__ as entry
    entry.build()
    from tdeed_amd import ops
    n = 0
    for H, W, samp in GEOMS:
        g = jpegdev.geometry(W, H, samp)
        for top, left, wh, ww in windows(H, W)[::7]:
            assert ops.jpeg_window_blocks(W, H, samp, top, left, wh, ww) == jpegdev.window_blocks(g, top, left, wh, ww).ranges
            n += 1
    assert n > 500
    with pytest.raises(ValueError):
        ops.jpeg_window_blocks(32, 24, 3, 0, 0, 25, 32)


def _kernel_lds_bytes(g, wb):
    """csrc/jpeg.hip jpeg_pixels_kernel, the bytes its planes span: 8 VS luma rows of ypitch, per chroma plane 8 rows (+ 2 halo
    rows, 4:2:0) of cpitch; the pitches are 8 x the block columns phase 1 runs -- the padded MCU grid's (bw0, mcus_x) without
    a window (wb None), window_blocks' with one"""
    nc, crows = (0 if g.ncomp == 1 else 2), 8 + (2 if g.vs == 2 else 0)
    if wb is None:
        ypitch, cpitch = 8 * g.bw[0], 8 * g.mcus_x
    else:
        ypitch, cpitch = 8 * (wb.y_cols[1] - wb.y_cols[0]), (8 * (wb.c_cols[1] - wb.c_cols[0]) if wb.c_cols else 0)
    return 8 * g.vs * ypitch + nc * crows * cpitch


def test_the_launchers_request_the_lds_bytes_the_kernel_addresses():
    """Every fixture geometry, and widths at which the padded grid is a luma block column wider than the frame (W % 16 in
    1..8 with 2:1 chroma: 17, 23 x 37, 65..72, 577..584, 1217..1224): the launchers of the frame instances size the planes
    from the padded grid, the window's from its block columns, the full window included."""
    import __graft_entry__ as entry
    entry.build()
    from tdeed_amd import ops
    extra = [(h, w, s) for s in (jpegdev.S422, jpegdev.S420, jpegdev.S444, jpegdev.GREY) for h in (8, 17)
             for w in (65, 72, 73, 577, 580, 584, 585, 1217, 1224, 4081)]
    n_wider = 0
    for H, W, samp in GEOMS + extra:
        g = jpegdev.geometry(W, H, samp)
        assert ops.jpeg_pixels_lds_bytes(W, H, samp) == _kernel_lds_bytes(g, None), (H, W, samp)
        full = jpegdev.window_blocks(g, 0, 0, H, W)
        assert ops.jpeg_pixels_lds_bytes(W, H, samp, (0, 0, H, W)) == _kernel_lds_bytes(g, full)
        n_wider += _kernel_lds_bytes(g, None) > _kernel_lds_bytes(g, full)
        for win in windows(H, W)[::11]:
            assert ops.jpeg_pixels_lds_bytes(W, H, samp, win) == _kernel_lds_bytes(g, jpegdev.window_blocks(g, *win)), (H, W, samp, win)
    assert n_wider >= 20                                     # the case the two sizes differ in is covered
    g = jpegdev.geometry(49, 17, jpegdev.S420)
    assert (g.bw[0], g.mcus_x) == (8, 4) and ops.jpeg_pixels_lds_bytes(49, 17, jpegdev.S420) == 16 * 64 + 2 * 10 * 32 == 1664
    with pytest.raises(ValueError):
        ops.jpeg_pixels_lds_bytes(32, 24, 3, (0, 0, 25, 32))


# ----------------------------------------------------------------------------- 2. the tables of a whole video
def _set_tables(n_frames, seed, pieces_of=None):
    """per frame of a set: table set (a few -1), side row for those, piece rows; per piece its MCUs (3 x 4 MCUs a frame)"""
    rs = np.random.RandomState(seed)
    frame_set = rs.randint(0, 3, n_frames).astype(np.int32)
    side = np.sort(rs.permutation(n_frames)[:max(n_frames // 5, 1)])
    frame_set[side] = -1
    side_row = np.full(n_frames, -1, np.int32)
    side_row[side] = np.arange(side.size)
    piece_n = np.where(frame_set >= 0, rs.randint(1, 4, n_frames) if pieces_of is None else pieces_of, 0).astype(np.int64)
    piece_lo = np.concatenate([[0], np.cumsum(piece_n)[:-1]]).astype(np.int64)
    return frame_set, side_row, piece_lo, piece_n


def _loop_tables(first, L, frame_set, side_row, piece_lo, piece_n, chunk, keep=None):
    slot_set, fill, items = np.full(L, -1, np.int32), np.full(L, -2, np.int32), []
    for t in range(L):
        f = first + t
        if side_row[f] >= 0:
            fill[t] = side_row[f]
            continue
        slot_set[t] = frame_set[f]
        for p in range(int(piece_lo[f]), int(piece_lo[f] + piece_n[f])):
            if keep is None or keep[p]:
                items.append((t // chunk, int(frame_set[f]), p, t))
    items.sort()
    waves, chunks = [], []
    i = 0
    while i < len(items):
        j = i
        while j < len(items) and items[j][:2] == items[i][:2] and j - i < 64:
            j += 1
        c = items[i][0]
        if not chunks or chunks[-1][0] != c * chunk:
            chunks.append([c * chunk, min((c + 1) * chunk, L), len(waves), len(waves)])
        waves.append((i, j - i))
        chunks[-1][3] = len(waves)
        i = j
    return slot_set, fill, np.asarray([(p, t) for _, _, p, t in items], np.int32).reshape(-1, 2), \
        np.asarray(waves, np.int32).reshape(-1, 2), [tuple(c) for c in chunks]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("chunk", [None, 4, 70])
def test_video_tables_equal_a_loop(stride, chunk):
    """two videos of 150 and 9 sampled frames in one set (the stride only changes how many frames the set holds): every
    slot is a device frame or a side frame, none is padding; a chunk smaller than the video; more than 64 items per set"""
    lens = [-(-299 // stride) if stride == 2 else 150, 9]
    n = sum(lens)
    frame_set, side_row, piece_lo, piece_n = _set_tables(n, 40 + stride)
    first = 0
    for L in lens:
        tb = TC.video_tables(first, L, frame_set, side_row, piece_lo, piece_n, chunk_slots=chunk)
        want = _loop_tables(first, L, frame_set, side_row, piece_lo, piece_n, chunk or L)
        assert tb.n_slots == L and np.array_equal(tb.slot_set, want[0]) and np.array_equal(tb.fill, want[1])
        assert not (tb.fill == -1).any() and np.all((tb.slot_set >= 0) ^ (tb.fill >= 0))
        assert np.array_equal(tb.items, want[2]) and np.array_equal(tb.waves, want[3]) and tb.chunks == want[4]
        assert tb.waves[:, 1].max() <= 64 and tb.items.shape[0] == int(piece_n[first:first + L].sum())
        first += L
    with pytest.raises(ValueError):
        TC.video_tables(0, 0, frame_set, side_row, piece_lo, piece_n)
    with pytest.raises(ValueError, match="neither decodable"):
        TC.video_tables(0, 3, np.full(3, -1, np.int32), np.full(3, -1, np.int32), piece_lo, piece_n)


@pytest.mark.parametrize("split", [1, 4], ids=["per_mcu", "per_row"])
@pytest.mark.parametrize("name", ["40x56_420_q90.jpg", "40x56_420_q75rst3.jpg"])
def test_the_mcu_row_filter_keeps_the_pieces_that_meet_the_rows(name, split):
    """40 x 56 4:2:0 is 3 x 4 MCUs; the restart file has segments of 3 MCUs, which straddle the MCU rows"""
    pk = jpegdev.pack_frames([J.data(name)] * 3, pinned=False)
    g = pk.geom
    assert (g.mcus_y, g.mcus_x) == (3, 4)
    pm = jpegdev.piece_ranges(pk.segments, split)
    cnt = jpegdev.piece_counts(pk.segments, split)
    assert pm.shape[0] == cnt.sum() and pm[:, 1].min() >= 1
    assert pm[:, 0].tolist() == [m for m0, nm in pk.segments[:, 1:3].tolist() for m in [m0] + jpegdev.split_points(m0, nm, split)]
    per_frame = pm.shape[0] // 3
    assert int(pm[:per_frame, 1].sum()) == 12                               # the pieces of a frame tile its MCUs
    frame_set = np.zeros(3, np.int32)
    side_row = np.full(3, -1, np.int32)
    fr_of_seg = pk.segments[:, 0]
    piece_n = np.bincount(np.repeat(fr_of_seg, cnt), minlength=3).astype(np.int64)
    piece_lo = np.concatenate([[0], np.cumsum(piece_n)[:-1]])
    for top, wh in ((16, 16), (17, 14), (0, 40), (0, 1), (31, 2), (15, 1), (16, 1)):
        wb = jpegdev.window_blocks(g, top, 8, wh, 16)
        tb = TC.video_tables(0, 3, frame_set, side_row, piece_lo, piece_n, piece_mcu=pm, mcus_x=g.mcus_x, mcu_rows=wb.mcu_rows)
        lo, hi = wb.mcu_rows
        want = [p for p in range(pm.shape[0])
                if any(lo <= m // g.mcus_x < hi for m in range(int(pm[p, 0]), int(pm[p, 0] + pm[p, 1])))]
        assert sorted(tb.items[:, 0].tolist()) == want, (top, wh)
        # every MCU of the rows is decoded by a listed piece
        covered = {m for p in tb.items[:, 0] for m in range(int(pm[p, 0]), int(pm[p, 0] + pm[p, 1]))}
        per = {(int(p), m) for p in tb.items[:, 0] for m in range(int(pm[p, 0]), int(pm[p, 0] + pm[p, 1]))}
        assert len(per) == 3 * len(covered) and {m for m in range(12) if lo <= m // 4 < hi} <= covered
    assert jpegdev.window_blocks(g, 17, 8, 14, 16).mcu_rows == (1, 2) and jpegdev.window_blocks(g, 16, 8, 16, 16).mcu_rows == (0, 3)
    with pytest.raises(ValueError, match="piece_mcu"):
        TC.video_tables(0, 3, frame_set, side_row, piece_lo, piece_n, mcu_rows=(0, 1))


# ----------------------------------------------------------------------------- 3. load_resident_jpegs(stride)
ENC = ["24x32_420_q90.jpg", "24x32_420_q100.jpg", "24x32_420_q30opt.jpg", "24x32_420_q75rst3.jpg"]


def _tree(root, lengths=(7, 4)):
    videos = []
    for v, n in enumerate(lengths):
        os.makedirs(os.path.join(root, f"v{v}"))
        for i in range(n):
            shutil.copy(J.fixture_path(ENC[(i + v) % 4]), os.path.join(root, f"v{v}", f"frame{i}.jpg"))
        videos.append(dict(video=f"v{v}", num_frames=n, fps=25.0 + v))
    return videos


def test_load_resident_jpegs_with_a_stride(tmp_path):
    root = str(tmp_path)
    videos = _tree(root)
    one = TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False)
    assert one.stride == 1 and one.video_len.tolist() == [7, 4] and one.video_first.tolist() == [0, 7]
    assert one.names == [os.path.join(root, f"v{v}", f"frame{i}.jpg") for v, n in enumerate((7, 4)) for i in range(n)]
    two = TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False, stride=2)
    assert two.stride == 2 and two.video_len.tolist() == [4, 2] and two.video_first.tolist() == [0, 4]
    assert two.names == [os.path.join(root, f"v{v}", f"frame{i}.jpg") for v, n in enumerate((7, 4)) for i in range(0, n, 2)]
    assert two.n_frames == 6 and two.fallback == [] and (two.frame_set >= 0).all()
    three = TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False, stride=3)
    assert three.video_len.tolist() == [3, 2]
    with pytest.raises(ValueError, match="stride"):
        TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False, stride=0)
    os.remove(os.path.join(root, "v0", "frame2.jpg"))                       # a hole on the sampled grid, and one beside it
    with pytest.raises(FileNotFoundError):
        TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False, stride=2)
    assert TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False, stride=3).video_len.tolist() == [3, 2]
    with pytest.raises(ValueError, match="num_frames"):
        TC.load_resident_jpegs(root, "soccernetball", [dict(video="v1", num_frames=5)], pinned=False, stride=2)


# ----------------------------------------------------------------------------- 4. argument errors, before any device
def test_resident_jpeg_videos_argument_errors_touch_no_device(tmp_path, monkeypatch):
    from tdeed_amd import streams
    root = str(tmp_path)
    videos = _tree(root)
    jpegs = TC.load_resident_jpegs(root, "soccernetball", videos, pinned=False, stride=2)

    def no_device(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(streams, "new_stream", no_device)
    with pytest.raises(ValueError, match="videos"):
        E.ResidentJpegVideos(videos[:1], jpegs)
    with pytest.raises(ValueError, match="stride 2"):
        E.ResidentJpegVideos([dict(videos[0], num_frames=9), videos[1]], jpegs)
    with pytest.raises(ValueError, match="larger than"):
        E.ResidentJpegVideos(videos, jpegs, crop=33)
    with pytest.raises(ValueError, match="larger than"):
        E.ResidentJpegVideos(videos, jpegs, crop=(25, 16))
    with pytest.raises(ValueError, match="positive"):
        E.ResidentJpegVideos(videos, jpegs, crop=0)
    with pytest.raises(ValueError, match="split_mcus"):
        E.ResidentJpegVideos(videos, jpegs, split_mcus=0)
    with pytest.raises(ValueError, match="max_coeff_bytes"):
        E.ResidentJpegVideos(videos, jpegs, max_coeff_bytes=0)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        E.ResidentJpegVideos(videos, jpegs, max_resident_bytes=1000)
    with pytest.raises(AssertionError, match="reached the device"):          # nothing wrong: construction goes on
        E.ResidentJpegVideos(videos, jpegs, crop=(16, 24))
    assert E._crop_window(16, 24, 32) == (4, 8, 16, 16) and E._crop_window((24, 32), 24, 32) is None


# ----------------------------------------------------------------------------- 5. the windowed band loop on the host
@pytest.fixture(scope="module")
def window_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    tmp = tmp_path_factory.mktemp("jpeg_window_check")
    exe, src = str(tmp / "jpeg_window_check"), os.path.join(ROOT, "tools", "jpeg_window_check.cpp")
    # with the address and undefined-behaviour sanitizers where the compiler has them (a stand-alone host program: a report
    # ends it with a non-zero status), plain otherwise
    san = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    r = subprocess.run(san, capture_output=True)
    if r.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 2:     # no arguments: the usage line
        subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe


@pytest.mark.parametrize("gid", ["40x56_420", "23x37_422", "17x49_444", "24x32_grey", "1x1_420"])
def test_window_check_program_over_its_grid(window_check, tmp_path, gid):
    """tools/jpeg_window_check.cpp: per window, IDCT for jc_window's blocks only, planes of exactly that width, coefficients of
    MCU rows outside the listed ones poisoned -- the window's pixels equal the whole-frame decode's and no sample is read
    that was not written"""
    pk = jpegdev.pack_frames([J.data(n) for n in J.groups()[gid]], pinned=False)
    src = str(tmp_path / "packed.bin")
    pk.save(src)
    r = subprocess.run([window_check, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n, bad, miss = (int(x) for x in (r.stdout.split()[0], r.stdout.split()[4], r.stdout.split()[6]))
    assert n >= 16 and bad == 0 and miss == 0, r.stdout
    # the dataset window on the command line
    if gid == "40x56_420":
        r = subprocess.run([window_check, src, "17", "9", "14", "31", "0", "0", "40", "56"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith(f"{2 * pk.n_frames} frame windows checked, 0 wrong"), r.stdout + r.stderr
        assert subprocess.run([window_check, src, "0", "0", "41", "56"], capture_output=True).returncode == 2
