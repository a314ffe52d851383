"""Resident JPEG streams without a GPU: the split rule, the per-batch table builder of `trainclips.ResidentJpegClips`, the
host object of `trainclips.load_resident_jpegs` (mixed files, shards), and tools/jpeg_split_check.cpp -- the decode of every
piece on its own from the recorded decoder states (csrc/jpeg_core.h) against the whole-segment decode, bit for bit."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import jpeg_cases as J
from helpers import ROOT
from tdeed_amd import jpegdev
from tdeed_amd import trainclips as TC

ENC = ["24x32_420_q90.jpg", "24x32_420_q100.jpg", "24x32_420_q30opt.jpg", "24x32_420_q75rst3.jpg"]
OTHER = ["24x32_444_q90.jpg", "24x32_grey_q90.jpg", "24x32_cmyk.jpg", "24x32_progressive.jpg"]


# ----------------------------------------------------------------------------- 1. the split rule
def _pieces(pk, split):
    return int(jpegdev.piece_counts(pk.segments, split).sum())


def test_split_rule_counts():
    assert jpegdev.split_points(0, 4, 2) == [2] and jpegdev.split_points(0, 4, 1) == [1, 2, 3]
    assert jpegdev.split_points(3, 1, 1) == [] and jpegdev.split_points(3, 3, 4) == [4] and jpegdev.split_points(4, 4, 4) == []
    assert jpegdev.split_points(0, 1, 1) == [] and jpegdev.split_points(5, 7, 3) == [6, 9]
    with pytest.raises(ValueError):
        jpegdev.split_points(0, 4, 0)
    pk = jpegdev.pack([J.data(n) for n in ENC])
    assert pk.geom.mcus_x == 2
    assert sorted(map(tuple, pk.segments[:, 1:3].tolist())) == [(0, 3), (0, 4), (0, 4), (0, 4), (3, 1)]
    assert _pieces(pk, pk.geom.mcus_x) == 9 and _pieces(pk, 1) == 16
    pk = jpegdev.pack([J.data("40x56_420_q75rst3.jpg")])
    assert (pk.geom.mcus_x, pk.geom.mcus_y) == (4, 3) and pk.segments[:, 1:3].tolist() == [[0, 3], [3, 3], [6, 3], [9, 3]]
    assert _pieces(pk, 4) == 6 and _pieces(pk, 1) == 12
    pk = jpegdev.pack([J.data("1x1_420_q90.jpg")])
    assert _pieces(pk, pk.geom.mcus_x) == 1 and _pieces(pk, 1) == 1
    # the vectorised count is the list's length for every row shape
    for first in range(0, 9):
        for n in range(1, 9):
            for split in range(1, 6):
                seg = np.array([[0, first, n, 0, 0, 0]], np.int32)
                assert jpegdev.piece_counts(seg, split)[0] == len(jpegdev.split_points(first, n, split)) + 1


def test_piece_row_layout():
    assert jpegdev.PIECE.itemsize == jpegdev.PIECE_BYTES == 72
    assert [jpegdev.PIECE.fields[k][1] for k in ("pos", "segment", "first_mcu", "n_mcu", "set", "left", "st")] == \
        [0, 8, 12, 16, 20, 24, 32]
    st = jpegdev.PIECE.fields["st"][0]
    assert [st.fields[k][1] for k in ("bits", "byte_off", "n", "pad", "marker", "pred")] == [0, 8, 12, 16, 20, 24]
    src = open(os.path.join(ROOT, "t-deed_amd", "csrc", "jpeg_core.h")).read()
    assert "#define JC_PIECE_BYTES 72" in src


# ----------------------------------------------------------------------------- 2. the per-batch tables
def _frame_tables():
    """two videos of 10 and 8 frames; frames 3 and 12 kept decoded, three table sets, frame 5 in 70 pieces"""
    n = 18
    frame_set = (np.arange(n) % 3).astype(np.int32)
    side_row = np.full(n, -1, np.int32)
    side_row[[3, 12]] = [0, 1]
    frame_set[[3, 12]] = -1
    piece_n = 1 + np.arange(n) % 4
    piece_n[5] = 70
    piece_n[[3, 12]] = 0
    piece_lo = np.concatenate([[0], np.cumsum(piece_n)[:-1]])
    return frame_set, side_row, piece_lo.astype(np.int64), piece_n.astype(np.int64)


def _brute(rows, T, stride, frame_set, side_row, piece_lo, piece_n):
    slot_set, fill, items = [], [], set()
    for k in range(rows.shape[1]):
        first, base, nfr = (int(rows[i, k]) for i in range(3))
        for t in range(T):
            f = base + t * stride
            s = k * T + t
            if not 0 <= f < nfr:
                slot_set.append(-1)
                fill.append(-1)
            elif side_row[first + f] >= 0:
                slot_set.append(-1)
                fill.append(int(side_row[first + f]))
            else:
                slot_set.append(int(frame_set[first + f]))
                fill.append(-2)
                items |= {(int(piece_lo[first + f]) + i, s) for i in range(int(piece_n[first + f]))}
    return slot_set, fill, items


@pytest.mark.parametrize("stride", [1, 2])
def test_batch_tables(stride):
    frame_set, side_row, piece_lo, piece_n = _frame_tables()
    T = 6
    # clips: before frame 0 of video 0, past the end of video 0 (the overhang would land in video 1), inside video 1 over its
    # side frame, past the end of video 1, wholly outside
    rows = np.array([[0, 0, 10, 10, 10], [-2, 5, 0, 5, -40], [10, 10, 8, 8, 8], [0, 0, 1, 1, 1]], np.int64)
    tb = TC.batch_tables(rows, T, stride, frame_set, side_row, piece_lo, piece_n)
    slot_set, fill, items = _brute(rows, T, stride, frame_set, side_row, piece_lo, piece_n)
    assert tb.n_slots == 30 and tb.slot_set.dtype == tb.fill.dtype == tb.items.dtype == tb.waves.dtype == np.int32
    assert tb.slot_set.tolist() == slot_set and tb.fill.tolist() == fill
    # the padding of ops.train_clip_gather: base + t * stride outside [0, num_frames) is a zero frame
    assert fill[:6] == ([-1, -1, -2, -2, -2, 0] if stride == 1 else [-1, -2, -2, -2, -2, -2])
    assert fill[6:12] == ([-2, -2, -2, -2, -2, -1] if stride == 1 else [-2, -2, -2, -1, -1, -1])
    assert all(v == -1 for v in fill[24:]) and all(v == -1 for v in slot_set[24:])
    assert [(s, r) for s, r in enumerate(fill) if r >= 0] == ([(5, 0), (14, 1)] if stride == 1 else [(13, 1)])   # exact pairs
    assert all((f == -1) <= (s == -1) for f, s in zip(fill, slot_set))          # padding slots carry set -1
    got = list(map(tuple, tb.items.tolist()))
    assert len(got) == len(set(got)) == len(items) and set(got) == items
    set_of_slot = np.asarray(slot_set)
    item_sets = set_of_slot[tb.items[:, 1]]
    assert np.all(np.diff(item_sets) >= 0)                                       # grouped by table set
    covered = []
    for lo, n in tb.waves.tolist():
        assert 1 <= n <= 64 and len(set(item_sets[lo:lo + n].tolist())) == 1     # no wave spans two sets or exceeds 64
        covered += range(lo, lo + n)
    assert covered == list(range(len(got)))
    assert tb.chunks == [(0, 30, 0, tb.waves.shape[0])]
    assert any(n == 64 for _, n in tb.waves.tolist())                            # frame 5's 70 pieces fill a wave


def test_batch_tables_chunks_and_clip_slots():
    frame_set, side_row, piece_lo, piece_n = _frame_tables()
    T = 4
    rows = np.array([[0, 10], [4, 2], [10, 8]], np.int64)
    tb = TC.batch_tables(rows, T, 1, frame_set, side_row, piece_lo, piece_n, n_slots=16, clip_slot=[0, 8], chunk_slots=3)
    assert tb.fill.tolist() == [-2] * 4 + [-2] * 4 + [1, -2, -2, -2] + [-2] * 4                  # slots 4..7, 12..15: unused
    assert tb.slot_set[4:8].tolist() == [-1] * 4 and tb.slot_set[12:].tolist() == [-1] * 4 and tb.slot_set[8] == -1
    chunk_of_item = tb.items[:, 1] // 3
    assert np.all(np.diff(chunk_of_item) >= 0)
    seen = []
    for lo, hi, w_lo, w_hi in tb.chunks:
        assert hi - lo <= 3 and lo % 3 == 0 and w_hi > w_lo
        for a, n in tb.waves[w_lo:w_hi].tolist():
            assert np.all((tb.items[a:a + n, 1] >= lo) & (tb.items[a:a + n, 1] < hi))
            assert len(set(tb.slot_set[tb.items[a:a + n, 1]].tolist())) == 1
            seen += range(a, a + n)
    assert seen == list(range(tb.items.shape[0])) and [c[0] for c in tb.chunks] == [0, 3, 9]    # 6..8: unused and side slots
    with pytest.raises(ValueError, match="slots"):
        TC.batch_tables(rows, T, 1, frame_set, side_row, piece_lo, piece_n, n_slots=16, clip_slot=[0, 2])
    lost = frame_set.copy()
    lost[4] = -1
    with pytest.raises(ValueError, match="neither"):
        TC.batch_tables(rows, T, 1, lost, side_row, piece_lo, piece_n)


# ----------------------------------------------------------------------------- 3. the loader's host object
def _tree(root, video, files):
    os.makedirs(os.path.join(root, video))
    for n, name in enumerate(files):
        shutil.copy(J.fixture_path(name), os.path.join(root, video, f"frame{n}.jpg"))
    return dict(video=video, num_frames=len(files), events=[])


def test_mixed_files_pack_and_load(tmp_path):
    pk = jpegdev.pack_frames([J.data(n) for n in ENC + OTHER])
    assert pk.fallback == [4, 5, 6, 7] and pk.n_sets == 4 and pk.n_segments == 5
    root = str(tmp_path)
    videos = [_tree(root, "va", ENC + OTHER)]
    cache = jpegdev.ParseCache()
    rj = TC.load_resident_jpegs(root, "soccernetball", videos, cache=cache)
    assert rj.fallback == [4, 5, 6, 7] and rj.n_sets == 4 and rj.n_segments == 5 and len(rj.shards) == 1
    assert rj.frame_set.tolist() == [0, 1, 2, 3, -1, -1, -1, -1] and (rj.height, rj.width, rj.samp) == (24, 32, jpegdev.S420)
    assert rj.video_first.tolist() == [0] and rj.video_len.tolist() == [8] and rj.n_frames == 8
    assert rj.names == [os.path.join(root, "va", f"frame{n}.jpg") for n in range(8)]
    assert np.array_equal(rj.table_sets, pk.table_sets) and np.array_equal(rj.shards[0].packed.segments, pk.segments)
    assert len(cache) == 8
    # missing files: the rules of load_resident_videos
    with pytest.raises(ValueError, match="num_frames"):
        TC.load_resident_jpegs(root, "soccernetball", [dict(videos[0], num_frames=9)])
    os.remove(os.path.join(root, "va", "frame2.jpg"))
    with pytest.raises(FileNotFoundError):
        TC.load_resident_jpegs(root, "soccernetball", videos)
    other = [_tree(root, "vb", [ENC[0], "23x37_420_q90.jpg"])]
    with pytest.raises(ValueError, match="does not fit"):
        TC.load_resident_jpegs(root, "soccernetball", other)


def test_shards_keep_one_numbering(tmp_path):
    root = str(tmp_path)
    files = [ENC[n % 4] for n in range(10)]
    videos = [_tree(root, "va", files), _tree(root, "vb", [ENC[(n + 1) % 4] for n in range(8)])]
    lens = [jpegdev.parse(J.data(n)).scan_end - jpegdev.parse(J.data(n)).scan_start for n in ENC[:3]]
    assert lens == [407, 1075, 82] and int(jpegdev.parse(J.data(ENC[3])).seg_len.sum()) + 2 == 220 + 2
    one = TC.load_resident_jpegs(root, "soccernetball", videos)
    rj = TC.load_resident_jpegs(root, "soccernetball", videos, shard_bytes=1024)
    assert len(one.shards) == 1 and len(rj.shards) >= 2 and rj.n_segments == one.n_segments == 18 + 4
    assert rj.n_sets == 4 and np.array_equal(rj.frame_set, one.frame_set) and rj.video_first.tolist() == [0, 10]
    assert np.concatenate([s.frames for s in rj.shards]).tolist() == list(range(18))
    base, pos = 0, []
    for s in rj.shards:
        pk = s.packed
        assert pk.stream_np.size <= 1024 or pk.n_frames == 1
        assert np.array_equal(pk.frame_set, rj.frame_set[s.frames])                 # the sets of the whole list
        for f, m0, nm, off, ln, sid in pk.segments.tolist():
            assert sid == rj.frame_set[s.frames[f]]
            pos.append(base + off)                                                  # absolute position of the row's first piece
        base += (pk.stream_np.size + 15) & ~15
    assert all(b > a for a, b in zip(pos, pos[1:]))                                 # absolute and increasing
    with pytest.raises(ValueError, match="shard_bytes"):
        TC.load_resident_jpegs(root, "soccernetball", videos, shard_bytes=1 << 31)


# ----------------------------------------------------------------------------- 4. the split check program
def _compile(tmp, name):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp / name)
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", name + ".cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_split_check")
    return _compile(tmp, "jpeg_split_check"), _compile(tmp, "jpeg_host_check"), tmp


def read_split_check_output(path, pk):
    fc, nf, ns = pk.geom.frame_blocks * 64, pk.n_frames, pk.n_segments
    raw = open(path, "rb").read()
    n_pieces = int(np.frombuffer(raw, np.int32, 1)[0])
    assert len(raw) == 4 + 2 * (2 * fc * nf) + 4 * (3 * ns + n_pieces + 1) + jpegdev.PIECE_BYTES * n_pieces
    o = 4
    whole = np.frombuffer(raw, np.int16, fc * nf, o).reshape(nf, fc)
    o += 2 * fc * nf
    status = np.frombuffer(raw, np.int32, ns, o)
    o += 4 * ns
    joined = np.frombuffer(raw, np.int16, fc * nf, o).reshape(nf, fc)
    o += 2 * fc * nf
    piece_status = np.frombuffer(raw, np.int32, n_pieces, o)
    o += 4 * n_pieces
    per_seg = np.frombuffer(raw, np.int32, ns, o)
    o += 4 * ns
    index_status = np.frombuffer(raw, np.int32, ns, o)
    overlaps = int(np.frombuffer(raw, np.int32, 1, o + 4 * ns)[0])
    rows = np.frombuffer(raw, jpegdev.PIECE, n_pieces, o + 4 * ns + 4)
    return SimpleNamespace(rows=rows, whole=whole, status=status, joined=joined, piece_status=piece_status, per_seg=per_seg,
                           index_status=index_status, overlaps=overlaps)


def _run_split(programs, pk, split, tag):
    exe, _, tmp = programs
    src, dst = str(tmp / f"{tag}.bin"), str(tmp / f"{tag}.out")
    pk.save(src)
    subprocess.run([exe, src, str(split), dst], check=True, capture_output=True, timeout=60)
    return read_split_check_output(dst, pk)


def test_pieces_join_to_the_whole_segment_decode_on_every_supported_fixture(programs):
    """every supported fixture, alone in its pack, split per MCU and per MCU row: the pieces, each decoded on its own from
    its recorded state into a fresh zero buffer, give the whole-segment coefficients bit for bit, with zero statuses"""
    pad_seen = {}
    for name in J.supported_names():
        pk = jpegdev.pack([J.data(name)])
        assert pk.fallback == [], name
        for split in (1, pk.geom.mcus_x):
            r = _run_split(programs, pk, split, "ok")
            want = jpegdev.piece_counts(pk.segments, split)
            assert r.per_seg.tolist() == want.tolist(), (name, split)
            assert not r.status.any() and not r.index_status.any() and not r.piece_status.any(), (name, split)
            assert np.array_equal(r.whole[0], J.reference(name).flat), name
            assert np.array_equal(r.joined, r.whole) and r.overlaps == 0, (name, split)
            rows = r.rows
            assert rows["first_mcu"].tolist() == [m for _, m0, nm, *_ in pk.segments.tolist()
                                                  for m in [m0] + jpegdev.split_points(m0, nm, split)], (name, split)
            seg = pk.segments[rows["segment"]]
            assert np.all(rows["pos"] == seg[:, 3] + rows["st"]["byte_off"]) and np.all(rows["left"] == seg[:, 4] - rows["st"]["byte_off"])
            assert np.all((0 <= rows["st"]["pad"]) & (rows["st"]["pad"] <= rows["st"]["n"]) & (rows["st"]["n"] <= 63))
            pad_seen[(name, split)] = int(rows["st"]["pad"].max())
    # why pad is part of the state: split per MCU, these files have a boundary inside the last four bytes of a segment,
    # where jc_refill has already fed zero bytes (the 82-byte scan of 24x32_420_q30opt has none: its last MCU is longer)
    assert {n for (n, split), pad in pad_seen.items() if pad > 0 and split == 1} >= \
        {"17x49_444_q30opt.jpg", "17x49_422_q30opt.jpg", "17x49_420_q30opt.jpg", "17x49_444_q75rst3.jpg", "17x49_422_q75rst3.jpg"}


def test_truncated_copies_terminate_with_the_host_checks_statuses(programs):
    exe, host, tmp = programs
    for name in J.supported_names():
        data = J.data(name)
        info = jpegdev.parse(data)
        for cut in (info.scan_start + (info.scan_end - info.scan_start) // 2, info.scan_end - 1):
            pk = jpegdev.pack([data[:cut]])
            if pk.fallback:
                continue
            src, dst = str(tmp / "cut.bin"), str(tmp / "cut.host")
            pk.save(src)
            subprocess.run([host, src, dst], check=True, capture_output=True, timeout=60)
            _, want, _ = J.read_host_check_output(dst, pk)
            for split in (1, pk.geom.mcus_x):
                r = _run_split(programs, pk, split, "cut")                       # terminates (timeout) and exits 0
                assert r.status.tolist() == want.tolist() == r.index_status.tolist(), (name, cut, split)
                good = r.status == 0
                assert r.per_seg[good].tolist() == jpegdev.piece_counts(pk.segments, split)[good].tolist()
