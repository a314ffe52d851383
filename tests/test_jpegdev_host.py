"""The device JPEG decoder's host side, without a GPU: the numpy model and Pillow's recorded decode agree bit for bit,
`parse` draws the line of the supported subset, `pack` lays segments and tables out as the kernels expect them, and the
host check program (the kernels' own arithmetic, csrc/jpeg_core.h, in plain loops) reproduces coefficients and pixels
and reports damaged streams per segment without touching the frames next to them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
from helpers import ROOT
from tdeed_amd import feeder, jpegdev


# ----------------------------------------------------------------------------- 1. the model against Pillow's record
@pytest.mark.parametrize("name", J.supported_names())
def test_reference_decode_equals_the_pillow_record(name):
    ref = J.reference(name)
    want = J.expected()[name]
    assert ref.rgb.dtype == np.uint8 and ref.rgb.shape == want.shape
    assert np.array_equal(ref.rgb, want)
    g = ref.info.geom
    assert [c.shape for c in ref.coeffs] == [(g.bh[c], g.bw[c], 64) for c in range(g.ncomp)]
    assert [p.shape for p in ref.planes] == [(g.ch[c], g.cw[c]) for c in range(g.ncomp)]
    assert ref.flat.dtype == np.int16 and ref.flat.size == g.frame_blocks * 64


def test_record_count():
    assert len(J.supported_names()) == 85 + 3 + 28 and len(J.expected()) == 90 + 28


def test_installed_pillow_still_decodes_as_recorded():
    """expected.npz was written by one Pillow / libjpeg-turbo build; if the installed one decodes differently, this test
    fails and the decoder tests above say nothing about the decoder."""
    for name, want in J.expected().items():
        assert np.array_equal(feeder.read_frame(J.fixture_path(name)).numpy(), want), name


# ----------------------------------------------------------------------------- 2. parse
def test_parse_rejects_what_the_kernels_do_not_decode():
    for name in J.UNSUPPORTED:
        assert jpegdev.parse(J.data(name)) is None, name
    assert jpegdev.parse(b"") is None and jpegdev.parse(b"\xff\xd8\xff\xd9") is None and jpegdev.parse(b"not a jpeg at all") is None
    good = J.data("24x32_420_q90.jpg")
    sof = good.index(b"\xff\xc0")
    assert jpegdev.parse(good[:sof + 1] + b"\xc2" + good[sof + 2:]) is None                   # progressive marker
    assert jpegdev.parse(good[:sof + 4] + b"\x0c" + good[sof + 5:]) is None                   # 12-bit samples
    assert jpegdev.parse(good[:sof]) is None                                                 # cut inside the headers


def test_parse_reports_geometry_sampling_and_segments():
    samp = {"444": jpegdev.S444, "422": jpegdev.S422, "420": jpegdev.S420}
    for (h, w) in J.SIZES:
        for s in J.SAMPLINGS:
            for e in J.ENCODINGS:
                info = jpegdev.parse(J.data(f"{h}x{w}_{s}_{e}.jpg"))
                assert info is not None and (info.height, info.width, info.samp, info.ncomp) == (h, w, samp[s], 3)
                hs, vs = (2 if s != "444" else 1), (2 if s == "420" else 1)
                mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
                assert info.mcus == mcus
                ri = 3 if e == "q75rst3" else 0
                assert info.restart_interval == ri
                assert info.n_segments == (-(-mcus // 3) if ri else 1) == len(info.seg_start) == len(info.seg_len)
                d = J.data(f"{h}x{w}_{s}_{e}.jpg")
                assert d[info.scan_end:info.scan_end + 2] == b"\xff\xd9"
                assert info.seg_start[0] == info.scan_start and info.seg_start[-1] + info.seg_len[-1] == info.scan_end
                for a, n in zip(info.seg_start[1:], info.seg_len[:-1]):                        # RSTn between the segments
                    assert d[a - 2] == 0xFF and 0xD0 <= d[a - 1] <= 0xD7
    info = jpegdev.parse(J.data(J.GREY))
    assert (info.height, info.width, info.samp, info.ncomp, info.mcus) == (24, 32, jpegdev.GREY, 1, 12)
    info = jpegdev.parse(np.frombuffer(J.data(J.WIDE[0]), np.uint8))                            # arrays as well as bytes
    assert (info.height, info.width, info.samp, info.mcus) == (224, 398, jpegdev.S420, 25 * 14)
    for name in J.supported_names():
        assert jpegdev.parse(J.data(name)) is not None, name


# ----------------------------------------------------------------------------- 3. pack
def _check_layout(pk):
    seg = pk.segments
    assert seg.dtype == np.int32 and seg.shape == (pk.n_segments, 6)
    assert np.all(np.diff(seg[:, 5]) >= 0)                                                      # a set's segments are contiguous
    assert np.all(seg[:, 3] % 4 == 0)
    order = np.argsort(seg[:, 3])
    ends = seg[order, 3] + seg[order, 4]
    nxt = np.concatenate([seg[order, 3][1:], [pk.stream_np.size]])
    assert np.all(nxt - ends >= 8)                                                              # guard bytes ...
    for a, b in zip(ends, nxt):
        assert not pk.stream_np[a:b].any()                                                      # ... that are zero
    assert pk.table_sets.shape == (pk.n_sets, jpegdev.TABLE_SET_BYTES) and pk.table_sets.dtype == np.uint8
    for lo, n in pk.waves():
        assert 1 <= n <= 64 and len(set(seg[lo:lo + n, 5])) == 1
    assert sorted(r for lo, n in pk.waves() for r in range(lo, lo + n)) == list(range(pk.n_segments))


def test_pack_shares_table_sets_and_lays_segments_out():
    pk = jpegdev.pack([J.data(n) for n in J.WIDE])                                              # one encoder: one set
    assert (pk.n_sets, pk.n_segments, pk.n_frames) == (1, 3, 3) and pk.frame_set.tolist() == [0, 0, 0] and pk.fallback == []
    _check_layout(pk)
    assert pk.waves().tolist() == [[0, 3]]
    for j, n in enumerate(J.WIDE):
        info = jpegdev.parse(J.data(n))
        f, m0, nm, off, ln, sid = pk.segments[j]
        assert (f, m0, nm, ln, sid) == (j, 0, info.mcus, info.scan_end - info.scan_start, 0)
        assert pk.stream_np[off:off + ln].tobytes() == J.data(n)[info.scan_start:info.scan_end]
    for gid, names in J.groups().items():
        pk = jpegdev.pack([J.data(n) for n in names])
        _check_layout(pk)
        infos = [jpegdev.parse(J.data(n)) for n in names]
        assert pk.n_segments == sum(i.n_segments for i in infos), gid
        assert pk.n_sets == len({i.tables_key for i in infos}), gid
    # the same file twice shares its set; frames 0 and 2 of a pack of (a, b, a) too
    a, b = J.data("40x56_420_q90.jpg"), J.data("40x56_420_q75rst3.jpg")
    pk = jpegdev.pack([a, b, a])
    assert pk.n_sets == 2 and pk.frame_set.tolist() == [0, 1, 0]
    assert pk.segments[:, 0].tolist() == [0, 2] + [1] * 4 and pk.segments[2:, 1].tolist() == [0, 3, 6, 9]
    assert pk.segments[2:, 2].tolist() == [3, 3, 3, 3]                                           # 12 MCUs, interval 3
    _check_layout(pk)
    assert pk.waves(1, 2).tolist() == [[2, 4]] and pk.waves(0, 1).tolist() == [[0, 1]] and pk.waves(2, 3).tolist() == [[1, 1]]
    pk = jpegdev.pack([J.data("17x49_420_q75rst3.jpg")])                                        # 4 x 2 MCUs: 3 + 3 + 2
    assert pk.segments[:, 2].tolist() == [3, 3, 2]


def test_pack_fallback_and_geometry():
    a = J.data("24x32_420_q90.jpg")
    pk = jpegdev.pack([J.data(J.UNSUPPORTED[0]), a, J.data(J.UNSUPPORTED[1]), J.data("24x32_444_q90.jpg"), a])
    assert pk.fallback == [0, 2, 3] and pk.frame_set.tolist() == [-1, 0, -1, -1, 0]            # another sampling: fallback
    assert (pk.height, pk.width, pk.samp) == (24, 32, jpegdev.S420)
    with pytest.raises(ValueError, match="does not fit"):
        jpegdev.pack([a, J.data("23x37_420_q90.jpg")])
    pk = jpegdev.pack([J.data(n) for n in J.UNSUPPORTED])
    assert pk.n_segments == 0 and pk.fallback == [0, 1]


# ----------------------------------------------------------------------------- 4. the host check program
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("jpeg_host_check") / "jpeg_host_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "jpeg_host_check.cpp")], check=True)

    def run(packed, tmp):
        src, dst = str(tmp / "packed.bin"), str(tmp / "out.bin")
        packed.save(src)
        subprocess.run([exe, src, dst], check=True, capture_output=True)
        return J.read_host_check_output(dst, packed)
    return run


@pytest.mark.parametrize("gid", list(J.groups()))
def test_host_check_program_equals_model_and_pillow(host_check, tmp_path, gid):
    names = J.groups()[gid]
    pk = jpegdev.pack([J.data(n) for n in names])
    coef, status, rgb = host_check(pk, tmp_path)
    assert not status.any()
    for j, n in enumerate(names):
        assert np.array_equal(coef[j], J.reference(n).flat), n
        assert np.array_equal(rgb[j], J.expected()[n]), n


def test_host_check_program_on_the_dataset_frames(host_check, tmp_path):
    by_dir = {}
    for n in J.supported_names():
        if n.startswith("frames/"):
            by_dir.setdefault(os.path.dirname(n), []).append(n)
    assert len(by_dir) == 4
    for names in by_dir.values():
        pk = jpegdev.pack([J.data(n) for n in names])
        coef, status, rgb = host_check(pk, tmp_path)
        assert not status.any() and pk.n_sets == 1
        for j, n in enumerate(names):
            assert np.array_equal(coef[j], J.reference(n).flat) and np.array_equal(rgb[j], J.expected()[n]), n


# ----------------------------------------------------------------------------- 5. damaged streams
def damaged_pack():
    """Seven 40x56 4:2:0 frames: 0 intact, 1 cut short, 2 with a restart marker written over two bytes of a file that has
    no restart interval, 3 and 6 a restart file with one byte of its third segment overwritten, 4 with the symbols of its
    own DC luma Huffman table clobbered, 5 intact.  An overwritten byte desynchronises the Huffman stream; many values
    still decode to the end of the segment (wrong coefficients, no error -- in libjpeg as well), so the two used here are
    ones after which the stream runs into a zero run past coefficient 63 (frame 3) and into a 16-bit window that is no
    code (frame 6).  -> (files, names of the intact originals, {frame: expected status})."""
    q90, q30, q100, rst = (J.data(f"40x56_420_{e}.jpg") for e in J.ENCODINGS)
    i90, i100, irst = jpegdev.parse(q90), jpegdev.parse(q100), jpegdev.parse(rst)
    cut = q90[:i90.scan_start + (i90.scan_end - i90.scan_start) * 6 // 10]
    mid = (i100.scan_start + i100.scan_end) // 2
    marked = q100[:mid] + b"\xff\xd3" + q100[mid + 2:]
    hits = []
    for off, val in ((11, 0x00), (19, 0xFE)):
        pos = int(irst.seg_start[2]) + off
        hits.append(rst[:pos] + bytes([val]) + rst[pos + 1:])
    dht = q30.index(b"\xff\xc4")
    assert q30[dht + 4] == 0x00                                                # table class 0 (DC), id 0
    nvals = sum(q30[dht + 5:dht + 21])
    clobbered = q30[:dht + 21] + b"\x0f" * nvals + q30[dht + 21 + nvals:]
    files = [q90, cut, marked, hits[0], clobbered, q100, hits[1]]
    return files, {0: "40x56_420_q90.jpg", 5: "40x56_420_q100.jpg"}, {1: 1, 2: 2, 3: 6, 4: 4, 6: 3}


def test_damaged_streams_are_reported_per_segment_and_leave_their_neighbours_alone(host_check, tmp_path):
    files, intact, want = damaged_pack()
    pk = jpegdev.pack(files)
    assert pk.fallback == [] and pk.n_frames == 7
    coef, status, rgb = host_check(pk, tmp_path)
    frame = pk.segments[:, 0]
    for f, name in intact.items():
        assert not status[frame == f].any()
        assert np.array_equal(rgb[f], J.expected()[name]) and np.array_equal(coef[f], J.reference(name).flat)
    for f, code in want.items():
        st = status[frame == f]
        if f in (3, 6):                                                            # only the hit restart interval
            assert st.tolist() == [0, 0, code, 0], (f, st)
            ref = J.reference("40x56_420_q75rst3.jpg")
            g = pk.geom
            ok = np.ones(g.frame_blocks, bool)                                      # blocks of MCUs 6, 7, 8 may differ
            for m in (6, 7, 8):
                my, mx = divmod(m, g.mcus_x)
                for v in range(2):
                    for h in range(2):
                        ok[(my * 2 + v) * g.bw[0] + mx * 2 + h] = False
                for c in (1, 2):
                    ok[g.boff[c] + my * g.mcus_x + mx] = False
            assert np.array_equal(coef[f].reshape(-1, 64)[ok], ref.flat.reshape(-1, 64)[ok])
        else:
            assert st.size == 1 and st[0] == code, (f, st)


def test_entry_points_check_their_arguments_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd._lib import call, HipCallError, load
    assert load().tdeed_jpeg_frame_coeffs(224, 224, 3) == (28 * 28 + 2 * 14 * 14) * 64
    assert load().tdeed_jpeg_frame_coeffs(1, 1, 0) == 64 and load().tdeed_jpeg_frame_coeffs(0, 1, 0) == -1
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_jpeg_entropy", None, 8, None, 1, None, 1, None, 1, 8, 8, 3, 0, 1, None, None, None)
    with pytest.raises(HipCallError, match="sampling"):
        call("tdeed_jpeg_entropy", 1 << 20, 8, 1 << 20, 1, 1 << 20, 1, 1 << 20, 1, 8, 8, 4, 0, 1, 1 << 20, 1 << 20, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_jpeg_pixels", None, None, None, 1, None, 0, 1, 8, 8, 3, None)
    with pytest.raises(HipCallError, match="LDS"):
        call("tdeed_jpeg_pixels", 1 << 20, 1 << 20, 1 << 20, 1, 1 << 20, 0, 1, 8, 4096, 3, None)


# ----------------------------------------------------------------------------- 6. the decode keyword of the video routes
def test_decode_keyword_selects_the_loader(monkeypatch):
    import torch
    from tdeed_amd import evalutil as E

    class Model:
        def predict_video(self, frames, **kw):
            return np.zeros((int(frames.shape[0]), 4), np.float32), np.ones(int(frames.shape[0]), np.int32)

        def predict_video_group(self, frames_list, **kw):               # what stitch_videos calls: a video is a group of one
            return [self.predict_video(f, **kw) for f in frames_list]

    base = os.path.join(ROOT, "tests", "golden", "frames", "soccernetball")
    src = dict(frame_dir=base, dataset="soccernetball", video_name="game_a/clip_1", num_frames=7)
    called = []
    real = feeder.load_video
    monkeypatch.setattr(feeder, "load_video", lambda *a, **kw: (called.append("host"), real(*a, **kw))[1])
    monkeypatch.setattr(feeder, "load_video_device",
                        lambda *a, **kw: (called.append("device"), real(*a, **{k: v for k, v in kw.items()}))[1])
    st = E.stitch_videos(Model(), [("v", 7, 25.0, src)], 4)
    assert called == ["host"] and st.tracks["v"][1].tolist() == [1] * 7
    E.stitch_videos(Model(), [("v", 7, 25.0, src)], 4, decode="device")
    E.stitch_videos(Model(), [("v", 7, 25.0, src), ("w", 7, 25.0, src)], 4, decode="device", group_videos=1)
    assert called == ["host", "device", "device", "device"]
    E.stitch_videos(Model(), [("v", 7, 25.0, torch.zeros((7, 3, 4, 4), dtype=torch.uint8))], 4, decode="device")   # tensors pass
    assert len(called) == 4
    for fn in (lambda: E.stitch_videos(Model(), [("v", 7, 25.0, src)], 4, decode="gpu"),
               lambda: E.spot_videos(Model(), [("v", 7, 25.0, src)], {"a": 1}, [("nms", 1, 0.01)], decode="gpu")):
        with pytest.raises(ValueError, match="decode"):
            fn()
