"""Host side of the device-decoded clip feed (feeder.device_clip_batches): `jpegdev.pack_frames` over the frames of several
videos, `jpegdev.ParseCache`, and the row table of a batch (`feeder.clip_batch_rows`).  No GPU."""
import os
import shutil

import numpy as np
import pytest

import jpeg_cases as J
from tdeed_amd import feeder, jpegdev

ENC = ["24x32_420_q90.jpg", "24x32_420_q100.jpg", "24x32_420_q30opt.jpg", "24x32_420_q75rst3.jpg"]
FIELDS = ("width", "height", "samp", "n_frames", "fallback")
ARRAYS = ("stream_np", "segments", "table_sets", "frame_set")


def _same_pack(a, b):
    for k in FIELDS:
        assert getattr(a, k) == getattr(b, k), k
    for k in ARRAYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), k
    assert type(a.stream) is type(b.stream) and np.array_equal(np.asarray(a.stream), np.asarray(b.stream))
    assert (a.geom is None) == (b.geom is None) and (a.geom is None or vars(a.geom) == vars(b.geom))
    assert np.array_equal(a.waves(), b.waves())


@pytest.mark.parametrize("names", [ENC, ENC[:1] + J.UNSUPPORTED + ENC[3:], [J.GREY] + ENC[:2], list(J.UNSUPPORTED), list(J.WIDE)],
                         ids=["four_sets", "unsupported_inside", "grey_first", "nothing_supported", "wide"])
def test_pack_is_pack_frames_with_and_without_infos(names):
    datas = [J.data(n) for n in names]
    a = jpegdev.pack(datas, pinned=False)
    _same_pack(a, jpegdev.pack_frames(datas, pinned=False))
    _same_pack(a, jpegdev.pack_frames(datas, [jpegdev.parse(d) for d in datas], pinned=False))
    cache = jpegdev.ParseCache()
    infos = [cache.lookup(n, len(d), 0, d) for n, d in zip(names, datas)]
    _same_pack(a, jpegdev.pack_frames(datas, infos, pinned=False))          # cached entries carry the built table set
    with pytest.raises(ValueError, match="infos"):
        jpegdev.pack_frames(datas, infos[:-1], pinned=False)


def test_pack_frames_rules():
    with pytest.raises(ValueError, match="does not fit"):
        jpegdev.pack_frames([J.data(ENC[0]), J.data("23x37_420_q90.jpg")], pinned=False)
    pk = jpegdev.pack_frames([J.data(ENC[0]), J.data("24x32_422_q90.jpg"), J.data(ENC[1])], pinned=False)
    assert pk.fallback == [1] and pk.frame_set.tolist() == [0, -1, 1] and pk.samp == jpegdev.S420


def test_pack_over_the_frames_of_three_videos():
    videos = [[ENC[0], ENC[1]], [ENC[2], ENC[3], ENC[0]], [ENC[3], ENC[1], ENC[2]]]
    names = [n for v in videos for n in v]
    datas = [J.data(n) for n in names]
    infos = [jpegdev.parse(d) for d in datas]
    pk = jpegdev.pack_frames(datas, pinned=False)
    assert (pk.height, pk.width, pk.samp, pk.n_frames, pk.fallback) == (24, 32, jpegdev.S420, 8, [])
    assert pk.n_sets == 4
    order = []                                                                 # table sets in order of first appearance
    for i in infos:
        if i.tables_key not in order:
            order.append(i.tables_key)
    assert pk.frame_set.tolist() == [order.index(i.tables_key) for i in infos]
    for f, i in enumerate(infos):
        assert np.array_equal(pk.table_sets[pk.frame_set[f]], jpegdev.table_set(i))
    assert infos[3].restart_interval == 3 and infos[3].n_segments > 1          # one of the sets has restart intervals
    want = []
    for f, i in enumerate(infos):
        ri = i.restart_interval or i.mcus
        for s in range(i.n_segments):
            want.append((int(pk.frame_set[f]), f, s * ri, min(ri, i.mcus - s * ri), int(i.seg_start[s]), int(i.seg_len[s])))
    want.sort(key=lambda r: r[:3])
    assert pk.n_segments == len(want) == sum(i.n_segments for i in infos)
    end = 0
    for row, (sid, f, m0, nm, src, ln) in zip(pk.segments.tolist(), want):
        assert (row[0], row[1], row[2], row[4], row[5]) == (f, m0, nm, ln, sid)
        off = row[3]
        assert off % 4 == 0 and off >= end                                     # aligned, in table order, not overlapping
        assert pk.stream_np[off:off + ln].tobytes() == datas[f][src:src + ln]
        assert not pk.stream_np[off + ln:off + ln + jpegdev.GUARD].any()
        end = off + ln + jpegdev.GUARD
    assert pk.stream_np.size >= end
    for lo, cnt in pk.waves().tolist():                                        # a wavefront never mixes table sets
        assert len(set(pk.segments[lo:lo + cnt, 5].tolist())) == 1


def test_parse_cache(tmp_path):
    p = str(tmp_path / "frame0.jpg")
    shutil.copy(J.fixture_path(J.WIDE[0]), p)
    size = os.path.getsize(p)
    cache = jpegdev.ParseCache()
    a = cache.get(p)
    assert (cache.hits, cache.misses, len(cache)) == (0, 1, 1)
    assert cache.get(p) is a and cache.get(p, open(p, "rb").read()) is a       # a hit returns the same object
    assert (cache.hits, cache.misses) == (2, 1)
    want = jpegdev.parse(J.data(J.WIDE[0]))
    assert (a.width, a.height, a.samp, a.n_segments, a.tables_key) == (398, 224, jpegdev.S420, 1, want.tables_key)
    assert np.array_equal(a.seg_start, want.seg_start) and np.array_equal(a.seg_len, want.seg_len)
    assert np.array_equal(a.table_set, jpegdev.table_set(want))
    # nothing in the cache is as large as the file: no contents, no pixels
    held = [v for v in vars(a).values()] + list(cache._sets.values()) + list(cache._sets)
    sizes = [v.nbytes if isinstance(v, np.ndarray) else len(v) for v in held if isinstance(v, (np.ndarray, bytes, bytearray))]
    assert len(sizes) >= 5 and max(sizes) < size
    assert not any(isinstance(v, (dict, list, tuple)) for v in vars(a).values())
    # a second file with the same tables shares the table set
    p1 = str(tmp_path / "frame1.jpg")
    shutil.copy(J.fixture_path(J.WIDE[1]), p1)
    assert cache.get(p1).table_set is a.table_set
    # rewritten with other bytes of another size: parsed again
    shutil.copy(J.fixture_path(ENC[3]), p)
    b = cache.get(p)
    assert b is not a and (b.width, b.height, b.n_segments) == (32, 24, jpegdev.parse(J.data(ENC[3])).n_segments)
    assert cache.misses == 3 and len(cache) == 2
    # the same size, another modification time: parsed again as well
    st = os.stat(p)
    os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    assert cache.get(p) is not b and cache.misses == 4
    # a file outside the decoder's subset is remembered as such
    q = str(tmp_path / "cmyk.jpg")
    shutil.copy(J.fixture_path("24x32_cmyk.jpg"), q)
    assert cache.get(q) is None and cache.get(q) is None and cache.misses == 5


def test_row_table_of_a_batch_with_padding_stride_and_twin():
    T = 6
    group = [dict(paths=["/d/va", 0, 2, 0, -1, T], stride=2, paths2=["/d/vb", 5, 0, 1, 4, T], stride2=1, label="x"),
             dict(paths=["/d/vc", 7, 0, 1, 3, T], stride=1, paths2=["/d/va", 4, 2, 1, -1, T], stride2=2, label="y")]
    names, rows, zero = feeder.clip_batch_rows(group, T)
    B = len(group)
    want_names, want_rows, want_zero = [], [], np.ones(2 * B * T, bool)
    for half, (kp, ks) in enumerate([("paths", "stride"), ("paths2", "stride2")]):
        for i, c in enumerate(group):
            base, start, pad_start, pad_end, ndigits, length = c[kp]
            for j in range(length - pad_start - pad_end):
                num = start + j * c[ks]
                want_names.append(f"{base}/frame{num}.jpg" if ndigits == -1 else f"{base}/{str(num).zfill(ndigits)}.jpg")
                want_rows.append(half * B * T + i * T + pad_start + j)
                want_zero[want_rows[-1]] = False
    assert names == want_names and rows.dtype == np.int32 and rows.tolist() == want_rows
    assert names[:4] == ["/d/va/frame0.jpg", "/d/va/frame2.jpg", "/d/va/frame4.jpg", "/d/va/frame6.jpg"]
    assert rows.tolist()[:4] == [2, 3, 4, 5] and "/d/vb/0005.jpg" in names and "/d/vc/007.jpg" in names
    got_zero = np.zeros(2 * B * T, bool)
    for lo, hi in zero:
        assert 0 <= lo < hi <= 2 * B * T and not got_zero[lo:hi].any()
        got_zero[lo:hi] = True
    assert np.array_equal(got_zero, want_zero) and int(want_zero.sum()) == 2 + 1 + 1 + 3
    # without a twin: the first half alone
    names1, rows1, zero1 = feeder.clip_batch_rows([{k: v for k, v in c.items() if not k.endswith("2")} for c in group], T)
    n1 = sum(1 for r in want_rows if r < B * T)
    assert names1 == want_names[:n1] and rows1.tolist() == want_rows[:n1] and zero1 == [z for z in zero if z[1] <= B * T]
    with pytest.raises(ValueError, match="do not fit"):
        feeder.clip_batch_rows(group, T - 1)
