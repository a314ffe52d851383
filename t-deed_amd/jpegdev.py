"""Host side of the device JPEG decoder (csrc/jpeg.hip): marker parsing, packing of a video's entropy segments and
tables for the kernels, and a slow numpy model of the whole decode that the tests hold the kernels against.

Nothing here decodes pixels on the product path: `parse` walks the markers of one file, `pack` lays the entropy-coded
segments of many files into one buffer with a segment table and de-duplicated table sets (the layouts of
csrc/jpeg_core.h), and the kernels do the rest.  `pack_frames` is `pack` for the frames of a clip batch (many videos,
already parsed infos accepted), `ParseCache` keeps the parse results across epochs.  Supported files: baseline / extended-sequential Huffman (SOF0, SOF1),
8-bit samples, greyscale or YCbCr with component ids 1, 2, 3, luma sampling 1x1, 2x1 or 2x2 with 1x1 chroma, one
interleaved scan, optional restart intervals, no Adobe marker.  Everything else makes `parse` return None, and the
caller decodes that frame with Pillow (feeder.load_video_device).  `split_points` / `piece_counts` / `PIECE` are the rule
and the row layout by which a resident stream's segments are cut into pieces that decode on their own
(trainclips.ResidentJpegClips).

`decode_reference` is the arithmetic of libjpeg-turbo as Pillow uses it (Huffman decode, integer "islow" IDCT, "fancy"
triangle up-sampling, integer YCbCr -> RGB), reproduced bit for bit; it exposes the intermediate stages.
"""
from types import SimpleNamespace

import numpy as np

GREY, S444, S422, S420 = 0, 1, 2, 3
SAMPLING_NAMES = {GREY: "grey", S444: "4:4:4", S422: "4:2:2", S420: "4:2:0"}
TABLE_SET_BYTES = 4240
SEG_COLS = 6          # frame, first MCU, MCU count, byte offset, byte length, table set
GUARD = 8             # zero bytes behind every segment

# zig-zag position -> natural (row-major) index
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                    60, 61, 54, 47, 55, 62, 63], dtype=np.uint8)

_HUFF = np.dtype([("look", "<u2", 256), ("maxcode", "<i4", 18), ("valoff", "<i4", 18), ("vals", "u1", 256)])
_SET = np.dtype([("quant", "<u2", (4, 64)), ("huff", _HUFF, 4), ("tq", "u1", 4), ("td", "u1", 4), ("ta", "u1", 4),
                 ("natural", "u1", 64), ("pad", "u1", 4)])
assert _HUFF.itemsize == 912 and _SET.itemsize == TABLE_SET_BYTES


def geometry(width, height, samp):
    """Block geometry of a frame, as csrc/jpeg_core.h jc_geom: per component the block grid (bw, bh), the down-sampled
    size (cw, ch) and the first block (boff) inside the frame's coefficient range of frame_blocks * 64 int16."""
    ncomp = 1 if samp == GREY else 3
    hs = 2 if samp in (S422, S420) else 1
    vs = 2 if samp == S420 else 1
    mcus_x, mcus_y = -(-width // (8 * hs)), -(-height // (8 * vs))
    bw, bh, cw, ch, boff, off = [], [], [], [], [], 0
    for c in range(ncomp):
        h, v = (hs, vs) if c == 0 else (1, 1)
        bw.append(mcus_x * h)
        bh.append(mcus_y * v)
        cw.append(-(-width * h // hs))
        ch.append(-(-height * v // vs))
        boff.append(off)
        off += bw[-1] * bh[-1]
    return SimpleNamespace(width=width, height=height, samp=samp, ncomp=ncomp, hs=hs, vs=vs, mcus_x=mcus_x, mcus_y=mcus_y,
                           mcus=mcus_x * mcus_y, bpm=1 if ncomp == 1 else hs * vs + 2, bw=bw, bh=bh, cw=cw, ch=ch, boff=boff,
                           frame_blocks=off)


def window_blocks(geom, top, left, wh, ww):
    """What a pixel pass over the window [top, top + wh) x [left, left + ww) of a frame reads, as csrc/jpeg_core.h jc_window
    (the launcher of ops.jpeg_pixels_window uses the same formulas).  Pure.  Every range is half-open (lo, hi):
    bands: the MCU rows that hold window rows (the grid); y_cols / y_rows: the luma block columns / block rows under the
    window; c_cols: the chroma block columns of the samples the up-sampling taps touch -- for 2:1 chroma sample x >> 1 and
    its clamped neighbour, x >> 1 - 1 for an even x, x >> 1 + 1 for an odd one -- None for greyscale; mcu_rows: the MCU
    rows whose coefficients are read: the bands, for 4:2:0 one more above when the window starts on a band's first row
    and one more below when it ends on a band's last row (the vertical taps' halo).  ranges: the ten ints of
    ops.jpeg_window_blocks.  A window that is empty or leaves the frame raises ValueError."""
    top, left, wh, ww = int(top), int(left), int(wh), int(ww)
    if min(wh, ww) < 1 or top < 0 or left < 0 or top + wh > geom.height or left + ww > geom.width:
        raise ValueError(f"window_blocks: the window {wh}x{ww} at ({top}, {left}) is empty or leaves the "
                         f"{geom.height}x{geom.width} frame")
    x1, y1 = left + ww - 1, top + wh - 1
    bands = (top // (8 * geom.vs), y1 // (8 * geom.vs) + 1)
    y_cols, y_rows = (left // 8, x1 // 8 + 1), (top // 8, y1 // 8 + 1)
    c_cols = None
    if geom.ncomp == 3:
        c_lo, c_hi = left, x1
        if geom.hs == 2:
            c_lo = left >> 1 if left & 1 else max((left >> 1) - 1, 0)
            c_hi = min((x1 >> 1) + 1, geom.cw[1] - 1) if x1 & 1 else x1 >> 1
        c_cols = (c_lo // 8, c_hi // 8 + 1)
    m_lo, m_hi = bands
    if geom.vs == 2 and geom.ncomp == 3:
        if top % 16 == 0 and m_lo > 0:
            m_lo -= 1
        if y1 % 16 == 15 and (y1 >> 1) + 1 < geom.ch[1]:
            m_hi += 1
    cc = c_cols or (0, 0)
    ranges = [bands[0], bands[1] - bands[0], y_cols[0], y_cols[1] - y_cols[0], y_rows[0], y_rows[1] - 1, cc[0], cc[1] - cc[0],
              m_lo, m_hi - 1]
    return SimpleNamespace(top=top, left=left, wh=wh, ww=ww, bands=bands, y_cols=y_cols, y_rows=y_rows, c_cols=c_cols,
                           mcu_rows=(m_lo, m_hi), ranges=ranges)


def _be16(a, p):
    return (int(a[p]) << 8) | int(a[p + 1])


def parse(data):
    """Walk the markers of one JPEG file (bytes or a uint8 array).  -> None when the file is outside the supported subset
    (module docstring) or its headers are damaged, otherwise an info object: width, height, samp, ncomp,
    restart_interval, mcus, n_segments, scan_start / scan_end (byte range of the entropy-coded data), seg_start /
    seg_len (int64 arrays, one entry per segment: the whole scan, or each restart interval), tables_key (the bytes
    that decide the table set) and the raw tables."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = a.size
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        return None
    qt, huff, key = {}, {}, []
    sof, ri, p = None, 0, 2
    while True:
        if p + 4 > n or a[p] != 0xFF:
            return None
        while p < n and a[p] == 0xFF:                 # fill bytes
            p += 1
        if p >= n:
            return None
        m = int(a[p])
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or p + 2 > n:
            return None                              # EOI before a scan
        ln = _be16(a, p)
        if ln < 2 or p + ln > n:
            return None
        seg = a[p + 2:p + ln]
        if m == 0xDB:
            key.append(a[p - 2:p + ln].tobytes())
            q = 0
            while q < seg.size:
                pq, tq = int(seg[q]) >> 4, int(seg[q]) & 15
                sz = 128 if pq else 64
                if pq > 1 or tq > 3 or q + 1 + sz > seg.size:
                    return None
                body = seg[q + 1:q + 1 + sz]
                zz = (body[0::2].astype(np.uint16) << 8 | body[1::2]) if pq else body.astype(np.uint16)
                nat = np.zeros(64, np.uint16)
                nat[NATURAL] = zz
                qt[tq] = nat
                q += 1 + sz
        elif m == 0xC4:
            key.append(a[p - 2:p + ln].tobytes())
            q = 0
            while q < seg.size:
                if q + 17 > seg.size:
                    return None
                tc, th = int(seg[q]) >> 4, int(seg[q]) & 15
                counts = seg[q + 1:q + 17].astype(np.int64)
                nv = int(counts.sum())
                if tc > 1 or th > 1 or nv > 256 or q + 17 + nv > seg.size:
                    return None
                huff[(tc, th)] = (counts, seg[q + 17:q + 17 + nv].copy())
                q += 17 + nv
        elif m in (0xC0, 0xC1):
            if sof is not None or seg.size < 6:
                return None
            prec, h, w, nc = int(seg[0]), _be16(seg, 1), _be16(seg, 3), int(seg[5])
            if prec != 8 or h == 0 or w == 0 or nc not in (1, 3) or seg.size < 6 + 3 * nc:
                return None
            comps = [(int(seg[6 + 3 * i]), int(seg[7 + 3 * i]) >> 4, int(seg[7 + 3 * i]) & 15, int(seg[8 + 3 * i]))
                     for i in range(nc)]
            sof = (w, h, comps)
        elif 0xC0 <= m <= 0xCF:                       # progressive, lossless, arithmetic, hierarchical
            return None
        elif m == 0xEE:                               # Adobe: the transform flag changes the colour space
            return None
        elif m == 0xDD:
            if seg.size < 2:
                return None
            ri = _be16(seg, 0)
        elif m == 0xDA:
            break
        p += ln
    if sof is None:
        return None
    w, h, comps = sof
    nc = len(comps)
    if nc == 1:
        samp = GREY
    else:
        if [c[0] for c in comps] != [1, 2, 3] or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
        samp = {(1, 1): S444, (2, 1): S422, (2, 2): S420}.get((comps[0][1], comps[0][2]))
        if samp is None:
            return None
    if seg.size < 4 + 2 * nc or int(seg[0]) != nc:
        return None
    td, ta = [], []
    for i in range(nc):
        if int(seg[1 + 2 * i]) != comps[i][0]:
            return None
        td.append(int(seg[2 + 2 * i]) >> 4)
        ta.append(int(seg[2 + 2 * i]) & 15)
    if (int(seg[1 + 2 * nc]), int(seg[2 + 2 * nc]), int(seg[3 + 2 * nc])) != (0, 63, 0):
        return None
    tq = [c[3] for c in comps]
    if any(t not in qt for t in tq) or any((0, t) not in huff for t in td) or any((1, t) not in huff for t in ta):
        return None
    for counts, _ in huff.values():                   # a code space that overflows its length cannot be tabulated
        code = 0
        for l in range(1, 17):
            code += int(counts[l - 1])
            if code > (1 << l):
                return None
            code <<= 1
    key.append(bytes([nc] + tq + td + ta))
    g = geometry(w, h, samp)
    start = p + ln
    body = a[start:]
    ff = np.flatnonzero(body[:-1] == 0xFF) if body.size > 1 else np.zeros(0, np.int64)
    nxt = body[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    stop = ff[(nxt != 0) & ~is_rst]
    if stop.size:
        end = start + int(stop[0])
        q = end
        while q < n and a[q] == 0xFF:
            q += 1
        if q < n and a[q] != 0xD9:                    # another scan (or tables) follows: not a one-scan file
            return None
    else:
        end = n                                       # truncated: the lanes report what is missing
    if ri:
        nseg = -(-g.mcus // ri)
        keep = ff[is_rst] < end - start
        rst, codes = ff[is_rst][keep] + start, nxt[is_rst][keep]
        if rst.size > nseg - 1 or np.any(codes != 0xD0 + (np.arange(rst.size) & 7)):
            return None
        seg_start = np.full(nseg, end, np.int64)
        seg_len = np.zeros(nseg, np.int64)
        seg_start[0] = start
        seg_start[1:rst.size + 1] = rst + 2
        bounds = np.concatenate([rst, [end]])
        seg_len[:rst.size + 1] = bounds - seg_start[:rst.size + 1]
    else:
        nseg = 1
        seg_start, seg_len = np.array([start], np.int64), np.array([end - start], np.int64)
    return SimpleNamespace(width=w, height=h, samp=samp, ncomp=nc, restart_interval=ri, mcus=g.mcus, n_segments=nseg,
                           scan_start=start, scan_end=end, seg_start=seg_start, seg_len=seg_len, tables_key=b"".join(key),
                           qt=qt, huff=huff, tq=tq, td=td, ta=ta, geom=g)


def _huff_tables(counts, vals):
    """(look, maxcode, valoff, vals256) of csrc/jpeg_core.h JcHuff"""
    look = np.zeros(256, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    v256 = np.zeros(256, np.uint8)
    v256[:vals.size] = vals
    code, k = 0, 0
    for l in range(1, 17):
        c = int(counts[l - 1])
        if c:
            valoff[l] = k - code
            if l <= 8:
                for i in range(c):
                    lo = (code + i) << (8 - l)
                    look[lo:lo + (1 << (8 - l))] = (l << 8) | int(vals[k + i])
            k += c
            code += c
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0x7FFFFFFF
    return look, maxcode, valoff, v256


def table_set(info):
    """One JcTableSet (uint8 array of TABLE_SET_BYTES) from a parsed file."""
    s = np.zeros((), _SET)
    for t, q in info.qt.items():
        s["quant"][t] = q
    for (tc, th), (counts, vals) in info.huff.items():
        look, maxcode, valoff, v256 = _huff_tables(counts, vals)
        hrec = s["huff"][2 * tc + th]
        hrec["look"], hrec["maxcode"], hrec["valoff"], hrec["vals"] = look, maxcode, valoff, v256
    s["tq"][:info.ncomp], s["td"][:info.ncomp], s["ta"][:info.ncomp] = info.tq, info.td, info.ta
    s["natural"] = NATURAL
    return np.frombuffer(s.tobytes(), np.uint8).copy()


class PackedJpegs:
    """The frames of one video, ready for the kernels.
    stream: uint8 buffer of every segment's entropy-coded bytes (page-locked torch tensor when a GPU runtime is there,
      numpy otherwise; `stream_np` is always the numpy view), each segment 4-byte aligned and followed by >= 8 zero bytes
    segments: int32 (n_segments, 6) rows of frame, first MCU, MCU count, byte offset, byte length, table set; rows are
      sorted by table set, then frame, then first MCU, so the segments of a set are contiguous
    table_sets: uint8 (n_sets, TABLE_SET_BYTES); frame_set: int32 (n_frames,) table set per frame, -1 = not on the device
    fallback: frames `parse` rejected or whose sampling differs from the video's (decode them with Pillow)"""

    def __init__(self, width, height, samp, n_frames, stream, stream_np, segments, table_sets, frame_set, fallback):
        self.width, self.height, self.samp, self.n_frames = width, height, samp, n_frames
        self.stream, self.stream_np, self.segments, self.table_sets = stream, stream_np, segments, table_sets
        self.frame_set, self.fallback = frame_set, fallback
        self.geom = geometry(width, height, samp) if width else None

    @property
    def n_segments(self):
        return int(self.segments.shape[0])

    @property
    def n_sets(self):
        return int(self.table_sets.shape[0])

    def rows(self, frame_lo, frame_hi):
        """indices of the segment rows whose frame lies in [frame_lo, frame_hi), in table order"""
        f = self.segments[:, 0]
        return np.flatnonzero((f >= frame_lo) & (f < frame_hi))

    def waves(self, frame_lo=0, frame_hi=None):
        """int32 (n_waves, 2) rows of (first segment row, count <= 64): the wavefronts of one entropy launch over the
        frames [frame_lo, frame_hi).  The rows of a wavefront are consecutive and share one table set."""
        idx = self.rows(frame_lo, self.n_frames if frame_hi is None else frame_hi)
        if idx.size == 0:
            return np.zeros((0, 2), np.int32)
        sets = self.segments[idx, 5]
        brk = np.flatnonzero((np.diff(idx) != 1) | (np.diff(sets) != 0)) + 1
        out = []
        for lo, hi in zip(np.concatenate([[0], brk]), np.concatenate([brk, [idx.size]])):
            first = int(idx[lo])
            for o in range(0, int(hi - lo), 64):
                out.append((first + o, min(64, int(hi - lo) - o)))
        return np.asarray(out, np.int32).reshape(-1, 2)

    def save(self, path):
        """The trivial file format of tools/jpeg_host_check.cpp: int32 header (magic, width, height, sampling, frames,
        segments, table sets, stream bytes), then frame_set, the segment table, the table sets and the stream."""
        hdr = np.array([0x314B504A, self.width, self.height, self.samp, self.n_frames, self.n_segments, self.n_sets,
                        self.stream_np.size], np.int32)
        with open(path, "wb") as f:
            for part in (hdr, self.frame_set, self.segments, self.table_sets, self.stream_np):
                f.write(np.ascontiguousarray(part).tobytes())


def pack(datas, pinned=True):
    """Pack the files of one video (bytes or uint8 arrays, one per frame) -> PackedJpegs.  Geometry and sampling are
    those of the first supported frame; a supported frame of another geometry raises ValueError (as feeder.load_video
    does when a frame does not fit), one of another sampling takes the fallback."""
    return pack_frames(datas, None, pinned)


def pack_frames(datas, infos=None, pinned=True):
    """`pack` for any list of frames -- the frames of a clip batch come from many videos -- with the same layout and the
    same rules: geometry and sampling of the first supported frame, another sampling -> fallback, another geometry ->
    ValueError.  infos: the `parse` result of every file (None for an unsupported one) when the caller has them already,
    e.g. from a ParseCache; an info that carries `table_set` (ParseCache's do) spares building the tables again."""
    if infos is None:
        infos = [parse(d) for d in datas]
    elif len(infos) != len(datas):
        raise ValueError(f"pack_frames: {len(infos)} infos for {len(datas)} files")
    arrs = [np.frombuffer(d, np.uint8) if not isinstance(d, np.ndarray) else d for d in datas]
    first = next((i for i in infos if i is not None), None)
    n = len(datas)
    frame_set = np.full(n, -1, np.int32)
    if first is None:
        return PackedJpegs(0, 0, 0, n, np.zeros(GUARD, np.uint8), np.zeros(GUARD, np.uint8), np.zeros((0, SEG_COLS), np.int32),
                           np.zeros((0, TABLE_SET_BYTES), np.uint8), frame_set, list(range(n)))
    sets, set_rows, fallback, rows = {}, [], [], []
    total = 0
    for f, info in enumerate(infos):
        if info is None or info.samp != first.samp:
            fallback.append(f)
            continue
        if (info.width, info.height) != (first.width, first.height):
            raise ValueError(f"frame {f}: {info.height}x{info.width} does not fit the video's {first.height}x{first.width}")
        sid = sets.get(info.tables_key)
        if sid is None:
            sid = sets[info.tables_key] = len(set_rows)
            ready = getattr(info, "table_set", None)
            set_rows.append(table_set(info) if ready is None else ready)
        frame_set[f] = sid
        ri = info.restart_interval or info.mcus
        for s in range(info.n_segments):
            rows.append((sid, f, s * ri, min(ri, info.mcus - s * ri), int(info.seg_start[s]), int(info.seg_len[s])))
    rows.sort(key=lambda r: r[:3])
    seg = np.zeros((len(rows), SEG_COLS), np.int32)
    offs = []
    for i, (sid, f, m0, nm, src, ln) in enumerate(rows):
        seg[i] = (f, m0, nm, total, ln, sid)
        offs.append(total)
        total += (ln + GUARD + 3) & ~3
    if total >= 1 << 31:
        raise ValueError(f"the packed stream of {total} bytes exceeds the segment table's 32-bit offsets")
    total = max(total, GUARD)
    stream, stream_np = None, None
    if pinned:
        try:
            import torch
            if torch.cuda.is_available():
                stream = torch.zeros(total, dtype=torch.uint8).pin_memory()
                stream_np = stream.numpy()
        except ImportError:
            pass
    if stream_np is None:
        stream = stream_np = np.zeros(total, np.uint8)
    for (sid, f, m0, nm, src, ln), off in zip(rows, offs):
        stream_np[off:off + ln] = arrs[f][src:src + ln]
    tsets = np.stack(set_rows) if set_rows else np.zeros((0, TABLE_SET_BYTES), np.uint8)
    return PackedJpegs(first.width, first.height, first.samp, n, stream, stream_np, seg, tsets, frame_set, fallback)


# ------------------------------------------------------------------------------------------------- pieces of a segment
# csrc/jpeg_core.h JcState / JcPiece: one row of the piece table of a resident stream
_STATE = np.dtype([("bits", "<u8"), ("byte_off", "<i4"), ("n", "<i4"), ("pad", "<i4"), ("marker", "<i4"), ("pred", "<i4", 3),
                   ("spare", "<i4")])
PIECE = np.dtype([("pos", "<i8"), ("segment", "<i4"), ("first_mcu", "<i4"), ("n_mcu", "<i4"), ("set", "<i4"), ("left", "<i4"),
                  ("spare", "<i4"), ("st", _STATE)])
PIECE_BYTES = 72
assert _STATE.itemsize == 40 and PIECE.itemsize == PIECE_BYTES


def split_points(first_mcu, n_mcu, split_mcus):
    """The MCUs at which a segment row (first_mcu, n_mcu) is cut into pieces: every m with first_mcu < m < first_mcu + n_mcu
    and m % split_mcus == 0.  k split points make k + 1 pieces."""
    if split_mcus < 1:
        raise ValueError("split_mcus must be positive")
    lo = (first_mcu // split_mcus + 1) * split_mcus
    return list(range(lo, first_mcu + n_mcu, split_mcus))


def piece_counts(segments, split_mcus):
    """pieces per row of a segment table (int64 (n_segments,)) under `split_points`, as csrc/jpeg_core.h jc_piece_count"""
    if split_mcus < 1:
        raise ValueError("split_mcus must be positive")
    first, n = segments[:, 1].astype(np.int64), segments[:, 2].astype(np.int64)
    return 1 + (first + n - 1) // split_mcus - first // split_mcus


def piece_ranges(segments, split_mcus):
    """(first MCU, MCU count) of every piece of a segment table under `split_points`, int64 (n_pieces, 2), in the piece
    table's order: segment row by segment row, the pieces of a row in ascending MCU order (what the index pass records in
    JcPiece.first_mcu / n_mcu, known on the host without it)."""
    out = []
    for m0, nm in np.asarray(segments)[:, 1:3].tolist():
        cuts = [m0] + split_points(m0, nm, split_mcus) + [m0 + nm]
        out += [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    return np.asarray(out, np.int64).reshape(-1, 2)


class ParseCache:
    """What `parse` finds in a file, kept per (path, size, mtime_ns), so that an epoch over files seen before only reads
    them and copies their segment bytes (`pack_frames(datas, infos)`).  An entry is what pack_frames needs short of the
    file's bytes: geometry, sampling, the segment byte ranges, tables_key and the built table set (one array per distinct
    tables_key, shared by its files); None for a file outside the decoder's subset.  Never pixel data or file contents.
    A file whose size or modification time changed is parsed again and replaces its entry."""

    def __init__(self):
        self._files = {}            # path -> (size, mtime_ns, info | None)
        self._sets = {}             # tables_key -> table set (uint8 TABLE_SET_BYTES)
        self.hits = self.misses = 0

    def __len__(self):
        return len(self._files)

    def lookup(self, path, size, mtime_ns, data):
        """the entry of `path`, whose size / mtime_ns (os.stat) and bytes the caller has read"""
        e = self._files.get(path)
        if e is not None and e[0] == size and e[1] == mtime_ns:
            self.hits += 1
            return e[2]
        self.misses += 1
        full = parse(data)
        info = None
        if full is not None:
            ts = self._sets.get(full.tables_key)
            if ts is None:
                ts = self._sets[full.tables_key] = table_set(full)
            info = SimpleNamespace(width=full.width, height=full.height, samp=full.samp, ncomp=full.ncomp,
                                   restart_interval=full.restart_interval, mcus=full.mcus, n_segments=full.n_segments,
                                   seg_start=full.seg_start, seg_len=full.seg_len, tables_key=full.tables_key, table_set=ts)
        self._files[path] = (size, mtime_ns, info)
        return info

    def get(self, path, data=None):
        """the entry of `path` (stat here; the file is read only when it has to be parsed and `data` is not given)"""
        import os
        st = os.stat(path)
        e = self._files.get(path)
        if data is None and not (e is not None and e[0] == st.st_size and e[1] == st.st_mtime_ns):
            with open(path, "rb") as f:
                data = f.read()
        return self.lookup(path, st.st_size, st.st_mtime_ns, data)


# ------------------------------------------------------------------------------------------------- the numpy model
def _decode_segment(bits24, nbytes, info, lut, first_mcu, n_mcu, coeffs):
    g = info.geom
    pos, limit = 0, nbytes * 8
    pred = [0, 0, 0]
    blocks = [(0, v, h) for v in range(g.vs) for h in range(g.hs)] if info.ncomp == 3 else [(0, 0, 0)]
    blocks += [(1, 0, 0), (2, 0, 0)] if info.ncomp == 3 else []

    def take(nb):
        nonlocal pos
        v = (bits24[pos >> 3] >> (8 - (pos & 7))) & 0xFFFF
        pos += nb
        return v >> (16 - nb) if nb else 0

    def symbol(t):
        nonlocal pos
        w = (bits24[pos >> 3] >> (8 - (pos & 7))) & 0xFFFF
        l, s = lut[t][w]
        if l == 0:
            raise ValueError("no Huffman code within 16 bits")
        pos += l
        return s

    for m in range(first_mcu, first_mcu + n_mcu):
        my, mx = divmod(m, g.mcus_x)
        for c, v, h in blocks:
            hc, vc = (g.hs, g.vs) if c == 0 else (1, 1)
            blk = coeffs[c][my * vc + v, mx * hc + h]
            t = symbol((0, info.td[c]))
            if t > 11:
                raise ValueError("DC category above 11")
            d = take(t)
            if t and d < (1 << (t - 1)):
                d = d - (1 << t) + 1
            pred[c] += d
            blk[0] = pred[c]
            k = 1
            while k < 64:
                rs = symbol((1, info.ta[c]))
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    if k > 63 or s > 10:
                        raise ValueError("bad AC run / size")
                    x = take(s)
                    if x < (1 << (s - 1)):
                        x = x - (1 << s) + 1
                    blk[NATURAL[k]] = x
                    k += 1
                elif r == 15:
                    k += 16
                else:
                    break
            if pos > limit:
                raise ValueError("entropy data exhausted")


def _lut16(counts, vals):
    """[(length, symbol)] for every 16-bit window"""
    ln = np.zeros(65536, np.uint8)
    sy = np.zeros(65536, np.uint8)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(int(counts[l - 1])):
            lo = code << (16 - l)
            ln[lo:lo + (1 << (16 - l))] = l
            sy[lo:lo + (1 << (16 - l))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return list(zip(ln.tolist(), sy.tolist()))


def _idct_1d(i, s):
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [(x + (1 << (s - 1))) >> s for x in out]


def idct_blocks(coef, quant):
    """coef (..., 64) int, quant (64,) -> samples (..., 8, 8) uint8"""
    x = (coef.astype(np.int64) * quant.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    cols = _idct_1d([x[..., r, :] for r in range(8)], 11)            # over columns: inputs are the rows of each column
    ws = np.stack(cols, axis=-2)
    rows = _idct_1d([ws[..., :, c] for c in range(8)], 18)
    return np.clip(np.stack(rows, axis=-1) + 128, 0, 255).astype(np.uint8)


def _up_h(p):
    """fancy 2x horizontal up-sampling of rows (any leading shape)"""
    p = p.astype(np.int32)
    left = np.concatenate([p[..., :1], p[..., :-1]], -1)
    right = np.concatenate([p[..., 1:], p[..., -1:]], -1)
    out = np.empty(p.shape[:-1] + (2 * p.shape[-1],), np.int32)
    out[..., 0::2] = (3 * p + left + 1) >> 2
    out[..., 1::2] = (3 * p + right + 2) >> 2
    return out


def _up_hv(p):
    p = p.astype(np.int32)
    up = np.concatenate([p[:1], p[:-1]], 0)
    dn = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int32)
    for par, nb in ((0, up), (1, dn)):
        cs = 3 * p + nb
        left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        out[par::2, 0::2] = (3 * cs + left + 8) >> 4
        out[par::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def decode_reference(data):
    """The whole decode in numpy (slow; for tests).  -> object with info, coeffs (per component int16 (bh, bw, 64),
    natural order, un-dequantised), planes (per component uint8, cropped to the down-sampled size), rgb uint8 (3,H,W)
    and flat (the frame's coefficient range in the kernels' layout).  Raises ValueError on an unsupported or damaged
    file."""
    info = parse(data)
    if info is None:
        raise ValueError("unsupported JPEG file")
    a = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    g = info.geom
    coeffs = [np.zeros((g.bh[c], g.bw[c], 64), np.int32) for c in range(g.ncomp)]
    lut = {k: _lut16(*v) for k, v in info.huff.items()}
    ri = info.restart_interval or g.mcus
    for s in range(info.n_segments):
        raw = a[info.seg_start[s]:info.seg_start[s] + info.seg_len[s]].tobytes().replace(b"\xff\x00", b"\xff")
        b = np.frombuffer(raw + b"\0" * 8, np.uint8).astype(np.int64)
        bits24 = ((b[:-2] << 16) | (b[1:-1] << 8) | b[2:]).tolist()
        _decode_segment(bits24, len(raw), info, lut, s * ri, min(ri, g.mcus - s * ri), coeffs)
    coeffs = [c.astype(np.int16) for c in coeffs]
    planes = []
    for c in range(g.ncomp):
        px = idct_blocks(coeffs[c], info.qt[info.tq[c]])                       # (bh, bw, 8, 8)
        planes.append(px.transpose(0, 2, 1, 3).reshape(g.bh[c] * 8, g.bw[c] * 8)[:g.ch[c], :g.cw[c]])
    H, W = info.height, info.width
    y = planes[0].astype(np.int32)
    if g.ncomp == 1:
        rgb = np.stack([planes[0]] * 3)
    else:
        if info.samp == S444:
            cb, cr = planes[1].astype(np.int32), planes[2].astype(np.int32)
        elif info.samp == S422:
            cb, cr = _up_h(planes[1])[:H, :W], _up_h(planes[2])[:H, :W]
        else:
            cb, cr = _up_hv(planes[1])[:H, :W], _up_hv(planes[2])[:H, :W]
        cb, cr = cb - 128, cr - 128
        r = y + ((91881 * cr + 32768) >> 16)
        gg = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        bl = y + ((116130 * cb + 32768) >> 16)
        rgb = np.clip(np.stack([r, gg, bl]), 0, 255).astype(np.uint8)
    flat = np.concatenate([c.reshape(-1) for c in coeffs])
    return SimpleNamespace(info=info, coeffs=coeffs, planes=planes, rgb=rgb, flat=flat)
