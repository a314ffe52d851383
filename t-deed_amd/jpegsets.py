"""A label list's frames as packed JPEG entropy streams, and the per-batch tables of their decode.

A set that stays on the device compressed: `load_resident_jpegs` packs the entropy streams of every frame once
(`join_resident_jpegs` makes one set of two), and a batch decodes the frames it drew on the device (csrc/jpeg.hip), one
lane per piece of a frame's scan; `batch_tables` is the host's share of a batch, `video_tables` that of a whole video --
both pure numpy.
"""
from types import SimpleNamespace

import numpy as np

from .cliptable import _strides_of


class ResidentJpegs:
    """The frames of a label list as packed entropy streams on the host (`load_resident_jpegs`).
    shards: [namespace(packed=jpegdev.PackedJpegs, frames=int64 (n,) -- the set-wide number of every frame of the pack)];
      the table-set column of every shard indexes `table_sets`, the one array of the whole set.
    frame_set int32 (n_frames,): table set per frame, -1 = not decodable on the device (in `fallback`).
    video_first / video_len: per video its first frame in the set-wide numbering and its length; names: every frame's file.
    width / height / samp: geometry and sampling of the set's first supported frame (0 x 0 when there is none).
    stride: the sampling of `load_resident_jpegs`: frame j of a video is its file j * stride."""

    def __init__(self, shards, table_sets, frame_set, fallback, video_first, video_len, names, width, height, samp, stride=1):
        self.stride = int(stride)
        self.shards, self.table_sets, self.frame_set, self.fallback = shards, table_sets, frame_set, fallback
        self.video_first, self.video_len, self.names = video_first, video_len, names
        self.width, self.height, self.samp = width, height, samp

    @property
    def n_frames(self):
        return len(self.names)

    @property
    def n_sets(self):
        return int(self.table_sets.shape[0])

    @property
    def n_segments(self):
        return sum(s.packed.n_segments for s in self.shards)

    @property
    def stream_bytes(self):
        return sum(int(s.packed.stream_np.size) for s in self.shards)


def load_resident_jpegs(frame_dir, dataset, videos, pool=None, cache=None, shard_bytes=1 << 30, pinned=True, stride=1):
    """Read every frame file of the label list ONCE (through `pool`'s threads when a DecodePool is given), parse it (with
    `cache`, a jpegdev.ParseCache, when given) and pack the entropy segments with `jpegdev.pack_frames`, in shards of
    consecutive frames whose stream stays under shard_bytes (a shard holds at least one frame; the default is below 2^31
    because a segment row's byte offset is int32) -> ResidentJpegs.  Geometry and sampling are those of the set's first
    supported frame: a supported frame of another geometry raises ValueError, one of another sampling takes the fallback,
    as a file outside the decoder's subset does.  Missing files: as `trainclips.load_resident_videos` -- num_frames must be
    the number of frames that exist (ValueError), a hole in front of an existing frame raises FileNotFoundError.
    stride = s: only the files j * s of every video are read and packed (`feeder.load_video`'s sampling) and video_len is
    ceil(num_frames / s); the set remembers s (`ResidentJpegs.stride`)."""
    import os
    from . import feeder, jpegdev
    if not 0 < shard_bytes < 1 << 31:
        raise ValueError("shard_bytes must be positive and below 2^31 (a segment row's byte offset is int32)")
    stride = int(stride)
    if stride < 1:
        raise ValueError("load_resident_jpegs: stride must be positive")
    names, video_first, video_len = [], [], []
    for v in videos:
        n = int(v["num_frames"])
        path_fn = feeder.frame_locator(frame_dir, dataset, v["video"], v.get("_source_info"))[3]
        if n < 1 or not os.path.exists(path_fn(n - 1)):
            raise ValueError(f"video {v['video']}: num_frames={n}, but {path_fn(max(n, 1) - 1)} does not exist -- num_frames must "
                             "be the number of frames that exist")
        own = [path_fn(j) for j in range(0, n, stride)]
        for p in own:
            if not os.path.exists(p):
                raise FileNotFoundError(f"video {v['video']}: {p} is missing although later frames exist")
        video_first.append(len(names))
        video_len.append(len(own))
        names += own
    reader = pool.ex.map if pool is not None and hasattr(pool, "ex") else map
    first = None
    keys, set_rows = {}, []                         # tables_key -> set of the whole list
    shards, fallback = [], []
    frame_set = np.full(len(names), -1, np.int32)
    cur, cur_bytes = [], 0                          # (frame, data, info | None) of the shard being filled

    def flush():
        nonlocal cur, cur_bytes
        if not cur:
            return
        infos = [c[2] for c in cur]
        packed = jpegdev.pack_frames([c[1] for c in cur], infos, pinned)
        frames = np.asarray([c[0] for c in cur], np.int64)
        local = []                                  # the shard's own sets, in pack_frames' order of first appearance
        for info in infos:
            if info is not None and info.tables_key not in local:
                local.append(info.tables_key)
        remap = np.zeros(max(len(local), 1), np.int32)
        for i, key in enumerate(local):
            if key not in keys:
                keys[key] = len(set_rows)
                set_rows.append(packed.table_sets[i])
            remap[i] = keys[key]
        if packed.n_segments:
            packed.segments[:, 5] = remap[packed.segments[:, 5]]
        on = packed.frame_set >= 0
        packed.frame_set[on] = remap[packed.frame_set[on]]
        frame_set[frames] = packed.frame_set
        fallback.extend(int(frames[f]) for f in packed.fallback)
        shards.append(SimpleNamespace(packed=packed, frames=frames))
        cur, cur_bytes = [], 0

    block = 256
    for lo in range(0, len(names), block):
        part = names[lo:lo + block]
        for k, (data, size, mtime) in enumerate(reader(feeder._read_file_stat, part)):
            info = cache.lookup(part[k], size, mtime, data) if cache is not None else jpegdev.parse(data)
            if info is not None:
                if first is None:
                    first = info
                if info.samp != first.samp:
                    info = None                     # another sampling: kept decoded, as pack_frames would decide per pack
                elif (info.width, info.height) != (first.width, first.height):
                    raise ValueError(f"frame {part[k]}: {info.height}x{info.width} does not fit the set's "
                                     f"{first.height}x{first.width}")
            need = 0 if info is None else sum((int(ln) + jpegdev.GUARD + 3) & ~3 for ln in info.seg_len)
            if cur and cur_bytes + need > shard_bytes:
                flush()
            cur.append((lo + k, data, info))
            cur_bytes += need
    flush()
    table_sets = np.stack(set_rows) if set_rows else np.zeros((0, jpegdev.TABLE_SET_BYTES), np.uint8)
    for s in shards:
        s.packed.table_sets = table_sets
    w, h, samp = (first.width, first.height, first.samp) if first is not None else (0, 0, 0)
    return ResidentJpegs(shards, table_sets, frame_set, sorted(fallback), np.asarray(video_first, np.int64),
                         np.asarray(video_len, np.int64), names, w, h, samp, stride)


def join_resident_jpegs(a, b):
    """One packed set over two (`load_resident_jpegs` each), a's videos and frames in front of b's; pure host code.
    The shards' streams are reused, not copied.  b's frame numbers are shifted by a's frames, and its table sets are
    renumbered into the joined array: a set whose bytes a already has keeps a's number, the others follow a's (b's segment
    tables and per-frame set columns are rewritten copies; a's shards are taken as they are, pointed at the joined array).
    Geometry and sampling are those of the joined set's first supported frame.  Another width or height in the other
    part raises ValueError.  With another chroma sampling, b's frames all take the existing route of a frame with
    another sampling: they join the fallback, are decoded once on the host and stay decoded in the side buffer; their
    shards are listed without segments.  The two sets must have been loaded with the same `stride`."""
    from . import jpegdev
    if a.stride != b.stride:
        raise ValueError(f"join_resident_jpegs: the sets were loaded with strides {a.stride} and {b.stride}")
    if a.width and b.width and (a.width, a.height) != (b.width, b.height):
        raise ValueError(f"join_resident_jpegs: frames of {b.height}x{b.width} do not fit the set's {a.height}x{a.width}")
    w, h, samp = (a.width, a.height, a.samp) if a.width else (b.width, b.height, b.samp)
    other = bool(a.width and b.width and a.samp != b.samp)            # b: all through the side buffer
    na = a.n_frames
    rows = [r for r in a.table_sets]
    seen = {r.tobytes(): i for i, r in enumerate(rows)}
    remap = np.zeros(max(b.n_sets, 1), np.int32)
    for i in range(0 if other else b.n_sets):
        key = b.table_sets[i].tobytes()
        if key not in seen:
            seen[key] = len(rows)
            rows.append(b.table_sets[i])
        remap[i] = seen[key]
    table_sets = np.stack(rows) if rows else np.zeros((0, jpegdev.TABLE_SET_BYTES), np.uint8)
    shards = []
    for s in a.shards:
        s.packed.table_sets = table_sets                    # a's numbers are the joined array's first rows
        shards.append(s)
    for s in b.shards:
        p = s.packed
        n = len(s.frames)
        if other:
            none = np.zeros(jpegdev.GUARD, np.uint8)
            packed = jpegdev.PackedJpegs(0, 0, 0, n, none, none, np.zeros((0, jpegdev.SEG_COLS), np.int32), table_sets,
                                         np.full(n, -1, np.int32), list(range(n)))
        else:
            seg = p.segments.copy()
            if seg.shape[0]:
                seg[:, 5] = remap[seg[:, 5]]
            fs = p.frame_set.copy()
            fs[fs >= 0] = remap[fs[fs >= 0]]
            packed = jpegdev.PackedJpegs(p.width, p.height, p.samp, p.n_frames, p.stream, p.stream_np, seg, table_sets, fs,
                                         list(p.fallback))
        shards.append(SimpleNamespace(packed=packed, frames=np.asarray(s.frames, np.int64) + na))
    fs_b = np.asarray(b.frame_set, np.int32).copy()
    if other:
        fs_b[:] = -1
        fall_b = list(range(b.n_frames))
    else:
        fs_b[fs_b >= 0] = remap[fs_b[fs_b >= 0]]
        fall_b = [int(f) for f in b.fallback]
    return ResidentJpegs(shards, table_sets, np.concatenate([np.asarray(a.frame_set, np.int32), fs_b]),
                         sorted([int(f) for f in a.fallback] + [f + na for f in fall_b]),
                         np.concatenate([np.asarray(a.video_first, np.int64), np.asarray(b.video_first, np.int64) + na]),
                         np.concatenate([np.asarray(a.video_len, np.int64), np.asarray(b.video_len, np.int64)]),
                         list(a.names) + list(b.names), w, h, samp, a.stride)


def _cut_waves(keys):
    """(first, count <= 64) rows over a sorted key column: no row spans two keys"""
    n = keys.size
    if n == 0:
        return np.zeros((0, 2), np.int32)
    brk = np.flatnonzero(np.diff(keys) != 0) + 1
    out = []
    for lo, hi in zip(np.concatenate([[0], brk]), np.concatenate([brk, [n]])):
        for o in range(int(lo), int(hi), 64):
            out.append((o, min(64, int(hi) - o)))
    return np.asarray(out, np.int32).reshape(-1, 2)


def batch_tables(rows, clip_len, stride, frame_set, side_row, piece_lo, piece_n, n_slots=None, clip_slot=None, chunk_slots=None,
                 piece_keep=None):
    """The tables of one batch of `trainclips.ResidentJpegClips` (pure numpy; no file, no device).
    rows: int64 (>= 3, n) -- per clip the first frame of its video in the set-wide numbering, the clip's base and the
    video's length (`ResidentClips`' rows).  Slot clip_slot[k] + t (default k * clip_len + t) of the batch shows frame
    first + base + t * stride of clip k, or zeros where base + t * stride falls outside the video (the window rule of
    ops.train_clip_gather).  frame_set / side_row / piece_lo / piece_n: per frame of the set its table set (-1: not decoded
    on the device), its row in the side buffer of decoded frames (-1: none), its first row in the piece table and its
    number of pieces.  stride: one for all clips, or one per clip (a joint batch; with mixup the partners' follow the
    clips', as the rows do).  chunk_slots: slots per coefficient chunk (default: all in one).  piece_keep: bool per row of the
    piece table, False leaves the piece out of the items (`video_tables`' MCU-row filter); default: every piece.
    -> namespace(n_slots,
         slot_set int32 (n_slots,): table set of every slot the device decodes, -1 for the others (padding, side, unused);
         fill int32 (n_slots,): -1 a padding slot (zeros), r >= 0 the side row to copy, -2 leave the slot alone;
         items int32 (n_items, 2): (piece row, slot) of every piece of every device slot, ordered by chunk, then table set;
         waves int32 (n_waves, 2): (first item, count <= 64), no wave spanning two sets or two chunks;
         chunks [(slot_lo, slot_hi, wave_lo, wave_hi)]: the waves of every chunk that has any)."""
    T = int(clip_len)
    first, base, nfr = (np.asarray(rows[i], np.int64) for i in range(3))
    n = first.size
    at = np.arange(n, dtype=np.int64) * T if clip_slot is None else np.asarray(clip_slot, np.int64)
    total = int(n_slots) if n_slots is not None else n * T
    f = base[:, None] + np.arange(T, dtype=np.int64)[None, :] * _strides_of(stride, n, "batch_tables")[:, None]
    real = ((f >= 0) & (f < nfr[:, None])).reshape(-1)
    g = np.where(real, (first[:, None] + f).reshape(-1), 0)
    slots = (at[:, None] + np.arange(T, dtype=np.int64)[None, :]).reshape(-1)
    if n and (slots.min() < 0 or slots.max() >= total or np.unique(slots).size != slots.size):
        raise ValueError("batch_tables: the clips' slots overlap or leave the batch")
    side = np.where(real, side_row[g], -1)
    sets = np.where(real & (side < 0), frame_set[g], -1)
    if np.any(real & (side < 0) & (sets < 0)):
        raise ValueError("batch_tables: a frame is neither decodable on the device nor in the side buffer")
    slot_set = np.full(total, -1, np.int32)
    fill = np.full(total, -2, np.int32)
    slot_set[slots] = sets
    fill[slots] = np.where(real, np.where(side >= 0, side, -2), -1)
    dev = np.flatnonzero(sets >= 0)
    cnt = piece_n[g[dev]].astype(np.int64)
    n_items = int(cnt.sum())
    it_slot = np.repeat(slots[dev], cnt)
    it_piece = np.repeat(piece_lo[g[dev]].astype(np.int64), cnt) + (np.arange(n_items) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    it_set = np.repeat(sets[dev], cnt)
    if piece_keep is not None:
        on = np.asarray(piece_keep, bool)[it_piece]
        it_slot, it_piece, it_set = it_slot[on], it_piece[on], it_set[on]
    per = total if not chunk_slots else int(chunk_slots)
    it_chunk = it_slot // max(per, 1)
    order = np.lexsort((it_piece, it_set, it_chunk))
    items = np.stack([it_piece[order], it_slot[order]], 1).astype(np.int32).reshape(-1, 2)
    n_sets = int(frame_set.max()) + 1 if frame_set.size else 0
    waves = _cut_waves(it_chunk[order] * max(n_sets, 1) + it_set[order])
    chunks = []
    if waves.shape[0]:
        wchunk = it_chunk[order][waves[:, 0]]
        for c in np.unique(wchunk):
            w = np.flatnonzero(wchunk == c)
            chunks.append((int(c) * per, min((int(c) + 1) * per, total), int(w[0]), int(w[-1]) + 1))
    return SimpleNamespace(n_slots=total, slot_set=slot_set, fill=fill, items=items, waves=waves, chunks=chunks)


def video_tables(first, length, frame_set, side_row, piece_lo, piece_n, chunk_slots=None, piece_mcu=None, mcus_x=None,
                 mcu_rows=None):
    """`batch_tables` for one whole video (pure numpy; no file, no device): the video is one "clip" of its own length at
    stride 1 over the set's numbering, so slot t shows frame first + t and no slot is padding.  chunk_slots: frames per
    coefficient chunk.  mcu_rows = (lo, hi): the MCU rows a windowed pixel pass reads (`jpegdev.window_blocks(...).mcu_rows`,
    halo rows included); a piece whose MCUs -- piece_mcu int (n_pieces, 2) rows of (first MCU, MCU count), `jpegdev.
    piece_ranges` -- lie wholly in other MCU rows (mcus_x MCUs each) is left out of the items.  -> batch_tables' namespace."""
    keep = None
    if mcu_rows is not None:
        if piece_mcu is None or not mcus_x or int(mcus_x) < 1:
            raise ValueError("video_tables: the MCU-row filter needs piece_mcu and mcus_x")
        lo, hi = int(mcu_rows[0]), int(mcu_rows[1])
        if not 0 <= lo < hi:
            raise ValueError(f"video_tables: MCU rows {lo}..{hi}")
        pm = np.asarray(piece_mcu, np.int64).reshape(-1, 2)
        keep = ((pm[:, 0] + pm[:, 1] - 1) // int(mcus_x) >= lo) & (pm[:, 0] // int(mcus_x) < hi)
    if int(length) < 1 or int(first) < 0:
        raise ValueError(f"video_tables: {int(length)} frames from frame {int(first)}")
    rows = np.asarray([[int(first)], [0], [int(length)]], np.int64)
    return batch_tables(rows, int(length), 1, frame_set, side_row, piece_lo, piece_n, chunk_slots=chunk_slots, piece_keep=keep)
