"""Planning for packed JPEG sets larger than the device budget, pure numpy.

A streamed set keeps the streams of the first videos that fit resident and the others in the host shards: `frame_extents`
says where every frame's bytes lie, `stream_plan` decides which videos stay resident and how large a staging region is, and
`stage_batch` gives the range copies and the relocation rows of one batch (or of one chunk of a video).
"""
from types import SimpleNamespace

import numpy as np

from .cliptable import _strides_of

_NO_BYTE = np.iinfo(np.int64).max


def _round16(x):
    return (x + 15) & ~15


def frame_extents(shards):
    """Where every frame's entropy streams lie on the host.  shards: `ResidentJpegs.shards`.
    -> namespace(shard int32 (n_frames,): the shard that lists the frame; lo / hi int64 (n_frames,): first byte and end byte
    of the frame's segments in that shard's stream, the end including the zero GUARD behind the last segment (padded to the
    segment alignment, as `jpegdev.pack_frames` lays it out) -- lo >= hi for a frame without segments (fallback);
    shard_first int64 (n_shards + 1,): the shards' frame boundaries).  The frames of a shard are a consecutive run."""
    from . import jpegdev
    n = sum(len(s.frames) for s in shards)
    shard = np.zeros(n, np.int32)
    lo = np.full(n, _NO_BYTE, np.int64)
    hi = np.zeros(n, np.int64)
    first = [0]
    for k, s in enumerate(shards):
        fr = np.asarray(s.frames, np.int64)
        if fr.size == 0 or fr[0] != first[-1] or np.any(np.diff(fr) != 1):
            raise ValueError("frame_extents: the frames of the shards must be consecutive runs in set order")
        first.append(first[-1] + fr.size)
        shard[fr] = k
        seg = s.packed.segments
        if seg.shape[0]:
            f = fr[seg[:, 0]]
            off = seg[:, 3].astype(np.int64)
            np.minimum.at(lo, f, off)
            np.maximum.at(hi, f, off + ((seg[:, 4].astype(np.int64) + jpegdev.GUARD + 3) & ~3))
    return SimpleNamespace(shard=shard, lo=lo, hi=hi, shard_first=np.asarray(first, np.int64))


def _shard_first(ext):
    if getattr(ext, "shard_first", None) is not None:
        return np.asarray(ext.shard_first, np.int64)
    sh = np.asarray(ext.shard, np.int64)
    n_sh = int(sh.max()) + 1 if sh.size else 0
    if sh.size and np.any(np.diff(sh) < 0):
        raise ValueError("the shards must hold consecutive runs of frames")
    return np.searchsorted(sh, np.arange(n_sh + 1)).astype(np.int64)


def _clip_ranges(ext, rows, clip_len, stride):
    """The byte ranges the clips `rows` need, one per clip and shard: every frame from the clip's first sampled frame that
    exists to its last, the frames a stride skips included, so that a clip is one contiguous copy per shard.  stride: one for
    all clips, or one per clip.
    -> (clip int64, shard int64, lo16 int64 -- the first byte rounded down to 16 --, hi int64), sorted by clip, then shard."""
    first, base, nfr = (np.asarray(rows[i], np.int64) for i in range(3))
    T, S = int(clip_len), _strides_of(stride, first.size, "_clip_ranges")      # S: one stride per clip
    a = base + np.where(base < 0, (-base + S - 1) // S, 0) * S                 # the first and the last sampled frame that exist
    b = base + np.minimum(T - 1, (nfr - 1 - base) // S) * S
    live = np.flatnonzero(a <= b)
    g0, g1 = first[live] + a[live], first[live] + b[live]
    sf = _shard_first(ext)
    lo_pad = np.concatenate([np.asarray(ext.lo, np.int64), [_NO_BYTE]])
    hi_pad = np.concatenate([np.asarray(ext.hi, np.int64), [0]])
    shard = np.asarray(ext.shard, np.int64)
    s0, s1 = shard[g0], shard[g1]
    out = [np.zeros(0, np.int64)] * 4
    for d in range(int((s1 - s0).max()) + 1 if live.size else 0):
        k = np.flatnonzero(s0 + d <= s1)
        s = s0[k] + d
        idx = np.stack([np.maximum(g0[k], sf[s]), np.minimum(g1[k], sf[s + 1] - 1) + 1], 1).reshape(-1)
        lo = np.minimum.reduceat(lo_pad, idx)[::2]
        hi = np.maximum.reduceat(hi_pad, idx)[::2]
        on = hi > lo
        out = [np.concatenate([o, x[on]]) for o, x in zip(out, (live[k], s, lo & ~15, hi))]
    order = np.lexsort((out[1], out[0]))
    return tuple(o[order] for o in out)


def stream_plan(ext, video_first, video_len, rows, clip_len, stride, operands, batch_size, depth, fixed_bytes,
                max_resident_bytes, who="ResidentJpegClips"):
    """Which videos of a set stay resident when the set is streamed (pure numpy; no file, no device).
    ext: `frame_extents`; video_first / video_len: the videos' frames in the set-wide numbering, in set order; rows: int64
    (4, n_clips) -- per clip the first frame of its video, its base, the video's length and the video (`_ClipLoader._rows`);
    stride: one for all clips, or one per clip (a joint set: `_ClipLoader._clip_stride`);
    operands: clips per batch item (2 with mixup); fixed_bytes: what is resident whatever the plan -- segment and piece
    tables, table sets, side buffer.
    One staging region holds a batch: operands x batch_size x the largest sum of byte ranges (`_clip_ranges`, rounded out
    to 16) that any clip of a streamed video needs.  First fixed_bytes and depth regions for the case that every video is
    streamed are reserved; resident are then the first v whole videos, v as large as the rest of the budget allows -- so a
    larger budget never keeps fewer videos resident.  Their streams take, per shard, the bytes from the shard's start to
    the end of its last resident frame, rounded up to 16.  The regions are then as large as the clips of the videos v.. need
    (none when every video is resident).  Counted against the budget: resident streams + fixed_bytes + depth regions.
    -> namespace(resident_videos, resident_frames, shard_bytes int64 (n_shards,) -- resident bytes per shard --, shard_base
       int64 (n_shards,) -- where a shard's position 0 lies in the numbering JcPiece.pos uses: its place in the device buffer
       for a shard with resident bytes, a position behind the buffer for the others --, stream_bytes (the resident streams),
       region_bytes, stage_lo (= stream_bytes: the first region's offset in the device buffer), buffer_bytes (= stream_bytes
       + depth * region_bytes), resident_bytes, needs int64 (videos + 1,): the budget that keeps v = 0 .. all videos resident,
       min_budget = needs[0]).
    ValueError when not even v = 0 fits; the message names min_budget."""
    vf, vl = np.asarray(video_first, np.int64), np.asarray(video_len, np.int64)
    nv = vf.size
    sf = _shard_first(ext)
    n_sh, n_frames = sf.size - 1, int(sf[-1])
    if nv == 0 or np.any(np.diff(vf) != vl[:-1]) or vf[0] != 0 or int(vf[-1] + vl[-1]) != n_frames:
        raise ValueError(f"{who}: the videos must tile the set's {n_frames} frames in order")
    depth, per_batch = int(depth), int(operands) * int(batch_size)
    # resident bytes of shard k when the frames below F are resident: the running maximum of the frames' end bytes
    hi = np.asarray(ext.hi, np.int64)
    run = hi.copy()
    for k in range(n_sh):
        run[sf[k]:sf[k + 1]] = np.maximum.accumulate(hi[sf[k]:sf[k + 1]])

    def shard_bytes(F):
        return np.asarray([_round16(int(run[min(F, int(sf[k + 1])) - 1])) if F > sf[k] else 0 for k in range(n_sh)], np.int64)
    # the largest clip of every video, and of the videos v.. (the streamed ones)
    clip, _, lo16, hi_ = _clip_ranges(ext, rows, clip_len, stride)
    need = np.zeros(np.asarray(rows[0]).size, np.int64)
    np.add.at(need, clip, _round16(hi_) - lo16)
    per_video = np.zeros(nv + 1, np.int64)
    np.maximum.at(per_video, np.asarray(rows[3], np.int64), need)
    region = np.maximum.accumulate(per_video[::-1])[::-1] * per_batch              # region[v]: videos v.. are streamed
    ends = np.concatenate([vf, [n_frames]])
    needs = np.asarray([int(shard_bytes(int(ends[v])).sum()) + int(fixed_bytes) + depth * int(region[0]) for v in range(nv + 1)],
                       np.int64)
    fits = np.flatnonzero(needs <= int(max_resident_bytes))
    if fits.size == 0:
        raise ValueError(f"{who}: with no video resident the set still needs {int(needs[0])} bytes on the device ({depth} staging "
                         f"regions of {int(region[0])}, {int(fixed_bytes)} of tables and frames kept decoded), more than "
                         f"max_resident_bytes={int(max_resident_bytes)}; the smallest max_resident_bytes that would do is "
                         f"{int(needs[0])}")
    v = int(fits[-1])
    sb = shard_bytes(int(ends[v]))
    stream_bytes, region_bytes = int(sb.sum()), int(region[v])
    buffer_bytes = stream_bytes + depth * region_bytes
    base = np.concatenate([[0], np.cumsum(sb)])[:-1]
    full = np.asarray([_round16(int(run[sf[k + 1] - 1])) if sf[k + 1] > sf[k] else 0 for k in range(n_sh)], np.int64)
    behind = _round16(buffer_bytes) + np.concatenate([[0], np.cumsum(full)])[:-1]
    return SimpleNamespace(resident_videos=v, resident_frames=int(ends[v]), shard_bytes=sb,
                           shard_base=np.where(sb > 0, base, behind).astype(np.int64), stream_bytes=stream_bytes,
                           region_bytes=region_bytes, stage_lo=stream_bytes, buffer_bytes=buffer_bytes, depth=depth,
                           resident_bytes=buffer_bytes + int(fixed_bytes), needs=needs, min_budget=int(needs[0]))


def stage_batch(plan, ext, rows, clip_len, stride, region_off, n_slots=None, clip_slot=None):
    """The copies and the relocation rows of one batch of a streamed set (pure numpy; no file, no device).
    rows / clip_slot / n_slots / stride: as `jpegsets.batch_tables` (rows with the video in row 3); region_off: where the
    batch's staging region starts in the device buffer (plan.stage_lo + ring entry * plan.region_bytes).
    -> (copies [(shard, host byte lo, host byte hi, device offset)]: one per clip of a streamed video and shard it touches,
          packed into the region one behind the other, each at a 16-byte boundary and starting at a host byte that is a
          multiple of 16;
        reloc int64 (n_slots, 3): per slot (delta, window lo, window hi) -- csrc/jpeg_core.h JcReloc.  A slot that shows a
          frame of a streamed video reads the copy that holds the frame: delta = plan.shard_base[shard] + host lo - device
          offset (a multiple of 16), the window is the copy.  Every other slot -- padding, a resident video's -- gets delta
          0 and the resident window [0, plan.stream_bytes).)
    ValueError when the ranges exceed plan.region_bytes."""
    T = int(clip_len)
    first, base, nfr, vid = (np.asarray(rows[i], np.int64) for i in range(4))
    n = first.size
    S = _strides_of(stride, n, "stage_batch")                                  # one stride per clip
    at = np.arange(n, dtype=np.int64) * T if clip_slot is None else np.asarray(clip_slot, np.int64)
    total = int(n_slots) if n_slots is not None else n * T
    reloc = np.zeros((total, 3), np.int64)
    reloc[:, 2] = plan.stream_bytes
    streamed = np.flatnonzero(vid >= plan.resident_videos)
    copies = []
    if streamed.size == 0:
        return copies, reloc
    clip, shard, lo16, hi = _clip_ranges(ext, [r[streamed] for r in (first, base, nfr)], T, S[streamed])
    size = _round16(hi) - lo16
    dev = int(region_off) + np.concatenate([[0], np.cumsum(size)])[:-1]
    if int(size.sum()) > plan.region_bytes:
        raise ValueError(f"stage_batch: the batch needs {int(size.sum())} bytes of staging, the region holds {plan.region_bytes}")
    copies = [(int(s), int(l), int(h), int(d)) for s, l, h, d in zip(shard, lo16, hi, dev)]
    fshard = np.asarray(ext.shard, np.int64)
    for c, s, l, h, d in zip(clip, shard, lo16, hi, dev):
        k = streamed[c]
        f = base[k] + np.arange(T, dtype=np.int64) * S[k]
        real = (f >= 0) & (f < nfr[k])
        g = np.where(real, first[k] + f, 0)
        on = real & (fshard[g] == s) & (np.asarray(ext.hi)[g] > np.asarray(ext.lo)[g])
        reloc[at[k] + np.flatnonzero(on)] = (int(plan.shard_base[s]) + int(l) - int(d), int(d), int(d) + int(h) - int(l))
    return copies, reloc
