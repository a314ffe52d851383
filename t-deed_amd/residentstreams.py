"""A packed JPEG set made resident on the device, and the decode pass over it.

`ResidentStreams` is what `trainclips.ResidentJpegClips` and `evalutil.ResidentJpegVideos` share: the upload of a
`jpegsets.ResidentJpegs`, its index pass and side buffer, the coefficient buffer, and the chunk loop that decodes the
slots of one `jpegsets.batch_tables` namespace.
"""
import numpy as np

from .streamplan import _round16, frame_extents, stream_plan


class ResidentStreams:
    """A packed set (`load_resident_jpegs`) made resident.
    The constructor is host arithmetic -- geometry, piece offsets, the resident bytes (stream, segment and piece tables,
    table sets, side buffer) held against max_resident_bytes, a ValueError naming `who` before anything is uploaded.
    `upload`, called inside the caller's stream context, copies the shards' streams into one buffer and the tables in one
    copy, runs the index pass (ops.jpeg_entropy_index, once per shard), reads the per-segment statuses back -- the one host
    synchronisation -- and decodes the fallback and the flagged frames once with `feeder.read_frame` into the side buffer
    (the budget is checked again when the index pass added side frames).  window = (top, left, wh, ww), here or through
    `set_window` before `upload`: the side buffer keeps that window of its frames only.  Afterwards: jstream, table_sets, pieces, side (device tensors or None),
    frame_set / side_row / piece_lo / piece_n per frame of the set, piece_mcu per piece row, `stats()`.
    `decode_buffers`, after `upload` in the same context, allocates what a decode pass needs; `decode` is the pass and
    `raise_errors` reads the error word it leaves.
    streamed=True: the set may exceed the budget.  The constructor then checks nothing; the caller, who knows the clips, calls
    `plan_streaming` before `upload` (`stream_plan` against the budget; ValueError before anything is uploaded).  `upload`
    copies only the resident bytes of every shard (plan.shard_bytes) into jstream and leaves plan.depth staging regions
    behind them in the same allocation.  The index pass still covers every shard: one with streamed frames is copied whole
    into the staging memory, indexed there, its piece rows' positions moved to the shard's own numbering (plan.shard_base),
    and the stream waited for before the next shard reuses the memory.  The shards stay alive on the host (`host_streams`,
    one tensor per shard): the batches copy from them -- asynchronously when they are page-locked (`load_resident_jpegs`'
    default), blocking the host when not (`pinned=False`).  `stats()` gains resident_videos, streamed_videos, stage_bytes and
    host_stream_bytes, resident_bytes includes the staging, stream_bytes stays the whole set's."""

    def __init__(self, who, jpegs, split_mcus, max_resident_bytes, window=None, streamed=False):
        from . import feeder, jpegdev
        self.who, self.jpegs, self.max_resident_bytes, self.window = who, jpegs, max_resident_bytes, window
        self.streamed, self.plan, self.ext = bool(streamed), None, None
        self.fr0 = None
        if jpegs.width:
            W, H, samp = jpegs.width, jpegs.height, jpegs.samp
        else:                                               # nothing for the device: the geometry comes from Pillow
            self.fr0 = feeder.read_frame(jpegs.names[0])
            H, W, samp = int(self.fr0.shape[1]), int(self.fr0.shape[2]), 0
        self.H, self.W, self.samp = H, W, samp
        self.geom = geom = jpegdev.geometry(W, H, samp)
        self.split = split = int(split_mcus) if split_mcus is not None else geom.mcus_x
        if split < 1:
            raise ValueError("split_mcus must be positive")
        self.side_shape, self.fb = (3, H, W), 3 * H * W
        self.shards = shards = [s for s in jpegs.shards]
        self.seg_lo, self.piece_cnt, self.base, total = [], [], [], 0
        n_seg = 0
        for s in shards:
            self.seg_lo.append(n_seg)
            n_seg += s.packed.n_segments
            self.piece_cnt.append(jpegdev.piece_counts(s.packed.segments, split) if s.packed.n_segments else np.zeros(0, np.int64))
            self.base.append(total)
            total += (int(s.packed.stream_np.size) + 15) & ~15 if s.packed.n_segments else 0
        self.n_seg, self.total = n_seg, total
        self.piece_off = np.concatenate([[0], np.cumsum(np.concatenate(self.piece_cnt))]) if n_seg else np.zeros(1, np.int64)
        self.n_pieces = int(self.piece_off[-1])
        if self.n_pieces >= 1 << 31:
            raise ValueError(f"{who}: {self.n_pieces} pieces exceed the item table's 32-bit rows")
        self.side_frames = sorted(int(f) for f in jpegs.fallback)
        self.flagged = []
        self.pieces = self.table_sets = self.jstream = self.side = self.side_host = None
        self.set_window(window)

    def set_window(self, window):
        """Before `upload`: keep the window (top, left, wh, ww) of the side frames only (None: whole frames), and hold the
        resident bytes against the budget with side frames of that size."""
        H, W = self.H, self.W
        if window is not None:
            top, left, wh, ww = (int(x) for x in window)
            if min(wh, ww) < 1 or top < 0 or left < 0 or top + wh > H or left + ww > W:
                raise ValueError(f"{self.who}: the window {wh}x{ww} at ({top}, {left}) is empty or leaves the {H}x{W} frames")
            window = (top, left, wh, ww)
        self.window = window
        self.side_shape = (3, H, W) if window is None else (3, window[2], window[3])
        self.fb = int(np.prod(self.side_shape))
        self.check(len(self.side_frames))

    def fixed(self, n_side):
        """the resident bytes besides the streams: segment and piece tables, table sets, side buffer"""
        from . import jpegdev
        return self.n_seg * 4 * jpegdev.SEG_COLS + self.n_pieces * jpegdev.PIECE_BYTES + \
            self.jpegs.n_sets * jpegdev.TABLE_SET_BYTES + n_side * self.fb

    def resident(self, n_side):
        if self.plan is not None:
            return self.plan.buffer_bytes + self.fixed(n_side)
        return self.total + self.fixed(n_side)

    def plan_streaming(self, rows, clip_len, stride, operands, batch_size, depth):
        """Streamed sets, before `upload`: `stream_plan` over the clips `rows` against the budget (ValueError naming the
        smallest budget that would do), and every shard that is not wholly resident held against the staging memory, through
        which its index pass runs (ValueError naming `shard_bytes`)."""
        self.ext = frame_extents(self.shards)
        self.plan = plan = stream_plan(self.ext, self.jpegs.video_first, self.jpegs.video_len, rows, clip_len, stride, operands,
                                       batch_size, depth, self.fixed(len(self.side_frames)), self.max_resident_bytes, self.who)
        stage = plan.buffer_bytes - plan.stage_lo
        for s, end in zip(self.shards, self.ext.shard_first[1:]):
            size = _round16(int(s.packed.stream_np.size))
            if s.packed.n_segments and end > plan.resident_frames and size > stage:
                raise ValueError(f"{self.who}: a streamed shard of {size} bytes does not fit the {stage} bytes of staging memory "
                                 "its index pass runs through; pass a smaller shard_bytes to load_resident_jpegs")
        return plan

    def check(self, n_side):
        if self.streamed:
            # before the plan: nothing to hold (plan_streaming does); after the upload: the index pass added side frames, and
            # a plan with fewer resident videos would need a new upload
            if self.plan is not None and self.resident(n_side) > self.max_resident_bytes:
                raise ValueError(f"{self.who}: the index pass left {n_side} frames to keep decoded, and with them the set needs "
                                 f"{self.resident(n_side)} bytes on the device, more than max_resident_bytes="
                                 f"{self.max_resident_bytes}")
            return
        if self.resident(n_side) > self.max_resident_bytes:
            raise ValueError(f"{self.who}: the set needs {self.resident(n_side)} bytes on the device ({self.total} of entropy "
                             f"streams, {n_side} frames kept decoded), more than max_resident_bytes={self.max_resident_bytes}")

    def upload(self, stream, dev, chunk_bytes):
        import torch
        from . import feeder, jpegdev, ops
        jpegs, shards, base, seg_lo, n_seg = self.jpegs, self.shards, self.base, self.seg_lo, self.n_seg
        W, H, samp, split, piece_off, n_pieces = self.W, self.H, self.samp, self.split, self.piece_off, self.n_pieces
        n_frames, names, side, flagged = jpegs.n_frames, jpegs.names, self.side_frames, []
        plan = self.plan
        if self.streamed and plan is None:
            raise RuntimeError(f"{self.who}: a streamed set is planned (plan_streaming) before it is uploaded")
        if n_seg:
            # the streams, shard by shard, into one buffer; every table in one copy from a page-locked block.  Streamed: the
            # resident bytes of every shard only (plan.shard_bytes), the staging regions behind them in the same allocation
            self.jstream = torch.zeros(self.total if plan is None else max(plan.buffer_bytes, 16), dtype=torch.uint8, device=dev)
            keep = []
            self.host_streams = []                          # per shard its stream as a host tensor (streamed sets copy from it)
            for k, (s, b) in enumerate(zip(shards, base)):
                src = s.packed.stream if isinstance(s.packed.stream, torch.Tensor) else torch.from_numpy(s.packed.stream_np)
                self.host_streams.append(src)
                if not s.packed.n_segments:
                    continue
                if plan is not None:
                    b = base[k] = int(plan.shard_base[k])
                end = src.numel() if plan is None else min(int(plan.shard_bytes[k]), src.numel())
                for lo in range(0, end, int(chunk_bytes)):
                    hi = min(lo + int(chunk_bytes), end)
                    self.jstream[b + lo:b + hi].copy_(src[lo:hi], non_blocking=True)
                keep.append(src)
            segs = np.concatenate([s.packed.segments for s in shards if s.packed.n_segments])
            waves = [s.packed.waves() for s in shards]
            parts = [segs.reshape(-1).view(np.uint8), piece_off.astype(np.int32).view(np.uint8),
                     jpegs.table_sets.reshape(-1)] + [np.ascontiguousarray(w).reshape(-1).view(np.uint8) for w in waves]
            offs, size = [], 0
            for a in parts:
                offs.append(size)
                size += (a.size + 15) & ~15
            host = torch.zeros(size, dtype=torch.uint8).pin_memory()
            hv = host.numpy()
            for a, o in zip(parts, offs):
                hv[o:o + a.size] = a
            meta = torch.empty(size, dtype=torch.uint8, device=dev)
            meta.copy_(host, non_blocking=True)

            def view(i, dtype, shape):
                return meta[offs[i]:offs[i] + parts[i].size].view(dtype).view(*shape)
            d_segs = view(0, torch.int32, (n_seg, jpegdev.SEG_COLS))
            d_off = view(1, torch.int32, (n_seg + 1,))
            self.table_sets = view(2, torch.uint8, (jpegs.n_sets, jpegdev.TABLE_SET_BYTES))
            self.pieces = torch.zeros((n_pieces, jpegdev.PIECE_BYTES), dtype=torch.uint8, device=dev)
            status = torch.zeros(n_seg, dtype=torch.int32, device=dev)
            for i, (s, b, s0) in enumerate(zip(shards, base, seg_lo)):
                n = s.packed.n_segments
                if not n:
                    continue
                staged = plan is not None and int(self.ext.shard_first[i + 1]) > plan.resident_frames
                if staged:
                    # a shard with streamed frames: through the staging memory, then its rows' positions moved from there
                    # to the shard's own base (plan.shard_base: 64-bit, behind the buffer for a shard without resident bytes)
                    src, at = self.host_streams[i], plan.stage_lo
                    self.jstream[at:at + src.numel()].copy_(src, non_blocking=True)
                ops.jpeg_entropy_index(self.jstream, at if staged else b, d_segs[s0:s0 + n],
                                       view(3 + i, torch.int32, (waves[i].shape[0], 2)), self.table_sets, W, H, samp, split,
                                       d_off[s0:s0 + n + 1], s0, self.pieces, status[s0:s0 + n])
                if staged:
                    self.pieces.view(torch.int64)[int(piece_off[s0]):int(piece_off[s0 + n]), 0] += b - at
                    stream.synchronize()                      # before the next shard reuses the staging memory
            h_status = torch.empty(n_seg, dtype=torch.int32).pin_memory()
            h_status.copy_(status, non_blocking=True)
            stream.synchronize()                          # the one host synchronisation of construction
            del keep, host
            bad = h_status.numpy() != 0
            for s, s0 in zip(shards, seg_lo):
                n = s.packed.n_segments
                if n and bad[s0:s0 + n].any():
                    flagged += [int(f) for f in np.unique(s.frames[s.packed.segments[bad[s0:s0 + n], 0]])]
            if flagged:
                side = sorted(set(side) | set(flagged))
                self.check(len(side))
        self.side_frames, self.flagged = side, flagged
        # per frame of the set: table set, side row, piece rows; per piece row: its MCUs
        self.frame_set = jpegs.frame_set.copy()
        self.side_row = np.full(n_frames, -1, np.int32)
        self.side_row[side] = np.arange(len(side), dtype=np.int32)
        self.frame_set[side] = -1
        self.piece_lo = np.zeros(n_frames, np.int64)
        self.piece_n = np.zeros(n_frames, np.int64)
        mcu = []
        for s, s0, cnt in zip(shards, seg_lo, self.piece_cnt):
            n = s.packed.n_segments
            if not n:
                continue
            fr = s.frames[s.packed.segments[:, 0]]
            lo = np.full(n_frames, np.iinfo(np.int64).max, np.int64)
            np.minimum.at(lo, fr, piece_off[s0:s0 + n])
            np.add.at(self.piece_n, fr, cnt)
            seen = np.unique(fr)
            self.piece_lo[seen] = lo[seen]
            mcu.append(jpegdev.piece_ranges(s.packed.segments, split))
        self.piece_mcu = np.concatenate(mcu) if mcu else np.zeros((0, 2), np.int64)
        if side:
            shape = self.side_shape
            h_side = torch.empty((len(side),) + shape, dtype=torch.uint8).pin_memory()
            for r, f in enumerate(side):
                fr = feeder.read_frame(names[f]) if not (f == 0 and self.fr0 is not None) else self.fr0
                if tuple(fr.shape) != (3, H, W):
                    raise ValueError(f"frame {names[f]}: {tuple(fr.shape)} does not fit the set's {(3, H, W)}")
                if self.window is not None:
                    top, left, wh, ww = self.window
                    fr = fr[:, top:top + wh, left:left + ww]
                h_side[r].copy_(fr)
            self.side = torch.empty((len(side),) + shape, dtype=torch.uint8, device=dev)
            self.side.copy_(h_side, non_blocking=True)
            self.side_host = h_side

    def chunk_frames(self, n_slots, max_coeff_bytes):
        """frames per coefficient chunk: what max_coeff_bytes holds, at least one and at most the n_slots of a pass"""
        from . import ops
        return min(int(n_slots), max(1, int(max_coeff_bytes) // (2 * ops.jpeg_frame_coeffs(self.W, self.H, self.samp))))

    def decode_buffers(self, dev, n_slots, max_coeff_bytes):
        """After `upload`, in the same stream context: what `decode` needs for passes of up to n_slots slots (the clip
        capacity of a batch, the longest video) -- `chunk` frames of `fc` coefficients each, the identity row table, the
        device error word and its page-locked twin."""
        import torch
        from . import ops
        self.fc = ops.jpeg_frame_coeffs(self.W, self.H, self.samp)
        self.chunk = self.chunk_frames(n_slots, max_coeff_bytes)
        self.coeff = torch.empty(self.chunk * self.fc, dtype=torch.int16, device=dev) if self.n_seg else None
        self.ident = torch.arange(int(n_slots), dtype=torch.int32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.err_host = torch.zeros(1, dtype=torch.int32).pin_memory()

    def decode(self, tb, items, waves, slot_set, out, reloc=None, before_items=None, events=None):
        """The decode pass of one `batch_tables` namespace `tb` (built with chunk_slots=self.chunk) on the current stream:
        per coefficient chunk zero the coefficients, ops.jpeg_entropy_items, one pixel pass into `out` -- ops.
        jpeg_pixels_rows, or ops.jpeg_pixels_window of the set's window.  items / waves / slot_set: tb's tables on the
        device; reloc: a streamed set's relocation rows; before_items(slot_lo) is called before a chunk's items launch,
        behind the zeroing; events: a list that gains one (start, between, end) triple of timing events around the two
        launches of every chunk.  The padding and the side frames (ops.jpeg_slot_fill) are the caller's."""
        import torch
        from . import ops
        for lo, hi, w_lo, w_hi in tb.chunks:
            n = hi - lo
            self.coeff[:n * self.fc].zero_()
            if before_items is not None:
                before_items(lo)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if events is not None else None
            if ev:
                ev[0].record()
            ops.jpeg_entropy_items(self.jstream, self.pieces, items, waves[w_lo:w_hi], self.table_sets, self.W, self.H,
                                   self.samp, lo, n, self.coeff, self.err, reloc=reloc)
            if ev:
                ev[1].record()
            if self.window is None:
                ops.jpeg_pixels_rows(self.coeff, slot_set, self.table_sets, out, self.ident, lo, n, self.samp)
            else:
                ops.jpeg_pixels_window(self.coeff, slot_set, self.table_sets, out, self.ident, lo, n, self.samp, self.H, self.W,
                                       self.window[0], self.window[1])
            if ev:
                ev[2].record()
                events.append(tuple(ev))

    def raise_errors(self, stream, what, copy=True, reset=False):
        """Copy the device error word to the host on `stream` (copy=False: the caller has queued `err_host.copy_(err)` behind
        its pass already), wait for the stream, and raise RuntimeError naming `what` ("pass 3", "video NAME") when a decode
        pass set the word; reset: zero it first, so that the next pass starts clean."""
        import torch
        if copy:
            with torch.cuda.stream(stream):
                self.err_host.copy_(self.err, non_blocking=True)
        stream.synchronize()
        word = int(self.err_host[0])
        if word:
            if reset:
                with torch.cuda.stream(stream):
                    self.err.zero_()
            codes = [c for c in range(1, 8) if word >> c & 1]
            raise RuntimeError(f"{self.who}: {what} met decode errors on the device (status codes {codes}); "
                               "the resident streams or tables are damaged")

    def stats(self):
        n_frames, n_side = self.jpegs.n_frames, len(self.side_frames)
        st = dict(frames=n_frames, device_frames=n_frames - n_side, fallback_frames=n_side,
                  index_flagged=sorted(self.flagged), segments=self.n_seg, pieces=self.n_pieces, shards=len(self.shards),
                  table_sets=self.jpegs.n_sets, stream_bytes=self.total, resident_bytes=self.resident(n_side),
                  decoded_bytes=n_frames * 3 * self.H * self.W)
        if self.plan is not None:                               # streamed: stream_bytes stays the whole set's
            nv = len(self.jpegs.video_len)
            st.update(resident_videos=self.plan.resident_videos, streamed_videos=nv - self.plan.resident_videos,
                      stage_bytes=self.plan.buffer_bytes - self.plan.stage_lo, host_stream_bytes=self.total - self.plan.stream_bytes)
        return st
