"""Live scoring: frames are pushed as they arrive, final rows of the score track come back (`TDEEDModel.live_scorer`).

The rules -- which clips are complete, which rows are final, how large the rings are -- are liveplan's, pure host arithmetic;
this module is the device side: a frame ring (frame p in row p % ring_frames, read by ops.clip_gather_ring), the batches of
`TDEEDModel._packed_track` on the engine's two slots, and ops.stitch_live after every batch on a score ring."""
import numpy as np
import torch

from . import liveplan, ops


class LiveScorer:
    """One stream of frames scored while it arrives; built by `TDEEDModel.live_scorer`, which documents the contract."""

    def __init__(self, model, frame_shape, overlap_len=None, pad_len=5, batch_size=1, augment=False, use_amp=True,
                 ring_frames=None):
        from .streams import new_stream
        try:
            shape = tuple(int(x) for x in frame_shape)
        except (TypeError, ValueError):
            raise TypeError("live_scorer: frame_shape must be (3,H,W)") from None
        if len(shape) != 3 or shape[0] != 3 or min(shape) < 1:
            raise ValueError(f"live_scorer: frame_shape must be (3,H,W), got {shape}")
        T = int(model._args.clip_len)
        ov = T // 4 * 3 if overlap_len is None else int(overlap_len)
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("live_scorer: batch_size must be positive")
        try:
            self._sched = liveplan.LiveSchedule(T, ov, pad_len, batch_size)
            fb = int(np.prod(shape))
            chunk = max(1, int(model.video_chunk_bytes) // fb)
            need = liveplan.frame_ring_rows(batch_size, chunk, T, ov)
            # default: room for a second batch, so that the upload of the next batch's frames need not wait for the running one
            R = need + liveplan.track_ring_rows(batch_size, T, ov) if ring_frames is None else \
                liveplan.check_frame_ring(ring_frames, batch_size, chunk, T, ov)
        except ValueError as e:
            raise ValueError(f"live_scorer: {e}") from None
        if batch_size * T > 65535:
            raise ValueError(f"live_scorer: batch_size * clip_len = {batch_size * T} frame slots exceed the gather's 65535")
        self._model, self._shape, self._fb, self._chunk = model, shape, fb, chunk
        self.clip_len, self.overlap_len, self.pad_len, self.batch_size = T, ov, int(pad_len), batch_size
        self.augment, self.use_amp, self.ring_frames = bool(augment), bool(use_amp), R
        self.track_rows = liveplan.track_ring_rows(batch_size, T, ov)
        self._V = 2 if augment else 1
        self._dt = torch.bfloat16 if use_amp else torch.float32
        model._model.eval()
        self._eng = model._model.engine(self._dt)
        self._K1 = K1 = model._score_cols(self._dt)
        dev = self._dev = model.device
        if model._stream is None:
            model._stream = new_stream()
        if getattr(model, "_stream2", None) is None:
            model._stream2 = new_stream(avoid=[model._stream])
        if getattr(model, "_copy_stream", None) is None:
            model._copy_stream = new_stream(avoid=[model._stream, model._stream2])
        self._streams, self._cp = [model._stream, model._stream2], model._copy_stream
        self._ring = torch.zeros((R,) + shape, dtype=torch.uint8, device=dev)
        self._ring_sum = torch.zeros((self.track_rows, K1), dtype=torch.float32, device=dev)
        self._ring_sup = torch.zeros((self.track_rows,), dtype=torch.int32, device=dev)
        self._scores = [torch.empty((self._V, batch_size, T, K1), dtype=torch.float32, device=dev) for _ in range(2)]
        self._tabs = [torch.empty((3 * batch_size,), dtype=torch.int32, device=dev) for _ in range(2)]
        self._stage = []                          # pinned staging buffers: [tensor, event of its last upload]
        cur = torch.cuda.current_stream()
        for st in self._streams + [self._cp]:
            st.wait_stream(cur)
        self.last_push_stats = dict(host_syncs=0, batches=0, rows=0, frames_h2d_bytes=0)
        self._fresh()

    def _fresh(self):
        self._sched.reset()
        self._released = []                       # per batch that may still read the frame ring: (slot, event, lowest frame read)
        self._arrived = self._stitched = None
        self._bi = 0

    # ------------------------------------------------------------------ properties
    @property
    def frames_pushed(self):
        return self._sched.pushed

    @property
    def rows_final(self):
        return self._sched.rows_final

    @property
    def latency_frames(self):
        """a frame's row is returned by the push that brings the frame this many frames after it, at the latest"""
        return liveplan.latency_frames(self.batch_size, self.clip_len, self.overlap_len)

    # ------------------------------------------------------------------ the frame ring
    def _wait_readers(self, below):
        """the copy stream waits for the batches that read a frame below `below`: the latest of them per stream"""
        n = 0
        while n < len(self._released) and self._released[n][2] < below:
            n += 1
        seen = set()
        for slot, ev, _ in reversed(self._released[:n]):
            if slot not in seen:
                seen.add(slot)
                self._cp.wait_event(ev)
        del self._released[:n]                    # later copies follow this one on the copy stream

    def _stage_buffer(self, k):
        """a pinned buffer of at least k <= chunk frames whose last copy has left it; a new one of k frames when there is none
        (pushes of a steady size settle on a few buffers of that size), never a host wait"""
        for entry in self._stage:
            if entry[0].shape[0] >= k and (entry[1] is None or entry[1].query()):
                return entry
        entry = [torch.empty((k,) + self._shape, dtype=torch.uint8).pin_memory(), None]
        self._stage.append(entry)
        return entry

    def _upload(self, piece):
        """frames pushed .. pushed + k - 1 into their ring rows, on the copy stream, behind the batches that still read the
        rows' earlier frames; host frames through a pinned staging buffer of the scorer's own"""
        R, p0, k = self.ring_frames, self._sched.pushed, int(piece.shape[0])
        self._wait_readers(p0 + k - R)
        r0 = p0 % R
        k1 = min(k, R - r0)                       # the piece may wrap around the end of the ring
        entry = None
        if piece.is_cuda:
            cur = torch.cuda.current_stream()
            self._cp.wait_stream(cur)             # the frames are the work of the caller's stream
            src = piece
        else:
            entry = self._stage_buffer(k)
            src = entry[0][:k]
            src.copy_(piece)
        with torch.cuda.stream(self._cp):
            self._ring[r0:r0 + k1].copy_(src[:k1], non_blocking=True)
            if k1 < k:
                self._ring[:k - k1].copy_(src[k1:], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._cp)
        self._arrived = ev                        # a batch is launched right behind the piece that completes it
        if entry is not None:
            entry[1] = ev
            return k * self._fb
        piece.record_stream(self._cp)
        cur.wait_event(ev)                        # the caller may overwrite its frames on its stream right away
        return 0

    # ------------------------------------------------------------------ one launch of the schedule
    def _run(self, launch, tab_host, out, row0):
        """one batch through gather, forward, post-processing and the stitch (or the stitch alone for a launch without
        clips), on the next slot's stream; rows that become final go to out[...][lo - row0:final_hi - row0]"""
        m, T, V = self._model, self.clip_len, self._V
        starts, lo, hi, limit = launch["starts"], launch["lo"], launch["final_hi"], launch["limit"]
        B = len(starts)
        slot = self._bi % 2
        st = self._streams[slot]
        dst = tuple(x[lo - row0:hi - row0] for x in out)
        with torch.cuda.stream(st):
            if B:
                tab = self._tabs[slot][:3 * B]
                tab_host[:B] = torch.as_tensor(starts, dtype=torch.int32)
                tab_host[B:2 * B] = 0
                tab_host[2 * B:3 * B] = limit
                st.wait_event(self._arrived)
                tab.copy_(tab_host[:3 * B], non_blocking=True)
                starts_dev, base_dev, lenv_dev = tab[:B], tab[B:2 * B], tab[2 * B:]
                scores = self._scores[slot].view(-1)[:V * B * T * self._K1].view(V, B, T, self._K1)
                pw = self._eng.pw
                for v in range(V):
                    head, _ = self._eng.forward_from_video(self._ring, starts_dev, augment_inference=bool(v), slot=slot,
                                                           ring=(self.ring_frames, limit), clip_base=base_dev,
                                                           clip_len_v=lenv_dev)
                    pred, _ = m._model._pack_head(head, B, T, pw.n_cls, pw.displ_col, None)
                    m._process_pred(pred, B, T, self._dt, out=scores[v])
                ev = torch.cuda.Event()
                ev.record(st)                     # the last gather of this batch is behind: its ring rows may be overwritten
                self._released.append((slot, ev, max(0, starts[0])))
            else:
                scores = starts_dev = None
            if self._stitched is not None:
                st.wait_event(self._stitched)     # the score ring is shared: launch k follows launch k - 1
            ops.stitch_live(self._ring_sum, self._ring_sup, scores, starts_dev, self.augment, lo, hi, limit, T=T, out=dst)
            self._stitched = torch.cuda.Event()
            self._stitched.record(st)
        self._bi += 1
        return st

    def _new_out(self, n, n_batches):
        K1, dev = self._K1, self._dev
        with torch.cuda.stream(self._streams[0]):
            out = (torch.empty((n, K1), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev),
                   torch.empty((n, K1), dtype=torch.float32, device=dev))
        tab_host = torch.empty((max(n_batches, 1), 3 * self.batch_size), dtype=torch.int32).pin_memory()
        return out, tab_host

    def _deliver(self, first_row, out, st, stats):
        """the rows of this call to the host: one synchronisation, of the stream of the last launch"""
        n = int(out[0].shape[0])
        with torch.cuda.stream(st):
            host = [torch.empty(tuple(x.shape), dtype=x.dtype).pin_memory() for x in out]
            for h, x in zip(host, out):
                if n:
                    h.copy_(x, non_blocking=True)
            st.synchronize()
        stats["host_syncs"] = 1
        stats["rows"] = n
        self.last_push_stats = stats
        return (first_row,) + tuple(h.numpy().copy() for h in host)

    def _nothing(self, first_row, stats):
        self.last_push_stats = stats
        K1 = self._K1
        return first_row, np.zeros((0, K1), np.float32), np.zeros((0,), np.int32), np.zeros((0, K1), np.float32)

    # ------------------------------------------------------------------ the public calls
    def push(self, frames):
        sched = self._sched
        if sched.closed:
            raise RuntimeError("live_scorer: push after close() (reset() starts a new stream)")
        if not isinstance(frames, torch.Tensor):
            frames = torch.as_tensor(np.asarray(frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4:
            raise TypeError("live_scorer: push takes a uint8 (m,3,H,W) tensor")
        if tuple(frames.shape[1:]) != self._shape:
            raise ValueError(f"live_scorer: frames of {tuple(frames.shape[1:])}, the scorer was built for {self._shape}")
        m = int(frames.shape[0])
        if m < 1:
            raise ValueError("live_scorer: a push carries at least one frame")
        if frames.is_cuda and frames.device != self._ring.device:
            frames = frames.to(self._ring.device)
        T, ov, pad, bs = self.clip_len, self.overlap_len, self.pad_len, self.batch_size
        first_row = sched.rows_final
        n_batches = (liveplan.clips_ready(sched.pushed + m, T, ov, pad) - sched.scored) // bs
        stats = dict(host_syncs=0, batches=n_batches, rows=0, frames_h2d_bytes=0)
        out = tab_host = st = None
        if n_batches:
            n_rows = liveplan.final_rows(sched.scored + n_batches * bs, T, ov, pad) - first_row
            out, tab_host = self._new_out(n_rows, n_batches)
            self._model._model.eval()
        done = ran = 0
        while done < m:
            free = self.ring_frames - (sched.pushed - sched.first_live_frame())
            k = min(m - done, free) if frames.is_cuda else min(m - done, free, self._chunk)
            stats["frames_h2d_bytes"] += self._upload(frames[done:done + k])
            done += k
            for launch in sched.push(k):
                st = self._run(launch, tab_host[ran], out, first_row)
                ran += 1
        if not n_batches:
            return self._nothing(first_row, stats)
        return self._deliver(first_row, out, st, stats)

    def close(self):
        sched = self._sched
        if sched.closed:
            raise RuntimeError("live_scorer: the stream is closed already (reset() starts a new one)")
        try:
            sched.check_close()
        except ValueError as e:
            raise ValueError(f"live_scorer: {e}") from None
        first_row = sched.rows_final
        launches = sched.close()
        n_batches = sum(1 for x in launches if x["starts"])
        stats = dict(host_syncs=0, batches=n_batches, rows=0, frames_h2d_bytes=0)
        if not launches:
            return self._nothing(first_row, stats)
        out, tab_host = self._new_out(sched.pushed - first_row, n_batches)
        self._model._model.eval()
        ran = 0
        for launch in launches:
            st = self._run(launch, tab_host[min(ran, tab_host.shape[0] - 1)], out, first_row)
            ran += 1 if launch["starts"] else 0
        return self._deliver(first_row, out, st, stats)

    def reset(self):
        """A new stream on the same buffers and graphs: both rings cleared, every counter back to zero."""
        s0, s1 = self._streams
        with torch.cuda.stream(s0):
            s0.wait_stream(s1)
            s0.wait_stream(self._cp)
            self._ring.zero_()
            self._ring_sum.zero_()
            self._ring_sup.zero_()
        s1.wait_stream(s0)
        self._cp.wait_stream(s0)
        self._fresh()
        self.last_push_stats = dict(host_syncs=0, batches=0, rows=0, frames_h2d_bytes=0)
