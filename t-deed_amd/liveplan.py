"""The rules of live scoring (`TDEEDModel.live_scorer`, `live.LiveScorer`): which clips can be scored after `pushed` frames of
a stream whose length is not known yet, which rows of the track are final, how large the two rings must be -- and the numpy
twin of the incremental stitch kernel (ops.stitch_live).  Pure Python / numpy: no torch, no GPU.

The clip grid is `evalutil.video_clip_starts`': start_j = -pad + j * s with s = T - ov.  It does not depend on the video's
length, so clip j can be scored the moment its last frame start_j + T - 1 has arrived, and a frame is final once the next
clip to be scored starts after it.  Every function takes T = clip_len, ov = overlap_len (0 <= ov < T) and pad = pad_len >= 0."""
import numpy as np

from .evalutil import video_clip_starts


def _stride(T, ov, pad=0):
    T, ov, pad = int(T), int(ov), int(pad)
    if T < 1 or not 0 <= ov < T or pad < 0:
        raise ValueError(f"liveplan: clips of {T} frames with overlap {ov} and pad {pad}: 0 <= overlap_len < clip_len, pad_len >= 0")
    return T - ov


def clip_start(j, T, ov, pad):
    """first frame of clip j of the grid"""
    return -int(pad) + int(j) * _stride(T, ov, pad)


def clips_ready(pushed, T, ov, pad):
    """The number of clips whose last frame start_j + T - 1 is below `pushed`: they are a prefix of the clip list of every
    video of at least `pushed` frames, with the same windows."""
    s = _stride(T, ov, pad)
    pushed = int(pushed)
    if pushed < 0:
        raise ValueError(f"liveplan: {pushed} frames pushed")
    return 0 if pushed < T - pad else (pushed - T + pad) // s + 1


def final_rows(scored, T, ov, pad):
    """The number of rows that are final while the stream is open after `scored` clips have been scored in order: the frames
    below the start of the next clip."""
    return max(0, -int(pad) + int(scored) * _stride(T, ov, pad))


def close_clips(L, T, ov, pad):
    """The number of clips of a video that ends after L frames: clips scored .. close_clips(L) - 1 are the ones close() still
    has to run, their windows cut at L."""
    _stride(T, ov, pad)
    return len(video_clip_starts(int(L), int(T), int(ov), pad_len=int(pad)))


def track_ring_rows(batch_size, T, ov):
    """The smallest score ring: the rows one batch of `batch_size` clips touches, T + (batch_size - 1) * s.  ov of them carry
    sums over from earlier batches, the rest start at zero."""
    if int(batch_size) < 1:
        raise ValueError("liveplan: batch_size must be positive")
    return int(T) + (int(batch_size) - 1) * _stride(T, ov)


def frame_ring_rows(batch_size, chunk, T, ov):
    """The smallest frame ring: one whole batch of unscored clips -- track_ring_rows(batch_size) frames, the span of their
    windows -- plus one staged chunk of `chunk` frames.  While no batch is complete fewer than a batch's span of frames are
    live, so a piece of up to `chunk` frames always finds room."""
    if int(chunk) < 1:
        raise ValueError("liveplan: a staged chunk holds at least one frame")
    return track_ring_rows(batch_size, T, ov) + int(chunk)


def latency_frames(batch_size, T, ov):
    """The bound on how many frames after frame p the row of p is returned while batches run only when full:
    T - 1 + (batch_size - 1) * s."""
    return track_ring_rows(batch_size, T, ov) - 1


def check_track_ring(rows, batch_size, T, ov):
    """ValueError, naming the minimum, when a score ring of `rows` rows is too small for batches of `batch_size` clips."""
    need = track_ring_rows(batch_size, T, ov)
    if int(rows) < need:
        raise ValueError(f"liveplan: a score ring of {int(rows)} rows, batches of {int(batch_size)} clips of {int(T)} frames "
                         f"(overlap {int(ov)}) touch {need}: at least {need} rows")
    return int(rows)


def check_frame_ring(rows, batch_size, chunk, T, ov):
    """ValueError, naming the minimum, when a frame ring of `rows` rows is too small for batches of `batch_size` clips fed in
    chunks of `chunk` frames."""
    need = frame_ring_rows(batch_size, chunk, T, ov)
    if int(rows) < need:
        raise ValueError(f"liveplan: ring_frames={int(rows)}, one batch of {int(batch_size)} clips of {int(T)} frames (overlap "
                         f"{int(ov)}) and one staged chunk of {int(chunk)} frames need {need}: at least ring_frames={need}")
    return int(rows)


class LiveSchedule:
    """The bookkeeping of one stream: `push(m)` and `close()` return the launches that are due, in order, each a dict of
    first (index of the batch's first clip), starts (the batch's clip starts, ascending; empty for a launch that only emits
    rows), lo / final_hi (rows final before / after the launch) and limit (frames that exist: the pushed count while open,
    the length at close) -- the arguments of ops.stitch_live / live_stitch_ref.  While the stream is open a batch is due only
    when `batch_size` complete clips are pending; close() cuts the remainder the same way, so the batches are those of
    `predict_video` on the complete video: the same clips in the same positions."""

    def __init__(self, T, ov, pad, batch_size):
        self.s = _stride(T, ov, pad)
        self.T, self.ov, self.pad, self.batch_size = int(T), int(ov), int(pad), int(batch_size)
        if self.batch_size < 1:
            raise ValueError("liveplan: batch_size must be positive")
        self.reset()

    def reset(self):
        self.pushed = self.scored = self.rows_final = self.batches = 0
        self.closed = False

    def _starts(self, first, n):
        return [clip_start(first + i, self.T, self.ov, self.pad) for i in range(n)]

    def first_live_frame(self):
        """the lowest frame a clip that is still to be scored reads: frames below it may be overwritten in the frame ring"""
        return max(0, clip_start(self.scored, self.T, self.ov, self.pad))

    def push(self, m):
        if self.closed:
            raise RuntimeError("liveplan: the stream is closed")
        if int(m) < 1:
            raise ValueError("liveplan: a push carries at least one frame")
        self.pushed += int(m)
        out = []
        while clips_ready(self.pushed, self.T, self.ov, self.pad) - self.scored >= self.batch_size:
            first, lo = self.scored, self.rows_final
            self.scored += self.batch_size
            self.rows_final = final_rows(self.scored, self.T, self.ov, self.pad)
            self.batches += 1
            out.append(dict(first=first, starts=self._starts(first, self.batch_size), lo=lo, final_hi=self.rows_final,
                            limit=self.pushed))
        return out

    def check_close(self):
        """the ValueError of close() on a stream `predict_video` would refuse, raised before anything changes"""
        if self.closed:
            raise RuntimeError("liveplan: the stream is closed")
        if self.pushed < 1:
            raise ValueError("liveplan: empty video")
        if close_clips(self.pushed, self.T, self.ov, self.pad) < 1:
            raise ValueError(f"liveplan: the video has no clips ({self.pushed} frames, overlap_len {self.ov}, pad_len 0)")

    def close(self):
        self.check_close()
        L, n = self.pushed, close_clips(self.pushed, self.T, self.ov, self.pad)
        out = []
        while self.scored < n:
            first, lo = self.scored, self.rows_final
            B = min(self.batch_size, n - first)
            self.scored += B
            self.rows_final = L if self.scored == n else final_rows(self.scored, self.T, self.ov, self.pad)
            self.batches += 1
            out.append(dict(first=first, starts=self._starts(first, B), lo=lo, final_hi=self.rows_final, limit=L))
        if self.rows_final < L:                                  # rows behind the last clip's start, all clips scored already
            out.append(dict(first=self.scored, starts=[], lo=self.rows_final, final_hi=L, limit=L))
            self.rows_final = L
        self.closed = True
        return out


def live_stitch_ref(ring_sum, ring_sup, scores, starts, count_all, lo, final_hi, limit):
    """numpy twin of the kernel of ops.stitch_live, and the statement of its order.  ring_sum float32 (R,K1) and ring_sup int32
    (R,) are the state between launches (frame p in row p % R) and are updated in place; scores float32 (V,B,T,K1) are the
    scores of ONE batch (None or B = 0: the launch only emits rows), starts its B ascending clip starts.  Every frame p in
    [lo, min(limit, max(final_hi, starts[-1] + T))) adds, clip after clip and view after view, the rows that cover it onto its
    ring row -- support counts every added row (count_all) or the ones that are not all zero -- and the frames below final_hi
    are then written out and their ring rows zeroed.  As on the device all frames accumulate before any row is emitted:
    with a ring smaller than the frames of one launch two frames share a row and the sums are wrong.
    -> (sums (final_hi - lo, K1) float32, support (final_hi - lo,) int32, mean (final_hi - lo, K1) float32)."""
    R, K1 = ring_sum.shape
    if ring_sum.dtype != np.float32 or ring_sup.dtype != np.int32 or ring_sup.shape != (R,):
        raise ValueError("live_stitch_ref: ring_sum float32 (R,K1) and ring_sup int32 (R,)")
    starts = [int(x) for x in starts]
    B = len(starts)
    lo, final_hi, limit = int(lo), int(final_hi), int(limit)
    if not 0 <= lo <= final_hi <= limit or final_hi - lo > R:
        raise ValueError(f"live_stitch_ref: rows [{lo}, {final_hi}) become final of {limit} frames in a ring of {R}")
    if B:
        scores = np.asarray(scores, np.float32)
        V, _, T, _ = scores.shape
        if scores.shape != (V, B, T, K1):
            raise ValueError(f"live_stitch_ref: scores {scores.shape} for {B} starts and {K1} columns")
    hi = min(limit, max(final_hi, starts[-1] + T if B else 0))
    for p in range(lo, hi):
        row = p % R
        for i in range(B):
            t = p - starts[i]
            if 0 <= t < T:
                for v in range(V):
                    x = scores[v, i, t]
                    ring_sum[row] += x
                    ring_sup[row] += 1 if (count_all or np.any(x != 0)) else 0
    n = final_hi - lo
    sums, support = np.zeros((n, K1), np.float32), np.zeros(n, np.int32)
    for p in range(lo, final_hi):
        row = p % R
        sums[p - lo], support[p - lo] = ring_sum[row], ring_sup[row]
        ring_sum[row] = 0
        ring_sup[row] = 0
    mean = sums / np.maximum(support, 1)[:, None].astype(np.float32)
    return sums, support, mean
