"""Host-side evaluation helpers around `TDEEDModel.predict`: stitching overlapping clip
predictions back into per-video score tracks, turning the tracks into spotted events, (soft) non-maximum suppression
and the tolerance-based mAP.  These are KB-sized numpy / python computations in the reference as well
(/root/reference/util/eval.py:34-261, 284-349; /root/reference/util/score.py:16-123); they stay on the CPU, restated here
with array operations where the reference loops in python, and are pinned against the reference's own functions by
`tests/golden/eval_utils.npz` (tools/make_goldens.py).

Event lists use the reference's records: {'video', 'events': [{'label', 'frame', 'score'}, ...], 'fps'}."""
from collections import defaultdict

import numpy as np

# util/eval.py:23-32
TOLERANCES = {"default": [1, 2, 4], "soccernet": [3, 6], "soccernetball": [6, 12]}
WINDOWS = {"default": [1, 3], "soccernet": [3, 6], "soccernetball": [6, 12], "tennis": [1, 3], "finegym": [1, 3]}


class ScoreStitcher:
    """Per-video accumulation of clip predictions (util/eval.py:284-349): scores (L, K+1) fp32 summed over the clips that
    cover a frame, support (L,) int32 counting them."""

    def __init__(self, videos, n_cols):
        """videos: iterable of (name, length, fps) like `dataset.videos`."""
        self.tracks = {v: (np.zeros((int(n), n_cols), np.float32), np.zeros(int(n), np.int32)) for v, n, _ in videos}
        self.fps = {v: f for v, _, f in videos}

    @staticmethod
    def _window(start, pred_len, video_len):
        """(offset into the clip, first video frame, number of frames) of a clip that may hang over either end."""
        off = -start if start < 0 else 0
        first = max(start, 0)
        n = min(pred_len - off, video_len - first)
        return off, first, max(n, 0)

    def add(self, video, start, pred_scores):
        """One clip of a dataloader batch: pred_scores (T, K+1).  A frame only counts as covered if the clip predicted
        something there (row sum != 0), util/eval.py:312-313."""
        scores, support = self.tracks[video]
        off, first, n = self._window(int(start), pred_scores.shape[0], scores.shape[0])
        p = pred_scores[off:off + n]
        scores[first:first + n] += p
        support[first:first + n] += (p.sum(axis=1) != 0).astype(np.int32)

    def add_views(self, video, start, pred_scores):
        """All views of one clip at once: pred_scores (V, T, K+1) (dataset-batched branch, util/eval.py:316-346)."""
        scores, support = self.tracks[video]
        off, first, n = self._window(int(start), pred_scores.shape[1], scores.shape[0])
        p = pred_scores[:, off:off + n]
        scores[first:first + n] += p.sum(axis=0)
        support[first:first + n] += p.shape[0]

    def normalised(self):
        """video -> mean score per frame (frames never covered divide by 1), util/eval.py:104-107."""
        out = {}
        for v in sorted(self.tracks):
            s, n = self.tracks[v]
            out[v] = s / np.maximum(n, 1)[:, None].astype(np.float32)
        return out


def stitch_predictions(model, loader, videos, n_cols, augment=False):
    """The prediction loop of `evaluate` (util/eval.py:284-349): run `model.predict` over the clips of `loader` and
    accumulate them per video.  Batches carry 'frame' (B,T,3,H,W), 'video' (names) and 'start' (first frame of each
    clip, may be negative).  augment=False: clips are scored one view each; augment=True: loader batch size 1 and every
    clip is scored twice, plain and horizontally flipped (`augment_inference=True`)."""
    st = ScoreStitcher(videos, n_cols)
    for clip in loader:
        starts = [int(s) for s in np.asarray(clip["start"]).reshape(-1)]
        if not augment:
            _, scores = model.predict(clip["frame"])
            for i in range(len(starts)):
                st.add(clip["video"][i], starts[i], scores[i])
        else:
            for flip in (False, True):
                _, scores = model.predict(clip["frame"], augment_inference=flip)
                st.add_views(clip["video"][0], starts[0], scores)
    return st


def video_clip_starts(num_frames, clip_len, overlap_len, stride=1, pad_len=5):
    """First frame of every evaluation clip of one video, in sampled-frame units and in dataset order: the loop of
    `ActionSpotVideoDataset.__init__` (dataset/frame.py:410-422) with the `start // stride` of its `__getitem__`
    (frame.py:451).  On the sampled frames (L = ceil(num_frames / stride) of them) this is the same list as
    video_clip_starts(L, clip_len, overlap_len, 1, pad_len): an integer is below num_frames / stride exactly when it is
    below its ceiling."""
    return [i // stride for i in range(-pad_len * stride, max(0, num_frames - overlap_len * stride),
                                       (clip_len - overlap_len) * stride)]


def stitch_clip_scores(scores, starts, L, flip_scores=None):
    """`stitch_clip_scores_seg` for one video of L frames (a group of one): scores (n,T,K+1) fp32, starts: n first frames
    (may be negative / hang over L).  Returns (sums (L,K+1) float32, support (L,) int32) -- equal, bit for bit, to what
    ScoreStitcher's clip-major loop leaves in its track."""
    return stitch_clip_scores_seg(scores, starts, [0, int(L)], [0, len(starts)], flip_scores)


def group_clip_table(lengths, clip_len, overlap_len, pad_len=5, clip_starts=None):
    """The tables of a group of videos scored as one packed job (`TDEEDModel.predict_video_group`): the videos' frames sit
    one after the other in one buffer, their clips one after the other in one list -- video-major, within a video in the
    order given; that order is what the gather, the batches and the stitch kernel walk.  lengths: frames per video;
    clip_starts: optional list (one entry per video) of each video's first frames, default `video_clip_starts` per video.
    Returns int32 arrays (seg_off (nv+1,): first packed frame of every video, the total last; clip_off (nv+1,): first clip
    of every video; starts (n,): video-local first frame of every clip; clip_base (n,) / clip_len_v (n,): seg_off and
    length of the clip's video).  Raises ValueError for a video without frames or without clips."""
    lengths = [int(x) for x in lengths]
    if clip_starts is not None and len(clip_starts) != len(lengths):
        raise ValueError(f"group_clip_table: clip starts for {len(clip_starts)} videos, {len(lengths)} lengths")
    seg_off, clip_off, starts, base, len_v = [0], [0], [], [], []
    for v, L in enumerate(lengths):
        if L <= 0:
            raise ValueError(f"group_clip_table: video {v} is empty")
        mine = video_clip_starts(L, clip_len, overlap_len, pad_len=pad_len) if clip_starts is None else \
            [int(x) for x in clip_starts[v]]
        if not mine:
            raise ValueError(f"group_clip_table: video {v} has no clips")
        starts += mine
        base += [seg_off[-1]] * len(mine)
        len_v += [L] * len(mine)
        seg_off.append(seg_off[-1] + L)
        clip_off.append(clip_off[-1] + len(mine))
    if seg_off[-1] >= 1 << 31:
        raise ValueError(f"group_clip_table: {seg_off[-1]} frames in one group do not fit int32")
    return tuple(np.asarray(a, np.int32) for a in (seg_off, clip_off, starts, base, len_v))


def frame_map_rows(L, clip_len, frame_batch):
    """Row arithmetic of the per-frame trunk maps of a video (or packed group) of L frames (`predict_video(reuse_frames=
    True)`): the frame pass runs chunks of frame_batch * clip_len consecutive frames, frames past the end black, and there is
    always at least one black row -- the map that a padded frame of a clip window copies.  -> (rows, pad_row, chunk):
    rows = ceil((L + 1) / chunk) * chunk, pad_row = L (the first black row), chunk = frame_batch * clip_len."""
    L, chunk = int(L), int(frame_batch) * int(clip_len)
    if L < 1 or chunk < 1:
        raise ValueError(f"frame_map_rows: {L} frames in chunks of {chunk}")
    return -(-(L + 1) // chunk) * chunk, L, chunk


def rows_gather_ref(maps, starts, L, pad_row, T, clip_base=None, clip_len_v=None):
    """numpy twin of ops.rows_gather / ops.rows_gather_seg: out[b, t] = maps[base[b] + starts[b] + t] when
    0 <= starts[b] + t < len[b] (one video: base 0, len L), maps[pad_row] otherwise."""
    if (clip_base is None) != (clip_len_v is None):
        raise ValueError("rows_gather_ref: clip_base and clip_len_v go together")
    maps = np.asarray(maps)
    B = len(starts)
    out = np.empty((B, T) + maps.shape[1:], maps.dtype)
    for b in range(B):
        base, lv = (0, int(L)) if clip_base is None else (int(clip_base[b]), int(clip_len_v[b]))
        for t in range(T):
            f = int(starts[b]) + t
            ok = 0 <= f < lv and base >= 0 and base + f < int(L)
            out[b, t] = maps[base + f if ok else pad_row]
    return out


def clip_gather_ring_ref(video, lo, ring_frames, starts, T, clip_base, clip_len_v, fill=0xA5):
    """numpy twin of ops.clip_gather_ring, with the ring it reads: `video` (L_total, ...) is the VIRTUAL packed buffer, of
    which the frames [lo, lo + ring_frames) (cut at L_total) are live: ring[p % ring_frames] = video[p] for those, every
    other row holds `fill`.  out[b, t] = ring[(clip_base[b] + starts[b] + t) % ring_frames] when 0 <= starts[b] + t <
    clip_len_v[b], zeros otherwise.  A real frame outside the live window is the caller's error (ValueError): the kernel
    would read whatever the row holds.  -> (out (B,T,...), ring (ring_frames,...))."""
    video = np.asarray(video)
    L, lo, rf = int(video.shape[0]), int(lo), int(ring_frames)
    if rf < 1 or not 0 <= lo < L:
        raise ValueError(f"clip_gather_ring_ref: a window from {lo} of {rf} rows over {L} frames")
    ring = np.full((rf,) + video.shape[1:], fill, video.dtype)
    for p in range(lo, min(lo + rf, L)):
        ring[p % rf] = video[p]
    B = len(starts)
    out = np.zeros((B, T) + video.shape[1:], video.dtype)
    for b in range(B):
        base, lv = int(clip_base[b]), int(clip_len_v[b])
        for t in range(T):
            f = int(starts[b]) + t
            if 0 <= f < lv and base >= 0 and base + f < L:
                p = base + f
                if not lo <= p < lo + rf:
                    raise ValueError(f"clip_gather_ring_ref: clip {b} reads frame {p}, live are [{lo}, {lo + rf})")
                out[b, t] = ring[p % rf]
    return out, ring


def ring_plan(lengths, frame_bytes, chunk_frames, max_resident_bytes, starts, clip_base, clip_len_v, clip_len, batch_size):
    """The plan of scoring a packed group whose frames exceed `max_resident_bytes` through a ring of frame chunks
    (`predict_video(stream_frames=True)`, `feeder.RingUpload`); pure host arithmetic.  Chunks are PackedUpload's: chunk c
    holds the packed frames [c * chunk_frames, (c + 1) * chunk_frames).  The ring has ring_chunks = max_resident_bytes //
    (chunk_frames * frame_bytes) slots of one chunk, chunk c lives in slot c % ring_chunks, so packed frame p sits in ring
    row p % ring_frames, ring_frames = ring_chunks * chunk_frames.  starts / clip_base / clip_len_v: `group_clip_table`'s;
    batches of `batch_size` are cut from the clip list in order.
    -> None when the frames fit the budget (the resident route serves them), else a namespace of ring_chunks, ring_frames
    and int arrays first / last (per batch: the chunks of the lowest / highest real packed frame the batch reads, -1 for a
    batch of nothing but padding) and last_reader (per chunk: the last batch that reads it, -1 for none).
    Raises ValueError when `first` decreases from one reading batch to the next (the ring moves forward only), and when
    the widest batch plus the one chunk the upload keeps ahead, max(last - first + 1) + 1 chunks, do not fit the ring.
    Together the two give what the upload relies on: when the host queues chunk c for a batch, every reader of the chunk
    it overwrites, c - ring_chunks, is an EARLIER batch (last_reader[c - ring_chunks] < that batch), and all frames one
    batch reads lie in distinct ring rows (clip_len <= ring_frames included)."""
    from types import SimpleNamespace
    lengths = [int(x) for x in lengths]
    L, fb, per, T, bs = sum(lengths), int(frame_bytes), int(chunk_frames), int(clip_len), int(batch_size)
    if min(fb, per, T, bs) < 1 or L < 1:
        raise ValueError(f"ring_plan: {L} frames of {fb} bytes in chunks of {per}, clips of {T} in batches of {bs}")
    if L * fb <= max_resident_bytes:
        return None
    ring_chunks = int(max_resident_bytes) // (per * fb)
    n = len(starts)
    n_chunks = -(-L // per)
    n_batches = -(-n // bs)
    first = np.full(n_batches, -1, np.int64)
    last = np.full(n_batches, -1, np.int64)
    last_reader = np.full(n_chunks, -1, np.int64)
    for i in range(n):
        s, base, lv = int(starts[i]), int(clip_base[i]), int(clip_len_v[i])
        a, z = base + max(s, 0), min(base + min(s + T, lv), L) - 1         # lowest / highest real packed frame of the clip
        if base < 0 or z < a:
            continue
        b, ca, cz = i // bs, a // per, z // per
        first[b] = ca if first[b] < 0 else min(first[b], ca)
        last[b] = max(last[b], cz)
        last_reader[ca:cz + 1] = b
    reading = np.nonzero(first >= 0)[0]
    for b0, b1 in zip(reading[:-1], reading[1:]):
        if first[b1] < first[b0]:
            raise ValueError(f"ring_plan: the streamed route needs clips in ascending order: batch {b1} reads from chunk "
                             f"{first[b1]} on, batch {b0} before it from chunk {first[b0]} on")
    need = (int((last - first).max()) + 1 if reading.size else 0) + 1
    if need > ring_chunks:
        raise ValueError(f"ring_plan: max_resident_bytes={max_resident_bytes} holds a ring of {ring_chunks} chunks of {per} "
                         f"frames, one batch and the chunk uploaded ahead of it need {need}: at least {need * per * fb} bytes")
    return SimpleNamespace(ring_chunks=ring_chunks, ring_frames=ring_chunks * per, first=first, last=last,
                           last_reader=last_reader)


def video_groups(lengths, frame_shapes, group_videos, max_resident_bytes, stream_frames=False):
    """Split consecutive videos, in the order given, into groups for `predict_video_group`: lists of indices.  A group closes
    when it holds `group_videos` videos, when the next video would push the frames of the group over `max_resident_bytes`,
    or when the frame geometry (3,H,W) changes.  A single video over the budget raises the ValueError predict_video
    raises for it; with stream_frames=True it becomes a group of its own instead (scored through the frame ring)."""
    if int(group_videos) < 1:
        raise ValueError("video_groups: group_videos must be positive")
    groups, cur, cur_bytes, cur_shape = [], [], 0, None
    for j, (L, shape) in enumerate(zip(lengths, frame_shapes)):
        shape = tuple(int(x) for x in shape)
        need = int(L) * int(np.prod(shape))
        if need > max_resident_bytes:
            if not stream_frames:
                raise ValueError(f"predict_video: the video needs {need} bytes on the device, more than max_resident_bytes="
                                 f"{max_resident_bytes} (stream_frames=True scores longer videos through a frame ring)")
            if cur:
                groups.append(cur)
            groups.append([j])
            cur, cur_bytes = [], 0
            continue
        if cur and (len(cur) >= int(group_videos) or cur_bytes + need > max_resident_bytes or shape != cur_shape):
            groups.append(cur)
            cur, cur_bytes = [], 0
        cur.append(j)
        cur_bytes += need
        cur_shape = shape
    if cur:
        groups.append(cur)
    return groups


def stitch_clip_scores_seg(scores, starts, seg_off, clip_off, flip_scores=None):
    """numpy twin of the stitch kernel (ops.stitch_scores_seg), and the statement of its order: per frame of video v, over
    that video's clips clip_off[v]:clip_off[v+1] of the group's clip list in the order given, the plain view's row and then
    the flipped view's row are added one after the other.  scores (n,T,K+1) fp32, starts: n video-local first frames (may be
    negative / hang over the video's end).  Without flip_scores support counts the added rows that are not all zero
    (`ScoreStitcher.add`); with flip_scores (n,T,K+1) it counts every added row (`ScoreStitcher.add_views`, once per view).
    Returns (sums (sum L,K+1) float32, support (sum L,) int32) over the packed frames."""
    scores = np.asarray(scores, np.float32)
    views = [scores] if flip_scores is None else [scores, np.asarray(flip_scores, np.float32)]
    _, T, K1 = scores.shape
    sums = np.zeros((int(seg_off[-1]), K1), np.float32)
    support = np.zeros(int(seg_off[-1]), np.int32)
    for v in range(len(seg_off) - 1):
        a, b = int(seg_off[v]), int(seg_off[v + 1])
        for f in range(b - a):
            for i in range(int(clip_off[v]), int(clip_off[v + 1])):
                t = f - int(starts[i])
                if 0 <= t < T:
                    for p in views:
                        sums[a + f] += p[i, t]
                        support[a + f] += 1 if (flip_scores is not None or np.any(p[i, t] != 0)) else 0
    return sums, support


def _with_loader(videos, decode):
    """A source that is a dict of `feeder.load_video` keyword arguments (frame_dir, dataset, video_name, num_frames, ...)
    becomes a callable: `feeder.load_video` for decode="host", `feeder.load_video_device` for decode="device".  Tensors
    and callables pass through."""
    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', not {decode!r}")
    import functools
    from . import feeder
    loader = feeder.load_video_device if decode == "device" else feeder.load_video
    return [(name, length, fps, functools.partial(loader, **src) if isinstance(src, dict) else src)
            for name, length, fps, src in videos]


def _decoded_groups(videos, group_videos, max_resident_bytes, decode_ahead=1, stream_frames=False):
    """The sources of `videos` (name, length, fps, frames | callable) in groups: batches of `group_videos` consecutive
    videos are materialised -- callables on a worker thread, up to `decode_ahead` batches ahead of the consumer -- and each
    batch is then split by `video_groups` (budget, geometry, stream_frames).  Yields lists of (name, length, fps, frames)."""
    from concurrent.futures import ThreadPoolExecutor
    import torch
    gv, ahead = int(group_videos), max(int(decode_ahead), 0)
    batches = [videos[lo:lo + gv] for lo in range(0, len(videos), gv)]

    def decode(batch):
        return [src() if callable(src) else src for _, _, _, src in batch]

    with ThreadPoolExecutor(max_workers=1, thread_name_prefix="tdeed-video") as ex:
        pending = {}
        for bi, batch in enumerate(batches):
            for k in range(bi, min(bi + ahead + 1, len(batches))):
                if k not in pending:
                    pending[k] = ex.submit(decode, batches[k])
            frames = pending.pop(bi).result()
            frames = [f if isinstance(f, torch.Tensor) else torch.as_tensor(np.asarray(f)) for f in frames]
            for (name, length, _, _), f in zip(batch, frames):
                if int(f.shape[0]) != int(length):
                    raise ValueError(f"video {name}: {int(f.shape[0])} frames delivered, {int(length)} announced")
            for idx in video_groups([b[1] for b in batch], [tuple(f.shape[1:]) for f in frames], gv, max_resident_bytes,
                                    stream_frames):
                yield [(batch[j][0], batch[j][1], batch[j][2], frames[j]) for j in idx]


def stitch_videos(model, videos, n_cols, augment=False, batch_size=8, overlap_len=None, decode_ahead=1, group_videos=1,
                  max_resident_bytes=16 << 30, reuse_frames=False, decode="host", stream_frames=False):
    """Whole-video counterpart of `stitch_predictions`: `videos` yields (name, length, fps, frames) with frames a uint8
    (length,3,H,W) tensor of the sampled frames or a callable returning one (e.g. a `feeder.load_video` closure); every
    video is scored once and its (sums, support) become the video's track of the returned ScoreStitcher, so
    `normalised()`, `frame_events`, both NMS functions and `mean_average_precisions` work on it unchanged.
    group_videos: up to that many consecutive videos (as far as `max_resident_bytes` and one frame geometry allow,
    `video_groups`) go through `model.predict_video_group` as one packed job whose batches are cut across the videos; 1
    (the default) scores video by video, each a group of one.  The callables of the next `decode_ahead` batches of
    `group_videos` videos are decoded on a worker thread meanwhile: decoding overlaps scoring.
    reuse_frames: passed on to `predict_video_group` (the per-frame trunk stages once per frame).
    stream_frames: a video over `max_resident_bytes` becomes a group of its own and is scored through a ring of frame chunks
    (`predict_video_group(stream_frames=True)`) instead of raising.
    decode: a `frames` entry may also be a dict of `feeder.load_video` keyword arguments; "host" loads it with
    `feeder.load_video`, "device" with `feeder.load_video_device` (JPEG decode on the device, same frames)."""
    videos = _with_loader(list(videos), decode)
    reuse = dict(reuse_frames=True) if reuse_frames else {}
    if stream_frames:
        reuse["stream_frames"] = True
    st = ScoreStitcher([(v, n, f) for v, n, f, _ in videos], n_cols)
    for group in _decoded_groups(videos, group_videos, max_resident_bytes, decode_ahead, stream_frames):
        out = model.predict_video_group([g[3] for g in group], overlap_len=overlap_len, batch_size=batch_size,
                                        augment=augment, max_resident_bytes=max_resident_bytes, **reuse)
        for (name, _, _, _), (sums, support) in zip(group, out):
            if sums.shape[1] != n_cols:
                raise ValueError(f"video {name}: the model scores {sums.shape[1]} columns, the stitcher holds {n_cols}")
            track, sup = st.tracks[name]
            track[...] = sums
            sup[...] = support
    return st


def frame_events(norm_scores, classes, fps, high_recall_score_threshold=0.01, labels=None):
    """`process_frame_predictions[_challenge]` (util/eval.py:86-192): per video the arg-max events and the high-recall
    events (every class whose score passes the threshold).  classes: name -> index (1-based, 0 = background).
    labels: optional video -> (L,) int ground truth; then the frame error rate and the foreground F1 counters
    (util/eval.py:34-84) are returned as well.
    Returns (pred_events, pred_events_high_recall, stats | None)."""
    inv = {v: k for k, v in classes.items()}
    cls_idx = np.array(sorted(inv), dtype=np.int64)
    events_all, recall_all = [], []
    n_err = n_tot = 0
    tp, fp, fn = defaultdict(int), defaultdict(int), defaultdict(int)
    for video in sorted(norm_scores):
        s = norm_scores[video]
        pred = s.argmax(axis=1)
        fg = np.nonzero(pred != 0)[0]
        events = [{"label": inv[int(pred[i])], "frame": int(i), "score": float(s[i, pred[i]])} for i in fg]
        ii, jj = np.nonzero(s[:, cls_idx] >= high_recall_score_threshold)       # row-major: frames, then classes ascending
        recall = [{"label": inv[int(cls_idx[j])], "frame": int(i), "score": float(s[i, cls_idx[j]])} for i, j in zip(ii, jj)]
        events_all.append({"video": video, "events": events, "fps": fps[video]})
        recall_all.append({"video": video, "events": recall, "fps": fps[video]})
        if labels is not None:
            true = np.asarray(labels[video])
            n_err += int((true != pred).sum())
            n_tot += true.shape[0]
            p_fg, t_fg = pred != 0, true != 0
            tp[None] += int((p_fg & t_fg).sum())
            fp[None] += int((p_fg & ~t_fg).sum())
            fn[None] += int((~p_fg & t_fg).sum())
            for k in inv:
                tp[k] += int(((pred == k) & (true == k)).sum())
                fp[k] += int(((pred == k) & (true != k)).sum())
                # a foreground frame of class k is missed when the prediction is anything else (background or another class)
                fn[k] += int(((true == k) & (pred != k)).sum())
    stats = None
    if labels is not None:
        def f1(k):
            den = tp[k] + 0.5 * fp[k] + 0.5 * fn[k]
            return tp[k] / (den if den != 0 else 1)
        stats = {"err": n_err / max(n_tot, 1), "f1": {k: f1(k) for k in [None] + sorted(inv)},
                 "tp_fp_fn": {k: (tp[k], fp[k], fn[k]) for k in [None] + sorted(inv)}}
    return events_all, recall_all, stats


def _by_label(events):
    groups = defaultdict(list)            # insertion order = first appearance, like the reference's defaultdict walk
    for e in events:
        groups[e["label"]].append(e)
    return groups


def _class_window(window, i):
    return window[i] if isinstance(window, list) else window


def non_maximum_suppression(pred, window, threshold=0.0):
    """util/eval.py:195-226: per video and label keep the best-scoring event, drop every other event of that label within
    +-window frames of it, repeat; stop at `threshold`.  (The first event found at the winner's frame is the one that
    is removed as "the winner", as in the reference.)"""
    out = []
    for vp in pred:
        kept = []
        for gi, evs in enumerate(_by_label(vp["events"]).values()):
            w = _class_window(window, gi)
            frames = np.array([e["frame"] for e in evs], dtype=np.int64)
            scores = np.array([e["score"] for e in evs], dtype=np.float64)
            alive = np.ones(len(evs), dtype=bool)
            while alive.any():
                cand = np.nonzero(alive)[0]
                best = cand[np.argmax(scores[cand])]                       # first maximum in list order, like max()
                if scores[best] < threshold:
                    break
                kept.append(dict(evs[best]))
                first_same = cand[np.nonzero(frames[cand] == frames[best])[0][0]]
                alive[first_same] = False
                alive &= ~((frames >= frames[best] - w) & (frames <= frames[best] + w))
        kept.sort(key=lambda e: e["frame"])
        nv = dict(vp)
        nv["events"] = kept
        nv["num_events"] = len(kept)
        out.append(nv)
    return out


def soft_non_maximum_suppression(pred, window, threshold=0.01):
    """util/eval.py:228-261: instead of dropping neighbours, scale their score by (distance / window)^2 (the winner's own
    frame gets 0), then remove only the winner."""
    out = []
    for vp in pred:
        kept = []
        for gi, evs in enumerate(_by_label(vp["events"]).values()):
            w = _class_window(window, gi)
            frames = np.array([e["frame"] for e in evs], dtype=np.int64)
            scores = np.array([e["score"] for e in evs], dtype=np.float64)
            alive = np.ones(len(evs), dtype=bool)
            while alive.any():
                cand = np.nonzero(alive)[0]
                best = cand[np.argmax(scores[cand])]
                if scores[best] < threshold:
                    break
                e = dict(evs[best])
                e["score"] = float(scores[best])
                kept.append(e)
                near = alive & (frames >= frames[best] - w) & (frames <= frames[best] + w)
                scores[near] = scores[near] * np.abs(frames[best] - frames[near]) ** 2 / (w ** 2)
                first_same = cand[np.nonzero(frames[cand] == frames[best])[0][0]]
                alive[first_same] = False
        kept.sort(key=lambda e: e["frame"])
        nv = dict(vp)
        nv["events"] = kept
        nv["num_events"] = len(kept)
        out.append(nv)
    return out


def label_order(first_frame, L):
    """Classes (>= 1) that have a high-recall candidate, in the order in which their labels first appear in the high-recall
    list (`_by_label`'s insertion order): by (first candidate frame, class).  first_frame: (K+1,), L where a class has none."""
    return sorted((c for c in range(1, len(first_frame)) if first_frame[c] < L), key=lambda c: (int(first_frame[c]), c))


def nms_rounds(mean, window, threshold, soft, hr_threshold=0.01):
    """numpy twin of the suppression kernel (ops.nms_track), and the statement of its order.  mean (L,K+1) fp32 (a
    normalised track); the candidates of class c >= 1 are the frames with mean[f,c] >= float32(hr_threshold), their score is
    float64(mean[f,c]) -- the high-recall list of `frame_events`.  The greedy loop of `non_maximum_suppression` /
    `soft_non_maximum_suppression` is replaced by rounds: in each round every live candidate with score >= threshold wins
    when no live candidate within +-R frames beats it in (score descending, frame ascending) order, and all winners of the
    round are kept at once.  Hard (R = w): a winner removes every candidate within +-w; scores never change.  Soft
    (R = 2w, so the winners of one round share no neighbour): a winner at p sets s[g] = s[g] * (p-g)^2 / w^2 for every live
    g within +-w, then only the winner is removed.  window: an int, or a list indexed by the label's appearance rank
    (`label_order`).  Returns (frames int32, classes int32, scores float64, rounds (K+1,) int32), events in the host's
    order: ascending frame, within a frame by appearance rank -- equal, bit for bit, to the two host functions applied to
    `frame_events(...)[1]`."""
    mean = np.asarray(mean, np.float32)
    L, K1 = mean.shape
    cand = mean >= np.float32(hr_threshold)
    cand[:, 0] = False
    first = np.where(cand.any(axis=0), cand.argmax(axis=0), L)
    rounds = np.zeros(K1, np.int32)
    kept = []                                                   # (frame, rank, class, score)
    for rank, c in enumerate(label_order(first, L)):
        w = int(_class_window(window, rank))
        if w < (1 if soft else 0):
            raise ValueError(f"nms_rounds: window {w}")
        reach = min(2 * w if soft else w, L - 1)
        alive = cand[:, c].copy()
        s = mean[:, c].astype(np.float64)
        for _ in range(int(alive.sum())):                       # every round keeps at least the best live candidate
            elig = alive & (s >= threshold)
            if not elig.any():
                break
            rounds[c] += 1
            win = elig.copy()
            for d in range(1, reach + 1):
                win[d:] &= ~(alive[:-d] & (s[:-d] >= s[d:]))    # an earlier frame wins ties
                win[:-d] &= ~(alive[d:] & (s[d:] > s[:-d]))
            for p in np.nonzero(win)[0]:
                kept.append((int(p), rank, c, float(s[p])))
            for p in np.nonzero(win)[0]:
                lo, hi = max(p - w, 0), min(p + w, L - 1)
                if soft:
                    g = np.arange(lo, hi + 1)
                    g = g[alive[g]]
                    s[g] = s[g] * np.abs(p - g) ** 2 / (w ** 2)
                    alive[p] = False
                else:
                    alive[lo:hi + 1] = False
    kept.sort(key=lambda e: (e[0], e[1]))
    return (np.array([e[0] for e in kept], np.int32), np.array([e[2] for e in kept], np.int32),
            np.array([e[3] for e in kept], np.float64), rounds)


def event_dicts(frames, classes_idx, scores, inv):
    """(frames, class indices, scores) arrays -> the reference's event dicts; inv: class index -> label."""
    return [{"label": inv[int(c)], "frame": int(f), "score": float(s)} for f, c, s in zip(frames, classes_idx, scores)]


def spot_videos(model, videos, classes, suppress, high_recall_score_threshold=0.01, augment=False, batch_size=8,
                overlap_len=None, decode_ahead=1, group_videos=1, max_resident_bytes=16 << 30, reuse_frames=False,
                decode="host", stream_frames=False):
    """Whole-video counterpart of `stitch_videos` + `frame_events` + the two NMS functions with the tail on the device:
    `videos` as in `stitch_videos`; every video is scored and spotted once.  suppress: entries (kind, window,
    threshold) with kind "nms" | "snms".  Returns (pred_events, [one list of video records per suppress entry],
    {video: pred (L,) int32}), videos in sorted order, records as `frame_events` / `non_maximum_suppression` /
    `soft_non_maximum_suppression` build them ('num_events' included), so `mean_average_precisions` works on them
    unchanged.  The label-dependent error / F1 counters of `frame_events` follow from the returned pred on the host.
    group_videos / decode_ahead: groups of videos go through `model.spot_video_group` as in `stitch_videos`.  reuse_frames:
    passed on to `spot_video_group`.  decode, stream_frames: as in `stitch_videos`."""
    videos = _with_loader(list(videos), decode)
    reuse = dict(reuse_frames=True) if reuse_frames else {}
    if stream_frames:
        reuse["stream_frames"] = True
    suppress = [tuple(e) for e in suppress]
    done = {}
    for group in _decoded_groups(videos, group_videos, max_resident_bytes, decode_ahead, stream_frames):
        out = model.spot_video_group([g[3] for g in group], classes, suppress=suppress,
                                     high_recall_score_threshold=high_recall_score_threshold, overlap_len=overlap_len,
                                     batch_size=batch_size, augment=augment, max_resident_bytes=max_resident_bytes, **reuse)
        for (name, _, fps, _), r in zip(group, out):
            done[name] = (fps, r)
    pred_events, lists, preds = [], [[] for _ in suppress], {}
    for name in sorted(done):
        fps, r = done[name]
        pred_events.append({"video": name, "events": r["events"], "fps": fps})
        for i, evs in enumerate(r["suppressed"]):
            lists[i].append({"video": name, "events": evs, "fps": fps, "num_events": len(evs)})
        preds[name] = r["pred"]
    return pred_events, lists, preds


def average_precision(pred, truth, tolerance=0):
    """util/score.py:45-96.  pred: [(video, frame, score)] sorted by descending score; truth: video -> [frames].
    Greedy matching: every prediction takes the closest not-yet-recalled ground-truth frame of its video (first one wins
    ties); precision is recorded at every new recall, interpolated (running max from the right) and averaged over the
    number of ground-truth events."""
    total = sum(len(v) for v in truth.values())
    open_gt = {v: list(f) for v, f in truth.items()}
    pc = []
    recalled = 0
    for i, (video, frame, _) in enumerate(pred, 1):
        gts = open_gt.get(video)
        if not gts:
            continue
        d = np.abs(np.asarray(gts) - frame)
        j = int(np.argmin(d))                                   # first closest, like the strict '>' of the reference
        if d[j] <= tolerance:
            hit = gts[j]
            gts[:] = [f for f in gts if f != hit]               # the reference keys recalled events by (video, frame)
            recalled += 1
            pc.append(recalled / i)
    if not pc:
        return 0.0
    interp = np.maximum.accumulate(np.asarray(pc)[::-1])
    return float(interp.sum() / total)


def mean_average_precisions(truth, pred, tolerances=(0, 1, 2, 4)):
    """`compute_mAPs` (util/score.py:99-160) without the printing / plotting: returns (mAP per tolerance, {label: [AP per
    tolerance]}).  truth / pred: lists of the event records described in the module docstring."""
    assert {v["video"] for v in truth} == {v["video"] for v in pred}, "Video set mismatch!"
    by_label = defaultdict(lambda: defaultdict(list))
    for x in truth:
        for e in x["events"]:
            by_label[e["label"]][x["video"]].append(e["frame"])
    flat = defaultdict(list)
    for x in pred:
        for e in x["events"]:
            flat[e["label"]].append((x["video"], e["frame"], e["score"]))
    for lab in flat:
        flat[lab].sort(key=lambda r: r[-1], reverse=True)       # stable, like list.sort in get_predictions
    aps = {lab: [average_precision(flat.get(lab, []), by_label[lab], tol) for tol in tolerances] for lab in sorted(by_label)}
    maps = [float(np.mean([aps[lab][i] for lab in aps])) for i in range(len(tolerances))]
    return maps, aps


# ----------------------------------------------------------------------------- average precision by counting
# `average_precision` walks one globally sorted list, but (1) whether a prediction recalls a ground-truth frame depends only
# on the earlier predictions of its own video, and (2) only the hits need a global position.  The three functions below state
# that decomposition; they are the oracle of the device route (csrc/ap.hip), as `nms_rounds` is of the suppression kernel.
def ap_match_video(frames, scores, gt, tolerance):
    """The greedy matching of `average_precision` for ONE label in ONE video.  frames / scores: the video's predictions of the
    label, frames unique; gt: its ground-truth frames in the truth record's list order, duplicates kept.
    -> (order, hits): order sorts the predictions by (score descending, frame ascending) -- the global order restricted to the
    video; hits are the positions in that order that recall a ground-truth frame: the closest open one within `tolerance`, the
    first in list order on equal distance; a hit closes every entry with that frame.  Stops when nothing is open."""
    frames, scores = np.asarray(frames, np.int64), np.asarray(scores, np.float64)
    order = np.lexsort((frames, -scores))
    open_gt, hits = [int(f) for f in gt], []
    for i, e in enumerate(order):
        if not open_gt:
            break
        d = np.abs(np.asarray(open_gt, np.int64) - frames[e])
        j = int(np.argmin(d))
        if d[j] <= tolerance:
            hit = open_gt[j]
            open_gt = [f for f in open_gt if f != hit]
            hits.append(i)
    return order, hits


def ap_hit_ranks(sorted_scores, hits):
    """sorted_scores: per video, in ordinal order, the label's scores in `ap_match_video`'s order; hits: per video the hit
    positions.  -> per video the hits' 1-based ranks among ALL predictions of the label in the order (score descending, video
    ordinal ascending, frame ascending) -- Python's stable sort(reverse=True) of the list `mean_average_precisions` builds --
    by counting: an earlier video precedes on equal score, a later one only with a greater score."""
    neg = [-np.asarray(s, np.float64) for s in sorted_scores]
    out = []
    for v, hv in enumerate(hits):
        ranks = []
        for pos in hv:
            s = neg[v][pos]
            before = int(pos)
            for u, a in enumerate(neg):
                if u != v:
                    before += int(np.searchsorted(a, s, side="right" if u < v else "left"))
            ranks.append(before + 1)
        out.append(ranks)
    return out


def ap_from_ranks(ranks, total):
    """ranks: the hits' global ranks, any order; total: the label's ground-truth count (duplicates included).  The k-th hit by
    rank has precision k / rank; running maximum from the right, sum, / total."""
    if len(ranks) == 0:
        return 0.0
    r = np.sort(np.asarray(ranks, np.int64))
    pc = np.arange(1, len(r) + 1) / r
    return float(np.maximum.accumulate(pc[::-1]).sum() / total)


def ap_restated(events, truth, tolerance):
    """One label over a dataset: events / truth per video in ordinal order, (frames, scores) and [ground-truth frames].
    -> dict(ap, hits: per video the hit positions, ranks: per video, frames / scores: per video in matching order, total)."""
    total = sum(len(g) for g in truth)
    frames, scores, hits = [], [], []
    for (f, s), g in zip(events, truth):
        f, s = np.asarray(f, np.int64), np.asarray(s, np.float64)
        order, hv = ap_match_video(f, s, g, tolerance)
        frames.append(f[order])
        scores.append(s[order])
        hits.append(hv)
    ranks = ap_hit_ranks(scores, hits)
    return dict(ap=ap_from_ranks([r for rv in ranks for r in rv], total), hits=hits, ranks=ranks, frames=frames, scores=scores,
                total=total)


def mean_average_precisions_by_counting(truth, pred, tolerances=(0, 1, 2, 4)):
    """`mean_average_precisions` through the decomposition above (the video ordinal is the record's position in `pred`) ->
    (mAP per tolerance, {label: [AP per tolerance]}, {(label, tolerance): ap_restated's dict})."""
    assert {v["video"] for v in truth} == {v["video"] for v in pred}, "Video set mismatch!"
    names = [x["video"] for x in pred]
    ordinal = {v: i for i, v in enumerate(names)}
    gt = defaultdict(lambda: [[] for _ in names])
    for x in truth:
        for e in x["events"]:
            gt[e["label"]][ordinal[x["video"]]].append(e["frame"])
    ev = defaultdict(lambda: [([], []) for _ in names])
    for x in pred:
        for e in x["events"]:
            f, s = ev[e["label"]][ordinal[x["video"]]]
            f.append(e["frame"])
            s.append(e["score"])
    detail = {(lab, tol): ap_restated(ev[lab], gt[lab], tol) for lab in sorted(gt) for tol in tolerances}
    aps = {lab: [detail[lab, tol]["ap"] for tol in tolerances] for lab in sorted(gt)}
    maps = [float(np.mean([aps[lab][i] for lab in aps])) for i in range(len(tolerances))]
    return maps, aps, detail


def truth_table(truth, ordinal, classes):
    """The truth records as the table `ops.ap_state` uploads: {(video ordinal, class index): [frames in list order]}."""
    table = defaultdict(list)
    for x in truth:
        for e in x["events"]:
            if e["label"] not in classes:
                raise ValueError(f"truth label {e['label']!r} is not one of the model's classes")
            table[ordinal[x["video"]], classes[e["label"]]].append(e["frame"])
    return dict(table)


def map_suppress_entries(suppress, who):
    """the suppress entries of a mAP pass as tuples: ("raw",) or (kind, window, threshold) with kind "nms" | "snms", at least one"""
    suppress = [tuple(e) for e in suppress]
    for e in suppress:
        if not e or e[0] not in ("raw", "nms", "snms") or len(e) != (1 if e[0] == "raw" else 3):
            raise ValueError(f"{who}: suppress entry {e!r}: ('raw',) or (kind, window, threshold) with kind nms | snms")
    if not suppress:
        raise ValueError(f"{who}: no suppress entry")
    return suppress


# ----------------------------------------------------------------------------- the mAP pass sharded over ranks
def shard_videos(lengths, world):
    """Who scores what in a validation pass sharded over `world` ranks: lengths in ordinal order -> `world` lists of ordinals
    (ascending), every ordinal in exactly one.  Longest video first (equal lengths: the lower ordinal) to the least-loaded
    rank, load counted in frames (equal loads: the lower rank) -- pure arithmetic on the lengths, so every rank computes the
    same table without communicating.  The loads then differ by at most the longest video.  A rank's list is empty when
    there are fewer videos than ranks."""
    world = int(world)
    lengths = [int(x) for x in lengths]
    if world < 1 or any(x < 0 for x in lengths):
        raise ValueError(f"shard_videos: world {world} and lengths >= 0")
    load, out = [0] * world, [[] for _ in range(world)]
    for o in sorted(range(len(lengths)), key=lambda o: (-lengths[o], o)):
        r = min(range(world), key=lambda r: (load[r], r))
        out[r].append(o)
        load[r] += lengths[o]
    return [sorted(x) for x in out]


def parse_shard(shard, who="map_videos"):
    """shard: None -> None; "auto" -> (rank, world) of the initialised default process group ((0, 1) without one); (rank,
    world) -> itself as ints.  ValueError for anything else."""
    if shard is None:
        return None
    if isinstance(shard, str):
        if shard != "auto":
            raise ValueError(f"{who}: shard must be None, 'auto' or (rank, world), not {shard!r}")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
        return 0, 1
    try:
        rank, world = shard
        ok = int(rank) == rank and int(world) == world and 0 <= int(rank) < int(world)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: shard must be None, 'auto' or (rank, world) with 0 <= rank < world, not {shard!r}")
    return int(rank), int(world)


def _ap_segments(ev_count, hit_count, vid_off, gt_off, K1):
    """the segments of the exchange in payload order: two lists of (ordinal, index of the segment's first element in its
    flattened store row, row, count) -- scores (e, c, ord), hits (e, t, ord*K1+c)"""
    ev_count, hit_count = np.asarray(ev_count), np.asarray(hit_count)
    E, C, NV = ev_count.shape
    T = hit_count.shape[1]
    sc = [(o, int(vid_off[o]), e * C + c, int(ev_count[e, c, o])) for e in range(E) for c in range(C) for o in range(NV)]
    hc = [(oc // K1, int(gt_off[oc]), e * T + t, int(hit_count[e, t, oc])) for e in range(E) for t in range(T) for oc in range(NV * K1)]
    return sc, hc


def ap_pack_ref(ev_score, ev_count, hit_pos, hit_count, vid_off, gt_off, K1, own_ords):
    """numpy restatement of ops.ap_state_pack: the stores of one rank (ev_score (E,K1-1,LT) float64, hit_pos (E,T,G) int32)
    with the counts already summed over the ranks -> (scores float64 (S,), hits int32 (Hh,)): the used part of every segment
    of own_ords at the exclusive scan of the counts, zeros elsewhere."""
    own = set(int(o) for o in own_ords)
    sc, hc = _ap_segments(ev_count, hit_count, vid_off, gt_off, K1)
    ev_score, hit_pos = np.asarray(ev_score), np.asarray(hit_pos)
    out = []
    for segs, store, dt in ((sc, ev_score.reshape(-1, ev_score.shape[-1]), np.float64), (hc, hit_pos.reshape(-1, hit_pos.shape[-1]), np.int32)):
        pay = np.zeros(sum(s[3] for s in segs), dt)
        at = 0
        for o, first, row, n in segs:
            if o in own:
                pay[at:at + n] = store[row, first:first + n]
            at += n
        out.append(pay)
    return out[0], out[1]


def ap_unpack_ref(ev_score, ev_count, hit_pos, hit_count, vid_off, gt_off, K1, own_ords, scores, hits):
    """numpy restatement of ops.ap_state_unpack: writes the segments of the videos NOT in own_ords from the summed payloads
    into ev_score / hit_pos, in place; own segments are not written."""
    own = set(int(o) for o in own_ords)
    sc, hc = _ap_segments(ev_count, hit_count, vid_off, gt_off, K1)
    for segs, store, pay in ((sc, ev_score.reshape(-1, ev_score.shape[-1]), scores), (hc, hit_pos.reshape(-1, hit_pos.shape[-1]), hits)):
        at = 0
        for o, first, row, n in segs:
            if o not in own:
                store[row, first:first + n] = pay[at:at + n]
            at += n


def frame_stats_ref(mean, labels, K1=None):
    """numpy restatement of ops.frame_stats_seg on one track: int64 (2 + 3*K1,) -- frames, errors, then (tp, fp, fn) for "any"
    and every class, by the counting rule of `frame_events(labels=...)`."""
    mean, true = np.asarray(mean), np.asarray(labels).astype(np.int64)
    K1 = mean.shape[1] if K1 is None else int(K1)
    pred = mean.argmax(axis=1)
    out = np.zeros(2 + 3 * K1, np.int64)
    out[0], out[1] = true.shape[0], int((true != pred).sum())
    p_fg, t_fg = pred != 0, true != 0
    out[2:5] = int((p_fg & t_fg).sum()), int((p_fg & ~t_fg).sum()), int((~p_fg & t_fg).sum())
    for k in range(1, K1):
        out[2 + 3 * k:5 + 3 * k] = (int(((pred == k) & (true == k)).sum()), int(((pred == k) & (true != k)).sum()),
                                    int(((true == k) & (pred != k)).sum()))
    return out


def frame_stats_dict(counters, classes):
    """The counter tensor of ops.frame_stats_seg (int64 (2 + 3*K1,), on the host) -> the stats dict `frame_events` returns as
    its third value: "err", "f1", "tp_fp_fn", keyed None ("any") and the class indices of `classes` (name -> index)."""
    c = [int(x) for x in np.asarray(counters).reshape(-1)]
    keys = [None] + sorted(classes.values())
    if len(c) < 2 + 3 * (max(keys[1:], default=0) + 1):
        raise ValueError(f"frame_stats_dict: {len(c)} counters for the classes {keys[1:]}")
    trip = {k: tuple(c[2 + 3 * (k or 0):5 + 3 * (k or 0)]) for k in keys}

    def f1(k):
        tp, fp, fn = trip[k]
        den = tp + 0.5 * fp + 0.5 * fn
        return tp / (den if den != 0 else 1)
    return {"err": c[1] / max(c[0], 1), "f1": {k: f1(k) for k in keys}, "tp_fp_fn": trip}


def check_labels(labels, lengths, K1, who):
    """labels: per video an (L,) integer array -> the uint8 arrays; ValueError when a length differs from the video's or a
    value lies outside 0..K1-1"""
    out = []
    for i, (lab, L) in enumerate(zip(labels, lengths)):
        a = np.asarray(lab)
        if a.ndim != 1 or a.shape[0] != int(L) or a.dtype.kind not in "iu":
            raise ValueError(f"{who}: the labels of video {i} must be {int(L)} integers, got {a.dtype} {a.shape}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > K1 - 1):
            raise ValueError(f"{who}: the labels of video {i} must lie in 0..{K1 - 1}")
        out.append(a.astype(np.uint8))
    return out


def merge_ap_state(state, own_ords, group=None, frame_stats=None):
    """Makes the ops.ApState of every rank of a sharded pass the state of a one-rank pass, as far as ops.ap_rank reads it:
    the three phases of ops.ap_state_counts / ap_state_pack / ap_state_unpack with torch.distributed sums in between
    (tdeed_amd.dist.init sets the default group up; device tensors go to all_reduce as they are, like GradReducer's torch
    backend: gloo in tests, RCCL in production).  own_ords: the ordinals this rank matched.  frame_stats: the counter
    tensor of ops.frame_stats_seg, summed with the count tables.  Every rank must call it.  Without an initialised process
    group, or with one rank, nothing happens.  -> dict(exchange_bytes: bytes of all tensors handed to collectives,
    host_syncs: 1 for the payload sizes, 0 when nothing happened)."""
    import torch.distributed as dist
    from . import ops
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return dict(exchange_bytes=0, host_syncs=0)
    nbytes = 0

    def total(x):
        nonlocal nbytes
        if x.numel():
            dist.all_reduce(x, op=dist.ReduceOp.SUM, group=group)
            nbytes += x.numel() * x.element_size()
    counts = ops.ap_state_counts(state, own_ords)
    for x in counts + ([frame_stats] if frame_stats is not None else []):
        total(x)
    scores, hits = ops.ap_state_pack(state, own_ords, owners=counts[2])
    total(scores)
    total(hits)
    ops.ap_state_unpack(state, own_ords, scores, hits)
    return dict(exchange_bytes=nbytes, host_syncs=1)


def map_videos(model, videos, classes, truth, suppress, tolerances=(0, 1, 2, 4), high_recall_score_threshold=0.01, augment=False,
               batch_size=8, overlap_len=None, decode_ahead=1, group_videos=1, max_resident_bytes=16 << 30, reuse_frames=False,
               decode="host", stream_frames=False, labels=None, shard=None):
    """`spot_videos` + `mean_average_precisions` per suppress entry with the whole tail on the device: no event list reaches the
    host.  videos and the keyword arguments as in `spot_videos`; truth: the records `mean_average_precisions` takes; suppress:
    entries ("raw",) -- the unsuppressed high-recall list -- or (kind, window, threshold) with kind "nms" | "snms".
    Returns per suppress entry (mAP per tolerance, {label: [AP per tolerance]}), `mean_average_precisions`' result: the APs
    come from the device (csrc/ap.hip), the mean over the truth's labels is taken here, in sorted label order.  The video
    ordinal -- the index of a video's name in sorted order -- decides ties between videos, whatever order the groups arrive
    in.  The host synchronises once per group and once for the (entries, tolerances, K+1) table; model.last_video_stats:
    the groups' totals plus groups, host_syncs, ap_d2h_bytes, videos_own (videos this rank scored) and exchange_bytes (bytes
    handed to collectives; 0 without an exchange).
    labels: {video: (L,) ints}, the ground-truth class of every frame.  Then the frame error / foreground-F1 counters are
    taken on the device as well (one more launch per group, ops.frame_stats_seg; they come back with the AP table) and the
    function returns (results, stats), stats being the dict `frame_events(labels=...)` returns as its third value.
    shard: None -- this process scores every video, no collective; "auto" -- rank and world of the initialised default
    process group; (rank, world).  The call still takes the list of ALL videos: names and lengths define the ordinals and the
    state.  `shard_videos` decides who scores what; the source of a video that belongs to another rank may be None and is
    never touched.  Groups are cut from the rank's own videos, after the last group the states are exchanged
    (`merge_ap_state`), and the rank + AP launch runs on every rank: every rank returns the same result, bit for bit the
    one-rank pass.  host_syncs <= own groups + 2."""
    from . import ops
    videos = list(videos)
    suppress = map_suppress_entries(suppress, "map_videos")
    tols = ops.ap_tolerances(tolerances, "map_videos")
    names = sorted(v[0] for v in videos)
    assert {x["video"] for x in truth} == set(names), "Video set mismatch!"
    if len(set(names)) != len(names):
        raise ValueError("map_videos: video names must be unique")
    ordinal = {v: i for i, v in enumerate(names)}
    length = {v[0]: int(v[1]) for v in videos}
    K1 = len(classes) + 1
    table = truth_table(truth, ordinal, classes)
    shard = parse_shard(shard)
    own_ords = None
    if shard is not None:
        own_ords = shard_videos([length[v] for v in names], shard[1])[shard[0]]
        own = set(own_ords)
        videos = [v for v in videos if ordinal[v[0]] in own]
        if shard[1] > 1:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() != shard[1]:
                raise ValueError(f"map_videos: shard {shard} needs an initialised process group of {shard[1]} ranks")
    missing = [v[0] for v in videos if v[3] is None]
    if missing:
        raise ValueError(f"map_videos: the videos {missing} are this rank's own and have no frame source")
    if labels is not None:
        if K1 > 256:
            raise ValueError(f"map_videos: {K1} score columns do not fit one-byte labels")
        absent = [v[0] for v in videos if v[0] not in labels]
        if absent:
            raise ValueError(f"map_videos: no labels for the videos {absent}")
        check_labels([labels[v[0]] for v in videos], [v[1] for v in videos], K1, "map_videos")
    videos = _with_loader(videos, decode)
    reuse = dict(reuse_frames=True) if reuse_frames else {}
    if stream_frames:
        reuse["stream_frames"] = True
    state = ops.ap_state([length[v] for v in names], table, K1, len(suppress), tols, device=model.device)
    counters = None
    if labels is not None:
        import torch
        counters = torch.zeros((ops.frame_stats_size(K1),), dtype=torch.int64, device=state.device)
    totals, groups = defaultdict(int), 0
    for group in _decoded_groups(videos, group_videos, max_resident_bytes, decode_ahead, stream_frames) if videos else ():
        with_labels = {} if labels is None else dict(labels=[labels[g[0]] for g in group], frame_stats=counters)
        model.map_video_group([g[3] for g in group], classes, state, [ordinal[g[0]] for g in group], suppress=suppress,
                              high_recall_score_threshold=high_recall_score_threshold, overlap_len=overlap_len,
                              batch_size=batch_size, augment=augment, max_resident_bytes=max_resident_bytes, **reuse, **with_labels)
        groups += 1
        for k, v in model.last_video_stats.items():
            if k in ("ring_frames", "ring_chunks", "resident_bytes"):       # (of the groups that streamed: the largest ring)
                totals[k] = max(totals[k], v)
            elif k != "views":
                totals[k] += v
    merged = dict(exchange_bytes=0, host_syncs=0) if shard is None else merge_ap_state(state, own_ords, frame_stats=counters)
    if counters is None:
        ap, _ = model.map_finish(state)
    else:
        ap, _, counters = model.map_finish(state, frame_stats=counters)
    for k, v in model.last_video_stats.items():
        totals[k] += v
    totals["groups"] = groups
    totals["host_syncs"] += merged["host_syncs"]
    totals["exchange_bytes"] = merged["exchange_bytes"]
    totals["videos_own"] = len(videos)
    model.last_video_stats = dict(totals)
    inv = {v: k for k, v in classes.items()}
    labelled = sorted(inv[c] for c in range(1, K1) if state.totals[c] > 0)
    out = []
    for i in range(len(suppress)):
        aps = {lab: [float(ap[i, t, classes[lab]]) for t in range(len(tols))] for lab in labelled}
        out.append(([float(np.mean([aps[lab][t] for lab in aps])) for t in range(len(tols))], aps))
    if labels is not None:
        return out, frame_stats_dict(counters, classes)
    return out


# ----------------------------------------------------------------------------- validation videos from resident JPEG streams
def _crop_window(crop, H, W):
    """crop: None, an int side or (wh, ww) -> the centre window (top, left, wh, ww) by engine.centre_window -- the rectangle
    `engine.trunk_geometry` gives the first launch -- or None when the window is the whole frame"""
    from .engine import centre_window
    if crop is None:
        return None
    wh, ww = (int(crop), int(crop)) if np.ndim(crop) == 0 else (int(crop[0]), int(crop[1]))
    if wh < 1 or ww < 1:
        raise ValueError(f"ResidentJpegVideos: crop {crop!r} must be positive")
    if wh > H or ww > W:
        raise ValueError(f"ResidentJpegVideos: the crop {wh}x{ww} is larger than the {H}x{W} frames")
    if (wh, ww) == (H, W):
        return None
    return centre_window(H, W, wh, ww)


class ResidentJpegVideos:
    """The videos of a validation split resident on the device COMPRESSED, each decoded there when it is scored: what
    `trainclips.ResidentJpegClips` is to training.  videos: the label list's dicts (video, num_frames, optionally fps);
    jpegs: their `jpegsets.load_resident_jpegs(..., stride=s)` pack, video i of which has ceil(num_frames / s) frames.
    Construction is `ResidentJpegClips`' (`residentstreams.ResidentStreams`): the shards' streams in one buffer, the tables in
    one copy, the index pass once per shard, one host synchronisation, fallback and flagged frames decoded once with
    `feeder.read_frame` into a side buffer; resident bytes over max_resident_bytes raise ValueError before anything is
    uploaded.  split_mcus: MCUs per piece (default one MCU row); max_coeff_bytes: the coefficient buffer, a video beyond
    it decodes in chunks of frames.

    crop: None, an int side or (wh, ww): `frames` returns the centre window only (`engine.centre_window`, the rectangle the
    first launch of a crop_dim model reads).  Then the pixel pass is ops.jpeg_pixels_window, the items leave out the pieces
    whose MCU rows the window does not read (`jpegsets.video_tables`), and the side buffer is kept cropped.

    `frames(i)` is video i as a device uint8 (L_i, 3, h, w) tensor, the bits of `feeder.load_video`'s frames (cut to the
    window); `sources()` is the `videos` argument of `stitch_videos`, `spot_videos`, `map_videos`: (name, length, fps,
    callable) with fps from the video dicts.  `stats`: `ResidentJpegClips.stats`' fields plus frame_shape and
    decoded_bytes_per_frame (of what `frames` returns).  `resident_bytes` and the budget count what construction leaves on the
    device, as `ResidentJpegClips` counts it.  Not counted: the coefficient buffer (max_coeff_bytes bounds it) and the item
    tables of the videos decoded so far, which are kept on the host and on the device for the next pass: 8 bytes per piece
    plus 8 per frame, about 120 bytes per 224-row 4:2:0 frame against some 20 000 of stream.
    stream_videos=True: a set whose resident bytes exceed max_resident_bytes is accepted, as `ResidentJpegClips(
    stream_clips=True)` accepts one: the tables and the streams of the first videos that fit stay resident, the other videos'
    streams stay in the host shards of `jpegs`, and `frames(i)` of such a video copies its byte ranges into one staging
    region on the object's stream before the relocating items entry decodes them -- chunk by chunk of the coefficient buffer,
    whose frames are what the region holds, so a video longer than a chunk is staged in several copies.  A resident video
    takes the path above untouched; the frames are the all-resident object's bit for bit.  The budget counts the region;
    too small a budget raises ValueError naming the smallest that would do, a shard larger than the region one naming
    `shard_bytes`.  `stats` gains resident_videos, streamed_videos, stage_bytes, host_stream_bytes.
    Not offered: the frame ring (`stream_frames=True`) fed by this decode, and `reuse_frames` beyond what the consumers do
    with any device tensor."""

    UPLOAD_CHUNK_BYTES = 64 << 20        # the streams are uploaded in copies of this size (`ResidentJpegClips`' default)

    def __init__(self, videos, jpegs, crop=None, split_mcus=None, max_resident_bytes=16 << 30, max_coeff_bytes=512 << 20,
                 device="cuda", stream_videos=False):
        import threading
        import torch
        from . import jpegdev, streams
        from .residentstreams import ResidentStreams
        videos = list(videos)
        stride = int(getattr(jpegs, "stride", 1))
        if not videos or len(videos) != len(jpegs.video_len):
            raise ValueError(f"ResidentJpegVideos: {len(videos)} videos, {len(jpegs.video_len)} in the packed set")
        for v, n in zip(videos, jpegs.video_len):
            if -(-int(v["num_frames"]) // stride) != int(n):
                raise ValueError(f"ResidentJpegVideos: video {v['video']} has {int(v['num_frames'])} frames at stride {stride}, "
                                 f"the packed set {int(n)}")
        if int(max(jpegs.video_len)) > 65535:
            raise ValueError(f"ResidentJpegVideos: a video of {int(max(jpegs.video_len))} frames exceeds the kernels' 65535 rows")
        if int(max_coeff_bytes) < 1:
            raise ValueError("ResidentJpegVideos: max_coeff_bytes must be positive")
        if jpegs.width:
            self.window = _crop_window(crop, jpegs.height, jpegs.width)      # argument errors before any file is touched
            rs = ResidentStreams("ResidentJpegVideos", jpegs, split_mcus, max_resident_bytes, self.window, streamed=stream_videos)
        else:                                                   # the geometry comes from Pillow's decode of the first frame
            rs = ResidentStreams("ResidentJpegVideos", jpegs, split_mcus, 1 << 62, None, streamed=stream_videos)
            self.window = _crop_window(crop, rs.H, rs.W)
            rs.max_resident_bytes = max_resident_bytes
            rs.set_window(self.window)                          # the budget, with side frames of the window's size
        self._rs, self.samp, self.split_mcus = rs, rs.samp, rs.split
        self.H, self.W = rs.H, rs.W
        self.shape = rs.side_shape
        self.names = [v["video"] for v in videos]
        self.fps = [v.get("fps") for v in videos]
        self.video_first = [int(x) for x in jpegs.video_first]
        self.video_len = [int(x) for x in jpegs.video_len]
        self._mcu_rows = jpegdev.window_blocks(rs.geom, *self.window).mcu_rows if self.window is not None else None
        self._plan = None
        longest = max(self.video_len)                           # at most 65535, checked above
        if stream_videos:
            # a streamed video is staged in the frame chunks of the coefficient buffer: the plan's "clips" are those chunks
            chunk = rs.chunk_frames(longest, max_coeff_bytes)
            rows = np.asarray([(f, lo, n, v) for v, (f, n) in enumerate(zip(self.video_first, self.video_len))
                               for lo in range(0, n, chunk)], np.int64).T
            self._plan = rs.plan_streaming(rows, chunk, 1, 1, 1, 1)
        self.device = dev = torch.device(device)
        self.stream = streams.new_stream(device)
        self.stream.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(self.stream):
            rs.upload(self.stream, dev, self.UPLOAD_CHUNK_BYTES)
            rs.decode_buffers(dev, longest, max_coeff_bytes)
            self._chunk = rs.chunk
        self.stream.synchronize()
        self._lock = threading.Lock()
        self._tabs = {}                                          # video -> (host tables, their device copies)
        # internal, for tools/bench_video.py only: set to a list and `frames` appends (start, between, end) timing events
        # around the entropy and the pixel launch of every chunk; None (the default) records nothing
        self._kernel_events = None
        self.stats = dict(rs.stats(), frame_shape=tuple(self.shape), decoded_bytes_per_frame=int(np.prod(self.shape)))

    def __len__(self):
        return len(self.names)

    def video_tables(self, i):
        """`jpegsets.video_tables` of video i: what `frames(i)` launches with (host arrays)"""
        from .jpegsets import video_tables
        rs = self._rs
        return video_tables(self.video_first[i], self.video_len[i], rs.frame_set, rs.side_row, rs.piece_lo, rs.piece_n,
                            chunk_slots=self._chunk, piece_mcu=rs.piece_mcu, mcus_x=rs.geom.mcus_x, mcu_rows=self._mcu_rows)

    def frames(self, i, out=None):
        """Video i decoded on the object's own stream: device uint8 (L_i, 3, h, w), into `out` when given.  Per coefficient
        chunk: zero it, ops.jpeg_entropy_items, the pixel pass (ops.jpeg_pixels_rows, or ops.jpeg_pixels_window with crop);
        then ops.jpeg_slot_fill for the side frames.  Waits for the stream and reads the device error word: non-zero raises
        RuntimeError naming the video.  No file is read.  Calls from several threads take turns (one coefficient buffer)."""
        import torch
        from . import ops
        i = int(i)
        if not 0 <= i < len(self.names):
            raise IndexError(f"ResidentJpegVideos: video {i} of {len(self.names)}")
        rs, L = self._rs, self.video_len[i]
        if out is None:
            out = torch.empty((L,) + tuple(self.shape), dtype=torch.uint8, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != rs.ident.device
              or not out.is_contiguous() or tuple(out.shape) != (L,) + tuple(self.shape)):
            raise ValueError(f"ResidentJpegVideos: out must be a contiguous uint8 {(L,) + tuple(self.shape)} tensor on "
                             f"{rs.ident.device}")
        with self._lock:
            if i not in self._tabs:
                tb = self.video_tables(i)
                to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)     # noqa: E731
                copies, d_reloc = {}, None
                if self._plan is not None:
                    # per coefficient chunk its range copies into the one staging region; the relocation rows of the whole
                    # video in one table (a resident video: no copies, delta 0 everywhere)
                    from .streamplan import stage_batch
                    reloc = np.zeros((L, 3), np.int64)
                    for lo, hi, _, _ in tb.chunks:
                        row = np.asarray([[self.video_first[i]], [lo], [L], [i]], np.int64)
                        copies[lo], reloc[lo:hi] = stage_batch(self._plan, rs.ext, row, hi - lo, 1, self._plan.stage_lo)
                    d_reloc = to(reloc)
                self._tabs[i] = (tb, to(tb.slot_set), to(tb.fill), to(tb.items), to(tb.waves), copies, d_reloc)
            tb, d_set, d_fill, d_items, d_waves, copies, d_reloc = self._tabs[i]
            self.stream.wait_stream(torch.cuda.current_stream(self.device))     # `out` may be a block this stream just freed

            def stage(lo):                  # a streamed video: a chunk's range copies, behind the last chunk's items launch
                for k, b_lo, b_hi, d in copies.get(lo, ()):
                    rs.jstream[d:d + b_hi - b_lo].copy_(rs.host_streams[k][b_lo:b_hi], non_blocking=True)

            with torch.cuda.stream(self.stream):
                rs.decode(tb, d_items, d_waves, d_set, out, reloc=d_reloc, before_items=stage if copies else None,
                          events=self._kernel_events)
                if bool((tb.fill >= 0).any()):
                    ops.jpeg_slot_fill(rs.side, d_fill, out)
                rs.err_host.copy_(rs.err, non_blocking=True)
            rs.raise_errors(self.stream, f"video {self.names[i]}", copy=False, reset=True)
        return out

    def sources(self):
        """[(name, length, fps, callable)]: the `videos` argument of stitch_videos / spot_videos / map_videos and, callables
        called, of predict_video_group; callable() is `frames(i)`"""
        import functools
        return [(self.names[i], self.video_len[i], self.fps[i], functools.partial(self.frames, i)) for i in range(len(self.names))]
