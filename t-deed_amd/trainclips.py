"""Training batches drawn from resident videos.

The reference's training dataset (`ActionSpotDataset`, dataset/frame.py:30-256) lists every clip window of every video
(`_store_clips`, one frame apart with the default overlap), draws clips at random (`_get_one`), decodes the `clip_len`
JPEGs of every drawn clip in DataLoader workers and, with mixup, a second clip per item (`__getitem__`).  Each frame
belongs to about `clip_len` clips, so it is decoded about `clip_len` times per pass over the list.  Here every frame is
decoded ONCE, all videos stay on the device in one packed uint8 buffer, and a batch is

  * a strided gather from that buffer (ops.train_clip_gather), or with mixup one gather-and-blend launch that writes the
    fp32 batch directly (ops.train_clip_gather_mix, called by `TDEEDModel.epoch()` once it has drawn the weights);
  * its labels from the videos' event lists (ops.clip_labels).

The host side restates what the reference computes and is pure numpy: `train_clip_table` (the clip list),
`rasterise_labels` (label / displacement rows, the reference of the label kernel) and `ClipDraws` (the index stream of
`__getitem__` under `random.seed(seed)` without workers).  `ResidentClips` is the loader `epoch()` consumes.

`ResidentJpegClips` is the same loader over a set that stays on the device compressed: `load_resident_jpegs` packs the
entropy streams of every frame once, and a batch decodes the frames it drew on the device (csrc/jpeg.hip), one lane per
piece of a frame's scan; `batch_tables` is the host's share of a batch, pure numpy.

`JointResidentClips` / `JointResidentJpegClips` are the two loaders over the reference's joint dataset
(`ActionSpotDatasetJoint`, dataset/frame.py:640-663: two `ActionSpotDataset`s, a coin per item): `JointDraws` restates its
draws, both parts live in the one packed buffer (`join_clip_tables`, `join_resident_jpegs`), every clip keeps the stride of its
part and a batch is served by the per-clip-stride entries (ops.train_clip_gather_ps / train_clip_gather_mix_ps /
clip_labels_ps); the batch dicts gain 'dataset'.
"""
import random
from types import SimpleNamespace

import numpy as np

DEFAULT_PAD_LEN = 5                                   # dataset/frame.py:26


def clip_step(clip_len, overlap):
    """Frames between consecutive clip bases (dataset/frame.py:63-66)."""
    if not 0 <= overlap <= 1:
        raise ValueError("overlap is a proportion of clip_len in [0, 1]")
    return 1 if overlap == 1 else int((1 - overlap) * clip_len)


def _reaches(ev_frame, base, clip_len, stride, r):
    """Does any of the events label a position of the clip at `base`?  (-r <= idx < clip_len + r, frame.py:155)"""
    idx = (ev_frame.astype(np.int64) - base) // stride
    return bool(np.any((idx >= -r) & (idx < clip_len + r)))


def train_clip_table(videos, classes, clip_len, stride=1, overlap=1, pad_len=DEFAULT_PAD_LEN, require_events=False,
                     radi_displacement=0):
    """The clip list of `ActionSpotDataset._store_clips` (dataset/frame.py:97-179) as flat arrays.
    videos: [dict(video=name, num_frames=n, events=[dict(frame=f, label=name), ...]), ...]; the frames of a video are the
    contiguous run 0 .. num_frames-1 (`feeder.load_video`'s assumption; a video whose last files are missing is listed
    with the number of frames that exist).  classes: {label name: class index >= 1}.  SoccerNet's game-time parsing stays
    with the caller: events arrive as frame numbers.
    Per video, in order, the bases range(-pad_len*stride, max(0, num_frames-1 + (2*pad_len - clip_len)*stride), step); a
    clip whose sampled frames base + j*stride, j < clip_len, hit no existing frame is dropped (the reference's
    `frames_paths[1] != -1`); require_events keeps only clips that carry a label (the reference's SoccerNet rule; it needs
    the label radius `radi_displacement`).
    -> namespace(clip_video int32 (n,), clip_base int64 (n,), ev_frame / ev_class int32 (n_events,) in file order,
       ev_off int32 (videos + 1,), num_frames int64 (videos,))."""
    if clip_len <= 0 or stride <= 0 or pad_len < 0:
        raise ValueError("clip_len and stride must be positive, pad_len not negative")
    if radi_displacement < 0:
        raise ValueError("radi_displacement must not be negative")
    step = clip_step(clip_len, overlap)
    if step <= 0:
        raise ValueError(f"overlap {overlap} of clip_len {clip_len} leaves no step between clips")
    ev_frame, ev_class, ev_off = [], [], [0]
    clip_video, clip_base = [], []
    for v, video in enumerate(videos):
        n = int(video["num_frames"])
        evs = video.get("events", [])
        fr = np.array([int(e["frame"]) for e in evs], np.int32)
        ev_frame.append(fr)
        ev_class.append(np.array([int(classes[e["label"]]) for e in evs], np.int32))
        ev_off.append(ev_off[-1] + len(evs))
        for base in range(-pad_len * stride, max(0, n - 1 + (2 * pad_len - clip_len) * stride), step):
            # sampled frames base + j*stride; the first one >= 0 must exist
            j0 = 0 if base >= 0 else (-base + stride - 1) // stride
            if j0 >= clip_len or base + j0 * stride >= n:
                continue
            if require_events and not _reaches(fr, base, clip_len, stride, radi_displacement):
                continue
            clip_video.append(v)
            clip_base.append(base)
    cat = (lambda xs: np.concatenate(xs) if xs else np.zeros((0,), np.int32))
    return SimpleNamespace(clip_video=np.asarray(clip_video, np.int32), clip_base=np.asarray(clip_base, np.int64),
                           ev_frame=cat(ev_frame).astype(np.int32), ev_class=cat(ev_class).astype(np.int32),
                           ev_off=np.asarray(ev_off, np.int32),
                           num_frames=np.asarray([int(v["num_frames"]) for v in videos], np.int64))


def rasterise_labels(table, clip_ids, clip_len, stride, radi_displacement):
    """label / labelD rows of the clips `clip_ids` as `_store_clips` + `_get_one` build them (dataset/frame.py:151-159,
    226-233): per event of the clip's video, in list order, idx = (frame - base) // stride (Python's floor division; the
    numerator is negative for events before the base); when -r <= idx < T + r every i in [max(0, idx-r), min(T, idx+r+1))
    gets label[i] = class, labelD[i] = i - idx.  Later events overwrite earlier ones.
    -> (label int64 (n,T), labelD int64 (n,T)).  A negative radius raises ValueError (the reference's branch for it reads
    an attribute that does not exist).  stride: one for all, or one per entry of clip_ids (a joined table's clips keep
    the stride of their part)."""
    r = int(radi_displacement)
    if r < 0:
        raise ValueError("radi_displacement must not be negative")
    T = int(clip_len)
    ids = np.asarray(clip_ids, np.int64).reshape(-1)
    strides = _strides_of(stride, len(ids), "rasterise_labels")
    label = np.zeros((len(ids), T), np.int64)
    labelD = np.zeros((len(ids), T), np.int64)
    for k, c in enumerate(ids):
        v = int(table.clip_video[c])
        base = int(table.clip_base[c])
        for e in range(int(table.ev_off[v]), int(table.ev_off[v + 1])):
            idx = (int(table.ev_frame[e]) - base) // int(strides[k])
            if -r <= idx < T + r:
                for i in range(max(0, idx - r), min(T, idx + r + 1)):
                    label[k, i] = int(table.ev_class[e])
                    labelD[k, i] = i - idx
    return label, labelD


class ClipDraws:
    """The clip indices `ActionSpotDataset.__getitem__` draws (dataset/frame.py:210-253) for a DataLoader without workers
    after `random.seed(seed)`: per item one `randint(0, n_clips-1)`, and a second one for the mixup partner.  Iterating
    yields one (idx int64 (B,), idx2 int64 (B,) | None) pair per batch; the last batch is short as a DataLoader's is, or
    left out (and not drawn) with drop_last.  The stream continues from pass to pass, as the global generator would.
    The draws come from a private `random.Random(seed)`: the global `random` stays untouched, `TDEEDModel.epoch()` takes
    its Beta(0.2, 0.2) mixup weights from it."""

    def __init__(self, n_clips, dataset_len, batch_size, mixup, seed, drop_last=False):
        if n_clips <= 0 or dataset_len <= 0 or batch_size <= 0:
            raise ValueError("n_clips, dataset_len and batch_size must be positive")
        self.n_clips, self.dataset_len, self.batch_size = int(n_clips), int(dataset_len), int(batch_size)
        self.mixup, self.drop_last = bool(mixup), bool(drop_last)
        self._rng = random.Random(seed)

    def __len__(self):
        full, rest = divmod(self.dataset_len, self.batch_size)
        return full + (1 if rest and not self.drop_last else 0)

    def __iter__(self):
        left = self.dataset_len
        for _ in range(len(self)):
            B = min(self.batch_size, left)
            left -= B
            a, b = [], []
            for _ in range(B):
                a.append(self._rng.randint(0, self.n_clips - 1))
                if self.mixup:
                    b.append(self._rng.randint(0, self.n_clips - 1))
            yield np.asarray(a, np.int64), (np.asarray(b, np.int64) if self.mixup else None)


class JointDraws:
    """The draws of `ActionSpotDatasetJoint.__getitem__` (dataset/frame.py:651-660) over two `ActionSpotDataset`s, for a
    DataLoader without workers after `random.seed(seed)`: per item one `random()` -- below 0.5 the item comes from part 1,
    otherwise from part 2 --, then that part's `_get_one`: one `randint(0, n_k - 1)` on its clip count and, with mixup, a
    second one on the same part (the partner never comes from the other part).  The pass has dataset_len items -- the sum of
    the two parts' lengths (frame.py:662-663), given as that sum or as the pair --, cut into batches as `ClipDraws` does.
    Iterating yields (part int64 (B,) of 1 / 2, idx int64 (B,), idx2 int64 (B,) | None) per batch; idx counts inside the
    part.  A private `random.Random(seed)`, continued from pass to pass; `reseed(seed)` starts it anew."""

    def __init__(self, n_clips, dataset_len, batch_size, mixup, seed, drop_last=False):
        n_clips = tuple(int(n) for n in n_clips)
        total = int(sum(dataset_len)) if isinstance(dataset_len, (tuple, list)) else int(dataset_len)
        if len(n_clips) != 2:
            raise ValueError("JointDraws: the reference joins two datasets")
        if min(n_clips) <= 0 or total <= 0 or batch_size <= 0:
            raise ValueError("n_clips, dataset_len and batch_size must be positive")
        self.n_clips, self.dataset_len, self.batch_size = n_clips, total, int(batch_size)
        self.mixup, self.drop_last = bool(mixup), bool(drop_last)
        self._rng = random.Random(seed)

    def __len__(self):
        full, rest = divmod(self.dataset_len, self.batch_size)
        return full + (1 if rest and not self.drop_last else 0)

    def reseed(self, seed):
        self._rng = random.Random(seed)

    def __iter__(self):
        left = self.dataset_len
        for _ in range(len(self)):
            B = min(self.batch_size, left)
            left -= B
            part, a, b = [], [], []
            for _ in range(B):
                k = 0 if self._rng.random() < 0.5 else 1
                part.append(k + 1)
                a.append(self._rng.randint(0, self.n_clips[k] - 1))
                if self.mixup:
                    b.append(self._rng.randint(0, self.n_clips[k] - 1))
            yield np.asarray(part, np.int64), np.asarray(a, np.int64), (np.asarray(b, np.int64) if self.mixup else None)


def join_clip_tables(tables):
    """One clip table over several parts (`train_clip_table` per part, in order): the concatenation, with the video indices
    and the event offsets of a part shifted by the videos and events of the parts in front.
    -> namespace(train_clip_table's fields, clip_part int64 (n,) -- 1-based --, part_clips int64 (parts + 1,): the parts'
    clip boundaries, part_videos int64 (parts + 1,): their video boundaries)."""
    if not tables:
        raise ValueError("join_clip_tables: no parts")
    nv = np.concatenate([[0], np.cumsum([len(t.num_frames) for t in tables])]).astype(np.int64)
    ne = np.concatenate([[0], np.cumsum([len(t.ev_frame) for t in tables])]).astype(np.int64)
    nc = np.concatenate([[0], np.cumsum([len(t.clip_video) for t in tables])]).astype(np.int64)
    return SimpleNamespace(
        clip_video=np.concatenate([t.clip_video.astype(np.int64) + nv[k] for k, t in enumerate(tables)]).astype(np.int32),
        clip_base=np.concatenate([t.clip_base for t in tables]).astype(np.int64),
        ev_frame=np.concatenate([t.ev_frame for t in tables]).astype(np.int32),
        ev_class=np.concatenate([t.ev_class for t in tables]).astype(np.int32),
        ev_off=np.concatenate([[0]] + [t.ev_off[1:].astype(np.int64) + ne[k] for k, t in enumerate(tables)]).astype(np.int32),
        num_frames=np.concatenate([t.num_frames for t in tables]).astype(np.int64),
        clip_part=np.repeat(np.arange(1, len(tables) + 1, dtype=np.int64), np.diff(nc)), part_clips=nc, part_videos=nv)


def _strides_of(stride, n, who):
    """one stride per clip, int64 (n,), from a scalar or a per-clip sequence; ValueError unless every one is positive"""
    s = np.asarray(stride)
    if s.ndim == 0:
        s = np.full(n, int(s))
    s = s.astype(np.int64).reshape(-1)
    if s.size != n:
        raise ValueError(f"{who}: {s.size} strides for {n} clips")
    if n and int(s.min()) <= 0:
        raise ValueError(f"{who}: every stride must be positive")
    return s


def load_resident_videos(frame_dir, dataset, videos, pool=None, decode="host"):
    """The `frames` argument of `ResidentClips` from a frame directory: per video of the label list one uint8
    (num_frames,3,H,W) tensor (page-locked when a GPU runtime is there), every JPEG decoded once by
    `feeder.load_video(..., stride=1)` -- concurrently when `pool` is a `feeder.DecodePool`.
    `feeder.load_video` turns trailing missing files into zero frames, which is right for a clip window but not for the
    clip LIST: the reference drops a clip whose sampled frames do not exist, and `train_clip_table` decides that from
    `num_frames`.  A video whose last frame file is missing therefore raises ValueError here: list it with the number of
    frames that exist.
    decode: "host" (Pillow, host tensors) or "device" (`feeder.load_video_device`: the JPEG bytes go to the device and are
    decoded there; device tensors with the same contents, which `ResidentClips` takes as they are)."""
    import os
    from . import feeder
    if decode not in ("host", "device"):
        raise ValueError(f"decode must be 'host' or 'device', not {decode!r}")
    out = []
    for v in videos:
        n = int(v["num_frames"])
        path_fn = feeder.frame_locator(frame_dir, dataset, v["video"], v.get("_source_info"))[3]
        if n < 1 or not os.path.exists(path_fn(n - 1)):
            raise ValueError(f"video {v['video']}: num_frames={n}, but {path_fn(max(n, 1) - 1)} does not exist -- num_frames must "
                             "be the number of frames that exist")
        if decode == "device":
            out.append(feeder.load_video_device(frame_dir, dataset, v["video"], n, stride=1, source_info=v.get("_source_info"),
                                                pool=pool))
            continue
        out.append(feeder.load_video(frame_dir, dataset, v["video"], n, stride=1, source_info=v.get("_source_info"), pool=pool))
    return out


class _DeferredMix:
    """Mixup of one batch, deferred until the epoch has drawn the weights: `mix(lam)` launches the gather-and-blend on the
    current stream and returns the fp32 (B,T,3,H,W) batch, a fresh tensor from torch's allocator on that stream (the one
    allocation per batch on this path; `ops_bwd.mix_frames` allocates the same way).  `tabs_a` / `tabs_b`: the batch's
    (first, base, nframes) device tables.  Valid until the batch is released (`feeder.done`)."""

    def __init__(self, loader, tabs_a, tabs_b, B, strides=None):
        self._loader, self.tabs_a, self.tabs_b, self.B, self.strides = loader, tabs_a, tabs_b, B, strides

    def __call__(self, lam):
        from . import ops
        ld = self._loader
        if self.strides is not None:                # a joint batch: the device int32 (B,) stride of every clip
            return ops.train_clip_gather_mix_ps(ld.video, self.tabs_a, self.tabs_b, lam.contiguous(), ld.clip_len, self.strides)
        return ops.train_clip_gather_mix(ld.video, self.tabs_a, self.tabs_b, lam.contiguous(), ld.clip_len, ld.stride)


class _ClipLoader:
    """What the resident loaders share: the clip table and its draws, the per-clip (first packed frame, base, video length,
    video) rows, the ring bookkeeping of the batch slots and the label launches."""

    def _init_clips(self, videos, lengths, classes, clip_len, stride, overlap, radi_displacement, mixup, dataset_len,
                    batch_size, seed, pad_len, require_events, drop_last, device, depth):
        part = dict(videos=videos, classes=classes, stride=stride, overlap=overlap, require_events=require_events,
                    dataset_len=dataset_len)
        self._init_parts([part], lengths, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, device, depth,
                         joint=False)

    def _init_parts(self, parts, lengths, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, device, depth,
                    joint):
        """parts: [dict(videos, classes, stride=1, overlap=1, require_events=False, dataset_len)], each with its own clip
        list; lengths: the length of every video of every part, in order (they are packed in that order).  joint=False (one
        part): the table, the rows and the draws of the single-set loaders, nothing else.  joint=True: the table is the
        concatenation (`join_clip_tables`), the draws are `JointDraws`, and every clip keeps the stride and the number of
        its part (`_clip_stride` int32, `table.clip_part`); a batch's device rows then end in one row of strides -- int32, in
        the first half of the int64 row -- and one of part numbers, the batch's 'dataset'."""
        name = type(self).__name__
        tables = []
        for k, p in enumerate(parts):
            tables.append(train_clip_table(p["videos"], p["classes"], clip_len, p.get("stride", 1), p.get("overlap", 1), pad_len,
                                           p.get("require_events", False), radi_displacement))
            if len(tables[-1].clip_video) == 0:
                raise ValueError(f"{name}: no clips" + (f" in part {k + 1}" if joint else ""))
        self.clip_len, self.radius, self.mixup = int(clip_len), int(radi_displacement), bool(mixup)
        self.joint = bool(joint)
        self._nrows = (8 if self.mixup else 4) + (2 if joint else 0)
        if joint:
            self.tables, self.table = tables, join_clip_tables(tables)
            self.stride, self.strides = None, tuple(int(p.get("stride", 1)) for p in parts)
            counts = np.diff(self.table.part_clips)
            self._clip_stride = _strides_of(np.repeat(np.asarray(self.strides, np.int64), counts), int(counts.sum()),
                                            name).astype(np.int32)
            self.draws = JointDraws(counts, [int(p["dataset_len"]) for p in parts], batch_size, mixup, seed, drop_last)
        else:
            self.table = tables[0]
            self.stride = int(parts[0]["stride"])
            self.draws = ClipDraws(len(self.table.clip_video), parts[0]["dataset_len"], batch_size, mixup, seed, drop_last)
        if batch_size * self.clip_len > 65535:
            raise ValueError(f"{name}: {batch_size} clips of {clip_len} frames exceed the gather's 65535 frame slots")
        self.device, self.depth = device, int(depth)
        # per clip: first packed frame and length of its video
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        cv = self.table.clip_video.astype(np.int64)
        self._rows = np.stack([offs[cv], self.table.clip_base, np.asarray(lengths, np.int64)[cv], cv])       # (4, n)

    def _drawn(self, draw):
        """(clip ids of the batch, the partners' | None, part numbers | None) of one item of `self.draws`"""
        if not self.joint:
            return draw[0], draw[1], None
        part, ia, ib = draw
        lo = self.table.part_clips[part - 1]
        return lo + ia, (lo + ib if ib is not None else None), part

    def _joint_rows(self, host_rows, ia, part):
        """the stride and the part row of a joint batch into its page-locked (rows, B) int64 block"""
        B, k = len(ia), self._nrows - 2
        host_rows[k].view(np.int32)[:B] = self._clip_stride[ia]
        host_rows[k + 1, :B] = part

    def _joint_views(self, dev_rows, B):
        """(strides int32 (B,), dataset int64 (B,)) of a joint batch's device rows"""
        import torch
        k = self._nrows - 2
        return dev_rows[k].view(torch.int32)[:B], dev_rows[k + 1, :B]

    def _init_ring(self):
        self._copied = [None] * self.depth        # event: the H2D copy of the slot's pinned table has finished
        self._consumed = [None] * self.depth      # event: the consumer is done with the slot's device buffers
        self._out = [False] * self.depth          # handed to a consumer and not released yet
        self._i = 0

    def __len__(self):
        return len(self.draws)

    def reseed(self, seed):
        """Start the draw stream anew from `seed` (the reference's workers reseed `random` per epoch, train_tdeed.py:126-127)."""
        d = self.draws
        self.draws = type(d)(d.n_clips, d.dataset_len, d.batch_size, d.mixup, seed, d.drop_last)

    def release(self, j, stream=None):
        """`feeder.done`: everything queued on `stream` (default: the current one) so far was the last use of slot j."""
        import torch
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        self._consumed[j] = ev
        self._out[j] = False

    def _next_slot(self):
        """the ring entry of the next batch; the host waits only for the table copy of `depth` batches ago"""
        j = self._i % self.depth
        self._i += 1
        if self._out[j]:
            raise RuntimeError(f"{type(self).__name__}: the batch handed out {self.depth} batches ago was never released "
                               "(feeder.done / feeder.prefetch); its buffers cannot be reused")
        if self._copied[j] is not None:
            self._copied[j].synchronize()                # a copy of `depth` batches ago: long finished
        return j

    def _label_launches(self, dev, lab, B, batch, strides=None):
        """the ops.clip_labels launches of one batch from its (4 * operands, B) device rows into the slot's label buffer;
        strides: a joint batch's device int32 (B,) strides, shared by a clip and its partner"""
        from . import ops
        T, S, r = self.clip_len, self.stride, self.radius
        k = 0
        for op, sfx in enumerate(("", "2") if self.mixup else ("",)):
            t4 = dev[4 * op:4 * op + 4]
            out = dict(label=lab[k, :B], labelD=lab[k + 1, :B] if r > 0 else None, displ=False)
            if strides is not None:
                label, labelD = ops.clip_labels_ps(t4[3, :B], t4[1, :B], T, strides, r, *self._ev, **out)
            else:
                label, labelD = ops.clip_labels(t4[3, :B], t4[1, :B], T, S, r, *self._ev, **out)
            batch["label" + sfx] = label
            if r > 0:
                batch["labelD" + sfx] = labelD
            k += 2 if r > 0 else 1


class ResidentClips(_ClipLoader):
    """The reference's training DataLoader over `ActionSpotDataset`, from videos that stay on the device.

    videos / classes / clip_len / stride / overlap / pad_len / require_events: `train_clip_table`.
    frames: per video one uint8 (num_frames,3,H,W) tensor -- host, pinned or device (`load_resident_videos` builds them
    from a frame directory).  All videos are packed into one device buffer, uploaded once in `chunk_bytes` chunks on a copy
    stream; the event arrays travel once, too.  The whole set must fit `max_resident_bytes` (ValueError otherwise, before
    anything is uploaded): the default 16 GiB holds 114 130 frames of 3 x 224 x 224 (76 minutes at 25 fps).  Epochs over a
    larger set, sharded over several resident subsets, are not implemented for decoded frames; a larger set of JPEG files
    trains through `ResidentJpegClips(stream_clips=True)`, which keeps the streams that do not fit on the host.
    Iterating yields ceil(dataset_len / batch_size) batch dicts of device tensors (the floor with drop_last), the clips
    `ClipDraws(seed=seed)` draws: 'frame' uint8 (B,T,3,H,W), 'label' int64 (B,T) and, when radi_displacement > 0, 'labelD'.
    With mixup there is no 'frame': the batch carries 'label2' (/ 'labelD2') and 'mix', the deferred blend -- `mix(lam)`
    returns the fp32 batch lam * clip + (1 - lam) * partner, bit for bit what `ops_bwd.mix_frames` gives on the two uint8
    clips, which are never built; `TDEEDModel.epoch()` calls it with the weights it draws.  'contains_event' is not
    delivered (epoch() never reads it).
    Stream ordering: the loader launches on a stream of its own into a small ring of output buffers (uint8 clips, labels,
    index tables; the fp32 batch of `mix(lam)` is allocated per call on the consumer's stream).  A batch holds
    '_slot' = (loader, ring index, arrival event): the consumer brackets its use with `feeder.wait(batch)` /
    `feeder.done(batch)`, or iterates through `feeder.prefetch(loader)` which does so for it (`epoch()` does).  A ring
    entry is reused only after its batch was released.  The per-batch index table goes through a pinned buffer; before
    rewriting it the host waits only on its copy of `depth` batches ago -- normally long finished, and the one point where
    a host that runs more than `depth` batches ahead of the device is held back."""

    def __init__(self, videos, frames, classes, clip_len, stride=1, overlap=1, radi_displacement=0, mixup=False,
                 dataset_len=1, batch_size=8, seed=None, pad_len=DEFAULT_PAD_LEN, require_events=False, drop_last=False,
                 max_resident_bytes=16 << 30, device="cuda", depth=3, chunk_bytes=64 << 20):
        part = dict(videos=videos, frames=frames, classes=classes, stride=stride, overlap=overlap, require_events=require_events,
                    dataset_len=dataset_len)
        self._build([part], False, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, max_resident_bytes,
                    device, depth, chunk_bytes)

    def _build(self, parts, joint, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, max_resident_bytes,
               device, depth, chunk_bytes):
        """The constructor over parts (`_ClipLoader._init_parts`; every part with its `frames`): the videos of all parts are
        packed into the one buffer, in order."""
        import torch
        from . import feeder
        from .streams import new_stream
        who = type(self).__name__
        if radi_displacement < 0:
            raise ValueError("radi_displacement must not be negative")
        srcs = []
        for p in parts:
            videos, frames = p["videos"], p["frames"]
            if len(frames) != len(videos) or not videos:
                raise ValueError(f"{who}: {len(videos)} videos, {len(frames)} frame tensors")
            for v, fr in zip(videos, frames):
                if not isinstance(fr, torch.Tensor):
                    fr = torch.as_tensor(np.asarray(fr))
                if fr.dtype != torch.uint8 or fr.dim() != 4:
                    raise TypeError(f"{who}: frames must be uint8 (num_frames,3,H,W) tensors")
                if fr.shape[0] != int(v["num_frames"]):
                    raise ValueError(f"{who}: video {v['video']} has {int(v['num_frames'])} frames, its tensor {fr.shape[0]}")
                srcs.append(fr)
        shape = tuple(srcs[0].shape[1:])
        if any(tuple(fr.shape[1:]) != shape for fr in srcs):
            raise ValueError(f"{who}: the videos share one frame geometry, got "
                             f"{sorted({tuple(fr.shape[1:]) for fr in srcs})}")
        lengths = [int(fr.shape[0]) for fr in srcs]
        fb = int(np.prod(shape))
        if sum(lengths) * fb > max_resident_bytes:
            raise ValueError(f"{who}: the videos need {sum(lengths) * fb} bytes on the device, more than "
                             f"max_resident_bytes={max_resident_bytes} (sharded epochs are not implemented)")
        self._init_parts(parts, lengths, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, device, depth,
                         joint)
        self.stream = new_stream(device)
        self._copy_stream = new_stream(device, avoid=[self.stream])
        cur = torch.cuda.current_stream(device)
        self.stream.wait_stream(cur)
        self._copy_stream.wait_stream(cur)
        srcs = [fr.contiguous() if not fr.is_cuda else fr.to(device).contiguous() for fr in srcs]
        self._upload = feeder.PackedUpload(srcs, device, self._copy_stream, chunk_bytes)
        self.video = self._upload.video
        resident = self._upload.all()
        B, T, nops = int(batch_size), self.clip_len, 2 if self.mixup else 1
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(resident)
            self._ev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                             for a in (self.table.ev_off, self.table.ev_frame, self.table.ev_class))
            self._host = [torch.zeros((self._nrows, B), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
            self._host_np = [h.numpy() for h in self._host]
            self._dev = [torch.zeros((self._nrows, B), dtype=torch.int64, device=device) for _ in range(self.depth)]
            self._frame = None if self.mixup else [torch.empty((B, T) + shape, dtype=torch.uint8, device=device)
                                                   for _ in range(self.depth)]
            nlab = nops * (2 if self.radius > 0 else 1)
            self._labels = [torch.empty((nlab, B, T), dtype=torch.int64, device=device) for _ in range(self.depth)]
        self._init_ring()

    def __iter__(self):
        import torch
        from . import ops
        T, S = self.clip_len, self.stride
        for draw in self.draws:
            ia, ib, part = self._drawn(draw)
            j = self._next_slot()
            B = len(ia)
            host = self._host_np[j]
            host[0:4, :B] = self._rows[:, ia]
            if ib is not None:
                host[4:8, :B] = self._rows[:, ib]
            if part is not None:
                self._joint_rows(host, ia, part)
            dev, lab = self._dev[j], self._labels[j]
            with torch.cuda.stream(self.stream):
                if self._consumed[j] is not None:
                    self.stream.wait_event(self._consumed[j])   # do not overwrite buffers the consumer still reads
                dev.copy_(self._host[j], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self._copied[j] = ev
                batch = {}
                strides = None
                if part is not None:
                    strides, batch["dataset"] = self._joint_views(dev, B)
                self._label_launches(dev, lab, B, batch, strides)
                tabs_a = (dev[0, :B], dev[1, :B], dev[2, :B])
                if self.mixup:
                    batch["mix"] = _DeferredMix(self, tabs_a, (dev[4, :B], dev[5, :B], dev[6, :B]), B, strides)
                elif strides is not None:
                    batch["frame"] = ops.train_clip_gather_ps(self.video, *tabs_a, T, strides, self._frame[j][:B])
                else:
                    batch["frame"] = ops.train_clip_gather(self.video, *tabs_a, T, S, self._frame[j][:B])
                arrived = torch.cuda.Event()
                arrived.record(self.stream)
            batch["_slot"] = (self, j, arrived)
            self._out[j] = True
            yield batch


def _two_parts(parts, frames_key, who):
    """the `parts` argument of the joint loaders: two dicts, each with videos, classes, dataset_len and `frames_key`"""
    parts = [dict(p) for p in parts]
    if len(parts) != 2:
        raise ValueError(f"{who}: the reference joins two datasets, got {len(parts)} parts")
    for k, p in enumerate(parts):
        missing = [key for key in ("videos", frames_key, "classes", "dataset_len") if key not in p]
        if missing:
            raise ValueError(f"{who}: part {k + 1} lacks {missing}")
        p.setdefault("stride", 1)
        p.setdefault("overlap", 1)
        p.setdefault("require_events", False)
        if int(p["stride"]) <= 0:
            raise ValueError(f"{who}: part {k + 1}: stride must be positive")
    return parts


class JointResidentClips(ResidentClips):
    """The reference's joint training DataLoader -- `ActionSpotDatasetJoint` over two `ActionSpotDataset`s, the `pretrain`
    branch of `get_datasets` (dataset/datasets.py:60-94, dataset/frame.py:640-663) -- from videos that stay on the device.

    parts: two dicts, [dict(videos=, frames=, classes=, stride=1, overlap=1, require_events=False, dataset_len=)]; the
    first is the reference's dataset 1 (batch['dataset'] == 1), the second its dataset 2.  Each part has its own clip list
    (`train_clip_table` with its stride / overlap / classes / require_events); clip_len, radi_displacement, mixup, pad_len
    and the frame geometry are shared, as the reference collates the items of both into one tensor.  The other keyword
    arguments are `ResidentClips`'.
    Both parts live in the one packed buffer and one launch serves a whole batch: the gather, the gather-and-blend and the
    label kernel take the batch's per-clip stride table (ops.train_clip_gather_ps / train_clip_gather_mix_ps /
    clip_labels_ps).  The draws are `JointDraws(seed)`; a pass has dataset_len_1 + dataset_len_2 items.
    Batches are `ResidentClips`' plus 'dataset', device int64 (B,) of 1 / 2.  The labels are each part's own class numbers
    (`TDEEDModel.epoch()` shifts part 2's 'label' with `update_labels_2heads` and leaves 'label2' as it is, as the reference
    does).  A validation loader is the same call with mixup=False."""

    def __init__(self, parts, clip_len, radi_displacement=0, mixup=False, batch_size=8, seed=None, pad_len=DEFAULT_PAD_LEN,
                 drop_last=False, max_resident_bytes=16 << 30, device="cuda", depth=3, chunk_bytes=64 << 20):
        parts = _two_parts(parts, "frames", "JointResidentClips")
        self._build(parts, True, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, max_resident_bytes,
                    device, depth, chunk_bytes)


# ------------------------------------------------------------------------------------------------- resident JPEG streams
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
    as a file outside the decoder's subset does.  Missing files: as `load_resident_videos` -- num_frames must be the number
    of frames that exist (ValueError), a hole in front of an existing frame raises FileNotFoundError.
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
    """The tables of one batch of `ResidentJpegClips` (pure numpy; no file, no device).
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


# ------------------------------------------------------------------------------------------------- streamed sets: planning
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
    rows / clip_slot / n_slots / stride: as `batch_tables` (rows with the video in row 3); region_off: where the batch's staging
    region starts in the device buffer (plan.stage_lo + ring entry * plan.region_bytes).
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


class _ResidentStreams:
    """What `ResidentJpegClips` and `evalutil.ResidentJpegVideos` share: a packed set (`load_resident_jpegs`) made resident.
    The constructor is host arithmetic -- geometry, piece offsets, the resident bytes (stream, segment and piece tables,
    table sets, side buffer) held against max_resident_bytes, a ValueError naming `who` before anything is uploaded.
    `upload`, called inside the caller's stream context, copies the shards' streams into one buffer and the tables in one
    copy, runs the index pass (ops.jpeg_entropy_index, once per shard), reads the per-segment statuses back -- the one host
    synchronisation -- and decodes the fallback and the flagged frames once with `feeder.read_frame` into the side buffer
    (the budget is checked again when the index pass added side frames).  window = (top, left, wh, ww), here or through
    `set_window` before `upload`: the side buffer keeps that window of its frames only.  Afterwards: jstream, table_sets, pieces, side (device tensors or None),
    frame_set / side_row / piece_lo / piece_n per frame of the set, piece_mcu per piece row, `stats()`.
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


class _SlotMix:
    """Mixup of one batch of `ResidentJpegClips`: `mix(lam)` is ops_bwd.mix_frames on the batch's two decoded uint8 clips
    (current stream, a fresh fp32 tensor).  Valid until the batch is released (`feeder.done`)."""

    def __init__(self, a, b):
        self.a, self.b = a, b

    def __call__(self, lam):
        from . import ops_bwd
        return ops_bwd.mix_frames(self.a, self.b, lam.contiguous())


class ResidentJpegClips(_ClipLoader):
    """`ResidentClips` over a set that stays on the device COMPRESSED: the entropy streams of every frame are resident
    (`load_resident_jpegs`), and a batch decodes the frames of the clips it drew with csrc/jpeg.hip.  Clip list, draws,
    labels, batch dicts and the `_slot` hand-over are `ResidentClips`'; so are the keyword arguments, plus split_mcus (MCUs
    per piece, default one MCU row: the index pass at construction records the decoder state at every such boundary, and
    a batch decodes one lane per piece) and max_coeff_bytes (the coefficient buffer of a batch, chunked beyond it).

    Construction uploads the shards' streams into one buffer and the tables in one copy, runs the index pass
    (ops.jpeg_entropy_index, once per shard) and reads the per-segment statuses back -- its one host synchronisation.
    Frames in a shard's fallback (outside the decoder's subset, another sampling) and frames the index pass flagged are
    decoded once with `feeder.read_frame` and kept decoded in a side buffer; one of another size raises ValueError.
    Resident bytes -- stream, segment and piece tables, table sets, side buffer -- above max_resident_bytes raise
    ValueError before anything is uploaded, and again after the index pass if it added side frames.  `stats` reports them.

    Per batch the host computes `batch_tables` (numpy over the batch's frame slots), which travel through the ring entry's
    page-locked block in one copy; the loader's stream then zeroes the coefficients, runs ops.jpeg_entropy_items and
    ops.jpeg_pixels_rows into the entry's uint8 slot, and ops.jpeg_slot_fill for padding and side frames.  With mixup the
    slot holds both clips and `mix(lam)` is ops_bwd.mix_frames on them.  No host synchronisation per batch beyond
    `ResidentClips`' table-reuse wait; at the end of each pass the device error word is read (one synchronisation) and a
    non-zero word raises RuntimeError naming the pass.

    stream_clips=True: a set whose resident bytes exceed max_resident_bytes is accepted.  The tables of the whole set and the
    streams of the first videos that fit stay resident (`stream_plan`: fixed bytes and `depth` staging regions are reserved
    first; a budget too small for those raises ValueError naming the smallest that would do); the streams of the other videos
    stay in the host shards of `jpegs`, which must outlive the loader's use (it keeps references).  Per batch `stage_batch`
    gives one byte range per clip of a streamed video and shard; they are copied into the ring entry's staging region on a
    copy stream, behind the event of the last items launch that read the region, the relocation rows travel with the other
    tables, and the relocating items entry (ops.jpeg_entropy_items(..., reloc=...)) decodes from the copies -- no host
    synchronisation added, the copies of a batch overlap the decode of the one before.  Everything a consumer sees is the
    all-resident loader's bit for bit.  A shard with streamed frames must fit the staging memory (ValueError: pass a smaller
    shard_bytes to `load_resident_jpegs`); pageable shards (`pinned=False`) work, their copies block the host.  `stats` gains
    resident_videos, streamed_videos, stage_bytes, host_stream_bytes; `stage_log`, set to a list, collects the bytes copied
    per batch.  Without the keyword nothing changes."""

    def __init__(self, videos, jpegs, classes, clip_len, stride=1, overlap=1, radi_displacement=0, mixup=False,
                 dataset_len=1, batch_size=8, seed=None, pad_len=DEFAULT_PAD_LEN, require_events=False, drop_last=False,
                 max_resident_bytes=16 << 30, device="cuda", depth=3, chunk_bytes=64 << 20, split_mcus=None,
                 max_coeff_bytes=512 << 20, stream_clips=False):
        part = dict(videos=videos, classes=classes, stride=stride, overlap=overlap, require_events=require_events,
                    dataset_len=dataset_len)
        self._build([part], False, jpegs, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last,
                    max_resident_bytes, device, depth, chunk_bytes, split_mcus, max_coeff_bytes, stream_clips)

    def _build(self, parts, joint, jpegs, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last,
               max_resident_bytes, device, depth, chunk_bytes, split_mcus, max_coeff_bytes, stream_clips):
        """The constructor over parts (`_ClipLoader._init_parts`); jpegs: the one packed set that holds the videos of all
        parts, in order (`join_resident_jpegs`)."""
        import torch
        from . import ops
        from .streams import new_stream
        who = type(self).__name__
        if radi_displacement < 0:
            raise ValueError("radi_displacement must not be negative")
        videos = [v for p in parts for v in p["videos"]]
        if not videos or any(not p["videos"] for p in parts) or len(videos) != len(jpegs.video_len):
            raise ValueError(f"{who}: {len(videos)} videos, {len(jpegs.video_len)} in the packed set")
        for v, n in zip(videos, jpegs.video_len):
            if int(v["num_frames"]) != int(n):
                raise ValueError(f"{who}: video {v['video']} has {int(v['num_frames'])} frames, the packed set {int(n)}")
        rs = _ResidentStreams(who, jpegs, split_mcus, max_resident_bytes, streamed=stream_clips)
        n_frames, n_seg, H, W, samp = jpegs.n_frames, rs.n_seg, rs.H, rs.W, rs.samp
        self._init_parts(parts, [int(n) for n in jpegs.video_len], clip_len, radi_displacement, mixup, batch_size, seed, pad_len,
                         drop_last, device, depth, joint)
        self._who = who
        self.shape, self.samp, self.split_mcus = (3, H, W), samp, rs.split
        self._plan = self._ext = self._copy_stream = None
        if stream_clips:
            self._plan = rs.plan_streaming(self._rows, self.clip_len, self._clip_stride if joint else self.stride,
                                           2 if self.mixup else 1, int(batch_size), self.depth)
            self._ext = rs.ext
        dev = torch.device(device)
        self.stream = new_stream(device)
        self.stream.wait_stream(torch.cuda.current_stream(device))
        if stream_clips:
            self._copy_stream = new_stream(device, avoid=[self.stream])
        with torch.cuda.stream(self.stream):
            self._ev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                             for a in (self.table.ev_off, self.table.ev_frame, self.table.ev_class))
            rs.upload(self.stream, dev, chunk_bytes)
            self.pieces, self.table_sets, self.jstream, self.side = rs.pieces, rs.table_sets, rs.jstream, rs.side
            self._frame_set, self._side_row, self._piece_lo, self._piece_n = rs.frame_set, rs.side_row, rs.piece_lo, rs.piece_n
            self._side_host = rs.side_host
            # the ring: per entry one page-locked block and its device twin (clip rows, then the batch tables), the uint8
            # slot of both operands and the labels; one coefficient buffer, since every batch decodes on the one stream
            B, T, nops = int(batch_size), self.clip_len, 2 if self.mixup else 1
            self._cap = cap = nops * B * T
            if cap > 65535:
                raise ValueError(f"{who}: {nops} x {B} clips of {T} frames exceed the kernels' 65535 frame slots")
            self._fc = fc = ops.jpeg_frame_coeffs(W, H, samp)
            self._chunk = min(cap, max(1, int(max_coeff_bytes) // (2 * fc)))
            max_pieces = int(self._piece_n.max()) if n_frames else 0
            cap_items = max(cap * max_pieces, 1)
            cap_waves = cap_items // 64 + max(jpegs.n_sets, 1) * -(-cap // self._chunk) + 1
            sizes = [self._nrows * B * 8, cap * 4, cap * 4, cap_items * 8, cap_waves * 8] + ([cap * 24] if stream_clips else [])
            self._offs = np.concatenate([[0], np.cumsum([(s + 15) & ~15 for s in sizes])]).astype(np.int64)
            nbytes = int(self._offs[-1])
            self._host = [torch.zeros(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
            self._host_np = [h.numpy() for h in self._host]
            self._dev = [torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(self.depth)]
            self._slots = [torch.empty((nops, B, T, 3, H, W), dtype=torch.uint8, device=dev) for _ in range(self.depth)]
            nlab = nops * (2 if self.radius > 0 else 1)
            self._labels = [torch.empty((nlab, B, T), dtype=torch.int64, device=dev) for _ in range(self.depth)]
            self._coeff = torch.empty(self._chunk * fc, dtype=torch.int16, device=dev) if n_seg else None
            self._ident = torch.arange(cap, dtype=torch.int32, device=dev)
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
            self._err_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            if stream_clips:
                self._host_streams = rs.host_streams if n_seg else []
                self._staged = [None] * self.depth        # event: the copies into the entry's staging region have finished
                self._items_done = [None] * self.depth    # event: the last items launch that reads the entry's region
                self._copy_stream.wait_stream(self.stream)
        self.stage_log = None                   # set to a list: the byte count of every batch's range copies
        self._caps = (cap_items, cap_waves)
        self._pass = 0
        self.item_events = None                 # set to a list: (start, end) events around every jpeg_entropy_items launch
        self._init_ring()
        self.stats = rs.stats()

    def _views(self, block, B, np_side):
        """(rows int64 (4 * operands, B) -- two more for a joint loader --, slot_set, fill, items (cap, 2), waves (cap, 2)) of a
        ring block"""
        o = self._offs
        nr = self._nrows
        cap_items, cap_waves = self._caps
        if np_side:
            part = lambda i, dt: block[o[i]:o[i + 1]].view(dt)                                   # noqa: E731
            return (part(0, np.int64)[:nr * B].reshape(nr, B), part(1, np.int32)[:self._cap],
                    part(2, np.int32)[:self._cap], part(3, np.int32)[:2 * cap_items].reshape(cap_items, 2),
                    part(4, np.int32)[:2 * cap_waves].reshape(cap_waves, 2))
        import torch
        part = lambda i, dt: block[int(o[i]):int(o[i + 1])].view(dt)                              # noqa: E731
        return (part(0, torch.int64)[:nr * B].view(nr, B), part(1, torch.int32)[:self._cap],
                part(2, torch.int32)[:self._cap], part(3, torch.int32)[:2 * cap_items].view(cap_items, 2),
                part(4, torch.int32)[:2 * cap_waves].view(cap_waves, 2))

    def _stage(self, j, rows, at, strides):
        """Streamed sets: the relocation rows of the batch into entry j's page-locked block, and its range copies from the
        host shards into the entry's staging region on the copy stream, behind the last items launch that read the region.
        -> True when anything was copied (the loader's stream then waits for self._staged[j])."""
        import torch
        plan = self._plan
        copies, reloc = stage_batch(plan, self._ext, rows, self.clip_len, strides, plan.stage_lo + j * plan.region_bytes,
                                    n_slots=self._cap, clip_slot=at)
        o = self._offs
        self._host_np[j][o[5]:o[5] + self._cap * 24].view(np.int64).reshape(self._cap, 3)[:] = reloc
        if self.stage_log is not None:
            self.stage_log.append(sum(hi - lo for _, lo, hi, _ in copies))
        if not copies:
            return False
        cs = self._copy_stream
        if self._items_done[j] is not None:
            cs.wait_event(self._items_done[j])
        with torch.cuda.stream(cs):
            for k, lo, hi, d in copies:
                self.jstream[d:d + hi - lo].copy_(self._host_streams[k][lo:hi], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        self._staged[j] = ev
        return True

    def __iter__(self):
        import torch
        from . import ops
        T, S = self.clip_len, self.stride
        Bcap = self.draws.batch_size
        _, H, W = self.shape
        self._pass += 1
        for draw in self.draws:
            ia, ib, part = self._drawn(draw)
            j = self._next_slot()
            B = len(ia)
            h_rows, h_set, h_fill, h_items, h_waves = self._views(self._host_np[j], Bcap, True)
            h_rows[0:4, :B] = self._rows[:, ia]
            rows = self._rows[:, ia]
            at = np.arange(B, dtype=np.int64) * T
            if part is not None:                                # a joint batch: every clip at the stride of its part
                self._joint_rows(h_rows, ia, part)
                S = self._clip_stride[ia]
            if ib is not None:
                h_rows[4:8, :B] = self._rows[:, ib]
                rows = np.concatenate([rows, self._rows[:, ib]], 1)
                at = np.concatenate([at, (Bcap + np.arange(B, dtype=np.int64)) * T])
                if part is not None:
                    S = np.concatenate([S, S])                  # the partner comes from the same part
            tb = batch_tables(rows, T, S, self._frame_set, self._side_row, self._piece_lo, self._piece_n, n_slots=self._cap,
                              clip_slot=at, chunk_slots=self._chunk)
            h_set[:], h_fill[:] = tb.slot_set, tb.fill
            h_items[:tb.items.shape[0]] = tb.items
            h_waves[:tb.waves.shape[0]] = tb.waves
            staged = self._plan is not None and self._stage(j, rows, at, S)
            slot, lab = self._slots[j], self._labels[j]
            with torch.cuda.stream(self.stream):
                if self._consumed[j] is not None:
                    self.stream.wait_event(self._consumed[j])   # do not overwrite buffers the consumer still reads
                self._dev[j].copy_(self._host[j], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self._copied[j] = ev
                d_rows, d_set, d_fill, d_items, d_waves = self._views(self._dev[j], Bcap, False)
                batch = {}
                strides = None
                if part is not None:
                    strides, batch["dataset"] = self._joint_views(d_rows, B)
                self._label_launches(d_rows, lab, B, batch, strides)
                d_reloc = None
                if self._plan is not None:
                    o = self._offs
                    d_reloc = self._dev[j][int(o[5]):int(o[5]) + self._cap * 24].view(torch.int64).view(self._cap, 3)
                    if staged:
                        self.stream.wait_event(self._staged[j])
                for lo, hi, w_lo, w_hi in tb.chunks:
                    self._coeff[:(hi - lo) * self._fc].zero_()
                    if self.item_events is not None:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(self.stream)
                    ops.jpeg_entropy_items(self.jstream, self.pieces, d_items[:tb.items.shape[0]], d_waves[w_lo:w_hi],
                                           self.table_sets, W, H, self.samp, lo, hi - lo, self._coeff, self._err, reloc=d_reloc)
                    if self.item_events is not None:
                        e1.record(self.stream)
                        self.item_events.append((e0, e1))
                    ops.jpeg_pixels_rows(self._coeff, d_set, self.table_sets, slot, self._ident, lo, hi - lo, self.samp)
                if staged:
                    done = torch.cuda.Event()
                    done.record(self.stream)
                    self._items_done[j] = done
                ops.jpeg_slot_fill(self.side, d_fill, slot)
                if self.mixup:
                    batch["mix"] = _SlotMix(slot[0, :B], slot[1, :B])
                else:
                    batch["frame"] = slot[0, :B]
                arrived = torch.cuda.Event()
                arrived.record(self.stream)
            batch["_slot"] = (self, j, arrived)
            self._out[j] = True
            yield batch
        with torch.cuda.stream(self.stream):
            self._err_host.copy_(self._err, non_blocking=True)
        self.stream.synchronize()                               # the one synchronisation of a pass
        word = int(self._err_host[0])
        if word:
            codes = [c for c in range(1, 8) if word >> c & 1]
            raise RuntimeError(f"{self._who}: pass {self._pass} met decode errors on the device (status codes {codes}); "
                               "the resident streams or tables are damaged")


class JointResidentJpegClips(ResidentJpegClips):
    """`JointResidentClips` over parts that stay on the device compressed: parts as there, with `jpegs`
    (`load_resident_jpegs` of the part's videos) in place of `frames`.  The two packed sets are joined into one
    (`join_resident_jpegs`: streams reused, table sets renumbered, a part 2 of another chroma sampling through the side
    buffer, another width or height ValueError), so one items launch and one pixel pass decode the clips of both parts;
    `batch_tables` -- and, with stream_clips=True, `stream_plan` / `stage_batch` -- take the batch's per-clip strides.  The
    other keyword arguments are `ResidentJpegClips`'.  Everything a consumer sees equals `JointResidentClips` fed the decoded
    frames, bit for bit."""

    def __init__(self, parts, clip_len, radi_displacement=0, mixup=False, batch_size=8, seed=None, pad_len=DEFAULT_PAD_LEN,
                 drop_last=False, max_resident_bytes=16 << 30, device="cuda", depth=3, chunk_bytes=64 << 20, split_mcus=None,
                 max_coeff_bytes=512 << 20, stream_clips=False):
        parts = _two_parts(parts, "jpegs", "JointResidentJpegClips")
        for k, p in enumerate(parts):
            if len(p["videos"]) != len(p["jpegs"].video_len):
                raise ValueError(f"JointResidentJpegClips: part {k + 1} lists {len(p['videos'])} videos, its packed set "
                                 f"{len(p['jpegs'].video_len)}")
        jpegs = join_resident_jpegs(parts[0]["jpegs"], parts[1]["jpegs"])
        self._build(parts, True, jpegs, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last,
                    max_resident_bytes, device, depth, chunk_bytes, split_mcus, max_coeff_bytes, stream_clips)
