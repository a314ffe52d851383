"""The reference's training dataset restated on the host, pure numpy.

The reference's training dataset (`ActionSpotDataset`, dataset/frame.py:30-256) lists every clip window of every video
(`_store_clips`, one frame apart with the default overlap), draws clips at random (`_get_one`), decodes the `clip_len`
JPEGs of every drawn clip in DataLoader workers and, with mixup, a second clip per item (`__getitem__`).  Here are
`train_clip_table` (the clip list), `rasterise_labels` (label / displacement rows, the reference of the label kernel) and
`ClipDraws` (the index stream of `__getitem__` under `random.seed(seed)` without workers).

For the reference's joint dataset (`ActionSpotDatasetJoint`, dataset/frame.py:640-663: two `ActionSpotDataset`s, a coin per
item) `JointDraws` restates the draws and `join_clip_tables` joins the two parts' tables.  The loaders are in `trainclips`.
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


class _Draws:
    """What the draw streams share: a pass of dataset_len items cut into batches -- the last one short as a DataLoader's
    is, or left out (and not drawn) with drop_last -- and a private `random.Random(seed)`, continued from pass to pass as
    the global generator would be; `reseed(seed)` starts it anew.  The global `random` stays untouched: `TDEEDModel.epoch()`
    takes its Beta(0.2, 0.2) mixup weights from it.  A subclass draws one item (`_item`: a tuple of ints, the mixup partner
    last); iterating yields a batch's items column by column, int64 (B,) each, None in the partner's place without mixup."""

    def __init__(self, n_clips, fewest, dataset_len, batch_size, mixup, seed, drop_last):
        if fewest <= 0 or dataset_len <= 0 or batch_size <= 0:
            raise ValueError("n_clips, dataset_len and batch_size must be positive")
        self.n_clips, self.dataset_len, self.batch_size = n_clips, int(dataset_len), int(batch_size)
        self.mixup, self.drop_last = bool(mixup), bool(drop_last)
        self.reseed(seed)

    def reseed(self, seed):
        self._rng = random.Random(seed)

    def __len__(self):
        full, rest = divmod(self.dataset_len, self.batch_size)
        return full + (1 if rest and not self.drop_last else 0)

    def __iter__(self):
        left, item = self.dataset_len, self._item
        for _ in range(len(self)):
            B = min(self.batch_size, left)
            left -= B
            cols = tuple(np.asarray(c, np.int64) for c in zip(*[item() for _ in range(B)]))
            yield cols if self.mixup else cols + (None,)


class ClipDraws(_Draws):
    """The clip indices `ActionSpotDataset.__getitem__` draws (dataset/frame.py:210-253) for a DataLoader without workers
    after `random.seed(seed)`: per item one `randint(0, n_clips-1)`, and a second one for the mixup partner.  Iterating
    yields one (idx int64 (B,), idx2 int64 (B,) | None) pair per batch (`_Draws`)."""

    def __init__(self, n_clips, dataset_len, batch_size, mixup, seed, drop_last=False):
        super().__init__(int(n_clips), n_clips, dataset_len, batch_size, mixup, seed, drop_last)

    def _item(self):
        draw, last = self._rng.randint, self.n_clips - 1
        return (draw(0, last), draw(0, last)) if self.mixup else (draw(0, last),)


class JointDraws(_Draws):
    """The draws of `ActionSpotDatasetJoint.__getitem__` (dataset/frame.py:651-660) over two `ActionSpotDataset`s, for a
    DataLoader without workers after `random.seed(seed)`: per item one `random()` -- below 0.5 the item comes from part 1,
    otherwise from part 2 --, then that part's `_get_one`: one `randint(0, n_k - 1)` on its clip count and, with mixup, a
    second one on the same part (the partner never comes from the other part).  The pass has dataset_len items -- the sum of
    the two parts' lengths (frame.py:662-663), given as that sum or as the pair --, cut into batches as `ClipDraws` does.
    Iterating yields (part int64 (B,) of 1 / 2, idx int64 (B,), idx2 int64 (B,) | None) per batch; idx counts inside the
    part."""

    def __init__(self, n_clips, dataset_len, batch_size, mixup, seed, drop_last=False):
        n_clips = tuple(int(n) for n in n_clips)
        total = int(sum(dataset_len)) if isinstance(dataset_len, (tuple, list)) else int(dataset_len)
        if len(n_clips) != 2:
            raise ValueError("JointDraws: the reference joins two datasets")
        super().__init__(n_clips, min(n_clips), total, batch_size, mixup, seed, drop_last)

    def _item(self):
        k = 0 if self._rng.random() < 0.5 else 1
        draw, last = self._rng.randint, self.n_clips[k] - 1
        return (k + 1, draw(0, last), draw(0, last)) if self.mixup else (k + 1, draw(0, last))


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
