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
    an attribute that does not exist)."""
    r = int(radi_displacement)
    if r < 0:
        raise ValueError("radi_displacement must not be negative")
    T = int(clip_len)
    ids = np.asarray(clip_ids, np.int64).reshape(-1)
    label = np.zeros((len(ids), T), np.int64)
    labelD = np.zeros((len(ids), T), np.int64)
    for k, c in enumerate(ids):
        v = int(table.clip_video[c])
        base = int(table.clip_base[c])
        for e in range(int(table.ev_off[v]), int(table.ev_off[v + 1])):
            idx = (int(table.ev_frame[e]) - base) // stride
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

    def __init__(self, loader, tabs_a, tabs_b, B):
        self._loader, self.tabs_a, self.tabs_b, self.B = loader, tabs_a, tabs_b, B

    def __call__(self, lam):
        from . import ops
        ld = self._loader
        return ops.train_clip_gather_mix(ld.video, self.tabs_a, self.tabs_b, lam.contiguous(), ld.clip_len, ld.stride)


class ResidentClips:
    """The reference's training DataLoader over `ActionSpotDataset`, from videos that stay on the device.

    videos / classes / clip_len / stride / overlap / pad_len / require_events: `train_clip_table`.
    frames: per video one uint8 (num_frames,3,H,W) tensor -- host, pinned or device (`load_resident_videos` builds them
    from a frame directory).  All videos are packed into one device buffer, uploaded once in `chunk_bytes` chunks on a copy
    stream; the event arrays travel once, too.  The whole set must fit `max_resident_bytes` (ValueError otherwise, before
    anything is uploaded): the default 16 GiB holds 114 130 frames of 3 x 224 x 224 (76 minutes at 25 fps).  Epochs over a
    larger set, sharded over several resident subsets, are not implemented.
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
        import torch
        from . import feeder
        from .streams import new_stream
        if radi_displacement < 0:
            raise ValueError("radi_displacement must not be negative")
        if len(frames) != len(videos) or not videos:
            raise ValueError(f"ResidentClips: {len(videos)} videos, {len(frames)} frame tensors")
        srcs = []
        for v, fr in zip(videos, frames):
            if not isinstance(fr, torch.Tensor):
                fr = torch.as_tensor(np.asarray(fr))
            if fr.dtype != torch.uint8 or fr.dim() != 4:
                raise TypeError("ResidentClips: frames must be uint8 (num_frames,3,H,W) tensors")
            if fr.shape[0] != int(v["num_frames"]):
                raise ValueError(f"ResidentClips: video {v['video']} has {int(v['num_frames'])} frames, its tensor {fr.shape[0]}")
            srcs.append(fr)
        shape = tuple(srcs[0].shape[1:])
        if any(tuple(fr.shape[1:]) != shape for fr in srcs):
            raise ValueError(f"ResidentClips: the videos share one frame geometry, got "
                             f"{sorted({tuple(fr.shape[1:]) for fr in srcs})}")
        lengths = [int(fr.shape[0]) for fr in srcs]
        fb = int(np.prod(shape))
        if sum(lengths) * fb > max_resident_bytes:
            raise ValueError(f"ResidentClips: the videos need {sum(lengths) * fb} bytes on the device, more than "
                             f"max_resident_bytes={max_resident_bytes} (sharded epochs are not implemented)")
        self.table = train_clip_table(videos, classes, clip_len, stride, overlap, pad_len, require_events, radi_displacement)
        n = len(self.table.clip_video)
        if n == 0:
            raise ValueError("ResidentClips: no clips")
        self.clip_len, self.stride, self.radius, self.mixup = int(clip_len), int(stride), int(radi_displacement), bool(mixup)
        self.draws = ClipDraws(n, dataset_len, batch_size, mixup, seed, drop_last)
        if batch_size * self.clip_len > 65535:
            raise ValueError(f"ResidentClips: {batch_size} clips of {clip_len} frames exceed the gather's 65535 frame slots")
        self.device, self.depth = device, int(depth)
        # per clip: first packed frame and length of its video
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        cv = self.table.clip_video.astype(np.int64)
        self._rows = np.stack([offs[cv], self.table.clip_base, np.asarray(lengths, np.int64)[cv], cv])       # (4, n)
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
            self._host = [torch.zeros((4 * nops, B), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
            self._host_np = [h.numpy() for h in self._host]
            self._dev = [torch.zeros((4 * nops, B), dtype=torch.int64, device=device) for _ in range(self.depth)]
            self._frame = None if self.mixup else [torch.empty((B, T) + shape, dtype=torch.uint8, device=device)
                                                   for _ in range(self.depth)]
            nlab = nops * (2 if self.radius > 0 else 1)
            self._labels = [torch.empty((nlab, B, T), dtype=torch.int64, device=device) for _ in range(self.depth)]
        self._copied = [None] * self.depth        # event: the H2D copy of the slot's pinned table has finished
        self._consumed = [None] * self.depth      # event: the consumer is done with the slot's device buffers
        self._out = [False] * self.depth          # handed to a consumer and not released yet
        self._i = 0

    def __len__(self):
        return len(self.draws)

    def reseed(self, seed):
        """Start the draw stream anew from `seed` (the reference's workers reseed `random` per epoch, train_tdeed.py:126-127)."""
        d = self.draws
        self.draws = ClipDraws(d.n_clips, d.dataset_len, d.batch_size, d.mixup, seed, d.drop_last)

    def release(self, j, stream=None):
        """`feeder.done`: everything queued on `stream` (default: the current one) so far was the last use of slot j."""
        import torch
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        self._consumed[j] = ev
        self._out[j] = False

    def __iter__(self):
        import torch
        from . import ops
        T, S, r = self.clip_len, self.stride, self.radius
        for ia, ib in self.draws:
            j = self._i % self.depth
            self._i += 1
            if self._out[j]:
                raise RuntimeError(f"ResidentClips: the batch handed out {self.depth} batches ago was never released "
                                   "(feeder.done / feeder.prefetch); its buffers cannot be reused")
            if self._copied[j] is not None:
                self._copied[j].synchronize()                # a copy of `depth` batches ago: long finished
            B = len(ia)
            host = self._host_np[j]
            host[0:4, :B] = self._rows[:, ia]
            if ib is not None:
                host[4:8, :B] = self._rows[:, ib]
            dev, lab = self._dev[j], self._labels[j]
            with torch.cuda.stream(self.stream):
                if self._consumed[j] is not None:
                    self.stream.wait_event(self._consumed[j])   # do not overwrite buffers the consumer still reads
                dev.copy_(self._host[j], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self._copied[j] = ev
                batch = {}
                k = 0
                for op, sfx in enumerate(("", "2") if self.mixup else ("",)):
                    t4 = dev[4 * op:4 * op + 4]
                    label, labelD = ops.clip_labels(t4[3, :B], t4[1, :B], T, S, r, *self._ev, label=lab[k, :B],
                                                    labelD=lab[k + 1, :B] if r > 0 else None, displ=False)
                    batch["label" + sfx] = label
                    if r > 0:
                        batch["labelD" + sfx] = labelD
                    k += 2 if r > 0 else 1
                tabs_a = (dev[0, :B], dev[1, :B], dev[2, :B])
                if self.mixup:
                    batch["mix"] = _DeferredMix(self, tabs_a, (dev[4, :B], dev[5, :B], dev[6, :B]), B)
                else:
                    batch["frame"] = ops.train_clip_gather(self.video, *tabs_a, T, S, self._frame[j][:B])
                arrived = torch.cuda.Event()
                arrived.record(self.stream)
            batch["_slot"] = (self, j, arrived)
            self._out[j] = True
            yield batch
