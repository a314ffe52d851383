"""Training batches drawn from resident videos.

Every frame of the reference's training dataset (`cliptable`) belongs to about `clip_len` clips, so the reference decodes it
about `clip_len` times per pass over the clip list.  Here every frame is decoded ONCE, all videos stay on the device in one
packed uint8 buffer, and a batch is

  * a strided gather from that buffer (ops.train_clip_gather), or with mixup one gather-and-blend launch that writes the
    fp32 batch directly (ops.train_clip_gather_mix, called by `TDEEDModel.epoch()` once it has drawn the weights);
  * its labels from the videos' event lists (ops.clip_labels).

`ResidentClips` is the loader `epoch()` consumes.  `ResidentJpegClips` is the same loader over a set that stays on the
device compressed (`jpegsets`, `residentstreams`; larger than the device budget: `streamplan`).

`JointResidentClips` / `JointResidentJpegClips` are the two loaders over the reference's joint dataset: both parts live in
the one packed buffer (`join_clip_tables`, `join_resident_jpegs`), every clip keeps the stride of its part and a batch is
served by the same three ops, given the batch's per-clip stride table; the batch dicts gain 'dataset'.  The names of
`cliptable`, `jpegsets`, `streamplan` and `residentstreams` are importable from here, too.
"""
import numpy as np

from .cliptable import (DEFAULT_PAD_LEN, ClipDraws, JointDraws, _reaches, _strides_of, clip_step,  # noqa: F401
                        join_clip_tables, rasterise_labels, train_clip_table)
from .jpegsets import (ResidentJpegs, _cut_waves, batch_tables, join_resident_jpegs, load_resident_jpegs,  # noqa: F401
                       video_tables)
from .residentstreams import ResidentStreams
from .streamplan import (_NO_BYTE, _clip_ranges, _round16, _shard_first, frame_extents, stage_batch,  # noqa: F401
                         stream_plan)


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
    (first, base, nframes) device tables; `strides`: the batch's stride as the ops take it (`_ClipLoader._batch_stride`).
    Valid until the batch is released (`feeder.done`)."""

    def __init__(self, loader, tabs_a, tabs_b, B, strides):
        self._loader, self.tabs_a, self.tabs_b, self.B, self.strides = loader, tabs_a, tabs_b, B, strides

    def __call__(self, lam):
        from . import ops
        ld = self._loader
        return ops.train_clip_gather_mix(ld.video, self.tabs_a, self.tabs_b, lam.contiguous(), ld.clip_len, self.strides)


class _ClipLoader:
    """What the resident loaders share: the clip table and its draws, the per-clip (first packed frame, base, video length,
    video) rows, the loader's stream, the ring of batch slots with its label buffers (a negative label radius is refused by
    `train_clip_table`), the label launches and the batch loop, to which a subclass supplies `_frame_launches` and, where
    it has any, `_host_share` and `_end_pass`."""

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

    def _open_stream(self):
        """the loader's stream, behind what the caller's stream has queued so far"""
        import torch
        from .streams import new_stream
        self.stream = new_stream(self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _init_ring(self, B):
        """Inside the loader's stream context: the event arrays, uploaded once, the label buffers of the `depth` ring entries
        and their bookkeeping.  The subclass adds, per entry, `_host` / `_dev` -- the page-locked block of a batch and its
        device twin -- and `_host_rows` / `_dev_rows`, their (rows, B) int64 clip rows."""
        import torch
        self._ev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                         for a in (self.table.ev_off, self.table.ev_frame, self.table.ev_class))
        nlab = (2 if self.mixup else 1) * (2 if self.radius > 0 else 1)
        self._labels = [torch.empty((nlab, B, self.clip_len), dtype=torch.int64, device=self.device) for _ in range(self.depth)]
        self._copied = [None] * self.depth        # event: the H2D copy of the slot's pinned table has finished
        self._consumed = [None] * self.depth      # event: the consumer is done with the slot's device buffers
        self._out = [False] * self.depth          # handed to a consumer and not released yet
        self._i = self._pass = 0

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

    def _batch_stride(self, dev_rows, B):
        """The stride the ops take for a batch: the loader's int, or -- a joint batch -- the device int32 (B,) table in its
        device rows, every clip's own stride (shared by a clip and its partner)."""
        if not self.joint:
            return self.stride
        import torch
        return dev_rows[self._nrows - 2].view(torch.int32)[:B]

    def __len__(self):
        return len(self.draws)

    def reseed(self, seed):
        """Start the draw stream anew from `seed` (the reference's workers reseed `random` per epoch, train_tdeed.py:126-127)."""
        self.draws.reseed(seed)

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

    def _label_launches(self, dev, lab, B, batch, stride):
        """the ops.clip_labels launches of one batch from its (4 * operands, B) device rows into the slot's label buffer;
        stride: `_batch_stride`"""
        from . import ops
        T, r = self.clip_len, self.radius
        k = 0
        for op, sfx in enumerate(("", "2") if self.mixup else ("",)):
            t4 = dev[4 * op:4 * op + 4]
            label, labelD = ops.clip_labels(t4[3, :B], t4[1, :B], T, stride, r, *self._ev, label=lab[k, :B],
                                            labelD=lab[k + 1, :B] if r > 0 else None, displ=False)
            batch["label" + sfx] = label
            if r > 0:
                batch["labelD" + sfx] = labelD
            k += 2 if r > 0 else 1

    def __iter__(self):
        """One pass.  Per batch: its draws and ring entry; the rows of the clips, of the partners and of a joint batch into
        the entry's page-locked block, then `_host_share` -- whatever else the subclass computes or queues off the loader's
        stream; on the loader's stream, behind the consumer's release of the entry, one copy of the block, the labels and
        `_frame_launches`; the batch leaves with '_slot' = (loader, ring entry, arrival event).  `_end_pass` closes a pass."""
        import torch
        self._pass += 1
        for draw in self.draws:
            ia, ib, part = self._drawn(draw)
            j = self._next_slot()
            B = len(ia)
            host = self._host_rows[j]
            host[0:4, :B] = self._rows[:, ia]
            if ib is not None:
                host[4:8, :B] = self._rows[:, ib]
            if part is not None:
                self._joint_rows(host, ia, part)
            work = self._host_share(j, B, ia, ib)
            dev = self._dev_rows[j]
            with torch.cuda.stream(self.stream):
                if self._consumed[j] is not None:
                    self.stream.wait_event(self._consumed[j])   # do not overwrite buffers the consumer still reads
                self._dev[j].copy_(self._host[j], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self._copied[j] = ev
                batch = {}
                stride = self._batch_stride(dev, B)
                if part is not None:
                    batch["dataset"] = dev[self._nrows - 1, :B]
                self._label_launches(dev, self._labels[j], B, batch, stride)
                self._frame_launches(j, B, stride, work, batch)
                arrived = torch.cuda.Event()
                arrived.record(self.stream)
            batch["_slot"] = (self, j, arrived)
            self._out[j] = True
            yield batch
        self._end_pass()

    def _host_share(self, j, B, ia, ib):
        """the subclass's host work for ring entry j's batch, off the loader's stream -> what its `_frame_launches` needs"""

    def _end_pass(self):
        """after the last batch of a pass"""


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
        self._open_stream()
        self._copy_stream = new_stream(device, avoid=[self.stream])
        self._copy_stream.wait_stream(torch.cuda.current_stream(device))
        srcs = [fr.contiguous() if not fr.is_cuda else fr.to(device).contiguous() for fr in srcs]
        self._upload = feeder.PackedUpload(srcs, device, self._copy_stream, chunk_bytes)
        self.video = self._upload.video
        resident = self._upload.all()
        B = int(batch_size)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(resident)
            self._init_ring(B)
            self._host = [torch.zeros((self._nrows, B), dtype=torch.int64).pin_memory() for _ in range(self.depth)]
            self._host_rows = [h.numpy() for h in self._host]
            self._dev = self._dev_rows = [torch.zeros((self._nrows, B), dtype=torch.int64, device=device) for _ in range(self.depth)]
            self._frame = None if self.mixup else [torch.empty((B, self.clip_len) + shape, dtype=torch.uint8, device=device)
                                                   for _ in range(self.depth)]

    def _frame_launches(self, j, B, stride, work, batch):
        from . import ops
        dev = self._dev_rows[j]
        tabs_a = (dev[0, :B], dev[1, :B], dev[2, :B])
        if self.mixup:
            batch["mix"] = _DeferredMix(self, tabs_a, (dev[4, :B], dev[5, :B], dev[6, :B]), B, stride)
        else:
            batch["frame"] = ops.train_clip_gather(self.video, *tabs_a, self.clip_len, stride, self._frame[j][:B])


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
    label kernel take the batch's per-clip stride table (ops.train_clip_gather / train_clip_gather_mix / clip_labels with
    a table for `stride`).  The draws are `JointDraws(seed)`; a pass has dataset_len_1 + dataset_len_2 items.
    Batches are `ResidentClips`' plus 'dataset', device int64 (B,) of 1 / 2.  The labels are each part's own class numbers
    (`TDEEDModel.epoch()` shifts part 2's 'label' with `update_labels_2heads` and leaves 'label2' as it is, as the reference
    does).  A validation loader is the same call with mixup=False."""

    def __init__(self, parts, clip_len, radi_displacement=0, mixup=False, batch_size=8, seed=None, pad_len=DEFAULT_PAD_LEN,
                 drop_last=False, max_resident_bytes=16 << 30, device="cuda", depth=3, chunk_bytes=64 << 20):
        parts = _two_parts(parts, "frames", "JointResidentClips")
        self._build(parts, True, clip_len, radi_displacement, mixup, batch_size, seed, pad_len, drop_last, max_resident_bytes,
                    device, depth, chunk_bytes)


# ------------------------------------------------------------------------------------------------- resident JPEG streams
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
    ops.jpeg_pixels_rows into the entry's uint8 slot (`ResidentStreams.decode`), and ops.jpeg_slot_fill for padding and side
    frames.  With mixup the slot holds both clips and `mix(lam)` is ops_bwd.mix_frames on them.  No host synchronisation per
    batch beyond `ResidentClips`' table-reuse wait; at the end of each pass the device error word is read (one
    synchronisation) and a non-zero word raises RuntimeError naming the pass.

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
        from .streams import new_stream
        who = type(self).__name__
        videos = [v for p in parts for v in p["videos"]]
        if not videos or any(not p["videos"] for p in parts) or len(videos) != len(jpegs.video_len):
            raise ValueError(f"{who}: {len(videos)} videos, {len(jpegs.video_len)} in the packed set")
        for v, n in zip(videos, jpegs.video_len):
            if int(v["num_frames"]) != int(n):
                raise ValueError(f"{who}: video {v['video']} has {int(v['num_frames'])} frames, the packed set {int(n)}")
        self._rs = rs = ResidentStreams(who, jpegs, split_mcus, max_resident_bytes, streamed=stream_clips)
        self._init_parts(parts, [int(n) for n in jpegs.video_len], clip_len, radi_displacement, mixup, batch_size, seed, pad_len,
                         drop_last, device, depth, joint)
        self.shape, self.samp, self.split_mcus = (3, rs.H, rs.W), rs.samp, rs.split
        self._plan = self._copy_stream = None
        if stream_clips:
            self._plan = rs.plan_streaming(self._rows, self.clip_len, self._clip_stride if joint else self.stride,
                                           2 if self.mixup else 1, int(batch_size), self.depth)
        dev = torch.device(device)
        self._open_stream()
        if stream_clips:
            self._copy_stream = new_stream(device, avoid=[self.stream])
        with torch.cuda.stream(self.stream):
            B, T, nops = int(batch_size), self.clip_len, 2 if self.mixup else 1
            self._init_ring(B)
            rs.upload(self.stream, dev, chunk_bytes)
            self.pieces, self.table_sets, self.jstream, self.side = rs.pieces, rs.table_sets, rs.jstream, rs.side
            # the ring: per entry one page-locked block and its device twin (clip rows, then the batch tables) and the uint8
            # slot of both operands; one coefficient buffer (`rs`), since every batch decodes on the one stream
            self._cap = cap = nops * B * T
            if cap > 65535:
                raise ValueError(f"{who}: {nops} x {B} clips of {T} frames exceed the kernels' 65535 frame slots")
            rs.decode_buffers(dev, cap, max_coeff_bytes)
            self._chunk = rs.chunk
            cap_items = max(cap * (int(rs.piece_n.max()) if jpegs.n_frames else 0), 1)
            cap_waves = cap_items // 64 + max(jpegs.n_sets, 1) * -(-cap // self._chunk) + 1
            self._caps = (cap_items, cap_waves)
            sizes = [self._nrows * B * 8, cap * 4, cap * 4, cap_items * 8, cap_waves * 8] + ([cap * 24] if stream_clips else [])
            self._offs = [0] + [int(x) for x in np.cumsum([(s + 15) & ~15 for s in sizes])]
            self._host = [torch.zeros(self._offs[-1], dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
            self._dev = [torch.zeros(self._offs[-1], dtype=torch.uint8, device=dev) for _ in range(self.depth)]
            self._host_tabs = [self._views(h.numpy(), B, np.int32, np.int64) for h in self._host]
            self._dev_tabs = [self._views(d, B, torch.int32, torch.int64) for d in self._dev]
            self._host_rows, self._dev_rows = [t[0] for t in self._host_tabs], [t[0] for t in self._dev_tabs]
            self._slots = [torch.empty((nops, B, T) + self.shape, dtype=torch.uint8, device=dev) for _ in range(self.depth)]
            if stream_clips:
                self._host_streams = rs.host_streams if rs.n_seg else []
                self._staged = [None] * self.depth        # event: the copies into the entry's staging region have finished
                self._items_done = [None] * self.depth    # event: the last items launch that reads the entry's region
                self._copy_stream.wait_stream(self.stream)
        self.stage_log = None                   # set to a list: the byte count of every batch's range copies
        self.item_events = None                 # set to a list: (start, end) events around every jpeg_entropy_items launch
        self.stats = rs.stats()

    def _views(self, block, B, i32, i64):
        """(rows int64 (4 * operands, B) -- two more for a joint loader --, slot_set, fill, items (cap, 2), waves (cap, 2),
        relocation rows int64 (cap, 3) of a streamed set | None) of a ring block; i32 / i64: the block's own dtypes, numpy's
        or torch's"""
        o, cap, (cap_items, cap_waves) = self._offs, self._cap, self._caps

        def part(i, dtype, *shape):
            return block[o[i]:o[i + 1]].view(dtype)[:int(np.prod(shape))].reshape(shape)
        return (part(0, i64, self._nrows, B), part(1, i32, cap), part(2, i32, cap), part(3, i32, cap_items, 2),
                part(4, i32, cap_waves, 2), part(5, i64, cap, 3) if self._rs.streamed else None)

    def _stage(self, j, rows, at, strides):
        """Streamed sets: the relocation rows of the batch into entry j's page-locked block, and its range copies from the
        host shards into the entry's staging region on the copy stream, behind the last items launch that read the region.
        -> True when anything was copied (the loader's stream then waits for self._staged[j])."""
        import torch
        plan = self._plan
        copies, reloc = stage_batch(plan, self._rs.ext, rows, self.clip_len, strides, plan.stage_lo + j * plan.region_bytes,
                                    n_slots=self._cap, clip_slot=at)
        self._host_tabs[j][5][:] = reloc
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

    def _host_share(self, j, B, ia, ib):
        """`batch_tables` of the batch -- the partners' slots at Bcap * T, a joint batch with every clip at the stride of its
        part -- into entry j's page-locked block and, for a streamed set, its staging -> (the tables, anything staged?)"""
        T, Bcap, rs = self.clip_len, self.draws.batch_size, self._rs
        ids, at = ia, np.arange(B, dtype=np.int64) * T
        if ib is not None:
            ids, at = np.concatenate([ia, ib]), np.concatenate([at, (Bcap + np.arange(B, dtype=np.int64)) * T])
        rows = self._rows[:, ids]
        S = self._clip_stride[ids] if self.joint else self.stride
        tb = batch_tables(rows, T, S, rs.frame_set, rs.side_row, rs.piece_lo, rs.piece_n, n_slots=self._cap, clip_slot=at,
                          chunk_slots=self._chunk)
        _, h_set, h_fill, h_items, h_waves, _ = self._host_tabs[j]
        h_set[:], h_fill[:] = tb.slot_set, tb.fill
        h_items[:tb.items.shape[0]] = tb.items
        h_waves[:tb.waves.shape[0]] = tb.waves
        return tb, self._plan is not None and self._stage(j, rows, at, S)

    def _frame_launches(self, j, B, stride, work, batch):
        import torch
        from . import ops
        tb, staged = work
        slot = self._slots[j]
        _, d_set, d_fill, d_items, d_waves, d_reloc = self._dev_tabs[j]
        if staged:
            self.stream.wait_event(self._staged[j])
        timed = [] if self.item_events is not None else None
        self._rs.decode(tb, d_items[:tb.items.shape[0]], d_waves, d_set, slot, reloc=d_reloc, events=timed)
        if timed:
            self.item_events += [ev[:2] for ev in timed]        # (start, end) around every items launch
        if staged:
            done = torch.cuda.Event()
            done.record(self.stream)
            self._items_done[j] = done
        ops.jpeg_slot_fill(self.side, d_fill, slot)
        if self.mixup:
            batch["mix"] = _SlotMix(slot[0, :B], slot[1, :B])
        else:
            batch["frame"] = slot[0, :B]

    def _end_pass(self):
        self._rs.raise_errors(self.stream, f"pass {self._pass}")       # the one synchronisation of a pass


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
