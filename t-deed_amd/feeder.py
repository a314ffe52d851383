"""Input pipeline of the hot path: JPEG frames -> uint8 clips -> device, overlapped with compute.

The reference decodes every frame with `torchvision.io.read_image` inside DataLoader workers (/root/reference/dataset/
frame.py:263-382 `FrameReader.load_frames`, 546-626 `FrameReaderVideo`), stacks them to a uint8 (T,3,H,W) clip and lets
`epoch()` / `predict()` move the batch with a blocking `.to(device).float()` (model/model.py:216, 342): 4 bytes per pixel
over PCIe, no overlap with the forward.  Here

  * `read_frame` / `load_clip` decode JPEGs (Pillow's libjpeg, the same decoder family as torchvision's) straight into a
    caller-provided uint8 buffer -- a slot of a pinned staging ring -- with the reference's zero padding of clips that
    start before / end after the video;
  * `PinnedRing` owns `depth` pinned host slots and matching device buffers; `upload()` issues ONE asynchronous H2D copy
    of a uint8 batch (1 byte per pixel: 15 MB per clip of 100 x 224 x 224 frames, ~0.24 ms at PCIe 5 x16) on a dedicated
    copy stream and returns the device tensor with the event that marks its arrival;
  * `prefetch(loader, ...)` wraps any iterable of batch dicts (the reference's loaders) so that batch i+1 is staged and
    copied while batch i is being processed: `TDEEDModel.epoch()` uses it for both the validation and the training loop.

Only plumbing lives here (host memory, streams, events); nothing in this file computes on the device, with one opt-in
exception: `load_video_device` hands the JPEG bytes of a video to the decode kernels (csrc/jpeg.hip) and returns the
frames as a device tensor, and `device_clip_batches` does the same per training batch (`clip_batches` with the decode on
the device).
"""
import os

import numpy as np
from types import SimpleNamespace
import torch


def read_frame(path, out=None):
    """JPEG (or any Pillow-readable image) -> uint8 (3,H,W) RGB, like torchvision.io.read_image (frame.py:271, 555).
    out: optional uint8 array/tensor view (3,H,W) to decode into."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"))                       # (H, W, 3) uint8
    chw = np.moveaxis(a, 2, 0)
    if out is None:
        return torch.from_numpy(np.ascontiguousarray(chw))
    dst = out.numpy() if isinstance(out, torch.Tensor) else out
    if tuple(dst.shape) != tuple(chw.shape):
        raise ValueError(f"frame {path}: {chw.shape} does not fit the buffer {tuple(dst.shape)}")
    np.copyto(dst, chw)
    return out


def load_clip_video(frame_dir, dataset, video_name, start, end, pad=False, stride=1, source_info=None, out=None):
    """`FrameReaderVideo.load_frames(video_name, start, end, pad, stride, source_info)` (frame.py:558-626) with the
    reference's per-dataset file naming (`frame_locator`)."""
    _, _, _, path_fn = frame_locator(frame_dir, dataset, video_name, source_info)
    return load_clip(path_fn, start, end, stride=stride, pad=pad, out=out)


def load_video(frame_dir, dataset, video_name, num_frames, stride=1, source_info=None, out=None, pool=None):
    """All sampled frames of one video, each decoded ONCE: uint8 (L,3,H,W) with L = ceil(num_frames / stride), row j =
    frame j*stride of the video (`frame_locator` file naming) -- the buffer `TDEEDModel.predict_video` keeps resident, from
    which every overlapping clip window of the evaluation reader (`load_clip_video(..., pad=True)`) is a gather.
    out: optional uint8 (>= L,3,H,W) tensor to decode into; otherwise a new one, page-locked when a GPU runtime is there.
    pool: a DecodePool to decode the frames concurrently.
    Trailing missing files (a video shorter than its label says) become zero frames, as the reference's end padding makes
    them.  A missing file FOLLOWED by an existing one raises FileNotFoundError: the reference's reader appends the frames it
    can read and pads the end (dataset/frame.py:609-626), which silently shifts every later frame of the clip forward;
    that is not reproduced here."""
    _, _, _, path_fn = frame_locator(frame_dir, dataset, video_name, source_info)
    L = (int(num_frames) + stride - 1) // stride
    names = [path_fn(j * stride) for j in range(L)]
    have = [os.path.exists(p) for p in names]
    n_real = L
    while n_real > 0 and not have[n_real - 1]:
        n_real -= 1
    if n_real == 0:
        raise FileNotFoundError(f"video {video_name}: no frame found (looked for {names[0] if names else frame_dir})")
    if not all(have[:n_real]):
        raise FileNotFoundError(f"video {video_name}: {names[have.index(False)]} is missing although later frames exist")
    if out is None:
        first = read_frame(names[0])
        out = torch.zeros((L,) + tuple(first.shape), dtype=torch.uint8)
        if torch.cuda.is_available():
            out = out.pin_memory()
        out[0].copy_(first)
        jobs = [(names[j], out[j]) for j in range(1, n_real)]
    else:
        if out.shape[0] < L:
            raise ValueError(f"the buffer holds {out.shape[0]} frames, the video has {L}")
        if n_real < L:
            out[n_real:L].zero_()
        jobs = [(names[j], out[j]) for j in range(n_real)]
    if pool is not None:
        pool.decode(jobs)
    else:
        for nm, dst in jobs:
            read_frame(nm, out=dst)
    return out[:L]


last_decode_stats = {}      # filled by load_video_device: what its last call did


def _read_file(path):
    with open(path, "rb") as f:
        return f.read()


class DeviceJpegs:
    """A `jpegdev.PackedJpegs` on the device: the tables go up in ONE copy from a page-locked block (segment table, table
    set per frame, the wave tables of every frame chunk, the table sets), the entropy stream in pieces of `piece_bytes`
    as the chunks need it (`stream_through`).  chunks: [(frame_lo, frame_hi, waves tensor | None)]; status: int32 per
    segment row, zero-filled."""

    def __init__(self, packed, device, chunk_frames, piece_bytes=16 << 20, rows=None):
        from . import jpegdev
        self.packed, self.piece = packed, int(piece_bytes)
        n = packed.n_frames
        bounds = [(lo, min(lo + chunk_frames, n)) for lo in range(0, n, chunk_frames)]
        waves = [packed.waves(lo, hi) for lo, hi in bounds]
        parts = [packed.segments.reshape(-1).view(np.uint8), packed.frame_set.view(np.uint8)] + \
                [w.reshape(-1).view(np.uint8) for w in waves] + [packed.table_sets.reshape(-1)]
        if rows is not None:                        # the row of every frame in the output (ops.jpeg_pixels_rows): same copy
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            if rows.shape != (n,):
                raise ValueError(f"DeviceJpegs: {rows.shape} rows for {n} frames")
            parts.append(rows.view(np.uint8))
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += (a.size + 15) & ~15
        host = torch.zeros(max(total, 16), dtype=torch.uint8).pin_memory()
        hv = host.numpy()
        for a, o in zip(parts, offs):
            hv[o:o + a.size] = a
        self._meta_host = host                      # keeps the page-locked block alive until the copy has run
        meta = torch.empty(host.numel(), dtype=torch.uint8, device=device)
        meta.copy_(host, non_blocking=True)

        def view(i, dtype, shape):
            nbytes = parts[i].size
            return meta[offs[i]:offs[i] + nbytes].view(dtype).view(*shape)
        self.segments = view(0, torch.int32, (packed.n_segments, 6))
        self.frame_set = view(1, torch.int32, (n,))
        self.table_sets = view(2 + len(waves), torch.uint8, (packed.n_sets, jpegdev.TABLE_SET_BYTES))
        self.dst_row = view(3 + len(waves), torch.int32, (n,)) if rows is not None else None
        self.chunks = [(lo, hi, view(2 + i, torch.int32, (w.shape[0], 2)) if w.shape[0] else None)
                       for i, ((lo, hi), w) in enumerate(zip(bounds, waves))]
        src = packed.stream if isinstance(packed.stream, torch.Tensor) else torch.from_numpy(packed.stream_np)
        self._src = src
        self.stream = torch.empty(src.numel(), dtype=torch.uint8, device=device)
        self.uploaded = 0
        self.status = torch.zeros(max(packed.n_segments, 1), dtype=torch.int32, device=device)
        self.meta_bytes = int(host.numel())

    def stream_through(self, nbytes):
        """queue the pieces of the entropy stream up to byte `nbytes` that are not queued yet (current stream)"""
        end = min(int(nbytes), self._src.numel())
        while self.uploaded < end:
            hi = min(self.uploaded + self.piece, self._src.numel())
            self.stream[self.uploaded:hi].copy_(self._src[self.uploaded:hi], non_blocking=True)
            self.uploaded = hi

    def need(self, lo, hi):
        """the stream bytes the frames [lo, hi) reach up to"""
        rows = self.packed.rows(lo, hi)
        seg = self.packed.segments
        return int((seg[rows, 3].astype(np.int64) + seg[rows, 4]).max()) + 8 if rows.size else 0


def coeff_chunk(packed, max_coeff_bytes=512 << 20):
    """(int16 values per frame, frames per chunk) of `decode_packed`'s coefficient buffer under max_coeff_bytes"""
    from . import ops
    fc = ops.jpeg_frame_coeffs(packed.width, packed.height, packed.samp)
    return fc, min(max(1, int(max_coeff_bytes) // (2 * fc)), 65535, max(packed.n_frames, 1))


def decode_packed(packed, out, max_coeff_bytes=512 << 20, rows=None, coeff=None):
    """Run the entropy and pixel kernels over a `jpegdev.PackedJpegs` on the current stream: frame j of the pack lands in
    out[j] (device uint8 (>= n_frames,3,H,W)); frames without a table set are left untouched.  The coefficient buffer is
    transient and holds at most max_coeff_bytes (at least one frame).  Returns (DeviceJpegs, number of chunks); nothing is
    synchronised -- the statuses are in `.status` on the device.
    rows: int32 (n_frames,) -- frame j lands in row rows[j] of out instead (a contiguous (...,3,H,W) buffer flattened to
    rows; a negative row stores nothing): the frames of a clip batch (`device_clip_batches`).  coeff: a caller-owned int16
    buffer of at least `coeff_chunk` values to use instead of a transient one."""
    from . import ops
    fc, per = coeff_chunk(packed, max_coeff_bytes)
    dj = DeviceJpegs(packed, out.device, per, rows=rows)
    if coeff is None:
        coeff = torch.empty(per * fc, dtype=torch.int16, device=out.device)
    elif coeff.numel() < per * fc:
        raise ValueError(f"decode_packed: the coefficient buffer holds {coeff.numel()} values, a chunk needs {per * fc}")
    chunks = 0
    for lo, hi, waves in dj.chunks:
        if waves is None:
            continue
        dj.stream_through(dj.need(lo, hi))
        coeff[:(hi - lo) * fc].zero_()
        ops.jpeg_entropy(dj.stream, dj.segments, waves, dj.table_sets, packed.width, packed.height, packed.samp, lo, hi - lo,
                         coeff, dj.status)
        if rows is None:
            ops.jpeg_pixels(coeff, dj.frame_set, dj.table_sets, out, lo, hi - lo, packed.samp)
        else:
            ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out, dj.dst_row, lo, hi - lo, packed.samp)
        chunks += 1
    return dj, chunks


def load_video_device(frame_dir, dataset, video_name, num_frames, stride=1, source_info=None, device="cuda", out=None,
                      stream=None, max_coeff_bytes=512 << 20, pool=None):
    """`load_video` with the decode on the device: the same uint8 (L,3,H,W) frames, bit for bit, as a DEVICE tensor; the
    JPEG files cross the host-device link instead of the decoded frames.  The files are read (through `pool`'s threads
    when a DecodePool is given), parsed and packed on the host (`jpegdev.pack`), uploaded on `stream` (default: the
    current one), and decoded there by csrc/jpeg.hip in chunks of frames whose transient coefficient buffer stays under
    max_coeff_bytes.  One host synchronisation per call, for the per-segment statuses.  Frames outside the decoder's
    subset (`jpegdev.parse`: progressive, CMYK, ...) and frames whose status is non-zero are decoded with `read_frame`
    and copied into their rows: whatever Pillow does with such a file, raising included, is then the behaviour.
    Missing files are treated as by `load_video`.  out: optional device uint8 (>= L,3,H,W) buffer.
    `last_decode_stats` tells what the call did."""
    from . import jpegdev
    _, _, _, path_fn = frame_locator(frame_dir, dataset, video_name, source_info)
    L = (int(num_frames) + stride - 1) // stride
    names = [path_fn(j * stride) for j in range(L)]
    have = [os.path.exists(p) for p in names]
    n_real = L
    while n_real > 0 and not have[n_real - 1]:
        n_real -= 1
    if n_real == 0:
        raise FileNotFoundError(f"video {video_name}: no frame found (looked for {names[0] if names else frame_dir})")
    if not all(have[:n_real]):
        raise FileNotFoundError(f"video {video_name}: {names[have.index(False)]} is missing although later frames exist")
    datas = list(pool.ex.map(_read_file, names[:n_real])) if pool is not None and hasattr(pool, "ex") else \
        [_read_file(p) for p in names[:n_real]]
    packed = jpegdev.pack(datas)
    first = None
    if packed.n_segments == 0:                       # nothing for the device: the geometry comes from Pillow
        first = read_frame(names[0])
        H, W = int(first.shape[1]), int(first.shape[2])
    else:
        H, W = packed.height, packed.width
    dev = torch.device(device)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(st):
        if out is None:
            out = torch.empty((L, 3, H, W), dtype=torch.uint8, device=dev)
        else:
            if not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous():
                raise TypeError("load_video_device: out must be a contiguous uint8 tensor on the device")
            if out.shape[0] < L:
                raise ValueError(f"the buffer holds {out.shape[0]} frames, the video has {L}")
            if tuple(out.shape[1:]) != (3, H, W):
                raise ValueError(f"video {video_name}: frames {(3, H, W)} do not fit the buffer {tuple(out.shape[1:])}")
        if n_real < L:
            out[n_real:L].zero_()
        bad, chunks, uploaded = set(packed.fallback), 0, 0
        if packed.n_segments:
            dj, chunks = decode_packed(packed, out, max_coeff_bytes)
            status = torch.empty(packed.n_segments, dtype=torch.int32).pin_memory()
            status.copy_(dj.status[:packed.n_segments], non_blocking=True)
            st.synchronize()
            uploaded = dj.uploaded + dj.meta_bytes
            bad.update(int(f) for f in np.unique(packed.segments[status.numpy() != 0, 0]))
        for j in sorted(bad):
            fr = first if (j == 0 and first is not None) else read_frame(names[j])
            if tuple(fr.shape) != (3, H, W):
                raise ValueError(f"frame {names[j]}: {tuple(fr.shape)} does not fit the buffer {(3, H, W)}")
            out[j].copy_(fr)
        if bad:
            st.synchronize()
    last_decode_stats.clear()
    last_decode_stats.update(frames=L, device_frames=n_real - len(bad), fallback_frames=len(bad), stream_bytes=int(uploaded),
                             table_sets=packed.n_sets, segments=packed.n_segments, chunks=chunks)
    return out[:L]


def load_clip(frame_path_fn, start, end, stride=1, pad=False, out=None):
    """`FrameReaderVideo.load_frames` (frame.py:558-626) for one clip: frames start, start+stride, ... < end through
    `frame_path_fn(frame_num) -> path`; frames before 0 pad the start with zeros, missing files pad the end (kept only
    when `pad`).  Returns a uint8 (T,3,H,W) tensor (a view of `out` when given), or -1 when no frame exists."""
    nums = list(range(start, end, stride))
    n_pad_start = sum(1 for n in nums if n < 0)
    todo = [n for n in nums if n >= 0]
    frames = []
    n_pad_end = 0
    for j, n in enumerate(todo):
        p = frame_path_fn(n)
        if not os.path.exists(p):
            n_pad_end += 1
            continue
        dst = None if out is None else out[n_pad_start + len(frames)]
        frames.append(read_frame(p, out=dst))
    if not frames:
        return -1
    T_real = len(frames)
    if out is not None:
        if n_pad_start:
            out[:n_pad_start].zero_()
        tail = n_pad_start + T_real
        if pad and n_pad_end:
            out[tail:tail + n_pad_end].zero_()
            tail += n_pad_end
        return out[:tail]
    clip = torch.stack(frames, 0)
    if n_pad_start > 0 or (pad and n_pad_end > 0):
        clip = torch.nn.functional.pad(clip, (0, 0, 0, 0, 0, 0, n_pad_start, n_pad_end if pad else 0))
    return clip


def frame_locator(frame_dir, dataset, video_name, source_info=None):
    """Where the frames of one video live, per dataset, as both of the reference's readers lay it out
    (frame.py:274-292 / 563-578 for the directory and the first frame number, 303-338 / 586-609 for the file names).
    Returns (base_path, frame0, ndigits, path_fn): frame index n of the video (0 = its first frame) is the file
    path_fn(n); ndigits is the zero-padded width of FineDiving's file names, -1 for the 'frame<N>.jpg' datasets."""
    ndigits = -1
    frame0 = 0
    if dataset == "finediving":
        base = os.path.join(frame_dir, video_name.replace("__", "/"))
        first = sorted(os.listdir(base))[0]
        ndigits, frame0 = len(first[:-4]), int(first[:-4])
        return base, frame0, ndigits, (lambda n: os.path.join(base, str(frame0 + n).zfill(ndigits) + ".jpg"))
    if dataset == "tennis":
        parts = video_name.split("_")
        frame0 = int(parts[-2])
        base = os.path.join(frame_dir, "_".join(parts[:-2]))
    elif dataset == "finegym":
        frame0 = source_info["start_frame"] - source_info["pad"][0]
        base = os.path.join(frame_dir, video_name.split("_")[0])
    elif dataset in ("soccernetball", "soccernet", "fs_comp", "fs_perf"):
        base = os.path.join(frame_dir, video_name)
    else:
        raise ValueError(f"unknown dataset {dataset!r}")
    return base, frame0, ndigits, (lambda n: os.path.join(base, "frame" + str(frame0 + n) + ".jpg"))


def load_paths(frame_dir, dataset, video_name, start, end, stride=1, source_info=None):
    """`FrameReader.load_paths` (frame.py:273-351), the training reader's clip descriptor:
    [base_path, first existing frame NUMBER (file numbering, -1 if none), pad_start, pad_end, ndigits, length] with
    length = (end - start) // stride.  Frames before 0 count as start padding; from the first missing file on every
    remaining step counts as end padding (the reference stops looking: a later file that exists is not read)."""
    base, frame0, ndigits, path_fn = frame_locator(frame_dir, dataset, video_name, source_info)
    found_start, pad_start, pad_end = -1, 0, 0
    for n in range(start, end, stride):
        if n < 0:
            pad_start += 1
            continue
        if pad_end > 0:
            pad_end += 1
            continue
        if os.path.exists(path_fn(n)):
            if found_start == -1:
                found_start = frame0 + n
        else:
            pad_end += 1
    return [base, found_start, pad_start, pad_end, ndigits, (end - start) // stride]


def load_frames(paths, pad=False, stride=1, out=None, pool=None):
    """`FrameReader.load_frames` (frame.py:353-382): the `length - pad_start - pad_end` frames numbered paths[1],
    paths[1] + stride, ... decoded into a uint8 (T,3,H,W) clip, zero frames in front for pad_start, behind for pad_end when
    `pad`.  out: optional uint8 buffer (>= T frames: a pinned ring slot) to decode into; pool: a DecodePool to decode the
    frames concurrently."""
    base, start, pad_start, pad_end, ndigits, length = paths
    n_real = length - pad_start - pad_end
    if ndigits == -1:
        names = [os.path.join(base, "frame") + str(start + j * stride) + ".jpg" for j in range(n_real)]
    else:
        names = [base + "/" + str(start + j * stride).zfill(ndigits) + ".jpg" for j in range(n_real)]
    return _assemble(names, pad_start, pad_end if pad else 0, out, pool)


def _assemble(names, n_pad_start, n_pad_end, out, pool):
    """Decode `names` into [zeros * n_pad_start | frames | zeros * n_pad_end]."""
    if out is None:
        first = read_frame(names[0])
        total = n_pad_start + len(names) + n_pad_end
        out = torch.zeros((total,) + tuple(first.shape), dtype=torch.uint8)
        out[n_pad_start].copy_(first)
        rest = [(nm, out[n_pad_start + 1 + i]) for i, nm in enumerate(names[1:])]
    else:
        total = n_pad_start + len(names) + n_pad_end
        if out.shape[0] < total:
            raise ValueError(f"staging buffer holds {out.shape[0]} frames, the clip needs {total}")
        if n_pad_start:
            out[:n_pad_start].zero_()
        if n_pad_end:
            out[n_pad_start + len(names):total].zero_()
        rest = [(nm, out[n_pad_start + i]) for i, nm in enumerate(names)]
    if pool is not None:
        pool.decode(rest)
    else:
        for nm, dst in rest:
            read_frame(nm, out=dst)
    return out[:total]


class DecodePool:
    """Decode threads of the input pipeline (the reference uses 4-8 DataLoader worker PROCESSES, train_tdeed.py:131-139;
    Pillow releases the GIL inside libjpeg, so threads scale and decode straight into pinned ring slots without a copy
    between processes).  decode([(path, uint8 (3,H,W) destination), ...]) returns when all frames are in place."""

    def __init__(self, threads=None):
        from concurrent.futures import ThreadPoolExecutor
        self.threads = threads if threads else min(32, (os.cpu_count() or 8))
        self.ex = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="tdeed-decode")

    def decode(self, jobs):
        futs = [self.ex.submit(read_frame, nm, dst) for nm, dst in jobs]
        for f in futs:
            f.result()

    def submit(self, jobs):
        """Asynchronous form: returns the futures (wait with .result())."""
        return [self.ex.submit(read_frame, nm, dst) for nm, dst in jobs]

    def close(self):
        self.ex.shutdown(wait=True)


class _Ack:
    """Future of one decode job of a ProcessDecodePool."""
    __slots__ = ("ev", "err", "worker")

    def __init__(self, worker=-1):
        import threading
        self.ev, self.err, self.worker = threading.Event(), None, worker

    def result(self, timeout=120.0):
        if not self.ev.wait(timeout):
            raise TimeoutError("decode worker did not answer")
        if self.err:
            raise RuntimeError(self.err)


class ProcessDecodePool:
    """Decode worker PROCESSES (what the reference's DataLoader workers are, train_tdeed.py:131-139): JPEG decode in Python
    scales to ~8 threads (DecodePool: Pillow releases the GIL only inside libjpeg), processes scale with the cores.  The
    workers (`_decode_worker.py`: numpy + Pillow, no torch) write straight into staging slots that live in POSIX shared
    memory and are page-locked in this process (`make_slots`), so a decoded batch is uploaded without a copy between
    processes.  Same interface as DecodePool."""

    def __init__(self, procs=None):
        import subprocess
        import sys
        import threading
        self.procs = procs if procs else min(32, (os.cpu_count() or 8))
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        boot = f"import sys; sys.path.insert(0, {root!r}); import tdeed_amd._decode_worker as w; w.main()"
        self._w, self._pending, self._lock, self._next, self._rr = [], {}, threading.Lock(), 0, 0
        self._shms, self._slots, self._slot_cache = [], [], {}
        self._alive = []
        self._closing = False
        # one decode thread per worker: numpy's BLAS / OpenMP pools otherwise start a thread per host core in EVERY worker
        # (128 workers on a 256-thread host = 32 k threads: the decode rate fell from 412 to 32 clips/s)
        wenv = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1", NUMEXPR_NUM_THREADS="1")
        for wi in range(self.procs):
            pr = subprocess.Popen([sys.executable, "-c", boot], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1,
                                  env=wenv)
            self._w.append(pr)
            self._alive.append(True)
            th = threading.Thread(target=self._reader, args=(pr, wi), daemon=True)
            th.start()

    def _reader(self, pr, wi):
        try:
            for line in pr.stdout:
                parts = line.rstrip("\n").split(" ", 2)
                try:
                    jid = int(parts[0])
                    status = parts[1]
                except (ValueError, IndexError):
                    continue                    # not a protocol line (a library's warning on the worker's stdout): skip it
                with self._lock:
                    ack = self._pending.pop(jid, None)
                if ack is not None:
                    if status != "ok":
                        ack.err = parts[2] if len(parts) > 2 else "decode worker error"
                    ack.ev.set()
        finally:
            # EOF on the worker's pipe (or this thread dying): the worker exited (crash, OOM kill, or close()).  Fail the
            # jobs it still owed right away instead of letting every result() run into its timeout, and take it out of
            # the rotation.
            try:
                rc = pr.wait(timeout=2.0)
            except Exception:           # noqa: BLE001  (still running: the pipe closed first)
                rc = pr.poll()
            with self._lock:
                self._alive[wi] = False
                owed = [j for j, a in self._pending.items() if a.worker == wi]
                for j in owed:
                    ack = self._pending.pop(j)
                    ack.err = f"decode worker {wi} exited (rc={rc}) with the job outstanding"
                    ack.ev.set()

    def _pick_worker(self):
        """next live worker of the rotation (caller holds the lock)"""
        for _ in range(self.procs):
            wi = self._rr % self.procs
            self._rr += 1
            if self._alive[wi]:
                return wi
        raise RuntimeError("ProcessDecodePool: no live decode worker left")

    def _send(self, wi, line, ack, jid):
        try:
            self._w[wi].stdin.write(line)
        except (BrokenPipeError, ValueError, OSError) as e:
            with self._lock:
                self._alive[wi] = False
                self._pending.pop(jid, None)
            ack.err = f"decode worker {wi} is gone ({type(e).__name__})"
            ack.ev.set()

    def make_slots(self, depth, shape):
        """`depth` uint8 staging tensors of `shape` in shared memory, page-locked when a GPU runtime is there.  Cached per
        (depth, shape): a second loader over the same pool reuses the blocks instead of piling up shared memory."""
        from multiprocessing import shared_memory
        key = (int(depth), tuple(int(v) for v in shape))
        if key in self._slot_cache:
            return self._slot_cache[key][0]
        n = int(np.prod(shape))
        out = []
        for _ in range(depth):
            shm = shared_memory.SharedMemory(create=True, size=n)
            t = torch.frombuffer(shm.buf, dtype=torch.uint8, count=n).view(*shape)
            if torch.cuda.is_available():
                rc = torch.cuda.cudart().cudaHostRegister(t.data_ptr(), n, 0)
                if int(rc) != 0:
                    raise RuntimeError(f"cudaHostRegister failed: {rc}")
            self._shms.append((shm, t.data_ptr(), n, torch.cuda.is_available()))
            self._slots.append(t)
            out.append(t)
        # the upload-event holders that guard a slot's reuse live WITH the slots: a second loader over the same pool and
        # shape (train + val, or a new epoch while an upload from the old generator is still in flight) waits on the same
        # events before it decodes into a slot
        from types import SimpleNamespace
        self._slot_cache[key] = (out, [SimpleNamespace(event=None) for _ in range(depth)])
        return out

    def slot_holders(self, depth, shape):
        """the per-slot upload-event holders of make_slots(depth, shape) (shared by every loader that uses those slots)"""
        self.make_slots(depth, shape)
        return self._slot_cache[(int(depth), tuple(int(v) for v in shape))][1]

    def _locate(self, dst):
        p = dst.data_ptr()
        for shm, base, n, _ in self._shms:
            if base <= p < base + n:
                return shm.name, p - base
        raise ValueError("ProcessDecodePool: destination is not inside a slot from make_slots()")

    def submit(self, jobs):
        acks = []
        for path, dst in jobs:
            name, off = self._locate(dst)
            with self._lock:
                wi = self._pick_worker()
                ack = _Ack(wi)
                jid = self._next
                self._next += 1
                self._pending[jid] = ack
            self._send(wi, f"{jid} {name} {off} {dst.shape[-2]} {dst.shape[-1]} {path}\n", ack, jid)
            acks.append(ack)
        self._flush(range(self.procs))
        return acks

    def _flush(self, workers):
        for wi in workers:
            if self._alive[wi]:
                try:
                    self._w[wi].stdin.flush()
                except (BrokenPipeError, ValueError, OSError):
                    pass                # the reader thread fails the worker's jobs at EOF

    def submit_rows(self, paths, dst, chunk=25):
        """Consecutive frames: paths[i] -> dst[i] (dst: a contiguous (n,3,H,W) view inside a slot), `chunk` frames per job
        line -- the parent's per-frame work (formatting, pipe write, acknowledgement) otherwise caps the pool near 30 000
        frames/s however many workers there are."""
        import json
        if not dst.is_contiguous():
            raise ValueError("submit_rows: the destination rows must be contiguous")
        name, off = self._locate(dst)
        H, W = dst.shape[-2], dst.shape[-1]
        acks, touched = [], set()
        for lo in range(0, len(paths), chunk):
            with self._lock:
                wi = self._pick_worker()
                ack = _Ack(wi)
                jid = self._next
                self._next += 1
                self._pending[jid] = ack
            self._send(wi, "J " + json.dumps(dict(id=jid, shm=name, off=off + lo * 3 * H * W, H=H, W=W,
                                                  paths=list(paths[lo:lo + chunk]))) + "\n", ack, jid)
            touched.add(wi)
            acks.append(ack)
        self._flush(touched)
        return acks

    def decode(self, jobs):
        for a in self.submit(jobs):
            a.result()

    def close(self):
        for pr in self._w:
            try:
                pr.stdin.write("quit\n")
                pr.stdin.flush()
                pr.stdin.close()
            except Exception:       # noqa: BLE001
                pass
        for pr in self._w:
            try:
                pr.wait(timeout=10)
            except Exception:       # noqa: BLE001
                pr.kill()
        self._w = []
        self._slots = []
        self._slot_cache = {}
        for shm, ptr_, n, pinned in self._shms:
            try:
                if pinned:
                    torch.cuda.cudart().cudaHostUnregister(ptr_)
            except Exception:       # noqa: BLE001
                pass
            try:
                shm.close()
            except BufferError:
                pass                # a tensor still views the block: the mapping goes with the process
            try:
                shm.unlink()
            except FileNotFoundError:
                pass
        self._shms = []

    def __del__(self):
        try:
            if self._w:
                self.close()
        except Exception:           # noqa: BLE001
            pass


def clip_batches(clips, batch_size, frame_shape, clip_len, pool=None, depth=3, pad=True):
    """Batches of decoded clips in pinned staging slots, ready for `prefetch`: `clips` is a list of descriptors
    dict(paths=<load_paths result>, stride=..) (+ any label entries, passed through per batch as lists); every batch dict
    holds 'frame' = a PINNED uint8 (B,T,3,H,W) tensor filled by `pool` (all frames of the batch are decode jobs of one
    pool call, so B * T JPEGs decode concurrently).  The slots rotate: a batch must be consumed (copied to the device)
    before `depth` further batches are produced.  `prefetch` uploads a pinned batch straight from its slot, asynchronously:
    it leaves the arrival event in the batch's `_src` holder, and a slot is not decoded into again before that event has
    completed (a consumer that never syncs -- graph replays -- would otherwise see frames overwritten mid-copy).  Rows of
    a clip behind its real frames are always zeroed (pad=False only drops the END padding from the clip's length in the
    reference, dataset/frame.py:355-382; a fixed-length slot must not show an earlier batch's frames there)."""
    own = pool is None
    pool = pool if pool is not None else DecodePool()
    shape = (batch_size, clip_len) + tuple(frame_shape)
    if hasattr(pool, "make_slots"):          # worker processes decode into shared, page-locked slots
        slots = pool.make_slots(depth, shape)
        holders = pool.slot_holders(depth, shape) if hasattr(pool, "slot_holders") else None
    else:
        holders = None
        # (page-locked when a GPU runtime is there, like make_slots: the decode logic itself also runs on a GPU-less host)
        slots = [torch.zeros(shape, dtype=torch.uint8) for _ in range(depth)]
        if torch.cuda.is_available():
            slots = [t_.pin_memory() for t_ in slots]
    if holders is None:
        holders = [SimpleNamespace(event=None) for _ in range(depth)]
    try:
        for bi, lo in enumerate(range(0, len(clips) - batch_size + 1, batch_size)):
            slot = slots[bi % depth]
            hold = holders[bi % depth]
            if hold.event is not None:       # the upload that last read this slot (prefetch) must have left it
                hold.event.synchronize()
                hold.event = None
            group = clips[lo:lo + batch_size]
            futs = []
            for i, c in enumerate(group):
                base, start, pad_start, pad_end, ndigits, length = c["paths"]
                stride = c.get("stride", 1)
                n_real = length - pad_start - pad_end
                dst = slot[i]
                if pad_start:
                    dst[:pad_start].zero_()
                if pad_start + n_real < clip_len:
                    dst[pad_start + n_real:].zero_()
                names = []
                for j in range(n_real):
                    num = start + j * stride
                    names.append((os.path.join(base, "frame") + str(num) + ".jpg") if ndigits == -1
                                 else (base + "/" + str(num).zfill(ndigits) + ".jpg"))
                if hasattr(pool, "submit_rows"):
                    futs += pool.submit_rows(names, dst[pad_start:pad_start + n_real])
                else:
                    futs += pool.submit([(nm, dst[pad_start + j]) for j, nm in enumerate(names)])
            for f in futs:
                f.result()
            extra = {k: [c[k] for c in group] for k in group[0] if k not in ("paths", "stride")}
            yield dict(frame=slot, _src=hold, **extra)
    finally:
        if own:
            pool.close()


def _clip_names(paths, stride):
    base, start, pad_start, pad_end, ndigits, length = paths
    nums = [start + j * stride for j in range(length - pad_start - pad_end)]
    return [(os.path.join(base, "frame") + str(n) + ".jpg") if ndigits == -1 else (base + "/" + str(n).zfill(ndigits) + ".jpg")
            for n in nums]


def clip_batch_rows(group, clip_len):
    """The row table of one batch of `device_clip_batches` (pure; no file is touched).  group: B clip descriptors.  The
    batch slot is (n,B,T,3,H,W) with n = 2 when the descriptors carry 'paths2' (the mixup twin: rows B*T .. 2*B*T - 1),
    flattened to rows: real frame j of clip i sits in row i*T + pad_start + j.
    -> (names, rows, zero): the file of every real frame, clip by clip and the twins behind; int32 row per file; the row
    ranges [(lo, hi), ...] that hold no frame (start and end padding of every clip), which a batch shows as zeros."""
    B, T = len(group), int(clip_len)
    names, rows, zero = [], [], []
    for half, (kp, ks) in enumerate((("paths", "stride"), ("paths2", "stride2"))):
        if half and "paths2" not in group[0]:
            break
        for i, c in enumerate(group):
            _, _, pad_start, pad_end, _, length = c[kp]
            n_real = length - pad_start - pad_end
            if pad_start < 0 or n_real < 0 or pad_start + n_real > T:
                raise ValueError(f"clip {i}: {pad_start} + {n_real} frames do not fit a clip of {T}")
            first = (half * B + i) * T
            names += _clip_names(c[kp], c.get(ks, 1))
            rows += range(first + pad_start, first + pad_start + n_real)
            if pad_start:
                zero.append((first, first + pad_start))
            if pad_start + n_real < T:
                zero.append((first + pad_start + n_real, first + T))
    return names, np.asarray(rows, dtype=np.int32), zero


def _read_file_stat(path):
    with open(path, "rb") as f:
        st = os.fstat(f.fileno())
        return f.read(), st.st_size, st.st_mtime_ns


class _DeviceSlots:
    """The `depth` device batch slots of `device_clip_batches` and their release events (the `_slot` holder of its
    batches: `feeder.done` calls release)."""

    def __init__(self, depth, shape, device):
        self.buf = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(depth)]
        self.consumed = [None] * depth
        self.out = [False] * depth

    def release(self, j, stream=None):
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        self.consumed[j] = ev
        self.out[j] = False


def device_clip_batches(clips, batch_size, frame_shape, clip_len, device="cuda", pool=None, depth=3, pad=True,
                        max_coeff_bytes=512 << 20, parse_cache=None):
    """`clip_batches` with the decode on the device: the same descriptors, the same batches bit for bit, but 'frame' is a
    DEVICE uint8 (B,T,3,H,W) tensor decoded by csrc/jpeg.hip from the JPEG files, which cross the host-device link
    instead of the decoded frames.  A descriptor may carry 'paths2' / 'stride2' for the mixup twin: the batch then holds
    'frame2' as well (both halves of one (2,B,T,3,H,W) slot, one pack, one decode).  Every batch brings the hand-over of
    `prefetch`'s device batches ('_slot'): bracket its use with `wait(batch)` / `done(batch)`, or iterate through
    `prefetch` (`TDEEDModel.epoch()` does); a slot is decoded into again only after its batch was released.

    All device work runs on one decode stream of the feed: the upload of the packed entropy stream and tables
    (`jpegdev.pack_frames` over the batch's files, `DeviceJpegs`), the kernels (`decode_packed` with the row table of
    `clip_batch_rows`, one persistent coefficient buffer chunked under max_coeff_bytes), the zeros of the padding rows
    (those rows only, every batch) and the copies of host-decoded frames.  The host never waits for the device as a
    whole, and the consumer's stream is never synchronised: the statuses of batch b are copied to page-locked memory
    behind an event, batch b + 1 is queued (when a slot is free) before the host waits for that event, and only then are
    b's statuses read.  Frames outside the decoder's subset (`packed.fallback`) and frames whose status is non-zero are
    decoded with `read_frame` and copied into their rows on the decode stream -- whatever Pillow does with such a file,
    raising included, is then the behaviour; a frame of another size raises ValueError.
    pool: a DecodePool whose threads read the files.  parse_cache: a `jpegdev.ParseCache` (default: a new one for this
    call) -- keep one across epochs and the files are parsed once.  pad: as for `clip_batches`, the rows behind a clip's
    real frames are zero either way.  The tail of `clips` that does not fill a batch is dropped.  `last_decode_stats`
    holds the numbers of the batch yielded last."""
    from collections import deque
    from . import jpegdev
    from .streams import new_stream
    B, T = int(batch_size), int(clip_len)
    C, H, W = (int(v) for v in frame_shape)
    if C != 3:
        raise ValueError(f"device_clip_batches: frames are (3,H,W), not {tuple(frame_shape)}")
    dev = torch.device(device)
    cache = parse_cache if parse_cache is not None else jpegdev.ParseCache()
    groups = [clips[lo:lo + B] for lo in range(0, len(clips) - B + 1, B)]
    if not groups:
        return
    twin = "paths2" in groups[0][0]
    halves = 2 if twin else 1
    n_rows = halves * B * T
    dec = new_stream(dev)
    with torch.cuda.stream(dec):
        slots = _DeviceSlots(depth, (halves, B, T, 3, H, W), dev)
    host_status = [None] * depth                    # page-locked int32, grown as a batch needs
    coeff = [None]
    reader = pool.ex.map if pool is not None and hasattr(pool, "ex") else map

    def fallback_copy(rows_view, names, rows, f):
        fr = read_frame(names[f])
        if tuple(fr.shape) != (3, H, W):
            raise ValueError(f"frame {names[f]}: {tuple(fr.shape)} does not fit the buffer {(3, H, W)}")
        rows_view[int(rows[f])].copy_(fr)

    def enqueue(bi):
        j = bi % depth
        group = groups[bi]
        if any(("paths2" in c) != twin for c in group):
            raise ValueError("device_clip_batches: either every descriptor has 'paths2' or none")
        names, rows, zero = clip_batch_rows(group, T)
        files = list(reader(_read_file_stat, names))
        infos = [cache.lookup(nm, size, mtime, data) for nm, (data, size, mtime) in zip(names, files)]
        packed = jpegdev.pack_frames([f[0] for f in files], infos)
        if packed.n_segments and (packed.height, packed.width) != (H, W):
            raise ValueError(f"batch {bi}: frames {(3, packed.height, packed.width)} do not fit the buffer {(3, H, W)}")
        slot = slots.buf[j]
        rows_view = slot.view(n_rows, 3, H, W)
        st = SimpleNamespace(bi=bi, j=j, names=names, rows=rows, packed=packed, rows_view=rows_view, dj=None, event=None,
                             status=None, chunks=0, late=[])
        with torch.cuda.stream(dec):
            if slots.consumed[j] is not None:       # the consumer's last use of the slot, on whichever stream it ran
                dec.wait_event(slots.consumed[j])
                slots.consumed[j] = None
            for lo, hi in zero:
                rows_view[lo:hi].zero_()
            if packed.n_segments:
                fc, per = coeff_chunk(packed, max_coeff_bytes)
                if coeff[0] is None or coeff[0].numel() < per * fc:
                    coeff[0] = torch.empty(per * fc, dtype=torch.int16, device=dev)
                st.dj, st.chunks = decode_packed(packed, slot, max_coeff_bytes, rows=rows, coeff=coeff[0])
                if host_status[j] is None or host_status[j].numel() < packed.n_segments:
                    host_status[j] = torch.empty(packed.n_segments, dtype=torch.int32).pin_memory()
                st.status = host_status[j][:packed.n_segments]
                st.status.copy_(st.dj.status[:packed.n_segments], non_blocking=True)
            for f in packed.fallback:
                fallback_copy(rows_view, names, rows, f)
            st.event = torch.cuda.Event()
            st.event.record(dec)
        slots.out[j] = True
        return st

    def finish(st):
        st.event.synchronize()                      # this batch's decode; the next batch is already queued behind it
        packed = st.packed
        if st.status is not None:
            st.late = sorted(int(f) for f in np.unique(packed.segments[st.status.numpy() != 0, 0]))
        with torch.cuda.stream(dec):
            for f in st.late:
                fallback_copy(st.rows_view, st.names, st.rows, f)
            ready = torch.cuda.Event()
            ready.record(dec)
        n_bad = len(packed.fallback) + len(st.late)
        last_decode_stats.clear()
        last_decode_stats.update(frames=n_rows, device_frames=len(st.names) - n_bad, fallback_frames=n_bad,
                                 stream_bytes=int(st.dj.uploaded + st.dj.meta_bytes) if st.dj is not None else 0,
                                 table_sets=packed.n_sets, segments=packed.n_segments, chunks=st.chunks,
                                 status_frames=list(st.late))
        group = groups[st.bi]
        extra = {k: [c[k] for c in group] for k in group[0] if k not in ("paths", "stride", "paths2", "stride2")}
        batch = dict(frame=slots.buf[st.j][0], _slot=(slots, st.j, ready), **extra)
        if twin:
            batch["frame2"] = slots.buf[st.j][1]
        return batch

    queued, nxt = deque(), 0
    while True:
        # run one batch ahead of the one handed out, as far as released slots allow
        while nxt < len(groups) and len(queued) < 2 and not slots.out[nxt % depth]:
            queued.append(enqueue(nxt))
            nxt += 1
        if not queued:
            if nxt < len(groups):
                raise RuntimeError(f"device_clip_batches: the batch handed out {depth} batches ago was never released "
                                   "(feeder.done / feeder.prefetch); its slot cannot be reused")
            return
        yield finish(queued.popleft())


class PinnedRing:
    """`depth` pinned host slots + device buffers of one batch geometry (B,T,3,H,W) uint8 and a copy stream."""

    def __init__(self, shape, device="cuda", depth=3):
        self.shape, self.device, self.depth = tuple(shape), device, depth
        self.host = [torch.empty(self.shape, dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.dev = [torch.empty(self.shape, dtype=torch.uint8, device=device) for _ in range(depth)]
        self.copied = [None] * depth            # event: H2D copy of the slot finished
        self.consumed = [None] * depth          # event: the consumer is done with the device buffer
        from .streams import new_stream
        self.stream = new_stream(device)                  # never the consumer's own stream (torch's pool wraps around)
        self.i = 0

    def next_slot(self):
        """Slot to fill next; blocks (host) only if its previous copy has not left the pinned buffer yet."""
        j = self.i % self.depth
        self.i += 1
        if self.copied[j] is not None:
            self.copied[j].synchronize()
        return j

    def upload(self, j, src=None):
        """Async H2D of slot j on the copy stream (src: an already pinned tensor to copy from instead of the slot's own
        host buffer).  Returns (device tensor, arrival event)."""
        host = self.host[j] if src is None else src
        with torch.cuda.stream(self.stream):
            if self.consumed[j] is not None:
                self.stream.wait_event(self.consumed[j])        # do not overwrite a buffer the forward still reads
            self.dev[j].copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.copied[j] = ev
        return self.dev[j], ev

    def release(self, j, stream=None):
        """The consumer's stream no longer needs slot j after everything queued on it so far."""
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream())
        self.consumed[j] = ev


class PackedUpload:
    """The frames of several videos in ONE device buffer `video` (sum L,3,H,W), filled in chunks of `chunk_bytes` on the
    copy stream `stream` (a chunk may span videos), one arrival event per chunk: the resident buffer of
    `TDEEDModel.predict_video` / `predict_video_group` and of `trainclips.ResidentClips`.  srcs: contiguous uint8
    (L_v,3,H,W) tensors of one frame geometry -- host, pinned or device.  `through(c)` queues the chunks up to c;
    pinned and device sources copy asynchronously, so all of them may be queued at once (`asynchronous`), while a copy
    from pageable memory stages on the host inside the call: a consumer keeps such an upload one chunk ahead."""

    def __init__(self, srcs, device, stream, chunk_bytes):
        self.srcs, self.stream = srcs, stream
        lengths = [int(fr.shape[0]) for fr in srcs]
        L = sum(lengths)
        self.frame_bytes = fb = int(srcs[0][0].numel())
        self.video = torch.empty((L,) + tuple(srcs[0].shape[1:]), dtype=torch.uint8, device=device)
        self.per = max(1, int(chunk_bytes) // fb)
        self.bounds = [(lo, min(lo + self.per, L)) for lo in range(0, L, self.per)]
        self.offs = np.concatenate([[0], np.cumsum(lengths)]).tolist()
        self.arrived = []
        self.h2d = 0                              # bytes that crossed the host-device link so far
        self.asynchronous = all(fr.is_cuda or fr.is_pinned() for fr in srcs)

    def through(self, c):
        """Queue every chunk up to and including c (clamped to the last) that is not queued yet."""
        with torch.cuda.stream(self.stream):
            while len(self.arrived) <= min(c, len(self.bounds) - 1):
                lo, hi = self.bounds[len(self.arrived)]
                for v, fr in enumerate(self.srcs):
                    a, b = max(lo, self.offs[v]), min(hi, self.offs[v + 1])
                    if a < b:
                        self.video[a:b].copy_(fr[a - self.offs[v]:b - self.offs[v]], non_blocking=True)
                        self.h2d += 0 if fr.is_cuda else (b - a) * self.frame_bytes
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self.arrived.append(ev)

    def all(self):
        """Queue everything; -> the event after which the whole buffer is resident."""
        self.through(len(self.bounds) - 1)
        return self.arrived[-1]


class RingUpload:
    """PackedUpload for frames that do not fit the device budget: the same chunks of the same packed buffer, uploaded in the
    same order on the copy stream with the same `through(c)` / `arrived[c]` protocol and `h2d` count, but into a RING
    `video` of (ring_chunks * per,3,H,W) rows.  Chunk c lives in slot c % ring_chunks, so packed frame p sits in row
    p % (ring_chunks * per) -- what ops.clip_gather_ring reads.  A chunk that spans videos is written piece by piece.
    last_reader: `evalutil.ring_plan`'s, per chunk the last batch that reads it.  The consumer calls `release(b, stream)`
    after batch b's forward has been queued on its stream; before chunk c >= ring_chunks is copied over chunk c -
    ring_chunks, the copy stream waits for the release of every batch up to last_reader[c - ring_chunks] -- the latest
    event of each stream the batches ran on.  ring_plan guarantees that those batches have been released when the host
    queues the copy, so nothing here synchronises the host.  Copies are queued only as far as `through` asks, never all
    at once (`asynchronous` tells whether a call returns before its copies have run, as for PackedUpload)."""

    def __init__(self, srcs, device, stream, chunk_bytes, ring_chunks, last_reader):
        self.srcs, self.stream = srcs, stream
        lengths = [int(fr.shape[0]) for fr in srcs]
        L = sum(lengths)
        self.frame_bytes = fb = int(srcs[0][0].numel())
        self.per = max(1, int(chunk_bytes) // fb)
        self.ring_chunks = int(ring_chunks)
        if self.ring_chunks < 1:
            raise ValueError("RingUpload: a ring needs at least one chunk")
        self.ring_frames = self.ring_chunks * self.per
        self.video = torch.empty((self.ring_frames,) + tuple(srcs[0].shape[1:]), dtype=torch.uint8, device=device)
        self.bounds = [(lo, min(lo + self.per, L)) for lo in range(0, L, self.per)]
        self.last_reader = [int(b) for b in last_reader]
        if len(self.last_reader) != len(self.bounds):
            raise ValueError(f"RingUpload: last_reader for {len(self.last_reader)} chunks, the frames make {len(self.bounds)}")
        self.offs = np.concatenate([[0], np.cumsum(lengths)]).tolist()
        self.arrived = []
        self.released = []                        # per batch (stream, event)
        self.h2d = 0                              # bytes that crossed the host-device link so far
        self.asynchronous = all(fr.is_cuda or fr.is_pinned() for fr in srcs)

    def release(self, b, stream):
        """Batch b (they come in order) no longer reads the ring after everything queued on `stream` so far."""
        if b != len(self.released):
            raise ValueError(f"RingUpload: batch {b} released, {len(self.released)} is next")
        ev = torch.cuda.Event()
        ev.record(stream)
        self.released.append((stream, ev))

    def _wait_readers(self, upto):
        """the copy stream waits for every released batch <= upto: the latest event of each stream among them"""
        if upto >= len(self.released):
            raise RuntimeError(f"RingUpload: batch {upto} still reads the slot to overwrite and has not been released "
                               f"({len(self.released)} batches have): the ring is too small for this order (evalutil.ring_plan)")
        streams, seen = {id(s) for s, _ in self.released[:upto + 1]}, set()
        for s, ev in reversed(self.released[:upto + 1]):
            if id(s) not in seen:
                seen.add(id(s))
                self.stream.wait_event(ev)
                if len(seen) == len(streams):
                    break

    def through(self, c):
        """Queue every chunk up to and including c (clamped to the last) that is not queued yet."""
        with torch.cuda.stream(self.stream):
            while len(self.arrived) <= min(c, len(self.bounds) - 1):
                ci = len(self.arrived)
                lo, hi = self.bounds[ci]
                if ci >= self.ring_chunks and self.last_reader[ci - self.ring_chunks] >= 0:
                    self._wait_readers(self.last_reader[ci - self.ring_chunks])
                row = (ci % self.ring_chunks) * self.per - lo          # packed frame p -> ring row p + row
                for v, fr in enumerate(self.srcs):
                    a, b = max(lo, self.offs[v]), min(hi, self.offs[v + 1])
                    if a < b:
                        self.video[a + row:b + row].copy_(fr[a - self.offs[v]:b - self.offs[v]], non_blocking=True)
                        self.h2d += 0 if fr.is_cuda else (b - a) * self.frame_bytes
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self.arrived.append(ev)


def wait(batch, stream=None):
    """Explicit mode of `prefetch`: make `stream` (default: the current one) wait for the batch's frames to have arrived."""
    slot = batch.get("_slot")
    if slot is not None:
        (stream if stream is not None else torch.cuda.current_stream()).wait_event(slot[2])


def done(batch, stream=None):
    """Explicit mode of `prefetch`: everything queued on `stream` so far was the last use of the batch's device frames."""
    slot = batch.pop("_slot", None)
    if slot is not None:
        slot[0].release(slot[1], stream)


def prefetch(loader, device="cuda", key="frame", depth=3, auto=True):
    """Iterate `loader` (batch dicts) one batch ahead: `batch[key]` (uint8 host tensor) is staged in a pinned ring and
    copied to the device on a copy stream while the previous batch is processed; the yielded dict holds the device tensor.
    Tensors that are already pinned are copied without the staging memcpy; device tensors pass through.
    auto=True: the stream that is current when the batch is yielded waits for the arrival, and the buffer is released on
    that same stream when the next batch is requested (single-stream consumers).  auto=False: the consumer brackets its use
    with `wait(batch)` / `done(batch)` inside its own stream context (consumers that alternate streams)."""
    ring = None
    pending = None

    def start(batch):
        nonlocal ring
        if "_slot" in batch:                 # a device-side loader (trainclips.ResidentClips): its batch is already on the
            return dict(batch)               # device and brings its own arrival event / release holder
        fr = batch[key]
        if not isinstance(fr, torch.Tensor):
            fr = torch.as_tensor(np.asarray(fr))
        if fr.is_cuda:
            return dict(batch)
        if fr.dtype != torch.uint8:
            fr = fr.round().clamp_(0, 255).to(torch.uint8)
        if ring is None or ring.shape != tuple(fr.shape):
            ring = PinnedRing(fr.shape, device, depth)
        j = ring.next_slot()
        if fr.is_pinned():
            dev, ev = ring.upload(j, src=fr.contiguous())
            src = batch.get("_src")
            if src is not None:              # the producer's staging slot is busy until this copy has left it
                src.event = ev
        else:
            ring.host[j].copy_(fr)
            dev, ev = ring.upload(j)
        out = dict(batch)
        out.pop("_src", None)
        out[key] = dev
        out["_slot"] = (ring, j, ev)
        return out

    def emit(b):
        if auto:
            wait(b)
            slot = b.pop("_slot", None)
            yield b
            if slot is not None:
                slot[0].release(slot[1])
        else:
            yield b

    for batch in loader:
        nxt = start(batch)
        if pending is not None:
            yield from emit(pending)
        pending = nxt
    if pending is not None:
        yield from emit(pending)
