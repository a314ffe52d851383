"""Feeding the training step: clips drawn from resident videos against clips decoded from JPEG, in ONE process.

    python tools/bench_train_feed.py [--videos 4] [--frames 300] [--clips 96] [--procs 16]     one JSON record, printed
                                                                                               and written to profiles/train_feed.json
    python tools/bench_train_feed.py --decode-device [same options]      the JPEG decode on the device against the decode on the
                                                                         host (decode_device_main), profiles/train_feed_device_decode.json
    python tools/bench_train_feed.py --resident-jpeg [same options]      clips decoded per batch from JPEG streams that stay on the
                                                                         device (resident_jpeg_main), profiles/train_feed_resident_jpeg.json
    python tools/bench_train_feed.py --resident-jpeg --stream-clips 0.5 min [same options]
                                                                         the same loader over a set larger than its budget
                                                                         (streamed_jpeg_main), profiles/train_feed_streamed_jpeg.json
    python tools/bench_train_feed.py --joint [same options]              the joint loader over two parts against the single-set
                                                                         loader over the same frames and the host-decoded joint
                                                                         feed (joint_main), profiles/train_feed_joint.json

Synthetic JPEG videos (224 x 224, quality 90) are written to a temporary directory with a label file.  Measured:
  loader   clips/s of `trainclips.ResidentClips` alone (T = 100, batch 8), without mixup (the uint8 batch) and with it (labels
           of both clips + the deferred gather-and-blend with Beta(0.2, 0.2) weights), after the one-off decode of every frame;
  epoch    clips/s of a RegNetY-200MF training epoch (`TDEEDModel.epoch`, bf16, mixup as train_tdeed.py trains) fed
           A  by `feeder.clip_batches` + `ProcessDecodePool(--procs)`: the same clips decoded from JPEG per draw, two per item,
           B  by `ResidentClips`;
           one warm-up epoch each, then `--repeats` timed epochs, alternating; every round draws new clips, the same ones on
           both routes."""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdeed_amd  # noqa: E402,F401
from tdeed_amd import synth, state_layout, feeder  # noqa: E402
from tdeed_amd import trainclips as TC  # noqa: E402

CFG = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4, num_classes=4,
           radi_displacement=2)
H = W = 224
CLASSES = {"a": 1, "b": 2, "c": 3, "d": 4}
DATASET = "fs_comp"                                  # frame_dir/<video>/frame<N>.jpg


def write_videos(root, n_videos, n_frames):
    from PIL import Image
    rs = np.random.RandomState(0)
    videos = []
    for v in range(n_videos):
        name = f"video{v:02d}"
        os.makedirs(os.path.join(root, name))
        base = rs.randint(0, 256, (H // 8, W // 8, 3), dtype=np.uint8)        # blocky content: ~10-20 KB per frame
        for i in range(n_frames):
            img = np.kron(np.roll(base, i, axis=1), np.ones((8, 8, 1), dtype=np.uint8))
            img = (img.astype(np.int16) + rs.randint(-12, 13, img.shape)).clip(0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, name, f"frame{i}.jpg"), quality=90)
        frames = sorted(rs.choice(n_frames, size=max(1, n_frames // 25), replace=False).tolist())
        videos.append(dict(video=name, num_frames=n_frames,
                           events=[dict(frame=int(f), label=list(CLASSES)[int(rs.randint(0, 4))]) for f in frames]))
    return videos


def decoded_loader(root, videos, pool, mixup, dataset_len, batch_size, seed):
    """The reference's route on the same draws: every drawn clip decoded from its JPEGs (`feeder.load_paths` ->
    `feeder.clip_batches`), two clips per item with mixup; labels from the host rule."""
    T, r = CFG["clip_len"], CFG["radi_displacement"]
    tab = TC.train_clip_table(videos, CLASSES, T)
    draws = list(TC.ClipDraws(len(tab.clip_video), dataset_len, batch_size, mixup, seed, drop_last=True))

    def descr(ids):
        return [dict(paths=feeder.load_paths(root, DATASET, videos[int(tab.clip_video[c])]["video"], int(tab.clip_base[c]),
                                             int(tab.clip_base[c]) + T, stride=1), stride=1) for c in ids]
    # (the pool hands out its staging slots per (depth, shape): the partner stream asks for another depth to get its own)
    streams = [feeder.clip_batches(descr(np.concatenate([d[k] for d in draws])), batch_size, (3, H, W), T, pool=pool, depth=3 + k)
               for k in range(2 if mixup else 1)]
    for (ia, ib), *got in zip(draws, *streams):
        lab, labD = TC.rasterise_labels(tab, ia, T, 1, r)
        b = dict(frame=got[0]["frame"], _src=got[0]["_src"], label=torch.from_numpy(lab), labelD=torch.from_numpy(labD))
        if mixup:
            lab2, labD2 = TC.rasterise_labels(tab, ib, T, 1, r)
            b.update(frame2=got[1]["frame"], label2=torch.from_numpy(lab2), labelD2=torch.from_numpy(labD2))
        yield b


def device_loader(root, videos, threads, mixup, dataset_len, batch_size, seed, cache, stats=None):
    """The same draws fed by `feeder.device_clip_batches`: the JPEG files go to the device and are decoded there, the
    mixup twin in the same slot.  stats: a list that collects the per-batch `feeder.last_decode_stats`."""
    T, r = CFG["clip_len"], CFG["radi_displacement"]
    tab = TC.train_clip_table(videos, CLASSES, T)
    draws = list(TC.ClipDraws(len(tab.clip_video), dataset_len, batch_size, mixup, seed, drop_last=True))

    def paths(c):
        return feeder.load_paths(root, DATASET, videos[int(tab.clip_video[c])]["video"], int(tab.clip_base[c]),
                                 int(tab.clip_base[c]) + T, stride=1)
    clips = []
    for ia, ib in draws:
        for i, c in enumerate(ia):
            d = dict(paths=paths(c), stride=1)
            if mixup:
                d.update(paths2=paths(ib[i]), stride2=1)
            clips.append(d)
    feed = feeder.device_clip_batches(clips, batch_size, (3, H, W), T, pool=threads, parse_cache=cache)
    for (ia, ib), got in zip(draws, feed):
        if stats is not None:
            stats.append(dict(feeder.last_decode_stats))
        lab, labD = TC.rasterise_labels(tab, ia, T, 1, r)
        b = dict(frame=got["frame"], _slot=got["_slot"], label=torch.from_numpy(lab), labelD=torch.from_numpy(labD))
        if mixup:
            lab2, labD2 = TC.rasterise_labels(tab, ib, T, 1, r)
            b.update(frame2=got["frame2"], label2=torch.from_numpy(lab2), labelD2=torch.from_numpy(labD2))
        yield b


def decode_device_main(a):
    """--decode-device: `feeder.device_clip_batches` against `feeder.clip_batches` + ProcessDecodePool + `prefetch` on the
    same noise-frame videos, in one run, the routes alternating: (a) the loader alone, the device feed with a cold and
    with a warm parse cache, (b) a 200MF training epoch with mixup fed by each; and the bytes per batch that cross the
    host-device link.  One JSON record, printed and written to profiles/train_feed_device_decode.json."""
    from tdeed_amd import jpegdev
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, bs = CFG["clip_len"], a.batch
    root = tempfile.mkdtemp(prefix="tdeed_train_feed_")
    out = dict(kind="train_feed_device_decode", cfg=CFG, videos=a.videos, frames_per_video=a.frames, clips_per_epoch=a.clips,
               batch_size=bs, decode_processes=a.procs, read_threads=a.read_threads, repeats=a.repeats,
               device=torch.cuda.get_device_name(0))
    pool = threads = None
    try:
        videos = write_videos(root, a.videos, a.frames)
        sizes = [os.path.getsize(os.path.join(root, v["video"], f"frame{i}.jpg")) for v in videos for i in range(a.frames)]
        out["jpeg_bytes_per_frame"] = round(float(np.mean(sizes)), 1)
        pool = feeder.ProcessDecodePool(a.procs)
        threads = feeder.DecodePool(a.read_threads) if a.read_threads > 0 else None       # None: the feed reads the files itself
        n_epoch = a.clips // bs * bs

        def drain(loader):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in feeder.prefetch(loader, "cuda"):
                pass
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        # ---- (a) the loader alone, plain clips; every round draws new clips, the same for both routes
        t_host, t_cold, t_warm, stats = [], [], [], []
        for rep in range(a.repeats + 1):
            seed = 10 + rep
            th = drain(decoded_loader(root, videos, pool, False, a.clips, bs, seed))
            tc = drain(device_loader(root, videos, threads, False, a.clips, bs, seed, jpegdev.ParseCache()))
            cache = jpegdev.ParseCache()
            drain(device_loader(root, videos, threads, False, a.clips, bs, seed, cache))
            tw = drain(device_loader(root, videos, threads, False, a.clips, bs, seed, cache, stats if rep else None))
            if rep:                                                            # the first round warms up
                t_host.append(th), t_cold.append(tc), t_warm.append(tw)
        out["loader"] = dict(host_decoded=_rate(t_host, n_epoch), device_first_epoch=_rate(t_cold, n_epoch),
                             device_warm_cache=_rate(t_warm, n_epoch))
        out["loader"]["device_warm_over_host"] = round(out["loader"]["device_warm_cache"]["clips_per_s"] /
                                                       out["loader"]["host_decoded"]["clips_per_s"], 3)
        out["link_bytes_per_batch"] = dict(host_decoded=bs * T * 3 * H * W,
                                           device_decoded=int(np.mean([s["stream_bytes"] for s in stats])))
        out["device_batch"] = {k: float(np.mean([s[k] for s in stats])) for k in
                               ("frames", "device_frames", "fallback_frames", "table_sets", "segments", "chunks")}

        # ---- (b) a training epoch with mixup fed by either route
        m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
        m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
        opt, _ = m.get_optimizer({"lr": 1e-4})
        cache = jpegdev.ParseCache()
        rnd = {"i": 0}
        routes = dict(A_host_decoded=lambda: decoded_loader(root, videos, pool, True, a.clips, bs, 2 + rnd["i"]),
                      C_device_decoded=lambda: device_loader(root, videos, threads, True, a.clips, bs, 2 + rnd["i"], cache))
        times, losses = {k: [] for k in routes}, {}
        for rep in range(a.repeats + 1):
            rnd["i"] = rep
            for k, mk in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses[k] = m.epoch(mk(), optimizer=opt)
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        out["epoch"] = {k: dict(_rate(v, n_epoch), last_loss=round(float(losses[k]), 5)) for k, v in times.items()}
        ra, rc = out["epoch"]["A_host_decoded"], out["epoch"]["C_device_decoded"]
        out["epoch"]["speedup_C_over_A"] = round(rc["clips_per_s"] / ra["clips_per_s"], 3)
        out["epoch"]["C_not_slower_than_A"] = bool(rc["clips_per_s"] >= ra["clips_per_s_min"])
        out["notes"] = [
            "the JPEG files stay in the page cache on both routes: decode is measured, not disk",
            "loader: plain clips (no twin), drained through feeder.prefetch; device_first_epoch parses every file "
            "(jpegdev.parse in Python), device_warm_cache has every file in the ParseCache",
            "epoch: mixup as train_tdeed.py trains; route A uploads 'frame2' by epoch()'s blocking copy, route C decodes it into "
            "the second half of the batch slot; route C's parse cache is cold in the warm-up round only where clips repeat",
            "link_bytes_per_batch is per plain batch; with the twin both routes move twice as much"]
    finally:
        if pool is not None:
            pool.close()
        if threads is not None:
            threads.close()
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    path = a.out if a.out else os.path.join(ROOT, "profiles", "train_feed_device_decode.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(line + "\n")
    return 0


def resident_jpeg_main(a):
    """--resident-jpeg: `trainclips.ResidentJpegClips` (the entropy streams resident, every batch decoded on the device)
    against `trainclips.ResidentClips` (every frame resident decoded) and `feeder.clip_batches` + ProcessDecodePool, on the
    same noise-frame videos, in one run, the routes alternating: (a) the loader alone, plain clips, (b) a 200MF training
    epoch with mixup fed by each.  Per route: clips/s with its spread over the rounds, resident bytes per frame, the time
    of its construction, and for the new route the time of the per-piece entropy kernel per batch from device events.  One
    JSON record, printed and written to profiles/train_feed_resident_jpeg.json.  No threshold: `faster` says for every pair
    of routes whether the slowest round of one beat the fastest round of the other."""
    from tdeed_amd import jpegdev
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, r, bs = CFG["clip_len"], CFG["radi_displacement"], a.batch
    root = tempfile.mkdtemp(prefix="tdeed_train_feed_")
    out = dict(kind="train_feed_resident_jpeg", cfg=CFG, videos=a.videos, frames_per_video=a.frames, clips_per_epoch=a.clips,
               batch_size=bs, decode_processes=a.procs, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    pool = None
    try:
        videos = write_videos(root, a.videos, a.frames)
        n_frames = a.videos * a.frames
        sizes = [os.path.getsize(os.path.join(root, v["video"], f"frame{i}.jpg")) for v in videos for i in range(a.frames)]
        out["jpeg_bytes_per_frame"] = round(float(np.mean(sizes)), 1)
        threads = feeder.DecodePool(a.procs)
        common = dict(clip_len=T, radi_displacement=r, batch_size=bs, drop_last=True, device="cuda", dataset_len=a.clips, seed=1)

        def build(mixup):
            """both resident loaders, with the time each took from the files to a loader that is ready"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            jp = TC.ResidentJpegClips(videos, TC.load_resident_jpegs(root, DATASET, videos, pool=threads,
                                                                     cache=jpegdev.ParseCache()), CLASSES, mixup=mixup, **common)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rc = TC.ResidentClips(videos, TC.load_resident_videos(root, DATASET, videos, pool=threads), CLASSES, mixup=mixup,
                                  **common)
            torch.cuda.synchronize()
            return jp, rc, round(t1 - t0, 3), round(time.perf_counter() - t1, 3)
        jp, rc, t_jp, t_rc = build(False)
        st = jp.stats
        out["set"] = {k: st[k] for k in ("frames", "device_frames", "fallback_frames", "segments", "pieces", "shards", "table_sets",
                                         "stream_bytes", "resident_bytes", "decoded_bytes")}
        out["pieces_per_frame"] = round(st["pieces"] / max(st["device_frames"], 1), 2)
        out["resident_bytes_per_frame"] = dict(resident_jpeg=round(st["resident_bytes"] / n_frames, 1),
                                               resident_decoded=round(st["decoded_bytes"] / n_frames, 1), host_decoded=0)
        out["frames_per_decoded_frame_budget"] = round(st["decoded_bytes"] / st["resident_bytes"], 2)
        out["construction_s"] = dict(resident_jpeg=t_jp, resident_decoded=t_rc, host_decoded=0.0)
        pool = feeder.ProcessDecodePool(a.procs)
        n_epoch = a.clips // bs * bs

        def drain(loader):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in feeder.prefetch(loader, "cuda"):
                pass
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def reseeded(ld, seed):
            ld.reseed(seed)
            return ld

        def faster(res):
            names = list(res)
            return {f"{x}_over_{y}": bool(res[x]["clips_per_s_min"] > res[y]["clips_per_s_max"]) for x in names for y in names if x != y}

        def ratios(res):
            return {f"resident_jpeg_over_{y}": round(res["resident_jpeg"]["clips_per_s"] / res[y]["clips_per_s"], 3)
                    for y in res if y != "resident_jpeg"}

        # ---- (a) the loader alone, plain clips; every round draws new clips, the same for every route
        routes = dict(resident_jpeg=lambda seed: reseeded(jp, seed), resident_decoded=lambda seed: reseeded(rc, seed),
                      host_decoded=lambda seed: decoded_loader(root, videos, pool, False, a.clips, bs, seed))
        times = {k: [] for k in routes}
        for rep in range(a.repeats + 1):
            jp.item_events = [] if rep else None
            for k, mk in routes.items():
                t = drain(mk(10 + rep))
                if rep:                                                        # the first round warms up
                    times[k].append(t)
            if rep:
                ms = [e0.elapsed_time(e1) for e0, e1 in jp.item_events]
                out.setdefault("item_kernel_ms_per_batch", []).append(round(float(np.sum(ms)) / max(len(jp), 1), 4))
        jp.item_events = None
        out["loader"] = {k: _rate(v, n_epoch) for k, v in times.items()}
        out["loader"]["ratio"] = ratios({k: out["loader"][k] for k in routes})
        out["loader"]["faster"] = faster({k: out["loader"][k] for k in routes})
        del jp, rc

        # ---- (b) a training epoch with mixup fed by each route
        jp, rc, t_jp, t_rc = build(True)
        out["construction_s_mixup"] = dict(resident_jpeg=t_jp, resident_decoded=t_rc, host_decoded=0.0)
        threads.close()
        m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
        m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
        opt, _ = m.get_optimizer({"lr": 1e-4})
        routes = dict(resident_jpeg=lambda seed: reseeded(jp, seed), resident_decoded=lambda seed: reseeded(rc, seed),
                      host_decoded=lambda seed: decoded_loader(root, videos, pool, True, a.clips, bs, seed))
        times, losses = {k: [] for k in routes}, {}
        for rep in range(a.repeats + 1):
            for k, mk in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses[k] = m.epoch(mk(2 + rep), optimizer=opt)
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        out["epoch"] = {k: dict(_rate(v, n_epoch), last_loss=round(float(losses[k]), 5)) for k, v in times.items()}
        out["epoch"]["ratio"] = ratios({k: out["epoch"][k] for k in routes})
        out["epoch"]["faster"] = faster({k: out["epoch"][k] for k in routes})
        out["notes"] = [
            "the JPEG files stay in the page cache on every route: decode is measured, not disk",
            "loader: plain clips, drained through feeder.prefetch; the resident routes' construction (construction_s: reading, "
            "parsing / decoding every file once, upload, index pass) is not in their rounds",
            "item_kernel_ms_per_batch: per timed loader round, the summed event time of ops.jpeg_entropy_items over the round "
            "divided by its batches",
            "epoch: mixup as train_tdeed.py trains; the host route uploads 'frame2' by epoch()'s blocking copy",
            "faster[x_over_y] is true only where x's slowest round beat y's fastest"]
    finally:
        if pool is not None:
            pool.close()
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    path = a.out if a.out else os.path.join(ROOT, "profiles", "train_feed_resident_jpeg.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(line + "\n")
    return 0


def streamed_jpeg_main(a):
    """--resident-jpeg --stream-clips F [F ...]: `trainclips.ResidentJpegClips(stream_clips=True)` at max_resident_bytes = F x
    the all-resident bytes of the set ("min": `stream_plan`'s smallest budget, everything streamed; a fraction below it is
    raised to it) against the all-resident loader (fraction 1.0, the keyword off) and `feeder.clip_batches` +
    ProcessDecodePool, on the same noise-frame videos, in one run, the routes alternating: (a) the loader alone, plain clips,
    (b) a 200MF training epoch with mixup fed by each.  Per setting: the budget, resident and streamed videos, staging and
    host-only bytes, clips/s with its spread over the rounds, the bytes copied per batch and the time of the per-piece entropy
    kernel per batch from device events.  One JSON record, printed and written to profiles/train_feed_streamed_jpeg.json.
    No threshold: `faster` says for every pair of routes whether the slowest round of one beat the fastest round of the other."""
    from tdeed_amd import jpegdev
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, r, bs = CFG["clip_len"], CFG["radi_displacement"], a.batch
    root = tempfile.mkdtemp(prefix="tdeed_train_feed_")
    out = dict(kind="train_feed_streamed_jpeg", cfg=CFG, videos=a.videos, frames_per_video=a.frames, clips_per_epoch=a.clips,
               batch_size=bs, decode_processes=a.procs, repeats=a.repeats, shard_bytes=a.shard_mib << 20,
               device=torch.cuda.get_device_name(0), measured_on_gpu=True)
    pool = None
    try:
        videos = write_videos(root, a.videos, a.frames)
        threads = feeder.DecodePool(a.procs)
        jpegs = TC.load_resident_jpegs(root, DATASET, videos, pool=threads, cache=jpegdev.ParseCache(), shard_bytes=a.shard_mib << 20)
        threads.close()
        common = dict(clip_len=T, radi_displacement=r, batch_size=bs, drop_last=True, device="cuda", dataset_len=a.clips, seed=1)
        n_epoch = a.clips // bs * bs

        def build(mixup):
            """{route: loader}: the all-resident loader and one streamed loader per setting, with what each keeps where"""
            made = dict(resident_all=TC.ResidentJpegClips(videos, jpegs, CLASSES, mixup=mixup, **common))
            whole = made["resident_all"].stats["resident_bytes"]
            low = TC.ResidentJpegClips(videos, jpegs, CLASSES, mixup=mixup, stream_clips=True, **common)._plan.min_budget
            info = dict(resident_all=dict(budget_fraction=1.0, resident_bytes=whole))
            for f in a.stream_clips:
                want = low if f == "min" else int(float(f) * whole)
                ld = TC.ResidentJpegClips(videos, jpegs, CLASSES, mixup=mixup, stream_clips=True, max_resident_bytes=max(want, low),
                                          **common)
                made[f"streamed_{f}"] = ld
                info[f"streamed_{f}"] = dict(budget_fraction=f, asked_bytes=want, max_resident_bytes=max(want, low),
                                             smallest_budget=low, raised_to_smallest=bool(want < low),
                                             **{k: ld.stats[k] for k in ("resident_bytes", "resident_videos", "streamed_videos",
                                                                         "stage_bytes", "host_stream_bytes", "stream_bytes")})
            torch.cuda.synchronize()
            return made, info

        def drain(loader):
            for _ in feeder.prefetch(loader, "cuda"):
                pass

        def reseeded(ld, seed):
            ld.reseed(seed)
            return ld

        def faster(res):
            names = list(res)
            return {f"{x}_over_{y}": bool(res[x]["clips_per_s_min"] > res[y]["clips_per_s_max"]) for x in names for y in names if x != y}

        def per_batch(made, res):
            """the event time of the items kernel and the bytes copied, per batch, of the timed rounds of every resident route"""
            for k, ld in made.items():
                ms = [e0.elapsed_time(e1) for e0, e1 in ld.item_events]
                res[k]["item_kernel_ms_per_batch"] = round(float(np.sum(ms)) / max(len(ld) * a.repeats, 1), 4)
                res[k]["copied_bytes_per_batch"] = int(np.mean(ld.stage_log)) if ld.stage_log else 0
                ld.item_events = ld.stage_log = None

        def run(made, host, first_seed, step):
            routes = {k: (lambda seed, ld=ld: reseeded(ld, seed)) for k, ld in made.items()}
            routes["host_decoded"] = host
            times, last = {k: [] for k in routes}, {}
            for rep in range(a.repeats + 1):
                if rep == 1:                                                   # the first round warms up
                    for ld in made.values():
                        ld.item_events, ld.stage_log = [], []
                for k, mk in routes.items():                                   # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = step(mk(first_seed + rep))
                    torch.cuda.synchronize()
                    if rep:
                        times[k].append(time.perf_counter() - t0)
            res = {k: dict(_rate(v, n_epoch), rounds_s=[round(x, 4) for x in v]) for k, v in times.items()}
            per_batch(made, res)
            return res, last

        # ---- (a) the loader alone, plain clips; every round draws new clips, the same for every route
        made, out["settings_plain"] = build(False)
        st = made["resident_all"].stats
        out["set"] = {k: st[k] for k in ("frames", "device_frames", "fallback_frames", "segments", "pieces", "shards", "table_sets",
                                         "stream_bytes", "resident_bytes", "decoded_bytes")}
        out["jpeg_stream_bytes_per_frame"] = round(st["stream_bytes"] / max(st["frames"], 1), 1)
        pool = feeder.ProcessDecodePool(a.procs)
        out["loader"], _ = run(made, lambda seed: decoded_loader(root, videos, pool, False, a.clips, bs, seed), 10,
                               drain)
        out["loader"]["faster"] = faster({k: v for k, v in out["loader"].items()})
        del made

        # ---- (b) a training epoch with mixup fed by each route
        made, out["settings_mixup"] = build(True)
        m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
        m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
        opt, _ = m.get_optimizer({"lr": 1e-4})
        out["epoch"], losses = run(made, lambda seed: decoded_loader(root, videos, pool, True, a.clips, bs, seed), 2,
                                   lambda ld: m.epoch(ld, optimizer=opt))
        for k, v in losses.items():
            out["epoch"][k]["last_loss"] = round(float(v), 5)
        out["epoch"]["faster"] = faster({k: v for k, v in out["epoch"].items()})
        out["notes"] = [
            "the JPEG files stay in the page cache on the host route: decode is measured, not disk",
            "resident_all is ResidentJpegClips without the keyword: every stream on the device, the absolute items entry",
            "streamed_F: stream_clips=True with max_resident_bytes = F x resident_all's bytes, raised to the smallest budget the plan "
            "allows where F asks for less (raised_to_smallest); streamed_min: that smallest budget, every video streamed",
            "copied_bytes_per_batch: mean bytes of the range copies host -> staging region per batch of the timed rounds; "
            "item_kernel_ms_per_batch: summed event time of the items launches of the timed rounds divided by their batches",
            "construction (reading and parsing every file once, upload, index pass) is not in the rounds",
            "faster[x_over_y] is true only where x's slowest round beat y's fastest"]
    finally:
        if pool is not None:
            pool.close()
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    path = a.out if a.out else os.path.join(ROOT, "profiles", "train_feed_streamed_jpeg.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(line + "\n")
    return 0


CLASSES2 = {"d": 1, "c": 2, "b": 3, "a": 4, "e": 5, "f": 6}          # the second part's own class list (and head)


def joint_decoded_loader(root, parts, pool, mixup, batch_size, seed):
    """The reference's joint route on `JointDraws`' draws: every drawn clip decoded from its JPEGs at the stride of its part
    (`feeder.load_paths` -> `feeder.clip_batches`), two clips per item with mixup; labels from the host rule, 'dataset' per
    item -- the batches `trainclips.JointResidentJpegClips` delivers."""
    T, r = CFG["clip_len"], CFG["radi_displacement"]
    tab = TC.join_clip_tables([TC.train_clip_table(p["videos"], p["classes"], T, p["stride"], p["overlap"]) for p in parts])
    videos = [v for p in parts for v in p["videos"]]
    per_clip = np.repeat([p["stride"] for p in parts], np.diff(tab.part_clips))
    draws = [(part, tab.part_clips[part - 1] + ia, None if ib is None else tab.part_clips[part - 1] + ib)
             for part, ia, ib in TC.JointDraws(np.diff(tab.part_clips), [p["dataset_len"] for p in parts], batch_size, mixup, seed,
                                               drop_last=True)]

    def descr(ids):
        return [dict(paths=feeder.load_paths(root, DATASET, videos[int(tab.clip_video[c])]["video"], int(tab.clip_base[c]),
                                             int(tab.clip_base[c]) + T * int(per_clip[c]), stride=int(per_clip[c])),
                     stride=int(per_clip[c])) for c in ids]
    streams = [feeder.clip_batches(descr(np.concatenate([d[1 + k] for d in draws])), batch_size, (3, H, W), T, pool=pool, depth=3 + k)
               for k in range(2 if mixup else 1)]
    for (part, ia, ib), *got in zip(draws, *streams):
        lab, labD = TC.rasterise_labels(tab, ia, T, per_clip[ia], r)
        b = dict(frame=got[0]["frame"], _src=got[0]["_src"], label=torch.from_numpy(lab), labelD=torch.from_numpy(labD),
                 dataset=torch.from_numpy(part))
        if mixup:
            lab2, labD2 = TC.rasterise_labels(tab, ib, T, per_clip[ib], r)
            b.update(frame2=got[1]["frame"], label2=torch.from_numpy(lab2), labelD2=torch.from_numpy(labD2))
        yield b


def joint_main(a):
    """--joint: `trainclips.JointResidentJpegClips` over two parts of equal size (the first and the second half of the tool's
    noise-frame videos, strides --joint-strides, two class lists) against (b) `trainclips.ResidentJpegClips` over the same
    frames as ONE set at the first part's stride -- the single-set code, the yardstick for what the per-clip tables cost --
    and (c) `feeder.clip_batches` + ProcessDecodePool producing the same joint batches; in one run, the routes alternating, a
    warm-up round then --repeats timed ones: the loader alone (plain clips), then a 200MF two-head mixup epoch on (a) and
    (c).  One JSON record, printed and written to profiles/train_feed_joint.json.  No threshold: `faster` says for every pair
    of routes whether the slowest round of one beat the fastest round of the other."""
    from tdeed_amd import jpegdev
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, r, bs = CFG["clip_len"], CFG["radi_displacement"], a.batch
    if a.videos < 2 or a.videos % 2:
        raise SystemExit("--joint: --videos must be even, two parts of equal size")
    root = tempfile.mkdtemp(prefix="tdeed_train_feed_")
    out = dict(kind="train_feed_joint", cfg=CFG, videos=a.videos, frames_per_video=a.frames, clips_per_epoch=a.clips,
               batch_size=bs, decode_processes=a.procs, repeats=a.repeats, strides=list(a.joint_strides),
               device=torch.cuda.get_device_name(0), measured_on_gpu=True)
    pool = None
    try:
        videos = write_videos(root, a.videos, a.frames)
        half = a.videos // 2
        threads = feeder.DecodePool(a.procs)
        cache = jpegdev.ParseCache()
        halves = [videos[:half], videos[half:]]
        packs = [TC.load_resident_jpegs(root, DATASET, vs, pool=threads, cache=cache) for vs in halves]
        whole = TC.load_resident_jpegs(root, DATASET, videos, pool=threads, cache=cache)
        threads.close()
        lens = [a.clips - a.clips // 2, a.clips // 2]
        parts = [dict(videos=vs, classes=cl, stride=int(s), overlap=1, dataset_len=n)
                 for vs, cl, s, n in zip(halves, (CLASSES, CLASSES2), a.joint_strides, lens)]
        common = dict(clip_len=T, radi_displacement=r, batch_size=bs, drop_last=True, device="cuda", seed=1)
        n_epoch = a.clips // bs * bs

        def build(mixup):
            joint = TC.JointResidentJpegClips([dict(p, jpegs=j) for p, j in zip(parts, packs)], mixup=mixup, **common)
            single = TC.ResidentJpegClips(videos, whole, CLASSES, stride=int(a.joint_strides[0]), mixup=mixup, dataset_len=a.clips,
                                          **common)
            torch.cuda.synchronize()
            return joint, single

        def drain(loader):
            for _ in feeder.prefetch(loader, "cuda"):
                pass

        def reseeded(ld, seed):
            ld.reseed(seed)
            return ld

        def faster(res):
            names = list(res)
            return {f"{x}_over_{y}": bool(res[x]["clips_per_s_min"] > res[y]["clips_per_s_max"]) for x in names for y in names if x != y}

        def run(routes, first_seed, step):
            times, last = {k: [] for k in routes}, {}
            for rep in range(a.repeats + 1):
                for k, mk in routes.items():                                   # alternating; the first round warms up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = step(mk(first_seed + rep))
                    torch.cuda.synchronize()
                    if rep:
                        times[k].append(time.perf_counter() - t0)
            return {k: dict(_rate(v, n_epoch), rounds_s=[round(x, 4) for x in v]) for k, v in times.items()}, last

        # ---- the loader alone, plain clips; every round draws new clips
        joint, single = build(False)
        out["set"] = dict(joint={k: joint.stats[k] for k in ("frames", "device_frames", "table_sets", "shards", "resident_bytes")},
                          single={k: single.stats[k] for k in ("frames", "device_frames", "table_sets", "shards", "resident_bytes")})
        pool = feeder.ProcessDecodePool(a.procs)
        routes = dict(a_joint_resident_jpeg=lambda seed: reseeded(joint, seed),
                      b_single_resident_jpeg=lambda seed: reseeded(single, seed),
                      c_joint_host_decoded=lambda seed: joint_decoded_loader(root, parts, pool, False, bs, seed))
        out["loader"], _ = run(routes, 10, drain)
        res = {k: out["loader"][k] for k in routes}
        out["loader"]["ratio"] = dict(a_over_b=round(res["a_joint_resident_jpeg"]["clips_per_s"] /
                                                     res["b_single_resident_jpeg"]["clips_per_s"], 3),
                                      a_over_c=round(res["a_joint_resident_jpeg"]["clips_per_s"] /
                                                     res["c_joint_host_decoded"]["clips_per_s"], 3))
        out["loader"]["faster"] = faster(res)
        del joint, single

        # ---- a two-head training epoch with mixup fed by (a) and by (c)
        joint, single = build(True)
        del single
        m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
        m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
        heads = [len(CLASSES) + 1, len(CLASSES2) + 1]
        m._model.update_pred_head(heads)
        m._num_classes = sum(heads)                                             # train_tdeed.py:147-148
        opt, _ = m.get_optimizer({"lr": 1e-4})
        routes = dict(a_joint_resident_jpeg=lambda seed: reseeded(joint, seed),
                      c_joint_host_decoded=lambda seed: joint_decoded_loader(root, parts, pool, True, bs, seed))
        out["epoch"], losses = run(routes, 2, lambda ld: m.epoch(ld, optimizer=opt))
        res = {k: out["epoch"][k] for k in routes}
        for k, v in losses.items():
            out["epoch"][k]["last_loss"] = round(float(v), 5)
        out["epoch"]["ratio"] = dict(a_over_c=round(res["a_joint_resident_jpeg"]["clips_per_s"] /
                                                    res["c_joint_host_decoded"]["clips_per_s"], 3))
        out["epoch"]["faster"] = faster(res)
        out["notes"] = [
            "the JPEG files stay in the page cache on the host route: decode is measured, not disk",
            "a: JointResidentJpegClips over two parts (half of the videos each); b: ResidentJpegClips over all of them as one set, "
            "the single-set code with its scalar stride; c: clip_batches + decode processes on the joint draws",
            "loader: plain clips, drained through feeder.prefetch; construction is not in the rounds",
            "epoch: update_pred_head([5, 7]), mixup as train_tdeed.py trains; the host route uploads 'frame2' by epoch()'s blocking copy",
            "faster[x_over_y] is true only where x's slowest round beat y's fastest"]
    finally:
        if pool is not None:
            pool.close()
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    path = a.out if a.out else os.path.join(ROOT, "profiles", "train_feed_joint.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(line + "\n")
    return 0


def _rate(times, clips):
    t = np.asarray(times)
    return dict(clips_per_s=round(clips / float(np.median(t)), 1), clips_per_s_min=round(clips / float(t.max()), 1),
                clips_per_s_max=round(clips / float(t.min()), 1), s_median=round(float(np.median(t)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--clips", type=int, default=96, help="clips per epoch (dataset_len)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--decode-device", action="store_true",
                    help="measure feeder.device_clip_batches against the host-decoded feed instead (profiles/train_feed_device_decode.json)")
    ap.add_argument("--resident-jpeg", action="store_true",
                    help="measure trainclips.ResidentJpegClips against ResidentClips and the host-decoded feed instead "
                         "(profiles/train_feed_resident_jpeg.json)")
    ap.add_argument("--stream-clips", nargs="+", default=None, metavar="BUDGET_FRACTION",
                    help="with --resident-jpeg: measure ResidentJpegClips(stream_clips=True) at these fractions of the all-resident "
                         "bytes ('min': the smallest budget) against the all-resident loader and the host-decoded feed "
                         "(profiles/train_feed_streamed_jpeg.json)")
    ap.add_argument("--joint", action="store_true",
                    help="measure trainclips.JointResidentJpegClips against ResidentJpegClips over the same frames and the "
                         "host-decoded joint feed instead (profiles/train_feed_joint.json)")
    ap.add_argument("--joint-strides", nargs=2, type=int, default=[1, 1], metavar="STRIDE", help="--joint: the two parts' strides")
    ap.add_argument("--shard-mib", type=int, default=16, help="--stream-clips: shard_bytes of load_resident_jpegs, in MiB")
    ap.add_argument("--read-threads", type=int, default=0,
                    help="--decode-device: threads that read the files (0: the feed's own thread; the files sit in the page cache, "
                         "where a read is too short to be worth a hand-over between threads)")
    ap.add_argument("--out", default=None, help="default: profiles/train_feed.json (train_feed_device_decode.json with --decode-device)")
    a = ap.parse_args()
    if a.decode_device:
        return decode_device_main(a)
    if a.joint:
        return joint_main(a)
    if a.resident_jpeg and a.stream_clips:
        return streamed_jpeg_main(a)
    if a.resident_jpeg:
        return resident_jpeg_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "train_feed.json")
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, r, bs = CFG["clip_len"], CFG["radi_displacement"], a.batch
    root = tempfile.mkdtemp(prefix="tdeed_train_feed_")
    out = dict(kind="train_feed", cfg=CFG, videos=a.videos, frames_per_video=a.frames, clips_per_epoch=a.clips, batch_size=bs,
               decode_processes=a.procs, repeats=a.repeats)
    pool = None
    try:
        videos = write_videos(root, a.videos, a.frames)
        threads = feeder.DecodePool(a.procs)
        t0 = time.perf_counter()
        frames = TC.load_resident_videos(root, DATASET, videos, pool=threads)
        out["decode_once_s"] = round(time.perf_counter() - t0, 3)
        out["decode_once_frames_per_s"] = round(a.videos * a.frames / (time.perf_counter() - t0), 1)
        threads.close()
        common = dict(clip_len=T, radi_displacement=r, batch_size=bs, drop_last=True, device="cuda")

        # ---- the loader alone
        out["loader"] = {}
        for mixup in (False, True):
            n = 64 * bs
            ld = TC.ResidentClips(videos, frames, CLASSES, mixup=mixup, dataset_len=n, seed=1, **common)
            times = []
            for rep in range(a.repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in feeder.prefetch(ld, "cuda"):
                    if mixup:
                        lam = torch.tensor([random.betavariate(0.2, 0.2) for _ in range(bs)], dtype=torch.float32, device="cuda")
                        b["mix"](lam)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t0)
            out["loader"]["mixup" if mixup else "plain"] = _rate(times, n)
            del ld

        # ---- a training epoch fed by either route
        m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
        m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
        opt, _ = m.get_optimizer({"lr": 1e-4})
        pool = feeder.ProcessDecodePool(a.procs)
        # both routes draw the SAME clips in every round: a fresh draw stream from seed 2 + round per epoch and route
        resident = TC.ResidentClips(videos, frames, CLASSES, mixup=True, dataset_len=a.clips, seed=2, **common)
        rnd = {"i": 0}

        def route_b():
            resident.reseed(2 + rnd["i"])
            return resident
        routes = dict(A_decoded=lambda: decoded_loader(root, videos, pool, True, a.clips, bs, 2 + rnd["i"]), B_resident=route_b)
        times = {k: [] for k in routes}
        losses = {}
        for rep in range(a.repeats + 1):
            rnd["i"] = rep
            for k, mk in routes.items():                                     # alternating; the first round warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses[k] = m.epoch(mk(), optimizer=opt)
                torch.cuda.synchronize()
                if rep:
                    times[k].append(time.perf_counter() - t0)
        n_epoch = a.clips // bs * bs
        out["epoch"] = {k: dict(_rate(v, n_epoch), last_loss=round(float(losses[k]), 5)) for k, v in times.items()}
        ra, rb = out["epoch"]["A_decoded"], out["epoch"]["B_resident"]
        out["epoch"]["speedup_B_over_A"] = round(rb["clips_per_s"] / ra["clips_per_s"], 3)
        out["epoch"]["B_not_slower_than_A"] = bool(rb["clips_per_s"] >= ra["clips_per_s_min"])
        out["epoch"]["notes"] = [
            "every round draws new clips (seed 2 + round), the same for both routes; the JPEG files themselves stay in the "
            "page cache, so route A pays decode, not disk",
            "route B's one-off cost -- the JPEG decode of every frame (decode_once_s) and the upload -- is not in its epochs",
            "route A's mixup partner clip ('frame2') is uploaded by epoch()'s blocking copy, not by the prefetch ring: that is "
            "how epoch() treats any host loader today, and it counts against route A"]
    finally:
        if pool is not None:
            pool.close()
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
