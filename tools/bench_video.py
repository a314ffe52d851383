"""Whole-video scoring against the clip-batch route, in ONE process, alternating the routes.

    python tools/bench_video.py [--frames 2030] [--repeats 5]          one JSON line
    python tools/bench_video.py --gather-only                           the gather launch alone (run it under
                                                                        `rocprofv3 --kernel-trace --stats -- python ...`)
    python tools/bench_video.py --decode [--decode-frames 400]          host only: load_video vs clip_batches, JPEG decode
    python tools/bench_video.py --decode-device [--decode-frames 400]   JPEG decode: load_video with 8 threads and with 16
                                                                        worker processes against load_video_device, one JSON
                                                                        line, also written to profiles/jpeg_device_decode.json
    python tools/bench_video.py --spot [--frames 5625]                  events: predict_video + the host chain against
                                                                        spot_video, one JSON line
    python tools/bench_video.py --group [--group-videos 32]             short videos: spot_videos video by video against
                                                                        spot_videos in packed groups, one JSON line
    python tools/bench_video.py --map [--map-videos 24]                 validation mAP: spot_videos + mean_average_precisions
                                                                        against map_videos, one JSON line, also written to
                                                                        profiles/video_map.json
    python tools/bench_video.py --map --ranks 2                         the validation pass sharded over ranks: child
                                                                        processes of this script, each step under a time limit
                                                                        (one rank with and without shard / labels, the exchange
                                                                        alone, then 2 ranks sharing the GPU), one JSON line,
                                                                        also written to profiles/video_map_sharded.json
    python tools/bench_video.py --reuse [--frames 2030]                 predict_video against predict_video(reuse_frames=
                                                                        True), one JSON line, also written to --out
    python tools/bench_video.py --ring [--frames 2030]                  predict_video resident against predict_video(
                                                                        stream_frames=True) at a quarter of the video's bytes,
                                                                        one JSON line, also written to profiles/video_ring.json
    python tools/bench_video.py --resident-jpeg [--frames 2030]         validation mAP fed by host decode, by load_video_device,
                                                                        by ResidentJpegVideos and by its crop=224, one JSON
                                                                        line, also written to profiles/video_resident_jpeg.json

Routes (RegNetY-200MF, T = 100, 224 x 224, bf16; 3/4 overlap like the evaluation datasets):
  A  the clip route: `evalutil.stitch_predictions` over host-resident PINNED uint8 clip batches of the video, at loader
     batch size 4 (the reference's INFERENCE_BATCH_SIZE) and 8; with augment=True at batch size 1, the only batch size the
     route (like the reference's) supports there.
  B  `TDEEDModel.predict_video(batch_size=8)` from the pinned frames of the video.
Every shape is warmed up once (plan build, graph capture); then the routes alternate, `--repeats` timed passes each."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tdeed_amd  # noqa: E402,F401
from tdeed_amd import synth, state_layout, ops, feeder  # noqa: E402
from tdeed_amd import evalutil as E  # noqa: E402

CFG = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4, num_classes=4,
           radi_displacement=2)
H = W = 224
COPY_GBPS = 6290.0        # measured HBM3E copy bandwidth of the MI355X (16-byte copy kernel, read + write; 8 TB/s spec), GB/s


def _stat(times, frames, clips):
    t = np.asarray(times)
    med = float(np.median(t))
    return dict(ms_median=round(med * 1e3, 2), ms_min=round(float(t.min()) * 1e3, 2), ms_max=round(float(t.max()) * 1e3, 2),
                frames_per_s=round(frames / med, 1), clips_per_s=round(clips / med, 1),
                clips_per_s_min=round(clips / float(t.max()), 1), clips_per_s_max=round(clips / float(t.min()), 1))


def bench(a):
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, L = CFG["clip_len"], a.frames
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    video = ops.fill_u8_hash((L, 3, H, W), 9, "cuda").cpu().pin_memory()
    starts = E.video_clip_starts(L, T, T // 4 * 3)
    n = len(starts)
    fb = 3 * H * W
    # route A's input: every clip window materialised on the host, pinned
    clips = torch.zeros((n, T, 3, H, W), dtype=torch.uint8).pin_memory()
    for i, s in enumerate(starts):
        lo, hi = max(s, 0), min(s + T, L)
        clips[i, lo - s:hi - s] = video[lo:hi]
    videos = [("v", L, 25.0)]

    def loader(bs):
        return [dict(frame=clips[lo:lo + bs], video=["v"] * len(starts[lo:lo + bs]), start=np.array(starts[lo:lo + bs]))
                for lo in range(0, n, bs)]

    out = dict(kind="video_scoring", cfg=CFG, frames=L, clips=n, repeats=a.repeats, settings={})
    for augment in (False, True):
        routes = {}
        if augment:
            routes["A_bs1"] = lambda: E.stitch_predictions(m, loader(1), videos, 5, augment=True).tracks["v"]
        else:
            routes["A_bs4"] = lambda: E.stitch_predictions(m, loader(4), videos, 5).tracks["v"]
            routes["A_bs8"] = lambda: E.stitch_predictions(m, loader(8), videos, 5).tracks["v"]
        routes["B_bs8"] = lambda: m.predict_video(video, batch_size=8, augment=augment)
        res = {k: fn() for k, fn in routes.items()}                     # warm-up of every shape
        times = {k: [] for k in routes}
        for _ in range(a.repeats):
            for k, fn in routes.items():                                # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        V = 2 if augment else 1
        st = {k: _stat(v, L, n * V) for k, v in times.items()}
        for k in st:
            st[k]["frame_bytes_h2d"] = m.last_video_stats["frames_h2d_bytes"] if k.startswith("B") else n * V * T * fb
        ref = "A_bs1" if augment else "A_bs8"
        eq = dict(reference=ref, sums_equal=bool(np.array_equal(res[ref][0], res["B_bs8"][0])),
                  support_equal=bool(np.array_equal(res[ref][1], res["B_bs8"][1])),
                  max_abs_diff=float(np.abs(res[ref][0] - res["B_bs8"][0]).max()))
        acc = {}
        for k in st:
            if k.startswith("A"):
                spread = st[k]["clips_per_s_max"] - st[k]["clips_per_s_min"]
                acc[k] = dict(ratio_B_over_A=round(st["B_bs8"]["clips_per_s"] / st[k]["clips_per_s"], 3),
                              B_not_below_A_minus_spread=bool(st["B_bs8"]["clips_per_s"] >= st[k]["clips_per_s"] - spread))
        out["settings"]["augment" if augment else "plain"] = dict(routes=st, equality=eq, acceptance=acc)
    if not out["settings"]["plain"]["equality"]["sums_equal"]:
        out["error"] = "predict_video differs from the clip route at batch size 8 without augmentation"
    print(json.dumps(out))
    return 0 if "error" not in out else 1


def _peaky_track(L, K1, seed=3):
    """a synthetic normalised track like a trained model's: narrow bumps per class on a low noise floor"""
    rng = np.random.RandomState(seed)
    x = (rng.rand(L, K1) ** 48 * 0.2).astype(np.float32)
    f = np.arange(L, dtype=np.float32)[:, None]
    for c in range(1, K1):
        centres = rng.choice(L, size=max(1, L // 150), replace=False).astype(np.float32)[None]
        amp = rng.uniform(0.3, 0.95, size=centres.shape).astype(np.float32)
        x[:, c] += (amp * np.exp(-0.5 * ((f - centres) / 2.0) ** 2)).max(axis=1)
    x[:, 0] = np.maximum(1.0 - x[:, 1:].sum(axis=1), 0.0)
    x /= x.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(x, np.float32)


def _host_chain(norm, classes, fps, suppress, hr):
    pe, recall, _ = E.frame_events(norm, classes, fps, high_recall_score_threshold=hr)
    lists = [(E.soft_non_maximum_suppression if kind == "snms" else E.non_maximum_suppression)(recall, w, thr)
             for kind, w, thr in suppress]
    return pe, recall, lists


def _median_ms(fn, repeats):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 3)


def spot(a):
    """Two routes on the same video, alternating: (1) predict_video -> ScoreStitcher.normalised -> frame_events -> NMS ->
    soft-NMS on the host, (2) spot_video.  Then the tail alone on a synthetic peaky track of the same length with K+1 = 13
    columns: the host chain against ops.frame_events_seg + ops.nms_track_seg (+ the copies of the event lists)."""
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    L = a.frames
    hr = 0.01
    suppress = (("nms", a.window, 0.01), ("snms", a.window, 0.01))
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    video = ops.fill_u8_hash((L, 3, H, W), 9, "cuda").cpu().pin_memory()
    classes = {f"c{k}": k for k in range(1, CFG["num_classes"] + 1)}

    def route_host():
        sums, sup = m.predict_video(video, batch_size=8)
        st = E.ScoreStitcher([("v", L, 25.0)], sums.shape[1])
        st.tracks["v"][0][...] = sums
        st.tracks["v"][1][...] = sup
        pe, _, lists = _host_chain(st.normalised(), classes, st.fps, suppress, hr)
        return pe[0]["events"], [x[0]["events"] for x in lists]

    def route_device():
        r = m.spot_video(video, classes, suppress=suppress, high_recall_score_threshold=hr, batch_size=8)
        return r["events"], r["suppressed"]

    routes = dict(host=route_host, device=route_device)
    res = {k: fn() for k, fn in routes.items()}                         # warm-up
    stats = dict(m.last_video_stats)
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():                                    # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    out = dict(kind="video_spotting", cfg=CFG, frames=L, clips=stats["clips"], repeats=a.repeats, window=a.window,
               predict_video_plus_host_chain_ms=round(float(np.median(times["host"])) * 1e3, 2),
               spot_video_ms=round(float(np.median(times["device"])) * 1e3, 2),
               events=dict(argmax=len(res["device"][0]), nms=len(res["device"][1][0]), snms=len(res["device"][1][1])),
               nms_rounds=stats["nms_rounds"], events_d2h_bytes=stats["events_d2h_bytes"], track_bytes=L * 5 * 4,
               equal=bool(res["host"] == res["device"]))
    # ---- the tail alone, peaky track
    K1 = 13
    mean = _peaky_track(L, K1)
    pk_classes = {f"c{k}": k for k in range(1, K1)}
    inv = {v: k for k, v in pk_classes.items()}
    dmean = torch.from_numpy(mean).cuda()

    def tail_host():
        return [x[0]["events"] for x in _host_chain({"v": mean}, pk_classes, {"v": 25.0}, suppress, hr)[2]]

    last = {}
    seg_off = torch.tensor([0, L], dtype=torch.int32, device="cuda")    # one video: a group of one; uploaded once, not timed

    def events_and_lists():
        first = torch.full((1, K1), L, dtype=torch.int32, device="cuda")
        _, _, first, cnt = ops.frame_events_seg(dmean, seg_off, L, hr, first_init=first)
        return cnt, [ops.nms_track_seg(dmean, seg_off, L, w, thr, kind == "snms", first, hr) for kind, w, thr in suppress]

    def tail_device():
        cnt, lists = events_and_lists()
        counts = [int(x[3].cpu()[1]) for x in lists]                    # synchronises
        host = [[t[:n].cpu().numpy() for t in x[:3]] for x, n in zip(lists, counts)]
        last["rounds"] = [int(x[4].max().cpu()) for x in lists]
        last["recall"] = int(cnt.sum().cpu())
        return [E.event_dicts(f, c, s, inv) for f, c, s in host]

    def tail_device_kernels():
        events_and_lists()
        torch.cuda.synchronize()

    th, td = tail_host(), tail_device()
    tail_device_kernels()
    out["tail_peaky"] = dict(K1=K1, high_recall_events=last["recall"], events=[len(x) for x in td], rounds=last["rounds"],
                             host_chain_ms=_median_ms(tail_host, a.repeats), device_ms=_median_ms(tail_device, a.repeats),
                             device_kernels_only_ms=_median_ms(tail_device_kernels, a.repeats), equal=bool(th == td))
    if not (out["equal"] and out["tail_peaky"]["equal"]):
        out["error"] = "the device route differs from the host chain"
    print(json.dumps(out))
    return 0 if "error" not in out else 1


GROUP_SPLITS = dict(diving=(96, 66, 220, 2.14), tennis=(48, 178, 1442, 2.78))     # videos, shortest, longest, skew


def group_lengths(split):
    """lengths of a synthetic split from a fixed hash: u in [0,1) per video, L = lo + (hi - lo) * u ** skew, the skew chosen
    so that the median sits near the median of the dataset the split is named after (101 / 362 frames)"""
    nvid, lo, hi, skew = GROUP_SPLITS[split]
    mix = lambda h: ((h ^ (h >> 29)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF          # FNV's high bits barely move
    u = [(mix(synth.fnv1a64(f"{split}{i}")) >> 11) / float(1 << 53) for i in range(nvid)]
    out = [lo + int((hi - lo) * x ** skew) for x in u]
    out[0], out[1] = lo, hi                                             # both ends of the range occur
    return out


def _event_keys(lists):
    return {(i, rec["video"], e["label"], e["frame"]): e["score"] for i, lst in enumerate(lists) for rec in lst
            for e in rec["events"]}


def group(a):
    """Two routes over the same synthetic split of short videos, alternating: A `evalutil.spot_videos(group_videos=1)` (one
    spot_video per video), B `spot_videos(group_videos=a.group_videos)` (packed groups).  Pinned frames, default suppression,
    batch size 8, bf16.  Per route: median / min / max seconds over `--repeats` passes, videos/s, clips/s, forward batches,
    host synchronisations and forward plans (one captured graph each) of one pass."""
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T = CFG["clip_len"]
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    classes = {f"c{k}": k for k in range(1, CFG["num_classes"] + 1)}
    suppress = (("nms", 1, 0.01), ("snms", 3, 0.01))
    eng = m._model.engine(torch.bfloat16)
    seen = dict(batches=0, syncs=0, plans=set())
    real_plan, real_sync = eng.plan, torch.cuda.Stream.synchronize

    def plan(*args, **kw):
        p = real_plan(*args, **kw)
        seen["plans"].add(id(p))
        return p

    def sync(self):
        seen["syncs"] += 1
        return real_sync(self)
    eng.plan = plan
    torch.cuda.Stream.synchronize = sync
    for name in ("spot_video", "spot_video_group"):
        def wrapped(*args, _fn=getattr(m, name), **kw):
            r = _fn(*args, **kw)
            seen["batches"] += m.last_video_stats["batches"]
            return r
        setattr(m, name, wrapped)
    out = dict(kind="video_groups", cfg=CFG, batch_size=8, group_videos=a.group_videos, repeats=a.repeats, suppress=suppress,
               splits={})
    for split in a.splits.split(","):
        lengths = group_lengths(split)
        off = np.concatenate([[0], np.cumsum(lengths)])
        packed = torch.empty((int(off[-1]), 3, H, W), dtype=torch.uint8).pin_memory()
        for lo in range(0, int(off[-1]), 2048):                         # generated on the device in pieces
            hi = min(lo + 2048, int(off[-1]))
            packed[lo:hi].copy_(ops.fill_u8_hash((hi - lo, 3, H, W), 9 + lo, "cuda"))
        vids = [(f"v{i:03d}", L, 25.0, packed[off[i]:off[i + 1]]) for i, L in enumerate(lengths)]
        n_clips = sum(len(E.video_clip_starts(L, T, T // 4 * 3)) for L in lengths)
        routes = dict(A=lambda: E.spot_videos(m, vids, classes, suppress, batch_size=8, group_videos=1),
                      B=lambda: E.spot_videos(m, vids, classes, suppress, batch_size=8, group_videos=a.group_videos))
        res, counts = {}, {}
        for k, fn in routes.items():                                    # warm-up of every shape; the second pass is counted
            fn()
            seen.update(batches=0, syncs=0, plans=set())
            res[k] = fn()
            counts[k] = dict(batches=seen["batches"], host_syncs=seen["syncs"], graphs=len(seen["plans"]))
        times = {k: [] for k in routes}
        for _ in range(a.repeats):
            for k, fn in routes.items():                                # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        st = {}
        for k, v in times.items():
            t = np.asarray(v)
            med = float(np.median(t))
            st[k] = dict(ms_median=round(med * 1e3, 2), ms_min=round(float(t.min()) * 1e3, 2),
                         ms_max=round(float(t.max()) * 1e3, 2), videos_per_s=round(len(lengths) / med, 1),
                         clips_per_s=round(n_clips / med, 1), **counts[k])
        ka, kb = _event_keys(res["A"][1]), _event_keys(res["B"][1])
        common = set(ka) & set(kb)
        spread = st["A"]["ms_max"] - st["A"]["ms_min"]
        out["splits"][split] = dict(
            videos=len(lengths), frames=int(off[-1]), clips=n_clips, length_min=min(lengths),
            length_median=float(np.median(lengths)), length_max=max(lengths), routes=st,
            speedup_B_over_A=round(st["A"]["ms_median"] / st["B"]["ms_median"], 3),
            B_not_slower_than_A_by_more_than_A_spread=bool(st["B"]["ms_median"] <= st["A"]["ms_median"] + spread),
            equal=bool(res["A"][0] == res["B"][0] and res["A"][1] == res["B"][1]),
            events=dict(A=len(ka), B=len(kb), common=len(common),
                        max_score_diff_common=max([abs(ka[k] - kb[k]) for k in common], default=0.0)))
        if split == a.splits.split(",")[0]:
            # fp32, the first six videos: per-frame mean scores of the two routes (other batches: a bound, not equality)
            six = [v[3] for v in vids[:6]]
            grp = m.predict_video_group(six, batch_size=8, use_amp=False)
            worst = 0.0
            for fr, (gs, gn) in zip(six, grp):
                s1, n1 = m.predict_video(fr, batch_size=8, use_amp=False)
                d = np.maximum(n1, 1)[:, None].astype(np.float32)
                worst = max(worst, float(np.abs(s1 / d - gs / d).max()))
            out["fp32_max_mean_diff_first6"] = worst
        del vids, packed
    print(json.dumps(out))
    return 0


def _map_workload(a):
    """the synthetic validation split of --map: the 200MF model, `--map-videos` videos of the diving split's lengths with
    hashed frames, a ground-truth event every 20 frames, two suppress entries, five tolerances"""
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    K = CFG["num_classes"]
    classes = {f"c{k}": k for k in range(1, K + 1)}
    suppress = (("nms", 1, 0.10), ("snms", 3, 0.01))
    tols = [0, 1, 2, 4, 8]
    lengths = group_lengths("diving")[:a.map_videos]
    off = np.concatenate([[0], np.cumsum(lengths)])
    packed = torch.empty((int(off[-1]), 3, H, W), dtype=torch.uint8).pin_memory()
    for lo in range(0, int(off[-1]), 2048):
        hi = min(lo + 2048, int(off[-1]))
        packed[lo:hi].copy_(ops.fill_u8_hash((hi - lo, 3, H, W), 9 + lo, "cuda"))
    vids = [(f"v{i:03d}", L, 25.0, packed[off[i]:off[i + 1]]) for i, L in enumerate(lengths)]
    # a ground-truth event every 20 frames, the classes in turn
    truth = [{"video": f"v{i:03d}", "events": [{"label": f"c{1 + (f // 20) % K}", "frame": f} for f in range(7, L, 20)]}
             for i, L in enumerate(lengths)]
    return m, classes, suppress, tols, lengths, off, vids, truth


def map_bench(a):
    """Two routes from the same synthetic videos and model to the mAP tables of a validation pass, alternating: (a)
    `evalutil.spot_videos` + `mean_average_precisions` per suppress entry (event lists to the host, dicts, the Python walk),
    (b) `evalutil.map_videos` (segment + match per group and one rank + AP launch on the device, one small table back).  Per
    route: wall time over `--repeats` passes, host synchronisations and device-to-host bytes of one pass.  The two results
    must agree within max(1, total) * 2^-52 per AP (summation order).  No speed-up is promised: route (a)'s time on the same
    box in the same run is what route (b) is read against."""
    m, classes, suppress, tols, lengths, off, vids, truth = _map_workload(a)
    totals = {lab: sum(1 for x in truth for e in x["events"] if e["label"] == lab) for lab in classes}
    seen = dict(syncs=0, d2h=0)
    real_sync, real_group = torch.cuda.Stream.synchronize, m.spot_video_group

    def sync(self):
        seen["syncs"] += 1
        return real_sync(self)

    def spot_group(*args, **kw):
        r = real_group(*args, **kw)
        seen["d2h"] += m.last_video_stats["events_d2h_bytes"]
        return r
    torch.cuda.Stream.synchronize = sync
    m.spot_video_group = spot_group
    kw = dict(batch_size=8, group_videos=a.group_videos)

    def route_a():
        _, lists, _ = E.spot_videos(m, vids, classes, suppress, **kw)
        seen["events"] = [sum(len(x["events"]) for x in lst) for lst in lists]
        return [E.mean_average_precisions(truth, lst, tols) for lst in lists]

    def route_b():
        r = E.map_videos(m, vids, classes, truth, suppress, tols, **kw)
        seen["d2h"] += m.last_video_stats["ap_d2h_bytes"]
        return r
    routes = dict(a_spot_videos_host_map=route_a, b_map_videos=route_b)
    res, counts = {}, {}
    for k, fn in routes.items():                                        # warm-up of every shape; the second pass is counted
        fn()
        seen.update(syncs=0, d2h=0)
        res[k] = fn()
        counts[k] = dict(host_syncs=seen["syncs"], d2h_bytes=seen["d2h"])
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():                                    # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    torch.cuda.Stream.synchronize = real_sync
    worst, ok = 0.0, True
    for (_, aps_a), (_, aps_b) in zip(res["a_spot_videos_host_map"], res["b_map_videos"]):
        ok = ok and sorted(aps_a) == sorted(aps_b)
        for lab in aps_a:
            for x, y in zip(aps_a[lab], aps_b.get(lab, [])):
                worst = max(worst, abs(x - y))
                ok = ok and abs(x - y) <= max(1, totals[lab]) * 2.0 ** -52
    st = {}
    for k, v in times.items():
        tt = np.asarray(v)
        st[k] = dict(ms_median=round(float(np.median(tt)) * 1e3, 2), ms_min=round(float(tt.min()) * 1e3, 2),
                     ms_max=round(float(tt.max()) * 1e3, 2), **counts[k])
    rec = dict(kind="video_map", device=torch.cuda.get_device_name(0), measured_on_gpu=True, cfg=CFG, videos=len(lengths),
               frames=int(off[-1]), group_videos=a.group_videos, batch_size=8, repeats=a.repeats, suppress=suppress, tolerances=tols,
               truth_events=totals, events_after_suppression=seen.get("events"), routes=st,
               ratio_a_over_b=round(st["a_spot_videos_host_map"]["ms_median"] / st["b_map_videos"]["ms_median"], 3),
               maps_a=[r[0] for r in res["a_spot_videos_host_map"]], maps_b=[r[0] for r in res["b_map_videos"]],
               max_abs_ap_diff=worst, agree_within_bound=bool(ok))
    if a.map_tail_videos:
        rec["tail_noise"] = _map_tail(a, tols)
        ok = ok and rec["tail_noise"]["agree_within_bound"]
    out = os.path.join(ROOT, "profiles", "video_map.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    assert ok, f"the two routes differ (model route by {worst})"
    return 0


def _map_tail(a, tols):
    """The tail alone at validation-set size, no model: `--map-tail-videos` noise tracks of 3 000 frames with K = 12 (noise
    gives far more high-recall events than a trained model: the upper end), entries raw and ("nms", 1, 0.10).  Host: the
    event records (raw: `evalutil.frame_events`; NMS: the device suppression's lists copied back and turned into dicts, as
    `spot_videos` does) and `mean_average_precisions`, one pass, each step timed.  Device: tables, event launch, suppression,
    segment + match, rank + AP and the copy of the table, `--repeats` passes."""
    nv, L, K1, hr = a.map_tail_videos, 3000, 13, 0.01
    rng = np.random.RandomState(1)
    tracks = []
    for _ in range(nv):
        x = rng.rand(L, K1).astype(np.float32)
        tracks.append(np.ascontiguousarray(x / x.sum(axis=1, keepdims=True), np.float32))
    names = [f"t{i:03d}" for i in range(nv)]
    classes = {f"c{k}": k for k in range(1, K1)}
    inv = {v: k for k, v in classes.items()}
    truth = [{"video": v, "events": [{"label": f"c{1 + (f // 20) % (K1 - 1)}", "frame": f} for f in range(7, L, 20)]} for v in names]
    totals = {lab: sum(1 for x in truth for e in x["events"] if e["label"] == lab) for lab in classes}
    entries = (("raw",), ("nms", 1, 0.10))
    table = E.truth_table(truth, {v: i for i, v in enumerate(names)}, classes)
    mean = torch.from_numpy(np.concatenate(tracks)).cuda()
    seg_off = torch.tensor(np.arange(nv + 1) * L, dtype=torch.int32, device="cuda")
    ords = torch.arange(nv, dtype=torch.int32, device="cuda")

    def device():
        state = ops.ap_state([L] * nv, table, K1, len(entries), tols, "cuda")
        first = ops.frame_events_seg(mean, seg_off, L, hr)[2]
        for i, e in enumerate(entries):
            planes = None if e[0] == "raw" else ops.nms_track_seg(mean, seg_off, L, e[1], e[2], e[0] == "snms", first, hr,
                                                                  planes=True)[5:]
            ops.ap_match_seg(state, i, mean, seg_off, ords, L, hr, planes=planes)
        return ops.ap_rank(state)[0].cpu().numpy()                      # synchronises
    ap = device()
    dev_ms = _median_ms(device, a.repeats)
    host = {}
    t0 = time.perf_counter()
    raw = E.frame_events({v: m_ for v, m_ in zip(names, tracks)}, classes, {v: 25.0 for v in names}, high_recall_score_threshold=hr)[1]
    host["raw_records_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    first = ops.frame_events_seg(mean, seg_off, L, hr)[2]
    fr, c8, sc, eoff, _ = ops.nms_track_seg(mean, seg_off, L, 1, 0.10, False, first, hr)
    eo = eoff.cpu().numpy()
    fr, c8, sc = fr[:eo[-1]].cpu().numpy(), c8[:eo[-1]].cpu().numpy(), sc[:eo[-1]].cpu().numpy()
    nms = [{"video": v, "events": E.event_dicts(fr[eo[i]:eo[i + 1]], c8[eo[i]:eo[i + 1]], sc[eo[i]:eo[i + 1]], inv)}
           for i, v in enumerate(names)]
    host["nms_device_suppression_copy_records_s"] = round(time.perf_counter() - t0, 3)
    worst, ok, maps = 0.0, True, []
    for i, (key, lst) in enumerate((("raw", raw), ("nms", nms))):
        t0 = time.perf_counter()
        m_, aps = E.mean_average_precisions(truth, lst, tols)
        host[f"{key}_mean_average_precisions_s"] = round(time.perf_counter() - t0, 3)
        host[f"{key}_events"] = sum(len(x["events"]) for x in lst)
        maps.append(m_)
        for lab in aps:
            for ti in range(len(tols)):
                d = abs(aps[lab][ti] - float(ap[i, ti, classes[lab]]))
                worst = max(worst, d)
                ok = ok and d <= max(1, totals[lab]) * 2.0 ** -52
    return dict(videos=nv, frames_per_video=L, K1=K1, entries=entries, tolerances=tols, truth_events=sum(totals.values()),
                host_one_pass=host, host_total_s=round(sum(v for k, v in host.items() if k.endswith("_s")), 3),
                device_ms_median=dev_ms, d2h_bytes_device=int(ap.size) * 8, maps_host=maps, max_abs_ap_diff=worst,
                agree_within_bound=bool(ok))


# ----------------------------------------------------------------------------- --map --ranks N: the pass sharded over ranks
def _frame_labels(truth, lengths, classes):
    """the truth records as per-frame labels: the class at every ground-truth frame, background elsewhere"""
    out = {}
    for x, L in zip(truth, lengths):
        lab = np.zeros(L, np.int64)
        for e in x["events"]:
            lab[e["frame"]] = classes[e["label"]]
        out[x["video"]] = lab
    return out


def _passes(routes, repeats):
    """one warm-up pass of every route, then `repeats` timed passes with the routes alternating -> ({route: last result},
    {route: [seconds]})"""
    res = {k: fn() for k, fn in routes.items()}
    times = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return res, times


def _ms(v):
    tt = np.asarray(v) * 1e3
    return dict(ms_median=round(float(np.median(tt)), 2), ms_min=round(float(tt.min()), 2), ms_max=round(float(tt.max()), 2))


def _map_sharded_one(a):
    """(a) one process, one rank: `map_videos` as it always ran against the same call with shard=(0, 1) and labels (one more
    launch per group, the merge skipped); (b) the exchange alone on the noise tail.  One JSON line."""
    m, classes, suppress, tols, lengths, off, vids, truth = _map_workload(a)
    labels = _frame_labels(truth, lengths, classes)
    kw = dict(batch_size=8, group_videos=a.group_videos)
    stats = {}

    def plain():
        r = E.map_videos(m, vids, classes, truth, suppress, tols, **kw)
        stats["plain"] = dict(m.last_video_stats)
        return r

    def sharded():
        r = E.map_videos(m, vids, classes, truth, suppress, tols, labels=labels, shard=(0, 1), **kw)
        stats["shard_0_1_labels"] = dict(m.last_video_stats)
        return r
    routes = dict(plain=plain) if a.shard_step == "plain" else dict(plain=plain, shard_0_1_labels=sharded)
    res, times = _passes(routes, a.repeats)
    rec = dict(device=torch.cuda.get_device_name(0), measured_on_gpu=True, lib_flavour=os.environ.get("TDEED_LIB_FLAVOUR", ""),
               videos=len(lengths), frames=int(off[-1]), suppress=suppress, tolerances=tols,
               routes={k: dict(_ms(v), host_syncs=stats[k]["host_syncs"], groups=stats[k]["groups"]) for k, v in times.items()},
               maps=[r[0] for r in res["plain"]])
    if a.shard_step == "one":
        rec["equal"] = bool(res["shard_0_1_labels"][0] == res["plain"])
        rec["frame_stats"] = dict(err=res["shard_0_1_labels"][1]["err"], f1_any=res["shard_0_1_labels"][1]["f1"][None])
        if a.map_tail_videos:
            rec["exchange_tail"] = _exchange_tail(a, tols)
    print(json.dumps(rec))
    return 0


def _exchange_tail(a, tols):
    """The exchange alone at the upper end: `_map_tail`'s noise tracks split over two pretend ranks by `shard_videos`, each
    with a state of its own; timed: the sums a collective would take (torch adds standing in for it), pack, unpack on both
    states -- next to the rank + AP launch of the same run."""
    nv, L, K1, hr = a.map_tail_videos, 3000, 13, 0.01
    rng = np.random.RandomState(1)
    tracks = []
    for _ in range(nv):
        x = rng.rand(L, K1).astype(np.float32)
        tracks.append(np.ascontiguousarray(x / x.sum(axis=1, keepdims=True), np.float32))
    names = [f"t{i:03d}" for i in range(nv)]
    classes = {f"c{k}": k for k in range(1, K1)}
    truth = [{"video": v, "events": [{"label": f"c{1 + (f // 20) % (K1 - 1)}", "frame": f} for f in range(7, L, 20)]} for v in names]
    entries = (("raw",), ("nms", 1, 0.10))
    table = E.truth_table(truth, {v: i for i, v in enumerate(names)}, classes)
    split = E.shard_videos([L] * nv, 2)

    def filled(own):
        state = ops.ap_state([L] * nv, table, K1, len(entries), tols, "cuda")
        mean = torch.from_numpy(np.concatenate([tracks[o] for o in own])).cuda()
        seg_off = torch.tensor(np.arange(len(own) + 1) * L, dtype=torch.int32, device="cuda")
        ords = torch.tensor(own, dtype=torch.int32, device="cuda")
        first = ops.frame_events_seg(mean, seg_off, L, hr)[2]
        for i, e in enumerate(entries):
            planes = None if e[0] == "raw" else ops.nms_track_seg(mean, seg_off, L, e[1], e[2], e[0] == "snms", first, hr,
                                                                  planes=True)[5:]
            ops.ap_match_seg(state, i, mean, seg_off, ords, L, hr, planes=planes)
        return state
    one = filled(list(range(nv)))
    states = [filled(own) for own in split]
    own_counts = [(s.ev_count.clone(), s.hit_count.clone()) for s in states]
    nbytes = [0]

    def exchange():
        counts = [ops.ap_state_counts(s, own) for s, own in zip(states, split)]
        sums = [counts[0][j] + counts[1][j] for j in range(3)]
        for c in counts:
            for j in range(3):
                c[j].copy_(sums[j])
        pays = [ops.ap_state_pack(s, own, owners=c[2]) for s, own, c in zip(states, split, counts)]
        scores, hits = pays[0][0] + pays[1][0], pays[0][1] + pays[1][1]
        for s, own in zip(states, split):
            ops.ap_state_unpack(s, own, scores, hits)
        nbytes[0] = sum(x.numel() * x.element_size() for x in sums + [scores, hits])
    t_x, t_r = [], []
    for i in range(a.repeats + 1):
        for s, (ec, hc) in zip(states, own_counts):                     # every pass starts from the ranks' own counts
            s.ev_count.copy_(ec)
            s.hit_count.copy_(hc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exchange()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ap = ops.ap_rank(states[0])[0]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i:                                                           # the first pass is the warm-up
            t_x.append(t1 - t0)
            t_r.append(t2 - t1)
    want = ops.ap_rank(one)[0]
    same = bool(torch.equal(ap, want) and torch.equal(ops.ap_rank(states[1])[0], want))
    return dict(videos=nv, frames_per_video=L, K1=K1, entries=entries, tolerances=tols, pretend_ranks=2,
                events=int(one.ev_count.sum()), hits=int(one.hit_count.sum()), exchange_bytes=nbytes[0],
                store_bytes_not_sent=int(one.ev_score.numel() * 12), exchange_both_ranks=_ms(t_x), ap_rank=_ms(t_r),
                ap_equal_to_one_rank=same,
                note="the sums between the phases are torch adds in one process, not a collective")


def _map_sharded_rank(a):
    """one rank of the sharded pass (RANK / WORLD_SIZE from the launching parent, gloo: the ranks share this box's GPU)"""
    from tdeed_amd import dist as tdist
    import torch.distributed as dist
    torch.cuda.set_device(0)
    rank, _, world = tdist.init(backend=os.environ.get("TDEED_DIST_BACKEND", "gloo"))
    m, classes, suppress, tols, lengths, off, vids, truth = _map_workload(a)
    labels = _frame_labels(truth, lengths, classes)
    names = sorted(v[0] for v in vids)
    ordinal = {v: i for i, v in enumerate(names)}
    length = {v[0]: v[1] for v in vids}
    own = set(E.shard_videos([length[v] for v in names], world)[rank])
    vids = [v if ordinal[v[0]] in own else (v[0], v[1], v[2], None) for v in vids]        # foreign sources: None
    stats = {}

    def sharded():
        dist.barrier()
        r = E.map_videos(m, vids, classes, truth, suppress, tols, labels=labels, shard="auto", batch_size=8,
                         group_videos=a.group_videos)
        stats.update(m.last_video_stats)
        return r
    res, times = _passes(dict(sharded=sharded), a.repeats)
    mine = torch.tensor([[stats["videos_own"], stats["frames"], stats["host_syncs"], stats["groups"], stats["exchange_bytes"]]],
                        dtype=torch.int64)
    every = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    if rank == 0:
        keys = ("videos_own", "frames", "host_syncs", "groups", "exchange_bytes")
        print(json.dumps(dict(world=world, backend=dist.get_backend(), rank0_pass=_ms(times["sharded"]),
                              ranks=[dict(zip(keys, x.view(-1).tolist())) for x in every], maps=[r[0] for r in res["sharded"][0]],
                              frame_stats=dict(err=res["sharded"][1]["err"], f1_any=res["sharded"][1]["f1"][None]))))
    dist.barrier()
    dist.destroy_process_group()
    return 0


def map_sharded(a):
    """`--map --ranks N`: profiles/video_map_sharded.json.  This process never touches the GPU; every step is a fresh child
    process of this script under a time limit of its own, and the first bad exit status ends the run:
      one     one rank: map_videos against map_videos(shard=(0, 1), labels=...), and the exchange alone on the noise tail
      parent  (when csrc/libtdeed_hip_parent.so exists, tools/build_ab.py parent <rev> ap.hip spot.hip) map_videos on the
              parent commit's kernels
      ranks   N ranks that share the GPU over gloo, each scoring its share: evidence that the route runs, not a speed-up"""
    if a.shard_step in ("one", "plain"):
        return _map_sharded_one(a)
    if a.shard_step == "ranks":
        return _map_sharded_rank(a)
    import socket
    import subprocess
    me = os.path.abspath(__file__)
    base = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, me, "--map", "--ranks", str(a.ranks), "--repeats",
            str(a.repeats), "--map-videos", str(a.map_videos), "--map-tail-videos", str(a.map_tail_videos), "--group-videos",
            str(a.group_videos)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}

    def line(out):
        got = [ln for ln in out.splitlines() if ln.startswith("{")]
        return json.loads(got[-1]) if got else None

    def step(name, extra_env=None):
        r = subprocess.run(base + ["--shard-step", name], env=dict(env, **(extra_env or {})), cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0 or line(r.stdout) is None:
            sys.stderr.write(f"bench_video --map --ranks: step {name} ended with status {r.returncode}\n")
            sys.exit(r.returncode or 1)
        return line(r.stdout)
    rec = dict(kind="video_map_sharded", cfg=CFG, repeats=a.repeats, group_videos=a.group_videos, batch_size=8)
    rec["one_rank"] = step("one")
    if os.path.exists(os.path.join(ROOT, "t-deed_amd", "csrc", "libtdeed_hip_parent.so")):
        rec["parent_commit_kernels"] = step("plain", dict(TDEED_LIB_FLAVOUR="parent"))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(a.ranks):
        renv = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                    HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(base + ["--shard-step", "ranks"], env=renv, cwd=ROOT, text=True,
                                      stdout=(subprocess.PIPE if r == 0 else subprocess.DEVNULL)))
    out0 = []
    import threading
    rd = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    while any(p.poll() is None for p in procs):                         # a rank that dies would leave the others waiting
        if any(p.poll() not in (None, 0) for p in procs):
            for p in procs:
                if p.poll() is None:
                    p.terminate()
        time.sleep(0.2)
    rd.join(timeout=10)
    bad = [p.returncode for p in procs if p.returncode != 0]
    if bad or line("".join(out0)) is None:
        sys.stderr.write(f"bench_video --map --ranks: the ranks ended with {[p.returncode for p in procs]}\n")
        sys.exit(bad[0] if bad else 1)
    rec["ranks"] = line("".join(out0))
    one = rec["one_rank"]["routes"]
    ref = rec.get("parent_commit_kernels", rec["one_rank"])["routes"]["plain"]
    rec["one_rank_cost"] = dict(
        reference="map_videos on the parent commit's kernels" if "parent_commit_kernels" in rec else "map_videos, this commit",
        reference_ms_median=ref["ms_median"], reference_spread_ms=round(ref["ms_max"] - ref["ms_min"], 2),
        shard_0_1_labels_ms_median=one["shard_0_1_labels"]["ms_median"], plain_ms_median=one["plain"]["ms_median"],
        within_reference_plus_spread=bool(one["shard_0_1_labels"]["ms_median"] <= ref["ms_median"] + (ref["ms_max"] - ref["ms_min"])))
    rec["sharded_equals_one_rank"] = bool(rec["ranks"]["maps"] == rec["one_rank"]["maps"]
                                          and rec["ranks"]["frame_stats"] == rec["one_rank"]["frame_stats"])
    rec["note"] = (f"{a.ranks} ranks share ONE GPU here: their pass time shows that the route runs, no speed-up is claimed or "
                   "expected; the 1 -> N curve has never been measured on multi-GPU hardware")
    out = os.path.join(ROOT, "profiles", "video_map_sharded.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return 0 if rec["sharded_equals_one_rank"] and rec["one_rank"]["equal"] else 1


def reuse(a):
    """Two routes over the same video, alternating: predict_video(batch_size=8) as it is, and with reuse_frames=True (stem and
    the blocks in front of the first gate-shift site once per frame instead of once per clip window).  Plain and augmented
    (two views), frames from pinned host memory and resident on the device.  Per setting: both times, their ratio, the
    frames that went through the per-frame stages on either route, and how far the scores are apart."""
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    T, L = CFG["clip_len"], a.frames
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    dev_video = ops.fill_u8_hash((L, 3, H, W), 9, "cuda")
    sources = dict(pinned=dev_video.cpu().pin_memory(), device=dev_video)
    eng = m._model.engine(torch.bfloat16)
    out = dict(kind="video_frame_reuse", cfg=CFG, frames=L, batch_size=8, repeats=a.repeats, frame_batch=m.frame_batch,
               first_site_block=eng.first_site_block(), settings={})
    for src, video in sources.items():
        for augment in (False, True):
            routes = dict(default=lambda: m.predict_video(video, batch_size=8, augment=augment),
                          reuse=lambda: m.predict_video(video, batch_size=8, augment=augment, reuse_frames=True))
            res, stats = {}, {}
            for k, fn in routes.items():                                # warm-up of every shape
                res[k] = fn()
                stats[k] = dict(m.last_video_stats)
            times = {k: [] for k in routes}
            for _ in range(a.repeats):
                for k, fn in routes.items():                            # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
            V, n = stats["reuse"]["views"], stats["reuse"]["clips"]
            st = {k: _stat(v, L, n * V) for k, v in times.items()}
            d = np.maximum(res["default"][1], 1)[:, None].astype(np.float32)
            out["settings"][f"{src}_{'augment' if augment else 'plain'}"] = dict(
                routes=st, ratio_reuse_over_default=round(st["reuse"]["ms_median"] / st["default"]["ms_median"], 3),
                speedup=round(st["default"]["ms_median"] / st["reuse"]["ms_median"], 3),
                views=V, clips=n, front_frames_default=V * n * T, frame_pass_frames=stats["reuse"]["frame_pass_frames"],
                map_bytes=stats["reuse"]["map_bytes"], frame_bytes=L * 3 * H * W,
                support_equal=bool(np.array_equal(res["default"][1], res["reuse"][1])),
                sums_equal=bool(np.array_equal(res["default"][0], res["reuse"][0])),
                max_abs_mean_score_diff=float(np.abs(res["default"][0] / d - res["reuse"][0] / d).max()))
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)
    return 0


def ring(a):
    """Two routes over the same host video, alternating: predict_video(batch_size=8) with the frames resident, and with
    stream_frames=True at a budget of a QUARTER of the video's bytes (the frame ring).  Upload chunks of 8 MiB on both routes
    (the default 64 MiB chunk is 445 frames: a batch of 8 clips spans 275, and a quarter of the tool's video could not hold
    a batch plus one chunk of that size).  Pinned and pageable frames, plain and augmented.  Per setting: both wall times,
    their ratio against the resident route's own spread, frames_h2d_bytes, ring_frames and whether the tracks are equal."""
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    L = a.frames
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    m.video_chunk_bytes = 8 << 20
    fb = 3 * H * W
    budget = L * fb // 4
    host = ops.fill_u8_hash((L, 3, H, W), 9, "cuda").cpu()
    sources = dict(pinned=host.pin_memory(), pageable=host)
    out = dict(kind="video_ring", device=torch.cuda.get_device_name(0), measured_on_gpu=True, cfg=CFG, frames=L, batch_size=8,
               repeats=a.repeats, video_bytes=L * fb, max_resident_bytes=budget, video_chunk_bytes=m.video_chunk_bytes,
               settings={})
    for src, video in sources.items():
        for augment in (False, True):
            routes = dict(resident=lambda: m.predict_video(video, batch_size=8, augment=augment),
                          ring=lambda: m.predict_video(video, batch_size=8, augment=augment, max_resident_bytes=budget,
                                                       stream_frames=True))
            res, stats = {}, {}
            for k, fn in routes.items():                                # warm-up of every shape
                res[k] = fn()
                stats[k] = dict(m.last_video_stats)
            times = {k: [] for k in routes}
            for _ in range(a.repeats):
                for k, fn in routes.items():                            # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    times[k].append(time.perf_counter() - t0)
            V, n = stats["ring"]["views"], stats["ring"]["clips"]
            st = {k: _stat(v, L, n * V) for k, v in times.items()}
            spread = st["resident"]["ms_max"] - st["resident"]["ms_min"]
            out["settings"][f"{src}_{'augment' if augment else 'plain'}"] = dict(
                routes=st, ratio_ring_over_resident=round(st["ring"]["ms_median"] / st["resident"]["ms_median"], 3),
                resident_spread_ms=round(spread, 2),
                ring_within_resident_spread=bool(st["ring"]["ms_median"] <= st["resident"]["ms_median"] + spread),
                frames_h2d_bytes={k: stats[k]["frames_h2d_bytes"] for k in stats}, ring_frames=stats["ring"]["ring_frames"],
                ring_chunks=stats["ring"]["ring_chunks"], resident_bytes=stats["ring"]["resident_bytes"],
                tracks_equal=bool(np.array_equal(res["resident"][0], res["ring"][0])
                                  and np.array_equal(res["resident"][1], res["ring"][1])))
    path = os.path.join(ROOT, "profiles", "video_ring.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0 if all(s["tracks_equal"] for s in out["settings"].values()) else 1


def gather_only(a):
    T, B, L = 100, 8, 400
    video = ops.fill_u8_hash((L, 3, H, W), 9, "cuda")
    sd = torch.tensor([-5, 20, 45, 70, 95, 120, 145, 170], dtype=torch.int32, device="cuda")
    out = torch.empty((B * T, 3, H, W), dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(5):
        ops.clip_gather(video, sd, T, out)
    ev[0].record()
    for _ in range(a.repeats * 10):
        ops.clip_gather(video, sd, T, out)
    ev[1].record()
    torch.cuda.synchronize()
    us = ev[0].elapsed_time(ev[1]) * 1e3 / (a.repeats * 10)
    moved = 2 * B * T * 3 * H * W
    print(json.dumps(dict(kind="clip_gather", B=B, T=T, frame_bytes=3 * H * W, us_per_launch_events=round(us, 2),
                          bytes_moved=moved, bound_us_at_copy_bandwidth=round(moved / (COPY_GBPS * 1e3), 2),
                          copy_bandwidth_GBps=COPY_GBPS)))
    return 0


def decode(a):
    """host only, measured on whichever host runs it: every sampled frame once (load_video) against the clip reader at 3/4
    overlap (clip_batches), same JPEG tree, same thread pool"""
    import tempfile
    from PIL import Image
    n, T = a.decode_frames, 100
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "vid")
        os.makedirs(d)
        for i in range(n):
            Image.fromarray(synth.uint8_clip(700 + i % 16, (H, W, 3))).save(os.path.join(d, f"frame{i}.jpg"), quality=92)
        pool = feeder.DecodePool(a.threads)
        t0 = time.perf_counter()
        feeder.load_video(tmp, "soccernetball", "vid", n, pool=pool)
        t_video = time.perf_counter() - t0
        starts = [s for s in E.video_clip_starts(n, T, 75) if s + T > 0]
        descs = [dict(paths=feeder.load_paths(tmp, "soccernetball", "vid", s, s + T)) for s in starts]
        t0 = time.perf_counter()
        nb = sum(1 for _ in feeder.clip_batches(descs, 1, (3, H, W), T, pool=pool))
        t_clips = time.perf_counter() - t0
        pool.close()
    print(json.dumps(dict(kind="video_decode_host_only", frames=n, clips=nb, threads=pool.threads,
                          load_video_frames_per_s=round(n / t_video, 1), load_video_s=round(t_video, 3),
                          clip_batches_video_frames_per_s=round(n / t_clips, 1), clip_batches_s=round(t_clips, 3),
                          ratio=round(t_clips / t_video, 2))))
    return 0


def decode_device(a):
    """JPEG decode of one video, three routes in one process, alternating, `--repeats` timed passes after a warm-up each:
    load_video with a DecodePool of 8 threads, load_video with a ProcessDecodePool of 16 workers (both into page-locked
    host memory, which is where those routes end), load_video_device (ends with the frames on the device).  Then the two
    kernels alone (HIP events) and the host's share of the device route alone (file reads, parse, pack)."""
    import tempfile
    from PIL import Image
    from tdeed_amd import jpegdev
    n = a.decode_frames
    dev = torch.device("cuda")

    def rate(times):
        t = np.asarray(times)
        return dict(frames_per_s=round(n / float(np.median(t)), 1), frames_per_s_min=round(n / float(t.max()), 1),
                    frames_per_s_max=round(n / float(t.min()), 1), ms_median=round(float(np.median(t)) * 1e3, 2))

    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "vid")
        os.makedirs(d)
        for i in range(n):
            Image.fromarray(synth.uint8_clip(700 + i % 16, (H, W, 3))).save(os.path.join(d, f"frame{i}.jpg"), quality=90)
        names = [os.path.join(d, f"frame{i}.jpg") for i in range(n)]
        file_bytes = sum(os.path.getsize(p) for p in names)
        tpool, ppool = feeder.DecodePool(8), feeder.ProcessDecodePool(16)
        try:
            slot = ppool.make_slots(1, (n, 3, H, W))[0]
            pinned = torch.zeros((n, 3, H, W), dtype=torch.uint8).pin_memory()
            dbuf = torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev)
            routes = dict(
                host_threads_8=lambda: feeder.load_video(tmp, "soccernetball", "vid", n, out=pinned, pool=tpool),
                host_processes_16=lambda: feeder.load_video(tmp, "soccernetball", "vid", n, out=slot, pool=ppool),
                device=lambda: feeder.load_video_device(tmp, "soccernetball", "vid", n, out=dbuf, pool=tpool))
            for fn in routes.values():
                fn()
            torch.cuda.synchronize()
            want = pinned.clone()
            same = bool(torch.equal(dbuf.cpu(), want)) and bool(torch.equal(slot, want))
            stats = dict(feeder.last_decode_stats)
            times = {k: [] for k in routes}
            for _ in range(a.repeats):
                for k, fn in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            # the host's share of the device route
            host_t = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                pk = jpegdev.pack([feeder._read_file(p) for p in names])
                host_t.append(time.perf_counter() - t0)
            # the kernels alone
            fc = ops.jpeg_frame_coeffs(W, H, pk.samp)
            dj = feeder.DeviceJpegs(pk, dev, n)
            dj.stream_through(pk.stream_np.size)
            (lo, hi, waves), = dj.chunks
            coeff = torch.zeros(n * fc, dtype=torch.int16, device=dev)
            k_ent, k_pix = [], []
            for it in range(a.repeats + 1):
                coeff.zero_()
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                ops.jpeg_entropy(dj.stream, dj.segments, waves, dj.table_sets, W, H, pk.samp, 0, n, coeff, dj.status)
                e[1].record()
                ops.jpeg_pixels(coeff, dj.frame_set, dj.table_sets, dbuf, 0, n, pk.samp)
                e[2].record()
                torch.cuda.synchronize()
                if it:
                    k_ent.append(e[0].elapsed_time(e[1]) * 1e-3)
                    k_pix.append(e[1].elapsed_time(e[2]) * 1e-3)
        finally:
            tpool.close()
            ppool.close()
    r = {k: rate(v) for k, v in times.items()}
    rec = dict(kind="jpeg_device_decode", device=torch.cuda.get_device_name(0), measured_on_gpu=True, frames=n,
               frame="224x224 4:2:0 quality 90, the tool's hash-noise frames (16 distinct)", repeats=a.repeats,
               identical_to_load_video=same, routes=r,
               ratio_device_over_host_threads_8=round(r["device"]["frames_per_s"] / r["host_threads_8"]["frames_per_s"], 2),
               ratio_device_over_host_processes_16=round(r["device"]["frames_per_s"] / r["host_processes_16"]["frames_per_s"], 2),
               entropy_kernel=rate(k_ent), pixels_kernel=rate(k_pix), host_read_parse_pack=rate(host_t),
               pcie_bytes_per_frame=dict(host_routes=3 * H * W, device=round(stats["stream_bytes"] / n, 1)),
               jpeg_file_bytes_per_frame=round(file_bytes / n, 1), last_decode_stats=stats)
    out = os.path.join(ROOT, "profiles", "jpeg_device_decode.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return 0


def _write_jpeg_set(tmp, lengths, FH, FW, K):
    """The synthetic validation set of the resident-JPEG modes: videos of `lengths` frames cycling 16 distinct pictures (a
    colour ramp, a wave and low noise), quality 90, 4:2:0 -> (video dicts, truth lists, bytes of all files)"""
    from PIL import Image
    yy, xx = np.mgrid[0:FH, 0:FW].astype(np.float64)
    pics = []
    for k in range(16):
        base = np.stack([30 + 180 * xx / (FW - 1), 40 + 170 * yy / (FH - 1), 128 + 90 * np.sin(0.11 * xx + k) * np.cos(0.07 * yy)], -1)
        noise = synth.uint8_clip(700 + k, (FH, FW, 3)).astype(np.float64) / 10.0 - 12.75
        pics.append(Image.fromarray(np.clip(base + noise, 0, 255).astype(np.uint8)))
    videos, file_bytes = [], 0
    for v, L in enumerate(lengths):
        d = os.path.join(tmp, f"v{v:03d}")
        os.makedirs(d)
        for i in range(L):
            pics[(i + 3 * v) % 16].save(os.path.join(d, f"frame{i}.jpg"), "JPEG", quality=90, subsampling=2)
            file_bytes += os.path.getsize(os.path.join(d, f"frame{i}.jpg"))
        videos.append(dict(video=f"v{v:03d}", num_frames=L, fps=25.0))
    truth = [{"video": v["video"], "events": [{"label": f"c{1 + (f // 20) % K}", "frame": f} for f in range(7, v["num_frames"], 20)]}
             for v in videos]
    return videos, truth, file_bytes


def streamed_jpeg(a):
    """--resident-jpeg --stream-clips F [F ...]: the validation pass of `resident_jpeg` fed by `evalutil.ResidentJpegVideos(
    stream_videos=True)` at max_resident_bytes = F x the all-resident bytes of the set ("min": the plan's smallest budget,
    every video streamed; a fraction below it is raised to it), against the all-resident object (fraction 1.0, the keyword off)
    and decode="host", in one process, the routes alternating: a warm-up pass per route, then `--repeats` timed passes (at
    least three), every pass listed.  Per setting what stays where, and the entropy kernel alone on the long video.  A route is
    called faster than another only when it is faster in every timed pass.  Written to profiles/video_streamed_jpeg.json."""
    import tempfile
    from types import SimpleNamespace
    from tdeed_amd.model import TDEEDModel
    from tdeed_amd import trainclips as TC
    FH, FW = 224, 398
    repeats = max(int(a.repeats), 3)
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    K = CFG["num_classes"]
    classes = {f"c{k}": k for k in range(1, K + 1)}
    suppress = (("nms", 1, 0.10), ("snms", 3, 0.01))
    tols = [0, 1, 2, 4]
    lengths = group_lengths("diving")[:a.map_videos] + [a.frames]
    n_frames = int(sum(lengths))
    kw = dict(batch_size=8, group_videos=min(a.group_videos, 8))
    coeff = a.coeff_mib << 20
    with tempfile.TemporaryDirectory() as tmp:
        videos, truth, file_bytes = _write_jpeg_set(tmp, lengths, FH, FW, K)
        tpool = feeder.DecodePool(a.threads)
        try:
            files = [(v["video"], v["num_frames"], v["fps"],
                      dict(frame_dir=tmp, dataset="soccernetball", video_name=v["video"], num_frames=v["num_frames"], pool=tpool))
                     for v in videos]
            jpegs = TC.load_resident_jpegs(tmp, "soccernetball", videos, pool=tpool, shard_bytes=a.shard_mib << 20)
            made = dict(resident_all=E.ResidentJpegVideos(videos, jpegs, max_coeff_bytes=coeff))
            whole = made["resident_all"].stats["resident_bytes"]
            low = E.ResidentJpegVideos(videos, jpegs, max_coeff_bytes=coeff, stream_videos=True)._plan.min_budget
            settings = dict(resident_all=dict(budget_fraction=1.0, resident_bytes=whole))
            for f in a.stream_clips:
                want = low if f == "min" else int(float(f) * whole)
                rv = E.ResidentJpegVideos(videos, jpegs, max_coeff_bytes=coeff, stream_videos=True, max_resident_bytes=max(want, low))
                made[f"streamed_{f}"] = rv
                settings[f"streamed_{f}"] = dict(budget_fraction=f, asked_bytes=want, max_resident_bytes=max(want, low),
                                                 smallest_budget=low, raised_to_smallest=bool(want < low), chunk_frames=rv._chunk,
                                                 **{k: rv.stats[k] for k in ("resident_bytes", "resident_videos", "streamed_videos",
                                                                             "stage_bytes", "host_stream_bytes", "stream_bytes")})
            routes = dict(a_decode_host=lambda: E.map_videos(m, files, classes, truth, suppress, tols, decode="host", **kw))
            for k, rv in made.items():
                routes[k] = lambda rv=rv: E.map_videos(m, rv.sources(), classes, truth, suppress, tols, **kw)
            res, first = {}, {}
            for k, fn in routes.items():                                    # warm-up: plans, graphs, table caches
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[k] = fn()
                torch.cuda.synchronize()
                first[k] = round((time.perf_counter() - t0) * 1e3, 1)
            times = {k: [] for k in routes}
            for _ in range(repeats):
                for k, fn in routes.items():                                # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            kernels = {}
            for key, rv in made.items():                                    # the entropy kernel alone, on the long video
                rv._kernel_events = []
                for _ in range(repeats + 1):
                    rv.frames(len(lengths) - 1)
                ev, rv._kernel_events = rv._kernel_events, None
                per = len(ev) // (repeats + 1)
                copies = rv._tabs[len(lengths) - 1][5]
                kernels[key] = dict(frames=lengths[-1], chunks=per, copied_bytes=int(sum(hi - lo for c in copies.values() for _, lo, hi, _ in c)),
                                    entropy_items_ms=[round(sum(e0.elapsed_time(e1) for e0, e1, _ in ev[i * per:(i + 1) * per]), 3)
                                                      for i in range(1, repeats + 1)])
        finally:
            tpool.close()
    same = {k: bool(res[k] == res["a_decode_host"]) for k in routes}
    rt = {}
    for k, v in times.items():
        tt = np.asarray(v) * 1e3
        rt[k] = dict(first_pass_ms=first[k], passes_ms=[round(float(x), 1) for x in tt], ms_min=round(float(tt.min()), 1),
                     ms_max=round(float(tt.max()), 1), ms_median=round(float(np.median(tt)), 1),
                     frames_per_s_median=round(n_frames / float(np.median(tt)) * 1e3, 1))
    verdicts = {}
    for new in made:
        for old in routes:
            if new != old and not (old in made and new == "resident_all"):
                x, y = np.asarray(times[new]), np.asarray(times[old])
                every = bool(np.all(x < y))
                verdicts[f"{new}_vs_{old}"] = dict(
                    faster_in_every_timed_pass=every, ratio_of_medians_old_over_new=round(float(np.median(y) / np.median(x)), 3),
                    note=("faster in every timed pass" if every else "slower in every timed pass" if bool(np.all(x > y)) else
                          "the ranges overlap or the order changes between passes: no claim"))
    rec = dict(kind="video_streamed_jpeg", device=torch.cuda.get_device_name(0), measured_on_gpu=True, cfg=CFG, videos=len(lengths),
               frames=n_frames, longest_video=lengths[-1], frame="224x398 4:2:0 quality 90, 16 distinct pictures (ramp + wave + low "
               "noise)", jpeg_file_bytes_per_frame=round(file_bytes / n_frames, 1), threads=tpool.threads, group_videos=kw["group_videos"],
               batch_size=8, repeats=repeats, max_coeff_bytes=coeff, shard_bytes=a.shard_mib << 20, settings=settings, routes=rt,
               maps_equal_route_a=same, verdicts=verdicts, kernels_alone_long_video=kernels)
    out = os.path.join(ROOT, "profiles", "video_streamed_jpeg.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    assert all(same.values()), f"the routes' mAP tables differ: {same}"
    return 0


def resident_jpeg(a):
    """A validation pass (`evalutil.map_videos`) over the tool's synthetic set -- `--map-videos` short videos of the diving
    split plus one of `--frames` frames, 224 x 398 4:2:0 JPEG files, the model cropping the centre 224 x 224 -- fed four ways,
    in one process, the routes alternating: (a) decode="host" with the tool's thread pool, (b) decode="device"
    (`feeder.load_video_device`: files read, parsed, packed and uploaded every pass), (c) `evalutil.ResidentJpegVideos`, (d) the
    same with crop=224 (windowed pixel pass, cropped frames).  A warm-up pass per route (reported as first_pass), then
    `--repeats` timed passes (at least three), every pass listed.  Construction of (c) and (d) is timed apart.  Then the
    entropy and the pixel kernel alone on the long video (HIP events), window against full, and the byte figures.  A route
    is called faster than another only when it is faster in every timed pass; otherwise the ranges are given."""
    import tempfile
    from types import SimpleNamespace
    from tdeed_amd.model import TDEEDModel
    from tdeed_amd import trainclips as TC
    FH, FW = 224, 398
    repeats = max(int(a.repeats), 3)
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    K = CFG["num_classes"]
    classes = {f"c{k}": k for k in range(1, K + 1)}
    suppress = (("nms", 1, 0.10), ("snms", 3, 0.01))
    tols = [0, 1, 2, 4]
    lengths = group_lengths("diving")[:a.map_videos] + [a.frames]
    n_frames = int(sum(lengths))
    budget = 16 << 30
    kw = dict(batch_size=8, group_videos=min(a.group_videos, 8))          # groups of 8: the next group decodes meanwhile
    with tempfile.TemporaryDirectory() as tmp:
        videos, truth, file_bytes = _write_jpeg_set(tmp, lengths, FH, FW, K)
        tpool = feeder.DecodePool(a.threads)
        try:
            files = [(v["video"], v["num_frames"], v["fps"],
                      dict(frame_dir=tmp, dataset="soccernetball", video_name=v["video"], num_frames=v["num_frames"], pool=tpool))
                     for v in videos]
            built, made = {}, {}
            for key, crop in (("c_resident_jpeg", None), ("d_resident_jpeg_crop", 224)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jpegs = TC.load_resident_jpegs(tmp, "soccernetball", videos, pool=tpool)
                t1 = time.perf_counter()
                made[key] = E.ResidentJpegVideos(videos, jpegs, crop=crop, max_resident_bytes=budget)
                torch.cuda.synchronize()
                built[key] = dict(read_parse_pack_ms=round((t1 - t0) * 1e3, 1), upload_index_ms=round((time.perf_counter() - t1) * 1e3, 1))
                del jpegs
            routes = dict(
                a_decode_host=lambda: E.map_videos(m, files, classes, truth, suppress, tols, decode="host", **kw),
                b_decode_device=lambda: E.map_videos(m, files, classes, truth, suppress, tols, decode="device", **kw),
                c_resident_jpeg=lambda: E.map_videos(m, made["c_resident_jpeg"].sources(), classes, truth, suppress, tols, **kw),
                d_resident_jpeg_crop=lambda: E.map_videos(m, made["d_resident_jpeg_crop"].sources(), classes, truth, suppress, tols, **kw))
            res, first, syncs = {}, {}, {}
            for k, fn in routes.items():                                    # warm-up: plans, graphs, table caches
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[k] = fn()
                torch.cuda.synchronize()
                first[k] = round((time.perf_counter() - t0) * 1e3, 1)
                syncs[k] = m.last_video_stats.get("host_syncs")
            times = {k: [] for k in routes}
            for _ in range(repeats):
                for k, fn in routes.items():                                # alternating
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            # the kernels alone, on the long video
            kernels = {}
            for key, rv in made.items():
                rv._kernel_events = []
                for _ in range(repeats + 1):
                    rv.frames(len(lengths) - 1)
                ev, rv._kernel_events = rv._kernel_events, None
                per = len(ev) // (repeats + 1)
                ent = [sum(e0.elapsed_time(e1) for e0, e1, _ in ev[i * per:(i + 1) * per]) for i in range(1, repeats + 1)]
                pix = [sum(e1.elapsed_time(e2) for _, e1, e2 in ev[i * per:(i + 1) * per]) for i in range(1, repeats + 1)]
                kernels[key] = dict(frames=lengths[-1], chunks=per, items=int(rv.video_tables(len(lengths) - 1).items.shape[0]),
                                    entropy_items_ms=[round(x, 3) for x in ent], pixels_ms=[round(x, 3) for x in pix])
            stats = {k: {f: (list(x) if isinstance(x, tuple) else x) for f, x in rv.stats.items() if f != "index_flagged"}
                     for k, rv in made.items()}
        finally:
            tpool.close()
    same = {k: bool(res[k] == res["a_decode_host"]) for k in routes}
    rt = {}
    for k, v in times.items():
        tt = np.asarray(v) * 1e3
        rt[k] = dict(first_pass_ms=first[k], passes_ms=[round(float(x), 1) for x in tt], ms_min=round(float(tt.min()), 1),
                     ms_max=round(float(tt.max()), 1), ms_median=round(float(np.median(tt)), 1),
                     frames_per_s_median=round(n_frames / float(np.median(tt)) * 1e3, 1), host_syncs_of_the_consumer=syncs[k])
    verdicts = {}
    for new, old in (("c_resident_jpeg", "a_decode_host"), ("c_resident_jpeg", "b_decode_device"),
                     ("d_resident_jpeg_crop", "a_decode_host"), ("d_resident_jpeg_crop", "b_decode_device"),
                     ("d_resident_jpeg_crop", "c_resident_jpeg")):
        x, y = np.asarray(times[new]), np.asarray(times[old])
        every = bool(np.all(x < y))
        verdicts[f"{new}_vs_{old}"] = dict(
            faster_in_every_timed_pass=every, ratio_of_medians_old_over_new=round(float(np.median(y) / np.median(x)), 3),
            note=("faster in every timed pass" if every else "slower in every timed pass" if bool(np.all(x > y)) else
                  "the ranges overlap or the order changes between passes: no claim"))
    st_c, st_d = stats["c_resident_jpeg"], stats["d_resident_jpeg_crop"]
    full_b, win_b = 3 * FH * FW, 3 * 224 * 224
    comp = st_c["resident_bytes"] / st_c["frames"]
    rec = dict(kind="video_resident_jpeg", device=torch.cuda.get_device_name(0), measured_on_gpu=True, cfg=CFG,
               videos=len(lengths), frames=n_frames, longest_video=lengths[-1], frame="224x398 4:2:0 quality 90, 16 distinct pictures "
               "(ramp + wave + low noise)", jpeg_file_bytes_per_frame=round(file_bytes / n_frames, 1), threads=tpool.threads,
               group_videos=kw["group_videos"], batch_size=8, repeats=repeats, routes=rt, construction=built,
               maps_equal_route_a=same, verdicts=verdicts, kernels_alone_long_video=kernels,
               bytes_per_frame=dict(resident_compressed=round(comp, 1), decoded_full=full_b, decoded_window=win_b,
                                    window_over_full=round(win_b / full_b, 4)),
               frames_that_fit_max_resident_bytes=dict(max_resident_bytes=budget, decoded_full=budget // full_b,
                                                       decoded_window=budget // win_b, compressed=int(budget // comp)),
               stats=stats)
    out = os.path.join(ROOT, "profiles", "video_resident_jpeg.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    assert all(same.values()), f"the routes' mAP tables differ: {same}"
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=None, help="default 2030, with --spot 5625")
    ap.add_argument("--spot", action="store_true")
    ap.add_argument("--group", action="store_true")
    ap.add_argument("--map", action="store_true", help="spot_videos + mean_average_precisions against map_videos")
    ap.add_argument("--map-videos", type=int, default=24, help="--map: videos of the synthetic diving split")
    ap.add_argument("--map-tail-videos", type=int, default=40, help="--map: noise tracks of the tail-only measurement (0: skip it)")
    ap.add_argument("--ranks", type=int, default=0,
                    help="--map: the pass sharded over this many ranks, self-launched as child processes that share the GPU "
                         "(profiles/video_map_sharded.json)")
    ap.add_argument("--shard-step", default=None, choices=["one", "plain", "ranks"], help="--map --ranks: set by the launching parent")
    ap.add_argument("--step-timeout", type=int, default=420, help="--map --ranks: seconds every child step may take")
    ap.add_argument("--reuse", action="store_true", help="predict_video against predict_video(reuse_frames=True)")
    ap.add_argument("--ring", action="store_true", help="predict_video resident against the frame ring (stream_frames=True)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_frame_reuse.json"), help="--reuse: where the JSON goes")
    ap.add_argument("--group-videos", type=int, default=32, help="--group: videos per packed group of route B")
    ap.add_argument("--splits", default="diving,tennis", help="--group: synthetic splits to run")
    ap.add_argument("--window", type=int, default=12, help="--spot: NMS / soft-NMS window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--decode-device", action="store_true", help="JPEG decode: two host routes against load_video_device")
    ap.add_argument("--decode-frames", type=int, default=400)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--resident-jpeg", action="store_true",
                    help="map_videos fed by host decode, device decode and ResidentJpegVideos (with and without crop)")
    ap.add_argument("--stream-clips", nargs="+", default=None, metavar="BUDGET_FRACTION",
                    help="with --resident-jpeg: ResidentJpegVideos(stream_videos=True) at these fractions of the all-resident bytes "
                         "('min': the smallest budget) against the all-resident object and host decode (profiles/video_streamed_jpeg.json)")
    ap.add_argument("--shard-mib", type=int, default=4, help="--stream-clips: shard_bytes of load_resident_jpegs, in MiB")
    ap.add_argument("--coeff-mib", type=int, default=128, help="--stream-clips: max_coeff_bytes, in MiB (its frame chunks are the staging region)")
    a = ap.parse_args()
    if a.frames is None:
        a.frames = 5625 if a.spot else 2030
    sys.exit(streamed_jpeg(a) if a.resident_jpeg and a.stream_clips else resident_jpeg(a) if a.resident_jpeg else ring(a) if a.ring else map_sharded(a) if a.map and a.ranks else map_bench(a) if a.map else decode_device(a) if a.decode_device else decode(a) if a.decode else gather_only(a) if a.gather_only else reuse(a) if a.reuse else group(a) if a.group
             else spot(a) if a.spot else bench(a))
