"""Live scoring against predict_video, in ONE process, the routes alternating -> profiles/live_scoring.json.

    python tools/bench_live.py [--frames 2030] [--push 25] [--rounds 3] [--out profiles/live_scoring.json]

RegNetY-200MF, T = 100 (overlap 75, pad 5), 224 x 398 noise frames of which the model crops the centre 224 x 224, bf16, frames
in pinned host memory.  One warm-up pass of every route (plans, graphs), then `--rounds` timed rounds; median and range.
  (a) replay throughput: `live_scorer(batch_size=b)` fed pushes of `--push` frames as fast as they are accepted, then close(),
      against `predict_video(batch_size=b)` on the same frames, b = 1 and 8; the tracks are compared bit for bit.
  (b) latency: wall time of every push that completes a batch, from the call to the rows on the host (same passes as (a)),
      and of the pushes that complete none (staging and queueing only).
  (c) the stitch alone: all `ops.stitch_live` launches of one video (b = 8, random scores) next to one
      `ops.stitch_scores_seg` launch over the whole clip list.
Needs the GPU: nothing here falls back."""
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
from tdeed_amd import synth, state_layout, ops  # noqa: E402
from tdeed_amd import evalutil as E  # noqa: E402
from tdeed_amd import liveplan as LP  # noqa: E402

CFG = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4, num_classes=4,
           radi_displacement=2)
H, W = 224, 398


def _ms(v):
    tt = np.asarray(v, np.float64) * 1e3
    return dict(ms_median=round(float(np.median(tt)), 3), ms_min=round(float(tt.min()), 3), ms_max=round(float(tt.max()), 3),
                n=int(tt.size))


def _noise_video(L):
    video = torch.empty((L, 3, H, W), dtype=torch.uint8).pin_memory()
    for lo in range(0, L, 256):                                         # generated on the device in pieces
        hi = min(lo + 256, L)
        video[lo:hi].copy_(ops.fill_u8_hash((hi - lo, 3, H, W), 9 + lo, "cuda"))
    return video


def _replay(sc, video, push):
    """one pass of the live route -> (sums, support, seconds per push that completed a batch, per push that did not)"""
    sc.reset()
    parts, with_batch, without = [], [], []
    for lo in range(0, video.shape[0], push):
        t0 = time.perf_counter()
        _, sums, sup, _ = sc.push(video[lo:lo + push])
        (with_batch if sc.last_push_stats["batches"] else without).append(time.perf_counter() - t0)
        parts.append((sums, sup))
    _, sums, sup, _ = sc.close()
    parts.append((sums, sup))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), with_batch, without


def throughput_and_latency(a, m, video):
    L, T = a.frames, CFG["clip_len"]
    out = {}
    for bs in (1, 8):
        sc = m.live_scorer((3, H, W), batch_size=bs)
        routes = dict(predict_video=lambda: m.predict_video(video, batch_size=bs) + ([], []),
                      live=lambda: _replay(sc, video, a.push))
        res = {k: fn() for k, fn in routes.items()}                     # warm-up of every shape
        times = {k: [] for k in routes}
        lat, idle = [], []
        for _ in range(a.rounds):
            for k, fn in routes.items():                                # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                times[k].append(time.perf_counter() - t0)
                lat += r[2]
                idle += r[3]
        n = LP.close_clips(L, T, sc.overlap_len, sc.pad_len)
        st = {k: dict(_ms(v), frames_per_s=round(L / float(np.median(v)), 1), clips_per_s=round(n / float(np.median(v)), 1))
              for k, v in times.items()}
        out[f"batch_size_{bs}"] = dict(
            routes=st, clips=n, pushes=-(-L // a.push), ring_frames=sc.ring_frames, track_rows=sc.track_rows,
            latency_frames_bound=sc.latency_frames,
            ratio_live_over_predict_video=round(st["live"]["ms_median"] / st["predict_video"]["ms_median"], 3),
            push_completing_a_batch=_ms(lat), push_completing_none=_ms(idle),
            sums_equal=bool(np.array_equal(res["live"][0].view(np.uint32), res["predict_video"][0].view(np.uint32))),
            support_equal=bool(np.array_equal(res["live"][1], res["predict_video"][1])))
    return out


def stitch_alone(a, K1=5, bs=8, inner=20):
    L, T = a.frames, CFG["clip_len"]
    ov, pad = T // 4 * 3, 5
    starts = E.video_clip_starts(L, T, ov, pad_len=pad)
    n = len(starts)
    scores = torch.randn((1, n, T, K1), device="cuda")
    sd = torch.tensor(starts, dtype=torch.int32, device="cuda")
    seg, coff = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in ([0, L], [0, n]))
    sched = LP.LiveSchedule(T, ov, pad, bs)
    launches = sched.push(L) + sched.close()
    batches = [(scores[:, x["first"]:x["first"] + len(x["starts"])].contiguous() if x["starts"] else None,
                sd[x["first"]:x["first"] + len(x["starts"])] if x["starts"] else None, x) for x in launches]
    R = LP.track_ring_rows(bs, T, ov)
    ring_sum = torch.zeros((R, K1), dtype=torch.float32, device="cuda")
    ring_sup = torch.zeros((R,), dtype=torch.int32, device="cuda")
    out = (torch.empty((L, K1), dtype=torch.float32, device="cuda"), torch.empty((L,), dtype=torch.int32, device="cuda"),
           torch.empty((L, K1), dtype=torch.float32, device="cuda"))

    def live():
        for sc_, sd_, x in batches:
            ops.stitch_live(ring_sum, ring_sup, sc_, sd_, False, x["lo"], x["final_hi"], x["limit"], T=T,
                            out=tuple(o[x["lo"]:x["final_hi"]] for o in out))
        return out

    def whole():
        return ops.stitch_scores_seg(scores, sd, seg, coff, L, count_all=False, mean=True)
    routes = dict(stitch_live_all_launches=live, stitch_scores_seg_one_launch=whole)
    res = {k: [x.clone() for x in fn()] for k, fn in routes.items()}    # warm-up
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, fn in routes.items():                                    # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / inner)
    equal = all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
                for x, y in zip(res["stitch_live_all_launches"], res["stitch_scores_seg_one_launch"]))
    return dict(frames=L, clips=n, K1=K1, batch_size=bs, ring_rows=R, launches=len(batches), passes_per_timing=inner,
                note="host clock around `passes_per_timing` passes ending in a device synchronise: launch overhead included",
                routes={k: _ms(v) for k, v in times.items()}, equal=equal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2030)
    ap.add_argument("--push", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_scoring.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_live: needs the MI355X (no CPU fallback)")
    from tdeed_amd.model import TDEEDModel
    from types import SimpleNamespace
    m = TDEEDModel(device="cuda", args=SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **CFG))
    m.load({k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 0).items()})
    video = _noise_video(a.frames)
    rec = dict(kind="live_scoring", device=torch.cuda.get_device_name(0), measured_on_gpu=True, cfg=CFG, frames=a.frames,
               frame="224x398 noise, centre 224x224 cropped by the model", push_frames=a.push, rounds=a.rounds,
               video_chunk_bytes=m.video_chunk_bytes)
    rec["replay"] = throughput_and_latency(a, m, video)
    rec["stitch_alone"] = stitch_alone(a)
    ok = rec["stitch_alone"]["equal"] and all(v["sums_equal"] and v["support_equal"] for v in rec["replay"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
