"""GPU tool: what the frozen eval-mode prefix (`frozen_stats='eval'`) does to the training step -> profiles/frozen_eval_prefix.json.
    python tools/bench_frozen_eval.py --part a|b|c [--out FILE] [--steps N] [--reps N]
    python tools/bench_frozen_eval.py --merge PART.json [PART.json ...] [--out FILE]

a. The captured bf16 step (TrainEngine.make_step: graph + optimizer launch), T = 100, 224 x 224, 200MF B = 8 and 800MF
   B = 16, with stem + s1 + s2 frozen and with `_features.*` frozen: 'batch' (the baseline: unchanged code) against 'eval'.
b. The default step -- no groups, and the two 'batch' steps -- of the library this process loads.  Run it once per library
   flavour (TDEED_LIB_FLAVOUR: the release build, and the parent commit's kernels from tools/build_ab.py), the processes
   alternating, and --merge the parts: the rounds of a flavour are pooled over its processes.
c. The stem alone on 1 600 fp32 frames of 224 x 224 with per-frame flips: tdeed_stem_mfma_eval_fwd against tdeed_stem_fwd
   (bf16 output).
Device events, inside one process the routes alternate in every round, one warm-up round and three timed ones, median and
range (tools/bench_guarded_step.py).  Compare the routes of one run with each other, never with a number from another run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import bench  # noqa: E402
from bench_guarded_step import ROUNDS, alternate, overlap  # noqa: E402
from tdeed_amd import _lib, ops, state_layout, synth  # noqa: E402

FRONT = [{"params": ("_features.stem.*", "_features.s1.*", "_features.s2.*"), "frozen": True}]
TRUNK = [{"params": ("_features.*",), "frozen": True}]
WORKLOADS = (("200MF_B8", "rny002_b8"), ("800MF_B16", "rny008_b16"))


def verdict(route, base, what):
    if overlap(route, base):
        return f"ranges overlap, neither is called faster ({what})"
    return ("faster in every round" if route["max_ms"] < base["min_ms"] else "slower in every round") + f" ({what})"


def _step_routes(workload, variants, steps):
    """variants: name -> (groups, frozen_stats | None = the keyword is not passed).  -> alternate()'s result with the launch
    counts of one eager step of each."""
    from tdeed_amd.regnet_spec import regnet_spec
    from tdeed_amd.trainer import TrainEngine
    wl = bench.CONFIGS[workload]
    cfg, B, H, W = wl["cfg"], wl["B"], wl["H"], wl["W"]
    T, dev, dt = cfg["clip_len"], "cuda", torch.bfloat16
    frames = ops.fill_u8_hash((B, T, 3, H, W), 1000, dev)
    lab_np, labD_np = synth.labels(5, B, T, cfg["num_classes"], max(cfg["radi_displacement"], 1))
    lab = torch.from_numpy(lab_np).to(dev)
    labD = torch.from_numpy(labD_np).float().to(dev) if cfg["radi_displacement"] else None
    C = regnet_spec(cfg["feature_arch"]).feat_dim
    masks = [((torch.rand((B, T, C), device=dev) >= 0.5).to(dt) * 2.0) for _ in range(2 if cfg["radi_displacement"] else 1)]
    routes, info, keep = {}, {}, []
    for name, (groups, stats) in variants.items():
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 0).items()}
        eng = TrainEngine(cfg, sd, dt, dev, lr=1e-4)
        if stats is None:
            eng.set_groups(groups)
        else:
            eng.set_groups(groups, frozen_stats=stats)
        with _lib.profile() as prof:               # the launches of one eager step, counted (not timed)
            eng.step(frames, lab, labD, drop_masks=masks)
        torch.cuda.synchronize()
        scopes = [r[4] for r in prof.rec]
        info[name] = dict(c_abi_calls=len(scopes), forward_calls=sum(1 for s in scopes if s.endswith(".fwd")),
                          prefix_calls=sum(1 for s in scopes if s == "prefix.fwd"),
                          backward_calls=sum(1 for s in scopes if s.endswith(".bwd")),
                          eval_prefix=list(getattr(eng, "eval_prefix", ())), frozen_tensors=len(eng.frozen))
        routes[name] = eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True)
        keep.append(eng)
    res = alternate(routes, steps)
    for eng in keep:
        assert bool(torch.isfinite(eng.params.flat).all())
    for k in info:
        res[k].update(info[k])
    res["workload"] = f"{workload}: batch {B}, {T} x {H} x {W}, bf16, captured graph + optimizer launch"
    return res


def part_a(steps):
    out = {}
    for name, wl in WORKLOADS:
        res = _step_routes(wl, {"stem_s1_s2_batch": (FRONT, "batch"), "stem_s1_s2_eval": (FRONT, "eval"),
                                "trunk_batch": (TRUNK, "batch"), "trunk_eval": (TRUNK, "eval")}, steps)
        for fs in ("stem_s1_s2", "trunk"):
            e, b = res[fs + "_eval"], res[fs + "_batch"]
            e["next_to_batch"] = verdict(e, b, "'eval' next to 'batch'")
            e["median_over_batch"] = round(e["median_ms"] / b["median_ms"], 4)
        out[name] = res
        print("a", name, json.dumps(res), flush=True)
        torch.cuda.empty_cache()
    return out


def part_b(steps):
    out = {}
    for name, wl in WORKLOADS:
        out[name] = _step_routes(wl, {"full": (None, None), "trunk_frozen": (TRUNK, None), "stem_s1_s2_frozen": (FRONT, None)},
                                 steps)
        print("b", os.environ.get("TDEED_LIB_FLAVOUR", "release"), name, json.dumps(out[name]), flush=True)
        torch.cuda.empty_cache()
    return out


def part_c(reps):
    from tdeed_amd.packing import stem_frags_on_device
    dev, N, H, W = "cuda", 1600, 224, 224
    frames = ops.fill_u8_hash((N, 3, H, W), 77, dev).float().mul_(0.75).add_(11.3)        # fp32 0..255, non-integer
    flips = (torch.arange(N, device=dev) % 2).to(torch.uint8)
    w = torch.from_numpy(synth.normalish(3, "stem", 32 * 27).astype("float32")).reshape(32, 3, 3, 3).mul(0.3).to(dev)
    sc = torch.from_numpy(synth.normalish(4, "sc", 32).astype("float32")).to(dev)
    sh = torch.from_numpy(synth.normalish(5, "sh", 32).astype("float32")).to(dev)
    wf, w27 = stem_frags_on_device(w), w.reshape(32, 27).contiguous()
    out_a = torch.empty((N, H // 2, W // 2, 32), dtype=torch.bfloat16, device=dev)
    out_b = torch.empty_like(out_a)
    res = alternate({"stem_mfma_eval": lambda: ops.stem_mfma_eval(frames, wf, sc, sh, None, flips, out=out_a),
                     "stem_fwd": lambda: ops.stem(frames, w27, sc, sh, torch.bfloat16, None, flips, out=out_b)}, reps)
    torch.cuda.synchronize()
    diff = (out_a.float() - out_b.float()).abs()
    res["max_abs_difference"] = float(diff.max())
    res["elements_that_differ"] = float((diff > 0).float().mean())
    nbytes = frames.numel() * 4 + out_a.numel() * 2
    for k in ("stem_mfma_eval", "stem_fwd"):
        res[k]["bytes"] = nbytes
        res[k]["GBps_at_median"] = round(nbytes / res[k]["median_ms"] / 1e6, 1)
    res["stem_mfma_eval"]["next_to_stem_fwd"] = verdict(res["stem_mfma_eval"], res["stem_fwd"], "the instance next to tdeed_stem_fwd")
    res["workload"] = f"{N} fp32 frames of {H} x {W}, alternating per-frame flips, bf16 output"
    print("c", json.dumps(res), flush=True)
    return res


def merge(parts):
    """Pool part b's rounds per library flavour over its processes; parts a and c pass through."""
    out = dict(tool="tools/bench_frozen_eval.py", rounds=ROUNDS,
               method="device events around `steps` back-to-back captured steps (part c: `reps` launches); routes alternate "
                      "inside each round; one warm-up round; median / min / max over the timed rounds.  Part b: one process "
                      "per library flavour and visit, the processes alternating; a flavour's rounds are pooled over its visits")
    pooled = {}
    for path in parts:
        with open(path) as f:
            p = json.load(f)
        out.setdefault("device", p.get("device"))
        for key in ("a_captured_step_batch_vs_eval", "c_stem_alone"):
            if key in p:
                out[key] = p[key]
        if "b_default_step" in p:
            fl = p["flavour"]
            for wl, res in p["b_default_step"].items():
                for route, r in res.items():
                    if isinstance(r, dict) and "rounds_ms" in r:
                        pooled.setdefault(wl, {}).setdefault(route, {}).setdefault(fl, []).extend(r["rounds_ms"])
    if pooled:
        b = {}
        for wl, routes in pooled.items():
            b[wl] = {}
            for route, by_fl in routes.items():
                st = {fl: dict(rounds_ms=v, median_ms=round(statistics.median(v), 5), min_ms=min(v), max_ms=max(v))
                      for fl, v in by_fl.items()}
                if "release" in st and "parent" in st:
                    st["this_commit_next_to_parent"] = verdict(st["release"], st["parent"], "this commit next to the parent's kernels")
                b[wl][route] = st
        out["b_default_step_this_commit_vs_parent"] = b
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b", "c"))
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_eval_prefix.json"))
    ap.add_argument("--steps", type=int, default=5, help="training steps per timing")
    ap.add_argument("--reps", type=int, default=20, help="launches per timing of the stem routes")
    a = ap.parse_args()
    if a.merge:
        out = merge(a.merge)
    else:
        assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
        out = dict(device=torch.cuda.get_device_name(0), flavour=os.environ.get("TDEED_LIB_FLAVOUR", "release"), steps=a.steps,
                   reps=a.reps)
        if a.part == "a":
            out["a_captured_step_batch_vs_eval"] = part_a(a.steps)
        elif a.part == "b":
            out["b_default_step"] = part_b(a.steps)
        else:
            out["c_stem_alone"] = part_c(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
