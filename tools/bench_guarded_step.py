"""GPU tool: what the guarded optimizer step costs next to the plain AdamW launch -> profiles/guarded_step.json.
    python tools/bench_guarded_step.py [--out FILE] [--reps N] [--steps N] [--no-train-step]

At the flat parameter sizes of the 200MF (rny002_b8) and 800MF (rny008_b8) models: the plain tdeed_adamw_step launch,
tdeed_grad_guard + tdeed_adamw_step_guarded with skipping only, and the same with clipping.  Device events, one process,
the three routes alternating inside every round, one warm-up round and three timed ones, median and range of the rounds.
Then one 200MF training step through TrainEngine.make_step (captured graph + optimizer), with and without the guard,
alternating in the same way.  Compare the routes of one run with each other, never with a number from another run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
from tdeed_amd import ops, state_layout, synth  # noqa: E402
from tdeed_amd.optim import FlatParams  # noqa: E402

ROUNDS = 3


def event_ms(fn, reps):
    """mean ms per call of `reps` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(routes, reps):
    """routes: name -> callable.  One warm-up round, then ROUNDS rounds in each of which every route is timed once, in
    turn -> name -> dict(rounds_ms, median_ms, min_ms, max_ms)."""
    for fn in routes.values():
        event_ms(fn, max(reps // 4, 1))
    got = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            got[k].append(event_ms(fn, reps))
    return {k: dict(rounds_ms=[round(x, 5) for x in v], median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5),
                    max_ms=round(max(v), 5)) for k, v in got.items()}


def overlap(a, b):
    return a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]


def flat_launches(n, reps):
    dev = "cuda"
    p = torch.randn(n, device=dev) * 0.05
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    guard = torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=dev)
    ws = ops.grad_guard_ws(n, dev)
    lr = 1e-6                                  # many timed steps on one gradient: keep the parameters where they are
    box = dict(t=0)

    def plain():
        box["t"] += 1
        ops.adamw_step(p, g, m, v, box["t"], lr)

    def guarded(max_norm):
        def run():
            box["t"] += 1
            ops.grad_guard(g, guard, ws, True)
            ops.adamw_step_guarded(p, g, m, v, box["t"], lr, guard=guard, skip_nonfinite=True, max_grad_norm=max_norm)
        return run

    norm = float(g.double().norm())
    res = alternate({"plain": plain, "guard_skip": guarded(None), "guard_skip_clip": guarded(0.5 * norm),
                     "statistics_only": lambda: ops.grad_guard(g, guard, ws, True)}, reps)
    rec = guard.cpu()
    assert int(rec[2]) == 0 and int(rec[3]) == 0 and bool(torch.isfinite(p).all())
    res["bytes"] = dict(plain=28 * n, statistics=4 * n)          # AdamW: four buffers read, three written
    for k in ("guard_skip", "guard_skip_clip"):
        res[k]["ranges_overlap_plain"] = overlap(res[k], res["plain"])
        res[k]["median_over_plain"] = round(res[k]["median_ms"] / res["plain"]["median_ms"], 4)
    return res


def train_step(workload, reps):
    from tdeed_amd.regnet_spec import regnet_spec
    from tdeed_amd.trainer import TrainEngine
    wl = bench.CONFIGS[workload]
    cfg, B, H, W = wl["cfg"], wl["B"], wl["H"], wl["W"]
    T, dev, dt = cfg["clip_len"], "cuda", torch.bfloat16
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 0).items()}
    eng = TrainEngine(cfg, sd, dt, dev, lr=1e-4)
    frames = ops.fill_u8_hash((B, T, 3, H, W), 1000, dev)
    lab_np, labD_np = synth.labels(5, B, T, cfg["num_classes"], max(cfg["radi_displacement"], 1))
    lab = torch.from_numpy(lab_np).to(dev)
    labD = torch.from_numpy(labD_np).float().to(dev) if cfg["radi_displacement"] else None
    C = regnet_spec(cfg["feature_arch"]).feat_dim
    masks = [((torch.rand((B, T, C), device=dev) >= 0.5).to(dt) * 2.0) for _ in range(2 if cfg["radi_displacement"] else 1)]
    step = eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True)
    eng.opt.set_guard(skip_nonfinite=True, max_grad_norm=1.0)
    record = eng.opt.guard

    def plain():
        eng.opt.guard = None                   # the plain launch, as if set_guard had never been called
        step()

    def guarded():
        eng.opt.guard = record
        step()

    res = alternate({"plain": plain, "guard_skip_clip": guarded}, reps)
    eng.opt.guard = record
    st = eng.opt.guard_stats()
    assert st["skipped"] == 0 and bool(torch.isfinite(eng.params.flat).all())
    res["guard_skip_clip"]["ranges_overlap_plain"] = overlap(res["guard_skip_clip"], res["plain"])
    res["guard_skip_clip"]["median_over_plain"] = round(res["guard_skip_clip"]["median_ms"] / res["plain"]["median_ms"], 4)
    res["workload"] = f"{workload}: batch {B}, {T} x {H} x {W}, bf16, captured graph + optimizer launch(es)"
    res["last_norm"] = st["last_norm"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guarded_step.json"))
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the flat-buffer routes")
    ap.add_argument("--steps", type=int, default=10, help="training steps per timing")
    ap.add_argument("--no-train-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    out = dict(tool="tools/bench_guarded_step.py", device=torch.cuda.get_device_name(0), rounds=ROUNDS, reps=a.reps,
               method="device events around `reps` back-to-back calls; routes alternate inside each round; one warm-up "
                      "round; median / min / max over the timed rounds", flat={})
    for name, wl in (("200MF", "rny002_b8"), ("800MF", "rny008_b8")):
        cfg = bench.CONFIGS[wl]["cfg"]
        shapes = state_layout.model_state_shapes(cfg)
        n = FlatParams.layout_only({k: torch.empty(s, device="meta") for k, (s, _) in shapes.items()}).numel
        out["flat"][name] = dict(workload=wl, numel=n, **flat_launches(n, a.reps))
        print(name, json.dumps(out["flat"][name]), flush=True)
    if not a.no_train_step:
        out["train_step_200MF"] = train_step("rny002_b8", a.steps)
        print("train step", json.dumps(out["train_step_200MF"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
