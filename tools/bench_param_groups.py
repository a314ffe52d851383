"""GPU tool: what parameter groups cost in the AdamW launch and what freezing saves in the step -> profiles/param_groups.json.
    python tools/bench_param_groups.py [--out FILE] [--reps N] [--steps N] [--no-train-step]

1. At the flat parameter sizes of the 200MF (rny002_b8) and 800MF (rny008_b8) models: the plain tdeed_adamw_step launch
   against tdeed_adamw_step_groups with one neutral run, with the three-group example of INTEGRATION.md (front of the trunk
   frozen, rest of the trunk at lr_scale 0.1, no decay on norms and biases) and with the whole trunk frozen.
2. The captured training step (TrainEngine.make_step: graph + optimizer launch) at 200MF B = 8 and 800MF B = 16, T = 100,
   224 x 224, bf16: nothing frozen against `_features.*` frozen against stem + s1 + s2 frozen, with the number of C-ABI
   calls an eager step of each issues.
Device events, one process, the routes alternating inside every round, one warm-up round and three timed ones, median and
range of the rounds (the method of tools/bench_guarded_step.py).  Compare the routes of one run with each other, never
with a number from another run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import bench  # noqa: E402
from bench_guarded_step import ROUNDS, alternate, overlap  # noqa: E402
from tdeed_amd import _lib, ops, state_layout, synth  # noqa: E402
from tdeed_amd.optim import FlatParams, group_table  # noqa: E402

FRONT = {"params": ("_features.stem.*", "_features.s1.*", "_features.s2.*"), "frozen": True}
EXAMPLE = [FRONT, {"params": ("_features.*",), "lr_scale": 0.1},
           {"params": ("*.bn.*", "*.ln*", "*.gn.*", "*.bias"), "weight_decay": 0.0}]
TRUNK = [{"params": ("_features.*",), "frozen": True}]


def verdict(route, plain):
    """the README's wording for a route next to the plain launch"""
    if overlap(route, plain):
        return "ranges overlap"
    return "slower in every round" if route["min_ms"] > plain["max_ms"] else "faster in every round"


def flat_launches(cfg, reps):
    dev = "cuda"
    shapes = state_layout.model_state_shapes(cfg)
    lay = FlatParams.layout_only({k: torch.empty(s, device="meta") for k, (s, _) in shapes.items()})
    n = lay.numel
    p = torch.randn(n, device=dev) * 0.05
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr = 1e-6                                  # many timed steps on one gradient: keep the parameters where they are
    box = dict(t=0)
    tables, info = {}, {}
    for name, groups in (("one_neutral_run", None), ("three_group_example", EXAMPLE), ("trunk_frozen", TRUNK)):
        runs = group_table(lay.index, n, groups, None)
        tables[name] = ops.adamw_run_table(runs, n, dev)
        lo, live = 0, 0
        for end, _, _, frozen in runs:
            live += 0 if frozen else end - lo
            lo = end
        info[name] = dict(runs=len(runs), trainable_elements=live, bytes=28 * live)

    def plain():
        box["t"] += 1
        ops.adamw_step(p, g, m, v, box["t"], lr)

    def grouped(name):
        def run():
            box["t"] += 1
            ops.adamw_step_groups(p, g, m, v, box["t"], lr, tables[name])
        return run

    routes = {"plain": plain}
    routes.update({k: grouped(k) for k in tables})
    res = alternate(routes, reps)
    assert bool(torch.isfinite(p).all())
    res["plain"]["bytes"] = 28 * n             # AdamW: four buffers read, three written
    for k in tables:
        res[k].update(info[k])
        res[k]["next_to_plain"] = verdict(res[k], res["plain"])
        res[k]["median_over_plain"] = round(res[k]["median_ms"] / res["plain"]["median_ms"], 4)
    res["numel"] = n
    return res


def train_step(workload, reps):
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
    for name, groups in (("full", None), ("trunk_frozen", TRUNK), ("stem_s1_s2_frozen", [FRONT])):
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 0).items()}
        eng = TrainEngine(cfg, sd, dt, dev, lr=1e-4)
        eng.set_groups(groups)
        with _lib.profile() as prof:               # the launches of one eager step, counted (not timed)
            eng.step(frames, lab, labD, drop_masks=masks)
        torch.cuda.synchronize()
        calls = [r for r in prof.rec]
        info[name] = dict(c_abi_calls=len(calls), backward_calls=sum(1 for r in calls if r[4].endswith(".bwd")),
                          backward_stages=len(eng.stages) if eng.stages is not None else "all",
                          frozen_tensors=len(eng.frozen))
        routes[name] = eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True)
        keep.append(eng)
    res = alternate(routes, reps)
    for eng in keep:
        assert bool(torch.isfinite(eng.params.flat).all())
    for k in info:
        res[k].update(info[k])
        if k != "full":
            res[k]["next_to_full"] = verdict(res[k], res["full"]).replace("ranges overlap", "ranges overlap with the full step")
            res[k]["median_over_full"] = round(res[k]["median_ms"] / res["full"]["median_ms"], 4)
    res["workload"] = f"{workload}: batch {B}, {T} x {H} x {W}, bf16, captured graph + optimizer launch"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_groups.json"))
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the flat-buffer routes")
    ap.add_argument("--steps", type=int, default=5, help="training steps per timing")
    ap.add_argument("--no-train-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    out = dict(tool="tools/bench_param_groups.py", device=torch.cuda.get_device_name(0), rounds=ROUNDS, reps=a.reps,
               steps=a.steps,
               method="device events around `reps` back-to-back calls; routes alternate inside each round; one warm-up "
                      "round; median / min / max over the timed rounds", flat={}, train_step={})
    for name, wl in (("200MF", "rny002_b8"), ("800MF", "rny008_b8")):
        out["flat"][name] = dict(workload=wl, **flat_launches(bench.CONFIGS[wl]["cfg"], a.reps))
        print(name, json.dumps(out["flat"][name]), flush=True)
    if not a.no_train_step:
        for name, wl in (("200MF_B8", "rny002_b8"), ("800MF_B16", "rny008_b16")):
            out["train_step"][name] = train_step(wl, a.steps)
            print("train step", name, json.dumps(out["train_step"][name]), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
