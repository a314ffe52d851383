"""GPU tool: what the weight EMA costs inside the AdamW launch, next to the separate pass it replaces -> profiles/ema_step.json.
    python tools/bench_ema.py [--out FILE] [--reps N] [--steps N] [--no-train-step]

1. At the flat parameter sizes of the 200MF (rny002_b8) and 800MF (rny008_b8) models, three families of three routes each:
   the launch without EMA, tdeed_adamw_step_ema, and the launch without EMA followed by a SEPARATE second pass over the
   buffer (tdeed_ema_tensors with one row per tensor over the flat buffer's views -- what the fused form replaces) --
   plain, with the guard (statistics + guarded launch, skip_nonfinite), and with the three-group example of INTEGRATION.md.
2. The captured training step (TrainEngine.make_step: graph + optimizer launch(es)) at 200MF B = 8 and 800MF B = 16, T = 100,
   224 x 224, bf16, without and with EMA (the statistics launch included).
Expectation from bytes alone, recorded next to the measurement: AdamW reads four buffers and writes three (7 words per
element); the EMA launch adds one read and one write of the shadow (9 words: 9/7 of the plain launch); the separate pass
re-reads p and reads and writes the shadow (3 more words, 10/7, and one more launch).
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
from bench_param_groups import EXAMPLE  # noqa: E402
from tdeed_amd import ops, state_layout, synth  # noqa: E402
from tdeed_amd.optim import FlatParams, group_table  # noqa: E402

DECAY = 0.999
WORDS = dict(base=7, ema=9, separate=10)       # fp32 words moved per element


def verdict(route, base, what):
    """the README's wording for a route next to another one"""
    if overlap(route, base):
        return f"ranges overlap with {what}"
    return f"slower than {what} in every round" if route["min_ms"] > base["max_ms"] else f"faster than {what} in every round"


def flat_launches(cfg, reps):
    dev = "cuda"
    shapes = state_layout.model_state_shapes(cfg)
    lay = FlatParams.layout_only({k: torch.empty(s, device="meta") for k, (s, _) in shapes.items()})
    n = lay.numel
    p = torch.randn(n, device=dev) * 0.05
    g = torch.randn(n, device=dev) * 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    e_fused, e_sep = p.clone(), p.clone()
    guard = torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=dev)
    ws = ops.grad_guard_ws(n, dev)
    runs = group_table(lay.index, n, EXAMPLE, None)
    table = ops.adamw_run_table(runs, n, dev)
    # the separate pass: one row per tensor, sources the flat buffer's views, the shadow laid out like the flat buffer
    order = sorted(lay.index, key=lambda k: lay.index[k][0])
    rows = ops.ema_tensor_table([p[lay.index[k][0]:lay.index[k][0] + lay.index[k][1]] for k in order],
                                [lay.index[k][0] for k in order])
    lr = 1e-6                                  # many timed steps on one gradient: keep the parameters where they are
    box = dict(t=0)

    def route(kind, family):
        gd = guard if family == "guard" else None
        tb = table if family == "groups" else None

        def run():
            box["t"] += 1
            t = box["t"]
            if gd is not None:
                ops.grad_guard(g, gd, ws, True)
            if kind == "ema":
                ops.adamw_step_ema(p, g, m, v, t, lr, e_fused, DECAY, True, 0, tb, guard=gd, skip_nonfinite=gd is not None)
                return
            if tb is not None:
                ops.adamw_step_groups(p, g, m, v, t, lr, tb)
            elif gd is not None:
                ops.adamw_step_guarded(p, g, m, v, t, lr, guard=gd, skip_nonfinite=True)
            else:
                ops.adamw_step(p, g, m, v, t, lr)
            if kind == "separate":
                ops.ema_tensors(rows, e_sep, t, DECAY, True, 0, guard=gd, skip_nonfinite=gd is not None)
        return run

    families = ("plain", "guard", "groups")
    res = alternate({f"{f}.{k}": route(k, f) for f in families for k in ("base", "ema", "separate")}, reps)
    rec = guard.cpu()
    assert int(rec[2]) == 0 and int(rec[3]) == 0
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(e_fused).all()) and bool(torch.isfinite(e_sep).all())
    out = dict(numel=n, tensors=len(order), group_runs=len(runs))
    for f in families:
        fam = {k: res[f"{f}.{k}"] for k in ("base", "ema", "separate")}
        for k in fam:
            fam[k]["bytes_over_base_expected"] = round(WORDS[k] / WORDS["base"], 4)
        for k in ("ema", "separate"):
            fam[k]["next_to_base"] = verdict(fam[k], fam["base"], "the launch without EMA")
            fam[k]["median_over_base"] = round(fam[k]["median_ms"] / fam["base"]["median_ms"], 4)
        fam["ema"]["next_to_separate"] = verdict(fam["ema"], fam["separate"], "the separate pass")
        fam["ema"]["median_over_separate"] = round(fam["ema"]["median_ms"] / fam["separate"]["median_ms"], 4)
        out[f] = fam
    return out


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
    routes, keep, info = {}, [], {}
    for name, ema in (("without_ema", None), ("with_ema", (DECAY, True))):
        sd = {k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 0).items()}
        eng = TrainEngine(cfg, sd, dt, dev, lr=1e-4)
        if ema is not None:
            eng.set_ema(*ema)
            info[name] = dict(shadow_elements=int(eng.opt.ema.numel()), statistics_rows=len(eng.ema_stat_index),
                              statistics_elements=int(eng.ema_stats.numel()))
        routes[name] = eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True)
        keep.append(eng)
    res = alternate(routes, reps)
    for eng in keep:
        assert bool(torch.isfinite(eng.params.flat).all())
    assert bool(torch.isfinite(keep[1].opt.ema).all()) and bool(torch.isfinite(keep[1].ema_stats).all())
    res["with_ema"].update(info["with_ema"])
    res["with_ema"]["next_to_without"] = verdict(res["with_ema"], res["without_ema"], "the step without EMA")
    res["with_ema"]["median_over_without"] = round(res["with_ema"]["median_ms"] / res["without_ema"]["median_ms"], 4)
    res["workload"] = f"{workload}: batch {B}, {T} x {H} x {W}, bf16, captured graph + optimizer launch(es)"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step.json"))
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the flat-buffer routes")
    ap.add_argument("--steps", type=int, default=5, help="training steps per timing")
    ap.add_argument("--no-train-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    out = dict(tool="tools/bench_ema.py", device=torch.cuda.get_device_name(0), rounds=ROUNDS, reps=a.reps, steps=a.steps,
               ema=dict(decay=DECAY, warmup=True),
               method="device events around `reps` back-to-back calls; routes alternate inside each round; one warm-up "
                      "round; median / min / max over the timed rounds",
               expectation_from_bytes="fp32 words per element: launch without EMA 7 (4 read, 3 written), EMA launch 9 "
                                      "(9/7 = 1.2857 of it), launch + separate pass 10 (10/7 = 1.4286) and one more "
                                      "launch; the separate pass runs one workgroup per tensor",
               flat={}, train_step={})
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
