"""GPU tool: what the loss options cost next to the plain loss launches and the plain training step
-> profiles/loss_options.json.
    python tools/bench_loss_options.py [--out FILE] [--steps N] [--reps N] [--step-only] [--root DIR]
                                       [--parent FILE ... --this FILE ...]

tdeed_loss_opt alone at (label_smoothing, focal_gamma) = (0.1, 0), (0, 2), (0.1, 2) against tdeed_loss_fwd +
tdeed_loss_bwd at 800 and 1600 rows, 5 and 33 classes; then, at T = 100 and 224 x 224, batch 8, bf16 (bench.py's
rny002_b8), the captured 200MF step without options and with (0.1, 2).  Device events, one process, the routes alternating
inside every round, one warm-up round and three timed ones, median and range of the rounds.  Compare the routes of one
run with each other, never with a number from another run.

The step without options against the commit before: `--step-only --root DIR` times that one route on another checkout of
the project (built there); `--parent FILE ... --this FILE ...` folds such results of the parent commit and of this one,
taken on the same box in processes that alternate, into the output and says whether their ranges overlap."""
import argparse
import json
import os
import statistics
import sys

ROUNDS = 3
SETTINGS = [(0.1, 0.0), (0.0, 2.0), (0.1, 2.0)]


def event_ms(torch, fn, reps):
    """mean ms per call of `reps` back-to-back calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(torch, routes, reps):
    """routes: name -> callable.  One warm-up round, then ROUNDS rounds in each of which every route is timed once, in
    turn -> name -> dict(rounds_ms, median_ms, min_ms, max_ms)."""
    for fn in routes.values():
        event_ms(torch, fn, max(reps // 4, 2))
    got = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            got[k].append(event_ms(torch, fn, reps))
    return {k: summary(v) for k, v in got.items()}


def summary(v):
    return dict(rounds_ms=[round(x, 5) for x in v], median_ms=round(statistics.median(v), 5), min_ms=round(min(v), 5),
                max_ms=round(max(v), 5))


def overlap(a, b):
    return a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]


def verdict(a, b, name_a, name_b):
    if overlap(a, b):
        return f"the ranges overlap: neither {name_a} nor {name_b} is called faster"
    return f"{name_a if a['max_ms'] < b['min_ms'] else name_b} is faster: the ranges do not overlap"


def steps(torch, bench, steps_per_timing, step_only):
    from tdeed_amd import ops, state_layout, synth
    from tdeed_amd.regnet_spec import regnet_spec
    from tdeed_amd.trainer import TrainEngine
    wl = bench.CONFIGS["rny002_b8"]
    cfg, B, H, W = wl["cfg"], wl["B"], wl["H"], wl["W"]
    T, dev, dt = cfg["clip_len"], "cuda", torch.bfloat16
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(cfg), 0).items()}
    eng = TrainEngine(cfg, sd, dt, dev, lr=1e-6)                 # many timed steps on one batch: keep the weights in place
    frames = ops.fill_u8_hash((B, T, 3, H, W), 1000, dev)
    lab_np, labD_np = synth.labels(5, B, T, cfg["num_classes"], max(cfg["radi_displacement"], 1))
    lab = torch.from_numpy(lab_np).to(dev)
    labD = torch.from_numpy(labD_np).float().to(dev) if cfg["radi_displacement"] else None
    C = regnet_spec(cfg["feature_arch"]).feat_dim
    masks = [((torch.rand((B, T, C), device=dev) >= 0.5).to(dt) * 2.0) for _ in range(2 if cfg["radi_displacement"] else 1)]
    routes = {"plain": eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True)}
    what = f"rny002_b8: batch {B}, {T} x {H} x {W}, bf16, captured graph + optimizer launch"
    if not step_only:
        plain = eng.last_graph
        loss = dict(label_smoothing=0.1, focal_gamma=2.0)
        eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True, loss=loss)
        hnd = eng.last_graph                                     # a second handle: the two graphs alternate on one engine
        routes["plain"] = lambda: eng.step_graph(plain, frames, lab, labD, drop_masks=masks)
        routes["options"] = lambda: eng.step_graph(hnd, frames, lab, labD, drop_masks=masks, loss=loss)
        what += "; with options: tdeed_loss_opt (label_smoothing 0.1, focal_gamma 2) in the graph instead of the two plain launches"
    res = alternate(torch, routes, steps_per_timing)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.params.flat).all())
    if "options" in res:
        res["options"]["median_over_plain"] = round(res["options"]["median_ms"] / res["plain"]["median_ms"], 4)
        res["options"]["against_plain"] = verdict(res["options"], res["plain"], "options", "plain")
    res["workload"] = what
    return res


def loss_alone(torch, rows, K1, reps):
    from tdeed_amd import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(rows + K1)
    head = (torch.randn((rows, K1 + 1), generator=g) * 2.0).to(dev)
    hard = torch.randint(0, K1, (rows,), generator=g).to(dev)
    labelD = torch.randn(rows, generator=g).to(dev)
    cls_w = torch.tensor([1.0] + [5.0] * (K1 - 1), device=dev)
    kw = dict(hard=hard, displ_col=K1, labelD=labelD)

    def pair():
        ops.loss(head, K1, cls_w, **kw)
        ops.loss_bwd(head, K1, cls_w, **kw)

    def opt(eps, gamma):
        return lambda: ops.loss_opt(head, K1, cls_w, label_smoothing=eps, focal_gamma=gamma, **kw)

    routes = {"loss_fwd_plus_loss_bwd": pair}
    for eps, gamma in SETTINGS:
        routes[f"loss_opt_eps{eps:g}_gamma{gamma:g}"] = opt(eps, gamma)
    res = alternate(torch, routes, reps)
    for k in res:
        if k != "loss_fwd_plus_loss_bwd":
            res[k]["against_pair"] = verdict(res[k], res["loss_fwd_plus_loss_bwd"], k, "loss_fwd_plus_loss_bwd")
    res["shape"] = f"{rows} rows, {K1} classes + displacement, hard labels; each call allocates its outputs like the step does"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10, help="training steps per timing")
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the loss routes")
    ap.add_argument("--step-only", action="store_true", help="only the step without options (also runs on older checkouts)")
    ap.add_argument("--root", default=None, help="another checkout of the project to import from (built there)")
    ap.add_argument("--parent", nargs="*", default=[], help="--step-only results of the parent commit from the same box")
    ap.add_argument("--this", nargs="*", default=[], help="--step-only results of this commit, processes alternating with those")
    a = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.abspath(a.root) if a.root else here
    sys.path.insert(0, root)
    import torch
    import bench
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing of this"
    out = dict(tool="tools/bench_loss_options.py", root=os.path.relpath(root, here), device=torch.cuda.get_device_name(0),
               rounds=ROUNDS, steps_per_timing=a.steps, reps=a.reps,
               method="device events around back-to-back calls; routes alternate inside each round; one warm-up round; "
                      "median / min / max over the timed rounds")
    if not a.step_only:
        out["loss_alone"] = {f"{rows}x{K1}": loss_alone(torch, rows, K1, a.reps) for rows in (800, 1600) for K1 in (5, 33)}
        print("loss alone", json.dumps(out["loss_alone"]), flush=True)
    out["train_step_200MF"] = steps(torch, bench, a.steps, a.step_only)
    print("train step", json.dumps(out["train_step_200MF"]), flush=True)
    if a.parent:
        def fold(paths):
            got = [json.load(open(p))["train_step_200MF"]["plain"] for p in paths]
            return dict(summary([x for g in got for x in g["rounds_ms"]]), processes=len(got))

        par = out["parent_step_only"] = fold(a.parent)
        mine = out["this_step_only"] = fold(a.this) if a.this else out["train_step_200MF"]["plain"]
        out["plain_against_parent"] = verdict(mine, par, "this commit", "the parent commit")
        print("step only", json.dumps(dict(parent=par, this=mine)), out["plain_against_parent"], flush=True)
    path = a.out or os.path.join(here, "profiles", "loss_options.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
