"""GPU tool: what distillation costs next to the plain training step -> profiles/distill_step.json.
    python tools/bench_distill.py [--out FILE] [--steps N] [--reps N] [--step-only] [--root DIR]
                                  [--parent FILE ... --this FILE ...]

At T = 100 and 224 x 224, batch 8, bf16 (bench.py's rny002_b8): the captured 200MF step without a teacher; the same step
with a 200MF teacher; the same step with an 800MF teacher -- teacher forward (ForwardEngine.forward_augmented on the step's
frames, eager launches) + captured graph with the tdeed_loss_kd launch + optimizer.  Then tdeed_loss_kd alone against
tdeed_loss_fwd + tdeed_loss_bwd at 800 and 1600 rows.  Device events, one process, the routes alternating inside every
round, one warm-up round and three timed ones, mean and range of the rounds.  Compare the routes of one run with each
other, never with a number from another run.

The step without a teacher against the commit before distillation: `--step-only --root DIR` times that one route on
another checkout of the project (built there); `--parent FILE ... --this FILE ...` folds such results of the parent commit
and of this one, taken on the same box in processes that alternate, into the output and says whether their ranges overlap
(like for like: in the full run the route shares its process with two teacher engines and a second graph handle)."""
import argparse
import json
import os
import statistics
import sys

ROUNDS = 3


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
    turn -> name -> dict(rounds_ms, mean_ms, min_ms, max_ms)."""
    for fn in routes.values():
        event_ms(torch, fn, max(reps // 4, 2))
    got = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            got[k].append(event_ms(torch, fn, reps))
    return {k: summary(v) for k, v in got.items()}


def summary(v):
    return dict(rounds_ms=[round(x, 5) for x in v], mean_ms=round(statistics.mean(v), 5), min_ms=round(min(v), 5),
                max_ms=round(max(v), 5))


def overlap(a, b):
    return a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]


def verdict(a, b, name_a, name_b):
    if overlap(a, b):
        return f"the ranges overlap: neither {name_a} nor {name_b} is called faster"
    return f"{name_a if a['max_ms'] < b['min_ms'] else name_b} is faster: the ranges do not overlap"


def steps(torch, bench, steps_per_timing, step_only):
    from tdeed_amd import ops, state_layout, synth
    from tdeed_amd.engine import ForwardEngine
    from tdeed_amd.regnet_spec import regnet_spec
    from tdeed_amd.trainer import TrainEngine
    wl = bench.CONFIGS["rny002_b8"]
    cfg, B, H, W = wl["cfg"], wl["B"], wl["H"], wl["W"]
    T, dev, dt = cfg["clip_len"], "cuda", torch.bfloat16

    def state(c, seed):
        return {k: torch.from_numpy(v) for k, v in synth.make_state(state_layout.model_state_shapes(c), seed).items()}

    eng = TrainEngine(cfg, state(cfg, 0), dt, dev, lr=1e-6)      # many timed steps on one batch: keep the weights in place
    frames = ops.fill_u8_hash((B, T, 3, H, W), 1000, dev)
    lab_np, labD_np = synth.labels(5, B, T, cfg["num_classes"], max(cfg["radi_displacement"], 1))
    lab = torch.from_numpy(lab_np).to(dev)
    labD = torch.from_numpy(labD_np).float().to(dev) if cfg["radi_displacement"] else None
    C = regnet_spec(cfg["feature_arch"]).feat_dim
    masks = [((torch.rand((B, T, C), device=dev) >= 0.5).to(dt) * 2.0) for _ in range(2 if cfg["radi_displacement"] else 1)]
    routes = {"no_teacher": eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True)}
    what = f"rny002_b8: batch {B}, {T} x {H} x {W}, bf16, captured graph + optimizer launch"
    if not step_only:
        teachers = {}
        for name, twl in (("teacher_200MF", "rny002_b8"), ("teacher_800MF", "rny008_b8")):
            tcfg = dict(bench.CONFIGS[twl]["cfg"], num_classes=cfg["num_classes"], radi_displacement=cfg["radi_displacement"])
            teachers[name] = ForwardEngine(tcfg, state(tcfg, 1), dt, dev)
        first = next(iter(teachers.values()))
        head, _ = first.forward_augmented(frames, None)
        head = head.view(B * T, -1)
        kd = dict(displ_col_t=first.pw.displ_col, alpha=0.5, temperature=2.0, displ_weight=0.0)
        eng.make_step(B, H, W, frames, lab, labD, masks, use_graph=True, kd=dict(kd, teacher=head))
        hnd = eng.last_graph                                     # one handle serves both teachers: the same head layout

        def with_teacher(teng):
            def run():
                th, _ = teng.forward_augmented(frames, None)
                eng.step_graph(hnd, frames, lab, labD, drop_masks=masks, teacher=th.view(B * T, -1), kd=kd)
            return run

        for name, teng in teachers.items():
            routes[name] = with_teacher(teng)
            routes[name + "_forward_alone"] = (lambda e: lambda: e.forward_augmented(frames, None))(teng)
        what += "; with a teacher: + its eval-mode bf16 forward on the same frames (eager launches) and tdeed_loss_kd in the graph"
    res = alternate(torch, routes, steps_per_timing)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.params.flat).all())
    for k in res:
        if k != "no_teacher":
            res[k]["mean_over_no_teacher"] = round(res[k]["mean_ms"] / res["no_teacher"]["mean_ms"], 4)
            res[k]["against_no_teacher"] = verdict(res[k], res["no_teacher"], k, "no_teacher")
    res["workload"] = what
    return res


def loss_alone(torch, rows, reps):
    from tdeed_amd import ops
    dev, K1 = "cuda", 5
    g = torch.Generator().manual_seed(rows)
    head = (torch.randn((rows, K1 + 1), generator=g) * 2.0).to(dev)
    teacher = (torch.randn((rows, K1 + 1), generator=g) * 4.0).to(dev)
    hard = torch.randint(0, K1, (rows,), generator=g).to(dev)
    labelD = torch.randn(rows, generator=g).to(dev)
    cls_w = torch.tensor([1.0] + [5.0] * (K1 - 1), device=dev)
    kw = dict(hard=hard, displ_col=K1, labelD=labelD)

    def pair():
        ops.loss(head, K1, cls_w, **kw)
        ops.loss_bwd(head, K1, cls_w, **kw)

    res = alternate(torch, {"loss_fwd_plus_loss_bwd": pair,
                            "loss_kd": lambda: ops.loss_kd(head, K1, cls_w, teacher, teacher_displ_col=K1, **kw)}, reps)
    res["loss_kd"]["against_pair"] = verdict(res["loss_kd"], res["loss_fwd_plus_loss_bwd"], "loss_kd", "loss_fwd_plus_loss_bwd")
    res["shape"] = f"{rows} rows, {K1} classes + displacement, hard labels; each call allocates its outputs like the step does"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=10, help="training steps per timing")
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the loss routes")
    ap.add_argument("--step-only", action="store_true", help="only the step without a teacher (also runs on older checkouts)")
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
    out = dict(tool="tools/bench_distill.py", root=os.path.relpath(root, here), device=torch.cuda.get_device_name(0), rounds=ROUNDS,
               steps_per_timing=a.steps, reps=a.reps,
               method="device events around back-to-back calls; routes alternate inside each round; one warm-up round; "
                      "mean / min / max over the timed rounds")
    out["train_step_200MF"] = steps(torch, bench, a.steps, a.step_only)
    print("train step", json.dumps(out["train_step_200MF"]), flush=True)
    if not a.step_only:
        out["loss_alone"] = {str(rows): loss_alone(torch, rows, a.reps) for rows in (800, 1600)}
        print("loss alone", json.dumps(out["loss_alone"]), flush=True)
    if a.parent:
        def fold(paths):
            got = [json.load(open(p))["train_step_200MF"]["no_teacher"] for p in paths]
            return dict(summary([x for g in got for x in g["rounds_ms"]]), processes=len(got))

        par = out["parent_step_only"] = fold(a.parent)
        mine = out["this_step_only"] = fold(a.this) if a.this else out["train_step_200MF"]["no_teacher"]
        out["no_teacher_against_parent"] = verdict(mine, par, "this commit", "the parent commit")
        print("step only", json.dumps(dict(parent=par, this=mine)), out["no_teacher_against_parent"], flush=True)
    path = a.out or os.path.join(here, "profiles", "distill_step.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
