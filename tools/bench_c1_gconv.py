"""GPU tool: conv1 + grouped 3x3 in one launch (tdeed_c1_gconv_fwd) alone at the shapes of the shipped models, with its phase
time stamps (tdeed_c1_gconv_set_debug), in both forms (per slab / slab loop) where both exist; then the form that also
computes the producer's conv3 (tdeed_c1_gconv_c3in_fwd) against the two launches it replaces, at 800 x 56 x 56 x 24 -> 56,
with c1_gconv's stamps; then the band walk, which is that form's one kernel (tdeed_c1_gconv_c3in_set_walk): the launch alone at
every run length of the sweep, 1 (runs of one band) included, with the stamps of a walking workgroup.
    python tools/bench_c1_gconv.py [--c3in]        (--c3in: only the conv3-in section)"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tdeed_amd import ops, _lib
from tdeed_amd.engine import pack_mfma_frags, pack_gconv_frags, pack_ws_weights

DEV = "cuda"


def timeit(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


SHAPES = [("200MF s2.b1", 800, 56, 24, 56, 8, 2), ("200MF s3.b1", 800, 28, 56, 152, 8, 2), ("200MF s4.b1", 800, 14, 152, 368, 8, 2),
          ("800MF s2.b1", 1600, 56, 64, 128, 16, 2), ("800MF s2.b2", 1600, 28, 128, 128, 16, 1), ("800MF s3.b1", 1600, 28, 128, 320, 16, 2)]
for name, N, Hi, Cin, C, gw, stride in ([] if "--c3in" in sys.argv else SHAPES):
    g = torch.Generator().manual_seed(0)
    if not ops.c1_gconv_fits(Hi, Hi, Cin, C, stride):
        print(f"{name}: not served")
        continue
    x = torch.relu(torch.randn(N, Hi, Hi, Cin, generator=g)).to(torch.bfloat16).to(DEV)
    W1 = torch.randn(C, Cin, generator=g) / Cin ** 0.5
    W2 = torch.randn(C, gw, 3, 3, generator=g) / (gw * 9) ** 0.5
    vec = lambda n, s=0.1, o=0.0: (torch.randn(n, generator=g) * s + o).to(DEV)      # noqa: E731
    s1, h1, s2, h2 = vec(C, .1, 1.), vec(C), vec(C, .1, 1.), vec(C)
    rows = 16 * ops.c1_gconv_slab_tiles(Hi, Hi, C, stride)
    w1f = pack_mfma_frags(W1.numpy(), DEV, rows=rows)
    w2f = pack_gconv_frags(W2.numpy(), gw, DEV)
    Ho = (Hi - 1) // stride + 1
    out = torch.empty((N, Ho, Ho, C), dtype=torch.bfloat16, device=DEV)
    parts = ops.gconv3x3_parts(Hi, Hi, C, stride, torch.bfloat16)
    pooled = torch.empty((N, parts, C), device=DEV)

    def run():
        ops.c1_gconv(x, w1f, s1, h1, w2f, s2, h2, gw, stride, C, out=out, pooled=pooled)

    # both forms where the slab loop exists for the shape (tdeed_c1_gconv_set_form): one workgroup per (frame, band, slab),
    # and one per (frame, band) that walks the slabs -- whose stamps are prologue, slab 0's conv1, barrier, slab 0's grouped
    # conv, the other slabs
    byt = (x.numel() + out.numel()) * 2
    forms = (0, 1) if ops.c1_gconv_slab_loop_fits(Hi, Hi, Cin, C, stride) else (0,)
    outs = {}
    for form in forms:
        ops.c1_gconv_set_form(form)
        us = timeit(run)
        nwg = ops.c1_gconv_workgroups(N, Hi, Hi, Cin, C, stride)
        dbg = torch.zeros((nwg + 64, 8), dtype=torch.int64, device=DEV)
        _lib.call("tdeed_c1_gconv_set_debug", dbg.data_ptr())
        run()
        torch.cuda.synchronize()
        _lib.call("tdeed_c1_gconv_set_debug", None)
        outs[form] = (out.clone(), pooled.clone())
        d = dbg.cpu().numpy().astype(np.float64)[:nwg] * 10.0 / 1e3          # us
        ok = d[:, 6] > 0
        d = d[ok]
        names = (["prologue (halo, fold, requests)", "slab 0 conv1 (wave 0)", "barrier", "slab 0 grouped conv", "other slabs", "-"] if form
                 else ["weights + halo", "conv1 tiles (wave 0)", "barrier", "grouped conv setup", "grouped conv tiles + stores", "squeeze sums"])
        ph = [np.median(d[:, i + 1] - d[:, i]) for i in range(6)]
        print(f"{name} N={N} {Hi}x{Hi} {Cin}->{C} stride {stride}, {'slab loop' if form else 'per slab '}: {us:7.1f} us per launch, "
              f"{byt / us / 1e3:6.0f} GB/s algorithmic, {nwg} workgroups ({int(ok.sum())} stamped); first start -> last end "
              f"{(d[:, 6].max() - d[:, 0].min()):.1f} us; workgroup median {np.median(d[:, 6] - d[:, 0]):.2f} us: "
              + ", ".join(f"{n_} {v:.2f}" for n_, v in zip(names, ph)), flush=True)
    ops.c1_gconv_set_form(-1)
    if len(outs) == 2:
        print(f"  forms identical: {torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])}", flush=True)


# ---- the producer's conv3 in front of conv1 (engine.S1_CONV3_IN_C1G): s1.b1.conv3 + s2.b1.conv1_conv2 of RegNetY-200MF
PHASES = ["weights + halo", "conv1 tiles (wave 0)", "barrier", "grouped conv setup", "grouped conv tiles + stores", "squeeze sums"]


def stamped(run, nwg):
    """median phase times (us) of one stamped launch of `run`, and the median workgroup time"""
    dbg = torch.zeros((nwg + 64, 8), dtype=torch.int64, device=DEV)
    _lib.call("tdeed_c1_gconv_set_debug", dbg.data_ptr())
    run()
    torch.cuda.synchronize()
    _lib.call("tdeed_c1_gconv_set_debug", None)
    d = dbg.cpu().numpy().astype(np.float64)[:nwg] * 10.0 / 1e3
    d = d[d[:, 6] > 0]
    return [float(np.median(d[:, i + 1] - d[:, i])) for i in range(6)], float(np.median(d[:, 6] - d[:, 0]))


N, Hi, Cp, C, gw = 800, 56, 24, 56, 8
if not ops.c1_gconv_c3in_fits(Hi, Hi, Cp, C):
    print("conv3 in front of conv1: not served by this library")
    sys.exit(0)
g = torch.Generator().manual_seed(1)
y2p = torch.relu(torch.randn(N, Hi, Hi, Cp, generator=g)).to(torch.bfloat16).to(DEV)
scp = torch.randn(N, Hi, Hi, Cp, generator=g).to(torch.bfloat16).to(DEV)
gate = torch.sigmoid(torch.randn(N, Cp, generator=g)).to(DEV)
W3 = pack_ws_weights((torch.randn(Cp, Cp, generator=g) / Cp ** 0.5).numpy(), torch.bfloat16, DEV)
W1 = torch.randn(C, Cp, generator=g) / Cp ** 0.5
W2 = torch.randn(C, gw, 3, 3, generator=g) / (gw * 9) ** 0.5
vec = lambda n, s=0.1, o=0.0: (torch.randn(n, generator=g) * s + o).to(DEV)          # noqa: E731
s3, h3, s1, h1, s2, h2 = vec(Cp, .1, 1.), vec(Cp), vec(C, .1, 1.), vec(C), vec(C, .1, 1.), vec(C)
w1f = pack_mfma_frags(W1.numpy(), DEV, rows=16 * ops.c1_gconv_slab_tiles(Hi, Hi, C, 2))
w2f = pack_gconv_frags(W2.numpy(), gw, DEV)
Ho = (Hi - 1) // 2 + 1
parts = ops.gconv3x3_parts(Hi, Hi, C, 2, torch.bfloat16)
mid = torch.empty((N, Hi, Hi, Cp), dtype=torch.bfloat16, device=DEV)
out, out_f = (torch.empty((N, Ho, Ho, C), dtype=torch.bfloat16, device=DEV) for _ in range(2))
pooled, pooled_f = (torch.empty((N, parts, C), device=DEV) for _ in range(2))
xs2 = torch.empty((N, Ho, Ho, Cp), dtype=torch.bfloat16, device=DEV)


def conv3():
    ops.gemm_ws(y2p, W3, Cp, Cp, s3, h3, ops.ACT_RELU, residual=scp, a_scale=gate, a_scale_rows=Hi * Hi, out=mid.view(-1, Cp))


def c1g():
    ops.c1_gconv(mid, w1f, s1, h1, w2f, s2, h2, gw, 2, C, out=out, pooled=pooled)


def chain():
    conv3()
    c1g()


def fused():
    ops.c1_gconv_c3in(y2p, scp, gate, W3, s3, h3, w1f, s1, h1, w2f, s2, h2, gw, C, xs2=xs2, out=out_f, pooled=pooled_f)


HAS_WALK = hasattr(_lib.load(), "tdeed_c1_gconv_c3in_set_walk")     # (not in an A/B flavour built from an older revision)
if HAS_WALK:
    ops.c1_gconv_c3in_set_walk(1)                                   # runs of one band
t3, tc, tch, tf = timeit(conv3), timeit(c1g), timeit(chain), timeit(fused)
same = torch.equal(out, out_f) and torch.equal(pooled, pooled_f) and torch.equal(xs2, mid[:, ::2, ::2, :])
print(f"conv3 in front of conv1, N={N} {Hi}x{Hi} {Cp}->{C}: conv3 alone {t3:.1f} us, c1_gconv alone {tc:.1f} us, the two back to back "
      f"{tch:.1f} us, fused {tf:.1f} us; outputs identical: {same}")
ph, wg = stamped(c1g, N * parts)
print(f"  c1_gconv workgroup median {wg:.2f} us: " + ", ".join(f"{n_} {v:.2f}" for n_, v in zip(PHASES, ph)), flush=True)


# ---- the band walk: one workgroup per (frame, run of `walk` bands).  The launch alone per run length (event timing, three
# rounds interleaved over the run lengths so that a drift of the box hits all of them), outputs against runs of one band, and
# the stamps of a walking workgroup: 0 start, 1 prologue end, 2 / 3 the first band's conv3 + conv1 and grouped conv (with the row
# copy and the barrier behind it), 4 / 5 the second band's (runs of two bands or more), 6 run end
if HAS_WALK:
    WALK_PHASES = ["prologue", "first band conv3 + conv1", "first band grouped conv + row copy", "second band conv3 + conv1",
                   "second band grouped conv + row copy", "the other bands"]
    ref = (out_f.clone(), pooled_f.clone(), xs2.clone())
    walks = [1, 2, 3, 4, 5, 7, 14]
    times = {w: [] for w in walks}
    for _ in range(3):
        for w in walks:
            ops.c1_gconv_c3in_set_walk(w)
            times[w].append(timeit(fused))
    routed = ops.c1_gconv_c3in_walk(Hi, Hi, Cp, C)
    print(f"band walk, N={N} {Hi}x{Hi} {Cp}->{C}, {parts} bands per frame, routed run length {routed}:")
    for w in walks:
        ops.c1_gconv_c3in_set_walk(w)
        nwg = ops.c1_gconv_c3in_workgroups(N, Hi, Hi, Cp, C)
        out_f.fill_(-7.0); xs2.fill_(-7.0); pooled_f.fill_(float("nan"))
        fused()
        torch.cuda.synchronize()
        same = torch.equal(out_f, ref[0]) and torch.equal(pooled_f, ref[1]) and torch.equal(xs2, ref[2])
        line = (f"  walk {w:2d}: {nwg:5d} workgroups, " + " / ".join(f"{t_:.1f}" for t_ in times[w])
                + f" us per launch (median {float(np.median(times[w])):.1f}); identical to runs of one band: {same}")
        ph, wg = stamped(fused, nwg)
        names = WALK_PHASES if w >= 2 else WALK_PHASES[:3]          # (runs of one band: no second band's stamps)
        line += f"; workgroup median {wg:.2f} us: " + ", ".join(f"{n_} {v:.2f}" for n_, v in zip(names, ph))
        print(line, flush=True)
    ops.c1_gconv_c3in_set_walk(0)
