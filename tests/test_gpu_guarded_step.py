"""The guarded optimizer step on the MI355X: tdeed_grad_guard's statistics against numpy, tdeed_adamw_step_guarded against
the plain launch (bit for bit), torch.optim.AdamW (skip) and clip_grad_norm_ (clipping); then the same through
TrainEngine (eager and captured), the public get_optimizer / epoch interface, the optimizer state and a two-rank job.
Non-finite values enter only as gradient values or through labelD.  -m gpu only."""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import act, cfg_ns, load_golden, max_abs, model_state, t
from tdeed_amd import synth, state_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 100003                     # tests/test_gpu_ops.py::test_adamw_step_matches_torch_optim: scalar tail of 3
LR = 8e-4
TRIP = 4096 * 256 * 4          # elements the capped grid covers in one trip of the grid-stride loop
N_WRAP = TRIP + 3075           # a second trip of 768 chunks (workgroups 0..2) and a scalar tail of 3
# the CFG of tests/test_gpu_dp.py: 200MF, clip_len 6; batches of two 64 x 64 clips, fp32
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
KEY = "_pred_fine._fc_out.weight"          # a parameter name FlatParams accepts for a stand-alone flat buffer


@pytest.fixture(scope="module")
def ops():
    from tdeed_amd import ops as o, _lib
    _lib.load()
    return o


def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


@functools.lru_cache(maxsize=None)
def _host_grad(n):
    """(fp32 gradient, binary64 sum of squares by numpy); computed once per size and left unchanged"""
    g = np.random.default_rng(9000 + n % 1000).standard_normal(n).astype(np.float32)
    return g, float(np.sum(g.astype(np.float64) ** 2))


def _new_guard(ops, n):
    return torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=DEV), ops.grad_guard_ws(n, DEV)


def _record(guard):
    rec = guard.cpu()
    assert int(rec[4:].abs().sum()) == 0                         # reserved words are written as zero
    return rec[:2].view(torch.float64)[0].item(), int(rec[2]), int(rec[3]), rec.numpy().copy()


def _grid(n):
    return min((n >> 2) // 256 + 1, 4096)


# ----------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize("n", [1, 3, 255, 1027, N, N_WRAP])
def test_statistics_match_numpy_and_are_reproducible(ops, n):
    """sumsq within n * 2^-52 relative of numpy's binary64 sum: the squares are exact in binary64 and a sum of n
    non-negative terms in any order is within (n - 1) * 2^-53 to first order.  Two launches give the same bits."""
    g, ref = _host_grad(n)
    guard, ws = _new_guard(ops, n)
    assert ws.numel() == _grid(n)
    gd = t(g).to(DEV)
    ops.grad_guard(gd, guard, ws, True)
    sumsq, bad, skipped, bits = _record(guard)
    print(f"n {n}: sumsq {sumsq!r} numpy {ref!r} rel {abs(sumsq - ref) / ref:.3e} bound {n * 2.0 ** -52:.3e}")
    assert (bad, skipped) == (0, 0)
    assert abs(sumsq - ref) <= n * 2.0 ** -52 * ref
    ops.grad_guard(gd, guard, ws, True)
    assert np.array_equal(_record(guard)[3], bits)


def _nonfinite_cases(n):
    n4 = n >> 2
    cases = [("inf in element 0", 0, float("inf"))]
    if n & 3:
        cases.append(("NaN in the last element (scalar tail)", n - 1, float("nan")))
    if n4:
        chunk = min(n4 - 1, (_grid(n) - 1) * 256 + 5)            # a chunk of the last workgroup's first trip
        cases.append(("-inf in the last workgroup", 4 * chunk + 2, float("-inf")))
    if n > TRIP:
        cases.append(("NaN in the wrapped second trip", TRIP + 4 * 300 + 1, float("nan")))
    return cases


@pytest.mark.parametrize("n", [3, 1027, N, N_WRAP])
def test_nonfinite_is_seen_wherever_it_sits(ops, n):
    g, _ = _host_grad(n)
    gd = t(g).to(DEV)
    cases = _nonfinite_cases(n)
    assert len(cases) == (4 if n > TRIP else 3 if n >> 2 else 2)
    for name, idx, val in cases:
        guard, ws = _new_guard(ops, n)
        x = gd.clone()
        x[idx] = val
        ops.grad_guard(x, guard, ws, True)
        sumsq, bad, skipped, _ = _record(guard)
        assert (bad, skipped) == (1, 1) and not math.isfinite(sumsq), (name, n, sumsq)


def test_flt_max_denormals_and_negative_zero_are_finite(ops):
    n = 1027
    guard, ws = _new_guard(ops, n)
    fmax = float(np.finfo(np.float32).max)
    ops.grad_guard(torch.full((n,), fmax, device=DEV), guard, ws, True)
    sumsq, bad, skipped, _ = _record(guard)
    ref = float(np.sum(np.full(n, fmax, dtype=np.float64) ** 2))
    assert (bad, skipped) == (0, 0) and abs(sumsq - ref) <= n * 2.0 ** -52 * ref
    g = np.zeros(n, dtype=np.float32)
    g[0::3] = np.float32(1e-40)                                  # fp32 denormals: their squares are normal in binary64
    g[1::3] = np.float32(-1.4e-45)                               # the smallest one
    g[2::3] = np.float32(-0.0)
    assert g[0] != 0 and g[1] != 0 and np.signbit(g[2])
    ops.grad_guard(t(g).to(DEV), guard, ws, True)
    sumsq, bad, skipped, _ = _record(guard)
    ref = float(np.sum(g.astype(np.float64) ** 2))
    assert ref > 0 and (bad, skipped) == (0, 0) and abs(sumsq - ref) <= n * 2.0 ** -52 * ref
    ops.grad_guard(torch.full((n,), -0.0, device=DEV), guard, ws, True)
    assert _record(guard)[:3] == (0.0, 0, 0)


def test_skipped_counts_only_when_asked(ops):
    n = 1027
    g, ref = _host_grad(n)
    good = t(g).to(DEV)
    bad_g = good.clone()
    bad_g[77] = float("nan")
    guard, ws = _new_guard(ops, n)
    seen = []
    for buf, skip in ((bad_g, False), (bad_g, True), (bad_g, True), (good, True), (bad_g, False)):
        ops.grad_guard(buf, guard, ws, skip)
        seen.append(_record(guard)[1:3])
    assert seen == [(1, 0), (1, 1), (1, 2), (0, 2), (1, 2)]


# ----------------------------------------------------------------------------- 2. finite gradients, no clipping
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_finite_unclipped_steps_are_bit_identical_to_the_plain_launch(ops, grad_scale):
    p0 = rnd(141, "p", (N,))
    pa, ma, va = p0.clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    pb, mb, vb = p0.clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    guard, ws = _new_guard(ops, N)
    for step in range(1, 4):
        g = rnd(150 + step, "g", (N,)).to(DEV)
        ops.adamw_step(pa, g, ma, va, step, LR, grad_scale=grad_scale)
        ops.grad_guard(g, guard, ws, True)
        ops.adamw_step_guarded(pb, g, mb, vb, step, LR, grad_scale=grad_scale, guard=guard, skip_nonfinite=True)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), step
    assert _record(guard)[1:3] == (0, 0)


# ----------------------------------------------------------------------------- 3. skip, 7. optimizer state
def _skip_grads():
    grads = [rnd(151, "g", (N,)), rnd(152, "g", (N,)), rnd(153, "g", (N,))]
    grads[1][N // 2] = float("nan")
    return grads


def _flat_optimizer(p0):
    from tdeed_amd.optim import FlatParams, FusedAdamW
    fp = FlatParams({KEY: p0.clone()}, DEV)
    opt = FusedAdamW(fp, lr=LR)
    opt.set_guard(skip_nonfinite=True)
    return fp, opt


def test_skipped_step_changes_nothing_and_does_not_advance_the_bias_correction(ops):
    """Step 2 carries one NaN: param, exp_avg, exp_avg_sq keep their bits.  Step 3 then equals torch.optim.AdamW given
    steps 1 and 3 only within 2e-6, the existing AdamW test's bound (same generator, n, lr): a counter that advanced
    would be off by about 2e-4 (1 - 0.9^2 against 1 - 0.9^3)."""
    p0 = rnd(141, "p", (N,))
    grads = _skip_grads()
    ref_p = p0.clone().requires_grad_(True)
    ref = torch.optim.AdamW([ref_p], lr=LR)
    for g in (grads[0], grads[2]):
        ref_p.grad = g.clone()
        ref.step()
    p, m, v = p0.clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    guard, ws = _new_guard(ops, N)

    def attempt(step):
        g = grads[step - 1].to(DEV)
        ops.grad_guard(g, guard, ws, True)
        ops.adamw_step_guarded(p, g, m, v, step, LR, guard=guard, skip_nonfinite=True)

    attempt(1)
    before = (p.clone(), m.clone(), v.clone())
    attempt(2)
    assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
    assert _record(guard)[1:3] == (1, 1)
    attempt(3)
    assert _record(guard)[1:3] == (0, 1)
    err = max_abs(p.cpu(), ref_p.detach())
    print(f"skip: max |param - AdamW(steps 1, 3)| = {err:.3e}")
    assert err < 2e-6
    assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())


def test_optimizer_state_round_trip_takes_the_same_path():
    """After the first two of those steps (one skipped) state_dict() goes into a fresh FusedAdamW; step 3 on both is
    torch.equal, bias correction included (both read skipped == 1 and take the device's powf)."""
    p0 = rnd(141, "p", (N,))
    grads = _skip_grads()
    fp, opt = _flat_optimizer(p0)
    for g in grads[:2]:
        fp.grad_view(KEY).copy_(g)
        opt.step()
    sd = opt.state_dict()
    assert (sd["t"], sd["skipped"]) == (2, 1) and opt.guard_stats()["last_nonfinite"]
    fp2, opt2 = _flat_optimizer(fp.flat[:N].cpu())
    opt2.load_state_dict(sd)
    for f_, o_ in ((fp, opt), (fp2, opt2)):
        f_.grad_view(KEY).copy_(grads[2])
        o_.step()
    assert torch.equal(fp.flat, fp2.flat) and torch.equal(opt.exp_avg, opt2.exp_avg)
    assert torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq)
    assert opt2.t == 3 and opt2.guard_stats() == opt.guard_stats() and opt.guard_stats()["skipped"] == 1
    assert not torch.equal(fp.flat[:N].cpu(), p0)


# ----------------------------------------------------------------------------- 4. clipping
# The C ABI carries the betas as fp32 (tdeed_adamw_step and tdeed_adamw_step_guarded alike), and 0.999 is not an fp32
# number: float32(0.999) is 1.3e-8 above it, which 1 - beta2 magnifies a thousandfold -- 1 - float32(0.999) = 9.99987e-04,
# a relative 1.287e-05 from 1e-03 in every term of exp_avg_sq, for any implementation behind that ABI.  A comparison of the
# moment buffers with torch to 1e-5 therefore has to hand both sides the SAME betas: the fp32 values, which torch takes
# as they are (1 - BETAS[1] in binary64 is exact and equals the kernel's 1.0f - beta2).  The figure for torch run at the
# decimal 0.999 is printed by test_clipping_exp_avg_sq_matches_torch_state; it was 1.515e-05 on an MI355X.
BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))


@pytest.fixture(scope="module")
def clip_case():
    """three steps on the CPU through clip_grad_norm_ + AdamW, max_grad_norm at half of step 1's norm and above step 2's"""
    p0 = rnd(141, "p", (N,))
    grads = [rnd(151, "g", (N,)), rnd(152, "g", (N,), 0.25), rnd(153, "g", (N,))]
    max_norm = 0.5 * float(grads[0].norm())
    assert float(grads[1].norm()) < max_norm < float(grads[2].norm())

    def torch_run(betas):
        p = p0.clone().requires_grad_(True)
        opt = torch.optim.AdamW([p], lr=LR, betas=betas)
        clipped = []
        for g in grads:
            p.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([p], max_norm)
            clipped.append(p.grad.clone())
            opt.step()
        return p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), clipped

    p, m, v, clipped = torch_run(BETAS)
    return dict(p0=p0, grads=grads, clipped=clipped, max_norm=max_norm, p=p, m=m, v=v,
                v_decimal=torch_run((0.9, 0.999))[2])           # printed, not asserted: see BETAS


def _clipped_run(ops, c, grad_scale):
    """the three guarded steps with clipping on -> (param, exp_avg, exp_avg_sq, record)"""
    p, m, v = c["p0"].clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    guard, ws = _new_guard(ops, N)
    for step, g in enumerate(c["grads"], 1):
        gd = (g / grad_scale).to(DEV)                            # grad_scale 0.5: the buffer holds 2 g
        ops.grad_guard(gd, guard, ws, False)
        ops.adamw_step_guarded(p, gd, m, v, step, LR, betas=BETAS, grad_scale=grad_scale, guard=guard,
                               max_grad_norm=c["max_norm"])
    return p, m, v, guard


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipping_matches_clip_grad_norm(ops, clip_case, grad_scale):
    """exp_avg against torch's opt.state with rtol 1e-5: the coefficient is an fp32 quotient of a binary64 norm (relative
    error about 2e-7; torch's own fp32 norm is 5.7e-07 from the binary64 one on these gradients); the factor 0.5 clipping
    applies is far outside.  exp_avg is a signed sum of three terms of size <= (1 - beta1) max|g| that may cancel, each
    with fp32 rounding of its own size: next to the relative bound stands 4 * 2^-24 * 0.1 * max|g| absolute.  param
    within 2e-6.  Clipping does not show in param after a single first step (Adam normalises): hence three steps and
    the moment buffers.  grad_scale 0.5: the norm that is clipped is the scaled one.  exp_avg_sq against torch's state:
    test_clipping_exp_avg_sq_matches_torch_state; here also against the plain launch fed torch's clipped gradients."""
    c = clip_case
    p, m, v, guard = _clipped_run(ops, c, grad_scale)
    atol_m = 4 * 2.0 ** -24 * 0.1 * max(float(g.abs().max()) for g in c["grads"])
    d_m = (m.cpu() - c["m"]).abs()
    print(f"clip x{grad_scale}: exp_avg max abs diff {float(d_m.max()):.3e} (atol {atol_m:.3e}), "
          f"param max abs diff {max_abs(p.cpu(), c['p']):.3e}")
    assert torch.allclose(m.cpu(), c["m"], rtol=1e-5, atol=atol_m)
    assert max_abs(p.cpu(), c["p"]) < 2e-6
    # the clipping itself: the same update code (ops.adamw_step) on the gradients clip_grad_norm_ left
    pq, mq, vq = c["p0"].clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    for step, g in enumerate(c["clipped"], 1):
        ops.adamw_step(pq, g.to(DEV), mq, vq, step, LR, betas=BETAS)
    rel = float(((v - vq).abs() / vq).max())
    print(f"clip x{grad_scale}: exp_avg_sq max rel diff to the plain launch on torch's clipped gradients {rel:.3e}")
    assert torch.allclose(v, vq, rtol=1e-5, atol=0.0) and torch.allclose(m, mq, rtol=1e-5, atol=atol_m)
    # the last step's norm as the record holds it
    sumsq = _record(guard)[0]
    want = float(c["grads"][2].double().norm())
    assert abs(grad_scale * math.sqrt(sumsq) - want) <= 1e-6 * want


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipping_exp_avg_sq_matches_torch_state(ops, clip_case, grad_scale):
    """exp_avg_sq against torch's opt.state after clip_grad_norm_ + AdamW, rtol 1e-5 and no absolute term (a sum of
    non-negative terms): the coefficient's relative error, squared into v.  Both sides run at BETAS (see there)."""
    c = clip_case
    _, _, v, _ = _clipped_run(ops, c, grad_scale)
    rel = float(((v.cpu() - c["v"]).abs() / c["v"]).max())
    rel_dec = float(((v.cpu() - c["v_decimal"]).abs() / c["v_decimal"]).max())
    print(f"clip x{grad_scale}: exp_avg_sq max rel diff to torch at the same fp32 betas {rel:.3e} (bound 1e-05); to torch "
          f"at the decimal betas (0.9, 0.999), which the fp32 ABI cannot carry, {rel_dec:.3e}")
    assert torch.allclose(v.cpu(), c["v"], rtol=1e-5, atol=0.0)


def test_a_bound_above_every_norm_changes_no_bit(ops, clip_case):
    c = clip_case
    pa, ma, va = c["p0"].clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    pb, mb, vb = c["p0"].clone().to(DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    guard, ws = _new_guard(ops, N)
    for step, g in enumerate(c["grads"], 1):
        gd = g.to(DEV)
        ops.adamw_step(pa, gd, ma, va, step, LR, betas=BETAS)
        ops.grad_guard(gd, guard, ws, False)
        ops.adamw_step_guarded(pb, gd, mb, vb, step, LR, betas=BETAS, guard=guard, max_grad_norm=1e6)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(ma.cpu(), c["m"])                    # and the clipped run did differ


# ----------------------------------------------------------------------------- 5. engine, eager and captured
def _batch(rank):
    B, T = 2, CFG["clip_len"]
    frames = t(synth.uint8_clip(1300 + rank, (B, T, 3, 64, 64)))
    lab, labD = synth.labels(1400 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
    return frames, t(lab).long(), t(labD).float()


def _engine(device=DEV):
    from tdeed_amd.trainer import TrainEngine
    sd = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}
    eng = TrainEngine(CFG, sd, act_dtype=torch.float32, device=device, lr=1e-3)
    eng.opt.set_guard(skip_nonfinite=True)
    return eng


@pytest.fixture(scope="module")
def twin_params():
    """parameters of a twin engine that only ran the finite step B (eager)"""
    eng = _engine()
    frames, lab, labD = _batch(0)
    eng.step(frames.to(DEV), lab.to(DEV), labD.to(DEV))
    torch.cuda.synchronize()
    assert eng.opt.guard_stats()["skipped"] == 0
    return {k: eng.state[k].detach().cpu().numpy().copy() for k in eng.params.index}


@pytest.mark.parametrize("graph", [False, True])
def test_engine_skips_a_nan_labelD_step_and_goes_on(twin_params, graph):
    """Step A: one NaN in labelD -> part of the gradient buffer is non-finite, part finite; every parameter keeps its
    bits.  Step B (finite) then equals the twin's single step within the DP test's bound 2e-7 + 1e-6 max|w|."""
    eng = _engine()
    frames, lab, labD = (x.to(DEV) for x in _batch(0))
    bad = labD.clone()
    bad[0, 2] = float("nan")
    start = eng.params.flat.clone()
    if graph:
        labD_in = bad.clone()                                    # the step re-reads it into the graph's static labelD
        step = eng.make_step(frames.shape[0], 64, 64, frames, lab, labD_in, None, use_graph=True)
        run_a = step
        def run_b():
            labD_in.copy_(labD)
            step()
    else:
        run_a = lambda: eng.step(frames, lab, bad)               # noqa: E731
        run_b = lambda: eng.step(frames, lab, labD)              # noqa: E731
    run_a()
    torch.cuda.synchronize()
    fin = torch.isfinite(eng.params.grad)
    assert bool(fin.any()) and not bool(fin.all())
    assert torch.equal(eng.params.flat, start)
    assert bool((eng.opt.exp_avg == 0).all()) and bool((eng.opt.exp_avg_sq == 0).all())
    st = eng.opt.guard_stats()
    assert st["skipped"] == 1 and st["last_nonfinite"] and eng.opt.t == 1
    run_b()
    torch.cuda.synchronize()
    st = eng.opt.guard_stats()
    assert st["skipped"] == 1 and not st["last_nonfinite"] and math.isfinite(st["last_norm"]) and eng.opt.t == 2
    for k in eng.params.index:
        got, want = eng.state[k].detach().cpu().numpy(), twin_params[k]
        assert np.abs(got - want).max() <= 2e-7 + 1e-6 * np.abs(want).max(), k
    assert not torch.equal(eng.params.flat, start)


# ----------------------------------------------------------------------------- 6. public interface
def test_get_optimizer_skip_nonfinite_survives_a_bad_batch():
    """epoch([good, bad]) with skip_nonfinite leaves parameters() bit-equal to a twin after epoch([good]); the scheduler
    stepped twice; the returned mean loss is nan like the reference's.  Control: the plain optimizer ends non-finite."""
    from tdeed_amd import augment
    from tdeed_amd.model import TDEEDModel
    meta, _ = load_golden("tiny_rny002_gsf")
    cfg = meta["cfg"]
    clip = synth.uint8_clip(meta["seed_x"], (meta["B"], cfg["clip_len"], 3, meta["H"], meta["W"]))
    lab, labD = synth.labels(3, meta["B"], cfg["clip_len"], cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.3)
    good = dict(frame=t(clip), label=t(lab), labelD=t(labD).float())
    labD_bad = t(labD).float().clone()
    labD_bad[0, 1] = float("nan")
    bad = dict(frame=t(clip), label=t(lab), labelD=labD_bad)

    def run(opt_args, loader):
        m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
        m.load({k: t(v) for k, v in model_state(cfg, meta["seed_w"]).items()})
        m._model.augment_fn = augment.crop_only
        optimizer, scaler = m.get_optimizer(opt_args)
        assert scaler is None
        sched = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=0.01, end_factor=1.0, total_iters=4)
        torch.manual_seed(4321)                                  # the dropout draws of the heads
        loss = m.epoch(loader, optimizer=optimizer, lr_scheduler=sched)
        return m, optimizer, sched, loss

    m, optimizer, sched, loss = run({"lr": 3e-4, "skip_nonfinite": True}, [good, bad])
    twin, opt_t, _, loss_t = run({"lr": 3e-4}, [good])
    assert math.isnan(loss) and math.isfinite(loss_t)
    for a, b in zip(m._model.parameters(), twin._model.parameters()):
        assert torch.equal(a, b)
    assert optimizer.guard_stats()["skipped"] == 1 and optimizer.engine.opt.t == 2
    assert sched.last_epoch == 2
    assert optimizer.param_groups[0]["skip_nonfinite"] is True and optimizer.param_groups[0]["max_grad_norm"] is None
    assert opt_t.engine.opt.guard is None                        # the plain form allocates and launches nothing new
    # the optimizer's state travels next to torch's param_groups
    sd = optimizer.state_dict()
    assert (sd["fused"]["t"], sd["fused"]["skipped"]) == (2, 1) and sd["param_groups"][0]["skip_nonfinite"] is True
    optimizer.load_state_dict(sd)
    assert optimizer.guard_stats()["skipped"] == 1
    # control: what one bad batch does to the plain optimizer
    ctl, _, _, _ = run({"lr": 3e-4}, [good, bad])
    assert not all(bool(torch.isfinite(p).all()) for p in ctl._model.parameters())


# ----------------------------------------------------------------------------- 8. two ranks on one GPU over gloo
def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from tdeed_amd import dist as tdist
    torch.cuda.set_device(0)                                     # both ranks share the one GPU
    tdist.init(backend="gloo")
    eng = _engine("cuda:0")
    assert eng.set_reducer("auto") is not None
    start = eng.params.flat.clone()
    frames, lab, labD = (x.to("cuda:0") for x in _batch(rank))
    bad = labD.clone()
    if rank == 1:
        bad[1, 3] = float("nan")                                 # only rank 1's batch is damaged
    eng.step(frames, lab, bad)
    torch.cuda.synchronize()
    skipped = eng.opt.guard_stats()["skipped"]
    unchanged = bool(torch.equal(eng.params.flat, start))
    eng.step(frames, lab, labD)
    torch.cuda.synchronize()
    q.put((rank, skipped, unchanged, eng.opt.guard_stats()["skipped"], eng.params.flat.detach().cpu().numpy(),
           bool(torch.equal(eng.params.flat, start))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decision_without_another_collective():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, skipped, unchanged, skipped2, flat, still in res:
        assert skipped == 1 and unchanged, rank                 # the all-reduce spread rank 1's NaN; both ranks skipped
        assert skipped2 == 1 and not still and np.isfinite(flat).all(), rank
    assert np.array_equal(res[0][4], res[1][4])
