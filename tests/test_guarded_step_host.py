"""The guarded optimizer step on the CPU: `optim.guarded_adamw_ref` (the restatement the GPU tests compare the kernels
with) against torch itself -- GradScaler's skip, clip_grad_norm_'s rule -- plus set_guard's argument checks and the
optimizer-state round trip.  No GPU, no kernel launch."""
import numpy as np
import pytest
import torch

from helpers import act, t
from tdeed_amd.optim import FlatParams, FusedAdamW, guarded_adamw_ref

N = 1027
LR = 8e-4


def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


def _fresh_state(n):
    return dict(exp_avg=torch.zeros(n), exp_avg_sq=torch.zeros(n), t=0, skipped=0)


def test_skip_equals_gradscaler_and_adamw_over_the_good_steps_bit_for_bit():
    """Steps {good, bad (inf), good}: the reference's route (GradScaler.step in front of torch.optim.AdamW) leaves the
    optimizer and its step count alone at the bad one; the restatement must give the same bits, and both must equal
    AdamW over the two good steps alone."""
    p0 = rnd(141, "p", (N,))
    grads = [rnd(151, "g", (N,)), rnd(152, "g", (N,)), rnd(153, "g", (N,))]
    grads[1][N // 3] = float("inf")
    # (a) GradScaler("cpu") + AdamW; init_scale 4.0 is a power of two, so scaling and unscaling are exact
    pa = p0.clone().requires_grad_(True)
    opt_a = torch.optim.AdamW([pa], lr=LR)
    scaler = torch.amp.GradScaler("cpu", init_scale=4.0)
    for g in grads:
        pa.grad = g * scaler.scale(torch.ones(()))               # what backward() of the scaled loss would leave
        scaler.step(opt_a)
        scaler.update()
        opt_a.zero_grad()
    assert int(opt_a.state[pa]["step"]) == 2
    # (b) AdamW over the two good steps alone
    pb = p0.clone().requires_grad_(True)
    opt_b = torch.optim.AdamW([pb], lr=LR)
    for g in (grads[0], grads[2]):
        pb.grad = g.clone()
        opt_b.step()
    assert torch.equal(pa.detach(), pb.detach())
    # (c) the restatement, all three attempts
    pc, st = p0.clone(), _fresh_state(N)
    seen = [guarded_adamw_ref(pc, g, st, LR, skip_nonfinite=True)["nonfinite"] for g in grads]
    assert seen == [False, True, False] and (st["t"], st["skipped"]) == (3, 1)
    assert torch.equal(pc, pa.detach())
    assert torch.equal(st["exp_avg"], opt_a.state[pa]["exp_avg"])
    assert torch.equal(st["exp_avg_sq"], opt_a.state[pa]["exp_avg_sq"])
    # without the guard the same three attempts end in NaN: what opting in removes
    pd, st_d = p0.clone(), _fresh_state(N)
    for g in grads:
        guarded_adamw_ref(pd, g, st_d, LR)
    assert not bool(torch.isfinite(pd).all()) and st_d["skipped"] == 0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipping_rule_matches_clip_grad_norm(grad_scale):
    """Three steps, max_grad_norm at half of step 1's norm and above step 2's.  torch's norm is an fp32 reduction, the
    restatement's a binary64 one rounded to fp32: the coefficients agree to a few fp32 ulp (2e-7 relative), exp_avg
    carries that once and exp_avg_sq twice, hence rtol 1e-5 on the moments; param within the plain AdamW test's 2e-6."""
    p0 = rnd(141, "p", (N,))
    grads = [rnd(151, "g", (N,)), rnd(152, "g", (N,), 0.25), rnd(153, "g", (N,))]
    max_norm = 0.5 * float(grads[0].norm())
    assert float(grads[1].norm()) < max_norm < float(grads[2].norm())
    pa = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pa], lr=LR)
    pc, st = p0.clone(), _fresh_state(N)
    coefs = []
    for g in grads:
        pa.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([pa], max_norm)
        opt.step()
        # the buffer holds g / grad_scale: the norm that is clipped is the one after grad_scale
        coefs.append(guarded_adamw_ref(pc, g / grad_scale, st, LR, grad_scale=grad_scale, max_grad_norm=max_norm)["coef"])
    assert abs(coefs[0] - 0.5) < 1e-6 and coefs[1] == 1.0 and coefs[2] < 1.0
    # exp_avg is a signed sum of three terms of size <= (1 - beta1) max|g| that may cancel: each carries fp32 rounding
    # of its own size, so next to the relative bound stands 4 * 2^-24 * 0.1 * max|g| absolute (4: three terms, one sum)
    atol_m = 4 * 2.0 ** -24 * 0.1 * max(float(g.abs().max()) for g in grads)
    d_m = (st["exp_avg"] - opt.state[pa]["exp_avg"]).abs()
    d_v = (st["exp_avg_sq"] - opt.state[pa]["exp_avg_sq"]).abs()
    print(f"exp_avg max abs diff {float(d_m.max()):.3e} (atol {atol_m:.3e}), exp_avg_sq max rel diff "
          f"{float((d_v / opt.state[pa]['exp_avg_sq']).max()):.3e}")
    assert torch.allclose(st["exp_avg"], opt.state[pa]["exp_avg"], rtol=1e-5, atol=atol_m)
    assert torch.allclose(st["exp_avg_sq"], opt.state[pa]["exp_avg_sq"], rtol=1e-5, atol=0.0)
    assert float((pc - pa.detach()).abs().max()) < 2e-6
    # a bound above every norm: bit-equal to no clipping at all
    pe, st_e = p0.clone(), _fresh_state(N)
    pf, st_f = p0.clone(), _fresh_state(N)
    for g in grads:
        assert guarded_adamw_ref(pe, g, st_e, LR, max_grad_norm=1e9)["coef"] == 1.0
        guarded_adamw_ref(pf, g, st_f, LR)
    assert torch.equal(pe, pf) and torch.equal(st_e["exp_avg_sq"], st_f["exp_avg_sq"])


def test_clipping_without_skipping_poisons_like_torch():
    """clip_grad_norm_(error_if_nonfinite=False) then step(): a NaN norm makes every gradient NaN."""
    p0 = rnd(141, "p", (N,))
    g = rnd(151, "g", (N,))
    g[5] = float("nan")
    pa = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pa], lr=LR)
    pa.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([pa], 1.0)
    opt.step()
    pc, st = p0.clone(), _fresh_state(N)
    guarded_adamw_ref(pc, g, st, LR, max_grad_norm=1.0)
    assert bool(torch.isnan(pa.detach()).all()) and bool(torch.isnan(pc).all())


def _cpu_optimizer(n=40):
    state = {"_pred_fine._fc_out.weight": torch.arange(n, dtype=torch.float32)}
    return FusedAdamW(FlatParams(state, "cpu"), lr=LR)


def test_set_guard_argument_errors():
    opt = _cpu_optimizer()
    assert opt.guard is None
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.set_guard(max_grad_norm=bad)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        opt.set_guard(skip_nonfinite="yes")
    assert opt.guard is None                                     # a refused call allocates nothing
    opt.set_guard()                                              # both off: still the plain step
    assert opt.guard is None and opt.guard_stats() == dict(skipped=0, last_nonfinite=False, last_norm=0.0)
    opt.set_guard(skip_nonfinite=True, max_grad_norm=2)
    assert opt.guard.dtype == torch.int32 and opt.guard.numel() == 8 and int(opt.guard.abs().sum()) == 0
    assert (opt.skip_nonfinite, opt.max_grad_norm) == (True, 2.0)
    rec = opt.guard
    opt.set_guard(skip_nonfinite=True)                           # allocated once
    assert opt.guard is rec and opt.max_grad_norm is None


def test_state_dict_round_trip():
    """The restatement's state IS FusedAdamW.state_dict(): it survives load_state_dict into a fresh optimizer with both
    counters, and a restatement resumed from the copy goes on bit for bit like the one that kept running."""
    n = 64
    p, st = rnd(141, "p", (n,)), _fresh_state(n)
    bad = rnd(152, "g", (n,))
    bad[7] = float("nan")
    for g in (rnd(151, "g", (n,)), bad):
        guarded_adamw_ref(p, g, st, LR, skip_nonfinite=True)
    assert (st["t"], st["skipped"]) == (2, 1)
    opt = _cpu_optimizer(n)
    opt.load_state_dict(st)
    got = opt.state_dict()
    assert sorted(got) == ["exp_avg", "exp_avg_sq", "skipped", "t"]
    assert (got["t"], got["skipped"]) == (2, 1) and opt.t == 2 and opt.guard is not None
    assert torch.equal(got["exp_avg"], st["exp_avg"]) and torch.equal(got["exp_avg_sq"], st["exp_avg_sq"])
    assert got["exp_avg"].data_ptr() != opt.exp_avg.data_ptr()              # clones, not views
    assert opt.guard_stats()["skipped"] == 1
    p2 = p.clone()
    g3 = rnd(153, "g", (n,))
    guarded_adamw_ref(p, g3, st, LR, skip_nonfinite=True)
    guarded_adamw_ref(p2, g3, got, LR, skip_nonfinite=True)
    assert torch.equal(p, p2) and (got["t"], got["skipped"]) == (3, 1)
    assert np.isfinite(p2.numpy()).all()
