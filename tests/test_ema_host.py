"""Weight EMA of the fused AdamW on the CPU: the restatement `optim.ema_ref` against the closed form, the warmup
schedule, the argument checks, ema_step0, the averaged state's keys and order, and the optimizer's state_dict without
EMA.  No GPU, no kernel launch."""
import numpy as np
import pytest
import torch

from helpers import t
from tdeed_amd import state_layout, synth
from tdeed_amd.optim import (FlatParams, FusedAdamW, check_ema, ema_decay_at, ema_ref, ema_stat_layout, ema_state_map)

# the tiny 200MF config of tests/test_gpu_param_groups.py
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)


def _state():
    return {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}


# ----------------------------------------------------------------------------- 1. the arithmetic
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_ema_ref_follows_the_closed_form(decay):
    """Constant p, no warmup: after n updates e_n = p - d^n (p - e_0).  Bound 5 n 2^-24 max(|p|, |e_0|): three roundings
    per step on quantities bounded by 2M, 2M and M (M = max(|p|, |e_0|); e stays between e_0 and p), each at most half an ulp
    = 2^-24 relative, i.e. 2.5 M 2^-24 per step against the fp32 d; the errors of earlier steps contract by d <= 1.  The
    closed form uses float32(decay), the d every layer uses."""
    rng = np.random.default_rng(5)
    p = torch.from_numpy(rng.standard_normal(4096).astype(np.float32))
    e0 = torch.from_numpy(rng.standard_normal(4096).astype(np.float32))
    e = e0.clone()
    d = float(np.float32(decay))
    M = torch.maximum(p.abs(), e0.abs()).double()
    worst = 0.0
    for n in range(1, 201):
        out = ema_ref(e, p, n, decay, False)
        assert out is e and e.dtype == torch.float32
        want = p.double() - d ** n * (p.double() - e0.double())
        err = (e.double() - want).abs()
        worst = max(worst, float((err / (5 * n * 2.0 ** -24 * M)).max()))
        assert bool((err <= 5 * n * 2.0 ** -24 * M).all()), (n, float(err.max()))
    print(f"ema_ref vs closed form, decay {decay}: worst error / bound over n = 1..200: {worst:.3f}")
    assert not torch.equal(e, e0)


def test_ema_ref_is_three_separate_roundings():
    """One update equals float32 arithmetic spelled out in numpy, element by element: no fused multiply-add."""
    rng = np.random.default_rng(6)
    p = rng.standard_normal(1000).astype(np.float32)
    e = rng.standard_normal(1000).astype(np.float32)
    w = np.float32(1.0) - np.float32(0.999)
    want = e + w * (p - e)
    assert want.dtype == np.float32
    got = ema_ref(torch.from_numpy(e.copy()), torch.from_numpy(p), 1, 0.999, False)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


# ----------------------------------------------------------------------------- 2. the warmup schedule
def test_warmup_schedule_and_its_crossing():
    d = 0.999
    for n, want in ((1, 2.0 / 11.0), (2, 3.0 / 12.0), (10, 11.0 / 20.0)):
        got = ema_decay_at(n, d, True)
        assert got.dtype == torch.float32
        assert float(got) == float(np.float32(np.float32(1 + n) / np.float32(10 + n))), n
        assert abs(float(got) - want) <= 2.0 ** -24 * want, n
    # (1 + n) / (10 + n) >= 0.999 from n = 8990 on: below it the ramp, from there float32(decay)
    assert float(ema_decay_at(1000, d, True)) == float(np.float32(np.float32(1001) / np.float32(1010)))
    assert float(ema_decay_at(8989, d, True)) < float(np.float32(d))
    assert float(ema_decay_at(8990, d, True)) == float(np.float32(d))
    assert float(ema_decay_at(10 ** 6, d, True)) == float(np.float32(d))
    # a small decay is reached at once: (1 + 1) / (10 + 1) > 0.1
    assert float(ema_decay_at(1, 0.1, True)) == float(np.float32(0.1))
    for n in (1, 2, 10, 1000):
        assert float(ema_decay_at(n, d, False)) == float(np.float32(d))
    # the shadow moves by exactly w = 1 - d_n of the distance at n = 1
    e = ema_ref(torch.zeros(3), torch.ones(3), 1, d, True)
    assert float(e[0]) == float(np.float32(1.0) - np.float32(np.float32(2) / np.float32(11)))
    with pytest.raises(ValueError, match="from 1"):
        ema_decay_at(0, d, True)


# ----------------------------------------------------------------------------- 3. argument errors
@pytest.mark.parametrize("decay, warmup", [(0.0, False), (-0.5, False), (1.0, False), (1.5, True), (float("nan"), False),
                                           ("0.9", False), (True, False), (0.9, 1), (0.9, None), (0.9, "yes"),
                                           (1.0 - 1e-12, False)])
def test_argument_errors(decay, warmup):
    with pytest.raises(ValueError, match="ema_"):
        check_ema(decay, warmup)
    opt = FusedAdamW(FlatParams(_state(), "cpu"), 1e-3)
    with pytest.raises(ValueError, match="ema_"):
        opt.set_ema(decay, warmup)
    assert opt.ema is None and opt.ema_decay is None
    with pytest.raises(ValueError, match="ema_"):
        ema_ref(torch.zeros(4), torch.zeros(4), 1, decay, warmup)


def test_set_ema_copies_the_flat_buffer_and_none_drops_it():
    opt = FusedAdamW(FlatParams(_state(), "cpu"), 1e-3)
    assert opt.ema is None
    opt.set_ema(0.999, warmup=True)
    assert torch.equal(opt.ema, opt.p.flat) and opt.ema.data_ptr() != opt.p.flat.data_ptr()
    assert (opt.ema_decay, opt.ema_warmup, opt.ema_step0) == (0.999, True, 0)
    shadow = opt.ema
    opt.set_ema(0.99)                                            # again: only the two settings change
    assert opt.ema is shadow and (opt.ema_decay, opt.ema_warmup) == (0.99, False)
    opt.set_ema(None)
    assert opt.ema is None and opt.ema_decay is None and opt.ema_warmup is False


# ----------------------------------------------------------------------------- 4. ema_step0
def test_ema_step0_counts_applied_steps_when_switched_on_late():
    opt = FusedAdamW(FlatParams(_state(), "cpu"), 1e-3)
    opt.t = 7                                                    # seven attempts so far, none skipped: no record, no sync
    opt.set_ema(0.999)
    assert opt.ema_step0 == 7
    opt.set_ema(None)
    opt.set_guard(skip_nonfinite=True)                           # a record with two skipped steps
    opt.guard[3] = 2
    opt.set_ema(0.999)
    assert opt.ema_step0 == 5
    sd = opt.state_dict()
    assert (sd["ema_step0"], sd["ema_decay"], sd["ema_warmup"], sd["skipped"], sd["t"]) == (5, 0.999, False, 2, 7)
    assert torch.equal(sd["ema"], opt.ema) and sd["ema"].data_ptr() != opt.ema.data_ptr() and sd["ema_stats"] is None
    # ... and comes back into an optimizer that had none
    other = FusedAdamW(FlatParams(_state(), "cpu"), 1e-3)
    sd["ema"] = sd["ema"] + 1.0
    other.load_state_dict(sd)
    assert other.ema_step0 == 5 and other.ema_decay == 0.999 and torch.equal(other.ema, sd["ema"])


# ----------------------------------------------------------------------------- 5. the averaged state
def test_ema_state_keys_and_order_are_the_models():
    """The pure function behind TrainEngine.ema_state() (the engine itself needs the GPU)."""
    shapes = state_layout.model_state_shapes(CFG)
    state = _state()
    live = dict(state)
    params = FlatParams(state, "cpu")
    opt = FusedAdamW(params, 1e-3)
    opt.set_ema(0.999)
    stat_index, total = ema_stat_layout(state)
    stat_keys = [k for k in state if k.endswith(("running_mean", "running_var"))]
    assert list(stat_index) == stat_keys and total == sum(state[k].numel() for k in stat_keys)
    offs = [stat_index[k][0] for k in stat_keys]
    assert offs == sorted(offs) and offs[0] == 0
    stats = torch.cat([state[k].reshape(-1) for k in stat_keys])
    avg = ema_state_map(state, params.index, opt.ema, stat_index, stats)
    assert list(avg) == list(shapes) == list(state)
    for k, (shape, _) in shapes.items():
        assert tuple(avg[k].shape) == tuple(shape), k
        assert torch.equal(avg[k].float(), live[k].float()), k      # the shadows start as copies
        if state_layout.is_parameter(k):
            o, n = params.index[k]
            assert avg[k].data_ptr() == opt.ema[o:].data_ptr() and avg[k].data_ptr() != state[k].data_ptr(), k
        elif k in stat_index:
            assert avg[k].data_ptr() == stats[stat_index[k][0]:].data_ptr(), k
        else:
            assert k.endswith("num_batches_tracked") and avg[k] is state[k], k      # the counters are live


def test_c_entries_check_their_arguments_before_any_launch():
    """The argument checks of both entries run on the host: an error code and a message, no launch (no GPU needed)."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from tdeed_amd._lib import call, HipCallError
    A = 1 << 20                                                  # any 16-byte-aligned non-null address: nothing is launched

    def adamw(step=3, ema=A, decay=0.999, step0=0):
        call("tdeed_adamw_step_ema", A, A, A, A, 1027, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0, None, 0, 0.0, None, 0, ema,
             decay, 1, step0, None)

    for kw, msg in ((dict(decay=0.0), "0 < ema_decay < 1"), (dict(decay=1.0), "0 < ema_decay < 1"),
                    (dict(decay=float("nan")), "0 < ema_decay < 1"), (dict(step0=-1), "ema_step0 >= 0"),
                    (dict(step0=3), "step - ema_step0 >= 1"), (dict(ema=A + 4), "16-byte aligned"),
                    (dict(ema=None), "null pointer"), (dict(step=0), "bad n/step")):
        with pytest.raises(HipCallError, match=msg):
            adamw(**kw)
    rows = np.zeros((2, 4), dtype=np.int32)
    rows[:, :2] = np.array([A, A], dtype=np.uint64).view(np.int32).reshape(-1, 2)
    rows[:, 2] = (0, 24)
    rows[:, 3] = (24, 368)
    host = rows.ctypes.data_as(ctypes.c_void_p)

    def tensors(nrows=2, shadow_n=24 + 368, decay=0.999, step=1, step0=0):
        call("tdeed_ema_tensors", A, host, nrows, A, shadow_n, step, None, 0, decay, 0, step0, None)

    for kw, msg in ((dict(shadow_n=24 + 367), "row 1 .offset 24, count 368. overruns the shadow of 391"),
                    (dict(nrows=0), "1 .. 65535 rows"), (dict(decay=1.0), "0 < ema_decay < 1"),
                    (dict(step=2, step0=2), "step - ema_step0 >= 1")):
        with pytest.raises(HipCallError, match=msg):
            tensors(**kw)
    rows[1, 3] = 0                                               # an empty row
    with pytest.raises(HipCallError, match="row 1"):
        tensors()


# ----------------------------------------------------------------------------- 6. without EMA nothing differs
def test_state_dict_without_ema_has_exactly_the_keys_it_had():
    opt = FusedAdamW(FlatParams(_state(), "cpu"), 1e-3)
    assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "t", "skipped"}
    opt.set_ema(0.999)
    assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "t", "skipped", "ema", "ema_stats", "ema_decay", "ema_warmup",
                                     "ema_step0"}
    opt.set_ema(None)
    assert set(opt.state_dict()) == {"exp_avg", "exp_avg_sq", "t", "skipped"}
    # a state without the EMA keys loads as before and switches nothing on
    other = FusedAdamW(FlatParams(_state(), "cpu"), 1e-3)
    other.load_state_dict(opt.state_dict())
    assert other.ema is None and other.ema_hook is None
