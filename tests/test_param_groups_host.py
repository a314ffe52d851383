"""Parameter groups of the fused AdamW on the CPU: the run table (`optim.group_table`), the backward stages a freeze set
leaves (`optim.freeze_plan`) and the restatement `optim.grouped_adamw_ref` against torch.optim.AdamW with real param
groups and a requires_grad_(False) tensor.  No GPU, no kernel launch."""
import fnmatch
import math

import numpy as np
import pytest
import torch

from helpers import act, t
from tdeed_amd import state_layout
from tdeed_amd.optim import (BUCKET_ALIGN, FlatParams, FusedAdamW, check_groups, freeze_plan, frozen_keys, group_table,
                             grouped_adamw_ref, is_late_bucket_key, backward_stages)
from tdeed_amd.regnet_spec import regnet_spec

# the tiny 200MF config of tests/test_gpu_guarded_step.py
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
LR = 8e-4
WD = 0.01
NORMS_AND_BIASES = {"params": ("*.bn.*", "*.ln*", "*.gn.*", "*.bias"), "weight_decay": 0.0}
EXAMPLE = [
    {"params": ("_features.stem.*", "_features.s1.*", "_features.s2.*"), "frozen": True},
    {"params": ("_features.*",), "lr_scale": 0.1},
    NORMS_AND_BIASES,
]


class _Shape:
    def __init__(self, shape):
        self.shape = shape

    def numel(self):
        return int(np.prod(self.shape)) if self.shape else 1


@pytest.fixture(scope="module")
def layout():
    shapes = state_layout.model_state_shapes(CFG)
    lay = FlatParams.layout_only({k: _Shape(s) for k, (s, _) in shapes.items()})
    lay.order = sorted(lay.index, key=lambda k: lay.index[k][0])
    return lay


def _settings_at(runs, off):
    for end, scale, wd, frozen in runs:
        if off < end:
            return scale, wd, frozen
    raise AssertionError(off)


def _check_cover(runs, numel):
    ends = [r[0] for r in runs]
    assert ends == sorted(set(ends)) and ends[-1] == numel and ends[0] > 0
    assert all(e % 4 == 0 for e in ends)
    assert all(a[1:] != b[1:] for a, b in zip(runs, runs[1:]))   # adjacent equal runs were merged


# ----------------------------------------------------------------------------- group_table
def test_no_groups_is_one_run(layout):
    assert group_table(layout.index, layout.numel, None, WD) == [(layout.numel, 1.0, WD, False)]
    assert group_table(layout.index, layout.numel, [], WD) == [(layout.numel, 1.0, WD, False)]
    assert layout.numel % BUCKET_ALIGN == 0 and len(layout.index) == 431


def test_runs_cover_the_buffer_and_follow_the_first_matching_group(layout):
    runs = group_table(layout.index, layout.numel, EXAMPLE, WD)
    _check_cover(runs, layout.numel)
    for k, (off, n) in layout.index.items():
        got = _settings_at(runs, off)
        assert got == _settings_at(runs, off + n - 1), k          # a tensor lies in one run
        if k.startswith(("_features.stem.", "_features.s1.", "_features.s2.")):
            want = (1.0, WD, True)                                # group 0, although groups 1 and 2 match as well
        elif k.startswith("_features."):
            want = (0.1, WD, False)                               # group 1 wins over group 2 for the trunk's BatchNorms
        elif any(fnmatch.fnmatchcase(k, p) for p in NORMS_AND_BIASES["params"]):
            want = (1.0, 0.0, False)
        else:
            want = (1.0, WD, False)                               # unmatched: the optimizer's defaults
        assert got == want, k
    assert _settings_at(runs, layout.index["temp_enc"][0]) == (1.0, WD, False)
    assert _settings_at(runs, layout.index["_features.s3.b1.conv2.bn.weight"][0]) == (0.1, WD, False)
    assert _settings_at(runs, layout.index["_temp_fine._sgp.0.ln.weight"][0]) == (1.0, 0.0, False)
    assert _settings_at(runs, layout.index["_temp_fine._sgp.0.mlp.0.weight"][0]) == (1.0, WD, False)


def test_third_group_alone_gives_a_run_per_tensor_or_two(layout):
    runs = group_table(layout.index, layout.numel, [NORMS_AND_BIASES], WD)
    _check_cover(runs, layout.numel)
    assert len(layout.index) // 4 < len(runs) <= len(layout.index)
    assert {r[1:] for r in runs} == {(1.0, WD, False), (1.0, 0.0, False)}
    # default_wd None stands for "the launch's decay" (what FusedAdamW uploads)
    runs_none = group_table(layout.index, layout.numel, [NORMS_AND_BIASES], None)
    assert [r[0] for r in runs_none] == [r[0] for r in runs] and {r[2] for r in runs_none} == {None, 0.0}


def test_padding_belongs_to_the_run_in_front(layout):
    """One group per side of each padded gap: the run of the tensor in front ends where the next tensor starts, so the
    4-element padding, the BUCKET_ALIGN padding at the bucket boundary and the padding at the end ride with it."""
    order = layout.order
    first_late = next(k for k in order if is_late_bucket_key(k))
    before = order[order.index(first_late) - 1]
    assert layout.index[first_late][0] % BUCKET_ALIGN == 0
    gap = layout.index[first_late][0] - sum(layout.index[before])
    assert gap >= 0
    runs = group_table(layout.index, layout.numel, [{"params": (before,), "lr_scale": 0.5}], WD)
    _check_cover(runs, layout.numel)
    ends = {r[0]: r[1:] for r in runs}
    assert ends[layout.index[first_late][0]] == (0.5, WD, False)  # `before`'s run reaches the bucket boundary
    assert layout.index[before][0] in ends or layout.index[before][0] == 0
    # an odd-sized tensor: its run ends at the next tensor's offset, not at its own last element
    odd = next(k for k in order[:-1] if layout.index[k][1] % 4)
    nxt = order[order.index(odd) + 1]
    runs = group_table(layout.index, layout.numel, [{"params": (odd,), "frozen": True}], WD)
    assert (layout.index[nxt][0], 1.0, WD, True) in runs and sum(layout.index[odd]) < layout.index[nxt][0]
    # the last tensor's run takes the padding at the end of the buffer
    last = order[-1]
    runs = group_table(layout.index, layout.numel, [{"params": (last,), "weight_decay": 0.5}], WD)
    assert runs[-1] == (layout.numel, 1.0, 0.5, False) and runs[-2][0] == layout.index[last][0]


def test_adjacent_tensors_with_equal_settings_merge(layout):
    runs = group_table(layout.index, layout.numel, [{"params": ("_features.*",), "frozen": True, "lr_scale": 0.3}], WD)
    first_late = min(o for k, (o, n) in layout.index.items() if is_late_bucket_key(k))
    assert runs == [(layout.index["_features.stem.conv.weight"][0], 1.0, WD, False), (first_late, 1.0, WD, True),
                    (layout.numel, 1.0, WD, False)]
    # two groups with the same settings merge across the group boundary
    two = [{"params": ("_features.s1.*",), "lr_scale": 0.5}, {"params": ("_features.s2.*",), "lr_scale": 0.5}]
    runs = group_table(layout.index, layout.numel, two, WD)
    assert [r[1] for r in runs] == [1.0, 0.5, 1.0]


def test_group_errors(layout):
    idx, n = layout.index, layout.numel
    with pytest.raises(ValueError, match=r"_featurs\.\*.*matches no parameter"):
        group_table(idx, n, [{"params": ("_featurs.*",), "frozen": True}], WD)
    with pytest.raises(ValueError, match="running_mean.*matches no parameter"):
        group_table(idx, n, [{"params": ("*.running_mean",)}], WD)          # buffers are not parameters
    with pytest.raises(ValueError, match="unknown key.*betas"):
        group_table(idx, n, [{"params": ("_features.*",), "betas": (0.9, 0.99)}], WD)
    with pytest.raises(ValueError, match="'params'"):
        group_table(idx, n, [{"lr_scale": 0.1}], WD)
    for key in ("lr_scale", "weight_decay"):
        for bad in (-0.1, float("nan"), float("inf"), "0.1", True):
            with pytest.raises(ValueError, match=key):
                group_table(idx, n, [{"params": ("_features.*",), key: bad}], WD)
    with pytest.raises(ValueError, match="frozen"):
        group_table(idx, n, [{"params": ("_features.*",), "frozen": 1}], WD)
    assert check_groups([{"params": "temp_enc", "lr_scale": 0}]) == ((("temp_enc",), 0.0, None, False),)


def test_fused_adamw_set_groups_on_the_host():
    """set_groups builds the runs, names the frozen tensors and zeroes their gradient ranges; None returns to the plain
    launch.  (CPU buffers: no table is uploaded and step() is not called.)"""
    state = {"temp_enc": torch.ones(6, 8), "_features.stem.conv.weight": torch.ones(5), "_pred_fine._fc_out.weight": torch.ones(7)}
    fp = FlatParams(state, "cpu")
    opt = FusedAdamW(fp, lr=LR)
    assert opt.groups is None and opt.run_table is None and opt.frozen == frozenset()
    fp.grad.fill_(3.0)
    opt.set_groups([{"params": ("_features.*",), "frozen": True}])
    assert opt.frozen == {"_features.stem.conv.weight"}
    assert float(fp.grad_view("_features.stem.conv.weight").abs().sum()) == 0.0 and float(fp.grad_view("temp_enc").min()) == 3.0
    assert [r[3] for r in opt.runs] == [False, True, False] and opt.runs[-1][0] == fp.numel
    assert opt.groups == [{"params": ("_features.*",), "lr_scale": 1.0, "frozen": True}]
    opt.set_groups(None)
    assert opt.groups is None and opt.runs is None and opt.frozen == frozenset()


# ----------------------------------------------------------------------------- freeze_plan
@pytest.fixture(scope="module")
def plan_case(layout):
    spec = regnet_spec(CFG["feature_arch"])
    return spec, list(layout.index), backward_stages(spec)


def _plan(plan_case, patterns):
    spec, keys, _ = plan_case
    fz = frozen_keys(keys, [{"params": tuple(patterns), "frozen": True}]) if patterns else frozenset()
    return freeze_plan(spec, fz, keys)


def test_freeze_plan(plan_case):
    spec, keys, stages = plan_case
    assert stages[:3] == ["temporal", "temp_enc", "s4.b7"] and stages[-2:] == ["s1.b1", "stem"] and len(stages) == 16
    assert _plan(plan_case, ()) == stages                                        # nothing frozen: every stage
    assert _plan(plan_case, ("_features.*",)) == ["temporal", "temp_enc"]
    assert _plan(plan_case, ("_features.*", "temp_enc")) == ["temporal"]
    got = _plan(plan_case, ("_features.stem.*", "_features.s1.*", "_features.s2.*"))
    assert got == stages[:stages.index("s3.b1") + 1] and got[-1] == "s3.b1"
    # only the heads (or the whole temporal stack) frozen: the trunk still needs d_feat, every stage runs
    assert _plan(plan_case, ("_pred_*",)) == stages
    assert _plan(plan_case, ("_temp_fine.*", "_pred_*")) == stages
    # a frozen block between trainable ones still runs: the gradient passes through it
    assert _plan(plan_case, ("_features.s3.b2.*", "_features.s4.*")) == stages
    assert _plan(plan_case, ("_features.stem.*", "_features.s3.*")) == stages[:-1]
    # one trainable tensor keeps its stage and everything in front of it
    fz = frozenset(k for k in keys if k.startswith("_features.") and k != "_features.s2.b1.se.fc1.bias")
    assert freeze_plan(spec, fz, keys)[-1] == "s2.b1"
    assert freeze_plan(spec, frozenset(keys), keys) == []


# ----------------------------------------------------------------------------- grouped_adamw_ref against torch
def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


def test_restatement_matches_torch_adamw_with_param_groups():
    """Four runs -- default, lr_scale 0.1 with its own decay, frozen, no decay -- over three steps against
    torch.optim.AdamW with one param group per run and a requires_grad_(False) tensor.  Bound: max abs 2e-6 at lr 8e-4 on
    unit-scale parameters, what tests/test_gpu_ops.py::test_adamw_step_matches_torch_optim holds the plain launch to;
    lr_scale <= 1 only shrinks the update, so the bound carries over."""
    sizes = [40, 24, 16, 20]
    runs = [(40, 1.0, None, False), (64, 0.1, 0.05, False), (80, 1.0, None, True), (100, 1.0, 0.0, False)]
    n = sum(sizes)
    p0 = rnd(141, "p", (n,))
    grads = [rnd(151 + s, "g", (n,)) for s in range(3)]
    parts = [p0[lo:hi].clone().requires_grad_(True) for lo, hi in ((0, 40), (40, 64), (64, 80), (80, 100))]
    parts[2].requires_grad_(False)
    ref = torch.optim.AdamW([dict(params=[parts[0]]), dict(params=[parts[1]], lr=LR * 0.1, weight_decay=0.05),
                             dict(params=[parts[3]], weight_decay=0.0)], lr=LR, weight_decay=WD)
    p = p0.clone()
    st = dict(exp_avg=torch.zeros(n), exp_avg_sq=torch.zeros(n), t=0, skipped=0)
    for g in grads:
        for part, (lo, hi) in zip(parts, ((0, 40), (40, 64), (64, 80), (80, 100))):
            part.grad = g[lo:hi].clone() if part.requires_grad else None
        ref.step()
        g_in = g.clone()
        g_in[64:80] = 0.0                                        # a frozen range of the flat gradient buffer holds zeros
        out = grouped_adamw_ref(p, g_in, st, runs, LR, weight_decay=WD)
        assert not out["nonfinite"] and abs(out["norm"] - float(g_in.double().norm())) < 1e-5
    want = torch.cat([x.detach() for x in parts])
    err = float((p - want).abs().max())
    print(f"grouped_adamw_ref vs torch.optim.AdamW with param groups: max abs {err:.3e}")
    assert err < 2e-6
    assert torch.equal(p[64:80], p0[64:80])                      # the frozen run keeps its bits, moments included
    assert float(st["exp_avg"][64:80].abs().sum()) == 0.0 and float(st["exp_avg_sq"][64:80].abs().sum()) == 0.0
    assert st["t"] == 3 and not torch.equal(p[:64], p0[:64]) and not torch.equal(p[80:], p0[80:])
    # the scaled run really stepped at a tenth of the rate, the decayed run really decayed
    assert float((p[40:64] - p0[40:64]).abs().max()) < 0.2 * float((p[:40] - p0[:40]).abs().max())


def test_restatement_neutral_runs_equal_the_unsplit_restatement_bit_for_bit():
    from tdeed_amd.optim import guarded_adamw_ref
    n = 100
    p0, g = rnd(141, "p", (n,)), rnd(151, "g", (n,))
    pa, sa = p0.clone(), dict(exp_avg=torch.zeros(n), exp_avg_sq=torch.zeros(n), t=0, skipped=0)
    pb, sb = p0.clone(), dict(exp_avg=torch.zeros(n), exp_avg_sq=torch.zeros(n), t=0, skipped=0)
    max_norm = 0.5 * float(g.norm())
    for _ in range(2):
        ra = guarded_adamw_ref(pa, g, sa, LR, weight_decay=WD, max_grad_norm=max_norm)
        rb = grouped_adamw_ref(pb, g, sb, [(36, 1.0, None, False), (100, 1.0, WD, False)], LR, weight_decay=WD,
                               max_grad_norm=max_norm)
        assert ra == rb and math.isclose(ra["coef"], 0.5, rel_tol=1e-5)      # ONE global coefficient
    assert torch.equal(pa, pb) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and sa["t"] == sb["t"] == 2
    bad = g.clone()
    bad[50] = float("inf")
    before = pb.clone()
    assert grouped_adamw_ref(pb, bad, sb, [(36, 1.0, None, False), (100, 0.5, WD, False)], LR, skip_nonfinite=True)["nonfinite"]
    assert torch.equal(pb, before) and (sb["t"], sb["skipped"]) == (3, 1)   # a skipped step writes nothing in any run
