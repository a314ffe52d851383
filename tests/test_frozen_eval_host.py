"""The frozen eval-mode prefix on the CPU: which stages `optim.eval_prefix` gives a freeze set, the `frozen_stats` keyword of
HipAdamW / set_groups (where it sits, how it travels in state_dict()), and the proof that the rounding bound
tests/test_gpu_frozen_eval.py holds the stem's eval instance to contains a correct kernel's output.  No GPU, no launch."""
import pytest
import torch

import frozen_eval_cases as C
import roundoff as R
from tdeed_amd import state_layout
from tdeed_amd.optim import (GROUP_KEYS, FlatParams, FusedAdamW, check_frozen_stats, checked_eval_prefix, eval_prefix,
                             forward_stages, frozen_keys)
from tdeed_amd.regnet_spec import regnet_spec


def _case(arch):
    cfg = dict(C.CFG, feature_arch=arch)
    keys = [k for k in state_layout.model_state_shapes(cfg) if state_layout.is_parameter(k)]
    return regnet_spec(arch), keys


def _prefix(arch, patterns):
    spec, keys = _case(arch)
    return eval_prefix(spec, frozen_keys(keys, [{"params": patterns, "frozen": True}]), keys)


@pytest.mark.parametrize("arch", ["rny002_gsf", "rny008_gsf"])
def test_eval_prefix(arch):
    spec, keys = _case(arch)
    stages = forward_stages(spec)
    assert stages[0] == "stem" and stages[1] == "s1.b1" and len(stages) == len(spec.blocks) + 1
    assert _prefix(arch, ("_features.*",)) == stages                              # temp_enc is never part of it
    assert _prefix(arch, ("_features.*", "temp_enc")) == stages
    front = [s for s in stages if s == "stem" or s.startswith(("s1.", "s2."))]
    assert _prefix(arch, ("_features.stem.*", "_features.s1.*", "_features.s2.*")) == front
    assert front[-1].startswith("s2.") and stages[len(front)] == "s3.b1"
    assert _prefix(arch, ("_features.s1.*",)) == []                               # the stem still trains
    with_hole = _prefix(arch, ("_features.stem.*", "_features.s1.*", "_features.s3.b1.*"))
    assert with_hole == [s for s in stages if s == "stem" or s.startswith("s1.")]  # s3.b1 sits behind a trainable stage
    assert _prefix(arch, ("_features.stem.*",)) == ["stem"]
    # one trainable tensor inside a stage takes the stage out
    some = [k for k in keys if k.startswith("_features.s1.b1.") and k.endswith("bn.bias")][0]
    frozen = frozen_keys(keys, [{"params": ("_features.*",), "frozen": True}]) - {some}
    assert eval_prefix(spec, frozen, keys) == ["stem"]
    assert eval_prefix(spec, frozenset(), keys) == []


def test_the_cases_of_the_gpu_tests_are_the_prefixes_they_name():
    spec, keys = _case(C.CFG["feature_arch"])
    stages = forward_stages(spec)
    n = {p: C.n_eval_stages(p) for p in C.PREFIXES}
    assert n["stem"] == 1 and stages[n["s1"]].startswith("s2.") and stages[n["s2"]] == "s3.b1"
    assert stages[n["s3mid"] - 1] == "s3.b2" and stages[n["s3mid"]] == "s3.b3" and n["trunk"] == len(stages)
    blk = {b.name: b for b in spec.blocks}
    assert blk["s3.b1"].gsf_fold > 0 and blk["s3.b2"].gsf_fold > 0 and blk["s3.b3"].gsf_fold > 0 and blk["s2.b1"].gsf_fold == 0


def test_frozen_stats_values():
    assert check_frozen_stats("batch") == "batch" and check_frozen_stats("eval") == "eval"
    for bad in ("Eval", "running", None, True, 1):
        with pytest.raises(ValueError, match="frozen_stats"):
            check_frozen_stats(bad)
    assert "frozen_stats" not in GROUP_KEYS                      # a keyword of the optimizer, not a key of a group
    spec, keys = _case(C.CFG["feature_arch"])
    frozen = frozen_keys(keys, [{"params": ("_features.s1.*",), "frozen": True}])
    assert checked_eval_prefix(spec, frozen, keys, "batch") == ()
    with pytest.raises(ValueError, match="empty eval prefix"):
        checked_eval_prefix(spec, frozen, keys, "eval")
    with pytest.raises(ValueError, match="frozen_stats"):
        checked_eval_prefix(spec, frozen, keys, "train")
    frozen = frozen_keys(keys, C.groups("s2"))
    assert checked_eval_prefix(spec, frozen, keys, "eval") == tuple(forward_stages(spec)[:C.n_eval_stages("s2")])
    assert checked_eval_prefix(spec, frozen, keys, "batch") == ()


def _host_engine():
    """A TrainEngine without its device half: the real FlatParams / FusedAdamW / set_groups over the model's state on the CPU;
    packing the prefix's weights needs the device and is counted instead."""
    from tdeed_amd.trainer import TrainEngine

    class HostEngine(TrainEngine):
        def __init__(self):
            self.cfg, self.device, self.dt = dict(C.CFG), "cpu", torch.float32
            self.state = C.start_state()
            self.params = FlatParams(self.state, "cpu")
            self.opt = FusedAdamW(self.params, 1e-3)
            self.spec = regnet_spec(C.CFG["feature_arch"])
            self.reducer, self.frozen, self.stages = None, frozenset(), None
            self.frozen_stats, self.eval_prefix, self.prefix, self.prefix_gen = "batch", (), None, 0
            self.reloads = 0

        def reload_prefix(self):
            self.reloads += 1
            self.prefix = "packed" if self.eval_prefix else None

    return HostEngine()


def test_hip_adamw_keyword_and_state_dict_round_trip():
    from tdeed_amd.trainer import HipAdamW
    eng = _host_engine()
    opt = HipAdamW(eng, lr=1e-3, groups=C.groups("s2"))
    assert "frozen_stats" not in opt.param_groups[0] and eng.eval_prefix == () and eng.frozen_stats == "batch"
    assert eng.reloads == 0 and "frozen_stats" not in opt.state_dict()["param_groups"][0]
    with pytest.raises(ValueError, match="frozen_stats"):
        HipAdamW(_host_engine(), lr=1e-3, groups=C.groups("s2"), frozen_stats="running")
    with pytest.raises(ValueError, match="empty eval prefix"):
        HipAdamW(_host_engine(), lr=1e-3, frozen_stats="eval")   # nothing frozen
    with pytest.raises(ValueError, match="empty eval prefix"):
        HipAdamW(_host_engine(), lr=1e-3, groups=[{"params": ("_features.s1.*",), "frozen": True}], frozen_stats="eval")
    with pytest.raises(ValueError, match="unknown key"):
        HipAdamW(_host_engine(), lr=1e-3, groups=[{"params": ("_features.*",), "frozen": True, "frozen_stats": "eval"}])
    # set_groups between steps
    opt.set_groups(C.groups("s2"), frozen_stats="eval")
    stages = forward_stages(eng.spec)
    assert opt.param_groups[0]["frozen_stats"] == "eval" and eng.eval_prefix == tuple(stages[:C.n_eval_stages("s2")])
    assert eng.reloads == 1
    opt.set_groups(C.groups("s2"), frozen_stats="eval")
    assert eng.reloads == 1                                      # the same prefix: nothing rebuilt
    opt.set_groups(C.groups("trunk"), frozen_stats="eval")
    assert eng.reloads == 2 and eng.eval_prefix == tuple(stages)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["frozen_stats"] == "eval"
    opt.set_groups(C.groups("trunk"))
    assert "frozen_stats" not in opt.param_groups[0] and eng.eval_prefix == () and eng.reloads == 3
    # the keyword at construction, and the round trip into an optimizer built without it
    eng2 = _host_engine()
    opt2 = HipAdamW(eng2, lr=1e-3, groups=C.groups("stem"), frozen_stats="eval")
    assert opt2.param_groups[0]["frozen_stats"] == "eval" and eng2.eval_prefix == ("stem",)
    eng3 = _host_engine()
    opt3 = HipAdamW(eng3, lr=1e-3)
    opt3.load_state_dict(sd)
    assert opt3.param_groups[0]["frozen_stats"] == "eval" and eng3.eval_prefix == tuple(stages) and eng3.frozen_stats == "eval"
    assert eng3.frozen == frozen_keys(eng3.params.index, C.groups("trunk"))
    opt3.load_state_dict(opt.state_dict())                       # ... and back to 'batch'
    assert "frozen_stats" not in opt3.param_groups[0] and eng3.eval_prefix == ()


@pytest.mark.parametrize("f32_frames", [False, True])
@pytest.mark.parametrize("gi", range(len(C.STEM_GEOMS)))
def test_the_stem_bound_contains_the_fp32_reference_rounded_once(gi, f32_frames):
    """The bound of the GPU test is not vacuous in the other direction: torch's fp32 convolution of the fp32 normalised
    frames, the fold and the ReLU in fp32 and ONE bf16 rounding stay inside it on the operands of every case."""
    c = C.stem_case(gi, f32_frames)
    z = torch.nn.functional.conv2d(c["x32"], c["w"], stride=2, padding=1)
    y = torch.relu(z * c["sc"].view(1, -1, 1, 1) + c["sh"].view(1, -1, 1, 1)).to(torch.bfloat16)
    name = f"stem eval, fp32 reference {C.STEM_GEOMS[gi]} f32={f32_frames}"
    R.assert_within(y.permute(0, 2, 3, 1).contiguous(), c["ref"], name, nhwc=True)
    frac = R.relu_open(c["ref"].ref)
    assert 0.2 < frac < 0.8, frac
    # and it does separate: the same value rounded TWICE (bf16 z, then the fold) leaves it somewhere
    y2 = torch.relu(z.to(torch.bfloat16).float() * c["sc"].view(1, -1, 1, 1) + c["sh"].view(1, -1, 1, 1)).to(torch.bfloat16)
    err = (R.f64(y2.permute(0, 2, 3, 1)) - c["ref"].ref).abs()
    assert int((err > c["ref"].d).sum()) > 0
