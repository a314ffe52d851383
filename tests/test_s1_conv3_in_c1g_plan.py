"""engine.S1_CONV3_IN_C1G without a GPU: the cfg2 plan (RegNetY-200MF + GSF, B = 8, T = 100, 224 x 224, bf16) built on
torch's "meta" device loses the `s1.b1.conv3` launch and the map it wrote, every other launch keeps its cost, the form stays
off wherever its conditions do not hold, and the new kernel instance keeps three workgroups per CU without scratch."""
import os
import re

import pytest
import torch

from helpers import plan_tool, model_state
from test_isa_guards import HIPCC, _resource_usage


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd import _lib
    return _lib.load()


_PACKED = {}


def _plan(monkeypatch, arch="rny002_gsf", dt=torch.bfloat16, n_layers=2, T=100, B=8, S=224, taps=(), fuse_front=True, **switches):
    """(plan, forms of the run of bottlenecks behind the front) with the engine switches given"""
    from tdeed_amd import engine as E
    tool = plan_tool()
    for k, v in switches.items():
        monkeypatch.setattr(E, k, v)
    tool.patch_meta(E, monkeypatch.setattr)
    runs, real = [], E.block_forms

    def recorded(blocks, *a):
        runs.append((blocks, real(blocks, *a)))
        return runs[-1][1]
    monkeypatch.setattr(E, "block_forms", recorded)
    cfg = tool.config(arch, n_layers, T)
    if (arch, dt) not in _PACKED:
        _PACKED[arch, dt] = E.PackedWeights(cfg, model_state(cfg, 3), dt, "meta")
    plan = tool.meta_engine(E, cfg, _PACKED[arch, dt], fuse_front=fuse_front).plan(B, S, S, taps=taps)
    (blocks, forms), = runs
    return plan, forms


def _cost(plan):
    return [(s.name, s.kernel, s.bytes, s.flops) for s in plan.steps]


def test_cfg2_plan_loses_the_conv3_launch_and_its_map(lib, monkeypatch):
    with monkeypatch.context() as m:
        off, f_off = _plan(m, S1_CONV3_IN_C1G=False)
    with monkeypatch.context() as m:
        on, f_on = _plan(m, S1_CONV3_IN_C1G=True)
    assert f_on[0].conv3_in is True and not any(f.conv3_in for f in f_on[1:])
    assert not any(f.conv3_in for f in f_off) and all(isinstance(f.conv3_in, bool) for f in f_on + f_off)
    assert f_on[0]._replace(conv3_in=False) == f_off[0] and f_on[1:] == f_off[1:]
    c_off, c_on = _cost(off), _cost(on)
    assert [c for c in c_off if c[0] != "s1.b1.conv3"] != c_off and len(c_on) == len(c_off) - 1
    assert [c[0] for c in c_on] == [c[0] for c in c_off if c[0] != "s1.b1.conv3"]
    # every other launch keeps name, kernel family, bytes and flops
    fused = "s2.b1.conv1_conv2"
    assert [c for c in c_on if c[0] != fused] == [c for c in c_off if c[0] not in (fused, "s1.b1.conv3")]
    assert on.pool_bytes < off.pool_bytes
    # the fused launch: the producer's y2 and shortcut map in, y2 of s2.b1 and the compact map out, the three weights; both
    # contractions and the grouped conv
    N, es, cin, c, gw = 800, 2, 24, 56, 8
    M, M2 = N * 56 * 56, N * 28 * 28
    st = next(s for s in on.steps if s.name == fused)
    assert st.kernel == "c1_gconv"
    assert st.bytes == (2 * M * cin + M2 * c + M2 * cin) * es + (cin * cin + c * (cin + gw * 9)) * es
    assert st.flops == 2 * M * cin * cin + 2 * M * cin * c + 2 * M2 * c * gw * 9
    # the chain's two launches together move and compute more than the one that replaces them
    two = [s for s in off.steps if s.name in (fused, "s1.b1.conv3")]
    assert len(two) == 2 and st.bytes < sum(s.bytes for s in two) and st.flops == sum(s.flops for s in two)


class _OlderLibrary:
    """the loaded library without the entry points of this form (an A/B flavour built from an older revision)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if "c1_gconv_c3in" in name:
            raise AttributeError(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("why", ["fp32", "unfused front", "tap", "C1_GCONV off", "rny008", "older library"])
def test_the_form_stays_off(lib, monkeypatch, why):
    from tdeed_amd import _lib, ops
    assert ops.c1_gconv_c3in_fits(56, 56, 24, 56)
    kw = {"fp32": dict(dt=torch.float32), "unfused front": dict(fuse_front=False), "tap": dict(taps=("_features.s1.b1",)),
          "C1_GCONV off": dict(C1_GCONV=False), "rny008": dict(arch="rny008_gsf", n_layers=3), "older library": {}}[why]
    if why == "older library":
        monkeypatch.setattr(_lib, "_lib", _OlderLibrary(lib))
        assert not ops.c1_gconv_c3in_fits(56, 56, 24, 56)
    plan, forms = _plan(monkeypatch, T=16, B=2, S1_CONV3_IN_C1G=True, **kw)
    assert not any(f.conv3_in for f in forms)
    assert "s1.b1.conv3" in [s.name for s in plan.steps]


def test_the_form_is_on_at_the_small_plan_too(lib, monkeypatch):
    plan, forms = _plan(monkeypatch, T=16, B=2, S1_CONV3_IN_C1G=True)
    assert forms[0].conv3_in and "s1.b1.conv3" not in [s.name for s in plan.steps]


# VGPRs of the c1_gconv_mfma_kernel<STRIDE, KS1> instances at the commit before this form existed (either stride)
PARENT_VGPR = {1: 127, 2: 157, 4: 168, 5: 147}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_c1_gconv_mfma_instances_keep_their_registers():
    """(the conv3-in instance of this kernel is gone: the form's one kernel is the band walk, test_c1_gconv_c3in_walk_host.py)"""
    use = _resource_usage("conv.hip")
    inst = {}
    for k, u in use.items():
        m = re.search(r"c1_gconv_mfma_kernelILi([12])ELi(\d)EEv", k)
        if m:
            inst[int(m.group(1)), int(m.group(2))] = u
    assert sorted(inst) == sorted((s, k) for s in (1, 2) for k in PARENT_VGPR), sorted(use)
    assert len([k for k in use if "c1_gconv_mfma_kernel" in k]) == 8
    for (s, k), u in inst.items():
        assert u["scratch"] == 0 and u["vgpr"] == PARENT_VGPR[k], ((s, k), u)
