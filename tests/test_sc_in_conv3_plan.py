"""engine.SC_IN_CONV3 without a GPU: the cfg2 plan (RegNetY-200MF + GSF, B = 8, T = 100, 224 x 224, bf16) built on torch's
"meta" device the way tools/plan_fingerprint.py builds it loses the two `.downsample` launches and their shortcut maps, and
the two-operand instances of gemm_ws_kernel that serve it do not spill."""
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


def _cfg2_plan(monkeypatch, on):
    from tdeed_amd import engine as E
    tool = plan_tool()
    monkeypatch.setattr(E, "SC_IN_CONV3", on)
    tool.patch_meta(E, monkeypatch.setattr)
    cfg = tool.config("rny002_gsf", 2, 100)
    return tool.meta_engine(E, cfg, E.PackedWeights(cfg, model_state(cfg, 3), torch.bfloat16, "meta")).plan(8, 224, 224)


def test_cfg2_plan_drops_two_launches_and_their_maps(lib, monkeypatch):
    with monkeypatch.context() as m:
        off = _cfg2_plan(m, False)
    with monkeypatch.context() as m:
        on = _cfg2_plan(m, True)
    names_off, names_on = [s.name for s in off.steps], [s.name for s in on.steps]
    assert len(names_on) == len(names_off) - 2
    assert {"s2.b1.downsample", "s3.b1.downsample"} <= set(names_off)
    assert not {"s2.b1.downsample", "s3.b1.downsample"} & set(names_on)
    assert set(names_off) - set(names_on) == {"s2.b1.downsample", "s3.b1.downsample"}
    assert on.pool_bytes < off.pool_bytes
    # the fused conv3 is charged y2 + the gathered rows of x + out + both weights, and both products
    N, es = 800, 2
    for name, cin, c, hw in (("s2.b1.conv3", 24, 56, 28 * 28), ("s3.b1.conv3", 56, 152, 14 * 14)):
        st = next(s for s in on.steps if s.name == name)
        M2 = N * hw
        assert st.kernel == "gemm_ws"
        assert st.bytes == (M2 * (2 * c + cin) + c * (c + cin)) * es
        assert st.flops == 2 * M2 * c * (c + cin)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_two_operand_instances_do_not_spill():
    use = _resource_usage("gemm.hip")
    inst = {k: u for k, u in use.items() if re.search(r"gemm_ws_kernelIDF16bLi(2ELb1ELi4ELi1|5ELb1ELi4ELi2)E", k)}
    assert len(inst) == 2, sorted(use)
    for k, u in inst.items():
        assert u["scratch"] == 0, (k, u)
        # two workgroups of four waves per CU (the 5 + 2 k-step form holds 70 KB of weights in LDS): 256 registers would do;
        # 168 keeps the third wave per SIMD that the narrow form's 12 KB allows
        assert u["vgpr"] <= 168, (k, u)
