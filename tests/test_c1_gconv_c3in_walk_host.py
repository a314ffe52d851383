"""The band walk of the conv3-in c1_gconv launch without a GPU: the override's argument checking, the routed run length and
the grid per shape (never a function of N), the kernels' registers, and cfg2's plan, which no walk setting changes."""
import functools
import os
import re

import pytest
import torch

from test_isa_guards import HIPCC, _resource_usage
from test_s1_conv3_in_c1g_plan import _plan, _cost

# (Hi, Wi, Cp, C) -> bands per frame
SHAPES = {(19, 56, 24, 56): 5, (18, 56, 24, 56): 5, (10, 56, 24, 56): 3, (15, 13, 24, 56): 1, (12, 20, 32, 64): 1,
          (8, 6, 8, 32): 1, (56, 56, 24, 56): 14}


@functools.lru_cache(maxsize=None)
def _conv_usage():
    return _resource_usage("conv.hip")                      # (one compile for the tests that read it)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def routed_walk_again(lib):
    yield
    assert lib.tdeed_c1_gconv_c3in_set_walk(0) == 0


def test_set_walk_checks_its_argument(lib):
    from tdeed_amd import ops, _lib
    for bad in (-1, -14, 1 << 20):
        with pytest.raises(_lib.HipCallError, match="c1_gconv_c3in_set_walk"):
            ops.c1_gconv_c3in_set_walk(bad)
    # a refused value leaves the setting alone
    ops.c1_gconv_c3in_set_walk(7)
    with pytest.raises(_lib.HipCallError):
        ops.c1_gconv_c3in_set_walk(-1)
    assert ops.c1_gconv_c3in_workgroups(1, 56, 56, 24, 56) == 2
    for ok in (0, 1, 2, 14, 1000):
        ops.c1_gconv_c3in_set_walk(ok)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_run_length_and_grid(lib, shape):
    from tdeed_amd import ops
    bands = SHAPES[shape]
    assert ops.c1_gconv_c3in_fits(*shape) and ops.gconv3x3_parts(shape[0], shape[1], shape[3], 2, torch.bfloat16) == bands
    routed = ops.c1_gconv_c3in_walk(*shape)
    assert 1 <= routed <= bands
    for N in (1, 3, 800):
        ops.c1_gconv_c3in_set_walk(0)
        assert ops.c1_gconv_c3in_walk(*shape) == routed                      # never a function of N or of the override
        assert ops.c1_gconv_c3in_workgroups(N, *shape) == N * -(-bands // routed)
        ops.c1_gconv_c3in_set_walk(1)
        assert ops.c1_gconv_c3in_workgroups(N, *shape) == N * bands
        for walk in (2, 3, 4, 5, 7, 14, 100):
            ops.c1_gconv_c3in_set_walk(walk)
            assert ops.c1_gconv_c3in_workgroups(N, *shape) == N * -(-bands // min(walk, bands)), (N, walk)
            assert ops.c1_gconv_c3in_walk(*shape) == routed
    ops.c1_gconv_c3in_set_walk(0)
    assert ops.c1_gconv_c3in_workgroups(0, *shape) == 0


def test_the_sweep_grids_at_the_timed_shape(lib):
    from tdeed_amd import ops
    for walk, grid in ((1, 11200), (2, 5600), (3, 4000), (4, 3200), (5, 2400), (7, 1600), (14, 800)):
        ops.c1_gconv_c3in_set_walk(walk)
        assert ops.c1_gconv_c3in_workgroups(800, 56, 56, 24, 56) == grid


def test_shapes_the_form_does_not_serve(lib):
    from tdeed_amd import ops
    for shape in ((56, 56, 64, 128), (56, 56, 24, 152), (56, 56, 12, 56)):
        assert not ops.c1_gconv_c3in_fits(*shape)
        assert ops.c1_gconv_c3in_walk(*shape) == 0 and ops.c1_gconv_c3in_workgroups(8, *shape) == 0


def test_a_frame_of_two_gib_is_not_served(lib):
    """the kernel addresses a frame with 32-bit byte offsets: from 2^31 bytes per frame on the form does not fit (the engine
    then runs the chain), at every run length setting.  Host calls only: nothing is allocated."""
    from tdeed_amd import ops
    shape = (600000, 56, 32, 64)
    assert shape[0] * shape[1] * shape[2] * 2 >= 2 ** 31
    for walk in (0, 1, 5):
        ops.c1_gconv_c3in_set_walk(walk)
        assert not ops.c1_gconv_c3in_fits(*shape)
        assert ops.c1_gconv_c3in_walk(*shape) == 0
        assert ops.c1_gconv_c3in_workgroups(1, *shape) == 0 and ops.c1_gconv_c3in_workgroups(800, *shape) == 0
    # the last row count below the limit is served
    below = ((2 ** 31 - 1) // (56 * 32 * 2), 56, 32, 64)
    assert below[0] * below[1] * below[2] * 2 < 2 ** 31 and ops.c1_gconv_c3in_fits(*below)
    assert ops.c1_gconv_c3in_walk(*below) == 5


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_walk_kernel_keeps_three_workgroups_per_cu_without_scratch():
    use = _conv_usage()
    inst = {int(m.group(1)): u for k, u in use.items() for m in [re.search(r"c1_gconv_c3in_walk_kernelILi(\d+)E", k)] if m}
    assert sorted(inst) == [16, 32, 64], sorted(use)
    assert not any("c1_gconv_mfma_kernel" in k for k in use if "c3in_walk" in k)
    for csp, u in inst.items():
        # 12 waves per CU (three workgroups of four, 42 KB band + 8 KB static LDS each): at most 168 registers, nothing in scratch
        assert u["scratch"] == 0 and u["vgpr"] <= 168, (csp, u)


# VGPRs and scratch bytes per lane of the c1_gconv kernels at the commit before the conv3-in kernels became one (the same helper
# on that commit's conv.hip): (kernel, template arguments) -> (VGPRs, scratch).  No kernel may need more.
BEFORE = {("c1_gconv_mfma_kernel", (1, 1)): (127, 0), ("c1_gconv_mfma_kernel", (1, 2)): (157, 0),
          ("c1_gconv_mfma_kernel", (1, 4)): (168, 0), ("c1_gconv_mfma_kernel", (1, 5)): (147, 0),
          ("c1_gconv_mfma_kernel", (2, 1)): (127, 0), ("c1_gconv_mfma_kernel", (2, 2)): (157, 0),
          ("c1_gconv_mfma_kernel", (2, 4)): (168, 0), ("c1_gconv_mfma_kernel", (2, 5)): (147, 0),
          ("c1_gconv_slab_loop_kernel", (2, 2)): (168, 0), ("c1_gconv_slab_loop_kernel", (2, 5)): (242, 0),
          ("c1_gconv_c3in_walk_kernel", (16,)): (130, 0), ("c1_gconv_c3in_walk_kernel", (32,)): (160, 0),
          ("c1_gconv_c3in_walk_kernel", (64,)): (167, 0)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_one_conv3_in_kernel_and_no_c1_gconv_kernel_needs_more_registers():
    use = _conv_usage()
    inst = {}
    for k, u in use.items():
        m = re.match(r"_Z\d+(c1_gconv_\w+?_kernel)I((?:L[ib]\d+E)+)Ev", k)
        if m:
            inst[(m.group(1), tuple(int(a) for a in re.findall(r"L[ib](\d+)E", m.group(2))))] = u
    mfma = sorted(a for n, a in inst if n == "c1_gconv_mfma_kernel")
    assert mfma == [(s, k) for s in (1, 2) for k in (1, 2, 4, 5)], mfma     # eight, none with a third template argument
    assert sorted(inst) == sorted(BEFORE), sorted(inst)
    for key, (vgpr, scratch) in BEFORE.items():
        assert inst[key]["vgpr"] <= vgpr and inst[key]["scratch"] <= scratch, (key, inst[key])


def test_cfg2_plan_is_the_same_under_every_walk_setting(lib, monkeypatch):
    from tdeed_amd import ops
    costs = {}
    for walk in (0, 1, 2, 14):
        ops.c1_gconv_c3in_set_walk(walk)
        with monkeypatch.context() as m:
            plan, forms = _plan(m, S1_CONV3_IN_C1G=True)
        assert forms[0].conv3_in
        costs[walk] = (_cost(plan), plan.pool_bytes)
    assert costs[1][0] and all(costs[w] == costs[1] for w in costs)
    st = next(c for c in costs[1][0] if c[0] == "s2.b1.conv1_conv2")
    assert st[1] == "c1_gconv"
