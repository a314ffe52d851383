"""engine.block_forms without a GPU: the launch form of every bottleneck against a table read off the plans of the commit
before the function existed (their step names, step bytes and pool takes), the agreement of forms and emitted steps under every
plan switch, and the function's purity.  Plans are built on torch's "meta" device (tools/plan_fingerprint.py)."""
import pytest
import torch

from helpers import plan_tool, model_state

FIELDS = ("one_launch", "c1g", "slice_in", "q_given", "blend_in", "qtail", "sc_in_conv3")
SWITCHES = ("BNECK_ONE_LAUNCH", "C1_GCONV", "SC_IN_CONV3", "BNECK_BLEND", "BNECK_QTAIL")


def _rows(text):
    """{block: (Fp, slice_next, set of true fields)} of a table `block Fp slice_next field ...`"""
    rows = {}
    for line in text.strip().splitlines():
        name, Fp, slice_next, *on = line.split()
        assert set(on) <= set(FIELDS), line
        rows[name] = (int(Fp), int(slice_next), set(on))
    return rows


# B = 2, T = 16, n_split = 1, fuse_front = True.  Columns: block, Fp (0: no gate-shift site), slice_next, the true booleans.
# bf16: s1.b1 runs in the front launch and is no block of the run.
TABLE = {
    ("rny002_gsf", 224, torch.bfloat16): _rows("""
        s2.b1  0 16 c1g sc_in_conv3
        s3.b1 16 40 c1g sc_in_conv3 slice_in
        s3.b2 40 40 one_launch blend_in qtail slice_in
        s3.b3 40 40 one_launch blend_in qtail slice_in q_given
        s3.b4 40 40 one_launch blend_in qtail slice_in q_given
        s4.b1 40 96 c1g slice_in q_given
        s4.b2 96 96 one_launch blend_in qtail slice_in
        s4.b3 96 96 one_launch blend_in qtail slice_in q_given
        s4.b4 96 96 one_launch blend_in qtail slice_in q_given
        s4.b5 96 96 one_launch blend_in qtail slice_in q_given
        s4.b6 96 96 one_launch blend_in qtail slice_in q_given
        s4.b7 96  0 one_launch blend_in slice_in q_given"""),
    # 6 x 6 maps: one launch with the blend, but no tail; 3 x 3 maps: the four-launch chain
    ("rny002_gsf", 96, torch.bfloat16): _rows("""
        s2.b1  0 16 c1g sc_in_conv3
        s3.b1 16 40 c1g sc_in_conv3 slice_in
        s3.b2 40 40 one_launch blend_in slice_in
        s3.b3 40 40 one_launch blend_in slice_in
        s3.b4 40 40 one_launch blend_in slice_in
        s4.b1 40 96 c1g slice_in
        s4.b2 96 96 slice_in
        s4.b3 96 96 slice_in
        s4.b4 96 96 slice_in
        s4.b5 96 96 slice_in
        s4.b6 96 96 slice_in
        s4.b7 96  0 slice_in"""),
    ("rny008_gsf", 224, torch.bfloat16): _rows("""
        s2.b1  0  0 c1g
        s2.b2  0  0 c1g
        s2.b3  0 32 c1g
        s3.b1 32 80 c1g slice_in
        s3.b2 80 80 slice_in
        s3.b3 80 80 slice_in
        s3.b4 80 80 slice_in
        s3.b5 80 80 slice_in
        s3.b6 80 80 slice_in
        s3.b7 80 80 slice_in
        s3.b8 80 80 slice_in
        s4.b1 80 192 slice_in
        s4.b2 192 0 slice_in"""),
    # fp32: no front launch (s1.b1 is the first block of the run), every launch form is the plain chain; the compact slice
    # in front of each site is taken all the same
    ("rny002_gsf", 224, torch.float32): _rows("""
        s1.b1  0  0
        s2.b1  0 16
        s3.b1 16 40 slice_in
        s3.b2 40 40 slice_in
        s3.b3 40 40 slice_in
        s3.b4 40 40 slice_in
        s4.b1 40 96 slice_in
        s4.b2 96 96 slice_in
        s4.b3 96 96 slice_in
        s4.b4 96 96 slice_in
        s4.b5 96 96 slice_in
        s4.b6 96 96 slice_in
        s4.b7 96  0 slice_in"""),
    ("rny008_gsf", 224, torch.float32): _rows("""
        s1.b1  0  0
        s2.b1  0  0
        s2.b2  0  0
        s2.b3  0 32
        s3.b1 32 80 slice_in
        s3.b2 80 80 slice_in
        s3.b3 80 80 slice_in
        s3.b4 80 80 slice_in
        s3.b5 80 80 slice_in
        s3.b6 80 80 slice_in
        s3.b7 80 80 slice_in
        s3.b8 80 80 slice_in
        s4.b1 80 192 slice_in
        s4.b2 192 0 slice_in"""),
}
TABLE["rny002_gsf", 96, torch.float32] = TABLE["rny002_gsf", 224, torch.float32]
PLANS = sorted(TABLE, key=str)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd import _lib
    return _lib.load()


_PACKED = {}          # (arch, dtype) -> PackedWeights on "meta", packed once (block_forms reads them, nothing writes what it reads)


def _plan(monkeypatch, arch, S, dt):
    """the plan of B = 2 clips of S x S, and the (blocks, forms) of the runs of bottlenecks that _blocks asked block_forms for"""
    from tdeed_amd import engine as E
    tool = plan_tool()
    tool.patch_meta(E, monkeypatch.setattr)
    runs, real = [], E.block_forms

    def recorded(blocks, *a):
        runs.append((blocks, real(blocks, *a)))
        return runs[-1][1]
    monkeypatch.setattr(E, "block_forms", recorded)
    cfg = tool.config(arch, 2, 16)
    if (arch, dt) not in _PACKED:
        _PACKED[arch, dt] = E.PackedWeights(cfg, model_state(cfg, 3), dt, "meta")
    plan = tool.meta_engine(E, cfg, _PACKED[arch, dt]).plan(2, S, S)
    return plan, runs


@pytest.mark.parametrize("arch,S,dt", PLANS, ids=lambda v: str(v).replace("torch.", ""))
def test_forms_are_the_parents(lib, monkeypatch, arch, S, dt):
    _, runs = _plan(monkeypatch, arch, S, dt)
    assert len(runs) == 1
    blocks, forms = runs[0]
    want = TABLE[arch, S, dt]
    assert [bw.spec.name for bw in blocks] == list(want)
    h = S // 2 if "s1.b1" in want else S // 4
    for bw, f in zip(blocks, forms):
        Fp, slice_next, on = want[bw.spec.name]
        got = (f.Fp, f.slice_next, f.site, {k for k in FIELDS if getattr(f, k)})
        assert got == (Fp, slice_next, Fp > 0, on), (bw.spec.name, f)
        assert all(isinstance(getattr(f, k), bool) for k in FIELDS + ("site",)), f
        assert (f.h, f.w) == (h, h) and (f.h2, f.w2) == ((h - 1) // bw.spec.stride + 1,) * 2, (bw.spec.name, f)
        h = f.h2


@pytest.mark.parametrize("off", (None,) + SWITCHES)
@pytest.mark.parametrize("arch,S,dt", PLANS, ids=lambda v: str(v).replace("torch.", ""))
def test_forms_and_plan_agree(lib, monkeypatch, arch, S, dt, off):
    from tdeed_amd import engine as E
    if off is not None:
        monkeypatch.setattr(E, off, False)
    plan, runs = _plan(monkeypatch, arch, S, dt)
    (blocks, forms), = runs
    names = {s.name for s in plan.steps}
    prev = None
    for bw, f in zip(blocks, forms):
        blk = bw.spec
        has = lambda step: blk.name + "." + step in names                                     # noqa: E731
        assert has("bneck") == f.one_launch, (blk.name, f)
        assert has("conv1_conv2") == f.c1g, (blk.name, f)
        assert (has("conv1") and has("conv2")) == (not f.one_launch and not f.c1g), (blk.name, f)
        assert has("conv1") == has("conv2"), blk.name
        assert has("gate_shift") == f.site, (blk.name, f)
        if blk.has_downsample:
            assert has("downsample") == (not f.sc_in_conv3), (blk.name, f)
        else:
            assert not has("downsample") and not f.sc_in_conv3, (blk.name, f)
        assert f.q_given == (prev is not None and prev.qtail), (blk.name, f)
        assert f.slice_in == (prev is not None and prev.slice_next == f.Fp > 0), (blk.name, f)
        assert f.one_launch or not f.blend_in, (blk.name, f)
        assert f.blend_in or not f.qtail, (blk.name, f)
        prev = f
    if off is not None:
        field = dict(BNECK_ONE_LAUNCH="one_launch", C1_GCONV="c1g", SC_IN_CONV3="sc_in_conv3", BNECK_BLEND="blend_in",
                     BNECK_QTAIL="qtail")[off]
        assert not any(getattr(f, field) for f in forms)


def test_block_forms_is_pure(lib, monkeypatch):
    from tdeed_amd import engine as E
    tool = plan_tool()
    tool.patch_meta(E, monkeypatch.setattr)
    cfg = tool.config("rny002_gsf", 2, 16)
    blocks = E.PackedWeights(cfg, model_state(cfg, 3), torch.bfloat16, "meta").W.blocks[1:]
    assert all(bw.c1g_w1f is None for bw in blocks)
    before = [sorted(vars(bw)) for bw in blocks]

    def no_take(*a):
        raise AssertionError("block_forms took a pool buffer")
    monkeypatch.setattr(E._Pool, "take", no_take)
    first = E.block_forms(blocks, 56, 56, torch.bfloat16, set(), False)
    assert first == E.block_forms(blocks, 56, 56, torch.bfloat16, set(), False)
    assert any(f.c1g for f in first) and any(f.qtail for f in first)
    assert all(bw.c1g_w1f is None for bw in blocks)
    assert [sorted(vars(bw)) for bw in blocks] == before
    # the last block writes into a slice of a shared buffer: its output is not contiguous, so it is not one launch
    assert first[-1].one_launch
    assert not E.block_forms(blocks, 56, 56, torch.bfloat16, set(), True)[-1].one_launch
    # a gs_out tap needs the blended slice in memory
    tapped = E.block_forms(blocks, 56, 56, torch.bfloat16, {"_features.s3.b3.gs_out"}, False)
    assert [f.blend_in for f in tapped] == [f.blend_in and bw.spec.name != "s3.b3" for bw, f in zip(blocks, first)]
