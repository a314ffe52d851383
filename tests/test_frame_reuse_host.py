"""Whole-video scoring with the per-frame trunk stages once per frame (reuse_frames=True), the parts that need no GPU: the
row / pad-row arithmetic, the numpy twin of the row gather, where the per-frame part of the trunk ends, and the argument
checks of the wrappers and of the C entry points."""
import numpy as np
import pytest
import torch

from helpers import plan_tool
from tdeed_amd import evalutil as E
from tdeed_amd import ops
from tdeed_amd.regnet_spec import regnet_spec, first_site_block


# ----------------------------------------------------------------------------- rows and the pad row
def test_rows_and_pad_row():
    assert E.frame_map_rows(37, 8, 2) == (48, 37, 16)
    # a video that ends exactly on a chunk boundary still gets a black row: one more chunk
    assert E.frame_map_rows(48, 8, 2) == (64, 48, 16)
    assert E.frame_map_rows(47, 8, 2) == (48, 47, 16)
    assert E.frame_map_rows(1, 100, 2) == (200, 1, 200)
    for L in range(1, 70):
        rows, pad, chunk = E.frame_map_rows(L, 8, 2)
        assert rows % chunk == 0 and L < rows <= L + chunk and pad == L
    with pytest.raises(ValueError):
        E.frame_map_rows(0, 8, 2)


def _maps(rows, shape, seed):
    return np.random.default_rng(seed).integers(1, 200, size=(rows,) + shape).astype(np.float32)


def test_rows_gather_ref_one_video():
    L, T = 37, 8
    rows, pad, _ = E.frame_map_rows(L, T, 2)
    maps = _maps(rows, (2, 3), 0)
    maps[pad] = -7.0                                           # a value no frame row holds
    maps[pad + 1:] = -9.0                                      # black rows too, but not THE pad row
    starts = [-8, -3, 0, 17, 30, 36, 37, 46]
    out = E.rows_gather_ref(maps, starts, L, pad, T)
    assert out.shape == (len(starts), T, 2, 3)
    for b, s in enumerate(starts):
        for t_ in range(T):
            f = s + t_
            assert np.array_equal(out[b, t_], maps[f] if 0 <= f < L else maps[pad]), (b, t_)
    assert np.all(out[0] == -7.0) and np.all(out[6] == -7.0)   # windows of nothing but padding
    assert not (out == -9.0).any()


def test_rows_gather_ref_group_with_a_video_shorter_than_one_clip():
    T, lengths = 8, [37, 5, 20]
    seg_off, clip_off, starts, base, len_v = E.group_clip_table(lengths, T, 6)
    L = int(seg_off[-1])
    rows, pad, chunk = E.frame_map_rows(L, T, 2)
    assert (L, rows, pad) == (62, 64, 62)
    maps = np.arange(rows, dtype=np.float32)[:, None] * np.ones((1, 4), np.float32)     # row p holds p
    maps[pad:] = -1.0
    out = E.rows_gather_ref(maps, starts, L, pad, T, base, len_v)
    v_of = np.searchsorted(clip_off, np.arange(len(starts)), side="right") - 1
    for b in range(len(starts)):
        v = int(v_of[b])
        for t_ in range(T):
            f = int(starts[b]) + t_
            want = float(seg_off[v] + f) if 0 <= f < lengths[v] else -1.0
            assert np.all(out[b, t_] == want), (b, t_)           # never a neighbour's row
    short = out[clip_off[1]:clip_off[2]]
    assert short.shape[0] >= 1 and set(np.unique(short)) <= {-1.0, 37.0, 38.0, 39.0, 40.0, 41.0}
    with pytest.raises(ValueError):
        E.rows_gather_ref(maps, starts, L, pad, T, clip_base=base)


def test_frame_pass_count_is_below_the_clip_route():
    # what last_video_stats reports: rows per view against clips * T of the default route
    for L, T in ((37, 8), (2030, 100)):
        rows, _, _ = E.frame_map_rows(L, T, 2)
        clips = len(E.video_clip_starts(L, T, T // 4 * 3))
        assert rows < clips * T


# ----------------------------------------------------------------------------- where the per-frame part ends
def test_first_site_block_from_the_spec():
    assert first_site_block(regnet_spec("rny002_gsf")) == 2
    assert first_site_block(regnet_spec("rny008_gsf")) == 4
    assert first_site_block(regnet_spec("rny002_gsm")) == 2
    spec = regnet_spec("rny002")
    assert first_site_block(spec) == len(spec.blocks)          # no site at all
    for arch in ("rny002_gsf", "rny008_gsf"):
        spec = regnet_spec(arch)
        k = first_site_block(spec)
        assert all(b.gsf_fold == 0 and b.stage < 3 for b in spec.blocks[:k]) and spec.blocks[k].name == "s3.b1"


def test_frame_and_tail_plans_are_the_two_halves_of_the_join_plan(monkeypatch):
    """On the "meta" device: the frame plan's launches are those of one sub-batch of the join_at = k plan, the tail plan's
    those of its tail -- same names, kernels and costs."""
    from tdeed_amd import engine as Eng, state_layout, synth
    tool = plan_tool()
    tool.patch_meta(Eng, monkeypatch.setattr)
    cfg = tool.config("rny002_gsf", 2, 8)
    sd = synth.make_state(state_layout.model_state_shapes(cfg), 3)
    for dt in (torch.bfloat16, torch.float32):
        pw = Eng.PackedWeights(cfg, sd, dt, "meta")
        eng = tool.meta_engine(Eng, cfg, pw)
        k = eng.first_site_block()
        assert k == 2 and eng.frame_map_shape(64, 64) == (8, 8, 56)
        fp, tp = eng.frame_plan(2, 64, 64), eng.tail_plan(4, 8, 8)
        assert eng.frame_plan(2, 64, 64) is fp and eng.tail_plan(4, 8, 8) is tp and eng.tail_plan(4, 8, 8, slot=1) is not tp
        assert tuple(fp.out.shape) == (16, 8, 8, 56) and tuple(tp.trunk_in.shape) == (32, 8, 8, 56)
        join = tool.meta_engine(Eng, cfg, pw, n_split=2, join_at=k).plan(4, 64, 64)
        sig = lambda steps: [(s.name, s.kernel, s.bytes, s.flops) for s in steps]     # noqa: E731
        assert sig(fp.steps) == sig(join.subs[0].steps)
        assert sig(tp.steps) == sig(join.tail.steps)
        assert fp.steps and not any(".gate_shift" in s.name or s.name.startswith("s3.") for s in fp.steps)
        assert tp.steps[0].name.startswith("s3.b1")


# ----------------------------------------------------------------------------- argument checks
def test_wrappers_reject_bad_arguments():
    maps = torch.zeros((48, 8, 8, 56), dtype=torch.bfloat16)
    out = torch.zeros((16, 8, 8, 56), dtype=torch.bfloat16)
    starts = torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.rows_gather(maps, starts, 37, 37, 8, out.float())                  # out of another dtype
    with pytest.raises(TypeError):
        ops.rows_gather(maps, starts.long(), 37, 37, 8, out)                   # int64 starts
    with pytest.raises(TypeError):
        ops.rows_gather_seg(maps, starts.long(), starts, starts, 37, 37, 8, out)
    with pytest.raises(ValueError, match="contiguous"):
        ops.rows_gather(maps[:, :, :, ::2], starts, 37, 37, 8, out[:, :, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        ops.rows_gather_seg(maps, starts, starts, starts, 37, 37, 8, out.transpose(1, 2))
    with pytest.raises(ValueError, match="go together"):
        ops.rows_gather_seg(maps, starts, starts, None, 37, 37, 8, out)
    with pytest.raises(ValueError, match="go together"):
        ops.rows_gather_seg(maps, starts, None, starts, 37, 37, 8, out)


def test_entry_points_check_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from tdeed_amd._lib import call, HipCallError
    P = 1 << 20
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_rows_gather", None, 48, 7168, 37, 37, P, 1, 8, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_rows_gather_seg", P, 48, 7168, 37, 37, P, P, None, 1, 8, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_rows_gather", P, 48, 0, 37, 37, P, 1, 8, P, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_rows_gather", P, 48, 7168, 37, 37, P, 700, 100, P, None)
    with pytest.raises(HipCallError, match="inside the 48 rows"):
        call("tdeed_rows_gather", P, 48, 7168, 37, 48, P, 1, 8, P, None)         # pad_row past the buffer
    with pytest.raises(HipCallError, match="inside the 48 rows"):
        call("tdeed_rows_gather_seg", P, 48, 7168, 49, 37, P, P, P, 1, 8, P, None)   # more frames than rows
    with pytest.raises(HipCallError, match="inside the 48 rows"):
        call("tdeed_rows_gather", P, 48, 7168, 37, -1, P, 1, 8, P, None)


def test_evalutil_passes_the_flag_on_only_when_set():
    seen = []

    class Model:
        def predict_video(self, frames, **kw):
            seen.append(kw)
            return np.zeros((int(frames.shape[0]), 4), np.float32), np.zeros(int(frames.shape[0]), np.int32)

        def predict_video_group(self, frames_list, **kw):               # what stitch_videos calls: a video is a group of one
            return [self.predict_video(f, **kw) for f in frames_list]

    videos = [("a", 5, 25.0, torch.zeros((5, 3, 4, 4), dtype=torch.uint8))]
    E.stitch_videos(Model(), videos, 4)
    E.stitch_videos(Model(), videos, 4, reuse_frames=True)
    assert "reuse_frames" not in seen[0] and seen[1]["reuse_frames"] is True
