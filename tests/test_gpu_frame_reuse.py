"""Whole-video scoring with the per-frame trunk stages once per frame (reuse_frames=True) on the MI355X: the row gather
against torch indexing, the per-frame claim itself (the frame plan's maps against what the join_at = k plan computes inside
overlapping windows, bit for bit), the engine route against forward() of a join_at = k engine, and the four public routes
against their default forms.  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import model_state, t, cfg_ns
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)                          # the configuration of test_gpu_video.py
CLASSES = {"c1": 1, "c2": 2, "c3": 3}
DTYPES = [torch.bfloat16, torch.float32]
L_VIDEO, T_CLIP, K_SITE = 37, 8, 2


def _bits(x):
    return x.contiguous().view(torch.uint8).cpu()


# ----------------------------------------------------------------------------- 1. the gather
def _rows(rows, shape, dtype, pad_row, seed):
    """rows of small integers 1 .. 120 (exact in bf16), the pad row filled with -5 (a value no other row holds)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(1, 121, (rows,) + shape, generator=g).to(dtype)
    m[pad_row] = -5
    return m


def _gather_ref(maps, starts, L, pad_row, T):
    idx = torch.as_tensor(starts, dtype=torch.long)[:, None] + torch.arange(T)[None]
    ok = (idx >= 0) & (idx < L)
    return maps[torch.where(ok, idx, torch.full_like(idx, pad_row))]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape,L,T,starts", [
    ((8, 8, 56), 23, 6, [-6, -3, 0, 9, 17, 22, 23, 32]),            # 7168 / 14336 bytes a row: the 16-byte path
    ((3, 5, 7), 23, 6, [-6, -3, 0, 9, 17, 22, 23, 32]),             # 210 / 420 bytes: the byte path
    ((8, 8, 56), 2, 1, [1]),                                        # B = 1, T = 1
    ((3, 5, 7), 4, 1, [3]),
], ids=["v16", "bytes", "v16_b1t1", "bytes_b1t1"])
def test_rows_gather_equals_torch_indexing(shape, L, T, starts, dtype):
    assert (-T in starts and -3 in starts and L in starts and L + 9 in starts) or T == 1
    assert L - 1 in starts
    rows, pad_row = L + 5, L + 2                                    # not the first row behind the frames: the index is honoured
    maps = _rows(rows, shape, dtype, pad_row, 7 + L)
    md = maps.to(DEV)
    sd = torch.tensor(starts, dtype=torch.int32, device=DEV)
    out = torch.full((len(starts) * T,) + shape, -99, dtype=dtype, device=DEV)        # -99: neither a row value nor the pad's
    ops.rows_gather(md, sd, L, pad_row, T, out)
    torch.cuda.synchronize()
    ref = _gather_ref(maps, starts, L, pad_row, T)
    got = out.cpu().view(len(starts), T, *shape)
    assert torch.equal(_bits(got), _bits(ref))
    assert not bool((got == -99).any())
    if T > 1:
        assert bool((got[0] == -5).all()) and bool((got[-1] == -5).all())           # windows of nothing but padding
        assert bool((got[2] != -5).all())
    assert torch.equal(_bits(md), _bits(maps))                                      # the source is only read


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(8, 8, 56), (3, 5, 7)], ids=["v16", "bytes"])
def test_rows_gather_seg_pads_at_the_videos_own_ends(shape, dtype):
    T, lengths = 6, [9, 3, 7]                                       # the second video is shorter than one clip
    mine = [[-6, -2, 0, 4, 8, 9], [-2, 0, 2], [-1, 3, 6, 7]]
    seg_off, clip_off, starts, base, len_v = E.group_clip_table(lengths, T, 4, clip_starts=mine)
    L = int(seg_off[-1])
    rows, pad_row, _ = E.frame_map_rows(L, T, 2)
    maps = _rows(rows, shape, dtype, pad_row, 3)
    as_int = torch.int16 if dtype == torch.bfloat16 else torch.int32
    ref = E.rows_gather_ref(maps.view(as_int).numpy(), starts, L, pad_row, T, base, len_v)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                 # noqa: E731
    out = torch.full((len(starts) * T,) + shape, -99, dtype=dtype, device=DEV)
    ops.rows_gather_seg(maps.to(DEV), dev(starts), dev(base), dev(len_v), L, pad_row, T, out)
    torch.cuda.synchronize()
    got = out.cpu().view(as_int).numpy().reshape(ref.shape)
    assert np.array_equal(got, ref)
    # a window over the end of video 0 holds the pad row, not the first rows of video 1
    last0 = out.cpu().view(len(starts), T, *shape)[4]               # start 8 of the 9-frame video
    assert bool((last0[0] != -5).all()) and bool((last0[1:] == -5).all())
    with pytest.raises(ValueError):
        ops.rows_gather_seg(maps.to(DEV), dev(starts), dev(base)[:3], dev(len_v), L, pad_row, T, out)
    with pytest.raises(ValueError):
        ops.rows_gather_seg(maps.to(DEV), dev(starts), dev(base), dev(len_v), L, pad_row, T, out[:5])


def test_rows_gather_checks_its_arguments():
    from tdeed_amd._lib import HipCallError
    maps = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    sd = torch.zeros((700,), dtype=torch.int32, device=DEV)
    with pytest.raises(HipCallError, match="65535"):
        ops.rows_gather(maps, sd, 3, 3, 100, torch.empty((700 * 100, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.rows_gather(maps, sd[:2], 3, 4, 4, torch.empty((8, 8), dtype=torch.float32, device=DEV))     # pad_row = rows
    with pytest.raises(ValueError):
        ops.rows_gather(maps, sd[:2], 5, 3, 4, torch.empty((8, 8), dtype=torch.float32, device=DEV))     # L > rows
    with pytest.raises(ValueError):
        ops.rows_gather(maps, sd[:2], 3, 3, 4, torch.empty((7, 8), dtype=torch.float32, device=DEV))


# ----------------------------------------------------------------------------- 2. / 3. the engine
@pytest.fixture(scope="module")
def tiny_video():
    return t(synth.uint8_clip(4100, (L_VIDEO, 3, 64, 64)))


def _windows(video, starts, T):
    L = video.shape[0]
    idx = torch.as_tensor(starts, dtype=torch.long)[:, None] + torch.arange(T)[None]
    ok = (idx >= 0) & (idx < L)
    out = video[idx.clamp(0, L - 1)]
    out[~ok] = 0
    return out


@pytest.fixture(scope="module", params=DTYPES, ids=["bf16", "fp32"])
def engines(request, tiny_video):
    """(reuse engine, join_at = k engine, stream, the resident video, per view the maps of all its frames in video order)"""
    from tdeed_amd.engine import ForwardEngine
    dt = request.param
    sd = model_state(TINY, 0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        eng = ForwardEngine(TINY, sd, dt, DEV)
        join = ForwardEngine(TINY, sd, dt, DEV, n_split=2)
        k = eng.first_site_block()
        assert k == K_SITE and join.merge_tail
        join.join_at = k
        video = tiny_video.to(DEV)
        rows, pad_row, chunk = E.frame_map_rows(L_VIDEO, T_CLIP, 2)
        assert (rows, pad_row, chunk) == (48, 37, 16)
        maps = torch.empty((2, rows) + eng.frame_map_shape(64, 64), dtype=dt, device=DEV)
        for v in range(2):
            for c in range(rows // chunk):
                eng.frame_maps(video, c * chunk, maps[v, c * chunk:(c + 1) * chunk], 2, flip=bool(v))
        st.synchronize()
    return eng, join, st, video, maps


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_the_trunk_in_front_of_the_first_site_is_per_frame(engines, tiny_video, flip):
    """Row f of the frame plan's map (frames in video order, two clips' worth a launch) carries the bits that the join_at = k
    plan computes for frame f inside every window that holds it -- whatever its position in the window and the batch --
    and the black rows those of the windows' padding."""
    eng, join, st, video, maps = engines
    m = maps[int(flip)].cpu()
    assert tuple(m.shape) == (48, 8, 8, 56)
    black = _bits(m[37])
    for r in range(38, 48):
        assert torch.equal(_bits(m[r]), black), r                   # every row behind the video is the same black map
    assert float(m[37].float().abs().sum()) > 0                     # ... and it is not zero
    seen = set()
    for starts in ([-8, -3, 0, 2], [6, 10, 14, 17], [21, 25, 30, 36]):
        with torch.cuda.stream(st):
            _, plan = join.forward(_windows(tiny_video, starts, T_CLIP).to(DEV), augment_inference=flip)
            st.synchronize()
        assert plan.trunk_map is not None and len(plan.subs) == 2
        tm = plan.trunk_map.cpu().view(4, T_CLIP, 8, 8, 56)
        for b, s in enumerate(starts):
            for i in range(T_CLIP):
                f = s + i
                row = f if 0 <= f < L_VIDEO else 37
                assert torch.equal(_bits(tm[b, i]), _bits(m[row])), (starts, b, i)
                seen.add(row)
    assert seen == set(range(38))                                   # every frame, most of them at several window positions
    assert not torch.equal(_bits(maps[0][:37]), _bits(maps[1][:37]))    # the flip view is another map


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_forward_from_frame_maps_equals_the_join_plan_on_the_windows(engines, tiny_video, flip):
    eng, join, st, video, maps = engines
    starts = [-8, -3, 0, 17, 30, 36]
    with torch.cuda.stream(st):
        sd = torch.tensor(starts, dtype=torch.int32, device=DEV)
        head, plan = eng.forward_from_frame_maps(maps[int(flip)], sd, 37, slot=0)
        got = head.clone()
        again, plan2 = eng.forward_from_frame_maps(maps[int(flip)], sd, 37, slot=0)      # the replay of the captured graph
        got2 = again.clone()
        ref, _ = join.forward(_windows(tiny_video, starts, T_CLIP).to(DEV), augment_inference=flip)
        ref = ref.clone()
        st.synchronize()
    assert plan2 is plan and plan.graph is not None
    assert tuple(got.shape) == (6 * T_CLIP, eng.pw.n_out) and float(got.abs().sum()) > 0
    assert torch.equal(got, ref), float((got - ref).abs().max())
    assert torch.equal(got2, ref)
    with pytest.raises(ValueError, match="go together"):
        eng.forward_from_frame_maps(maps[0], sd, 37, clip_base=sd)
    with pytest.raises(TypeError):
        eng.forward_from_frame_maps(maps[0].to(torch.float64), sd, 37)


# ----------------------------------------------------------------------------- 4. the model
def _model(cfg, join):
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m.load({k: t(v) for k, v in model_state(cfg, 0).items()})
    if join:
        for dt in DTYPES:                                           # before any plan is built
            eng = m._model.engine(dt)
            assert not eng._plans
            eng.join_at = eng.first_site_block()
    return m


@pytest.fixture(scope="module")
def join_model():
    """a model whose default route runs the join_at = k plan: the launch forms of the reuse route"""
    return _model(TINY, True)


@pytest.fixture(scope="module")
def plain_model():
    return _model(TINY, False)


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
def test_predict_video_reuse_is_bit_identical_to_the_join_route(join_model, tiny_video, use_amp, augment):
    m = join_model
    m.video_chunk_bytes = 7 * 3 * 64 * 64                           # several upload chunks
    kw = dict(batch_size=4, augment=augment, use_amp=use_amp)       # 18 clips: the last batch has 2
    ref_sums, ref_sup = m.predict_video(tiny_video, **kw)
    ref_stats = dict(m.last_video_stats)
    sums, sup = m.predict_video(tiny_video, reuse_frames=True, **kw)
    stats = dict(m.last_video_stats)
    assert np.array_equal(sup, ref_sup)
    assert np.array_equal(sums, ref_sums), float(np.abs(sums - ref_sums).max())
    assert float(sums.sum()) > 0 and int(sup.max()) >= 1
    V = 2 if augment else 1
    base = dict(frames=37, clips=18, batches=5, views=V, frames_h2d_bytes=37 * 3 * 64 * 64)
    assert ref_stats == base                                        # the default route: today's keys, nothing else
    assert stats == dict(base, frame_pass_frames=V * 48, map_bytes=V * 48 * 8 * 8 * 56 * (2 if use_amp else 4))
    assert stats["frame_pass_frames"] // V < stats["clips"] * 8     # 48 rows against 144 frames through the front
    # resident and pinned sources, and a second call on warm plans
    for src in (tiny_video.to(DEV), tiny_video.pin_memory()):
        s2, n2 = m.predict_video(src, reuse_frames=True, **kw)
        assert np.array_equal(s2, ref_sums) and np.array_equal(n2, ref_sup)


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
def test_spot_video_reuse_is_bit_identical_to_the_join_route(join_model, tiny_video, use_amp, augment):
    m = join_model
    kw = dict(batch_size=4, augment=augment, use_amp=use_amp)
    ref = m.spot_video(tiny_video, CLASSES, **kw)
    got = m.spot_video(tiny_video, CLASSES, reuse_frames=True, **kw)
    assert np.array_equal(got["pred"], ref["pred"])
    assert got["events"] == ref["events"]
    assert got["suppressed"] == ref["suppressed"] and len(got["suppressed"]) == 2
    print(f"events {len(ref['events'])}, suppressed {[len(x) for x in ref['suppressed']]}")
    assert m.last_video_stats["frame_pass_frames"] == (2 if augment else 1) * 48


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
def test_predict_video_group_reuse_is_bit_identical_to_the_join_route(join_model, use_amp, augment):
    m = join_model
    m.video_chunk_bytes = 9 * 3 * 64 * 64
    videos = [t(synth.uint8_clip(4200 + i, (n, 3, 64, 64))) for i, n in enumerate((37, 5, 20))]
    kw = dict(batch_size=4, augment=augment, use_amp=use_amp)
    ref = m.predict_video_group(videos, **kw)
    ref_stats = dict(m.last_video_stats)
    got = m.predict_video_group(videos, reuse_frames=True, **kw)
    stats = dict(m.last_video_stats)
    worst = max(float(np.abs(a[0] - b[0]).max()) for a, b in zip(got, ref))
    print(f"group, reuse against the join route: largest difference {worst}")
    for (s, n), (rs, rn) in zip(got, ref):
        assert np.array_equal(n, rn)
        assert np.array_equal(s, rs), worst
    V = 2 if augment else 1
    assert set(ref_stats) == {"frames", "clips", "batches", "views", "frames_h2d_bytes", "videos", "host_syncs"}
    assert stats == dict(ref_stats, frame_pass_frames=V * 64, map_bytes=V * 64 * 8 * 8 * 56 * (2 if use_amp else 4))
    sg = m.spot_video_group(videos, CLASSES, reuse_frames=True, **kw)
    sr = m.spot_video_group(videos, CLASSES, **kw)
    for a, b in zip(sg, sr):
        assert np.array_equal(a["pred"], b["pred"]) and a["events"] == b["events"] and a["suppressed"] == b["suppressed"]


@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
def test_odd_batches_stay_within_the_measured_launch_form_difference(join_model, plain_model, tiny_video, use_amp):
    """batch_size 5 and 1: the split plan does not exist, the default route runs the whole network as one plan, whose first
    site reads the compact slice that s2.b1 wrote beside its output; the reuse route runs the site on the gathered map.  The
    bound is measured here on existing code: the largest difference between the join_at = k route and the default route at
    batch_size 4 differs by the same launch form; twice that is allowed."""
    kw = dict(augment=True, use_amp=use_amp)
    d_sums, _ = plain_model.predict_video(tiny_video, batch_size=4, **kw)
    j_sums, _ = join_model.predict_video(tiny_video, batch_size=4, **kw)
    measured = float(np.abs(d_sums - j_sums).max())
    print(f"join_at = k against the default route at batch_size 4: largest difference {measured}")
    for bs in (5, 1):
        ref, ref_sup = plain_model.predict_video(tiny_video, batch_size=bs, **kw)
        got, sup = plain_model.predict_video(tiny_video, batch_size=bs, reuse_frames=True, **kw)
        diff = float(np.abs(got - ref).max())
        print(f"batch_size {bs}: reuse against the default route: largest difference {diff}")
        assert np.array_equal(sup, ref_sup)
        assert diff <= 2 * measured, f"batch_size {bs}: {diff} against the measured {measured} (allowed: twice that)"


def test_reuse_counts_the_maps_towards_max_resident_bytes(plain_model, tiny_video, monkeypatch):
    m = plain_model
    map_bytes = 48 * 8 * 8 * 56 * 2
    budget = tiny_video.numel() + map_bytes - 1
    m.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget)          # the frames alone fit
    launched = []
    for gather in ("clip_gather", "clip_gather_seg", "rows_gather", "rows_gather_seg"):       # every gather the model may call
        monkeypatch.setattr(ops, gather, lambda *a, **k: launched.append(1))
    with pytest.raises(ValueError, match="max_resident_bytes"):
        m.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget, reuse_frames=True)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        m.predict_video_group([tiny_video], batch_size=4, max_resident_bytes=budget, reuse_frames=True)
    assert not launched
    monkeypatch.undo()
    m.predict_video(tiny_video, batch_size=4, max_resident_bytes=budget + 1, reuse_frames=True)
    assert m.last_video_stats["map_bytes"] == map_bytes
