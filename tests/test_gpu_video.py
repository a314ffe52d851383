"""Whole-video scoring on the MI355X: the clip gather and the score stitch kernels against torch / ScoreStitcher, and
`TDEEDModel.predict_video` bit for bit against the clip-batch route (`predict` + `ScoreStitcher`).  -m gpu only."""
import numpy as np
import pytest
import torch

from helpers import model_state, t, cfg_ns
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth
from test_video_host import stitch_inputs, STITCH_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------- 5. gather
def _gather_ref(video, starts, T):
    L = video.shape[0]
    idx = torch.as_tensor(starts, dtype=torch.long)[:, None] + torch.arange(T)[None]
    ok = (idx >= 0) & (idx < L)
    out = video[idx.clamp(0, L - 1)]
    out[~ok] = 0
    return out


@pytest.mark.parametrize("shape,L,T,starts", [
    ((3, 224, 224), 40, 8, [-8, -3, 0, 17, 32, 39, 40, 5]),          # 150 528 bytes: the 16-byte path
    ((3, 5, 7), 23, 6, [-6, -2, 0, 9, 18, 22, 30]),                  # 105 bytes: the byte path
    ((3, 224, 224), 2, 1, [1]),                                      # B = 1, T = 1
    ((3, 5, 7), 4, 1, [3]),
    ((3, 224, 224), 260, 100, [-100, -5, 20, 45, 120, 161, 259, 200]),   # B = 8, T = 100 at 224 x 224
], ids=["v16", "bytes", "v16_b1t1", "bytes_b1t1", "b8_t100_224"])
def test_clip_gather_equals_torch_indexing(shape, L, T, starts):
    video = ops.fill_u8_hash((L,) + shape, 31 + L, DEV)
    assert -T in starts or T == 1
    assert L - 1 in starts
    sd = torch.tensor(starts, dtype=torch.int32, device=DEV)
    out = torch.full((len(starts) * T,) + shape, 9, dtype=torch.uint8, device=DEV)
    ops.clip_gather(video, sd, T, out)
    torch.cuda.synchronize()
    ref = _gather_ref(video.cpu(), starts, T)
    got = out.cpu().view(len(starts), T, *shape)
    assert torch.equal(got, ref)
    assert int(ref[0].sum()) == 0 or T == 1                          # a clip of nothing but padding
    assert int(video.sum()) > 0


def test_clip_gather_checks_its_arguments():
    from tdeed_amd._lib import HipCallError
    video = torch.zeros((4, 3, 4, 4), dtype=torch.uint8, device=DEV)
    sd = torch.zeros((700,), dtype=torch.int32, device=DEV)
    with pytest.raises(HipCallError, match="65535"):
        ops.clip_gather(video, sd, 100, torch.empty((700 * 100, 3, 4, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.clip_gather(video, sd[:2], 4, torch.empty((7, 3, 4, 4), dtype=torch.uint8, device=DEV))


# ----------------------------------------------------------------------------- 6. stitch
@pytest.mark.parametrize("case", STITCH_CASES)
@pytest.mark.parametrize("V", [1, 2])
def test_stitch_scores_equals_the_score_stitcher(case, V):
    L = case["L"]
    starts, plain, flip = stitch_inputs(L, starts=case.get("starts"), seed=case["seed"])
    st = E.ScoreStitcher([("v", L, 25.0)], 4)
    for i, s in enumerate(starts):
        if V == 1:
            st.add("v", s, plain[i])
        else:
            st.add_views("v", s, plain[i][None])
            st.add_views("v", s, flip[i][None])
    sc = torch.from_numpy(np.stack([plain, flip][:V])).to(DEV)
    sd = torch.tensor(starts, dtype=torch.int32, device=DEV)
    sums, sup, mean = ops.stitch_scores(sc, sd, L, mean=True)
    torch.cuda.synchronize()
    assert torch.equal(sums.cpu(), t(st.tracks["v"][0]))
    assert torch.equal(sup.cpu(), t(st.tracks["v"][1]))
    assert torch.equal(mean.cpu(), t(st.normalised()["v"]))


# ----------------------------------------------------------------------------- 7. end to end, tiny model
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)


def _model(cfg, seed=0, heads=None):
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m.load({k: t(v) for k, v in model_state(cfg, seed).items()})
    if heads is not None:
        m._model.update_pred_head(heads)
    return m


def _windows(video, starts, T):
    return _gather_ref(video, starts, T)


def _yardstick(m, video, starts, batch_size, augment, use_amp):
    """The existing public path: the same clip windows materialised on the host, `predict` on the same batches in the same
    order, ScoreStitcher.add per clip (plain) or add_views per view, plain first (augmented).  Returns (sums, support,
    bytes of frames handed to predict)."""
    T = m._args.clip_len
    L = video.shape[0]
    st, moved = None, 0
    for lo in range(0, len(starts), batch_size):
        ss = starts[lo:lo + batch_size]
        batch = _windows(video, ss, T)
        _, sc = m.predict(batch, use_amp=use_amp)
        moved += batch.numel()
        if st is None:
            st = E.ScoreStitcher([("v", L, 25.0)], sc.shape[-1])
        if augment:
            _, sf = m.predict(batch, use_amp=use_amp, augment_inference=True)
            moved += batch.numel()
        for i, s in enumerate(ss):
            if augment:
                st.add_views("v", s, sc[i][None])
                st.add_views("v", s, sf[i][None])
            else:
                st.add("v", s, sc[i])
    return st.tracks["v"][0], st.tracks["v"][1], moved


@pytest.fixture(scope="module")
def tiny_model():
    return _model(TINY)


@pytest.fixture(scope="module")
def tiny_video():
    return t(synth.uint8_clip(4100, (37, 3, 64, 64)))


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
@pytest.mark.parametrize("use_amp", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("batch_size", [4, 5])
def test_predict_video_is_bit_identical_to_the_clip_route(tiny_model, tiny_video, batch_size, use_amp, augment):
    m = tiny_model
    m.video_chunk_bytes = 7 * 3 * 64 * 64                  # several upload chunks: batches wait for their own chunk only
    starts = E.video_clip_starts(37, 8, 6)
    assert len(starts) == 18
    sums, sup = m.predict_video(tiny_video, batch_size=batch_size, augment=augment, use_amp=use_amp)
    stats = dict(m.last_video_stats)
    ref_sums, ref_sup, _ = _yardstick(m, tiny_video, starts, batch_size, augment, use_amp)
    assert sums.dtype == np.float32 and sums.shape == (37, 4) and sup.dtype == np.int32 and sup.shape == (37,)
    assert np.array_equal(sup, ref_sup)
    assert np.array_equal(sums, ref_sums), float(np.abs(sums - ref_sums).max())
    assert float(sums.sum()) > 0 and int(sup.max()) >= 1
    assert stats == dict(frames=37, clips=18, batches=-(-18 // batch_size), views=2 if augment else 1,
                         frames_h2d_bytes=37 * 3 * 64 * 64)


def test_predict_video_batch_of_one_equals_stitch_predictions(tiny_model, tiny_video):
    m = tiny_model
    starts = E.video_clip_starts(37, 8, 6)
    loader = [dict(frame=_windows(tiny_video, [s], 8), video=["v"], start=np.array([s])) for s in starts]
    st = E.stitch_predictions(m, loader, [("v", 37, 25.0)], 4, augment=True)
    sums, sup = m.predict_video(tiny_video, batch_size=1, augment=True)
    assert np.array_equal(sums, st.tracks["v"][0]) and np.array_equal(sup, st.tracks["v"][1])
    # explicit clip starts in another order, other overlap: still the clip route on the same batches
    mine = [20, -5, 31, 3, 12, 36]
    s2, n2 = m.predict_video(tiny_video, clip_starts=mine, batch_size=4)
    r2, rn2, _ = _yardstick(m, tiny_video, mine, 4, False, True)
    assert np.array_equal(s2, r2) and np.array_equal(n2, rn2)
    s3, n3 = m.predict_video(tiny_video, overlap_len=4, batch_size=4)
    r3, rn3, _ = _yardstick(m, tiny_video, E.video_clip_starts(37, 8, 4), 4, False, True)
    assert np.array_equal(s3, r3) and np.array_equal(n3, rn3)


@pytest.mark.parametrize("kind", ["no_displacement", "double_head"])
def test_predict_video_other_head_layouts(tiny_video, kind):
    if kind == "no_displacement":
        m = _model(dict(TINY, radi_displacement=0), seed=2)
    else:
        m = _model(TINY, seed=3, heads=[4, 5])             # [K+1, K2+1] as train_tdeed.py:146 passes them
    starts = E.video_clip_starts(37, 8, 6)
    sums, sup = m.predict_video(tiny_video, batch_size=4, augment=True)
    ref_sums, ref_sup, _ = _yardstick(m, tiny_video, starts, 4, True, True)
    assert np.array_equal(sums, ref_sums) and np.array_equal(sup, ref_sup) and float(sums.sum()) > 0


# ----------------------------------------------------------------------------- 8. end to end, full size
CFG2 = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4, num_classes=4,
            radi_displacement=2)


def test_predict_video_full_size_once():
    m = _model(CFG2, seed=5)
    L, fb = 430, 3 * 224 * 224
    video = ops.fill_u8_hash((L, 3, 224, 224), 77, DEV).cpu()
    starts = E.video_clip_starts(L, 100, 75)
    assert len(starts) == 15
    sums, sup = m.predict_video(video, batch_size=8, augment=True)
    stats = dict(m.last_video_stats)
    ref_sums, ref_sup, moved = _yardstick(m, video, starts, 8, True, True)
    assert np.array_equal(sup, ref_sup)
    assert np.array_equal(sums, ref_sums), float(np.abs(sums - ref_sums).max())
    assert stats["batches"] == 2 and stats["clips"] == 15 and stats["views"] == 2
    assert stats["frames_h2d_bytes"] == 430 * 150528 and moved == 15 * 2 * 100 * 150528, \
        f"predict_video moved {stats['frames_h2d_bytes']} frame bytes to the device, the clip route {moved}"


# ----------------------------------------------------------------------------- 9. / 10.
def test_predict_video_frame_sources_and_repeat(tiny_model, tiny_video):
    m = tiny_model
    m.video_chunk_bytes = 5 * 3 * 64 * 64
    a = m.predict_video(tiny_video, batch_size=4, augment=True)
    b = m.predict_video(tiny_video.pin_memory(), batch_size=4, augment=True)
    assert m.last_video_stats["frames_h2d_bytes"] == tiny_video.numel()
    c = m.predict_video(tiny_video.to(DEV), batch_size=4, augment=True)
    assert m.last_video_stats["frames_h2d_bytes"] == 0
    d = m.predict_video(tiny_video, batch_size=4, augment=True)
    for other in (b, c, d):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])


def test_predict_video_refuses_a_video_that_does_not_fit(tiny_model, tiny_video, monkeypatch):
    launched = []
    for gather in ("clip_gather", "clip_gather_seg", "rows_gather", "rows_gather_seg"):       # every gather the model may call
        monkeypatch.setattr(ops, gather, lambda *a, **k: launched.append(1))
    with pytest.raises(ValueError, match="max_resident_bytes"):
        tiny_model.predict_video(tiny_video, max_resident_bytes=tiny_video.numel() - 1)
    assert not launched
