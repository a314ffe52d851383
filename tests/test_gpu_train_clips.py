"""Training batches drawn from resident videos on the MI355X: the strided gather, the gather-and-blend and the label kernel
against torch indexing / ops_bwd.mix_frames / trainclips.rasterise_labels (exact), `trainclips.ResidentClips` against batches
assembled on the host from the same table and draws, and `TDEEDModel.epoch()` fed by it against the same epoch fed by a plain
list of host batch dicts.  -m gpu only."""
import random

import numpy as np
import pytest
import torch

from helpers import load_golden, cfg_ns
from tdeed_amd import feeder, ops, ops_bwd, synth
from tdeed_amd import trainclips as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 24, 32), (3, 6, 6), (3, 5, 7)]            # 2304 B (16-byte path), 108 B (4-byte mix path), 105 B (byte paths)
IDS = ["v16_2304B", "quad_108B", "bytes_105B"]
LENGTHS = [3, 7, 37]
T = 8


def _i64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64).to(DEV)


def packed_videos(shape, seed=5, offset=0):
    """The three videos packed one after the other, every byte non-zero (a byte of a neighbouring video in a window
    could not pass for padding).  offset=1: a view one byte into a larger buffer (unaligned for every vector path)."""
    L = sum(LENGTHS)
    n = L * int(np.prod(shape))
    store = (ops.fill_u8_hash((n + offset,), seed, DEV) % 255 + 1).to(torch.uint8).contiguous()
    video = store[offset:].view((L,) + shape)
    assert video.is_contiguous() and video.data_ptr() % 16 == (offset % 16 if offset else 0) and int(video.min()) >= 1
    return video


def hand_tables(stride):
    """Per video: a negative base, a window over the end, windows wholly outside (before / behind: the one behind video 0
    or 1 would land inside the next video), base 0 (on video 0 the overhang would land inside video 1), the last frame."""
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    first, base, nfr = [], [], []
    for v, L in enumerate(LENGTHS):
        for b in (-3, L - 2, L + 5, -T * stride - 1, 0, L - 1, -(T - 1) * stride):
            first.append(int(offs[v]))
            base.append(b)
            nfr.append(L)
    return np.array(first), np.array(base), np.array(nfr)


def host_gather(video_cpu, first, base, nfr, stride):
    out = torch.zeros((len(first), T) + tuple(video_cpu.shape[1:]), dtype=torch.uint8)
    n_pad = 0
    for b in range(len(first)):
        for t in range(T):
            f = int(base[b]) + t * stride
            if 0 <= f < int(nfr[b]):
                out[b, t] = video_cpu[int(first[b]) + f]
            else:
                n_pad += 1
    return out, n_pad


# ----------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_train_clip_gather_equals_torch_indexing(shape, stride):
    first, base, nfr = hand_tables(stride)
    B = len(first)
    for offset in (0, 1):                                             # aligned buffer, then the one-byte-offset view
        video = packed_videos(shape, offset=offset)
        want, n_pad = host_gather(video.cpu(), first, base, nfr, stride)
        out = torch.full((B, T) + shape, 9, dtype=torch.uint8, device=DEV)
        ops.train_clip_gather(video, _i64(first), _i64(base), _i64(nfr), T, stride, out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), (shape, stride, offset)
        assert n_pad > B and int((want.flatten(2).max(dim=2).values == 0).sum()) == n_pad     # real frames have no zero row
    assert (first[2] + base[2] < sum(LENGTHS)) and base[2] >= nfr[2]      # video 0, base L+5: lands inside video 1


def test_train_clip_entry_points_check_their_arguments():
    from tdeed_amd._lib import call, HipCallError
    P = 1 << 20
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_train_clip_gather_u8", None, 4, 48, P, P, P, 1, 1, 1, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_train_clip_gather_u8", P, 4, 48, P, P, None, 1, 1, 1, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_train_clip_gather_u8", P, 4, 48, P, P, P, 1, 0, 1, P, None)
    with pytest.raises(HipCallError, match="stride"):
        call("tdeed_train_clip_gather_u8", P, 4, 48, P, P, P, 1, 1, 0, P, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_train_clip_gather_u8", P, 4, 48, P, P, P, 700, 100, 1, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_train_clip_gather_mix_f32", P, 4, 48, P, P, P, P, P, P, None, 1, 1, 1, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_train_clip_gather_mix_f32", P, 4, 48, P, P, P, P, P, P, P, 1, -1, 1, P, None)
    with pytest.raises(HipCallError, match="stride"):
        call("tdeed_train_clip_gather_mix_f32", P, 4, 48, P, P, P, P, P, P, P, 1, 1, -2, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_clip_labels", P, None, 1, 8, 1, 1, P, P, P, 1, 1, P, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_clip_labels", P, P, 1, 0, 1, 1, P, P, P, 1, 1, P, P, None)
    with pytest.raises(HipCallError, match="stride"):
        call("tdeed_clip_labels", P, P, 1, 8, 0, 1, P, P, P, 1, 1, P, P, None)
    with pytest.raises(HipCallError, match="radius"):
        call("tdeed_clip_labels", P, P, 1, 8, 1, -1, P, P, P, 1, 1, P, P, None)
    video = packed_videos((3, 6, 6))
    tab = _i64([0, 0])
    with pytest.raises(ValueError):
        ops.train_clip_gather(video, tab, tab, tab[:1], T, 1, torch.empty((2, T, 3, 6, 6), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.train_clip_gather(video, tab, tab, tab, T, 1, torch.empty((1, T, 3, 6, 6), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.train_clip_gather(video, tab.int(), tab.int(), tab.int(), T, 1,
                              torch.empty((2, T, 3, 6, 6), dtype=torch.uint8, device=DEV))


# ----------------------------------------------------------------------------- 2. labels
def _labels_on_device(tab, ids, T_, S, r):
    cv = _i64(tab.clip_video[ids])
    cb = _i64(tab.clip_base[ids])
    ev = [torch.from_numpy(a).to(DEV) for a in (tab.ev_off, tab.ev_frame, tab.ev_class)]
    return ops.clip_labels(cv, cb, T_, S, r, *ev)


def test_clip_labels_equal_the_host_rule_on_every_fixture_case():
    meta, _ = load_golden("train_clips")
    for case in meta["cases"]:
        T_, S, r = case["clip_len"], case["stride"], case["radi_displacement"]
        tab = TC.train_clip_table(meta["videos"], meta["classes"], T_, S, case["overlap"], case["pad_len"])
        ids = np.arange(len(tab.clip_video))
        want, wantD = TC.rasterise_labels(tab, ids, T_, S, r)
        label, labelD = _labels_on_device(tab, ids, T_, S, r)
        torch.cuda.synchronize()
        assert label.dtype == labelD.dtype == torch.int64
        assert torch.equal(label.cpu(), torch.from_numpy(want)), case
        assert torch.equal(labelD.cpu(), torch.from_numpy(wantD)), case
        assert want.any() and (r == 0 or (wantD < 0).any())


def test_clip_labels_with_300_events_and_without_any():
    rs = np.random.RandomState(4)
    classes = {"a": 1, "b": 2, "c": 3}
    names = list(classes)
    busy = dict(video="busy", num_frames=100, events=[dict(frame=int(rs.randint(0, 100)), label=names[int(rs.randint(0, 3))])
                                                      for _ in range(300)])
    quiet = dict(video="quiet", num_frames=20, events=[])
    for S, r in ((2, 2), (1, 0), (3, 1)):
        tab = TC.train_clip_table([quiet, busy, quiet], classes, T, S)
        ids = np.arange(len(tab.clip_video))
        want, wantD = TC.rasterise_labels(tab, ids, T, S, r)
        label, labelD = _labels_on_device(tab, ids, T, S, r)
        torch.cuda.synchronize()
        assert torch.equal(label.cpu(), torch.from_numpy(want)) and torch.equal(labelD.cpu(), torch.from_numpy(wantD))
        assert want[tab.clip_video[ids] == 1].all(axis=1).any() and not want[tab.clip_video[ids] != 1].any()
    none = TC.train_clip_table([quiet], classes, T, 1)
    label, labelD = _labels_on_device(none, np.arange(len(none.clip_video)), T, 1, 2)
    torch.cuda.synchronize()
    assert int(label.abs().max()) == 0 and int(labelD.abs().max()) == 0


# ----------------------------------------------------------------------------- 3. gather + mixup
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_mix_equals_mix_frames_on_the_gathered_clips(shape, stride):
    first, base, nfr = hand_tables(stride)
    B = len(first)
    perm = np.random.RandomState(7).permutation(B)
    fb_, bb_, nb_ = first[perm], base[perm], nfr[perm]
    # operand b of the first three clips: wholly padded, like operand a of clips 2 and 3 -> one or both operands padded
    fb_[:3], bb_[:3], nb_[:3] = first[[2, 3, 2]], base[[2, 3, 2]], nfr[[2, 3, 2]]
    lam_np = np.concatenate([[0.0, 1.0, 0.5, 0.123456, 1e-8], np.random.RandomState(8).beta(0.2, 0.2, B - 5)]).astype(np.float32)
    lam = torch.from_numpy(lam_np).to(DEV)
    for offset in (0, 1):
        video = packed_videos(shape, offset=offset)
        ta = tuple(_i64(x) for x in (first, base, nfr))
        tb = tuple(_i64(x) for x in (fb_, bb_, nb_))
        a = ops.train_clip_gather(video, *ta, T, stride, torch.empty((B, T) + shape, dtype=torch.uint8, device=DEV))
        b = ops.train_clip_gather(video, *tb, T, stride, torch.empty((B, T) + shape, dtype=torch.uint8, device=DEV))
        want = ops_bwd.mix_frames(a, b, lam)
        got = ops.train_clip_gather_mix(video, ta, tb, lam, T, stride)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got, want), (shape, stride, offset, float((got - want).abs().max()))
        pad_a = a.flatten(2).max(dim=2).values == 0
        pad_b = b.flatten(2).max(dim=2).values == 0
        assert bool((pad_a & pad_b).any()) and bool((pad_a & ~pad_b).any()) and bool((~pad_a & pad_b).any())
        assert float(got.max()) > 1.0


# ----------------------------------------------------------------------------- 4. the loader
CLASSES = {"dive": 1, "turn": 2, "land": 3}


def tiny_set(shape, lengths=(3, 7, 37, 20), seed=40):
    ev = lambda *pairs: [dict(frame=f, label=l) for f, l in pairs]     # noqa: E731
    events = [ev((1, "dive")), ev((0, "turn"), (6, "land")), ev((0, "dive"), (1, "turn"), (17, "land"), (19, "dive"), (36, "turn")),
              ev((9, "land"), (8, "dive"))]
    videos = [dict(video=f"v{n:03d}", num_frames=n, events=events[i % 4]) for i, n in enumerate(lengths)]
    frames = [torch.from_numpy(synth.uint8_clip(seed + i, (n,) + shape)) for i, n in enumerate(lengths)]
    return videos, frames


def host_batches(videos, frames, clip_len, stride, overlap, r, mixup, dataset_len, batch_size, seed, passes=1, drop_last=False):
    """What the reference's DataLoader would hand to epoch(): the table, the draws and the label rule on the host, the
    clips by plain indexing."""
    tab = TC.train_clip_table(videos, CLASSES, clip_len, stride, overlap)
    draws = TC.ClipDraws(len(tab.clip_video), dataset_len, batch_size, mixup, seed, drop_last)

    def clips(ids):
        out = torch.zeros((len(ids), clip_len) + tuple(frames[0].shape[1:]), dtype=torch.uint8)
        for k, c in enumerate(ids):
            v, base = int(tab.clip_video[c]), int(tab.clip_base[c])
            for t_ in range(clip_len):
                f = base + t_ * stride
                if 0 <= f < frames[v].shape[0]:
                    out[k, t_] = frames[v][f]
        return out
    batches = []
    for _ in range(passes):
        for ia, ib in draws:
            lab, labD = TC.rasterise_labels(tab, ia, clip_len, stride, r)
            b = dict(frame=clips(ia), label=torch.from_numpy(lab))
            if r > 0:
                b["labelD"] = torch.from_numpy(labD)
            if mixup:
                lab2, labD2 = TC.rasterise_labels(tab, ib, clip_len, stride, r)
                b.update(frame2=clips(ib), label2=torch.from_numpy(lab2))
                if r > 0:
                    b["labelD2"] = torch.from_numpy(labD2)
            batches.append(b)
    return batches


@pytest.mark.parametrize("source", ["host", "pinned", "device"])
@pytest.mark.parametrize("mixup", [False, True], ids=["plain", "mixup"])
def test_resident_clips_batches_equal_the_host_batches_over_two_passes(mixup, source):
    shape = (3, 24, 32)
    videos, frames = tiny_set(shape)
    kw = dict(clip_len=8, stride=2, overlap=1, mixup=mixup, dataset_len=11, batch_size=4, seed=21)
    want = host_batches(videos, frames, r=2, passes=2, **kw)
    src = {"host": lambda f: f, "pinned": lambda f: f.pin_memory(), "device": lambda f: f.to(DEV)}[source]
    loader = TC.ResidentClips(videos, [src(f) for f in frames], CLASSES, radi_displacement=2, device=DEV,
                              chunk_bytes=5 * 2304, **kw)                      # several upload chunks, some spanning videos
    assert len(loader) == 3 and loader.depth == 3                             # 6 batches through 3 ring entries
    rs = np.random.RandomState(3)
    n = 0
    for _ in range(2):
        for got in feeder.prefetch(loader, DEV):
            w = want[n]
            keys = {k for k in got if not k.startswith("_")}
            B = w["label"].shape[0]
            assert B == (3 if n % 3 == 2 else 4)
            for k in ("label", "labelD") + (("label2", "labelD2") if mixup else ()):
                assert got[k].dtype == torch.int64 and torch.equal(got[k].cpu(), w[k]), (n, k)
            if mixup:
                assert keys == {"label", "labelD", "label2", "labelD2", "mix"}
                lam = torch.from_numpy(rs.beta(0.2, 0.2, B).astype(np.float32)).to(DEV)
                mixed = got["mix"](lam)
                assert torch.equal(mixed, ops_bwd.mix_frames(w["frame"].to(DEV), w["frame2"].to(DEV), lam)), n
                a, b = (ops.train_clip_gather(loader.video, *tabs, 8, 2, torch.empty((B, 8) + shape, dtype=torch.uint8, device=DEV))
                        for tabs in (got["mix"].tabs_a, got["mix"].tabs_b))
                assert torch.equal(a.cpu(), w["frame"]) and torch.equal(b.cpu(), w["frame2"]), n
            else:
                assert keys == {"frame", "label", "labelD"}
                assert got["frame"].dtype == torch.uint8 and torch.equal(got["frame"].cpu(), w["frame"]), n
            n += 1
    assert n == 6
    loader.reseed(21)                                                          # the draw stream starts anew
    first = next(iter(feeder.prefetch(loader, DEV)))
    assert torch.equal(first["label"].cpu(), want[0]["label"]) and torch.equal(first["labelD"].cpu(), want[0]["labelD"])


def test_resident_clips_explicit_wait_and_done_on_the_consumers_stream():
    videos, frames = tiny_set((3, 6, 6))
    kw = dict(clip_len=8, stride=1, overlap=0.5, mixup=False, dataset_len=11, batch_size=2, seed=2, drop_last=True)
    want = host_batches(videos, frames, r=0, **kw)
    loader = TC.ResidentClips(videos, frames, CLASSES, radi_displacement=0, device=DEV, **kw)
    st = torch.cuda.Stream()
    held = []
    with torch.cuda.stream(st):
        for w, got in zip(want, loader):
            assert "labelD" not in got and "_slot" in got
            feeder.wait(got)
            held.append((got["frame"].clone(), got["label"].clone()))     # queued on st, after the arrival event
            feeder.done(got)
        st.synchronize()
    assert len(held) == len(want) == 5
    for (fr, lab), w in zip(held, want):
        assert torch.equal(fr.cpu(), w["frame"]) and torch.equal(lab.cpu(), w["label"])
    with pytest.raises(RuntimeError, match="never released"):
        list(loader)                                                      # batches kept and never released


def test_resident_clips_refuse_what_does_not_fit_before_uploading(monkeypatch):
    videos, frames = tiny_set((3, 6, 6))

    def no_upload(*a, **k):
        raise AssertionError("uploaded before the check")
    monkeypatch.setattr(feeder, "PackedUpload", no_upload)
    total = sum(f.numel() for f in frames)
    kw = dict(clip_len=8, dataset_len=4, batch_size=2, seed=0, device=DEV)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        TC.ResidentClips(videos, frames, CLASSES, max_resident_bytes=total - 1, **kw)
    other = [frames[0], frames[1][:, :, :5], frames[2], frames[3]]
    with pytest.raises(ValueError, match="geometry"):
        TC.ResidentClips(videos, other, CLASSES, **kw)
    with pytest.raises(ValueError):
        TC.ResidentClips(videos, frames[:3], CLASSES, **kw)
    with pytest.raises(ValueError):
        TC.ResidentClips(videos, frames, CLASSES, radi_displacement=-1, **kw)
    with pytest.raises(AssertionError, match="uploaded before"):
        TC.ResidentClips(videos, frames, CLASSES, max_resident_bytes=total, **kw)      # exactly fitting: goes on to upload


# ----------------------------------------------------------------------------- 5. epoch()
def _tiny_model():
    from tdeed_amd.model import TDEEDModel
    meta, _ = load_golden("tiny_rny002_gsf")
    torch.manual_seed(11)
    return TDEEDModel(device=DEV, args=cfg_ns(meta["cfg"])), meta


def _train_once(make_loader):
    m, meta = _tiny_model()
    opt, _ = m.get_optimizer({"lr": 3e-4})
    loader = make_loader(meta)
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    loss = m.epoch(loader, optimizer=opt)
    torch.cuda.synchronize()
    after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(before[k], after[k]) for k in after)          # the epoch trained
    return loss, after


def _spread(a, b):
    return max(float((a[k].double() - b[k].double()).abs().max()) for k in a if a[k].is_floating_point())


def test_training_epoch_fed_by_resident_clips_equals_the_host_fed_epoch():
    """Mixup, radi_displacement = 2, the tiny 200MF model.  The host-fed epoch is run twice: when loss and parameters repeat
    bit for bit the resident epoch must match bit for bit; otherwise its distance is bounded by twice the run-to-run spread.
    Measured on an MI355X: the host-fed epoch repeats exactly (spread 0.0 in the loss and in every parameter), so the exact
    branch is the one that runs, and the resident epoch matched it exactly."""
    def inputs(meta):
        cfg = meta["cfg"]
        videos, frames = tiny_set((3, meta["H"], meta["W"]), lengths=(20, 37, 9), seed=60)
        kw = dict(clip_len=cfg["clip_len"], stride=1, overlap=1, mixup=True, dataset_len=4, batch_size=2, seed=31)
        return videos, frames, cfg["radi_displacement"], kw

    def host(meta):
        videos, frames, r, kw = inputs(meta)
        return host_batches(videos, frames, r=r, **kw)

    def res(meta):
        videos, frames, r, kw = inputs(meta)
        return TC.ResidentClips(videos, frames, CLASSES, radi_displacement=r, device=DEV, **kw)
    l1, p1 = _train_once(host)
    l2, p2 = _train_once(host)
    lr_, pr = _train_once(res)
    assert np.isfinite(l1) and np.isfinite(lr_)
    spread_l, spread_p = abs(l1 - l2), _spread(p1, p2)
    print(f"host-fed run-to-run spread: loss {spread_l:.3e}, parameters {spread_p:.3e}; "
          f"resident vs host: loss {abs(lr_ - l1):.3e}, parameters {_spread(pr, p1):.3e}")
    if spread_l == 0.0 and all(torch.equal(p1[k], p2[k]) for k in p1):
        assert lr_ == l1
        assert all(torch.equal(pr[k], p1[k]) for k in p1)
    else:
        assert abs(lr_ - l1) <= 2 * spread_l
        assert _spread(pr, p1) <= 2 * spread_p


def test_validation_epoch_fed_by_resident_clips_equals_the_host_fed_one():
    m, meta = _tiny_model()
    cfg = meta["cfg"]
    videos, frames = tiny_set((3, meta["H"], meta["W"]), lengths=(20, 37, 9), seed=60)
    kw = dict(clip_len=cfg["clip_len"], stride=2, overlap=1, mixup=False, dataset_len=5, batch_size=2, seed=33)
    want = m.epoch(host_batches(videos, frames, r=cfg["radi_displacement"], **kw))
    got = m.epoch(TC.ResidentClips(videos, frames, CLASSES, radi_displacement=cfg["radi_displacement"], device=DEV, **kw))
    assert np.isfinite(want) and got == want
