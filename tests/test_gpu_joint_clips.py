"""Joint datasets on the MI355X: the three per-clip-stride kernels against numpy and against their scalar twins,
`trainclips.JointResidentClips` against tests/golden/train_clips_joint.npz (the reference's own ActionSpotDatasetJoint),
`trainclips.JointResidentJpegClips` against `JointResidentClips` fed Pillow-decoded frames, and a two-head mixup epoch of
`TDEEDModel.epoch()` fed by the loader against the same epoch fed by host-built batch dicts.  -m gpu only."""
import itertools
import random

import numpy as np
import pytest
import torch

import joint_cases as JC
from helpers import cfg_ns, load_golden
from tdeed_amd import feeder, ops, ops_bwd
from tdeed_amd import trainclips as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8
STRIDES = [1, 2, 12, 3, 1]
SHAPES = [(3, 8, 8), (3, 5, 7)]                          # 192 B: the 16-byte / 4-byte paths; 105 B: the byte / scalar paths
IDS = ["v16_192B", "bytes_105B"]
LENGTHS = [5, 30, 9]                                    # video 0 is shorter than a clip; 44 packed frames


def _i64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int64).to(DEV)


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


def _video(shape, seed=5):
    """the three videos packed one after the other, every byte non-zero: a neighbour's byte cannot pass for padding"""
    L = sum(LENGTHS)
    return (ops.fill_u8_hash((L,) + shape, seed, DEV) % 255 + 1).to(torch.uint8).contiguous()


# B = 5 clips, one per entry of STRIDES: (video, base) -- a negative base, a window over its video's end (stride 2 from frame
# 24 of 30: the overhang would land in video 2), a stride-12 window from a negative base (frames -7, 5, 17, 29, then out), a
# window wholly behind its video (it would lie inside video 1), and the video shorter than the clip from frame 0
CLIPS = [(1, -3), (1, 24), (1, -7), (0, 6), (0, 0)]
PARTNERS = [(2, 5), (0, -2), (2, -20), (1, 0), (1, 29)]     # over the end, negative, wholly outside (before), inside, last frame


def _tables(clips):
    offs = np.concatenate([[0], np.cumsum(LENGTHS)])
    first = np.array([offs[v] for v, _ in clips])
    base = np.array([b for _, b in clips])
    nfr = np.array([LENGTHS[v] for v, _ in clips])
    return first, base, nfr


def _host_gather(video_cpu, first, base, nfr, strides):
    out = torch.zeros((len(first), T) + tuple(video_cpu.shape[1:]), dtype=torch.uint8)
    pads = 0
    for b in range(len(first)):
        for t in range(T):
            f = int(base[b]) + t * int(strides[b])
            if 0 <= f < int(nfr[b]):
                out[b, t] = video_cpu[int(first[b]) + f]
            else:
                pads += 1
    return out, pads


# ----------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_ps_equals_numpy_indexing(shape):
    video = _video(shape)
    first, base, nfr = _tables(CLIPS)
    want, pads = _host_gather(video.cpu(), first, base, nfr, STRIDES)
    out = torch.full((5, T) + shape, 9, dtype=torch.uint8, device=DEV)
    ops.train_clip_gather(video, _i64(first), _i64(base), _i64(nfr), T, _i32(STRIDES), out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    assert pads == int((want.flatten(2).max(dim=2).values == 0).sum()) and pads > 5
    assert not want[3].any() and want[4, :5].all() and not want[4, 5:].any()
    assert want[2, 1:4].flatten(1).any(dim=1).all() and not want[2, 4:].any() and not want[2, 0].any()
    # a host sequence of strides is checked and uploaded
    out2 = torch.empty_like(out)
    ops.train_clip_gather(video, _i64(first), _i64(base), _i64(nfr), T, STRIDES, out2)
    assert torch.equal(out2, out)
    # a row that points outside the packed buffer touches nothing it should not: zeros, and the neighbours stay right
    L = sum(LENGTHS)
    bad_first = first.copy()
    bad_first[[0, 3]] = [L + 7, -40]
    out.fill_(9)
    ops.train_clip_gather(video, _i64(bad_first), _i64(base), _i64(nfr), T, _i32(STRIDES), out)
    torch.cuda.synchronize()
    assert not out[0].any() and not out[3].any() and torch.equal(out[[1, 2, 4]].cpu(), want[[1, 2, 4]])
    # behind the buffer's end by the window only: first inside, first + base + t * stride outside
    edge = (_i64([L - 2]), _i64([0]), _i64([30]))
    o1 = torch.full((1, T) + shape, 9, dtype=torch.uint8, device=DEV)
    ops.train_clip_gather(video, *edge, T, _i32([1]), o1)
    torch.cuda.synchronize()
    assert torch.equal(o1[0, :2], video[L - 2:]) and not o1[0, 2:].any()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_mix_ps_equals_mix_frames_of_the_two_gathers(shape):
    video = _video(shape)
    ta = tuple(_i64(x) for x in _tables(CLIPS))
    tb = tuple(_i64(x) for x in _tables(PARTNERS))
    S = _i32(STRIDES)
    lam = torch.tensor([0.0, 1.0, 0.5, 0.123456, 1e-8], dtype=torch.float32, device=DEV)
    a = ops.train_clip_gather(video, *ta, T, S, torch.empty((5, T) + shape, dtype=torch.uint8, device=DEV))
    b = ops.train_clip_gather(video, *tb, T, S, torch.empty((5, T) + shape, dtype=torch.uint8, device=DEV))
    hb, _ = _host_gather(video.cpu(), *_tables(PARTNERS), STRIDES)
    assert torch.equal(b.cpu(), hb)
    want = ops_bwd.mix_frames(a, b, lam)
    got = ops.train_clip_gather_mix(video, ta, tb, lam, T, S)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
    pa, pb = a.flatten(2).max(dim=2).values == 0, b.flatten(2).max(dim=2).values == 0
    assert bool((pa & pb).any()) and bool((pa & ~pb).any()) and bool((~pa & pb).any()) and float(got.max()) > 1.0
    # one operand's row outside the buffer: that operand contributes zeros, nothing else changes
    bad = (_i64(_tables(PARTNERS)[0] + 10 ** 6), tb[1], tb[2])
    got = ops.train_clip_gather_mix(video, ta, bad, lam, T, S)
    torch.cuda.synchronize()
    assert torch.equal(got, ops_bwd.mix_frames(a, torch.zeros_like(b), lam))


@pytest.mark.parametrize("r", [0, 2])
def test_clip_labels_ps_equal_the_host_rule(r):
    meta, _ = JC.golden()
    case = dict(meta["cases"][0], strides=[12, 3], overlaps=[1, 1])
    parts = JC.parts_of(case, frames=False)
    _, tab = JC.joined_table(parts, T, r)
    n1 = int(tab.part_clips[1])
    # five clips at the strides [1, 2, 12, 3, 1] -- any clip may be labelled at any stride -- and then every clip at its own
    for ids, S in ((np.array([3, n1 - 1, 40, n1 + 5, len(tab.clip_video) - 1]), np.array(STRIDES)),
                   (np.arange(len(tab.clip_video)), np.repeat([12, 3], np.diff(tab.part_clips)))):
        want, wantD = TC.rasterise_labels(tab, ids, T, S, r)
        ev = [torch.from_numpy(x).to(DEV) for x in (tab.ev_off, tab.ev_frame, tab.ev_class)]
        label, labelD = ops.clip_labels(_i64(tab.clip_video[ids]), _i64(tab.clip_base[ids]), T, _i32(S), r, *ev)
        torch.cuda.synchronize()
        assert label.dtype == labelD.dtype == torch.int64
        assert torch.equal(label.cpu(), torch.from_numpy(want)) and torch.equal(labelD.cpu(), torch.from_numpy(wantD))
        assert want.any() and (r == 0 or (wantD < 0).any())
    assert want[n1:].max() > 3                                              # part 2's own class numbers


@pytest.mark.parametrize("stride", [1, 3])
def test_ps_entries_with_equal_strides_are_their_scalar_twins_bit_for_bit(stride):
    for shape in SHAPES:
        video = _video(shape)
        ta = tuple(_i64(x) for x in _tables(CLIPS))
        tb = tuple(_i64(x) for x in _tables(PARTNERS))
        S = _i32([stride] * 5)
        new = lambda: torch.empty((5, T) + shape, dtype=torch.uint8, device=DEV)      # noqa: E731
        assert torch.equal(ops.train_clip_gather(video, *ta, T, S, new()), ops.train_clip_gather(video, *ta, T, stride, new()))
        lam = torch.tensor([0.3, 0.9, 0.5, 0.0, 0.77], dtype=torch.float32, device=DEV)
        assert torch.equal(ops.train_clip_gather_mix(video, ta, tb, lam, T, S), ops.train_clip_gather_mix(video, ta, tb, lam, T, stride))
    meta, _ = JC.golden()
    case = dict(meta["cases"][0], strides=[stride, stride])
    _, tab = JC.joined_table(JC.parts_of(case, frames=False), T, 2)
    n = len(tab.clip_video)
    ev = [torch.from_numpy(x).to(DEV) for x in (tab.ev_off, tab.ev_frame, tab.ev_class)]
    cv, cb = _i64(tab.clip_video), _i64(tab.clip_base)
    a, aD = ops.clip_labels(cv, cb, T, _i32([stride] * n), 2, *ev)
    b, bD = ops.clip_labels(cv, cb, T, stride, 2, *ev)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(aD, bD) and bool(a.any())


def test_ps_entry_points_check_their_arguments():
    from tdeed_amd._lib import call, HipCallError
    P = 1 << 20
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_train_clip_gather_u8_ps", P, 4, 48, P, P, P, 1, 1, None, P, None)
    with pytest.raises(HipCallError, match="bad sizes"):
        call("tdeed_train_clip_gather_u8_ps", P, 4, 48, P, P, P, 1, 0, P, P, None)
    with pytest.raises(HipCallError, match="65535"):
        call("tdeed_train_clip_gather_u8_ps", P, 4, 48, P, P, P, 700, 100, P, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_train_clip_gather_mix_f32_ps", P, 4, 48, P, P, P, P, P, P, P, 1, 1, None, P, None)
    with pytest.raises(HipCallError, match="null pointer"):
        call("tdeed_clip_labels_ps", P, P, 1, 8, None, 1, P, P, P, 1, 1, P, P, None)
    with pytest.raises(HipCallError, match="radius"):
        call("tdeed_clip_labels_ps", P, P, 1, 8, P, -1, P, P, P, 1, 1, P, P, None)
    video = _video((3, 5, 7))
    tab = _i64([0, 0])
    out = torch.empty((2, T, 3, 5, 7), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="positive"):                       # refused on the host
        ops.train_clip_gather(video, tab, tab, tab, T, [1, 0], out)
    with pytest.raises(ValueError, match="positive"):
        ops.train_clip_gather_mix(video, (tab,) * 3, (tab,) * 3, torch.ones(2, device=DEV), T, np.array([2, -1]))
    with pytest.raises(ValueError):
        ops.train_clip_gather(video, tab, tab, tab, T, _i64([1, 1]), out)            # int64 on the device
    with pytest.raises(ValueError):
        ops.train_clip_gather(video, tab, tab, tab, T, _i32([1]), out)
    ev = [_i32([0, 1]), _i32([3]), _i32([1])]
    with pytest.raises(ValueError, match="positive"):
        ops.clip_labels(tab, tab, T, [0, 1], 1, *ev)


# ----------------------------------------------------------------------------- 2. JointResidentClips against the fixture
@pytest.mark.parametrize("ci", range(5))
def test_joint_resident_clips_equal_the_recorded_items_over_two_passes(ci):
    """Two passes of 10 items in batches of 4, 4, 2 are the first 20 recorded items: part, labels of both operands, and
    the frames -- against the reference's own arrays where they are recorded, and always against the clips gathered on
    the host from the decoded frames with each clip's own stride."""
    meta, g = JC.golden()
    case = meta["cases"][ci]
    Tc, r, mixup = case["clip_len"], case["radi_displacement"], case["mixup"]
    parts = JC.parts_of(dict(case, dataset_len=[5, 5]))
    kw = dict(clip_len=Tc, radi_displacement=r, mixup=mixup, batch_size=4, seed=case["seed"])
    loader = TC.JointResidentClips(parts, device=DEV, chunk_bytes=7 * 192, **kw)
    want = JC.host_batches(parts, Tc, r, mixup, 4, case["seed"], passes=2)
    assert len(loader) == 3 and len(want) == 6
    rs = np.random.RandomState(3)
    n = at = 0
    for _ in range(2):
        for got in feeder.prefetch(loader, DEV):
            w = want[n]
            B = w["label"].shape[0]
            assert B == (2 if n % 3 == 2 else 4)
            keys = {k for k in got if not k.startswith("_")}
            assert keys == set(case["keys"]) | {"dataset", "mix" if mixup else "frame"}
            assert got["dataset"].dtype == torch.int64 and got["dataset"].is_cuda
            assert np.array_equal(got["dataset"].cpu().numpy(), g[f"part__{ci}"][at:at + B])
            for k in case["keys"]:
                assert got[k].dtype == torch.int64
                assert np.array_equal(got[k].cpu().numpy(), g[f"{k}__{ci}"][at:at + B]), (n, k)
                assert torch.equal(got[k].cpu(), w[k]), (n, k)
            if mixup:
                S = got["mix"].strides
                assert S.dtype == torch.int32 and S.cpu().tolist() == [case["strides"][p - 1] for p in w["dataset"].tolist()]
                shape = tuple(w["frame"].shape[2:])
                a, b = (ops.train_clip_gather(loader.video, *tabs, Tc, S, torch.empty((B, Tc) + shape, dtype=torch.uint8, device=DEV))
                        for tabs in (got["mix"].tabs_a, got["mix"].tabs_b))
                lam = torch.from_numpy(rs.beta(0.2, 0.2, B).astype(np.float32)).to(DEV)
                assert torch.equal(got["mix"](lam), ops_bwd.mix_frames(w["frame"].to(DEV), w["frame2"].to(DEV), lam)), n
                frames = dict(frame=a.cpu(), frame2=b.cpu())
            else:
                assert got["frame"].dtype == torch.uint8
                frames = dict(frame=got["frame"].cpu())
            for k, f in frames.items():
                assert torch.equal(f, w[k]), (n, k)
                if k in case["frame_keys"]:
                    assert np.array_equal(f.numpy(), g[f"{k}__{ci}"][at:at + B]), (n, k)
            at += B
            n += 1
    assert n == 6 and at == 20
    loader.reseed(case["seed"])
    first = next(iter(feeder.prefetch(loader, DEV)))
    assert np.array_equal(first["label"].cpu().numpy(), g[f"label__{ci}"][:4]) and np.array_equal(first["dataset"].cpu().numpy(),
                                                                                                g[f"part__{ci}"][:4])


def test_joint_resident_clips_refuse_bad_parts():
    meta, _ = JC.golden()
    parts = JC.parts_of(meta["cases"][0])
    kw = dict(clip_len=8, batch_size=2, seed=0, device=DEV)
    with pytest.raises(ValueError, match="two"):
        TC.JointResidentClips(parts[:1], **kw)
    with pytest.raises(ValueError, match="positive"):
        TC.JointResidentClips([parts[0], dict(parts[1], stride=0)], **kw)
    with pytest.raises(ValueError, match="geometry"):
        TC.JointResidentClips([parts[0], dict(parts[1], frames=[f[:, :, :, :5] for f in parts[1]["frames"]])], **kw)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        TC.JointResidentClips(parts, max_resident_bytes=1000, **kw)


# ----------------------------------------------------------------------------- 3. JointResidentJpegClips
def _jpeg_parts(tree, strides, overlaps, dataset_len):
    jp, fr = [], []
    for k, (d, videos) in enumerate(tree):
        common = dict(videos=videos, classes=JC.CLASSES[k], stride=strides[k], overlap=overlaps[k], dataset_len=dataset_len[k])
        jp.append(dict(common, jpegs=TC.load_resident_jpegs(d, "soccernetball", videos, shard_bytes=1024)))
        fr.append(dict(common, frames=TC.load_resident_videos(d, "soccernetball", videos)))             # Pillow-decoded
    return jp, fr


def _compare(ref, got, passes=2, lam_seed=3):
    rs = np.random.RandomState(lam_seed)
    n, parts = 0, set()
    for _ in range(passes):
        for w, g in itertools.zip_longest(feeder.prefetch(ref, DEV), feeder.prefetch(got, DEV)):
            assert w is not None and g is not None
            assert {k for k in w if not k.startswith("_")} == {k for k in g if not k.startswith("_")}
            for k in w:
                if k.startswith("label") or k == "dataset":
                    assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), (n, k)
            parts |= set(w["dataset"].cpu().tolist())
            B = w["label"].shape[0]
            if "mix" in w:
                lam = torch.from_numpy(rs.beta(0.2, 0.2, B).astype(np.float32)).to(DEV)
                a, b = g["mix"](lam), w["mix"](lam)
                assert a.dtype == torch.float32 and torch.equal(a, b), n
            else:
                assert g["frame"].dtype == torch.uint8 and g["frame"].shape == w["frame"].shape
                assert torch.equal(g["frame"], w["frame"]) and bool(g["frame"].any()), n
            n += 1
    torch.cuda.synchronize()
    assert parts == {1, 2}
    return n


@pytest.mark.parametrize("route", ["420", "444_side_buffer", "streamed"])
@pytest.mark.parametrize("mixup", [False, True], ids=["plain", "mixup"])
def test_joint_resident_jpeg_clips_equal_joint_resident_clips(tmp_path, mixup, route):
    """24 x 32; part 1 at quality 90, part 2 at quality 30 with optimize=True (other table sets), strides 1 | 2.
    444_side_buffer: part 2 written 4:4:4, all of it through the side buffer.  streamed: stream_clips=True at the plan's
    smallest budget, every video's streams staged from the host."""
    tree = JC.write_trees(str(tmp_path), subsampling2=0 if route == "444_side_buffer" else 2)
    jp, fr = _jpeg_parts(tree, (1, 2), (1, 0.5), (4, 3))
    kw = dict(clip_len=6, radi_displacement=2, mixup=mixup, batch_size=3, seed=21, device=DEV)
    ref = TC.JointResidentClips(fr, **kw)
    if route == "streamed":
        probe = TC.JointResidentJpegClips(jp, stream_clips=True, **kw)
        assert probe.stats["resident_videos"] == 4
        budget = probe._plan.min_budget
        with pytest.raises(ValueError, match=f"smallest max_resident_bytes that would do is {budget}$"):
            TC.JointResidentJpegClips(jp, stream_clips=True, max_resident_bytes=budget - 1, **kw)
        got = TC.JointResidentJpegClips(jp, stream_clips=True, max_resident_bytes=budget, **kw)
        assert (got.stats["resident_videos"], got.stats["streamed_videos"]) == (0, 4) and got.stats["resident_bytes"] <= budget
        got.stage_log = []
    else:
        got = TC.JointResidentJpegClips(jp, **kw)
    st = got.stats
    assert st["frames"] == 29 and st["index_flagged"] == []
    if route == "444_side_buffer":
        assert (st["device_frames"], st["fallback_frames"]) == (14, 15)
    else:
        assert (st["device_frames"], st["fallback_frames"]) == (29, 0) and st["table_sets"] >= 2 and st["shards"] >= 2
    assert len(got) == len(ref) == 3
    assert _compare(ref, got) == 6
    if route == "streamed":
        assert len(got.stage_log) == 6 and min(got.stage_log) > 0 and max(got.stage_log) <= got._plan.region_bytes


# ----------------------------------------------------------------------------- 4. epoch()
def _two_head_model():
    from tdeed_amd.model import TDEEDModel
    meta, _ = load_golden("tiny_rny002_gsf")
    torch.manual_seed(11)
    m = TDEEDModel(device=DEV, args=cfg_ns(meta["cfg"]))
    heads = [meta["cfg"]["num_classes"] + 1, 6]                             # part 1: 3 classes, part 2: 5
    m._model.update_pred_head(heads)
    m._num_classes = sum(heads)                                             # train_tdeed.py:147-148
    return m, meta


def _epoch_inputs(meta):
    """part 1 at stride 1, part 2 at stride 2; 6 items in three batches of 2"""
    gm, g = JC.golden()
    cfg = meta["cfg"]
    assert cfg["num_classes"] == 3
    rs = np.random.RandomState(60)
    parts = []
    for k, p in enumerate(gm["parts"]):
        videos = p["videos"][1:3]
        frames = [torch.from_numpy(rs.randint(0, 256, (v["num_frames"], 3, meta["H"], meta["W"])).astype(np.uint8)) for v in videos]
        parts.append(dict(videos=videos, frames=frames, classes=p["classes"], stride=k + 1, overlap=1, dataset_len=3))
    return parts, dict(clip_len=cfg["clip_len"], radi_displacement=cfg["radi_displacement"], mixup=True, batch_size=2, seed=31)


def _train_once(make_loader):
    m, meta = _two_head_model()
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


def test_two_head_mixup_epoch_fed_by_joint_resident_clips_equals_the_host_fed_epoch():
    """The tiny 200MF model with update_pred_head([4, 6]), mixup, three batches.  Loss and every parameter bit for bit."""
    def host(meta):
        parts, kw = _epoch_inputs(meta)
        batches = JC.host_batches(parts, kw["clip_len"], kw["radi_displacement"], True, 2, kw["seed"])
        assert len(batches) == 3 and {int(x) for b in batches for x in b["dataset"]} == {1, 2}
        return batches

    def res(meta):
        parts, kw = _epoch_inputs(meta)
        return TC.JointResidentClips(parts, device=DEV, **kw)
    l1, p1 = _train_once(host)
    lr_, pr = _train_once(res)
    spread = max(float((pr[k].double() - p1[k].double()).abs().max()) for k in p1 if p1[k].is_floating_point())
    print(f"joint resident vs host-fed: loss {abs(lr_ - l1):.3e}, parameters {spread:.3e}")
    assert np.isfinite(l1) and lr_ == l1
    assert all(torch.equal(pr[k], p1[k]) for k in p1)


def test_two_head_validation_epoch_fed_by_joint_resident_clips_equals_the_host_fed_one():
    m, meta = _two_head_model()
    parts, kw = _epoch_inputs(meta)
    kw = dict(kw, mixup=False)
    want = m.epoch(JC.host_batches(parts, kw["clip_len"], kw["radi_displacement"], False, 2, kw["seed"]))
    got = m.epoch(TC.JointResidentClips(parts, device=DEV, **kw))
    assert np.isfinite(want) and got == want
