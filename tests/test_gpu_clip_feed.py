"""The device-decoded clip feed on the MI355X: the pixel kernel with a row table (ops.jpeg_pixels_rows) against the numpy
model and against ops.jpeg_pixels, and `feeder.device_clip_batches` against `feeder.clip_batches` bit for bit -- padding,
stride, table sets, fallback frames, a slot that is reused, the mixup twin, a damaged frame, and a training epoch fed by
either.  -m gpu only."""
import io
import os
import random
import shutil

import numpy as np
import pytest
import torch

import jpeg_cases as J
from helpers import cfg_ns, load_golden
from tdeed_amd import feeder, jpegdev, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENC = ["24x32_420_q90.jpg", "24x32_420_q100.jpg", "24x32_420_q30opt.jpg", "24x32_420_q75rst3.jpg"]
SHAPE, T, B = (3, 24, 32), 4, 2


# ----------------------------------------------------------------------------- 1. the kernel with a row table
def _grey(h, w):
    """three greyscale files of one size (the fixtures hold one greyscale file, 24 x 32)"""
    from PIL import Image
    out = []
    for i, q in enumerate((90, 100, 75)):
        px = np.random.default_rng(70 + i).integers(0, 256, (h, w), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(px, "L").save(buf, "JPEG", quality=q)
        out.append(buf.getvalue())
    return out


def _kernel_case(samp, h, w):
    if samp == "grey":
        datas = _grey(h, w)
        refs = [jpegdev.decode_reference(d).rgb for d in datas]
    else:
        names = [f"{h}x{w}_{samp}_{e}.jpg" for e in ("q90", "q100", "q75rst3")]
        datas, refs = [J.data(n) for n in names], [J.reference(n).rgb for n in names]
    return datas, refs


@pytest.mark.parametrize("samp,h,w", [("444", 17, 49), ("422", 23, 37), ("420", 17, 49), ("grey", 17, 49),
                                      ("444", 1, 1), ("422", 1, 1), ("420", 1, 1), ("grey", 1, 1)])
def test_pixels_land_in_the_rows_of_the_table(samp, h, w):
    datas, refs = _kernel_case(samp, h, w)
    pk = jpegdev.pack_frames(datas)
    assert pk.fallback == [] and (pk.height, pk.width) == (h, w) and jpegdev.SAMPLING_NAMES[pk.samp].replace(":", "") == samp
    dj = feeder.DeviceJpegs(pk, torch.device(DEV), 3, rows=[4, -1, 0])
    dj.stream_through(pk.stream_np.size)
    (lo, hi, waves), = dj.chunks
    fc = ops.jpeg_frame_coeffs(w, h, pk.samp)
    coeff = torch.zeros(3 * fc, dtype=torch.int16, device=DEV)
    ops.jpeg_entropy(dj.stream, dj.segments, waves, dj.table_sets, w, h, pk.samp, 0, 3, coeff, dj.status)
    out = torch.full((6, 3, h, w), 0xA5, dtype=torch.uint8, device=DEV)
    assert dj.dst_row.tolist() == [4, -1, 0]
    ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out, dj.dst_row, 0, 3, pk.samp)
    torch.cuda.synchronize()
    assert not dj.status.cpu().numpy().any()
    got = out.cpu().numpy()
    assert np.array_equal(got[4], refs[0]) and np.array_equal(got[0], refs[2])
    assert (got[[1, 2, 3, 5]] == 0xA5).all()
    # rows outside the buffer store nothing either; a batch-shaped buffer is flattened to rows
    out2 = torch.full((2, 3, 3, h, w), 0xA5, dtype=torch.uint8, device=DEV)
    ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out2, torch.tensor([6, 2, -5], dtype=torch.int32, device=DEV), 0, 3, pk.samp)
    got2 = out2.cpu().numpy().reshape(6, 3, h, w)
    assert np.array_equal(got2[2], refs[1]) and (got2[[0, 1, 3, 4, 5]] == 0xA5).all()
    # the identity table is ops.jpeg_pixels
    same = torch.full((3, 3, h, w), 0x5A, dtype=torch.uint8, device=DEV)
    plain = torch.full((3, 3, h, w), 0x5A, dtype=torch.uint8, device=DEV)
    ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, same, torch.arange(3, dtype=torch.int32, device=DEV), 0, 3, pk.samp)
    ops.jpeg_pixels(coeff, dj.frame_set, dj.table_sets, plain, 0, 3, pk.samp)
    assert torch.equal(same, plain) and np.array_equal(plain.cpu().numpy(), np.stack(refs))
    # a frame range inside the pack: frame 1 alone, its coefficients at the start of the buffer
    one = torch.full((6, 3, h, w), 0xA5, dtype=torch.uint8, device=DEV)
    ops.jpeg_pixels_rows(coeff[fc:], dj.frame_set, dj.table_sets, one, torch.tensor([0, 5, 1], dtype=torch.int32, device=DEV), 1, 1, pk.samp)
    got1 = one.cpu().numpy()
    assert np.array_equal(got1[5], refs[1]) and (got1[:5] == 0xA5).all()


def test_jpeg_pixels_rows_validates_its_tensors():
    pk = jpegdev.pack_frames([J.data(ENC[0])])
    dj = feeder.DeviceJpegs(pk, torch.device(DEV), 1, rows=[0])
    coeff = torch.zeros(ops.jpeg_frame_coeffs(32, 24, pk.samp), dtype=torch.int16, device=DEV)
    out = torch.zeros((1,) + SHAPE, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError, match="dst_row"):
        ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out, dj.dst_row.long(), 0, 1, pk.samp)
    with pytest.raises(TypeError, match="dst_row"):
        ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out, dj.dst_row.cpu(), 0, 1, pk.samp)
    with pytest.raises(ValueError, match="outside"):
        ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out, dj.dst_row, 0, 2, pk.samp)
    with pytest.raises(ValueError, match="coeff holds"):
        ops.jpeg_pixels_rows(coeff[:-1], dj.frame_set, dj.table_sets, out, dj.dst_row, 0, 1, pk.samp)
    with pytest.raises(TypeError):
        ops.jpeg_pixels_rows(coeff, dj.frame_set, dj.table_sets, out.int(), dj.dst_row, 0, 1, pk.samp)


# ----------------------------------------------------------------------------- 2. the feed against the host feed
def _tree(root, replace_a=None, replace_b=None):
    """va: ten files frame<n>.jpg; vb: eight files <nnnn>.jpg; both cycle through the four table sets"""
    os.makedirs(os.path.join(root, "va"))
    os.makedirs(os.path.join(root, "vb"))
    for n in range(10):
        shutil.copy(J.fixture_path((replace_a or {}).get(n, ENC[n % 4])), os.path.join(root, "va", f"frame{n}.jpg"))
    for n in range(8):
        shutil.copy(J.fixture_path((replace_b or {}).get(n, ENC[(n + 1) % 4])), os.path.join(root, "vb", f"{n:04d}.jpg"))


def _descr(root, video, start, end, stride=1):
    ds = "soccernetball" if video == "va" else "finediving"
    return dict(paths=feeder.load_paths(root, ds, video, start, end, stride=stride), stride=stride, tag=f"{video}:{start}")


def _clips(root):
    """three batches of two: fallback frames first, the padded clips last, where the reused slot held frames"""
    cs = [_descr(root, "va", 3, 7), _descr(root, "vb", 0, 4), _descr(root, "va", 2, 10, stride=2), _descr(root, "vb", 4, 8),
          _descr(root, "va", -1, 3), _descr(root, "va", 8, 12)]
    assert cs[4]["paths"][2:4] == [1, 0] and cs[5]["paths"][2:4] == [0, 2] and cs[1]["paths"][4] == 4 and cs[0]["paths"][4] == -1
    return cs


def _host_feed(clips, shape=SHAPE, clip_len=T, batch=B):
    pool = feeder.DecodePool(2)
    try:
        return [dict(b, frame=b["frame"].clone()) for b in feeder.clip_batches(clips, batch, shape, clip_len, pool=pool, depth=2)]
    finally:
        pool.close()


def _device_feed(clips, **kw):
    """the batches' frames (clones) and per-batch stats, consumed with the explicit wait / done protocol"""
    frames, stats, extras = [], [], []
    for b in feeder.device_clip_batches(clips, B, SHAPE, T, device=DEV, **kw):
        stats.append(dict(feeder.last_decode_stats))
        feeder.wait(b)
        assert b["frame"].is_cuda and b["frame"].dtype == torch.uint8 and tuple(b["frame"].shape) == (B, T) + SHAPE
        frames.append({k: b[k].clone() for k in ("frame", "frame2") if k in b})
        extras.append({k: v for k, v in b.items() if not k.startswith("_") and k not in ("frame", "frame2")})
        feeder.done(b)
    torch.cuda.synchronize()
    return frames, stats, extras


def test_feed_equals_the_host_feed(tmp_path):
    root = str(tmp_path)
    _tree(root, replace_a={5: "24x32_cmyk.jpg"}, replace_b={1: "24x32_grey_q90.jpg"})
    clips = _clips(root)
    want = _host_feed(clips)
    pool = feeder.DecodePool(2)
    cache = jpegdev.ParseCache()
    try:
        got, stats, extras = _device_feed(clips, pool=pool, depth=2, parse_cache=cache)
        again, stats2, _ = _device_feed(clips, pool=pool, depth=2, parse_cache=cache)          # second epoch: parsed already
    finally:
        pool.close()
    assert len(got) == len(want) == 3
    for g, a, w, e in zip(got, again, want, extras):
        assert torch.equal(g["frame"].cpu(), w["frame"]) and torch.equal(a["frame"], g["frame"])
        assert e == {"tag": w["tag"]}
    last = got[2]["frame"].cpu()
    assert not last[0, :1].any() and not last[1, 2:].any() and last[0, 1:].any() and last[1, :2].any()     # padding rows are zero
    assert [s["fallback_frames"] for s in stats] == [2, 0, 0] and sum(s["fallback_frames"] for s in stats) == 2
    assert [s["device_frames"] for s in stats] == [6, 8, 5] and [s["frames"] for s in stats] == [8, 8, 8]
    assert [s["table_sets"] for s in stats] == [4, 4, 3] and all(s["chunks"] == 1 and s["stream_bytes"] > 0 for s in stats)
    assert [s["segments"] > s["device_frames"] for s in stats] == [True, True, False]      # the restart files have several
    assert cache.misses == len(cache) and cache.hits > cache.misses                        # every file was parsed once
    assert stats2 == stats
    # chunks under max_coeff_bytes as decode_packed makes them: one frame per chunk
    few, stats3, _ = _device_feed(clips[2:4], max_coeff_bytes=1)
    assert stats3[0]["chunks"] == 8 and torch.equal(few[0]["frame"], got[1]["frame"])
    # the tail that does not fill a batch is dropped; nothing to do is no batch
    assert len(_device_feed(clips[:3])[0]) == 1 and _device_feed(clips[:1])[0] == []
    with pytest.raises(ValueError, match="do not fit"):
        list(feeder.device_clip_batches(clips, B, (3, 16, 16), T, device=DEV))


def test_twin_clips_share_the_slot(tmp_path):
    root = str(tmp_path)
    _tree(root)
    clips = _clips(root)[2:]
    twins = [clips[3], clips[0], clips[2], clips[1]]
    both = [dict(c, paths2=t["paths"], stride2=t["stride"]) for c, t in zip(clips, twins)]
    want, want2 = _host_feed(clips), _host_feed(twins)
    alone, _, _ = _device_feed(clips)
    got = []
    for b in feeder.prefetch(feeder.device_clip_batches(both, B, SHAPE, T, device=DEV), DEV):          # the auto hand-over
        assert "_slot" not in b and b["tag"] == [c["tag"] for c in clips[len(got) * B:len(got) * B + B]]
        got.append((b["frame"].clone(), b["frame2"].clone(), dict(feeder.last_decode_stats)))
    torch.cuda.synchronize()
    assert len(got) == 2
    for (f, f2, s), a, w, w2 in zip(got, alone, want, want2):
        assert torch.equal(f.cpu(), w["frame"]) and torch.equal(f2.cpu(), w2["frame"]) and torch.equal(f, a["frame"])
        assert s["frames"] == 2 * B * T and s["fallback_frames"] == 0
    with pytest.raises(ValueError, match="paths2"):
        list(feeder.device_clip_batches([both[0], clips[1]], B, SHAPE, T, device=DEV))


def test_damaged_frame_is_whatever_pillow_makes_of_it(tmp_path):
    root = str(tmp_path)
    _tree(root)
    name = os.path.join(root, "va", "frame5.jpg")
    data = open(name, "rb").read()
    info = jpegdev.parse(data)
    cut = data[:info.scan_start + (info.scan_end - info.scan_start) // 2]                 # truncated in the middle of its scan
    with open(name, "wb") as f:
        f.write(cut)
    # the kernels report it
    pk = jpegdev.pack_frames([cut])
    out = torch.zeros((1,) + SHAPE, dtype=torch.uint8, device=DEV)
    dj, _ = feeder.decode_packed(pk, out)
    assert pk.fallback == [] and dj.status[:pk.n_segments].cpu().numpy().any()
    clips = [_descr(root, "va", 4, 8), _descr(root, "vb", 0, 4)]
    try:
        want, exc = feeder.read_frame(name), None
    except Exception as e:          # noqa: BLE001  (whatever the installed Pillow raises is what the feed must raise)
        want, exc = None, e
    if exc is not None:
        with pytest.raises(type(exc)):
            _device_feed(clips)
        torch.cuda.synchronize()
        return
    got, stats, _ = _device_feed(clips)
    assert stats[0]["status_frames"] == [1] and stats[0]["fallback_frames"] == 1 and stats[0]["device_frames"] == 7
    assert torch.equal(got[0]["frame"][0, 1].cpu(), want)
    assert torch.equal(got[0]["frame"].cpu(), _host_feed(clips)[0]["frame"])


# ----------------------------------------------------------------------------- 3. a training epoch fed by either
def _write_video(d, n, h, w, seed):
    from PIL import Image
    os.makedirs(d)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    for i in range(n):
        base = np.stack([30 + 180 * xx / (w - 1), 40 + 170 * yy / (h - 1), 128 + 90 * np.sin(0.11 * xx + i) * np.cos(0.07 * yy)], -1)
        px = np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(px).save(os.path.join(d, f"frame{i}.jpg"), "JPEG", quality=90, subsampling=2)


def _train_once(make_loader):
    from tdeed_amd.model import TDEEDModel
    meta, _ = load_golden("tiny_rny002_gsf")
    torch.manual_seed(11)
    m = TDEEDModel(device=DEV, args=cfg_ns(meta["cfg"]))
    opt, _ = m.get_optimizer({"lr": 3e-4})
    before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    loss = m.epoch(make_loader(), optimizer=opt)
    torch.cuda.synchronize()
    after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert any(not torch.equal(before[k], after[k]) for k in after)          # the epoch trained
    return loss, after


def test_training_epoch_fed_by_the_device_feed_equals_the_host_fed_epoch(tmp_path):
    """The tiny 200MF model of the other epoch tests (fp32 engine, 64 x 64 frames, clips of 16), two batches of two clips, one
    clip padded in front and one behind.  The batches are the same bits, so loss and parameters are."""
    meta, _ = load_golden("tiny_rny002_gsf")
    cfg, h, w = meta["cfg"], meta["H"], meta["W"]
    Tm = cfg["clip_len"]
    root = str(tmp_path)
    _write_video(os.path.join(root, "vid"), 40, h, w, 900)
    clips = [dict(paths=feeder.load_paths(root, "soccernetball", "vid", s, s + Tm), stride=1) for s in (-3, 10, 20, 30)]
    assert clips[0]["paths"][2] == 3 and clips[3]["paths"][3] == 6
    labels = [synth.labels(7 + i, 2, Tm, cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.3) for i in range(2)]

    def with_labels(batches, keep):
        for b, (lab, labD) in zip(batches, labels):
            yield dict(frame=b["frame"], label=torch.from_numpy(lab), labelD=torch.from_numpy(labD).float(), **{keep: b[keep]})

    pool = feeder.DecodePool(2)

    def host():
        return with_labels(feeder.clip_batches(clips, 2, (3, h, w), Tm, pool=pool, depth=3), "_src")

    def dev():
        return with_labels(feeder.device_clip_batches(clips, 2, (3, h, w), Tm, device=DEV, depth=3), "_slot")
    try:
        l_host, p_host = _train_once(host)
        l_dev, p_dev = _train_once(dev)
    finally:
        pool.close()
    assert feeder.last_decode_stats["fallback_frames"] == 0 and feeder.last_decode_stats["device_frames"] == 2 * Tm - 6
    print(f"loss host-fed {l_host!r}, device-fed {l_dev!r}")
    assert np.isfinite(l_host) and l_dev == l_host
    assert all(torch.equal(p_dev[k], p_host[k]) for k in p_host)
