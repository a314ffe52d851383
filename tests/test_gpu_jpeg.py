"""JPEG decode on the MI355X (csrc/jpeg.hip): coefficients against the numpy model, pixels against Pillow's decode, both
exactly; `feeder.load_video_device` against `feeder.load_video`; the consumers of resident videos fed either way.
Well-formed streams only (damaged ones run on the host program, tests/test_jpegdev_host.py).  -m gpu only."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import jpeg_cases as J
from helpers import ROOT, cfg_ns, model_state, t
from tdeed_amd import evalutil as E
from tdeed_amd import feeder, jpegdev, ops
from tdeed_amd import trainclips as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _synthetic(h, w, seed, noise=12):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([30 + 180 * xx / (w - 1), 40 + 170 * yy / (h - 1), 128 + 90 * np.sin(0.11 * xx + seed) * np.cos(0.07 * yy)], -1)
    return np.clip(base + rng.integers(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)


def _write_video(d, n, h, w, seed, **kw):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        Image.fromarray(_synthetic(h, w, seed + i)).save(os.path.join(d, f"frame{i}.jpg"), "JPEG", **kw)


# ----------------------------------------------------------------------------- 1. the two kernels on the fixtures
@pytest.mark.parametrize("gid", list(J.groups()))
def test_kernels_on_fixtures_by_geometry(gid):
    names = J.groups()[gid]
    pk = jpegdev.pack([J.data(n) for n in names])
    n = pk.n_frames
    dj = feeder.DeviceJpegs(pk, torch.device(DEV), n)
    dj.stream_through(pk.stream_np.size)
    (lo, hi, waves), = dj.chunks
    assert (lo, hi) == (0, n) and waves.shape[0] == len(pk.waves())
    fc = ops.jpeg_frame_coeffs(pk.width, pk.height, pk.samp)
    assert fc == pk.geom.frame_blocks * 64
    coeff = torch.zeros(n * fc, dtype=torch.int16, device=DEV)
    out = torch.full((n, 3, pk.height, pk.width), 0xA5, dtype=torch.uint8, device=DEV)
    ops.jpeg_entropy(dj.stream, dj.segments, waves, dj.table_sets, pk.width, pk.height, pk.samp, 0, n, coeff, dj.status)
    ops.jpeg_pixels(coeff, dj.frame_set, dj.table_sets, out, 0, n, pk.samp)
    torch.cuda.synchronize()
    assert not dj.status.cpu().numpy().any()
    got = coeff.cpu().numpy().reshape(n, fc)
    for j, nm in enumerate(names):
        assert np.array_equal(got[j], J.reference(nm).flat), nm
        assert torch.equal(out[j].cpu(), torch.from_numpy(J.expected()[nm])), nm


# ----------------------------------------------------------------------------- 2. more than one wavefront, chunks, odd width
@pytest.fixture(scope="module")
def video70(tmp_path_factory):
    base = tmp_path_factory.mktemp("v70")
    _write_video(str(base / "vid"), 70, 224, 224, 500, quality=90, subsampling=2)
    want = torch.stack([feeder.read_frame(str(base / "vid" / f"frame{i}.jpg")) for i in range(70)])
    return str(base), want


def test_seventy_frames_two_wavefronts_and_three_chunks(video70):
    base, want = video70
    got = feeder.load_video_device(base, "soccernetball", "vid", 70)
    stats = dict(feeder.last_decode_stats)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    assert (stats["frames"], stats["device_frames"], stats["fallback_frames"], stats["table_sets"], stats["segments"],
            stats["chunks"]) == (70, 70, 0, 1, 70, 1)
    assert 0 < stats["stream_bytes"] < want.numel() // 2                      # the files cross the link, not the frames
    pk = jpegdev.pack([open(os.path.join(base, "vid", f"frame{i}.jpg"), "rb").read() for i in range(70)])
    assert pk.waves().tolist() == [[0, 64], [64, 6]]
    fc = ops.jpeg_frame_coeffs(224, 224, jpegdev.S420)
    again = feeder.load_video_device(base, "soccernetball", "vid", 70, max_coeff_bytes=30 * fc * 2)
    assert feeder.last_decode_stats["chunks"] == 3
    assert torch.equal(again, got)
    buf = torch.full((72, 3, 224, 224), 9, dtype=torch.uint8, device=DEV)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()                                                   # buf is filled before the other stream writes it
    into = feeder.load_video_device(base, "soccernetball", "vid", 70, out=buf, stream=st, max_coeff_bytes=1)   # a frame per chunk
    assert feeder.last_decode_stats["chunks"] == 70 and into.data_ptr() == buf.data_ptr()
    assert torch.equal(into, got) and int(buf[70:].min()) == 9


def test_width_that_is_no_multiple_of_16(tmp_path):
    d = tmp_path / "wide"
    d.mkdir()
    for i, nm in enumerate(J.WIDE):
        shutil.copy(J.fixture_path(nm), str(d / f"frame{i}.jpg"))
    got = feeder.load_video_device(str(tmp_path), "soccernetball", "wide", 3)
    assert tuple(got.shape) == (3, 3, 224, 398)
    for i, nm in enumerate(J.WIDE):
        assert torch.equal(got[i].cpu(), torch.from_numpy(J.expected()[nm])), nm


# ----------------------------------------------------------------------------- 3. load_video_device against load_video
def _frame_dirs():
    g = np.load(os.path.join(ROOT, "tests", "golden", "frame_reader.npz"))
    meta = json.loads(str(g["meta"]))
    base = os.path.join(ROOT, "tests", "golden", "frames")
    return meta, [(ds, os.path.join(base, ds), v[0], meta["source_info"].get(ds)) for ds, v in meta["layouts"].items()]


def test_load_video_device_equals_load_video_on_the_dataset_layouts(tmp_path):
    meta, dirs = _frame_dirs()
    n = meta["n_frames"]
    assert n == 7 and sorted(d[0] for d in dirs) == ["finediving", "finegym", "soccernetball", "tennis"]
    for ds, fdir, vname, si in dirs:
        for stride in (1, 2):
            want = feeder.load_video(fdir, ds, vname, n, stride=stride, source_info=si)
            got = feeder.load_video_device(fdir, ds, vname, n, stride=stride, source_info=si)
            assert got.is_cuda and torch.equal(got.cpu(), want), (ds, stride)
            assert feeder.last_decode_stats["fallback_frames"] == 0 and feeder.last_decode_stats["device_frames"] == want.shape[0]
        want = feeder.load_video(fdir, ds, vname, n + 2, source_info=si)                       # trailing zero frames
        got = feeder.load_video_device(fdir, ds, vname, n + 2, source_info=si)
        assert got.shape[0] == n + 2 and torch.equal(got.cpu(), want) and not got[n:].any()
    d = tmp_path / "vid"
    d.mkdir()
    for i in (0, 1, 3, 4):
        shutil.copy(J.fixture_path("24x32_420_q90.jpg"), str(d / f"frame{i}.jpg"))
    with pytest.raises(FileNotFoundError, match="frame2.jpg"):
        feeder.load_video_device(str(tmp_path), "soccernetball", "vid", 5)
    assert feeder.load_video_device(str(tmp_path), "soccernetball", "vid", 2).shape[0] == 2
    with pytest.raises(FileNotFoundError):
        feeder.load_video_device(str(tmp_path), "soccernetball", "nothing_here", 2)


# ----------------------------------------------------------------------------- 4. frames the kernels do not decode
def test_unsupported_frames_take_the_pillow_route(tmp_path):
    d = tmp_path / "mixed"
    d.mkdir()
    files = ["24x32_420_q90.jpg", "24x32_progressive.jpg", "24x32_420_q30opt.jpg", "24x32_cmyk.jpg", "24x32_420_q75rst3.jpg",
             "24x32_420_q100.jpg"]
    for i, nm in enumerate(files):
        shutil.copy(J.fixture_path(nm), str(d / f"frame{i}.jpg"))
    want = feeder.load_video(str(tmp_path), "soccernetball", "mixed", 6)
    pool = feeder.DecodePool(2)
    try:
        got = feeder.load_video_device(str(tmp_path), "soccernetball", "mixed", 6, pool=pool)
    finally:
        pool.close()
    assert torch.equal(got.cpu(), want)
    s = feeder.last_decode_stats
    assert (s["frames"], s["device_frames"], s["fallback_frames"], s["table_sets"]) == (6, 4, 2, 4)
    only = tmp_path / "only"
    only.mkdir()
    shutil.copy(J.fixture_path("24x32_progressive.jpg"), str(only / "frame0.jpg"))
    got = feeder.load_video_device(str(tmp_path), "soccernetball", "only", 1)
    assert torch.equal(got.cpu(), feeder.load_video(str(tmp_path), "soccernetball", "only", 1))
    assert feeder.last_decode_stats["fallback_frames"] == 1 and feeder.last_decode_stats["chunks"] == 0


# ----------------------------------------------------------------------------- 5. through the consumers
TINY = dict(feature_arch="rny002_gsf", clip_len=8, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
            radi_displacement=2)


@pytest.fixture(scope="module")
def tiny_model():
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(TINY))
    m.load({k: t(v) for k, v in model_state(TINY, 0).items()})
    return m


def test_predict_video_from_device_decoded_frames(tiny_model, tmp_path):
    _write_video(str(tmp_path / "clip_a"), 21, 64, 64, 900, quality=85, subsampling=2)
    args = (str(tmp_path), "soccernetball", "clip_a", 21)
    host, dev = feeder.load_video(*args), feeder.load_video_device(*args)
    assert torch.equal(dev.cpu(), host)
    a = tiny_model.predict_video(host, batch_size=4, augment=True)
    b = tiny_model.predict_video(dev, batch_size=4, augment=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    src = dict(frame_dir=args[0], dataset=args[1], video_name=args[2], num_frames=21)
    st_h = E.stitch_videos(tiny_model, [("clip_a", 21, 25.0, src)], 4, augment=True, batch_size=4)
    st_d = E.stitch_videos(tiny_model, [("clip_a", 21, 25.0, src)], 4, augment=True, batch_size=4, decode="device")
    assert np.array_equal(st_h.tracks["clip_a"][0], a[0]) and np.array_equal(st_d.tracks["clip_a"][0], a[0])
    assert np.array_equal(st_d.tracks["clip_a"][1], st_h.tracks["clip_a"][1])


def test_resident_clips_from_device_decoded_videos(tmp_path):
    classes = {"dive": 1, "turn": 2, "land": 3}
    videos = [dict(video="va", num_frames=13, events=[dict(frame=2, label="dive"), dict(frame=9, label="land")]),
              dict(video="vb", num_frames=9, events=[dict(frame=4, label="turn")])]
    for i, v in enumerate(videos):
        _write_video(str(tmp_path / v["video"]), v["num_frames"], 24, 32, 700 + 50 * i, quality=90, subsampling=2)
    host = TC.load_resident_videos(str(tmp_path), "fs_comp", videos)
    dev = TC.load_resident_videos(str(tmp_path), "fs_comp", videos, decode="device")
    assert all(d.is_cuda and torch.equal(d.cpu(), h) for d, h in zip(dev, host))
    with pytest.raises(ValueError, match="decode"):
        TC.load_resident_videos(str(tmp_path), "fs_comp", videos, decode="gpu")
    kw = dict(clip_len=8, stride=1, overlap=1, mixup=False, dataset_len=6, batch_size=3, seed=5)
    batches = []
    for frames in (host, dev):
        loader = TC.ResidentClips(videos, frames, classes, radi_displacement=2, device=DEV, **kw)
        batches.append([{k: v.cpu() for k, v in b.items() if not k.startswith("_")} for b in feeder.prefetch(loader, DEV)])
    assert len(batches[0]) == len(batches[1]) == 2
    for a, b in zip(*batches):
        assert sorted(a) == sorted(b) and "frame" in a
        for k in a:
            assert torch.equal(a[k], b[k]), k
