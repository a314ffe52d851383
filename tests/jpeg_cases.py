"""Shared by the JPEG decoder tests: the files of tests/golden/jpeg/ (tools/make_jpeg_fixtures.py), Pillow's recorded
decode of each, the numpy model's decode (computed once per process), and the files grouped as one packed call takes
them."""
import functools
import os

import numpy as np

from helpers import ROOT

JPEG_DIR = os.path.join(ROOT, "tests", "golden", "jpeg")
FRAMES_DIR = os.path.join(ROOT, "tests", "golden", "frames")
SIZES = [(24, 32), (23, 37), (17, 49), (40, 56), (8, 8), (1, 1), (33, 16)]
SAMPLINGS = ["444", "422", "420"]
ENCODINGS = ["q90", "q30opt", "q100", "q75rst3"]
UNSUPPORTED = ["24x32_progressive.jpg", "24x32_cmyk.jpg"]
WIDE = [f"224x398_420_q75_{i}.jpg" for i in range(3)]
GREY = "24x32_grey_q90.jpg"


@functools.lru_cache(maxsize=None)
def expected():
    with np.load(os.path.join(JPEG_DIR, "expected.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_path(name):
    return os.path.join(FRAMES_DIR, name[len("frames/"):]) if name.startswith("frames/") else os.path.join(JPEG_DIR, name)


@functools.lru_cache(maxsize=None)
def data(name):
    with open(fixture_path(name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def reference(name):
    """jpegdev.decode_reference of a fixture, once per process; nobody writes to it"""
    from tdeed_amd import jpegdev
    return jpegdev.decode_reference(data(name))


def supported_names():
    return [k for k in expected() if k not in UNSUPPORTED]


def groups():
    """{id: [file names]}: per size and sampling the four encodings (several table sets, and a restart file with many
    segments, in one packed call), the greyscale file, and the three wide files"""
    g = {f"{h}x{w}_{s}": [f"{h}x{w}_{s}_{e}.jpg" for e in ENCODINGS] for h, w in SIZES for s in SAMPLINGS}
    g["24x32_grey"] = [GREY]
    g["224x398_420"] = list(WIDE)
    return g


def read_host_check_output(path, packed):
    """(coefficients int16 (frames, frame values), status int32 (segments,), rgb uint8 (frames,3,H,W)) of
    tools/jpeg_host_check.cpp"""
    fc, nf, ns = packed.geom.frame_blocks * 64, packed.n_frames, packed.n_segments
    raw = open(path, "rb").read()
    assert len(raw) == 2 * fc * nf + 4 * ns + nf * 3 * packed.height * packed.width
    coef = np.frombuffer(raw, np.int16, fc * nf).reshape(nf, fc)
    status = np.frombuffer(raw, np.int32, ns, offset=2 * fc * nf)
    rgb = np.frombuffer(raw, np.uint8, offset=2 * fc * nf + 4 * ns).reshape(nf, 3, packed.height, packed.width)
    return coef, status, rgb
