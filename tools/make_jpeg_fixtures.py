"""Write tests/golden/jpeg/: the JPEG files the device-decoder tests run on, and expected.npz with Pillow's decode of
each (feeder.read_frame), which is what the decoder has to reproduce bit for bit.

    python tools/make_jpeg_fixtures.py

Everything is written by Pillow from a seeded synthetic image (smooth gradients plus noise, so that short and long
Huffman codes both occur):
  * seven sizes (H x W: 24x32, 23x37, 17x49, 40x56, 8x8, 1x1, 33x16) x three samplings (4:4:4, 4:2:2, 4:2:0) x four
    encodings (quality 90; quality 30 with optimised Huffman tables; quality 100; quality 75 with a restart interval of
    3 MCUs), and one greyscale file: 85 supported files;
  * one progressive and one CMYK file (24x32), which the decoder hands to Pillow;
  * three 224x398 (H x W) 4:2:0 files, a width that is no multiple of 16.
expected.npz also holds the decode of the 28 frames under tests/golden/frames/ (keys "frames/<relative path>").  It
depends on the Pillow / libjpeg-turbo build that wrote it; tests/test_jpegdev_host.py checks that the installed one
still agrees.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")

SIZES = [(24, 32), (23, 37), (17, 49), (40, 56), (8, 8), (1, 1), (33, 16)]
SAMPLINGS = {"444": 0, "422": 1, "420": 2}                       # Pillow's subsampling argument
ENCODINGS = {"q90": dict(quality=90), "q30opt": dict(quality=30, optimize=True), "q100": dict(quality=100),
             "q75rst3": dict(quality=75, restart_marker_blocks=3)}


def image(h, w, seed, noise=24):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([40 + 170 * xx / max(w - 1, 1), 30 + 190 * yy / max(h - 1, 1),
                     128 + 100 * np.sin(0.35 * xx + seed) * np.cos(0.27 * yy)], -1)
    return np.clip(base + rng.integers(-noise, noise + 1, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    from PIL import Image
    import tdeed_amd  # noqa: F401
    from tdeed_amd import feeder
    os.makedirs(OUT, exist_ok=True)
    names = []
    for si, (h, w) in enumerate(SIZES):
        im = Image.fromarray(image(h, w, 100 + si))
        for sname, sub in SAMPLINGS.items():
            for ename, kw in ENCODINGS.items():
                nm = f"{h}x{w}_{sname}_{ename}.jpg"
                im.save(os.path.join(OUT, nm), "JPEG", subsampling=sub, **kw)
                names.append(nm)
    im = Image.fromarray(image(24, 32, 100))
    im.convert("L").save(os.path.join(OUT, "24x32_grey_q90.jpg"), "JPEG", quality=90)
    im.save(os.path.join(OUT, "24x32_progressive.jpg"), "JPEG", quality=90, progressive=True, subsampling=2)
    im.convert("CMYK").save(os.path.join(OUT, "24x32_cmyk.jpg"), "JPEG", quality=90)
    names += ["24x32_grey_q90.jpg", "24x32_progressive.jpg", "24x32_cmyk.jpg"]
    for i in range(3):
        nm = f"224x398_420_q75_{i}.jpg"
        Image.fromarray(image(224, 398, 200 + i, noise=6)).save(os.path.join(OUT, nm), "JPEG", quality=75, subsampling=2)
        names.append(nm)
    expected = {nm: feeder.read_frame(os.path.join(OUT, nm)).numpy() for nm in names}
    frames = os.path.join(ROOT, "tests", "golden", "frames")          # the committed dataset-layout frames as well
    for d, _, files in sorted(os.walk(frames)):
        for fn in sorted(files):
            if fn.endswith(".jpg"):
                path = os.path.join(d, fn)
                expected["frames/" + os.path.relpath(path, frames).replace(os.sep, "/")] = feeder.read_frame(path).numpy()
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(names)} files, {total} bytes in {OUT}")


if __name__ == "__main__":
    main()
