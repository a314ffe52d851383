"""What the joint-loader tests share: the parts of tests/golden/train_clips_joint.npz (two label lists, two class lists, the
decoded frames of every video, recorded from the reference's own ActionSpotDatasetJoint), joint batches assembled on the
host from `trainclips`' tables and draws by plain indexing, and two small Pillow-written JPEG trees."""
import os

import numpy as np
import torch

from helpers import load_golden
from tdeed_amd import trainclips as TC

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = load_golden("train_clips_joint")
    return _CACHE["g"]


def parts_of(case, frames=True):
    """the `parts` argument of `JointResidentClips` for one fixture case"""
    meta, g = golden()
    out = []
    for k, p in enumerate(meta["parts"]):
        part = dict(videos=p["videos"], classes=p["classes"], stride=case["strides"][k], overlap=case["overlaps"][k],
                    dataset_len=case["dataset_len"][k])
        if frames:
            part["frames"] = [torch.from_numpy(np.ascontiguousarray(g[f"video__p{k}__{vi}"])) for vi in range(len(p["videos"]))]
        out.append(part)
    return out


def joined_table(parts, clip_len, radius=0, pad_len=TC.DEFAULT_PAD_LEN):
    tables = [TC.train_clip_table(p["videos"], p["classes"], clip_len, p["stride"], p["overlap"], pad_len,
                                  p.get("require_events", False), radius) for p in parts]
    return tables, TC.join_clip_tables(tables)


def gather(frames, table, ids, strides, clip_len):
    """clips by plain indexing: frames -- one tensor per video of the joined table --, zeros outside the clip's video"""
    out = torch.zeros((len(ids), clip_len) + tuple(frames[0].shape[1:]), dtype=torch.uint8)
    for k, c in enumerate(ids):
        v, base = int(table.clip_video[c]), int(table.clip_base[c])
        for t in range(clip_len):
            f = base + t * int(strides[k])
            if 0 <= f < frames[v].shape[0]:
                out[k, t] = frames[v][f]
    return out


def host_batches(parts, clip_len, radius, mixup, batch_size, seed, passes=1, drop_last=False):
    """What the reference's DataLoader over ActionSpotDatasetJoint would hand to epoch(): table, draws and label rule on
    the host, the clips by plain indexing.  parts carry `frames`."""
    tables, tab = joined_table(parts, clip_len, radius)
    frames = [f for p in parts for f in p["frames"]]
    per_clip = np.repeat([p["stride"] for p in parts], np.diff(tab.part_clips))
    draws = TC.JointDraws(np.diff(tab.part_clips), [p["dataset_len"] for p in parts], batch_size, mixup, seed, drop_last)
    batches = []
    for _ in range(passes):
        for part, ia, ib in draws:
            lo = tab.part_clips[part - 1]
            S = per_clip[lo + ia]
            lab, labD = TC.rasterise_labels(tab, lo + ia, clip_len, S, radius)
            b = dict(frame=gather(frames, tab, lo + ia, S, clip_len), label=torch.from_numpy(lab), dataset=torch.from_numpy(part))
            if radius > 0:
                b["labelD"] = torch.from_numpy(labD)
            if mixup:
                lab2, labD2 = TC.rasterise_labels(tab, lo + ib, clip_len, S, radius)
                b.update(frame2=gather(frames, tab, lo + ib, S, clip_len), label2=torch.from_numpy(lab2))
                if radius > 0:
                    b["labelD2"] = torch.from_numpy(labD2)
            batches.append(b)
    return batches


CLASSES = ({"dive": 1, "turn": 2}, {"jump": 1, "spin": 2, "step": 3, "fall": 4})


def write_trees(root, subsampling2=2, h=24, w=32):
    """Two parts written by Pillow at h x w: part 1 (two videos) at quality 90, 4:2:0; part 2 (two videos) at quality 30 with
    optimize=True -- other quantisation AND other Huffman tables -- and the given subsampling (2: 4:2:0, 0: 4:4:4).
    -> [(directory, videos)] per part"""
    from PIL import Image
    from tdeed_amd import synth
    ev = lambda *pairs: [dict(frame=f, label=l) for f, l in pairs]     # noqa: E731
    spec = [("p1", dict(quality=90, subsampling=2), [("a0", 9, ev((1, "dive"), (7, "turn"))), ("a1", 5, ev((0, "turn"), (4, "dive")))]),
            ("p2", dict(quality=30, optimize=True, subsampling=subsampling2),
             [("b0", 4, ev((2, "fall"))), ("b1", 11, ev((0, "jump"), (5, "step"), (6, "spin"), (10, "fall")))])]
    out = []
    for k, (sub, kw, vids) in enumerate(spec):
        d = os.path.join(root, sub)
        videos = []
        for vi, (name, n, events) in enumerate(vids):
            os.makedirs(os.path.join(d, name))
            # smooth content with some noise: frames that differ, and chroma that the two samplings treat differently
            for i in range(n):
                yy, xx = np.mgrid[0:h, 0:w]
                base = np.stack([(xx * 7 + i * 9 + 40 * k) % 256, (yy * 9 + 13 * vi + 3 * i) % 256, ((xx + yy) * 5 + 70 * k) % 256], -1)
                px = (base.astype(np.int64) + synth.uint8_clip(300 + 100 * k + 10 * vi + i, (h, w, 3)) // 8).clip(0, 255)
                Image.fromarray(px.astype(np.uint8)).save(os.path.join(d, name, f"frame{i}.jpg"), **kw)
            videos.append(dict(video=name, num_frames=n, events=events))
        out.append((d, videos))
    return out
