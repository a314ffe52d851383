"""Streamed JPEG sets without a GPU: `trainclips.stream_plan` (which videos stay resident, the staging region, the budget) and
`trainclips.stage_batch` (the range copies and relocation rows of a batch) on a hand-made set, against a brute-force
restatement and a byte-level simulation of the device buffer; and tools/jpeg_stage_check.cpp -- every piece decoded from a
staged copy through csrc/jpeg_core.h's relocation predicate -- under the host sanitizers where the compiler has them."""
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import jpeg_cases as J
from tdeed_amd import jpegdev
from tdeed_amd import trainclips as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# three videos of 5, 4 and 256 frames in two shards: frames 0..6 and 7..264, so video 1 (frames 5..8) straddles the boundary.
# Every frame's bytes follow the previous frame's in its shard; frame 10 has none (kept decoded).  The last video is long
# against a clip, as real ones are: keeping it resident costs more than staging its clips.
LENGTHS = [5, 4, 256]
SIZES = [100, 60, 84, 120, 48, 200, 64, 96, 52, 180, 0, 72] + [120 + (i * 53) % 120 for i in range(253)]
SHARD = [0] * 7 + [1] * 258
FIXED = 1000
S1 = sum(SIZES[7:])                                     # bytes of shard 1


def _set():
    lo, hi, at = [], [], {0: 0, 1: 0}
    for f, (n, s) in enumerate(zip(SIZES, SHARD)):
        lo.append(at[s] if n else np.iinfo(np.int64).max)
        hi.append(at[s] + n if n else 0)
        at[s] += n
    ext = SimpleNamespace(shard=np.asarray(SHARD, np.int32), lo=np.asarray(lo, np.int64), hi=np.asarray(hi, np.int64),
                          shard_first=np.asarray([0, 7, 265], np.int64))
    videos = [dict(video=f"v{v}", num_frames=n, events=[]) for v, n in enumerate(LENGTHS)]
    return ext, videos, [at[0], at[1]]


def _rows(videos, clip_len, stride):
    table = TC.train_clip_table(videos, {}, clip_len, stride)
    offs = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    cv = table.clip_video.astype(np.int64)
    return np.stack([offs[cv], table.clip_base, np.asarray(LENGTHS, np.int64)[cv], cv])


def _r16(x):
    return (x + 15) // 16 * 16


def _clip_ranges_brute(ext, first, base, nfr, T, S):
    """[(shard, lo16, hi)] of one clip: every frame from its first existing frame to its last, per shard"""
    fs = [base + t * S for t in range(T) if 0 <= base + t * S < nfr]
    a, b = min(fs), max(fs)
    out = {}
    for g in range(first + a, first + b + 1):
        if ext.hi[g] > ext.lo[g]:
            s = int(ext.shard[g])
            lo, hi = out.get(s, (1 << 60, 0))
            out[s] = (min(lo, int(ext.lo[g])), max(hi, int(ext.hi[g])))
    return [(s, lo // 16 * 16, hi) for s, (lo, hi) in sorted(out.items())]


def _needs_brute(ext, rows, T, S, per_batch, depth):
    """-> (the budget that keeps v = 0 .. 3 videos resident: their streams, FIXED and depth regions for every clip of the set;
           the region when the videos v.. are streamed)"""
    firsts = np.concatenate([[0], np.cumsum(LENGTHS)])
    res, region = [], []
    for v in range(len(LENGTHS) + 1):
        F = int(firsts[v])
        res.append(sum(_r16(max([int(ext.hi[g]) for g in range(F) if ext.shard[g] == s], default=0)) for s in range(2)))
        clip = 0
        for first, base, nfr, vid in rows.T.tolist():
            if vid >= v:
                clip = max(clip, sum(_r16(hi) - lo for _, lo, hi in _clip_ranges_brute(ext, first, base, nfr, T, S)))
        region.append(per_batch * clip)
    return [r + FIXED + depth * region[0] for r in res], region


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("operands", [1, 2], ids=["plain", "mixup"])
def test_stream_plan_chooses_the_longest_resident_prefix_that_fits(stride, operands):
    ext, videos, _ = _set()
    T, B, depth = 4, 3, 2
    rows = _rows(videos, T, stride)
    assert rows[1].min() < 0 and rows.shape[1] > 10                       # clips with padding in front
    vf, vl = [0, 5, 9], LENGTHS
    plan = TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, 1 << 40)
    want, region = _needs_brute(ext, rows, T, stride, operands * B, depth)
    assert plan.needs.tolist() == want == sorted(want) and region[3] == 0 < region[2] <= region[1] <= region[0]
    # ample: everything resident, no staging, the resident bytes of today's convention
    assert (plan.resident_videos, plan.region_bytes, plan.stage_lo) == (3, 0, _r16(676) + _r16(S1))
    assert plan.resident_bytes == plan.buffer_bytes + FIXED == _r16(676) + _r16(S1) + FIXED
    assert plan.shard_base.tolist() == [0, _r16(676)] and plan.shard_bytes.tolist() == [_r16(676), _r16(S1)]
    for v in range(4):
        p = TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, want[v])
        assert p.resident_videos == v and p.region_bytes == region[v]
        assert p.resident_bytes == want[v] - depth * (region[0] - region[v]) <= want[v]
        assert p.resident_frames == [0, 5, 9, 265][v] and p.region_bytes % 16 == 0 and p.stage_lo == p.stream_bytes
        if v < 3:
            assert TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, want[v + 1] - 1).resident_videos == v
        assert p.buffer_bytes == p.stream_bytes + depth * p.region_bytes and p.stream_bytes == int(p.shard_bytes.sum())
        assert all(int(b) % 16 == 0 for b in p.shard_base) and p.min_budget == want[0]
    # video 1 resident means shard 1 is resident up to frame 8 only
    p = TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, want[2])
    assert p.resident_videos == 2 and p.shard_bytes.tolist() == [_r16(676), _r16(96 + 52)] and p.shard_base.tolist() == [0, _r16(676)]
    p = TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, want[0])
    assert p.resident_videos == 0 and p.shard_bytes.tolist() == [0, 0] and p.stream_bytes == 0
    assert p.shard_base.tolist() == [p.buffer_bytes, p.buffer_bytes + _r16(676)]      # behind the buffer, 64-bit positions
    # one byte short of the smallest sufficient budget: the message names it, and that budget does
    with pytest.raises(ValueError, match=f"smallest max_resident_bytes that would do is {want[0]}$"):
        TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, want[0] - 1)
    assert TC.stream_plan(ext, vf, vl, rows, T, stride, operands, B, depth, FIXED, want[0]).resident_bytes == want[0]
    with pytest.raises(ValueError, match="tile"):
        TC.stream_plan(ext, [0, 5, 8], vl, rows, T, stride, operands, B, depth, FIXED, 1 << 40)


def test_a_straddling_clip_and_a_stride_two_clip_by_hand():
    """clip_len 4 over video 1 (frames 5..8, set-wide): base 1 at stride 1 shows frames 6, 7, 8 and padding -- frame 6 ends
    shard 0 (bytes 612..676), frames 7 and 8 start shard 1 (0..148): two ranges.  base 0 at stride 2 shows frames 5 and 7 and
    copies frame 6 between them too."""
    ext, videos, _ = _set()
    plan = SimpleNamespace(resident_videos=1, stream_bytes=416, region_bytes=4096, shard_base=np.asarray([0, 1 << 34], np.int64))
    rows = np.asarray([[5], [1], [4], [1]], np.int64)
    copies, reloc = TC.stage_batch(plan, ext, rows, 4, 1, 1024)
    assert copies == [(0, 608, 676, 1024), (1, 0, 148, 1024 + 80)]
    assert reloc.tolist() == [[608 - 1024, 1024, 1024 + 68], [(1 << 34) - 1104, 1104, 1104 + 148]] * 1 + \
        [[(1 << 34) - 1104, 1104, 1104 + 148], [0, 0, 416]]
    rows = np.asarray([[5], [0], [4], [1]], np.int64)
    copies, reloc = TC.stage_batch(plan, ext, rows, 4, 2, 2048)
    assert copies == [(0, 400, 676, 2048), (1, 0, 96, 2048 + 288)]
    assert reloc.tolist() == [[400 - 2048, 2048, 2048 + 276], [(1 << 34) - 2336, 2336, 2336 + 96], [0, 0, 416], [0, 0, 416]]
    # a clip of the resident video: nothing to copy
    copies, reloc = TC.stage_batch(plan, ext, np.asarray([[0], [-2], [5], [0]], np.int64), 4, 1, 1024)
    assert copies == [] and reloc.tolist() == [[0, 0, 416]] * 4
    with pytest.raises(ValueError, match="staging"):
        TC.stage_batch(SimpleNamespace(**dict(vars(plan), region_bytes=200)), ext, rows, 4, 2, 2048)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("resident", [0, 1, 2])
def test_staged_batches_put_every_frames_bytes_where_its_slot_looks(stride, resident):
    """The device buffer simulated in numpy: the resident bytes uploaded as the plan says, every batch's copies made, and every
    slot that shows a frame with bytes finds exactly those bytes at pos - delta, inside its window; mixup batches of every
    clip of the set, two ring entries."""
    ext, videos, shard_size = _set()
    T, B, depth, nops = 4, 3, 2, 2
    rows = _rows(videos, T, stride)
    want, _ = _needs_brute(ext, rows, T, stride, nops * B, depth)
    plan = TC.stream_plan(ext, [0, 5, 9], LENGTHS, rows, T, stride, nops, B, depth, FIXED, want[resident])
    assert plan.resident_videos == resident
    rs = np.random.RandomState(7)
    host = [rs.randint(1, 255, n).astype(np.uint8) for n in shard_size]
    dev = np.zeros(plan.buffer_bytes, np.uint8)
    for k in range(2):
        n = min(int(plan.shard_bytes[k]), shard_size[k])
        dev[plan.shard_base[k]:plan.shard_base[k] + n] = host[k][:n]
    n_clips = rows.shape[1]
    order = rs.permutation(n_clips)
    seen = 0
    for i, lo in enumerate(range(0, n_clips - 2 * B + 1, 2 * B)):
        ids = order[lo:lo + 2 * B]
        at = np.concatenate([np.arange(B), B + np.arange(B)]) * T
        region = plan.stage_lo + (i % depth) * plan.region_bytes
        copies, reloc = TC.stage_batch(plan, ext, rows[:, ids], T, stride, region, n_slots=nops * B * T, clip_slot=at)
        dev[region:region + plan.region_bytes] = 0                         # whatever the last batch left must not be needed
        for k, b_lo, b_hi, d in copies:
            assert b_lo % 16 == 0 and d % 16 == 0 and region <= d and d + b_hi - b_lo <= region + plan.region_bytes
            dev[d:d + b_hi - b_lo] = host[k][b_lo:b_hi]
        assert reloc.shape == (nops * B * T, 3) and not np.any(reloc[:, 0] % 16)
        assert len(copies) == len({(c[0], c[3]) for c in copies})
        for c, (first, base, nfr, vid) in enumerate(rows[:, ids].T.tolist()):
            for t in range(T):
                f = base + t * stride
                delta, w_lo, w_hi = reloc[at[c] + t].tolist()
                if not 0 <= f < nfr or ext.hi[first + f] <= ext.lo[first + f] or vid < plan.resident_videos:
                    assert (delta, w_lo, w_hi) == (0, 0, plan.stream_bytes)
                    if not 0 <= f < nfr or ext.hi[first + f] <= ext.lo[first + f]:
                        continue
                g = first + f
                s = int(ext.shard[g])
                pos = int(plan.shard_base[s]) + int(ext.lo[g])
                n = int(ext.hi[g] - ext.lo[g])
                assert 0 <= w_lo <= pos - delta and pos - delta + n <= w_hi <= dev.size
                assert np.array_equal(dev[pos - delta:pos - delta + n], host[s][ext.lo[g]:ext.hi[g]]), (ids, c, t)
                seen += 1
    assert seen > 200


def test_frame_extents_of_a_packed_set():
    names = ["24x32_420_q90.jpg", "24x32_420_q100.jpg", "24x32_cmyk.jpg", "24x32_420_q75rst3.jpg", "24x32_420_q30opt.jpg"]
    datas = [J.data(n) for n in names]
    shards = [SimpleNamespace(packed=jpegdev.pack_frames(datas[:3], pinned=False), frames=np.arange(0, 3)),
              SimpleNamespace(packed=jpegdev.pack_frames(datas[3:], pinned=False), frames=np.arange(3, 5))]
    ext = TC.frame_extents(shards)
    assert ext.shard.tolist() == [0, 0, 0, 1, 1] and ext.shard_first.tolist() == [0, 3, 5]
    assert ext.hi[2] <= ext.lo[2]                                          # the CMYK file has no segments
    for f in (0, 1, 3, 4):
        s = shards[ext.shard[f]]
        seg = s.packed.segments[s.frames[s.packed.segments[:, 0]] == f]
        assert ext.lo[f] == seg[:, 3].min() and ext.hi[f] >= (seg[:, 3] + seg[:, 4]).max() + jpegdev.GUARD
        assert ext.hi[f] <= s.packed.stream_np.size and ext.hi[f] % 4 == 0
    assert len(shards[1].packed.segments[shards[1].packed.segments[:, 0] == 0]) == 2      # the restart file: two segments, one extent
    assert max(ext.hi[:3]) == shards[0].packed.stream_np.size and max(ext.hi[3:]) == shards[1].packed.stream_np.size
    with pytest.raises(ValueError, match="consecutive"):
        TC.frame_extents(shards[::-1])


# ----------------------------------------------------------------------------- the stand-alone program
@pytest.fixture(scope="module")
def stage_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    tmp = tmp_path_factory.mktemp("jpeg_stage_check")
    exe, src = str(tmp / "jpeg_stage_check"), os.path.join(ROOT, "tools", "jpeg_stage_check.cpp")
    # with the address and undefined-behaviour sanitizers where the compiler has them (a stand-alone host program: a report
    # ends it with a non-zero status), plain otherwise
    san = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src]
    r = subprocess.run(san, capture_output=True)
    if r.returncode != 0 or subprocess.run([exe], capture_output=True).returncode != 2:     # no arguments: the usage line
        subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe


@pytest.mark.parametrize("gid", ["24x32_420", "23x37_422", "17x49_444", "24x32_grey", "40x56_420"])
def test_stage_check_program_decodes_every_piece_from_its_staged_copy(stage_check, tmp_path, gid):
    """tools/jpeg_stage_check.cpp: ranges copied into exact-size heap blocks at a shifted offset, every piece decoded through
    jc_piece_reloc_ok from its block equals the whole-stream decode, every row that leaves its window is rejected"""
    pk = jpegdev.pack_frames([J.data(n) for n in J.groups()[gid]], pinned=False)
    src = str(tmp_path / "packed.bin")
    pk.save(src)
    for split, n_ranges, shift in ((1, 1, 0), (0, 2, 48), (1, 3, 4096), (2, pk.n_segments, 16)):
        r = subprocess.run([stage_check, src, str(split), str(n_ranges), str(shift)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (split, n_ranges, shift, r.stdout, r.stderr)
        got = dict(zip(r.stdout.split()[::2], map(int, r.stdout.split()[1::2])))
        n_pieces = int(jpegdev.piece_counts(pk.segments, split or pk.geom.mcus_x).sum())
        assert got["pieces"] == got["decoded"] == got["accepted_tight"] == n_pieces and got["ranges"] == min(n_ranges, pk.n_segments)
        assert got["rejected"] >= 11 * n_pieces
    r = subprocess.run([stage_check, src, "1", "2", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "multiple of 16" in r.stderr
