"""The validation pass sharded over ranks on the MI355X: the exchange of the AP state (`ops.ap_state_counts` / `ap_state_pack`
/ `ap_state_unpack`) with the ranks played in one process, bit for bit against the one-rank pass; the frame counters
(`ops.frame_stats_seg`) against `evalutil.frame_events(labels=...)`; `evalutil.map_videos(labels=..., shard=...)` end to end, in
one process and as two processes that share the GPU over gloo.  -m gpu only."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import t, load_golden
from tdeed_amd import evalutil as E
from tdeed_amd import ops, synth
import test_spot_host as H
import test_ap_host as A
import test_gpu_map as G
import test_map_shard_host as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLITS = ([[0], [1, 2]], [[2, 0], [1]], [[], [0, 1, 2]], [[0], [1], [2]])


# ----------------------------------------------------------------------------- the ranks played in one process
def fill(state, tracks, ords, idx, entries, hr=0.01):
    """G.device_route's launches for the tracks idx (one group, in that order), without the rank launch"""
    lens = [tracks[i].shape[0] for i in idx]
    mean = torch.from_numpy(np.concatenate([tracks[i] for i in idx])).to(DEV)
    seg_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)
    od = torch.tensor([ords[i] for i in idx], dtype=torch.int32, device=DEV)
    first = ops.frame_events_seg(mean, seg_off, max(lens), hr)[2]
    for e, entry in enumerate(entries):
        planes = None
        if entry[0] != "raw":
            planes = ops.nms_track_seg(mean, seg_off, max(lens), entry[1], entry[2], entry[0] == "snms", first, hr, planes=True)[5:]
        ops.ap_match_seg(state, e, mean, seg_off, od, max(lens), hr, planes=planes)


def stores_of(state):
    return dict(ev_score=state.ev_score.cpu().numpy(), ev_count=state.ev_count.cpu().numpy(), hit_pos=state.hit_pos.cpu().numpy(),
                hit_count=state.hit_count.cpu().numpy(), vid_off=state.vid_off_host.astype(np.int64),
                gt_off=state.gt_off.cpu().numpy().astype(np.int64), ev_frame=state.ev_frame.cpu().numpy())


def exchange_bytes_formula(E_, T, K1, NV, S_, Hh, counters=True):
    return 4 * E_ * (K1 - 1) * NV + 4 * E_ * T * NV * K1 + 4 * NV + (8 * (2 + 3 * K1) if counters else 0) + 8 * S_ + 4 * Hh


def simulated_ranks(tracks, ords, truth, tols, entries, split, hr=0.01):
    """every rank of `split` (lists of ordinals) fills a state of its own with its share; the sums a collective would take are
    taken here.  -> (states, [(ap, nhits, rank) per rank], bytes that went through the sums)"""
    K1, nv = tracks[0].shape[1], len(tracks)
    by_ord = {o: i for i, o in enumerate(ords)}
    lens = [tracks[by_ord[o]].shape[0] for o in range(nv)]
    states = []
    for own in split:
        st = ops.ap_state(lens, truth, K1, len(entries), tols, DEV)
        st.ev_score.fill_(float("nan"))                                   # whatever the exchange leaves alone stays visible
        st.ev_frame.fill_(-5)
        st.hit_pos.fill_(-7)
        if own:
            fill(st, tracks, ords, [by_ord[o] for o in own], entries, hr)
        states.append(st)
    counts = [ops.ap_state_counts(st, own) for st, own in zip(states, split)]
    assert all(c[0] is st.ev_count and c[1] is st.hit_count for c, st in zip(counts, states))
    sums = [sum(c[j] for c in counts) for j in range(3)]
    nbytes = sum(x.numel() * x.element_size() for x in sums)
    for c in counts:
        for j in range(3):
            c[j].copy_(sums[j])
    pays = [ops.ap_state_pack(st, own, owners=c[2]) for st, own, c in zip(states, split, counts)]
    for (sc, hp), own in zip(pays, split):
        assert sc.dtype == torch.float64 and hp.dtype == torch.int32
        if not own:
            assert not sc.any() and not hp.any()                          # a rank without videos sends zeros
    written = sum((p[0] != 0).to(torch.int32) for p in pays)
    assert int(written.max()) <= 1 if written.numel() else True           # one writer per element
    scores, hits = sum(p[0] for p in pays), sum(p[1] for p in pays)
    nbytes += scores.numel() * 8 + hits.numel() * 4
    out = []
    for st, own in zip(states, split):
        ops.ap_state_unpack(st, own, scores, hits)
        ap, nhits, rank = ops.ap_rank(st)
        out.append((ap.cpu().numpy(), nhits.cpu().numpy(), rank.cpu().numpy()))
    torch.cuda.synchronize()
    return states, out, nbytes


def check_merged(states, results, nbytes, split, one, K1):
    """one: G.device_route's (state, ap, nhits, rank) of the one-rank pass"""
    ref = stores_of(one[0])
    want_used = S.used_parts(ref, K1)
    S_, Hh = int(ref["ev_count"].sum()), int(ref["hit_count"].sum())
    st0 = one[0]
    assert nbytes == exchange_bytes_formula(st0.E, st0.T, K1, st0.NV, S_, Hh, counters=False)
    for st, got, own in zip(states, results, split):
        for a, b in zip(got, one[1:]):
            assert np.array_equal(a, b), (split, own)                     # ap, nhits, rank: identical bits
        s = stores_of(st)
        assert np.array_equal(s["ev_count"], ref["ev_count"]) and np.array_equal(s["hit_count"], ref["hit_count"])
        assert S.used_parts(s, K1) == want_used, (split, own)
        vo, go = s["vid_off"], s["gt_off"]
        for o in range(st.NV):
            if o not in own:                                              # ev_frame of foreign videos is left as it was
                assert (s["ev_frame"][:, :, vo[o]:vo[o + 1]] == -5).all(), (split, own, o)
            for e in range(st.E):
                for c in range(K1 - 1):                                   # nothing beyond a segment's count was written
                    assert np.isnan(s["ev_score"][e, c, vo[o] + s["ev_count"][e, c, o]:vo[o + 1]]).all(), (split, own, o, e, c)
                for ti in range(st.T):
                    for oc in range(o * K1, (o + 1) * K1):
                        assert (s["hit_pos"][e, ti, go[oc] + s["hit_count"][e, ti, oc]:go[oc + 1]] == -7).all()


@pytest.mark.parametrize("K1", [2, 5])
@pytest.mark.parametrize("L", [1, 64, 65, 1025])
def test_simulated_ranks_equal_the_one_rank_pass(L, K1):
    """segments of 0, 1, exactly a wave, a wave plus one and more than a workgroup; "sixths": ties within and across videos"""
    n_hits = 0
    for variant in ("uniform", "sixths"):
        tracks, ords, truth, tols, _ = G.grid_case(L, K1, 3, variant)
        one = G.device_route(tracks, ords, G.ENTRIES, tols, truth)
        n_hits += int(one[2].sum())
        for split in SPLITS:
            states, results, nbytes = simulated_ranks(tracks, ords, truth, tols, G.ENTRIES, split)
            check_merged(states, results, nbytes, split, one, K1)
    assert n_hits > 0


def test_ownership_is_checked_before_any_payload_is_built():
    tracks, ords, truth, tols, _ = G.grid_case(64, 2, 3, "uniform")
    lens = [tracks[{o: i for i, o in enumerate(ords)}[o]].shape[0] for o in range(3)]
    st = ops.ap_state(lens, truth, 2, 1, tols, DEV)
    owners = torch.tensor([1, 2, 0], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"twice \[1\], never \[2\]"):
        ops.ap_state_pack(st, [0, 1], owners=owners)
    with pytest.raises(ValueError):
        ops.ap_state_counts(st, [0, 0])
    with pytest.raises(ValueError):
        ops.ap_state_counts(st, [3])
    with pytest.raises(ValueError):
        ops.ap_state_unpack(st, [0], torch.zeros(3, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))       # float32 scores


def test_the_reference_goldens_through_a_two_way_split():
    meta, g = load_golden("eval_utils")
    videos, classes, norm, _ = H.golden_inputs(meta)
    names = sorted(v for v, _, _ in videos)
    tracks = [np.ascontiguousarray(norm[v]) for v in names]
    ords = list(range(len(names)))
    table = E.truth_table(A.golden_truth(meta, videos), {v: i for i, v in enumerate(names)}, classes)
    labelled = sorted({c for _, c in table})
    split = E.shard_videos([tr.shape[0] for tr in tracks], 2)
    assert all(split)
    for entry, tols, key in ((("raw",), [0, 1, 2, 4], "maps_hr"), (("nms", 2, 0.10), [1, 2, 4], "maps_nms")):
        _, results, _ = simulated_ranks(tracks, ords, table, tols, [entry], split, hr=meta["hr_thr"])
        for ap, _, _ in results:
            maps = [float(np.mean([ap[0, ti, c] for c in labelled])) for ti in range(len(tols))]
            assert np.allclose(maps, g[key], atol=1e-12), (key, maps, g[key])


# ----------------------------------------------------------------------------- frame counters
def label_patterns(tracks):
    """all background; all foreground; the LAST maximum of every row -- where the top scores of a frame tie, the label names a
    maximum that np.argmax does not pick, so the frame is an error only if the first maximum wins"""
    K1 = tracks[0].shape[1]
    yield "background", [np.zeros(m.shape[0], np.int64) for m in tracks]
    yield "foreground", [1 + (np.arange(m.shape[0]) + v) % (K1 - 1) for v, m in enumerate(tracks)]
    yield "last_maximum", [K1 - 1 - m[:, ::-1].argmax(axis=1) for m in tracks]


def device_counters(tracks, labels, stats=None):
    mean = torch.from_numpy(np.concatenate(tracks)).to(DEV)
    lab = torch.from_numpy(np.concatenate(labels).astype(np.uint8)).to(DEV)
    return ops.frame_stats_seg(mean, lab, stats)


def host_stats(tracks, labels):
    K1 = tracks[0].shape[1]
    classes = {f"c{k}": k for k in range(1, K1)}
    names = [f"v{i}" for i in range(len(tracks))]
    return E.frame_events(dict(zip(names, tracks)), classes, {v: 25.0 for v in names}, labels=dict(zip(names, labels)))[2], classes


@pytest.mark.parametrize("K1", [2, 5])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 1025])
def test_frame_stats_equal_frame_events_integers(L, K1):
    lens = [L, L // 2 + 2, 2 * L + 1]                                     # three videos of unequal length
    ties = 0
    for variant in ("uniform", "sixths"):
        tracks = [H.make_track(n, K1, variant, 97 * L + 5 * K1 + v) for v, n in enumerate(lens)]
        for tag, labels in label_patterns(tracks):
            got = device_counters(tracks, labels).cpu().numpy()
            assert got.dtype == np.int64 and got.shape == (2 + 3 * K1,)
            assert np.array_equal(got, sum(E.frame_stats_ref(m, lab) for m, lab in zip(tracks, labels))), (variant, tag)
            want, classes = host_stats(tracks, labels)
            assert got[0] == sum(lens) and E.frame_stats_dict(got, classes) == want, (variant, tag)
            if tag == "last_maximum":
                ties += int(got[1])                                       # errors of this pattern are exactly the tied frames
                assert got[1] == sum(int((lab != m.argmax(axis=1)).sum()) for m, lab in zip(tracks, labels))
    if L >= 63:
        assert ties > 0


def test_frame_stats_accumulate_and_stride():
    """two launches into one tensor add up; a track longer than one sweep of the bounded grid (256 workgroups of 256 frames)"""
    K1 = 5
    tracks = [H.make_track(n, K1, "sixths", 11 + v) for v, n in enumerate((40, 7, 90))]
    labels = [np.arange(m.shape[0]) % K1 for m in tracks]
    stats = device_counters(tracks, labels)
    once = stats.cpu().numpy().copy()
    assert device_counters(tracks[:2], labels[:2], stats) is stats
    assert np.array_equal(stats.cpu().numpy(), once + sum(E.frame_stats_ref(m, lab) for m, lab in zip(tracks[:2], labels[:2])))
    n = 256 * 256 + 77
    long_track = H.make_track(n, 3, "uniform", 5)
    lab = (np.arange(n) * 7 % 3).astype(np.int64)
    assert np.array_equal(device_counters([long_track], [lab]).cpu().numpy(), E.frame_stats_ref(long_track, lab))
    with pytest.raises(ValueError):
        ops.frame_stats_seg(torch.zeros((4, 3), device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.frame_stats_seg(torch.zeros((4, 3), device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV),
                            torch.zeros(11, dtype=torch.int32, device=DEV))


def test_frame_stats_on_the_golden_tracks_equal_the_recorded_counters():
    meta, g = load_golden("eval_utils")
    videos, classes, norm, _ = H.golden_inputs(meta)
    labels = S.golden_labels(meta, videos)
    names = [v for v, _, _ in videos]
    got = device_counters([np.ascontiguousarray(norm[v]) for v in names], [labels[v] for v in names]).cpu().numpy()
    assert np.array_equal(got[2:].reshape(meta["K1"], 3), g["tpfpfn"])
    assert abs(E.frame_stats_dict(got, classes)["err"] - float(g["err"])) < 1e-12


# ----------------------------------------------------------------------------- end to end, tiny model
LENS = {"b": 37, "a": 23, "c": 30}
SUPPRESS = (("raw",), ("nms", 1, 0.01), ("snms", [3, 1, 2], 0.01))
TOLS = [0, 1, 2, 4]
KW = dict(augment=True, batch_size=4, group_videos=2)


def tiny_inputs():
    frames = {v: t(synth.uint8_clip(4100 + 100 * i, (n, 3, 64, 64))) for i, (v, n) in enumerate(LENS.items())}
    truth = [{"video": v, "events": [{"label": "c1", "frame": 3}, {"label": "c2", "frame": 10}, {"label": "c2", "frame": 10},
                                     {"label": "c3", "frame": 17}, {"label": "c1", "frame": n - 1}]} for v, n in LENS.items()]
    labels = {v: (np.arange(n) * (3 + i) // 5) % 4 for i, (v, n) in enumerate(LENS.items())}
    return frames, truth, labels


def test_map_videos_with_labels_and_a_one_rank_shard():
    from test_gpu_spot import TINY, CLASSES, _model
    m = _model(TINY)
    frames, truth, labels = tiny_inputs()
    vids = [("b", 37, 25.0, frames["b"]), ("a", 23, 30.0, lambda: frames["a"]), ("c", 30, 25.0, frames["c"])]
    plain = E.map_videos(m, vids, CLASSES, truth, SUPPRESS, TOLS, **KW)
    plain_stats = dict(m.last_video_stats)
    got, stats = E.map_videos(m, vids, CLASSES, truth, SUPPRESS, TOLS, labels=labels, shard=(0, 1), **KW)
    run = dict(m.last_video_stats)
    assert got == plain                                                   # every float identical
    st = E.stitch_videos(m, vids, 4, **KW)
    want = E.frame_events(st.normalised(), CLASSES, st.fps, high_recall_score_threshold=0.01, labels=labels)[2]
    assert stats == want and want["tp_fp_fn"][None] != (0, 0, 0)
    preds = E.spot_videos(m, vids, CLASSES, SUPPRESS[1:], **KW)[2]        # the pred the host route counts from
    counters = sum(E.frame_stats_ref(np.eye(4, dtype=np.float32)[preds[v]], labels[v]) for v in LENS)
    assert E.frame_stats_dict(counters, CLASSES) == stats
    assert run["groups"] == 2 and run["host_syncs"] <= run["groups"] + 2
    assert run["videos_own"] == 3 and run["videos"] == 3 and run["frames"] == 90
    assert run["exchange_bytes"] == 0                                     # one rank: nothing is handed to a collective
    assert plain_stats["exchange_bytes"] == 0 and plain_stats["videos_own"] == 3
    assert plain_stats["host_syncs"] <= plain_stats["groups"] + 1
    assert run["ap_d2h_bytes"] == plain_stats["ap_d2h_bytes"] + 8 * (2 + 3 * 4)
    # labels alone, no shard: the same numbers
    got2, stats2 = E.map_videos(m, vids, CLASSES, truth, SUPPRESS, TOLS, labels=labels, **KW)
    assert got2 == plain and stats2 == stats
    with pytest.raises(ValueError, match="labels and frame_stats go together"):
        m.map_video_group([frames["a"]], CLASSES, ops.ap_state([23], {}, 4, 1, [0], DEV), [0], suppress=[("raw",)],
                          labels=[labels["a"]])
    with pytest.raises(ValueError, match="23 integers"):
        m.map_video_group([frames["a"]], CLASSES, ops.ap_state([23], {}, 4, 1, [0], DEV), [0], suppress=[("raw",)],
                          labels=[labels["a"][:5]], frame_stats=torch.zeros(14, dtype=torch.int64, device=DEV))


def _shard_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from tdeed_amd import dist as tdist
    from test_gpu_spot import TINY, CLASSES, _model
    torch.cuda.set_device(0)                                  # both ranks share the one GPU of the box
    tdist.init(backend="gloo")
    m = _model(TINY)
    frames, truth, labels = tiny_inputs()
    names = sorted(LENS)
    own = E.shard_videos([LENS[v] for v in names], world)[rank]
    mine = {names[o] for o in own}
    vids = [(v, n, 25.0, frames[v] if v in mine else None) for v, n in LENS.items()]      # foreign sources: None
    got, stats = E.map_videos(m, vids, CLASSES, truth, SUPPRESS, TOLS, labels=labels, shard="auto", **KW)
    q.put((rank, got, stats, dict(m.last_video_stats)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_return_the_one_rank_result(monkeypatch):
    from test_gpu_dp import _free_port
    from test_gpu_spot import TINY, CLASSES, _model
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=300) for _ in procs), key=lambda x: x[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()                                 # past its limit: ended, never retried
    # the one-rank pass of this process; the state it leaves gives S and Hh of the byte condition
    seen = []
    real = ops.ap_state
    monkeypatch.setattr(ops, "ap_state", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    m = _model(TINY)
    frames, truth, labels = tiny_inputs()
    vids = [(v, n, 25.0, frames[v]) for v, n in LENS.items()]
    want, want_stats = E.map_videos(m, vids, CLASSES, truth, SUPPRESS, TOLS, labels=labels, **KW)
    state = seen[0]
    S_, Hh = int(state.ev_count.sum()), int(state.hit_count.sum())
    assert S_ > 0 and Hh > 0
    formula = exchange_bytes_formula(len(SUPPRESS), len(TOLS), 4, 3, S_, Hh)
    for rank, got, stats, run in res:
        assert got == want and stats == want_stats, rank      # bit for bit, on both ranks
        assert formula <= run["exchange_bytes"] <= formula + 64, (run["exchange_bytes"], formula)
        assert run["host_syncs"] <= run["groups"] + 2
    assert [r[3]["videos_own"] for r in res] == [1, 2] and sum(r[3]["videos_own"] for r in res) == 3
