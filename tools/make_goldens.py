"""Generate tests/golden/*.npz by running the REFERENCE (imported from /root/reference).

Runs only in the build container (the reference does not exist on the GPU box).
    python tools/make_goldens.py [--only NAME]
Inputs and weights come from tdeed_amd.synth (seeded, hash-based), so fixtures hold
only seeds + expected outputs.  Each fixture carries a json ``meta`` entry.
"""
import argparse
import hashlib
import json
import os
import sys
import types
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from transformers import RegNetConfig, RegNetModel  # noqa: E402  (before the fake torchvision goes in)
import ref_stubs  # noqa: E402
ref_stubs.install()
import tdeed_amd  # noqa: E402,F401
from tdeed_amd import synth  # noqa: E402

import model.modules as rmod  # noqa: E402  (reference)
import model.impl.gsf as rgsf  # noqa: E402
import model.impl.gsm as rgsm  # noqa: E402
rgsm.ftens = torch.FloatTensor      # torch.cuda.FloatTensor crashes on CPU
import model.model as rmodel  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)


def shapes_of(module):
    return {k: (tuple(v.shape), "int64" if v.dtype == torch.int64 else "float32")
            for k, v in module.state_dict().items()}


def fill(module, seed, prefix=""):
    sh = shapes_of(module)
    st = synth.make_state({prefix + k: v for k, v in sh.items()}, seed)
    module.load_state_dict({k: torch.from_numpy(st[prefix + k]) for k in sh})
    return st


def save(name, meta, **arrays):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **{k: np.asarray(v) for k, v in arrays.items()})
    print(f"  wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def act(seed, name, shape, scale=1.0):
    n = int(np.prod(shape))
    return (synth.normalish(seed, name, n) * scale).reshape(shape).astype(np.float32)


# ----------------------------------------------------------------------------- full model
def full_model(name, cfg, B, H, W, seed_w=0, seed_x=1000, augment=False, taps=()):
    args = types.SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **cfg)
    t0 = time.time()
    m = rmodel.TDEEDModel(device="cpu", args=args)
    fill(m._model, seed_w)
    m._model.eval()
    clip = synth.uint8_clip(seed_x, (B, cfg["clip_len"], 3, H, W))
    x = torch.from_numpy(clip).float()
    feats = {}
    hooks = []

    def mk(nm):
        def hook(mod, inp, out):
            feats[nm] = out.detach().numpy()
        return hook
    hooks.append(m._model._features.register_forward_hook(mk("pooled")))
    hooks.append(m._model._temp_fine.register_forward_hook(mk("sgp_out")))
    for tname in taps:
        mod = m._model
        for part in tname.split("."):
            mod = getattr(mod, part)
        hooks.append(mod.register_forward_hook(mk("tap:" + tname)))
    pred, _ = m._model(x, inference=True, augment_inference=augment)
    if isinstance(pred, dict):
        logits, displ = pred["im_feat"].numpy(), pred["displ_feat"].numpy()
    else:
        logits, displ = pred.numpy(), np.zeros((0,), np.float32)
    # the reference's own predict() post-processing on the same clip
    cls, scores = m.predict(torch.from_numpy(clip), use_amp=False, augment_inference=augment)
    for h in hooks:
        h.remove()
    Tn = cfg["clip_len"]
    pooled = feats["pooled"].reshape(B, Tn, -1)
    arrays = dict(logits=logits, displ=displ, pooled=pooled, sgp_out=feats["sgp_out"],
                  predict_cls=cls.astype(np.int64), predict_scores=scores)
    for k, v in feats.items():
        if k.startswith("tap:"):
            # taps are (B*T,C,h,w): keep channel means per frame + one full frame
            arrays[k + ":mean_hw"] = v.mean(axis=(2, 3))
            arrays[k + ":frame1"] = v[1]
    meta = dict(kind="full_model", cfg=cfg, B=B, H=H, W=W, seed_w=seed_w, seed_x=seed_x, augment=augment,
                n_params=int(sum(p.numel() for p in m._model.parameters())),
                n_state=len(m._model.state_dict()), secs=round(time.time() - t0, 1),
                layout_sha1=hashlib.sha1("\n".join(f"{k}:{tuple(v.shape)}" for k, v in m._model.state_dict().items())
                                         .encode()).hexdigest())
    save(name, meta, **arrays)
    return m


CFG_SMALL = dict(feature_arch="rny002_gsf", clip_len=100, crop_dim=224, n_layers=2, sgp_ks=7, sgp_r=4,
                 num_classes=4, radi_displacement=2)
CFG_BIG = dict(feature_arch="rny008_gsf", clip_len=100, crop_dim=224, n_layers=3, sgp_ks=7, sgp_r=4,
               num_classes=4, radi_displacement=2)
CFG_SNB = dict(feature_arch="rny008_gsf", clip_len=250, crop_dim=None, n_layers=2, sgp_ks=9, sgp_r=4,
               num_classes=12, radi_displacement=4)


def tiny(arch, T=16, **kw):
    d = dict(feature_arch=arch, clip_len=T, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2,
             num_classes=3, radi_displacement=2)
    d.update(kw)
    return d


# ----------------------------------------------------------------------------- module level
def mod_sgp_block(name, C, T, B, ks, r, seed=3):
    blk = rmod.SGPBlock(C, kernel_size=ks, k=r, init_conv_vars=0.1).eval()
    fill(blk, seed, "blk.")
    x = act(seed, name + ":x", (B, C, T))
    y = blk(torch.from_numpy(x)).numpy()
    save(name, dict(kind="sgp_block", C=C, T=T, B=B, ks=ks, r=r, seed=seed, layout="B,C,T"), y=y)


def mod_sgp_mixer(name, C, T_hi, T_lo, B, ks, r, seed=4):
    mx = rmod.SGPMixer(C, kernel_size=ks, k=r, init_conv_vars=0.1, t_size=T_hi, concat=True).eval()
    fill(mx, seed, "mix.")
    z = act(seed, name + ":z", (B, C, T_hi))
    x = act(seed, name + ":x", (B, C, T_lo))
    y = mx(x=torch.from_numpy(x), z=torch.from_numpy(z)).numpy()
    save(name, dict(kind="sgp_mixer", C=C, T_hi=T_hi, T_lo=T_lo, B=B, ks=ks, r=r, seed=seed, layout="B,C,T"), y=y)


def mod_pyramid(name, C, L, n, B, ks, r, seed=5):
    net = rmod.EDSGPMIXERLayers(C, L, num_layers=n, ks=ks, k=r, concat=True).eval()
    fill(net, seed, "_temp_fine.")
    x = act(seed, name + ":x", (B, L, C))
    y = net(torch.from_numpy(x)).numpy()
    save(name, dict(kind="pyramid", C=C, L=L, n=n, B=B, ks=ks, r=r, seed=seed, layout="B,T,C"), y=y)


def mod_misc(name="misc_ops", seed=6):
    out = {}
    ln = rmod.LayerNorm(48).eval()
    fill(ln, seed, "ln.")
    x = act(seed, "ln:x", (2, 48, 25))
    out["ln_y"] = ln(torch.from_numpy(x).clone()).numpy()
    for (L, O) in [(25, 13), (125, 63), (100, 50), (13, 7)]:
        x = act(seed, f"pool{L}:x", (2, 16, L))
        out[f"pool_{L}_{O}"] = torch.nn.AdaptiveMaxPool1d(O)(torch.from_numpy(x)).numpy()
    for (Lo, Hi) in [(13, 25), (25, 50), (63, 125), (50, 100)]:
        x = act(seed, f"up{Lo}:x", (2, 16, Lo))
        out[f"up_{Lo}_{Hi}"] = torch.nn.Upsample(size=Hi, mode="linear", align_corners=True)(torch.from_numpy(x)).numpy()
    save(name, dict(kind="misc", seed=seed, ln_C=48, ln_T=25), **out)


def mod_gate_shift(name, mode, F, T, B, h, w, seed=7):
    cls = rgsf._GSF if mode == "gsf" else rgsm._GSM
    gs = cls(F, T, 100).eval() if mode == "gsf" else cls(F, T).eval()
    fill(gs, seed, "gs.")
    x = act(seed, name + ":x", (B * T, F, h, w))
    y = gs(torch.from_numpy(x)).numpy()
    save(name, dict(kind="gate_shift", mode=mode, F=F, T=T, B=B, h=h, w=w, seed=seed, layout="N,C,H,W"), y=y)


def mod_loss(name="loss_postproc", seed=8):
    import torch.nn.functional as Fn
    B, T, K1 = 3, 20, 5
    logits = act(seed, "logits", (B, T, K1), 2.0)
    displ = act(seed, "displ", (B, T), 1.5)
    lab, labD = synth.labels(seed, B, T, K1 - 1, 2, fg_frac=0.3)
    w = torch.FloatTensor([1] + [5] * (K1 - 1))
    lg = torch.from_numpy(logits)
    hard = Fn.cross_entropy(lg.reshape(-1, K1), torch.from_numpy(lab).flatten(), weight=w)
    lam = synth.uniform01(seed, "lam", B)
    lab2, labD2 = synth.labels(seed + 1, B, T, K1 - 1, 2, fg_frac=0.3)
    soft = np.zeros((B, T, K1), np.float32)
    for i in range(B):
        soft[i, np.arange(T), lab[i]] += np.float32(lam[i])
        soft[i, np.arange(T), lab2[i]] += np.float32(1 - lam[i])
    softl = Fn.cross_entropy(lg.reshape(-1, K1), torch.from_numpy(soft).view(-1, K1), weight=w)
    mse = Fn.mse_loss(torch.from_numpy(displ), torch.from_numpy(labD).float(), reduction="none").mean()
    pp = rmod.process_prediction(lg, torch.from_numpy(displ)).numpy()
    pdh = rmod.process_double_head(lg, torch.from_numpy(displ), num_classes=3).numpy()
    pl = rmod.process_labels(torch.from_numpy(lab), torch.from_numpy(labD), num_classes=K1).numpy()
    # displacement values exactly at .5 exercise round-half-to-even
    d_half = np.tile(np.array([0.5, 1.5, -0.5, -1.5, 2.5], np.float32), (B, T // 5))
    pp_half = rmod.process_prediction(lg, torch.from_numpy(d_half)).numpy()
    save(name, dict(kind="loss", B=B, T=T, K1=K1, seed=seed, fg_weight=5),
         ce_hard=hard.numpy(), ce_soft=softl.numpy(), mse=mse.numpy(), soft_labels=soft,
         process_prediction=pp, process_double_head=pdh, process_labels=pl,
         d_half=d_half, process_prediction_half=pp_half)


def mod_eval_utils(name="eval_utils", seed=12):
    """Row f3: clip stitching, frame -> event conversion, (soft) NMS and mAP of the reference (util/eval.py,
    util/score.py) on synthetic score tracks.  Only expected outputs are stored; the inputs are regenerated from
    tdeed_amd.synth by the test."""
    for nm in ("SoccerNet", "SoccerNet.Evaluation", "SoccerNet.Evaluation.ActionSpotting", "SoccerNet.Evaluation.utils",
               "matplotlib", "matplotlib.pyplot"):
        if nm not in sys.modules:
            sys.modules[nm] = types.ModuleType(nm)
    sys.modules["SoccerNet.Evaluation.ActionSpotting"].average_mAP = None
    sys.modules["SoccerNet.Evaluation.utils"].LoadJsonFromZip = None
    import util.eval as reval
    import util.score as rscore
    K1, T = 5, 20
    videos = [("vid_b", 57, 25.0), ("vid_a", 43, 30.0), ("vid_c", 30, 25.0)]
    classes = {f"c{k}": k for k in range(1, K1)}

    class DS:
        pass
    ds = DS()
    ds.videos = videos
    ds._dataset = "finediving"
    labels = {}
    for vi, (v, L, _) in enumerate(videos):
        lab = synth.labels(seed + vi, 1, L, K1 - 1, 1, fg_frac=0.15)[0][0]
        labels[v] = lab
    ds.get_labels = lambda v: labels[v]
    # clips: stride T//2 starting before 0, softmax-like non-negative scores; some all-zero rows
    pred_dict = {v: (np.zeros((L, K1), np.float32), np.zeros(L, np.int32)) for v, L, _ in videos}
    clips = []
    for vi, (v, L, _) in enumerate(videos):
        for ci, start in enumerate(range(-T // 2, L, T // 2)):
            sc = np.abs(act(seed + 10 * vi + ci, f"clip{vi}_{ci}", (T, K1))).astype(np.float32)
            sc[:, 0] *= 2.5
            sc /= sc.sum(axis=1, keepdims=True)
            sc[(ci * 7) % T] = 0.0
            clips.append((v, start, sc))
            scores, support = pred_dict[v]
            ps, st = sc, start
            if st < 0:
                ps = ps[-st:, :]
                st = 0
            end = st + ps.shape[0]
            if end >= scores.shape[0]:
                end = scores.shape[0]
                ps = ps[:end - st, :]
            scores[st:end, :] += ps        # the accumulation of evaluate() (util/eval.py:299-313), which itself needs a model + DataLoader
            support[st:end] += (ps.sum(axis=1) != 0) * 1
    stitched = {v: (pred_dict[v][0].copy(), pred_dict[v][1].copy()) for v in pred_dict}
    err, f1, pe, pehr, pscores = reval.process_frame_predictions(ds, classes, pred_dict, high_recall_score_threshold=0.05)

    def pack(evlist):
        out = {}
        inv = classes
        for x in evlist:
            out[x["video"]] = np.array([[e["frame"], inv[e["label"]], e["score"]] for e in x["events"]], np.float64).reshape(-1, 3)
        return out
    nms1 = reval.non_maximum_supression(pehr, window=2, threshold=0.10)
    nms2 = reval.non_maximum_supression(pehr, window=[1, 3, 2, 4], threshold=0.0)
    snms = reval.soft_non_maximum_supression(pehr, window=3, threshold=0.05)
    truth = [{"video": v, "events": [{"label": f"c{int(k)}", "frame": int(i)} for i, k in enumerate(labels[v]) if k != 0]}
             for v, _, _ in videos]
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        maps_hr, _ = rscore.compute_mAPs(truth, pehr, tolerances=[0, 1, 2, 4])
        maps_nms, _ = rscore.compute_mAPs(truth, nms1, tolerances=[1, 2, 4])
        maps_pe, _ = rscore.compute_mAPs(truth, pe, tolerances=[0, 2])
    arrays = dict(err=np.float64(err.get()), f1_any=np.float64(f1.get(None)),
                  f1_cls=np.array([f1.get(k) for k in range(1, K1)], np.float64),
                  tpfpfn=np.array([f1.tp_fp_fn(k) for k in [None] + list(range(1, K1))], np.int64),
                  maps_hr=np.array(maps_hr), maps_nms=np.array(maps_nms), maps_pe=np.array(maps_pe))
    for tag, evl in (("pe", pe), ("pehr", pehr), ("nms1", nms1), ("nms2", nms2), ("snms", snms)):
        for v, a in pack(evl).items():
            arrays[f"{tag}__{v}"] = a
    for v in stitched:
        arrays[f"scores__{v}"] = stitched[v][0]
        arrays[f"support__{v}"] = stitched[v][1]
    save(name, dict(kind="eval_utils", seed=seed, K1=K1, T=T, videos=videos, hr_thr=0.05), **arrays)


def hf_regnet_crosscheck(name, arch, seed=9):
    """Independent structural check of the RegNetY trunk restatement (timm is absent): HuggingFace's
    RegNetYLayer stack, weights copied from the same synthetic state, same input -> pooled features."""
    from tdeed_amd.regnet_spec import regnet_spec
    spec = regnet_spec(arch)
    cfg = RegNetConfig(num_channels=3, embedding_size=32, hidden_sizes=list(spec.widths), depths=list(spec.depths),
                       groups_width=spec.gw, layer_type="y", hidden_act="relu")
    hf = RegNetModel(cfg).eval()
    ours = ref_stubs.RegNet(arch).eval()
    st = fill(ours, seed, "_features.")
    osd = ours.state_dict()
    hsd = hf.state_dict()

    def cp(dst, src):
        assert hsd[dst].shape == osd[src].shape, (dst, src)
        hsd[dst] = osd[src].clone()

    def cbn(dst, src):
        cp(dst + ".convolution.weight", src + ".conv.weight")
        for a in ("weight", "bias", "running_mean", "running_var"):
            cp(dst + ".normalization." + a, src + ".bn." + a)
    cbn("embedder.embedder", "stem")
    for b in spec.blocks:
        d = f"encoder.stages.{b.stage - 1}.layers.{b.index - 1}"
        s = b.name
        cbn(d + ".layer.0", s + ".conv1")
        cbn(d + ".layer.1", s + ".conv2")
        cp(d + ".layer.2.attention.0.weight", s + ".se.fc1.weight")
        cp(d + ".layer.2.attention.0.bias", s + ".se.fc1.bias")
        cp(d + ".layer.2.attention.2.weight", s + ".se.fc2.weight")
        cp(d + ".layer.2.attention.2.bias", s + ".se.fc2.bias")
        cbn(d + ".layer.3", s + ".conv3")
        if b.has_downsample:
            cbn(d + ".shortcut", s + ".downsample")
    hf.load_state_dict(hsd)
    x = act(seed, name + ":x", (2, 3, 64, 64))
    out = hf(torch.from_numpy(x)).pooler_output.flatten(1).numpy()
    n_params = sum(p.numel() for p in ours.parameters())
    save(name, dict(kind="hf_regnet", arch=arch, seed=seed, n_params_with_fc=int(n_params)), pooled=out)


def init_stats(name="init_stats", n_models=3):
    """Construction-time state of the reference (VERDICT r2 missing 1): per state_dict entry the mean / std / min / max
    over `n_models` freshly constructed reference models (torch.manual_seed 0, 1, 2), for the part of the model the
    reference itself constructs -- temp_enc, gate-shift modules, temporal stack, heads, every BatchNorm buffer.  The trunk
    convolutions come from the stand-in timm module (torch default init, NOT timm's) and are left out."""
    cfgs = {"gsf": tiny("rny002_gsf", T=16), "gsm": tiny("rny002_gsm", T=16)}
    arrays = {}
    metas = {}
    for tag, cfg in cfgs.items():
        acc = {}
        for s_ in range(n_models):
            torch.manual_seed(s_)
            args = types.SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **cfg)
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                m = rmodel.TDEEDModel(device="cpu", args=args)
            for k, v in m._model.state_dict().items():
                own = (not k.startswith("_features.")) or ".gs." in k or k.endswith(("running_mean", "running_var", "num_batches_tracked"))
                if own:
                    acc.setdefault(k, []).append(v.double().reshape(-1).numpy())
        keys = list(acc)
        st = np.zeros((len(keys), 5))
        for i, k in enumerate(keys):
            a = np.concatenate(acc[k])
            st[i] = [a.mean(), a.std(), a.min(), a.max(), a.size]
        arrays[f"{tag}_stats"] = st
        metas[tag] = dict(cfg=cfg, keys=keys)
    save(name, dict(kind="init_stats", n_models=n_models, cases=metas, columns=["mean", "std", "min", "max", "n"]), **arrays)


def timm_keymap(name="timm_keymap"):
    """Which state_dict key of the (stand-in) timm trunk each `_features.*` tensor of the reference model is: tensors are
    followed by identity (data_ptr) through make_temporal_shift (model/shift.py:46-59) and the model's own registration
    (model.py:60).  Pins init.timm_key_map's `conv1.* -> conv1.net.*` rewrite against the reference's wrapping."""
    out = {}
    for arch in ("rny002_gsf", "rny008_gsf", "rny002_gsm", "rny002"):
        cfg = tiny(arch, T=8)
        made = {}
        orig_create = sys.modules["timm"].create_model

        def create(nm, pretrained=False):
            made["net"] = orig_create(nm, pretrained)
            made["keep"] = dict(made["net"].state_dict())         # hold every tensor: a freed one's address may be reused
            made["before"] = {k: v.data_ptr() for k, v in made["keep"].items()}
            return made["net"]
        sys.modules["timm"].create_model = create
        rmodel.timm.create_model = create
        try:
            args = types.SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **cfg)
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                m = rmodel.TDEEDModel(device="cpu", args=args)
        finally:
            sys.modules["timm"].create_model = orig_create
            rmodel.timm.create_model = orig_create
        by_ptr = {p_: k for k, p_ in made["before"].items()}
        pairs = []
        for k, v in m._model.state_dict().items():
            if k.startswith("_features.") and v.data_ptr() in by_ptr:
                pairs.append([k, by_ptr[v.data_ptr()]])
        dropped = sorted(set(made["before"]) - {b for _, b in pairs})
        out[arch] = dict(pairs=pairs, dropped=dropped)
    save(name, dict(kind="timm_keymap", archs=out))


def frame_reader(name="frame_reader"):
    """Row f4: the reference's clip readers (dataset/frame.py:263-382 FrameReader.load_paths / load_frames, the training
    reader; 546-626 FrameReaderVideo.load_frames, the evaluation reader) on the small JPEG directories committed under
    tests/golden/frames/ (written here once from tdeed_amd.synth, then data).  torchvision.io.read_image is the Pillow
    stand-in of ref_stubs, so what the fixture pins is path naming, start / end padding, stride and the missing-file
    rules -- not the JPEG decoder."""
    from PIL import Image
    import dataset.frame as rframe
    base = os.path.join(GOLD, "frames")
    layouts = {
        # dataset -> (video_name handed to the reader, directory below frame_dir, file name of frame index i)
        "soccernetball": ("game_a/clip_1", "game_a/clip_1", lambda i: f"frame{i}.jpg"),
        "finediving": ("dive__01", "dive/01", lambda i: str(37 + i).zfill(5) + ".jpg"),
        "tennis": ("match_x_120_150", "match_x", lambda i: f"frame{120 + i}.jpg"),
        "finegym": ("vidA_E_0001", "vidA", lambda i: f"frame{40 - 3 + i}.jpg"),
    }
    src_info = {"finegym": dict(start_frame=40, pad=[3, 3])}
    n_frames, h, w = 7, 24, 32
    for ds, (vname, sub, fn) in layouts.items():
        d = os.path.join(base, ds, sub)
        os.makedirs(d, exist_ok=True)
        for i in range(n_frames):
            pth = os.path.join(d, fn(i))
            if not os.path.exists(pth):
                px = synth.uint8_clip(500 + i, (h, w, 3))
                Image.fromarray(px).save(pth, quality=92)
    arrays = {}
    cases = []
    spans = [(0, 7, 1, False), (-3, 4, 1, False), (3, 10, 1, False), (3, 10, 1, True), (-2, 10, 2, True), (0, 6, 2, False),
             (-4, 12, 3, True), (9, 14, 1, True)]
    for ds, (vname, sub, fn) in layouts.items():
        fdir = os.path.join(base, ds)
        rv = rframe.FrameReaderVideo(fdir, "rgb", ds)
        rt = rframe.FrameReader(fdir, "rgb", ds)
        for ci, (st, en, stride, pad) in enumerate(spans):
            got = rv.load_frames(vname, st, en, pad=pad, stride=stride, source_info=src_info.get(ds))
            key = f"video__{ds}__{ci}"
            arrays[key] = np.array(-1) if isinstance(got, int) else got.numpy()
            paths = rt.load_paths(vname, st, en, stride=stride, source_info=src_info.get(ds))
            rec = dict(dataset=ds, video=vname, start=st, end=en, stride=stride, pad=pad, video_key=key,
                       paths=[os.path.relpath(paths[0], base)] + [int(x) for x in paths[1:]])
            if paths[1] != -1 and paths[5] - paths[2] - paths[3] > 0:
                tr = rt.load_frames(paths, pad=pad, stride=stride)
                rec["train_key"] = f"train__{ds}__{ci}"
                arrays[rec["train_key"]] = tr.numpy()
            cases.append(rec)
    save(name, dict(kind="frame_reader", cases=cases, source_info=src_info, n_frames=n_frames, h=h, w=w,
                    layouts={k: [v[0], v[1]] for k, v in layouts.items()}), **arrays)


def video_clips(name="video_clips"):
    """The clip lists of the reference's evaluation dataset (dataset/frame.py:385-452 ActionSpotVideoDataset): per case the
    (video, start) list of `_clips` in dataset order and the (name, length, fps) triples of `.videos`, from a temporary
    label file.  Dataset names other than soccernet / soccernetball (those read label paths at construction).  Covers
    strides 1, 2, 12, videos shorter than a clip, videos no longer than overlap_len * stride (the range's end collapses
    to 0) and lengths that are no multiple of the stride."""
    import tempfile
    import dataset.frame as rframe
    lengths = [3, 6, 7, 8, 37, 75, 100, 101, 430, 899, 1201]
    settings = [  # (clip_len, overlap_len, stride, dataset)
        (8, 6, 1, "finediving"), (8, 6, 2, "finediving"), (8, 6, 12, "fs_comp"), (8, 4, 1, "tennis"), (8, 0, 2, "fs_perf"),
        (100, 75, 1, "finediving"), (100, 75, 2, "fs_comp"), (100, 50, 12, "tennis"), (100, 75, 12, "fs_perf"),
    ]
    arrays, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        labels = [dict(video=f"v{n:05d}", num_frames=n, fps=25.0, events=[]) for n in lengths]
        lf = os.path.join(tmp, "labels.json")
        with open(lf, "w") as fh:
            json.dump(labels, fh)
        for ci, (clip_len, overlap, stride, ds) in enumerate(settings):
            d = rframe.ActionSpotVideoDataset({}, lf, tmp, "rgb", clip_len, overlap_len=overlap, stride=stride, dataset=ds)
            vids = [v for v, _ in d._clips]
            arrays[f"clip_video__{ci}"] = np.array([lengths.index(int(v[1:])) for v in vids], np.int32)
            arrays[f"clip_start__{ci}"] = np.array([s for _, s in d._clips], np.int64)
            arrays[f"clip_start_sampled__{ci}"] = np.array([s // stride for _, s in d._clips], np.int64)   # frame.py:451
            vv = d.videos
            arrays[f"videos_len__{ci}"] = np.array([n for _, n, _ in vv], np.int64)
            arrays[f"videos_fps__{ci}"] = np.array([f for _, _, f in vv], np.float64)
            cases.append(dict(clip_len=clip_len, overlap_len=overlap, stride=stride, dataset=ds, pad_len=rframe.DEFAULT_PAD_LEN,
                              videos=[v for v, _, _ in vv]))
    save(name, dict(kind="video_clips", lengths=lengths, names=[f"v{n:05d}" for n in lengths], cases=cases), **arrays)


def train_clips(name="train_clips"):
    """The reference's TRAINING dataset (dataset/frame.py:30-256 ActionSpotDataset, store_mode='store') on a temporary label
    file and frame directories of tiny JPEGs: per case the clip list (video, base_idx) of `_store_clips` and, after
    `random.seed(s)`, the label / labelD / label2 / labelD2 rows of the first 12 `__getitem__` calls (the reference's own
    `_get_one`, frames decoded and thrown away).  Dataset names other than soccernet / soccernetball.  The events hold two
    of different classes closer than 2r (overwrite order), events within r of frame 0 and of the last frame, events before
    a clip's base (negative numerator of the floor division) and events at frames that are no multiple of the stride."""
    import random
    import tempfile
    from PIL import Image
    import dataset.frame as rframe
    classes = {"dive": 1, "turn": 2, "land": 3}
    ev = lambda *pairs: [dict(frame=f, label=l) for f, l in pairs]     # noqa: E731
    videos = [
        dict(video="v00003", num_frames=3, events=ev((1, "dive"))),
        dict(video="v00006", num_frames=6, events=ev((0, "turn"), (5, "land"))),
        dict(video="v00007", num_frames=7, events=ev((3, "land"), (4, "dive"))),
        dict(video="v00037", num_frames=37, events=ev((0, "dive"), (1, "turn"), (17, "land"), (19, "dive"), (35, "land"),
                                                      (36, "turn"))),
        dict(video="v00101", num_frames=101, events=ev((2, "turn"), (53, "land"), (50, "dive"), (99, "dive"), (100, "turn"))),
        dict(video="v00430", num_frames=430, events=ev((1, "land"), (7, "dive"), (100, "turn"), (103, "land"), (215, "dive"),
                                                       (301, "turn"), (300, "land"), (427, "dive"), (429, "turn"))),
    ]
    settings = [  # (clip_len, stride, overlap, radi_displacement, mixup, dataset, seed)
        (8, 1, 1, 0, True, "fs_comp", 11), (8, 1, 1, 2, True, "fs_comp", 12), (8, 2, 1, 2, True, "fs_perf", 13),
        (8, 3, 0.5, 1, True, "fs_comp", 14), (100, 1, 1, 4, True, "fs_perf", 15), (100, 12, 1, 2, True, "fs_comp", 16),
        (8, 1, 1, 2, False, "fs_comp", 17),
    ]
    n_items = 12
    arrays, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for v in videos:
            d = os.path.join(tmp, "frames", v["video"])
            os.makedirs(d)
            for i in range(v["num_frames"]):
                Image.fromarray(synth.uint8_clip(700 + i, (8, 8, 3))).save(os.path.join(d, f"frame{i}.jpg"), quality=90)
        lf = os.path.join(tmp, "train.json")
        with open(lf, "w") as fh:
            json.dump(videos, fh)
        names = [v["video"] for v in videos]
        for ci, (clip_len, stride, overlap, radi, mixup, ds, seed) in enumerate(settings):
            d = rframe.ActionSpotDataset(classes, lf, os.path.join(tmp, "frames"), os.path.join(tmp, f"store{ci}"), "store", "rgb",
                                         clip_len, n_items, stride=stride, overlap=overlap, radi_displacement=radi, mixup=mixup,
                                         dataset=ds)
            # the clip list: _frame_paths holds [base_path, found_start, pad_start, pad_end, ndigits, length] per kept clip;
            # base_idx is recovered by replaying the reference's own range and its keep rule on its own load_paths
            kept_video, kept_base = [], []
            k = 0
            for vi, v in enumerate(videos):
                for base_idx in range(-d._pad_len * d._stride, max(0, v["num_frames"] - 1 + (2 * d._pad_len - d._clip_len) * d._stride),
                                      d._overlap):
                    paths = d._frame_reader.load_paths(v["video"], base_idx, base_idx + d._clip_len * d._stride, stride=d._stride)
                    if paths[1] != -1:
                        assert d._frame_paths[k] == paths, (ci, vi, base_idx)
                        kept_video.append(vi)
                        kept_base.append(base_idx)
                        k += 1
            assert k == len(d._frame_paths) == d._total_len
            arrays[f"clip_video__{ci}"] = np.array(kept_video, np.int32)
            arrays[f"clip_base__{ci}"] = np.array(kept_base, np.int64)
            random.seed(seed)
            items = [d[i] for i in range(n_items)]
            keys = ["label"] + (["labelD"] if radi > 0 else []) + ((["label2"] + (["labelD2"] if radi > 0 else [])) if mixup else [])
            for key in keys:
                arrays[f"{key}__{ci}"] = np.stack([it[key] for it in items]).astype(np.int64)
            cases.append(dict(clip_len=clip_len, stride=stride, overlap=overlap, radi_displacement=radi, mixup=mixup, dataset=ds,
                              seed=seed, pad_len=rframe.DEFAULT_PAD_LEN, n_clips=int(d._total_len), keys=keys))
    save(name, dict(kind="train_clips", classes=classes, videos=videos, names=names, n_items=n_items, cases=cases), **arrays)


def train_clips_joint(name="train_clips_joint"):
    """The reference's JOINT training dataset (dataset/frame.py:640-663 ActionSpotDatasetJoint over two ActionSpotDataset,
    store_mode='store' -- the `pretrain` branch of get_datasets) on two temporary label files and frame directories of 8 x 8
    JPEGs.  Two class lists, dataset names other than soccernet / soccernetball, the events with the hard cases of
    `train_clips`.  Per case (the parts' stride / overlap pairs (1, 1 | 2, 0.5), (2, 0.9 | 2, 0.5) -- at clip_len 40, where
    int((1 - 0.9) * 40) truncates to a step of 3 --, (12, 1 | 1, 1), and two without mixup): each part's clip list and, after
    `random.seed(s)`, of the first 24 items the part, the clip index inside the part and the partner's -- the arguments and
    results of the reference's own `random.randint` calls, recorded while it draws -- and the label / labelD / label2 /
    labelD2 rows; for case 0 the `frame` / `frame2` arrays too.  The decoded frames of every video are stored as the
    reference's reader returns them, so that a test can rebuild any clip.  Asserts per case that both parts occur and that
    a recorded clip hangs over the end of its video."""
    import random
    import tempfile
    from PIL import Image
    import dataset.frame as rframe
    ev = lambda *pairs: [dict(frame=f, label=l) for f, l in pairs]     # noqa: E731
    parts = [
        dict(dataset="fs_comp", classes={"dive": 1, "turn": 2, "land": 3}, videos=[
            dict(video="v00003", num_frames=3, events=ev((1, "dive"))),
            dict(video="v00007", num_frames=7, events=ev((3, "land"), (4, "dive"))),
            dict(video="v00037", num_frames=37, events=ev((0, "dive"), (1, "turn"), (17, "land"), (19, "dive"), (35, "land"),
                                                          (36, "turn"))),
            dict(video="v00101", num_frames=101, events=ev((2, "turn"), (53, "land"), (50, "dive"), (99, "dive"), (100, "turn"))),
        ]),
        dict(dataset="fs_perf", classes={"jump": 1, "spin": 2, "step": 3, "fall": 4, "bow": 5}, videos=[
            dict(video="w00006", num_frames=6, events=ev((0, "spin"), (5, "fall"))),
            dict(video="w00020", num_frames=20, events=ev((9, "step"), (8, "jump"), (19, "bow"))),
            dict(video="w00064", num_frames=64, events=ev((1, "fall"), (7, "jump"), (30, "spin"), (33, "step"), (31, "bow"),
                                                          (62, "bow"), (63, "jump"))),
        ]),
    ]
    settings = [  # (clip_len, (stride, overlap) of part 1, of part 2, radi_displacement, mixup, seed)
        (8, (1, 1), (2, 0.5), 2, True, 41), (40, (2, 0.9), (2, 0.5), 2, True, 42), (8, (12, 1), (1, 1), 1, True, 43),
        (8, (1, 1), (2, 0.5), 0, False, 44), (8, (3, 0.5), (2, 1), 2, False, 45),
    ]
    n_items = 24
    arrays, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for k, p in enumerate(parts):
            fdir = os.path.join(tmp, f"frames{k}")
            reader = rframe.FrameReader(fdir, "rgb", p["dataset"])
            for vi, v in enumerate(p["videos"]):
                d = os.path.join(fdir, v["video"])
                os.makedirs(d)
                for i in range(v["num_frames"]):
                    Image.fromarray(synth.uint8_clip(900 + 1000 * k + 37 * vi + i, (8, 8, 3))).save(os.path.join(d, f"frame{i}.jpg"),
                                                                                                     quality=90)
                arrays[f"video__p{k}__{vi}"] = np.stack([reader.read_frame(os.path.join(d, f"frame{i}.jpg")).numpy()
                                                         for i in range(v["num_frames"])]).astype(np.uint8)
            p["label_file"] = os.path.join(tmp, f"train{k}.json")
            with open(p["label_file"], "w") as fh:
                json.dump(p["videos"], fh)
        for ci, (clip_len, sp1, sp2, radi, mixup, seed) in enumerate(settings):
            dsets = []
            for k, (p, (stride, overlap)) in enumerate(zip(parts, (sp1, sp2))):
                d = rframe.ActionSpotDataset(p["classes"], p["label_file"], os.path.join(tmp, f"frames{k}"),
                                             os.path.join(tmp, f"store{ci}_{k}"), "store", "rgb", clip_len, n_items // 2, stride=stride,
                                             overlap=overlap, radi_displacement=radi, mixup=mixup, dataset=p["dataset"])
                kept_video, kept_base, n = [], [], 0
                for vi, v in enumerate(p["videos"]):
                    for base_idx in range(-d._pad_len * d._stride,
                                          max(0, v["num_frames"] - 1 + (2 * d._pad_len - d._clip_len) * d._stride), d._overlap):
                        paths = d._frame_reader.load_paths(v["video"], base_idx, base_idx + d._clip_len * d._stride, stride=d._stride)
                        if paths[1] != -1:
                            assert d._frame_paths[n] == paths, (ci, k, vi, base_idx)
                            kept_video.append(vi)
                            kept_base.append(base_idx)
                            n += 1
                assert n == len(d._frame_paths) == d._total_len
                arrays[f"clip_video__{ci}__p{k}"] = np.array(kept_video, np.int32)
                arrays[f"clip_base__{ci}__p{k}"] = np.array(kept_base, np.int64)
                dsets.append(d)
            joint = rframe.ActionSpotDatasetJoint(*dsets)
            assert len(joint) == n_items
            calls = []
            real_randint = random.randint

            def spy(a, b):
                r = real_randint(a, b)
                calls.append((a, b, r))
                return r
            random.seed(seed)
            random.randint = spy
            try:
                items, drawn = [], []
                for i in range(n_items):
                    del calls[:]
                    items.append(joint[i])
                    drawn.append(list(calls))
            finally:
                random.randint = real_randint
            part = np.array([it["dataset"] for it in items], np.int64)
            assert set(part.tolist()) == {1, 2}, (ci, part)
            for it, dr in zip(items, drawn):
                assert len(dr) == (2 if mixup else 1) and all(a == 0 and b == dsets[it["dataset"] - 1]._total_len - 1 for a, b, _ in dr)
            idx = np.array([dr[0][2] for dr in drawn], np.int64)
            arrays[f"part__{ci}"], arrays[f"idx__{ci}"] = part, idx
            if mixup:
                arrays[f"idx2__{ci}"] = np.array([dr[1][2] for dr in drawn], np.int64)
            over = 0
            for pk, c in zip(part, idx):
                k = int(pk) - 1
                v = parts[k]["videos"][int(arrays[f"clip_video__{ci}__p{k}"][c])]
                over += int(arrays[f"clip_base__{ci}__p{k}"][c]) + (clip_len - 1) * (sp1, sp2)[k][0] >= v["num_frames"]
            assert over > 0, ci
            keys = ["label"] + (["labelD"] if radi > 0 else []) + ((["label2"] + (["labelD2"] if radi > 0 else [])) if mixup else [])
            for key in keys:
                arrays[f"{key}__{ci}"] = np.stack([np.asarray(it[key]) for it in items]).astype(np.int64)
            frame_keys = []
            if ci == 0:
                frame_keys = ["frame", "frame2"]
                for key in frame_keys:
                    arrays[f"{key}__{ci}"] = np.stack([it[key].numpy() for it in items]).astype(np.uint8)
            cases.append(dict(clip_len=clip_len, strides=[sp1[0], sp2[0]], overlaps=[sp1[1], sp2[1]], radi_displacement=radi,
                              mixup=mixup, seed=seed, pad_len=rframe.DEFAULT_PAD_LEN, dataset_len=[n_items // 2, n_items // 2],
                              n_clips=[int(d._total_len) for d in dsets], keys=keys, frame_keys=frame_keys))
    save(name, dict(kind="train_clips_joint", n_items=n_items, cases=cases,
                    parts=[dict(dataset=p["dataset"], classes=p["classes"], videos=p["videos"]) for p in parts]), **arrays)


# ----------------------------------------------------------------------------- training
TRAIN_KEYS = [
    "_features.stem.conv.weight", "_features.stem.bn.weight", "_features.s1.b1.downsample.conv.weight",
    "_features.s2.b1.se.fc1.weight", "_features.s3.b1.conv1.gs.conv3D.weight", "_features.s3.b1.conv1.gs.bn.weight",
    "_features.s3.b1.conv1.gs.channel_conv1.weight", "_features.s3.b2.conv2.conv.weight",
    "_features.s4.b2.conv1.gs.channel_conv2.bias", "_features.s4.b1.se.fc2.bias", "_features.s4.b3.conv3.bn.bias",
    "_features.s4.b7.conv1.net.conv.weight", "temp_enc",
    "_temp_fine._sgp.0.ln.weight", "_temp_fine._sgp.1.convkw.weight", "_temp_fine._sgp.2.mlp.0.weight",
    "_temp_fine._sgp.4.gn.bias", "_temp_fine._sgp.3.mlp.2.bias", "_temp_fine._sgpMixer.0.concat_fc.weight",
    "_temp_fine._sgpMixer.1.psi2.weight", "_temp_fine._sgpMixer.0.global_fc1.weight",
    "_pred_fine._fc_out.weight", "_pred_fine._fc_out.bias", "_pred_displ._fc_out.weight",
]


def sample_flat(a, cap=8192):
    """what a fixture keeps of a tensor: all of it up to `cap` values, else every stride-th value"""
    a = np.asarray(a).reshape(-1)
    stride = 1 if a.size <= cap else a.size // 4096 + 1
    return a[::stride].copy()


class _MaskDrop(torch.nn.Module):
    """nn.Dropout() of FCLayers (modules.py:372) with its random keep-mask replaced by a recorded one: x * mask, mask in
    {0, 1/(1-p)} = {0, 2} -- exactly what F.dropout(p=0.5, training=True) computes for that draw."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


def drop_masks(seed, B, T, C, n):
    return [((synth.normalish(seed + i, "dropmask", B * T * C) > 0).astype(np.float32) * 2.0).reshape(B, T, C)
            for i in range(n)]


def _train_model(cfg, seed_w, mask_seed, B):
    args = types.SimpleNamespace(modality="rgb", temporal_arch="ed_sgp_mixer", pretrain=None, **cfg)
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        m = rmodel.TDEEDModel(device="cpu", args=args)
    fill(m._model, seed_w)
    C = m._model._feat_dim
    mk = drop_masks(mask_seed, B, cfg["clip_len"], C, 2)
    m._model._pred_fine.dropout = _MaskDrop(torch.from_numpy(mk[0]))       # class head
    m._model._pred_displ.dropout = _MaskDrop(torch.from_numpy(mk[1]))      # displacement head
    return m, args


def _chained(opt, warm_steps, cos_steps):
    """train_tdeed.py:79-87 get_lr_scheduler: LinearLR(0.01 -> 1) chained with CosineAnnealingLR"""
    from torch.optim.lr_scheduler import ChainedScheduler, LinearLR, CosineAnnealingLR
    return ChainedScheduler([LinearLR(opt, start_factor=0.01, end_factor=1.0, total_iters=warm_steps),
                             CosineAnnealingLR(opt, cos_steps)])


def train_step(name, arch="rny002_gsf", seed_w=21, seed_x=2100, n_steps=3, lr=5e-5):
    """Reference TDEEDModel in .train(): Impl.forward(x, inference=True) (center-crop branch: no random augmentation,
    model.py:119-129) with BatchNorm batch statistics and the heads' dropout on a recorded mask, the loss of epoch()
    (model.py:208-211, 308-319), modules.step() (390-404) with AdamW from get_optimizer (37-39) and the chained
    LinearLR + CosineAnnealingLR of train_tdeed.py:79-87 -- `n_steps` steps on the same batch."""
    import torch.nn.functional as Fn
    cfg = tiny(arch, T=16)
    B, H, W = 2, 64, 64
    t0 = time.time()
    m, args = _train_model(cfg, seed_w, seed_x + 7, B)
    net = m._model
    net.train()
    clip = synth.uint8_clip(seed_x, (B, cfg["clip_len"], 3, H, W))
    lab, labD = synth.labels(seed_x + 1, B, cfg["clip_len"], cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.3)
    K1 = cfg["num_classes"] + 1
    wgt = torch.FloatTensor([1] + [5] * (K1 - 1))
    opt, scaler = m.get_optimizer({"lr": lr})
    assert scaler is None
    sched = _chained(opt, 2, 4)
    names = [k for k, _ in net.named_parameters()]
    proj = {k: synth.normalish(77, "proj:" + k, p.numel()).astype(np.float64) for k, p in net.named_parameters()}
    arrays = {}
    losses, lrs = [], [opt.param_groups[0]["lr"]]
    grabbed = {}

    def grab(optimizer, a_, kw_):                       # the gradients modules.step() hands to AdamW, first step only
        if not grabbed:
            grabbed.update({k: p.grad.detach().double().numpy().reshape(-1).copy() for k, p in net.named_parameters()})
    opt.register_step_pre_hook(grab)
    with torch.enable_grad():
        for s_ in range(n_steps):
            pred, _ = net(torch.from_numpy(clip).float(), inference=True)
            loss = Fn.cross_entropy(pred["im_feat"].reshape(-1, K1), torch.from_numpy(lab).flatten(), weight=wgt)
            loss = loss + Fn.mse_loss(pred["displ_feat"], torch.from_numpy(labD).float(), reduction="none").mean()
            losses.append(float(loss.detach()))
            if s_ == 0:
                arrays["logits0"] = pred["im_feat"].detach().numpy().copy()
                arrays["displ0"] = pred["displ_feat"].detach().numpy().copy()
            rmod.step(opt, scaler, loss, lr_scheduler=sched)
            lrs.append(opt.param_groups[0]["lr"])
            if s_ == 0:
                sd1 = net.state_dict()
                for k in TRAIN_KEYS:
                    arrays["param1:" + k] = sample_flat(sd1[k].detach().numpy())
    g = grabbed
    arrays["grad_norm"] = np.array([np.linalg.norm(g[k]) for k in names])
    arrays["grad_proj"] = np.array([float(g[k] @ proj[k]) for k in names])
    for k in TRAIN_KEYS:
        arrays["grad:" + k] = sample_flat(g[k].astype(np.float32))
    sd = net.state_dict()
    for k in TRAIN_KEYS:
        arrays["param:" + k] = sample_flat(sd[k].detach().numpy())
    bn_keys = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    arrays["bn_running"] = np.concatenate([sd[k].numpy().reshape(-1) for k in bn_keys])
    arrays["bn_tracked"] = np.array([int(sd[k]) for k in sd if k.endswith("num_batches_tracked")], np.int64)
    arrays["losses"] = np.array(losses, np.float64)
    arrays["lrs"] = np.array(lrs, np.float64)
    meta = dict(kind="train_step", cfg=cfg, B=B, H=H, W=W, seed_w=seed_w, seed_x=seed_x, mask_seed=seed_x + 7,
                label_seed=seed_x + 1, n_steps=n_steps, lr=lr, warm_steps=2, cos_steps=4, fg_frac=0.3, proj_seed=77,
                param_names=names, bn_keys=bn_keys, keys=TRAIN_KEYS, sample_cap=8192, secs=round(time.time() - t0, 1))
    save(name, meta, **arrays)


def train_epoch(name, arch="rny002_gsf", seed_w=23, seed_x=2300, lr=2e-3):
    """The reference's own TDEEDModel.epoch() training branch (model.py:193-332) on a two-batch loader -- a plain batch
    and a mixup batch ('frame2' / 'label2' / 'labelD2', Beta(0.2, 0.2) weights from `random`) -- with acc_grad_iter=2,
    AdamW and the chained scheduler.  crop_dim None and the augmentation Compose emptied (the draw in which no
    RandomApply fires and no flip happens), dropout on recorded masks."""
    import random
    cfg = tiny(arch, T=16)
    B, H, W, T_ = 2, 64, 64, 16
    t0 = time.time()
    m, args = _train_model(cfg, seed_w, seed_x + 7, B)
    net = m._model
    net.augmentation = sys.modules["torchvision.transforms"].Compose([])
    batches = []
    for i in range(2):
        fr = synth.uint8_clip(seed_x + 10 * i, (B, T_, 3, H, W))
        lab, labD = synth.labels(seed_x + 10 * i + 1, B, T_, cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.3)
        bt = {"frame": torch.from_numpy(fr), "label": torch.from_numpy(lab), "labelD": torch.from_numpy(labD)}
        if i == 1:
            fr2 = synth.uint8_clip(seed_x + 10 * i + 5, (B, T_, 3, H, W))
            lab2, labD2 = synth.labels(seed_x + 10 * i + 6, B, T_, cfg["num_classes"], cfg["radi_displacement"], fg_frac=0.3)
            bt.update(frame2=torch.from_numpy(fr2), label2=torch.from_numpy(lab2), labelD2=torch.from_numpy(labD2))
        batches.append(bt)
    opt, scaler = m.get_optimizer({"lr": lr})
    sched = _chained(opt, 2, 4)
    random.seed(5)
    rmodel.tqdm = lambda it: it
    with torch.enable_grad():
        avg = m.epoch(batches, optimizer=opt, scaler=scaler, lr_scheduler=sched, acc_grad_iter=2)
    random.seed(5)
    lam = [random.betavariate(0.2, 0.2) for _ in range(B)]
    sd = net.state_dict()
    arrays = {"loss": np.float64(avg), "lam": np.array(lam, np.float64), "lr_after": np.float64(opt.param_groups[0]["lr"])}
    for k in TRAIN_KEYS:
        arrays["param:" + k] = sample_flat(sd[k].detach().numpy())
    bn_keys = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    arrays["bn_running"] = np.concatenate([sd[k].numpy().reshape(-1) for k in bn_keys])
    arrays["bn_tracked"] = np.array([int(sd[k]) for k in sd if k.endswith("num_batches_tracked")], np.int64)
    meta = dict(kind="train_epoch", cfg=cfg, B=B, H=H, W=W, seed_w=seed_w, seed_x=seed_x, mask_seed=seed_x + 7, lr=lr,
                warm_steps=2, cos_steps=4, acc_grad_iter=2, random_seed=5, fg_frac=0.3, keys=TRAIN_KEYS, bn_keys=bn_keys,
                sample_cap=8192, secs=round(time.time() - t0, 1))
    save(name, meta, **arrays)


CASES = {
    "init_stats": lambda: init_stats(),
    "timm_keymap": lambda: timm_keymap(),
    "frame_reader": lambda: frame_reader(),
    "video_clips": lambda: video_clips(),
    "misc_ops": lambda: mod_misc(),
    "loss_postproc": lambda: mod_loss(),
    "eval_utils": lambda: mod_eval_utils(),
    "sgp_block_c32_t25": lambda: mod_sgp_block("sgp_block_c32_t25", 32, 25, 2, 5, 2),
    "sgp_block_c368_t100": lambda: mod_sgp_block("sgp_block_c368_t100", 368, 100, 1, 7, 4),
    "sgp_block_c48_t13": lambda: mod_sgp_block("sgp_block_c48_t13", 48, 13, 2, 9, 4),
    "sgp_mixer_c32_t25": lambda: mod_sgp_mixer("sgp_mixer_c32_t25", 32, 25, 13, 2, 5, 2),
    "sgp_mixer_c368_t100": lambda: mod_sgp_mixer("sgp_mixer_c368_t100", 368, 100, 50, 1, 7, 4),
    "pyramid_c32_l25_n2": lambda: mod_pyramid("pyramid_c32_l25_n2", 32, 25, 2, 2, 5, 2),
    "pyramid_c64_l100_n3": lambda: mod_pyramid("pyramid_c64_l100_n3", 64, 100, 3, 2, 7, 4),
    "pyramid_c48_l250_n2": lambda: mod_pyramid("pyramid_c48_l250_n2", 48, 250, 2, 1, 9, 4),
    "gsf_f16": lambda: mod_gate_shift("gsf_f16", "gsf", 16, 8, 2, 6, 6),
    "gsf_f40": lambda: mod_gate_shift("gsf_f40", "gsf", 40, 6, 1, 5, 5),
    "gsf_f92": lambda: mod_gate_shift("gsf_f92", "gsf", 92, 5, 1, 4, 4),
    "gsm_f16": lambda: mod_gate_shift("gsm_f16", "gsm", 16, 8, 2, 6, 6),
    "hf_regnet_rny002": lambda: hf_regnet_crosscheck("hf_regnet_rny002", "rny002"),
    "hf_regnet_rny008": lambda: hf_regnet_crosscheck("hf_regnet_rny008", "rny008"),
    "tiny_rny002_gsf": lambda: full_model("tiny_rny002_gsf", tiny("rny002_gsf"), 2, 64, 64,
                                          taps=("_features.s3.b1", "_features.s4.b2")),
    "tiny_rny008_gsf": lambda: full_model("tiny_rny008_gsf", tiny("rny008_gsf", n_layers=3, sgp_ks=7, sgp_r=4), 2, 64, 64),
    "tiny_rny002_gsm": lambda: full_model("tiny_rny002_gsm", tiny("rny002_gsm"), 2, 64, 64),
    "tiny_rny002_crop_flip": lambda: full_model("tiny_rny002_crop_flip", tiny("rny002_gsf", crop_dim=64, radi_displacement=0),
                                                1, 72, 80, augment=True),
    "finediving_small": lambda: full_model("finediving_small", CFG_SMALL, 1, 224, 224),
    "finediving_big": lambda: full_model("finediving_big", CFG_BIG, 1, 224, 224),
    "snb_t250": lambda: full_model("snb_t250", CFG_SNB, 1, 160, 160),
    "train_step_tiny_rny002": lambda: train_step("train_step_tiny_rny002"),
    "train_epoch_tiny_rny002": lambda: train_epoch("train_epoch_tiny_rny002"),
    "train_clips": train_clips,
    "train_clips_joint": train_clips_joint,
}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    for k, fn in CASES.items():
        if a.only and k not in a.only:
            continue
        print(k)
        fn()
