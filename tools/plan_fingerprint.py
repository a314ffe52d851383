"""Fingerprints of the forward engine's launch plans and packed weights, computed without a GPU.

    python tools/plan_fingerprint.py [TREE] --plans [--forms] | --weights [--set NAME=VALUE ...] | --variants

Two trees (two commits) whose outputs are byte-identical build the same plans -- the same launches with the same costs over
the same buffer assignment -- and pack the same weights.  What the fingerprint cannot see are the arguments captured in the
Step closures; the GPU suite checks those.

--plans builds the plans on torch's "meta" device: the engine is made without its constructor, its weights are packed for
"meta" (every GPU-only form is chosen as on the card, the *_fits / *_parts / *_form predicates are host functions of the built
library), no Step is ever called.  --weights packs on the CPU.  --set flips a module attribute of `engine` after import;
--variants runs --plans once per plan switch, each in a process of its own (some switches are read at import).  --forms adds,
under each plan's line, one line per bottleneck of each of its runs with the launch form that engine.block_forms chose.
"""
import argparse
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import torch

VARIANTS = [{}, {"TDEED_BNECK": "0"}, {"TDEED_C1_GCONV": "0"}, {"TDEED_GS_SRC_ORDER": "0"}, {"TDEED_SGP_GEMM": "0"},
            {"TDEED_SGP_FUSED": "0"}, {"TDEED_SGP_F32_STREAM": "0"}, ["BNECK_BLEND=False"], ["BNECK_QTAIL=False"], ["SC_IN_CONV3=False"],
            ["S1_CONV3_IN_C1G=False"], ["BNECK_ONE_LAUNCH=False", "C1_GCONV=False"]]
GEOMETRIES = [("rny002_gsf", 2, 100, 8, 224), ("rny008_gsf", 3, 100, 16, 224), ("rny008_gsf", 3, 250, 4, 224),
              ("rny002_gsm", 2, 16, 2, 224), ("rny002", 2, 16, 2, 224), ("rny002_gsf", 2, 16, 2, 112), ("rny002_gsf", 2, 16, 2, 96)]
OPTIONS = [{}, dict(n_split=2), dict(n_split=2, join_at=3), dict(n_split=2, merge_tail=False), dict(fuse_front=False)]
DTYPES = (torch.bfloat16, torch.float32)


def digest(obj):
    return hashlib.sha256(repr(obj).encode()).hexdigest()[:16]


def config(arch, n_layers, T):
    return dict(feature_arch=arch, clip_len=T, crop_dim=None, n_layers=n_layers, sgp_ks=5, sgp_r=2, num_classes=3,
                radi_displacement=2)


def patch_meta(E, set_attr=setattr):
    """What planning on "meta" replaces in the engine module (set_attr: setattr, or a pytest monkeypatch's)."""
    set_attr(E, "new_stream", lambda *a, **k: None)
    for mod in {E, sys.modules.get("tdeed_amd.packing", E)}:      # the folded-BN vectors of the front are read back on the host
        set_attr(mod, "_np", (lambda real: lambda v: np.zeros(tuple(v.shape), np.float32)
                              if getattr(v, "is_meta", False) else real(v))(mod._np))


def meta_engine(E, cfg, pw, n_split=1, merge_tail=True, join_at=None, fuse_front=True):
    """A ForwardEngine over the weights pw = E.PackedWeights(cfg, state, dtype, "meta"), made without its constructor."""
    eng = object.__new__(E.ForwardEngine)
    eng.cfg, eng.crop_dim, eng.pw, eng.act_dtype, eng.device = cfg, None, pw, pw.act_dtype, "meta"
    eng.use_graph, eng.fuse_front, eng.n_split, eng.merge_tail, eng.join_at = False, fuse_front, n_split, merge_tail, join_at
    eng._plans = {}
    return eng


def plans(E, synth, state_layout, show_forms=False):
    log = []                                                      # pool events of the plan being built
    runs = []                                                     # (blocks, forms) of every run of bottlenecks in it
    take, give = E._Pool.take, E._Pool.give
    raw_index = lambda pool, t: next(i for i, b in enumerate(pool.all) if b is t._td_raw)   # noqa: E731

    def logged_take(pool, shape, dtype):
        t = take(pool, shape, dtype)
        log.append(("take", tuple(shape), str(dtype), raw_index(pool, t)))
        return t

    def logged_give(pool, t):
        log.append(("give", raw_index(pool, t)))
        give(pool, t)

    E._Pool.take, E._Pool.give = logged_take, logged_give
    patch_meta(E)
    if show_forms:
        block_forms = E.block_forms

        def logged_forms(blocks, *a):
            runs.append((blocks, block_forms(blocks, *a)))
            return runs[-1][1]
        E.block_forms = logged_forms

    weights = {}

    def engine(arch, n_layers, T, dt, **opt):
        cfg = config(arch, n_layers, T)
        if (arch, n_layers, T, dt) not in weights:
            sd = synth.make_state(state_layout.model_state_shapes(cfg), 3)
            weights[arch, n_layers, T, dt] = E.PackedWeights(cfg, sd, dt, "meta")
        return meta_engine(E, cfg, weights[arch, n_layers, T, dt], **opt)

    def show(label, dt, build):
        del log[:], runs[:]
        p = build()
        steps = [(s.name, s.kernel, s.bytes, s.flops) for s in p.steps]
        print(f"{label} {str(dt)[6:]}: steps {len(steps)} takes {sum(e[0] == 'take' for e in log)} "
              f"pool_bytes {p.pool_bytes} digest {digest((steps, log))}")
        if show_forms:
            for blocks, forms in runs:
                for bw, f in zip(blocks, forms):
                    print(f"    {bw.spec.name} " + " ".join(f"{k}={int(v)}" for k, v in f._asdict().items()))

    for (arch, n, T, B, S), opt, dt in itertools.product(GEOMETRIES, OPTIONS, DTYPES):
        show(f"{arch} n{n} T{T} B{B} {S}x{S} {opt}", dt, lambda: engine(arch, n, T, dt, **opt).plan(B, S, S))
    for dt in DTYPES:
        eng = engine("rny002_gsf", 2, 16, dt)
        show("flip + taps", dt, lambda: eng.plan(2, 224, 224, flip=True, taps=("_features.s3.b2", "_temp_fine._sgp.1")))
        show("stem tap", dt, lambda: eng.plan(2, 224, 224, taps=("_features.stem",)))
        flips = torch.zeros((2 * 16,), dtype=torch.uint8, device="meta")
        show("per-frame flips, fp32 frames 200x200", dt, lambda: eng._whole(2, 200, 200, flips, frames_dtype=torch.float32))
    # whole videos with the per-frame stages once per frame: the frame plan (blocks [0, k)) and the tail plan (blocks [k:] on)
    for (arch, n, T, B), dt in itertools.product([("rny002_gsf", 2, 100, 8), ("rny008_gsf", 3, 100, 8)], DTYPES):
        eng = engine(arch, n, T, dt)
        h, w, _ = eng.frame_map_shape(224, 224)
        show(f"{arch} n{n} T{T} frame plan Bf2 224x224 k{eng.first_site_block()}", dt, lambda: eng.frame_plan(2, 224, 224))
        show(f"{arch} n{n} T{T} tail plan B{B} {h}x{w}", dt, lambda: eng.tail_plan(B, h, w))


def tensors(obj, path=""):
    """every tensor reachable from obj (namespaces, lists, dicts, objects with attributes) with its path"""
    if isinstance(obj, torch.Tensor):
        yield path, obj
    elif isinstance(obj, np.ndarray):
        yield path, torch.from_numpy(np.ascontiguousarray(obj))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from tensors(v, f"{path}[{i}]")
    elif isinstance(obj, dict) or hasattr(obj, "__dict__"):
        for k, v in sorted((obj if isinstance(obj, dict) else vars(obj)).items()):
            if k != "spec":
                yield from tensors(v, f"{path}.{k}")


def tensor_digest(obj):
    return digest([(p, str(t.dtype), tuple(t.shape), hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest())
                   for p, t in tensors(obj)])


def weights(E, synth, state_layout, repack, regnet_spec):
    for arch, n in (("rny002_gsf", 2), ("rny008_gsf", 3), ("rny002_gsm", 2)):
        cfg = config(arch, n, 16)
        sd = synth.make_state(state_layout.model_state_shapes(cfg), 3)
        packed, on_device, ws = [], [], []
        on_device.append(E.stem_frags_on_device(torch.from_numpy(sd["_features.stem.conv.weight"])))
        for blk in regnet_spec(arch).blocks:
            bp = "_features." + blk.name
            c1 = bp + (".conv1.net" if blk.gsf_fold else ".conv1")
            dense = [sd[c1 + ".conv.weight"], sd[bp + ".conv3.conv.weight"]] + ([sd[bp + ".downsample.conv.weight"]] if blk.has_downsample else [])
            for w in dense:
                w = w.reshape(w.shape[0], -1)
                packed += [E.pack_ws_weights(w, torch.float32, "cpu"), E.pack_ws_weights(w, torch.bfloat16, "cpu"),
                           E.pack_mfma_frags(w, "cpu"), E.pack_mfma_frags(w, "cpu", rows=(w.shape[0] + 127) // 64 * 64),
                           E.pack_mfma_frags(w, "cpu", ks_mult=12)]
                if w.shape == (320, 320):
                    ws += [repack.pack_ws(torch.from_numpy(w)), repack.pack_ws(torch.from_numpy(w).t())]
            se = sd[bp + ".se.fc1.weight"], sd[bp + ".se.fc2.weight"]
            w2 = sd[bp + ".conv2.conv.weight"]
            packed += [E.pack_se_bf16(*se, "cpu"), E.pack_se_mfma(*se, "cpu"), E.pack_gconv_frags(w2, blk.gw, "cpu"),
                       E.pack_gconv_frags(w2, blk.gw, "cpu", tap_major=True)]
            on_device.append(E.gconv_frags_on_device(torch.from_numpy(w2), blk.gw))
            if blk.gsf_fold:
                w3d = sd[bp + ".conv1.gs.conv3D.weight"]
                packed += [E.pack_gsf_q_frags(w3d, "cpu"), E.pack_gsf_p_frags(w3d, "cpu"),
                           E.gs_source_order_columns(dense[0].reshape(blk.cout, blk.cin), blk.gsf_fold)]
                on_device.append(E.gsf_q_frags_on_device(torch.from_numpy(w3d)))
        b0 = regnet_spec(arch).blocks[0]
        g = lambda k: sd["_features." + k]                                                    # noqa: E731
        bn = lambda p: [g(p + ".weight"), g(p + ".bias")]                                     # noqa: E731
        p0 = b0.name
        packed.append(E.pack_front_weights(g("stem.conv.weight"), *bn("stem.bn"), g(p0 + ".conv1.conv.weight").reshape(b0.cout, b0.cin),
                                           *bn(p0 + ".conv1.bn"), g(p0 + ".downsample.conv.weight").reshape(b0.cout, b0.cin),
                                           *bn(p0 + ".downsample.bn"), g(p0 + ".conv2.conv.weight"), b0.gw, *bn(p0 + ".conv2.bn"), "cpu"))
        print(f"{arch}: packers {tensor_digest(packed)} on_device {tensor_digest(on_device)} pack_ws {tensor_digest(ws)} "
              + " ".join(f"PackedWeights {str(dt)[6:]} {tensor_digest(E.PackedWeights(cfg, sd, dt, 'cpu').W)}" for dt in DTYPES))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--plans", action="store_true")
    ap.add_argument("--forms", action="store_true", help="with --plans: every bottleneck's launch form under its plan's line")
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--variants", action="store_true", help="--plans once per plan switch, each in its own process")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="engine attribute set after import")
    a = ap.parse_args()
    if a.variants:
        for v in VARIANTS:
            env, sets = (v, []) if isinstance(v, dict) else ({}, v)
            print(f"== {' '.join(f'{k}={x}' for k, x in env.items()) or ' '.join(sets) or 'default'}", flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), a.tree, "--plans"] + [x for s in sets for x in ("--set", s)],
                           env=dict(os.environ, **env), check=True)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    import tdeed_amd  # noqa: F401
    from tdeed_amd import engine as E, repack, state_layout, synth
    from tdeed_amd.regnet_spec import regnet_spec
    for s in a.set:
        name, value = s.split("=")
        setattr(E, name, {"True": True, "False": False}[value])
    if a.plans:
        plans(E, synth, state_layout, a.forms)
    if a.weights:
        weights(E, synth, state_layout, repack, regnet_spec)


if __name__ == "__main__":
    main()
