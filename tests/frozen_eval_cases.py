"""Cases and CPU references of the frozen eval-mode prefix (tests/test_frozen_eval_host.py, tests/test_gpu_frozen_eval.py).

The expected values are the CPU oracle composed per stage: `O._conv_bn` for the stem and `O.regnet_block` per block with
training=False inside the prefix and training=True behind it (torch's .eval() on the frozen sub-modules), then temp_enc,
`O.ed_sgp_mixer`, `O.heads` and `O.loss_fn` as helpers.oracle_train_loss composes them.  Each reference is computed once per
case and left unchanged.  CPU torch only; no GPU, no kernel."""
import functools

import torch

from helpers import drop_masks, t
from tdeed_amd import synth, state_layout
from tdeed_amd.regnet_spec import regnet_spec

# the configuration of tests/test_gpu_param_groups.py: 200MF gsf, clip_len 6, B = 2, 64 x 64, state seed 17
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
SEED = 17
B = 2
# freeze sets whose eval prefix is the whole set: the stem alone; stem + s1; stem + s1 + s2 (the cut in front of the first
# gate-shift block); a cut between two gate-shift blocks of s3; the whole trunk
PREFIXES = {
    "stem": ("_features.stem.*",),
    "s1": ("_features.stem.*", "_features.s1.*"),
    "s2": ("_features.stem.*", "_features.s1.*", "_features.s2.*"),
    "s3mid": ("_features.stem.*", "_features.s1.*", "_features.s2.*", "_features.s3.b1.*", "_features.s3.b2.*"),
    "trunk": ("_features.*",),
}
# (H, W, crop, per-clip flip flags | False): the second geometry is a crop of 64 x 80 frames with one clip of two flipped
GEOMS = {"full": (64, 64, None, False), "crop": (64, 80, (8, 16, 48, 48), (True, False))}


def groups(prefix):
    return [{"params": PREFIXES[prefix], "frozen": True}]


def start_state():
    return {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), SEED).items()}


def batch(geom, rank=0):
    H, W, _, _ = GEOMS[geom]
    T = CFG["clip_len"]
    frames = t(synth.uint8_clip(1300 + rank, (B, T, 3, H, W)))
    lab, labD = synth.labels(1400 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
    return frames, t(lab).long(), t(labD).float()


def masks():
    spec = regnet_spec(CFG["feature_arch"])
    return drop_masks(77, B, CFG["clip_len"], spec.feat_dim, 2)


def n_eval_stages(prefix):
    """how many forward stages (the stem counts) the freeze set's eval prefix holds"""
    from tdeed_amd.optim import eval_prefix, frozen_keys
    spec = regnet_spec(CFG["feature_arch"])
    keys = [k for k in state_layout.model_state_shapes(CFG) if state_layout.is_parameter(k)]
    return len(eval_prefix(spec, frozen_keys(keys, groups(prefix)), keys))


def oracle_forward(frames, sd, n_eval, lab, labD, drop, crop=None, flip_clips=False):
    """The composition of the module docstring.  n_eval: forward stages in eval mode (0: the plain train-mode forward).
    Returns (loss, the input map of the first train-mode stage NCHW -- the trunk's output when every stage is in eval mode)."""
    from oracle import tdeed_oracle as O
    spec = regnet_spec(CFG["feature_arch"])
    x = frames.float() / 255.0
    if crop is not None:
        top, left, ch, cw = crop
        x = x[..., top:top + ch, left:left + cw]
    if flip_clips:
        x = torch.stack([xi.flip(-1) if f else xi for xi, f in zip(x, flip_clips)], 0)
    mean = torch.tensor(O.IMAGENET_MEAN).view(1, 1, 3, 1, 1)
    std = torch.tensor(O.IMAGENET_STD).view(1, 1, 3, 1, 1)
    x = (x - mean) / std
    Bn, T = x.shape[:2]
    x = x.reshape(Bn * T, *x.shape[2:])
    x = O._conv_bn(x, sd, "_features.stem", stride=2, training=n_eval < 1)
    outs = [x]                                                   # outs[s]: the output of forward stage s (0: the stem)
    for i, blk in enumerate(spec.blocks):
        x = O.regnet_block(x, sd, "_features." + blk.name, blk, T, "gsf", training=i + 1 >= n_eval)
        outs.append(x)
    cut = outs[n_eval - 1].detach() if n_eval > 0 else None
    f = x.mean(dim=(2, 3)).reshape(Bn, T, -1) + sd["temp_enc"][None]
    enc = O.ed_sgp_mixer(f, sd, CFG["n_layers"], CFG["clip_len"])
    cls, displ = O.heads(enc, sd, CFG["radi_displacement"], drop_mask=(drop[1], drop[0]))
    return O.loss_fn(cls, lab, displ, labD), cut


@functools.lru_cache(maxsize=None)
def reference(prefix, geom):
    """Autograd on the composition for one (freeze set, geometry), computed once: dict(loss, grads {trainable name: grad},
    cut (block k's input map, NHWC), bn (the BatchNorm buffers the train-mode stages leave: O.BN_UPDATES), frozen)."""
    from oracle import tdeed_oracle as O
    from tdeed_amd.optim import frozen_keys
    sd0 = start_state()
    par = [k for k in sd0 if state_layout.is_parameter(k)]
    frozen = frozen_keys(par, groups(prefix))
    train = [k for k in par if k not in frozen]
    sdr = {k: (v.clone().requires_grad_(True) if k in train else v.clone()) for k, v in sd0.items()}
    sdr[O.BN_UPDATES] = {}
    frames, lab, labD = batch(geom)
    _, _, crop, flips = GEOMS[geom]
    loss, cut = oracle_forward(frames, sdr, n_eval_stages(prefix), lab, labD, masks(), crop, flips)
    loss.backward()
    return dict(loss=float(loss.detach()), grads={k: sdr[k].grad.detach().clone() for k in train},
                cut=cut.permute(0, 2, 3, 1).contiguous(), bn={k: v.detach().clone() for k, v in sdr[O.BN_UPDATES].items()},
                frozen=frozen, train=train)


# ----------------------------------------------------------------------------- the eval instance of the MFMA stem, alone
# (frames, H, W, crop): a ragged last tile column and 112 rows in bands of 16; a short last row band behind a crop; unaligned
# crop offsets with an odd window
STEM_GEOMS = [(6, 224, 224, None), (5, 96, 128, (8, 16, 80, 96)), (3, 70, 90, (3, 5, 61, 75))]


@functools.lru_cache(maxsize=None)
def stem_case(gi, f32_frames):
    """Operands and the fp64 reference with its bound for STEM_GEOMS[gi]: uint8 frames or fp32 0..255 frames (a mixup of two
    clips: non-integer values), alternating per-frame flip flags, a fold with scales of both signs (roundoff.fold).
    The bound is roundoff's for conv2d(normalised frames, w, 2, sc, sh) -> relu -> store_bf16 with the operand error of
    tests/test_gpu_bf16_anchors.py::test_stem_mfma: input and weight are split into a bf16 head and tail and the tail x tail
    product is dropped, 3 * 2^-18 < 2^-16 of each term, carried as the input's error.  fp32 frames: the kernel's
    fmaf(u, na, nb) rounds once, the emulation below rounds u * na + nb to fp64 first, which can move the fp32 value by one
    ulp: 2^-23 of it more.
    -> dict(frames, w, sc, sh, flips (N,) uint8, crop, ref: RB in NHWC, x32: the normalised fp32 input NCHW)."""
    import numpy as np
    import roundoff as R
    from helpers import act
    N, H, W, crop = STEM_GEOMS[gi]
    fr = t(synth.uint8_clip(2100 + gi, (N, 3, H, W)))
    if f32_frames:
        other = t(synth.uint8_clip(2200 + gi, (N, 3, H, W)))
        fr = (fr.float() * np.float32(0.6) + other.float() * np.float32(0.4)).contiguous()
    flips = torch.tensor([i % 2 for i in range(N)], dtype=torch.uint8)
    w = t(act(2300, "w", (32, 3, 3, 3), 0.3))
    sc, sh = R.fold(2301, "stemfold", 32)
    assert int((sc < 0).sum()) >= 4 and int((sc > 0).sum()) >= 4
    plain, flipped = R.normalised_bf16(fr, crop, False)[1], R.normalised_bf16(fr, crop, True)[1]
    x32 = torch.where(flips.bool().view(N, 1, 1, 1), flipped, plain)
    rel = 2.0 ** -16 + (2.0 ** -23 if f32_frames else 0.0)
    x = R.RB(x32.double(), rel * x32.double().abs())
    ref = R.permute(R.store_bf16(R.relu(R.conv2d(x, w, 2, 1, sc, sh))), 0, 2, 3, 1)
    return dict(frames=fr, w=w, sc=sc, sh=sh, flips=flips, crop=crop, ref=ref, x32=x32)
