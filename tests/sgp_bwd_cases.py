"""Operands of the backward rounding tests of the temporal stage (test_roundoff_sgp_bwd_host.py, test_gpu_sgp_bwd_roundoff.py).
Inputs are those of sgp_cases.py (unit-normal rows, one offset case at OFFSET_RATIO, every branch of the depthwise stage
visible), gradients are unit normal in the stream's type.  `check_norm_conditions` and `check_branch_conditions` assert on the
fp64 reference what the tests rely on.  The weight-gradient forms get EXACT operands next to the random ones: m / 4 with
integer |m| <= 15, so every product is a multiple of 2^-4 of at most 14.1, every partial sum over M <= 70 000 rows an fp32
number (< 2^20 in steps of 2^-4: 24 bits), and the fp32 accumulation exact in any order."""
import numpy as np
import torch

import roundoff as R
import sgp_cases as S
from helpers import synth

BF, F32 = torch.bfloat16, torch.float32

# (rows, C): 24 = three bf16 chunks in one lane round and the smallest C for the unbiased-variance defect; (520, 40): 65
# workgroups, the wide reduce_partials form; (64, 768): the second chunk round of the bf16 instance, the third of the fp32 one
LN_SHAPES = [(7, 24), (77, 32), (200, 368), (520, 40), (64, 768)]
# (B, T, C), G = 16: 23 channels per group; the 96 KB slab (the raised dynamic LDS limit); 3 channels per group
GN_SHAPES = [(3, 25, 32), (2, 13, 368), (1, 250, 768), (2, 7, 48)]
GN_G = 16
GN_OFFSET_SHAPE = (2, 13, 368)     # 299 values per group: the small groups of (2, 7, 48) leave the first-order regime there
BRANCH_SHAPES = S.FRONT_SHAPES[:5]
UPSAMPLE_T = S.MIXER_T + [(250, 125)]
POOL_T = [(25, 13), (100, 50), (125, 63), (7, 4), (13, 13)]
# a window of one row (13 -> 13) has no preimage other than the row itself: quarters only
POOL_CASES = [(a, b, how) for a, b in POOL_T for how in ("quarters", "preimage") if not (how == "preimage" and a == b)]
ELTWISE_N = [8, 8 * 257, 64 * 96]
# (kernel, M, N, K, bias, k0): every dispatch branch of tdeed_wgrad.  k0: the X0 splice (0: none)
WGRAD_CASES = [("wgrad_kernel_f32", 37, 24, 40, True, 0), ("wgrad_kernel_f32", 100, 12, 20, True, 0),
               ("wgrad_kernel_bf16", 100, 12, 20, True, 0),         # N % 8 != 0: (37, 24, 40) in bf16 is the MFMA form's
               ("wgrad_mfma", 37, 24, 40, True, 0), ("wgrad_mfma", 1000, 72, 136, True, 0),
               ("wgrad_tr", 4096, 24, 40, True, 0), ("wgrad_tr", 4099, 152, 56, True, 0), ("wgrad_tr", 4099, 152, 56, True, 8),
               ("wgrad_tr", 4099, 152, 56, True, 56),
               ("wgrad_tr128", 4099, 96, 104, True, 0), ("wgrad_tr128", 4160, 136, 264, True, 0),
               ("wgrad_tr128", 4099, 320, 320, True, 0), ("wgrad_tr128", 4099, 320, 320, True, 80),
               ("wgrad_tr160", 4099, 320, 320, False, 0), ("wgrad_tr160", 4099, 320, 320, False, 80)]


def wgrad_id(case):
    kern, M, N, K, bias, k0 = case
    return f"{kern}-{M}x{N}x{K}" + ("-bias" if bias else "") + (f"-splice{k0}" if k0 else "")


def wgrad_dtype(case):
    return F32 if case[0].endswith("f32") else BF


def wgrad_branch(M, N, K, dt, bias):
    """the dispatch of tdeed_wgrad (sgp_bwd.hip), restated: which kernel serves the case"""
    if dt == F32:
        return "wgrad_kernel_f32"
    if not (N % 8 == 0 and K % 8 == 0):
        return "wgrad_kernel_bf16"
    if M >= 4096 and N == 320 and K == 320 and not bias:
        return "wgrad_tr160"
    if M >= 4096 and N >= 96 and K >= 96:
        return "wgrad_tr128"
    return "wgrad_tr" if M >= 4096 else "wgrad_mfma"


def grad(seed, name, shape, dt):
    return S.rnd(seed, name, shape).to(dt)


def exact_operand(seed, name, shape, dt):
    """m / 4, integer |m| <= 15: exact in bf16 and fp32"""
    n = int(np.prod(shape))
    m = np.clip(np.rint(synth.normalish(seed, name, n) * 6.0), -15, 15)
    return torch.from_numpy((m / 4.0).astype(np.float32).reshape(shape)).to(dt)


def wgrad_operands(case, exact, seed=131):
    """-> dY (M, N), X (M, K), X0 (M, k0) or None, base (dW, db) for `accumulate`"""
    kern, M, N, K, bias, k0 = case
    dt = wgrad_dtype(case)
    assert wgrad_branch(M, N, K, dt, bias) == kern, (case, wgrad_branch(M, N, K, dt, bias))
    make = exact_operand if exact else (lambda s, n, shp, d: S.rnd(s, n, shp).to(d))
    dY, X = make(seed, f"dY{M}x{N}", (M, N), dt), make(seed + 1, f"X{M}x{K}", (M, K), dt)
    X0 = make(seed + 2, f"X0{M}x{k0}", (M, k0), dt) if k0 else None
    base = (exact_operand(seed + 3, f"bW{N}x{K}", (N, K), F32), exact_operand(seed + 4, f"bb{N}", (N,), F32))
    return dY, X, X0, base


# ----------------------------------------------------------------------------- normalisation backward
def ln_bwd_case(rows, C, dt, offset=0.0, accumulate=False):
    """-> x, dy (rows, C), w (C), base (rows, C) or None"""
    x = S.stream_input(141, f"x{rows}x{C}", (1, rows, C), dt, offset).view(rows, C)
    dy = grad(142, f"dy{rows}x{C}", (rows, C), dt)
    return x, dy, S.ln_params(143, f"ln{C}", C)[0], (grad(144, f"b{rows}x{C}", (rows, C), dt) if accumulate else None)


def gn_bwd_case(B, T, C, dt, offset=0.0, accumulate=False):
    x = S.stream_input(151, f"x{B}x{T}x{C}", (B, T, C), dt, offset)
    dy = grad(152, f"dy{B}x{T}x{C}", (B, T, C), dt)
    w = (1.0 + S.rnd(153, f"gw{C}", (C,), 0.2)).float()
    return x, dy, w, (grad(154, f"b{B}x{T}x{C}", (B, T, C), dt) if accumulate else None)


def check_norm_conditions(st, name=""):
    fo = R.first_order(st)
    print(f"[conditions] {name}: smallest var / E[x^2] {fo:.3f}")
    assert fo >= 1.0 / 32, (name, fo)


# ----------------------------------------------------------------------------- depthwise-branch backward
def branch_bwd_case(shape, dt, slabs=False):
    """-> o, (g_conv, g_inst, g_id), dw, db.  slabs: the mixer's call -- o is slab 4 of a (B, T, 6C) tensor, the gradients are
    slabs 0, 2, 4 of another, all on the row stride 6C (temporal_train.py, mixer_bwd); else one gradient in all three roles"""
    B, T, C, ks, up = shape
    dw, db = S.branch_params(163, f"dw{C}", C, ks, up)
    if not slabs:
        o = S.stream_input(161, f"o{shape}", (B, T, C), dt)
        g = grad(162, f"g{shape}", (B, T, C), dt)
        return o, (g, g, g), dw, db
    cat = S.stream_input(164, f"cat{shape}", (B, T, 6 * C), dt)
    dcat = grad(165, f"dcat{shape}", (B, T, 6 * C), dt)
    sl = lambda v, i: v[..., i * C:(i + 1) * C]                                # noqa: E731
    return (cat, dcat), (sl(cat, 4), (sl(dcat, 0), sl(dcat, 2), sl(dcat, 4))), dw, db


def check_branch_conditions(parts, unsure, T, name=""):
    """phi open on 20 .. 80 % of the channels and none within its own error of the ReLU's kink; every term of d_o visible.
    The dmean term is dpre wg / T with dpre a sum of T products of unit-normal gradients, so its rms goes like 1 / sqrt(T):
    dmean sqrt(T) is the T-free figure held to 0.25 .. 4 (dmean T is 2.2 at T = 7 and 13 at T = 250 for ANY unit-normal
    gradient), and dmean itself must stand above the bf16 rounding of d_o: rms(dmean) >= 4 * 2^-8 rms(d_o)"""
    frac = R.relu_open(parts["pre"].ref)
    figs = dict(identity=S.rms(parts["identity"]), inst=S.rms(parts["inst"]), gate=S.rms(parts["gate"]),
                dmean_sqrtT=S.rms(parts["dmean"]) * T ** 0.5)
    d_o = S.rms(parts["identity"] + parts["inst"] + parts["gate"] + parts["dmean"].unsqueeze(1))
    print(f"[conditions] {name}: rms " + ", ".join(f"{k} {v:.2f}" for k, v in figs.items()) +
          f", dmean T {S.rms(parts['dmean']) * T:.2f}, d_o {d_o:.2f}, phi open on {frac:.2f}, {unsure} within d_pre of the kink")
    assert unsure == 0, (name, unsure)
    assert 0.2 <= frac <= 0.8, (name, frac)
    for k, v in figs.items():
        assert 0.25 <= v <= 4.0, (name, k, v)
    assert S.rms(parts["dmean"]) >= 4 * R.U_BF16 * d_o, (name, S.rms(parts["dmean"]), d_o)


# ----------------------------------------------------------------------------- up-sampling, max-pool, element-wise
def upsample_bwd_case(T_hi, T_lo, dt, B=2, C=24, wide=False):
    """-> d_xu (B, T_hi, C); wide: slab 5 of a (B, T_hi, 6C) tensor (ld = 6C)"""
    if wide:
        return grad(171, f"w{T_hi}", (B, T_hi, 6 * C), dt)[..., 5 * C:]
    return grad(171, f"g{T_hi}", (B, T_hi, C), dt)


def maxpool_bwd_case(T_in, T_out, dt, how, B=2, C=24):
    """how 'quarters': x quantised to quarters, so that ties occur inside windows; 'preimage': sgp_cases.pool_preimage"""
    dy = grad(182, f"dy{T_out}", (B, T_out, C), dt)
    if how == "quarters":
        x = (S.rnd(181, f"x{T_in}", (B, T_in, C)) * 2.0).round() / 4.0
        return x.to(dt), dy
    P = S.stream_input(183, f"P{T_out}", (B, T_out, C), dt)
    return S.pool_preimage(P, T_in, 184), dy


def count_ties(x, T_out):
    """windows whose maximum is attained more than once"""
    xx = R.f64(x)
    return sum(int(((xx[:, lo:hi] == xx[:, lo:hi].amax(1, keepdim=True)).sum(1) > 1).sum())
               for lo, hi in R.pool_windows(xx.shape[1], T_out))


def eltwise_case(n, dt):
    return S.rnd(191, f"x{n}", (n,), 1.5).to(dt), grad(192, f"dy{n}", (n,), dt)
