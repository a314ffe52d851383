"""Operands of the SGP-stage rounding tests (test_roundoff_sgp_host.py, test_gpu_sgp_roundoff.py): every branch visible.
The goldens inherit the reference's initialisation (depthwise weights N(0, 0.1), biases 0), under which fc * phi is below one
bf16 ulp of the output; here the taps have scale 1 / sqrt(taps), fc and global_fc are of order 1, the biases of order 0.3 .. 1
with both signs, ln_b of order 0.5.  `check_front_conditions` asserts on the fp64 reference what the tests rely on."""
import torch

import roundoff as R
from helpers import act, t

BF = torch.bfloat16

# (B, T, C, ks, up)
FRONT_SHAPES = [(2, 13, 24, 5, 13), (2, 7, 40, 7, 33), (3, 25, 48, 7, 33), (1, 125, 32, 9, 41), (1, 250, 16, 11, 49),
                (2, 100, 368, 7, 33)]
MIXER_T = [(13, 7), (25, 13), (100, 50), (7, 4), (2, 1), (1, 1)]
GEMM_SHAPES = [(2, 13, 48), (1, 25, 368), (2, 34, 112), (1, 13, 768)]
# |mean| / std of the offset case of every normalising launch: the next power of two above the largest ratio the oracle's
# pyramid shows at a block or mixer input on the three pyramid goldens (2.32 over rows, 2.84 over groups: DESIGN section 2)
OFFSET_RATIO = 4.0


def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


def signed(seed, name, n, lo, hi):
    """magnitudes lo .. hi, both signs"""
    a = rnd(seed, name + "s", (n,))
    return (torch.where(a >= 0, 1.0, -1.0) * (lo + (hi - lo) * rnd(seed, name + "m", (n,)).abs().clamp(max=1.0))).float()


def branch_params(seed, name, C, ks, up):
    """dw (C, 2 ks + up + 2) = [psi | convw | convkw | fc | global_fc], db (5, C) in the layout of engine._dwpack"""
    dw = torch.cat([rnd(seed, name + "psi", (C, ks), ks ** -0.5), rnd(seed, name + "cw", (C, ks), ks ** -0.5),
                    rnd(seed, name + "ckw", (C, up), up ** -0.5), signed(seed, name + "fc", C, 0.5, 1.5).view(C, 1),
                    signed(seed, name + "g", C, 0.5, 1.5).view(C, 1)], 1).contiguous()
    db = torch.stack([signed(seed, name + f"b{i}", C, 0.3, 1.0) for i in range(5)]).contiguous()
    return dw.float(), db.float()


def ln_params(seed, name, C):
    return (1.0 + rnd(seed, name + "w", (C,), 0.2)).float(), signed(seed, name + "b", C, 0.25, 0.75)


def stream_input(seed, name, shape, dtype, offset=0.0):
    """unit-normal rows; offset: every row's and every group's mean is `offset` standard deviations from zero (the rows are
    standardised first, so that each row keeps var / E[x^2] = 1 / (1 + offset^2) whatever its sample statistics were)"""
    x = rnd(seed, name, shape)
    if offset:
        x = (x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True, unbiased=False)
        x = x + offset * torch.where(rnd(seed, name + "o", (shape[0], 1, 1)) >= 0, 1.0, -1.0)      # one sign per clip
    return x.to(dtype)


def pool_preimage(P, T_in, seed):
    """x (B, T_in, C) whose AdaptiveMaxPool1d is exactly P (B, T_out, C): every window has a row of its own that holds P's
    row, every other row lies below the rows of all windows it belongs to.  (The maximum of random rows moves their mean and
    narrows them; this is how the max-pool's offset case gets pooled rows with the |mean| / std it is about.)"""
    B, T_out, C = P.shape
    win = R.pool_windows(T_in, T_out)
    cover = [[i for i, (lo, hi) in enumerate(win) if lo <= t_ < hi] for t_ in range(T_in)]
    own = {}
    for i, (lo, hi) in enumerate(win):
        mine = [t_ for t_ in range(lo, hi) if cover[t_] == [i]]
        assert mine, (T_in, T_out, i)
        own[i] = mine[i % len(mine)]
    below = rnd(seed, "below", (B, T_in, C)).abs() + 0.05
    x = torch.empty(B, T_in, C)
    for t_ in range(T_in):
        base = torch.stack([P[:, i].float() for i in cover[t_]]).amin(0)
        x[:, t_] = base if own[cover[t_][0]] == t_ else base - below[:, t_] * base.abs().clamp_min(1.0)
    return x.to(P.dtype)


def rms(v):
    return float(v.double().pow(2).mean().sqrt())


def check_front_conditions(x, parts, name=""):
    """every branch visible, phi open on 20 .. 80 % of the channels, every row in the first-order regime"""
    figs = dict(x=rms(x), ln=rms(parts["ln"].ref), inst=rms(parts["inst"].ref), gate=rms(parts["gate"].ref))
    frac = R.relu_open(parts["phi"].ref)
    print(f"[conditions] {name}: rms " + ", ".join(f"{k} {v:.2f}" for k, v in figs.items()) + f", phi open on {frac:.2f}")
    for k, v in figs.items():
        assert 0.25 <= v <= 4.0, (name, k, v)
    assert 0.2 <= frac <= 0.8, (name, frac)
    st = parts["stats"]
    if st.var is not None:
        assert R.first_order(st) >= 1.0 / 32, (name, R.first_order(st))


def split_parts(full, n):
    """`full` as n parts with power-of-two weights (exact): what a producer with n tiles would hand over"""
    w = [2.0 ** -min(i + 1, n - 1) for i in range(n)] if n > 1 else [1.0]
    assert abs(sum(w) - 1.0) < 1e-12
    return torch.stack([full * wi for wi in w]).contiguous()


def row_sums(xf):
    """(rows, 2) fp32 (sum, sum of squares) over C of every row of x (B, T, C)"""
    xf = xf.float().reshape(-1, xf.shape[-1])
    return torch.stack([xf.sum(1), (xf * xf).sum(1)], -1).contiguous()


def row_mean_rstd(xf, eps=1e-5):
    """(rows, 2) fp32 (mean, rstd), computed in fp64 and rounded: what avgpool_posenc / maxpool_rowstat hand over"""
    xd = xf.double().reshape(-1, xf.shape[-1])
    m = xd.mean(1)
    return torch.stack([m, 1.0 / torch.sqrt((xd * xd).mean(1) - m * m + eps)], -1).float().contiguous()


def channel_sums(yf):
    """(B, C, 2) fp32 (sum, sum of squares) over T of y (B, T, C)"""
    yf = yf.float()
    return torch.stack([yf.sum(1), (yf * yf).sum(1)], -1).contiguous()


def gemm_operands(seed, B, T, K, N, adt, offset=0.0):
    """rows of type adt, weights rounded to bf16 before packing, biases of order 0.3 .. 1, a GroupNorm affine"""
    y = stream_input(seed, f"y{B}x{T}x{K}", (B, T, K), adt, offset)
    W = R.bf16_weights(rnd(seed + 1, f"W{N}x{K}", (N, K), K ** -0.5))
    bias = signed(seed + 2, f"b{N}", N, 0.3, 1.0)
    gw, gb = (1.0 + rnd(seed + 3, f"gw{K}", (K,), 0.2)).float(), signed(seed + 4, f"gb{K}", K, 0.1, 0.5)
    return y, W, bias, gw, gb
