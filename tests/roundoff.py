"""fp64 references of the bf16 kernels together with a first-order bound on what a correct kernel may differ from them.

A value travels as a pair (ref, d): `ref` is the operation in fp64 on the operands exactly as the kernel receives them
(bf16 activations, the weights its pack function stores), `d >= 0` has the same shape and bounds |kernel value - ref| for a
kernel that accumulates in fp32 and rounds to bf16 (to nearest, ties to even) exactly where its header says it does.
Every term is derived, none is fitted to a kernel's output:

  contraction + affine   y = sc (W x) + sh + r, K terms per output element
                         d_y = |sc| (|W| d_x) + d_r + (K + 4) 2^-23 (|sc| (|W| |x|) + |sh| + |r|)
                         the second term is the fp32 accumulation bound K 2^-24 (+ the three roundings of the epilogue),
                         doubled: an accumulator that truncates its adds, or sums in any order (split-K workspaces, MFMA
                         internal order), stays inside it
  stored as bf16         d_y += 2^-8 (|y| + d_y)        2^-8 = unit roundoff of bf16 under round-to-nearest-even
  ReLU                   d unchanged (1-Lipschitz)
  GELU                   d *= 1.13 (its Lipschitz constant: max |gelu'| = 1.129), + the fp32 transcendental term
  sigmoid                d *= 0.25, + the fp32 transcendental term
  fp32 transcendental    d += 16 2^-24 (|x| + |f(x)|).  The 16 is not tuned: an fp32-grade erff / exp2 / rcp is good to about
                         2^-21, a bf16-grade defect is 2^-8, three orders of magnitude apart, so anything from 4 to 64
                         separates them (torch's own fp32 gelu on the CPU uses 0.3 of the term: test_roundoff_host.py).

The SGP stage (sgp_fused.hip, sgp_tile.h, sgp_gemm.hip, sgp.hip) adds, with u = 2^-24:

  product                d(ab) = |a| d_b + |b| d_a + d_a d_b + u |ab|
  sum of n values        d = sum d_i + n 2^-23 sum |v_i|                 (the fp32 summation bound n u, doubled as above)
  depthwise conv over T  zero padding, K taps in one fp32 fma chain: the contraction rule with K = number of taps
  mean over T            d = mean d + (T + 4) 2^-23 mean |x|
  linear up-sampling     align_corners=True: l0 x[i0] + l1 x[i1] is a two-term contraction; the position scale * t is an fp32
                         product of an fp32 quotient, off by at most T_hi 2^-23, which moves the value by that times the
                         steepest of the segment's and its two neighbours' slopes (the position may cross a node)
  max-pool               d = max of d over the window (exact on exact inputs)
  LayerNorm / GroupNorm  one pass in fp32: s = sum x, q = sum x^2 over n values carry the doubled summation bound,
                         m = s / n (+ u |m|), var = max(q/n - m^2, 0) with d_var = d_q/n + 2 |m| d_m + d_m^2 + 3 u (q/n + m^2)
                         (the cancellation term: three roundings of magnitude q/n, m^2 and their difference),
                         rstd = 1 / sqrt(var + eps) with d_rstd / rstd = d_var / (2 (var + eps)) + 2 u, then through
                         (x - m) rstd w + b; the rounding term 4 2^-23 (rstd |w| (|x| + |m|) + |b|) is that of the table form
                         fmaf(x, rstd w, fmaf(-m, rstd w, b)) of sgp_gemm.hip, which the direct forms stay inside
  handed statistics      (mean, rstd) pairs, chsum parts and rowstat partial sums are exact operands, in fp64: only the
                         arithmetic behind them carries error -- the ordered sum of the parts (doubled summation bound over
                         the number of parts), q/n - m^2, the rsqrt
  GELU of sgp_gemm.hip   Abramowitz-Stegun 7.1.26 with rcpf and exp2f: |err| <= 1.5e-7 on erf is 0.75e-7 |x| on the output; rcpf
                         and exp2f are good to 2^-23 relative, rcpf's error reaches erf through t poly'(t) / poly(t) <= 3.5, the
                         five fmas of the Horner form add 5 u of partial sums <= 1.5: together below 1.3e-6 on erf, 6.5e-7 |x| on
                         the output, inside the existing transcendental term 16 u (|x| + |f(x)|) >= 9.5e-7 |x|
                         (test_roundoff_sgp_host.py measures it, with both intrinsics pushed one ulp either way)

The temporal stage's backward kernels (sgp_bwd.hip) add, all operands exact (a launch receives bf16 or fp32 tensors as they are):

  normalisation backward two passes in fp32: m = s / n as above, then q = sum (x - m_k)^2 around the KERNEL's mean m_k.  Exactly
                         sum (x - m_k)^2 = sum (x - m)^2 + n (m_k - m)^2, so the mean's error moves var by at most d_m^2; the
                         rounding of the differences, squares, the sum and the division is (n + 4) 2^-23 var: no cancellation
                         term of magnitude E[x^2] (moments()' one-pass d_var is an upper bound of this).  xhat = (x - m) rstd:
                         d_xhat = rstd (d_m + u |x - m|) + |x - m| d_rstd + u |xhat|.  g = dy w (u |g|), s1 = mean g and
                         s2 = mean g xhat carry the doubled summation bound over n terms, inner = g - s1 - xhat s2 the
                         cancellation term 4 2^-23 (|g| + |s1| + |xhat s2|), dx = rstd inner:
                         d_dx = rstd d_inner + |inner| d_rstd + u |dx|; `accumulate` adds the old value in fp32 (one more
                         add) IN FRONT OF the one rounding of the store.  The parameter sums dw = sum dy xhat, db = sum dy are
                         fp32 sums over `rows` terms in any order (per wave, per workgroup, reduce_partials):
                         sum |dy| d_xhat + rows 2^-23 sum |dy xhat|
  depthwise branch       the forward products again (dwconv, scale_shift, mean_T above), d psi = g (cw + ckw), d s = g psi by the
                         product rule, the input gradient one fma chain over 3 + 2 ks + up terms (contraction rule), sums over
                         T and over the clips by the summation rule.  The ReLU gate of phi is discontinuous: the bound holds
                         for channels with |pre| > d_pre, `branch_bwd_ref` counts the others and the tests assert there are none
  up-sampling backward   the transpose of the forward: a gather over T_hi with the weights 1 - l1, l1.  The fp32 position is off
                         by at most T_hi 2^-23, which moves both weights by that much, and, where the position lies that close
                         to a node, moves the contribution to the node on the other side of it
  max-pool backward      the first maximum of a window takes its gradient (exact operands: exact ties); an input collects at
                         most 3 windows: the summation rule
  GELU backward          dy (cdf + x pdf): the transcendental term on |x|, |cdf| and |x pdf| (erff, expf), times |dy|
  weight gradient        dW = dY^T X is the contraction rule with K = M rows, db an M-term sum, `accumulate` one more add.  At
                         M >= 4096 the worst case (M + 4) 2^-23 sum |a| |b| is about 2 % of a typical element: no defect hides
                         from BIT EQUALITY on exact operands instead (sgp_bwd_cases.exact_operand: every partial sum an fp32
                         number, so the accumulation is exact in any order, on MFMA or VALU, through any number of slices)

The first-order rule for rstd FAILS as var -> 0 (d_var / (var + eps) is no longer small, and with q/n >> var the cancellation
term alone exceeds var): the bound is stated for rows and groups with var >= E[x^2] / 32, which `first_order` returns and the
tests assert on every reference.

CPU torch / numpy in fp64 only; no GPU, no kernel."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from helpers import act, t

U_BF16 = 2.0 ** -8          # unit roundoff of bf16, round to nearest even
U_F32 = 2.0 ** -24
TRANSCENDENTAL = 16         # see the module docstring
GELU_LIP = 1.13
BF = torch.bfloat16

RB = namedtuple("RB", "ref d")      # reference value and bound, fp64 CPU tensors of one shape


def f64(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.detach().cpu().to(torch.float64)


def exact(x):
    """an operand the kernel receives as it is (a bf16 activation, a uint8 frame): no error"""
    x = f64(x)
    return RB(x, torch.zeros_like(x))


def bf16_weights(w):
    """the values a pack function that ends in a bf16 cast stores (packing._bf16 / _dense): w rounded to bf16, as fp32"""
    w = w if isinstance(w, torch.Tensor) else t(w)
    return w.float().to(BF).float()


# ----------------------------------------------------------------------------- operands
def fold(seed, name, n, shift_scale=1.0):
    """a random BatchNorm fold (the _fold of test_gpu_s1_conv3_in_c1g): scales of both signs with magnitude 0.5 .. 1.5,
    shifts of order 1 and different in every channel -- a neighbour's table entry cannot hide under them"""
    a = t(act(seed, name + "s", (n,)))
    sc = torch.where(a >= 0, 1.0, -1.0) * (0.5 + t(act(seed, name + "m", (n,))).abs().clamp(max=1.0))
    return sc.float(), (t(act(seed, name + "h", (n,))) * shift_scale).float()


def relu_open(ref):
    """fraction of outputs on which the ReLU in front of `ref` is open"""
    return float((ref > 0).double().mean())


# ----------------------------------------------------------------------------- propagation
def _affine(lin, lin_d, lin_mag, K, sc, sh, res, cdim):
    """y = sc * lin + sh + res along channel dim `cdim`; lin_d = |W| d_x, lin_mag = |W| |x|"""
    shape = [1] * lin.dim()
    shape[cdim] = -1
    sc = torch.ones(lin.shape[cdim], dtype=torch.float64) if sc is None else f64(sc)
    sh = torch.zeros(lin.shape[cdim], dtype=torch.float64) if sh is None else f64(sh)
    sc, sh = sc.view(shape), sh.view(shape)
    y = sc * lin + sh
    mag = sc.abs() * lin_mag + sh.abs()
    d = sc.abs() * lin_d
    if res is not None:
        y = y + res.ref
        mag = mag + res.ref.abs()
        d = d + res.d
    return RB(y, d + (K + 4) * 2.0 ** -23 * mag)


def contraction(x, W):
    """(W x, |W| d_x, |W| |x|, K) of x (M, K) . W (N, K)^T: shared by the epilogue forms of one operand pair"""
    W = f64(W)
    return x.ref @ W.T, x.d @ W.abs().T, x.ref.abs() @ W.abs().T, W.shape[1]


def affine(c, sc=None, sh=None, res=None):
    """per-column affine (+ residual RB) behind a contraction()"""
    return _affine(c[0], c[1], c[2], c[3], sc, sh, res, 1)


def linear(x, W, sc=None, sh=None, res=None):
    """x (M, K) . W (N, K)^T, per-column affine, optional residual RB (M, N)"""
    return affine(contraction(x, W), sc, sh, res)


def permute(v, *dims):
    return RB(v.ref.permute(*dims).contiguous(), v.d.permute(*dims).contiguous())


def reshape(v, *shape):
    return RB(v.ref.reshape(*shape), v.d.reshape(*shape))


def conv2d(x, w, stride, groups=1, sc=None, sh=None):
    """x (N, C, H, W) NCHW, 3 x 3, padding 1; per-channel affine"""
    w = f64(w)
    cv = lambda a, k: F.conv2d(a, k, stride=stride, padding=1, groups=groups)      # noqa: E731
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return _affine(cv(x.ref, w), cv(x.d, w.abs()), cv(x.ref.abs(), w.abs()), K, sc, sh, None, 1)


def store_bf16(v):
    """a rounding point: the value is kept as bf16 from here on"""
    return RB(v.ref, v.d + U_BF16 * (v.ref.abs() + v.d))


def _transcendental(x, fx):
    return TRANSCENDENTAL * U_F32 * (x.abs() + fx.abs())


def relu(v):
    return RB(torch.relu(v.ref), v.d)


def gelu(v):
    """gelu_erf of common.h: 0.5 x (1 + erf(x / sqrt 2)) with fp32 erff"""
    fx = 0.5 * v.ref * (1.0 + torch.erf(v.ref * 0.70710678118654752440))
    return RB(fx, GELU_LIP * v.d + _transcendental(v.ref, fx))


def sigmoid(v):
    fx = torch.sigmoid(v.ref)
    return RB(fx, 0.25 * v.d + _transcendental(v.ref, fx))


def activation(v, actn):
    return [lambda a: a, relu, gelu][actn](v)


def scaled_operand_bf16(A, gate, rows):
    """the operand under a_scale as the gemm kernels build it (gemm.hip lstore / gemm_ws staging): bf16 -> fp32, ONE fp32
    multiply by the frame's gate, one rounding back to bf16.  Both steps are IEEE operations, so the operand is emulated
    exactly (fp32 multiply, bf16 cast) and carries no error; a kernel that does not round it is outside the bound."""
    M, K = A.shape
    g = gate.float().repeat_interleave(rows, dim=0)[:M]
    return exact((A.float() * g).to(BF))


def normalised_bf16(frames_u8, crop=None, flip=False):
    """the normalised input patch of front.hip (s1_front / stem_mfma): fmaf(u, na, nb) with the fp32 constants
    na = 1 / (255 std), nb = -mean / std as the kernel folds them, rounded to fp32 (the fma) and then to bf16.  u * na + nb is
    exact in fp64 (8 + 24 bits), so the two casts below are the kernel's two roundings.  Returns (bf16 patch, fp32 value)."""
    f32 = np.float32
    mean, std = [f32(0.485), f32(0.456), f32(0.406)], [f32(0.229), f32(0.224), f32(0.225)]
    na = np.array([f32(1.0) / (f32(255.0) * s) for s in std], dtype=np.float32)
    nb = np.array([-m / s for m, s in zip(mean, std)], dtype=np.float32)
    u = frames_u8.detach().cpu().numpy().astype(np.float64)
    if crop is not None:
        u = u[..., crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
    if flip:
        u = u[..., ::-1]
    v32 = (u * na.astype(np.float64).reshape(1, 3, 1, 1) + nb.astype(np.float64).reshape(1, 3, 1, 1)).astype(np.float32)
    v32 = torch.from_numpy(np.ascontiguousarray(v32))
    return v32.to(BF), v32


def normalised_f32(frames_u8, crop=None, flip=False):
    """the VALU stem's input (conv.hip stem_kernel): (u / 255 - mean) / std in fp32 -- three roundings (a division, a
    subtraction of magnitude <= u/255 + mean, a division), each 2^-24 of its result; 4 2^-24 covers them"""
    mean = torch.tensor(np.array([0.485, 0.456, 0.406], np.float32)).double().view(1, 3, 1, 1)
    std = torch.tensor(np.array([0.229, 0.224, 0.225], np.float32)).double().view(1, 3, 1, 1)
    u = f64(frames_u8)
    if crop is not None:
        u = u[..., crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
    if flip:
        u = u.flip(-1)
    return RB((u / 255.0 - mean) / std, 4 * U_F32 * (u / 255.0 + mean) / std)


# ----------------------------------------------------------------------------- the SGP stage: element-wise pieces
def product(a, b):
    ab = a.ref * b.ref
    return RB(ab, a.ref.abs() * b.d + b.ref.abs() * a.d + a.d * b.d + U_F32 * ab.abs())


def total(*vs):
    """fp32 sum of the values, in any order"""
    ref, d, mag = sum(v.ref for v in vs), sum(v.d for v in vs), sum(v.ref.abs() for v in vs)
    return RB(ref, d + len(vs) * 2.0 ** -23 * mag)


def scale_shift(v, w, b):
    """fmaf(w, v, b) per channel (last dim): the contraction rule with K = 1"""
    w, b = f64(w), f64(b)
    return RB(w * v.ref + b, w.abs() * v.d + 5 * 2.0 ** -23 * ((w * v.ref).abs() + b.abs()))


def dwconv(x, w, b):
    """depthwise temporal convolution of x (B, T, C) with w (C, K), bias b (C): zero padding, K taps, one fp32 fma chain"""
    w, b = f64(w), f64(b)
    C, K = w.shape
    cv = lambda a, k: F.conv1d(a.transpose(1, 2), k.unsqueeze(1), padding=K // 2, groups=C).transpose(1, 2)   # noqa: E731
    mag = cv(x.ref.abs(), w.abs()) + b.abs()
    return RB(cv(x.ref, w) + b, cv(x.d, w.abs()) + (K + 4) * 2.0 ** -23 * mag)


def mean_T(x):
    T = x.ref.shape[1]
    return RB(x.ref.mean(1), x.d.mean(1) + (T + 4) * 2.0 ** -23 * x.ref.abs().mean(1))


def upsample_linear(x, T_hi):
    """nn.Upsample(T_hi, 'linear', align_corners=True) of x (B, T_lo, C), as modules.py:236"""
    B, T_lo, C = x.ref.shape
    if T_hi == T_lo:
        return x
    pos = torch.arange(T_hi, dtype=torch.float64) * ((T_lo - 1) / (T_hi - 1) if T_hi > 1 else 0.0)
    i0 = pos.floor().long().clamp(max=T_lo - 1)
    i1 = (i0 + 1).clamp(max=T_lo - 1)
    l1 = (pos - i0).view(1, -1, 1)
    l0 = 1.0 - l1
    ref = l0 * x.ref[:, i0] + l1 * x.ref[:, i1]
    slope = torch.zeros(B, T_lo + 1, C, dtype=torch.float64)            # slope[j] = |x[j] - x[j-1]|, 0 outside
    if T_lo > 1:
        slope[:, 1:T_lo] = (x.ref[:, 1:] - x.ref[:, :-1]).abs()
    steep = torch.maximum(torch.maximum(slope[:, i0], slope[:, i1]), slope[:, (i0 + 2).clamp(max=T_lo)])
    dnode = torch.maximum(torch.maximum(x.d[:, i0], x.d[:, i1]), x.d[:, (i0 - 1).clamp(min=0)])
    dpos = T_hi * 2.0 ** -23
    d = (l0 * x.d[:, i0] + l1 * x.d[:, i1] + dpos * (steep + dnode)
         + 6 * 2.0 ** -23 * (l0 * x.ref[:, i0].abs() + l1 * x.ref[:, i1].abs()))
    return RB(ref, d)


def pool_windows(T_in, T_out):
    return [((i * T_in) // T_out, -((-(i + 1) * T_in) // T_out)) for i in range(T_out)]


def maxpool(x, T_out):
    """AdaptiveMaxPool1d(T_out) along T of (B, T, C)"""
    win = pool_windows(x.ref.shape[1], T_out)
    return RB(torch.stack([x.ref[:, lo:hi].amax(1) for lo, hi in win], 1), torch.stack([x.d[:, lo:hi].amax(1) for lo, hi in win], 1))


# ----------------------------------------------------------------------------- the SGP stage: normalisation
Stats = namedtuple("Stats", "m d_m rstd d_rstd var ex2")     # per row / group; ex2 = E[x^2] (None for a handed (mean, rstd))


def sums_of(x, dims):
    """(s, d_s, q, d_q, n) of x.ref over dims, summed in fp32 in one pass"""
    n = int(np.prod([x.ref.shape[i] for i in dims]))
    a = x.ref.abs()
    q = (x.ref * x.ref).sum(dims)
    return (x.ref.sum(dims), x.d.sum(dims) + n * 2.0 ** -23 * a.sum(dims),
            q, (2 * a * x.d + x.d * x.d).sum(dims) + n * 2.0 ** -23 * q, n)


def handed_sums(parts, dims):
    """parts (..., 2) = (sum, sum of squares) partials, exact operands; summed over dims in fp32, in order"""
    p = f64(parts)
    nterms = int(np.prod([p.shape[i] for i in dims]))
    s, q = p[..., 0].sum(dims), p[..., 1].sum(dims)
    return s, nterms * 2.0 ** -23 * p[..., 0].abs().sum(dims), q, nterms * 2.0 ** -23 * p[..., 1].abs().sum(dims)


def moments(s, d_s, q, d_q, n, eps):
    m = s / n
    d_m = d_s / n + U_F32 * m.abs()
    ex2 = q / n
    var = (ex2 - m * m).clamp_min(0.0)
    d_var = d_q / n + 2 * m.abs() * d_m + d_m * d_m + 3 * U_F32 * (ex2 + m * m)
    rstd = 1.0 / torch.sqrt(var + eps)
    return Stats(m, d_m, rstd, rstd * (d_var / (2 * (var + eps)) + 2 * U_F32), var, ex2)


def handed_mean_rstd(rowstat):
    """(mean, rstd) pairs (rows, 2) handed to the kernel: exact operands"""
    r = f64(rowstat)
    z = torch.zeros_like(r[..., 0])
    return Stats(r[..., 0], z, r[..., 1], z, None, None)


def first_order(st):
    """smallest var / E[x^2] over the rows / groups: the bound is stated for >= 1 / 32"""
    return float((st.var / st.ex2.clamp_min(1e-300)).min())


def normalise(x, m, d_m, rstd, d_rstd, w, b):
    """(x - m) rstd w + b; the statistics already broadcast to x, w and b along the last dim"""
    w, b = f64(w), f64(b)
    xm = x.ref - m
    dxm = x.d + d_m
    d = w.abs() * (rstd * dxm + xm.abs() * d_rstd + dxm * d_rstd)
    return RB(xm * rstd * w + b, d + 4 * 2.0 ** -23 * (rstd * w.abs() * (x.ref.abs() + m.abs()) + b.abs()))


def layernorm_stats(x, eps, rowstat=None):
    """rowstat: None (computed from the row), (rows, 2) handed (mean, rstd), (parts, rows, 2) handed partial sums"""
    C = x.ref.shape[-1]
    if rowstat is None:
        s, d_s, q, d_q, n = sums_of(x, (-1,))
        return moments(s, d_s, q, d_q, n, eps)
    if rowstat.dim() == 2:
        st = handed_mean_rstd(rowstat)
        return Stats(*[None if v is None else v.view(x.ref.shape[:-1]) for v in st])
    s, d_s, q, d_q = handed_sums(rowstat, (0,))
    shp = x.ref.shape[:-1]
    return moments(s.view(shp), d_s.view(shp), q.view(shp), d_q.view(shp), C, eps)


def layernorm(x, w, b, eps=1e-5, rowstat=None):
    """channel LayerNorm over the last dim of x (B, T, C) (modules.py:320-363: biased variance, eps inside the sqrt)"""
    st = layernorm_stats(x, eps, rowstat)
    u = lambda v: v.unsqueeze(-1)                                       # noqa: E731
    return normalise(x, u(st.m), u(st.d_m), u(st.rstd), u(st.d_rstd), w, b), st


def groupnorm_stats(x, G, eps, chsum=None):
    """chsum: None or handed (parts, B, C, 2) / (B, C, 2) per-channel (sum, sum of squares) over the clip's rows"""
    B, T, C = x.ref.shape
    cg = C // G
    if chsum is None:
        xg = RB(x.ref.view(B, T, G, cg), x.d.view(B, T, G, cg))
        s, d_s, q, d_q, n = sums_of(xg, (1, 3))
        return moments(s, d_s, q, d_q, n, eps)
    p = f64(chsum)
    p = p.unsqueeze(0) if p.dim() == 3 else p
    s, d_s, q, d_q = handed_sums(p.view(p.shape[0], B, G, cg, 2), (0, 3))
    return moments(s, d_s, q, d_q, T * cg, eps)


def groupnorm(x, G, w, b, eps=1e-5, chsum=None):
    """GroupNorm(G) of x (B, T, C) over (C / G) x T"""
    st = groupnorm_stats(x, G, eps, chsum)
    cg = x.ref.shape[-1] // G
    u = lambda v: v.repeat_interleave(cg, dim=1).unsqueeze(1)            # noqa: E731  (B, G) -> (B, 1, C)
    return normalise(x, u(st.m), u(st.d_m), u(st.rstd), u(st.d_rstd), w, b), st


def round_bf16(v):
    """an INTERMEDIATE bf16 rounding of a value known to d << one bf16 ulp (an fp32 value in front of a bf16 operand or a
    bf16 LDS tile).  store_bf16 would carry 2^-8 |v| through every term of the contraction or convolution behind it, a
    worst-case sum a defect in one term hides under.  Rounding is monotone, so the kernel's value lies between the roundings
    of ref - d and ref + d: the reference is the rounding of ref itself and d what those two can differ from it -- zero unless
    a rounding boundary lies within d of ref.  (The interval is widened by 2^-23 for the cast's own path through fp32.)"""
    r = lambda a: a.float().to(BF).double()                                           # noqa: E731
    w = v.d + 2.0 ** -23 * v.ref.abs()
    mid, lo, hi = r(v.ref), r(v.ref - w), r(v.ref + w)
    return RB(mid, torch.maximum((hi - mid).abs(), (lo - mid).abs()))


def as_stored(v, dtype):
    """the fp32 value v written out as `dtype`: one bf16 rounding, or none (the fp32 store keeps the value)"""
    return store_bf16(v) if dtype == BF else v


def as_stream(v, dtype):
    """a value kept in the residual stream's type inside a kernel: a rounding point for bf16, none for fp32"""
    return round_bf16(v) if dtype == BF else v


# ----------------------------------------------------------------------------- the SGP stage: its five launches
def dw_split(dw, db, ks, up):
    """dw (C, 2 ks + up + 2) = [psi | convw | convkw | fc | global_fc], db (5, C) as engine._dwpack lays them out"""
    return dict(psi=(dw[:, :ks], db[0]), cw=(dw[:, ks:2 * ks], db[1]), ckw=(dw[:, 2 * ks:2 * ks + up], db[2]),
                fc=(dw[:, 2 * ks + up], db[3]), g=(dw[:, 2 * ks + up + 1], db[4]))


def branches(o, dw, db, ks, up):
    """(conv_gate, inst, phi) of sgp_tile.h on the normalised sequence o (B, T, C): (convw + convkw) psi, fc phi"""
    p = dw_split(dw, db, ks, up)
    gate = product(total(dwconv(o, *p["cw"]), dwconv(o, *p["ckw"])), dwconv(o, *p["psi"]))
    phi = relu(scale_shift(mean_T(o), *p["g"]))
    inst = product(scale_shift(o, *p["fc"]), RB(phi.ref.unsqueeze(1), phi.d.unsqueeze(1)))
    return gate, inst, phi


def sgp_front_ref(x, ks, up, ln_w, ln_b, dw, db, eps=1e-5, rowstat=None):
    """sgp_front_kernel: y = x + ((fc phi + (convw + convkw) psi) + LN(x)) in fp32, LN(x) NOT rounded in either stream type.
    -> (y in fp32 before the store, dict of the parts)"""
    xe = exact(x)
    o, st = layernorm(xe, ln_w, ln_b, eps, rowstat)
    gate, inst, phi = branches(o, dw, db, ks, up)
    return total(xe, o, inst, gate), dict(ln=o, gate=gate, inst=inst, phi=phi, stats=st)


def mixer_front_ref(z, xlo, ks, up, ln1_w, ln1_b, ln2_w, ln2_b, dw1, db1, dw2, db2, eps=1e-5, rowstat_z=None, rowstat_x=None):
    """mixer_front_kernel: zn = LN1(z) and xn = LN2(x_lo) rounded to the stream's type, xu = up(xn) rounded to it again, the
    branches on zn and xu; cat = [out1 | out2 | out3 | out4 | zn | xu] before its store.  -> (cat, parts)"""
    T_hi, sdt = z.shape[1], z.dtype
    zn, stz = layernorm(exact(z), ln1_w, ln1_b, eps, rowstat_z)
    xn, stx = layernorm(exact(xlo), ln2_w, ln2_b, eps, rowstat_x)
    zn, xn = as_stream(zn, sdt), as_stream(xn, sdt)
    xu = as_stream(upsample_linear(xn, T_hi), sdt)
    g1, i1, p1 = branches(zn, dw1, db1, ks, up)
    g2, i2, p2 = branches(xu, dw2, db2, ks, up)
    slabs = [g1, g2, i1, i2, zn, xu]
    cat = RB(torch.cat([s.ref for s in slabs], -1), torch.cat([s.d for s in slabs], -1))
    return cat, dict(slabs=slabs, phi=(p1, p2), stats=(stz, stx))


def rows(v):
    return reshape(v, -1, v.ref.shape[-1])


def gn_fc1_ref(y, chsum, gn_w, gn_b, W, bias, G=16, eps=1e-5):
    """MODE 0 of sgp_gemm.hip: the GroupNorm table from the handed channel sums, the normalised operand rounded to bf16 (the B
    operand of the MFMA), fp32 accumulation, + bias, GELU, one bf16 store.  -> (H (B, T, N), Stats)"""
    B, T, K = y.shape
    a, st = groupnorm(exact(y), G, gn_w, gn_b, eps, chsum)
    h = store_bf16(gelu(linear(rows(round_bf16(a)), W, None, bias)))
    return reshape(h, B, T, -1), st


def fc2_ref(H, W, bias, resid):
    """MODE 1 before its store: resid + H W^T + b in fp32 (B, T, N)"""
    B, T, K = H.shape
    return reshape(linear(rows(exact(H)), W, None, bias, rows(exact(resid))), B, T, -1)


def cat_fc_ref(A, W, bias):
    """MODE 2 before its store: GELU(A W^T + b) in fp32 (B, T, N)"""
    B, T, K = A.shape
    return reshape(gelu(linear(rows(exact(A)), W, None, bias)), B, T, -1)


# ----------------------------------------------------------------------------- the temporal stage's backward kernels
def sum_over(v, dims, nterms=None):
    """fp32 sum of v over dims, in any order: the summation rule with n = the number of terms"""
    n = int(np.prod([v.ref.shape[i] for i in dims])) if nterms is None else nterms
    return RB(v.ref.sum(dims), v.d.sum(dims) + n * 2.0 ** -23 * v.ref.abs().sum(dims))


def two_pass_stats(x, dims, eps):
    """mean, then the variance around the kernel's own mean (see the module docstring); statistics keep their dims"""
    n = int(np.prod([x.ref.shape[i] for i in dims]))
    a = x.ref.abs()
    m = x.ref.sum(dims, keepdim=True) / n
    d_m = (x.d.sum(dims, keepdim=True) + n * 2.0 ** -23 * a.sum(dims, keepdim=True)) / n + U_F32 * m.abs()
    ex2 = (x.ref * x.ref).sum(dims, keepdim=True) / n
    var = ((x.ref - m) ** 2).sum(dims, keepdim=True) / n
    d_var = d_m * d_m + (n + 4) * 2.0 ** -23 * (var + d_m * d_m)
    rstd = 1.0 / torch.sqrt(var + eps)
    return Stats(m, d_m, rstd, rstd * (d_var / (2 * (var + eps)) + 2 * U_F32), var, ex2), n


def _norm_bwd(x, dy, w, dims, pdims, eps, base):
    """x, dy exact, w broadcast to them; statistics over dims, parameter sums over pdims -> (dx, dw, db, Stats)"""
    st, n = two_pass_stats(x, dims, eps)
    xm = x.ref - st.m
    xhat = RB(xm * st.rstd, st.rstd * (st.d_m + U_F32 * xm.abs()) + xm.abs() * st.d_rstd + st.d_m * st.d_rstd
              + U_F32 * (xm * st.rstd).abs())
    g = product(dy, RB(w, torch.zeros_like(w)))
    def mean(v):                                                          # an n-term fp32 sum, one division
        s_ = v.ref.sum(dims, keepdim=True) / n
        return RB(s_, (v.d.sum(dims, keepdim=True) + n * 2.0 ** -23 * v.ref.abs().sum(dims, keepdim=True)) / n + U_F32 * s_.abs())

    s1, s2 = mean(g), mean(product(g, xhat))
    xs2 = product(xhat, s2)
    inner = g.ref - s1.ref - xs2.ref
    d_inner = g.d + s1.d + xs2.d + 4 * 2.0 ** -23 * (g.ref.abs() + s1.ref.abs() + xs2.ref.abs())
    dx = inner * st.rstd
    dx = RB(dx, st.rstd * d_inner + inner.abs() * st.d_rstd + d_inner * st.d_rstd + U_F32 * dx.abs())
    if base is not None:
        dx = total(dx, RB(f64(base).view(dx.ref.shape), torch.zeros_like(dx.ref)))
    rows = int(np.prod([x.ref.shape[i] for i in pdims]))
    p = dy.ref * xhat.ref
    dw = RB(p.sum(pdims), (dy.ref.abs() * xhat.d).sum(pdims) + rows * 2.0 ** -23 * p.abs().sum(pdims))
    db = RB(dy.ref.sum(pdims), rows * 2.0 ** -23 * dy.ref.abs().sum(pdims))
    return dx, dw, db, st


def layernorm_bwd_ref(x, dy, w, eps=1e-5, base=None):
    """layernorm_bwd_kernel on x, dy (rows, C): -> (dx in fp32 before the store, dw (C), db (C)), Stats per row.
    base: the old contents of dx under `accumulate` (added in fp32 in front of the store)"""
    dx, dw, db, st = _norm_bwd(exact(x), exact(dy), f64(w).view(1, -1), (1,), (0,), eps, base)
    return (dx, dw, db), Stats(*[v.reshape(-1) for v in st])


def groupnorm_bwd_ref(x, dy, G, w, eps=1e-5, base=None):
    """groupnorm_bwd_kernel on x, dy (B, T, C): the same algebra over a [T][C / G] slab; the per-channel parameter sums run
    over T in the launch, then over B in reduce_partials"""
    B, T, C = x.shape
    v5 = lambda a: RB(a.ref.view(B, T, G, C // G), a.d.view(B, T, G, C // G))    # noqa: E731
    dx, dw, db, st = _norm_bwd(v5(exact(x)), v5(exact(dy)), f64(w).view(1, 1, G, C // G), (1, 3), (0, 1), eps,
                               None if base is None else f64(base).view(B, T, G, C // G))
    return (reshape(dx, B, T, C), reshape(dw, C), reshape(db, C)), Stats(*[v.reshape(B, G) for v in st])


def _corr_T(v, w):
    """sum_k w[c][k] v[t + K // 2 - k] with zero padding: the transpose of dwconv's taps -> (ref, |w| d_v, |w| |v|)"""
    w = f64(w).flip(-1)
    C, K = w.shape
    cv = lambda a, k: F.conv1d(a.transpose(1, 2), k.unsqueeze(1), padding=K // 2, groups=C).transpose(1, 2)   # noqa: E731
    return cv(v.ref, w), cv(v.d, w.abs()), cv(v.ref.abs(), w.abs())


def shifted(o, off):
    """o[:, t + off] with zeros outside: (B, T, C) fp64"""
    T = o.shape[1]
    out = torch.zeros_like(o)
    lo, hi = max(0, -off), min(T, T - off)
    if lo < hi:
        out[:, lo:hi] = o[:, lo + off:hi + off]
    return out


def branch_bwd_ref(o, g_conv, g_inst, g_id, ks, up, dw, db):
    """branch_bwd_core in fp64 on exact o and gradients (B, T, C) -> (d_o in fp32 before the store, d_dw (C, 2 ks + up + 2),
    d_db (5, C) in _dwpack's layout, parts, number of (clip, channel) pairs with |pre| <= d_pre: outside the bound's claim)"""
    oe, gc, gi, gd = exact(o), exact(g_conv), exact(g_inst), exact(g_id)
    B, T, C = oe.ref.shape
    p = dw_split(dw, db, ks, up)
    psi, s = dwconv(oe, *p["psi"]), total(dwconv(oe, *p["cw"]), dwconv(oe, *p["ckw"]))
    dpsi, ds = product(gc, s), product(gc, psi)                               # zero outside [0, T): the LDS halo
    fc = scale_shift(oe, *p["fc"])
    mean = mean_T(oe)
    pre = scale_shift(mean, *p["g"])
    phi = relu(pre)
    unsure = int((pre.ref.abs() <= pre.d).sum())
    op = (pre.ref > 0).double()
    bc = lambda v: RB(v.ref.unsqueeze(1), v.d.unsqueeze(1))                   # noqa: E731  (B, C) -> (B, 1, C)
    dphi = sum_over(product(gi, fc), (1,))
    dpre = RB(dphi.ref * op, dphi.d * op)
    wf, wg = f64(p["fc"][0]), f64(p["g"][0])
    dmean = RB(dpre.ref * wg / T, wg.abs() * dpre.d / T + 2 * U_F32 * (dpre.ref * wg / T).abs())
    inst = product(gi, bc(product(RB(wf.expand(B, C), torch.zeros(B, C, dtype=torch.float64)), phi)))
    lin, lin_d, lin_mag = [sum(v) for v in zip(_corr_T(dpsi, p["psi"][0]), _corr_T(ds, p["cw"][0]), _corr_T(ds, p["ckw"][0]))]
    head_mag = gd.ref.abs() + inst.ref.abs() + dmean.ref.abs().unsqueeze(1)
    d_o = RB(gd.ref + inst.ref + dmean.ref.unsqueeze(1) + lin,
             inst.d + dmean.d.unsqueeze(1) + lin_d + (2 * ks + up + 3 + 4) * 2.0 ** -23 * (head_mag + lin_mag))
    # weight gradients: one fma chain over T per (clip, tap, channel), then the clips in reduce_partials: B T terms
    cols = []
    for src, K, in ((dpsi, ks), (ds, ks), (ds, up)):
        for k in range(K):
            osh = shifted(oe.ref, k - K // 2)
            cols.append(sum_over(RB(src.ref * osh, src.d * osh.abs()), (0, 1)))
    s_go, s_g = sum_over(product(gi, oe), (1,)), sum_over(gi, (1,))
    cols.append(sum_over(product(phi, s_go), (0,)))
    cols.append(sum_over(product(dpre, mean), (0,)))
    d_dw = RB(torch.stack([c_.ref for c_ in cols], 1), torch.stack([c_.d for c_ in cols], 1))
    b_psi, b_s = sum_over(dpsi, (0, 1)), sum_over(ds, (0, 1))
    rows5 = [b_psi, b_s, b_s, sum_over(product(phi, s_g), (0,)), sum_over(dpre, (0,))]
    d_db = RB(torch.stack([r.ref for r in rows5]), torch.stack([r.d for r in rows5]))
    parts = dict(identity=gd.ref, inst=inst.ref, gate=lin, dmean=dmean.ref, phi=phi, pre=pre, dpsi=dpsi, ds=ds)
    return d_o, d_dw, d_db, parts, unsure


def upsample_bwd_ref(d_xu, T_lo):
    """upsample_bwd_kernel: d_xn[j] = sum_t wgt(t, j) d_xu[t] over (B, T_hi, C), one fma chain over the contributing t"""
    g = f64(d_xu)
    B, T_hi, C = g.shape
    if T_hi == T_lo:
        return exact(d_xu)
    pos = torch.arange(T_hi, dtype=torch.float64) * ((T_lo - 1) / (T_hi - 1) if T_hi > 1 else 0.0)
    i0 = pos.floor().long().clamp(max=T_lo - 1)
    i1 = (i0 + 1).clamp(max=T_lo - 1)
    l1 = pos - i0
    dpos = T_hi * 2.0 ** -23
    W = torch.zeros(T_hi, T_lo, dtype=torch.float64)                          # the weights
    E = torch.zeros(T_hi, T_lo, dtype=torch.float64)                          # what the position error can move
    tt = torch.arange(T_hi)
    W[tt, i0] += 1.0 - l1
    W[tt, i1] += l1
    E[tt, i0] += dpos
    E[tt, i1] += dpos
    below = (l1 <= dpos) & (i0 > 0)                                           # the kernel may floor to i0 - 1
    above = (1.0 - l1 <= dpos) & (i0 + 2 <= T_lo - 1)                         # or to i0 + 1, whose upper node is i0 + 2
    E[tt[below], i0[below] - 1] += dpos
    E[tt[above], i0[above] + 2] += dpos
    E = E.clamp(max=dpos)
    nterms = int((W != 0).sum(0).max()) + 2
    ein = lambda M_, v: torch.einsum("tj,btc->bjc", M_, v)                     # noqa: E731
    return RB(ein(W, g), ein(E, g.abs()) + (nterms + 6) * 2.0 ** -23 * ein(W, g.abs()))


def maxpool_bwd_ref(x, dy):
    """maxpool_bwd_kernel: the FIRST maximum of each window of x (B, T_in, C) takes that window's dy (B, T_out, C)"""
    xx, g = f64(x), f64(dy)
    B, T_in, C = xx.shape
    ref, mag, cnt = torch.zeros_like(xx), torch.zeros_like(xx), torch.zeros_like(xx)
    for i, (lo, hi) in enumerate(pool_windows(T_in, g.shape[1])):
        at_max = xx[:, lo:hi] == xx[:, lo:hi].amax(1, keepdim=True)
        first = at_max & at_max.double().cumsum(1).eq(1)                     # the first of equal maxima
        ref[:, lo:hi] += first * g[:, i:i + 1]
        mag[:, lo:hi] += first * g[:, i:i + 1].abs()
        cnt[:, lo:hi] += first
    assert int(cnt.max()) <= 3
    return RB(ref, cnt * 2.0 ** -23 * mag)


def gelu_bwd(x, dy):
    """mode 1 of eltwise_kernel: dy (cdf + x pdf), cdf = 0.5 (1 + erff(x / sqrt 2)), pdf = expf(-x^2 / 2) / sqrt(2 pi)"""
    xx, g = f64(x), f64(dy)
    cdf = 0.5 * (1.0 + torch.erf(xx * 0.70710678118654752440))
    xp = xx * 0.39894228040143267794 * torch.exp(-0.5 * xx * xx)
    return RB(g * (cdf + xp), g.abs() * TRANSCENDENTAL * U_F32 * (xx.abs() + cdf.abs() + xp.abs()))


def eltwise_ref(x, dy, mode):
    """the four modes of eltwise_kernel in fp32 before the store: gelu, gelu backward, x + dy, x * dy (one fp32 operation)"""
    if mode == 0:
        return gelu(exact(x))
    if mode == 1:
        return gelu_bwd(x, dy)
    v = f64(x) + f64(dy) if mode == 2 else f64(x) * f64(dy)
    return RB(v, U_F32 * v.abs())


def wgrad_ref(dY, X, X0=None, k0=0, base=None):
    """tdeed_wgrad: dW[n][k] = sum_m dY[m][n] X[m][k], the columns k < k0 of X from X0; db[n] = sum_m dY[m][n].
    base = (dW, db) old contents under `accumulate`.  -> (dW (N, K), db (N))"""
    Y, Xe = f64(dY), f64(X).clone()
    if X0 is not None:
        Xe[:, :k0] = f64(X0)[:, :k0]
    dW = affine(contraction(exact(Y.T), Xe.T))                               # (N, M) . (K, M)^T: K = M terms per element
    db = sum_over(exact(Y), (0,))
    if base is not None:
        dW, db = total(dW, exact(base[0])), total(db, exact(base[1]))
    return dW, db


# ----------------------------------------------------------------------------- checks
def _index(flat, shape, nhwc):
    idx = np.unravel_index(int(flat), tuple(shape))
    if nhwc and len(shape) == 4:
        return "frame %d row %d col %d channel %d" % idx
    return str(tuple(int(i) for i in idx))


def assert_within(out, v, name="", nhwc=False):
    """no element of `out` further from v.ref than v.d (for a bf16 output v is behind store_bf16).  Zero violations."""
    o, ref, tol = f64(out), v.ref, v.d
    assert o.shape == ref.shape, (o.shape, ref.shape)
    assert bool(torch.isfinite(o).all()), f"{name}: non-finite output"
    err = (o - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    worst = int(torch.argmax(ratio))
    nviol = int((err > tol).sum())
    fig = float(ratio.reshape(-1)[worst])
    print(f"[roundoff] {name}: worst err/tol {fig:.3f} at {_index(worst, ref.shape, nhwc)}, {nviol} of {o.numel()} outside")
    assert nviol == 0, (f"{name}: {nviol} of {o.numel()} elements outside the rounding bound, worst err/tol {fig:.3f} at "
                        f"{_index(worst, ref.shape, nhwc)} (out {float(o.reshape(-1)[worst])!r}, "
                        f"ref {float(ref.reshape(-1)[worst])!r}, tol {float(tol.reshape(-1)[worst]):.3e})")
    return fig


def signed_ulp_error(out, ref):
    """mean of (|out| - |ref|) / ulp_bf16(ref) over the elements with |ref| > 2^-10 max|ref|, and their number"""
    o, r = f64(out).reshape(-1), f64(ref).reshape(-1)
    keep = r.abs() > 2.0 ** -10 * r.abs().max()
    o, r = o[keep], r[keep]
    ulp = torch.exp2(torch.floor(torch.log2(r.abs())) - 7)
    return float(((o.abs() - r.abs()) / ulp).mean()), int(keep.sum())


def assert_unbiased(out, ref, name=""):
    """Only where the output is ONE rounding of an fp32 value.  Round-to-nearest-even leaves a mean signed error of 0 ulp with
    sigma <= 0.29 / sqrt(n) <= 0.003 at the n >= 10 000 the shape must supply; a truncating store gives -0.5."""
    ref = ref.ref if isinstance(ref, RB) else ref
    mean, n = signed_ulp_error(out, ref)
    print(f"[roundoff] {name}: mean signed error {mean:+.4f} ulp over {n} elements")
    assert n >= 10000, f"{name}: {n} elements above 2^-10 max|ref|: the shape is too small for the bias check"
    assert abs(mean) < 0.05, f"{name}: mean signed error {mean:+.4f} ulp (round-to-nearest-even: 0, truncation: -0.5)"
    return mean


def assert_pooled_consistent(pooled, y, name=""):
    """squeeze sums of the ROUNDED outputs: pooled (N, parts, C) summed over its parts against the fp64 sum over the pixels of
    the y (N, H, W, C) that the kernel itself wrote, within the doubled fp32 summation bound npix 2^-23 sum|y|"""
    yy = f64(y)
    npix = yy.shape[1] * yy.shape[2]
    got, want = f64(pooled).sum(1), yy.sum(dim=(1, 2))
    tol = npix * 2.0 ** -23 * yy.abs().sum(dim=(1, 2))
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite squeeze sums"
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    worst = int(torch.argmax(ratio))
    nviol = int((err > tol).sum())
    print(f"[roundoff] {name}: squeeze sums worst err/tol {float(ratio.reshape(-1)[worst]):.3f}, {nviol} of {got.numel()} outside")
    assert nviol == 0, (f"{name}: {nviol} of {got.numel()} squeeze sums are not the sums of the stored outputs, worst err/tol "
                        f"{float(ratio.reshape(-1)[worst]):.3f} at (frame, channel) {_index(worst, got.shape, False)}")


def assert_sums_consistent(got, v, dims, name=""):
    """handed statistics are those of the STORED values: got (..., 2) = (sum, sum of squares), already summed over its parts,
    against the fp64 sums over `dims` of the tensor v the kernel itself stored, within the doubled fp32 summation bound
    n 2^-23 sum|v| and the same form for v^2"""
    vv, g = f64(v), f64(got)
    n = int(np.prod([vv.shape[i] for i in dims]))
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite statistics"
    worst = 0.0
    for k, (want, mag) in enumerate(((vv.sum(dims), vv.abs().sum(dims)), ((vv * vv).sum(dims), (vv * vv).sum(dims)))):
        gk = g[..., k].reshape(want.shape)
        err, tol = (gk - want).abs(), n * 2.0 ** -23 * mag
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
        nviol = int((err > tol).sum())
        worst = max(worst, float(ratio.max()))
        print(f"[roundoff] {name}: {('sums', 'sums of squares')[k]} worst err/tol {float(ratio.max()):.3f}, {nviol} of {err.numel()} outside")
        assert nviol == 0, (f"{name}: {nviol} of {err.numel()} {('sums', 'sums of squares')[k]} are not those of the stored "
                            f"values, worst err/tol {float(ratio.max()):.3f}")
    return worst


def old_metric(out, ref):
    """the expression of the older anchor tests: max|out - ref| / max|ref|"""
    o, r = f64(out), f64(ref)
    return float((o - r).abs().max() / r.abs().max().clamp_min(1e-6))
