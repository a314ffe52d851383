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


def old_metric(out, ref):
    """the expression of the older anchor tests: max|out - ref| / max|ref|"""
    o, r = f64(out), f64(ref)
    return float((o - r).abs().max() / r.abs().max().clamp_min(1e-6))
