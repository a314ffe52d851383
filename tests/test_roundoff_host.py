"""The rounding bound of tests/roundoff.py proved on the CPU: a torch emulation of the bf16 kernels' arithmetic (fp32
accumulation, fp32 epilogue, one round-to-nearest-even bf16 store at each rounding point) stays inside it with zero
violations, and each of the defects the older anchor tests (`max|out - ref| / max|ref| < 3e-2`) let through falls outside it
on the SAME operands.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roundoff as R
from helpers import act, t

BF = torch.bfloat16
OLD_TOL = 3e-2                       # BF16_TOL of tests/test_gpu_ops.py


def rnd(seed, name, shape, scale=1.0):
    return t(act(seed, name, shape, scale))


def rne(v):
    return v.to(BF)


def truncate(v):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def emu_linear(A, W, sc, sh, res=None, actn=0, store=rne, partial_every=None):
    """fp32 accumulation, fp32 epilogue, one bf16 store; partial_every: the running sum is rounded to bf16 every so many k"""
    A32, W32 = A.float(), W.float()
    if partial_every is None:
        acc = A32 @ W32.T
    else:
        acc = torch.zeros(A.shape[0], W.shape[0])
        for k in range(0, A.shape[1], partial_every):
            acc = (acc + A32[:, k:k + partial_every] @ W32[:, k:k + partial_every].T).to(BF).float()
    v = acc * sc + sh
    if res is not None:
        v = v + res.float()
    v = [v, torch.relu(v), F.gelu(v)][actn]
    return store(v)


def ref_linear(A, W, sc, sh, res=None, actn=0):
    v = R.linear(R.exact(A), W, sc, sh, None if res is None else R.exact(res))
    return R.store_bf16(R.activation(v, actn))


def gemm_operands(M, K, N, shift_scale=1.0):
    A = rnd(1, f"A{M}", (M, K)).to(BF)
    W = R.bf16_weights(rnd(2, f"W{N}", (N, K), 1.0 / np.sqrt(K)))
    sc, sh = R.fold(3, f"f{N}", N, shift_scale)
    return A, W, sc, sh, rnd(5, f"R{M}", (M, N)).to(BF)


GEMM = [(257, 24, 56), (129, 152, 368)]


# ----------------------------------------------------------------------------- contraction + affine + residual + activation
@pytest.mark.parametrize("M,K,N", GEMM)
def test_faithful_gemm_is_inside_the_bound_and_unbiased(M, K, N):
    A, W, sc, sh, res = gemm_operands(M, K, N)
    out = emu_linear(A, W, sc, sh)
    ref = ref_linear(A, W, sc, sh)
    R.assert_within(out, ref, "plain")
    R.assert_unbiased(out, ref, "plain")
    for actn in (1, 2):
        out = emu_linear(A, W, sc, sh, res, actn)
        ref = ref_linear(A, W, sc, sh, res, actn)
        R.assert_within(out, ref, f"residual, act {actn}")
        if actn == 1:
            assert 0.2 < R.relu_open(ref.ref) < 0.8
    ones, zeros = torch.ones(N), torch.zeros(N)
    R.assert_within(emu_linear(A, W, ones, zeros), ref_linear(A, W, None, None), "no scale")


@pytest.mark.parametrize("M,K,N", GEMM)
def test_truncating_store_passes_the_old_check_and_fails_the_bias_check(M, K, N):
    A, W, sc, sh, _ = gemm_operands(M, K, N)
    out = emu_linear(A, W, sc, sh, store=truncate)
    ref = ref_linear(A, W, sc, sh)
    assert R.old_metric(out, ref.ref) < OLD_TOL
    mean, n = R.signed_ulp_error(out, ref.ref)
    assert n >= 10000 and -0.6 < mean < -0.4, mean
    with pytest.raises(AssertionError, match="mean signed error"):
        R.assert_unbiased(out, ref, "truncating store")
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(out, ref, "truncating store")


def test_bf16_partial_sums_pass_the_old_check_and_fail_the_bound():
    M, K, N = 129, 152, 368
    A, W, sc, sh, _ = gemm_operands(M, K, N)
    ref = ref_linear(A, W, sc, sh)
    R.assert_within(emu_linear(A, W, sc, sh), ref, "faithful")
    out = emu_linear(A, W, sc, sh, partial_every=32)
    assert R.old_metric(out, ref.ref) < OLD_TOL
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(out, ref, "bf16 partials every 32 k")


@pytest.mark.parametrize("M,K,N", GEMM)
def test_a_neighbours_shift_on_the_last_8_channels_fails_even_at_the_old_shift_scale(M, K, N):
    A, W, sc, sh, _ = gemm_operands(M, K, N, shift_scale=0.1)
    ref = ref_linear(A, W, sc, sh, None, 1)
    R.assert_within(emu_linear(A, W, sc, sh, None, 1), ref, "faithful")
    bad = sh.clone()
    bad[-8:] = sh[-16:-8]
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(emu_linear(A, W, sc, bad, None, 1), ref, "neighbour's shift")


def test_row_tail_reading_the_previous_rows_last_k_chunk_fails():
    M, K, N = 257, 24, 56                         # one row behind two 128-row tiles
    A, W, sc, sh, res = gemm_operands(M, K, N)
    ref = ref_linear(A, W, sc, sh, res, 1)
    R.assert_within(emu_linear(A, W, sc, sh, res, 1), ref, "faithful")
    Abad = A.clone()
    Abad[M - 1, K - 8:] = A[M - 2, K - 8:]
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(emu_linear(Abad, W, sc, sh, res, 1), ref, "row tail")


def test_unrounded_scaled_operand_fails():
    Fr, hw, K, N = 6, 49, 152, 368
    M = Fr * hw
    A, W, sc, sh, _ = gemm_operands(M, K, N)
    gate = torch.sigmoid(rnd(11, "g", (Fr, K)))
    xs = R.scaled_operand_bf16(A, gate, hw)
    ref = R.store_bf16(R.linear(xs, W, sc, sh))
    scaled32 = A.float() * gate.repeat_interleave(hw, dim=0)
    R.assert_within(emu_linear(scaled32.to(BF), W, sc, sh), ref, "faithful")
    out = rne((scaled32 @ W.T) * sc + sh)         # the scaled operand kept in fp32
    assert R.old_metric(out, ref.ref) < OLD_TOL
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(out, ref, "scaled operand not rounded")


# ----------------------------------------------------------------------------- grouped 3 x 3
GCONV = [(56, 8, 1, 9, 7), (56, 8, 2, 15, 13)]     # stride 1; stride 2 on an odd map


def gconv_operands(C, gw, H, W, N=3):
    x = rnd(31, f"x{C}", (N, C, H, W)).to(BF)
    w = R.bf16_weights(rnd(32, f"w{C}", (C, gw, 3, 3), 1.0 / np.sqrt(9 * gw)))
    sc, sh = R.fold(33, f"g{C}", C)
    return x, w, sc, sh


def emu_gconv_pre(x, w, sc, sh, stride, gw):
    """fp32 value in front of the ReLU and the store, NCHW"""
    acc = F.conv2d(x.float(), w, stride=stride, padding=1, groups=x.shape[1] // gw)
    return acc * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)


def ref_gconv(x, w, sc, sh, stride, gw):
    return R.store_bf16(R.relu(R.conv2d(R.exact(x), w, stride, x.shape[1] // gw, sc, sh)))


@pytest.mark.parametrize("C,gw,stride,H,W", GCONV)
def test_faithful_grouped_conv_and_a_missing_corner_tap(C, gw, stride, H, W):
    x, w, sc, sh = gconv_operands(C, gw, H, W)
    ref = ref_gconv(x, w, sc, sh, stride, gw)
    assert 0.2 < R.relu_open(ref.ref) < 0.8
    pre = emu_gconv_pre(x, w, sc, sh, stride, gw)
    R.assert_within(rne(torch.relu(pre)), ref, "faithful")
    # tap (0, 0) of the last output pixel of frame 1 (an in-bounds tap) left out of the sum
    Ho, Wo = pre.shape[2:]
    iy, ix = (Ho - 1) * stride - 1, (Wo - 1) * stride - 1
    assert 0 <= iy < H and 0 <= ix < W
    xin = x.float()[1, :, iy, ix].view(C // gw, gw)                               # [group][ci]
    tap = torch.einsum("goi,gi->go", w[:, :, 0, 0].view(C // gw, gw, gw), xin).reshape(C)
    acc = F.conv2d(x.float(), w, stride=stride, padding=1, groups=C // gw)
    acc[1, :, Ho - 1, Wo - 1] -= tap
    bad = rne(torch.relu(acc * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)))
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(bad.permute(0, 2, 3, 1), R.RB(ref.ref.permute(0, 2, 3, 1), ref.d.permute(0, 2, 3, 1)),
                        "missing tap", nhwc=True)


def test_unbiased_store_of_the_grouped_conv():
    C, gw, stride, H, W = GCONV[0]
    x, w, sc, sh = gconv_operands(C, gw, H, W)
    ref = R.store_bf16(R.conv2d(R.exact(x), w, stride, C // gw, sc, sh))          # no ReLU: 10 584 elements
    pre = emu_gconv_pre(x, w, sc, sh, stride, gw)
    R.assert_unbiased(rne(pre), ref, "faithful")
    with pytest.raises(AssertionError, match="mean signed error"):
        R.assert_unbiased(truncate(pre), ref, "truncating store")


@pytest.mark.parametrize("C,gw,stride,H,W", GCONV)
def test_squeeze_sums_of_unrounded_values_fail(C, gw, stride, H, W):
    x, w, sc, sh = gconv_operands(C, gw, H, W)
    v = torch.relu(emu_gconv_pre(x, w, sc, sh, stride, gw))
    y = rne(v).permute(0, 2, 3, 1).contiguous()                                    # what the kernel stores, NHWC
    good = y.float().sum(dim=(1, 2))[:, None, :]                                   # sums of the rounded outputs, one part
    R.assert_pooled_consistent(good, y, "faithful")
    bad = v.sum(dim=(2, 3))[:, None, :]                                            # sums taken in front of the rounding
    ref_mean = ref_gconv(x, w, sc, sh, stride, gw).ref.mean(dim=(2, 3))
    assert R.old_metric(bad[:, 0] / (y.shape[1] * y.shape[2]), ref_mean) < OLD_TOL
    with pytest.raises(AssertionError, match="not the sums of the stored outputs"):
        R.assert_pooled_consistent(bad, y, "un-rounded squeeze")


# ----------------------------------------------------------------------------- two stages with bf16 in between
@pytest.mark.parametrize("stride,H,W", [(1, 9, 7), (2, 15, 13)])
def test_faithful_chain_y1_y2(stride, H, W):
    """conv1 (1 x 1, BatchNorm, ReLU, bf16) -> grouped 3 x 3 (BatchNorm, ReLU, bf16): the bound of y1 travels through conv2"""
    N, Cin, C, gw = 3, 24, 56, 8
    x = rnd(41, "x", (N, H, W, Cin)).to(BF)
    W1 = R.bf16_weights(rnd(42, "w1", (C, Cin), 1.0 / np.sqrt(Cin)))
    s1, h1 = R.fold(43, "c1", C)
    _, w2, s2, h2 = gconv_operands(C, gw, H, W)
    y1 = emu_linear(x.view(-1, Cin), W1, s1, h1, None, 1)                         # bf16
    y1_nchw = y1.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    y2 = rne(torch.relu(emu_gconv_pre(y1_nchw, w2, s2, h2, stride, gw)))
    r1 = ref_linear(x.view(-1, Cin), W1, s1, h1, None, 1)
    R.assert_within(y1, r1, "y1")
    nchw = lambda a: a.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()           # noqa: E731
    r2 = R.store_bf16(R.relu(R.conv2d(R.RB(nchw(r1.ref), nchw(r1.d)), w2, stride, C // gw, s2, h2)))
    assert 0.2 < R.relu_open(r2.ref) < 0.8
    R.assert_within(y2, r2, "y2")
    # conv2 fed with a y1 whose last 8 channels took their neighbours' shift: outside the propagated bound too
    bad = h1.clone()
    bad[-8:] = h1[-16:-8]
    y1b = emu_linear(x.view(-1, Cin), W1, s1, bad, None, 1).view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        R.assert_within(rne(torch.relu(emu_gconv_pre(y1b, w2, s2, h2, stride, gw))), r2, "y2 behind a wrong y1")


def test_transcendental_terms_hold_for_fp32_gelu_and_sigmoid():
    x = rnd(51, "x", (20000,), 3.0)
    v = R.RB(x.double(), torch.zeros(20000, dtype=torch.float64))
    R.assert_within(F.gelu(x), R.gelu(v), "fp32 gelu")
    R.assert_within(torch.sigmoid(x), R.sigmoid(v), "fp32 sigmoid")
    with pytest.raises(AssertionError, match="outside the rounding bound"):       # a bf16-grade function is far outside
        R.assert_within(F.gelu(x.to(BF)).float(), R.gelu(v), "bf16 gelu")
