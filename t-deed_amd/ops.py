"""torch-tensor front ends of the C-ABI entry points (one function per ``tdeed_*_fwd``).

Tensors must live on the GPU ("cuda" is the ROCm device string); activations are
channels-last (NHWC images, NTC sequences).  Nothing here computes on the host: each
function validates shapes, allocates the output with torch (device memory plumbing) and
launches the HIP kernel on the current stream.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr, dtype_code, ACT_NONE, ACT_RELU, ACT_GELU  # noqa: F401


def _chk(t, name, dtype=None):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (tdeed_amd has no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _flip_args(flip, N):
    """flip: bool (all frames) or a uint8/bool tensor of N per-frame flags -> (int flag, mask tensor | None)."""
    if isinstance(flip, torch.Tensor):
        m = flip.to(torch.uint8).contiguous()
        if m.numel() != N or not m.is_cuda:
            raise ValueError(f"flip mask must hold one flag per frame on the GPU ({m.numel()} vs {N})")
        return 0, m
    return int(bool(flip)), None


def stem(frames_u8, w, scale, shift, act_dtype, crop=None, flip=False, out=None, relu=True):
    """frames (N,3,H,W) uint8 (or fp32 holding 0..255: mixup batches) -> (N,Ho,Wo,32).  crop = (top,left,h,w) or None.
    flip: bool for all frames, or a (N,) uint8 tensor of per-frame flags."""
    _chk(frames_u8, "frames", torch.float32 if frames_u8.dtype == torch.float32 else torch.uint8)
    N, _, H, W = frames_u8.shape
    top, left, ch, cw = crop if crop is not None else (0, 0, H, W)
    Ho, Wo = (ch + 1) // 2, (cw + 1) // 2
    if out is None:
        out = torch.empty((N, Ho, Wo, 32), dtype=act_dtype, device=frames_u8.device)
    fl, fmask = _flip_args(flip, N)
    call("tdeed_stem_fwd", ptr(frames_u8), int(frames_u8.dtype == torch.float32), N, H, W, top, left, ch, cw, fl,
         ptr(fmask), ptr(w), ptr(scale), ptr(shift),
         ptr(out), int(relu), dtype_code(act_dtype), stream_ptr())
    return out


def stem_mfma_parts(ch, cw):
    return _lib.load().tdeed_stem_mfma_parts(ch, cw)


def stem_mfma(frames, wfrag, crop=None, flip=False):
    """Training stem on the MFMA pipe (bf16): frames (N,3,H,W) uint8 or fp32 0..255 -> (z (N,Ho,Wo,32) raw conv output,
    colpart (N*parts, 2, 32) fp32 per-workgroup column sums / sums of squares of z)."""
    _chk(frames, "frames", torch.float32 if frames.dtype == torch.float32 else torch.uint8)
    _chk(wfrag, "wfrag", torch.float32)
    N, _, H, W = frames.shape
    top, left, ch, cw = crop if crop is not None else (0, 0, H, W)
    parts = stem_mfma_parts(ch, cw)
    if parts <= 0:
        raise RuntimeError(f"stem_mfma: a {cw}-pixel row band does not fit LDS")
    z = torch.empty((N, (ch + 1) // 2, (cw + 1) // 2, 32), dtype=torch.bfloat16, device=frames.device)
    colpart = torch.empty((N * parts, 2, 32), dtype=torch.float32, device=frames.device)
    fl, fmask = _flip_args(flip, N)
    call("tdeed_stem_mfma_fwd", ptr(frames), int(frames.dtype == torch.float32), N, H, W, top, left, ch, cw, fl, ptr(fmask),
         ptr(wfrag), ptr(z), ptr(colpart), stream_ptr())
    return z, colpart


def stem_mfma_eval(frames, wfrag, scale, shift, crop=None, flip=False, out=None):
    """The eval instance of the MFMA stem (bf16): frames (N,3,H,W) uint8 or fp32 0..255 -> (N,Ho,Wo,32) bf16 activation map
    relu(scale * conv + shift), the folded BatchNorm applied to the fp32 accumulator (one rounding).  scale, shift fp32 (32,).
    crop / flip as `stem`; serves the geometries with stem_mfma_parts(ch, cw) > 0."""
    _chk(frames, "frames", torch.float32 if frames.dtype == torch.float32 else torch.uint8)
    _chk(wfrag, "wfrag", torch.float32)
    _chk(scale, "scale", torch.float32)
    _chk(shift, "shift", torch.float32)
    if scale.numel() != 32 or shift.numel() != 32:
        raise ValueError("stem_mfma_eval: scale and shift hold one value per stem channel (32)")
    N, _, H, W = frames.shape
    top, left, ch, cw = crop if crop is not None else (0, 0, H, W)
    if stem_mfma_parts(ch, cw) <= 0:
        raise RuntimeError(f"stem_mfma_eval: a {cw}-pixel row band does not fit LDS")
    shape = (N, (ch + 1) // 2, (cw + 1) // 2, 32)
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=frames.device)
    _chk(out, "out", torch.bfloat16)
    if tuple(out.shape) != shape:
        raise ValueError(f"stem_mfma_eval: out {tuple(out.shape)}, expected {shape}")
    fl, fmask = _flip_args(flip, N)
    call("tdeed_stem_mfma_eval_fwd", ptr(frames), int(frames.dtype == torch.float32), N, H, W, top, left, ch, cw, fl, ptr(fmask),
         ptr(wfrag), ptr(scale), ptr(shift), ptr(out), stream_ptr())
    return out


def s1_front_parts(ch, cw, C1):
    return _lib.load().tdeed_s1_front_parts(ch, cw, C1)


def s1_front(frames_u8, fw, crop=None, flip=False, y2=None, shortcut=None, pooled=None):
    """Fused pre-proc + stem + s1.b1.{conv1, conv2, downsample} (bf16).  fw: packing.pack_front_weights(...).
    frames (N,3,H,W) uint8 -> y2 (N,Ho,Wo,C1), shortcut (N,Ho,Wo,C1), pooled (N,parts,C1) fp32 sums."""
    _chk(frames_u8, "frames", torch.uint8)
    N, _, H, W = frames_u8.shape
    top, left, ch, cw = crop if crop is not None else (0, 0, H, W)
    Hs, Ws = (ch + 1) // 2, (cw + 1) // 2
    Ho, Wo = (Hs + 1) // 2, (Ws + 1) // 2
    C1 = fw.C1
    dev = frames_u8.device
    if y2 is None:
        y2 = torch.empty((N, Ho, Wo, C1), dtype=torch.bfloat16, device=dev)
    if shortcut is None:
        shortcut = torch.empty((N, Ho, Wo, C1), dtype=torch.bfloat16, device=dev)
    if pooled is None:
        pooled = torch.empty((N, s1_front_parts(ch, cw, C1), C1), dtype=torch.float32, device=dev)
    call("tdeed_s1_front_fwd", ptr(frames_u8), N, H, W, top, left, ch, cw, int(flip), ptr(fw.stem_wf), ptr(fw.stem_sc),
         ptr(fw.stem_sh), C1, ptr(fw.w1f), ptr(fw.sc1), ptr(fw.sh1), ptr(fw.wdf), ptr(fw.scd), ptr(fw.shd),
         ptr(fw.w2f), ptr(fw.sc2), ptr(fw.sh2), ptr(y2), ptr(shortcut), ptr(pooled), stream_ptr())
    return y2, shortcut, pooled


def gemm_colpart_rows(M):
    """rows of the per-tile column-statistics buffer of gemm(colpart=...): one per 128-row tile"""
    return (M + 127) // 128


def _out2(out2, A):
    if out2 is None:
        return None, 0, 0
    _chk(out2, "out2", A.dtype)
    return ptr(out2), out2.shape[-1], out2.shape[-1]


def gemm(A, W, scale=None, shift=None, act=ACT_NONE, residual=None, a_scale=None, a_scale_rows=0,
         A0=None, k0=0, gather=None, out=None, M=None, lda=None, ldc=None, colpart=None, out2=None, out2_pre=False):
    """C = act((A' @ W^T) * scale + shift + residual).  A (M,K) / W (N,K) same dtype.
    gather = (stride, hi, wi, ho, wo) for the stride-2 1x1 shortcut.  out2 (.., n2): also receives columns [0, n2);
    out2_pre: out2 gets them before residual / activation and C keeps only the residual there."""
    _chk(A, "A"); _chk(W, "W", A.dtype)
    K = W.shape[1]
    N = W.shape[0]
    if M is None:
        M = A.numel() // A.shape[-1]
        if gather is not None:
            s, hi, wi, ho, wo = gather
            M = (M // (hi * wi)) * ho * wo
    lda = A.shape[-1] if lda is None else lda
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    ldc = N if ldc is None else ldc
    g = gather if gather is not None else (1, 0, 0, 0, 0)
    call("tdeed_gemm_fwd", ptr(A), lda, ptr(A0), (A0.shape[-1] if A0 is not None else 0), k0,
         ptr(a_scale), a_scale_rows, M, K, N, ptr(W), W.shape[1], ptr(scale), ptr(shift),
         ptr(residual), (residual.shape[-1] if residual is not None else 0), act, ptr(out), ldc,
         g[0], g[1], g[2], g[3], g[4], ptr(colpart), *_out2(out2, A), int(bool(out2_pre)), dtype_code(A.dtype), stream_ptr())
    return out


def c1_gconv_fits(Hi, Wi, Cin, C, stride):
    return _lib.load().tdeed_c1_gconv_fits(Hi, Wi, Cin, C, stride) != 0


def c1_gconv_slab_loop_fits(Hi, Wi, Cin, C, stride):
    """True when the slab-loop form of c1_gconv (one workgroup per (frame, band) walks the channel slabs) exists for the shape."""
    lib = _lib.load()
    if not hasattr(lib, "tdeed_c1_gconv_slab_loop_fits"):    # an A/B flavour of the library built from an older revision
        return False
    return lib.tdeed_c1_gconv_slab_loop_fits(Hi, Wi, Cin, C, stride) != 0


def c1_gconv_set_form(form):
    """-1: c1_gconv's form as routed (default: the slab loop wherever it fits); 0: per slab everywhere; 1: the same as -1."""
    call("tdeed_c1_gconv_set_form", form)


def c1_gconv_workgroups(N, Hi, Wi, Cin, C, stride):
    """the grid c1_gconv launches for N frames of this shape under the form in force"""
    return _lib.load().tdeed_c1_gconv_workgroups(N, Hi, Wi, Cin, C, stride)


def c1_gconv_slab_tiles(Hi, Wi, C, stride):
    return _lib.load().tdeed_c1_gconv_slab_tiles(Hi, Wi, C, stride)


def c1_gconv(x, w1f, s1, h1, wfrag, scale, shift, gw, stride, C, G=None, out=None, pooled=None):
    """conv1 + grouped 3x3 of one bottleneck in one launch (tdeed_c1_gconv_fwd): x (N,Hi,Wi,Cin) bf16 -> y2 (N,Ho,Wo,C),
    pooled (N, parts, C) squeeze partial sums.  G (N*Hi*Wi, Fp): gate-shift output spliced into conv1's operand."""
    _chk(x, "x", torch.bfloat16); _chk(G, "G", torch.bfloat16)
    N, Hi, Wi, Cin = x.shape
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    if pooled is None:
        pooled = torch.empty((N, gconv3x3_parts(Hi, Wi, C, stride, x.dtype), C), dtype=torch.float32, device=x.device)
    call("tdeed_c1_gconv_fwd", ptr(x), ptr(G), (G.shape[-1] if G is not None else 0), N, Hi, Wi, Cin, C, gw, stride, ptr(w1f),
         ptr(s1), ptr(h1), ptr(wfrag), ptr(scale), ptr(shift), ptr(out), ptr(pooled), stream_ptr())
    return out, pooled


def c1_gconv_c3in_fits(Hi, Wi, Cp, C):
    """True when c1_gconv_c3in() serves a stride-2 block of Cp -> C channels behind a producer conv3 of Cp -> Cp (one channel
    slab, the band fits LDS, a frame of the operands below 2^31 bytes)."""
    lib = _lib.load()
    if not hasattr(lib, "tdeed_c1_gconv_c3in_fits"):    # an A/B flavour of the library built from an older revision
        return False
    return lib.tdeed_c1_gconv_c3in_fits(Hi, Wi, Cp, C) != 0


def c1_gconv_c3in_set_walk(walk):
    """0: the run length of c1_gconv_c3in's band walk as routed per shape (default); k >= 1: one workgroup per (frame, run
    of k bands), clamped to the frame's band count (1: runs of one band).  The same kernel and the same bits at every k."""
    call("tdeed_c1_gconv_c3in_set_walk", walk)


def c1_gconv_c3in_walk(Hi, Wi, Cp, C):
    """the routed run length of c1_gconv_c3in for the shape (at most the frame's band count; 0: the shape is not served)"""
    return _lib.load().tdeed_c1_gconv_c3in_walk(Hi, Wi, Cp, C)


def c1_gconv_c3in_workgroups(N, Hi, Wi, Cp, C):
    """the grid c1_gconv_c3in launches for N frames of this shape under the run length in force"""
    return _lib.load().tdeed_c1_gconv_c3in_workgroups(N, Hi, Wi, Cp, C)


def c1_gconv_c3in(y2p, scp, gate, w3frag, s3, h3, w1f, s1, h1, wfrag, scale, shift, gw, C, xs2=None, out=None, pooled=None):
    """c1_gconv(gemm_ws(y2p, w3frag, Cp, Cp, s3, h3, ACT_RELU, residual=scp, a_scale=gate, a_scale_rows=Hi*Wi), ..., stride 2)
    in one launch (tdeed_c1_gconv_c3in_fwd), bit for bit: the producer's conv3 runs per pixel tile in front of conv1 and its
    output map never exists.  y2p / scp (N,Hi,Wi,Cp) bf16, gate (N,Cp) fp32, w3frag from packing.pack_ws_weights.
    xs2 (N,Ho,Wo,Cp): receives the producer's output at even rows and columns (the rows the block's shortcut conv gathers)."""
    _chk(y2p, "y2p", torch.bfloat16); _chk(scp, "scp", torch.bfloat16); _chk(gate, "gate", torch.float32)
    _chk(xs2, "xs2", torch.bfloat16)
    N, Hi, Wi, Cp = y2p.shape
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    if tuple(scp.shape) != (N, Hi, Wi, Cp) or gate.numel() != N * Cp or (xs2 is not None and xs2.numel() != N * Ho * Wo * Cp):
        raise ValueError(f"c1_gconv_c3in: y2p {tuple(y2p.shape)}, scp {tuple(scp.shape)}, gate {tuple(gate.shape)}, "
                         f"xs2 {None if xs2 is None else tuple(xs2.shape)} do not belong together")
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=y2p.dtype, device=y2p.device)
    if pooled is None:
        pooled = torch.empty((N, gconv3x3_parts(Hi, Wi, C, 2, y2p.dtype), C), dtype=torch.float32, device=y2p.device)
    call("tdeed_c1_gconv_c3in_fwd", ptr(y2p), ptr(scp), ptr(gate), ptr(w3frag), ptr(s3), ptr(h3), ptr(xs2), N, Hi, Wi, Cp, C, gw,
         ptr(w1f), ptr(s1), ptr(h1), ptr(wfrag), ptr(scale), ptr(shift), ptr(out), ptr(pooled), stream_ptr())
    return out, pooled


def bneck_fits(h, w, C, R):
    return _lib.load().tdeed_bneck_fits(h, w, C, R) != 0


def bneck(x, w1f, s1, h1, w2f, s2, h2, se_w1f, se_b1, se_w2f, se_b2, R, w3f, s3, h3, G=None, out=None, out2=None,
          w2_tap_major=True):
    """Whole stride-1 bottleneck in one launch (tdeed_bneck_fwd): x (N,h,w,C) bf16 -> (N,h,w,C); G (N*h*w, Fp): gate-shift
    output spliced into conv1's operand; out2 (N*h*w, n2): compact copy of the first n2 output channels.
    w2f: packing.pack_gconv_frags(..., tap_major=w2_tap_major) -- tap-major k-slots are the conflict-free order of this launch
    (group width 8: bit-identical to the chain either way); False: the order tdeed_gconv3x3_fwd reads (16-wide groups)."""
    _chk(x, "x", torch.bfloat16); _chk(G, "G", torch.bfloat16); _chk(out2, "out2", torch.bfloat16)
    N, h, w, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    call("tdeed_bneck_fwd", ptr(x), ptr(G), (G.shape[-1] if G is not None else 0), N, h, w, C, ptr(w1f), ptr(s1),
         ptr(h1), ptr(w2f), ptr(s2), ptr(h2), ptr(se_w1f), ptr(se_b1), ptr(se_w2f), ptr(se_b2), R, ptr(w3f), ptr(s3), ptr(h3),
         ptr(out), ptr(out2), (out2.shape[-1] if out2 is not None else 0), int(bool(w2_tap_major)), stream_ptr())
    return out


def bneck_gs(x, gx, gate, ysum, xsum, cw1, cb1, cw2, cb2, T, F, Fp, w1f, s1, h1, w2f, s2, h2, se_w1f, se_b1, se_w2f, se_b2, R,
             w3f, s3, h3, out=None, out2=None, w2_tap_major=True, qtail=None):
    """The one-launch bottleneck behind a gate-shift-fuse site with the site's blend inside its frame load
    (tdeed_bneck_gs_fwd): gx (N,h,w,ldx >= Fp) the slice's source, gate / ysum / xsum from gate_shift(gates_only=True).
    == bneck(x, G=gate_shift(gx, ..., src_order=True)), bit for bit.
    qtail = (wpf, bn, F, Q): also the tap maps Q (N,h,w,6) of the NEXT block's site (fold F, wpf = packing.pack_gsf_p_frags,
    bn = gsq_bn_table) -- what gate_shift's first launch computes from `out`, in another fp32 summation order; that site then
    runs gate_shift(q_given=True)."""
    _chk(x, "x", torch.bfloat16); _chk(gx, "gx", torch.bfloat16); _chk(out2, "out2", torch.bfloat16)
    N, h, w, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    call("tdeed_bneck_gs_fwd", ptr(x), ptr(gx), gx.shape[-1], ptr(gate), ptr(ysum), ptr(xsum), ptr(cw1), ptr(cb1), ptr(cw2),
         ptr(cb2), T, F, Fp, N, h, w, C, ptr(w1f), ptr(s1), ptr(h1), ptr(w2f), ptr(s2), ptr(h2), ptr(se_w1f), ptr(se_b1),
         ptr(se_w2f), ptr(se_b2), R, ptr(w3f), ptr(s3), ptr(h3), ptr(out), ptr(out2),
         (out2.shape[-1] if out2 is not None else 0), int(bool(w2_tap_major)),
         *((ptr(qtail[0]), ptr(qtail[1]), int(qtail[2]), ptr(qtail[3])) if qtail is not None else (None, None, 0, None)),
         stream_ptr())
    return out


def bneck_qtail_fits(h, w, C, F):
    return _lib.load().tdeed_bneck_qtail_fits(h, w, C, F) != 0


def gsq_bn_table(bn_scale, bn_shift):
    """[2][8 * ceil(F / 8)] fp32: the site's folded BatchNorm3d scale | shift, zeros behind channel F (tdeed_bneck_gs_fwd's q_bn)."""
    F = bn_scale.numel()
    t = torch.zeros((2, (F + 7) // 8 * 8), dtype=torch.float32, device=bn_scale.device)
    t[0, :F] = bn_scale
    t[1, :F] = bn_shift
    return t


def gemm_ws_fits_mode(K, N, act_dtype):
    """0: no; 1: weights fit LDS (preferred kernel for narrow layers); 2: weights streamed from L2 (wide layers)."""
    return _lib.load().tdeed_gemm_ws_fits(K, N, dtype_code(act_dtype))


def gemm_ws_fits(K, N, act_dtype):
    return gemm_ws_fits_mode(K, N, act_dtype) != 0


def gemm_ws(A, Wfrag, K, N, scale=None, shift=None, act=ACT_NONE, residual=None, a_scale=None, a_scale_rows=0,
            A0=None, k0=0, gather=None, out=None, M=None, lda=None, ldc=None, out2=None):
    """Weight-stationary streaming form of gemm(); Wfrag from packing.pack_ws_weights."""
    _chk(A, "A")
    if M is None:
        M = A.numel() // A.shape[-1]
        if gather is not None:
            s, hi, wi, ho, wo = gather
            M = (M // (hi * wi)) * ho * wo
    lda = A.shape[-1] if lda is None else lda
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    ldc = N if ldc is None else ldc
    g = gather if gather is not None else (1, 0, 0, 0, 0)
    call("tdeed_gemm_ws_fwd", ptr(A), lda, ptr(A0), (A0.shape[-1] if A0 is not None else 0), k0,
         ptr(a_scale), a_scale_rows, M, K, N, ptr(Wfrag), ptr(scale), ptr(shift),
         ptr(residual), (residual.shape[-1] if residual is not None else 0), act, ptr(out), ldc,
         g[0], g[1], g[2], g[3], g[4], *_out2(out2, A), dtype_code(A.dtype), stream_ptr())
    return out


def gemm_ws_sc_fits(K, Ks, N, act_dtype):
    """True when gemm_ws_sc() serves a conv3 of K -> N channels with a shortcut conv of Ks -> N."""
    lib = _lib.load()
    if not hasattr(lib, "tdeed_gemm_ws_sc_fits"):       # an A/B flavour of the library built from an older revision
        return False
    return lib.tdeed_gemm_ws_sc_fits(K, Ks, N, dtype_code(act_dtype)) != 0


def gemm_ws_sc(A, Wfrag, K, N, scale, shift, As, Wsfrag, Ks, sscale, sshift, act=ACT_NONE, a_scale=None, a_scale_rows=0,
               A0=None, k0=0, gather=None, out=None, M=None, out2=None):
    """gemm_ws(A, ..., residual=gemm_ws(As, Wsfrag, Ks, N, sscale, sshift, ACT_NONE, gather=gather)) in one launch
    (tdeed_gemm_ws_sc_fwd): the shortcut conv of a bottleneck inside its conv3, bit for bit.  A (M, K) bf16; As the block's
    input rows (.., Ks), gathered with gather = (stride, hi, wi, ho, wo) when the block is strided."""
    _chk(A, "A", torch.bfloat16); _chk(As, "As", torch.bfloat16)
    if M is None:
        M = A.numel() // A.shape[-1]
    rows_s = As.numel() // As.shape[-1]
    g = gather if gather is not None else (1, 0, 0, 0, 0)
    need = (M // (g[3] * g[4])) * g[1] * g[2] if gather is not None else M
    if rows_s < need or A.numel() // A.shape[-1] < M:
        raise ValueError(f"gemm_ws_sc: operands hold {A.numel() // A.shape[-1]} / {rows_s} rows, {M} / {need} needed")
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    call("tdeed_gemm_ws_sc_fwd", ptr(A), A.shape[-1], ptr(A0), (A0.shape[-1] if A0 is not None else 0), k0,
         ptr(a_scale), a_scale_rows, M, K, N, ptr(Wfrag), ptr(scale), ptr(shift), ptr(As), As.shape[-1], Ks, ptr(Wsfrag),
         ptr(sscale), ptr(sshift), act, ptr(out), N, g[0], g[1], g[2], g[3], g[4], *_out2(out2, A), dtype_code(A.dtype),
         stream_ptr())
    return out


def gemm_rs_fits(M, K, N):
    return _lib.load().tdeed_gemm_rs_fits(M, K, N) != 0


def gemm_rs(A, Wfrag, K, N, scale=None, shift=None, act=ACT_NONE, residual=None, a_scale=None, a_scale_rows=0, A0=None, k0=0,
            out=None, M=None, out2=None):
    """Register-stationary form of gemm_ws() for K = N = 320 (tdeed_gemm_rs_fwd); Wfrag from packing.pack_ws_weights."""
    _chk(A, "A", torch.bfloat16)
    if M is None:
        M = A.numel() // A.shape[-1]
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    call("tdeed_gemm_rs_fwd", ptr(A), A.shape[-1], ptr(A0), (A0.shape[-1] if A0 is not None else 0), k0, ptr(a_scale),
         a_scale_rows, M, K, N, ptr(Wfrag), ptr(scale), ptr(shift), ptr(residual),
         (residual.shape[-1] if residual is not None else 0), act, ptr(out), N, *_out2(out2, A), stream_ptr())
    return out


def gemm_rs_stats(A, Wfrag, K, N, M=None, A0=None, k0=0):
    """Training forward of a K = N = 320 layer on the register-stationary kernel: raw output + the (sums, sums of squares,
    row stride, rows) partials of its BatchNorm statistics (tdeed_gemm_rs_stats_fwd), like gemm(colpart=...)."""
    _chk(A, "A", torch.bfloat16)
    if M is None:
        M = A.numel() // A.shape[-1]
    out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    P = _lib.load().tdeed_gemm_rs_grid(M)
    cp = torch.empty((P, 2, N), dtype=torch.float32, device=A.device)
    call("tdeed_gemm_rs_stats_fwd", ptr(A), A.shape[-1], ptr(A0), (A0.shape[-1] if A0 is not None else 0), k0, M, K, N,
         ptr(Wfrag), ptr(out), N, ptr(cp), stream_ptr())
    flat = cp.view(-1)
    return out, (flat, flat[N:], 2 * N, P)


def gemm_splitk_splits(K):
    return _lib.load().tdeed_gemm_splitk_splits(K)


def gemm_splitk_workspace(M, K, N, device):
    """fp32 scratch for gemm_splitk: one [M][N] partial per K chunk."""
    return torch.empty((_lib.load().tdeed_gemm_splitk_splits(K), M, N), dtype=torch.float32, device=device)


def gemm_splitk(A, W, scale, shift, act=ACT_NONE, residual=None, out=None, M=None, workspace=None):
    """Split-K contraction for short sequences (bf16): act((A . W^T) * scale + shift + residual)."""
    _chk(A, "A", torch.bfloat16)
    _chk(W, "W", torch.bfloat16)
    N, K = W.shape
    if M is None:
        M = A.numel() // K
    if out is None:
        out = torch.empty(tuple(A.shape[:-1]) + (N,), dtype=A.dtype, device=A.device)
    if workspace is None:
        workspace = gemm_splitk_workspace(M, K, N, A.device)
    call("tdeed_gemm_splitk_fwd", ptr(A), K, M, K, N, ptr(W), K, ptr(scale), ptr(shift), ptr(residual), N, act,
         ptr(out), N, ptr(workspace), stream_ptr())
    return out


def se_gate_mfma_fits(C, R):
    return _lib.load().tdeed_se_gate_mfma_fits(C, R) != 0


def se_gate_mfma(pooled, inv_cnt, w1f, b1, w2f, b2, R, out=None):
    """SE excitation on the MFMA pipe; pooled (N, parts, C) fp32 partial sums -> gate (N, C) fp32."""
    N, parts, C = pooled.shape
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=pooled.device)
    call("tdeed_se_gate_mfma_fwd", ptr(pooled), parts, float(inv_cnt), N, C, R, ptr(w1f), ptr(b1), ptr(w2f), ptr(b2),
         ptr(out), stream_ptr())
    return out


def se_gate_bf16(pooled, inv_cnt, w1p, b1, w2p, b2, R, out=None):
    """SE excitation with bf16 packed weights (packing.pack_se_bf16): pooled (N,parts,C) sums -> gate (N,C)."""
    N, parts, C = pooled.shape
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=pooled.device)
    call("tdeed_se_gate_bf16_fwd", ptr(pooled), parts, float(inv_cnt), N, C, R, ptr(w1p), ptr(b1), ptr(w2p), ptr(b2),
         ptr(out), stream_ptr())
    return out


def gconv3x3_mfma_fits(Hi, Wi, C, stride):
    return _lib.load().tdeed_gconv3x3_mfma_fits(Hi, Wi, C, stride) != 0


def gconv3x3_parts(Hi, Wi, C, stride, act_dtype):
    return _lib.load().tdeed_gconv3x3_parts(Hi, Wi, C, stride, dtype_code(act_dtype))


def gconv3x3(x, w_packed, scale, shift, gw, stride, wfrag=None, out=None, pooled=None, relu=True, pooled_sq=None,
             in_affine=None):
    """x (N,Hi,Wi,C) -> y (N,Ho,Wo,C), pooled (N,parts,C) fp32 partial sums over pixels.
    w_packed: fp32 [G][9][gw][gw] (VALU path); wfrag: bf16 MFMA fragments (bf16 path).
    in_affine = (a, b) fp32 [C] (bf16 MFMA path): x is a raw conv output, relu(a*x + b) is applied while it is staged."""
    _chk(x, "x")
    N, Hi, Wi, C = x.shape
    Ho, Wo = (Hi - 1) // stride + 1, (Wi - 1) // stride + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    parts = gconv3x3_parts(Hi, Wi, C, stride, x.dtype) if wfrag is not None else 1
    if pooled is None:
        pooled = torch.empty((N, parts, C), dtype=torch.float32, device=x.device)
    call("tdeed_gconv3x3_fwd", ptr(x), N, Hi, Wi, C, gw, stride, ptr(w_packed), ptr(wfrag), ptr(scale), ptr(shift),
         ptr(out), ptr(pooled), ptr(pooled_sq), ptr(in_affine[0] if in_affine else None),
         ptr(in_affine[1] if in_affine else None), int(relu), dtype_code(x.dtype), stream_ptr())
    return out, pooled


def se_gate(pooled, inv_cnt, w1t, b1, w2t, b2, out=None):
    """pooled (N,parts,C) partial sums -> gate (N,C).  w1t (C,R), w2t (R,C)."""
    N, parts, C = pooled.shape
    R = w1t.shape[1]
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=pooled.device)
    call("tdeed_se_gate_fwd", ptr(pooled), parts, float(inv_cnt), N, C, R, ptr(w1t), ptr(b1), ptr(w2t), ptr(b2),
         ptr(out), stream_ptr())
    return out


def gate_shift(x, B, T, F, Fp, bn_scale, bn_shift, wq, b3d, cw1=None, cb1=None, cw2=None, cb2=None,
               bufs=None, wqf=None, separate_weight=False, src_order=False, gates_only=False, q_given=False):
    """x (B*T,h,w,C) -> (B*T*h*w, Fp): gated/shifted/fused first F channels (+ pad copy).
    GSM when cw1 is None.  bufs: optional dict of preallocated gate/ysum/xsum/fw/out.
    src_order (GSF, bf16): the output stays in source channel order, out[:, gs_source_order(F)] is the module's output.
    q_given: bufs["q"] already holds the site's tap maps (bneck_gs's qtail): the first launch is skipped.
    gates_only: stop behind the gate launches and return (gate, ysum, xsum) -- the caller's next launch does the blend (bneck_gs)."""
    _chk(x, "x")
    N, h, w, C = x.shape
    dev = x.device
    bufs = bufs or {}
    gate = bufs.get("gate")
    if gate is None:
        gate = torch.empty((N, h, w, 2), dtype=torch.float32, device=dev)
    ysum = bufs.get("ysum")
    if ysum is None:
        ysum = torch.empty((N, F), dtype=torch.float32, device=dev)
    xsum = bufs.get("xsum")
    if xsum is None:
        xsum = torch.empty((N, F), dtype=torch.float32, device=dev)
    out = bufs.get("out")
    if out is None and not gates_only:
        out = torch.empty((N * h * w, Fp), dtype=x.dtype, device=dev)
    q = bufs.get("q")
    if q is None:
        q = torch.empty((N, h, w, 6), dtype=torch.float32, device=dev)
    dc = dtype_code(x.dtype)
    if q_given:
        if x.dtype != torch.bfloat16 or bufs.get("q") is None:
            raise ValueError("gate_shift: q_given needs bufs['q'] and bf16")
        call("tdeed_gsf_gate_sums_fwd", ptr(x), B, T, h, w, C, F, ptr(b3d), ptr(q), ptr(gate), ptr(ysum), ptr(xsum), stream_ptr())
    else:
        call("tdeed_gsf_gate_fwd", ptr(x), B, T, h, w, C, F, ptr(bn_scale), ptr(bn_shift), ptr(wq), ptr(wqf), ptr(b3d),
             ptr(q), ptr(gate), ptr(ysum), ptr(xsum), dc, stream_ptr())
    if gates_only:
        return gate, ysum, xsum
    if src_order:
        if cw1 is None or separate_weight or x.dtype != torch.bfloat16:
            raise ValueError("gate_shift: src_order is the fused bf16 GSF launch only")
        call("tdeed_gsf_blend_src_fwd", ptr(x), ptr(gate), ptr(ysum), ptr(xsum), ptr(cw1), ptr(cb1), ptr(cw2), ptr(cb2),
             B, T, h, w, C, F, Fp, ptr(out), dc, stream_ptr())
        return out
    if cw1 is not None and not separate_weight:
        call("tdeed_gsf_apply_fused_fwd", ptr(x), ptr(gate), ptr(ysum), ptr(xsum), ptr(cw1), ptr(cb1), ptr(cw2), ptr(cb2),
             B, T, h, w, C, F, Fp, ptr(out), dc, stream_ptr())
        return out
    fw = None
    if cw1 is not None:
        fw = bufs.get("fw")
        if fw is None:
            fw = torch.empty((B, F, T), dtype=torch.float32, device=dev)
        call("tdeed_gsf_weight_fwd", ptr(ysum), ptr(xsum), B, T, F, h * w, ptr(cw1), ptr(cb1), ptr(cw2), ptr(cb2),
             ptr(fw), stream_ptr())
    call("tdeed_gsf_apply_fwd", ptr(x), ptr(gate), ptr(fw), B, T, h, w, C, F, Fp, ptr(out), dc, stream_ptr())
    return out


def gs_source_order(F):
    """Source channel of every output channel of the gate-shift module's interleave (impl/gsf.py:88-91: inside each half,
    c = i*(F/4)+j -> 2j+i): module_out[:, co] = src_order_out[:, gs_source_order(F)[co]]."""
    Fh, Fq = F // 2, F // 4
    return [g * Fh + (col & 1) * Fq + (col >> 1) for g in range(2) for col in range(Fh)]


def avgpool_posenc(x, B, T, temp_enc, out=None, rowstat=None):
    """rowstat: optional fp32 (B*T, 2) output, LayerNorm mean / rstd over C of every feature row."""
    N, h, w, C = x.shape
    if out is None:
        out = torch.empty((B, T, C), dtype=x.dtype, device=x.device)
    call("tdeed_avgpool_posenc_fwd", ptr(x), B, T, h * w, C, ptr(temp_enc), ptr(out), ptr(rowstat), dtype_code(x.dtype),
         dtype_code(out.dtype), stream_ptr())
    return out


def layernorm(x, w, b, eps=1e-5, out=None, ldy=None, rows=None, C=None, ldx=None):
    C = x.shape[-1] if C is None else C
    rows = x.numel() // x.shape[-1] if rows is None else rows
    if out is None:
        out = torch.empty_like(x)
    call("tdeed_layernorm_fwd", ptr(x), (C if ldx is None else ldx), rows, C, ptr(w), ptr(b), eps, ptr(out),
         (C if ldy is None else ldy), dtype_code(x.dtype), stream_ptr())
    return out


def sgp_branch(o, x, ks, up, dw, db, out=None):
    B, T, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    call("tdeed_sgp_branch_fwd", ptr(o), ptr(x), B, T, C, ks, up, ptr(dw), ptr(db), ptr(out), dtype_code(x.dtype),
         stream_ptr())
    return out


def mixer_branch(xn, cat, T_hi, ks, up, dw1, db1, dw2, db2):
    B, T_lo, C = xn.shape
    call("tdeed_mixer_branch_fwd", ptr(xn), B, T_hi, T_lo, C, ks, up, ptr(dw1), ptr(db1), ptr(dw2), ptr(db2),
         ptr(cat), dtype_code(xn.dtype), stream_ptr())
    return cat


def _rs_parts(rowstat):
    """rowstat (rows, 2) = (mean, rstd) -> 0; (n, rows, 2) = partial (sum, sum of squares) per column tile -> n"""
    return 0 if rowstat is None or rowstat.dim() == 2 else int(rowstat.shape[0])


def sgp_front(x, ks, up, ln_w, ln_b, dw, db, eps=1e-5, out=None, chsum=None, rowstat=None, out16=None):
    """SGPBlock front half with the LayerNorm computed in-kernel: y = x + LN(x) + fc*phi + (convw+convkw)*psi.
    chsum: optional fp32 (B, C, 2) output, per-channel sum / sum of squares over T of y (for sgp_gemm_gn_gelu's GroupNorm);
    rowstat: optional fp32 (B*T, 2) input, LayerNorm statistics of every row of x: (mean, rstd) as avgpool_posenc leaves them, or (n, B*T, 2) partial (sum, sum of
    squares) per column tile as sgp_gemm_residual does."""
    B, T, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    call("tdeed_sgp_front_fwd", ptr(x), B, T, C, ks, up, ptr(ln_w), ptr(ln_b), eps, ptr(dw), ptr(db), ptr(out),
         ptr(chsum), ptr(rowstat), _rs_parts(rowstat), ptr(out16), dtype_code(x.dtype), stream_ptr())
    return out


def mixer_front(z, xlo, cat, ks, up, ln1_w, ln1_b, ln2_w, ln2_b, dw1, db1, dw2, db2, eps=1e-5, rowstat_z=None,
                rowstat_x=None):
    """SGPMixer front half with both LayerNorms in-kernel: fills all six slabs of cat (B, T_hi, 6C)."""
    B, T_hi, C = z.shape
    T_lo = xlo.shape[1]
    call("tdeed_mixer_front_fwd", ptr(z), ptr(xlo), B, T_hi, T_lo, C, ks, up, ptr(ln1_w), ptr(ln1_b), ptr(ln2_w),
         ptr(ln2_b), eps, ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(cat), ptr(rowstat_z), _rs_parts(rowstat_z),
         ptr(rowstat_x), _rs_parts(rowstat_x), dtype_code(z.dtype), dtype_code(cat.dtype), stream_ptr())
    return cat


def groupnorm(x, G, w, b, eps=1e-5, out=None):
    B, T, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    call("tdeed_groupnorm_fwd", ptr(x), B, T, C, G, ptr(w), ptr(b), eps, ptr(out), dtype_code(x.dtype), stream_ptr())
    return out


def maxpool(x, T_out, out=None):
    B, T_in, C = x.shape
    if out is None:
        out = torch.empty((B, T_out, C), dtype=x.dtype, device=x.device)
    call("tdeed_maxpool_fwd", ptr(x), B, T_in, T_out, C, ptr(out), dtype_code(x.dtype), stream_ptr())
    return out


def maxpool_rowstat(x, T_out, out=None, rowstat=None, eps=1e-5):
    """AdaptiveMaxPool1d(T_out) along T of (B,T,C) + the LayerNorm (mean, rstd) of every pooled row in rowstat (B*T_out, 2)"""
    B, T_in, C = x.shape
    if out is None:
        out = torch.empty((B, T_out, C), dtype=x.dtype, device=x.device)
    if rowstat is None:
        rowstat = torch.empty((B * T_out, 2), dtype=torch.float32, device=x.device)
    call("tdeed_maxpool_rowstat_fwd", ptr(x), B, T_in, T_out, C, ptr(out), ptr(rowstat), eps, dtype_code(x.dtype), stream_ptr())
    return out, rowstat


def heads(x, w, b, out=None):
    rows = x.numel() // x.shape[-1]
    C = x.shape[-1]
    n_out = w.shape[0]
    if out is None:
        out = torch.empty((rows, n_out), dtype=torch.float32, device=x.device)
    call("tdeed_heads_fwd", ptr(x), rows, C, ptr(w), ptr(b), n_out, ptr(out), dtype_code(x.dtype), stream_ptr())
    return out


def _chk_labels(head_out, hard, soft, labelD, K):
    """Host-side argument checks of the loss entry points (dtype / contiguity / shape; no device sync).  Label VALUES are
    checked by the kernels: a label outside [0, K) is never used as an index and turns the loss into NaN."""
    _chk(head_out, "head_out", torch.float32)
    rows = head_out.shape[0]
    if hard is not None:
        _chk(hard, "labels", torch.int64)
        if hard.numel() != rows:
            raise ValueError(f"labels: {hard.numel()} entries for {rows} rows")
    if soft is not None:
        _chk(soft, "soft labels", torch.float32)
        if soft.numel() != rows * K:
            raise ValueError(f"soft labels: {tuple(soft.shape)} for {rows} rows x {K} classes")
    if labelD is not None:
        _chk(labelD, "labelD", torch.float32)
        if labelD.numel() != rows:
            raise ValueError(f"labelD: {labelD.numel()} entries for {rows} rows")
    if hard is None and soft is None:
        raise ValueError("loss needs hard or soft labels")


def loss(head_out, K1, cls_w, hard=None, soft=None, displ_col=-1, labelD=None, out=None):
    rows, ld = head_out.shape
    _chk_labels(head_out, hard, soft, labelD, K1)
    _chk(cls_w, "cls_w", torch.float32)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=head_out.device)
    call("tdeed_loss_fwd", ptr(head_out), rows, ld, K1, ptr(hard), ptr(soft), ptr(cls_w), displ_col, ptr(labelD),
         ptr(out), stream_ptr())
    return out


def loss_bwd(head_out, K1, cls_w, hard=None, soft=None, displ_col=-1, labelD=None, grad_scale=1.0):
    """d(CE+MSE)/d(head_out) (rows, ld) fp32."""
    rows, ld = head_out.shape
    _chk_labels(head_out, hard, soft, labelD, K1)
    dhead = torch.empty_like(head_out)
    call("tdeed_loss_bwd", ptr(head_out), rows, ld, K1, ptr(hard), ptr(soft), ptr(cls_w), displ_col, ptr(labelD),
         float(grad_scale), ptr(dhead), stream_ptr())
    return dhead


def check_kd(alpha, temperature, displ_weight):
    """Ranges of the distillation settings -> (alpha, temperature, displ_weight) as floats; ValueError outside them."""
    alpha, temperature, displ_weight = float(alpha), float(temperature), float(displ_weight)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1], got {alpha}")
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError(f"temperature must be positive and finite, got {temperature}")
    if not (displ_weight >= 0.0 and displ_weight < float("inf")):
        raise ValueError(f"displ_weight must be non-negative and finite, got {displ_weight}")
    return alpha, temperature, displ_weight


def loss_kd(head_out, K1, cls_w, teacher, hard=None, soft=None, displ_col=-1, labelD=None, teacher_displ_col=-1, alpha=0.5,
            temperature=2.0, displ_weight=0.0, grad_scale=1.0, want_grad=True):
    """Distillation loss, value and gradient in one launch -> (out5 [total, ce, mse, kd, kd_displ], dhead (rows, ld) | None).
    total = (1-alpha) ce + mse + alpha kd + displ_weight kd_displ with ce / mse the terms of loss() and
    kd = temperature^2 * KL(softmax(teacher / temperature) || softmax(logits / temperature)) averaged over the rows,
    kd_displ = mean (d - d_teacher)^2.  teacher: the teacher's head buffer (rows, ld_t) fp32, read in place: its first K1
    columns are the class logits, column teacher_displ_col (or -1) its displacement."""
    alpha, temperature, displ_weight = check_kd(alpha, temperature, displ_weight)
    if head_out.dim() != 2 or teacher.dim() != 2:
        raise ValueError("loss_kd: head_out (rows, ld) and teacher (rows, ld_t)")
    rows, ld = head_out.shape
    ld_t = teacher.shape[1]
    if teacher.shape[0] != rows:
        raise ValueError(f"teacher: {teacher.shape[0]} rows for {rows} rows")
    if not 0 < K1 <= min(ld, ld_t):
        raise ValueError(f"loss_kd: {K1} classes in heads of {ld} and {ld_t} (teacher) columns")
    if not (-1 <= displ_col < ld and -1 <= teacher_displ_col < ld_t):
        raise ValueError(f"loss_kd: displacement columns {displ_col} / {teacher_displ_col} outside heads of {ld} / {ld_t} columns")
    if displ_weight > 0.0 and (displ_col < 0 or teacher_displ_col < 0):
        raise ValueError("loss_kd: displ_weight > 0 needs a displacement column in both heads")
    if cls_w.numel() < K1:
        raise ValueError(f"cls_w: {cls_w.numel()} weights for {K1} classes")
    _chk_labels(head_out, hard, soft, labelD, K1)
    _chk(cls_w, "cls_w", torch.float32)
    _chk(teacher, "teacher", torch.float32)
    if teacher.device != head_out.device:
        raise ValueError(f"teacher on {teacher.device}, head_out on {head_out.device}")
    out = torch.empty(5, dtype=torch.float32, device=head_out.device)
    dhead = torch.empty_like(head_out) if want_grad else None
    call("tdeed_loss_kd", ptr(head_out), rows, ld, K1, ptr(hard), ptr(soft), ptr(cls_w), displ_col, ptr(labelD), ptr(teacher),
         ld_t, teacher_displ_col, alpha, temperature, displ_weight, float(grad_scale), ptr(out), ptr(dhead), stream_ptr())
    return out, dhead


def check_loss_options(label_smoothing=0.0, focal_gamma=0.0, class_weights=None, K1=None):
    """Ranges and shapes of the loss options -> (label_smoothing, focal_gamma as floats, class_weights as a tuple of K1
    floats or None); ValueError with the offending value outside them: 0 <= label_smoothing <= 1, focal_gamma >= 0 and
    finite, class_weights a vector of K1 finite non-negative numbers."""
    eps, gamma = float(label_smoothing), float(focal_gamma)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1], got {eps}")
    if not (gamma >= 0.0 and gamma < float("inf")):
        raise ValueError(f"focal_gamma must be non-negative and finite, got {gamma}")
    if class_weights is not None:
        w = torch.as_tensor(class_weights).detach().cpu().double()
        if w.dim() != 1 or (K1 is not None and w.numel() != K1) or w.numel() == 0:
            raise ValueError(f"class_weights must be a vector of {K1 if K1 is not None else 'K1'} weights, got shape "
                             f"{tuple(w.shape)}")
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError(f"class_weights must be finite and non-negative, got {w.tolist()}")
        class_weights = tuple(w.tolist())
    return eps, gamma, class_weights


def loss_opt(head_out, K1, cls_w, teacher=None, hard=None, soft=None, displ_col=-1, labelD=None, teacher_displ_col=-1,
             alpha=0.0, temperature=1.0, displ_weight=0.0, label_smoothing=0.0, focal_gamma=0.0, grad_scale=1.0,
             want_grad=True):
    """The loss with its options, value and gradient in one launch -> (out5 [total, ce, mse, kd, kd_displ], dhead (rows, ld)
    | None):  ce = sum_r sum_c w_c t'_c (1 - p_c)^focal_gamma (-log p_c) / den  with t' = (1 - label_smoothing) t +
    label_smoothing / K1 (t the one-hot of the hard label or the soft row) and den = sum_r w[y_r] (hard) or rows (soft), so
    focal_gamma = 0 is F.cross_entropy(weight=cls_w, label_smoothing=).  cls_w: K1 free per-class weights.  With a
    teacher head (rows, ld_t) the distillation terms of loss_kd() on top (total = (1-alpha) ce + mse + alpha kd +
    displ_weight kd_displ); without one kd = kd_displ = 0 and alpha / displ_weight must be 0.  Neutral options give the bits
    of loss_kd(), without a teacher those of loss() + loss_bwd()."""
    label_smoothing, focal_gamma, _ = check_loss_options(label_smoothing, focal_gamma)
    if head_out.dim() != 2:
        raise ValueError("loss_opt: head_out (rows, ld)")
    rows, ld = head_out.shape
    ld_t = 0
    if teacher is None:
        if float(alpha) != 0.0 or float(displ_weight) != 0.0:
            raise ValueError(f"loss_opt: alpha {alpha} / displ_weight {displ_weight} without a teacher")
        alpha, temperature, displ_weight, teacher_displ_col = 0.0, 1.0, 0.0, -1
    else:
        alpha, temperature, displ_weight = check_kd(alpha, temperature, displ_weight)
        if teacher.dim() != 2 or teacher.shape[0] != rows:
            raise ValueError(f"teacher: {tuple(teacher.shape)} for {rows} rows")
        ld_t = teacher.shape[1]
        if not 0 < K1 <= ld_t:
            raise ValueError(f"loss_opt: {K1} classes in a teacher head of {ld_t} columns")
        if not -1 <= teacher_displ_col < ld_t:
            raise ValueError(f"loss_opt: displacement column {teacher_displ_col} outside a teacher head of {ld_t} columns")
        if displ_weight > 0.0 and (displ_col < 0 or teacher_displ_col < 0):
            raise ValueError("loss_opt: displ_weight > 0 needs a displacement column in both heads")
        _chk(teacher, "teacher", torch.float32)
        if teacher.device != head_out.device:
            raise ValueError(f"teacher on {teacher.device}, head_out on {head_out.device}")
    if not 0 < K1 <= ld:
        raise ValueError(f"loss_opt: {K1} classes in a head of {ld} columns")
    if not -1 <= displ_col < ld:
        raise ValueError(f"loss_opt: displacement column {displ_col} outside a head of {ld} columns")
    if cls_w.numel() < K1:
        raise ValueError(f"cls_w: {cls_w.numel()} weights for {K1} classes")
    _chk_labels(head_out, hard, soft, labelD, K1)
    _chk(cls_w, "cls_w", torch.float32)
    out = torch.empty(5, dtype=torch.float32, device=head_out.device)
    dhead = torch.empty_like(head_out) if want_grad else None
    call("tdeed_loss_opt", ptr(head_out), rows, ld, K1, ptr(hard), ptr(soft), ptr(cls_w), displ_col, ptr(labelD), ptr(teacher),
         ld_t, teacher_displ_col, alpha, temperature, displ_weight, label_smoothing, focal_gamma, float(grad_scale), ptr(out),
         ptr(dhead), stream_ptr())
    return out, dhead


def loss2(head_out, B, T, K1a, K1b, dataset, hard, cls_w, displ_col=-1, labelD=None, want_grad=False, grad_scale=1.0,
          soft=None):
    """Double-head (joint dataset) loss of model.py:278-306 -> (out[3], dhead | None).  hard: int64 labels over the
    concatenated heads, or soft: (B*T, K1a+K1b) fp32 label distributions (mixup)."""
    ld = head_out.shape[-1]
    _chk_labels(head_out, hard, soft, labelD, K1a + K1b)
    _chk(dataset, "dataset", torch.int64)
    if dataset.numel() != B or cls_w.numel() < max(K1a, K1b):
        raise ValueError("loss2: dataset needs one id per clip, cls_w max(K1a, K1b) weights")
    out = torch.empty(3, dtype=torch.float32, device=head_out.device)
    dhead = torch.empty_like(head_out) if want_grad else None
    call("tdeed_loss2", ptr(head_out), B, T, ld, K1a, K1b, ptr(dataset), ptr(hard), ptr(soft), ptr(cls_w), displ_col,
         ptr(labelD), float(grad_scale), ptr(out), ptr(dhead), stream_ptr())
    return out, dhead


def loss2_soft(head_out, B, T, K1a, K1b, dataset, soft, cls_w, displ_col=-1, labelD=None, grad_scale=1.0):
    return loss2(head_out, B, T, K1a, K1b, dataset, None, cls_w, displ_col, labelD, True, grad_scale, soft=soft)


def heads_bwd(dout, x, w, need_dx=True):
    """FCLayers backward: returns (dx | None, dw (n_out,C) fp32, db (n_out,) fp32)."""
    rows, n_out = dout.shape
    C = x.shape[-1]
    ws = torch.empty(_lib.load().tdeed_heads_bwd_workspace(rows, C, n_out), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty((n_out, C), dtype=torch.float32, device=x.device)
    db = torch.empty((n_out,), dtype=torch.float32, device=x.device)
    call("tdeed_heads_bwd", ptr(dout), ptr(x), rows, C, ptr(w), n_out, ptr(dx), ptr(dw), ptr(db), ptr(ws),
         dtype_code(x.dtype), stream_ptr())
    return dx, dw, db


def adamw_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
               grad_scale=1.0):
    """In-place fused AdamW on flat fp32 buffers (torch.optim.AdamW semantics)."""
    for t_ in (param, grad, exp_avg, exp_avg_sq):
        _chk(t_, "adamw buffer", torch.float32)
    call("tdeed_adamw_step", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
         float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale), stream_ptr())
    return param


GUARD_WORDS = 8        # the guard record of tdeed_grad_guard as int32 words: [sumsq lo, hi, nonfinite, skipped, 4 reserved]


def grad_guard_ws(n, device):
    """The workspace tdeed_grad_guard wants for a flat buffer of n elements (one binary64 partial per workgroup)."""
    return torch.empty(_lib.load().tdeed_grad_guard_ws_bytes(int(n)) // 8, dtype=torch.float64, device=device)


def grad_guard(grad, guard, ws, skip_nonfinite=False):
    """Statistics of the flat fp32 gradient buffer into the 32-byte record `guard` (int32 (8,), zero before the first call):
    binary64 sum of squares, non-finite flag and, with skip_nonfinite, the cumulative count of skipped steps."""
    _chk(grad, "grad_guard buffer", torch.float32)
    _chk(guard, "guard record", torch.int32)
    _chk(ws, "grad_guard workspace", torch.float64)
    if guard.numel() != GUARD_WORDS or ws.numel() * 8 < _lib.load().tdeed_grad_guard_ws_bytes(grad.numel()):
        raise ValueError("grad_guard: the record is 8 int32 words, the workspace grad_guard_ws(n) elements")
    call("tdeed_grad_guard", ptr(grad), grad.numel(), int(bool(skip_nonfinite)), ptr(guard), ptr(ws), stream_ptr())
    return guard


def adamw_step_guarded(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
                       grad_scale=1.0, guard=None, skip_nonfinite=False, max_grad_norm=None):
    """adamw_step behind the record grad_guard wrote for `grad`: nothing is written when skip_nonfinite is set and the
    gradient held an inf / NaN; max_grad_norm clips by the global norm (clip_grad_norm_'s rule); `step` counts attempts."""
    for t_ in (param, grad, exp_avg, exp_avg_sq):
        _chk(t_, "adamw buffer", torch.float32)
    _chk(guard, "guard record", torch.int32)
    if guard is None or guard.numel() != GUARD_WORDS:
        raise ValueError("adamw_step_guarded: needs the record grad_guard wrote (8 int32 words)")
    call("tdeed_adamw_step_guarded", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
         float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale), ptr(guard),
         int(bool(skip_nonfinite)), 0.0 if max_grad_norm is None else float(max_grad_norm), stream_ptr())
    return param


ADAMW_MAX_RUNS = 16384   # csrc/train.hip: the run ends of one table are staged in LDS


def adamw_run_table(runs, n, device):
    """The device table of tdeed_adamw_step_groups for a flat buffer of n elements: int32 (R, 4) holding, per run,
    [end in 16-byte chunks, lr_scale bits, weight_decay bits, frozen].  runs: (end_element, lr_scale, weight_decay | None,
    frozen) ascending and covering [0, n), as optim.group_table returns them; None stands for the launch's weight decay.
    Every boundary but the last must be a multiple of 4 elements (a run never splits a 16-byte chunk)."""
    import numpy as np
    runs = list(runs)
    if not 1 <= len(runs) <= ADAMW_MAX_RUNS:
        raise ValueError(f"adamw_run_table: 1 .. {ADAMW_MAX_RUNS} runs, got {len(runs)}")
    tab = np.zeros((len(runs), 4), dtype=np.int32)
    prev = 0
    for i, (end, scale, wd, frozen) in enumerate(runs):
        end, scale = int(end), float(scale)
        wd = -1.0 if wd is None else float(wd)
        last = i == len(runs) - 1
        if not prev < end <= n or (end % 4 and not last):
            raise ValueError(f"adamw_run_table: run {i} ends at {end} (previous end {prev}, n {n}): ends ascend in "
                             f"multiples of 4 elements")
        if not (scale >= 0 and scale < float("inf")) or wd != wd or wd == float("inf") or (wd < 0 and wd != -1.0):
            raise ValueError(f"adamw_run_table: run {i}: lr_scale {scale} / weight_decay {wd} must be finite and >= 0")
        tab[i, 0] = (end + 3) // 4
        tab[i, 1:3] = np.array([scale, wd], dtype=np.float32).view(np.int32)
        tab[i, 3] = int(bool(frozen))
        prev = end
    if prev != n:
        raise ValueError(f"adamw_run_table: the runs end at {prev}, the buffer at {n}")
    return torch.from_numpy(tab).to(device)


def adamw_step_groups(param, grad, exp_avg, exp_avg_sq, step, lr, run_table, betas=(0.9, 0.999), eps=1e-8,
                      weight_decay=0.01, grad_scale=1.0, guard=None, skip_nonfinite=False, max_grad_norm=None):
    """adamw_step over the runs of `run_table` (adamw_run_table): a run steps at lr * lr_scale with its own weight decay, a
    frozen run is neither read nor written.  guard: the record grad_guard wrote for `grad` (adamw_step_guarded's
    semantics over the whole buffer), or None for the unguarded form."""
    for t_ in (param, grad, exp_avg, exp_avg_sq):
        _chk(t_, "adamw buffer", torch.float32)
        if t_.numel() != param.numel():
            raise ValueError("adamw_step_groups: param, grad, exp_avg and exp_avg_sq must have one length")
    _chk(run_table, "adamw run table", torch.int32)
    if run_table.dim() != 2 or run_table.shape[1] != 4 or not 1 <= run_table.shape[0] <= ADAMW_MAX_RUNS:
        raise ValueError("adamw_step_groups: the run table is int32 (R, 4) as adamw_run_table builds it")
    if guard is not None:
        _chk(guard, "guard record", torch.int32)
        if guard.numel() != GUARD_WORDS:
            raise ValueError("adamw_step_groups: the guard is the record grad_guard wrote (8 int32 words)")
    call("tdeed_adamw_step_groups", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
         float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale), ptr(guard),
         int(bool(skip_nonfinite)), 0.0 if max_grad_norm is None else float(max_grad_norm), ptr(run_table),
         int(run_table.shape[0]), stream_ptr())
    return param


def adamw_step_ema(param, grad, exp_avg, exp_avg_sq, step, lr, ema, ema_decay, ema_warmup=False, ema_step0=0, run_table=None,
                   betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=1.0, guard=None, skip_nonfinite=False,
                   max_grad_norm=None):
    """adamw_step / adamw_step_guarded (guard) / adamw_step_groups (run_table) with the shadow `ema` updated in the same
    launch from the parameter it has just computed: e += (1 - d_n) (p_new - e), optim.ema_ref's arithmetic, at
    n = (step - skipped) - ema_step0.  A skipped step and a frozen run leave the shadow untouched."""
    for t_ in (param, grad, exp_avg, exp_avg_sq, ema):
        _chk(t_, "adamw buffer", torch.float32)
        if t_.numel() != param.numel():
            raise ValueError("adamw_step_ema: param, grad, exp_avg, exp_avg_sq and ema must have one length")
    nruns = 0
    if run_table is not None:
        _chk(run_table, "adamw run table", torch.int32)
        if run_table.dim() != 2 or run_table.shape[1] != 4 or not 1 <= run_table.shape[0] <= ADAMW_MAX_RUNS:
            raise ValueError("adamw_step_ema: the run table is int32 (R, 4) as adamw_run_table builds it")
        nruns = int(run_table.shape[0])
    if guard is not None:
        _chk(guard, "guard record", torch.int32)
        if guard.numel() != GUARD_WORDS:
            raise ValueError("adamw_step_ema: the guard is the record grad_guard wrote (8 int32 words)")
    call("tdeed_adamw_step_ema", ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
         float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale), ptr(guard),
         int(bool(skip_nonfinite)), 0.0 if max_grad_norm is None else float(max_grad_norm), ptr(run_table), nruns,
         ptr(ema), float(ema_decay), int(bool(ema_warmup)), int(ema_step0), stream_ptr())
    return param


class EmaTensorTable:
    """The row table of tdeed_ema_tensors: `.dev` int32 (R, 4) on the device, `.host` the same rows as numpy (what the
    entry checks against the shadow's length), `.total` the shadow elements the rows cover, `.offsets` / `.counts` per row;
    `.keep` holds the source tensors so that the pointers in the table stay valid."""

    def __init__(self, dev, host, offsets, counts, keep):
        self.dev, self.host, self.offsets, self.counts, self.keep = dev, host, offsets, counts, keep
        self.total = max((o + c for o, c in zip(offsets, counts)), default=0)


def ema_tensor_table(tensors, offsets=None):
    """Row table for `ema_tensors`: one row {src pointer, offset, count} per tensor (fp32, contiguous, on one device; views
    at 4-byte-aligned offsets of larger buffers are fine).  offsets: the first shadow element of each row; default: the
    rows packed back to back in the order given.  Written on the host once, uploaded once."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("ema_tensor_table: no tensors")
    for t_ in tensors:
        _chk(t_, "ema source", torch.float32)
        if t_.numel() < 1 or t_.numel() >= 1 << 31:
            raise ValueError("ema_tensor_table: a row holds 1 .. 2^31 - 1 elements")
    counts = [int(t_.numel()) for t_ in tensors]
    if offsets is None:
        offsets = [int(x) for x in np.cumsum([0] + counts[:-1])]
    offsets = [int(o) for o in offsets]
    if len(offsets) != len(tensors) or any(o < 0 or o + c >= 1 << 31 for o, c in zip(offsets, counts)):
        raise ValueError("ema_tensor_table: one offset >= 0 per tensor, offset + count below 2^31")
    host = np.zeros((len(tensors), 4), dtype=np.int32)
    host[:, :2] = np.array([t_.data_ptr() for t_ in tensors], dtype=np.uint64).view(np.int32).reshape(-1, 2)
    host[:, 2] = offsets
    host[:, 3] = counts
    return EmaTensorTable(torch.from_numpy(host).to(tensors[0].device), host, offsets, counts, tensors)


def ema_tensors(table, shadow, step, ema_decay, ema_warmup=False, ema_step0=0, guard=None, skip_nonfinite=False):
    """shadow[offset + i] += (1 - d_n) (src[i] - shadow[offset + i]) for every row of `table` (ema_tensor_table) in one
    launch, optim.ema_ref's arithmetic at n = (step - skipped) - ema_step0; with the record of grad_guard a skipped step
    leaves the shadow untouched.  A row that does not lie inside `shadow` is refused."""
    _chk(shadow, "ema shadow", torch.float32)
    if guard is not None:
        _chk(guard, "guard record", torch.int32)
        if guard.numel() != GUARD_WORDS:
            raise ValueError("ema_tensors: the guard is the record grad_guard wrote (8 int32 words)")
    call("tdeed_ema_tensors", ptr(table.dev), table.host.ctypes.data, int(table.host.shape[0]), ptr(shadow),
         shadow.numel(), int(step), ptr(guard), int(bool(skip_nonfinite)), float(ema_decay), int(bool(ema_warmup)),
         int(ema_step0), stream_ptr())
    return shadow


def process_prediction(head_out, B, T, K1, displ_col, out=None):
    """out: optional contiguous fp32 (B,T,K1) tensor (e.g. a slice of a per-video score buffer) to write the scores into."""
    ld = head_out.shape[-1]
    if out is None:
        scores = torch.empty((B, T, K1), dtype=torch.float32, device=head_out.device)
    else:
        if out.dtype != torch.float32 or tuple(out.shape) != (B, T, K1) or not out.is_contiguous():
            raise ValueError(f"process_prediction: out must be a contiguous float32 {(B, T, K1)} tensor")
        scores = out
    cls = torch.empty((B, T), dtype=torch.int64, device=head_out.device)
    call("tdeed_process_prediction", ptr(head_out), B, T, ld, K1, displ_col, ptr(scores), ptr(cls), stream_ptr())
    return cls, scores


def clip_gather(video_u8, starts_dev, T, out):
    """out[b*T + t] = video_u8[starts[b] + t], zero frames outside [0, L) (the evaluation reader's padding).
    video_u8: uint8 (L, ...) on the device; starts_dev: int32 (B,) on the device; out: uint8 buffer of B*T frames."""
    if video_u8.dtype != torch.uint8 or out.dtype != torch.uint8 or starts_dev.dtype != torch.int32:
        raise TypeError("clip_gather: uint8 frames and int32 starts")
    if not (video_u8.is_contiguous() and out.is_contiguous() and starts_dev.is_contiguous()):
        raise ValueError("clip_gather: contiguous tensors only")
    L, B = video_u8.shape[0], starts_dev.numel()
    fb = video_u8[0].numel()
    if out.numel() != B * T * fb:
        raise ValueError(f"clip_gather: out holds {out.numel()} bytes, {B} clips of {T} frames need {B * T * fb}")
    call("tdeed_clip_gather_u8", ptr(video_u8), L, fb, ptr(starts_dev), B, T, ptr(out), stream_ptr())
    return out


def _chk_track(mean, who):
    if not isinstance(mean, torch.Tensor) or mean.dtype != torch.float32:
        raise TypeError(f"{who}: the track must be a float32 tensor")
    if mean.dim() != 2 or mean.shape[0] < 1 or mean.shape[1] < 2 or not mean.is_contiguous():
        raise ValueError(f"{who}: the track must be a contiguous (L, K+1) tensor with L >= 1 and K >= 1")
    return int(mean.shape[0]), int(mean.shape[1])


def _one_video(dev, *ends):
    """the offset table [0, end] of a group of one video, per end, as int32 tensors on dev"""
    tab = torch.tensor([x for e in ends for x in (0, int(e))], dtype=torch.int32, device=dev)
    return [tab[2 * i:2 * i + 2] for i in range(len(ends))]


# ---- one video: conveniences over the group functions below (a video is a group of one; tests and tools use them)
def stitch_scores(clip_scores, starts_dev, L, count_all=None, track_sum=None, support=None, mean=False):
    """clip_scores fp32 (V,n,T,K1), starts_dev int32 (n,) on the device -> (track_sum (L,K1), support (L,) int32, mean
    (L,K1) | None): the device twin of evalutil.ScoreStitcher (add per clip for count_all=False, add_views per view for
    count_all=True; default: True when V > 1).  track_sum / support: accumulate onto these instead of fresh zeros."""
    seg_off, clip_off = _one_video(clip_scores.device, L, clip_scores.shape[1])
    return stitch_scores_seg(clip_scores, starts_dev, seg_off, clip_off, L, count_all, track_sum, support, mean)


def frame_events(mean, hr_threshold=0.01, pred_u8=None):
    """mean fp32 (L,K1) on the device (stitch_scores(..., mean=True)) -> (pred (L,) int32: arg-max column, first maximum
    like np.argmax; pred_score (L,) fp32 = mean[f, pred[f]]; first_frame (K1,) int32: per class c >= 1 the first frame with
    mean[f,c] >= float32(hr_threshold), L when there is none (and at index 0); count (K1,) int32: the number of such
    frames).  The comparison is in fp32, as numpy compares an fp32 array with a python float.
    pred_u8: optional uint8 (L,) tensor that receives pred once more, one byte per frame (K1 <= 256): what spot_video copies
    to the host."""
    L, _ = _chk_track(mean, "frame_events")
    pred, pred_score, first, count = frame_events_seg(mean, _one_video(mean.device, L)[0], L, hr_threshold, pred_u8)
    return pred, pred_score, first[0], count[0]


def nms_track(mean, window, threshold, soft, hr_threshold=0.01, first_frame=None, classes_u8=None):
    """Exact (soft) non-maximum suppression of a track's high-recall events on the device: what
    evalutil.non_maximum_suppression (soft=False) / soft_non_maximum_suppression (soft=True) keep of
    `evalutil.frame_events(...)[1]`, bit for bit (evalutil.nms_rounds states the kernel's order).
    mean fp32 (L,K1) on the device; window: an int for every class, or a list indexed like the reference's -- by the order in
    which labels first appear in the high-recall list; first_frame: frame_events(mean, hr_threshold)[2] when the caller has
    it already.  Returns device tensors (frames int32, classes int32, scores float64, count int32 (1,), rounds int32 (K1,)):
    the first `count` entries are the events, ascending frame and within a frame by label appearance; rounds[c] is the number
    of rounds class c took.  classes_u8: optional uint8 tensor of L*(K1-1) entries that receives the classes once more, one
    byte each.
    Raises ValueError for a soft window below 1, a negative window, or a window list with fewer than K1-1 entries -- the host
    only fails (IndexError) once more labels appear than the list has entries; this wrapper refuses the list up front."""
    L, K1 = _chk_track(mean, "nms_track")
    dev, cap = mean.device, L * (K1 - 1)
    if classes_u8 is not None and (classes_u8.dtype != torch.uint8 or classes_u8.numel() != cap or not classes_u8.is_contiguous()
                                   or classes_u8.device != dev):
        raise ValueError(f"nms_track: classes_u8 must be a contiguous uint8 tensor of {cap} entries on the track's device")
    seg_off = _one_video(dev, L)[0]
    if first_frame is None:
        first_frame = frame_events_seg(mean, seg_off, L, hr_threshold)[2]
    elif isinstance(first_frame, torch.Tensor) and first_frame.dim() == 1:
        first_frame = first_frame.unsqueeze(0)
    frames, cls8, scores, event_off, rounds = nms_track_seg(mean, seg_off, L, window, threshold, soft, first_frame, hr_threshold)
    if classes_u8 is not None:
        classes_u8.view(-1).copy_(cls8)
    return frames, cls8.to(torch.int32), scores, event_off[1:], rounds[0]


# ---- a group of videos packed one after the other (tables: evalutil.group_clip_table, int32 on the device)
MAX_GROUP_VIDEOS = 65535


def _chk_table(tab, n, dev, who, what):
    if not isinstance(tab, torch.Tensor) or tab.dtype != torch.int32 or tab.dim() != 1 or tab.numel() != n \
            or not tab.is_contiguous() or tab.device != dev:
        raise ValueError(f"{who}: {what} must be a contiguous int32 ({n},) tensor on the data's device")


def _chk_group(seg_off, dev, who):
    if not isinstance(seg_off, torch.Tensor) or seg_off.dtype != torch.int32:
        raise TypeError(f"{who}: seg_off must be an int32 tensor")
    nv = seg_off.numel() - 1
    if nv < 1:
        raise ValueError(f"{who}: seg_off needs at least two entries")
    if nv > MAX_GROUP_VIDEOS:
        raise ValueError(f"{who}: {nv} videos in one group, at most {MAX_GROUP_VIDEOS}")
    _chk_table(seg_off, nv + 1, dev, who, "seg_off")
    return nv


def _chk_windows(window, K1, soft, who):
    """window: an int for every class, or a list / tuple with an entry per class (K1 - 1 of them, further ones are ignored)
    -> the list of ints the C entry takes: one entry, or K1 - 1."""
    is_list = isinstance(window, (list, tuple))
    wins = [int(w) for w in window] if is_list else [int(window)]
    if is_list and len(wins) < K1 - 1:
        raise ValueError(f"{who}: a window list of {len(wins)} entries for {K1 - 1} classes")
    if any(w < (1 if soft else 0) or w > 1 << 30 for w in wins):
        raise ValueError(f"{who}: windows {wins}: soft suppression needs windows >= 1, hard suppression >= 0 (and at most 2^30)")
    return wins[:K1 - 1] if is_list and len(wins) > 1 else wins[:1]       # (K1 == 2: one class, the entry is its window)


def clip_gather_seg(video_u8, starts_dev, clip_base, clip_len_v, T, out):
    """clip_gather over several videos packed into video_u8 (sum L, ...): out[b*T + t] = video_u8[clip_base[b] + starts[b] + t]
    when 0 <= starts[b] + t < clip_len_v[b], a zero frame otherwise -- the window ends where the clip's own video ends.
    starts_dev / clip_base / clip_len_v: int32 (B,) on the device."""
    if video_u8.dtype != torch.uint8 or out.dtype != torch.uint8 or starts_dev.dtype != torch.int32:
        raise TypeError("clip_gather_seg: uint8 frames and int32 starts")
    if not (video_u8.is_contiguous() and out.is_contiguous() and starts_dev.is_contiguous()):
        raise ValueError("clip_gather_seg: contiguous tensors only")
    L, B = video_u8.shape[0], starts_dev.numel()
    _chk_table(starts_dev, B, video_u8.device, "clip_gather_seg", "starts")
    _chk_table(clip_base, B, video_u8.device, "clip_gather_seg", "clip_base")
    _chk_table(clip_len_v, B, video_u8.device, "clip_gather_seg", "clip_len_v")
    fb = video_u8[0].numel()
    if out.numel() != B * T * fb:
        raise ValueError(f"clip_gather_seg: out holds {out.numel()} bytes, {B} clips of {T} frames need {B * T * fb}")
    call("tdeed_clip_gather_seg_u8", ptr(video_u8), L, fb, ptr(starts_dev), ptr(clip_base), ptr(clip_len_v), B, T, ptr(out),
         stream_ptr())
    return out


def clip_gather_ring(ring_u8, ring_frames, L_total, starts_dev, clip_base, clip_len_v, T, out):
    """clip_gather_seg over a virtual packed buffer of L_total frames of which ring_u8 (ring_frames, ...) holds a window:
    packed frame p sits in ring_u8[p % ring_frames] (feeder.RingUpload).  The windows and their padding are clip_gather_seg's
    on the whole buffer.  That the frames a clip reads are live in the ring is the caller's duty (evalutil.ring_plan)."""
    if ring_u8.dtype != torch.uint8 or out.dtype != torch.uint8 or starts_dev.dtype != torch.int32:
        raise TypeError("clip_gather_ring: uint8 frames and int32 starts")
    if not (ring_u8.is_contiguous() and out.is_contiguous() and starts_dev.is_contiguous()):
        raise ValueError("clip_gather_ring: contiguous tensors only")
    ring_frames, L_total, B = int(ring_frames), int(L_total), starts_dev.numel()
    if ring_u8.shape[0] != ring_frames or ring_frames < 1 or L_total < 1:
        raise ValueError(f"clip_gather_ring: a ring of {ring_u8.shape[0]} rows for ring_frames={ring_frames}, L_total={L_total}")
    _chk_table(starts_dev, B, ring_u8.device, "clip_gather_ring", "starts")
    _chk_table(clip_base, B, ring_u8.device, "clip_gather_ring", "clip_base")
    _chk_table(clip_len_v, B, ring_u8.device, "clip_gather_ring", "clip_len_v")
    fb = ring_u8[0].numel()
    if out.numel() != B * T * fb:
        raise ValueError(f"clip_gather_ring: out holds {out.numel()} bytes, {B} clips of {T} frames need {B * T * fb}")
    call("tdeed_clip_gather_ring_u8", ptr(ring_u8), ring_frames, L_total, fb, ptr(starts_dev), ptr(clip_base), ptr(clip_len_v),
         B, T, ptr(out), stream_ptr())
    return out


def _chk_rows_gather(maps, starts_dev, L, pad_row, T, out, who):
    if not all(isinstance(t_, torch.Tensor) for t_ in (maps, starts_dev, out)):
        raise TypeError(f"{who}: tensors only")
    if maps.dtype != out.dtype or starts_dev.dtype != torch.int32:
        raise TypeError(f"{who}: maps and out of one dtype ({maps.dtype} / {out.dtype}) and int32 starts ({starts_dev.dtype})")
    if not (maps.is_contiguous() and out.is_contiguous()):
        raise ValueError(f"{who}: contiguous tensors only")
    if maps.dim() < 2 or not maps.is_cuda or out.device != maps.device:
        raise ValueError(f"{who}: maps (rows, ...) and out on one device")
    rows, B = maps.shape[0], starts_dev.numel()
    _chk_table(starts_dev, B, maps.device, who, "starts")
    if B < 1 or T < 1 or not (0 < L <= rows) or not (0 <= pad_row < rows):
        raise ValueError(f"{who}: {B} clips of {T} frames, {L} frames and pad_row {pad_row} in {rows} rows")
    rb = maps[0].numel() * maps.element_size()
    if out.numel() * out.element_size() != B * T * rb:
        raise ValueError(f"{who}: out holds {out.numel() * out.element_size()} bytes, {B} clips of {T} rows need {B * T * rb}")
    return rows, rb, B


def rows_gather(maps, starts_dev, L, pad_row, T, out):
    """out[b*T + t] = maps[starts[b] + t] when 0 <= starts[b] + t < L, maps[pad_row] otherwise: clip windows of per-frame rows
    (the trunk map of every frame of a video) with the row of a black frame as padding.  maps: (rows, ...) of any dtype on
    the device, rows >= L; starts_dev: int32 (B,) on the device; out: B*T rows of maps' dtype."""
    rows, rb, B = _chk_rows_gather(maps, starts_dev, L, pad_row, T, out, "rows_gather")
    call("tdeed_rows_gather", ptr(maps), rows, rb, int(L), int(pad_row), ptr(starts_dev), B, T, ptr(out), stream_ptr())
    return out


def rows_gather_seg(maps, starts_dev, clip_base, clip_len_v, L, pad_row, T, out):
    """rows_gather over the packed rows of several videos (clip_gather_seg's tables): out[b*T + t] = maps[clip_base[b] +
    starts[b] + t] when 0 <= starts[b] + t < clip_len_v[b], maps[pad_row] otherwise.  L: the packed total."""
    if (clip_base is None) != (clip_len_v is None):
        raise ValueError("rows_gather_seg: clip_base and clip_len_v go together")
    rows, rb, B = _chk_rows_gather(maps, starts_dev, L, pad_row, T, out, "rows_gather_seg")
    _chk_table(clip_base, B, maps.device, "rows_gather_seg", "clip_base")
    _chk_table(clip_len_v, B, maps.device, "rows_gather_seg", "clip_len_v")
    call("tdeed_rows_gather_seg", ptr(maps), rows, rb, int(L), int(pad_row), ptr(starts_dev), ptr(clip_base), ptr(clip_len_v),
         B, T, ptr(out), stream_ptr())
    return out


def stitch_scores_seg(clip_scores, starts_dev, seg_off, clip_off, L, count_all=None, track_sum=None, support=None, mean=False):
    """stitch_scores per video of a group: clip_scores fp32 (V,n,T,K1) of the group's clip list (video-major), starts_dev
    int32 (n,) video-local, seg_off / clip_off int32 (nv+1,) on the device, L = sum of the lengths.  -> (track_sum (sum L,K1), support (sum L,) int32,
    mean | None) over the packed frames; rows seg_off[v]:seg_off[v+1] carry the bits of stitch_scores on video v alone."""
    if not isinstance(clip_scores, torch.Tensor) or clip_scores.dim() != 4:
        raise TypeError("stitch_scores_seg: clip_scores must be a (V,n,T,K1) tensor")
    V, n, T, K1 = clip_scores.shape
    if clip_scores.dtype != torch.float32 or starts_dev.dtype != torch.int32 or not clip_scores.is_contiguous():
        raise TypeError("stitch_scores_seg: contiguous float32 scores and int32 starts")
    dev = clip_scores.device
    nv = _chk_group(seg_off, dev, "stitch_scores_seg")
    _chk_table(starts_dev, n, dev, "stitch_scores_seg", "starts")
    _chk_table(clip_off, nv + 1, dev, "stitch_scores_seg", "clip_off")
    L = int(L)
    if L < nv:
        raise ValueError(f"stitch_scores_seg: {L} packed frames for {nv} videos")
    if track_sum is None:
        track_sum = torch.zeros((L, K1), dtype=torch.float32, device=dev)
    if support is None:
        support = torch.zeros((L,), dtype=torch.int32, device=dev)
    if tuple(track_sum.shape) != (L, K1) or tuple(support.shape) != (L,) or track_sum.dtype != torch.float32 \
            or support.dtype != torch.int32 or not (track_sum.is_contiguous() and support.is_contiguous()) \
            or track_sum.device != dev or support.device != dev:
        raise ValueError("stitch_scores_seg: track_sum float32 (L,K1) and support int32 (L,), contiguous")
    mean_out = torch.empty((L, K1), dtype=torch.float32, device=dev) if mean else None
    ca = (V > 1) if count_all is None else bool(count_all)
    call("tdeed_stitch_scores_seg", ptr(clip_scores), V, n, T, K1, ptr(starts_dev), ptr(seg_off), ptr(clip_off), nv, int(ca), L,
         ptr(track_sum), ptr(support), ptr(mean_out), stream_ptr())
    return track_sum, support, mean_out


def stitch_live(ring_sum, ring_sup, clip_scores, starts_dev, count_all, lo, final_hi, limit, T=None, out=None):
    """stitch_scores for a stream whose length is not known yet, one launch per batch (evalutil's twin: liveplan.live_stitch_ref,
    the schedule: liveplan.LiveSchedule).  ring_sum fp32 (R,K1) / ring_sup int32 (R,): the state between launches, frame p in
    row p % R, zero before the first launch.  clip_scores fp32 (V,B,T,K1): the scores of this batch, starts_dev int32 (B,)
    ascending, on the device; both None for a launch that only emits rows (then T is needed).  lo / final_hi: rows final
    before / after this launch, limit: frames that exist.  -> (sums (final_hi - lo, K1), support (final_hi - lo,) int32, mean
    (final_hi - lo, K1)): the rows that became final, with the bits of stitch_scores over the whole clip list.  out: three
    tensors of those shapes to write into instead of fresh ones."""
    if not isinstance(ring_sum, torch.Tensor) or ring_sum.dtype != torch.float32 or ring_sum.dim() != 2 \
            or not ring_sum.is_contiguous() or not ring_sum.is_cuda:
        raise TypeError("stitch_live: ring_sum must be a contiguous float32 (R,K1) tensor on the device")
    R, K1 = ring_sum.shape
    dev = ring_sum.device
    _chk_table(ring_sup, R, dev, "stitch_live", "ring_sup")
    lo, final_hi, limit = int(lo), int(final_hi), int(limit)
    if not 0 <= lo <= final_hi <= limit or final_hi - lo > R:
        raise ValueError(f"stitch_live: rows [{lo}, {final_hi}) become final of {limit} frames in a ring of {R} rows")
    if clip_scores is None:
        if starts_dev is not None or T is None:
            raise ValueError("stitch_live: a launch without scores has no starts and needs T")
        V, B, T = 1, 0, int(T)
    else:
        if not isinstance(clip_scores, torch.Tensor) or clip_scores.dim() != 4 or clip_scores.dtype != torch.float32 \
                or not clip_scores.is_contiguous() or clip_scores.device != dev:
            raise TypeError("stitch_live: clip_scores must be a contiguous float32 (V,B,T,K1) tensor on the rings' device")
        V, B, Ts, k1 = clip_scores.shape
        if k1 != K1 or B < 1 or (T is not None and int(T) != Ts):
            raise ValueError(f"stitch_live: scores {tuple(clip_scores.shape)} for rings of {K1} columns and T={T}")
        T = Ts
        _chk_table(starts_dev, B, dev, "stitch_live", "starts")
    n = final_hi - lo
    if out is None:
        out = (torch.empty((n, K1), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev),
               torch.empty((n, K1), dtype=torch.float32, device=dev))
    sums, support, mean = out
    for x, shape, dt in ((sums, (n, K1), torch.float32), (support, (n,), torch.int32), (mean, (n, K1), torch.float32)):
        if not isinstance(x, torch.Tensor) or tuple(x.shape) != shape or x.dtype != dt or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"stitch_live: out must be contiguous (sums, support, mean) of {n} rows on the rings' device")
    call("tdeed_stitch_live", ptr(clip_scores), V, B, T, K1, ptr(starts_dev), int(bool(count_all)), lo, final_hi, limit, R,
         ptr(ring_sum), ptr(ring_sup), ptr(sums) if n else None, ptr(support) if n else None, ptr(mean) if n else None,
         stream_ptr())
    return sums, support, mean


def frame_events_seg(mean, seg_off, max_len, hr_threshold=0.01, pred_u8=None, first_init=None):
    """frame_events per video of a packed track: mean fp32 (sum L,K1), seg_off int32 (nv+1,) on the device, max_len the
    longest video (a host number).  -> (pred (sum L,) int32, pred_score (sum L,) fp32, first_frame (nv,K1) int32 in
    video-local frames, L_v where a class has no candidate, count (nv,K1) int32).  first_init: optional int32 (nv,K1) tensor
    already holding L_v in row v (a caller that uploads its tables anyway); it is written to and returned."""
    L, K1 = _chk_track(mean, "frame_events_seg")
    dev = mean.device
    nv = _chk_group(seg_off, dev, "frame_events_seg")
    max_len = int(max_len)
    if not 1 <= max_len <= L:
        raise ValueError(f"frame_events_seg: max_len {max_len} for {L} packed frames")
    if pred_u8 is not None:
        if K1 > 256:
            raise ValueError(f"frame_events_seg: {K1} columns do not fit a one-byte prediction")
        if pred_u8.dtype != torch.uint8 or tuple(pred_u8.shape) != (L,) or not pred_u8.is_contiguous() or pred_u8.device != dev:
            raise ValueError("frame_events_seg: pred_u8 must be a contiguous uint8 (L,) tensor on the track's device")
    if first_init is None:
        first = (seg_off[1:] - seg_off[:-1]).unsqueeze(1).repeat(1, K1)
    else:
        first = first_init
        if first.dtype != torch.int32 or tuple(first.shape) != (nv, K1) or not first.is_contiguous() or first.device != dev:
            raise ValueError("frame_events_seg: first_init must be a contiguous int32 (nv,K1) tensor on the track's device")
    pred = torch.empty((L,), dtype=torch.int32, device=dev)
    pred_score = torch.empty((L,), dtype=torch.float32, device=dev)
    count = torch.zeros((nv, K1), dtype=torch.int32, device=dev)
    call("tdeed_frame_events_seg", ptr(mean), ptr(seg_off), nv, L, max_len, K1, float(hr_threshold), ptr(pred), ptr(pred_u8),
         ptr(pred_score), ptr(first), ptr(count), stream_ptr())
    return pred, pred_score, first, count


def nms_track_seg(mean, seg_off, max_len, window, threshold, soft, first_frame, hr_threshold=0.01, planes=False):
    """nms_track per video of a packed track, one launch for the whole group: mean fp32 (sum L,K1), seg_off int32 (nv+1,),
    first_frame int32 (nv,K1) from frame_events_seg with the same hr_threshold; window / threshold / soft as nms_track
    (which is this function on a group of one video).
    Returns device tensors (frames int32, classes uint8, scores float64, event_off int32 (nv+1,), rounds int32 (nv,K1)):
    entries event_off[v]:event_off[v+1] are video v's kept events (video-local frames, nms_track's order), the lists of
    the videos following each other densely in video order.
    planes=True: the dense planes the kernel leaves behind follow as two more entries: emitted uint8 (K1,sum L), non-zero where
    class c keeps frame f, and kept_score float64 (K1,sum L), that event's score -- what ap_match_seg reads (row 0 is unused)."""
    L, K1 = _chk_track(mean, "nms_track_seg")
    dev = mean.device
    nv = _chk_group(seg_off, dev, "nms_track_seg")
    max_len = int(max_len)
    if not 1 <= max_len <= L:
        raise ValueError(f"nms_track_seg: max_len {max_len} for {L} packed frames")
    soft = bool(soft)
    wins = _chk_windows(window, K1, soft, "nms_track_seg")
    if not isinstance(first_frame, torch.Tensor) or first_frame.dtype != torch.int32 or tuple(first_frame.shape) != (nv, K1) \
            or not first_frame.is_contiguous() or first_frame.device != dev:
        raise ValueError("nms_track_seg: first_frame must be a contiguous int32 (nv,K1) tensor on the track's device")
    cap = L * (K1 - 1)
    ws_bytes = int(_lib.load().tdeed_nms_track_seg_workspace(L, max_len, K1))
    ws = torch.empty((ws_bytes // 8 + 1,), dtype=torch.float64, device=dev) if ws_bytes else None
    emitted = torch.empty((K1, L), dtype=torch.uint8, device=dev)
    kept = torch.empty((K1, L), dtype=torch.float64, device=dev)
    st_i = torch.empty((cap + nv,), dtype=torch.int32, device=dev)           # staged frames, then the nv list lengths
    st_c = torch.empty((cap,), dtype=torch.uint8, device=dev)
    st_s = torch.empty((cap,), dtype=torch.float64, device=dev)
    frames = torch.empty((cap,), dtype=torch.int32, device=dev)
    classes = torch.empty((cap,), dtype=torch.uint8, device=dev)
    scores = torch.empty((cap,), dtype=torch.float64, device=dev)
    event_off = torch.empty((nv + 1,), dtype=torch.int32, device=dev)
    rounds = torch.empty((nv, K1), dtype=torch.int32, device=dev)
    warr = (ctypes.c_int * len(wins))(*wins)
    call("tdeed_nms_track_seg", ptr(mean), ptr(seg_off), nv, L, max_len, K1, float(hr_threshold), float(threshold), int(soft),
         warr, len(wins), ptr(first_frame), ptr(ws), ptr(emitted), ptr(kept), ptr(st_i), ptr(st_c), ptr(st_s), ptr(st_i[cap:]),
         ptr(frames), ptr(classes), ptr(scores), ptr(event_off), ptr(rounds), stream_ptr())
    if planes:
        return frames, classes, scores, event_off, rounds, emitted, kept
    return frames, classes, scores, event_off, rounds


# ---- average precision of the spotted events on the device (ap.hip; evalutil.ap_restated is the written statement)
def ap_lds_frames():
    """longest video whose events ap_match_seg orders in LDS (longer ones are ordered in place in the store)"""
    return int(_lib.load().tdeed_ap_lds_frames())


def ap_max_tolerances():
    return int(_lib.load().tdeed_ap_max_tolerances())


def ap_max_truth(n_tol):
    """ground-truth frames one class may have in one video when n_tol tolerances are scored at once"""
    return int(_lib.load().tdeed_ap_max_truth(int(n_tol)))


def ap_tolerances(tolerances, who="ap_state"):
    """the tolerance list as ints: 1 .. ap_max_tolerances() whole numbers >= 0 (needs no device)"""
    tols = list(tolerances)
    if not 1 <= len(tols) <= ap_max_tolerances():
        raise ValueError(f"{who}: {len(tols)} tolerances, 1 to {ap_max_tolerances()} are scored at once")
    if any(int(t_) != t_ or not 0 <= int(t_) < 1 << 31 for t_ in tols):
        raise ValueError(f"{who}: tolerances {tols} must be whole numbers of frames >= 0")
    return [int(t_) for t_ in tols]


class ApState:
    """The device side of one mAP pass over a dataset (ap_state builds it): the tables of the videos and the truth, the
    ordered predictions of every (entry, class, video) and the hits of every (entry, tolerance, class, video)."""


def ap_state(lengths, truth, K1, n_entries, tolerances, device="cuda"):
    """lengths: frames of every video in ORDINAL order (the index of the video's name in sorted order); truth: {(ordinal,
    class index): [ground-truth frames in the truth record's list order, duplicates kept]}, classes 1 .. K1-1; n_entries:
    event lists scored side by side (the suppress entries); tolerances: in frames.  Uploads the tables once and allocates the
    stores ap_match_seg fills group by group: 12 bytes per frame, class and entry for the ordered predictions, 4 bytes per
    ground-truth frame, tolerance and entry for the hits."""
    tols = ap_tolerances(tolerances)
    lengths = [int(x) for x in lengths]
    NV, K1, E, T = len(lengths), int(K1), int(n_entries), len(tols)
    if NV < 1 or min(lengths) < 1 or sum(lengths) >= 1 << 31 or not 2 <= K1 <= 256 or E < 1 or NV * K1 >= 1 << 31:
        raise ValueError(f"ap_state: {NV} videos of {sum(lengths)} frames, {K1} columns, {E} entries")
    gt_off = np.zeros(NV * K1 + 1, np.int64)
    for (o, c), fr in truth.items():
        if not (0 <= int(o) < NV and 1 <= int(c) < K1):
            raise ValueError(f"ap_state: truth for video {o}, class {c} outside {NV} videos and the classes 1..{K1 - 1}")
        if any(int(f) != f or not 0 <= int(f) < 1 << 31 for f in fr):
            raise ValueError(f"ap_state: the ground-truth frames of video {o}, class {c} must be whole numbers >= 0")
        gt_off[int(o) * K1 + int(c) + 1] = len(fr)
    max_gt = int(gt_off.max())
    if max_gt > ap_max_truth(T):
        raise ValueError(f"ap_state: {max_gt} ground-truth frames of one class in one video, at most {ap_max_truth(T)} with {T} "
                         "tolerances")
    per_class = gt_off[1:].reshape(NV, K1).sum(axis=0)
    gt_off = np.cumsum(gt_off)
    G = int(gt_off[-1])
    if G >= 1 << 31:
        raise ValueError(f"ap_state: {G} ground-truth frames")
    frames = np.zeros(max(G, 1), np.int32)
    for (o, c), fr in truth.items():
        a = int(gt_off[int(o) * K1 + int(c)])
        frames[a:a + len(fr)] = np.asarray(fr, np.int64)
    st = ApState()
    st.NV, st.K1, st.E, st.T, st.G, st.max_gt, st.tolerances, st.lengths = NV, K1, E, T, G, max_gt, tols, lengths
    st.LT = sum(lengths)
    st.totals = [int(x) for x in per_class]
    st.vid_off_host = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
    st.vid_off, st.gt_off, st.gt_frames = up(st.vid_off_host), up(gt_off), up(frames)
    st.class_off = up(np.concatenate([[0], np.cumsum(per_class)]))
    dev = st.vid_off.device
    st.device = dev
    Gb = max(G, 1)
    st.ev_score = torch.empty((E, K1 - 1, st.LT), dtype=torch.float64, device=dev)
    st.ev_frame = torch.empty((E, K1 - 1, st.LT), dtype=torch.int32, device=dev)
    st.ev_count = torch.zeros((E, K1 - 1, NV), dtype=torch.int32, device=dev)
    st.hit_pos = torch.zeros((E, T, Gb), dtype=torch.int32, device=dev)
    st.hit_count = torch.zeros((E, T, NV * K1), dtype=torch.int32, device=dev)
    return st


def ap_match_seg(state, entry, mean, seg_off, ords, max_len, hr_threshold=0.01, planes=None):
    """Segment + match for one entry of one group of videos: mean fp32 (sum L,K1) the group's packed track, seg_off int32
    (nv+1,), ords int32 (nv,) the videos' ordinals in the dataset of `state`, all on the state's device; max_len the longest
    video (a host number).  planes=None: the raw high-recall list (mean[f,c] >= float32(hr_threshold), score
    float64(mean[f,c])); planes=(emitted, kept_score) of nms_track_seg(..., planes=True): that suppression's list.  Fills the
    state's stores for these videos (the launch is asynchronous on the current stream); nothing is returned."""
    if not isinstance(state, ApState):
        raise TypeError("ap_match_seg: state must come from ap_state")
    L, K1 = _chk_track(mean, "ap_match_seg")
    dev = mean.device
    nv = _chk_group(seg_off, dev, "ap_match_seg")
    _chk_table(ords, nv, dev, "ap_match_seg", "ords")
    max_len, entry = int(max_len), int(entry)
    if K1 != state.K1 or dev != state.device:
        raise ValueError(f"ap_match_seg: a track of {K1} columns on {dev} for a state of {state.K1} columns on {state.device}")
    if not 1 <= max_len <= L or L > state.LT or nv > state.NV:
        raise ValueError(f"ap_match_seg: max_len {max_len}, {L} packed frames, {nv} videos for a dataset of {state.LT} / {state.NV}")
    if not 0 <= entry < state.E:
        raise ValueError(f"ap_match_seg: entry {entry} of {state.E}")
    em = ks = None
    if planes is not None:
        em, ks = planes
        if em.dtype != torch.uint8 or ks.dtype != torch.float64 or tuple(em.shape) != (K1, L) or tuple(ks.shape) != (K1, L) \
                or not (em.is_contiguous() and ks.is_contiguous()) or em.device != dev or ks.device != dev:
            raise ValueError("ap_match_seg: planes are (emitted uint8 (K1,L), kept_score float64 (K1,L)), contiguous, on the track's device")
    tarr = (ctypes.c_int * state.T)(*state.tolerances)
    call("tdeed_ap_match_seg", ptr(mean), ptr(em), ptr(ks), ptr(seg_off), nv, L, max_len, K1, float(hr_threshold), ptr(ords),
         state.NV, ptr(state.vid_off), state.LT, ptr(state.gt_off), ptr(state.gt_frames), state.G, state.max_gt, tarr, state.T,
         ptr(state.ev_score[entry]), ptr(state.ev_frame[entry]), ptr(state.ev_count[entry]), ptr(state.hit_pos[entry]),
         ptr(state.hit_count[entry]), stream_ptr())


def ap_rank(state):
    """Rank + AP once every video of the state's dataset went through ap_match_seg for every entry -> device tensors (ap
    float64 (entries, tolerances, K1): the interpolated average precision per class, column 0 and classes without truth 0;
    nhits int32 of that shape; rank int32 (entries, tolerances, max(G,1)): per hit, in the truth table's layout, its 1-based
    position among the class's predictions of all videos)."""
    if not isinstance(state, ApState):
        raise TypeError("ap_rank: state must come from ap_state")
    E, T, K1, dev = state.E, state.T, state.K1, state.device
    rank = torch.zeros((E, T, max(state.G, 1)), dtype=torch.int32, device=dev)
    psorted = torch.empty((E, T, max(state.G, 1)), dtype=torch.float64, device=dev)
    ap = torch.empty((E, T, K1), dtype=torch.float64, device=dev)
    nhits = torch.empty((E, T, K1), dtype=torch.int32, device=dev)
    call("tdeed_ap_rank", ptr(state.ev_score), ptr(state.ev_count), ptr(state.vid_off), state.NV, state.LT, ptr(state.gt_off),
         state.G, K1, E, T, ptr(state.hit_pos), ptr(state.hit_count), ptr(state.class_off), ptr(rank), ptr(psorted), ptr(ap),
         ptr(nhits), stream_ptr())
    return ap, nhits, rank


# ---- a mAP pass sharded over ranks: every rank matches its own videos, then the states are exchanged (three phases, each
# returning or taking the tensors that go through a sum over the ranks; evalutil.merge_ap_state is the glue)
def _own_table(state, own_ords, who):
    """own_ords -> (sorted tuple, int32 (NV,) device table: 1 for the ordinals this rank matched), cached on the state"""
    if not isinstance(state, ApState):
        raise TypeError(f"{who}: state must come from ap_state")
    key = tuple(sorted(int(o) for o in own_ords))
    if len(set(key)) != len(key) or any(not 0 <= o < state.NV for o in key):
        raise ValueError(f"{who}: own ordinals {list(key)} must be distinct videos of the state's {state.NV}")
    cached = getattr(state, "_own", None)
    if cached is None or cached[0] != key:
        tab = np.zeros(state.NV, np.int32)
        tab[list(key)] = 1
        state._own = (key, torch.from_numpy(tab).to(state.device))
    return state._own


def ap_state_counts(state, own_ords):
    """Phase 1 of the exchange -> [state.ev_count, state.hit_count, owners]: the int32 tensors to be summed over the ranks IN
    PLACE (a caller that sums elsewhere copies the sums back into them).  The two count tables are zero wherever this rank
    matched nothing; owners int32 (NV,) is 1 for own_ords, so its sum must be 1 everywhere: ap_state_pack checks it."""
    _, own = _own_table(state, own_ords, "ap_state_counts")
    return [state.ev_count, state.hit_count, own.clone()]


def ap_owner_errors(owners):
    """The ordinals the summed ownership table names more than once / never, as the RuntimeError every rank raises before any
    payload is built (None when every video was matched exactly once).  Host arithmetic only."""
    owners = np.asarray(owners).reshape(-1)
    twice = np.nonzero(owners > 1)[0].tolist()
    never = np.nonzero(owners < 1)[0].tolist()
    if not twice and not never:
        return None
    return RuntimeError(f"ap_state: the ranks do not partition the videos: ordinals scored twice {twice}, never {never}")


def _ap_scans(state):
    sc_end = torch.cumsum(state.ev_count.view(-1), 0, dtype=torch.int64)
    hc_end = torch.cumsum(state.hit_count.view(-1), 0, dtype=torch.int64)
    return sc_end, hc_end


def ap_state_pack(state, own_ords, owners=None):
    """Phase 2, once state.ev_count / state.hit_count hold the sums over the ranks -> (scores float64 (S,), hits int32 (Hh,)),
    S = sum(ev_count), Hh = sum(hit_count): the dense payloads with this rank's own segments in place and zeros elsewhere, to
    be summed over the ranks (every element is written by one rank, scores are not negative: x + 0.0 is exact).  Segment (e,
    c, ord) of the scores starts at the exclusive scan of ev_count in the store's own order, segment (e, t, ord*K1+c) of the
    hits at that of hit_count.  owners: the summed ownership table of ap_state_counts; it is read in the one host
    synchronisation that sizes the payloads, and a video matched twice or never raises ap_owner_errors' RuntimeError before
    a payload exists."""
    key, own = _own_table(state, own_ords, "ap_state_pack")
    dev = state.device
    sc_end, hc_end = _ap_scans(state)
    parts = [sc_end[-1:], hc_end[-1:]]
    if owners is not None:
        _chk_table(owners, state.NV, dev, "ap_state_pack", "owners")
        parts.append(owners.to(torch.int64))
    small = torch.cat(parts)
    h_small = torch.empty(small.shape, dtype=torch.int64).pin_memory()
    h_small.copy_(small, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    vals = h_small.numpy()
    if owners is not None:
        err = ap_owner_errors(vals[2:])
        if err is not None:
            raise err
    S, Hh = int(vals[0]), int(vals[1])
    scores = torch.zeros((S,), dtype=torch.float64, device=dev)
    hits = torch.zeros((Hh,), dtype=torch.int32, device=dev)
    call("tdeed_ap_state_pack", ptr(state.ev_score), ptr(state.hit_pos), ptr(scores) if S else None, ptr(hits) if Hh else None,
         ptr(sc_end), ptr(hc_end), S, Hh, ptr(own), ptr(state.vid_off), ptr(state.gt_off), state.NV, state.K1, state.E, state.T,
         state.LT, state.G, stream_ptr())
    return scores, hits


def ap_state_unpack(state, own_ords, scores, hits):
    """Phase 3: writes the segments of the videos that are NOT in own_ords from the summed payloads into state.ev_score /
    state.hit_pos; own segments are not written.  ev_frame of foreign videos is left as it is -- ap_rank does not read it, so
    after the exchange the state answers ap_rank like a one-rank pass, but its ev_frame is only this rank's share."""
    key, own = _own_table(state, own_ords, "ap_state_unpack")
    dev = state.device
    for x, dt, what in ((scores, torch.float64, "scores float64"), (hits, torch.int32, "hits int32")):
        if not isinstance(x, torch.Tensor) or x.dtype != dt or x.dim() != 1 or not x.is_contiguous() or x.device != dev:
            raise ValueError(f"ap_state_unpack: {what} must be a contiguous 1-d tensor on the state's device")
    sc_end, hc_end = _ap_scans(state)
    S, Hh = scores.numel(), hits.numel()
    call("tdeed_ap_state_unpack", ptr(state.ev_score), ptr(state.hit_pos), ptr(scores) if S else None, ptr(hits) if Hh else None,
         ptr(sc_end), ptr(hc_end), S, Hh, ptr(own), ptr(state.vid_off), ptr(state.gt_off), state.NV, state.K1, state.E, state.T,
         state.LT, state.G, stream_ptr())


def frame_stats_size(K1):
    """entries of the frame counter tensor: frames, errors, then (tp, fp, fn) for "any" and every class"""
    return 2 + 3 * int(K1)


def frame_stats_seg(mean, labels_u8, stats=None):
    """The frame error / foreground-F1 counters of evalutil.frame_events(labels=...) over a packed track: mean fp32 (sum L,K1),
    labels_u8 uint8 (sum L,) the ground-truth class of every packed frame (K1 <= 256, values < K1), both on the device.  stats
    int64 (2 + 3*K1,) is accumulated into (fresh zeros when None) and returned: [0] frames, [1] frames whose arg-max (first
    maximum, np.argmax) differs from the label, then (tp, fp, fn) at 2 + 3*k for k = 0 ("any") and the classes k >= 1
    (evalutil.frame_stats_dict turns it into frame_events' stats dict).  One asynchronous launch on the current stream."""
    L, K1 = _chk_track(mean, "frame_stats_seg")
    dev = mean.device
    if K1 > 256:
        raise ValueError(f"frame_stats_seg: {K1} columns do not fit one-byte labels")
    if not isinstance(labels_u8, torch.Tensor) or labels_u8.dtype != torch.uint8 or tuple(labels_u8.shape) != (L,) \
            or not labels_u8.is_contiguous() or labels_u8.device != dev:
        raise ValueError(f"frame_stats_seg: labels must be a contiguous uint8 ({L},) tensor on the track's device")
    if stats is None:
        stats = torch.zeros((frame_stats_size(K1),), dtype=torch.int64, device=dev)
    elif not isinstance(stats, torch.Tensor) or stats.dtype != torch.int64 or tuple(stats.shape) != (frame_stats_size(K1),) \
            or not stats.is_contiguous() or stats.device != dev:
        raise ValueError(f"frame_stats_seg: stats must be a contiguous int64 ({frame_stats_size(K1)},) tensor on the track's device")
    call("tdeed_frame_stats_seg", ptr(mean), ptr(labels_u8), L, K1, ptr(stats), stream_ptr())
    return stats


def cast_bf16(src_f32):
    out = torch.empty(src_f32.shape, dtype=torch.bfloat16, device=src_f32.device)
    call("tdeed_cast_f32_to_bf16", ptr(src_f32), ptr(out), src_f32.numel(), stream_ptr())
    return out


def fill_u8_hash(shape, seed, device="cuda"):
    """Device-side twin of tdeed_amd.synth.uint8_clip (bit-identical bytes)."""
    from .synth import fnv1a64
    n = 1
    for s in shape:
        n *= int(s)
    out = torch.empty(((n + 7) // 8) * 8, dtype=torch.uint8, device=device)
    base = ((seed * 0x9E3779B97F4A7C15) ^ fnv1a64("clip")) & 0xFFFFFFFFFFFFFFFF
    call("tdeed_fill_u8_hash", ptr(out), n, base, stream_ptr())
    return out[:n].view(*shape)


# ---------------------------------------------------------------------------------------------- JPEG decode (jpeg.hip)
def jpeg_frame_coeffs(W, H, sampling):
    """int16 values of one frame's coefficient range (jpegdev.geometry(...).frame_blocks * 64)"""
    n = int(_lib.load().tdeed_jpeg_frame_coeffs(int(W), int(H), int(sampling)))
    if n < 0:
        raise ValueError(f"jpeg_frame_coeffs: bad geometry {H}x{W}, sampling {sampling}")
    return n


def _chk_jpeg_tables(who, dev, **tabs):
    for name, (t_, dtype) in tabs.items():
        if not isinstance(t_, torch.Tensor) or t_.dtype != dtype or t_.device != dev or not t_.is_contiguous():
            raise TypeError(f"{who}: {name} must be a contiguous {dtype} tensor on {dev}")


def jpeg_entropy(stream, segments, waves, table_sets, W, H, sampling, frame_lo, n_frames, coeff, status):
    """Entropy-decode the segments listed by `waves` (jpegdev.PackedJpegs.waves(frame_lo, frame_lo + n_frames)) into coeff,
    int16 (>= n_frames * jpeg_frame_coeffs) that the caller has zero-filled on this stream; status int32 (n_segments,)
    gets 0 or the error code per decoded row.  stream uint8, segments int32 (n_segments, 6), waves int32 (n_waves, 2),
    table_sets uint8 (n_sets, 4240): all on the device."""
    dev = coeff.device
    _chk(coeff, "coeff", torch.int16)
    _chk_jpeg_tables("jpeg_entropy", dev, stream=(stream, torch.uint8), segments=(segments, torch.int32),
                     waves=(waves, torch.int32), table_sets=(table_sets, torch.uint8), status=(status, torch.int32))
    if segments.dim() != 2 or segments.shape[1] != 6 or waves.dim() != 2 or waves.shape[1] != 2:
        raise ValueError("jpeg_entropy: segments (n, 6) and waves (n, 2)")
    if table_sets.dim() != 2 or table_sets.shape[1] != 4240 or table_sets.shape[0] < 1:
        raise ValueError("jpeg_entropy: table_sets (n_sets, 4240)")
    if status.numel() < segments.shape[0]:
        raise ValueError(f"jpeg_entropy: {status.numel()} status entries for {segments.shape[0]} segments")
    fc = jpeg_frame_coeffs(W, H, sampling)
    if coeff.numel() < int(n_frames) * fc:
        raise ValueError(f"jpeg_entropy: coeff holds {coeff.numel()} values, {n_frames} frames need {int(n_frames) * fc}")
    call("tdeed_jpeg_entropy", ptr(stream), stream.numel(), ptr(segments), segments.shape[0], ptr(waves), waves.shape[0],
         ptr(table_sets), table_sets.shape[0], int(W), int(H), int(sampling), int(frame_lo), int(n_frames), ptr(coeff),
         ptr(status), stream_ptr())
    return coeff


def jpeg_pixels(coeff, frame_set, table_sets, out, frame_lo, n_frames, sampling):
    """coeff of the frames frame_lo .. frame_lo + n_frames - 1 (jpeg_entropy) -> out[frame_lo : frame_lo + n_frames] of the
    uint8 (L,3,H,W) video buffer; frame_set int32 (L,) table set per frame, a frame with -1 is left as it is."""
    dev = out.device
    _chk(out, "out", torch.uint8)
    _chk(coeff, "coeff", torch.int16)
    _chk_jpeg_tables("jpeg_pixels", dev, frame_set=(frame_set, torch.int32), table_sets=(table_sets, torch.uint8))
    if out.dim() != 4 or out.shape[1] != 3:
        raise ValueError("jpeg_pixels: out must be (L,3,H,W)")
    L, _, H, W = out.shape
    if table_sets.dim() != 2 or table_sets.shape[1] != 4240 or table_sets.shape[0] < 1:
        raise ValueError("jpeg_pixels: table_sets (n_sets, 4240)")
    if frame_lo < 0 or n_frames < 1 or frame_lo + n_frames > L or frame_set.numel() < frame_lo + n_frames:
        raise ValueError(f"jpeg_pixels: frames {frame_lo}..{frame_lo + n_frames} outside the {L} of out / {frame_set.numel()} of frame_set")
    fc = jpeg_frame_coeffs(W, H, sampling)
    if coeff.numel() < int(n_frames) * fc:
        raise ValueError(f"jpeg_pixels: coeff holds {coeff.numel()} values, {n_frames} frames need {int(n_frames) * fc}")
    call("tdeed_jpeg_pixels", ptr(coeff), ptr(frame_set), ptr(table_sets), table_sets.shape[0], ptr(out), int(frame_lo),
         int(n_frames), int(H), int(W), int(sampling), stream_ptr())
    return out


def jpeg_pixels_rows(coeff, frame_set, table_sets, out, dst_row, frame_lo, n_frames, sampling):
    """jpeg_pixels with a row table: pack frame f (frame_lo <= f < frame_lo + n_frames) -> row dst_row[f] of out, a contiguous
    uint8 (...,3,H,W) buffer whose leading dimensions are flattened to rows (a (B,T,3,H,W) batch slot: row i * T + t).
    dst_row int32 (>= frame_lo + n_frames,) on the device; a frame whose row is negative or past the last row, or whose
    frame_set entry is -1, stores nothing."""
    dev = out.device
    _chk(out, "out", torch.uint8)
    _chk(coeff, "coeff", torch.int16)
    _chk_jpeg_tables("jpeg_pixels_rows", dev, frame_set=(frame_set, torch.int32), table_sets=(table_sets, torch.uint8),
                     dst_row=(dst_row, torch.int32))
    if out.dim() < 4 or out.shape[-3] != 3:
        raise ValueError("jpeg_pixels_rows: out must be (...,3,H,W)")
    H, W = int(out.shape[-2]), int(out.shape[-1])
    rows = out.numel() // (3 * H * W)
    if table_sets.dim() != 2 or table_sets.shape[1] != 4240 or table_sets.shape[0] < 1:
        raise ValueError("jpeg_pixels_rows: table_sets (n_sets, 4240)")
    if rows < 1 or frame_lo < 0 or n_frames < 1 or min(frame_set.numel(), dst_row.numel()) < frame_lo + n_frames:
        raise ValueError(f"jpeg_pixels_rows: frames {frame_lo}..{frame_lo + n_frames} outside the {frame_set.numel()} of frame_set / "
                         f"{dst_row.numel()} of dst_row, or out has no row")
    fc = jpeg_frame_coeffs(W, H, sampling)
    if coeff.numel() < int(n_frames) * fc:
        raise ValueError(f"jpeg_pixels_rows: coeff holds {coeff.numel()} values, {n_frames} frames need {int(n_frames) * fc}")
    call("tdeed_jpeg_pixels_rows", ptr(coeff), ptr(frame_set), ptr(table_sets), table_sets.shape[0], ptr(out), rows, ptr(dst_row),
         int(frame_lo), int(n_frames), int(H), int(W), int(sampling), stream_ptr())
    return out


def jpeg_pixels_window(coeff, frame_set, table_sets, out, dst_row, frame_lo, n_frames, sampling, H, W, top, left):
    """jpeg_pixels_rows over a window of the H x W frames: out is a contiguous uint8 (...,3,wh,ww) buffer and row dst_row[f]
    of it gets the pixels [top, top + wh) x [left, left + ww) of frame f.  Only the bands of the window are launched and
    only the blocks under it are transformed (jpegdev.window_blocks): the coefficients of every other block are never
    read.  The full window (0, 0, H, W) gives the bits of jpeg_pixels_rows.  A window that is empty or leaves the frame
    raises ValueError."""
    dev = out.device
    _chk(out, "out", torch.uint8)
    _chk(coeff, "coeff", torch.int16)
    _chk_jpeg_tables("jpeg_pixels_window", dev, frame_set=(frame_set, torch.int32), table_sets=(table_sets, torch.uint8),
                     dst_row=(dst_row, torch.int32))
    if out.dim() < 4 or out.shape[-3] != 3:
        raise ValueError("jpeg_pixels_window: out must be (...,3,wh,ww)")
    wh, ww = int(out.shape[-2]), int(out.shape[-1])
    H, W, top, left = int(H), int(W), int(top), int(left)
    if min(wh, ww) < 1 or top < 0 or left < 0 or top + wh > H or left + ww > W:
        raise ValueError(f"jpeg_pixels_window: the window {wh}x{ww} at ({top}, {left}) is empty or leaves the {H}x{W} frame")
    rows = out.numel() // (3 * wh * ww)
    if table_sets.dim() != 2 or table_sets.shape[1] != 4240 or table_sets.shape[0] < 1:
        raise ValueError("jpeg_pixels_window: table_sets (n_sets, 4240)")
    if rows < 1 or frame_lo < 0 or n_frames < 1 or min(frame_set.numel(), dst_row.numel()) < frame_lo + n_frames:
        raise ValueError(f"jpeg_pixels_window: frames {frame_lo}..{frame_lo + n_frames} outside the {frame_set.numel()} of frame_set "
                         f"/ {dst_row.numel()} of dst_row, or out has no row")
    fc = jpeg_frame_coeffs(W, H, sampling)
    if coeff.numel() < int(n_frames) * fc:
        raise ValueError(f"jpeg_pixels_window: coeff holds {coeff.numel()} values, {n_frames} frames need {int(n_frames) * fc}")
    call("tdeed_jpeg_pixels_window", ptr(coeff), ptr(frame_set), ptr(table_sets), table_sets.shape[0], ptr(out), rows, ptr(dst_row),
         int(frame_lo), int(n_frames), H, W, int(sampling), top, left, wh, ww, stream_ptr())
    return out


def jpeg_window_blocks(W, H, sampling, top, left, wh, ww):
    """the launcher's block ranges of a window (csrc/jpeg_core.h jc_window) as ten ints, in jpegdev.window_blocks' order:
    band lo / n, luma block columns lo / n, luma block rows lo / hi, chroma block columns lo / n, MCU rows lo / hi"""
    import ctypes
    r = (ctypes.c_int * 10)()
    if _lib.load().tdeed_jpeg_window_blocks(int(W), int(H), int(sampling), int(top), int(left), int(wh), int(ww), r) != 0:
        raise ValueError(f"jpeg_window_blocks: bad geometry {H}x{W}, sampling {sampling} or window {wh}x{ww} at ({top}, {left})")
    return list(r)


def jpeg_pixels_lds_bytes(W, H, sampling, window=None):
    """dynamic LDS bytes per workgroup that the pixel launchers request: jpeg_pixels / jpeg_pixels_rows without `window`,
    jpeg_pixels_window with window = (top, left, wh, ww)"""
    top, left, wh, ww = window if window is not None else (0, 0, 0, 0)
    n = int(_lib.load().tdeed_jpeg_pixels_lds_bytes(int(W), int(H), int(sampling), int(window is not None), int(top), int(left),
                                                    int(wh), int(ww)))
    if n < 0:
        raise ValueError(f"jpeg_pixels_lds_bytes: bad geometry {H}x{W}, sampling {sampling} or window {window}")
    return n


PIECE_BYTES = 72          # csrc/jpeg_core.h JcPiece, jpegdev.PIECE


def _chk_jpeg_resident(who, stream, table_sets, waves):
    if waves.dim() != 2 or waves.shape[1] != 2 or waves.shape[0] < 1:
        raise ValueError(f"{who}: waves (n, 2)")
    if table_sets.dim() != 2 or table_sets.shape[1] != 4240 or table_sets.shape[0] < 1:
        raise ValueError(f"{who}: table_sets (n_sets, 4240)")
    if stream.dim() != 1 or stream.numel() < 1:
        raise ValueError(f"{who}: stream must be a 1-d uint8 tensor")


def jpeg_entropy_index(stream, base, segments, waves, table_sets, W, H, sampling, split_mcus, piece_off, seg_base, pieces,
                       status):
    """The index pass over the segments of one shard of a resident stream: nothing is decoded into coefficients, the decoder
    state at every split point (jpegdev.split_points) is recorded.  stream uint8: the whole resident stream, the shard's
    byte offsets count from `base`; segments int32 (n, 6), waves int32 (n_waves, 2) over them, piece_off int32 (n + 1,):
    segment row i writes the rows piece_off[i] .. piece_off[i + 1] - 1 of pieces, uint8 (n_pieces, 72); seg_base: the
    shard's first row in the numbering the piece rows carry; status int32 (>= n,): 0 or the error code per row."""
    dev = stream.device
    _chk_jpeg_tables("jpeg_entropy_index", dev, stream=(stream, torch.uint8), segments=(segments, torch.int32),
                     waves=(waves, torch.int32), table_sets=(table_sets, torch.uint8), piece_off=(piece_off, torch.int32),
                     pieces=(pieces, torch.uint8), status=(status, torch.int32))
    if not stream.is_cuda:
        raise TypeError("jpeg_entropy_index: the tensors must be on the device")
    _chk_jpeg_resident("jpeg_entropy_index", stream, table_sets, waves)
    if segments.dim() != 2 or segments.shape[1] != 6 or segments.shape[0] < 1:
        raise ValueError("jpeg_entropy_index: segments (n, 6)")
    n = int(segments.shape[0])
    if piece_off.numel() != n + 1 or status.numel() < n:
        raise ValueError(f"jpeg_entropy_index: {piece_off.numel()} piece offsets / {status.numel()} status entries for {n} segments")
    if pieces.dim() != 2 or pieces.shape[1] != PIECE_BYTES or pieces.shape[0] < 1:
        raise ValueError(f"jpeg_entropy_index: pieces (n_pieces, {PIECE_BYTES})")
    if not 0 <= int(base) <= stream.numel() or int(split_mcus) < 1 or int(seg_base) < 0:
        raise ValueError(f"jpeg_entropy_index: base {base} outside the stream of {stream.numel()} bytes, split_mcus {split_mcus} "
                         f"or seg_base {seg_base}")
    jpeg_frame_coeffs(W, H, sampling)
    call("tdeed_jpeg_entropy_index", ptr(stream), stream.numel(), int(base), ptr(segments), n, ptr(waves), waves.shape[0],
         ptr(table_sets), table_sets.shape[0], int(W), int(H), int(sampling), int(split_mcus), ptr(piece_off), int(seg_base),
         ptr(pieces), pieces.shape[0], ptr(status), stream_ptr())
    return pieces


RELOC_BYTES = 24          # csrc/jpeg_core.h JcReloc: int64 delta, lo, hi


def jpeg_entropy_items(stream, pieces, items, waves, table_sets, W, H, sampling, slot_lo, n_slots, coeff, err, reloc=None):
    """Decode the items listed by `waves` -- items int32 (n_items, 2) rows of (piece row, coefficient slot), waves int32
    (n_waves, 2) rows of (first item, count <= 64), one table set per wave -- into coeff, int16 (>= n_slots *
    jpeg_frame_coeffs) that the caller has zero-filled on this stream: slot s lands at (s - slot_lo) frames into it.  err:
    int32 (1,) on the device, bit `code` of the word is set for every error code met; nothing else is reported.
    reloc: None, or int64 (n, 3) on the device, row s = (delta, lo, hi) of slot s (streamplan.stage_batch): the bytes of a
    piece of that slot are a staged copy at stream[pos - delta ...] and must lie in stream[lo:hi]; a piece that does not, or
    a slot without a row, sets bit 7 of err and decodes nothing (tdeed_jpeg_entropy_items_reloc)."""
    dev = coeff.device
    _chk(coeff, "coeff", torch.int16)
    _chk_jpeg_tables("jpeg_entropy_items", dev, stream=(stream, torch.uint8), pieces=(pieces, torch.uint8),
                     items=(items, torch.int32), waves=(waves, torch.int32), table_sets=(table_sets, torch.uint8),
                     err=(err, torch.int32))
    _chk_jpeg_resident("jpeg_entropy_items", stream, table_sets, waves)
    if items.dim() != 2 or items.shape[1] != 2 or items.shape[0] < 1:
        raise ValueError("jpeg_entropy_items: items (n, 2)")
    if pieces.dim() != 2 or pieces.shape[1] != PIECE_BYTES or pieces.shape[0] < 1:
        raise ValueError(f"jpeg_entropy_items: pieces (n_pieces, {PIECE_BYTES})")
    if err.numel() != 1 or int(slot_lo) < 0 or int(n_slots) < 1:
        raise ValueError(f"jpeg_entropy_items: err holds {err.numel()} words, slots {slot_lo}..{int(slot_lo) + int(n_slots)}")
    fc = jpeg_frame_coeffs(W, H, sampling)
    if coeff.numel() < int(n_slots) * fc:
        raise ValueError(f"jpeg_entropy_items: coeff holds {coeff.numel()} values, {n_slots} slots need {int(n_slots) * fc}")
    if reloc is not None:
        _chk_jpeg_tables("jpeg_entropy_items", dev, reloc=(reloc, torch.int64))
        if reloc.dim() != 2 or reloc.shape[1] != 3 or reloc.shape[0] < 1:
            raise ValueError("jpeg_entropy_items: reloc (n, 3) rows of (delta, lo, hi)")
        call("tdeed_jpeg_entropy_items_reloc", ptr(stream), stream.numel(), ptr(pieces), pieces.shape[0], ptr(items),
             items.shape[0], ptr(waves), waves.shape[0], ptr(table_sets), table_sets.shape[0], int(W), int(H), int(sampling),
             int(slot_lo), int(n_slots), ptr(reloc), reloc.shape[0], ptr(coeff), ptr(err), stream_ptr())
        return coeff
    call("tdeed_jpeg_entropy_items", ptr(stream), stream.numel(), ptr(pieces), pieces.shape[0], ptr(items), items.shape[0],
         ptr(waves), waves.shape[0], ptr(table_sets), table_sets.shape[0], int(W), int(H), int(sampling), int(slot_lo),
         int(n_slots), ptr(coeff), ptr(err), stream_ptr())
    return coeff


def jpeg_slot_fill(side, fill, out):
    """The rows of a batch slot that no decode fills: out uint8 (..., 3, H, W) flattened to fill.numel() rows; fill int32 on
    the device: -2 leaves the row as it is, -1 zeroes it, r >= 0 copies side[r] (side: uint8 (n, 3, H, W), or None when no
    frame is kept decoded)."""
    dev = out.device
    _chk(out, "out", torch.uint8)
    _chk_jpeg_tables("jpeg_slot_fill", dev, fill=(fill, torch.int32))
    n = int(fill.numel())
    if n < 1 or n > 65535 or out.numel() % n:
        raise ValueError(f"jpeg_slot_fill: {n} rows for an output of {out.numel()} bytes")
    fb = out.numel() // n
    rows = 0
    if side is not None:
        _chk_jpeg_tables("jpeg_slot_fill", dev, side=(side, torch.uint8))
        if side.numel() % fb:
            raise ValueError(f"jpeg_slot_fill: side holds {side.numel()} bytes, a row has {fb}")
        rows = side.numel() // fb
    call("tdeed_jpeg_slot_fill", ptr(side) if rows else None, rows, fb, ptr(fill), n, ptr(out), stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------- SGP contractions (sgp_gemm.hip)
def sgp_gemm_ksteps(K):
    return int(_lib.load().tdeed_sgp_gemm_ksteps(K))


def sgp_gemm_form(mode, B, T, N, K):
    """(MT, NT) of the tile the launcher wants for this contraction: 16 MT rows of one clip x 64 NT features per workgroup.
    mode 0 / 3: GroupNorm + fc1 + GELU on bf16 / fp32 rows, 1: fc2 + residual, 2: concat_fc + GELU"""
    f = int(_lib.load().tdeed_sgp_gemm_form(mode, B, T, N, K))
    return f >> 4, f & 15


def sgp_gemm_tiles(T, N, form):
    """(row tiles per clip, column tiles) of a form: the leading dimensions of chs_out / rowstat_part"""
    L = _lib.load()
    return int(L.tdeed_sgp_gemm_row_tiles(T, form[0])), int(L.tdeed_sgp_gemm_col_tiles(N, form[1]))


def sgp_gemm_gn_gelu(y, chsum, gn_w, gn_b, Wp, bias, N, out=None, form=None, G=16, eps=1e-5):
    """H (B,T,N) bf16 = GELU(GroupNorm(y) @ W^T + b).  y (B,T,K) bf16 | fp32; chsum fp32 (parts,B,K,2) or (B,K,2): per-channel
    (sum, sum of squares) of y over each clip's rows; Wp: packing.pack_mfma_frags(W, ks_mult=12)."""
    B, T, K = y.shape
    parts = 1 if chsum.dim() == 3 else chsum.shape[0]
    form = form or sgp_gemm_form(0 if y.dtype == torch.bfloat16 else 3, B, T, N, K)
    if out is None:
        out = torch.empty((B, T, N), dtype=torch.bfloat16, device=y.device)
    call("tdeed_sgp_gemm_gn_gelu", ptr(y), B, T, K, ptr(chsum), parts, ptr(gn_w), ptr(gn_b), G, eps, ptr(Wp), ptr(bias), N,
         ptr(out), form[0] * 16 + form[1], dtype_code(y.dtype), stream_ptr())
    return out


def sgp_gemm_residual(H, Wp, bias, resid, out=None, rowstat_part=None, pooled=None, rowstat_pool_part=None, form=None):
    """out (B,T,N) = resid + H @ W^T + b (H bf16 (B,T,K); out / resid / pooled bf16 | fp32).  rowstat_part fp32 (nct, B*T, 2):
    (sum, sum of squares) of every stored row over each column tile; pooled (B,T/2,N): AdaptiveMaxPool1d(T/2) of out and its
    rowstat_pool_part (nct, B*T/2, 2).  -> (out, form)"""
    B, T, K = H.shape
    N = resid.shape[-1]
    form = form or sgp_gemm_form(1, B, T, N, K)
    if out is None:
        out = torch.empty_like(resid)
    call("tdeed_sgp_gemm_residual", ptr(H), B, T, K, ptr(Wp), ptr(bias), N, ptr(resid), ptr(out), ptr(rowstat_part),
         ptr(pooled), ptr(rowstat_pool_part), 0 if pooled is None else pooled.shape[1], form[0] * 16 + form[1],
         dtype_code(out.dtype), stream_ptr())
    return out


def sgp_gemm_gelu_chsum(A, Wp, bias, N, out, chs_out, form=None, out16=None):
    """out (B,T,N) bf16 | fp32 = GELU(A @ W^T + b), A bf16 (B,T,K); chs_out fp32 (NJ,B,N,2): per-channel (sum, sum of squares)
    of the stored rows per row tile"""
    B, T, K = A.shape
    form = form or sgp_gemm_form(2, B, T, N, K)
    call("tdeed_sgp_gemm_gelu_chsum", ptr(A), B, T, K, ptr(Wp), ptr(bias), N, ptr(out), ptr(chs_out), ptr(out16),
         form[0] * 16 + form[1], dtype_code(out.dtype), stream_ptr())
    return out


# ---- training clips drawn from resident videos (trainclips.hip; tables: cliptable.train_clip_table, int64 on the device)
def _chk_clip_tables(frames_u8, tabs, who):
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() < 2:
        raise TypeError(f"{who}: frames must be uint8 (L, ...)")
    if not frames_u8.is_cuda or not frames_u8.is_contiguous():
        raise ValueError(f"{who}: frames must be a contiguous GPU tensor")
    if not tabs or not all(isinstance(tab, torch.Tensor) for tab in tabs):
        raise ValueError(f"{who}: the clip tables must be tensors")
    B = tabs[0].numel()
    for tab in tabs:
        if tab.dtype != torch.int64 or tab.dim() != 1 or tab.numel() != B or not tab.is_contiguous() \
                or tab.device != frames_u8.device:
            raise ValueError(f"{who}: the clip tables must be contiguous int64 ({B},) tensors on the frames' device")
    return B, int(frames_u8.shape[0]), int(frames_u8[0].numel())


def _clip_strides(strides, n, dev, who):
    """The `stride` of the three clip ops -> (suffix of the C entry, its stride operand).  A scalar is one stride for all
    clips: the scalar entry, ("", the scalar as given).  Anything else (a tensor, a sequence, an array) is one stride per clip
    (trainclips.JointResidentClips): the ..._ps entry, "_ps" and a contiguous int32 (n,) tensor on `dev`.  A host sequence /
    array is held against the rule (every entry > 0, ValueError) and uploaded; a device tensor is the caller's own table,
    checked on the host where it was built -- the kernels do not follow an entry <= 0."""
    if isinstance(strides, (int, float, np.generic)) or (isinstance(strides, np.ndarray) and strides.ndim == 0):
        return "", strides
    if not isinstance(strides, torch.Tensor) or not strides.is_cuda:
        host = np.asarray(strides.numpy() if isinstance(strides, torch.Tensor) else strides)
        if host.ndim != 1 or host.size != n or not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f"{who}: strides must be {n} integers, one per clip")
        if host.size and int(host.min()) <= 0:
            raise ValueError(f"{who}: every stride must be positive")
        return "_ps", torch.from_numpy(np.ascontiguousarray(host, np.int32)).to(dev)
    if strides.dtype != torch.int32 or strides.dim() != 1 or strides.numel() != n or not strides.is_contiguous() \
            or strides.device != dev:
        raise ValueError(f"{who}: strides must be a contiguous int32 ({n},) tensor on the tables' device")
    return "_ps", strides


def train_clip_gather(frames_u8, first, base, nframes, T, stride, out):
    """out[b*T + t] = frames_u8[first[b] + base[b] + t*stride] when 0 <= base[b] + t*stride < nframes[b], a zero frame
    otherwise.  frames_u8: the packed frames of all resident videos (sum L, ...); first / base / nframes: int64 (B,) on the
    device (first packed frame and length of the clip's video, the clip's first original frame).  stride: an int, or one
    per clip -- strides[b] in place of stride --: int32 (B,) on the device, or a host sequence (checked: every entry > 0)."""
    B, L, fb = _chk_clip_tables(frames_u8, (first, base, nframes), "train_clip_gather")
    ps, stride = _clip_strides(stride, B, frames_u8.device, "train_clip_gather")
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != frames_u8.device:
        raise TypeError("train_clip_gather: out must be a contiguous uint8 tensor on the frames' device")
    if out.numel() != B * T * fb:
        raise ValueError(f"train_clip_gather: out holds {out.numel()} bytes, {B} clips of {T} frames need {B * T * fb}")
    call("tdeed_train_clip_gather_u8" + ps, ptr(frames_u8), L, fb, ptr(first), ptr(base), ptr(nframes), B, T,
         ptr(stride) if ps else stride, ptr(out), stream_ptr())
    return out


def train_clip_gather_mix(frames_u8, tabs_a, tabs_b, lam, T, stride, out=None):
    """fp32 (B,T,...) = lam[b] * A[b] + (1 - lam[b]) * B[b] with A / B the windows train_clip_gather would write for the
    table triples tabs_a / tabs_b = (first, base, nframes): the bits of ops_bwd.mix_frames on those two batches, which are
    never materialised.  lam: fp32 (B,) on the device.  stride: as `train_clip_gather`; a clip's own stride is shared by its
    two operands."""
    if not isinstance(tabs_a, (tuple, list)) or not isinstance(tabs_b, (tuple, list)) or len(tabs_a) != 3 or len(tabs_b) != 3:
        raise ValueError("train_clip_gather_mix: (first, base, nframes) per operand")
    B, L, fb = _chk_clip_tables(frames_u8, tuple(tabs_a) + tuple(tabs_b), "train_clip_gather_mix")
    ps, stride = _clip_strides(stride, B, frames_u8.device, "train_clip_gather_mix")
    if lam.dtype != torch.float32 or lam.numel() != B or not lam.is_contiguous() or lam.device != frames_u8.device:
        raise ValueError(f"train_clip_gather_mix: lam must be a contiguous fp32 ({B},) tensor on the frames' device")
    if out is None:
        out = torch.empty((B, T) + tuple(frames_u8.shape[1:]), dtype=torch.float32, device=frames_u8.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * T * fb or out.device != frames_u8.device:
        raise ValueError(f"train_clip_gather_mix: out must be a contiguous fp32 tensor of {B * T * fb} elements")
    call("tdeed_train_clip_gather_mix_f32" + ps, ptr(frames_u8), L, fb, *(ptr(x) for x in tabs_a), *(ptr(x) for x in tabs_b),
         ptr(lam), B, T, ptr(stride) if ps else stride, ptr(out), stream_ptr())
    return out


def clip_labels(clip_video, clip_base, T, stride, r, ev_off, ev_frame, ev_class, label=None, labelD=None, displ=True):
    """Per-frame labels of n clips from their videos' event lists (cliptable.rasterise_labels on the device): clip_video /
    clip_base int64 (n,), ev_off int32 (nv+1,), ev_frame / ev_class int32 (n_events,), all on the device.  stride: as
    `train_clip_gather`, an int or one per clip.
    -> (label int64 (n,T), labelD int64 (n,T) or None when displ is False)."""
    dev = clip_video.device
    n = clip_video.numel()
    for tab, dt, what in ((clip_video, torch.int64, "clip_video"), (clip_base, torch.int64, "clip_base"),
                          (ev_off, torch.int32, "ev_off"), (ev_frame, torch.int32, "ev_frame"), (ev_class, torch.int32, "ev_class")):
        if not isinstance(tab, torch.Tensor) or tab.dtype != dt or tab.dim() != 1 or not tab.is_contiguous() \
                or not tab.is_cuda or tab.device != dev:
            raise ValueError(f"clip_labels: {what} must be a contiguous 1-d {dt} GPU tensor")
    if clip_base.numel() != n or ev_class.numel() != ev_frame.numel() or ev_off.numel() < 2:
        raise ValueError("clip_labels: table lengths do not match")
    ps, stride = _clip_strides(stride, n, dev, "clip_labels")
    if label is None:
        label = torch.empty((n, T), dtype=torch.int64, device=dev)
    if labelD is None and displ:
        labelD = torch.empty((n, T), dtype=torch.int64, device=dev)
    for o in (label, labelD):
        if o is not None and (o.dtype != torch.int64 or not o.is_contiguous() or o.numel() != n * T or o.device != dev):
            raise ValueError(f"clip_labels: outputs must be contiguous int64 ({n},{T}) tensors")
    ne = ev_frame.numel()
    call("tdeed_clip_labels" + ps, ptr(clip_video), ptr(clip_base), n, T, ptr(stride) if ps else stride, r, ptr(ev_off),
         ptr(ev_frame) if ne else None, ptr(ev_class) if ne else None, ev_off.numel() - 1, ne, ptr(label), ptr(labelD), stream_ptr())
    return label, labelD
