"""Weight layouts of the HIP kernels: reference-format weights -> MFMA fragment orders, each stated once.

Pure functions of numpy / torch (no kernel, no plan switch).  The loop nests are the statement of what the kernels read;
`frag_index` turns any of them into an index map, so that the same layout can also be applied to a tensor where it lives
(one gather, no host round trip) and recorded by repack.PackPlan like any other copy.
"""
from types import SimpleNamespace

import numpy as np
import torch

from .ops import gs_source_order


def _np(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def _f32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _dense(a, act_dtype, device):
    return _f32(a, device).to(act_dtype).contiguous()


def _bf16(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).to(torch.bfloat16).contiguous()


_IDX = {}


def frag_index(layout, shape, device, *args):
    """Index map of a layout function (weight array of `shape`, *args -> fragment array with zero holes):
    fragments = cat([0, w.reshape(-1)])[idx]."""
    key = (layout.__name__, tuple(shape), args, str(device))
    if key not in _IDX:
        ids = (np.arange(int(np.prod(shape)), dtype=np.float32) + 1).reshape(tuple(shape))     # exact in fp32 (< 2^24)
        _IDX[key] = torch.from_numpy(layout(ids, *args).astype(np.int64)).to(device)
    return _IDX[key]


def gather_frags(layout, w, *args):
    """layout(w, *args) of a tensor where it lives, by one gather through the cached index map (a training step re-packs an
    updated weight without a host round trip; under repack.PackPlan's recording w holds tagged positions, not values)."""
    idx = frag_index(layout, w.shape, w.device, *args)
    return torch.cat([torch.zeros(1, dtype=w.dtype, device=w.device), w.reshape(-1)])[idx].contiguous()


def _to_bf16(t):
    return t.to(torch.bfloat16)


def _ws_frags_np(W, epc):
    N, K = W.shape
    KS = (K + 4 * epc - 1) // (4 * epc)
    NT = (N + 31) // 32 * 2
    Wp = np.zeros((NT * 16, KS * 4 * epc), np.float32)
    n = np.arange(16)
    for nt in range(NT):
        t, h = divmod(nt, 2)
        L = 32 * t + 8 * (n // 4) + 4 * h + (n % 4)
        ok = L < N
        Wp[nt * 16 + n[ok], :K] = W[L[ok]]
    fr = Wp.reshape(NT, 16, KS, 4, epc).transpose(0, 2, 3, 1, 4)          # [NT][KS][q][n][epc]
    return np.ascontiguousarray(fr).reshape(NT, KS, 64, epc)


def pack_ws_weights(W, act_dtype, device):
    """[N][K] dense weight -> fragments for gemm_ws_kernel: [NT][KS][64][epc] with NT = 2*ceil(N/32),
    KS = ceil(K/(4*epc)); MFMA row n of tile 2t+h holds logical channel 32t + 8(n//4) + 4h + n%4 so that a
    lane's accumulators of a tile pair are 8 consecutive output channels."""
    fr = _ws_frags_np(_np(W).astype(np.float32), 8 if act_dtype == torch.bfloat16 else 4)
    return torch.from_numpy(fr).to(device).to(act_dtype).contiguous()


def pack_se_bf16(fc1_w, fc2_w, device):
    """SE weights for the bf16 excitation kernel: fc1.weight [R][C][1][1] -> bf16 [C][ceil8(R)] (transposed, zero padded);
    fc2.weight [C][R][1][1] -> bf16 [R][C] (transposed)."""
    w1 = _np(fc1_w).astype(np.float32)
    w1 = w1.reshape(w1.shape[0], -1)
    w2 = _np(fc2_w).astype(np.float32)
    w2 = w2.reshape(w2.shape[0], -1)
    R, C = w1.shape
    R8 = (R + 7) // 8 * 8
    p1 = np.zeros((C, R8), np.float32)
    p1[:, :R] = w1.T
    return dict(se_w1p=_bf16(p1, device), se_w2p=_bf16(w2.T, device))


def pack_mfma_frags(W, device, rows=None, ks_mult=1):
    """A dense [N][K] weight as MFMA A-operand fragments [ceil(N/16)][ceil(K/32)][64][8] (bf16, zero padded; lane l holds row
    l&15, k = 8*(l>>4)+j of the 16 x 32 tile).  rows: pad N up to this many rows (whole channel slabs); ks_mult: pad the
    k-steps to a multiple of this (sgp_gemm: whole super-iterations of its chunk ring, 12)."""
    W = _np(W).astype(np.float32)
    W = W.reshape(W.shape[0], -1)
    N, K = W.shape
    NT, KS = (max(N, rows or 0) + 15) // 16, (K + 31) // 32
    KS = (KS + ks_mult - 1) // ks_mult * ks_mult
    Wp = np.zeros((NT * 16, KS * 32), np.float32)
    Wp[:N, :K] = W
    fr = Wp.reshape(NT, 16, KS, 4, 8).transpose(0, 2, 3, 1, 4)
    return _bf16(fr.reshape(NT, KS, 64, 8), device)


def pack_se_mfma(fc1_w, fc2_w, device):
    """SE weights as MFMA A-operand fragments: fc1.weight [R][C] -> [ceil(R/16)][ceil(C/32)][64][8],
    fc2.weight [C][R] -> [ceil(C/16)][ceil(R/32)][64][8] (pack_mfma_frags)."""
    return dict(w1f=pack_mfma_frags(fc1_w, device), w2f=pack_mfma_frags(fc2_w, device))


def pack_front_weights(stem_w, stem_sc, stem_sh, w1, sc1, sh1, wd, scd, shd, w2, gw, sc2, sh2, device):
    """Weight fragments of s1_front_kernel (front.hip).  stem_w [32][3][3][3]; w1/wd [C1][32]; w2 [C1][gw][3][3].
    Stem k-slot s = 4ks+q -> (ky = s>>1, half = s&1), element j -> (kx = 2half + j//4, c = j%4 (3 = pad));
    conv1/downsample k-slot q element j -> stem channel 4q+j (j<4) / 16+4q+j-4: the order in which the stem's
    MFMA accumulators hand the 32 channels over."""
    stem_w, w1, wd = _np(stem_w).astype(np.float32), _np(w1).astype(np.float32), _np(wd).astype(np.float32)
    C1 = w1.shape[0]
    sw = _stem_frags_np(stem_w)
    nt = (C1 + 15) // 16

    def kperm(W):
        fr = np.zeros((nt, 64, 8), np.float32)
        for t in range(nt):
            for q in range(4):
                for j in range(8):
                    chn = 4 * q + j if j < 4 else 16 + 4 * q + j - 4
                    for n in range(16):
                        if t * 16 + n < C1:
                            fr[t, q * 16 + n, j] = W[t * 16 + n, chn]
        return fr
    bf = lambda a: _bf16(a, device)                                                    # noqa: E731
    f32 = lambda a: _f32(_np(a), device)                                              # noqa: E731
    return SimpleNamespace(C1=C1, stem_wf=bf(sw), stem_sc=f32(stem_sc), stem_sh=f32(stem_sh), w1f=bf(kperm(w1)),
                           sc1=f32(sc1), sh1=f32(sh1), wdf=bf(kperm(wd)), scd=f32(scd), shd=f32(shd),
                           w2f=pack_gconv_frags(w2, gw, device), sc2=f32(sc2), sh2=f32(sh2))


def _stem_frags_np(stem_w):
    """stem conv weight [32][3][3][3] -> MFMA A fragments [2 channel tiles][2 k-steps][64 lanes][8] (front.hip: k-slot
    s = 4ks+q -> (ky = s>>1, half = s&1), element j -> (kx = 2half + j//4, c = j%4, 3 = pad))."""
    sw = np.zeros((2, 2, 64, 8), stem_w.dtype)
    for t in range(2):
        for ks in range(2):
            for q in range(4):
                s_ = 4 * ks + q
                if s_ >= 6:
                    continue
                ky, half = s_ >> 1, s_ & 1
                for j in range(8):
                    kx, c = 2 * half + j // 4, j % 4
                    if kx > 2 or c > 2:
                        continue
                    sw[t, ks, q * 16:(q + 1) * 16, j] = stem_w[t * 16:(t + 1) * 16, c, ky, kx]
    return sw


def stem_frags_on_device(w):
    """_features.stem.conv.weight (32,3,3,3) fp32 on the device -> the fragments of _stem_frags_np (kept in fp32: the training
    stem splits them into bf16 head + tail itself)."""
    return gather_frags(_stem_frags_np, w)


def gs_source_order_columns(w1, F):
    """conv1 weight (cout, cin) of a gate-shift-fuse site -> the same weight for a slice left in SOURCE channel order:
    out[:, ci] = w1[:, co] for the output channel co that source channel ci is interleaved to (impl/gsf.py:88-91);
    columns >= F unchanged."""
    w = np.array(w1, copy=True)
    src = gs_source_order(F)                      # src[co] = ci
    w[:, src] = w1[:, :F]
    return w


def _gsf_q_frags_np(w3d):
    Fh = w3d.shape[1]
    F = 2 * Fh
    nch = (F + 7) // 8
    KS = (9 * nch + 3) // 4
    fr = np.zeros((KS, 64, 8), np.float32)
    for ks in range(KS):
        for q in range(4):
            s_ = 4 * ks + q
            tap, ck = divmod(s_, nch)
            if tap >= 9:
                continue
            dy, dx = divmod(tap, 3)
            for n in range(6):
                jt, g = divmod(n, 2)
                for e in range(8):
                    c = ck * 8 + e
                    if c < F and c // Fh == g:
                        fr[ks, q * 16 + n, e] = w3d[g, c - g * Fh, jt, dy, dx]
    return fr


def pack_gsf_q_frags(w3d, device):
    """conv3D.weight [2][F/2][3][3][3] -> bf16 MFMA A fragments [KS][64][8] for gsf_q_mfma_kernel:
    row n = jg = 2*j_t + g (rows 6..15 zero); k-slot s = 4ks+q = tap*nch + chunk, element e = channel 8*chunk+e,
    non-zero only for channels of gate group g."""
    return _bf16(_gsf_q_frags_np(_np(w3d).astype(np.float32)), device)


def gsf_q_frags_on_device(w3d, to_bf16=_to_bf16):
    """conv3D.weight (2,F/2,3,3,3) fp32 on the device -> the bf16 MFMA fragments of pack_gsf_q_frags (to_bf16: the cast;
    repack.to_bf16 where the copy may be recorded)."""
    return to_bf16(gather_frags(_gsf_q_frags_np, w3d)).contiguous()


def _gsf_p_frags_np(w3d):
    Fh = w3d.shape[1]
    F = 2 * Fh
    nch = (F + 7) // 8
    KSc = (nch + 3) // 4
    fr = np.zeros((4, KSc, 64, 8), np.float32)
    for rt in range(4):
        for n in range(16):
            r = rt * 16 + n
            if r >= 54:
                continue
            tap, jg = divmod(r, 6)
            dy, dx = divmod(tap, 3)
            jt, g = divmod(jg, 2)
            for ks in range(KSc):
                for q in range(4):
                    for e in range(8):
                        c = (4 * ks + q) * 8 + e
                        if c < F and c // Fh == g:
                            fr[rt, ks, q * 16 + n, e] = w3d[g, c - g * Fh, jt, dy, dx]
    return fr


def pack_gsf_p_frags(w3d, device):
    """conv3D.weight [2][F/2][3][3][3] -> bf16 MFMA A fragments [4][ceil(nch/4)][64][8] for the tap-map tail of
    tdeed_bneck_gs_fwd: row r = tap*6 + jg (jg = 2*j_t + g as in pack_gsf_q_frags; rows 54..63 zero), k = channel,
    non-zero only for channels of gate group g -- the 3x3x3 conv as ONE 1x1 contraction to per-tap sums."""
    return _bf16(_gsf_p_frags_np(_np(w3d).astype(np.float32)), device)


def pack_gconv_frags(w, gw, device, tap_major=False):
    """Conv2d.weight [C][gw][3][3] -> bf16 MFMA A-operand fragments [ceil4(C/16)][5][64][8] for
    gconv3x3_mfma_kernel: unit u = output channels [16u,16u+16); lane l holds Wt[n=l&15][k=8(l>>4)+j];
    k-slot s = 4*ks + (l>>4) = half*9 + tap; for gw=8 'half' selects which of the unit's two groups
    the 8 input channels belong to (block-diagonal), for gw=16 which half of the group's 16 inputs.
    tap_major (tdeed_bneck_fwd): s = 2*tap + half -- the two k-slots of a ds_read_b128 lane group then differ by 16 bytes
    at the SAME tap pixel, which is conflict-free at the one-launch bottleneck's even row stride (bneck.hip)."""
    return _bf16(_gconv_frags_np(_np(w).astype(np.float32), gw, tap_major), device)


def _gconv_frags_np(w, gw, tap_major=False):
    C = w.shape[0]
    nu = (C + 15) // 16
    nu4 = (nu + 3) // 4 * 4
    fr = np.zeros((nu4, 5, 64, 8), np.float32)
    for u in range(nu):
        for ks in range(5):
            for q in range(4):
                s_ = 4 * ks + q
                if s_ >= 18:
                    continue
                half, tap = (s_ & 1, s_ >> 1) if tap_major else divmod(s_, 9)
                ky, kx = divmod(tap, 3)
                for n in range(16):
                    co = u * 16 + n
                    if co >= C:
                        continue
                    lane = q * 16 + n
                    if gw == 16:
                        fr[u, ks, lane, :] = w[co, half * 8:half * 8 + 8, ky, kx]
                    elif n // 8 == half:
                        fr[u, ks, lane, :] = w[co, :, ky, kx]
    return fr


def gconv_frag_index(C, gw, device):
    """Index map of pack_gconv_frags: frags = cat([0, w.reshape(-1)])[idx]."""
    return frag_index(_gconv_frags_np, (C, gw, 3, 3), device, gw)


def gconv_frags_on_device(w, gw, to_bf16=_to_bf16):
    """Conv2d.weight (C,gw,3,3) fp32 on the device -> bf16 MFMA fragments (same layout as pack_gconv_frags; to_bf16 as in
    gsf_q_frags_on_device)."""
    return to_bf16(gather_frags(_gconv_frags_np, w, gw)).contiguous()
