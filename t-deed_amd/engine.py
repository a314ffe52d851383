"""Launch plan of the T-DEED inference forward on one MI355X.

``ForwardEngine`` turns a reference-format state_dict into packed device weights (BN folded
into per-channel scale/shift epilogues, depthwise weights packed per channel, dense weights in
the activation dtype) and, per input geometry, a static list of kernel launches over
pre-allocated buffers.  The list is captured once into a HIP graph and replayed: no tracing
compiler, no per-op host work in the steady state.

Mirrors ``TDEEDModel.Impl.forward(x, inference=True)`` (/root/reference/model/model.py:105-149).
"""
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import ops, _lib
from .streams import new_stream
from .regnet_spec import regnet_spec, sgp_up_size, pyramid_lengths, first_site_block
# the weight layouts (also importable from here, where they used to live)
from .packing import (_np, _f32, _dense, pack_ws_weights, pack_se_bf16, pack_mfma_frags, pack_se_mfma,  # noqa: F401
                      pack_front_weights, _stem_frags_np, gs_source_order_columns, _gsf_q_frags_np, pack_gsf_q_frags,
                      _gsf_p_frags_np, pack_gsf_p_frags, pack_gconv_frags, _gconv_frags_np, stem_frags_on_device,
                      gsf_q_frags_on_device, gconv_frag_index, gconv_frags_on_device)

BN_EPS = 1e-5


class _Pool:
    """Free-list of device byte buffers so that dead activations are recycled (keeps the working
    set small enough to live in the 256 MiB Infinity Cache between producer and consumer)."""

    def __init__(self, device):
        self.device = device
        self.free = []
        self.all = []

    def take(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        n = (n + 255) // 256 * 256
        best = None
        for i, b in enumerate(self.free):
            if b.numel() >= n and (best is None or b.numel() < self.free[best].numel()):
                best = i
        if best is not None and self.free[best].numel() <= 2 * n + (1 << 20):
            raw = self.free.pop(best)
        else:
            raw = torch.empty(n, dtype=torch.uint8, device=self.device)
            self.all.append(raw)
        t = raw[:int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)
        t._td_raw = raw
        return t

    def give(self, t):
        self.free.append(t._td_raw)

    def total_bytes(self):
        return sum(b.numel() for b in self.all)


def _dwpack(sd, pre, names, C, device):
    """per-channel depthwise weights [C][sum of taps] and biases [len(names)][C]"""
    ws = [_np(sd[f"{pre}.{n}.weight"]).reshape(C, -1) for n in names]
    bs = [_np(sd[f"{pre}.{n}.bias"]).reshape(C) for n in names]
    return _f32(np.concatenate(ws, axis=1), device), _f32(np.stack(bs, axis=0), device)


SGP_GEMM = os.environ.get("TDEED_SGP_GEMM", "1") == "1"             # the SGP contractions on sgp_gemm.hip (round 5)
# its residual stream (block / mixer inputs and outputs, the stash) in fp32 under a bf16 trunk, like the reference's autocast
SGP_F32_STREAM = os.environ.get("TDEED_SGP_F32_STREAM", "1") == "1"
# feature dimensions above this get a bf16 copy of the fc1 operand beside the fp32 rows (a wide fc1 launch is bound by the
# bytes per CU; narrow ones are latency bound and take the fp32 rows directly)
SGP_BF16_OPERAND_MIN_C = int(os.environ.get("TDEED_SGP_BF16_OPERAND_MIN_C", "384"))


def sgp_stream_dtype(act_dtype, device):
    """type of the temporal stage's residual stream (feat, block / mixer outputs, the stash) for a trunk in act_dtype"""
    if SGP_GEMM and SGP_F32_STREAM and act_dtype == torch.bfloat16 and str(device) != "cpu":
        return torch.float32
    return act_dtype


def _pack_mlp(sd, pre, C, o, act_dtype, device):
    o.w_fc1 = _dense(_np(sd[pre + ".mlp.0.weight"]).reshape(4 * C, C), act_dtype, device)
    o.b_fc1 = _f32(_np(sd[pre + ".mlp.0.bias"]), device)
    o.w_fc2 = _dense(_np(sd[pre + ".mlp.2.weight"]).reshape(C, 4 * C), act_dtype, device)
    o.b_fc2 = _f32(_np(sd[pre + ".mlp.2.bias"]), device)
    o.gn_w, o.gn_b = _f32(_np(sd[pre + ".gn.weight"]), device), _f32(_np(sd[pre + ".gn.bias"]), device)
    o.w1g = o.w2g = None
    if act_dtype == torch.bfloat16 and str(device) != "cpu" and C % 16 == 0 and SGP_GEMM:
        # sgp_gemm.hip: plain MFMA fragments of the whole weight, k-steps padded to its chunk ring
        o.w1g = pack_mfma_frags(_np(sd[pre + ".mlp.0.weight"]).reshape(4 * C, C), device, ks_mult=12)
        o.w2g = pack_mfma_frags(_np(sd[pre + ".mlp.2.weight"]).reshape(C, 4 * C), device, ks_mult=12)


# gate-shift-fuse slice left in source channel order, the module's interleave folded into conv1's weight columns
GS_SRC_ORDER = os.environ.get("TDEED_GS_SRC_ORDER", "1") == "1"
WS_WIDE_MIN_ROWS = 250000     # 0: never the sliced form
RS_MIN_ROWS = int(os.environ.get("TDEED_RS_MIN_ROWS", "60000"))                # 0: never the register-stationary kernel


class DenseW:
    """A dense [N][K] weight in the layout the chosen contraction kernel wants."""

    def __init__(self, W, act_dtype, device, gated=False):
        """gated: the layer is a conv3 (SE gate on its operand + residual)."""
        W = _np(W)
        self.N, self.K = W.shape
        # mode 1: the whole W sits in LDS; mode 2: W does not fit, equal column slices over blockIdx.y (activations re-read per
        # slice, 8 waves per workgroup).
        mode = ops.gemm_ws_fits_mode(self.K, self.N, act_dtype) if str(device) != "cpu" else 0
        self.ws = mode == 1
        # The weight-stationary kernel was built for the narrow RegNetY-200MF layers (24 .. 152 channels), where it wins by
        # 20-35 %; on the 64- and 128-wide layers of the 800MF trunk the tiled kernel is the faster one
        # (tools/bench_ws_vs_gemm.py, us: 64x64 conv1 135 vs 152, conv3 190 vs 221; 128x128 conv3 101 vs 123; conv1 a tie)
        if self.ws and ((self.K == 64 and self.N == 64) or (gated and self.K >= 64 and self.K % 64 == 0)):
            self.ws = False
        self.w = pack_ws_weights(W, act_dtype, device) if self.ws else _dense(W, act_dtype, device)
        # wide layers over MANY rows (the 320-wide s3 layers of RegNetY-800MF at 3 * 10^5 rows): the sliced form reads the
        # activations once per slice instead of once per 64-column tile -- tools/bench_ws_wide.py, M = 313600, K = N = 320: 134
        # vs 180 us.  Below that the operands of the micro-benchmark sit in the Infinity Cache and in the forward, where two
        # sub-batches share the chip, a kernel that takes whole CUs (150 KB of LDS) pushes the other stream's launches out:
        # 800MF B = 16 (156 800 rows per sub-batch) 1437 vs 1460 clips/s with it, cfg2 3525 vs 3560 -- hence the threshold
        self.wide = (not self.ws) and mode == 2 and WS_WIDE_MIN_ROWS > 0
        self.w_wide = pack_ws_weights(W, act_dtype, device) if self.wide else None
        self.kernel = "gemm_ws" if self.ws else "gemm"

    def _use_wide(self, M):
        return self.wide and M is not None and M >= WS_WIDE_MIN_ROWS

    def _use_rs(self, M, kw):
        """register-stationary kernel (K = N = 320, W in the registers of a 10-wave workgroup) -- conv1-shaped calls and, since
        the kernel re-reads its BatchNorm fold from LDS per 16-row tile instead of holding it across the MFMA loops (no spills
        left at its 168-register budget), conv3 with the SE re-scale and the residual too (tools/bench_ws_wide.py at
        M = 313 600: plain 114 vs 181 us tiled, conv3 172 vs 247; the a_scale tile must span at most two frames)"""
        return (RS_MIN_ROWS > 0 and self.wide and M is not None and M >= RS_MIN_ROWS
                and (kw.get("a_scale") is None or kw.get("a_scale_rows", 0) >= 64)
                and kw.get("gather") is None and kw.get("lda") is None and kw.get("ldc") is None
                and ops.gemm_rs_fits(M, self.K, self.N))

    def kern(self, M):
        """kernel family that serves this layer at M rows"""
        return "gemm_ws" if (self.ws or self._use_wide(M)) else "gemm"

    def run(self, A, scale, shift, act, **kw):
        if self.ws:
            return ops.gemm_ws(A, self.w, self.K, self.N, scale, shift, act, **kw)
        if act in (ops.ACT_NONE, ops.ACT_RELU) and self._use_rs(kw.get("M"), kw):
            return ops.gemm_rs(A, self.w_wide, self.K, self.N, scale, shift, act,
                               **{k: v for k, v in kw.items() if k in ("A0", "k0", "out", "M", "out2", "residual", "a_scale",
                                                                       "a_scale_rows")})
        if self._use_wide(kw.get("M")):
            return ops.gemm_ws(A, self.w_wide, self.K, self.N, scale, shift, act, **kw)
        return ops.gemm(A, self.w, scale, shift, act, **kw)


def pack_sgp_block(sd, pre, C, act_dtype, device):
    """SGPBlock parameters (modules.py:91-145) in kernel layout."""
    o = SimpleNamespace(C=C)
    o.ln_w = _f32(_np(sd[pre + ".ln.weight"]).reshape(C), device)
    o.ln_b = _f32(_np(sd[pre + ".ln.bias"]).reshape(C), device)
    o.dw, o.db = _dwpack(sd, pre, ["psi", "convw", "convkw", "fc", "global_fc"], C, device)
    o.ks = _np(sd[pre + ".psi.weight"]).shape[-1]
    o.up = _np(sd[pre + ".convkw.weight"]).shape[-1]
    _pack_mlp(sd, pre, C, o, act_dtype, device)
    return o


def pack_sgp_mixer(sd, pre, C, act_dtype, device):
    """SGPMixer parameters (modules.py:192-254) in kernel layout."""
    o = SimpleNamespace(C=C)
    for n in ("ln1", "ln2"):
        setattr(o, n + "_w", _f32(_np(sd[f"{pre}.{n}.weight"]).reshape(C), device))
        setattr(o, n + "_b", _f32(_np(sd[f"{pre}.{n}.bias"]).reshape(C), device))
    o.dw1, o.db1 = _dwpack(sd, pre, ["psi1", "convw1", "convkw1", "fc1", "global_fc1"], C, device)
    o.dw2, o.db2 = _dwpack(sd, pre, ["psi2", "convw2", "convkw2", "fc2", "global_fc2"], C, device)
    o.ks = _np(sd[pre + ".psi1.weight"]).shape[-1]
    o.up = _np(sd[pre + ".convkw1.weight"]).shape[-1]
    o.w_cat = _dense(_np(sd[pre + ".concat_fc.weight"]).reshape(C, 6 * C), act_dtype, device)
    o.b_cat = _f32(_np(sd[pre + ".concat_fc.bias"]), device)
    o.wcg = (pack_mfma_frags(_np(sd[pre + ".concat_fc.weight"]).reshape(C, 6 * C), device, ks_mult=12)
             if act_dtype == torch.bfloat16 and str(device) != "cpu" and C % 16 == 0 and SGP_GEMM else None)
    _pack_mlp(sd, pre, C, o, act_dtype, device)
    return o


def _se(pooled, inv_cnt, bw, gate):
    """SE excitation: bf16 packed weights in throughput mode, fp32 weights in parity mode."""
    if bw.se_mf is not None:
        return ops.se_gate_mfma(pooled, inv_cnt, bw.se_mf.w1f, bw.se_b1, bw.se_mf.w2f, bw.se_b2, bw.spec.se_rd, out=gate)
    if bw.se_bf is not None:
        return ops.se_gate_bf16(pooled, inv_cnt, bw.se_bf.se_w1p, bw.se_b1, bw.se_bf.se_w2p, bw.se_b2, bw.spec.se_rd, out=gate)
    return ops.se_gate(pooled, inv_cnt, bw.se_w1t, bw.se_b1, bw.se_w2t, bw.se_b2, out=gate)


BNECK_ONE_LAUNCH = os.environ.get("TDEED_BNECK", "1") == "1"
# the gate-shift-fuse blend inside the one-launch bottleneck's frame load (tdeed_bneck_gs_fwd): the site's third launch and the
# round trip of its output slice are gone
BNECK_BLEND = True
# ... and the tap maps of the NEXT block's site in the same launch's tail (tdeed_bneck_gs_fwd's Q): that site's first launch is gone
BNECK_QTAIL = True
C1_GCONV = os.environ.get("TDEED_C1_GCONV", "1") == "1"           # conv1 (+ downsample) computed inside the grouped conv's launch
C1_GCONV_MAX_CIN = 160
# the shortcut conv of a strided block as a second contraction inside conv3's launch (tdeed_gemm_ws_sc_fwd): no `.downsample`
# launch, and the shortcut map is neither written nor read back
SC_IN_CONV3 = True
# conv3 of the block in the fused front (s1.b1) inside the conv1 + grouped-conv launch of the block behind it
# (tdeed_c1_gconv_c3in_fwd): no `s1.b1.conv3` launch, and s1.b1's output map is neither written nor read -- only its pixels at
# even rows and columns, which the shortcut conv of s2.b1 gathers, are stored
S1_CONV3_IN_C1G = True


# The launch form of one bottleneck of a run (block_forms):
# h, w, h2, w2    input and output map size
# one_launch      the whole block is ONE launch (tdeed_bneck_fwd / tdeed_bneck_gs_fwd)
# c1g             conv1 runs inside the grouped conv's launch (tdeed_c1_gconv_fwd): the y1 map never exists
# site, Fp        the block has a gate-shift site; its fold padded to whole 8-channel groups (0 without a site)
# slice_in        the gate-shift launches read the compact slice that the producer of the input wrote beside it
# q_given         the launch in front of the block already wrote the site's tap maps
# blend_in        the site's blend runs inside the one-launch bottleneck's frame load
# qtail           the launch's tail writes the NEXT site's tap maps
# slice_next      channels of the compact slice written for the next block's site (0: none)
# sc_in_conv3     the shortcut conv is a second contraction inside conv3's launch (tdeed_gemm_ws_sc_fwd)
# conv3_in        the conv1 + grouped-conv launch also computes the PRODUCER's conv3 from its y2, shortcut map and gate
#                 (tdeed_c1_gconv_c3in_fwd): the block's input map never exists, its shortcut reads a compact stride-2 copy
BlockForm = namedtuple("BlockForm",
                       "h w h2 w2 one_launch c1g site Fp slice_in q_given blend_in qtail slice_next sc_in_conv3 conv3_in")


def block_forms(blocks, h, w, act_dtype, taps, last_out_is_slice, pending=None):
    """The launch form of every bottleneck of a run over an (h, w) input map: one BlockForm per block.  Pure: decided from the
    block specs, from which packed forms the weights have, from the module switches (read now) and from the library's host
    predicates; nothing is allocated, packed or written.  last_out_is_slice: the last block writes into a slice of a shared
    buffer (no one-launch form: its output is not contiguous).  pending: the weights of the block in the fused front when its
    conv3 has not been emitted yet (the run's input map does not exist so far): the first block may take it in (conv3_in)."""
    forms = []
    for bi, bw in enumerate(blocks):
        blk = bw.spec
        nbw = blocks[bi + 1] if bi + 1 < len(blocks) else None
        # bf16, stride 1, identity shortcut, a map small enough for a workgroup's frames to stay in LDS (s3.b2-b4 and s4.b2-b7
        # of RegNetY-200MF), contiguous output
        one_launch = bool(BNECK_ONE_LAUNCH and getattr(bw, "fused", None) is not None and bw.se_mf is not None
                          and blk.stride == 1 and not blk.has_downsample and blk.cin == blk.cout
                          and not (last_out_is_slice and nbw is None) and ops.bneck_fits(h, w, blk.cout, blk.se_rd))
        # narrow block inputs, bf16 (block inputs up to 160 channels = 5 k-steps of conv1 fragments per wave; s4.b1 of
        # RegNetY-200MF, 152 -> 368: 4072 vs 4002 clips/s with it on the same box)
        c1g = bool(C1_GCONV and not one_launch and act_dtype == torch.bfloat16 and bw.w2frag is not None
                   and blk.cin <= C1_GCONV_MAX_CIN and ops.c1_gconv_fits(h, w, blk.cin, blk.cout, blk.stride))
        site = blk.gsf_fold > 0
        Fp = (blk.gsf_fold + 7) // 8 * 8 if site else 0
        blend_in = bool(site and one_launch and BNECK_BLEND and bw.gs_src and bw.gs_cw1 is not None and h * w >= 14
                        and 2 * Fp <= blk.cin and ("_features." + blk.name + ".gs_out") not in taps)
        # the gate-shift launches read only channels [0, Fp) of their input: every producer writes them once more as a compact
        # slice beside its output (a slice of the channels-last map drags whole cache lines)
        slice_next = (nbw.spec.gsf_fold + 7) // 8 * 8 if (nbw is not None and nbw.spec.gsf_fold) else 0
        # (the tail's input slice is the block's own output rows)
        qtail = bool(blend_in and BNECK_QTAIL and slice_next and getattr(nbw, "gs_wqf", None) is not None
                     and ops.bneck_qtail_fits(h, w, blk.cout, nbw.spec.gsf_fold))
        sc_in_conv3 = bool(SC_IN_CONV3 and blk.has_downsample and act_dtype == torch.bfloat16 and bw.w3.ws and bw.wd.ws
                           and ops.gemm_ws_sc_fits(blk.cout, blk.cin, blk.cout, act_dtype))
        h2, w2 = (h - 1) // blk.stride + 1, (w - 1) // blk.stride + 1
        slice_in, q_given = bool(site and forms and forms[-1].slice_next == Fp), bool(forms and forms[-1].qtail)
        # the producer's conv3 in this block's first launch: nobody else may read the producer's output (no site here, no tap
        # there), its conv3 is one k-step of the weight-stationary kernel, and this block has a shortcut conv (stride 2)
        conv3_in = bool(S1_CONV3_IN_C1G and pending is not None and bi == 0 and c1g and not site and blk.stride == 2
                        and blk.has_downsample and act_dtype == torch.bfloat16 and pending.w3.ws
                        and pending.spec.cout == blk.cin and ("_features." + pending.spec.name) not in taps
                        and ops.c1_gconv_c3in_fits(h, w, blk.cin, blk.cout))
        forms.append(BlockForm(h, w, h2, w2, one_launch, c1g, site, Fp, slice_in, q_given, blend_in, qtail, slice_next, sc_in_conv3,
                               conv3_in))
        h, w = h2, w2
    return forms


class Step:
    """One kernel launch of a plan with its algorithmic cost (what a perfect kernel must move / compute)."""
    __slots__ = ("name", "kernel", "fn", "bytes", "flops")

    def __init__(self, name, kernel, fn, nbytes=0, flops=0):
        self.name, self.kernel, self.fn, self.bytes, self.flops = name, kernel, fn, int(nbytes), int(flops)


def _esz(dt):
    return 2 if dt == torch.bfloat16 else 4


def gemm_cost(M, K, N, es, residual=False, extra=0):
    return (M * K + N * K + M * N * (2 if residual else 1)) * es + extra, 2 * M * K * N


class SgpBuilder:
    """Appends the launches of SGP blocks / mixers / the whole encoder-decoder to a step list."""

    def __init__(self, pool, steps, keep, taps, B, act_dtype):
        self.pool, self.steps, self.keep, self.taps, self.B, self.dt = pool, steps, keep, taps, B, act_dtype
        self.splitk_rows = 4096
        # fused launches (sgp_fused.hip): LayerNorm inside the branch kernels (both dtypes), GroupNorm + fc1 + GELU + fc2 +
        # residual in one MFMA launch (bf16).  TDEED_SGP_FUSED=0 restores the launch-per-op chain (A/B measurements).
        self.fused = os.environ.get("TDEED_SGP_FUSED", "1") == "1"
        # round 5: the contractions on sgp_gemm.hip (full K per workgroup, no fp32 partials, no fold launches); `adt` is the
        # type of the stage's residual stream -- fp32 under a bf16 trunk unless TDEED_SGP_F32_STREAM=0
        self.gemm = SGP_GEMM and act_dtype == torch.bfloat16
        # (the residual stream's type is the type of what the stage is handed: sgp_stream_dtype() for the model's plans)

    def _mlp_gemm(self, name, y, o, Tn, chsum, pool_to=None, y16=None):
        """out = y + mlp(GN(y)) as two sgp_gemm launches; leaves the output's partial row sums on it (`_td_rowstat`) and, when
        the following AdaptiveMaxPool1d halves the length, the pooled rows in `self.last_pooled`."""
        pool, steps, B, C = self.pool, self.steps, self.B, o.C
        R, adt = B * Tn, y.dtype
        es = _esz(adt)
        ya = y if y16 is None else y16           # fc1's operand: the rows themselves, or their bf16 copy (wide models, fp32 stream)
        f1 = ops.sgp_gemm_form(0 if ya.dtype == torch.bfloat16 else 3, B, Tn, 4 * C, C)
        f2 = ops.sgp_gemm_form(1, B, Tn, C, 4 * C)
        nct = ops.sgp_gemm_tiles(Tn, C, f2)[1]
        H = pool.take((B, Tn, 4 * C), torch.bfloat16)
        outb = pool.take((B, Tn, C), adt)
        rsp = torch.empty((nct, R, 2), dtype=torch.float32, device=y.device)          # lives as long as the plan (tiny)
        pooled = rpp = None
        if pool_to is not None and 2 * pool_to == Tn:
            pooled = pool.take((B, pool_to, C), adt)
            rpp = torch.empty((nct, B * pool_to, 2), dtype=torch.float32, device=y.device)
            pooled._td_rowstat = rpp
        self.last_pooled = pooled
        steps.append(Step(name + ".fc1", "sgp_gemm", lambda: ops.sgp_gemm_gn_gelu(ya, chsum, o.gn_w, o.gn_b, o.w1g, o.b_fc1, 4 * C,
                                                                                out=H, form=f1),
                          R * C * _esz(ya.dtype) + 4 * C * C * 2 + R * 4 * C * 2, 2 * R * 4 * C * C))
        steps.append(Step(name + ".fc2", "sgp_gemm", lambda: ops.sgp_gemm_residual(H, o.w2g, o.b_fc2, y, out=outb, rowstat_part=rsp,
                                                                                 pooled=pooled, rowstat_pool_part=rpp, form=f2),
                          R * 4 * C * 2 + 4 * C * C * 2 + 2 * R * C * es + (0 if pooled is None else B * pool_to * C * es),
                          2 * R * 4 * C * C))
        pool.give(H)
        outb._td_rowstat = rsp
        return outb

    def dense(self, name, A, Wt, bias, act, out, R, residual=None):
        """One Conv1d(k=1) of the mlp / concat_fc.  Short sequences (bf16, <= splitk_rows rows) go through the split-K
        kernel: a tiled contraction would be ~40 workgroups each walking K in 20+ dependent round trips."""
        N, K = Wt.shape
        es = _esz(self.dt)
        if (self.dt == torch.bfloat16 and R <= self.splitk_rows
                and ops.gemm_splitk_splits(K) >= 4):      # K = 4C / 6C; for K = C the tiled kernel is faster (11 vs 15 us)
            ws = self.pool.take((ops.gemm_splitk_splits(K), R, N), torch.float32)
            self.steps.append(Step(name, "gemm_splitk", lambda: ops.gemm_splitk(A, Wt, None, bias, act, residual=residual,
                                                                                 out=out, M=R, workspace=ws),
                                   *gemm_cost(R, K, N, es, residual is not None)))
            self.pool.give(ws)
        else:
            self.steps.append(Step(name, "gemm", lambda: ops.gemm(A, Wt, None, bias, act, residual=residual, out=out, M=R),
                                   *gemm_cost(R, K, N, es, residual is not None)))

    def _mlp(self, name, y, o, outb, Tn):
        """out = y + mlp(GN(y)) as groupnorm + two contractions (fp32 mode and TDEED_SGP_GEMM=0; the bf16 path is _mlp_gemm)."""
        pool, steps, B, C, dt = self.pool, self.steps, self.B, o.C, self.dt
        es, R = _esz(dt), B * Tn
        self.last_pooled = None
        gn = pool.take((B, Tn, C), dt)
        hid = pool.take((B, Tn, 4 * C), dt)
        steps.append(Step(name + ".gn", "groupnorm", lambda: ops.groupnorm(y, 16, o.gn_w, o.gn_b, out=gn), 2 * R * C * es))
        self.dense(name + ".fc1", gn, o.w_fc1, o.b_fc1, ops.ACT_GELU, hid, R)
        self.dense(name + ".fc2", hid, o.w_fc2, o.b_fc2, ops.ACT_NONE, outb, R, residual=y)
        pool.give(gn)
        pool.give(hid)

    def _tap(self, name, outb):
        if name in self.taps:
            self.keep[name] = outb
        return outb

    def block(self, xin, Tn, o, name, pool_to=None):
        """One SGPBlock.  pool_to: length of the AdaptiveMaxPool1d that follows (encoder half); when the MLP launch can
        carry it, `self.last_pooled` holds the pooled tensor afterwards (else None: the caller adds a max-pool launch)."""
        pool, steps, B, C, dt = self.pool, self.steps, self.B, o.C, self.dt
        self.last_pooled = None
        R, wl = B * Tn, 2 * o.ks + o.up + 2
        if self.fused:
            gemm = self.gemm and getattr(o, "w1g", None) is not None      # the MLP on sgp_gemm.hip, over the stream's own type
            adt = xin.dtype if gemm else dt
            es = _esz(adt)
            y = pool.take((B, Tn, C), adt)
            y16 = pool.take((B, Tn, C), torch.bfloat16) if (gemm and adt == torch.float32 and C > SGP_BF16_OPERAND_MIN_C) else None
            chs = pool.take((B, C, 2), torch.float32) if gemm else None
            outb = None if gemm else pool.take((B, Tn, C), dt)            # (_mlp_gemm takes its own)
            rs_in = getattr(xin, "_td_rowstat", None)          # LayerNorm statistics left by the producer of xin (avgpool_posenc)
            steps.append(Step(name + ".front", "sgp_front", lambda: ops.sgp_front(xin, o.ks, o.up, o.ln_w, o.ln_b, o.dw, o.db,
                                                                                 out=y, chsum=chs, rowstat=rs_in, out16=y16),
                              2 * R * C * es + C * (wl + 7) * 4 + (0 if y16 is None else R * C * 2), 2 * R * C * (wl + 3)))
            if gemm:
                outb = self._mlp_gemm(name, y, o, Tn, chs, pool_to=pool_to, y16=y16)
            else:
                self._mlp(name, y, o, outb, Tn)
            for t_ in (y, y16, chs):
                if t_ is not None:
                    pool.give(t_)
            return self._tap(name, outb)
        ln = pool.take((B, Tn, C), dt)
        y = pool.take((B, Tn, C), dt)
        gn = pool.take((B, Tn, C), dt)
        hid = pool.take((B, Tn, 4 * C), dt)
        outb = pool.take((B, Tn, C), dt)
        es = _esz(dt)
        steps.append(Step(name + ".ln", "layernorm", lambda: ops.layernorm(xin, o.ln_w, o.ln_b, out=ln), 2 * R * C * es))
        steps.append(Step(name + ".branch", "sgp_branch", lambda: ops.sgp_branch(ln, xin, o.ks, o.up, o.dw, o.db, out=y),
                          3 * R * C * es + C * (wl + 5) * 4, 2 * R * C * (wl + 3)))
        steps.append(Step(name + ".gn", "groupnorm", lambda: ops.groupnorm(y, 16, o.gn_w, o.gn_b, out=gn), 2 * R * C * es))
        self.dense(name + ".fc1", gn, o.w_fc1, o.b_fc1, ops.ACT_GELU, hid, R)
        self.dense(name + ".fc2", hid, o.w_fc2, o.b_fc2, ops.ACT_NONE, outb, R, residual=y)
        for t_ in (ln, y, gn, hid):
            pool.give(t_)
        return self._tap(name, outb)

    def mixer(self, xlo, T_lo, z, T_hi, o, name):
        pool, steps, B, C, dt = self.pool, self.steps, self.B, o.C, self.dt
        R, Rl, wl = B * T_hi, B * T_lo, 2 * o.ks + o.up + 2
        if self.fused:
            gemm = self.gemm and getattr(o, "wcg", None) is not None      # concat_fc and the MLP on sgp_gemm.hip
            adt = z.dtype if gemm else dt
            if gemm and xlo.dtype != adt:
                raise TypeError("SgpBuilder.mixer: z and x_lo must share the residual stream's type")
            es = _esz(adt)
            cat = pool.take((B, T_hi, 6 * C), torch.bfloat16 if gemm else dt)
            if not gemm:
                mo = pool.take((B, T_hi, C), dt)
                outb = pool.take((B, T_hi, C), dt)
            rs_z, rs_x = getattr(z, "_td_rowstat", None), getattr(xlo, "_td_rowstat", None)
            steps.append(Step(name + ".front", "mixer_front",
                              lambda: ops.mixer_front(z, xlo, cat, o.ks, o.up, o.ln1_w, o.ln1_b, o.ln2_w, o.ln2_b, o.dw1,
                                                      o.db1, o.dw2, o.db2, rowstat_z=rs_z, rowstat_x=rs_x),
                              (R + Rl) * C * es + 6 * R * C * _esz(cat.dtype) + 2 * C * (wl + 7) * 4, 4 * R * C * (wl + 3)))
            if not gemm:
                self.dense(name + ".cat", cat, o.w_cat, o.b_cat, ops.ACT_GELU, mo, R)
                self._mlp(name, mo, o, outb, T_hi)
                pool.give(cat)
                pool.give(mo)
                return self._tap(name, outb)
            fc = ops.sgp_gemm_form(2, B, T_hi, C, 6 * C)
            NJ = ops.sgp_gemm_tiles(T_hi, C, fc)[0]
            mo = pool.take((B, T_hi, C), adt)
            mo16 = pool.take((B, T_hi, C), torch.bfloat16) if (adt == torch.float32 and C > SGP_BF16_OPERAND_MIN_C) else None
            chs = pool.take((NJ, B, C, 2), torch.float32)
            steps.append(Step(name + ".cat", "sgp_gemm", lambda: ops.sgp_gemm_gelu_chsum(cat, o.wcg, o.b_cat, C, mo, chs, form=fc,
                                                                                       out16=mo16),
                              R * 6 * C * 2 + 6 * C * C * 2 + R * C * es + (0 if mo16 is None else R * C * 2), 2 * R * 6 * C * C))
            pool.give(cat)
            outb = self._mlp_gemm(name, mo, o, T_hi, chs, y16=mo16)
            pool.give(mo)
            if mo16 is not None:
                pool.give(mo16)
            pool.give(chs)
            return self._tap(name, outb)
        cat = pool.take((B, T_hi, 6 * C), dt)
        xn = pool.take((B, T_lo, C), dt)
        mo = pool.take((B, T_hi, C), dt)
        gn = pool.take((B, T_hi, C), dt)
        hid = pool.take((B, T_hi, 4 * C), dt)
        outb = pool.take((B, T_hi, C), dt)
        zslab = cat.view(-1)[4 * C:]
        es = _esz(dt)
        steps.append(Step(name + ".ln1", "layernorm", lambda: ops.layernorm(z, o.ln1_w, o.ln1_b, out=zslab, ldy=6 * C,
                                                                            rows=R, C=C), 2 * R * C * es))
        steps.append(Step(name + ".ln2", "layernorm", lambda: ops.layernorm(xlo, o.ln2_w, o.ln2_b, out=xn), 2 * Rl * C * es))
        steps.append(Step(name + ".branch", "mixer_branch",
                          lambda: ops.mixer_branch(xn, cat, T_hi, o.ks, o.up, o.dw1, o.db1, o.dw2, o.db2),
                          (6 * R + Rl) * C * es + 2 * C * (wl + 5) * 4, 4 * R * C * (wl + 3)))
        self.dense(name + ".cat", cat, o.w_cat, o.b_cat, ops.ACT_GELU, mo, R)
        steps.append(Step(name + ".gn", "groupnorm", lambda: ops.groupnorm(mo, 16, o.gn_w, o.gn_b, out=gn), 2 * R * C * es))
        self.dense(name + ".fc1", gn, o.w_fc1, o.b_fc1, ops.ACT_GELU, hid, R)
        self.dense(name + ".fc2", hid, o.w_fc2, o.b_fc2, ops.ACT_NONE, outb, R, residual=mo)
        for t_ in (cat, xn, mo, gn, hid):
            pool.give(t_)
        return self._tap(name, outb)

    def pyramid(self, feat, T, n, sgp, mixers, pre="_temp_fine."):
        """EDSGPMIXERLayers.forward (modules.py:69-87) on an NTC tensor."""
        pool, steps, B, dt = self.pool, self.steps, self.B, self.dt
        C = sgp[0].C
        lens = pyramid_lengths(T, n)
        cur = feat
        stash = []
        for i in range(n):
            cur = self.block(cur, lens[i], sgp[i], f"{pre}_sgp.{i}", pool_to=lens[i + 1])
            stash.append(cur)
            pooled = self.last_pooled
            if pooled is None:
                pooled = pool.take((B, lens[i + 1], C), cur.dtype)
                if self.gemm and self.fused:
                    # lengths that do not halve: a pooling launch that also leaves the pooled rows' LayerNorm statistics
                    prs = torch.empty((B * lens[i + 1], 2), dtype=torch.float32, device=cur.device)
                    pooled._td_rowstat = prs
                    steps.append(Step(f"{pre}pool{i}", "maxpool", lambda a=cur, b=pooled, L=lens[i + 1], r=prs:
                                      ops.maxpool_rowstat(a, L, out=b, rowstat=r), B * (lens[i] + lens[i + 1]) * C * _esz(cur.dtype)))
                else:
                    steps.append(Step(f"{pre}pool{i}", "maxpool", lambda a=cur, b=pooled, L=lens[i + 1]: ops.maxpool(a, L, out=b),
                                      B * (lens[i] + lens[i + 1]) * C * _esz(cur.dtype)))
            cur = pooled
        cur = self.block(cur, lens[n], sgp[n], f"{pre}_sgp.{n}")
        for i in range(n):
            lvl = n - 1 - i
            cur = self.mixer(cur, lens[lvl + 1], stash[lvl], lens[lvl], mixers[lvl], f"{pre}_sgpMixer.{lvl}")
            cur = self.block(cur, lens[lvl], sgp[n + 1 + i], f"{pre}_sgp.{n + 1 + i}")
        return cur


TrunkGeometry = namedtuple("TrunkGeometry", "crop ch cw maps")


def centre_window(H, W, ch, cw):
    """(top, left, ch, cw) of the centre window of ch x cw pixels in an H x W frame: the crop rectangle of the first launch,
    and of everything that has to cut the same pixels (evalutil.ResidentJpegVideos)"""
    return (int(round((H - ch) / 2.0)), int(round((W - cw) / 2.0)), ch, cw)


def trunk_geometry(blocks, crop, H, W):
    """Map sizes of the trunk over H x W frames.  Pure.  blocks: the block specs; crop: side of the centre crop (None or 0:
    none).  crop: the rectangle (top, left, ch, cw) the first launch reads (None: the whole frame), ch, cw: its size;
    maps[k]: (h, w, channels) of the map that block k reads -- maps[0] is the stem's output, maps[len(blocks)] the trunk's."""
    ch, cw, rect = H, W, None
    if crop is not None and crop > 0 and (crop != H or crop != W):
        ch = cw = crop
        rect = centre_window(H, W, ch, cw)
    h, w = (ch + 1) // 2, (cw + 1) // 2
    maps = [(h, w, blocks[0].cin)]
    for blk in blocks:
        h, w = (h - 1) // blk.stride + 1, (w - 1) // blk.stride + 1
        maps.append((h, w, blk.cout))
    return TrunkGeometry(rect, ch, cw, maps)


class SubPlan:
    """One chain of launches of a plan, issued on one stream: those of a sub-batch (`frames` is their input buffer; h, w: the
    size of the map they end in, where they stop inside the trunk) or, with frames = None, those behind the sub-batches' join
    over all the plan's clips.  sgp_out: the encoder-decoder's output, where the chain holds the temporal stage."""
    __slots__ = ("frames", "steps", "keep", "head_out", "pool_bytes", "B", "T", "h", "w", "sgp_out")

    def __init__(self, frames, steps, keep, head_out, pool_bytes, B, T, h=None, w=None):
        self.frames, self.steps, self.keep, self.head_out, self.pool_bytes = frames, steps, keep, head_out, pool_bytes
        self.B, self.T, self.h, self.w, self.sgp_out = B, T, h, w, keep.get("sgp_out")


class Plan:
    """What run_plan launches: subs[i] on streams[i] (None: the launching stream), then `tail` behind their join."""
    __slots__ = ("subs", "streams", "tail", "steps", "head_out", "keep", "graph", "pool_bytes", "B", "T", "trunk_map", "out", "h",
                 "w", "trunk_in", "flip_buf")

    def __init__(self, subs, head_out, B, T, streams=None, tail=None, trunk_map=None, out=None, h=None, w=None, trunk_in=None,
                 flip_buf=None):
        self.subs, self.streams, self.tail = subs, streams or [None] * len(subs), tail
        chains = subs + ([] if tail is None else [tail])
        self.steps = [st for c in chains for st in c.steps]
        self.pool_bytes = sum(c.pool_bytes for c in chains)
        self.head_out, self.keep, self.graph, self.B, self.T = head_out, (subs[0].keep if subs else {}), None, B, T
        self.trunk_map, self.out, self.h, self.w, self.trunk_in, self.flip_buf = trunk_map, out, h, w, trunk_in, flip_buf


# the block in the fused front while its SE + conv3 are still to be emitted; behind bw its temporaries, in the order taken
_Front = namedtuple("_Front", "bw y2 sc pooled gate")


class TrunkBuilder:
    """Appends the launches of B clips -- the trunk (fused front or stem, bottlenecks), the pooling, the temporal stage with
    the heads: the three stages below -- to a step list of its own over a buffer pool of its own."""

    def __init__(self, pw, act_dtype, device, taps, B, fuse_front=True):
        self.pw, self.act_dtype, self.device, self.taps, self.B, self.fuse_front = pw, act_dtype, device, taps, B, fuse_front
        self.pool, self.steps, self.keep = _Pool(device), [], {}
        self.N = B * pw.clip_len
        self.frames = self.head_out = None
        self.front = None          # the _Front of a trunk whose first block sits in the fused front, until its conv3 is emitted
        # fp32 fragments of the stem weight (packing.stem_frags_on_device): set by a caller that wants the un-fused bf16 stem
        # on the MFMA kernel's eval instance (prefix.EvalPrefix); None: tdeed_stem_fwd
        self.stem_wf = None

    # ------------------------------------------------------------------ bottlenecks
    def _se_conv3(self, bw, h2, w2, y2, pooled, gate, sc, out, out2=None, sc_from=None):
        """The last two steps of a bottleneck that is not one launch: the SE excitation from the grouped conv's pooled sums,
        and conv3 with the gate on its operand + shortcut `sc` + ReLU (out2: the next block's gate-shift slice beside `out`).
        sc_from = (x, gather): no `sc` map -- conv3's launch computes the shortcut conv from the block's input x itself."""
        blk, es, N, M2 = bw.spec, _esz(self.act_dtype), self.N, self.N * h2 * w2
        se = Step(blk.name + ".se", "se_gate", lambda: _se(pooled, 1.0 / (h2 * w2), bw, gate),
                  2 * N * blk.cout * 4 + 2 * blk.cout * blk.se_rd * 4, 4 * N * blk.cout * blk.se_rd)
        if sc_from is not None:
            x, gather = sc_from
            return (se, Step(blk.name + ".conv3", "gemm_ws", lambda: ops.gemm_ws_sc(
                y2, bw.w3.w, blk.cout, blk.cout, bw.s3, bw.h3, x, bw.wd.w, blk.cin, bw.sd, bw.hd, ops.ACT_RELU, a_scale=gate,
                a_scale_rows=h2 * w2, gather=gather, out=out, M=M2, out2=out2),
                # y2, the gathered rows of x, out, both weights
                (M2 * (2 * blk.cout + blk.cin) + blk.cout * (blk.cout + blk.cin)) * es,
                2 * M2 * blk.cout * (blk.cout + blk.cin)))
        return (se, Step(blk.name + ".conv3", bw.w3.kern(M2), lambda: bw.w3.run(
            y2, bw.s3, bw.h3, ops.ACT_RELU, residual=sc, a_scale=gate, a_scale_rows=h2 * w2, out=out, M=M2, out2=out2),
            *gemm_cost(M2, blk.cout, blk.cout, es, True)))

    def _block_done(self, blk, dead, x, x_kept, out):
        """A bottleneck's epilogue: its temporaries `dead` and its input x (unless a tap keeps it, or it is not the pool's) go
        back to the pool, its output is recorded when it is a tap.  Returns whether the output must be kept."""
        for t_ in dead:
            self.pool.give(t_)
        if not x_kept and hasattr(x, "_td_raw"):
            self.pool.give(x)
        tapname = "_features." + blk.name
        if tapname in self.taps:
            self.keep[tapname] = out
        return tapname in self.taps

    def _gs_site(self, bw, f, xg, q):
        """Appends the gate-shift launch of a block's site over xg (the block's input, or its compact slice) and returns the
        site's buffers.  q: the site's tap maps where the launch in front of the block wrote them (f.q_given).  Under
        f.blend_in the launch leaves only the gates and the sums (the blend runs inside the bottleneck's launch); otherwise
        gb["out"] is the blended slice that conv1 splices in."""
        pool, B, blk, T = self.pool, self.B, bw.spec, self.pw.clip_len
        N, F, Fp = self.N, blk.gsf_fold, f.Fp
        M = N * f.h * f.w
        gb = dict(gate=pool.take((N, f.h, f.w, 2), torch.float32),
                  q=(q if f.q_given else pool.take((N, f.h, f.w, 6), torch.float32)),
                  ysum=pool.take((N, F), torch.float32),
                  xsum=pool.take((N, F), torch.float32))
        if not f.blend_in:
            gb["out"] = pool.take((M, Fp), self.act_dtype)
            if bw.gs_cw1 is not None:
                gb["fw"] = pool.take((B, F, T), torch.float32)
        self.steps.append(Step(blk.name + ".gate_shift", "gate_shift", lambda: ops.gate_shift(
            xg, B, T, F, Fp, bw.gs_scale, bw.gs_shift, bw.gs_wq, bw.gs_b3d, bw.gs_cw1, bw.gs_cb1,
            bw.gs_cw2, bw.gs_cb2, bufs=gb, wqf=bw.gs_wqf, src_order=bw.gs_src, gates_only=f.blend_in, q_given=f.q_given),
            M * ((1 if f.blend_in else 2) * F + (0 if f.blend_in else Fp)) * _esz(self.act_dtype) + M * 16, 2 * M * F * 27))
        tap = "_features." + blk.name + ".gs_out"
        if tap in self.taps:
            if bw.gs_src:
                raise ValueError("the gs_out tap is in module channel order: build the engine with TDEED_GS_SRC_ORDER=0")
            self.keep[tap] = gb["out"]
        return gb

    def _one_launch(self, bw, f, x, xg, gb, nbw):
        """Appends a bottleneck as ONE launch, conv1 (+ splice) -> conv2 -> SE -> conv3 + shortcut: only x and the output cross
        HBM.  gb: the buffers of the block's site ({} without one), xg: what the site read, nbw: the next block's weights.
        Returns the output, the next site's compact slice and the next site's tap maps (None where the form has none)."""
        pool, blk, T, dt = self.pool, bw.spec, self.pw.clip_len, self.act_dtype
        N, es = self.N, _esz(dt)
        M = N * f.h * f.w
        out = pool.take((N, f.h, f.w, blk.cout), dt)
        xs_next = pool.take((N, f.h, f.w, f.slice_next), dt) if f.slice_next else None
        o2 = xs_next.view(-1, f.slice_next) if f.slice_next else None
        q_next = None
        if f.blend_in:
            qt = None
            if f.qtail:
                q_next = pool.take((N, f.h, f.w, 6), torch.float32)
                qt = (nbw.gs_wpf, nbw.gs_bnq, nbw.spec.gsf_fold, q_next)
            run = lambda: ops.bneck_gs(                                                                       # noqa: E731
                x, xg, gb["gate"], gb["ysum"], gb["xsum"], bw.gs_cw1, bw.gs_cb1, bw.gs_cw2, bw.gs_cb2, T, blk.gsf_fold, f.Fp,
                bw.fused.w1f, bw.s1, bw.h1, bw.fused.w2f, bw.s2, bw.h2, bw.se_mf.w1f, bw.se_b1, bw.se_mf.w2f, bw.se_b2,
                blk.se_rd, bw.fused.w3f, bw.s3, bw.h3, out=out, out2=o2, w2_tap_major=bw.fused.w2_tap_major, qtail=qt)
        else:
            G = gb.get("out")
            run = lambda: ops.bneck(                                                                          # noqa: E731
                x, bw.fused.w1f, bw.s1, bw.h1, bw.fused.w2f, bw.s2, bw.h2, bw.se_mf.w1f, bw.se_b1, bw.se_mf.w2f, bw.se_b2,
                blk.se_rd, bw.fused.w3f, bw.s3, bw.h3, G=G, out=out, out2=o2, w2_tap_major=bw.fused.w2_tap_major)
        self.steps.append(Step(blk.name + ".bneck", "bneck", run,
                               # x in, out; with the blend: each slice piece's temporal neighbour and the gate maps; the tail's Q
                               (2 * M * blk.cout + (M * f.Fp if f.blend_in else 0)) * es + (8 * M if f.blend_in else 0)
                               + (24 * M if f.qtail else 0)
                               + (2 * blk.cout * blk.cout + blk.cout * blk.gw * 9) * es,
                               2 * M * blk.cout * (2 * blk.cout + blk.gw * 9)))
        return out, xs_next, q_next

    def _chain(self, bw, f, x, y1, G, out, dead_site):
        """Appends a bottleneck as a chain of launches: conv1 into y1 and the grouped conv, or both in one launch (f.c1g, no
        y1); SE; the shortcut conv, unless conv3's launch computes it (f.sc_in_conv3); conv3.  G: the blended slice of the
        block's site that conv1 splices in (None without a site), out: where the block writes instead of a pool buffer,
        dead_site: the site's buffers.  Under f.conv3_in the first launch computes the conv3 of the fused front's block
        (self.front) from its y2 / sc / gate -- there is no x; the shortcut reads the compact stride-2 map that launch writes.
        Returns the output, the next site's compact slice and everything that dies here."""
        pool, steps, blk, dt = self.pool, self.steps, bw.spec, self.act_dtype
        N, es, s = self.N, _esz(dt), blk.stride
        h, w, h2, w2 = f.h, f.w, f.h2, f.w2
        M, M2 = N * h * w, N * h2 * w2
        if y1 is not None:
            splice = dict(A0=G, k0=f.Fp) if f.site else {}
            steps.append(Step(blk.name + ".conv1", bw.w1.kern(M), lambda: bw.w1.run(
                x, bw.s1, bw.h1, ops.ACT_RELU, out=y1, M=M, **splice), *gemm_cost(M, blk.cin, blk.cout, es)))
        y2 = pool.take((N, h2, w2, blk.cout), dt)
        parts = ops.gconv3x3_parts(h, w, blk.cout, s, dt) if bw.w2frag is not None else 1
        pooled = pool.take((N, parts, blk.cout), torch.float32)
        gate = pool.take((N, blk.cout), torch.float32)
        if f.c1g and bw.c1g_w1f is None:
            bw.c1g_w1f = pack_mfma_frags(bw.w1_raw, self.device, rows=16 * ops.c1_gconv_slab_tiles(h, w, blk.cout, s))
        xs2 = None
        if f.conv3_in:
            front, self.front = self.front, None
            pbw = front.bw
            xs2 = pool.take((N, h2, w2, blk.cin), dt)
            steps.append(Step(blk.name + ".conv1_conv2", "c1_gconv", lambda: ops.c1_gconv_c3in(
                front.y2, front.sc, front.gate, pbw.w3.w, pbw.s3, pbw.h3, bw.c1g_w1f, bw.s1, bw.h1, bw.w2frag, bw.s2, bw.h2,
                blk.gw, blk.cout, xs2=xs2, out=y2, pooled=pooled),
                # the producer's y2 and shortcut map in, this block's y2 and the compact map out, the three weights
                (2 * M * blk.cin + M2 * blk.cout + M2 * blk.cin) * es + (blk.cin * blk.cin + blk.cout * (blk.cin + blk.gw * 9)) * es,
                2 * M * blk.cin * blk.cin + 2 * M * blk.cin * blk.cout + 2 * M2 * blk.cout * blk.gw * 9))
            for t_ in front[1:]:                                            # the front block's temporaries die with that launch
                pool.give(t_)
            x = xs2
        elif f.c1g:
            steps.append(Step(blk.name + ".conv1_conv2", "c1_gconv", lambda: ops.c1_gconv(
                x, bw.c1g_w1f, bw.s1, bw.h1, bw.w2frag, bw.s2, bw.h2, blk.gw, s, blk.cout, G=G, out=y2, pooled=pooled),
                (M * blk.cin + M2 * blk.cout) * es + blk.cout * (blk.cin + blk.gw * 9) * es,
                2 * M * blk.cin * blk.cout + 2 * M2 * blk.cout * blk.gw * 9))
        else:
            steps.append(Step(blk.name + ".conv2", "gconv3x3", lambda: ops.gconv3x3(
                y1, bw.w2, bw.s2, bw.h2, blk.gw, s, wfrag=bw.w2frag, out=y2, pooled=pooled),
                (M + M2) * blk.cout * es + blk.cout * blk.gw * 9 * 4, 2 * M2 * blk.cout * blk.gw * 9))
        sc, shortcut, sc_from = x, [], None
        gather = (s, h, w, h2, w2) if (s > 1 and xs2 is None) else None      # (the compact map holds the gathered rows)
        if f.sc_in_conv3:
            sc, sc_from = None, (x, gather)
        elif blk.has_downsample:
            sc = pool.take((N, h2, w2, blk.cout), dt)
            shortcut = [Step(blk.name + ".downsample", bw.wd.kern(M2), lambda: bw.wd.run(
                x, bw.sd, bw.hd, ops.ACT_NONE, gather=gather, out=sc, M=M2), *gemm_cost(M2, blk.cin, blk.cout, es))]
        if out is None:
            out = pool.take((N, h2, w2, blk.cout), dt)
        xs_next = pool.take((N, h2, w2, f.slice_next), dt) if f.slice_next else None
        se, conv3 = self._se_conv3(bw, h2, w2, y2, pooled, gate, sc, out, out2=xs_next, sc_from=sc_from)
        steps += [se, *shortcut, conv3]                     # (the shortcut conv launches between the two)
        # liveness: everything but `out` (and the next block's slice) dies here
        return out, xs_next, (([y1] if y1 is not None else []) + [y2, pooled, gate] + dead_site + ([sc] if shortcut else [])
                              + ([xs2] if xs2 is not None else []))

    def _blocks(self, x, h, w, blocks, x_kept, out_last=None):
        """Appends the launches of a run of bottlenecks, each in the form that block_forms chose; x (N,h,w,Cin) is the input
        map (owned by the pool unless x_kept).  out_last: where the last block writes its output (a slice of a buffer shared
        with the plan that continues the trunk) instead of a pool buffer.  Behind the fused front (self.front) x does not
        exist yet: the front block's SE + conv3 are appended here, conv3 as its own launch into a map x or, when the first
        block takes it in (conv3_in), inside that block's first launch.  Returns (x, h, w, x_kept)."""
        pool, N, dt, fr = self.pool, self.N, self.act_dtype, self.front
        xs = q = None       # the compact slice and the tap maps of the coming block's site, where the launch in front wrote them
        forms = block_forms(blocks, h, w, dt, self.taps, out_last is not None, *(() if fr is None else (fr.bw,)))
        if fr is not None:
            if forms and forms[0].conv3_in:
                self.steps.append(self._se_conv3(fr.bw, h, w, fr.y2, fr.pooled, fr.gate, fr.sc, None)[0])
            else:
                x = pool.take((N, h, w, fr.bw.spec.cout), dt)
                self.steps += self._se_conv3(fr.bw, h, w, fr.y2, fr.pooled, fr.gate, fr.sc, x)
                x_kept = self._block_done(fr.bw.spec, fr[1:], None, True, x)
                self.front = None
        for bi, f in enumerate(forms):
            bw, last = blocks[bi], bi + 1 == len(blocks)
            # (conv1's map is taken in front of the site's buffers: the pool is best-fit, so the order of takes decides which
            # buffer a tensor lands in)
            y1 = None if (f.one_launch or f.c1g) else pool.take((N, f.h, f.w, bw.spec.cout), dt)
            xg = xs if f.slice_in else x
            gb = self._gs_site(bw, f, xg, q) if f.site else {}
            dead = list(gb.values()) + ([xs] if f.slice_in else [])
            if f.one_launch:
                out, xs, q = self._one_launch(bw, f, x, xg, gb, None if last else blocks[bi + 1])
            else:
                out, xs, dead = self._chain(bw, f, x, y1, gb.get("out"), out_last if last else None, dead)
                q = None
            x_kept = self._block_done(bw.spec, dead, x, x_kept, out)
            x, h, w = out, f.h2, f.w2
        return x, h, w, x_kept

    # ------------------------------------------------------------------ the three stages
    def trunk(self, H, W, crop, flip, frames_dtype=torch.uint8, stop=None, out_last=None, rect=None, frames=None):
        """Stage 1: the fused front or the stem over self.frames (N,3,H,W), made here, and the blocks [0, stop) (None: all).
        crop: side of the centre crop (None: the caller's window as it is); flip: bool (all frames) or a uint8 device tensor
        (N,) of per-frame flags (the augmented eval path); out_last: see _blocks.  rect: instead of `crop`, a LIST
        [top, left, ch, cw] that the first launch reads at every run (the caller may move the window between runs, not resize
        it); frames: the caller's input buffer instead of one made here.  Returns (x, h, w, x_kept) of its map."""
        Wt, pool, steps, N, dt, es = self.pw.W, self.pool, self.steps, self.N, self.act_dtype, _esz(self.act_dtype)
        if rect is not None:
            geo = trunk_geometry(self.pw.spec.blocks, None, rect[2], rect[3])
            win = lambda: tuple(rect)                                                                        # noqa: E731
        else:
            geo = trunk_geometry(self.pw.spec.blocks, crop, H, W)
            win = lambda: geo.crop                                                                           # noqa: E731
        ch, cw, (Ho, Wo, c0) = geo.ch, geo.cw, geo.maps[0]
        if frames is None:
            frames = torch.empty((N, 3, H, W), dtype=frames_dtype, device=self.device)
        self.frames = frames
        blocks = list(Wt.blocks[:stop])
        if (Wt.front is not None and "_features.stem" not in self.taps and self.fuse_front and frames_dtype == torch.uint8
                and blocks and not isinstance(flip, torch.Tensor) and ops.s1_front_parts(ch, cw, Wt.blocks[0].spec.cout) > 0):
            bw = blocks.pop(0)
            blk, (h, w, _) = bw.spec, geo.maps[1]
            parts, M2 = ops.s1_front_parts(ch, cw, blk.cout), N * h * w
            y2 = pool.take((N, h, w, blk.cout), dt)
            sc = pool.take((N, h, w, blk.cout), dt)
            pooled = pool.take((N, parts, blk.cout), torch.float32)
            gate = pool.take((N, blk.cout), torch.float32)
            steps.append(Step("s1_front", "s1_front", lambda: ops.s1_front(
                frames, Wt.front, win(), flip, y2=y2, shortcut=sc, pooled=pooled),
                              N * 3 * ch * cw + 2 * M2 * blk.cout * es,
                              2 * N * Ho * Wo * 32 * (27 + 2 * blk.cout) // 1 + 2 * M2 * blk.cout * blk.gw * 9))
            # the block's SE + conv3 follow in _blocks, where the form of the block behind decides how conv3 is launched
            self.front = _Front(bw, y2, sc, pooled, gate)
            x, x_kept = None, True
        else:
            x, h, w = pool.take((N, Ho, Wo, c0), dt), Ho, Wo
            if self.stem_wf is not None and dt == torch.bfloat16 and ops.stem_mfma_parts(ch, cw) > 0:
                # the eval instance of the training stem's MFMA kernel (a frozen prefix inside the training step)
                wf = self.stem_wf
                steps.append(Step("stem", "stem_mfma", lambda: ops.stem_mfma_eval(frames, wf, Wt.stem_scale, Wt.stem_shift, win(),
                                                                                flip, out=x),
                                  N * 3 * ch * cw * (4 if frames_dtype == torch.float32 else 1) + N * Ho * Wo * 32 * es,
                                  2 * N * Ho * Wo * 32 * 27))
            else:
                steps.append(Step("stem", "stem", lambda: ops.stem(frames, Wt.stem_w, Wt.stem_scale, Wt.stem_shift, dt, win(),
                                                                   flip, out=x),
                                  N * 3 * ch * cw + N * Ho * Wo * 32 * es, 2 * N * Ho * Wo * 32 * 27))
            x_kept = "_features.stem" in self.taps
            if x_kept:
                self.keep["_features.stem"] = x
        if out_last is not None and not blocks:
            raise ValueError("join_at must leave at least one un-fused bottleneck in the sub-batch plans")
        return self._blocks(x, h, w, blocks, x_kept, out_last=out_last)

    def avgpool(self, x, h, w, x_kept, feat=None, frs=None):
        """Stage 2: avg-pool + positional encoding of the trunk's map x into feat (default: a pool buffer of the temporal
        stage's stream type), with the LayerNorm statistics of the feature rows for the first SGP block's front kernel (frs:
        the caller's slice of a shared buffer); x goes back to the pool unless x_kept.  Returns feat."""
        pw, Wt, B, C = self.pw, self.pw.W, self.B, self.pw.spec.feat_dim
        if feat is None:
            feat = self.pool.take((B, pw.clip_len, C), sgp_stream_dtype(self.act_dtype, self.device))
        if frs is None:
            frs = torch.empty((self.N, 2), dtype=torch.float32, device=self.device)
        feat._td_rowstat = frs
        self.steps.append(Step("avgpool", "avgpool_posenc", lambda: ops.avgpool_posenc(x, B, pw.clip_len, Wt.temp_enc, out=feat,
                                                                                      rowstat=frs),
                               (self.N * h * w + self.N) * C * _esz(self.act_dtype)))
        self.keep["feat"] = feat
        if not x_kept:
            self.pool.give(x)
        return feat

    def sgp_heads(self, feat, head_out=None):
        """Stage 3: the SGP encoder-decoder over feat (its output: keep["sgp_out"]) and the heads into head_out (default: a
        buffer of its own)."""
        pw, Wt, N, C = self.pw, self.pw.W, self.N, self.pw.spec.feat_dim
        if head_out is None:
            head_out = torch.empty((N, pw.n_out), dtype=torch.float32, device=self.device)
        self.head_out = head_out
        cur = SgpBuilder(self.pool, self.steps, self.keep, self.taps, self.B, self.act_dtype).pyramid(
            feat, pw.clip_len, pw.n_layers, Wt.sgp, Wt.mixer)
        self.steps.append(Step("heads", "heads", lambda: ops.heads(cur, Wt.head_w, Wt.head_b, out=head_out),
                               N * C * _esz(self.act_dtype) + N * pw.n_out * 4, 2 * N * C * pw.n_out))
        self.keep["sgp_out"] = cur

    def sub_plan(self, h=None, w=None):
        return SubPlan(self.frames, self.steps, self.keep, self.head_out, self.pool.total_bytes(), self.B, self.pw.clip_len, h, w)


class PackedWeights:
    """Device-side weights in kernel layouts.  ``state``: reference key grammar."""

    def __init__(self, cfg, state, act_dtype, device):
        g = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        self.arch = g("feature_arch")
        self.spec = regnet_spec(self.arch)
        self.mode = "gsm" if self.arch.endswith("_gsm") else ("gsf" if self.arch.endswith("_gsf") else None)
        self.clip_len = g("clip_len")
        self.n_layers = g("n_layers")
        self.ks = g("sgp_ks")
        self.up = sgp_up_size(self.ks, g("sgp_r"))
        self.radi = g("radi_displacement")
        self.act_dtype = act_dtype
        self.device = device
        sd = {k: _np(v) for k, v in state.items()}
        self.double_head = "_pred_fine._fc1._fc_out.weight" in sd
        f32 = lambda a: _f32(a, device)                                                          # noqa: E731
        bf16_gpu = act_dtype == torch.bfloat16 and str(device) != "cpu"       # the MFMA forms exist on the card only

        def bn_fold(pre):
            w, b = sd[pre + ".weight"].astype(np.float64), sd[pre + ".bias"].astype(np.float64)
            m, v = sd[pre + ".running_mean"].astype(np.float64), sd[pre + ".running_var"].astype(np.float64)
            s = w / np.sqrt(v + BN_EPS)
            return f32(s), f32(b - m * s)

        W = SimpleNamespace()
        p = "_features."
        W.stem_w = f32(sd[p + "stem.conv.weight"].reshape(32, 27))
        W.stem_scale, W.stem_shift = bn_fold(p + "stem.bn")
        W.blocks = []
        for blk in self.spec.blocks:
            bp = p + blk.name
            bw = SimpleNamespace(spec=blk)
            c1 = bp + (".conv1.net" if blk.gsf_fold else ".conv1")
            w1_mat = _np(sd[c1 + ".conv.weight"]).reshape(blk.cout, blk.cin)
            # gate-shift-fuse sites of the bf16 engine: the module's channel interleave is folded into conv1's columns (the
            # blend launch leaves its slice in source channel order, ops.gate_shift(src_order=True)): column ci of the
            # packed weight is the column of the output channel that source channel ci is interleaved to
            bw.gs_src = bool(blk.gsf_fold and GS_SRC_ORDER and self.mode == "gsf" and bf16_gpu)
            if bw.gs_src:
                w1_mat = gs_source_order_columns(w1_mat, blk.gsf_fold)
            bw.w1 = DenseW(w1_mat, act_dtype, device)
            bw.w1_raw = w1_mat
            bw.wd_raw = _np(sd[bp + ".downsample.conv.weight"]).reshape(blk.cout, blk.cin) if blk.has_downsample else None
            bw.c1g_w1f = None    # conv1 / downsample as MFMA fragments padded to whole channel slabs
                                              # (tdeed_c1_gconv_fwd), packed on first use
            bw.s1, bw.h1 = bn_fold(c1 + ".bn")
            w2 = sd[bp + ".conv2.conv.weight"]                       # [C][gw][3][3]
            G, gw = blk.groups, blk.gw
            w2 = w2.reshape(G, gw, gw, 3, 3).transpose(0, 3, 4, 2, 1)  # [G][ky][kx][in][out]
            bw.w2 = f32(w2.reshape(G, 9, gw, gw))
            bw.s2, bw.h2 = bn_fold(bp + ".conv2.bn")
            bw.w2frag = pack_gconv_frags(sd[bp + ".conv2.conv.weight"], gw, device) if act_dtype == torch.bfloat16 else None
            bw.se_w1t = f32(sd[bp + ".se.fc1.weight"].reshape(blk.se_rd, blk.cout).T)
            bw.se_b1 = f32(sd[bp + ".se.fc1.bias"])
            bw.se_w2t = f32(sd[bp + ".se.fc2.weight"].reshape(blk.cout, blk.se_rd).T)
            bw.se_b2 = f32(sd[bp + ".se.fc2.bias"])
            bw.se_bf = (SimpleNamespace(**pack_se_bf16(sd[bp + ".se.fc1.weight"], sd[bp + ".se.fc2.weight"], device))
                        if bf16_gpu else None)
            bw.se_mf = (SimpleNamespace(**pack_se_mfma(sd[bp + ".se.fc1.weight"], sd[bp + ".se.fc2.weight"], device))
                        if (bf16_gpu and ops.se_gate_mfma_fits(blk.cout, blk.se_rd)) else None)
            bw.w3 = DenseW(sd[bp + ".conv3.conv.weight"].reshape(blk.cout, blk.cout), act_dtype, device, gated=True)
            # MFMA-fragment copies of conv1 / conv3 for the one-launch bottleneck (stride-1 identity blocks up to 384 wide)
            bw.fused = (SimpleNamespace(w1f=pack_mfma_frags(w1_mat, device),
                                        w2f=pack_gconv_frags(sd[bp + ".conv2.conv.weight"], gw, device, tap_major=(gw == 8)),
                                        w2_tap_major=(gw == 8),
                                        w3f=pack_mfma_frags(sd[bp + ".conv3.conv.weight"].reshape(blk.cout, blk.cout), device))
                        if (bw.se_mf is not None and blk.stride == 1 and not blk.has_downsample and blk.cin == blk.cout
                            and blk.cout <= 384) else None)
            bw.s3, bw.h3 = bn_fold(bp + ".conv3.bn")
            if blk.has_downsample:
                bw.wd = DenseW(sd[bp + ".downsample.conv.weight"].reshape(blk.cout, blk.cin), act_dtype, device)
                bw.sd, bw.hd = bn_fold(bp + ".downsample.bn")
            if blk.gsf_fold:
                gp = bp + ".conv1.gs"
                F = blk.gsf_fold
                bw.gs_scale, bw.gs_shift = bn_fold(gp + ".bn")
                w3d = sd[gp + ".conv3D.weight"]                       # [2][F/2][3][3][3]
                bw.gs_wq = f32(w3d.reshape(F, 27).T)                  # [27][F], c = g*F/2 + cl
                bw.gs_b3d = f32(sd[gp + ".conv3D.bias"])
                bw.gs_wqf = pack_gsf_q_frags(w3d, device) if bf16_gpu else None
                bw.gs_bnq = ops.gsq_bn_table(bw.gs_scale, bw.gs_shift) if bw.gs_wqf is not None else None
                bw.gs_wpf = pack_gsf_p_frags(w3d, device) if bw.gs_wqf is not None else None
                if self.mode == "gsf":
                    bw.gs_cw1 = f32(sd[gp + ".channel_conv1.weight"].reshape(18))
                    bw.gs_cb1 = f32(sd[gp + ".channel_conv1.bias"])
                    bw.gs_cw2 = f32(sd[gp + ".channel_conv2.weight"].reshape(18))
                    bw.gs_cb2 = f32(sd[gp + ".channel_conv2.bias"])
                else:
                    bw.gs_cw1 = bw.gs_cb1 = bw.gs_cw2 = bw.gs_cb2 = None
            W.blocks.append(bw)
        W.front = None
        b0 = self.spec.blocks[0]
        if bf16_gpu and b0.stride == 2 and b0.has_downsample and b0.cout <= 64 and not b0.gsf_fold:
            bw0, bp0 = W.blocks[0], p + b0.name
            W.front = pack_front_weights(
                sd[p + "stem.conv.weight"], W.stem_scale, W.stem_shift,
                sd[bp0 + ".conv1.conv.weight"].reshape(b0.cout, b0.cin), bw0.s1, bw0.h1,
                sd[bp0 + ".downsample.conv.weight"].reshape(b0.cout, b0.cin), bw0.sd, bw0.hd,
                sd[bp0 + ".conv2.conv.weight"], b0.gw, bw0.s2, bw0.h2, device)
        W.temp_enc = f32(sd["temp_enc"])
        C = self.spec.feat_dim

        W.sgp = [pack_sgp_block(sd, f"_temp_fine._sgp.{i}", C, act_dtype, device) for i in range(2 * self.n_layers + 1)]
        W.mixer = [pack_sgp_mixer(sd, f"_temp_fine._sgpMixer.{i}", C, act_dtype, device) for i in range(self.n_layers)]
        if self.double_head:
            hw = [sd["_pred_fine._fc1._fc_out.weight"], sd["_pred_fine._fc2._fc_out.weight"]]
            hb = [sd["_pred_fine._fc1._fc_out.bias"], sd["_pred_fine._fc2._fc_out.bias"]]
        else:
            hw, hb = [sd["_pred_fine._fc_out.weight"]], [sd["_pred_fine._fc_out.bias"]]
        self.n_cls = int(sum(w.shape[0] for w in hw))
        if self.radi > 0:
            hw.append(sd["_pred_displ._fc_out.weight"])
            hb.append(sd["_pred_displ._fc_out.bias"])
        W.head_w = f32(np.concatenate(hw, axis=0))
        W.head_b = f32(np.concatenate(hb, axis=0))
        self.n_out = W.head_w.shape[0]
        self.displ_col = self.n_cls if self.radi > 0 else -1
        self.W = W


_DEAD_GRAPHS = []          # graph executables of dropped engines, destroyed by _drain_dead_graphs()
_CAPTURING = 0


def _drain_dead_graphs():
    """Destroy the graph executables of engines that were garbage-collected (safe point: no capture in progress; the device
    is synchronised first so that none of them is still executing)."""
    if not _DEAD_GRAPHS or _CAPTURING:
        return
    torch.cuda.synchronize()
    while _DEAD_GRAPHS:
        _lib.call("tdeed_graph_destroy", _DEAD_GRAPHS.pop())


class ForwardEngine:
    def __init__(self, cfg, state, act_dtype=torch.bfloat16, device="cuda", use_graph=True, fuse_front=True, n_split=2):
        if not torch.cuda.is_available():
            raise RuntimeError("tdeed_amd.ForwardEngine needs an MI355X (no CPU path)")
        _lib.load()
        self.cfg = cfg
        g = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        self.crop_dim = g("crop_dim")
        self.pw = PackedWeights(cfg, state, act_dtype, device)
        self.act_dtype = act_dtype
        self.device = device
        self.use_graph = use_graph
        self.fuse_front = fuse_front
        self.n_split = int(os.environ.get("TDEED_SPLIT", n_split))
        # the temporal stage (SGP encoder-decoder + heads) of a split batch runs ONCE over all clips behind the join of the
        # sub-batch trunks: its launches are latency bound and their cost does not depend on the row count at these sizes
        self.merge_tail = True
        # where the sub-batch pipelines join inside the trunk (index into the block list; None = behind the last block)
        self.join_at = None
        self._plans = {}
        self._frame_starts = {}

    # ------------------------------------------------------------------ plan construction
    def _builder(self, B, taps=()):
        return TrunkBuilder(self.pw, self.act_dtype, self.device, set(taps), B, self.fuse_front)

    def _geometry(self, H, W):
        return trunk_geometry(self.pw.spec.blocks, self.crop_dim, H, W)

    def _whole(self, B, H, W, flip, taps=(), crop=None, head_out=None, frames_dtype=torch.uint8):
        """Sub-plan of a whole forward of B clips: the three stages in a row."""
        tb = self._builder(B, taps)
        feat = tb.avgpool(*tb.trunk(H, W, crop, flip, frames_dtype))
        tb.sgp_heads(feat, head_out)
        return tb.sub_plan()

    def _head(self, B, H, W, flip, k, out):
        """Sub-plan of the trunk's head for B clips: the front or stem and the blocks [0, k), the last one writing into `out`."""
        tb = self._builder(B)
        _, h, w, _ = tb.trunk(H, W, self.crop_dim, flip, stop=k, out_last=out)
        return tb.sub_plan(h, w)

    def _tail(self, B, feat, head_out, trunk_in=None, k=None):
        """The launches behind the sub-batch join, over all B clips: optionally the rest of the trunk (the blocks from k on, over
        the map `trunk_in` = (x, h, w) that the sub-batch plans wrote) + avg-pool, then SGP encoder-decoder + heads."""
        tb = self._builder(B)
        if trunk_in is not None:
            x, h, w, _ = tb._blocks(*trunk_in, list(self.pw.W.blocks[k:]), True)
            # (x_kept: the trunk's last map is not given back, so the temporal stage takes no buffer of the trunk's size)
            tb.avgpool(x, h, w, True, feat)
        tb.sgp_heads(feat, head_out)
        return tb.sub_plan()

    def plan(self, B, H, W, flip=False, taps=(), slot=0):
        """Launch plan for a batch geometry.  With n_split > 1 (and no taps) the batch is cut into n_split
        sub-batches of whole clips, each with its own buffers and its own HIP stream: two half-batch
        pipelines in flight keep the CUs busy while the other one sits in a latency-bound small launch."""
        # slot: independent buffer sets / graphs of the same geometry, so that consecutive batches can be in flight together
        key = (B, H, W, bool(flip), tuple(sorted(taps)), slot)
        if key in self._plans:
            return self._plans[key]
        flip, T, dev = bool(flip), self.pw.clip_len, self.device
        ns = self.n_split if (not taps and self.n_split > 1 and B % self.n_split == 0 and B >= self.n_split) else 1
        if ns == 1:
            sub = self._whole(B, H, W, flip, taps, self.crop_dim)
            plan = Plan([sub], sub.head_out, B, T)
        else:
            Bs = B // ns
            rows = [slice(i * Bs * T, (i + 1) * Bs * T) for i in range(ns)]          # the frames of sub-batch i
            head_out = torch.empty((B * T, self.pw.n_out), dtype=torch.float32, device=dev)
            tail = trunk_map = None
            if not self.merge_tail:
                subs = [self._whole(Bs, H, W, flip, (), self.crop_dim, head_out=head_out[r]) for r in rows]
            else:
                feat = torch.empty((B, T, self.pw.spec.feat_dim), dtype=sgp_stream_dtype(self.act_dtype, dev), device=dev)
                k = self.join_at
                if k is not None and 0 < k < len(self.pw.W.blocks):
                    # the sub-batches split only the bandwidth-bound head of the trunk (blocks [0, k)); the latency-bound
                    # small maps behind it run once for the whole batch, like the temporal stage
                    hh, ww, cc = self._geometry(H, W).maps[k]
                    trunk_map = torch.empty((B * T, hh, ww, cc), dtype=self.act_dtype, device=dev)
                    subs = [self._head(Bs, H, W, flip, k, trunk_map[r]) for r in rows]
                    tail = self._tail(B, feat, head_out, trunk_in=(trunk_map, hh, ww), k=k)
                else:
                    frs = torch.empty((B * T, 2), dtype=torch.float32, device=dev)
                    feat._td_rowstat = frs
                    subs = []
                    for i, r in enumerate(rows):          # trunk and pooling into the sub-batch's rows of the shared features
                        tb = self._builder(Bs)
                        tb.avgpool(*tb.trunk(H, W, self.crop_dim, flip), feat[i * Bs:(i + 1) * Bs], frs[r])
                        subs.append(tb.sub_plan())
                    tail = self._tail(B, feat, head_out)
            forks = []
            for _ in range(ns - 1):
                forks.append(new_stream(dev, avoid=forks))
            # (trunk_map: the block-join_at input of all B clips, None without a trunk join)
            plan = Plan(subs, head_out, B, T, streams=[None] + forks, tail=tail, trunk_map=trunk_map)
        self._plans[key] = plan
        return plan

    def set_frames(self, plan, frames_u8):
        """Copy a (B,T,3,H,W) uint8 batch into the plan's input buffers (one per sub-batch)."""
        B, T = frames_u8.shape[:2]
        Bs = B // len(plan.subs)
        for i, sb in enumerate(plan.subs):
            sb.frames.copy_(frames_u8[i * Bs:(i + 1) * Bs].reshape(Bs * T, *frames_u8.shape[2:]), non_blocking=True)

    # ------------------------------------------------------------------ execution
    def _launch_all(self, plan, main):
        """Issue every sub-batch's launches: sub-batch 0 on `main`, the others forked onto their own streams; then the tail's."""
        joins = []
        if len(plan.subs) > 1:
            fork = torch.cuda.Event()
            fork.record(main)
        for sb, st in zip(plan.subs, plan.streams):
            if st is None or st.cuda_stream == main.cuda_stream:   # (the pool handed the launching stream out again)
                for s_ in sb.steps:
                    s_.fn()
            else:
                st.wait_event(fork)
                with torch.cuda.stream(st):
                    for s_ in sb.steps:
                        s_.fn()
                    ev = torch.cuda.Event()
                    ev.record(st)
                    joins.append(ev)
        for ev in joins:
            main.wait_event(ev)
        if plan.tail is not None:
            for s_ in plan.tail.steps:
                s_.fn()

    def _capture(self, st, fn):
        """Capture what fn() launches on stream `st` into a graph executable (fn has run once already: modules loaded,
        arguments validated)."""
        import ctypes
        import gc
        # no cyclic garbage collection between begin and end of the capture: the finaliser of an engine that an earlier
        # caller dropped would otherwise run here at a random allocation and call into the HIP runtime (graph
        # destruction, frees) from the capturing thread -- the graph launched afterwards then crashed the host
        global _CAPTURING
        gc_was = gc.isenabled()
        gc.disable()
        _CAPTURING += 1
        _lib.call("tdeed_graph_begin", st.cuda_stream)
        try:
            fn()
        finally:
            h = ctypes.c_void_p()
            try:
                _lib.call("tdeed_graph_end", st.cuda_stream, ctypes.byref(h))
            finally:
                _CAPTURING -= 1
                if gc_was:
                    gc.enable()
        return h

    def run_plan(self, plan):
        """Launch the plan on the current stream (eager) or replay its HIP graph(s)."""
        st = torch.cuda.current_stream()
        if not self.use_graph:
            self._launch_all(plan, st)
            return
        if st.cuda_stream == 0:
            raise RuntimeError("graph replay needs a non-default stream: wrap the call in torch.cuda.stream(s)")
        if plan.graph is None:
            _drain_dead_graphs()
            self._launch_all(plan, st)         # warm-up launch (module load, validates arguments)
            st.synchronize()
            plan.graph = self._capture(st, lambda: self._launch_all(plan, st))   # forked streams join through the fork event
        _lib.call("tdeed_graph_launch", plan.graph, st.cuda_stream)

    def forward(self, frames_u8, augment_inference=False, taps=(), slot=0):
        """frames: uint8 (B,T,3,H,W) on the GPU.  Returns head_out fp32 (B*T, n_cls [+1]) (a view of the plan's buffer:
        consume it on the launching stream before the same slot runs again)."""
        if frames_u8.dtype != torch.uint8:
            raise TypeError("frames must be uint8 (0..255); callers holding floats convert with .to(torch.uint8)")
        B, T, Cc, H, W = frames_u8.shape
        if T != self.pw.clip_len:
            raise ValueError(f"clip length {T} != clip_len {self.pw.clip_len} (gate-shift needs exact clips)")
        plan = self.plan(B, H, W, augment_inference, taps, slot=slot)
        self.set_frames(plan, frames_u8)
        self.run_plan(plan)
        return plan.head_out, plan

    def forward_from_video(self, video_u8, starts_dev, augment_inference=False, slot=0, clip_base=None, clip_len_v=None,
                           ring=None):
        """forward() over clip windows of a frame buffer that is resident on the device: video_u8 uint8 (L,3,H,W), starts_dev
        int32 (B,) on the device (first frame of each clip; windows that hang over either end are zero padded like the
        evaluation reader's).  The windows are gathered straight into the plan's input buffers (ops.clip_gather, one launch
        per sub-batch) in place of set_frames' copy of a materialised batch; same plan keys and graphs as forward(), so the
        result carries the same bits as forward() on the materialised windows.
        clip_base / clip_len_v (int32 (B,) on the device, both or neither): video_u8 packs several videos, clip b belongs to
        the one that starts at packed frame clip_base[b] and has clip_len_v[b] frames, starts_dev is local to it and the
        window is padded at that video's ends (ops.clip_gather_seg).
        ring = (ring_frames, L_total): video_u8 is a ring of ring_frames rows of a packed buffer of L_total frames, packed
        frame p in row p % ring_frames (ops.clip_gather_ring; needs the tables).  Only the gather differs."""
        if (clip_base is None) != (clip_len_v is None):
            raise ValueError("clip_base and clip_len_v go together")
        if ring is not None and clip_base is None:
            raise ValueError("a frame ring is gathered with the group's tables (clip_base, clip_len_v)")
        if video_u8.dtype != torch.uint8 or video_u8.dim() != 4 or not video_u8.is_cuda:
            raise TypeError("video frames must be a uint8 (L,3,H,W) tensor on the device")
        if starts_dev.dtype != torch.int32 or starts_dev.dim() != 1 or not starts_dev.is_cuda:
            raise TypeError("clip starts must be an int32 (B,) tensor on the device")
        B = starts_dev.numel()
        _, _, H, W = video_u8.shape
        plan = self.plan(B, H, W, augment_inference, (), slot=slot)
        Bs = B // len(plan.subs)
        for i, sb in enumerate(plan.subs):
            part = slice(i * Bs, (i + 1) * Bs)
            if clip_base is None:
                ops.clip_gather(video_u8, starts_dev[part], self.pw.clip_len, sb.frames)
            elif ring is not None:
                ops.clip_gather_ring(video_u8, ring[0], ring[1], starts_dev[part], clip_base[part], clip_len_v[part],
                                     self.pw.clip_len, sb.frames)
            else:
                ops.clip_gather_seg(video_u8, starts_dev[part], clip_base[part], clip_len_v[part], self.pw.clip_len, sb.frames)
        self.run_plan(plan)
        return plan.head_out, plan

    # ------------------------------------------------------------------ whole videos: the per-frame trunk stages once per frame
    def first_site_block(self):
        """Index k of the first block with a gate-shift site: the stem and the blocks [0, k) are functions of one frame."""
        return first_site_block(self.pw.spec)

    def _reuse_k(self):
        k = self.first_site_block()
        if not 0 < k < len(self.pw.W.blocks):
            raise ValueError(f"frame reuse needs a gate-shift site behind the first block ({self.pw.arch}: k = {k})")
        return k

    def frame_map_shape(self, H, W):
        """(h, w, C) of one frame's row of the resident map: the input of block first_site_block()."""
        return self._geometry(H, W).maps[self._reuse_k()]

    def frame_plan(self, Bf, H, W, flip=False):
        """Plan of the per-frame head of the trunk -- stem and blocks [0, k), k = first_site_block() -- for Bf * clip_len
        consecutive FRAMES (no clip structure: nothing in front of block k mixes frames): plan.subs[0].frames is the input,
        plan.out (Bf*T, h, w, C) the block-k input map of those frames.  The launches are those of a sub-batch of Bf clips of a
        join_at = k plan.  Replays as a HIP graph through run_plan."""
        key = ("frames", Bf, H, W, bool(flip))
        if key in self._plans:
            return self._plans[key]
        k, T = self._reuse_k(), self.pw.clip_len
        hh, ww, cc = self._geometry(H, W).maps[k]
        out = torch.empty((Bf * T, hh, ww, cc), dtype=self.act_dtype, device=self.device)
        plan = Plan([self._head(Bf, H, W, bool(flip), k, out)], None, Bf, T, out=out, h=hh, w=ww)
        self._plans[key] = plan
        return plan

    def tail_plan(self, B, h, w, slot=0):
        """Plan of everything behind the per-frame head for B clips -- blocks [k:], pooling, SGP encoder-decoder, heads -- on a
        fixed input buffer plan.trunk_in (B*T, h, w, C): the tail of a join_at = k plan.  One per slot; the flipped view needs
        none of its own (the flip happens at the frames)."""
        key = ("tail", B, h, w, slot)
        if key in self._plans:
            return self._plans[key]
        k, T = self._reuse_k(), self.pw.clip_len
        cc = self._geometry(h, w).maps[k][2]          # (the channels do not depend on the frame size)
        buf = torch.empty((B * T, h, w, cc), dtype=self.act_dtype, device=self.device)
        head_out = torch.empty((B * T, self.pw.n_out), dtype=torch.float32, device=self.device)
        feat = torch.empty((B, T, self.pw.spec.feat_dim), dtype=sgp_stream_dtype(self.act_dtype, self.device), device=self.device)
        plan = Plan([], head_out, B, T, tail=self._tail(B, feat, head_out, trunk_in=(buf, h, w), k=k), trunk_in=buf)
        self._plans[key] = plan
        return plan

    def frame_maps(self, video_u8, first_frame, maps_out, Bf, flip=False):
        """Run the frame plan over the Bf * clip_len frames of video_u8 (L,3,H,W) from `first_frame` on (frames past the end
        are black: ops.clip_gather's padding) and store their maps in maps_out (Bf*T, h, w, C), a slice of the resident map."""
        T = self.pw.clip_len
        _, _, H, W = video_u8.shape
        plan = self.frame_plan(Bf, H, W, flip)
        key = (Bf, int(first_frame))
        starts = self._frame_starts.get(key)
        if starts is None:             # (built once per chunk position: nothing is uploaded in the steady state)
            starts = self._frame_starts[key] = torch.arange(int(first_frame), int(first_frame) + Bf * T, T, dtype=torch.int32,
                                                            device=self.device)
        ops.clip_gather(video_u8, starts, T, plan.subs[0].frames)
        self.run_plan(plan)
        maps_out.copy_(plan.out, non_blocking=True)
        return plan

    def forward_from_frame_maps(self, maps, starts_dev, pad_row, slot=0, clip_base=None, clip_len_v=None, n_frames=None):
        """forward_from_video over the resident per-frame maps instead of the frames: maps (rows, h, w, C) in the activation
        dtype, row f the block-k input map of frame f (frame_maps), rows >= n_frames (default: pad_row) those of black frames
        and pad_row one of them; starts_dev int32 (B,) on the device, clip_base / clip_len_v as in forward_from_video.  The
        windows are gathered into the tail plan's input (ops.rows_gather[_seg], launched in front of the replay) and the tail
        runs.  Returns head_out (a view of the slot's buffer) and the plan."""
        if (clip_base is None) != (clip_len_v is None):
            raise ValueError("clip_base and clip_len_v go together")
        if maps.dtype != self.act_dtype or maps.dim() != 4 or not maps.is_cuda:
            raise TypeError(f"frame maps must be a {self.act_dtype} (rows,h,w,C) tensor on the device")
        if starts_dev.dtype != torch.int32 or starts_dev.dim() != 1 or not starts_dev.is_cuda:
            raise TypeError("clip starts must be an int32 (B,) tensor on the device")
        B, T = starts_dev.numel(), self.pw.clip_len
        _, h, w, cc = maps.shape
        plan = self.tail_plan(B, h, w, slot)
        if tuple(plan.trunk_in.shape[1:]) != (h, w, cc):
            raise ValueError(f"frame maps of {(h, w, cc)}, block {self._reuse_k()} reads {tuple(plan.trunk_in.shape[1:])}")
        L = int(pad_row if n_frames is None else n_frames)
        if clip_base is None:
            ops.rows_gather(maps, starts_dev, L, int(pad_row), T, plan.trunk_in)
        else:
            ops.rows_gather_seg(maps, starts_dev, clip_base, clip_len_v, L, int(pad_row), T, plan.trunk_in)
        self.run_plan(plan)
        return plan.head_out, plan

    def forward_augmented(self, frames, flip_frames=None):
        """Eval-mode forward (running-statistics BatchNorm) of frames that the caller has already cropped / augmented:
        frames (B,T,3,h,w) uint8 or fp32 0..255 on the GPU, flip_frames: optional uint8 (B*T,) per-frame h-flip flags.
        What `Impl.forward(inference=False)` runs under .eval() (model/model.py:105-129 with the BatchNorms in eval mode).
        Eager launches of a cached plan (fp32 frames and per-frame flips go through the stand-alone stem kernel)."""
        if frames.dtype not in (torch.uint8, torch.float32):
            raise TypeError("frames must be uint8 or float32 (0..255)")
        B, T, Cc, H, W = frames.shape
        if T != self.pw.clip_len:
            raise ValueError(f"clip length {T} != clip_len {self.pw.clip_len} (gate-shift needs exact clips)")
        key = ("aug", B, H, W, frames.dtype, flip_frames is not None)
        plan = self._plans.get(key)
        if plan is None:
            fbuf = torch.zeros((B * T,), dtype=torch.uint8, device=self.device) if flip_frames is not None else None
            # (crop=None: the caller's window, no centre crop on top of it)
            sub = self._whole(B, H, W, False if fbuf is None else fbuf, crop=None, frames_dtype=frames.dtype)
            plan = self._plans[key] = Plan([sub], sub.head_out, B, T, flip_buf=fbuf)
        plan.subs[0].frames.copy_(frames.reshape(B * T, Cc, H, W), non_blocking=True)
        if flip_frames is not None:
            plan.flip_buf.copy_(flip_frames.to(torch.uint8), non_blocking=True)
        self._launch_all(plan, torch.cuda.current_stream())
        return plan.head_out, plan

    def __del__(self):
        # graph executables are not destroyed from a finaliser (it may run at any allocation, e.g. inside another engine's
        # capture, and the graph may still be executing): they are parked and destroyed at the next plan build, after a
        # device synchronisation
        try:
            for p in self._plans.values():
                if p.graph is not None:
                    _DEAD_GRAPHS.append(p.graph)
                    p.graph = None
        except Exception:
            pass
