"""One optimisation step of T-DEED on the HIP kernels: train-mode forward, loss, backward and fused AdamW, the
counterpart of the training branch of `TDEEDModel.epoch` (/root/reference/model/model.py:193-263) and
`BaseRGBModel.step` / `get_optimizer` (model/modules.py:37-39, 390-404) with the LR schedule of
train_tdeed.py:79-87.

    uint8 clip (B,T,3,H,W) --crop/flip/standardise + stem conv--> BN(batch stats)+ReLU --> 13/14 bottlenecks
    (trunk_train.py; gate-shift on s3/s4) --> avg-pool + temp_enc --> SGP encoder-decoder + heads + loss
    (temporal_train.py) --> the same chain backwards --> gradients in ONE flat fp32 buffer --> AdamW in one launch.

Every numeric step is a HIP kernel behind the C ABI and is parity-tested against torch autograd on the CPU oracle
(tests/test_gpu_bwd.py).  `build_graph/step_graph` capture weight re-packing + forward + loss + backward + gradient
write-out into one HIP graph (AdamW stays outside: lr and the step count change every step).  The step is correct but only
lightly tuned: DESIGN.md section 8 has the per-kernel breakdown.  Both gate-shift variants train: `_gsf` (every shipped
config) and the optional `_gsm` (impl/gsm.py; the same backward kernels without the fusion-conv path)."""
import os

import torch

from . import ops, ops_bwd as B_, _lib
from .streams import new_stream
from .optim import FlatParams, FusedAdamW, warmup_cosine_lr, is_late_bucket_key
from .regnet_spec import regnet_spec
from .temporal_train import TemporalStack
from .trunk_train import BottleneckTrain, StemTrain, BN_EPS

STEM_MFMA = True
STEM_BN_FUSED = True


def kd_settings(kd, teacher=None):
    """The distillation settings of a step in their canonical form -- dict(ld_t, displ_col_t, alpha, temperature,
    displ_weight), what a graph handle records and compares -- from the caller's dict (None: no distillation).  ld_t comes
    from the dict or from the teacher head tensor; a 'teacher' entry is dropped."""
    if kd is None:
        if teacher is not None:
            raise ValueError("a teacher head needs its kd settings")
        return None
    unknown = set(kd) - {"teacher", "ld_t", "displ_col_t", "alpha", "temperature", "displ_weight"}
    if unknown:
        raise ValueError(f"kd: unknown settings {sorted(unknown)}")
    ld_t = kd.get("ld_t")
    if teacher is not None:
        if ld_t is not None and int(ld_t) != teacher.shape[-1]:
            raise ValueError(f"kd: ld_t {ld_t} but the teacher head has {teacher.shape[-1]} columns")
        ld_t = teacher.shape[-1]
    if ld_t is None:
        raise ValueError("kd: ld_t (the teacher head's row stride) is missing")
    alpha, tau, beta = ops.check_kd(kd.get("alpha", 0.5), kd.get("temperature", 2.0), kd.get("displ_weight", 0.0))
    return dict(ld_t=int(ld_t), displ_col_t=int(kd.get("displ_col_t", -1)), alpha=alpha, temperature=tau, displ_weight=beta)


def loss_settings(loss, K1=None):
    """The loss options of a step in their canonical form -- dict(label_smoothing, focal_gamma as floats, class_weights as a
    tuple of K1 floats or None), what a graph handle records and compares -- from the caller's dict (None: the plain
    loss).  Ranges and shapes: ops.check_loss_options."""
    if loss is None:
        return None
    unknown = set(loss) - {"label_smoothing", "focal_gamma", "class_weights"}
    if unknown:
        raise ValueError(f"loss: unknown settings {sorted(unknown)}")
    eps, gamma, cw = ops.check_loss_options(loss.get("label_smoothing", 0.0), loss.get("focal_gamma", 0.0),
                                            loss.get("class_weights"), K1)
    return dict(label_smoothing=eps, focal_gamma=gamma, class_weights=cw)


class TrainEngine:
    """state: name -> tensor (reference state_dict names; fp32 parameters, BN buffers).  The parameters are moved into one
    flat buffer (`FlatParams`), `state` afterwards holds views into it."""

    def __init__(self, cfg, state, act_dtype=torch.bfloat16, device="cuda", lr=1e-3, weight_decay=0.01):
        self.cfg, self.dt, self.device = dict(cfg), act_dtype, device
        for k in list(state):                                    # in place: the caller's dict ends up holding the views
            v = state[k]
            state[k] = (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)).to(device)
        self.state = state
        self.params = FlatParams(self.state, device)
        self.opt = FusedAdamW(self.params, lr, weight_decay=weight_decay)
        self.spec = regnet_spec(cfg["feature_arch"])
        self.T = cfg["clip_len"]
        sd = self.state
        self.blocks = [BottleneckTrain(sd, "_features." + b.name, b, act_dtype, clip_len=self.T) for b in self.spec.blocks]
        self.temporal = TemporalStack(sd, self.cfg, act_dtype)
        self.stem = StemTrain(sd, act_dtype)
        self.one32 = torch.ones(32, device=device)
        self.zero32 = torch.zeros(32, device=device)
        self.sched_step = 0
        self.reducer = None                                      # dist.GradReducer of a data-parallel job (set_reducer)
        self.frozen = frozenset()                                # set_groups(): names of the frozen parameters
        self.stages = None                                       # ... and the backward stages that run (None: all)
        # set_groups(frozen_stats='eval'): the stages from the stem on that run in eval mode on the inference kernels
        # (optim.eval_prefix), their launches (prefix.EvalPrefix) and the generation of its packed weights
        self.frozen_stats, self.eval_prefix, self.prefix, self.prefix_gen = "batch", (), None, 0
        self._nbt_inc = None                                     # step-counter increments with zeros at the prefix stages
        self._static_frames = None                               # build_graph(): the captured step's frame buffer
        # set_ema(): the shadow of the BatchNorm running statistics, its layout and its row table (ops.ema_tensor_table)
        self.ema_stats, self.ema_stat_index, self._ema_rows = None, None, None
        # kernel-layout weight copies through recorded index tables (TDEED_REPACK_GATHER=0: every module re-packs itself
        # with its own casts / transposes / gathers, ~350 small launches per step)
        import os
        self.pack = None
        self.pack_gather = os.environ.get("TDEED_REPACK_GATHER", "1") == "1"
        if self.pack_gather:
            self.repack()

    # ------------------------------------------------------------------ data parallel
    def grad_buckets(self):
        """Element ranges of the flat gradient buffer in the order the backward completes them: [temporal stack + heads]
        (everything from the first `_temp_fine.` tensor to the end of the buffer), then [temp_enc + trunk]."""
        idx = self.params.index
        first = min(o for k, (o, n) in idx.items() if is_late_bucket_key(k))
        stray = [k for k, (o, n) in idx.items() if (o >= first) != is_late_bucket_key(k)]
        if stray:
            # the buckets are element RANGES reduced as soon as backward_heads / backward_trunk have written them: a state
            # dict whose trunk tensors sit behind the temporal stack would have them reduced before they are written
            raise RuntimeError(f"state_dict order: trunk and temporal-stack tensors interleave in the flat buffer ({stray[:3]} ...)")
        return [(first, self.params.numel), (0, first)]

    def _check_bucket_keys(self, keys, role):
        """Every gradient the write-out of bucket `role` carries must lie inside that bucket's element range (the range is
        all-reduced right after the write-out)."""
        bad = [k for k in keys if is_late_bucket_key(k) != (role == 0)]
        if bad:
            raise RuntimeError(f"gradient of {bad[0]} was produced by the {'temporal' if role == 0 else 'trunk'} backward "
                               f"but belongs to the other gradient bucket")

    def set_reducer(self, reducer="auto"):
        """Attach the gradient reducer of a data-parallel job (one process per GPU).  "auto": a dist.GradReducer over this
        engine's flat gradient buffer when torch.distributed is initialised with more than one rank, else none."""
        from . import dist as tdist
        import torch.distributed as td
        if reducer == "auto":
            reducer = None
            if td.is_available() and td.is_initialized() and td.get_world_size() > 1:
                reducer = tdist.GradReducer(self.params.grad, self.grad_buckets(), device=torch.device(self.device))
        self.reducer = reducer
        self._mark_frozen_buckets()
        return reducer

    # ------------------------------------------------------------------ weight EMA
    def set_ema(self, decay, warmup=False):
        """Exponential moving average of the model (`FusedAdamW.set_ema`; None switches it off and drops the buffers).  The
        parameters' shadow lives in the optimizer and moves inside the AdamW launch.  This engine owns the shadow of the
        BatchNorm running statistics -- every running_mean / running_var of `self.state` in state-dict order, packed back to
        back, a copy of the live values now -- and its row table, written and uploaded once; one `ops.ema_tensors` launch
        right behind the AdamW launch moves it with the same n, decay and guard record, so a skipped step leaves both shadows
        untouched.  num_batches_tracked is not averaged.
        Data parallel: the ranks hold the same parameters and the same scalars (t, skipped, ema_step0, decay), so their
        parameter shadows agree bit for bit without a collective; the statistics shadows are per rank, as the live running
        statistics are.
        A non-finite FORWARD still reaches the live running statistics, as in the reference, and from there the averaged ones
        at the next applied step."""
        from .optim import ema_stat_layout
        self.opt.set_ema(decay, warmup)
        if decay is None:
            self.ema_stats, self.ema_stat_index, self._ema_rows = None, None, None
            self.opt.ema_hook = self.opt.ema_stats_get = self.opt.ema_stats_set = None
            return
        if self.ema_stats is None:
            index, total = ema_stat_layout(self.state)
            srcs = [self.state[k].reshape(-1) for k in index]     # (views: the rows point at the live tensors)
            if any(s.data_ptr() != self.state[k].data_ptr() for s, k in zip(srcs, index)):
                raise RuntimeError("a running statistic of the state is not contiguous")
            self._ema_rows = ops.ema_tensor_table(srcs, [o for o, _ in index.values()])
            assert self._ema_rows.total == total
            self.ema_stats = torch.cat([s.detach() for s in srcs])
            self.ema_stat_index = index
            self.opt.ema_hook = self._ema_stats_step
            self.opt.ema_stats_get = lambda: self.ema_stats
            self.opt.ema_stats_set = lambda v: self.ema_stats.copy_(v)

    def _ema_stats_step(self, opt):
        ops.ema_tensors(self._ema_rows, self.ema_stats, opt.t, opt.ema_decay, opt.ema_warmup, opt.ema_step0, opt.guard,
                        opt.skip_nonfinite)

    def ema_state(self):
        """The averaged model: an ordered mapping with the model's own keys in the model's own order -- parameters as views
        of the optimizer's shadow through `params.index`, running statistics as views of the statistics shadow, the step
        counters live.  Views, not copies: `ForwardEngine(cfg, ema_state(), ...)` packs its own."""
        from .optim import ema_state_map
        if self.opt.ema is None:
            raise RuntimeError("ema_state(): the optimizer has no EMA (get_optimizer({'ema_decay': ...}) / set_ema())")
        return ema_state_map(self.state, self.params.index, self.opt.ema, self.ema_stat_index, self.ema_stats)

    # ------------------------------------------------------------------ parameter groups, frozen tensors
    def set_groups(self, groups, frozen_stats="batch"):
        """Parameter groups of the optimizer (`optim.check_groups`; None: none).  A frozen tensor keeps its bits: its
        gradient is not written into the flat buffer (its range there stays zero) and not reduced, and the backward stops
        after the earliest stage that still owns a trainable parameter (`optim.freeze_plan`).
        frozen_stats 'batch' (default): the forward is untouched -- a frozen BatchNorm normalises with batch statistics and
        moves its running statistics.  'eval': the eval prefix (`optim.eval_prefix`: the stem and the bottlenecks behind it,
        in order, as long as every parameter is frozen; `self.eval_prefix`) runs as torch's .eval() + requires_grad_(False)
        would: running statistics in the BatchNorms (2d and the gate-shift modules' 3d), buffers and step counters keep their
        bits, nothing is kept for a backward; its launches are those of the inference engine (prefix.EvalPrefix).  A frozen
        stage BEHIND the first trainable one keeps batch statistics (the gradient passes through it).  ValueError when the
        prefix is empty.
        A captured step belongs to the (freeze set, eval prefix) it was captured under: the handle make_step() kept is
        dropped."""
        from .optim import freeze_plan, frozen_keys, checked_eval_prefix
        frozen = frozen_keys(self.params.index, groups)          # (checks the groups: nothing is changed on an error)
        stages = freeze_plan(self.spec, frozen, self.params.index) if frozen else None
        if stages is not None and not stages:
            raise ValueError("the groups freeze every parameter: nothing left to train")
        pre = checked_eval_prefix(self.spec, frozen, self.params.index, frozen_stats)
        self.opt.set_groups(groups)
        self.frozen, self.stages = frozen, stages
        self.last_graph = None
        self._mark_frozen_buckets()
        changed = pre != self.eval_prefix
        self.frozen_stats, self.eval_prefix = frozen_stats, pre
        if changed or (pre and self.prefix is None):
            self.reload_prefix()

    def reload_prefix(self):
        """(Re)build the eval prefix's packed weights from the state's tensors: when the prefix is set or changes, and after
        load() / load_state_dict().  NOT part of repack(): an optimizer step leaves frozen tensors alone.  Graphs captured
        over the old copies are stale from here on (step_graph raises, make_step rebuilds)."""
        if not self.eval_prefix and self.prefix is None:
            return                                               # no prefix before, none now: nothing to rebuild or invalidate
        self.prefix_gen += 1
        self.last_graph = None
        if not self.eval_prefix:
            self.prefix, self._nbt_inc = None, None
            return
        from .optim import stage_of
        from .prefix import EvalPrefix
        self.prefix = EvalPrefix(self.cfg, self.state, len(self.eval_prefix) - 1, self.dt, self.device)
        nbt = [k for k in self.state if k.endswith("num_batches_tracked")]
        inc = [0 if (k.startswith("_features.") and stage_of(k) in self.eval_prefix) else 1 for k in nbt]
        self._nbt_inc = torch.tensor(inc or [1], dtype=torch.int64, device=self.device)

    def _mark_frozen_buckets(self):
        """A gradient bucket whose tensors are all frozen is not reduced (its range is zeros on every rank)."""
        if self.reducer is None or not hasattr(self.reducer, "set_frozen"):
            return
        idx = self.params.index
        self.reducer.set_frozen([all(k in self.frozen for k, (o, n) in idx.items() if lo <= o < hi)
                                 for lo, hi in self.reducer.buckets])

    def _runs(self, stage):
        return self.stages is None or stage in self.stages

    def _trainable(self, grads):
        """`grads` without the frozen tensors (their weight gradients were computed by launches that also produce what the
        stages behind them need; they are dropped here, never written out)."""
        return {k: g for k, g in grads.items() if k not in self.frozen} if self.frozen else grads

    # ------------------------------------------------------------------ forward + backward
    def _frame_flip(self, flip, Bn, T):
        """bool (all frames) or per-clip flags (B,) -> what ops.stem takes: bool or per-frame uint8 flags (B*T,)."""
        if isinstance(flip, torch.Tensor):
            if flip.numel() != Bn:
                raise ValueError(f"flip: one flag per clip expected ({flip.numel()} vs {Bn})")
            return flip.to(self.device).to(torch.uint8).repeat_interleave(T).contiguous()
        return bool(flip)

    def forward_train(self, frames_u8, crop=None, flip=False, drop_masks=None):
        """Train-mode forward (`Impl.forward` under .train(): batch-statistics BatchNorm with running-stat updates, dropout
        through the given keep-masks, model.py:105-149).  frames (B,T,3,H,W) uint8 (or fp32 0..255) on the device;
        crop = (top, left, h, w) shared by all clips (model.py:115); flip: bool or per-clip flags (B,) (model.py:83).
        Returns (head_out (B*T, n_out) fp32, ctx for backward_train)."""
        sd, dt = self.state, self.dt
        _lib.SCOPE = "stem.fwd"
        Bn, T = frames_u8.shape[:2]
        fr = frames_u8.reshape(Bn * T, *frames_u8.shape[2:])
        fl = self._frame_flip(flip, Bn, T)
        H_, W_ = fr.shape[-2:]
        chw = (crop[2], crop[3]) if crop is not None else (H_, W_)
        k0 = len(self.eval_prefix) - 1                          # blocks [0, k0) belong to the eval prefix (-1: none)
        z0 = y0 = bn0 = pmap = None
        if k0 >= 0:
            # the frozen prefix in eval mode: block k0's input map from the inference kernels, on this stream.  The map is a
            # buffer of the prefix's plan: (plan, run count) goes into the ctx so that the backward can tell a map that a
            # later forward of the same geometry has overwritten
            x = self.prefix.run(fr.contiguous(), crop, fl, static=frames_u8 is self._static_frames)
            pmap = (x, self.prefix.last_plan, self.prefix.last_plan.runs)
        elif self.stem.wf is not None and STEM_MFMA and ops.stem_mfma_parts(*chw) > 0:
            # bf16: conv on the MFMA pipe, BatchNorm statistics from its epilogue (no second pass over the 112^2 map)
            z0, cp = ops.stem_mfma(fr, self.stem.wf, crop=crop, flip=fl)
            cpf = cp.view(-1)
            y0, bn0 = B_.bn_finalize_apply(z0, cpf, cpf[32:], 64, cp.shape[0], sd["_features.stem.bn.weight"],
                                           sd["_features.stem.bn.bias"], BN_EPS, 0.1, sd["_features.stem.bn.running_mean"],
                                           sd["_features.stem.bn.running_var"], relu=True)
        else:
            z0 = ops.stem(fr, sd["_features.stem.conv.weight"], self.one32, self.zero32, dt, crop=crop, flip=fl, relu=False)
            y0, bn0 = B_.bn_train(z0, sd["_features.stem.bn.weight"], sd["_features.stem.bn.bias"], BN_EPS, 0.1,
                                  sd["_features.stem.bn.running_mean"], sd["_features.stem.bn.running_var"], relu=True)
        if k0 < 0:
            x = y0
        xs = None
        for i, blk in enumerate(self.blocks):
            if i < k0:
                continue
            _lib.SCOPE = blk.blk.name + ".fwd"
            nxt = self.blocks[i + 1] if i + 1 < len(self.blocks) else None
            x = blk.forward(x, xs=xs, next_fold=(nxt.blk.gsf_fold if nxt is not None and nxt.gs is not None else 0))
            xs = blk.ctx.out_slice
        _lib.SCOPE = "temporal.fwd"
        hw = x.shape[1] * x.shape[2]
        feat = ops.avgpool_posenc(x, Bn, T, sd["temp_enc"])
        head_out, tctx = self.temporal.forward_heads(feat, drop_masks)
        # BatchNorm step counters (nn.BatchNorm.num_batches_tracked); those of the eval prefix keep their bits
        self.params.nbt += 1 if self._nbt_inc is None else self._nbt_inc
        from types import SimpleNamespace
        return head_out, SimpleNamespace(fr=fr, crop=crop, flip=fl, z0=z0, y0=y0, bn0=bn0, x_shape=x.shape, hw=hw, tctx=tctx,
                                         B=Bn, T=T, pmap=pmap)

    def backward_train(self, ctx, dhead):
        """Backward of forward_train from d(loss)/d(head_out): returns grads dict name -> fp32 tensor."""
        grads = {}
        _lib.SCOPE = "temporal.bwd"
        d_feat = self.temporal.backward_heads(ctx.tctx, dhead, grads)
        grads.update(self.backward_trunk(ctx, d_feat))
        return {k: B_.materialize(g) for k, g in self._trainable(grads).items()}

    def backward_trunk(self, ctx, d_feat):
        """Backward of avg-pool + positional encoding, the bottlenecks and the stem from d(loss)/d(features).  With frozen
        tensors (set_groups) it ends after the last stage of `self.stages`; the stages behind are not launched."""
        sd = self.state
        grads = {}
        if not self._runs("temp_enc"):
            return grads
        dx, d_enc = B_.avgpool_posenc_bwd(d_feat, ctx.hw)
        grads["temp_enc"] = d_enc
        dx = dx.view(ctx.x_shape)
        from .trunk_train import ZMASK, SINK
        nb = len(self.blocks)
        k0 = len(self.eval_prefix) - 1
        pmap = getattr(ctx, "pmap", None)
        if (pmap is None) != (k0 < 0):
            raise RuntimeError("the eval prefix changed between this forward and its backward")
        if 0 <= k0 < nb and pmap[1].runs != pmap[2]:
            # block k0 re-reads its input, and that map is the prefix plan's buffer, not an allocation of this forward
            raise RuntimeError("another forward of the same geometry has overwritten the eval prefix's map since this one: "
                               "with frozen_stats='eval', run each backward before the next forward")
        # a block of the eval prefix has no train-mode forward and so no sink of its own
        sinks = [(blk.make_sink() if i >= k0 else None) for i, blk in enumerate(self.blocks[:-1])] if SINK else []
        stem_sink = B_.GradSink(ctx.y0, ctx.z0, ctx.bn0[0]) if (SINK and k0 < 0) else None
        if SINK and 0 <= k0 < nb:
            # The first block behind the prefix keeps the backward form it has under 'batch' (the fused launches that mask and
            # sum for the stage in front): it fills a stand-in sink over its own input map -- the true ReLU mask, the map as
            # "z" with mean 0 -- of the geometry of that stage's real sink.  Nobody reads the sums or the input gradient.
            xk = pmap[0]
            zero = torch.zeros(xk.shape[-1], dtype=torch.float32, device=xk.device)
            ds = k0 > 0 and self.blocks[k0 - 1].blk.has_downsample
            stand = B_.GradSink(xk, xk, zero, zd=(xk if ds else None), mean_d=(zero if ds else None))
            if k0 > 0:
                sinks[k0 - 1] = stand
            else:
                stem_sink = stand
        for i in reversed(range(nb)):
            blk = self.blocks[i]
            if not self._runs(blk.blk.name):
                return grads
            _lib.SCOPE = blk.blk.name + ".bwd"
            if SINK:
                # block i's input gradient is produced masked by the ReLU in front of it, with the column sums the BatchNorm
                # backward of block i-1 (or of the stem) needs
                dx = blk.backward(dx, grads, sink_in=(sinks[i] if i + 1 < nb else None),
                                  sink_out=(sinks[i - 1] if i > 0 else stem_sink))
            else:
                dx = blk.backward(dx, grads)
        if not self._runs("stem"):
            return grads
        _lib.SCOPE = "stem.bwd"
        wbn = sd["_features.stem.bn.weight"]
        fr4 = ctx.fr.view(-1, *ctx.fr.shape[-3:])
        if SINK and STEM_BN_FUSED and B_.stem_wgrad_bn_fits(fr4, ctx.crop, dx.dtype):
            # the stem BatchNorm's backward is applied inside the weight-gradient launch while it stages the gradient rows:
            # dz0 (the largest map of the step) is neither written nor read back
            sums = B_.bn_sums_from_sink(ctx.z0, dx, ctx.bn0, wbn, stem_sink, q=1)
            grads["_features.stem.bn.weight"], grads["_features.stem.bn.bias"] = sums[1], sums[0]
            grads["_features.stem.conv.weight"] = B_.stem_wgrad(ctx.fr, dx, crop=ctx.crop, flip=ctx.flip,
                                                                bn=(ctx.z0, sums, ctx.bn0[0], ctx.bn0[1], wbn))
            return grads
        if SINK:
            dz0, dw, db = B_.bn_bwd_from_parts(ctx.z0, dx, ctx.bn0, wbn, stem_sink, q=1)
        else:
            dz0, _, dw, db = B_.bn_train_bwd(ctx.z0, dx, None if ZMASK else ctx.y0, ctx.bn0, wbn, relu=True)
        grads["_features.stem.bn.weight"], grads["_features.stem.bn.bias"] = dw, db
        grads["_features.stem.conv.weight"] = B_.stem_wgrad(ctx.fr, dz0, crop=ctx.crop, flip=ctx.flip)
        return grads

    def loss_and_grads(self, frames_u8, label, labelD=None, soft=None, crop=None, flip=False, drop_masks=None,
                       fg_weight=5.0, dataset=None):
        """frames (B,T,3,H,W) uint8 on the device; label int64 (B,T) or None with soft (B,T,K+1); labelD float (B,T).
        crop = (top, left, h, w) (the one random crop the reference shares across B and T, model.py:115) or None.
        Returns (loss[3] = total, ce, mse ; grads dict name -> fp32 tensor)."""
        head_out, ctx = self.forward_train(frames_u8, crop, flip, drop_masks)
        loss, dhead = self.temporal.loss_fwd_bwd(
            head_out, ctx.B, ctx.T, None if label is None else label.reshape(-1).contiguous(),
            labelD=None if labelD is None else labelD.reshape(-1).float().contiguous(),
            soft=None if soft is None else soft.reshape(-1, soft.shape[-1]).contiguous(), fg_weight=fg_weight,
            dataset=dataset)
        return loss, self.backward_train(ctx, dhead)

    def repack(self):
        """Refresh the kernel-layout copies of the weights (after an optimizer step or a load_state_dict): one gather
        launch per dtype through the recorded index tables (repack.PackPlan)."""
        if not self.pack_gather:
            for blk in self.blocks:
                blk.repack()
            self.temporal.repack()
            self.stem.repack()
        elif self.pack is None:
            from .repack import PackPlan
            self.pack = PackPlan(self.params, self.device).build(list(self.blocks) + [self.temporal, self.stem])
        else:
            self.pack.run()
            for blk in self.blocks:          # the gather refreshed every block's packed copies in place (blk.repack() bumps
                blk.pack_gen = getattr(blk, "pack_gen", 0) + 1   # its own counter): a backward of an older forward must not recompute from them

    # ------------------------------------------------------------------ one optimiser step
    def write_grads(self, grads, scale=1.0, first=True, partial=False, role=0):
        """Gradient write-out into the flat buffer (times `scale`; overwriting when `first`, adding otherwise:
        `acc_grad_iter` of the reference's step()): multi-tensor copies, a handful of launches instead of one per tensor."""
        grads = self._trainable(grads)
        if not partial:
            missing = set(self.params.index) - self.frozen - set(grads)
            if missing:
                raise RuntimeError(f"no gradient produced for {sorted(missing)[:4]} ...")
        keys = list(grads)
        if not keys and self.frozen:
            return                                               # every tensor of this write-out is frozen
        srcs = [grads[k] for k in keys]                          # tensors (contiguous or column slices) or LazyFold partials
        for k, g in zip(keys, srcs):
            if g.numel() != self.params.index[k][1] or g.dtype != torch.float32:
                raise RuntimeError(f"gradient of {k}: {tuple(g.shape)} {g.dtype} does not match the parameter")
        # one launch for all tensors (a per-tensor device copy is ~3 us and a step has 431 of them)
        if not hasattr(self, "_grad_tabs"):
            self._grad_tabs = B_.PinnedTables(max_entries=len(self.params.index) + 8)
        B_.multi_copy(srcs, [self.params.index[k][0] for k in keys], self.params.grad, scale=scale, accumulate=not first,
                      tables=self._grad_tabs, role=role)

    def accumulate(self, frames_u8, label, labelD=None, soft=None, crop=None, flip=False, drop_masks=None, scale=1.0,
                   first=True, dataset=None, fg_weight=5.0, reduce=False, teacher=None, kd=None, loss=None):
        """forward + backward of one (micro-)batch; its gradients (times `scale`) go into the flat gradient buffer.
        reduce (data parallel, last micro-batch of a step): each bucket's all-reduce is enqueued as soon as the backward has
        produced it -- the temporal stack + heads travel over xGMI while the trunk backward runs."""
        head_out, ctx = self.forward_train(frames_u8, crop, flip, drop_masks)
        loss, dhead = self.temporal.loss_fwd_bwd(
            head_out, ctx.B, ctx.T, None if label is None else label.reshape(-1).contiguous(),
            labelD=None if labelD is None else labelD.reshape(-1).float().contiguous(),
            soft=None if soft is None else soft.reshape(-1, soft.shape[-1]).contiguous(), fg_weight=fg_weight,
            dataset=dataset, teacher=teacher, kd=kd, loss=loss)
        self.backward_and_write(ctx, dhead, scale, first, reduce)
        return loss

    def backward_and_write(self, ctx, dhead, scale=1.0, first=True, reduce=False):
        """Backward of forward_train from d(loss)/d(head_out) with the gradients (times `scale`) written into the flat
        buffer bucket by bucket; with `reduce` each bucket's all-reduce starts as soon as it is complete."""
        red = self.reducer if reduce else None
        g_t = {}
        # weight gradients stay in their per-workgroup partials until the bucket's write-out launch folds them
        lazy = os.environ.get("TDEED_LAZY_WGRAD", "1") == "1"
        B_.LAZY_WGRAD = lazy
        _lib.SCOPE = "temporal.bwd"
        try:
            d_feat = self.temporal.backward_heads(ctx.tctx, dhead, g_t)
        finally:
            B_.LAZY_WGRAD = False
        self._check_bucket_keys(g_t, 0)
        _lib.SCOPE = "write_grads"
        self.write_grads(g_t, scale, first, partial=True, role=0)
        if red is not None:
            red.reduce_bucket(0)
        B_.LAZY_WGRAD = lazy
        try:
            g_b = self.backward_trunk(ctx, d_feat)
        finally:
            B_.LAZY_WGRAD = False
        missing = set(self.params.index) - self.frozen - set(g_t) - set(g_b)
        if missing:
            raise RuntimeError(f"no gradient produced for {sorted(missing)[:4]} ...")
        self._check_bucket_keys(g_b, 1)
        _lib.SCOPE = "write_grads"
        self.write_grads(g_b, scale, first, partial=True, role=1)
        if red is not None:
            red.reduce_bucket(1)
        self._reduced = red is not None                          # apply() checks it (scale only what was reduced)

    def apply(self, lr=None, lr_factor=1.0, all_reduce=None):
        """AdamW on the accumulated gradients (one launch), then refresh the kernels' views of the weights.  With a reducer
        attached the current stream first waits for the bucket all-reduces and the 1/world of the mean rides on AdamW's
        grad_scale; `all_reduce` is the older blocking form (callable(flat_grad))."""
        gs = 1.0
        _lib.SCOPE = "optim"
        if all_reduce is not None:
            all_reduce(self.params.grad)
        elif self.reducer is not None:
            if not getattr(self, "_reduced", False):
                # the step's gradients were accumulated without `reduce=True` (e.g. accumulate() called directly): sum them
                # over the ranks now, blocking on nothing but the device -- never scale un-reduced gradients by 1/world
                self.reducer.reduce_all()
            self.reducer.join()
            gs = self.reducer.scale
        self._reduced = False
        if lr is not None:
            self.opt.lr = lr
        self.opt.step(lr_factor=lr_factor, grad_scale=gs)
        self.repack()

    def step(self, frames_u8, label, labelD=None, soft=None, crop=None, flip=False, drop_masks=None, lr_factor=1.0,
             all_reduce=None, teacher=None, kd=None, loss=None):
        """forward + backward + (data parallel: bucketed gradient all-reduce overlapped with the backward) + AdamW.
        all_reduce: the older blocking form, a callable(flat_grad) (dist.all_reduce_mean_).  Returns [total, ce, mse]
        (with a teacher head and its kd settings, or with loss options -- `loss`, see loss_settings --,
        TemporalTrain.loss_fwd_bwd: [total, ce, mse, kd, kd_displ])."""
        out = self.accumulate(frames_u8, label, labelD, soft, crop, flip, drop_masks,
                              reduce=self.reducer is not None and all_reduce is None, teacher=teacher, kd=kd,
                              loss=loss_settings(loss, self.cfg["num_classes"] + 1))
        self.apply(lr_factor=lr_factor, all_reduce=all_reduce)
        return out

    # ------------------------------------------------------------------ the step as one HIP graph
    def build_graph(self, *args, **kw):
        """`_build_graph` with the engine's note of the static frame buffer cleared whatever happens, and the prefix plans
        built over that buffer dropped when the capture fails (on success the handle owns them)."""
        try:
            return self._build_graph(*args, **kw)
        except BaseException:
            if self.prefix is not None:
                self.prefix.take_static()
            raise
        finally:
            self._static_frames = None

    def _build_graph(self, B, H, W, frames_dtype=torch.uint8, with_labelD=None, soft=False, fg_weight=5.0, kd=None,
                     loss=None):
        """Capture weight re-packing + train-mode forward + loss + backward + gradient write-out for one batch geometry
        into a HIP graph (the eager step is host-bound: ~1700 launches).  Inputs live in static buffers
        (`.frames/.label/.labelD/.soft/.masks` of the returned handle); the AdamW launch stays outside the graph because lr
        and the step count change every step.  torch's graph-private memory pool keeps every temporary of the step alive
        between replays.
        kd (opt-in distillation): dict(ld_t=, displ_col_t=, alpha=, temperature=, displ_weight=) -- the handle gets a static
        teacher head buffer `.teacher` (B*T, ld_t) that the captured loss launch reads; the teacher's own forward stays
        outside the graph (it is the inference engine's business), step_graph() copies its head in.
        loss (opt-in loss options): dict(label_smoothing=, focal_gamma=, class_weights=) -- the captured loss launch is
        ops.loss_opt with these settings (the class weight vector is uploaded by the eager warm-up, not inside the graph).
        Data parallel (default, `mode == "two"`): the step is captured as TWO graphs -- [re-pack, forward, loss, temporal
        backward, bucket 0 write-out] and [trunk backward, bucket 1 write-out] -- and bucket 0's all-reduce is launched
        between the two replays on the communicator's own stream, so it travels while the trunk backward runs.  With
        TDEED_DP_IN_GRAPH=1 and the C-ABI RCCL communicator the all-reduces are captured into ONE graph instead (its stream
        forks from / joins the captured stream through events, `mode == "one"`); if that capture fails the two-graph form is
        built."""
        import os
        import sys
        from types import SimpleNamespace
        dev, T = self.device, self.T
        K1 = self.cfg["num_classes"] + 1
        radi = self.cfg.get("radi_displacement", 0)
        if with_labelD is None:
            with_labelD = radi > 0
        C = self.spec.feat_dim
        h = SimpleNamespace(B=B)
        h.frames = torch.zeros((B, T, 3, H, W), dtype=frames_dtype, device=dev)
        self._static_frames = h.frames                           # (the eval prefix reads it in place)
        h.label = None if soft else torch.zeros((B, T), dtype=torch.int64, device=dev)
        h.soft = torch.full((B, T, K1), 1.0 / K1, dtype=torch.float32, device=dev) if soft else None
        h.labelD = torch.zeros((B, T), dtype=torch.float32, device=dev) if with_labelD else None
        h.masks = [torch.ones((B, T, C), dtype=self.dt, device=dev) for _ in range(2 if radi > 0 else 1)]
        h.kd = kd_settings(kd)
        h.loss_opt = loss_settings(loss, K1)
        h.teacher = None if h.kd is None else torch.zeros((B * T, h.kd["ld_t"]), dtype=torch.float32, device=dev)
        red = self.reducer
        # the gradient write-out launches read their record tables from pinned host memory at every replay: the graph gets
        # tables of its own (the eager steps' ring and other graphs of this engine must never rewrite them)
        eager_tabs = getattr(self, "_grad_tabs", None)
        self._grad_tabs = B_.PinnedTables(max_entries=len(self.params.index) + 8, depth=1)
        # default: two graphs with the collectives launched eagerly between them -- the same overlap, and nothing depends
        # on the collective library's behaviour under stream capture (which no single-GPU box can exercise);
        # TDEED_DP_IN_GRAPH=1 captures the RCCL calls into one graph instead
        want_in_graph = red is not None and red.capturable and os.environ.get("TDEED_DP_IN_GRAPH", "0") == "1"
        keep = {k: v.clone() for k, v in self.state.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}

        def restore():
            for k, v in keep.items():
                self.state[k].copy_(v)

        def part_a():
            head_out, ctx = self.forward_train(h.frames, None, False, h.masks)
            loss, dhead = self.temporal.loss_fwd_bwd(
                head_out, ctx.B, ctx.T, None if h.label is None else h.label.reshape(-1),
                labelD=None if h.labelD is None else h.labelD.reshape(-1),
                soft=None if h.soft is None else h.soft.reshape(-1, h.soft.shape[-1]), fg_weight=fg_weight,
                teacher=h.teacher, kd=h.kd, loss=h.loss_opt)
            g_t = {}
            B_.LAZY_WGRAD = os.environ.get("TDEED_LAZY_WGRAD", "1") == "1"
            try:
                d_feat = self.temporal.backward_heads(ctx.tctx, dhead, g_t)
            finally:
                B_.LAZY_WGRAD = False
            self._check_bucket_keys(g_t, 0)
            self.write_grads(g_t, 1.0, True, partial=True, role=0)
            return loss, ctx, d_feat, set(g_t)

        def part_b(ctx, d_feat, done):
            B_.LAZY_WGRAD = os.environ.get("TDEED_LAZY_WGRAD", "1") == "1"
            try:
                g_b = self.backward_trunk(ctx, d_feat)
            finally:
                B_.LAZY_WGRAD = False
            missing = set(self.params.index) - self.frozen - done - set(g_b)
            if missing:
                raise RuntimeError(f"no gradient produced for {sorted(missing)[:4]} ...")
            self._check_bucket_keys(g_b, 1)
            self.write_grads(g_b, 1.0, True, partial=True, role=1)

        def capture_one(in_graph):
            run = lambda: self.accumulate(h.frames, h.label, h.labelD, soft=h.soft, drop_masks=h.masks,      # noqa: E731
                                          reduce=in_graph, fg_weight=fg_weight, teacher=h.teacher, kd=h.kd,
                                          loss=h.loss_opt)
            # eager warm-up on a side stream (lazy kernel attributes / module loads must happen outside the capture); the
            # BatchNorm buffers it touches are restored afterwards
            side = new_stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.repack()
                run()
                if in_graph:
                    red.join()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            restore()
            g = torch.cuda.CUDAGraph()
            # thread-local capture: other threads (the RCCL watchdog of a data-parallel job) may keep calling the runtime
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                self.repack()
                h.loss = run()
                if in_graph:
                    red.join()
            h.graph, h.graph_b, h.mode, h.reduce_in_graph = g, None, "one", in_graph

        def capture_two():
            side = new_stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self.repack()
                _, ctx, d_feat, done = part_a()
                red.reduce_bucket(0)
                part_b(ctx, d_feat, done)
                red.reduce_bucket(1)
                red.join()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            restore()
            ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga, stream=side, capture_error_mode="thread_local"):
                self.repack()
                h.loss, ctx, d_feat, done = part_a()
            if self._runs("temp_enc"):
                with torch.cuda.graph(gb, pool=ga.pool(), stream=side, capture_error_mode="thread_local"):
                    part_b(ctx, d_feat, done)
            else:
                gb = None                                        # everything behind the temporal stack is frozen
            h.keep_ctx = (ctx, d_feat)                           # activations of the first half that the second half reads
            h.graph, h.graph_b, h.mode, h.reduce_in_graph = ga, gb, "two", False

        if red is None:
            capture_one(False)
        elif want_in_graph:
            try:
                capture_one(True)
            except Exception as e:                               # noqa: BLE001  (a runtime that cannot capture the collectives)
                print(f"[tdeed_amd] capturing the RCCL collectives failed ({type(e).__name__}: {e}); "
                      f"falling back to two graphs with the all-reduces launched between them", file=sys.stderr, flush=True)
                torch.cuda.synchronize()
                capture_two()
        else:
            capture_two()
        h.frozen = self.frozen                                   # the freeze set the backward was captured under
        h.prefix = (self.eval_prefix, self.prefix_gen)           # ... and the eval prefix (with its packed weights) of the forward
        # the prefix's launch list over h.frames and its buffers live as long as the handle
        h.prefix_plans = self.prefix.take_static() if self.prefix is not None else None
        h.keep = self._grad_tabs                                 # the gradient write-out tables the graph's copies read
        if eager_tabs is not None:
            self._grad_tabs = eager_tabs
        else:
            del self._grad_tabs
        self._reduced = False                                    # (the warm-up pass of an in-graph capture reduced)
        restore()                                                # capture does not execute, but stay explicit
        torch.cuda.synchronize()
        return h

    def step_graph(self, h, frames, label, labelD=None, soft=None, drop_masks=None, lr=None, lr_factor=1.0, all_reduce=None,
                   teacher=None, kd=None, loss=None):
        """One optimisation step through a captured graph: refresh the static inputs, replay, all-reduce (DP), AdamW.
        teacher / kd: the teacher's head (B*T, ld_t) fp32 and the distillation settings of this call; they must be the
        settings the handle was captured with (none for a handle built without kd).  loss: the loss options of this call,
        held to the handle's in the same way."""
        want = kd_settings(kd, teacher)
        if want != getattr(h, "kd", None):
            raise RuntimeError(f"this graph was captured under other distillation settings ({getattr(h, 'kd', None)}, the call "
                               f"has {want}): build_graph() again (make_step() does)")
        want_loss = loss_settings(loss, self.cfg["num_classes"] + 1)
        if want_loss != getattr(h, "loss_opt", None):
            raise RuntimeError(f"this graph was captured under other loss options ({getattr(h, 'loss_opt', None)}, the call has "
                               f"{want_loss}): build_graph() again (make_step() does)")
        if getattr(h, "frozen", frozenset()) != self.frozen:
            raise RuntimeError("this graph was captured under another set of frozen parameters: build_graph() again "
                               "(make_step() does) after set_groups()")
        if getattr(h, "prefix", ((), 0)) != (self.eval_prefix, self.prefix_gen):
            raise RuntimeError("this graph was captured under another eval prefix (frozen_stats) or over packed weights that "
                               "were rebuilt since: build_graph() again (make_step() does)")
        h.frames.copy_(frames, non_blocking=True)
        if h.label is not None:
            h.label.copy_(label, non_blocking=True)
        if h.soft is not None:
            h.soft.copy_(soft, non_blocking=True)
        if h.labelD is not None:
            h.labelD.copy_(labelD, non_blocking=True)
        if drop_masks is not None:
            for dst, src in zip(h.masks, drop_masks):
                dst.copy_(src, non_blocking=True)
        if want is not None:
            h.teacher.copy_(teacher, non_blocking=True)
        h.graph.replay()
        gs = 1.0
        if h.mode == "two":
            # bucket 0 (temporal stack + heads) is complete: its all-reduce travels while the trunk backward replays
            if all_reduce is None:
                self.reducer.reduce_bucket(0)
            if h.graph_b is not None:
                h.graph_b.replay()
            if all_reduce is None:
                self.reducer.reduce_bucket(1)
                self.reducer.join()
                gs = self.reducer.scale
        elif all_reduce is None and self.reducer is not None:
            if not h.reduce_in_graph:
                # a graph captured before set_reducer(): its gradients are local, reduce them here
                self.reducer.reduce_all()
                self.reducer.join()
            gs = self.reducer.scale                             # (else: reduced and joined inside the graph)
        if all_reduce is not None:
            all_reduce(self.params.grad)
        if lr is not None:
            self.opt.lr = lr
        self.opt.step(lr_factor=lr_factor, grad_scale=gs)       # the next replay starts with repack(): no refresh needed here
        return h.loss

    def make_step(self, B, H, W, frames, label, labelD=None, drop_masks=None, use_graph=True, world=1, all_reduce=None,
                  kd=None, loss=None):
        """A zero-argument callable running one optimisation step on the given (static) batch: through the captured HIP graph
        or eagerly; for world > 1 the flat gradient buffer is all-reduced (RCCL) before AdamW.  all_reduce: a callable
        (flat_grad) replacing the bucketed reduction (the bench's "no communication" arm passes a no-op).
        kd (opt-in distillation): dict(teacher=the teacher's head tensor (B*T, ld_t) fp32 -- read at every call, so the
        caller refreshes it in place --, displ_col_t=, alpha=, temperature=, displ_weight=).
        loss (opt-in loss options): dict(label_smoothing=, focal_gamma=, class_weights=)."""
        ar = all_reduce
        los = loss_settings(loss, self.cfg["num_classes"] + 1)
        tch = None if kd is None else kd["teacher"]
        kds = kd_settings(kd, tch)
        if world > 1 and self.reducer is None:
            self.set_reducer("auto")
        if not use_graph:
            return lambda: self.step(frames, label, labelD, drop_masks=drop_masks, all_reduce=ar, teacher=tch, kd=kds,
                                     loss=los)
        hnd = getattr(self, "last_graph", None)
        if (hnd is None or getattr(hnd, "geom", None) != (B, H, W) or getattr(hnd, "frozen", frozenset()) != self.frozen
                or getattr(hnd, "prefix", ((), 0)) != (self.eval_prefix, self.prefix_gen) or getattr(hnd, "kd", None) != kds
                or getattr(hnd, "loss_opt", None) != los):
            hnd = self.build_graph(B, H, W, kd=kds, loss=los)
            hnd.geom = (B, H, W)
        self.last_graph = hnd                                    # (tests / the bench line read .mode)
        return lambda: self.step_graph(hnd, frames, label, labelD, drop_masks=drop_masks, all_reduce=ar, teacher=tch, kd=kds,
                                       loss=los)

    def lr_factor(self, warmup_steps, cosine_steps):
        f = warmup_cosine_lr(self.sched_step, warmup_steps, cosine_steps)
        self.sched_step += 1
        return f


class HipAdamW(torch.optim.Optimizer):
    """What `TDEEDModel.get_optimizer` returns: a torch.optim.Optimizer whose single "parameter" is the flat fp32
    buffer and whose step() is the fused AdamW launch, so the reference's LR schedulers (LinearLR + CosineAnnealingLR
    chained, train_tdeed.py:79-87) drive it unchanged through param_groups[0]['lr'].
    skip_nonfinite / max_grad_norm (opt-in, `FusedAdamW.set_guard`): what the reference's GradScaler did for the optimizer
    -- a step whose gradients hold an inf or a NaN changes nothing -- and clipping by the global norm.  Both sit in
    param_groups[0] and are read at every step(), like lr.  An LR scheduler steps whether or not the update was skipped,
    as in the reference.
    groups (opt-in, `TrainEngine.set_groups`): per-tensor lr_scale / weight_decay / frozen by fnmatch patterns over the
    state_dict names.  There is still ONE torch param group: param_groups[0]['lr'] is what the schedulers move and what
    lr_scale multiplies at every step; the groups sit in param_groups[0]['groups'] and travel in state_dict().  Without the
    keyword the key is absent and nothing else differs.
    frozen_stats (opt-in, 'batch' | 'eval', `TrainEngine.set_groups`): 'eval' runs the frozen prefix of the trunk in eval mode.
    A keyword of the optimizer, not a key of a group; it sits in param_groups[0]['frozen_stats'] only when it is 'eval' and
    travels in state_dict() there.
    ema_decay / ema_warmup (opt-in, `TrainEngine.set_ema`): an exponential moving average of the weights, updated inside the
    AdamW launch, and of the BatchNorm running statistics, one launch behind it; `TDEEDModel.averaged()` scores with it.  The
    two keys sit in param_groups[0] only when given, are read at every step() and travel in state_dict(); the shadows
    travel under "fused"."""

    def __init__(self, engine: TrainEngine, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, skip_nonfinite=False,
                 max_grad_norm=None, groups=None, frozen_stats="batch", ema_decay=None, ema_warmup=False):
        self.engine = engine
        engine.opt.lr, engine.opt.betas, engine.opt.eps, engine.opt.wd = lr, betas, eps, weight_decay
        engine.opt.set_guard(skip_nonfinite, max_grad_norm)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, skip_nonfinite=skip_nonfinite,
                        max_grad_norm=max_grad_norm)
        from .optim import check_frozen_stats
        if check_frozen_stats(frozen_stats) == "eval" or groups:
            engine.set_groups(groups, frozen_stats=frozen_stats)
        if groups:
            defaults["groups"] = engine.opt.groups
        if frozen_stats == "eval":
            defaults["frozen_stats"] = "eval"                    # (absent under the default, like 'groups')
        if ema_decay is not None:
            engine.set_ema(ema_decay, ema_warmup)                # (ValueError on a bad pair: nothing was changed)
            defaults["ema_decay"], defaults["ema_warmup"] = engine.opt.ema_decay, engine.opt.ema_warmup
        elif ema_warmup is not False:
            raise ValueError("ema_warmup without ema_decay")
        super().__init__([engine.params.flat], defaults)

    def zero_grad(self, set_to_none=False):
        self.engine.opt.zero_grad()

    def set_groups(self, groups, frozen_stats="batch"):
        """Replace the parameter groups between steps (e.g. to unfreeze gradually); None returns to the plain launch.
        frozen_stats: 'batch' (default) or 'eval' (`TrainEngine.set_groups`); it sits in param_groups[0] only when 'eval'."""
        self.engine.set_groups(groups, frozen_stats=frozen_stats)
        if self.engine.opt.groups is None:
            self.param_groups[0].pop("groups", None)
        else:
            self.param_groups[0]["groups"] = self.engine.opt.groups
        if frozen_stats == "eval":
            self.param_groups[0]["frozen_stats"] = "eval"
        else:
            self.param_groups[0].pop("frozen_stats", None)

    @torch.no_grad()
    def step(self, closure=None, all_reduce=None):
        g = self.param_groups[0]
        o = self.engine.opt
        o.betas, o.eps, o.wd = g["betas"], g["eps"], g["weight_decay"]
        if (g["skip_nonfinite"], g["max_grad_norm"]) != (o.skip_nonfinite, o.max_grad_norm):
            o.set_guard(g["skip_nonfinite"], g["max_grad_norm"])
        if g.get("groups") != o.groups or g.get("frozen_stats", "batch") != self.engine.frozen_stats:
            # param_groups[0]['groups'] / ['frozen_stats'] was edited by hand
            self.engine.set_groups(g.get("groups"), frozen_stats=g.get("frozen_stats", "batch"))
        if (g.get("ema_decay"), g.get("ema_warmup", False)) != (o.ema_decay, o.ema_warmup):
            self.engine.set_ema(g.get("ema_decay"), g.get("ema_warmup", False))
        self.engine.apply(lr=g["lr"], all_reduce=all_reduce)

    def guard_stats(self):
        """`FusedAdamW.guard_stats`: dict(skipped, last_nonfinite, last_norm); one device synchronisation."""
        return self.engine.opt.guard_stats()

    def state_dict(self):
        """torch's state_dict (param_groups) with the fused optimizer's state next to it under "fused": exp_avg,
        exp_avg_sq, t, skipped and, with EMA on, ema, ema_stats, ema_decay, ema_warmup, ema_step0 (`FusedAdamW.state_dict`)."""
        sd = super().state_dict()
        sd["fused"] = self.engine.opt.state_dict()
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        fused = sd.pop("fused")
        super().load_state_dict(sd)
        g = self.param_groups[0]
        if g.get("groups") != self.engine.opt.groups or g.get("frozen_stats", "batch") != self.engine.frozen_stats:
            self.set_groups(g.get("groups"), frozen_stats=g.get("frozen_stats", "batch"))
        if g.get("ema_decay") is not None or self.engine.opt.ema is not None:
            self.engine.set_ema(g.get("ema_decay"), g.get("ema_warmup", False))   # (the shadows come back with `fused`)
        self.engine.opt.load_state_dict(fused)
