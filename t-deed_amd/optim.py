"""Optimizer-side pieces of the training path.

``FlatParams`` keeps every trainable tensor of the model in ONE flat fp32 device buffer (the tensors of the
state_dict become views into it), so the fused AdamW kernel updates all 431 tensors in a single launch and the
same buffer is what a data-parallel job all-reduces (``dist.all_reduce_mean_``).  ``FusedAdamW`` mirrors
``BaseRGBModel.get_optimizer`` (/root/reference/model/modules.py:37-39: torch.optim.AdamW with default betas / eps /
weight decay 0.01 on *all* parameters), ``warmup_cosine_lr`` mirrors ``get_lr_scheduler``
(/root/reference/train_tdeed.py:79-87: LinearLR(0.01 -> 1) chained with CosineAnnealingLR, both stepping from 0).
`trainer.TrainEngine` fills the gradient buffer (train-mode forward + backward kernels) and drives these classes.
"""
import math

import torch

from . import ops, state_layout


BUCKET_ALIGN = 64      # elements: bucket boundaries of the flat buffer are multiples of this (see FlatParams)


def is_late_bucket_key(key):
    """Tensors whose gradients the backward completes first (temporal stack + heads): bucket 0 of the data-parallel
    reduction (trainer.TrainEngine.grad_buckets)."""
    return key.startswith(("_temp_fine.", "_pred_"))


# ------------------------------------------------------------------------------------------ parameter groups
# get_optimizer({'groups': [...]}): each group is a dict with 'params' (fnmatch patterns over the state_dict names of
# parameters) and any of 'lr_scale', 'weight_decay', 'frozen'.  For every tensor the first group that matches wins; an
# unmatched tensor takes the optimizer's defaults.  Everything here is host arithmetic on names and offsets.
GROUP_KEYS = ("params", "lr_scale", "weight_decay", "frozen")


def check_groups(groups):
    """-> the groups as a tuple of (patterns, lr_scale, weight_decay | None, frozen); ValueError on anything else."""
    out = []
    for gi, g in enumerate(groups):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(f"group {gi}: a dict with 'params' expected, got {g!r}")
        unknown = sorted(set(g) - set(GROUP_KEYS))
        if unknown:
            raise ValueError(f"group {gi} {g['params']!r}: unknown key(s) {unknown}; a group takes {GROUP_KEYS}")
        pats = (g["params"],) if isinstance(g["params"], str) else tuple(g["params"])
        if not pats or not all(isinstance(p, str) for p in pats):
            raise ValueError(f"group {gi}: 'params' must be a tuple of fnmatch patterns, got {g['params']!r}")
        scale, wd, frozen = g.get("lr_scale", 1.0), g.get("weight_decay"), g.get("frozen", False)
        for name, val in (("lr_scale", scale), ("weight_decay", wd)):
            if val is None and name == "weight_decay":
                continue
            if isinstance(val, bool) or not isinstance(val, (int, float)) or not math.isfinite(val) or val < 0:
                raise ValueError(f"group {gi} {pats!r}: {name} must be a finite float >= 0, got {val!r}")
        if not isinstance(frozen, bool):
            raise ValueError(f"group {gi} {pats!r}: frozen must be a bool, got {frozen!r}")
        out.append((pats, float(scale), None if wd is None else float(wd), frozen))
    return tuple(out)


def match_groups(keys, groups):
    """-> {key: index of the first group one of whose patterns matches it} (unmatched keys are absent).  A group whose
    patterns match no parameter name at all is a ValueError naming it: a typo must not pass as 'defaults'."""
    return _match(keys, check_groups(groups))


def _match(keys, groups_n):
    import fnmatch
    keys = list(keys)
    owner = {}
    for gi, (pats, *_rest) in enumerate(groups_n):
        hit = [k for k in keys if any(fnmatch.fnmatchcase(k, p) for p in pats)]
        if not hit:
            raise ValueError(f"group {gi} {pats!r} matches no parameter")
        for k in hit:
            owner.setdefault(k, gi)
    return owner


def frozen_keys(keys, groups):
    """The parameter names a frozen group owns (first match wins)."""
    groups_n = check_groups(groups or ())
    return frozenset(k for k, gi in _match(keys, groups_n).items() if groups_n[gi][3])


def group_table(index, numel, groups, default_wd):
    """Runs (end_element, lr_scale, weight_decay, frozen) covering [0, numel) of a flat buffer with `index` = name ->
    (offset, size) (FlatParams.index / layout_only).  A tensor's padding belongs to the run in front of it (the padding
    behind tensor i sits in tensor i's run); adjacent tensors with equal settings merge into one run.  default_wd: what an
    unmatched tensor, or a group without 'weight_decay', decays with -- None stands for "the launch's" and is what
    FusedAdamW uploads, so that param_groups[0]['weight_decay'] keeps working without a new table."""
    groups_n = check_groups(groups or ())
    owner = _match(index, groups_n)
    order = sorted(index, key=lambda k: index[k][0])
    runs = []
    for i, k in enumerate(order):
        off, n = index[k]
        end = index[order[i + 1]][0] if i + 1 < len(order) else numel
        assert off % 4 == 0 and end % 4 == 0 and off + n <= end, (k, off, n, end)   # FlatParams._layout guarantees it
        if i == 0:
            assert off == 0, (k, off)
        gi = owner.get(k)
        scale, wd, frozen = (1.0, None, False) if gi is None else groups_n[gi][1:]
        cfg = (scale, default_wd if wd is None else wd, frozen)
        if frozen:
            cfg = (1.0, default_wd, True)                        # a frozen run's other settings do not matter: merge them
        if runs and runs[-1][1:] == cfg:
            runs[-1] = (end,) + cfg
        else:
            runs.append((end,) + cfg)
    if not runs:
        raise ValueError("group_table: no parameters")
    return runs


def groups_as_dicts(groups):
    """The groups with every option spelled out, as plain dicts: what param_groups[0]['groups'] and state_dict() hold."""
    out = []
    for pats, scale, wd, frozen in check_groups(groups):
        g = {"params": tuple(pats), "lr_scale": scale, "frozen": frozen}
        if wd is not None:
            g["weight_decay"] = wd
        out.append(g)
    return out


def backward_stages(spec):
    """The stages of the backward in the order it runs them: heads + temporal stack, avg-pool + temp_enc, the
    bottlenecks last to first, the stem."""
    return ["temporal", "temp_enc"] + [b.name for b in reversed(spec.blocks)] + ["stem"]


def stage_of(key):
    """The backward stage that produces the gradient of parameter `key`."""
    if is_late_bucket_key(key):
        return "temporal"
    if key == "temp_enc":
        return "temp_enc"
    if key.startswith("_features.stem."):
        return "stem"
    if key.startswith("_features."):
        return ".".join(key.split(".")[1:3])                     # "_features.s3.b2.conv1..." -> "s3.b2"
    raise ValueError(f"no backward stage owns parameter {key!r}")


def freeze_plan(spec, frozen, keys):
    """Which backward stages run when the parameters `frozen` (names) of `keys` (all parameter names) are frozen: the
    backward stops after the earliest stage of the model -- the last one it reaches -- that owns a trainable parameter.
    Every stage in front of that point runs, frozen or not, because the gradient has to pass through it; a stage behind it
    is not launched.  -> the list of stage names in backward order (empty when nothing is trainable)."""
    stages = backward_stages(spec)
    trainable = {stage_of(k) for k in keys if k not in frozen}
    unknown = trainable - set(stages)
    if unknown:
        raise ValueError(f"parameters of unknown stages {sorted(unknown)}")
    last = max((stages.index(s) for s in trainable), default=-1)
    return stages[:last + 1]


FROZEN_STATS = ("batch", "eval")


def check_frozen_stats(frozen_stats):
    """'batch' (frozen BatchNorms go on normalising with batch statistics and move their running statistics, the default) or
    'eval' (the frozen prefix of the trunk runs in eval mode, `eval_prefix`); ValueError on anything else."""
    if frozen_stats not in FROZEN_STATS:
        raise ValueError(f"frozen_stats must be one of {FROZEN_STATS}, got {frozen_stats!r}")
    return frozen_stats


def forward_stages(spec):
    """The stages of the trunk's forward in the order it runs them: the stem, then the bottlenecks."""
    return ["stem"] + [b.name for b in spec.blocks]


def eval_prefix(spec, frozen, keys):
    """The eval prefix of the freeze set `frozen` (names) of `keys` (all parameter names): the longest run of forward stages
    starting at the stem -- `stem`, then the bottlenecks in order -- in which every parameter is frozen.  -> the stage names
    (empty when the stem still trains).  temp_enc and the temporal stack are never part of it; a frozen stage behind the
    first trainable one is not either (the gradient passes through it: it keeps batch statistics)."""
    trainable = {stage_of(k) for k in keys if k not in frozen}
    out = []
    for s in forward_stages(spec):
        if s in trainable:
            break
        out.append(s)
    return out


def checked_eval_prefix(spec, frozen, keys, frozen_stats):
    """eval_prefix under frozen_stats = 'eval' (ValueError when it is empty), () under 'batch'."""
    if check_frozen_stats(frozen_stats) == "batch":
        return ()
    pre = tuple(eval_prefix(spec, frozen, keys))
    if not pre:
        raise ValueError("frozen_stats='eval' with an empty eval prefix: the stem still has a trainable parameter, so no "
                         "stage of the trunk can run in eval mode (freeze '_features.stem.*' and the stages behind it, "
                         "in order)")
    return pre


class FlatParams:
    @staticmethod
    def _layout(keys, sizes):
        """-> (offsets, numel).  Every tensor starts on a 16-byte boundary so that per-tensor kernels can use vector
        accesses; the boundary between the trunk and the temporal stack (= the boundary between the two gradient buckets of
        a data-parallel job) and the end of the buffer sit on multiples of BUCKET_ALIGN elements, so that each bucket
        divides evenly over 2, 4 and 8 ranks with 16-byte-aligned shards: the reduce-scatter + all-gather form of the
        all-reduce wants that (with 4-element padding only, both buckets were 4 mod 8 and fell back to
        a plain all-reduce at 8 ranks)."""
        offs, cur = [], 0
        prev_late = None
        for k, n in zip(keys, sizes):
            late = is_late_bucket_key(k)
            if prev_late is not None and late != prev_late:
                cur = (cur + BUCKET_ALIGN - 1) // BUCKET_ALIGN * BUCKET_ALIGN
            prev_late = late
            offs.append(cur)
            cur += (n + 3) // 4 * 4
        cur = (cur + BUCKET_ALIGN - 1) // BUCKET_ALIGN * BUCKET_ALIGN
        return offs, cur

    @classmethod
    def layout_only(cls, state):
        """The index / numel this class would give `state` (name -> anything with .numel() / .shape), nothing allocated."""
        from types import SimpleNamespace
        keys = [k for k in state if state_layout.is_parameter(k)]
        sizes = [int(state[k].numel()) for k in keys]
        offs, numel = cls._layout(keys, sizes)
        return SimpleNamespace(numel=numel, index={k: (o, n) for k, o, n in zip(keys, offs, sizes)})

    def __init__(self, state, device=None):
        keys = [k for k in state if state_layout.is_parameter(k)]
        device = device if device is not None else state[keys[0]].device
        sizes = [int(state[k].numel()) for k in keys]
        offs, cur = self._layout(keys, sizes)
        self.numel = cur
        self.flat = torch.zeros(cur, dtype=torch.float32, device=device)
        self.grad = torch.zeros(cur, dtype=torch.float32, device=device)
        self.index, self.shapes = {}, {}
        for k, o, n in zip(keys, offs, sizes):
            view = self.flat[o:o + n].view(state[k].shape)
            view.copy_(state[k].to(device=device, dtype=torch.float32))
            state[k] = view                      # the state_dict entry now aliases the flat buffer
            self.index[k] = (o, n)
            self.shapes[k] = tuple(view.shape)
        # BatchNorm step counters (nn.BatchNorm.num_batches_tracked): one int64 vector, bumped by one launch per step
        nbt = [k for k in state if k.endswith("num_batches_tracked")]
        self.nbt = torch.zeros(max(len(nbt), 1), dtype=torch.int64, device=device)
        for i, k in enumerate(nbt):
            self.nbt[i] = state[k].to(device=device, dtype=torch.int64).reshape(())
            state[k] = self.nbt[i:i + 1].view(())

    def grad_view(self, key):
        o, n = self.index[key]
        return self.grad[o:o + n]


class FusedAdamW:
    def __init__(self, params: FlatParams, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        self.p, self.lr, self.betas, self.eps, self.wd = params, lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(params.flat)
        self.exp_avg_sq = torch.zeros_like(params.flat)
        self.t = 0                      # the host's count of step() calls (attempts): skipped ones included
        self.guard = None               # set_guard(): the device record of tdeed_grad_guard, int32 (8,)
        self.guard_ws = None
        self.skip_nonfinite, self.max_grad_norm = False, None
        self._last_grad_scale = 1.0
        self.groups, self.runs, self.run_table = None, None, None    # set_groups(): the grouped launch
        self.frozen = frozenset()
        # set_ema(): the shadow of the flat buffer, updated inside the AdamW launch (tdeed_adamw_step_ema)
        self.ema, self.ema_decay, self.ema_warmup, self.ema_step0 = None, None, False, 0
        self.ema_gen = 0                # bumped whenever the shadow (or a statistics shadow behind ema_hook) may have changed
        self.ema_hook = None            # callable(opt) issued right behind the EMA launch (TrainEngine: the BatchNorm statistics)
        self.ema_stats_get = self.ema_stats_set = None   # the hook owner's statistics shadow, for state_dict()

    def zero_grad(self):
        self.p.grad.zero_()

    def set_groups(self, groups):
        """Parameter groups (opt-in; None or an empty list returns to the plain launch).  Builds the run table once and
        uploads it; step() then takes tdeed_adamw_step_groups.  The gradient ranges of frozen tensors are zeroed here:
        nothing writes them from now on, and a stale value from before the freeze must not reach the global norm."""
        if not groups:
            self.groups, self.runs, self.run_table, self.frozen = None, None, None, frozenset()
            return
        runs = group_table(self.p.index, self.p.numel, groups, None)
        self.groups, self.runs = groups_as_dicts(groups), runs
        self.frozen = frozen_keys(self.p.index, groups)
        dev = self.p.flat.device
        self.run_table = ops.adamw_run_table(runs, self.p.numel, dev) if dev.type == "cuda" else None
        for k in self.frozen:
            self.p.grad_view(k).zero_()

    def set_guard(self, skip_nonfinite=False, max_grad_norm=None):
        """Guard the update (opt-in).  skip_nonfinite: a step whose gradient buffer holds an inf or a NaN writes nothing
        and does not advance the bias correction -- what the reference's GradScaler.step() did (modules.py:390-404).
        max_grad_norm: clip by the global norm with torch.nn.utils.clip_grad_norm_'s rule, applied to the gradient AdamW
        sees (after grad_scale).  The record and the workspace are allocated once; from then on step() takes the guarded
        launch, also with both options off again, because the count of skipped steps lives in the record."""
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0:
                raise ValueError(f"max_grad_norm must be None or > 0, got {max_grad_norm}")
        if not isinstance(skip_nonfinite, (bool, int)):
            raise ValueError(f"skip_nonfinite must be a bool, got {skip_nonfinite!r}")
        self.skip_nonfinite, self.max_grad_norm = bool(skip_nonfinite), max_grad_norm
        if self.guard is None and (self.skip_nonfinite or max_grad_norm is not None):
            self._alloc_guard()

    def set_ema(self, decay, warmup=False):
        """Exponential moving average of the weights (opt-in; None switches it off and drops the buffers).  The shadow
        starts as a copy of the flat buffer now, and every APPLIED step from now on moves it inside the AdamW launch by
        ema_ref's arithmetic at n = (t - skipped) - ema_step0.  ema_step0 = t - skipped is recorded here: one device
        synchronisation when a guard record exists, none otherwise.  Calling it again while EMA is on only changes decay /
        warmup (the shadow and ema_step0 stay)."""
        if decay is None:
            self.ema, self.ema_decay, self.ema_warmup, self.ema_step0 = None, None, False, 0
            self.ema_gen += 1
            return
        decay, warmup = check_ema(decay, warmup)
        if self.ema is None:
            self.ema = self.p.flat.clone()
            self.ema_step0 = self.t - self._record()[2]
            self.ema_gen += 1
        self.ema_decay, self.ema_warmup = decay, warmup

    def _alloc_guard(self):
        dev = self.p.flat.device
        self.guard = torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=dev)
        if dev.type == "cuda":
            self.guard_ws = ops.grad_guard_ws(self.p.flat.numel(), dev)

    def step(self, lr_factor=1.0, grad_scale=1.0):
        self.t += 1
        if self.ema is not None:
            # one launch for all three forms below (run table and record are optional), the shadow updated in it
            if self.guard is not None and (self.skip_nonfinite or self.max_grad_norm is not None):
                ops.grad_guard(self.p.grad, self.guard, self.guard_ws, self.skip_nonfinite)
            self._last_grad_scale = grad_scale
            ops.adamw_step_ema(self.p.flat, self.p.grad, self.exp_avg, self.exp_avg_sq, self.t, self.lr * lr_factor,
                               self.ema, self.ema_decay, self.ema_warmup, self.ema_step0, self.run_table, self.betas,
                               self.eps, self.wd, grad_scale, self.guard, self.skip_nonfinite, self.max_grad_norm)
            if self.ema_hook is not None:
                self.ema_hook(self)
            self.ema_gen += 1
            return
        if self.run_table is not None:
            # frozen gradient ranges are zeros (set_groups; nothing writes them), so the statistics over the whole buffer
            # are those of the trainable parameters and the one global clipping coefficient is clip_grad_norm_'s
            if self.guard is not None and (self.skip_nonfinite or self.max_grad_norm is not None):
                ops.grad_guard(self.p.grad, self.guard, self.guard_ws, self.skip_nonfinite)
            self._last_grad_scale = grad_scale
            ops.adamw_step_groups(self.p.flat, self.p.grad, self.exp_avg, self.exp_avg_sq, self.t, self.lr * lr_factor,
                                  self.run_table, self.betas, self.eps, self.wd, grad_scale, self.guard,
                                  self.skip_nonfinite, self.max_grad_norm)
            return
        if self.guard is None:
            ops.adamw_step(self.p.flat, self.p.grad, self.exp_avg, self.exp_avg_sq, self.t, self.lr * lr_factor,
                           self.betas, self.eps, self.wd, grad_scale)
            return
        # Statistics, then the update behind them, both on the current stream: no host synchronisation, legal under capture.
        # Data parallel: this runs after reducer.join() / the blocking all_reduce (TrainEngine.apply, step_graph), when
        # every rank holds the same summed gradient buffer bit for bit (tests/test_gpu_dp.py asserts it).  The statistics
        # are a fixed-order function of that buffer, so every rank skips or clips alike WITHOUT another collective.
        if self.skip_nonfinite or self.max_grad_norm is not None:
            ops.grad_guard(self.p.grad, self.guard, self.guard_ws, self.skip_nonfinite)
        self._last_grad_scale = grad_scale
        ops.adamw_step_guarded(self.p.flat, self.p.grad, self.exp_avg, self.exp_avg_sq, self.t, self.lr * lr_factor,
                               self.betas, self.eps, self.wd, grad_scale, self.guard, self.skip_nonfinite,
                               self.max_grad_norm)

    def _record(self):
        """(sumsq, nonfinite, skipped) of the record; one device synchronisation."""
        if self.guard is None:
            return 0.0, 0, 0
        rec = self.guard.cpu()
        return float(rec[:2].view(torch.float64)[0]), int(rec[2]), int(rec[3])

    def guard_stats(self):
        """dict(skipped: steps skipped so far, last_nonfinite: whether the last step's gradient held an inf / NaN,
        last_norm: grad_scale * sqrt(sumsq) of the last step, the norm clipping compares).  Costs ONE device
        synchronisation: call it per epoch or for logging, not per step."""
        sumsq, bad, skipped = self._record()
        norm = float("nan") if math.isnan(sumsq) else self._last_grad_scale * math.sqrt(sumsq)
        return dict(skipped=skipped, last_nonfinite=bool(bad), last_norm=norm)

    def state_dict(self):
        """exp_avg, exp_avg_sq (clones), t (attempts) and skipped (the device half of the step count; one synchronisation).
        The same dict is the `state` of guarded_adamw_ref."""
        sd = dict(exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), t=int(self.t),
                  skipped=self._record()[2])
        if self.ema is not None:
            # with EMA on: the shadow, the statistics shadow of the hook's owner (None without one) and the three scalars
            stats = self.ema_stats_get() if self.ema_stats_get is not None else None
            sd.update(ema=self.ema.clone(), ema_stats=None if stats is None else stats.clone(),
                      ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema_step0=int(self.ema_step0))
        return sd

    def load_state_dict(self, sd):
        """Both counters come back as saved, so the resumed optimizer takes the bias-correction path (host values while
        skipped == 0, device powf of t - skipped afterwards) the one that went on running takes."""
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.t = int(sd["t"])
        skipped = int(sd.get("skipped", 0))
        if self.guard is None and skipped:
            self._alloc_guard()
        if self.guard is not None:
            self.guard.zero_()
            self.guard[3] = skipped
        if sd.get("ema") is not None:                            # (a state without the EMA keys loads as before)
            self.set_ema(sd["ema_decay"], sd["ema_warmup"])
            self.ema.copy_(sd["ema"])
            self.ema_step0 = int(sd["ema_step0"])
            if sd.get("ema_stats") is not None and self.ema_stats_set is not None:
                self.ema_stats_set(sd["ema_stats"])
            self.ema_gen += 1


def check_ema(decay, warmup=False):
    """-> (float decay, bool warmup); ValueError unless 0 < decay < 1 (a number) and warmup is a bool."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 < float(decay) < 1.0:
        raise ValueError(f"ema_decay must be a float with 0 < decay < 1, got {decay!r}")
    if not isinstance(warmup, bool):
        raise ValueError(f"ema_warmup must be a bool, got {warmup!r}")
    import numpy as np
    if not 0.0 < float(np.float32(decay)) < 1.0:
        raise ValueError(f"ema_decay must lie inside (0, 1) as a float32, got {decay!r}")
    return float(decay), warmup


def ema_decay_at(n, decay, warmup=False):
    """d_n as a float32 tensor: float32(decay), or with warmup min(that, float32(1 + n) / float32(10 + n)) -- a correctly
    rounded fp32 quotient.  n >= 1: the number of applied updates since EMA was switched on, counting this one."""
    if n < 1:
        raise ValueError(f"ema: n counts applied updates from 1, got {n}")
    d = torch.tensor(decay, dtype=torch.float32)
    if warmup:
        d = torch.minimum(d, torch.tensor(1 + n, dtype=torch.float32) / torch.tensor(10 + n, dtype=torch.float32))
    return d


def ema_ref(shadow, param, n, decay, warmup=False):
    """The EMA update of the fused launch restated on torch-CPU fp32 tensors, in place on `shadow`: w = 1 - d_n, then per
    element diff = param - shadow, prod = w * diff, shadow += prod -- three roundings, nothing fused.  The device result
    equals this bit for bit (tests/test_gpu_ema.py).  -> shadow."""
    decay, warmup = check_ema(decay, warmup)
    if shadow.dtype != torch.float32 or param.dtype != torch.float32 or shadow.is_cuda or param.is_cuda:
        raise TypeError("ema_ref: float32 CPU tensors")
    w = torch.tensor(1.0, dtype=torch.float32) - ema_decay_at(int(n), decay, warmup)
    diff = param - shadow
    prod = diff * w
    shadow.add_(prod)
    return shadow


def is_ema_stat(key):
    """The buffers the statistics shadow averages: BatchNorm running_mean / running_var (num_batches_tracked is not
    averaged: the averaged model carries the live counters)."""
    return key.rsplit(".", 1)[-1] in ("running_mean", "running_var")


def ema_stat_layout(state):
    """-> ({key: (offset, count)} for every running_mean / running_var of `state` in state-dict order, packed back to back;
    total elements): the layout of the statistics shadow and of its row table."""
    out, cur = {}, 0
    for k, v in state.items():
        if is_ema_stat(k):
            n = int(v.numel())
            out[k] = (cur, n)
            cur += n
    return out, cur


def ema_state_map(state, index, shadow, stat_index, stat_shadow):
    """The averaged model as an ordered mapping with the keys and the order of `state`: parameters as views of `shadow`
    (the flat buffer's twin) through `index` (FlatParams.index), running statistics as views of `stat_shadow` through
    `stat_index` (ema_stat_layout), everything else (the step counters) the live tensor.  Nothing is copied."""
    from collections import OrderedDict
    out = OrderedDict()
    for k, v in state.items():
        if k in index:
            o, n = index[k]
            out[k] = shadow[o:o + n].view(v.shape)
        elif k in stat_index:
            o, n = stat_index[k]
            out[k] = stat_shadow[o:o + n].view(v.shape)
        else:
            out[k] = v
    return out


def guarded_adamw_ref(param, grad, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=1.0,
                      skip_nonfinite=False, max_grad_norm=None):
    """Restatement on torch-CPU tensors of FusedAdamW.step() with a guard, for the tests: one attempt on `param` (fp32,
    updated in place) with `state` = dict(exp_avg, exp_avg_sq, t, skipped) as FusedAdamW.state_dict() gives it (updated in
    place).  The update is torch.optim.AdamW's single-tensor arithmetic in its order, at the effective step t - skipped.
    -> dict(nonfinite, norm, coef) of this attempt."""
    state["t"] += 1
    sumsq = float((grad.double() ** 2).sum())
    bad = not math.isfinite(sumsq)
    norm = torch.tensor(grad_scale * math.sqrt(sumsq) if sumsq == sumsq else float("nan"), dtype=torch.float64).float()
    if skip_nonfinite and bad:
        state["skipped"] += 1
        return dict(nonfinite=True, norm=float(norm), coef=None)
    gscale = torch.tensor(grad_scale, dtype=torch.float32)
    coef = None
    if max_grad_norm is not None:
        coef = torch.clamp(torch.tensor(max_grad_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
        gscale = gscale * coef
    g = grad if float(gscale) == 1.0 else grad * gscale
    step = state["t"] - state["skipped"]
    b1, b2 = betas
    m, v = state["exp_avg"], state["exp_avg_sq"]
    param.mul_(1 - lr * weight_decay)
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2_sqrt = (1 - b2 ** step) ** 0.5
    denom = (v.sqrt() / bc2_sqrt).add_(eps)
    param.addcdiv_(m, denom, value=-(lr / bc1))
    return dict(nonfinite=bad, norm=float(norm), coef=None if coef is None else float(coef))


def grouped_adamw_ref(param, grad, state, runs, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=1.0,
                      skip_nonfinite=False, max_grad_norm=None):
    """Restatement on torch-CPU tensors of FusedAdamW.step() with parameter groups, for the tests: one attempt over the
    `runs` of group_table (a weight_decay of None: `weight_decay`).  The decision to skip and the clipping coefficient are
    those of the whole buffer (guarded_adamw_ref's rule); each run is then guarded_adamw_ref on its slice at
    float32(lr) * float32(lr_scale) with the run's decay, and a frozen run is left untouched.
    -> dict(nonfinite, norm, coef) of this attempt."""
    import numpy as np
    sumsq = float((grad.double() ** 2).sum())
    bad = not math.isfinite(sumsq)
    norm = torch.tensor(grad_scale * math.sqrt(sumsq) if sumsq == sumsq else float("nan"), dtype=torch.float64).float()
    state["t"] += 1
    if skip_nonfinite and bad:
        state["skipped"] += 1
        return dict(nonfinite=True, norm=float(norm), coef=None)
    gscale, coef = torch.tensor(grad_scale, dtype=torch.float32), None
    if max_grad_norm is not None:
        coef = torch.clamp(torch.tensor(max_grad_norm, dtype=torch.float32) / (norm + 1e-6), max=1.0)
        gscale = gscale * coef
    lo = 0
    for end, scale, wd, frozen in runs:
        if not frozen:
            sub = dict(exp_avg=state["exp_avg"][lo:end], exp_avg_sq=state["exp_avg_sq"][lo:end], t=state["t"] - 1,
                       skipped=state["skipped"])
            guarded_adamw_ref(param[lo:end], grad[lo:end], sub, float(np.float32(lr) * np.float32(scale)), betas, eps,
                              weight_decay if wd is None else wd, grad_scale=float(gscale))
        lo = end
    return dict(nonfinite=bad, norm=float(norm), coef=None if coef is None else float(coef))


def warmup_cosine_lr(step, warmup_steps, cosine_steps, start_factor=0.01):
    """LR multiplier after `step` scheduler steps of ChainedScheduler([LinearLR, CosineAnnealingLR(T_max)])."""
    lin = 1.0 if warmup_steps <= 0 else start_factor + (1.0 - start_factor) * min(step, warmup_steps) / warmup_steps
    cos = 0.5 * (1.0 + math.cos(math.pi * step / cosine_steps)) if cosine_steps > 0 else 1.0
    return lin * cos
