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

    def zero_grad(self):
        self.p.grad.zero_()

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

    def _alloc_guard(self):
        dev = self.p.flat.device
        self.guard = torch.zeros(ops.GUARD_WORDS, dtype=torch.int32, device=dev)
        if dev.type == "cuda":
            self.guard_ws = ops.grad_guard_ws(self.p.flat.numel(), dev)

    def step(self, lr_factor=1.0, grad_scale=1.0):
        self.t += 1
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
        return dict(exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(), t=int(self.t),
                    skipped=self._record()[2])

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


def warmup_cosine_lr(step, warmup_steps, cosine_steps, start_factor=0.01):
    """LR multiplier after `step` scheduler steps of ChainedScheduler([LinearLR, CosineAnnealingLR(T_max)])."""
    lin = 1.0 if warmup_steps <= 0 else start_factor + (1.0 - start_factor) * min(step, warmup_steps) / warmup_steps
    cos = 0.5 * (1.0 + math.cos(math.pi * step / cosine_steps)) if cosine_steps > 0 else 1.0
    return lin * cos
