"""The frozen, eval-mode prefix of the trunk inside the training step (`TrainEngine.set_groups(frozen_stats='eval')`).

A run of trunk stages from the stem on whose parameters are all frozen (`optim.eval_prefix`) has constant weights and, in
eval mode, constant BatchNorm affines: torch's `.eval()` + `requires_grad_(False)` on those sub-modules.  That is what the
inference engine packs and launches, so the prefix runs as the launches of a `TrunkBuilder` over `PackedWeights` made from
the frozen tensors -- folded BatchNorm, one-launch bottlenecks, gate-shift sites inside the blocks, nothing saved for a
backward -- and hands block k's input map to the train-mode code behind it.  Everything is issued on the step's stream, so
`TrainEngine.build_graph` captures it with the rest.

The packed copies are made when the prefix is set and again when the tensors are loaded (`TrainEngine.reload_prefix`); an
optimizer step does not touch frozen tensors, so `repack()` leaves them alone."""
import torch

from . import _lib
from .engine import PackedWeights, TrunkBuilder
from .packing import stem_frags_on_device

SCOPE = "prefix.fwd"
# bf16, wherever the fused front does not take the frames (fp32 frames, per-frame flips, a stem-only prefix, a band that does
# not fit the front): the eval instance of the training stem's MFMA kernel instead of tdeed_stem_fwd
STEM_MFMA_EVAL = True
# launch lists kept for eager steps (each owns its buffers: at 800MF B = 16 the stem map alone is 1.3 GB); the least
# recently used one goes first.  Two: a loop whose batches alternate between "no flip" and per-clip flags rebuilds nothing
MAX_PLANS = 2


class _PrefixPlan:
    __slots__ = ("frames", "flip_buf", "rect", "steps", "out", "h", "w", "pool_bytes", "runs")


class EvalPrefix:
    """The stem and the blocks [0, k) of the trunk in eval mode.  state: the train engine's state (device tensors)."""

    def __init__(self, cfg, state, k, act_dtype, device):
        self.k, self.dt, self.device = int(k), act_dtype, device
        self.pw = PackedWeights(cfg, state, act_dtype, device)
        self.stem_wf = None
        if act_dtype == torch.bfloat16 and STEM_MFMA_EVAL:
            self.stem_wf = stem_frags_on_device(state["_features.stem.conv.weight"].detach().float()).clone()
        self._plans = {}                                         # insertion order = least recently used first
        self.last_plan = None                                    # the plan of the last run(); .runs counts its runs

    def _plan(self, N, H, W, frames_dtype, chw, per_frame, flip_all, static):
        """One launch list per (frames, window size, flip form): the window's origin and the flags are read at every run.
        static: the caller's frame buffer, read in place (a captured step's input); None: a buffer of the plan's."""
        T = self.pw.clip_len
        key = (N, H, W, frames_dtype, chw, per_frame, flip_all, None if static is None else static.data_ptr())
        pl = self._plans.pop(key, None)
        if pl is not None:
            self._plans[key] = pl                                # (most recently used: last)
            return pl
        eager = [k for k in self._plans if k[-1] is None]
        if static is None and len(eager) >= MAX_PLANS:
            # (a forward still waiting for its backward holds the evicted plan's map through its ctx)
            del self._plans[eager[0]]
        pl = _PrefixPlan()
        pl.runs = 0
        pl.flip_buf = torch.zeros((N,), dtype=torch.uint8, device=self.device) if per_frame else None
        pl.rect = [0, 0, chw[0], chw[1]]
        tb = TrunkBuilder(self.pw, self.dt, self.device, set(), N // T, fuse_front=True)
        tb.stem_wf = self.stem_wf                                # (the fused front, where it serves the frames, comes first)
        x, h, w, _ = tb.trunk(H, W, None, pl.flip_buf if per_frame else flip_all, frames_dtype, stop=self.k, rect=pl.rect,
                              frames=static)
        # x is the last buffer taken from the builder's pool and is never given back: nothing recycles block k's input,
        # which block k's backward reads again
        pl.frames, pl.steps, pl.out, pl.h, pl.w, pl.pool_bytes = tb.frames, tb.steps, x, h, w, tb.pool.total_bytes()
        self._plans[key] = pl
        return pl

    def take_static(self):
        """Hand over the plans built over a caller's static frame buffer (and forget them here): a captured step holds their
        buffers' addresses, so they must live exactly as long as its handle."""
        keys = [k for k in self._plans if k[-1] is not None]
        return [self._plans.pop(k) for k in keys]

    def run(self, fr, crop, flip, static=False):
        """fr (N,3,H,W) uint8 or fp32 0..255; crop (top,left,h,w) or None; flip: bool or per-frame uint8 flags (N,) (what
        TrainEngine._frame_flip returns).  static: fr is a buffer that lives as long as the engine's captured step (read in
        place).  Returns block k's input map (N,h,w,C) in the engine's dtype: a buffer of the plan (self.last_plan), valid
        until the next run of the same plan (its .runs counts them; TrainEngine.backward_trunk checks it)."""
        N, _, H, W = fr.shape
        chw = (crop[2], crop[3]) if crop is not None else (H, W)
        per_frame = isinstance(flip, torch.Tensor)
        pl = self._plan(N, H, W, fr.dtype, chw, per_frame, False if per_frame else bool(flip), fr if static else None)
        if crop is not None:
            if crop[0] < 0 or crop[1] < 0 or crop[0] + crop[2] > H or crop[1] + crop[3] > W:
                raise ValueError(f"crop {tuple(crop)} leaves the {H} x {W} frame")
            pl.rect[0], pl.rect[1] = int(crop[0]), int(crop[1])
        else:
            pl.rect[0] = pl.rect[1] = 0
        if pl.frames.data_ptr() != fr.data_ptr():
            pl.frames.copy_(fr, non_blocking=True)
        if per_frame:
            pl.flip_buf.copy_(flip, non_blocking=True)
        pl.runs += 1
        self.last_plan = pl
        scope, _lib.SCOPE = _lib.SCOPE, SCOPE
        try:
            for st in pl.steps:
                st.fn()
        finally:
            _lib.SCOPE = scope
        return pl.out
