"""Drop-in counterpart of the reference's ``model/model.py`` API, backed by the HIP engine.

Same constructor arguments, attributes and method signatures as
``TDEEDModel`` / ``TDEEDModel.Impl`` (/root/reference/model/model.py:21-376) and
``BaseRGBModel`` (/root/reference/model/modules.py:35-55), so ``train_tdeed.py:142-148``,
``util/eval.py:301-339`` and ``evaluate_tdeed_challenge.py`` can import this module
instead.  There is exactly one execution backend (the gfx950 kernels); without the
built library or without a GPU every compute call raises.
"""
import contextlib
from types import SimpleNamespace

import numpy as np
import torch

from . import ops, state_layout, augment
from . import init as ref_init
from .engine import ForwardEngine
from .regnet_spec import regnet_spec


def _cfg_from_args(args):
    crop = getattr(args, "crop_dim", None)
    if crop is not None and crop <= 0:      # train_tdeed.py:110-111
        crop = None
    return dict(feature_arch=args.feature_arch, clip_len=args.clip_len, crop_dim=crop,
                n_layers=args.n_layers, sgp_ks=args.sgp_ks, sgp_r=args.sgp_r,
                num_classes=args.num_classes, radi_displacement=args.radi_displacement)


class TDEEDModel:

    class Impl:
        """The network.  Holds the fp32 master state in the reference's key grammar."""

        def __init__(self, args=None, seed=None):
            self._modality = args.modality
            assert self._modality == "rgb", "Only RGB supported for now"
            self._temp_arch = args.temporal_arch
            assert self._temp_arch in ["ed_sgp_mixer"], "Only ed_sgp_mixer supported for now"
            self._radi_displacement = args.radi_displacement
            self._feature_arch = args.feature_arch
            assert "rny" in self._feature_arch, "Only rny supported for now"
            if not self._feature_arch.startswith(("rny002", "rny008")):
                raise NotImplementedError(self._feature_arch)
            self._double_head = False
            self._cfg = _cfg_from_args(args)
            self._spec = regnet_spec(self._feature_arch)
            self._d = self._feat_dim = self._spec.feat_dim
            self._require_clip_len = args.clip_len if self._feature_arch.endswith(("_gsm", "_gsf")) else -1
            self.croping = self._cfg["crop_dim"]
            self._head_classes = None
            # The reference's construction-time state (init.py: timm's RegNet init with zero_init_last, BatchNorm identity
            # statistics, temp_enc ~ N(0, 1/L), depthwise convs N(0, 0.1) with zero biases, torch defaults elsewhere;
            # model.py:38-70, modules.py:146-157, 255-275).  There is no network here, so the ImageNet weights that
            # `pretrained=True` (model.py:38-41) downloads arrive through load_timm_backbone() / load().
            # seed: None draws from torch's global CPU generator like the reference's constructors do.
            shapes = state_layout.model_state_shapes(self._cfg)
            gen = None if seed is None else torch.Generator().manual_seed(int(seed))
            self._state = ref_init.reference_init(shapes, self._cfg, gen)
            self._device = "cpu"
            self.training = False
            self._engines = {}
            self._train_engine = None               # trainer.TrainEngine over self._state (get_optimizer / first train-mode call)
            self._train_dtype = torch.bfloat16      # the reference trains under autocast; torch.float32 for parity runs
            self._train_ctx = None                  # activations of the last train-mode forward (for the backward)
            self._averaged = False                  # inside TDEEDModel.averaged(): engine() serves the averaged weights
            self._ema_engines = {}                  # act_dtype -> (FusedAdamW.ema_gen they were packed at, ForwardEngine)
            self.augment_fn = None                  # optional hook replacing the built-in train-time augmentation:
            #   augment_fn(frames (B,T,3,H,W) uint8|fp32 0..255 on the device, crop (top,left,h,w)|None) -> frames of the
            #   crop window (B,T,3,h,w), uint8 or fp32 0..255, on the device (flips included, if wanted)
            self.augment_generator = None           # torch.Generator for the augmentation draws (None: the global CPU one)
            self._kd_wanted = False                 # a teacher is set (TDEEDModel.distill_from): train-mode forwards hand
            self._kd_view = None                    # ... their view (crop-window frames, per-frame flip flags) over here
            self.dropout_mask_fn = None             # optional hook replaying a recorded dropout draw of the heads:
            #   dropout_mask_fn(B, T, C, n_heads) -> n_heads tensors (B,T,C) of 0 / 2 (class head(s) first, displacement last)

        # ---- nn.Module-like surface the reference's callers touch
        @staticmethod
        def _norm_device(device):
            d = torch.device(device)
            if d.type == "cuda" and d.index is None and torch.cuda.is_available():
                d = torch.device("cuda", torch.cuda.current_device())
            return d

        def to(self, device):
            if self._train_engine is not None and self._norm_device(device) != self._norm_device(self._device):
                raise RuntimeError("the model cannot change device once its training engine exists")
            self._device = str(device)
            for k in list(self._state):          # in place: trainer / optimizer may hold this dict
                self._state[k] = self._state[k].to(device)
            self._engines = {}
            return self

        def cuda(self):
            return self.to("cuda")

        def train(self, mode=True):
            self.training = mode
            return self

        def eval(self):
            return self.train(False)

        def state_dict(self):
            return dict(self._state)

        def load_state_dict(self, sd, strict=True):
            missing = [k for k in self._state if k not in sd]
            extra = [k for k in sd if k not in self._state]
            if strict and (missing or extra):
                raise RuntimeError(f"state_dict mismatch: missing {missing[:5]} unexpected {extra[:5]}")
            for k, v in sd.items():
                if k in self._state:
                    v = torch.as_tensor(v)
                    if tuple(v.shape) != tuple(self._state[k].shape):
                        raise RuntimeError(f"shape mismatch for {k}: {tuple(v.shape)} vs {tuple(self._state[k].shape)}")
                    # in place: after get_optimizer() the parameters are views into one flat buffer that the fused
                    # optimizer and the train engine hold on to
                    self._state[k].copy_(v.detach().to(self._state[k].dtype).to(self._device))
            self._engines = {}
            if self._train_engine is not None:
                # the train engine keeps packed copies (bf16 casts, transposes, MFMA fragments) of the master weights
                self._train_engine.repack()
                # ... and, for a frozen eval-mode prefix, folded copies that no optimizer step refreshes
                self._train_engine.reload_prefix()

        def load_timm_backbone(self, timm_state_dict):
            """Fill the trunk from a timm `regnety_002` / `regnety_008` state_dict (what `timm.create_model(...,
            pretrained=True)` holds at model.py:38-41): `stem.* / s{1..4}.b{n}.*` -> `_features.*`, with `conv1.*` ->
            `conv1.net.*` on the gate-shift stages s3 / s4 (shift.py:46-59); `head.fc.*` is dropped (model.py:45).  The
            gate-shift modules, temp_enc, the temporal stack and the heads keep their construction-time state.
            Returns the list of keys it filled."""
            mapped = ref_init.map_timm_backbone(timm_state_dict, self._cfg)
            self.load_state_dict(mapped, strict=False)
            return list(mapped)

        def parameters(self):
            return [v for k, v in self._state.items() if state_layout.is_parameter(k)]

        def update_pred_head(self, num_classes=[1, 1]):
            """model.py:169-172: replace the class head by two heads (joint-dataset training)."""
            C = self._feat_dim
            for k in [k for k in self._state if k.startswith("_pred_fine.")]:
                del self._state[k]
            shapes = {}
            for i, n in enumerate(num_classes, start=1):
                shapes[f"_pred_fine._fc{i}._fc_out.weight"] = ((n, C), "float32")
                shapes[f"_pred_fine._fc{i}._fc_out.bias"] = ((n,), "float32")
            new = {k: v.to(self._device) for k, v in ref_init.reference_init(shapes, self._cfg, None).items()}   # nn.Linear defaults
            # keep the reference's key order: heads sit before _pred_displ
            displ = {k: self._state.pop(k) for k in [k for k in self._state if k.startswith("_pred_displ.")]}
            self._state.update(new)
            self._state.update(displ)
            self._double_head = True
            self._head_classes = list(num_classes)
            self._engines = {}
            if self._train_engine is not None:
                raise RuntimeError("update_pred_head() must be called before get_optimizer() (train_tdeed.py:147-151 does)")

        def print_stats(self):
            def cnt(pfx):
                return sum(v.numel() for k, v in self._state.items()
                           if k.startswith(pfx) and state_layout.is_parameter(k))
            print("Model params:", cnt(""))
            print("  CNN features:", cnt("_features."))
            print("  Temporal:", cnt("_temp_fine."))
            print("  Head:", cnt("_pred_fine."))

        # ---- forward
        def engine(self, act_dtype):
            if self._averaged:
                return self._ema_engine(act_dtype)
            if act_dtype not in self._engines:
                if not str(self._device).startswith("cuda"):
                    raise RuntimeError("tdeed_amd runs on the GPU only: construct TDEEDModel(device='cuda')")
                self._engines[act_dtype] = ForwardEngine(self._cfg, self._state, act_dtype, self._device)
            return self._engines[act_dtype]

        def _ema_engine(self, act_dtype):
            """The inference engine over the averaged weights (TrainEngine.ema_state()), from a cache of its own: rebuilt only
            when the shadows have moved (an applied or attempted step, set_ema, load_state_dict) since it was packed.  The
            live engines, the packed training weights and every live tensor are not touched."""
            te = self._train_engine
            gen = te.opt.ema_gen
            hit = self._ema_engines.get(act_dtype)
            if hit is None or hit[0] != gen:
                hit = (gen, ForwardEngine(self._cfg, te.ema_state(), act_dtype, self._device))
                self._ema_engines[act_dtype] = hit
            return hit[1]

        def train_engine(self):
            """The training engine over this model's state (created by get_optimizer(), or lazily by the first
            train-mode forward): moves the parameters into one flat buffer, `self._state` then holds views into it."""
            if self._train_engine is None:
                if not str(self._device).startswith("cuda"):
                    raise RuntimeError("tdeed_amd runs on the GPU only: construct TDEEDModel(device='cuda')")
                from .trainer import TrainEngine
                self._train_engine = TrainEngine(self._cfg, self._state, act_dtype=self._train_dtype, device=self._device)
                self._engines = {}
            return self._train_engine

        def _pack_head(self, head, B, T, n_cls, displ_col, y):
            head = head.view(B, T, -1)
            im_feat = head[..., :n_cls]
            if self._radi_displacement > 0:
                return {"im_feat": im_feat, "displ_feat": head[..., displ_col], "_head_out": head}, y
            return im_feat, y

        def _draw_view(self, x):
            """The draws of the training branch (model.py:110-129) on frames (B,T,3,H,W) on the device: one random crop window
            for the whole batch, then augment_fn or the built-in per-clip augmentation and flips.
            -> (frames, crop, flip_c): the frames after the augmentation (the crop window only once it has been applied),
            the window (top, left, h, w) that is still to be cut out of them or None, and the per-clip flip flags (B,) uint8
            on the CPU, None when no clip flips."""
            B, T, _, H, W = x.shape
            cd = self.croping
            crop = None
            if cd and (cd != H or cd != W):
                # torchvision RandomCrop.get_params: torch.randint for the row, then for the column; ONE window for
                # the whole batch (model.py:115 crops the 5-D tensor)
                g = self.augment_generator
                top = int(torch.randint(0, H - cd + 1, size=(1,), generator=g).item())
                left = int(torch.randint(0, W - cd + 1, size=(1,), generator=g).item())
                crop = (top, left, cd, cd)
            flip_c = None
            if self.augment_fn is not None:
                x = self.augment_fn(x, crop)
                crop = None
                if x.dtype not in (torch.uint8, torch.float32) or not x.is_cuda:
                    raise TypeError("augment_fn must return uint8 / float32 frames on the device")
                x = x.contiguous()
            else:
                prm, flip_c = augment.draw_params(B, self.augment_generator)
                if not augment.is_identity(prm):
                    x = augment.apply(x, prm, crop)                 # fp32 0..255 frames of the crop window
                    crop = None
                if not bool(flip_c.any()):
                    flip_c = None
            return x, crop, flip_c

        def _view_of(self, x, crop, flip_c):
            """What `_draw_view` drew as an eval-mode forward takes it (ForwardEngine.forward_augmented): the crop-window
            frames (B,T,3,h,w), contiguous, and the per-frame flip flags (B*T,) uint8 on the device or None."""
            if crop is not None:
                x = x[..., crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
            flip_frames = None
            if flip_c is not None:
                flip_frames = flip_c.to(self._device).to(torch.uint8).repeat_interleave(x.shape[1]).contiguous()
            return x.contiguous(), flip_frames

        def _forward_train(self, x, y, inference, augment_inference):
            """model.py:105-149 under .train(): batch-statistics BatchNorm (running stats updated), dropout in the heads;
            `inference` only selects the crop / augmentation branch (model.py:110-129) like in the reference."""
            import random
            eng = self.train_engine()
            if x.dtype not in (torch.uint8, torch.float32):
                x = x.float()
            x = x.to(self._device).contiguous()           # uint8, or fp32 0..255 (mixup batches / callers' .float())
            B, T, _, H, W = x.shape
            if self._require_clip_len > 0 and T != self._require_clip_len:
                raise ValueError(f"clip length {T} != clip_len {self._require_clip_len} (gate-shift needs exact clips)")
            cd = self.croping
            crop, flip = None, False
            if not inference:
                x, crop, flip_c = self._draw_view(x)
                if flip_c is not None:
                    flip = flip_c.to(self._device)
                if self._kd_wanted:
                    # distillation (TDEEDModel.distill_from): the teacher gets exactly these pixels
                    self._kd_view = self._view_of(x, crop, flip_c)
            else:
                if cd and (cd != H or cd != W):
                    crop = (int(round((H - cd) / 2.0)), int(round((W - cd) / 2.0)), cd, cd)
                flip = bool(augment_inference)
            C = self._feat_dim
            n_heads = (2 if self._double_head else 1) + (1 if self._radi_displacement > 0 else 0)
            if self.dropout_mask_fn is not None:
                # replay of a recorded nn.Dropout draw (parity tests against reference fixtures): n_heads tensors (B,T,C)
                # holding 0 / 2, class head(s) first, displacement head last
                masks = [m.to(self._device).to(eng.dt).contiguous() for m in self.dropout_mask_fn(B, T, C, n_heads)]
            else:
                masks = [((torch.rand((B, T, C), device=self._device) >= 0.5).to(eng.dt) * 2.0) for _ in range(n_heads)]
            head, ctx = eng.forward_train(x, crop=crop, flip=flip, drop_masks=masks)
            self._train_ctx = ctx
            n_cls, dcol, _ = eng.temporal.head_layout()
            return self._pack_head(head, B, T, n_cls, dcol, y)

        def _forward_eval_augmented(self, x, y, act_dtype):
            """model.py:105-129 with `inference=False` on a module in eval() mode: the training branch's random crop (one
            window for the whole batch, model.py:115) and per-clip augmentation (model.py:76-83, 154-157) in front of
            running-statistics BatchNorm and no dropout.  No caller of the reference uses this pairing (epoch() pairs
            train() with inference=False and eval() with inference=True, model.py:196-203); it is here because the
            reference's nn.Module allows it.  Same RNG draw order as the train-mode forward."""
            if x.dtype not in (torch.uint8, torch.float32):
                x = x.float()
            x = x.to(self._device).contiguous()
            B, T = x.shape[:2]
            x, flip_frames = self._view_of(*self._draw_view(x))
            eng = self.engine(act_dtype)
            head, _ = eng.forward_augmented(x, flip_frames)
            pw = eng.pw
            return self._pack_head(head, B, T, pw.n_cls, pw.displ_col, y)

        def forward(self, x, y=None, inference=False, augment_inference=False, act_dtype=torch.bfloat16, slot=0):
            """model.py:105-149.  x: (B,T,3,H,W) uint8, or float holding 0..255 values.  Like the reference's nn.Module,
            .train()/.eval() select BatchNorm statistics + dropout and `inference` selects the crop / augmentation branch.
            slot (eval only): which of the engine's independent buffer sets to use (two batches in flight on two streams)."""
            if self.training:
                if self._averaged:
                    raise RuntimeError("a train-mode forward inside averaged(): the averaged weights are for scoring only")
                return self._forward_train(x, y, inference, augment_inference)
            if not inference:
                return self._forward_eval_augmented(x, y, act_dtype)
            if x.dtype != torch.uint8:
                x = x.round().clamp_(0, 255).to(torch.uint8)
            x = x.to(self._device)
            B, T = x.shape[:2]
            eng = self.engine(act_dtype)
            head, _ = eng.forward(x.contiguous(), augment_inference, slot=slot)
            pw = eng.pw
            return self._pack_head(head, B, T, pw.n_cls, pw.displ_col, y)

        __call__ = forward

    # ----------------------------------------------------------------------------------------
    def __init__(self, device="cuda", args=None):
        self.device = device
        self._model = TDEEDModel.Impl(args=args)
        self._model.print_stats()
        self._args = args
        self._model.to(device)
        self._num_classes = args.num_classes + 1
        self._stream = None
        self._kd = None                 # distill_from(): (teacher, teacher_dtype, settings)
        self._kd_last = None            # the teacher's head buffer of the last distillation step (a reference, not a copy)
        self.loss_parts = None          # after a training epoch with a teacher: means of ce / mse / kd / kd_displ
        self._loss_opt = None           # loss_options(): dict(label_smoothing, focal_gamma, class_weights) or None

    # BaseRGBModel (modules.py:35-55)
    def get_optimizer(self, opt_args):
        """modules.py:37-39: AdamW over all parameters (+ a GradScaler in the reference; bf16 needs none -> None).
        The returned optimizer is a torch.optim.Optimizer over the model's single flat parameter buffer whose step() is
        the fused AdamW kernel, so torch LR schedulers work on it unchanged.
        opt_args['groups'] (opt-in): a list of {'params': fnmatch patterns over the state_dict names, 'lr_scale',
        'weight_decay', 'frozen'} -- per-tensor settings inside the one launch, and frozen tensors whose backward is not
        run (trainer.HipAdamW, optim.check_groups).
        opt_args['frozen_stats'] (opt-in): 'eval' runs the frozen prefix of the trunk -- the stem and the bottlenecks behind
        it, as long as every parameter is frozen -- in eval mode on the inference kernels (TrainEngine.set_groups);
        'batch' (default) leaves the forward as it is.
        opt_args['ema_decay'] / ['ema_warmup'] (opt-in): an exponential moving average of the weights inside the AdamW launch
        and of the BatchNorm running statistics behind it (TrainEngine.set_ema); averaged() / ema_state_dict() use it."""
        from .trainer import HipAdamW
        eng = self._model.train_engine()
        if eng.reducer is None:
            eng.set_reducer("auto")          # data-parallel job (torch.distributed initialised, world > 1): bucketed all-reduce
        return HipAdamW(eng, **opt_args), None

    def distill_from(self, teacher, alpha=0.5, temperature=2.0, displ_weight=0.0, teacher_dtype=torch.bfloat16):
        """Train this model against `teacher`'s per-frame class distributions (opt-in; `distill_from(None)` clears it).
        Every training batch of epoch() then runs the teacher in eval mode on exactly the frames this model saw -- the same
        crop window, augmentation, flips and mixup blend, through `teacher._model.engine(teacher_dtype).forward_augmented`,
        with whatever weights that engine serves (the averaged ones inside `teacher.averaged()`) -- and minimises
            (1-alpha) ce + mse + alpha kd + displ_weight kd_displ,
        kd = temperature^2 * KL(softmax(t / temperature) || softmax(s / temperature)) averaged over the B*T frames and
        kd_displ = mean (d - d_teacher)^2 (ops.loss_kd: one launch for the value and the gradient).  epoch() still returns
        the mean of the total; `loss_parts` holds the means of ce, mse, kd and kd_displ.  Validation epochs never run the
        teacher, and the teacher takes no random draw.
        The settings and the teacher are not part of state_dict(): a reloaded model distils only after another call.
        ValueError: ranges (0 <= alpha <= 1, temperature > 0, displ_weight >= 0), the model as its own teacher, another
        num_classes or clip_len, the joint-dataset double head on either model, displ_weight > 0 unless both models have a
        displacement head; at the first batch, a teacher on another device.  Feature-map distillation is out of scope."""
        if teacher is None:
            self._kd, self._kd_last, self.loss_parts = None, None, None
            self._model._kd_wanted, self._model._kd_view = False, None
            return self
        alpha, temperature, displ_weight = ops.check_kd(alpha, temperature, displ_weight)
        if not isinstance(teacher, TDEEDModel):
            raise TypeError("distill_from: the teacher is a TDEEDModel")
        if teacher is self or teacher._model is self._model:
            raise ValueError("distill_from: the model cannot be its own teacher")
        if teacher_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"distill_from: teacher_dtype {teacher_dtype} (bfloat16 or float32)")
        ms, mt = self._model, teacher._model
        if ms._double_head or mt._double_head:
            raise ValueError("distill_from: the joint-dataset double head is not covered")
        if teacher._num_classes != self._num_classes:
            raise ValueError(f"distill_from: the teacher has {teacher._num_classes - 1} classes, the model {self._num_classes - 1}")
        if mt._cfg["clip_len"] != ms._cfg["clip_len"]:
            raise ValueError(f"distill_from: the teacher's clip_len {mt._cfg['clip_len']} != {ms._cfg['clip_len']}")
        if displ_weight > 0.0 and not (ms._radi_displacement > 0 and mt._radi_displacement > 0):
            raise ValueError("distill_from: displ_weight > 0 needs a displacement head on both models")
        self._kd = (teacher, teacher_dtype, dict(alpha=alpha, temperature=temperature, displ_weight=displ_weight))
        self._kd_last, self.loss_parts = None, None
        ms._kd_wanted = True
        return self

    def loss_options(self, label_smoothing=0.0, focal_gamma=0.0, class_weights=None):
        """Options of the classification loss of the training epochs (opt-in; all-neutral arguments clear them):
            ce = sum_r sum_c w_c t'_c (1 - p_c)^focal_gamma (-log p_c) / den,  t' = (1 - label_smoothing) t + label_smoothing / K1
        with t the one-hot label (or the mixup soft label, so mixup composes with smoothing) and den = sum_r w[y_r] (hard
        labels) or the number of frames (soft labels): focal_gamma = 0 is F.cross_entropy(weight=, label_smoothing=).
        class_weights: one finite non-negative weight per class, background first; it replaces the [1, fg_weight, ...]
        vector, so epoch()'s fg_weight is ignored in training epochs while it is set.  Value and gradient come from one
        launch (ops.loss_opt), with the distillation terms of distill_from() on top when a teacher is set.  epoch() still
        returns the mean of the total; `loss_parts` holds the means of ce and mse (and kd, kd_displ with a teacher).
        Validation epochs keep the plain loss, so that validation losses stay comparable across runs.
        The options are not part of state_dict().  ValueError: ranges (0 <= label_smoothing <= 1, focal_gamma >= 0 and
        finite), a class_weights vector of another length or with a negative / non-finite entry, the joint-dataset double
        head."""
        eps, gamma, cw = ops.check_loss_options(label_smoothing, focal_gamma, class_weights, self._num_classes)
        if eps == 0.0 and gamma == 0.0 and cw is None:
            self._loss_opt = None
            if self._kd is None:
                self.loss_parts = None
            return self
        if self._model._double_head:
            raise ValueError("loss_options: the joint-dataset double head is not covered")
        self._loss_opt = dict(label_smoothing=eps, focal_gamma=gamma, class_weights=cw)
        self.loss_parts = None
        return self

    def _teacher_head(self):
        """Run the teacher on the view of the train-mode forward that has just run, on the current stream -> (its head
        buffer (B*T, ld_t) fp32, kd settings for TemporalTrain.loss_fwd_bwd)."""
        teacher, dt, settings = self._kd
        ms, mt = self._model, teacher._model
        if ms._norm_device(mt._device) != ms._norm_device(ms._device):
            raise ValueError(f"distill_from: the teacher is on {mt._device}, the model on {ms._device}")
        view, flip_frames = ms._kd_view
        ms._kd_view = None
        teng = mt.engine(dt)
        thead, _ = teng.forward_augmented(view, flip_frames)
        thead = thead.view(view.shape[0] * view.shape[1], -1)
        self._kd_last = thead
        return thead, dict(settings, ld_t=thead.shape[1], displ_col_t=teng.pw.displ_col)

    @property
    def _train_dtype(self):
        return self._model._train_dtype

    @_train_dtype.setter
    def _train_dtype(self, dt):
        if self._model._train_engine is not None:
            raise RuntimeError("set _train_dtype before get_optimizer() / the first train-mode forward")
        self._model._train_dtype = dt

    def ema_state_dict(self):
        """The averaged model as a state_dict of clones: the optimizer's weight EMA, the averaged BatchNorm running statistics
        and the live step counters, with the model's keys in the model's order -- loadable by load() and by the reference.
        RuntimeError unless get_optimizer() was given 'ema_decay'."""
        te = self._model._train_engine
        if te is None or te.opt.ema is None:
            raise RuntimeError("ema_state_dict(): the optimizer has no EMA (get_optimizer({'ema_decay': ...}))")
        return {k: v.detach().clone() for k, v in te.ema_state().items()}

    @contextlib.contextmanager
    def averaged(self):
        """Context manager: inside it predict, predict_video / spot_video / *_group, evalutil.stitch_videos / spot_videos /
        map_videos and epoch(optimizer=None) run on inference engines built from the averaged weights
        (TrainEngine.ema_state()).  Those engines sit in a cache of their own and are rebuilt only when an optimizer step has
        happened since they were packed; the live engines, the packed training weights and every live tensor keep their
        bits.  epoch() with an optimizer, or a train-mode forward, inside the context is a RuntimeError, and so is
        averaged() on a model whose optimizer has no EMA."""
        te = self._model._train_engine
        if te is None or te.opt.ema is None:
            raise RuntimeError("averaged(): the optimizer has no EMA (get_optimizer({'ema_decay': ...}))")
        if self._model._averaged:
            raise RuntimeError("averaged() is already active")
        self._model._averaged = True
        try:
            yield self
        finally:
            self._model._averaged = False

    def _get_params(self):
        return list(self._model.parameters())

    def state_dict(self):
        return self._model.state_dict()

    def load(self, state_dict):
        self._model.load_state_dict(state_dict)

    def _ctx(self):
        if self._stream is None:
            from .streams import new_stream
            self._stream = new_stream()
        return torch.cuda.stream(self._stream)

    def predict(self, seq, use_amp=True, augment_inference=False):
        """model.py:334-369 -> (pred_cls (B,T) int64 numpy, scores (B,T,K+1) float32 numpy)."""
        if not isinstance(seq, torch.Tensor):
            seq = torch.as_tensor(np.asarray(seq))
        if seq.dim() == 4:
            seq = seq.unsqueeze(0)
        self._model.eval()
        dt = torch.bfloat16 if use_amp else torch.float32
        cur = torch.cuda.current_stream()
        with self._ctx():
            self._stream.wait_stream(cur)
            pred, _ = self._model(seq.to(self.device), inference=True, augment_inference=augment_inference,
                                  act_dtype=dt)
            B, T = seq.shape[:2]
            cls, scores = self._process_pred(pred, B, T, dt)
            self._stream.synchronize()
        return cls.cpu().numpy(), scores.cpu().numpy()

    def _score_cols(self, dt):
        """number of score columns predict() / predict_video() deliver for the current head layout"""
        pw = self._model.engine(dt).pw
        if self._model._radi_displacement > 0 and self._model._double_head:
            return self._args.num_classes + 1
        return pw.n_cls

    def _process_pred(self, pred, B, T, dt, out=None):
        """model.py:351-367 on what Impl.forward returned (displacement column, no displacement, double head): softmax +
        displacement scatter-max on the current stream -> (cls (B,T) int64, scores (B,T,K+1) fp32) on the device.
        out: where to write the scores."""
        if isinstance(pred, dict):
            head = pred["_head_out"].reshape(B * T, -1)
            pw = self._model.engine(dt).pw
            return ops.process_prediction(head, B, T, self._score_cols(dt), pw.displ_col, out=out)
        head = pred.reshape(B * T, -1).contiguous()
        return ops.process_prediction(head, B, T, head.shape[-1], -1, out=out)

    video_chunk_bytes = 64 << 20        # upload granularity of predict_video (one arrival event per chunk)

    def predict_video(self, frames, clip_starts=None, overlap_len=None, pad_len=5, batch_size=8, augment=False, use_amp=True,
                      max_resident_bytes=16 << 30, reuse_frames=False, stream_frames=False):
        """Score a whole video from one resident frame buffer: what the prediction loop of `evaluate` (util/eval.py:284-349)
        leaves in its per-video track, -> (scores_sum (L,K+1) float32, support (L,) int32) numpy, i.e.
        `ScoreStitcher.tracks[video]`.

        frames: uint8 (L,3,H,W) sampled frames (frame j = original frame j*stride), a host tensor (pinned or not) or a
        device tensor.  clip_starts: first sampled frame of every clip, in the order they are to be scored; default
        `evalutil.video_clip_starts(L, clip_len, overlap_len, pad_len=pad_len)` with overlap_len = clip_len // 4 * 3.
        Clips go through the forward in batches of `batch_size` in list order (the last one may be smaller, like a
        DataLoader's); augment=True scores every batch a second time horizontally flipped.

        Host frames are uploaded ONCE, in chunks of `video_chunk_bytes` on a copy stream; a batch waits only for the chunk
        that holds its last frame.  Clip windows are gathered on the device into the engine's input buffers, consecutive
        batches alternate over two engine slots / streams like epoch()'s validation loop, the clip scores stay on the
        device and one stitch launch (ops.stitch_scores_seg) adds them per frame in ScoreStitcher's order.  Apart from the
        warm-up of a geometry seen for the first time (graph capture) the host synchronises once per video.
        Raises ValueError when the video does not fit `max_resident_bytes`.

        stream_frames=True: host frames that do not fit `max_resident_bytes` are scored through a RING of upload chunks
        instead (`feeder.RingUpload`, `evalutil.ring_plan`): the device holds max_resident_bytes // chunk bytes chunks, chunk
        c in slot c mod that count, and a chunk is copied over an older one once the batches that read the older one have
        run (stream events, no host synchronisation).  Every frame still crosses the link once, the batches, graphs and
        the stitch launch are the same and so are the bits of the result.  The clips must come in ascending order and one
        batch plus one chunk must fit the ring (ValueError otherwise, naming the budget that would do).  last_video_stats
        gains ring_frames, ring_chunks and resident_bytes.  Frames that fit take the resident route untouched; a video
        that is a device tensor already is used where it is; together with reuse_frames it works only when frames and
        maps fit (ValueError otherwise: the maps have no ring).

        reuse_frames=True: the trunk stages in front of the first gate-shift site (stem and blocks [0, k), k =
        `ForwardEngine.first_site_block()`; functions of one frame alone in eval mode) run ONCE per frame and view, in chunks
        of `frame_batch` clips' worth of consecutive frames, into a resident map of the block-k inputs; a batch gathers its
        windows from that map (ops.rows_gather_seg, the row of a black frame as padding) and runs only the rest of the network
        (`ForwardEngine.forward_from_frame_maps`).  The maps count towards `max_resident_bytes`; last_video_stats gains
        frame_pass_frames (views x rows of the map) and map_bytes.  The launches are those of the engine's join_at = k
        plan: same scores bit for bit where that plan would have served the batch (an even batch size), the first site's
        launch form otherwise."""
        out = self._predict_videos("predict_video", [frames], None if clip_starts is None else [clip_starts], overlap_len, pad_len,
                                   batch_size, augment, use_amp, max_resident_bytes, reuse_frames, stream_frames)
        self._one_video_stats()
        return out[0]

    def live_scorer(self, frame_shape, overlap_len=None, pad_len=5, batch_size=1, augment=False, use_amp=True, ring_frames=None):
        """Score a video whose length is not known yet -- a camera, a feed, a file still being written: -> `live.LiveScorer`.
        Frames are pushed as they arrive and the FINAL rows of predict_video's track come back.

        The clip grid start_j = -pad_len + j * (clip_len - overlap_len) does not depend on the length, so a clip is scored
        the moment its last frame has arrived, and a row is final once the next clip to be scored starts after it
        (`liveplan`).  Batches of `batch_size` clips run only when full while the stream is open and close() cuts the rest
        the same way: they are predict_video's batches, so for ANY split of a video into pushes the concatenated sums and
        support equal predict_video(frames, overlap_len=, pad_len=, batch_size=, augment=, use_amp=) bit for bit, and the
        mean equals ops.stitch_scores(..., mean=True)'s.  Custom clip starts are not offered: the closed-form grid is what
        makes rows final.  frame_shape: (3,H,W) of the sampled frames.

        push(frames): uint8 (m,3,H,W), m >= 1, a host tensor (pinned or pageable) or a device tensor; the caller's buffer is
        free when push returns (host frames are staged into pinned memory of the scorer's own, `video_chunk_bytes` at a time,
        and go up on the copy stream into a ring of `ring_frames` rows, frame p in row p % ring_frames; a row is overwritten
        only behind the event of the last batch that read it).  Every complete batch runs as a batch of predict_video does
        (ring gather, both views when augment, post-processing, alternating engine slots) and ops.stitch_live follows on
        its stream: it adds the batch onto a score ring of liveplan.track_ring_rows(batch_size) rows and writes out the rows
        that became final.  -> (first_row, sums (r,K+1) float32, support (r,) int32, mean (r,K+1) float32) numpy, rows
        consecutive across calls, r may be 0.  A push that completes no batch does not synchronise the host, one that does
        synchronises once, at its end; last_push_stats (host_syncs, batches, rows, frames_h2d_bytes) tells which.
        close(): runs the remaining clips, their windows cut at the length, and returns all remaining rows; afterwards push
        raises RuntimeError.  reset(): a new stream on the same buffers and graphs.  frames_pushed, rows_final,
        latency_frames = clip_len - 1 + (batch_size - 1) * (clip_len - overlap_len): a frame's row comes back at most that
        many frames after it.

        Raises before any launch: TypeError / ValueError for a wrong dtype, rank or geometry, ValueError for ring_frames
        below liveplan.frame_ring_rows (naming the minimum), and close() raises predict_video's ValueError for a stream
        without frames or without clips.  Suppression is left to the caller (ops.nms_track on the complete track): no prefix
        of its output is final."""
        from .live import LiveScorer
        return LiveScorer(self, frame_shape, overlap_len, pad_len, batch_size, augment, use_amp, ring_frames)

    def spot_video(self, frames, classes, suppress=(("nms", 1, 0.01), ("snms", 3, 0.01)), high_recall_score_threshold=0.01,
                   clip_starts=None, overlap_len=None, pad_len=5, batch_size=8, augment=False, use_amp=True,
                   max_resident_bytes=16 << 30, reuse_frames=False, stream_frames=False):
        """Score a whole video like predict_video and spot its events on the device: the tail of `evaluate`
        (util/eval.py:87-261, 386-391) -- `frame_events` and (soft) non-maximum suppression of the high-recall list -- without
        the (L,K+1) track ever leaving the device.  classes: name -> index (1-based); suppress: entries (kind, window,
        threshold), kind "nms" | "snms", window an int or a list indexed by label appearance like the reference's (defaults:
        the reference's thresholds with WINDOWS['default']); the other keyword arguments are predict_video's.
        -> dict(pred (L,) int32 numpy: arg-max class per frame; events: the arg-max events; suppressed: one event list per
        entry of suppress), events being the reference's dicts {'label','frame','score'}, equal to what
        `evalutil.frame_events` / `non_maximum_suppression` / `soft_non_maximum_suppression` give on the normalised track.
        The host synchronises twice: once for pred, pred_score and the event counts, once for the first `count` entries of
        every event list.  Class indices travel as one byte (pred: 1 + 4 bytes per frame with its score; an event: frame
        int32, class uint8, score float64 = 13 bytes), which limits K+1 to 256 columns here.  last_video_stats gains events_d2h_bytes and nms_rounds (per suppress entry, the maximum over
        the classes)."""
        out = self._spot_videos("spot_video", [frames], classes, suppress, high_recall_score_threshold,
                                None if clip_starts is None else [clip_starts], overlap_len, pad_len, batch_size, augment, use_amp,
                                max_resident_bytes, reuse_frames, stream_frames)
        self._one_video_stats()
        return out[0]

    def _one_video_stats(self):
        """last_video_stats of the one-video methods: the group's keys without the group's own (videos, host_syncs)"""
        self.last_video_stats = {k: v for k, v in self.last_video_stats.items() if k not in ("videos", "host_syncs")}

    def predict_video_group(self, frames_list, clip_starts=None, overlap_len=None, pad_len=5, batch_size=8, augment=False,
                            use_amp=True, max_resident_bytes=16 << 30, reuse_frames=False, stream_frames=False):
        """predict_video for a group of videos scored as one packed job -> [(scores_sum (L_v,K+1) float32, support (L_v,)
        int32)], per video what predict_video returns for the same batches.

        frames_list: uint8 (L_v,3,H,W) tensors of one geometry, host (pinned or pageable) or device; clip_starts: optional
        list of one start list per video.  Every frame is uploaded once into one packed buffer (video v from frame
        seg_off[v] on, `evalutil.group_clip_table`), in `video_chunk_bytes` chunks on the copy stream; the clips of all
        videos form one list, video-major, and batches of `batch_size` are cut from it ACROSS the videos, so only the
        group's last batch may be short (short videos fill whole batches together); a batch waits only for the chunk with
        the last packed frame one of its clips reads.  All clip scores go into one (V,n,T,K+1) buffer and one segmented
        stitch launch (ops.stitch_scores_seg) adds them per frame in ScoreStitcher's order for that frame's video.  Apart
        from the warm-up of a geometry seen for the first time the host synchronises once per group.
        last_video_stats: predict_video's keys as totals over the group, plus videos and host_syncs.
        Raises ValueError for an empty list, an empty video, mixed geometries or a group over `max_resident_bytes`;
        stream_frames=True scores a group of host videos over the budget through predict_video's frame ring instead."""
        return self._predict_videos("predict_video_group", list(frames_list), clip_starts, overlap_len, pad_len, batch_size,
                                    augment, use_amp, max_resident_bytes, reuse_frames, stream_frames)

    def _predict_videos(self, who, frames_list, clip_starts, overlap_len, pad_len, batch_size, augment, use_amp,
                        max_resident_bytes, reuse_frames, stream_frames=False):
        """predict_video_group under the name `who` (the prefix of its errors): predict_video is the group of one video."""
        track, support, _, s0, stats, keep, g = self._packed_track(who, frames_list, clip_starts, overlap_len, pad_len, batch_size,
                                                                   augment, use_amp, max_resident_bytes, want_mean=False,
                                                                   reuse_frames=reuse_frames, stream_frames=stream_frames)
        L, K1 = track.shape
        with torch.cuda.stream(s0):
            out_sum = torch.empty((L, K1), dtype=torch.float32).pin_memory()
            out_sup = torch.empty((L,), dtype=torch.int32).pin_memory()
            out_sum.copy_(track, non_blocking=True)
            out_sup.copy_(support, non_blocking=True)
            s0.synchronize()
        del keep
        stats["host_syncs"] = 1
        self.last_video_stats = stats
        sums, sup, off = out_sum.numpy(), out_sup.numpy(), g.seg_off
        return [(sums[off[v]:off[v + 1]].copy(), sup[off[v]:off[v + 1]].copy()) for v in range(g.nv)]

    def spot_video_group(self, frames_list, classes, suppress=(("nms", 1, 0.01), ("snms", 3, 0.01)),
                         high_recall_score_threshold=0.01, clip_starts=None, overlap_len=None, pad_len=5, batch_size=8,
                         augment=False, use_amp=True, max_resident_bytes=16 << 30, reuse_frames=False, stream_frames=False):
        """spot_video for a group of videos scored as one packed job (predict_video_group's pipeline) -> one spot_video
        dict per video.  On the packed track: one segmented event launch (ops.frame_events_seg), one suppression launch per
        entry of `suppress` with a workgroup per (class, video) (ops.nms_track_seg), whose compaction leaves the videos' event
        lists one after the other in video order.  The host synchronises twice per group: once for pred bytes, their scores,
        the event offsets and the rounds, once for one contiguous range of events per entry (skipped when nothing was
        kept).  last_video_stats: totals over the group; nms_rounds per entry is the maximum over videos and classes."""
        return self._spot_videos("spot_video_group", list(frames_list), classes, suppress, high_recall_score_threshold,
                                 clip_starts, overlap_len, pad_len, batch_size, augment, use_amp, max_resident_bytes, reuse_frames,
                                 stream_frames)

    def _spot_videos(self, who, frames_list, classes, suppress, high_recall_score_threshold, clip_starts, overlap_len, pad_len,
                     batch_size, augment, use_amp, max_resident_bytes, reuse_frames, stream_frames=False):
        """spot_video_group under the name `who` (the prefix of its errors): spot_video is the group of one video."""
        from . import evalutil
        suppress = [tuple(e) for e in suppress]
        for kind, window, _ in suppress:
            if kind not in ("nms", "snms"):
                raise ValueError(f"{who}: suppression kind {kind!r} (nms | snms)")
        inv = {v: k for k, v in classes.items()}
        K1 = self._score_cols(torch.bfloat16 if use_amp else torch.float32)
        if K1 > 256:
            raise ValueError(f"{who}: {K1} score columns, at most 256")
        if sorted(inv) != list(range(1, K1)):
            raise ValueError(f"{who}: classes must name the indices 1..{K1 - 1} of the model's score columns")
        track, _, mean, s0, stats, keep, g = self._packed_track(who, frames_list, clip_starts, overlap_len, pad_len, batch_size,
                                                                augment, use_amp, max_resident_bytes, want_mean=True,
                                                                reuse_frames=reuse_frames, stream_frames=stream_frames)
        L, nv = track.shape[0], g.nv
        hr = float(high_recall_score_threshold)
        n = len(suppress)
        with torch.cuda.stream(s0):
            pred8 = torch.empty((L,), dtype=torch.uint8, device=mean.device)
            _, pred_score, first, _ = ops.frame_events_seg(mean, g.seg_off_dev, g.max_len, hr, pred_u8=pred8,
                                                           first_init=g.first_init)
            lists = [ops.nms_track_seg(mean, g.seg_off_dev, g.max_len, window, thr, kind == "snms", first, hr)
                     for kind, window, thr in suppress]
            h_pred = torch.empty((L,), dtype=torch.uint8).pin_memory()
            h_score = torch.empty((L,), dtype=torch.float32).pin_memory()
            # per entry the ends of the videos' event lists (event_off[1:]; event_off[0] is 0) and the rounds
            h_small = torch.empty((n, nv + nv * K1), dtype=torch.int32).pin_memory()
            h_pred.copy_(pred8, non_blocking=True)
            h_score.copy_(pred_score, non_blocking=True)
            for i, (_, _, _, event_off, rounds) in enumerate(lists):
                h_small[i, :nv].copy_(event_off[1:], non_blocking=True)
                h_small[i, nv:].copy_(rounds.view(-1), non_blocking=True)
            s0.synchronize()
            syncs = 1
            small = h_small.numpy()
            ends = [[0] + small[i, :nv].tolist() for i in range(n)]
            totals = [e[-1] for e in ends]
            host = []
            for (fr, c8, sc, _, _), m in zip(lists, totals):
                bufs = (torch.empty((m,), dtype=torch.int32).pin_memory(), torch.empty((m,), dtype=torch.uint8).pin_memory(),
                        torch.empty((m,), dtype=torch.float64).pin_memory())
                if m:
                    for dst, src in zip(bufs, (fr, c8, sc)):
                        dst.copy_(src[:m], non_blocking=True)
                host.append(tuple(b.numpy() for b in bufs))
            if any(totals):
                s0.synchronize()
                syncs += 1
        del keep
        pred_all = h_pred.numpy().astype(np.int32)
        score_all = h_score.numpy()
        out = []
        for v in range(nv):
            a, b = int(g.seg_off[v]), int(g.seg_off[v + 1])
            pred_np, score_np = pred_all[a:b].copy(), score_all[a:b]
            fg = np.nonzero(pred_np != 0)[0]
            events = [{"label": inv[int(pred_np[i])], "frame": int(i), "score": float(score_np[i])} for i in fg]
            suppressed = []
            for (f, c, s_), e in zip(host, ends):
                suppressed.append(evalutil.event_dicts(f[e[v]:e[v + 1]], c[e[v]:e[v + 1]], s_[e[v]:e[v + 1]], inv))
            out.append(dict(pred=pred_np, events=events, suppressed=suppressed))
        stats["events_d2h_bytes"] = L * 5 + n * (nv + nv * K1) * 4 + 13 * sum(totals)
        stats["nms_rounds"] = [int(small[i, nv:].max()) for i in range(n)]
        stats["host_syncs"] = syncs
        self.last_video_stats = stats
        return out

    def map_video_group(self, frames_list, classes, state, ordinals, suppress=(("nms", 1, 0.01), ("snms", 3, 0.01)),
                        high_recall_score_threshold=0.01, clip_starts=None, overlap_len=None, pad_len=5, batch_size=8,
                        augment=False, use_amp=True, max_resident_bytes=16 << 30, reuse_frames=False, stream_frames=False,
                        labels=None, frame_stats=None):
        """spot_video_group's pipeline for a mAP pass (evalutil.map_videos): the group is scored as one packed job, then on the
        packed track one event launch, per entry of `suppress` its suppression launch (none for ("raw",), the unsuppressed
        high-recall list) and the segment + match launch (ops.ap_match_seg), which leaves the group's ordered predictions and
        hits in `state` (ops.ap_state, one per dataset, as many entries as `suppress`).  ordinals: per video its index among
        the dataset's sorted names.  Nothing is copied to the host -- no pred, no event list; the host synchronises once, so
        that the resident buffers outlive the stream work.  Returns state.  last_video_stats: the group's totals, host_syncs
        1, ap_d2h_bytes 0.
        labels (per video of the group an (L,) integer array, the ground-truth class of every frame) and frame_stats (the int64
        (2 + 3*(K+1),) device tensor of ops.frame_stats_seg) go together: one more launch on the packed track adds the
        group's frame error / foreground-F1 counters to frame_stats.  A length that differs from the video's or a value
        outside 0..K raises ValueError before any launch."""
        who = "map_video_group"
        from . import evalutil
        frames_list = list(frames_list)
        suppress = evalutil.map_suppress_entries(suppress, who)
        if not isinstance(state, ops.ApState):
            raise TypeError(f"{who}: state must come from ops.ap_state")
        K1 = self._score_cols(torch.bfloat16 if use_amp else torch.float32)
        if K1 > 256:
            raise ValueError(f"{who}: {K1} score columns, at most 256")
        if sorted(classes.values()) != list(range(1, K1)):
            raise ValueError(f"{who}: classes must name the indices 1..{K1 - 1} of the model's score columns")
        ordinals = [int(o) for o in ordinals]
        if state.K1 != K1 or state.E != len(suppress):
            raise ValueError(f"{who}: a state of {state.K1} columns and {state.E} entries for {K1} columns and {len(suppress)} entries")
        if len(ordinals) != len(frames_list) or len(set(ordinals)) != len(ordinals) \
                or any(not 0 <= o < state.NV or state.lengths[o] != int(fr.shape[0]) for o, fr in zip(ordinals, frames_list)):
            raise ValueError(f"{who}: ordinals {ordinals} do not name {len(frames_list)} videos of the state's dataset by length")
        h_labels = None
        if (labels is None) != (frame_stats is None):
            raise ValueError(f"{who}: labels and frame_stats go together")
        if labels is not None:
            labels = list(labels)
            if len(labels) != len(frames_list):
                raise ValueError(f"{who}: {len(labels)} label tracks for {len(frames_list)} videos")
            packed = evalutil.check_labels(labels, [int(fr.shape[0]) for fr in frames_list], K1, who)
            if not isinstance(frame_stats, torch.Tensor) or frame_stats.dtype != torch.int64 or not frame_stats.is_cuda \
                    or tuple(frame_stats.shape) != (ops.frame_stats_size(K1),):
                raise ValueError(f"{who}: frame_stats must be an int64 ({ops.frame_stats_size(K1)},) device tensor")
            h_labels = torch.from_numpy(np.concatenate(packed)).pin_memory()
        _, _, mean, s0, stats, keep, g = self._packed_track(who, frames_list, clip_starts, overlap_len, pad_len, batch_size,
                                                            augment, use_amp, max_resident_bytes, want_mean=True,
                                                            reuse_frames=reuse_frames, stream_frames=stream_frames)
        hr = float(high_recall_score_threshold)
        h_ords = torch.tensor(ordinals, dtype=torch.int32).pin_memory()
        with torch.cuda.stream(s0):
            ords = torch.empty((g.nv,), dtype=torch.int32, device=mean.device)
            ords.copy_(h_ords, non_blocking=True)
            first = None
            for i, e in enumerate(suppress):
                planes = None
                if e[0] != "raw":
                    if first is None:
                        first = ops.frame_events_seg(mean, g.seg_off_dev, g.max_len, hr, first_init=g.first_init)[2]
                    planes = ops.nms_track_seg(mean, g.seg_off_dev, g.max_len, e[1], e[2], e[0] == "snms", first, hr,
                                               planes=True)[5:]
                ops.ap_match_seg(state, i, mean, g.seg_off_dev, ords, g.max_len, hr, planes=planes)
            if h_labels is not None:
                lab = torch.empty((mean.shape[0],), dtype=torch.uint8, device=mean.device)
                lab.copy_(h_labels, non_blocking=True)
                ops.frame_stats_seg(mean, lab, frame_stats)
            s0.synchronize()
        del keep, h_ords, h_labels
        stats["host_syncs"] = 1
        stats["ap_d2h_bytes"] = 0
        self.last_video_stats = stats
        return state

    def map_finish(self, state, frame_stats=None):
        """The end of a mAP pass: rank + AP over everything the groups left in `state` (ops.ap_rank), then the one copy of the
        pass: -> (ap float64 (entries, tolerances, K+1), hits int32 of that shape) numpy.  One host synchronisation;
        last_video_stats: host_syncs 1 and ap_d2h_bytes, 12 bytes per (entry, tolerance, column) whatever the events.
        frame_stats: the counter tensor the groups accumulated (map_video_group(labels=...)); it rides in the same copy and
        follows as a third entry (int64 numpy), 8 more bytes per counter in ap_d2h_bytes."""
        if not isinstance(state, ops.ApState):
            raise TypeError("map_finish: state must come from ops.ap_state")
        from .streams import new_stream
        if self._stream is None:
            self._stream = new_stream()
        s0 = self._stream
        s0.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s0):
            ap, nhits, _ = ops.ap_rank(state)
            h_ap = torch.empty(ap.shape, dtype=torch.float64).pin_memory()
            h_n = torch.empty(nhits.shape, dtype=torch.int32).pin_memory()
            h_ap.copy_(ap, non_blocking=True)
            h_n.copy_(nhits, non_blocking=True)
            if frame_stats is not None:
                h_fs = torch.empty(frame_stats.shape, dtype=torch.int64).pin_memory()
                h_fs.copy_(frame_stats, non_blocking=True)
            s0.synchronize()
        self.last_video_stats = dict(host_syncs=1, ap_d2h_bytes=ap.numel() * 12)
        if frame_stats is not None:
            self.last_video_stats["ap_d2h_bytes"] += frame_stats.numel() * 8
            return h_ap.numpy().copy(), h_n.numpy().copy(), h_fs.numpy().copy()
        return h_ap.numpy().copy(), h_n.numpy().copy()

    frame_batch = 2                     # clips' worth of frames per launch of the per-frame pass (reuse_frames=True)

    def _packed_track(self, who, frames_list, clip_starts, overlap_len, pad_len, batch_size, augment, use_amp,
                      max_resident_bytes, want_mean, reuse_frames=False, stream_frames=False):
        """A group of videos (one video: a group of one) through upload, batches and the stitch launch, nothing synchronised.
        The videos are packed one after the other into one resident buffer -- a single video that is on the device already
        is used where it is -- and one clip list (evalutil.group_clip_table, clip_starts one list per video), batches are
        cut from that list across the videos, the gathers and the stitch are the segmented kernels.  -> (track (sum L,K+1)
        fp32, support (sum L,) int32, mean (sum L,K+1) fp32 | None: device tensors over the packed frames, written on stream
        s0; s0; the last_video_stats dict; the resident buffers, to be kept alive until s0 has been synchronised; a
        namespace of the group's tables).  who: the public method, the prefix of the errors.
        reuse_frames: the per-frame trunk stages run once per (packed) frame and view into a resident map, chunk by chunk on a
        stream of their own with an event per chunk -- the chunk with the first black row (the padding of every window)
        first, then in frame order; a batch waits for the chunk that holds its last frame and runs the rest of the network
        on rows gathered from the map.
        stream_frames: host frames over the budget go through feeder.RingUpload instead of PackedUpload -- the same chunks
        into a ring of them, per evalutil.ring_plan -- and the batches gather with ops.clip_gather_ring; a batch records its
        release on its stream, the upload waits for the releases of a slot's last readers before it overwrites the slot."""
        from types import SimpleNamespace
        from . import evalutil
        from .streams import new_stream
        srcs = []
        for fr in frames_list:
            if not isinstance(fr, torch.Tensor):
                fr = torch.as_tensor(np.asarray(fr))
            if fr.dtype != torch.uint8 or fr.dim() != 4:
                raise TypeError(f"{who}: frames must be a uint8 (L,3,H,W) tensor")
            srcs.append(fr)
        if not srcs:
            raise ValueError(f"{who}: no videos")
        lengths = [int(fr.shape[0]) for fr in srcs]
        if min(lengths) == 0:
            raise ValueError(f"{who}: empty video")
        shape = tuple(srcs[0].shape[1:])
        if any(tuple(fr.shape[1:]) != shape for fr in srcs):
            raise ValueError(f"{who}: the videos of one group share one frame geometry, got "
                             f"{sorted({tuple(fr.shape[1:]) for fr in srcs})}")
        nv, L = len(srcs), sum(lengths)
        fb = int(srcs[0][0].numel())
        if nv > ops.MAX_GROUP_VIDEOS:
            raise ValueError(f"{who}: {nv} videos in one group, at most {ops.MAX_GROUP_VIDEOS}")
        what = "group" if who.endswith("_group") else "video"
        # over the budget: only host frames can stream through a ring (a device tensor is where it is)
        over = L * fb > max_resident_bytes
        if over and not (stream_frames and not any(fr.is_cuda for fr in srcs)):
            raise ValueError(f"{who}: the {what} needs {L * fb} bytes on the device, more than "
                             f"max_resident_bytes={max_resident_bytes} (stream_frames=True scores host frames over the "
                             "budget through a frame ring)")
        T = self._args.clip_len
        ov = T // 4 * 3 if overlap_len is None else int(overlap_len)
        seg_off, clip_off, starts_np, base_np, lenv_np = evalutil.group_clip_table(lengths, T, ov, pad_len, clip_starts)
        starts, base, len_v = starts_np.tolist(), base_np.tolist(), lenv_np.tolist()
        n = len(starts)
        if batch_size < 1:
            raise ValueError(f"{who}: batch_size must be positive")
        # last packed frame a clip reads (-1: none before the front of its video)
        last_of = [b + min(lv - 1, s_ + T - 1) if s_ + T - 1 >= 0 else -1 for s_, b, lv in zip(starts, base, len_v)]
        V = 2 if augment else 1
        self._model.eval()
        dt = torch.bfloat16 if use_amp else torch.float32
        eng = self._model.engine(dt)
        pw = eng.pw
        K1 = self._score_cols(dt)
        dev = self.device
        if reuse_frames:
            Bf = int(self.frame_batch)
            mh, mw, mc = eng.frame_map_shape(*shape[1:])
            rows, pad_row, chunk = evalutil.frame_map_rows(L, T, Bf)
            map_bytes = V * rows * mh * mw * mc * (2 if dt == torch.bfloat16 else 4)
            if L * fb + map_bytes > max_resident_bytes:
                if stream_frames:
                    raise ValueError(f"{who}: stream_frames=True and reuse_frames=True are not combined yet: the {what} needs "
                                     f"{L * fb + map_bytes} bytes on the device ({map_bytes} of them per-frame maps, which "
                                     f"have no ring), more than max_resident_bytes={max_resident_bytes}")
                raise ValueError(f"{who}: the {what} needs {L * fb + map_bytes} bytes on the device "
                                 f"({map_bytes} of them per-frame maps), more than max_resident_bytes={max_resident_bytes} "
                                 "(the maps have no ring: stream_frames=True streams frames only)")
        ring = None
        if over:
            try:
                ring = evalutil.ring_plan(lengths, fb, max(1, int(self.video_chunk_bytes) // fb), max_resident_bytes, starts_np,
                                          base_np, lenv_np, T, batch_size)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from None
        if self._stream is None:
            self._stream = new_stream()
        if getattr(self, "_stream2", None) is None:
            self._stream2 = new_stream(avoid=[self._stream])
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = new_stream(avoid=[self._stream, self._stream2])
        streams, cp = [self._stream, self._stream2], self._copy_stream
        cur = torch.cuda.current_stream()
        for st in streams + [cp]:
            st.wait_stream(cur)
        if reuse_frames:
            if getattr(self, "_frame_stream", None) is None:
                self._frame_stream = new_stream(avoid=[self._stream, self._stream2, self._copy_stream])
            self._frame_stream.wait_stream(cur)
        # ---- the resident buffers (kept alive until the one synchronisation at the end); the tables travel in one copy
        first_init = np.repeat(np.asarray(lengths, np.int32), K1)
        parts = [starts_np, base_np, lenv_np, seg_off, clip_off, first_init]
        tab_host = torch.from_numpy(np.concatenate(parts)).pin_memory()
        tab_dev = torch.empty((tab_host.numel(),), dtype=torch.int32, device=dev)
        clip_scores = torch.empty((V, n, T, K1), dtype=torch.float32, device=dev)
        with torch.cuda.stream(cp):
            tab_dev.copy_(tab_host, non_blocking=True)
            ev_starts = torch.cuda.Event()
            ev_starts.record(cp)
        cuts = np.cumsum([0] + [len(x) for x in parts]).tolist()
        starts_dev, base_dev, lenv_dev, seg_dev, coff_dev, first_dev = (tab_dev[cuts[i]:cuts[i + 1]] for i in range(6))
        g = SimpleNamespace(nv=nv, lengths=lengths, seg_off=seg_off, max_len=max(lengths), seg_off_dev=seg_dev,
                            first_init=first_dev.view(nv, K1), K1=K1)
        srcs = [fr.contiguous() if not fr.is_cuda else fr.to(dev).contiguous() for fr in srcs]
        packed = nv > 1 or not srcs[0].is_cuda
        up = None
        if packed:
            # one buffer for all frames, filled in chunks of video_chunk_bytes on the copy stream (a chunk may span videos)
            from . import feeder
            if ring is not None:
                # over the budget: the same chunks into a ring of them; a chunk is queued when a batch asks for it, behind
                # the release events of the batches that read the chunk it overwrites (never all at once)
                up = feeder.RingUpload(srcs, dev, cp, self.video_chunk_bytes, ring.ring_chunks, ring.last_reader)
            else:
                up = feeder.PackedUpload(srcs, dev, cp, self.video_chunk_bytes)
            video, per, arrived = up.video, up.per, up.arrived
            if ring is None and up.asynchronous:
                up.all()                              # asynchronous copies: queue all frames behind the first chunk
        else:
            video = srcs[0]
        # ---- the per-frame pass (reuse_frames): chunk fc covers the rows [fc * chunk, (fc + 1) * chunk) of every view's map
        maps = None
        if reuse_frames:
            maps = torch.empty((V, rows, mh, mw, mc), dtype=dt, device=dev)
            n_chunks = rows // chunk
            order = [n_chunks - 1] + list(range(n_chunks - 1))          # the chunk of pad_row first: every padded window reads it
            pos = {fc: i for i, fc in enumerate(order)}
            map_ready = {}

            def frame_pass_through(fc_need):
                while len(map_ready) <= pos[fc_need]:
                    fc = order[len(map_ready)]
                    need = ev_starts
                    last = min((fc + 1) * chunk, L) - 1
                    if packed and last >= fc * chunk:
                        c = last // per
                        up.through(c + 1)
                        need = arrived[c]
                    with torch.cuda.stream(self._frame_stream):
                        self._frame_stream.wait_event(need)
                        for v in range(V):
                            eng.frame_maps(video, fc * chunk, maps[v, fc * chunk:(fc + 1) * chunk], Bf, flip=bool(v))
                        ev = torch.cuda.Event()
                        ev.record(self._frame_stream)
                    map_ready[fc] = ev
        # ---- the batches: gather -> forward -> post-processing, two in flight
        n_batches = 0
        ring_arg = None if ring is None else (ring.ring_frames, L)
        for bi, lo in enumerate(range(0, n, batch_size)):
            B = min(batch_size, n - lo)
            slot = bi % 2
            st = streams[slot]
            need = ev_starts
            if reuse_frames:
                # (every chunk's event follows the first one's -- the chunk of pad_row -- on the frame stream, and the tables')
                last = max(last_of[lo:lo + B])
                fc = last // chunk if last >= 0 else order[0]
                if last >= 0 and fc == order[0]:
                    fc = order[-1]                    # frames of pad_row's own chunk: the chunks in front of it run behind it
                frame_pass_through(fc)
                need = map_ready[fc]
            elif packed:
                last = max(last_of[lo:lo + B])
                if last >= 0:
                    c = last // per
                    up.through(c + 1)                 # pageable frames: the copy call stages on the host, keep one chunk ahead
                    need = arrived[c]
            with torch.cuda.stream(st):
                st.wait_event(need)                   # a chunk's event follows the tables' on the copy stream
                tables = dict(clip_base=base_dev[lo:lo + B], clip_len_v=lenv_dev[lo:lo + B])
                for v in range(V):
                    if reuse_frames:
                        head, _ = eng.forward_from_frame_maps(maps[v], starts_dev[lo:lo + B], pad_row, slot=slot, **tables)
                    else:
                        head, _ = eng.forward_from_video(video, starts_dev[lo:lo + B], augment_inference=bool(v), slot=slot,
                                                         ring=ring_arg, **tables)
                    pred, _ = self._model._pack_head(head, B, T, pw.n_cls, pw.displ_col, None)
                    # head is a view of the slot's buffer: consumed here, on the launching stream, before the slot runs again
                    self._process_pred(pred, B, T, dt, out=clip_scores[v, lo:lo + B])
                if ring is not None:
                    up.release(bi, st)                # the last gather of this batch is behind: its chunks may be overwritten
            n_batches += 1
        # ---- one stitch launch
        s0 = streams[0]
        s0.wait_stream(streams[1])
        s0.wait_stream(cp)
        if reuse_frames:
            frame_pass_through(order[-1])             # (rows nobody read: the count of the stats holds, and nothing is left unqueued)
            s0.wait_stream(self._frame_stream)
        with torch.cuda.stream(s0):
            track, support, mean = ops.stitch_scores_seg(clip_scores, starts_dev, seg_dev, coff_dev, L, count_all=augment,
                                                         mean=want_mean)
        stats = dict(frames=L, clips=n, batches=n_batches, views=V, frames_h2d_bytes=up.h2d if up is not None else 0, videos=nv)
        if reuse_frames:
            stats["frame_pass_frames"] = V * rows
            stats["map_bytes"] = map_bytes
        if ring is not None:
            stats.update(ring_frames=ring.ring_frames, ring_chunks=ring.ring_chunks, resident_bytes=ring.ring_frames * fb)
        return track, support, mean, s0, stats, (video, srcs, clip_scores, tab_dev, tab_host, maps), g

    def epoch(self, loader, optimizer=None, scaler=None, lr_scheduler=None, acc_grad_iter=1, fg_weight=5,
              valMAP=False):
        """model.py:193-332: validation pass (optimizer None) or one training epoch (optimizer from get_optimizer)."""
        if optimizer is not None:
            if self._model._averaged:
                raise RuntimeError("epoch() with an optimizer inside averaged(): the averaged weights are for scoring only")
            return self._train_epoch(loader, optimizer, lr_scheduler, acc_grad_iter, fg_weight)
        self._model.eval()
        K1 = self._num_classes
        w = torch.tensor([1.0] + [float(fg_weight)] * (K1 - 1), dtype=torch.float32, device=self.device)
        map_labels, map_preds = [], []
        n = 0
        # two batches in flight: consecutive batches alternate between two buffer sets / HIP graphs on two streams
        from .streams import new_stream
        if self._stream is None:
            self._stream = new_stream()
        if getattr(self, "_stream2", None) is None:
            self._stream2 = new_stream(avoid=[self._stream])
        streams = [self._stream, self._stream2]
        totals = [torch.zeros((), dtype=torch.float32, device=self.device) for _ in streams]
        torch.cuda.current_stream().synchronize()     # w / totals were filled on the current stream; the two are non-blocking
        from . import feeder
        for i, batch in enumerate(feeder.prefetch(loader, self.device, auto=False)):
            slot = i % 2
            with torch.cuda.stream(streams[slot]):
                feeder.wait(batch)                     # uint8 frames: pinned staging ring + copy stream, one batch ahead
                frame = batch["frame"].to(self.device)
                label = batch["label"].to(self.device)
                B, T = frame.shape[:2]
                pred, _ = self._model(frame, y=label, inference=True, slot=slot)
                labelD = batch["labelD"].to(self.device).float().reshape(-1).contiguous() if "labelD" in batch else None
                if isinstance(pred, dict):
                    head = pred["_head_out"].reshape(B * T, -1)
                    dcol = self._model.engine(torch.bfloat16).pw.displ_col if labelD is not None else -1
                else:
                    head, dcol = pred.reshape(B * T, -1).contiguous(), -1
                if self._model._double_head:
                    # joint-dataset validation (model.py:278-306): per-clip CE on the clip's own head
                    k1a, k1b = self._model._head_classes
                    ds = torch.as_tensor(batch["dataset"]).to(self.device).long()
                    lab2 = update_labels_2heads(label.clone(), ds, self._args.num_classes).reshape(-1).contiguous()
                    w2 = torch.tensor([1.0] + [float(fg_weight)] * (max(k1a, k1b) - 1), dtype=torch.float32, device=self.device)
                    out, _ = ops.loss2(head, B, T, k1a, k1b, ds, lab2, w2, displ_col=dcol, labelD=labelD)
                else:
                    out = ops.loss(head, K1, w, hard=label.reshape(-1).contiguous(), displ_col=dcol, labelD=labelD)
                totals[slot] += out[0]
                n += 1
                if valMAP:
                    cls, scores = ops.process_prediction(head, B, T, K1, dcol)
                    map_preds.append(scores.cpu())
                    from .modules import process_labels
                    map_labels.append(process_labels(label.cpu(), batch.get("labelD"), num_classes=K1))
                feeder.done(batch)
        for st in streams:
            st.synchronize()
        total = totals[0] + totals[1]
        avg = float(total.item()) / max(n, 1)       # one device sync per epoch, not per batch
        if valMAP:
            return avg, torch.cat(map_labels, 0), torch.cat(map_preds, 0)
        return avg


def _train_epoch_impl(self, loader, optimizer, lr_scheduler, acc_grad_iter, fg_weight):
    """Training branch of model.py:193-332 + BaseRGBModel.step (modules.py:390-404): per batch, mixup when the loader
    delivers 'frame2'/'label2'/'labelD2' (model.py:233-260: Beta(0.2,0.2) weights from `random`, soft labels), the
    train-mode `Impl.forward(frame, inference=False)` (one random crop per batch, per-clip augmentation, dropout), the
    loss (single or joint-dataset double head, hard or soft labels), the backward and, every `acc_grad_iter` batches,
    the optimizer + scheduler step."""
    import random
    eng = optimizer.engine
    if eng is not self._model.train_engine():
        raise RuntimeError("the optimizer was built for another model")
    self._model.train()
    optimizer.zero_grad()
    total = torch.zeros((), dtype=torch.float32, device=self.device)
    opts = self._loss_opt
    if opts is not None and self._model._double_head:
        raise ValueError("loss_options: the joint-dataset double head is not covered")
    parts = None if self._kd is None and opts is None else torch.zeros(5, dtype=torch.float32, device=self.device)
    self.loss_parts = None
    n = 0
    cur = torch.cuda.current_stream()
    with self._ctx():
        self._stream.wait_stream(cur)        # engine construction / load() / zero_grad were queued on the caller's stream
        from . import feeder
        for batch_idx, batch in enumerate(feeder.prefetch(loader, self.device, auto=False)):
            feeder.wait(batch)

            def u8(x):
                x = x.to(self.device)
                return (x if x.dtype == torch.uint8 else x.round().clamp_(0, 255).to(torch.uint8)).contiguous()
            # trainclips.ResidentClips with mixup: the blend is deferred until lam is drawn, no uint8 clip is delivered
            mix = batch.get("mix")
            frame = u8(batch["frame"]) if mix is None else None
            label = batch["label"].to(self.device)
            labelD = batch["labelD"].to(self.device).float() if "labelD" in batch else None
            B, T = (frame if frame is not None else label).shape[:2]
            soft = None
            dataset = None
            if self._model._double_head:
                dataset = torch.as_tensor(batch["dataset"]).to(self.device).long()
                label = update_labels_2heads(label.clone(), dataset, self._args.num_classes)
            if "frame2" in batch or mix is not None:
                from . import ops_bwd
                K1 = self._num_classes                               # train_tdeed.py:148 widens it for the double head
                lam = torch.tensor([random.betavariate(0.2, 0.2) for _ in range(B)], dtype=torch.float32, device=self.device)
                if mix is not None:
                    frame = mix(lam)                                 # gather + blend in one launch, the same fp32 bits
                else:
                    frame = ops_bwd.mix_frames(frame, u8(batch["frame2"]), lam)      # fp32 0..255 frames
                label2 = batch["label2"].to(self.device)
                oh = torch.nn.functional.one_hot
                soft = (lam.view(B, 1, 1) * oh(label, K1).float() + (1 - lam).view(B, 1, 1) * oh(label2, K1).float())
                label = None
                if "labelD2" in batch:
                    labelD = lam.view(B, 1) * labelD + (1 - lam).view(B, 1) * batch["labelD2"].to(self.device).float()
            pred, _ = self._model(frame, y=label, inference=False)
            head = (pred["_head_out"] if isinstance(pred, dict) else pred).reshape(B * T, -1)
            scale = 1.0 / acc_grad_iter
            # distillation: the teacher's eval-mode forward on the student's view, on this stream, before the loss
            thead, kd = (None, None) if self._kd is None else self._teacher_head()
            loss, dhead = eng.temporal.loss_fwd_bwd(
                head, B, T, None if label is None else label.reshape(-1).contiguous(),
                labelD=None if labelD is None else labelD.reshape(-1).contiguous(),
                soft=None if soft is None else soft.reshape(B * T, -1).contiguous(), fg_weight=fg_weight, dataset=dataset,
                teacher=thead, kd=kd, loss=opts)
            last = (batch_idx + 1) % acc_grad_iter == 0
            # data parallel (one process per GPU under torchrun): the bucket all-reduces of the step's last micro-batch are
            # enqueued from inside the backward; optimizer.step() waits for them on the device
            eng.backward_and_write(self._model._train_ctx, dhead, scale=scale, first=batch_idx % acc_grad_iter == 0,
                                   reduce=last and eng.reducer is not None)
            self._model._train_ctx = None
            if last:
                optimizer.step()
                if lr_scheduler is not None:
                    lr_scheduler.step()
                optimizer.zero_grad()
            if parts is None:
                total += loss[0]
            else:
                parts += loss
            n += 1
            feeder.done(batch)
        self._stream.synchronize()
    self._model._engines = {}                      # the inference engines hold packed copies of the old weights
    if parts is not None:
        p = [float(v) / max(n, 1) for v in parts.tolist()]           # the epoch's one host synchronisation
        self.loss_parts = dict(ce=p[1], mse=p[2], kd=p[3], kd_displ=p[4]) if self._kd is not None else dict(ce=p[1], mse=p[2])
        return p[0]
    return float(total.item()) / max(n, 1)


TDEEDModel._train_epoch = _train_epoch_impl


def update_labels_2heads(labels, datasets, num_classes1=1):
    """model.py:371-376."""
    for i in range(len(datasets)):
        if datasets[i] == 2:
            labels[i] = labels[i] + num_classes1 + 1
    return labels
