"""Distillation on the MI355X: tdeed_loss_kd against fp64 autograd and against the plain loss kernels, then the teacher's
view, the epoch plumbing, the captured step and a teacher of another size through the public interface.  -m gpu only.
Cases, reference and bounds: tests/distill_cases.py.  Tiny models as tests/test_gpu_ema.py builds them."""
import functools
import random

import numpy as np
import pytest
import torch

import distill_cases as D
from helpers import cfg_ns, drop_masks, model_state, t
from tdeed_amd import synth, state_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
K1 = CFG["num_classes"] + 1
# (case arguments, displ_weight > 0 allowed): the host test's shapes; 255 / 256 / 513 rows (a ragged last trip, exactly one
# trip, a third trip of one thread); ld_t != ld; a displacement column on one side only
KERNEL_CASES = [((r, k), True) for r, k in D.SHAPES] + [((255, 5), True), ((256, 5), True), ((513, 5), True),
                                                        ((60, 5, True, True, 2), True), ((60, 5, False, True), False),
                                                        ((60, 5, True, False), False)]


@pytest.fixture(scope="module")
def ops():
    from tdeed_amd import ops as o, _lib
    _lib.load()
    return o


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    if a.dtype != torch.float32:                                 # (the BatchNorm step counters)
        return a.dtype == b.dtype and torch.equal(a.detach().cpu(), b.detach().cpu())
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _launch(ops, c, kind, tau, alpha, beta, **kw):
    """c: a case already on the device"""
    return ops.loss_kd(c["head"], c["K1"], c["cls_w"], kw.pop("teacher", c["teacher"]), displ_col=c["displ_col"],
                       labelD=c["labelD"], teacher_displ_col=c["teacher_displ_col"], alpha=alpha, temperature=tau,
                       displ_weight=beta, grad_scale=kw.pop("grad_scale", D.GRAD_SCALE), **D.label_kw(c, kind), **kw)


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("kind", ["hard", "soft"])
@pytest.mark.parametrize("args,with_beta", KERNEL_CASES)
def test_kernel_against_fp64_autograd(ops, args, with_beta, kind):
    c = D.case(*args)
    cd = _dev(c)
    worst = (0.0, 0.0)
    for tau, alpha, beta in D.SETTINGS:
        if beta > 0.0 and not with_beta:
            continue
        out5, dhead = _launch(ops, cd, kind, tau, alpha, beta)
        assert tuple(out5.shape) == (5,) and dhead.shape == c["head"].shape
        ev, eg = D.assert_within(out5.cpu(), dhead, *D.formula64(c, kind, tau, alpha, beta), (args, kind, tau, alpha, beta))
        worst = (max(worst[0], ev), max(worst[1], eg))
        if not with_beta:
            assert float(out5[4]) == 0.0                         # one displacement column is missing: kd_displ is 0
    print(f"loss_kd vs fp64 autograd {args} {kind}: value {worst[0]:.2e}, gradient {worst[1]:.2e}")


def test_value_only_launch(ops):
    cd = _dev(D.case(60, 5))
    for kind in ("hard", "soft"):
        out5, dhead = _launch(ops, cd, kind, 2.0, 0.5, 0.25)
        only, none = _launch(ops, cd, kind, 2.0, 0.5, 0.25, want_grad=False)
        assert none is None and dhead is not None and _same_bits(only, out5)


@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_alpha_zero_equals_the_plain_kernels(ops, kind):
    """alpha = 0, displ_weight = 0: total, ce, mse and the gradient are the numbers of ops.loss / ops.loss_bwd."""
    for args in [(r, k) for r, k in D.SHAPES] + [(513, 5), (60, 5, True, True, 2), (60, 5, False, True)]:
        cd = _dev(D.case(*args))
        kw = dict(displ_col=cd["displ_col"], labelD=cd["labelD"], **D.label_kw(cd, kind))
        want = ops.loss(cd["head"], cd["K1"], cd["cls_w"], **kw)
        want_d = ops.loss_bwd(cd["head"], cd["K1"], cd["cls_w"], grad_scale=D.GRAD_SCALE, **kw)
        for tau in D.TAUS:
            out5, dhead = _launch(ops, cd, kind, tau, 0.0, 0.0)
            assert torch.equal(out5[:3], want), (args, tau, out5, want)
            assert torch.equal(dhead, want_d), (args, tau)
            assert float(out5[3]) > 0.0


def test_two_launches_give_the_same_bits(ops):
    cd = _dev(D.case(513, 5))
    for kind in ("hard", "soft"):
        a, da = _launch(ops, cd, kind, 2.0, 0.5, 0.25)
        b, db = _launch(ops, cd, kind, 2.0, 0.5, 0.25)
        assert _same_bits(a, b) and _same_bits(da, db)


def test_bad_inputs(ops):
    """Nothing is clamped: a NaN teacher logit reaches kd and its row's gradient; an out-of-range hard label is never used
    as an index and turns the loss (not the gradient) into NaN."""
    c = D.case(60, 5)
    cd = _dev(c)
    sick = cd["teacher"].clone()
    sick[17, 2] = float("nan")
    out5, dhead = _launch(ops, cd, "hard", 2.0, 0.5, 0.0, teacher=sick)
    assert bool(torch.isnan(out5[3])) and bool(torch.isnan(out5[0])) and bool(torch.isfinite(out5[1:3]).all())
    bad_rows = (~torch.isfinite(dhead)).any(dim=1).nonzero().reshape(-1).tolist()
    assert bad_rows == [17]
    for label in (-1, c["K1"], c["K1"] + 100):
        hard = cd["hard"].clone()
        hard[5] = label
        out5, dhead = ops.loss_kd(cd["head"], c["K1"], cd["cls_w"], cd["teacher"], hard=hard, displ_col=cd["displ_col"],
                                  labelD=cd["labelD"], teacher_displ_col=cd["teacher_displ_col"])
        assert bool(torch.isnan(out5[0])) and bool(torch.isnan(out5[1])) and bool(torch.isfinite(out5[2:]).all())
        assert bool(torch.isfinite(dhead).all())


# ----------------------------------------------------------------------------- models
def _batch(rank=0, twins=False):
    B, T = 2, CFG["clip_len"]
    frames = t(synth.uint8_clip(2300 + rank, (B, T, 3, 64, 64)))
    lab, labD = synth.labels(2400 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
    out = dict(frame=frames, label=t(lab).long(), labelD=t(labD).float())
    if twins:
        lab2, labD2 = synth.labels(2500 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
        out.update(frame2=t(synth.uint8_clip(2600 + rank, (B, T, 3, 64, 64))), label2=t(lab2).long(), labelD2=t(labD2).float())
    return out


def _model(cfg=CFG, seed=17, augment_off=True, replay_dropout=True):
    from tdeed_amd import augment
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m._train_dtype = torch.float32
    m.load({k: t(v) for k, v in model_state(cfg, seed).items()})
    if augment_off:
        m._model.augment_fn = augment.crop_only
    if replay_dropout:
        m._model.dropout_mask_fn = lambda B, T, C, n: drop_masks(77, B, T, C, n)
    return m


@functools.lru_cache(maxsize=None)
def _teacher(arch="rny002_gsf", crop=None, radi=2):
    """a teacher is only ever scored: one per configuration, shared"""
    return _model(dict(CFG, feature_arch=arch, crop_dim=crop, radi_displacement=radi), seed=23, augment_off=False)


def _draws(seed, B=2, H=64, W=64, cd=48):
    """what a forward with a generator in this state draws, on the CPU: (identity augmentation?, per-clip flips)"""
    from tdeed_amd import augment
    g = torch.Generator().manual_seed(seed)
    torch.randint(0, H - cd + 1, size=(1,), generator=g)
    torch.randint(0, W - cd + 1, size=(1,), generator=g)
    prm, flip = augment.draw_params(B, g)
    return augment.is_identity(prm), flip


def _seed(want):
    return next(s for s in range(4000) if want(*_draws(s)))


SEED_AUGMENTED = _seed(lambda ident, flip: not ident and not bool(flip.any()))
SEED_AUGMENTED_FLIPS = _seed(lambda ident, flip: not ident and bool(flip.any()) and not bool(flip.all()))
SEED_FLIPS_ONLY = _seed(lambda ident, flip: ident and bool(flip.any()) and not bool(flip.all()))


# ----------------------------------------------------------------------------- 2. the teacher sees the student's view
@pytest.mark.parametrize("seed,twins", [(SEED_AUGMENTED, False), (SEED_AUGMENTED_FLIPS, False), (SEED_FLIPS_ONLY, False),
                                        (SEED_AUGMENTED_FLIPS, True)])
def test_teacher_head_is_the_eval_forward_of_the_students_view(seed, twins):
    """One distillation batch with a random crop window and the built-in augmentation drawn from a seeded generator: the
    teacher's head equals, bit for bit, its own eval-mode `forward(inference=False)` on the same frames under a generator
    in the same starting state -- colour / blur draws, flips only, and mixup twins (the blended fp32 frames)."""
    cfg = dict(CFG, crop_dim=48)
    m, teacher = _model(cfg, augment_off=False), _teacher(crop=48)
    m.distill_from(teacher)
    opt, _ = m.get_optimizer({"lr": 1e-3})
    batch = _batch(0, twins)
    m._model.augment_generator = torch.Generator().manual_seed(seed)
    random.seed(5)
    loss = m.epoch([batch], optimizer=opt)
    torch.cuda.synchronize()
    got = m._kd_last.clone()
    B, T = batch["label"].shape
    assert np.isfinite(loss) and tuple(got.shape) == (B * T, K1 + 1)
    frame = batch["frame"].to(DEV)
    if twins:
        from tdeed_amd import ops_bwd
        random.seed(5)
        lam = torch.tensor([random.betavariate(0.2, 0.2) for _ in range(B)], dtype=torch.float32, device=DEV)
        frame = ops_bwd.mix_frames(frame, batch["frame2"].to(DEV), lam)
    tm = teacher._model
    tm.augment_generator = torch.Generator().manual_seed(seed)
    try:
        tm.eval()
        pred, _ = tm(frame, inference=False)
    finally:
        tm.augment_generator = None
    want = pred["_head_out"].reshape(B * T, -1)
    torch.cuda.synchronize()
    assert _same_bits(got, want)
    assert m._kd_last.data_ptr() == want.data_ptr()              # a reference to the teacher engine's head buffer, no copy
    assert float(got.abs().sum()) > 0.0


# ----------------------------------------------------------------------------- 3. no effect when off
def test_alpha_zero_distillation_trains_the_same_bits():
    """Two steps with distill_from(teacher, alpha=0, displ_weight=0) against two steps without a teacher: the loss, every
    parameter and every BatchNorm buffer are equal bit for bit.  Crop, augmentation (global CPU generator) and dropout
    (global device generator) are drawn, so a random draw taken by the teacher would show in the second step."""
    cfg = dict(CFG, crop_dim=48)
    batches = [_batch(0), _batch(1)]
    res = []
    for with_teacher in (False, True):
        m = _model(cfg, augment_off=False, replay_dropout=False)
        if with_teacher:
            m.distill_from(_teacher(crop=48), alpha=0.0, displ_weight=0.0)
        opt, _ = m.get_optimizer({"lr": 1e-3})
        torch.manual_seed(11)
        loss = m.epoch(batches, optimizer=opt)
        torch.cuda.synchronize()
        assert opt.engine.opt.t == 2
        res.append((loss, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, m.loss_parts))
    (la, sa, pa), (lb, sb, pb) = res
    assert la == lb and np.isfinite(la)
    assert pa is None and set(pb) == {"ce", "mse", "kd", "kd_displ"} and pb["kd"] > 0.0
    for k in sa:
        assert _same_bits(sa[k], sb[k]), k
    start = model_state(cfg, 17)
    assert not torch.equal(sa["_features.stem.bn.running_mean"], t(start["_features.stem.bn.running_mean"]))


# ----------------------------------------------------------------------------- 4. plumbing
def test_epoch_loss_and_parts_are_loss_kd_on_the_two_heads(ops):
    batch = _batch(0)
    B, T = batch["label"].shape
    kd = dict(alpha=0.3, temperature=3.0, displ_weight=0.25)
    m, teacher = _model(), _teacher()
    m.distill_from(teacher, teacher_dtype=torch.float32, **kd)
    opt, _ = m.get_optimizer({"lr": 1e-3})
    loss = m.epoch([batch], optimizer=opt, acc_grad_iter=1)
    torch.cuda.synchronize()
    parts = m.loss_parts
    # the student's head of that step from a twin: the same weights, frames and dropout masks
    twin = _model()
    twin._model.train()
    pred, _ = twin._model(batch["frame"].to(DEV), y=batch["label"].to(DEV), inference=False)
    head = pred["_head_out"].reshape(B * T, -1)
    cls_w = torch.tensor([1.0] + [5.0] * (K1 - 1), dtype=torch.float32, device=DEV)
    out5, _ = ops.loss_kd(head, K1, cls_w, m._kd_last, hard=batch["label"].to(DEV).reshape(-1).contiguous(), displ_col=K1,
                          labelD=batch["labelD"].to(DEV).reshape(-1).contiguous(), teacher_displ_col=K1,
                          temperature=kd["temperature"], alpha=kd["alpha"], displ_weight=kd["displ_weight"])
    out5 = out5.cpu()
    assert loss == float(out5[0])
    assert parts == dict(ce=float(out5[1]), mse=float(out5[2]), kd=float(out5[3]), kd_displ=float(out5[4]))
    assert parts["kd"] > 0.0 and parts["kd_displ"] > 0.0 and parts["mse"] > 0.0
    # a validation epoch never runs the teacher, and clearing restores None
    last = m._kd_last.clone()
    m.epoch([batch])
    assert _same_bits(m._kd_last, last)
    m.distill_from(None)
    assert m.loss_parts is None and m._kd_last is None
    assert np.isfinite(m.epoch([batch], optimizer=opt)) and m.loss_parts is None


def test_teacher_on_another_device_is_refused_at_the_first_batch():
    from tdeed_amd.model import TDEEDModel
    m = _model()
    cpu_teacher = TDEEDModel(device="cpu", args=cfg_ns(CFG))
    m.distill_from(cpu_teacher)                                  # accepted at the call: the device is checked per batch
    opt, _ = m.get_optimizer({"lr": 1e-3})
    with pytest.raises(ValueError, match="the teacher is on cpu"):
        m.epoch([_batch(0)], optimizer=opt)


# ----------------------------------------------------------------------------- 5. the captured step
def _engine():
    from tdeed_amd.trainer import TrainEngine
    sd = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}
    return TrainEngine(CFG, sd, act_dtype=torch.float32, device=DEV, lr=1e-3)


def test_captured_step_equals_the_eager_step_and_records_its_settings():
    b = _batch(0)
    frames, lab, labD = b["frame"].to(DEV), b["label"].to(DEV), b["labelD"].to(DEV)
    B, T = lab.shape
    rng = np.random.default_rng(31)
    heads = [torch.from_numpy(rng.standard_normal((B * T, K1 + 3)).astype(np.float32) * 3.0).to(DEV) for _ in range(2)]
    engines, steps, teachers = [], [], []
    for graph in (True, False):
        eng, tch = _engine(), heads[0].clone()
        kd = dict(teacher=tch, displ_col_t=K1 + 2, alpha=0.5, temperature=2.0, displ_weight=0.25)
        step = eng.make_step(B, 64, 64, frames, lab, labD, None, use_graph=graph, kd=kd)
        loss = step()
        assert tuple(loss.shape) == (5,)
        tch.copy_(heads[1])                                      # the teacher head is read at every call
        step()
        torch.cuda.synchronize()
        engines.append(eng)
        steps.append(kd)
    a, e = engines
    assert a.opt.t == 2 and e.opt.t == 2
    for x, y, what in ((a.params.flat, e.params.flat, "flat"), (a.opt.exp_avg, e.opt.exp_avg, "m"),
                       (a.opt.exp_avg_sq, e.opt.exp_avg_sq, "v")):
        assert _same_bits(x, y), what
    # the second step used the second head: an engine fed the first head twice ends elsewhere
    c, tch = _engine(), heads[0].clone()
    step = c.make_step(B, 64, 64, frames, lab, labD, None, use_graph=False, kd=dict(steps[1], teacher=tch))
    step(), step()
    assert not _same_bits(c.params.flat, e.params.flat)
    # the handle records its settings: the same ones reuse it, others rebuild, and the stale handle refuses them
    kd = steps[0]
    h = a.last_graph
    assert h.kd == dict(ld_t=K1 + 3, displ_col_t=K1 + 2, alpha=0.5, temperature=2.0, displ_weight=0.25)
    assert tuple(h.teacher.shape) == (B * T, K1 + 3)
    a.make_step(B, 64, 64, frames, lab, labD, None, kd=kd)
    assert a.last_graph is h
    other = dict(kd, alpha=0.25)
    a.make_step(B, 64, 64, frames, lab, labD, None, kd=other)
    assert a.last_graph is not h and a.last_graph.kd["alpha"] == 0.25
    t_before = a.opt.t
    for kw in (dict(teacher=other["teacher"], kd=other), dict()):
        with pytest.raises(RuntimeError, match="other distillation settings"):
            a.step_graph(h, frames, lab, labD, **kw)
    with pytest.raises(RuntimeError, match="other distillation settings"):
        a.step_graph(a.last_graph, frames, lab, labD)            # a kd handle called without a teacher
    assert a.opt.t == t_before                                   # the refused calls ran nothing


# ----------------------------------------------------------------------------- 6. a teacher of another size
def test_an_800mf_teacher_distils_into_a_200mf_student():
    batch = _batch(0)
    teacher = _teacher(arch="rny008_gsf")
    assert teacher._model._feat_dim != _teacher()._model._feat_dim
    states = []
    for with_teacher in (False, True):
        m = _model()
        if with_teacher:
            m.distill_from(teacher, displ_weight=0.25)
        opt, _ = m.get_optimizer({"lr": 1e-3})
        loss = m.epoch([batch], optimizer=opt)
        torch.cuda.synchronize()
        assert np.isfinite(loss) and opt.engine.opt.t == 1
        states.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        if with_teacher:
            p = m.loss_parts
            assert all(np.isfinite(v) for v in p.values()) and p["kd"] > 0.0 and p["kd_displ"] > 0.0
    moved = [k for k in states[0] if state_layout.is_parameter(k) and not _same_bits(states[0][k], states[1][k])]
    assert len(moved) > 0.9 * sum(state_layout.is_parameter(k) for k in states[0])
