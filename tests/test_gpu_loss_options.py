"""The loss options on the MI355X: tdeed_loss_opt against fp64 autograd, against the plain and the distillation kernels at
neutral settings, then TemporalTrain.loss_fwd_bwd, the epoch plumbing and the captured step on a tiny model.  -m gpu only.
Cases, reference and bounds: tests/loss_option_cases.py.  Tiny models as tests/test_gpu_distill.py builds them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import distill_cases as D
import loss_option_cases as L
from helpers import cfg_ns, drop_masks, model_state, t
from tdeed_amd import synth, state_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)
K1 = CFG["num_classes"] + 1
OPTS = dict(label_smoothing=0.1, focal_gamma=2.0)
# the case table and, for the kernel's row loop, 255 / 256 / 513 rows (a ragged last trip, exactly one trip, a third trip of
# one thread)
KERNEL_CASES = L.CASES + ["255x5", "256x5", "513x5"]


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


@functools.lru_cache(maxsize=None)
def _dev(name):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in L.case(name).items()}


def _launch(ops, name, kind, eps, gamma, teacher=True, **kw):
    c = _dev(name)
    return ops.loss_opt(c["head"], c["K1"], c["cls_w"], **{**L.opt_kw(c, kind, eps, gamma, teacher), **kw})


# ----------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("teacher", [False, True])
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernel_against_fp64_autograd(ops, name, kind, teacher):
    c = L.case(name)
    worst = (0.0, 0.0)
    for eps, gamma in L.SETTINGS:
        out5, dhead = _launch(ops, name, kind, eps, gamma, teacher)
        assert tuple(out5.shape) == (5,) and dhead.shape == c["head"].shape
        out5, dhead = out5.cpu(), dhead.cpu()
        ref5, refg = L.formula64(name, kind, eps, gamma, teacher)
        ev, eg = D.errors(out5, dhead, ref5, refg)
        print(f"loss_opt {name} {kind} teacher={teacher} eps={eps} gamma={gamma}: value {ev:.2e}, gradient {eg:.2e}")
        assert bool(torch.isfinite(dhead).all())
        D.assert_within(out5, dhead, ref5, refg, (name, kind, teacher, eps, gamma))
        if not teacher:
            assert float(out5[3]) == 0.0 and float(out5[4]) == 0.0
        # unused columns (and a displacement column without labels) come back 0
        used = list(range(c["K1"])) + ([c["displ_col"]] if c["displ_col"] >= 0 else [])
        rest = [k for k in range(c["head"].shape[1]) if k not in used]
        assert not rest or float(dhead[:, rest].abs().max()) == 0.0
        worst = (max(worst[0], ev), max(worst[1], eg))
    print(f"loss_opt vs fp64 autograd {name} {kind} teacher={teacher}: value {worst[0]:.2e}, gradient {worst[1]:.2e}")


@pytest.mark.parametrize("teacher", [False, True])
def test_value_only_launch(ops, teacher):
    """dhead = NULL: the same five values, within the bounds as well"""
    for name, kind, (eps, gamma) in [(n, k, s) for n in ("60x5", "sat0", "zero_weight") for k in L.KINDS
                                     for s in ((0.0, 0.0), (0.1, 2.0), (1.0, 0.5))]:
        out5, dhead = _launch(ops, name, kind, eps, gamma, teacher)
        only, none = _launch(ops, name, kind, eps, gamma, teacher, want_grad=False)
        assert none is None and dhead is not None and _same_bits(only, out5)
        D.assert_within(only.cpu(), None, *L.formula64(name, kind, eps, gamma, teacher), (name, kind, eps, gamma))


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_neutral_options_equal_the_sibling_kernels(ops, name, kind):
    """eps = gamma = 0: the bits of ops.loss + ops.loss_bwd without a teacher, those of ops.loss_kd with one"""
    c = _dev(name)
    kw = dict(displ_col=c["displ_col"], labelD=c["labelD"], **D.label_kw(c, kind))
    want = ops.loss(c["head"], c["K1"], c["cls_w"], **kw)
    want_d = ops.loss_bwd(c["head"], c["K1"], c["cls_w"], grad_scale=L.GRAD_SCALE, **kw)
    out5, dhead = _launch(ops, name, kind, 0.0, 0.0, False)
    assert torch.equal(out5[:3], want) and float(out5[3]) == 0.0 and float(out5[4]) == 0.0, (out5, want)
    assert torch.equal(dhead, want_d)
    for beta in {0.0, L.beta_of(c)}:
        kd5, kd_d = ops.loss_kd(c["head"], c["K1"], c["cls_w"], c["teacher"], teacher_displ_col=c["teacher_displ_col"],
                                alpha=L.KD["alpha"], temperature=L.KD["tau"], displ_weight=beta, grad_scale=L.GRAD_SCALE, **kw)
        out5, dhead = _launch(ops, name, kind, 0.0, 0.0, True, displ_weight=beta)
        assert torch.equal(out5, kd5), (out5, kd5)
        assert torch.equal(dhead, kd_d)


@pytest.mark.parametrize("kind", L.KINDS)
def test_a_teacher_with_zero_weights_changes_nothing(ops, kind):
    """teacher present with alpha = displ_weight = 0: total, ce, mse and the gradient of the call without a teacher"""
    for name, (eps, gamma) in [(n, s) for n in ("60x5", "257x33", "wide", "sat2") for s in L.SETTINGS]:
        a5, ad = _launch(ops, name, kind, eps, gamma, False)
        b5, bd = _launch(ops, name, kind, eps, gamma, True, alpha=0.0, displ_weight=0.0)
        assert torch.equal(a5[:3], b5[:3]) and torch.equal(ad, bd), (name, eps, gamma)
        assert float(b5[3]) > 0.0                                # kd is still reported


def test_two_launches_give_the_same_bits(ops):
    for kind, teacher, (eps, gamma) in [(k, tc, s) for k in L.KINDS for tc in (False, True) for s in ((0.1, 2.0), (1.0, 0.5))]:
        a, da = _launch(ops, "513x5", kind, eps, gamma, teacher)
        b, db = _launch(ops, "513x5", kind, eps, gamma, teacher)
        assert _same_bits(a, b) and _same_bits(da, db)


def test_out_of_range_label(ops):
    """never used as an index: the classification value becomes NaN, the gradient stays finite"""
    c = _dev("60x5")
    for label in (-1, c["K1"], c["K1"] + 100):
        hard = c["hard"].clone()
        hard[5] = label
        for eps, gamma in ((0.0, 0.0), (0.1, 2.0)):
            out5, dhead = _launch(ops, "60x5", "hard", eps, gamma, True, hard=hard)
            assert bool(torch.isnan(out5[0])) and bool(torch.isnan(out5[1])) and bool(torch.isfinite(out5[2:]).all())
            assert bool(torch.isfinite(dhead).all())


def test_argument_errors_are_error_codes():
    from tdeed_amd import _lib
    lib = _lib.load()
    c = _dev("16x2")
    out, dh = torch.empty(5, device=DEV), torch.empty_like(c["head"])
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())           # noqa: E731

    def rc(teacher=None, ld=3, K1=2, displ_col=2, ld_t=3, displ_col_t=2, alpha=0.0, tau=1.0, beta=0.0, eps=0.0, gamma=0.0,
           hard=c["hard"]):
        return lib.tdeed_loss_opt(p(c["head"]), 16, ld, K1, p(hard), None, p(c["cls_w"]), displ_col, p(c["labelD"]), p(teacher),
                                  ld_t, displ_col_t, alpha, tau, beta, eps, gamma, 1.0, p(out), p(dh), None)

    tch = c["teacher"]
    assert rc() == 0 and rc(teacher=tch, alpha=0.5, tau=2.0, beta=0.25, eps=0.1, gamma=2.0) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(eps=-0.1), dict(eps=1.5), dict(eps=nan), dict(gamma=-1.0), dict(gamma=inf), dict(gamma=nan),
               dict(alpha=0.5), dict(beta=0.5), dict(K1=4), dict(displ_col=3), dict(hard=None),
               dict(teacher=tch, alpha=1.5), dict(teacher=tch, tau=0.0), dict(teacher=tch, beta=-1.0),
               dict(teacher=tch, ld_t=1), dict(teacher=tch, displ_col_t=3), dict(teacher=tch, beta=0.5, displ_col_t=-1)):
        assert rc(**kw) != 0, kw
        assert b"loss_opt" in lib.tdeed_last_error()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- models
def _batch(rank=0):
    B, T = 2, CFG["clip_len"]
    frames = t(synth.uint8_clip(2300 + rank, (B, T, 3, 64, 64)))
    lab, labD = synth.labels(2400 + rank, B, T, CFG["num_classes"], CFG["radi_displacement"], fg_frac=0.4)
    return dict(frame=frames, label=t(lab).long(), labelD=t(labD).float())


def _model(cfg=CFG, seed=17):
    from tdeed_amd import augment
    from tdeed_amd.model import TDEEDModel
    m = TDEEDModel(device=DEV, args=cfg_ns(cfg))
    m._train_dtype = torch.float32
    m.load({k: t(v) for k, v in model_state(cfg, seed).items()})
    m._model.augment_fn = augment.crop_only
    m._model.dropout_mask_fn = lambda B, T, C, n: drop_masks(77, B, T, C, n)
    return m


def _engine():
    from tdeed_amd.trainer import TrainEngine
    sd = {k: t(v) for k, v in synth.make_state(state_layout.model_state_shapes(CFG), 17).items()}
    return TrainEngine(CFG, sd, act_dtype=torch.float32, device=DEV, lr=1e-3)


def _epoch(m, batches, train=True):
    loss = m.epoch(batches, optimizer=m.get_optimizer({"lr": 1e-3})[0] if train else None)
    torch.cuda.synchronize()
    return loss, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, m.loss_parts


@functools.lru_cache(maxsize=None)
def _plain_epoch():
    """two training batches on a model that never had options: shared, left unchanged"""
    return _epoch(_model(), [_batch(0), _batch(1)])


# ----------------------------------------------------------------------------- 2. loss_fwd_bwd
@pytest.mark.parametrize("kind", L.KINDS)
def test_loss_fwd_bwd_with_class_weights_against_the_reference(kind):
    """the 60 x 5 case as B = 6 clips of T = 10 frames through TemporalTrain.loss_fwd_bwd(loss=...) with the class weight
    vector that holds a zero, with and without a teacher; the vector is uploaded once"""
    c, cd = L.case("zero_weight"), _dev("zero_weight")
    eng = _engine()
    ts = eng.temporal
    ts.K1, ts.radi = c["K1"], 2
    ts.head_layout = lambda: (c["K1"], c["K1"], False)
    eps, gamma = 0.1, 2.0
    loss = dict(label_smoothing=eps, focal_gamma=gamma, class_weights=L.ZERO_WEIGHTS)
    lab = dict(label=cd["hard"], soft=None) if kind == "hard" else dict(label=None, soft=cd["soft"])
    for teacher in (False, True):
        kw = dict(teacher=cd["teacher"], kd=dict(displ_col_t=c["teacher_displ_col"], alpha=L.KD["alpha"],
                                                 temperature=L.KD["tau"], displ_weight=L.beta_of(c))) if teacher else {}
        out5, dhead = ts.loss_fwd_bwd(cd["head"], 6, 10, lab["label"], labelD=cd["labelD"], soft=lab["soft"], fg_weight=5.0,
                                      grad_scale=L.GRAD_SCALE, loss=loss, **kw)
        assert tuple(out5.shape) == (5,)
        D.assert_within(out5.cpu(), dhead, *L.formula64("zero_weight", kind, eps, gamma, teacher), (kind, teacher))
    keys = [k for k in ts._cls_w if isinstance(k, tuple) and k[0] == "class_weights"]
    assert len(keys) == 1 and ts._cls_w[keys[0]].tolist() == L.ZERO_WEIGHTS
    ptr = ts._cls_w[keys[0]].data_ptr()
    ts.loss_fwd_bwd(cd["head"], 6, 10, lab["label"], labelD=cd["labelD"], soft=lab["soft"], loss=dict(loss, class_weights=tuple(L.ZERO_WEIGHTS)))
    assert ts._cls_w[keys[0]].data_ptr() == ptr and len([k for k in ts._cls_w if isinstance(k, tuple)]) == 1
    with pytest.raises(ValueError, match="class_weights"):
        ts.loss_fwd_bwd(cd["head"], 6, 10, lab["label"], labelD=cd["labelD"], soft=lab["soft"], loss=dict(class_weights=[1.0, 2.0]))


# ----------------------------------------------------------------------------- 3. the epoch
def test_options_set_and_cleared_train_the_plain_bits():
    m = _model()
    m.loss_options(**OPTS, class_weights=[1.0, 2.0, 3.0, 4.0])
    m.loss_options()
    la, sa, pa = _epoch(m, [_batch(0), _batch(1)])
    lb, sb, pb = _plain_epoch()
    assert la == lb and np.isfinite(la) and pa is None and pb is None
    for k in sa:
        assert _same_bits(sa[k], sb[k]), k


def test_options_change_the_training_and_report_their_parts(ops):
    m = _model()
    m.loss_options(**OPTS)
    loss, state, parts = _epoch(m, [_batch(0), _batch(1)])
    assert np.isfinite(loss) and set(parts) == {"ce", "mse"} and all(np.isfinite(v) for v in parts.values())
    assert abs(loss - (parts["ce"] + parts["mse"])) <= 1e-5 * max(1.0, abs(loss))
    lb, sb, _ = _plain_epoch()
    assert loss != lb
    moved = [k for k in state if state_layout.is_parameter(k) and not _same_bits(state[k], sb[k])]
    assert len(moved) > 0.9 * sum(state_layout.is_parameter(k) for k in state)
    # class_weights override epoch()'s fg_weight: the first batch's loss is loss_opt on a twin's head with that vector
    batch = _batch(0)
    B, T = batch["label"].shape
    cw = [1.0, 2.0, 0.0, 4.0]
    m2 = _model().loss_options(**OPTS, class_weights=cw)
    opt, _ = m2.get_optimizer({"lr": 1e-3})
    got = m2.epoch([batch], optimizer=opt, fg_weight=9)
    twin = _model()
    twin._model.train()
    pred, _ = twin._model(batch["frame"].to(DEV), y=batch["label"].to(DEV), inference=False)
    head = pred["_head_out"].reshape(B * T, -1)
    out5, _ = ops.loss_opt(head, K1, torch.tensor(cw, device=DEV), hard=batch["label"].to(DEV).reshape(-1).contiguous(),
                           displ_col=K1, labelD=batch["labelD"].to(DEV).reshape(-1).contiguous(), **OPTS)
    out5 = out5.cpu()
    assert got == float(out5[0]) and m2.loss_parts == dict(ce=float(out5[1]), mse=float(out5[2]))


def test_a_validation_epoch_keeps_the_plain_loss():
    batches = [_batch(0), _batch(1)]
    plain, _, _ = _epoch(_model(), batches, train=False)
    m = _model().loss_options(**OPTS, class_weights=[1.0, 2.0, 3.0, 4.0])
    got, _, parts = _epoch(m, batches, train=False)
    assert got == plain and np.isfinite(got) and parts is None


def test_options_and_a_teacher_combine():
    teacher = _model(seed=23)
    m = _model().distill_from(teacher, displ_weight=0.25).loss_options(**OPTS)
    loss, _, parts = _epoch(m, [_batch(0)])
    assert np.isfinite(loss) and set(parts) == {"ce", "mse", "kd", "kd_displ"}
    assert all(np.isfinite(v) for v in parts.values()) and parts["kd"] > 0.0 and parts["kd_displ"] > 0.0
    assert abs(loss - (0.5 * parts["ce"] + parts["mse"] + 0.5 * parts["kd"] + 0.25 * parts["kd_displ"])) <= 1e-5 * max(1.0, abs(loss))


def test_the_double_head_with_options_is_refused():
    m = _model()
    m.loss_options(**OPTS)
    m._model.update_pred_head([2, 2])
    opt, _ = m.get_optimizer({"lr": 1e-3})
    with pytest.raises(ValueError, match="double head"):
        m.epoch([dict(_batch(0), dataset=torch.tensor([1, 2]))], optimizer=opt)
    with pytest.raises(ValueError, match="double head"):
        m.loss_options(focal_gamma=1.0)
    eng = opt.engine
    head = torch.zeros((12, eng.temporal.head_layout()[0] + 1), device=DEV)
    with pytest.raises(ValueError, match="double head"):
        eng.temporal.loss_fwd_bwd(head, 2, 6, torch.zeros(12, dtype=torch.int64, device=DEV), loss=dict(OPTS),
                                  dataset=torch.tensor([1, 2], device=DEV))


# ----------------------------------------------------------------------------- 4. the captured step
def test_captured_step_equals_the_eager_step_and_records_its_settings():
    b = _batch(0)
    frames, lab, labD = b["frame"].to(DEV), b["label"].to(DEV), b["labelD"].to(DEV)
    B, T = lab.shape
    loss = dict(OPTS, class_weights=[1.0, 2.0, 3.0, 4.0])
    engines = []
    for graph in (True, False):
        eng = _engine()
        step = eng.make_step(B, 64, 64, frames, lab, labD, None, use_graph=graph, loss=loss)
        out5 = step()
        assert tuple(out5.shape) == (5,) and bool(torch.isfinite(out5).all())
        step()
        torch.cuda.synchronize()
        engines.append(eng)
    a, e = engines
    assert a.opt.t == 2 and e.opt.t == 2
    for x, y, what in ((a.params.flat, e.params.flat, "flat"), (a.opt.exp_avg, e.opt.exp_avg, "m"),
                       (a.opt.exp_avg_sq, e.opt.exp_avg_sq, "v")):
        assert _same_bits(x, y), what
    # the options took effect: two plain steps end elsewhere
    c = _engine()
    step = c.make_step(B, 64, 64, frames, lab, labD, None, use_graph=False)
    step(), step()
    assert not _same_bits(c.params.flat, e.params.flat)
    # the handle records its settings: the same ones reuse it, others rebuild, and the stale handle refuses them
    h = a.last_graph
    assert h.loss_opt == dict(label_smoothing=0.1, focal_gamma=2.0, class_weights=(1.0, 2.0, 3.0, 4.0)) and h.kd is None
    a.make_step(B, 64, 64, frames, lab, labD, None, loss=dict(loss))
    assert a.last_graph is h
    other = dict(loss, focal_gamma=1.0)
    a.make_step(B, 64, 64, frames, lab, labD, None, loss=other)
    assert a.last_graph is not h and a.last_graph.loss_opt["focal_gamma"] == 1.0
    t_before = a.opt.t
    for kw in (dict(loss=other), dict(), dict(loss=dict(loss, class_weights=None))):
        with pytest.raises(RuntimeError, match="other loss options"):
            a.step_graph(h, frames, lab, labD, **kw)
    a.make_step(B, 64, 64, frames, lab, labD, None)
    with pytest.raises(RuntimeError, match="other loss options"):
        a.step_graph(a.last_graph, frames, lab, labD, loss=loss)     # a plain handle called with options
    assert a.opt.t == t_before                                   # the refused calls ran nothing
