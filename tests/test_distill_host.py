"""Distillation without a GPU: `losses.kd_ref` against fp64 autograd of the formula, its alpha = 0 and teacher = student
ends, and the argument errors of `ops.loss_kd` and `TDEEDModel.distill_from` (CPU-constructed models)."""
import pytest
import torch

import distill_cases as D
from helpers import cfg_ns
from tdeed_amd import losses, ops

CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)


def _kd_ref(c, kind, tau, alpha, beta, teacher=None, dtype=torch.float32):
    kw = {k: v.to(dtype) if k == "soft" else v for k, v in D.label_kw(c, kind).items()}
    return losses.kd_ref(c["head"].to(dtype), c["K1"], c["cls_w"].to(dtype), (c["teacher"] if teacher is None else teacher).to(dtype),
                         displ_col=c["displ_col"], labelD=c["labelD"], teacher_displ_col=c["teacher_displ_col"], alpha=alpha,
                         temperature=tau, displ_weight=beta, grad_scale=D.GRAD_SCALE, **kw)


@pytest.mark.parametrize("kind", ["hard", "soft"])
@pytest.mark.parametrize("shape", D.SHAPES)
def test_kd_ref_against_fp64_autograd(shape, kind):
    c = D.case(*shape)
    worst = (0.0, 0.0)
    for tau, alpha, beta in D.SETTINGS:
        out5, dhead = _kd_ref(c, kind, tau, alpha, beta)
        assert out5.dtype == torch.float32 and dhead.dtype == torch.float32 and dhead.shape == c["head"].shape
        ev, eg = D.assert_within(out5, dhead, *D.formula64(c, kind, tau, alpha, beta), (shape, kind, tau, alpha, beta))
        worst = (max(worst[0], ev), max(worst[1], eg))
    print(f"kd_ref fp32 vs fp64 autograd {shape} {kind}: value {worst[0]:.2e}, gradient {worst[1]:.2e}")


def test_kd_ref_works_in_fp64():
    c = D.case(60, 5)
    out5, dhead = _kd_ref(c, "soft", 2.0, 0.5, 0.25, dtype=torch.float64)
    ref5, refg = D.formula64(c, "soft", 2.0, 0.5, 0.25)
    assert out5.dtype == torch.float64 and float((out5 - ref5).abs().max()) < 1e-12 and float((dhead - refg).abs().max()) < 1e-13


@pytest.mark.parametrize("kind", ["hard", "soft"])
@pytest.mark.parametrize("shape", D.SHAPES)
def test_alpha_zero_is_the_plain_loss(shape, kind):
    """alpha = 0, displ_weight = 0: ce, mse, total and the gradient are the plain loss's numbers (a zero's sign apart)."""
    c = D.case(*shape)
    ce, mse, plain = losses.plain_ref(c["head"], c["K1"], c["cls_w"], displ_col=c["displ_col"], labelD=c["labelD"],
                                      grad_scale=D.GRAD_SCALE, **D.label_kw(c, kind))
    for tau in D.TAUS:
        out5, dhead = _kd_ref(c, kind, tau, 0.0, 0.0)
        assert torch.equal(out5[1], ce) and torch.equal(out5[2], mse) and torch.equal(out5[0], ce + mse)
        assert torch.equal(dhead, plain)
        assert float(out5[3]) > 0.0                              # kd is still reported


@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_teacher_equal_to_the_student(kind):
    for shape in D.SHAPES:
        c = D.case(*shape)
        _, _, plain = losses.plain_ref(c["head"], c["K1"], c["cls_w"], displ_col=c["displ_col"], labelD=c["labelD"],
                                       grad_scale=D.GRAD_SCALE, **D.label_kw(c, kind))
        for tau, alpha in ((1.0, 0.5), (2.0, 1.0), (4.0, 0.25)):
            out5, dhead = _kd_ref(c, kind, tau, alpha, 0.0, teacher=c["head"])
            assert abs(float(out5[3])) <= 1e-6 and float(out5[4]) == 0.0
            want = (1.0 - alpha) * plain
            want[:, c["displ_col"]] = plain[:, c["displ_col"]]
            assert float((dhead - want).abs().max()) <= 1e-7, (shape, tau, alpha)


def test_loss_kd_argument_errors():
    c = D.case(16, 2)
    head, tch, w, K1 = c["head"], c["teacher"], c["cls_w"], c["K1"]
    ok = dict(hard=c["hard"], displ_col=2, labelD=c["labelD"], teacher_displ_col=2)
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
               dict(temperature=float("inf")), dict(displ_weight=-0.5)):
        with pytest.raises(ValueError, match="alpha|temperature|displ_weight"):
            ops.loss_kd(head, K1, w, tch, **{**ok, **kw})
    with pytest.raises(ValueError, match="both heads"):
        ops.loss_kd(head, K1, w, tch, **{**ok, "teacher_displ_col": -1, "displ_weight": 0.5})
    with pytest.raises(ValueError, match="both heads"):
        ops.loss_kd(head, K1, w, tch, **{**ok, "displ_col": -1, "displ_weight": 0.5})
    with pytest.raises(ValueError, match="rows"):
        ops.loss_kd(head, K1, w, tch[:-1], **ok)
    with pytest.raises(ValueError, match="classes"):
        ops.loss_kd(head, K1, w, tch[:, :1], **{**ok, "teacher_displ_col": -1})       # K1 > ld_t
    with pytest.raises(ValueError, match="displacement columns"):
        ops.loss_kd(head, K1, w, tch, **{**ok, "teacher_displ_col": 3})
    with pytest.raises(ValueError, match="weights"):
        ops.loss_kd(head, K1, w[:1], tch, **ok)
    with pytest.raises(ValueError, match="both heads"):
        losses.kd_ref(head, K1, w, tch, hard=c["hard"], displ_col=2, displ_weight=0.5)
    # past the value checks a CPU tensor is refused like in every other wrapper: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.loss_kd(head, K1, w, tch, **ok)


def _cpu_model(**over):
    from tdeed_amd.model import TDEEDModel
    return TDEEDModel(device="cpu", args=cfg_ns(dict(CFG, **over)))


def test_distill_from_argument_errors(capsys):
    m, teacher = _cpu_model(), _cpu_model(feature_arch="rny008_gsf")
    assert m.loss_parts is None and m._kd is None
    for kw in (dict(alpha=-0.1), dict(alpha=1.1), dict(temperature=0.0), dict(displ_weight=-1.0)):
        with pytest.raises(ValueError, match="alpha|temperature|displ_weight"):
            m.distill_from(teacher, **kw)
    with pytest.raises(ValueError, match="own teacher"):
        m.distill_from(m)
    with pytest.raises(ValueError, match="classes"):
        m.distill_from(_cpu_model(num_classes=4))
    with pytest.raises(ValueError, match="clip_len"):
        m.distill_from(_cpu_model(clip_len=8))
    with pytest.raises(ValueError, match="displacement head"):
        m.distill_from(_cpu_model(radi_displacement=0), displ_weight=0.5)
    with pytest.raises(ValueError, match="displacement head"):
        _cpu_model(radi_displacement=0).distill_from(teacher, displ_weight=0.5)
    with pytest.raises(ValueError, match="teacher_dtype"):
        m.distill_from(teacher, teacher_dtype=torch.float16)
    two = _cpu_model()
    two._model.update_pred_head([2, 2])
    with pytest.raises(ValueError, match="double head"):
        m.distill_from(two)
    with pytest.raises(ValueError, match="double head"):
        two.distill_from(teacher)
    assert m._kd is None and not m._model._kd_wanted                 # nothing was set by the refused calls
    # a teacher without a displacement head is fine as long as displ_weight is 0
    assert m.distill_from(_cpu_model(radi_displacement=0)) is m
    keys = list(m.state_dict())
    m.distill_from(teacher, alpha=0.3, temperature=3.0, displ_weight=0.5, teacher_dtype=torch.float32)
    assert m._kd[0] is teacher and m._kd[1] == torch.float32
    assert m._kd[2] == dict(alpha=0.3, temperature=3.0, displ_weight=0.5) and m._model._kd_wanted
    assert list(m.state_dict()) == keys                              # the settings are not part of the state
    m.loss_parts = dict(ce=0.0, mse=0.0, kd=0.0, kd_displ=0.0)       # (what a training epoch leaves)
    m.distill_from(None)
    assert m.loss_parts is None and m._kd is None and m._kd_last is None and not m._model._kd_wanted


def test_kd_settings_of_the_captured_step():
    from tdeed_amd.trainer import kd_settings
    assert kd_settings(None) is None
    tch = torch.zeros(12, 5)
    want = dict(ld_t=5, displ_col_t=4, alpha=0.5, temperature=2.0, displ_weight=0.0)
    assert kd_settings(dict(teacher=tch, displ_col_t=4), tch) == want and kd_settings(dict(ld_t=5, displ_col_t=4)) == want
    assert kd_settings(dict(want, alpha=0.25)) != want
    for bad in (dict(displ_col_t=4), dict(ld_t=5, alpha=2.0), dict(ld_t=5, tau=1.0)):
        with pytest.raises(ValueError):
            kd_settings(bad)
    with pytest.raises(ValueError):
        kd_settings(dict(ld_t=4), tch)
    with pytest.raises(ValueError):
        kd_settings(None, tch)
