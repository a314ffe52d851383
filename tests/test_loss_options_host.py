"""The loss options without a GPU: `losses.opt_ref` against fp64 autograd of the formula (fp64 within 1e-12, fp32 within the
project's bounds), its neutral end against `plain_ref` / `kd_ref`, the saturated rows, and the argument errors of
`ops.check_loss_options`, `trainer.loss_settings` and `TDEEDModel.loss_options` (CPU-constructed models).
Cases, reference and bounds: tests/loss_option_cases.py."""
import pytest
import torch

import distill_cases as D
import loss_option_cases as L
from helpers import cfg_ns
from tdeed_amd import losses, ops

CFG = dict(feature_arch="rny002_gsf", clip_len=6, crop_dim=None, n_layers=2, sgp_ks=5, sgp_r=2, num_classes=3,
           radi_displacement=2)


def _opt_ref(name, kind, eps, gamma, teacher, dtype):
    c = L.case(name)
    return losses.opt_ref(c["head"].to(dtype), c["K1"], c["cls_w"].to(dtype), **L.opt_kw(c, kind, eps, gamma, teacher, dtype))


@pytest.mark.parametrize("teacher", [False, True])
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", L.CASES)
def test_opt_ref_fp64_against_autograd(name, kind, teacher):
    worst = (0.0, 0.0)
    for eps, gamma in L.SETTINGS:
        out5, dhead = _opt_ref(name, kind, eps, gamma, teacher, torch.float64)
        ref5, refg = L.formula64(name, kind, eps, gamma, teacher)
        assert out5.dtype == torch.float64 and dhead.shape == refg.shape
        ev, eg = float((out5 - ref5).abs().max()), float((dhead - refg).abs().max())
        assert bool(torch.isfinite(out5).all()) and ev < 1e-12 and eg < 1e-12, (name, kind, eps, gamma, ev, eg)
        worst = (max(worst[0], ev), max(worst[1], eg))
    print(f"opt_ref fp64 vs autograd {name} {kind} teacher={teacher}: value {worst[0]:.2e}, gradient {worst[1]:.2e}")


@pytest.mark.parametrize("teacher", [False, True])
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", L.CASES)
def test_opt_ref_fp32_within_the_bounds(name, kind, teacher):
    worst = (0.0, 0.0)
    for eps, gamma in L.SETTINGS:
        out5, dhead = _opt_ref(name, kind, eps, gamma, teacher, torch.float32)
        assert out5.dtype == torch.float32 and dhead.dtype == torch.float32
        ev, eg = D.assert_within(out5, dhead, *L.formula64(name, kind, eps, gamma, teacher), (name, kind, eps, gamma))
        worst = (max(worst[0], ev), max(worst[1], eg))
    print(f"opt_ref fp32 vs fp64 autograd {name} {kind} teacher={teacher}: value {worst[0]:.2e}, gradient {worst[1]:.2e}")


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("name", L.CASES)
def test_neutral_options_are_the_plain_and_the_kd_loss(name, kind):
    c = L.case(name)
    h, w = c["head"].double(), c["cls_w"].double()
    lab = dict(hard=c["hard"]) if kind == "hard" else dict(soft=c["soft"].double())
    labD = None if c["labelD"] is None else c["labelD"].double()
    ce, mse, plain = losses.plain_ref(h, c["K1"], w, displ_col=c["displ_col"], labelD=labD, grad_scale=L.GRAD_SCALE, **lab)
    out5, dhead = _opt_ref(name, kind, 0.0, 0.0, False, torch.float64)
    want = torch.stack([ce + mse, ce, mse, torch.zeros_like(ce), torch.zeros_like(ce)])
    assert float((out5 - want).abs().max()) < 1e-12 and float((dhead - plain).abs().max()) < 1e-12
    ref5, refd = losses.kd_ref(h, c["K1"], w, c["teacher"].double(), displ_col=c["displ_col"], labelD=labD,
                               teacher_displ_col=c["teacher_displ_col"], alpha=L.KD["alpha"], temperature=L.KD["tau"],
                               displ_weight=L.beta_of(c), grad_scale=L.GRAD_SCALE, **lab)
    out5, dhead = _opt_ref(name, kind, 0.0, 0.0, True, torch.float64)
    assert float((out5 - ref5).abs().max()) < 1e-12 and float((dhead - refd).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_saturated_rows_are_finite_at_every_gamma(dtype):
    for name, kind, (eps, gamma), teacher in [(n, k, s, t) for n in ("sat0", "sat2") for k in L.KINDS for s in L.SETTINGS
                                              for t in (False, True)]:
        out5, dhead = _opt_ref(name, kind, eps, gamma, teacher, dtype)
        assert bool(torch.isfinite(out5).all()) and bool(torch.isfinite(dhead).all()), (name, kind, eps, gamma, teacher)
    # p_y == 1 and nothing smoothed: the focal term and its gradient vanish exactly
    for gamma in L.GAMMAS[1:]:
        out5, dhead = _opt_ref("sat0", "hard", 0.0, gamma, False, dtype)
        assert float(out5[1]) == 0.0 and float(dhead.abs().max()) == 0.0
    # p_y == 0: the focal factor is 1, the value is the plain cross-entropy of that row
    for gamma in L.GAMMAS:
        out5, _ = _opt_ref("sat2", "hard", 0.0, gamma, False, dtype)
        assert float(out5[1]) == 200.0


def test_gamma_zero_is_torch_cross_entropy():
    """the formula at gamma = 0 against F.cross_entropy itself, hard labels with a zero weight included"""
    for name, kind, eps in [(n, k, e) for n in ("60x5", "zero_weight", "257x33") for k in L.KINDS for e in L.EPSILONS]:
        c = L.case(name)
        tgt = c["hard"] if kind == "hard" else c["soft"].double()
        want = torch.nn.functional.cross_entropy(c["head"][:, :c["K1"]].double(), tgt, weight=c["cls_w"].double(),
                                                 label_smoothing=eps)
        out5, _ = _opt_ref(name, kind, eps, 0.0, False, torch.float64)
        assert abs(float(out5[1] - want)) < 1e-12, (name, kind, eps)


def test_check_loss_options():
    assert ops.check_loss_options(0.1, 2, [1, 2.5, 0], 3) == (0.1, 2.0, (1.0, 2.5, 0.0))
    assert ops.check_loss_options(0, 0, None, 3) == (0.0, 0.0, None)
    assert ops.check_loss_options(1.0, 0.0, torch.tensor([1.0, 2.0]), 2)[2] == (1.0, 2.0)
    for bad, word in ((dict(label_smoothing=-0.1), "-0.1"), (dict(label_smoothing=1.5), "1.5"),
                      (dict(label_smoothing=float("nan")), "nan"), (dict(focal_gamma=-1.0), "-1.0"),
                      (dict(focal_gamma=float("nan")), "nan"), (dict(focal_gamma=float("inf")), "inf"),
                      (dict(class_weights=[1.0, 2.0]), r"\(2,\)"), (dict(class_weights=[[1.0, 2.0, 3.0]]), r"\(1, 3\)"),
                      (dict(class_weights=[1.0, -2.0, 3.0]), "-2.0"), (dict(class_weights=[1.0, float("nan"), 3.0]), "nan"),
                      (dict(class_weights=[1.0, float("inf"), 3.0]), "inf")):
        with pytest.raises(ValueError, match=word):
            ops.check_loss_options(**{**dict(label_smoothing=0.0, focal_gamma=0.0, class_weights=None, K1=3), **bad})


def test_loss_opt_argument_errors():
    c = L.case("16x2")
    head, w, K1 = c["head"], c["cls_w"], c["K1"]
    ok = dict(hard=c["hard"], displ_col=2, labelD=c["labelD"])
    for kw in (dict(label_smoothing=-0.1), dict(label_smoothing=2.0), dict(focal_gamma=-0.5), dict(focal_gamma=float("nan"))):
        with pytest.raises(ValueError, match="label_smoothing|focal_gamma"):
            ops.loss_opt(head, K1, w, **{**ok, **kw})
        with pytest.raises(ValueError, match="label_smoothing|focal_gamma"):
            losses.opt_ref(head, K1, w, **{**ok, **kw})
    with pytest.raises(ValueError, match="without a teacher"):
        ops.loss_opt(head, K1, w, alpha=0.5, **ok)
    with pytest.raises(ValueError, match="without a teacher"):
        ops.loss_opt(head, K1, w, displ_weight=0.5, **ok)
    with pytest.raises(ValueError, match="both heads"):
        ops.loss_opt(head, K1, w, c["teacher"], displ_weight=0.5, **ok)
    with pytest.raises(ValueError, match="alpha"):
        ops.loss_opt(head, K1, w, c["teacher"], alpha=1.5, **ok)
    with pytest.raises(ValueError, match="rows"):
        ops.loss_opt(head, K1, w, c["teacher"][:-1], **ok)
    with pytest.raises(ValueError, match="weights"):
        ops.loss_opt(head, K1, w[:1], **ok)
    with pytest.raises(ValueError, match="classes"):
        ops.loss_opt(head, 4, w, **ok)
    # past the value checks a CPU tensor is refused like in every other wrapper: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.loss_opt(head, K1, w, label_smoothing=0.1, focal_gamma=2.0, **ok)


def test_loss_settings_of_the_captured_step():
    from tdeed_amd.trainer import loss_settings
    assert loss_settings(None) is None
    want = dict(label_smoothing=0.1, focal_gamma=2.0, class_weights=None)
    assert loss_settings(dict(label_smoothing=0.1, focal_gamma=2)) == want
    assert loss_settings(dict(want, class_weights=[1, 2, 3]), 3) == dict(want, class_weights=(1.0, 2.0, 3.0))
    assert loss_settings(dict(want, focal_gamma=1.0)) != want
    assert loss_settings({}) == dict(label_smoothing=0.0, focal_gamma=0.0, class_weights=None)
    for bad in (dict(label_smoothing=1.5), dict(focal_gamma=-1.0), dict(gamma=2.0), dict(class_weights=[1.0, 2.0])):
        with pytest.raises(ValueError):
            loss_settings(bad, 3)


def _cpu_model(**over):
    from tdeed_amd.model import TDEEDModel
    return TDEEDModel(device="cpu", args=cfg_ns(dict(CFG, **over)))


def test_model_loss_options():
    m = _cpu_model()
    assert m._loss_opt is None
    for kw in (dict(label_smoothing=-0.1), dict(label_smoothing=1.1), dict(focal_gamma=-2.0), dict(focal_gamma=float("nan")),
               dict(class_weights=[1.0, 2.0]), dict(class_weights=[1.0, 2.0, -3.0, 4.0]),
               dict(class_weights=[1.0, 2.0, float("inf"), 4.0])):
        with pytest.raises(ValueError, match="label_smoothing|focal_gamma|class_weights"):
            m.loss_options(**kw)
    assert m._loss_opt is None                                       # nothing was set by the refused calls
    keys = list(m.state_dict())
    assert m.loss_options(label_smoothing=0.1, focal_gamma=2.0, class_weights=[1, 2, 3, 4]) is m
    assert m._loss_opt == dict(label_smoothing=0.1, focal_gamma=2.0, class_weights=(1.0, 2.0, 3.0, 4.0))
    assert list(m.state_dict()) == keys                              # the options are not part of the state
    m.loss_options(focal_gamma=1.0)
    assert m._loss_opt == dict(label_smoothing=0.0, focal_gamma=1.0, class_weights=None)
    m.loss_parts = dict(ce=0.0, mse=0.0)                             # (what a training epoch leaves)
    m.loss_options()
    assert m._loss_opt is None and m.loss_parts is None
    # the options and a teacher combine; clearing the options keeps the teacher
    teacher = _cpu_model(feature_arch="rny008_gsf")
    m.distill_from(teacher).loss_options(label_smoothing=0.1)
    assert m._kd is not None and m._loss_opt["label_smoothing"] == 0.1
    m.loss_options()
    assert m._kd is not None and m._loss_opt is None
    two = _cpu_model()
    two._model.update_pred_head([2, 2])
    with pytest.raises(ValueError, match="double head"):
        two.loss_options(focal_gamma=2.0)
    assert two.loss_options() is two                                 # clearing is always allowed
