"""Cases, the fp64 reference and the bounds that tests/test_distill_host.py and tests/test_gpu_distill.py share.

The reference is fp64 autograd of the formula written out with torch's own loss functions:
    total = (1-a) F.cross_entropy(weight=w) + F.mse_loss(displ) + a tau^2 F.kl_div(batchmean) + b F.mse_loss(d_s, d_t).
Bounds: every value within 1e-5 * max(1, |ref|), every gradient element within 1e-6 -- what tests/test_gpu_ops.py holds
the plain loss to, scaled for values above 1.  torch's own fp32 against fp64 gives 1.8e-6 / 1.6e-8 at these shapes."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = [(60, 5), (16, 2), (257, 33)]
TAUS = [1.0, 2.0, 4.0]
ALPHAS = [0.0, 0.5, 1.0]
BETAS = [0.0, 0.25]
GRAD_SCALE = 0.5
FG_WEIGHT = 5.0
VALUE_BOUND = 1e-5
GRAD_BOUND = 1e-6
SETTINGS = list(itertools.product(TAUS, ALPHAS, BETAS))


@functools.lru_cache(maxsize=None)
def case(rows, K1, s_displ=True, t_displ=True, t_extra=0):
    """Inputs of one shape, drawn once and left unchanged (fp32, CPU): student head (rows, ld) with logits of scale 2.0,
    teacher head (rows, ld_t) with logits of scale 4.0, hard and soft labels, displacement labels, class weights.
    t_extra: unused columns between the teacher's logits and its displacement column (ld_t != ld)."""
    rng = np.random.default_rng(9000 + 100 * rows + K1)
    ld = K1 + (1 if s_displ else 0)
    ld_t = K1 + t_extra + (1 if t_displ else 0)
    head = torch.from_numpy(rng.standard_normal((rows, ld)).astype(np.float32))
    head[:, :K1] *= 2.0
    teacher = torch.from_numpy(rng.standard_normal((rows, ld_t)).astype(np.float32))
    teacher[:, :K1] *= 4.0
    hard = torch.from_numpy(rng.integers(0, K1, rows).astype(np.int64))
    soft = torch.softmax(torch.from_numpy(rng.standard_normal((rows, K1)).astype(np.float32)) * 2.0, dim=1).contiguous()
    labelD = torch.from_numpy(rng.standard_normal(rows).astype(np.float32)) if s_displ else None
    cls_w = torch.tensor([1.0] + [FG_WEIGHT] * (K1 - 1), dtype=torch.float32)
    return dict(rows=rows, K1=K1, head=head, teacher=teacher, hard=hard, soft=soft, labelD=labelD, cls_w=cls_w,
                displ_col=K1 if s_displ else -1, teacher_displ_col=ld_t - 1 if t_displ else -1)


def label_kw(c, kind):
    return dict(hard=c["hard"]) if kind == "hard" else dict(soft=c["soft"])


def formula64(c, kind, tau, alpha, beta, grad_scale=GRAD_SCALE, teacher=None):
    """-> (values fp64 [total, ce, mse, kd, kd_displ], d(grad_scale * total)/d(head) fp64) by autograd."""
    K1 = c["K1"]
    head = c["head"].double().requires_grad_(True)
    tch = (c["teacher"] if teacher is None else teacher).double()
    w = c["cls_w"].double()
    s, t = head[:, :K1], tch[:, :K1]
    ce = F.cross_entropy(s, c["hard"] if kind == "hard" else c["soft"].double(), weight=w)
    zero = torch.zeros((), dtype=torch.float64)
    mse = F.mse_loss(head[:, c["displ_col"]], c["labelD"].double()) if c["displ_col"] >= 0 else zero
    kd = F.kl_div(F.log_softmax(s / tau, dim=1), F.softmax(t / tau, dim=1), reduction="batchmean") * tau ** 2
    both = c["displ_col"] >= 0 and c["teacher_displ_col"] >= 0
    kdd = F.mse_loss(head[:, c["displ_col"]], tch[:, c["teacher_displ_col"]]) if both else zero
    total = (1.0 - alpha) * ce + mse + alpha * kd + beta * kdd
    (total * grad_scale).backward()
    return torch.stack([total, ce, mse, kd, kdd]).detach(), head.grad


def errors(out5, dhead, ref5, refg):
    """-> (largest value error relative to max(1, |ref|), largest gradient element error)"""
    out5, ref5 = out5.detach().double().cpu(), ref5.double()
    ev = float(((out5 - ref5).abs() / ref5.abs().clamp(min=1.0)).max())
    eg = 0.0 if dhead is None else float((dhead.detach().double().cpu() - refg).abs().max())
    return ev, eg


def assert_within(out5, dhead, ref5, refg, what):
    ev, eg = errors(out5, dhead, ref5, refg)
    assert bool(torch.isfinite(out5).all()) and ev <= VALUE_BOUND and eg <= GRAD_BOUND, (what, ev, eg)
    return ev, eg
