"""Cases, the fp64 reference and the bounds that tests/test_loss_options_host.py and tests/test_gpu_loss_options.py share.

The conventions are those of tests/distill_cases.py (its shapes, student logits of scale 2, GRAD_SCALE, class weights
[1, 5, ...], its bounds); on top of them one row, a head with unused columns (ld > K1 + 1), a head without a displacement
column, a saturated head [[100, 0, -100]] (label 0: p_y == 1 in fp32 and in fp64; label 2: p_y == 0) and a class weight
vector with a zero in it.

The reference is fp64 autograd of the classification term written with torch's own functions --
    gamma == 0:  F.cross_entropy(weight=w, label_smoothing=eps)
    gamma  > 0:  sum_r sum_c w_c t'_c (1 - p_c)^gamma (-log p_c) / den,  t' = (1 - eps) t + eps / K1,
                 den = sum_r w[y_r] (hard labels) or rows (soft labels)
-- plus the mse / kd / kd_displ terms of distill_cases.formula64: total = that formula's total + (1 - alpha) (ce - its ce).
Where 1 - p_c rounds to 0 in fp64 (the saturated row's own class) the focal term and its gradient are set to their limit
0 for gamma > 0: autograd through pow(0, gamma < 1) would give inf * 0.

Bounds (distill_cases): every value within 1e-5 * max(1, |ref|), every gradient element within 1e-6."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import distill_cases as D

EPSILONS = [0.0, 0.1, 1.0]
GAMMAS = [0.0, 0.5, 1.0, 2.0, 5.0]
KINDS = ["hard", "soft"]
SETTINGS = list(itertools.product(EPSILONS, GAMMAS))
GRAD_SCALE = D.GRAD_SCALE
KD = dict(tau=2.0, alpha=0.5, beta=0.25)                       # the distillation settings of the cases with a teacher
CASES = ["60x5", "16x2", "257x33", "1x5", "wide", "no_displ", "sat0", "sat2", "zero_weight"]
ZERO_WEIGHTS = [0.5, 0.0, 2.0, 1.0, 3.0]


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs of one case, built once and left unchanged (fp32, CPU): the keys of distill_cases.case."""
    if "x" in name:
        rows, K1 = (int(v) for v in name.split("x"))
        return D.case(rows, K1)
    if name == "no_displ":
        return D.case(60, 5, False, True)
    if name == "zero_weight":
        return dict(D.case(60, 5), cls_w=torch.tensor(ZERO_WEIGHTS, dtype=torch.float32))
    if name == "wide":
        # two unused columns between the logits and the displacement column: their gradient must come back 0
        c = D.case(60, 5)
        rng = np.random.default_rng(77)
        extra = torch.from_numpy(rng.standard_normal((60, 2)).astype(np.float32))
        head = torch.cat([c["head"][:, :5], extra, c["head"][:, 5:]], dim=1).contiguous()
        return dict(c, head=head, displ_col=7)
    if name in ("sat0", "sat2"):
        rng = np.random.default_rng(78)
        soft = torch.softmax(torch.from_numpy(rng.standard_normal((1, 3)).astype(np.float32)) * 2.0, dim=1).contiguous()
        teacher = torch.from_numpy(rng.standard_normal((1, 3)).astype(np.float32)) * 4.0
        return dict(rows=1, K1=3, head=torch.tensor([[100.0, 0.0, -100.0]]), teacher=teacher,
                    hard=torch.tensor([0 if name == "sat0" else 2]), soft=soft, labelD=None,
                    cls_w=torch.tensor([1.0, D.FG_WEIGHT, D.FG_WEIGHT]), displ_col=-1, teacher_displ_col=-1)
    raise KeyError(name)


def beta_of(c):
    return KD["beta"] if c["displ_col"] >= 0 and c["teacher_displ_col"] >= 0 else 0.0


@functools.lru_cache(maxsize=None)
def ce64(name, kind, eps, gamma):
    """-> (ce fp64, d ce / d head fp64) by autograd"""
    c = case(name)
    K1, rows = c["K1"], c["rows"]
    head = c["head"].double().requires_grad_(True)
    s, w = head[:, :K1], c["cls_w"].double()
    target = c["hard"] if kind == "hard" else c["soft"].double()
    if gamma == 0.0:
        ce = F.cross_entropy(s, target, weight=w, label_smoothing=eps)
    else:
        logp = F.log_softmax(s, dim=1)
        q = 1.0 - logp.exp()
        t = F.one_hot(c["hard"], K1).double() if kind == "hard" else target
        den = w[c["hard"]].sum() if kind == "hard" else float(rows)
        live = q > 0
        term = w * ((1.0 - eps) * t + eps / K1) * torch.where(live, q, torch.ones_like(q)).pow(gamma) * (-logp)
        ce = torch.where(live, term, torch.zeros_like(term)).sum() / den
    ce.backward()
    return ce.detach(), head.grad


@functools.lru_cache(maxsize=None)
def _rest64(name, kind, tau, alpha, beta):
    return D.formula64(case(name), kind, tau, alpha, beta, grad_scale=GRAD_SCALE)


@functools.lru_cache(maxsize=None)
def formula64(name, kind, eps, gamma, teacher=True):
    """-> (values fp64 [total, ce, mse, kd, kd_displ], d(GRAD_SCALE * total)/d(head) fp64); teacher=False: no distillation
    terms (alpha = displ_weight = 0, kd = kd_displ = 0)."""
    c = case(name)
    tau, alpha, beta = (KD["tau"], KD["alpha"], beta_of(c)) if teacher else (1.0, 0.0, 0.0)
    v, g = _rest64(name, kind, tau, alpha, beta)
    ce, gce = ce64(name, kind, eps, gamma)
    ce0, gce0 = ce64(name, kind, 0.0, 0.0)
    v = v.clone()
    v[0] = v[0] + (1.0 - alpha) * (ce - ce0)
    v[1] = ce
    if not teacher:
        v[3:] = 0.0
    return v, g + (1.0 - alpha) * GRAD_SCALE * (gce - gce0)


def opt_kw(c, kind, eps, gamma, teacher=True, dtype=None):
    """keyword arguments of ops.loss_opt / losses.opt_ref after (head_out, K1, cls_w) for one case"""
    cast = (lambda x: x) if dtype is None else (lambda x: None if x is None else x.to(dtype))
    kw = dict(displ_col=c["displ_col"], labelD=cast(c["labelD"]), label_smoothing=eps, focal_gamma=gamma, grad_scale=GRAD_SCALE)
    kw.update(dict(hard=c["hard"]) if kind == "hard" else dict(soft=cast(c["soft"])))
    if teacher:
        kw.update(teacher=cast(c["teacher"]), teacher_displ_col=c["teacher_displ_col"], alpha=KD["alpha"],
                  temperature=KD["tau"], displ_weight=beta_of(c))
    return kw
