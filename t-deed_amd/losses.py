"""Host restatements (torch on the CPU, any floating dtype) of the loss kernels: the tests' oracle next to fp64 autograd.

`plain_ref` is the weighted cross-entropy + displacement MSE of `ops.loss` / `ops.loss_bwd` with its analytic gradient;
`kd_ref` is the distillation loss of `ops.loss_kd` built on top of it, term for term as the kernel states it; `opt_ref` is
`ops.loss_opt`: label smoothing, the focal exponent and free class weights on the classification term, with or without the
distillation terms."""
import torch

from .ops import check_kd, check_loss_options


def _rows(head_out, K1, cls_w, hard, soft, labelD):
    if head_out.is_cuda:
        raise TypeError("the host restatements take CPU tensors")
    if (hard is None) == (soft is None):
        raise ValueError("loss needs hard or soft labels (one of them)")
    rows = head_out.shape[0]
    dt = head_out.dtype
    w = cls_w.to(dt)[:K1]
    if soft is not None:
        soft = soft.to(dt).reshape(rows, K1)
    if hard is not None:
        hard = hard.reshape(rows).long()
    if labelD is not None:
        labelD = labelD.to(dt).reshape(rows)
    return rows, dt, w, hard, soft, labelD


def plain_ref(head_out, K1, cls_w, hard=None, soft=None, displ_col=-1, labelD=None, grad_scale=1.0):
    """-> (ce, mse, dhead): F.cross_entropy(weight=cls_w) on hard labels (denominator sum_r w[y_r]) or on soft label
    distributions (denominator rows), F.mse_loss of the displacement column, and grad_scale * d(ce + mse)/d(head_out) with
    zeros in the columns outside the loss."""
    rows, dt, w, hard, soft, labelD = _rows(head_out, K1, cls_w, hard, soft, labelD)
    s = head_out[:, :K1]
    logp = torch.log_softmax(s, dim=1)
    p = logp.exp()
    dhead = torch.zeros_like(head_out)
    if soft is not None:
        ce = -(w * soft * logp).sum() / rows
        wp = (w * soft).sum(dim=1, keepdim=True)
        dhead[:, :K1] = (p * wp - w * soft) * (grad_scale / rows)
    else:
        wy = w[hard]
        den = wy.sum()
        ce = -(wy * logp[torch.arange(rows), hard]).sum() / den
        oh = torch.nn.functional.one_hot(hard, K1).to(dt)
        dhead[:, :K1] = wy[:, None] * (p - oh) * (grad_scale / den)
    mse = torch.zeros((), dtype=dt)
    if displ_col >= 0 and labelD is not None:
        d = head_out[:, displ_col] - labelD
        mse = (d * d).sum() / rows
        dhead[:, displ_col] = 2.0 * d * (grad_scale / rows)
    return ce, mse, dhead


def kd_ref(head_out, K1, cls_w, teacher, hard=None, soft=None, displ_col=-1, labelD=None, teacher_displ_col=-1, alpha=0.5,
           temperature=2.0, displ_weight=0.0, grad_scale=1.0):
    """`ops.loss_kd` on the host -> (out5 [total, ce, mse, kd, kd_displ], dhead), in head_out's dtype:
    total = (1-alpha) ce + mse + alpha kd + displ_weight kd_displ,
    kd = temperature^2 / rows * sum q (log q - log p) with p = softmax(head_out[:, :K1] / temperature) and
    q = softmax(teacher[:, :K1] / temperature), kd_displ = mean (d - d_teacher)^2 when both displacement columns exist."""
    alpha, tau, beta = check_kd(alpha, temperature, displ_weight)
    both_d = displ_col >= 0 and teacher_displ_col >= 0
    if beta > 0.0 and not both_d:
        raise ValueError("kd_ref: displ_weight > 0 needs a displacement column in both heads")
    rows, dt = head_out.shape[0], head_out.dtype
    teacher = teacher.to(dt)
    ce, mse, plain = plain_ref(head_out, K1, cls_w, hard, soft, displ_col, labelD, grad_scale)
    logp = torch.log_softmax(head_out[:, :K1] / tau, dim=1)
    logq = torch.log_softmax(teacher[:, :K1] / tau, dim=1)
    q = logq.exp()
    kd = (q * (logq - logp)).sum() * (tau * tau / rows)
    dhead = (1.0 - alpha) * plain
    dhead[:, :K1] += (alpha * tau * grad_scale / rows) * (logp.exp() - q)
    kdd = torch.zeros((), dtype=dt)
    if displ_col >= 0:
        dhead[:, displ_col] = plain[:, displ_col]                 # the MSE term is not scaled by (1-alpha)
        if both_d:
            e = head_out[:, displ_col] - teacher[:, teacher_displ_col]
            kdd = (e * e).sum() / rows
            dhead[:, displ_col] += (2.0 * beta * grad_scale / rows) * e
    total = (1.0 - alpha) * ce + mse + alpha * kd + beta * kdd
    return torch.stack([total, ce, mse, kd, kdd]), dhead


def opt_ref(head_out, K1, cls_w, teacher=None, hard=None, soft=None, displ_col=-1, labelD=None, teacher_displ_col=-1, alpha=0.0,
            temperature=1.0, displ_weight=0.0, label_smoothing=0.0, focal_gamma=0.0, grad_scale=1.0):
    """`ops.loss_opt` on the host -> (out5 [total, ce, mse, kd, kd_displ], dhead), in head_out's dtype.  Per row
    logp = log_softmax(s), p = exp(logp), q = -expm1(logp), t' = (1-eps) t + eps / K1, a = w t':
        ce = sum a q^gamma (-logp) / den,   g = -a q^gamma (gamma p rho + 1),  rho = -logp / q (1 where q == 0),
        dlogit = (g - p sum_c g_c) grad_scale / den,
    den = sum_r w[y_r] (hard labels) or rows (soft labels); terms with a == 0 contribute exactly 0.  The mse, kd and
    kd_displ terms and the blend are `kd_ref`'s; without a teacher kd = kd_displ = 0."""
    eps, gamma, _ = check_loss_options(label_smoothing, focal_gamma)
    rows, dt, w, hard, soft, labelD = _rows(head_out, K1, cls_w, hard, soft, labelD)
    if teacher is None:
        if float(alpha) != 0.0 or float(displ_weight) != 0.0:
            raise ValueError("opt_ref: alpha / displ_weight without a teacher")
        alpha, tau, beta = 0.0, 1.0, 0.0
    else:
        alpha, tau, beta = check_kd(alpha, temperature, displ_weight)
        teacher = teacher.to(dt)
    both_d = teacher is not None and displ_col >= 0 and teacher_displ_col >= 0
    if beta > 0.0 and not both_d:
        raise ValueError("opt_ref: displ_weight > 0 needs a displacement column in both heads")
    s = head_out[:, :K1]
    logp = torch.log_softmax(s, dim=1)
    p = logp.exp()
    if soft is not None:
        t, den = soft, torch.tensor(float(rows), dtype=dt)
    else:
        t, den = torch.nn.functional.one_hot(hard, K1).to(dt), w[hard].sum()
    a = w * ((1.0 - eps) * t + eps / K1)
    on = a != 0
    if gamma == 0.0:
        f, h = torch.ones_like(p), torch.ones_like(p)
    else:
        q = -torch.expm1(logp)
        rho = torch.where(q > 0, -logp / torch.where(q > 0, q, torch.ones_like(q)), torch.ones_like(q))
        f, h = q.pow(gamma), gamma * p * rho + 1.0
    zero = torch.zeros_like(p)
    ce = torch.where(on, a * f * (-logp), zero).sum() / den
    g = torch.where(on, -(a * f) * h, zero)
    dhead = torch.zeros_like(head_out)
    dhead[:, :K1] = (g - p * g.sum(dim=1, keepdim=True)) * (grad_scale / den)
    mse = torch.zeros((), dtype=dt)
    kd, kdd = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt)
    if teacher is not None:
        lps = torch.log_softmax(s / tau, dim=1)
        lqt = torch.log_softmax(teacher[:, :K1] / tau, dim=1)
        qt = lqt.exp()
        kd = (qt * (lqt - lps)).sum() * (tau * tau / rows)
        dhead[:, :K1] = (1.0 - alpha) * dhead[:, :K1] + (alpha * tau * grad_scale / rows) * (lps.exp() - qt)
    if displ_col >= 0:
        if labelD is not None:
            d = head_out[:, displ_col] - labelD
            mse = (d * d).sum() / rows
            dhead[:, displ_col] = 2.0 * d * (grad_scale / rows)
        if both_d:
            e = head_out[:, displ_col] - teacher[:, teacher_displ_col]
            kdd = (e * e).sum() / rows
            dhead[:, displ_col] += (2.0 * beta * grad_scale / rows) * e
    total = (1.0 - alpha) * ce + mse + alpha * kd + beta * kdd
    return torch.stack([total, ce, mse, kd, kdd]), dhead
