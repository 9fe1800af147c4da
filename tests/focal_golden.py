"""Float64 restatement, in plain torch, of the fused focal head's formulas (include/cabinet_hip.h).

With z the low logits, U the bilinear upsample (align_corners=False), t the label, per valid pixel
    l = lse(Uz) - (Uz)_t,  p = exp(-l),  q = 1 - p = -expm1(-l)
and per head  D = sum w_t,  S = sum w_t q^gamma l,  loss = S / D,
    a = q^gamma + gamma p q^(gamma-1) l = q^gamma (1 + gamma p l / q),     dloss/dz = (g / D) U^T[w_t a (softmax - onehot)].
Pinned: q^0 = 1 also at q = 0; gamma > 0 and q = 0: term and a are 0.  Autograd is used for the LINEAR map U^T only; the
per-pixel factor is the closed form above, not the derivative of anything."""
import torch
import torch.nn.functional as F


def focal_q_pow_a(l, gamma):
    """q, q^gamma and a for a float64 tensor of per-pixel l."""
    q = (-torch.expm1(-l)).clamp_min(0.0)
    pos = q > 0
    qs = torch.where(pos, q, torch.ones_like(q))
    if gamma == 0:
        qg = torch.ones_like(q)
    else:
        qg = torch.where(pos, qs ** gamma, torch.zeros_like(q))
    a = torch.where(pos, qg * (1.0 + gamma * (1.0 - q) * l / qs), qg)
    return q, qg, a


def focal_up_ref(low, labels, size, gamma, weight=None, ignore_lb=255, upstream=1.0):
    """-> loss (python float, NaN when D == 0), dlow (float64, exactly 0 when D == 0), (n_valid, D, S)."""
    z = low.detach().double().cpu().requires_grad_(True)
    labels = labels.cpu()
    C = z.shape[1]
    up = F.interpolate(z, size=tuple(size), mode="bilinear", align_corners=False)
    valid = labels != ignore_lb
    t = torch.where(valid, labels, torch.zeros_like(labels)).clamp(0, C - 1)
    x = up.detach()
    lse = torch.logsumexp(x, dim=1)
    l = lse - x.gather(1, t.unsqueeze(1)).squeeze(1)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().double().cpu()
    wt = torch.where(valid, w[t], torch.zeros_like(l))
    _, qg, a = focal_q_pow_a(l, float(gamma))
    D = float(wt.sum())
    S = float((wt * qg * l).sum())
    n_valid = int(valid.sum())
    if D > 0:
        soft = torch.softmax(x, dim=1)
        onehot = F.one_hot(t, C).permute(0, 3, 1, 2).double()
        G = (wt * a).unsqueeze(1) * (soft - onehot) * (float(upstream) / D)
        (dlow,) = torch.autograd.grad(up, z, G)   # U^T G
        loss = S / D
    else:
        dlow = torch.zeros_like(z)
        loss = float("nan")
    return loss, dlow.detach(), (n_valid, D, S)
