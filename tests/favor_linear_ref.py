"""The formulas of csrc/favor_linear.h restated in plain torch, float64, no autograd: what the kernels are written from.
tests/test_favor_linear_cpu.py holds this restatement against the autograd reference (oracle/ref_cpu.py::favor_attention), which makes
the formulas - derived by hand - the contract.

Notation favor.h's, per (task, head):  E = ratio exp(dd - diag - stab),  F = E + re,  re = ratio 1e-4;  the row maximum stabilises a
query row, the maximum over the WHOLE batch every key.  Centre c[e] = v[first shot, e].
"""
import torch

EPS = 1e-4


def features(x, proj, is_query):
    """x [T,H,N,d] -> (E [T,H,N,m], dd): E = ratio exp(dd - diag - stab)."""
    d, m = x.shape[-1], proj.shape[0]
    c, ratio = d ** -0.25, m ** -0.5
    dd = torch.einsum("thnd,md->thnm", c * x, proj)
    diag = (x * x).sum(-1, keepdim=True) * 0.5 * c * c
    stab = dd.max(dim=-1, keepdim=True).values if is_query else dd.max()
    return ratio * torch.exp(dd - diag - stab), dd


def forward(q, k, v, proj):
    """-> out [T,H,Nq,d] and what the backward keeps."""
    m = proj.shape[0]
    re = m ** -0.5 * EPS
    Eq, ddq = features(q, proj, True)
    Ek, ddk = features(k, proj, False)
    Fq, Fk = Eq + re, Ek + re
    c = v[:, :, :1]                                            # the centre: the first shot's value row
    ksum = Fk.sum(dim=2)                                       # [T,H,m]
    Ctx = torch.einsum("thnj,thne->thje", Fk, v - c)           # [T,H,m,d]
    D = torch.einsum("thqj,thj->thq", Fq, ksum)                # [T,H,Nq]
    out = c + torch.einsum("thqj,thje->thqe", Fq, Ctx) / D[..., None]
    return out, dict(Eq=Eq, Ek=Ek, Fq=Fq, Fk=Fk, ddq=ddq, ddk=ddk, c=c, ksum=ksum, Ctx=Ctx, D=D, out=out)


def backward(q, k, v, proj, s, dO):
    """dO [T,H,Nq,d] -> dq, dk, dv.  The gradient with respect to the centre is identically zero (sum_j F_q ksum = D): no term for it."""
    d = q.shape[-1]
    cn = d ** -0.25
    u = s["out"] - s["c"]
    g = dO / s["D"][..., None]
    w = (g * u).sum(-1)                                                                   # [T,H,Nq]
    dFq = torch.einsum("thqe,thje->thqj", g, s["Ctx"]) - w[..., None] * s["ksum"][:, :, None, :]
    dCtx = torch.einsum("thqj,thqe->thje", s["Fq"], g)
    dks = -torch.einsum("thqj,thq->thj", s["Fq"], w)
    dFk = torch.einsum("thje,thne->thnj", dCtx, v - s["c"]) + dks[:, :, None, :]
    dv = torch.einsum("thnj,thje->thne", s["Fk"], dCtx)
    Gq, Gk = dFq * s["Eq"], dFk * s["Ek"]
    rs_q, rs_k = Gq.sum(-1), Gk.sum(-1)
    # the stabilisers' gradients: a query row's sum goes to the row's (first) arg-max, the batch-wide sum to THE arg-max key element
    ddd_q = Gq.clone()
    ddd_q.scatter_add_(-1, s["ddq"].argmax(dim=-1, keepdim=True), -rs_q[..., None])
    ddd_k = Gk.clone()
    ddd_k.view(-1)[s["ddk"].argmax()] -= rs_k.sum()
    dq = cn * torch.einsum("thnj,jd->thnd", ddd_q, proj) - cn * cn * q * rs_q[..., None]
    dk = cn * torch.einsum("thnj,jd->thnd", ddd_k, proj) - cn * cn * k * rs_k[..., None]
    return dq, dk, dv


def run(x, dtype=torch.float64):
    """inputs (q, k, v, wout, proj) -> {out, dq, dk, dv} for the loss (out * wout).sum()."""
    q, k, v, wout, proj = (t.to(dtype) for t in (x.q, x.k, x.v, x.wout, x.proj))
    out, s = forward(q, k, v, proj)
    dq, dk, dv = backward(q, k, v, proj, s, wout)
    return dict(out=out, dq=dq, dk=dk, dv=dv)
