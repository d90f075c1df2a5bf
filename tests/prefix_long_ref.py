"""Float64 statements of FAVOR+ over context prefixes of any length (csrc/favor_prefix_long.h) and the inputs the
prefix-long tests share.  Layout [T, H, N, d] like oracle.ref_cpu.

`direct` IS the definition: per prefix size kk the attention of tests/favor_cached_ref.py on the first kk shots (task t's first
min(kk, lens[t])), with the key stabiliser M_kk = the maximum of dd over the valid shots < kk of ALL tasks, heads and features.
`streamed` restates the kernel's walk: chunks of 32 shots in ascending order, per shot the running maximum Mref[n], carried sums P, p,
vs, cnt relative to the running maximum at the end of the last chunk, rescaled by exp(M_old - M_new) <= 1; a prefix that ends inside a
chunk weights column n by exp(Mref[n] - M_kk), adds eps rowsum(F_q) per valid column and takes the carried
exp(M_prev - M_kk) P + eps rowsum(F_q) vs  (p and cnt likewise).  The two agree to rounding in float64 (tests/test_prefix_long_cpu.py)."""
import functools
import math

import torch

from tests import favor_cached_ref as R
from tests import favor_summary_ref as S

EPS = 1e-4
CHUNK = 32
T, H = 2, 8
SHAPES = S.SHAPES                                   # (d, m): (16, 16), (64, 266), (256, 1419)
NCS = [1, 31, 32, 33, 64, 65, 97]
NQS = [1, 16, 17]
KINDS = ["live", "big", "peak_last", "equal"]
# per-task context sizes for the masking tests: a task that ends below a chunk edge, at one, one shot behind one, and at a single shot
LENS = {33: [(33, 31), (32, 33), (1, 33)], 65: [(65, 31), (33, 64), (63, 65)], 97: [(97, 30), (64, 97), (1, 65)]}


def _key_terms(k, proj):
    k, proj = k.double(), proj.double()
    c = k.shape[-1] ** -0.25
    dd = torch.einsum("thnd,md->thnm", c * k, proj)
    return dd, (k * k).sum(dim=-1, keepdim=True) * 0.5 * (c * c)


def _valid(lens, Tn, Nc):
    lens = [Nc] * Tn if lens is None else list(lens)
    return torch.arange(Nc)[None, :] < torch.tensor(lens)[:, None]              # [T, Nc]


def shot_maxima(k, proj, lens=None):
    """smax[n]: the maximum of dd over the tasks that hold shot n, all heads and features (-inf where no task holds it)."""
    dd, _ = _key_terms(k, proj)
    valid = _valid(lens, k.shape[0], k.shape[2])
    return torch.where(valid[:, None, :, None], dd, torch.full((), -math.inf, dtype=torch.float64)).amax(dim=(0, 1, 3))


def direct(q, k, v, proj, ks, lens=None):
    """-> (out [K, T, H, Nq, d], den [K, T, H, Nq]): per prefix the reference's attention, the projections taken once."""
    Tn, Nc = k.shape[0], k.shape[2]
    fq = R.query_features(q, proj, EPS)
    dd, diag = _key_terms(k, proj)
    valid = _valid(lens, Tn, Nc)
    run = torch.cummax(shot_maxima(k, proj, lens), dim=0).values
    ratio = proj.shape[0] ** -0.5
    outs, dens = [], []
    for kk in ks:
        fk = ratio * (torch.exp(dd[:, :, :kk] - diag[:, :, :kk] - run[kk - 1]) + EPS)
        fk = torch.where(valid[:, None, :kk, None], fk, torch.zeros((), dtype=torch.float64))
        Sm = torch.einsum("thqm,thnm->thqn", fq, fk)
        vv = torch.where(valid[:, None, :kk, None], v[:, :, :kk].double(), torch.zeros((), dtype=torch.float64))
        den = Sm.sum(dim=-1)
        outs.append(torch.einsum("thqn,thne->thqe", Sm, vv) / den[..., None])
        dens.append(den)
    return torch.stack(outs), torch.stack(dens)


def streamed(q, k, v, proj, ks, lens=None, chunk=CHUNK):
    """-> (out [K, T, H, Nq, d], den [K, T, H, Nq]) by the chunked walk; the denominators are in units of the key feature's ratio."""
    Tn, Hn, Nc, d = k.shape
    fq = R.query_features(q, proj, EPS)
    fs = fq.sum(dim=-1)                                                         # [T, H, Nq]
    dd, diag = _key_terms(k, proj)
    valid = _valid(lens, Tn, Nc)
    smax = shot_maxima(k, proj, lens)
    zero = torch.zeros((), dtype=torch.float64)
    vv = torch.where(valid[:, None, :, None], v.double(), zero)
    P = torch.zeros(Tn, Hn, q.shape[2], d, dtype=torch.float64)
    p = torch.zeros(Tn, Hn, q.shape[2], dtype=torch.float64)
    vs = torch.zeros(Tn, Hn, d, dtype=torch.float64)
    cnt = torch.zeros(Tn, dtype=torch.float64)
    Mprev, outs, dens, ks = -math.inf, [], [], list(ks)

    def scale(a, b):                                                            # exp(a - b) with a <= b; 1 where equal (-inf included)
        return 1.0 if a == b else math.exp(a - b)
    for c0 in range(0, ks[-1], chunk):
        c1 = min(c0 + chunk, Nc)
        mref = torch.cummax(torch.cat([torch.tensor([Mprev], dtype=torch.float64), smax[c0:c1]]), dim=0).values[1:]
        ok = valid[:, None, c0:c1, None]
        E = torch.where(ok, torch.exp(torch.where(ok, dd[:, :, c0:c1] - diag[:, :, c0:c1] - mref[None, None, :, None], zero)), zero)
        Sc = torch.einsum("thqm,thnm->thqn", fq, E)                             # relative to Mref[n], column by column
        okc = valid[:, None, None, c0:c1]

        def part(pn, Mk, eps):
            w = torch.tensor([scale(mref[i].item(), Mk) for i in range(pn)], dtype=torch.float64)
            Sf = torch.where(okc[..., :pn], Sc[..., :pn] * w + eps * fs[..., None], zero)
            return torch.einsum("thqn,thne->thqe", Sf, vv[:, :, c0:c0 + pn]), Sf.sum(dim=-1)
        for kk in [x for x in ks if c0 < x <= c0 + chunk]:
            Mk = mref[kk - c0 - 1].item()
            g = scale(Mprev, Mk)
            num, den = part(kk - c0, Mk, EPS)
            num = g * P + EPS * fs[..., None] * vs[:, :, None, :] + num
            den = g * p + EPS * cnt[:, None, None] * fs + den
            outs.append(num / den[..., None])
            dens.append(den)
        Mend = mref[-1].item()
        g = scale(Mprev, Mend)
        num, den = part(c1 - c0, Mend, 0.0)
        P, p = g * P + num, g * p + den
        vs = vs + vv[:, :, c0:c1].sum(dim=2)
        cnt = cnt + valid[:, c0:c1].sum(dim=1).double()
        Mprev = Mend
    return torch.stack(outs), torch.stack(dens)


def merged(out):
    """[K, T, H, N, d] -> the kernels' [K, T, N, d*H]: out[k, t, n, e*H + h]."""
    K, Tn, Hn, N, d = out.shape
    return out.permute(0, 1, 3, 4, 2).reshape(K, Tn, N, d * Hn)


# ---- the inputs the CPU and GPU tests share ---------------------------------------------------------------------------------------
def ks_sets(Nc):
    """name -> strictly increasing context sizes: all of them, the last, the chunk-edge quartet, and every size next to a chunk edge."""
    edges = sorted({x for e in range(CHUNK, Nc + CHUNK, CHUNK) for x in (e - 1, e, e + 1) if 1 <= x <= Nc} | {1, Nc})
    return {"all": list(range(1, Nc + 1)), "last": [Nc], "1_32_33_Nc": sorted({x for x in (1, 32, 33, Nc) if x <= Nc}), "edges": edges}


def peak_shot(Nc):
    """The dominating key of "peak_last": the second shot of the last chunk (the first where the chunk holds one shot) - every
    earlier prefix has a lower stabiliser, the carried sums are rescaled by exp(-50) and so is the column before it in its chunk."""
    n0 = (Nc - 1) // CHUNK * CHUNK
    return min(n0 + 1, Nc - 1)


@functools.lru_cache(maxsize=None)
def case(kind, d, m, Nc, Nq=max(NQS)):
    """-> dict: q [T, H, Nq, d], k / v [T, H, Nc, d], proj [m, d]; fp32, CPU.  The first rows of q serve a smaller Nq (row-wise op)."""
    proj = S.proj_for(d, m)
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nc + len(kind))
    q = 0.25 * torch.randn(T, H, Nq, d, generator=g)
    k = 0.25 * torch.randn(T, H, Nc, d, generator=g)
    v = torch.randn(T, H, Nc, d, generator=g)
    if kind == "big":
        q, k = 4 * q, 4 * k
    elif kind == "peak_last":
        k = 0.05 * torch.randn(T, H, Nc, d, generator=g)
        pr = proj[m // 2]
        k[T - 1, H - 1, peak_shot(Nc)] = pr * (50.0 / (d ** -0.25 * float(pr @ pr)))
    elif kind == "equal":
        k = k[:1, :1, :1].expand(T, H, Nc, d).contiguous()
    else:
        assert kind == "live"
    return dict(q=q, k=k, v=v, proj=proj)


@functools.lru_cache(maxsize=2)
def reference(kind, d, m, Nc, lens=None):
    """(out [Nc, T, H, Nq, d], den) of `streamed` for ALL sizes 1..Nc - computed once, indexed by the tests (row kk - 1 = size kk)."""
    c = case(kind, d, m, Nc)
    return streamed(c["q"], c["k"], c["v"], c["proj"], range(1, Nc + 1), lens)


def want(kind, d, m, Nc, ks, Nq, lens=None):
    """The kernels' [K, T, Nq, d*H] in float64 for the sizes `ks` and the first Nq target rows."""
    out = reference(kind, d, m, Nc, lens)[0]
    return merged(out[[kk - 1 for kk in ks]][:, :, :, :Nq])
