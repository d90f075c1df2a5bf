"""Float64 restatement of the streaming FAVOR+ summary state (csrc/favor_summary.h) and the inputs the summary tests
share.  Per (task, head) the state holds, relative to ONE stabiliser M (the maximum of dd over every valid shot of all tasks, heads and
features absorbed so far):  A[j, e] = sum_n exp(dd[n, j] - diag[n] - M) v[n, e],  a[j] = sum_n exp(dd[n, j] - diag[n] - M),
vs[e] = sum_n v[n, e]  and cnt.  Absorbing rescales by exp(M - M'); a fresh state has M = -inf.  The query is
out = F_q (A + eps vs) / F_q (a + eps cnt)  with tests/favor_cached_ref.py's query features - equal to favor_cached_ref.attention on
the concatenated valid shots in exact arithmetic (the key side's ratio cancels).  Layout [T, H, N, d] like oracle.ref_cpu."""
import functools
import math
import os

import numpy as np
import torch

from oracle import ref_cpu as O
from tests import favor_cached_ref as R
from tests import ragged_ref as RR
from tests import util as U

EPS = 1e-4


class State:
    def __init__(self, T, H, d, m):
        self.A = torch.zeros(T, H, m, d, dtype=torch.float64)
        self.a = torch.zeros(T, H, m, dtype=torch.float64)
        self.vs = torch.zeros(T, H, d, dtype=torch.float64)
        self.cnt = [0] * T
        self.M = -math.inf

    def absorb(self, k, v, proj, lens=None):
        """k, v [T, H, n, d]; task t's new shots are its first lens[t] rows (default n); the other rows are never read."""
        T, H, n, d = k.shape
        lens = [n] * T if lens is None else list(lens)
        c = d ** -0.25
        dds, new_max = [], -math.inf
        for t in range(T):
            kt = k[t, :, :lens[t]].double()
            dd = torch.einsum("hnd,md->hnm", c * kt, proj.double())
            dds.append((dd, (kt * kt).sum(dim=-1, keepdim=True) * 0.5 * (c * c)))
            if lens[t]:
                new_max = max(new_max, dd.max().item())
        M2 = max(self.M, new_max)
        if M2 == -math.inf:
            return self                           # nothing valid yet: exp(-inf - -inf) must not be formed
        scale = math.exp(self.M - M2) if self.M > -math.inf else 0.0
        self.A *= scale
        self.a *= scale
        for t in range(T):
            dd, diag = dds[t]
            e = torch.exp(dd - diag - M2)         # [H, n_t, m]
            vt = v[t, :, :lens[t]].double()
            self.A[t] += torch.einsum("hnm,hne->hme", e, vt)
            self.a[t] += e.sum(dim=1)
            self.vs[t] += vt.sum(dim=1)
            self.cnt[t] += lens[t]
        self.M = M2
        return self

    def query(self, q, proj):
        """q [T, H, Nq, d] -> out [T, H, Nq, d]; every task must have absorbed a shot."""
        assert min(self.cnt) >= 1
        fq = R.query_features(q, proj, EPS)
        cnt = torch.tensor(self.cnt, dtype=torch.float64)[:, None, None]
        num = torch.einsum("thqm,thme->thqe", fq, self.A) + EPS * fq.sum(dim=-1, keepdim=True) * self.vs[:, :, None, :]
        den = torch.einsum("thqm,thm->thq", fq, self.a) + EPS * cnt * fq.sum(dim=-1)
        return num / den[..., None]


# ---- the inputs the CPU and GPU tests share ---------------------------------------------------------------------------------------
H = 2
SHAPES = [(16, 16), (64, 266), (256, 1419)]
# name -> the absorb calls: (slots n, valid new shots per task or None = all n) - for two tasks; one task takes the first entry
CHUNKINGS = {
    "one": [(1, None)],
    "cap_plus_one": [(32, None), (1, None)],
    "7_32_31": [(7, None), (32, None), (31, None)],
    "ragged": [(5, (5, 0)), (32, (32, 32)), (9, (0, 9))],
}
# test_condition_gpu.py's four, and two more placements of the dominating key: in the LAST chunk (everything absorbed before is
# rescaled by exp(-50)), and in the FIRST chunk of task 0 only (the other task's shots never see their own maximum)
KINDS = ["live", "big", "peak", "equal", "peak_last", "peak_first_t0"]
NQ = 20


def tasks(d, m):
    return 1 if (d, m) == (256, 1419) else 2


@functools.lru_cache(maxsize=None)
def proj_for(d, m):
    if (d, m) == (64, 266):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor.npz"))["d64_big/proj"])
    if (d, m) == (256, 1419):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor_c5.npz"))["proj"])
    with torch.random.fork_rng():
        torch.manual_seed(77 + m)
        return O.gaussian_orthogonal_random_matrix(m, d).float()


def chunk_lens(chunking, T):
    """[(n, [valid new shots per task])] for T tasks."""
    return [(n, [n] * T if lens is None else list(lens[:T])) for n, lens in CHUNKINGS[chunking]]


@functools.lru_cache(maxsize=None)
def case(kind, d, m, chunking, Nq=NQ):
    """-> dict: q [T, H, Nq, d], proj, k / v [T, H, Nmax, d] (task t's valid shots are its first totals[t] rows, zeros behind),
    totals, chunks [(k_c, v_c [T, H, n, d] with zeros in the invalid slots, lens)], peak (task, head, row) or None.  All fp32, CPU."""
    T = tasks(d, m)
    calls = chunk_lens(chunking, T)
    totals = [sum(l[t] for _, l in calls) for t in range(T)]
    Nmax = max(totals)
    proj = proj_for(d, m)
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nmax + len(kind) + len(chunking))
    q = 0.25 * torch.randn(T, H, Nq, d, generator=g)
    k = 0.25 * torch.randn(T, H, Nmax, d, generator=g)
    v = torch.randn(T, H, Nmax, d, generator=g)
    peak = None
    if kind == "big":
        q, k = 4 * q, 4 * k
        if (d, m) == (64, 266):
            fx = np.load(os.path.join(U.GOLDEN, "favor.npz"))
            fq, fk, fv = (torch.from_numpy(fx[f"d64_big/{n}"]) for n in ("q", "k", "v"))
            q = fq[:T, :H][:, :, torch.arange(Nq) % fq.shape[2]].contiguous()
            k, v = fk[:T, :H, torch.arange(Nmax) % 15].contiguous(), fv[:T, :H, torch.arange(Nmax) % 15].contiguous()
    elif kind.startswith("peak"):
        k = 0.05 * torch.randn(T, H, Nmax, d, generator=g)
        if kind == "peak":                       # test_condition_gpu.py's placement: the last shot of the last task
            peak = (T - 1, 0, totals[T - 1] - 1)
        elif kind == "peak_last":                # the first new shot of the last call that brings one, in the last task it gives one
            last = max(i for i, (_, l) in enumerate(calls) if any(l))
            t = max(t for t in range(T) if calls[last][1][t] > 0)
            peak = (t, H - 1, sum(l[t] for _, l in calls[:last]))
        else:                                    # the first shot of task 0
            peak = (0, 0, 0)
        p = proj[m // 2]
        k[peak] = p * (50.0 / (d ** -0.25 * float(p @ p)))
    elif kind == "equal":
        k = k[:1, :1, :1].expand(T, H, Nmax, d).contiguous()
    else:
        assert kind == "live"
    valid = RR.valid_mask(totals, Nmax)[:, None, :, None]
    k, v = torch.where(valid, k, torch.zeros(())), torch.where(valid, v, torch.zeros(()))
    chunks, at = [], [0] * T
    for n, lens in calls:
        kc, vc = torch.zeros(T, H, n, d), torch.zeros(T, H, n, d)
        for t in range(T):
            kc[t, :, :lens[t]] = k[t, :, at[t]:at[t] + lens[t]]
            vc[t, :, :lens[t]] = v[t, :, at[t]:at[t] + lens[t]]
            at[t] += lens[t]
        chunks.append((kc, vc, lens))
    return dict(T=T, q=q, proj=proj, k=k, v=v, totals=totals, chunks=chunks, peak=peak)


def reference(c):
    """favor_cached_ref.attention on the concatenated valid shots (tests/ragged_ref.py's form of it where the totals differ)."""
    if len(set(c["totals"])) == 1:
        return R.attention(c["q"], c["k"], c["v"], c["proj"])
    return RR.attention(c["q"], c["k"], c["v"], c["proj"], c["totals"])


def streamed(c):
    """The float64 summary state after the case's absorb calls."""
    T, _, _, d = c["q"].shape
    st = State(T, H, d, c["proj"].shape[0])
    for kc, vc, lens in c["chunks"]:
        st.absorb(kc, vc, c["proj"], lens)
    return st
