"""Float64 restatement of picking and combining TASKS across FAVOR+ summary states (csrc/favor_summary.h) over
tests/favor_summary_ref.py's State, and the libraries of separately built states that the CPU and GPU tests share.  Output task t is
the sum of its parts (state i, task u):  A'[t] = sum_p exp(M_i - M') A_i[u], a' likewise, vs' and cnt' plain sums, with M' the maximum
over EVERY state passed (and the floor) - merge (tests/favor_merge_ref.py) with a row per task."""
import functools
import math

import torch

from tests import favor_summary_ref as S

KINDS = S.KINDS        # the input kinds of the merge tests, placed over a library of states (library())


def gather(states, parts, floor=-math.inf):
    """The kernel's contract: -> a new favor_summary_ref.State of len(parts) tasks; every state enters M', named or not."""
    _, H, m, d = states[0].A.shape
    out = S.State(len(parts), H, d, m)
    out.M = max([st.M for st in states] + [floor])
    for t, row in enumerate(parts):
        for i, u in row:
            st = states[i]
            s = 1.0 if st.M == out.M else math.exp(st.M - out.M) if st.M > -math.inf else 0.0
            out.A[t] += s * st.A[u]
            out.a[t] += s * st.a[u]
            out.vs[t] += st.vs[u]
            out.cnt[t] += st.cnt[u]
    return out


def named(parts):
    return sorted({i for row in parts for i, _ in row})


def op(states, parts, floor=-math.inf):
    """mlhot.ops.favor_gather's meaning: the states that no part names are dropped first, so they do not enter M'."""
    keep = named(parts)
    slot = {i: k for k, i in enumerate(keep)}
    if not keep:
        _, H, m, d = states[0].A.shape
        out = S.State(len(parts), H, d, m)
        out.M = floor
        return out
    return gather([states[i] for i in keep], [[(slot[i], u) for i, u in row] for row in parts], floor)


class Source:
    """One separately conditioned batch: k, v [T, H, n, d] fp32, task t's shots are its first lens[t] rows."""

    def __init__(self, k, v, lens, proj):
        self.k, self.v, self.lens, self.proj = k, v, list(lens), proj
        self.T = k.shape[0]

    @functools.cached_property
    def state(self):
        T, H, _, d = self.k.shape
        return S.State(T, H, d, self.proj.shape[0]).absorb(self.k, self.v, self.proj, self.lens)


def direct(sources, parts, M):
    """The float64 stream over each output task's shots under the FORCED stabiliser M: what condition(form="summary") builds from the
    chosen shots in a batch whose stabiliser is M."""
    _, H, _, d = sources[0].k.shape
    proj = sources[0].proj.double()
    out = S.State(len(parts), H, d, proj.shape[0])
    out.M = M
    c = d ** -0.25
    for t, row in enumerate(parts):
        for i, u in row:
            src = sources[i]
            kt, vt = src.k[u, :, :src.lens[u]].double(), src.v[u, :, :src.lens[u]].double()
            dd = torch.einsum("hnd,md->hnm", c * kt, proj)
            e = torch.exp(dd - (kt * kt).sum(dim=-1, keepdim=True) * 0.5 * (c * c) - M)
            out.A[t] += torch.einsum("hnm,hne->hme", e, vt)
            out.a[t] += e.sum(dim=1)
            out.vs[t] += vt.sum(dim=1)
            out.cnt[t] += src.lens[u]
    return out


@functools.lru_cache(maxsize=None)
def library(kind, tasks, H, d, m, shots=5, seed=0):
    """len(tasks) sources, source i with tasks[i] tasks of `shots` shots each (a task count of 0 stands for a FRESH source: one task,
    no shot, M = -inf).  The kinds are the merge tests' (favor_summary_ref.case), placed over the library: "big" 4 x the keys; "peak" /
    "peak_last" a key with dd = 50 in the last source's last task (every other state is rescaled by about exp(-50)),
    "peak_first_t0" in source 0's task 0; "equal" one key everywhere.  Every source's keys carry their own scale, so the stabilisers
    differ from state to state by small and by large amounts."""
    proj = S.proj_for(d, m)
    g = torch.Generator().manual_seed(7919 * d + m + 31 * len(tasks) + 1000 * seed + len(kind))
    out = []
    live = [i for i, T in enumerate(tasks) if T > 0]
    for i, T in enumerate(tasks):
        T1 = max(T, 1)
        scale = (0.05 if kind.startswith("peak") else 0.25) * (1.0 + 0.6 * (i % 3)) * (4.0 if kind == "big" else 1.0)
        k = scale * torch.randn(T1, H, shots, d, generator=g)
        v = torch.randn(T1, H, shots, d, generator=g)
        if kind == "equal":
            k = k[:1, :1, :1].expand(T1, H, shots, d).contiguous()
        p = proj[m // 2]
        if kind in ("peak", "peak_last") and i == live[-1]:
            k[T1 - 1, H - 1, shots - 1] = p * (50.0 / (d ** -0.25 * float(p @ p)))
        if kind == "peak_first_t0" and i == live[0]:
            k[0, 0, 0] = p * (50.0 / (d ** -0.25 * float(p @ p)))
        out.append(Source(k, v, [shots if T > 0 else 0] * T1, proj))
    return tuple(out)


def queries(T, H, d, Nq=7, seed=5):
    return 0.25 * torch.randn(T, H, Nq, d, generator=torch.Generator().manual_seed(seed + d))
