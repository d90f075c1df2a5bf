"""Float64 restatement of what the sliding-window cached contexts compute: the row compaction of an eviction and
the retracting stream of a summary state, on tests/favor_summary_ref.py's State and tests/ragged_ref.py's key features."""
import math

import torch

from tests import favor_summary_ref as S


def compact(src, plan):
    """src [T, cap, ...], plan [T][cap] host ints -> dst: row s of task t is row plan[t][s] of src, zeros where plan[t][s] is outside
    0 .. cap - 1 (selected by index: nothing of a row that is not named is read)."""
    T, cap = src.shape[:2]
    dst = torch.zeros_like(src)
    for t in range(T):
        for s, p in enumerate(plan[t]):
            if 0 <= p < cap:
                dst[t, s] = src[t, p]
    return dst


class Stream(S.State):
    """S.State with the retracting step and a forced stabiliser."""

    def __init__(self, T, H, d, m, M=-math.inf):
        super().__init__(T, H, d, m)
        self.M = M                                # absorb keeps max(M, the new maximum): a forced M above every dd stays

    def retract(self, k, v, proj, lens=None):
        """k, v [T, H, n, d]: task t gives up its first lens[t] rows (default n).  M stays; e = exp(min(dd - M, 0) - diag)."""
        T, H, n, d = k.shape
        lens = [n] * T if lens is None else list(lens)
        c = d ** -0.25
        for t in range(T):
            kt, vt = k[t, :, :lens[t]].double(), v[t, :, :lens[t]].double()
            dd = torch.einsum("hnd,md->hnm", c * kt, proj.double())
            diag = (kt * kt).sum(dim=-1, keepdim=True) * 0.5 * (c * c)
            e = torch.exp(torch.clamp(dd - self.M, max=0.0) - diag)
            self.A[t] -= torch.einsum("hnm,hne->hme", e, vt)
            self.a[t] = torch.clamp(self.a[t] - e.sum(dim=1), min=0.0)
            self.vs[t] -= vt.sum(dim=1)
            self.cnt[t] -= lens[t]
        return self


def absorbed(k, v, proj, lens, M=-math.inf):
    """The float64 state of task t's first lens[t] rows of k, v [T, H, N, d], absorbed 32 at a time, at the stabiliser max(M, theirs)."""
    T, H, N, d = k.shape
    st = Stream(T, H, d, proj.shape[0], M)
    for s in range(0, N, 32):
        st.absorb(k[:, :, s:s + 32], v[:, :, s:s + 32], proj, [min(max(L - s, 0), min(32, N - s)) for L in lens])
    return st


def kappa(before, after, m):
    """max over (t, h, j < m) of a_before[j] / a_after[j]: how much the retraction amplifies a relative error of the state."""
    return (before.a[:, :, :m] / after.a[:, :, :m]).max().item()
