"""Float64 restatement of merging FAVOR+ summary states (csrc/favor_summary.h) over tests/favor_summary_ref.py's State,
and the splits of a case's absorb calls into separately built parts that the CPU and GPU tests share.  With M' = max_i M_i:
A' = sum_i exp(M_i - M') A_i, a' likewise, vs' = sum_i vs_i, cnt' = sum_i cnt_i; a state that has absorbed nothing (M = -inf) adds
nothing, and exp(-inf - -inf) is never formed."""
import math

from tests import favor_summary_ref as S

SPLITS = ["all", "first_rest", "per_call"]


def merge(states, floor=-math.inf):
    """-> a new favor_summary_ref.State; `floor`: the stabiliser is at least this."""
    T, H, m, d = states[0].A.shape
    out = S.State(T, H, d, m)
    out.M = max([st.M for st in states] + [floor])
    for st in states:
        s = 1.0 if st.M == out.M else math.exp(st.M - out.M) if st.M > -math.inf else 0.0
        out.A += s * st.A
        out.a += s * st.a
        out.vs += st.vs
        out.cnt = [x + y for x, y in zip(out.cnt, st.cnt)]
    return out


def groups(c, split):
    """The case's absorb calls as lists of calls, one list per separately built part."""
    chunks = c["chunks"]
    if split == "all":
        return [chunks]
    if split == "first_rest":
        return [chunks[:1], chunks[1:]]
    assert split == "per_call"
    return [[ch] for ch in chunks]


def part(c, calls):
    """The float64 state of some of the case's absorb calls alone."""
    T, _, _, d = c["q"].shape
    st = S.State(T, S.H, d, c["proj"].shape[0])
    for kc, vc, lens in calls:
        st.absorb(kc, vc, c["proj"], lens)
    return st


def part_lens(calls, T):
    return [sum(lens[t] for _, _, lens in calls) for t in range(T)]
