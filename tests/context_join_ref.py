"""The case tables and the index reference of the join tests, shared by the CPU and the GPU files: a plain-Python
restatement of mlhot.ragged.gather_rows, mlhot_rows_gather's contract by torch indexing, and the plans of the kernel grid."""
import torch

from tests import favor_summary_ref as S

H = S.H

# ---- mlhot_rows_gather ---------------------------------------------------------------------------------------------------------------
SRC_SHAPES = ((1, 1), (2, 33), (3, 257), (1, 5), (2, 2), (4, 7), (1, 64), (2, 9))      # (T_j, cap_j) of source j: the first nsrc are used
WIDTHS = ((4,), (8,), (2048,), (4, 2048), (8, 8))                                       # the row sets of one call
NSRCS = (1, 2, 3, 5, 8)                                                                 # 3 and 5: the descriptors behind nsrc match nothing
CAPS = (1, 5, 33, 257)
TS = (1, 3)
SPECIALS = 6                                                                            # entries special_entries() returns


def special_entries(nsrc, rows):
    """The plan entries every kernel case holds: the fill, a source index of nsrc, a row of rows[ps], a row of -5, and one source
    row named twice."""
    last = nsrc - 1
    return [(-1, -1), (nsrc, 0), (last, rows[last]), (0, -5), (last, rows[last] - 1), (last, rows[last] - 1)]


def kernel_plans(T, cap, nsrc, seed):
    """Plans [T][cap][2] (host ints) over the first nsrc of SRC_SHAPES: the special entries in front, valid random entries behind them.
    Where T * cap < SPECIALS the specials are spread over as many plans as it takes."""
    rows = [t * c for t, c in SRC_SHAPES[:nsrc]]
    g = torch.Generator().manual_seed(seed)
    special, n, plans = special_entries(nsrc, rows), T * cap, []
    for v in range(0, SPECIALS, min(n, SPECIALS)):
        flat = special[v:v + n]
        ps = torch.randint(0, nsrc, (n - len(flat),), generator=g).tolist()
        flat += [(p, int(torch.randint(0, rows[p], (1,), generator=g))) for p in ps]
        plans.append([flat[t * cap:(t + 1) * cap] for t in range(T)])
    return plans


def named(plan, nsrc):
    """Per source the set of flat rows that a valid plan entry names."""
    rows = [t * c for t, c in SRC_SHAPES[:nsrc]]
    out = [set() for _ in range(nsrc)]
    for task in plan:
        for ps, pr in task:
            if 0 <= ps < nsrc and 0 <= pr < rows[ps]:
                out[ps].add(pr)
    return out


def gathered(srcs, plan):
    """mlhot_rows_gather's contract by torch indexing: srcs[j] [T_j, cap_j, ...] (one row set), plan an int [T, cap, 2] tensor on their
    device -> [T, cap, ...]: the named row, exact zeros where the source or the row is out of range."""
    flat = [x.reshape(x.shape[0] * x.shape[1], -1) for x in srcs]
    rows = torch.tensor([f.shape[0] for f in flat], device=plan.device)
    start = torch.cumsum(rows, 0) - rows
    ps, pr = plan[..., 0].long(), plan[..., 1].long()
    ok = (ps >= 0) & (ps < len(srcs))
    psc = ps.clamp(0, len(srcs) - 1)
    ok &= (pr >= 0) & (pr < rows[psc])
    idx = torch.where(ok, start[psc] + pr, torch.zeros_like(pr))
    out = torch.cat(flat).index_select(0, idx.reshape(-1))
    out = torch.where(ok.reshape(-1, 1), out, torch.zeros((), device=plan.device))
    return out.view(*plan.shape[:2], *srcs[0].shape[2:])


# ---- the host plan -------------------------------------------------------------------------------------------------------------------
def gather_rows(parts, lens, caps, capacity):
    """mlhot.ragged.gather_rows restated slot by slot: -> (table [T][capacity][2], the new lens)."""
    table, total = [], []
    for task in parts:
        slots = []
        for state, t in task:
            for s in range(lens[state][t]):
                slots.append((state, t * caps[state] + s))
        total.append(len(slots))
        while len(slots) < capacity:
            slots.append((-1, -1))
        table.append(slots)
    return table, tuple(total)


# states of 3 tasks: (lens, capacity)
PLAN_STATES = (((4, 2, 1), 4), ((1, 5, 3), 8), ((2, 2, 2), 2), ((33, 1, 7), 40), ((1, 1, 1), 1), ((3, 0, 2), 3), ((6, 6, 1), 6), ((2, 9, 4), 12))
PLAN_CASES = {
    "one_part": [[(0, 0)], [(1, 1)], [(3, 2)]],
    "two_parts": [[(0, 0), (1, 0)], [(1, 1), (0, 1)], [(2, 2), (3, 0)]],
    "eight_parts": [[(i, 0) for i in range(8)], [(i, (i + 1) % 3) for i in range(8)], [(7 - i, 2) for i in range(8)]],
    "the_same_pair_in_two_tasks": [[(3, 0)], [(3, 0), (0, 0)], [(0, 0), (3, 0)]],
    "a_part_without_a_shot": [[(5, 1), (0, 0)], [(0, 1), (5, 1)], [(5, 0)]],
}

# ---- concat's finishing step ---------------------------------------------------------------------------------------------------------
KEY_SHAPES = ((16, 16), (64, 266))                       # (d, m)
KEY_JOINS = (("keys", 5, 7), ("long", 20, 20), ("paged", 200, 60))
KEY_T = 2
