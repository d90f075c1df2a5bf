"""The case table of the attention-mass tests (tests/test_attention_mass_cpu.py, tests/test_attention_mass_gpu.py):
the smallest shapes at which the three mass kernels can go wrong.  T = 2, H = 2, d = 16; m 16 and 40 (one and three 16-feature
chunks, 40 no multiple of 16); Nq either side of the 16-row tile and three tiles with a ragged last one; Nc at the edges of every
form - the keys entry's 32 slots, the long entry's 32-slot chunks and 256 slots, the paged entry's 256-slot pages (257: a second
page of one slot, 512: two full pages, 513: three).  Layout [T, H, N, d] on the CPU, like oracle.ref_cpu; inputs are generated once
per case and shared."""
import functools

import torch

from oracle import ref_cpu as O

T, H, D = 2, 2, 16
MS = [16, 40]
NQS = [1, 15, 16, 17, 33]
NQ = max(NQS)                  # rows generated per case; a smaller Nq takes the first rows (w is row-wise in q)
NCS = {"cached": [1, 31, 32], "long": [33, 64, 255, 256], "paged": [257, 512, 513]}
EDGE = {"cached": 16, "long": 32, "paged": 256}        # the S tile's 16-slot half, the 32-slot chunk, the 256-slot page


def lens_patterns(form, Nc):
    """full (None), one task at a single shot, and (Nc - 1, an edge + 1) - held to 1 .. Nc, duplicates dropped"""
    pats = [None]
    for p in ((1, Nc), (max(Nc - 1, 1), min(EDGE[form] + 1, Nc))):
        if p != (Nc, Nc) and p not in pats:
            pats.append(p)
    return pats


CASES = [(form, Nc, m, lens) for form in ("cached", "long", "paged") for Nc in NCS[form] for m in MS for lens in lens_patterns(form, Nc)]


def case_id(case):
    form, Nc, m, lens = case
    return f"{form}-Nc{Nc}-m{m}-" + ("full" if lens is None else "x".join(str(n) for n in lens))


@functools.lru_cache(maxsize=None)
def proj(m):
    with torch.random.fork_rng():
        torch.manual_seed(177 + m)
        return O.gaussian_orthogonal_random_matrix(m, D).float()


@functools.lru_cache(maxsize=None)
def inputs(Nc, m):
    """(q [T, H, NQ, d], k, v [T, H, Nc, d], proj [m, d], tw [T, NQ] >= 0 with exact zeros among them)"""
    g = torch.Generator().manual_seed(31 * Nc + m)
    q = 0.5 * torch.randn(T, H, NQ, D, generator=g)
    k = 0.5 * torch.randn(T, H, Nc, D, generator=g)
    v = torch.randn(T, H, Nc, D, generator=g)
    tw = 2.0 * torch.rand(T, NQ, generator=g)
    tw[0, 3] = 0.0
    tw[1, 16] = 0.0
    return q, k, v, proj(m), tw


def valid(lens, Nc):
    """[T, Nc] bool: slot c of task t holds a shot"""
    if lens is None:
        return torch.ones(T, Nc, dtype=torch.bool)
    return torch.arange(Nc)[None, :] < torch.tensor(lens)[:, None]


def poisoned(x, lens, fill):
    """x [T, H, Nc, d] with `fill` in the rows behind lens[t]"""
    return torch.where(valid(lens, x.shape[2])[:, None, :, None], x, torch.full((), fill))
