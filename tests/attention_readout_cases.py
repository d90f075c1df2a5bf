"""The inputs of the attention read-out tests (tests/test_attention_readout_cpu.py, tests/test_attention_readout_gpu.py), one recipe
for both: tests/test_condition_gpu.py's shapes and value kinds - the smallest at which the tile logic can go wrong - with Nc 16 and
17 added either side of the 16-slot S tile.  Layout [T, H, N, d] on the CPU, like oracle.ref_cpu; the float64 references are
computed once per case and shared."""
import functools
import os

import numpy as np
import torch

from oracle import ref_cpu as O
from tests import attention_readout_ref as AR
from tests import favor_cached_ref as R
from tests import ragged_ref as RR
from tests import util as U

T, H = 2, 2
DM = [(16, 16), (64, 266), (256, 1419), (256, 1536)]
NCS = [1, 15, 16, 17, 32]
NQS = [1, 17, 100]
NQ = 100                       # rows generated per case; a smaller Nq takes the first rows (w is row-wise in q)
KINDS = ["live", "big", "peak", "equal"]


@functools.lru_cache(maxsize=None)
def proj(d, m):
    if (d, m) == (64, 266):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor.npz"))["d64_big/proj"])
    if (d, m) == (256, 1419):
        return torch.from_numpy(np.load(os.path.join(U.GOLDEN, "favor_c5.npz"))["proj"])
    with torch.random.fork_rng():
        torch.manual_seed(77 + m)
        return O.gaussian_orthogonal_random_matrix(m, d).float()


@functools.lru_cache(maxsize=None)
def inputs(kind, d, m, Nc):
    """(q [T, H, NQ, d], k, v [T, H, Nc, d], proj [m, d])"""
    g = torch.Generator().manual_seed(1000 * d + m + 17 * Nc + len(kind))
    q = 0.25 * torch.randn(T, H, NQ, d, generator=g)
    k = 0.25 * torch.randn(T, H, Nc, d, generator=g)
    v = torch.randn(T, H, Nc, d, generator=g)
    if kind == "big":                    # favor.npz's large-norm case: its own tensors where the shape is its own, the live regime x 4 elsewhere
        q, k = 4 * q, 4 * k
        if (d, m) == (64, 266):
            fx = np.load(os.path.join(U.GOLDEN, "favor.npz"))
            fq, fk, fv = (torch.from_numpy(fx[f"d64_big/{n}"]) for n in ("q", "k", "v"))       # [2, 8, 15, 64]: heads 0..H-1, shots cycled
            q = fq[:, :H][:, :, torch.arange(NQ) % fq.shape[2]].contiguous()
            k, v = fk[:, :H, torch.arange(Nc) % 15].contiguous(), fv[:, :H, torch.arange(Nc) % 15].contiguous()
    elif kind == "peak":                 # one key whose dd maximum sits ~50 above the rest: most key features are the 1e-4 floor
        k = 0.05 * torch.randn(T, H, Nc, d, generator=g)
        p = proj(d, m)[m // 2]
        k[1, 0, Nc - 1] = p * (50.0 / (d ** -0.25 * float(p @ p)))
    elif kind == "equal":                # all keys equal
        k = k[:1, :1, :1].expand(T, H, Nc, d).contiguous()
    else:
        assert kind == "live"
    return q, k, v, proj(d, m)


@functools.lru_cache(maxsize=None)
def want(kind, d, m, Nc):
    """(w64 [T, H, NQ, Nc], out64 [T, H, NQ, d]) of inputs(kind, d, m, Nc)"""
    q, k, v, p = inputs(kind, d, m, Nc)
    return AR.weights(q, k, p), R.attention(q, k, v, p)


def masked_lens(Nc):
    """The two length patterns of the masked cases: one task at a single shot resp. half of its slots, the other full.  Nc == 1 has
    one pattern only - a task holds at least one context shot."""
    return [(1, Nc)] if Nc == 1 else [(1, Nc), (Nc // 2, Nc)]


@functools.lru_cache(maxsize=None)
def masked(kind, d, m, Nc, lens):
    """(q, k with NaN in the rows behind lens[t], v with zeros there, proj, w64, out64): the state favor_keys(..., lens=) serves"""
    q, k, v, p = inputs(kind, d, m, Nc)
    valid = RR.valid_mask(lens, Nc)[:, None, :, None]
    kn = torch.where(valid, k, torch.full((), float("nan")))
    vz = torch.where(valid, v, torch.zeros(()))
    return q, kn, vz, p, AR.weights(q, k, p, lens), RR.attention(q, k, v, p, lens)


def rowsum_bound(Nc):
    """|sum_n w - 1| for fp32 quotients S / D summed exactly: one rounding per quotient plus the Nc - 1 of D's own sum"""
    return Nc * 2.0 ** -23
