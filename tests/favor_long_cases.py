"""The inputs of the long per-shot state's tests (tests/test_favor_long_cpu.py, tests/test_favor_long_gpu.py), one
recipe for both: tests/attention_readout_cases.py's value kinds and shapes at the slot counts either side of every 32-slot chunk
edge up to the capacity of 256.  The float64 references are computed once per case and shared."""
import functools

import torch

from tests import attention_readout_cases as AC
from tests import attention_readout_ref as AR
from tests import ragged_ref as RR

T, H = AC.T, AC.H
DM = [(16, 16), (64, 266)]
DM_BIG = (256, 1419)           # one case at the shipped ResNet shape: the largest F_q tile beside the wide S tile
NC_BIG, NQ_BIG = 65, 17
NCS = [33, 48, 64, 65, 255, 256]
NQS = [1, 16, 17, 40]
NQ = 40                        # query rows per case: the first 40 of AC.inputs' 100
KINDS = AC.KINDS
TIE_NCS = [1, 15, 32]          # sent through the long entries: one chunk, the shipped kernels' bits
RAGGED_NCS = [48, 65, 256]


def inputs(kind, d, m, Nc):
    """(q [T, H, NQ, d], k, v [T, H, Nc, d], proj [m, d])"""
    q, k, v, p = AC.inputs(kind, d, m, Nc)
    return q[:, :, :NQ].contiguous(), k, v, p


def cases():
    """every (kind, d, m, Nc) the GPU value test runs"""
    return [(kind, d, m, Nc) for d, m in DM for Nc in NCS for kind in KINDS] + [(kind, *DM_BIG, NC_BIG) for kind in KINDS]


@functools.lru_cache(maxsize=None)
def want(kind, d, m, Nc):
    """(w64 [T, H, NQ, Nc], out64 [T, H, NQ, d])"""
    w, out = AC.want(kind, d, m, Nc)
    return w[:, :, :NQ], out[:, :, :NQ]


def ragged_lens(Nc):
    """1, 32, 33 and full, two tasks at a time: a task of one shot beside a full one, and the two sides of the first chunk edge"""
    return [(1, Nc), (32, 33), (Nc, 33)]


@functools.lru_cache(maxsize=None)
def ragged(kind, d, m, Nc, lens):
    """(q, k with NaN behind lens[t], v with +-1e30 there, proj, w64 [T, H, NQ, Nc], out64, F_k64 [T, H, Nc, m], M64)"""
    q, k, v, p = inputs(kind, d, m, Nc)
    valid = RR.valid_mask(lens, Nc)[:, None, :, None]
    kn = torch.where(valid, k, torch.full((), float("nan")))
    sign = torch.where(torch.arange(Nc) % 2 == 0, 1.0, -1.0)[None, None, :, None]
    vp = torch.where(valid, v, 1e30 * sign.expand_as(v))
    fk, M = RR.key_features(k, p, lens)
    return q, kn, vp, p, AR.weights(q, k, p, lens), RR.attention(q, k, v, p, lens), fk, M


@functools.lru_cache(maxsize=None)
def peak_first(d, m, Nc=40):
    """(q, k, v, proj) of Nc shots whose batch maximum sits in the first 32: kind peak at 32 shots (the peak is slot 31 of task 1,
    head 0) and Nc - 32 further quiet keys.  The cached state of the first 32 shots then has the stabiliser of all Nc."""
    q, k32, v32, p = inputs("peak", d, m, 32)
    g = torch.Generator().manual_seed(5 + d + m)
    k = torch.cat([k32, 0.05 * torch.randn(T, H, Nc - 32, d, generator=g)], dim=2)
    v = torch.cat([v32, torch.randn(T, H, Nc - 32, d, generator=g)], dim=2)
    dd = d ** -0.25 * torch.einsum("thnd,md->thnm", k.double(), p.double())
    assert float(dd[:, :, :32].max()) > float(dd[:, :, 32:].max()) + 1.0
    return q, k, v, p
