"""Shared by tests/test_favor_linear_cpu.py and tests/test_favor_linear_gpu.py: the case table of FAVOR+'s linear-form route
(csrc/favor_linear.h, option "favor_linear": above 32 shots on either side) and the judge every case is held to.

Inputs, reference and bound are tests/favor_cases.py's: q and k are randn * d ** -0.25, v and wout randn, the projection is
favor_cases.projection; the reference is oracle/ref_cpu.py::favor_attention plus (out * wout).sum().backward() in float64 on the
float32 inputs; a kernel may be off by U.RTOL + 2 x the reference's own float32 error per tensor, dead tensors judged at dv's scale
(favor_cases.floors' rule).  That reference is itself the linear form, so its float32 run is a fair yardstick by construction.

Envelope of the route, stated here as literals (tests/test_favor_linear_cpu.py holds them against the constants in favor_linear.h):
  max(Nq, Nc) > 32, Nq, Nc >= 1, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536
"""
import functools
import types

import torch

from oracle import ref_cpu as O
from tests import favor_cases as FC
from tests import util as U

NAMES = FC.NAMES
VARIANT_SEED = {None: 0, "dup": 1, "outlier": 2, "peak_last": 3}


def in_envelope(T, H, Nq, Nc, d, m):
    return max(Nq, Nc) > 32 and Nq >= 1 and Nc >= 1 and d % 16 == 0 and 16 <= d <= 256 and 16 <= m <= 1536


def _case(shape, note, variant=None):
    """shape = (T, H, Nq, Nc, d, m); variant: None | "dup" | "outlier" | "peak_last"."""
    T, H, Nq, Nc, d, m = shape
    name = "T{}_H{}_Nq{}_Nc{}_d{}_m{}".format(*shape) + (f"_{variant}" if variant else "")
    # favor_cases' rule: one key -> out = v whatever q and k are (with the centre Ctx is exactly 0, so dq and dk are exactly 0); equal
    # keys -> out = mean(v) whatever q is; outlier -> dq and dk are cancellation residue.  Those are judged at dv's scale.
    dead = ("dq", "dk") if Nc == 1 or variant == "outlier" else (("dq",) if variant == "dup" else ())
    exact_zero = ("dq", "dk") if Nc == 1 else (("dq",) if variant == "dup" else ())
    return types.SimpleNamespace(name=name, shape=shape, T=T, H=H, Nq=Nq, Nc=Nc, d=d, m=m, note=note, variant=variant, dead=dead,
                                 exact_zero=exact_zero)


CASES = [
    _case((2, 2, 12, 33, 64, 266), "first size over the cap"),
    _case((1, 2, 33, 4, 32, 110), "Nq alone over the cap"),
    _case((2, 2, 40, 70, 64, 266), "both over, neither a multiple of 16"),
    _case((1, 2, 48, 96, 16, 16), "smallest d and m, exact tiles"),
    _case((1, 2, 5, 40, 64, 17), "15 padded features"),
    _case((1, 1, 5, 40, 64, 1536), "largest m"),
    _case((1, 1, 1, 64, 256, 1419), "widest d, one query"),
    _case((5, 3, 3, 35, 32, 110), "odd H, odd T"),
    _case((1, 2, 35, 1, 64, 266), "one key"),
    _case((2, 2, 40, 40, 64, 266), "every key equal, queries 0 and 1 equal", variant="dup"),
    _case((2, 2, 40, 40, 64, 266), "one key x 6: the floor terms carry the result", variant="outlier"),
    _case((2, 2, 40, 70, 64, 266), "the last key of the last task x 3: the batch maximum sits in the last task's last tile", variant="peak_last"),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
STAGED = BY_NAME["T2_H2_Nq12_Nc33_d64_m266"]
FUNCTION = [BY_NAME["T2_H2_Nq40_Nc70_d64_m266"], BY_NAME["T5_H3_Nq3_Nc35_d32_m110"]]      # the two cases that also go through FavorFunction


def seed_of(case):
    """favor_cases.seed_of's rule: a function of the shape and the variant alone."""
    s = 20261
    for x in case.shape:
        s = (s * 1000003 + x) % (2 ** 31 - 1)
    return s + VARIANT_SEED[case.variant]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 q [T,H,Nq,d], k, v [T,H,Nc,d], wout [T,H,Nq,d], proj [m,d], drawn as favor_cases.inputs draws them."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(seed_of(c))
    q = torch.randn(c.T, c.H, c.Nq, c.d, generator=g) * c.d ** -0.25
    k = torch.randn(c.T, c.H, c.Nc, c.d, generator=g) * c.d ** -0.25
    v = torch.randn(c.T, c.H, c.Nc, c.d, generator=g)
    wout = torch.randn(c.T, c.H, c.Nq, c.d, generator=g)
    if c.variant == "dup":
        k[:] = k[0, 0, 0].clone()
        q[:, :, 1] = q[:, :, 0]
    elif c.variant == "outlier":
        k[0, 0, 0] *= 6
    elif c.variant == "peak_last":
        k[-1, :, -1] *= 3
    return types.SimpleNamespace(q=q, k=k, v=v, wout=wout, proj=FC.projection(c.m, c.d))


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    x = inputs(name)
    q, k, v = (t.to(dtype).clone().requires_grad_() for t in (x.q, x.k, x.v))
    out = O.favor_attention(q, k, v, x.proj.to(dtype))
    (out * x.wout.to(dtype)).sum().backward()
    return tuple(t.detach().double() for t in (out, q.grad, k.grad, v.grad))


def reference(case, dtype=torch.float64):
    """(out, dq, dk, dv) of the autograd reference run in `dtype`, as float64 tensors [T,H,N,d].  Computed once; do not write into them."""
    return dict(zip(NAMES, _reference(case.name, dtype)))


floors = FC.floors                  # max|dv_ref| for the dead tensors, else no floor


@functools.lru_cache(maxsize=None)
def _e32(name):
    c = BY_NAME[name]
    r32, r64 = reference(c, torch.float32), reference(c, torch.float64)
    fl = floors(c, r64)
    return tuple(U.rel_err(r32[n], r64[n], fl[n]) for n in NAMES)


def e32(case):
    """The reference's own float32 error per tensor, at floors()."""
    return dict(zip(NAMES, _e32(case.name)))


def bounds(case):
    """favor_cases.bounds' rule: U.RTOL + 2 e32 per tensor."""
    return {n: U.RTOL + 2.0 * e for n, e in e32(case).items()}


kernel_layout = FC.kernel_layout
reference_layout = FC.reference_layout


def judge(case, got, what):
    """`got` (reference layout) is finite and inside bounds() of the float64 reference; every figure is printed before it is asserted."""
    ref, e, bound = reference(case, torch.float64), e32(case), bounds(case)
    floor = floors(case, ref)
    finite = {n: bool(torch.isfinite(got[n]).all()) for n in NAMES}
    err = {n: U.rel_err(got[n], ref[n], floor[n]) if finite[n] else float("inf") for n in NAMES}
    print(f"favor_linear {case.name} {what}: " + " ".join(f"{n}={err[n]:.2e}/{bound[n]:.2e}" for n in NAMES))
    assert all(finite.values()), (case.name, what, finite)
    for n in NAMES:
        assert err[n] <= bound[n], f"{case.name} {what}: {n} rel err {err[n]:.3e} > {bound[n]:.3e} (e32 {e[n]:.2e})"
    return err
