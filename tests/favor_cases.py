"""Shared by tests/test_favor_cases_cpu.py and tests/test_favor_envelope_gpu.py: the case table that walks the envelope of the FAVOR+
kernels (csrc/favor2.h fv::applies(), and favor.h's operator chain outside it) and the float64 reference every case is judged by.

The reference is oracle/ref_cpu.py::favor_attention, a restatement of networks/fast_attention.py that runs in any dtype; nothing here
needs a fixture.  The float32 inputs are the master copy: the float64 run converts those very float32 values, so the float32 run of
the same function (e32 below) measures the reference's own arithmetic error on the data the kernels see.

Route facts the table states itself (tests/test_favor_cases_cpu.py holds them against the constants in favor2.h):
  two-launch route  Nq <= 32, Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536
  row tiles         f1_kernel<2> / b2_kernel<2> for Nq + Nc <= 32, <4> above
  feature chunks    ceil(m / 192), four partial row maxima each (at most 32)
"""
import functools
import types

import torch

from oracle import ref_cpu as O
from tests import util as U

NAMES = ("out", "dq", "dk", "dv")
PROJ_SEED = 77


def _case(shape, note, route="two_launch", rt=None, chunks=None, variant=None):
    """shape = (T, H, Nq, Nc, d, m).  route: the side of fv::applies() the case sits on; rt: 16-row tiles per block of the F1 / B2
    instantiation (two-launch cases); chunks: F1 feature chunks; variant: None | "dup" | "outlier"."""
    T, H, Nq, Nc, d, m = shape
    name = "T{}_H{}_Nq{}_Nc{}_d{}_m{}".format(*shape) + (f"_{variant}" if variant else "")
    # tensors whose exact value is zero (one key: out = v whatever q and k are; equal keys: out = mean(v) whatever q is) or that are
    # cancellation residue (outlier): they are judged at dv's scale, and exempt from the liveness condition
    dead = ("dq", "dk") if Nc == 1 or variant == "outlier" else (("dq",) if variant == "dup" else ())
    exact_zero = ("dq", "dk") if Nc == 1 else (("dq",) if variant == "dup" else ())
    return types.SimpleNamespace(name=name, shape=shape, T=T, H=H, Nq=Nq, Nc=Nc, d=d, m=m, note=note, route=route, rt=rt, chunks=chunks,
                                 variant=variant, dead=dead, exact_zero=exact_zero)


CASES = [
    # ---- the two-launch route ----
    _case((2, 2, 1, 1, 64, 266), "one shot on each side", rt=2, chunks=2),
    _case((1, 1, 32, 1, 128, 621), "one key, 32 queries", rt=4, chunks=4),
    _case((1, 1, 1, 32, 256, 1419), "one query, 32 keys, widest d", rt=4, chunks=8),
    _case((1, 2, 16, 16, 32, 110), "32 rows: last shape of <2>", rt=2, chunks=1),
    _case((1, 2, 17, 16, 32, 110), "33 rows: first shape of <4>", rt=4, chunks=1),
    _case((2, 1, 16, 17, 16, 44), "smallest d, H = 1, less than one wave's 48 features", rt=4, chunks=1),
    _case((2, 2, 32, 32, 64, 266), "64 rows: both sides full", rt=4, chunks=2),
    _case((2, 8, 20, 20, 256, 1419), "the shipped width at 20 + 20", rt=4, chunks=8),
    _case((1, 2, 9, 24, 48, 185), "d not a multiple of 64, 24 key rows", rt=4, chunks=1),
    _case((1, 2, 6, 6, 80, 350), "d = 64 + 16", rt=2, chunks=2),
    _case((5, 3, 4, 3, 32, 110), "odd H, T not a power of two", rt=2, chunks=1),
    _case((1, 2, 5, 6, 64, 16), "smallest m", rt=2, chunks=1),
    _case((1, 2, 5, 6, 64, 17), "mp = 32: 15 padded features", rt=2, chunks=1),
    _case((1, 2, 7, 5, 64, 192), "exactly one chunk", rt=2, chunks=1),
    _case((1, 2, 7, 5, 64, 193), "one feature into the second chunk", rt=2, chunks=2),
    _case((1, 1, 5, 6, 64, 1536), "largest m, npart = 32", rt=2, chunks=8),
    # ---- outside applies(): favor.h's chain is the only route ----
    _case((2, 2, 12, 33, 64, 266), "Nc = 33", route="chain"),
    _case((1, 2, 33, 4, 32, 110), "Nq = 33", route="chain"),
    _case((1, 2, 6, 6, 40, 147), "d = 40: no multiple of 16", route="chain"),
    _case((1, 1, 5, 6, 64, 1537), "m = 1537", route="chain"),
    _case((1, 2, 5, 6, 64, 15), "m = 15", route="chain"),
    # ---- ties and cancellation ----
    _case((2, 2, 7, 5, 64, 266), "every key row equal, query rows 0 and 1 equal", rt=2, chunks=2, variant="dup"),
    _case((2, 2, 7, 5, 64, 266), "one key 6 x larger: every other key feature at the floor", rt=2, chunks=2, variant="outlier"),
    _case((2, 2, 32, 32, 64, 266), "every key row equal, query rows 0 and 1 equal, 64 rows", rt=4, chunks=2, variant="dup"),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
IN_ENVELOPE = [c for c in CASES if c.route == "two_launch"]
STAGED = [BY_NAME[n] for n in ("T1_H2_Nq17_Nc16_d32_m110", "T2_H2_Nq32_Nc32_d64_m266", "T2_H2_Nq12_Nc33_d64_m266")]


def seed_of(case):
    """One generator seed per case: a function of the shape and the variant alone."""
    s = 20261
    for x in case.shape:
        s = (s * 1000003 + x) % (2 ** 31 - 1)
    return s + {None: 0, "dup": 1, "outlier": 2}[case.variant]


@functools.lru_cache(maxsize=None)
def projection(m, d):
    """torch.manual_seed(77), then the reference's projection draw; the global generator is put back afterwards."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(PROJ_SEED)
        return O.gaussian_orthogonal_random_matrix(m, d).float().contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """float32 q [T,H,Nq,d], k, v [T,H,Nc,d], wout [T,H,Nq,d], proj [m,d].  q and k are randn * d ** -0.25 (dd has unit spread, the
    features sit far above the 1e-4 floor, so dq and dk are live); v and wout are plain randn."""
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
    return types.SimpleNamespace(q=q, k=k, v=v, wout=wout, proj=projection(c.m, c.d))


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    x = inputs(name)
    q, k, v = (t.to(dtype).clone().requires_grad_() for t in (x.q, x.k, x.v))
    out = O.favor_attention(q, k, v, x.proj.to(dtype))
    (out * x.wout.to(dtype)).sum().backward()
    return tuple(t.detach().double() for t in (out, q.grad, k.grad, v.grad))


def reference(case, dtype=torch.float64):
    """(out, dq, dk, dv) of O.favor_attention and (out * wout).sum().backward() run in `dtype` on the case's float32 inputs, as
    float64 tensors in the reference's [T,H,N,d] layout.  Computed once per (case, dtype); callers must not write into them."""
    return dict(zip(NAMES, _reference(case.name, dtype)))


def floors(case, ref64):
    """rel_err's floor per tensor: max|dv_ref| for the tensors whose own scale is zero or residue, else none."""
    dv_scale = ref64["dv"].abs().max().item()
    return {n: (dv_scale if n in case.dead else 0.0) for n in NAMES}


@functools.lru_cache(maxsize=None)
def _e32(name):
    c = BY_NAME[name]
    r32, r64 = reference(c, torch.float32), reference(c, torch.float64)
    fl = floors(c, r64)
    return tuple(U.rel_err(r32[n], r64[n], fl[n]) for n in NAMES)


def e32(case):
    """The reference's own float32 error per tensor: rel_err(reference(float32), reference(float64)) at floors()."""
    return dict(zip(NAMES, _e32(case.name)))


def bounds(case):
    """What a kernel may be off the float64 reference by: the project's tolerance plus twice the reference's own float32 error (the
    kernel sums in another order than the reference, so it may err as much again as the reference's float32 arithmetic does)."""
    return {n: U.RTOL + 2.0 * e for n, e in e32(case).items()}


def kernel_layout(x):
    """The kernels' operands from inputs(): q [T,Nq,H,d], k, v [T,Nc,H,d], dout [T,Nq,d*H] (merged order), proj - contiguous CPU."""
    T, H, Nq, d = x.q.shape
    qn, kn, vn = (t.permute(0, 2, 1, 3).contiguous() for t in (x.q, x.k, x.v))
    dout = x.wout.permute(0, 2, 3, 1).reshape(T, Nq, d * H).contiguous()
    return qn, kn, vn, dout, x.proj


def reference_layout(case, out, dq, dk, dv):
    """The kernels' results back in the reference's [T,H,N,d] layout."""
    out = out.view(case.T, case.Nq, case.d, case.H).permute(0, 3, 1, 2)
    return dict(out=out, dq=dq.permute(0, 2, 1, 3), dk=dk.permute(0, 2, 1, 3), dv=dv.permute(0, 2, 1, 3))
