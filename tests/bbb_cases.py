"""Shared by tests/test_bbb_cases_cpu.py and tests/test_bbb_envelope_gpu.py: the case table that walks the value and size edges of the
Bayes-by-backprop sample kernels (mlhot_bbb_sample_fwd / _bwd: csrc/ops_direct.h BbbSample / BbbSampleBwd under run_foreach and
run_reduce1; mlhot_bbb_sample_multi_fwd / _bwd: csrc/bbb_multi.h), the float64 reference every case is judged by, the bounds, and the
harness that calls the four C entries on buffers the test owns.  torch only at import; run() takes the library (GPU build or hostsim).

The operation, per element:  sigma = log1p(exp(rho)),  w = mu + eps sigma  (w2 = mu + eps2 sigma),
    klterm = 0.5 (2 log(sigma / 0.1) - 1 + (0.1 / sigma)^2 + (mu / sigma)^2),   kl = sum of klterm over every element of every item,
and the gradients of  sum(w dw) + sum(w2 dw2) + dkl kl  for mu and rho.  The reference writes exactly that in float64 and takes the
gradients by float64 autograd.  The float32 inputs are the master copy: the float64 run converts those very values.

How an output is judged: beside each output element the reference computes its TERM SCALE S_i, the sum of the absolute values of its
addends (scales() below).  The error of a case is max_i |x_i - x64_i| / S_i - a rounding error of a few ulp in any addend is a few
2^-24 of S_i however the addends cancel (they do: 1 / sigma - 0.01 / sigma^3 - mu^2 / sigma^3 passes through zero at sigma = 0.1).
Where S_i = 0 every addend is zero and the output must be exactly the reference's.

The bounds are not chosen: REF32_WORST holds the same error of the SAME expression in float32 (torch on the CPU, autograd for the
gradients) against float64, worst over the table, as measured by tests/test_bbb_cases_cpu.py; BOUND = 4 x that, the factor allowing a
different but legitimate order of summation and expf / log1pf implementation.  The CPU test re-measures and holds the float32 reference
under BOUND / 4."""
import ctypes as C
import functools
import math
import types
import zlib

import torch

RHO_EDGE = math.log(math.expm1(0.1))          # sigma = 0.1: 1 / sigma - 0.01 / sigma^3 = 0 and log(sigma / 0.1) = 0
RHOS = (-12.0, -8.0, -5.0, -3.0, RHO_EDGE - 1e-3, RHO_EDGE, RHO_EDGE + 1e-3, -1.0, 0.0, 3.0, 12.0)
MUS = (0.0, 1e-3, -1e-3, 0.1, -0.1, 3.0, -3.0)
EPSS = (0.0, 1.0, -1.0, 4.0, -4.0)
CROSS = len(RHOS) * len(MUS) * len(EPSS)      # 385 (rho, mu, eps) triples
OVERFLOW_RHOS = (88.0, 89.0, 100.0)           # expf overflows between 88 and 89: the recorded-behaviour case
DKLS = (0.0, 1e-7, 0.3, 1.0)
KINDS = ("w", "klterm", "kl", "dmu", "drho")

# max_i |x32_i - x64_i| / S_i of the float32 reference expression, worst over CASES (measured; test_bbb_cases_cpu.py re-measures)
REF32_WORST = dict(w=1.9e-07, klterm=4.9e-07, kl=1.8e-07, dmu=4.4e-07, drho=7.1e-07)
BOUND = {k: 4.0 * v for k, v in REF32_WORST.items()}

GRID_CLAMP = 256 * 16 * 256                   # run_foreach launches at most 256 * 16 workgroups of 256 threads
BAND = 64                                     # NaN floats in front of, between and behind the output slices


def _item(n, dw=True, two="none"):
    """two: "none" (no eps2), "dw2" (eps2 and dw2), "nodw2" (eps2, dw2 = NULL: the second sample received no gradient)."""
    assert two in ("none", "dw2", "nodw2")
    return types.SimpleNamespace(n=n, dw=dw, two=two)


def _case(name, items, dkl, fill="cross", note=""):
    return types.SimpleNamespace(name=name, items=items, dkl=dkl, fill=fill, note=note,
                                 both=len(items) == 1 and items[0].dw and items[0].two == "none")


SINGLE_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 3073, 4095, 4096, 4097, GRID_CLAMP + 1)
ITEM_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049)


def _table():
    c = []
    # ---- one tensor, both routes: the 256-thread block, the 1024-element chunk, reduce1's 4 x 1024 stride, the grid clamp ----
    for k, n in enumerate(SINGLE_SIZES):
        c.append(_case(f"one_n{n}", [_item(n)], DKLS[(k + 2) % 4]))
    for dkl in DKLS:
        c.append(_case(f"one_n1025_dkl{dkl:g}", [_item(1025)], dkl))
    c.append(_case("one_n2049_random", [_item(2049)], 0.3, fill="random"))
    # ---- one item, the forms only the multi route has ----
    c.append(_case("multi1_no_dw", [_item(1025, dw=False)], 0.3))
    c.append(_case("multi1_no_dw_dkl0", [_item(1025, dw=False)], 0.0, note="gradients exactly 0"))
    c.append(_case("multi1_two", [_item(1025, two="dw2")], 1.0))
    c.append(_case("multi1_two_nodw2", [_item(1025, two="nodw2")], 1e-7))
    c.append(_case("multi1_only_dw2", [_item(257, dw=False, two="dw2")], 0.3))
    # ---- two items: a chunk boundary that is an item boundary, the last item has one element ----
    c.append(_case("multi2_1024_1", [_item(1024), _item(1, dw=False)], 0.3))
    c.append(_case("multi2_1_1", [_item(1, two="dw2"), _item(1)], 1.0))
    c.append(_case("multi2_2049_1_dkl0", [_item(2049, two="nodw2"), _item(1, dw=False)], 0.0))
    # ---- single-chunk items before and after multi-chunk ones ----
    c.append(_case("multi_mixed_chunks", [_item(1), _item(2049), _item(255, dw=False), _item(1025, two="dw2"), _item(1024), _item(2049, two="nodw2"),
                                          _item(257), _item(1)], 0.3))
    # ---- 32 items: every size, every form; item 3 mod 5 has no dw; the last item has one element ----
    forms = ("none", "dw2", "nodw2")
    for dkl in (0.0, 1.0):
        items = [_item(ITEM_SIZES[(i * 3 + 1) % 8], dw=i % 5 != 3, two=forms[i % 3]) for i in range(31)] + [_item(1, two="dw2")]
        c.append(_case(f"multi32_dkl{dkl:g}", items, dkl))
    # ---- many workgroups: the item search with large block indices, the partial reduce's strides ----
    c.append(_case("multi_1025_workgroups", [_item(1), _item(1022 * 1024 + 1, two="dw2"), _item(1, dw=False)], 1e-7, note="1 + 1023 + 1"))
    c.append(_case("multi_4097_workgroups", [_item(4096 * 1024 + 1)], 0.3, note="past the i + 3072 < n loop of the partial reduce"))
    return c


CASES = _table()
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BOTH = [c for c in CASES if c.both]
LARGEST = ("one_n1048577", "multi_1025_workgroups", "multi_4097_workgroups")          # a million elements and more
OVERFLOW = _case("overflow", [_item(len(OVERFLOW_RHOS) * len(MUS) * len(EPSS))], 0.3, fill="overflow", note="recorded behaviour, no float64 target")


def workgroups(c):
    return sum((it.n + 1023) // 1024 for it in c.items)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _values(n, fill, g, rot):
    """float32 (mu, rho, eps, eps2) of n elements.  "cross": elements 0 .. 769 walk the whole (rho, mu, eps) cross twice, from triple
    `rot` on (eps2 takes another eps value of the same set), the elements behind them are random draws of the same ranges."""
    if fill == "overflow":
        k = torch.arange(n)
        rho = torch.tensor(OVERFLOW_RHOS)[k % 3]
        mu, eps = torch.tensor(MUS)[(k // 3) % 7], torch.tensor(EPSS)[k // 21]
        return mu, rho, eps, torch.tensor(EPSS)[(k // 21 + 1) % 5]
    rho = torch.rand(n, generator=g) * 24.0 - 12.0
    mu = 10.0 ** (torch.rand(n, generator=g) * 3.5 - 3.0) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)       # 1e-3 .. 3.16, both signs
    eps = torch.randn(n, generator=g).clamp(-4.0, 4.0)
    eps2 = torch.randn(n, generator=g).clamp(-4.0, 4.0)
    if fill == "cross":
        m = min(n, 2 * CROSS)
        k = (torch.arange(m) + rot) % CROSS
        rho[:m] = torch.tensor(RHOS, dtype=torch.float64)[k % 11].float()
        mu[:m] = torch.tensor(MUS)[(k // 11) % 7]
        eps[:m] = torch.tensor(EPSS)[k // 77]
        eps2[:m] = torch.tensor(EPSS)[(k // 77 + 1 + k % 3) % 5]
    else:
        assert fill == "random", fill
    return mu.clamp(-3.0, 3.0), rho, eps, eps2


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = OVERFLOW if name == "overflow" else BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    out = []
    for i, it in enumerate(c.items):
        mu, rho, eps, eps2 = _values(it.n, c.fill, g, rot=(i * 97 + zlib.crc32(name.encode())) % CROSS)
        out.append(types.SimpleNamespace(mu=mu, rho=rho, eps=eps, eps2=eps2 if it.two != "none" else None,
                                         dw=torch.randn(it.n, generator=g) if it.dw else None,
                                         dw2=torch.randn(it.n, generator=g) if it.two == "dw2" else None))
    return out


def inputs(c):
    """Per item: float32 mu, rho, eps, eps2 / dw / dw2 (None where the item has none); callers must not write into them."""
    return _inputs(c.name)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def expression(c, dtype):
    """The operation as torch tensor arithmetic in `dtype`, gradients by autograd -> per item (w, w2, klterm, dmu, drho), kl."""
    items, kl, total, keep = [], 0.0, 0.0, []
    for it, x in zip(c.items, inputs(c)):
        mu, rho = x.mu.to(dtype).clone().requires_grad_(), x.rho.to(dtype).clone().requires_grad_()
        sigma = torch.log1p(torch.exp(rho))
        w = mu + x.eps.to(dtype) * sigma
        w2 = mu + x.eps2.to(dtype) * sigma if x.eps2 is not None else None
        klterm = 0.5 * (2 * torch.log(sigma / 0.1) - 1 + (0.1 / sigma).pow(2) + (mu / sigma).pow(2))
        kl = kl + klterm.sum()
        if x.dw is not None:
            total = total + (w * x.dw.to(dtype)).sum()
        if x.dw2 is not None:
            total = total + (w2 * x.dw2.to(dtype)).sum()
        keep.append((mu, rho, w, w2, klterm))
    (total + c.dkl * kl).backward()
    for mu, rho, w, w2, klterm in keep:
        items.append(types.SimpleNamespace(w=w.detach(), w2=None if w2 is None else w2.detach(), klterm=klterm.detach(), dmu=mu.grad, drho=rho.grad))
    return items, kl.detach()


def scales(c):
    """Per item the term scales S_i of w, w2, klterm, dmu, drho (float64), and of the scalar kl (the sum of klterm's)."""
    out, skl = [], 0.0
    for x in inputs(c):
        mu, rho, eps = x.mu.double(), x.rho.double(), x.eps.double()
        sigma, g = torch.log1p(torch.exp(rho)), abs(c.dkl)
        zero = torch.zeros_like(mu)
        dw, dw2 = (zero if x.dw is None else x.dw.double().abs()), (zero if x.dw2 is None else x.dw2.double().abs())
        eps2 = zero if x.eps2 is None else x.eps2.double()
        s = types.SimpleNamespace(
            w=mu.abs() + (eps * sigma).abs(), w2=mu.abs() + (eps2 * sigma).abs(),
            klterm=0.5 * ((2 * torch.log(sigma / 0.1)).abs() + 1 + (0.1 / sigma) ** 2 + (mu / sigma) ** 2),
            dmu=dw + dw2 + g * mu.abs() / sigma ** 2,
            drho=torch.sigmoid(rho) * (dw * eps.abs() + dw2 * eps2.abs() + g * (1 / sigma + 0.01 / sigma ** 3 + mu ** 2 / sigma ** 3)))
        skl = skl + float(s.klterm.sum())
        out.append(s)
    return out, skl


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    items, kl = expression(c, torch.float64)
    s, skl = scales(c)
    return types.SimpleNamespace(items=items, kl=kl, scales=s, kl_scale=skl)


def reference(c):
    """float64 outputs and term scales, computed once per case; callers must not write into them."""
    return _reference(c.name)


# ---- judging -------------------------------------------------------------------------------------------------------------------
def term_err(got, want, scale):
    """max_i |got_i - want_i| / S_i; where S_i = 0 the element must equal the reference exactly (else inf)."""
    got, want = got.detach().double().cpu().reshape(-1), want.reshape(-1)
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    if got.numel() == 0:
        return 0.0
    d = (got - want).abs()
    e = torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    return float(e.max())


def errors(c, out):
    """out: what run() or expression() returned, as (items, kl) -> {kind: worst error over the items of the case}.  klterm is judged
    where the output has it (the single-tensor route and the expression; the multi route sums it inside the kernel)."""
    items, kl = out
    r = reference(c)
    err = dict(w=0.0, dmu=0.0, drho=0.0)
    for it, o, want, s in zip(c.items, items, r.items, r.scales):
        err["w"] = max(err["w"], term_err(o.w, want.w, s.w))
        if it.two != "none":
            err["w"] = max(err["w"], term_err(o.w2, want.w2, s.w2))
        if getattr(o, "klterm", None) is not None:
            err["klterm"] = max(err.get("klterm", 0.0), term_err(o.klterm, want.klterm, s.klterm))
        err["dmu"] = max(err["dmu"], term_err(o.dmu, want.dmu, s.dmu))
        err["drho"] = max(err["drho"], term_err(o.drho, want.drho, s.drho))
    err["kl"] = abs(float(kl) - float(r.kl)) / r.kl_scale
    return err


def exact_zero_items(c):
    """Items whose gradients are exactly 0: no gradient reaches either sample and the KL's is 0."""
    return [i for i, it in enumerate(c.items) if c.dkl == 0.0 and not it.dw and it.two != "dw2"]


# ---- the harness: the C entries on buffers the test owns -----------------------------------------------------------------------
NAN_BITS = 0x7fc00000


class _Arena:
    """One float32 buffer filled with NaN; the outputs are slices of it with BAND NaN floats in front of, between and behind them."""

    def __init__(self, sizes, device):
        self.bounds, off = [], BAND
        for n in sizes:
            self.bounds.append((off, off + n))
            off += n + BAND
        self.buf = torch.full((off,), float("nan"), device=device)

    def view(self, i):
        lo, hi = self.bounds[i]
        return self.buf[lo:hi]

    def bands_untouched(self):
        bits = self.buf.cpu().view(torch.int32)
        inside = torch.zeros(bits.numel(), dtype=torch.bool)
        for lo, hi in self.bounds:
            inside[lo:hi] = True
        return bool((bits[~inside] == NAN_BITS).all())


def _P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream) if torch.device(device).type == "cuda" else None


def _ok(lib, rc, what):
    assert rc == 0, f"{what}: rc {rc}: {lib.c.mlhot_last_error().decode()}"


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def run(lib, c, route, device):
    """The case through mlhot_bbb_sample_fwd / _bwd (route "single": one item with dw and without eps2) or mlhot_bbb_sample_multi_fwd /
    _bwd (route "multi") with every output a slice of a NaN-filled buffer -> (items [w, w2, klterm, dmu, drho on the CPU], kl,
    whether every float outside the slices is still the NaN it was)."""
    from mlhot.binding import BbbItem
    x = [types.SimpleNamespace(**{k: (None if v is None else v.to(device)) for k, v in vars(i).items()}) for i in inputs(c)]
    ns = [it.n for it in c.items]
    w, w2, dmu, drho, klt = (_Arena(ns, device) for _ in range(5))
    kl = torch.full((3,), float("nan"), device=device)
    dkl = torch.tensor(c.dkl, device=device)
    s = _stream(device)
    if route == "single":
        assert c.both
        i = x[0]
        _ok(lib, lib.c.mlhot_bbb_sample_fwd(_P(i.mu), _P(i.rho), _P(i.eps), _P(w.view(0)), _P(klt.view(0)), _P(kl[1:]), ns[0], s), "bbb_sample_fwd")
        _ok(lib, lib.c.mlhot_bbb_sample_bwd(_P(i.mu), _P(i.rho), _P(i.eps), _P(i.dw), _P(dkl), _P(dmu.view(0)), _P(drho.view(0)), ns[0], s), "bbb_sample_bwd")
    else:
        assert route == "multi"
        arr = (BbbItem * len(ns))()
        for k, (it, i) in enumerate(zip(c.items, x)):
            a = arr[k]
            a.mu, a.rho, a.eps, a.n = i.mu.data_ptr(), i.rho.data_ptr(), i.eps.data_ptr(), it.n
            a.w, a.dmu, a.drho = w.view(k).data_ptr(), dmu.view(k).data_ptr(), drho.view(k).data_ptr()
            a.dw = None if i.dw is None else i.dw.data_ptr()
            a.eps2 = None if i.eps2 is None else i.eps2.data_ptr()
            a.w2 = None if i.eps2 is None else w2.view(k).data_ptr()
            a.dw2 = None if i.dw2 is None else i.dw2.data_ptr()
        npart = lib.c.mlhot_bbb_sample_multi_scratch_floats(arr, len(ns))
        assert npart == max(1, workgroups(c))
        partial = _Arena([npart], device)
        _ok(lib, lib.c.mlhot_bbb_sample_multi_fwd(arr, len(ns), _P(partial.view(0)), _P(kl[1:]), s), "bbb_sample_multi_fwd")
        _ok(lib, lib.c.mlhot_bbb_sample_multi_bwd(arr, len(ns), _P(dkl), s), "bbb_sample_multi_bwd")
    _sync(device)
    klc = kl.cpu()
    clean = all(a.bands_untouched() for a in (w, w2, dmu, drho, klt)) and bool(torch.isnan(klc[0])) and bool(torch.isnan(klc[2]))
    if route == "multi":
        clean = clean and partial.bands_untouched() and bool(torch.isnan(klt.buf).all())
        for k, it in enumerate(c.items):
            if it.two == "none":
                clean = clean and bool(torch.isnan(w2.view(k)).all())           # no second sample: w2 is not written
    else:
        clean = clean and bool(torch.isnan(w2.buf).all())
    items = []
    for k, it in enumerate(c.items):
        items.append(types.SimpleNamespace(w=w.view(k).cpu(), w2=w2.view(k).cpu() if it.two != "none" else None,
                                           klterm=klt.view(k).cpu() if route == "single" else None, dmu=dmu.view(k).cpu(), drho=drho.view(k).cpu()))
    return items, klc[1], clean


def same_bits(a, b):
    """Two results of run(): every output bit for bit."""
    (ia, ka, _), (ib, kb, _) = a, b
    def eq(p, q):
        return (p is None and q is None) or torch.equal(p.view(torch.int32), q.view(torch.int32))
    return eq(ka.reshape(1), kb.reshape(1)) and all(eq(getattr(p, f), getattr(q, f)) for p, q in zip(ia, ib) for f in ("w", "w2", "klterm", "dmu", "drho"))


def nonfinite_pattern(t):
    """0 finite, 1 +inf, 2 -inf, 3 nan, per element."""
    t = t.detach().float().cpu().reshape(-1)
    return torch.isposinf(t) * 1 + torch.isneginf(t) * 2 + torch.isnan(t) * 3
