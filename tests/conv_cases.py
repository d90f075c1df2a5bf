"""Shared by tests/test_conv_cases_cpu.py and tests/test_conv_envelope_gpu.py: the case table that walks the envelope of the
run-time-shaped convolution (csrc/conv_rt.h, ConvFwdRT / ConvDgradRT / ConvWgradRT in csrc/problems.h, csrc/igemm.h), the two kinds
of input every case is run on, and the float64 reference it is judged by.

A case is (N, Cin, H, W, Cout, k, s, p) and states the route it takes as literals; route() restates conv_rt.h and igemm.h in Python
and tests/test_conv_cases_cpu.py holds the literals against it (and against the library where the library exposes them):
  fwd    (row tile, wgs64)                 run_conv_igemm: 16-row tiles while wgs64 = ceil(M / 64) ceil(N / 64) < 128, else 128-row
  dgrad  (classes, no tap, skipped, batches)
                                           s * s parity classes of input positions; a class with ny == 0 or nx == 0 is skipped, one
                                           that no tap reaches (stride > k) stores zeros; the others go out four to a launch, and each
                                           launch picks its tile by the SUM of its members' wgs64: batches = ((members, row tile), ...)
  wgrad  (split asked, split run)          conv_wgrad_split (what the scratch is sized by), and what run_igemm makes of it once
                                           k_chunk is a multiple of 32

Exact pass: x, w, b, dy are integers of {-3 .. 3} in float32.  Every product and partial sum, in any order and through any split, is
an integer below 9 K + 3 < 2^24, so the float64 reference IS the float32 result: the kernels must return its bits.  Real pass: unit
normals (w scaled by 1 / sqrt(Cin k k)), judged by
    rel_err(kernel, float64) <= tol + 2 x rel_err(torch float32 on the CPU, float64)        tol = 1e-5 (y), 2e-5 (dx, dw, db)
"""
import ctypes as C
import functools
import types

import torch
import torch.nn.functional as F

from tests import util as U

NAMES = ("y", "dx", "dw", "db")
TOL = dict(y=1e-5, dx=2e-5, dw=2e-5, db=2e-5)      # what tests/test_gpu_parity.py::test_conv2d_runtime_shapes_vs_torch holds
KINDS = ("exact", "real")
ERR_ARG, ERR_WORKSPACE = 1, 2                      # csrc/common.h MLHOT_ERR_ARG, MLHOT_ERR_WORKSPACE
CONV_BK = 32                                       # conv_rt.h: k-depth of one igemm iteration; run_igemm rounds k_chunk up to it


def _cdiv(a, b):
    return -(-a // b)


def geometry(shape):
    N, Cin, H, W, Cout, k, s, p = shape
    HO, WO = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return types.SimpleNamespace(HO=HO, WO=WO, pos=N * HO * WO, K=Cin * k * k)


def route(shape):
    """conv_rt.h's and igemm.h's host decisions for one shape, restated."""
    N, Cin, H, W, Cout, k, s, p = shape
    g = geometry(shape)
    tile = lambda wgs64: 16 if wgs64 < 128 else 128
    fwd_wgs = _cdiv(g.pos, 64) * _cdiv(Cout, 64)
    # conv_rt_backward: the parity classes in launch order
    classes, skipped = [], 0
    for py in range(s):
        for px in range(s):
            ky0, kx0 = (py + p) % s, (px + p) % s
            nty = _cdiv(k - ky0, s) if ky0 < k else 0
            ntx = _cdiv(k - kx0, s) if kx0 < k else 0
            ny, nx = (H - py + s - 1) // s, (W - px + s - 1) // s
            if ny <= 0 or nx <= 0:
                skipped += 1
                continue
            M = N * ny * nx
            classes.append(types.SimpleNamespace(py=py, px=px, ny=ny, nx=nx, nty=nty, ntx=ntx, M=M, K=nty * ntx * Cout,
                                                 wgs=_cdiv(M, 64) * _cdiv(Cin, 64)))
    batches = tuple((len(b), tile(sum(c.wgs for c in b))) for b in (classes[i:i + 4] for i in range(0, len(classes), 4)))
    # conv_wgrad_split, then run_igemm's k_chunk rounding
    tiles = _cdiv(Cout, 64) * _cdiv(g.K + 1, 64)
    asked = max(1, min(_cdiv(512, tiles), g.pos // 64, 256))
    k_chunk = max(CONV_BK, _cdiv(_cdiv(g.pos, asked), CONV_BK) * CONV_BK)
    run = max(1, _cdiv(g.pos, k_chunk))
    return types.SimpleNamespace(fwd=(tile(fwd_wgs), fwd_wgs),
                                 dgrad=(s * s, sum(c.K == 0 for c in classes), skipped, batches),
                                 wgrad=(asked, run), classes=classes, tiles=tiles, k_chunk=k_chunk,
                                 last_chunk=g.pos - (run - 1) * k_chunk, bias_col=g.K % 64,
                                 max_K=max([g.K, g.pos] + [c.K for c in classes]))


def _case(shape, note, fwd, dgrad, wgrad):
    N, Cin, H, W, Cout, k, s, p = shape
    name = "N{}_C{}_{}x{}_O{}_k{}_s{}_p{}".format(*shape)
    return types.SimpleNamespace(name=name, shape=shape, N=N, Cin=Cin, H=H, W=W, Cout=Cout, k=k, s=s, p=p, note=note, fwd=fwd, dgrad=dgrad,
                                 wgrad=wgrad, **vars(geometry(shape)))


CASES = [
    # ---- forward: the tile switch and the K edges ----
    _case((1, 1, 64, 127, 8, 1, 1, 0), "fwd wgs64 = 127: last shape of the 16-row tile, K = 1",
          fwd=(16, 127), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(127, 127)),
    _case((1, 1, 64, 128, 8, 1, 1, 0), "fwd wgs64 = 128: first shape of the 128-row tile",
          fwd=(128, 128), dgrad=(1, 0, 0, ((1, 128),)), wgrad=(128, 128)),
    _case((1, 3, 65, 126, 8, 3, 1, 1), "M = 8190: partial last 128-row tile, K = 27 < 32",
          fwd=(128, 128), dgrad=(1, 0, 0, ((1, 128),)), wgrad=(127, 86)),
    _case((1, 3, 9, 14, 5, 5, 2, 2), "K = 75: the 5 x 5 stem on 3 channels",
          fwd=(16, 1), dgrad=(4, 0, 0, ((4, 16),)), wgrad=(1, 1)),
    _case((1, 2, 10, 13, 6, 4, 2, 1), "K = 32 exactly; even kernel k = 4, stride 2",
          fwd=(16, 1), dgrad=(4, 0, 0, ((4, 16),)), wgrad=(1, 1)),
    _case((1, 2, 63, 64, 65, 3, 1, 1), "Cout = 65: a second N tile of one column, 16-row side (wgs64 = 126)",
          fwd=(16, 126), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(63, 63)),
    _case((1, 2, 64, 64, 65, 3, 1, 1), "Cout = 65: a second N tile of one column, 128-row side (wgs64 = 128)",
          fwd=(128, 128), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(64, 64)),
    # ---- data gradient: N tiles, class batches, class and padding edges ----
    _case((1, 70, 6, 9, 4, 3, 1, 1), "dgrad N = Cin = 70 on 16-row tiles",
          fwd=(16, 1), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    _case((1, 65, 64, 64, 4, 3, 1, 1), "dgrad N = Cin = 65 on 128-row tiles",
          fwd=(16, 64), dgrad=(1, 0, 0, ((1, 128),)), wgrad=(52, 43)),
    _case((2, 4, 64, 64, 8, 3, 2, 1), "stride 2: four classes of 32 workgroups, the sum (128) decides: 128-row tiles",
          fwd=(16, 32), dgrad=(4, 0, 0, ((4, 128),)), wgrad=(32, 32)),
    _case((2, 4, 62, 64, 8, 3, 2, 1), "stride 2: four classes of 31 workgroups, sum 124: 16-row tiles",
          fwd=(16, 31), dgrad=(4, 0, 0, ((4, 16),)), wgrad=(31, 31)),
    _case((1, 2, 144, 144, 3, 3, 3, 1), "stride 3: 9 classes of 36 workgroups, batches 4 + 4 (128-row) + 1 (16-row) in one call",
          fwd=(16, 36), dgrad=(9, 0, 0, ((4, 128), (4, 128), (1, 16))), wgrad=(36, 36)),
    _case((1, 2, 11, 7, 3, 3, 3, 1), "stride 3 with H > W",
          fwd=(16, 1), dgrad=(9, 0, 0, ((4, 16), (4, 16), (1, 16))), wgrad=(1, 1)),
    _case((1, 2, 9, 10, 3, 3, 4, 1), "stride 4 > k: 16 classes, 7 without a tap (stored zeros)",
          fwd=(16, 1), dgrad=(16, 7, 0, ((4, 16), (4, 16), (4, 16), (4, 16))), wgrad=(1, 1)),
    _case((2, 4, 7, 10, 70, 1, 2, 0), "k = 1, stride 2, Cout = 70: three of four classes without a tap; wgrad second M tile",
          fwd=(16, 2), dgrad=(4, 3, 0, ((4, 16),)), wgrad=(1, 1)),
    _case((1, 1, 1, 7, 2, 1, 2, 1), "H < stride: the odd-row classes have ny == 0 and are skipped; pad >= k: every output is bias only",
          fwd=(16, 1), dgrad=(4, 2, 2, ((2, 16),)), wgrad=(1, 1)),
    _case((2, 3, 10, 7, 4, 5, 2, 2), "(H + 2p - k) % s != 0: the trailing input row gets fewer taps; stride 2 with H > W",
          fwd=(16, 1), dgrad=(4, 0, 0, ((4, 16),)), wgrad=(1, 1)),
    _case((1, 2, 6, 8, 3, 3, 2, 0), "p = 0: the last input row and column are reached by no output, dx there is a stored 0",
          fwd=(16, 1), dgrad=(4, 0, 0, ((4, 16),)), wgrad=(1, 1)),
    _case((1, 2, 6, 9, 3, 2, 3, 0), "even kernel k = 2 under stride 3: 5 of 9 classes without a tap",
          fwd=(16, 1), dgrad=(9, 5, 0, ((4, 16), (4, 16), (1, 16))), wgrad=(1, 1)),
    _case((1, 4, 9, 6, 3, 4, 1, 2), "k = 4, stride 1, Cin k k + 1 = 65: the bias column alone in its tile",
          fwd=(16, 2), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    # ---- weight gradient: split-K ----
    _case((1, 2, 7, 9, 3, 3, 1, 1), "pos = 63: split 1",
          fwd=(16, 1), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    _case((1, 2, 4, 16, 3, 3, 1, 1), "pos = 64: split 1",
          fwd=(16, 1), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    _case((1, 2, 1, 127, 3, 3, 1, 1), "pos = 127: split 1",
          fwd=(16, 2), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    _case((1, 2, 8, 16, 3, 3, 1, 1), "pos = 128: split 2",
          fwd=(16, 2), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(2, 2)),
    _case((1, 2, 18, 32, 3, 3, 1, 1), "pos = 576: asks 9, runs 9",
          fwd=(16, 9), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(9, 9)),
    _case((1, 2, 20, 30, 3, 3, 1, 1), "pos = 600: asks 9, k_chunk 96, runs 7 with a last chunk of 24",
          fwd=(16, 10), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(9, 7)),
    _case((4, 1, 64, 64, 8, 3, 1, 1), "pos = 16384: the cap of 256 splits",
          fwd=(128, 256), dgrad=(1, 0, 0, ((1, 128),)), wgrad=(256, 256)),
    _case((1, 1, 127, 129, 4, 3, 1, 1), "pos = 16383: asks 255, k_chunk 96, runs 171 (no multiple of 8)",
          fwd=(128, 256), dgrad=(1, 0, 0, ((1, 128),)), wgrad=(255, 171)),
    _case((1, 3, 16, 20, 70, 3, 1, 1), "Cout = 70: a second M tile under a split",
          fwd=(16, 10), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(5, 5)),
    _case((1, 7, 9, 12, 5, 3, 1, 1), "Cin k k + 1 = 64: the bias column is the last of its tile",
          fwd=(16, 2), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    _case((1, 64, 6, 11, 5, 1, 1, 0), "Cin k k + 1 = 65 (k = 1): the bias column alone in its tile; fwd K = 64",
          fwd=(16, 2), dgrad=(1, 0, 0, ((1, 16),)), wgrad=(1, 1)),
    _case((1, 128, 88, 126, 2, 1, 1, 0), "3 tiles: ceil(512 / 3) = 171 binds the split, not pos / 64 = 173",
          fwd=(128, 174), dgrad=(1, 0, 0, ((1, 128),)), wgrad=(171, 116)),
]
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the split-K cases whose slab reduction is run twice and compared bit for bit: the 256 cap, 171 and 7 splits
TWICE = [BY_NAME[n] for n in ("N4_C1_64x64_O8_k3_s1_p1", "N1_C1_127x129_O4_k3_s1_p1", "N1_C2_20x30_O3_k3_s1_p1")]
# the cases run through the C entry points on NaN-filled outputs between guard bands
BANDED = [BY_NAME[n] for n in ("N1_C2_9x10_O3_k3_s4_p1", "N1_C2_6x8_O3_k3_s2_p0", "N1_C1_1x7_O2_k1_s2_p1", "N1_C2_63x64_O65_k3_s1_p1",
                               "N1_C2_64x64_O65_k3_s1_p1", "N1_C1_127x129_O4_k3_s1_p1", "N1_C2_11x7_O3_k3_s3_p1", "N1_C4_9x6_O3_k4_s1_p2")]


def seed_of(case, kind):
    """One generator seed per (case, kind of input): a function of the shape alone."""
    s = 20263 + KINDS.index(kind)
    for x in case.shape:
        s = (s * 1000003 + x) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    """float32 x [N,Cin,H,W], w [Cout,Cin,k,k], b [Cout], dy [N,Cout,HO,WO].  Callers must not write into them."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(seed_of(c, kind))
    shapes = ((c.N, c.Cin, c.H, c.W), (c.Cout, c.Cin, c.k, c.k), (c.Cout,), (c.N, c.Cout, c.HO, c.WO))
    if kind == "exact":
        x, w, b, dy = (torch.randint(-3, 4, s, generator=g).float() for s in shapes)
    else:
        x, w, b, dy = (torch.randn(s, generator=g) for s in shapes)
        w = w / (c.Cin * c.k * c.k) ** 0.5
    return types.SimpleNamespace(x=x, w=w, b=b, dy=dy)


@functools.lru_cache(maxsize=None)
def _forward(name, kind, bias, dtype):
    c, i = BY_NAME[name], inputs(name, kind)
    return F.conv2d(i.x.to(dtype), i.w.to(dtype), i.b.to(dtype) if bias else None, stride=c.s, padding=c.p)


def preact(case, kind, bias=True, dtype=torch.float64):
    """The convolution before its ReLU, in `dtype` on the case's float32 inputs."""
    return _forward(case.name, kind, bias, dtype)


def _grads(case, kind, dtype, mask):
    """The linear backward of dy * mask (mask None: of dy) in `dtype`: dx, dw, db as float64."""
    i = inputs(case.name, kind)
    x, w = (t.to(dtype).clone().requires_grad_() for t in (i.x, i.w))
    g = i.dy.to(dtype) if mask is None else i.dy.to(dtype) * mask.to(dtype)
    F.conv2d(x, w, None, stride=case.s, padding=case.p).backward(g)
    return x.grad.double(), w.grad.double(), g.sum(dim=(0, 2, 3)).double()


@functools.lru_cache(maxsize=None)
def _reference(name, kind, relu, bias, dtype):
    c = BY_NAME[name]
    pre = preact(c, kind, bias, dtype)
    # the float64 pre-activation decides the mask in either dtype: e32 then measures arithmetic, never a flipped decision
    mask = (preact(c, kind, bias, torch.float64) > 0) if relu else None
    return (torch.relu(pre).double() if relu else pre.double(),) + _grads(c, kind, dtype, mask)


def reference(case, kind, relu, bias=True, dtype=torch.float64, mask=None):
    """{y, dx, dw, db} as float64 tensors: F.conv2d (+ ReLU) and the backward of dy through it, run in `dtype`.  With relu the gradient
    is taken under `mask` (a bool tensor of y's shape: the kernel's own y > 0, which is what Conv2dFunction differentiates through);
    None or a mask equal to the float64 pre-activation's sign gives the cached tensors, which callers must not write into."""
    ref = dict(zip(NAMES, _reference(case.name, kind, bool(relu), bool(bias), dtype)))
    if relu and mask is not None and not torch.equal(mask.reshape(ref["y"].shape), preact(case, kind, bias, torch.float64) > 0):
        ref.update(zip(NAMES[1:], _grads(case, kind, dtype, mask.reshape(ref["y"].shape))))
    return ref


@functools.lru_cache(maxsize=None)
def _e32(name, relu, bias):
    c = BY_NAME[name]
    r32, r64 = reference(c, "real", relu, bias, dtype=torch.float32), reference(c, "real", relu, bias)
    return tuple(U.rel_err(r32[n], r64[n]) for n in NAMES)


def e32(case, relu, bias=True):
    """torch's own float32 error on the CPU per tensor: rel_err(reference(float32), reference(float64)), real inputs."""
    return dict(zip(NAMES, _e32(case.name, bool(relu), bool(bias))))


def bounds(case, relu, bias=True):
    """What a kernel may be off the float64 reference by on the real inputs: the tolerance the project already holds for this kernel
    plus twice the float32 reference's own error (the kernel sums in another order, so it may err as much again)."""
    return {n: TOL[n] + 2.0 * e for n, e in e32(case, relu, bias).items()}


def bits(t):
    """The float32 bit patterns of a float32 tensor, on the CPU."""
    return t.detach().cpu().contiguous().view(torch.int32)


def exact_bits(ref64):
    """The float32 bits of an exact-pass reference tensor.  Its entries are integers below 2^24, so the cast is exact; `+ 0.0` makes
    every zero +0.0, which is what a sum that starts at +0.0 gives (the kernels' accumulators do, and x + -0.0 keeps +0.0)."""
    f = ref64.float()
    assert torch.equal(f.double(), ref64)
    return bits(f + 0.0)


def judge(case, kind, relu, got, bias=True, what="", log=None):
    """`got`: {y, dx, dw, db} float32 CPU tensors of one forward + backward (a missing or None entry is not judged).  Exact pass: the
    reference's bits.  Real pass: within bounds() of the float64 reference taken under the kernel's own ReLU mask, and every mask entry
    that differs from the float64 pre-activation's sign is a tie.  Returns (errors, flips); `log` gets one line."""
    mask, flips = None, 0
    if relu:
        mask = got["y"] > 0
        flips = U.relu_flips(mask, preact(case, kind, bias), f"{case.name} {what}")
        if kind == "exact":
            assert flips == 0, f"{case.name} {what}: integer pre-activations have no ties"
    ref = reference(case, kind, relu, bias, mask=mask)
    present = [n for n in NAMES if got.get(n) is not None]
    finite = {n: bool(torch.isfinite(got[n]).all()) for n in present}
    err = {n: U.rel_err(got[n], ref[n]) if finite[n] else float("inf") for n in present}
    bound = {n: 0.0 for n in NAMES} if kind == "exact" else bounds(case, relu, bias)
    if log is not None:
        log(f"conv_envelope {case.name} {kind} relu={int(bool(relu))} {what}: "
            + " ".join(f"{n}={err[n]:.2e}/{bound[n]:.2e}" for n in present) + f" flips={flips}")
    assert all(finite.values()), (case.name, what, finite)
    for n in present:
        if kind == "exact":
            bad = bits(got[n]).reshape(-1) != exact_bits(ref[n]).reshape(-1)
            assert not bool(bad.any()), (f"{case.name} {kind} relu={int(bool(relu))} {what}: {n} differs from the exact result in {int(bad.sum())} of "
                                         f"{bad.numel()} elements, first at flat index {int(bad.nonzero()[0])}")
        else:
            assert err[n] <= bound[n], f"{case.name} {kind} relu={int(bool(relu))} {what}: {n} rel err {err[n]:.3e} > {bound[n]:.3e}"
    return err, flips


def run(lib, case, kind, relu, device="cpu", bias=True, need_dx=True):
    """conv2d_fwd, then conv2d_bwd on the forward's own y (what mlhot.ops.Conv2dFunction does) through `lib`'s binding -> {y, dx, dw,
    db} on the CPU; db is None without a bias, dx None when it is not asked for."""
    i = inputs(case.name, kind)
    x, w, b, dy = (t.to(device) for t in (i.x, i.w, i.b, i.dy))
    y = lib.conv2d_fwd(x, w, b if bias else None, case.s, case.p, relu)
    dx, dw, db = lib.conv2d_bwd(x, w, y, dy, case.s, case.p, relu, need_dx=need_dx, has_bias=bias)
    return {n: (None if t is None else t.cpu()) for n, t in zip(NAMES, (y, dx, dw, db))}


# shapes all three entry points refuse (MLHOT_ERR_ARG; 0 scratch bytes): a non-positive extent, or a kernel larger than the padded
# image in either direction (HO or WO would be <= 0)
REFUSED = [
    ((0, 2, 6, 6, 3, 3, 1, 1), "N = 0"), ((1, 0, 6, 6, 3, 3, 1, 1), "Cin = 0"), ((1, 2, 6, 6, 0, 3, 1, 1), "Cout = 0"),
    ((1, 2, 6, 6, 3, 0, 1, 1), "k = 0"), ((1, 2, 6, 6, 3, 3, 0, 1), "stride = 0"), ((1, 2, 6, 6, 3, 3, 1, -1), "pad < 0"),
    ((1, 2, 2, 6, 3, 3, 1, 0), "H + 2 pad < k"), ((1, 2, 6, 2, 3, 3, 1, 0), "W + 2 pad < k"), ((1, 2, 2, 9, 3, 5, 2, 1), "H + 2 pad = k - 1"),
    ((1, 2, 9, 1, 3, 4, 3, 1), "W + 2 pad = k - 1"), ((1, 2, 1, 1, 3, 5, 1, 1), "both"),
]
# ... and their nearest neighbours, which all three accept: the kernel exactly fills the padded image (HO = 1 or WO = 1)
ACCEPTED_EDGE = [(1, 2, 3, 6, 3, 3, 1, 0), (1, 2, 6, 3, 3, 3, 1, 0), (1, 2, 3, 9, 3, 5, 2, 1), (1, 2, 9, 2, 3, 4, 3, 1)]


def abi_call(lib, shape, device="cpu", with_dw=True):
    """mlhot_conv2d_bwd_scratch_bytes, mlhot_conv2d_fwd and mlhot_conv2d_bwd on integer inputs and sentinel-filled outputs of the sizes
    the nearest valid shape would need -> (scratch bytes, rc_fwd, rc_bwd, outputs, inputs).  with_dw False: dw is NULL."""
    N, Cin, H, W, Cout, k, s, p = shape
    n, ci, co, kk = max(N, 1), max(Cin, 1), max(Cout, 1), max(k, 1)
    ho, wo = (max((d + 2 * p - k) // max(s, 1) + 1, 1) for d in (H, W))
    g = torch.Generator().manual_seed(sum(shape) + 99)
    ins = [torch.randint(-3, 4, sh, generator=g).float().to(device) for sh in ((n, ci, H, W), (co, ci, kk, kk), (co,), (n, co, ho, wo))]
    x, w, b, dy = ins
    outs = dict(y=torch.full_like(dy, -777.25), dx=torch.full_like(x, -777.25), dw=torch.full_like(w, -777.25), db=torch.full_like(b, -777.25))
    sb = lib.c.mlhot_conv2d_bwd_scratch_bytes(*shape)
    scratch = torch.zeros(max(sb, 4 * co * (ci * kk * kk + 1) + 256), dtype=torch.uint8, device=device)
    P = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream) if device != "cpu" else None
    rc_f = lib.c.mlhot_conv2d_fwd(P(x), P(w), P(b), P(outs["y"]), *shape, 0, stream)
    rc_b = lib.c.mlhot_conv2d_bwd(P(x), P(w), P(outs["y"]), P(dy), *shape, 0, P(outs["dx"]), P(outs["dw"]) if with_dw else None, P(outs["db"]), P(scratch),
                                  scratch.numel(), stream)
    if device != "cpu":
        torch.cuda.synchronize()
    return sb, rc_f, rc_b, {n: t.cpu() for n, t in outs.items()}, [t.cpu() for t in ins]


def check_refusals(lib, device):
    """All three entries refuse REFUSED (MLHOT_ERR_ARG named by mlhot_last_error, 0 scratch bytes, no output written), the backward
    refuses db without dw, and all three take
    ACCEPTED_EDGE, where the kernel exactly fills the padded image, with the exact result."""
    for shape, why in REFUSED:
        sb, rc_f, rc_b, outs, _ = abi_call(lib, shape, device)
        assert sb == 0, (why, sb)
        assert rc_f == ERR_ARG, (why, rc_f)
        assert rc_b == ERR_ARG and b"conv2d_bwd: bad argument" in lib.c.mlhot_last_error(), (why, rc_b)
        assert all(bool((t == -777.25).all()) for t in outs.values()), f"{why}: a refused call wrote something"
    # db is a column of the weight-gradient problem: asked for without dw it would stay unwritten, so that is refused as well
    sb, rc_f, rc_b, outs, _ = abi_call(lib, ACCEPTED_EDGE[0], device, with_dw=False)
    assert (rc_f, rc_b) == (0, ERR_ARG) and b"needs dw" in lib.c.mlhot_last_error()
    assert all(bool((outs[n] == -777.25).all()) for n in ("dx", "dw", "db"))
    for shape in ACCEPTED_EDGE:
        sb, rc_f, rc_b, outs, (x, w, b, dy) = abi_call(lib, shape, device)
        assert sb > 0 and (rc_f, rc_b) == (0, 0), (shape, sb, rc_f, rc_b)
        xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
        yr = F.conv2d(xr, wr, br, stride=shape[6], padding=shape[7])
        yr.backward(dy.double())
        for n, ref in (("y", yr.detach()), ("dx", xr.grad), ("dw", wr.grad), ("db", br.grad)):
            assert torch.equal(bits(outs[n]), exact_bits(ref)), (shape, n)
