"""Shared by tests/test_linear_abi_cpu.py and tests/test_linear_abi_gpu.py: the case table of mlhot_linear_fwd / mlhot_linear_bwd's C
ABI (every stride, offset, flag and null pointer the header allows), a ctypes caller that runs a case on windows of larger,
sentinel-filled buffers, and the float64 reference.

Routes (csrc/mlhot.hip mlhot_linear_fwd / _bwd, csrc/np_vanilla.h lin_fwd / lin_dgrad / lin_wgrad, csrc/igemm.h run_igemm_auto; the host
flavour of the library takes the generic chain on every leg):
  forward   skinny (linear_skinny.h) when M <= 512, K % 4 == 0, x and w 16-byte aligned, ldx % 4 == 0; else the generic GEMM
  backward  ONE combined skinny launch when dw and dx, M <= 512, N % 4 == 0, dy aligned with lddy % 4 == 0, and y aligned with
            ldy % 4 == 0 unless act is none; else separate launches:
              weight gradient  skinny when M <= 512 (no alignment condition), else generic
              data gradient    skinny under the combined launch's conditions on N, dy and y, else generic
  generic   16 x 64 tiles when ceil(M' / 64) * ceil(N' / 64) < 128, else 64 x 64 (the weight gradient's problem is M' = N, N' = K + 1)
"""
import ctypes as C
import types

import torch

from tests import util as U

ACTS = ["none", "relu", "tanh"]
ACT_CODE = {"none": 0, "relu": 1, "tanh": 2}
SENTINEL = -777.25            # finite, exactly representable, far from every value a case computes
PAD = 5                       # spare columns behind every row of a buffer (and room for the element offsets)
MAX_ROWS = 512                # sk::MAX_ROWS


def case(name, M, K, N, **kw):
    """One call pair.  ldx / ldy / lddy / lddx: row strides in floats (default: the natural K or N); off: element offsets of the
    operands' first elements inside their buffers {"x", "w", "y", "dy", "dx"} (1 float = not 16-byte aligned); accumulate; b, dx, dw,
    db: False = pass NULL."""
    c = dict(name=name, M=M, K=K, N=N, ldx=K, ldy=N, lddy=N, lddx=K, off={}, accumulate=0, b=True, dx=True, dw=True, db=True)
    assert set(kw) <= set(c), kw
    c.update(kw)
    c["off"] = {**dict(x=0, w=0, y=0, dy=0, dx=0), **c["off"]}
    return types.SimpleNamespace(**c)


def _cases():
    out = []
    # skinny row tiles of 32: forward skinny, backward combined
    out += [case(f"rows_M{M}", M, 64, 48) for M in (1, 31, 32, 33)]
    # sk::MAX_ROWS: 511 / 512 skinny + combined, 513 generic on every leg
    out += [case(f"maxrows_M{M}", M, 36, 20) for M in (511, 512, 513)]
    for M in (37, 512):
        # x / w off by one float: forward generic (backward still combined - it has no condition on x or w)
        out.append(case(f"xoff_M{M}", M, 64, 48, off=dict(x=1)))
        out.append(case(f"woff_M{M}", M, 64, 48, off=dict(w=1)))
        # dy off by one float: forward skinny; backward separate, weight gradient skinny, data gradient generic
        out.append(case(f"dyoff_M{M}", M, 64, 48, off=dict(dy=1)))
    # y off by one float: backward combined for act none, separate (data gradient generic) for relu / tanh
    out.append(case("yoff_M37", 37, 64, 48, off=dict(y=1)))
    # K % 4 != 0, N % 4 != 0: forward generic; backward separate, weight gradient skinny, data gradient generic
    out += [case(f"odd_K{K}_N{N}", 65, K, N) for K in (17, 18, 19) for N in (130, 131)]
    # run_igemm_auto's tile variants, M = 513 (9 row tiles): forward 9 * 14 = 126 -> 16 x 64 tiles, 9 * 15 = 135 -> 64 x 64
    out += [case("tiles_fwd_126", 513, 8, 896), case("tiles_fwd_135", 513, 8, 897)]
    # ... and the weight gradient's problem (M' = N = 1024: 16 tiles; N' = K + 1): 16 * 7 = 112 -> 16 x 64, 16 * 8 = 128 -> 64 x 64
    out += [case("tiles_wgrad_112", 513, 447, 1024), case("tiles_wgrad_128", 513, 448, 1024)]
    # strides, multiples of 4 (skinny / combined) ...
    out.append(case("strides_x4", 40, 32, 24, ldx=32 + 4, ldy=24 + 8, lddy=24 + 4, lddx=32 + 12))
    # ... and odd ones: forward generic (ldx), backward separate with the generic data gradient (lddy)
    out.append(case("strides_odd", 40, 32, 24, ldx=32 + 1, ldy=24 + 3, lddy=24 + 1, lddx=32 + 3))
    # x = columns [8, 40) of a [40, 64] buffer, dx written into the same window of another: skinny / combined
    out.append(case("colwindow", 40, 32, 24, ldx=64, lddx=64, off=dict(x=8, dx=8)))
    # accumulate = 1 on each data-gradient route: combined (7, 40), skinny data gradient alone (dw = NULL), generic (513, and dy offset)
    out += [case(f"acc_M{M}", M, 32, 24, accumulate=1) for M in (7, 40, 513)]
    out += [case(f"acc_dxonly_M{M}", M, 32, 24, accumulate=1, dw=False, db=False) for M in (7, 40)]
    out.append(case("acc_dyoff_M40", 40, 32, 24, accumulate=1, off=dict(dy=1)))
    # one gradient only: both fall out of the combined launch
    for M in (40, 513):
        out.append(case(f"dxonly_M{M}", M, 32, 24, dw=False, db=False))
        out.append(case(f"dwonly_M{M}", M, 32, 24, dx=False))
    # nullable bias / bias gradient (include/mlhot.h: "b may be NULL", "dx/dw/db may be NULL")
    out.append(case("nob_M40", 40, 32, 24, b=False))
    out.append(case("nodb_M40", 40, 32, 24, db=False))
    out.append(case("nob_nodb_M513", 513, 32, 24, b=False, db=False))
    # no rows: N = 24 meets the combined launch's conditions, N = 22 does not
    out += [case(f"empty_N{N}", 0, 32, N) for N in (24, 22)]
    # long reduction, few rows
    out.append(case("longK", 16, 4096, 64, accumulate=1, lddx=4096 + 4))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
PAIR_SHAPES = [(37, 64, 48), (512, 64, 48)]          # skinny vs generic on the same data


def _window_index(off, rows, cols, ld):
    return (off + torch.arange(rows).unsqueeze(1) * ld + torch.arange(cols).unsqueeze(0)).reshape(-1)


class _Operand:
    """A [rows, cols] window (row stride ld, first element at `off`) of a sentinel-filled flat buffer of (buf_rows) x (ld + PAD)."""

    def __init__(self, rows, cols, ld, off, buf_rows, device, values=None):
        assert ld >= cols and off >= 0
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.buf = torch.full((buf_rows * (ld + PAD),), SENTINEL, dtype=torch.float32)
        self.idx = _window_index(off, rows, cols, ld)
        assert rows == 0 or int(self.idx[-1]) < self.buf.numel(), "window leaves its buffer"
        if values is not None:
            self.buf[self.idx] = values.reshape(-1).float()
        self.buf = self.buf.to(device)
        self.before = self.buf.clone()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.off)

    def aligned4(self):
        return (self.buf.data_ptr() + 4 * self.off) % 16 == 0 and self.ld % 4 == 0

    def window(self):
        return self.buf.cpu()[self.idx].reshape(self.rows, self.cols)

    def outside_unchanged(self):
        """Nothing but the logical window changed: padding columns, rows >= rows, the elements in front of the offset."""
        now, was = self.buf.cpu(), self.before.cpu()
        keep = torch.ones(now.numel(), dtype=torch.bool)
        keep[self.idx] = False
        return bool(torch.equal(now[keep], was[keep])) and int(keep.sum()) >= self.ld + PAD      # at least one spare row is watched

    def unchanged(self):
        return bool(torch.equal(self.buf, self.before))


def make_data(M, K, N, seed=0):
    """The values of a case: a function of the shape alone, so that two cases of one shape (aligned / offset) see the same data."""
    g = torch.Generator().manual_seed(100003 * seed + 7919 * M + 101 * K + N)
    return types.SimpleNamespace(
        x=torch.randn(M, K, generator=g), w=torch.randn(N, K, generator=g) / K ** 0.5, b=0.5 * torch.randn(N, generator=g),
        dy=torch.randn(M, N, generator=g), dx0=torch.randn(M, K, generator=g))


def expected_bwd_labels(c, act, dy_aligned, y_aligned, device_build=True):
    """The launch labels mlhot_prof_end reports for the backward of case `c` on the device build (docstring above)."""
    d_ok = c.M <= MAX_ROWS and c.N % 4 == 0 and dy_aligned and (act == "none" or y_aligned)
    if c.dw and c.dx and d_ok:
        return ["linear_bwd"]                                   # the combined launch (at M == 0: its weight-gradient half alone)
    labels = ["linear_bwd.w"] if c.dw else []                   # at M == 0 the launch still runs: it writes the zeros
    if c.dx and c.M > 0:
        labels.append("linear_bwd.x")
    return labels


def call_linear(lib, c, act, device="cpu", data=None, profile=False):
    """mlhot_linear_fwd, then mlhot_linear_bwd on the forward's own y, through ctypes.  Returns a namespace: y, dx, dw, db (CPU
    tensors or None), rc_fwd / rc_bwd, data (the inputs), dx0 (what dx held before an accumulating call), untouched (bool: nothing
    outside the logical windows of y, dx, dw, db changed and no input changed), labels (profile=True: the backward's launches) and
    the alignment facts expected_bwd_labels needs."""
    d = data or make_data(c.M, c.K, c.N)
    M, K, N = c.M, c.K, c.N
    x = _Operand(M, K, c.ldx, c.off["x"], M + 2, device, d.x)
    w = _Operand(N, K, K, c.off["w"], N + 2, device, d.w)
    b = _Operand(1, N, N, 0, 2, device, d.b)
    y = _Operand(M, N, c.ldy, c.off["y"], M + 2, device)
    dy = _Operand(M, N, c.lddy, c.off["dy"], M + 2, device, d.dy)
    dx = _Operand(M, K, c.lddx, c.off["dx"], M + 2, device, d.dx0 if c.accumulate else None)
    dw = _Operand(N, K, K, 0, N + 2, device)
    db = _Operand(1, N, N, 0, 2, device)
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream) if str(device).startswith("cuda") else None
    r = types.SimpleNamespace(data=d, dx0=d.dx0 if c.accumulate else None, labels=None)
    r.rc_fwd = lib.c.mlhot_linear_fwd(x.ptr(), c.ldx, w.ptr(), b.ptr() if c.b else None, y.ptr(), c.ldy, M, K, N, ACT_CODE[act], stream)
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    r.y = y.window()
    y_now = y.buf.clone()
    if profile:
        lib.prof_begin(64)
    r.rc_bwd = lib.c.mlhot_linear_bwd(x.ptr(), c.ldx, w.ptr(), y.ptr(), c.ldy, dy.ptr(), c.lddy, M, K, N, ACT_CODE[act],
                                      dx.ptr() if c.dx else None, c.lddx, c.accumulate, dw.ptr() if c.dw else None,
                                      db.ptr() if c.db else None, None, 0, stream)
    if profile:
        r.labels = [label for label, _ in lib.prof_end()]
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    r.dx = dx.window() if c.dx else None
    r.dw = dw.window() if c.dw else None
    r.db = db.window().reshape(-1) if c.db else None
    r.dy_aligned, r.y_aligned = dy.aligned4(), y.aligned4()
    inputs_kept = x.unchanged() and w.unchanged() and b.unchanged() and dy.unchanged() and bool(torch.equal(y.buf, y_now))
    outputs = [y.outside_unchanged(),
               dx.outside_unchanged() if c.dx else dx.unchanged(),
               dw.outside_unchanged() if c.dw else dw.unchanged(),
               db.outside_unchanged() if c.db else db.unchanged()]
    r.untouched = inputs_kept and all(outputs)
    return r


def _act64(act, pre):
    return torch.relu(pre) if act == "relu" else (torch.tanh(pre) if act == "tanh" else pre)


def reference(c, act, data, y_kernel, dx0=None):
    """float64 on the CPU: y = act(x w^T + b) and autograd's dx, dw, db under the upstream dy.  The ReLU mask is the KERNEL's (y > 0 of
    the y the backward was handed - the ABI differentiates through that y); with accumulate, dx0 is added."""
    x = data.x.double().requires_grad_(True)
    w = data.w.double().requires_grad_(True)
    b = (data.b.double() if c.b else torch.zeros(c.N, dtype=torch.float64)).requires_grad_(True)
    pre = x @ w.t() + b
    y = _act64(act, pre).detach()
    out = pre * (y_kernel.double() > 0).double() if act == "relu" else _act64(act, pre)
    out.backward(data.dy.double())
    dx = x.grad + (dx0.double() if dx0 is not None else 0.0)
    return types.SimpleNamespace(y=y, dx=dx, dw=w.grad, db=b.grad)


def edge_errors(got, want):
    """(whole tensor, last row alone, last column alone): rel_err scales by the tensor's largest entry, under which a wrong last
    partial tile row / column of small values could hide - those two are compared again at their own scale."""
    errs = [U.rel_err(got, want)]
    if got.dim() == 2 and got.shape[0] > 0:
        errs += [U.rel_err(got[-1], want[-1]), U.rel_err(got[:, -1], want[:, -1])]
    return errs


def check_case(lib, c, act, device, profile=False):
    """Run case `c`, assert everything the issue asks of it, return {output: worst error}."""
    r = call_linear(lib, c, act, device, profile=profile)
    assert r.rc_fwd == 0 and r.rc_bwd == 0, (r.rc_fwd, r.rc_bwd, lib.c.mlhot_last_error().decode())
    assert r.untouched, f"{c.name}/{act}: an element outside the logical windows (or an input) changed"
    if profile:
        want_labels = expected_bwd_labels(c, act, r.dy_aligned, r.y_aligned)
        assert sorted(r.labels) == sorted(want_labels), f"{c.name}/{act}: launches {r.labels}, expected {want_labels}"
    ref = reference(c, act, r.data, r.y, r.dx0)
    worst = {}
    for name in ("y", "dx", "dw", "db"):
        got = getattr(r, name)
        if got is None or got.numel() == 0:      # a NULL output, or the empty y / dx of M == 0 (their buffers are checked above)
            continue
        assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any()), f"{c.name}/{act}: {name} has unwritten elements"
        if c.M == 0 and name in ("dw", "db"):
            assert int(torch.count_nonzero(got)) == 0, f"{c.name}/{act}: {name} of an empty batch is not zero"
        errs = edge_errors(got, getattr(ref, name))
        worst[name] = max(errs)
        print(f"linear_abi {c.name}/{act} {name}: whole {errs[0]:.2e}" + (f" last row {errs[1]:.2e} last col {errs[2]:.2e}" if len(errs) > 1 else ""))
        assert worst[name] <= U.RTOL, f"{c.name}/{act}: {name} rel err {errs} > {U.RTOL}"
    return worst


def check_pair(lib, shape, act, device):
    """The same data through the aligned call (device: skinny forward, combined backward) and through a call with x, w, dy and y off
    by one float (device: generic on every leg but the weight gradient): the two agree within RTOL of the reference's scale."""
    M, K, N = shape
    data = make_data(M, K, N, seed=1)
    a = call_linear(lib, case("pair_aligned", M, K, N), act, device, data=data)
    o = call_linear(lib, case("pair_offset", M, K, N, off=dict(x=1, w=1, dy=1, y=1, dx=1)), act, device, data=data)
    assert a.rc_fwd == 0 and a.rc_bwd == 0 and o.rc_fwd == 0 and o.rc_bwd == 0
    assert a.untouched and o.untouched
    ref = reference(case("pair_ref", M, K, N), act, data, a.y)
    worst = {}
    for name in ("y", "dx", "dw", "db"):
        scale = getattr(ref, name).abs().max().item()
        worst[name] = (getattr(a, name).double() - getattr(o, name).double()).abs().max().item() / scale
        print(f"linear_abi pair {M}x{K}x{N}/{act} {name}: aligned vs offset {worst[name]:.2e}")
        assert worst[name] <= U.RTOL, f"pair {shape}/{act}: {name} differs by {worst[name]:.2e} of the reference's scale"
    return worst
