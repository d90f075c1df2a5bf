"""Shared by tests/test_job_tables_cpu.py and tests/test_job_tables_gpu.py: the case table of csrc/mlp_chain.h's four C entries
(mlhot_mlp_chain_fwd / _bwd, mlhot_linear_multi_fwd / _bwd), a ctypes caller that runs a case on windows of larger, sentinel-filled
buffers (tests/linear_abi.py's _Operand), and the float64 reference (explicit torch.cat, per-layer activations, autograd in double).

What the cases reach (read from csrc/mlp_chain.h and csrc/linear_skinny.h):
  chain_fwd_kernel    a workgroup = 16 rows, 8 waves; wave wv owns the 16-column tiles wv and wv + 8 of a layer (N <= 128: the first
                      alone; N % 16 != 0: a partial last tile; a wave without a tile still reaches the barrier); the weights come in
                      passes of 256 k with the last k group clamped to K - 4
  chain_dgrad_kernel  N % 16 == 0: MFMA passes of 16 column tiles of K (K = 260: 17 tiles, the second pass is wave 0's alone); any other
                      N: the scalar "narrow" path; the G stage holds 8 elements per thread at N = 256
  chain_backward      one multi_wgrad job per layer and one more per side: four layers with four sides fill MAXJ = 8
  job tables          every kernel finds its job with `while (blockIdx.x >= j[ji + 1].first)`: jobs of different shapes, 8 jobs, jobs
                      without rows (the forward drops them; the backward keeps their weight-gradient blocks, which write the zeros)
  two-source bodies   fwd_body picks the source per float4 group, wgrad_body per element of a 64-column tile, dgrad_body routes groups of
                      4 columns to dx or dx2: K1 in {4, 20, 60, 68} x K2 in {4, 12} puts the seam inside a 16-deep chunk and a 64-wide tile
Every layer of a chain has a width of its own, so that a swapped buffer, offset or stride cannot cancel.
"""
import ctypes as C
import types
import zlib

import torch

from mlhot.binding import ChainGrads, ChainLayer, LinearJob
from tests import util as U
from tests.linear_abi import ACT_CODE, PAD, SENTINEL, _Operand

MAX_ROWS, MAXL, MAXJ, KMAX, NMAX = 512, 4, 8, 512, 256
RELU_MARGIN = 1e-5            # no ReLU pre-activation of the float64 reference lies within this share of its tensor's scale from zero


def _up4(n):
    return (n + 3) // 4 * 4


def _cdiv(a, b):
    return (a + b - 1) // b


def _odd(n):
    """the smallest odd stride larger than n"""
    return n + 1 + n % 2


# ---- the chain's cases ---------------------------------------------------------------------------------------------------------------
def layer(N, act="none", side_w=0, side_first=0, b=True, dside=True, dside_acc=0, K=None):
    """One layer.  b = False: b and db NULL; dside = False: the side's gradient is not wanted; K: the struct's K when it is NOT
    side_w + the previous width (refusals)."""
    return types.SimpleNamespace(N=N, act=act, side_w=side_w, side_first=side_first, b=b, dside=dside, dside_acc=dside_acc, K_arg=K)


def chain(name, M, K0, layers, dx0=True, dx0_acc=0, tight=False, ld=None, off=None, seed=0):
    """x0 [M, K0] and the layers.  Row strides (floats): every one larger than its width unless tight - multiples of 4 where the header
    wants them (x0, side, g), odd where it does not (y, dy, dx0, dside); x0 is a column window (4 floats in) of a wider buffer.
    ld / off override single strides / element offsets: keys "x0", "dy", "dx0", ("y", k), ("side", k), ("g", k), ("dside", k), ("w", k)."""
    c = types.SimpleNamespace(name=name, M=M, K0=K0, layers=layers, dx0=dx0, dx0_acc=dx0_acc, seed=seed, ld={}, off={})
    prev = K0
    for k, l in enumerate(layers):
        l.pw = prev
        l.K = l.K_arg if l.K_arg is not None else prev + l.side_w
        l.wK = max(l.K, 1)
        p = 0 if tight else 1
        c.ld.update({("y", k): _odd(l.N) if p else l.N, ("side", k): l.side_w + 4 * p, ("g", k): _up4(l.N) + 4 * p,
                     ("dside", k): _odd(l.side_w) if p else l.side_w})
        c.off.update({("w", k): 0, ("side", k): 0})
        prev = l.N
    p = 0 if tight else 1
    c.ld.update({"x0": _up4(K0) + 8 * p, "dy": _odd(prev) if p else prev, "dx0": _odd(K0) if p else K0})
    c.off["x0"] = 4 * p
    c.ld.update(ld or {})
    c.off.update(off or {})
    return c


def _chain_cases():
    L = layer
    out = [
        # one layer: the row edges of the 16-row workgroup, every last-layer N, every K of the weight passes
        chain("one_M1_K4_N1", 1, 4, [L(1)]),
        chain("one_M15_K8_N2_tanh", 15, 8, [L(2, "tanh")]),
        chain("one_M16_K252_N3_relu", 16, 252, [L(3, "relu")]),
        chain("one_M17_K256_N5", 17, 256, [L(5)]),
        chain("one_M33_K260_N17_relu", 33, 260, [L(17, "relu")]),
        chain("one_M33_K512_N255_tanh", 33, 512, [L(255, "tanh")]),
        # N = 256: both tiles of every wave, the G stage's 8 elements per thread; K = 260: 17 column tiles, the second MFMA pass is wave 0's
        chain("one_M17_K260_N256_relu", 17, 260, [L(256, "relu")]),
        chain("one_M512_K8_N4", 512, 8, [L(4)]),
        chain("one_M16_K512_N144_tanh", 16, 512, [L(144, "tanh")]),         # MFMA data gradient over exactly two full passes
        # inner widths: 4 (the next K = 4), 12 / 20 (narrow data gradient), 128 (tiles 0 .. 7 alone), 132 / 144 (a ninth tile, partial / whole), 256
        chain("two_inner4", 17, 8, [L(4, "relu"), L(2)]),
        chain("three_inner12_20", 33, 8, [L(12, "tanh"), L(20, "relu"), L(3, "tanh")]),
        chain("four_inner128_132_144", 17, 12, [L(128, "relu"), L(132, "tanh"), L(144), L(5, "relu")]),
        chain("two_inner256", 16, 252, [L(256, "tanh"), L(1, "relu")]),
        chain("four_M512", 512, 4, [L(8, "relu"), L(12), L(16, "tanh"), L(3)]),
        # a side input at every layer position, in front and behind; side_w 4, 12, 256
        chain("side0_first_w4", 17, 8, [L(12, "relu", 4, 1), L(2)]),
        chain("side0_behind_w12", 17, 8, [L(16, "tanh", 12, 0), L(3)]),
        chain("side1_first_w256", 33, 8, [L(4, "relu"), L(16, "none", 256, 1), L(5, "tanh")]),      # K = 260 on the MFMA path, routed to two tensors
        chain("side1_behind_w4", 17, 8, [L(12, "tanh"), L(20, "relu", 4, 0), L(3)]),
        chain("side2_first_w12", 17, 8, [L(4), L(12, "relu"), L(3, "tanh", 12, 1)]),
        chain("side2_behind_w256", 15, 4, [L(8, "relu"), L(4, "tanh"), L(17, "none", 256, 0)]),
        chain("side3_first_w4", 17, 4, [L(8, "tanh"), L(12), L(20, "relu"), L(2, "none", 4, 1)]),
        chain("side3_behind_w12", 17, 4, [L(8), L(12, "relu"), L(20, "tanh"), L(5, "relu", 12, 0)]),
        # four layers, four sides: the weight-gradient table holds MAXJ = 8 jobs
        chain("four_sides", 17, 4, [L(8, "relu", 4, 1), L(12, "tanh", 12, 0), L(16, "relu", 4, 0), L(5, "none", 12, 1)]),
        # no side and dx0 = NULL: the walk ends after layer 0's G stage
        chain("noside_nodx0", 17, 8, [L(12, "relu"), L(3, "tanh")], dx0=False),
        chain("nob_nodb", 17, 8, [L(12, "relu", 4, 1, b=False), L(5, "tanh", b=False)]),
        chain("nodside", 17, 8, [L(12, "relu", 4, 0, dside=False), L(16, "tanh", 12, 1, dside=False), L(3)]),
        chain("nodside_nodx0_one", 17, 8, [L(16, "relu", 4, 1, dside=False)], dx0=False, seed=1),
        # accumulate onto non-zero prior contents: narrow path, MFMA path
        chain("acc_narrow", 17, 8, [L(12, "relu", 4, 1, dside_acc=1), L(5, "tanh", 12, 0, dside_acc=1)], dx0_acc=1),
        chain("acc_mfma", 33, 8, [L(16, "tanh", 12, 0, dside_acc=1), L(32, "relu", 4, 1, dside_acc=1)], dx0_acc=1),
        # ... and over more than one MFMA pass (17 column tiles): a tile computed twice would be added twice
        chain("acc_mfma_K260", 17, 260, [L(32, "tanh")], dx0_acc=1),
        chain("acc_mfma_side256", 33, 8, [L(4, "relu"), L(16, "tanh", 256, 1, dside_acc=1)]),
        chain("acc_dx0_only", 17, 8, [L(12, "relu", 4, 1), L(5)], dx0_acc=1),
        chain("tight", 17, 8, [L(12, "relu", 4, 1), L(5, "tanh")], tight=True),
        # no rows: the forward launches nothing, the backward its weight-gradient table alone (dw, db = zeros)
        chain("M0", 0, 8, [L(12, "relu", 4, 1), L(16, "tanh"), L(5, "none", 12, 0)]),
        chain("M0_nob", 0, 8, [L(3, "relu", b=False)]),
    ]
    return out


CHAIN_CASES = _chain_cases()


def _chain_refusals():
    """(case, stage): stage "fwd" = both entries refuse, "bwd" = the forward runs and the backward refuses."""
    L = layer
    return [
        (chain("ref_M513", 513, 8, [L(4)]), "fwd"),
        (chain("ref_5layers", 17, 8, [L(4), L(8), L(12), L(16), L(3)]), "fwd"),
        (chain("ref_K6", 17, 6, [L(4)]), "fwd"),
        (chain("ref_K516", 17, 516, [L(4)]), "fwd"),
        (chain("ref_N257", 17, 8, [L(257)]), "fwd"),
        (chain("ref_inner_N6", 17, 8, [L(6), L(3, K=8)]), "fwd"),
        (chain("ref_K_mismatch", 17, 8, [L(12), L(3, K=16)]), "fwd"),
        (chain("ref_ldy_short", 17, 8, [L(12), L(5)], ld={("y", 1): 4}), "fwd"),
        (chain("ref_x0_unaligned", 17, 8, [L(4)], off={"x0": 1}), "fwd"),
        (chain("ref_w_unaligned", 17, 8, [L(4)], off={("w", 0): 1}), "fwd"),
        (chain("ref_side_unaligned", 17, 8, [L(4, "none", 4, 1)], off={("side", 0): 1}), "fwd"),
        (chain("ref_side_ld6", 17, 8, [L(4, "none", 4, 1)], ld={("side", 0): 6}), "fwd"),
        (chain("ref_ldg6", 17, 8, [L(4)], ld={("g", 0): 6}), "bwd"),
        (chain("ref_ldg_short", 17, 8, [L(12)], ld={("g", 0): 8}), "bwd"),
        (chain("ref_lddy_short", 17, 8, [L(12)], ld={"dy": 8}), "bwd"),
    ]


CHAIN_REFUSALS = _chain_refusals()


def chain_refused(c, bwd):
    """check_chain + chain_backward's argument checks, restated on the case (buffers start 16-byte aligned): the reason, or None."""
    a16 = lambda key: c.off[key] % 4 == 0
    if not 1 <= len(c.layers) <= MAXL or not 0 <= c.M <= MAX_ROWS or not a16("x0") or c.ld["x0"] % 4:
        return "bad argument"
    prev = None
    for k, l in enumerate(c.layers):
        pw = l.K - l.side_w
        if (l.K < 4 or l.K > KMAX or l.K % 4 or l.N < 1 or l.N > NMAX or l.side_w % 4 or pw < 4 or pw % 4 or not a16(("w", k)) or c.ld[("y", k)] < l.N
                or (l.side_w and (not a16(("side", k)) or c.ld[("side", k)] % 4))):
            return f"layer {k}"
        if k > 0 and pw != prev:
            return f"layer {k} width"
        if k == 0 and c.ld["x0"] < pw:
            return "x0 rows"
        if k + 1 < len(c.layers) and l.N % 4:
            return f"inner layer {k}"
        prev = l.N
    if bwd:
        if c.ld["dy"] < c.layers[-1].N:
            return "lddy"
        for k, l in enumerate(c.layers):
            if c.ld[("g", k)] < l.N or c.ld[("g", k)] % 4:
                return f"layer {k} g"
    return None


def chain_wgrad_jobs(c):
    """chain_backward's weight-gradient table: [(K columns, N)] - per layer the previous-layer columns, then the side's."""
    jobs = []
    for l in c.layers:
        jobs.append((l.K - l.side_w, l.N))
        if l.side_w:
            jobs.append((l.side_w, l.N))
    return jobs


def chain_blocks(c):
    """(chain_fwd / chain_dgrad workgroups, multi_wgrad blocks): 16 rows each; ceil(N / 16) * ceil(K / 64) per weight-gradient job."""
    return _cdiv(c.M, 16), sum(_cdiv(N, 16) * _cdiv(K, 64) for K, N in chain_wgrad_jobs(c))


def _gen(name, seed):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) + 7919 * seed)


def chain_data(c):
    g = _gen("chain/" + c.name, c.seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = types.SimpleNamespace(x0=r(c.M, c.K0), dy=r(c.M, c.layers[-1].N), dx0_prior=r(c.M, c.K0), w=[], b=[], side=[], dside_prior=[])
    for l in c.layers:
        d.w.append(r(l.N, l.wK) / l.wK ** 0.5)
        d.b.append(0.5 * r(l.N))
        d.side.append(r(c.M, l.side_w))
        d.dside_prior.append(r(c.M, l.side_w))
    return d


def act64(act, pre):
    return torch.relu(pre) if act == "relu" else (torch.tanh(pre) if act == "tanh" else pre)


def chain_reference(c, d):
    """float64: ys, pres (pre-activations), g (their gradients), dx0, dside, dw, db - the accumulate flags' prior contents added."""
    x0 = d.x0.double().requires_grad_(True)
    h, ys, pres, ws, bs, sides = x0, [], [], [], [], []
    for k, l in enumerate(c.layers):
        w = d.w[k].double().requires_grad_(True)
        b = d.b[k].double().requires_grad_(True) if l.b else None
        side = d.side[k].double().requires_grad_(True) if l.side_w else None
        inp = h if side is None else (torch.cat([side, h], -1) if l.side_first else torch.cat([h, side], -1))
        pre = inp @ w.t() + (b if b is not None else 0.0)
        pre.retain_grad()
        h = act64(l.act, pre)
        ys.append(h.detach()); pres.append(pre); ws.append(w); bs.append(b); sides.append(side)
    h.backward(d.dy.double())
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    ref = types.SimpleNamespace(y=ys, pre=[p.detach() for p in pres], g=[zero(p) for p in pres], dw=[zero(w) for w in ws],
                                db=[zero(b) if b is not None else None for b in bs], dside=[], dx0=None)
    for k, l in enumerate(c.layers):
        ref.dside.append(None if not (l.side_w and l.dside) else zero(sides[k]) + (d.dside_prior[k].double() if l.dside_acc else 0.0))
    if c.dx0:
        ref.dx0 = zero(x0) + (d.dx0_prior.double() if c.dx0_acc else 0.0)
    return ref


def relu_margin_ok(pre):
    """The ReLU condition on a case's inputs: no float64 pre-activation within RELU_MARGIN of the tensor's scale from zero."""
    return pre.numel() == 0 or float(pre.abs().min()) > RELU_MARGIN * float(pre.abs().max())


# ---- operands ------------------------------------------------------------------------------------------------------------------------
class _Bank:
    """The operands of one call: name -> (_Operand, role).  Roles: "in" (must not change), "out" (only its window may change), "null"
    (passed as NULL: must not change)."""

    def __init__(self, device):
        self.device, self.ops = device, {}

    def add(self, name, role, rows, cols, ld, off=0, values=None):
        if cols == 0:                    # an absent side / second source: no window, a buffer that must stay as it is
            rows, values = 0, None
        op = _Operand(rows, cols, max(ld, cols), off, rows + 2, self.device, values)
        op.ld = ld                       # a refusal may pass a stride shorter than the width: the buffer is laid out for the width
        self.ops[name] = (op, role)
        return op

    def addr(self, name):
        op, role = self.ops[name]
        return None if role == "null" else op.buf.data_ptr() + 4 * op.off

    def win(self, name):
        op, role = self.ops[name]
        return None if role == "null" else op.window()

    def snapshot(self):
        for op, _ in self.ops.values():
            op.before = op.buf.clone()

    def untouched(self, everything=False):
        """-> the names of the operands that changed where they must not ([] = all is well)."""
        bad = []
        for name, (op, role) in self.ops.items():
            ok = op.outside_unchanged() if (role == "out" and not everything) else op.unchanged()
            if not ok:
                bad.append(name)
        return bad


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream) if str(device).startswith("cuda") else None


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def _labelled(lib, fn):
    labels, rc = U.launch_labels(lib, fn)
    return rc, labels


# ---- the chain's caller --------------------------------------------------------------------------------------------------------------
def run_chain(lib, c, device, bwd=True):
    """mlhot_mlp_chain_fwd, then (bwd) mlhot_mlp_chain_bwd on the forward's own ys, on windows of sentinel-filled buffers.  Returns a
    namespace: rc_fwd / rc_bwd, labels_fwd / labels_bwd, y, g, dw, db, dside (lists), dx0, bad_fwd / bad_bwd (operands that changed
    where they must not), bank, data."""
    d = chain_data(c)
    n, M, B = len(c.layers), c.M, _Bank(device)
    B.add("x0", "in", M, c.K0, c.ld["x0"], c.off["x0"], d.x0)
    B.add("dy", "in", M, c.layers[-1].N, c.ld["dy"], 0, d.dy)
    B.add("dx0", "out" if c.dx0 else "null", M, c.K0, c.ld["dx0"], 0, d.dx0_prior if c.dx0_acc else None)
    for k, l in enumerate(c.layers):
        B.add(f"w{k}", "in", l.N, l.wK, l.wK, c.off[("w", k)], d.w[k])
        B.add(f"b{k}", "in" if l.b else "null", 1, l.N, l.N, 0, d.b[k])
        B.add(f"side{k}", "in", M, l.side_w, c.ld[("side", k)], c.off[("side", k)], d.side[k])
        B.add(f"y{k}", "out", M, l.N, c.ld[("y", k)])
        B.add(f"g{k}", "out", M, l.N, c.ld[("g", k)])
        B.add(f"dw{k}", "out", l.N, l.wK, l.wK)
        B.add(f"db{k}", "out" if l.b else "null", 1, l.N, l.N)
        B.add(f"dside{k}", "out" if (l.side_w and l.dside) else "null", M, l.side_w, c.ld[("dside", k)], 0, d.dside_prior[k] if l.dside_acc else None)
    B.snapshot()
    Ls, Gs = (ChainLayer * n)(), (ChainGrads * n)()
    for k, l in enumerate(c.layers):
        Ls[k] = ChainLayer(B.addr(f"w{k}"), B.addr(f"b{k}"), l.K, l.N, ACT_CODE[l.act], B.addr(f"side{k}") if l.side_w else None, l.side_w,
                           c.ld[("side", k)], l.side_first, B.addr(f"y{k}"), c.ld[("y", k)])
        Gs[k] = ChainGrads(B.addr(f"dw{k}"), B.addr(f"db{k}"), B.addr(f"g{k}"), c.ld[("g", k)], B.addr(f"dside{k}"), c.ld[("dside", k)], l.dside_acc)
    st = _stream(device)
    r = types.SimpleNamespace(data=d, bank=B, rc_bwd=None, labels_bwd=None, bad_bwd=None)
    r.rc_fwd, r.labels_fwd = _labelled(lib, lambda: lib.c.mlhot_mlp_chain_fwd(C.c_void_p(B.addr("x0")), c.ld["x0"], M, Ls, n, st))
    _sync(device)
    bwd_outs = {"dx0"} | {f"{p}{k}" for k in range(n) for p in ("g", "dw", "db", "dside")}
    r.bad_fwd = [name for name in B.untouched() if name not in bwd_outs] + [name for name in bwd_outs if not B.ops[name][0].unchanged()]
    r.y = [B.win(f"y{k}") for k in range(n)]
    if bwd:
        B.snapshot()                    # the ys are inputs from here on
        for k in range(n):
            B.ops[f"y{k}"] = (B.ops[f"y{k}"][0], "in")
        r.rc_bwd, r.labels_bwd = _labelled(lib, lambda: lib.c.mlhot_mlp_chain_bwd(
            C.c_void_p(B.addr("x0")), c.ld["x0"], M, Ls, Gs, n, C.c_void_p(B.addr("dy")), c.ld["dy"],
            C.c_void_p(B.addr("dx0")) if c.dx0 else None, c.ld["dx0"], c.dx0_acc, st))
        _sync(device)
        r.bad_bwd = B.untouched()
        r.g, r.dw, r.db = ([B.win(f"{p}{k}") for k in range(n)] for p in ("g", "dw", "db"))
        r.db = [None if v is None else v.reshape(-1) for v in r.db]
        r.dside = [B.win(f"dside{k}") for k in range(n)]
        r.dx0 = B.win("dx0")
    return r


def chain_wgrad_alone(lib, c, r, device):
    """Every weight-gradient job of the chain through mlhot_linear_bwd (dx = NULL: the skinny weight gradient alone) on the chain's own
    g and inputs -> [(layer, first column, dw [N, cols], db | None)]."""
    out, st, B = [], _stream(device), r.bank
    for k, l in enumerate(c.layers):
        xin = B.ops["x0"][0] if k == 0 else B.ops[f"y{k - 1}"][0]
        g = B.ops[f"g{k}"][0]
        srcs = [(xin, l.side_w if l.side_first else 0, l.K - l.side_w, l.b)]
        if l.side_w:
            srcs.append((B.ops[f"side{k}"][0], 0 if l.side_first else l.K - l.side_w, l.side_w, False))
        for x, col0, cols, with_b in srcs:
            dw = torch.full((l.N, cols), SENTINEL, device=device)
            db = torch.full((l.N,), SENTINEL, device=device)
            rc = lib.c.mlhot_linear_bwd(x.ptr(), x.ld, B.ops[f"w{k}"][0].ptr(), None, 0, g.ptr(), g.ld, c.M, cols, l.N, 0, None, 0, 0,
                                        C.c_void_p(dw.data_ptr()), C.c_void_p(db.data_ptr()) if with_b else None, None, 0, st)
            assert rc == 0, lib.c.mlhot_last_error().decode()
            _sync(device)
            out.append((k, col0, dw.cpu(), db.cpu() if with_b else None))
    return out


# ---- linear_multi's cases ------------------------------------------------------------------------------------------------------------
def job(M, K, N, act="none", K2=0, dx=True, dx2=False, acc=0, b=True, K2_arg=None, tight=False, ld=None, off=None):
    """One Linear job: x [M, K - K2] (+ x2 [M, K2]).  dx / dx2: which input gradients are wanted; b = False: b and db NULL; K2_arg: the
    struct's K2 when it is not the second operand's width (refusals).  Strides: all larger than their width and multiples of 4
    (N % 4 != 0, forward only: ldy odd) unless tight; x and dx are column windows 4 floats into wider buffers."""
    p = 0 if tight else 1
    K1 = K - K2
    j = types.SimpleNamespace(M=M, K=K, N=N, act=act, K1=K1, K2=K2, dx=dx, dx2=dx2, acc=acc, b=b, K2_arg=K2 if K2_arg is None else K2_arg)
    j.ld = dict(x=_up4(K1) + 4 * p, x2=K2 + 8 * p, y=N + (4 if N % 4 == 0 else 1) * p, dy=N + 4 * p, dx=_up4(K1) + 8 * p, dx2=K2 + 4 * p)
    j.off = dict(x=4 * p, x2=0, w=0, y=0, dy=0, dx=4 * p, dx2=0)
    j.ld.update(ld or {})
    j.off.update(off or {})
    return j


def table(name, jobs, bwd=True, seed=0):
    for i, j in enumerate(jobs):
        j.jid, j.seed = f"{name}/{i}", seed
    return types.SimpleNamespace(name=name, jobs=jobs, bwd=bwd, seed=seed)


SEAMS = [(K1, K2) for K1 in (4, 20, 60, 68) for K2 in (4, 12)]
MODES = [dict(dx=True, dx2=False), dict(dx=False, dx2=True), dict(dx=True, dx2=True)]


def _seam_table(shift):
    acts = ["none", "relu", "tanh"]
    return table(f"two_source_{shift}", [job(33 + 2 * i, K1 + K2, 8 + 4 * i, acts[i % 3], K2=K2, acc=int((i + shift) % 4 == 1), **MODES[(i + shift) % 3])
                                        for i, (K1, K2) in enumerate(SEAMS)])


def _multi_cases():
    J = job
    return [
        table("one_M1_K4_N4", [J(1, 4, 4)]),
        table("two_shapes", [J(31, 20, 124, "relu"), J(33, 64, 132, "tanh")]),
        # 8 jobs, every M of the 32-row tile edges, every K (516 = past two 256-k trips), the backward's N edges of the 128-column trips
        table("eight_shapes", [J(1, 4, 4), J(31, 20, 124, "relu"), J(32, 64, 128, "tanh"), J(33, 260, 132), J(63, 516, 4, "relu"),
                               J(64, 8, 12, "tanh"), J(65, 12, 20), J(512, 16, 8, "relu")], seed=1),
        table("fwd_oddN", [J(33, 20, 5, "relu"), J(17, 8, 1), J(64, 12, 131, "tanh"), J(31, 24, 6, "none", K2=4)], bwd=False),
        _seam_table(0), _seam_table(1), _seam_table(2),
        table("acc", [J(40, 32, 24, "relu", acc=1), J(17, 24, 8, "tanh", K2=4, dx2=True, acc=1)]),
        table("nob_nodb", [J(33, 20, 12, "relu", b=False), J(17, 24, 8, "none", K2=12, dx2=True, b=False)]),
        table("tight", [J(33, 20, 12, "tanh", tight=True), J(17, 24, 8, "relu", K2=4, dx2=True, tight=True)]),
        # jobs without rows: first, in the middle, last, the whole table
        table("empty_first", [J(0, 20, 12, "relu"), J(33, 8, 4), J(17, 24, 8, "tanh", K2=4, dx2=True)]),
        table("empty_middle", [J(33, 8, 4), J(0, 24, 8, "tanh", K2=4, dx2=True), J(17, 20, 12, "relu")]),
        table("empty_last", [J(33, 8, 4), J(17, 20, 12, "relu"), J(0, 68, 20, "none", b=False)]),
        table("empty_all", [J(0, 20, 12, "relu"), J(0, 8, 4), J(0, 24, 8, "tanh", K2=4, dx2=True)]),
    ]


MULTI_CASES = _multi_cases()


def _multi_refusals():
    J = job
    ok = lambda: J(17, 8, 4)
    return [
        (table("ref_M513", [ok(), J(513, 8, 4)]), "fwd"),
        (table("ref_9jobs", [J(17, 8, 4) for _ in range(9)]), "fwd"),
        (table("ref_K6", [J(17, 6, 4)]), "fwd"),
        (table("ref_x_unaligned", [ok(), J(17, 8, 4, off=dict(x=1))]), "fwd"),
        (table("ref_w_unaligned", [J(17, 8, 4, off=dict(w=1))]), "fwd"),
        (table("ref_ldx6", [J(17, 8, 4, ld=dict(x=10))]), "fwd"),
        (table("ref_x2_unaligned", [J(17, 12, 4, K2=4, off=dict(x2=1))]), "fwd"),
        (table("ref_K2_is_K", [J(17, 12, 4, K2=4, K2_arg=12)]), "fwd"),
        (table("ref_K2_odd", [J(17, 12, 4, K2=4, K2_arg=6)]), "fwd"),
        (table("ref_ldy_short", [J(17, 8, 12, ld=dict(y=8))]), "fwd"),
        (table("ref_bwd_N6", [J(17, 8, 6)]), "bwd"),
        (table("ref_bwd_no_dx", [ok(), J(17, 8, 4, dx=False)]), "bwd"),
        (table("ref_bwd_no_dx_dx2", [J(17, 12, 4, K2=4, dx=False, dx2=False)]), "bwd"),
        (table("ref_bwd_dy_unaligned", [J(17, 8, 4, off=dict(dy=1))]), "bwd"),
        (table("ref_bwd_lddy_short", [J(17, 8, 12, ld=dict(dy=8))]), "bwd"),
    ]


MULTI_REFUSALS = _multi_refusals()


def multi_refused(t, bwd):
    """check_multi restated on the table (buffers start 16-byte aligned): the reason, or None."""
    if not 1 <= len(t.jobs) <= MAXJ:
        return "job count"
    for i, j in enumerate(t.jobs):
        al = lambda key: j.off[key] % 4 == 0 and j.ld[key] % 4 == 0
        ok = 0 <= j.M <= MAX_ROWS and j.K >= 4 and j.K % 4 == 0 and j.N >= 1 and al("x") and j.off["w"] % 4 == 0 and j.ld["y"] >= j.N
        if j.K2:
            ok = ok and j.K2_arg >= 4 and j.K2_arg % 4 == 0 and j.K2_arg < j.K and al("x2")
        if bwd:
            ok = ok and (j.M == 0 or j.dx or (j.K2 and j.dx2)) and j.N % 4 == 0 and al("dy") and j.ld["dy"] >= j.N and (j.act == "none" or al("y"))
            ok = ok and (not j.dx or al("dx")) and (not (j.K2 and j.dx2) or al("dx2"))
        if not ok:
            return f"job {i}"
    return None


def multi_blocks(t, bwd):
    """fill_jobs restated: [(first block, blocks)] of the jobs the launch keeps.  Forward: gdx * ceil(N / 16), gdx = ceil(M / 32), jobs
    without rows dropped; backward: gdx * ceil(K / 16) data-gradient blocks + ceil(N / 16) * ceil(K / 64) weight-gradient blocks (a job
    without rows keeps the latter)."""
    out, total = [], 0
    for j in t.jobs:
        gdx = _cdiv(j.M, 32)
        if not bwd and j.M == 0:
            continue
        blocks = gdx * _cdiv(j.N, 16) if not bwd else gdx * _cdiv(j.K, 16) + _cdiv(j.N, 16) * _cdiv(j.K, 64)
        out.append((total, blocks))
        total += blocks
    return out


def job_data(j):
    g = _gen("job/" + j.jid, j.seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return types.SimpleNamespace(x=r(j.M, j.K1), x2=r(j.M, j.K2), w=r(j.N, j.K) / j.K ** 0.5, b=0.5 * r(j.N), dy=r(j.M, j.N), dx_prior=r(j.M, j.K1),
                                 dx2_prior=r(j.M, j.K2))


def job_reference(j, d):
    x, x2 = d.x.double().requires_grad_(True), d.x2.double().requires_grad_(True)
    w = d.w.double().requires_grad_(True)
    b = d.b.double().requires_grad_(True) if j.b else None
    pre = (torch.cat([x, x2], -1) if j.K2 else x) @ w.t() + (b if b is not None else 0.0)
    y = act64(j.act, pre)
    y.backward(d.dy.double())
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return types.SimpleNamespace(y=y.detach(), pre=pre.detach(), dw=zero(w), db=zero(b) if b is not None else None,
                                 dx=zero(x) + (d.dx_prior.double() if j.acc else 0.0) if j.dx else None,
                                 dx2=zero(x2) + (d.dx2_prior.double() if j.acc else 0.0) if (j.K2 and j.dx2) else None)


def _job_bank(j, d, device):
    B = _Bank(device)
    B.add("x", "in", j.M, j.K1, j.ld["x"], j.off["x"], d.x)
    B.add("x2", "in", j.M, j.K2, j.ld["x2"], j.off["x2"], d.x2)
    B.add("w", "in", j.N, j.K, j.K, j.off["w"], d.w)
    B.add("b", "in" if j.b else "null", 1, j.N, j.N, 0, d.b)
    B.add("y", "out", j.M, j.N, j.ld["y"], j.off["y"])
    B.add("dy", "in", j.M, j.N, j.ld["dy"], j.off["dy"], d.dy)
    B.add("dx", "out" if j.dx else "null", j.M, j.K1, j.ld["dx"], j.off["dx"], d.dx_prior if j.acc else None)
    B.add("dx2", "out" if (j.K2 and j.dx2) else "null", j.M, j.K2, j.ld["dx2"], j.off["dx2"], d.dx2_prior if j.acc else None)
    B.add("dw", "out", j.N, j.K, j.K)
    B.add("db", "out" if j.b else "null", 1, j.N, j.N)
    B.snapshot()
    return B


def _job_struct(j, B):
    return LinearJob(B.addr("x"), j.ld["x"], B.addr("w"), B.addr("b"), B.addr("y"), j.ld["y"], j.M, j.K, j.N, ACT_CODE[j.act], B.addr("dy"), j.ld["dy"],
                     B.addr("dx"), j.ld["dx"], j.acc, B.addr("dw"), B.addr("db"), B.addr("x2") if j.K2 else None, j.ld["x2"], j.K2_arg,
                     B.addr("dx2"), j.ld["dx2"])


def run_multi(lib, jobs, device, bwd=True):
    """mlhot_linear_multi_fwd, then (bwd) mlhot_linear_multi_bwd on the forward's own ys, every job on its own sentinel-filled buffers.
    Returns a namespace: rc_fwd / rc_bwd, labels_*, bad_* ("job/operand" that changed where it must not), jobs: [namespace(y, dx, dx2,
    dw, db, bank, data)]."""
    n = len(jobs)
    data = [job_data(j) for j in jobs]
    banks = [_job_bank(j, d, device) for j, d in zip(jobs, data)]
    Js = (LinearJob * n)()
    for i, (j, B) in enumerate(zip(jobs, banks)):
        Js[i] = _job_struct(j, B)
    st = _stream(device)
    r = types.SimpleNamespace(rc_bwd=None, labels_bwd=None, bad_bwd=None)
    r.rc_fwd, r.labels_fwd = _labelled(lib, lambda: lib.c.mlhot_linear_multi_fwd(Js, n, st))
    _sync(device)
    bwd_outs = ("dx", "dx2", "dw", "db")
    r.bad_fwd = [f"{i}/{name}" for i, B in enumerate(banks) for name in B.untouched() if name not in bwd_outs]
    r.bad_fwd += [f"{i}/{name}" for i, B in enumerate(banks) for name in bwd_outs if not B.ops[name][0].unchanged()]
    r.jobs = [types.SimpleNamespace(y=B.win("y"), bank=B, data=d) for B, d in zip(banks, data)]
    if bwd:
        for B in banks:
            B.snapshot()
            B.ops["y"] = (B.ops["y"][0], "in")
        r.rc_bwd, r.labels_bwd = _labelled(lib, lambda: lib.c.mlhot_linear_multi_bwd(Js, n, st))
        _sync(device)
        r.bad_bwd = [f"{i}/{name}" for i, B in enumerate(banks) for name in B.untouched()]
        for o, B in zip(r.jobs, banks):
            o.dx, o.dx2, o.dw, o.db = B.win("dx"), B.win("dx2"), B.win("dw"), B.win("db")
            o.db = None if o.db is None else o.db.reshape(-1)
    return r


def run_job_alone(lib, j, device):
    """A one-source job through mlhot_linear_fwd / mlhot_linear_bwd (skinny forward, combined skinny backward: the same sk:: bodies in
    the same order) on the same data, strides and offsets -> namespace(y, dx, dw, db)."""
    assert not j.K2 and j.dx
    d = job_data(j)
    B = _job_bank(j, d, device)
    p = lambda name: None if B.addr(name) is None else C.c_void_p(B.addr(name))
    st = _stream(device)
    rc = lib.c.mlhot_linear_fwd(p("x"), j.ld["x"], p("w"), p("b"), p("y"), j.ld["y"], j.M, j.K, j.N, ACT_CODE[j.act], st)
    assert rc == 0, lib.c.mlhot_last_error().decode()
    _sync(device)
    o = types.SimpleNamespace(y=B.win("y"), labels=None)
    if j.N % 4 == 0:
        o.rc, o.labels = _labelled(lib, lambda: lib.c.mlhot_linear_bwd(p("x"), j.ld["x"], p("w"), p("y"), j.ld["y"], p("dy"), j.ld["dy"], j.M, j.K, j.N,
                                                                       ACT_CODE[j.act], p("dx"), j.ld["dx"], j.acc, p("dw"), p("db"), None, 0, st))
        assert o.rc == 0, lib.c.mlhot_last_error().decode()
        _sync(device)
        o.dx, o.dw, o.db = B.win("dx"), B.win("dw"), B.win("db")
        o.db = None if o.db is None else o.db.reshape(-1)
    return o


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
