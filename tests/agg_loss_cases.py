"""Shared by tests/test_agg_loss_cases_cpu.py (host flavour of the library) and tests/test_agg_loss_envelope_gpu.py (MI355X): the
shot-axis aggregators (AggFwd / AggBwd in csrc/ops_direct.h, AggPrefixFwd in csrc/prefix.h) and the losses (LossRed / LossBwd and their
Plus twins over reduce1_kernel in csrc/foreach.h), called directly through the binding - bit for bit where the operation is exact or a
single rounding (mean on a dyadic grid, max and its arg-max, the prefix rows against agg_fwd, loss_prefix_fwd against loss_fwd,
loss_plus against loss + axpy), against float64 where it sums or divides (BACO per column at util.RTOL, the loss values at the bound of
test_losses_against_reference_vectors, the loss gradients at util.RTOL).

Sizes: run_foreach clamps its grid at 4096 workgroups of 256 threads and strides beyond, the aggregators run one lane per (task,
feature), so T * R = 4096 * 256 sits at the clamp and the two shapes past it stride.  reduce1_block sums rows < 1024 one per thread,
rows up to 3072 in the `i += 1024` tail loop and rows > 3072 in four accumulators per thread: LOSS_ROWS has one below / at / above each
change, and the four-accumulator loop with one, two and three full rounds plus a tail.

The inputs of the selecting operations (max, the quaternion's minimum and signs, the degree error's fold and wrap) are built so that
float64 and fp32 cannot choose differently; tests/test_agg_loss_cases_cpu.py checks that on every case, with no exception allowed."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import util as U
from tests.glue_ops import CLAMP, bits_equal, need  # noqa: F401  (need: re-exported for the two test files)

ERR_ARG = 1                                        # csrc/common.h MLHOT_ERR_ARG
SENTINEL = -777.25

AGG_SHAPES = [(1, 1, 1), (1, 1, 257), (3, 2, 100), (2, 30, 64), (2, 33, 7), (5, 7, 255), (5, 7, 256), (5, 7, 257),
              (4096, 1, 256), (4097, 2, 256), (1, 3, CLAMP + 1)]
BACO_SHAPES = [(3, 7, 100), (2, 30, 64)]
BACO_REGIMES = ["randn2", "threshold", "deep", "all_deep"]
PREFIX_SHAPE = (2, 30, 64)                         # mean / max rows against agg_fwd at Nc = 30

LOSS_ROWS = [1, 2, 1023, 1024, 1025, 3072, 3073, 4095, 4096, 4097, 8193, 12289]
# (kind, y_dim, gt_dim)
LOSS_KINDS = [("mse", 1, 1), ("mse", 3, 3), ("mse", 8, 8), ("azimuth", 2, 2), ("azimuth", 2, 3), ("quaternion", 4, 4),
              ("degree", 2, 1), ("degree", 2, 3), ("distractor", 2, 2)]
TRAIN_KINDS = [("azimuth", 2, 3), ("mse", 3, 3), ("quaternion", 4, 4), ("distractor", 2, 2)]
PREFIX_P = [1, 2, 25]
PREFIX_ROWS = [1025, 4097]
PLUS_ROWS = [1, 1025, 4097]
UPSTREAM = [1.0, -2.25]
TASK = {"azimuth": ("shapenet_1d", False), "mse": ("pascal_1d", False), "quaternion": ("shapenet_3d", False),
        "degree": ("shapenet_1d", True), "distractor": ("distractor", False)}
QUAT_SCALES = (0.01, 1.0, 37.0)
RAD2DEG = 180.0 / math.pi


def ids(case):
    return "-".join(str(v) for v in case) if isinstance(case, tuple) else str(case)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(torch.device(dev)).cuda_stream) if dev != "cpu" else None


def _P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def column_err(got, ref):
    """Worst error over the (task, feature) columns: max |got - ref| over the shots of a column / max |ref| over the same column (floor
    1e-30).  got, ref: [T, Nc, R] with the shots on axis 1, or [T, R] (a column of one entry)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.dim() == 2:
        got, ref = got.unsqueeze(1), ref.unsqueeze(1)
    diff = (got - ref).abs().amax(dim=1)
    return float((diff / ref.abs().amax(dim=1).clamp_min(1e-30)).max())


# ---- mean -------------------------------------------------------------------------------------------------------------------
def mean_inputs(shape):
    """rs and dr on the dyadic grid k / 64, |k| <= 256: every partial sum of <= 33 shots is a multiple of 2^-6 below 2^8, exact in fp32."""
    T, Nc, R = shape
    g = _gen(101 + T + 10 * Nc + R)
    rs = torch.randint(-256, 257, (T, Nc, R), generator=g).float() / 64.0
    dr = torch.randint(-256, 257, (T, R), generator=g).float() / 64.0
    return rs, dr


def mean_reference(rs):
    """Row k-1: the float64 sum of the first k shots cast to fp32 (exact) and divided by float32(k) in fp32 - one rounding.  [Nc, T, R]."""
    Nc = rs.shape[1]
    sums = rs.double().cumsum(dim=1).float()
    return (sums / torch.arange(1, Nc + 1, dtype=torch.float32).view(1, Nc, 1)).permute(1, 0, 2).contiguous()


def check_mean(lib, shape, dev):
    T, Nc, R = shape
    rs, dr = mean_inputs(shape)
    rows = mean_reference(rs)
    rsd = rs.to(dev)
    r, sigma, amax = lib.agg_fwd("mean", rsd)
    assert bits_equal(r, rows[Nc - 1]), f"agg_fwd mean {shape}: {int((r.cpu() != rows[Nc - 1]).sum())} of {T * R} differ"
    drs, dlv = lib.agg_bwd("mean", rsd, None, r, sigma, amax, dr.to(dev))
    want = (dr / torch.tensor(float(Nc), dtype=torch.float32)).unsqueeze(1).expand(T, Nc, R)
    assert dlv is None and bits_equal(drs, want), f"agg_bwd mean {shape}"
    pre, _ = lib.agg_prefix_fwd("mean", rsd)
    assert bits_equal(pre, rows), f"agg_prefix_fwd mean {shape}"
    print(f"agg mean {shape}: r, drs and {Nc} prefix rows bit-equal to the one-rounding reference")


# ---- max --------------------------------------------------------------------------------------------------------------------
MAX_VALUES = torch.tensor([-1.5, -0.0, 0.0, 0.75, 0.75])   # the largest twice as likely; -0.0 against 0.0; most columns tie for Nc >= 3


def max_inputs(shape):
    T, Nc, R = shape
    g = _gen(211 + T + 10 * Nc + R)
    rs = MAX_VALUES[torch.randint(0, 5, (T, Nc, R), generator=g)]
    dr = torch.randn(T, R, generator=g)
    return rs, dr


def first_greater_scan(rs):
    """The stored convention: the winner is the first maximum in shot order, replaced only by a STRICTLY greater value (-0.0 == 0.0, so
    whichever zero comes first stays).  Returns (values [Nc, T, R] with the winner's bits for every prefix, arg [T, R] int32)."""
    T, Nc, R = rs.shape
    best, arg = rs[:, 0].clone(), torch.zeros(T, R, dtype=torch.int32)
    rows = [best.clone()]
    for n in range(1, Nc):
        v = rs[:, n]
        take = v > best
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, n), arg)
        rows.append(best.clone())
    return torch.stack(rows), arg


def max_tie_fraction(rs):
    return float(((rs == rs.max(dim=1, keepdim=True).values).sum(dim=1) > 1).float().mean())


def check_max(lib, shape, dev):
    T, Nc, R = shape
    rs, dr = max_inputs(shape)
    rows, arg = first_greater_scan(rs)
    rsd = rs.to(dev)
    r, sigma, amax = lib.agg_fwd("max", rsd)
    assert bits_equal(r, rows[Nc - 1]), f"agg_fwd max {shape}: value bits"
    assert torch.equal(r.cpu(), rs.max(dim=1).values), f"agg_fwd max {shape}: value"
    assert amax.dtype == torch.int32 and torch.equal(amax.cpu(), arg), f"agg_fwd max {shape}: arg-max (first maximum in shot order)"
    drs, _ = lib.agg_bwd("max", rsd, None, r, sigma, amax, dr.to(dev))
    want = torch.zeros(T, Nc, R).scatter_(1, arg.long().unsqueeze(1), dr.unsqueeze(1))
    assert bits_equal(drs, want), f"agg_bwd max {shape}: dr at the winner, +0.0 elsewhere"
    pre, _ = lib.agg_prefix_fwd("max", rsd)
    assert bits_equal(pre, rows), f"agg_prefix_fwd max {shape}"
    print(f"agg max {shape}: {max_tie_fraction(rs):.0%} of the columns tie; r, amax, drs and {Nc} prefix rows bit-equal to the scan")


# ---- BACO -------------------------------------------------------------------------------------------------------------------
THRESHOLD_LV = (19.5, 20.0, 20.000002, 20.5, 60.0, 100.0)   # F.softplus's threshold of 20: below, at, one fp32 ulp above, far above
DEEP_LV = (-15.0, -17.0, -30.0, -100.0)                     # softplus 3e-7 ... exactly 0: var is the 1e-5 floor; expf(-lv) overflows at -100


def baco_inputs(shape, regime):
    T, Nc, R = shape
    g = _gen(307 + T + 10 * Nc + R + 1000 * BACO_REGIMES.index(regime))
    rs, dr = torch.randn(T, Nc, R, generator=g), torch.randn(T, R, generator=g)
    lv = torch.randn(T, Nc, R, generator=g)
    if regime == "randn2":
        lv = lv * 2
    elif regime == "all_deep":
        lv = torch.full_like(lv, -100.0)
    else:
        special = torch.tensor(THRESHOLD_LV if regime == "threshold" else DEEP_LV)
        pick = special[torch.randint(0, len(special), (T, Nc, R), generator=g)]
        lv = torch.where(torch.rand(T, Nc, R, generator=g) < 0.3, pick, lv)
    return rs, lv, dr


def baco_reference(rs, lv, dr):
    """O.agg_baco(rs, 1e-5 + softplus(lv)) in float64 under autograd, and every prefix of it as running sums.  -> dict"""
    rr, ll = rs.double().requires_grad_(True), lv.double().requires_grad_(True)
    var = 1e-5 + F.softplus(ll)
    mu_z, sigma_z = O.agg_baco(rr, var)
    mu_z.backward(dr.double())
    with torch.no_grad():
        inv = 1.0 / var
        s1 = 1.0 + inv.cumsum(dim=1)
        pre_r, pre_sigma = (inv * rr).cumsum(dim=1) / s1, 1.0 / s1
    return dict(r=mu_z.detach(), sigma_z=sigma_z.detach(), drs=rr.grad, dlv=ll.grad, prefix_r=pre_r, prefix_sigma=pre_sigma)


def check_baco(lib, shape, regime, dev):
    """r, sigma_z, drs, dlv and the prefix rows against float64, per (task, feature) column at util.RTOL -> {quantity: worst error}."""
    rs, lv, dr = baco_inputs(shape, regime)
    ref = baco_reference(rs, lv, dr)
    rsd, lvd = rs.to(dev), lv.to(dev)
    r, sigma, amax = lib.agg_fwd("baco", rsd, lvd)
    drs, dlv = lib.agg_bwd("baco", rsd, lvd, r, sigma, amax, dr.to(dev))
    pre_r, pre_sigma = lib.agg_prefix_fwd("baco", rsd, lvd, want_sigma=True)
    got = dict(r=r, sigma_z=sigma, drs=drs, dlv=dlv, prefix_r=pre_r.permute(1, 0, 2), prefix_sigma=pre_sigma.permute(1, 0, 2))
    for k in ("r", "sigma_z", "drs", "dlv"):
        assert bool(torch.isfinite(got[k]).all()), f"agg baco {shape} {regime}: {k} is not finite"
    errs = {k: column_err(got[k], ref[k]) for k in ref}
    print(f"agg baco {shape} {regime}: worst per-column error " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f" (bound {U.RTOL:.0e})")
    for k, e in errs.items():
        assert e <= U.RTOL, f"agg baco {shape} {regime}: {k} per-column error {e:.2e} > {U.RTOL:.0e}"
    return errs


# ---- the prefix rows against agg_fwd on the sliced input --------------------------------------------------------------------
def check_prefix_rows_equal_agg_fwd(lib, mode, shape, regime, dev):
    """Row k-1 of agg_prefix_fwd has the bits of agg_fwd(rs[:, :k]) (csrc/prefix.h's header), sigma_z included."""
    if mode == "baco":
        rs, lv, _ = baco_inputs(shape, regime)
    else:
        rs, lv = (mean_inputs if mode == "mean" else max_inputs)(shape)[0], None
        if mode == "mean":
            rs = rs + torch.randn(rs.shape, generator=_gen(5)) * 0.37        # off the grid: the sums round
    rsd, lvd = rs.to(dev), (lv.to(dev) if lv is not None else None)
    pre_r, pre_sigma = lib.agg_prefix_fwd(mode, rsd, lvd, want_sigma=True)
    bad = []
    for k in range(1, shape[1] + 1):
        r, sigma, _ = lib.agg_fwd(mode, rsd[:, :k].contiguous(), lvd[:, :k].contiguous() if lvd is not None else None)
        if not bits_equal(pre_r[k - 1], r) or (mode == "baco" and not bits_equal(pre_sigma[k - 1], sigma)):
            bad.append((k, U.rel_err(pre_r[k - 1], r)))
    print(f"agg prefix rows {mode} {shape} {regime}: {shape[1] - len(bad)} of {shape[1]} rows bit-equal to agg_fwd on the slice")
    assert not bad, f"agg_prefix_fwd {mode} {shape} {regime}: rows (k, rel err) differ from agg_fwd(rs[:, :k]): {bad[:5]}"


# ---- aggregator refusals ----------------------------------------------------------------------------------------------------
AGG_REFUSED = [(3, 2, 3, 4, "mode = 3"), (-1, 2, 3, 4, "mode = -1"), (0, 0, 3, 4, "T = 0"), (1, 2, 0, 4, "Nc = 0"), (2, 2, 3, 0, "R = 0")]


def check_agg_refusals(lib, dev):
    """MLHOT_ERR_ARG through the raw entries, named by mlhot_last_error, and nothing written."""
    stream = _stream(dev)
    for mode, T, Nc, R, why in AGG_REFUSED:
        t, n, rr = max(T, 1), max(Nc, 1), max(R, 1)
        rs, lv, dr = (torch.ones(t, n, rr, device=dev), torch.ones(t, n, rr, device=dev), torch.ones(t, rr, device=dev))
        r, sigma, drs, dlv = (torch.full(s, SENTINEL, device=dev) for s in ((n, t, rr), (n, t, rr), (t, n, rr), (t, n, rr)))
        amax = torch.full((t, rr), -7, dtype=torch.int32, device=dev)
        calls = {"agg_fwd": lambda: lib.c.mlhot_agg_fwd(mode, _P(rs), _P(lv), T, Nc, R, _P(r), _P(sigma), _P(amax), stream),
                 "agg_bwd": lambda: lib.c.mlhot_agg_bwd(mode, _P(rs), _P(lv), _P(r), _P(sigma), _P(amax), _P(dr), T, Nc, R, _P(drs), _P(dlv), stream)}
        if dev != "cpu" or hasattr(lib.c, "mlhot_agg_prefix_fwd"):      # the product must export it; the host flavour may lack it
            calls["agg_prefix_fwd"] = lambda: lib.c.mlhot_agg_prefix_fwd(mode, _P(rs), _P(lv), T, Nc, R, _P(r), _P(sigma), stream)
        for name, call in calls.items():
            rc = call()
            assert rc == ERR_ARG, (name, why, rc)
            assert name.encode() in lib.c.mlhot_last_error(), (name, why, lib.c.mlhot_last_error())
        _sync(dev)
        assert all(bool((t_ == SENTINEL).all()) for t_ in (r, sigma, drs, dlv)) and bool((amax == -7).all()), f"{why}: a refused call wrote something"


# ---- loss inputs ------------------------------------------------------------------------------------------------------------
def _unit(x):
    return x / x.pow(2).sum(dim=-1, keepdim=True).sqrt()


def quaternion_inputs(rows, P, g):
    """gt = +-v for a random unit v (even rows +, odd rows -), mu[p] = s * u_p for a unit u_p whose every component is at least 0.05
    off v's and a scale s from QUAT_SCALES: u_p is close to sign * gt, so the L1 distance to that side is <= 0.8 and to the other
    >= 2 |u|_1 - 0.8 >= 1.2 (|u|_1 >= |u|_2 = 1): the minimum, `sgn` and every sign(sgn * g_j - u_j) are decided far from a tie."""
    v = _unit(torch.randn(rows, 4, generator=g, dtype=torch.float64))
    u = torch.empty(P, rows, 4, dtype=torch.float64)
    todo = torch.ones(P, rows, dtype=torch.bool)
    for _ in range(200):
        n = int(todo.sum())
        if n == 0:
            break
        d = (0.08 + 0.12 * torch.rand(n, 4, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (n, 4), generator=g) * 2 - 1)
        base = v.unsqueeze(0).expand(P, rows, 4)[todo]
        cand = _unit(base + d)
        ok = (cand - base).abs().amin(dim=-1) >= 0.05
        idx = todo.nonzero()[ok]
        u[idx[:, 0], idx[:, 1]] = cand[ok]
        todo[idx[:, 0], idx[:, 1]] = False
    assert not bool(todo.any()), "quaternion_inputs: rejection sampling did not finish"
    r = torch.arange(rows)
    sign = torch.where(r % 2 == 0, 1.0, -1.0).double().unsqueeze(-1)
    scale = torch.tensor(QUAT_SCALES, dtype=torch.float64)[(r.unsqueeze(0) + torch.arange(P).unsqueeze(1)) % 3].unsqueeze(-1)
    return (scale * u).float(), (sign * v).float()


def degree_inputs(rows, gt_dim, P, g):
    """mu = (cos a, sin a), 12 <= a <= 168 degrees (row % 4 == 0: m[1] > 0) or 192 <= a <= 348 (row % 4 == 1: m[1] < 0, the fold), or
    (cos a, +0.0) / (cos a, -0.0) with a <= 168 (row % 4 == 2, 3: neither folds): the predicted angle pd lies in [12, 348], |cos a| <= 0.98.
    The label's angle gd picks the winning wrap for every such pd ((row // 4) % 3): 170 .. 190 -> |gd - pd| <= 178, the others >= 182;
    -300 .. -170 -> |gd + 360 - pd| wins by >= 4 degrees; 530 .. 650 -> |gd - (pd + 360)| wins by >= 4 degrees.  The label's other
    columns (gt_dim > 1; the kernel reads the last) hold 100 + N(0, 1)."""
    r = torch.arange(rows)
    fold = (r % 4).unsqueeze(0).expand(P, rows)
    a = 12.0 + 156.0 * torch.rand(P, rows, generator=g, dtype=torch.float64)
    a = torch.where(fold == 1, a + 180.0, a) / RAD2DEG
    m1 = torch.where(fold == 2, torch.tensor(0.0, dtype=torch.float64), torch.where(fold == 3, torch.tensor(-0.0, dtype=torch.float64), a.sin()))
    mu = torch.stack([a.cos(), m1], dim=-1).float()
    w = (r // 4) % 3
    lo = torch.tensor([170.0, -300.0, 530.0], dtype=torch.float64)[w]
    span = torch.tensor([20.0, 130.0, 120.0], dtype=torch.float64)[w]
    gd = lo + span * torch.rand(rows, generator=g, dtype=torch.float64)
    gt = 100.0 + torch.randn(rows, gt_dim, generator=g, dtype=torch.float64)
    gt[:, -1] = gd / RAD2DEG
    return mu, gt.float()


def distractor_inputs(rows, P, g, equal_row=None):
    """|mu - gt| between 2e-3 and 2 in every row (>= 1e-3 after the rounding to fp32); equal_row: that row of every mu[p] is gt's, bit for bit."""
    gt = torch.randn(rows, 2, generator=g, dtype=torch.float64)
    dist = 2e-3 * 10.0 ** (3.0 * torch.rand(P, rows, 1, generator=g, dtype=torch.float64))
    ang = 2.0 * math.pi * torch.rand(P, rows, generator=g, dtype=torch.float64)
    mu = (gt.unsqueeze(0) + dist * torch.stack([ang.cos(), ang.sin()], dim=-1)).float()
    gt = gt.float()
    if equal_row is not None:
        mu[:, equal_row] = gt[equal_row]
    else:
        assert float((mu.double() - gt.double()).pow(2).sum(-1).sqrt().min()) >= 1e-3
    return mu, gt


def loss_inputs(case, rows, P=1, equal_row=None):
    """mu [P, rows, y_dim] and the labels [rows, gt_dim] the P slices share."""
    kind, y_dim, gt_dim = case
    g = _gen(401 + 7 * LOSS_KINDS.index(case) + 131 * rows + 17 * P)
    if kind == "quaternion":
        return quaternion_inputs(rows, P, g)
    if kind == "degree":
        return degree_inputs(rows, gt_dim, P, g)
    if kind == "distractor":
        return distractor_inputs(rows, P, g, equal_row)
    return torch.randn(P, rows, y_dim, generator=g), torch.randn(rows, gt_dim, generator=g)


def quaternion_choices(mu, gt):
    """What the quaternion loss selects, in mu's dtype: (the branch p < q, sign(sgn * g_j - u_j), |p - q|, min_j |sgn * g_j - u_j|)."""
    u = mu / mu.pow(2).sum(dim=-1, keepdim=True).sqrt()
    p, q = (gt - u).abs().sum(dim=-1), (-gt - u).abs().sum(dim=-1)
    sgn = torch.where(p <= q, 1.0, -1.0).to(mu.dtype).unsqueeze(-1)
    e = sgn * gt - u
    return p < q, torch.sign(e), (p - q).abs(), e.abs().amin(dim=-1)


def degree_choices(mu, gt):
    """What the degree error selects, in mu's dtype: (the fold m[1] < 0, the winning wrap candidate, its margin over the other two in degrees)."""
    gd = torch.rad2deg(gt[..., -1])
    ang = torch.acos(mu[..., 0])
    fold = mu[..., 1] < 0
    pd = torch.rad2deg(torch.where(fold, 2 * math.pi - ang, ang))
    err = torch.stack([(gd - pd).abs(), (gd + 360.0 - pd).abs(), (gd - (pd + 360.0)).abs()], dim=-1)
    two = err.topk(2, dim=-1, largest=False).values
    return fold, err.argmin(dim=-1), two[..., 1] - two[..., 0]


def loss_reference(case, mu, gt):
    """O.calc_loss on float64 copies -> (value, d loss / d mu for an upstream of 1, or None for the evaluation-only degree error)."""
    task, test = TASK[case[0]]
    m = mu.double().requires_grad_(True)
    loss = O.calc_loss(task, m, gt.double(), test=test)
    if test:
        return float(loss.detach()), None
    loss.backward()
    return float(loss.detach()), m.grad


# ---- loss checks ------------------------------------------------------------------------------------------------------------
def value_bound(want):
    return 1e-5 * max(1.0, abs(want))               # test_losses_against_reference_vectors' bound


def check_loss(lib, case, rows, dev):
    """loss_fwd against float64 at value_bound, loss_bwd for both upstream scalars against float64 autograd at util.RTOL (degree:
    all zeros) -> (value error / bound, worst gradient error)."""
    kind = case[0]
    mu, gt = loss_inputs(case, rows)
    mu = mu[0]
    want, grad = loss_reference(case, mu, gt)
    mud, gtd = mu.to(dev), gt.to(dev)
    loss = lib.loss_fwd(kind, mud, gtd).item()
    verr, worst = abs(loss - want), 0.0
    for up in UPSTREAM:
        dmu = lib.loss_bwd(kind, mud, gtd, torch.tensor(up, device=dev))
        assert dmu.shape == mu.shape
        if grad is None:
            assert int(torch.count_nonzero(dmu)) == 0, f"loss_bwd {case} rows={rows}: the evaluation-only degree error has a gradient"
            continue
        errs = [U.rel_err(dmu, up * grad)]
        if kind == "quaternion":                    # d mu scales with 1 / |mu|: the rows of each scale against their own largest entry
            errs += [U.rel_err(dmu.cpu()[k::3], up * grad[k::3]) for k in range(min(3, rows))]
        worst = max(worst, *errs)
    print(f"loss {ids(case)} rows={rows}: value {loss:.8g} want {want:.8g} |diff| {verr:.2e} (bound {value_bound(want):.2e}); gradient {worst:.2e} (bound {U.RTOL:.0e})")
    assert verr <= value_bound(want), f"loss_fwd {case} rows={rows}: {loss!r} against {want!r}"
    assert worst <= U.RTOL, f"loss_bwd {case} rows={rows}: rel err {worst:.2e}"
    return verr / value_bound(want), worst


def check_loss_prefix(lib, case, rows, P, dev):
    """Every entry of loss_prefix_fwd against float64 at value_bound, and with the bits of loss_fwd on its slice -> worst error / bound."""
    kind = case[0]
    mu, gt = loss_inputs(case, rows, P)
    mud, gtd = mu.to(dev), gt.to(dev)
    got = lib.loss_prefix_fwd(kind, mud, gtd)
    assert got.shape == (P,)
    worst = 0.0
    for p in range(P):
        want, _ = loss_reference(case, mu[p], gt)
        worst = max(worst, abs(got[p].item() - want) / value_bound(want))
        assert abs(got[p].item() - want) <= value_bound(want), f"loss_prefix_fwd {case} rows={rows} P={P}: entry {p} {got[p].item()!r} against {want!r}"
        assert bits_equal(got[p], lib.loss_fwd(kind, mud[p], gtd)), f"loss_prefix_fwd {case} rows={rows} P={P}: entry {p} differs from loss_fwd on the slice"
    print(f"loss_prefix {ids(case)} rows={rows} P={P}: worst |diff| / bound {worst:.2e}; every entry has loss_fwd's bits")
    return worst


def check_distractor_equal_row(lib, dev, rows=1025, equal_row=1024):
    """One row with mu == gt: sqrt(0) = 0 in the value; its gradient is 0 / 0 - NaN in torch's float64 autograd and NaN from the kernel.
    Every other row meets util.RTOL."""
    case = ("distractor", 2, 2)
    mu, gt = loss_inputs(case, rows, equal_row=equal_row)
    mu = mu[0]
    want, grad = loss_reference(case, mu, gt)
    loss = lib.loss_fwd("distractor", mu.to(dev), gt.to(dev)).item()
    assert math.isfinite(loss) and abs(loss - want) <= value_bound(want), (loss, want)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[equal_row] = False
    assert bool(grad[equal_row].isnan().all()) and bool(torch.isfinite(grad[keep]).all())
    for up in UPSTREAM:
        dmu = lib.loss_bwd("distractor", mu.to(dev), gt.to(dev), torch.tensor(up, device=dev)).cpu()
        assert bool(dmu[equal_row].isnan().all()), dmu[equal_row]
        e = U.rel_err(dmu[keep], up * grad[keep])
        print(f"loss distractor rows={rows} with row {equal_row} mu == gt: value |diff| {abs(loss - want):.2e}; the other rows' gradient {e:.2e}")
        assert e <= U.RTOL, e


PLUS_TRIPLES = [(1383162.5, 1e-7, 1.0), (3.0, 0.5, -2.25)]          # (kl, beta, upstream)


def check_loss_plus(lib, case, rows, dev):
    """loss_plus_fwd has the bits of loss_fwd followed by axpy, loss_plus_bwd those of loss_bwd and axpy(None, upstream, beta)."""
    kind = case[0]
    mu, gt = loss_inputs(case, rows)
    mud, gtd = mu[0].to(dev), gt.to(dev)
    for kl_v, beta, up_v in PLUS_TRIPLES:
        kl, up = torch.tensor(kl_v, device=dev), torch.tensor(up_v, device=dev)
        total = lib.loss_plus_fwd(kind, mud, gtd, kl, beta)
        assert bits_equal(total, lib.axpy(lib.loss_fwd(kind, mud, gtd), kl, beta)), (case, rows, kl_v, beta)
        dmu, dkl = lib.loss_plus_bwd(kind, mud, gtd, up, beta)
        assert bits_equal(dmu, lib.loss_bwd(kind, mud, gtd, up)) and bits_equal(dkl, lib.axpy(None, up, beta)), (case, rows, kl_v, beta)
        assert lib.loss_plus_bwd(kind, mud, gtd, up, beta, need_dx=False)[1] is None
    print(f"loss_plus {ids(case)} rows={rows}: total, d mu and d kl bit-equal to loss_fwd / loss_bwd + axpy")


# ---- loss refusals ----------------------------------------------------------------------------------------------------------
# (kind, rows, y_dim, gt_dim)
LOSS_REFUSED = [(1, 4, 9, 9, "y_dim = 9"), (1, 4, 0, 2, "y_dim = 0"), (1, 0, 2, 2, "rows = 0"), (5, 4, 2, 2, "kind = 5"), (1, 4, 2, 0, "gt_dim = 0")]


def check_loss_refusals(lib, dev):
    """All five entries return MLHOT_ERR_ARG, name themselves in mlhot_last_error and write nothing."""
    stream = _stream(dev)
    for kind, rows, y_dim, gt_dim, why in LOSS_REFUSED:
        mu, gt = torch.ones(2, 4, 9, device=dev), torch.ones(4, 9, device=dev)
        one = torch.ones((), device=dev)
        loss, total, dmu, dx = (torch.full(s, SENTINEL, device=dev) for s in ((2,), (2,), (2, 4, 9), (2,)))
        c = lib.c
        calls = {"loss_fwd": lambda: c.mlhot_loss_fwd(kind, _P(mu), _P(gt), rows, y_dim, gt_dim, _P(loss), stream),
                 "loss_bwd": lambda: c.mlhot_loss_bwd(kind, _P(mu), _P(gt), rows, y_dim, gt_dim, _P(one), _P(dmu), stream),
                 "loss_plus_fwd": lambda: c.mlhot_loss_plus_fwd(kind, _P(mu), _P(gt), rows, y_dim, gt_dim, _P(one), 0.5, _P(loss), _P(total), stream),
                 "loss_plus_bwd": lambda: c.mlhot_loss_plus_bwd(kind, _P(mu), _P(gt), rows, y_dim, gt_dim, _P(one), 0.5, _P(dmu), _P(dx), stream)}
        if dev != "cpu" or hasattr(c, "mlhot_loss_prefix_fwd"):         # the product must export it; the host flavour may lack it
            calls["loss_prefix_fwd"] = lambda: c.mlhot_loss_prefix_fwd(kind, _P(mu), _P(gt), 2, rows, y_dim, gt_dim, _P(loss), stream)
        for name, call in calls.items():
            rc = call()
            assert rc == ERR_ARG, (name, why, rc)
            assert name.encode() in c.mlhot_last_error(), (name, why, c.mlhot_last_error())
        _sync(dev)
        assert all(bool((t == SENTINEL).all()) for t in (loss, total, dmu, dx)), f"{why}: a refused call wrote something"
