"""Shared by tests/test_ntx_cases_cpu.py and tests/test_ntx_envelope_gpu.py: the case table that walks the envelope of the NT-Xent
kernels (csrc/nt_xent.h: 1 <= N <= 2048 rows, d % 16 == 0 up to 256, label(i) = (i // div) % mod, t > 0, any upstream gradient) and the
float64 reference every case is judged by.  No GPU and no project import: torch only.

The reference is the definition in the header comment of nt_xent.h as float64 tensor arithmetic (ref below; tests/test_ntx_cases_cpu.py
holds it against oracle.ref_cpu.nt_xent, the pair-by-pair restatement, on every case of at most 65 rows).  The float32 inputs are the
master copy: the float64 run converts those very float32 values.

What the kernels do with d (the table's reason for its d values): the backward's dzn = H' z product gives wave w of 4 the columns
[64 w, 64 w + 64) and lane (lr, lq) of it the four columns 64 w + 4 lr ..; when d % 64 != 0 the last wave that has columns has
(d % 64) / 4 lanes per quarter inside d and the rest outside.  partial_block() names the part of dz that the lanes outside touch if the
matrix instruction is issued under a per-lane mask: columns >= 64 floor(d / 64) of the tile rows >= (d % 64) / 4 of every 16-anchor
tile; defect_model() is that defect in float64."""
import functools
import types
import zlib

import torch

TINY = float(torch.finfo(torch.float32).tiny)
NORM_FLOOR = 1e-12
LOSS_RTOL = 1e-6          # the bar of test_nt_xent_kernel_vs_definition, times max(1, 0.07 / t): see loss_bound
STAT_RTOL = 1e-5          # rinv, negmax, E and W of the workspace against the reference's
INT_MAX = 2 ** 31 - 1


def _case(name, N, d, div, mod, t=0.07, gscale=1.0, recipe="randn", zero=False, bits_of=None, note=""):
    """recipe: how z is drawn (inputs); zero: loss and gradient are exactly 0 (no positives or no negatives); bits_of: the name of a
    case with the same labels whose loss and dz this case must equal bit for bit."""
    return types.SimpleNamespace(name=name, N=N, d=d, div=div, mod=mod, t=t, gscale=gscale, recipe=recipe, zero=zero, bits_of=bits_of, note=note)


def _table():
    c = []
    # ---- d sweep: three 16-anchor tiles, the last one partial; every d % 64 in {0, 16, 32, 48} below and above one full block ----
    for d in (16, 32, 48, 64, 80, 112, 128, 144, 192, 208, 240, 256):
        c.append(_case(f"d{d}_N37", 37, d, 1, 5))
    for d in (16, 80, 240):
        c.append(_case(f"d{d}_N16", 16, d, 1, 5, note="exactly one tile"))
        c.append(_case(f"d{d}_N17", 17, d, 1, 5, note="one row into the second tile"))
    # ---- N edges at d = 80, labels i % 2 ----
    c.append(_case("N2_mod1_exact_zero", 2, 80, 1, 1, zero=True, note="one group: no negatives"))
    c.append(_case("N2_mod2_exact_zero", 2, 80, 1, 2, zero=True, note="two groups of one: no positives"))
    for N in (3, 15, 16, 17, 31, 32, 33, 64, 65):
        c.append(_case(f"N{N}_d80_mod2", N, 80, 1, 2))
    # ---- label structures at d = 48 ----
    c.append(_case("lab_pairs", 44, 48, 1, 22, note="contrastive_loss: label = row % T, N = 2 T"))
    c.append(_case("lab_pairs_one_unpaired", 45, 48, 1, 23, note="label = row % 23: row 22 has no positive"))
    c.append(_case("lab_blocks", 45, 48, 5, 9, note="contrastive_loss_ANP: label = row // Nq"))
    c.append(_case("lab_blocks_incomplete", 45, 48, 7, 7, note="six groups of 7 and one of 3"))
    c.append(_case("lab_wrap", 45, 48, 2, 4, note="labels wrap: a label's rows are not contiguous"))
    c.append(_case("lab_unequal", 45, 48, 10, 3, note="groups of 20, 15 and 10 rows"))
    c.append(_case("lab_all_but_one", 45, 48, 44, 2, note="one group of 44 rows, one row alone: one negative per anchor"))
    c.append(_case("lab_mod_N", 45, 48, 5, 45, note="mod = N: the labels of lab_blocks"))
    c.append(_case("lab_mod_N_plus_7", 45, 48, 5, 52, bits_of="lab_mod_N"))
    c.append(_case("lab_mod_int_max", 45, 48, 5, INT_MAX, bits_of="lab_mod_N", note="pair_count counts with min(mod, N) buckets"))
    # ---- temperature ----
    for d in (80, 128):
        for t in (0.01, 0.07, 0.5, 5.0):
            c.append(_case(f"t{t}_d{d}", 37, d, 1, 5, t=t))
    # ---- upstream gradient ----
    for gs in (0.0, 1.0, -2.5, 1e-3):
        c.append(_case(f"gscale{gs}_d80", 37, 80, 1, 5, gscale=gs))
    # ---- the LDS limit: 16 (d + 4) + 16 (N16 + 4) + N16 + 64 floats ----
    c.append(_case("lds_2048_256", 2048, 256, 64, 32, note="156416 bytes: the largest launch"))
    c.append(_case("lds_2033_240", 2033, 240, 19, 107, note="partial row tile and partial column block at the limit"))
    # ---- degenerate rows at (33, 80), labels i % 3; DEGENERATE_ROW sits in the part of a tile that partial_block() names ----
    for r in ("zero_row", "tiny_row", "twins_other_label", "twins_same_label", "six_decades"):
        c.append(_case(f"deg_{r}", 33, 80, 1, 3, recipe=r))
    return c


CASES = _table()
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SMALL = [c for c in CASES if c.N <= 65]
GSCALE_CASES = [c for c in CASES if c.name.startswith("gscale")]
DEGENERATE_ROW = 21           # tile row 5 of the second tile
TWIN_ROWS = {"twins_other_label": (21, 25), "twins_same_label": (21, 27)}        # labels i % 3: 0 and 1; 0 and 0


def labels(c):
    return (torch.arange(c.N) // c.div) % c.mod


def inputs(name):
    """float32 z [N, d]; callers must not write into it."""
    return _inputs(name).clone()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.N},{c.d},{c.recipe}".encode()))      # cases of one shape share their z
    z = torch.randn(c.N, c.d, generator=g) * (1.0 + torch.rand(c.N, 1, generator=g))
    if c.recipe == "zero_row":
        z[DEGENERATE_ROW] = 0.0
    elif c.recipe == "tiny_row":
        z[DEGENERATE_ROW] *= 1e-20                 # |z| ~ 1e-19 < 1e-12: the norm's clamp is active
    elif c.recipe in TWIN_ROWS:
        a, b = TWIN_ROWS[c.recipe]
        z[b] = z[a]
    elif c.recipe == "six_decades":
        z *= 10.0 ** ((torch.arange(c.N) * 7 % 13).float() / 2.0 - 3.0)[:, None]          # 1e-3 .. 1e3, mixed over the tile rows
    else:
        assert c.recipe == "randn", c.recipe
    return z


def special_rows(c):
    """Rows whose gradient is 1e12 x everyone else's (rinv = 1 / 1e-12): judged on their own."""
    return [DEGENERATE_ROW] if c.recipe in ("zero_row", "tiny_row") else []


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
def _loss_of_zn(zn, lab, t):
    """The definition on unit rows zn (float64): (loss, statistics).  Per anchor the negatives' maximum and exp-sum, per positive
    pair m = max(s_ap, negmax_a) as a constant, -log(e^{s_ap - m} / (e^{s_ap - m} + sum_n e^{s_an - m}) + tiny), mean over the positive
    pairs of the anchors that have a negative."""
    N = zn.shape[0]
    sim = zn @ zn.t() / t
    same = lab[:, None] == lab[None, :]
    has_neg = ~same.all(dim=1)
    pos = same & ~torch.eye(N, dtype=torch.bool) & has_neg[:, None]
    negmax = sim.detach().masked_fill(same, float("-inf")).max(dim=1).values
    nm = torch.where(has_neg, negmax, torch.zeros_like(negmax))[:, None]              # finite stand-in where nothing is summed
    m = torch.maximum(sim.detach(), nm)
    num = torch.exp(sim - m)
    # sum_n exp(s_an - m_ap) = E_a exp(negmax_a - m_ap), E_a = sum_n exp(s_an - negmax_a)   (O(N^2) instead of O(N^3))
    E = (torch.exp(sim - nm) * ~same).sum(dim=1)
    den = E[:, None] * torch.exp(nm - m) + num
    q = num / den
    per = -torch.log(q + TINY)
    pairs = int(pos.sum())
    loss = per[pos].sum() / pairs if pairs else zn.sum() * 0.0
    W = ((q / (q + TINY) * torch.exp(nm - m) / den) * pos).sum(dim=1)
    return loss, types.SimpleNamespace(negmax=negmax, E=E.detach(), W=W.detach(), has_neg=has_neg, pairs=pairs)


def ref(z64, div, mod, t, gscale):
    """-> (loss, dz) in float64: the NT-Xent of z64 [N, d] under label(i) = (i // div) % mod and gscale x its gradient."""
    z = z64.detach().clone().requires_grad_()
    lab = (torch.arange(z.shape[0]) // div) % mod
    zn = z / z.norm(dim=1, keepdim=True).clamp_min(NORM_FLOOR)
    loss, _ = _loss_of_zn(zn, lab, t)
    (loss * gscale).backward()
    return loss.detach(), z.grad


def _norm_backward(z, rinv, dzn):
    """dz_i = rinv_i (dzn_i - zn_i (zn_i . dzn_i)), the kernels' form (for a clamped row zn is ~ 0 and the second term vanishes)."""
    zn = z * rinv
    return rinv * (dzn - zn * (zn * dzn).sum(dim=1, keepdim=True))


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    z = inputs(name).double()
    loss, dz = ref(z, c.div, c.mod, c.t, c.gscale)
    rinv = 1.0 / z.norm(dim=1, keepdim=True).clamp_min(NORM_FLOOR)
    zn = (z * rinv).requires_grad_()
    l2, st = _loss_of_zn(zn, labels(c), c.t)
    (l2 * c.gscale).backward()
    return types.SimpleNamespace(loss=loss, dz=dz, dzn=zn.grad, rinv=rinv[:, 0], negmax=st.negmax, E=st.E, W=st.W, has_neg=st.has_neg, pairs=st.pairs)


def reference(c):
    """loss, dz (gscale applied), dzn = gscale dL/dzn, and the forward's saved statistics rinv, negmax, E, W - float64, computed once
    per case; callers must not write into them."""
    return _reference(c.name)


# ---- judging -----------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    """tests/util.py::rel_err (max |a - b| / max |b|), restated: this file imports torch alone."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def dz_err(c, got, want):
    """Worst tensor-scale error of dz: the zero / 1e-20 rows each against their own row maximum, the remaining rows against the
    maximum over those (a row with rinv = 1e12 would otherwise set the scale and hide every other row)."""
    sp = special_rows(c)
    rest = [i for i in range(c.N) if i not in sp]
    return max([rel_err(got[rest], want[rest])] + [rel_err(got[i], want[i]) for i in sp])


def loss_bound(c, want):
    """|loss - ref| may be 1e-6 max(1, 0.07 / t) max(1, |ref|): the fp32 error of s = cos / t grows as 1 / t, and |dL/ds| <= 1."""
    return LOSS_RTOL * max(1.0, 0.07 / c.t) * max(1.0, abs(float(want)))


# ---- the partial column block -------------------------------------------------------------------------------------------------
def partial_block(c):
    """(row mask [N], first column) of the part of dz that the lanes outside d of the last column block carry operands for, or None
    when d % 64 == 0 or no row of the case sits there (N <= (d % 64) / 4)."""
    if c.d % 64 == 0:
        return None
    rows = (torch.arange(c.N) % 16) >= (c.d % 64) // 4
    return (rows, 64 * (c.d // 64)) if bool(rows.any()) else None


def defect_model(c):
    """dz as a backward would give it whose matrix product for the partial column block loses the A rows (anchors) of the lanes outside
    d: dzn is zero on partial_block(), then the normalisation's backward (whose row dot product sees the zeros too).  float64."""
    r, pb = reference(c), partial_block(c)
    dzn = r.dzn.clone()
    if pb is not None:
        rows, c0 = pb
        dzn[rows, c0:] = 0.0
    return _norm_backward(inputs(c.name).double(), r.rinv[:, None], dzn)
