"""The attention mass on the MI355X: mlhot_favor_query_mass_fwd / _long_mass_fwd / _paged_mass_fwd through
mlhot.ops.favor_query(mass=) on random kh / vh / qh, no encoder.  Cases: tests/attention_mass_cases.py; the documented fp32 order and
the float64 statement: tests/attention_mass_ref.py.  Run with -m gpu.

What "float64" is here.  The weighted mass is held to relative (Nq + 2) 2^-24 per element: Nq - 1 adds of non-negative terms, one
multiply and one divide rounding.  That bar counts the roundings of THIS reduction, so the reference is the float64 sum of
tw x w over the read-out's own fp32 weights w = S / D (mlhot.ops.favor_query(weights=True) on the same arguments) - the exact value
of what the kernel approximates.  S and D themselves (exp, the MFMA chains) carry the read-out's error against a float64 forward,
which tests/test_attention_readout_gpu.py holds to U.RTOL; the same bar is asserted here for the mass against the float64
definition from the inputs, so both statements are checked.

The keys entry (Nc <= 32) takes no lens: a ragged state's slots behind lens[t] are zero rows of F_k, and v is read there as
mlhot_favor_query_fwd reads it - poison goes into k alone, v is zero-filled.  The long and paged entries never read either."""
import functools

import pytest
import torch

from tests import attention_mass_cases as MC
from tests import attention_mass_ref as MR
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, H, D = MC.T, MC.H, MC.D
KEYS = {"cached": "favor_keys", "long": "favor_keys_long", "paged": "favor_keys_paged"}


def _dev(t):
    """[T, H, N, d] -> the kernels' [T, N, H, d] on the device."""
    return t.permute(0, 2, 1, 3).contiguous().to(DEV)


def _state(form, k, p, lens, cap=None):
    """The key state of `form` on k [T, H, Nc, d] (CPU), optionally kept in `cap` slots"""
    from mlhot import ops
    kd = _dev(k)
    if cap is not None and cap > kd.shape[1]:
        kd = torch.cat([kd, torch.full((T, cap - kd.shape[1], H, D), float("nan"), device=DEV)], dim=1)
        lens = lens if lens is not None else (k.shape[2],) * T
    state = getattr(ops, KEYS[form])(kd, p.to(DEV), lens=lens)
    assert state.route == form
    return state


def _v(form, v, lens, cap=None):
    vd = _dev(MC.poisoned(v, lens, 0.0 if form == "cached" else float("nan")))
    if cap is not None and cap > vd.shape[1]:
        vd = torch.cat([vd, torch.full((T, cap - vd.shape[1], H, D), 0.0 if form == "cached" else float("nan"), device=DEV)], dim=1)
    return vd


@functools.lru_cache(maxsize=None)
def _setup(form, Nc, m, lens):
    q, k, v, p, tw = MC.inputs(Nc, m)
    return _dev(q), _state(form, MC.poisoned(k, lens, float("nan")), p, lens), _v(form, v, lens), p.to(DEV), tw.to(DEV)


@pytest.mark.parametrize("form,Nc,m,lens", MC.CASES, ids=[MC.case_id(c) for c in MC.CASES])
def test_mass_per_case(gpulib, form, Nc, m, lens):
    """out bit-equal to the plain entry; tw None: mass bit-equal to fold32 of the read-out's w; tw given: within (Nq + 2) 2^-24 of
    float64 over the same weights and within U.RTOL of the float64 definition; invalid columns and zero references exactly 0;
    NaN in the invalid rows of k (and v: long, paged) reaches nothing."""
    from mlhot.ops import favor_query
    qd, state, vd, pd, tw = _setup(form, Nc, m, lens)
    q, k, _, p, tw_cpu = MC.inputs(Nc, m)
    invalid = ~MC.valid(lens, Nc)[:, None, :].expand(T, H, Nc)
    label = {"cached": "favor.querymass", "long": "favor.lquerymass", "paged": "favor.pquerymass"}[form]
    for Nq in MC.NQS:
        rows = qd[:, :Nq].contiguous()
        plain = favor_query(rows, state, vd, pd)
        out_w, w = favor_query(rows, state, vd, pd, weights=True)
        labels, (out, mass) = U.launch_labels(gpulib, lambda: favor_query(rows, state, vd, pd, mass=True))
        assert labels == [label, "favor.massfold"], labels
        assert mass.shape == (T, H, Nc) and mass.dtype == torch.float32 and mass.is_contiguous()
        assert bool(torch.isfinite(plain).all()) and torch.equal(out, plain) and torch.equal(out_w, plain), Nq
        want = MR.fold32(w)
        assert torch.equal(mass.cpu(), want), (Nq, float((mass.cpu() - want).abs().max()))
        assert bool((mass.cpu()[invalid] == 0.0).all())
        # the tile partials, unfolded
        out_t, part = favor_query(rows, state, vd, pd, mass="tiles")
        assert part.shape == (T, H, (Nq + 15) // 16, Nc) and torch.equal(out_t, plain)
        assert torch.equal(part.cpu(), torch.from_numpy(MR.tile_partials32(w)))
        assert torch.equal(gpulib.favor_mass_fold(part), mass)
        # weighted
        twq = tw[:, :Nq].contiguous()
        out2, wmass = favor_query(rows, state, vd, pd, mass=True, target_weight=twq)
        assert torch.equal(out2, plain)
        exact = MR.mass64_of(w.cpu(), tw_cpu[:, :Nq])
        got = wmass.cpu().double()
        rel = float(((got - exact).abs() / exact.clamp_min(1e-300)).max())
        defn = MR.mass64(q[:, :, :Nq], k, p, lens, tw_cpu[:, :Nq])
        line = (f"attention mass {MC.case_id((form, Nc, m, lens))} Nq={Nq}: weighted against float64 over the read-out's w {rel:.2e} "
                f"(bound {(Nq + 2) * 2.0 ** -24:.2e}), against the float64 definition {U.rel_err(wmass, defn):.2e} of its scale")
        print(line)
        assert bool((got[exact == 0.0] == 0.0).all()) and bool((got[invalid] == 0.0).all()), line
        assert bool(((got - exact).abs() <= (Nq + 2) * 2.0 ** -24 * exact).all()), line
        assert U.rel_err(wmass, defn) <= U.RTOL and U.rel_err(mass, MR.mass64(q[:, :, :Nq], k, p, lens)) <= U.RTOL, line
        assert torch.equal(wmass.cpu(), MR.fold32(w, tw_cpu[:, :Nq])), line            # the documented order, multiply and add apart
        if Nq == 16:                                                                  # a weight of exactly 0 on every target of task 0
            zero = twq.clone()
            zero[0] = 0.0
            assert bool((favor_query(rows, state, vd, pd, mass=True, target_weight=zero)[1][0] == 0.0).all())


@pytest.mark.parametrize("form,Nc,cap", [("long", 40, 200), ("paged", 40, 300), ("paged", 300, 600), ("paged", 513, 1100)])
def test_same_shots_at_another_capacity_give_the_same_bits(gpulib, form, Nc, cap):
    from mlhot.ops import favor_query
    m = 40
    q, k, v, p, tw = MC.inputs(Nc, m)
    qd, pd, twd = _dev(q), p.to(DEV), tw.to(DEV)
    lens = (Nc - 3, Nc)
    a = favor_query(qd, _state(form, MC.poisoned(k, lens, float("nan")), p, lens), _v(form, v, lens), pd, mass=True, target_weight=twd)
    b = favor_query(qd, _state(form, MC.poisoned(k, lens, float("nan")), p, lens, cap), _v(form, v, lens, cap), pd, mass=True, target_weight=twd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1][:, :, :Nc]) and bool((b[1][:, :, Nc:] == 0.0).all())


@pytest.mark.parametrize("Nc", [1, 31, 32, 33, 255, 256])
def test_smaller_states_give_the_smaller_forms_bits(gpulib, Nc):
    """A paged state of at most 256 slots gives the long entry's bits, a long state of at most 32 the keys entry's."""
    from mlhot.ops import favor_query
    m = 40
    q, k, v, p, tw = MC.inputs(Nc, m)
    qd, vd, pd, twd = _dev(q), _dev(v), p.to(DEV), tw.to(DEV)
    res = {form: favor_query(qd, _state(form, k, p, None), vd, pd, mass=True, target_weight=twd)
           for form in (("cached", "long", "paged") if Nc <= 32 else ("long", "paged"))}
    for form in res:
        assert torch.equal(res[form][0], res["long"][0]) and torch.equal(res[form][1], res["long"][1]), form


@pytest.mark.parametrize("form,Nc", [("cached", 31), ("long", 255), ("paged", 513)])
def test_chunked_calls_fold_to_the_single_calls_bits(gpulib, form, Nc):
    from mlhot.ops import favor_query
    m, lens = 40, (Nc - 1, min(MC.EDGE[form] + 1, Nc))
    qd, state, vd, pd, tw = _setup(form, Nc, m, lens)
    for weight in (None, tw):
        out, mass = favor_query(qd, state, vd, pd, mass=True, target_weight=weight)
        for chunk in (16, 32):
            res = [favor_query(qd[:, i:i + chunk].contiguous(), state, vd, pd, mass="tiles",
                               target_weight=None if weight is None else weight[:, i:i + chunk].contiguous()) for i in range(0, MC.NQ, chunk)]
            assert torch.equal(torch.cat([r[0] for r in res], dim=1), out)
            assert torch.equal(gpulib.favor_mass_fold(torch.cat([r[1] for r in res], dim=2)), mass), (chunk, weight is None)


def test_unsupported_shapes_write_nothing(gpulib):
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    q, v, proj = torch.zeros(1, 4, 2, 16, device=DEV), torch.zeros(1, 40, 2, 16, device=DEV), torch.zeros(16, 16, device=DEV)
    state, ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    out, mass = torch.full((1, 4, 32), 7.0, device=DEV), torch.full((1, 2, 40), 7.0, device=DEV)
    rc = gpulib.c.mlhot_favor_query_mass_fwd(p(q), p(state), p(v), p(proj), None, 1, 2, 4, 40, 16, 16, p(out), p(mass), 1, p(ws), ws.numel(), None)
    assert rc != 0 and b"Nc <= 32" in gpulib.c.mlhot_last_error()                  # MLHOT_ERR_UNSUPPORTED
    rc = gpulib.c.mlhot_favor_query_long_mass_fwd(p(q), p(state), p(v), p(proj), None, None, 1, 2, 4, 40, 16, 16, p(out), None, 1, p(ws), ws.numel(), None)
    assert rc != 0 and b"bad argument" in gpulib.c.mlhot_last_error()
    rc = gpulib.c.mlhot_favor_query_long_mass_fwd(p(q), p(state), p(v), p(proj), None, None, 1, 2, 4, 40, 16, 16, p(out), p(mass), 1, p(ws), 256, None)
    assert rc != 0 and b"workspace too small" in gpulib.c.mlhot_last_error()
    assert gpulib.favor_query_mass_bytes(1, 2, 4, 40, 16, 16) == 512               # 1 * 2 * 1 * 40 floats = 320 bytes, in blocks of 256
    assert gpulib.favor_query_mass_bytes(1, 2, 4, 5000, 16, 16) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mass == 7.0).all())


def test_peak_memory_stays_far_below_w(gpulib):
    """T = 2, H = 8, Nq = 512, Nc = 4096, d = m = 16: w would be 128 MiB; the call's peak over what was allocated before it stays
    below a quarter of that (the tile partials are 8 MiB, out and mass less than 1 MiB)."""
    from mlhot.ops import favor_keys_paged, favor_query
    Tn, Hn, Nq, Nc, d, m = 2, 8, 512, 4096, 16, 16
    g = torch.Generator().manual_seed(11)
    qd = (0.5 * torch.randn(Tn, Nq, Hn, d, generator=g)).to(DEV)
    kd = (0.5 * torch.randn(Tn, Nc, Hn, d, generator=g)).to(DEV)
    vd = torch.randn(Tn, Nc, Hn, d, generator=g).to(DEV)
    pd = MC.proj(m).to(DEV)
    state = favor_keys_paged(kd, pd)
    assert gpulib.favor_query_mass_bytes(Tn, Hn, Nq, Nc, d, m) == Tn * Hn * (Nq // 16) * Nc * 4
    w_bytes = Tn * Hn * Nq * Nc * 4
    assert w_bytes == 128 << 20
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, mass = favor_query(qd, state, vd, pd, mass=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"attention mass memory: peak over the call {peak / 2 ** 20:.1f} MiB, w would be {w_bytes / 2 ** 20:.0f} MiB")
    # max_memory_allocated in a process of its own: the operands plus the call's peak (other modules' cached tensors left out)
    operands = sum(t.numel() * t.element_size() for t in (qd, kd, vd, pd, state.buf))
    assert operands + peak < w_bytes // 4
    s = mass.double().sum(dim=-1)                                                # rows of w sum to 1: the mass sums to Nq
    assert bool(torch.isfinite(out).all()) and float((s - Nq).abs().max()) <= Nq * Nc * 2.0 ** -23
