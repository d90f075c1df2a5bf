"""The paged per-shot key state without a GPU: the float64 references the GPU tests use against a dense FAVOR+
written here independently, pack_mask above 256 slots, the host build's entries, and every host-side refusal of form="paged" (all
raised before anything touches a GPU)."""
import ctypes as C
import importlib
import types

import pytest
import torch

from tests import context_mask_ref as CM
from tests import favor_long_ref as LR
from tests import favor_paged_cases as PC
from tests import util as U

CFGV = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
            n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
             tasks_per_batch=2)
MODELS = {
    "resnet_anp": ("ANP", dict(CFG3D, agg_mode="attention"), (3, 64, 64), 4),
    "resnet_cnp_max": ("CondNeuralProcess", dict(CFG3D, agg_mode="max"), (3, 64, 64), 4),
    "vanilla_anp": ("ANPShapeNet1D", dict(CFGV, agg_mode="attention", dim_r=64), (1, 128, 128), 3),
    "vanilla_cnp_mean": ("CNPShapeNet1D", dict(CFGV, agg_mode="mean", dim_r=100), (1, 128, 128), 3),
}
TOL = 1e-12


# ---- the references against a dense statement written here ------------------------------------------------------------------------------
def _dense(q, k, v, proj, lens, mask=None):
    """FAVOR+ without a softmax, in one piece and in float64: phi(x) = m^-1/2 (exp(c x P^T - c^2 |x|^2 / 2 - stab) + 1e-4), the key
    stabiliser the maximum over the valid keys of the batch, the query's its own row's; w = phi(q) phi(k)^T over the kept valid
    slots, normalised per row; out = w v.  mask bool [T, Nq, Nc] or None."""
    T, Hn, Nc, d = k.shape
    m = proj.shape[0]
    q, k, v, P = q.double(), k.double(), v.double(), proj.double()
    valid = torch.arange(Nc)[None, :] < torch.tensor(lens)[:, None]                     # [T, Nc]
    c = d ** -0.25
    k = torch.where(valid[:, None, :, None], k, torch.zeros((), dtype=torch.float64))
    v = torch.where(valid[:, None, :, None], v, torch.zeros((), dtype=torch.float64))
    xk, xq = c * k @ P.T, c * q @ P.T
    stab = xk[valid[:, None, :].expand(T, Hn, Nc)].max()
    fk = (torch.exp(xk - 0.5 * c * c * (k * k).sum(-1, keepdim=True) - stab) + 1e-4) / m ** 0.5
    fq = (torch.exp(xq - 0.5 * c * c * (q * q).sum(-1, keepdim=True) - xq.max(dim=-1, keepdim=True).values) + 1e-4) / m ** 0.5
    keep = valid[:, None, None, :] if mask is None else (mask & valid[:, None, :])[:, None]
    S = (fq @ fk.transpose(-1, -2)) * keep
    w = S / S.sum(-1, keepdim=True)
    return w @ v, w


@pytest.mark.parametrize("Nc", [257, 513])
@pytest.mark.parametrize("d,m", PC.DM)
def test_the_references_are_the_dense_statement(d, m, Nc):
    for kind in PC.KINDS:
        q, k, v, p = PC.inputs(kind, d, m, Nc)
        w64, out64 = PC.want(kind, d, m, Nc)
        out, w = _dense(q, k, v, p, (Nc,) * PC.T)
        sout, sw = LR.stream(q, k, v, p)                                # the chunked walk, general in Nc
        eo, ew = U.rel_err(out64, out), U.rel_err(w64, w)
        print(f"paged references {kind} d={d} m={m} Nc={Nc}: out {eo:.2e}, w {ew:.2e} of their scales against the dense statement")
        assert eo <= TOL and ew <= TOL and U.rel_err(sout, out) <= TOL and U.rel_err(sw, w) <= TOL
    for lens in PC.ragged_lens(Nc):
        q, kn, vp, p, w64, out64, fk64, M64 = PC.ragged("live", d, m, Nc, lens)
        out, w = _dense(q, torch.nan_to_num(kn), vp, p, lens)
        assert U.rel_err(out64, out) <= TOL and U.rel_err(w64, w) <= TOL
        for t, L in enumerate(lens):
            assert not w64[t, :, :, L:].any() and not fk64[t, :, L:].any()


@pytest.mark.parametrize("Nc", PC.MASK_NCS)
def test_the_masked_reference_is_the_dense_statement(Nc):
    d, m = 64, 266
    q, k, v, p = PC.mask_inputs(Nc, d, m)
    for pattern in ("page", "tail"):
        mk, out64, w64 = PC.mask_want(Nc, d, m, pattern)
        for g in range(mk.shape[1]):
            out, w = _dense(q, k, v, p, PC.mask_lens(Nc), mk[:, g])
            assert bool(torch.isfinite(w).all())                        # these patterns leave no row empty
            assert U.rel_err(out64[:, g], out) <= TOL and U.rel_err(w64[:, g], w) <= TOL, (pattern, g)


def test_the_dominant_shot_holds_nearly_all_the_weight():
    q, k, v, p, mk, out64, w64, full = PC.dominant()
    slot = PC.DOMINANT["slot"]
    print(f"dominant shot {slot} of {PC.DOMINANT['Nc']}: its weight is at least {float(full[..., slot].min()):.4f}")
    assert float(full[..., slot].min()) > 0.9
    assert not w64[:, 0, ..., slot].any() and float(w64[:, 1, ..., slot].min()) > 0.9
    out, w = _dense(q, k, v, p, (PC.DOMINANT["Nc"],) * PC.T, mk[:, 0])
    assert U.rel_err(out64[:, 0], out) <= TOL and U.rel_err(w64[:, 0], w) <= TOL


# ---- pack_mask above 256 slots ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", [257, 512, 513])
def test_pack_mask_round_trips_above_256_slots(Nc):
    from mlhot.ragged import pack_mask
    mk = torch.rand(2, 3, 5, Nc, generator=torch.Generator().manual_seed(Nc)) < 0.5
    mk[0, 0, 0], mk[1, 2, 4] = True, False
    mk[0, 1, 1, Nc - 1], mk[0, 1, 2, 256], mk[0, 1, 3, 255] = True, True, True
    words = pack_mask(mk, Nc)
    W = (Nc + 31) // 32
    assert words.shape == (2, 3, 5, W) and words.dtype == torch.int32 and words.is_contiguous()
    bits = (words.to(torch.int64)[..., None] >> torch.arange(32)) & 1                   # [.., W, 32]
    back = bits.reshape(2, 3, 5, 32 * W).bool()
    assert torch.equal(back[..., :Nc], mk) and not bool(back[..., Nc:].any())
    assert torch.equal(pack_mask(mk[:, 1], Nc), words[:, 1:2])


# ---- the host build -------------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_entries_and_they_are_unsupported(hostsim):
    c = hostsim.c
    assert c.mlhot_favor_paged_supported(2, 2, 300, 64, 266) == 0
    assert c.mlhot_favor_keys_paged_bytes(2, 2, 300, 64, 266) == 0
    assert c.mlhot_favor_query_paged_bytes(2, 2, 5, 300, 64, 266, 0) == 0 and c.mlhot_favor_query_paged_bytes(2, 2, 5, 300, 64, 266, 3) == 0
    buf = torch.full((1024,), 7.0)
    p = C.c_void_p(buf.data_ptr())
    calls = {
        "favor_keys_paged_fwd": lambda: c.mlhot_favor_keys_paged_fwd(p, p, None, 2, 2, 300, 64, 266, p, 4096, None),
        "favor_query_paged_fwd": lambda: c.mlhot_favor_query_paged_fwd(p, p, p, p, None, 2, 2, 5, 300, 64, 266, p, p, p, 4096, None),
        "favor_query_paged_masked_fwd": lambda: c.mlhot_favor_query_paged_masked_fwd(p, p, p, p, None, p, 2, 2, 2, 5, 300, 64, 266, p, p, p, 4096, None),
    }
    for name, call in calls.items():
        assert call() == 4, name                                    # MLHOT_ERR_UNSUPPORTED
        msg = c.mlhot_last_error().decode()
        assert name in msg and "Nc=300" in msg and "d=64" in msg and "m=266" in msg, (name, msg)
    assert bool((buf == 7.0).all())
    from mlhot.binding import MlhotError
    assert not hostsim.favor_paged_supported(2, 2, 300, 64, 266)
    with pytest.raises(MlhotError, match="favor_keys_paged_fwd serves"):              # the wrapper refuses before it allocates
        hostsim.favor_keys_paged_fwd(torch.zeros(2, 300, 2, 64), torch.zeros(266, 64))


# ---- host-side refusals -------------------------------------------------------------------------------------------------------------
def _model(name):
    method, cfg, img, L = MODELS[name]
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval(), img, L


def _images(n, img, L):
    return torch.rand(2, 1, 1, 1, 1).expand(2, n, *img), torch.rand(2, n, L)


@pytest.mark.parametrize("name", list(MODELS))
def test_condition_refusals_of_the_paged_form(name):
    from mlhot import cached, ragged
    assert "paged" in ragged.FORMS and ragged.MAX_PAGED_CAPACITY == 4096
    assert ragged.MAX_LONG_CAPACITY == 256 and ragged.MAX_ATTENTION_CAPACITY == 32              # the other forms keep their caps
    model, img, L = _model(name)
    cx, cy = _images(4, img, L)
    assert cached.supports(model)[0]
    entries = [lambda *a, **kw: cached.condition(model, *a, **kw)] + ([lambda *a, **kw: model.condition(*a, **kw)] if hasattr(model, "extend") else [])
    for cond in entries:
        if not model.ATTENTION:
            with pytest.raises(ValueError, match='form="paged" serves the attention models'):          # a latent model
                cond(cx, cy, form="paged")
            continue
        with pytest.raises(ValueError, match="capacity = 4097 is outside the paged attention kernels' envelope.*at most 4096"):
            cond(cx, cy, form="paged", capacity=4097)
        with pytest.raises(ValueError, match="capacity = 3 is smaller than the 4 context slots"):
            cond(cx, cy, form="paged", capacity=3)
        with pytest.raises(ValueError, match="capacity must be an integer"):
            cond(cx, cy, form="paged", capacity=300.0)
        for bad in ([0, 4], [1, 5]):
            with pytest.raises(ValueError, match=r"ctx_len must lie in 1\.\.4"):
                cond(cx, cy, form="paged", ctx_len=bad)
        with pytest.raises(ValueError, match="capacity = 257 is outside the long attention kernels' envelope"):
            cond(cx, cy, form="long", capacity=257)                                                   # "long" keeps its cap
    if model.ATTENTION:
        with pytest.raises(ValueError, match="capacity = 4097 is outside the paged"):                 # ... also as the default capacity
            cached.condition(model, *_images(4097, img, L), form="paged")
        with pytest.raises(ValueError, match="at least one context shot"):
            cached.condition(model, cx[:, :0], cy[:, :0], form="paged")
        model.train()
        with pytest.raises(ValueError, match="eval"):
            cached.condition(model, cx, cy, form="paged")


def _paged_state(model, lens=(300, 257), cap=320):
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    from networks._resnet_np import ResNetNP
    d = 256 if isinstance(model, ResNetNP) else 64
    keys = FavorKeyState("paged", (2, cap, 8, d, model.attn.projection_matrix.shape[0]), buf=None, lens=tuple(lens))
    rows = torch.zeros(2, cap, 8, d)
    return ContextState(model, 2, cap, fingerprint(model), "attention", keys=keys, vh=rows, kh=rows, lens=lens, form="paged")


@pytest.mark.parametrize("name", ["resnet_anp", "vanilla_anp"])
def test_extend_merge_select_and_route_refusals_on_a_paged_state(name):
    from mlhot import cached
    model, img, L = _model(name)
    state = _paged_state(model)
    assert state.capacity == 320 and state.form == "paged" and state.lens == (300, 257)
    (nx, ny), qx = _images(30, img, L), torch.rand(2, 3, *img)
    with pytest.raises(ValueError, match="task 0 would hold 330 context shots, the state's capacity is 320"):
        cached.extend(model, state, nx, ny)
    with pytest.raises(ValueError, match=r"new_len must lie in 0\.\.30"):
        cached.extend(model, state, nx, ny, new_len=[31, 0])
    with pytest.raises(ValueError, match=r"merge: states\[0\] has form 'paged'.*per-shot rows in at most 4096 slots"):
        cached.merge(model, [state])
    with pytest.raises(ValueError, match=r"select: states\[0\] has form 'paged'.*per-shot rows in at most 4096 slots"):
        cached.select(model, [state], [(0, 0), (0, 1)])
    if name == "vanilla_anp":
        with pytest.raises(ValueError, match='route "fused".*a paged state'):
            cached.predict(model, state, qx, route="fused")
        with pytest.raises(ValueError, match='route "fused_summary" reads a FAVOR\\+ summary state.*\'paged\'.*route "composed"'):
            cached.predict(model, state, qx, route="fused_summary")
        with pytest.raises(ValueError, match='route "fused"'):
            cached.predict(model, state, qx, route="fused", return_attention=True)
        ones = torch.ones(2, 3, 320, dtype=torch.bool)
        for route in ("fused", "fused_summary"):
            with pytest.raises(ValueError, match=f'context_mask= with route "{route}"'):
                cached.predict(model, state, qx, route=route, context_mask=ones)
    else:
        with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
            cached.predict(model, state, qx, route="fused")
    with pytest.raises(ValueError, match="keeps none of the 257 valid context shots of task 1 for target 2"):
        mk = torch.ones(2, 3, 320, dtype=torch.bool)
        mk[1, 2, :257] = False
        cached.predict(model, state, qx, context_mask=mk)
    other, _, _ = _model(name)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(other, state, qx, return_attention=True)


def test_ops_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ops import MAX_PAGED_NC, FavorKeyState, favor_gather, favor_keys_paged, favor_merge
    assert MAX_PAGED_NC == 4096
    k, proj = torch.zeros(2, 300, 2, 16), torch.zeros(16, 16)
    with pytest.raises(MlhotError, match="needs tensors on a ROCm device"):
        favor_keys_paged(k, proj)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_keys_paged(k.clone().requires_grad_(), proj)
    paged = FavorKeyState("paged", (2, 300, 2, 16, 16), buf=torch.zeros(8, dtype=torch.uint8), lens=(300, 3))
    with pytest.raises(MlhotError, match=r"favor_merge: states\[0\] has route 'paged'"):
        favor_merge([paged])
    with pytest.raises(ValueError, match=r"favor_gather: states\[0\] has route 'paged'.*hold rows, not sums"):
        favor_gather([paged], [[(0, 0)]])
    with pytest.raises(MlhotError, match="no summary"):
        paged.summary()


def test_linear_rows_any_needs_a_gpu_and_no_gradient():
    from mlhot.binding import MlhotError
    from mlhot.ops import linear_rows_any
    x, w, b = torch.zeros(5, 3), torch.zeros(16, 3), torch.zeros(16)
    with pytest.raises(MlhotError):
        linear_rows_any([(x, 1, 0)], w, b)
