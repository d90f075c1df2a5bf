"""The long per-shot key state without a GPU: the float64 restatement of the chunked stream
(tests/favor_long_ref.py) against tests/favor_cached_ref.py and tests/attention_readout_ref.py on every input the GPU tests use, the
host build's four entries, and every host-side refusal of form="long" (all raised before anything touches a GPU)."""
import ctypes as C
import importlib
import types

import pytest
import torch

from tests import favor_long_cases as LC
from tests import favor_long_ref as LR
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


# ---- the chunked stream against the one-piece statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,m,Nc", LC.cases())
def test_the_chunked_stream_is_the_attention_and_its_weights(kind, d, m, Nc):
    q, k, v, p = LC.inputs(kind, d, m, Nc)
    w64, out64 = LC.want(kind, d, m, Nc)
    out, w = LR.stream(q, k, v, p)
    eo, ew = U.rel_err(out, out64), U.rel_err(w, w64)
    print(f"chunked stream {kind} d={d} m={m} Nc={Nc}: out {eo:.2e}, w {ew:.2e} of their scales")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all())
    assert eo <= TOL and ew <= TOL


@pytest.mark.parametrize("Nc", LC.RAGGED_NCS)
@pytest.mark.parametrize("d,m", LC.DM)
def test_the_masked_stream_selects_by_index(d, m, Nc):
    for lens in LC.ragged_lens(Nc):
        q, kn, vp, p, w64, out64, fk64, M64 = LC.ragged("live", d, m, Nc, lens)
        assert bool(torch.isnan(kn).any()) and float(vp.abs().max()) > 9e29       # the poison is there
        fk, M = LR.key_features(kn, p, lens)
        out, w = LR.stream(q, kn, vp, p, lens)
        assert bool(torch.isfinite(fk).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(w).all())
        for t, L in enumerate(lens):
            assert not fk[t, :, L:].any() and not w[t, :, :, L:].any() and float(w[t, :, :, :L].min()) > 0.0
        assert abs(float(M - M64)) <= TOL * max(1.0, abs(float(M64)))
        assert U.rel_err(fk, fk64) <= TOL and U.rel_err(out, out64) <= TOL and U.rel_err(w, w64) <= TOL


@pytest.mark.parametrize("Nc", LC.TIE_NCS)
def test_one_chunk_is_the_cached_statement(Nc):
    d, m = 64, 266
    q, k, v, p = LC.inputs("live", d, m, Nc)
    w64, out64 = LC.want("live", d, m, Nc)
    out, w = LR.stream(q, k, v, p)
    assert U.rel_err(out, out64) <= TOL and U.rel_err(w, w64) <= TOL


def test_the_peak_of_the_tie_case_sits_in_the_first_chunk():
    for d, m in LC.DM:
        q, k, v, p = LC.peak_first(d, m)
        full, M = LR.key_features(k, p)
        first, M32 = LR.key_features(k[:, :, :32], p)
        assert float(M) == float(M32) and torch.equal(full[:, :, :32], first)


# ---- the host build -----------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_four_entries_and_they_are_unsupported(hostsim):
    c = hostsim.c
    assert c.mlhot_favor_long_supported(2, 2, 64, 64, 266) == 0
    assert c.mlhot_favor_keys_long_bytes(2, 2, 64, 64, 266) == 0
    buf = torch.full((1024,), 7.0)
    p = C.c_void_p(buf.data_ptr())
    calls = {
        "favor_keys_long_fwd": lambda: c.mlhot_favor_keys_long_fwd(p, p, None, 2, 2, 64, 64, 266, p, 4096, None),
        "favor_query_long_fwd": lambda: c.mlhot_favor_query_long_fwd(p, p, p, p, None, 2, 2, 5, 64, 64, 266, p, p, p, 4096, None),
    }
    for name, call in calls.items():
        assert call() == 4, name                                    # MLHOT_ERR_UNSUPPORTED
        assert name in c.mlhot_last_error().decode(), (name, c.mlhot_last_error().decode())
    assert bool((buf == 7.0).all())
    from mlhot.binding import MlhotError
    assert not hostsim.favor_long_supported(2, 2, 64, 64, 266)
    with pytest.raises(MlhotError, match="favor_keys_long_fwd serves"):             # the wrapper refuses before it allocates
        hostsim.favor_keys_long_fwd(torch.zeros(2, 64, 2, 64), torch.zeros(266, 64))


# ---- host-side refusals -------------------------------------------------------------------------------------------------------------
def _model(name):
    method, cfg, img, L = MODELS[name]
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval(), img, L


def _images(n, img, L):
    return torch.rand(2, 1, 1, 1, 1).expand(2, n, *img), torch.rand(2, n, L)


@pytest.mark.parametrize("name", list(MODELS))
def test_condition_refusals_of_the_long_form(name):
    from mlhot import cached, ragged
    assert "long" in ragged.FORMS and ragged.MAX_LONG_CAPACITY == 256 and ragged.MAX_ATTENTION_CAPACITY == 32
    model, img, L = _model(name)
    cx, cy = _images(4, img, L)
    entries = [lambda *a, **kw: cached.condition(model, *a, **kw)] + ([lambda *a, **kw: model.condition(*a, **kw)] if hasattr(model, "extend") else [])
    for cond in entries:
        if not model.ATTENTION:
            with pytest.raises(ValueError, match='form="long" serves the attention models'):          # a latent model
                cond(cx, cy, form="long")
            continue
        with pytest.raises(ValueError, match="capacity = 257 is outside the long attention kernels' envelope"):
            cond(cx, cy, form="long", capacity=257)
        with pytest.raises(ValueError, match="capacity = 257 is outside"):                            # ... also as the default capacity
            cond(*_images(257, img, L), form="long")
        with pytest.raises(ValueError, match="capacity = 3 is smaller than the 4 context slots"):
            cond(cx, cy, form="long", capacity=3)
        with pytest.raises(ValueError, match="capacity must be an integer"):
            cond(cx, cy, form="long", capacity=40.0)
        for bad in ([0, 4], [1, 5]):
            with pytest.raises(ValueError, match=r"ctx_len must lie in 1\.\.4"):                      # lens out of range
                cond(cx, cy, form="long", ctx_len=bad)
        with pytest.raises(ValueError, match="ctx_len has 3 entries"):
            cond(cx, cy, form="long", ctx_len=[1, 2, 3])
        with pytest.raises(ValueError, match="capacity = 33 is outside the cached attention kernels' envelope"):
            cond(cx, cy, capacity=33)                                                                 # form="keys" keeps its cap ...
        with pytest.raises(ValueError, match="capacity = 33 is outside the cached attention kernels' envelope"):
            cond(cx, cy, form="keys", ctx_len=[1, 2], capacity=33)                                    # ... however it is asked
    if model.ATTENTION:
        with pytest.raises(ValueError, match="at least one context shot"):
            cached.condition(model, cx[:, :0], cy[:, :0], form="long")
        model.train()
        with pytest.raises(ValueError, match="eval"):
            cached.condition(model, cx, cy, form="long")


def _long_state(model, lens=(40, 31), cap=64):
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    from networks._resnet_np import ResNetNP
    d = 256 if isinstance(model, ResNetNP) else 64
    keys = FavorKeyState("long", (2, cap, 8, d, model.attn.projection_matrix.shape[0]), buf=None, lens=tuple(lens))
    rows = torch.zeros(2, cap, 8, d)
    return ContextState(model, 2, cap, fingerprint(model), "attention", keys=keys, vh=rows, kh=rows, lens=lens, form="long")


@pytest.mark.parametrize("name", ["resnet_anp", "vanilla_anp"])
def test_extend_merge_and_route_refusals_on_a_long_state(name):
    from mlhot import cached
    model, img, L = _model(name)
    state = _long_state(model)
    assert state.capacity == 64 and state.form == "long" and state.lens == (40, 31)
    (nx, ny), qx = _images(30, img, L), torch.rand(2, 3, *img)
    with pytest.raises(ValueError, match="task 0 would hold 70 context shots, the state's capacity is 64"):
        cached.extend(model, state, nx, ny)
    with pytest.raises(ValueError, match=r"new_len must lie in 0\.\.30"):
        cached.extend(model, state, nx, ny, new_len=[31, 0])
    with pytest.raises(ValueError, match=r"states\[0\] has form 'long'.*per-shot rows in at most 256 slots"):
        cached.merge(model, [state])
    if name == "vanilla_anp":
        with pytest.raises(ValueError, match='route "fused".*a long state'):
            cached.predict(model, state, qx, route="fused")
        with pytest.raises(ValueError, match='route "fused"'):
            cached.predict(model, state, qx, route="fused", return_attention=True)
    other, _, _ = _model(name)
    with pytest.raises(ValueError, match="not made by this model"):
        cached.predict(other, state, qx, return_attention=True)


def test_ops_refusals():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_keys_long, favor_merge
    k, proj = torch.zeros(2, 40, 2, 16), torch.zeros(16, 16)
    with pytest.raises(MlhotError, match="needs tensors on a ROCm device"):
        favor_keys_long(k, proj)
    with pytest.raises(MlhotError, match="forward-only"):
        favor_keys_long(k.clone().requires_grad_(), proj)
    long = FavorKeyState("long", (2, 40, 2, 16, 16), buf=torch.zeros(8, dtype=torch.uint8), lens=(40, 3))
    with pytest.raises(MlhotError, match=r"states\[0\] has route 'long'"):
        favor_merge([long])
    with pytest.raises(MlhotError, match="no summary"):
        long.summary()
