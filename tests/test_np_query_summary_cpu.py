"""The one-launch query tail on a FAVOR+ summary state without a GPU: the float64 statement
tests/np_query_summary_ref.py against tests/np_query_ref.py on the concatenated shots, the host build's two entries, and the
bookkeeping of predict's route "fused_summary" on a recording stand-in for the library - every refusal before a call is recorded."""
import ctypes as C
import importlib
import types

import pytest
import torch

from tests import favor_cached_ref as R
from tests import np_query_ref as NR
from tests import np_query_summary_ref as QS

CFGV = dict(seed=2578, img_size=[128, 128, 1], tasks_per_batch=2, input_dim=3, output_dim=2, img_agg="", dim_w=64,
            n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", temperature=0.07)
CFG3D = dict(seed=2578, temperature=0.07, task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape",
             tasks_per_batch=2)
MODELS = {
    "resnet_anp": ("ANP", dict(CFG3D, agg_mode="attention"), (3, 64, 64)),
    "vanilla_anp": ("ANPShapeNet1D", dict(CFGV, agg_mode="attention", dim_r=64), (1, 128, 128)),
}


# ---- the reference against the per-shot mathematics ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 33, 100])
@pytest.mark.parametrize("d,m", [(16, 16), (32, 40), (64, 266)])
def test_reference_on_a_float64_summary_equals_np_query_ref_on_the_shots(d, m, N):
    x, k, v = QS.case(d, m, N, 20)
    p, proj = QS.params(d), QS.proj_matrix(d, m)
    want = NR.query_tail(p, x, {"kind": "attention", "fk": R.key_features(k, proj)[0], "vh": v.double()}, QS.tanh_for(d), proj)
    st = QS.state_from_shots(k, v, proj)
    assert st.cnt == [N, N]
    got = QS.tail_of_state(p, x, st, proj, QS.tanh_for(d))
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"summary tail reference d={d} m={m} {N} shots: {err:.2e} of mu's scale")
    assert got.shape == (QS.T, 20, QS.Y_DIM) and bool(torch.isfinite(got).all()) and err <= 1e-10


# ---- the host build -----------------------------------------------------------------------------------------------------------------
def test_hostsim_has_the_two_entries_and_they_are_unsupported(hostsim):
    from mlhot.binding import NpParams
    dims = hostsim.np_dims(2, 40, 1, 3, 2, 64, 64, 64, [100, 100], 100, "attention", True, 266)
    assert not hostsim.np_query_summary_supported(dims)
    buf = torch.full((1024,), 7.0)
    p = C.c_void_p(buf.data_ptr())
    assert hostsim.c.mlhot_np_query_summary_fwd(C.byref(dims), C.byref(NpParams()), p, 5, p, p, None) == 4      # MLHOT_ERR_UNSUPPORTED
    assert "np_query_summary_fwd" in hostsim.c.mlhot_last_error().decode()
    assert hostsim.c.mlhot_np_query_summary_fwd(C.byref(dims), C.byref(NpParams()), p, 0, p, p, None) == 1      # MLHOT_ERR_ARG: Nq < 1
    assert hostsim.c.mlhot_np_query_summary_fwd(C.byref(dims), C.byref(NpParams()), p, 5, None, p, None) == 1   # ... a NULL state
    assert bool((buf == 7.0).all())


# ---- predict's route ------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library and the operators behind predict: records every call that would launch."""

    def __init__(self, served=True):
        from mlhot.binding import MlhotLib
        self.calls, self.served, self.np_dims = [], served, MlhotLib.np_dims

    def np_query_supported(self, dims):
        return True

    def np_query_summary_supported(self, dims):
        return self.served

    def linear_rows_supported(self, k0, k1, n):
        return True

    def np_query_summary_fwd(self, dims, params, x_qry, summary_state, proj, out=None):
        self.calls.append(("np_query_summary_fwd", tuple(x_qry.shape), summary_state.data_ptr(), tuple(proj.shape)))
        return torch.zeros(dims.T, x_qry.shape[1], dims.y_dim)

    def np_query_fwd(self, dims, params, x_qry, **kw):
        self.calls.append(("np_query_fwd", tuple(x_qry.shape)))
        return torch.zeros(dims.T, x_qry.shape[1], dims.y_dim)

    # the operators mlhot.cached calls by name
    def encode(self, model, imgs):
        self.calls.append(("encode", imgs.shape[1]))
        return torch.zeros(imgs.shape[0] * imgs.shape[1], model.dim_w)

    def linear_rows(self, sources, w, b, act):
        self.calls.append(("linear_rows", w.shape[0]))
        return torch.zeros(max(x.shape[0] * rep for x, rep, _ in sources), w.shape[0])

    def favor_query(self, qh, keys, vh, proj, weights=False):
        self.calls.append(("favor_query", keys.route))
        return torch.zeros(qh.shape[0], qh.shape[1], qh.shape[2] * qh.shape[3])

    def launches(self):
        return [c for c in self.calls if c[0] != "encode"]


def _model(name):
    method, cfg, img = MODELS[name]
    c = types.SimpleNamespace(device=torch.device("cpu"), **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval(), img


def _patched(monkeypatch, served=True):
    import networks._vanilla as V
    from mlhot import cached
    rec = _Recorder(served)
    monkeypatch.setattr(cached, "lib", lambda: rec)
    monkeypatch.setattr(V, "lib", lambda: rec)
    monkeypatch.setattr(cached, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(cached, "_encode", rec.encode)
    monkeypatch.setattr(cached, "linear_rows", rec.linear_rows)
    monkeypatch.setattr(cached, "favor_query", rec.favor_query)
    return rec


def _state(model, form="summary", kind="attention", lens=(40, 31)):
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    m = model.attn.projection_matrix.shape[0]
    d = model.attn.projection_matrix.shape[1]
    if kind != "attention":
        return ContextState(model, 2, 0 if kind == "empty" else 5, fingerprint(model), kind, z=torch.zeros(2, 64))
    route = {"summary": "summary", "keys": "cached", "long": "long"}[form]
    keys = FavorKeyState(route, (2, max(lens), 8, d, m), buf=torch.zeros(64, dtype=torch.uint8), lens=tuple(lens))
    rows = None if form == "summary" else torch.zeros(2, max(lens), 8, d)
    return ContextState(model, 2, max(lens), fingerprint(model), "attention", keys=keys, vh=rows, kh=rows, lens=lens, form=form,
                        wq=(torch.zeros(8 * d, d), torch.zeros(8 * d)))


def test_fused_summary_reaches_the_launch_once_per_chunk(monkeypatch):
    from mlhot import cached
    model, img = _model("vanilla_anp")
    rec = _patched(monkeypatch)
    state = _state(model)
    qx = torch.rand(2, 7, *img)
    mu = cached.predict(model, state, qx, route="fused_summary")
    assert state.route == "fused_summary" and mu.shape == (2, 7, 2)
    want = ("np_query_summary_fwd", (2, 7, 64), state.keys.buf.data_ptr(), tuple(model.attn.projection_matrix.shape))
    assert rec.calls == [("encode", 7), want]
    rec.calls.clear()
    mu = cached.predict(model, state, qx, chunk=3, route="fused_summary")
    assert mu.shape == (2, 7, 2)
    assert [c[:2] for c in rec.calls] == [("encode", 3), ("np_query_summary_fwd", (2, 3, 64))] * 2 + [("encode", 1), ("np_query_summary_fwd", (2, 1, 64))]
    assert "fused_summary" in cached.ROUTES and cached.ROUTES[:2] == ("fused", "composed")


def test_route_none_on_a_summary_state_still_runs_composed(monkeypatch):
    from mlhot import cached
    model, img = _model("vanilla_anp")
    rec = _patched(monkeypatch)
    state = _state(model)
    for route in (None, "composed"):
        rec.calls.clear()
        cached.predict(model, state, torch.rand(2, 7, *img), route=route)
        assert state.route == "composed"
        names = [c[0] for c in rec.launches()]
        assert names == ["linear_rows", "favor_query"] + ["linear_rows"] * 5 and ("favor_query", "summary") in rec.calls
    with pytest.raises(ValueError, match='route "fused".*fused_summary'):          # the per-shot launch still refuses, and names the way
        cached.predict(model, state, torch.rand(2, 7, *img), route="fused")
    assert "np_query_summary_fwd" not in [c[0] for c in rec.calls]


def test_every_refusal_comes_before_a_call(monkeypatch):
    from mlhot import cached
    model, img = _model("vanilla_anp")
    rec = _patched(monkeypatch)
    qx = torch.rand(2, 3, *img)
    cases = [
        (_state(model, "keys", lens=(5, 5)), {}, r"this state is 'keys' and is served by route \"fused\""),
        (_state(model, "long", lens=(40, 40)), {}, r"this state is 'long' and is served by route \"composed\""),
        (_state(model, kind="latent"), {}, r"this state is 'latent' and is served by route \"fused\""),
        (_state(model, kind="empty"), {}, r"this state is 'empty' and is served by"),
        (_state(model), {"return_attention": True}, "a summary state keeps no per-shot rows"),
        (_state(model, "keys", lens=(5, 5)), {"return_attention": True}, 'return_attention=True with route "fused_summary"'),
        (_state(model, lens=(40, 0)), {}, r"has absorbed no shot \(shots per task: \[40, 0\]\)"),
    ]
    for state, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            cached.predict(model, state, qx, route="fused_summary", **kw)
        assert state.route is None
    with pytest.raises(ValueError, match="route must be one of"):
        cached.predict(model, _state(model), qx, route="fused-summary")
    assert rec.calls == []
    # dimensions outside the envelope: an error, not another route
    rec = _patched(monkeypatch, served=False)
    state = _state(model)
    with pytest.raises(ValueError, match=r"dimensions are outside mlhot_np_query_summary_fwd's envelope"):
        cached.predict(model, state, qx, route="fused_summary")
    assert rec.calls == [] and state.route is None
    # a ResNet-family model has no route= at all
    resnet, rimg = _model("resnet_anp")
    with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
        cached.predict(resnet, None, torch.rand(2, 3, *rimg), route="fused_summary")


def test_sweep_names_its_own_two_routes(monkeypatch):
    from mlhot import cached
    model, img = _model("vanilla_anp")
    cx, cy, qx = torch.rand(2, 4, *img), torch.rand(2, 4, 3), torch.rand(2, 3, *img)
    for bad in ("fused_summary", "summary"):
        with pytest.raises(ValueError, match=r"sweep: route must be one of \('fused', 'composed'\), got"):
            cached.sweep(model, cx, cy, qx, route=bad)
