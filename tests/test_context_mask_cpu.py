"""Per-target context masks without a GPU: mlhot.ragged.pack_mask against a bit-by-bit loop, the float64
statement (tests/context_mask_ref.py) against tests/favor_cached_ref.py - all ones is the unmasked attention, a leave-one-out row is
the attention on the context without that shot under the same stabiliser -, and every refusal of predict(context_mask=) and
leave_one_out, raised on the host before a device is asked for."""
import importlib
import types

import pytest
import torch

from tests import context_mask_cases as CC
from tests import context_mask_ref as CM
from tests import favor_cached_ref as R
from tests import ragged_ref as RR
from tests import util as U


# ---- pack_mask ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", [1, 31, 32, 33, 64, 65, 256])
def test_pack_mask_against_a_loop_over_the_bits(Nc):
    from mlhot.ragged import pack_mask
    T, G, Nq, W = 2, 3, 5, (Nc + 31) // 32
    mask = torch.rand(T, G, Nq, Nc, generator=torch.Generator().manual_seed(Nc)) < 0.5
    mask[0, 0, 0], mask[0, 0, 1] = True, False                        # a full and an empty row
    mask[1, 2, 4] = torch.arange(Nc) % 32 == 31                       # only the sign bits of the int32 words
    words = pack_mask(mask, Nc)
    assert words.shape == (T, G, Nq, W) and words.dtype == torch.int32 and words.is_contiguous()
    for t in range(T):
        for g in range(G):
            for n in range(Nq):
                for c in range(W):
                    want = sum(1 << j for j in range(32) if 32 * c + j < Nc and bool(mask[t, g, n, 32 * c + j]))
                    assert int(words[t, g, n, c]) & 0xFFFFFFFF == want, (t, g, n, c)
    assert torch.equal(pack_mask(mask[:, 1], Nc), words[:, 1:2])      # [T, Nq, Nc] is one group
    for bad in (mask.float(), mask[0, 0], mask[..., :-1] if Nc > 1 else mask.int()):
        with pytest.raises(ValueError, match="pack_mask"):
            pack_mask(bad, Nc)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in CC.SHAPES if s[2] is None], ids=str)
def test_all_ones_is_the_unmasked_attention(shape):
    _, Nc, _, d, m = shape
    q, k, v, p = CC.inputs(Nc, d, m)
    out, w = CM.masked(q, k, v, p, torch.ones(CC.T, 2, CC.NQ, Nc, dtype=torch.bool))
    want = R.attention(q, k, v, p)
    for g in range(2):
        assert U.rel_err(out[:, g], want) <= 1e-12
        assert float((w[:, g].sum(dim=-1) - 1.0).abs().max()) <= 1e-12


@pytest.mark.parametrize("shape", [s for s in CC.SHAPES if s[1] > 1], ids=str)
def test_a_leave_one_out_row_is_the_attention_without_that_shot(shape):
    """... given the same M: the key features come from the whole (ragged) context, then the shot's row is cut out."""
    _, Nc, lens, d, m = shape
    q, k, v, p = CC.inputs(Nc, d, m)
    L = CC.lens_of(shape)
    _, out, w = CC.want(shape, "loo")
    fk = RR.key_features(k, p, L)[0]
    for t in range(CC.T):
        for c in sorted({0, 1, 31, 32, L[t] - 1, Nc - 1} & set(range(Nc))):
            keep = [n for n in range(L[t]) if n != c]
            if not keep:
                assert not bool(out[t, c].any()) and not bool(w[t, c].any())
                continue
            want = R.query(q[t:t + 1], fk[t:t + 1, :, keep], v[t:t + 1, :, keep], p)
            assert U.rel_err(out[t, c], want[0]) <= 1e-12, (t, c)
            assert not bool(w[t, c, :, :, c].any()) and not bool(w[t, c, :, :, L[t]:].any())


def test_the_empty_row_is_zeros_and_the_dominant_case_is_dominant():
    mk, out, w = CC.want(CC.SHAPES[4], "bit32")                        # lens (33, 20): task 1 has no slot 32
    assert not bool(out[1].any()) and not bool(w[1].any()) and bool(torch.isfinite(out).all())
    assert float((w[0].sum(dim=-1) - 1.0).abs().max()) <= 1e-12
    full = CC.dominant()[-1]
    assert float(full[..., CC.DOMINANT["slot"]].min()) > 0.999


# ---- the refusals of predict(context_mask=) ----------------------------------------------------------------------------------------
CFG3D = dict(task="shapenet_3d", img_size=[64, 64, 4], input_dim=4, output_dim=4, img_agg="reshape")
CFG1D = dict(img_size=[128, 128, 1], img_agg="", dim_w=64, n_hidden_units_r=[100, 100], dim_z=64, task="shapenet_1d", input_dim=3, output_dim=2)
NQ, NC = 4, 3


def _cpu_model(method, **cfg):
    c = types.SimpleNamespace(device=torch.device("cpu"), seed=2578, temperature=0.07, tasks_per_batch=2, **cfg)
    return getattr(importlib.import_module("networks." + method), method)(c).eval()


def _attention_state(model, heads, d, route="cached", form="keys", lens=(3, 3)):
    from mlhot.context import ContextState, fingerprint
    from mlhot.ops import FavorKeyState
    m = model.attn.projection_matrix.shape[0]
    keys = FavorKeyState(route, (2, NC, heads, d, m), buf=torch.zeros(16, dtype=torch.uint8), lens=lens if form == "summary" else None)
    rows = None if form == "summary" else torch.zeros(2, NC, heads, d)
    return ContextState(model, 2, NC, fingerprint(model), "attention", keys=keys, vh=rows, kh=rows, form=form, lens=lens)


def _refusals(predict, loo, model, state_of, latent, empty, qx):
    ones = torch.ones(2, NQ, NC, dtype=torch.bool)
    for state in (latent, empty):
        with pytest.raises(ValueError, match="context_mask=.*has no attention"):
            predict(state, qx, context_mask=ones)
    with pytest.raises(ValueError, match="context_mask=.*summary state keeps no per-shot rows"):
        predict(state_of(route="summary", form="summary"), qx, context_mask=ones)
    with pytest.raises(ValueError, match="context_mask= needs the cached kernels' envelope"):
        predict(state_of(route="plain"), qx, context_mask=ones)
    state = state_of()
    for bad, why in ((ones.float(), "bool tensor"), ([[True]], "bool tensor"), (ones[:, :3], "got"), (ones[..., :2], "got"),
                     (ones[0], "got"), (ones[:, None][:, :0], "got"), (ones[:1], "got")):
        with pytest.raises(ValueError, match="context_mask must be.*" + why):
            predict(state, qx, context_mask=bad)
    hole = ones.clone()
    hole[1, 2] = False
    with pytest.raises(ValueError, match="keeps none of the 3 valid context shots of task 1 for target 2"):
        predict(state, qx, context_mask=hole)
    behind = torch.zeros(2, 2, NQ, NC, dtype=torch.bool)
    behind[..., 2] = True                                             # only slot 2, which task 0 of lens (2, 3) does not hold
    with pytest.raises(ValueError, match="valid context shots of task 0 for target 0 in group 0"):
        predict(state_of(lens=(2, 3)), qx, context_mask=behind)
    with pytest.raises(ValueError, match="single context shot"):
        loo(state_of(lens=(1, 3)), qx)
    # the existing refusals are unchanged and come first
    with pytest.raises(ValueError, match="same tasks"):
        predict(state, qx[:1], context_mask=ones)
    with pytest.raises(ValueError, match="not made by this model"):
        predict(object(), qx, context_mask=ones)
    stale = state_of()
    stale.fingerprint = (-1,) + tuple(stale.fingerprint[1:])
    with pytest.raises(ValueError, match="stale"):
        predict(stale, qx, context_mask=ones)
    model.train()
    with pytest.raises(ValueError, match="eval"):
        predict(state, qx, context_mask=ones)
    model.eval()


def test_resnet_predict_refuses_a_mask_it_cannot_serve():
    from mlhot import cached
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, NQ, 3, 64, 64)
    anp = _cpu_model("ANP", agg_mode="attention", **CFG3D)
    latent = ContextState(anp, 2, NC, fingerprint(anp), "latent", z=torch.zeros(2, 256))
    empty = ContextState(anp, 2, 0, fingerprint(anp), "empty")
    for predict in (anp.predict, lambda *a, **kw: cached.predict(anp, *a, **kw)):
        _refusals(predict, lambda s, x: cached.leave_one_out(anp, s, x), anp, lambda **kw: _attention_state(anp, 8, 256, **kw), latent, empty, qx)
    with pytest.raises(ValueError, match="route= belongs to the vanilla family"):
        cached.predict(anp, _attention_state(anp, 8, 256), qx, route="fused", context_mask=torch.ones(2, NQ, NC, dtype=torch.bool))


def test_vanilla_predict_refuses_a_mask_it_cannot_serve():
    from mlhot import cached
    from mlhot.binding import MlhotError
    from mlhot.context import ContextState, fingerprint
    qx = torch.rand(2, NQ, 1, 128, 128)
    anp = _cpu_model("ANPShapeNet1D", agg_mode="attention", dim_r=64, **CFG1D)
    latent = ContextState(anp, 2, NC, fingerprint(anp), "latent", z=torch.zeros(2, 64))
    empty = ContextState(anp, 2, 0, fingerprint(anp), "empty", z=torch.zeros(2, 64))
    _refusals(lambda *a, **kw: cached.predict(anp, *a, **kw), lambda s, x: cached.leave_one_out(anp, s, x), anp,
              lambda **kw: _attention_state(anp, 8, 64, **kw), latent, empty, qx)
    ones = torch.ones(2, NQ, NC, dtype=torch.bool)
    for route in ("fused", "fused_summary"):
        with pytest.raises(ValueError, match=f'context_mask= with route "{route}".*composed route'):
            cached.predict(anp, _attention_state(anp, 8, 64), qx, route=route, context_mask=ones)
    with pytest.raises(ValueError, match="route must be one of"):
        cached.predict(anp, _attention_state(anp, 8, 64), qx, route="both", context_mask=ones)
    with pytest.raises(MlhotError, match="ROCm device"):               # every host check passed: the next thing asked for is the device
        cached.predict(anp, _attention_state(anp, 8, 64), qx, context_mask=ones)


def test_favor_query_refuses_a_mask_on_states_without_cached_rows():
    from mlhot.binding import MlhotError
    from mlhot.ops import FavorKeyState, favor_query
    qh, proj = torch.randn(1, 5, 2, 16), torch.randn(32, 16)
    mask = torch.ones(1, 5, 3, dtype=torch.bool)
    summary = FavorKeyState("summary", (1, 3, 2, 16, 32), buf=torch.zeros(16, dtype=torch.uint8), lens=(3,))
    with pytest.raises(MlhotError, match="mask= - a summary state keeps no per-shot rows"):
        favor_query(qh, summary, None, proj, mask=mask)
    plain = FavorKeyState("plain", (1, 40, 2, 16, 32), kh=torch.randn(1, 40, 2, 16))
    with pytest.raises(MlhotError, match=r"mask= needs the cached kernels' envelope"):
        favor_query(qh, plain, torch.randn(1, 40, 2, 16), proj, mask=torch.ones(1, 5, 40, dtype=torch.bool))
