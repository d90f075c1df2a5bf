"""Shared by tests/test_tail_cases_cpu.py (host flavour of the library) and tests/test_tail_envelope_gpu.py (MI355X): everything between
the vanilla encoder and the loss (csrc/np_vanilla.h and the kernels it launches: tail_fused.h, tail_cnp.h, the operator chain) through the
raw entry np_vanilla_fwd / np_vanilla_bwd, AWAY from the shipped widths, against float64.

Every shipped configuration has hidden = (100, 100) = dec_hidden and dim_w = dim_z = 64, so a kernel that reads one width where it
means another, strides a tile by the wrong layer's width or indexes a gradient slab by the wrong one passes every whole-model test.
The cases here make every width differ from every other, and stand on both sides of every bound np_route() draws:

  LDS       a fused family runs only if EVERY launch of it, forward and backward, gets its dynamic LDS (160 KB per workgroup on
            gfx950).  attention_lds / cnp_lds restate the kernels' *_lds_bytes; the binding constraint is phase B' in m_feat
            (dim_w 64: m 416 fits, 417 does not; dim_w 128: m 224 fits, 225 does not, and FastAttention's default m = 621 does not),
            phase A' in the hidden widths, the CNP backward in the hidden widths.
  dim_w     % 64 and <= 128 for the attention family (phase A's key-head block computes kh as one 16-column tile per wave of 8; at
            dim_w 192 and m <= 32 the LDS would fit), % 16 for the pooled one; dim_r <= 128 for the pooled one.
  shots     1 .. 16 context and <= 16 target shots per task (one MFMA row tile); Nc = 0 is the empty context.
  n_hidden  2 for the fused families; 1 and MLHOT_MAX_HIDDEN = 4 run the chain's loops.

`family` is what must run under the default options; with tail_fused = 0 every case runs the chain.  Refusals (np_check_dims) are in
REFUSALS: nothing is launched for them.

Parameters: util.enc_params for the encoder, N(0, 1 / fan_in) weights and 0.1 N(0, 1) biases behind it (as tests/np_query_ref.py draws
the query side), all from the case's own seed.  The encoder's last Linear is then re-centred and scaled so that the image features have
spread 0.5 around 0 (test_tail_with_sharp_attention_vs_oracle): the attention weights differ from key to key and the W_q / W_k
gradients are first class, the max aggregator's winners differ from feature to feature.  The upstream gradient dmu is random."""
import collections
import functools

import torch

from oracle import ref_cpu as O
from tests import util as U

HEADS = 8
MAX_HIDDEN = 4
LDS_LIMIT = 160 * 1024           # bytes per workgroup, gfx950
KEYHEAD_MAX_DW = 128             # tail_fused.h: 8 waves x one 16-column tile of kh
QK_MIN = 1e-6                    # smallest W_q / W_k gradient, of the model's largest (a condition on the inputs)
QK_TOL = 2e-4                    # W_q / W_k gradients, of their own scale, no floor


def qk_live(c):
    """Whether the W_q / W_k gradients are first class.  With ONE context shot FAVOR+'s output is the value row itself, (q' . k') v /
    (q' . k'), whatever q and k are: those gradients are mathematically zero and what float arithmetic leaves of them is compared
    like every other small gradient, at the floor."""
    return c.agg == "attention" and c.Nc >= 2

Case = collections.namedtuple("Case", "name T Nc Nq label_dim y_dim dim_w dim_r dim_z hidden dec_hidden agg out_tanh m_feat family")

_DISTINCT = dict(T=2, Nc=3, Nq=4, label_dim=3, y_dim=2, dim_w=64, dim_r=64, dim_z=48, hidden=(80, 112), dec_hidden=72, agg="attention",
                 out_tanh=True, m_feat=266, family="attention")
_POOLED = dict(_DISTINCT, dim_w=48, dim_r=72, dim_z=40, hidden=(56, 88), dec_hidden=104, agg="mean", m_feat=0, family="cnp")


def _case(name, base=_DISTINCT, **kw):
    d = dict(base, **kw)
    if d["agg"] == "attention":
        d["dim_r"] = d["dim_w"]
    return Case(name=name, **d)


CASES = [
    # ---- attention ---------------------------------------------------------------------------------------------------------------
    _case("attn_distinct", Nc=5, Nq=7),                                                  # every width differs from every other
    _case("attn_distinct_rows", hidden=(96, 104)),                                       # ... and from the row strides dim_w + dim_w / 4, dim_w + dim_z
    _case("attn_small_widths", dim_z=20, hidden=(36, 52), dec_hidden=24),                # ldpad tiles mostly padding
    _case("attn_odd_hidden", dim_z=20, hidden=(37, 50), dec_hidden=23),                  # K % 4 != 0: the layer function's dword weight loads
    _case("attn_y8", label_dim=1, y_dim=8),
    _case("attn_y1", label_dim=5, y_dim=1, out_tanh=False),
    _case("attn_m416", m_feat=416),                                                      # the last m whose phase B' fits
    _case("attn_m417", m_feat=417, family="generic"),
    _case("attn_dw128", dim_w=128, dim_z=64, hidden=(100, 100), dec_hidden=100, m_feat=621, family="generic"),   # ANPShapeNet1D(dim_w = 128)
    _case("attn_dw128_fused", dim_w=128, m_feat=224),                                    # two 64-column blocks; the last m that fits there
    _case("attn_dw128_m225", dim_w=128, m_feat=225, family="generic"),
    _case("attn_dw192_m32", dim_w=192, m_feat=32, family="generic"),                     # LDS would fit; the key-head block's 8 tiles do not
    _case("attn_shots_1_1_1", T=1, Nc=1, Nq=1),
    _case("attn_shots_1_16_16", T=1, Nc=16, Nq=16),                                      # full row tiles
    _case("attn_shots_2_17_3", Nc=17, Nq=3, family="generic"),
    _case("attn_shots_2_0_4", Nc=0, Nq=4, family="generic"),                             # the empty context
    _case("attn_wide_hidden_fits", hidden=(512, 528)),                                   # the last phase A' that fits
    _case("attn_wide_hidden", hidden=(512, 544), family="generic"),
    # ---- pooled ------------------------------------------------------------------------------------------------------------------
    _case("cnp_distinct_mean", _POOLED, Nc=5, Nq=7),
    _case("cnp_distinct_rows", _POOLED, hidden=(56, 96), agg="max"),
    _case("cnp_max_dr128", _POOLED, dim_w=16, dim_r=128, agg="max"),                      # the route's dim_r limit
    _case("cnp_dr132", _POOLED, dim_r=132, agg="max", family="generic"),
    _case("cnp_dw24", _POOLED, dim_w=24, family="generic"),                               # % 4, not % 16
    _case("cnp_odd_hidden", _POOLED, dim_r=70, dim_z=20, hidden=(37, 50), dec_hidden=23, agg="max"),
    _case("cnp_wide_hidden_fits", _POOLED, hidden=(320, 272)),                            # the last backward that fits
    _case("cnp_wide_hidden", _POOLED, hidden=(320, 288), family="generic"),
    _case("baco_distinct", _POOLED, agg="baco", family="generic"),
    _case("hidden1", _POOLED, hidden=(56,), family="generic"),
    _case("hidden_max", _POOLED, hidden=(56, 88, 44, 60), agg="max", family="generic"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(c.T * (c.Nc + c.Nq) <= 40 for c in CASES)         # the float64 oracle of a case takes seconds

# (name, the dims that differ from attn_distinct / cnp_distinct_mean, error code, what the message must name)
ERR_ARG, ERR_UNSUPPORTED = 1, 4
REFUSALS = [
    ("dim_w_62", _case("r", _POOLED, dim_w=62), ERR_ARG, "dim_w"),
    ("dim_z_50", _case("r", dim_z=50), ERR_ARG, "dim_z"),
    ("dim_z_0", _case("r", _POOLED, dim_z=0), ERR_ARG, "dim_z"),
    ("dec_hidden_0", _case("r", dec_hidden=0), ERR_ARG, "dec_hidden"),
    ("hidden1_0", _case("r", hidden=(80, 0)), ERR_ARG, "hidden[1]"),
    ("attention_dim_r", _case("r")._replace(dim_r=72), ERR_ARG, "dim_r"),
    ("rows_overflow", _case("r", T=1 << 20, Nc=16, Nq=16), ERR_UNSUPPORTED, "rows"),
]


# ---- the route, restated (csrc/np_vanilla.h np_route, csrc/tail_fused.h / tail_cnp.h *_lds_bytes) ------------------------------------
def ldpad(w):
    return (w + 15) // 16 * 16 + 4


def _ptab(n_pointers):
    return (2 * n_pointers + 3) // 4 * 4


PTAB_TAIL = _ptab(16 + 6 * HEADS + 3)       # tf::TailParams
PTAB_CNP = _ptab(16)                        # tf::CnpParams


def attention_lds(c):
    """Bytes of dynamic LDS per launch of the run-time-shaped attention kernels."""
    dw, dz, (h0, h1), dh, m = c.dim_w, c.dim_z, c.hidden, c.dec_hidden, c.m_feat
    ldc, ldd = dw + dw // 4, dw + dz
    chain = 16 * (ldpad(ldc) + ldpad(h0) + ldpad(h1) + ldpad(dw) + ldpad(c.label_dim)) + 8 * 256
    return {
        "tail.A": 4 * (max(chain, 32 * ldpad(dw) + 16) + PTAB_TAIL),
        "tail.B": 4 * (16 * (5 * ldpad(dw) + 2 * ldpad(m)) + 8 * 16 * 17 + 64 + 16),
        "tail.C": 4 * (16 * (ldpad(dw) + ldpad(ldd) + 2 * ldpad(dh)) + 8 * 256 + PTAB_TAIL),
        "tail.bwd.C": 4 * (16 * (ldpad(c.y_dim) + 4 * ldpad(dh) + 2 * ldpad(ldd) + 2 * ldpad(dw)) + 8 * 256 + PTAB_TAIL),
        "tail.bwd.B": 4 * (16 * (12 * ldpad(dw) + 4 * ldpad(m)) + 2 * 16 * 17 + 64),
        "tail.bwd.A": 4 * (16 * (2 * ldpad(ldc) + 2 * ldpad(h0) + 2 * ldpad(h1) + 2 * ldpad(dw) + ldpad(c.label_dim)) + 8 * 256 + PTAB_TAIL),
    }


def cnp_lds(c):
    dw, dr, dz, (h0, h1), dh = c.dim_w, c.dim_r, c.dim_z, c.hidden, c.dec_hidden
    ldc, ldd = dw + dw // 4, dw + dz
    return {
        "tail.cnp": 4 * (16 * (ldpad(ldc) + ldpad(h0) + ldpad(h1) + 2 * ldpad(dr) + ldpad(dz) + ldpad(ldd) + 2 * ldpad(dh) + ldpad(c.label_dim))
                         + 8 * 256 + PTAB_CNP),
        "tail.bwd.cnp": 4 * (16 * (ldpad(c.y_dim) + 4 * ldpad(dh) + 2 * ldpad(ldd) + 4 * ldpad(dr) + ldpad(dz) + 2 * ldpad(h1) + 2 * ldpad(h0)
                                   + 2 * ldpad(ldc) + ldpad(c.label_dim)) + 8 * 256 + PTAB_CNP),
    }


def lds_bytes(c):
    """{launch label: bytes} of the fused family the case's aggregation would take, {} where there is none."""
    if len(c.hidden) != 2:
        return {}
    return attention_lds(c) if c.agg == "attention" else cnp_lds(c) if c.agg in ("mean", "max") else {}


def route(c):
    """The family np_route() must pick under the default options.  No case has the shipped widths, so the kernels specialised for
    them (tail_spec.h / cnp_spec.h, whose LDS is a constant that fits) never apply here."""
    one_tile = 1 <= c.Nc <= 16 and c.Nq <= 16 and len(c.hidden) == 2
    if not one_tile or c.agg == "baco":
        return "generic"
    fits = max(lds_bytes(c).values()) <= LDS_LIMIT
    if c.agg == "attention":
        ok = c.dim_w % 64 == 0 and c.dim_w <= KEYHEAD_MAX_DW and c.dim_r == c.dim_w and c.m_feat <= 4096 and c.T * c.Nc * HEADS < 1 << 19
        return "attention" if ok and fits else "generic"
    return "cnp" if c.dim_w % 16 == 0 and c.dim_r <= 128 and fits else "generic"


# what the profiler labels of a forward / backward must contain, and must not
FAMILY_LABELS = {
    "attention": (["tail.A", "tail.B", "tail.C"], ["tail.bwd.C", "tail.bwd.B", "tail.bwd.A"]),
    "cnp": (["tail.cnp"], ["tail.bwd.cnp"]),
    "generic": (["np.decoder0.0", "np.decoder0.2", "np.decoder0.4"], ["np.bwd.dec4.w", "np.bwd.dec2.w", "np.bwd.dec0.w"]),
}


def family_of(labels):
    """The family a list of launch labels belongs to: exactly one family's labels may appear."""
    seen = {fam for fam, (f, b) in FAMILY_LABELS.items() if any(x in labels for x in f + b)}
    assert len(seen) == 1, f"launches of {sorted(seen)} in one pass: {labels}"
    fam = seen.pop()
    f, b = FAMILY_LABELS[fam]
    assert all(x in labels for x in f) or all(x in labels for x in b), f"{fam}: incomplete launch list {labels}"
    return fam


# ---- inputs and parameters -------------------------------------------------------------------------------------------------------
def _seed(c):
    return 7919 * (CASES.index(c) if c in CASES else 999) + 13


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (ctx_x [T,Nc,1,128,128], ctx_y [T,Nc,label_dim], qry_x [T,Nq,1,128,128], dmu [T,Nq,y_dim]) on the CPU, fp32."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(c))
    cx = torch.rand(c.T, c.Nc, 1, 128, 128, generator=g)
    qx = torch.rand(c.T, c.Nq, 1, 128, 128, generator=g)
    cy = torch.rand(c.T, c.Nc, c.label_dim, generator=g) * 2 - 1
    dmu = torch.randn(c.T, c.Nq, c.y_dim, generator=g)
    return cx, cy, qx, dmu


@functools.lru_cache(maxsize=None)
def params(name):
    """State-dict-keyed fp32 parameters of the case (for attention with "attn.projection_matrix")."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(_seed(c) + 1)
    p = dict(U.enc_params(c.dim_w, _seed(c) + 2))

    def lin(key, n_out, n_in):
        p[key + ".weight"] = torch.randn(n_out, n_in, generator=g) * n_in ** -0.5
        p[key + ".bias"] = 0.1 * torch.randn(n_out, generator=g)
    dw, dr, dz, dh = c.dim_w, c.dim_r, c.dim_z, c.dec_hidden
    lin("transform_y", dw // 4, c.label_dim)
    lin("r_to_z", dz, dr)
    widths = [dw + dw // 4, *c.hidden, dr]
    for i in range(len(c.hidden) + 1):
        lin(f"encoder_r.layers.{2 * i}", widths[i + 1], widths[i])
    lin("decoder0.0", dh, dw + dz)
    lin("decoder0.2", dh, dh)
    lin("decoder0.4", c.y_dim, dh)
    if c.agg == "baco":
        lin("rs_to_mu", dr, dr)
        lin("rs_to_var", dr, dr)
    if c.agg == "attention":
        for tag in ("_W_k", "_W_v", "_W_q"):
            for i in range(HEADS):
                lin(f"{tag}.{i}.linear", dw, dw)
        lin("_W.linear", dw, HEADS * dw)
        with torch.random.fork_rng():
            torch.manual_seed(_seed(c) + 3)
            p["attn.projection_matrix"] = O.gaussian_orthogonal_random_matrix(c.m_feat, dw).float()
    # re-centre and scale the encoder's last Linear: features = 0.5 / spread * (features - mean) over the case's own images
    cx, _, qx, _ = inputs(name)
    with torch.no_grad():
        f = O.vanilla_encoder(torch.cat([cx.reshape(c.T * c.Nc, 1, 128, 128), qx.reshape(c.T * c.Nq, 1, 128, 128)]), p)
        spread = f.std(dim=0).mean().item()
        scale = 0.5 / spread
        p["encoder_w0.8.bias"] = (p["encoder_w0.8.bias"] - f.mean(dim=0)) * scale
        p["encoder_w0.8.weight"] = p["encoder_w0.8.weight"] * scale
    return {k: v.contiguous() for k, v in p.items()}


def dims_of(lib, c):
    return lib.np_dims(c.T, c.Nc, c.Nq, c.label_dim, c.y_dim, c.dim_w, c.dim_r, c.dim_z, list(c.hidden), c.dec_hidden, c.agg, c.out_tanh, c.m_feat)


# ---- one run of the library, and the float64 oracle under its routing ------------------------------------------------------------------
def run(lib, c, dev, flat=True, loss=None):
    """np_vanilla_fwd + np_vanilla_bwd of `lib` on `dev` -> dict(mu, grads, views (saved activations, CPU), routes, fwd / bwd labels (on
    the device)).  loss: None (the upstream gradient is the case's dmu), or "bwd_loss": the mse loss against the case's dmu as labels,
    its gradient taken inside the backward call (mlhot_np_vanilla_bwd_loss), or "loss_then_bwd": the same loss, its gradient from
    loss_bwd, then the plain call."""
    from tests.test_gpu_parity import _vanilla_routes           # imported, not copied: one statement of the routes' form
    on_gpu = dev != "cpu"
    cx, cy, qx, dmu = (t.to(dev) for t in inputs(c.name))
    p = {k: v.to(dev) for k, v in params(c.name).items()}
    proj = p.pop("attn.projection_matrix", None)
    dims = dims_of(lib, c)
    cxf, qxf = cx.reshape(c.T * c.Nc, 1, 128, 128), qx.reshape(c.T * c.Nq, 1, 128, 128)
    out = {}

    def fwd():
        return lib.np_vanilla_fwd(dims, p, cxf, cy, qxf, proj)

    def bwd(mu, saved, scratch):
        if loss is None:
            return lib.np_vanilla_bwd(dims, p, cxf, cy, qxf, mu, dmu, saved, scratch, proj, flat=flat)
        one = torch.ones((), device=dev)
        if loss == "bwd_loss":
            return lib.np_vanilla_bwd(dims, p, cxf, cy, qxf, mu, None, saved, scratch, proj, loss=("mse", dmu, one), flat=flat)
        return lib.np_vanilla_bwd(dims, p, cxf, cy, qxf, mu, lib.loss_bwd("mse", mu, dmu, one), saved, scratch, proj, flat=flat)
    if on_gpu:
        out["fwd_labels"], (mu, saved, scratch) = U.launch_labels(lib, fwd)
        out["bwd_labels"], grads = U.launch_labels(lib, lambda: bwd(mu, saved, scratch))
        torch.cuda.synchronize()
    else:
        mu, saved, scratch = fwd()
        grads = bwd(mu, saved, scratch)
    out["mu"], out["grads"] = mu.cpu(), {k: g.cpu() for k, g in grads.items()}
    views = lib.np_saved_views(saved, dims)
    routes = _vanilla_routes(lib, [("np", dims, saved)], c.T, c.Nc, c.Nq, c.agg)
    if not on_gpu:      # the host flavour's generic encoder keeps a1 itself and writes no sign-bit words: its conv1 mask is a1 > 0
        a1 = (lib.enc_saved_views(saved, views["n"])[0] > 0).float()
        Rc = c.T * c.Nc
        routes["enc_qry"] = (a1[Rc:],) + tuple(routes["enc_qry"][1:])
        if c.Nc:
            routes["enc_ctx"] = (a1[:Rc],) + tuple(routes["enc_ctx"][1:])
    out["routes"] = routes
    out["views"] = {k: ([t.cpu().clone() for t in v] if isinstance(v, list) else v.cpu().clone()) for k, v in views.items()
                    if k not in ("enc", "n", "amax", "kh", "vh", "qh", "merged")}
    return out


def oracle(c, routes=None, dtype=torch.float64):
    """oracle.ref_cpu.vanilla_np_forward in `dtype` under `routes` (None: its own decisions), loss = sum(mu * dmu)
    -> dict(mu, grads, acts (the saved activations' names), pres)."""
    cx, cy, qx, dmu = (t.to(dtype) for t in inputs(c.name))
    p = {k: v.to(dtype).requires_grad_("projection" not in k) for k, v in params(c.name).items()}
    taps, pres = {}, {}
    if routes is not None:
        routes = {k: (tuple(t.to(dtype) if t.is_floating_point() else t for t in v) if isinstance(v, tuple) else
                      [t.to(dtype) for t in v] if isinstance(v, list) else v) for k, v in routes.items()}
    mu = O.vanilla_np_forward(p, cx, cy, qx, c.agg, tanh=c.out_tanh, taps=taps, routes=routes, pres=pres if routes is not None else None)
    (mu * dmu).sum().backward()
    acts = {"dec_in": torch.cat([taps["x_qry"], taps["z"]], dim=-1)}
    if routes is not None:
        acts["d1"], acts["d2"] = (v.detach() * m for v, m in zip(pres["d"], routes["d"]))
        if c.Nc:
            acts["h"] = [v.detach() * m for v, m in zip(pres["h"], routes["h"])]
    if c.Nc:
        ly = torch.nn.functional.linear(cy, p["transform_y.weight"], p["transform_y.bias"])
        acts["cat_in"] = torch.cat([taps["x_ctx"], ly], dim=-1)
        acts["rs"] = taps["rs"]
        if c.agg == "attention":
            acts["rr"] = taps["r"]
        else:
            acts["r"], acts["zt"] = taps["r"], taps["z"][:, 0]
    return {"mu": mu.detach(), "grads": {k: v.grad for k, v in p.items() if "projection" not in k}, "pres": pres,
            "acts": {k: ([t.detach() for t in v] if isinstance(v, list) else v.detach()) for k, v in acts.items()}}


def qk_share(grads):
    """Smallest largest-entry of a W_q / W_k gradient, as a share of the model's largest gradient entry."""
    gmax = max(g.abs().max().item() for g in grads.values() if g is not None)
    return min(g.abs().max().item() / gmax for k, g in grads.items() if k.startswith("_W_q") or k.startswith("_W_k"))


def compare(c, got, ref, what, rtol=U.RTOL):
    """mu, every saved activation and every gradient of one run against the oracle under that run's routing; every routing decision
    that differs from the oracle's own is proven a tie, their share is bounded -> dict(act, grad, qk: worst errors; flips, decisions)."""
    from tests.test_gpu_parity import _count_decisions, _vanilla_flips
    errs = {"mu": U.rel_err(got["mu"], ref["mu"])}
    for k, v in ref["acts"].items():
        if isinstance(v, list):
            errs.update({f"{k}[{i}]": U.rel_err(g, r) for i, (g, r) in enumerate(zip(got["views"][k], v))})
        else:
            errs[k] = U.rel_err(got["views"][k], v)
    worst_act = max(errs.items(), key=lambda kv: kv[1])
    for k, e in errs.items():
        assert e <= rtol, f"{c.name} {what}: {k} rel err {e:.2e} > {rtol:.0e}"
    flips = _vanilla_flips(got["routes"], ref["pres"])
    decisions = _count_decisions(got["routes"])
    assert flips <= max(1, U.FLIP_RATE * decisions), f"{c.name} {what}: {flips} of {decisions} routing decisions differ (on ties): change the seed"
    live = {k: g for k, g in ref["grads"].items() if g is not None}
    gmax = max(g.abs().max().item() for g in live.values())
    worst, worst_qk = (0.0, None), (0.0, None)
    for k, g in live.items():
        if qk_live(c) and (k.startswith("_W_q") or k.startswith("_W_k")):
            e = U.rel_err(got["grads"][k], g)
            worst_qk = max(worst_qk, (e, k))
            assert e <= QK_TOL, f"{c.name} {what}: {k}: {e:.2e} of its own scale"
        else:
            e = U.rel_err(got["grads"][k], g, floor=U.GRAD_FLOOR * gmax)
            worst = max(worst, (e, k))
            assert e <= rtol, f"{c.name} {what}: gradient {k}: {e:.2e} > {rtol:.0e}"
    print(f"[tail envelope] {c.name} {what}: worst activation {worst_act[1]:.2e} ({worst_act[0]}), worst gradient {worst[0]:.2e} ({worst[1]}), "
          f"W_q / W_k {worst_qk[0]:.2e} ({worst_qk[1]}); {flips} of {decisions} decisions on a tie fell the other way; LDS {lds_bytes(c)}")
    return {"act": worst_act[1], "grad": worst[0], "qk": worst_qk[0], "flips": flips, "decisions": decisions}


def refusal(lib, c):
    """(error code, message) of mlhot_np_vanilla_fwd for dims that np_check_dims must refuse; every pointer null - the check comes
    before anything is read or launched."""
    import ctypes as C
    from mlhot.binding import NpParams
    dims, ps = dims_of(lib, c), NpParams()
    rc = lib.c.mlhot_np_vanilla_fwd(C.byref(dims), C.byref(ps), None, None, None, None, None, None, 0, None)
    return rc, lib.c.mlhot_last_error().decode()
