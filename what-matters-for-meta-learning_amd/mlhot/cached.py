"""Cached-context inference as functions: `condition` once, `predict` for any targets.

    state = mlhot.cached.condition(model, ctx_x, ctx_y, ctx_len=None, capacity=None, form="keys")     # "summary": beyond 32 shots (6c-4)
    state = mlhot.cached.extend(model, state, new_x, new_y, new_len=None)        # more context shots, only they are encoded (6c-3)
    mu = mlhot.cached.predict(model, state, qry_x, chunk=None)        # [T, Nq, y_dim]
    ok, reason = mlhot.cached.supports(model)
    mu = mlhot.cached.sweep(model, ctx_x, ctx_y, qry_x, ks=None, route=None)      # [len(ks), T, Nq, y_dim]: every context prefix (6b-2)
    ok, reason = mlhot.cached.supports_sweep(model)

For a ResNetNP instance the two functions are `model.condition` / `model.predict`.  For the vanilla 128x128x1 family (the classes
whose forward is VanillaNP.forward: CNPVanillaPascal1D, CNPShapeNet1D, ANPVanillaPascal1D, ANPShapeNet1D) they run the path of this
module - the classes themselves gain no attribute.  `condition` does everything of `forward(..., test=True)` that does not see the
targets, from existing entries; `predict` runs the encoder on the target images and then ONE launch, mlhot_np_query_fwd
(csrc/np_query.h; route "fused"), or - for dimensions that kernel does not serve - the same mathematics from linear_rows and
favor_query (route "composed").  `predict(condition(cx, cy), qx)` equals `model(cx, cy, qx, test=True)[0]` to the kernels'
tolerance, not to the bit.  Eval mode only; a state serves the T tasks it was conditioned on and dies with the next weight update.
"""
import logging
import numbers

import torch

from mlhot import lib, ragged
from mlhot.binding import HEADS
from mlhot.ops import LinearFunction, _c, _need_gpu, agg_prefixes, favor_keys, favor_prefixes_long, favor_query, linear_rows
from networks._resnet_np import ResNetNP
from networks._vanilla import VanillaNP
from networks._vanilla_mr import VanillaMR

ROUTES = ("fused", "composed")
_FRESH_WEIGHTS = ("Bayes-by-backprop draws fresh weights in every forward, so a cached context is not the reference's forward")
_logged = set()


class VanillaContextState:
    """What condition leaves for predict on a vanilla model.  `kind`: "attention" - `keys` (mlhot.ops.FavorKeyState for 8 heads) and
    the value heads `vh` [T, Nc, 8, dim_w]; "latent" - `z` [T, dim_z], the aggregated context through r_to_z; "empty" - no context
    shot, `z` zeros.  `owner` is the model, `fingerprint` its parameters' and buffers' versions when the state was made.  `route`
    is the route the last predict on this state took ("fused" | "composed"; None before the first).

    For extend the state also keeps `lens` (context shots per task, host ints), `capacity` (slots per task: `Nc`
    is the capacity, what the kernels see) and the per-shot rows in slot order [T, capacity, ...]: `kh` and the zero-filled `vh`
    (attention), `rs` - baco: rs_to_mu's output - and `lv` (latent), with `r`, the aggregate before r_to_z.

    `form` "summary" (DESIGN.md 6c-4): `keys` is a fixed-size summary state (mlhot.ops.favor_absorb), `Nc` the largest of `lens`;
    there is no capacity and there are no per-shot rows - `vh`, `kh` are None."""

    def __init__(self, owner, T, Nc, fingerprint, kind, keys=None, vh=None, z=None, wq=None, lens=None, kh=None, rs=None, lv=None, r=None,
                 form="keys"):
        self.owner, self.T, self.Nc, self.fingerprint, self.kind = owner, T, Nc, fingerprint, kind
        self.keys, self.vh, self.z, self.wq, self.route = keys, vh, z, wq, None
        self.lens, self.capacity, self.form = (Nc,) * T if lens is None else tuple(lens), Nc if form == "keys" else None, form
        self.kh, self.rs, self.lv, self.r = kh, rs, lv, r


def supports(model):
    """(bool, reason): whether condition / predict serve this model, and through what - or why not."""
    if isinstance(model, ResNetNP):
        if model.PREFIX_SWEEP_REFUSAL:
            return False, _FRESH_WEIGHTS
        return True, "ResNetNP.condition / predict"
    if type(model).forward is VanillaNP.forward:
        return True, "the vanilla family's query tail (mlhot_np_query_fwd)"
    if isinstance(model, VanillaMR):
        return False, _FRESH_WEIGHTS
    return False, "cached-context inference is not built for this class"


def _fingerprint(model):
    return tuple(p._version for p in model.parameters()) + tuple(b._version for b in model.buffers())


def _refuse(model, what):
    ok, reason = supports(model)
    if not ok:
        raise ValueError(f"{type(model).__name__}: mlhot.cached.{what}: {reason}")
    if model.training:
        raise ValueError(f"{what} is a test-mode path: call model.eval() first")


def _enc_params(model):
    e = model.encoder_w0
    return tuple(t.detach() for i in (0, 2, 5, 8) for t in (e[i].weight, e[i].bias))


def _encode(model, imgs):
    """[T, N, 1, 128, 128] -> the encoder's rows [T * N, dim_w] (mlhot_enc_vanilla_fwd; its `saved` buffer dies here)."""
    flat = _c(imgs.reshape(-1, model.img_channels, model.img_size[0], model.img_size[1]).float())
    return lib().enc_vanilla_fwd(flat, None, _enc_params(model), model.dim_w)[0]


def _stacked(mods):
    return (torch.cat([m.linear.weight.detach() for m in mods], dim=0), torch.cat([m.linear.bias.detach() for m in mods], dim=0))


def condition(model, ctx_x, ctx_y, ctx_len=None, capacity=None, form="keys"):
    """(ctx images [T, Nc, ...], ctx labels [T, Nc, L]) -> the state for predict: ResNetNP.condition for that family; for the
    vanilla family the encoder, transform_y and encoder_r, then the key / value heads and mlhot.ops.favor_keys (attention) or the
    aggregation and r_to_z (mean / max / baco).  No new kernel; the row count is T * Nc whatever follows.

    `ctx_len` (T host ints, 1 .. Nslots): the images are [T, Nslots, ...] and task t's context is its first ctx_len[t] slots; the other
    slots' images and labels are never read.  `capacity` >= Nslots reserves empty slots for extend (default Nslots; an attention
    model takes at most 32).  Without either argument this is the call it always was.

    `form="summary"` (attention models): the state is FAVOR+'s fixed-size summary of the context - any number of
    shots, `ctx_len` honoured, no `capacity`, no per-shot rows kept; extend absorbs any number of further shots and predict runs
    the composed route.  The default "keys" is every call as it was."""
    ragged.check_form("condition", form)
    if isinstance(model, ResNetNP):
        if form != "keys":
            return model.condition(ctx_x, ctx_y, ctx_len=ctx_len, capacity=capacity, form=form)
        if ctx_len is None and capacity is None:
            return model.condition(ctx_x, ctx_y)                  # today's call, as it always went out
        return model.condition(ctx_x, ctx_y, ctx_len=ctx_len, capacity=capacity)
    _refuse(model, "condition")
    T, Nc = ctx_x.shape[0], ctx_x.shape[1]
    if T != model.task_num:
        raise ValueError(f"condition: {T} tasks, the model was built for tasks_per_batch = {model.task_num}")
    if form == "summary":
        lens = ragged.summary_condition_args("condition", T, Nc, ctx_len, capacity, model.ATTENTION)
        _need_gpu(ctx_x, ctx_y, *model.parameters())
        with torch.no_grad():
            model._check_agg()
            return _absorb(model, None, ctx_x, ctx_y, lens, _stacked(model._W_q))
    lens, capacity = ragged.condition_args("condition", T, Nc, ctx_len, capacity, model.ATTENTION)
    _need_gpu(ctx_x, ctx_y, *model.parameters())
    with torch.no_grad():
        wq = _stacked(model._W_q) if model.ATTENTION else None
        if lens is not None:
            model._check_agg()
            return _grow(model, None, (0,) * T, capacity, ctx_x, ctx_y, lens, wq)
        if Nc == 0:
            return VanillaContextState(model, T, 0, _fingerprint(model), "empty", z=torch.zeros(T, model.dim_z, device=ctx_x.device), wq=wq)
        model._check_agg()
        x_ctx = _encode(model, ctx_x)
        ly = LinearFunction.apply(ctx_y.reshape(T * Nc, -1), model.transform_y.weight, model.transform_y.bias, "none")
        rs = model.encoder_r(torch.cat([x_ctx, ly], dim=1))
        if model.ATTENTION:
            kh = LinearFunction.apply(x_ctx, *_stacked(model._W_k), "none").view(T, Nc, HEADS, -1)
            vh = LinearFunction.apply(rs, *_stacked(model._W_v), "none").view(T, Nc, HEADS, -1)
            keys = favor_keys(kh, model.attn.projection_matrix)
            return VanillaContextState(model, T, Nc, _fingerprint(model), "attention", keys=keys, vh=vh.contiguous(), wq=wq, kh=kh.contiguous())
        lv = None
        if model.agg_mode == "baco":         # csrc/np_vanilla.h's order: rs_to_mu, rs_to_var, then the aggregation
            lv = LinearFunction.apply(rs, model.rs_to_var.weight, model.rs_to_var.bias, "none").view(T, Nc, -1)
            rs = LinearFunction.apply(rs, model.rs_to_mu.weight, model.rs_to_mu.bias, "none")
        r = lib().agg_fwd(model.agg_mode, rs.view(T, Nc, -1), lv)[0]
        z = LinearFunction.apply(r, model.r_to_z.weight, model.r_to_z.bias, "none")
        return VanillaContextState(model, T, Nc, _fingerprint(model), "latent", z=z, rs=rs.view(T, Nc, -1), lv=lv, r=r)


def extend(model, state, new_x, new_y, new_len=None):
    """(state, new ctx images [T, n, ...], their labels [T, n, L], new_len) -> a NEW state whose task t holds new_len[t] more context
    shots (0 .. n each; default n), written behind its current ones; the old state stays valid.  Only the new shots are encoded;
    then the masked key launches (attention) or the prefix aggregate with its gather and r_to_z (latent) run on the kept rows.  A
    state needs spare slots: condition with capacity=.  ResNetNP: model.extend."""
    if isinstance(model, ResNetNP):
        return model.extend(state, new_x, new_y, new_len=new_len)
    _refuse(model, "extend")
    if not isinstance(state, VanillaContextState) or state.owner is not model:
        raise ValueError("extend: the state was not made by this model's condition()")
    T, n = new_x.shape[0], new_x.shape[1]
    if T != state.T or state.T != model.task_num:
        raise ValueError(f"extend: the state holds {state.T} tasks, the new shots {T} (the key stabiliser is the maximum over the "
                         "conditioned batch: extend serves the same tasks)")
    if state.fingerprint != _fingerprint(model):
        raise ValueError("extend: the state is stale - a parameter of the model changed since condition()")
    if state.form == "summary":
        add = ragged.summary_extend_args("extend", T, n, new_len)
        _need_gpu(new_x, new_y, *model.parameters())
        with torch.no_grad():
            return _absorb(model, state, new_x, new_y, add, state.wq)
    add = ragged.extend_args("extend", state, T, n, new_len)
    _need_gpu(new_x, new_y, *model.parameters())
    with torch.no_grad():
        return _grow(model, state, state.lens, state.capacity, new_x, new_y, add, state.wq)


def _shot_rows(model, imgs, labels):
    """The per-shot part of condition for a packed list of P shots: images [P, 1, 128, 128], labels [P, L] -> (kh, vh) [P, 8, dim_w]
    for the attention models, (rs, lv) [P, R] for the others (baco: rs_to_mu's and rs_to_var's outputs; else lv None)."""
    x_ctx = _encode(model, imgs)
    ly = LinearFunction.apply(labels, model.transform_y.weight, model.transform_y.bias, "none")
    rs = model.encoder_r(torch.cat([x_ctx, ly], dim=1))
    if model.ATTENTION:
        return (LinearFunction.apply(x_ctx, *_stacked(model._W_k), "none").view(-1, HEADS, model.dim_w),
                LinearFunction.apply(rs, *_stacked(model._W_v), "none").view(-1, HEADS, model.dim_w))
    if model.agg_mode == "baco":
        lv = LinearFunction.apply(rs, model.rs_to_var.weight, model.rs_to_var.bias, "none")
        return LinearFunction.apply(rs, model.rs_to_mu.weight, model.rs_to_mu.bias, "none"), lv
    return rs, None


def _absorb(model, state, images, labels, add, wq):
    """`add[t]` of the slots of images / labels [T, n, ...] into the summary state (state None: a fresh one): only those shots are
    encoded, as a packed list, and nothing absorbed earlier is read again."""
    T, n = model.task_num, images.shape[1]
    plan = ragged.Plan((0,) * T, add, n, n, images.device)
    keys = None if state is None else state.keys
    if plan.n:
        imgs = ragged.pack(images.reshape(T, n, model.img_channels, model.img_size[0], model.img_size[1]), plan.src)
        new_k, new_v = _shot_rows(model, imgs, ragged.pack(labels.reshape(T, n, -1), plan.src))
        keys = ragged.summary_absorb(keys, new_k, new_v, plan, T, n, model.attn.projection_matrix, add)
    total = keys.lens
    return VanillaContextState(model, T, max(total), _fingerprint(model), "attention", keys=keys, wq=wq, lens=total, form="summary")


def _grow(model, state, lens, capacity, images, labels, add, wq):
    """`add[t]` of the slots of images / labels [T, n, ...] behind task t's lens[t] kept rows (state None: nothing kept yet), then the
    finishing step on the kept rows.  The valid shots travel as a packed list: a slot that is no shot is never read."""
    T, dev = model.task_num, images.device
    plan = ragged.Plan(lens, add, images.shape[1], capacity, dev)
    total = plan.total
    a_rows, b_rows = (None, None) if state is None else (state.kh, state.vh) if model.ATTENTION else (state.rs, state.lv)
    if state is not None and a_rows is None:
        raise ValueError("extend: the state carries no per-shot rows (it was not made by condition())")
    if plan.n:
        src, dst = plan.src, plan.dst
        imgs = ragged.pack(images.reshape(T, images.shape[1], model.img_channels, model.img_size[0], model.img_size[1]), src)
        new_a, new_b = _shot_rows(model, imgs, ragged.pack(labels.reshape(T, images.shape[1], -1), src))
        if state is None:
            a_rows = torch.zeros(T, capacity, *new_a.shape[1:], device=dev)
            b_rows = torch.zeros_like(a_rows) if new_b is not None else None
        a_rows = ragged.scatter(a_rows, dst, new_a)
        b_rows = ragged.scatter(b_rows, dst, new_b) if new_b is not None else None
    if model.ATTENTION:
        keys = ragged.masked_keys(a_rows, model.attn.projection_matrix, plan)
        return VanillaContextState(model, T, capacity, _fingerprint(model), "attention", keys=keys, vh=b_rows, wq=wq, lens=total, kh=a_rows)
    r = ragged.gathered_aggregate(model.agg_mode, a_rows, b_rows, plan)
    z = LinearFunction.apply(r, model.r_to_z.weight, model.r_to_z.bias, "none")
    return VanillaContextState(model, T, capacity, _fingerprint(model), "latent", z=z, lens=total, rs=a_rows, lv=b_rows, r=r)


def predict(model, state, qry_x, chunk=None, route=None):
    """(state, target images [T, Nq, ...]) -> mu [T, Nq, y_dim] = `model(ctx, labels, targets, test=True)[0]` for the context the
    state was made from, any Nq >= 1.  `chunk` bounds the targets per launch sequence (and the encoder's activations with them).
    `route`: None picks "fused" where mlhot_np_query_supported says yes and "composed" otherwise; a test may force either.  The
    state's `route` says which one ran."""
    if isinstance(model, ResNetNP):
        if route is not None:
            raise ValueError("predict: route= belongs to the vanilla family")
        return model.predict(state, qry_x, chunk=chunk)
    _refuse(model, "predict")
    if not isinstance(state, VanillaContextState) or state.owner is not model:
        raise ValueError("predict: the state was not made by this model's condition()")
    if qry_x.shape[0] != state.T or state.T != model.task_num:
        raise ValueError(f"predict: the state holds {state.T} tasks, the targets {qry_x.shape[0]} (the key stabiliser is the maximum "
                         "over the conditioned batch: predict serves the same tasks)")
    if state.fingerprint != _fingerprint(model):
        raise ValueError("predict: the state is stale - a parameter of the model changed since condition()")
    Nq = qry_x.shape[1]
    if Nq < 1:
        raise ValueError("predict needs at least one target")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"predict: chunk must be a positive number of targets, got {chunk}")
    if route is not None and route not in ROUTES:
        raise ValueError(f"predict: route must be one of {ROUTES}, got {route!r}")
    if state.form == "summary":
        if route == "fused":
            raise ValueError('predict: route "fused" - mlhot_np_query_fwd reads per-shot key features; a summary state is served by '
                             "the composed route (linear_rows and favor_query)")
        route = "composed"
    _need_gpu(qry_x)
    dims = model._dims(state.Nc, 1)
    if route is None:
        route = "fused" if lib().np_query_supported(dims) and (state.keys is None or state.keys.route == "cached") else "composed"
        if route == "composed" and type(model).__name__ not in _logged:
            _logged.add(type(model).__name__)
            logging.getLogger(__name__).info("mlhot.cached.predict: %s's dimensions are outside mlhot_np_query_fwd's envelope; the query tail "
                                             "runs composed from linear_rows / favor_query", type(model).__name__)
    state.route = route
    step = Nq if chunk is None else min(int(chunk), Nq)
    with torch.no_grad():
        out = [_predict_targets(model, state, qry_x[:, i:i + step], dims, route) for i in range(0, Nq, step)]
    return out[0] if len(out) == 1 else torch.cat(out, dim=1)


def _rows(sources, lin_w, lin_b, act):
    """linear_rows, or - for a layer it does not serve (logged once) - LinearFunction on the gathered rows."""
    k0, k1 = sources[0][0].shape[1], sources[1][0].shape[1] if len(sources) > 1 else 0
    if lib().linear_rows_supported(k0, k1, lin_w.shape[0]):
        return linear_rows(sources, lin_w, lin_b, act)
    if (k0, k1, lin_w.shape[0]) not in _logged:
        _logged.add((k0, k1, lin_w.shape[0]))
        logging.getLogger(__name__).info("mlhot.cached.predict: no row-invariant kernel for a Linear [%d | %d] -> %d", k0, k1, lin_w.shape[0])
    x = torch.cat([x.repeat_interleave(rep, dim=0) if rep > 1 else x for x, rep, _ in sources], dim=1)
    return LinearFunction.apply(x, lin_w, lin_b, act)


def composed_tail(params, x_qry, T, Nq, tanh, keys=None, vh=None, proj=None, z=None, wq=None):
    """The query tail from the existing row-invariant operators - the yardstick of the fused launch and the route for dimensions
    it does not serve.  params: state_dict key -> tensor; x_qry [T * Nq, dim_w]; attention: keys (FavorKeyState), vh, proj (wq: the
    stacked _W_q weight and bias, else stacked here); otherwise z [T, dim_z].  -> mu [T, Nq, y_dim]."""
    def lin(sources, name, act="none"):
        return _rows(sources, params[name + ".weight"], params[name + ".bias"], act)
    if keys is not None:
        w, b = wq if wq is not None else (torch.cat([params[f"_W_q.{i}.linear.weight"] for i in range(HEADS)]),
                                          torch.cat([params[f"_W_q.{i}.linear.bias"] for i in range(HEADS)]))
        qh = _rows([(x_qry, 1, 0)], w, b, "none").view(T, Nq, HEADS, -1)
        merged = favor_query(qh, keys, vh, proj).view(T * Nq, -1)
        zq = lin([(lin([(merged, 1, 0)], "_W.linear"), 1, 0)], "r_to_z")
        h = lin([(x_qry, 1, 0), (zq, 1, 0)], "decoder0.0", "relu")
    else:
        h = lin([(x_qry, 1, 0), (z, Nq, 0)], "decoder0.0", "relu")
    h = lin([(h, 1, 0)], "decoder0.2", "relu")
    return lin([(h, 1, 0)], "decoder0.4", "tanh" if tanh else "none").view(T, Nq, -1)


def _long_tail(params, x_qry, T, Nq, tanh, favor, kh, vh, proj, wq, ks):
    """composed_tail for the prefixes `ks` of an attention context of any length: the query heads once, `favor` (favor_prefixes_long)
    once for all prefixes, then every Linear once over the len(ks) * T * Nq rows - row-invariant, so a row has composed_tail's bits."""
    def lin(sources, name, act="none"):
        return _rows(sources, params[name + ".weight"], params[name + ".bias"], act)
    qh = _rows([(x_qry, 1, 0)], wq[0], wq[1], "none").view(T, Nq, HEADS, -1)
    merged = favor(qh, kh, vh, proj, ks).view(len(ks) * T * Nq, -1)
    zq = lin([(lin([(merged, 1, 0)], "_W.linear"), 1, 0)], "r_to_z")
    h = lin([(x_qry, 1, T * Nq), (zq, 1, 0)], "decoder0.0", "relu")
    h = lin([(h, 1, 0)], "decoder0.2", "relu")
    return lin([(h, 1, 0)], "decoder0.4", "tanh" if tanh else "none").view(len(ks), T, Nq, -1)


def _predict_targets(model, state, qry_x, dims, route):
    T, Nq = qry_x.shape[0], qry_x.shape[1]
    x_qry = _encode(model, qry_x)
    proj = _c(model.attn.projection_matrix) if model.ATTENTION else None
    params = {k: _c(p.detach()) for k, p in model.named_parameters()}
    if state.kind != "attention":
        if route == "fused":
            return lib().np_query_fwd(dims, params, x_qry.view(T, Nq, -1), z=state.z)
        return composed_tail(params, x_qry, T, Nq, model.OUT_TANH, z=state.z)
    if route == "fused":
        return lib().np_query_fwd(dims, params, x_qry.view(T, Nq, -1), key_state=state.keys.buf, vh=state.vh, proj=proj)
    return composed_tail(params, x_qry, T, Nq, model.OUT_TANH, keys=state.keys, vh=state.vh, proj=proj, wq=state.wq)


# ---- prefix sweep for the vanilla family ---------------------------------------------------------------------------
def supports_sweep(model):
    """(bool, reason): whether `sweep` serves this model, and through what - or why not."""
    if isinstance(model, ResNetNP):
        if model.PREFIX_SWEEP_REFUSAL:
            return False, _FRESH_WEIGHTS
        return True, "ResNetNP.forward_prefixes"
    if type(model).forward is VanillaNP.forward:
        return True, "the vanilla family's prefix sweep (mlhot_np_prefix_fwd)"
    if isinstance(model, VanillaMR):
        return False, _FRESH_WEIGHTS
    return False, "the prefix sweep is not built for this class"


def _sweep_ks(ks, Nc):
    if ks is None:
        return tuple(range(1, Nc + 1))
    if isinstance(ks, torch.Tensor):
        if ks.is_cuda or ks.is_floating_point() or ks.dtype == torch.bool or ks.dim() != 1:
            raise ValueError("sweep: ks must be a host sequence of integers (its values are checked on the host)")
        ks = ks.tolist()
    try:
        ks = list(ks)
    except TypeError:
        raise ValueError(f"sweep: ks must be a sequence of context sizes, got {type(ks).__name__}") from None
    if any(isinstance(k, bool) or not isinstance(k, numbers.Integral) for k in ks):
        raise ValueError(f"sweep: ks must hold integers, got {ks}")
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1 or max(ks) > Nc or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"sweep: ks must be strictly increasing context sizes in 1..{Nc}, got {list(ks)}")
    return ks


def sweep(model, ctx_x, ctx_y, qry_x, ks=None, route=None):
    """(ctx images [T, Nc, ...], ctx labels [T, Nc, L], target images [T, Nq, ...]) -> mu [len(ks), T, Nq, y_dim]: row i equals
    `model(ctx_x[:, :ks[i]], ctx_y[:, :ks[i]], qry_x, test=True)[0]` to the kernels' tolerance.  `ks`: strictly increasing context
    sizes in 1..Nc (host ints; default 1..Nc).  ONE encoder pass over the context and target images together, the per-shot Linears
    of `condition`, then route "fused": the prefix aggregate through r_to_z (mean / max / baco) or the key-side launches (attention,
    inside the call) and ONE mlhot_np_prefix_fwd launch for all prefixes (csrc/np_prefix.h); or route "composed", the parent
    operators alone: per k the masked state `condition(ctx_len=[k] * T)` builds and `composed_tail` - the yardstick, and the route
    for dimensions outside the kernel's envelope.  `route=None` picks fused where mlhot_np_prefix_supported says yes; a forced
    "fused" outside the envelope is an error.  Eval mode only.  A ResNetNP model goes to its forward_prefixes.

    An attention model with Nc > 32 runs composed with mlhot.ops.favor_prefixes_long in place of the per-prefix
    FAVOR+ stage: the shots are walked once in chunks of 32 for all of `ks`, and the Linears behind it run once over the rows of all
    prefixes through linear_rows - bit-equal however `ks` is split; route "fused" is an error there.  `sweep.last_attention` says
    which FAVOR+ stage the last attention sweep ran: "np_prefix" | "favor_keys" | "prefix_long"."""
    if isinstance(model, ResNetNP):
        if route is not None:
            raise ValueError("sweep: route= belongs to the vanilla family")
        return model.forward_prefixes(ctx_x, ctx_y, qry_x, ks=ks)
    ok, reason = supports_sweep(model)
    if not ok:
        raise ValueError(f"{type(model).__name__}: mlhot.cached.sweep: {reason}")
    if model.training:
        raise ValueError("sweep is a test-mode path: call model.eval() first")
    T, Nc, Nq = ctx_x.shape[0], ctx_x.shape[1], qry_x.shape[1]
    if T != model.task_num or qry_x.shape[0] != T or ctx_y.shape[0] != T:
        raise ValueError(f"sweep: {T} context and {qry_x.shape[0]} target tasks, the model was built for tasks_per_batch = {model.task_num}")
    if Nc < 1 or Nq < 1 or ctx_y.shape[1] != Nc:
        raise ValueError(f"sweep needs at least one context shot with its label and one target (got {Nc} shots, {ctx_y.shape[1]} labels, {Nq} targets)")
    ks = _sweep_ks(ks, Nc)
    if route is not None and route not in ROUTES:
        raise ValueError(f"sweep: route must be one of {ROUTES}, got {route!r}")
    model._check_agg()
    _need_gpu(ctx_x, ctx_y, qry_x, *model.parameters())
    K = len(ks)
    dims = model._dims(Nc, 1)
    long_ctx = model.ATTENTION and Nc > ragged.MAX_ATTENTION_CAPACITY
    if long_ctx and route == "fused":
        raise ValueError(f"sweep: route 'fused' - mlhot_np_prefix_fwd serves at most {ragged.MAX_ATTENTION_CAPACITY} context shots (got {Nc}); "
                         "a longer attention context runs composed, with mlhot.ops.favor_prefixes_long")
    served = not long_ctx and lib().np_prefix_supported(dims, K)
    if route == "fused" and not served:
        raise ValueError(f"sweep: route 'fused' - {type(model).__name__}'s dimensions are outside mlhot_np_prefix_fwd's envelope")
    if route is None:
        route = "fused" if served else "composed"
        if route == "composed" and not long_ctx and ("sweep", type(model).__name__) not in _logged:
            _logged.add(("sweep", type(model).__name__))
            logging.getLogger(__name__).info("mlhot.cached.sweep: %s's dimensions are outside mlhot_np_prefix_fwd's envelope; the sweep runs "
                                             "composed, one masked state and one composed tail per context size", type(model).__name__)
    sweep.last_route = route
    dev = ctx_x.device
    with torch.no_grad():
        # the host's one upload goes out before the first launch (an upload from pageable memory waits for the stream)
        up = None
        if route == "composed" and not long_ctx:
            up = torch.tensor([[k] * T for k in ks] if model.ATTENTION else [[(k - 1) * T + t for t in range(T)] for k in ks], dtype=torch.int32).to(dev)
        elif not model.ATTENTION and K != Nc:
            up = torch.tensor([k - 1 for k in ks], dtype=torch.int32).to(dev)
        shape = (-1, model.img_channels, model.img_size[0], model.img_size[1])
        x_ctx, x_qry, _ = lib().enc_vanilla_fwd(_c(ctx_x.reshape(shape).float()), _c(qry_x.reshape(shape).float()), _enc_params(model), model.dim_w)
        ly = LinearFunction.apply(ctx_y.reshape(T * Nc, -1), model.transform_y.weight, model.transform_y.bias, "none")
        rs = model.encoder_r(torch.cat([x_ctx, ly], dim=1))
        proj = _c(model.attn.projection_matrix) if model.ATTENTION else None
        params = {k: _c(p.detach()) for k, p in model.named_parameters()}
        if model.ATTENTION:
            kh = _c(LinearFunction.apply(x_ctx, *_stacked(model._W_k), "none").view(T, Nc, HEADS, -1))
            vh = _c(LinearFunction.apply(rs, *_stacked(model._W_v), "none").view(T, Nc, HEADS, -1))
            sweep.last_attention = "prefix_long" if long_ctx else "np_prefix" if route == "fused" else "favor_keys"
            if route == "fused":
                return lib().np_prefix_fwd(dims, params, x_qry.view(T, Nq, -1), ks, kh=kh, vh=vh, proj=proj)
            wq = _stacked(model._W_q)
            if long_ctx:
                return _long_tail(params, x_qry, T, Nq, model.OUT_TANH, favor_prefixes_long, kh, vh, proj, wq, ks)
            return torch.stack([composed_tail(params, x_qry, T, Nq, model.OUT_TANH, keys=favor_keys(kh, proj, lens=(k,) * T, lens_dev=up[i]), vh=vh,
                                              proj=proj, wq=wq) for i, k in enumerate(ks)])
        lv = None
        if model.agg_mode == "baco":
            lv = LinearFunction.apply(rs, model.rs_to_var.weight, model.rs_to_var.bias, "none").view(T, Nc, -1)
            rs = LinearFunction.apply(rs, model.rs_to_mu.weight, model.rs_to_mu.bias, "none")
        r = agg_prefixes(model.agg_mode, rs.view(T, Nc, -1), lv)                          # [Nc, T, R]
        if route == "fused":
            if up is not None:
                r = r.index_select(0, up.long())
            z = _rows([(r.reshape(K * T, -1), 1, 0)], model.r_to_z.weight.detach(), model.r_to_z.bias.detach(), "none")
            return lib().np_prefix_fwd(dims, params, x_qry.view(T, Nq, -1), ks, z=z.view(K, T, -1))
        out = []
        for i in range(K):                                                                # ragged.gathered_aggregate's rows, then condition's r_to_z
            rk = r.view(Nc * T, -1).index_select(0, up[i].long())
            z = LinearFunction.apply(rk, model.r_to_z.weight, model.r_to_z.bias, "none")
            out.append(composed_tail(params, x_qry, T, Nq, model.OUT_TANH, z=z))
        return torch.stack(out)


sweep.last_route = None
sweep.last_attention = None
