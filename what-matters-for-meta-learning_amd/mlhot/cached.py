"""Cached-context inference as functions: `condition` once, `predict` for any targets.

    state = mlhot.cached.condition(model, ctx_x, ctx_y, ctx_len=None, capacity=None, form="keys")     # "summary": beyond 32 shots (6c-4)
                                                                    # "long": per-shot rows for up to 256 shots, attention read-out (6c-7)
                                                                    # "paged": the same for up to 4096 shots (6c-11)
    state = mlhot.cached.extend(model, state, new_x, new_y, new_len=None)        # more context shots, only they are encoded (6c-3)
    state = mlhot.cached.evict(model, state, drop)                  # drop[t]: the slots task t lets go; no image is encoded (6c-12)
    state = mlhot.cached.retract(model, state, old_x, old_y, old_len=None)       # the same for a summary: the old shots are handed in
    state = mlhot.cached.slide(model, state, new_x, new_y, new_len=None)         # a window: the oldest shots go, the new ones come
    state = mlhot.cached.merge(model, [state_a, state_b, ..])       # summary states conditioned apart -> one, no image re-read (6c-6)
    state = mlhot.cached.select(model, [state_a, state_b, ..], picks)      # a batch put together from the TASKS of summary states:
                                                                    # picks[t] = (state, task) or a list of such pairs (6c-8)
    state = mlhot.cached.concat(model, [state_a, state_b, ..], form=None, capacity=None)      # per-shot or latent states conditioned apart
                                                                    # -> one: rows are copied by one launch, none recomputed (6c-13)
    state = mlhot.cached.regroup(model, [state_a, state_b, ..], picks, form=None, capacity=None)     # select's picks for those states
    state = mlhot.cached.summarize(model, state)                    # a per-shot attention state -> form="summary", for merge / select
    mu = mlhot.cached.predict(model, state, qry_x, chunk=None)        # [T, Nq, y_dim]
    mu, attn = mlhot.cached.predict(model, state, qry_x, return_attention=True)      # attn [T, 8, Nq, Nc slots]: FAVOR+'s weight per context
                                                                                      # slot, head and target (attention models; 6c-5)
    mu = mlhot.cached.predict(model, state, qry_x, context_mask=mask)     # mask bool [T, Nq, Nc slots]: every target attends to its own
                                                                    # subset of the context; [T, G, Nq, Nc] -> mu [T, G, Nq, y_dim], G masks
                                                                    # of the same targets from one encoder pass and one query launch (6c-10)
    mu = mlhot.cached.leave_one_out(model, state, qry_x)            # [T, Nc slots, Nq, y_dim]: group c predicts without context slot c
    mu, mass = mlhot.cached.predict(model, state, qry_x, attention_mass=True, target_weight=None)     # mass [T, 8, Nc slots]: attn summed over
                                                                    # the targets inside the query launch, attn never stored (6c-14)
    state, drop = mlhot.cached.prune(model, state, qry_x, keep)     # keep[t] slots with the largest mass stay, the rest go through evict
    mu, idx, w = mlhot.cached.predict(model, state, qry_x, top_k=8) # [T, 8, Nq, k]: the k heaviest context slots per head and target (6c-15)
    mu = mlhot.cached.predict(model, state, qry_x, shared_targets=True)   # qry_x [Nq, ...] without a task axis: one frame asked of all T
                                                                    # stored contexts, encoded once, F_q formed once -> [T, Nq, y_dim] (6c-16)
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
The state class and the lifecycle (entry checks, growth, absorption, the chunk loop) are mlhot/context.py's, shared with ResNetNP;
this module supplies the vanilla family's adapter (_Vanilla).
"""
import logging
import numbers

import torch

from mlhot import context, lib, ragged
from mlhot.binding import HEADS
from mlhot.context import ContextState as VanillaContextState          # noqa: F401  one class for both families; the name stays importable
from mlhot.context import fingerprint as _fingerprint                  # noqa: F401
from mlhot.ops import LinearFunction, _c, _need_gpu, agg_prefixes, favor_keys, favor_prefixes_long, favor_query, linear_rows, linear_rows_any
from networks._resnet_np import ResNetNP, _CachedContext
from networks._vanilla import VanillaNP
from networks._vanilla_mr import VanillaMR

ROUTES = ("fused", "composed", "fused_summary")      # predict's; "fused_summary" is opt-in, never picked by route=None
SWEEP_ROUTES = ("fused", "composed")                  # sweep's own two
_FRESH_WEIGHTS = ("Bayes-by-backprop draws fresh weights in every forward, so a cached context is not the reference's forward")
# what serves a family (_family) at each entry point, or why nothing does
_CACHED = {"resnet": "ResNetNP.condition / predict", "vanilla": "the vanilla family's query tail (mlhot_np_query_fwd)",
           "fresh": _FRESH_WEIGHTS, None: "cached-context inference is not built for this class"}
_SWEEP = {"resnet": "ResNetNP.forward_prefixes", "vanilla": "the vanilla family's prefix sweep (mlhot_np_prefix_fwd)",
          "fresh": _FRESH_WEIGHTS, None: "the prefix sweep is not built for this class"}
_logged = set()


def _family(model):
    """"resnet" | "vanilla": who serves the model; "fresh": a Bayes-by-backprop class of either; None: another class."""
    if isinstance(model, ResNetNP):
        return "fresh" if model.PREFIX_SWEEP_REFUSAL else "resnet"
    if type(model).forward is VanillaNP.forward:
        return "vanilla"
    return "fresh" if isinstance(model, VanillaMR) else None


def supports(model):
    """(bool, reason): whether condition / predict serve this model, and through what - or why not."""
    family = _family(model)
    return family in ("resnet", "vanilla"), _CACHED[family]


def supports_sweep(model):
    """(bool, reason): whether `sweep` serves this model, and through what - or why not."""
    family = _family(model)
    return family in ("resnet", "vanilla"), _SWEEP[family]


def _refuse(model, what, reasons=_CACHED):
    family = _family(model)
    if family not in ("resnet", "vanilla"):
        raise ValueError(f"{type(model).__name__}: mlhot.cached.{what}: {reasons[family]}")
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


def _encoded_rows(model, x_ctx, labels, invariant=False):
    """The per-shot stage behind the encoder: its rows x_ctx [P, dim_w], labels [P, L] -> (kh, vh) [P, 8, dim_w] for the attention
    models, (rs, lv) [P, R] for the others (baco: rs_to_mu's and rs_to_var's outputs, rs_to_var first; else lv None)."""
    if invariant:                    # form "paged" (DESIGN.md 6c-11): every Linear row-invariant, attention models
        ly = linear_rows_any([(labels, 1, 0)], model.transform_y.weight, model.transform_y.bias)
        lins = model.encoder_r.linears()
        rs = linear_rows_any([(x_ctx, 1, 0), (ly, 1, 0)], lins[0].weight, lins[0].bias, "relu" if len(lins) > 1 else "none")
        for i, lin in enumerate(lins[1:], 1):
            rs = linear_rows_any([(rs, 1, 0)], lin.weight, lin.bias, "relu" if i < len(lins) - 1 else "none")
        return (linear_rows_any([(x_ctx, 1, 0)], *_stacked(model._W_k)).view(-1, HEADS, model.dim_w),
                linear_rows_any([(rs, 1, 0)], *_stacked(model._W_v)).view(-1, HEADS, model.dim_w))
    ly = LinearFunction.apply(labels, model.transform_y.weight, model.transform_y.bias, "none")
    rs = model.encoder_r(torch.cat([x_ctx, ly], dim=1))
    if model.ATTENTION:
        return (LinearFunction.apply(x_ctx, *_stacked(model._W_k), "none").view(-1, HEADS, model.dim_w),
                LinearFunction.apply(rs, *_stacked(model._W_v), "none").view(-1, HEADS, model.dim_w))
    if model.agg_mode == "baco":
        lv = LinearFunction.apply(rs, model.rs_to_var.weight, model.rs_to_var.bias, "none")
        return LinearFunction.apply(rs, model.rs_to_mu.weight, model.rs_to_mu.bias, "none"), lv
    return rs, None


def _shot_rows(model, imgs, labels, invariant=False):
    """The per-shot part of condition for a packed list of P shots: images [P, 1, 128, 128], labels [P, L] -> _encoded_rows."""
    return _encoded_rows(model, _encode(model, imgs), labels, invariant)


class _Vanilla:
    """mlhot.context's adapter for the vanilla family; `route` is what predict's caller asked for."""

    def __init__(self, model, route=None, attention=False):
        # attention: False, or the keyword that asks for per-shot weights, as the refusals name it
        self.model, self.asked, self.dims, self.attention = model, route, None, "return_attention=True" if attention is True else attention
        self.masked = False          # context.predict sets it for predict(context_mask=)

    finish = property(lambda self: self.model.r_to_z)

    def refuse(self, what):
        _refuse(self.model, what)

    def prepare(self, *tensors):
        _need_gpu(*tensors, *self.model.parameters())

    def begin(self, launches):
        if launches:
            self.model._check_agg()
        return _stacked(self.model._W_q) if self.model.ATTENTION else None

    def shot_rows(self, imgs, labels, invariant=False):
        return _shot_rows(self.model, imgs, labels, invariant)

    def empty_z(self, device):
        return torch.zeros(self.model.task_num, self.model.dim_z, device=device)

    def route(self, state, qry_x):
        model, route = self.model, self.asked
        if route is not None and route not in ROUTES:
            raise ValueError(f"predict: route must be one of {ROUTES}, got {route!r}")
        if self.masked:              # the one-launch tails take no mask
            if route in ("fused", "fused_summary"):
                raise ValueError(f'predict: context_mask= with route "{route}" - the one-launch tails keep S inside their launch and stay as '
                                 "they are; per-target context masks run the composed route (linear_rows and favor_query)")
            route = "composed"
        if route == "fused_summary":             # opt-in, an error where it cannot run - never another route
            self._route_fused_summary(state, qry_x)
            return
        if self.attention:           # the one-launch tail forms no weights to read out
            if route == "fused":
                raise ValueError(f'predict: {self.attention} with route "fused" - mlhot_np_query_fwd keeps S and D inside its one launch '
                                 "and stays as it is; the attention read-out runs the composed route (linear_rows and favor_query)")
            route = "composed"
        if state.form == "summary":
            if route == "fused":
                raise ValueError('predict: route "fused" - mlhot_np_query_fwd reads per-shot key features; a summary state is served by '
                                 'the composed route (linear_rows and favor_query) or, on request, by route "fused_summary"')
            route = "composed"
        if state.form == "long":
            if route == "fused":
                raise ValueError('predict: route "fused" - mlhot_np_query_fwd reads at most 32 context slots in one chunk; a long state is '
                                 "served by the composed route (linear_rows and favor_query)")
            route = "composed"
        if state.form == "paged":
            if route == "fused":
                raise ValueError('predict: route "fused" - mlhot_np_query_fwd reads at most 32 context slots in one chunk; a paged state is '
                                 "served by the composed route (linear_rows and favor_query)")
            route = "composed"
        _need_gpu(qry_x)
        self.dims = model._dims(state.Nc, 1)
        if route is None:
            route = "fused" if lib().np_query_supported(self.dims) and (state.keys is None or state.keys.route == "cached") else "composed"
            if route == "composed" and type(model).__name__ not in _logged:
                _logged.add(type(model).__name__)
                logging.getLogger(__name__).info("mlhot.cached.predict: %s's dimensions are outside mlhot_np_query_fwd's envelope; the query tail "
                                                 "runs composed from linear_rows / favor_query", type(model).__name__)
        state.route = route

    def _route_fused_summary(self, state, qry_x):
        """The checks of route "fused_summary" (mlhot_np_query_summary_fwd): every refusal is a ValueError before any launch."""
        model = self.model
        if self.attention:           # context.predict has refused a summary state already; this is the wording for every other form
            raise ValueError(f'predict: {self.attention} with route "fused_summary" - a summary state keeps no per-shot rows, so there is '
                             "no weight per context shot to read out")
        if state.form != "summary":
            what = {"empty": "empty", "latent": "latent"}.get(state.kind, state.form)
            serves = {"keys": 'route "fused" (mlhot_np_query_fwd) or "composed"', "long": 'route "composed" (linear_rows and favor_query)',
                      "paged": 'route "composed" (linear_rows and favor_query)',
                      "latent": 'route "fused" (mlhot_np_query_fwd on z) or "composed"', "empty": 'route "fused" (mlhot_np_query_fwd on z) or "composed"'}[what]
            raise ValueError(f'predict: route "fused_summary" reads a FAVOR+ summary state (condition(form="summary"), extend, merge, select); this state '
                             f"is {what!r} and is served by {serves}")
        if min(state.lens) < 1:
            raise ValueError(f'predict: route "fused_summary" - a task of the summary state has absorbed no shot (shots per task: {list(state.lens)}): '
                             "its attention is 0 / 0")
        _need_gpu(qry_x)
        self.dims = model._dims(state.Nc, 1)
        if not lib().np_query_summary_supported(self.dims):
            raise ValueError(f'predict: route "fused_summary" - {type(model).__name__}\'s dimensions are outside mlhot_np_query_summary_fwd\'s envelope '
                             f"(dim_w={self.dims.dim_w} dim_r={self.dims.dim_r} dim_z={self.dims.dim_z} dec_hidden={self.dims.dec_hidden} "
                             f"y_dim={self.dims.y_dim} m={self.dims.m_feat}); the composed route serves them")
        state.route = "fused_summary"

    def route_shared(self, state, imgs):
        """predict(shared_targets=True): the composed route, whose linear_rows sources broadcast the shared rows."""
        if self.asked is not None and self.asked not in ROUTES:
            raise ValueError(f"predict: route must be one of {ROUTES}, got {self.asked!r}")
        if self.asked in ("fused", "fused_summary"):
            raise ValueError(f'predict: shared_targets=True with route "{self.asked}" - the one-launch tails read one target set per task and '
                             "stay as they are; shared targets run the composed route (linear_rows and favor_query(shared=True))")
        _need_gpu(imgs)
        self.dims = self.model._dims(state.Nc, 1)
        state.route = "composed"

    def predict_shared(self, state, imgs, attention=False):
        model = self.model
        x_qry = _encode(model, imgs)                 # [n, dim_w]: the n shared targets, once
        params = {k: _c(p.detach()) for k, p in model.named_parameters()}
        if state.kind != "attention":
            return composed_tail(params, x_qry, state.T, imgs.shape[0], model.OUT_TANH, z=state.z, shared=True)
        return composed_tail(params, x_qry, state.T, imgs.shape[0], model.OUT_TANH, keys=state.keys, vh=state.vh,
                             proj=_c(model.attn.projection_matrix), wq=state.wq, weights=attention, shared=True)

    def predict_targets(self, state, qry_x, attention=False, mask_words=None, target_weight=None):
        model, T, Nq = self.model, qry_x.shape[0], qry_x.shape[1]
        x_qry = _encode(model, qry_x)
        proj = _c(model.attn.projection_matrix) if model.ATTENTION else None
        params = {k: _c(p.detach()) for k, p in model.named_parameters()}
        if mask_words is not None:   # G masked read-outs of one query pass, then the tail over the G * T * Nq rows
            G, att = mask_words.shape[1], []

            def favor(qh):
                res = favor_query(qh, state.keys, state.vh, proj, weights=attention, mask=mask_words)
                if attention:
                    att.append(res[1])
                    res = res[0]
                return res.transpose(0, 1).contiguous()               # [G, T, Nq, d*H]: the target rows wrap every T * Nq, as for prefixes
            mu = composed_tail(params, x_qry, T, Nq, model.OUT_TANH, wq=state.wq, favor=favor, prefixes=G).transpose(0, 1).contiguous()
            return (mu, att[0]) if attention else mu
        if state.kind != "attention":
            if state.route == "fused":
                return lib().np_query_fwd(self.dims, params, x_qry.view(T, Nq, -1), z=state.z)
            return composed_tail(params, x_qry, T, Nq, model.OUT_TANH, z=state.z)
        if state.route == "fused":
            return lib().np_query_fwd(self.dims, params, x_qry.view(T, Nq, -1), key_state=state.keys.buf, vh=state.vh, proj=proj)
        if state.route == "fused_summary":
            return lib().np_query_summary_fwd(self.dims, params, x_qry.view(T, Nq, -1), state.keys.buf, proj)
        return composed_tail(params, x_qry, T, Nq, model.OUT_TANH, keys=state.keys, vh=state.vh, proj=proj, wq=state.wq, weights=attention,
                             target_weight=target_weight)


def condition(model, ctx_x, ctx_y, ctx_len=None, capacity=None, form="keys"):
    """(ctx images [T, Nc, ...], ctx labels [T, Nc, L]) -> the state for predict: ResNetNP.condition for that family; for the
    vanilla family the encoder, transform_y and encoder_r, then the key / value heads and mlhot.ops.favor_keys (attention) or the
    aggregation and r_to_z (mean / max / baco) - mlhot.context.condition with this module's per-shot stage.  No new kernel; the row
    count is T * Nc whatever follows.

    `ctx_len` (T host ints, 1 .. Nslots): the images are [T, Nslots, ...] and task t's context is its first ctx_len[t] slots; the other
    slots' images and labels are never read.  `capacity` >= Nslots reserves empty slots for extend (default Nslots; an attention
    model takes at most 32).  Without either argument this is the call it always was.

    `form="summary"` (attention models): the state is FAVOR+'s fixed-size summary of the context - any number of
    shots, `ctx_len` honoured, no `capacity`, no per-shot rows kept; extend absorbs any number of further shots and predict runs
    the composed route, or - on request, `predict(route="fused_summary")`, vanilla family - the one-launch tail on the summary
    (mlhot_np_query_summary_fwd).  The default "keys" is every call as it was.

    `form="long"` (attention models): per-shot key features for up to 256 slots (`capacity` defaults to Nslots),
    everything of "keys" - `ctx_len`, `capacity`, extend, `return_attention=True` - through the chunked kernels of
    csrc/favor_long.h; predict runs the composed route.  It is the form that returns attention weights above 32 shots.

    `form="paged"` (attention models): everything of "long" for up to 4096 slots - `ctx_len`, `capacity`, extend,
    `return_attention=True`, `context_mask=` and leave_one_out - the query walking the slots in pages of 256 (csrc/favor_paged.h);
    predict runs the composed route, a forced "fused" or "fused_summary" is a ValueError.  Never a default: ask for it."""
    ragged.check_form("condition", form)
    if isinstance(model, ResNetNP):
        if form != "keys":
            return model.condition(ctx_x, ctx_y, ctx_len=ctx_len, capacity=capacity, form=form)
        if ctx_len is None and capacity is None:
            return model.condition(ctx_x, ctx_y)                  # today's call, as it always went out
        return model.condition(ctx_x, ctx_y, ctx_len=ctx_len, capacity=capacity)
    return context.condition(_Vanilla(model), ctx_x, ctx_y, ctx_len, capacity, form)


def extend(model, state, new_x, new_y, new_len=None):
    """(state, new ctx images [T, n, ...], their labels [T, n, L], new_len) -> a NEW state whose task t holds new_len[t] more context
    shots (0 .. n each; default n), written behind its current ones; the old state stays valid.  Only the new shots are encoded;
    then the masked key launches (attention) or the prefix aggregate with its gather and r_to_z (latent) run on the kept rows.  A
    state needs spare slots: condition with capacity=.  ResNetNP: model.extend."""
    if isinstance(model, ResNetNP):
        return model.extend(state, new_x, new_y, new_len=new_len)
    return context.extend(_Vanilla(model), state, new_x, new_y, new_len)


def _adapter(model):
    return _CachedContext(model) if isinstance(model, ResNetNP) else _Vanilla(model)


def evict(model, state, drop):
    """(per-shot or latent state, drop) -> a NEW state without the context shots in the slots `drop[t]` of task t.
    `drop` is a sequence of T sequences of host ints: distinct slot indices below `state.lens[t]`, possibly none.  Capacity, form and
    kind stay; `lens[t]` shrinks by `len(drop[t])`; the kept shots move to the front in their order and the freed slots behind them
    are zero rows, exactly as `condition(ctx_len=, capacity=)` leaves spare slots, so `extend`, `predict`, `return_attention=True`,
    `context_mask=` and `leave_one_out` serve the result like any state of its form.  The old state stays valid.  No image is
    encoded again: ONE launch (mlhot_rows_compact) moves the kept rows of both row sets, then the state's own key launches run with
    the new lens - the key stabiliser is the maximum over the shots that remain, exactly what a fresh `condition` computes
    (attention) - or extend's finishing steps, the prefix aggregate with its gather and r_to_z (latent).  Both families; eval
    mode.  Refused with ValueError before anything touches the GPU: a foreign or stale state or one of another T, a summary or
    empty state, an index out of range or named twice, a `drop` that leaves a task without a shot.  ResNetNP: model.evict."""
    if isinstance(model, ResNetNP):
        return model.evict(state, drop)
    return context.evict(_Vanilla(model), state, drop)


def retract(model, state, old_x, old_y, old_len=None):
    """(summary state, ctx images [T, n, ...] it holds, their labels [T, n, L], old_len) -> a NEW summary state without the first
    `old_len[t]` (0 .. n; default n) of them per task; the old state stays valid.  A summary keeps no per-shot rows,
    so the caller hands in the shots to take out; they are encoded like extend's new shots and subtracted
    (mlhot.ops.favor_retract).  The key stabiliser stays the state's: in exact arithmetic the result is
    `condition(form="summary")` on the remaining shots with the stabiliser of the larger set - merge's and select's caveat (6c-6):
    the result moves within the eps terms - and in fp32 it carries the rounding of a subtraction at the scale of the state before
    the retraction.  Shots that the state never absorbed give a finite but meaningless state.  Both families; eval mode.  Refused
    with ValueError before anything touches the GPU: everything extend refuses on a summary state, a state that is no summary, and
    `old_len[t] >= state.lens[t]` - a task keeps at least one shot."""
    return context.retract(_adapter(model), state, old_x, old_y, old_len)


def slide(model, state, new_x, new_y, new_len=None):
    """(per-shot or latent state, new ctx images [T, n, ...], labels, new_len) -> a NEW state holding the new shots like extend's,
    every task having given up its OLDEST slots first, only as many as `new_len[t]` needs beyond the spare capacity (DESIGN.md
    6c-12): a window over the last `capacity` shots of a stream in which only the new shots are ever encoded.  evict, then extend.
    `new_len[t]` above the capacity, a summary or empty state and whatever extend refuses raise ValueError."""
    return context.slide(_adapter(model), state, new_x, new_y, new_len)


def concat(model, states, form=None, capacity=None):
    """(1 .. 8 states of this model that keep per-shot rows, conditioned apart on the SAME T tasks) -> a NEW state whose task t holds
    the shots of states[0] task t, then states[1] task t, and so on: context shards, several sources for one task,
    stored per-object contexts - with everything only per-shot states offer (`return_attention=True`, `context_mask=`,
    `leave_one_out`, `evict`, `slide`).  All states are per-shot attention states - "keys", "long", "paged", mixed freely - or all are
    latent (CNP) states.  `lens` add up; the inputs stay valid.  No image is encoded and no row is recomputed: one plan upload, ONE
    launch (mlhot_rows_gather) copies the rows of both row sets into a new buffer, then evict's finishing step runs on them - the
    key launches of the result's form with the new lens, so the key stabiliser is the maximum over all shots of the result, which
    is what a fresh `condition` computes (attention), or the prefix aggregate with its gather and the finishing Linear (latent).
    `capacity` defaults to the largest total of a task (spare slots beyond it serve `extend`); `form` (attention only) defaults to
    the smallest form that holds the capacity - "keys" up to 32, "long" up to 256, "paged" up to 4096 - and an explicit one must hold
    it.  When every source and the result are "paged" the result is, bit for bit, `condition(form="paged", capacity=)` on the
    concatenated shots; for the other forms it agrees with a fresh condition to the kernels' tolerance (the per-shot Linears of the
    sources picked their kernel by row count).  More than 8 states: calls nest.  Both families; eval mode.  Refused with ValueError
    before anything touches the GPU: a foreign or stale state or one of another T, a summary state (merge / select combine those;
    `summarize` maps a per-shot state to one), an empty state, attention and latent states mixed, more than 8 states, a total above
    the capacity, a capacity above the form's, `form=` on latent states."""
    return context.concat(_adapter(model), states, form, capacity)


def regroup(model, states, picks, form=None, capacity=None):
    """`select`'s picks for states that keep per-shot rows: `states` as `concat` takes them, conditioned on ANY
    batches; `picks` has `tasks_per_batch` entries, entry t one (state_index, task_index) pair - task t of the result is that task -
    or a list of 1 .. 8 pairs whose shots stand behind one another in task t.  Any task of any state may stand in any slot, also in
    several; tasks and states that no pick names are left out.  The launches, `form`, `capacity` and the bit statements are
    concat's: `concat(model, states)` is `regroup(model, states, [[(0, t), (1, t), ..] for t in range(T)])`.  Also refused: an empty
    `picks[t]`, the same pair twice inside one task, a pair out of range, more than 8 parts in a task."""
    return context.regroup(_adapter(model), states, picks, form, capacity)


def summarize(model, state):
    """(per-shot attention state: "keys", "long" or "paged") -> a NEW form="summary" state of the same shots, the
    bridge to `merge` / `select`: the kept key and value rows go through mlhot.ops.favor_absorb as extend's new shots do on a
    summary, no image is encoded, the old state stays valid.  `merge`, `select`, `extend`, `retract` and `predict` serve the result
    like any summary state.  A latent, empty or summary state raises ValueError."""
    return context.summarize(_adapter(model), state)


def merge(model, states):
    """(summary states of this model, conditioned apart on the SAME T tasks) -> a NEW state holding all their context shots, as if
    `condition(..., form="summary")` had seen them together: shards of one context, several sources or streams per
    task, a stored library of per-object contexts.  FAVOR+'s summary is a sum over shots, so this is one launch per 8 states over
    the states alone (mlhot.ops.favor_merge) - no image is encoded again - and it equals the joint state in exact arithmetic, with
    one key stabiliser for the whole.  `lens` add up, `Nc` is their maximum; the inputs stay valid; `predict` and `extend` serve the
    result like any summary state.  Both families; eval mode.  A latent state (it is stored behind its finishing Linear), a
    form="keys" state (capped per-shot rows), a foreign or a stale state raise ValueError."""
    return context.merge(_CachedContext(model) if isinstance(model, ResNetNP) else _Vanilla(model), states)


def select(model, states, picks):
    """(summary states of this model, conditioned apart on ANY batches; picks) -> a NEW state for a batch put together from their
    tasks: a stored library of per-object contexts served as whatever batch is asked for.  `picks` has
    `tasks_per_batch` entries; entry t is one (state_index, task_index) pair - task t of the result is that task - or a list of
    1 .. 8 pairs whose context shots add up, as `merge` adds whole states.  Objects conditioned in batches (a0, a1) and (b0, b1) are
    queried as (a1, b0) with `select(model, [a, b], [(0, 1), (1, 0)])`; the same pair may stand in several tasks, tasks and states
    that no pick names are left out.  One launch per 8 named states over the states alone (mlhot.ops.favor_gather) - no image is
    encoded again.  The result is what `condition(..., form="summary")` builds from the chosen shots in a batch whose key stabiliser
    is the maximum over the named states - the reference's forward on the UNION of the source batches, restricted to the picked
    tasks; a batch of the picked tasks alone may have a lower stabiliser, which moves the result within the eps terms (6c-6).
    `predict` and `extend` serve the result like any summary state.  Both families; eval mode.  A foreign, stale, latent, "keys" or
    "long" state, an empty pick and the same pair twice inside one task raise ValueError."""
    return context.select(_CachedContext(model) if isinstance(model, ResNetNP) else _Vanilla(model), states, picks)


def predict(model, state, qry_x, chunk=None, route=None, return_attention=False, context_mask=None, attention_mass=False, target_weight=None,
            top_k=None, shared_targets=False):
    """(state, target images [T, Nq, ...]) -> mu [T, Nq, y_dim] = `model(ctx, labels, targets, test=True)[0]` for the context the
    state was made from, any Nq >= 1.  `chunk` bounds the targets per launch sequence (and the encoder's activations with them).
    `route`: None picks "fused" where mlhot_np_query_supported says yes and "composed" otherwise; a test may force either.  The
    state's `route` says which one ran.  "fused_summary"  is opt-in and never picked by None: on a form="summary"
    state of the vanilla attention models it runs everything behind the encoder as ONE launch (mlhot_np_query_summary_fwd) for any
    number of absorbed shots; another form, return_attention=True, dimensions outside that kernel's envelope and a task without a
    shot are ValueErrors before any launch.

    `return_attention=True` -> (mu, attn): attn [T, 8, Nq, Nc slots] is FAVOR+'s weight of every context slot per
    head and target (rows sum to 1; slots behind a task's ctx_len are exact zeros), concatenated over the chunks like mu.  The
    vanilla family runs the composed route for it - `route=None` picks it, a forced "fused" is a ValueError - and mu is bit-equal
    to `predict(..., route="composed")`; for a ResNetNP model mu is bit-equal to the call without the keyword.  A model without
    attention and a summary state refuse with ValueError; a form="long" state serves it for up to 256 slots, a
    form="paged" state for up to 4096 (6c-11).

    `context_mask`: a bool tensor [T, Nq, Nc slots] - target n of task t attends only to the slots that are True
    (and valid: behind no ctx_len) - -> mu [T, Nq, y_dim]; or [T, G, Nq, Nc slots], G masks of the same targets (leave-one-out,
    k-fold over the context, a causal stream) -> mu [T, G, Nq, y_dim] and, with return_attention=True, attn [T, G, 8, Nq, Nc] with
    exact zeros in the masked columns.  The targets go through the encoder ONCE and the query features are formed once per target;
    the G masked read-outs are one launch (mlhot_favor_query_masked_fwd / _long_masked_fwd), the Linears behind them run over the
    T * G * Nq rows through linear_rows.  The key stabiliser stays the state's (the maximum over all conditioned shots, the masked
    ones included), so against a forward on the sub-context the result moves within the eps terms when a mask drops the shot
    that holds it (6c-6).  An all-True mask gives the bits of `predict(..., route="composed")` (ResNetNP: of plain predict); a 4-D
    mask gives the bits of its G 3-D calls; chunked equals unchunked.  The vanilla family runs the composed route for it: a forced
    "fused" or "fused_summary" is a ValueError.  Also refused, before any launch: a summary, latent or empty state, keys kept on
    another route than "cached" / "long" / "paged", a mask of the wrong shape or dtype, and a mask that leaves a (task, group, target)
    without any of the task's valid shots - that check reads ONE reduced bool back from the mask's device.

    `attention_mass=True` -> (mu, mass): mass [T, 8, Nc slots] = attn summed over the targets, each weighed by
    `target_weight` [T, Nq] (finite and >= 0; None: 1) - how much this batch of targets attended to each stored shot, per head -
    reduced inside the query launch in a fixed order, so attn [T, 8, Nq, Nc] is never stored (the call holds 1/16 of it): the
    read-out that still fits at 4096 slots.  With target_weight None, mass is bit-equal to `fold32` of return_attention=True's attn
    (16-row tiles in ascending row order, then the tiles in order); slots behind a task's ctx_len are exact zeros; mu has the bits
    return_attention=True's mu has.  `chunk` must be a multiple of 16: the chunks' tile partials are folded once behind the last
    chunk, so every such chunk size gives the same bits as chunk=None.  Served and routed exactly where return_attention=True is;
    summary, latent and empty states refuse in its words; return_attention=True and context_mask= do not combine with it.
    `prune` chooses the slots to keep by this quantity.

    `top_k=k`, an integer in 1 .. 16 -> (mu, idx, w): idx int32 and w fp32 [T, 8, Nq, k], per head and target the k
    stored shots the prediction rests on most and the share of the attention each holds - the valid slots ranked by FAVOR+'s
    un-normalised score (descending, ties to the lower slot), w the very bits return_attention=True's attn has at [t, h, n, idx] -
    selected inside the query launch, the paged form in its one walk over the pages, so attn [T, 8, Nq, Nc] is never stored.
    Entries behind a task's ctx_len shots are idx = -1, w = 0.  The result is per target row: ANY `chunk` gives chunk=None's bits;
    mu has the bits return_attention=True's mu has.  Slot indices are the state's slot order: after `evict` / `prune` / `concat`
    they refer to the new state's.  Served and routed exactly where return_attention=True is; summary, latent and empty states and
    models without attention refuse in its words; return_attention=True, context_mask= and attention_mass=True do not combine with
    it; a forced "fused" / "fused_summary" route is a ValueError.

    `shared_targets=True`: `qry_x` is [Nq, ...] with NO task axis - one incoming frame or a set of probe images
    asked of all T stored contexts - -> mu [T, Nq, y_dim] (and attn [T, 8, Nq, Nc slots] with return_attention=True).  The targets go
    through the encoder (ResNetNP: the trunks) ONCE, as Nq images instead of T * Nq; the query-head Linear runs on Nq rows; the
    attention is ONE launch that forms the FAVOR+ query features once per 16 targets for all tasks
    (mlhot.ops.favor_query(shared=True)); only the Linears behind it see T * Nq rows, through linear_rows, whose sources
    broadcast.  Against `predict` on `qry_x.expand(T, ...)` the result agrees to the kernels' tolerance (the attention itself to
    the bit; the encoder's and the few-row Linears' bits may depend on the row count).  Served: per-shot states of form "keys" and
    "long", latent states (z[t] against the shared rows) and empty states; the vanilla family runs the composed route.  `chunk`
    bounds the targets per launch sequence; chunked equals unchunked to the bit.  Refused with ValueError before any launch:
    `context_mask=`, `attention_mass=True`, `target_weight=`, `top_k=`, a "summary" or "paged" state, a `qry_x` that carries a
    task axis, a forced "fused" / "fused_summary" route, and whatever plain predict refuses.  The default False is every call as
    it was."""
    if shared_targets:
        if isinstance(model, ResNetNP):
            if route is not None:
                raise ValueError("predict: route= belongs to the vanilla family")
            return model.predict(state, qry_x, chunk=chunk, return_attention=return_attention, context_mask=context_mask,
                                 attention_mass=attention_mass, target_weight=target_weight, top_k=top_k, shared_targets=True)
        return context.predict_shared(_Vanilla(model, route, return_attention), state, qry_x, chunk, return_attention, context_mask, attention_mass,
                                      target_weight, top_k)
    if isinstance(model, ResNetNP):
        if route is not None:
            raise ValueError("predict: route= belongs to the vanilla family")
        if top_k is not None:
            return model.predict(state, qry_x, chunk=chunk, return_attention=return_attention, context_mask=context_mask,
                                 attention_mass=attention_mass, target_weight=target_weight, top_k=top_k)
        if attention_mass or target_weight is not None:
            return model.predict(state, qry_x, chunk=chunk, return_attention=return_attention, context_mask=context_mask,
                                 attention_mass=attention_mass, target_weight=target_weight)
        if context_mask is not None:
            return model.predict(state, qry_x, chunk=chunk, return_attention=return_attention, context_mask=context_mask)
        if return_attention:
            return model.predict(state, qry_x, chunk=chunk, return_attention=True)
        return model.predict(state, qry_x, chunk=chunk)
    asks = "top_k=" if top_k is not None else "attention_mass=True" if attention_mass else return_attention
    return context.predict(_Vanilla(model, route, asks), state, qry_x, chunk, return_attention, context_mask, attention_mass, target_weight, top_k)


def prune(model, state, qry_x, keep, target_weight=None, chunk=None):
    """(per-shot attention state, target images [T, Nq, ...], keep) -> (a NEW state, drop): relevance-based forgetting for a bounded
    stream.  Per task the `keep[t]` valid slots (`keep`: an int or T ints, each >= 1) with the largest attention
    mass of these targets - `predict(attention_mass=True, target_weight=)` summed over the heads - stay, in their order; the others
    are let go through `evict`, with everything evict states: one row-compaction launch, no image encoded, the key stabiliser
    re-derived as the maximum over the shots that remain, the old state still valid.  Ties go to the lower slot index; a task with
    `lens[t] <= keep[t]` is untouched.  `drop`, T ascending lists of slot indices, is what evict was given - log it.  The choice
    costs ONE device-to-host copy of [T, Nc] floats.  `chunk` as predict(attention_mass=True) takes it (a multiple of 16).  Refused
    with ValueError: `keep[t] < 1`, and whatever predict(attention_mass=True) and evict refuse."""
    ad = _CachedContext(model) if isinstance(model, ResNetNP) else _Vanilla(model, None, "attention_mass=True")
    return context.prune(ad, state, qry_x, keep, target_weight, chunk)


def leave_one_out(model, state, qry_x, chunk=None):
    """(state, target images [T, Nq, ...]) -> mu [T, Nc slots, Nq, y_dim]: group c is the prediction WITHOUT context slot c - the
    influence of every shot on the prediction itself, not only on the attention weight; with the context's own images as targets,
    outlier detection among the context labels.  It is `predict(context_mask=)` with the G = Nc masks
    ~eye(Nc) built on the device: one encoder pass over the targets, one masked query launch per chunk.  Groups c >= lens[t] drop
    a slot that holds no shot and equal the unmasked prediction.  A task with a single shot is refused (nothing would be left),
    and so is everything predict(context_mask=) refuses."""
    Nc, lens = getattr(state, "Nc", 0), getattr(state, "lens", ())
    if getattr(state, "kind", None) == "attention" and lens and min(lens) < 2:
        raise ValueError(f"leave_one_out: a task of the state holds a single context shot (shots per task: {list(lens)}): without it "
                         "nothing is left to attend to")
    mask = ~torch.eye(max(Nc, 1), dtype=torch.bool, device=qry_x.device)[None, :, None, :].expand(qry_x.shape[0], -1, qry_x.shape[1], -1)
    return predict(model, state, qry_x, chunk=chunk, context_mask=mask)


def _rows(sources, lin_w, lin_b, act):
    """linear_rows, or - for a layer it does not serve (logged once) - LinearFunction on the gathered rows."""
    k0, k1 = sources[0][0].shape[1], sources[1][0].shape[1] if len(sources) > 1 else 0
    if lib().linear_rows_supported(k0, k1, lin_w.shape[0]):
        return linear_rows(sources, lin_w, lin_b, act)
    if (k0, k1, lin_w.shape[0]) not in _logged:
        _logged.add((k0, k1, lin_w.shape[0]))
        logging.getLogger(__name__).info("mlhot.cached.predict: no row-invariant kernel for a Linear [%d | %d] -> %d", k0, k1, lin_w.shape[0])
    rows = next(x.shape[0] * rep for x, rep, period in sources if period == 0)

    def gathered(x, rep, period):                # a source that wraps before the last row (shared targets) is gathered by index
        if period and period < rows:
            idx = torch.arange(rows, device=x.device)
            return x[(idx // rep) % period]
        return x.repeat_interleave(rep, dim=0) if rep > 1 else x
    x = torch.cat([gathered(*s) for s in sources], dim=1)
    return LinearFunction.apply(x, lin_w, lin_b, act)


def composed_tail(params, x_qry, T, Nq, tanh, keys=None, vh=None, proj=None, z=None, wq=None, favor=None, prefixes=None, weights=False,
                  target_weight=None, shared=False):
    """The query tail from the existing row-invariant operators - the yardstick of the fused launch and the route for dimensions
    it does not serve.  params: state_dict key -> tensor; x_qry [T * Nq, dim_w]; attention: keys (FavorKeyState), vh, proj (wq: the
    stacked _W_q weight and bias, else stacked here); otherwise z [T, dim_z].  -> mu [T, Nq, y_dim].

    `favor` (attention): the FAVOR+ stage, query heads [T, Nq, 8, dim_w] -> merged; default favor_query on `keys`.  With `prefixes`
    = K it answers for K context prefixes at once (favor_prefixes_long) and every Linear behind it runs once over the K * T * Nq
    rows, x_qry wrapping every T * Nq - row-invariant, so a row has the single tail's bits.  -> mu [K, T, Nq, y_dim].

    `weights` (with `keys`, the default FAVOR+ stage): -> (mu, w), w [T, 8, Nq, Nc] from favor_query(weights=True); mu's bits stay.
    `weights="mass"`: -> (mu, part), the tile partials [T, 8, ceil(Nq / 16), Nc] of favor_query(mass="tiles",
    target_weight=); mu's bits stay.  `weights=("topk", k)`: -> (mu, [idx, wk]) of favor_query(topk=k); mu's bits stay.

    `shared=True`: x_qry is [Nq, dim_w], the encoder's rows of Nq targets shared by the T tasks.  The query-head
    Linear runs on those Nq rows, the attention is favor_query(shared=True), and the Linears behind it run over the T * Nq rows
    with x_qry wrapping every Nq.  With `keys` (weights False or True) or `z`; -> mu [T, Nq, y_dim] (and w [T, 8, Nq, Nc])."""
    def lin(sources, name, act="none"):
        return _rows(sources, params[name + ".weight"], params[name + ".bias"], act)
    if shared:
        att = None
        if keys is not None:
            w, b = wq if wq is not None else (torch.cat([params[f"_W_q.{i}.linear.weight"] for i in range(HEADS)]),
                                              torch.cat([params[f"_W_q.{i}.linear.bias"] for i in range(HEADS)]))
            qh = _rows([(x_qry, 1, 0)], w, b, "none").view(Nq, HEADS, -1)
            merged = favor_query(qh, keys, vh, proj, weights=bool(weights), shared=True)
            if weights:
                merged, att = merged
            zq = lin([(lin([(merged.view(T * Nq, -1), 1, 0)], "_W.linear"), 1, 0)], "r_to_z")
            h = lin([(x_qry, 1, Nq), (zq, 1, 0)], "decoder0.0", "relu")
        else:
            h = lin([(x_qry, 1, Nq), (z, Nq, 0)], "decoder0.0", "relu")
        h = lin([(h, 1, 0)], "decoder0.2", "relu")
        mu = lin([(h, 1, 0)], "decoder0.4", "tanh" if tanh else "none").view(T, Nq, -1)
        return (mu, att) if weights else mu
    K = 1 if prefixes is None else prefixes
    if keys is not None or favor is not None:
        w, b = wq if wq is not None else (torch.cat([params[f"_W_q.{i}.linear.weight"] for i in range(HEADS)]),
                                          torch.cat([params[f"_W_q.{i}.linear.bias"] for i in range(HEADS)]))
        qh = _rows([(x_qry, 1, 0)], w, b, "none").view(T, Nq, HEADS, -1)
        att = None
        if weights:
            if isinstance(weights, tuple):
                merged, *att = favor_query(qh, keys, vh, proj, topk=weights[1])
            else:
                merged, att = (favor_query(qh, keys, vh, proj, mass="tiles", target_weight=target_weight) if weights == "mass"
                               else favor_query(qh, keys, vh, proj, weights=True))
            merged = merged.view(K * T * Nq, -1)
        else:
            merged = (favor_query(qh, keys, vh, proj) if favor is None else favor(qh)).view(K * T * Nq, -1)
        zq = lin([(lin([(merged, 1, 0)], "_W.linear"), 1, 0)], "r_to_z")
        h = lin([(x_qry, 1, T * Nq), (zq, 1, 0)], "decoder0.0", "relu")
    else:
        h = lin([(x_qry, 1, T * Nq), (z, Nq, 0)], "decoder0.0", "relu")
    h = lin([(h, 1, 0)], "decoder0.2", "relu")
    mu = lin([(h, 1, 0)], "decoder0.4", "tanh" if tanh else "none")
    mu = mu.view(T, Nq, -1) if prefixes is None else mu.view(K, T, Nq, -1)
    return (mu, att) if weights else mu


# ---- prefix sweep for the vanilla family ---------------------------------------------------------------------------
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
    _refuse(model, "sweep", _SWEEP)
    T, Nc, Nq = ctx_x.shape[0], ctx_x.shape[1], qry_x.shape[1]
    if T != model.task_num or qry_x.shape[0] != T or ctx_y.shape[0] != T:
        raise ValueError(f"sweep: {T} context and {qry_x.shape[0]} target tasks, the model was built for tasks_per_batch = {model.task_num}")
    if Nc < 1 or Nq < 1 or ctx_y.shape[1] != Nc:
        raise ValueError(f"sweep needs at least one context shot with its label and one target (got {Nc} shots, {ctx_y.shape[1]} labels, {Nq} targets)")
    ks = _sweep_ks(ks, Nc)
    if route is not None and route not in SWEEP_ROUTES:
        raise ValueError(f"sweep: route must be one of {SWEEP_ROUTES}, got {route!r}")
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
        a_rows, b_rows = _encoded_rows(model, x_ctx, ctx_y.reshape(T * Nc, -1))           # condition's per-shot stage
        proj = _c(model.attn.projection_matrix) if model.ATTENTION else None
        params = {k: _c(p.detach()) for k, p in model.named_parameters()}
        if model.ATTENTION:
            kh, vh = _c(a_rows.view(T, Nc, HEADS, -1)), _c(b_rows.view(T, Nc, HEADS, -1))
            sweep.last_attention = "prefix_long" if long_ctx else "np_prefix" if route == "fused" else "favor_keys"
            if route == "fused":
                return lib().np_prefix_fwd(dims, params, x_qry.view(T, Nq, -1), ks, kh=kh, vh=vh, proj=proj)
            wq = _stacked(model._W_q)
            if long_ctx:
                return composed_tail(params, x_qry, T, Nq, model.OUT_TANH, wq=wq, prefixes=K,
                                     favor=lambda qh: favor_prefixes_long(qh, kh, vh, proj, ks))
            return torch.stack([composed_tail(params, x_qry, T, Nq, model.OUT_TANH, keys=favor_keys(kh, proj, lens=(k,) * T, lens_dev=up[i]), vh=vh,
                                              proj=proj, wq=wq) for i, k in enumerate(ks)])
        r = agg_prefixes(model.agg_mode, a_rows.view(T, Nc, -1), None if b_rows is None else b_rows.view(T, Nc, -1))      # [Nc, T, R]
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
