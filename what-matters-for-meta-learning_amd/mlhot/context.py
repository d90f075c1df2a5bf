"""Cached-context inference, the part both model families share: the state `condition` leaves for `predict`, and
the lifecycle condition -> extend / merge / select -> predict with its entry checks, written once.  ResNetNP.condition / extend / predict
(networks/_resnet_np.py) and mlhot.cached.condition / extend / predict (the vanilla family) are thin callers of the functions here.

What differs per family comes in as an adapter `ad`, a small object with
    model                               the owner: task_num, ATTENTION, agg_mode, img_channels, img_size, attn.projection_matrix
    refuse(what)                        raises, in the family's own words, for a model or a mode the path does not serve
    prepare(*tensors)                   host work before the first launch (the gradient arena / the device check)
    begin(launches)                     inside no_grad, before condition's launches -> what the state carries as `wq`
    shot_rows(imgs [P, C, H, W], labels [P, L])     the per-shot stage -> (kh, vh) [P, H, d] or (rs, lv) [P, R], lv None but for baco;
                                        invariant=True (form "paged", attention): its Linears through mlhot.ops.linear_rows_any
    finish                              the Linear behind the aggregate (`mu` / `r_to_z`)
    empty_z(device)                     `z` of the state without a context shot
    route(state, qry_x)                 predict's own checks and choices, behind the shared ones
    predict_targets(state, qry_x)       one launch sequence for the targets of one chunk -> mu [T, n, y_dim]; called with
                                        attention=True for predict(return_attention=True) -> (mu, attn [T, H, n, Nc])
    route_shared(state, imgs)           route's part for predict(shared_targets=True)
    predict_shared(state, imgs [n, C, H, W])        predict_targets for n targets WITHOUT a task axis, asked of all T tasks
This module imports nothing from networks/: both families import it."""
import numbers

import torch

from mlhot import lib, ragged
from mlhot.ops import GATHER_PARTS, PER_SHOT_ROUTES, LinearFunction, _c, favor_gather, favor_keys, favor_merge, target_weight_arg, topk_arg


class ContextState:
    """What condition leaves for predict.  `kind`: "attention" - `keys` (mlhot.ops.FavorKeyState) and the value heads `vh`
    [T, Nc, H, d]; "latent" - the task embedding `z` [T, dim_z], the aggregated context through the finishing Linear; "empty" - no
    context shot (`z` zeros or None).  `owner` is the model, `fingerprint` its parameters' and buffers' versions when the state
    was made: extend and predict refuse a state whose model has moved on.  `wq`: the stacked query-head weight and bias where the
    family keeps them with the state (vanilla), `route` the route the last vanilla predict on this state took ("fused" |
    "composed"; None before the first).

    For extend the state also keeps `lens` (context shots per task, host ints), `capacity` (slots per task: `Nc`
    is the capacity, what the kernels see) and the per-shot rows in slot order [T, capacity, ...]: `kh` and the zero-filled `vh`
    (attention), `rs` - baco: the mean Linear's output - and `lv` (latent), with `r`, the aggregate before the finishing Linear.

    `form` "summary" (DESIGN.md 6c-4): `keys` is a fixed-size summary state (mlhot.ops.favor_absorb), `Nc` the largest of `lens`;
    there is no capacity and there are no per-shot rows - `vh`, `kh` are None.

    `form` "long" (DESIGN.md 6c-7): everything of "keys" - `lens`, `capacity`, `kh` and `vh` in slot order - with up to 256 slots;
    `keys` is mlhot.ops.favor_keys_long's state.

    `form` "paged" (DESIGN.md 6c-11): the same with up to 4096 slots; `keys` is mlhot.ops.favor_keys_paged's state."""

    def __init__(self, owner, T, Nc, fingerprint, kind, keys=None, vh=None, z=None, lens=None, kh=None, rs=None, lv=None, r=None,
                 form="keys", wq=None):
        self.owner, self.T, self.Nc, self.fingerprint, self.kind = owner, T, Nc, fingerprint, kind
        self.keys, self.vh, self.z, self.wq, self.route = keys, vh, z, wq, None
        self.lens, self.capacity, self.form = (Nc,) * T if lens is None else tuple(lens), None if form == "summary" else Nc, form
        self.kh, self.rs, self.lv, self.r = kh, rs, lv, r


def fingerprint(model):
    return tuple(p._version for p in model.parameters()) + tuple(b._version for b in model.buffers())


def _images(model, images):
    """[T, n, ...] -> [T, n, C, H, W]"""
    return images.reshape(images.shape[0], images.shape[1], model.img_channels, model.img_size[0], model.img_size[1])


def _enter(ad, what, state, rows, noun):
    """The checks extend and predict share; `rows` [T, n, ...] are the new shots / the targets."""
    ad.refuse(what)
    if not isinstance(state, ContextState) or state.owner is not ad.model:
        raise ValueError(f"{what}: the state was not made by this model's condition()")
    if rows.shape[0] != state.T or state.T != ad.model.task_num:
        raise ValueError(f"{what}: the state holds {state.T} tasks, the {noun} {rows.shape[0]} (the key stabiliser is the maximum over the "
                         f"conditioned batch: {what} serves the same tasks)")
    if state.fingerprint != fingerprint(ad.model):
        raise ValueError(f"{what}: the state is stale - a parameter of the model changed since condition()")


def condition(ad, ctx_x, ctx_y, ctx_len=None, capacity=None, form="keys"):
    """(ctx images [T, Nc, ...], ctx labels [T, Nc, L]) -> ContextState: the per-shot stage, then the FAVOR+ key features
    (attention) or the aggregation and the finishing Linear.  `ctx_len` / `capacity`: the masked path (_grow); `form="summary"`:
    _absorb; `form="long"` / `"paged"`: always _grow, with mlhot.ops.favor_keys_long / favor_keys_paged behind it; neither: the call
    as it always was."""
    model = ad.model
    ragged.check_form("condition", form)
    ad.refuse("condition")
    T, Nc = ctx_x.shape[0], ctx_x.shape[1]
    if T != model.task_num:
        raise ValueError(f"condition: {T} tasks, the model was built for tasks_per_batch = {model.task_num}")
    if form == "summary":
        lens = ragged.summary_condition_args("condition", T, Nc, ctx_len, capacity, model.ATTENTION)
    elif form in ragged.PER_SHOT_CAPACITY:
        lens, capacity = ragged.long_condition_args("condition", T, Nc, ctx_len, capacity, model.ATTENTION, form)
    else:
        lens, capacity = ragged.condition_args("condition", T, Nc, ctx_len, capacity, model.ATTENTION)
    ad.prepare(ctx_x, ctx_y)
    with torch.no_grad():
        if form == "summary":
            return _absorb(ad, None, ctx_x, ctx_y, lens, ad.begin(True))
        wq = ad.begin(lens is not None or Nc > 0)
        if lens is not None:
            return _grow(ad, None, (0,) * T, capacity, ctx_x, ctx_y, lens, wq, form)
        if Nc == 0:
            return ContextState(model, T, 0, fingerprint(model), "empty", z=ad.empty_z(ctx_x.device), wq=wq)
        a_rows, b_rows = ad.shot_rows(ctx_x.reshape(T * Nc, model.img_channels, model.img_size[0], model.img_size[1]), ctx_y.reshape(T * Nc, -1))
        a_rows = a_rows.view(T, Nc, *a_rows.shape[1:])
        b_rows = b_rows.view(T, Nc, *b_rows.shape[1:]) if b_rows is not None else None
        if model.ATTENTION:
            keys = favor_keys(a_rows, model.attn.projection_matrix)
            return ContextState(model, T, Nc, fingerprint(model), "attention", keys=keys, vh=b_rows.contiguous(), wq=wq, kh=a_rows.contiguous())
        return _latent(ad, Nc, a_rows, b_rows, lib().agg_fwd(model.agg_mode, a_rows, b_rows)[0])


def extend(ad, state, new_x, new_y, new_len=None):
    """(state, new ctx images [T, n, ...], their labels [T, n, L], new_len) -> a NEW state whose task t holds new_len[t] more context
    shots (0 .. n each; default n), written behind its current ones; the old state stays valid.  Only the new shots go through the
    per-shot stage."""
    _enter(ad, "extend", state, new_x, "new shots")
    T, n = new_x.shape[0], new_x.shape[1]
    if state.form == "summary":
        add = ragged.summary_extend_args("extend", T, n, new_len)
    else:
        add = ragged.extend_args("extend", state, T, n, new_len)
    ad.prepare(new_x, new_y)
    with torch.no_grad():
        if state.form == "summary":
            return _absorb(ad, state, new_x, new_y, add, state.wq)
        return _grow(ad, state, state.lens, state.capacity, new_x, new_y, add, state.wq, state.form)


def _own(ad, what, state):
    """_enter's checks for a call that brings no rows of its own (evict)."""
    ad.refuse(what)
    if not isinstance(state, ContextState) or state.owner is not ad.model:
        raise ValueError(f"{what}: the state was not made by this model's condition()")
    if state.T != ad.model.task_num:
        raise ValueError(f"{what}: the state holds {state.T} tasks, the model was built for tasks_per_batch = {ad.model.task_num}")
    if state.fingerprint != fingerprint(ad.model):
        raise ValueError(f"{what}: the state is stale - a parameter of the model changed since condition()")


def _refuse_rowless(what, state, instead):
    """evict's and slide's: a state without per-shot rows has no slot to free."""
    if state.kind == "empty":
        raise ValueError(f"{what}: the state holds no context shot")
    if state.form == "summary":
        raise ValueError(f"{what}: a summary state keeps no per-shot rows, so there is no slot to free; {instead}")


def _compact(state, plan):
    """The per-shot rows of `state` moved by plan.rows: ONE mlhot_rows_compact launch for both row sets -> (kh, vh) / (rs, lv)."""
    a_rows, b_rows = (state.kh, state.vh) if state.kind == "attention" else (state.rs, state.lv)
    if a_rows is None:
        raise ValueError("evict: the state carries no per-shot rows (it was not made by condition())")
    out = lib().rows_compact([_c(x) for x in (a_rows, b_rows) if x is not None], plan.rows)
    return out[0], out[1] if b_rows is not None else None


def evict(ad, state, drop):
    """(state, drop) -> a NEW state without the context shots in the slots drop[t] of task t: the kept shots move to
    the front in their order, the freed slots behind them are zero rows as condition(ctx_len=, capacity=) leaves spare slots;
    capacity, form and kind stay, the old state stays valid.  No image is encoded: one mlhot_rows_compact launch moves the kept rows,
    then the finishing step of extend runs on them - the key launches of the state's form with the new lens, so the key stabiliser
    is the maximum over the shots that remain, exactly condition's on them (attention), or the prefix aggregate with its gather
    and the finishing Linear (latent)."""
    what = "evict"
    _own(ad, what, state)
    _refuse_rowless(what, state, "mlhot.cached.retract takes shots out of a summary")
    drop = ragged.evict_args(what, state, drop)
    ad.prepare()
    model = ad.model
    with torch.no_grad():
        plan = ragged.KeepPlan(state.lens, drop, state.capacity, (state.kh if state.kind == "attention" else state.rs).device)
        a_rows, b_rows = _compact(state, plan)
        if state.kind == "attention":
            keys = ragged.masked_keys(a_rows, model.attn.projection_matrix, plan, state.form)
            return ContextState(model, state.T, state.capacity, fingerprint(model), "attention", keys=keys, vh=b_rows, wq=state.wq, lens=plan.total,
                                kh=a_rows, form=state.form)
        return _latent(ad, state.capacity, a_rows, b_rows, ragged.gathered_aggregate(model.agg_mode, a_rows, b_rows, plan), plan.total)


def retract(ad, state, old_x, old_y, old_len=None):
    """(summary state, ctx images [T, n, ...] that were conditioned or extended into it, their labels [T, n, L], old_len) -> a NEW
    summary state without the first old_len[t] (0 .. n; default n) of them per task; the old state stays valid.  A
    summary keeps no per-shot rows, so the shots to take out are handed in again: they go through the per-shot stage like extend's
    new shots and are subtracted (mlhot.ops.favor_retract).  The key stabiliser stays the state's."""
    what = "retract"
    _enter(ad, what, state, old_x, "old shots")
    if state.form != "summary":
        raise ValueError(f"{what}: the state is no summary ({state.kind!r}, form {state.form!r}) - a state with per-shot rows lets shots go by "
                         "their slots: mlhot.cached.evict")
    T, n = old_x.shape[0], old_x.shape[1]
    sub = ragged.retract_args(what, state, T, n, old_len)
    ad.prepare(old_x, old_y)
    model = ad.model
    with torch.no_grad():
        plan = ragged.Plan((0,) * T, sub, n, n, old_x.device)
        keys = state.keys
        if plan.n:
            old_k, old_v = ad.shot_rows(ragged.pack(_images(model, old_x), plan.src), ragged.pack(old_y.reshape(T, n, -1), plan.src))
            keys = ragged.summary_retract(keys, old_k, old_v, plan, T, n, model.attn.projection_matrix, sub)
        return ContextState(model, T, max(keys.lens), fingerprint(model), "attention", keys=keys, wq=state.wq, lens=keys.lens, form="summary")


def slide(ad, state, new_x, new_y, new_len=None):
    """(per-shot or latent state, new ctx images [T, n, ...], labels, new_len) -> a NEW state that holds the new shots like extend's,
    every task having given up its OLDEST slots first - only as many as new_len[t] needs beyond the spare capacity:
    the window of the last `capacity` shots of a stream.  evict, then extend; of evict only the row compaction runs, its finishing
    step would be overwritten by extend's on the same rows."""
    what = "slide"
    _enter(ad, what, state, new_x, "new shots")
    _refuse_rowless(what, state, "a summary follows a stream with mlhot.cached.retract and extend")
    T, n = new_x.shape[0], new_x.shape[1]
    add, drop = ragged.slide_args(what, state, T, n, new_len)
    ad.prepare(new_x, new_y)
    with torch.no_grad():
        kept = state
        if any(drop):
            plan = ragged.KeepPlan(state.lens, drop, state.capacity, new_x.device)
            a_rows, b_rows = _compact(state, plan)
            rows = dict(kh=a_rows, vh=b_rows) if state.kind == "attention" else dict(rs=a_rows, lv=b_rows)
            kept = ContextState(state.owner, T, state.capacity, state.fingerprint, state.kind, lens=plan.total, form=state.form, **rows)
        return _grow(ad, kept, kept.lens, state.capacity, new_x, new_y, add, state.wq, state.form)


def _summary_states(ad, what, states, same_tasks=True):
    """merge's and select's checks of their states: a non-empty sequence of this model's own, fresh attention states of
    form="summary" -> the list."""
    try:
        states = list(states)
    except TypeError:
        raise ValueError(f"{what}: states must be a sequence of states of condition(form=\"summary\"), got {type(states).__name__}") from None
    if not states:
        raise ValueError(f"{what}: needs at least one state (got an empty sequence)")
    for i, s in enumerate(states):
        if not isinstance(s, ContextState) or s.owner is not ad.model:
            raise ValueError(f"{what}: the state was not made by this model's condition() (states[{i}])")
        if s.kind != "attention":
            raise ValueError(f"{what}: states[{i}] is a {s.kind!r} state - it is stored behind its finishing Linear, which is not a sum over "
                             f"shots any more; only attention states of form=\"summary\" {what}")
        if s.form != "summary":
            slots = ragged.PER_SHOT_CAPACITY.get(s.form, ragged.MAX_ATTENTION_CAPACITY)
            raise ValueError(f"{what}: states[{i}] has form {s.form!r} - it holds per-shot rows in at most {slots} "
                             "slots, not sums over shots; condition the parts with form=\"summary\"")
        if same_tasks and (s.T != states[0].T or s.T != ad.model.task_num):
            raise ValueError(f"{what}: states[{i}] holds {s.T} tasks, states[0] {states[0].T}, the model {ad.model.task_num} (the key stabiliser "
                             f"is the maximum over the conditioned batch: {what} serves the same tasks)")
        if s.fingerprint != fingerprint(ad.model):
            raise ValueError(f"{what}: the state is stale - a parameter of the model changed since condition() (states[{i}])")
    return states


def merge(ad, states):
    """Summary states of ONE model that were conditioned apart - shards of a context, several sources, stored per-object contexts -
    -> a NEW state holding all their shots, as if condition(form="summary") had seen them together (DESIGN.md 6c-6:
    mlhot.ops.favor_merge, one launch per 8 states, no image is encoded again).  The inputs stay valid.  `lens` add up, `Nc` is their
    maximum; predict and extend serve the result like any summary state."""
    what = "merge"
    ad.refuse(what)
    states = _summary_states(ad, what, states)
    with torch.no_grad():
        keys = favor_merge([s.keys for s in states])
    return ContextState(ad.model, states[0].T, max(keys.lens), states[0].fingerprint, "attention", keys=keys, wq=states[0].wq, lens=keys.lens,
                        form="summary")


def select(ad, states, picks):
    """Pick and combine TASKS across summary states of ONE model (mlhot.ops.favor_gather, no image is encoded
    again): `picks` has one entry per task of the model's batch, a (state_index, task_index) pair or a list of 1 .. 8 such pairs
    whose shots add up -> a NEW summary state whose task t holds them.  Any task of any state can stand in any slot, also in
    several; tasks that no pick names are left out, and so are states that no pick names (they do not enter the stabiliser).  The
    inputs stay valid; predict and extend serve the result like any summary state.  It is the state condition(form="summary")
    builds from the chosen shots in a batch whose stabiliser is the maximum over the named states."""
    what = "select"
    ad.refuse(what)
    states = _summary_states(ad, what, states, same_tasks=False)
    try:
        picks = list(picks)
    except TypeError:
        raise ValueError(f"{what}: picks must be a sequence with one entry per task, got {type(picks).__name__}") from None
    if len(picks) != ad.model.task_num:
        raise ValueError(f"{what}: {len(picks)} picks, the model was built for tasks_per_batch = {ad.model.task_num}")
    table = []
    for t, pick in enumerate(picks):
        if isinstance(pick, (tuple, list)) and len(pick) == 2 and all(isinstance(x, numbers.Integral) for x in pick):
            pick = [pick]                               # one pair
        try:
            pick = [tuple(pair) for pair in pick]
        except TypeError:
            raise ValueError(f"{what}: picks[{t}] must be a (state_index, task_index) pair or a list of such pairs, got {pick!r}") from None
        if not pick:
            raise ValueError(f"{what}: picks[{t}] is empty - a task without a context shot has no attention (0 / 0)")
        if len(pick) > GATHER_PARTS:
            raise ValueError(f"{what}: picks[{t}] names {len(pick)} parts; a task takes at most {GATHER_PARTS}")
        if len(set(pick)) != len(pick):
            twice = next(pair for k, pair in enumerate(pick) if pair in pick[:k])
            raise ValueError(f"{what}: picks[{t}] names {twice} twice - its shots would count double inside one task (the same pair may "
                             "stand in different tasks)")
        table.append(pick)
    with torch.no_grad():
        keys = favor_gather([s.keys for s in states], table)          # ValueError for a pair that is no pair or out of range
    return ContextState(ad.model, len(table), max(keys.lens), states[0].fingerprint, "attention", keys=keys, wq=states[0].wq, lens=keys.lens,
                        form="summary")


def _row_states(ad, what, states, same_tasks):
    """concat's and regroup's checks of their states: 1 .. 8 of this model's own, fresh states that keep per-shot
    rows, all attention ("keys", "long", "paged", mixed freely) or all latent -> (the list, the model's fingerprint)."""
    try:
        states = list(states)
    except TypeError:
        raise ValueError(f"{what}: states must be a sequence of per-shot or latent states of condition(), got {type(states).__name__}") from None
    if not states:
        raise ValueError(f"{what}: needs at least one state (got an empty sequence)")
    if len(states) > ragged.JOIN_PARTS:
        raise ValueError(f"{what}: {len(states)} states; a call takes at most {ragged.JOIN_PARTS} - calls nest: {what} the states in groups, "
                         "then the results")
    fresh = fingerprint(ad.model)                      # once: it walks every parameter and buffer
    for i, s in enumerate(states):
        if not isinstance(s, ContextState) or s.owner is not ad.model:
            raise ValueError(f"{what}: the state was not made by this model's condition() (states[{i}])")
        if s.kind == "empty":
            raise ValueError(f"{what}: states[{i}] holds no context shot - there is no row to take from it")
        if s.form == "summary":
            raise ValueError(f"{what}: states[{i}] is a summary state - it keeps sums over shots, no per-shot rows; mlhot.cached.merge and "
                             "mlhot.cached.select combine summary states, and mlhot.cached.summarize maps a per-shot state to a summary "
                             "to mix the two")
        if s.kind != states[0].kind:
            raise ValueError(f"{what}: states[{i}] is a {s.kind!r} state, states[0] a {states[0].kind!r} one - attention and latent states "
                             "do not mix")
        if same_tasks and (s.T != states[0].T or s.T != ad.model.task_num):
            raise ValueError(f"{what}: states[{i}] holds {s.T} tasks, states[0] {states[0].T}, the model {ad.model.task_num} (task t of the "
                             f"result is task t of every state: {what} serves the same tasks)")
        if s.fingerprint != fresh:
            raise ValueError(f"{what}: the state is stale - a parameter of the model changed since condition() (states[{i}])")
        if (s.kh if s.kind == "attention" else s.rs) is None or s.capacity is None:
            raise ValueError(f"{what}: states[{i}] carries no per-shot rows (it was not made by condition())")
        for x in ((s.kh, s.vh) if s.kind == "attention" else (s.rs, s.lv)):
            if x is not None and x[0, 0].numel() % 4:
                raise ValueError(f"{what}: states[{i}] keeps per-shot rows of {x[0, 0].numel()} floats; mlhot_rows_gather moves rows whose "
                                 "width is a multiple of 4 floats")
    return states, fresh


def _join(ad, what, states, parts, total, form, capacity, fresh):
    """regroup's and concat's launches: one plan upload, ONE mlhot_rows_gather launch for both row sets, then evict's finishing step
    on the gathered rows."""
    model, kind = ad.model, states[0].kind
    ad.prepare()
    with torch.no_grad():
        sources = [[_c(x) for x in ((s.kh, s.vh) if kind == "attention" else (s.rs, s.lv)) if x is not None] for s in states]
        plan = ragged.GatherPlan(parts, [s.lens for s in states], [s.capacity for s in states], capacity, sources[0][0].device)
        out = lib().rows_gather(sources, plan.rows, len(parts), capacity)
        a_rows, b_rows = out[0], out[1] if len(out) > 1 else None
        if kind == "attention":
            keys = ragged.masked_keys(a_rows, model.attn.projection_matrix, plan, form)
            return ContextState(model, len(parts), capacity, fresh, "attention", keys=keys, vh=b_rows, wq=states[0].wq, lens=plan.total,
                                kh=a_rows, form=form)
        return _latent(ad, capacity, a_rows, b_rows, ragged.gathered_aggregate(model.agg_mode, a_rows, b_rows, plan), plan.total)


def regroup(ad, states, picks, form=None, capacity=None):
    """select's picks for states that keep per-shot rows: `states` 1 .. 8 per-shot attention states ("keys", "long",
    "paged", mixed freely) or latent states of ONE model; `picks` has one entry per task of the model's batch, a (state_index,
    task_index) pair or a list of 1 .. 8 such pairs whose shots stand behind one another in task t -> a NEW state.  Any task of any
    state may stand in any slot, also in several; the inputs stay valid and no image is encoded: one plan upload, ONE
    mlhot_rows_gather launch for both row sets, then evict's finishing step - the key launches of the result's form with the new
    lens, so the key stabiliser is the maximum over the shots of the result, exactly condition's on them (attention), or the
    prefix aggregate with its gather and the finishing Linear (latent).  `capacity` defaults to the largest total, `form`
    (attention only) to the smallest form that holds the capacity; `wq` is states[0]'s."""
    what = "regroup"
    ad.refuse(what)
    states, fresh = _row_states(ad, what, states, same_tasks=False)
    attention = states[0].kind == "attention"
    parts, total, form, capacity = ragged.regroup_args(what, [(s.lens, s.capacity) for s in states], picks, ad.model.task_num, attention, form, capacity)
    return _join(ad, what, states, parts, total, form, capacity, fresh)


def concat(ad, states, form=None, capacity=None):
    """Per-shot attention states or latent states of ONE model that were conditioned apart on the SAME T tasks -> a NEW state whose
    task t holds the shots of states[0] task t, then states[1] task t, and so on: regroup with picks[t] =
    [(0, t), (1, t), ..].  `lens` add up; the inputs stay valid."""
    what = "concat"
    ad.refuse(what)
    states, fresh = _row_states(ad, what, states, same_tasks=True)
    attention = states[0].kind == "attention"
    parts, total, form, capacity = ragged.join_args(what, [(s.lens, s.capacity) for s in states], ad.model.task_num, attention, form, capacity)
    return _join(ad, what, states, parts, total, form, capacity, fresh)


def summarize(ad, state):
    """A per-shot attention state ("keys", "long", "paged") -> a NEW form="summary" state of the same shots: the
    kept kh / vh rows, packed, go through ragged.summary_absorb as _absorb's new shots do (mlhot.ops.favor_absorb, chunks of 32); no
    image is encoded and the old state stays valid.  merge, select, extend, retract and predict serve the result like any summary."""
    what = "summarize"
    _own(ad, what, state)
    if state.kind == "empty":
        raise ValueError(f"{what}: the state holds no context shot")
    if state.kind != "attention":
        raise ValueError(f"{what}: the state is a {state.kind!r} state - it is one aggregate per task behind its finishing Linear; only "
                         'attention states have a form="summary"')
    if state.form == "summary":
        raise ValueError(f"{what}: the state is a summary already")
    if state.kh is None or state.vh is None:
        raise ValueError(f"{what}: the state carries no per-shot rows (it was not made by condition())")
    ad.prepare()
    model, T, cap = ad.model, state.T, state.capacity
    with torch.no_grad():
        plan = ragged.Plan((0,) * T, state.lens, cap, cap, state.kh.device)
        keys = ragged.summary_absorb(None, ragged.pack(state.kh, plan.src), ragged.pack(state.vh, plan.src), plan, T, cap,
                                     model.attn.projection_matrix, state.lens)
    return ContextState(model, T, max(keys.lens), fingerprint(model), "attention", keys=keys, wq=state.wq, lens=keys.lens, form="summary")


def _absorb(ad, state, images, labels, add, wq):
    """`add[t]` of the slots of images / labels [T, n, ...] into the summary state (state None: a fresh one): only those shots go
    through the per-shot stage, as a packed list, and nothing absorbed earlier is read again."""
    model = ad.model
    T, n = model.task_num, images.shape[1]
    plan = ragged.Plan((0,) * T, add, n, n, images.device)
    keys = None if state is None else state.keys
    if plan.n:
        new_k, new_v = ad.shot_rows(ragged.pack(_images(model, images), plan.src), ragged.pack(labels.reshape(T, n, -1), plan.src))
        keys = ragged.summary_absorb(keys, new_k, new_v, plan, T, n, model.attn.projection_matrix, add)
    return ContextState(model, T, max(keys.lens), fingerprint(model), "attention", keys=keys, wq=wq, lens=keys.lens, form="summary")


def _grow(ad, state, lens, capacity, images, labels, add, wq, form="keys"):
    """`add[t]` of the slots of images / labels [T, n, ...] behind task t's lens[t] kept rows (state None: nothing kept yet), then the
    finishing step on the kept rows.  The valid shots travel as a packed list: a slot that is no shot is never read."""
    model = ad.model
    T, n, dev = model.task_num, images.shape[1], images.device
    plan = ragged.Plan(lens, add, n, capacity, dev)
    a_rows, b_rows = (None, None) if state is None else (state.kh, state.vh) if model.ATTENTION else (state.rs, state.lv)
    if state is not None and a_rows is None:
        raise ValueError("extend: the state carries no per-shot rows (it was not made by condition())")
    if plan.n:
        shots = (ragged.pack(_images(model, images), plan.src), ragged.pack(labels.reshape(T, n, -1), plan.src))
        # "paged" (DESIGN.md 6c-11): the Linears of the per-shot stage through the row-invariant kernel - a shot's rows have the
        # same bits whatever shares the call, so a state grown by extend IS the state conditioned on all its shots
        new_a, new_b = ad.shot_rows(*shots, invariant=True) if form == "paged" else ad.shot_rows(*shots)
        if state is None:
            a_rows = torch.zeros(T, capacity, *new_a.shape[1:], device=dev)
            b_rows = torch.zeros_like(a_rows) if new_b is not None else None
        a_rows = ragged.scatter(a_rows, plan.dst, new_a)
        b_rows = ragged.scatter(b_rows, plan.dst, new_b) if new_b is not None else None
    if model.ATTENTION:
        keys = ragged.masked_keys(a_rows, model.attn.projection_matrix, plan, form)
        return ContextState(model, T, capacity, fingerprint(model), "attention", keys=keys, vh=b_rows, wq=wq, lens=plan.total, kh=a_rows, form=form)
    return _latent(ad, capacity, a_rows, b_rows, ragged.gathered_aggregate(model.agg_mode, a_rows, b_rows, plan), plan.total)


def _latent(ad, Nc, rs, lv, r, lens=None):
    """The latent state behind the aggregate r [T, R] of the per-shot rows rs, lv [T, Nc, R]."""
    z = LinearFunction.apply(r, ad.finish.weight, ad.finish.bias, "none")
    return ContextState(ad.model, rs.shape[0], Nc, fingerprint(ad.model), "latent", z=z, lens=lens, rs=rs, lv=lv, r=r)


def _refuse_attention(ad, state):
    """predict(return_attention=True): what has no per-shot weights to read out.  Host checks only."""
    if state.kind != "attention":
        raise ValueError(f"predict: return_attention=True - {type(ad.model).__name__} (agg_mode {ad.model.agg_mode!r}) has no attention: its "
                         f"state is {state.kind!r}, the context enters the prediction as one aggregate")
    if state.form == "summary":
        raise ValueError("predict: return_attention=True - a summary state keeps no per-shot rows, so there is no weight per context shot to "
                         'read out (condition with the default form="keys" for at most 32 shots, or with form="long" for at most '
                         f"{ragged.MAX_LONG_CAPACITY})")
    if state.keys.route not in PER_SHOT_ROUTES:
        raise ValueError("predict: return_attention=True needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, "
                         f"16 <= m <= 1536); this state's keys are kept {state.keys.route!r} (T, Nc, H, d, m = {state.keys.dims})")


def _refuse_mask(ad, state, mask, Nq):
    """predict(context_mask=): what has no per-shot column to mask, a mask of the wrong shape or dtype, and a (task, group, target)
    left without a valid shot.  Host checks only, in that order; the last costs ONE host read of a reduced mask
    (a bool per task), whichever device the mask lies on.  -> the mask as [T, G, Nq, Nc slots]."""
    if state.kind != "attention":
        raise ValueError(f"predict: context_mask= - {type(ad.model).__name__} (agg_mode {ad.model.agg_mode!r}) has no attention: its "
                         f"state is {state.kind!r}, the context enters the prediction as one aggregate with no per-shot column to mask")
    if state.form == "summary":
        raise ValueError("predict: context_mask= - a summary state keeps no per-shot rows, so there is no column per context shot to "
                         'mask (condition with the default form="keys" for at most 32 shots, or with form="long" for at most '
                         f"{ragged.MAX_LONG_CAPACITY})")
    if state.keys.route not in PER_SHOT_ROUTES:
        raise ValueError("predict: context_mask= needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, "
                         f"16 <= m <= 1536); this state's keys are kept {state.keys.route!r} (T, Nc, H, d, m = {state.keys.dims})")
    T, Nc = state.T, state.Nc
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        got = str(mask.dtype) if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f"predict: context_mask must be a bool tensor (True = the target sees the slot), got {got}")
    if mask.dim() not in (3, 4) or (mask.shape[0], mask.shape[-2], mask.shape[-1]) != (T, Nq, Nc) or mask.shape[1] < 1:
        raise ValueError(f"predict: context_mask must be [T={T}, Nq={Nq}, Nc={Nc} slots] or [T, G, Nq, Nc], got {tuple(mask.shape)}")
    mask4 = mask if mask.dim() == 4 else mask[:, None]
    valid = torch.arange(Nc)[None, :] < torch.tensor(state.lens)[:, None]                          # [T, Nc]
    kept = (mask4 & valid.to(mask.device)[:, None, None, :]).any(dim=-1)                            # [T, G, Nq]
    if not bool(kept.all()):                                                                        # the one host read
        t, g, n = (int(x) for x in (~kept).nonzero()[0])
        raise ValueError(f"predict: context_mask keeps none of the {state.lens[t]} valid context shots of task {t} for target {n}"
                         f"{f' in group {g}' if mask.dim() == 4 else ''}: its attention is 0 / 0")
    return mask4


def prune_choice(score, lens, keep):
    """prune's slot choice, host work only: score [T][Nc] (numbers; any nested sequence, array or CPU tensor), lens the valid slots
    per task, keep an int or T ints >= 1 -> drop, T ascending lists of slot indices: per task the valid slots that are NOT among the
    keep[t] with the largest score.  Ties go to the lower slot index; a task with lens[t] <= keep[t] drops nothing."""
    T = len(lens)
    if isinstance(keep, bool) or (isinstance(keep, numbers.Integral) and not isinstance(keep, bool)):
        keep = [keep] * T
    elif isinstance(keep, torch.Tensor):
        keep = keep.tolist()
    try:
        keep = list(keep)
    except TypeError:
        raise ValueError(f"prune: keep must be an int or a sequence of {T} ints, got {type(keep).__name__}") from None
    if len(keep) != T:
        raise ValueError(f"prune: keep has {len(keep)} entries for {T} tasks")
    for k in keep:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral):
            raise ValueError(f"prune: keep must hold integers, got {k!r}")
    if min(keep) < 1:
        raise ValueError(f"prune: keep must be at least 1 for every task (a task without a context shot has no attention), got {[int(k) for k in keep]}")
    drop = []
    for t in range(T):
        if score is None or lens[t] <= keep[t]:
            drop.append([])
            continue
        row = [float(x) for x in score[t][:lens[t]]]
        order = sorted(range(lens[t]), key=lambda c: (-row[c], c))
        drop.append(sorted(order[int(keep[t]):]))
    return drop


def prune(ad, state, qry_x, keep, target_weight=None, chunk=None):
    """(per-shot attention state, target images [T, Nq, ...], keep) -> (a NEW state, drop): per task the keep[t] valid slots with the
    largest attention mass of these targets, summed over the heads (predict(attention_mass=True, target_weight=)),
    stay - in their order - and the rest go through evict, whose statement about the key stabiliser holds: it becomes the maximum
    over the shots that remain.  `drop` is what evict was given, T ascending slot lists, for a caller's log.  Ties go to the lower
    slot index; a task with lens[t] <= keep[t] is untouched.  One device-to-host copy of [T, Nc] floats."""
    what = "prune"
    _enter(ad, what, state, qry_x, "targets")
    _refuse_rowless(what, state, "a summary has no per-shot weights to prune by")
    prune_choice(None, state.lens, keep)                                   # keep's own refusals, before any launch
    _, mass = predict(ad, state, qry_x, chunk, attention_mass=True, target_weight=target_weight)
    score = mass[:, 0]
    for h in range(1, mass.shape[1]):                                      # the heads in ascending order: one order, whatever torch.sum's
        score = score + mass[:, h]
    drop = prune_choice(score.cpu(), state.lens, keep)                     # the one device-to-host copy
    return evict(ad, state, drop), drop


def _refuse_mass(ad, state, chunk, return_attention, context_mask):
    """predict(attention_mass=True): what it does not combine with, the states without per-shot weights - in the read-out's words -
    and a chunk that would split a 16-row tile.  Host checks only."""
    if return_attention:
        raise ValueError("predict: attention_mass=True with return_attention=True - the mass exists so that attn [T, H, Nq, Nc] is never "
                         "stored; ask for one of the two (the mass is attn summed over the targets)")
    if context_mask is not None:
        raise ValueError("predict: attention_mass=True with context_mask= - the masked read-outs have no reduced form; ask for "
                         "return_attention=True with the mask and sum over the targets")
    try:
        _refuse_attention(ad, state)
    except ValueError as e:
        raise ValueError(str(e).replace("return_attention=True", "attention_mass=True")) from None
    if chunk is not None and int(chunk) % 16:
        raise ValueError(f"predict: attention_mass=True sums the targets in tiles of 16 rows; chunk must be a multiple of 16 so that "
                         f"every chunk starts on a tile and the mass is the same bits for every chunk size, got {chunk}")


def _refuse_topk(ad, state, top_k, return_attention, context_mask, attention_mass):
    """predict(top_k=): a k outside 1 .. 16, what it does not combine with, and the states without per-shot weights - in the read-out's
    words.  Host checks only.  -> k as an int."""
    k = topk_arg("predict", top_k)
    if return_attention:
        raise ValueError("predict: top_k= with return_attention=True - the top-k exists so that attn [T, H, Nq, Nc] is never stored; ask "
                         "for one of the two (torch.topk of attn gives the same weights)")
    if context_mask is not None:
        raise ValueError("predict: top_k= with context_mask= - the masked read-outs have no reduced form; ask for return_attention=True "
                         "with the mask and take torch.topk of it")
    if attention_mass:
        raise ValueError("predict: top_k= with attention_mass=True - each is one reduction of the read-out inside the query launch (over "
                         "the slots, over the targets); ask for one per call")
    try:
        _refuse_attention(ad, state)
    except ValueError as e:
        raise ValueError(str(e).replace("return_attention=True", "top_k=")) from None
    return k


def _shared_images(model, qry_x):
    """predict(shared_targets=True): qry_x [Nq, C, H, W] (or [Nq, H, W] for one channel) -> [Nq, C, H, W]; a tensor with a task axis,
    or of another image shape, is a ValueError."""
    C, H, W = model.img_channels, model.img_size[0], model.img_size[1]
    if not isinstance(qry_x, torch.Tensor) or not (tuple(qry_x.shape[1:]) == (C, H, W) or (C == 1 and tuple(qry_x.shape[1:]) == (H, W))):
        got = tuple(qry_x.shape) if isinstance(qry_x, torch.Tensor) else type(qry_x).__name__
        raise ValueError(f"predict: shared_targets=True takes qry_x [Nq, {C}, {H}, {W}] with no task axis - the same targets are asked of "
                         f"every task of the state - got {got}; targets of their own per task go through the call without shared_targets")
    return qry_x.reshape(qry_x.shape[0], C, H, W)


def predict_shared(ad, state, qry_x, chunk=None, return_attention=False, context_mask=None, attention_mass=False, target_weight=None, top_k=None):
    """predict(shared_targets=True): (state, target images [Nq, ...] WITHOUT a task axis) -> mu [T, Nq, y_dim], the
    prediction of every stored context of the state for the same Nq targets; return_attention=True -> (mu, attn [T, H, Nq, Nc slots]).
    The targets go through the encoder / the trunks ONCE, as Nq images, the query-head Linear runs on Nq rows and the attention is
    ONE launch that forms the query features once per 16 targets for all tasks (mlhot.ops.favor_query(shared=True)); only the
    Linears behind it see T * Nq rows, through linear_rows, whose sources broadcast.  Latent and empty states are served: z[t]
    against the shared target rows.  Per-shot states "keys" and "long".  Every refusal is a ValueError before any launch."""
    what = "predict"
    _own(ad, what, state)
    for on, name in ((context_mask is not None, "context_mask="), (attention_mass, "attention_mass=True"), (target_weight is not None, "target_weight="),
                     (top_k is not None, "top_k=")):
        if on:
            raise ValueError(f"predict: shared_targets=True with {name} - the shared-target launch forms the plain read-out alone (mu, and attn "
                             "with return_attention=True); masks, the attention mass and the top-k run on per-task targets: expand qry_x "
                             "to [T, Nq, ...] and call without shared_targets")
    if state.form in ("summary", "paged"):
        raise ValueError(f'predict: shared_targets=True serves per-shot states of form "keys" and "long" and latent states; this state is a '
                         f'{state.form!r} state, for which no shared-target kernel is built - expand qry_x to [T, Nq, ...] and call '
                         "without shared_targets")
    if state.kind == "attention" and state.keys.route not in ("cached", "long"):
        raise ValueError("predict: shared_targets=True needs the cached kernels' envelope (Nc <= 32 or form=\"long\", d % 16 == 0, d <= 256, "
                         f"16 <= m <= 1536); this state's keys are kept {state.keys.route!r} (T, Nc, H, d, m = {state.keys.dims})")
    imgs = _shared_images(ad.model, qry_x)
    Nq = imgs.shape[0]
    if Nq < 1:
        raise ValueError("predict needs at least one target")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"predict: chunk must be a positive number of targets, got {chunk}")
    if return_attention:
        _refuse_attention(ad, state)
    ad.route_shared(state, imgs)
    step = Nq if chunk is None else min(int(chunk), Nq)
    with torch.no_grad():
        if return_attention:
            out, att = zip(*[ad.predict_shared(state, imgs[i:i + step], attention=True) for i in range(0, Nq, step)])
            return (out[0], att[0]) if len(out) == 1 else (torch.cat(out, dim=1), torch.cat(att, dim=2))
        out = [ad.predict_shared(state, imgs[i:i + step]) for i in range(0, Nq, step)]
    return out[0] if len(out) == 1 else torch.cat(out, dim=1)


def predict(ad, state, qry_x, chunk=None, return_attention=False, context_mask=None, attention_mass=False, target_weight=None, top_k=None):
    """(state, target images [T, Nq, ...]) -> mu [T, Nq, y_dim] for the context the state was made from, any Nq >= 1.  `chunk` bounds
    the targets per launch sequence.  `return_attention`: -> (mu, attn), attn [T, H, Nq, Nc slots] FAVOR+'s weight of
    every context slot per head and target (mlhot.ops.favor_query(weights=True)), exact zeros at the slots behind a task's ctx_len,
    concatenated over the chunks like mu; mu has the bits of the call without it on the same route.

    `context_mask`: bool [T, Nq, Nc slots] - target n of task t attends only to the slots whose entry is True -
    -> mu [T, Nq, y_dim]; or [T, G, Nq, Nc] for G masks of the same targets -> mu [T, G, Nq, y_dim] and attn [T, G, H, Nq, Nc], from
    ONE encoder pass over the targets and one masked query launch per chunk (mlhot.ops.favor_query(mask=)).  The key stabiliser
    stays the state's.  Refusals: _refuse_mask.

    `attention_mass`: -> (mu, mass), mass [T, H, Nc slots] = sum over the targets n of target_weight[t, n] *
    attn[t, :, n, :] (`target_weight` [T, Nq] finite and >= 0; None: the plain sum), reduced inside the query launch
    (mlhot.ops.favor_query(mass=)) - attn itself is never stored.  The chunks hand back their 16-row tile partials and ONE fold
    runs behind the last chunk, so the mass has the same bits for every chunk (a multiple of 16) and for chunk=None.  mu has the
    bits of the call without it on the same route.  Refusals: _refuse_mass.

    `top_k`: an integer k in 1 .. 16 -> (mu, idx, w), idx int32 and w fp32 [T, H, Nq, k]: per head and target the k
    valid slots of largest un-normalised score (descending, ties to the lower slot) and their attention weights, the bits attn has
    there, selected inside the query launch (mlhot.ops.favor_query(topk=)) - attn itself is never stored; -1 / 0 behind a task's
    shots.  The result is per target row, so the chunks are concatenated along the target axis and ANY chunk gives chunk=None's
    bits.  mu has the bits of the call without it on the same route.  Refusals: _refuse_topk."""
    _enter(ad, "predict", state, qry_x, "targets")
    Nq = qry_x.shape[1]
    if Nq < 1:
        raise ValueError("predict needs at least one target")
    if chunk is not None and int(chunk) < 1:
        raise ValueError(f"predict: chunk must be a positive number of targets, got {chunk}")
    if target_weight is not None and not attention_mass:
        raise ValueError("predict: target_weight= weighs the targets of attention_mass=True; without it there is nothing to weigh")
    if top_k is not None:
        k = _refuse_topk(ad, state, top_k, return_attention, context_mask, attention_mass)
        ad.route(state, qry_x)
        step = Nq if chunk is None else min(int(chunk), Nq)
        with torch.no_grad():
            res = [ad.predict_targets(state, qry_x[:, i:i + step], attention=("topk", k)) for i in range(0, Nq, step)]
        if len(res) == 1:
            return res[0][0], res[0][1][0], res[0][1][1]
        return torch.cat([r[0] for r in res], dim=1), torch.cat([r[1][0] for r in res], dim=2), torch.cat([r[1][1] for r in res], dim=2)
    if attention_mass:
        _refuse_mass(ad, state, chunk, return_attention, context_mask)
        tw = target_weight_arg("predict", target_weight, state.T, Nq, qry_x.device, ValueError)
        ad.route(state, qry_x)
        step = Nq if chunk is None else min(int(chunk), Nq)
        with torch.no_grad():
            out, part = zip(*[ad.predict_targets(state, qry_x[:, i:i + step], attention="mass",
                                                 target_weight=None if tw is None else tw[:, i:i + step].contiguous())
                              for i in range(0, Nq, step)])
            mass = lib().favor_mass_fold(part[0] if len(part) == 1 else torch.cat(part, dim=2))
        return (out[0] if len(out) == 1 else torch.cat(out, dim=1)), mass
    if return_attention:
        _refuse_attention(ad, state)
    if context_mask is not None:
        mask4 = _refuse_mask(ad, state, context_mask, Nq)
        ad.masked = True
        ad.route(state, qry_x)
        step = Nq if chunk is None else min(int(chunk), Nq)
        with torch.no_grad():
            words = ragged.pack_mask(mask4.to(qry_x.device), state.Nc)                              # [T, G, Nq, W]
            res = [ad.predict_targets(state, qry_x[:, i:i + step], attention=return_attention, mask_words=words[:, :, i:i + step].contiguous())
                   for i in range(0, Nq, step)]
        if return_attention:
            mu, att = (r[0] if len(res) == 1 else torch.cat(r, dim=k) for r, k in zip(zip(*res), (2, 3)))
        else:
            mu, att = res[0] if len(res) == 1 else torch.cat(res, dim=2), None
        if context_mask.dim() == 3:
            mu, att = mu[:, 0], None if att is None else att[:, 0]
        return (mu, att) if return_attention else mu
    ad.route(state, qry_x)
    step = Nq if chunk is None else min(int(chunk), Nq)
    with torch.no_grad():
        if return_attention:
            out, att = zip(*[ad.predict_targets(state, qry_x[:, i:i + step], attention=True) for i in range(0, Nq, step)])
            return (out[0], att[0]) if len(out) == 1 else (torch.cat(out, dim=1), torch.cat(att, dim=2))
        out = [ad.predict_targets(state, qry_x[:, i:i + step]) for i in range(0, Nq, step)]
    return out[0] if len(out) == 1 else torch.cat(out, dim=1)
