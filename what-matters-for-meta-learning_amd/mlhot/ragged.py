"""Per-task context sizes and growing states for cached-context inference: what ResNetNP.condition / extend and
mlhot.cached.condition / extend share.  The argument checks are host work only and raise ValueError before anything touches the
GPU; the device part is index arithmetic on the kept per-shot rows and the two finishing steps - the masked key state
(mlhot.ops.favor_keys with lens) or the prefix aggregate with a gather of row lens[t] - 1 (mlhot.ops.agg_prefixes)."""
import numbers

import torch

from mlhot.ops import agg_prefixes, favor_absorb, favor_keys, favor_keys_long, favor_keys_paged, favor_retract, host_lens

MAX_ATTENTION_CAPACITY = 32        # the cached FAVOR+ kernels' envelope on the context side (csrc/favor_cached.h)
MAX_LONG_CAPACITY = 256            # the long per-shot kernels' (csrc/favor_long.h)
MAX_PAGED_CAPACITY = 4096          # the paged per-shot kernels' (csrc/favor_paged.h)
# what an attention state holds: per-shot key features (<= 32 slots), the fixed-size summary, per-shot key features in 32-slot
# chunks (<= 256 slots), or the same with the query in 256-slot pages (<= 4096 slots)
FORMS = ("keys", "summary", "long", "paged")
# the forms with per-shot rows beyond "keys": the masked path always, one capacity each
PER_SHOT_CAPACITY = {"long": MAX_LONG_CAPACITY, "paged": MAX_PAGED_CAPACITY}


def condition_args(what, T, Nslots, ctx_len, capacity, attention):
    """-> (lens, capacity), or (None, Nslots) for the call without ctx_len / capacity (the unmasked path, as before)."""
    if ctx_len is None and capacity is None:
        return None, Nslots
    lens = (Nslots,) * T if ctx_len is None else host_lens(ctx_len, T, 1, Nslots, f"{what}: ctx_len", ValueError)
    if Nslots < 1:
        raise ValueError(f"{what}: capacity= needs at least one context shot to start from")
    if capacity is None:
        capacity = Nslots
    if isinstance(capacity, bool) or not isinstance(capacity, numbers.Integral):
        raise ValueError(f"{what}: capacity must be an integer, got {capacity!r}")
    capacity = int(capacity)
    if capacity < Nslots:
        raise ValueError(f"{what}: capacity = {capacity} is smaller than the {Nslots} context slots handed in")
    if attention and capacity > MAX_ATTENTION_CAPACITY:
        raise ValueError(f"{what}: capacity = {capacity} is outside the cached attention kernels' envelope "
                         f"(at most {MAX_ATTENTION_CAPACITY} context slots per task)")
    return lens, capacity


def check_form(what, form):
    if form not in FORMS:
        raise ValueError(f"{what}: form must be one of {FORMS}, got {form!r}")
    return form


def summary_condition_args(what, T, Nslots, ctx_len, capacity, attention):
    """-> lens for condition(form="summary"): any number of slots, no capacity."""
    if not attention:
        raise ValueError(f'{what}: form="summary" serves the attention models; a latent state is one aggregate per task and is not '
                         "capped at 32 shots - use the default form")
    if capacity is not None:
        raise ValueError(f'{what}: form="summary" takes no capacity - a summary state has a fixed size and absorbs any number of shots')
    if Nslots < 1:
        raise ValueError(f'{what}: form="summary" needs at least one context shot')
    return (Nslots,) * T if ctx_len is None else host_lens(ctx_len, T, 1, Nslots, f"{what}: ctx_len", ValueError)


def long_condition_args(what, T, Nslots, ctx_len, capacity, attention, form="long"):
    """-> (lens, capacity) for condition(form="long" | "paged"): always the masked path, lens defaults to every slot full
    (DESIGN.md 6c-7, 6c-11)."""
    if not attention:
        raise ValueError(f'{what}: form="{form}" serves the attention models; a latent state is one aggregate per task and is not '
                         "capped at 32 shots - use the default form")
    if Nslots < 1:
        raise ValueError(f'{what}: form="{form}" needs at least one context shot')
    lens = (Nslots,) * T if ctx_len is None else host_lens(ctx_len, T, 1, Nslots, f"{what}: ctx_len", ValueError)
    if capacity is None:
        capacity = Nslots
    if isinstance(capacity, bool) or not isinstance(capacity, numbers.Integral):
        raise ValueError(f"{what}: capacity must be an integer, got {capacity!r}")
    capacity = int(capacity)
    if capacity < Nslots:
        raise ValueError(f"{what}: capacity = {capacity} is smaller than the {Nslots} context slots handed in")
    if capacity > PER_SHOT_CAPACITY[form]:
        raise ValueError(f"{what}: capacity = {capacity} is outside the {form} attention kernels' envelope "
                         f"(at most {PER_SHOT_CAPACITY[form]} context slots per task)")
    return lens, capacity


def summary_extend_args(what, T, n, new_len):
    """-> the new shots per task for extend on a summary state: 0 .. n each, no capacity to check."""
    if n < 1:
        raise ValueError(f"{what}: no new context slot handed in")
    return (n,) * T if new_len is None else host_lens(new_len, T, 0, n, f"{what}: new_len", ValueError)


def summary_absorb(keys, new_k, new_v, plan, T, n, proj, add):
    """The packed head rows new_k, new_v [P, H, d] of the valid new shots (plan.dst: their flat slots t * n + j) into the summary
    state `keys` (None: a fresh one) -> the new summary state (mlhot.ops.favor_absorb; the old one stays valid)."""
    kh = torch.zeros(T * n, *new_k.shape[1:], device=new_k.device)
    vh = torch.zeros_like(kh)
    kh.index_copy_(0, plan.dst, new_k)
    vh.index_copy_(0, plan.dst, new_v)
    return favor_absorb(keys, kh.view(T, n, *new_k.shape[1:]), vh.view(T, n, *new_k.shape[1:]), proj, lens=add)


def summary_retract(keys, old_k, old_v, plan, T, n, proj, sub):
    """summary_absorb with the sign turned: the packed head rows old_k, old_v [P, H, d] of the shots to take out (plan.dst: their flat
    slots t * n + j) out of the summary state `keys` -> the new summary state (mlhot.ops.favor_retract; the old one stays valid)."""
    kh = torch.zeros(T * n, *old_k.shape[1:], device=old_k.device)
    vh = torch.zeros_like(kh)
    kh.index_copy_(0, plan.dst, old_k)
    vh.index_copy_(0, plan.dst, old_v)
    return favor_retract(keys, kh.view(T, n, *old_k.shape[1:]), vh.view(T, n, *old_k.shape[1:]), proj, lens=sub)


def extend_args(what, state, T, n, new_len):
    """-> the new shots per task; the state's own lens / capacity are checked against them."""
    lens, capacity = getattr(state, "lens", None), getattr(state, "capacity", None)
    if lens is None or capacity is None:
        raise ValueError(f"{what}: the state carries no per-shot rows (it was not made by condition())")
    add = (n,) * T if new_len is None else host_lens(new_len, T, 0, n, f"{what}: new_len", ValueError)
    over = [(t, l + a) for t, (l, a) in enumerate(zip(lens, add)) if l + a > capacity]
    if over:
        t, total = over[0]
        raise ValueError(f"{what}: task {t} would hold {total} context shots, the state's capacity is {capacity} - condition with "
                         "capacity= to reserve room for later shots")
    return add


def _slots(what, state):
    lens, capacity = getattr(state, "lens", None), getattr(state, "capacity", None)
    if lens is None or capacity is None or getattr(state, "kind", None) not in ("attention", "latent"):
        raise ValueError(f"{what}: the state carries no per-shot rows (it was not made by condition())")
    return lens, capacity


def evict_args(what, state, drop):
    """-> drop as T sorted tuples of slot indices: distinct host ints below lens[t], and every task keeps a shot."""
    lens, _ = _slots(what, state)
    if isinstance(drop, torch.Tensor):
        raise ValueError(f"{what}: drop must be a host sequence with one sequence of slot indices per task, got a tensor")
    try:
        drop = list(drop)
        if any(isinstance(d, torch.Tensor) and d.is_cuda for d in drop):
            raise ValueError(f"{what}: drop must hold host values (they are checked on the host), got a tensor on the GPU")
        drop = [list(d.tolist() if isinstance(d, torch.Tensor) else d) for d in drop]
    except TypeError:
        raise ValueError(f"{what}: drop must be a sequence with one sequence of slot indices per task, got {drop!r}") from None
    if len(drop) != len(lens):
        raise ValueError(f"{what}: drop has {len(drop)} entries, the state holds {len(lens)} tasks")
    out = []
    for t, (d, l) in enumerate(zip(drop, lens)):
        if any(isinstance(x, bool) or not isinstance(x, numbers.Integral) for x in d):
            raise ValueError(f"{what}: drop[{t}] must hold integers (host values: they are checked on the host), got {d!r}")
        d = [int(x) for x in d]
        if d and (min(d) < 0 or max(d) >= l):
            raise ValueError(f"{what}: drop[{t}] = {d} names a slot outside 0..{l - 1}, the {l} context shots task {t} holds")
        if len(set(d)) != len(d):
            raise ValueError(f"{what}: drop[{t}] = {d} names a slot twice")
        if len(d) >= l:
            raise ValueError(f"{what}: drop[{t}] would leave task {t} without a context shot (it holds {l}); a task keeps at least one")
        out.append(tuple(sorted(d)))
    return out


def keep_rows(lens, drop, capacity):
    """The plan of an eviction on the host: per task the source slot of every destination slot - the kept shots in their order,
    then -1 ("a row of zeros") up to the capacity - and the new lens."""
    rows, total = [], []
    for l, d in zip(lens, drop):
        gone = set(d)
        keep = [s for s in range(l) if s not in gone]
        rows.append(keep + [-1] * (capacity - len(keep)))
        total.append(len(keep))
    return rows, tuple(total)


class KeepPlan:
    """An eviction's indices on the device after ONE upload made before the first launch (Plan's rule): `rows` int32 [T, capacity]
    is what mlhot_rows_compact reads (keep_rows); `total`, `lens` and `last` are Plan's, for the finishing steps on the kept rows."""

    def __init__(self, lens, drop, capacity, device):
        T = len(lens)
        rows, self.total = keep_rows(lens, drop, capacity)
        last = [(l - 1) * T + t for t, l in enumerate(self.total)]
        buf = torch.tensor([s for r in rows for s in r] + last + list(self.total), dtype=torch.int32).to(device)
        self.rows, self.last, self.lens = buf[:T * capacity].view(T, capacity), buf[T * capacity:T * capacity + T].long(), buf[T * capacity + T:]


JOIN_PARTS = 8                     # states per concat / regroup call and parts per task (csrc/rows_gather.h: ROWS_GATHER_MAX_SRC)


def smallest_form(capacity):
    """The smallest per-shot form that holds `capacity` slots: "keys" up to 32, "long" up to 256, "paged" up to 4096."""
    return "keys" if capacity <= MAX_ATTENTION_CAPACITY else "long" if capacity <= MAX_LONG_CAPACITY else "paged"


def regroup_args(what, metas, picks, T, attention, form=None, capacity=None, name="picks"):
    """The host checks of mlhot.cached.regroup behind those of its states.  metas: (lens, capacity) per state;
    picks: one entry per task of the model's batch, a (state_index, task_index) pair or a list of 1 .. 8 such pairs
    -> (parts, the new lens, form, capacity): parts[t] the list of pairs of task t; `capacity` defaults to the largest total, `form`
    (attention only) to the smallest that holds the capacity.  `name`: what a message calls an entry ("picks", or concat's
    "states" - its parts are [(0, t), (1, t), ..])."""
    try:
        picks = list(picks)
    except TypeError:
        raise ValueError(f"{what}: picks must be a sequence with one entry per task, got {type(picks).__name__}") from None
    if len(picks) != T:
        raise ValueError(f"{what}: {len(picks)} picks, the model was built for tasks_per_batch = {T}")
    parts, total = [], []
    for t, pick in enumerate(picks):
        if isinstance(pick, (tuple, list)) and len(pick) == 2 and all(isinstance(x, numbers.Integral) and not isinstance(x, bool) for x in pick):
            pick = [pick]                               # one pair
        try:
            pick = [tuple(pair) for pair in pick]
        except TypeError:
            raise ValueError(f"{what}: picks[{t}] must be a (state_index, task_index) pair or a list of such pairs, got {pick!r}") from None
        if not pick:
            raise ValueError(f"{what}: picks[{t}] is empty - a task without a context shot has no attention (0 / 0) and no aggregate")
        if len(pick) > JOIN_PARTS:
            raise ValueError(f"{what}: picks[{t}] names {len(pick)} parts; a task takes at most {JOIN_PARTS} per call - calls nest: "
                             f"{what} the parts in groups, then the results")
        for pair in pick:
            if len(pair) != 2 or any(isinstance(x, bool) or not isinstance(x, numbers.Integral) for x in pair):
                raise ValueError(f"{what}: picks[{t}] holds {pair!r}, which is no (state_index, task_index) pair of integers")
            si, ti = pair
            if not 0 <= si < len(metas) or not 0 <= ti < len(metas[si][0]):
                tasks = f"states[{si}] holds {len(metas[si][0])} tasks" if 0 <= si < len(metas) else f"there are {len(metas)} states"
                raise ValueError(f"{what}: picks[{t}] names {pair}, which is out of range - {tasks}")
        if len(set(pick)) != len(pick):
            twice = next(pair for k, pair in enumerate(pick) if pair in pick[:k])
            raise ValueError(f"{what}: picks[{t}] names {twice} twice - its shots would count double inside one task (the same pair may "
                             "stand in different tasks)")
        parts.append([(int(si), int(ti)) for si, ti in pick])
        total.append(sum(metas[si][0][ti] for si, ti in pick))
    if capacity is None:
        capacity = max(max(total), 1)
    if isinstance(capacity, bool) or not isinstance(capacity, numbers.Integral):
        raise ValueError(f"{what}: capacity must be an integer, got {capacity!r}")
    capacity = int(capacity)
    if not attention and form is not None:
        raise ValueError(f"{what}: form= belongs to the attention models - a latent state keeps its per-shot rows in one layout at any "
                         f"capacity (got form={form!r})")
    if attention:
        if form is not None and form not in PER_SHOT_CAPACITY and form != "keys":
            hint = '; mlhot.cached.summarize maps the result to form="summary"' if form == "summary" else ""
            raise ValueError(f'{what}: form must be one of ("keys", "long", "paged") or None, got {form!r}{hint}')
        if capacity > MAX_PAGED_CAPACITY:
            raise ValueError(f"{what}: capacity = {capacity} is above the {MAX_PAGED_CAPACITY} slots of the largest per-shot form (\"paged\"); "
                             f'beyond it a context is held as form="summary": mlhot.cached.summarize the parts, then merge / select them')
        if form is None:
            form = smallest_form(capacity)
        cap = MAX_ATTENTION_CAPACITY if form == "keys" else PER_SHOT_CAPACITY[form]
        if capacity > cap:
            raise ValueError(f"{what}: capacity = {capacity} is outside the {form} attention kernels' envelope (at most {cap} context slots "
                             f'per task); form="{smallest_form(capacity)}" holds it')
    elif capacity > MAX_PAGED_CAPACITY:
        raise ValueError(f"{what}: capacity = {capacity} is above the {MAX_PAGED_CAPACITY} slots mlhot_rows_gather serves")
    for t, n in enumerate(total):
        if n > capacity:
            who = f"picks[{t}]" if name == "picks" else f"task {t} over all states"
            raise ValueError(f"{what}: {who} holds {n} context shots in all, the capacity is {capacity}")
        if n < 1:
            who = f"picks[{t}]" if name == "picks" else f"task {t} of the states"
            raise ValueError(f"{what}: {who} holds no context shot - a task without one has no attention (0 / 0) and no aggregate")
    return parts, tuple(total), form, capacity


def join_args(what, metas, T, attention, form=None, capacity=None):
    """regroup_args for mlhot.cached.concat: task t is task t of every state, in the states' order."""
    return regroup_args(what, metas, [[(i, t) for i in range(len(metas))] for t in range(T)], T, attention, form, capacity, name="states")


def gather_rows(parts, lens, caps, capacity):
    """The plan of a join on the host: parts[t] = [(state_index, task_index), ..]; lens[i] the shots per task of
    state i, caps[i] its capacity -> (table [T][capacity][2], the new lens).  Per task the lens[i][j] valid shots of every part
    (i, j) stand in the order given, as (i, flat row j * caps[i] + s); then (-1, -1) - "a row of zeros" - up to the capacity."""
    table, total = [], []
    for task in parts:
        rows = [(i, j * caps[i] + s) for i, j in task for s in range(lens[i][j])]
        total.append(len(rows))
        table.append(rows + [(-1, -1)] * (capacity - len(rows)))
    return table, tuple(total)


class GatherPlan:
    """A join's indices on the device after ONE upload made before the first launch (Plan's rule): `rows` int32 [T, capacity, 2] is
    what mlhot_rows_gather reads (gather_rows); `total`, `lens` and `last` are Plan's, for the finishing steps on the gathered rows."""

    def __init__(self, parts, lens, caps, capacity, device):
        T = len(parts)
        rows, self.total = gather_rows(parts, lens, caps, capacity)
        last = [(l - 1) * T + t for t, l in enumerate(self.total)]
        # lens in front, padded to 16 bytes: both it and rows start aligned, so no entry copies them on the way in (mlhot.ops._c)
        pad = -T % 4
        buf = torch.tensor(list(self.total) + [0] * pad + [x for r in rows for pair in r for x in pair] + last, dtype=torch.int32).to(device)
        a, n = T + pad, 2 * T * capacity
        self.rows, self.last, self.lens = buf[a:a + n].view(T, capacity, 2), buf[a + n:].long(), buf[:T]


def retract_args(what, state, T, n, old_len):
    """-> the shots per task a summary state gives up: 0 .. n each, and fewer than the task holds."""
    sub = summary_extend_args(what, T, n, old_len)
    for t, (s, l) in enumerate(zip(sub, state.lens)):
        if s >= l:
            raise ValueError(f"{what}: task {t} holds {l} context shots and would give up {s}; a task keeps at least one")
    return sub


def slide_args(what, state, T, n, new_len):
    """-> (the new shots per task, the oldest slots every task gives up for them): only as many as do not fit into the spare slots."""
    lens, capacity = _slots(what, state)
    if n < 1:
        raise ValueError(f"{what}: no new context slot handed in")
    add = (n,) * T if new_len is None else host_lens(new_len, T, 0, n, f"{what}: new_len", ValueError)
    for t, a in enumerate(add):
        if a > capacity:
            raise ValueError(f"{what}: task {t} takes {a} new context shots, the state's capacity is {capacity}")
    return add, [tuple(range(max(0, l + a - capacity))) for l, a in zip(lens, add)]


def pack_mask(mask, Nc):
    """A per-target context mask as the words the masked query kernels read: bool [T, Nq, Nc] (one group) or
    [T, G, Nq, Nc] -> int32 [T, G, Nq, ceil(Nc / 32)], bit j of word c = slot 32 c + j (the bit pattern of the kernels' uint32; the
    bits at slots >= Nc are 0).  Pure torch on the mask's device - a CPU tensor packs on the CPU."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() not in (3, 4):
        got = f"{mask.dtype} {tuple(mask.shape)}" if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f"pack_mask: mask must be a bool tensor [T, Nq, Nc] or [T, G, Nq, Nc], got {got}")
    if isinstance(Nc, bool) or not isinstance(Nc, numbers.Integral) or Nc < 1 or mask.shape[-1] != Nc:
        raise ValueError(f"pack_mask: the mask's last axis has {mask.shape[-1]} slots, Nc = {Nc!r} (at least 1)")
    if mask.dim() == 3:
        mask = mask[:, None]
    W = (Nc + 31) // 32
    bits = torch.nn.functional.pad(mask, (0, 32 * W - Nc)).reshape(*mask.shape[:-1], W, 32).to(torch.int64)
    words = (bits << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(dim=-1)            # 0 .. 2^32 - 1
    return torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32).contiguous()


class Plan:
    """Every index a growth step needs, on the device after ONE upload made before the first launch (an upload from pageable host
    memory waits for the stream: made later it would hold the host until the encoder is done).  `src` / `dst`: flat indices of the
    new valid slots, source t * src_stride + j and destination t * capacity + start[t] + j for j < count[t] (int64); `total` =
    start + count per task, host ints; `lens` the same as int32 on the device (what mlhot_favor_keys_ragged_fwd reads); `last`:
    row (total[t] - 1) * T + t of mlhot_agg_prefix_fwd's [capacity, T, R] output, flattened (int64)."""

    def __init__(self, start, count, src_stride, capacity, device):
        T = len(start)
        self.total = tuple(s + c for s, c in zip(start, count))
        src = [t * src_stride + j for t, c in enumerate(count) for j in range(c)]
        dst = [t * capacity + s + j for t, (s, c) in enumerate(zip(start, count)) for j in range(c)]
        last = [(l - 1) * T + t for t, l in enumerate(self.total)]
        buf = torch.tensor(src + dst + last + list(self.total), dtype=torch.int32).to(device)
        P = len(src)
        idx = buf[:2 * P + T].long()
        self.n, self.src, self.dst, self.last, self.lens = P, idx[:P], idx[P:2 * P], idx[2 * P:], buf[2 * P + T:]


def slot_indices(start, count, src_stride, dst_stride, device):
    """(src, dst) of a Plan alone."""
    plan = Plan(start, count, src_stride, dst_stride, device)
    return plan.src, plan.dst


def pack(t, idx):
    """Rows idx of t flattened over its first two axes [T, N, ...] -> [P, ...]."""
    return t.reshape(t.shape[0] * t.shape[1], *t.shape[2:]).index_select(0, idx)


def scatter(buf, idx, rows):
    """A copy of buf [T, cap, ...] (None: nothing kept yet - zeros of rows' trailing shape are the caller's to hand in) with
    rows [P, ...] written at the flat slots idx.  The old buffer stays as it is: the old state stays valid."""
    out = buf.clone()
    out.view(buf.shape[0] * buf.shape[1], *buf.shape[2:]).index_copy_(0, idx, rows.reshape(rows.shape[0], *buf.shape[2:]))
    return out


def masked_keys(kh, proj, plan, form="keys"):
    """The masked key state over the kept key rows kh [T, cap, H, d] (two launches): mlhot_favor_keys_ragged_fwd, for form "long"
    mlhot_favor_keys_long_fwd, for form "paged" mlhot_favor_keys_paged_fwd."""
    if form == "paged":
        return favor_keys_paged(kh, proj, lens=plan.total, lens_dev=plan.lens)
    if form == "long":
        return favor_keys_long(kh, proj, lens=plan.total, lens_dev=plan.lens)
    return favor_keys(kh, proj, lens=plan.total, lens_dev=plan.lens)


def gathered_aggregate(mode, rs, lv, plan):
    """mean / max / baco of every task's first total[t] rows of rs [T, cap, R]: mlhot_agg_prefix_fwd's row (total[t] - 1, t) - the
    operations of mlhot_agg_fwd on the slice, in its order.  -> r [T, R]"""
    T, cap, R = rs.shape
    return agg_prefixes(mode, rs, lv).view(cap * T, R).index_select(0, plan.last)          # of [cap, T, R]
