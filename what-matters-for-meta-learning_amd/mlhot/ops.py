"""torch.autograd bridges onto the C ABI (one Function per hot-path row of SURVEY.md §8a).

The Functions are glue only: they hand raw device pointers to libmlhot.so and keep the
opaque `saved` workspace alive between forward and backward.  There is NO eager/CPU
fallback - a tensor that is not on a HIP device raises.
"""
import numbers

import torch

from . import lib
from .binding import MlhotError


# Test / diagnostic hook: when set to a list, the whole-model and encoder bridges append (kind, dims | n_images, saved) for every
# forward, so that a parity test can read the kernels' own ReLU / pool routing decisions (binding.enc_routes, np_saved_views).
saved_taps = None


# Strict sharded parity of the FAVOR+ key stabiliser (mlhot.dist.StabiliserExchange): when set, the attention passes run as two
# staged calls around exchange.forward(x) / exchange.backward(x) on a 4-float device block (include/mlhot.h, "strict sharded parity").
_stab_exchange = None


def set_stabiliser_exchange(exchange):
    """exchange: an object with forward(x) / backward(x) (x: 4 floats on the device), or None for the rank-local stabiliser."""
    global _stab_exchange
    _stab_exchange = exchange


# The loss's gradient inside the model's backward.  LossFunc.calc_loss(mu, ., y).backward() is two dependent launches in front of
# the model's first backward kernel (the loss reduction, then d loss / d mu); the gradient needs no reduction, so when mu comes
# straight out of VanillaNPFunction the loss hands the model's backward a DESCRIPTOR (kind, labels, upstream scalar) instead of a
# gradient tensor, and the first backward kernel derives d loss / d mu itself (mlhot_np_vanilla_bwd_loss).  What autograd carries
# between the two nodes is a cached all-zero tensor of mu's shape: whatever else may flow into mu's gradient is ADDED to it by
# autograd as usual and the kernel adds the loss's share on top, so the result equals the unfused graph's for any consumer set.
#
# OPT-IN (round 6; it was a global default): the hand-over assumes that the backward pass which runs LossFunction.backward also runs
# the producer's node.  `loss.backward()` of a training step does; `torch.autograd.grad(loss, mu)` or `loss.backward(inputs=[mu])`
# stop at mu and would be handed the placeholder.  So only a caller that owns the whole step switches it on - `with
# loss_grad_in_backward():` around calc_loss + backward (trainer.ModelTrainer, bench.py's step) - and even there every hand-over is
# checked: LossFunction.backward queues an end-of-pass callback on the autograd engine, and a descriptor that is still parked on
# the producer when the pass ends (the pass stopped at mu, or raised in between) is removed and reported as an error instead of
# leaving zeros in somebody's gradient and a stale descriptor for the next pass.
defer_loss_grad = False
_zero_grads = {}


class loss_grad_in_backward:
    """Scope in which calc_loss(...).backward() leaves d loss / d mu to the model's first backward kernel (see above)."""

    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        global defer_loss_grad
        self.prev, defer_loss_grad = defer_loss_grad, bool(self.enabled)
        return self

    def __exit__(self, *exc):
        global defer_loss_grad
        defer_loss_grad = self.prev
        return False


def _zero_like(mu):
    key = (tuple(mu.shape), mu.device)
    z = _zero_grads.get(key)
    if z is None:
        z = _zero_grads[key] = torch.zeros_like(mu)
    return z


def _check_handed_over(node, desc):
    """End of the backward pass that parked `desc` on `node`: the producer's backward must have taken it."""
    def check():
        if node.loss is desc:
            node.loss = None
            raise RuntimeError("mlhot: the loss's gradient was left to the model's backward (loss_grad_in_backward), but this "
                               "backward pass ended without running it (autograd.grad(loss, mu) / backward(inputs=[mu])?): the "
                               "gradient handed out for mu is a placeholder of zeros.  Run such passes outside the scope.")
    return check


# The loss VALUE off the critical path.  Nothing in the backward reads the value, but as a launch of its own the reduction sits
# between the forward's last kernel and the backward's first.  Inside `with loss_value_aside():` a loss whose gradient is deferred to
# the model's backward (above) defers its value too: LossFunction.forward returns an UNWRITTEN scalar and the model's first backward
# kernel fills it from one extra workgroup (mlhot_loss_desc.value; the bits of mlhot_loss_fwd's result).  The caller promises to run
# the backward before it reads the loss and not to compute with the value in between (loss + kl * beta does: trainer.ModelTrainer
# switches this on only for a bare loss) - bench.py's step and the trainer's step are such callers.  Round 5: the first form of this
# switch ran the reduction on a forked stream (a parallel branch of the captured graph): 0.585 -> 0.608 ms per c3 step - a two-branch
# graph costs the step's other kernels more than the 4.7 us it takes out of the chain; this form has no branch.
_loss_aside = False


class loss_value_aside:
    """`enabled`: leave the loss VALUE to the backward as well; the scope always implies loss_grad_in_backward (the value rides on
    the gradient's descriptor)."""

    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        global _loss_aside, defer_loss_grad
        self.prev, _loss_aside = (_loss_aside, defer_loss_grad), bool(self.enabled)
        defer_loss_grad = True
        return self

    def __exit__(self, *exc):
        global _loss_aside, defer_loss_grad
        _loss_aside, defer_loss_grad = self.prev
        return False


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise MlhotError("mlhot: the hand-written HIP path needs tensors on a ROCm device "
                             "(got a CPU tensor); there is no CPU fallback")


def _c4(t):
    """Contiguous, at the tensor's own address: for mlhot_linear_fwd / _bwd, whose operands need 4-byte alignment only."""
    return t if t is None or t.is_contiguous() else t.contiguous()


def _c(t):
    """What every other entry may be handed (include/mlhot.h: all pointers 16-byte aligned): `t` itself when it is contiguous and
    aligned, else a copy - a contiguous tensor that starts inside its buffer (flat[1:].view(...)) is copied like a strided view."""
    if t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _need_aligned(what, *ts):
    """For operands that cannot be copied - buffers the kernels update in place or whose storage the caller's parameters are views
    of: refuse before anything is launched."""
    for t in ts:
        if t is not None and (not t.is_contiguous() or t.data_ptr() % 16):
            raise MlhotError(f"{what} must be contiguous and 16-byte aligned (include/mlhot.h); it cannot be copied on the way in")


class VanillaNPFunction(torch.autograd.Function):
    """Whole CNP/ANP vanilla forward+backward: mlhot_np_vanilla_fwd / _bwd."""

    @staticmethod
    def forward(ctx, dims, keys, proj, ctx_x, ctx_y, qry_x, *params):
        _need_gpu(ctx_x, ctx_y, qry_x, *params)
        L = lib()
        ctx_x, ctx_y, qry_x = _c(ctx_x.float()), _c(ctx_y.float()), _c(qry_x.float())
        pd = {k: _c(p.detach()) for k, p in zip(keys, params)}
        proj = _c(proj)
        # the exchange only concerns the attention models with a context (the empty-context branch has no keys)
        ctx.xchg = (_stab_exchange, torch.zeros(4, device=qry_x.device)) if _stab_exchange is not None and proj is not None and dims.Nc > 0 else None
        mu, saved, scratch = L.np_vanilla_fwd(dims, pd, ctx_x, ctx_y, qry_x, proj, exchange=ctx.xchg)
        if saved_taps is not None:
            saved_taps.append(("np", dims, saved))
        ctx.dims, ctx.keys, ctx.proj = dims, keys, proj
        ctx.takes_loss = ctx.xchg is None       # LossFunction may leave its gradient to this node's backward (a descriptor in ctx.loss)
        ctx.loss = None
        ctx.scratch = scratch
        ctx.save_for_backward(ctx_x, ctx_y, qry_x, mu, saved, *[pd[k] for k in keys])
        return mu

    @staticmethod
    def backward(ctx, dmu):
        ctx_x, ctx_y, qry_x, mu, saved, *params = ctx.saved_tensors
        pd = dict(zip(ctx.keys, params))
        loss, ctx.loss = ctx.loss, None
        if loss is not None and dmu.data_ptr() == _zero_like(mu).data_ptr():
            dmu = None                          # nothing but the loss flowed into mu: the kernel does not even read an addend
        grads = lib().np_vanilla_bwd(ctx.dims, pd, ctx_x, ctx_y, qry_x, mu, _c(dmu) if dmu is not None else None, saved, ctx.scratch, ctx.proj,
                                     exchange=ctx.xchg, loss=loss)
        ctx.scratch = None
        used = used_param_keys(ctx.keys, ctx.dims.Nc)
        return (None, None, None, None, None, None) + tuple(grads[k] if k in used else None for k in ctx.keys)


def used_param_keys(keys, Nc):
    """Parameters the forward touches: with an empty context only the image encoder and the
    decoder run (the zero-latent branch, ANPShapeNet1D.py:148-149), the rest get grad=None."""
    if Nc > 0:
        return set(keys)
    return {k for k in keys if k.startswith("encoder_w0.") or k.startswith("decoder0.")}


class EncVanillaFunction(torch.autograd.Function):
    """E1 alone: mlhot_enc_vanilla_fwd / _bwd on one image batch."""

    @staticmethod
    def forward(ctx, img, *params):
        _need_gpu(img, *params)
        img = _c(img.float())
        ps = [_c(p.detach()) for p in params]
        dim_w = ps[6].shape[0]
        feat, _, saved = lib().enc_vanilla_fwd(img, None, ps, dim_w)
        if saved_taps is not None:
            saved_taps.append(("enc", img.shape[0], saved))
        ctx.dim_w = dim_w
        ctx.save_for_backward(img, saved, *ps)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        img, saved, *ps = ctx.saved_tensors
        empty = torch.empty(0, ctx.dim_w, device=img.device)
        grads = lib().enc_vanilla_bwd(img, None, ps, ctx.dim_w, _c(dfeat), empty, saved)
        return (None,) + tuple(grads)


class LinearFunction(torch.autograd.Function):
    """y = act(x W^T + b): mlhot_linear_fwd / _bwd (rows = all leading dims)."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        _need_gpu(x, w, b)
        shp = x.shape
        x2 = _c4(x.reshape(-1, shp[-1]).float())
        y = lib().linear_fwd(x2, _c4(w.detach()), _c4(b.detach()) if b is not None else None, act)
        ctx.act, ctx.shp, ctx.has_b = act, shp, b is not None
        ctx.save_for_backward(x2, _c4(w.detach()), y, *([_c4(b.detach())] if b is not None else []))
        return y.view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, y, *bias = ctx.saved_tensors
        dx, dw, db = lib().linear_bwd(x2, w, y, _c4(dy.reshape(-1, w.shape[0])), ctx.act, need_dx=ctx.needs_input_grad[0],
                                      b=bias[0] if bias else None)
        return (dx.view(ctx.shp) if dx is not None else None), dw, (db if ctx.has_b else None), None


class StackedLinearFunction(torch.autograd.Function):
    """y = x [W_0; W_1; ...]^T + [b_0; b_1; ...] for the per-head Linear layers of the attention (networks/ANP.py:75-93 runs
    them one by one and stacks the outputs): ONE linear over the stacked weight.  `stack_w` / `stack_b` are the buffers the
    heads' parameters are views of (networks/_resnet_np.py::HeadStack), so nothing is concatenated per step; the backward's
    dW / db are handed to the heads as views of one gradient tensor."""

    @staticmethod
    def forward(ctx, x, stack_w, stack_b, n_heads, *head_params):
        _need_gpu(x, stack_w, stack_b)
        shp = x.shape
        x2 = _c4(x.reshape(-1, shp[-1]).float())
        y = lib().linear_fwd(x2, stack_w, stack_b, "none")
        ctx.shp, ctx.n_heads = shp, n_heads
        ctx.save_for_backward(x2, stack_w, y, stack_b)
        return y.view(*shp[:-1], stack_w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, y, b = ctx.saved_tensors
        dx, dw, db = lib().linear_bwd(x2, w, y, _c4(dy.reshape(-1, w.shape[0])), "none", need_dx=ctx.needs_input_grad[0], b=b)
        h = ctx.n_heads
        return ((dx.view(ctx.shp) if dx is not None else None), None, None, None,
                *dw.view(h, w.shape[0] // h, w.shape[1]).unbind(0), *db.view(h, -1).unbind(0))


class Linear2Function(torch.autograd.Function):
    """y = act(cat([xa, xb], -1) W^T + b) on few rows without the concatenation: the two inputs are the two k ranges of ONE launch
    (mlhot_linear_multi_* with a two-source job; the reference's torch.cat([x_ctx, labels]) -> Linear, ANP.py:113, and
    torch.cat([x, sample_features]) -> fc_mu, models.py:182-184).  Backward: both input gradients, dW and db in one launch."""

    @staticmethod
    def forward(ctx, xa, xb, w, b, act):
        _need_gpu(xa, xb, w, b)
        shp_a, shp_b = xa.shape, xb.shape
        a2, b2 = _c(xa.reshape(-1, shp_a[-1]).float()), _c(xb.reshape(-1, shp_b[-1]).float())
        wd, bd = _c(w.detach()), (_c(b.detach()) if b is not None else None)
        (y,) = lib().linear_multi_fwd([(a2, wd, bd, act, b2)])
        ctx.act, ctx.shp_a, ctx.shp_b, ctx.has_b = act, shp_a, shp_b, b is not None
        ctx.save_for_backward(a2, b2, wd, y, *([bd] if bd is not None else []))
        return y.view(*shp_a[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        a2, b2, w, y, *bias = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # the entry computes dW beside an input gradient (include/mlhot.h: the backward needs dx): with both inputs frozen it still
        # writes dxa, which is dropped here
        ((dxa, dw, db, dxb),) = lib().linear_multi_bwd([(a2, w, y, _c(dy.reshape(-1, w.shape[0]).float()), ctx.act, bias[0] if bias else None,
                                                         b2, need_a or not need_b, need_b)])
        return (dxa.view(ctx.shp_a) if need_a else None, dxb.view(ctx.shp_b) if dxb is not None else None, dw,
                db if ctx.has_b else None, None)


def linear2_ok(xa, xb, w):
    """Shapes the two-source few-row Linear takes (else: torch.cat + LinearFunction)."""
    rows = xa.numel() // xa.shape[-1]
    return (xa.is_cuda and rows <= 512 and xa.shape[-1] % 4 == 0 and xb.shape[-1] % 4 == 0 and xb.shape[-1] >= 4 and w.shape[0] % 4 == 0
            and xa.shape[-1] + xb.shape[-1] == w.shape[1])


class ScaledAddFunction(torch.autograd.Function):
    """a + alpha * x for same-shaped fp32 device tensors (the trainer's `loss + kl * beta`, trainer/model_trainer.py:77-78): one launch
    per direction instead of torch's mul + add (+ mul in the backward); the same two roundings."""

    @staticmethod
    def forward(ctx, a, x, alpha):
        _need_gpu(a, x)
        ctx.alpha = float(alpha)
        return lib().axpy(_c(a.float()), _c(x.float()), ctx.alpha)

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy.float())
        return (dy if ctx.needs_input_grad[0] else None), (lib().axpy(None, dy, ctx.alpha) if ctx.needs_input_grad[1] else None), None


def add_scaled(a, x, alpha):
    """a + x * alpha the way the reference writes it; fused into one launch when both are fp32 device tensors of one shape."""
    if torch.is_tensor(a) and torch.is_tensor(x) and a.is_cuda and x.is_cuda and a.shape == x.shape and a.dtype == x.dtype == torch.float32:
        return ScaledAddFunction.apply(a, x, alpha)
    if not torch.is_tensor(x) and x * alpha == 0:
        return a                           # the models without a KL term return the int 0: loss + 0 is loss, no launch
    return a + x * alpha


class MlpChainFunction(torch.autograd.Function):
    """Up to four Linear(+ReLU / tanh) layers on few rows in ONE launch (backward: two): mlhot_mlp_chain_fwd / _bwd
    (csrc/mlp_chain.h).  Layer k's input is the previous layer's output, optionally concatenated with a second tensor
    (`side`, before or behind it) - the reference's torch.cat([x, sample_features]) / cat([x_ctx, labels]) folded into the
    kernel.  Call through mlp_chain()."""

    @staticmethod
    def forward(ctx, spec, x0, *tensors):
        # spec: per layer (act, has_bias, has_side, side_first); tensors: per layer weight[, bias][, side]
        _need_gpu(x0, *tensors)
        shp = x0.shape
        x2 = _c(x0.reshape(-1, shp[-1]).float())
        layers, it, where = [], iter(range(len(tensors))), []
        for act, has_b, has_side, side_first in spec:
            iw = next(it)
            ib = next(it) if has_b else None
            isd = next(it) if has_side else None
            side = tensors[isd] if isd is not None else None
            layers.append((_c(tensors[iw].detach()), _c(tensors[ib].detach()) if ib is not None else None, act,
                           _c(side.detach().reshape(-1, side.shape[-1]).float()) if side is not None else None, side_first))
            where.append((iw, ib, isd))
        ys = lib().mlp_chain_fwd(x2, layers)
        ctx.spec, ctx.where, ctx.shp, ctx.n_t = spec, where, shp, len(tensors)
        ctx.side_shapes = [tensors[isd].shape if isd is not None else None for _, _, isd in where]
        flat = [x2]
        for (w, b, _, side, _), y in zip(layers, ys):
            flat += [w, y] + ([b] if b is not None else []) + ([side] if side is not None else [])
        ctx.save_for_backward(*flat)
        return ys[-1].view(*shp[:-1], ys[-1].shape[-1])

    @staticmethod
    def backward(ctx, dy):
        saved = list(ctx.saved_tensors)
        x2, pos = saved[0], 1
        layers, ys = [], []
        for act, has_b, has_side, side_first in ctx.spec:
            w, y = saved[pos], saved[pos + 1]
            pos += 2
            b = side = None
            if has_b:
                b, pos = saved[pos], pos + 1
            if has_side:
                side, pos = saved[pos], pos + 1
            layers.append((w, b, act, side, side_first))
            ys.append(y)
        need_side = [isd is not None and ctx.needs_input_grad[2 + isd] for _, _, isd in ctx.where]
        dx0, gl = lib().mlp_chain_bwd(x2, layers, ys, _c(dy.reshape(-1, dy.shape[-1]).float()), need_dx0=ctx.needs_input_grad[1],
                                      need_dside=need_side)
        grads = [None] * ctx.n_t
        for (iw, ib, isd), (dw, db, ds), shp in zip(ctx.where, gl, ctx.side_shapes):
            grads[iw] = dw
            if ib is not None:
                grads[ib] = db
            if isd is not None and ds is not None:
                grads[isd] = ds.view(shp)
        return (None, dx0.view(ctx.shp) if dx0 is not None else None) + tuple(grads)


def mlp_chain(x0, layers):
    """layers: [(weight, bias | None, act, side | None, side_first)] -> the last layer's output, or None when the shapes are
    outside the chain kernels' limits (the caller then runs the layers one by one)."""
    rows = x0.reshape(-1, x0.shape[-1])
    probe = [(w, b, act, side.reshape(-1, side.shape[-1]) if side is not None else None, sf) for w, b, act, side, sf in layers]
    if not x0.is_cuda or not lib().chain_ok(rows, probe):
        return None
    spec, tensors = [], []
    for w, b, act, side, side_first in layers:
        spec.append((act, b is not None, side is not None, bool(side_first)))
        tensors += [w] + ([b] if b is not None else []) + ([side] if side is not None else [])
    return MlpChainFunction.apply(tuple(spec), x0, *tensors)


class HeadStacksFunction(torch.autograd.Function):
    """The per-head Linear stacks of SEVERAL attention inputs (query, key, value: ANP.py:80-93) in one launch per direction:
    mlhot_linear_multi_fwd / _bwd over the stacked head weights (networks/_resnet_np.py::HeadStack).  Inputs: n stacks of
    (x [T, N, h], stacked weight [H h, h], stacked bias [H h]) followed by every head's own Parameters (their gradients are views of
    the stacks' gradient tensors).  Returns n tensors [T, N, H, h]."""

    @staticmethod
    def forward(ctx, n_heads, n_stacks, *args):
        xs, ws, bs = args[0:3 * n_stacks:3], args[1:3 * n_stacks:3], args[2:3 * n_stacks:3]
        _need_gpu(*xs, *ws, *bs)
        _need_aligned("HeadStacksFunction: a stacked weight / bias", *ws, *bs)
        x2 = [_c(x.reshape(-1, x.shape[-1]).float()) for x in xs]
        ys = lib().linear_multi_fwd([(x, w, b, "none") for x, w, b in zip(x2, ws, bs)])
        ctx.n_heads, ctx.n_stacks, ctx.shapes = n_heads, n_stacks, [x.shape for x in xs]
        ctx.save_for_backward(*x2, *ws, *ys, *bs)
        return tuple(y.view(*x.shape[:-1], n_heads, w.shape[0] // n_heads) for y, x, w in zip(ys, xs, ws))      # no -1: x may have no rows

    @staticmethod
    def backward(ctx, *dys):
        n, h = ctx.n_stacks, ctx.n_heads
        sv = ctx.saved_tensors
        x2, ws, ys, bs = sv[:n], sv[n:2 * n], sv[2 * n:3 * n], sv[3 * n:]
        outs = lib().linear_multi_bwd([(x, w, y, _c(dy.reshape(-1, w.shape[0]).float()), "none", b)
                                       for x, w, y, dy, b in zip(x2, ws, ys, dys, bs)])
        lead = []
        heads_w, heads_b = [], []
        for (dx, dw, db), shp, w in zip(outs, ctx.shapes, ws):
            lead += [dx.view(shp), None, None]
            heads_w.append(dw.view(h, w.shape[0] // h, w.shape[1]).unbind(0))
            heads_b.append(db.view(h, -1).unbind(0))
        per_stack = []
        for hw, hb in zip(heads_w, heads_b):          # the order HeadStack.params() hands the Parameters over: weights, then biases
            per_stack += list(hw) + list(hb)
        return (None, None) + tuple(lead) + tuple(per_stack)


class NTXentFunction(torch.autograd.Function):
    """NT-Xent of [N, d] embeddings whose labels are arange blocks, label(i) = (i // div) % mod: mlhot_nt_xent_fwd / _bwd
    (trainer/losses.py:82-99).  No host-side index tensors, no host -> device copies, capturable."""

    @staticmethod
    def forward(ctx, z, div, mod, t):
        _need_gpu(z)
        z2 = _c(z.float())
        loss, ws = lib().nt_xent_fwd(z2, div, mod, float(t))
        ctx.meta = (div, mod, float(t))
        ctx.save_for_backward(z2, ws)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        z2, ws = ctx.saved_tensors
        div, mod, t = ctx.meta
        return lib().nt_xent_bwd(z2, div, mod, t, ws, _c(dloss.float())), None, None, None


class AggFunction(torch.autograd.Function):
    """mean / max / baco over dim 1 of rs[T,Nc,R]: mlhot_agg_fwd / _bwd.
    For baco, `rs` is mu and `lv` the pre-softplus variance logits; returns (r, sigma_z)."""

    @staticmethod
    def forward(ctx, mode, rs, lv):
        _need_gpu(rs, lv)
        rs, lv = _c(rs), _c(lv)
        r, sigma, amax = lib().agg_fwd(mode, rs, lv)
        ctx.mode = mode
        ctx.save_for_backward(rs, lv, r, sigma, amax)
        ctx.mark_non_differentiable(sigma)
        return r, sigma

    @staticmethod
    def backward(ctx, dr, _dsigma):
        rs, lv, r, sigma, amax = ctx.saved_tensors
        drs, dlv = lib().agg_bwd(ctx.mode, rs, lv, r, sigma, amax, _c(dr))
        return None, drs, dlv


class FavorFunction(torch.autograd.Function):
    """FAVOR+ attention on token-major rows q[T,Nq,H,d], k/v[T,Nc,H,d] -> merged [T,Nq,d*H]."""

    @staticmethod
    def forward(ctx, q, k, v, proj):
        _need_gpu(q, k, v, proj)
        q, k, v, proj = _c(q), _c(k), _c(v), _c(proj)
        ctx.xchg = (_stab_exchange, torch.zeros(4, device=q.device)) if _stab_exchange is not None else None
        out, ws = lib().favor_fwd(q, k, v, proj, exchange=ctx.xchg)
        ctx.save_for_backward(q, k, v, proj, out, ws)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, proj, out, ws = ctx.saved_tensors
        dq, dk, dv = lib().favor_bwd(q, k, v, proj, out, _c(dout), ws, exchange=ctx.xchg)
        return dq, dk, dv, None


def favor_route(T, H, Nq, Nc, d, m):
    """Which implementation FavorFunction (lib().favor_fwd / favor_bwd) runs for these dimensions under the options as they stand:
    "two_launch" (csrc/favor2.h: both sides <= 32 shots), "linear" (csrc/favor_linear.h: option "favor_linear", above 32 shots) or
    "chain" (csrc/favor.h).  Options are read from what MlhotLib.set_option was told (MLHOT_OPTS included); under a stabiliser
    exchange (strict sharded parity) the passes are staged and never take the linear route."""
    L = lib()
    two = Nq <= 32 and Nc <= 32 and d % 16 == 0 and d <= 256 and 16 <= m <= 1536        # fv::applies (tests/test_favor_cases_cpu.py)
    if L.options.get("favor2", 1) and two:
        return "two_launch"
    if L.options.get("favor_linear", 0) and _stab_exchange is None and L.favor_linear_supported(T, H, Nq, Nc, d, m):
        return "linear"
    return "chain"


def apply_config_switches(config):
    """The library switches a run's config may set, read once by the trainer and the evaluator: config.favor_linear (absent = off)
    turns the option "favor_linear" on - FAVOR+ forward and backward in linear form above 32 shots.  It is set once,
    before any step, because a backward must run the route of its forward."""
    if getattr(config, "favor_linear", False) and torch.device(config.device).type == "cuda":
        lib().set_option("favor_linear", 1)


def _forward_only(what, *ts):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise MlhotError(f"{what} is forward-only (the evaluator's prefix sweep): call it under torch.no_grad() or on detached tensors")


def agg_prefixes(mode, feats, lv=None):
    """mean / max / baco over EVERY context prefix of feats [T, Nc, R] in one launch (csrc/prefix.h) -> r [Nc, T, R]:
    r[k-1] is AggFunction's result for feats[:, :k].  Forward only."""
    _forward_only("agg_prefixes", feats, lv)
    _need_gpu(feats, lv)
    r, _ = lib().agg_prefix_fwd(mode, _c(feats), _c(lv))
    return r


def favor_prefixes(qh, kh, vh, proj):
    """FAVOR+ attention for EVERY context prefix: q [T, Nq, H, d], k / v [T, Nc, H, d] -> [Nc, T, Nq, d*H], element k-1 =
    FavorFunction on kh[:, :k], vh[:, :k] (its batch-global key stabiliser over those k shots only).  Three launches
    (csrc/prefix.h) in favor2.h's shape regime; other shapes loop mlhot_favor_fwd over the prefixes.  Forward only."""
    _forward_only("favor_prefixes", qh, kh, vh, proj)
    _need_gpu(qh, kh, vh, proj)
    qh, kh, vh, proj = _c(qh), _c(kh), _c(vh), _c(proj)
    T, Nq, H, d = qh.shape
    Nc = kh.shape[1]
    if lib().favor_prefix_supported(T, H, Nq, Nc, d, proj.shape[0]):
        return lib().favor_prefix_fwd(qh, kh, vh, proj)
    return torch.stack([lib().favor_fwd(qh, kh[:, :k].contiguous(), vh[:, :k].contiguous(), proj)[0] for k in range(1, Nc + 1)])


PREFIX_LONG_MAX_K = 64     # prefixes per mlhot_favor_prefix_long_fwd call


def prefix_sizes(ks, Nc, what, exc=MlhotError):
    """ks (None: 1..Nc; a host int sequence or CPU integer tensor) -> a tuple of strictly increasing context sizes in 1..Nc, or `exc`."""
    if ks is None:
        return tuple(range(1, Nc + 1))
    if isinstance(ks, torch.Tensor):
        if ks.is_cuda or ks.is_floating_point() or ks.is_complex() or ks.dtype == torch.bool or ks.dim() != 1:
            raise exc(f"{what}: ks must be a host sequence of integers (its values are checked on the host)")
        ks = ks.tolist()
    try:
        ks = list(ks)
    except TypeError:
        raise exc(f"{what}: ks must be a sequence of context sizes, got {type(ks).__name__}") from None
    if any(isinstance(k, bool) or not isinstance(k, numbers.Integral) for k in ks):
        raise exc(f"{what}: ks must hold integers, got {ks}")
    ks = tuple(int(k) for k in ks)
    if not ks or min(ks) < 1 or max(ks) > Nc or any(b <= a for a, b in zip(ks, ks[1:])):
        raise exc(f"{what}: ks must be strictly increasing context sizes in 1..{Nc}, got {list(ks)}")
    return ks


def favor_prefixes_long(qh, kh, vh, proj, ks=None, lens=None):
    """FAVOR+ attention for the context prefixes `ks` of a context of ANY length: q [T, Nq, H, d], k / v [T, Nc, H, d], proj [m, d]
    -> [K, T, Nq, d*H], element i = FavorFunction on kh[:, :ks[i]], vh[:, :ks[i]] in exact arithmetic - its batch-global key
    stabiliser taken over those ks[i] shots only, and the key feature's floor relative to it.  `ks`: strictly increasing host ints
    in 1..Nc (default 1..Nc); more than 64 go out in calls of 64, and an element's bits do not depend on which others are asked for.
    `lens` (a host int sequence or CPU integer tensor of T values in 1..Nc; checked on the host, then uploaded and read on the
    device): task t's context is its first lens[t] shots - a prefix size above lens[t] saturates at lens[t] for that task, while the
    stabiliser of prefix i still follows every task's valid shots < ks[i]; rows of k AND v behind lens[t] are never read.  A task
    without a shot has no attention (0 / 0): lens = 0 is refused here.  The shots are walked in chunks of 32 with running sums
    (csrc/favor_prefix_long.h): three launches per call, no state of the context's size times m, row-invariant in the targets.
    d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, else MlhotError.  Forward only."""
    _forward_only("favor_prefixes_long", qh, kh, vh, proj)
    _need_gpu(qh, kh, vh, proj)
    qh, kh, vh, proj = _c(qh.detach()), _c(kh.detach()), _c(vh.detach()), _c(proj.detach())
    if qh.dim() != 4 or kh.dim() != 4 or vh.shape != kh.shape or qh.shape[1] < 1 or kh.shape[1] < 1 or proj.dim() != 2 or \
            (kh.shape[0], kh.shape[2], kh.shape[3]) != (qh.shape[0], qh.shape[2], qh.shape[3]) or proj.shape[1] != qh.shape[3]:
        raise MlhotError(f"favor_prefixes_long: q must be [T, Nq >= 1, H, d], k and v [T, Nc >= 1, H, d] and proj [m, d], got "
                         f"{tuple(qh.shape)}, {tuple(kh.shape)}, {tuple(vh.shape)}, {tuple(proj.shape)}")
    T, Nq, H, d = qh.shape
    Nc, m = kh.shape[1], proj.shape[0]
    ks = prefix_sizes(ks, Nc, "favor_prefixes_long")
    if lens is not None:
        lens = host_lens(lens, T, 1, Nc, "favor_prefixes_long: lens")
    if not lib().favor_prefix_long_supported(T, H, Nq, Nc, d, m, min(len(ks), PREFIX_LONG_MAX_K)):
        raise MlhotError(f"favor_prefixes_long serves d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, got d={d} m={m} (T={T} H={H} Nq={Nq} Nc={Nc})")
    dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(qh.device)      # the one upload, before the first launch
    out = torch.empty(len(ks), T, Nq, d * H, device=qh.device)
    for i in range(0, len(ks), PREFIX_LONG_MAX_K):
        lib().favor_prefix_long_fwd(qh, kh, vh, proj, ks[i:i + PREFIX_LONG_MAX_K], lens=dev, out=out[i:i + PREFIX_LONG_MAX_K])
    return out


PER_SHOT_ROUTES = ("cached", "long", "paged")      # the states that keep F_k per slot: weights and masks can be read out of them
TOPK_MAX = 16                                      # slots per row of the top-k read-out (csrc/favor_topk.h: one lane per kept slot)


class FavorKeyState:
    """What favor_keys / favor_absorb leave for favor_query.  `route` says what it holds: "cached" - `buf` is mlhot_favor_keys_fwd's
    state (the finished key features F_k and the batch-global stabiliser M; features() shows them) and favor_query is row-invariant;
    "plain" - a shape outside the cached kernels' envelope: `kh` itself, favor_query runs mlhot_favor_fwd, no invariance;
    "summary" - favor_absorb's fixed-size state (csrc/favor_summary.h; summary() shows it), any number of shots, row-invariant;
    "long" - favor_keys_long's state (csrc/favor_long.h): F_k and M in the "cached" layout for up to 256 slots,
    walked in chunks of 32; row-invariant, and like "cached" it reads out weights.  It carries `lens_dev`, the device copy of `lens`
    that its query reads (None: every task full).
    "paged" - favor_keys_paged's state (csrc/favor_paged.h): the "long" layout for up to 4096 slots, the query
    walking pages of 256 slots; row-invariant, reads out weights and takes masks like "long".
    `lens`: None, or the per-task context sizes (a tuple of T ints) of a masked state (mlhot_favor_keys_ragged_fwd): rows
    n >= lens[t] of F_k are exact zeros.  A summary state always carries `lens`, the shots each task has absorbed so far, and its
    dims[1] is the largest of them."""

    def __init__(self, route, dims, buf=None, kh=None, lens=None, lens_dev=None):
        self.route, self.dims, self.buf, self.kh, self.lens = route, dims, buf, kh, lens      # dims = (T, Nc, H, d, m)
        self.lens_dev = lens_dev

    def features(self):
        """(F_k [T, H, Nc, mp], M [1]) of a "cached", a "long" or a "paged" state, as views."""
        if self.route not in PER_SHOT_ROUTES:
            raise MlhotError(f"FavorKeyState.features: this state holds no key features (route {self.route!r})")
        T, Nc, H, d, m = self.dims
        return lib().favor_state_views(self.buf, T, H, Nc, m)

    def summary(self):
        """(A [T, H, mp, d], a [T, H, mp], vs [T, H, d], cnt [T, H] int32, M [1]) of a "summary" state, as views."""
        if self.route != "summary":
            raise MlhotError(f"FavorKeyState.summary: this state is no summary (route {self.route!r})")
        T, _, H, d, m = self.dims
        return lib().favor_summary_views(self.buf, T, H, d, m)


def host_lens(lens, T, lo, hi, what, exc=MlhotError):
    """A host int sequence or CPU integer tensor of T values in lo .. hi -> a tuple of ints, or `exc` naming what is wrong.  Host
    work only: the callers refuse before anything touches the GPU."""
    if isinstance(lens, torch.Tensor):
        if lens.is_cuda:
            raise exc(f"{what} must be a host int sequence or a CPU integer tensor (its values are checked on the host), got a tensor on {lens.device}")
        if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
            raise exc(f"{what} must hold integers, got a {lens.dtype} tensor")
        if lens.dim() != 1:
            raise exc(f"{what} must be one-dimensional with one entry per task, got shape {tuple(lens.shape)}")
        lens = lens.tolist()
    try:
        lens = list(lens)
    except TypeError:
        raise exc(f"{what} must be a sequence with one entry per task, got {type(lens).__name__}") from None
    if len(lens) != T:
        raise exc(f"{what} has {len(lens)} entries for {T} tasks")
    vals = []
    for x in lens:
        if isinstance(x, bool) or not isinstance(x, numbers.Integral):
            raise exc(f"{what} must hold integers, got {x!r}")
        vals.append(int(x))
    if min(vals) < lo or max(vals) > hi:
        raise exc(f"{what} must lie in {lo}..{hi}, got {vals}")
    return tuple(vals)


def favor_keys(kh, proj, lens=None, lens_dev=None):
    """The context side of FAVOR+ once: k [T, Nc, H, d] (the head projections' layout), proj [m, d] -> FavorKeyState for any
    number of favor_query calls on the SAME T tasks (the key stabiliser is the maximum over the whole batch of kh).  Two launches
    (csrc/favor_cached.h) for Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536; other shapes keep kh.  Forward only.

    `lens` (a host int sequence or CPU integer tensor of T values in 1..Nc; checked on the host, then uploaded): row n of task t is
    a context shot iff n < lens[t].  The stabiliser is the maximum over the valid rows only, the invalid rows of F_k are exact zeros
    and their kh is never read (mlhot_favor_keys_ragged_fwd).  The state is "cached" and carries `lens`; outside the cached
    envelope this raises MlhotError - mlhot_favor_fwd has no mask, so there is no "plain" route here.  `lens_dev`: the caller's own
    int32 copy of `lens` on kh's device, for a caller that uploaded it earlier (mlhot.ragged.Plan); `lens` is still what is checked."""
    _forward_only("favor_keys", kh, proj)
    _need_gpu(kh, proj)
    kh, proj = _c(kh.detach()), _c(proj.detach())
    T, Nc, H, d = kh.shape
    dims = (T, Nc, H, d, proj.shape[0])
    if lens is not None:
        lens = host_lens(lens, T, 1, Nc, "favor_keys: lens")
        if not lib().favor_keys_bytes(T, H, Nc, d, proj.shape[0]):
            bad = [f"{n}={v}" for n, v, ok in (("Nc", Nc, Nc <= 32), ("d", d, d % 16 == 0 and 16 <= d <= 256),
                                                ("m", proj.shape[0], 16 <= proj.shape[0] <= 1536)) if not ok] or [f"T*H={T * H}"]
            raise MlhotError(f"favor_keys: lens needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536), "
                             f"got {', '.join(bad)}; mlhot_favor_fwd has no mask")
        dev = torch.tensor(lens, dtype=torch.int32).to(kh.device) if lens_dev is None else _c(lens_dev)
        return FavorKeyState("cached", dims, buf=lib().favor_keys_ragged_fwd(kh, proj, dev), lens=lens)
    if lib().favor_keys_bytes(T, H, Nc, d, proj.shape[0]):
        return FavorKeyState("cached", dims, buf=lib().favor_keys_fwd(kh, proj))
    return FavorKeyState("plain", dims, kh=kh)


MAX_LONG_NC = 256          # context slots per task of the long per-shot state (csrc/favor_long.h)


def favor_keys_long(kh, proj, lens=None, lens_dev=None):
    """favor_keys for up to 256 context slots: k [T, Nc, H, d], proj [m, d] -> FavorKeyState of route "long", the
    per-shot key features of every slot in favor_keys' layout (features() shows them), built 32 rows at a time in two launches
    (csrc/favor_long.h).  favor_query walks the slots in chunks of 32 in ONE row-invariant launch and, unlike a summary state, can
    read out the weights (weights=True).  `lens` / `lens_dev` as favor_keys takes them: row n of task t is a context shot iff
    n < lens[t]; the other rows of kh are never read and are exact zeros in F_k.  The same shots give the same bits at any
    capacity Nc, and with Nc <= 32 the state and favor_query's results have the bits of favor_keys' "cached" route.
    Nc <= 256, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, else MlhotError - there is no other route.  Forward only."""
    _forward_only("favor_keys_long", kh, proj)
    _need_gpu(kh, proj)
    kh, proj = _c(kh.detach()), _c(proj.detach())
    if kh.dim() != 4 or proj.dim() != 2 or proj.shape[1] != kh.shape[3]:
        raise MlhotError(f"favor_keys_long: k must be [T, Nc, H, d] and proj [m, d], got {tuple(kh.shape)}, {tuple(proj.shape)}")
    T, Nc, H, d = kh.shape
    m = proj.shape[0]
    if lens is not None:
        lens = host_lens(lens, T, 1, Nc, "favor_keys_long: lens")
    if not lib().favor_long_supported(T, H, Nc, d, m):
        bad = [f"{n}={v}" for n, v, ok in (("Nc", Nc, 1 <= Nc <= MAX_LONG_NC), ("d", d, d % 16 == 0 and 16 <= d <= 256),
                                            ("m", m, 16 <= m <= 1536)) if not ok] or [f"T*H={T * H}"]
        raise MlhotError(f"favor_keys_long serves Nc <= {MAX_LONG_NC}, d % 16 == 0, d <= 256, 16 <= m <= 1536, got {', '.join(bad)}")
    dev = None
    if lens is not None:
        dev = torch.tensor(lens, dtype=torch.int32).to(kh.device) if lens_dev is None else _c(lens_dev)
    return FavorKeyState("long", (T, Nc, H, d, m), buf=lib().favor_keys_long_fwd(kh, proj, dev), lens=lens, lens_dev=dev)


MAX_PAGED_NC = 4096        # context slots per task of the paged per-shot state (csrc/favor_paged.h: FAVOR_PAGED_MAXNC)


def favor_keys_paged(kh, proj, lens=None, lens_dev=None):
    """favor_keys_long beyond 256 context slots: k [T, Nc, H, d], proj [m, d] -> FavorKeyState of route "paged",
    the per-shot key features of every slot in favor_keys' layout (features() shows them) from favor_keys_long's own two launches.
    favor_query walks the slots in pages of 256 in ONE row-invariant launch, D and the chains of out carried from page to page, and
    serves weights=True and mask= like a "long" state.  `lens` / `lens_dev` as favor_keys_long takes them.  The same shots give the
    same bits at any capacity Nc, and with Nc <= 256 the state and favor_query's results have the bits of the "long" route.
    Nc <= 4096, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, else MlhotError - there is no other route.  Forward only."""
    _forward_only("favor_keys_paged", kh, proj)
    _need_gpu(kh, proj)
    kh, proj = _c(kh.detach()), _c(proj.detach())
    if kh.dim() != 4 or proj.dim() != 2 or proj.shape[1] != kh.shape[3]:
        raise MlhotError(f"favor_keys_paged: k must be [T, Nc, H, d] and proj [m, d], got {tuple(kh.shape)}, {tuple(proj.shape)}")
    T, Nc, H, d = kh.shape
    m = proj.shape[0]
    if lens is not None:
        lens = host_lens(lens, T, 1, Nc, "favor_keys_paged: lens")
    if not lib().favor_paged_supported(T, H, Nc, d, m):
        bad = [f"{n}={v}" for n, v, ok in (("Nc", Nc, 1 <= Nc <= MAX_PAGED_NC), ("d", d, d % 16 == 0 and 16 <= d <= 256),
                                            ("m", m, 16 <= m <= 1536)) if not ok] or [f"T*H={T * H}, T*Nc={T * Nc}"]
        raise MlhotError(f"favor_keys_paged serves Nc <= {MAX_PAGED_NC}, d % 16 == 0, d <= 256, 16 <= m <= 1536, got {', '.join(bad)}")
    dev = None
    if lens is not None:
        dev = torch.tensor(lens, dtype=torch.int32).to(kh.device) if lens_dev is None else _c(lens_dev)
    return FavorKeyState("paged", (T, Nc, H, d, m), buf=lib().favor_keys_paged_fwd(kh, proj, dev), lens=lens, lens_dev=dev)


ABSORB_CHUNK = 32          # new shots per task and mlhot_favor_summary_absorb call


def favor_absorb(state, kh, vh, proj, lens=None):
    """More context shots into a fixed-size FAVOR+ summary: k, v [T, n, H, d] (any n >= 1), proj [m, d] -> a NEW FavorKeyState of
    route "summary"; `state` (None: a fresh one) stays valid.  The state's size does not depend on the shots it holds and nothing
    absorbed earlier is read again (csrc/favor_summary.h); the key stabiliser follows the maximum over all valid shots of all T tasks
    seen so far.  `lens` (a host int sequence or CPU integer tensor of T values in 0..n): task t's new shots are its first lens[t]
    rows, the others are never read.  Longer inputs go in calls of 32 shots.  d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, else
    MlhotError.  Forward only."""
    _forward_only("favor_absorb", kh, vh, proj)
    _need_gpu(kh, vh, proj)
    kh, vh, proj = _c(kh.detach()), _c(vh.detach()), _c(proj.detach())
    if kh.dim() != 4 or vh.shape != kh.shape or kh.shape[1] < 1 or proj.dim() != 2 or proj.shape[1] != kh.shape[3]:
        raise MlhotError(f"favor_absorb: k and v must be [T, n >= 1, H, d] and proj [m, d], got {tuple(kh.shape)}, {tuple(vh.shape)}, {tuple(proj.shape)}")
    T, n, H, d = kh.shape
    m = proj.shape[0]
    if state is not None and (not isinstance(state, FavorKeyState) or state.route != "summary"):
        raise MlhotError("favor_absorb: state must be None or a summary state (favor_keys' states hold per-shot rows: they do not absorb)")
    if state is not None and (state.dims[0], *state.dims[2:]) != (T, H, d, m):
        raise MlhotError(f"favor_absorb: the state was built for T={state.dims[0]} H={state.dims[2]} d={state.dims[3]} m={state.dims[4]}; "
                         f"got k {tuple(kh.shape)}, proj {tuple(proj.shape)}")
    add = (n,) * T if lens is None else host_lens(lens, T, 0, n, "favor_absorb: lens")
    if not lib().favor_summary_bytes(T, H, d, m):
        raise MlhotError(f"favor_absorb serves d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, got d={d} m={m}")
    starts = range(0, n, ABSORB_CHUNK)
    dev = None            # one upload for every chunk's lens, before the first launch
    if lens is not None:
        dev = torch.tensor([[min(max(a - s, 0), ABSORB_CHUNK) for a in add] for s in starts], dtype=torch.int32).to(kh.device)
    buf = lib().favor_summary_init(T, H, d, m, kh.device) if state is None else state.buf
    for i, s in enumerate(starts):
        if lens is not None and max(add) <= s:
            break                                      # nothing valid from here on
        e = min(s + ABSORB_CHUNK, n)
        fresh = i > 0 or state is None                 # a buffer of this call's own is updated in place; the caller's state is not
        buf = lib().favor_summary_absorb(_c(kh[:, s:e]), _c(vh[:, s:e]), proj, buf, lens=None if dev is None else dev[i], out=buf if fresh else None)
    if state is not None and buf is state.buf:                 # no valid shot at all: still a state of its own
        buf = buf.clone()
    total = tuple(a + b for a, b in zip(add, state.lens if state is not None else (0,) * T))
    return FavorKeyState("summary", (T, max(total), H, d, m), buf=buf, lens=total)


def favor_retract(state, kh, vh, proj, lens=None):
    """Context shots out of a FAVOR+ summary again: `state` a summary state, k, v [T, n, H, d] (any n >= 1) the head
    rows of shots that were absorbed into it earlier, proj [m, d] -> a NEW FavorKeyState of route "summary"; `state` stays valid.
    `lens` (a host int sequence or CPU integer tensor of T values in 0..n): task t gives up its first lens[t] rows, the others are
    never read; every task must keep at least one shot.  The stabiliser M stays the state's: in exact arithmetic the result is the
    state absorbed from the remaining shots at the M of the larger set (the caveat of favor_merge and favor_gather), in fp32 the
    subtraction rounds at the scale of the state before the retraction.  A shot that was never absorbed gives values that are
    undefined but finite.  Longer inputs go in calls of 32 shots (mlhot_favor_summary_retract).  Forward only."""
    _forward_only("favor_retract", kh, vh, proj)
    _need_gpu(kh, vh, proj)
    kh, vh, proj = _c(kh.detach()), _c(vh.detach()), _c(proj.detach())
    if kh.dim() != 4 or vh.shape != kh.shape or kh.shape[1] < 1 or proj.dim() != 2 or proj.shape[1] != kh.shape[3]:
        raise MlhotError(f"favor_retract: k and v must be [T, n >= 1, H, d] and proj [m, d], got {tuple(kh.shape)}, {tuple(vh.shape)}, {tuple(proj.shape)}")
    T, n, H, d = kh.shape
    m = proj.shape[0]
    if not isinstance(state, FavorKeyState) or state.route != "summary":
        raise MlhotError("favor_retract: state must be a summary state (favor_absorb's; a per-shot state lets shots go by compacting its rows)")
    if (state.dims[0], *state.dims[2:]) != (T, H, d, m):
        raise MlhotError(f"favor_retract: the state was built for T={state.dims[0]} H={state.dims[2]} d={state.dims[3]} m={state.dims[4]}; "
                         f"got k {tuple(kh.shape)}, proj {tuple(proj.shape)}")
    sub = (n,) * T if lens is None else host_lens(lens, T, 0, n, "favor_retract: lens")
    short = [(t, s, l) for t, (s, l) in enumerate(zip(sub, state.lens)) if s >= l]
    if short:
        t, s, l = short[0]
        raise MlhotError(f"favor_retract: task {t} holds {l} shots and would give up {s}; a task keeps at least one (its attention is 0 / 0 otherwise)")
    starts = range(0, n, ABSORB_CHUNK)
    dev = None            # one upload for every chunk's lens, before the first launch
    if lens is not None:
        dev = torch.tensor([[min(max(a - s, 0), ABSORB_CHUNK) for a in sub] for s in starts], dtype=torch.int32).to(kh.device)
    buf = None
    for i, s in enumerate(starts):
        if lens is not None and max(sub) <= s:
            break                                      # nothing valid from here on
        e = min(s + ABSORB_CHUNK, n)
        # the first call writes a buffer of this call's own, the later ones update it in place; the caller's state is only read
        buf = lib().favor_summary_retract(_c(kh[:, s:e]), _c(vh[:, s:e]), proj, state.buf if buf is None else buf,
                                          lens=None if dev is None else dev[i], out=buf)
    if buf is None:                                    # no valid shot at all: still a state of its own
        buf = state.buf.clone()
    total = tuple(l - s for l, s in zip(state.lens, sub))
    return FavorKeyState("summary", (T, max(total), H, d, m), buf=buf, lens=total)


MERGE_GROUP = 8            # states per mlhot_favor_summary_merge call


def favor_merge(states, floor=None):
    """Summary states that were absorbed apart (several sources per task, several streams, a stored library of contexts) -> ONE new
    FavorKeyState of route "summary" holding all their shots; the inputs stay valid and unchanged.  The summary is a sum over
    shots, so with M' = max_i M_i:  A' = sum_i exp(M_i - M') A_i, a' likewise, vs' = sum_i vs_i, cnt' = sum_i cnt_i - in exact
    arithmetic the state favor_absorb builds from all the shots, one stabiliser for the whole (csrc/favor_summary.h, DESIGN.md
    6c-6).  `states`: a non-empty sequence of summary states of the same (T, H, d, m), device and dtype.  More than 8 are folded in
    groups, left to right: the first 8 in one launch, then the result with the next 7, and so on - the order of every sum is a
    function of len(states) alone.  lens add up and dims[1] is their maximum, as favor_absorb sets them.

    `floor`: None, or ONE fp32 value on the states' device - "the stabiliser is at least this": M' = max(M_0, .., floor).  A floor
    at or below every M_i changes nothing; a higher one scales A and a by one common factor exp(max_i M_i - floor).  favor_query's
    quotient cancels that factor up to its eps terms: the key feature's +eps is relative to the stabiliser, so the result is the one
    of a batch whose stabiliser IS the floor - what a caller needs who must agree on one stabiliser with states it does not hold.
    Forward only."""
    try:
        states = list(states)
    except TypeError:
        raise MlhotError(f"favor_merge: states must be a sequence of summary states, got {type(states).__name__}") from None
    if not states:
        raise MlhotError("favor_merge: needs at least one summary state (got an empty sequence)")
    for i, s in enumerate(states):
        if not isinstance(s, FavorKeyState):
            raise MlhotError(f"favor_merge: states[{i}] is a {type(s).__name__}, not a FavorKeyState of favor_absorb")
        if s.route != "summary":
            why = ("favor_keys' per-shot states hold rows, not sums: they do not merge (build the parts with favor_absorb)" if s.route == "cached"
                   else "only favor_absorb's summary states are sums over shots")
            raise MlhotError(f"favor_merge: states[{i}] has route {s.route!r}; {why}")
    T, _, H, d, m = states[0].dims
    for i, s in enumerate(states[1:], 1):
        if (s.dims[0], *s.dims[2:]) != (T, H, d, m):
            raise MlhotError(f"favor_merge: states[{i}] was built for T={s.dims[0]} H={s.dims[2]} d={s.dims[3]} m={s.dims[4]}, "
                             f"states[0] for T={T} H={H} d={d} m={m}")
        if s.buf.device != states[0].buf.device or s.buf.dtype != states[0].buf.dtype:
            raise MlhotError(f"favor_merge: states[{i}] lies on {s.buf.device} as {s.buf.dtype}, states[0] on {states[0].buf.device} as {states[0].buf.dtype}")
    if floor is not None and (not isinstance(floor, torch.Tensor) or floor.dtype != torch.float32 or floor.numel() != 1 or floor.device != states[0].buf.device):
        raise MlhotError(f"favor_merge: floor must be None or one fp32 value on {states[0].buf.device} (the stabiliser is at least this)")
    bufs = [s.buf for s in states]
    buf = lib().favor_summary_merge(bufs[:MERGE_GROUP], T, H, d, m, floor=floor)
    for at in range(MERGE_GROUP, len(bufs), MERGE_GROUP - 1):
        buf = lib().favor_summary_merge([buf] + bufs[at:at + MERGE_GROUP - 1], T, H, d, m, floor=floor)
    total = tuple(sum(s.lens[t] for s in states) for t in range(T))
    return FavorKeyState("summary", (T, max(total), H, d, m), buf=buf, lens=total)


GATHER_PARTS = 8           # parts per output task of favor_gather


def _gather_parts(parts, states):
    """favor_gather's table on the host: parts[t] = a sequence of (state_index, task_index) pairs -> a list of lists of int pairs,
    every index in range, at most 8 pairs per task; ValueError names what is wrong."""
    try:
        rows = [list(row) for row in parts]
    except TypeError:
        raise ValueError("favor_gather: parts must be a sequence with one sequence of (state_index, task_index) pairs per output task") from None
    if not rows:
        raise ValueError("favor_gather: parts is empty - the gathered state needs at least one task")
    table = []
    for t, row in enumerate(rows):
        if len(row) > GATHER_PARTS:
            raise ValueError(f"favor_gather: parts[{t}] names {len(row)} parts; a task takes at most {GATHER_PARTS}")
        pairs = []
        for p, pair in enumerate(row):
            try:
                i, u = pair
            except (TypeError, ValueError):
                raise ValueError(f"favor_gather: parts[{t}][{p}] must be a (state_index, task_index) pair, got {pair!r}") from None
            if any(isinstance(x, bool) or not isinstance(x, numbers.Integral) for x in (i, u)):
                raise ValueError(f"favor_gather: parts[{t}][{p}] must hold two integers, got {pair!r}")
            if not 0 <= i < len(states):
                raise ValueError(f"favor_gather: parts[{t}][{p}] names state {i}; there are {len(states)} states (0 .. {len(states) - 1})")
            if not 0 <= u < states[i].dims[0]:
                raise ValueError(f"favor_gather: parts[{t}][{p}] names task {u} of states[{i}], which holds {states[i].dims[0]} tasks "
                                 f"(0 .. {states[i].dims[0] - 1})")
            pairs.append((int(i), int(u)))
        table.append(pairs)
    return table


def favor_gather(states, parts, floor=None):
    """Pick and combine TASKS across summary states: output task t = the sum of the parts parts[t] = [(state_index,
    task_index), ..] - merge with a row per task -> ONE new FavorKeyState of route "summary" with len(parts) tasks; the inputs stay
    valid and unchanged.  Any task of any state can move into any slot, the same task may stand in several slots, tasks can be
    dropped, and the states may hold different numbers of tasks.  With M' = the maximum of the stabilisers of the states that a
    part names (and of `floor`): A'[t] = sum_p exp(M_i - M') A_i[u] over parts[t], a' likewise, vs' and cnt' plain sums, one chain
    per element in the order of parts[t] (csrc/favor_summary.h) - in exact arithmetic the state favor_absorb builds from the chosen
    shots in a batch whose stabiliser is M'.  A task without a part gets the rows of a fresh state (favor_query refuses it).

    `states`: a non-empty sequence of summary states of the same (H, d, m), device and dtype; `parts`: a host sequence, at most 8
    pairs per task, every index in range - else ValueError, before any launch.  States that no part names are dropped before the
    call: they do not enter M'.  More than 8 named states are folded in groups like favor_merge's: the first 8 in one launch, then
    the running result (as the first part of every task that has one) with the next 7, and so on - the order of every sum is a
    function of the arguments alone.  lens[t] is the sum of the parts' lens, dims carries len(parts) and max(lens).  `floor` as in
    favor_merge.  Forward only."""
    try:
        states = list(states)
    except TypeError:
        raise ValueError(f"favor_gather: states must be a sequence of summary states, got {type(states).__name__}") from None
    if not states:
        raise ValueError("favor_gather: needs at least one summary state (got an empty sequence)")
    for i, s in enumerate(states):
        if not isinstance(s, FavorKeyState):
            raise ValueError(f"favor_gather: states[{i}] is a {type(s).__name__}, not a FavorKeyState of favor_absorb")
        if s.route != "summary":
            why = ("favor_keys' per-shot states hold rows, not sums: their tasks do not combine (build the parts with favor_absorb)"
                   if s.route in PER_SHOT_ROUTES else "only favor_absorb's summary states are sums over shots")
            raise ValueError(f"favor_gather: states[{i}] has route {s.route!r}; {why}")
    _, _, H, d, m = states[0].dims
    for i, s in enumerate(states[1:], 1):
        if tuple(s.dims[2:]) != (H, d, m):
            raise ValueError(f"favor_gather: states[{i}] was built for H={s.dims[2]} d={s.dims[3]} m={s.dims[4]}, states[0] for H={H} d={d} m={m}")
        if s.buf.device != states[0].buf.device or s.buf.dtype != states[0].buf.dtype:
            raise ValueError(f"favor_gather: states[{i}] lies on {s.buf.device} as {s.buf.dtype}, states[0] on {states[0].buf.device} as {states[0].buf.dtype}")
    dev = states[0].buf.device
    if floor is not None and (not isinstance(floor, torch.Tensor) or floor.dtype != torch.float32 or floor.numel() != 1 or floor.device != dev):
        raise ValueError(f"favor_gather: floor must be None or one fp32 value on {dev} (the stabiliser is at least this)")
    table = _gather_parts(parts, states)
    T_out = len(table)
    named = sorted({i for row in table for i, _ in row})
    if not named:                                       # no part at all: the fresh state, through the same launch (floor included)
        fresh = lib().favor_summary_init(1, H, d, m, dev)
        buf = lib().favor_summary_gather([fresh], [1], torch.full((T_out, 1, 2), -1, dtype=torch.int32).to(dev), H, d, m, floor=floor)
        return FavorKeyState("summary", (T_out, 0, H, d, m), buf=buf, lens=(0,) * T_out)
    # one launch per group of named states: 8 first, then the running result and the next 7
    groups = [named[:MERGE_GROUP]] + [named[at:at + MERGE_GROUP - 1] for at in range(MERGE_GROUP, len(named), MERGE_GROUP - 1)]
    buf, seen = None, [False] * T_out                   # seen[t]: the running result holds a part of task t
    for g, group in enumerate(groups):
        slot = {i: k + (g > 0) for k, i in enumerate(group)}
        rows = [([(0, t)] if g > 0 and seen[t] else []) + [(slot[i], u) for i, u in row if i in slot] for t, row in enumerate(table)]
        P = max(1, max(len(r) for r in rows))
        dev_rows = torch.tensor([r + [(-1, 0)] * (P - len(r)) for r in rows], dtype=torch.int32).to(dev)
        bufs, tasks = [states[i].buf for i in group], [states[i].dims[0] for i in group]
        if g > 0:
            bufs, tasks = [buf] + bufs, [T_out] + tasks
        buf = lib().favor_summary_gather(bufs, tasks, dev_rows, H, d, m, floor=floor)
        seen = [s or any(i in slot for i, _ in row) for s, row in zip(seen, table)]
    total = tuple(sum(states[i].lens[u] for i, u in row) for row in table)
    return FavorKeyState("summary", (T_out, max(total), H, d, m), buf=buf, lens=total)


def linear_rows_any(sources, weight, bias, act="none"):
    """linear_rows for sources [(x [R, k], 1, 0), ..] whose LAST width need not be a multiple of 4 (the kernel's k granule): that
    source and the weight's trailing columns are padded with zero columns, which add exact zeros to every chain.  The per-shot
    stage of condition(form="paged") runs its Linears through this: the bits of a shot's rows then do not depend
    on how many shots share the call, so extend equals conditioning on all shots to the bit.  A shape linear_rows still does not
    serve raises MlhotError - there is no other row-invariant route.  Forward only."""
    srcs = [tuple(s) for s in sources]
    pad = -srcs[-1][0].shape[1] % 4
    if pad:
        srcs[-1] = (torch.nn.functional.pad(srcs[-1][0], (0, pad)),) + srcs[-1][1:]
        weight = torch.nn.functional.pad(weight.detach(), (0, pad))
    k0, k1 = srcs[0][0].shape[1], srcs[1][0].shape[1] if len(srcs) > 1 else 0
    if not lib().linear_rows_supported(k0, k1, weight.shape[0]):
        raise MlhotError(f"linear_rows_any: no row-invariant kernel for a Linear [{k0} | {k1}] -> {weight.shape[0]}")
    return linear_rows(srcs, weight, bias, act)


def _mask_words(mask, T, Nq, Nc, device):
    """favor_query's `mask`: a bool tensor [T, Nq, Nc] / [T, G, Nq, Nc] or packed words [T, G, Nq, ceil(Nc / 32)] (int32 or uint32)
    -> int32 words on `device`."""
    from mlhot.ragged import pack_mask                   # ragged imports this module
    W = (Nc + 31) // 32
    if not isinstance(mask, torch.Tensor):
        raise MlhotError(f"favor_query: mask must be a bool tensor or packed int32 words, got {type(mask).__name__}")
    if mask.dtype == torch.bool:
        if mask.dim() not in (3, 4) or (mask.shape[0], mask.shape[-2], mask.shape[-1]) != (T, Nq, Nc):
            raise MlhotError(f"favor_query: a bool mask must be [T={T}, Nq={Nq}, Nc={Nc}] or [T, G, Nq, Nc], got {tuple(mask.shape)}")
        return pack_mask(mask.to(device), Nc)
    if mask.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise MlhotError(f"favor_query: mask must be bool or packed int32 / uint32 words, got {mask.dtype}")
    if mask.dim() != 4 or mask.shape[1] < 1 or (mask.shape[0], mask.shape[2], mask.shape[3]) != (T, Nq, W):
        raise MlhotError(f"favor_query: packed mask words must be [T={T}, G, Nq={Nq}, {W}], got {tuple(mask.shape)}")
    return _c(mask.view(torch.int32).to(device))


def target_weight_arg(what, tw, T, Nq, device, exc=MlhotError):
    """`target_weight` of the attention mass: None, or a real tensor [T, Nq], finite and >= 0 -> fp32 on `device`.
    The values are checked where the tensor lies (a device tensor costs ONE reduced bool read back), before any launch."""
    if tw is None:
        return None
    if not isinstance(tw, torch.Tensor) or not tw.is_floating_point():
        got = str(tw.dtype) if isinstance(tw, torch.Tensor) else type(tw).__name__
        raise exc(f"{what}: target_weight must be a floating-point tensor [T={T}, Nq={Nq}], got {got}")
    if tuple(tw.shape) != (T, Nq):
        raise exc(f"{what}: target_weight must be [T={T}, Nq={Nq}], one weight per target, got {tuple(tw.shape)}")
    tw = tw.detach()
    if not bool((torch.isfinite(tw) & (tw >= 0)).all()):
        raise exc(f"{what}: target_weight must be finite and >= 0 (the mass is a sum of non-negative terms)")
    return _c(tw.to(device=device, dtype=torch.float32))


def topk_arg(what, k, name="top_k", exc=ValueError):
    """`top_k` of the top-k attention read-out: an integer in 1 .. 16 (a bool is none) -> int.  Host check."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= TOPK_MAX:
        raise exc(f"{what}: {name} must be an integer in 1 .. {TOPK_MAX} (the kernels keep at most {TOPK_MAX} slots per row), got {k!r}")
    return int(k)


SHARED_ROUTES = ("cached", "long")                 # the states the shared-target query serves (csrc/favor_shared.h)


def _favor_query_shared(qh, state, vh, proj, weights, mask, mass, target_weight, topk, task_group):
    """favor_query(shared=True): the refusals, all on the host, then mlhot_favor_query_shared_fwd / _long_shared_fwd."""
    for on, name in ((mask is not None, "mask="), (bool(mass), "mass="), (target_weight is not None, "target_weight="), (topk is not None, "topk=")):
        if on:
            raise MlhotError(f"favor_query: shared=True with {name} - the shared-target launch forms the plain read-out alone (out, and w "
                             "with weights=True); expand the query rows to [T, Nq, H, d] and call without shared=True")
    if not isinstance(state, FavorKeyState):
        raise MlhotError("favor_query: state must come from favor_keys")
    if state.route not in SHARED_ROUTES:
        why = {"plain": "its keys lie outside the cached kernels' envelope and mlhot_favor_fwd takes one query set per task",
               "summary": "it keeps sums over shots, and mlhot_favor_summary_query_fwd takes one query set per task",
               "paged": "its query walks pages of 256 slots (csrc/favor_paged.h), for which no shared-target kernel is built"}.get(state.route, "")
        raise MlhotError(f"favor_query: shared=True serves \"cached\" and \"long\" states; this state's route is {state.route!r} - {why}")
    if isinstance(task_group, bool) or not isinstance(task_group, numbers.Integral) or task_group < 0:
        raise MlhotError(f"favor_query: task_group must be an integer >= 0 (0: the library picks), got {task_group!r}")
    _forward_only("favor_query", qh, vh, proj)
    _need_gpu(qh, vh, proj)
    qh, vh, proj = _c(qh.detach()), _c(vh.detach()), _c(proj.detach())
    T, Nc, H, d, m = state.dims
    if tuple(vh.shape) != (T, Nc, H, d) or qh.dim() != 3 or tuple(qh.shape[1:]) != (H, d) or tuple(proj.shape) != (m, d):
        raise MlhotError(f"favor_query: shared=True takes q [Nq, H={H}, d={d}] without a task axis against the state built for T={T} Nc={Nc} "
                         f"m={m}; got q {tuple(qh.shape)}, v {tuple(vh.shape)}, proj {tuple(proj.shape)}")
    return lib().favor_query_shared_fwd(qh, state.buf, vh, proj, state.route, lens=state.lens_dev if state.route == "long" else None,
                                        weights=bool(weights), task_group=int(task_group))


def favor_query(qh, state, vh, proj, weights=False, mask=None, mass=False, target_weight=None, topk=None, shared=False, task_group=0):
    """FAVOR+ attention of q [T, Nq, H, d] against a favor_keys state and v [T, Nc, H, d] -> merged [T, Nq, d*H], any Nq >= 1 in
    one launch.  On the "cached" route the bits of a row do not depend on the other rows of the call (csrc/favor_cached.h), nor on
    the "long" route (favor_keys_long, csrc/favor_long.h: up to 256 slots in chunks of 32, weights=True included); the
    "plain" route is mlhot_favor_fwd on the kept keys.  Forward only.  Against a masked state (favor_keys with lens) the rows of v
    behind lens[t] must be finite - zero-fill them: their column of S is exactly 0, and 0 x NaN is not.  A "summary" state
    (favor_absorb) holds what it needs of v: `vh` may be None and is ignored; the call is row-invariant there too
    (csrc/favor_summary.h) and refuses on the host if a task of the state has absorbed no shot.

    `weights=True` -> (merged, w): w [T, H, Nq, Nc] = S / D of the same launch (mlhot_favor_query_weights_fwd),
    FAVOR+'s implied attention per head, query row and context slot - non-negative, rows summing to 1, exact zeros behind a masked
    state's lens[t], row-invariant like merged; merged has the bits of the call without it.  "cached" and "long" states only: a
    "plain" or a "summary" state raises MlhotError.  Without it the call launches what it always did.

    `mask`: per-target context masks, bool [T, Nq, Nc] / [T, G, Nq, Nc] (True = the target sees the slot) or the
    packed words of mlhot.ragged.pack_mask -> merged [T, G, Nq, d*H] (and w [T, G, H, Nq, Nc]): G masked read-outs of ONE query
    pass (mlhot_favor_query_masked_fwd / _long_masked_fwd) - the masked sums are sums of the kept columns, the stabiliser stays the
    state's, rows and groups are independent bit for bit, all-ones reproduces the unmasked call's bits, and a row that keeps no
    valid slot comes back as exact zeros (callers that cannot have that check first, as predict does).  "cached" and "long"
    states only.  Without `mask` the call is the one it always was.

    A "paged" state (favor_keys_paged, csrc/favor_paged.h, DESIGN.md 6c-11: up to 4096 slots in pages of 256) is served like a
    "long" one throughout - row-invariant, `weights=True` and `mask=` included (mlhot_favor_query_paged_fwd / _paged_masked_fwd).

    `mass=True` -> (merged, mass): mass [T, H, Nc] = sum over the targets n of target_weight[t, n] * w[t, h, n, :]
    (`target_weight` [T, Nq] finite and >= 0, or None: the plain column sum), reduced INSIDE the query launch in a fixed order -
    16-row tiles in ascending row order, then the tiles in ascending order - so w [T, H, Nq, Nc] is never stored: the call holds
    1/16 of it.  With target_weight None the result is bit-equal to that fold of `weights=True`'s w; merged has the plain call's
    bits.  "cached", "long" and "paged" states, refused where `weights=True` is; exclusive with `weights=True` and `mask=`.
    `mass="tiles"` -> (merged, part [T, H, ceil(Nq / 16), Nc]): the tile partials, unfolded, for a caller that splits the targets at
    multiples of 16 and folds once (mlhot.lib().favor_mass_fold).

    `topk=k`, 1 <= k <= 16 -> (merged, idx int32 [T, H, Nq, k], wk fp32 [T, H, Nq, k]): per head and query row the k
    valid slots with the largest un-normalised score S, descending, ties to the lower slot, and their weights wk = S / D - the bits
    `weights=True` stores into w[t, h, n, idx] - selected INSIDE the query launch (mlhot_favor_query_topk_fwd / _long_topk_fwd /
    _paged_topk_fwd), the paged form in its ONE walk over the pages; w is never stored.  Entries behind the task's valid slots are
    idx = -1, wk = +0.  merged has the plain call's bits; every row's result is its own.  "cached", "long" and "paged" states,
    refused where `weights=True` is; exclusive with `weights=True`, `mask=` and `mass=`.

    `shared=True`: q is [Nq, H, d] WITHOUT a task axis - one frame, or one set of probe rows, asked of all T stored
    contexts of the state -> merged [T, Nq, d*H] (and w [T, H, Nq, Nc] with weights=True) in ONE launch
    (mlhot_favor_query_shared_fwd / _long_shared_fwd): the query features are formed once per (head, 16 rows) instead of once per
    task, then the per-task kernel's own steps run against every task of the workgroup's group.  The bits are those of the call
    on `q.expand(T, ...)`.  `task_group`: tasks per workgroup (0: the library picks so the grid covers the CUs about once); the
    bits do not depend on it.  "cached" and "long" states only - a "plain", "summary" or "paged" state raises MlhotError naming the
    state's route - and `mask=`, `mass=` and `topk=` do not combine with it.  Without it the call is the one it always was."""
    if shared:
        return _favor_query_shared(qh, state, vh, proj, weights, mask, mass, target_weight, topk, task_group)
    if task_group != 0:
        raise MlhotError("favor_query: task_group= groups the tasks of shared=True; without it every workgroup serves one task")
    if topk is not None:
        topk = topk_arg("favor_query", topk, "topk")
        for on, name, why in ((weights, "weights=True", "the top-k exists so that w [T, H, Nq, Nc] is never stored; ask for one of the two"),
                              (mask is not None, "mask=", "the masked read-outs have no reduced form; ask for weights=True with the mask"),
                              (mass, "mass=", "each is one reduction of the read-out inside the launch; ask for one per call")):
            if on:
                raise ValueError(f"favor_query: topk= with {name} - {why}")
        if isinstance(state, FavorKeyState) and state.route not in PER_SHOT_ROUTES:
            if state.route == "summary":
                raise MlhotError("favor_query: topk= - a summary state keeps no per-shot rows, so there is no weight per context shot to "
                                 "read out (condition with the default form for at most 32 shots)")
            T, Nc, H, d, m = state.dims
            raise MlhotError(f"favor_query: topk= needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536), "
                             f"got Nc={Nc} d={d} m={m}: mlhot_favor_fwd on the kept keys forms no per-shot weights")
    if mass:
        if weights:
            raise ValueError("favor_query: mass=True with weights=True - the mass exists so that w [T, H, Nq, Nc] is never stored; ask for one "
                             "of the two (the mass is the fold of w over the targets)")
        if mask is not None:
            raise ValueError("favor_query: mass=True with mask= - the masked read-outs have no reduced form; ask for weights=True with the mask "
                             "and sum over the targets")
    elif target_weight is not None:
        raise ValueError("favor_query: target_weight= weighs the targets of mass=True; without it there is nothing to weigh")
    if mass and isinstance(state, FavorKeyState) and state.route not in PER_SHOT_ROUTES:
        if state.route == "summary":
            raise MlhotError("favor_query: mass=True - a summary state keeps no per-shot rows, so there is no weight per context shot to "
                             "read out (condition with the default form for at most 32 shots)")
        T, Nc, H, d, m = state.dims
        raise MlhotError(f"favor_query: mass=True needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536), "
                         f"got Nc={Nc} d={d} m={m}: mlhot_favor_fwd on the kept keys forms no per-shot weights")
    if mask is not None and isinstance(state, FavorKeyState) and state.route not in PER_SHOT_ROUTES:
        if state.route == "summary":
            raise MlhotError("favor_query: mask= - a summary state keeps no per-shot rows, so there is no column of S to mask "
                             '(condition with the default form for at most 32 shots, or with form="long")')
        T, Nc, H, d, m = state.dims
        raise MlhotError(f"favor_query: mask= needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536), "
                         f"got Nc={Nc} d={d} m={m}: mlhot_favor_fwd on the kept keys takes no mask")
    if weights and isinstance(state, FavorKeyState) and state.route not in PER_SHOT_ROUTES:
        if state.route == "summary":
            raise MlhotError("favor_query: weights=True - a summary state keeps no per-shot rows, so there is no weight per context shot to "
                             "read out (condition with the default form for at most 32 shots)")
        T, Nc, H, d, m = state.dims
        raise MlhotError(f"favor_query: weights=True needs the cached kernels' envelope (Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536), "
                         f"got Nc={Nc} d={d} m={m}: mlhot_favor_fwd on the kept keys forms no per-shot weights")
    if isinstance(state, FavorKeyState) and state.route == "summary":
        _forward_only("favor_query", qh, proj)
        T, _, H, d, m = state.dims
        if min(state.lens) < 1:
            raise MlhotError(f"favor_query: a task of the summary state has absorbed no shot (shots per task: {list(state.lens)}): "
                             "its attention is 0 / 0")
        _need_gpu(qh, proj)
        qh, proj = _c(qh.detach()), _c(proj.detach())
        if qh.dim() != 4 or (qh.shape[0], qh.shape[2], qh.shape[3]) != (T, H, d) or tuple(proj.shape) != (m, d):
            raise MlhotError(f"favor_query: the state was built for T={T} H={H} d={d} m={m}; got q {tuple(qh.shape)}, proj {tuple(proj.shape)}")
        return lib().favor_summary_query_fwd(qh, state.buf, proj)
    _forward_only("favor_query", qh, vh, proj)
    _need_gpu(qh, vh, proj)
    if not isinstance(state, FavorKeyState):
        raise MlhotError("favor_query: state must come from favor_keys")
    qh, vh, proj = _c(qh.detach()), _c(vh.detach()), _c(proj.detach())
    T, Nc, H, d, m = state.dims
    if tuple(vh.shape) != (T, Nc, H, d) or qh.dim() != 4 or (qh.shape[0], qh.shape[2], qh.shape[3]) != (T, H, d) or tuple(proj.shape) != (m, d):
        raise MlhotError(f"favor_query: the state was built for T={T} Nc={Nc} H={H} d={d} m={m}; got q {tuple(qh.shape)}, v {tuple(vh.shape)}, proj {tuple(proj.shape)}")
    if topk is not None:
        return lib().favor_query_topk_fwd(qh, state.buf, vh, proj, state.route, topk, lens=state.lens_dev)
    if mass:
        tw = target_weight_arg("favor_query", target_weight, T, qh.shape[1], qh.device)
        return lib().favor_query_mass_fwd(qh, state.buf, vh, proj, state.route, lens=state.lens_dev, tw=tw, fold=mass != "tiles")
    if mask is not None:
        words = _mask_words(mask, T, qh.shape[1], Nc, qh.device)
        if state.route == "paged":
            return lib().favor_query_paged_fwd(qh, state.buf, vh, proj, lens=state.lens_dev, weights=weights, mask_words=words)
        if state.route == "long":
            return lib().favor_query_masked_fwd(qh, state.buf, vh, proj, words, lens=state.lens_dev, long=True, weights=weights)
        return lib().favor_query_masked_fwd(qh, state.buf, vh, proj, words, weights=weights)
    if state.route == "cached":
        if weights:
            return lib().favor_query_weights_fwd(qh, state.buf, vh, proj)
        return lib().favor_query_fwd(qh, state.buf, vh, proj)
    if state.route == "long":
        return lib().favor_query_long_fwd(qh, state.buf, vh, proj, lens=state.lens_dev, weights=weights)
    if state.route == "paged":
        return lib().favor_query_paged_fwd(qh, state.buf, vh, proj, lens=state.lens_dev, weights=weights)
    return lib().favor_fwd(qh, state.kh, vh, proj)[0]


def linear_rows(sources, weight, bias, act="none", rows=None):
    """y = act([src_0 | src_1] W^T + b) over the rows of MANY prefixes in one launch, with bits per row that do not depend on the
    number of rows (csrc/linear_rows.h; LinearFunction picks its kernel by row count).  sources: one or two (tensor [R, k], rep,
    period) - output row i reads source row (i // rep) % period, period 0 = no wrap.  Forward only."""
    srcs = [tuple(s) for s in sources]
    _forward_only("linear_rows", *[s[0] for s in srcs], weight, bias)
    _need_gpu(*[s[0] for s in srcs], weight, bias)
    srcs = [(x if x.stride(-1) == 1 else x.contiguous(), rep, period) for x, rep, period in srcs]
    return lib().linear_rows_fwd(srcs, _c(weight.detach()), _c(bias.detach()) if bias is not None else None, act, rows=rows)


def loss_prefixes(kind, mu, gt):
    """LossFunction's value for each of mu[0 .. P-1] against the shared labels, [P], one launch (mlhot_loss_prefix_fwd): element p
    has the bits of LossFunction.apply(kind, mu[p], gt).  Forward only."""
    _forward_only("loss_prefixes", mu, gt)
    _need_gpu(mu, gt)
    return lib().loss_prefix_fwd(kind, _c(mu.float()), _c(gt.float()))


class LossFunction(torch.autograd.Function):
    """LossFunc.calc_loss kinds: mlhot_loss_fwd / _bwd."""

    @staticmethod
    def forward(ctx, kind, mu, gt):
        _need_gpu(mu, gt)
        node = mu.grad_fn
        mu_c, gt = _c(mu.float()), _c(gt.float())
        ctx.kind = kind
        # the producer of mu takes the loss's gradient itself when it says so and mu reaches the loss as it left the producer
        # (not when the caller wants d loss / d mu itself - retain_grad() or a tensor hook on mu - which the placeholder would hide)
        ctx.node = node if (defer_loss_grad and kind != "degree" and mu_c is mu and getattr(node, "takes_loss", False)
                            and not mu.retains_grad and not mu._backward_hooks) else None
        ctx.save_for_backward(mu_c, gt)
        ctx.value = None
        if ctx.node is not None and _loss_aside:          # (node: mu carries a graph, i.e. a backward can follow)
            out = torch.empty((), device=mu_c.device)             # written by the model's backward (loss_value_aside above)
            ctx.value = out.detach()                               # (the same storage without the output's grad_fn: no reference cycle)
            return out
        return lib().loss_fwd(kind, mu_c, gt)

    @staticmethod
    def backward(ctx, dloss):
        mu, gt = ctx.saved_tensors
        dloss = _c(dloss.float())
        if ctx.node is not None and ctx.node.loss is None:
            # VanillaNPFunction.backward runs next (it is this gradient's only consumer node)
            desc = ctx.node.loss = (ctx.kind, gt, dloss) if ctx.value is None else (ctx.kind, gt, dloss, ctx.value)
            torch.autograd.Variable._execution_engine.queue_callback(_check_handed_over(ctx.node, desc))
            return None, _zero_like(mu), None
        if ctx.value is not None:                         # the producer's slot was taken (a second loss on the same mu): the value now
            ctx.value.copy_(lib().loss_fwd(ctx.kind, mu, gt))
        return None, lib().loss_bwd(ctx.kind, mu, gt, dloss), None


class LossPlusFunction(torch.autograd.Function):
    """loss(kind; mu, gt) + alpha * x for a device scalar x - the trainer's `losses = loss + kl * beta` (trainer/model_trainer.py:77-78)
    inside the loss's own launches: mlhot_loss_plus_fwd / _bwd (ABI 7).  Bit-identical to LossFunction followed by ScaledAddFunction
    (same reduction, product and sum rounded separately); in a replayed step it is two dependent launches instead of four, and every
    dependent launch of a graph costs ~4.7 us on this GPU whatever it computes.  Call through loss_plus()."""

    @staticmethod
    def forward(ctx, kind, mu, gt, x, alpha):
        _need_gpu(mu, gt, x)
        mu_c, gt, x = _c(mu.float()), _c(gt.float()), _c(x.float())
        ctx.kind, ctx.alpha = kind, float(alpha)
        ctx.save_for_backward(mu_c, gt)
        return lib().loss_plus_fwd(kind, mu_c, gt, x, ctx.alpha)

    @staticmethod
    def backward(ctx, dtotal):
        mu, gt = ctx.saved_tensors
        dmu, dx = lib().loss_plus_bwd(ctx.kind, mu, gt, _c(dtotal.float()), ctx.alpha, need_dx=ctx.needs_input_grad[3])
        return None, (dmu if ctx.needs_input_grad[1] else None), None, dx, None


def loss_plus(kind, mu, gt, x, alpha):
    """`LossFunction.apply(kind, mu, gt) + x * alpha` the way the reference's trainer writes its objective; one launch per direction
    when x is a one-element fp32 device tensor (a KL term), add_scaled() behind the plain loss otherwise (x = 0: the bare loss)."""
    if torch.is_tensor(x) and x.is_cuda and x.numel() == 1 and x.dtype == torch.float32 and mu.is_cuda and kind != "degree":
        return LossPlusFunction.apply(kind, mu, gt, x.reshape(()), alpha)
    return add_scaled(LossFunction.apply(kind, mu, gt), x, alpha)


class Conv2dFunction(torch.autograd.Function):
    """nn.Conv2d (+ optional fused ReLU): mlhot_conv2d_fwd / _bwd (generic run-time-shaped conv)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, relu):
        _need_gpu(x, w, b)
        x, w = _c(x.float()), _c(w)
        bb = _c(b) if b is not None else None
        y = lib().conv2d_fwd(x, w.detach(), bb.detach() if bb is not None else None, stride, pad, relu)
        ctx.cfg = (stride, pad, relu, b is not None)
        ctx.save_for_backward(x, w.detach(), y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, relu, has_b = ctx.cfg
        dx, dw, db = lib().conv2d_bwd(x, w, y, _c(dy), stride, pad, relu, need_dx=ctx.needs_input_grad[0], has_bias=has_b)
        return dx, dw, db, None, None, None


class AddReluFunction(torch.autograd.Function):
    """Residual join relu(a + b) of a BasicBlock."""

    @staticmethod
    def forward(ctx, a, b):
        _need_gpu(a, b)
        y = lib().add_relu_fwd(_c(a), _c(b))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        g = lib().add_relu_bwd(y, _c(dy))
        return g, g


class MaxPool2Function(torch.autograd.Function):
    """2x2 max-pool (AdaptiveMaxPool2d((2,2)) on a 4x4 map)."""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = _c(x)
        y, amax = lib().pool2_fwd(x)
        ctx.hw = x.shape[2:]
        ctx.save_for_backward(amax)
        return y

    @staticmethod
    def backward(ctx, dy):
        (amax,) = ctx.saved_tensors
        return lib().pool2_bwd(_c(dy), amax, *ctx.hw)


class BBBSampleFunction(torch.autograd.Function):
    """(mu, rho, eps) -> (w = mu + eps*softplus(rho), kl): mlhot_bbb_sample_fwd / _bwd."""

    @staticmethod
    def forward(ctx, mu, rho, eps):
        _need_gpu(mu, rho, eps)
        mu, rho, eps = _c(mu.detach()), _c(rho.detach()), _c(eps)
        w, kl = lib().bbb_sample_fwd(mu, rho, eps)
        ctx.save_for_backward(mu, rho, eps)
        return w, kl

    @staticmethod
    def backward(ctx, dw, dkl):
        mu, rho, eps = ctx.saved_tensors
        if dw is None:
            dw = torch.zeros_like(mu)
        if dkl is None:
            dkl = torch.zeros((), device=mu.device)
        dmu, drho = lib().bbb_sample_bwd(mu, rho, eps, _c(dw), _c(dkl.float()))
        return dmu, drho, None


class BBBSampleMultiFunction(torch.autograd.Function):
    """All weight / bias samples of a Bayes-by-backprop encoder in one launch pair (mlhot_bbb_sample_multi_fwd / _bwd).
    apply(eps_list, mu_0, rho_0, mu_1, rho_1, ...) -> (w_0, w_1, ..., kl); eps_list[i] is the device tensor of draw i.
    With 2k draws for k (mu, rho) pairs, the second k draws make a SECOND independent sample of every tensor in the same launch:
    -> (w_0 .. w_{k-1}, w2_0 .. w2_{k-1}, kl); the KL does not depend on eps and is computed once, and the backward folds both
    samples' gradients into d mu / d rho in one pass (no per-tensor accumulation kernels)."""

    @staticmethod
    def forward(ctx, eps_list, *mu_rho):
        _need_gpu(*mu_rho, *eps_list)
        mus = [_c(t.detach()) for t in mu_rho[0::2]]
        rhos = [_c(t.detach()) for t in mu_rho[1::2]]
        k = len(mus)
        if len(eps_list) not in (k, 2 * k):
            raise MlhotError(f"BBBSampleMultiFunction: {k} tensors need {k} or {2 * k} eps draws, got {len(eps_list)}")
        epss = [_c(e) for e in eps_list]
        ctx.k, ctx.two = k, len(epss) == 2 * k
        ctx.save_for_backward(*mus, *rhos, *epss)
        if ctx.two:
            ws, ws2, kl = lib().bbb_sample_multi_fwd(mus, rhos, epss[:k], epss[k:])
            return (*ws, *ws2, kl)
        ws, kl = lib().bbb_sample_multi_fwd(mus, rhos, epss)
        return (*ws, kl)

    @staticmethod
    def backward(ctx, *grads):
        k = ctx.k
        saved = ctx.saved_tensors
        mus, rhos, epss = saved[:k], saved[k:2 * k], saved[2 * k:]
        dws = [(_c(g) if g is not None else None) for g in grads[:k]]
        dws2 = [(_c(g) if g is not None else None) for g in grads[k:2 * k]] if ctx.two else None
        dkl = grads[-1]
        if dkl is None:
            dkl = torch.zeros((), device=mus[0].device)
        if ctx.two:
            dmus, drhos = lib().bbb_sample_multi_bwd(mus, rhos, epss[:k], dws, _c(dkl.float()), epss[k:], dws2)
        else:
            dmus, drhos = lib().bbb_sample_multi_bwd(mus, rhos, epss, dws, _c(dkl.float()))
        out = [None]
        for a, b in zip(dmus, drhos):
            out += [a, b]
        return tuple(out)


class ResNetTrunkFunction(torch.autograd.Function):
    """Every ResNet-trunk pass of a model step in ONE call per direction (mlhot_trunk_fwd / _bwd; csrc/resnet_trunk.h).
    apply(spec, *tensors): spec = (passes, skip_ks, n_imgs, taps) with passes = [(image tensor index, weight-set index)],
    skip_ks[w] = 1 | 3 the skip convolution of weight set w, n_imgs the number of leading image tensors, taps = None or a list
    that receives, per pass, the nine post-ReLU activations; tensors = the image batches [n, C, H, H], then 26 tensors per weight
    set (w, b of the stem and of (conv1, conv2, skip) of the four blocks).  Returns one output map [n, 64, H/32, H/32] per pass.
    Gradients flow to the weights only (images are leaves of the models)."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        passes, skip_ks, n_imgs, taps = spec
        _need_gpu(*tensors)
        imgs = [_c(t.float()) for t in tensors[:n_imgs]]
        flat_w = [_c(t.detach()) for t in tensors[n_imgs:]]
        wsets = [(flat_w[26 * i:26 * i + 26], skip_ks[i]) for i in range(len(skip_ks))]
        acts = lib().trunk_fwd([(imgs[i], w) for i, w in passes], wsets)
        ctx.spec = (tuple(passes), tuple(skip_ks), n_imgs)
        ctx.n_acts = [len(a) for a in acts]
        ctx.save_for_backward(*imgs, *flat_w, *[a for ac in acts for a in ac])
        if taps is not None:
            taps.extend([list(ac) for ac in acts])
        return tuple(ac[8] for ac in acts)

    @staticmethod
    def backward(ctx, *dfeats):
        passes, skip_ks, n_imgs = ctx.spec
        saved = ctx.saved_tensors
        imgs, nw = saved[:n_imgs], 26 * len(skip_ks)
        flat_w, flat_a = saved[n_imgs:n_imgs + nw], saved[n_imgs + nw:]
        wsets = [(list(flat_w[26 * i:26 * i + 26]), skip_ks[i]) for i in range(len(skip_ks))]
        full, dfs = [], []
        for pi, (i, w) in enumerate(passes):
            acts = list(flat_a[9 * pi:9 * pi + 9])
            full.append((imgs[i], w, acts))
            df = dfeats[pi]
            dfs.append(_c(df) if df is not None else torch.zeros_like(acts[8]))
        grads = lib().trunk_bwd(full, wsets, dfs)
        return (None,) + (None,) * n_imgs + tuple(g for gs in grads for g in gs)


class BatchNormReluFunction(torch.autograd.Function):
    """Train-mode batch norm over dim 0 (+ fused ReLU), updating the running buffers in place like
    F.batch_norm(training=True): mlhot_bn_relu_fwd / _bwd."""

    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, momentum, eps):
        _need_gpu(x, gamma, beta, run_mean, run_var)
        _need_aligned("BatchNormReluFunction: run_mean / run_var (updated in place)", run_mean, run_var)
        x = _c(x)
        y, mean, var = lib().bn_relu_fwd(x, _c(gamma.detach()), _c(beta.detach()), run_mean, run_var, momentum, eps)
        ctx.eps = eps
        ctx.save_for_backward(x, y, _c(gamma.detach()), mean, var)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, var = ctx.saved_tensors
        dx, dgamma, dbeta = lib().bn_relu_bwd(x, y, _c(dy), gamma, mean, var, ctx.eps)
        return dx, dgamma, dbeta, None, None, None, None


class SpatialMeanFunction(torch.autograd.Function):
    """[n, C, H, W] -> [n, C] mean over the spatial axes."""

    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = _c(x)
        ctx.shape = tuple(x.shape)
        return lib().spatial_mean_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return lib().spatial_mean_bwd(_c(dy), ctx.shape)
