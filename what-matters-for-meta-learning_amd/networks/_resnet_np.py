"""Common implementation of the ResNet-encoder neural processes for ShapeNet3D / Distractor
(reference: networks/CondNeuralProcess.py, networks/ANP.py).

Same construction order / state_dict keys as the reference; the forward composes the mlhot HIP
operators (run-time-shaped convolutions, linears, shot-axis aggregators, FAVOR+ attention).
"""
import torch
from torch import nn

import logging

from mlhot import context, lib, ragged
from mlhot.context import ContextState         # noqa: F401  one class for both families; the name stays importable from here
from mlhot.ops import (AggFunction, FavorFunction, HeadStacksFunction, LinearFunction, StackedLinearFunction, agg_prefixes,
                       favor_prefixes, favor_prefixes_long, favor_query, linear_rows, linear_rows_any)
from networks.ResNet import run_conv
from networks.fast_attention import FastAttention
from networks.models import AttnLinear, ImageEncoder, NPDecoder, _aggregate_feature_map, _mlp3, run_trunks


_fold_refusals = set()      # (k0, k1, N) of layers mlhot_linear_rows_fwd does not serve, each logged once


def _take_prefixes(t, ks):
    """t[[k - 1 for k in ks]]: a view for consecutive context sizes, else one index_select."""
    if all(b == a + 1 for a, b in zip(ks, ks[1:])):
        return t[ks[0] - 1:ks[0] - 1 + len(ks)]
    return t.index_select(0, torch.tensor([k - 1 for k in ks], device=t.device))


def _fold_linear(sources, lin, act, n_prefix):
    """One Linear over the rows of `n_prefix` prefixes: mlhot.ops.linear_rows (bits per row independent of the row count).  A
    layer the kernel does not serve runs per prefix through LinearFunction on the gathered rows - the rows of one prefix in one
    call whatever the chunk, so still independent of the chunking."""
    rows = next(x.shape[0] * rep for x, rep, period in sources if period == 0)
    k0, k1 = sources[0][0].shape[1], sources[1][0].shape[1] if len(sources) > 1 else 0
    if lib().linear_rows_supported(k0, k1, lin.weight.shape[0]):
        return linear_rows(sources, lin.weight, lin.bias, act, rows=rows)
    if (k0, k1, lin.weight.shape[0]) not in _fold_refusals:
        _fold_refusals.add((k0, k1, lin.weight.shape[0]))
        logging.getLogger(__name__).info("forward_prefixes(fold=True): no row-invariant kernel for a Linear [%d | %d] -> %d; it runs once per prefix",
                                         k0, k1, lin.weight.shape[0])
    idx = torch.arange(rows, device=lin.weight.device)
    cols = [x[(idx // rep) % period if period else idx // rep] for x, rep, period in sources]
    x = torch.cat(cols, dim=1) if len(cols) > 1 else cols[0]
    return torch.cat([LinearFunction.apply(c, lin.weight, lin.bias, act) for c in x.chunk(n_prefix)])


class _Stacked:
    """A head stack's [N*h, k] weight and [N*h] bias with nn.Linear's attribute names (for _fold_linear)."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


class HeadStack:
    """The weights / biases of the N per-head AttnLinear layers as views of ONE [N*h, h] / [N*h] buffer, so that the heads run as
    one linear without a torch.cat per forward (3 stacks x (weight + bias) = 6 concatenations of 6 MB per step, and as many
    gradient splits in the backward).  The modules keep their own Parameters and state_dict keys (the reference's layout:
    `_W_k.3.linear.weight`); only their storage is shared.  `.to(device)` / `load_state_dict(assign=True)` give every
    parameter a storage of its own again - tensors() notices (data pointers) and re-stacks."""

    def __init__(self, mods):
        self.mods, self.w, self.b = list(mods), None, None

    def _aliased(self):
        if self.w is None:
            return False
        h = self.mods[0].linear.weight.shape[0]
        for i, m in enumerate(self.mods):
            wt, bs = m.linear.weight, m.linear.bias
            if (wt.device != self.w.device or wt.data_ptr() != self.w.data_ptr() + 4 * i * h * wt.shape[1] or not wt.is_contiguous()
                    or bs.data_ptr() != self.b.data_ptr() + 4 * i * h):
                return False
        return True

    def _adopt(self):
        """The heads' Parameters already lie behind one another in ONE storage (mlhot.optim.FlatAdam re-points every parameter at
        a view of its flat buffer, laid out by ResNetNP.flat_layout with the stacks contiguous): the stack IS that range - take
        views of it instead of concatenating (a cat would pull the parameters out of the optimizer's buffer again)."""
        ws, bs = [m.linear.weight for m in self.mods], [m.linear.bias for m in self.mods]
        for ts in (ws, bs):
            t0, n = ts[0], ts[0].numel()
            for i, t in enumerate(ts):
                if (not t.is_contiguous() or t.device != t0.device or t.dtype != t0.dtype or t.shape != t0.shape
                        or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr() or t.storage_offset() != t0.storage_offset() + i * n):
                    return False
        N, (h, k) = len(ws), ws[0].shape
        with torch.no_grad():
            self.w = torch.empty(0, dtype=ws[0].dtype, device=ws[0].device).set_(ws[0].untyped_storage(), ws[0].storage_offset(), (N * h, k))
            self.b = torch.empty(0, dtype=bs[0].dtype, device=bs[0].device).set_(bs[0].untyped_storage(), bs[0].storage_offset(), (N * h,))
        return True

    def tensors(self):
        if not self._aliased() and not self._adopt():
            ws, bs = [m.linear.weight for m in self.mods], [m.linear.bias for m in self.mods]
            h = ws[0].shape[0]
            if any(t.untyped_storage().nbytes() > 4 * t.numel() + 64 for t in ws + bs):
                # views of a larger buffer (mlhot.optim.FlatAdam's) that do not lie behind one another: concatenating would pull them out
                # of the optimizer's buffer and training of these heads would stop without a word
                raise RuntimeError("HeadStack: the heads' parameters are views of a flat buffer but not one contiguous block "
                                   "(ResNetNP.flat_layout lays a stack's weights, then its biases, back to back)")
            with torch.no_grad():
                self.w, self.b = torch.cat([t.detach() for t in ws], dim=0), torch.cat([t.detach() for t in bs], dim=0)
                for i, (wt, bt) in enumerate(zip(ws, bs)):
                    wt.data = self.w[i * h:(i + 1) * h]
                    bt.data = self.b[i * h:(i + 1) * h]
        return self.w, self.b

    def params(self):
        return [m.linear.weight for m in self.mods] + [m.linear.bias for m in self.mods]


class _CachedContext:
    """mlhot.context's adapter for ResNetNP: what its condition / extend / predict do differently from the vanilla family's.
    mlhot.cached.merge and mlhot.cached.select reach context.merge / context.select through it; the class gains no method for them."""

    def __init__(self, model):
        self.model, self.finish, self.refuse, self.shot_rows = model, model.mu, model._cached_refusals, model._shot_rows

    def prepare(self, *tensors):
        self.model._refresh_arena()

    def begin(self, launches):
        if self.model.ATTENTION:
            for mods in (self.model._W_q, self.model._W_k, self.model._W_v):   # stack the heads now: re-pointing a parameter must not look like an update later
                self.model._stack(mods).tensors()

    def empty_z(self, device):
        return None

    def route(self, state, qry_x):
        pass

    def route_shared(self, state, imgs):
        pass

    def predict_shared(self, state, imgs, attention=False):
        return self.model._predict_shared(state, imgs.contiguous(), return_attention=bool(attention))

    def predict_targets(self, state, qry_x, attention=False, mask_words=None, target_weight=None):
        if isinstance(attention, tuple):     # ("topk", k) -> (mu, [idx, wk])
            return self.model._predict_targets(state, qry_x.contiguous(), return_attention=attention)
        if attention == "mass":      # -> (mu, the tile partials of the attention mass)
            return self.model._predict_targets(state, qry_x.contiguous(), return_attention="mass", target_weight=target_weight)
        if mask_words is not None:
            return self.model._predict_targets(state, qry_x.contiguous(), return_attention=attention, mask_words=mask_words)
        if attention:
            return self.model._predict_targets(state, qry_x.contiguous(), return_attention=True)
        return self.model._predict_targets(state, qry_x.contiguous())


class ResNetNP(nn.Module):
    ATTENTION = False
    TRANSFORM_Y = False   # *Distractor classes: labels go through Linear(label_dim -> dim_w) first (CNPDistractor.py:43,89)
    CONTRASTIVE = False   # FCL* classes: forward takes the target labels too and returns a 4th value, the NT-Xent term
    N_HEADS = 8
    PREFIX_SWEEP_REFUSAL = None   # set by subclasses whose forward is not a function of the batch alone: why forward_prefixes refuses

    def __init__(self, config):
        super().__init__()
        self.device = config.device
        self.img_size = config.img_size
        self.img_channels = self.img_size[2] - 1 if config.task == "shapenet_3d" else self.img_size[2]
        self.task_num = config.tasks_per_batch
        self.label_dim = config.input_dim
        self.agg_mode = config.agg_mode
        self.img_agg = config.img_agg
        self.y_dim = config.output_dim
        if self.ATTENTION:
            self.temperature = getattr(config, "temperature", 0.07)
        if self.TRANSFORM_Y:
            self.dim_w = config.dim_w
        torch.manual_seed(config.seed)

        self.img_encoder = ImageEncoder(aggregate=self.img_agg, task_num=self.task_num, img_channels=self.img_channels)
        label_width = self.label_dim
        if self.TRANSFORM_Y:
            self.transform_y = nn.Linear(self.label_dim, self.dim_w)
            label_width = self.dim_w
        self.task_encoder = nn.Sequential(nn.Linear(256 + label_width, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(),
                                          nn.Linear(256, 256), nn.ReLU())
        if not self.ATTENTION and self.agg_mode == "baco":
            self.latent_mu = nn.Linear(256, 256)
            self.latent_var = nn.Linear(256, 256)
        self.mu = nn.Linear(256, 256)
        self.decoder = NPDecoder(aggregate=self.img_agg, output_dim=self.y_dim, task_num=self.task_num,
                                 img_channels=self.img_channels, img_size=self.img_size)
        if self.ATTENTION:
            h = 256
            self._W_k = nn.ModuleList([AttnLinear(h, h) for _ in range(self.N_HEADS)])
            self._W_v = nn.ModuleList([AttnLinear(h, h) for _ in range(self.N_HEADS)])
            self._W_q = nn.ModuleList([AttnLinear(h, h) for _ in range(self.N_HEADS)])
            self._W = AttnLinear(self.N_HEADS * h, h)
            self.attn = FastAttention(dim_heads=256, causal=False)
            self.n_heads = self.N_HEADS

    def early_grad_parameters(self):
        """Parameters whose gradients are complete before the image trunks' backward starts (that backward - ONE C call over
        the context / target / decoder passes - is the last node of the autograd graph): the MLPs, the attention and the decoder
        head, i.e. everything outside `img_encoder`, `decoder.resnet` and `decoder.conv1`.  mlhot.dist.GradBucket(early=...) all-reduces them
        from inside the backward, under the trunks' ~1 ms."""
        return [p for k, p in self.named_parameters() if not self._trunk_parameter(k)]

    @staticmethod
    def _trunk_parameter(name):
        """Gradient produced by the image trunks' backward: the encoder, the decoder's ResNet and the decoder's stem convolution
        (`decoder.conv1` is the first layer of the decoder's trunk pass, models.py:120-192 - until round 5 it was counted among the
        early parameters, so an armed eager backward issued the early bucket only after the trunks: correct, but nothing overlapped)."""
        return name.startswith("img_encoder.") or name.startswith("decoder.resnet.") or name.startswith("decoder.conv1.")

    def flat_layout(self, ctx_num=None, test_num=None):
        """(total floats, {parameter name: offset}, floats that are ever stepped) for mlhot.optim.FlatAdam: ONE flat parameter buffer
        (and, through enable_flat_grads(), its mirror for the gradients) - the early-bucket parameters first (the range
        mlhot.dist.GradBucket all-reduces from inside the backward stays contiguous), each per-head AttnLinear stack as one block
        (its 8 weights, then its 8 biases: HeadStack adopts the range), the image trunks, and at the very end the parameters no
        forward ever uses (`resnet.fc.*`: part of the reference's state_dict and of its optimizer, never given a gradient - torch's
        Adam skips them, the flat update stops in front of them).  Every slice 16-byte aligned.  The batch shape does not matter."""
        named = dict(self.named_parameters())
        order, seen = [], set()

        def take(names):
            for n in names:
                if n in named and n not in seen:
                    seen.add(n)
                    order.append(n)
        if self.ATTENTION:
            for stack in ("_W_q", "_W_k", "_W_v"):
                take([f"{stack}.{i}.linear.weight" for i in range(self.N_HEADS)])
                take([f"{stack}.{i}.linear.bias" for i in range(self.N_HEADS)])
        dead = [n for n in named if ".resnet.fc." in n]
        late = [n for n in named if self._trunk_parameter(n) and n not in dead]
        take([n for n in named if n not in late and n not in dead])
        take(late)
        active_names = len(order)
        take(dead)
        offs, total, active = {}, 0, 0
        stacked = set()        # members of a head stack's block except the last: laid back to back, the 16-byte padding behind the block
        if self.ATTENTION:
            for stack in ("_W_q", "_W_k", "_W_v"):
                for kind in ("weight", "bias"):
                    stacked.update(f"{stack}.{i}.linear.{kind}" for i in range(self.N_HEADS - 1))
        for i, n in enumerate(order):
            if i == active_names:
                active = total
            offs[n] = total
            total += named[n].numel() if n in stacked else (named[n].numel() + 3) // 4 * 4
        if active_names == len(order):
            active = total
        return total, offs, active

    def enable_flat_grads(self, on=True):
        """Every gradient of this model in ONE flat buffer (mlhot/arena.py): the kernels write weight / bias gradients straight
        into their slots, mlhot.dist.GradBucket all-reduces the buffer in place (the early bucket = its first range) instead of
        packing / unpacking <= 15 MB per step.  Process-global while on (one model trains at a time)."""
        from mlhot import binding
        from mlhot.arena import GradArena
        arena = GradArena(self.parameters(), first=self.early_grad_parameters()) if on else None
        self.__dict__["_arena"] = arena
        binding.set_grad_arena(arena)
        return arena

    def enable_split_backward(self, on=True):
        """Cut the autograd graph in front of the image trunks: the forward hands everything downstream DETACHED copies of the
        trunks' output maps (and of the Bayes-by-backprop KL) and remembers the (output, leaf) pairs, so that the backward can run
        in two parts - mlhot.dist.backward_in_two: all early-bucket gradients, then the trunks - with the first bucket's
        all-reduce in between.  Values and gradients are unchanged; a plain loss.backward() on a cut forward would stop at the
        cut, so only callers that run the second part switch this on."""
        self.__dict__["_split_backward"] = bool(on)
        self.__dict__["_cut_pairs"] = []

    def _cut(self, tensors):
        """Identity unless enable_split_backward(True): then each tensor that carries a graph is replaced by a detached leaf."""
        if not self.__dict__.get("_split_backward") or not torch.is_grad_enabled():
            return tensors
        out = []
        for t in tensors:
            if torch.is_tensor(t) and t.requires_grad:
                leaf = t.detach().requires_grad_(True)
                self.__dict__["_cut_pairs"].append((t, leaf))
                out.append(leaf)
            else:
                out.append(t)
        return out

    def _refresh_arena(self):
        arena = self.__dict__.get("_arena")
        if arena is not None:
            arena.refresh()          # a no-op unless a parameter's storage changed (first step: the head stacks were just built)

    # the 8 per-head AttnLinear layers run as ONE linear over the stacked weights; rows come out
    # token-major / head-minor, which is the layout the FAVOR+ kernels take
    def _heads(self, x, mods):
        stacks = self.__dict__.setdefault("_head_stacks", {})
        st = stacks.get(id(mods))
        if st is None:
            st = stacks[id(mods)] = HeadStack(mods)
        w, b = st.tensors()
        T, N, _ = x.shape
        return StackedLinearFunction.apply(x, w, b, self.N_HEADS, *st.params()).view(T, N, self.N_HEADS, -1)

    def _stack(self, mods):
        stacks = self.__dict__.setdefault("_head_stacks", {})
        st = stacks.get(id(mods))
        if st is None:
            st = stacks[id(mods)] = HeadStack(mods)
        return st

    def _head_projections(self, k, v, q):
        if q.is_cuda and max(q.shape[0] * q.shape[1], k.shape[0] * k.shape[1]) <= 512 and q.shape[-1] % 4 == 0:
            # the three head stacks in ONE launch per direction (few rows: mlhot_linear_multi_*)
            sts = [self._stack(m) for m in (self._W_q, self._W_k, self._W_v)]
            args, params = [], []
            for x, st in zip((q, k, v), sts):
                w, b = st.tensors()
                args += [x, w, b]
                params += st.params()
            qh, kh, vh = HeadStacksFunction.apply(self.N_HEADS, 3, *args, *params)
        else:
            qh, kh, vh = self._heads(q, self._W_q), self._heads(k, self._W_k), self._heads(v, self._W_v)
        return qh, kh, vh

    def _multihead_attention(self, k, v, q):
        qh, kh, vh = self._head_projections(k, v, q)
        merged = FavorFunction.apply(qh, kh, vh, self.attn.projection_matrix)
        return self._W(merged)

    def _latent_rows(self, feats, quirk=False):
        """What the shot-axis aggregation reads, per shot: (feats, None) for mean / max, (latent_mu, latent_var outputs) for baco."""
        if self.agg_mode in ("mean", "max"):
            return feats, None
        if self.agg_mode == "baco":
            mu_l = LinearFunction.apply(feats, self.latent_mu.weight, self.latent_mu.bias, "none")
            return mu_l, LinearFunction.apply(mu_l if quirk else feats, self.latent_var.weight, self.latent_var.bias, "none")
        raise TypeError("agg_mode is not applicable for CNP, choose from ['mean', 'max', 'baco']")

    def _aggregate(self, feats, quirk=False):
        """Shot-axis aggregation of the task-encoder features + `mu` -> task embedding [T, 256].  `quirk`: the target-set path
        of FCLCNPDistractor feeds latent_var with latent_mu's OUTPUT (FCLCNPDistractor.py:133-134); reproduced as is."""
        rs, lv = self._latent_rows(feats, quirk)
        r, _ = AggFunction.apply(self.agg_mode, rs, lv)
        return LinearFunction.apply(r, self.mu.weight, self.mu.bias, "none")

    def forward(self, batch_train_images, label_train, batch_test_images, *rest, test=False):
        """(ctx images, ctx labels, target images[, test]) -> (mu, var, 0); the FCL classes take the target labels as 4th
        positional argument and return (mu, var, 0, contrastive term) like the reference (FCLANP.py:108, FCLCNPDistractor.py:82)."""
        self._refresh_arena()
        label_test = None
        if self.CONTRASTIVE:
            if not rest:
                raise TypeError("forward() missing the target labels (label_test)")
            label_test, rest = rest[0], rest[1:]
        if rest:
            test = rest[0]
        from trainer.losses import LossFunc
        self.test_num = batch_test_images.shape[1]
        self.ctx_num = batch_train_images.shape[1]
        C, H, W = self.img_channels, self.img_size[0], self.img_size[1]
        tgt_imgs = batch_test_images.reshape(-1, C, H, W)
        ctx_imgs = batch_train_images.reshape(-1, C, H, W)
        contra_cnp = self.CONTRASTIVE and not test and not self.ATTENTION
        # Every ResNet pass of the step goes out together (one launch sequence instead of one per pass): context images and -
        # for the attention / contrastive models - target images through the encoder, target images through the decoder.  Call
        # order of the reference (and of the tap logs): context, [target,] decoder.
        jobs, roles = [], []
        if self.ctx_num:
            jobs.append(self.img_encoder.trunk_job(ctx_imgs)); roles.append("ctx")
            if self.ATTENTION or contra_cnp:
                jobs.append(self.img_encoder.trunk_job(tgt_imgs)); roles.append("tgt")
        jobs.append(self.decoder.trunk_job(tgt_imgs)); roles.append("dec")
        if self.__dict__.get("_split_backward"):
            self.__dict__["_cut_pairs"] = []
        maps = run_trunks(jobs)
        if maps is not None:
            maps = self._cut(maps)
        fm = dict(zip(roles, maps)) if maps is not None else {}

        def encode(imgs, role):
            return self.img_encoder.features(fm[role]) if role in fm else self.img_encoder(imgs)

        z_0 = None
        if self.ctx_num:
            if self.TRANSFORM_Y:
                label_train = LinearFunction.apply(label_train, self.transform_y.weight, self.transform_y.bias, "none")
            x_ctx = encode(ctx_imgs, "ctx")
            feats = _mlp3(x_ctx, self.task_encoder, last_relu=True, side=label_train)      # cat([x_ctx, labels]), ANP.py:113
            pre = None
            if self.ATTENTION:
                x_tgt = encode(tgt_imgs, "tgt")
                sample = self._multihead_attention(x_ctx, feats, x_tgt)
                if self.CONTRASTIVE and not test:                 # the contrastive term reads mu's output itself
                    sample = LinearFunction.apply(sample, self.mu.weight, self.mu.bias, "none")
                else:
                    pre = self.mu                                 # mu runs inside the decoder head's launch (models._mlp3)
            else:
                z_0 = self._aggregate(feats)
                sample = z_0[:, None, :].expand(-1, self.test_num, -1)
        else:
            sample, pre = torch.zeros(self.task_num, self.test_num, 256, device=batch_test_images.device), None
        contra = 0
        if self.CONTRASTIVE and not test:
            if self.ATTENTION:
                contra = LossFunc.contrastive_loss_ANP(sample, t=self.temperature)
            else:
                if z_0 is None:
                    raise ValueError("the contrastive term needs a non-empty context set (the reference fails here as well: z_0 is unbound)")
                x_qry = encode(tgt_imgs, "tgt")
                if self.TRANSFORM_Y:
                    label_test = LinearFunction.apply(label_test, self.transform_y.weight, self.transform_y.bias, "none")
                z_q = self._aggregate(_mlp3(torch.cat([x_qry, label_test], dim=2), self.task_encoder, last_relu=True), quirk=True)
                contra = LossFunc.contrastive_loss(z_0, z_q)
        out, var = self.decoder(batch_test_images, sample, fmap=fm.get("dec"), pre=pre)
        if self.CONTRASTIVE:
            return out, var, 0, contra
        return out, var, 0

    def _fold_head(self, x_dec, sample, rep, n_prefix, Nq):
        """The decoder head over the rows of all prefixes: fc_mu[0] on [x_dec | sample] - the plain forward's cat([x, sample]) - with
        the decoder features wrapping every T * Nq rows and `sample` row i serving `rep` rows, then fc_mu[2], fc_mu[4]."""
        x2 = x_dec.reshape(self.task_num * Nq, -1)
        fc = self.decoder.fc_mu
        h = _fold_linear([(x2, 1, x2.shape[0]), (sample, rep, 0)], fc[0], "relu", n_prefix)
        h = _fold_linear([(h, 1, 0)], fc[2], "relu", n_prefix)
        return _fold_linear([(h, 1, 0)], fc[4], "none", n_prefix).view(n_prefix, self.task_num, Nq, -1)

    def forward_prefixes(self, batch_train_images, label_train, batch_test_images, ks=None, fold=False):
        """The test-mode output for EVERY context prefix of one batch: (ctx images [T, Nc, ...], ctx labels, target images) ->
        mu [K, T, Nq, out], element i equal to `self(ctx[:, :ks[i]], labels[:, :ks[i]], targets, test=True)[0]`; `ks` defaults to
        1..Nc (a caller may chunk it: the results do not depend on the chunking, bit for bit).  Forward only, eval mode.

        Nothing a ResNet trunk computes depends on the context size, so ONE run_trunks call does the context, target and decoder
        passes of all prefixes; the task encoder and the head projections are per shot and run once too.  What sees k is the
        shot-axis aggregation or the FAVOR+ attention - for all prefixes at once in mlhot.ops.agg_prefixes / favor_prefixes
        (csrc/prefix.h) - and the Linears behind it: `_W` / `mu` and the decoder head.  Those run once per prefix over the plain
        forward's T * Nq rows: the Linear entry picks its kernel by row count, so a launch over the rows of several prefixes would
        take another kernel than the plain forward and than the same prefixes in a smaller chunk.

        `fold=True` runs each of those Linears ONCE over the len(ks) * T * Nq rows of all prefixes through mlhot.ops.linear_rows,
        whose bits per row do not depend on the row count (csrc/linear_rows.h): chunked == unchunked still holds bit for bit; against
        fold=False and the plain forward the results agree to the Linear kernels' tolerance, not to the bit."""
        if self.PREFIX_SWEEP_REFUSAL:
            raise ValueError(f"{type(self).__name__}.forward_prefixes: {self.PREFIX_SWEEP_REFUSAL}")
        if self.training:
            raise ValueError("forward_prefixes is the evaluator's test-mode path: call model.eval() first")
        Nc, Nq = batch_train_images.shape[1], batch_test_images.shape[1]
        if Nc < 1:
            raise ValueError("forward_prefixes needs at least one context shot")
        ks = list(range(1, Nc + 1)) if ks is None else [int(k) for k in ks]
        if not ks or min(ks) < 1 or max(ks) > Nc:
            raise ValueError(f"forward_prefixes: ks must be context sizes in 1..{Nc}, got {ks}")
        self._refresh_arena()
        with torch.no_grad():
            C, H, W = self.img_channels, self.img_size[0], self.img_size[1]
            tgt_imgs = batch_test_images.reshape(-1, C, H, W)
            ctx_imgs = batch_train_images.reshape(-1, C, H, W)
            jobs, roles = [self.img_encoder.trunk_job(ctx_imgs)], ["ctx"]
            if self.ATTENTION:
                jobs.append(self.img_encoder.trunk_job(tgt_imgs)); roles.append("tgt")
            jobs.append(self.decoder.trunk_job(tgt_imgs)); roles.append("dec")
            maps = run_trunks(jobs)
            if maps is None:            # no weight-stationary kernels for this image size: the per-operator route, still once per pass
                dec_map = self.decoder.resnet.trunk(run_conv(self.decoder.conv1, tgt_imgs, relu=True), None)
                x_ctx = self.img_encoder(ctx_imgs)
                x_tgt = self.img_encoder(tgt_imgs) if self.ATTENTION else None
            else:
                fm = dict(zip(roles, maps))
                dec_map = fm["dec"]
                x_ctx = self.img_encoder.features(fm["ctx"])
                x_tgt = self.img_encoder.features(fm["tgt"]) if self.ATTENTION else None
            x_dec = _aggregate_feature_map(dec_map, self.decoder.aggregate).reshape(self.task_num, Nq, -1)
            feats = self._task_features(x_ctx, label_train)
            if self.ATTENTION:
                qh, kh, vh = self._head_projections(x_ctx, feats, x_tgt)
                sel = ks                                                                      # merged[k - 1] for k in sel
                if Nc > ragged.MAX_ATTENTION_CAPACITY:        # one walk over the shots, the asked-for sizes only
                    sizes = sorted(set(ks))
                    merged = favor_prefixes_long(qh, kh, vh, self.attn.projection_matrix, sizes)
                    sel = [sizes.index(k) + 1 for k in ks]
                    self.last_prefix_attention = "prefix_long"
                else:
                    merged = favor_prefixes(qh, kh, vh, self.attn.projection_matrix)         # [Nc, T, Nq, heads * 256]
                    self.last_prefix_attention = "prefix"
                if fold:
                    rows = _take_prefixes(merged, sel).reshape(len(ks) * self.task_num * Nq, -1)
                    sample = _fold_linear([(rows, 1, 0)], self._W.linear, "none", len(ks))
                    sample = _fold_linear([(sample, 1, 0)], self.mu, "none", len(ks))
                    return self._fold_head(x_dec, sample, 1, len(ks), Nq)
                samples, pre = (self._W(merged[k - 1]) for k in sel), self.mu
            else:
                r = agg_prefixes(self.agg_mode, *self._latent_rows(feats))
                if fold:
                    z = _fold_linear([(_take_prefixes(r, ks).reshape(len(ks) * self.task_num, -1), 1, 0)], self.mu, "none", len(ks))
                    return self._fold_head(x_dec, z, Nq, len(ks), Nq)
                samples = (LinearFunction.apply(r[k - 1], self.mu.weight, self.mu.bias, "none")[:, None, :].expand(-1, Nq, -1) for k in ks)
                pre = None
            out = [_mlp3(sample, self.decoder.fc_mu, last_relu=False, side=x_dec, side_first=True, pre=pre) for sample in samples]
            return torch.stack(out)

    # ---- cached context: condition once, predict for any targets; the lifecycle itself is mlhot/context.py ---------
    def _fingerprint(self):
        return context.fingerprint(self)

    def _cached_refusals(self, what):
        if self.PREFIX_SWEEP_REFUSAL:
            raise ValueError(f"{type(self).__name__}.{what}: Bayes-by-backprop draws fresh weights in every forward, so a cached "
                             f"context is not the reference's forward ({self.PREFIX_SWEEP_REFUSAL})")
        if self.training:
            raise ValueError(f"{what} is a test-mode path: call model.eval() first")

    def condition(self, batch_train_images, label_train, ctx_len=None, capacity=None, form="keys"):
        """(ctx images [T, Nc, ...], ctx labels) -> ContextState: everything of `forward(..., test=True)` that does not depend on
        the targets, once - the context trunk pass, the task encoder and, for the attention models, the key / value head
        projections and the FAVOR+ key features (mlhot.ops.favor_keys); for the others the aggregation and `mu`.  The key
        stabiliser is the maximum over all T tasks of THIS batch, so predict reproduces forward on the same T tasks.  Eval mode.

        `ctx_len` (T host ints, 1 .. Nslots): the images are [T, Nslots, ...] and task t's context is its first ctx_len[t] slots; the
        other slots' images and labels are never read.  `capacity` >= Nslots reserves empty slots for extend (default Nslots; an
        attention model takes at most 32).  Without either argument this is the call it always was.

        `form="summary"` (attention models): the state is FAVOR+'s fixed-size summary of the context - any number
        of shots, `ctx_len` honoured, no `capacity`, no per-shot rows kept; extend absorbs any number of further shots.

        `form="long"` (attention models): per-shot key features for up to 256 slots (`capacity` defaults to
        Nslots) through the chunked kernels of csrc/favor_long.h - `ctx_len`, `capacity`, extend and
        `predict(..., return_attention=True)` all as for "keys"; the form that returns attention weights above 32 shots.

        `form="paged"` (attention models): the same for up to 4096 slots, the query walking pages of 256 slots
        (csrc/favor_paged.h) - read-out, `context_mask=` and extend included.  Never a default."""
        return context.condition(_CachedContext(self), batch_train_images, label_train, ctx_len, capacity, form)

    def extend(self, state, new_images, new_labels, new_len=None):
        """(ContextState, new ctx images [T, n, ...], their labels, new_len) -> a NEW ContextState whose task t holds new_len[t] more
        context shots (0 .. n each; default n), written behind its current ones; the old state stays valid.  Only the new shots
        run through the trunk, the task encoder and the head projections; then the masked key launches (attention) or the prefix
        aggregate with its gather and `mu` (latent) run on the kept rows.  A state needs spare slots: condition with capacity=.
        A form="long" state grows the same way, its key features re-derived by mlhot.ops.favor_keys_long."""
        return context.extend(_CachedContext(self), state, new_images, new_labels, new_len)

    def evict(self, state, drop):
        """(ContextState with per-shot rows, drop) -> a NEW ContextState without the context shots in the slots drop[t] of task t
        (T sequences of distinct host ints below state.lens[t]); the kept shots move to the front, the freed slots are spare again
        and the old state stays valid.  No image runs through the trunk: one row-compaction launch, then extend's finishing step
        on the kept rows (mlhot.cached.evict states the refusals)."""
        return context.evict(_CachedContext(self), state, drop)

    def _task_features(self, x_ctx, labels, invariant=False):
        """transform_y (the *Distractor classes) and the task encoder over [x_ctx | labels], per shot.  `invariant` (form "paged",
        DESIGN.md 6c-11): every Linear through the row-invariant kernel (mlhot.ops.linear_rows_any)."""
        if invariant:
            if self.TRANSFORM_Y:
                labels = linear_rows_any([(labels, 1, 0)], self.transform_y.weight, self.transform_y.bias)
            lins = [m for m in self.task_encoder if isinstance(m, nn.Linear)]
            h = linear_rows_any([(x_ctx, 1, 0), (labels, 1, 0)], lins[0].weight, lins[0].bias, "relu")
            for lin in lins[1:]:
                h = linear_rows_any([(h, 1, 0)], lin.weight, lin.bias, "relu")
            return h
        if self.TRANSFORM_Y:
            labels = LinearFunction.apply(labels, self.transform_y.weight, self.transform_y.bias, "none")
        return _mlp3(x_ctx, self.task_encoder, last_relu=True, side=labels)

    def _shot_rows(self, imgs, labels, invariant=False):
        """The per-shot part of condition for a packed list of P shots: images [P, C, H, W], labels [P, L] -> (kh, vh) [P, heads, 256]
        for the attention models, (rs, lv) [P, 256] for the others (baco: latent_mu's and latent_var's outputs; else lv None)."""
        maps = run_trunks([self.img_encoder.trunk_job(imgs)])
        enc = self.img_encoder
        fmap = maps[0] if maps is not None else enc.resnet.trunk(run_conv(enc.conv1, imgs, relu=True), enc._taps())
        x_ctx = _aggregate_feature_map(fmap, enc.aggregate)
        if invariant:                # form "paged": attention models only (mlhot.ragged.long_condition_args)
            feats = self._task_features(x_ctx, labels, invariant=True)
            return tuple(linear_rows_any([(x, 1, 0)], *self._stack(mods).tensors()).view(x.shape[0], self.N_HEADS, -1)
                         for x, mods in ((x_ctx, self._W_k), (feats, self._W_v)))
        feats = self._task_features(x_ctx, labels)
        if self.ATTENTION:
            return self._heads(x_ctx[None], self._W_k)[0], self._heads(feats[None], self._W_v)[0]
        return self._latent_rows(feats)

    def predict(self, state, batch_test_images, chunk=None, return_attention=False, context_mask=None, attention_mass=False, target_weight=None,
                top_k=None, shared_targets=False):
        """(ContextState, target images [T, Nq, ...]) -> mu [T, Nq, out] = `forward(ctx, labels, targets, test=True)[0]` for the
        context the state was made from, any Nq >= 1.  One run_trunks call does the target (attention models) and decoder passes;
        the query head projection, `_W`, `mu` and the decoder head go through mlhot.ops.linear_rows and the attention through
        mlhot.ops.favor_query, so nothing behind the trunks depends on how many targets share the call.  `chunk` bounds the
        targets per launch sequence.  Against forward the result agrees to the kernels' tolerance, not to the bit.

        `return_attention=True` (attention models, state forms "keys", "long" and "paged") -> (mu, attn): attn [T, heads, Nq, Nc
        slots] is FAVOR+'s weight of every context slot for every head and target, read out of the same favor_query launch - rows
        sum to 1, slots behind a task's ctx_len are exact zeros, and mu has the bits of the call without the keyword.  A model
        without attention and a summary state refuse with ValueError.

        `context_mask`: bool [T, Nq, Nc slots] -> mu [T, Nq, out], every target attending only to the slots that
        are True; [T, G, Nq, Nc slots] -> mu [T, G, Nq, out] and attn [T, G, heads, Nq, Nc]: G masks of the same targets from ONE
        pass through the trunks and one masked favor_query launch, the Linears behind it over the T * G * Nq rows.  An all-True
        mask gives plain predict's bits.  mlhot.cached.predict states the refusals.

        `attention_mass=True` -> (mu, mass): mass [T, heads, Nc slots] = attn summed over the targets, weighed by
        `target_weight` [T, Nq] (None: 1), reduced inside the favor_query launch so that attn is never stored; bit-equal to the
        documented fp32 fold of return_attention=True's attn, the same for every chunk that is a multiple of 16; mu has plain
        predict's bits.  mlhot.cached.predict states the rest.

        `top_k=k`, 1 <= k <= 16 -> (mu, idx, w), idx int32 and w fp32 [T, heads, Nq, k]: per head and target the k
        heaviest context slots (by the un-normalised score, descending, ties to the lower slot) and their weights - attn's bits
        there - selected inside the favor_query launch so that attn is never stored; -1 / 0 behind a task's shots; the same bits for
        any chunk; mu has plain predict's bits.  mlhot.cached.predict states the rest.

        `shared_targets=True`: the target images are [Nq, ...] with NO task axis and are asked of all T stored
        contexts -> mu [T, Nq, out] (and attn [T, heads, Nq, Nc slots]).  The target and decoder trunk passes run ONCE on the Nq
        images, the query head projection on Nq rows, the attention is one favor_query(shared=True) launch, and only the few-row
        Linears behind it (`_W`, `mu`, the decoder head) see T * Nq rows, the decoder features wrapping every Nq.  State forms
        "keys" and "long", latent and empty states; masks, the attention mass and top-k refuse.  mlhot.cached.predict states the
        rest."""
        if shared_targets:
            return context.predict_shared(_CachedContext(self), state, batch_test_images, chunk, return_attention, context_mask, attention_mass,
                                          target_weight, top_k)
        return context.predict(_CachedContext(self), state, batch_test_images, chunk, return_attention, context_mask, attention_mass, target_weight,
                               top_k)

    def _predict_shared(self, state, imgs, return_attention=False):
        """_predict_targets for n target images [n, C, H, W] WITHOUT a task axis, asked of all T tasks: the trunk
        passes and the query head projection see the n images once; favor_query(shared=True) answers for every task; `_W`, `mu` and
        the decoder head run over the T * n rows, the decoder features wrapping every n.  -> mu [T, n, out] (and attn)."""
        self._refresh_arena()
        with torch.no_grad():
            T, Nq = self.task_num, imgs.shape[0]
            attend = state.kind == "attention"
            jobs = ([self.img_encoder.trunk_job(imgs)] if attend else []) + [self.decoder.trunk_job(imgs)]
            maps = run_trunks(jobs)
            if maps is None:            # no weight-stationary kernels for this image size: the per-operator route
                enc = self.img_encoder
                dec_map = self.decoder.resnet.trunk(run_conv(self.decoder.conv1, imgs, relu=True), None)
                enc_map = enc.resnet.trunk(run_conv(enc.conv1, imgs, relu=True), enc._taps()) if attend else None
            else:
                dec_map, enc_map = maps[-1], maps[0] if attend else None
            # the encoder's features as rows [n, F]: ImageEncoder.features would fold them into [T, N, F], and n is no multiple of T
            x_tgt = _aggregate_feature_map(enc_map, self.img_encoder.aggregate) if attend else None
            x_dec = _aggregate_feature_map(dec_map, self.decoder.aggregate).reshape(Nq, -1)
            fc = self.decoder.fc_mu

            def head(sample, rep):
                h = _fold_linear([(x_dec, 1, Nq), (sample, rep, 0)], fc[0], "relu", 1)
                h = _fold_linear([(h, 1, 0)], fc[2], "relu", 1)
                return _fold_linear([(h, 1, 0)], fc[4], "none", 1).view(T, Nq, -1)
            if attend:
                w, b = self._stack(self._W_q).tensors()
                qh = _fold_linear([(x_tgt.reshape(Nq, -1), 1, 0)], _Stacked(w, b), "none", 1).view(Nq, self.N_HEADS, -1)
                res = favor_query(qh, state.keys, state.vh, self.attn.projection_matrix, weights=return_attention, shared=True)
                merged, attn = res if return_attention else (res, None)
                sample = _fold_linear([(merged.reshape(T * Nq, -1), 1, 0)], self._W.linear, "none", 1)
                sample = _fold_linear([(sample, 1, 0)], self.mu, "none", 1)
                mu = head(sample, 1)
                return (mu, attn) if return_attention else mu
            if state.kind == "latent":
                return head(state.z, Nq)
            return head(torch.zeros(T * Nq, 256, device=imgs.device), 1)

    def _predict_targets(self, state, batch_test_images, return_attention=False, mask_words=None, target_weight=None):
        self._refresh_arena()
        with torch.no_grad():
            T, Nq = self.task_num, batch_test_images.shape[1]
            C, H, W = self.img_channels, self.img_size[0], self.img_size[1]
            tgt_imgs = batch_test_images.reshape(-1, C, H, W)
            attend = state.kind == "attention"
            jobs = ([self.img_encoder.trunk_job(tgt_imgs)] if attend else []) + [self.decoder.trunk_job(tgt_imgs)]
            maps = run_trunks(jobs)
            if maps is None:            # no weight-stationary kernels for this image size: the per-operator route
                dec_map = self.decoder.resnet.trunk(run_conv(self.decoder.conv1, tgt_imgs, relu=True), None)
                x_tgt = self.img_encoder(tgt_imgs) if attend else None
            else:
                dec_map = maps[-1]
                x_tgt = self.img_encoder.features(maps[0]) if attend else None
            x_dec = _aggregate_feature_map(dec_map, self.decoder.aggregate).reshape(T, Nq, -1)
            if attend:
                w, b = self._stack(self._W_q).tensors()
                qh = _fold_linear([(x_tgt.reshape(T * Nq, -1), 1, 0)], _Stacked(w, b), "none", 1).view(T, Nq, self.N_HEADS, -1)
                attn = None
                if mask_words is not None:       # G masked read-outs; rows [G, T, Nq] so the decoder features wrap every T * Nq
                    G = mask_words.shape[1]
                    res = favor_query(qh, state.keys, state.vh, self.attn.projection_matrix, weights=return_attention, mask=mask_words)
                    merged, attn = res if return_attention else (res, None)
                    sample = _fold_linear([(merged.transpose(0, 1).reshape(G * T * Nq, -1), 1, 0)], self._W.linear, "none", G)
                    sample = _fold_linear([(sample, 1, 0)], self.mu, "none", G)
                    mu = self._fold_head(x_dec, sample, 1, G, Nq).transpose(0, 1).contiguous()
                    return (mu, attn) if return_attention else mu
                if isinstance(return_attention, tuple):
                    merged, *attn = favor_query(qh, state.keys, state.vh, self.attn.projection_matrix, topk=return_attention[1])
                elif return_attention == "mass":
                    merged, attn = favor_query(qh, state.keys, state.vh, self.attn.projection_matrix, mass="tiles", target_weight=target_weight)
                elif return_attention:
                    merged, attn = favor_query(qh, state.keys, state.vh, self.attn.projection_matrix, weights=True)
                else:
                    merged = favor_query(qh, state.keys, state.vh, self.attn.projection_matrix)
                sample = _fold_linear([(merged.reshape(T * Nq, -1), 1, 0)], self._W.linear, "none", 1)
                sample = _fold_linear([(sample, 1, 0)], self.mu, "none", 1)
                mu = self._fold_head(x_dec, sample, 1, 1, Nq)[0]
                return (mu, attn) if return_attention else mu
            if state.kind == "latent":
                return self._fold_head(x_dec, state.z, Nq, 1, Nq)[0]
            return self._fold_head(x_dec, torch.zeros(T * Nq, 256, device=batch_test_images.device), 1, 1, Nq)[0]
