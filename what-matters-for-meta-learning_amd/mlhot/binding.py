"""ctypes binding of the C ABI in include/mlhot.h.

`MlhotLib(path)` wraps ONE shared object.  The product loads
`csrc/libmlhot.so` through `mlhot.lib()`; the test-suite additionally wraps the
host-simulation flavour (tests/hostsim) with the same class to check the index
arithmetic without a GPU.  The signatures are declared once, in `SIGNATURES`,
and applied when a library is loaded.  Every wrapper takes torch tensors, passes
raw `data_ptr()`s and the current HIP stream, and raises `MlhotError` on a
non-zero return code - nothing here computes anything.
"""
import ctypes as C
import math
import os

import torch

HEADS = 8
MAX_HIDDEN = 4

ACT = {"none": 0, "relu": 1, "tanh": 2}
AGG = {"mean": 0, "max": 1, "baco": 2, "attention": 3}
LOSS = {"azimuth": 0, "mse": 1, "quaternion": 2, "degree": 3, "distractor": 4}

_f = C.c_void_p  # every device pointer travels as void*

ABI_VERSION = 8     # include/mlhot.h MLHOT_ABI_VERSION (2: + nt_xent, mt19937_normal, the *_staged entries, trunk / skinny flat gradients; 3: + conv12_fwd / _bwd; 4: + np_vanilla_bwd_loss; 5: + mt19937_advance; 6: + host_f32_to_u8_exact; 7: + loss_plus_fwd / _bwd; 8: adam_step / adam_step_counter take beta1, beta2 as doubles)


# sizeof of the records the augmenting ingests read (tensors built by mlhot/augment.py), checked against the library's *_bytes() at load
AUG_RECORD_BYTES = 128       # mlhot_aug_record
AUG_IMG_RECORD_BYTES = 160   # mlhot_aug_record_img
COLOUR_TABS_BYTES = 12896    # mlhot_colour_tabs


class MlhotError(RuntimeError):
    pass


class EncParams(C.Structure):       # struct mlhot_enc_params
    _fields_ = [(n, _f) for n in ("w1", "b1", "w2", "b2", "w3", "b3", "wl", "bl")]


EncGrads = EncParams                # struct mlhot_enc_grads: the same eight pointers, not const


class NpDims(C.Structure):
    _fields_ = [("T", C.c_int), ("Nc", C.c_int), ("Nq", C.c_int), ("label_dim", C.c_int), ("y_dim", C.c_int),
                ("dim_w", C.c_int), ("dim_r", C.c_int), ("dim_z", C.c_int), ("n_hidden", C.c_int),
                ("hidden", C.c_int * MAX_HIDDEN), ("dec_hidden", C.c_int), ("agg_mode", C.c_int),
                ("out_tanh", C.c_int), ("m_feat", C.c_int)]


class NpParams(C.Structure):
    """Mirrors mlhot_np_params AND mlhot_np_grads (same field order, grads lack `proj`)."""
    _fields_ = [("enc", EncParams), ("ty_w", _f), ("ty_b", _f),
                ("er_w", _f * (MAX_HIDDEN + 1)), ("er_b", _f * (MAX_HIDDEN + 1)),
                ("r2z_w", _f), ("r2z_b", _f), ("dec_w", _f * 3), ("dec_b", _f * 3),
                ("mu_w", _f), ("mu_b", _f), ("var_w", _f), ("var_b", _f),
                ("wk_w", _f * HEADS), ("wk_b", _f * HEADS), ("wv_w", _f * HEADS), ("wv_b", _f * HEADS),
                ("wq_w", _f * HEADS), ("wq_b", _f * HEADS), ("wo_w", _f), ("wo_b", _f), ("proj", _f)]


class NpGrads(C.Structure):
    _fields_ = NpParams._fields_[:-1]


class LossDesc(C.Structure):
    """mlhot_loss_desc: the loss whose gradient mlhot_np_vanilla_bwd_loss takes itself."""
    _fields_ = [("kind", C.c_int), ("gt", C.c_void_p), ("gt_dim", C.c_int), ("dloss", C.c_void_p), ("value", C.c_void_p)]


# (struct path, state_dict key) for the vanilla CNP/ANP family
def vanilla_param_map(n_hidden, baco, attention):
    m = [(("enc", "w1"), "encoder_w0.0.weight"), (("enc", "b1"), "encoder_w0.0.bias"),
         (("enc", "w2"), "encoder_w0.2.weight"), (("enc", "b2"), "encoder_w0.2.bias"),
         (("enc", "w3"), "encoder_w0.5.weight"), (("enc", "b3"), "encoder_w0.5.bias"),
         (("enc", "wl"), "encoder_w0.8.weight"), (("enc", "bl"), "encoder_w0.8.bias"),
         (("ty_w",), "transform_y.weight"), (("ty_b",), "transform_y.bias"),
         (("r2z_w",), "r_to_z.weight"), (("r2z_b",), "r_to_z.bias")]
    for i in range(n_hidden + 1):
        m += [(("er_w", i), f"encoder_r.layers.{2 * i}.weight"), (("er_b", i), f"encoder_r.layers.{2 * i}.bias")]
    for i in range(3):
        m += [(("dec_w", i), f"decoder0.{2 * i}.weight"), (("dec_b", i), f"decoder0.{2 * i}.bias")]
    if baco:
        m += [(("mu_w",), "rs_to_mu.weight"), (("mu_b",), "rs_to_mu.bias"),
              (("var_w",), "rs_to_var.weight"), (("var_b",), "rs_to_var.bias")]
    if attention:
        for tag, name in (("wk", "_W_k"), ("wv", "_W_v"), ("wq", "_W_q")):
            for i in range(HEADS):
                m += [((tag + "_w", i), f"{name}.{i}.linear.weight"), ((tag + "_b", i), f"{name}.{i}.linear.bias")]
        m += [(("wo_w",), "_W.linear.weight"), (("wo_b",), "_W.linear.bias")]
    return m


def _set(struct, path, ptr):
    if len(path) == 1:
        setattr(struct, path[0], ptr)
    elif isinstance(path[1], int):
        getattr(struct, path[0])[path[1]] = ptr
    else:
        setattr(getattr(struct, path[0]), path[1], ptr)


def _get(struct, path):
    if len(path) == 1:
        return getattr(struct, path[0])
    if isinstance(path[1], int):
        return getattr(struct, path[0])[path[1]]
    return getattr(getattr(struct, path[0]), path[1])


class BbbItem(C.Structure):          # struct mlhot_bbb_item
    _fields_ = [("mu", C.c_void_p), ("rho", C.c_void_p), ("eps", C.c_void_p), ("w", C.c_void_p), ("dw", C.c_void_p), ("dmu", C.c_void_p),
                ("drho", C.c_void_p), ("n", C.c_size_t), ("eps2", C.c_void_p), ("w2", C.c_void_p), ("dw2", C.c_void_p)]


class TrunkWset(C.Structure):        # struct mlhot_trunk_wset
    _fields_ = [("w", C.c_void_p * 13), ("b", C.c_void_p * 13), ("dw", C.c_void_p * 13), ("db", C.c_void_p * 13), ("skip_k", C.c_int)]


class TrunkPass(C.Structure):        # struct mlhot_trunk_pass
    _fields_ = [("img", C.c_void_p), ("n_img", C.c_int), ("wset", C.c_int), ("act", C.c_void_p * 9), ("dfeat", C.c_void_p)]


class ChainLayer(C.Structure):       # struct mlhot_chain_layer
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("K", C.c_int), ("N", C.c_int), ("act", C.c_int), ("side", C.c_void_p),
                ("side_w", C.c_int), ("side_ld", C.c_int), ("side_first", C.c_int), ("y", C.c_void_p), ("ldy", C.c_int)]


class ChainGrads(C.Structure):       # struct mlhot_chain_grads
    _fields_ = [("dw", C.c_void_p), ("db", C.c_void_p), ("g", C.c_void_p), ("ldg", C.c_int), ("dside", C.c_void_p),
                ("dside_ld", C.c_int), ("dside_accumulate", C.c_int)]


class RowsSrc(C.Structure):          # struct mlhot_rows_src
    _fields_ = [("x", C.c_void_p), ("ld", C.c_int), ("k", C.c_int), ("rep", C.c_int), ("period", C.c_int)]


class LinearJob(C.Structure):        # struct mlhot_linear_job
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("w", C.c_void_p), ("b", C.c_void_p), ("y", C.c_void_p), ("ldy", C.c_int),
                ("M", C.c_int), ("K", C.c_int), ("N", C.c_int), ("act", C.c_int), ("dy", C.c_void_p), ("lddy", C.c_int),
                ("dx", C.c_void_p), ("lddx", C.c_int), ("dx_accumulate", C.c_int), ("dw", C.c_void_p), ("db", C.c_void_p),
                ("x2", C.c_void_p), ("ldx2", C.c_int), ("K2", C.c_int), ("dx2", C.c_void_p), ("lddx2", C.c_int)]


_GRAD_ARENA = None


def set_grad_arena(arena):
    """Install (or, with None, remove) the flat gradient buffer the weight / bias gradients of the following calls are written
    into (mlhot/arena.py).  Process-global, like the parameters it mirrors: one model trains at a time."""
    global _GRAD_ARENA
    _GRAD_ARENA = arena


def get_grad_arena():
    return _GRAD_ARENA


def _grad_like(t):
    """Storage a kernel writes the gradient of `t` into: its slot in the installed arena while the arena may hand it out
    (GradArena.take: no live .grad in it, not handed out before in this backward pass), else a fresh tensor."""
    if _GRAD_ARENA is not None:
        v = _GRAD_ARENA.take(t)
        if v is not None:
            return v
    return torch.empty_like(t)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _addr(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _chk(*ts):
    for t in ts:
        if t is not None and (t.dtype not in (torch.float32, torch.int32, torch.uint8) or not t.is_contiguous()):
            raise MlhotError(f"mlhot expects contiguous fp32 tensors, got {t.dtype} contiguous={t.is_contiguous()}")


def _align256(x):
    return (x + 255) // 256 * 256


def _ingest_out(wrapper, src, out):
    """The fp32 [..., C, H, W] destination of an ingest of src [..., H, W, C]: `out` when it fits, a new tensor when it is None."""
    shape = (*src.shape[:-3], src.shape[-1], *src.shape[-3:-1])
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=src.device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != src.device:
        raise MlhotError(f"{wrapper}: out must be fp32 {shape} on {src.device}")
    return out


def _nhwc(wrapper, src):
    """(n_img, H, W, C) of a uint8 [..., H, W, C] batch; n_img is the product of the leading dimensions."""
    if src.dtype != torch.uint8 or src.dim() < 3:
        raise MlhotError(f"{wrapper} expects a uint8 [..., H, W, C] tensor, got {src.dtype} {tuple(src.shape)}")
    return (math.prod(src.shape[:-3]), *src.shape[-3:])


# ---- the C ABI, once: name -> (restype, argtypes), one line per prototype of include/mlhot.h in the header's order
# (tests/test_binding_abi.py holds this table to the header).  MlhotLib applies it when it loads a library.
i, z, P, f32, i64, u64, L, s, _p = C.c_int, C.c_size_t, C.c_void_p, C.c_float, C.c_int64, C.c_uint64, C.c_long, C.c_char_p, C.POINTER
f64 = C.c_double
_qkvp = [P, P, P, P, i, i, i, i, i, i]                # q, k, v, proj, T, H, Nq, Nc, d, m
_model = [_p(NpDims), _p(NpParams), P, P, P]          # dims, params, ctx_x, ctx_y, qry_x
_trunk = [_p(TrunkPass), i, _p(TrunkWset), i, i, i]   # passes, n_pass, wsets, n_wset, C, H
SIGNATURES = {
    "mlhot_version": (i, []),
    "mlhot_last_error": (s, []),
    "mlhot_set_option": (i, [s, i]),
    # bench-only launch profiler
    "mlhot_prof_begin": (i, [i]),
    "mlhot_prof_end": (i, [_p(s), _p(f32), i]),
    # NT-Xent
    "mlhot_nt_xent_ws_floats": (z, [i]),
    "mlhot_nt_xent_fwd": (i, [P, i, i, i, i, f32, P, P, P]),
    "mlhot_nt_xent_bwd": (i, [P, i, i, i, i, f32, P, P, P, P]),
    # torch's CPU normal_() stream; host-only helpers
    "mlhot_mt19937_normal": (i, [P, P, P, P, i, i64, i64, P]),
    "mlhot_mt19937_jump_ws_words": (z, [i]),
    "mlhot_mt19937_normal_par": (i, [P, P, P, P, i, i64, i64, P, i, i, P, P]),
    "mlhot_mt19937_advance": (i, [P, u64]),
    "mlhot_host_f32_to_u8_exact": (i, [P, P, i64, f32, i, _p(i64)]),
    # E1: vanilla image encoder, and its first block on its own
    "mlhot_enc_vanilla_saved_bytes": (z, [i]),
    "mlhot_enc_vanilla_scratch_bytes": (z, [i, i]),
    "mlhot_enc_vanilla_fwd": (i, [P, i, P, i, _p(EncParams), i, P, i, P, i, P, P, z, P]),
    "mlhot_enc_vanilla_bwd": (i, [P, i, P, i, _p(EncParams), i, P, i, P, i, P, _p(EncGrads), P, z, P]),
    "mlhot_conv12_scratch_bytes": (z, [i]),
    "mlhot_conv12_fwd": (i, [P, i, P, P, P, P, P, P]),
    "mlhot_conv12_bwd": (i, [P, i, P, P, P, P, P, P, P, P, P, P, z, P]),
    # nn.Linear; chains of few-row Linears; independent few-row Linears
    "mlhot_linear_bwd_scratch_bytes": (z, [i, i, i]),
    "mlhot_linear_fwd": (i, [P, i, P, P, P, i, i, i, i, i, P]),
    "mlhot_linear_bwd": (i, [P, i, P, P, i, P, i, i, i, i, i, P, i, i, P, P, P, z, P]),
    "mlhot_mlp_chain_fwd": (i, [P, i, i, _p(ChainLayer), i, P]),
    "mlhot_mlp_chain_bwd": (i, [P, i, i, _p(ChainLayer), _p(ChainGrads), i, P, i, P, i, i, P]),
    "mlhot_linear_multi_fwd": (i, [_p(LinearJob), i, P]),
    "mlhot_linear_multi_bwd": (i, [_p(LinearJob), i, P]),
    # G1: aggregation over the shot axis
    "mlhot_agg_fwd": (i, [i, P, P, i, i, i, P, P, P, P]),
    "mlhot_agg_bwd": (i, [i, P, P, P, P, P, P, i, i, i, P, P, P]),
    # FAVOR+
    "mlhot_favor_ws_bytes": (z, [i] * 6),
    "mlhot_favor_fwd": (i, _qkvp + [P, P, z, P]),
    "mlhot_favor_bwd": (i, _qkvp + [P, P, P, P, P, P, z, P]),
    "mlhot_favor_linear_supported": (i, [i] * 6),
    # every context prefix of one batch; the Linears and the loss behind the prefix operators
    "mlhot_agg_prefix_fwd": (i, [i, P, P, i, i, i, P, P, P]),
    "mlhot_favor_prefix_ws_bytes": (z, [i] * 6),
    "mlhot_favor_prefix_fwd": (i, _qkvp + [P, P, z, P]),
    "mlhot_linear_rows_supported": (i, [i, i, i]),
    "mlhot_linear_rows_fwd": (i, [_p(RowsSrc), i, P, P, P, i, i, i, i, P]),
    "mlhot_loss_prefix_fwd": (i, [i, P, P, i, i, i, i, P, P]),
    # cached context: the key side once, the query side for any number of rows
    "mlhot_favor_keys_bytes": (z, [i] * 5),
    "mlhot_favor_keys_fwd": (i, [P, P, i, i, i, i, i, P, z, P]),
    "mlhot_favor_query_ws_bytes": (z, [i] * 6),
    "mlhot_favor_query_fwd": (i, _qkvp + [P, P, z, P]),
    "mlhot_favor_query_weights_fwd": (i, _qkvp + [P, P, P, z, P]),
    # cached context with per-task context sizes: the masked key state
    "mlhot_favor_keys_ragged_fwd": (i, [P, P, P, i, i, i, i, i, P, z, P]),
    # cached context of the vanilla family: the query tail in one launch
    "mlhot_np_query_supported": (i, [_p(NpDims)]),
    "mlhot_np_query_fwd": (i, [_p(NpDims), _p(NpParams), P, i, P, P, P, P, P]),
    # the same tail against a FAVOR+ summary state
    "mlhot_np_query_summary_supported": (i, [_p(NpDims)]),
    "mlhot_np_query_summary_fwd": (i, [_p(NpDims), _p(NpParams), P, i, P, P, P]),
    # prefix sweep of the vanilla family: the query tail for K context prefixes in one launch
    "mlhot_np_prefix_supported": (i, [_p(NpDims), i]),
    "mlhot_np_prefix_ws_bytes": (z, [_p(NpDims), i]),
    "mlhot_np_prefix_fwd": (i, [_p(NpDims), _p(NpParams), P, i, P, i, P, P, P, P, P, z, P]),
    # cached context beyond 32 shots: the fixed-size summary state
    "mlhot_favor_summary_bytes": (z, [i] * 4),
    "mlhot_favor_summary_ws_bytes": (z, [i] * 5),
    "mlhot_favor_summary_init": (i, [i, i, i, i, P, z, P]),
    "mlhot_favor_summary_absorb": (i, [P, P, P, P, i, i, i, i, i, P, P, z, P, z, P]),
    "mlhot_favor_summary_query_ws_bytes": (z, [i] * 5),
    "mlhot_favor_summary_query_fwd": (i, [P, P, P, i, i, i, i, i, P, P, z, P]),
    "mlhot_favor_summary_merge": (i, [P, i, P, i, i, i, i, P, z, P]),
    "mlhot_favor_summary_gather": (i, [P, P, i, P, i, P, i, i, i, i, P, z, P]),
    "mlhot_favor_summary_retract": (i, [P, P, P, P, i, i, i, i, i, P, P, z, P, z, P]),
    # prefix sweep beyond 32 context shots: chunked running FAVOR+ prefixes
    "mlhot_favor_prefix_long_supported": (i, [i] * 7),
    "mlhot_favor_prefix_long_workspace_bytes": (z, [i] * 7),
    "mlhot_favor_prefix_long_fwd": (i, [P, P, P, P, P, i, P, i, i, i, i, i, i, P, P, z, P]),
    # per-shot key states beyond 32 context slots: chunked keys and query with read-out
    "mlhot_favor_long_supported": (i, [i] * 5),
    "mlhot_favor_keys_long_bytes": (z, [i] * 5),
    "mlhot_favor_keys_long_fwd": (i, [P, P, P, i, i, i, i, i, P, z, P]),
    "mlhot_favor_query_long_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, P, P, P, z, P]),
    # per-target context masks: one query pass, G masked read-outs
    "mlhot_favor_query_masked_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, i, P, P, P, z, P]),
    "mlhot_favor_query_long_masked_fwd": (i, [P, P, P, P, P, P, i, i, i, i, i, i, i, P, P, P, z, P]),
    # per-shot key states beyond 256 context slots: the query walks pages of 256 slots
    "mlhot_favor_paged_supported": (i, [i] * 5),
    "mlhot_favor_keys_paged_bytes": (z, [i] * 5),
    "mlhot_favor_query_paged_bytes": (z, [i] * 7),
    "mlhot_favor_keys_paged_fwd": (i, [P, P, P, i, i, i, i, i, P, z, P]),
    "mlhot_favor_query_paged_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, P, P, P, z, P]),
    "mlhot_favor_query_paged_masked_fwd": (i, [P, P, P, P, P, P, i, i, i, i, i, i, i, P, P, P, z, P]),
    # attention mass per context slot: the read-out reduced over the targets inside the query launch
    "mlhot_favor_query_mass_bytes": (z, [i] * 6),
    "mlhot_favor_query_mass_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, P, P, i, P, z, P]),
    "mlhot_favor_query_long_mass_fwd": (i, [P, P, P, P, P, P, i, i, i, i, i, i, P, P, i, P, z, P]),
    "mlhot_favor_query_paged_mass_fwd": (i, [P, P, P, P, P, P, i, i, i, i, i, i, P, P, i, P, z, P]),
    "mlhot_favor_mass_fold": (i, [P, i, i, i, P, P]),
    # top-k attention read-out: the k heaviest context slots per target row inside the query launch
    "mlhot_favor_query_topk_fwd": (i, [P, P, P, P, i, i, i, i, i, i, P, i, P, P, P, z, P]),
    "mlhot_favor_query_long_topk_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, P, i, P, P, P, z, P]),
    "mlhot_favor_query_paged_topk_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, P, i, P, P, P, z, P]),
    # shared targets: one set of query rows against every stored context
    "mlhot_favor_query_shared_ws_bytes": (z, [i] * 6),
    "mlhot_favor_query_long_shared_ws_bytes": (z, [i] * 6),
    "mlhot_favor_query_shared_fwd": (i, [P, P, P, P, i, i, i, i, i, i, i, P, P, P, z, P]),
    "mlhot_favor_query_long_shared_fwd": (i, [P, P, P, P, P, i, i, i, i, i, i, i, P, P, P, z, P]),
    # cached contexts that let shots go: the per-shot rows moved by a plan
    "mlhot_rows_compact": (i, [P, P, P, i, P, i, i, P]),
    # cached contexts joined or regrouped across states: per-shot rows gathered from several sources
    "mlhot_rows_gather": (i, [P, P, i, P, P, i, P, i, i, P]),
    # strict sharded parity of the key stabiliser
    "mlhot_favor_fwd_staged": (i, _qkvp + [P, P, z, i, P, P]),
    "mlhot_favor_bwd_staged": (i, _qkvp + [P, P, P, P, P, P, z, i, P, P]),
    # L1: losses
    "mlhot_loss_fwd": (i, [i, P, P, i, i, i, P, P]),
    "mlhot_loss_bwd": (i, [i, P, P, i, i, i, P, P, P]),
    "mlhot_loss_plus_fwd": (i, [i, P, P, i, i, i, P, f32, P, P, P]),
    "mlhot_loss_plus_bwd": (i, [i, P, P, i, i, i, P, f32, P, P, P]),
    # E2 / D2: ResNet building blocks
    "mlhot_conv2d_bwd_scratch_bytes": (z, [i] * 8),
    "mlhot_conv2d_fwd": (i, [P, P, P, P] + [i] * 9 + [P]),
    "mlhot_conv2d_bwd": (i, [P, P, P, P] + [i] * 9 + [P, P, P, P, z, P]),
    "mlhot_axpy": (i, [P, P, f32, P, z, P]),
    "mlhot_add_relu_fwd": (i, [P, P, P, z, P]),
    "mlhot_add_relu_bwd": (i, [P, P, P, z, P]),
    "mlhot_pool2_fwd": (i, [P, P, P, i, i, i, P]),
    "mlhot_pool2_bwd": (i, [P, P, P, i, i, i, P]),
    # whole ResNet trunks
    "mlhot_trunk_act_floats": (z, [i] * 4),
    "mlhot_trunk_scratch_bytes": (z, _trunk + [i]),
    "mlhot_trunk_fwd": (i, _trunk + [P, z, P]),
    "mlhot_trunk_bwd": (i, _trunk + [P, z, P]),
    # B1: Bayes-by-backprop weight sample + KL
    "mlhot_bbb_sample_fwd": (i, [P, P, P, P, P, P, z, P]),
    "mlhot_bbb_sample_bwd": (i, [P, P, P, P, P, P, P, z, P]),
    "mlhot_bbb_sample_multi_scratch_floats": (z, [_p(BbbItem), i]),
    "mlhot_bbb_sample_multi_fwd": (i, [_p(BbbItem), i, P, P, P]),
    "mlhot_bbb_sample_multi_bwd": (i, [_p(BbbItem), i, P, P]),
    # batch ingest, with and without device augmentation
    "mlhot_ingest_u8_nhwc": (i, [P, P, L, i, i, i, f32, P]),
    "mlhot_augment_record_bytes": (z, []),
    "mlhot_augment_ingest_u8": (i, [P, P, L, i, i, i, f32, P, P, i, P]),
    "mlhot_augment_img_record_bytes": (z, []),
    "mlhot_colour_tabs_bytes": (z, []),
    "mlhot_augment_ingest_u8_img": (i, [P, P, L, i, i, i, i, f32, f32, P, P, i, P, P]),
    "mlhot_pool_ingest_u8": (i, [P, L, P, P, L, P, P, L, i, i, f32, P]),
    "mlhot_pool_augment_ingest_u8_img": (i, [P, L, P, P, L, P, P, L, i, i, f32, P, P, i, P, P]),
    "mlhot_pool1_ingest_u8": (i, [P, L, P, P, L, i, i, f32, P]),
    "mlhot_pool1_augment_ingest_u8": (i, [P, L, P, P, L, i, i, f32, P, P, i, P]),
    "mlhot_pool1_augment_ingest_u8_img": (i, [P, L, P, P, L, i, i, i, f32, f32, P, P, i, P, P]),
    # optimizer
    "mlhot_adam_step": (i, [P, P, P, P, z, f32, f64, f64, f32, f32, f32, i, P]),
    "mlhot_adam_step_counter": (i, [P, P, P, P, z, f32, f64, f64, f32, f32, f32, P, P]),
    # X1: ConvEmbeddingModel building blocks
    "mlhot_bn_relu_fwd": (i, [P, P, P, P, P, f32, f32, i, i, i, P, P, P, P]),
    "mlhot_bn_relu_bwd": (i, [P, P, P, P, P, P, f32, i, i, i, P, P, P, P]),
    "mlhot_spatial_mean_fwd": (i, [P, P, i, i, P]),
    "mlhot_spatial_mean_bwd": (i, [P, P, i, i, P]),
    # whole vanilla CNP/ANP model
    "mlhot_np_struct_bytes": (z, [i]),
    "mlhot_np_saved_bytes": (z, [_p(NpDims)]),
    "mlhot_np_scratch_bytes": (z, [_p(NpDims)]),
    "mlhot_np_grads_flat_layout": (z, [_p(NpDims), _p(NpGrads)]),
    "mlhot_np_vanilla_fwd": (i, _model + [P, P, P, z, P]),
    "mlhot_np_vanilla_bwd": (i, _model + [P, P, _p(NpGrads), P, P, z, P]),
    "mlhot_np_vanilla_bwd_loss": (i, _model + [P, P, _p(LossDesc), _p(NpGrads), P, P, z, P]),
    "mlhot_np_vanilla_fwd_staged": (i, _model + [P, P, P, z, i, P, P]),
    "mlhot_np_vanilla_bwd_staged": (i, _model + [P, P, _p(NpGrads), P, P, z, i, P, P]),
}
del i, z, P, f32, i64, u64, L, s


class MlhotLib:
    _last = None      # the most recently loaded library (size queries of the static test helpers)

    def __init__(self, path):
        if not os.path.exists(path):
            raise MlhotError(f"mlhot: shared library not found: {path} (run __graft_entry__.build())")
        self.path = path
        self.c = c = C.CDLL(path)
        self.options = {}     # what set_option() has been told since loading (the library has no getter); absent = csrc/options.h's default
        MlhotLib._last = self
        if c.mlhot_version() != ABI_VERSION:       # before any other symbol is touched: an older prebuilt library lacks the newer ones
            raise MlhotError(f"mlhot: libmlhot.so has ABI version {c.mlhot_version()}, this binding needs {ABI_VERSION} "
                             f"(include/mlhot.h MLHOT_ABI_VERSION) - rebuild with mlhot.build.build_product(force=True)")
        # a prebuilt library of the right ABI version may still predate an entry added within that version: it loads, and the
        # wrappers of what it lacks say so when they are called (_fn)
        self.missing = {name for name in SIGNATURES if not hasattr(c, name)}
        for name, (restype, argtypes) in SIGNATURES.items():
            if name not in self.missing:
                fn = getattr(c, name)
                fn.restype = restype
                fn.argtypes = argtypes
        sizes = [("mlhot_np_struct_bytes", (w,), C.sizeof(st), st.__name__)
                 for w, st in enumerate((NpDims, NpParams, NpGrads, ChainLayer, ChainGrads, LinearJob))]
        sizes += [("mlhot_augment_record_bytes", (), AUG_RECORD_BYTES, "mlhot_aug_record"), ("mlhot_colour_tabs_bytes", (), COLOUR_TABS_BYTES, "mlhot_colour_tabs"),
                  ("mlhot_augment_img_record_bytes", (), AUG_IMG_RECORD_BYTES, "mlhot_aug_record_img")]
        for symbol, args, want, what in sizes:
            if symbol not in self.missing and getattr(c, symbol)(*args) != want:
                raise MlhotError(f"mlhot: ABI struct size mismatch for {what}")

    def _fn(self, wrapper, symbol):
        """The entry `symbol` of the loaded library, for the wrappers of entries added within an ABI version."""
        if symbol in self.missing:
            raise MlhotError(f"{wrapper}: {self.path} lacks {symbol} - rebuild with mlhot.build.build_product(force=True)")
        return getattr(self.c, symbol)

    # ------------------------------------------------------------------------------------------
    def _rc(self, rc, what):
        if rc != 0:
            raise MlhotError(f"{what} failed (code {rc}): {self.c.mlhot_last_error().decode()}")

    @staticmethod
    def _bytes(n, like):
        return torch.empty(max(int(n), 256), dtype=torch.uint8, device=like.device)

    def set_option(self, name, value):
        self._rc(self.c.mlhot_set_option(name.encode(), int(value)), "mlhot_set_option")
        self.options[name] = int(value)

    # ---- bench-only launch profiler -----------------------------------------------------------
    def prof_begin(self, max_records=4096):
        self._prof_cap = max_records
        self._rc(self.c.mlhot_prof_begin(max_records), "mlhot_prof_begin")

    def prof_end(self):
        """-> list of (label, ms) per kernel launch since prof_begin()"""
        cap = self._prof_cap
        labels, ms = (C.c_char_p * cap)(), (C.c_float * cap)()
        n = self.c.mlhot_prof_end(labels, ms, cap)
        return [(labels[i].decode(), float(ms[i])) for i in range(n)]

    # ---- E1 ------------------------------------------------------------------------------------
    @staticmethod
    def enc_struct(tensors):
        """tensors: (w1,b1,w2,b2,w3,b3,wl,bl)"""
        s = EncParams()
        for name, t in zip(("w1", "b1", "w2", "b2", "w3", "b3", "wl", "bl"), tensors):
            setattr(s, name, t.data_ptr())
        return s

    def enc_vanilla_fwd(self, img0, img1, params, dim_w):
        """img0 [n0,1,128,128], img1 [n1,1,128,128] or None -> feat0 [n0,dim_w], feat1, saved"""
        n0 = img0.shape[0]
        n1 = 0 if img1 is None else img1.shape[0]
        _chk(img0, img1, *params)
        n = n0 + n1
        feat0 = torch.empty(n0, dim_w, device=img0.device)
        feat1 = torch.empty(n1, dim_w, device=img0.device)
        saved = self._bytes(self.c.mlhot_enc_vanilla_saved_bytes(n), img0)
        sb = self.c.mlhot_enc_vanilla_scratch_bytes(n, dim_w)
        scratch = self._bytes(sb, img0)
        ps = self.enc_struct(params)
        self._rc(self.c.mlhot_enc_vanilla_fwd(_ptr(img0), n0, _ptr(img1), n1, C.byref(ps), dim_w, _ptr(feat0), dim_w,
                                              _ptr(feat1), dim_w, _ptr(saved), _ptr(scratch), sb, _stream(img0)),
                 "mlhot_enc_vanilla_fwd")
        return feat0, feat1, saved

    def conv12_fwd(self, img, w1, b1, w2, b2):
        """The encoder's first block on its own (conv1 + ReLU + conv2 + ReLU + 2x2 max-pool of [n,1,128,128] images) ->
        (p2 [n,48,16,16], arg-max uint8 [n,48,16,16], saved); `saved` as enc_vanilla_fwd's (enc_saved_views / enc_routes)."""
        _chk(img, w1, b1, w2, b2)
        n = img.shape[0]
        saved = self._bytes(self.c.mlhot_enc_vanilla_saved_bytes(n), img)
        self._rc(self.c.mlhot_conv12_fwd(_ptr(img), n, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(saved), _stream(img)),
                 "mlhot_conv12_fwd")
        _, p2, am2, _ = self.enc_saved_views(saved, n)
        return p2, am2, saved

    def conv12_bwd(self, img, w1, b1, w2, dp2, saved):
        """d p2 [n,48,16,16] -> (dw1, db1, dw2, db2) of the block."""
        _chk(img, w1, b1, w2, dp2)
        n = img.shape[0]
        dw1, db1, dw2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2)
        db2 = torch.empty(48, device=img.device)
        sb = self.c.mlhot_conv12_scratch_bytes(n)
        scratch = self._bytes(sb, img)
        self._rc(self.c.mlhot_conv12_bwd(_ptr(img), n, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(dp2), _ptr(saved), _ptr(dw1), _ptr(db1),
                                         _ptr(dw2), _ptr(db2), _ptr(scratch), sb, _stream(img)), "mlhot_conv12_bwd")
        return dw1, db1, dw2, db2

    @staticmethod
    def enc_saved_views(saved, n):
        """Test / diagnostic helper: the activations the encoder forward kept for its backward
        (csrc/encoder.h EncSaved: 256-byte aligned a1 | p2 | am2 | a3) as tensor views."""
        o = 0
        a1 = saved[o:o + n * 32 * 4096 * 4].view(torch.float32).view(n, 32, 64, 64)
        o = _align256(o + n * 32 * 4096 * 4)
        p2 = saved[o:o + n * 48 * 256 * 4].view(torch.float32).view(n, 48, 16, 16)
        o = _align256(o + n * 48 * 256 * 4)
        am2 = saved[o:o + n * 48 * 256].view(n, 48, 16, 16)
        o = _align256(o + n * 48 * 256)
        a3 = saved[o:o + n * 4096 * 4].view(torch.float32).view(n, 64, 8, 8)
        return a1, p2, am2, a3

    @staticmethod
    def enc_routes(saved, n):
        """Test / diagnostic helper: the piecewise-linear routing decisions the fused encoder forward took, in the form
        oracle.ref_cpu.vanilla_encoder_routed takes them: (conv1 ReLU mask [n,32,64,64] unpacked from the forward's sign-bit
        words, pool arg-max [n,48,16,16], pooled-conv2 ReLU mask, conv3 ReLU mask) as CPU tensors."""
        _, p2, am2, a3 = MlhotLib.enc_saved_views(saved, n)
        o = _align256(n * 32 * 4096 * 4)
        o = _align256(o + n * 48 * 256 * 4)
        o = _align256(o + n * 48 * 256)
        o = _align256(o + n * 4096 * 4)
        # records [img][row][column group cg][dword 4r + 2h + g], bit 16e + c = channel 16h + c of column 16cg + 4(2g + e) + r
        # (csrc/conv_tc.h m1_record)
        words = saved[o:o + n * 4096 * 4].view(torch.int32).view(n, 64, 4, 4, 2, 2, 1, 1).cpu()      # n, y, cg, r, h, g
        shifts = (16 * torch.arange(2, dtype=torch.int32).view(2, 1) + torch.arange(16, dtype=torch.int32).view(1, 16))
        bits = (words >> shifts) & 1                                                                # n, y, cg, r, h, g, e, c
        m1 = bits.permute(0, 4, 7, 1, 2, 5, 6, 3).reshape(n, 32, 64, 64).float()                   # n, (h c), y, (cg g e r)
        return m1, am2.cpu(), (p2 > 0).float().cpu(), (a3 > 0).float().cpu()

    @staticmethod
    def np_saved_views(saved, dims):
        """Test / diagnostic helper: activations mlhot_np_vanilla_fwd kept (csrc/np_vanilla.h np_saved_carve) as tensor views:
        the encoder blob (first; see enc_routes) and the task-side layers' post-ReLU outputs."""
        Rc, Rq = dims.T * dims.Nc, dims.T * dims.Nq
        n, dw = Rc + Rq, dims.dim_w
        lib = MlhotLib._last
        o = _align256(lib.c.mlhot_enc_vanilla_saved_bytes(n))

        def take(rows, cols, dtype=torch.float32):
            nonlocal o
            v = saved[o:o + rows * cols * 4].view(dtype).view(rows, cols)
            o = _align256(o + rows * cols * 4)
            return v
        out = {"enc": saved, "n": n}
        out["dec_in"] = take(Rq, dw + dims.dim_z)
        out["d1"], out["d2"] = take(Rq, dims.dec_hidden), take(Rq, dims.dec_hidden)
        if dims.Nc > 0:
            out["cat_in"] = take(Rc, dw + dw // 4)
            out["h"] = [take(Rc, dims.hidden[i]) for i in range(dims.n_hidden)]
            out["rs"] = take(Rc, dims.dim_r)
            if dims.agg_mode != AGG["attention"]:
                out["r"], out["zt"] = take(dims.T, dims.dim_r), take(dims.T, dims.dim_z)
                out["amax"] = take(dims.T, dims.dim_r, torch.int32)
            else:
                out["kh"], out["vh"], out["qh"] = take(Rc, HEADS * dw), take(Rc, HEADS * dw), take(Rq, HEADS * dw)
                out["merged"], out["rr"] = take(Rq, HEADS * dw), take(Rq, dw)
        return out

    def enc_vanilla_bwd(self, img0, img1, params, dim_w, dfeat0, dfeat1, saved):
        n0 = img0.shape[0]
        n1 = 0 if img1 is None else img1.shape[0]
        _chk(dfeat0, dfeat1)
        grads = [torch.empty_like(p) for p in params]
        sb = self.c.mlhot_enc_vanilla_scratch_bytes(n0 + n1, dim_w)
        scratch = self._bytes(sb, img0)
        ps, gs = self.enc_struct(params), self.enc_struct(grads)
        self._rc(self.c.mlhot_enc_vanilla_bwd(_ptr(img0), n0, _ptr(img1), n1, C.byref(ps), dim_w, _ptr(dfeat0), dim_w,
                                              _ptr(dfeat1), dim_w, _ptr(saved), C.byref(gs), _ptr(scratch), sb, _stream(img0)),
                 "mlhot_enc_vanilla_bwd")
        return grads

    # ---- E2 / D2 / B1 building blocks ----------------------------------------------------------
    def conv2d_fwd(self, x, w, b, stride, pad, relu):
        _chk(x, w, b)
        N, Cin, H, W = x.shape
        Cout, _, k, _ = w.shape
        HO, WO = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        y = torch.empty(N, Cout, HO, WO, device=x.device)
        self._rc(self.c.mlhot_conv2d_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), N, Cin, H, W, Cout, k, stride, pad, int(relu), _stream(x)),
                 "mlhot_conv2d_fwd")
        return y

    def conv2d_bwd(self, x, w, y, dy, stride, pad, relu, need_dx=True, has_bias=True):
        _chk(x, w, y, dy)
        N, Cin, H, W = x.shape
        Cout, _, k, _ = w.shape
        dx = torch.empty_like(x) if need_dx else None
        dw = torch.empty_like(w)
        db = torch.empty(Cout, device=x.device) if has_bias else None
        sb = self.c.mlhot_conv2d_bwd_scratch_bytes(N, Cin, H, W, Cout, k, stride, pad)
        scratch = self._bytes(sb, x)
        self._rc(self.c.mlhot_conv2d_bwd(_ptr(x), _ptr(w), _ptr(y), _ptr(dy), N, Cin, H, W, Cout, k, stride, pad, int(relu),
                                         _ptr(dx), _ptr(dw), _ptr(db), _ptr(scratch), sb, _stream(x)), "mlhot_conv2d_bwd")
        return dx, dw, db

    def add_relu_fwd(self, a, b):
        _chk(a, b)
        y = torch.empty_like(a)
        self._rc(self.c.mlhot_add_relu_fwd(_ptr(a), _ptr(b), _ptr(y), a.numel(), _stream(a)), "mlhot_add_relu_fwd")
        return y

    def add_relu_bwd(self, y, dy):
        _chk(y, dy)
        g = torch.empty_like(y)
        self._rc(self.c.mlhot_add_relu_bwd(_ptr(y), _ptr(dy), _ptr(g), y.numel(), _stream(y)), "mlhot_add_relu_bwd")
        return g

    def pool2_fwd(self, x):
        _chk(x)
        N, Cc, H, W = x.shape
        y = torch.empty(N, Cc, H // 2, W // 2, device=x.device)
        amax = torch.empty(N, Cc, H // 2, W // 2, dtype=torch.uint8, device=x.device)
        self._rc(self.c.mlhot_pool2_fwd(_ptr(x), _ptr(y), _ptr(amax), N * Cc, H, W, _stream(x)), "mlhot_pool2_fwd")
        return y, amax

    def pool2_bwd(self, dy, amax, H, W):
        _chk(dy, amax)
        N, Cc = dy.shape[:2]
        dx = torch.empty(N, Cc, H, W, device=dy.device)
        self._rc(self.c.mlhot_pool2_bwd(_ptr(dy), _ptr(amax), _ptr(dx), N * Cc, H, W, _stream(dy)), "mlhot_pool2_bwd")
        return dx

    def bbb_sample_fwd(self, mu, rho, eps):
        _chk(mu, rho, eps)
        w, klterm = torch.empty_like(mu), torch.empty_like(mu)
        kl = torch.empty((), device=mu.device)
        self._rc(self.c.mlhot_bbb_sample_fwd(_ptr(mu), _ptr(rho), _ptr(eps), _ptr(w), _ptr(klterm), _ptr(kl), mu.numel(), _stream(mu)),
                 "mlhot_bbb_sample_fwd")
        return w, kl

    def bbb_sample_bwd(self, mu, rho, eps, dw, dkl):
        _chk(dw, dkl)
        dmu, drho = _grad_like(mu), _grad_like(rho)
        self._rc(self.c.mlhot_bbb_sample_bwd(_ptr(mu), _ptr(rho), _ptr(eps), _ptr(dw), _ptr(dkl), _ptr(dmu), _ptr(drho), mu.numel(), _stream(mu)),
                 "mlhot_bbb_sample_bwd")
        return dmu, drho

    def _bbb_items(self, mus, rhos, epss, ws=None, dws=None, dmus=None, drhos=None, epss2=None, ws2=None, dws2=None):
        n = len(mus)
        if n > 32:
            raise MlhotError("bbb_sample_multi: at most 32 tensors per call")
        arr = (BbbItem * max(n, 1))()
        for i in range(n):
            it = arr[i]
            it.mu, it.rho, it.eps = mus[i].data_ptr(), rhos[i].data_ptr(), epss[i].data_ptr()
            it.w = ws[i].data_ptr() if ws is not None else None
            it.dw = dws[i].data_ptr() if dws is not None and dws[i] is not None else None
            it.dmu = dmus[i].data_ptr() if dmus is not None else None
            it.drho = drhos[i].data_ptr() if drhos is not None else None
            it.n = mus[i].numel()
            it.eps2 = epss2[i].data_ptr() if epss2 is not None else None
            it.w2 = ws2[i].data_ptr() if ws2 is not None else None
            it.dw2 = dws2[i].data_ptr() if dws2 is not None and dws2[i] is not None else None
        return arr

    def bbb_sample_multi_fwd(self, mus, rhos, epss, epss2=None):
        """Every (mu, rho, eps) triple sampled in ONE launch: returns ([w_i], kl = sum of all KL terms); with `epss2` a second
        independent sample of every tensor as well: ([w_i], [w2_i], kl)."""
        _chk(*mus, *rhos, *epss, *(epss2 or []))
        ws = [torch.empty_like(m) for m in mus]
        ws2 = [torch.empty_like(m) for m in mus] if epss2 is not None else None
        kl = torch.empty((), device=mus[0].device)
        items = self._bbb_items(mus, rhos, epss, ws=ws, epss2=epss2, ws2=ws2)
        partial = torch.empty(self.c.mlhot_bbb_sample_multi_scratch_floats(items, len(mus)), device=mus[0].device)
        self._rc(self.c.mlhot_bbb_sample_multi_fwd(items, len(mus), _ptr(partial), _ptr(kl), _stream(mus[0])), "mlhot_bbb_sample_multi_fwd")
        return (ws, kl) if epss2 is None else (ws, ws2, kl)

    def bbb_sample_multi_bwd(self, mus, rhos, epss, dws, dkl, epss2=None, dws2=None):
        _chk(*[d for d in dws if d is not None], dkl, *[d for d in (dws2 or []) if d is not None])
        dmus, drhos = [_grad_like(m) for m in mus], [_grad_like(r) for r in rhos]
        items = self._bbb_items(mus, rhos, epss, dws=dws, dmus=dmus, drhos=drhos, epss2=epss2, dws2=dws2)
        self._rc(self.c.mlhot_bbb_sample_multi_bwd(items, len(mus), _ptr(dkl), _stream(mus[0])), "mlhot_bbb_sample_multi_bwd")
        return dmus, drhos

    # ---- NT-Xent -----------------------------------------------------------------------------------
    def nt_xent_fwd(self, z, div, mod, t):
        """z [N, d] -> (loss scalar tensor, ws kept for the backward)."""
        _chk(z)
        if not z.is_cuda:
            raise MlhotError("mlhot_nt_xent_fwd: device tensors only")
        N, d = z.shape
        ws = torch.empty(self.c.mlhot_nt_xent_ws_floats(N), device=z.device)
        loss = torch.empty((), device=z.device)
        self._rc(self.c.mlhot_nt_xent_fwd(_ptr(z), N, d, div, mod, t, _ptr(ws), _ptr(loss), _stream(z)), "mlhot_nt_xent_fwd")
        return loss, ws

    def nt_xent_bwd(self, z, div, mod, t, ws, dloss):
        _chk(z, ws, dloss)
        N, d = z.shape
        dz = torch.empty_like(z)
        self._rc(self.c.mlhot_nt_xent_bwd(_ptr(z), N, d, div, mod, t, _ptr(ws), _ptr(dloss), _ptr(dz), _stream(z)), "mlhot_nt_xent_bwd")
        return dz

    # ---- torch's CPU normal_() stream on the device ---------------------------------------------
    def mt19937_normal(self, engine, uniform_ws, out, segs, nseg, total_outputs, total_groups):
        """engine: int32 [626] device tensor (state, left, next), advanced in place; segs: int64 [nseg, 4] device tensor."""
        if not (engine.is_cuda and uniform_ws.is_cuda and out.is_cuda and segs.is_cuda):
            raise MlhotError("mlhot_mt19937_normal: device tensors only")
        if engine.dtype != torch.int32 or engine.numel() != 626 or segs.dtype != torch.int64 or out.dtype != torch.float32:
            raise MlhotError("mlhot_mt19937_normal: engine int32[626], segs int64[nseg, 4], out float32")
        self._rc(self.c.mlhot_mt19937_normal(_ptr(engine), _ptr(uniform_ws), _ptr(out), _ptr(segs), nseg, total_outputs, total_groups,
                                             _stream(out)), "mlhot_mt19937_normal")

    def mt19937_normal_par(self, engine, uniform_ws, out, segs, nseg, total_outputs, total_groups, polys, n_sub, stride_blocks, jump_ws):
        """The same draw from n_sub jump-ahead sub-streams (polys: int32 [n_sub - 1, 624] device tensor from mlhot.mt_jump)."""
        if not (engine.is_cuda and uniform_ws.is_cuda and out.is_cuda and segs.is_cuda and polys.is_cuda and jump_ws.is_cuda):
            raise MlhotError("mlhot_mt19937_normal_par: device tensors only")
        if engine.dtype != torch.int32 or engine.numel() != 626 or segs.dtype != torch.int64 or out.dtype != torch.float32 or \
                polys.dtype != torch.int32 or tuple(polys.shape) != (n_sub - 1, 624) or jump_ws.dtype != torch.int32:
            raise MlhotError("mlhot_mt19937_normal_par: engine int32[626], segs int64[nseg, 4], out float32, polys int32[n_sub - 1, 624]")
        if jump_ws.numel() < self.c.mlhot_mt19937_jump_ws_words(n_sub):
            raise MlhotError("mlhot_mt19937_normal_par: jump workspace too small")
        self._rc(self.c.mlhot_mt19937_normal_par(_ptr(engine), _ptr(uniform_ws), _ptr(out), _ptr(segs), nseg, total_outputs, total_groups,
                                                 _ptr(polys), n_sub, stride_blocks, _ptr(jump_ws), _stream(out)), "mlhot_mt19937_normal_par")

    def mt19937_jump_ws_words(self, n_sub):
        return int(self.c.mlhot_mt19937_jump_ws_words(n_sub))

    def host_f32_to_u8_exact(self, src_ptr, dst_ptr, n, div=255.0, threads=1):
        """Raw host pointers (ints), n elements: bytes into dst, returns the number of elements that do NOT round-trip through
        (float)byte / div bit for bit.  Host only; `threads` native threads inside the call (the GIL is released for its duration)."""
        bad = C.c_int64(0)
        self._rc(self.c.mlhot_host_f32_to_u8_exact(C.c_void_p(src_ptr), C.c_void_p(dst_ptr), int(n), float(div), int(threads), C.byref(bad)),
                 "mlhot_host_f32_to_u8_exact")
        return int(bad.value)

    def mt19937_advance(self, engine, n_outputs):
        """engine: numpy uint32[626] (state, left, next), advanced IN PLACE by n_outputs calls.  Host only: works without a GPU."""
        import numpy as np
        if not (isinstance(engine, np.ndarray) and engine.dtype == np.uint32 and engine.size == 626 and engine.flags.c_contiguous and engine.flags.writeable):
            raise MlhotError("mt19937_advance: engine must be a writeable contiguous numpy uint32[626]")
        self._rc(self.c.mlhot_mt19937_advance(C.c_void_p(engine.ctypes.data), int(n_outputs)), "mlhot_mt19937_advance")
        return engine

    # ---- whole ResNet trunks -------------------------------------------------------------------
    @staticmethod
    def trunk_supported(C_, H):
        return (C_, H) in ((3, 64), (1, 128))

    @staticmethod
    def _trunk_structs(passes, wsets, grads=None, dfeats=None):
        """passes: [(img [n,C,H,H], wset index, [9 activation tensors])]; wsets: [([w0, b0, w1, b1, ...], skip_k)]"""
        wa = (TrunkWset * len(wsets))()
        for i, (tensors, skip_k) in enumerate(wsets):
            for c in range(13):
                wa[i].w[c], wa[i].b[c] = tensors[2 * c].data_ptr(), tensors[2 * c + 1].data_ptr()
                if grads is not None:
                    wa[i].dw[c], wa[i].db[c] = grads[i][2 * c].data_ptr(), grads[i][2 * c + 1].data_ptr()
            wa[i].skip_k = skip_k
        pa = (TrunkPass * len(passes))()
        for i, (img, wset, acts) in enumerate(passes):
            pa[i].img, pa[i].n_img, pa[i].wset = img.data_ptr(), img.shape[0], wset
            for k in range(9):
                pa[i].act[k] = acts[k].data_ptr()
            if dfeats is not None:
                pa[i].dfeat = dfeats[i].data_ptr()
        return pa, wa

    def trunk_acts(self, img):
        """The nine saved-activation tensors of one pass (a0, then (mid_i, y_i) of the four blocks) as views of one buffer."""
        n, C_, H, _ = img.shape
        sizes = [self.c.mlhot_trunk_act_floats(C_, H, n, k) for k in range(9)]
        offs, tot = [], 0
        for sz in sizes:
            offs.append(tot)
            tot += (sz + 63) // 64 * 64
        flat = torch.empty(tot, device=img.device)
        out = []
        for k, (o, sz) in enumerate(zip(offs, sizes)):
            side = H // 2 if k == 0 else H >> ((k + 1) // 2 + 1)
            out.append(flat[o:o + sz].view(n, 64, side, side))
        return out

    def _trunk_scratch(self, pa, n_pass, wa, n_wset, C_, H, backward, like):
        sb = self.c.mlhot_trunk_scratch_bytes(pa, n_pass, wa, n_wset, C_, H, backward)
        if sb == 0:
            raise MlhotError(f"mlhot_trunk: {self.c.mlhot_last_error().decode()}")
        return sb, self._bytes(sb, like)

    def trunk_fwd(self, passes, wsets):
        """passes: [(img, wset index)], wsets: [([w0, b0, ..., w12, b12], skip_k)] -> per pass the list of its 9 activations
        (the last one is the trunk's output map)."""
        imgs = [p[0] for p in passes]
        _chk(*imgs, *[t for ts, _ in wsets for t in ts])
        C_, H = imgs[0].shape[1], imgs[0].shape[2]
        full = [(img, w, self.trunk_acts(img)) for img, w in passes]
        pa, wa = self._trunk_structs(full, wsets)
        sb, scratch = self._trunk_scratch(pa, len(full), wa, len(wsets), C_, H, 0, imgs[0])
        self._rc(self.c.mlhot_trunk_fwd(pa, len(full), wa, len(wsets), C_, H, _ptr(scratch), sb, _stream(imgs[0])), "mlhot_trunk_fwd")
        return [acts for _, _, acts in full]

    def trunk_bwd(self, passes, wsets, dfeats):
        """passes: [(img, wset index, acts)], dfeats: gradient wrt each pass's output map -> per weight set its 26 gradients."""
        _chk(*dfeats)
        imgs = [p[0] for p in passes]
        C_, H = imgs[0].shape[1], imgs[0].shape[2]
        grads = [[_grad_like(t) for t in ts] for ts, _ in wsets]
        pa, wa = self._trunk_structs(passes, wsets, grads=grads, dfeats=dfeats)
        sb, scratch = self._trunk_scratch(pa, len(passes), wa, len(wsets), C_, H, 1, imgs[0])
        self._rc(self.c.mlhot_trunk_bwd(pa, len(passes), wa, len(wsets), C_, H, _ptr(scratch), sb, _stream(imgs[0])), "mlhot_trunk_bwd")
        return grads

    # ---- X1 building blocks --------------------------------------------------------------------
    def bn_relu_fwd(self, x, gamma, beta, run_mean, run_var, momentum=0.1, eps=1e-5):
        _chk(x, gamma, beta, run_mean, run_var)
        N, Cc = x.shape[:2]
        HW = x.numel() // (N * Cc)
        y = torch.empty_like(x)
        mean, var = torch.empty(Cc, device=x.device), torch.empty(Cc, device=x.device)
        self._rc(self.c.mlhot_bn_relu_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(run_mean), _ptr(run_var), momentum, eps, N, Cc, HW,
                                          _ptr(y), _ptr(mean), _ptr(var), _stream(x)), "mlhot_bn_relu_fwd")
        return y, mean, var

    def bn_relu_bwd(self, x, y, dy, gamma, mean, var, eps=1e-5):
        _chk(dy)
        N, Cc = x.shape[:2]
        HW = x.numel() // (N * Cc)
        dx, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        self._rc(self.c.mlhot_bn_relu_bwd(_ptr(x), _ptr(y), _ptr(dy), _ptr(gamma), _ptr(mean), _ptr(var), eps, N, Cc, HW,
                                          _ptr(dx), _ptr(dgamma), _ptr(dbeta), _stream(x)), "mlhot_bn_relu_bwd")
        return dx, dgamma, dbeta

    def spatial_mean_fwd(self, x):
        _chk(x)
        N, Cc = x.shape[:2]
        HW = x.numel() // (N * Cc)
        y = torch.empty(N, Cc, device=x.device)
        self._rc(self.c.mlhot_spatial_mean_fwd(_ptr(x), _ptr(y), N * Cc, HW, _stream(x)), "mlhot_spatial_mean_fwd")
        return y

    def spatial_mean_bwd(self, dy, shape):
        _chk(dy)
        dx = torch.empty(shape, device=dy.device)
        N, Cc = shape[:2]
        self._rc(self.c.mlhot_spatial_mean_bwd(_ptr(dy), _ptr(dx), N * Cc, dx.numel() // (N * Cc), _stream(dy)), "mlhot_spatial_mean_bwd")
        return dx

    # ---- linear --------------------------------------------------------------------------------
    def linear_fwd(self, x, w, b, act="none"):
        _chk(x, w, b)
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, device=x.device)
        self._rc(self.c.mlhot_linear_fwd(_ptr(x), K, _ptr(w), _ptr(b), _ptr(y), N, M, K, N, ACT[act], _stream(x)), "mlhot_linear_fwd")
        return y

    def linear_rows_supported(self, k0, k1, N):
        """Whether mlhot_linear_rows_fwd serves a layer with k ranges k0 | k1 and N outputs (pointers are checked per call)."""
        return bool(self._fn("linear_rows_supported", "mlhot_linear_rows_supported")(int(k0), int(k1), int(N)))

    def linear_rows_fwd(self, sources, w, b, act="none", rows=None, out=None):
        """y[M, N] = act([src_0 | src_1] w^T + b) with bits that do not depend on M (csrc/linear_rows.h).  sources: one or two
        (x [R, k] with unit column stride, rep, period): output row i reads x[(i // rep) % period] (period 0: no wrap).  M = `rows`,
        or R * rep of the sources without a period.  `out`: a [>= M, >= N] fp32 tensor with unit column stride to write into
        (its first M rows x N columns are written, nothing else)."""
        fn = self._fn("linear_rows_fwd", "mlhot_linear_rows_fwd")
        sources = [tuple(s) for s in sources]
        if len(sources) not in (1, 2) or any(len(s) != 3 for s in sources):
            raise MlhotError("linear_rows_fwd: sources must be one or two (tensor, rep, period) tuples")
        if act not in ACT:
            raise MlhotError(f"linear_rows_fwd: act must be one of {sorted(ACT)}, got {act!r}")
        M = None if rows is None else int(rows)
        for x, rep, period in sources:
            if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or min(x.shape) < 1 or x.stride(1) != 1 or x.device != w.device:
                raise MlhotError("linear_rows_fwd: a source must be a non-empty fp32 [rows, k] tensor with unit column stride on the weight's device")
            if int(rep) < 1 or int(period) < 0:
                raise MlhotError(f"linear_rows_fwd: rep >= 1 and period >= 0, got {rep}, {period}")
            if rows is None and int(period) == 0:
                if M is not None and M != x.shape[0] * int(rep):
                    raise MlhotError(f"linear_rows_fwd: the sources disagree on the row count ({M} against {x.shape[0] * int(rep)})")
                M = x.shape[0] * int(rep)
        if M is None or M < 1:
            raise MlhotError("linear_rows_fwd: every source wraps (period > 0): pass rows=")
        for x, rep, period in sources:      # the last source row any output row reads must exist
            last = (M - 1) // int(rep)
            need = min(last + 1, int(period)) if int(period) else last + 1
            if need > x.shape[0]:
                raise MlhotError(f"linear_rows_fwd: {M} rows with rep {rep}, period {period} read {need} source rows, the source has {x.shape[0]}")
        ktot = sum(s[0].shape[1] for s in sources)
        if w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != ktot or (b is not None and (b.dtype != torch.float32 or tuple(b.shape) != (w.shape[0],) or b.device != w.device)):
            raise MlhotError(f"linear_rows_fwd: weight {tuple(w.shape)} / bias do not fit sources of {ktot} columns")
        _chk(w, b)
        N = w.shape[0]
        if out is None:
            out = torch.empty(M, N, device=w.device)
        elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < M or out.shape[1] < N or out.stride(1) != 1 or out.device != w.device:
            raise MlhotError(f"linear_rows_fwd: out must be fp32 [>= {M}, >= {N}] with unit column stride on {w.device}")
        arr = (RowsSrc * len(sources))()
        for j, (x, rep, period) in enumerate(sources):
            arr[j].x, arr[j].ld, arr[j].k = x.data_ptr(), (x.stride(0) if x.shape[0] > 1 else x.shape[1]), x.shape[1]
            arr[j].rep, arr[j].period = int(rep), int(period)
        ldy = out.stride(0) if out.shape[0] > 1 else out.shape[1]
        self._rc(fn(arr, len(sources), _ptr(w), _ptr(b), _ptr(out), ldy, M, N, ACT[act], _stream(w)), "mlhot_linear_rows_fwd")
        return out

    def linear_bwd(self, x, w, y, dy, act="none", need_dx=True, b=None):
        """`b`: the layer's bias tensor, only to find its gradient's slot in an installed arena."""
        _chk(x, w, y, dy)
        M, K = x.shape
        N = w.shape[0]
        dx = torch.empty_like(x) if need_dx else None
        dw, db = _grad_like(w), (_grad_like(b) if b is not None else torch.empty(N, device=x.device))
        self._rc(self.c.mlhot_linear_bwd(_ptr(x), K, _ptr(w), _ptr(y), N, _ptr(dy), N, M, K, N, ACT[act], _ptr(dx), K, 0,
                                         _ptr(dw), _ptr(db), None, 0, _stream(x)), "mlhot_linear_bwd")
        return dx, dw, db

    # ---- chains of few-row linears / independent few-row linears in one launch (csrc/mlp_chain.h) --------------
    @staticmethod
    def chain_ok(x0, layers):
        """Shapes mlhot_mlp_chain_* take: <= 4 layers, <= 512 rows, input widths <= 512 (multiples of 4), outputs <= 256."""
        M = x0.shape[0]
        if not (1 <= len(layers) <= 4 and M <= 512 and x0.shape[1] % 4 == 0):
            return False
        prev = x0.shape[1]
        for k, (w, b, act, side, side_first) in enumerate(layers):
            sw = side.shape[1] if side is not None else 0
            N, K = w.shape
            if K != prev + sw or K > 512 or K % 4 or sw % 4 or N > 256 or (k + 1 < len(layers) and N % 4):
                return False
            prev = N
        return True

    def _chain_structs(self, x0, layers, ys):
        L = (ChainLayer * len(layers))()
        for k, (w, b, act, side, side_first) in enumerate(layers):
            _chk(w, b, side)
            N, K = w.shape
            L[k] = ChainLayer(_addr(w), _addr(b), K, N, ACT[act], _addr(side), side.shape[1] if side is not None else 0,
                              side.shape[1] if side is not None else 0, int(bool(side_first)), _addr(ys[k]), N)
        return L

    def mlp_chain_fwd(self, x0, layers):
        """x0 [M, K0]; layers: [(w [N, K], b, act, side [M, side_w] | None, side_first)] -> list of the layers' outputs [M, N]."""
        _chk(x0)
        M = x0.shape[0]
        ys = [torch.empty(M, w.shape[0], device=x0.device) for (w, *_rest) in layers]
        L = self._chain_structs(x0, layers, ys)
        self._rc(self.c.mlhot_mlp_chain_fwd(_ptr(x0), x0.shape[1], M, L, len(layers), _stream(x0)), "mlhot_mlp_chain_fwd")
        return ys

    def mlp_chain_bwd(self, x0, layers, ys, dy, need_dx0=True, need_dside=None):
        """-> (dx0 | None, [(dw, db, dside | None)] per layer)."""
        _chk(x0, dy)
        M = x0.shape[0]
        need_dside = need_dside or [False] * len(layers)
        L = self._chain_structs(x0, layers, ys)
        G = (ChainGrads * len(layers))()
        outs, keep = [], []
        for k, (w, b, act, side, side_first) in enumerate(layers):
            dw, db = _grad_like(w), (_grad_like(b) if b is not None else None)
            g = torch.empty(M, w.shape[0] + (-w.shape[0]) % 4, device=x0.device)
            ds = torch.empty_like(side) if (side is not None and need_dside[k]) else None
            G[k] = ChainGrads(_addr(dw), _addr(db), _addr(g), g.shape[1], _addr(ds), ds.shape[1] if ds is not None else 0, 0)
            outs.append((dw, db, ds))
            keep.append(g)
        dx0 = torch.empty_like(x0) if need_dx0 else None
        self._rc(self.c.mlhot_mlp_chain_bwd(_ptr(x0), x0.shape[1], M, L, G, len(layers), _ptr(dy), dy.shape[1], _ptr(dx0), x0.shape[1], 0,
                                            _stream(x0)), "mlhot_mlp_chain_bwd")
        return dx0, outs

    def linear_multi_fwd(self, jobs):
        """jobs: [(x [M, K1], w [N, K], b, act[, x2 [M, K - K1]])] - independent layers, one launch -> [y].  x2: the layer's input is
        cat([x, x2], -1) (folded into the kernel)."""
        J = (LinearJob * len(jobs))()
        ys = []
        for k, (x, w, b, act, *second) in enumerate(jobs):
            x2 = second[0] if second else None
            _chk(x, w, b, x2)
            y = torch.empty(x.shape[0], w.shape[0], device=x.device)
            J[k] = LinearJob(_addr(x), x.shape[1], _addr(w), _addr(b), _addr(y), w.shape[0], x.shape[0], w.shape[1], w.shape[0], ACT[act],
                             None, 0, None, 0, 0, None, None, _addr(x2), x2.shape[1] if x2 is not None else 0,
                             x2.shape[1] if x2 is not None else 0, None, 0)
            ys.append(y)
        self._rc(self.c.mlhot_linear_multi_fwd(J, len(jobs), _stream(jobs[0][0])), "mlhot_linear_multi_fwd")
        return ys

    def linear_multi_bwd(self, jobs):
        """jobs: [(x, w, y, dy, act[, bias[, x2, need_dx, need_dx2]])] -> [(dx, dw, db[, dx2])], all gradient bodies in one launch."""
        J = (LinearJob * len(jobs))()
        outs = []
        for k, (x, w, y, dy, act, *rest) in enumerate(jobs):
            b = rest[0] if rest else None
            x2, need_dx, need_dx2 = (rest[1], rest[2], rest[3]) if len(rest) > 1 else (None, True, False)
            _chk(x, w, y, dy, x2)
            dx = torch.empty_like(x) if need_dx else None
            dx2 = torch.empty_like(x2) if (x2 is not None and need_dx2) else None
            dw, db = _grad_like(w), (_grad_like(b) if b is not None else torch.empty(w.shape[0], device=x.device))
            J[k] = LinearJob(_addr(x), x.shape[1], _addr(w), None, _addr(y), w.shape[0], x.shape[0], w.shape[1], w.shape[0], ACT[act],
                             _addr(dy), dy.shape[1], _addr(dx), x.shape[1], 0, _addr(dw), _addr(db),
                             _addr(x2), x2.shape[1] if x2 is not None else 0, x2.shape[1] if x2 is not None else 0,
                             _addr(dx2), x2.shape[1] if x2 is not None else 0)
            outs.append((dx, dw, db) if x2 is None else (dx, dw, db, dx2))
        self._rc(self.c.mlhot_linear_multi_bwd(J, len(jobs), _stream(jobs[0][0])), "mlhot_linear_multi_bwd")
        return outs

    def axpy(self, a, x, alpha):
        """a + alpha * x (a None: alpha * x), elementwise, one launch."""
        _chk(a, x)
        y = torch.empty_like(x)
        self._rc(self.c.mlhot_axpy(_ptr(a), _ptr(x), float(alpha), _ptr(y), x.numel(), _stream(x)), "mlhot_axpy")
        return y

    # ---- aggregators ---------------------------------------------------------------------------
    def agg_fwd(self, mode, rs, lv=None):
        _chk(rs, lv)
        T, Nc, R = rs.shape
        r = torch.empty(T, R, device=rs.device)
        sigma = torch.empty(T, R, device=rs.device)
        amax = torch.empty(T, R, dtype=torch.int32, device=rs.device)
        self._rc(self.c.mlhot_agg_fwd(AGG[mode], _ptr(rs), _ptr(lv), T, Nc, R, _ptr(r), _ptr(sigma), _ptr(amax), _stream(rs)), "mlhot_agg_fwd")
        return r, sigma, amax

    def agg_bwd(self, mode, rs, lv, r, sigma, amax, dr):
        _chk(dr)
        T, Nc, R = rs.shape
        drs = torch.empty_like(rs)
        dlv = torch.empty_like(rs) if mode == "baco" else None
        self._rc(self.c.mlhot_agg_bwd(AGG[mode], _ptr(rs), _ptr(lv), _ptr(r), _ptr(sigma), _ptr(amax), _ptr(dr), T, Nc, R,
                                      _ptr(drs), _ptr(dlv), _stream(rs)), "mlhot_agg_bwd")
        return drs, dlv

    def agg_prefix_fwd(self, mode, rs, lv=None, want_sigma=False):
        """rs [T,Nc,R] (baco: + lv) -> r [Nc,T,R] (and sigma_z [Nc,T,R] when asked): row k-1 = agg_fwd of rs[:, :k].  Forward only."""
        fn = self._fn("agg_prefix_fwd", "mlhot_agg_prefix_fwd")
        if mode not in ("mean", "max", "baco"):
            raise MlhotError(f"agg_prefix_fwd: mode must be 'mean', 'max' or 'baco', got {mode!r}")
        if rs.dtype != torch.float32 or rs.dim() != 3 or min(rs.shape) < 1:
            raise MlhotError(f"agg_prefix_fwd expects a non-empty fp32 [T, Nc, R] tensor, got {rs.dtype} {tuple(rs.shape)}")
        if mode == "baco" and (lv is None or lv.dtype != torch.float32 or lv.shape != rs.shape or lv.device != rs.device):
            raise MlhotError(f"agg_prefix_fwd: baco needs lv as fp32 {tuple(rs.shape)} on {rs.device}")
        if mode != "baco":
            lv = None
        _chk(rs, lv)
        T, Nc, R = rs.shape
        r = torch.empty(Nc, T, R, device=rs.device)
        sigma = torch.empty(Nc, T, R, device=rs.device) if (want_sigma and mode == "baco") else None
        self._rc(fn(AGG[mode], _ptr(rs), _ptr(lv), T, Nc, R, _ptr(r), _ptr(sigma), _stream(rs)), "mlhot_agg_prefix_fwd")
        return r, sigma

    # ---- FAVOR+ --------------------------------------------------------------------------------
    def favor_prefix_supported(self, T, H, Nq, Nc, d, m):
        """Whether mlhot_favor_prefix_fwd serves this shape (else callers loop favor_fwd over the prefixes)."""
        return self.favor_prefix_ws_bytes(T, H, Nq, Nc, d, m) > 0

    def favor_prefix_ws_bytes(self, T, H, Nq, Nc, d, m):
        """Workspace bytes of mlhot_favor_prefix_fwd; 0 for a shape it does not serve."""
        return self._fn("favor_prefix_fwd", "mlhot_favor_prefix_ws_bytes")(T, H, Nq, Nc, d, m)

    def favor_prefix_fwd(self, q, k, v, proj):
        """q [T,Nq,H,d], k/v [T,Nc,H,d], proj [m,d] -> out [Nc,T,Nq,d*H]: out[k-1] = favor_fwd on the first k keys / values.  Forward only."""
        for name, t in (("q", q), ("k", k), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"favor_prefix_fwd: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = k.shape[1]
        if tuple(k.shape) != (T, Nc, H, d) or v.shape != k.shape or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d:
            raise MlhotError(f"favor_prefix_fwd: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (k, v, proj)):
            raise MlhotError("favor_prefix_fwd: q, k, v and proj must lie on one device")
        m = proj.shape[0]
        wb = self.favor_prefix_ws_bytes(T, H, Nq, Nc, d, m)
        if not wb:
            raise MlhotError(f"favor_prefix_fwd serves Nq, Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536 (got Nq={Nq} Nc={Nc} d={d} m={m}); "
                             "mlhot.ops.favor_prefixes loops favor_fwd for other shapes")
        _chk(q, k, v, proj)
        out = torch.empty(Nc, T, Nq, d * H, device=q.device)
        ws = self._bytes(wb, q)
        fn = self._fn("favor_prefix_fwd", "mlhot_favor_prefix_fwd")
        self._rc(fn(_ptr(q), _ptr(k), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(ws), ws.numel(), _stream(q)), "mlhot_favor_prefix_fwd")
        return out

    def favor_keys_bytes(self, T, H, Nc, d, m):
        """State bytes of mlhot_favor_keys_fwd; 0 for a shape the cached-context kernels do not serve."""
        return self._fn("favor_keys_fwd", "mlhot_favor_keys_bytes")(T, H, Nc, d, m)

    def favor_keys_fwd(self, k, proj):
        """k [T,Nc,H,d], proj [m,d] -> state (uint8): the finished key features F_k [T,H,Nc,mp] and the batch-global stabiliser M
        (include/mlhot.h; favor_state_views shows them).  Forward only."""
        if k.dtype != torch.float32 or k.dim() != 4 or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != k.shape[3] or proj.device != k.device:
            raise MlhotError(f"favor_keys_fwd: k must be fp32 [T, Nc, H, d] and proj fp32 [m, d] on one device, got {tuple(k.shape)}, {tuple(proj.shape)}")
        T, Nc, H, d = k.shape
        m = proj.shape[0]
        nb = self.favor_keys_bytes(T, H, Nc, d, m)
        if not nb:
            raise MlhotError(f"favor_keys_fwd serves Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536 (got Nc={Nc} d={d} m={m}); "
                             "mlhot.ops.favor_keys keeps the keys for other shapes")
        _chk(k, proj)
        state = self._bytes(nb, k)
        fn = self._fn("favor_keys_fwd", "mlhot_favor_keys_fwd")
        self._rc(fn(_ptr(k), _ptr(proj), T, H, Nc, d, m, _ptr(state), state.numel(), _stream(k)), "mlhot_favor_keys_fwd")
        return state

    def favor_keys_ragged_fwd(self, k, proj, lens):
        """favor_keys_fwd with lens [T] (int32, on k's device): row n of task t is a context shot iff n < lens[t].  The same state
        layout; M over the valid rows only, invalid rows exact zeros, their k never read (include/mlhot.h).  The values of lens are
        the caller's to check (1 .. Nc): they are read on the device.  Forward only."""
        fn = self._fn("favor_keys_ragged_fwd", "mlhot_favor_keys_ragged_fwd")
        if k.dtype != torch.float32 or k.dim() != 4 or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != k.shape[3] or proj.device != k.device:
            raise MlhotError(f"favor_keys_ragged_fwd: k must be fp32 [T, Nc, H, d] and proj fp32 [m, d] on one device, got {tuple(k.shape)}, {tuple(proj.shape)}")
        T, Nc, H, d = k.shape
        if lens.dtype != torch.int32 or tuple(lens.shape) != (T,) or lens.device != k.device:
            raise MlhotError(f"favor_keys_ragged_fwd: lens must be int32 [{T}] on {k.device}, got {lens.dtype} {tuple(lens.shape)} on {lens.device}")
        m = proj.shape[0]
        nb = self.favor_keys_bytes(T, H, Nc, d, m)
        if not nb:
            raise MlhotError(f"favor_keys_ragged_fwd serves Nc <= 32, d % 16 == 0, d <= 256, 16 <= m <= 1536 (got Nc={Nc} d={d} m={m}); "
                             "there is no masked form outside that envelope")
        _chk(k, proj, lens)
        state = self._bytes(nb, k)
        self._rc(fn(_ptr(k), _ptr(proj), _ptr(lens), T, H, Nc, d, m, _ptr(state), state.numel(), _stream(k)), "mlhot_favor_keys_ragged_fwd")
        return state

    @staticmethod
    def favor_state_views(state, T, H, Nc, m):
        """(F_k [T,H,Nc,mp], M [1]) as fp32 views of a mlhot_favor_keys_fwd state."""
        mp = (m + 15) // 16 * 16
        f = state.view(torch.float32)
        n = T * H * Nc * mp
        return f[:n].view(T, H, Nc, mp), f[n:n + 1]

    def _favor_query_dims(self, what, q, state, v, proj):
        """The checks favor_query_fwd and favor_query_weights_fwd share -> (T, H, Nq, Nc, d, m)."""
        for name, t in (("q", q), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"{what}: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = v.shape[1]
        if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
            raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (state, v, proj)):
            raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
        m = proj.shape[0]
        nb = self.favor_keys_bytes(T, H, Nc, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"{what}: the state is not mlhot_favor_keys_fwd's for T={T} H={H} Nc={Nc} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        _chk(q, v, proj, state)
        return T, H, Nq, Nc, d, m

    def favor_query_fwd(self, q, state, v, proj):
        """q [T,Nq,H,d], a mlhot_favor_keys_fwd state, v [T,Nc,H,d], proj [m,d] -> out [T,Nq,d*H] (merged order), any Nq >= 1, bits
        per row independent of the other rows (csrc/favor_cached.h).  Forward only."""
        T, H, Nq, Nc, d, m = self._favor_query_dims("favor_query_fwd", q, state, v, proj)
        out = torch.empty(T, Nq, d * H, device=q.device)
        ws = self._bytes(self._fn("favor_query_fwd", "mlhot_favor_query_ws_bytes")(T, H, Nq, Nc, d, m), q)
        fn = self._fn("favor_query_fwd", "mlhot_favor_query_fwd")
        self._rc(fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(ws), ws.numel(), _stream(q)), "mlhot_favor_query_fwd")
        return out

    def favor_query_weights_fwd(self, q, state, v, proj):
        """favor_query_fwd with FAVOR+'s per-shot weights read out: -> (out [T,Nq,d*H], w [T,H,Nq,Nc]), w = S / D of the same launch
        (include/mlhot.h).  out has favor_query_fwd's bits; the columns of w behind a masked state's lens[t] are exact
        zeros.  Forward only."""
        fn = self._fn("favor_query_weights_fwd", "mlhot_favor_query_weights_fwd")
        T, H, Nq, Nc, d, m = self._favor_query_dims("favor_query_weights_fwd", q, state, v, proj)
        out = torch.empty(T, Nq, d * H, device=q.device)
        w = torch.empty(T, H, Nq, Nc, device=q.device)
        ws = self._bytes(self._fn("favor_query_weights_fwd", "mlhot_favor_query_ws_bytes")(T, H, Nq, Nc, d, m), q)
        self._rc(fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(w), _ptr(ws), ws.numel(), _stream(q)),
                 "mlhot_favor_query_weights_fwd")
        return out, w

    # ---- per-shot key states of up to 256 slots (csrc/favor_long.h) -------------------------------
    def favor_long_supported(self, T, H, Nc, d, m):
        """Whether mlhot_favor_keys_long_fwd / mlhot_favor_query_long_fwd serve these dimensions."""
        return bool(self._fn("favor_keys_long_fwd", "mlhot_favor_long_supported")(T, H, Nc, d, m))

    def favor_keys_long_bytes(self, T, H, Nc, d, m):
        """State bytes of mlhot_favor_keys_long_fwd; 0 for a shape the long kernels do not serve."""
        return self._fn("favor_keys_long_fwd", "mlhot_favor_keys_long_bytes")(T, H, Nc, d, m)

    @staticmethod
    def _long_lens(what, lens, T, like):
        if lens is not None and (lens.dtype != torch.int32 or tuple(lens.shape) != (T,) or lens.device != like.device):
            raise MlhotError(f"{what}: lens must be int32 [{T}] on {like.device}, got {lens.dtype} {tuple(lens.shape)} on {lens.device}")

    def favor_keys_long_fwd(self, k, proj, lens=None, out=None):
        """k [T,Nc,H,d] with Nc <= 256, proj [m,d], lens [T] int32 on k's device or None (every task full) -> state (uint8): F_k
        [T,H,Nc,mp] and M in favor_keys_fwd's layout (favor_state_views shows them), rows n >= lens[t] exact zeros and their k never
        read (include/mlhot.h).  The values of lens are the caller's to check (1 .. Nc).  `out`: a buffer of
        favor_keys_long_bytes bytes to fill.  Forward only."""
        fn = self._fn("favor_keys_long_fwd", "mlhot_favor_keys_long_fwd")
        if k.dtype != torch.float32 or k.dim() != 4 or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != k.shape[3] or proj.device != k.device:
            raise MlhotError(f"favor_keys_long_fwd: k must be fp32 [T, Nc, H, d] and proj fp32 [m, d] on one device, got {tuple(k.shape)}, {tuple(proj.shape)}")
        T, Nc, H, d = k.shape
        self._long_lens("favor_keys_long_fwd", lens, T, k)
        m = proj.shape[0]
        nb = self.favor_keys_long_bytes(T, H, Nc, d, m)
        if not nb:
            raise MlhotError(f"favor_keys_long_fwd serves Nc <= 256, d % 16 == 0, d <= 256, 16 <= m <= 1536 (got Nc={Nc} d={d} m={m})")
        _chk(k, proj, lens)
        state = self._bytes(nb, k) if out is None else out
        if state.dtype != torch.uint8 or state.numel() < nb or state.device != k.device or not state.is_contiguous():
            raise MlhotError(f"favor_keys_long_fwd: out must be {nb} contiguous bytes (uint8) on {k.device}")
        self._rc(fn(_ptr(k), _ptr(proj), _ptr(lens), T, H, Nc, d, m, _ptr(state), state.numel(), _stream(k)), "mlhot_favor_keys_long_fwd")
        return state

    def favor_query_long_fwd(self, q, state, v, proj, lens=None, weights=False):
        """q [T,Nq,H,d], a favor_keys_long_fwd state, v [T,Nc,H,d], proj [m,d], the state's lens (or None) -> out [T,Nq,d*H] (merged
        order), any Nq >= 1 in one launch, bits per row independent of the other rows; weights=True -> (out, w [T,H,Nq,Nc]), w = S / D
        of the same launch with exact zeros behind lens[t], out bit-equal to the call without (csrc/favor_long.h).  Forward only."""
        what = "favor_query_long_fwd"
        fn = self._fn(what, "mlhot_favor_query_long_fwd")
        for name, t in (("q", q), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"{what}: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = v.shape[1]
        if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
            raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (state, v, proj)):
            raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
        self._long_lens(what, lens, T, q)
        m = proj.shape[0]
        nb = self.favor_keys_long_bytes(T, H, Nc, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"{what}: the state is not mlhot_favor_keys_long_fwd's for T={T} H={H} Nc={Nc} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        _chk(q, v, proj, state, lens)
        out = torch.empty(T, Nq, d * H, device=q.device)
        w = torch.empty(T, H, Nq, Nc, device=q.device) if weights else None
        ws = self._bytes(256, q)
        self._rc(fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), _ptr(lens), T, H, Nq, Nc, d, m, _ptr(out), _ptr(w), _ptr(ws), ws.numel(), _stream(q)),
                 "mlhot_favor_query_long_fwd")
        return (out, w) if weights else out

    # ---- per-target context masks: one query pass, G masked read-outs -----------
    def favor_query_masked_fwd(self, q, state, v, proj, mask_words, lens=None, long=False, weights=False):
        """q [T,Nq,H,d], a favor_keys_fwd state (long=True: a favor_keys_long_fwd state and its lens), v [T,Nc,H,d], proj [m,d],
        mask_words [T,G,Nq,ceil(Nc/32)] int32 on q's device (bit j of word c = slot 32 c + j, mlhot.ragged.pack_mask) ->
        out [T,G,Nq,d*H]; weights=True -> (out, w [T,G,H,Nq,Nc]).  ONE launch: the query features and S once per 16 rows, the G
        masked read-outs behind them; a row that keeps no valid slot gets exact zeros (include/mlhot.h).  Forward only."""
        what = "favor_query_long_masked_fwd" if long else "favor_query_masked_fwd"
        fn = self._fn(what, "mlhot_" + what)
        if long:
            for name, t in (("q", q), ("v", v)):
                if t.dtype != torch.float32 or t.dim() != 4:
                    raise MlhotError(f"{what}: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
            T, Nq, H, d = q.shape
            Nc = v.shape[1]
            if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
                raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
            if any(t.device != q.device for t in (state, v, proj)):
                raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
            self._long_lens(what, lens, T, q)
            m = proj.shape[0]
            nb = self.favor_keys_long_bytes(T, H, Nc, d, m)
            if not nb or state.dtype != torch.uint8 or state.numel() < nb:
                raise MlhotError(f"{what}: the state is not mlhot_favor_keys_long_fwd's for T={T} H={H} Nc={Nc} d={d} m={m} "
                                 f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
            _chk(q, v, proj, state, lens)
            ws = self._bytes(256, q)
        else:
            T, H, Nq, Nc, d, m = self._favor_query_dims(what, q, state, v, proj)
            ws = self._bytes(self._fn(what, "mlhot_favor_query_ws_bytes")(T, H, Nq, Nc, d, m), q)
        W = (Nc + 31) // 32
        if (not isinstance(mask_words, torch.Tensor) or mask_words.dtype != torch.int32 or mask_words.dim() != 4 or mask_words.shape[1] < 1
                or (mask_words.shape[0], mask_words.shape[2], mask_words.shape[3]) != (T, Nq, W) or mask_words.device != q.device):
            got = f"{mask_words.dtype} {tuple(mask_words.shape)} on {mask_words.device}" if isinstance(mask_words, torch.Tensor) else type(mask_words).__name__
            raise MlhotError(f"{what}: mask_words must be int32 [T={T}, G, Nq={Nq}, {W}] on {q.device}, got {got}")
        _chk(mask_words)
        G = mask_words.shape[1]
        out = torch.empty(T, G, Nq, d * H, device=q.device)
        w = torch.empty(T, G, H, Nq, Nc, device=q.device) if weights else None
        if long:
            rc = fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), _ptr(lens), _ptr(mask_words), G, T, H, Nq, Nc, d, m, _ptr(out), _ptr(w), _ptr(ws),
                    ws.numel(), _stream(q))
        else:
            rc = fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), _ptr(mask_words), G, T, H, Nq, Nc, d, m, _ptr(out), _ptr(w), _ptr(ws), ws.numel(), _stream(q))
        self._rc(rc, "mlhot_" + what)
        return (out, w) if weights else out

    # ---- per-shot key states of up to 4096 slots, the query in pages of 256 (csrc/favor_paged.h) -----
    def favor_paged_supported(self, T, H, Nc, d, m):
        """Whether mlhot_favor_keys_paged_fwd / mlhot_favor_query_paged_fwd serve these dimensions."""
        return bool(self._fn("favor_keys_paged_fwd", "mlhot_favor_paged_supported")(T, H, Nc, d, m))

    def favor_keys_paged_bytes(self, T, H, Nc, d, m):
        """State bytes of mlhot_favor_keys_paged_fwd; 0 for a shape the paged kernels do not serve."""
        return self._fn("favor_keys_paged_fwd", "mlhot_favor_keys_paged_bytes")(T, H, Nc, d, m)

    def favor_keys_paged_fwd(self, k, proj, lens=None, out=None):
        """k [T,Nc,H,d] with Nc <= 4096, proj [m,d], lens [T] int32 on k's device or None (every task full) -> state (uint8) in
        favor_keys_long_fwd's layout and under its contract (include/mlhot.h).  Forward only."""
        what = "favor_keys_paged_fwd"
        fn = self._fn(what, "mlhot_favor_keys_paged_fwd")
        if k.dtype != torch.float32 or k.dim() != 4 or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != k.shape[3] or proj.device != k.device:
            raise MlhotError(f"{what}: k must be fp32 [T, Nc, H, d] and proj fp32 [m, d] on one device, got {tuple(k.shape)}, {tuple(proj.shape)}")
        T, Nc, H, d = k.shape
        self._long_lens(what, lens, T, k)
        m = proj.shape[0]
        nb = self.favor_keys_paged_bytes(T, H, Nc, d, m)
        if not nb:
            raise MlhotError(f"{what} serves Nc <= 4096, d % 16 == 0, d <= 256, 16 <= m <= 1536 (got Nc={Nc} d={d} m={m})")
        _chk(k, proj, lens)
        state = self._bytes(nb, k) if out is None else out
        if state.dtype != torch.uint8 or state.numel() < nb or state.device != k.device or not state.is_contiguous():
            raise MlhotError(f"{what}: out must be {nb} contiguous bytes (uint8) on {k.device}")
        self._rc(fn(_ptr(k), _ptr(proj), _ptr(lens), T, H, Nc, d, m, _ptr(state), state.numel(), _stream(k)), "mlhot_favor_keys_paged_fwd")
        return state

    def favor_query_paged_fwd(self, q, state, v, proj, lens=None, weights=False, mask_words=None):
        """q [T,Nq,H,d], a favor_keys_paged_fwd state, v [T,Nc,H,d], proj [m,d], the state's lens (or None) -> out [T,Nq,d*H];
        weights=True -> (out, w [T,H,Nq,Nc]).  mask_words [T,G,Nq,ceil(Nc/32)] int32 (mlhot.ragged.pack_mask): the masked entry,
        out [T,G,Nq,d*H] and w [T,G,H,Nq,Nc].  ONE launch either way (csrc/favor_paged.h).  Forward only."""
        what = "favor_query_paged_fwd" if mask_words is None else "favor_query_paged_masked_fwd"
        fn = self._fn(what, "mlhot_" + what)
        for name, t in (("q", q), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"{what}: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = v.shape[1]
        if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
            raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (state, v, proj)):
            raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
        self._long_lens(what, lens, T, q)
        m = proj.shape[0]
        nb = self.favor_keys_paged_bytes(T, H, Nc, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"{what}: the state is not mlhot_favor_keys_paged_fwd's for T={T} H={H} Nc={Nc} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        _chk(q, v, proj, state, lens)
        G = 0
        if mask_words is not None:
            W = (Nc + 31) // 32
            if (not isinstance(mask_words, torch.Tensor) or mask_words.dtype != torch.int32 or mask_words.dim() != 4 or mask_words.shape[1] < 1
                    or (mask_words.shape[0], mask_words.shape[2], mask_words.shape[3]) != (T, Nq, W) or mask_words.device != q.device):
                got = f"{mask_words.dtype} {tuple(mask_words.shape)} on {mask_words.device}" if isinstance(mask_words, torch.Tensor) else type(mask_words).__name__
                raise MlhotError(f"{what}: mask_words must be int32 [T={T}, G, Nq={Nq}, {W}] on {q.device}, got {got}")
            _chk(mask_words)
            G = mask_words.shape[1]
        ws = self._bytes(self._fn(what, "mlhot_favor_query_paged_bytes")(T, H, Nq, Nc, d, m, G), q)
        if G:
            out = torch.empty(T, G, Nq, d * H, device=q.device)
            w = torch.empty(T, G, H, Nq, Nc, device=q.device) if weights else None
            rc = fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), _ptr(lens), _ptr(mask_words), G, T, H, Nq, Nc, d, m, _ptr(out), _ptr(w), _ptr(ws),
                    ws.numel(), _stream(q))
        else:
            out = torch.empty(T, Nq, d * H, device=q.device)
            w = torch.empty(T, H, Nq, Nc, device=q.device) if weights else None
            rc = fn(_ptr(q), _ptr(state), _ptr(v), _ptr(proj), _ptr(lens), T, H, Nq, Nc, d, m, _ptr(out), _ptr(w), _ptr(ws), ws.numel(), _stream(q))
        self._rc(rc, "mlhot_" + what)
        return (out, w) if weights else out

    # ---- attention mass per context slot (csrc/favor_mass.h) ----------------------
    def favor_query_mass_bytes(self, T, H, Nq, Nc, d, m):
        """Workspace bytes of the mass entries - the tile partials, T H ceil(Nq/16) Nc floats: the path's whole footprint beside out
        and mass; 0 for a shape none of them serves."""
        return self._fn("favor_query_mass_fwd", "mlhot_favor_query_mass_bytes")(T, H, Nq, Nc, d, m)

    def favor_query_mass_fwd(self, q, state, v, proj, form, lens=None, tw=None, fold=True):
        """q [T,Nq,H,d], a per-shot key state of `form` ("cached" | "long" | "paged") with its lens, v [T,Nc,H,d], proj [m,d], tw
        [T,Nq] fp32 on q's device or None -> (out [T,Nq,d*H], mass [T,H,Nc]): mass[t,h,c] = sum_n tw[t,n] w[t,h,n,c] of the read-out
        w = S / D, reduced inside the query launch in a fixed order - w itself is never stored; out has the plain entry's bits
        (include/mlhot.h).  fold=False -> (out, part [T,H,ceil(Nq/16),Nc]), the tile partials for favor_mass_fold.  Forward only."""
        what = {"cached": "favor_query_mass_fwd", "long": "favor_query_long_mass_fwd", "paged": "favor_query_paged_mass_fwd"}[form]
        fn = self._fn(what, "mlhot_" + what)
        for name, t in (("q", q), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"{what}: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = v.shape[1]
        if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
            raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (state, v, proj)):
            raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
        self._long_lens(what, lens, T, q)
        if form == "cached" and lens is not None:
            raise MlhotError(f"{what}: a keys state carries its lens as zero rows of F_k; the entry takes none")
        m = proj.shape[0]
        nb = {"cached": self.favor_keys_bytes, "long": self.favor_keys_long_bytes, "paged": self.favor_keys_paged_bytes}[form](T, H, Nc, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"{what}: the state is not this form's for T={T} H={H} Nc={Nc} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        if tw is not None and (not isinstance(tw, torch.Tensor) or tw.dtype != torch.float32 or tuple(tw.shape) != (T, Nq) or tw.device != q.device):
            got = f"{tw.dtype} {tuple(tw.shape)} on {tw.device}" if isinstance(tw, torch.Tensor) else type(tw).__name__
            raise MlhotError(f"{what}: tw must be fp32 [T={T}, Nq={Nq}] on {q.device}, got {got}")
        _chk(q, v, proj, state, lens, tw)
        out = torch.empty(T, Nq, d * H, device=q.device)
        ntile = (Nq + 15) // 16
        mass = torch.empty((T, H, Nc) if fold else (T, H, ntile, Nc), device=q.device)
        ws = self._bytes(self.favor_query_mass_bytes(T, H, Nq, Nc, d, m) if fold else 256, q)
        head = (_ptr(q), _ptr(state), _ptr(v), _ptr(proj)) + (() if form == "cached" else (_ptr(lens),))
        self._rc(fn(*head, _ptr(tw), T, H, Nq, Nc, d, m, _ptr(out), _ptr(mass), int(bool(fold)), _ptr(ws), ws.numel(), _stream(q)), "mlhot_" + what)
        return out, mass

    # ---- top-k attention read-out (csrc/favor_topk.h) ---------------------------
    def favor_query_topk_fwd(self, q, state, v, proj, form, k, lens=None):
        """q [T,Nq,H,d], a per-shot key state of `form` ("cached" | "long" | "paged") with its lens, v [T,Nc,H,d], proj [m,d], 1 <= k
        <= 16 -> (out [T,Nq,d*H], idx int32 [T,H,Nq,k], wk fp32 [T,H,Nq,k]): per row the k valid slots of largest S, descending, ties to
        the lower slot, and wk = S / D with the bits the read-out stores into w[t,h,n,idx]; -1 / +0 behind the valid slots; selected
        inside the query launch - w itself is never stored; out has the plain entry's bits (include/mlhot.h).  Forward only."""
        what = {"cached": "favor_query_topk_fwd", "long": "favor_query_long_topk_fwd", "paged": "favor_query_paged_topk_fwd"}[form]
        fn = self._fn(what, "mlhot_" + what)
        for name, t in (("q", q), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"{what}: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = v.shape[1]
        if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
            raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (state, v, proj)):
            raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 16:
            raise MlhotError(f"{what}: k must be an integer in 1 .. 16, got {k!r}")
        self._long_lens(what, lens, T, q)
        if form == "cached" and lens is not None:
            raise MlhotError(f"{what}: a keys state carries its lens as zero rows of F_k; the entry takes none")
        m = proj.shape[0]
        nb = {"cached": self.favor_keys_bytes, "long": self.favor_keys_long_bytes, "paged": self.favor_keys_paged_bytes}[form](T, H, Nc, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"{what}: the state is not this form's for T={T} H={H} Nc={Nc} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        _chk(q, v, proj, state, lens)
        out = torch.empty(T, Nq, d * H, device=q.device)
        idx = torch.empty(T, H, Nq, k, device=q.device, dtype=torch.int32)
        wk = torch.empty(T, H, Nq, k, device=q.device)
        ws = self._bytes(256, q)
        head = (_ptr(q), _ptr(state), _ptr(v), _ptr(proj)) + (() if form == "cached" else (_ptr(lens),))
        self._rc(fn(*head, T, H, Nq, Nc, d, m, _ptr(out), k, _ptr(idx), _ptr(wk), _ptr(ws), ws.numel(), _stream(q)), "mlhot_" + what)
        return out, idx, wk

    # ---- shared targets: one set of query rows against every stored context (csrc/favor_shared.h) ----
    def favor_query_shared_fwd(self, q, state, v, proj, form, lens=None, weights=False, task_group=0):
        """q [Nq,H,d] WITHOUT a task axis, a per-shot key state of `form` ("cached" | "long") for T tasks with its lens, v [T,Nc,H,d],
        proj [m,d] -> out [T,Nq,d*H]; weights=True -> (out, w [T,H,Nq,Nc]).  ONE launch: the query features once per (head, 16 rows),
        then the per-task entry's steps for each task of the workgroup's group of `task_group` tasks (0: the library picks).  out and
        w have the bits of favor_query_fwd / _weights_fwd / _long_fwd on q expanded to [T,Nq,H,d], whatever task_group
        (include/mlhot.h).  Forward only."""
        what = {"cached": "favor_query_shared_fwd", "long": "favor_query_long_shared_fwd"}[form]
        fn = self._fn(what, "mlhot_" + what)
        if q.dtype != torch.float32 or q.dim() != 3:
            raise MlhotError(f"{what}: q must be fp32 [Nq, H, d] - the targets are shared by the tasks - got {q.dtype} {tuple(q.shape)}")
        if v.dtype != torch.float32 or v.dim() != 4:
            raise MlhotError(f"{what}: v must be fp32 [T, Nc, H, d], got {v.dtype} {tuple(v.shape)}")
        Nq, H, d = q.shape
        T, Nc = v.shape[0], v.shape[1]
        if tuple(v.shape) != (T, Nc, H, d) or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d or Nq < 1:
            raise MlhotError(f"{what}: q {tuple(q.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (state, v, proj)):
            raise MlhotError(f"{what}: q, state, v and proj must lie on one device")
        if isinstance(task_group, bool) or not isinstance(task_group, int) or task_group < 0:
            raise MlhotError(f"{what}: task_group must be an integer >= 0 (0: the library picks), got {task_group!r}")
        self._long_lens(what, lens, T, q)
        if form == "cached" and lens is not None:
            raise MlhotError(f"{what}: a keys state carries its lens as zero rows of F_k; the entry takes none")
        m = proj.shape[0]
        nb = {"cached": self.favor_keys_bytes, "long": self.favor_keys_long_bytes}[form](T, H, Nc, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"{what}: the state is not this form's for T={T} H={H} Nc={Nc} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        _chk(q, v, proj, state, lens)
        out = torch.empty(T, Nq, d * H, device=q.device)
        w = torch.empty(T, H, Nq, Nc, device=q.device) if weights else None
        ws = self._bytes(self._fn(what, "mlhot_" + what.replace("_fwd", "_ws_bytes"))(T, H, Nq, Nc, d, m), q)
        head = (_ptr(q), _ptr(state), _ptr(v), _ptr(proj)) + (() if form == "cached" else (_ptr(lens),))
        self._rc(fn(*head, T, H, Nq, Nc, d, m, task_group, _ptr(out), _ptr(w), _ptr(ws), ws.numel(), _stream(q)), "mlhot_" + what)
        return (out, w) if weights else out

    def favor_mass_fold(self, part):
        """part [T,H,tiles,Nc] (the tile partials of favor_query_mass_fwd(fold=False), concatenated along the tile axis in target
        order) -> mass [T,H,Nc]: the tiles added per column in ascending order, one rounded add each."""
        fn = self._fn("favor_mass_fold", "mlhot_favor_mass_fold")
        if part.dtype != torch.float32 or part.dim() != 4 or part.shape[2] < 1:
            raise MlhotError(f"favor_mass_fold: part must be fp32 [T, H, tiles, Nc], got {part.dtype} {tuple(part.shape)}")
        _chk(part)
        T, H, ntile, Nc = part.shape
        mass = torch.empty(T, H, Nc, device=part.device)
        self._rc(fn(_ptr(part), T * H, ntile, Nc, _ptr(mass), _stream(part)), "mlhot_favor_mass_fold")
        return mass

    # ---- the fixed-size FAVOR+ summary state (csrc/favor_summary.h) ------------------------------
    def favor_summary_bytes(self, T, H, d, m):
        """State bytes of the summary kernels; 0 for a shape they do not serve."""
        return self._fn("favor_summary_init", "mlhot_favor_summary_bytes")(T, H, d, m)

    def favor_summary_init(self, T, H, d, m, device):
        """A fresh summary state (uint8) for T tasks, H heads, proj [m, d]: M = -inf, everything else 0."""
        nb = self.favor_summary_bytes(T, H, d, m)
        if not nb:
            raise MlhotError(f"favor_summary_init serves d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536 (got d={d} m={m})")
        state = torch.empty(nb, dtype=torch.uint8, device=device)
        self._rc(self._fn("favor_summary_init", "mlhot_favor_summary_init")(T, H, d, m, _ptr(state), nb, _stream(state)), "mlhot_favor_summary_init")
        return state

    def favor_summary_absorb(self, k, v, proj, state, lens=None, out=None):
        """k, v [T,n,H,d] (n <= 32 new shots per task), proj [m,d], a summary state, lens [T] int32 on k's device or None -> the
        state with the valid new shots absorbed: `out` (may be `state` itself: in place) or a new buffer; `state` is then left as it
        is.  Rows at or behind lens[t] of k and v are never read.  The values of lens are the caller's to check (0 .. n)."""
        return self._favor_summary_step("favor_summary_absorb", k, v, proj, state, lens, out)

    def favor_summary_retract(self, k, v, proj, state, lens=None, out=None):
        """favor_summary_absorb's arguments with the sign turned: k, v [T,n,H,d] are shots that WERE absorbed into
        `state` and are taken out again -> `out` (may be `state` itself: in place, the same bits) or a new buffer.  The stabiliser
        stays the state's.  That the shots were absorbed, and that no task goes below zero shots, is the caller's to see to."""
        return self._favor_summary_step("favor_summary_retract", k, v, proj, state, lens, out)

    def _favor_summary_step(self, what, k, v, proj, state, lens, out):
        """mlhot_favor_summary_absorb / _retract: one argument list, one set of checks."""
        fn = self._fn(what, "mlhot_" + what)
        if k.dtype != torch.float32 or k.dim() != 4 or v.dtype != torch.float32 or v.shape != k.shape or proj.dtype != torch.float32 or proj.dim() != 2 \
                or proj.shape[1] != k.shape[3] or any(t.device != k.device for t in (v, proj, state)):
            raise MlhotError(f"{what}: k and v must be fp32 [T, n, H, d] and proj fp32 [m, d] on the state's device, got "
                             f"{tuple(k.shape)}, {tuple(v.shape)}, {tuple(proj.shape)}")
        T, n, H, d = k.shape
        m = proj.shape[0]
        if lens is not None and (lens.dtype != torch.int32 or tuple(lens.shape) != (T,) or lens.device != k.device):
            raise MlhotError(f"{what}: lens must be int32 [{T}] on {k.device}, got {lens.dtype} {tuple(lens.shape)} on {lens.device}")
        nb = self.favor_summary_bytes(T, H, d, m)
        wb = self._fn(what, "mlhot_favor_summary_ws_bytes")(T, H, n, d, m)
        if not nb or not wb:
            raise MlhotError(f"{what} serves 1 <= n <= 32 new shots per call, d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536 "
                             f"(got n={n} d={d} m={m}); mlhot.ops.favor_absorb chunks longer inputs")
        if out is None:
            out = torch.empty(nb, dtype=torch.uint8, device=k.device)
        for name, s in (("state", state), ("out", out)):
            if s.dtype != torch.uint8 or s.numel() < nb or s.device != k.device:
                raise MlhotError(f"{what}: {name} is not a summary state for T={T} H={H} d={d} m={m} ({s.numel()} bytes, {nb} needed)")
        _chk(k, v, proj, state, out, *([lens] if lens is not None else []))
        ws = self._bytes(wb, k)
        self._rc(fn(_ptr(k), _ptr(v), _ptr(proj), _ptr(lens) if lens is not None else None, T, H, n, d, m, _ptr(state), _ptr(out), nb,
                    _ptr(ws), ws.numel(), _stream(k)), "mlhot_" + what)
        return out

    @staticmethod
    def favor_summary_views(state, T, H, d, m):
        """(A [T,H,mp,d], a [T,H,mp], vs [T,H,d], cnt [T,H] int32, M [1]) as views of a summary state (include/mlhot.h)."""
        mp = (m + 15) // 16 * 16
        f = state.view(torch.float32)
        nA, na, nv = T * H * mp * d, T * H * mp, T * H * d
        at = nA + na + nv
        cnt = state.view(torch.int32)[at + 16:at + 16 + T * H].view(T, H)
        return f[:nA].view(T, H, mp, d), f[nA:nA + na].view(T, H, mp), f[nA + na:at].view(T, H, d), cnt, f[at:at + 1]

    def favor_summary_query_fwd(self, q, state, proj):
        """q [T,Nq,H,d], a summary state, proj [m,d] -> out [T,Nq,d*H] (merged order), any Nq >= 1 in one launch, bits per row
        independent of the other rows (csrc/favor_summary.h).  Forward only."""
        if q.dtype != torch.float32 or q.dim() != 4 or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != q.shape[3] or q.shape[1] < 1:
            raise MlhotError(f"favor_summary_query_fwd: q must be fp32 [T, Nq, H, d] and proj fp32 [m, d], got {tuple(q.shape)}, {tuple(proj.shape)}")
        if any(t.device != q.device for t in (state, proj)):
            raise MlhotError("favor_summary_query_fwd: q, state and proj must lie on one device")
        T, Nq, H, d = q.shape
        m = proj.shape[0]
        nb = self.favor_summary_bytes(T, H, d, m)
        if not nb or state.dtype != torch.uint8 or state.numel() < nb:
            raise MlhotError(f"favor_summary_query_fwd: the state is not a summary state for T={T} H={H} d={d} m={m} "
                             f"({state.numel()} bytes, {nb} needed; 0 = shape not served)")
        _chk(q, proj, state)
        out = torch.empty(T, Nq, d * H, device=q.device)
        ws = self._bytes(self._fn("favor_summary_query_fwd", "mlhot_favor_summary_query_ws_bytes")(T, H, Nq, d, m), q)
        fn = self._fn("favor_summary_query_fwd", "mlhot_favor_summary_query_fwd")
        self._rc(fn(_ptr(q), _ptr(state), _ptr(proj), T, H, Nq, d, m, _ptr(out), _ptr(ws), ws.numel(), _stream(q)), "mlhot_favor_summary_query_fwd")
        return out

    MERGE_MAX = 8          # states per mlhot_favor_summary_merge call

    def favor_summary_merge(self, bufs, T, H, d, m, floor=None, out=None):
        """1 .. 8 summary states (uint8, favor_summary_bytes(T, H, d, m) bytes each) that were absorbed apart -> the state of all their
        shots, in a buffer of its own (`out`, or a new one); the inputs are only read.  M' = max of the states' stabilisers and of
        `floor` (None, or ONE fp32 value on the states' device: "the stabiliser is at least this"); A and a are rescaled by
        exp(M_i - M') and added in the order of `bufs`, vs and cnt are added (include/mlhot.h).  One launch."""
        fn = self._fn("favor_summary_merge", "mlhot_favor_summary_merge")
        bufs = list(bufs)
        nb = self.favor_summary_bytes(T, H, d, m)
        if not nb:
            raise MlhotError(f"favor_summary_merge serves d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536 (got d={d} m={m})")
        if not 1 <= len(bufs) <= self.MERGE_MAX:
            raise MlhotError(f"favor_summary_merge takes 1 .. {self.MERGE_MAX} states per call (got {len(bufs)}); mlhot.ops.favor_merge folds more in groups")
        if out is None:
            out = torch.empty(nb, dtype=torch.uint8, device=bufs[0].device)
        for name, s in [(f"state {k}", b) for k, b in enumerate(bufs)] + [("out", out)]:
            if not isinstance(s, torch.Tensor) or s.dtype != torch.uint8 or s.numel() < nb or s.device != bufs[0].device or not s.is_cuda:
                raise MlhotError(f"favor_summary_merge: {name} is not a summary state for T={T} H={H} d={d} m={m} on one GPU ({nb} bytes needed)")
        if floor is not None and (not isinstance(floor, torch.Tensor) or floor.dtype != torch.float32 or floor.numel() != 1 or floor.device != out.device):
            raise MlhotError(f"favor_summary_merge: floor must be one fp32 value on {out.device}")
        _chk(out, floor, *bufs)
        table = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
        self._rc(fn(table, len(bufs), _ptr(floor), T, H, d, m, _ptr(out), nb, _stream(out)), "mlhot_favor_summary_merge")
        return out

    GATHER_PARTS = 8       # parts per task and mlhot_favor_summary_gather call

    def favor_summary_gather(self, bufs, tasks, parts, H, d, m, floor=None, out=None):
        """1 .. 8 summary states of the same (H, d, m) - bufs[i] (uint8) holds tasks[i] tasks - and parts, an int32 [T_out, P, 2]
        tensor on their device (1 <= P <= 8; entry (i, u): task u of state i, i < 0 ends a row) -> the state of T_out tasks whose
        task t is the sum of its row's parts, in a buffer of its own (`out`, or a new one); the inputs are only read.  M' = max of
        ALL the states' stabilisers and of `floor` (as in favor_summary_merge); the kernel reads the table and holds every index to
        its range, whether the table means what the caller wants is the caller's to check (include/mlhot.h).
        One launch."""
        fn = self._fn("favor_summary_gather", "mlhot_favor_summary_gather")
        bufs, tasks = list(bufs), [int(t) for t in tasks]
        if not 1 <= len(bufs) <= self.MERGE_MAX or len(tasks) != len(bufs):
            raise MlhotError(f"favor_summary_gather takes 1 .. {self.MERGE_MAX} states per call and one task count for each (got {len(bufs)} states, "
                             f"{len(tasks)} counts); mlhot.ops.favor_gather folds more in groups")
        if not isinstance(parts, torch.Tensor) or parts.dtype != torch.int32 or parts.dim() != 3 or parts.shape[0] < 1 or parts.shape[2] != 2 \
                or not 1 <= parts.shape[1] <= self.GATHER_PARTS:
            raise MlhotError(f"favor_summary_gather: parts must be an int32 [T_out, P, 2] tensor with 1 <= P <= {self.GATHER_PARTS}, got "
                             f"{getattr(parts, 'dtype', type(parts).__name__)} {tuple(getattr(parts, 'shape', ()))}")
        T_out, P = parts.shape[0], parts.shape[1]
        need = [self.favor_summary_bytes(t, H, d, m) if t >= 1 else 0 for t in tasks]
        nb = self.favor_summary_bytes(T_out, H, d, m)
        if not nb or not all(need):
            raise MlhotError(f"favor_summary_gather serves d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536 and at least one task per state "
                             f"(got d={d} m={m}, tasks {tasks} -> {T_out})")
        if out is None:
            out = torch.empty(nb, dtype=torch.uint8, device=bufs[0].device)
        for name, s, want in [(f"state {k}", b, n) for k, (b, n) in enumerate(zip(bufs, need))] + [("out", out, nb), ("parts", parts, 0)]:
            if not isinstance(s, torch.Tensor) or s.device != bufs[0].device or not s.is_cuda or (want and (s.dtype != torch.uint8 or s.numel() < want)):
                raise MlhotError(f"favor_summary_gather: {name} is not a summary state for H={H} d={d} m={m} on one GPU ({want} bytes needed)"
                                 if want else f"favor_summary_gather: parts must lie on the states' GPU, {bufs[0].device}")
        if floor is not None and (not isinstance(floor, torch.Tensor) or floor.dtype != torch.float32 or floor.numel() != 1 or floor.device != out.device):
            raise MlhotError(f"favor_summary_gather: floor must be one fp32 value on {out.device}")
        _chk(out, floor, parts, *bufs)
        table = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
        counts = (C.c_int * len(bufs))(*tasks)
        self._rc(fn(table, counts, len(bufs), _ptr(parts), P, _ptr(floor), T_out, H, d, m, _ptr(out), nb, _stream(out)), "mlhot_favor_summary_gather")
        return out

    # ---- per-shot rows moved by a plan (csrc/rows_compact.h) --------------------------------------
    ROWS_COMPACT_SETS = 4  # row sets per mlhot_rows_compact call

    def rows_compact(self, srcs, plan):
        """1 .. 4 row sets srcs[i] fp32 [T, cap, ...] that share plan, int32 [T, cap] on their device -> new tensors of the same
        shapes: row s of task t is row plan[t, s] of the source, a row of exact zeros where plan[t, s] is -1 (or out of range).
        ONE launch (rows.compact); the sources are only read.  cap <= 4096 and row widths that are multiples of 4 floats, else
        MlhotError."""
        fn = self._fn("rows_compact", "mlhot_rows_compact")
        srcs = list(srcs)
        if not 1 <= len(srcs) <= self.ROWS_COMPACT_SETS:
            raise MlhotError(f"rows_compact takes 1 .. {self.ROWS_COMPACT_SETS} row sets per call (got {len(srcs)})")
        if not isinstance(plan, torch.Tensor) or plan.dtype != torch.int32 or plan.dim() != 2 or not plan.is_cuda:
            raise MlhotError("rows_compact: plan must be an int32 [T, cap] tensor on the GPU")
        T, cap = plan.shape
        for k, x in enumerate(srcs):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 3 or tuple(x.shape[:2]) != (T, cap) or x.device != plan.device:
                raise MlhotError(f"rows_compact: row set {k} must be fp32 [T={T}, cap={cap}, ...] on {plan.device}")
        _chk(plan, *srcs)
        outs = [torch.empty_like(x) for x in srcs]
        n = len(srcs)
        self._rc(fn((C.c_void_p * n)(*[x.data_ptr() for x in srcs]), (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                    (C.c_int * n)(*[x[0, 0].numel() for x in srcs]), n, _ptr(plan), T, cap, _stream(plan)), "mlhot_rows_compact")
        return outs

    # ---- per-shot rows gathered from several sources (csrc/rows_gather.h) ---------------------------
    ROWS_GATHER_SETS = 2     # row sets per mlhot_rows_gather call
    ROWS_GATHER_SOURCES = 8  # sources per call

    def rows_gather(self, sources, plan, T, cap):
        """sources[j]: the 1 .. 2 row sets of source j, fp32 [T_j, cap_j, ...] each (the same trailing shape per set in every source;
        T_j and cap_j are the source's own), 1 .. 8 sources; plan int32 [T, cap, 2] on their device = (source, flat row t_j * cap_j +
        s_j in it) -> new tensors [T, cap, ...], one per row set: row s of task t is the named row, a row of exact zeros where the
        source or the row is out of range ((-1, -1) is the fill).  ONE launch (rows.gather); the sources are only read.  cap <= 4096
        and row widths that are multiples of 4 floats, else MlhotError."""
        fn = self._fn("rows_gather", "mlhot_rows_gather")
        sources = [list(src) for src in sources]
        if not 1 <= len(sources) <= self.ROWS_GATHER_SOURCES:
            raise MlhotError(f"rows_gather takes 1 .. {self.ROWS_GATHER_SOURCES} sources per call (got {len(sources)})")
        n = len(sources[0])
        if not 1 <= n <= self.ROWS_GATHER_SETS or any(len(src) != n for src in sources):
            raise MlhotError(f"rows_gather takes 1 .. {self.ROWS_GATHER_SETS} row sets, the same number from every source (got {[len(src) for src in sources]})")
        if not isinstance(plan, torch.Tensor) or plan.dtype != torch.int32 or tuple(plan.shape) != (T, cap, 2) or not plan.is_cuda:
            raise MlhotError(f"rows_gather: plan must be an int32 [T={T}, cap={cap}, 2] tensor on the GPU")
        for j, src in enumerate(sources):
            for k, x in enumerate(src):
                if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 3 or x.device != plan.device
                        or x.shape[:2] != src[0].shape[:2] or x.shape[2:] != sources[0][k].shape[2:]):
                    raise MlhotError(f"rows_gather: row set {k} of source {j} must be fp32 [T_j, cap_j, {', '.join(map(str, sources[0][k].shape[2:]))}] "
                                     f"on {plan.device}")
        _chk(plan, *[x for src in sources for x in src])
        outs = [torch.empty(T, cap, *x.shape[2:], dtype=torch.float32, device=plan.device) for x in sources[0]]
        ns = len(sources)
        self._rc(fn((C.c_void_p * (n * ns))(*[sources[j][k].data_ptr() for k in range(n) for j in range(ns)]),
                    (C.c_int64 * ns)(*[src[0].shape[0] * src[0].shape[1] for src in sources]), ns, (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                    (C.c_int * n)(*[x[0, 0].numel() for x in sources[0]]), n, _ptr(plan), T, cap, _stream(plan)), "mlhot_rows_gather")
        return outs

    # ---- prefix sweep beyond 32 context shots (csrc/favor_prefix_long.h) --------------------------
    def favor_prefix_long_supported(self, T, H, Nq, Nc, d, m, K):
        """Whether mlhot_favor_prefix_long_fwd serves these dimensions and this number of prefixes."""
        return bool(self._fn("favor_prefix_long_fwd", "mlhot_favor_prefix_long_supported")(T, H, Nq, Nc, d, m, K))

    def favor_prefix_long_workspace_bytes(self, T, H, Nq, Nc, d, m, K):
        """Workspace bytes of mlhot_favor_prefix_long_fwd; 0 for a call it does not serve."""
        return self._fn("favor_prefix_long_fwd", "mlhot_favor_prefix_long_workspace_bytes")(T, H, Nq, Nc, d, m, K)

    def favor_prefix_long_fwd(self, q, k, v, proj, ks, lens=None, out=None):
        """q [T,Nq,H,d], k/v [T,Nc,H,d], proj [m,d], ks (host ints, strictly increasing in 1..Nc, at most 64) -> out [K,T,Nq,d*H]:
        out[i] = favor_fwd on the first ks[i] shots.  lens [T] int32 on q's device or None: task t's context is its first lens[t]
        shots (values 1..Nc are the caller's to check); rows behind it of k and v are never read.  Forward only."""
        fn = self._fn("favor_prefix_long_fwd", "mlhot_favor_prefix_long_fwd")
        for name, t in (("q", q), ("k", k), ("v", v)):
            if t.dtype != torch.float32 or t.dim() != 4:
                raise MlhotError(f"favor_prefix_long_fwd: {name} must be fp32 [T, N, H, d], got {t.dtype} {tuple(t.shape)}")
        T, Nq, H, d = q.shape
        Nc = k.shape[1]
        if tuple(k.shape) != (T, Nc, H, d) or v.shape != k.shape or proj.dtype != torch.float32 or proj.dim() != 2 or proj.shape[1] != d:
            raise MlhotError(f"favor_prefix_long_fwd: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, proj {tuple(proj.shape)} do not fit together")
        if any(t.device != q.device for t in (k, v, proj)):
            raise MlhotError("favor_prefix_long_fwd: q, k, v and proj must lie on one device")
        ks = [int(x) for x in ks]
        K, m = len(ks), proj.shape[0]
        if not ks or any(x < 1 or x > Nc for x in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
            raise MlhotError(f"favor_prefix_long_fwd: ks must be strictly increasing in 1..Nc = {Nc}, got {ks}")
        if lens is not None and (lens.dtype != torch.int32 or tuple(lens.shape) != (T,) or lens.device != q.device):
            raise MlhotError(f"favor_prefix_long_fwd: lens must be int32 [{T}] on {q.device}, got {lens.dtype} {tuple(lens.shape)} on {lens.device}")
        wb = self.favor_prefix_long_workspace_bytes(T, H, Nq, Nc, d, m, K)
        if not wb:
            raise MlhotError(f"favor_prefix_long_fwd serves d % 16 == 0, 16 <= d <= 256, 16 <= m <= 1536, 1 <= K <= 64, Nq, Nc >= 1 "
                             f"(got Nq={Nq} Nc={Nc} d={d} m={m} K={K})")
        if out is None:
            out = torch.empty(K, T, Nq, d * H, device=q.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (K, T, Nq, d * H) or out.device != q.device or not out.is_contiguous():
            raise MlhotError(f"favor_prefix_long_fwd: out must be contiguous fp32 {(K, T, Nq, d * H)} on {q.device}")
        _chk(q, k, v, proj, *([lens] if lens is not None else []))
        ws = self._bytes(wb, q)
        self._rc(fn(_ptr(q), _ptr(k), _ptr(v), _ptr(proj), (C.c_int32 * K)(*ks), K, _ptr(lens) if lens is not None else None, T, H, Nq, Nc, d, m,
                    _ptr(out), _ptr(ws), ws.numel(), _stream(q)), "mlhot_favor_prefix_long_fwd")
        return out

    @staticmethod
    def _staged(call, exchange, direction):
        """Run `call(stage, xchg_ptr)` as the two staged halves around the caller's collective (include/mlhot.h, "strict sharded
        parity"): exchange = (object with forward(x) / backward(x), x = 4 floats on the device)."""
        ex, x = exchange
        _chk(x)
        call(0, _ptr(x))
        (ex.forward if direction == "fwd" else ex.backward)(x)
        call(1, _ptr(x))

    def favor_linear_supported(self, T, H, Nq, Nc, d, m):
        """Whether the linear-form route of favor_fwd / favor_bwd (option "favor_linear", csrc/favor_linear.h) serves these dimensions:
        the envelope alone, whatever the option says."""
        return bool(self._fn("favor_linear_supported", "mlhot_favor_linear_supported")(T, H, Nq, Nc, d, m))

    def favor_fwd(self, q, k, v, proj, exchange=None):
        """q [T,Nq,H,d], k/v [T,Nc,H,d], proj [m,d] -> out [T,Nq,d*H] (merged order), ws"""
        _chk(q, k, v, proj)
        T, Nq, H, d = q.shape
        Nc, m = k.shape[1], proj.shape[0]
        out = torch.empty(T, Nq, d * H, device=q.device)
        wb = self.c.mlhot_favor_ws_bytes(T, H, Nq, Nc, d, m)
        ws = self._bytes(wb, q)
        if exchange is not None:
            self._staged(lambda st, xp: self._rc(self.c.mlhot_favor_fwd_staged(
                _ptr(q), _ptr(k), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(ws), wb, st, xp, _stream(q)),
                "mlhot_favor_fwd_staged"), exchange, "fwd")
            return out, ws
        self._rc(self.c.mlhot_favor_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(ws), wb, _stream(q)),
                 "mlhot_favor_fwd")
        return out, ws

    def favor_bwd(self, q, k, v, proj, out, dout, ws, exchange=None):
        _chk(dout)
        T, Nq, H, d = q.shape
        Nc, m = k.shape[1], proj.shape[0]
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        if exchange is not None:
            self._staged(lambda st, xp: self._rc(self.c.mlhot_favor_bwd_staged(
                _ptr(q), _ptr(k), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(dout), _ptr(dq), _ptr(dk), _ptr(dv),
                _ptr(ws), ws.numel(), st, xp, _stream(q)), "mlhot_favor_bwd_staged"), exchange, "bwd")
            return dq, dk, dv
        self._rc(self.c.mlhot_favor_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(proj), T, H, Nq, Nc, d, m, _ptr(out), _ptr(dout),
                                        _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), ws.numel(), _stream(q)), "mlhot_favor_bwd")
        return dq, dk, dv

    # ---- losses --------------------------------------------------------------------------------
    def loss_fwd(self, kind, mu, gt):
        _chk(mu, gt)
        rows = mu.numel() // mu.shape[-1]
        loss = torch.empty((), device=mu.device)
        self._rc(self.c.mlhot_loss_fwd(LOSS[kind], _ptr(mu), _ptr(gt), rows, mu.shape[-1], gt.shape[-1], _ptr(loss), _stream(mu)), "mlhot_loss_fwd")
        return loss

    def loss_prefix_fwd(self, kind, mu, gt):
        """mu [P, ..., y_dim], gt [..., gt_dim] shared by the prefixes -> loss [P]: loss[p] = loss_fwd(kind, mu[p], gt), same bits, one launch."""
        fn = self._fn("loss_prefix_fwd", "mlhot_loss_prefix_fwd")
        if kind not in LOSS:
            raise MlhotError(f"loss_prefix_fwd: kind must be one of {sorted(LOSS)}, got {kind!r}")
        if mu.dim() < 2 or mu.numel() == 0 or gt.numel() == 0:
            raise MlhotError(f"loss_prefix_fwd expects mu [P, ..., y_dim], got {tuple(mu.shape)}")
        _chk(mu, gt)
        P, y_dim = mu.shape[0], mu.shape[-1]
        rows = mu.numel() // (P * y_dim)
        if gt.numel() // gt.shape[-1] != rows or mu.dtype != torch.float32 or gt.dtype != torch.float32:
            raise MlhotError(f"loss_prefix_fwd: labels {tuple(gt.shape)} do not fit mu {tuple(mu.shape)} (fp32, one label row per row of a prefix)")
        loss = torch.empty(P, device=mu.device)
        self._rc(fn(LOSS[kind], _ptr(mu), _ptr(gt), P, rows, y_dim, gt.shape[-1], _ptr(loss), _stream(mu)), "mlhot_loss_prefix_fwd")
        return loss

    def loss_bwd(self, kind, mu, gt, dloss):
        _chk(dloss)
        rows = mu.numel() // mu.shape[-1]
        dmu = torch.empty_like(mu)
        self._rc(self.c.mlhot_loss_bwd(LOSS[kind], _ptr(mu), _ptr(gt), rows, mu.shape[-1], gt.shape[-1], _ptr(dloss), _ptr(dmu), _stream(mu)),
                 "mlhot_loss_bwd")
        return dmu

    def loss_plus_fwd(self, kind, mu, gt, x, alpha):
        """loss(kind; mu, gt) + alpha * x (x a device scalar: the KL term) in the loss's launch; the total, a device scalar."""
        _chk(mu, gt, x)
        if x.numel() != 1:
            raise MlhotError(f"loss_plus_fwd: x must be a scalar, got {tuple(x.shape)}")
        rows = mu.numel() // mu.shape[-1]
        total = torch.empty((), device=mu.device)
        self._rc(self.c.mlhot_loss_plus_fwd(LOSS[kind], _ptr(mu), _ptr(gt), rows, mu.shape[-1], gt.shape[-1], _ptr(x), float(alpha), None,
                                            _ptr(total), _stream(mu)), "mlhot_loss_plus_fwd")
        return total

    def loss_plus_bwd(self, kind, mu, gt, dtotal, alpha, need_dx=True):
        """(d mu, d x) of loss_plus_fwd for the upstream scalar dtotal; d x = alpha * dtotal (None when not needed)."""
        _chk(dtotal)
        rows = mu.numel() // mu.shape[-1]
        dmu = torch.empty_like(mu)
        dx = torch.empty((), device=mu.device) if need_dx else None
        self._rc(self.c.mlhot_loss_plus_bwd(LOSS[kind], _ptr(mu), _ptr(gt), rows, mu.shape[-1], gt.shape[-1], _ptr(dtotal), float(alpha),
                                            _ptr(dmu), _ptr(dx) if dx is not None else None, _stream(mu)), "mlhot_loss_plus_bwd")
        return dmu, dx

    # ---- batch ingest ---------------------------------------------------------------------------
    def ingest_u8_nhwc(self, src, out=None, div=255.0):
        """src: uint8 [..., H, W, C] on the device (channel-last, as the data loaders hold images) ->
        fp32 [..., C, H, W] = src / div (dataset/shapenet_1d.py:189-190 + utils/utils.py:26-30)."""
        n_img, H, W, Cc = _nhwc("ingest_u8_nhwc", src)
        _chk(src, out)
        out = _ingest_out("ingest_u8_nhwc", src, out)
        self._rc(self.c.mlhot_ingest_u8_nhwc(_ptr(src), _ptr(out), n_img, H, W, Cc, float(div), _stream(src)), "mlhot_ingest_u8_nhwc")
        return out

    @staticmethod
    def _table_args(wrapper, device, n_img, records, ints, luts, colour_tabs=None, pre_op=0):
        """The table of an augmenting ingest of n_img images on `device`: records int32 [n_img, ints], luts uint8 [n, 256] or None, and
        for the image entries colour_tabs uint8 [COLOUR_TABS_BYTES] or None and pre_op; -> n_luts."""
        if records.dtype != torch.int32 or records.numel() != n_img * ints or records.device != device:
            raise MlhotError(f"{wrapper}: records must be int32 [{n_img}, {ints}] on {device}")
        if luts is not None and (luts.dtype != torch.uint8 or luts.dim() != 2 or luts.shape[1] != 256 or luts.device != device):
            raise MlhotError(f"{wrapper}: luts must be uint8 [n, 256] on {device}")
        if colour_tabs is not None and (colour_tabs.dtype != torch.uint8 or colour_tabs.numel() != COLOUR_TABS_BYTES
                                        or colour_tabs.device != device):
            raise MlhotError(f"{wrapper}: colour_tabs must be uint8 [{COLOUR_TABS_BYTES}] on {device}")
        if pre_op not in (0, 1):
            raise MlhotError(f"{wrapper}: pre_op is 0 or 1, got {pre_op!r}")
        _chk(records, luts, colour_tabs)
        return 0 if luts is None else luts.shape[0]

    def augment_ingest_u8(self, src, records, luts=None, out=None, div=255.0):
        """ingest_u8_nhwc with the 1D loaders' data augmentation in front (csrc/augment.h, include/mlhot.h mlhot_aug_record):
        src uint8 [..., H, W, 1] -> fp32 [..., 1, H, W].  records: int32 [n_img, 32] (mlhot.augment.Sampler), luts: uint8
        [n_luts, 256] or None; both on src's device."""
        n_img, H, W, Cc = _nhwc("augment_ingest_u8", src)
        fn = self._fn("augment_ingest_u8", "mlhot_augment_ingest_u8")
        n_luts = self._table_args("augment_ingest_u8", src.device, n_img, records, AUG_RECORD_BYTES // 4, luts)
        _chk(src, out)
        out = _ingest_out("augment_ingest_u8", src, out)
        self._rc(fn(_ptr(src), _ptr(out), n_img, H, W, Cc, float(div), _ptr(records), _ptr(luts) if n_luts else None, n_luts, _stream(src)),
                 "mlhot_augment_ingest_u8")
        return out

    def augment_ingest_u8_img(self, src, records, luts=None, colour_tabs=None, out=None, pre_op=0, div=255.0, div2=1.0):
        """The image tasks' augmenting ingest (csrc/augment_img.h, include/mlhot.h mlhot_aug_record_img): src uint8 [..., H, W, C]
        (C = 3 with H, W <= 64, or C = 1 with H, W <= 128) -> fp32 [..., C, H, W] = augmented byte / div / div2.  records: int32
        [n_img, 40] (mlhot.augment.ImageSampler), luts: uint8 [n_luts, 256] or None, colour_tabs: uint8 [12896]
        (mlhot.augment.colour_tables(device)) or None; all on src's device."""
        n_img, H, W, Cc = _nhwc("augment_ingest_u8_img", src)
        fn = self._fn("augment_ingest_u8_img", "mlhot_augment_ingest_u8_img")
        n_luts = self._table_args("augment_ingest_u8_img", src.device, n_img, records, AUG_IMG_RECORD_BYTES // 4, luts, colour_tabs, pre_op)
        _chk(src, out)
        out = _ingest_out("augment_ingest_u8_img", src, out)
        self._rc(fn(_ptr(src), _ptr(out), n_img, H, W, Cc, int(pre_op), float(div), float(div2), _ptr(records), _ptr(luts) if n_luts else None,
                    n_luts, _ptr(colour_tabs), _stream(src)), "mlhot_augment_ingest_u8_img")
        return out

    # ---- resident image pools (csrc/pool_ingest.h): RGBA uint8 [N, H, W, 4] with a bank, or grey uint8 [N, H, W, 1] (pool1) --------
    @staticmethod
    def _pool_args(wrapper, pool, channels, ids, out, bank=None, bg=None):
        """Shapes, dtypes and devices of a call on a pool of `channels` (4: RGBA, delivered as 3; 1: grey, which has neither bank nor bg);
        -> (n_pool, n_bank, n_img, H, W, bg, out).  Indices that live on the host (the host build) are range-checked here; device
        indices are trusted - BatchIngest.stage_ids checks them before it ships them."""
        rgba = channels == 4
        if pool.dtype != torch.uint8 or pool.dim() != 4 or pool.shape[-1] != channels:
            raise MlhotError(f"{wrapper}: the pool must be uint8 [N, H, W, {channels}] ({'RGBA, channel-last' if rgba else 'single-channel'}), "
                             f"got {pool.dtype} {tuple(pool.shape)}")
        n_pool, H, W, _ = pool.shape
        if bank is not None and (bank.dtype != torch.uint8 or bank.dim() != 4 or tuple(bank.shape[1:]) != (H, W, 3) or bank.device != pool.device):
            raise MlhotError(f"{wrapper}: the bank must be uint8 [B, {H}, {W}, 3] on {pool.device}, got {bank.dtype} {tuple(bank.shape)}")
        n_bank = 0 if bank is None else bank.shape[0]
        if ids.dtype != torch.int32 or ids.device != pool.device:
            raise MlhotError(f"{wrapper}: ids must be int32 on {pool.device}")
        n_img = ids.numel()
        if bg is None and rgba:
            bg = torch.full((n_img,), -1, dtype=torch.int32, device=pool.device)
        if bg is not None and (bg.dtype != torch.int32 or bg.numel() != n_img or bg.device != pool.device):
            raise MlhotError(f"{wrapper}: bg must be int32 [{n_img}] on {pool.device}")
        if not ids.is_cuda:
            from .ingest import check_pool_indices
            check_pool_indices(ids.numpy(), (torch.full(tuple(ids.shape), -1) if bg is None else bg).numpy(), n_pool, n_bank)
        shape = (*ids.shape, 3 if rgba else 1, H, W)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=pool.device)
        elif out.dtype != torch.float32 or out.numel() != math.prod(shape) or out.device != pool.device:
            raise MlhotError(f"{wrapper}: out must be fp32 {shape} on {pool.device}")
        _chk(pool, ids, bank, bg, out)
        return n_pool, n_bank, n_img, H, W, bg, out

    def pool_ingest_u8(self, pool, ids, bank=None, bg=None, out=None, div=255.0):
        """Images `ids` (int32 [...]) of the resident pool (uint8 [N, H, W, 4]) with bank[bg] (uint8 [B, H, W, 3]; bg int32, -1 = none)
        behind every pixel whose alpha is 255 -> fp32 [..., 3, H, W] = byte / div (include/mlhot.h mlhot_pool_ingest_u8)."""
        fn = self._fn("pool_ingest_u8", "mlhot_pool_ingest_u8")
        n_pool, n_bank, n_img, H, W, bg, out = self._pool_args("pool_ingest_u8", pool, 4, ids, out, bank, bg)
        self._rc(fn(_ptr(pool), n_pool, _ptr(ids), _ptr(bank) if n_bank else None, n_bank, _ptr(bg), _ptr(out), n_img, H, W, float(div),
                    _stream(pool)), "mlhot_pool_ingest_u8")
        return out

    def pool_augment_ingest_u8_img(self, pool, ids, records, bank=None, bg=None, luts=None, colour_tabs=None, out=None, div=255.0):
        """pool_ingest_u8 with the shapenet_3d image augmentation behind the composition (augment_ingest_u8_img's records int32
        [n_img, 40], luts and colour tables; C = 3, pre_op = 0); H, W <= 64."""
        fn = self._fn("pool_augment_ingest_u8_img", "mlhot_pool_augment_ingest_u8_img")
        n_pool, n_bank, n_img, H, W, bg, out = self._pool_args("pool_augment_ingest_u8_img", pool, 4, ids, out, bank, bg)
        n_luts = self._table_args("pool_augment_ingest_u8_img", pool.device, n_img, records, AUG_IMG_RECORD_BYTES // 4, luts, colour_tabs)
        self._rc(fn(_ptr(pool), n_pool, _ptr(ids), _ptr(bank) if n_bank else None, n_bank, _ptr(bg), _ptr(out), n_img, H, W, float(div),
                    _ptr(records), _ptr(luts) if n_luts else None, n_luts, _ptr(colour_tabs), _stream(pool)),
                 "mlhot_pool_augment_ingest_u8_img")
        return out

    def pool1_ingest_u8(self, pool, ids, out=None, div=255.0):
        """Images `ids` (int32 [...]) of the resident grey pool (uint8 [N, H, W, 1]) -> fp32 [..., 1, H, W] = byte / div: the bits of
        ingest_u8_nhwc(pool[ids]) (include/mlhot.h mlhot_pool1_ingest_u8)."""
        fn = self._fn("pool1_ingest_u8", "mlhot_pool1_ingest_u8")
        n_pool, _, n_img, H, W, _, out = self._pool_args("pool1_ingest_u8", pool, 1, ids, out)
        self._rc(fn(_ptr(pool), n_pool, _ptr(ids), _ptr(out), n_img, H, W, float(div), _stream(pool)), "mlhot_pool1_ingest_u8")
        return out

    def pool1_augment_ingest_u8(self, pool, ids, records, luts=None, out=None, div=255.0):
        """augment_ingest_u8 (the 1D sequences; records int32 [n_img, 32]) on images `ids` of the grey pool; H, W <= 128."""
        fn = self._fn("pool1_augment_ingest_u8", "mlhot_pool1_augment_ingest_u8")
        n_pool, _, n_img, H, W, _, out = self._pool_args("pool1_augment_ingest_u8", pool, 1, ids, out)
        n_luts = self._table_args("pool1_augment_ingest_u8", pool.device, n_img, records, AUG_RECORD_BYTES // 4, luts)
        self._rc(fn(_ptr(pool), n_pool, _ptr(ids), _ptr(out), n_img, H, W, float(div), _ptr(records), _ptr(luts) if n_luts else None, n_luts,
                    _stream(pool)), "mlhot_pool1_augment_ingest_u8")
        return out

    def pool1_augment_ingest_u8_img(self, pool, ids, records, luts=None, colour_tabs=None, out=None, pre_op=0, div=255.0, div2=1.0):
        """augment_ingest_u8_img with C = 1 (Distractor's sequence; records int32 [n_img, 40], pre_op, div, div2 as there) on images
        `ids` of the grey pool; H, W <= 128."""
        fn = self._fn("pool1_augment_ingest_u8_img", "mlhot_pool1_augment_ingest_u8_img")
        n_pool, _, n_img, H, W, _, out = self._pool_args("pool1_augment_ingest_u8_img", pool, 1, ids, out)
        n_luts = self._table_args("pool1_augment_ingest_u8_img", pool.device, n_img, records, AUG_IMG_RECORD_BYTES // 4, luts, colour_tabs, pre_op)
        self._rc(fn(_ptr(pool), n_pool, _ptr(ids), _ptr(out), n_img, H, W, int(pre_op), float(div), float(div2), _ptr(records),
                    _ptr(luts) if n_luts else None, n_luts, _ptr(colour_tabs), _stream(pool)), "mlhot_pool1_augment_ingest_u8_img")
        return out

    # ---- fused Adam over flat buffers -------------------------------------------------------------
    def adam_step(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, grad_scale, step):
        _chk(param, grad, exp_avg, exp_avg_sq)
        n = param.numel()
        if not (grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == n):
            raise MlhotError("adam_step: buffers differ in size")
        self._rc(self.c.mlhot_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, lr, beta1, beta2, eps,
                                        weight_decay, grad_scale, int(step), _stream(param)), "mlhot_adam_step")

    def adam_step_counter(self, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, grad_scale, step_counter):
        """adam_step with the step count in device memory (int32 tensor of one element, incremented by the call)."""
        _chk(param, grad, exp_avg, exp_avg_sq, step_counter)
        n = param.numel()
        if not (grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == n) or step_counter.dtype != torch.int32:
            raise MlhotError("adam_step_counter: buffers differ in size, or the counter is not int32")
        self._rc(self.c.mlhot_adam_step_counter(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, lr, beta1, beta2, eps,
                                                weight_decay, grad_scale, _ptr(step_counter), _stream(param)), "mlhot_adam_step_counter")

    def np_grads_layout(self, dims):
        """(total floats, {state_dict key: float offset}) of the library's flat gradient buffer for `dims`."""
        offs = NpGrads()
        total = self.c.mlhot_np_grads_flat_layout(C.byref(dims), C.byref(offs))
        pm = vanilla_param_map(dims.n_hidden, dims.agg_mode == AGG["baco"], dims.agg_mode == AGG["attention"])
        return total, {key: (_get(offs, path) or 0) // 4 for path, key in pm}

    # ---- whole vanilla model -------------------------------------------------------------------
    @staticmethod
    def np_dims(T, Nc, Nq, label_dim, y_dim, dim_w, dim_r, dim_z, hidden, dec_hidden, agg_mode, out_tanh, m_feat):
        d = NpDims()
        d.T, d.Nc, d.Nq, d.label_dim, d.y_dim = T, Nc, Nq, label_dim, y_dim
        d.dim_w, d.dim_r, d.dim_z, d.n_hidden, d.dec_hidden = dim_w, dim_r, dim_z, len(hidden), dec_hidden
        for i, h in enumerate(hidden):
            d.hidden[i] = h
        d.agg_mode, d.out_tanh, d.m_feat = AGG[agg_mode], int(out_tanh), m_feat
        return d

    @staticmethod
    def np_struct(cls, dims, tensors, proj=None):
        """tensors: dict state_dict-key -> tensor (params or grads)"""
        s = cls()
        pm = vanilla_param_map(dims.n_hidden, dims.agg_mode == AGG["baco"], dims.agg_mode == AGG["attention"])
        for path, key in pm:
            _set(s, path, tensors[key].data_ptr())
        if proj is not None:
            s.proj = proj.data_ptr()
        return s

    def np_vanilla_fwd(self, dims, params, ctx_x, ctx_y, qry_x, proj=None, exchange=None):
        _chk(ctx_x, ctx_y, qry_x, proj, *params.values())
        mu = torch.empty(dims.T, dims.Nq, dims.y_dim, device=qry_x.device)
        saved = self._bytes(self.c.mlhot_np_saved_bytes(C.byref(dims)), qry_x)
        sb = self.c.mlhot_np_scratch_bytes(C.byref(dims))
        scratch = self._bytes(sb, qry_x)
        ps = self.np_struct(NpParams, dims, params, proj)
        if exchange is not None:
            self._staged(lambda st, xp: self._rc(self.c.mlhot_np_vanilla_fwd_staged(
                C.byref(dims), C.byref(ps), _ptr(ctx_x), _ptr(ctx_y), _ptr(qry_x), _ptr(mu), _ptr(saved), _ptr(scratch), sb, st, xp,
                _stream(qry_x)), "mlhot_np_vanilla_fwd_staged"), exchange, "fwd")
            return mu, saved, scratch
        self._rc(self.c.mlhot_np_vanilla_fwd(C.byref(dims), C.byref(ps), _ptr(ctx_x), _ptr(ctx_y), _ptr(qry_x), _ptr(mu),
                                             _ptr(saved), _ptr(scratch), sb, _stream(qry_x)), "mlhot_np_vanilla_fwd")
        return mu, saved, scratch

    # ---- cached context of the vanilla family (csrc/np_query.h) ------------------------------------------------
    def np_query_supported(self, dims):
        """Whether mlhot_np_query_fwd serves these dimensions (dims.Nq is not looked at; pointers are checked per call)."""
        return bool(self._fn("np_query_supported", "mlhot_np_query_supported")(C.byref(dims)))

    def np_query_fwd(self, dims, params, x_qry, key_state=None, vh=None, z=None, proj=None):
        """x_qry [T, Nq, dim_w] (the encoder's target rows) -> mu [T, Nq, y_dim] in ONE launch, any Nq >= 1, against a conditioned
        context: key_state (favor_keys_fwd's, for 8 heads) + vh [T, Nc, 8, dim_w] + proj for an attention model with dims.Nc > 0,
        z [T, dim_z] otherwise.  params: state_dict key -> tensor; the query-side ones are read (_W_q, _W, r_to_z, decoder0)."""
        fn = self._fn("np_query_fwd", "mlhot_np_query_fwd")
        attend = dims.agg_mode == AGG["attention"] and dims.Nc > 0
        if x_qry.dtype != torch.float32 or x_qry.dim() != 3 or x_qry.shape[0] != dims.T or x_qry.shape[1] < 1 or x_qry.shape[2] != dims.dim_w:
            raise MlhotError(f"np_query_fwd: x_qry must be fp32 [T = {dims.T}, Nq >= 1, dim_w = {dims.dim_w}], got {x_qry.dtype} {tuple(x_qry.shape)}")
        if attend:
            want = (dims.T, dims.Nc, HEADS, dims.dim_w)
            if key_state is None or vh is None or proj is None or z is not None or vh.dtype != torch.float32 or tuple(vh.shape) != want or \
                    proj.dtype != torch.float32 or tuple(proj.shape) != (dims.m_feat, dims.dim_w) or key_state.dtype != torch.uint8:
                raise MlhotError(f"np_query_fwd: the attention takes key_state (uint8), vh fp32 {want} and proj fp32 [{dims.m_feat}, {dims.dim_w}], no z")
            if key_state.numel() < self.favor_keys_bytes(dims.T, HEADS, dims.Nc, dims.dim_w, dims.m_feat):
                raise MlhotError("np_query_fwd: key_state is smaller than mlhot_favor_keys_bytes for these dimensions")
        elif z is None or key_state is not None or vh is not None or z.dtype != torch.float32 or tuple(z.shape) != (dims.T, dims.dim_z):
            raise MlhotError(f"np_query_fwd: without attention or context the call takes z fp32 [{dims.T}, {dims.dim_z}], no key_state / vh")
        ps = NpParams()
        used = []
        for path, key in vanilla_param_map(dims.n_hidden, False, attend):
            if path[0] in ("dec_w", "dec_b") or (attend and path[0] in ("r2z_w", "r2z_b", "wq_w", "wq_b", "wo_w", "wo_b")):
                _set(ps, path, params[key].data_ptr())
                used.append(params[key])
        if attend:
            ps.proj = proj.data_ptr()
        live = [t for t in (x_qry, key_state, vh, z, proj, *used) if t is not None]
        if any(t.device != x_qry.device for t in live):
            raise MlhotError("np_query_fwd: x_qry, the state and the parameters must lie on one device")
        _chk(*live)
        mu = torch.empty(dims.T, x_qry.shape[1], dims.y_dim, device=x_qry.device)
        self._rc(fn(C.byref(dims), C.byref(ps), _ptr(x_qry), x_qry.shape[1], _ptr(key_state), _ptr(vh), _ptr(z), _ptr(mu), _stream(x_qry)),
                 "mlhot_np_query_fwd")
        return mu

    # ---- the same tail against a FAVOR+ summary state (csrc/np_query_summary.h) -------------------------------
    def np_query_summary_supported(self, dims):
        """Whether mlhot_np_query_summary_fwd serves these dimensions (dims.Nc and dims.Nq are not looked at)."""
        return bool(self._fn("np_query_summary_supported", "mlhot_np_query_summary_supported")(C.byref(dims)))

    def np_query_summary_fwd(self, dims, params, x_qry, summary_state, proj, out=None):
        """x_qry [T, Nq, dim_w] (the encoder's target rows) -> mu [T, Nq, y_dim] in ONE launch, any Nq >= 1, against summary_state:
        favor_summary_absorb's / _merge's / _gather's state (uint8) for T tasks, 8 heads, dim_w and proj [m, dim_w], whatever number of
        shots it holds (every task at least one: the caller's to check).  params: state_dict key -> tensor; the query-side ones are
        read (_W_q, _W, r_to_z, decoder0).  `out`: a contiguous fp32 [T, Nq, y_dim] tensor to write into (default: a new one)."""
        fn = self._fn("np_query_summary_fwd", "mlhot_np_query_summary_fwd")
        if x_qry.dtype != torch.float32 or x_qry.dim() != 3 or x_qry.shape[0] != dims.T or x_qry.shape[1] < 1 or x_qry.shape[2] != dims.dim_w:
            raise MlhotError(f"np_query_summary_fwd: x_qry must be fp32 [T = {dims.T}, Nq >= 1, dim_w = {dims.dim_w}], got {x_qry.dtype} {tuple(x_qry.shape)}")
        if summary_state is None or proj is None or summary_state.dtype != torch.uint8 or proj.dtype != torch.float32 or \
                tuple(proj.shape) != (dims.m_feat, dims.dim_w):
            raise MlhotError(f"np_query_summary_fwd takes summary_state (uint8) and proj fp32 [{dims.m_feat}, {dims.dim_w}]")
        if not self.np_query_summary_supported(dims):
            raise MlhotError(f"np_query_summary_fwd serves attention models with dim_w % 16 == 0, dim_w <= 64, dim_z % 4 == 0, dim_z <= 64, dec_hidden % 4 == 0, "
                             f"dec_hidden <= 128, y_dim <= 16, dim_r == dim_w, 16 <= m <= 272 (got dim_w={dims.dim_w} dim_r={dims.dim_r} dim_z={dims.dim_z} "
                             f"dec_hidden={dims.dec_hidden} y_dim={dims.y_dim} m={dims.m_feat})")
        nb = self.favor_summary_bytes(dims.T, HEADS, dims.dim_w, dims.m_feat)
        if not nb or summary_state.numel() < nb:
            raise MlhotError(f"np_query_summary_fwd: summary_state holds {summary_state.numel()} bytes, mlhot_favor_summary_bytes asks for {nb} "
                             f"(T={dims.T}, 8 heads, d={dims.dim_w}, m={dims.m_feat})")
        ps = NpParams()
        used = []
        for path, key in vanilla_param_map(dims.n_hidden, False, True):
            if path[0] in ("dec_w", "dec_b", "r2z_w", "r2z_b", "wq_w", "wq_b", "wo_w", "wo_b"):
                _set(ps, path, params[key].data_ptr())
                used.append(params[key])
        ps.proj = proj.data_ptr()
        shape = (dims.T, x_qry.shape[1], dims.y_dim)
        if out is None:
            out = torch.empty(shape, device=x_qry.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != shape:
            raise MlhotError(f"np_query_summary_fwd: out must be fp32 {shape}, got {out.dtype} {tuple(out.shape)}")
        live = [x_qry, summary_state, proj, out, *used]
        if any(t.device != x_qry.device for t in live):
            raise MlhotError("np_query_summary_fwd: x_qry, the state, the parameters and out must lie on one device")
        _chk(*live)
        self._rc(fn(C.byref(dims), C.byref(ps), _ptr(x_qry), x_qry.shape[1], _ptr(summary_state), _ptr(out), _stream(x_qry)), "mlhot_np_query_summary_fwd")
        return out

    # ---- prefix sweep of the vanilla family (csrc/np_prefix.h) -------------------------------------------------
    def np_prefix_supported(self, dims, K):
        """Whether mlhot_np_prefix_fwd serves these dimensions (dims.Nc: all the context shots) for K prefixes."""
        return bool(self._fn("np_prefix_supported", "mlhot_np_prefix_supported")(C.byref(dims), int(K)))

    def np_prefix_fwd(self, dims, params, x_qry, ks, kh=None, vh=None, z=None, proj=None):
        """x_qry [T, Nq, dim_w] -> mu [K, T, Nq, y_dim]: row i is np_query_fwd's result against the first ks[i] of the dims.Nc context
        shots.  ks: host ints, strictly increasing in 1..Nc.  Attention: kh, vh [T, Nc, 8, dim_w] and proj (the key side runs inside
        the call); otherwise z [K, T, dim_z].  params: state_dict key -> tensor, the query-side ones are read."""
        fn = self._fn("np_prefix_fwd", "mlhot_np_prefix_fwd")
        attend = dims.agg_mode == AGG["attention"]
        ks = [int(k) for k in ks]
        K = len(ks)
        if x_qry.dtype != torch.float32 or x_qry.dim() != 3 or x_qry.shape[0] != dims.T or x_qry.shape[1] < 1 or x_qry.shape[2] != dims.dim_w:
            raise MlhotError(f"np_prefix_fwd: x_qry must be fp32 [T = {dims.T}, Nq >= 1, dim_w = {dims.dim_w}], got {x_qry.dtype} {tuple(x_qry.shape)}")
        if not ks or any(k < 1 or k > dims.Nc for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
            raise MlhotError(f"np_prefix_fwd: ks must be strictly increasing in 1..Nc = {dims.Nc}, got {ks}")
        if not self.np_prefix_supported(dims, K):
            raise MlhotError(f"np_prefix_fwd serves 1 <= K <= 32 prefixes of 1 <= Nc <= 32 shots within np_query_fwd's envelope (got K={K} Nc={dims.Nc} "
                             f"dim_w={dims.dim_w} dim_r={dims.dim_r} dim_z={dims.dim_z} dec_hidden={dims.dec_hidden} y_dim={dims.y_dim} m={dims.m_feat})")
        if attend:
            want = (dims.T, dims.Nc, HEADS, dims.dim_w)
            if kh is None or vh is None or proj is None or z is not None or any(t.dtype != torch.float32 or tuple(t.shape) != want for t in (kh, vh)) or \
                    proj.dtype != torch.float32 or tuple(proj.shape) != (dims.m_feat, dims.dim_w):
                raise MlhotError(f"np_prefix_fwd: the attention takes kh, vh fp32 {want} and proj fp32 [{dims.m_feat}, {dims.dim_w}], no z")
        elif z is None or kh is not None or vh is not None or z.dtype != torch.float32 or tuple(z.shape) != (K, dims.T, dims.dim_z):
            raise MlhotError(f"np_prefix_fwd: without attention the call takes z fp32 [{K}, {dims.T}, {dims.dim_z}], no kh / vh")
        ps = NpParams()
        used = []
        for path, key in vanilla_param_map(dims.n_hidden, False, attend):
            if path[0] in ("dec_w", "dec_b") or (attend and path[0] in ("r2z_w", "r2z_b", "wq_w", "wq_b", "wo_w", "wo_b")):
                _set(ps, path, params[key].data_ptr())
                used.append(params[key])
        if attend:
            ps.proj = proj.data_ptr()
        live = [t for t in (x_qry, kh, vh, z, proj, *used) if t is not None]
        if any(t.device != x_qry.device for t in live):
            raise MlhotError("np_prefix_fwd: x_qry, the context rows and the parameters must lie on one device")
        _chk(*live)
        nb = self._fn("np_prefix_fwd", "mlhot_np_prefix_ws_bytes")(C.byref(dims), K)
        ws = self._bytes(nb, x_qry) if attend else None
        mu = torch.empty(K, dims.T, x_qry.shape[1], dims.y_dim, device=x_qry.device)
        self._rc(fn(C.byref(dims), C.byref(ps), _ptr(x_qry), x_qry.shape[1], (C.c_int32 * K)(*ks), K, _ptr(kh), _ptr(vh), _ptr(z), _ptr(mu),
                    _ptr(ws), 0 if ws is None else ws.numel(), _stream(x_qry)), "mlhot_np_prefix_fwd")
        return mu

    def np_vanilla_bwd(self, dims, params, ctx_x, ctx_y, qry_x, mu, dmu, saved, scratch=None, proj=None, exchange=None, loss=None, flat=True):
        """loss: None, or (kind, gt, dloss[, value]) - the loss whose gradient the call takes itself (mlhot_np_vanilla_bwd_loss): the
        gradient of mu is then dmu (may be None) + d loss / d mu * dloss; `value`: None, or the scalar tensor that receives the loss
        VALUE from the same call (what loss_fwd would have written).  flat = False: every gradient is a tensor of its own instead of
        a view of one buffer in the library's flat layout (the tail's slabs then reduce segment by segment)."""
        _chk(dmu, mu)
        if loss is not None and exchange is not None:
            raise MlhotError("np_vanilla_bwd: the staged pass takes dmu, not a loss descriptor")
        # one flat gradient buffer in the library's preferred order; the per-parameter gradients are views of it
        offs = NpGrads()
        total = self.c.mlhot_np_grads_flat_layout(C.byref(dims), C.byref(offs))
        buf = torch.empty(total if flat else 0, dtype=torch.float32, device=qry_x.device)
        pm = vanilla_param_map(dims.n_hidden, dims.agg_mode == AGG["baco"], dims.agg_mode == AGG["attention"])
        grads = {}
        for path, key in pm:
            off = (_get(offs, path) or 0) // 4
            grads[key] = buf[off:off + params[key].numel()].view_as(params[key]) if flat else torch.empty_like(params[key])
        sb = self.c.mlhot_np_scratch_bytes(C.byref(dims))
        if scratch is None or scratch.numel() < sb:
            scratch = self._bytes(sb, qry_x)
        ps = self.np_struct(NpParams, dims, params, proj)
        gs = self.np_struct(NpGrads, dims, grads)
        if exchange is not None:
            self._staged(lambda st, xp: self._rc(self.c.mlhot_np_vanilla_bwd_staged(
                C.byref(dims), C.byref(ps), _ptr(ctx_x), _ptr(ctx_y), _ptr(qry_x), _ptr(mu), _ptr(dmu), C.byref(gs), _ptr(saved),
                _ptr(scratch), sb, st, xp, _stream(qry_x)), "mlhot_np_vanilla_bwd_staged"), exchange, "bwd")
            return grads
        if loss is not None:
            kind, gt, dloss, *rest = loss
            value = rest[0] if rest else None
            _chk(gt, dloss)
            if value is not None:
                _chk(value)
            if gt.numel() % (dims.T * dims.Nq) or LOSS[kind] == LOSS["degree"]:
                raise MlhotError(f"np_vanilla_bwd: loss {kind!r} with labels {tuple(gt.shape)} does not fit mu {tuple(mu.shape)}")
            ld = LossDesc(LOSS[kind], _ptr(gt), gt.numel() // (dims.T * dims.Nq), _ptr(dloss), _ptr(value))
            self._rc(self.c.mlhot_np_vanilla_bwd_loss(C.byref(dims), C.byref(ps), _ptr(ctx_x), _ptr(ctx_y), _ptr(qry_x), _ptr(mu), _ptr(dmu),
                                                      C.byref(ld), C.byref(gs), _ptr(saved), _ptr(scratch), sb, _stream(qry_x)), "mlhot_np_vanilla_bwd_loss")
            return grads
        self._rc(self.c.mlhot_np_vanilla_bwd(C.byref(dims), C.byref(ps), _ptr(ctx_x), _ptr(ctx_y), _ptr(qry_x), _ptr(mu), _ptr(dmu),
                                             C.byref(gs), _ptr(saved), _ptr(scratch), sb, _stream(qry_x)), "mlhot_np_vanilla_bwd")
        return grads
