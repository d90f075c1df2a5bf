"""Numpy statement of mlhot_linear_rows_fwd's row map and of the layer it computes (csrc/linear_rows.h)."""
import numpy as np


def source_rows(M, rep, period):
    """Source row read by each of the M output rows: (i // rep) % period, period 0 = no wrap."""
    i = np.arange(M) // rep
    return i % period if period else i


def gather(x, M, rep, period):
    """The rows of `x` (numpy or torch, [R, k]) the M output rows read, materialised [M, k]."""
    idx = source_rows(M, rep, period)
    return x[idx] if isinstance(x, np.ndarray) else x[idx.tolist()]


def linear_rows_np(sources, w, b, act, M):
    """float64 act([src_0 | src_1] w^T + b); sources: (array [R, k], rep, period)."""
    x = np.concatenate([np.asarray(gather(np.asarray(s, dtype=np.float64), M, rep, period)) for s, rep, period in sources], axis=1)
    y = x @ np.asarray(w, dtype=np.float64).T + (0.0 if b is None else np.asarray(b, dtype=np.float64))
    return np.maximum(y, 0.0) if act == "relu" else np.tanh(y) if act == "tanh" else y
