"""Restatement of the gradient-norm / clipping rule (include/skf.h: skf_segment_norms, skf_adam_step_clipped) in numpy: the sums in
float64, the scales and the gradient the sweep sees in float32, operation by operation.  Shared by the CPU and the GPU tests."""
import numpy as np

CHUNK = 16384       # SKF_SEGMENT_CHUNK: logical elements per work chunk


def entry(offset, rows, cols, row_stride=None, name=None):
    e = {"offset": int(offset), "rows": int(rows), "cols": int(cols), "row_stride": int(cols if row_stride is None else row_stride)}
    if name is not None:
        e["name"] = name
    return e


def view(flat, e):
    """The (rows, cols) view of one entry inside a flat array (no copy; strided entries stay strided)."""
    return np.lib.stride_tricks.as_strided(flat[e["offset"]:], shape=(e["rows"], e["cols"]),
                                           strides=(e["row_stride"] * flat.itemsize, flat.itemsize))


def n_chunks(entries):
    return sum(-(-(e["rows"] * e["cols"]) // CHUNK) for e in entries)


def sum_squares(flat, entries):
    """float64 sum of squares per entry (only the entries' own elements are read)."""
    return np.array([np.sum(np.square(view(flat, e).astype(np.float64))) for e in entries], dtype=np.float64)


def norms(flat, entries, grad_scale=1.0):
    """-> (per-entry norms, global norm) in float64: sqrt of the float64 sums times grad_scale (a float32 factor)."""
    ss = sum_squares(flat, entries)
    gs = np.float64(np.float32(grad_scale))
    return np.sqrt(ss) * gs, np.sqrt(np.sum(ss)) * gs


def scale(norm, c):
    """c / max(norm, c) in float32: exactly 1 for norm <= c and for a zero norm."""
    norm, c = np.float32(norm), np.float32(c)
    return np.float32(c / np.maximum(norm, c))


def scales(entry_norms32, global_norm32, mode, c):
    """-> (global scale, per-entry scales) float32 for mode 'none' | 'per_variable' | 'global', from float32 norms."""
    E = len(entry_norms32)
    one = np.ones(E, dtype=np.float32)
    if mode == "global":
        return scale(global_norm32, c), one
    if mode == "per_variable":
        return np.float32(1.0), np.array([scale(n, c) for n in entry_norms32], dtype=np.float32)
    return np.float32(1.0), one


def nonfinite(flat, entries):
    return int(sum(np.count_nonzero(~np.isfinite(view(flat, e))) for e in entries))


def skip(n_nonfinite, skip_nonfinite):
    return bool(skip_nonfinite) and n_nonfinite > 0


def swept_gradient(g, grad_scale=1.0, s=1.0, clipvalue=0.0):
    """The gradient an element of the clipped sweep sees: gg = (g * grad_scale) * s, then clamped to +-clipvalue (float32)."""
    gg = (np.asarray(g, np.float32) * np.float32(grad_scale)) * np.float32(s)
    if clipvalue > 0:
        gg = np.minimum(np.maximum(gg, np.float32(-clipvalue)), np.float32(clipvalue))
    return gg.astype(np.float32)


# ---- the Keras forms (tf.clip_by_norm, tf.clip_by_global_norm), in float32 like TensorFlow evaluates them
def keras_clip_by_norm(g, c):
    g = np.asarray(g, np.float32)
    l2 = np.float32(np.sqrt(np.sum(np.square(g.astype(np.float64)))))
    return (g * np.float32(c)) / np.maximum(l2, np.float32(c))


def keras_clip_by_global_norm(gs, c):
    gn = np.float32(np.sqrt(sum(np.sum(np.square(np.asarray(g, np.float64))) for g in gs)))
    c = np.float32(c)
    factor = c * np.minimum(np.float32(1.0) / gn, np.float32(1.0) / c)
    return [np.asarray(g, np.float32) * factor for g in gs]
