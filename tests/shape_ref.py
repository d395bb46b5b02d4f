"""NumPy restatement of kx_shape_logits and of the sampler's min-p filter (include/kosmosx_hip.h, "Logit shaping"): integer counts,
single float32 operations and threshold compares, so the kernels are held to it bit for bit."""
import math

import numpy as np

import sampling_ref as R


def shape_row(logits, counts, *, bias=(), frequency=0.0, presence=0.0, last_token=None, finished=False):
    """One row of one launch.  ``logits`` float32 [V]; ``counts`` int32 [V] or None; ``bias`` (id, value) pairs.
    Returns (the new row, the new counts) as copies."""
    l = np.array(logits, dtype=np.float32, copy=True)
    c = None if counts is None else np.array(counts, dtype=np.int32, copy=True)
    V = l.shape[0]
    if finished:
        return l, c
    if c is not None and last_token is not None and 0 <= int(last_token) < V:
        c[int(last_token)] += 1
    with np.errstate(all="ignore"):
        for i, v in bias:
            if 0 <= i < V and l[i] > -np.inf:                  # -inf and NaN keep their bits
                l[i] = np.float32(l[i]) + np.float32(v)
        if c is not None:
            f, p = np.float32(frequency), np.float32(presence)
            on = (c > 0) & (l > -np.inf)
            t = (f * c[on].astype(np.float32)).astype(np.float32)
            u = (l[on] - t).astype(np.float32)
            l[on] = (u - p).astype(np.float32)
    return l, c


def shape_rows(logits, counts, *, bias=None, frequency=0.0, presence=0.0, last_token=None, finished=None):
    """[B, V] at once: ``bias`` a list of B lists of pairs (or None)."""
    B = logits.shape[0]
    out_l, out_c = [], []
    for b in range(B):
        l, c = shape_row(logits[b], None if counts is None else counts[b], bias=() if bias is None else bias[b], frequency=frequency,
                         presence=presence, last_token=None if last_token is None else last_token[b],
                         finished=finished is not None and bool(finished[b]))
        out_l.append(l)
        out_c.append(c)
    return np.stack(out_l), (None if counts is None else np.stack(out_c))


def log_min_p(min_p) -> np.float32:
    """lm = (float)log((double)m) for the float the C ABI carries."""
    return np.float32(math.log(float(np.float32(min_p))))


def min_p_keep(x, keep, min_p) -> np.ndarray:
    """``keep`` (after top-k and top-p) restricted to x_i >= x_max + lm, x_max over the whole row; one float32 add and a compare."""
    if float(min_p) == 0.0 or not keep.any():
        return keep.copy()
    with np.errstate(all="ignore"):
        thr = np.float32(np.float32(x.max()) + log_min_p(min_p))
    return keep & (x >= thr)


def sample_keep(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, history=None):
    """(x, the kept set of a sampling launch): penalty -> temperature -> top-k -> top-p -> min-p."""
    x = R.scaled(logits, temperature, history, repetition_penalty)
    keep, _, _ = R.filter_row(x, top_k, top_p)
    return x, min_p_keep(x, keep, min_p)


def min_p_keep_float64(x, top_k, top_p, min_p) -> np.ndarray:
    """The sentence itself in float64: p_i >= m * p_max (softmax over the whole row; the ratio is what matters), after top-k and top-p."""
    keep, _, _ = R.filter_row(x, top_k, top_p)
    x64 = x.astype(np.float64)
    with np.errstate(all="ignore"):
        ratio = np.where(x64 == x64.max(), 1.0, np.exp(x64 - x64.max()))
    return keep & (ratio >= float(np.float32(min_p)))
