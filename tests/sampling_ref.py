"""CPU restatement of the token-sampling contract (kx_sample_logits in include/kosmosx_hip.h), numpy / float64.

Test infrastructure, written from the contract, not from the kernel.  Per row:
  repetition penalty (once per distinct id of the history) -> temperature -> top-k (ties kept) -> top-p ("mass of the
  strictly greater values < p", on the softmax over what top-k kept) -> Gumbel-max draw with Philox4x32-10 uniforms.
The two divisions that define x (penalty, temperature) are single IEEE fp32 operations and are done in np.float32 here:
they are exactly reproducible, and the greedy arg max is specified on those fp32 values.  Everything after them (exp, log,
sums) is float64.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11).  Counter words: arrays (broadcast together); key words: Python ints.
    Returns four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n1 = p1 & MASK32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        n3 = p0 & MASK32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniforms(seed: int, sequence_id: int, position: int, V: int) -> np.ndarray:
    """u_i, i < V: (2 (w >> 9) + 1) 2^-24, w = word i & 3 of philox(counter = (position, sequence_id, i >> 2, 0), key = seed)."""
    nblk = (V + 3) // 4
    w = philox4x32_10(np.full(nblk, position & 0xFFFFFFFF), np.full(nblk, sequence_id & 0xFFFFFFFF), np.arange(nblk), 0,
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=1).reshape(-1)[:V].astype(np.uint64)
    return (2.0 * (words >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def penalised(logits, history=None, repetition_penalty=1.0) -> np.ndarray:
    """fp32 row after the repetition penalty; NaN and -inf become -inf (never a candidate)."""
    l = np.array(logits, dtype=np.float32, copy=True)
    r = np.float32(repetition_penalty)
    if history is not None and len(history) and r != np.float32(1.0):
        ids = np.unique(np.asarray(history, dtype=np.int64))
        ids = ids[(ids >= 0) & (ids < l.shape[0])]
        with np.errstate(invalid="ignore"):
            l[ids] = np.where(l[ids] > 0, l[ids] / r, l[ids] * r).astype(np.float32)
    l[~(l > -np.inf)] = -np.inf
    return l


def scaled(logits, temperature, history=None, repetition_penalty=1.0) -> np.ndarray:
    """x = penalised logit / T, fp32."""
    x = (penalised(logits, history, repetition_penalty) / np.float32(temperature)).astype(np.float32)
    x[~(x > -np.inf)] = -np.inf
    return x


def mass_ahead(x, keep) -> np.ndarray:
    """For every token of `keep`: the probability mass (softmax over `keep`) of the tokens with strictly greater x."""
    x = np.asarray(x, dtype=np.float64)
    out = np.full(x.shape, np.inf)
    idx = np.nonzero(keep)[0]
    if idx.size == 0:
        return out
    xv = x[idx]
    with np.errstate(invalid="ignore"):
        e = np.where(xv == xv.max(), 1.0, np.exp(xv - xv.max()))   # +inf ties at the maximum count as 1 each
    order = np.argsort(-xv, kind="stable")
    xs, es = xv[order], e[order]
    cum = np.concatenate([[0.0], np.cumsum(es)])               # cum[j] = mass of the j largest
    first = np.searchsorted(-xs, -xs, side="left")             # first position of each run of equal values
    out[idx[order]] = cum[first] / cum[-1]
    return out


def topk_keep(x, top_k) -> np.ndarray:
    valid = x > -np.inf
    V = x.shape[0]
    if 0 < top_k < V and int(valid.sum()) >= top_k:
        thr = np.sort(x[valid])[-top_k]
        return valid & (x >= thr)
    return valid


def filter_row(x, top_k=0, top_p=1.0):
    """(keep mask, mass-ahead of every top-k survivor).  top_p is the fp32 value the C ABI carries."""
    keepk = topk_keep(x, top_k)
    ahead = mass_ahead(x, keepk)
    p = float(np.float32(top_p))
    keep = keepk & (ahead < p) if p < 1.0 else keepk.copy()
    return keep, ahead, keepk


def sample_row(logits, *, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, do_sample=True, seed=0,
               position=0, sequence_id=0, history=None, pad_token_id=1):
    """dict(token, keep, x, score, ahead, keepk).  token == pad_token_id with `none` set when no candidate is left."""
    greedy = (not do_sample) or temperature == 0
    if greedy:
        x = penalised(logits, history, repetition_penalty)
        keep = x > -np.inf
        if not keep.any():
            return dict(token=pad_token_id, none=True, keep=keep, x=x, score=None, ahead=None, keepk=keep)
        return dict(token=int(np.argmax(x)), none=False, keep=keep, x=x, score=x.astype(np.float64), ahead=None, keepk=keep)
    x = scaled(logits, temperature, history, repetition_penalty)
    keep, ahead, keepk = filter_row(x, top_k, top_p)
    if not keep.any():
        return dict(token=pad_token_id, none=True, keep=keep, x=x, score=None, ahead=ahead, keepk=keepk)
    u = uniforms(seed, sequence_id, position, x.shape[0])
    with np.errstate(invalid="ignore"):
        score = x.astype(np.float64) - np.log(-np.log(u))
    masked = np.where(keep, score, -np.inf)
    return dict(token=int(np.argmax(masked)), none=False, keep=keep, x=x, score=score, ahead=ahead, keepk=keepk)


def check_draw(token, ref, eps_p=1e-5, eps_g=1e-4, top_p=1.0):
    """The drawn-token rule: `token` equals the reference's, or its float64 score is within eps_g of the reference's best
    and it lies inside the tolerant kept set (top-k survivor with mass-ahead <= p + eps_p).  Returns "exact" / "eps" and
    raises AssertionError otherwise."""
    if token == ref["token"]:
        return "exact"
    assert not ref["none"], (token, "the reference has no candidate")
    assert 0 <= token < ref["x"].shape[0] and ref["keepk"][token], (token, "outside what top-k kept")
    if float(np.float32(top_p)) < 1.0:
        assert ref["ahead"][token] <= float(np.float32(top_p)) + eps_p, (token, ref["ahead"][token])
    best = ref["score"][ref["token"]]
    assert ref["score"][token] >= best - eps_g, (token, ref["token"], ref["score"][token], best)
    return "eps"
