"""NumPy restatement of the kx_constrain_logits contract (include/kosmosx_hip.h), written from the contract.

A function of a row's LOGICAL token sequence (the ragged batch's padding columns already taken out, see ``logical``), the
logits row and the settings.  Returns which ids are banned and whether the row stops.  Ids outside [0, V) are compared as values
and never index anything."""
from __future__ import annotations

import numpy as np


def logical(history_row, hist_len, prompt_width=None, prompt_len=None) -> list:
    """The logical sequence of one physical history row: columns [0, hist_len), or — the ragged form — columns
    [0, prompt_len) followed by [prompt_width, hist_len)."""
    h = [int(t) for t in history_row[:hist_len]]
    if prompt_len is None:
        return h
    return h[:prompt_len] + h[prompt_width:]


def constrain_row(seq, row, *, new_tokens=0, ngram=0, bad_words=(), stop_sequences=(), min_new=0, eos_id=-1, finished=False):
    """(ban bool [V], finished bool) for the logical sequence ``seq`` and the fp32 logits ``row`` [V]."""
    s = [int(t) for t in seq]
    n, V, g = len(s), int(np.asarray(row).shape[0]), int(new_tokens)
    ban = np.zeros(V, dtype=bool)

    def mark(t):
        if 0 <= t < V:
            ban[t] = True

    if finished:
        return ban, True
    if g >= 1:
        for w in stop_sequences:
            w = [int(t) for t in w]
            if 1 <= len(w) <= n and s[n - len(w):] == w:
                return ban, True                                   # no bans for a row that has just stopped
    N = int(ngram)
    if N >= 1 and n + 1 >= N:
        prefix = s[n - (N - 1):] if N > 1 else []
        for i in range(n - N + 1):                                 # i + N - 1 < n
            if s[i:i + N - 1] == prefix:
                mark(s[i + N - 1])
    for w in bad_words:
        w = [int(t) for t in w]
        m = len(w)
        if m == 1:
            mark(w[0])
        elif m > 1 and n >= m - 1 and s[n - (m - 1):] == w[:-1]:
            mark(w[-1])
    if g < int(min_new) and eos_id is not None and eos_id >= 0:
        mark(int(eos_id))
    return ban, False


def apply(row, ban) -> np.ndarray:
    """The row after the launch: -inf where banned, the input bits elsewhere."""
    out = np.array(row, dtype=np.float32, copy=True)
    out[ban] = -np.inf
    return out
