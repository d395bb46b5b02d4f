"""NumPy restatement of kx_automaton_step's contract (include/kosmosx_hip.h, rules 1-6), one row at a time, from the four raw CSR
arrays alone: it knows nothing of kosmosx.automaton.TokenAutomaton, and the device kernel knows nothing of it."""
import numpy as np


def _edges(tables, s):
    """State s's edges as (ids, next states) after the range rules: offsets clamped into [0, E], out of order = none."""
    off, tok, nxt, _ = tables
    E = len(tok)
    lo, hi = min(max(int(off[s]), 0), E), min(max(int(off[s + 1]), 0), E)
    if hi < lo:
        hi = lo
    return [int(t) for t in tok[lo:hi]], [int(n) for n in nxt[lo:hi]]


def _state(v, S):
    """A next state outside [0, S) is the dead state."""
    return int(v) if 0 <= int(v) < S else -1


def entering_state(tables, state_in, src, b):
    """Rule 1: the state row b comes from (``src``: the src_row array or None)."""
    S = len(tables[3])
    i = b if src is None else int(src[b])
    if not 0 <= i < len(state_in):
        return -1
    return _state(state_in[i], S)


def step_row(tables, s, last_token, finished, V):
    """Rules 2-5 for one row that enters in state ``s`` (already through rule 1; any value outside [0, S) is dead).
    ``last_token``: an int or None.  Returns (new_state, ban_mask bool [V]); a finished row bans nothing."""
    S = len(tables[3])
    s = _state(s, S)
    ban = np.zeros(V, dtype=bool)
    if finished:
        return s, ban
    if last_token is not None and s >= 0:
        t = int(last_token)
        if not 0 <= t < V:
            s = -1
        else:
            ids, nexts = _edges(tables, s)
            s = _state(nexts[ids.index(t)] if t in ids else tables[3][s], S)
    if s < 0:
        ban[:] = True
        return s, ban
    ban[:] = _state(tables[3][s], S) < 0
    for t, n in zip(*_edges(tables, s)):
        if 0 <= t < V:
            ban[t] = _state(n, S) < 0
    return s, ban


def apply(row, ban):
    """The row after the mask: -inf where banned, the input's bits elsewhere."""
    out = np.array(row, dtype=np.float32, copy=True)
    out[ban] = -np.inf
    return out
