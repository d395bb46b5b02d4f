"""numpy / float64 restatement of the beam-search contract (include/kosmosx_hip.h, "Beam search on the device"), written from
the contract text, and the comparison rule the beam tests share.

State of one batch row: W live beams with cumulative scores, a pool (list of at most W dicts score / end / parent, in slot
order) and a done flag.  ``step`` ranks the Win * V candidates of one batch row, ``finalize`` offers the live beams and orders
the pool, ``backtrack`` follows the backpointers.

Comparison rule (after sampling_ref.check_draw): every decision the reference takes comes with its margin — the gap between the
two fp64 numbers compared.  ``step`` / ``finalize`` return the smallest margin among the decisions that fix their outcome; the
device must take the same outcome where it exceeds EPS_M; where it does not, either outcome is accepted and a case in which the
device took the other one is counted (``Tally``: at most 1 % of a test's cases).
Scores agree within EPS_S: with |x|, |lse| < 64 and |s| < 256 the fp32 roundings of x - lse (2^-18 relative to 64: 3.8e-6),
m + log (3.8e-6), s + lp (1.5e-5 at |s| < 256), the fixed-point truncation (V * 2^-40 relative) and logf (a few ulp of < 16)
sum to less than 3e-5; the division by n^alpha only shrinks them."""
import numpy as np

EPS_M = 2e-4          # a decision whose margin exceeds this is the device's decision too
EPS_S = 1e-4          # absolute score tolerance
FLT_MAX = float(np.finfo(np.float32).max)


def log_softmax_row(x):
    """(lp [V] float64 with -inf for the non-candidates): the load rules, then x - (m + log sum exp(x - m))."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[~(x > -np.inf)] = -np.inf                         # NaN and -inf are never candidates
    x[x > FLT_MAX] = FLT_MAX                            # +inf is clamped
    x = x + 0.0                                         # -0 reads as +0
    if not (x > -np.inf).any():
        return x
    m = x.max()
    with np.errstate(under="ignore"):
        z = np.exp(x - m).sum()
    with np.errstate(invalid="ignore"):
        return x - (m + np.log(z))


def _offer(pool, W, score, end, parent, margins):
    """The replacement rule.  Returns the new pool (slot order kept)."""
    pool = [dict(p) for p in pool]
    new = dict(score=float(score), end=int(end), parent=int(parent))
    if len(pool) < W:
        pool.append(new)
        return pool
    sc = np.array([p["score"] for p in pool])
    worst = max(k for k in range(W) if sc[k] == sc.min())     # the later slot among equal ones
    others = np.delete(sc, worst)
    margins.append(abs(score - sc[worst]))                    # replace or not
    if score > sc[worst]:
        if others.size:
            margins.append(others.min() - sc[worst])          # which entry is the worst
        pool[worst] = new
    return pool


def step(logits, scores, pool, g, *, W, eos=None, pad=1, alpha=1.0, early=False, done=False):
    """One step of one batch row.  logits [Win, V], scores [Win] (Win = 1 at g = 0, else W).
    -> dict(token [W], parent [W], score [W] float64, pool, done, margin)."""
    logits = np.asarray(logits)
    Win, V = logits.shape
    scores = np.asarray(scores, dtype=np.float64)
    assert Win == (1 if g == 0 else W) and scores.shape == (Win,)
    if done:                                            # frozen
        par = [i if i < Win else 0 for i in range(W)]
        return dict(token=[pad] * W, parent=par, score=[float(scores[p]) for p in par], pool=[dict(p) for p in pool], done=True,
                    margin=np.inf)
    c = np.full((Win, V), -np.inf)
    for j in range(Win):
        if scores[j] > -np.inf:
            c[j] = scores[j] + log_softmax_row(logits[j])
    flat = c.ravel()
    K = 2 * W
    order = np.argsort(-flat, kind="stable")[: K + 1]   # descending, ties to the lower flat index
    order = [int(i) for i in order if flat[i] > -np.inf]
    margins = []
    pen = float(g + 1) ** float(alpha)
    tok, par, sc = [], [], []
    best_live = -np.inf
    walked = 0
    for k, i in enumerate(order[:K]):
        if len(tok) == W:
            break
        walked = k + 1
        j, v = divmod(i, V)
        if eos is not None and v == eos:
            if k < W:
                pool = _offer(pool, W, flat[i] / pen, g, j, margins)
            continue
        if not tok:
            best_live = flat[i]
        tok.append(v), par.append(j), sc.append(float(flat[i]))
    # the gaps that fix the walk: between consecutive walked candidates and to the first one not walked
    for k in range(min(walked, len(order) - 1)):
        margins.append(flat[order[k]] - flat[order[k + 1]])
    for i in range(len(tok), W):
        tok.append(pad), par.append(i if i < Win else 0), sc.append(-np.inf)
    now_done = False
    if len(pool) == W:
        worst = min(p["score"] for p in pool)
        if early:
            now_done = True
        else:
            now_done = bool(worst >= best_live / pen)
            if np.isfinite(best_live):
                margins.append(abs(worst - best_live / pen))
    return dict(token=tok, parent=par, score=sc, pool=pool, done=now_done, margin=min(margins) if margins else np.inf)


def finalize(scores, pool, done, n, *, W, R, alpha=1.0):
    """-> dict(pool, order [R] pool slots or None, score [R], margin)."""
    margins = []
    pool = [dict(p) for p in pool]
    if not done:
        pen = float(n) ** float(alpha)
        for i in range(W):
            if scores[i] > -np.inf:
                pool = _offer(pool, W, float(scores[i]) / pen, n, i, margins)
    sc = np.array([p["score"] for p in pool], dtype=np.float64)
    ranked = [int(k) for k in np.argsort(-sc, kind="stable")]
    for k in range(min(R, len(ranked) - 1)):
        margins.append(sc[ranked[k]] - sc[ranked[k + 1]])
    order = [ranked[r] if r < len(ranked) else None for r in range(R)]
    return dict(pool=pool, order=order, score=[-np.inf if k is None else float(sc[k]) for k in order],
                margin=min(margins) if margins else np.inf)


def backtrack(entry, parent, token, n, *, eos=None, pad=1):
    """The n tokens of a pool entry (None: all pad).  parent / token: [n, W] backpointers of ONE batch row."""
    out = [pad] * n
    if entry is None:
        return out
    end, slot = entry["end"], entry["parent"]
    if end < n:
        out[end] = eos
    for g in range(end - 1, -1, -1):
        out[g] = int(token[g][slot])
        slot = int(parent[g][slot])
    return out


class Tally:
    """Counts the (row, step) cases in which the device took the other outcome of a decision whose margin is inside EPS_M; at
    most 1 % of a test's cases may be."""

    def __init__(self):
        self.cases = self.counted = 0

    def check(self):
        assert self.counted <= 0.01 * self.cases, (self.counted, self.cases)


def _same_pool(got, ref):
    gs, ge, gp, gc = got
    return int(gc) == len(ref) and all((int(ge[k]), int(gp[k])) == (p["end"], p["parent"]) for k, p in enumerate(ref))


def check_pool(got, ref, msg=""):
    """got = (score [W], end [W], parent [W], count) of one batch row against the reference's pool list."""
    assert _same_pool(got, ref), (msg, [list(map(float, got[0])), list(map(int, got[1])), list(map(int, got[2])), int(got[3])], ref)
    for k, p in enumerate(ref):
        assert abs(float(got[0][k]) - p["score"]) <= EPS_S, (msg, k, float(got[0][k]), p["score"])


def check_step(got, ref, tally, msg=""):
    """got = dict(token, parent, score [W], pool = (score, end, parent, count), done) of one batch row and step.  As
    sampling_ref.check_draw: the device's outcome equals the reference's ("exact": then the scores agree within EPS_S too), or
    the reference's smallest deciding margin is inside EPS_M and the case is counted ("eps"); anything else fails."""
    tally.cases += 1
    same = ([int(t) for t in got["token"]] == ref["token"] and [int(p) for p in got["parent"]] == ref["parent"]
            and _same_pool(got["pool"], ref["pool"]) and bool(got["done"]) == ref["done"])
    if not same:
        assert ref["margin"] <= EPS_M, (msg, ref["margin"], list(map(int, got["token"])), ref["token"],
                                        list(map(int, got["parent"])), ref["parent"], bool(got["done"]), ref["done"])
        tally.counted += 1
        return "eps"
    for a, b in zip(got["score"], ref["score"]):
        assert (float(a) == b) if not np.isfinite(b) else abs(float(a) - b) <= EPS_S, (msg, list(map(float, got["score"])), ref["score"])
    check_pool(got["pool"], ref["pool"], msg)
    return "exact"


def brute_force(step_logits, n, W, alpha=1.0):
    """Exhaustive search without EOS: step_logits(prefix tuple) -> logits [V].  Every length-n sequence with its summed
    log-probability / n^alpha, best first (ties to the lexicographically smaller sequence) -> [(score, tokens)][:W]."""
    seqs = [((), 0.0)]
    for _ in range(n):
        nxt = []
        for pre, s in seqs:
            lp = log_softmax_row(step_logits(pre))
            nxt.extend((pre + (v,), s + lp[v]) for v in range(lp.shape[0]) if lp[v] > -np.inf)
        seqs = nxt
    ranked = sorted(seqs, key=lambda t: (-t[1], t[0]))[:W]
    return [(s / float(n) ** alpha, list(p)) for p, s in ranked]
