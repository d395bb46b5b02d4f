"""NumPy / float64 restatement of the sampler's truncation stages (include/kosmosx_hip.h, "Truncation sampling"): typical-p, epsilon
and eta behind top-k / top-p / min-p, the `transformers` warper order, each stage over the softmax renormalised on what the stage
before it kept.  Test infrastructure on top of tests/sampling_ref.py and tests/shape_ref.py, written from the sentences of the
contract (probabilities, entropy, logarithms in float64), not from the kernel's integer arithmetic.

Next to every kept set comes the set of UNSURE elements: those so close to a stage's threshold that fp32 against float64 may
decide them either way.  delta = 1e-4 (the clearance tests/test_sample_min_p_gpu.py asks of a threshold compare) and eps_p = 1e-5
(sampling_ref.check_draw's tolerance on a mass boundary):
  typical-p        i is unsure iff mass{d_j < d_i - delta} < t + eps_p and mass{d_j < d_i + delta} >= t - eps_p;
  epsilon and eta  i is unsure iff |log p_i - log threshold| <= delta.
"""
from __future__ import annotations

import numpy as np

import sampling_ref as R
import shape_ref as SR

DELTA, EPS_P, EPS_G = 1e-4, 1e-5, 1e-4


def log_probs(x, keep):
    """(p, log p) of the softmax over ``keep`` in float64; 0 / -inf outside.  +inf ties at the maximum share the whole mass."""
    x = np.asarray(x, dtype=np.float64)
    p, lp = np.zeros(x.shape), np.full(x.shape, -np.inf)
    idx = np.nonzero(keep)[0]
    if idx.size == 0:
        return p, lp
    xv = x[idx]
    m = xv.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(xv == m, 0.0, xv - m)                         # (inf - inf is a tie: 0)
        lse = np.log(np.exp(s).sum())
        lp[idx] = s - lse
    p[idx] = np.exp(lp[idx])
    return p, lp


def entropy(p, lp):
    with np.errstate(invalid="ignore"):
        return float(-np.where(p > 0, p * lp, 0.0).sum())           # (0 log 0 = 0, the nansum of the warper)


def typical_stage(x, keep, t):
    """(kept, unsure).  i stays iff the mass of {j : d_j < d_i} is < t, d = |-log p - H|; ties in d stay or go together."""
    t = float(np.float32(t))
    if t >= 1.0 or not keep.any():
        return keep.copy(), np.zeros(keep.shape, dtype=bool)
    p, lp = log_probs(x, keep)
    H = entropy(p, lp)
    idx = np.nonzero(keep)[0]
    with np.errstate(invalid="ignore"):
        d = np.abs(-lp[idx] - H)
    order = np.argsort(d, kind="stable")
    ds, cum = d[order], np.concatenate([[0.0], np.cumsum(p[idx][order])])

    def below(v):                                                   # mass of {d_j < v}
        return cum[np.searchsorted(ds, v, side="left")]
    out, unsure = np.zeros(keep.shape, dtype=bool), np.zeros(keep.shape, dtype=bool)
    out[idx] = below(d) < t
    unsure[idx] = (below(d - DELTA) < t + EPS_P) & (below(d + DELTA) >= t - EPS_P)
    return out, unsure


def _cut_stage(x, keep, p, thr):
    """p_i >= thr, or x_i is the maximum of ``keep``; unsure within delta of the threshold in log p."""
    out, unsure = np.zeros(keep.shape, dtype=bool), np.zeros(keep.shape, dtype=bool)
    idx = np.nonzero(keep)[0]
    top = x[idx] == x[idx].max()
    out[idx] = (p[idx] >= thr) | top
    with np.errstate(divide="ignore"):
        unsure[idx] = (np.abs(np.log(p[idx]) - np.log(thr)) <= DELTA) & ~top
    return out, unsure


def epsilon_stage(x, keep, e):
    e = float(np.float32(e))
    if e == 0.0 or not keep.any():
        return keep.copy(), np.zeros(keep.shape, dtype=bool)
    return _cut_stage(x, keep, log_probs(x, keep)[0], e)


def eta_stage(x, keep, e):
    e = float(np.float32(e))
    if e == 0.0 or not keep.any():
        return keep.copy(), np.zeros(keep.shape, dtype=bool)
    p, lp = log_probs(x, keep)
    return _cut_stage(x, keep, p, min(e, np.sqrt(e) * np.exp(-entropy(p, lp))))


def truncate_keep(x, keep, *, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """``keep`` (after top-k, top-p and min-p) through the three stages.  Returns (kept, unsure, stages): ``unsure`` is the union
    of the stages' unsure elements, ``stages`` the kept set after each stage (whether each one bound is read off their sizes)."""
    unsure = np.zeros(keep.shape, dtype=bool)
    stages = []
    for stage, v in ((typical_stage, typical_p), (epsilon_stage, epsilon_cutoff), (eta_stage, eta_cutoff)):
        keep, u = stage(x, keep, v)
        unsure |= u
        stages.append(keep)
    return keep, unsure, stages


def sample_keep(logits, *, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0,
                repetition_penalty=1.0, history=None):
    """(x, kept, unsure, stages, S0) of a sampling launch: penalty -> temperature -> top-k -> top-p -> min-p -> typical-p ->
    epsilon -> eta."""
    x, s0 = SR.sample_keep(logits, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                           repetition_penalty=repetition_penalty, history=history)
    keep, unsure, stages = truncate_keep(x, s0, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
    return x, keep, unsure, stages, s0


def sample_row(logits, *, seed=0, position=0, sequence_id=0, pad_token_id=1, **kw):
    """dict(token, none, keep, unsure, x, score): the Gumbel arg max (sampling_ref's uniforms) over the kept set."""
    x, keep, unsure, _, _ = sample_keep(logits, **kw)
    if not keep.any():
        return dict(token=pad_token_id, none=True, keep=keep, unsure=unsure, x=x, score=None)
    u = R.uniforms(seed, sequence_id, position, x.shape[0])
    with np.errstate(invalid="ignore"):
        score = x.astype(np.float64) - np.log(-np.log(u))
    return dict(token=int(np.argmax(np.where(keep, score, -np.inf))), none=False, keep=keep, unsure=unsure, x=x, score=score)


def check_draw(token, ref, eps_g=EPS_G):
    """The drawn-token rule with unsure elements: ``token`` is the reference's, or it is the arg max — within eps_g on the float64
    score — over some set between (kept minus unsure) and (kept plus unsure).  Returns "exact" / "eps", raises otherwise."""
    if token == ref["token"]:
        return "exact"
    assert not ref["none"], (token, "the reference has no candidate")
    assert 0 <= token < ref["x"].shape[0] and (ref["keep"][token] or ref["unsure"][token]), (token, "outside the kept set")
    sure = ref["keep"] & ~ref["unsure"]
    if sure.any():
        best = ref["score"][sure].max()
        assert ref["score"][token] >= best - eps_g, (token, ref["token"], ref["score"][token], best)
    return "eps"


# ---- the rows and the cases the kept-set tests share (tests/test_truncate.py asserts their band conditions on the CPU,
# tests/test_sample_truncate_gpu.py compares the device's kept sets on them) ----

SCALES = (0.3, 1.0, 1.0, 2.0, 3.0, 3.0, 5.0, 8.0)           # per row: from nearly flat to peaked, so that a filter binds here and is slack there
SEEDS = {5: 0, 37: 1, 502: 44, 1500: 163, 4099: 0, 64007: 0}   # chosen so that the band conditions hold (asserted, not assumed)
EXACT_V = 1500                                              # up to here kept sets are compared for equality


def case_rows(V):
    """Gaussian rows [B, V] float32, row b at scale SCALES[b]; B = 8, or 2 (scales 1 and 3) at the product's vocabulary."""
    scales = np.array(SCALES if V < 64007 else (1.0, 3.0), dtype=np.float64)
    g = np.random.default_rng(7919 * SEEDS[V] + V).standard_normal((len(scales), V))
    return (g * scales[:, None]).astype(np.float32)


def case_history(rows):
    """The four most likely ids of every row: a repetition penalty over them moves the maximum."""
    return np.stack([np.argsort(-r, kind="stable")[:4] for r in rows]).astype(np.int64)


PEN = dict(repetition_penalty=1.7, history=True)            # (history=True: case_history of the rows)
ALONE = [dict(typical_p=0.2), dict(typical_p=0.9), dict(typical_p=0.95, temperature=0.7),
         dict(epsilon_cutoff=3e-4), dict(epsilon_cutoff=0.02, temperature=1.3),
         dict(eta_cutoff=2e-3), dict(eta_cutoff=0.05, temperature=0.7)]
FRONTED = [dict(typical_p=0.9, top_k=20), dict(typical_p=0.5, top_p=0.9), dict(typical_p=0.8, min_p=0.05), dict(typical_p=0.9, **PEN),
           dict(epsilon_cutoff=0.02, top_k=20), dict(epsilon_cutoff=2e-3, top_p=0.9), dict(epsilon_cutoff=0.01, min_p=0.02),
           dict(epsilon_cutoff=2e-3, **PEN),
           dict(eta_cutoff=0.05, top_k=20), dict(eta_cutoff=2e-3, top_p=0.9), dict(eta_cutoff=0.02, min_p=0.02), dict(eta_cutoff=2e-3, **PEN)]
TOGETHER = [dict(typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3, temperature=0.8),
            dict(typical_p=0.95, epsilon_cutoff=2e-3, eta_cutoff=0.02, top_k=50, top_p=0.95, min_p=0.01, **PEN)]


def case_keep(rows, case):
    """[(x, kept, unsure, stages, S0)] of every row under ``case`` (top_k is clipped below V as the tests pass it)."""
    kw = dict(case)
    hist = case_history(rows) if kw.pop("history", False) else None
    if "top_k" in kw:
        kw["top_k"] = min(kw["top_k"], rows.shape[1] - 1)
    return [sample_keep(r, history=None if hist is None else hist[b], **kw) for b, r in enumerate(rows)]
