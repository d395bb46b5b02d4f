"""Contrastive search restated in NumPy, for tests/test_contrast.py and the three GPU test files.

float64: the unit hidden rows (unit_rows), the degeneration penalty (penalty), the score and the choice (scores, choose).
fp32: the three operations of the score exactly as the header states them (scores_fp32: two products and one difference, each
rounded once, 1 - alpha rounded to fp32 on the host) and the stated operation sequence of the unit rows (unit_rows_fp32), which is
an error model and not a bit-for-bit restatement: NumPy's sums run in another order than the kernel's.

The tolerance of the hidden-rows tests is 8 x the largest deviation unit_rows_fp32 shows against unit_rows on the very rows under
test, computed on the CPU inside the test.  Measured on the CPU for rows of the kind the tests use (residual rows of the tiny
models, D = 128, entries of order 1, and the D = 2048 rows of hidden_rows(0, 18, 2048)): largest deviation 3.9e-08 at D = 128 and
1.7e-08 at D = 2048 (a unit row's entries are ~ 1 / sqrt(D), so an ulp is smaller there), i.e. tolerances of about 3.1e-07 and
1.3e-07 on entries of a unit vector.

select_case builds the synthetic candidates and histories of the op-level tests; CASES and GENERATE_SEEDS are the seeds the GPU
tests use.  tests/test_contrast.py asserts on the CPU that the float64 scores of the best two candidates differ by more than 1e-3
at every row of every one of them, so the GPU tests may demand the chosen index exactly."""
import numpy as np

ALPHA = 0.6
EPS = 1e-5


def unit_rows(x, g, b, eps=EPS):
    """float64: LayerNorm (biased variance) of the rows of ``x`` with gamma ``g`` and beta ``b``, scaled to unit length."""
    x = np.asarray(x, np.float64)
    c = x - x.mean(-1, keepdims=True)
    h = c / np.sqrt((c * c).mean(-1, keepdims=True) + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)
    return h / np.sqrt((h * h).sum(-1, keepdims=True))


def unit_rows_fp32(x, g, b, eps=EPS, xb=None):
    """The header's sequence in fp32: v = x (+ xb); mean = sum(v) / D; c = v - mean; var = sum(c * c) / D; r = 1 / sqrt(var + eps);
    h = (c * r) * g + b; n = sqrt(sum(h * h)); u = h / n."""
    f = np.float32
    v = np.asarray(x, f) if xb is None else np.asarray(x, f) + np.asarray(xb, f)
    D = f(v.shape[-1])
    mean = v.sum(-1, keepdims=True, dtype=f) / D
    c = v - mean
    var = (c * c).sum(-1, keepdims=True, dtype=f) / D
    r = f(1.0) / np.sqrt(var + f(eps), dtype=f)
    h = (c * r) * np.asarray(g, f) + np.asarray(b, f)
    n = np.sqrt((h * h).sum(-1, keepdims=True, dtype=f), dtype=f)
    return h / n


def penalty(u, hist):
    """float64: u [k, D] candidates, hist [P, D] history rows -> [k], the largest dot product of each candidate with a row."""
    return (np.asarray(u, np.float64) @ np.asarray(hist, np.float64).T).max(-1)


def cosine_penalty(u, hist):
    """The direct formulation: the largest cosine similarity, norms divided out (equals penalty() on unit rows)."""
    u, hist = np.asarray(u, np.float64), np.asarray(hist, np.float64)
    out = np.empty(len(u))
    for j, a in enumerate(u):
        out[j] = max(float(a @ h) / (np.linalg.norm(a) * np.linalg.norm(h)) for h in hist)
    return out


def scores(prob, pen, alpha=ALPHA):
    a = float(np.float32(alpha))
    return (1.0 - a) * np.asarray(prob, np.float64) - a * np.asarray(pen, np.float64)


def scores_fp32(prob, pen, alpha=ALPHA):
    f = np.float32
    a = f(alpha)
    oma = f(1.0 - float(a))                               # 1 - alpha on the host, rounded to fp32 once
    return (oma * np.asarray(prob, f)).astype(f) - (a * np.asarray(pen, f)).astype(f)


def choose(s):
    """The largest score, the lowest index among equal ones; a NaN loses to every number (all NaN: 0)."""
    best = 0
    for j in range(1, len(s)):
        if s[j] == s[j] and (not s[best] == s[best] or s[j] > s[best]):
            best = j
    return best


def best_gap(s):
    t = np.sort(np.asarray(s, np.float64))
    return np.inf if len(t) < 2 else float(t[-1] - t[-2])


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def select_case(seed, k, D, Ps, cap=None):
    """B = len(Ps) sequences with P_b history rows: history fp32 [B, cap, D] (unit rows, zeros beyond P_b), u fp32 [B * k, D] unit
    candidates — mixtures of a history row and noise, so that the penalties spread over (0, 1) — and prob fp32 [B * k], descending
    per sequence as a top-k's are."""
    rng = np.random.default_rng(seed)
    B = len(Ps)
    cap = max(Ps) + 2 if cap is None else cap
    history = np.zeros((B, cap, D), np.float32)
    u = np.empty((B * k, D), np.float32)
    prob = np.empty(B * k, np.float32)
    for b, P in enumerate(Ps):
        history[b, :P] = _unit(rng.standard_normal((P, D)))
        mix = rng.uniform(0.0, 1.0, k)
        for j in range(k):
            row = history[b, rng.integers(0, P)].astype(np.float64)
            u[b * k + j] = _unit(mix[j] * row + (1.0 - mix[j]) * _unit(rng.standard_normal(D)).astype(np.float64))
        p = np.sort(rng.dirichlet(np.ones(k + 1))[:k])[::-1]
        prob[b * k:(b + 1) * k] = p.astype(np.float32)
    return dict(history=history, u=u, prob=prob, Ps=list(Ps), k=k, D=D, cap=cap)


def case_reference(case, alpha=ALPHA):
    """float64 penalties [B, k], scores [B, k] and choices [B] of a select_case."""
    k, pens, scs, picks = case["k"], [], [], []
    for b, P in enumerate(case["Ps"]):
        pen = penalty(case["u"][b * k:(b + 1) * k], case["history"][b, :P])
        s = scores(case["prob"][b * k:(b + 1) * k], pen, alpha)
        pens.append(pen), scs.append(s), picks.append(choose(s))
    return np.array(pens), np.array(scs), picks


def hidden_rows(seed, M, D):
    """Residual rows of order 1 with a common offset, and an affine pair, for the hidden-rows checks."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, D)) * 1.5 + rng.standard_normal((M, 1)) * 0.5).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    return x, g, b


# (seed, k, D, [P_b]) of tests/test_contrast_select_gpu.py: D in {128, 2048}, k in {1, 2, 5, 16}, B in {1, 3}, P_b mixed from
# 1, 63, 64, 65, 257, 1000 — one row, around a wave, around a chunk edge, many chunks
CASES = [(s, k, D, Ps) for D, s0 in ((128, 200), (2048, 1200)) for k in (1, 2, 5, 16)
         for s, Ps in ((s0 + k, [257]), (s0 + 40 + k, [1, 65, 1000] if k != 16 else [63, 64, 1000]))]
# model seeds of tests/test_generate_contrast_gpu.py, per (B, k)
GENERATE_SEEDS = {(1, 2): 7, (2, 3): 7, (3, 6): 7}
