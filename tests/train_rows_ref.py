"""Plain restatements of the training step's row, reduction and operand kernels (the first half of csrc/kx_backward.hip): no GPU and
no kernel of this project.  tests/test_train_rows_ref.py ties every function here to something independent of it on the CPU,
tests/test_train_rows_gpu.py holds the kernels to them.

  * LayerNorm backward (and its GELU-rebuilding form), erf-GELU and its derivative, column sums and scalar sums are restated in
    float64 on the fp32 values as given.
  * Sums of integer-valued fp32 inputs are restated in int64: while every possible partial sum stays below 2^24 in magnitude, every
    fp32 addition is exact in ANY order, so a kernel's result equals the integer sum bit for bit (int_bound and the checks of
    tests/test_train_rows_ref.py keep that condition).  Equality is the assertion that sees one dropped or doubled row.
  * The GEMM operand rows (bf16, and the two bf16x3 row layouts) are packed with rowops_ref.pack_bf16, written from the format.

The inputs of the GPU test are generated here (fixed seeds), so that the CPU test can measure, on the very same inputs, what torch's
fp32 CPU operators lose against float64.  A kernel is held to LN_TOL_FACTOR (4: rowops_ref's factor for a different but legitimate
summation order) times the pinned figure; the project's 2e-5 is a floor for the `baseline` class only.  How an error is normalised:

  * dx: per row, max |dx - ref| over the row's RMS of the reference.  A single-column row without dres has an all-zero reference
    (x - mean and g - mean(g) vanish); it is normalised by the scale of its terms instead, rstd * rms(g): the kernels' g - mean(g) is
    a rounding residual of the product dy * gamma there (the multiply is contracted into the subtraction), as torch's is;
  * dbeta, column sums, scalar sums: per column, |got - ref| over the float64 sum of |term| of that column, so that a large column
    cannot hide a small one;
  * dgamma: per column, |got - ref| over sum_r |dy| * (|xhat| + rms(xhat of row r)).  The plain sum_r |dy * xhat| is unsound here: the
    error of xhat = (x - mean) * rstd is absolute (an ulp of |mean| times rstd), not relative to |xhat|, so with one row the figure is
    the relative error of the single product whose x lies closest to the row mean.  torch's fp32 CPU operator measures 4.25 (425 %)
    that way on the `offset` class at 1 x 8188 and 1.4e-4 on `baseline` at 1 x 6144, figures set by one element each, and four times
    such a figure bounds nothing.  Adding the row's RMS of xhat (1 unless the row is constant) keeps the bound per column and per
    row-scale and keeps it zero exactly where xhat is zero;
  * GELU and its backward: absolute.
Where a normaliser is ZERO (a single-column row, an integer-constant row: xhat = 0; a column of zero dy) the float64 result is exactly
zero and so is any fp32 evaluation of the kernels' formula: those entries are left out of the figures and the GPU test asserts them
for equality (exact_where_zero).  torch's CPU operator does not have that property at cols = 1, which is why they cannot be ratios.

All CPU figures are measured with torch restricted to ONE thread: torch's parallel reductions split rows between threads, so the
figure would otherwise depend on the machine.
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import rowops_ref as R

EPS = 1e-5
LN_TOL_FACTOR = R.LN_TOL_FACTOR
BASELINE_FLOOR = R.LN_BASELINE_TOL          # 2e-5
EXACT = 1 << 24                             # integers up to here are fp32 values


def _g(seed):
    return torch.Generator().manual_seed(seed)


@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def ratio_max(err, norm):
    """max of err / norm over the elements with norm > 0 (0.0 if there is none)."""
    err, norm = err.double().reshape(-1), norm.double().reshape(-1)
    r = torch.where(norm > 0, err / norm.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))
    return float(r.max())


def exact_where_zero(got, ref, norm):
    """True if got == ref (== 0) wherever the normaliser is zero."""
    z = norm.double() == 0
    return bool((got.double()[z] == ref.double()[z]).all())


def row_rms(ref):
    return ref.double().pow(2).mean(-1).sqrt()


def row_err(got, ref, norm=None):
    """dx: max over rows of (max |got - ref| over the row) / (RMS of the reference row, or the given per-row normaliser)."""
    ref = ref.double()
    return ratio_max((got.double() - ref).abs().amax(-1), row_rms(ref) if norm is None else norm)


def col_err(got, ref, norm):
    return ratio_max((got.double() - ref.double()).abs(), norm)


# ---------------------------------------------------------------------------------------------------------------------------------
# erf-GELU
# ---------------------------------------------------------------------------------------------------------------------------------
def _Phi(x):
    return 0.5 * torch.special.erfc(-x * math.sqrt(0.5))          # erfc: no cancellation in the lower tail


def gelu_ref(x):
    """x * Phi(x) in float64."""
    x = x.double()
    return x * _Phi(x)


def gelu_grad_ref(x):
    """Phi(x) + x * phi(x) in float64."""
    x = x.double()
    return _Phi(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_backward_ref(x, gamma, dy, eps=EPS, dres=None, gelu_in=False):
    """float64 backward of y = xhat * gamma + beta, xhat = (x - mean) * rstd (two-pass mean, biased variance, eps as the fp32 value
    the kernels receive):  g = dy * gamma,  dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ dres),  dgamma = sum_r dy * xhat,
    dbeta = sum_r dy.  gelu_in: the normalised row is the float64 erf-GELU of x ROUNDED ONCE to fp32 (csrc/kx_gelu_load.h pins
    it the same way; rowops_ref.gelu_layernorm_ref) and dx is the gradient at that activation.
    -> dict(dx, dgamma, dbeta, dx_norm = the row's RMS of dx (rstd * rms(g) where that is zero), dgamma_norm = sum_r |dy| * (|xhat| +
    rms(xhat_r)), dbeta_norm = sum_r |dy|, dx_scale = rstd * rms(g)), all float64."""
    v = gelu_ref(x).float().double() if gelu_in else x.double()
    d, gm = dy.double(), gamma.double()
    mean = v.mean(-1, keepdim=True)
    c = v - mean
    rstd = 1.0 / torch.sqrt((c * c).mean(-1, keepdim=True) + R._eps32(eps))
    xh = c * rstd
    g = d * gm
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    scale = (rstd * g.pow(2).mean(-1, keepdim=True).sqrt()).reshape(-1)
    if dres is not None:
        dx = dx + dres.double()
    gnorm = (d.abs() * (xh.abs() + xh.pow(2).mean(-1, keepdim=True).sqrt())).sum(0)
    return _with_dx({"dgamma": (d * xh).sum(0), "dbeta": d.sum(0), "dgamma_norm": gnorm, "dbeta_norm": d.abs().sum(0),
                     "dx_scale": scale}, dx)


def _with_dx(ref, dx):
    rms = row_rms(dx)
    return dict(ref, dx=dx, dx_norm=torch.where(rms > 0, rms, ref["dx_scale"]))


def add_dres(ref, dres):
    """The reference of the same inputs with dres added to dx."""
    return _with_dx(ref, ref["dx"] + dres.double())


LNB_CLASSES = ["baseline", "offset", "spike", "intconst", "int_dy"]
# (rows, cols) per route of layernorm_backward_impl (csrc/kx_backward.hip); the GPU test's docstring derives them.
FUSED_COLS = [1024, 2048, 3072, 4096, 6144, 8192]


def fused_rows(cols):
    """1, 3, and one more than the one-pass kernel's workgroup target (512 up to 4096 columns, 256 above): workgroups then carry two
    rows and the last one carries one."""
    return [1, 3, 513 if cols <= 4096 else 257]


BLOCK_COLS, BLOCK_ROWS = [4, 260, 1028, 5120, 8188], [1, 7]
WAVE_COLS, WAVE_ROWS = [1, 3, 63, 65, 130, 8196, 12290], [1, 4, 5, 7]
SHIFTED_COLS, SHIFTED_ROWS = [256, 2048], [5]             # x one float into its buffer: the wave-per-row kernel at aligned widths
SLICE_CAP = [(16390, 68), (16390, 1024)]                   # rows > 16384: 256 slices of 65 rows (two-kernel form) / the one-pass form


# route -> every (rows, cols) the GPU test runs it at.  A route is a row kernel of layernorm_backward_impl: ln_bwd_fused_kernel
# (gelu_fused: its GELU_IN form through kx_gelu_layernorm_backward), ln_bwd_row_block_kernel, ln_bwd_row_kernel; `slice` is the two
# shapes past the slice cap.  The tolerances are pinned per (route, class).
LNB_ROUTES = {
    "fused": [(r, c) for c in FUSED_COLS for r in fused_rows(c)],
    "gelu_fused": [(r, c) for c in FUSED_COLS for r in fused_rows(c)],
    "block": [(r, c) for c in BLOCK_COLS for r in BLOCK_ROWS],
    "wave": [(r, c) for c in WAVE_COLS for r in WAVE_ROWS] + [(r, c) for c in SHIFTED_COLS for r in SHIFTED_ROWS],
    "slice": SLICE_CAP,
}


def lnb_inputs(cls, rows, cols, gelu=False):
    """-> dict(x [rows, cols], gamma [cols], dy, dres [rows, cols]) fp32 on the CPU.  gelu: x is the pre-activation.
      baseline  unit normal x 2 + 0.5 (gelu: pre-activations spread over [-6, 6])
      offset    row means ~1e3 with unit spread
      spike     one 1e4 entry per row
      intconst  every entry of a row the same small integer k (3 .. 9; gelu: 6 .. 12, where gelu(k) == k in fp32): sums of the row
                are exact in fp32, so xhat is exactly 0 in fp32 as in float64: dgamma = 0 and dx = (g - mean g) / sqrt(eps)
      int_dy    baseline x, dy integer-valued in [-4, 4]: dbeta is exact in any order"""
    g = _g(1_000_003 * LNB_CLASSES.index(cls) + 131 * rows + cols + (500_000_000 if gelu else 0))
    gamma = 1 + 0.2 * torch.randn(cols, generator=g)
    dy = torch.randn(rows, cols, generator=g)
    dres = torch.randn(rows, cols, generator=g)
    base = (lambda: torch.rand(rows, cols, generator=g) * 12 - 6) if gelu else (lambda: torch.randn(rows, cols, generator=g) * 2 + 0.5)
    if cls == "offset":
        x = torch.randn(rows, cols, generator=g) + 1000.0 * (1 + 0.25 * torch.rand(rows, 1, generator=g))
    elif cls == "spike":
        x = base() if gelu else torch.randn(rows, cols, generator=g)
        r = torch.arange(rows)
        x[r, (7 * r + cols - 2) % cols] = 1.0e4
    elif cls == "intconst":
        x = ((torch.arange(rows) % 7) + (6 if gelu else 3)).float()[:, None].expand(rows, cols).contiguous()
    else:
        x = base()
        if cls == "int_dy":
            dy = torch.randint(-4, 5, (rows, cols), generator=g).float()
    return {"x": x, "gamma": gamma, "dy": dy, "dres": dres}


def lnb_cpu_fp32(inp, gelu=False, with_dres=False):
    """torch's fp32 CPU autograd of F.layer_norm (gelu: at the fp32 F.gelu activation) -> (dx, dgamma, dbeta)."""
    cols = inp["x"].shape[1]
    x = (F.gelu(inp["x"]) if gelu else inp["x"]).detach().clone().requires_grad_()
    gam, bet = inp["gamma"].clone().requires_grad_(), torch.zeros(cols, requires_grad=True)
    (F.layer_norm(x, (cols,), gam, bet, EPS) * inp["dy"]).sum().backward()
    return (x.grad + inp["dres"] if with_dres else x.grad), gam.grad, bet.grad


def lnb_errors(got, ref):
    """(dx, dgamma, dbeta) normalised errors of a (dx, dgamma, dbeta) triple against an ln_backward_ref dict."""
    return (row_err(got[0], ref["dx"], ref["dx_norm"]), col_err(got[1], ref["dgamma"], ref["dgamma_norm"]),
            col_err(got[2], ref["dbeta"], ref["dbeta_norm"]))


def lnb_cpu_fp32_error(route, cls):
    """max over LNB_ROUTES[route] of torch's fp32 CPU error on lnb_inputs(cls, ...), with and without dres."""
    worst, gelu = [0.0, 0.0, 0.0], route == "gelu_fused"
    with one_thread():
        for rows, cols in LNB_ROUTES[route]:
            inp = lnb_inputs(cls, rows, cols, gelu)
            ref = ln_backward_ref(inp["x"], inp["gamma"], inp["dy"], EPS, None, gelu)
            e = list(lnb_errors(lnb_cpu_fp32(inp, gelu), ref))
            ref = add_dres(ref, inp["dres"])
            e[0] = max(e[0], row_err(lnb_cpu_fp32(inp, gelu, True)[0], ref["dx"], ref["dx_norm"]))
            worst = [max(a, b) for a, b in zip(worst, e)]
    return tuple(worst)


# (route, class) -> (dx, dgamma, dbeta) of lnb_cpu_fp32_error, measured on an x86-64 CPU build of torch 2.10 and rounded up;
# tests/test_train_rows_ref.py re-measures and requires measured <= pinned <= 4 x measured.  None: the quantity is asserted exactly
# for that class (intconst: dgamma == 0; int_dy: dbeta == the integer sum), so it has no tolerance.
LNB_CPU_ERR = {
    ("fused", "baseline"): (1.8e-06, 1.8e-07, 3e-07),      # measured 1.18e-06, 1.20e-07, 1.97e-07
    ("fused", "offset"): (0.00022, 0.00024, 2.6e-07),      # measured 1.45e-04, 1.55e-04, 1.70e-07
    ("fused", "spike"): (8.2e-06, 6.8e-07, 2.6e-07),      # measured 5.43e-06, 4.48e-07, 1.70e-07
    ("fused", "intconst"): (1.9e-06, None, 2.7e-07),      # measured 1.27e-06, 0.00e+00, 1.79e-07
    ("fused", "int_dy"): (8.7e-07, 2.2e-07, None),      # measured 5.74e-07, 1.44e-07, 0.00e+00
    ("gelu_fused", "baseline"): (1.8e-06, 4.3e-07, 2.8e-07),      # measured 1.16e-06, 2.82e-07, 1.83e-07
    ("gelu_fused", "offset"): (0.0003, 0.00017, 2.8e-07),      # measured 1.99e-04, 1.10e-04, 1.83e-07
    ("gelu_fused", "spike"): (7e-06, 7.3e-07, 2.6e-07),      # measured 4.65e-06, 4.80e-07, 1.71e-07
    ("gelu_fused", "intconst"): (1.6e-06, None, 3.6e-07),      # measured 1.04e-06, 0.00e+00, 2.35e-07
    ("gelu_fused", "int_dy"): (8.6e-07, 4e-07, None),      # measured 5.67e-07, 2.61e-07, 0.00e+00
    ("block", "baseline"): (1.3e-06, 2.4e-07, 2.2e-07),      # measured 8.27e-07, 1.59e-07, 1.42e-07
    ("block", "offset"): (0.0009, 9.3e-05, 2.6e-07),      # measured 5.94e-04, 6.17e-05, 1.73e-07
    ("block", "spike"): (1.6e-06, 3.4e-07, 2.1e-07),      # measured 1.02e-06, 2.20e-07, 1.37e-07
    ("block", "intconst"): (1.3e-06, None, 2.2e-07),      # measured 8.35e-07, 0.00e+00, 1.44e-07
    ("block", "int_dy"): (3e-06, 1.7e-07, None),      # measured 1.99e-06, 1.09e-07, 0.00e+00
    ("wave", "baseline"): (9.6e-05, 2e-07, 2.2e-07),      # measured 6.40e-05, 1.27e-07, 1.41e-07
    ("wave", "offset"): (0.017, 0.0002, 2.4e-07),      # measured 1.12e-02, 1.30e-04, 1.53e-07
    ("wave", "spike"): (7e-06, 3.4e-07, 2.3e-07),      # measured 4.61e-06, 2.22e-07, 1.50e-07
    ("wave", "intconst"): (0.00051, None, 2.4e-07),      # measured 3.38e-04, 0.00e+00, 1.53e-07
    ("wave", "int_dy"): (0.00012, 1.7e-07, None),      # measured 7.99e-05, 1.09e-07, 0.00e+00
    ("slice", "baseline"): (1.7e-06, 1.2e-07, 2.5e-07),      # measured 1.09e-06, 7.93e-08, 1.61e-07
    ("slice", "offset"): (0.0005, 2.7e-06, 1.8e-07),      # measured 3.32e-04, 1.76e-06, 1.17e-07
    ("slice", "spike"): (4.5e-06, 2.3e-07, 1.7e-07),      # measured 3.00e-06, 1.47e-07, 1.07e-07
    ("slice", "intconst"): (1.8e-06, None, 1.4e-07),      # measured 1.17e-06, 0.00e+00, 9.33e-08
    ("slice", "int_dy"): (9.4e-07, 8.8e-08, None),      # measured 6.26e-07, 5.85e-08, 0.00e+00
}


def lnb_tol(kind, cls):
    """-> (dx, dgamma, dbeta) bounds of the normalised errors; None where the class asserts the quantity exactly."""
    floor = BASELINE_FLOOR if cls == "baseline" else 0.0
    return tuple(None if p is None else max(floor, LN_TOL_FACTOR * p) for p in LNB_CPU_ERR[(kind, cls)])


# ---------------------------------------------------------------------------------------------------------------------------------
# erf-GELU forward / backward inputs and tolerances
# ---------------------------------------------------------------------------------------------------------------------------------
GELU_NS = [1, 3, 4, 5, 1027, 4096]


def gelu_points(n):
    """-> (pre [n] spread over [-12, 12] with +0.0, -0.0 and both ends where they fit, dg [n] unit normal), fp32."""
    g = _g(31000 + n)
    pre = torch.rand(n, generator=g) * 24 - 12
    for i, v in enumerate([0.0, -0.0, 12.0, -12.0][:max(1, n - 1)]):
        pre[i] = v
    return pre, torch.randn(n, generator=g)


def gelu_cpu_fp32_error():
    """(forward, backward) max absolute error of torch's fp32 CPU F.gelu and its autograd over gelu_points(n), n in GELU_NS."""
    ef = eb = 0.0
    with one_thread():
        for n in GELU_NS:
            pre, dg = gelu_points(n)
            p = pre.clone().requires_grad_()
            y = F.gelu(p)
            (y * dg).sum().backward()
            ef = max(ef, float((y.detach().double() - gelu_ref(pre)).abs().max()))
            eb = max(eb, float((p.grad.double() - dg.double() * gelu_grad_ref(pre)).abs().max()))
    return ef, eb


GELU_CPU_ERR = (1.3e-06, 7e-07)          # (forward, backward); measured 8.56e-07, 4.62e-07


def gelu_tol():
    return LN_TOL_FACTOR * GELU_CPU_ERR[0], LN_TOL_FACTOR * GELU_CPU_ERR[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# Column sums and scalar sums
# ---------------------------------------------------------------------------------------------------------------------------------
def colsum_ref(x):
    """-> (float64 column sums, float64 column sums of |x|)."""
    v = x.double()
    return v.sum(0), v.abs().sum(0)


def sum_ref(x, squares=False):
    """-> (float64 sum of x (of x^2), float64 sum of |term|)."""
    v = x.double().reshape(-1)
    v = v * v if squares else v
    return v.sum(), v.abs().sum()


def colsum_int(x):
    """Column sums of an integer-valued matrix in int64, as an fp32 tensor (exact below 2^24)."""
    assert bool((x == x.round()).all())
    s = x.long().sum(0)
    assert int(s.abs().max()) < EXACT
    return s.float()


def sum_int(x, squares=False):
    assert bool((x == x.round()).all())
    v = x.long().reshape(-1)
    s = int((v * v if squares else v).sum())
    assert abs(s) < EXACT
    return torch.tensor([float(s)], dtype=torch.float32)


ACC_PREV = 1000                      # |out| before an accumulate=True call of the equality tests (an integer)
COLSUM_INT_SHAPES = [(1, 1), (3, 5), (5, 260), (64, 256), (65, 257), (16390, 8)]
COLSUM_GAUSS = (700, 130)
REDUCE_NS = [1, 3, 4, 5, 1023, 4096, 4097, 4096 * 1024 + 1]
REDUCE_GAUSS_N, REDUCE_GAUSS_SEEDS = 100003, 8
PAIR_SHAPES = [(1, 8), (5, 260), (65, 72), (129, 8), (70, 132)]


def int_bound(n, squares=False):
    """Largest |v| of n integer-valued terms (v^2 summed when squares) such that every partial sum, and the sum added to a previous
    |out| <= ACC_PREV, stays below 2^24."""
    room = (EXACT - 1 - ACC_PREV) // n
    return max(1, min(1000, math.isqrt(room) if squares else room))


def int_values(shape, n_terms, seed, squares=False):
    """Integer-valued fp32 tensor of `shape` with |v| <= int_bound(n_terms, squares): n_terms is the number of terms of one sum."""
    b = int_bound(n_terms, squares)
    return torch.randint(-b, b + 1, shape, generator=_g(seed)).float()


def colsum_gauss():
    return torch.randn(*COLSUM_GAUSS, generator=_g(41)) * 2 + 0.3


def reduce_gauss(seed):
    return torch.randn(REDUCE_GAUSS_N, generator=_g(4300 + seed)) * 1.5 + 0.1


def sums_cpu_fp32_error():
    """(column sums, scalar sum, scalar sum of squares): torch's fp32 CPU .sum(0) / .sum() against float64 on colsum_gauss() and on
    reduce_gauss(0 .. REDUCE_GAUSS_SEEDS - 1), normalised by the float64 sum of |term|, max over columns / seeds."""
    with one_thread():
        x = colsum_gauss()
        ref, norm = colsum_ref(x)
        ec = col_err(x.sum(0), ref, norm)
        es = [0.0, 0.0]
        for seed in range(REDUCE_GAUSS_SEEDS):
            v = reduce_gauss(seed)
            for sq in (False, True):
                ref, norm = sum_ref(v, sq)
                got = (v * v).sum() if sq else v.sum()
                es[sq] = max(es[sq], col_err(got, ref, norm))
    return ec, es[0], es[1]


SUMS_CPU_ERR = (4.8e-08, 1.8e-08, 1.6e-07)          # measured 3.20e-08, 1.14e-08, 1.04e-07


def sums_tol():
    return tuple(LN_TOL_FACTOR * p for p in SUMS_CPU_ERR)


# ---------------------------------------------------------------------------------------------------------------------------------
# GEMM operand rows, from the format definitions
# ---------------------------------------------------------------------------------------------------------------------------------
OPERAND_FORMATS = ["bf16", "bf16x3_act", "bf16x3_w"]
OPERAND_SHAPES = [(1, 1), (3, 8), (5, 257), (64, 64), (70, 130), (129, 61)]


def _bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


# ties of the bf16 rounding (low half 0x8000: to the even upper half), values whose residual lo = bf16(v - hi) is subnormal or
# zero, both zeros, fp32 subnormals, and the neighbourhood of the largest finite bf16 (0x7F7F0000) up to the last value that
# still rounds to it (0x7F7F7FFF; the tie above it rounds to infinity and is left out: finite operands only)
OPERAND_EDGES = torch.cat([
    _bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000]),                      # ties: 1 + 2^-8 -> 1.0, 1 + 3 * 2^-8 -> 1 + 2^-6
    torch.tensor([2.0 ** -120 * (1 + 2.0 ** -10), -2.0 ** -125 * (1 + 2.0 ** -9), 2.0 ** -126 * (1 + 2.0 ** -12)]),   # lo subnormal
    torch.tensor([-0.0, 0.0, 1.5, -3.0, 2.0 ** -126]),                             # lo zero
    _bits([0x7F7F0000, 0x7F7F7FFF, 0x7F7E8000, 0x7F7EFFFF, 0xFF7F0000, 0xFF7F7FFF, 0x7F7F0001, 0xFF7E8001]),
    _bits([0x00000001, 0x00400000, 0x80000003, 0x007FFFFF]),                      # fp32 subnormals
    torch.tensor([1.00390625 + 2.0 ** -16, 0.1, -0.1, 3.0e38]),
]).float()


def operand_values(rows, cols, seed=0):
    """[rows, cols] fp32: normal values over eight decades with OPERAND_EDGES (as many as fit) at the front of the matrix."""
    g = _g(52000 + 1000 * seed + 7 * rows + cols)
    x = torch.randn(rows, cols, generator=g) * (10.0 ** torch.randint(-4, 5, (rows, cols), generator=g).float())
    flat = x.reshape(-1)
    m = min(flat.numel(), OPERAND_EDGES.numel())
    flat[:m] = OPERAND_EDGES[:m]
    return flat.reshape(rows, cols)


def pad64(n):
    return (n + 63) // 64 * 64


def operand_ref(x, fmt, transpose=False, kp=None):
    """kx_to_operand's output from the definition: O = x^T if transpose else x, [orows, K]; K zero-padded to kp (default: the next
    multiple of 64); rows [hi] (bf16), [hi | hi | lo] (bf16x3 activation rows) or [hi | lo | hi] (bf16x3 weight rows), every plane
    kp wide, hi = bf16(v), lo = bf16(v - float(hi)) (the subtraction is exact in fp32).  -> bf16 [orows, kp or 3 kp]."""
    o = x.detach().cpu().float()
    o = o.t().contiguous() if transpose else o.contiguous()
    orows, K = o.shape
    kp = pad64(K) if kp is None else kp
    assert kp >= K
    v = torch.zeros(orows, kp, dtype=torch.float32)
    v[:, :K] = o
    hi = R.pack_bf16(v)
    if fmt == "bf16":
        return hi.contiguous()
    lo = R.pack_bf16(v - hi.float())
    planes = {"bf16x3_act": [hi, hi, lo], "bf16x3_w": [hi, lo, hi]}[fmt]
    return torch.cat(planes, dim=1).contiguous()
