"""train_rows_ref.py checked on the CPU: every reference against something independent of it (torch float64 autograd, torch's own
bf16 converter, Python int arithmetic), the conditions the equality assertions of test_train_rows_gpu.py rest on, and every pinned
tolerance against a re-measured fp32 CPU baseline."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
import train_rows_ref as T
from kosmosx import grad_ops as G


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------
def _autograd64(x64, gamma, dy, dres):
    cols = x64.shape[1]
    x = x64.clone().requires_grad_()
    gam, bet = gamma.double().requires_grad_(), torch.zeros(cols, dtype=torch.float64, requires_grad=True)
    (F.layer_norm(x, (cols,), gam, bet, R._eps32(T.EPS)) * dy.double()).sum().backward()
    return (x.grad if dres is None else x.grad + dres.double()), gam.grad, bet.grad


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("gelu", [False, True])
def test_ln_backward_ref_matches_torch_float64_autograd(gelu, cls):
    for rows, cols in [(4, 3), (5, 65), (7, 260), (3, 1024)]:
        inp = T.lnb_inputs(cls, rows, cols, gelu)
        x64 = F.gelu(inp["x"].double()).float().double() if gelu else inp["x"].double()
        for dres in (None, inp["dres"]):
            ref = T.ln_backward_ref(inp["x"], inp["gamma"], inp["dy"], T.EPS, dres, gelu)
            dx, dg, db = _autograd64(x64, inp["gamma"], inp["dy"], dres)
            assert all(v.dtype == torch.float64 for v in ref.values())
            # 1e-13 on well-conditioned O(1) gradients; LayerNorm's condition number on x is |x| * rstd (~3e3 for three values around
            # 1e3, or for constant rows where rstd = 316) and both float64 evaluations carry it, |dx| reaches 1e3 there as well
            cond = max(1.0, float((x64.abs() / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + T.EPS)).max()))
            for got, want in ((ref["dx"], dx), (ref["dgamma"], dg), (ref["dbeta"], db)):
                assert float((got - want).abs().max()) <= 1e-13 * cond * max(1.0, float(want.abs().max())), (rows, cols, cond)
            assert torch.equal(ref["dbeta_norm"], inp["dy"].double().abs().sum(0))
            assert bool((ref["dgamma_norm"] + 1e-300 >= ref["dgamma"].abs()).all())


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
def test_ln_backward_ref_of_single_column_rows_is_exactly_zero(cls):
    """cols = 1: x - mean is exactly zero, so dgamma = 0 and dx = dres.  (torch's float64 operator returns dgamma ~ 1e-11 here on the
    `offset` class: its own rounding, which is why this shape is checked by the closed form and not against it.)"""
    for rows in (1, 4, 7):
        inp = T.lnb_inputs(cls, rows, 1)
        ref = T.ln_backward_ref(inp["x"], inp["gamma"], inp["dy"], T.EPS, inp["dres"])
        assert float(ref["dgamma"].abs().max()) == 0.0 and float(ref["dgamma_norm"].max()) == 0.0
        assert torch.equal(ref["dx"], inp["dres"].double()) and torch.equal(ref["dbeta"], inp["dy"].double().sum(0))


def test_ln_backward_input_classes_are_what_they_claim():
    for gelu in (False, True):
        for rows, cols in [(7, 3), (7, 260), (5, 3072), (4, 12290)]:
            i = T.lnb_inputs("intconst", rows, cols, gelu)
            k = (torch.arange(rows) % 7 + (6 if gelu else 3)).float()
            assert torch.equal(i["x"], k[:, None].expand(rows, cols)) and float(k.max()) * cols < T.EXACT
            if gelu:                                     # the activation the kernels normalise is the same integer, exactly
                assert torch.equal(T.gelu_ref(i["x"]).float(), i["x"])
            ref = T.ln_backward_ref(i["x"], i["gamma"], i["dy"], T.EPS, None, gelu)
            assert float(ref["dgamma"].abs().max()) == 0.0 and float(ref["dgamma_norm"].max()) == 0.0
            g = i["dy"].double() * i["gamma"].double()
            closed = (g - g.mean(-1, keepdim=True)) / math.sqrt(R._eps32(T.EPS))
            assert float((ref["dx"] - closed).abs().max()) <= 1e-12 * float(closed.abs().max())
            off = T.lnb_inputs("offset", rows, cols, gelu)["x"].double().mean(-1)
            assert bool((off > 900).all()) and bool((off < 1400).all())
            sp = T.lnb_inputs("spike", rows, cols, gelu)["x"]
            assert bool(((sp == 1e4).sum(-1) == 1).all())
            d = T.lnb_inputs("int_dy", rows, cols, gelu)["dy"]
            assert bool((d == d.round()).all()) and float(d.abs().max()) == 4.0
    # int_dy: every partial sum of dbeta is an integer below 2^24 at the largest row count any test uses
    assert 4 * max(r for shapes in T.LNB_ROUTES.values() for r, _ in shapes) < T.EXACT


def test_every_route_of_the_launcher_has_its_shapes():
    """The shape lists against the dispatch conditions of layernorm_backward_impl, restated: one-pass kernel for cols a multiple of
    1024 up to 4096, 6144 and 8192; else the workgroup-per-row kernel for cols % 4 == 0 up to 8192; else the wave-per-row kernel."""
    def fused(c):
        return c % 1024 == 0 and (1 <= c // 1024 <= 4 or c // 1024 in (6, 8))
    assert all(fused(c) for c in T.FUSED_COLS) and len(T.FUSED_COLS) == 6
    assert all(not fused(c) and c % 4 == 0 and c <= 8192 for c in T.BLOCK_COLS)
    assert all(c % 4 != 0 or c > 8192 for c in T.WAVE_COLS) and all(c % 64 != 0 for c in T.WAVE_COLS)
    assert all(c % 4 == 0 and c <= 8192 for c in T.SHIFTED_COLS)
    for c in T.FUSED_COLS:                            # workgroups of two rows, the last one of one row
        target, rows = (256 if c >= 6144 else 512), T.fused_rows(c)[-1]
        rpb = -(-rows // target)
        assert rows == target + 1 and rpb == 2 and rows % rpb == 1
    (r1, c1), (r2, c2) = T.SLICE_CAP                  # slices_for: min(256, ceil(rows / 64)) slices of ceil(rows / slices) rows
    ns = min(256, -(-r1 // 64))
    rps = -(-r1 // ns)
    assert r1 > 16384 and ns == 256 and rps == 65 and r1 % rps != 0 and not fused(c1) and c1 % 4 == 0 and fused(c2) and r2 == r1


# ---- GELU -----------------------------------------------------------------------------------------------------------------------
def test_gelu_refs_match_torch_float64():
    x = torch.cat([torch.linspace(-12, 12, 4801, dtype=torch.float64), torch.tensor([0.0, -0.0, 30.0, -30.0], dtype=torch.float64)])
    p = x.clone().requires_grad_()
    y = F.gelu(p)
    y.sum().backward()
    assert float((T.gelu_ref(x) - y.detach()).abs().max()) < 1e-14
    assert float((T.gelu_grad_ref(x) - p.grad).abs().max()) < 1e-12
    # the exact cases the GPU test asserts hold for the reference rounded to fp32
    e = torch.tensor([30.0, -30.0])
    assert T.gelu_ref(e).float().abs().tolist() == [30.0, 0.0] and T.gelu_grad_ref(e).float().tolist() == [1.0, 0.0]
    for n in T.GELU_NS:
        pre, dg = T.gelu_points(n)
        assert pre.shape == dg.shape == (n,) and float(pre.abs().max()) <= 12.0 and float(pre[0]) == 0.0
    pre, _ = T.gelu_points(4096)
    assert math.copysign(1.0, float(pre[1])) == -1.0 and float(pre[1]) == 0.0 and float(pre.min()) == -12.0 and float(pre.max()) == 12.0


# ---- operand packers ------------------------------------------------------------------------------------------------------------
def test_operand_edges_hold_the_cases_they_name():
    x = T.OPERAND_EDGES
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(x.to(torch.bfloat16).float()).all())
    low = x.view(torch.int32) & 0xFFFF
    assert int((low == 0x8000).sum()) >= 5                                       # ties of the rounding
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16).float()
    tiny = 2.0 ** -126
    assert bool(((lo != 0) & (lo.abs() < tiny)).any())                           # subnormal residual
    assert bool(((lo == 0) & (x != 0)).any())                                    # zero residual
    assert bool(((x != 0) & (x.abs() < tiny)).any())                             # fp32 subnormal inputs
    assert float(hi.float().abs().max()) == float(torch.finfo(torch.bfloat16).max)
    bits = (x.view(torch.int32) & 0x7FFFFFFF).tolist()
    assert 0x7F7F7FFF in bits and 0 in bits and bool((x.view(torch.int32) == -(1 << 31)).any())    # last value below infinity, +0, -0
    # round-to-even of the ties: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert R.pack_bf16(x[:2]).float().tolist() == [1.0, 1.015625]


@pytest.mark.parametrize("rows,cols", T.OPERAND_SHAPES + T.PAIR_SHAPES)
def test_operand_ref_against_torchs_converter(rows, cols):
    x = T.operand_values(rows, cols)
    assert x.shape == (rows, cols) and bool(torch.isfinite(x).all())
    for tr in (False, True):
        o = x.t().contiguous() if tr else x
        orows, K = o.shape
        for kp in (None, (K + 7) // 8 * 8):
            kpv = T.pad64(K) if kp is None else kp
            hi = torch.zeros(orows, kpv, dtype=torch.bfloat16)
            hi[:, :K] = o.to(torch.bfloat16)
            lo = torch.zeros(orows, kpv, dtype=torch.bfloat16)
            lo[:, :K] = (o - o.to(torch.bfloat16).float()).to(torch.bfloat16)
            for fmt, planes in (("bf16", [hi]), ("bf16x3_act", [hi, hi, lo]), ("bf16x3_w", [hi, lo, hi])):
                got = T.operand_ref(x, fmt, tr, kp)
                assert got.dtype == torch.bfloat16 and got.shape == (orows, len(planes) * kpv)
                assert torch.equal(R.as_bytes(got), R.as_bytes(torch.cat(planes, dim=1)))
            # the padding is +0.0 bits in every plane
            assert not bool(R.as_bytes(T.operand_ref(x, "bf16x3_w", tr, kp)).reshape(orows, 3, kpv, 2)[:, :, K:].any())


def test_operand_formats_are_the_wrappers():
    assert list(G.FMT) == T.OPERAND_FORMATS and [G.FMT[f] for f in T.OPERAND_FORMATS] == [1, 2, 3]


# ---- integer-exact sums ---------------------------------------------------------------------------------------------------------
def test_integer_sums_against_python_ints():
    x = T.int_values((65, 7), 65, 3)
    want = [sum(int(v) for v in x[:, c].tolist()) for c in range(7)]
    assert T.colsum_int(x).tolist() == [float(w) for w in want]
    v = T.int_values((4097,), 4097, 4)
    assert T.sum_int(v).tolist() == [float(sum(int(a) for a in v.tolist()))]
    v = T.int_values((4097,), 4097, 4, squares=True)
    assert T.sum_int(v, True).tolist() == [float(sum(int(a) ** 2 for a in v.tolist()))]
    with pytest.raises(AssertionError):
        T.colsum_int(torch.tensor([[0.5]]))
    with pytest.raises(AssertionError):
        T.sum_int(torch.full((3,), 2.0 ** 23))


def test_integer_generators_keep_every_partial_sum_exact():
    """n * max|v| (n * max v^2 for squares), plus the previous |out| of an accumulate call, below 2^24: every fp32 partial sum in any
    order is an integer below 2^24, hence exact."""
    for n in T.REDUCE_NS:
        for sq in (False, True):
            b = T.int_bound(n, sq)
            v = T.int_values((n,), n, 11, sq)
            m = int(v.abs().max())
            assert 1 <= m <= b and n * (b * b if sq else b) + T.ACC_PREV < T.EXACT, (n, sq)
            assert bool((v == v.round()).all())
    assert T.int_bound(T.REDUCE_NS[-1]) == 3 and T.int_bound(T.REDUCE_NS[-1], True) == 1 and T.int_bound(1) == 1000
    for rows, cols in T.COLSUM_INT_SHAPES + T.PAIR_SHAPES:
        x = T.int_values((rows, cols), rows, 12)
        assert rows * int(x.abs().max()) + T.ACC_PREV < T.EXACT and rows * T.int_bound(rows) + T.ACC_PREV < T.EXACT


# ---- pinned tolerances ----------------------------------------------------------------------------------------------------------
def _window(measured, pinned, what):
    assert measured <= pinned <= 4 * measured or (measured == 0.0 and pinned == 0.0), (what, measured, pinned)


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("kind", list(T.LNB_ROUTES))
def test_layernorm_backward_tolerances_are_tied_to_the_fp32_cpu_baseline(kind, cls):
    m = T.lnb_cpu_fp32_error(kind, cls)
    pinned, tol = T.LNB_CPU_ERR[(kind, cls)], T.lnb_tol(kind, cls)
    print(f"{kind} {cls}: torch fp32 CPU (dx, dgamma, dbeta) " + ", ".join(f"{v:.3e}" for v in m) + f"; pinned {pinned}; bounds {tol}")
    exact = {"intconst": 1, "int_dy": 2}.get(cls)
    for k, name in enumerate(("dx", "dgamma", "dbeta")):
        if k == exact:
            assert pinned[k] is None and tol[k] is None
            continue
        _window(m[k], pinned[k], (kind, cls, name))
        assert tol[k] == max(2e-5 if cls == "baseline" else 0.0, 4 * pinned[k])
    assert T.LN_TOL_FACTOR == 4.0


def test_gelu_and_sum_tolerances_are_tied_to_the_fp32_cpu_baseline():
    m = T.gelu_cpu_fp32_error()
    print(f"gelu: torch fp32 CPU max|err| forward {m[0]:.3e}, backward {m[1]:.3e}; pinned {T.GELU_CPU_ERR}; bounds {T.gelu_tol()}")
    for k in range(2):
        _window(m[k], T.GELU_CPU_ERR[k], ("gelu", k))
        assert T.gelu_tol()[k] == 4 * T.GELU_CPU_ERR[k]
    s = T.sums_cpu_fp32_error()
    print("sums: torch fp32 CPU (colsum, sum, sum of squares) " + ", ".join(f"{v:.3e}" for v in s) + f"; pinned {T.SUMS_CPU_ERR}")
    for k in range(3):
        _window(s[k], T.SUMS_CPU_ERR[k], ("sums", k))
        assert T.sums_tol()[k] == 4 * T.SUMS_CPU_ERR[k] and T.SUMS_CPU_ERR[k] > 0


# ---- the wrappers refuse what the C entries cannot express (host only: nothing is launched) ---------------------------------------
def test_layernorm_backward_wrappers_refuse_strided_views():
    """kx_layernorm_backward / kx_gelu_layernorm_backward take no row pitch: a view with a pitch would be read as if dense and give a
    plausible wrong gradient.  The check comes before anything touches the device, so it is tested on CPU tensors through the
    function the wrappers call."""
    x = torch.zeros(6, 16)
    G._need_dense(x, x[:3], None, x.reshape(-1)[4:20].view(1, 16))
    for bad in (x[:, :8], x[::2], x.t()):
        with pytest.raises(ValueError, match="contiguous"):
            G._need_dense(x, bad)
        for fn in (G.layernorm_backward, G.gelu_layernorm_backward):
            good, gam = torch.zeros(*bad.shape), torch.zeros(bad.shape[1])
            for args, kw in (((bad, gam, good), {}), ((good, gam, bad), {}), ((good, gam, good), {"dres": bad})):
                with pytest.raises(ValueError, match="contiguous"):
                    fn(*args, **kw)
