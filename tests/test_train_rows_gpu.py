"""The training step's row, reduction and operand kernels (the first half of csrc/kx_backward.hip: kx_layernorm_backward,
kx_gelu_layernorm_backward, kx_colsum, kx_reduce_sum, kx_to_operand, kx_to_operand_pair, kx_gelu_backward_operand_pair, kx_transpose,
kx_gelu_forward, kx_gelu_backward) against the restatements of tests/train_rows_ref.py, which tests/test_train_rows_ref.py checks on
the CPU.  Tolerances and how errors are normalised: the docstring of train_rows_ref.py.  Sums of integer-valued inputs and everything
that only moves or rounds bits are compared for EQUALITY, whole buffers at a time, over a sentinel fill with a guard row behind them.

Which kernel a case launches, from the dispatch conditions of the launchers (there is one launch record per entry point, not per
kernel, so this is by reading them):
  layernorm_backward_impl   cols a multiple of 1024 up to 4096, or 6144, or 8192, and x / gamma / dy / dres / dx 16-byte aligned:
                            ln_bwd_fused_kernel<NV, NW, GELU_IN> with <1,4> <2,4> <3,4> <4,4> <2,12> <2,16> for 1024 .. 8192, rows split
                            over at most 512 (256 from 6144 columns) workgroups, + ln_bwd_fused_final_kernel unless dgamma is NULL
                            (want_param_grads=False: part == nullptr).  T.FUSED_COLS x T.fused_rows, plain and through
                            kx_gelu_layernorm_backward: all twelve instantiations, each against float64.
                            else cols % 4 == 0, cols <= 8192, aligned: ln_bwd_row_block_kernel (T.BLOCK_COLS);
                            else ln_bwd_row_kernel, four rows per workgroup (T.WAVE_COLS: cols % 4 != 0 or cols > 8192; T.SHIFTED_COLS
                            with x one float into its buffer: unaligned).  Both are followed by ln_bwd_param_kernel (64 columns per
                            workgroup: every T.WAVE_COLS has cols % 64 != 0) and ln_bwd_param_final_kernel.
                            rows = 16390 > 16384: slices_for stops at 256, 65 rows per slice, the last slices short or empty.
  kx_colsum                 colsum_partial_kernel's float4 branch needs c + 3 < cols, ld % 4 == 0 and a 16-byte aligned base; the
                            scalar branch takes the ragged last columns, ld = cols + 3 and the shifted source; colsum_final_kernel.
  kx_reduce_sum             reduce_partial_kernel<SQ>: min(1024, ceil(n / 4096)) workgroups: 4096 * 1024 + 1 is past the cap; the head
                            offsets 0 .. 3 floats exercise the scalar head and tail; reduce_final_kernel adds to out when accumulating.
  kx_to_operand             transpose: to_operand_kernel<true>; else ld % 4 == 0 and a 16-byte aligned source: to_operand_rows_kernel
                            (layout "aligned": ld = cols rounded up to 4); else to_operand_kernel<false> ("shifted": x[:, 1:] of a wider
                            matrix; "odd_ld": aligned base, ld % 4 == 1).
  kx_to_operand_pair        to_operand_pair_kernel<false>, kx_gelu_backward_operand_pair: <true>; + colsum_final_kernel.
  kx_transpose              fp32: transpose_kernel<float>; bf16 with rows, cols and both pitches multiples of 8: transpose_bf16_v8_kernel
                            ((72, 200), also with ld = cols + 8 and with pad_to = 64); else transpose_kernel<bf16_t>.
  kx_gelu_forward/backward  n % 4 == 0 and aligned buffers: gelu_fwd_v4_kernel / gelu_bwd_v4_kernel (n = 4, 4096); else the scalar kernels
                            (every other n, and every n one float into the buffer).

Measured on the MI355X (worst normalised error / bound over a route's shapes, printed by the tests as `fig` lines; "-" is a quantity
the class asserts exactly: dgamma == 0 on integer-constant rows, dbeta == the integer sum on integer dy):
  route        class      dx                  dgamma              dbeta
  fused        baseline   1.1e-06 / 2.0e-05   1.5e-07 / 2.0e-05   1.1e-07 / 2.0e-05
               offset     4.2e-05 / 8.8e-04   7.4e-05 / 9.6e-04   1.1e-07 / 1.0e-06
               spike      1.3e-06 / 3.3e-05   1.4e-07 / 2.7e-06   1.1e-07 / 1.0e-06
               intconst   9.1e-07 / 7.6e-06   -                   1.1e-07 / 1.1e-06
               int_dy     5.7e-07 / 3.5e-06   1.2e-07 / 8.8e-07   -
  gelu_fused   baseline   1.1e-06 / 2.0e-05   1.8e-07 / 2.0e-05   1.1e-07 / 2.0e-05
               offset     3.1e-05 / 1.2e-03   9.5e-05 / 6.8e-04   1.1e-07 / 1.1e-06
               spike      1.4e-06 / 2.8e-05   1.7e-07 / 2.9e-06   1.1e-07 / 1.0e-06
               intconst   9.3e-07 / 6.4e-06   -                   1.1e-07 / 1.4e-06
               int_dy     5.3e-07 / 3.4e-06   2.0e-07 / 1.6e-06   -
  block        baseline   1.1e-06 / 2.0e-05   1.2e-07 / 2.0e-05   1.1e-07 / 2.0e-05
               offset     1.9e-04 / 3.6e-03   1.3e-04 / 3.7e-04   1.1e-07 / 1.0e-06
               spike      8.9e-07 / 6.4e-06   1.2e-07 / 1.4e-06   1.1e-07 / 8.4e-07
               intconst   7.3e-07 / 5.2e-06   -                   1.2e-07 / 8.8e-07
               int_dy     1.1e-06 / 1.2e-05   1.0e-07 / 6.8e-07   -
  wave         baseline   4.9e-06 / 3.8e-04   1.4e-07 / 2.0e-05   1.2e-07 / 2.0e-05
               offset     1.1e-02 / 6.8e-02   1.5e-04 / 8.0e-04   1.1e-07 / 9.6e-07
               spike      4.2e-06 / 2.8e-05   8.3e-07 / 1.4e-06   1.2e-07 / 9.2e-07
               intconst   9.0e-07 / 2.0e-03   -                   1.1e-07 / 9.6e-07
               int_dy     8.0e-07 / 4.8e-04   1.5e-07 / 6.8e-07   -
  slice        baseline   1.1e-06 / 2.0e-05   6.2e-09 / 2.0e-05   1.4e-08 / 2.0e-05
               offset     1.7e-04 / 2.0e-03   1.1e-06 / 1.1e-05   8.3e-09 / 7.2e-07
               spike      1.3e-06 / 1.8e-05   6.2e-09 / 9.2e-07   8.7e-09 / 6.8e-07
               intconst   9.0e-07 / 7.2e-06   -                   6.6e-09 / 5.6e-07
               int_dy     5.0e-07 / 3.8e-06   1.1e-08 / 3.5e-07   -
  (the wave route's dx bounds are wide because torch's own operator is poor on its 1- and 3-column rows: 1.1e-2 on three values
  around 1e3; the kernel measures the same there)
  kx_colsum Gaussian 700 x 130: 4.3e-08 / 1.9e-07 in both branches; kx_reduce_sum n = 100003: 6.2e-09 / 7.2e-08, squares 4.0e-08 /
  6.4e-07; kx_gelu_forward 4.3e-07 / 5.2e-06 and kx_gelu_backward 2.7e-07 / 2.8e-06 (absolute), float4 and scalar kernels alike.
  Everything else in this file is an equality.

Two kernel findings of these tests, fixed in csrc/kx_backward.hip:
  * ln_bwd_fused_kernel at 3072 and 6144 columns, integer-constant rows: `mean *= 1.0f / COLS` was contracted into the centring
    (x - sum * inv as one fma), so the rounding error of the reciprocal (1 / 3 is not an fp32 value) reached x - mean un-rounded:
    a constant row centred to -2^-25 x instead of 0, and dgamma came out as 3e-5 |dy| instead of 0.  The mean is a division now.
  * ln_bwd_row_kernel on single-column rows (the `spike` class at 5 x 1 with dres: 5.9e-05 against 2.8e-05): g - mean(g) was
    contracted into fma(dy, gamma, -a) and returned rstd times the product's rounding residual instead of 0.  g is pinned as the
    rounded product now.
"""
import math

import pytest
import torch

import rowops_ref as R
import train_rows_ref as T
from kosmosx import _hip as H
from kosmosx import grad_ops as G
from kosmosx.ops import _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0xA5
OUT_FILL = 777.0                    # fp32 outputs that must keep what lies beyond their last column
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(R.as_bytes(a), R.as_bytes(b))


def _view(x, ld_extra=0, shift=0):
    """x's bits on the device as the [:, :cols] view (a 1-D x: as n values) of a matrix of pitch cols + ld_extra that starts `shift`
    elements into a 16-byte aligned allocation; everything around the values is NaN, so a read outside them poisons a sum."""
    flat = x.dim() == 1
    x2 = x.reshape(1, -1) if flat else x
    rows, cols = x2.shape
    ld = cols + ld_extra
    buf = torch.full((rows * ld + 16,), float("nan"), dtype=x.dtype, device=DEV)
    v = buf[shift:shift + rows * ld].view(rows, ld)[:, :cols]
    it = INT_OF[x.dtype]
    v.view(it).copy_(x2.contiguous().view(it))
    assert buf.data_ptr() % 16 == 0 and v.stride() == (ld, 1) and v.data_ptr() == buf.data_ptr() + shift * x.element_size()
    return v.reshape(-1) if flat and ld_extra == 0 else v


def _sentinel(rows, cols, dtype=torch.bfloat16):
    """[rows + 1, cols] of `dtype` filled with the sentinel byte: the last row is a guard behind the output."""
    return torch.full((rows + 1, cols * dtype.itemsize), SENTINEL, dtype=torch.uint8, device=DEV).view(dtype)


def _guard_intact(buf):
    return bool((R.as_bytes(buf[-1]) == SENTINEL).all())


def _fig(kernel, cls, what, err, tol):
    print(f"fig {kernel} {cls} {what} {err:.3e} {tol:.3e}")


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------
def _check_lnb(route, cls, rows, cols, shifted=False):
    """One (route, class, shape): dx, dgamma and dbeta against float64 with and without dres, dres leaving the parameter gradients
    alone, want_param_grads=False, caller-supplied outputs, and a second run bit for bit.  -> the CPU (dx, dgamma, dbeta) with dres."""
    gelu = route == "gelu_fused"
    inp = T.lnb_inputs(cls, rows, cols, gelu)
    ref = T.ln_backward_ref(inp["x"], inp["gamma"], inp["dy"], T.EPS, None, gelu)
    ref_res = T.add_dres(ref, inp["dres"])
    tol = T.lnb_tol(route, cls)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    if shifted:
        dev["x"] = _view(inp["x"].reshape(-1), 0, 1).view(rows, cols)
        assert dev["x"].is_contiguous() and dev["x"].data_ptr() % 16 == 4
    fn = G.gelu_layernorm_backward if gelu else G.layernorm_backward

    def run(dres, **kw):
        out = fn(dev["x"], dev["gamma"], dev["dy"], T.EPS, dres=dev["dres"] if dres else None, **kw)
        torch.cuda.synchronize()
        return out

    def cpu(out):
        return tuple(None if t is None else t.cpu() for t in out)

    with_res, plain = cpu(run(True)), cpu(run(False))
    for got, rf, tag in ((with_res, ref_res, "dres"), (plain, ref, "plain")):
        assert got[0].shape == (rows, cols) and got[1].shape == got[2].shape == (cols,)
        assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in got)
        e = T.lnb_errors(got, rf)
        for k, name in enumerate(("dx", "dgamma", "dbeta")):
            if tol[k] is not None:
                _fig(f"lnb/{route}", cls, name, e[k], tol[k])
        where = (route, cls, rows, cols, tag)
        assert e[0] <= tol[0], (where, "dx", e[0], tol[0])
        assert T.exact_where_zero(got[0], rf["dx"], rf["dx_norm"]), (where, "dx of a row without terms")
        if cls == "intconst":               # xhat is exactly zero in fp32: anything else is a wrong mean, divisor or lane
            assert float(got[1].abs().max()) == 0.0, (where, "dgamma of constant rows")
        else:
            assert e[1] <= tol[1], (where, "dgamma", e[1], tol[1])
            assert T.exact_where_zero(got[1], rf["dgamma"], rf["dgamma_norm"]), (where, "dgamma of zero terms")
        if cls == "int_dy":                 # integer terms: exact in any order, so one dropped or doubled row shows
            assert _same_bits(got[2], inp["dy"].long().sum(0).float()), (where, "dbeta of integer dy")
        else:
            assert e[2] <= tol[2], (where, "dbeta", e[2], tol[2])
            assert T.exact_where_zero(got[2], rf["dbeta"], rf["dbeta_norm"]), (where, "dbeta of zero terms")
    assert _same_bits(with_res[1], plain[1]) and _same_bits(with_res[2], plain[2])          # dres reaches dx only
    if not gelu:                                                                            # part == nullptr in the one-pass kernel
        dx, dg, db = cpu(run(False, want_param_grads=False))
        assert dg is None and db is None and _same_bits(dx, plain[0])
    dgo, dbo = torch.full((cols,), math.nan, device=DEV), torch.full((cols,), math.nan, device=DEV)
    out = run(True, dgamma_out=dgo, dbeta_out=dbo)
    assert out[1].data_ptr() == dgo.data_ptr() and out[2].data_ptr() == dbo.data_ptr()
    again = cpu(run(True))
    for a, b, c in zip(with_res, cpu(out), again):                                          # fixed summation order
        assert _same_bits(a, b) and _same_bits(a, c)
    return with_res


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("cols", T.FUSED_COLS)
@pytest.mark.parametrize("route", ["fused", "gelu_fused"])
def test_layernorm_backward_one_pass_kernel(route, cols, cls):
    for rows in T.fused_rows(cols):
        _check_lnb(route, cls, rows, cols)


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("cols", T.BLOCK_COLS)
def test_layernorm_backward_workgroup_per_row_kernel(cols, cls):
    for rows in T.BLOCK_ROWS:
        _check_lnb("block", cls, rows, cols)


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("cols", T.WAVE_COLS)
def test_layernorm_backward_wave_per_row_kernel(cols, cls):
    for rows in T.WAVE_ROWS:
        _check_lnb("wave", cls, rows, cols)


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("cols", T.SHIFTED_COLS)
def test_layernorm_backward_unaligned_x_takes_the_wave_kernel(cols, cls):
    """x one float into its buffer forces ln_bwd_row_kernel at widths the aligned kernels own (256: workgroup-per-row, 2048: one-pass).
    Both runs are within their bounds of the reference, and of each other within the sum of the two (at most twice the larger)."""
    aligned_route = "fused" if cols in T.FUSED_COLS else "block"
    for rows in T.SHIFTED_ROWS:
        a = _check_lnb("wave", cls, rows, cols, shifted=True)
        inp = T.lnb_inputs(cls, rows, cols)
        b = tuple(t.cpu() for t in G.layernorm_backward(inp["x"].to(DEV), inp["gamma"].to(DEV), inp["dy"].to(DEV), T.EPS,
                                                        dres=inp["dres"].to(DEV)))
        ref = T.ln_backward_ref(inp["x"], inp["gamma"], inp["dy"], T.EPS, inp["dres"])
        ta, tb = T.lnb_tol("wave", cls), T.lnb_tol(aligned_route, cls)
        eb = T.lnb_errors(b, ref)
        pair = (T.row_err(a[0], b[0].double(), ref["dx_norm"]), T.col_err(a[1], b[1], ref["dgamma_norm"]), T.col_err(a[2], b[2], ref["dbeta_norm"]))
        for k in range(3):
            if ta[k] is not None:
                assert eb[k] <= tb[k] and pair[k] <= ta[k] + tb[k] <= 2 * max(ta[k], tb[k]), (cls, rows, cols, k, eb[k], pair[k])


@pytest.mark.parametrize("cls", T.LNB_CLASSES)
@pytest.mark.parametrize("rows,cols", T.SLICE_CAP)
def test_layernorm_backward_past_the_slice_cap(rows, cols, cls):
    """16390 rows: the two-kernel form sums 256 slices of 65 rows (the last ones short or empty), the one-pass form 497 workgroups of
    33 rows.  int_dy makes dbeta an exact count of the rows."""
    _check_lnb("slice", cls, rows, cols)


# ---- kx_colsum ------------------------------------------------------------------------------------------------------------------
COLSUM_LAYOUTS = {"dense": (0, 0), "ld+4": (4, 0), "ld+3": (3, 0), "shifted": (0, 1)}


@pytest.mark.parametrize("rows,cols", T.COLSUM_INT_SHAPES)
def test_colsum_of_integers_is_the_integer_sum(rows, cols):
    x = T.int_values((rows, cols), rows, 100 + rows)
    want = T.colsum_int(x)
    prev = torch.randint(-T.ACC_PREV, T.ACC_PREV + 1, (cols,), generator=torch.Generator().manual_seed(rows)).float()
    for name, (extra, shift) in COLSUM_LAYOUTS.items():
        xd = _view(x, extra, shift)
        out = torch.full((cols + 5,), OUT_FILL, device=DEV)
        assert G.colsum(xd, out=out).data_ptr() == out.data_ptr()
        got = out.cpu()
        assert _same_bits(got[:cols], want), name
        assert bool((got[cols:] == OUT_FILL).all()), name                    # nothing beyond `cols` is written
        out[:cols] = prev.to(DEV)
        G.colsum(xd, out=out, accumulate=True)
        got = out.cpu()
        assert _same_bits(got[:cols], prev + want) and bool((got[cols:] == OUT_FILL).all()), name
        assert _same_bits(G.colsum(xd).cpu(), want), name                     # the wrapper's own output


def test_colsum_of_gaussian_columns_against_float64():
    x = T.colsum_gauss()
    ref, norm = T.colsum_ref(x)
    tol = T.sums_tol()[0]
    for name, extra in (("scalar", 0), ("float4", 2)):                        # ld = 130 / 132
        xd = _view(x, extra)
        got = G.colsum(xd).cpu()
        e = T.col_err(got, ref, norm)
        _fig("colsum", name, "sum", e, tol)
        assert e <= tol, (name, e, tol)
        acc = G.colsum(xd, out=got.to(DEV), accumulate=True).cpu()
        e2 = T.col_err(acc, got.double() + ref, norm + got.double().abs())
        assert e2 <= tol, (name, e2, tol)


# ---- kx_reduce_sum --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.REDUCE_NS)
def test_reduce_sum_of_integers_is_the_integer_sum(n):
    for sq in (False, True):
        v = T.int_values((n,), n, 200 + int(sq), sq)
        want = T.sum_int(v, sq)
        for off in range(4):                                                  # head of 0, 3, 2, 1 floats before the 16-byte loads
            x = _view(v, 0, off)
            assert x.data_ptr() % 16 == 4 * off
            got = G.reduce_sum(x, squares=sq).cpu()
            assert _same_bits(got, want), (n, sq, off, float(got), float(want))
            prev = float(37 * off - T.ACC_PREV // 2)
            out = torch.tensor([prev], device=DEV)
            G.reduce_sum(x, squares=sq, out=out, accumulate=True)
            assert _same_bits(out.cpu(), want + prev), (n, sq, off)


def test_reduce_sum_of_gaussian_values_against_float64():
    tols = T.sums_tol()
    for seed in range(T.REDUCE_GAUSS_SEEDS):
        v = T.reduce_gauss(seed)
        for sq in (False, True):
            ref, norm = T.sum_ref(v, sq)
            for off in (0, 1):
                got = G.reduce_sum(_view(v, 0, off), squares=sq).cpu()
                e = T.col_err(got, ref, norm)
                _fig("reduce_sum", "squares" if sq else "plain", "sum", e, tols[1 + sq])
                assert e <= tols[1 + sq], (seed, sq, off, e)


# ---- kx_to_operand --------------------------------------------------------------------------------------------------------------
def _to_operand(xd, fmt, transpose, kp):
    rows, cols = xd.shape
    orows = cols if transpose else rows
    out = _sentinel(orows, kp * (1 if fmt == "bf16" else 3))
    H.check(H.load().kx_to_operand(H.ptr(xd), H.ptr(out), rows, cols, xd.stride(0), kp, int(transpose), G.FMT[fmt], _stream()),
            "kx_to_operand")
    torch.cuda.synchronize()
    assert _guard_intact(out)
    return out[:-1].cpu()


@pytest.mark.parametrize("fmt", T.OPERAND_FORMATS)
@pytest.mark.parametrize("rows,cols", T.OPERAND_SHAPES)
def test_to_operand_whole_buffer_is_the_packed_matrix(rows, cols, fmt):
    x = T.operand_values(rows, cols)
    layouts = {"aligned": _view(x, -cols % 4, 0), "shifted": _view(x, 1, 1), "odd_ld": _view(x, -cols % 4 + 1, 0)}
    assert layouts["aligned"].stride(0) % 4 == 0 and layouts["odd_ld"].stride(0) % 4 == 1 and layouts["shifted"].data_ptr() % 16 == 4
    for transpose in (False, True):
        K = rows if transpose else cols
        for kp in sorted({T.pad64(K), (K + 7) // 8 * 8}):
            want = T.operand_ref(x, fmt, transpose, kp)
            for name, xd in layouts.items():
                got = _to_operand(xd, fmt, transpose, kp)
                assert _same_bits(got, want), (name, transpose, kp)
    assert _same_bits(G.to_operand(layouts["aligned"], fmt).cpu(), T.operand_ref(x, fmt))
    assert _same_bits(G.to_operand(layouts["shifted"], fmt, transpose_=True).cpu(), T.operand_ref(x, fmt, True))


# ---- kx_to_operand_pair / kx_gelu_backward_operand_pair -------------------------------------------------------------------------
def _pair(xd, pre=None):
    """-> (straight [rows, kp], transposed [cols, kpt], colsum [cols]) on the CPU, each checked for writes beyond it."""
    rows, cols = xd.shape
    kp, kpt = T.pad64(cols), T.pad64(rows)
    a, t = _sentinel(rows, kp), _sentinel(cols, kpt)
    cs = torch.full((cols + 3,), OUT_FILL, device=DEV)
    lib = H.load()
    ws = torch.empty(max(int(lib.kx_to_operand_pair_workspace_bytes(rows, cols)), 4096), dtype=torch.uint8, device=DEV)
    if pre is None:
        rc = lib.kx_to_operand_pair(H.ptr(xd), H.ptr(a), H.ptr(t), rows, cols, xd.stride(0), kp, kpt, H.ptr(cs), H.ptr(ws), ws.numel(),
                                    _stream())
    else:
        assert pre.stride() == xd.stride()
        rc = lib.kx_gelu_backward_operand_pair(H.ptr(xd), H.ptr(pre), H.ptr(a), H.ptr(t), rows, cols, xd.stride(0), kp, kpt, H.ptr(cs),
                                               H.ptr(ws), ws.numel(), _stream())
    H.check(rc, "operand pair")
    torch.cuda.synchronize()
    assert _guard_intact(a) and _guard_intact(t) and bool((cs[cols:] == OUT_FILL).all())
    return a[:-1].cpu(), t[:-1].cpu(), cs[:cols].cpu()


@pytest.mark.parametrize("rows,cols", T.PAIR_SHAPES)
def test_to_operand_pair_both_outputs_are_the_packed_matrix(rows, cols):
    for x in (T.operand_values(rows, cols, seed=1), T.int_values((rows, cols), rows, 300 + rows)):
        for extra in (0, 8):                                                  # dense, and a row-strided view (ld = cols + 8)
            a, t, cs = _pair(_view(x, extra))
            assert _same_bits(a, T.operand_ref(x, "bf16")) and _same_bits(t, T.operand_ref(x, "bf16", True)), extra
            if bool((x == x.round()).all()):
                assert _same_bits(cs, T.colsum_int(x)), extra
            else:
                ref, norm = T.colsum_ref(x)                                   # values over eight decades: the a-priori bound of ANY
                assert T.col_err(cs, ref, norm) <= rows * 2.0 ** -24          # order of fp32 additions; the equality is the real check
    a, t = G.to_operand_pair(_view(x))
    assert _same_bits(a.cpu(), T.operand_ref(x, "bf16")) and _same_bits(t.cpu(), T.operand_ref(x, "bf16", True))


@pytest.mark.parametrize("rows,cols", T.PAIR_SHAPES)
def test_gelu_backward_operand_pair_is_the_packed_fp32_gelu_backward(rows, cols):
    g = torch.Generator().manual_seed(400 + rows)
    cases = [(torch.rand(rows, cols, generator=g) * 12 - 6, T.operand_values(rows, cols, seed=2).clamp(-1e30, 1e30)),
             # |pre| = 30: gelu' is exactly 1 or 0, so integer dg gives integer terms and an exact bias gradient
             (torch.where(torch.rand(rows, cols, generator=g) < 0.5, -30.0, 30.0), T.int_values((rows, cols), rows, 500 + rows))]
    for k, (pre, dg) in enumerate(cases):
        dpre = G.gelu_backward(pre.to(DEV), dg.to(DEV)).cpu()                 # the fp32 kernel, held to float64 below
        for extra in (0, 8):
            a, t, cs = _pair(_view(dg, extra), _view(pre, extra))
            assert _same_bits(a, T.operand_ref(dpre, "bf16")) and _same_bits(t, T.operand_ref(dpre, "bf16", True)), (k, extra)
            if k == 1:
                assert torch.equal(dpre, torch.where(pre > 0, dg, torch.zeros(())))
                assert _same_bits(cs, T.colsum_int(dg * (pre > 0))), extra
            else:
                ref, norm = T.colsum_ref(dpre)
                assert T.col_err(cs, ref, norm) <= rows * 2.0 ** -24          # any order of fp32 additions of these terms


# ---- kx_transpose ---------------------------------------------------------------------------------------------------------------
SPECIAL_BITS = {torch.float32: [0x7FC12345, 0x7FA00001, -0x3FFFFF, 0x7F800000, -0x800000, -0x80000000, 0x00000001],
                torch.bfloat16: [0x7FC1, 0x7FA1, -0x3F, 0x7F80, -0x80, -0x8000, 0x0001]}     # NaN payloads, +-inf, -0.0, a subnormal


def _transpose_values(rows, cols, dt):
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)).to(dt)
    flat = x.view(INT_OF[dt]).reshape(-1)
    sp = torch.tensor(SPECIAL_BITS[dt], dtype=INT_OF[dt])
    m = min(flat.numel(), sp.numel())
    flat[flat.numel() - m:] = sp[:m]                                          # the matrix's last elements: the ragged tiles
    return x


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (72, 200)])
def test_transpose_moves_bits(rows, cols, dt):
    x = _transpose_values(rows, cols, dt)
    it = INT_OF[dt]
    want = x.view(it).t().contiguous()
    lib = H.load()
    for extra in (0, 8, 3):
        xd = _view(x, extra)
        assert torch.equal(G.transpose(xd).cpu().view(it), want), extra
        for pad in (32, 64):
            rp = (rows + pad - 1) // pad * pad
            got = G.transpose(xd, pad_to=pad).cpu().view(it)                   # the wrapper zero-fills the padding columns
            assert got.shape == (cols, rp) and torch.equal(got[:, :rows], want) and not bool(got[:, rows:].any())
            dst = _sentinel(cols, rp, dt)                                      # the kernel itself writes the [cols, rows] block only
            H.check(lib.kx_transpose(H.ptr(xd), H.ptr(dst), rows, cols, xd.stride(0), rp, H.KX_F32 if dt == torch.float32 else H.KX_BF16,
                                     _stream()), "kx_transpose")
            torch.cuda.synchronize()
            raw = dst.cpu()
            assert torch.equal(raw[:-1].view(it)[:, :rows], want), (extra, pad)
            assert bool((R.as_bytes(raw[:-1])[:, rows * dt.itemsize:] == SENTINEL).all()) and _guard_intact(dst), (extra, pad)


# ---- kx_gelu_forward / kx_gelu_backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.GELU_NS)
def test_gelu_forward_and_backward_against_float64(n):
    pre, dg = T.gelu_points(n)
    want_f, want_b = T.gelu_ref(pre), dg.double() * T.gelu_grad_ref(pre)
    tol_f, tol_b = T.gelu_tol()
    outs = []
    for shift in (0, 1):                       # aligned: the float4 kernels when n % 4 == 0; one float in: the scalar kernels
        p, d = _view(pre, 0, shift), _view(dg, 0, shift)
        y, b = G.gelu(p).cpu(), G.gelu_backward(p, d).cpu()
        ef, eb = float((y.double() - want_f).abs().max()), float((b.double() - want_b).abs().max())
        _fig("gelu", "v4" if n % 4 == 0 and shift == 0 else "scalar", "forward", ef, tol_f)
        _fig("gelu", "v4" if n % 4 == 0 and shift == 0 else "scalar", "backward", eb, tol_b)
        assert y.shape == b.shape == (n,) and ef <= tol_f and eb <= tol_b, (n, shift, ef, eb)
        outs.append((y, b))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1])          # float4 and scalar kernels: same bits


@pytest.mark.parametrize("n,shift", [(4, 0), (4, 1), (3, 0)])
def test_gelu_saturates_exactly(n, shift):
    """|x| = 30: erf is +-1 and the density is 0 in fp32: gelu(30) == 30, |gelu(-30)| == 0, gelu'(30) == 1, gelu'(-30) == 0."""
    pre = torch.tensor([30.0, -30.0, 30.0, -30.0][:n])
    p, one = _view(pre, 0, shift), _view(torch.ones(n), 0, shift)
    y, b = G.gelu(p).cpu(), G.gelu_backward(p, one).cpu()
    assert y.abs().tolist() == [30.0, 0.0, 30.0, 0.0][:n] and float(y[0]) == 30.0
    assert b.abs().tolist() == [1.0, 0.0, 1.0, 0.0][:n] and float(b[0]) == 1.0
