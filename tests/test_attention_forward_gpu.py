"""The forward attention kernels (kx_attention, csrc/kx_attention.hip) against the float64 reference of tests/attention_ref.py.

tests/test_attention_ref.py shows on the CPU that these inputs and bounds accept a right kernel and reject kernels that drop or
double a key, walk the causal block pairs wrongly, skip a rescale or mix up heads or batch rows; the bounds and their derivation
are in the docstring of attention_ref.py.  Every comparison below goes through attention_ref's probe_ratio / parity_ratio /
lse_ratio and verdict, the code the CPU file runs its mutants through.

kx_attention's dispatch (no dropout, no KX_PREC_F16CHL rows) and the tests that launch each branch:
  KX_PREC_F16C    attn_f16s_kernel<causal / unmasked>        test_key_set_probe, test_parity, test_spike..., test_lse_out [f16c]
  KX_PREC_F16     attn_bf16_v2_kernel<causal / unmasked, F16> test_key_set_probe, test_parity, test_spike... [fp16]
  KX_PREC_BF16, key 2 = 1   attn_bf16_kernel<causal / unmasked>   test_key_set_probe [bf16-v1]
  KX_PREC_BF16    attn_bf16_v2_kernel<causal / unmasked>      test_key_set_probe, test_parity, test_spike..., test_lse_out,
                                                              test_strided_rows... [bf16]
  KX_PREC_F32     attn_f32_mfma_kernel<causal / unmasked>     the same five [fp32]
  KX_PREC_F32, key 2 = 1    attn_f32_kernel<causal / unmasked>    test_key_set_probe, test_parity, test_lse_out [fp32-valu]
  the refusal of lse_out under KX_PREC_F16                    test_fp16_with_lse_out_is_refused_and_launches_nothing
B = 2, H = 3 unless stated: an odd head count and a second batch row, different inputs for every (b, h)."""
import ctypes as C

import pytest
import torch

import attention_ref as AR
from kosmosx import _hip
from kosmosx import ops

pytestmark = pytest.mark.gpu

B, H = 2, 3
MASKS = [True, False]
MASK_IDS = ["causal", "unmasked"]
LSE_SHAPES = {True: [(1, 1), (65, 65), (257, 257), (640, 640)], False: [(64, 321), (385, 130)]}


def _launch(name, q, k, v, causal, out_dtype=torch.float32, lse_out=None):
    """One kx_attention launch of configuration `name` on device copies -> the output on the CPU."""
    lib = _hip.load()
    key2 = 1 if name in ("fp32-valu", "bf16-v1") else 0
    lib.kx_set_tuning(2, key2)
    try:
        out = ops.attention(q.cuda(), k.cuda(), v.cuda(), causal, out_dtype=out_dtype, f16c=name == "f16c", lse_out=lse_out)
        torch.cuda.synchronize()
    finally:
        lib.kx_set_tuning(2, 0)
    return out.cpu()


def _label(test, name, causal):
    return f"{test}, {name}, {'causal' if causal else 'unmasked'}"


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", list(AR.CONFIGS))
def test_key_set_probe(name, causal):
    """q = 0, integer v: every P is exactly 1, l and the P V sums are integers below 2^24, so a row of the output is the exact
    mean of the value rows its query sees, up to the final division: bound 2^-21 |ref| (8 fp32 ulps), where one key more or less
    moves a row by about 1 / T >= 1e-3.
    Measured on an MI355X: worst error / bound 0.24 for bf16, fp16, f16c, fp32 and bf16-v1 (causal T = 127; unmasked 0.20 at
    (128, 63)) and 0.13 for fp32-valu (T = 1025; unmasked 0.12 at (129, 257)): two fp32 ulps at the most, on all 31 shapes."""
    dtype = AR.CONFIGS[name][0]
    got = []
    for Tq, Tk in AR.shapes(causal):
        q, k, v, R = AR.case("probe", B, H, Tq, Tk, dtype, causal)
        out = _launch(name, q, k, v, causal)
        assert out.dtype == torch.float32
        got.append((AR.probe_ratio(out, R), (Tq, Tk)))
    AR.verdict(got, _label("probe", name, causal))


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", ["bf16", "fp16", "f16c", "fp32", "fp32-valu"])
def test_parity(name, causal):
    """Random inputs (q = randn * 0.35: score std 2.8), the reference on the inputs as rounded to the kernel's input dtype: the
    fp32-output launch is finite and inside the elementwise bound; the 2-byte-output launch of bf16 / fp16 is the fp32 launch
    rounded to nearest even, bit for bit.  Last case: H = 9, B = 1, T = 257 (the grid is head-fastest and tuned for H % 8 == 0).
    Measured on an MI355X: worst error / bound, causal | unmasked: bf16 0.38 (T = 511) | 0.38 (H = 9, T = 257); fp16 0.34
    (T = 31) | 0.30 (385, 130); f16c 0.37 (T = 640) | 0.30 (H = 9); fp32 0.53 (T = 640) | 0.43 (385, 130); fp32-valu 0.57 (T = 1025) |
    0.54 (129, 257).  (bf16 and fp16 sit where the float64 restatement of tests/test_attention_ref.py sits, 0.37 at T = 511 and 0.34 at T = 31;
    against the bound without attention_ref's binade term they measured 0.77 and 0.63.)"""
    dtype = AR.CONFIGS[name][0]
    got = []
    for Bc, Hc, Tq, Tk in [(B, H, tq, tk) for tq, tk in AR.shapes(causal)] + [(1, 9, 257, 257)]:
        q, k, v, R = AR.case("random", Bc, Hc, Tq, Tk, dtype, causal)
        out = _launch(name, q, k, v, causal)
        assert out.dtype == torch.float32
        got.append((AR.parity_ratio(name, out, R), (Bc, Hc, Tq, Tk)))
        if name in ("bf16", "fp16"):
            o16 = _launch(name, q, k, v, causal, out_dtype=None)
            assert o16.dtype == dtype and torch.equal(AR.bits(o16), AR.bits(out.to(dtype))), (Tq, Tk)
    AR.verdict(got, _label("parity", name, causal))


@pytest.mark.parametrize("name", ["bf16", "fp16", "f16c", "fp32"])
def test_spike_across_block_pairs(name):
    """A key k = c q[query] holding about half of its query's softmax weight (a one-hot row cannot tell a missed rescale from a
    right one).  Causal T = 640, nx = 5 — pairs (0, 4), (1, 3) and block 2 alone: (query, key) = (600, 5) second pass, first tile;
    (600, 590) second pass, diagonal tile; (300, 130) the middle block; (70, 64) first pass, a key at a tile start.  Unmasked
    (129, 321): key 320, the last of a ragged tile, for query 128, a block of one query.
    Measured on an MI355X: worst error / bound bf16 0.38, fp16 0.28, fp32 0.70, all at (300, 130); f16c 0.25 at the unmasked spike."""
    dtype = AR.CONFIGS[name][0]
    got = []
    for i, (Tq, Tk, causal, query, key) in enumerate(AR.SPIKES):
        q, k, v, R, w = AR.spike_case(dtype, i)
        assert all(0.3 <= x <= 0.7 for x in w), (i, w)
        out = _launch(name, q, k, v, causal)
        got.append((AR.parity_ratio(name, out, R), (Tq, Tk, query, key)))
    AR.verdict(got, f"spike, {name}")


@pytest.mark.parametrize("causal", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", ["bf16", "f16c", "fp32", "fp32-valu"])
def test_lse_out(name, causal):
    """lse_out [B, H, Tq] (what the backward pass rebuilds P from) against the float64 log-sum-exp of the ROUNDED inputs:
    |d| <= 2 u_p + 1e-5 max(1, |ref|); the output of the same launch stays inside the parity bound, and lse elements are all
    written (the buffer starts as NaN).
    Measured on an MI355X: worst lse error / bound, causal | unmasked: bf16 0.34 (T = 257) | 0.31 (385, 130); f16c 0.07 | 0.02; fp32
    0.06 | 0.03; fp32-valu 0.08 | 0.04 (causal T = 640 or 257, unmasked (385, 130))."""
    dtype = AR.CONFIGS[name][0]
    got, got_out = [], []
    for Tq, Tk in LSE_SHAPES[causal]:
        q, k, v, R = AR.case("random", B, H, Tq, Tk, dtype, causal)
        lse = torch.full((B, H, Tq), float("nan"), device="cuda")
        out = _launch(name, q, k, v, causal, lse_out=lse)
        got.append((AR.lse_ratio(name, lse.cpu(), R), (Tq, Tk)))
        got_out.append((AR.parity_ratio(name, out, R), (Tq, Tk)))
    AR.verdict(got_out, _label("lse launch, output", name, causal))
    AR.verdict(got, _label("lse", name, causal))


def _args(q, k, v, out, causal, prec, odt, lse=None):
    """kx_attn_args of 4-D views q [B, Tq, H, 64], k / v [B, Tk, H, 64] (any batch / row strides) and a 3-D output view."""
    a = _hip.AttnArgs()
    a.q, a.q_batch_stride, a.q_row_stride = q.data_ptr(), q.stride(0), q.stride(1)
    a.k, a.v, a.kv_batch_stride, a.kv_row_stride = k.data_ptr(), v.data_ptr(), k.stride(0), k.stride(1)
    a.out, a.out_batch_stride, a.out_row_stride, a.odt = out.data_ptr(), out.stride(0), out.stride(1), odt
    a.B, a.H, a.Tq, a.Tk = q.shape[0], q.shape[2], q.shape[1], k.shape[1]
    a.mask, a.prec = (_hip.KX_ATTN_CAUSAL if causal else _hip.KX_ATTN_FULL), prec
    a.lse_out = None if lse is None else lse.data_ptr()
    assert q.stride(2) == 64 and q.stride(3) == 1 and k.stride() == v.stride() and k.stride(2) == 64 and out.stride(2) == 1
    return a


def _call(a):
    rc = _hip.load().kx_attention(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_fp16_with_lse_out_is_refused_and_launches_nothing():
    """KX_PREC_F16 produces no lse: the call returns the documented error, and neither buffer loses its poison."""
    q, k, v, _ = AR.case("random", B, H, 65, 65, torch.float16, True)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    for odt, dt in ((_hip.KX_F32, torch.float32), (_hip.KX_F16, torch.float16)):
        out = torch.full((B, 65, H * 64), float("nan"), dtype=dt, device="cuda")
        lse = torch.full((B, H, 65), float("nan"), device="cuda")
        out0, lse0 = AR.bits(out.cpu()).clone(), AR.bits(lse.cpu()).clone()
        assert _call(_args(qd, kd, vd, out, True, _hip.KX_PREC_F16, odt, lse)) != 0
        assert "no lse" in _hip.last_error()
        assert torch.equal(AR.bits(out.cpu()), out0) and torch.equal(AR.bits(lse.cpu()), lse0)
    with pytest.raises(RuntimeError, match="no lse"):                        # ... and through the wrapper
        ops.attention(qd, kd, vd, True, lse_out=torch.zeros(B, H, 65, device="cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["bf16", "fp32"])
def test_strided_rows_and_untouched_neighbours(name):
    """kx_attn_args with nothing dense: q = columns D .. 2D of a fused [B, Tq, 3D + 64] buffer whose batch stride is padded by 128
    elements, k and v = columns of a second [B, Tk, 2D + 32] buffer, the output rows 2 .. 2 + Tq, columns 32 .. 32 + D of a
    NaN-filled [B, Tq + 3, D + 64] buffer (out_row_stride = D + 64).  Every input element outside the slices is NaN, so a read
    outside them shows in the output; the output rows are inside the parity bound, and every element of the output buffer outside
    them keeps its poison (compared as integer bits).  The same with a 2-byte output: the fp32 rows rounded to nearest even.
    T = 130 causal and (65, 200) unmasked.
    Measured on an MI355X: worst error / bound of the rows bf16 0.31, fp32 0.32, both at T = 130; no element outside them changed."""
    dtype = AR.CONFIGS[name][0]
    prec = _hip.KX_PREC_BF16 if name == "bf16" else _hip.KX_PREC_F32
    D = H * 64
    got = []
    for Tq, Tk, causal in ((130, 130, True), (65, 200, False)):
        q, k, v, R = AR.case("random", B, H, Tq, Tk, dtype, causal)
        qrow = 3 * D + 64
        qflat = torch.full((B * (Tq * qrow + 128),), float("nan"), dtype=dtype, device="cuda")
        qbuf = qflat.as_strided((B, Tq, qrow), (Tq * qrow + 128, qrow, 1))
        kvbuf = torch.full((B, Tk, 2 * D + 32), float("nan"), dtype=dtype, device="cuda")
        qv = qbuf[:, :, D:2 * D].unflatten(2, (H, 64))
        kv, vv = kvbuf[:, :, :D].unflatten(2, (H, 64)), kvbuf[:, :, D + 32:].unflatten(2, (H, 64))
        qv.copy_(q.cuda()), kv.copy_(k.cuda()), vv.copy_(v.cuda())
        rows32 = None
        for odt, odtype in ((_hip.KX_F32, torch.float32), (_hip.KX_BF16, torch.bfloat16)):
            obuf = torch.full((B, Tq + 3, D + 64), float("nan"), dtype=odtype, device="cuda")
            before = AR.bits(obuf.cpu()).clone().reshape(obuf.shape)
            oview = obuf[:, 2:2 + Tq, 32:32 + D]
            assert _call(_args(qv, kv, vv, oview, causal, prec, odt)) == 0, _hip.last_error()
            after = AR.bits(obuf.cpu()).reshape(obuf.shape)
            rows = obuf.cpu()[:, 2:2 + Tq, 32:32 + D]
            if odt == _hip.KX_F32:
                rows32 = rows
                got.append((AR.parity_ratio(name, rows, R), (Tq, Tk)))
            else:
                assert torch.equal(AR.bits(rows), AR.bits(rows32.to(torch.bfloat16))), (Tq, Tk)
            before[:, 2:2 + Tq, 32:32 + D] = 0
            after[:, 2:2 + Tq, 32:32 + D] = 0
            assert torch.equal(before, after), (Tq, Tk, odtype)
    AR.verdict(got, f"strided rows, {name}")
