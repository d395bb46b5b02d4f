"""kx_attention_extend (csrc/kx_attention.hip: the EXT instantiations of the three causal flash kernels + the cache append at a
row offset) against the float64 reference of tests/extend_ref.py.

H = 2, Tmax = 288, cache rows >= P NaN before every launch.  The (P, Tn) cases put P and P + Tn on, before and after the 64-key
tile edges and the 128-query block edges, run the pair pass (Tn > 128: query blocks (0, 1) in one workgroup), a single query on a
long cache and P + Tn = Tmax.  Both cache layouts, every output form of every precision, the partial row statistics.

Bounds, from the same kernels' existing tests: fp32 rel_err < 2e-5 (test_attention_f32), bf16 < 1.5e-2 (test_attention_bf16),
f16c max |err| < 3e-6 * max(1, |ref|max) at q * 0.6, k * 1.5 (test_attention_f16c_split_products); the statistics as
test_attention_partial_row_stats.  A 2-byte / KX_F16C output form adds its format's rounding to the bound and must be the
rounding of the fp32 form bit for bit.

Bit equality: per query the key tiles start at 0 in both launches, a query's column never mixes with another's and a skipped
tile is an all-masked one, so rows P .. P + Tn - 1 of the full causal kx_attention launch over the P + Tn rows are the extend
launch's output bit for bit — asserted for the fp32 and the f16c kernel.
The bf16 kernel is NOT bit-equal, and not because of a sum: its rescale factor is alpha = exp2(fma(m_old, log2e, -(m_new *
log2e))), and with m_new == m_old the fma returns the rounding residue of m * log2e, not 0 — alpha is 1 +- 1 ulp when |m * log2e|
is a few units.  A wave runs a key tile when ANY of its 32 queries has a key there, so a query whose own keys ended in the tile
before has O and l multiplied by that alpha once more; which queries share a wave depends on P (query i sits in row i of the
launch, not row P + i), so the two launches differ where (P + i) and i fall into different waves' last tiles.  First seen at
(P, Tn) = (63, 2): max 1 ulp.  Bound for that kernel, from the mechanism: the extra tile comes after the query's last own tile and
at most once per launch (a wave spans 32 queries, a tile 64 keys); O and l are rounded once each after the multiply (2^-24 each,
relative) and 1 / l and O / l once more — under 8 * 2^-24 per launch and element, both launches: |full - out| <= 2^-20 |out|, plus
2^-20 of the row's largest |value| for elements that cancel.  Its float64 bound stays as for every case."""
import pytest
import torch

import decode_ref as DR
import extend_ref as ER
from kosmosx import _hip
from kosmosx import ops

pytestmark = pytest.mark.gpu

HEADS, TMAX = 2, 288
D = HEADS * 64
CASES = [(0, 1), (0, 64), (0, 130), (1, 1), (5, 33), (63, 2), (64, 64), (65, 127), (127, 129), (128, 128), (100, 188), (200, 17),
         (287, 1)]
# precision -> (torch dtype of qkv and caches, q scale, k scale, nan_to_num in the reference, the non-fp32 output form)
PRECS = {"fp32": (torch.float32, 0.35, 1.0, True, "bf16"), "bf16": (torch.bfloat16, 0.35, 1.0, False, "bf16"),
         "f16c": (torch.float32, 0.6, 1.5, True, "f16c")}


def _row_major(c):
    return c.permute(0, 2, 1, 3).contiguous()                      # [B, H, Tmax, 64] -> [B, Tmax, H, 64]


def _launch(prec, qkv, kc, vc, P, layout, form, stats=False):
    """One launch on device copies -> (out, kcache after, vcache after, stats) on the CPU, the caches back in [B, H, Tmax, 64]."""
    rm = layout == "row_major"
    kd, vd = (_row_major(kc) if rm else kc).cuda(), (_row_major(vc) if rm else vc).cuda()
    st = torch.zeros(qkv.shape[0], HEADS, 2, device="cuda") if stats else None
    lib = _hip.load()
    try:
        if rm:
            lib.kx_set_tuning(9, 1)
        out = ops.attention_extend(qkv.cuda(), kd, vd, P, out_dtype=form, stats_out=st, layout=layout, f16c=prec == "f16c")
        torch.cuda.synchronize()
    finally:
        if rm:
            lib.kx_set_tuning(9, 0)
    k1, v1 = kd.cpu(), vd.cpu()
    return out.cpu(), (_row_major(k1) if rm else k1), (_row_major(v1) if rm else v1), None if st is None else st.cpu()


def _err(prec, out, ref):
    if prec == "f16c":
        return float((out.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    return DR.rel_err64(out, ref)


BOUND = {"fp32": 2e-5, "bf16": 1.5e-2, "f16c": 3e-6}


def _full_causal(prec, qkv, kc, vc, B, P, Tn):
    """Rows P .. P + Tn - 1 of ops.attention(causal=True) over the concatenated P + Tn rows (the rows < P get queries of their own)."""
    q, kn, vn = ER.new_rows(qkv, B, HEADS)                                                   # [B, H, Tn, 64]
    g = torch.Generator().manual_seed(P)
    q0 = (torch.randn(B, HEADS, P, 64, generator=g) * 0.35).to(qkv.dtype)
    cat = lambda a, b: torch.cat([a, b], 2).permute(0, 2, 1, 3).contiguous().cuda()          # -> [B, P + Tn, H, 64]
    o = ops.attention(cat(q0, q), cat(kc[:, :, :P], kn), cat(vc[:, :, :P], vn), True, out_dtype=torch.float32, f16c=prec == "f16c")
    return o[:, P:].reshape(B * Tn, D).cpu()


def _check_case(prec, B, P, Tn):
    dtype, qs, ks, n2n, form2 = PRECS[prec]
    qkv, kc, vc = ER.random_extend(B, HEADS, TMAX, P, Tn, dtype, seed=10000 + 300 * P + Tn, q_scale=qs, k_scale=ks)
    ref, k_ref, v_ref = ER.extend_attention_ref(qkv, kc, vc, P, n2n)
    rms = float(ref.pow(2).mean().sqrt())
    worst = 0.0
    for layout in ("head_major", "row_major"):
        out, k1, v1, st = _launch(prec, qkv, kc, vc, P, layout, "f32", stats=True)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B * Tn, D) and bool(torch.isfinite(out).all())
        e = _err(prec, out, ref)
        worst = max(worst, e)
        print(f"attention_extend {prec} B={B} P={P} Tn={Tn} {layout}: error {e:.3e} (bound {BOUND[prec]:.1e})")
        assert e < BOUND[prec], (prec, P, Tn, layout, e)
        # rows [P, P + Tn) = the qkv rows' k | v bit for bit, rows < P untouched, rows >= P + Tn still the poison
        kn, vn = ER.new_rows(qkv, B, HEADS)[1:]
        assert torch.equal(DR.bits(k1[:, :, P:P + Tn]), DR.bits(kn)) and torch.equal(DR.bits(v1[:, :, P:P + Tn]), DR.bits(vn))
        assert torch.equal(DR.bits(k1[:, :, :P]), DR.bits(kc[:, :, :P])) and torch.equal(DR.bits(v1[:, :, :P]), DR.bits(vc[:, :, :P]))
        assert bool(torch.isnan(k1[:, :, P + Tn:].float()).all()) and bool(torch.isnan(v1[:, :, P + Tn:].float()).all())
        assert torch.equal(DR.bits(k1), DR.bits(k_ref)) and torch.equal(DR.bits(v1), DR.bits(v_ref))
        # statistics (sum, M2 about the mean) per (row, head), as test_attention_partial_row_stats bounds them
        fin = ops.row_stats_finalize(st.cuda(), 64, 1e-5).cpu()
        assert float((fin[:, 0] - out.mean(1)).abs().max()) < 2e-5
        rstd = 1 / torch.sqrt(out.var(1, unbiased=False) + 1e-5)
        assert float(((fin[:, 1] - rstd) / rstd).abs().max()) < 5e-5
        if prec == "f16c":
            assert float((st[:, :, 0].double() - ref.view(B * Tn, HEADS, 64).sum(-1)).abs().max()) < 1e-4
        # the precision's other output form: the rounding of the fp32 form, and inside the bound plus the format's own rounding
        o2, k2, v2, _ = _launch(prec, qkv, kc, vc, P, layout, form2)
        assert torch.equal(DR.bits(k2), DR.bits(k_ref)) and torch.equal(DR.bits(v2), DR.bits(v_ref))
        if form2 == "bf16":
            assert o2.dtype == torch.bfloat16 and torch.equal(DR.bits(o2), DR.bits(out.to(torch.bfloat16)))
            assert bool(((o2.double() - ref).abs() <= ref.abs() * 2.0 ** -8 + BOUND[prec] * rms).all())
        else:
            assert o2.dtype == torch.uint8 and torch.equal(o2, ops.pack_f16c_rows(out))
            h, _, r = ops.unpack_f16c_rows(o2, D)                # fp16 piece + fp8 residual: 2^-15 relative, 2^-21 absolute
            val = h.double() + r.double() / 2048.0
            assert bool(((val - ref).abs() <= ref.abs() * 2.0 ** -14 + 1e-6 + BOUND[prec] * max(1.0, float(ref.abs().max()))).all())
        if layout == "head_major":
            full = _full_causal(prec, qkv, kc, vc, B, P, Tn)
            if prec == "bf16":                                   # the rescale by exp2(rounding residue): see the module docstring
                d = (full.double() - out.double()).abs()
                print(f"attention_extend bf16 B={B} P={P} Tn={Tn}: full causal launch differs by at most {float(d.max()):.3e}")
                assert bool((d <= 2.0 ** -20 * (out.double().abs() + out.double().abs().max(1, keepdim=True).values)).all()), (P, Tn)
            else:
                assert torch.equal(DR.bits(full), DR.bits(out)), (prec, P, Tn, "rows of the full causal launch differ in bits")
    return worst


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("P,Tn", CASES)
def test_parity(P, Tn, prec):
    """Measured on an MI355X, worst over the cases and both layouts: fp32 rel_err 9.5e-6 at (100, 188) (bound 2e-5), bf16 4.4e-3
    at (100, 188) (bound 1.5e-2), f16c 1.6e-6 at (128, 128) (bound 3e-6); the bf16 kernel against the full causal launch: at most
    2.4e-7 absolute (1 ulp), fp32 and f16c bit for bit."""
    _check_case(prec, 1, P, Tn)


@pytest.mark.parametrize("prec", list(PRECS))
def test_parity_two_sequences(prec):
    """B = 2 at (65, 127): a batch-stride mix-up in the q rows, the caches or the output shows."""
    _check_case(prec, 2, 65, 127)


def test_refusals_return_an_error_and_launch_nothing():
    lib = _hip.load()
    qkv, kc, vc = ER.random_extend(1, HEADS, TMAX, 287, 2, torch.float32, seed=1)
    kd, vd, qd = kc.cuda(), vc.cuda(), qkv.cuda()

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(DR.bits(kd.cpu()), DR.bits(kc)) and torch.equal(DR.bits(vd.cpu()), DR.bits(vc))
    with pytest.raises(RuntimeError, match="outside the cache"):                                 # P + Tn > Tmax
        ops.attention_extend(qd, kd, vd, 287)
    assert untouched()
    with pytest.raises(RuntimeError, match="outside the cache"):                                 # P < 0
        ops.attention_extend(qd, kd, vd, -1)
    out = torch.zeros(2, D, device="cuda")
    args = (qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    assert lib.kx_attention_extend(*args, _hip.KX_F32, None, 1, HEADS, 0, 5, TMAX, _hip.KX_PREC_F32, None) == 1   # Tn = 0
    assert "outside the cache" in _hip.last_error()
    with pytest.raises(RuntimeError):                                                            # ... and through the wrapper
        ops.attention_extend(qd[:0], kd, vd, 5)
    with pytest.raises(TypeError, match="share one dtype"):                                      # dtype mismatch
        ops.attention_extend(qd.to(torch.bfloat16), kd, vd, 5)
    with pytest.raises(TypeError, match="share one dtype"):
        ops.attention_extend(qd, kd.to(torch.bfloat16), vd.to(torch.bfloat16), 5)
    # an output form the precision does not write: KX_F16C rows from the bf16 kernel, bf16 from the f16c kernel
    assert lib.kx_attention_extend(*args, _hip.KX_F16C, None, 1, HEADS, 2, 5, TMAX, _hip.KX_PREC_BF16, None) == 1
    assert lib.kx_attention_extend(*args, _hip.KX_BF16, None, 1, HEADS, 2, 5, TMAX, _hip.KX_PREC_F16C, None) == 1
    assert lib.kx_attention_extend(*args, _hip.KX_F32, None, 1, HEADS, 2, 5, TMAX, 99, None) == 1
    assert "precision" in _hip.last_error()
    with pytest.raises(ValueError, match="same number of new rows"):
        ops.attention_extend(torch.zeros(3, 3 * D, device="cuda"), torch.zeros(2, HEADS, TMAX, 64, device="cuda"),
                             torch.zeros(2, HEADS, TMAX, 64, device="cuda"), 0)
    assert untouched() and float(out.abs().max()) == 0.0
