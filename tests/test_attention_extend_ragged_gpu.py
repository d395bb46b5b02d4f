"""kx_attention_extend_ragged (csrc/kx_attention.hip: the KX_EXT_RAGGED instantiations of the three causal flash kernels + the
cache append at a per-sequence row offset read on the device) against the float64 reference of tests/extend_ragged_ref.py and,
bit for bit, against B = 1 kx_attention_extend launches.

H = 2, B = 3, Tmax = 288, cache rows at and after P_b NaN before every launch, both cache layouts, three precisions.  The cases
put P_b and P_b + Tn on, before and after the 64-key tile and 128-query block edges and make the sequences of one launch walk
different tile counts; Tn >= 129 runs the query-block pairing.

Bounds against float64: BOUND of tests/test_attention_extend_gpu.py (the same kernels' bounds; not re-derived here).
Bit equality: sequence b of the launch has the same P, Tn and grid coordinates (x, y) as the B = 1 uniform launch at P = P_b, and
P / Tk enter the same code as workgroup-uniform values — outputs, statistics and cache rows are equal in all three precisions."""
import pytest
import torch

import decode_ref as DR
import extend_ragged_ref as RR
import extend_ref as ER
from kosmosx import _hip
from kosmosx import ops

pytestmark = pytest.mark.gpu

HEADS, TMAX, B = 2, 288, 3
D = HEADS * 64
CASES = [((0, 63, 200), 1), ((1, 64, 65), 2), ((5, 127, 128), 33), ((63, 64, 200), 64), ((0, 127, 158), 130), ((100, 0, 17), 188)]
# precision -> (torch dtype of qkv and caches, q scale, k scale, nan_to_num in the reference): as tests/test_attention_extend_gpu.py
PRECS = {"fp32": (torch.float32, 0.35, 1.0, True), "bf16": (torch.bfloat16, 0.35, 1.0, False), "f16c": (torch.float32, 0.6, 1.5, True)}
BOUND = {"fp32": 2e-5, "bf16": 1.5e-2, "f16c": 3e-6}
SENTINEL = 12345.0


def test_the_bounds_are_those_of_the_uniform_extend_test():
    import test_attention_extend_gpu as U
    assert BOUND == U.BOUND and {k: v[:4] for k, v in U.PRECS.items()} == PRECS and (HEADS, TMAX) == (U.HEADS, U.TMAX)


def _row_major(c):
    return c.permute(0, 2, 1, 3).contiguous()                      # [B, H, Tmax, 64] -> [B, Tmax, H, 64]


def _err(prec, out, ref):
    if prec == "f16c":
        return float((out.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    return DR.rel_err64(out, ref)


def _launch(prec, qkv, kc, vc, positions, layout):
    """The ragged launch (positions a list) or the uniform one (an int) on device copies, output rows and statistics pre-filled with
    SENTINEL -> (out, kcache after, vcache after, stats, error word) on the CPU, the caches back in [B, H, Tmax, 64]."""
    rm = layout == "row_major"
    kd, vd = (_row_major(kc) if rm else kc).cuda(), (_row_major(vc) if rm else vc).cuda()
    st = torch.full((qkv.shape[0], HEADS, 2), SENTINEL, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = _hip.load()
    try:
        if rm:
            lib.kx_set_tuning(9, 1)
        if isinstance(positions, int):
            out = ops.attention_extend(qkv.cuda(), kd, vd, positions, stats_out=st, layout=layout, f16c=prec == "f16c")
        else:
            out = torch.full((qkv.shape[0], D), SENTINEL, device="cuda")
            ops.attention_extend_ragged(qkv.cuda(), kd, vd, torch.tensor(positions, dtype=torch.int32, device="cuda"), err,
                                        stats_out=st, layout=layout, f16c=prec == "f16c", out=out)
        torch.cuda.synchronize()
    finally:
        if rm:
            lib.kx_set_tuning(9, 0)
    k1, v1 = kd.cpu(), vd.cpu()
    return out.cpu(), (_row_major(k1) if rm else k1), (_row_major(v1) if rm else v1), st.cpu(), int(err.item())


def _check_case(prec, positions, Tn, seed):
    dtype, qs, ks, n2n = PRECS[prec]
    qkv, kc, vc = RR.random_extend_ragged(HEADS, TMAX, positions, Tn, dtype, seed, qs, ks)
    ref, k_ref, v_ref = RR.extend_ragged_attention_ref(qkv, kc, vc, positions, n2n)
    bad = [RR.guarded(P, Tn, TMAX) for P in positions]
    for layout in ("head_major", "row_major"):
        out, k1, v1, st, word = _launch(prec, qkv, kc, vc, list(positions), layout)
        assert word == (_hip.KX_RAGGED_ERR_CACHE if any(bad) else 0), (positions, Tn, word)
        # (c) rows [P_b, P_b + Tn) = the qkv rows' k | v, every other row untouched (the reference's caches, NaN rows included)
        assert torch.equal(DR.bits(k1), DR.bits(k_ref)) and torch.equal(DR.bits(v1), DR.bits(v_ref)), (prec, positions, Tn, layout)
        kn, vn = ER.new_rows(qkv, B, HEADS)[1:]
        for b, P in enumerate(positions):
            rows = slice(b * Tn, (b + 1) * Tn)
            if bad[b]:                                               # (d) nothing of a guarded sequence is written
                assert bool((out[rows] == SENTINEL).all()) and bool((st[rows] == SENTINEL).all())
                assert torch.equal(DR.bits(k1[b]), DR.bits(kc[b])) and torch.equal(DR.bits(v1[b]), DR.bits(vc[b]))
                continue
            assert torch.equal(DR.bits(k1[b, :, P:P + Tn]), DR.bits(kn[b])) and torch.equal(DR.bits(v1[b, :, P:P + Tn]), DR.bits(vn[b]))
            assert bool(torch.isfinite(out[rows]).all())
            e = _err(prec, out[rows], ref[rows])                     # (a)
            print(f"attention_extend_ragged {prec} P={positions} Tn={Tn} {layout} sequence {b}: error {e:.3e} (bound {BOUND[prec]:.1e})")
            assert e < BOUND[prec], (prec, positions, Tn, layout, b, e)
            # (b) the B = 1 uniform launch at P = P_b, bit for bit: outputs, statistics, cache rows
            o1, ku, vu, su, _ = _launch(prec, *RR.sequence(qkv, kc, vc, b, Tn), int(P), layout)
            assert torch.equal(DR.bits(out[rows]), DR.bits(o1)), (prec, positions, Tn, layout, b, "outputs differ in bits")
            assert torch.equal(DR.bits(st[rows]), DR.bits(su)), (prec, positions, Tn, layout, b, "statistics differ in bits")
            assert torch.equal(DR.bits(k1[b:b + 1]), DR.bits(ku)) and torch.equal(DR.bits(v1[b:b + 1]), DR.bits(vu))


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("positions,Tn", CASES)
def test_parity_and_bit_equality(positions, Tn, prec):
    _check_case(prec, positions, Tn, seed=20000 + 300 * positions[1] + Tn)


@pytest.mark.parametrize("prec", list(PRECS))
@pytest.mark.parametrize("positions,Tn", [((5, -1, 128), 33), ((63, 64, TMAX + 1 - 64), 64), ((TMAX + 1 - 130, 127, 158), 130)])
def test_a_sequence_outside_the_cache_writes_nothing_and_sets_the_error_word(positions, Tn, prec):
    """One sequence has P_b = -1 or P_b + Tn = Tmax + 1: a guarded error return.  Its outputs, statistics and caches keep what they
    held, the word carries KX_RAGGED_ERR_CACHE, the other two sequences still match their B = 1 launches bit for bit."""
    _check_case(prec, positions, Tn, seed=30000 + Tn)


def test_refusals_return_an_error_and_launch_nothing():
    lib = _hip.load()
    Tn = 2
    qkv, kc, vc = RR.random_extend_ragged(HEADS, TMAX, (5, 6, 7), Tn, torch.float32, seed=1)
    kd, vd, qd = kc.cuda(), vc.cuda(), qkv.cuda()
    pos = torch.tensor([5, 6, 7], dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(B * Tn, D, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return (torch.equal(DR.bits(kd.cpu()), DR.bits(kc)) and torch.equal(DR.bits(vd.cpu()), DR.bits(vc)) and
                float(out.abs().max()) == 0.0 and int(err.item()) == 0)
    args = (qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    f32, p32 = _hip.KX_F32, _hip.KX_PREC_F32
    call = lib.kx_attention_extend_ragged
    assert call(*args, f32, None, B, HEADS, Tn, None, TMAX, p32, err.data_ptr(), None) == 1                 # null positions
    assert "null positions" in _hip.last_error()
    assert call(*args, f32, None, B, HEADS, Tn, pos.data_ptr(), TMAX, p32, None, None) == 1                 # null error word
    assert call(None, *args[1:], f32, None, B, HEADS, Tn, pos.data_ptr(), TMAX, p32, err.data_ptr(), None) == 1
    assert "null pointer" in _hip.last_error()
    assert call(*args, f32, None, B, HEADS, 0, pos.data_ptr(), TMAX, p32, err.data_ptr(), None) == 1        # Tn = 0
    assert "outside the cache" in _hip.last_error()
    assert call(*args, f32, None, B, HEADS, TMAX + 1, pos.data_ptr(), TMAX, p32, err.data_ptr(), None) == 1  # Tn > Tmax
    assert call(*args, f32, None, B, HEADS, Tn, pos.data_ptr(), TMAX, 99, err.data_ptr(), None) == 1
    assert "precision" in _hip.last_error()
    # an output form the precision does not write: KX_F16C rows from the bf16 kernel, bf16 from the f16c kernel
    assert call(*args, _hip.KX_F16C, None, B, HEADS, Tn, pos.data_ptr(), TMAX, _hip.KX_PREC_BF16, err.data_ptr(), None) == 1
    assert call(*args, _hip.KX_BF16, None, B, HEADS, Tn, pos.data_ptr(), TMAX, _hip.KX_PREC_F16C, err.data_ptr(), None) == 1
    assert call(args[0] + 4, *args[1:], f32, None, B, HEADS, Tn, pos.data_ptr(), TMAX, p32, err.data_ptr(), None) == 1
    assert "aligned" in _hip.last_error()
    lib.kx_set_tuning(2, 1)                                          # the first-version fp32 kernel has no cache form
    try:
        assert call(*args, f32, None, B, HEADS, Tn, pos.data_ptr(), TMAX, p32, err.data_ptr(), None) == 1
    finally:
        lib.kx_set_tuning(2, 0)
    with pytest.raises(TypeError, match="positions"):                                            # ... and through the wrapper
        ops.attention_extend_ragged(qd, kd, vd, pos.to(torch.int64), err)
    with pytest.raises(TypeError, match="positions"):
        ops.attention_extend_ragged(qd, kd, vd, pos[:2].contiguous(), err)
    with pytest.raises(TypeError, match="error_word"):
        ops.attention_extend_ragged(qd, kd, vd, pos, None)
    with pytest.raises(TypeError, match="share one dtype"):
        ops.attention_extend_ragged(qd.to(torch.bfloat16), kd, vd, pos, err)
    with pytest.raises(ValueError, match="same number of new rows"):
        ops.attention_extend_ragged(qd[:5], kd, vd, pos, err)
    assert untouched()
