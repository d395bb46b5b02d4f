"""kx_attention_decode_shared (csrc/kx_attention.hip): C candidates of K rows read the cache sequences cache_seq[c] of a shared
prompt cache and nobody appends.

The contract is bit equality with kx_attention_decode_block on a cache replicated per candidate (K = 1: with the ragged launch) —
outputs and statistics, in every output form and under both cache layouts — with the shared caches bitwise untouched.  The float64
agreement is checked directly as well, at the bound tests/test_attention_decode_gpu.py holds this arithmetic to.  Bases sit on both
sides of the first-round boundary (128 keys with the fp32 cache, 256 with bf16) and at 0 (every key comes from the qkv rows); cache
rows at and after the base are NaN, so a key read from the cache where the qkv row holds it shows (tests/test_score.py checks that
these inputs tell the wrong kernels from the right one)."""
import pytest
import torch

import decode_ref as DR
import score_ref as R
from kosmosx import _hip
from kosmosx import ops

pytestmark = pytest.mark.gpu

BOUND = 2e-5            # tests/test_attention_decode_gpu.py: the fp32-attention bound, both caches (measured there at 2e-6)
# measured here (MI355X): worst rel_err 2.7e-6 over the fp32 cache (K = 5), 1.7e-6 over the bf16 cache (K = 16)
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _layout(c, layout):
    return c.transpose(1, 2).contiguous() if layout == "row_major" else c


def _shared(qkv, kc, vc, pos, seq, K, form="f32", layout="head_major"):
    """-> (out, stats, kcache, vcache after the launch, error word), on the CPU."""
    kd, vd = _layout(kc, layout).cuda(), _layout(vc, layout).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.zeros(qkv.shape[0], R.HH, 2, device="cuda")
    out = ops.attention_decode_shared(qkv.cuda(), kd, vd, pos.cuda(), seq.cuda(), err, rows_per_candidate=K, out_dtype=form,
                                      stats_out=st, layout=layout)
    torch.cuda.synchronize()
    return out.cpu(), st.cpu(), kd.cpu(), vd.cpu(), int(err.item())


def _replicated(qkv, kc, vc, pos, seq, K, form="f32", layout="head_major"):
    """The block launch (K = 1: the ragged launch) on the caches gathered by cache_seq: one private sequence per candidate."""
    idx = seq.long()
    kd, vd = _layout(kc[idx], layout).cuda(), _layout(vc[idx], layout).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.zeros(qkv.shape[0], R.HH, 2, device="cuda")
    if K == 1:
        out = ops.attention_decode(qkv.cuda(), kd, vd, positions=pos.cuda(), error_word=err, out_dtype=form, stats_out=st, layout=layout)
    else:
        out = ops.attention_decode_block(qkv.cuda(), kd, vd, pos.cuda(), err, rows_per_sequence=K, out_dtype=form, stats_out=st,
                                         layout=layout)
    torch.cuda.synchronize()
    return out.cpu(), st.cpu(), int(err.item())


def _bits_equal(a, b):
    return torch.equal(DR.bits(a) if a.is_floating_point() else a, DR.bits(b) if b.is_floating_point() else b)


@pytest.mark.parametrize("K", R.ROWS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_shared_launch_is_the_block_launch_on_replicated_caches_and_leaves_the_caches_alone(dtype, K):
    worst = 0.0
    for i, t0 in enumerate(R.BASES):
        qkv, kc, vc, pos, seq = R.shared_inputs(t0, K, dtype, seed=1000 * K + i)
        out, st, k1, v1, word = _shared(qkv, kc, vc, pos, seq, K)
        want = _replicated(qkv, kc, vc, pos, seq, K)
        assert word == 0 and want[2] == 0
        assert _bits_equal(out, want[0]) and _bits_equal(st, want[1]), (t0, "not the block launch's bits")
        assert _bits_equal(k1, kc) and _bits_equal(v1, vc), (t0, "the shared caches changed")
        ref, _, _ = R.shared_attention_ref(qkv, kc, vc, t0, seq, K, nan_to_num=dtype == torch.float32)
        assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        for r in range(out.shape[0]):
            e = DR.rel_err64(out[r:r + 1], ref[r:r + 1])
            worst = max(worst, e)
            assert e < BOUND, (t0, r, e)
    print(f"decode shared attention, {dtype} cache, K = {K}: worst rel_err {worst:.3e} (bound {BOUND:.0e})")


@pytest.mark.parametrize("form,layout,dtype", [("f16c", "head_major", torch.float32), ("f16p", "head_major", torch.float32),
                                               ("bf16", "head_major", torch.bfloat16), ("f32", "row_major", torch.float32),
                                               ("f32", "row_major", torch.bfloat16)])
def test_output_forms_and_the_row_major_layout(form, layout, dtype):
    lib = _hip.load()
    K, t0 = 5, 127
    qkv, kc, vc, pos, seq = R.shared_inputs(t0, K, dtype, seed=77)
    lib.kx_set_tuning(9, 1 if layout == "row_major" else 0)
    try:
        out, st, k1, v1, word = _shared(qkv, kc, vc, pos, seq, K, form, layout)
        want = _replicated(qkv, kc, vc, pos, seq, K, form, layout)
    finally:
        lib.kx_set_tuning(9, 0)
    assert word == 0 and want[2] == 0
    assert _bits_equal(out, want[0]) and _bits_equal(st, want[1])
    assert _bits_equal(k1, _layout(kc, layout)) and _bits_equal(v1, _layout(vc, layout))
    assert bool(out.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["cache_seq", "off_base", "tmax"])
def test_a_rejected_row_writes_nothing_sets_the_bit_and_leaves_the_others_alone(case, dtype):
    """One cache_seq entry = Bc (all K rows of that candidate are rejected), one row with t != t0 + j, one row at t = Tmax."""
    K = 4
    t0 = R.TMAX - 3 if case == "tmax" else 10                      # tmax: every candidate's last row sits at Tmax
    qkv, kc, vc, pos, seq = R.shared_inputs(t0, K, dtype, seed=31)
    if case == "tmax":
        assert int(pos[K - 1]) == R.TMAX
        bad_rows = [K - 1, 2 * K - 1, 3 * K - 1]
        # the clean run: the same rows over caches one (poisoned) row longer, where position Tmax exists
        pad = torch.full((R.BC, R.HH, 1, 64), float("nan"), dtype=dtype)
        c = _shared(qkv, torch.cat([kc, pad], 2), torch.cat([vc, pad], 2), pos, seq, K)
        assert c[4] == 0
        clean = (c[0], c[1])
    else:
        c = _shared(qkv, kc, vc, pos, seq, K)
        assert c[4] == 0
        clean = (c[0], c[1])
        if case == "cache_seq":
            seq = seq.clone()
            seq[1] = R.BC
            bad_rows = [K, K + 1, K + 2, K + 3]
        else:
            pos = pos.clone()
            pos[2 * K + 2] = t0 + 3                                # 10, 11, 13, 13
            bad_rows = [2 * K + 2]
    kd, vd = kc.cuda(), vc.cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    # sentinel-filled outputs: the wrapper's zeroed buffer would hide a row that wrote zeros, so the library is driven directly
    D = R.HH * 64
    out = torch.full((3 * K, D), 12345.0, device="cuda")
    st = torch.full((3 * K, R.HH, 2), 12345.0, device="cuda")
    prec = _hip.KX_PREC_BF16 if dtype == torch.bfloat16 else _hip.KX_PREC_F32
    qd, pd, sd = qkv.cuda(), pos.cuda(), seq.cuda()
    _hip.check(_hip.load().kx_attention_decode_shared(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), _hip.KX_F32,
                                                      st.data_ptr(), 3, K, R.HH, pd.data_ptr(), sd.data_ptr(), R.BC, R.TMAX, prec,
                                                      err.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "kx_attention_decode_shared")
    torch.cuda.synchronize()
    out, st = out.cpu(), st.cpu()
    assert int(err.item()) == _hip.KX_RAGGED_ERR_CACHE
    for r in range(3 * K):
        if r in bad_rows:
            assert bool((out[r] == 12345.0).all()) and bool((st[r] == 12345.0).all()), r
        else:
            assert _bits_equal(out[r], clean[0][r]) and _bits_equal(st[r], clean[1][r]), r
    assert _bits_equal(kd.cpu(), kc) and _bits_equal(vd.cpu(), vc)


def test_the_wrapper_checks_its_shapes():
    qkv, kc, vc, pos, seq = R.shared_inputs(5, 2, torch.float32, seed=1)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        ops.attention_decode_shared(qkv.cuda(), kc.cuda(), vc.cuda(), pos[:2].cuda(), seq.cuda(), err, rows_per_candidate=2)
    with pytest.raises(TypeError):
        ops.attention_decode_shared(qkv.cuda(), kc.cuda(), vc.cuda(), pos.cuda(), seq.long().cuda(), err, rows_per_candidate=2)
