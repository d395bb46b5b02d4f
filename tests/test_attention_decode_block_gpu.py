"""kx_attention_decode_block (csrc/kx_attention.hip): K rows of one launch belong to one cache sequence at consecutive positions.

The contract is bit equality with K successive kx_attention_decode_ragged launches on the same sequence — outputs, statistics and
cache rows, in every output form and under both cache layouts — so the float64 agreement of the ragged kernel
(tests/test_attention_decode_gpu.py) carries over; it is checked here directly as well, at that file's bound.  Bases straddle the
first-round boundary (128 keys with the fp32 cache, 256 with bf16), sit at 0 (every key comes from the qkv block) and put the last
row at Tmax - 1; cache rows at and after a sequence's base are NaN before every launch."""
import pytest
import torch

import decode_ref as DR
from kosmosx import _hip
from kosmosx import ops

pytestmark = pytest.mark.gpu

BOUND = 2e-5                                                # tests/test_attention_decode_gpu.py: the fp32-attention bound, both caches
HH, TMAX = 2, 288
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
FORMS = {torch.float32: ("f32", "bf16", "f16c", "f16p"), torch.bfloat16: ("f32", "bf16")}   # what the ragged entry accepts


def _inputs(bases, K, dtype, seed, Tmax=TMAX, Hh=HH):
    """qkv [B * K, 3D], caches [B, H, Tmax, 64] with rows >= the sequence's base poisoned, positions [B * K] — on the CPU."""
    B, D = len(bases), Hh * 64
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * K, 3 * D, generator=g)
    qkv[:, :D] *= 0.35
    kc, vc = torch.randn(B, Hh, Tmax, 64, generator=g), torch.randn(B, Hh, Tmax, 64, generator=g)
    for b, t0 in enumerate(bases):
        kc[b, :, t0:], vc[b, :, t0:] = float("nan"), float("nan")
    pos = torch.tensor([t0 + j for t0 in bases for j in range(K)], dtype=torch.int32)
    return qkv.to(dtype), kc.to(dtype), vc.to(dtype), pos


def _layout(c, layout):
    return c.transpose(1, 2).contiguous() if layout == "row_major" else c


def _sequential(qkv, kc, vc, pos, K, form, layout):
    """K ragged launches: launch j steps row j of every sequence.  -> (out [B * K, ...], stats [B * K, H, 2], caches, error word)."""
    B = kc.shape[0]
    kd, vd = _layout(kc, layout).cuda(), _layout(vc, layout).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    q3, p2 = qkv.view(B, K, -1), pos.view(B, K)
    outs, stats = [], []
    for j in range(K):
        st = torch.zeros(B, HH, 2, device="cuda")
        outs.append(ops.attention_decode(q3[:, j].contiguous().cuda(), kd, vd, positions=p2[:, j].contiguous().cuda(), error_word=err,
                                         out_dtype=form, stats_out=st, layout=layout))
        stats.append(st)
    out = torch.stack(outs, 1).reshape(B * K, -1)
    return out.cpu(), torch.stack(stats, 1).reshape(B * K, HH, 2).cpu(), kd.cpu(), vd.cpu(), int(err.item())


def _block(qkv, kc, vc, pos, K, form, layout):
    kd, vd = _layout(kc, layout).cuda(), _layout(vc, layout).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.zeros(qkv.shape[0], HH, 2, device="cuda")
    out = ops.attention_decode_block(qkv.cuda(), kd, vd, pos.cuda(), err, rows_per_sequence=K, out_dtype=form, stats_out=st,
                                     layout=layout)
    torch.cuda.synchronize()
    return out.cpu(), st.cpu(), kd.cpu(), vd.cpu(), int(err.item())


def _same(a, b):
    return all(torch.equal(DR.bits(x) if x.is_floating_point() else x, DR.bits(y) if y.is_floating_point() else y)
               for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _bases(dtype, K):
    rb = 128 if dtype == torch.float32 else 256              # keys of the first round
    return [[0], [rb - 2], [rb - 1], [TMAX - K], [rb - 1, 5], [0, TMAX - K], [rb - 2, rb - 1]]


@pytest.mark.parametrize("K", [2, 4, 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_block_launch_is_k_ragged_launches_bit_for_bit(dtype, K):
    lib = _hip.load()
    n = 0
    for i, bases in enumerate(_bases(dtype, K)):
        qkv, kc, vc, pos = _inputs(bases, K, dtype, seed=100 * K + i)
        for layout in ("head_major", "row_major"):
            lib.kx_set_tuning(9, 1 if layout == "row_major" else 0)
            try:
                for form in FORMS[dtype]:
                    want = _sequential(qkv, kc, vc, pos, K, form, layout)
                    got = _block(qkv, kc, vc, pos, K, form, layout)
                    assert want[4] == 0 and _same(got, want), (bases, layout, form)
                    n += 1
            finally:
                lib.kx_set_tuning(9, 0)
        # the cache after the launch: rows base .. base + K - 1 are the block's k | v, everything else is what it was
        k1, v1 = got[2], got[3]                                # (row-major, the last layout run)
        D = HH * 64
        for b, t0 in enumerate(bases):
            rows = qkv.view(len(bases), K, 3, D)[b]
            assert torch.equal(DR.bits(k1[b, t0:t0 + K].reshape(K, D)), DR.bits(rows[:, 1]))
            assert torch.equal(DR.bits(v1[b, t0:t0 + K].reshape(K, D)), DR.bits(rows[:, 2]))
            assert torch.equal(DR.bits(k1[b, :t0]), DR.bits(_layout(kc, "row_major")[b, :t0]))
            assert bool(torch.isnan(k1[b, t0 + K:].float()).all()) and bool(torch.isnan(v1[b, t0 + K:].float()).all())
    print(f"decode block attention, {dtype} cache, K = {K}: {n} launches bit-equal to K ragged launches")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_rows_against_the_float64_reference(dtype):
    """Row (b, j) = the single-query attention at t = base + j over the cache with rows base .. base + j - 1 appended from the
    block's own qkv rows, in float64."""
    worst = 0.0
    for K, bases in ((16, [0, 120]), (4, [254, 126]), (2, [TMAX - 2, 255])):
        qkv, kc, vc, pos = _inputs(bases, K, dtype, seed=7 + K)
        out, _, _, _, word = _block(qkv, kc, vc, pos, K, "f32", "head_major")
        assert word == 0 and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        for b, t0 in enumerate(bases):
            kb, vb = kc[b:b + 1].clone(), vc[b:b + 1].clone()
            for j in range(K):
                r = b * K + j
                ref, kb, vb = DR.decode_attention_ref(qkv[r:r + 1], kb, vb, t0 + j, nan_to_num=dtype == torch.float32)
                e = DR.rel_err64(out[r:r + 1], ref)
                worst = max(worst, e)
                assert e < BOUND, (K, b, j, e)
    print(f"decode block attention, {dtype} cache: worst rel_err {worst:.3e} (bound {BOUND:.0e})")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_row_outside_the_cache_or_off_its_base_writes_nothing_and_sets_the_bit(dtype):
    """The validated-error path: sequence 0's last row would sit at Tmax; sequence 1's row 2 is not at base + 2.  Those rows'
    outputs and cache rows stay as they were, the error word gets KX_RAGGED_ERR_CACHE, every other row is the ragged launches'."""
    K, Tmax = 4, 64
    bases = [Tmax - 3, 10]
    qkv, kc, vc, pos = _inputs(bases, K, dtype, seed=31, Tmax=Tmax)
    assert int(pos[3]) == Tmax
    pos[K + 2] = 13                                            # 10, 11, 13, 13
    got = _block(qkv, kc, vc, pos, K, "f32", "head_major")
    out, st, k1, v1, word = got
    assert word == _hip.KX_RAGGED_ERR_CACHE
    for r in (3, K + 2):
        assert not bool(out[r].any()) and not bool(st[r].any())                         # (the wrapper hands zeroed buffers in)
    D = HH * 64
    good = qkv.view(2, K, 3, D)
    assert torch.equal(DR.bits(k1[0, :, Tmax - 3:]).transpose(0, 1).reshape(3, D), DR.bits(good[0, :3, 1]))
    assert torch.equal(DR.bits(k1[0, :, :Tmax - 3]), DR.bits(kc[0, :, :Tmax - 3]))
    assert bool(torch.isnan(k1[1, :, 12].float()).all()) and bool(torch.isnan(v1[1, :, 12].float()).all())   # row 2 appended nothing
    assert torch.equal(DR.bits(k1[1, :, 13]).reshape(D), DR.bits(good[1, 3, 1]))
    # the rows before the rejected ones: the K ragged launches' bits (the ragged kernel rejects the row at Tmax the same way)
    pos_ok = pos.clone()
    pos_ok[K + 2] = 12
    want = _sequential(qkv, kc, vc, pos_ok, K, "f32", "head_major")
    assert want[4] == _hip.KX_RAGGED_ERR_CACHE
    for r in (0, 1, 2, K, K + 1):
        assert torch.equal(DR.bits(out[r]), DR.bits(want[0][r])) and torch.equal(DR.bits(st[r]), DR.bits(want[1][r])), r
    assert bool(torch.isfinite(out[K + 3]).all())              # row 3 of sequence 1 is at base + 3: it ran (key 12 from qkv row 2)
    with pytest.raises(TypeError):
        ops.attention_decode_block(qkv.cuda(), kc.cuda(), vc.cuda(), pos[:K].cuda(), torch.zeros(1, dtype=torch.int32, device="cuda"),
                                   rows_per_sequence=K)
