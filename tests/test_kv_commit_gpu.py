"""kx_kv_cache_commit on the device against a torch indexing restatement: both cache dtypes, both cache layouts (tuning key 9),
ragged P_b including 0 and Tmax - 1, a finished row, and a chosen index the kernel refuses."""
import pytest
import torch

from kosmosx import _hip as H
from kosmosx import ops

pytestmark = pytest.mark.gpu
L, B, K, NH, TMAX, TTAIL = 2, 3, 4, 3, 10, 2


def _buffers(dtype, layout, seed):
    g = torch.Generator().manual_seed(seed)
    cs, ts = ((L, B, NH, TMAX, 64), (L, B * K, NH, TTAIL, 64)) if layout == "head_major" else ((L, B, TMAX, NH, 64), (L, B * K, TTAIL, NH, 64))
    kc, vc = (torch.randn(cs, generator=g).to(dtype).cuda() for _ in range(2))
    kt, vt = (torch.randn(ts, generator=g).to(dtype).cuda() for _ in range(2))
    return kc, vc, kt, vt


def _expect(cache, tail, layout, b, j, p):
    """The cache after tail row 0 of row b * K + j went to row p of sequence b (a clone; every other element as it was)."""
    want = cache.clone()
    if layout == "head_major":
        want[:, b, :, p] = tail[:, b * K + j, :, 0]
    else:
        want[:, b, p] = tail[:, b * K + j, 0]
    return want


def _run(dtype, layout, chosen, P, finished=None):
    kc, vc, kt, vt = _buffers(dtype, layout, len(chosen) + sum(P))
    k0, v0 = kc.clone(), vc.clone()
    ch = torch.tensor(chosen, dtype=torch.int32, device="cuda")
    pos = torch.tensor(P, dtype=torch.int32, device="cuda").repeat_interleave(K).contiguous()
    fin = None if finished is None else torch.tensor(finished, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = H.load()
    if layout == "row_major":
        lib.kx_set_tuning(9, 1)
    try:
        ops.kv_cache_commit(kt, vt, kc, vc, ch, pos, err, finished=fin, layout=layout)
        torch.cuda.synchronize()
    finally:
        lib.kx_set_tuning(9, 0)
    return k0, v0, kc, vc, kt, vt, pos.view(B, K).cpu(), int(err.item())


@pytest.mark.parametrize("layout", ["head_major", "row_major"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_commit_writes_the_chosen_tail_row_and_nothing_else(dtype, layout):
    chosen, P = [2, 0, 3], [0, TMAX - 1, 4]
    k0, v0, kc, vc, kt, vt, pos, err = _run(dtype, layout, chosen, P)
    wk, wv = k0, v0
    for b in range(B):
        wk, wv = _expect(wk, kt, layout, b, chosen[b], P[b]), _expect(wv, vt, layout, b, chosen[b], P[b])
    assert torch.equal(kc.view(torch.uint8), wk.view(torch.uint8)) and torch.equal(vc.view(torch.uint8), wv.view(torch.uint8))
    assert pos.tolist() == [[p + 1] * K for p in P] and err == 0


@pytest.mark.parametrize("layout", ["head_major", "row_major"])
def test_a_finished_row_is_skipped(layout):
    chosen, P = [1, 3, 0], [5, 2, 7]
    k0, v0, kc, vc, kt, vt, pos, err = _run(torch.float32, layout, chosen, P, finished=[0, 1, 0])
    wk, wv = k0, v0
    for b in (0, 2):
        wk, wv = _expect(wk, kt, layout, b, chosen[b], P[b]), _expect(wv, vt, layout, b, chosen[b], P[b])
    assert torch.equal(kc, wk) and torch.equal(vc, wv)
    assert pos.tolist() == [[6] * K, [2] * K, [8] * K] and err == 0


def test_a_bad_chosen_index_or_position_raises_the_error_bit_and_writes_nothing():
    """Values the kernel itself checks before it reads or writes through them."""
    chosen, P = [K, -1, 1], [3, 3, TMAX]
    k0, v0, kc, vc, _, _, pos, err = _run(torch.float32, "head_major", chosen, P)
    assert torch.equal(kc, k0) and torch.equal(vc, v0)
    assert pos.tolist() == [[p] * K for p in P] and err == H.KX_RAGGED_ERR_COMMIT


def test_wrapper_argument_checks():
    kc, vc, kt, vt = _buffers(torch.float32, "head_major", 0)
    ch, pos, err = (torch.zeros(n, dtype=torch.int32, device="cuda") for n in (B, B * K, 1))
    with pytest.raises(TypeError, match="chosen"):
        ops.kv_cache_commit(kt, vt, kc, vc, ch.long(), pos, err)
    with pytest.raises(TypeError, match="positions"):
        ops.kv_cache_commit(kt, vt, kc, vc, ch, pos[:B], err)
    with pytest.raises(TypeError, match="dtype"):
        ops.kv_cache_commit(kt.bfloat16(), vt, kc, vc, ch, pos, err)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.kv_cache_commit(kt, kt, kc, vc, ch, pos, err)
    with pytest.raises(RuntimeError, match="not on a CUDA"):
        ops.kv_cache_commit(kt.cpu(), vt, kc, vc, ch, pos, err)
