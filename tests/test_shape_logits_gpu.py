"""kx_shape_logits on the GPU against tests/shape_ref.py, bit for bit: uint32 compare of the rows, of the guard columns between them
(ld > V) and integer compare of the counts.  Shapes: V = 1, 37, one below / at / one above the kernel's slice width, and 64007; one
and three rows."""
import numpy as np
import pytest
import torch

import shape_ref as SR
from kosmosx import ops

pytestmark = pytest.mark.gpu

S = ops.SHAPE_SLICE
VS = [1, 37, S - 1, S, S + 1, 64007]
GUARD = 5                                                   # columns between the rows: ld = V + GUARD
INF = float("inf")


def _rows(B, V, seed, special=True):
    """fp32 [B, V + GUARD] with -inf and NaN logits sprinkled in; the guard columns hold a pattern nobody may touch."""
    rng = np.random.default_rng(seed)
    full = (rng.standard_normal((B, V + GUARD)) * 4).astype(np.float32)
    if special and V > 8:
        for b in range(B):
            full[b, rng.choice(V, 3, replace=False)] = -np.inf
            full[b, rng.choice(V, 2, replace=False)] = np.nan
    full[:, V:] = np.float32(12345.5)
    return full


def _edge_ids(V):
    """0, V - 1 and both sides of every slice edge inside the row."""
    ids = {0, V - 1}
    for e in range(S, V, S):
        ids |= {e - 1, e}
    return sorted(ids)


def _bias(B, V, seed):
    """Per row: the edge ids plus a few random ones, finite values of both signs and one -inf; row 1 (if any) has no entries."""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        if b == 1:
            rows.append([])
            continue
        ids = sorted(set(_edge_ids(V)) | set(int(i) for i in rng.choice(V, min(V, 6), replace=False)))
        vals = [float(np.float32(v)) for v in rng.standard_normal(len(ids)) * 3]
        if len(ids) > 1:
            vals[int(rng.integers(len(ids)))] = -INF
        rows.append(list(zip(ids, vals)))
    return rows


def _run(full, V, *, bias=None, counts=None, f=0.0, p=0.0, last=None, finished=None, table=None):
    """One launch on a device copy of ``full`` (a [B, V] view with ld = V + GUARD).  Returns (the whole buffer, the counts) as numpy."""
    dev = torch.device("cuda")
    buf = torch.from_numpy(full.copy()).to(dev)
    cnt = None if counts is None else torch.from_numpy(counts.copy()).to(dev)
    ops.shape_logits(buf[:, :V], bias=table if table is not None else (None if bias is None else ops.BiasTable(bias, dev)), counts=cnt,
                     frequency_penalty=f, presence_penalty=p,
                     last_token=None if last is None else torch.tensor(last, dtype=torch.int64, device=dev),
                     finished=None if finished is None else torch.tensor(finished, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), (None if cnt is None else cnt.cpu().numpy())


def _same_bits(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad[0].size == 0, (bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])


def _check(full, V, *, bias=None, counts=None, f=0.0, p=0.0, last=None, finished=None):
    got, gc = _run(full, V, bias=bias, counts=counts, f=f, p=p, last=last, finished=finished)
    want = full.copy()
    want[:, :V], wc = SR.shape_rows(full[:, :V], counts, bias=bias, frequency=f, presence=p, last_token=last, finished=finished)
    _same_bits(got, want)                                                   # the rows AND the guard columns
    if counts is not None:
        assert gc.dtype == np.int32 and np.array_equal(gc, wc)
    return got, gc


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_bias_counts_and_penalties_together(B, V):
    rng = np.random.default_rng(V * 7 + B)
    full = _rows(B, V, seed=V + B)
    counts = rng.integers(0, 4, (B, V)).astype(np.int32) * (rng.random((B, V)) < 0.3)
    last = [[0, V - 1, V // 2][b % 3] for b in range(B)]
    got, gc = _check(full, V, bias=_bias(B, V, seed=V), counts=counts, f=0.37, p=0.81, last=last)
    for b in range(B):
        assert gc[b, last[b]] == counts[b, last[b]] + 1
    if V > 8:                                                               # -inf and NaN logits kept their bits, biased and penalised or not
        keep = ~(full[:, :V] > -np.inf)
        assert keep.sum() >= 3 * B and np.array_equal(got[:, :V].view(np.uint32)[keep], full[:, :V].view(np.uint32)[keep])


@pytest.mark.parametrize("V", VS)
def test_negative_penalties_and_the_last_token_at_both_ends(V):
    B = 3
    rng = np.random.default_rng(V)
    full = _rows(B, V, seed=2 * V + 1)
    counts = rng.integers(0, 3, (B, V)).astype(np.int32)
    _check(full, V, counts=counts, f=-0.6, p=-1.25, last=[0, V - 1, V - 1])
    _check(full, V, counts=counts, f=0.0, p=2.0, last=[V - 1, 0, 0])         # presence alone
    _check(full, V, counts=counts, f=1.5, p=0.0, last=None)                  # step 0: nothing to count


@pytest.mark.parametrize("V", [37, S + 1])
def test_a_last_token_out_of_range_is_ignored(V):
    B = 3
    full = _rows(B, V, seed=9)
    counts = np.zeros((B, V), dtype=np.int32)
    counts[:, V // 3] = 2
    got, gc = _check(full, V, counts=counts, f=0.5, p=0.5, last=[-1, V, (1 << 40) + 3])
    assert np.array_equal(gc, counts)                                       # nothing counted, nothing written outside the rows (the guards compared above)


@pytest.mark.parametrize("V", [37, S + 1, 64007])
def test_a_finished_row_keeps_logits_and_counts(V):
    B = 3
    rng = np.random.default_rng(5)
    full = _rows(B, V, seed=11)
    counts = rng.integers(0, 3, (B, V)).astype(np.int32)
    bias = [[(0, 2.0), (V - 1, -INF)]] * B
    got, gc = _check(full, V, bias=bias, counts=counts, f=0.7, p=0.2, last=[3, 4, 5], finished=[0, 1, 0])
    _same_bits(got[1], full[1])
    assert np.array_equal(gc[1], counts[1]) and gc[0, 3] == counts[0, 3] + 1 and gc[2, 5] == counts[2, 5] + 1


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_a_bias_without_counts_and_counts_without_a_bias(B, V):
    full = _rows(B, V, seed=3 * V + B)
    got, _ = _check(full, V, bias=_bias(B, V, seed=V + 1))
    if V > 1:
        ban = [(b, i) for b, r in enumerate(_bias(B, V, seed=V + 1)) for i, v in r if v == -INF]
        assert ban and all(got[b, i] == -np.inf or np.isnan(full[b, i]) for b, i in ban)   # a -inf bias bans (a NaN stays a NaN)
    counts = np.random.default_rng(V).integers(0, 2, (B, V)).astype(np.int32)
    _check(full, V, counts=counts, f=0.25, p=0.5, last=[V - 1] * B)


def test_a_bias_never_revives_a_banned_id():
    V = 37
    full = _rows(1, V, seed=1, special=False)
    full[0, 4], full[0, 9] = -np.inf, np.nan
    got, _ = _check(full, V, bias=[[(4, 1e30), (9, 5.0), (10, 1.0)]])
    assert got[0, 4] == -np.inf and np.isnan(got[0, 9]) and got[0, 10] == np.float32(full[0, 10] + np.float32(1.0))


@pytest.mark.parametrize("V", [37, 2 * S + 5])
def test_a_malformed_table_changes_what_is_shaped_never_what_is_addressed(V):
    """Offsets out of range or out of order, ids outside the vocabulary: rows without a usable entry list stay as they are, ids
    outside [0, V) are skipped, the guard columns and the neighbouring rows are never written."""
    B = 3
    full = _rows(B, V, seed=13)
    dev = torch.device("cuda")
    ids = [-5, 2, V - 1, V, V + 3, 1 << 30]                                 # ascending; three of them outside the row
    val = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    for off, rows in (([0, 6, 6, 6], [[(2, 2.0), (V - 1, 3.0)], [], []]),           # row 0 sees every entry: the outside ones are skipped
                      ([-7, 3, 99, 2], [[(2, 2.0), (V - 1, 3.0)], [], []]),         # clamped to [0, 3) and [3, 6) (all outside), then out of order
                      ([0, 1, 4, 6], [[], [(2, 2.0), (V - 1, 3.0)], []]),           # well formed offsets over the same ids
                      ([6, 0, 0, 0], [[], [], []])):                                # out of order everywhere: no entries
        table = ops.BiasTable.raw(off, ids, val, dev)
        got, _ = _run(full, V, table=table)
        want = full.copy()
        want[:, :V], _ = SR.shape_rows(full[:, :V], None, bias=rows)
        _same_bits(got, want)


def test_five_consecutive_launches_count_like_bincount():
    B, V = 3, S + 1
    dev = torch.device("cuda")
    seq = np.array([[5, 5, S, 0, 5], [V - 1, 0, V - 1, 7, 7], [S - 1, S, S - 1, S, S - 1]])    # the tokens steps 0..4 emit
    bias = _bias(B, V, seed=2)
    table = ops.BiasTable(bias, dev)
    counts = torch.zeros((B, V), dtype=torch.int32, device=dev)
    ref_c = np.zeros((B, V), dtype=np.int32)
    f, p = 0.3, 0.9
    for g in range(6):                                                      # launch g counts token g - 1: five counting launches after step 0
        full = _rows(B, V, seed=100 + g)
        buf = torch.from_numpy(full.copy()).to(dev)
        last = None if g == 0 else torch.tensor(seq[:, g - 1], dtype=torch.int64, device=dev)
        ops.shape_logits(buf[:, :V], bias=table, counts=counts, frequency_penalty=f, presence_penalty=p, last_token=last)
        want = full.copy()
        want[:, :V], ref_c = SR.shape_rows(full[:, :V], ref_c, bias=bias, frequency=f, presence=p,
                                           last_token=None if g == 0 else seq[:, g - 1])
        _same_bits(buf.cpu().numpy(), want)
    got = counts.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], np.bincount(seq[b], minlength=V))


def test_the_wrapper_refuses_bad_tensors():
    dev = torch.device("cuda")
    row = torch.zeros((2, 10), device=dev)
    with pytest.raises(ValueError, match="counts"):
        ops.shape_logits(row, counts=torch.zeros((2, 9), dtype=torch.int32, device=dev), frequency_penalty=1.0)
    with pytest.raises(TypeError, match="counts"):
        ops.shape_logits(row, counts=torch.zeros((2, 10), dtype=torch.int64, device=dev), frequency_penalty=1.0)
    with pytest.raises(ValueError, match="bias"):
        ops.shape_logits(row, bias=ops.BiasTable([[(1, 1.0)]], dev))
    with pytest.raises(RuntimeError, match="counts"):
        ops.shape_logits(row, bias=ops.BiasTable([[(1, 1.0)], []], dev), frequency_penalty=1.0)
    with pytest.raises(RuntimeError, match="nothing to shape"):
        ops.shape_logits(row)
