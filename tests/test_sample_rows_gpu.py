"""Per-row sampling options inside the sampler (kx_sample_logits_rows) against the scalar entry points, bit for bit.

The reference of row b is a ONE-ROW launch of ops.sample_logits without ``rows`` — kx_sample_logits, _min_p or _truncate, whichever the
row's values select — with the row's values, its ``sequence_ids[b]`` and its position; those entry points are themselves pinned to
the float64 references by tests/test_sample_logits_gpu.py and tests/test_sample_truncate_gpu.py.  ``next_token``, ``kept_count`` and
``keep_mask`` must be EQUAL: no tolerance."""
import functools

import numpy as np
import pytest
import torch

from kosmosx import _hip as H
from kosmosx import ops

pytestmark = pytest.mark.gpu

VS = [37, 1500, 64007]
B = 6
HIST = 5                                                      # ids of history in front of the slot the launch appends to
PAD = 1


def records(V):
    """Six mutually different requests."""
    return [dict(do_sample=False, temperature=0.7, top_k=3),                                     # 0: greedy (its filters are ignored)
            dict(do_sample=True, temperature=0.65),                                              # 1: temperature only
            dict(do_sample=True, temperature=1.0, top_k=min(12, V - 1), top_p=0.8, seed=3),       # 2: top-k + top-p
            dict(do_sample=True, temperature=1.1, min_p=0.05, typical_p=0.9, seed=3),             # 3: min-p + typical-p
            dict(do_sample=True, temperature=0.9, epsilon_cutoff=2e-3, eta_cutoff=0.02, repetition_penalty=1.3, seed=4),   # 4
            dict(do_sample=True, temperature=0.8, top_k=min(40, V - 1), top_p=0.95, min_p=0.02, typical_p=0.95, epsilon_cutoff=3e-4,
                 eta_cutoff=2e-3, repetition_penalty=0.8, seed=2 ** 63 + 12345)]                 # 5: everything, its own seed


@functools.lru_cache(maxsize=None)
def _logits(V):
    g = np.random.default_rng(V)
    x = (g.standard_normal((B, V)) * 2.5).astype(np.float32)
    x[g.random((B, V)) < 0.1] = -np.inf                       # banned ids in every row
    x[:, 0] = g.standard_normal(B).astype(np.float32)         # (never a row of -inf alone)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _history(V):
    """Ids the rows' repetition penalties see: the row's most likely ids among them, so that the penalty changes the draw."""
    x = _logits(V)
    h = np.stack([np.argsort(-x[b])[:HIST] for b in range(B)]).astype(np.int64)
    h.setflags(write=False)
    return h


def _hist(V, rows=slice(None)):
    h = _history(V)[rows]
    return torch.tensor(np.concatenate([h, np.zeros((len(h), 1), dtype=np.int64)], axis=1), device="cuda")


SEQ = [4, 9, 2, 7, 1, 30]


def _scalar_row(V, b, rec, *, position=None, positions=None, advance=0, history=True, seq=SEQ, **more):
    """Row b alone through the scalar entry point."""
    x = torch.tensor(_logits(V)[b:b + 1], device="cuda")
    kw = dict(rec, sequence_ids=torch.tensor([seq[b]], dtype=torch.int64, device="cuda"), return_debug=True, **more)
    if history:
        kw.update(history=_hist(V, slice(b, b + 1)), hist_len=HIST)
    if positions is not None:
        kw.update(positions=positions, advance=advance)
    else:
        kw.update(position=position)
    tok, kept, mask = ops.sample_logits(x, **kw)
    return int(tok[0]), int(kept[0]), mask[0].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(V, position):
    """The six one-row scalar launches at ``position``, computed once and shared."""
    return tuple(_scalar_row(V, b, rec, position=position) for b, rec in enumerate(records(V)))


def _table(V, recs=None, flags=None):
    """``flags``: a launch summary other than the pack's (a launch that does not carry the bitmap, or ignores the budgets)."""
    t = ops.SampleRowTable(records(V) if recs is None else recs, V, "cuda")
    if flags is not None:
        t.flags = flags
    return t


def _equal(got, want, what):
    tok, kept, mask = got
    for b, (t, k, m) in enumerate(want):
        assert int(tok[b]) == t and int(kept[b]) == k and np.array_equal(mask[b].cpu().numpy(), m), (what, b, int(tok[b]), t, int(kept[b]), k)


@pytest.mark.parametrize("V", VS)
def test_a_mixed_batch_gives_every_row_the_bits_of_its_own_scalar_launch(V):
    x = torch.tensor(_logits(V), device="cuda")
    seq = torch.tensor(SEQ, dtype=torch.int64, device="cuda")
    table = _table(V)
    assert table.flags == H.SAMPLE_ROWS_PENALTY and table.B == B
    for position in (3, 40):
        want = _reference(V, position)
        # the scalars of the call are ignored: values the rows do not use
        got = ops.sample_logits(x, rows=table, position=position, sequence_ids=seq, history=_hist(V), hist_len=HIST, return_debug=True,
                                temperature=5.0, top_k=2, top_p=0.1, repetition_penalty=3.0, seed=999, do_sample=False)
        _equal(got, want, ("uniform", position))
        # the ragged form: every row at its own device position, advance 0 and 1, the positions moved as the scalar launch moves them
        for advance in (0, 1):
            pos = torch.full((B,), position - advance, dtype=torch.int32, device="cuda")
            got = ops.sample_logits(x, rows=table, positions=pos, advance=advance, sequence_ids=seq, history=_hist(V), hist_len=HIST,
                                    return_debug=True)
            _equal(got, want, ("ragged", position, advance))
            assert torch.equal(pos, torch.full((B,), position, dtype=torch.int32, device="cuda"))
    base = torch.tensor([7, 3, 19, 3, 40, 11], dtype=torch.int32, device="cuda")                  # unlike positions
    pos = base.clone()
    got = ops.sample_logits(x, rows=table, positions=pos, advance=1, sequence_ids=seq, history=_hist(V), hist_len=HIST, return_debug=True)
    want = []
    for b, rec in enumerate(records(V)):
        p1 = base[b:b + 1].clone()
        want.append(_scalar_row(V, b, rec, positions=p1, advance=1))
        assert int(p1[0]) == int(pos[b]) == int(base[b]) + 1                                      # ``positions`` advanced identically
    _equal(got, want, "ragged, unlike positions")
    # the rows are unlike in effect too: rows 0 and 1 keep every candidate, row 2 at most its top-k (exact ties aside: none here)
    candidates = np.isfinite(_logits(V)).sum(axis=1)
    assert int(got[1][0]) == candidates[0] and int(got[1][1]) == candidates[1] and 1 <= int(got[1][2]) <= min(12, V - 1)


@pytest.mark.parametrize("V", [37, 1500])
def test_permuting_the_rows_permutes_the_outputs(V):
    perm = [3, 5, 0, 4, 2, 1]
    x = torch.tensor(_logits(V), device="cuda")
    recs = records(V)
    out = ops.sample_logits(x, rows=_table(V), position=9, sequence_ids=torch.tensor(SEQ, device="cuda"), history=_hist(V), hist_len=HIST,
                            return_debug=True)
    idx = torch.tensor(perm, device="cuda")
    got = ops.sample_logits(x[idx].contiguous(), rows=_table(V, [recs[i] for i in perm]), position=9,
                            sequence_ids=torch.tensor([SEQ[i] for i in perm], device="cuda"), history=_hist(V)[idx].contiguous(),
                            hist_len=HIST, return_debug=True)
    for a, b in zip(out, got):
        assert torch.equal(a[idx], b)
    # a row's outputs do not depend on B or on its row index: rows 2.. alone
    part = ops.sample_logits(x[2:].contiguous(), rows=_table(V, recs[2:]), position=9, sequence_ids=torch.tensor(SEQ[2:], device="cuda"),
                             history=_hist(V)[2:].contiguous(), hist_len=HIST, return_debug=True)
    for a, b in zip(out, part):
        assert torch.equal(a[2:], b)


@pytest.mark.parametrize("V", VS)
def test_equal_records_give_the_bits_of_the_scalar_launch_at_B_rows(V):
    x = torch.tensor(_logits(V), device="cuda")
    seq = torch.tensor(SEQ, device="cuda")
    for rec in (records(V)[5], records(V)[2], records(V)[0], dict(do_sample=True)):
        want = ops.sample_logits(x, position=21, sequence_ids=seq, history=_hist(V), hist_len=HIST, return_debug=True, **rec)
        got = ops.sample_logits(x, rows=_table(V, [rec] * B), position=21, sequence_ids=seq, history=_hist(V), hist_len=HIST, return_debug=True)
        for a, b in zip(want, got):
            assert torch.equal(a, b), rec
        again = ops.sample_logits(x, rows=_table(V, [rec] * B), position=21, sequence_ids=seq, history=_hist(V), hist_len=HIST, return_debug=True)
        for a, b in zip(got, again):
            assert torch.equal(a, b)                                                              # two calls give identical bits


def test_a_budget_finishes_the_row_in_the_launch_that_writes_its_last_token():
    V, n = 1500, 4
    x = torch.tensor(_logits(V)[:3], device="cuda")
    sample = dict(do_sample=True, temperature=0.9, top_k=50, seed=6)
    table = _table(V, [dict(sample, max_new_tokens=1), dict(sample, max_new_tokens=3), dict(sample)])
    assert table.flags == H.SAMPLE_ROWS_BUDGET
    out = torch.full((3, n), -7, dtype=torch.int64, device="cuda")
    free = torch.full((3, n), -7, dtype=torch.int64, device="cuda")
    finished, never = torch.zeros(3, dtype=torch.uint8, device="cuda"), torch.zeros(3, dtype=torch.uint8, device="cuda")
    flips = []
    for col in range(n):
        ops.sample_logits(x, rows=table, position=10 + col, finished=finished, out_tokens=out, out_col=col, pad_token_id=PAD)
        ops.sample_logits(x, position=10 + col, finished=never, out_tokens=free, out_col=col, pad_token_id=PAD, **sample)   # no budget
        flips.append(finished.cpu().tolist())
    assert flips == [[1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 0]]                                  # out_col + 1 >= max_new, and not before
    out, free = out.cpu(), free.cpu()
    assert torch.equal(out[0], torch.tensor([int(free[0, 0]), PAD, PAD, PAD]))                    # the token of that launch is emitted
    assert torch.equal(out[1], torch.tensor([*free[1, :3].tolist(), PAD]))
    assert torch.equal(out[2], free[2]) and never.sum() == 0
    # an EOS ends the row earlier, the budget not at all; and flag bit 1 clear reads every budget as 0
    eos = int(free[1, 0])
    fin = torch.zeros(3, dtype=torch.uint8, device="cuda")
    tok = ops.sample_logits(x, rows=table, position=10, finished=fin, eos_token_id=eos, out_col=0, pad_token_id=PAD)
    assert fin.cpu().tolist() == [1, 1, int(free[2, 0]) == eos] and int(tok[1]) == eos
    fin = torch.zeros(3, dtype=torch.uint8, device="cuda")
    ops.sample_logits(x, rows=_table(V, [dict(sample, max_new_tokens=1)] * 3, flags=0), position=10, finished=fin, out_col=0)
    assert fin.sum() == 0
    with pytest.raises(RuntimeError, match="null finished"):
        ops.sample_logits(x, rows=table, position=10, out_col=0)


@pytest.mark.parametrize("V", [37, 1500])
def test_a_penalty_without_the_bitmap_is_read_as_one(V):
    x = torch.tensor(_logits(V), device="cuda")
    seq = torch.tensor(SEQ, device="cuda")
    recs = records(V)
    plain = [dict(r, repetition_penalty=1.0) for r in recs]
    want = ops.sample_logits(x, rows=_table(V, plain), position=5, sequence_ids=seq, return_debug=True)
    launches = [dict(rows=_table(V, recs, flags=0), history=_hist(V), hist_len=HIST),             # flag bit 0 clear
                dict(rows=_table(V, recs)),                                                        # no history
                dict(rows=_table(V, recs), history=_hist(V), hist_len=0)]                          # an empty history
    for kw in launches:
        got = ops.sample_logits(x, position=5, sequence_ids=seq, return_debug=True, **kw)
        for a, b in zip(want, got):
            assert torch.equal(a, b)
    for b in (4, 5):                                                                              # and r = 1 is what the scalar launch gives
        t, k, m = _scalar_row(V, b, plain[b], position=5, history=False)
        assert int(want[0][b]) == t and int(want[1][b]) == k and np.array_equal(want[2][b].cpu().numpy(), m)
    # with the bitmap the launch appended every row's token to the history, as the scalar launch does
    h = _hist(V)
    got = ops.sample_logits(x, rows=_table(V, recs), position=5, sequence_ids=seq, history=h, hist_len=HIST, return_debug=True)
    assert torch.equal(h[:, HIST], got[0])


def test_finished_rows_and_rows_without_a_candidate_behave_as_in_the_scalar_launch():
    V = 1500
    x = torch.tensor(_logits(V), device="cuda").clone()
    x[3] = float("-inf")                                                                          # no candidate
    x[4, 1:] = float("nan")
    seq = torch.tensor(SEQ, device="cuda")
    fin0 = torch.tensor([0, 1, 0, 0, 0, 1], dtype=torch.uint8, device="cuda")
    f1, f2 = fin0.clone(), fin0.clone()
    got = ops.sample_logits(x, rows=_table(V, [records(V)[5]] * B), position=8, sequence_ids=seq, finished=f1, pad_token_id=PAD,
                            eos_token_id=0, return_debug=True)
    want = ops.sample_logits(x, position=8, sequence_ids=seq, finished=f2, pad_token_id=PAD, eos_token_id=0, return_debug=True, **records(V)[5])
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert torch.equal(f1, f2) and f1.cpu().tolist()[:4] == [0, 1, 0, 1]
    assert got[0][[1, 3, 5]].cpu().tolist() == [PAD] * 3 and got[1][[1, 3, 5]].sum() == 0 and got[2][[1, 3, 5]].sum() == 0
    assert int(got[0][4]) == 0 and f1[4] == 1                                                     # the one candidate is the EOS


def test_the_table_is_what_the_library_packed():
    with pytest.raises(ValueError, match="row 1: top_p"):
        _table(37, [dict(), dict(top_p=0.0)])
    with pytest.raises(ValueError, match="names"):
        _table(37, [dict(presence_penalty=1.0)])
    t = _table(37, [dict(min_p=0.25, seed=-1)])
    assert t.host[0].seed == 2 ** 64 - 1 and t.table.numel() == 56 and bytes(t.table.cpu().numpy()) == bytes(t.host)
    x = torch.tensor(_logits(37), device="cuda")
    with pytest.raises(ValueError, match="records"):
        ops.sample_logits(x, rows=t, position=0)
