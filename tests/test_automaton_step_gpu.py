"""kx_automaton_step on the device against the NumPy restatement of its contract (tests/automaton_ref.py), exactly: every output
element is either the input's bit pattern or -inf, ``state_out`` equals the reference's, ``state_in`` is unchanged and nothing
around the rows is written — the rows are a ``[:, -1]`` view of a [B + 2, 4, V] tensor (ld = 4 V != V) whose first and last batch
entries are guards (the two large cases: ld = V, rows 1..B of a [B + 2, V] tensor)."""
import numpy as np
import pytest
import torch

import automaton_ref as AR
from kosmosx import ops

pytestmark = pytest.mark.gpu

B = 3
V_LIMIT = 1 << 23                   # include/kosmosx_hip.h: kx_automaton_step's stated limit
SA, SD, NONE, FREE, ONE, BIG = range(6)
S = 6


def make_tables(V):
    """One table of six states: sparse-allow (edges on ids 0 and V - 1), sparse-deny (-1 edges on 0 and V - 1 plus one real edge),
    no edges and default -1 (the whole row is banned), no edges and a default (nothing is stored), a single edge, and the big state:
    every other id below 5003, 2502 edges from V = 5003 on — more than two strides of the workgroup over one slice and edges in two
    slices — a third of them -1.  (At tiny V the ids coincide: a later entry replaces an earlier one, the ids stay strictly ascending.)"""
    big = {t: (-1 if k % 3 == 0 else k % S) for k, t in enumerate(range(0, min(V, 5003), 2))}
    states = [({0: SD, V - 1: NONE}, -1), ({V // 2: ONE, 0: -1, V - 1: -1}, SA), ({}, -1), ({}, BIG), ({V // 2: BIG}, -1), (big, -1)]
    off, tok, nxt = [0], [], []
    for edges, _ in states:
        for t in sorted(edges):
            tok.append(t)
            nxt.append(edges[t])
        off.append(len(tok))
    return tuple(np.array(a, dtype=np.int32) for a in (off, tok, nxt, [d for _, d in states]))


def _check(tables, V, state_in, *, rows=B, src=None, last=None, finished=None, seed=0, flat=False):
    """One launch on ``rows`` rows; returns (ban masks [rows, V], state_out [rows]) after comparing everything with the reference."""
    rng = np.random.default_rng(seed)
    shape = (rows + 2, V) if flat else (rows + 2, 4, V)
    full = rng.standard_normal(shape, dtype=np.float32) * 3
    mine = full[1:rows + 1] if flat else full[1:rows + 1, -1]                        # (a view: planting writes ``full``)
    mine[0, min(5, V - 1)], mine[1, min(6, V - 1)] = np.nan, -np.inf                # input bits are kept whatever they are
    dev = torch.from_numpy(full).cuda()
    view = dev[1:rows + 1] if flat else dev[1:rows + 1, -1]
    assert view.shape == (rows, V) and view.stride(0) == (V if flat else 4 * V)
    state_in = np.asarray(state_in, dtype=np.int32)
    sin = torch.from_numpy(state_in.copy()).cuda()
    sout = torch.full((rows,), -99, dtype=torch.int32, device="cuda")
    table = ops.AutomatonTable(*tables, "cuda")
    ops.automaton_step(view, table, sin, sout,
                       src_row=None if src is None else torch.tensor(src, dtype=torch.int32).cuda(),
                       last_token=None if last is None else torch.tensor(last, dtype=torch.int64).cuda(),
                       finished=None if finished is None else torch.tensor(finished, dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    got, got_state = dev.cpu().numpy(), sout.cpu().numpy()
    want, bans, states = full.copy(), np.zeros((rows, V), dtype=bool), []
    wrows = want[1:rows + 1] if flat else want[1:rows + 1, -1]
    for b in range(rows):
        s = AR.entering_state(tables, state_in, src, b)
        s, ban = AR.step_row(tables, s, None if last is None else last[b], bool(finished[b]) if finished is not None else False, V)
        wrows[b] = AR.apply(mine[b], ban)
        bans[b] = ban
        states.append(s)
    assert got_state.tolist() == states, (got_state, states)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                 # the rows, their other slots, both guards
    assert np.array_equal(sin.cpu().numpy(), state_in)
    return bans, got_state


@pytest.mark.parametrize("V", [1, 31, 32, 33, 64, 65, 502, 5003])
def test_masks_and_advances_against_the_reference(V):
    """Bitmap word edges (31..65), one slice and two (5003 > 4096)."""
    t = make_tables(V)
    seen = []
    # every state as the entering state, plus the dead state and two values outside [0, S): mask only
    for k, enter in enumerate(([SA, SD, NONE], [FREE, ONE, BIG], [-1, S, -7])):
        bans, states = _check(t, V, enter, seed=k)
        seen.append(bans)
        assert states.tolist() == [s if 0 <= s < S else -1 for s in enter]
    assert seen[0][2].all() and not seen[1][0].any() and seen[2].all()               # NONE bans the row, FREE stores nothing, dead rows
    # advances: the first, a middle and the last listed edge of the big state
    ids = list(range(0, min(V, 5003), 2))
    bans, states = _check(t, V, [BIG] * 3, last=[ids[0], ids[len(ids) // 2], ids[-1]], seed=3)
    seen.append(bans)
    assert states.tolist() == [(-1 if k % 3 == 0 else k % S) for k in (0, len(ids) // 2, len(ids) - 1)]
    # an unlisted id without a default and with one, and a -1 edge
    unlisted = 1 if V > 2 else 0
    bans, states = _check(t, V, [SA if V > 2 else NONE, SD if V > 2 else FREE, SD], last=[unlisted, unlisted, 0], seed=4)
    seen.append(bans)
    assert states.tolist() == [-1, SA if V > 2 else BIG, -1]
    # a token outside the vocabulary
    bans, states = _check(t, V, [FREE, FREE, BIG], last=[-1, V, 1 << 40], seed=5)
    seen.append(bans)
    assert states.tolist() == [-1, -1, -1] and bans.all()
    every = np.concatenate(seen)
    assert every.any() and not every.all()                                           # nothing vacuous: bans and allowed ids both occur


def test_a_large_vocabulary_with_rows_of_alternating_alignment():
    V = 64007                                                                        # ld = V: 4 V is no multiple of 16 bytes
    t = make_tables(V)
    bans, states = _check(t, V, [SA, SD, BIG], flat=True)
    assert bans[0].sum() == V - 2 and bans[1].sum() == 2 and states.tolist() == [SA, SD, BIG]
    bans, states = _check(t, V, [BIG, FREE, ONE], last=[V - 1, 17, V // 2], flat=True, seed=1)
    assert states[1:].tolist() == [BIG, BIG] and bans.any() and not bans.all()


def test_the_vocabulary_limit_and_one_past_it():
    t = make_tables(V_LIMIT)
    bans, states = _check(t, V_LIMIT, [SA, SD, BIG], last=None, flat=True)
    assert bans[0].sum() == V_LIMIT - 2 and bans[1].sum() == 2 and not bans[2, 2] and bans[2, 1] and bans[2, V_LIMIT - 1]
    del bans
    V = V_LIMIT + 1
    rows = torch.zeros((1, V), dtype=torch.float32, device="cuda")
    sin, sout = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), -99, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="kx_automaton_step.*V=8388609 exceeds 8388608"):
        ops.automaton_step(rows, ops.AutomatonTable(*make_tables(64), "cuda"), sin, sout)
    torch.cuda.synchronize()
    assert int(sout[0]) == -99 and not bool(torch.isinf(rows).any())                 # refused before any launch


@pytest.mark.parametrize("V", [65, 502])
def test_finished_rows_keep_their_logits_and_carry_their_state(V):
    t = make_tables(V)
    bans, states = _check(t, V, [NONE, SA, 9], last=[0, 0, 0], finished=[1, 0, 1])
    assert not bans[0].any() and bans[1].any() and not bans[1].all() and not bans[2].any()
    assert states.tolist() == [NONE, SD, -1]                                         # carried over (9: dead), advanced, carried over


@pytest.mark.parametrize("V", [33, 5003])
def test_src_row_follows_the_backpointers(V):
    """B_in = 2 states feed B = 6 rows through a permutation with duplicates; one entry is out of range (the dead state)."""
    t = make_tables(V)
    bans, states = _check(t, V, [SA, BIG], rows=6, src=[1, 0, 0, 2, 1, -1], last=[2, 0, V - 1, 0, 1, 0])
    assert states.tolist() == [SD, SD, NONE, -1, -1, -1]
    assert bans[3].all() and bans[5].all() and not bans[1].all() and bans[1].any()
    bans, states = _check(t, V, [SD, FREE], rows=6, src=[0, 1, 1, 0, 1, 0], seed=1)   # no advance: step 0 of a beam search is B_in = B
    assert states.tolist() == [SD, FREE, FREE, SD, FREE, SD] and not bans[1].any() and bans[0].sum() == 2


def test_malformed_tables_change_what_is_banned_never_what_is_addressed():
    """Out-of-range edge_tok and edge_next values in an otherwise valid CSR, offsets outside [0, E] and out of order."""
    V = 502
    off, tok, nxt, dflt = (a.copy() for a in make_tables(V))
    lo = off[BIG]
    tok[lo] = -5                                            # (still ascending) skipped: id 0 falls back to the default
    tok[off[BIG + 1] - 1] = V + 3                           # skipped
    nxt[lo + 1], nxt[lo + 2], nxt[lo + 4] = S, -9, 1 << 30  # read as -1: ids 2, 4 and 8 are banned
    tok[off[ONE]] = 1 << 30                                 # the single edge of ONE: skipped, the row is banned whole
    t = (off, tok, nxt, dflt)
    bans, states = _check(t, V, [BIG, ONE, BIG], seed=0)
    assert bans[0, 0] and bans[0, 2] and bans[0, 4] and bans[0, 8] and not bans[0, 10] and bans[1].all()
    bans, states = _check(t, V, [BIG, BIG, ONE], last=[2, 10, V // 2], seed=1)
    assert states.tolist() == [-1, 5 % S, -1]
    good = make_tables(V)
    off2 = good[0].copy()
    off2[SA] = -7                                           # clamped to 0: SA as it was
    off2[ONE] += 4                                          # beyond ONE's end: out of order, no edges (NONE and FREE are not entered)
    off2[BIG + 1] = len(tok) + 1000                         # clamped to E: BIG as it was
    bans, states = _check((off2,) + good[1:], V, [SA, BIG, ONE], seed=2)
    assert bans[0].sum() == V - 2 and bans[1].any() and not bans[1].all() and bans[2].all()
    assert not _check(good, V, [SA, BIG, ONE], seed=2)[0][2].all()                   # (with its offsets in order ONE allows an id)
    dflt2 = dflt.copy()
    dflt2[FREE] = S + 4                                     # a default outside [-1, S): read as -1
    bans, states = _check((off, tok, nxt, dflt2), V, [FREE, FREE, SD], last=[3, 3, 3], seed=3)
    assert states.tolist() == [-1, -1, SA] and bans[0].all() and not bans[2].all()


def test_overlapping_state_buffers_are_refused_with_nothing_launched():
    V = 64
    table = ops.AutomatonTable(*make_tables(V), "cuda")
    rows = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    buf = torch.full((2 * B,), NONE, dtype=torch.int32, device="cuda")
    for sin, sout in ((buf[:B], buf[:B]), (buf[:B], buf[1:B + 1]), (buf[1:B + 1], buf[:B])):
        with pytest.raises(RuntimeError, match="kx_automaton_step.*overlap"):
            ops.automaton_step(rows, table, sin, sout)
    torch.cuda.synchronize()
    assert not bool(torch.isinf(rows).any()) and buf.tolist() == [NONE] * (2 * B)
    ops.automaton_step(rows, table, buf[:B], buf[B:])                                # adjacent halves do not overlap
    torch.cuda.synchronize()
    assert bool(torch.isinf(rows).all())


def test_the_wrapper_names_the_argument():
    V = 64
    table = ops.AutomatonTable(*make_tables(V), "cuda")
    rows = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    sin, sout = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError, match="table"):
        ops.automaton_step(rows, make_tables(V), sin, sout)
    with pytest.raises(TypeError, match="logits"):
        ops.automaton_step(rows.double(), table, sin, sout)
    with pytest.raises(TypeError, match="state_out"):
        ops.automaton_step(rows, table, sin, sout.long())
    with pytest.raises(TypeError, match="last_token"):
        ops.automaton_step(rows, table, sin, sout, last_token=sin)
    with pytest.raises(TypeError, match="finished"):
        ops.automaton_step(rows, table, sin, sout, finished=torch.zeros(B, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="state_in"):
        ops.automaton_step(rows, table, sin[:2], sout)
    with pytest.raises(ValueError, match="src_row"):
        ops.automaton_step(rows, table, sin[:2], sout, src_row=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="edge_off"):
        ops.AutomatonTable([0, 1, 1], [3], [0], [0], "cuda")
