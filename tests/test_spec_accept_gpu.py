"""kx_spec_accept (csrc/kx_spec.hip) against tests/spec_ref.py: integer work, so every output is compared for equality — the
outputs, the history, the counters, the positions, the finished bytes, out_src, emitted and the next block's tokens, and the
slots the launch must not touch (sentinels)."""
import random

import pytest
import torch

import spec_ref as R
from kosmosx import ops

pytestmark = pytest.mark.gpu

S_HIST, S_SRC, S_EMIT, S_NEXT = -7, -1, -2, -9               # sentinels in what the launch may leave untouched


def _check(seqs, *, K, Kin, max_new, step, ngram_max=2, eos=None, pad=1, prefill_len=5, draft_from=None):
    """``seqs``: per sequence dict(history, out, finished, base, fed, picked[, out_src]).  Launch once, compare with R.step."""
    B = len(seqs)
    hist_ld = max(len(s["history"]) + max_new - len(s["out"]) for s in seqs) + 3
    dev = "cuda"
    history = torch.full((B, hist_ld), S_HIST, dtype=torch.int64)
    out = torch.full((B, max_new), pad, dtype=torch.int64)
    out_src = torch.full((B, max_new), S_SRC, dtype=torch.int32)
    emitted = torch.full((B, step + 2), S_EMIT, dtype=torch.int32)
    positions = torch.full((B * K,), -5, dtype=torch.int32)
    want = []
    for b, s in enumerate(seqs):
        history[b, :len(s["history"])] = torch.tensor(s["history"], dtype=torch.int64)
        out[b, :len(s["out"])] = torch.tensor(s["out"], dtype=torch.int64) if s["out"] else out[b, :0]
        src = s.get("out_src", list(range(len(s["out"]))))
        out_src[b, :len(src)] = torch.tensor(src, dtype=torch.int32) if src else out_src[b, :0]
        if Kin == K:
            positions[b * K:(b + 1) * K] = torch.arange(K, dtype=torch.int32) + s["base"]
        st = dict(history=list(s["history"]), out=list(s["out"]), out_src=list(src), finished=bool(s["finished"]),
                  base=s["base"] if Kin == K else None, prefill_len=prefill_len)
        e, nxt = R.step(st, s["fed"], s["picked"], K=K, max_new=max_new, step_index=step, ngram_max=ngram_max, eos=eos, pad=pad,
                        draft_from=None if draft_from is None else draft_from[b])
        want.append((st, e, nxt))
    n_out = torch.tensor([len(s["out"]) for s in seqs], dtype=torch.int32)
    hist_len = torch.tensor([len(s["history"]) for s in seqs], dtype=torch.int32)
    finished = torch.tensor([int(s["finished"]) for s in seqs], dtype=torch.uint8)
    picked = torch.tensor([t for s in seqs for t in s["picked"]], dtype=torch.int64)
    fed = torch.tensor([t for s in seqs for t in s["fed"]], dtype=torch.int64) if Kin == K else None
    nxt = torch.full((B * K,), S_NEXT, dtype=torch.int64)
    df = None if draft_from is None else torch.tensor(draft_from, dtype=torch.int64).cuda()
    d = dict(history=history.to(dev), out=out.to(dev), out_src=out_src.to(dev), emitted=emitted.to(dev), positions=positions.to(dev),
             n_out=n_out.to(dev), hist_len=hist_len.to(dev), finished=finished.to(dev), nxt=nxt.to(dev))
    ops.spec_accept(picked.to(dev), fed=None if fed is None else fed.to(dev), rows_per_sequence=K, positions=d["positions"],
                    prefill_len=prefill_len, history=d["history"], hist_len=d["hist_len"], out_tokens=d["out"], n_out=d["n_out"],
                    finished=d["finished"], next_tokens=d["nxt"], max_new_tokens=max_new, step=step, ngram_max=ngram_max,
                    eos_token_id=eos, pad_token_id=pad, out_src=d["out_src"], emitted=d["emitted"], draft_from=df)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in d.items()}
    for b, (st, e, nx) in enumerate(want):
        tag = (b, e, st["out"][-4:])
        assert got["history"][b].tolist() == st["history"] + [S_HIST] * (hist_ld - len(st["history"])), tag
        assert got["out"][b].tolist() == st["out"] + [pad] * (max_new - len(st["out"])), tag
        assert got["out_src"][b].tolist() == st["out_src"] + [S_SRC] * (max_new - len(st["out_src"])), tag
        assert got["emitted"][b].tolist() == [S_EMIT] * step + [e, S_EMIT], tag
        assert int(got["n_out"][b]) == len(st["out"]) and int(got["hist_len"][b]) == len(st["history"]), tag
        assert bool(got["finished"][b]) == st["finished"], tag
        pos = [-5] * K if st["base"] is None else [st["base"] + j for j in range(K)]
        assert got["positions"][b * K:(b + 1) * K].tolist() == pos, tag
        assert got["nxt"][b * K:(b + 1) * K].tolist() == nx, tag
    return want


def _seq(history, n_out, fed_drafts, picked, finished=False, base=40):
    return dict(history=list(history), out=list(history[len(history) - n_out:]), finished=finished, base=base,
                fed=[history[-1]] + list(fed_drafts), picked=list(picked))


def test_the_first_step_initialises_positions_and_drafts_from_the_prompt():
    seqs = [dict(history=[3, 4, 5, 3, 4], out=[], finished=False, base=None, fed=None, picked=[5]),       # the lookup continues 3 4 5
            dict(history=[6], out=[], finished=False, base=None, fed=None, picked=[2]),                    # no match: 2 2 2
            dict(history=[1, 2, 1, 2], out=[], finished=False, base=None, fed=None, picked=[0])]           # EOS at once
    for K in (2, 4, 16):
        want = _check(seqs, K=K, Kin=1, max_new=9, step=0, eos=0, pad=1, prefill_len=12)
        assert want[0][2][:2] == [5, 3] and want[0][0]["base"] == 12 and want[1][2] == [2] * K
        assert want[2][0]["finished"] and want[2][2] == [1] * K and want[2][1] == 1
    _check(seqs[:1], K=4, Kin=1, max_new=1, step=0, prefill_len=3)                                      # the budget of one token


def test_all_some_and_none_accepted():
    h = [1, 2, 3, 4, 5, 6, 1, 2]
    for K in (2, 4, 16):
        right = [3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6][:K]                                     # picks = the continuation
        seqs = [_seq(h, 2, right[:K - 1], right),                                                         # every draft right: K emitted
                _seq(h, 2, [0] * (K - 1), right),                                                         # none: one emitted
                _seq(h, 2, right[:K // 2] + [0] * (K - 1 - K // 2), right)]                              # the first K // 2
        want = _check(seqs, K=K, Kin=K, max_new=40, step=3)
        assert [w[1] for w in want] == [K, 1, K // 2 + 1]


def test_eos_budget_finished_and_draft_from():
    K = 4
    h = [5, 6, 5, 6, 5]
    # EOS inside the accepted run: cut after it; the budget cut; a finished row; EOS as the correction token
    seqs = [_seq(h, 3, [6, 2, 6], [6, 2, 6, 5]), _seq(h, 3, [6, 5, 6], [6, 5, 6, 5]), _seq(h, 3, [6, 5, 6], [6, 5, 6, 5], finished=True),
            _seq(h, 1, [1, 1, 1], [2, 3, 3, 3])]
    want = _check(seqs, K=K, Kin=K, max_new=5, step=2, eos=2, pad=0)
    assert [w[1] for w in want] == [2, 2, 0, 1] and [w[0]["finished"] for w in want] == [True, True, True, True]
    # draft_from: per output slot; slots past its end get the last token
    df = [[10, 11, 12, 13, 14, 15, 16, 17], [20, 21, 22, 23, 24, 25, 26, 27]]
    seqs = [_seq(h, 3, [6, 5, 6], [6, 5, 6, 4]), _seq(h, 5, [0, 0, 0], [3, 3, 3, 3])]
    want = _check(seqs, K=K, Kin=K, max_new=8, step=1, draft_from=df)
    assert want[0][2] == [4, 17, 4, 4] and want[1][2] == [3, 26, 27, 3]


def test_out_of_range_ids_are_values_not_indices():
    """Ids far outside any vocabulary, negative ones included, in the history, the picks and the fed block: compared and copied,
    never used as an index (the launch neither faults nor writes outside its rows: the sentinels hold)."""
    big, neg = 2 ** 40 + 3, -(2 ** 35)
    h = [big, neg, 7, big, neg]
    seqs = [_seq(h, 2, [7, big, neg], [7, big, 1, 1]), _seq([neg] * 70, 5, [neg, neg, neg], [neg, neg, neg, big])]
    want = _check(seqs, K=4, Kin=4, max_new=30, step=1, ngram_max=64)
    assert want[0][1] == 3 and want[0][2] == [1, 1, 1, 1] and want[1][2][0] == big


@pytest.mark.parametrize("K", [2, 4, 16])
def test_long_histories_where_the_strided_scan_wraps(K):
    """More start positions than the workgroup has threads: the match sits in a later stride, in several strides (the largest
    start wins), or only at the very first position."""
    rng = random.Random(K)
    base = [rng.randrange(100, 200) for _ in range(700)]      # ids 100..199; the markers 1..6 occur only where placed
    a = list(base)
    a[300:303] = [1, 2, 3]
    a[-2:] = [1, 2]                                            # the 2-gram at 300 (second stride)
    b = list(base)
    for at in (10, 270, 530):
        b[at:at + 3] = [1, 2, at]
    b[-2:] = [1, 2]                                            # three occurrences: 530 wins
    c = list(base)
    c[0:3] = [4, 5, 6]
    c[-2:] = [4, 5]                                            # only at position 0
    d = list(base)
    d[513] = 6
    d[-1] = 6                                                  # no 2-gram, the 1-gram in the third stride
    seqs = [_seq(s, 4, [0] * (K - 1), [7] * K) for s in (a, b, c, d)]
    want = _check(seqs, K=K, Kin=K, max_new=64, step=5, ngram_max=2)
    # (the emitted token 7 is appended first: the suffix looked up is "2 7" / "5 7", which has no match, then the 1-gram 7)
    assert all(w[2] == [7] * K for w in want)
    seqs = [_seq(s, 4, [0] * (K - 1), [s[-1]] * K) for s in (a, b, c, d)]                                 # ... so emit the marker itself
    for s, m in zip(seqs, (a, b, c, d)):
        s["history"] = m[:-1]
        s["out"] = m[-5:-1]
        s["fed"] = [m[-2]] + [0] * (K - 1)
    want = _check(seqs, K=K, Kin=K, max_new=64, step=5, ngram_max=2)
    assert want[0][2][:2] == [2, 3] and want[1][2][:2] == [2, 530] and want[2][2][:2] == [5, 6] and want[3][2][1] == base[514]


@pytest.mark.parametrize("K", [2, 4, 16])
def test_random_small_cases(K):
    rng = random.Random(77 + K)
    V = 7
    for case in range(40):
        B = rng.randrange(1, 5)
        max_new = rng.randrange(1, 40)
        eos = rng.choice([None, rng.randrange(V)])
        use_df = case % 4 == 3
        seqs, df = [], []
        for b in range(B):
            n_out = rng.randrange(0, max_new)
            L = n_out + rng.randrange(1, 1 + rng.choice([4, 30, 300]))
            h = [rng.randrange(V) for _ in range(L)]
            picked = [rng.randrange(V) for _ in range(K)]
            drafts = [picked[j] if rng.random() < 0.75 else (picked[j] + 1) % V for j in range(K - 1)]
            seqs.append(_seq(h, n_out, drafts, picked, finished=rng.random() < 0.15, base=rng.randrange(0, 500)))
            df.append([rng.randrange(V) for _ in range(max_new)])
        _check(seqs, K=K, Kin=K, max_new=max_new, step=rng.randrange(0, 50), ngram_max=rng.choice([1, 2, 3, 64]), eos=eos,
               pad=rng.randrange(V), draft_from=df if use_df else None)
        if case % 5 == 0:                                     # ... and as a first step
            first = [dict(history=s["history"], out=[], finished=False, base=None, fed=None, picked=s["picked"][:1]) for s in seqs]
            _check(first, K=K, Kin=1, max_new=max_new, step=0, ngram_max=2, eos=eos, prefill_len=rng.randrange(1, 90))
