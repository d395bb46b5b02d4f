"""kx_constrain_logits on the device against the NumPy restatement of its contract (tests/constrain_ref.py), exactly: every
output element is either the input's bit pattern or -inf, ``finished`` equals the reference's, and nothing around the rows is
written — the rows are a ``[:, -1]`` view of a [B + 2, 4, V] tensor (ld = 4 V != V) whose first and last batch entries are guards."""
import numpy as np
import pytest
import torch

import constrain_ref as CR
from kosmosx import ops

pytestmark = pytest.mark.gpu

B = 3
A = 7            # histories over 7 ids: matches are plentiful


def _check(hist, hist_len, V, *, seed=0, prompt_width=None, prompt_lens=None, g=0, ngram=0, bad=(), stop=(), min_new=0, eos=None,
           finished=None, extra_cols=1, ref_lens=None):
    """One launch on B rows; returns (ban masks [B, V], finished [B]) after comparing everything with the reference."""
    rng = np.random.default_rng(seed)
    hist = np.asarray(hist, dtype=np.int64).reshape(B, -1)
    assert hist.shape[1] >= hist_len
    phys = np.concatenate([hist[:, :hist_len], np.full((B, extra_cols), 3, dtype=np.int64)], axis=1)   # room to append
    full = (rng.standard_normal((B + 2, 4, V)) * 3).astype(np.float32)
    full[1, -1, 5], full[2, -1, 6] = np.nan, -np.inf                              # input bits are kept whatever they are
    dev = torch.from_numpy(full).cuda()
    rows = dev[1:B + 1, -1]
    assert rows.stride(0) == 4 * V and rows.shape == (B, V)
    fin_in = np.zeros(B, dtype=np.uint8) if finished is None else np.asarray(finished, dtype=np.uint8)
    fin = torch.from_numpy(fin_in.copy()).cuda()
    h = torch.from_numpy(phys).cuda() if hist_len or prompt_lens is not None else None
    ops.constrain_logits(rows, history=h, hist_len=hist_len if h is not None else 0,
                         prompt_width=0 if prompt_width is None else prompt_width,
                         prompt_lens=None if prompt_lens is None else torch.tensor(prompt_lens, dtype=torch.int32).cuda(),
                         new_tokens=g, no_repeat_ngram_size=ngram, bad_words=ops.SequenceTable(bad, "cuda") if bad else None,
                         stop_sequences=ops.SequenceTable(stop, "cuda") if stop else None, min_new_tokens=min_new,
                         eos_token_id=eos, finished=fin)
    torch.cuda.synchronize()
    got, got_fin = dev.cpu().numpy(), fin.cpu().numpy()
    want, bans = full.copy(), np.zeros((B, V), dtype=bool)
    for b in range(B):
        s = CR.logical(phys[b], hist_len, prompt_width, None if prompt_lens is None else (ref_lens or prompt_lens)[b])
        ban, f = CR.constrain_row(s, full[1 + b, -1], new_tokens=g, ngram=ngram, bad_words=bad, stop_sequences=stop, min_new=min_new,
                                  eos_id=eos, finished=bool(fin_in[b]))
        want[1 + b, -1] = CR.apply(full[1 + b, -1], ban)
        bans[b] = ban
        assert bool(got_fin[b]) == f, (b, got_fin, f)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))             # the rows, the other 3 slots of each, both guards
    if h is not None:
        assert np.array_equal(h.cpu().numpy(), phys)
    return bans, got_fin


def _history(rng, n, N, planted):
    h = rng.integers(0, A, (B, n))
    if planted and n >= N:
        for b in range(B):
            if n - N + 1 >= N - 1:
                h[b, :N - 1] = h[b, n - N + 1:]
            else:
                h[b, :] = h[b, 0]
    return h


@pytest.mark.parametrize("V", [502, 1003])
def test_ngram_bad_words_and_minimum_length_against_the_reference(V):
    rng = np.random.default_rng(V)
    cases = 0
    for N in (1, 2, 3, 5):
        for n in sorted({0, 1, N - 1, N, 70, 700}):                               # 700: more than two strides of the workgroup
            for planted in (False, True):
                h = _history(rng, n, N, planted)
                bans, _ = _check(h, n, V, seed=n + N, ngram=N)
                if planted and n >= N:                                            # a planted repeat bans in every row: nothing vacuous
                    assert bans.any(axis=1).all(), (N, n)
                    cases += 1
                # everything at once: bad words (singles; prefixes cut from row 0's tail, so some complete), the minimum length
                words = [[int(rng.integers(0, V))], [int(t) for t in rng.integers(0, A, 2)]]
                for m in (2, 3, 4, 64):
                    if n >= m - 1:
                        words.append([int(t) for t in h[0, n - (m - 1):]] + [int(rng.integers(0, V))])
                _check(h, n, V, seed=n, g=2, ngram=N, bad=words, min_new=3, eos=V - 1)
                _check(h, n, V, seed=n, g=3, bad=words, min_new=3, eos=V - 1)     # g == min_new: EOS is free again
    assert cases == 4 * 3                                                         # n in {N, 70, 700} for each N


def test_the_largest_ngram_and_sequences():
    """ngram = 64 (a 63-id prefix) over a periodic history, a 64-id bad word and a 64-id stop sequence: the staged tail in full."""
    V, n = 502, 700
    rng = np.random.default_rng(1)
    period = rng.integers(0, 400, 90)
    h = np.stack([np.resize(np.roll(period, b), n) for b in range(B)])
    bans, _ = _check(h, n, V, ngram=64)
    assert bans.any(axis=1).all()                                                 # every row's 63-gram recurs 90 tokens earlier
    word = [int(t) for t in h[1, n - 63:]] + [77]
    bans, _ = _check(h, n, V, bad=[word])
    assert bans[1, 77] and bans.sum() == 1
    _, fin = _check(h, n, V, g=1, stop=[[int(t) for t in h[2, n - 64:]]], ngram=1)
    assert list(fin) == [0, 0, 1]


def test_ragged_padding_takes_part_in_no_match():
    """prompt_lens = [2, 5, 9] at prompt_width = 9, padded as mask_padding pads (copies of the row's first token), generated columns
    after it.  Row 0 = [a, b] + padding [a] * 7 + generated [c, d, a], N = 2: the logical sequence [a, b, c, d, a] bans b alone;
    the padding holds the 2-gram (a, a), which a scan over physical columns would ban too."""
    V, W, lens = 502, 9, [2, 5, 9]
    a, b_, c, d = 11, 12, 13, 14
    rng = np.random.default_rng(2)
    prompts = rng.integers(20, 20 + A, (B, W))
    prompts[0, :2] = (a, b_)
    for r, L in enumerate(lens):
        prompts[r, L:] = prompts[r, 0]
    gen = rng.integers(20, 20 + A, (B, 3))
    gen[0] = (c, d, a)
    h = np.concatenate([prompts, gen], axis=1)
    bans, _ = _check(h, W + 3, V, prompt_width=W, prompt_lens=lens, g=3, ngram=2)
    assert set(np.nonzero(bans[0])[0]) == {b_}                                    # not a
    for N in (1, 3):
        _check(h, W + 3, V, prompt_width=W, prompt_lens=lens, g=3, ngram=N)
    # one generated token: the staged tail crosses the padding.  Row 0 is [a, b, c]: the bad word [b, c, 99] completes, [a, c, 98]
    # (the physical neighbours) does not; the stop sequence [b, c] starts inside the prompt and ends in the generated part
    bans, fin = _check(h, W + 1, V, prompt_width=W, prompt_lens=lens, g=1, bad=[[b_, c, 99], [a, c, 98]], ngram=2)
    assert set(np.nonzero(bans[0])[0]) == {99}
    _, fin = _check(h, W + 1, V, prompt_width=W, prompt_lens=lens, g=1, stop=[[b_, c]], ngram=2)
    assert list(fin) == [1, 0, 0]
    _, fin = _check(h, W + 1, V, prompt_width=W, prompt_lens=lens, g=1, stop=[[a, c]])          # physical neighbours: no stop
    assert not fin.any()
    # a prompt_lens entry outside [0, prompt_width] is clamped into it (memory safety does not depend on device data)
    _check(h, W + 3, V, prompt_width=W, prompt_lens=[W + 50, -3, 5], ref_lens=[W, 0, 5], g=3, ngram=2)


@pytest.mark.parametrize("V", [502, 1003])
def test_ids_outside_the_vocabulary_ban_nothing_and_corrupt_nothing(V):
    rng = np.random.default_rng(3)
    h = rng.integers(0, A, (B, 70))
    h[:, 10], h[:, 40], h[:, 69] = -1, V + 5, -1                                  # in the prefix position and as the id to ban
    h[1, 68], h[1, 20] = V + 5, V + 5
    h[1, 69], h[1, 21] = V, V                                                     # the 2-gram (V + 5, V) recurs: its ban is out of range
    h[2, 69] = 2 ** 40
    for N in (1, 2):
        _check(h, 70, V, ngram=N, bad=[[-1], [V + 5], [V], [-1, V + 5], [int(h[0, 68]), -1, V + 7], [2 ** 40, 3]], min_new=2, eos=V)
    bans, _ = _check(h, 70, V, ngram=1)
    assert bans.sum(axis=1).max() <= A                                            # only the ids of the alphabet
    bans, _ = _check(h, 70, V, bad=[[2 ** 40, 3]])
    assert list(np.nonzero(bans[2])[0]) == [3] and not bans[:2].any()             # an out-of-range id still matches as a value


def test_stop_sequences_and_finished_rows():
    V, n = 502, 12
    rng = np.random.default_rng(4)
    h = rng.integers(0, A, (B, n))
    h[0, -2:] = (300, 301)                                                        # row 0 ends in the stop sequence
    h[1, 3:5] = (300, 301)                                                        # row 1 holds it in the middle only
    h[2, -1] = 300
    stop = [[300, 301], [400]]
    _, fin = _check(h, n, V, g=2, stop=stop, ngram=1, bad=[[9]])
    assert list(fin) == [1, 0, 0]                                                 # (and row 0 got no bans: _check compared it)
    _, fin = _check(h, n, V, g=0, stop=stop, ngram=1)                             # g = 0: the prompt alone never stops a row
    assert not fin.any()
    h2 = h.copy()
    h2[2, -1] = 400
    _, fin = _check(h2, n, V, g=1, stop=stop)                                     # a one-id stop sequence
    assert list(fin) == [1, 0, 1]
    _, fin = _check(h, n, V, g=2, stop=[[int(t) for t in h[1, :n]] + [5]])        # longer than the sequence
    assert not fin.any()
    # an already finished row is left untouched (no bans), the others are processed
    bans, fin = _check(h, n, V, g=2, ngram=1, bad=[[9]], min_new=5, eos=8, finished=[0, 1, 0])
    assert list(fin) == [0, 1, 0] and not bans[1].any() and bans[0].any() and bans[2].any()
    # the wrapper names a history too short to append to, and a prompt_width beyond the columns in use
    rows, hh = torch.zeros(B, V).cuda(), torch.zeros((B, n), dtype=torch.int64).cuda()
    with pytest.raises(ValueError, match="constrain_logits: hist_len = 12 outside"):
        ops.constrain_logits(rows, history=hh, hist_len=n, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="constrain_logits: prompt_width = 11 outside"):
        ops.constrain_logits(rows, history=hh, hist_len=10, prompt_width=11, prompt_lens=torch.zeros(B, dtype=torch.int32).cuda())
    # no history at all (the beam-search form): single-id bad words and the minimum length
    bans, _ = _check(np.zeros((B, 0)), 0, V, g=1, bad=[[9], [10]], min_new=2, eos=8)
    assert all(set(np.nonzero(bans[b])[0]) == {8, 9, 10} for b in range(B))
