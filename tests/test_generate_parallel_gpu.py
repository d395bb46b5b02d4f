"""Parallel sampling: generate(do_sample=True, num_return_sequences=n) — n continuations per prompt over ONE prompt KV cache.

The loop contract: after one prefill at B rows, (a) the new path (generation.parallel_loop: the prompt's caches read only, a private
tail cache per sample, kx_decoder_decode_step_prefix) against (b) generation.generate_loop on a state whose caches were repeated per
sample — same seed, sequence ids and lengths.  The step's attention gives the ragged launch's bits on the assembled cache
(tests/test_attention_decode_prefix_gpu.py) and everything else in the step is row-wise, so the tokens are equal and the logits
bit-equal.  (b) is the path tests/test_generate_ragged_gpu.py holds against the CPU oracle.  Then the public surface."""
import pytest
import torch

from helpers import tiny_config
from kosmosx import generation as G
from kosmosx.model import Kosmos, KosmosLanguage

pytestmark = pytest.mark.gpu

V = 102
SAMPLE = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, repetition_penalty=1.15, seed=33)
PRECS = pytest.mark.parametrize("prec", ["fp32", "mixed"])


def _lm(max_pos=64, seed=5):
    return KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=seed, _perturb=0.1,
                          _max_positions=max_pos).eval().to("cuda")


def _tok(B, T, seed=4, vocab=V):
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _loop_pair(model, prompt, prompt_lengths, n, N, kw, chunk=None):
    """-> ((tokens, logits) of parallel_loop, (tokens, logits) of generate_loop on the caches repeated per sample)."""
    with torch.no_grad():
        tokens, lens, T, state, logits, prows = G._prefill(model, prompt, prompt_lengths, N, chunk=chunk)
        B = tokens.shape[0]
        plens = [T] * B if lens is None else [prompt["prefix_rows"] + l for l in lens]
        tlens = [tokens.shape[1]] * B if lens is None else lens
        seq = [b for b in range(B) for _ in range(n)]
        rep = dict(state)
        rep.update(kcache=state["kcache"].repeat_interleave(n, dim=1), vcache=state["vcache"].repeat_interleave(n, dim=1), batch=B * n)
        if prows is None:
            first = logits[torch.arange(B, device="cuda"), torch.tensor([l - 1 for l in plens], device="cuda")]
        else:
            first = logits[:, 0]
        first = first.repeat_interleave(n, dim=0).unsqueeze(1).clone()
        opts = G.loop_options(logits.shape[2], B, output_logits=True, **kw)   # (nothing per row among them: the same for both)
        a = G.parallel_loop(model.decoder, model.precision, state, logits, tokens.long(), N, opts, num_return_sequences=n,
                            pos_shift=prompt["pos_shift"], lengths=None if lens is None else plens, text_lengths=lens, prompt_rows=prows)
        b = G.generate_loop(model.decoder, model.precision, rep, first, tokens.long().repeat_interleave(n, dim=0), N, opts,
                            pos_shift=prompt["pos_shift"], lengths=[plens[i] for i in seq], text_lengths=[tlens[i] for i in seq],
                            prompt_rows=T)
        assert "prefix" in state and "prefix" not in rep
        assert tuple(state["prefix"]["ktail"].shape) == (state["kcache"].shape[0], B * n, state["kcache"].shape[2], N, 64)
        assert state["kcache"].shape[1] == B and rep["kcache"].shape[1] == B * n
        assert int(state["error"].item()) == 0 and int(rep["error"].item()) == 0
    return a, b


def _assert_same(a, b, rows, N):
    assert a[0].shape == (rows, N) and a[0].dtype == torch.int64 and a[1].shape == (rows, N, b[1].shape[2])
    assert bool(torch.isfinite(a[1]).all())
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])                                            # bit-equal logits


@PRECS
@pytest.mark.parametrize("B,n", [(2, 3), (3, 6)], ids=["6-rows-streaming", "18-rows-tiles"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "prompt_lengths"])
def test_the_loop_gives_the_bits_of_the_loop_on_repeated_caches(prec, B, n, ragged):
    lm = _lm()
    lm.precision = prec
    tok, N = _tok(B, 11), 14
    lens = [11, 5, 8][:B] if ragged else None
    a, b = _loop_pair(lm, lm._prompt(tok), lens, n, N, SAMPLE)
    _assert_same(a, b, B * n, N)
    # the public call is the loop: same tokens and logits, row b * n + i
    got, logits = lm.generate(tok, N, num_return_sequences=n, output_logits=True, prompt_lengths=lens, **SAMPLE)
    assert torch.equal(got, a[0]) and torch.equal(logits, a[1])
    for r in range(B):                                                        # the samples of one prompt start from one logits row,
        assert all(torch.equal(logits[r * n, 0], logits[r * n + i, 0]) for i in range(n))
    assert not torch.equal(logits[0, 0], logits[n, 0])                        # the next prompt's from another: row b * n + i


def test_constraints_and_a_stop_sequence_work_row_by_row():
    lm = _lm()
    lm.precision = "fp32"
    tok, N, B, n = _tok(2, 9, seed=8), 16, 2, 3
    free = lm.generate(tok, N, num_return_sequences=n, **SAMPLE)
    stop = [[int(free[1, 4]), int(free[1, 5])]]                               # two ids row 1 generates, unconstrained
    kw = dict(SAMPLE, no_repeat_ngram_size=2, stop_sequences=stop, eos_poll=4)
    a, b = _loop_pair(lm, lm._prompt(tok), None, n, N, kw)
    width = a[0].shape[1]
    _assert_same(a, b, B * n, width)
    got = a[0].cpu()
    for r in range(B * n):                                                    # no bigram of prompt + output occurs twice
        row = got[r].tolist()
        cut = next((j + 2 for j in range(width - 1) if row[j:j + 2] == stop[0]), width)
        assert all(t == 1 for t in row[cut:])                                 # padded after the stop sequence
        ids = tok[r // n].tolist() + row[:cut]
        grams = list(zip(ids, ids[1:]))
        assert len(set(grams)) == len(grams), r


def test_shape_order_seeds_and_diversity():
    lm = _lm()
    lm.precision = "fp32"
    B, n, N = 2, 4, 16
    tok = _tok(B, 10, seed=6)
    kw = dict(do_sample=True, temperature=1.5, seed=3)
    got = lm.generate(tok, N, num_return_sequences=n, **kw)
    assert got.shape == (B * n, N) and got.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < V
    assert torch.equal(lm.generate(tok, N, num_return_sequences=n, **kw), got)                       # the same seed, the same tokens
    assert not torch.equal(lm.generate(tok, N, num_return_sequences=n, **dict(kw, seed=4)), got)     # another seed
    for b in range(B):
        rows = got[b * n:(b + 1) * n]
        assert not bool((rows == rows[:1]).all()), b                          # the n samples of a prompt are not all equal
    # the default Philox streams are the rows' indices b * n + i
    assert torch.equal(lm.generate(tok, N, num_return_sequences=n, sequence_ids=torch.arange(B * n).cuda(), **kw), got)
    ids = torch.tensor([7, 7, 9, 11, 2, 2, 2, 5]).cuda()                      # equal streams over one prompt: equal samples
    same = lm.generate(tok, N, num_return_sequences=n, sequence_ids=ids, **kw)
    assert torch.equal(same[0], same[1]) and torch.equal(same[4], same[5]) and torch.equal(same[5], same[6])
    assert not torch.equal(same[0], same[2])


def test_eos_and_pad_behave_per_row():
    lm = _lm()
    lm.precision = "fp32"
    B, n, N, PAD = 2, 3, 16, 0
    tok = _tok(B, 10, seed=9)
    kw = dict(do_sample=True, temperature=1.2, seed=12)
    free = lm.generate(tok, N, num_return_sequences=n, **kw).cpu()
    eos = int(free[2, 5])                                                     # a token row 2 draws at step 5
    got = lm.generate(tok, N, num_return_sequences=n, eos_token_id=eos, pad_token_id=PAD, eos_poll=4, **kw).cpu()
    width = got.shape[1]
    ended = 0
    for r in range(B * n):
        hits = (free[r] == eos).nonzero()
        j = int(hits[0]) if len(hits) else N
        assert torch.equal(got[r, :min(j + 1, width)], free[r, :min(j + 1, width)]), r
        assert bool((got[r, j + 1:] == PAD).all()), r
        ended += j < N
    assert 1 <= ended and int(free[2].tolist().index(eos)) <= 5


def test_a_chunked_prefill_gives_the_tokens_of_the_one_piece_prefill():
    lm = _lm()
    lm.precision = "fp32"
    tok, N, n = _tok(2, 21, seed=10), 12, 3
    for lens in (None, [21, 13]):
        want = lm.generate(tok, N, num_return_sequences=n, prompt_lengths=lens, **SAMPLE)
        got = lm.generate(tok, N, num_return_sequences=n, prompt_lengths=lens, prefill_chunk=8, **SAMPLE)
        assert torch.equal(got, want)
    a, b = _loop_pair(lm, lm._prompt(tok), [21, 13], n, N, SAMPLE, chunk=8)   # (the gathered [B, 1, V] logits of the chunked prefill)
    _assert_same(a, b, 2 * n, N)
    assert torch.equal(a[0], got)


@PRECS
def test_kosmos_generate_agrees_with_the_loop_contract(prec):
    m = Kosmos._from_config(tiny_config(), seed=0, perturb=0.1).eval().to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, m.cfg.vocab, (2, 10), generator=g).cuda()
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    N, n = 12, 2
    for lens in (None, [10, 6]):
        got, logits = m.generate(tok, img, N, num_return_sequences=n, output_logits=True, prompt_lengths=lens, **SAMPLE)
        assert got.shape == (2 * n, N) and logits.shape == (2 * n, N, m.cfg.vocab)
        a, b = _loop_pair(m, m._prompt(tok, img), lens, n, N, SAMPLE)
        _assert_same(a, b, 2 * n, N)
        assert torch.equal(got, a[0]) and torch.equal(logits, a[1])


def test_a_budget_overrun_raises_before_any_launch():
    lm = _lm(max_pos=32)
    lm.precision = "fp32"
    tok = _tok(2, 9)
    rows = lm.decoder.embed_positions.weight.shape[0] - 2
    with pytest.raises(IndexError, match="index out of range in self"):
        lm.generate(tok, rows - 9 + 1, num_return_sequences=3, do_sample=True)
    got = lm.generate(tok, rows - 9, num_return_sequences=3, do_sample=True)  # the whole table
    assert got.shape == (6, rows - 9)
