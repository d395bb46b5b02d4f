"""generate(logit_bias=, presence_penalty=, frequency_penalty=, min_p=) end to end on the device.

The scheme of tests/test_generate_constrain_gpu.py: ``output_logits`` returns the model's own logits of every step; the NumPy
restatement of kx_shape_logits (tests/shape_ref.py) is applied to THOSE logits with the counts of the tokens emitted so far, then
the pick is repeated — greedy: arg max, lowest id on ties; sampled: ops.sample_logits on the reference-shaped row with the call's
seed, position and sequence id — and must reproduce the emitted token exactly.  No tolerance is involved."""
import numpy as np
import pytest
import torch

import sampling_ref as R
import shape_ref as SR
from helpers import tiny_config
from kosmosx import ops
from kosmosx.model import Kosmos, KosmosLanguage

pytestmark = pytest.mark.gpu

V = 502
PAD = 1
INF = float("inf")
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=21)
SHAPE = dict(frequency_penalty=0.7, presence_penalty=0.4)


def _lm(seed=5):
    lm = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=seed, _perturb=0.1,
                        _max_positions=64).eval().to("cuda")
    lm.precision = "fp32"
    return lm


def _tok(B, T, seed=4, vocab=V):
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(seed))


def _pairs(bias, B):
    if bias is None:
        return [()] * B
    rows = [bias] * B if hasattr(bias, "items") else list(bias)
    return [sorted(r.items()) for r in rows]


def _replay(tokens, logits, kw, positions, *, seq_ids=None, eos=None):
    """Every token of every row from the returned raw logits and zero counts at the start of the call.  Returns the counts [B, V]."""
    tokens, logits = tokens.cpu().numpy(), logits.cpu().numpy()
    B, n = tokens.shape
    vocab = logits.shape[2]
    bias = _pairs(kw.get("logit_bias"), B)
    f, p = kw.get("frequency_penalty", 0.0), kw.get("presence_penalty", 0.0)
    greedy = not kw.get("do_sample", False)
    total = np.zeros((B, vocab), dtype=np.int32)
    for b in range(B):
        counts, last, finished = np.zeros(vocab, dtype=np.int32), None, False
        for g in range(n):
            if finished:
                assert int(tokens[b, g]) == PAD, (b, g)
                continue
            row, counts = SR.shape_row(logits[b, g], counts, bias=bias[b], frequency=f, presence=p, last_token=last)
            if greedy:
                x = R.penalised(row)
                assert (x > -np.inf).any()
                want = int(np.argmax(x))                                     # (the first of exact ties)
            else:
                want = int(ops.sample_logits(torch.from_numpy(row[None]).cuda(), temperature=kw["temperature"], top_k=kw.get("top_k", 0),
                                             top_p=kw.get("top_p", 1.0), min_p=kw.get("min_p", 0.0), seed=kw["seed"],
                                             position=positions[b] + g, pad_token_id=PAD,
                                             sequence_ids=torch.tensor([b if seq_ids is None else seq_ids[b]], device="cuda"))[0])
            assert int(tokens[b, g]) == want, (b, g, int(tokens[b, g]), want)
            last = want
            finished = eos is not None and want == eos
        if last is not None and not finished:
            counts[last] += 1                                               # (the last token is counted by a launch that never came)
        total[b] = counts
    return total


def test_greedy_tokens_replay_exactly():
    lm = _lm()
    B, P, N = 3, 9, 12
    tok = _tok(B, P).cuda()
    free = lm.generate(tok, N).cpu()
    bias = [{int(free[0, 0]): -INF, 7: 3.0}, {}, {int(free[2, 1]): -2.5, 0: 1.0, V - 1: 0.5}]
    kw = dict(SHAPE, logit_bias=bias)
    got, logits = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, **kw)
    assert got.shape == (B, N) and not torch.equal(got.cpu(), free)
    assert bool(torch.isfinite(logits).all())                               # the model's own logits: no -inf from the bias
    counts = _replay(got, logits, kw, [P] * B)
    assert counts.sum() == B * N and int(free[0, 0]) not in got[0].tolist()
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, **kw), got)     # without the logits kept
    for one in (dict(logit_bias=bias), dict(frequency_penalty=-0.5), dict(presence_penalty=1.5)):
        g1, l1 = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, **one)
        _replay(g1, l1, one, [P] * B)


def test_sampled_tokens_replay_exactly_and_repeat():
    lm = _lm(seed=7)
    B, P, N = 3, 9, 12
    tok = _tok(B, P).cuda()
    for extra in (dict(min_p=0.1), dict(SHAPE, min_p=0.05, logit_bias={3: 2.0, 400: -INF, 77: -1.0}), dict(SHAPE)):
        kw = dict(SAMPLE, **extra)
        got, logits = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, **kw)
        _replay(got, logits, kw, [P] * B)
        assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, **kw), got)
    plain = lm.generate(tok, N, pad_token_id=PAD, **SAMPLE)
    tight = lm.generate(tok, N, pad_token_id=PAD, **dict(SAMPLE, min_p=0.9))
    assert not torch.equal(plain, tight)                                    # (min-p is a real filter)


def test_min_p_is_ignored_under_greedy():
    lm = _lm()
    tok = _tok(3, 9).cuda()
    assert torch.equal(lm.generate(tok, 8, min_p=0.9), lm.generate(tok, 8))


def test_a_ban_a_boost_and_a_large_frequency_penalty():
    lm = _lm()
    B, P, N = 3, 9, 12
    tok = _tok(B, P).cuda()
    free = lm.generate(tok, N).cpu()
    target = int(free[0, 0])
    for kw in (dict(), SAMPLE):
        banned = lm.generate(tok, N, logit_bias={target: -INF}, **kw)
        assert target not in banned.cpu().reshape(-1).tolist()
    boosted = lm.generate(tok, N, logit_bias={123: 1e4})
    assert bool((boosted == 123).all())                                     # greedy emits the boosted id every step
    per_row = lm.generate(tok, N, logit_bias=[{123: 1e4}, {}, {45: 1e4}]).cpu()
    assert bool((per_row[0] == 123).all()) and bool((per_row[2] == 45).all()) and torch.equal(per_row[1], free[1])
    distinct = lm.generate(tok, N, frequency_penalty=1e4).cpu()
    for b in range(B):
        assert len(set(distinct[b].tolist())) == N                          # no id twice while n < V
    again = lm.generate(tok, N, frequency_penalty=-1e4).cpu()
    assert bool((again == again[:, :1]).all())                              # a negative penalty repeats the first token for ever


def test_ragged_rows_equal_the_rows_run_alone():
    lm = _lm()
    B, N = 3, 10
    tok = _tok(B, 9).cuda()
    lens = [4, 9, 6]
    bias = [{5: 2.0, 300: -INF}, {9: -1.0}, {}]
    for kw in (dict(SHAPE), dict(SAMPLE, **SHAPE, min_p=0.1)):
        got, logits = lm.generate(tok, N, prompt_lengths=lens, logit_bias=bias, output_logits=True, pad_token_id=PAD, **kw)
        _replay(got, logits, dict(kw, logit_bias=bias), lens)
        for b, L in enumerate(lens):
            alone = lm.generate(tok[b:b + 1, :L].contiguous(), N, logit_bias=bias[b], pad_token_id=PAD, sequence_ids=torch.tensor([b]), **kw)
            assert torch.equal(alone[0], got[b]), (b, kw)


def test_parallel_samples_equal_the_prompt_repeated():
    lm = _lm(seed=7)
    B, N, n = 2, 8, 3
    tok = _tok(B, 9).cuda()
    bias = [{11: 3.0, 12: -INF}, {400: 4.0}]
    kw = dict(SAMPLE, **SHAPE, min_p=0.05)
    got, logits = lm.generate(tok, N, num_return_sequences=n, logit_bias=bias, output_logits=True, pad_token_id=PAD, **kw)
    rep = lm.generate(tok.repeat_interleave(n, dim=0), N, logit_bias=[bias[b] for b in range(B) for _ in range(n)], pad_token_id=PAD, **kw)
    assert got.shape == (B * n, N) and torch.equal(got, rep)
    _replay(got, logits, dict(kw, logit_bias=[bias[b] for b in range(B) for _ in range(n)]), [9] * (B * n))
    assert len({tuple(r) for r in got[:n].tolist()}) > 1                    # the samples of a prompt differ: each has its own counts
    assert 12 not in got[:n].cpu().reshape(-1).tolist()
    shared = lm.generate(tok, N, num_return_sequences=n, logit_bias={400: 4.0}, pad_token_id=PAD, **kw)
    assert torch.equal(shared[n:], got[n:])                                 # one dict for every row = prompt 1's own dict here


def test_a_session_turn_starts_from_zero_counts():
    lm = _lm()
    B, P, N1, N2 = 3, 9, 8, 8
    tok = _tok(B, P)
    kw = dict(frequency_penalty=2.0, presence_penalty=1.0, logit_bias={9: 1.5})
    out1, logits1, session = lm.generate(tok.cuda(), N1, output_logits=True, pad_token_id=PAD, return_session=True, **kw)
    _replay(out1, logits1, kw, [P] * B)
    assert torch.equal(out1, lm.generate(tok.cuda(), N1, pad_token_id=PAD, **kw))
    x2 = _tok(B, 3, seed=9)
    out2, logits2 = session.generate(x2.cuda(), N2, output_logits=True, pad_token_id=PAD, **kw)
    _replay(out2, logits2, kw, [P + N1 + 3] * B)                            # the reference starts the turn with zero counts too
    cat = torch.cat([tok, out1.cpu(), x2], dim=1)
    fresh = lm.generate(cat.cuda(), N2, prompt_lengths=[cat.shape[1]] * B, pad_token_id=PAD, **kw)   # the prompt does not count either
    assert torch.equal(out2, fresh)
    out3, logits3 = session.generate(x2.cuda(), 4, output_logits=True, pad_token_id=PAD, **dict(SAMPLE, min_p=0.2, **SHAPE))
    _replay(out3, logits3, dict(SAMPLE, min_p=0.2, **SHAPE), [P + N1 + 3 + N2 + 3] * B)


def test_kosmos_with_an_image():
    m = Kosmos._from_config(tiny_config(), seed=1, perturb=0.1).eval().to("cuda")
    m.precision = "fp32"
    g = torch.Generator().manual_seed(5)
    B, Tt, N = 2, 10, 12
    vocab = m.cfg.vocab
    tok = torch.randint(0, vocab, (B, Tt), generator=g).cuda()
    img = torch.randn(B, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    free = m.generate(tok, img, N).cpu()
    bias = [{int(free[0, 0]): -INF, vocab - 1: 2.0}, {0: 1.0}]
    T0 = Tt + m.cfg.perceiver.latents
    for kw in (dict(SHAPE, logit_bias=bias), dict(SAMPLE, min_p=0.1, top_k=min(50, vocab - 1), **SHAPE, logit_bias=bias)):
        got, logits = m.generate(tok, img, N, output_logits=True, pad_token_id=PAD, **kw)
        _replay(got, logits, kw, [T0] * B)
        assert int(free[0, 0]) not in got[0].tolist()
        assert torch.equal(m.generate(tok, img, N, pad_token_id=PAD, **kw), got)


def test_logprobs_are_still_those_of_the_models_own_distribution():
    """``output_logprobs`` reports score()'s arithmetic (kx_token_logprob) on the raw rows, whatever the shaping did to the row the
    sampler read; without ``output_logits`` the raw row is the clone taken before the launch."""
    lm = _lm()
    B, P, N, k = 3, 9, 8, 4
    tok = _tok(B, P).cuda()
    for kw in (dict(SHAPE, logit_bias={7: 5.0, 20: -INF}), dict(SAMPLE, min_p=0.1, **SHAPE)):
        tokens, logits, lp, tl, ti = lm.generate(tok, N, output_logits=True, output_logprobs=True, top_logprobs=k, pad_token_id=PAD, **kw)
        _replay(tokens, logits, kw, [P] * B)
        flat = logits.reshape(B * N, V)
        want = ops.token_logprob(flat, tokens.reshape(B * N).contiguous()).view(B, N)
        assert torch.equal(lp, want) and bool((lp < 0).all())
        plain = lm.generate(tok, N, output_logits=True)[1]
        assert torch.equal(logits[:, 0].view(torch.int32), plain[:, 0].view(torch.int32))      # step 0's raw row is the unshaped one
        idx = torch.arange(B * N, dtype=torch.int32, device="cuda").repeat_interleave(k)
        same = ops.token_logprob(flat, ti.reshape(B * N * k).contiguous(), row_index=idx).view(B, N, k)
        assert torch.equal(tl, same)
        lean = lm.generate(tok, N, output_logprobs=True, top_logprobs=k, pad_token_id=PAD, **kw)
        assert torch.equal(lean[0], tokens) and torch.equal(lean[1], lp) and torch.equal(lean[2], tl) and torch.equal(lean[3], ti)


def test_with_the_defaults_nothing_is_launched(monkeypatch):
    lm = _lm()
    tok = _tok(3, 9).cuda()
    calls = [lambda **kw: lm.generate(tok, 6, **kw), lambda **kw: lm.generate(tok, 6, prompt_lengths=[4, 9, 6], **SAMPLE, **kw),
             lambda **kw: lm.generate(tok, 6, num_return_sequences=2, **SAMPLE, **kw)]
    before = [c() for c in calls]
    real, names = ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)

    def boom(*a, **k):
        raise AssertionError("kx_shape_logits launched with the keywords at their defaults")
    monkeypatch.setattr(ops, "shape_logits", boom)
    monkeypatch.setattr(ops.H, "load", lambda: Spy())
    for call, out in zip(calls, before):
        assert torch.equal(call(logit_bias=None, presence_penalty=0.0, frequency_penalty=0.0, min_p=0.0), out)
        assert torch.equal(call(logit_bias={}), out)
    assert "kx_sample_logits" in names and "kx_sample_logits_ragged" in names
    assert "kx_sample_logits_min_p" not in names and "kx_shape_logits" not in names
    lm.generate(tok, 4, min_p=0.3, **SAMPLE)                                # min_p alone: the new sampler entry point, no shaping launch
    assert "kx_sample_logits_min_p" in names
    with pytest.raises(AssertionError, match="launched"):
        lm.generate(tok, 4, presence_penalty=0.5)
