"""generate(token_automaton=...): token-automaton constrained decoding end to end on the device.

The scheme of tests/test_generate_constrain_gpu.py: ``output_logits`` returns the model's own logits of every step; the NumPy
restatement of kx_automaton_step (tests/automaton_ref.py, from the raw tables) and then of the sampler (tests/sampling_ref.py) are
applied to THOSE logits with the state walked so far, and must reproduce the emitted token exactly.  No tolerance is involved."""
import numpy as np
import pytest
import torch

import automaton_ref as AR
import beam_ref as BR
import constrain_ref as CR
import logprob_ref as LR
import sampling_ref as R
from helpers import tiny_config
from kosmosx import _hip as H
from kosmosx import ops
from kosmosx.automaton import TokenAutomaton
from kosmosx.model import Kosmos, KosmosLanguage
from test_generate_beam_gpu import _replay as _beam_replay

pytestmark = pytest.mark.gpu

V = 502
PAD = 1
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=21)
# three choices of 2-5 ids, two of them sharing a prefix; no id is the pad
CHOICES = [[17, 230, 41], [17, 230, 99, 301, 7], [404, 12]]
FREE = TokenAutomaton([{}], default=[0])                    # one state that allows everything: nothing is stored


def _lm(seed=5):
    lm = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=seed, _perturb=0.1,
                        _max_positions=64).eval().to("cuda")
    lm.precision = "fp32"
    return lm


def _tok(B, T, seed=4, vocab=V):
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(seed))


def _replay(tokens, logits, tables, starts, kw, positions, *, seq_ids=None, cons=None, prompts=None, eos=None):
    """Every token of every row: the automaton reference (and constrain_ref, with ``cons``) then the sampler reference, on the
    returned logits.  Tokens must match exactly.  Returns per row (the valid tokens, the final state, whether it ended with nothing
    allowed)."""
    tokens, logits = tokens.cpu().numpy(), logits.cpu().numpy()
    B, n = tokens.shape
    rows = []
    for b in range(B):
        s, finished, stuck, valid = starts[b], False, False, []
        for g in range(n):
            s, ban = AR.step_row(tables, s, None if g == 0 else int(tokens[b, g - 1]), finished, logits.shape[2])
            if cons is not None and not finished:
                hist = np.concatenate([prompts[b], tokens[b, :g]])
                cban, fin = CR.constrain_row(hist, logits[b, g], new_tokens=g, bad_words=cons.get("bad_words_ids") or (),
                                             min_new=cons.get("min_new_tokens", 0), eos_id=eos, finished=False)
                assert not fin
                ban = ban | cban
            if finished:
                assert int(tokens[b, g]) == PAD, (b, g)
                continue
            ref = R.sample_row(AR.apply(logits[b, g], ban), temperature=kw.get("temperature", 1.0), top_k=kw.get("top_k", 0),
                               top_p=kw.get("top_p", 1.0), do_sample=kw.get("do_sample", False), seed=kw.get("seed", 0),
                               position=positions[b] + g, sequence_id=b if seq_ids is None else seq_ids[b], pad_token_id=PAD)
            assert int(tokens[b, g]) == ref["token"], (b, g, int(tokens[b, g]), ref["token"])
            assert ref["none"] == bool(ban.all())
            if ref["none"]:
                finished = stuck = True
            else:
                assert not ban[ref["token"]]
                valid.append(ref["token"])
                finished = eos is not None and ref["token"] == eos
        rows.append((valid, s, stuck))
    return rows


def test_greedy_choices_end_rows_without_an_eos_and_the_poll_ends_the_loop():
    lm = _lm()
    B, P, N = 3, 9, 16
    tok = _tok(B, P).cuda()
    auto = TokenAutomaton.from_choices(CHOICES)
    free = lm.generate(tok, N).cpu()
    for b in range(B):                                                      # left alone the model says something else
        assert not any(free[b, :len(c)].tolist() == c for c in CHOICES), free[b]
    got, logits = lm.generate(tok, N, token_automaton=auto, output_logits=True, pad_token_id=PAD, eos_poll=2)
    n = got.shape[1]
    assert n < N and n <= 6 + 2 and logits.shape == (B, n, V)               # the longest choice ends at step 5: no EOS, no stop sequence
    assert bool(torch.isfinite(logits).all())                               # the model's own logits: no -inf from the mask
    rows = _replay(got, logits, auto.tables(), [auto.start] * B, {}, [P] * B)
    for b, (valid, s, stuck) in enumerate(rows):
        assert valid in CHOICES and stuck, (b, valid)                       # exactly one choice, then pads
        assert got[b, len(valid):].tolist() == [PAD] * (n - len(valid))
    assert torch.equal(lm.generate(tok, N, token_automaton=auto, pad_token_id=PAD, eos_poll=2), got)
    full = lm.generate(tok, N, token_automaton=auto, pad_token_id=PAD, eos_poll=0)   # no poll: the rows are padded to the end
    assert full.shape == (B, N) and torch.equal(full[:, :n], got) and bool((full[:, n:] == PAD).all())


def test_sampled_tokens_replay_exactly_and_repeat():
    lm = _lm(seed=7)
    B, P, N = 3, 9, 12
    tok = _tok(B, P).cuda()
    ids = sorted(int(t) for t in np.random.default_rng(0).choice(V, 16, replace=False))
    for auto in (TokenAutomaton.from_allowed(ids), TokenAutomaton.from_choices(CHOICES + [[404, 13, 5]])):
        got, logits = lm.generate(tok, N, token_automaton=auto, output_logits=True, pad_token_id=PAD, eos_poll=0, **SAMPLE)
        rows = _replay(got, logits, auto.tables(), [auto.start] * B, SAMPLE, [P] * B)
        assert torch.equal(lm.generate(tok, N, token_automaton=auto, pad_token_id=PAD, eos_poll=0, **SAMPLE), got)
        if auto.num_states == 1:
            assert all(len(valid) == N and set(valid) <= set(ids) for valid, _, _ in rows)
            other = lm.generate(tok, N, token_automaton=auto, pad_token_id=PAD, eos_poll=0, **dict(SAMPLE, seed=22))
            assert not torch.equal(other, got)                              # (the seed matters: the draws are real)
        else:
            assert all(stuck for _, _, stuck in rows)


def test_an_automaton_that_allows_everything_changes_nothing():
    lm = _lm()
    tok = _tok(3, 9).cuda()
    for kw in (dict(), SAMPLE, dict(SAMPLE, prompt_lengths=[4, 9, 6])):
        off = lm.generate(tok, 10, output_logits=True, **kw)
        on = lm.generate(tok, 10, output_logits=True, token_automaton=FREE, **kw)
        assert torch.equal(on[0], off[0]) and torch.equal(on[1].view(torch.int32), off[1].view(torch.int32))


def test_ragged_rows_with_their_own_grammars_equal_the_rows_run_alone():
    lm = _lm()
    B, N = 3, 10
    tok = _tok(B, 9).cuda()
    lens = [4, 9, 6]
    a0 = TokenAutomaton.from_choices(CHOICES)
    a1 = TokenAutomaton.from_allowed([3, 77, 78, 250, 499])
    u, starts = TokenAutomaton.union([a0, a1])
    mine = [starts[0], starts[1], starts[0]]
    for kw in (dict(), SAMPLE):
        got, logits = lm.generate(tok, N, prompt_lengths=lens, token_automaton=u, automaton_start=mine, pad_token_id=PAD, eos_poll=0,
                                  output_logits=True, **kw)
        rows = _replay(got, logits, u.tables(), mine, kw, lens)
        assert rows[0][0] in CHOICES and rows[2][0] in CHOICES and set(rows[1][0]) <= {3, 77, 78, 250, 499} and len(rows[1][0]) == N
        for b, L in enumerate(lens):
            alone = lm.generate(tok[b:b + 1, :L].contiguous(), N, token_automaton=(a0, a1, a0)[b], pad_token_id=PAD, eos_poll=0,
                                sequence_ids=torch.tensor([b]), **kw)
            assert torch.equal(alone[0], got[b]), (b, kw)
        as_tensor = lm.generate(tok, N, prompt_lengths=lens, token_automaton=u, automaton_start=torch.tensor(mine), pad_token_id=PAD,
                                eos_poll=0, **kw)
        assert torch.equal(as_tensor, got)


def test_parallel_samples_equal_the_prompt_repeated():
    lm = _lm(seed=7)
    B, N, n = 2, 8, 3
    tok = _tok(B, 9).cuda()
    u, starts = TokenAutomaton.union([TokenAutomaton.from_allowed(range(40, 60)), TokenAutomaton.from_choices(CHOICES)])
    got, logits = lm.generate(tok, N, num_return_sequences=n, token_automaton=u, automaton_start=starts, pad_token_id=PAD, eos_poll=0,
                              output_logits=True, **SAMPLE)
    rep = lm.generate(tok.repeat_interleave(n, dim=0), N, token_automaton=u, automaton_start=[s for s in starts for _ in range(n)],
                      pad_token_id=PAD, eos_poll=0, **SAMPLE)
    assert got.shape == (B * n, N) and torch.equal(got, rep)
    rows = _replay(got, logits, u.tables(), [s for s in starts for _ in range(n)], SAMPLE, [9] * (B * n))
    assert all(set(v) <= set(range(40, 60)) and len(v) == N for v, _, _ in rows[:n]) and all(v in CHOICES for v, _, _ in rows[n:])
    assert len({tuple(v) for v, _, _ in rows[:n]}) > 1                      # the samples of a prompt differ


def test_kosmos_with_an_image_follows_the_choices():
    m = Kosmos._from_config(tiny_config(), seed=1, perturb=0.1).eval().to("cuda")
    m.precision = "fp32"
    g = torch.Generator().manual_seed(5)
    B, Tt, N = 2, 10, 12
    vocab = m.cfg.vocab
    tok = torch.randint(0, vocab, (B, Tt), generator=g).cuda()
    img = torch.randn(B, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    choices = [[c % vocab for c in ch] for ch in CHOICES]
    assert len({tuple(c) for c in choices}) == 3 and all(PAD not in c for c in choices)
    auto = TokenAutomaton.from_choices(choices)
    free = m.generate(tok, img, N).cpu()
    for b in range(B):
        assert not any(free[b, :len(c)].tolist() == c for c in choices)
    got, logits = m.generate(tok, img, N, token_automaton=auto, output_logits=True, pad_token_id=PAD, eos_poll=2)
    n = got.shape[1]
    assert n < N
    rows = _replay(got, logits, auto.tables(), [auto.start] * B, {}, [Tt + m.cfg.perceiver.latents] * B)
    for b, (valid, s, stuck) in enumerate(rows):
        assert valid in choices and stuck and got[b, len(valid):].tolist() == [PAD] * (n - len(valid))


def test_logprobs_are_those_of_the_returned_logits():
    lm = _lm()
    B, P, N, k = 3, 9, 8, 4
    tok = _tok(B, P).cuda()
    auto = TokenAutomaton.from_choices(CHOICES)
    for kw in (dict(), SAMPLE):
        tokens, logits, lp, tl, ti = lm.generate(tok, N, token_automaton=auto, output_logits=True, output_logprobs=True, top_logprobs=k,
                                                 pad_token_id=PAD, eos_poll=0, **kw)
        rows = _replay(tokens, logits, auto.tables(), [auto.start] * B, kw, [P] * B)
        live = torch.zeros((B, N), dtype=torch.bool)
        for b, (valid, _, _) in enumerate(rows):
            live[b, :len(valid)] = True                                     # the pad of the step with nothing allowed is no token
        live = live.cuda()
        flat = logits.reshape(B * N, V)
        want = ops.token_logprob(flat, tokens.reshape(B * N).contiguous()).view(B, N)
        assert torch.equal(lp[live], want[live]) and bool((lp[~live] == 0.0).all()) and bool((lp[live] < 0).all())
        ref = torch.stack([LR.top_ref(r, k)[0] for r in flat.cpu()]).view(B, N, k).cuda()
        assert torch.equal(ti[live], ref[live]) and bool((ti[~live] == -1).all()) and bool((tl[~live] == 0.0).all())
        idx = torch.arange(B * N, dtype=torch.int32, device="cuda").repeat_interleave(k)
        same = ops.token_logprob(flat, ti.reshape(B * N * k).clamp(min=0).contiguous(), row_index=idx).view(B, N, k)
        assert torch.equal(tl[live], same[live])
        # the alternatives are the model's own: at step 0 the arg max of the free run is listed though the automaton bans it
        assert bool((ti[:, 0, 0] != tokens[:, 0]).any())
        lean = lm.generate(tok, N, token_automaton=auto, output_logprobs=True, top_logprobs=k, pad_token_id=PAD, eos_poll=0, **kw)
        assert torch.equal(lean[0], tokens) and torch.equal(lean[1], lp) and torch.equal(lean[2], tl) and torch.equal(lean[3], ti)


def test_the_bans_add_up_with_the_other_constraints():
    lm = _lm()
    B, P, N, eos = 3, 9, 10, 2
    tok = _tok(B, P)
    auto = TokenAutomaton.from_choices(CHOICES, eos_token_id=eos)
    alone = lm.generate(tok.cuda(), N, token_automaton=auto, eos_token_id=eos, pad_token_id=PAD, eos_poll=0).cpu()
    first = int(alone[0, 0])                                                # ban what row 0 begins with: it must take the other branch
    cons = dict(bad_words_ids=[[first]], min_new_tokens=4)
    got, logits = lm.generate(tok.cuda(), N, token_automaton=auto, eos_token_id=eos, pad_token_id=PAD, eos_poll=0, output_logits=True,
                              **cons)
    rows = _replay(got, logits, auto.tables(), [auto.start] * B, {}, [P] * B, cons=cons, prompts=tok.numpy(), eos=eos)
    other = [c for c in CHOICES if c[0] != first]
    for b, (valid, s, stuck) in enumerate(rows):
        assert valid[0] != first and (valid[:-1] if valid[-1] == eos else valid) in other
        # a choice shorter than min_new_tokens cannot take its EOS: nothing is allowed, the row is padded and finished
        assert stuck == (len(valid) < 4) and (stuck or valid[-1] == eos)
        assert got[b, len(valid):].tolist() == [PAD] * (N - len(valid))
    # an automaton and a bad word that leave nothing at step 0
    stuck0 = lm.generate(tok.cuda(), 4, token_automaton=TokenAutomaton.from_allowed([first]), bad_words_ids=[[first]], pad_token_id=PAD,
                         eos_poll=0)
    assert bool((stuck0 == PAD).all())


def test_a_session_turn_with_its_own_automaton_equals_a_fresh_constrained_call():
    lm = _lm()
    B, P, N1, N2 = 3, 9, 8, 8
    tok = _tok(B, P)
    a1 = TokenAutomaton.from_choices(CHOICES)
    a2 = TokenAutomaton.from_choices([[55, 56, 57], [58, 59], [55, 60]])
    out1, session = lm.generate(tok.cuda(), N1, token_automaton=a1, pad_token_id=PAD, eos_poll=0, return_session=True)
    assert torch.equal(out1, lm.generate(tok.cuda(), N1, token_automaton=a1, pad_token_id=PAD, eos_poll=0))
    said = []
    for b in range(B):
        row = out1[b].tolist()
        said.append(next(c for c in CHOICES if row[:len(c)] == c))
        assert row[len(said[b]):] == [PAD] * (N1 - len(said[b]))
    assert session.lengths == [P + len(c) for c in said]                    # the pad of the step with nothing allowed is no token
    x2 = _tok(B, 3, seed=9)
    out2 = session.generate(x2.cuda(), N2, token_automaton=a2, pad_token_id=PAD, eos_poll=0)
    lens = [P + len(c) + 3 for c in said]
    cat = torch.full((B, max(lens)), 0, dtype=torch.int64)
    for b in range(B):
        cat[b, :lens[b]] = torch.cat([tok[b], torch.tensor(said[b]), x2[b]])
    fresh, logits = lm.generate(cat.cuda(), N2, prompt_lengths=lens, token_automaton=a2, pad_token_id=PAD, eos_poll=0, output_logits=True)
    assert torch.equal(out2, fresh)
    rows = _replay(fresh, logits, a2.tables(), [a2.start] * B, {}, lens)
    assert all(valid in ([55, 56, 57], [58, 59], [55, 60]) and stuck for valid, _, stuck in rows)


def test_beam_search_returns_exactly_the_choices():
    lm = _lm(seed=7)
    B, P, N, e = 2, 9, 8, 2
    W = R_ = len(CHOICES)
    tok = _tok(B, P).cuda()
    auto = TokenAutomaton.from_choices(CHOICES, eos_token_id=e)
    tables = auto.tables()
    seqs, scores, tr = lm.generate(tok, N, num_beams=W, num_return_sequences=R_, token_automaton=auto, eos_token_id=e, pad_token_id=PAD,
                                   output_scores=True, output_trace=True, eos_poll=0)
    assert seqs.shape == (B, R_, N)
    t = _beam_replay(tr, seqs, scores, B=B, W=W, R=R_, eos=e)               # token, parent and score of every step against beam_ref
    print(f"beam replay under an automaton: {t.counted} of {t.cases} cases inside the margin")
    lg, parent, token = tr["logits"].cpu().numpy(), tr["parent"].cpu().numpy(), tr["token"].cpu().numpy()
    n = token.shape[0]
    states = None
    for g in range(n):                                                      # every beam's state rebuilt along the backpointers
        cur = []
        for r in range(B if g == 0 else B * W):                             # (step 0 has one input beam per batch row)
            if g == 0:
                s, ban = AR.step_row(tables, auto.start, None, False, V)
                x = lg[0, r * W]
            else:
                src = (r // W) * (1 if g == 1 else W) + int(parent[g - 1, r])           # kx_beam_step's src_row
                came = states[src] if 0 <= src < len(states) else -1
                s, ban = AR.step_row(tables, came, int(token[g - 1, r]), False, V)
                x = lg[g, r]
            cur.append(s)
            assert np.array_equal(x == -np.inf, ban), (g, r)                # -inf exactly where the reference bans
            assert bool(np.isfinite(x[~ban]).all())
        states = cur
    want = {tuple(c + [e] + [PAD] * (N - len(c) - 1)) for c in CHOICES}
    for b in range(B):
        assert {tuple(seqs[b, r].tolist()) for r in range(R_)} == want      # the hypotheses are exactly the set of choices
    assert bool(torch.isfinite(scores).all())


def test_without_an_automaton_nothing_is_launched(monkeypatch):
    lm = _lm()
    tok = _tok(3, 9).cuda()
    calls = [lambda: lm.generate(tok, 6), lambda: lm.generate(tok, 6, prompt_lengths=[4, 9, 6], **SAMPLE),
             lambda: lm.generate(tok, 6, num_return_sequences=2, **SAMPLE), lambda: lm.generate(tok, 6, num_beams=3)]

    def launches(call):
        H.prof_enable(True)
        try:
            out = call()
            torch.cuda.synchronize()
            return out, len(H.prof_collect())
        finally:
            H.prof_enable(False)
    before = [launches(c) for c in calls]
    with_auto, n_auto = launches(lambda: lm.generate(tok, 6, token_automaton=FREE))
    assert n_auto == before[0][1] + 6 and torch.equal(with_auto, before[0][0])   # one launch per token, and only with the argument

    def boom(*a, **k):
        raise AssertionError("kx_automaton_step launched without a token_automaton")
    monkeypatch.setattr(ops, "automaton_step", boom)
    for call, (out, n) in zip(calls, before):
        again, m = launches(call)
        assert torch.equal(again, out) and m == n
    with pytest.raises(AssertionError, match="launched"):
        lm.generate(tok, 4, token_automaton=FREE)
