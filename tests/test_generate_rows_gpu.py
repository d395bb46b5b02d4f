"""generate(row_options=) end to end on the device, on the tiny LM of tests/test_generate_truncate_gpu.py.

``output_logits`` returns the model's own logits of every step; every emitted token is replayed by running the SCALAR device sampler
(ops.sample_logits without ``rows``: the entry points tests/test_sample_logits_gpu.py and tests/test_sample_truncate_gpu.py pin to the
float64 references) on the returned ``logits[b, g]`` alone, with row b's resolved scalars, position len_b + g, sequence id b and the
row's own history.  The replay is exact: no tolerance, no allowed share.  Behind a row's budget every token is the pad."""
import numpy as np
import pytest
import torch

import guidance_ref as GR
from kosmosx import generation as G
from kosmosx import ops
from kosmosx.model import KosmosLanguage

pytestmark = pytest.mark.gpu

V = 502
PAD = 1
CALL = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=21)
# four unlike requests: a greedy one, filters of its own, its own seed and a budget, a repetition penalty
ROWS = [dict(do_sample=False), dict(temperature=1.1, typical_p=0.9, min_p=0.02), dict(seed=77, max_new_tokens=4, top_k=0, epsilon_cutoff=2e-3),
        dict(repetition_penalty=1.3, eta_cutoff=0.02, top_p=1.0)]
NEW = ("kx_sample_rows_pack", "kx_sample_logits_rows", "kx_shape_logits_rows")
OLD_SAMPLERS = ("kx_sample_logits", "kx_sample_logits_ragged", "kx_sample_logits_min_p", "kx_sample_logits_truncate")
SAMPLER_KEYS = ("do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "seed")


@pytest.fixture(scope="module")
def lm():
    m = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=7, _perturb=0.1, _max_positions=64).eval().to("cuda")
    m.precision = "fp32"
    return m


def _tok(B, T, seed=4):
    return torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(seed))


def _resolve(rows, N, call=CALL):
    return G.check_row_options(V, len(rows), row_options=rows, max_new_tokens=N, **call)


def _replay(tokens, logits, resolved, prompts, *, seq_ids=None):
    """Every token of every row from the returned rows ``logits`` through the scalar device sampler, one row at a time.
    ``prompts``: row b's prompt ids (what its repetition penalty sees before the first new token)."""
    tokens = tokens.cpu()
    logits = torch.as_tensor(logits).cuda()
    B, n = tokens.shape
    for b in range(B):
        r = resolved[b]
        budget = r["max_new_tokens"] or n
        for g in range(n):
            if g >= budget:
                assert int(tokens[b, g]) == PAD, (b, g)
                continue
            hist = torch.cat([prompts[b].cpu().long(), tokens[b, :g], torch.zeros(1, dtype=torch.int64)])[None].cuda()
            want = ops.sample_logits(logits[b, g][None].contiguous(), position=len(prompts[b]) + g, history=hist, hist_len=hist.shape[1] - 1,
                                     sequence_ids=torch.tensor([b if seq_ids is None else seq_ids[b]], device="cuda"), pad_token_id=PAD,
                                     **{k: r[k] for k in SAMPLER_KEYS})
            assert int(want[0]) == int(tokens[b, g]), (b, g, int(want[0]), int(tokens[b, g]))


def test_plain_and_ragged_tokens_replay_and_repeat(lm):
    B, P, N = 4, 9, 10
    tok = _tok(B, P).cuda()
    res = _resolve(ROWS, N)
    got, logits = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, row_options=ROWS, **CALL)
    assert got.shape == (B, N)
    _replay(got, logits, res, [tok[b] for b in range(B)])
    assert torch.equal(got[2, 4:].cpu(), torch.full((N - 4,), PAD))
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, row_options=ROWS, **CALL), got)     # repeatable, with or without the logits kept
    assert not torch.equal(got, lm.generate(tok, N, pad_token_id=PAD, **CALL))                   # the options are real
    lens = [4, 9, 6, 7]
    rag, rlogits = lm.generate(tok, N, prompt_lengths=lens, output_logits=True, pad_token_id=PAD, row_options=ROWS, **CALL)
    _replay(rag, rlogits, res, [tok[b, :L] for b, L in enumerate(lens)])
    assert torch.equal(lm.generate(tok, N, prompt_lengths=lens, pad_token_id=PAD, row_options=ROWS, **CALL), rag)
    for b, L in enumerate(lens):                                                                 # a row of the mixed batch is the row run alone
        kw = {k: res[b][k] for k in SAMPLER_KEYS}
        m = res[b]["max_new_tokens"] or N
        alone = lm.generate(tok[b:b + 1, :L].contiguous(), N, pad_token_id=PAD, sequence_ids=torch.tensor([b]), **kw)
        assert torch.equal(alone[0, :m], rag[b, :m]) and (rag[b, m:] == PAD).all(), b
    # a sequence that resolves every row to the call's own scalars gives the call's tokens
    same = [dict(temperature=0.8), dict(seed=21), dict(top_k=50, top_p=0.9), dict(do_sample=True)]
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, row_options=same, **CALL), lm.generate(tok, N, pad_token_id=PAD, **CALL))


def test_presence_and_frequency_per_row_equal_the_one_row_calls(lm):
    """On the ragged path, whose rows generate what they would generate alone (tests/test_generate_truncate_gpu.py checks it that way)."""
    B, P, N = 3, 9, 10
    tok = _tok(B, P).cuda()
    rows = [dict(presence_penalty=1.5, frequency_penalty=0.5, temperature=1.3), dict(), dict(frequency_penalty=-2.0, do_sample=False)]
    res = _resolve(rows, N)
    got = lm.generate(tok, N, pad_token_id=PAD, row_options=rows, **CALL)
    lens = [5, 9, 7]
    rag = lm.generate(tok, N, pad_token_id=PAD, prompt_lengths=lens, row_options=rows, **CALL)
    for b in range(B):
        kw = {k: res[b][k] for k in SAMPLER_KEYS + ("presence_penalty", "frequency_penalty")}
        alone = lm.generate(tok[b:b + 1, :lens[b]].contiguous(), N, pad_token_id=PAD, sequence_ids=torch.tensor([b]), **kw)
        assert torch.equal(rag[b], alone[0]), b
    assert not torch.equal(got[2], lm.generate(tok, N, pad_token_id=PAD, row_options=[{}, {}, dict(do_sample=False)], **CALL)[2])
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, row_options=rows, **CALL), got)


def test_budgets_stop_the_loop_and_keep_the_logprob_slots_behind_them_empty(lm):
    B, P, N = 3, 9, 8
    tok = _tok(B, P).cuda()
    early = lm.generate(tok, N, pad_token_id=PAD, eos_poll=2, row_options=[dict(max_new_tokens=2), dict(max_new_tokens=1), dict(max_new_tokens=2)], **CALL)
    free, flp, ftop, fids = lm.generate(tok, N, pad_token_id=PAD, output_logprobs=True, top_logprobs=2, **CALL)
    assert early.shape == (B, 2) and torch.equal(early[:, 0], free[:, 0]) and early[1, 1] == PAD  # every row finished: the stop poll ended the loop
    budgets = [3, None, 1]
    rows = [{} if m is None else dict(max_new_tokens=m) for m in budgets]
    got, lp, top, ids = lm.generate(tok, N, pad_token_id=PAD, output_logprobs=True, top_logprobs=2, row_options=rows, **CALL)
    for b, m in enumerate(budgets):
        m = N if m is None else m
        assert torch.equal(got[b, :m], free[b, :m]) and (got[b, m:] == PAD).all()
        assert torch.equal(lp[b, :m], flp[b, :m]) and torch.equal(ids[b, :m], fids[b, :m]) and torch.equal(top[b, :m], ftop[b, :m])
        assert (lp[b, m:] == 0).all() and (top[b, m:] == 0).all() and (ids[b, m:] == -1).all()


def test_parallel_samples_equal_the_prompt_repeated_with_the_options_repeated(lm):
    B, N, n = 2, 8, 2
    tok = _tok(B, 9).cuda()
    rows = [dict(temperature=1.2, typical_p=0.9, seed=5, presence_penalty=0.8), dict(top_k=0, eta_cutoff=0.01, max_new_tokens=5, repetition_penalty=1.2)]
    got, logits = lm.generate(tok, N, num_return_sequences=n, output_logits=True, pad_token_id=PAD, row_options=rows, **CALL)
    assert got.shape == (B * n, N)
    rep = [rows[b] for b in range(B) for _ in range(n)]
    assert torch.equal(got, lm.generate(tok.repeat_interleave(n, dim=0), N, pad_token_id=PAD, row_options=rep, **CALL))
    assert (got[2:, 5:] == PAD).all() and not torch.equal(got[0], got[1])
    _replay(got[2:], logits[2:], _resolve(rep, N)[2:], [tok[1], tok[1]], seq_ids=[2, 3])      # (rows 0, 1 carry a presence penalty: not in the raw logits)


def test_guided_tokens_replay(lm):
    """The guided row is rebuilt as tests/test_generate_guidance_gpu.py does: the device's own log-probs of the two returned raw rows,
    combined by tests/guidance_ref.py."""
    B, P, N, s = 3, 9, 8, 1.5
    tok, neg = _tok(B, P).cuda(), _tok(B, 4, seed=11).cuda()
    rows = [ROWS[1], ROWS[2], ROWS[3]]
    got, cond, uncond = lm.generate(tok, N, output_logits=True, pad_token_id=PAD, guidance_scale=s, negative_prompt_ids=neg, row_options=rows, **CALL)

    def logprobs(r):
        Rn, Vn = r.shape
        tgt = torch.arange(Vn, dtype=torch.int64, device=r.device).repeat(Rn)
        idx = torch.arange(Rn, dtype=torch.int32, device=r.device).repeat_interleave(Vn)
        return ops.token_logprob(r, tgt, row_index=idx).view(Rn, Vn).cpu().numpy()
    guided = GR.guided_row_f32(logprobs(cond.reshape(B * N, V).contiguous()), logprobs(uncond.reshape(B * N, V).contiguous()), s)
    _replay(got, np.ascontiguousarray(guided.reshape(B, N, V)), _resolve(rows, N), [tok[b] for b in range(B)])
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, guidance_scale=s, negative_prompt_ids=neg, row_options=rows, **CALL), got)
    assert not torch.equal(got, lm.generate(tok, N, pad_token_id=PAD, guidance_scale=s, negative_prompt_ids=neg, **CALL))


def test_session_turns_take_their_own_options_and_budgets(lm):
    B, P, N1, N2 = 3, 9, 6, 6
    tok = _tok(B, P)
    rows1 = [dict(max_new_tokens=2, temperature=1.1), dict(typical_p=0.9), dict(max_new_tokens=5, seed=9)]
    out1, logits1, session = lm.generate(tok.cuda(), N1, output_logits=True, pad_token_id=PAD, return_session=True, row_options=rows1, **CALL)
    valid = [2, N1, 5]
    assert session.lengths == [P + v for v in valid]                            # n_valid[b] is the budget
    _replay(out1, logits1, _resolve(rows1, N1), [tok[b] for b in range(B)])
    assert torch.equal(out1, lm.generate(tok.cuda(), N1, pad_token_id=PAD, row_options=rows1, **CALL))
    x2 = _tok(B, 3, seed=9)
    rows2 = [dict(eta_cutoff=0.01), dict(do_sample=False, max_new_tokens=3), dict(temperature=0.6, min_p=0.05, repetition_penalty=1.2)]
    out2, logits2 = session.generate(x2.cuda(), N2, output_logits=True, pad_token_id=PAD, row_options=rows2, **CALL)
    convo = [torch.cat([tok[b], out1[b, :valid[b]].cpu(), x2[b]]) for b in range(B)]
    _replay(out2, logits2, _resolve(rows2, N2), convo)
    assert session.lengths == [len(c) + v for c, v in zip(convo, [N2, 3, N2])]
    cat = torch.nn.utils.rnn.pad_sequence(convo, batch_first=True)
    fresh = lm.generate(cat.cuda(), N2, prompt_lengths=[len(c) for c in convo], pad_token_id=PAD, row_options=rows2, **CALL)
    assert torch.equal(out2, fresh)


def test_without_options_nothing_new_is_launched_and_with_them_one_sampler_launch_per_token(lm, monkeypatch):
    tok = _tok(3, 9).cuda()
    N = 6
    calls = [lambda **kw: lm.generate(tok, N, **kw), lambda **kw: lm.generate(tok, N, prompt_lengths=[4, 9, 6], **CALL, **kw),
             lambda **kw: lm.generate(tok, N, num_return_sequences=2, **CALL, **kw),
             lambda **kw: lm.generate(tok, N, presence_penalty=0.5, min_p=0.05, eta_cutoff=1e-3, **CALL, **kw)]
    before = [c() for c in calls]
    real, names = ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ops.H, "load", lambda: Spy())
    for call, out in zip(calls, before):
        assert torch.equal(call(row_options=None), out)
        assert torch.equal(call(row_options=[{}, {}, {}]), out)
        assert torch.equal(call(row_options=({}, {}, {})), out)
    assert not set(NEW) & set(names) and "kx_sample_logits" in names and "kx_sample_logits_truncate" in names and "kx_shape_logits" in names
    del names[:]
    lm.generate(tok, N, row_options=[dict(temperature=0.5), {}, dict(repetition_penalty=1.1, max_new_tokens=2)], **CALL)
    assert names.count("kx_sample_logits_rows") == N and names.count("kx_sample_rows_pack") == 1     # one launch per token, one pack per call
    assert not set(OLD_SAMPLERS) & set(names) and "kx_shape_logits_rows" not in names and "kx_shape_logits" not in names
    del names[:]
    lm.generate(tok, N, prompt_lengths=[4, 9, 6], row_options=[dict(frequency_penalty=0.5), {}, {}], **CALL)
    assert names.count("kx_sample_logits_rows") == N and names.count("kx_shape_logits_rows") == N
    assert not set(OLD_SAMPLERS) & set(names) and "kx_shape_logits" not in names
    del names[:]
    lm.generate(tok, N, logit_bias={5: 1.0}, row_options=[dict(seed=4), {}, {}], **CALL)            # a bias alone: the old shaping entry point
    assert names.count("kx_sample_logits_rows") == N and names.count("kx_shape_logits") == N and "kx_shape_logits_rows" not in names


def test_a_budget_under_an_automaton_counts_as_tokens_and_a_dead_end_still_does_not(lm):
    """With an automaton a row the sampler launch finishes on a token other than the EOS is taken for a dead end (its pad is no token of
    the row) — except in the launch its budget names, whose token is one."""
    from kosmosx.automaton import TokenAutomaton
    B, P, N = 3, 9, 6
    tok = _tok(B, P).cuda()
    auto = TokenAutomaton.from_choices([[40, 41, 42, 43], [40, 44]])                     # 4 or 2 tokens, then nothing is allowed
    rows = [dict(max_new_tokens=1), dict(max_new_tokens=3, temperature=1.2), dict()]
    got, lp, session = lm.generate(tok, N, pad_token_id=PAD, token_automaton=auto, output_logprobs=True, return_session=True,
                                   row_options=rows, **CALL)
    free, flp = lm.generate(tok, N, pad_token_id=PAD, token_automaton=auto, output_logprobs=True, row_options=[{}, dict(temperature=1.2), {}], **CALL)
    said = [int((free[b] != PAD).sum()) for b in range(B)]                              # the choice row b took: 2 or 4 tokens
    assert set(said) <= {2, 4}
    valid = [1, min(3, said[1]), said[2]]
    assert session.lengths == [P + v for v in valid]
    for b, v in enumerate(valid):
        assert torch.equal(got[b, :v], free[b, :v]) and (got[b, v:] == PAD).all()
        assert torch.equal(lp[b, :v], flp[b, :v]) and (lp[b, :v] < 0).all() and (lp[b, v:] == 0).all()


def test_a_dead_end_in_the_budgets_own_column_is_still_no_token(lm):
    """The automaton allows exactly m - 1 tokens and the budget is m: the launch of column m - 1 has no candidate AND spends the
    budget.  What it emits is a pad — not a token of the row, for the session's lengths and for the log-prob slots alike."""
    from kosmosx.automaton import TokenAutomaton
    B, P, N = 3, 9, 6
    tok = _tok(B, P).cuda()
    auto = TokenAutomaton.from_choices([[40, 41]])                                       # one choice: two tokens, then nothing is allowed
    rows = [dict(max_new_tokens=3), dict(max_new_tokens=2), dict(max_new_tokens=1)]      # dead end in the budget's column; budget on the last token; budget first
    got, lp, session = lm.generate(tok, N, pad_token_id=PAD, token_automaton=auto, output_logprobs=True, return_session=True,
                                   row_options=rows, **CALL)
    valid = [2, 2, 1]
    assert session.lengths == [P + v for v in valid]
    for b, v in enumerate(valid):
        assert got[b, :v].tolist() == [40, 41][:v] and (got[b, v:] == PAD).all()
        assert (lp[b, :v] < 0).all() and (lp[b, v:] == 0).all()
    # the next turn reads the conversation without the pad
    x2 = _tok(B, 2, seed=9)
    out2 = session.generate(x2.cuda(), 3, pad_token_id=PAD, **CALL)
    convo = [torch.cat([tok[b].cpu(), got[b, :valid[b]].cpu(), x2[b]]) for b in range(B)]
    cat = torch.nn.utils.rnn.pad_sequence(convo, batch_first=True)
    assert torch.equal(out2, lm.generate(cat.cuda(), 3, prompt_lengths=[len(c) for c in convo], pad_token_id=PAD, **CALL))


def test_a_call_level_penalty_that_rows_override_is_the_rows_own(lm, monkeypatch):
    """The call's presence / frequency penalty is what a row inherits, not what every row gets: rows that override it to 0 are
    shaped by nothing, also when ALL of them do (then no shaping launch runs), also at B = 1."""
    B, P, N = 3, 9, 8
    tok = _tok(B, P).cuda()
    lens = [5, 9, 7]
    # (negative penalties favour what was emitted: the shaped call repeats itself, so the penalty certainly shows)
    for pen in (dict(presence_penalty=-4.0), dict(frequency_penalty=-3.0), dict(presence_penalty=2.0, frequency_penalty=-4.0)):
        off = {k: 0.0 for k in pen}
        plain = lm.generate(tok, N, pad_token_id=PAD, prompt_lengths=lens, **CALL)
        shaped = lm.generate(tok, N, pad_token_id=PAD, prompt_lengths=lens, **CALL, **pen)
        assert not torch.equal(plain, shaped)                                            # the penalty is real
        assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, prompt_lengths=lens, row_options=[off] * B, **CALL, **pen), plain)
        assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, row_options=[off] * B, **CALL, **pen), lm.generate(tok, N, pad_token_id=PAD, **CALL))
        one = lm.generate(tok[:1], N, pad_token_id=PAD, row_options=[off], **CALL, **pen)
        assert torch.equal(one, lm.generate(tok[:1], N, pad_token_id=PAD, **CALL))
        mixed = lm.generate(tok, N, pad_token_id=PAD, prompt_lengths=lens, row_options=[off, {}, dict(seed=3)], **CALL, **pen)
        assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[1], shaped[1])     # row 0 opted out, row 1 inherits
        alone = lm.generate(tok[2:3, :lens[2]].contiguous(), N, pad_token_id=PAD, sequence_ids=torch.tensor([2]), **dict(CALL, seed=3), **pen)
        assert torch.equal(mixed[2], alone[0])
    # with a bias in the call the launch still runs, with zero penalties
    bias = {7: 4.0, 9: -3.0}
    assert torch.equal(lm.generate(tok, N, pad_token_id=PAD, logit_bias=bias, presence_penalty=1.5, row_options=[dict(presence_penalty=0)] * B, **CALL),
                       lm.generate(tok, N, pad_token_id=PAD, logit_bias=bias, **CALL))
    real, names = ops.H.load(), []

    class Spy:
        def __getattr__(self, name):
            names.append(name)
            return getattr(real, name)
    monkeypatch.setattr(ops.H, "load", lambda: Spy())
    lm.generate(tok, N, pad_token_id=PAD, presence_penalty=1.5, row_options=[dict(presence_penalty=0.0)] * B, **CALL)
    assert "kx_shape_logits" not in names and "kx_shape_logits_rows" not in names and names.count("kx_sample_logits_rows") == N
