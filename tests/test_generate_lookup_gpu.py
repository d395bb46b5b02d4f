"""generate(prompt_lookup_num_tokens=D): prompt-lookup speculative decoding (kosmosx.generation.lookup_loop) on the tiny models of
tests/test_generate_gpu.py.

Model parity and pick parity are checked separately, as there: the logits row every emitted token was picked from is returned
(``output_logits``) and compared with the CPU oracle's forward over prompt + generated tokens at the incremental path's
tolerances, and every token must be the reference sampler's greedy pick ON THAT ROW — so a logits difference inside the tolerance
cannot flip a token in the test.  Acceptance is driven deterministically through ``_draft_from``."""
import math

import pytest
import torch

import sampling_ref as SR
import spec_ref
from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=64)


def _lm(seed=5):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=64).eval()


def _picks_are_the_greedy_rule(tokens, logits, n_valid=None):
    tokens, logits = tokens.cpu().numpy(), logits.cpu().numpy()
    for b in range(tokens.shape[0]):
        for g in range(tokens.shape[1] if n_valid is None else n_valid[b]):
            assert int(tokens[b, g]) == SR.sample_row(logits[b, g], do_sample=False)["token"], (b, g)


def _acceptance_is_consistent(acc, n_rows, K):
    """Column 0 is the prefill's token; a row emits 1..K per step until its tokens are out, then 0."""
    acc = acc.cpu()
    assert acc.dtype == torch.int32 and bool((acc[:, 0] == 1).all())
    for b, n in enumerate(n_rows):
        row = acc[b].tolist()
        assert sum(row) == n, (row, n)
        live = [e for e in row if e > 0]
        assert row[:len(live)] == live and all(1 <= e <= K for e in live)


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])
def test_language_logits_against_the_oracle_and_tokens_against_the_greedy_rule(prec, tol):
    lm0 = _lm(seed=7)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    P, n, D = 9, 24, 3
    tok = torch.randint(0, 502, (3, P), generator=torch.Generator().manual_seed(4))
    got, logits, acc = lm.generate(tok.cuda(), n, prompt_lookup_num_tokens=D, output_logits=True, output_acceptance=True)
    assert got.shape == (3, n) and got.dtype == torch.int64 and logits.shape == (3, n, 502) and logits.dtype == torch.float32
    full = torch.cat([tok, got.cpu()[:, :-1]], 1)
    ref = O.kosmos_language_forward(w, full, CFG)[:, P - 1:]
    e = rel_err(logits, ref)
    print(f"lookup generate logits vs oracle ({prec}): {e:.3e}; tokens per step {n / acc.shape[1]:.2f}")
    assert e < tol
    _picks_are_the_greedy_rule(got, logits)
    _acceptance_is_consistent(acc, [n] * 3, D + 1)
    again = lm.generate(tok.cuda(), n, prompt_lookup_num_tokens=D, output_logits=True, output_acceptance=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (got, logits, acc)))              # bit for bit
    assert torch.equal(lm.generate(tok.cuda(), n, prompt_lookup_num_tokens=D), got)


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_logits_against_the_oracle_forward_over_prompt_and_generated_tokens(prec, tol, alias):
    """Both u1_inplace_alias values: under the alias a generated token carries two position rows (pos_shift in kx_step_prepare)."""
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    Tt, n, D = 10, 14, 3
    tok = torch.randint(0, m.cfg.vocab, (2, Tt), generator=g)
    tok[:, 5:] = tok[:, :5]                                    # a prompt that repeats itself: the lookup has something to find
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    n_img = m.cfg.perceiver.latents
    got, logits, acc = m.generate(tok.cuda(), img.cuda(), n, prompt_lookup_num_tokens=D, output_logits=True, output_acceptance=True)
    assert got.shape == (2, n) and logits.shape == (2, n, m.cfg.vocab)
    text = torch.cat([tok, got.cpu()[:, :-1]], 1)
    ref = O.kosmos_forward(w, text, img, cfg, oracle_switches(sw))[:, Tt + n_img - 1:]
    e = rel_err(logits, ref)
    print(f"Kosmos lookup generate logits vs oracle ({prec}, alias={alias}): {e:.3e}")
    assert e < tol
    _picks_are_the_greedy_rule(got, logits)
    _acceptance_is_consistent(acc, [n] * 2, D + 1)


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
@pytest.mark.parametrize("D", [1, 3, 7])
def test_acceptance_driven_by_draft_from(D, prec):
    """B * K = 4, 8 and 16 rows: the step's paired (<= 4 rows), wave-per-row and full-tile forms."""
    lm = _lm(seed=6).to("cuda")
    lm.precision = prec
    K = D + 1
    B = 2
    tok = torch.randint(0, 502, (B, 9), generator=torch.Generator().manual_seed(2)).cuda()
    n = 22                                                     # not a multiple of K for K = 4, 8; 1 + 21 for K = 2
    plain = lm.generate(tok, n)
    # every draft right: K tokens per step after the first
    got, logits, acc = lm.generate(tok, n, prompt_lookup_num_tokens=D, _draft_from=plain, output_acceptance=True, output_logits=True)
    _picks_are_the_greedy_rule(got, logits)
    assert torch.equal(got, plain)
    steps = 1 + math.ceil((n - 1) / K)
    assert acc.shape == (B, steps) and bool((acc.sum(1) == n).all())
    assert bool((acc[:, 1:-1] == K).all()) and bool((acc[:, -1] == n - 1 - K * (steps - 2)).all())
    # drafts corrupted at chosen output slots: a step emits exactly up to (and including the correction of) the first bad slot
    bad = plain.clone()
    slots = [[4, 5, 13], [2, 20]]
    for b, ss in enumerate(slots):
        for i in ss:
            bad[b, i] = (bad[b, i] + 1) % 502
    got2, acc2 = lm.generate(tok, n, prompt_lookup_num_tokens=D, _draft_from=bad, output_acceptance=True)
    assert torch.equal(got2, plain)
    rows = plain.tolist()
    for b in range(B):
        # (a row past a wrong draft, or past the budget, has a pick the contract never looks at: any value serves)
        want, fed = spec_ref.run(lambda seq: rows[b][min(len(seq) - 9, n - 1)], tok[b].tolist(), n, D, draft_from=bad[b].tolist())
        assert want == rows[b]
        row = acc2[b].tolist()
        assert row[:len(fed)] == fed and not any(row[len(fed):]), (b, row, fed)
    # every draft wrong: one token per step, the price of the K-row step
    got3, acc3 = lm.generate(tok, n, prompt_lookup_num_tokens=D, _draft_from=(plain + 1) % 502, output_acceptance=True, eos_poll=5)
    assert torch.equal(got3, plain) and acc3.shape == (B, n) and bool((acc3 == 1).all())


@pytest.mark.parametrize("ngram", [1, 2, 3])
def test_the_lookup_itself_on_a_prompt_of_one_repeated_block(ngram):
    """The drafts come from the row's own history; whatever the model answers, the acceptance per step is what the contract says
    for the picks the returned logits give (spec_ref.run fed those picks)."""
    lm = _lm(seed=9).to("cuda")
    lm.precision = "fp32"
    D, n = 3, 20
    block = torch.randint(0, 502, (2, 4), generator=torch.Generator().manual_seed(11))
    tok = block.repeat(1, 4).cuda()                             # 16 prompt tokens: one block four times
    got, logits, acc = lm.generate(tok, n, prompt_lookup_num_tokens=D, max_matching_ngram_size=ngram, output_logits=True,
                                   output_acceptance=True)
    _picks_are_the_greedy_rule(got, logits)
    picks = logits.argmax(-1).cpu()
    assert torch.equal(picks, got.cpu())
    for b in range(2):
        # a next-token function that replays the run: the model's pick after a prefix of the final sequence; any other prefix is a
        # rejected draft's row, whose pick the contract never looks at (a value that can confirm nothing)
        final = tok[b].tolist() + got[b].tolist()

        def nxt(seq, final=final):
            return final[len(seq)] if seq == final[:len(seq)] and len(seq) < len(final) else -1
        want, steps = spec_ref.run(nxt, tok[b].tolist(), n, D, ngram)
        assert want == got[b].tolist()
        row = acc[b].tolist()
        assert row[:len(steps)] == steps and not any(row[len(steps):]), (b, row, steps)


def test_eos_budget_and_poll(monkeypatch):
    from kosmosx import ops
    calls = []
    real = ops.spec_accept
    monkeypatch.setattr(ops, "spec_accept", lambda *a, **k: (calls.append(k["step"]), real(*a, **k))[1])
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(6)).cuda()
    n, pad, D = 22, 1, 3
    free = lm.generate(tok, n).cpu()
    eos = int(free[0, 3])
    first = [(free[b] == eos).nonzero()[0].item() if (free[b] == eos).any() else None for b in range(3)]
    got, acc = lm.generate(tok, n, eos_token_id=eos, pad_token_id=pad, prompt_lookup_num_tokens=D, _draft_from=free.cuda(),
                           output_acceptance=True, eos_poll=2)
    got = got.cpu()
    for b in range(3):
        f = n if first[b] is None else first[b]
        assert torch.equal(got[b, :min(f + 1, got.shape[1])], free[b, :min(f + 1, got.shape[1])])       # up to and including the EOS
        assert bool((got[b, f + 1:] == pad).all())
        assert int(acc[b].sum()) == min(f + 1, n)
    assert got.shape[1] == max(min((n if f is None else f) + 1, n) for f in first)
    # one row: the poll ends the loop no later than eos_poll steps after the row finished
    del calls[:]
    one, acc1 = lm.generate(tok[:1], n, eos_token_id=eos, pad_token_id=pad, prompt_lookup_num_tokens=D, _draft_from=free[:1].cuda(),
                            output_acceptance=True, eos_poll=2)
    assert one.shape[1] == first[0] + 1 and torch.equal(one.cpu()[0], free[0, :first[0] + 1])
    assert acc1.shape[1] == 1 + math.ceil(first[0] / (D + 1))                             # the steps that emitted ...
    assert calls == list(range(len(calls))) and acc1.shape[1] <= len(calls) < acc1.shape[1] + 2 and len(calls) < n   # ... and the steps issued
    # max_new_tokens is never exceeded, whatever n is against K, and the lookup proper gives the plain tokens
    for m in (1, 2, 5, 9):
        out, a = lm.generate(tok, m, prompt_lookup_num_tokens=D, _draft_from=free[:, :m].contiguous().cuda(), output_acceptance=True)
        assert out.shape == (3, m) and torch.equal(out.cpu(), free[:, :m]) and bool((a.sum(1) == m).all())
    with pytest.raises(IndexError, match="draft rows"):
        lm.generate(tok, 62 - 9 - D + 1, prompt_lookup_num_tokens=D)
    assert lm.generate(tok, 62 - 9 - D, prompt_lookup_num_tokens=D).shape == (3, 62 - 9 - D)


def test_the_defaults_issue_no_lookup_launch_and_give_the_same_tokens(monkeypatch):
    from kosmosx import ops
    calls = {"spec_accept": 0, "attention_decode_block": 0}
    real = ops.spec_accept

    def counted(*a, **k):
        calls["spec_accept"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "spec_accept", counted)
    monkeypatch.setattr(ops, "attention_decode_block", lambda *a, **k: calls.__setitem__("attention_decode_block", 1))
    lm = _lm(seed=6).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(2)).cuda()
    n = 12
    got = lm.generate(tok, n)
    assert calls == {"spec_accept": 0, "attention_decode_block": 0}
    # the tokens of the single-token loop: the incremental path with argmax (tests/test_generate_gpu.py)
    state, seq, want = {}, tok, []
    out = lm(seq, incremental_state=state)
    for _ in range(n):
        nxt = out[:, -1].argmax(-1)
        want.append(nxt)
        seq = torch.cat([seq, nxt[:, None]], 1)
        if len(want) < n:
            out = lm(seq, incremental_state=state)
    assert torch.equal(got, torch.stack(want, 1))
    assert torch.equal(lm.generate(tok, n, prompt_lookup_num_tokens=0), got) and calls["spec_accept"] == 0
    assert torch.equal(lm.generate(tok, n, prompt_lookup_num_tokens=2), got) and calls["spec_accept"] >= 1
