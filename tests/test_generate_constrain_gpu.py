"""generate() with constraints (no_repeat_ngram_size, bad_words_ids, min_new_tokens, stop_sequences), end to end on the device.

The replay tests follow tests/test_generate_gpu.py's scheme: ``output_logits`` returns the model's own logits of every step;
the NumPy restatement of kx_constrain_logits (tests/constrain_ref.py) and then of the sampler (tests/sampling_ref.py) are applied
to THOSE logits with the row's own logical history so far, and must reproduce the emitted token."""
import numpy as np
import pytest
import torch

import constrain_ref as CR
import sampling_ref as R
from helpers import tiny_config
from kosmosx import ops
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from test_generate_beam_gpu import _replay as _beam_replay

pytestmark = pytest.mark.gpu

EPS_P, EPS_G = 1e-5, 1e-4
PAD = 1
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.2, seed=21)
KWS = pytest.mark.parametrize("kw", [dict(), SAMPLE], ids=["greedy", "sampled"])


def _lm(seed=5):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=64).eval()


def _constraints(free):
    """Constraints that bite on the unconstrained greedy run ``free`` [B, n]: ids and pairs it emits early."""
    free = free.cpu()
    return dict(no_repeat_ngram_size=2, bad_words_ids=[[int(free[0, 1])], [int(free[-1, 2]), int(free[-1, 3])]],
                min_new_tokens=4, eos_token_id=int(free[0, 2]))


def _with_stop(run, cons):
    """``cons`` plus a stop sequence the constrained run is certain to meet: a pair of consecutive tokens that a row of
    ``run(cons)`` emits while it is still running — at steps 6 and 7, or earlier where the row meets EOS before (min_new_tokens = 4
    keeps every row running for four tokens).  Decoding is deterministic (greedy, or Philox addressed by seed, sequence and position),
    so the run with the stop sequence emits the same tokens up to that pair and the row then stops (unless it met the pair earlier)."""
    got = run(cons).cpu()
    eos = cons["eos_token_id"]
    row, g = 0, 0
    for b in range(got.shape[0]):
        live = next((i for i, t in enumerate(got[b, :8].tolist()) if t in (eos, PAD)), 8)      # tokens 0 .. live - 1 are real
        if live - 1 > g:
            row, g = b, live - 1
    assert g >= 1, got
    return dict(cons, stop_sequences=[[int(got[row, g - 1]), int(got[row, g])]])


def _replay(tokens, logits, prompts, starts, kw, cons):
    """Every token of every row: constrain_ref, then sampling_ref, on the returned logits with the row's logical history.
    Returns the number of steps at which a ban removed the raw row's arg max (the constraints did something)."""
    tokens, logits = tokens.cpu().numpy(), logits.cpu().numpy()
    B, n = tokens.shape
    eos = cons.get("eos_token_id")
    used = bites = stops = 0
    for b in range(B):
        finished = False
        for g in range(n):
            hist = np.concatenate([prompts[b], tokens[b, :g]])
            ban, fin = CR.constrain_row(hist, logits[b, g], new_tokens=g, ngram=cons.get("no_repeat_ngram_size", 0),
                                        bad_words=cons.get("bad_words_ids") or (), stop_sequences=cons.get("stop_sequences") or (),
                                        min_new=cons.get("min_new_tokens", 0), eos_id=eos, finished=finished)
            if fin:                                                       # finished before, or stopped now: pad from here on
                stops += not finished
                finished = True
                assert int(tokens[b, g]) == PAD, (b, g)
                continue
            bites += bool(ban[int(np.nanargmax(logits[b, g]))])
            ref = R.sample_row(CR.apply(logits[b, g], ban), temperature=kw.get("temperature", 1.0), top_k=kw.get("top_k", 0),
                               top_p=kw.get("top_p", 1.0), repetition_penalty=kw.get("repetition_penalty", 1.0),
                               do_sample=kw.get("do_sample", False), seed=kw.get("seed", 0), position=starts[b] + g, sequence_id=b,
                               history=hist, pad_token_id=PAD)
            used += R.check_draw(int(tokens[b, g]), ref, EPS_P, EPS_G, kw.get("top_p", 1.0)) == "eps"
            assert not ban[int(tokens[b, g])] or ref["none"], (b, g)
            finished = ref["none"] or (eos is not None and int(tokens[b, g]) == eos)
    assert used <= 0.01 * B * n, used
    return bites, stops


@KWS
def test_language_tokens_replay_through_the_references(kw):
    lm = _lm(seed=7).to("cuda")
    lm.precision = "fp32"
    B, P, n = 3, 9, 24
    tok = torch.randint(0, 502, (B, P), generator=torch.Generator().manual_seed(4))
    base = _constraints(lm.generate(tok.cuda(), n))
    cons = _with_stop(lambda c: lm.generate(tok.cuda(), n, pad_token_id=PAD, eos_poll=0, **c, **kw), base)
    got, logits = lm.generate(tok.cuda(), n, output_logits=True, pad_token_id=PAD, eos_poll=0, **cons, **kw)
    assert got.shape == (B, n) and logits.shape == (B, n, 502)
    bites, stops = _replay(got, logits, tok.numpy(), [P] * B, kw, cons)
    print(f"language replay: the bans removed the arg max at {bites} steps, {stops} rows stopped")
    assert stops >= 1 and (bites > 0 or kw)                              # (greedy: the constraints come from the greedy run and must bite)
    assert torch.equal(lm.generate(tok.cuda(), n, pad_token_id=PAD, eos_poll=0, **cons, **kw), got)
    # the returned logits are the model's own: no -inf from the bans
    assert bool(torch.isfinite(logits).all())
    # ragged: every row replayed with its own logical history (the padding takes part in nothing)
    lens = [4, 9, 6]
    cons = _with_stop(lambda c: lm.generate(tok.cuda(), n, prompt_lengths=lens, pad_token_id=PAD, eos_poll=0, **c, **kw), base)
    got, logits = lm.generate(tok.cuda(), n, output_logits=True, prompt_lengths=lens, pad_token_id=PAD, eos_poll=0, **cons, **kw)
    bites, stops = _replay(got, logits, [tok[b, :L].numpy() for b, L in enumerate(lens)], lens, kw, cons)
    assert stops >= 1 and (bites > 0 or kw)
    junk = tok.clone()
    for b, L in enumerate(lens):
        junk[b, L:] = 499 - b                                             # whatever the padding holds
    assert torch.equal(lm.generate(junk.cuda(), n, prompt_lengths=lens, pad_token_id=PAD, eos_poll=0, **cons, **kw), got)


@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_tokens_replay_through_the_references(alias):
    m = Kosmos._from_config(tiny_config(), seed=1, switches=Switches(u1_inplace_alias=alias), perturb=0.1).eval().to("cuda")
    m.precision = "fp32"
    g = torch.Generator().manual_seed(5)
    B, Tt, n = 2, 10, 14
    tok = torch.randint(0, m.cfg.vocab, (B, Tt), generator=g)
    img = torch.randn(B, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    n_img = m.cfg.perceiver.latents
    base = _constraints(m.generate(tok.cuda(), img, n))
    for kw in (dict(), SAMPLE):
        cons = _with_stop(lambda c: m.generate(tok.cuda(), img, n, pad_token_id=PAD, eos_poll=0, **c, **kw), base)
        got, logits = m.generate(tok.cuda(), img, n, output_logits=True, pad_token_id=PAD, eos_poll=0, **cons, **kw)
        assert got.shape == (B, n)
        bites, stops = _replay(got, logits, tok.numpy(), [Tt + n_img] * B, kw, cons)   # the history is the text ids only
        assert stops >= 1 and (bites > 0 or kw)
        lens = [5, 10]
        cons = _with_stop(lambda c: m.generate(tok.cuda(), img, n, prompt_lengths=lens, pad_token_id=PAD, eos_poll=0, **c, **kw), base)
        got, logits = m.generate(tok.cuda(), img, n, output_logits=True, prompt_lengths=lens, pad_token_id=PAD, eos_poll=0,
                                 **cons, **kw)
        bites, stops = _replay(got, logits, [tok[b, :L].numpy() for b, L in enumerate(lens)], [n_img + L for L in lens], kw, cons)
        assert stops >= 1 and (bites > 0 or kw)


def _repeated_bigrams(seq):
    grams = list(zip(seq, seq[1:]))
    return len(grams) - len(set(grams))


def test_no_bigram_occurs_twice_under_no_repeat_ngram_size_2():
    # (model and prompt seeds: on the CPU oracle's logits every row of the plain greedy run repeats four to six 2-grams, and the
    # smallest top-2 margin of the run is 3.6e-3)
    lm = _lm(seed=6).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(4))
    assert all(_repeated_bigrams(tok[b].tolist()) == 0 for b in range(3))
    n = 30
    free = torch.cat([tok, lm.generate(tok.cuda(), n).cpu()], 1)
    assert all(_repeated_bigrams(free[b].tolist()) > 0 for b in range(3))            # without the argument every row repeats one
    got = torch.cat([tok, lm.generate(tok.cuda(), n, no_repeat_ngram_size=2).cpu()], 1)
    assert all(_repeated_bigrams(got[b].tolist()) == 0 for b in range(3))
    first = min(g for b in range(3) for g in range(n) if free[b, 9 + g] != got[b, 9 + g])
    assert torch.equal(got[:, :9 + first], free[:, :9 + first])                       # identical until the first ban matters


def test_a_stop_sequence_ends_the_row_and_the_poll_ends_the_loop():
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (1, 9), generator=torch.Generator().manual_seed(6)).cuda()
    y = lm.generate(tok, 16)[0].cpu()
    stop = [[int(y[3]), int(y[4])]]
    assert not any(y[g - 1] == y[3] and y[g] == y[4] for g in range(1, 4))           # the pair is first complete at step 4
    got = lm.generate(tok, 16, stop_sequences=stop, pad_token_id=PAD, eos_poll=2)[0].cpu()
    assert got.shape[0] < 16 and got.shape[0] <= 5 + 2                                # the poll ends the loop: no eos_token_id needed
    assert torch.equal(got[:5], y[:5]) and bool((got[5:] == PAD).all())
    full = lm.generate(tok, 16, stop_sequences=stop, pad_token_id=PAD, eos_poll=0)[0].cpu()
    assert full.shape[0] == 16 and torch.equal(full[:5], y[:5]) and bool((full[5:] == PAD).all())
    # a stop sequence that starts inside the prompt and ends with the first generated token
    got = lm.generate(tok, 8, stop_sequences=[[int(tok[0, -1]), int(y[0])]], pad_token_id=PAD, eos_poll=0)[0].cpu()
    assert int(got[0]) == int(y[0]) and bool((got[1:] == PAD).all())
    # one that lies wholly in the prompt stops nothing
    got = lm.generate(tok, 8, stop_sequences=[[int(tok[0, -2]), int(tok[0, -1])]], pad_token_id=PAD, eos_poll=0)[0].cpu()
    assert torch.equal(got, y[:8])


def test_min_new_tokens_keeps_eos_away():
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(6)).cuda()
    n = 24
    free = lm.generate(tok, n).cpu()
    eos = int(free[0, 1])                                                             # what row 0 emits at step 1
    plain = lm.generate(tok, n, eos_token_id=eos, pad_token_id=PAD, eos_poll=0).cpu()
    assert int(plain[0, 1]) == eos and bool((plain[0, 2:] == PAD).all())              # without the argument row 0 ends at once
    got = lm.generate(tok, n, eos_token_id=eos, pad_token_id=PAD, eos_poll=0, min_new_tokens=4).cpu()
    assert not bool((got[:, :4] == eos).any())
    assert int(got[0, 0]) == int(free[0, 0]) and int(got[0, 1]) != eos
    ended = 0
    for b in range(3):
        hit = (got[b] == eos).nonzero()
        if len(hit):
            assert bool((got[b, int(hit[0]) + 1:] == PAD).all())                      # still ends with pad after its first EOS
            ended += 1
    print(f"min_new_tokens: {ended} of 3 rows reached EOS after the minimum")
    with pytest.raises(ValueError, match="min_new_tokens = 4 needs an eos_token_id"):
        lm.generate(tok, n, min_new_tokens=4)


def test_the_defaults_issue_no_constrain_launch(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("kx_constrain_logits launched with every constraint at its default")
    monkeypatch.setattr(ops, "constrain_logits", boom)
    lm = _lm(seed=6).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(2)).cuda()
    n = 20
    got = lm.generate(tok, n, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, stop_sequences=None)
    state, seq, want = {}, tok, []
    out = lm(seq, incremental_state=state)
    for _ in range(n):                                                    # the existing greedy test's expectation
        nxt = out[:, -1].argmax(-1)
        want.append(nxt)
        seq = torch.cat([seq, nxt[:, None]], 1)
        if len(want) < n:
            out = lm(seq, incremental_state=state)
    assert torch.equal(got, torch.stack(want, 1))
    assert torch.equal(lm.generate(tok, n, bad_words_ids=[], stop_sequences=[]), got)
    assert torch.equal(lm.generate(tok, n, prompt_lengths=[9, 9, 9], **SAMPLE), lm.generate(tok, n, **SAMPLE))
    assert lm.generate(tok, 6, num_beams=3).shape == (3, 6)
    with pytest.raises(AssertionError, match="launched"):
        lm.generate(tok, 4, no_repeat_ngram_size=2)


def test_beam_search_with_the_history_free_constraints():
    lm = _lm(seed=7).to("cuda")
    lm.precision = "fp32"
    B, P, n, W = 2, 9, 10, 3
    tok = torch.randint(0, 502, (B, P), generator=torch.Generator().manual_seed(4)).cuda()
    free = lm.generate(tok, n, num_beams=W).cpu()
    k, eos = int(free[0, 0]), int(free[1, 1])                             # ids the unconstrained search uses early
    assert k != eos and PAD not in (k, eos)
    seqs, scores, tr = lm.generate(tok, n, num_beams=W, min_new_tokens=3, bad_words_ids=[[k]], eos_token_id=eos, pad_token_id=PAD,
                                   output_scores=True, output_trace=True, eos_poll=0)
    assert seqs.shape == (B, n)
    t = _beam_replay(tr, seqs, scores, B=B, W=W, R=1, eos=eos)           # the trace's logits carry the bans: the reference is unchanged
    print(f"beam replay with constraints: {t.counted} of {t.cases} cases inside the margin")
    lg, token = tr["logits"].cpu(), tr["token"].cpu()
    ninf = float("-inf")
    assert bool((lg[0].view(B, W, 502)[:, 0, k] == ninf).all()) and bool((lg[1:, :, k] == ninf).all())
    assert bool((lg[0].view(B, W, 502)[:, 0, eos] == ninf).all()) and bool((lg[1:3, :, eos] == ninf).all())
    assert bool(torch.isfinite(lg[3:, :, eos]).all())                     # free again from step 3 on
    assert not bool((token == k).any()) and not bool((token[:3] == eos).any())
    assert not bool((seqs == k).any()) and not bool((seqs[:, :3] == eos).any())
    assert int(seqs[0, 0]) != int(free[0, 0])
