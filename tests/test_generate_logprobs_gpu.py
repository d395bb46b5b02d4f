"""generate(output_logprobs=True, top_logprobs=k): every generated token's log-prob and the k most likely alternatives, taken on the
device by one kx_step_logprobs launch per step (tests/test_step_logprobs_gpu.py holds the kernel to float64).

What the loops add is plumbing, so the checks are exact: with the feature on, the tokens and the ``output_logits`` rows are those of
the call without it; token_logprobs[b, g] is, bit for bit, kx_token_logprob of the returned row logits[b, g] at tokens[b, g] — the
model's own distribution, whatever the bans, the penalty and the filters did to the row afterwards; top_ids[b, g] is the reference
order of that row (tests/logprob_ref.py); the slots after a row's end are exactly 0.0 / -1.  The tiny models are those of
tests/test_generate_parallel_gpu.py."""
import pytest
import torch

import logprob_ref as R
from helpers import tiny_config
from kosmosx import _hip as H
from kosmosx import ops
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage

pytestmark = pytest.mark.gpu

V = 102
SAMPLE = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, repetition_penalty=1.15, seed=33)
PRECS = pytest.mark.parametrize("prec", ["fp32", "mixed"])


def _lm(prec, max_pos=64, seed=5):
    lm = KosmosLanguage(vocab_size=V, dim=128, depth=2, ffn_dim=256, decoder_heads=2, _seed=seed, _perturb=0.1,
                        _max_positions=max_pos).eval().to("cuda")
    lm.precision = prec
    return lm


def _tok(B, T, seed=4, vocab=V):
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _live(tokens, prompts, eos=None, stop=None):
    """[B, n] bool: the slots a row filled before it ended — its EOS, or the last id of its first stop sequence, included.
    ``prompts``: per row the text ids in front of the output (a stop sequence may begin in them)."""
    B, n = tokens.shape
    live = torch.ones((B, n), dtype=torch.bool)
    for b in range(B):
        row = tokens[b].tolist()
        end = n
        if eos is not None and eos in row:
            end = row.index(eos) + 1
        for s in stop or []:
            ids = list(prompts[b]) + row
            P = len(prompts[b])
            for j in range(n):
                if P + j + 1 >= len(s) and ids[P + j + 1 - len(s):P + j + 1] == s:
                    end = min(end, j + 1)
                    break
        live[b, end:] = False
    return live


def _check(gen, k, live_of=None):
    """``gen(**kw)`` -> what generate() returns.  The feature on against the feature off; returns the outputs of the call with it on."""
    off = gen(output_logits=True)
    on = gen(output_logits=True, output_logprobs=True, top_logprobs=k)
    assert len(off) == 2 and len(on) == (5 if k else 3)
    tokens, logits, lp = on[:3]
    assert torch.equal(tokens, off[0]) and torch.equal(logits, off[1])       # nothing the call returned before has changed
    B, n, vocab = logits.shape
    assert lp.shape == (B, n) and lp.dtype == torch.float32
    live = (torch.ones((B, n), dtype=torch.bool) if live_of is None else live_of(tokens.cpu())).cuda()
    flat = logits.reshape(B * n, vocab)
    want = ops.token_logprob(flat, tokens.reshape(B * n).contiguous()).view(B, n)
    assert torch.equal(lp[live], want[live])                                 # bit-equal to the gather on the returned rows
    assert bool((lp[~live] == 0.0).all())                                    # exactly zero after a row's end
    assert bool((lp[live] < 0).all())
    if k:
        tl, ti = on[3:]
        assert tl.shape == (B, n, k) and tl.dtype == torch.float32 and ti.shape == (B, n, k) and ti.dtype == torch.int64
        ref = torch.stack([R.top_ref(r, k)[0] for r in flat.cpu()]).view(B, n, k).cuda()
        assert torch.equal(ti[live], ref[live])
        assert bool((ti[~live] == -1).all()) and bool((tl[~live] == 0.0).all())
        rows = torch.arange(B * n, dtype=torch.int32, device="cuda").repeat_interleave(k)
        same = ops.token_logprob(flat, ti.reshape(B * n * k).clamp(min=0).contiguous(), row_index=rows).view(B, n, k)
        assert torch.equal(tl[live], same[live])
        assert bool((tl[..., 0] >= lp)[live].all())
        picked = (ti == tokens[..., None]).any(-1)                           # where the token is among the alternatives: its log-prob
        assert torch.equal(tl[ti == tokens[..., None]], lp[picked])
    # without output_logits (no clone is kept): the same numbers
    lean = gen(output_logprobs=True, top_logprobs=k)
    assert len(lean) == len(on) - 1 and torch.equal(lean[0], tokens)
    assert all(torch.equal(a, b) for a, b in zip(lean[1:], on[2:]))
    return on


@PRECS
def test_greedy_uniform(prec):
    lm = _lm(prec)
    tok = _tok(3, 11)
    on = _check(lambda **kw: lm.generate(tok, 9, **kw), 5)
    assert bool((on[4][..., 0] == on[0]).all())                              # greedy: the token is the first alternative
    assert torch.equal(on[3][..., 0], on[2])
    _check(lambda **kw: lm.generate(tok, 9, **kw), 0)
    res = lm.generate(tok, 9, output_logprobs=True)                          # one extra output: a pair
    assert isinstance(res, tuple) and len(res) == 2 and torch.equal(res[1], on[2])


@PRECS
def test_sampled_ragged(prec):
    lm = _lm(prec)
    tok = _tok(3, 11)
    _check(lambda **kw: lm.generate(tok, 10, prompt_lengths=[11, 5, 8], **SAMPLE, **kw), 16)
    _check(lambda **kw: lm.generate(tok, 10, prompt_lengths=[11, 5, 8], prefill_chunk=4, **SAMPLE, **kw), 1)


@PRECS
def test_parallel_sampling(prec):
    lm = _lm(prec)
    tok = _tok(2, 9, seed=8)
    on = _check(lambda **kw: lm.generate(tok, 8, num_return_sequences=3, **SAMPLE, **kw), 5)
    assert on[0].shape == (6, 8) and on[2].shape == (6, 8) and on[4].shape == (6, 8, 5)
    for b in range(2):                                                       # rows b * n + i: one first row per prompt
        assert torch.equal(on[4][3 * b, 0], on[4][3 * b + 1, 0]) and torch.equal(on[3][3 * b, 0], on[3][3 * b + 2, 0])


@PRECS
def test_a_session_second_turn(prec):
    lm = _lm(prec)
    tok, x2 = _tok(2, 9, seed=8), _tok(2, 3, seed=9)

    def second(**kw):
        first = lm.generate(tok, 6, return_session=True, **SAMPLE)
        return first[-1].generate(x2, 7, prompt_lengths=[3, 2], **SAMPLE, **kw)
    _check(second, 5)
    # the first turn: the session stays last
    res = lm.generate(tok, 6, return_session=True, output_logits=True, output_logprobs=True, top_logprobs=2, **SAMPLE)
    assert len(res) == 6 and res[1].shape == (2, 6, V) and res[2].shape == (2, 6) and res[3].shape == (2, 6, 2)
    assert res[4].dtype == torch.int64 and hasattr(res[5], "generate")
    plain = lm.generate(tok, 6, return_session=True, **SAMPLE)
    assert torch.equal(plain[0], res[0]) and res[5].lengths == plain[1].lengths


@PRECS
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_with_images(prec, alias):
    m = Kosmos._from_config(tiny_config(), seed=1, switches=Switches(u1_inplace_alias=alias), perturb=0.1).eval().to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(0, m.cfg.vocab, (2, 10), generator=g).cuda()
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    _check(lambda **kw: m.generate(tok, img, 8, **kw), 5)
    _check(lambda **kw: m.generate(tok, img, 8, prompt_lengths=[10, 6], num_return_sequences=2, **SAMPLE, **kw), 3)


@PRECS
def test_finished_rows_hold_exact_zeros(prec):
    lm = _lm(prec)
    B, N = 3, 12
    tok = _tok(B, 10, seed=9)
    kw = dict(do_sample=True, temperature=1.2, seed=12, pad_token_id=0, eos_poll=4)
    free = lm.generate(tok, N, **kw).cpu()
    prompts = tok.cpu().tolist()
    eos = int(free[1, 2])                                                    # a token row 1 draws at step 2
    on = _check(lambda **c: lm.generate(tok, N, eos_token_id=eos, **kw, **c), 5, lambda t: _live(t, prompts, eos=eos))
    live = _live(on[0].cpu(), prompts, eos=eos)
    assert not bool(live[1, 3:].any()) and bool(live[1, 0])                  # row 1 ends at step 2 at the latest ...
    end = int(live[1].sum()) - 1
    assert int(on[0][1, end]) == eos and float(on[2][1, end]) < 0            # ... and its EOS slot is live
    assert bool((on[2][1, end + 1:] == 0.0).all()) and bool((on[4][1, end + 1:] == -1).all())
    # ragged rows (the sampler's device positions) and a session's pad count see the same moment
    _check(lambda **c: lm.generate(tok, N, eos_token_id=eos, prompt_lengths=[10, 7, 4], **kw, **c), 2,
           lambda t: _live(t, [p[:l] for p, l in zip(prompts, [10, 7, 4])], eos=eos))
    stop = [[int(free[2, 3]), int(free[2, 4])]]                              # two ids row 2 generates
    on = _check(lambda **c: lm.generate(tok, N, stop_sequences=stop, **kw, **c), 5, lambda t: _live(t, prompts, stop=stop))
    live = _live(on[0].cpu(), prompts, stop=stop)
    end = int(live[2].sum()) - 1
    assert end <= 4 and int(on[0][2, end]) == stop[0][1] and float(on[2][2, end]) < 0                   # the stop token's slot is live
    assert end + 1 == on[0].shape[1] or (float(on[2][2, end + 1]) == 0.0 and int(on[4][2, end + 1, 0]) == -1)


@PRECS
def test_logprobs_are_of_the_raw_logits_under_bans(prec):
    lm = _lm(prec)
    tok = _tok(2, 9, seed=8)
    free = lm.generate(tok, 10).cpu()
    banned = int(free[0, 0])                                                 # what row 0 picks first, unconstrained
    cons = dict(bad_words_ids=[[banned]], no_repeat_ngram_size=2)
    on = _check(lambda **kw: lm.generate(tok, 10, **cons, **kw), 5)
    assert not bool((on[0] == banned).any())                                 # never generated ...
    assert int(on[4][0, 0, 0]) == banned and int(on[0][0, 0]) != banned      # ... but still the most likely alternative of its step
    assert float(on[3][0, 0, 0]) > float(on[2][0, 0])
    _check(lambda **kw: lm.generate(tok, 10, min_new_tokens=3, eos_token_id=int(free[1, 1]), eos_poll=0, **kw), 2,
           lambda t: _live(t, None, eos=int(free[1, 1])))                    # a constraint launch on the first steps only
    _check(lambda **kw: lm.generate(tok, 10, **cons, **SAMPLE, **kw), 16)


def _launches(fn):
    H.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return len(H.prof_collect()), out
    finally:
        H.prof_enable(False)


@pytest.mark.parametrize("k", [0, 5])
def test_one_more_launch_per_step_and_none_by_default(k):
    lm = _lm("mixed")
    tok, N = _tok(2, 9, seed=8), 7
    for kw in (dict(), dict(bad_words_ids=[[3]], stop_sequences=[[5, 6, 7, 8]], eos_token_id=101, prompt_lengths=[9, 4], **SAMPLE)):
        lm.generate(tok, N, **kw)                                            # (warm: packing and workspaces)
        before, plain = _launches(lambda: lm.generate(tok, N, **kw))
        with_lp, on = _launches(lambda: lm.generate(tok, N, output_logprobs=True, top_logprobs=k, **kw))
        after, again = _launches(lambda: lm.generate(tok, N, **kw))
        n = on[0].shape[1]
        assert torch.equal(on[0], plain) and torch.equal(again, plain)
        assert before == after                                               # the default path launches what it launched
        assert with_lp == before + n, (before, with_lp, n)                   # one kx_step_logprobs per step, nothing else
