"""generate(guidance_scale=, negative_prompt_ids=, negative_prompt_lengths=, negative_images=) end to end on the device.

Exact replay, the scheme of tests/test_generate_shape_gpu.py: ``output_logits`` returns the conditional AND the unconditional rows'
raw logits of every step; the guided row is rebuilt from them — the device's own log-probs (ops.token_logprob) combined by
tests/guidance_ref.py — then the constraint and shaping references are applied where the case uses them and the pick is repeated:
arg max with the lowest id on ties, or ops.sample_logits on the rebuilt row with the call's seed, position and sequence id.  Every
emitted token must match exactly.

Feeding, the part the replay cannot see: both returned logits tensors against the CPU oracle's full forward, row by row over the
unpadded prompt_b + tokens_b and negative_b + tokens_b, teacher forced, at the tolerances of tests/test_generate_gpu.py."""
import numpy as np
import pytest
import torch

import constrain_ref as CR
import guidance_ref as GR
import sampling_ref as R
import shape_ref as SR
from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx import _hip, ops
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

V = 502
PAD = 1
CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=V, max_pos=64)
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=21)
TOL = {"fp32": 2e-4, "mixed": 1e-3}
B, P, N = 3, 9, 12


@pytest.fixture(scope="module")
def lm():
    """(the model on the device, its weights for the oracle): built once, read only."""
    m = KosmosLanguage(vocab_size=V, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=7, _perturb=0.1, _max_positions=64).eval()
    w = oracle_weights(m)
    return m.to("cuda"), w


def _tok(rows, T, seed, vocab=V):
    return torch.randint(2, vocab, (rows, T), generator=torch.Generator().manual_seed(seed))


def _logprobs(rows):
    """kx_token_logprob of every id of every row of the device fp32 [R, V] tensor -> numpy [R, V]."""
    Rn, Vn = rows.shape
    tgt = torch.arange(Vn, dtype=torch.int64, device=rows.device).repeat(Rn)
    idx = torch.arange(Rn, dtype=torch.int32, device=rows.device).repeat_interleave(Vn)
    return ops.token_logprob(rows, tgt, row_index=idx).view(Rn, Vn).cpu().numpy()


def _guided(cond, uncond, s):
    """The guided rows [B, n, V] (numpy fp32) from the two returned raw logits tensors."""
    b, n, v = cond.shape
    lc, lu = _logprobs(cond.reshape(b * n, v).contiguous()), _logprobs(uncond.reshape(b * n, v).contiguous())
    return GR.guided_row_f32(lc, lu, s).reshape(b, n, v)


def _replay(tokens, cond, uncond, s, kw, positions, prompts, *, eos=None, seq_ids=None):
    """Every token of every row from the rebuilt guided rows.  ``prompts``: row b's unpadded conditional prompt ids (the history
    the constraints read); ``positions``: row b's Philox position at step 0 (the conditional row's).  Returns the steps at which
    each row was still running."""
    guided = _guided(cond, uncond, s)
    tokens = tokens.cpu().numpy()
    rows, n = tokens.shape
    bias = kw.get("logit_bias")
    pairs = [sorted(bias.items())] * rows if bias else [()] * rows
    f, p, ngram = kw.get("frequency_penalty", 0.0), kw.get("presence_penalty", 0.0), kw.get("no_repeat_ngram_size", 0)
    greedy = not kw.get("do_sample", False)
    live = []
    for b in range(rows):
        counts, last, finished, steps = (np.zeros(V, dtype=np.int32) if f or p else None), None, False, 0
        for g in range(n):
            if finished:
                assert int(tokens[b, g]) == PAD, (b, g)
                continue
            steps += 1
            row = guided[b, g]
            if ngram:
                ban, _ = CR.constrain_row(list(prompts[b]) + tokens[b, :g].tolist(), row, new_tokens=g, ngram=ngram)
                row = CR.apply(row, ban)
            if bias or f or p:
                row, counts = SR.shape_row(row, counts, bias=pairs[b], frequency=f, presence=p, last_token=last)
            if greedy:
                x = R.penalised(row)
                assert (x > -np.inf).any()
                want = int(np.argmax(x))                                     # (the first of exact ties)
            else:
                want = int(ops.sample_logits(torch.from_numpy(row[None]).cuda(), temperature=kw["temperature"], top_k=kw.get("top_k", 0),
                                             top_p=kw.get("top_p", 1.0), seed=kw["seed"], position=positions[b] + g, pad_token_id=PAD,
                                             sequence_ids=torch.tensor([b if seq_ids is None else seq_ids[b]], device="cuda"))[0])
            assert int(tokens[b, g]) == want, (b, g, int(tokens[b, g]), want)
            last = want
            finished = eos is not None and want == eos
        live.append(steps)
    return live


def _feeding(w, prompts, tokens, logits, live, tol, what):
    """Teacher forced, one unpadded row at a time: logits[b, g] is the oracle's row at position len_b - 1 + g of prompt_b + tokens_b."""
    tokens = tokens.cpu()
    worst = 0.0
    for b, prompt in enumerate(prompts):
        n = live[b]
        full = torch.cat([torch.tensor(prompt, dtype=torch.int64), tokens[b, :n - 1]])[None]
        ref = O.kosmos_language_forward(w, full, CFG)[:, len(prompt) - 1:]
        worst = max(worst, rel_err(logits[b:b + 1, :n], ref))
    print(f"guided generate, {what} logits vs oracle: {worst:.3e}")
    assert worst < tol, (what, worst)


NEG_SHORT, NEG_LONG = _tok(B, 4, seed=11), _tok(B, 14, seed=12)
LANGUAGE_CASES = {
    "greedy-short-negative": dict(s=1.5, neg=NEG_SHORT),
    "sampled-long-negative-ragged": dict(s=3.0, neg=NEG_LONG, lens=[4, 9, 6], nlens=[14, 3, 8], kw=SAMPLE),
    "greedy-ragged-negative-scale-below-one": dict(s=-0.5, neg=NEG_LONG, nlens=[1, 14, 9]),
    "shaping-and-ngrams": dict(s=1.5, neg=NEG_SHORT, kw=dict(logit_bias={7: 3.0, 400: -float("inf"), 77: -1.0}, frequency_penalty=0.7,
                                                          no_repeat_ngram_size=2)),
    "sampled-shaping": dict(s=2.0, neg=NEG_LONG, lens=[9, 5, 7], kw=dict(SAMPLE, presence_penalty=0.4, frequency_penalty=0.3)),
    "eos": dict(s=1.5, neg=NEG_SHORT, eos=True, kw=SAMPLE),
    "prefill-chunk": dict(s=1.5, neg=NEG_LONG, lens=[4, 9, 6], nlens=[14, 3, 8], kw=dict(prefill_chunk=4)),
    "mixed": dict(s=1.5, neg=NEG_SHORT, prec="mixed", kw=SAMPLE),
    "default-negative": dict(s=1.5, neg=None, lens=[4, 9, 6]),
}


@pytest.mark.parametrize("name", list(LANGUAGE_CASES))
def test_language_tokens_replay_exactly_and_both_rows_are_fed_right(lm, name):
    model, w = lm
    case = LANGUAGE_CASES[name]
    s, neg, lens, nlens, kw = case["s"], case["neg"], case.get("lens"), case.get("nlens"), dict(case.get("kw", {}))
    model.precision = prec = case.get("prec", "fp32")
    tok = _tok(B, P, seed=4)
    call = dict(kw, guidance_scale=s, pad_token_id=PAD)
    if lens is not None:
        call["prompt_lengths"] = lens
    if neg is not None:
        call["negative_prompt_ids"] = neg.cuda()
    if nlens is not None:
        call["negative_prompt_lengths"] = nlens
    if case.get("eos"):
        first = model.generate(tok.cuda(), N, **call).cpu()
        others = set(first[0].tolist()) | set(first[2].tolist())
        stop = [g for g in range(N - 4) if int(first[1, g]) not in others]  # a token only row 1 emits: the rows do not see each other
        assert stop, first
        call["eos_token_id"] = int(first[1, stop[0]])                       # row 1 finishes early and pads, rows 0 and 2 run on
    tokens, cond, uncond = model.generate(tok.cuda(), N, output_logits=True, **call)
    assert tokens.shape == (B, N) and cond.shape == uncond.shape == (B, N, V) and uncond.dtype == torch.float32
    prompts = [tok[b, :(P if lens is None else lens[b])].tolist() for b in range(B)]
    if neg is None:
        negatives = [p[-1:] for p in prompts]                               # the last prompt token
    else:
        negatives = [neg[b, :(neg.shape[1] if nlens is None else nlens[b])].tolist() for b in range(B)]
    eos = call.get("eos_token_id")
    live = _replay(tokens, cond, uncond, s, kw, [len(p) for p in prompts], prompts, eos=eos)
    if eos is not None:
        assert live == [N, stop[0] + 1, N] and int(tokens[1, stop[0]]) == eos and bool((tokens[1, stop[0] + 1:] == PAD).all())
        assert torch.equal(tokens.cpu()[[0, 2]], first[[0, 2]])
    assert torch.equal(model.generate(tok.cuda(), N, **call), tokens)       # without the logits kept
    _feeding(w, prompts, tokens, cond, live, TOL[prec], f"{name}: conditional")
    _feeding(w, negatives, tokens, uncond, live, TOL[prec], f"{name}: unconditional")


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("negative", ["text", "images"])
def test_kosmos_tokens_replay_and_logits_match_the_oracle(alias, negative):
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = "fp32"
    g = torch.Generator().manual_seed(5)
    rows, Tt, n, vocab, n_img = 2, 10, 12, m.cfg.vocab, m.cfg.perceiver.latents
    tok = torch.randint(2, vocab, (rows, Tt), generator=g)
    img = torch.randn(rows, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    neg_tok = torch.randint(2, vocab, (rows, 6), generator=g) if negative == "text" else tok
    neg_img = torch.randn(rows, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g) if negative == "images" else img
    extra = dict(negative_prompt_ids=neg_tok.cuda()) if negative == "text" else dict(negative_images=neg_img.cuda())
    for kw in (dict(), dict(SAMPLE, top_k=50)):
        call = dict(kw, guidance_scale=2.0, pad_token_id=PAD, **extra)
        tokens, cond, uncond = m.generate(tok.cuda(), img.cuda(), n, output_logits=True, **call)
        assert tokens.shape == (rows, n) and cond.shape == uncond.shape == (rows, n, vocab)
        guided = _guided(cond, uncond, 2.0)
        for b in range(rows):
            for step in range(n):
                if kw:
                    want = int(ops.sample_logits(torch.from_numpy(guided[b, step][None]).cuda(), temperature=kw["temperature"],
                                                 top_k=kw["top_k"], top_p=kw["top_p"], seed=kw["seed"], position=Tt + n_img + step,
                                                 pad_token_id=PAD, sequence_ids=torch.tensor([b], device="cuda"))[0])
                else:
                    want = int(np.argmax(R.penalised(guided[b, step])))
                assert int(tokens[b, step]) == want, (b, step)
        assert torch.equal(m.generate(tok.cuda(), img.cuda(), n, **call), tokens)
        for text, pix, got, what in ((tok, img, cond, "conditional"), (neg_tok, neg_img, uncond, "unconditional")):
            full = torch.cat([text, tokens.cpu()[:, :-1]], 1)
            ref = O.kosmos_forward(w, full, pix, cfg, oracle_switches(sw))[:, text.shape[1] + n_img - 1:]
            e = rel_err(got, ref)
            print(f"guided Kosmos.generate (alias={alias}, negative {negative}, {'sampled' if kw else 'greedy'}), {what} vs oracle: {e:.3e}")
            assert e < TOL["fp32"]


def test_guidance_changes_the_tokens(lm):
    model, _ = lm
    model.precision = "fp32"
    tok = _tok(B, P, seed=4).cuda()
    plain = model.generate(tok, N, pad_token_id=PAD, **SAMPLE)
    guided = model.generate(tok, N, guidance_scale=3.0, negative_prompt_ids=NEG_LONG.cuda(), pad_token_id=PAD, **SAMPLE)
    assert guided.shape == plain.shape and not torch.equal(guided, plain)


def test_logprobs_are_those_of_the_conditional_rows(lm):
    model, _ = lm
    model.precision = "fp32"
    tok = _tok(B, P, seed=4).cuda()
    k = 4
    for kw in (dict(), dict(SAMPLE, logit_bias={7: 5.0})):
        call = dict(kw, guidance_scale=2.0, negative_prompt_ids=NEG_SHORT.cuda(), pad_token_id=PAD, output_logprobs=True, top_logprobs=k)
        tokens, cond, uncond, lp, tl, ti = model.generate(tok, N, output_logits=True, **call)
        flat = cond.reshape(B * N, V)
        want = ops.token_logprob(flat, tokens.reshape(B * N).contiguous()).view(B, N)
        assert torch.equal(lp.view(torch.int32), want.view(torch.int32)) and bool((lp < 0).all())
        idx = torch.arange(B * N, dtype=torch.int32, device="cuda").repeat_interleave(k)
        assert torch.equal(tl, ops.token_logprob(flat, ti.reshape(B * N * k).contiguous(), row_index=idx).view(B, N, k))
        lean = model.generate(tok, N, **call)                               # the raw row is then the clone taken before the launch
        assert len(lean) == 4 and torch.equal(lean[0], tokens) and torch.equal(lean[1], lp) and torch.equal(lean[2], tl)


def test_a_scale_of_one_is_off(lm):
    model, _ = lm
    model.precision = "fp32"
    tok = _tok(B, P, seed=4).cuda()
    calls = [lambda **kw: model.generate(tok, 6, output_logits=True, **kw),
             lambda **kw: model.generate(tok, 6, output_logits=True, prompt_lengths=[4, 9, 6], **SAMPLE, **kw)]

    def records(call, **kw):
        _hip.prof_enable(True)
        try:
            out = call(**kw)
            torch.cuda.synchronize()
            return out, _hip.prof_collect()
        finally:
            _hip.prof_enable(False)

    for call in calls:
        (t0, l0), before = records(call)                                    # the call as the tree before the feature made it
        res, after = records(call, guidance_scale=1.0)
        assert len(res) == 2 and torch.equal(res[0], t0) and torch.equal(res[1].view(torch.int32), l0.view(torch.int32))
        assert [r[:4] for r in after] == [r[:4] for r in before]            # the same launches, one for one
        assert not [r for r in after if r[0] == "misc" and r[3] == 33]      # no kx_guidance_logits record
        _, on = records(call, guidance_scale=1.5)
        assert len([r for r in on if r[0] == "misc" and r[3] == 33]) == 6   # one per token when it is on
