"""generate(): the device-resident decoding loop (kosmosx.generation) for both model classes.

Model parity and sampler parity are checked separately: the logits every token was drawn from are returned
(``output_logits=True``) and compared with the CPU oracle's full forward over prompt + generated tokens (teacher forced) at
the incremental path's tolerances; the tokens are compared with the CPU restatement of the sampler applied to THOSE
logits, so a logits difference inside the tolerance cannot flip a token in the test."""
import numpy as np
import pytest
import torch

import sampling_ref as R
from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

EPS_P, EPS_G = 1e-5, 1e-4
CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=64)
SAMPLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, repetition_penalty=1.2, seed=21)


def _lm(seed=5):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=64).eval()


def _sampler_parity(tokens, logits, prompt, T, kw):
    """Every returned token against the reference sampler on the returned logits (the drawn-token rule)."""
    tokens, logits, prompt = tokens.cpu().numpy(), logits.cpu().numpy(), prompt.cpu().numpy()
    B, n = tokens.shape
    used = 0
    for b in range(B):
        for g in range(n):
            ref = R.sample_row(logits[b, g], temperature=kw.get("temperature", 1.0), top_k=kw.get("top_k", 0),
                               top_p=kw.get("top_p", 1.0), repetition_penalty=kw.get("repetition_penalty", 1.0),
                               do_sample=kw.get("do_sample", False), seed=kw.get("seed", 0), position=T + g, sequence_id=b,
                               history=np.concatenate([prompt[b], tokens[b, :g]]))
            used += R.check_draw(int(tokens[b, g]), ref, EPS_P, EPS_G, kw.get("top_p", 1.0)) == "eps"
    assert used <= 0.01 * B * n, used


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_language_greedy_equals_the_incremental_path_with_argmax(prec):
    lm = _lm(seed=6).to("cuda")
    lm.precision = prec
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(2)).cuda()
    n = 20
    got = lm.generate(tok, n)
    assert got.shape == (3, n) and got.dtype == torch.int64
    state, seq, want = {}, tok, []
    out = lm(seq, incremental_state=state)
    for _ in range(n):
        nxt = out[:, -1].argmax(-1)
        want.append(nxt)
        seq = torch.cat([seq, nxt[:, None]], 1)
        if len(want) < n:
            out = lm(seq, incremental_state=state)
    assert torch.equal(got, torch.stack(want, 1))


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_kosmos_greedy_equals_the_incremental_path_with_argmax(prec):
    m = Kosmos._from_config(tiny_config(), seed=0, perturb=0.1).eval().to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, m.cfg.vocab, (2, 10), generator=g).cuda()
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g).cuda()
    n = 12
    got = m.generate(tok, img, n)
    assert got.shape == (2, n)
    feats = m.clip_model.run(img, prec, m._ws)
    feats, _ = m.perceive.run(feats, prec, m._ws, m.image_proj.weight)
    state, text, want = {}, tok, []
    out = m.decoder._forward_incremental(None, state, m.decoder.embed(text, prec, img=feats), prec)
    for _ in range(n):
        nxt = out[:, -1].argmax(-1)
        want.append(nxt)
        text = torch.cat([text, nxt[:, None]], 1)
        if len(want) < n:          # the whole spliced sequence is re-embedded as forward() would; its last row is the step's input
            out = m.decoder._forward_incremental(None, state, m.decoder.embed(text, prec, img=feats), prec)
    assert torch.equal(got, torch.stack(want, 1))


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])
@pytest.mark.parametrize("kw", [dict(), SAMPLE], ids=["greedy", "sampled"])
def test_language_logits_against_the_oracle_and_tokens_against_the_reference_sampler(prec, tol, kw):
    lm0 = _lm(seed=7)
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    P, n = 9, 24
    tok = torch.randint(0, 502, (3, P), generator=torch.Generator().manual_seed(4))
    got, logits = lm.generate(tok.cuda(), n, output_logits=True, **kw)
    assert got.shape == (3, n) and logits.shape == (3, n, 502) and logits.dtype == torch.float32
    assert int(got.min()) >= 0 and int(got.max()) < 502
    full = torch.cat([tok, got.cpu()[:, :-1]], 1)
    ref = O.kosmos_language_forward(w, full, CFG)[:, P - 1:]
    e = rel_err(logits, ref)
    print(f"generate logits vs oracle ({prec}): {e:.3e}")
    assert e < tol
    _sampler_parity(got, logits, tok, P, kw)
    again = lm.generate(tok.cuda(), n, **kw)
    assert torch.equal(again, got)


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("mixed", 1e-3)])
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_logits_against_the_oracle_forward_over_prompt_and_generated_tokens(prec, tol, alias):
    """Teacher forced through O.kosmos_forward with the generated tokens appended to text_tokens: a generated token must
    enter the decoder as forward() would embed it (two position rows under u1_inplace_alias).  Also the first test of the
    ``passed_x`` prefill."""
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    Tt, n = 10, 14
    tok = torch.randint(0, m.cfg.vocab, (2, Tt), generator=g)
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    n_img = m.cfg.perceiver.latents
    for kw in (dict(), SAMPLE):
        got, logits = m.generate(tok.cuda(), img.cuda(), n, output_logits=True, **kw)
        assert got.shape == (2, n) and logits.shape == (2, n, m.cfg.vocab)
        text = torch.cat([tok, got.cpu()[:, :-1]], 1)
        ref = O.kosmos_forward(w, text, img, cfg, oracle_switches(sw))[:, Tt + n_img - 1:]
        e = rel_err(logits, ref)
        print(f"Kosmos.generate logits vs oracle ({prec}, alias={alias}, {'sampled' if kw else 'greedy'}): {e:.3e}")
        assert e < tol
        _sampler_parity(got, logits, tok, Tt + n_img, kw)


def test_eos_pads_finished_rows_and_the_poll_ends_the_loop():
    lm = _lm(seed=8).to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, 9), generator=torch.Generator().manual_seed(6)).cuda()
    n, pad = 24, 1
    free = lm.generate(tok, n).cpu()
    eos = int(free[0, 3])                                       # a token greedy produces at step 3 for row 0
    got = lm.generate(tok, n, eos_token_id=eos, pad_token_id=pad, eos_poll=4).cpu()
    first = [(free[b] == eos).nonzero()[0].item() if (free[b] == eos).any() else None for b in range(3)]
    assert first[0] is not None and first[0] <= 3
    for b in range(3):
        f = n if first[b] is None else first[b]
        assert torch.equal(got[b, : min(f + 1, got.shape[1])], free[b, : min(f + 1, got.shape[1])])   # up to and including EOS
        assert (got[b, f + 1:] == pad).all()                    # padded from the next step on; the other rows run on
    # every row finished: the poll ends the loop early, no later than eos_poll steps after the last row finished
    one = lm.generate(tok[:1], n, eos_token_id=eos, pad_token_id=pad, eos_poll=4).cpu()
    assert one.shape[1] < n and one.shape[1] <= first[0] + 1 + 4
    assert torch.equal(one[0, : first[0] + 1], free[0, : first[0] + 1]) and (one[0, first[0] + 1:] == pad).all()
    # without a poll the loop runs to the end, with the same tokens
    nopoll = lm.generate(tok[:1], n, eos_token_id=eos, pad_token_id=pad, eos_poll=0).cpu()
    assert nopoll.shape[1] == n and torch.equal(nopoll[:, : one.shape[1]], one)


def test_limits():
    lm = _lm(seed=9).to("cuda")
    tok = torch.randint(0, 502, (2, 9), generator=torch.Generator().manual_seed(7)).cuda()
    with pytest.raises(IndexError, match="index out of range in self"):
        lm.generate(tok, 62 - 9 + 1)                            # 62 usable positions in a 64-row table
    assert lm.generate(tok, 62 - 9).shape == (2, 53)
    lm.precision = "bf16x3"
    with pytest.raises(ValueError, match="no KV-cache kernels"):
        lm.generate(tok, 4)
    lm.precision = "fp32"
    bad = tok.clone()
    bad[1, 2] = 502
    with pytest.raises(IndexError, match="index out of range"):
        lm.generate(bad, 4)                                     # the prompt is still range-checked, once
    m = Kosmos._from_config(tiny_config(), seed=0).eval().to("cuda")
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image).cuda()
    with pytest.raises(IndexError, match="index out of range in self"):
        m.generate(torch.zeros(2, 10, dtype=torch.long).cuda(), img, 62 - 18 + 1)


def test_full_size_language_model_sampled():
    lm = KosmosLanguage(vocab_size=32002, _seed=0).eval().to("cuda")
    lm.precision = "mixed"
    tok = torch.randint(0, 32002, (4, 9), generator=torch.Generator().manual_seed(8)).cuda()
    kw = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=5)
    got, logits = lm.generate(tok, 16, output_logits=True, **kw)
    assert got.shape == (4, 16) and logits.shape == (4, 16, 32002) and bool(torch.isfinite(logits).all())
    assert int(got.min()) >= 0 and int(got.max()) < 32002
    assert torch.equal(lm.generate(tok, 16, **kw), got)
    _sampler_parity(got, logits, tok, 9, kw)
