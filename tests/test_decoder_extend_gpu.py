"""Chunked prefill: kx_decoder_extend under KosmosLanguage.extend() and under generate() / score(prefill_chunk=...).

The model of tests/test_incremental.py (vocab 502, dim 256, depth 2, ffn 512, 4 heads, _perturb = 0.1) with a 324-row position
table, so that 300-token sequences cross the attention kernels' 128-query block; the reference is the CPU oracle's full forward
(O.kosmos_language_forward / O.kosmos_forward), the tolerances that file's: fp32 2e-4, bf16 6e-2, f16c and mixed 1e-3."""
import pytest
import torch

from helpers import oracle_cfg, oracle_switches, oracle_weights, rel_err, tiny_config
from kosmosx.config import Switches
from kosmosx.model import Kosmos, KosmosLanguage
from oracle import kosmos_oracle as O

pytestmark = pytest.mark.gpu

CFG = O.DecoderCfg(layers=2, dim=256, ffn=512, heads=4, vocab=502, max_pos=324)
TOL = {"fp32": 2e-4, "bf16": 6e-2, "f16c": 1e-3, "mixed": 1e-3}
LP_BOUND = 2e-5                                            # tests/test_score_gpu.py: absolute, on the log-probs
SEED, TG, NG = 8, 150, 6                                   # the generate tests' prompt seed (gap / bound = 23 on the CPU oracle; seeds 1 and 6: 2.4, 1.5), prompt length, new tokens


def _lm(seed=6):
    return KosmosLanguage(vocab_size=502, dim=256, depth=2, ffn_dim=512, decoder_heads=4, _seed=seed, _perturb=0.1,
                          _max_positions=324).eval()


@pytest.fixture(scope="module")
def long_ref():
    """(tokens [3, 300], the oracle's logits [3, 300, V]): computed once, shared, never written."""
    tok = torch.randint(0, 502, (3, 300), generator=torch.Generator().manual_seed(2))
    return tok, O.kosmos_language_forward(oracle_weights(_lm()), tok, CFG)


@pytest.mark.parametrize("prec", list(TOL))
def test_prefill_extends_then_steps_match_the_full_forward(prec, long_ref):
    tok, ref = long_ref
    tol = TOL[prec]
    lm = _lm().to("cuda")
    lm.precision = prec
    tokd = tok.cuda()
    state = {}
    out = lm(tokd[:, :9], incremental_state=state)
    assert rel_err(out, ref[:, :9]) < tol and state["len"] == 9
    t, worst = 9, 0.0
    for n in (1, 54, 130, 97):
        out = lm.extend(tokd[:, t:t + n], state)
        assert out.shape == (3, n, 502) and out.dtype == torch.float32
        e = rel_err(out, ref[:, t:t + n])
        worst = max(worst, e)
        assert e < tol, (t, n, e)
        t += n
        assert state["len"] == t
    for _ in range(5):
        step = lm(tokd[:, :t + 1], incremental_state=state)
        e = rel_err(step, ref[:, t:t + 1])
        worst = max(worst, e)
        assert step.shape == (3, 1, 502) and e < tol, (t, e)
        t += 1
        assert state["len"] == t
    # the caches against a one-piece prefill of the same 296 tokens with the same XPos centring (keys are stored rotated and scaled)
    one = {"max_len": state["max_len"], "xpos_centre": 9}
    lm(tokd[:, :t], incremental_state=one)
    ek = rel_err(state["kcache"][:, :, :, :t], one["kcache"][:, :, :, :t])
    ev = rel_err(state["vcache"][:, :, :, :t], one["vcache"][:, :, :, :t])
    print(f"extend ({prec}): worst logits rel_err {worst:.3e}, caches vs one-piece prefill k {ek:.3e} v {ev:.3e} (tol {tol:.0e})")
    assert ek < tol and ev < tol


def test_extend_without_logits_on_an_empty_state_and_the_refusals(long_ref):
    tok, ref = long_ref
    lm = _lm().to("cuda")
    lm.precision = "fp32"
    tokd = tok.cuda()
    state = {}
    out = lm.extend(tokd[:, :40], state)                                     # an empty state: the prefill
    assert state["len"] == 40 and rel_err(out, ref[:, :40]) < 2e-4
    assert lm.extend(tokd[:, 40:75], state, output_logits=False) is None and state["len"] == 75
    assert rel_err(lm.extend(tokd[:, 75:140], state), ref[:, 75:140]) < 2e-4 and state["len"] == 140
    # past max_len / the position table: IndexError with the step's text, the state where it was
    with pytest.raises(IndexError, match="exceeds the table / cache"):
        lm.extend(torch.cat([tokd, tokd], 1)[:, :200], state)                # 140 + 200 > 322
    assert state["len"] == 140
    short = {"max_len": 50}
    lm.extend(tokd[:, :40], short)
    with pytest.raises(IndexError, match="exceeds the table / cache"):
        lm.extend(tokd[:, 40:51], short)
    assert short["len"] == 40
    assert rel_err(lm.extend(tokd[:, 40:50], short), ref[:, 40:50]) < 2e-4 and short["len"] == 50
    # an id outside the vocabulary
    bad = tokd[:, 140:150].clone()
    bad[1, 3] = 502
    with pytest.raises(IndexError):
        lm.extend(bad, state)
    assert state["len"] == 140
    # another batch size
    with pytest.raises(ValueError, match="batch size"):
        lm.extend(tokd[:2, 140:150], state)
    assert state["len"] == 140
    assert rel_err(lm.extend(tokd[:, 140:150], state), ref[:, 140:150]) < 2e-4 and state["len"] == 150
    # a ragged state
    ragged = dict(state, positions=torch.full((3,), 150, dtype=torch.int32, device="cuda"), pos_max=150)
    with pytest.raises(ValueError, match="ragged incremental state"):
        lm.extend(tokd[:, 150:160], ragged)
    assert ragged["len"] == 150
    step = lm(tokd[:, :151], incremental_state=state)                        # single-token steps continue as before
    assert rel_err(step, ref[:, 150:151]) < 2e-4 and state["len"] == 151


def _count_extends(lm):
    """Record (rows, output_logits) of every Decoder._extend call of ``lm``: the slices a chunked prefill really ran."""
    calls, inner = [], lm.decoder._extend

    def spy(x, state, prec, output_logits=True, tokens=None):
        calls.append(((tokens if x is None else x).shape[1], bool(output_logits)))
        return inner(x, state, prec, output_logits, tokens=tokens)
    lm.decoder._extend = spy
    return calls


@pytest.fixture(scope="module")
def gen_ref():
    """The unchunked fp32 generate() of the module's prompt, once: (prompt, tokens, logits)."""
    lm = _lm().to("cuda")
    lm.precision = "fp32"
    tok = torch.randint(0, 502, (3, TG), generator=torch.Generator().manual_seed(SEED))
    got, logits = lm.generate(tok.cuda(), NG, output_logits=True)
    return tok, got.cpu(), logits.cpu()


def test_the_prompt_seed_leaves_a_wide_top_two_gap(gen_ref):
    """Token equality between the chunked and the one-piece prefill is only asserted because no pick is close: the smallest
    top-two logit gap of the unchunked run exceeds 10 x the fp32 tolerance x the logits' rms.  A property of SEED (chosen on the
    CPU oracle, where the ratio is printed by the same formula), not of the model."""
    _, _, logits = gen_ref
    top = logits.topk(2, -1).values
    gap, rms = float((top[..., 0] - top[..., 1]).min()), float(logits.pow(2).mean().sqrt())
    print(f"smallest top-two gap {gap:.3e}, 10 x tol x rms = {10 * 2e-4 * rms:.3e}")
    assert gap > 10 * 2e-4 * rms


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
@pytest.mark.parametrize("chunk", [1, 7, 64, TG, TG + 5])
def test_generate_with_a_chunked_prefill(chunk, prec, gen_ref):
    tok, want, want_logits = gen_ref
    lm0 = _lm()
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    calls = _count_extends(lm)
    got, logits = lm.generate(tok.cuda(), NG, output_logits=True, prefill_chunk=chunk)
    assert got.shape == (3, NG) and logits.shape == (3, NG, 502)
    assert calls == [(min(chunk, TG - s), s > TG - 1 - chunk) for s in range(chunk, TG, chunk)]   # (rows, logits asked for) per slice
    if prec == "fp32":
        print(f"generate(prefill_chunk={chunk}) logits vs the one-piece prefill's: {float((logits.cpu() - want_logits).abs().max()):.3e}")
    ref = O.kosmos_language_forward(w, torch.cat([tok, got.cpu()[:, :-1]], 1), CFG)[:, TG - 1:]
    e = rel_err(logits, ref)
    print(f"generate(prefill_chunk={chunk}) logits vs oracle ({prec}): {e:.3e}")
    assert e < TOL[prec]
    if prec == "fp32":
        assert torch.equal(got.cpu(), want)                                  # (test_the_prompt_seed_leaves_a_wide_top_two_gap)
    assert torch.equal(lm.generate(tok.cuda(), NG, prefill_chunk=chunk), got)


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_generate_ragged_prompts_whose_last_positions_fall_in_different_chunks(prec):
    lm0 = _lm()
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = prec
    tok = torch.randint(0, 502, (3, TG), generator=torch.Generator().manual_seed(SEED))
    lens = [TG, 70, 9]                                                       # chunks of 64: slices 2, 1 and 0
    got, logits = lm.generate(tok.cuda(), NG, output_logits=True, prompt_lengths=lens, prefill_chunk=64, seed=3,
                              do_sample=True, top_k=20)
    for b, n in enumerate(lens):
        full = torch.cat([tok[b, :n], got[b, :-1].cpu()])[None]
        e = rel_err(logits[b], O.kosmos_language_forward(w, full, CFG)[0, n - 1:])
        assert e < TOL[prec], (b, e)


def test_chunked_prefill_under_lookup_beams_and_constraints(gen_ref):
    """The other loops take the gathered [B, 1, V] rows and ``prompt_rows`` = T: a loop that still read T off the logits' shape
    would place its tokens at position 1.  fp32, the seed whose top-two gap is asserted above.  Prompt lookup is greedy decoding:
    its tokens are the plain loop's, its logits the oracle's.  Beams: the tokens and scores of the one-piece run, and the best
    hypothesis' score against the oracle's log-probs — bound 2 x tol x rms (the logit and the log-sum-exp each move by at most
    tol x rms, the score is their mean over the tokens).  Constraints on ragged prompts: the returned (unbanned) logits against
    the oracle."""
    tok, want, want_logits = gen_ref
    lm0 = _lm()
    w = oracle_weights(lm0)
    lm = lm0.to("cuda")
    lm.precision = "fp32"
    tokd = tok.cuda()
    bound = 2 * TOL["fp32"] * float(want_logits.pow(2).mean().sqrt())
    look, rows = lm.generate(tokd, NG, prompt_lookup_num_tokens=3, prefill_chunk=64, output_logits=True)
    assert torch.equal(look.cpu(), want)
    ref = O.kosmos_language_forward(w, torch.cat([tok, want[:, :-1]], 1), CFG)[:, TG - 1:]
    assert rel_err(rows, ref) < TOL["fp32"]
    n = 4
    one, one_scores = lm.generate(tokd, n, num_beams=3, num_return_sequences=3, output_scores=True)
    beams, scores = lm.generate(tokd, n, num_beams=3, num_return_sequences=3, output_scores=True, prefill_chunk=64)
    assert beams.shape == (3, 3, n) and torch.equal(beams, one)
    assert float((scores - one_scores).abs().max()) < bound
    best = beams[:, 0].cpu()
    lp = torch.log_softmax(O.kosmos_language_forward(w, torch.cat([tok, best[:, :-1]], 1), CFG)[:, TG - 1:].double(), -1)
    ref_score = lp.gather(2, best[:, :, None])[:, :, 0].sum(1) / n
    e = float((scores[:, 0].cpu().double() - ref_score).abs().max())
    print(f"beam scores with prefill_chunk=64 vs the oracle's log-probs: {e:.3e} (bound {bound:.3e})")
    assert e < bound
    lens = [TG, 70, 9]
    got, logits = lm.generate(tokd, NG, prompt_lengths=lens, prefill_chunk=64, no_repeat_ngram_size=2, min_new_tokens=3,
                              eos_token_id=5, output_logits=True)
    for b, m in enumerate(lens):
        full = torch.cat([tok[b, :m], got[b, :-1].cpu()])[None]
        assert rel_err(logits[b], O.kosmos_language_forward(w, full, CFG)[0, m - 1:]) < TOL["fp32"], b
        assert 5 not in got[b, :3].tolist()                                  # min_new_tokens


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
@pytest.mark.parametrize("alias", [True, False])
def test_kosmos_generate_with_chunk_boundaries_inside_and_just_after_the_image_rows(prec, alias):
    """tiny_config: 8 image rows spliced after two tokens (rows 2 .. 9).  prefill_chunk = 5: boundaries at 5 (inside the image
    rows) and 10 (just after them); 3: 3, 6 and 9 inside."""
    sw = Switches(u1_inplace_alias=alias)
    m0 = Kosmos._from_config(tiny_config(), seed=1, switches=sw, perturb=0.1).eval()
    w, cfg = oracle_weights(m0), oracle_cfg(m0.cfg)
    m = m0.to("cuda")
    m.precision = prec
    g = torch.Generator().manual_seed(5)
    Tt, n = 10, 8
    tok = torch.randint(0, m.cfg.vocab, (2, Tt), generator=g)
    img = torch.randn(2, 3, m.cfg.vit.image, m.cfg.vit.image, generator=g)
    n_img = m.cfg.perceiver.latents
    assert n_img == 8
    for chunk in (5, 3):
        got, logits = m.generate(tok.cuda(), img.cuda(), n, output_logits=True, prefill_chunk=chunk)
        text = torch.cat([tok, got.cpu()[:, :-1]], 1)
        ref = O.kosmos_forward(w, text, img, cfg, oracle_switches(sw))[:, Tt + n_img - 1:]
        e = rel_err(logits, ref)
        print(f"Kosmos.generate(prefill_chunk={chunk}) logits vs oracle ({prec}, alias={alias}): {e:.3e}")
        assert e < TOL[prec]


def test_score_with_a_chunked_prefill_matches_score_without():
    lm = _lm().to("cuda")
    lm.precision = "fp32"
    g = torch.Generator().manual_seed(4)
    tok = torch.randint(0, 502, (2, 100), generator=g).cuda()
    cont = torch.randint(0, 502, (6, 4), generator=g).cuda()
    lens = [4, 1, 3, 2, 4, 2]
    calls = _count_extends(lm)
    for plens in (None, [100, 37]):
        want = lm.score(tok, cont, continuation_lengths=lens, prompt_lengths=plens)
        assert not calls
        for chunk in (1, 33, 64, 100, 105):
            lp = lm.score(tok, cont, continuation_lengths=lens, prompt_lengths=plens, prefill_chunk=chunk)
            assert len(calls) == (100 - 1) // chunk                          # the slices after the first
            del calls[:]
            e = float((lp.double() - want.double()).abs().max())
            print(f"score(prefill_chunk={chunk}, prompt_lengths={plens}) vs score(): {e:.3e} (bound {LP_BOUND:.0e})")
            assert lp.shape == want.shape and e <= LP_BOUND
